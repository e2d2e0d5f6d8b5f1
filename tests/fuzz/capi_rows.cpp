// Stand-alone driver (its own main, no fuzzer) for the layer of capi.hip that both fields share: it walks the host rows of
// tests/test_capi_messages.py - bad, edge and good calls of hg_verify_public*, hg_claims_settle*, hg_instance_mle*, the batches without
// a context, and hg_pcs_open* .. hg_claims_verify* on host commitments - and checks the return codes. Meant to be built with
// -fsanitize=address,undefined and linked against a library whose host code has the same sanitizers, so that they watch the shared
// routines read and write the caller's blocks:
//   bash scripts/build_variant.sh asan "-fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer -g -shared-libsan"
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -shared-libsan tests/fuzz/capi_rows.cpp -o build/fuzz/capi_rows \
//       -Lbuild/asan -lhypergreco -Wl,-rpath,$PWD/build/asan -Wl,-rpath,<directory of libclang_rt.asan-x86_64.so>
//   ASAN_OPTIONS=detect_leaks=0:verify_asan_link_order=0:detect_odr_violation=0 UBSAN_OPTIONS=halt_on_error=1 ./build/fuzz/capi_rows
// (the program links the sanitizer's runtime itself, as fuzz_pcs.cpp does). Host only, no context anywhere. Exit code 0: every row
// gave the expected code.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/hg.h"

static int failures = 0, rows = 0;
static void expect(int rc, int want, const char* what) {
    rows++;
    if (rc == want) return;
    failures++;
    fprintf(stderr, "%s: returned %d, expected %d (%s)\n", what, rc, want, hg_last_error());
}

static const uint64_t GL_P = 0xFFFFFFFF00000001ull;
static const uint64_t FR_R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

// one field's rows; W words per element, claims of type Claim
template <class Claim, int W>
static void field_rows(bool bn, const hg_params& pr, const hg_pk* pk, const hg_witness* w, const hg_witness* w_other, const void* inst, const void* inst_other) {
    size_t nc = 0, nco = 0;
    expect(hg_pk_claim_shape(pk, &nc, &nco), 0, "hg_pk_claim_shape");
    std::vector<Claim> claims(nc);
    std::vector<uint64_t> points(W * nco);
    size_t got = 0;
    std::vector<uint8_t> junk(4096);
    for (size_t i = 0; i < junk.size(); i++) junk[i] = (uint8_t)i;
    auto vpub = [&](const hg_pk* k, const void* in, const uint8_t* proof, void* cl, size_t ccap, uint64_t* pts, size_t pcap, size_t* n) {
        return bn ? hg_verify_public_bn254(k, in, proof, junk.size(), cl, ccap, pts, pcap, n) : hg_verify_public(k, in, 0, proof, junk.size(), cl, ccap, pts, pcap, n);
    };
    expect(vpub(pk, inst, junk.data(), claims.data(), nc, points.data(), nco, &got), 1, "verify_public: a proof that is not one");
    expect(vpub(nullptr, inst, junk.data(), claims.data(), nc, points.data(), nco, &got), -1, "verify_public: null key");
    expect(vpub(pk, inst, junk.data(), claims.data(), nc, points.data(), nco, nullptr), -1, "verify_public: null n_claims");
    expect(vpub(pk, inst_other, junk.data(), claims.data(), nc, points.data(), nco, &got), -1, "verify_public: other parameters");
    expect(vpub(pk, inst, junk.data(), claims.data(), nc - 1, points.data(), nco, &got), -1, "verify_public: claim capacity");
    expect(vpub(pk, inst, junk.data(), claims.data(), nc, nullptr, nco, &got), -1, "verify_public: null points");
    // the batches and the device forms without a context
    const void* insts[2] = {inst, inst};
    const hg_witness* ws[2] = {w, w};
    const uint8_t* proofs[2] = {junk.data(), junk.data()};
    size_t lens[2] = {junk.size(), junk.size()}, counts[2] = {0, 0};
    int res[2] = {7, 7};
    char reasons[16];
    expect(bn ? hg_verify_device_batch_bn254(nullptr, pk, ws, proofs, lens, 2, res, reasons, 8) : hg_verify_device_batch(nullptr, pk, ws, proofs, lens, 2, 0, res, reasons, 8), -1,
           "verify_device_batch: no context");
    std::vector<Claim> claims2(2 * nc);
    std::vector<uint64_t> points2(2 * W * nco);
    expect(bn ? hg_verify_public_batch_bn254(nullptr, pk, insts, proofs, lens, 2, res, claims2.data(), nc, points2.data(), nco, counts, reasons, 8)
              : hg_verify_public_batch(nullptr, pk, insts, proofs, lens, 2, 0, res, claims2.data(), nc, points2.data(), nco, counts, reasons, 8), -1, "verify_public_batch: no context");
    // hg_instance_mle*
    const size_t nv = 11;
    std::vector<uint64_t> pt(W * nv, 0), out(2 * W, 0);
    for (size_t j = 0; j < nv; j++) pt[W * j] = 5 + j;
    auto mle = [&](const void* in, int which, int index, const uint64_t* p, size_t n, uint64_t* o) {
        return bn ? hg_instance_mle_bn254(nullptr, in, which, index, p, n, o) : hg_instance_mle(nullptr, in, which, index, p, n, o);
    };
    expect(mle(inst, 0, 0, pt.data(), nv, out.data()), 0, "instance_mle: ais[0]");
    expect(mle(inst, 1, 0, pt.data(), nv, out.data()), 0, "instance_mle: ct0is");
    expect(mle(nullptr, 0, 0, pt.data(), nv, out.data()), -1, "instance_mle: null instance");
    expect(mle(inst, 2, 0, pt.data(), nv, out.data()), -1, "instance_mle: selector");
    expect(mle(inst, 0, 1, pt.data(), nv, out.data()), -1, "instance_mle: modulus index");
    expect(mle(inst, 0, 0, pt.data(), nv - 1, out.data()), -1, "instance_mle: variables");
    std::vector<uint64_t> bad = pt;
    if constexpr (W == 4) memcpy(&bad[W * (nv - 1)], FR_R, 32); else bad[W * (nv - 1)] = GL_P;
    expect(mle(inst, 0, 0, bad.data(), nv, out.data()), -1, "instance_mle: non-canonical coordinate");
    expect(bn ? hg_instance_mle_batch_bn254(nullptr, insts, 2, 0, 0, pt.data(), nv, out.data()) : hg_instance_mle_batch(nullptr, insts, 2, 0, 0, pt.data(), nv, out.data()), -1,
           "instance_mle_batch: no context");
    // hg_claims_settle*: input 0 (s) at the all-zero point is word 0 of the table
    uint64_t s0 = 0;
    hg_witness_get(w, 0, &s0, 1);
    Claim c;
    memset(&c, 0, sizeof(c));
    c.input = 0; c.nvars = (uint32_t)nv; c.point_off = 0;
    if (bn && s0 > GL_P / 2) {   // the signed lift: r - (p - s0)
        unsigned __int128 borrow = 0;
        const uint64_t m = GL_P - s0;
        for (int i = 0; i < W; i++) {
            const unsigned __int128 d = (unsigned __int128)FR_R[i] - (i == 0 ? m : 0) - borrow;
            c.value[i] = (uint64_t)d;
            borrow = (d >> 64) ? 1 : 0;
        }
    } else {
        c.value[0] = s0;
    }
    std::vector<uint64_t> zero(W * 41, 0);
    auto settle = [&](const hg_witness* wi, const Claim* cl, size_t n, const uint64_t* p) {
        return bn ? hg_claims_settle_bn254(nullptr, &pr, wi, cl, n, p) : hg_claims_settle(nullptr, &pr, wi, cl, n, p);
    };
    expect(settle(w, &c, 1, zero.data()), 0, "claims_settle: a claim that holds");
    expect(settle(w, nullptr, 0, nullptr), 0, "claims_settle: no claims");
    expect(settle(w_other, &c, 1, zero.data()), -1, "claims_settle: other parameters");
    Claim d = c;
    memset(d.value, 0, sizeof(d.value));
    d.value[0] = 12345;
    expect(settle(w, &d, 1, zero.data()), 1, "claims_settle: another value");
    d = c; d.input = 6;
    expect(settle(w, &d, 1, zero.data()), -1, "claims_settle: input id");
    d = c; d.nvars = 41;
    expect(settle(w, &d, 1, zero.data()), -1, "claims_settle: 41 coordinates");
    expect(settle(w, &c, 1, bad.data()), -1, "claims_settle: non-canonical coordinate");
    d = c;
    if constexpr (W == 4) memcpy(d.value, FR_R, 32); else d.value[0] = GL_P;
    expect(settle(w, &d, 1, zero.data()), -1, "claims_settle: non-canonical value");
    // hg_secrets_commit*, hg_claims_open*, hg_claims_verify*
    void* cm = nullptr;
    uint8_t root[32];
    auto commit = [&](const hg_witness* wi, size_t log2_row, void** h) { return bn ? hg_secrets_commit_bn254(nullptr, &pr, wi, log2_row, h, root) : hg_secrets_commit(nullptr, &pr, wi, log2_row, h, root); };
    expect(commit(w_other, 0, &cm), -1, "secrets_commit: other parameters");
    expect(commit(w, 11, &cm), -1, "secrets_commit: log2_row");
    expect(commit(w, 0, &cm), 0, "secrets_commit");
    std::vector<uint8_t> opening(1 << 17);
    size_t olen = 0;
    auto copen = [&](const void* h, const Claim* cl, size_t n, const uint64_t* p, size_t nq, size_t cap) {
        return bn ? hg_claims_open_bn254(nullptr, &pr, h, cl, n, p, nq, opening.data(), cap, &olen) : hg_claims_open(nullptr, &pr, h, cl, n, p, nq, opening.data(), cap, &olen);
    };
    auto cverify = [&](const Claim* cl, size_t n, const uint64_t* p, size_t nq, size_t len) {
        return bn ? hg_claims_verify_bn254(&pr, root, 0, cl, n, p, nq, opening.data(), len) : hg_claims_verify(&pr, root, 0, cl, n, p, nq, opening.data(), len);
    };
    d = c; d.input = 3;
    expect(copen(cm, &d, 1, zero.data(), 3, opening.size()), -1, "claims_open: a public input");
    d = c; d.nvars = 10;
    expect(copen(cm, &d, 1, zero.data(), 3, opening.size()), -1, "claims_open: coordinates");
    expect(copen(cm, &c, 1, bad.data(), 3, opening.size()), -1, "claims_open: non-canonical coordinate");
    expect(copen(cm, &c, 1, zero.data(), 65537, opening.size()), -1, "claims_open: queries");
    expect(copen(cm, &c, 1, zero.data(), 3, 64), -1, "claims_open: buffer too small");
    expect(copen(cm, &c, 1, zero.data(), 3, opening.size()), 0, "claims_open");
    expect(cverify(&c, 1, zero.data(), 3, olen), 0, "claims_verify");
    expect(cverify(&c, 1, zero.data(), 3, olen - 1), 1, "claims_verify: a byte short");
    opening[40] ^= 1;
    expect(cverify(&c, 1, zero.data(), 3, olen), 1, "claims_verify: tampered");
    expect(cverify(&c, 1, bad.data(), 3, olen), -1, "claims_verify: non-canonical coordinate");
    // hg_pcs_open*, hg_pcs_verify*: the handle of the secrets as a commitment to caller tables; its first table is s
    const uint32_t nvars[5] = {11, 11, 11, 11, 10};
    uint32_t table[2] = {0, 5};
    std::vector<uint64_t> vals(2 * W, 0);
    memcpy(vals.data(), c.value, 8 * W);
    auto popen = [&](const void* h, size_t n, const uint64_t* p, const uint64_t* v) {
        return bn ? hg_pcs_open_bn254(nullptr, h, table, p, v, n, 3, opening.data(), opening.size(), &olen) : hg_pcs_open(nullptr, h, table, p, v, n, 3, opening.data(), opening.size(), &olen);
    };
    auto pverify = [&](size_t n, const uint64_t* p, const uint64_t* v, size_t len) {
        return bn ? hg_pcs_verify_bn254(root, nvars, 5, 0, table, p, v, n, 3, opening.data(), len) : hg_pcs_verify(root, nvars, 5, 0, table, p, v, n, 3, opening.data(), len);
    };
    expect(popen(cm, 2, zero.data(), vals.data()), -1, "pcs_open: table index");
    expect(popen(cm, 1, bad.data(), vals.data()), -1, "pcs_open: non-canonical coordinate");
    expect(popen(cm, 1, zero.data(), bad.data() + W * (nv - 1)), -1, "pcs_open: non-canonical value");
    expect(popen(nullptr, 1, zero.data(), vals.data()), -1, "pcs_open: null commitment");
    expect(popen(cm, 1, zero.data(), vals.data()), 0, "pcs_open");
    expect(pverify(1, zero.data(), vals.data(), olen), 0, "pcs_verify");
    expect(pverify(2, zero.data(), vals.data(), olen), -1, "pcs_verify: table index");
    expect(pverify(1, zero.data(), vals.data(), olen - 8), 1, "pcs_verify: short");
    expect(pverify(0, nullptr, nullptr, olen), 1, "pcs_verify: no claims against an opening of one");
    hg_pcs_free(cm);
    // the other field's handle
    void* other = nullptr;
    expect(bn ? hg_secrets_commit(nullptr, &pr, w, 0, &other, root) : hg_secrets_commit_bn254(nullptr, &pr, w, 0, &other, root), 0, "secrets_commit of the other field");
    expect(copen(other, &c, 1, zero.data(), 3, opening.size()), -1, "claims_open: the other field's commitment");
    expect(popen(other, 1, zero.data(), vals.data()), -1, "pcs_open: the other field's commitment");
    hg_pcs_free(other);
}

int main() {
    hg_params pr, pr_other;
    expect(hg_params_builtin(1024, 1, &pr), 0, "hg_params_builtin");
    expect(hg_params_builtin(2048, 1, &pr_other), 0, "hg_params_builtin");
    hg_pk* pk = nullptr;
    expect(hg_setup(nullptr, &pr, &pk), 0, "hg_setup (host only)");
    hg_witness *w = nullptr, *w_other = nullptr;
    expect(hg_witness_synthetic(&pr, 0xca91, &w), 0, "hg_witness_synthetic");
    expect(hg_witness_synthetic(&pr_other, 0xca92, &w_other), 0, "hg_witness_synthetic");
    void *inst = nullptr, *inst_other = nullptr;
    expect(hg_instance_from_witness(&pr, w, &inst), 0, "hg_instance_from_witness");
    expect(hg_instance_from_witness(&pr_other, w_other, &inst_other), 0, "hg_instance_from_witness");
    if (failures) return 2;
    field_rows<hg_input_claim, 2>(false, pr, pk, w, w_other, inst, inst_other);
    field_rows<hg_input_claim_bn254, 4>(true, pr, pk, w, w_other, inst, inst_other);
    const int64_t* none[1] = {nullptr};
    expect(hg_prove_encryptions(nullptr, pk, none, none, none, none, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr), -1, "hg_prove_encryptions: no context");
    expect(hg_prove_encryptions_bn254(nullptr, pk, none, none, none, none, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr), -1, "hg_prove_encryptions_bn254: no context");
    hg_instance_free(inst); hg_instance_free(inst_other);
    hg_witness_free(w); hg_witness_free(w_other);
    hg_pk_free(pk);
    printf("capi_rows: %d rows, %d failures\n", rows, failures);
    return failures ? 1 : 0;
}
