// C ABI (include/hg.h). No exception crosses the boundary: every entry point catches, stores the
// message for hg_last_error() and returns a negative status.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include "prover.hpp"
#include "pcs.hpp"
#include "pcs_bn254.hpp"

// BN254 slice (bn254.hip)
namespace hg { namespace bn {
void sumcheck_bn254(hg_ctx* ctx, int kind, size_t nv, size_t ntab, const u64* const* tables, const u64* pw4, size_t npw, const u64* claim4,
                    size_t chain_skip, u64* msgs, u64* point, u64* evals, u64* sums);
void prodsum_jobs_bn254(hg_ctx* ctx, size_t njobs, const size_t* nv, const size_t* npairs, const u64* const* tables, const size_t* win, size_t chain_skip,
                        u64* sums4, u64* evals4);
void field_op_bn254(hg_ctx* ctx, int op, size_t n, const u64* a, const u64* b, u64* out);
void challenges_bn254_raw(size_t n, uint64_t* out4);
void mle_eval_bn254(hg_ctx* ctx, const u64* table4, size_t nv, const u64* point4, u64* out4);
void ntt_bn254(hg_ctx* ctx, const u64* in4, size_t log2n, bool inverse, size_t batch, u64* out4);
void grand_product_bn254(hg_ctx* ctx, size_t nb, size_t len, const u64* const* tables, size_t chain_skip, std::vector<uint8_t>& proof,
                         u64* claims_out, u64* point_out);
void lasso_prove_bn254(hg_ctx* ctx, const hg_pk* pk, const u64* in4, size_t chain_skip, std::vector<uint8_t>& proof, u64* claim_out);
void circuit_eval_bn254(hg_ctx* ctx, const hg_pk* pk, const Witness& w, int which, std::vector<u64>& out4);
void prove_bn254(hg_ctx* ctx, const hg_pk* pk, const Witness& w, std::vector<uint8_t>& proof, double* ms);
} }
using namespace hg;

static thread_local std::string g_last_error;

#define HG_TRY try {
#define HG_CATCH(ret)                                                           \
    }                                                                           \
    catch (const std::exception& ex) { g_last_error = ex.what(); return ret; } \
    catch (...) { g_last_error = "unknown error"; return ret; }
#define HG_ENTRY(...) HG_TRY return __VA_ARGS__; HG_CATCH(-1)   // an entry that is one call of a routine of the shared layer

// (called from the worker threads of hg_setup's node loop: the current device is per thread, the key's list of allocations is shared.
// ONE lock for every element type: a static inside the template would be one mutex per instantiation, and the u32, u64 and
// GatherSeg uploads of different threads would push onto pk->owned at the same time)
static std::mutex g_upload_mu;
template <typename T>
static const T* upload_vec(hg_pk* pk, const std::vector<T>& v) {
    if (!pk->ctx) return nullptr;  // host-only key (hg_setup(NULL, ..)): wiring without a device copy
    std::lock_guard<std::mutex> lock(g_upload_mu);
    hip_check(hipSetDevice(pk->ctx->device), "hipSetDevice");
    T* d = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    hip_check(hipMalloc((void**)&d, bytes), "hipMalloc(prover key)");
    if (!v.empty()) hip_check(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "upload prover key");
    pk->owned.push_back(d);
    return d;
}

// counting-sort a term list into a CSR keyed by position `key(t)` in [0, S)
template <typename Term, typename KeyFn, typename EmitFn>
static void build_csr(const std::vector<const Term*>& terms, size_t S, KeyFn key, std::vector<u32>& ptr, EmitFn emit) {
    ptr.assign(S + 1, 0);
    for (const Term* t : terms) ptr[key(*t) + 1]++;
    for (size_t i = 0; i < S; i++) ptr[i + 1] += ptr[i];
    std::vector<u32> fill(ptr.begin(), ptr.end() - 1);
    for (const Term* t : terms) emit(*t, fill[key(*t)]++);
}

// A witness handle must have been built for the prover key's parameter set: the provers and verifiers index its
// tables with sizes taken from the key (k * 2^L, k * 2^P ...), so a mismatch would read out of bounds.
static void check_witness(const hg_pk* pk, const hg_witness* w, const char* who) {
    const hg_params& a = pk->params.raw;
    const hg_params& b = w->params;
    if (a.n != b.n || a.k != b.k) throw Error(std::string(who) + ": witness was built for n=" + std::to_string(b.n) + " k=" + std::to_string(b.k) + ", the prover key for n=" + std::to_string(a.n) + " k=" + std::to_string(a.k));
    const size_t SZ = pk->params.SZ(), PZ = pk->params.PZ(), k = (size_t)pk->params.k;
    const Witness& v = w->w;
    if (v.s.size() != SZ || v.e.size() != SZ || v.k1.size() != SZ || v.ais.size() != k * SZ || v.r1is.size() != k * SZ || v.r2is.size() != k * PZ ||
        v.ct0is.size() != k * SZ)
        throw Error(std::string(who) + ": witness table sizes do not match the parameter set");
}

static const hg_instance* as_instance(const void* h) { return static_cast<const hg_instance*>(h); }

// the instance must have been built for the key's parameter set: the walk indexes its coefficients with sizes taken from the key
static void check_instance(const hg_pk* pk, const hg_instance* in, const char* who) {
    const hg_params& a = pk->params.raw;
    const hg_params& b = in->params;
    const size_t kn = (size_t)a.k * a.n;
    if (a.n != b.n || a.k != b.k || memcmp(a.qis, b.qis, sizeof(a.qis[0]) * a.k) != 0 || in->inst.a.size() != kn || in->inst.ct0.size() != kn)
        throw Error(std::string(who) + ": the instance was built for other parameters than the key (n=" + std::to_string(b.n) + " k=" + std::to_string(b.k) + " against n=" +
                    std::to_string(a.n) + " k=" + std::to_string(a.k) + ", or other moduli)");
}

// ---- the layer both fields share -------------------------------------------------------------------------------------------------
// Every entry point that exists over Goldilocks and over bn256::Fr (`_bn254`) checks its arguments, converts claims, writes results
// and reasons in the routines below, once. What they need to know of a field is how an element crosses the ABI and which walk,
// evaluator or commitment scheme to call: GlAbi (an Ext2 element, 2 words, canonical when both are below GL_P) and BnAbi (an Fr
// element, 4 little-endian words, canonical when below r). The checks, their order and their messages are part of the interface
// (tests/test_capi_messages.py pins them): where two siblings differ, the difference is a parameter here, marked "historical".
// An entry without protocol modes passes mode 0.
namespace {   // (internal linkage: the library exports nothing but the C ABI)
struct GlAbi {
    static constexpr size_t WORDS = 2;
    static constexpr pcs::Field FIELD = pcs::GOLDILOCKS;
    typedef OpenClaim Open;
    typedef hg_input_claim Wire;
    typedef pcs::Claim PcsClaim;
    typedef pcs::VerifyItem PcsItem;
    typedef E2 Elem;
    static bool canonical(const u64* w) { return w[0] < GL_P && w[1] < GL_P; }
    static Elem elem(const u64* w) { return e2(w[0], w[1]); }
    static std::string other_field(const char* who) { (void)who; return "the commitment is over BN254: open it with the _bn254 entry"; }
    static size_t nvars(const Open& c) { return c.point.size(); }
    static Open open_claim(size_t input, const u64* value, const u64* point, size_t nv) {
        Open c{input, std::vector<E2>(nv), elem(value)};
        for (size_t j = 0; j < nv; j++) c.point[j] = elem(point + 2 * j);
        return c;
    }
    static void put(const Open& c, u64* value, u64* point) {
        value[0] = c.value.c0; value[1] = c.value.c1;
        for (size_t j = 0; j < c.point.size(); j++) { point[2 * j] = c.point[j].c0; point[2 * j + 1] = c.point[j].c1; }
    }
    static std::vector<E2> point_of(const u64* point, size_t nv) {
        std::vector<E2> pt(nv);
        for (size_t i = 0; i < nv; i++) pt[i] = elem(point + 2 * i);
        return pt;
    }
    // root (hg_verify_public_bound*, else null): the walk of a bound proof
    static std::string verify_public(hg_ctx* ctx, bool device, const hg_pk* pk, const Instance& inst, const uint8_t* proof, size_t len, int mode, std::vector<Open>& open,
                                     const uint8_t* root) {
        return device ? verify_public_device(ctx, pk, inst, proof, len, mode, open, root) : hg::verify_public(pk->params, pk->lasso, pk->circuit, inst, proof, len, mode, open, root);
    }
    static std::string settle(hg_ctx* ctx, const Params& p, const Witness& w, const std::vector<Open>& cl) { return ctx ? claims_settle_device(ctx, p, w, cl) : claims_settle(p, w, cl); }
    static void mle(hg_ctx* ctx, const Params& p, const Instance& inst, int which, int index, const u64* point, size_t nv, u64* out) {
        const std::vector<E2> pt = point_of(point, nv);
        const E2 v = ctx ? instance_mle_device(ctx, p, inst, which, index, pt) : instance_mle(p, inst, which, index, pt);
        out[0] = v.c0; out[1] = v.c1;
    }
    static void mle_batch(hg_ctx* ctx, const Params& p, const std::vector<const Instance*>& I, int which, int index, const u64* point, size_t nv, u64* out) {
        std::vector<E2> res(I.size());
        instance_mle_batch_device(ctx, p, I, which, index, point_of(point, nv), res.data());
        for (size_t i = 0; i < I.size(); i++) { out[2 * i] = res[i].c0; out[2 * i + 1] = res[i].c1; }
    }
    // historical: a commit error of hg_secrets_commit is wrapped with the entry's name here, the BN254 commit is given the name instead
    static pcs::Commitment* commit_secrets(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tabs) {
        try {
            return ctx ? pcs::commit_device(ctx, sh, tabs) : pcs::commit_host(sh, tabs);
        } catch (const std::exception& e) {
            throw Error(std::string(who) + ": " + e.what());
        }
    }
    static std::vector<uint8_t> pcs_open(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& cl, size_t Q) { return pcs::open(who, cm, cl, Q); }
    // ctx: the device form (hg_pcs_verify_device), whose errors carry the entry's name
    static std::string pcs_verify(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& cl, size_t Q, const uint8_t* proof, size_t len) {
        if (!ctx) return pcs::verify(sh, root, cl, Q, proof, len);
        try {
            return pcs::verify_device(ctx, sh, root, cl, Q, proof, len);
        } catch (const std::exception& e) {
            throw Error(std::string(who) + ": " + e.what());
        }
    }
    static std::vector<std::string> pcs_verify_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<PcsItem>& items, size_t Q) {
        return pcs::verify_device_batch(who, ctx, sh, items, Q);
    }
    // folded openings; ctx: the device form of the verifier
    static std::vector<uint8_t> pcs_open_folded(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& cl, size_t Q) { return pcs::open_folded(who, cm, cl, Q); }
    static std::string pcs_verify_folded(hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& cl, size_t Q, const uint8_t* proof, size_t len) {
        return ctx ? pcs::verify_folded_device(ctx, sh, root, cl, Q, proof, len) : pcs::verify_folded(sh, root, cl, Q, proof, len);
    }
    // the batch forms of commit and open (device only): tabs[i * m + t] = table t of member i
    typedef pcs::OpenItem PcsOpenItem;
    static size_t opening_bytes(const pcs::Shape& sh, size_t n_claims, size_t Q) { return pcs::opening_bytes(sh, n_claims, Q); }
    static std::vector<pcs::Commitment*> commit_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tabs, size_t n, bool) {
        return pcs::commit_device_batch(who, ctx, sh, tabs, n);
    }
    static std::vector<pcs::Opened> pcs_open_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q) {
        return pcs::open_device_batch(who, single, ctx, items, Q);
    }
    // the batch forms of the folded openings
    static size_t folded_opening_bytes(const pcs::Shape& sh, size_t Q) { return pcs::folded_opening_bytes(sh, Q); }
    static std::vector<pcs::Opened> pcs_open_folded_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q) {
        return pcs::open_folded_device_batch(who, single, ctx, items, Q);
    }
    static std::vector<std::string> pcs_verify_folded_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<PcsItem>& items, size_t Q) {
        return pcs::verify_folded_device_batch(who, ctx, sh, items, Q);
    }
};

struct BnAbi {
    static constexpr size_t WORDS = 4;
    static constexpr pcs::Field FIELD = pcs::BN254;
    typedef OpenClaimBn Open;
    typedef hg_input_claim_bn254 Wire;
    typedef bn::PcsClaim PcsClaim;
    typedef bn::VerifyItem PcsItem;
    typedef bn::Fr Elem;
    static bool canonical(const u64* w) { return bn254_canonical(w); }
    static Elem elem(const u64* w) { bn::Fr x; memcpy(x.l, w, 32); return x; }
    static std::string other_field(const char* who) {   // names the Goldilocks entry: `who` without its suffix
        const std::string w(who);
        return "the commitment is over Goldilocks: open it with " + w.substr(0, w.size() - strlen("_bn254"));
    }
    static size_t nvars(const Open& c) { return c.point4.size() / 4; }
    static Open open_claim(size_t input, const u64* value, const u64* point, size_t nv) {
        Open c;
        c.input = input;
        memcpy(c.value, value, 32);
        c.point4.assign(point, point + 4 * nv);
        return c;
    }
    static void put(const Open& c, u64* value, u64* point) {
        memcpy(value, c.value, 32);
        if (!c.point4.empty()) memcpy(point, c.point4.data(), c.point4.size() * 8);
    }
    static std::string verify_public(hg_ctx* ctx, bool device, const hg_pk* pk, const Instance& inst, const uint8_t* proof, size_t len, int, std::vector<Open>& open,
                                     const uint8_t*) {   // (BN254 has no protocol modes, so no bound proofs)
        return device ? bn::verify_public_device_bn254(ctx, pk, inst, proof, len, open) : verify_public_bn254(pk->params, pk->lasso, pk->circuit, inst, proof, len, open);
    }
    static std::string settle(hg_ctx* ctx, const Params& p, const Witness& w, const std::vector<Open>& cl) { return ctx ? bn::claims_settle_device_bn254(ctx, p, w, cl) : claims_settle_bn254(p, w, cl); }
    static void mle(hg_ctx* ctx, const Params& p, const Instance& inst, int which, int index, const u64* point, size_t nv, u64* out) {
        if (ctx) bn::instance_mle_device_bn254(ctx, p, inst, which, index, point, nv, out);
        else instance_mle_bn254(p, inst, which, index, point, nv, out);
    }
    static void mle_batch(hg_ctx* ctx, const Params& p, const std::vector<const Instance*>& I, int which, int index, const u64* point, size_t nv, u64* out) {
        std::vector<u64> res(4 * I.size());   // (an error of the device pass leaves out alone)
        bn::instance_mle_batch_device_bn254(ctx, p, I, which, index, point, nv, res.data());
        memcpy(out, res.data(), res.size() * sizeof(u64));
    }
    // the witness words are lifted into Fr by the signed rule (the table hg_claims_settle_bn254 evaluates)
    static pcs::Commitment* commit_secrets(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tabs) {
        return ctx ? bn::pcs_commit_device(who, ctx, sh, tabs, true) : bn::pcs_commit_host(who, sh, tabs, true);
    }
    static std::vector<uint8_t> pcs_open(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& cl, size_t Q) { return bn::pcs_open(who, cm, cl, Q); }
    // ctx: the device form (hg_pcs_verify_device_bn254), whose errors carry the entry's name
    static std::string pcs_verify(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& cl, size_t Q, const uint8_t* proof, size_t len) {
        if (!ctx) return bn::pcs_verify(sh, root, cl, Q, proof, len);
        try {
            return bn::pcs_verify_device(ctx, sh, root, cl, Q, proof, len);
        } catch (const std::exception& e) {
            throw Error(std::string(who) + ": " + e.what());
        }
    }
    static std::vector<std::string> pcs_verify_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<PcsItem>& items, size_t Q) {
        return bn::pcs_verify_device_batch(who, ctx, sh, items, Q);
    }
    // folded openings; ctx: the device form of the verifier
    static std::vector<uint8_t> pcs_open_folded(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& cl, size_t Q) { return bn::pcs_open_folded(who, cm, cl, Q); }
    static std::string pcs_verify_folded(hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& cl, size_t Q, const uint8_t* proof, size_t len) {
        return ctx ? bn::pcs_verify_folded_device(ctx, sh, root, cl, Q, proof, len) : bn::pcs_verify_folded(sh, root, cl, Q, proof, len);
    }
    // the batch forms of commit and open (device only): `secrets` says that the tables are witness words, lifted by the signed rule
    typedef bn::PcsOpenItem PcsOpenItem;
    static size_t opening_bytes(const pcs::Shape& sh, size_t n_claims, size_t Q) { return bn::pcs_opening_bytes(sh, n_claims, Q); }
    static std::vector<pcs::Commitment*> commit_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tabs, size_t n, bool secrets) {
        return bn::pcs_commit_device_batch(who, ctx, sh, tabs, n, secrets);
    }
    static std::vector<pcs::Opened> pcs_open_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q) {
        return bn::pcs_open_device_batch(who, single, ctx, items, Q);
    }
    // the batch forms of the folded openings
    static size_t folded_opening_bytes(const pcs::Shape& sh, size_t Q) { return bn::pcs_folded_opening_bytes(sh, Q); }
    static std::vector<pcs::Opened> pcs_open_folded_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q) {
        return bn::pcs_open_folded_device_batch(who, single, ctx, items, Q);
    }
    static std::vector<std::string> pcs_verify_folded_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<PcsItem>& items, size_t Q) {
        return bn::pcs_verify_folded_device_batch(who, ctx, sh, items, Q);
    }
};
}  // namespace

// a decision of a verifier: "" accepted (0), else rejected (1) with the reason where hg_last_error() finds it
static int decision(const std::string& why) {
    if (why.empty()) return 0;
    g_last_error = why;
    return 1;
}

// item i's slot of a caller's `reasons`: the text cut to reason_cap - 1 bytes, always terminated
static void write_reason(char* reasons, size_t reason_cap, size_t i, const std::string& why) {
    if (!reasons || !reason_cap) return;
    char* r = reasons + i * reason_cap;
    const size_t m = std::min(why.size(), reason_cap - 1);
    memcpy(r, why.data(), m);
    r[m] = 0;
}

// why[i] -> results[i] and the reason slots; returns how many were rejected
static int write_results(const std::vector<std::string>& why, int* results, char* reasons, size_t reason_cap) {
    int rejected = 0;
    for (size_t i = 0; i < why.size(); i++) {
        results[i] = why[i].empty() ? 0 : 1;
        rejected += results[i];
        write_reason(reasons, reason_cap, i, why[i]);
    }
    return rejected;
}

// hg_prove_encryptions*: run(want_witnesses, &total_ms) is the field's pipeline. Historical: the Goldilocks entry also sums gpu_ms and
// replay_ms into the timings (gpu_timings). cmt (hg_prove_encryptions_committed[_bn254]): the run fills it with every proven item's handle;
// commitments and roots are required then, a refused item gets a null handle and a zero root, upload_ms sums the commits' device time.
static std::vector<uint32_t> secrets_nvars(const Params& p);
template <class Run>
static int prove_encryptions_entry(const std::string& who, bool gpu_timings, hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e,
                                   const int64_t* const* k1, const int64_t* const* a, size_t n_enc, uint8_t* proofs, size_t cap_each, size_t* lens, int* status,
                                   hg_witness** ws, char* reasons, size_t reason_cap, hg_timings* timings, Run run, EncCommit* cmt = nullptr, size_t log2_row = 0,
                                   void** commitments = nullptr, uint8_t* roots = nullptr) {
    if (ws) for (size_t i = 0; i < n_enc; i++) ws[i] = nullptr;
    if (cmt && commitments) for (size_t i = 0; i < n_enc; i++) commitments[i] = nullptr;
    if (!ctx) throw Error(who + ": needs a device context (derivation and proving run on the GPU and have no host fallback)");
    if (!pk || (n_enc && (!s || !e || !k1 || !a || !proofs || !lens || !status || (cmt && (!commitments || !roots))))) throw Error(who + ": null argument");
    if (!pk->ctx) throw Error(who + ": host-only prover key (created without a context)");
    for (size_t i = 0; i < n_enc; i++)
        if (!s[i] || !e[i] || !k1[i] || !a[i]) throw Error(who + ": encryption " + std::to_string(i) + ": null polynomial");
    if (cmt) {   // hg_prove_encryptions_committed: the shape of hg_secrets_commit_values, ahead of anything enqueued
        const std::vector<uint32_t> nv = secrets_nvars(pk->params);
        cmt->sh = pcs::make_shape(who.c_str(), nv.data(), nv.size(), log2_row);
        if (cmt->sh.R > 65535) throw Error(who + ": more than 65535 rows (choose a larger log2_row)");
    }
    double total = 0;
    std::vector<EncResult> rs = run(ws != nullptr, &total);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->total_ms = total; }
    for (size_t i = 0; i < n_enc; i++)
        if (!rs[i].refused && rs[i].r.proof.size() > cap_each)
            throw Error(who + ": encryption " + std::to_string(i) + ": proof buffer too small (" + std::to_string(rs[i].r.proof.size()) + " bytes)");
    int refused = 0;
    for (size_t i = 0; i < n_enc; i++) {
        const EncResult& r = rs[i];
        status[i] = r.refused ? 1 : 0;
        lens[i] = r.refused ? 0 : r.r.proof.size();
        write_reason(reasons, reason_cap, i, r.reason);
        if (cmt) memset(roots + 32 * i, 0, 32);
        if (r.refused) { refused++; continue; }
        memcpy(proofs + i * cap_each, r.r.proof.data(), r.r.proof.size());
        if (ws) ws[i] = new hg_witness{std::move(rs[i].w), pk->params.raw};
        if (cmt) {
            memcpy(roots + 32 * i, cmt->cms[i]->root(), 32);
            commitments[i] = cmt->cms[i].release();
            if (timings) timings->upload_ms += cmt->ms[i];
        }
        if (timings) { timings->prove_ms += r.r.prove_ms; timings->witness_ms += r.witness_gpu_ms; }
        if (timings && gpu_timings) { timings->gpu_ms += r.r.gpu_ms; timings->replay_ms += r.r.replay_ms; }
    }
    return refused;
}

// the caller's room against hg_pk_claim_shape, ahead of the walk (`each`: " per proof" in a batch)
static void check_claim_room(const std::string& who, const hg_pk* pk, const void* claims, size_t claim_cap, const u64* points, size_t coord_cap, const char* each) {
    size_t need_claims = 0, need_coords = 0;
    claim_shape(pk->params, pk->lasso, pk->circuit, &need_claims, &need_coords);
    if (claim_cap < need_claims || coord_cap < need_coords || (need_claims && !claims) || (need_coords && !points))
        throw Error(who + ": room for " + std::to_string(need_claims) + " claims and " + std::to_string(need_coords) + " coordinates" + each + " is needed (hg_pk_claim_shape)");
}

// ... and after it, before anything is written: an error of the call leaves the outputs alone
template <class A>
static void check_claim_count(const std::string& who, const std::vector<typename A::Open>& open, size_t claim_cap, size_t coord_cap) {
    size_t coords = 0;
    for (const typename A::Open& c : open) coords += A::nvars(c);
    if (open.size() > claim_cap || coords > coord_cap) throw Error(who + ": the walk left more claims than hg_pk_claim_shape counts");
}

// a run of open claims into a caller's block: the claims, and their points one behind the other
template <class A>
static void put_claims(const std::vector<typename A::Open>& open, void* claims, u64* points) {
    typename A::Wire* out = static_cast<typename A::Wire*>(claims);
    size_t off = 0;
    for (size_t i = 0; i < open.size(); i++) {
        out[i].input = (uint32_t)open[i].input;
        out[i].nvars = (uint32_t)A::nvars(open[i]);
        out[i].point_off = off;
        A::put(open[i], out[i].value, points + A::WORDS * off);
        off += out[i].nvars;
    }
}

// the entries that bind a proof to its statement (hg.h: "Bound proofs"): modes 1 and 3 only
static void check_bound_mode(const std::string& who, int mode) {
    if (mode < 0 || mode > 3) throw Error(who + ": unknown mode bits");
    if (!(mode & 1)) throw Error(who + ": binding needs the absorbing transcript (mode bit 1)");
}

// hg_verify_public*, hg_verify_public_device*; bound (hg_verify_public_bound*): the walk of a bound proof against `root`
template <class A>
static int verify_public_entry(const char* who, hg_ctx* ctx, bool device, const hg_pk* pk, const void* instance, int mode, const uint8_t* proof, size_t len,
                               void* claims, size_t claim_cap, uint64_t* points, size_t coord_cap, size_t* n_claims, bool bound = false, const uint8_t* root = nullptr) {
    if (n_claims) *n_claims = 0;
    if (device && (!ctx || !pk || !pk->ctx)) throw Error(std::string(who) + ": needs a device context and a device prover key");
    if (!pk || !instance || !proof || !n_claims || (bound && !root)) throw Error(std::string(who) + ": null argument");
    if (mode < 0 || mode > 3) throw Error(std::string(who) + ": unknown mode bits");
    if (bound) check_bound_mode(who, mode);
    const hg_instance* in = as_instance(instance);
    check_instance(pk, in, who);
    check_claim_room(who, pk, claims, claim_cap, points, coord_cap, "");
    std::vector<typename A::Open> open;
    const std::string why = A::verify_public(ctx, device, pk, in->inst, proof, len, mode, open, bound ? root : nullptr);
    if (!why.empty()) return decision(why);
    check_claim_count<A>(who, open, claim_cap, coord_cap);
    put_claims<A>(open, claims, points);
    *n_claims = open.size();
    return 0;
}

// The four batch entries in one frame: the argument checks, every element checked and gathered, the device pass with its errors given
// the entry's name, results and reasons, and for the instance-checked ones (hg_verify_public_batch*) the claims. Item is Witness
// (handles: hg_witness) or Instance (handles: hg_instance); run(items, P, N, why, open) is the field's device pass.
// Historical: the witness batches report a missing context as "null argument" and a host-only key second, in words of its own; the
// public batches report both first, in one message.
// bound (hg_verify_public_bound_batch): roots[i] is item i's 32-byte root - the array and every element checked here, the mode by
// check_bound_mode; run reads the array as it is.
template <class A, class Item, class Run>
static int batch_entry(const std::string& who, hg_ctx* ctx, const hg_pk* pk, const void* const* handles, const uint8_t* const* proofs, const size_t* lens, size_t n, int mode,
                       int* results, void* claims, size_t claim_cap_each, uint64_t* points, size_t coord_cap_each, size_t* n_claims, char* reasons, size_t reason_cap, Run run,
                       bool bound = false, const uint8_t* const* roots = nullptr) {
    constexpr bool pub = std::is_same<Item, Instance>::value;
    if (bound) check_bound_mode(who, mode);   // (the mode rule comes first, as in hg_prove_committed_mode: its text is part of the contract)
    if (pub) {
        if (!ctx || !pk || !pk->ctx) throw Error(who + ": needs a device context and a device prover key");
        if (n && (!handles || !proofs || !lens || !results || !n_claims || (bound && !roots))) throw Error(who + ": null argument");
    } else {
        if (!ctx || !pk || (n && (!handles || !proofs || !lens || !results))) throw Error(who + ": null argument");
        if (!pk->ctx) throw Error(who + ": needs a device prover key (hg_setup with a context)");
    }
    if (mode < 0 || mode > 3) throw Error(who + ": unknown mode bits");
    if (pub && n) check_claim_room(who, pk, claims, claim_cap_each, points, coord_cap_each, " per proof");
    std::vector<const Item*> items(n);
    std::vector<const uint8_t*> P(n);
    std::vector<size_t> N(n);
    for (size_t i = 0; i < n; i++) {
        if (!handles[i] || !proofs[i]) throw Error(who + ": null " + (pub ? "instance" : "witness") + " or proof at index " + std::to_string(i));
        if (bound && !roots[i]) throw Error(who + ": null root at index " + std::to_string(i));
        if constexpr (pub) {
            check_instance(pk, as_instance(handles[i]), (who + ": index " + std::to_string(i)).c_str());
            items[i] = &as_instance(handles[i])->inst;
        } else {
            check_witness(pk, static_cast<const hg_witness*>(handles[i]), who.c_str());
            items[i] = &static_cast<const hg_witness*>(handles[i])->w;
        }
        P[i] = proofs[i]; N[i] = lens[i];
    }
    if (!n) return 0;
    std::vector<std::string> why;
    std::vector<std::vector<typename A::Open>> open;
    try {
        run(items, P, N, why, open);
    } catch (const std::exception& e) {
        const std::string m = e.what();
        throw Error(m.rfind(who, 0) == 0 ? m : who + ": " + m);
    }
    if (pub)
        for (size_t i = 0; i < n; i++) check_claim_count<A>(who + ": proof " + std::to_string(i), open[i], claim_cap_each, coord_cap_each);
    const int rejected = write_results(why, results, reasons, reason_cap);
    if (pub)
        for (size_t i = 0; i < n; i++) {
            n_claims[i] = results[i] ? 0 : open[i].size();
            if (!results[i]) put_claims<A>(open[i], static_cast<typename A::Wire*>(claims) + i * claim_cap_each, points + A::WORDS * i * coord_cap_each);
        }
    return rejected;
}

// hg_claims_settle*: the claims of the caller's block against the witness handle, on the host or with a context on the device
template <class A>
static int claims_settle_entry(const std::string& who, hg_ctx* ctx, const hg_params* params, const hg_witness* w, const void* claims, size_t n, const uint64_t* points) {
    if (!params || !w || (n && (!claims || !points))) throw Error(who + ": null argument");
    Params p(*params);
    const size_t SZ = p.SZ(), k = (size_t)p.k;
    const Witness& v = w->w;
    if (w->params.n != params->n || w->params.k != params->k || v.s.size() != SZ || v.e.size() != SZ || v.k1.size() != SZ || v.ais.size() != k * SZ ||
        v.r1is.size() != k * SZ || v.r2is.size() != k * p.PZ())
        throw Error(who + ": the witness was built for other parameters");
    const typename A::Wire* in = static_cast<const typename A::Wire*>(claims);
    std::vector<typename A::Open> cl(n);
    for (size_t i = 0; i < n; i++) {
        if (in[i].input > 3 + 2 * k) throw Error(who + ": input " + std::to_string(in[i].input) + " is not an input of the circuit");
        if (in[i].nvars > 40) throw Error(who + ": a claim with " + std::to_string(in[i].nvars) + " coordinates");
        const u64* pt = points + A::WORDS * in[i].point_off;
        cl[i] = A::open_claim(in[i].input, in[i].value, pt, in[i].nvars);
        for (size_t j = 0; j < in[i].nvars; j++) if (!A::canonical(pt + A::WORDS * j)) throw Error(who + ": non-canonical coordinate");
        if (!A::canonical(in[i].value)) throw Error(who + ": non-canonical value");
    }
    return decision(A::settle(ctx, p, v, cl));
}

// hg_instance_mle* (batch false: instances is the one handle) and hg_instance_mle_batch* (device only; every instance of the
// parameters of the first)
template <class A>
static int instance_mle_entry(const std::string& who, bool batch, hg_ctx* ctx, const void* const* instances, size_t n, int which, int index, const uint64_t* point,
                              size_t nvars, uint64_t* out) {
    if (batch && !ctx) throw Error(who + ": needs a device context");
    if (!instances || (!batch && !instances[0]) || (nvars && !point) || !out) throw Error(who + ": null argument");
    if (!n) return 0;
    std::vector<const Instance*> I(n);
    for (size_t i = 0; i < n; i++) {
        if (batch) {
            if (!instances[i]) throw Error(who + ": null instance at index " + std::to_string(i));
            const hg_params &a = as_instance(instances[0])->params, &b = as_instance(instances[i])->params;
            if (a.n != b.n || a.k != b.k || memcmp(a.qis, b.qis, sizeof(a.qis[0]) * a.k) != 0)
                throw Error(who + ": the instance at index " + std::to_string(i) + " was built for other parameters than the first");
        }
        I[i] = &as_instance(instances[i])->inst;
    }
    Params p(as_instance(instances[0])->params);
    if (which != 0 && which != 1) throw Error(who + ": which is 0 (ais[index]) or 1 (ct0is)");
    if (which == 0 && (index < 0 || index >= p.k)) throw Error(who + ": no such modulus");
    if (nvars != (size_t)(which ? p.ct0is_log2() : p.L)) throw Error(who + ": the table has " + std::to_string(which ? p.ct0is_log2() : p.L) + " variables");
    if (batch)
        for (const Instance* x : I)
            if (x->a.size() != (size_t)p.k * p.PZ() || x->ct0.size() != (size_t)p.k * p.PZ()) throw Error(who + ": an instance of the wrong size");
    for (size_t i = 0; i < nvars; i++)
        if (!A::canonical(point + A::WORDS * i)) throw Error(who + ": non-canonical coordinate");
    if (batch) A::mle_batch(ctx, p, I, which, index, point, nvars, out);
    else A::mle(ctx, p, *I[0], which, index, point, nvars, out);
    return 0;
}

// ---- polynomial commitment (pcs.hpp, pcs_bn254.hpp): hg_pcs_* on caller tables, hg_secrets_commit / hg_claims_open / hg_claims_verify
// for the five secret inputs of an encryption
template <class A>
static std::vector<typename A::PcsClaim> pcs_claims(const char* who, const pcs::Shape& sh, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n) {
    const std::string w(who);
    if (n > pcs::MAX_CLAIMS) throw Error(w + ": more than " + std::to_string(pcs::MAX_CLAIMS) + " claims");
    std::vector<typename A::PcsClaim> cl(n);
    const uint64_t* pt = points;
    for (size_t i = 0; i < n; i++) {
        if (table[i] >= sh.nvars.size()) throw Error(w + ": claim " + std::to_string(i) + " names table " + std::to_string(table[i]) + " of " + std::to_string(sh.nvars.size()));
        cl[i].table = table[i];
        cl[i].point.resize((size_t)sh.nvars[table[i]]);
        for (size_t j = 0; j < cl[i].point.size(); j++) cl[i].point[j] = A::elem(pt + A::WORDS * j);
        cl[i].value = A::elem(values + A::WORDS * i);
        for (size_t j = 0; j < cl[i].point.size(); j++) if (!A::canonical(pt + A::WORDS * j)) throw Error(w + ": claim " + std::to_string(i) + ": non-canonical coordinate");
        if (!A::canonical(values + A::WORDS * i)) throw Error(w + ": claim " + std::to_string(i) + ": non-canonical value");
        pt += A::WORDS * cl[i].point.size();
    }
    return cl;
}
static size_t pcs_queries(const char* who, size_t n_queries) {
    if (n_queries > pcs::MAX_QUERIES) throw Error(std::string(who) + ": more than " + std::to_string(pcs::MAX_QUERIES) + " queries");
    return n_queries ? n_queries : pcs::DEFAULT_QUERIES;
}
static void pcs_emit(const char* who, const std::vector<uint8_t>& bytes, uint8_t* out, size_t cap, size_t* len) {
    *len = bytes.size();
    if (bytes.size() > cap) throw Error(std::string(who) + ": the opening has " + std::to_string(bytes.size()) + " bytes, the buffer " + std::to_string(cap));
    memcpy(out, bytes.data(), bytes.size());
}
// the secret inputs as commitment tables, in input order s, e, k1, r1is[0..k-1], r2is
static std::vector<uint32_t> secrets_nvars(const Params& p) {
    std::vector<uint32_t> v(3 + (size_t)p.k, (uint32_t)p.L);
    v.push_back((uint32_t)(p.n_log2 + p.log2k));
    return v;
}
// an array of input claims -> (table, points, values) of the commitment over the secret inputs
template <class A>
static void secrets_claims(const char* who, const Params& p, const void* claims, size_t n, const uint64_t* points, std::vector<uint32_t>& table,
                           std::vector<uint64_t>& pts, std::vector<uint64_t>& vals) {
    const std::string w(who);
    if (n > pcs::MAX_CLAIMS) throw Error(w + ": more than " + std::to_string(pcs::MAX_CLAIMS) + " claims");
    const typename A::Wire* in = static_cast<const typename A::Wire*>(claims);
    const std::vector<uint32_t> nv = secrets_nvars(p);
    const uint32_t k = (uint32_t)p.k;
    for (size_t i = 0; i < n; i++) {
        const uint32_t id = in[i].input;
        uint32_t t;
        if (id < 3) t = id;
        else if (id >= 3 + k && id < 3 + 2 * k) t = id - k;
        else if (id == 3 + 2 * k) t = 3 + k;
        else throw Error(w + ": claim " + std::to_string(i) + " is on input " + std::to_string(id) + ", which is not a secret input (0, 1, 2, " + std::to_string(3 + k) + " .. " + std::to_string(3 + 2 * k) + ")");
        if (in[i].nvars != nv[t]) throw Error(w + ": claim " + std::to_string(i) + " has " + std::to_string(in[i].nvars) + " coordinates, input " + std::to_string(id) + " has " + std::to_string(nv[t]) + " variables");
        table.push_back(t);
        pts.insert(pts.end(), points + A::WORDS * in[i].point_off, points + A::WORDS * (in[i].point_off + in[i].nvars));
        vals.insert(vals.end(), in[i].value, in[i].value + A::WORDS);
    }
}

// hg_pcs_open* after its null checks, and the tail of hg_claims_open* (which has checked the field already)
template <class A>
static int pcs_open_entry(const char* who, hg_ctx* ctx, const pcs::Commitment* cm, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims,
                          size_t n_queries, uint8_t* proof, size_t cap, size_t* len) {
    if (cm->field != A::FIELD) throw Error(std::string(who) + ": " + A::other_field(who));
    if (cm->ctx != ctx) throw Error(std::string(who) + ": the commitment was made " + (cm->ctx ? "on a device context: pass that context" : "by the host form: pass no context"));
    const std::vector<typename A::PcsClaim> cl = pcs_claims<A>(who, cm->sh, table, points, values, n_claims);
    pcs_emit(who, A::pcs_open(who, *cm, cl, pcs_queries(who, n_queries)), proof, cap, len);
    return 0;
}

template <class A>
static int pcs_open_api(const char* who, hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims,
                        size_t n_queries, uint8_t* proof, size_t cap, size_t* len) {
    if (len) *len = 0;
    if (!commitment || !proof || !len || (n_claims && (!table || !points || !values))) throw Error(std::string(who) + ": null argument");
    return pcs_open_entry<A>(who, ctx, static_cast<const pcs::Commitment*>(commitment), table, points, values, n_claims, n_queries, proof, cap, len);
}

// hg_pcs_verify* (device == false) and hg_pcs_verify_device: the same argument checks in the same order, then the form's verifier
template <class A>
static int pcs_verify_entry(const char* who, bool device, hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row,
                            const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    const std::string w(who);
    if (!root || !nvars || (len && !proof) || (n_claims && (!table || !points || !values))) throw Error(w + ": null argument");
    const pcs::Shape sh = pcs::make_shape(who, nvars, n_tables, log2_row);
    const std::vector<typename A::PcsClaim> cl = pcs_claims<A>(who, sh, table, points, values, n_claims);
    const size_t Q = pcs_queries(who, n_queries);
    if (device && !ctx) throw Error(w + ": no context");
    return decision(A::pcs_verify(who, device ? ctx : nullptr, sh, root, cl, Q, proof, len));
}

// hg_secrets_commit*
template <class A>
static int secrets_commit_entry(const char* who, hg_ctx* ctx, const hg_params* params, const hg_witness* w, size_t log2_row, void** commitment, uint8_t root[32]) {
    if (commitment) *commitment = nullptr;
    if (!params || !w || !commitment || !root) throw Error(std::string(who) + ": null argument");
    Params p(*params);
    const size_t SZ = p.SZ(), k = (size_t)p.k;
    const Witness& v = w->w;
    if (w->params.n != params->n || w->params.k != params->k || v.s.size() != SZ || v.e.size() != SZ || v.k1.size() != SZ || v.r1is.size() != k * SZ ||
        v.r2is.size() != k * p.PZ())
        throw Error(std::string(who) + ": the witness was built for other parameters");
    const std::vector<uint32_t> nv = secrets_nvars(p);
    std::vector<const uint64_t*> tabs = {v.s.data(), v.e.data(), v.k1.data()};
    for (size_t i = 0; i < k; i++) tabs.push_back(v.r1is.data() + i * SZ);
    tabs.push_back(v.r2is.data());
    const pcs::Shape sh = pcs::make_shape(who, nv.data(), nv.size(), log2_row);
    pcs::Commitment* cm = A::commit_secrets(who, ctx, sh, tabs.data());
    memcpy(root, cm->root(), 32);
    *commitment = cm;
    return 0;
}

// a values object of this key and this context (hg_secrets_commit_values, hg_values_instance_digest, hg_prove_committed_mode)
static void check_values_of(const std::string& w, hg_ctx* ctx, const hg_pk* pk, const hg_values* v) {
    if (!ctx) throw Error(w + ": no context");
    if (!pk->ctx) throw Error(w + ": host-only prover key (created without a context)");
    if (v->pk_serial != pk->serial) throw Error(w + ": the values were laid out for another prover key");
    if (v->ctx != ctx || pk->ctx != ctx) throw Error(w + ": the values or the prover key belong to another context");
}

// where the public tables of a values object lie (the laid-out read of the statement digest): inputs 3 .. 3+k-1 and ct0is
static pcs::DigestMember values_public_tables(const std::string& w, const hg_pk* pk, const hg_values* v) {
    const Params& p = pk->params;
    const std::vector<int>& ids = pk->circuit.input_ids;
    if (ids.size() != 3 + 2 * (size_t)p.k + 1) throw Error(w + ": unexpected input nodes");
    pcs::DigestMember mem;
    memset(&mem, 0, sizeof(mem));
    for (size_t i = 0; i < (size_t)p.k; i++) {
        const size_t id = (size_t)ids[3 + i];
        if (id >= v->d_vals.size() || !v->d_vals[id])
            throw Error(w + ": input " + std::to_string(3 + i) + " is not resident in these values (a rank's share of hg_witness_gen_shard holds only what the rank reads)");
        if (v->sizes[id] != p.SZ()) throw Error(w + ": table size mismatch");
        mem.a[i] = v->d_vals[id];
    }
    if (!v->d_ct0is) throw Error(w + ": ct0is is not resident in these values (a rank's share of hg_witness_gen_shard holds only what the rank reads)");
    if (v->ct0is_len != (size_t)p.k * p.SZ()) throw Error(w + ": table size mismatch");
    mem.ct0 = v->d_ct0is;
    return mem;
}

// hg_secrets_commit_values: the tables of secrets_commit_entry where hg_witness_gen left them in HBM. dg (hg_prove_committed_mode, may be
// null): the statement digest of the same values object beside the commit
static int secrets_commit_values_entry(const char* who, hg_ctx* ctx, const hg_pk* pk, const hg_values* v, size_t log2_row, void** commitment, uint8_t root[32],
                                       pcs::DigestJob* dg = nullptr) {
    const std::string w(who);
    if (commitment) *commitment = nullptr;
    if (!pk || !v || !commitment || !root) throw Error(w + ": null argument");
    check_values_of(w, ctx, pk, v);
    const Params& p = pk->params;
    const size_t k = (size_t)p.k;
    const std::vector<int>& ids = pk->circuit.input_ids;
    if (ids.size() != 3 + 2 * k + 1) throw Error(w + ": unexpected input nodes");
    const std::vector<uint32_t> nv = secrets_nvars(p);
    std::vector<size_t> inputs = {0, 1, 2};
    for (size_t i = 0; i < k; i++) inputs.push_back(3 + k + i);
    inputs.push_back(3 + 2 * k);
    std::vector<const u64*> tabs;
    for (size_t t = 0; t < inputs.size(); t++) {
        const size_t id = (size_t)ids[inputs[t]];
        if (id >= v->d_vals.size() || !v->d_vals[id])
            throw Error(w + ": input " + std::to_string(inputs[t]) + " is not resident in these values (a rank's share of hg_witness_gen_shard holds only what the rank reads)");
        if (v->sizes[id] != (size_t)1 << nv[t]) throw Error(w + ": table size mismatch");
        tabs.push_back(v->d_vals[id]);
    }
    const pcs::Shape sh = pcs::make_shape(who, nv.data(), nv.size(), log2_row);
    pcs::Commitment* cm;
    if (dg) { dg->p = &p; dg->mem = values_public_tables(w, pk, v); }
    try {
        cm = pcs::commit_device_values(ctx, sh, tabs.data(), dg);
    } catch (const std::exception& e) {
        throw Error(w + ": " + e.what());
    }
    if (dg && dg->flag) { delete cm; throw Error(w + ": a word of ais or ct0is is not a signed value in [-(q_i-1)/2, (q_i-1)/2]"); }
    memcpy(root, cm->root(), 32);
    *commitment = cm;
    return 0;
}

// ---- folded openings (pcs.hpp, pcs_bn254.hpp). hg_pcs_open_folded* after its null checks, and the tail of hg_claims_open_folded*
template <class A>
static int pcs_open_folded_entry(const char* who, hg_ctx* ctx, const pcs::Commitment* cm, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims,
                                 size_t n_queries, uint8_t* proof, size_t cap, size_t* len) {
    const std::string w(who);
    if (cm->field != A::FIELD) throw Error(w + ": " + A::other_field(who));
    if (cm->ctx != ctx) throw Error(w + ": the commitment was made " + (cm->ctx ? "on a device context: pass that context" : "by the host form: pass no context"));
    if (!n_claims) throw Error(w + ": a folded opening needs a claim");
    const std::vector<typename A::PcsClaim> cl = pcs_claims<A>(who, cm->sh, table, points, values, n_claims);
    pcs_emit(who, A::pcs_open_folded(who, *cm, cl, pcs_queries(who, n_queries)), proof, cap, len);
    return 0;
}
template <class A>
static int pcs_open_folded_api(const char* who, hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims,
                               size_t n_queries, uint8_t* proof, size_t cap, size_t* len) {
    if (len) *len = 0;
    if (!commitment || !proof || !len || (n_claims && (!table || !points || !values))) throw Error(std::string(who) + ": null argument");
    return pcs_open_folded_entry<A>(who, ctx, static_cast<const pcs::Commitment*>(commitment), table, points, values, n_claims, n_queries, proof, cap, len);
}
// hg_pcs_verify_folded* (device == false) and hg_pcs_verify_folded_device*: pcs_verify_entry's checks in its order, then the form's verifier
template <class A>
static int pcs_verify_folded_entry(const char* who, bool device, hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row,
                                   const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    const std::string w(who);
    if (!root || !nvars || (len && !proof) || (n_claims && (!table || !points || !values))) throw Error(w + ": null argument");
    const pcs::Shape sh = pcs::make_shape(who, nvars, n_tables, log2_row);
    if (!n_claims) throw Error(w + ": a folded opening needs a claim");
    const std::vector<typename A::PcsClaim> cl = pcs_claims<A>(who, sh, table, points, values, n_claims);
    const size_t Q = pcs_queries(who, n_queries);
    if (!device) return decision(A::pcs_verify_folded(nullptr, sh, root, cl, Q, proof, len));
    if (!ctx) throw Error(w + ": no context");
    try {
        return decision(A::pcs_verify_folded(ctx, sh, root, cl, Q, proof, len));
    } catch (const std::exception& e) {
        throw Error(w + ": " + e.what());
    }
}

// hg_claims_open*: `mine` names the entry that made the commitment (hg_secrets_commit*)
template <class A>
static int claims_open_entry(const char* who, const char* mine, hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points,
                             size_t n_queries, uint8_t* opening, size_t cap, size_t* len, bool folded = false) {
    if (len) *len = 0;
    if (!params || !commitment || !opening || !len || (n && (!claims || !points))) throw Error(std::string(who) + ": null argument");
    Params p(*params);
    const pcs::Commitment* cm = static_cast<const pcs::Commitment*>(commitment);
    if (cm->field != A::FIELD) throw Error(std::string(who) + ": " + A::other_field(who));
    const std::vector<uint32_t> nv = secrets_nvars(p);
    if (cm->sh.nvars.size() != nv.size() || !std::equal(nv.begin(), nv.end(), cm->sh.nvars.begin(), [](uint32_t a, int b) { return (int)a == b; }))
        throw Error(std::string(who) + ": the commitment is not " + mine + "'s for these parameters");
    std::vector<uint32_t> table;
    std::vector<uint64_t> pts, vals;
    secrets_claims<A>(who, p, claims, n, points, table, pts, vals);
    if (folded) return pcs_open_folded_entry<A>(who, ctx, cm, table.data(), pts.data(), vals.data(), n, n_queries, opening, cap, len);
    return pcs_open_entry<A>(who, ctx, cm, table.data(), pts.data(), vals.data(), n, n_queries, opening, cap, len);
}

// hg_claims_verify*, hg_claims_verify_device
template <class A>
static int claims_verify_entry(const char* who, bool device, hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n,
                               const uint64_t* points, size_t n_queries, const uint8_t* opening, size_t len, bool folded = false) {
    if (!params || !root || (len && !opening) || (n && (!claims || !points))) throw Error(std::string(who) + ": null argument");
    Params p(*params);
    const std::vector<uint32_t> nv = secrets_nvars(p);
    std::vector<uint32_t> table;
    std::vector<uint64_t> pts, vals;
    (void)pcs::make_shape(who, nv.data(), nv.size(), log2_row);   // a shape error is reported ahead of a claim's
    secrets_claims<A>(who, p, claims, n, points, table, pts, vals);
    if (folded) return pcs_verify_folded_entry<A>(who, device, ctx, root, nv.data(), nv.size(), log2_row, table.data(), pts.data(), vals.data(), n, n_queries, opening, len);
    return pcs_verify_entry<A>(who, device, ctx, root, nv.data(), nv.size(), log2_row, table.data(), pts.data(), vals.data(), n, n_queries, opening, len);
}

// hg_pcs_verify_device_batch and hg_claims_verify_batch after their argument checks (every item's, ahead of anything enqueued: an
// error of the call writes no output): the device pass with its errors given the entry's name, results and reasons
template <class A>
static int pcs_verify_batch_tail(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const uint8_t* const* roots, const std::vector<std::vector<typename A::PcsClaim>>& cl,
                                 size_t Q, const uint8_t* const* proofs, const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap, bool folded = false) {
    const std::string w(who);
    if (!n) return 0;
    if (!ctx) throw Error(w + ": no context");
    // folded: an item without a claim (hg_claims_verify_folded_batch lets it through) is rejected here and never reaches the device
    std::vector<size_t> at;
    for (size_t i = 0; i < n; i++)
        if (!folded || !cl[i].empty()) at.push_back(i);
    std::vector<typename A::PcsItem> items(at.size());
    for (size_t k = 0; k < at.size(); k++) items[k] = typename A::PcsItem{roots[at[k]], &cl[at[k]], proofs[at[k]], lens[at[k]]};
    std::vector<std::string> got, why(n, folded ? w + ": a folded opening needs a claim" : std::string());
    try {
        got = folded ? A::pcs_verify_folded_batch(who, ctx, sh, items, Q) : A::pcs_verify_batch(who, ctx, sh, items, Q);
    } catch (const std::exception& e) {
        const std::string m = e.what();
        throw Error(m.rfind(w, 0) == 0 ? m : w + ": " + m);
    }
    for (size_t k = 0; k < at.size(); k++) why[at[k]] = std::move(got[k]);
    return write_results(why, results, reasons, reason_cap);
}

// hg_pcs_verify_device_batch*: item i's checks are pcs_verify_entry's, in its order, under the name "<entry>: index i"
template <class A>
static int pcs_verify_batch_entry(const char* who, hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row,
                                  const uint32_t* const* tables, const uint64_t* const* points, const uint64_t* const* values, const size_t* n_claims, size_t n_queries,
                                  const uint8_t* const* proofs, const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap, bool folded = false) {
    const std::string w(who);
    if (!nvars || (n && (!roots || !n_claims || !proofs || !lens || !results))) throw Error(w + ": null argument");
    const pcs::Shape sh = pcs::make_shape(who, nvars, n_tables, log2_row);
    const size_t Q = pcs_queries(who, n_queries);
    std::vector<std::vector<typename A::PcsClaim>> cl(n);
    for (size_t i = 0; i < n; i++) {
        const std::string at = w + ": index " + std::to_string(i);
        const bool has = n_claims[i] != 0;
        if (!roots[i] || (lens[i] && !proofs[i]) || (has && (!tables || !points || !values || !tables[i] || !points[i] || !values[i]))) throw Error(at + ": null argument");
        if (folded && !has) throw Error(at + ": a folded opening needs a claim");
        cl[i] = pcs_claims<A>(at.c_str(), sh, has ? tables[i] : nullptr, has ? points[i] : nullptr, has ? values[i] : nullptr, n_claims[i]);
    }
    return pcs_verify_batch_tail<A>(who, ctx, sh, roots, cl, Q, proofs, lens, n, results, reasons, reason_cap, folded);
}

// hg_claims_verify_batch*: the claim and point blocks as hg_verify_public_batch* writes them, item i's under claims_verify_entry's mapping
template <class A>
static int claims_verify_batch_entry(const char* who, hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims,
                                     size_t claim_cap_each, const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries,
                                     const uint8_t* const* openings, const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap, bool folded = false) {
    const std::string w(who);
    if (!params || (n && (!roots || !n_claims || !openings || !lens || !results))) throw Error(w + ": null argument");
    Params p(*params);
    const std::vector<uint32_t> nv = secrets_nvars(p);
    const pcs::Shape sh = pcs::make_shape(who, nv.data(), nv.size(), log2_row);
    const size_t Q = pcs_queries(who, n_queries);
    std::vector<std::vector<typename A::PcsClaim>> cl(n);
    for (size_t i = 0; i < n; i++) {
        const std::string at = w + ": index " + std::to_string(i);
        if (!roots[i] || (lens[i] && !openings[i]) || (n_claims[i] && (!claims || !points))) throw Error(at + ": null argument");
        if (n_claims[i] > claim_cap_each) throw Error(at + ": " + std::to_string(n_claims[i]) + " claims in a block of " + std::to_string(claim_cap_each));
        const typename A::Wire* in = static_cast<const typename A::Wire*>(claims) + i * claim_cap_each;
        for (size_t j = 0; j < n_claims[i]; j++)
            if (in[j].point_off > coord_cap_each || in[j].nvars > coord_cap_each - in[j].point_off)
                throw Error(at + ": claim " + std::to_string(j) + " has its point outside the block of " + std::to_string(coord_cap_each) + " coordinates");
        std::vector<uint32_t> table;
        std::vector<uint64_t> pts, vals;
        secrets_claims<A>(at.c_str(), p, in, n_claims[i], points ? points + A::WORDS * i * coord_cap_each : nullptr, table, pts, vals);
        cl[i] = pcs_claims<A>(at.c_str(), sh, table.data(), pts.data(), vals.data(), n_claims[i]);
    }
    return pcs_verify_batch_tail<A>(who, ctx, sh, roots, cl, Q, openings, lens, n, results, reasons, reason_cap, folded);
}

// ---- the batch forms of commit and open (device only). An error of the call writes nothing: every item is checked before anything
// is enqueued, and the outputs are written once the whole run is done.
// hg_pcs_commit_batch* and hg_secrets_commit_batch* after their argument checks: tabs[i * m + t] = table t of member i (`secrets`:
// the tables are witness words, which the BN254 form lifts by the signed rule)
template <class A>
static int commit_batch_tail(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<const u64*>& tabs, size_t n, bool secrets, void** commitments, uint8_t* roots) {
    const std::string w(who);
    if (sh.R > 65535) throw Error(w + ": more than 65535 rows (choose a larger log2_row)");
    if (!n) return 0;
    if (!ctx) throw Error(w + ": no context");
    std::vector<pcs::Commitment*> cms;
    try {
        cms = A::commit_batch(who, ctx, sh, tabs.data(), n, secrets);
    } catch (const std::exception& e) {
        const std::string m = e.what();
        throw Error(m.rfind(w, 0) == 0 ? m : w + ": " + m);
    }
    for (size_t i = 0; i < n; i++) {
        memcpy(roots + 32 * i, cms[i]->root(), 32);
        commitments[i] = cms[i];
    }
    return 0;
}

// hg_pcs_commit_batch*
template <class A>
static int pcs_commit_batch_entry(const char* who, hg_ctx* ctx, const uint64_t* const* const* tables, const uint32_t* nvars, size_t n_tables, size_t log2_row, size_t n,
                                  void** commitments, uint8_t* roots) {
    const std::string w(who);
    if (!nvars || (n && (!tables || !commitments || !roots))) throw Error(w + ": null argument");
    const pcs::Shape sh = pcs::make_shape(who, nvars, n_tables, log2_row);
    std::vector<const u64*> tabs;
    for (size_t i = 0; i < n; i++) {
        const std::string at = w + ": index " + std::to_string(i);
        if (!tables[i]) throw Error(at + ": null argument");
        for (size_t t = 0; t < n_tables; t++) {
            if (!tables[i][t]) throw Error(at + ": null table " + std::to_string(t));
            tabs.push_back(tables[i][t]);
        }
    }
    return commit_batch_tail<A>(who, ctx, sh, tabs, n, false, commitments, roots);
}

// hg_secrets_commit_batch*: member i's tables are secrets_commit_entry's for ws[i]
template <class A>
static int secrets_commit_batch_entry(const char* who, hg_ctx* ctx, const hg_params* params, const hg_witness* const* ws, size_t n, size_t log2_row, void** commitments,
                                      uint8_t* roots) {
    const std::string w(who);
    if (!params || (n && (!ws || !commitments || !roots))) throw Error(w + ": null argument");
    Params p(*params);
    const size_t SZ = p.SZ(), k = (size_t)p.k;
    const std::vector<uint32_t> nv = secrets_nvars(p);
    const pcs::Shape sh = pcs::make_shape(who, nv.data(), nv.size(), log2_row);
    std::vector<const u64*> tabs;
    for (size_t i = 0; i < n; i++) {
        const std::string at = w + ": index " + std::to_string(i);
        if (!ws[i]) throw Error(at + ": null argument");
        const Witness& v = ws[i]->w;
        if (ws[i]->params.n != params->n || ws[i]->params.k != params->k || v.s.size() != SZ || v.e.size() != SZ || v.k1.size() != SZ || v.r1is.size() != k * SZ ||
            v.r2is.size() != k * p.PZ())
            throw Error(at + ": the witness was built for other parameters");
        tabs.insert(tabs.end(), {v.s.data(), v.e.data(), v.k1.data()});
        for (size_t j = 0; j < k; j++) tabs.push_back(v.r1is.data() + j * SZ);
        tabs.push_back(v.r2is.data());
    }
    return commit_batch_tail<A>(who, ctx, sh, tabs, n, true, commitments, roots);
}

// item i's handle of an open batch: a device commitment of this field, of this context and of the shape of item 0's
template <class A>
static const pcs::Commitment* open_batch_handle(const char* who, const std::string& at, hg_ctx* ctx, const void* handle, const pcs::Commitment* first) {
    if (!handle) throw Error(at + ": null argument");
    const pcs::Commitment* cm = static_cast<const pcs::Commitment*>(handle);
    if (cm->field != A::FIELD) throw Error(at + ": " + A::other_field(who));
    if (!cm->ctx) throw Error(at + ": the commitment was made by the host form: a run is opened on device commitments only");
    if (ctx && cm->ctx != ctx) throw Error(at + ": the commitment was made on another context");
    if (first && (cm->sh.c != first->sh.c || cm->sh.nvars != first->sh.nvars)) throw Error(at + ": the commitment's shape differs from that of index 0");
    return cm;
}

// hg_pcs_open_batch* and hg_claims_open_batch* after their argument checks. `single` names the entry that opens one item: a refused
// item's reason is the text that entry leaves
template <class A>
static int pcs_open_batch_tail(const char* who, const char* single, hg_ctx* ctx, const std::vector<const pcs::Commitment*>& cms,
                               const std::vector<std::vector<typename A::PcsClaim>>& cl, size_t Q, uint8_t* openings, size_t cap_each, size_t* lens, int* status,
                               char* reasons, size_t reason_cap, bool folded = false) {
    const std::string w(who);
    const size_t n = cms.size();
    if (!n) return 0;
    size_t need = 0;
    for (size_t i = 0; i < n; i++) need = std::max(need, folded ? A::folded_opening_bytes(cms[i]->sh, Q) : A::opening_bytes(cms[i]->sh, cl[i].size(), Q));
    if (cap_each < need) throw Error(w + ": the largest opening of the run has " + std::to_string(need) + " bytes, cap_each is " + std::to_string(cap_each));
    if (!ctx) throw Error(w + ": no context");
    std::vector<typename A::PcsOpenItem> items(n);
    for (size_t i = 0; i < n; i++) items[i] = typename A::PcsOpenItem{cms[i], &cl[i]};
    std::vector<pcs::Opened> got;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: what the run costs around its device passes, on stderr
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    try {
        got = folded ? A::pcs_open_folded_batch(who, single, ctx, items, Q) : A::pcs_open_batch(who, single, ctx, items, Q);
    } catch (const std::exception& e) {
        const std::string m = e.what();
        throw Error(m.rfind(w, 0) == 0 ? m : w + ": " + m);
    }
    int refused = 0;
    const double t1 = now();
    [[maybe_unused]] const int nthr = std::max(1, std::min<int>(hg_omp_threads(), (int)n));   // (the device pass of hipcc ignores the pragmas)
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthr)
    for (long long i = 0; i < (long long)n; i++)
        if (!got[i].refused) memcpy(openings + (size_t)i * cap_each, got[i].bytes.data(), got[i].bytes.size());
    for (size_t i = 0; i < n; i++) {
        status[i] = got[i].refused ? 1 : 0;
        refused += status[i];
        lens[i] = got[i].bytes.size();
        write_reason(reasons, reason_cap, i, got[i].reason);
    }
    if (times) {
        const double t2 = now();
        std::vector<pcs::Opened>().swap(got);
        fprintf(stderr, "[hg pcs] open run of %zu items: the passes %.2f ms, the openings into the caller's buffers %.2f, their release %.2f\n", n, t1 - t0, t2 - t1, now() - t2);
    }
    return refused;
}

// hg_pcs_open_batch*: item i's claim checks are pcs_open_entry's under the name "<entry>: index i"
template <class A>
static int pcs_open_batch_entry(const char* who, const char* single, hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points,
                                const uint64_t* const* values, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens,
                                int* status, char* reasons, size_t reason_cap, bool folded = false) {
    const std::string w(who);
    if (n && (!commitments || !n_claims || !openings || !lens || !status)) throw Error(w + ": null argument");
    const size_t Q = pcs_queries(who, n_queries);
    std::vector<const pcs::Commitment*> cms(n);
    std::vector<std::vector<typename A::PcsClaim>> cl(n);
    for (size_t i = 0; i < n; i++) {
        const std::string at = w + ": index " + std::to_string(i);
        const bool has = n_claims[i] != 0;
        if (has && (!tables || !points || !values || !tables[i] || !points[i] || !values[i])) throw Error(at + ": null argument");
        cms[i] = open_batch_handle<A>(who, at, ctx, commitments[i], i ? cms[0] : nullptr);
        if (folded && !has) throw Error(at + ": a folded opening needs a claim");
        cl[i] = pcs_claims<A>(at.c_str(), cms[i]->sh, has ? tables[i] : nullptr, has ? points[i] : nullptr, has ? values[i] : nullptr, n_claims[i]);
    }
    return pcs_open_batch_tail<A>(who, single, ctx, cms, cl, Q, openings, cap_each, lens, status, reasons, reason_cap, folded);
}

// hg_claims_open_batch*: the claim and point blocks as hg_verify_public_batch* writes them, item i's under claims_open_entry's mapping;
// `mine` names the entry that makes a commitment to the secrets
template <class A>
static int claims_open_batch_entry(const char* who, const char* single, const char* mine, hg_ctx* ctx, const hg_params* params, const void* const* commitments,
                                   const void* claims, size_t claim_cap_each, const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries,
                                   size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap, bool folded = false) {
    const std::string w(who);
    if (!params || (n && (!commitments || !n_claims || !openings || !lens || !status))) throw Error(w + ": null argument");
    Params p(*params);
    const std::vector<uint32_t> nv = secrets_nvars(p);
    const size_t Q = pcs_queries(who, n_queries);
    std::vector<const pcs::Commitment*> cms(n);
    std::vector<std::vector<typename A::PcsClaim>> cl(n);
    for (size_t i = 0; i < n; i++) {
        const std::string at = w + ": index " + std::to_string(i);
        if (n_claims[i] && (!claims || !points)) throw Error(at + ": null argument");
        cms[i] = open_batch_handle<A>(who, at, ctx, commitments[i], i ? cms[0] : nullptr);
        if (cms[i]->sh.nvars.size() != nv.size() || !std::equal(nv.begin(), nv.end(), cms[i]->sh.nvars.begin(), [](uint32_t a, int b) { return (int)a == b; }))
            throw Error(at + ": the commitment is not " + mine + "'s for these parameters");
        if (folded && !n_claims[i]) throw Error(at + ": a folded opening needs a claim");
        if (n_claims[i] > claim_cap_each) throw Error(at + ": " + std::to_string(n_claims[i]) + " claims in a block of " + std::to_string(claim_cap_each));
        const typename A::Wire* in = static_cast<const typename A::Wire*>(claims) + i * claim_cap_each;
        for (size_t j = 0; j < n_claims[i]; j++)
            if (in[j].point_off > coord_cap_each || in[j].nvars > coord_cap_each - in[j].point_off)
                throw Error(at + ": claim " + std::to_string(j) + " has its point outside the block of " + std::to_string(coord_cap_each) + " coordinates");
        std::vector<uint32_t> table;
        std::vector<uint64_t> pts, vals;
        secrets_claims<A>(at.c_str(), p, in, n_claims[i], points ? points + A::WORDS * i * coord_cap_each : nullptr, table, pts, vals);
        cl[i] = pcs_claims<A>(at.c_str(), cms[i]->sh, table.data(), pts.data(), vals.data(), n_claims[i]);
    }
    return pcs_open_batch_tail<A>(who, single, ctx, cms, cl, Q, openings, cap_each, lens, status, reasons, reason_cap, folded);
}

extern "C" {

const char* hg_last_error(void) { return g_last_error.c_str(); }

int hg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

hg_ctx* hg_create(int device_id) {
    HG_TRY
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        throw Error("no HIP device available: the prover has no CPU fallback (the CPU restatement lives in oracle/ and is test-only)");
    if (device_id < 0 || device_id >= n) throw Error("device id out of range");
    hip_check(hipSetDevice(device_id), "hipSetDevice");
    hg_ctx* c = new hg_ctx();
    c->device = device_id;
    // Plain streams. Stream priorities (main high, second low) measured no better on the streams themselves (3.00-3.02 ms either
    // way) and much worse under the cached launch graph: the second and every later graph instantiated on a context replays its side
    // branch on a stream of NORMAL priority, which competes with the high-priority main branch instead of hiding under it - 5.0 ms
    // per prove instead of 3.05 (scripts/ub/repro_graph_slow.py). Removed in round 5.
    hip_check(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate");
    hip_check(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking), "hipStreamCreate");
    hip_check(hipStreamCreateWithFlags(&c->stream_col, hipStreamNonBlocking), "hipStreamCreate");
    hip_check(hipEventCreateWithFlags(&c->ev_col, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming), "hipEventCreate");
    for (auto& e : c->ev_aux) hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    c->prof_stream = c->stream;
    c->res_cap = (size_t)1 << 17;
    hip_check(hipHostMalloc((void**)&c->h_res, c->res_cap * sizeof(E2), hipHostMallocDefault), "hipHostMalloc(results)");
    // The kernels write the (≈160 KB of) result slots straight into the pinned host buffer: no device-to-host copy at the end of
    // a prove (measured -0.05 ms at n=32768 k=16).
    c->d_res = c->h_res;
    hip_check(hipMalloc((void**)&c->d_partials, dev::PARTIALS_BYTES), "hipMalloc(partials)");
    hip_check(hipMalloc((void**)&c->d_partials2, dev::PARTIALS_BYTES), "hipMalloc(partials2)");
    hip_check(hipMemset(c->d_partials, 0, dev::PARTIALS_BYTES), "hipMemset(partials)");
    hip_check(hipMemset(c->d_partials2, 0, dev::PARTIALS_BYTES), "hipMemset(partials2)");
    hip_check(hipMalloc((void**)&c->d_partials3, dev::PARTIALS_BYTES), "hipMalloc(partials3)");
    hip_check(hipMemset(c->d_partials3, 0, dev::PARTIALS_BYTES), "hipMemset(partials3)");
    hip_check(hipStreamCreateWithFlags(&c->stream_sum, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : c->ev_sum) hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipMalloc((void**)&c->d_partials4, dev::PARTIALS_BYTES), "hipMalloc(partials4)");
    hip_check(hipMemset(c->d_partials4, 0, dev::PARTIALS_BYTES), "hipMemset(partials4)");
    c->stage_cap = (size_t)4 << 20;
    hip_check(hipHostMalloc((void**)&c->h_stage, c->stage_cap, hipHostMallocDefault), "hipHostMalloc(staging)");
    c->ensure_chain(16384);
    ctx_register(c, true);
    return c;
    HG_CATCH(nullptr)
}

void hg_destroy(hg_ctx* ctx) { delete ctx; }

int hg_set_option(hg_ctx* ctx, const char* name, int64_t value) {
    HG_TRY
    if (!ctx || !name) throw Error("hg_set_option: null argument");
    const std::string n(name);
    if (n == "one_stream") { if (ctx->one_stream != (value != 0)) ctx->walk_counts.clear(); ctx->one_stream = value != 0; }
    else if (n == "graph") { ctx->use_graph = value != 0; if (!ctx->use_graph) prove_cache_drop(ctx); }
    else if (n == "gp_claims_device") {   // (a cached launch graph holds the descriptors and transcript steps of the form it was walked in)
        if (ctx->gp_claims_device != (value != 0)) { prove_cache_drop(ctx); ctx->walk_counts.clear(); }
        ctx->gp_claims_device = value != 0;
    }
    else if (n == "graph_const_tables") {   // (a cached launch graph was recorded with or without those launches)
        if (ctx->graph_const_tables != (value != 0)) { prove_cache_drop(ctx); ctx->walk_counts.clear(); }
        ctx->graph_const_tables = value != 0;
    }
    else if (n == "verify_batch_group") { if (value < 0) throw Error("hg_set_option: verify_batch_group must be >= 0"); ctx->verify_batch_group = value; }
    else if (n == "bound_batch_slice") { if (value < 0) throw Error("hg_set_option: bound_batch_slice must be >= 0"); ctx->bound_batch_slice = value; }
    else throw Error("hg_set_option: unknown option " + n);
    return 0;
    HG_CATCH(-1)
}

int hg_params_builtin(uint32_t n, uint32_t k, hg_params* out) {
    HG_TRY
    if (!params_builtin(n, k, out)) throw Error("no built-in parameter set for this (n, k)");
    return 0;
    HG_CATCH(-1)
}

static double now_ms_capi() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int hg_setup(hg_ctx* ctx, const hg_params* params, hg_pk** out) {
    HG_TRY
    if (!params || !out) throw Error("hg_setup: null argument");
    if (ctx) hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    std::unique_ptr<hg_pk> pk(new hg_pk(*params));
    static std::atomic<uint64_t> next_serial{1};
    pk->serial = next_serial++;
    pk->ctx = ctx;
    const bool times = hg_times("setup");
    const double ts0 = now_ms_capi();
    auto lap = [&](const char* what) { if (times) fprintf(stderr, "[hg setup] %8.2f ms  %s\n", now_ms_capi() - ts0, what); };
    pk->lasso = lasso_preprocess(pk->params);
    lap("lasso_preprocess");
    pk->circuit = build_circuit(pk->params, pk->lasso);
    lap("build_circuit");
    const LassoPlan& lp = pk->lasso;
    if (lp.alpha > 32 || lp.lookups.size() > 32) throw Error("lasso: more than 32 memories / lookup types");
    dev::LassoDev& L = pk->lasso_dev;
    memset(&L, 0, sizeof(L));
    L.nu = lp.nu; L.alpha = lp.alpha; L.num_lookups = (int)lp.lookups.size(); L.seg_shift = lp.seg_shift; L.rows = lp.rows;
    L.seg_lookup = upload_vec(pk.get(), lp.seg_lookup);
    for (size_t l = 0; l < lp.lookups.size(); l++) {
        int tb = lp.lookups[l].total_bits;
        L.lookup_mask[l] = tb >= 64 ? ~0ULL : ((1ULL << tb) - 1);
        L.lookup_nmems[l] = (int)lp.lookups[l].mems.size();
        if (lp.lookups[l].mems.size() > 4) throw Error("lasso: lookup touches more than C memories");
        for (size_t i = 0; i < lp.lookups[l].mems.size(); i++) {
            L.lookup_uses[l] |= 1ULL << lp.lookups[l].mems[i];
            L.lookup_mems[l][i] = lp.lookups[l].mems[i];
        }
    }
    for (int m = 0; m < lp.alpha; m++) { L.mem_dim[m] = lp.mems[m].dim; L.mem_cutoff[m] = (u32)lp.mems[m].cutoff; }
    if (lp.seg_lookup.size() > 128) throw Error("lasso: more than 128 row segments");
    for (auto& chk : lp.chunks) {
        int c = chk.first;  // counter memory = memory index c (lasso.rs:317-319)
        if (c >= 4) throw Error("lasso: chunk index exceeds C");
        for (size_t sg = 0; sg < lp.seg_lookup.size(); sg++)
            if ((L.lookup_uses[lp.seg_lookup[sg]] >> c) & 1) L.cnt_segs[c][L.cnt_nsegs[c]++] = (uint8_t)sg;
    }
    L.mpow[0] = 1;
    for (int i = 1; i < 5; i++) L.mpow[i] = gl_mul(L.mpow[i - 1], 65536);
    // circuit wiring as CSR per (node, input)
    const HCircuit& c = pk->circuit;
    pk->node_dev.resize(c.nodes.size());
    for (size_t id = 0; id < c.nodes.size(); id++) {   // twiddle tables, one per transform size and direction
        const HNode& n = c.nodes[id];
        if (n.kind == NK_FFT) {
            for (int inv = 0; inv < 2; inv++) {
                auto& tab = inv ? pk->w_inv : pk->w_fwd;
                if (tab.count(n.log2_size)) continue;
                size_t N = (size_t)1 << n.log2_size;
                std::vector<u64> W(N);
                u64 w = root_of_unity(n.log2_size);
                if (inv) w = gl_inv(w);
                W[0] = 1;
                for (size_t i = 1; i < N; i++) W[i] = gl_mul(W[i - 1], w);
                tab[n.log2_size] = upload_vec(pk.get(), W);
            }
        }
    }
    lap("twiddle tables");
    // the Vanilla nodes' wiring in the forms the kernels read, node by node on all host threads (round 6: this loop was 0.8 of the
    // 1.1 s a set-up took on eight cores): a node touches its own NodeDev only, uploads go through upload_vec's lock
    std::exception_ptr node_error;
    std::vector<size_t> by_size;
    for (size_t id = 0; id < c.nodes.size(); id++) if (c.nodes[id].kind == NK_VANILLA) by_size.push_back(id);
    std::sort(by_size.begin(), by_size.end(), [&](size_t a, size_t b) { return c.nodes[a].lin.size() + 2 * c.nodes[a].mul.size() > c.nodes[b].lin.size() + 2 * c.nodes[b].mul.size(); });
    [[maybe_unused]] const int setup_threads = std::max(1, std::min(hg_omp_threads(), 64));
#pragma omp parallel for schedule(dynamic, 1) num_threads(setup_threads)
    for (long long qi = 0; qi < (long long)by_size.size(); qi++) {
      try {
        const size_t id = by_size[(size_t)qi];
        const HNode& n = c.nodes[id];
        hg_pk::NodeDev& nd = pk->node_dev[id];
        const size_t S = (size_t)1 << n.log2_sub_in;
        nd.lin.assign(n.arity, dev::CsrLin{nullptr, nullptr, nullptr});
        nd.mulL.assign(n.arity, dev::CsrMul{nullptr, nullptr, nullptr, nullptr, nullptr});
        nd.mulR.assign(n.arity, dev::CsrMul{nullptr, nullptr, nullptr, nullptr, nullptr});
        nd.seg.assign(n.arity, hg_pk::NodeDev::Seg{});
        std::vector<std::vector<const LinTerm*>> lin_by(n.arity);
        std::vector<std::vector<const MulTerm*>> ml_by(n.arity), mr_by(n.arity);
        for (auto& t : n.lin) lin_by[t.in].push_back(&t);
        for (auto& t : n.mul) { ml_by[t.i0].push_back(&t); mr_by[t.i1].push_back(&t); }
        std::vector<std::vector<dev::GatherSeg>> segs_of(n.arity);   // run-length form per input (empty: not affine), for eq_form below
        for (int i = 0; i < n.arity; i++) {
            if (!lin_by[i].empty()) {
                std::vector<u32> ptr, gate(lin_by[i].size());
                std::vector<u64> coef(lin_by[i].size());
                build_csr<LinTerm>(lin_by[i], S, [](const LinTerm& t) { return (size_t)t.j; }, ptr,
                                   [&](const LinTerm& t, u32 at) { gate[at] = t.gate; coef[at] = t.c; });
                nd.lin[i] = dev::CsrLin{upload_vec(pk.get(), ptr), upload_vec(pk.get(), gate), upload_vec(pk.get(), coef)};
            }
            auto mk = [&](const std::vector<const MulTerm*>& ts, bool left) {
                std::vector<u32> ptr, gate(ts.size()), oin(ts.size()), oj(ts.size());
                std::vector<u64> coef(ts.size());
                build_csr<MulTerm>(ts, S, [left](const MulTerm& t) { return (size_t)(left ? t.j0 : t.j1); }, ptr,
                                   [&](const MulTerm& t, u32 at) {
                                       gate[at] = t.gate; coef[at] = t.c;
                                       oin[at] = left ? t.i1 : t.i0;
                                       oj[at] = left ? t.j1 : t.j0;
                                   });
                return dev::CsrMul{upload_vec(pk.get(), ptr), upload_vec(pk.get(), gate), upload_vec(pk.get(), coef),
                                   upload_vec(pk.get(), oin), upload_vec(pk.get(), oj)};
            };
            if (!ml_by[i].empty()) nd.mulL[i] = mk(ml_by[i], true);
            if (!mr_by[i].empty()) nd.mulR[i] = mk(mr_by[i], false);
            {   // run-length segments of the phase-1 table of input i
                struct Ent { int other_in; long long goff, joff; u64 c; u32 x; };
                std::vector<Ent> ents;
                ents.reserve(lin_by[i].size() + ml_by[i].size());
                for (const LinTerm* t : lin_by[i]) ents.push_back(Ent{-1, (long long)t->gate - (long long)t->j, 0, t->c, t->j});
                for (const MulTerm* t : ml_by[i]) ents.push_back(Ent{(int)t->i1, (long long)t->gate - (long long)t->j0, (long long)t->j1 - (long long)t->j0, t->c, t->j0});
                std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) {
                    return std::tie(a.other_in, a.goff, a.joff, a.c, a.x) < std::tie(b.other_in, b.goff, b.joff, b.c, b.x);
                });
                std::vector<dev::GatherSeg> segs;
                bool ok = !ents.empty();
                for (size_t e = 0; e < ents.size() && ok; e++) {
                    const Ent& t = ents[e];
                    if (!segs.empty()) {
                        dev::GatherSeg& g = segs.back();
                        const bool same = g.other_in == t.other_in && g.goff == (int)t.goff && g.joff == (int)t.joff && g.coef == t.c;
                        if (same && t.x == g.hi) { g.hi++; continue; }
                        if (same && t.x < g.hi) { ok = false; break; }  // the same term twice: leave it to the general form
                    }
                    if (segs.size() >= 64 || t.goff < INT32_MIN || t.goff > INT32_MAX) { ok = false; break; }
                    segs.push_back(dev::GatherSeg{t.x, t.x + 1, (int)t.goff, t.other_in, (int)t.joff, 0, t.c});
                }
                if (ok) {
                    segs_of[i] = segs;
                    hg_pk::NodeDev::Seg& sg = nd.seg[i];
                    sg.nseg = (int)segs.size();
                    sg.d = upload_vec(pk.get(), segs);
                    const dev::GatherSeg& g = segs[0];
                    sg.alias = segs.size() == 1 && g.other_in < 0 && g.coef == 1 && g.lo == 0 && g.hi == S && g.goff >= 0 &&
                               (n.log2_reps == 0 || (n.log2_sub_out == n.log2_sub_in && g.goff == 0));
                    sg.alias_off = (size_t)g.goff;
                    sg.win_lo = segs[0].lo; sg.win_hi = segs[0].hi;
                    for (auto& q : segs) { sg.win_lo = std::min<size_t>(sg.win_lo, q.lo); sg.win_hi = std::max<size_t>(sg.win_hi, q.hi); }
                }
            }
        }
        {   // eq-factored form of the node's Libra phase 1 (kernels.hpp PsJob::eq_n): no mul gates, every used input relays the same
            // aligned window [lo, lo + 2^w) of its positions onto aligned 2^w blocks of gates (any constant coefficient per block),
            // constants constant over such blocks. Table i is then kappa_i eq(z', .), kappa_i = sum_t coef_t eq(z_(w..); block_t).
            hg_pk::NodeDev::EqForm& ef = nd.eq_form;
            const int nin = n.log2_sub_in + n.log2_reps;
            bool ok = n.mul.empty() && nin <= dev::PS_EQ_MAX_VARS;
            long long lo0 = -1; int w0 = -1;
            ef.terms.assign(n.arity, {});
            int used = 0;
            for (int i = 0; i < n.arity && ok; i++) {
                if (!n.left_use[i]) continue;
                used++;
                if (segs_of[i].empty()) { ok = false; break; }
                for (const dev::GatherSeg& g : segs_of[i]) {
                    if (g.other_in >= 0) { ok = false; break; }
                    if (n.log2_reps > 0) {   // replicated sub-circuit: only the identity relay (gate = position in every repetition)
                        if (!(n.log2_sub_out == n.log2_sub_in && g.lo == 0 && g.hi == S && g.goff == 0)) { ok = false; break; }
                        if (w0 >= 0 && (lo0 != 0 || w0 != nin)) { ok = false; break; }
                        lo0 = 0; w0 = nin;
                        ef.terms[i].push_back({g.coef, 0u});
                        continue;
                    }
                    const u64 len = (u64)g.hi - g.lo;
                    const long long g0 = (long long)g.goff + (long long)g.lo;
                    if (len == 0 || (len & (len - 1)) || (g.lo & (len - 1)) || g0 < 0 || ((u64)g0 & (len - 1))) { ok = false; break; }
                    const int w = 63 - __builtin_clzll(len);
                    if (w0 >= 0 && (lo0 != (long long)g.lo || w0 != w)) { ok = false; break; }
                    lo0 = g.lo; w0 = w;
                    ef.terms[i].push_back({g.coef, (u32)((u64)g0 >> w)});
                }
            }
            if (ok && used > 0 && !n.w0.empty()) {
                if (n.log2_reps > 0) ok = false;
                // block-uniform means: EVERY gate of the block carries the constant exactly once, with one value. Counted per DISTINCT gate
                // (a wiring with two constant terms on some gates of a block and none on others has 2^w entries too)
                std::map<u32, std::pair<u64, size_t>> blocks;   // block -> (value, distinct gates seen)
                std::vector<u32> gates;
                gates.reserve(n.w0.size());
                for (auto& t : n.w0) gates.push_back(t.gate);
                std::sort(gates.begin(), gates.end());
                if (std::adjacent_find(gates.begin(), gates.end()) != gates.end()) ok = false;   // a gate with two constant terms: not the form
                for (auto& t : n.w0) {
                    if (!ok) break;
                    auto it = blocks.find(t.gate >> w0);
                    if (it == blocks.end()) blocks[t.gate >> w0] = {t.c, 1};
                    else if (it->second.first != t.c) ok = false;
                    else it->second.second++;
                }
                for (auto& kv : blocks) { if (kv.second.second != ((size_t)1 << w0)) ok = false; ef.consts.push_back({kv.second.first, kv.first}); }
            }
            ef.ok = ok && used > 0 && w0 >= 0;
            ef.w = w0; ef.hib = ef.ok ? (unsigned)((u64)lo0 >> w0) : 0;
            if (!ef.ok) { ef.terms.clear(); ef.consts.clear(); }
        }
        {   // gate-major (forward) wiring for witness generation on the device
            dev::EvalNode& f = nd.fwd;
            memset(&f, 0, sizeof(f));
            f.log2_G = n.log2_sub_out; f.log2_S = n.log2_sub_in; f.log2_R = n.log2_reps; f.num_gates = n.num_gates;
            const size_t G = n.num_gates;
            if (!n.lin.empty()) {
                std::vector<u32> ptr(G + 1, 0), in(n.lin.size()), jj(n.lin.size());
                std::vector<u64> cf(n.lin.size());
                for (auto& t : n.lin) ptr[t.gate + 1]++;
                for (size_t i = 0; i < G; i++) ptr[i + 1] += ptr[i];
                std::vector<u32> fill(ptr.begin(), ptr.end() - 1);
                for (auto& t : n.lin) { u32 at = fill[t.gate]++; in[at] = t.in; jj[at] = t.j; cf[at] = t.c; }
                f.lptr = upload_vec(pk.get(), ptr); f.lin_in = upload_vec(pk.get(), in); f.lin_j = upload_vec(pk.get(), jj); f.lcoef = upload_vec(pk.get(), cf);
            }
            if (!n.mul.empty()) {
                std::vector<u32> ptr(G + 1, 0), i0(n.mul.size()), j0(n.mul.size()), i1(n.mul.size()), j1(n.mul.size());
                std::vector<u64> cf(n.mul.size());
                for (auto& t : n.mul) ptr[t.gate + 1]++;
                for (size_t i = 0; i < G; i++) ptr[i + 1] += ptr[i];
                std::vector<u32> fill(ptr.begin(), ptr.end() - 1);
                for (auto& t : n.mul) { u32 at = fill[t.gate]++; i0[at] = t.i0; j0[at] = t.j0; i1[at] = t.i1; j1[at] = t.j1; cf[at] = t.c; }
                f.mptr = upload_vec(pk.get(), ptr); f.mi0 = upload_vec(pk.get(), i0); f.mj0 = upload_vec(pk.get(), j0);
                f.mi1 = upload_vec(pk.get(), i1); f.mj1 = upload_vec(pk.get(), j1); f.mcoef = upload_vec(pk.get(), cf);
            }
            if (!n.w0.empty()) {
                std::vector<u64> dense(G, 0);
                for (auto& t : n.w0) dense[t.gate] = gl_add(dense[t.gate], t.c);
                f.w0 = upload_vec(pk.get(), dense);
            }
        }
        if (!n.w0.empty()) {
            std::vector<u32> g;
            std::vector<u64> cf;
            for (auto& t : n.w0) { g.push_back(t.gate); cf.push_back(t.c); }
            nd.const_gate = upload_vec(pk.get(), g);
            nd.const_coef = upload_vec(pk.get(), cf);
            nd.nconst = g.size();
        }
      } catch (...) {
#pragma omp critical(hg_setup_error)
        if (!node_error) node_error = std::current_exception();
      }
    }
    if (node_error) std::rethrow_exception(node_error);
    lap("node wiring (CSR, segments, eq forms, gate-major form) built and uploaded");
    *out = pk.release();
    return 0;
    HG_CATCH(-1)
}

void hg_pk_free(hg_pk* pk) {
    if (!pk) return;
    for (void* p : pk->owned) (void)hipFree(p);
    delete pk;
}

int hg_pk_lasso_layout(const hg_pk* pk, char* out, size_t cap) {
    HG_TRY
    if (!pk || !out) throw Error("hg_pk_lasso_layout: null argument");
    std::string s = pk->lasso.layout_text();
    if (s.size() + 1 > cap) throw Error("buffer too small");
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
    HG_CATCH(-1)
}

int hg_pk_info(const hg_pk* pk, uint64_t out[6]) {
    if (!pk || !out) { g_last_error = "hg_pk_info: null argument"; return -1; }
    out[4] = (uint64_t)pk->circuit.lasso_in_id;
    out[5] = (uint64_t)pk->circuit.sum_id;
    out[0] = (uint64_t)pk->lasso.nu;
    out[1] = pk->circuit.nodes.size();
    out[2] = pk->lasso.rows;
    out[3] = (uint64_t)pk->lasso.alpha;
    return 0;
}

int hg_pk_node_eq_form(const hg_pk* pk, int node, int64_t out[6]) {
    if (!pk || !out) { g_last_error = "hg_pk_node_eq_form: null argument"; return -1; }
    if (node < 0 || (size_t)node >= pk->circuit.nodes.size()) { g_last_error = "hg_pk_node_eq_form: no such node"; return -1; }
    const HNode& n = pk->circuit.nodes[node];
    out[0] = n.kind == NK_VANILLA ? 1 : (n.kind == NK_FFT ? 2 : (n.kind == NK_LASSO ? 3 : 0));
    out[1] = out[2] = out[3] = out[4] = out[5] = 0;
    if (n.kind != NK_VANILLA) return 0;
    const hg_pk::NodeDev::EqForm& ef = pk->node_dev[node].eq_form;
    out[1] = ef.ok ? 1 : 0;
    out[2] = ef.w; out[3] = ef.hib;
    for (auto& t : ef.terms) out[4] += (int64_t)t.size();
    out[5] = n.log2_sub_in + n.log2_reps;
    return 0;
}

int hg_witness_from_json(const hg_params* params, const char* path, hg_witness** w) {
    HG_TRY
    if (!params || !path || !w) throw Error("hg_witness_from_json: null argument");
    Params p(*params);
    std::unique_ptr<hg_witness> hw(new hg_witness{witness_from_json(p, path), *params});
    *w = hw.release();
    return 0;
    HG_CATCH(-1)
}

int hg_witness_synthetic(const hg_params* params, uint64_t seed, hg_witness** w) {
    HG_TRY
    if (!params || !w) throw Error("hg_witness_synthetic: null argument");
    Params p(*params);
    std::unique_ptr<hg_witness> hw(new hg_witness{witness_synthetic(p, seed), *params});
    *w = hw.release();
    return 0;
    HG_CATCH(-1)
}

int hg_witness_from_arrays(const hg_params* params, const uint64_t* s, const uint64_t* e, const uint64_t* k1, const uint64_t* ais,
                           const uint64_t* r1is, const uint64_t* r2is, const uint64_t* ct0is, hg_witness** w) {
    HG_TRY
    if (!params || !s || !e || !k1 || !ais || !r1is || !r2is || !ct0is || !w) throw Error("hg_witness_from_arrays: null argument");
    Params p(*params);
    const size_t SZ = p.SZ(), PZ = p.PZ(), k = (size_t)p.k;
    std::unique_ptr<hg_witness> hw(new hg_witness());
    hw->params = *params;
    auto cp = [](std::vector<u64>& dst, const u64* src, size_t n) {
        dst.assign(src, src + n);
        for (u64 v : dst) if (v >= GL_P) throw Error("witness: non-canonical field element");
    };
    cp(hw->w.s, s, SZ); cp(hw->w.e, e, SZ); cp(hw->w.k1, k1, SZ);
    cp(hw->w.ais, ais, k * SZ); cp(hw->w.r1is, r1is, k * SZ); cp(hw->w.r2is, r2is, k * PZ); cp(hw->w.ct0is, ct0is, k * SZ);
    *w = hw.release();
    return 0;
    HG_CATCH(-1)
}

int hg_witness_derive(hg_ctx* ctx, const hg_params* params, const uint64_t* s, const uint64_t* e, const uint64_t* k1, const uint64_t* ais,
                      hg_witness** w) {
    HG_TRY
    if (w) *w = nullptr;
    if (!ctx) throw Error("hg_witness_derive: needs a device context (the derivation runs on the GPU and has no host fallback)");
    if (!params || !s || !e || !k1 || !ais || !w) throw Error("hg_witness_derive: null argument");
    Params p(*params);
    std::unique_ptr<hg_witness> hw(new hg_witness{witness_derive(ctx, p, s, e, k1, ais), *params});
    *w = hw.release();
    return 0;
    HG_CATCH(-1)
}

int hg_witness_derive_into(hg_ctx* ctx, const hg_pk* pk, const uint64_t* s, const uint64_t* e, const uint64_t* k1, const uint64_t* ais,
                           hg_values* v, hg_witness** w, hg_timings* timings) {
    HG_TRY
    if (w) *w = nullptr;
    if (!ctx) throw Error("hg_witness_derive_into: needs a device context (the derivation runs on the GPU and has no host fallback)");
    if (!pk || !s || !e || !k1 || !ais || !v) throw Error("hg_witness_derive_into: null argument");
    if (!pk->ctx) throw Error("hg_witness_derive_into: host-only prover key (created without a context)");
    double total = 0, gpu = 0;
    Witness host;
    witness_derive_into(ctx, pk, s, e, k1, ais, v, w ? &host : nullptr, &total, timings ? &gpu : nullptr);
    if (w) *w = new hg_witness{std::move(host), pk->params.raw};
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->witness_ms = total; timings->total_ms = total; timings->gpu_ms = gpu; }
    return 0;
    HG_CATCH(-1)
}

int64_t hg_witness_get(const hg_witness* w, int which, uint64_t* out, size_t cap) {
    if (!w) { g_last_error = "hg_witness_get: null witness"; return -1; }
    const std::vector<u64>* v = nullptr;
    switch (which) {
        case 0: v = &w->w.s; break;
        case 1: v = &w->w.e; break;
        case 2: v = &w->w.k1; break;
        case 3: v = &w->w.ais; break;
        case 4: v = &w->w.r1is; break;
        case 5: v = &w->w.r2is; break;
        case 6: v = &w->w.ct0is; break;
        default: g_last_error = "hg_witness_get: bad selector"; return -1;
    }
    if (out) memcpy(out, v->data(), std::min(cap, v->size()) * 8);
    return (int64_t)v->size();
}

void hg_witness_free(hg_witness* w) { delete w; }

int hg_witness_gen(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, hg_values** out, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !w || !out || !pk->ctx) throw Error("hg_witness_gen: needs a device context and a device prover key");
    check_witness(pk, w, "hg_witness_gen");
    double wm = 0, um = 0;
    *out = witness_gen(ctx, pk, w->w, &wm, &um);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->witness_ms = wm; timings->upload_ms = um; }
    return 0;
    HG_CATCH(-1)
}

int hg_witness_gen_into(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, hg_values* v, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !w || !v || !pk->ctx) throw Error("hg_witness_gen_into: needs a device context, a device prover key and an existing values object");
    check_witness(pk, w, "hg_witness_gen_into");
    double wm = 0, um = 0;
    witness_gen_into(ctx, pk, w->w, v, &wm, &um);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->witness_ms = wm; timings->upload_ms = um; }
    return 0;
    HG_CATCH(-1)
}

int hg_witness_gen_shard(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int rank, int world, hg_values** out, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !w || !out || !pk->ctx) throw Error("hg_witness_gen_shard: needs a device context and a device prover key");
    check_witness(pk, w, "hg_witness_gen_shard");
    double wm = 0, um = 0;
    *out = witness_gen_shard(ctx, pk, w->w, rank, world, &wm, &um);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->witness_ms = wm; timings->upload_ms = um; }
    return 0;
    HG_CATCH(-1)
}
int hg_values_info(const hg_values* v, uint64_t out[4]) {
    HG_TRY
    if (!v || !out) throw Error("hg_values_info: null argument");
    size_t n = 0;
    for (auto p : v->d_vals) n += p != nullptr;
    size_t full = v->full_bytes, res = v->resident_bytes;
    if (v->shard_rank < 0) { full = v->ct0is_len * 8; for (size_t q : v->sizes) full += q * 8; res = full; }
    out[0] = res; out[1] = full; out[2] = n; out[3] = v->d_vals.size();
    return 0;
    HG_CATCH(-1)
}

int64_t hg_values_peak_bytes(const hg_values* v) {
    if (!v) return -1;
    uint64_t info[4];
    if (hg_values_info(v, info) != 0) return -1;
    return (int64_t)(info[0] + v->cone_bytes);
}

void hg_values_free(hg_values* v) { values_free(v); }

int64_t hg_values_get(hg_ctx* ctx, const hg_values* v, int node, uint64_t* out, size_t cap) {
    HG_TRY
    if (out && !ctx) throw Error("hg_values_get: null context");
    if (!v || node < 0 || (size_t)node >= v->d_vals.size()) throw Error("hg_values_get: bad node id");
    size_t n = v->sizes[node];
    if (out && v->d_vals[node]) {
        hip_check(hipSetDevice(ctx->device), "hipSetDevice");
        hip_check(hipMemcpy(out, v->d_vals[node], std::min(cap, n) * 8, hipMemcpyDeviceToHost), "download node values");
    }
    return (int64_t)n;
    HG_CATCH(-1)
}


int hg_prove_resident(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !v || !pk->ctx) throw Error("hg_prove_resident: needs a device context, a device prover key and resident values");
    double t0 = now_ms_capi();
    ProveResult r = prove_resident(ctx, pk, v, true);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = now_ms_capi() - t0; timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms; }
    const std::vector<uint8_t>& pb = r.bytes();
    *len = pb.size();
    if (pb.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, pb.data(), pb.size());
    return 0;
    HG_CATCH(-1)
}

int hg_prove_shard_begin(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int rank, int world, uint64_t** partial, size_t* n_u64) {
    HG_TRY
    if (!ctx || !pk || !v || !pk->ctx) throw Error("hg_prove_shard_begin: needs a device context, a device prover key and resident values");
    size_t n = prove_shard_begin(ctx, pk, v, rank, world);
    *partial = reinterpret_cast<uint64_t*>(ctx->h_res);
    *n_u64 = 2 * n;
    return 0;
    HG_CATCH(-1)
}

int hg_prove_shard_combine(hg_ctx* ctx, const uint64_t* gathered, int world, size_t n_u64) {
    HG_TRY
    if (!ctx || !gathered || world < 1) throw Error("hg_prove_shard_combine: bad argument");
    prove_shard_combine(ctx, gathered, world, n_u64);
    return 0;
    HG_CATCH(-1)
}

int hg_shard_combine_host(const uint64_t* gathered, int world, size_t n_u64, uint64_t* out) {
    HG_TRY
    if (!gathered || !out || world < 1) throw Error("hg_shard_combine_host: bad argument");
    shard_combine_host(gathered, world, n_u64, out);
    return 0;
    HG_CATCH(-1)
}

int hg_prove_shard_finish(hg_ctx* ctx, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings) {
    HG_TRY
    if (!ctx) throw Error("hg_prove_shard_finish: null context");
    ProveResult r = prove_shard_finish(ctx);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = r.prove_ms; timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms; }
    *len = r.proof.size();
    if (r.proof.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, r.proof.data(), r.proof.size());
    return 0;
    HG_CATCH(-1)
}

int hg_comm_unique_id(uint8_t out[128]) {
    HG_TRY
    if (!out) throw Error("hg_comm_unique_id: null argument");
    comm_unique_id(out);
    return 0;
    HG_CATCH(-1)
}
int hg_comm_init(hg_ctx* ctx, const uint8_t id[128], int rank, int world) {
    HG_TRY
    if (!ctx || !id) throw Error("hg_comm_init: null argument");
    comm_init(ctx, id, rank, world);
    return 0;
    HG_CATCH(-1)
}
int hg_comm_destroy(hg_ctx* ctx) {
    HG_TRY
    if (!ctx) throw Error("hg_comm_destroy: null context");
    comm_destroy(ctx);
    return 0;
    HG_CATCH(-1)
}
int hg_comm_count(hg_ctx* ctx, int* ranks) {
    HG_TRY
    if (!ctx || !ranks) throw Error("hg_comm_count: null argument");
    *ranks = comm_count(ctx);
    return 0;
    HG_CATCH(-1)
}
int hg_comm_selftest(hg_ctx* ctx, const uint64_t* rank_buffers, int world, size_t n_u64, uint64_t* out) {
    HG_TRY
    if (!ctx || !rank_buffers || !out) throw Error("hg_comm_selftest: null argument");
    comm_selftest(ctx, rank_buffers, world, n_u64, out);
    return 0;
    HG_CATCH(-1)
}
int hg_prove_sharded(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !v || !pk->ctx || !proof || !len) throw Error("hg_prove_sharded: needs a device context, a device prover key and resident values");
    ProveResult r = prove_sharded(ctx, pk, v);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = r.prove_ms; timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms; }
    *len = r.proof.size();
    if (r.proof.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, r.proof.data(), r.proof.size());
    return 0;
    HG_CATCH(-1)
}

int hg_prove(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !w) throw Error("hg_prove: null argument");
    if (!pk->ctx) throw Error("hg_prove: host-only prover key (created without a context)");
    if (!proof || !len) throw Error("hg_prove: null output argument");
    check_witness(pk, w, "hg_prove");
    double t0 = now_ms_capi();
    double wm = 0, um = 0;
    // the node tables live in a values object owned by the context and are refilled in place, so the launch graph recorded for
    // them (third hg_prove with one key) proves every later witness without a protocol walk
    if (ctx->scratch_values && ctx->scratch_serial != pk->serial) { values_free(ctx->scratch_values); ctx->scratch_values = nullptr; }
    if (!ctx->scratch_values) { ctx->scratch_values = witness_gen(ctx, pk, w->w, &wm, &um); ctx->scratch_serial = pk->serial; }
    else witness_gen_into_staged(ctx, pk, w->w, ctx->scratch_values, &wm, &um);
    ProveResult r = prove_resident(ctx, pk, ctx->scratch_values, true);
    if (timings) { timings->witness_ms = wm; timings->upload_ms = um; timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = now_ms_capi() - t0; timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms; }
    const std::vector<uint8_t>& pb = r.bytes();
    *len = pb.size();
    if (pb.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, pb.data(), pb.size());
    return 0;
    HG_CATCH(-1)
}

int hg_warmup(hg_ctx* ctx, const hg_pk* pk, double* ms) {
    HG_TRY
    if (!ctx || !pk) throw Error("hg_warmup: null argument");
    if (!pk->ctx) throw Error("hg_warmup: host-only prover key (created without a context)");
    const double t = prove_warmup(ctx, pk);
    if (ms) *ms = t;
    return 0;
    HG_CATCH(-1)
}

int hg_prove_stream(hg_ctx* ctx, const hg_pk* pk, const hg_witness* const* ws, size_t n, uint8_t* proofs, size_t cap_each, size_t* lens, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || (n && (!ws || !proofs || !lens))) throw Error("hg_prove_stream: null argument");
    if (!pk->ctx) throw Error("hg_prove_stream: host-only prover key (created without a context)");
    std::vector<const Witness*> W(n);
    for (size_t i = 0; i < n; i++) {
        if (!ws[i]) throw Error("hg_prove_stream: null witness");
        check_witness(pk, ws[i], "hg_prove_stream");
        W[i] = &ws[i]->w;
    }
    double total = 0;
    std::vector<ProveResult> rs = prove_stream(ctx, pk, W, &total);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->total_ms = total; }
    for (size_t i = 0; i < n; i++) {
        lens[i] = rs[i].proof.size();
        if (rs[i].proof.size() > cap_each) throw Error("proof buffer too small");
        memcpy(proofs + i * cap_each, rs[i].proof.data(), rs[i].proof.size());
        if (timings) { timings->prove_ms += rs[i].prove_ms; timings->gpu_ms += rs[i].gpu_ms; timings->replay_ms += rs[i].replay_ms; }
    }
    return 0;
    HG_CATCH(-1)
}

int hg_encryption_layout(const hg_params* params, const int64_t* s, const int64_t* e, const int64_t* k1, const int64_t* a, uint64_t* s_t,
                         uint64_t* e_t, uint64_t* k1_t, uint64_t* ais_t) {
    HG_TRY
    if (!params || !s || !e || !k1 || !a || !s_t || !e_t || !k1_t || !ais_t) throw Error("hg_encryption_layout: null argument");
    Params p(*params);
    encryption_layout(p, s, e, k1, a, s_t, e_t, k1_t, ais_t);
    return 0;
    HG_CATCH(-1)
}

int hg_prove_encryptions(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                         const int64_t* const* a, size_t n_enc, uint8_t* proofs, size_t cap_each, size_t* lens, int* status, hg_witness** ws,
                         char* reasons, size_t reason_cap, hg_timings* timings) {
    HG_ENTRY(prove_encryptions_entry("hg_prove_encryptions", true, ctx, pk, s, e, k1, a, n_enc, proofs, cap_each, lens, status, ws, reasons, reason_cap, timings,
                                     [&](bool want, double* total) { return prove_encryptions(ctx, pk, s, e, k1, a, n_enc, want, total); }))
}

int hg_prove_encryptions_committed(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                                   const int64_t* const* a, size_t n_enc, size_t log2_row, uint8_t* proofs, size_t cap_each, size_t* lens,
                                   int* status, void** commitments, uint8_t* roots, hg_witness** ws, char* reasons, size_t reason_cap,
                                   hg_timings* timings) {
    HG_TRY
    if (commitments) for (size_t i = 0; i < n_enc; i++) commitments[i] = nullptr;
    EncCommit cmt;   // (an error of the call drops every handle made so far with it)
    return prove_encryptions_entry("hg_prove_encryptions_committed", true, ctx, pk, s, e, k1, a, n_enc, proofs, cap_each, lens, status, ws, reasons, reason_cap, timings,
                                   [&](bool want, double* total) { return prove_encryptions(ctx, pk, s, e, k1, a, n_enc, want, total, "hg_prove_encryptions_committed", &cmt); },
                                   &cmt, log2_row, commitments, roots);
    HG_CATCH(-1)
}

int hg_prove_encryptions_bn254(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                               const int64_t* const* a, size_t n_enc, uint8_t* proofs, size_t cap_each, size_t* lens, int* status, hg_witness** ws,
                               char* reasons, size_t reason_cap, hg_timings* timings) {
    HG_ENTRY(prove_encryptions_entry("hg_prove_encryptions_bn254", false, ctx, pk, s, e, k1, a, n_enc, proofs, cap_each, lens, status, ws, reasons, reason_cap, timings,
                                     [&](bool want, double* total) { return bn::prove_encryptions_bn254(ctx, pk, s, e, k1, a, n_enc, want, total); }))
}

int hg_prove_encryptions_committed_bn254(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                                         const int64_t* const* a, size_t n_enc, size_t log2_row, uint8_t* proofs, size_t cap_each, size_t* lens,
                                         int* status, void** commitments, uint8_t* roots, hg_witness** ws, char* reasons, size_t reason_cap,
                                         hg_timings* timings) {
    HG_TRY
    if (commitments) for (size_t i = 0; i < n_enc; i++) commitments[i] = nullptr;
    EncCommit cmt;   // (an error of the call drops every handle made so far with it)
    return prove_encryptions_entry("hg_prove_encryptions_committed_bn254", false, ctx, pk, s, e, k1, a, n_enc, proofs, cap_each, lens, status, ws, reasons, reason_cap,
                                   timings,
                                   [&](bool want, double* total) {
                                       return bn::prove_encryptions_bn254(ctx, pk, s, e, k1, a, n_enc, want, total, "hg_prove_encryptions_committed_bn254", &cmt);
                                   },
                                   &cmt, log2_row, commitments, roots);
    HG_CATCH(-1)
}

int hg_prove_resident_mode(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int mode, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !v || !pk->ctx || !proof || !len) throw Error("hg_prove_resident_mode: needs a device context, a device prover key and resident values");
    double t0 = now_ms_capi();
    ProveResult r = prove_resident_mode(ctx, pk, v, mode);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = now_ms_capi() - t0; timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms; }
    *len = r.proof.size();
    if (r.proof.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, r.proof.data(), r.proof.size());
    return 0;
    HG_CATCH(-1)
}
// ---- ranks of a sharded round-by-round prove ------------------------------------------------------------------------------------
struct hg_group {
    int world = 1;
    // external: the caller's all-reduce
    int (*fn)(void*, uint64_t*, size_t) = nullptr;
    void* user = nullptr;
    // local: ranks are threads of this process
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint64_t> acc, res;
    int arrived = 0;
    unsigned long long gen = 0;
    bool broken = false;
};
static int group_reduce(void* gp, uint64_t* words, size_t n) {
    hg_group* g = static_cast<hg_group*>(gp);
    if (g->fn) return g->fn(g->user, words, n);
    std::unique_lock<std::mutex> lk(g->mu);
    if (g->broken) return -1;
    if (g->arrived == 0) g->acc.assign(words, words + n);
    else {
        if (g->acc.size() != n) { g->broken = true; g->cv.notify_all(); return -1; }   // the ranks are not in the same round
        for (size_t i = 0; i < n; i++) g->acc[i] = gl_add(g->acc[i], words[i]);
    }
    if (++g->arrived == g->world) {
        g->res = g->acc;
        g->arrived = 0;
        g->gen++;
        g->cv.notify_all();
    } else {
        const unsigned long long mine = g->gen;
        // a rank that never arrives (it failed) must not hold the others for ever
        if (!g->cv.wait_for(lk, std::chrono::seconds(20), [&] { return g->gen != mine || g->broken; }) || g->broken) { g->broken = true; g->cv.notify_all(); return -1; }
    }
    std::copy(g->res.begin(), g->res.end(), words);
    return 0;
}
hg_group* hg_group_local(int world) {
    HG_TRY
    if (world < 1 || world > 64) throw Error("hg_group_local: world out of range");
    hg_group* g = new hg_group();
    g->world = world;
    return g;
    HG_CATCH(nullptr)
}
hg_group* hg_group_external(void* reduce_fn, void* user, int world) {
    HG_TRY
    if (world < 1 || !reduce_fn) throw Error("hg_group_external: needs a reduce function and a world size");
    hg_group* g = new hg_group();
    g->world = world;
    g->fn = reinterpret_cast<int (*)(void*, uint64_t*, size_t)>(reduce_fn);
    g->user = user;
    return g;
    HG_CATCH(nullptr)
}
void hg_group_free(hg_group* g) { delete g; }
int hg_prove_resident_mode_sharded(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int mode, int rank, hg_group* group, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !v || !pk->ctx || !proof || !len || !group) throw Error("hg_prove_resident_mode_sharded: needs a device context, a device prover key, resident values and a group");
    double t0 = now_ms_capi();
    ProveResult r = prove_resident_mode_sharded(ctx, pk, v, mode, rank, group->world, group_reduce, group);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = now_ms_capi() - t0; timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms; }
    *len = r.proof.size();
    if (r.proof.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, r.proof.data(), r.proof.size());
    return 0;
    HG_CATCH(-1)
}
int hg_prove_mode(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int mode, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings) {
    HG_TRY
    if (!ctx || !pk || !w || !proof || !len) throw Error("hg_prove_mode: null argument");
    if (!pk->ctx) throw Error("hg_prove_mode: host-only prover key (created without a context)");
    check_witness(pk, w, "hg_prove_mode");
    double t0 = now_ms_capi();
    double wm = 0, um = 0;
    hg_values* v = witness_gen(ctx, pk, w->w, &wm, &um);
    ProveResult r;
    try { r = prove_resident_mode(ctx, pk, v, mode); } catch (...) { values_free(v); throw; }
    values_free(v);
    if (timings) { memset(timings, 0, sizeof(*timings)); timings->witness_ms = wm; timings->upload_ms = um; timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = now_ms_capi() - t0; timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms; }
    *len = r.proof.size();
    if (r.proof.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, r.proof.data(), r.proof.size());
    return 0;
    HG_CATCH(-1)
}
int hg_verify_mode(const hg_pk* pk, const hg_witness* w, int mode, const uint8_t* proof, size_t len) {
    HG_TRY
    if (!pk || !w || !proof) throw Error("hg_verify_mode: null argument");
    if (mode < 0 || mode > 3) throw Error("hg_verify_mode: unknown mode bits");
    check_witness(pk, w, "hg_verify_mode");
    return decision(verify_proof(pk->params, pk->lasso, pk->circuit, w->w, proof, len, mode));
    HG_CATCH(-1)
}

int hg_verify(const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len) {
    HG_TRY
    if (!pk || !w || !proof) throw Error("hg_verify: null argument");
    check_witness(pk, w, "hg_verify");
    return decision(verify_proof(pk->params, pk->lasso, pk->circuit, w->w, proof, len));
    HG_CATCH(-1)
}

int hg_verify_device(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len) {
    HG_TRY
    if (!ctx || !pk || !w || !proof || !pk->ctx) throw Error("hg_verify_device: needs a device context and a device prover key");
    check_witness(pk, w, "hg_verify_device");
    return decision(verify_proof_device(ctx, pk, w->w, proof, len));
    HG_CATCH(-1)
}

int hg_verify_device_mode(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int mode, const uint8_t* proof, size_t len) {
    HG_TRY
    if (!ctx || !pk || !w || !proof || !pk->ctx) throw Error("hg_verify_device_mode: needs a device context and a device prover key");
    if (mode < 0 || mode > 3) throw Error("hg_verify_device_mode: unknown mode bits");
    check_witness(pk, w, "hg_verify_device_mode");
    return decision(verify_proof_device(ctx, pk, w->w, proof, len, mode));
    HG_CATCH(-1)
}

int hg_verify_device_batch(hg_ctx* ctx, const hg_pk* pk, const hg_witness* const* ws, const uint8_t* const* proofs, const size_t* lens, size_t n,
                           int mode, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(batch_entry<GlAbi, Witness>("hg_verify_device_batch", ctx, pk, reinterpret_cast<const void* const*>(ws), proofs, lens, n, mode, results, nullptr, 0, nullptr, 0, nullptr, reasons, reason_cap,
                                       [&](auto& W, auto& P, auto& N, auto& why, auto&) { verify_batch_device(ctx, pk, W, P, N, mode, why); }))
}

// ---- verification from the ciphertext (hg.h: hg_verify_public and what goes with it) -------------------------------------------
int hg_instance_from_ciphertext(const hg_params* params, const int64_t* a, const int64_t* ct0, void** out) {
    HG_TRY
    if (out) *out = nullptr;
    if (!params || !a || !ct0 || !out) throw Error("hg_instance_from_ciphertext: null argument");
    Params p(*params);
    std::unique_ptr<hg_instance> h(new hg_instance{instance_from_ciphertext(p, a, ct0), *params});
    *out = h.release();
    return 0;
    HG_CATCH(-1)
}

int hg_instance_from_witness(const hg_params* params, const hg_witness* w, void** out) {
    HG_TRY
    if (out) *out = nullptr;
    if (!params || !w || !out) throw Error("hg_instance_from_witness: null argument");
    Params p(*params);
    if (w->params.n != params->n || w->params.k != params->k || w->w.ais.size() != (size_t)p.k * p.SZ() || w->w.ct0is.size() != (size_t)p.k * p.SZ())
        throw Error("hg_instance_from_witness: the witness was built for other parameters");
    std::unique_ptr<hg_instance> h(new hg_instance{instance_from_witness(p, w->w), *params});
    *out = h.release();
    return 0;
    HG_CATCH(-1)
}

void hg_instance_free(void* instance) { delete static_cast<hg_instance*>(instance); }

int hg_instance_coeffs(const void* instance, int64_t* a, int64_t* ct0) {
    HG_TRY
    if (!instance || !a || !ct0) throw Error("hg_instance_coeffs: null argument");
    const Instance& in = as_instance(instance)->inst;
    memcpy(a, in.a.data(), in.a.size() * 8);
    memcpy(ct0, in.ct0.data(), in.ct0.size() * 8);
    return 0;
    HG_CATCH(-1)
}

int64_t hg_instance_get(const void* instance, int which, uint64_t* out, size_t cap) {
    HG_TRY
    if (!instance) throw Error("hg_instance_get: null instance");
    if (which != 0 && which != 1) throw Error("hg_instance_get: bad selector");
    const hg_instance* in = as_instance(instance);
    Params p(in->params);
    const size_t n = p.PZ(), SZ = p.SZ(), k = (size_t)p.k, top = which ? SZ - 2 : n - 1;
    const std::vector<int64_t>& c = which ? in->inst.ct0 : in->inst.a;
    if (out)
        for (size_t x = 0; x < std::min(cap, k * SZ); x++) {   // word w of block i: coefficient top - w where there is one, else padding
            const size_t i = x / SZ, w = x % SZ;
            const int64_t z = (w <= top && w + n > top) ? c[i * n + (top - w)] : 0;
            out[x] = z >= 0 ? (u64)z : GL_P - (u64)(-z);
        }
    return (int64_t)(k * SZ);
    HG_CATCH(-1)
}

int hg_pk_claim_shape(const hg_pk* pk, size_t* n_claims, size_t* n_coords) {
    HG_TRY
    if (!pk || !n_claims || !n_coords) throw Error("hg_pk_claim_shape: null argument");
    claim_shape(pk->params, pk->lasso, pk->circuit, n_claims, n_coords);
    return 0;
    HG_CATCH(-1)
}

int hg_verify_public(const hg_pk* pk, const void* instance, int mode, const uint8_t* proof, size_t len, void* claims, size_t claim_cap, uint64_t* points,
                     size_t coord_cap, size_t* n_claims) {
    HG_ENTRY(verify_public_entry<GlAbi>("hg_verify_public", nullptr, false, pk, instance, mode, proof, len, claims, claim_cap, points, coord_cap, n_claims))
}

int hg_verify_public_device(hg_ctx* ctx, const hg_pk* pk, const void* instance, int mode, const uint8_t* proof, size_t len, void* claims, size_t claim_cap,
                            uint64_t* points, size_t coord_cap, size_t* n_claims) {
    HG_ENTRY(verify_public_entry<GlAbi>("hg_verify_public_device", ctx, true, pk, instance, mode, proof, len, claims, claim_cap, points, coord_cap, n_claims))
}

int hg_verify_public_batch(hg_ctx* ctx, const hg_pk* pk, const void* const* instances, const uint8_t* const* proofs, const size_t* lens, size_t n, int mode,
                           int* results, void* claims, size_t claim_cap_each, uint64_t* points, size_t coord_cap_each, size_t* n_claims, char* reasons,
                           size_t reason_cap) {
    HG_ENTRY(batch_entry<GlAbi, Instance>("hg_verify_public_batch", ctx, pk, instances, proofs, lens, n, mode, results, claims, claim_cap_each, points, coord_cap_each, n_claims,
                                        reasons, reason_cap, [&](auto& I, auto& P, auto& N, auto& why, auto& open) { verify_public_batch_device(ctx, pk, I, P, N, mode, why, open); }))
}

int hg_verify_public_bound_batch(hg_ctx* ctx, const hg_pk* pk, const void* const* instances, const uint8_t* const* roots, const uint8_t* const* proofs, const size_t* lens,
                                 size_t n, int mode, int* results, void* claims, size_t claim_cap_each, uint64_t* points, size_t coord_cap_each, size_t* n_claims,
                                 uint8_t* digests, char* reasons, size_t reason_cap) {
    HG_TRY
    std::vector<uint8_t> dg;   // (an error of the call leaves digests alone)
    const int rejected = batch_entry<GlAbi, Instance>("hg_verify_public_bound_batch", ctx, pk, instances, proofs, lens, n, mode, results, claims, claim_cap_each, points,
                                                      coord_cap_each, n_claims, reasons, reason_cap, [&](auto& I, auto& P, auto& N, auto& why, auto& open) {
                                                          verify_public_bound_batch_device(ctx, pk, I, std::vector<const uint8_t*>(roots, roots + n), P, N, mode, why, open, dg);
                                                      }, true, roots);
    if (digests && !dg.empty()) memcpy(digests, dg.data(), dg.size());
    return rejected;
    HG_CATCH(-1)
}

int hg_claims_settle(hg_ctx* ctx, const hg_params* params, const hg_witness* w, const void* claims, size_t n, const uint64_t* points) {
    HG_ENTRY(claims_settle_entry<GlAbi>("hg_claims_settle", ctx, params, w, claims, n, points))
}

int hg_instance_mle(hg_ctx* ctx, const void* instance, int which, int index, const uint64_t* point, size_t nvars, uint64_t out2[2]) {
    HG_ENTRY(instance_mle_entry<GlAbi>("hg_instance_mle", false, ctx, &instance, 1, which, index, point, nvars, out2))
}

int hg_instance_mle_batch(hg_ctx* ctx, const void* const* instances, size_t n, int which, int index, const uint64_t* point, size_t nvars, uint64_t* out) {
    HG_ENTRY(instance_mle_entry<GlAbi>("hg_instance_mle_batch", true, ctx, instances, n, which, index, point, nvars, out))
}

// ---- proofs bound to the secrets' commitment and the ciphertext (hg.h: "Bound proofs") ------------------------------------------
// hg_instance_digest (batch false: instances is the one handle, ctx may be null: the host tree), hg_instance_digest_batch and
// hg_instance_digest_group (group: the digest of the bound batch, out of its staged sets)
static int instance_digest_entry(const char* who, bool batch, hg_ctx* ctx, const void* const* instances, size_t n, uint8_t* out, bool group = false) {
    const std::string w(who);
    if (batch && !n) return 0;
    if (!instances || !out) throw Error(w + ": null argument");
    if (batch && !ctx) throw Error(w + ": no context");
    std::vector<const Instance*> I(n);
    for (size_t i = 0; i < n; i++) {
        if (!instances[i]) throw Error(batch ? w + ": instance " + std::to_string(i) + ": null" : w + ": null argument");
        const hg_instance* in = as_instance(instances[i]);
        const hg_params &a = as_instance(instances[0])->params, &b = in->params;
        if (a.n != b.n || a.k != b.k || memcmp(a.qis, b.qis, sizeof(a.qis[0]) * a.k) != 0) throw Error(w + ": instances of mixed parameters (instance " + std::to_string(i) + ")");
        I[i] = &in->inst;
    }
    const Params p(as_instance(instances[0])->params);
    std::vector<uint8_t> res(32 * n);   // (an error of the call leaves out alone)
    if (!ctx) instance_digest_host(p, *I[0], res.data());
    else {
        try {
            if (group) instance_digest_group_device(ctx, p, I, res.data());
            else pcs::instance_digest_device(ctx, p, I, res.data());
        } catch (const std::exception& e) {
            throw Error(w + ": " + e.what());
        }
    }
    memcpy(out, res.data(), res.size());
    return 0;
}

int hg_instance_digest(hg_ctx* ctx, const void* instance, uint8_t out32[32]) {
    HG_ENTRY(instance_digest_entry("hg_instance_digest", false, ctx, &instance, 1, out32))
}

int hg_instance_digest_batch(hg_ctx* ctx, const void* const* instances, size_t n, uint8_t* out) {
    HG_ENTRY(instance_digest_entry("hg_instance_digest_batch", true, ctx, instances, n, out))
}

int hg_instance_digest_group(hg_ctx* ctx, const void* const* instances, size_t n, uint8_t* out) {
    HG_ENTRY(instance_digest_entry("hg_instance_digest_group", true, ctx, instances, n, out, true))
}

int hg_values_instance_digest(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, uint8_t out32[32]) {
    HG_TRY
    const std::string w = "hg_values_instance_digest";
    if (!pk || !v || !out32) throw Error(w + ": null argument");
    check_values_of(w, ctx, pk, v);
    const pcs::DigestMember mem = values_public_tables(w, pk, v);
    uint8_t res[32];
    try {
        pcs::instance_digest_values(ctx, pk->params, mem, res);
    } catch (const std::exception& e) {
        throw Error(w + ": " + e.what());
    }
    memcpy(out32, res, 32);
    return 0;
    HG_CATCH(-1)
}

int hg_bound_seed(const hg_params* params, int mode, const uint8_t digest32[32], const uint8_t root32[32], uint8_t* out, size_t cap, size_t* len) {
    HG_TRY
    const std::string w = "hg_bound_seed";
    if (len) *len = 0;
    if (!params || !digest32 || !root32 || !len) throw Error(w + ": null argument");
    check_bound_mode(w, mode);
    try {
        Params p(*params);
    } catch (const std::exception& e) {
        throw Error(w + ": " + e.what());
    }
    const std::vector<uint8_t> s = bound_seed(*params, mode, digest32, root32);
    *len = s.size();
    if (!out || s.size() > cap) throw Error(w + ": buffer too small (" + std::to_string(s.size()) + " bytes)");
    memcpy(out, s.data(), s.size());
    return 0;
    HG_CATCH(-1)
}

int hg_prove_committed_mode(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int mode, size_t log2_row, uint8_t* proof, size_t cap, size_t* len, void** commitment,
                            uint8_t root[32], hg_timings* timings) {
    HG_TRY
    const std::string w = "hg_prove_committed_mode";
    if (commitment) *commitment = nullptr;
    if (len) *len = 0;
    check_bound_mode(w, mode);
    const double t0 = now_ms_capi();
    void* h = nullptr;
    uint8_t rt[32];
    pcs::DigestJob dg;
    secrets_commit_values_entry(w.c_str(), ctx, pk, v, log2_row, commitment ? &h : nullptr, root ? rt : nullptr, &dg);
    std::unique_ptr<pcs::Commitment> cm(static_cast<pcs::Commitment*>(h));   // (an error below drops the handle with it)
    if (!proof || !len) throw Error(w + ": null argument");
    const double t1 = now_ms_capi();
    ProveResult r;
    try {
        r = prove_resident_mode(ctx, pk, v, mode, bound_seed(pk->params.raw, mode, dg.digest, rt));
    } catch (const std::exception& e) {
        throw Error(w + ": " + e.what());
    }
    *len = r.proof.size();
    if (r.proof.size() > cap) throw Error(w + ": proof buffer too small (" + std::to_string(r.proof.size()) + " bytes)");
    memcpy(proof, r.proof.data(), r.proof.size());
    if (timings) {   // as hg_prove_resident_mode; upload_ms: the commit and the digest
        memset(timings, 0, sizeof(*timings));
        timings->upload_ms = t1 - t0; timings->prove_ms = r.prove_ms; timings->gpu_ms = r.gpu_ms; timings->total_ms = now_ms_capi() - t0;
        timings->enqueue_ms = r.enqueue_ms; timings->sync_ms = r.sync_ms; timings->replay_ms = r.replay_ms;
    }
    memcpy(root, rt, 32);
    *commitment = cm.release();
    return 0;
    HG_CATCH(-1)
}

int hg_verify_public_bound(const hg_pk* pk, const void* instance, int mode, const uint8_t root[32], const uint8_t* proof, size_t len, void* claims, size_t claim_cap,
                           uint64_t* points, size_t coord_cap, size_t* n_claims) {
    HG_ENTRY(verify_public_entry<GlAbi>("hg_verify_public_bound", nullptr, false, pk, instance, mode, proof, len, claims, claim_cap, points, coord_cap, n_claims, true, root))
}

int hg_verify_public_bound_device(hg_ctx* ctx, const hg_pk* pk, const void* instance, int mode, const uint8_t root[32], const uint8_t* proof, size_t len, void* claims,
                                  size_t claim_cap, uint64_t* points, size_t coord_cap, size_t* n_claims) {
    HG_ENTRY(verify_public_entry<GlAbi>("hg_verify_public_bound_device", ctx, true, pk, instance, mode, proof, len, claims, claim_cap, points, coord_cap, n_claims, true, root))
}

int hg_verify_bn254(const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len) {
    HG_TRY
    if (!pk || !w || !proof) throw Error("hg_verify_bn254: null argument");
    check_witness(pk, w, "hg_verify_bn254");
    return decision(verify_proof_bn254(pk->params, pk->lasso, pk->circuit, w->w, proof, len));
    HG_CATCH(-1)
}

int hg_verify_device_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len) {
    HG_TRY
    if (!ctx || !pk || !w || !proof || !pk->ctx) throw Error("hg_verify_device_bn254: needs a device context and a device prover key");
    check_witness(pk, w, "hg_verify_device_bn254");
    return decision(hg::bn::verify_proof_device_bn254(ctx, pk, w->w, proof, len));
    HG_CATCH(-1)
}

int hg_verify_device_batch_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* const* ws, const uint8_t* const* proofs, const size_t* lens, size_t n,
                                 int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(batch_entry<BnAbi, Witness>("hg_verify_device_batch_bn254", ctx, pk, reinterpret_cast<const void* const*>(ws), proofs, lens, n, 0, results, nullptr, 0, nullptr, 0, nullptr, reasons, reason_cap,
                                       [&](auto& W, auto& P, auto& N, auto& why, auto&) { hg::bn::verify_batch_device_bn254(ctx, pk, W, P, N, why); }))
}

// ---- verification from the ciphertext over bn256::Fr (hg.h: hg_verify_public_bn254 and what goes with it) -------------------------
int hg_verify_public_bn254(const hg_pk* pk, const void* instance, const uint8_t* proof, size_t len, void* claims, size_t claim_cap, uint64_t* points4,
                           size_t coord_cap, size_t* n_claims) {
    HG_ENTRY(verify_public_entry<BnAbi>("hg_verify_public_bn254", nullptr, false, pk, instance, 0, proof, len, claims, claim_cap, points4, coord_cap, n_claims))
}

int hg_verify_public_device_bn254(hg_ctx* ctx, const hg_pk* pk, const void* instance, const uint8_t* proof, size_t len, void* claims, size_t claim_cap,
                                  uint64_t* points4, size_t coord_cap, size_t* n_claims) {
    HG_ENTRY(verify_public_entry<BnAbi>("hg_verify_public_device_bn254", ctx, true, pk, instance, 0, proof, len, claims, claim_cap, points4, coord_cap, n_claims))
}

int hg_verify_public_batch_bn254(hg_ctx* ctx, const hg_pk* pk, const void* const* instances, const uint8_t* const* proofs, const size_t* lens, size_t n,
                                 int* results, void* claims, size_t claim_cap_each, uint64_t* points4, size_t coord_cap_each, size_t* n_claims, char* reasons,
                                 size_t reason_cap) {
    HG_ENTRY(batch_entry<BnAbi, Instance>("hg_verify_public_batch_bn254", ctx, pk, instances, proofs, lens, n, 0, results, claims, claim_cap_each, points4, coord_cap_each, n_claims,
                                        reasons, reason_cap, [&](auto& I, auto& P, auto& N, auto& why, auto& open) { hg::bn::verify_public_batch_device_bn254(ctx, pk, I, P, N, why, open); }))
}

int hg_claims_settle_bn254(hg_ctx* ctx, const hg_params* params, const hg_witness* w, const void* claims, size_t n, const uint64_t* points4) {
    HG_ENTRY(claims_settle_entry<BnAbi>("hg_claims_settle_bn254", ctx, params, w, claims, n, points4))
}

int hg_instance_mle_bn254(hg_ctx* ctx, const void* instance, int which, int index, const uint64_t* point4, size_t nvars, uint64_t out4[4]) {
    HG_ENTRY(instance_mle_entry<BnAbi>("hg_instance_mle_bn254", false, ctx, &instance, 1, which, index, point4, nvars, out4))
}

int hg_instance_mle_batch_bn254(hg_ctx* ctx, const void* const* instances, size_t n, int which, int index, const uint64_t* point4, size_t nvars, uint64_t* out4) {
    HG_ENTRY(instance_mle_entry<BnAbi>("hg_instance_mle_batch_bn254", true, ctx, instances, n, which, index, point4, nvars, out4))
}

int hg_circuit_eval(const hg_pk* pk, const hg_witness* w, uint64_t* lasso_in, size_t lasso_cap, uint64_t* sum_out, size_t sum_cap) {
    HG_TRY
    if (!pk || !w) throw Error("hg_circuit_eval: null argument");
    check_witness(pk, w, "hg_circuit_eval");
    auto vals = circuit_evaluate(pk->circuit, pk->params, w->w);
    const auto& li = vals[pk->circuit.lasso_in_id];
    const auto& so = vals[pk->circuit.sum_id];
    if (lasso_in) { if (li.size() > lasso_cap) throw Error("lasso_in buffer too small"); memcpy(lasso_in, li.data(), li.size() * 8); }
    if (sum_out) { if (so.size() > sum_cap) throw Error("sum_out buffer too small"); memcpy(sum_out, so.data(), so.size() * 8); }
    return 0;
    HG_CATCH(-1)
}

int hg_lasso_prove(hg_ctx* ctx, const hg_pk* pk, const uint64_t* lasso_in, uint8_t* proof, size_t cap, size_t* len, uint64_t* claim_out) {
    return hg_lasso_prove_at(ctx, pk, lasso_in, 0, proof, cap, len, claim_out);
}

int hg_lasso_prove_at(hg_ctx* ctx, const hg_pk* pk, const uint64_t* lasso_in, size_t chain_skip, uint8_t* proof, size_t cap, size_t* len,
                      uint64_t* claim_out) {
    HG_TRY
    if (!ctx || !pk || !pk->ctx) throw Error("hg_lasso_prove: needs a device context and a device prover key");
    if (!lasso_in || !proof || !len) throw Error("hg_lasso_prove: null argument");
    std::vector<E2> claim;
    std::vector<uint8_t> pr = prove_lasso_node(ctx, pk, lasso_in, chain_skip, &claim);
    *len = pr.size();
    if (pr.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, pr.data(), pr.size());
    if (claim_out) for (size_t i = 0; i < claim.size(); i++) { claim_out[2 * i] = claim[i].c0; claim_out[2 * i + 1] = claim[i].c1; }
    return 0;
    HG_CATCH(-1)
}

int hg_lasso_num_challenges(const hg_pk* pk, size_t* n_e) {
    HG_TRY
    if (!pk || !n_e) throw Error("hg_lasso_num_challenges: null argument");
    // r: nu; collation rounds: nu; gamma, tau: 2; a grand product over 2^v entries: mu of layer 0, then per layer j = 1..v-1
    // one batching challenge, j round challenges and mu (lasso.rs:85-111, prover.rs:183-266)
    auto gp = [](size_t v) { size_t c = 1; for (size_t j = 1; j < v; j++) c += 2 + j; return c; };
    const size_t nu = (size_t)pk->lasso.nu;
    *n_e = nu + nu + 2 + gp(nu) + gp(16);
    return 0;
    HG_CATCH(-1)
}

int hg_sumcheck(hg_ctx* ctx, int kind, size_t nv, size_t ntab, const uint64_t* const* tables, const int* is_base, const uint64_t* pw,
                size_t npw, const uint64_t* claim2, size_t chain_skip, uint64_t* msgs, uint64_t* point, uint64_t* evals, uint64_t* sums) {
    HG_TRY
    if (!ctx || !tables || !is_base || !claim2 || (npw && !pw)) throw Error("hg_sumcheck: null argument (a HIP device is required)");
    if (ntab == 0 || nv == 0 || nv > 30) throw Error("hg_sumcheck: bad shape");
    // everything the kernels cannot do is refused here, on the host, before anything is uploaded or launched
    if (kind < 0 || kind > 2) throw Error("hg_sumcheck: kind must be 0 (collation), 1 (grand product) or 2 (prodsum)");
    if (kind != 0 && (ntab & 1)) throw Error("hg_sumcheck: kinds 1 and 2 take an even number of tables (pairs)");
    const size_t max_tab = kind == 0 ? (size_t)dev::PW_ENTRY_MAX : kind == 1 ? 2 * (size_t)dev::PW_ENTRY_MAX : 2 * (size_t)dev::PS_MAX_PAIRS;
    if (ntab > max_tab) throw Error("hg_sumcheck: kind " + std::to_string(kind) + " carries at most " + std::to_string(max_tab) + " tables");
    const size_t need_pw = kind == 0 ? ntab : kind == 1 ? ntab / 2 : 0;
    if (npw < need_pw) throw Error("hg_sumcheck: kind " + std::to_string(kind) + " with " + std::to_string(ntab) + " tables needs " + std::to_string(need_pw) + " powers");
    for (size_t i = 0; i < ntab; i++) {
        if (!tables[i]) throw Error("hg_sumcheck: null table");
        if (kind == 2 ? (is_base[i] != 0) != (i % 2 == 0) : (is_base[i] != 0) != (is_base[0] != 0))
            throw Error(kind == 2 ? "hg_sumcheck: prodsum expects (base, ext) table pairs" : "hg_sumcheck: mixed table fields");
    }
    if (claim2[0] >= GL_P || claim2[1] >= GL_P) throw Error("hg_sumcheck: non-canonical claim");
    for (size_t i = 0; i < 2 * npw; i++) if (pw[i] >= GL_P) throw Error("hg_sumcheck: non-canonical power");
    for (size_t i = 0; i < ntab; i++) {
        const size_t words = (is_base[i] ? (size_t)1 : (size_t)2) << nv;
        for (size_t j = 0; j < words; j++) if (tables[i][j] >= GL_P) throw Error("hg_sumcheck: non-canonical entry in table " + std::to_string(i));
    }
    SumcheckIO io;
    io.kind = kind; io.nv = nv; io.chain_skip = chain_skip;
    io.tables.assign(tables, tables + ntab);
    io.is_base.assign(is_base, is_base + ntab);
    for (size_t i = 0; i < npw; i++) io.pw.push_back(e2(pw[2 * i], pw[2 * i + 1]));
    io.claim = e2(claim2[0], claim2[1]);
    sumcheck_on_tables(ctx, io);
    auto put = [](uint64_t* dst, const std::vector<E2>& v) { if (dst) for (size_t i = 0; i < v.size(); i++) { dst[2 * i] = v[i].c0; dst[2 * i + 1] = v[i].c1; } };
    put(msgs, io.msgs); put(point, io.point); put(evals, io.evals); put(sums, io.sums);
    return 0;
    HG_CATCH(-1)
}

int hg_prodsum_jobs(hg_ctx* ctx, size_t njobs, const size_t* nv, const size_t* npairs, const uint64_t* const* tables, const size_t* eq4,
                    const uint64_t* kappa2, size_t chain_skip, uint64_t* sums2, uint64_t* evals2) {
    HG_TRY
    if (!ctx) throw Error("hg_prodsum_jobs: null argument (a HIP device is required)");
    prodsum_jobs(ctx, njobs, nv, npairs, tables, eq4, kappa2, chain_skip, sums2, evals2);
    return 0;
    HG_CATCH(-1)
}
int hg_claim_tables_eq(hg_ctx* ctx, size_t njobs, const size_t* n, const size_t* nclaims, const size_t* point_off, const size_t* alpha_off,
                       uint64_t* const* out) {
    HG_TRY
    if (!ctx) throw Error("hg_claim_tables_eq: null argument (a HIP device is required)");
    claim_tables_eq(ctx, njobs, n, nclaims, point_off, alpha_off, out);
    return 0;
    HG_CATCH(-1)
}
int hg_claim_tables_fft(hg_ctx* ctx, size_t njobs, const size_t* L, const int* inverse, const size_t* nclaims, const size_t* point_off,
                        const size_t* alpha_off, uint64_t* const* out) {
    HG_TRY
    if (!ctx) throw Error("hg_claim_tables_fft: null argument (a HIP device is required)");
    claim_tables_fft(ctx, njobs, L, inverse, nclaims, point_off, alpha_off, out);
    return 0;
    HG_CATCH(-1)
}

int hg_grand_product(hg_ctx* ctx, size_t nb, size_t len, const uint64_t* const* tables, size_t chain_skip, uint8_t* proof, size_t cap,
                     size_t* proof_len, uint64_t* claims2, uint64_t* point2) {
    HG_TRY
    if (!ctx || !tables || !proof || !proof_len) throw Error("hg_grand_product: null argument (a HIP device is required)");
    std::vector<E2> claims, point;
    std::vector<uint8_t> bytes = grand_product_on_tables(ctx, nb, len, tables, chain_skip, &claims, &point);
    *proof_len = bytes.size();
    if (bytes.size() > cap) throw Error("proof buffer too small");
    memcpy(proof, bytes.data(), bytes.size());
    if (claims2) for (size_t i = 0; i < claims.size(); i++) { claims2[2 * i] = claims[i].c0; claims2[2 * i + 1] = claims[i].c1; }
    if (point2) for (size_t i = 0; i < point.size(); i++) { point2[2 * i] = point[i].c0; point2[2 * i + 1] = point[i].c1; }
    return 0;
    HG_CATCH(-1)
}
// the kernel-level entries take canonical words (hg.h): the first word that is not below p refuses the call
static void require_canonical(const char* entry, const char* what, const uint64_t* v, size_t words) {
    for (size_t i = 0; i < words; i++)
        if (v[i] >= GL_P) throw Error(std::string(entry) + ": non-canonical " + what + " (word " + std::to_string(i) + ")");
}
int hg_fold(hg_ctx* ctx, const uint64_t* table, size_t nv, int is_base, const uint64_t r2[2], uint64_t* out) {
    HG_TRY
    if (!ctx || !table || !r2 || !out) throw Error("hg_fold: null argument (a HIP device is required)");
    if (nv < 1 || nv > 30) throw Error("hg_fold: table size out of range");
    if (r2[0] >= GL_P || r2[1] >= GL_P) throw Error("hg_fold: non-canonical r");
    require_canonical("hg_fold", "table entry", table, (is_base ? (size_t)1 : (size_t)2) << nv);
    fold_device(ctx, table, nv, is_base != 0, e2(r2[0], r2[1]), reinterpret_cast<E2*>(out));
    return 0;
    HG_CATCH(-1)
}
int hg_params_derive(uint32_t n, uint32_t k, const uint64_t* qis, uint64_t t, hg_params* out) {
    HG_TRY
    if (!qis || !out) throw Error("hg_params_derive: null argument");
    params_derive(n, k, qis, t, out);
    return 0;
    HG_CATCH(-1)
}

int hg_mle_eval(hg_ctx* ctx, const uint64_t* table, size_t nv, const uint64_t* point, uint64_t out2[2]) {
    HG_TRY
    if (!ctx || !table || (nv && !point) || !out2) throw Error("hg_mle_eval: null argument (a HIP device is required)");
    if (nv > 30) throw Error("hg_mle_eval: table size out of range");
    require_canonical("hg_mle_eval", "point coordinate", point, 2 * nv);
    require_canonical("hg_mle_eval", "table entry", table, (size_t)1 << nv);
    std::vector<E2> pt(nv);
    for (size_t i = 0; i < nv; i++) pt[i] = e2(point[2 * i], point[2 * i + 1]);
    E2 v = mle_eval_device(ctx, table, nv, pt.data());
    out2[0] = v.c0; out2[1] = v.c1;
    return 0;
    HG_CATCH(-1)
}

int hg_ntt(hg_ctx* ctx, const uint64_t* in, size_t log2n, int inverse, size_t batch, uint64_t* out) {
    HG_TRY
    if (!ctx || !in || !out) throw Error("hg_ntt: null argument (a HIP device is required)");
    if (log2n < 1 || log2n > 32) throw Error("hg_ntt: size out of range");
    if (batch == 0) throw Error("hg_ntt: empty batch");
    if (log2n >= 8 && log2n <= 16 && batch > 65535) throw Error("hg_ntt: more than 65535 transforms in one four-step batch");
    if (batch > (SIZE_MAX >> 4 >> log2n)) throw Error("hg_ntt: batch out of range");
    require_canonical("hg_ntt", "input word", in, batch << log2n);
    ntt_device(ctx, in, (int)log2n, inverse != 0, batch, out);
    return 0;
    HG_CATCH(-1)
}

int hg_challenges(size_t n, uint64_t* out) {
    HG_TRY
    if (!out) throw Error("hg_challenges: null argument");
    const u64* c = challenge_chain(n);
    memcpy(out, c, n * 8);
    return 0;
    HG_CATCH(-1)
}

int hg_challenges_bn254(size_t n, uint64_t* out4) {
    HG_TRY
    hg::bn::challenges_bn254_raw(n, out4);
    return 0;
    HG_CATCH(-1)
}
int hg_bn254_field_op(hg_ctx* ctx, int op, size_t n, const uint64_t* a4, const uint64_t* b4, uint64_t* out4) {
    HG_TRY
    if (!ctx) throw hg::Error("hg_bn254_field_op: no context (a HIP device is required)");
    hg::bn::field_op_bn254(ctx, op, n, a4, b4, out4);
    return 0;
    HG_CATCH(-1)
}
int hg_sumcheck_bn254(hg_ctx* ctx, int kind, size_t nv, size_t ntab, const uint64_t* const* tables, const uint64_t* pw4, size_t npw,
                      const uint64_t* claim4, size_t chain_skip, uint64_t* msgs, uint64_t* point, uint64_t* evals, uint64_t* sums) {
    HG_TRY
    if (!ctx) throw hg::Error("hg_sumcheck_bn254: no context (a HIP device is required)");
    hg::bn::sumcheck_bn254(ctx, kind, nv, ntab, tables, pw4, npw, claim4, chain_skip, msgs, point, evals, sums);
    return 0;
    HG_CATCH(-1)
}
int hg_prodsum_jobs_bn254(hg_ctx* ctx, size_t njobs, const size_t* nv, const size_t* npairs, const uint64_t* const* tables, const size_t* win, size_t chain_skip,
                          uint64_t* sums4, uint64_t* evals4) {
    HG_TRY
    if (!ctx) throw hg::Error("hg_prodsum_jobs_bn254: no context (a HIP device is required)");
    hg::bn::prodsum_jobs_bn254(ctx, njobs, nv, npairs, tables, win, chain_skip, sums4, evals4);
    return 0;
    HG_CATCH(-1)
}

int hg_grand_product_bn254(hg_ctx* ctx, size_t nb, size_t len, const uint64_t* const* tables, size_t chain_skip, uint8_t* proof, size_t cap,
                           size_t* proof_len, uint64_t* claims4, uint64_t* point4) {
    HG_TRY
    if (!ctx) throw hg::Error("hg_grand_product_bn254: no context (a HIP device is required)");
    std::vector<uint8_t> bytes;
    ctx->arena_reset();
    hg::bn::grand_product_bn254(ctx, nb, len, tables, chain_skip, bytes, claims4, point4);
    *proof_len = bytes.size();
    if (bytes.size() > cap) throw hg::Error("proof buffer too small");
    memcpy(proof, bytes.data(), bytes.size());
    return 0;
    HG_CATCH(-1)
}
int hg_lasso_prove_bn254(hg_ctx* ctx, const hg_pk* pk, const uint64_t* lasso_in4, size_t chain_skip, uint8_t* proof, size_t cap, size_t* len,
                         uint64_t* claim_out4) {
    HG_TRY
    if (!ctx || !pk) throw hg::Error("hg_lasso_prove_bn254: null argument (a HIP device is required)");
    std::vector<uint8_t> bytes;
    ctx->arena_reset();
    hg::bn::lasso_prove_bn254(ctx, pk, lasso_in4, chain_skip, bytes, claim_out4);
    *len = bytes.size();
    if (bytes.size() > cap) throw hg::Error("proof buffer too small");
    memcpy(proof, bytes.data(), bytes.size());
    return 0;
    HG_CATCH(-1)
}
int hg_witness_from_json_bn254(const hg_params* params, const char* path, hg_witness** out) {
    HG_TRY
    if (!params || !path || !out) throw hg::Error("hg_witness_from_json_bn254: null argument");
    std::unique_ptr<hg_witness> w(new hg_witness());
    w->params = *params;
    w->w = hg::witness_from_json_bn254(hg::Params(*params), path);
    *out = w.release();
    return 0;
    HG_CATCH(-1)
}
int hg_circuit_eval_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int which, uint64_t* out4, size_t cap_elems, size_t* n_elems) {
    HG_TRY
    if (!ctx || !pk || !w || !n_elems) throw hg::Error("hg_circuit_eval_bn254: null argument (a HIP device is required)");
    check_witness(pk, w, "hg_circuit_eval_bn254");
    std::vector<uint64_t> v;
    hg::bn::circuit_eval_bn254(ctx, pk, w->w, which, v);
    *n_elems = v.size() / 4;
    if (v.size() / 4 > cap_elems) throw hg::Error("hg_circuit_eval_bn254: output buffer too small");
    memcpy(out4, v.data(), v.size() * 8);
    return 0;
    HG_CATCH(-1)
}
int hg_prove_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, uint8_t* proof, size_t cap, size_t* len, double* ms2) {
    HG_TRY
    if (!ctx || !pk || !w || !len) throw hg::Error("hg_prove_bn254: null argument (a HIP device is required)");
    check_witness(pk, w, "hg_prove_bn254");
    std::vector<uint8_t> bytes;
    hg::bn::prove_bn254(ctx, pk, w->w, bytes, ms2);
    *len = bytes.size();
    if (bytes.size() > cap) throw hg::Error("proof buffer too small");
    memcpy(proof, bytes.data(), bytes.size());
    return 0;
    HG_CATCH(-1)
}
int hg_mle_eval_bn254(hg_ctx* ctx, const uint64_t* table4, size_t nv, const uint64_t* point4, uint64_t out4[4]) {
    HG_TRY
    if (!ctx || !table4 || (nv && !point4) || !out4) throw hg::Error("hg_mle_eval_bn254: null argument (a HIP device is required)");
    hg::bn::mle_eval_bn254(ctx, table4, nv, point4, out4);
    return 0;
    HG_CATCH(-1)
}
int hg_ntt_bn254(hg_ctx* ctx, const uint64_t* in4, size_t log2n, int inverse, size_t batch, uint64_t* out4) {
    HG_TRY
    if (!ctx || !in4 || !out4) throw hg::Error("hg_ntt_bn254: null argument (a HIP device is required)");
    hg::bn::ntt_bn254(ctx, in4, log2n, inverse != 0, batch, out4);
    return 0;
    HG_CATCH(-1)
}

// ---- polynomial commitment: the entries (their bodies: pcs_open_entry .. claims_verify_entry of the shared layer)
int hg_pcs_commit(hg_ctx* ctx, const uint64_t* const* tables, const uint32_t* nvars, size_t n_tables, size_t log2_row, void** commitment, uint8_t root[32]) {
    HG_TRY
    if (commitment) *commitment = nullptr;
    if (!tables || !nvars || !commitment || !root) throw Error("hg_pcs_commit: null argument");
    const pcs::Shape sh = pcs::make_shape("hg_pcs_commit", nvars, n_tables, log2_row);
    for (size_t t = 0; t < n_tables; t++) if (!tables[t]) throw Error("hg_pcs_commit: null table " + std::to_string(t));
    pcs::Commitment* cm = ctx ? pcs::commit_device(ctx, sh, tables) : pcs::commit_host(sh, tables);
    memcpy(root, cm->root(), 32);
    *commitment = cm;
    return 0;
    HG_CATCH(-1)
}

void hg_pcs_free(void* commitment) { delete static_cast<pcs::Commitment*>(commitment); }

int hg_pcs_open(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims, size_t n_queries,
                uint8_t* proof, size_t cap, size_t* len) {
    HG_ENTRY(pcs_open_api<GlAbi>("hg_pcs_open", ctx, commitment, table, points, values, n_claims, n_queries, proof, cap, len))
}

int hg_pcs_verify(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points,
                  const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_entry<GlAbi>("hg_pcs_verify", false, nullptr, root, nvars, n_tables, log2_row, table, points, values, n_claims, n_queries, proof, len))
}

int hg_pcs_verify_device(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points,
                         const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_entry<GlAbi>("hg_pcs_verify_device", true, ctx, root, nvars, n_tables, log2_row, table, points, values, n_claims, n_queries, proof, len))
}

int hg_secrets_commit(hg_ctx* ctx, const hg_params* params, const hg_witness* w, size_t log2_row, void** commitment, uint8_t root[32]) {
    HG_ENTRY(secrets_commit_entry<GlAbi>("hg_secrets_commit", ctx, params, w, log2_row, commitment, root))
}

int hg_claims_open(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points, size_t n_queries,
                   uint8_t* opening, size_t cap, size_t* len) {
    HG_ENTRY(claims_open_entry<GlAbi>("hg_claims_open", "hg_secrets_commit", ctx, params, commitment, claims, n, points, n_queries, opening, cap, len))
}

int hg_claims_verify(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points,
                     size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<GlAbi>("hg_claims_verify", false, nullptr, params, root, log2_row, claims, n, points, n_queries, opening, len))
}

int hg_claims_verify_device(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points,
                            size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<GlAbi>("hg_claims_verify_device", true, ctx, params, root, log2_row, claims, n, points, n_queries, opening, len))
}

int hg_pcs_open_folded(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims, size_t n_queries,
                       uint8_t* proof, size_t cap, size_t* len) {
    HG_ENTRY(pcs_open_folded_api<GlAbi>("hg_pcs_open_folded", ctx, commitment, table, points, values, n_claims, n_queries, proof, cap, len))
}
int hg_pcs_verify_folded(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points,
                         const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_folded_entry<GlAbi>("hg_pcs_verify_folded", false, nullptr, root, nvars, n_tables, log2_row, table, points, values, n_claims, n_queries, proof, len))
}
int hg_pcs_verify_folded_device(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points,
                                const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_folded_entry<GlAbi>("hg_pcs_verify_folded_device", true, ctx, root, nvars, n_tables, log2_row, table, points, values, n_claims, n_queries, proof, len))
}
int hg_claims_open_folded(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points, size_t n_queries,
                          uint8_t* opening, size_t cap, size_t* len) {
    HG_ENTRY(claims_open_entry<GlAbi>("hg_claims_open_folded", "hg_secrets_commit", ctx, params, commitment, claims, n, points, n_queries, opening, cap, len, true))
}
int hg_claims_verify_folded(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points,
                            size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<GlAbi>("hg_claims_verify_folded", false, nullptr, params, root, log2_row, claims, n, points, n_queries, opening, len, true))
}
int hg_claims_verify_folded_device(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points,
                                   size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<GlAbi>("hg_claims_verify_folded_device", true, ctx, params, root, log2_row, claims, n, points, n_queries, opening, len, true))
}

int hg_pcs_open_folded_batch(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points, const uint64_t* const* values,
                             const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap) {
    HG_ENTRY(pcs_open_batch_entry<GlAbi>("hg_pcs_open_folded_batch", "hg_pcs_open_folded", ctx, commitments, tables, points, values, n_claims, n_queries, n, openings, cap_each, lens,
                                         status, reasons, reason_cap, true))
}
int hg_claims_open_folded_batch(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each, const uint64_t* points,
                                size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status,
                                char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_open_batch_entry<GlAbi>("hg_claims_open_folded_batch", "hg_claims_open_folded", "hg_secrets_commit", ctx, params, commitments, claims, claim_cap_each, points,
                                            coord_cap_each, n_claims, n_queries, n, openings, cap_each, lens, status, reasons, reason_cap, true))
}
int hg_pcs_verify_folded_device_batch(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* const* tables,
                                      const uint64_t* const* points, const uint64_t* const* values, const size_t* n_claims, size_t n_queries, const uint8_t* const* proofs,
                                      const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(pcs_verify_batch_entry<GlAbi>("hg_pcs_verify_folded_device_batch", ctx, roots, nvars, n_tables, log2_row, tables, points, values, n_claims, n_queries, proofs, lens, n,
                                           results, reasons, reason_cap, true))
}
int hg_claims_verify_folded_batch(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims, size_t claim_cap_each,
                                  const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, const uint8_t* const* openings, const size_t* lens,
                                  size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_verify_batch_entry<GlAbi>("hg_claims_verify_folded_batch", ctx, params, roots, log2_row, claims, claim_cap_each, points, coord_cap_each, n_claims, n_queries,
                                              openings, lens, n, results, reasons, reason_cap, true))
}

int hg_pcs_verify_device_batch(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* const* tables,
                               const uint64_t* const* points, const uint64_t* const* values, const size_t* n_claims, size_t n_queries, const uint8_t* const* proofs,
                               const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(pcs_verify_batch_entry<GlAbi>("hg_pcs_verify_device_batch", ctx, roots, nvars, n_tables, log2_row, tables, points, values, n_claims, n_queries, proofs, lens, n, results, reasons, reason_cap))
}

int hg_claims_verify_batch(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims, size_t claim_cap_each,
                           const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, const uint8_t* const* openings, const size_t* lens,
                           size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_verify_batch_entry<GlAbi>("hg_claims_verify_batch", ctx, params, roots, log2_row, claims, claim_cap_each, points, coord_cap_each, n_claims, n_queries, openings, lens, n, results, reasons, reason_cap))
}

int hg_pcs_commit_batch(hg_ctx* ctx, const uint64_t* const* const* tables, const uint32_t* nvars, size_t n_tables, size_t log2_row, size_t n, void** commitments,
                        uint8_t* roots) {
    HG_ENTRY(pcs_commit_batch_entry<GlAbi>("hg_pcs_commit_batch", ctx, tables, nvars, n_tables, log2_row, n, commitments, roots))
}

int hg_secrets_commit_values(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, size_t log2_row, void** commitment, uint8_t root[32]) {
    HG_ENTRY(secrets_commit_values_entry("hg_secrets_commit_values", ctx, pk, v, log2_row, commitment, root))
}

int hg_secrets_commit_batch(hg_ctx* ctx, const hg_params* params, const hg_witness* const* ws, size_t n, size_t log2_row, void** commitments, uint8_t* roots) {
    HG_ENTRY(secrets_commit_batch_entry<GlAbi>("hg_secrets_commit_batch", ctx, params, ws, n, log2_row, commitments, roots))
}

int hg_pcs_open_batch(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points, const uint64_t* const* values,
                      const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap) {
    HG_ENTRY(pcs_open_batch_entry<GlAbi>("hg_pcs_open_batch", "hg_pcs_open", ctx, commitments, tables, points, values, n_claims, n_queries, n, openings, cap_each, lens, status,
                                         reasons, reason_cap))
}

int hg_claims_open_batch(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each, const uint64_t* points,
                         size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status,
                         char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_open_batch_entry<GlAbi>("hg_claims_open_batch", "hg_claims_open", "hg_secrets_commit", ctx, params, commitments, claims, claim_cap_each, points,
                                            coord_cap_each, n_claims, n_queries, n, openings, cap_each, lens, status, reasons, reason_cap))
}

// ---- the same entries over bn256::Fr (pcs_bn254.hpp): an element crosses as 4 canonical words
int hg_pcs_commit_bn254(hg_ctx* ctx, const uint64_t* const* tables4, const uint32_t* nvars, size_t n_tables, size_t log2_row, void** commitment, uint8_t root[32]) {
    HG_TRY
    if (commitment) *commitment = nullptr;
    if (!tables4 || !nvars || !commitment || !root) throw Error("hg_pcs_commit_bn254: null argument");
    const pcs::Shape sh = pcs::make_shape("hg_pcs_commit_bn254", nvars, n_tables, log2_row);
    for (size_t t = 0; t < n_tables; t++) if (!tables4[t]) throw Error("hg_pcs_commit_bn254: null table " + std::to_string(t));
    pcs::Commitment* cm = ctx ? bn::pcs_commit_device("hg_pcs_commit_bn254", ctx, sh, tables4, false) : bn::pcs_commit_host("hg_pcs_commit_bn254", sh, tables4, false);
    memcpy(root, cm->root(), 32);
    *commitment = cm;
    return 0;
    HG_CATCH(-1)
}

int hg_pcs_open_bn254(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points4, const uint64_t* values4, size_t n_claims, size_t n_queries,
                      uint8_t* proof, size_t cap, size_t* len) {
    HG_ENTRY(pcs_open_api<BnAbi>("hg_pcs_open_bn254", ctx, commitment, table, points4, values4, n_claims, n_queries, proof, cap, len))
}

int hg_pcs_verify_bn254(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points4,
                        const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_entry<BnAbi>("hg_pcs_verify_bn254", false, nullptr, root, nvars, n_tables, log2_row, table, points4, values4, n_claims, n_queries, proof, len))
}

int hg_pcs_verify_device_bn254(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points4,
                               const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_entry<BnAbi>("hg_pcs_verify_device_bn254", true, ctx, root, nvars, n_tables, log2_row, table, points4, values4, n_claims, n_queries, proof, len))
}

int hg_secrets_commit_bn254(hg_ctx* ctx, const hg_params* params, const hg_witness* w, size_t log2_row, void** commitment, uint8_t root[32]) {
    HG_ENTRY(secrets_commit_entry<BnAbi>("hg_secrets_commit_bn254", ctx, params, w, log2_row, commitment, root))
}

int hg_claims_open_bn254(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points4, size_t n_queries,
                         uint8_t* opening, size_t cap, size_t* len) {
    HG_ENTRY(claims_open_entry<BnAbi>("hg_claims_open_bn254", "hg_secrets_commit_bn254", ctx, params, commitment, claims, n, points4, n_queries, opening, cap, len))
}

int hg_claims_verify_bn254(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points4,
                           size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<BnAbi>("hg_claims_verify_bn254", false, nullptr, params, root, log2_row, claims, n, points4, n_queries, opening, len))
}

int hg_claims_verify_device_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points4,
                                  size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<BnAbi>("hg_claims_verify_device_bn254", true, ctx, params, root, log2_row, claims, n, points4, n_queries, opening, len))
}

int hg_pcs_open_folded_bn254(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points4, const uint64_t* values4, size_t n_claims, size_t n_queries,
                             uint8_t* proof, size_t cap, size_t* len) {
    HG_ENTRY(pcs_open_folded_api<BnAbi>("hg_pcs_open_folded_bn254", ctx, commitment, table, points4, values4, n_claims, n_queries, proof, cap, len))
}
int hg_pcs_verify_folded_bn254(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points4,
                               const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_folded_entry<BnAbi>("hg_pcs_verify_folded_bn254", false, nullptr, root, nvars, n_tables, log2_row, table, points4, values4, n_claims, n_queries, proof, len))
}
int hg_pcs_verify_folded_device_bn254(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points4,
                                      const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len) {
    HG_ENTRY(pcs_verify_folded_entry<BnAbi>("hg_pcs_verify_folded_device_bn254", true, ctx, root, nvars, n_tables, log2_row, table, points4, values4, n_claims, n_queries, proof, len))
}
int hg_claims_open_folded_bn254(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points4, size_t n_queries,
                                uint8_t* opening, size_t cap, size_t* len) {
    HG_ENTRY(claims_open_entry<BnAbi>("hg_claims_open_folded_bn254", "hg_secrets_commit_bn254", ctx, params, commitment, claims, n, points4, n_queries, opening, cap, len, true))
}
int hg_claims_verify_folded_bn254(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points4,
                                  size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<BnAbi>("hg_claims_verify_folded_bn254", false, nullptr, params, root, log2_row, claims, n, points4, n_queries, opening, len, true))
}
int hg_claims_verify_folded_device_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points4,
                                         size_t n_queries, const uint8_t* opening, size_t len) {
    HG_ENTRY(claims_verify_entry<BnAbi>("hg_claims_verify_folded_device_bn254", true, ctx, params, root, log2_row, claims, n, points4, n_queries, opening, len, true))
}

int hg_pcs_open_folded_batch_bn254(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points4, const uint64_t* const* values4,
                                   const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status, char* reasons,
                                   size_t reason_cap) {
    HG_ENTRY(pcs_open_batch_entry<BnAbi>("hg_pcs_open_folded_batch_bn254", "hg_pcs_open_folded_bn254", ctx, commitments, tables, points4, values4, n_claims, n_queries, n, openings,
                                         cap_each, lens, status, reasons, reason_cap, true))
}
int hg_claims_open_folded_batch_bn254(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each, const uint64_t* points4,
                                      size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status,
                                      char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_open_batch_entry<BnAbi>("hg_claims_open_folded_batch_bn254", "hg_claims_open_folded_bn254", "hg_secrets_commit_bn254", ctx, params, commitments, claims,
                                            claim_cap_each, points4, coord_cap_each, n_claims, n_queries, n, openings, cap_each, lens, status, reasons, reason_cap, true))
}
int hg_pcs_verify_folded_device_batch_bn254(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* const* tables,
                                            const uint64_t* const* points4, const uint64_t* const* values4, const size_t* n_claims, size_t n_queries,
                                            const uint8_t* const* proofs, const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(pcs_verify_batch_entry<BnAbi>("hg_pcs_verify_folded_device_batch_bn254", ctx, roots, nvars, n_tables, log2_row, tables, points4, values4, n_claims, n_queries, proofs,
                                           lens, n, results, reasons, reason_cap, true))
}
int hg_claims_verify_folded_batch_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims, size_t claim_cap_each,
                                        const uint64_t* points4, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, const uint8_t* const* openings,
                                        const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_verify_batch_entry<BnAbi>("hg_claims_verify_folded_batch_bn254", ctx, params, roots, log2_row, claims, claim_cap_each, points4, coord_cap_each, n_claims,
                                              n_queries, openings, lens, n, results, reasons, reason_cap, true))
}

int hg_pcs_verify_device_batch_bn254(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* const* tables,
                                     const uint64_t* const* points4, const uint64_t* const* values4, const size_t* n_claims, size_t n_queries, const uint8_t* const* proofs,
                                     const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(pcs_verify_batch_entry<BnAbi>("hg_pcs_verify_device_batch_bn254", ctx, roots, nvars, n_tables, log2_row, tables, points4, values4, n_claims, n_queries, proofs, lens, n, results, reasons, reason_cap))
}

int hg_claims_verify_batch_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims, size_t claim_cap_each,
                                 const uint64_t* points4, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, const uint8_t* const* openings, const size_t* lens,
                                 size_t n, int* results, char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_verify_batch_entry<BnAbi>("hg_claims_verify_batch_bn254", ctx, params, roots, log2_row, claims, claim_cap_each, points4, coord_cap_each, n_claims, n_queries, openings, lens, n, results, reasons, reason_cap))
}

int hg_pcs_commit_batch_bn254(hg_ctx* ctx, const uint64_t* const* const* tables4, const uint32_t* nvars, size_t n_tables, size_t log2_row, size_t n, void** commitments,
                              uint8_t* roots) {
    HG_ENTRY(pcs_commit_batch_entry<BnAbi>("hg_pcs_commit_batch_bn254", ctx, tables4, nvars, n_tables, log2_row, n, commitments, roots))
}

int hg_secrets_commit_batch_bn254(hg_ctx* ctx, const hg_params* params, const hg_witness* const* ws, size_t n, size_t log2_row, void** commitments, uint8_t* roots) {
    HG_ENTRY(secrets_commit_batch_entry<BnAbi>("hg_secrets_commit_batch_bn254", ctx, params, ws, n, log2_row, commitments, roots))
}

int hg_pcs_open_batch_bn254(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points4, const uint64_t* const* values4,
                            const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status, char* reasons,
                            size_t reason_cap) {
    HG_ENTRY(pcs_open_batch_entry<BnAbi>("hg_pcs_open_batch_bn254", "hg_pcs_open_bn254", ctx, commitments, tables, points4, values4, n_claims, n_queries, n, openings, cap_each,
                                         lens, status, reasons, reason_cap))
}

int hg_claims_open_batch_bn254(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each, const uint64_t* points4,
                               size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each, size_t* lens, int* status,
                               char* reasons, size_t reason_cap) {
    HG_ENTRY(claims_open_batch_entry<BnAbi>("hg_claims_open_batch_bn254", "hg_claims_open_bn254", "hg_secrets_commit_bn254", ctx, params, commitments, claims, claim_cap_each,
                                            points4, coord_cap_each, n_claims, n_queries, n, openings, cap_each, lens, status, reasons, reason_cap))
}

int hg_profile(hg_ctx* ctx, int level) {
    if (!ctx) { g_last_error = "hg_profile: null context"; return -1; }
    ctx->prof_level = level;
    return 0;
}
int hg_profile_select(hg_ctx* ctx, const char* name) {
    if (!ctx || !name) { g_last_error = "hg_profile_select: null argument"; return -1; }
    bool found = false;
    for (auto& s : ctx->prof_stats) found = found || s.name == name;
    if (!found) { g_last_error = std::string("hg_profile_select: no kernel class named ") + name; return -1; }
    for (auto& s : ctx->prof_stats) s.dominant = s.name == name;
    return 0;
}
int hg_profile_reset(hg_ctx* ctx) {
    if (!ctx) { g_last_error = "hg_profile_reset: null context"; return -1; }
    for (auto& s : ctx->prof_stats) { s.launches = 0; s.ms = 0; s.bytes = 0; s.model = 0; s.design = 0; }
    return 0;
}
int hg_profile_get(hg_ctx* ctx, hg_kernel_stat* out, int cap) {
    if (!ctx || (!out && cap > 0)) { g_last_error = "hg_profile_get: null argument"; return -1; }
    int n = 0;
    for (auto& s : ctx->prof_stats) {
        if (n >= cap) break;
        memset(&out[n], 0, sizeof(out[n]));
        strncpy(out[n].name, s.name.c_str(), sizeof(out[n].name) - 1);
        out[n].launches = s.launches; out[n].total_ms = s.ms; out[n].algo_bytes = s.bytes; out[n].model_bytes = s.model; out[n].hbm_bytes = s.design;
        n++;
    }
    return n;
}

}  // extern "C"
