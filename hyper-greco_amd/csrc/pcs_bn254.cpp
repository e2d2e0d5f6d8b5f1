// Host side of the polynomial commitment over bn256::Fr (pcs_bn254.hpp): the host form of commit, the opening's transcript and byte
// layout (shared by both forms) and the verifier. Elements at rest are canonical plain words; weights and twiddles are in Montgomery
// form, so fr_mul(weight, element) is the plain product.
#include "pcs_bn254.hpp"
#include <algorithm>
#include <memory>

namespace hg {
namespace bn {

using pcs::Commitment;
using pcs::Shape;

static Fr fr_load(const u64* p) { return fr_make(p[0], p[1], p[2], p[3]); }

// w^i, i < count, in Montgomery form; w = 7^((r-1)/2^log2n) (the root of hg_ntt_bn254)
static std::vector<Fr> root_powers(int log2n, size_t count) {
    if (log2n > 28) throw Error("bn254: two-adicity is 28");
    Fr w = fr_to_mont(fr_make(0xd34f1ed960c37c9cULL, 0x3215cf6dd39329c8ULL, 0x98865ea93dd31f74ULL, 0x03ddb9f5166d18b7ULL));
    for (int i = log2n; i < 28; i++) w = fr_mul(w, w);
    std::vector<Fr> W(count);
    Fr x = fr_one_mont();
    for (size_t i = 0; i < count; i++) { W[i] = x; x = fr_mul(x, w); }
    return W;
}
// forward radix-2 transform in place, natural order in and out; W = root_powers(log2n, n / 2). Linear, so plain words stay plain.
static void ntt_host_fr(Fr* a, int log2n, const Fr* W) {
    const size_t n = (size_t)1 << log2n;
    for (size_t i = 0, j = 0; i < n; i++) {
        if (i < j) std::swap(a[i], a[j]);
        size_t bit = n >> 1;
        for (; bit && (j & bit); bit >>= 1) j ^= bit;
        j |= bit;
    }
    for (int s = 0; s < log2n; s++) {
        const size_t span = (size_t)1 << s;
        for (size_t g = 0; g < n; g += 2 * span)
            for (size_t k = 0; k < span; k++) {
                const Fr u = a[g + k], v = fr_mul(a[g + k + span], W[k << (log2n - 1 - s)]);
                a[g + k] = fr_add(u, v);
                a[g + k + span] = fr_sub(u, v);
            }
    }
}

static void leaf_hash_fr(const Fr* col, size_t R, uint8_t out[32]) {   // Keccak256(LE64(0) || repr(col[0]) || ..); little-endian host
    std::vector<u64> msg(4 * R + 1);
    msg[0] = 0;
    memcpy(msg.data() + 1, col, 32 * R);
    keccak256(reinterpret_cast<const uint8_t*>(msg.data()), 8 * msg.size(), out);
}
std::vector<Fr> pcs_eq_table(const Fr* pt_canon, size_t n) {   // Montgomery form; coordinate i belongs to bit i of the index
    std::vector<Fr> t(1, fr_one_mont());
    t.reserve((size_t)1 << n);
    for (size_t i = 0; i < n; i++) {
        const Fr z = fr_to_mont(pt_canon[i]);
        const size_t h = t.size();
        t.resize(2 * h);
        for (size_t x = 0; x < h; x++) {
            const Fr hi = fr_mul(t[x], z);
            t[x + h] = hi;
            t[x] = fr_sub(t[x], hi);
        }
    }
    return t;
}
std::vector<Fr> pcs_rho_powers(const Fr& rho_canon, size_t R) {
    std::vector<Fr> w(R);
    const Fr rho = fr_to_mont(rho_canon);
    Fr x = fr_one_mont();
    for (size_t r = 0; r < R; r++) { w[r] = x; x = fr_mul(x, rho); }
    return w;
}
static Fr dot_fr(const Fr* w_mont, const Fr* x_canon, size_t n) {   // canonical
    Fr s = fr_zero();
    for (size_t i = 0; i < n; i++) s = fr_add(s, fr_mul(w_mont[i], x_canon[i]));
    return s;
}

Commitment* pcs_commit_host(const char* who, const Shape& sh, const u64* const* tables, bool words) {
    std::unique_ptr<Commitment> cm(new Commitment());
    cm->field = pcs::BN254;
    cm->sh = sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    cm->rows.resize(4 * R * C);
    [[maybe_unused]] const int nt = hg_omp_threads();   // (the device pass of hipcc ignores the pragmas)
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t len = (size_t)1 << sh.nvars[t];
        Fr* dst = reinterpret_cast<Fr*>(cm->rows.data()) + sh.off[t] * C;
        if (words) {
#pragma omp parallel for schedule(static) num_threads(nt) if (len >= 4096)
            for (long long i = 0; i < (long long)len; i++) dst[i] = fr_lift_signed_canon(tables[t][i]);
        } else {
            for (size_t i = 0; i < len; i++)
                if (fr_geq_p(fr_load(tables[t] + 4 * i))) throw Error(std::string(who) + ": a table holds an element that is not below r");
            memcpy(dst, tables[t], len * 32);
        }
    }
    cm->M.assign(4 * R * N, 0);
    const Fr* rows = reinterpret_cast<const Fr*>(cm->rows.data());
    Fr* M = reinterpret_cast<Fr*>(cm->M.data());
    const std::vector<Fr> W = root_powers(sh.depth(), N / 2);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long long r = 0; r < (long long)R; r++) {
        memcpy(M + r * N, rows + r * C, C * 32);
        ntt_host_fr(M + r * N, sh.depth(), W.data());
    }
    cm->tree.resize(32 * (2 * N - 1));
    // two adjacent columns (one cache line of every encoded row) per pass
    const size_t tile = std::min<size_t>(2, N);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long long j0 = 0; j0 < (long long)N; j0 += tile) {
        std::vector<Fr> col(tile * R);
        for (size_t r = 0; r < R; r++)
            for (size_t jj = 0; jj < tile; jj++) col[jj * R + r] = M[r * N + j0 + jj];
        for (size_t jj = 0; jj < tile; jj++) leaf_hash_fr(col.data() + jj * R, R, cm->tree.data() + 32 * (j0 + jj));
    }
    for (int l = 1; l <= sh.depth(); l++) {
        const size_t cnt = N >> l;
        const uint8_t* below = cm->node(l - 1, 0);
        uint8_t* here = cm->tree.data() + (cm->node(l, 0) - cm->tree.data());
#pragma omp parallel for schedule(static) num_threads(nt) if (cnt >= 1024)
        for (long long i = 0; i < (long long)cnt; i++) pcs::node_hash(below + 64 * i, below + 64 * i + 32, here + 32 * i);
    }
    return cm.release();
}

void pcs_combine_host(const Commitment& cm, const std::vector<PcsJob>& jobs, Fr* u) {
    const size_t C = cm.sh.C();
    const Fr* rows = reinterpret_cast<const Fr*>(cm.rows.data());
    constexpr size_t TILE = 16, CHUNK = 1024;   // w512_reduce takes a sum below 2^10 r^2: 1024 products of residues
    const size_t tiles = (C + TILE - 1) / TILE;
    [[maybe_unused]] const int nt = hg_omp_threads();
#pragma omp parallel for schedule(dynamic, 4) num_threads(nt) if (jobs.size() * C >= 4096)
    for (long long id = 0; id < (long long)(jobs.size() * tiles); id++) {
        const size_t q = (size_t)id / tiles, j0 = ((size_t)id % tiles) * TILE, j1 = std::min(C, j0 + TILE);
        const PcsJob& job = jobs[q];
        Fr s[TILE];
        for (size_t j = 0; j < TILE; j++) s[j] = fr_zero();
        for (size_t r0 = 0; r0 < job.nrows; r0 += CHUNK) {
            const size_t r1 = std::min(job.nrows, r0 + CHUNK);
            W512 acc[TILE];
            for (size_t j = 0; j < TILE; j++) acc[j] = w512_zero();
            for (size_t r = r0; r < r1; r++) {
                const Fr* row = rows + (job.row0 + r) * C;
                const Fr w = job.w[r];
                for (size_t j = j0; j < j1; j++) w512_mac(acc[j - j0], w, row[j]);
            }
            for (size_t j = j0; j < j1; j++) s[j - j0] = fr_add(s[j - j0], w512_reduce(acc[j - j0]));
        }
        for (size_t j = j0; j < j1; j++) u[q * C + j] = s[j - j0];
    }
}
void pcs_columns_host(const Commitment& cm, const std::vector<size_t>& js, Fr* cols) {
    const size_t N = cm.sh.N(), R = cm.sh.R;
    const Fr* M = reinterpret_cast<const Fr*>(cm.M.data());
    for (size_t q = 0; q < js.size(); q++)
        for (size_t r = 0; r < R; r++) cols[q * R + r] = M[r * N + js[q]];
}

// ---- the transcript both sides and both forms of the verifier share (declared in pcs_bn254.hpp): FsTranscript's pending bytes and
// proof stream under the BN254 rules
static void put_le32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i))); }
void pcs_absorb(FsTranscript& tr, const Fr* x, size_t count) {   // little-endian host: canonical words are the repr
    const uint8_t* b = reinterpret_cast<const uint8_t*>(x);
    tr.pending.insert(tr.pending.end(), b, b + 32 * count);
}
Fr pcs_squeeze(FsTranscript& tr) {   // LE(hash) mod r, the state re-hashed: hg_challenges_bn254's rule over the absorbed bytes
    uint8_t h[32];
    keccak256(tr.pending.data(), tr.pending.size(), h);
    tr.pending.assign(h, h + 32);
    Fr v;
    memcpy(v.l, h, 32);
    while (fr_geq_p(v)) v = fr_sub_p(v);   // 2^256 / r < 6
    return v;
}
FsTranscript pcs_start_transcript(const Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q) {
    FsTranscript tr;
    tr.absorb = true;
    static const char tag[] = "hg-pcs-bn254-1";
    tr.pending.assign(tag, tag + sizeof(tag) - 1);
    tr.pending.insert(tr.pending.end(), root, root + 32);
    put_le32(tr.pending, (uint32_t)sh.c);
    put_le32(tr.pending, (uint32_t)sh.nvars.size());
    for (int v : sh.nvars) put_le32(tr.pending, (uint32_t)v);
    put_le32(tr.pending, (uint32_t)Q);
    put_le32(tr.pending, (uint32_t)claims.size());
    for (const PcsClaim& cl : claims) {
        put_le32(tr.pending, (uint32_t)cl.table);
        pcs_absorb(tr, cl.point.data(), cl.point.size());
        pcs_absorb(tr, &cl.value, 1);
    }
    return tr;
}
std::vector<size_t> pcs_squeeze_indices(FsTranscript& tr, size_t N, size_t Q) {   // the low 64 bits of a squeezed element & (N - 1)
    std::vector<size_t> js(Q);
    for (size_t q = 0; q < Q; q++) js[q] = (size_t)(pcs_squeeze(tr).l[0] & (u64)(N - 1));
    return js;
}
static void write_be32(std::vector<uint8_t>& out, const Fr& x) {   // 32 bytes big-endian, as every BN254 proof element
    for (int w = 3; w >= 0; w--)
        for (int b = 7; b >= 0; b--) out.push_back((uint8_t)(x.l[w] >> (8 * b)));
}
Fr pcs_read_be32(const uint8_t* p) {
    Fr v;
    for (int w = 0; w < 4; w++) {
        u64 a = 0;
        for (int i = 0; i < 8; i++) a = (a << 8) | p[8 * (3 - w) + i];
        v.l[w] = a;
    }
    return v;
}

std::vector<uint8_t> pcs_open(const char* who, const Commitment& cm, const std::vector<PcsClaim>& claims, size_t Q) {
    const Shape& sh = cm.sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R, n = claims.size();
    FsTranscript tr = pcs_start_transcript(sh, cm.root(), claims, Q);
    std::vector<PcsJob> jobs(n + 1);
    jobs[0].row0 = 0; jobs[0].nrows = R; jobs[0].w = pcs_rho_powers(pcs_squeeze(tr), R);
    for (size_t i = 0; i < n; i++) {
        const PcsClaim& cl = claims[i];
        jobs[i + 1].row0 = sh.off[cl.table];
        jobs[i + 1].nrows = (size_t)1 << (sh.nvars[cl.table] - sh.c);
        jobs[i + 1].w = pcs_eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
    }
    std::vector<Fr> u((n + 1) * C);
    if (cm.ctx) pcs_combine_device(cm, jobs, u.data()); else pcs_combine_host(cm, jobs, u.data());
    for (size_t i = 0; i < n; i++) {   // the prover holds u_i: the check is free
        const std::vector<Fr> lo = pcs_eq_table(claims[i].point.data(), (size_t)sh.c);
        if (!fr_eq(dot_fr(lo.data(), u.data() + (i + 1) * C, C), claims[i].value))
            throw Error(std::string(who) + ": claim " + std::to_string(i) + ": the value is not the evaluation of table " + std::to_string(claims[i].table) + " at the point");
    }
    std::vector<uint8_t>& out = tr.bytes;
    out.reserve(pcs_opening_bytes(sh, n, Q));
    for (const Fr& x : u) write_be32(out, x);
    pcs_absorb(tr, u.data(), u.size());
    const std::vector<size_t> js = pcs_squeeze_indices(tr, N, Q);
    std::vector<Fr> cols(Q * R);
    if (Q) { if (cm.ctx) pcs_columns_device(cm, js, cols.data()); else pcs_columns_host(cm, js, cols.data()); }
    for (size_t q = 0; q < Q; q++) {
        for (size_t r = 0; r < R; r++) write_be32(out, cols[q * R + r]);
        size_t idx = js[q];
        for (int l = 0; l < sh.depth(); l++, idx >>= 1) {
            const uint8_t* sib = cm.node(l, idx ^ 1);
            out.insert(out.end(), sib, sib + 32);
        }
    }
    if (out.size() != pcs_opening_bytes(sh, n, Q)) throw Error(std::string(who) + ": internal: opening length");
    return std::move(tr.bytes);
}

std::string pcs_verify(const Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R, n = claims.size();
    const int depth = sh.depth();
    // 1. exact length
    const std::string bad_len = pcs::length_reason(len, pcs_opening_bytes(sh, n, Q));
    if (!bad_len.empty()) return bad_len;
    // 2. every element below r
    const size_t u_bytes = 32 * C * (n + 1), q_bytes = 32 * R + 32 * (size_t)depth;
    std::vector<Fr> u((n + 1) * C);
    for (size_t i = 0; i < u.size(); i++) {
        u[i] = pcs_read_be32(proof + 32 * i);
        if (fr_geq_p(u[i])) return pcs::reason_noncanonical(32 * i);
    }
    std::vector<Fr> cols(Q * R);
    for (size_t q = 0; q < Q; q++)
        for (size_t r = 0; r < R; r++) {
            const size_t at = u_bytes + q * q_bytes + 32 * r;
            cols[q * R + r] = pcs_read_be32(proof + at);
            if (fr_geq_p(cols[q * R + r])) return pcs::reason_noncanonical(at);
        }
    // 3. <u_i, eq(z_i[..c])> == y_i
    for (size_t i = 0; i < n; i++) {
        const std::vector<Fr> lo = pcs_eq_table(claims[i].point.data(), (size_t)sh.c);
        if (!fr_eq(dot_fr(lo.data(), u.data() + (i + 1) * C, C), claims[i].value)) return pcs::reason_evaluation(i);
    }
    // the challenges
    FsTranscript tr = pcs_start_transcript(sh, root, claims, Q);
    const std::vector<Fr> rho = pcs_rho_powers(pcs_squeeze(tr), R);
    pcs_absorb(tr, u.data(), u.size());
    const std::vector<size_t> js = pcs_squeeze_indices(tr, N, Q);
    // Enc(u_i)
    std::vector<Fr> enc((n + 1) * N, fr_zero());
    std::vector<std::vector<Fr>> w(n);
    if (Q) {
        const std::vector<Fr> W = root_powers(depth, N / 2);
        [[maybe_unused]] const int nt = hg_omp_threads();
#pragma omp parallel for schedule(static) num_threads(nt) if (N >= 1024)
        for (long long i = 0; i < (long long)(n + 1); i++) {
            memcpy(enc.data() + i * N, u.data() + i * C, 32 * C);
            ntt_host_fr(enc.data() + i * N, depth, W.data());
        }
        for (size_t i = 0; i < n; i++) w[i] = pcs_eq_table(claims[i].point.data() + sh.c, (size_t)(sh.nvars[claims[i].table] - sh.c));
    }
    // 4. per query: path, proximity, claims
    for (size_t q = 0; q < Q; q++) {
        const Fr* col = cols.data() + q * R;
        const uint8_t* sib = proof + u_bytes + q * q_bytes + 32 * R;
        uint8_t h[32], nx[32];
        leaf_hash_fr(col, R, h);
        size_t idx = js[q];
        for (int l = 0; l < depth; l++, idx >>= 1) {
            if (idx & 1) pcs::node_hash(sib + 32 * l, h, nx); else pcs::node_hash(h, sib + 32 * l, nx);
            memcpy(h, nx, 32);
        }
        if (memcmp(h, root, 32) != 0) return pcs::reason_merkle(q);
        if (!fr_eq(dot_fr(rho.data(), col, R), enc[js[q]])) return pcs::reason_proximity(q);
        for (size_t i = 0; i < n; i++)
            if (!fr_eq(dot_fr(w[i].data(), col + sh.off[claims[i].table], w[i].size()), enc[(i + 1) * N + js[q]])) return pcs::reason_claim(i, q);
    }
    return "";
}

}  // namespace bn
}  // namespace hg
