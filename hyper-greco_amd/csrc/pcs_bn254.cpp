// Host side of the polynomial commitment over bn256::Fr (pcs_bn254.hpp): the host form of commit, the opening's transcript and byte
// layout (shared by both forms) and the verifier; the folded opening's host flow (both forms), its host reduction, its host verifier
// and the header walk both folded verifiers share. Elements at rest are canonical plain words; weights and twiddles are in Montgomery
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
FsTranscript pcs_start_transcript(const Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const char* tag) {
    FsTranscript tr;
    tr.absorb = true;
    tr.pending.assign(tag, tag + strlen(tag));
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

// the end of an opening, folded or not: the u vectors written and absorbed, the Q column indices squeezed, then per query the R column
// elements and the siblings of the path. `total`: the bytes of the finished opening
static void write_u_and_queries(FsTranscript& tr, const Commitment& cm, const std::vector<Fr>& u, size_t Q, size_t total) {
    const Shape& sh = cm.sh;
    const size_t N = sh.N(), R = sh.R;
    std::vector<uint8_t>& out = tr.bytes;
    out.reserve(total);
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
}

std::vector<uint8_t> pcs_open(const char* who, const Commitment& cm, const std::vector<PcsClaim>& claims, size_t Q) {
    const Shape& sh = cm.sh;
    const size_t C = sh.C(), R = sh.R, n = claims.size();
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
    write_u_and_queries(tr, cm, u, Q, pcs_opening_bytes(sh, n, Q));
    if (tr.bytes.size() != pcs_opening_bytes(sh, n, Q)) throw Error(std::string(who) + ": internal: opening length");
    return std::move(tr.bytes);
}


// ---- the body of an opening - n + 1 u vectors, then Q queries - as pcs_verify and pcs_verify_folded check it
// Reads the u vectors and the Q R column elements of a body that starts at byte `base` of its opening -> "" or the reason of the lowest
// element that is not below r
static std::string read_body(const Shape& sh, size_t n, size_t Q, const uint8_t* body, size_t base, std::vector<Fr>& u, std::vector<Fr>& cols) {
    const size_t C = sh.C(), R = sh.R;
    const size_t u_bytes = 32 * C * (n + 1), q_bytes = 32 * R + 32 * (size_t)sh.depth();
    u.resize((n + 1) * C);
    for (size_t i = 0; i < u.size(); i++) {
        u[i] = pcs_read_be32(body + 32 * i);
        if (fr_geq_p(u[i])) return pcs::reason_noncanonical(base + 32 * i);
    }
    cols.resize(Q * R);
    for (size_t q = 0; q < Q; q++)
        for (size_t r = 0; r < R; r++) {
            const size_t at = u_bytes + q * q_bytes + 32 * r;
            cols[q * R + r] = pcs_read_be32(body + at);
            if (fr_geq_p(cols[q * R + r])) return pcs::reason_noncanonical(base + at);
        }
    return "";
}
// a claim as the queries see it: its weights (Montgomery form) over the rows from row0 on
struct RowWeights { size_t row0; std::vector<Fr> w; };
// The u vectors into the transcript, the column indices out of it, then per query: path, proximity (rho: the R powers), claims.
// weights(i): claim i's, called once and only if there is a query
template <class Weights>
static std::string check_queries(const Shape& sh, const uint8_t root[32], FsTranscript& tr, const std::vector<Fr>& rho, size_t n, Weights weights, const std::vector<Fr>& u,
                                 const std::vector<Fr>& cols, size_t Q, const uint8_t* body) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int depth = sh.depth();
    const size_t u_bytes = 32 * C * (n + 1), q_bytes = 32 * R + 32 * (size_t)depth;
    pcs_absorb(tr, u.data(), u.size());
    const std::vector<size_t> js = pcs_squeeze_indices(tr, N, Q);
    // Enc(u_i)
    std::vector<Fr> enc((n + 1) * N, fr_zero());
    std::vector<RowWeights> w(n);
    if (Q) {
        const std::vector<Fr> W = root_powers(depth, N / 2);
        [[maybe_unused]] const int nt = hg_omp_threads();
#pragma omp parallel for schedule(static) num_threads(nt) if (N >= 1024)
        for (long long i = 0; i < (long long)(n + 1); i++) {
            memcpy(enc.data() + i * N, u.data() + i * C, 32 * C);
            ntt_host_fr(enc.data() + i * N, depth, W.data());
        }
        for (size_t i = 0; i < n; i++) w[i] = weights(i);
    }
    for (size_t q = 0; q < Q; q++) {
        const Fr* col = cols.data() + q * R;
        const uint8_t* sib = body + u_bytes + q * q_bytes + 32 * R;
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
            if (!fr_eq(dot_fr(w[i].w.data(), col + w[i].row0, w[i].w.size()), enc[(i + 1) * N + js[q]])) return pcs::reason_claim(i, q);
    }
    return "";
}

std::string pcs_verify(const Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), R = sh.R, n = claims.size();
    // 1. exact length
    const std::string bad_len = pcs::length_reason(len, pcs_opening_bytes(sh, n, Q));
    if (!bad_len.empty()) return bad_len;
    // 2. every element below r
    std::vector<Fr> u, cols;
    const std::string bad_word = read_body(sh, n, Q, proof, 0, u, cols);
    if (!bad_word.empty()) return bad_word;
    // 3. <u_i, eq(z_i[..c])> == y_i
    for (size_t i = 0; i < n; i++) {
        const std::vector<Fr> lo = pcs_eq_table(claims[i].point.data(), (size_t)sh.c);
        if (!fr_eq(dot_fr(lo.data(), u.data() + (i + 1) * C, C), claims[i].value)) return pcs::reason_evaluation(i);
    }
    // the challenges, then 4. per query: path, proximity, claims
    FsTranscript tr = pcs_start_transcript(sh, root, claims, Q);
    const std::vector<Fr> rho = pcs_rho_powers(pcs_squeeze(tr), R);
    auto weights = [&](size_t i) { return RowWeights{sh.off[claims[i].table], pcs_eq_table(claims[i].point.data() + sh.c, (size_t)(sh.nvars[claims[i].table] - sh.c))}; };
    return check_queries(sh, root, tr, rho, n, weights, u, cols, Q, proof);
}

// ---- folded openings (hg.h "Folded openings over BN254"): pcs.cpp's with F = E = Fr. Table entries, the round's sums, the Y_t and every
// element written are plain canonical words; beta^i, the challenges as multipliers, g and the tails are in Montgomery form, so a
// Montgomery product of one of each is the plain product.
static const char FOLD_TAG[] = "hg-pcs-bn254-fold-1";
// eq(z, r) for one coordinate: z r + (1 - z) (1 - r), all in Montgomery form
static Fr eq1(const Fr& z, const Fr& r) {
    const Fr zr = fr_mul(z, r);
    return fr_sub(fr_add(fr_add(zr, zr), fr_one_mont()), fr_add(z, r));
}
// the weights of the combined row over all R rows: w[off_t + r] = delta^t eq(rho[c..v_t))[r]
static std::vector<Fr> combined_weights(const Shape& sh, const std::vector<Fr>& rho_canon, const Fr& delta_canon) {
    std::vector<Fr> w(sh.R);
    const Fr delta = fr_to_mont(delta_canon);
    Fr d = fr_one_mont();
    for (size_t t = 0; t < sh.nvars.size(); t++, d = fr_mul(d, delta)) {
        const std::vector<Fr> eq = pcs_eq_table(rho_canon.data() + sh.c, (size_t)(sh.nvars[t] - sh.c));
        for (size_t r = 0; r < eq.size(); r++) w[sh.off[t] + r] = fr_mul(d, eq[r]);
    }
    return w;
}
static void write_fr(FsTranscript& tr, const Fr& x) {   // an element of the header: into the opening and into the transcript
    write_be32(tr.bytes, x);
    pcs_absorb(tr, &x, 1);
}

// The host form of the reduction: every table (plain) and its g (Montgomery) as vectors, folded in place
struct FoldHost : PcsFoldSource {
    std::vector<std::vector<Fr>> t, g;
    void step(size_t j, const Fr& r, Fr s[3]) override {
        [[maybe_unused]] const int nt = hg_omp_threads();
        const Fr rm = fr_to_mont(r);
        for (size_t x = 0; x < t.size(); x++) {
            std::vector<Fr>&a = t[x], &b = g[x];
            if (a.empty()) continue;   // retired
            if (j > 0) {
                const long long h = (long long)(a.size() / 2);
                std::vector<Fr> a2((size_t)h), b2((size_t)h);
#pragma omp parallel for schedule(static) num_threads(nt) if (h >= 4096)
                for (long long i = 0; i < h; i++) {
                    a2[i] = fr_add(a[2 * i], fr_mul(rm, fr_sub(a[2 * i + 1], a[2 * i])));
                    b2[i] = fr_add(b[2 * i], fr_mul(rm, fr_sub(b[2 * i + 1], b[2 * i])));
                }
                a.swap(a2);
                b.swap(b2);
            }
            if (a.size() == 1) {
                T[x] = a[0];
                G[x] = b[0];
                a.clear();
                b.clear();
            }
        }
        if (!s) return;
        s[0] = s[1] = s[2] = fr_zero();
        for (size_t x = 0; x < t.size(); x++) {
            const std::vector<Fr>&a = t[x], &b = g[x];
            const long long h = (long long)(a.size() / 2);
            const int parts = h >= 4096 ? nt : 1;
            std::vector<Fr> part(3 * (size_t)parts, fr_zero());
#pragma omp parallel for schedule(static) num_threads(parts)
            for (int q = 0; q < parts; q++) {
                Fr s0 = fr_zero(), s1 = fr_zero(), s2 = fr_zero();
                for (long long i = h * q / parts; i < h * (q + 1) / parts; i++) {
                    s0 = fr_add(s0, fr_mul(b[2 * i], a[2 * i]));
                    s1 = fr_add(s1, fr_mul(b[2 * i + 1], a[2 * i + 1]));
                    s2 = fr_add(s2, fr_mul(fr_sub(b[2 * i + 1], b[2 * i]), fr_sub(a[2 * i + 1], a[2 * i])));
                }
                part[3 * q] = s0; part[3 * q + 1] = s1; part[3 * q + 2] = s2;
            }
            for (int q = 0; q < parts; q++)
                for (int k = 0; k < 3; k++) s[k] = fr_add(s[k], part[3 * q + k]);
        }
    }
};
std::unique_ptr<PcsFoldSource> pcs_fold_source_host(const Commitment& cm, const std::vector<PcsClaim>& claims, const std::vector<Fr>& bpow) {
    const Shape& sh = cm.sh;
    const size_t m = sh.nvars.size(), C = sh.C();
    std::unique_ptr<FoldHost> f(new FoldHost());
    f->T.assign(m, fr_zero());
    f->G.assign(m, fr_zero());
    f->t.resize(m);
    f->g.resize(m);
    const Fr* rows = reinterpret_cast<const Fr*>(cm.rows.data());
    for (size_t x = 0; x < m; x++) {
        const size_t len = (size_t)1 << sh.nvars[x];
        f->t[x].assign(rows + sh.off[x] * C, rows + sh.off[x] * C + len);
        f->g[x].assign(len, fr_zero());
    }
    [[maybe_unused]] const int nt = hg_omp_threads();
    for (size_t i = 0; i < claims.size(); i++) {
        const std::vector<Fr> eq = pcs_eq_table(claims[i].point.data(), claims[i].point.size());
        std::vector<Fr>& g = f->g[claims[i].table];
        const Fr b = bpow[i];
#pragma omp parallel for schedule(static) num_threads(nt) if (eq.size() >= 4096)
        for (long long k = 0; k < (long long)eq.size(); k++) g[k] = fr_add(g[k], fr_mul(b, eq[k]));
    }
    return f;
}

PcsFoldProver::PcsFoldProver(const Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q)
    : tr(pcs_start_transcript(sh, root, claims, Q, FOLD_TAG)), tail(sh.nvars.size(), fr_one_mont()), rho(pcs::fold_rounds(sh)), claim(fr_zero()), r(fr_zero()) {
    bpow = pcs_rho_powers(pcs_squeeze(tr), claims.size());
    for (size_t i = 0; i < claims.size(); i++) claim = fr_add(claim, fr_mul(bpow[i], claims[i].value));
}
bool PcsFoldProver::round(const Shape& sh, size_t j, const Fr s[3], const std::vector<Fr>& T, const std::vector<Fr>& G) {
    const size_t m = sh.nvars.size();
    Fr k = fr_zero();   // the retired tables: K_t prod (1 - r_j') (1 - X), plain
    for (size_t t = 0; t < m; t++)
        if ((size_t)sh.nvars[t] <= j) k = fr_add(k, fr_mul(fr_mul(G[t], tail[t]), T[t]));
    const Fr c0 = fr_add(s[0], k), c2 = s[2], c1 = fr_sub(fr_sub(s[1], s[0]), fr_add(s[2], k));
    if (!fr_eq(fr_add(fr_add(c0, c0), fr_add(c1, c2)), claim)) return false;   // (round 0 is where a wrong value shows)
    write_fr(tr, c0);
    write_fr(tr, c1);
    write_fr(tr, c2);
    r = rho[j] = pcs_squeeze(tr);
    const Fr rm = fr_to_mont(r);
    claim = fr_add(c0, fr_mul(rm, fr_add(c1, fr_mul(rm, c2))));
    for (size_t t = 0; t < m; t++)
        if ((size_t)sh.nvars[t] <= j) tail[t] = fr_mul(tail[t], fr_sub(fr_one_mont(), rm));
    return true;
}
bool PcsFoldProver::finish(const Shape& sh, const std::vector<Fr>& T, const std::vector<Fr>& G) {
    const size_t m = sh.nvars.size();
    Fr fin = fr_zero();
    for (size_t t = 0; t < m; t++) fin = fr_add(fin, fr_mul(fr_mul(G[t], tail[t]), T[t]));
    if (!fr_eq(fin, claim)) return false;
    for (size_t t = 0; t < m; t++) write_fr(tr, T[t]);
    return true;
}
std::vector<PcsJob> PcsFoldProver::body_jobs(const Shape& sh) {
    const Fr delta = pcs_squeeze(tr);
    std::vector<PcsJob> jobs(2);
    jobs[0].row0 = 0; jobs[0].nrows = sh.R; jobs[0].w = pcs_rho_powers(pcs_squeeze(tr), sh.R);
    jobs[1].row0 = 0; jobs[1].nrows = sh.R; jobs[1].w = combined_weights(sh, rho, delta);
    return jobs;
}
void PcsFoldProver::write_u(const Fr* u, size_t n) {
    for (size_t i = 0; i < n; i++) write_be32(tr.bytes, u[i]);
    pcs_absorb(tr, u, n);
}

std::vector<uint8_t> pcs_open_folded(const char* who, const Commitment& cm, const std::vector<PcsClaim>& claims, size_t Q) {
    const Shape& sh = cm.sh;
    const size_t C = sh.C(), n = claims.size(), V = pcs::fold_rounds(sh);
    const std::string w(who);
    if (!n) throw Error(w + ": a folded opening needs a claim");
    PcsFoldProver P(sh, cm.root(), claims, Q);
    // a running claim the sums do not meet: a value is wrong. The claims one by one, as pcs_open checks them, to name the lowest
    auto refuse = [&]() {
        for (size_t i = 0; i < n; i++) {
            const PcsClaim& cl = claims[i];
            std::vector<PcsJob> job(1);
            job[0].row0 = sh.off[cl.table];
            job[0].nrows = (size_t)1 << (sh.nvars[cl.table] - sh.c);
            job[0].w = pcs_eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
            std::vector<Fr> u(C);
            if (cm.ctx) pcs_combine_device(cm, job, u.data()); else pcs_combine_host(cm, job, u.data());
            const std::vector<Fr> lo = pcs_eq_table(cl.point.data(), (size_t)sh.c);
            if (!fr_eq(dot_fr(lo.data(), u.data(), C), cl.value))
                throw Error(w + ": claim " + std::to_string(i) + ": the value is not the evaluation of table " + std::to_string(cl.table) + " at the point");
        }
        throw Error(w + ": internal: the reduction does not meet its claim");
    };
    std::unique_ptr<PcsFoldSource> src;
    try {
        src = cm.ctx ? pcs_fold_source_device(who, cm, claims, P.bpow) : pcs_fold_source_host(cm, claims, P.bpow);
    } catch (const std::exception& e) {
        throw Error(w + ": " + e.what());
    }
    for (size_t j = 0; j < V; j++) {
        Fr s[3];
        src->step(j, P.r, s);
        if (!P.round(sh, j, s, src->T, src->G)) refuse();
    }
    src->step(V, P.r, nullptr);
    if (!P.finish(sh, src->T, src->G)) refuse();
    src.reset();   // (the device form's scratch is the context's arena, which the row combinations take next)
    const std::vector<PcsJob> jobs = P.body_jobs(sh);
    std::vector<Fr> u(2 * C);
    if (cm.ctx) pcs_combine_device(cm, jobs, u.data()); else pcs_combine_host(cm, jobs, u.data());
    write_u_and_queries(P.tr, cm, u, Q, pcs_folded_opening_bytes(sh, Q));
    if (P.tr.bytes.size() != pcs_folded_opening_bytes(sh, Q)) throw Error(w + ": internal: opening length");
    return std::move(P.tr.bytes);
}

PcsFoldedHeader pcs_folded_header(const Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof) {
    const size_t R = sh.R, n = claims.size(), m = sh.nvars.size(), V = pcs::fold_rounds(sh);
    PcsFoldedHeader H;
    std::vector<Fr> el(3 * V + m);
    for (size_t i = 0; i < el.size(); i++) {
        el[i] = pcs_read_be32(proof + 32 * i);
        if (fr_geq_p(el[i])) { H.noncanonical = 32 * i; return H; }
    }
    H.tr = pcs_start_transcript(sh, root, claims, Q, FOLD_TAG);
    const std::vector<Fr> bpow = pcs_rho_powers(pcs_squeeze(H.tr), n);
    Fr claim = fr_zero();
    for (size_t i = 0; i < n; i++) claim = fr_add(claim, fr_mul(bpow[i], claims[i].value));
    std::vector<Fr> rho(V), rm(V);
    for (size_t j = 0; j < V; j++) {
        const Fr c0 = el[3 * j], c1 = el[3 * j + 1], c2 = el[3 * j + 2];
        if (H.reason.empty() && !fr_eq(fr_add(fr_add(c0, c0), fr_add(c1, c2)), claim)) H.reason = "pcs: fold round " + std::to_string(j) + " does not match the running claim";
        pcs_absorb(H.tr, &el[3 * j], 3);
        rho[j] = pcs_squeeze(H.tr);
        rm[j] = fr_to_mont(rho[j]);
        claim = fr_add(c0, fr_mul(rm[j], fr_add(c1, fr_mul(rm[j], c2))));
    }
    const Fr* Y = el.data() + 3 * V;
    pcs_absorb(H.tr, Y, m);
    // sum_t Y_t g_t(rho[..v_t)) prod_{j >= v_t} (1 - rho_j), g_t from the claims: n V products
    std::vector<Fr> gt(m, fr_zero());
    for (size_t i = 0; i < n; i++) {
        Fr e = bpow[i];
        for (size_t b = 0; b < claims[i].point.size(); b++) e = fr_mul(e, eq1(fr_to_mont(claims[i].point[b]), rm[b]));
        gt[claims[i].table] = fr_add(gt[claims[i].table], e);
    }
    Fr fin = fr_zero();
    for (size_t t = 0; t < m; t++) {
        Fr e = gt[t];
        for (size_t j = (size_t)sh.nvars[t]; j < V; j++) e = fr_mul(e, fr_sub(fr_one_mont(), rm[j]));
        fin = fr_add(fin, fr_mul(e, Y[t]));
    }
    if (H.reason.empty() && !fr_eq(fin, claim)) H.reason = "pcs: fold final evaluation mismatch";
    // the body's one claim
    const Fr delta = pcs_squeeze(H.tr);
    H.rho_pw = pcs_rho_powers(pcs_squeeze(H.tr), R);
    H.w = combined_weights(sh, rho, delta);
    H.lo.assign(rho.begin(), rho.begin() + sh.c);
    H.y = fr_zero();
    const Fr dm = fr_to_mont(delta);
    Fr d = fr_one_mont();
    for (size_t t = 0; t < m; t++, d = fr_mul(d, dm)) H.y = fr_add(H.y, fr_mul(d, Y[t]));
    return H;
}

std::string pcs_verify_folded(const Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), hb = pcs_folded_header_bytes(sh);
    // 1. exact length
    const std::string bad_len = pcs::length_reason(len, pcs_folded_opening_bytes(sh, Q));
    if (!bad_len.empty()) return bad_len;
    // 2. every element below r, the header's first
    PcsFoldedHeader H = pcs_folded_header(sh, root, claims, Q, proof);
    if (H.noncanonical != ~(size_t)0) return pcs::reason_noncanonical(H.noncanonical);
    std::vector<Fr> u, cols;
    const std::string bad_word = read_body(sh, 1, Q, proof + hb, hb, u, cols);
    if (!bad_word.empty()) return bad_word;
    // 3., 4. the rounds and the final evaluation
    if (!H.reason.empty()) return H.reason;
    // 5. <u_1, eq(rho[..c))> == sum_t delta^t Y_t
    const std::vector<Fr> lo = pcs_eq_table(H.lo.data(), (size_t)sh.c);
    if (!fr_eq(dot_fr(lo.data(), u.data() + C, C), H.y)) return pcs::reason_evaluation(0);
    // 6. per query: path, proximity, the combined claim
    auto weights = [&](size_t) { return RowWeights{0, H.w}; };
    return check_queries(sh, root, H.tr, H.rho_pw, 1, weights, u, cols, Q, proof + hb);
}

}  // namespace bn
}  // namespace hg
