// Host side of the polynomial commitment (pcs.hpp): the host form of commit, the opening's transcript and byte layout (shared by
// both forms), the host verifier and the pieces it shares with the device verifier (pcs.hip); the folded opening's host flow (both
// forms), its host reduction, its host verifier and the header walk both folded verifiers share.
#include "pcs.hpp"
#include <algorithm>
#include <memory>

namespace hg {
namespace pcs {

Shape make_shape(const char* who, const uint32_t* nvars, size_t n_tables, size_t log2_row) {
    const std::string w(who);
    if (n_tables < 1 || n_tables > (size_t)MAX_TABLES) throw Error(w + ": between 1 and " + std::to_string(MAX_TABLES) + " tables");
    Shape sh;
    size_t total = 0;
    uint32_t vmin = nvars[0];
    for (size_t t = 0; t < n_tables; t++) {
        if (nvars[t] > (uint32_t)MAX_NVARS) throw Error(w + ": table " + std::to_string(t) + " has more than " + std::to_string(MAX_NVARS) + " variables");
        total += (size_t)1 << nvars[t];
        vmin = std::min(vmin, nvars[t]);
    }
    size_t c = log2_row;
    if (c == 0) {
        while ((c < 32) && (((size_t)1 << (2 * c)) < total)) c++;   // ceil(log2(total) / 2)
        c = std::min<size_t>(c, vmin);
    }
    if (c > (size_t)MAX_LOG2_ROW) throw Error(w + ": log2_row above " + std::to_string(MAX_LOG2_ROW));
    for (size_t t = 0; t < n_tables; t++)
        if (c > nvars[t]) throw Error(w + ": log2_row " + std::to_string(c) + " exceeds the " + std::to_string(nvars[t]) + " variables of table " + std::to_string(t));
    sh.c = (int)c;
    for (size_t t = 0; t < n_tables; t++) {
        sh.nvars.push_back((int)nvars[t]);
        sh.off.push_back(sh.R);
        sh.R += (size_t)1 << (nvars[t] - c);
    }
    return sh;
}

void leaf_hash(const u64* words, size_t R, uint8_t out[32]) {
    std::vector<u64> msg(R + 1);   // little-endian host: the words are their LE64 encoding
    msg[0] = 0;
    memcpy(msg.data() + 1, words, R * 8);
    keccak256(reinterpret_cast<const uint8_t*>(msg.data()), 8 * (R + 1), out);
}
void node_hash(const uint8_t* left, const uint8_t* right, uint8_t out[32]) {
    uint8_t msg[72] = {1, 0, 0, 0, 0, 0, 0, 0};
    memcpy(msg + 8, left, 32);
    memcpy(msg + 40, right, 32);
    keccak256(msg, 72, out);
}
std::vector<E2> eq_table(const E2* pt, size_t n) {
    std::vector<E2> t(1, e2_one());
    t.reserve((size_t)1 << n);
    for (size_t i = 0; i < n; i++) {
        const size_t h = t.size();
        t.resize(2 * h);
        for (size_t x = 0; x < h; x++) {
            const E2 hi = e2_mul(t[x], pt[i]);
            t[x + h] = hi;
            t[x] = e2_sub(t[x], hi);
        }
    }
    return t;
}

Commitment* commit_host(const Shape& sh, const u64* const* tables) {
    std::unique_ptr<Commitment> cm(new Commitment());
    cm->sh = sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    cm->rows.resize(R * C);
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t len = (size_t)1 << sh.nvars[t];
        for (size_t i = 0; i < len; i++)
            if (tables[t][i] >= GL_P) throw Error("hg_pcs_commit: table " + std::to_string(t) + " holds a word that is not below p");
        memcpy(cm->rows.data() + sh.off[t] * C, tables[t], len * 8);
    }
    cm->M.assign(R * N, 0);
    [[maybe_unused]] const int nt = hg_omp_threads();   // (the device pass of hipcc ignores the pragmas)
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long long r = 0; r < (long long)R; r++) {
        memcpy(cm->M.data() + r * N, cm->rows.data() + r * C, C * 8);
        ntt_host(cm->M.data() + r * N, sh.depth(), false);
    }
    cm->tree.resize(32 * (2 * N - 1));
    // eight adjacent columns (one cache line of every encoded row) per pass
    const size_t tile = std::min<size_t>(8, N);
#pragma omp parallel for schedule(static) num_threads(nt)
    for (long long j0 = 0; j0 < (long long)N; j0 += tile) {
        std::vector<u64> col(tile * R);
        for (size_t r = 0; r < R; r++)
            for (size_t jj = 0; jj < tile; jj++) col[jj * R + r] = cm->M[r * N + j0 + jj];
        for (size_t jj = 0; jj < tile; jj++) leaf_hash(col.data() + jj * R, R, cm->tree.data() + 32 * (j0 + jj));
    }
    for (int l = 1; l <= sh.depth(); l++) {
        const size_t cnt = N >> l;
        const uint8_t* below = cm->node(l - 1, 0);
        uint8_t* here = cm->tree.data() + (cm->node(l, 0) - cm->tree.data());
#pragma omp parallel for schedule(static) num_threads(nt) if (cnt >= 1024)
        for (long long i = 0; i < (long long)cnt; i++) node_hash(below + 64 * i, below + 64 * i + 32, here + 32 * i);
    }
    return cm.release();
}

void combine_host(const Commitment& cm, const std::vector<CombineJob>& jobs, E2* u) {
    const size_t C = cm.sh.C();
    for (size_t q = 0; q < jobs.size(); q++) {
        E2* out = u + q * C;
        for (size_t j = 0; j < C; j++) out[j] = e2_zero();
        for (size_t r = 0; r < jobs[q].nrows; r++) {
            const u64* row = cm.rows.data() + (jobs[q].row0 + r) * C;
            const E2 w = jobs[q].w[r];
            for (size_t j = 0; j < C; j++) out[j] = e2_add(out[j], e2_mul_f(w, row[j]));
        }
    }
}
void columns_host(const Commitment& cm, const std::vector<size_t>& js, u64* cols) {
    const size_t N = cm.sh.N(), R = cm.sh.R;
    for (size_t q = 0; q < js.size(); q++)
        for (size_t r = 0; r < R; r++) cols[q * R + r] = cm.M[r * N + js[q]];
}

// ---- the transcript both sides start from
static void put_le32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i))); }
static void put_le64(std::vector<uint8_t>& v, u64 x) { for (int i = 0; i < 8; i++) v.push_back((uint8_t)(x >> (8 * i))); }
FsTranscript start_transcript(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const char* tag) {
    FsTranscript tr;
    tr.absorb = true;
    tr.pending.assign(tag, tag + strlen(tag));
    tr.pending.insert(tr.pending.end(), root, root + 32);
    put_le32(tr.pending, (uint32_t)sh.c);
    put_le32(tr.pending, (uint32_t)sh.nvars.size());
    for (int v : sh.nvars) put_le32(tr.pending, (uint32_t)v);
    put_le32(tr.pending, (uint32_t)Q);
    put_le32(tr.pending, (uint32_t)claims.size());
    for (const Claim& cl : claims) {
        put_le32(tr.pending, (uint32_t)cl.table);
        for (const E2& x : cl.point) { put_le64(tr.pending, x.c0); put_le64(tr.pending, x.c1); }
        put_le64(tr.pending, cl.value.c0);
        put_le64(tr.pending, cl.value.c1);
    }
    return tr;
}
std::vector<E2> rho_powers(E2 rho, size_t R) {
    std::vector<E2> w(R);
    E2 x = e2_one();
    for (size_t r = 0; r < R; r++) { w[r] = x; x = e2_mul(x, rho); }
    return w;
}
static E2 dot_e(const E2* a, const E2* b, size_t n) {
    E2 s = e2_zero();
    for (size_t i = 0; i < n; i++) s = e2_add(s, e2_mul(a[i], b[i]));
    return s;
}

// the end of an opening, folded or not: the u vectors written and absorbed, the Q column indices squeezed, then per query the R column
// words and the siblings of the path
static void write_u_and_queries(FsTranscript& tr, const Commitment& cm, const std::vector<E2>& u, size_t Q) {
    const Shape& sh = cm.sh;
    const size_t N = sh.N(), R = sh.R;
    for (const E2& x : u) tr.write_e(x);
    std::vector<size_t> js(Q);
    for (size_t q = 0; q < Q; q++) js[q] = (size_t)(tr.squeeze_f() & (u64)(N - 1));
    std::vector<u64> cols(Q * R);
    if (Q) { if (cm.ctx) columns_device(cm, js, cols.data()); else columns_host(cm, js, cols.data()); }
    std::vector<uint8_t>& out = tr.bytes;
    out.reserve(out.size() + Q * (8 * R + 32 * (size_t)sh.depth()));
    for (size_t q = 0; q < Q; q++) {
        for (size_t r = 0; r < R; r++) {
            const u64 be = __builtin_bswap64(cols[q * R + r]);
            const uint8_t* b = reinterpret_cast<const uint8_t*>(&be);
            out.insert(out.end(), b, b + 8);
        }
        size_t idx = js[q];
        for (int l = 0; l < sh.depth(); l++, idx >>= 1) {
            const uint8_t* sib = cm.node(l, idx ^ 1);
            out.insert(out.end(), sib, sib + 32);
        }
    }
}

std::vector<uint8_t> open(const char* who, const Commitment& cm, const std::vector<Claim>& claims, size_t Q) {
    const Shape& sh = cm.sh;
    const size_t C = sh.C(), R = sh.R, n = claims.size();
    FsTranscript tr = start_transcript(sh, cm.root(), claims, Q);
    std::vector<CombineJob> jobs(n + 1);
    jobs[0].row0 = 0; jobs[0].nrows = R; jobs[0].w = rho_powers(tr.squeeze(), R);
    for (size_t i = 0; i < n; i++) {
        const Claim& cl = claims[i];
        jobs[i + 1].row0 = sh.off[cl.table];
        jobs[i + 1].nrows = (size_t)1 << (sh.nvars[cl.table] - sh.c);
        jobs[i + 1].w = eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
    }
    std::vector<E2> u((n + 1) * C);
    if (cm.ctx) combine_device(cm, jobs, u.data()); else combine_host(cm, jobs, u.data());
    for (size_t i = 0; i < n; i++) {   // the prover holds u_i: the check is free
        const std::vector<E2> lo = eq_table(claims[i].point.data(), (size_t)sh.c);
        if (!e2_eq(dot_e(u.data() + (i + 1) * C, lo.data(), C), claims[i].value))
            throw Error(std::string(who) + ": claim " + std::to_string(i) + ": the value is not the evaluation of table " + std::to_string(claims[i].table) + " at the point");
    }
    write_u_and_queries(tr, cm, u, Q);
    if (tr.bytes.size() != opening_bytes(sh, n, Q)) throw Error(std::string(who) + ": internal: opening length");
    return std::move(tr.bytes);
}

static u64 read_be64(const uint8_t* p) { u64 v; memcpy(&v, p, 8); return __builtin_bswap64(v); }

// ---- shared by verify and verify_device
std::string length_reason(size_t len, size_t want) {
    return len == want ? "" : "pcs: the opening has " + std::to_string(len) + " bytes, " + std::to_string(want) + " expected";
}
std::string length_reason(const Shape& sh, size_t n_claims, size_t Q, size_t len) { return length_reason(len, opening_bytes(sh, n_claims, Q)); }
void absorb_words(FsTranscript& tr, const u64* words, size_t count) {   // little-endian host: the words are their LE64 encoding
    const uint8_t* b = reinterpret_cast<const uint8_t*>(words);
    tr.pending.insert(tr.pending.end(), b, b + 8 * count);
}
std::vector<size_t> squeeze_indices(FsTranscript& tr, size_t N, size_t Q) {
    std::vector<size_t> js(Q);
    for (size_t q = 0; q < Q; q++) js[q] = (size_t)(tr.squeeze_f() & (u64)(N - 1));
    return js;
}
std::string reason_noncanonical(size_t byte) { return "pcs: non-canonical word at byte " + std::to_string(byte); }
std::string reason_evaluation(size_t claim) { return "pcs: evaluation mismatch at claim " + std::to_string(claim); }
std::string reason_merkle(size_t query) { return "pcs: Merkle path mismatch at query " + std::to_string(query); }
std::string reason_proximity(size_t query) { return "pcs: proximity mismatch at query " + std::to_string(query); }
std::string reason_claim(size_t claim, size_t query) { return "pcs: claim " + std::to_string(claim) + " inconsistent at query " + std::to_string(query); }

// ---- the body of an opening - n + 1 u vectors, then Q queries - as verify and verify_folded check it
// Reads the u vectors and the Q R column words of a body that starts at byte `base` of its opening -> "" or the reason of the lowest
// word that is not below p
static std::string read_body(const Shape& sh, size_t n, size_t Q, const uint8_t* body, size_t base, std::vector<E2>& u, std::vector<u64>& cols) {
    const size_t C = sh.C(), R = sh.R;
    const size_t u_words = 2 * C * (n + 1), q_bytes = 8 * R + 32 * (size_t)sh.depth();
    u.resize((n + 1) * C);
    for (size_t i = 0; i < u_words; i++) {
        const u64 v = read_be64(body + 8 * i);
        if (v >= GL_P) return reason_noncanonical(base + 8 * i);
        if (i & 1) u[i / 2].c1 = v; else u[i / 2].c0 = v;
    }
    cols.resize(Q * R);
    for (size_t q = 0; q < Q; q++)
        for (size_t r = 0; r < R; r++) {
            const size_t at = 8 * u_words + q * q_bytes + 8 * r;
            const u64 v = read_be64(body + at);
            if (v >= GL_P) return reason_noncanonical(base + at);
            cols[q * R + r] = v;
        }
    return "";
}
// a claim as the queries see it: its weights over the rows from row0 on
struct RowWeights { size_t row0; std::vector<E2> w; };
// The u vectors into the transcript, the column indices out of it, then per query: path, proximity (rho: the R powers), claims
static std::string check_queries(const Shape& sh, const uint8_t root[32], FsTranscript& tr, const std::vector<E2>& rho, const std::vector<RowWeights>& w,
                                 const std::vector<E2>& u, const std::vector<u64>& cols, size_t Q, const uint8_t* body) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R, n = w.size();
    const int depth = sh.depth();
    const size_t u_words = 2 * C * (n + 1), q_bytes = 8 * R + 32 * (size_t)depth;
    static_assert(sizeof(E2) == 16, "an E2 vector is read as its c0, c1 words");
    absorb_words(tr, reinterpret_cast<const u64*>(u.data()), 2 * u.size());
    const std::vector<size_t> js = squeeze_indices(tr, N, Q);
    if (!Q) return "";
    // Enc(u_i): the code acts on the c0 and the c1 coordinates separately
    std::vector<u64> enc(2 * (n + 1) * N, 0);
    [[maybe_unused]] const int nt = hg_omp_threads();
#pragma omp parallel for schedule(static) num_threads(nt) if (N >= 4096)
    for (long long i = 0; i < (long long)(n + 1); i++) {
        u64* a = enc.data() + 2 * i * N;
        for (size_t j = 0; j < C; j++) { a[j] = u[i * C + j].c0; a[N + j] = u[i * C + j].c1; }
        ntt_host(a, depth, false);
        ntt_host(a + N, depth, false);
    }
    for (size_t q = 0; q < Q; q++) {
        const u64* col = cols.data() + q * R;
        const uint8_t* sib = body + 8 * u_words + q * q_bytes + 8 * R;
        uint8_t h[32], nx[32];
        leaf_hash(col, R, h);
        size_t idx = js[q];
        for (int l = 0; l < depth; l++, idx >>= 1) {
            if (idx & 1) node_hash(sib + 32 * l, h, nx); else node_hash(h, sib + 32 * l, nx);
            memcpy(h, nx, 32);
        }
        if (memcmp(h, root, 32) != 0) return reason_merkle(q);
        E2 s = e2_zero();
        for (size_t r = 0; r < R; r++) s = e2_add(s, e2_mul_f(rho[r], col[r]));
        if (!e2_eq(s, e2(enc[js[q]], enc[N + js[q]]))) return reason_proximity(q);
        for (size_t i = 0; i < n; i++) {
            const u64* part = col + w[i].row0;
            E2 t = e2_zero();
            for (size_t r = 0; r < w[i].w.size(); r++) t = e2_add(t, e2_mul_f(w[i].w[r], part[r]));
            if (!e2_eq(t, e2(enc[2 * (i + 1) * N + js[q]], enc[(2 * (i + 1) + 1) * N + js[q]])))
                return reason_claim(i, q);
        }
    }
    return "";
}

std::string verify(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), R = sh.R, n = claims.size();
    // 1. exact length
    const std::string bad_len = length_reason(sh, n, Q, len);
    if (!bad_len.empty()) return bad_len;
    // 2. every element and column word below p
    std::vector<E2> u;
    std::vector<u64> cols;
    const std::string bad_word = read_body(sh, n, Q, proof, 0, u, cols);
    if (!bad_word.empty()) return bad_word;
    // 3. <u_i, eq(z_i[..c])> == y_i
    for (size_t i = 0; i < n; i++) {
        const std::vector<E2> lo = eq_table(claims[i].point.data(), (size_t)sh.c);
        if (!e2_eq(dot_e(u.data() + (i + 1) * C, lo.data(), C), claims[i].value)) return reason_evaluation(i);
    }
    // the challenges, then 4. per query: path, proximity, claims
    FsTranscript tr = start_transcript(sh, root, claims, Q);
    const std::vector<E2> rho = rho_powers(tr.squeeze(), R);
    std::vector<RowWeights> w(n);
    for (size_t i = 0; i < n; i++) w[i] = RowWeights{sh.off[claims[i].table], eq_table(claims[i].point.data() + sh.c, (size_t)(sh.nvars[claims[i].table] - sh.c))};
    return check_queries(sh, root, tr, rho, w, u, cols, Q, proof);
}

// ---- folded openings (hg.h "Folded openings")
static const char FOLD_TAG[] = "hg-pcs-fold-1";
// eq(z, r) for one coordinate: z r + (1 - z) (1 - r)
static E2 eq1(E2 z, E2 r) {
    const E2 zr = e2_mul(z, r);
    return e2_sub(e2_add(e2_add(zr, zr), e2_one()), e2_add(z, r));
}
// the weights of the combined row over all R rows: w[off_t + r] = delta^t eq(rho[c..v_t))[r]
static std::vector<E2> combined_weights(const Shape& sh, const std::vector<E2>& rho, E2 delta) {
    std::vector<E2> w(sh.R);
    E2 d = e2_one();
    for (size_t t = 0; t < sh.nvars.size(); t++, d = e2_mul(d, delta)) {
        const std::vector<E2> eq = eq_table(rho.data() + sh.c, (size_t)(sh.nvars[t] - sh.c));
        for (size_t r = 0; r < eq.size(); r++) w[sh.off[t] + r] = e2_mul(d, eq[r]);
    }
    return w;
}

// The host form of the reduction: every table and its g as E vectors, folded in place
struct FoldHost : FoldSource {
    std::vector<std::vector<E2>> t, g;
    void step(size_t j, E2 r, E2 s[3]) override {
        [[maybe_unused]] const int nt = hg_omp_threads();
        for (size_t x = 0; x < t.size(); x++) {
            std::vector<E2>&a = t[x], &b = g[x];
            if (a.empty()) continue;   // retired
            if (j > 0) {
                const size_t h = a.size() / 2;
                // (entry i is written after entries 2i and 2i + 1 were read and before any later pair is: in place, in order)
                for (size_t i = 0; i < h; i++) {
                    a[i] = e2_add(a[2 * i], e2_mul(r, e2_sub(a[2 * i + 1], a[2 * i])));
                    b[i] = e2_add(b[2 * i], e2_mul(r, e2_sub(b[2 * i + 1], b[2 * i])));
                }
                a.resize(h);
                b.resize(h);
            }
            if (a.size() == 1) {
                T[x] = a[0];
                G[x] = b[0];
                a.clear();
                b.clear();
            }
        }
        if (!s) return;
        s[0] = s[1] = s[2] = e2_zero();
        for (size_t x = 0; x < t.size(); x++) {
            const std::vector<E2>&a = t[x], &b = g[x];
            const long long h = (long long)(a.size() / 2);
            const int parts = h >= 4096 ? nt : 1;
            std::vector<E2> part(3 * (size_t)parts, e2_zero());
#pragma omp parallel for schedule(static) num_threads(parts)
            for (int q = 0; q < parts; q++) {
                E2 s0 = e2_zero(), s1 = e2_zero(), s2 = e2_zero();
                for (long long i = h * q / parts; i < h * (q + 1) / parts; i++) {
                    s0 = e2_add(s0, e2_mul(b[2 * i], a[2 * i]));
                    s1 = e2_add(s1, e2_mul(b[2 * i + 1], a[2 * i + 1]));
                    s2 = e2_add(s2, e2_mul(e2_sub(b[2 * i + 1], b[2 * i]), e2_sub(a[2 * i + 1], a[2 * i])));
                }
                part[3 * q] = s0; part[3 * q + 1] = s1; part[3 * q + 2] = s2;
            }
            for (int q = 0; q < parts; q++)
                for (int k = 0; k < 3; k++) s[k] = e2_add(s[k], part[3 * q + k]);
        }
    }
};
std::unique_ptr<FoldSource> fold_source_host(const Commitment& cm, const std::vector<Claim>& claims, const std::vector<E2>& bpow) {
    const Shape& sh = cm.sh;
    const size_t m = sh.nvars.size(), C = sh.C();
    std::unique_ptr<FoldHost> f(new FoldHost());
    f->T.assign(m, e2_zero());
    f->G.assign(m, e2_zero());
    f->t.resize(m);
    f->g.resize(m);
    for (size_t x = 0; x < m; x++) {
        const size_t len = (size_t)1 << sh.nvars[x];
        const u64* src = cm.rows.data() + sh.off[x] * C;
        f->t[x].resize(len);
        for (size_t i = 0; i < len; i++) f->t[x][i] = e2(src[i], 0);
        f->g[x].assign(len, e2_zero());
    }
    for (size_t i = 0; i < claims.size(); i++) {
        const std::vector<E2> eq = eq_table(claims[i].point.data(), claims[i].point.size());
        std::vector<E2>& g = f->g[claims[i].table];
        for (size_t k = 0; k < eq.size(); k++) g[k] = e2_add(g[k], e2_mul(bpow[i], eq[k]));
    }
    return f;
}

FoldProver::FoldProver(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q)
    : tr(start_transcript(sh, root, claims, Q, FOLD_TAG)), tail(sh.nvars.size(), e2_one()), rho(fold_rounds(sh)), claim(e2_zero()), r(e2_zero()) {
    bpow = rho_powers(tr.squeeze(), claims.size());
    for (size_t i = 0; i < claims.size(); i++) claim = e2_add(claim, e2_mul(bpow[i], claims[i].value));
}
bool FoldProver::round(const Shape& sh, size_t j, const E2 s[3], const std::vector<E2>& T, const std::vector<E2>& G) {
    const size_t m = sh.nvars.size();
    E2 k = e2_zero();   // the retired tables: K_t prod (1 - r_j') (1 - X)
    for (size_t t = 0; t < m; t++)
        if ((size_t)sh.nvars[t] <= j) k = e2_add(k, e2_mul(e2_mul(T[t], G[t]), tail[t]));
    const E2 c0 = e2_add(s[0], k), c2 = s[2], c1 = e2_sub(e2_sub(s[1], s[0]), e2_add(s[2], k));
    if (!e2_eq(e2_add(e2_add(c0, c0), e2_add(c1, c2)), claim)) return false;   // (round 0 is where a wrong value shows)
    tr.write_e(c0);
    tr.write_e(c1);
    tr.write_e(c2);
    r = rho[j] = tr.squeeze();
    claim = e2_add(c0, e2_mul(r, e2_add(c1, e2_mul(r, c2))));
    for (size_t t = 0; t < m; t++)
        if ((size_t)sh.nvars[t] <= j) tail[t] = e2_mul(tail[t], e2_sub(e2_one(), r));
    return true;
}
bool FoldProver::finish(const Shape& sh, const std::vector<E2>& T, const std::vector<E2>& G) {
    const size_t m = sh.nvars.size();
    E2 fin = e2_zero();
    for (size_t t = 0; t < m; t++) fin = e2_add(fin, e2_mul(e2_mul(T[t], G[t]), tail[t]));
    if (!e2_eq(fin, claim)) return false;
    for (size_t t = 0; t < m; t++) tr.write_e(T[t]);
    return true;
}
std::vector<CombineJob> FoldProver::body_jobs(const Shape& sh) {
    const E2 delta = tr.squeeze();
    std::vector<CombineJob> jobs(2);
    jobs[0].row0 = 0; jobs[0].nrows = sh.R; jobs[0].w = rho_powers(tr.squeeze(), sh.R);
    jobs[1].row0 = 0; jobs[1].nrows = sh.R; jobs[1].w = combined_weights(sh, rho, delta);
    return jobs;
}

void FoldProver::write_u(const E2* u, size_t n) {
    for (size_t i = 0; i < n; i++) tr.write_e(u[i]);
}

std::vector<uint8_t> open_folded(const char* who, const Commitment& cm, const std::vector<Claim>& claims, size_t Q) {
    const Shape& sh = cm.sh;
    const size_t C = sh.C(), n = claims.size(), V = fold_rounds(sh);
    const std::string w(who);
    if (!n) throw Error(w + ": a folded opening needs a claim");
    FoldProver P(sh, cm.root(), claims, Q);
    // a running claim the sums do not meet: a value is wrong. The claims one by one, as open checks them, to name the lowest
    auto refuse = [&]() {
        for (size_t i = 0; i < n; i++) {
            const Claim& cl = claims[i];
            std::vector<CombineJob> job(1);
            job[0].row0 = sh.off[cl.table];
            job[0].nrows = (size_t)1 << (sh.nvars[cl.table] - sh.c);
            job[0].w = eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
            std::vector<E2> u(C);
            if (cm.ctx) combine_device(cm, job, u.data()); else combine_host(cm, job, u.data());
            const std::vector<E2> lo = eq_table(cl.point.data(), (size_t)sh.c);
            if (!e2_eq(dot_e(u.data(), lo.data(), C), cl.value))
                throw Error(w + ": claim " + std::to_string(i) + ": the value is not the evaluation of table " + std::to_string(cl.table) + " at the point");
        }
        throw Error(w + ": internal: the reduction does not meet its claim");
    };
    std::unique_ptr<FoldSource> src;
    try {
        src = cm.ctx ? fold_source_device(cm, claims, P.bpow) : fold_source_host(cm, claims, P.bpow);
    } catch (const std::exception& e) {
        throw Error(w + ": " + e.what());
    }
    for (size_t j = 0; j < V; j++) {
        E2 s[3];
        src->step(j, P.r, s);
        if (!P.round(sh, j, s, src->T, src->G)) refuse();
    }
    src->step(V, P.r, nullptr);
    if (!P.finish(sh, src->T, src->G)) refuse();
    src.reset();   // (the device form's scratch is the context's arena, which the row combinations take next)
    const std::vector<CombineJob> jobs = P.body_jobs(sh);
    std::vector<E2> u(2 * C);
    if (cm.ctx) combine_device(cm, jobs, u.data()); else combine_host(cm, jobs, u.data());
    write_u_and_queries(P.tr, cm, u, Q);
    if (P.tr.bytes.size() != folded_opening_bytes(sh, Q)) throw Error(w + ": internal: opening length");
    return std::move(P.tr.bytes);
}

FoldedHeader folded_header(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof) {
    const size_t R = sh.R, n = claims.size(), m = sh.nvars.size(), V = fold_rounds(sh);
    FoldedHeader H;
    std::vector<E2> el(3 * V + m);
    for (size_t i = 0; i < 2 * el.size(); i++) {
        const u64 v = read_be64(proof + 8 * i);
        if (v >= GL_P) { H.noncanonical = 8 * i; return H; }
        if (i & 1) el[i / 2].c1 = v; else el[i / 2].c0 = v;
    }
    H.tr = start_transcript(sh, root, claims, Q, FOLD_TAG);
    const std::vector<E2> bpow = rho_powers(H.tr.squeeze(), n);
    E2 claim = e2_zero();
    for (size_t i = 0; i < n; i++) claim = e2_add(claim, e2_mul(bpow[i], claims[i].value));
    std::vector<E2> rho(V);
    for (size_t j = 0; j < V; j++) {
        const E2 c0 = el[3 * j], c1 = el[3 * j + 1], c2 = el[3 * j + 2];
        if (H.reason.empty() && !e2_eq(e2_add(e2_add(c0, c0), e2_add(c1, c2)), claim)) H.reason = "pcs: fold round " + std::to_string(j) + " does not match the running claim";
        absorb_words(H.tr, reinterpret_cast<const u64*>(&el[3 * j]), 6);
        const E2 r = rho[j] = H.tr.squeeze();
        claim = e2_add(c0, e2_mul(r, e2_add(c1, e2_mul(r, c2))));
    }
    const E2* Y = el.data() + 3 * V;
    absorb_words(H.tr, reinterpret_cast<const u64*>(Y), 2 * m);
    // sum_t Y_t g_t(rho[..v_t)) prod_{j >= v_t} (1 - rho_j), g_t from the claims: n V products
    std::vector<E2> gt(m, e2_zero());
    for (size_t i = 0; i < n; i++) {
        E2 e = bpow[i];
        for (size_t b = 0; b < claims[i].point.size(); b++) e = e2_mul(e, eq1(claims[i].point[b], rho[b]));
        gt[claims[i].table] = e2_add(gt[claims[i].table], e);
    }
    E2 fin = e2_zero();
    for (size_t t = 0; t < m; t++) {
        E2 e = e2_mul(Y[t], gt[t]);
        for (size_t j = (size_t)sh.nvars[t]; j < V; j++) e = e2_mul(e, e2_sub(e2_one(), rho[j]));
        fin = e2_add(fin, e);
    }
    if (H.reason.empty() && !e2_eq(fin, claim)) H.reason = "pcs: fold final evaluation mismatch";
    // the body's one claim
    const E2 delta = H.tr.squeeze();
    H.rho_pw = rho_powers(H.tr.squeeze(), R);
    H.w = combined_weights(sh, rho, delta);
    H.lo.assign(rho.begin(), rho.begin() + sh.c);
    H.y = e2_zero();
    E2 d = e2_one();
    for (size_t t = 0; t < m; t++, d = e2_mul(d, delta)) H.y = e2_add(H.y, e2_mul(d, Y[t]));
    return H;
}

std::string verify_folded(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), hb = folded_header_bytes(sh);
    // 1. exact length
    const std::string bad_len = length_reason(len, folded_opening_bytes(sh, Q));
    if (!bad_len.empty()) return bad_len;
    // 2. every element and column word below p, the header's first
    FoldedHeader H = folded_header(sh, root, claims, Q, proof);
    if (H.noncanonical != ~(size_t)0) return reason_noncanonical(H.noncanonical);
    std::vector<E2> u;
    std::vector<u64> cols;
    const std::string bad_word = read_body(sh, 1, Q, proof + hb, hb, u, cols);
    if (!bad_word.empty()) return bad_word;
    // 3., 4. the rounds and the final evaluation
    if (!H.reason.empty()) return H.reason;
    // 5. <u_1, eq(rho[..c))> == sum_t delta^t Y_t
    const std::vector<E2> lo = eq_table(H.lo.data(), (size_t)sh.c);
    if (!e2_eq(dot_e(u.data() + C, lo.data(), C), H.y)) return reason_evaluation(0);
    // 6. per query: path, proximity, the combined claim
    return check_queries(sh, root, H.tr, H.rho_pw, {RowWeights{0, H.w}}, u, cols, Q, proof + hb);
}


}  // namespace pcs
}  // namespace hg
