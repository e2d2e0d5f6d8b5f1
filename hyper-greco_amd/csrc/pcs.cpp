// Host side of the polynomial commitment (pcs.hpp): the host form of commit, the opening's transcript and byte layout (shared by
// both forms), the host verifier and the pieces it shares with the device verifier (pcs.hip).
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
FsTranscript start_transcript(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q) {
    FsTranscript tr;
    tr.absorb = true;
    static const char tag[] = "hg-pcs-1";
    tr.pending.assign(tag, tag + 8);
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

std::vector<uint8_t> open(const char* who, const Commitment& cm, const std::vector<Claim>& claims, size_t Q) {
    const Shape& sh = cm.sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R, n = claims.size();
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
    for (const E2& x : u) tr.write_e(x);
    std::vector<size_t> js(Q);
    for (size_t q = 0; q < Q; q++) js[q] = (size_t)(tr.squeeze_f() & (u64)(N - 1));
    std::vector<u64> cols(Q * R);
    if (Q) { if (cm.ctx) columns_device(cm, js, cols.data()); else columns_host(cm, js, cols.data()); }
    std::vector<uint8_t>& out = tr.bytes;
    out.reserve(opening_bytes(sh, n, Q));
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
    if (out.size() != opening_bytes(sh, n, Q)) throw Error(std::string(who) + ": internal: opening length");
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

std::string verify(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R, n = claims.size();
    const int depth = sh.depth();
    // 1. exact length
    const std::string bad_len = length_reason(sh, n, Q, len);
    if (!bad_len.empty()) return bad_len;
    // 2. every element and column word below p
    const size_t u_words = 2 * C * (n + 1), q_bytes = 8 * R + 32 * (size_t)depth;
    std::vector<E2> u((n + 1) * C);
    for (size_t i = 0; i < u_words; i++) {
        const u64 v = read_be64(proof + 8 * i);
        if (v >= GL_P) return reason_noncanonical(8 * i);
        if (i & 1) u[i / 2].c1 = v; else u[i / 2].c0 = v;
    }
    std::vector<u64> cols(Q * R);
    for (size_t q = 0; q < Q; q++)
        for (size_t r = 0; r < R; r++) {
            const size_t at = 8 * u_words + q * q_bytes + 8 * r;
            const u64 v = read_be64(proof + at);
            if (v >= GL_P) return reason_noncanonical(at);
            cols[q * R + r] = v;
        }
    // 3. <u_i, eq(z_i[..c])> == y_i
    for (size_t i = 0; i < n; i++) {
        const std::vector<E2> lo = eq_table(claims[i].point.data(), (size_t)sh.c);
        if (!e2_eq(dot_e(u.data() + (i + 1) * C, lo.data(), C), claims[i].value)) return reason_evaluation(i);
    }
    // the challenges
    FsTranscript tr = start_transcript(sh, root, claims, Q);
    const std::vector<E2> rho = rho_powers(tr.squeeze(), R);
    static_assert(sizeof(E2) == 16, "an E2 vector is read as its c0, c1 words");
    absorb_words(tr, reinterpret_cast<const u64*>(u.data()), 2 * u.size());
    const std::vector<size_t> js = squeeze_indices(tr, N, Q);
    // Enc(u_i): the code acts on the c0 and the c1 coordinates separately
    std::vector<u64> enc(2 * (n + 1) * N, 0);
    std::vector<std::vector<E2>> w(n);
    if (Q) {
        [[maybe_unused]] const int nt = hg_omp_threads();
#pragma omp parallel for schedule(static) num_threads(nt) if (N >= 4096)
        for (long long i = 0; i < (long long)(n + 1); i++) {
            u64* a = enc.data() + 2 * i * N;
            for (size_t j = 0; j < C; j++) { a[j] = u[i * C + j].c0; a[N + j] = u[i * C + j].c1; }
            ntt_host(a, depth, false);
            ntt_host(a + N, depth, false);
        }
        for (size_t i = 0; i < n; i++) w[i] = eq_table(claims[i].point.data() + sh.c, (size_t)(sh.nvars[claims[i].table] - sh.c));
    }
    // 4. per query: path, proximity, claims
    for (size_t q = 0; q < Q; q++) {
        const u64* col = cols.data() + q * R;
        const uint8_t* sib = proof + 8 * u_words + q * q_bytes + 8 * R;
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
            const u64* part = col + sh.off[claims[i].table];
            E2 t = e2_zero();
            for (size_t r = 0; r < w[i].size(); r++) t = e2_add(t, e2_mul_f(w[i][r], part[r]));
            if (!e2_eq(t, e2(enc[2 * (i + 1) * N + js[q]], enc[(2 * (i + 1) + 1) * N + js[q]])))
                return reason_claim(i, q);
        }
    }
    return "";
}

}  // namespace pcs
}  // namespace hg
