// Device form of the polynomial commitment (pcs.hpp): rows staged into the zero-padded 4C-stride matrix and encoded by the batched
// NTT, one Keccak-f[1600] state per thread for the column hashes and the tree, the E x F row combinations of an opening through
// the deferred-reduction accumulators, a gather of the opened columns. The handle owns the raw and the encoded matrix in HBM.
// The verifier of an opening reuses the encoding and the leaf hash and adds five kernels of its own.
// Every step has one kernel, written for a group of members and driven by a member or job table; the forms for a run (commit_device_batch,
// open_device_batch, verify_device_batch) launch it once over a group, whose matrices lie in one allocation that its handles share,
// and the forms for one (commit_device, combine_device, verify_device) launch it over a group of one from a host flow of their own.
// A commitment to tables that lie in HBM (commit_tables_enqueue: hg_secrets_commit_values, the encryption pipeline) stages them with one
// kernel of its own and goes on with the encoding, the leaf hash and the tree of commit_device.
#include <omp.h>
#include "pcs.hpp"
#include "prover.hpp"
#include "gl_wide.hpp"
#include "pcs_keccak.hpp"
#include "verifier_batch.hpp"

namespace hg {
namespace pcs {

constexpr int PCS_TPB = 256;

// ---- the kernels of a commitment, written for a group of G members of one shape (commit_device_batch); one commitment is a group
// of one. Member m's raw rows lie at rows + m R C, its encoded rows at M + m R N (so a group's encoding is one ntt_batch over G R
// rows) and its tree at trees + m tree_words.
// blockIdx.y = the member, its words grid-strided over blockIdx.x: M[r][j] = j < C ? rows[r][j] : 0 ahead of the encoding; a word that
// is not below p sets the member's flag
__global__ __launch_bounds__(PCS_TPB) void k_pcsb_stage(const u64* __restrict__ rows, u64* __restrict__ M, size_t R, int c, unsigned* __restrict__ flags) {
    const size_t total = R << (c + 2);
    const size_t C = (size_t)1 << c, Nm = ((size_t)4 << c) - 1;
    const u64* src = rows + (((size_t)blockIdx.y * R) << c);
    u64* dst = M + (size_t)blockIdx.y * total;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * PCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * PCS_TPB) {
        const size_t r = i >> (c + 2), j = i & Nm;
        u64 v = 0;
        if (j < C) { v = src[(r << c) + j]; bad |= v >= GL_P; }
        dst[i] = v;
    }
    if (bad) atomicOr(flags + blockIdx.y, 1u);
}

// Keccak256(LE64(0) || col[0] || col[stride] || .. || col[(R-1) * stride]) into the first four words of `a`: 17 message words per
// permutation, the prefix word first; padding 0x01 .. 0x80
__device__ __forceinline__ void leaf_absorb(const u64* __restrict__ col, size_t stride, size_t R, u64 (&a)[25]) {
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    const size_t words = R + 1;                       // message words, the prefix included
    const size_t blocks = words / RATE_WORDS + 1;     // the last block holds the rest (possibly nothing) and the padding
    for (size_t b = 0; b < blocks; b++) {
        const size_t base = b * RATE_WORDS;
#pragma unroll
        for (int i = 0; i < RATE_WORDS; i++) {
            const size_t idx = base + i;              // word 0 is LE64(0), word idx >= 1 is element idx - 1 of the column
            u64 w = 0;
            if (idx >= 1 && idx < words) w = col[(idx - 1) * stride];
            if (idx == words) w = 0x01;
            a[i] ^= w;
        }
        if (b + 1 == blocks) a[RATE_WORDS - 1] ^= 0x8000000000000000ull;
        keccak_f(a);
    }
}
// One thread per (member m, column j) of the encoded matrices (N = 2^depth columns), id = m N + j: the leaf hash of the member's
// M[0][j] .. M[R-1][j] into the leaves of its own tree. A wavefront reads 64 adjacent words of a row at a time.
__global__ __launch_bounds__(PCS_TPB) void k_pcsb_leaf_hash(const u64* __restrict__ M, size_t G, int depth, size_t R, u64* __restrict__ trees, size_t tree_words) {
    const size_t id = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (id >= G << depth) return;
    const size_t N = (size_t)1 << depth, m = id >> depth, j = id & (N - 1);
    u64 a[25];
    leaf_absorb(M + m * R * N + j, N, R, a);
    u64* out = trees + m * tree_words + 4 * j;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}
// One level of the trees, one thread per (member, node): node i of the 2^lg at word below_at + 8 * 2^lg of a tree =
// Keccak256(LE64(1) || nodes 2i and 2i + 1 of the 2 * 2^lg at word below_at), one permutation a node
__global__ __launch_bounds__(PCS_TPB) void k_pcsb_merkle(u64* __restrict__ trees, size_t tree_words, size_t below_at, int lg, size_t G) {
    const size_t id = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (id >= G << lg) return;
    const size_t count = (size_t)1 << lg;
    u64* below = trees + (id >> lg) * tree_words + below_at;
    merkle_node(below, below + 8 * count, id & (count - 1));
}
// One workgroup per member (blockIdx.x): the levels from `count` (<= PCS_TPB) nodes up to the root of its tree; the levels lie one
// behind the other in the tree buffer
__global__ __launch_bounds__(PCS_TPB) void k_pcsb_merkle_top(u64* __restrict__ trees, size_t tree_words, size_t below_at, size_t count) {
    u64* below = trees + (size_t)blockIdx.x * tree_words + below_at;
    while (count >= 1) {
        u64* here = below + 8 * count;   // `below` has 2 * count nodes of 4 words
        if (threadIdx.x < count) merkle_node(below, here, threadIdx.x);
        __syncthreads();
        below = here;
        count >>= 1;
    }
}

// sum_{r < nrows} w[r] * src[r << shift]. Products go into two accumulators (c0 and c1 of the weight) that are reduced every
// COMBINE_CHUNK rows: the carry counters of gl_wide.hpp stay below 2^8 for up to 127 products.
constexpr int COMBINE_CHUNK = 64;
__device__ __forceinline__ E2 dot_chunked(const u64* __restrict__ src, int shift, const E2* __restrict__ w, u64 nrows) {
    u64 s0 = 0, s1 = 0;
    for (u64 r0 = 0; r0 < nrows; r0 += COMBINE_CHUNK) {
        const u64 r1 = r0 + COMBINE_CHUNK < nrows ? r0 + COMBINE_CHUNK : nrows;
        WAcc A = wacc_zero(), B = wacc_zero();
        for (u64 r = r0; r < r1; r++) {
            const u64 x = src[r << shift];
            const E2 wr = w[r];
            wmac2(A, x, wr.c0, B, x, wr.c1);
        }
        s0 = gl_add(s0, wreduce(A));
        s1 = gl_add(s1, wreduce(B));
    }
    return e2(s0, s1);
}

// cols[q][r] = M[r][js[q]]
__global__ __launch_bounds__(PCS_TPB) void k_pcs_gather(const u64* __restrict__ M, size_t N, size_t R, const u64* __restrict__ js, u64* __restrict__ cols) {
    const size_t r = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (r >= R) return;
    cols[(size_t)blockIdx.y * R + r] = M[r * N + js[blockIdx.y]];
}

// ---- the kernels of the verifier, written for a group of G openings of one shape and one Q (verify_device_batch); one opening
// (verify_device) is a group of one, its device copy the set. What differs by member (its claim count, where its opening, u, columns,
// encoded rows, jobs and weights lie) is read from its descriptor, never derived from a flat id. Grids over queries are
// one-dimensional: Q reaches 65536, one more than a grid's y. A word of an opening only ever becomes a number; every index below comes
// from the shape, from the host's masked j_q or from table offsets the entry point validated. A result cell holds the lowest
// offending key (atomicMin), so the reason is the host's also where several checks fail at once.
constexpr u64 PCSV_NONE = ~(u64)0;   // a cell no thread lowered: nothing failed
__device__ __forceinline__ void cell_min(u64* cell, u64 v) { atomicMin(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)v); }
struct CombineDesc { u64 row0, nrows, woff; };   // a row combination: sum_{r < nrows} w[woff + r] * row_{row0 + r}
struct VbMember {
    u64 proof, u, cols, enc_row;               // word offsets of its opening in the set, of its u and of its columns; its first row of enc
    u64 n, claim0, job0;                       // its claims; the claims and the jobs (claims + 1 each) of the members before it
    u64 root_at, jobs_at, y_at, z_at, w_at;    // byte offsets in the group's staged copy: root, job descriptors, values, low coordinates, weights
};
struct VbGroup { u64 G, Q, R, q_words; int c, depth; };

// Big-endian words of an opening -> native words; blockIdx.y = the member, its words grid-strided over blockIdx.x. Word i < u_words is
// coordinate i & 1 of element i >> 1 of the u vectors: kept in u (as E2) and scattered into row 2 * (i >> (c+1)) + (i & 1) of the
// member's rows of the matrix the NTT encodes (zeroed beforehand). The others are the Q * R column words, query q at word
// u_words + q * q_words. cells[3m] = the lowest byte offset, within its opening, of a word that is not below p.
__global__ __launch_bounds__(PCS_TPB) void k_pcsvb_canon(const u64* __restrict__ set, const VbMember* __restrict__ mem, VbGroup g, u64* __restrict__ u,
                                                         u64* __restrict__ cols, u64* __restrict__ enc, u64* __restrict__ cells) {
    const VbMember M = mem[blockIdx.y];
    const int c = g.c;
    const size_t Q = g.Q, R = g.R, u_words = (M.n + 1) << (c + 1), total = u_words + Q * R, Cm = ((size_t)1 << c) - 1;
    const u64* proof = set + M.proof;
    u64* mu = u + M.u;
    u64* mcols = cols + M.cols;
    u64* menc = enc + (M.enc_row << (c + 2));
    u64 bad = PCSV_NONE;
    for (size_t i = (size_t)blockIdx.x * PCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * PCS_TPB) {
        size_t at = i;
        if (i >= u_words) { const size_t k = i - u_words, q = k / R; at = u_words + q * g.q_words + (k - q * R); }
        const u64 v = __builtin_bswap64(proof[at]);
        if (v >= GL_P && 8 * at < bad) bad = 8 * at;
        if (i < u_words) {
            const size_t e = i >> 1, row = 2 * (e >> c) + (i & 1);
            mu[i] = v;
            menc[(row << (c + 2)) + (e & Cm)] = v;
        } else {
            mcols[i - u_words] = v;
        }
    }
    if (bad != PCSV_NONE) cell_min(cells + 3 * blockIdx.y, bad);
}

// <ui, eq(z[..c])> != y, by one workgroup; the answer is thread 0's. eq(z, x) = prod_b (x_b ? z_b : 1 - z_b) is formed per entry: a
// thread keeps the factor of the low eight bits of x, which its entries share.
__device__ __forceinline__ bool eval_differs(const E2* __restrict__ ui, const E2* __restrict__ z, const E2* __restrict__ y, int c) {
    __shared__ E2 part[PCS_TPB];
    const size_t C = (size_t)1 << c;
    const int lob = c < 8 ? c : 8;
    E2 f = e2_one();
    for (int b = 0; b < lob; b++) f = e2_mul(f, (threadIdx.x >> b) & 1 ? z[b] : e2_sub(e2_one(), z[b]));
    E2 s = e2_zero();
    for (size_t x = threadIdx.x; x < C; x += PCS_TPB) {
        E2 gq = f;
        for (int b = 8; b < c; b++) gq = e2_mul(gq, (x >> b) & 1 ? z[b] : e2_sub(e2_one(), z[b]));
        s = e2_add(s, e2_mul(ui[x], gq));
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = PCS_TPB / 2; h >= 1; h >>= 1) {
        if (threadIdx.x < h) part[threadIdx.x] = e2_add(part[threadIdx.x], part[threadIdx.x + h]);
        __syncthreads();
    }
    return threadIdx.x == 0 && !e2_eq(part[0], *y);
}
// <u_i, eq(z_i[..c])> == y_i, one workgroup per (member, claim): block b belongs to the last member whose claim0 is <= b (a member
// without claims owns no block). cells[3m + 1] = the member's lowest failing claim.
__global__ __launch_bounds__(PCS_TPB) void k_pcsvb_eval(const VbMember* __restrict__ mem, unsigned G, int c, const u64* __restrict__ u, const char* __restrict__ stage,
                                                        u64* __restrict__ cells) {
    unsigned lo = 0, hi = G;
    while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].claim0 <= blockIdx.x) lo = mid; else hi = mid; }
    const VbMember M = mem[lo];
    const size_t i = blockIdx.x - M.claim0;
    if (i >= M.n) return;   // (uniform over the workgroup; the grid has exactly the claims of the group)
    if (eval_differs(reinterpret_cast<const E2*>(u + M.u) + ((i + 1) << c), reinterpret_cast<const E2*>(stage + M.z_at) + i * (size_t)c,
                     reinterpret_cast<const E2*>(stage + M.y_at) + i, c))
        cell_min(cells + 3 * lo + 1, (u64)i);
}

// One thread per (member m, query q), id = m Q + q: the leaf hash of its R column words -> leaves[id]
__global__ __launch_bounds__(PCS_TPB) void k_pcsvb_leaf(const VbMember* __restrict__ mem, VbGroup g, const u64* __restrict__ cols, u64* __restrict__ leaves) {
    const size_t id = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (id >= g.G * g.Q) return;
    const size_t m = id / g.Q, q = id - m * g.Q;
    u64 a[25];
    leaf_absorb(cols + mem[m].cols + q * g.R, 1, g.R, a);
    u64* out = leaves + 4 * id;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}

// One thread per (member, query, job): s[id] = sum_{r < nrows} w[woff + r] * col_q[row0 + r]. Member m owns the ids from Q job0_m;
// within it id - Q job0_m = q (n_m + 1) + job. Job 0 is the proximity combination (rho^r over the whole column), job 1 + i claim i's
// (eq(z_i[c..]) over the rows of its table).
__global__ __launch_bounds__(PCS_TPB) void k_pcsvb_dots(const VbMember* __restrict__ mem, VbGroup g, size_t total, const u64* __restrict__ cols,
                                                        const char* __restrict__ stage, E2* __restrict__ s) {
    const size_t id = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (id >= total) return;
    unsigned lo = 0, hi = (unsigned)g.G;
    while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].job0 * g.Q <= id) lo = mid; else hi = mid; }
    const VbMember M = mem[lo];
    const size_t local = id - M.job0 * g.Q, njobs = M.n + 1, q = local / njobs;
    const CombineDesc job = reinterpret_cast<const CombineDesc*>(stage + M.jobs_at)[local - q * njobs];
    s[id] = dot_chunked(cols + M.cols + q * g.R + job.row0, 0, reinterpret_cast<const E2*>(stage + M.w_at) + job.woff, job.nrows);
}

// One thread per (member m, query q), id = m Q + q, once the host has every member's column indices (js[id]): the path from the leaf
// hash over the c+2 siblings (32 raw bytes each behind the query's column words) against the member's root, then s[q][0] against
// Enc(u_0)[j_q], then s[q][1 + i] against Enc(u_i)[j_q]. enc: rows 2i, 2i + 1 of the member = the encoded c0, c1 coordinates of
// u_i. cells[3m + 2] = the member's lowest q (n_m + 2) + kind that failed: kind 0 the path, 1 proximity, 2 + i claim i.
__global__ __launch_bounds__(PCS_TPB) void k_pcsvb_query(const u64* __restrict__ set, const VbMember* __restrict__ mem, VbGroup g, const u64* __restrict__ leaves,
                                                         const E2* __restrict__ s, const u64* __restrict__ enc, const u64* __restrict__ js,
                                                         const char* __restrict__ stage, u64* __restrict__ cells) {
    const size_t id = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (id >= g.G * g.Q) return;
    const size_t m = id / g.Q, q = id - m * g.Q;
    const VbMember M = mem[m];
    const int depth = g.depth;
    const size_t N = (size_t)1 << depth, j = js[id], n = M.n, u_words = (n + 1) << (g.c + 1);
    const u64* sib = set + M.proof + u_words + q * g.q_words + g.R;
    const u64* root = reinterpret_cast<const u64*>(stage + M.root_at);
    u64 h[4] = {leaves[4 * id], leaves[4 * id + 1], leaves[4 * id + 2], leaves[4 * id + 3]};
    merkle_climb(h, sib, j, depth);
    u64* cell = cells + 3 * m + 2;
    const size_t key = q * (n + 2);
    if (h[0] != root[0] || h[1] != root[1] || h[2] != root[2] || h[3] != root[3]) { cell_min(cell, key); return; }
    const E2* sq = s + M.job0 * g.Q + q * (n + 1);
    const u64* menc = enc + (M.enc_row << depth);
    for (size_t i = 0; i <= n; i++)
        if (!e2_eq(sq[i], e2(menc[2 * i * N + j], menc[(2 * i + 1) * N + j]))) { cell_min(cell, key + 1 + i); return; }
}

// ---- the kernels of the prover's side of an opening, written for a group of items (open_device_batch); the row combinations of one
// opening (combine_device) are a job table of their own. What differs by item lies in three flat tables of the staged copy: a job a
// row combination (the proximity combination and one a claim, every member's behind the other), a claim an evaluation check, a
// member where its matrix, its u vectors and its opening image lie. Every grid is one-dimensional.
struct ObJob { const u64* src; u64 nrows, w_at, u_at; };     // its first raw row; the byte offset of its weights in the staged copy; where u goes (elements)
struct ObClaim { u64 u_at, z_at, y_at, member, claim; };      // its u_i (elements); byte offsets of the low coordinates and of the value
struct ObMember { const u64* M; u64 img, u, u_words; };       // its encoded matrix; word offsets of its image and of its u vectors; 2 C (n + 1)

// Row combinations: u[u_at + j] = sum_{r < nrows} w[r] * src[r][j] for the job of the block, a thread owns column j. Block b serves job
// b / cb, columns (b % cb) PCS_TPB .. ; the weights are uniform over the workgroup.
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_combine(int c, unsigned cb, const ObJob* __restrict__ jobs, const char* __restrict__ stage, E2* __restrict__ u) {
    const size_t C = (size_t)1 << c;
    const unsigned jq = blockIdx.x / cb;
    const size_t j = (size_t)(blockIdx.x - jq * cb) * PCS_TPB + threadIdx.x;
    if (j >= C) return;
    const ObJob job = jobs[jq];
    u[job.u_at + j] = dot_chunked(job.src + j, c, reinterpret_cast<const E2*>(stage + job.w_at), job.nrows);
}
// One workgroup per (member, claim): <u_i, eq(z_i[..c])> == y_i; cells[member] = its lowest failing claim
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_eval(const ObClaim* __restrict__ claims, int c, const E2* __restrict__ u, const char* __restrict__ stage,
                                                        u64* __restrict__ cells) {
    const ObClaim cl = claims[blockIdx.x];
    if (eval_differs(u + cl.u_at, reinterpret_cast<const E2*>(stage + cl.z_at), reinterpret_cast<const E2*>(stage + cl.y_at), c)) cell_min(cells + cl.member, cl.claim);
}
// Word i of the group's u vectors, big-endian, into its member's image: the member is the last one whose u offset is <= i
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_emit(const ObMember* __restrict__ mem, unsigned G, size_t total, const u64* __restrict__ u, u64* __restrict__ img) {
    for (size_t i = (size_t)blockIdx.x * PCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * PCS_TPB) {
        unsigned lo = 0, hi = G;
        while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].u <= i) lo = mid; else hi = mid; }
        img[mem[lo].img + (i - mem[lo].u)] = __builtin_bswap64(u[i]);
    }
}
// One thread per (member m, query q, row r), id = (m Q + q) R + r: M_m[r][j_q] big-endian at its place in the member's image.
// js[m Q + q] = j_q (masked by the host); js[G Q + m] != 0: the member takes part (it was not refused)
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_gather(const ObMember* __restrict__ mem, size_t G, size_t Q, size_t R, size_t N, size_t q_words,
                                                          const u64* __restrict__ js, u64* __restrict__ img) {
    const size_t id = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (id >= G * Q * R) return;
    const size_t m = id / (Q * R), k = id - m * Q * R, q = k / R, r = k - q * R;
    if (!js[G * Q + m]) return;
    const ObMember M = mem[m];
    img[M.img + M.u_words + q * q_words + r] = __builtin_bswap64(M.M[r * N + js[m * Q + q]]);
}

Commitment::~Commitment() {
    if (owner) return;   // (the matrices lie in a group's slab, which goes with its last handle)
    if (d_rows) (void)hipFree(d_rows);
    if (d_M) (void)hipFree(d_M);
}

static unsigned blocks_for(size_t n) { return (unsigned)((n + PCS_TPB - 1) / PCS_TPB); }

// The levels above the leaf hashes of the G trees at trees + m tree_words: one launch a level over every (member, node) while a level
// has more than PCS_TPB nodes, then one workgroup a member
void merkle_levels_device_batch(hipStream_t st, u64* d_trees, size_t tree_words, size_t N, size_t G) {
    size_t below_at = 0, count = N / 2;
    for (; count > (size_t)PCS_TPB; count >>= 1) {
        k_pcsb_merkle<<<blocks_for(G * count), PCS_TPB, 0, st>>>(d_trees, tree_words, below_at, __builtin_ctzll(count), G);
        below_at += 8 * count;
    }
    k_pcsb_merkle_top<<<(unsigned)G, PCS_TPB, 0, st>>>(d_trees, tree_words, below_at, count);
}
void merkle_levels_device(hipStream_t st, u64* d_tree, size_t N) { merkle_levels_device_batch(st, d_tree, 8 * N, N, 1); }

Commitment* commit_device(hg_ctx* ctx, const Shape& sh, const u64* const* tables) {
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    std::unique_ptr<Commitment> cm(new Commitment());
    cm->sh = sh;
    cm->ctx = ctx;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int log2n = sh.depth();
    if (R > 65535) throw Error("hg_pcs_commit: more than 65535 rows (choose a larger log2_row)");
    hip_check(hipMalloc((void**)&cm->d_rows, R * C * 8), "hipMalloc(pcs rows)");
    hip_check(hipMalloc((void**)&cm->d_M, R * N * 8), "hipMalloc(pcs encoded matrix)");
    u64* scratch = ctx->alloc_n<u64>(R * N);
    u64* W = ctx->alloc_n<u64>(N);
    u64* d_tree = ctx->alloc_n<u64>(4 * 2 * N);
    unsigned* d_flag = ctx->alloc_n<unsigned>(4);
    hip_check(hipMemsetAsync(d_flag, 0, 16, st), "memset");
    for (size_t t = 0; t < sh.nvars.size(); t++)
        hip_check(hipMemcpyAsync(cm->d_rows + sh.off[t] * C, tables[t], ((size_t)8) << sh.nvars[t], hipMemcpyHostToDevice, st), "upload tables");
    k_pcsb_stage<<<(unsigned)std::min<size_t>(blocks_for(R * N), 4096), PCS_TPB, 0, st>>>(cm->d_rows, cm->d_M, R, sh.c, d_flag);
    dev::powers_table(st, W, root_of_unity(log2n), N);
    dev::ntt_batch(st, cm->d_M, log2n, R, W, 1, scratch);
    k_pcsb_leaf_hash<<<blocks_for(N), PCS_TPB, 0, st>>>(cm->d_M, 1, log2n, R, d_tree, 8 * N);
    merkle_levels_device(st, d_tree, N);
    cm->tree.resize(32 * (2 * N - 1));
    unsigned flag = 0;
    hip_check(hipMemcpyAsync(cm->tree.data(), d_tree, cm->tree.size(), hipMemcpyDeviceToHost, st), "download tree");
    hip_check(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st), "download flag");
    hip_check(hipStreamSynchronize(st), "hg_pcs_commit: sync");
    hip_check(hipGetLastError(), "hg_pcs_commit: launch");
    if (flag) throw Error("hg_pcs_commit: a table holds a word that is not below p");
    return cm.release();
}

// ---- a commitment to tables that lie in HBM already (commit_tables_enqueue, commit_device_values): k_pcsb_stage and the copies
// ahead of it in one pass over the source tables. A unit is what a thread moves at a time: two words (16 bytes) when VEC, else one.
// A row has U = C / unit words units; 2^lanes_log2 = min(PCS_TPB, U) threads work on a row, so a workgroup holds PCS_TPB >> lanes_log2
// rows at a time, and a row of more than PCS_TPB units is walked in U >> lanes_log2 steps of which every workgroup of the row takes
// `split`-th part. The table of a row is looked up once a row (uniform over the workgroup as soon as a row has PCS_TPB units), from
// the descriptor in the kernel arguments. Per unit: one load, the word test, one store into rows, one into M and three zero stores
// into the padding of M's row; a wavefront's accesses are adjacent in every one of them.
struct StageTables {
    const u64* src[MAX_TABLES];
    unsigned off[MAX_TABLES + 1];   // first row of table t; off[nt] = R
    unsigned nt;
};
template <bool VEC>
__global__ __launch_bounds__(PCS_TPB) void k_pcs_stage_tables(const StageTables T, u64* __restrict__ rows, u64* __restrict__ M, int c, int lanes_log2, int split_log2,
                                                              unsigned* __restrict__ flag) {
    typedef typename std::conditional<VEC, ulonglong2, u64>::type Unit;
    const int u_log2 = VEC ? c - 1 : c;                      // log2 of the units in a row
    const int steps_log2 = u_log2 - lanes_log2 - split_log2;   // steps a workgroup walks along its row(s)
    const size_t R = T.off[T.nt];
    const unsigned lane = threadIdx.x & ((1u << lanes_log2) - 1), sub = threadIdx.x >> lanes_log2, rpb = PCS_TPB >> lanes_log2;
    const size_t groups = (R + rpb - 1) / rpb, items = groups << split_log2;
    bool bad = false;
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const size_t r = (item >> split_log2) * rpb + sub, part = item & (((size_t)1 << split_log2) - 1);
        if (r >= R) continue;
        unsigned t = 0;
        while (t + 1 < T.nt && T.off[t + 1] <= r) t++;
        const Unit* src = reinterpret_cast<const Unit*>(T.src[t] + ((r - T.off[t]) << c));
        Unit* drow = reinterpret_cast<Unit*>(rows + (r << c));
        Unit* mrow = reinterpret_cast<Unit*>(M + (r << (c + 2)));
        const size_t U = (size_t)1 << u_log2;
        for (size_t s = 0; s < ((size_t)1 << steps_log2); s++) {
            const size_t u = (((part << steps_log2) + s) << lanes_log2) + lane;
            const Unit v = src[u];
            Unit z;
            if constexpr (VEC) { bad |= v.x >= GL_P || v.y >= GL_P; z.x = 0; z.y = 0; }
            else { bad |= v >= GL_P; z = 0; }
            drow[u] = v;
            mrow[u] = v;
            mrow[U + u] = z;
            mrow[2 * U + u] = z;
            mrow[3 * U + u] = z;
        }
    }
    if (bad) atomicOr(flag, 1u);
}

void commit_tables_enqueue(hipStream_t st, const Shape& sh, const u64* const* d_tables, u64* d_rows, u64* d_M, u64* scratch, u64* W, u64* d_tree, unsigned* d_flag,
                           hg_ctx* prof, int cls) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R, nt = sh.nvars.size();
    const int log2n = sh.depth();
    if (nt > (size_t)MAX_TABLES || R > 65535) throw Error("commit_tables_enqueue: a shape the staging kernel does not take");
    StageTables T;
    bool vec = sh.c >= 1 && ((uintptr_t)d_rows & 15) == 0 && ((uintptr_t)d_M & 15) == 0;
    for (size_t t = 0; t < nt; t++) {
        T.src[t] = d_tables[t];
        T.off[t] = (unsigned)sh.off[t];
        vec = vec && ((uintptr_t)d_tables[t] & 15) == 0;
    }
    T.off[nt] = (unsigned)R;
    T.nt = (unsigned)nt;
    const int u_log2 = vec ? sh.c - 1 : sh.c, lanes_log2 = std::min(u_log2, 8);
    static_assert(PCS_TPB == 256, "2^8 threads a workgroup");
    const size_t groups = (R + (PCS_TPB >> lanes_log2) - 1) / (PCS_TPB >> lanes_log2);
    int split_log2 = 0;   // the workgroups of a row: enough of them for about 2048 in all
    while (split_log2 < u_log2 - lanes_log2 && (groups << split_log2) < 2048) split_log2++;
    const unsigned grid = (unsigned)std::min<size_t>(groups << split_log2, (size_t)1 << 20);
    auto begin = [&](double bytes) { if (prof) prof->prof_begin(cls, bytes); };
    auto end = [&] { if (prof) prof->prof_end(); };
    hip_check(hipMemsetAsync(d_flag, 0, 4, st), "memset");
    begin((double)R * (2 * C + N) * 8);
    if (vec) k_pcs_stage_tables<true><<<grid, PCS_TPB, 0, st>>>(T, d_rows, d_M, sh.c, lanes_log2, split_log2, d_flag);
    else k_pcs_stage_tables<false><<<grid, PCS_TPB, 0, st>>>(T, d_rows, d_M, sh.c, lanes_log2, split_log2, d_flag);
    end();
    begin((double)R * N * 32);
    dev::powers_table(st, W, root_of_unity(log2n), N);
    dev::ntt_batch(st, d_M, log2n, R, W, 1, scratch);
    end();
    begin((double)R * N * 8);
    k_pcsb_leaf_hash<<<blocks_for(N), PCS_TPB, 0, st>>>(d_M, 1, log2n, R, d_tree, 8 * N);
    end();
    begin((double)N * 96);
    merkle_levels_device(st, d_tree, N);
    end();
}

std::shared_ptr<void> slab_alloc(size_t bytes, u64** p) {
    std::shared_ptr<Slab> slab = std::make_shared<Slab>();
    hip_check(hipMalloc((void**)&slab->p, bytes), "hipMalloc(pcs rows and encoded matrices of a group)");
    slab->bytes = bytes;
    *p = slab->p;
    return slab;
}

Commitment* commit_device_values(hg_ctx* ctx, const Shape& sh, const u64* const* d_tables) {
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    std::unique_ptr<Commitment> cm(new Commitment());
    cm->sh = sh;
    cm->ctx = ctx;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    if (R > 65535) throw Error("more than 65535 rows (choose a larger log2_row)");
    hip_check(hipMalloc((void**)&cm->d_rows, R * C * 8), "hipMalloc(pcs rows)");
    hip_check(hipMalloc((void**)&cm->d_M, R * N * 8), "hipMalloc(pcs encoded matrix)");
    u64* scratch = ctx->alloc_n<u64>(R * N);
    u64* W = ctx->alloc_n<u64>(N);
    u64* d_tree = ctx->alloc_n<u64>(4 * 2 * N);
    unsigned* d_flag = ctx->alloc_n<unsigned>(4);
    unsigned flag = 0;
    DrainOne drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
    ctx->prof_stream = st;
    commit_tables_enqueue(st, sh, d_tables, cm->d_rows, cm->d_M, scratch, W, d_tree, d_flag, ctx, ctx->prof_class("pcs_commit_values", false));
    cm->tree.resize(32 * (2 * N - 1));
    hip_check(hipMemcpyAsync(cm->tree.data(), d_tree, cm->tree.size(), hipMemcpyDeviceToHost, st), "download tree");
    hip_check(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st), "download flag");
    hip_check(hipStreamSynchronize(st), "sync");
    hip_check(hipGetLastError(), "launch");
    ctx->prof_collect();
    if (flag) throw Error("a table holds a word that is not below p");
    return cm.release();
}

void combine_device(const Commitment& cm, const std::vector<CombineJob>& jobs, E2* u) {
    hg_ctx* ctx = cm.ctx;
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t C = cm.sh.C(), nj = jobs.size();
    if (nj > 65535) throw Error("hg_pcs_open: more than 65534 claims");
    // the job table and the weights in one staged copy; job q's u vector is the q-th
    size_t nw = 0;
    for (const CombineJob& j : jobs) nw += j.nrows;
    const size_t desc_bytes = (nj * sizeof(ObJob) + 15) & ~(size_t)15;
    std::vector<char> stage(desc_bytes + nw * sizeof(E2));
    ObJob* hd = reinterpret_cast<ObJob*>(stage.data());
    size_t w_at = desc_bytes;
    for (size_t q = 0; q < nj; q++) {
        hd[q].src = cm.d_rows + (jobs[q].row0 << cm.sh.c); hd[q].nrows = jobs[q].nrows; hd[q].w_at = w_at; hd[q].u_at = q * C;
        memcpy(stage.data() + w_at, jobs[q].w.data(), jobs[q].nrows * sizeof(E2));
        w_at += jobs[q].nrows * sizeof(E2);
    }
    char* d_stage = ctx->alloc_n<char>(stage.size());
    E2* d_u = ctx->alloc_n<E2>(nj * C);
    const unsigned cb = blocks_for(C);   // (at most 2^16 workgroups a job and, by the entry point, MAX_CLAIMS + 1 jobs: inside a grid's x)
    hip_check(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload weights");
    k_pcsob_combine<<<(unsigned)(nj * cb), PCS_TPB, 0, st>>>(cm.sh.c, cb, reinterpret_cast<const ObJob*>(d_stage), d_stage, d_u);
    hip_check(hipMemcpyAsync(u, d_u, nj * C * sizeof(E2), hipMemcpyDeviceToHost, st), "download combinations");
    hip_check(hipStreamSynchronize(st), "hg_pcs_open: sync");
    hip_check(hipGetLastError(), "hg_pcs_open: launch");
}

void columns_device(const Commitment& cm, const std::vector<size_t>& js, u64* cols) {
    hg_ctx* ctx = cm.ctx;
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    const size_t N = cm.sh.N(), R = cm.sh.R, Q = js.size();
    if (Q > 65535) throw Error("hg_pcs_open: more than 65535 queries on the device");
    std::vector<u64> hj(js.begin(), js.end());
    u64* d_js = ctx->alloc_n<u64>(Q);
    u64* d_cols = ctx->alloc_n<u64>(Q * R);
    hip_check(hipMemcpyAsync(d_js, hj.data(), Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
    k_pcs_gather<<<dim3(blocks_for(R), (unsigned)Q), PCS_TPB, 0, st>>>(cm.d_M, N, R, d_js, d_cols);
    hip_check(hipMemcpyAsync(cols, d_cols, Q * R * 8, hipMemcpyDeviceToHost, st), "download columns");
    hip_check(hipStreamSynchronize(st), "hg_pcs_open: sync");
    hip_check(hipGetLastError(), "hg_pcs_open: launch");
}

// ---- what the two verifiers share on the host: a member's block of the staged copy and the reading of its three result cells
// the entries of a member's weight tables: R powers of rho, then eq(z_i[c..]) over the rows of every claim's table
static size_t weights_of(const Shape& sh, const std::vector<Claim>& claims) {
    size_t nw = sh.R;
    for (const Claim& cl : claims) nw += (size_t)1 << (sh.nvars[cl.table] - sh.c);
    return nw;
}
// The block of a member of n claims and nw weights from byte `at` (a multiple of 16) of a staged copy on: root, job descriptors,
// values, the low coordinates of the points, weight tables. Into its descriptor -> the byte behind the block
static size_t member_block_layout(VbMember& d, const Shape& sh, size_t n, size_t nw, size_t at) {
    d.root_at = at;
    d.jobs_at = d.root_at + 32;
    d.y_at = d.jobs_at + (((n + 1) * sizeof(CombineDesc) + 15) & ~(size_t)15);
    d.z_at = d.y_at + n * sizeof(E2);
    d.w_at = d.z_at + n * (size_t)sh.c * sizeof(E2);
    return d.w_at + nw * sizeof(E2);
}
// fills the block -> the member's transcript, rho squeezed
static FsTranscript member_block_fill(char* h_stage, const VbMember& d, const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q) {
    const size_t R = sh.R;
    FsTranscript tr = start_transcript(sh, root, claims, Q);
    const std::vector<E2> rho = rho_powers(tr.squeeze(), R);
    memcpy(h_stage + d.root_at, root, 32);
    CombineDesc* hd = reinterpret_cast<CombineDesc*>(h_stage + d.jobs_at);
    E2* hy = reinterpret_cast<E2*>(h_stage + d.y_at);
    E2* hz = reinterpret_cast<E2*>(h_stage + d.z_at);
    E2* hw = reinterpret_cast<E2*>(h_stage + d.w_at);
    hd[0].row0 = 0; hd[0].nrows = R; hd[0].woff = 0;
    memcpy(hw, rho.data(), R * sizeof(E2));
    size_t off = R;
    for (size_t i = 0; i < claims.size(); i++) {
        const Claim& cl = claims[i];
        const std::vector<E2> w = eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
        hd[i + 1].row0 = sh.off[cl.table]; hd[i + 1].nrows = w.size(); hd[i + 1].woff = off;
        memcpy(hw + off, w.data(), w.size() * sizeof(E2));
        off += w.size();
        hy[i] = cl.value;
        memcpy(hz + i * (size_t)sh.c, cl.point.data(), (size_t)sh.c * sizeof(E2));
    }
    return tr;
}
// the host's order: a non-canonical word, the lowest claim whose evaluation fails, the lowest failing query; "" = accepted
static std::string cells_reason(const u64* cells, size_t n) {
    if (cells[0] != PCSV_NONE) return reason_noncanonical((size_t)cells[0]);
    if (cells[1] != PCSV_NONE) return reason_evaluation((size_t)cells[1]);
    if (cells[2] == PCSV_NONE) return "";
    const size_t q = (size_t)(cells[2] / (n + 2)), kind = (size_t)(cells[2] % (n + 2));
    return kind == 0 ? reason_merkle(q) : kind == 1 ? reason_proximity(q) : reason_claim(kind - 2, q);
}

// hg_pcs_verify_device: a group of one member, whose opening in the arena is the set. Everything but the last kernel needs no column
// index, so it is enqueued first and runs while the host hashes the u_i; the indices follow on the same stream, then the three
// result cells come back: one synchronisation.
std::string verify_device(hg_ctx* ctx, const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R, n = claims.size();
    const int depth = sh.depth();
    const std::string bad_len = length_reason(sh, n, Q, len);
    if (!bad_len.empty()) return bad_len;
    const size_t u_words = 2 * C * (n + 1), q_words = R + 4 * (size_t)depth, njobs = n + 1;
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    // the member's descriptor and its block in one staged copy
    const size_t nw = weights_of(sh, claims);
    VbMember desc{};   // (every offset into the set and the arena buffers is 0)
    desc.n = n;
    std::vector<char> stage(member_block_layout(desc, sh, n, nw, sizeof(VbMember)));
    static_assert(sizeof(VbMember) % 16 == 0, "the block starts at a multiple of 16");
    memcpy(stage.data(), &desc, sizeof(VbMember));
    FsTranscript tr = member_block_fill(stage.data(), desc, sh, root, claims, Q);
    const bool four_step = depth >= 8 && depth <= 16;
    u64 *d_proof, *d_u, *d_cols, *d_enc, *d_scratch = nullptr, *d_W, *d_leaves, *d_js, *d_cells;
    char* d_stage;
    E2* d_s;
    try {
        d_proof = ctx->alloc_n<u64>(len / 8);
        d_stage = ctx->alloc_n<char>(stage.size());
        d_u = ctx->alloc_n<u64>(u_words);
        d_cols = ctx->alloc_n<u64>(Q * R);
        d_enc = ctx->alloc_n<u64>(2 * njobs * N);
        if (four_step) d_scratch = ctx->alloc_n<u64>(2 * njobs * N);
        d_W = ctx->alloc_n<u64>(N);
        d_leaves = ctx->alloc_n<u64>(4 * Q);
        d_s = ctx->alloc_n<E2>(Q * njobs);
        d_js = ctx->alloc_n<u64>(Q);
        d_cells = ctx->alloc_n<u64>(4);
    } catch (const std::exception& e) {
        throw Error(std::string("the context's arena cannot hold the opening (") + e.what() + ")");
    }
    DrainOne drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
    const int cls = ctx->prof_class("pcs_verify", false);
    ctx->prof_stream = st;
    const VbMember* d_mem = reinterpret_cast<const VbMember*>(d_stage);
    const VbGroup vg{1, (u64)Q, (u64)R, (u64)q_words, sh.c, depth};
    hip_check(hipMemcpyAsync(d_proof, proof, len, hipMemcpyHostToDevice, st), "upload opening");
    hip_check(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload claims");
    hip_check(hipMemsetAsync(d_cells, 0xff, 32, st), "memset");
    hip_check(hipMemsetAsync(d_enc, 0, 2 * njobs * N * 8, st), "memset");
    ctx->prof_begin(cls, (double)(u_words + Q * R) * 24);
    k_pcsvb_canon<<<(unsigned)std::min<size_t>(blocks_for(u_words + Q * R), 4096), PCS_TPB, 0, st>>>(d_proof, d_mem, vg, d_u, d_cols, d_enc, d_cells);
    ctx->prof_end();
    if (n) {
        ctx->prof_begin(cls, (double)n * C * 16);
        k_pcsvb_eval<<<(unsigned)n, PCS_TPB, 0, st>>>(d_mem, 1, sh.c, d_u, d_stage, d_cells);
        ctx->prof_end();
    }
    ctx->prof_begin(cls, (double)njobs * N * 64);
    dev::powers_table(st, d_W, root_of_unity(depth), N);
    dev::ntt_batch(st, d_enc, depth, 2 * njobs, d_W, 1, d_scratch);
    ctx->prof_end();
    ctx->prof_begin(cls, (double)Q * R * 8);
    k_pcsvb_leaf<<<blocks_for(Q), PCS_TPB, 0, st>>>(d_mem, vg, d_cols, d_leaves);
    ctx->prof_end();
    ctx->prof_begin(cls, (double)Q * nw * 24);
    k_pcsvb_dots<<<blocks_for(Q * njobs), PCS_TPB, 0, st>>>(d_mem, vg, Q * njobs, d_cols, d_stage, d_s);
    ctx->prof_end();
    // the host's share, beside the kernels: the u_i into the transcript, the column indices out of it
    std::vector<u64> words(u_words);
    for (size_t i = 0; i < u_words; i++) { u64 v; memcpy(&v, proof + 8 * i, 8); words[i] = __builtin_bswap64(v); }
    absorb_words(tr, words.data(), u_words);
    const std::vector<size_t> js = squeeze_indices(tr, N, Q);
    const std::vector<u64> hj(js.begin(), js.end());
    hip_check(hipMemcpyAsync(d_js, hj.data(), Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
    ctx->prof_begin(cls, (double)Q * (32.0 * depth + 48.0 * njobs));
    k_pcsvb_query<<<blocks_for(Q), PCS_TPB, 0, st>>>(d_proof, d_mem, vg, d_leaves, d_s, d_enc, d_js, d_stage, d_cells);
    ctx->prof_end();
    u64 cells[4];
    hip_check(hipMemcpyAsync(cells, d_cells, 32, hipMemcpyDeviceToHost, st), "download verdict");
    hip_check(hipStreamSynchronize(st), "hg_pcs_verify_device: sync");
    hip_check(hipGetLastError(), "hg_pcs_verify_device: launch");
    ctx->prof_collect();
    return cells_reason(cells, n);
}

// hg_pcs_verify_device_batch. The items whose length is right are cut into groups (the option verify_batch_group, VB_PCS_BUDGET,
// the rows ntt_batch takes on its four-step path). A group: its openings gathered into a page-locked set on the host threads and
// copied on the upload stream; every member's transcript start, rho powers and weight tables written into one staged copy, one
// member a task; the index-free kernels, one launch each over all members; the members' u_i hashed on the host threads meanwhile;
// all indices up, the query kernel, three cells a member down: one synchronisation a group. The next group's openings are gathered
// and copied into the other set before that synchronisation, under this group's kernels.
std::vector<std::string> verify_device_batch(const char* who_c, hg_ctx* ctx, const Shape& sh, const std::vector<VerifyItem>& items, size_t Q) {
    const std::string who(who_c);
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int depth = sh.depth();
    const size_t q_words = R + 4 * (size_t)depth;
    const bool four_step = depth >= 8 && depth <= 16;
    std::vector<std::string> why(items.size());
    std::vector<size_t> good;   // the items that reach the device
    for (size_t i = 0; i < items.size(); i++) {
        why[i] = length_reason(sh, items[i].claims->size(), Q, items[i].len);
        if (why[i].empty()) good.push_back(i);
    }
    if (good.empty()) return why;
    // what a member takes: its opening in a set; u, columns, enc rows (and the scratch), leaves, s, indices in the arena
    auto rows_of = [](size_t n) { return 2 * (n + 1); };
    auto bytes_of = [&](size_t n, size_t len) {
        return len + 8 * (2 * C * (n + 1) + Q * R + rows_of(n) * N * (four_step ? 2 : 1) + 5 * Q) + 16 * Q * (n + 1);
    };
    size_t cap = VB_MAX_GROUP;
    if (ctx->verify_batch_group > 0) cap = std::min<size_t>(cap, (size_t)ctx->verify_batch_group);
    constexpr size_t NTT_ROWS = 65535;   // ntt_batch: the batch is the y extent of its four-step grids
    std::vector<std::pair<size_t, size_t>> groups;   // [first, last) of good
    for (size_t a = 0; a < good.size();) {
        size_t b = a, bytes = 0, rows = 0;
        while (b < good.size() && b - a < cap) {
            const size_t n = items[good[b]].claims->size();
            if (b > a && (bytes + bytes_of(n, items[good[b]].len) > VB_PCS_BUDGET || (four_step && rows + rows_of(n) > NTT_ROWS))) break;
            bytes += bytes_of(n, items[good[b]].len);
            rows += rows_of(n);
            b++;
        }
        groups.push_back({a, b});
        a = b;
    }
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    hipStream_t st = ctx->stream;
    std::vector<u64> hj, cells;   // (declared ahead of the guard: copies of them may be queued when it drains)
    DrainOne drain_up{B->up}, drain{st};   // (the upload stream as well: no kernel on a set left behind)
    hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());        // (the device pass of hipcc ignores the pragmas)
    const int cls = ctx->prof_class("pcs_verify_batch", false);
    ctx->prof_stream = st;

    struct Member { size_t idx, n, nw; FsTranscript tr; std::string error; };
    // the openings of group g into set g & 1, at word offsets that the descriptors repeat
    auto proof_offsets = [&](size_t g) {
        std::vector<size_t> off;
        size_t at = 0;
        for (size_t x = groups[g].first; x < groups[g].second; x++) { off.push_back(at); at += items[good[x]].len / 8; }
        off.push_back(at);
        return off;
    };
    auto stage = [&](size_t g) {
        const std::vector<size_t> off = proof_offsets(g);
        std::vector<BatchBlob> blobs;
        for (size_t x = groups[g].first; x < groups[g].second; x++) blobs.push_back(BatchBlob{items[good[x]].proof, items[good[x]].len, off[x - groups[g].first]});
        batch_stage_blobs(B, (int)(g & 1), blobs, off.back(), nthr, who_c);
    };
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr
    double t_stage = omp_get_wtime();
    stage(0);
    t_stage = omp_get_wtime() - t_stage;
    for (size_t g = 0; g < groups.size(); g++) {
        const double t0 = omp_get_wtime();
        const size_t G = groups[g].second - groups[g].first;
        const int set = (int)(g & 1);
        std::vector<Member> mem(G);
        std::vector<VbMember> desc(G);
        const std::vector<size_t> poff = proof_offsets(g);
        // the layout of the staged copy: the descriptors, then every member's block, and of the arena buffers
        size_t at = (G * sizeof(VbMember) + 15) & ~(size_t)15, u_at = 0, row_at = 0, claim_at = 0;
        for (size_t m = 0; m < G; m++) {
            Member& x = mem[m];
            const VerifyItem& it = items[good[groups[g].first + m]];
            x.idx = good[groups[g].first + m];
            x.n = it.claims->size();
            x.nw = weights_of(sh, *it.claims);
            VbMember& d = desc[m];
            d.proof = poff[m]; d.u = u_at; d.cols = m * Q * R; d.enc_row = row_at;
            d.n = x.n; d.claim0 = claim_at; d.job0 = claim_at + m;
            at = member_block_layout(d, sh, x.n, x.nw, at);
            u_at += 2 * C * (x.n + 1);
            row_at += rows_of(x.n);
            claim_at += x.n;
        }
        const size_t stage_bytes = at, u_total = u_at, rows = row_at, claims_total = claim_at, jobs_total = claim_at + G;
        char* h_stage = batch_desc_host(B, stage_bytes);   // (the previous group's copy of it was waited for)
        memcpy(h_stage, desc.data(), G * sizeof(VbMember));
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                const VerifyItem& it = items[x.idx];
                x.tr = member_block_fill(h_stage, desc[mq], sh, it.root, *it.claims, Q);
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        u64 *d_u, *d_cols, *d_enc, *d_scratch = nullptr, *d_W, *d_leaves, *d_js, *d_cells;
        char* d_stage;
        E2* d_s;
        try {
            d_stage = ctx->alloc_n<char>(stage_bytes);
            d_u = ctx->alloc_n<u64>(u_total);
            d_cols = ctx->alloc_n<u64>(G * Q * R);
            d_enc = ctx->alloc_n<u64>(rows * N);
            if (four_step) d_scratch = ctx->alloc_n<u64>(rows * N);
            d_W = ctx->alloc_n<u64>(N);
            d_leaves = ctx->alloc_n<u64>(4 * G * Q);
            d_s = ctx->alloc_n<E2>(Q * jobs_total);
            d_js = ctx->alloc_n<u64>(G * Q);
            d_cells = ctx->alloc_n<u64>(3 * G);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold " + (G == 1 ? "the opening at index " + std::to_string(mem[0].idx) : "a group of " + std::to_string(G) + " openings: lower verify_batch_group") +
                        " (" + e.what() + ")");
        }
        const u64* d_set = B->d_in[set];
        const VbMember* d_mem = reinterpret_cast<const VbMember*>(d_stage);
        const VbGroup vg{(u64)G, (u64)Q, (u64)R, (u64)q_words, sh.c, depth};
        size_t words_max = 0, nw_total = 0;
        for (const Member& x : mem) { words_max = std::max(words_max, 2 * C * (x.n + 1) + Q * R); nw_total += x.nw; }
        hip_check(hipStreamWaitEvent(st, B->ev[set], 0), "hipStreamWaitEvent");   // the set's openings are up
        hip_check(hipMemcpyAsync(d_stage, h_stage, stage_bytes, hipMemcpyHostToDevice, st), "upload claims");
        hip_check(hipMemsetAsync(d_cells, 0xff, 3 * G * 8, st), "memset");
        hip_check(hipMemsetAsync(d_enc, 0, rows * N * 8, st), "memset");
        ctx->prof_begin(cls, (double)(u_total + G * Q * R) * 24);
        k_pcsvb_canon<<<dim3((unsigned)std::min<size_t>(blocks_for(words_max), 1024), (unsigned)G), PCS_TPB, 0, st>>>(d_set, d_mem, vg, d_u, d_cols, d_enc, d_cells);
        ctx->prof_end();
        if (claims_total) {
            ctx->prof_begin(cls, (double)claims_total * C * 16);
            k_pcsvb_eval<<<(unsigned)claims_total, PCS_TPB, 0, st>>>(d_mem, (unsigned)G, sh.c, d_u, d_stage, d_cells);
            ctx->prof_end();
        }
        ctx->prof_begin(cls, (double)rows * N * 32);
        dev::powers_table(st, d_W, root_of_unity(depth), N);
        dev::ntt_batch(st, d_enc, depth, rows, d_W, 1, d_scratch);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * Q * R * 8);
        k_pcsvb_leaf<<<blocks_for(G * Q), PCS_TPB, 0, st>>>(d_mem, vg, d_cols, d_leaves);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)Q * nw_total * 24);
        k_pcsvb_dots<<<blocks_for(Q * jobs_total), PCS_TPB, 0, st>>>(d_mem, vg, Q * jobs_total, d_cols, d_stage, d_s);
        ctx->prof_end();
        // the host's share, beside the kernels: every member's u_i into its transcript, its column indices out of it
        const double t2 = omp_get_wtime();
        hj.assign(G * Q, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                const uint8_t* proof = items[x.idx].proof;
                const size_t u_words = 2 * C * (x.n + 1);
                std::vector<u64> words(u_words);
                for (size_t i = 0; i < u_words; i++) { u64 v; memcpy(&v, proof + 8 * i, 8); words[i] = __builtin_bswap64(v); }
                absorb_words(x.tr, words.data(), u_words);
                const std::vector<size_t> js = squeeze_indices(x.tr, N, Q);
                for (size_t q = 0; q < Q; q++) hj[(size_t)mq * Q + q] = js[q];
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        const double t3 = omp_get_wtime();
        hip_check(hipMemcpyAsync(d_js, hj.data(), G * Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
        ctx->prof_begin(cls, (double)G * Q * 32.0 * depth + (double)Q * jobs_total * 48.0);
        k_pcsvb_query<<<blocks_for(G * Q), PCS_TPB, 0, st>>>(d_set, d_mem, vg, d_leaves, d_s, d_enc, d_js, d_stage, d_cells);
        ctx->prof_end();
        cells.assign(3 * G, 0);
        hip_check(hipMemcpyAsync(cells.data(), d_cells, 3 * G * 8, hipMemcpyDeviceToHost, st), "download verdicts");
        const double t4 = omp_get_wtime();
        if (g + 1 < groups.size()) stage(g + 1);   // into the other set, under this group's kernels
        const double t5 = omp_get_wtime();
        hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
        if (times)
            fprintf(stderr, "[hg pcs] group %zu of %zu members: gather and copy of its openings %.2f ms, transcripts and weights %.2f, enqueue %.2f, hash %.2f, "
                            "query enqueue %.2f, next group's gather %.2f, wait %.2f\n", g, G, t_stage * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3,
                    (t5 - t4) * 1e3, (omp_get_wtime() - t5) * 1e3);
        t_stage = t5 - t4;
        hip_check(hipGetLastError(), (who + ": launch").c_str());
        ctx->prof_collect();
        for (size_t m = 0; m < G; m++) why[mem[m].idx] = cells_reason(cells.data() + 3 * m, mem[m].n);
    }
    return why;
}

// hg_pcs_commit_batch. A group: one allocation for its members' raw and encoded rows, the tables uploaded straight into it, then
// k_pcsb_stage, one ntt_batch over G R rows, the leaf hashes, the tree levels (per level while a level has more than PCS_TPB nodes,
// then one workgroup a member), one download of all trees and flags, one synchronisation.
std::vector<Commitment*> commit_device_batch(const char* who_c, hg_ctx* ctx, const Shape& sh, const u64* const* tables, size_t n) {
    const std::string who(who_c);
    const size_t C = sh.C(), N = sh.N(), R = sh.R, nt = sh.nvars.size();
    const int log2n = sh.depth();
    if (R > 65535) throw Error(who + ": more than 65535 rows (choose a larger log2_row)");
    const size_t tree_words = 8 * N;   // 2N nodes of 4 words: the 2N - 1 of a tree and one unused
    // what a member takes: its rows and encoded rows in the slab; the NTT scratch and its tree in the arena
    const size_t member_bytes = 8 * (R * C + 2 * R * N + tree_words) + 4;
    const std::vector<std::pair<size_t, size_t>> groups = cut_groups(ctx, n, [&](size_t) { return member_bytes; }, R, 65535);   // ntt_batch: the batch is the y extent of its four-step grids
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    std::vector<std::unique_ptr<Commitment>> made;
    std::vector<u64> h_out;   // (declared ahead of the guard: a copy into it may be queued when it drains)
    DrainOne drain{st};
    hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    const int cls = ctx->prof_class("pcs_commit_batch", false);
    ctx->prof_stream = st;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr
    for (const auto& grp : groups) {
        const double t0 = omp_get_wtime();
        const size_t first = grp.first, G = grp.second - grp.first;
        std::shared_ptr<Slab> slab = std::make_shared<Slab>();
        hip_check(hipMalloc((void**)&slab->p, G * (R * C + R * N) * 8), "hipMalloc(pcs rows and encoded matrices of a group)");
        u64* d_rows = slab->p;
        u64* d_M = slab->p + G * R * C;
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        u64 *scratch, *W, *d_out;
        const size_t out_words = G * tree_words + (G + 1) / 2;   // the trees, then one 32-bit flag a member
        try {
            scratch = ctx->alloc_n<u64>(G * R * N);
            W = ctx->alloc_n<u64>(N);
            d_out = ctx->alloc_n<u64>(out_words);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold a group of " + std::to_string(G) + " commitments: lower verify_batch_group (" + e.what() + ")");
        }
        unsigned* d_flags = reinterpret_cast<unsigned*>(d_out + G * tree_words);
        hip_check(hipMemsetAsync(d_flags, 0, ((G + 1) / 2) * 8, st), "memset");
        for (size_t m = 0; m < G; m++)
            for (size_t t = 0; t < nt; t++)
                hip_check(hipMemcpyAsync(d_rows + (m * R + sh.off[t]) * C, tables[(first + m) * nt + t], ((size_t)8) << sh.nvars[t], hipMemcpyHostToDevice, st), "upload tables");
        const double t2 = omp_get_wtime();
        ctx->prof_begin(cls, (double)G * R * (C + N) * 8);
        k_pcsb_stage<<<dim3((unsigned)std::min<size_t>(blocks_for(R * N), (4096 + G - 1) / G), (unsigned)G), PCS_TPB, 0, st>>>(d_rows, d_M, R, sh.c, d_flags);   // about 4096 workgroups in all; G in the grid's y: cut_groups keeps it at VB_MAX_GROUP = 64 or below
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * R * N * 32);
        dev::powers_table(st, W, root_of_unity(log2n), N);
        dev::ntt_batch(st, d_M, log2n, G * R, W, 1, scratch);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * R * N * 8);
        k_pcsb_leaf_hash<<<blocks_for(G * N), PCS_TPB, 0, st>>>(d_M, G, log2n, R, d_out, tree_words);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * N * 96);
        merkle_levels_device_batch(st, d_out, tree_words, N, G);
        ctx->prof_end();
        h_out.resize(out_words);
        hip_check(hipMemcpyAsync(h_out.data(), d_out, out_words * 8, hipMemcpyDeviceToHost, st), "download trees and flags");
        const double t3 = omp_get_wtime();
        hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
        const double t4 = omp_get_wtime();
        hip_check(hipGetLastError(), (who + ": launch").c_str());
        ctx->prof_collect();
        const unsigned* flags = reinterpret_cast<const unsigned*>(h_out.data() + G * tree_words);
        for (size_t m = 0; m < G; m++)
            if (flags[m]) throw Error(who + ": index " + std::to_string(first + m) + ": a table holds a word that is not below p");
        for (size_t m = 0; m < G; m++) {
            std::unique_ptr<Commitment> cm(new Commitment());
            cm->sh = sh;
            cm->ctx = ctx;
            cm->d_rows = d_rows + m * R * C;
            cm->d_M = d_M + m * R * N;
            cm->owner = slab;
            const uint8_t* tree = reinterpret_cast<const uint8_t*>(h_out.data() + m * tree_words);
            cm->tree.assign(tree, tree + 32 * (2 * N - 1));
            made.push_back(std::move(cm));
        }
        if (times)
            fprintf(stderr, "[hg pcs] commit group of %zu members: allocation %.2f ms, uploads %.2f, enqueue %.2f, wait %.2f, trees into the handles %.2f\n", G, (t1 - t0) * 1e3,
                    (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (omp_get_wtime() - t4) * 1e3);
    }
    std::vector<Commitment*> out;
    for (auto& cm : made) out.push_back(cm.release());
    return out;
}

// hg_pcs_open_batch. A group: the host threads write every member's transcript start, rho powers, weight tables and table entries into
// one staged copy; the combinations, the evaluation checks and the big-endian u vectors run as one launch each; the u vectors and one
// cell a member come back (first synchronisation); the host threads hash each member's u_i, one member a thread; all indices go up,
// the gather writes the opened columns into the images, the images come back (second synchronisation); the host copies the siblings
// from each handle's tree into the gaps.
std::vector<Opened> open_device_batch(const char* who_c, const char* single, hg_ctx* ctx, const std::vector<OpenItem>& items, size_t Q) {
    const std::string who(who_c);
    std::vector<Opened> res(items.size());
    if (items.empty()) return res;
    const Shape& sh = items[0].cm->sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int depth = sh.depth();
    const size_t q_words = R + 4 * (size_t)depth;
    auto align16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    auto nw_of = [&](const std::vector<Claim>& cl) { size_t nw = R; for (const Claim& x : cl) nw += (size_t)1 << (sh.nvars[x.table] - sh.c); return nw; };
    // what a member takes: its block of the staged copy, its u vectors and its image in the arena, its indices
    auto bytes_of = [&](size_t i) {
        const std::vector<Claim>& cl = *items[i].claims;
        return sizeof(ObMember) + (cl.size() + 1) * sizeof(ObJob) + cl.size() * (sizeof(ObClaim) + (size_t)(sh.c + 1) * sizeof(E2)) + nw_of(cl) * sizeof(E2) + 64 +
               16 * C * (cl.size() + 1) + opening_bytes(sh, cl.size(), Q) + 8 * Q + 16;
    };
    const std::vector<std::pair<size_t, size_t>> groups = cut_groups(ctx, items.size(), bytes_of, 0, 0);
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    hipStream_t st = ctx->stream;
    std::vector<u64> hj;   // (declared ahead of the guard: a copy of it may be queued when it drains)
    DrainOne drain{st};
    hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());        // (the device pass of hipcc ignores the pragmas)
    const int cls = ctx->prof_class("pcs_open_batch", false);
    ctx->prof_stream = st;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr

    struct Member { size_t idx, n, nw, job0, claim0, y_at, z_at, w_at, img, u, u_words, len; FsTranscript tr; bool refused = false; std::string error; };
    for (size_t g = 0; g < groups.size(); g++) {
        const double t0 = omp_get_wtime();
        const size_t G = groups[g].second - groups[g].first;
        std::vector<Member> mem(G);
        // the layout of the staged copy: the three tables, then every member's values, low coordinates and weights
        size_t jobs_total = 0, claims_total = 0, u_total = 0, img_total = 0;
        for (size_t m = 0; m < G; m++) {
            Member& x = mem[m];
            x.idx = groups[g].first + m;
            x.n = items[x.idx].claims->size();
            x.nw = nw_of(*items[x.idx].claims);
            x.job0 = jobs_total; x.claim0 = claims_total; x.u = u_total; x.img = img_total;
            x.u_words = 2 * C * (x.n + 1);
            x.len = opening_bytes(sh, x.n, Q);
            jobs_total += x.n + 1; claims_total += x.n; u_total += x.u_words; img_total += x.len / 8;
        }
        const size_t mem_at = 0, jobs_at = align16(G * sizeof(ObMember)), claims_at = jobs_at + align16(jobs_total * sizeof(ObJob));
        size_t at = claims_at + align16(claims_total * sizeof(ObClaim));
        for (Member& x : mem) {
            x.y_at = at;
            x.z_at = x.y_at + x.n * sizeof(E2);
            x.w_at = x.z_at + x.n * (size_t)sh.c * sizeof(E2);
            at = x.w_at + x.nw * sizeof(E2);
        }
        const size_t stage_bytes = std::max<size_t>(at, 16);
        char* h_stage = batch_desc_host(B, stage_bytes);   // (the previous group's copy of it was waited for)
        // results of the group, page-locked: the u vectors, the images, one cell a member
        const size_t hu_at = 0, himg_at = u_total * 8, hcell_at = himg_at + img_total * 8;
        char* h_out = batch_out_host(B, hcell_at + G * 8);
        const u64* h_u = reinterpret_cast<const u64*>(h_out + hu_at);
        uint8_t* h_img = reinterpret_cast<uint8_t*>(h_out + himg_at);
        const u64* h_cells = reinterpret_cast<const u64*>(h_out + hcell_at);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                const Commitment& cm = *items[x.idx].cm;
                const std::vector<Claim>& claims = *items[x.idx].claims;
                x.tr = start_transcript(sh, cm.root(), claims, Q);
                const std::vector<E2> rho = rho_powers(x.tr.squeeze(), R);
                ObMember* hm = reinterpret_cast<ObMember*>(h_stage + mem_at) + mq;
                hm->M = cm.d_M; hm->img = x.img; hm->u = x.u; hm->u_words = x.u_words;
                ObJob* hd = reinterpret_cast<ObJob*>(h_stage + jobs_at) + x.job0;
                ObClaim* hc = reinterpret_cast<ObClaim*>(h_stage + claims_at) + x.claim0;
                E2* hy = reinterpret_cast<E2*>(h_stage + x.y_at);
                E2* hz = reinterpret_cast<E2*>(h_stage + x.z_at);
                E2* hw = reinterpret_cast<E2*>(h_stage + x.w_at);
                hd[0].src = cm.d_rows; hd[0].nrows = R; hd[0].w_at = x.w_at; hd[0].u_at = x.u / 2;
                memcpy(hw, rho.data(), R * sizeof(E2));
                size_t off = R;
                for (size_t i = 0; i < x.n; i++) {
                    const Claim& cl = claims[i];
                    const std::vector<E2> w = eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
                    hd[i + 1].src = cm.d_rows + (sh.off[cl.table] << sh.c); hd[i + 1].nrows = w.size(); hd[i + 1].w_at = x.w_at + off * sizeof(E2);
                    hd[i + 1].u_at = x.u / 2 + (i + 1) * C;
                    memcpy(hw + off, w.data(), w.size() * sizeof(E2));
                    off += w.size();
                    hy[i] = cl.value;
                    memcpy(hz + i * (size_t)sh.c, cl.point.data(), (size_t)sh.c * sizeof(E2));
                    hc[i].u_at = hd[i + 1].u_at; hc[i].z_at = x.z_at + i * (size_t)sh.c * sizeof(E2); hc[i].y_at = x.y_at + i * sizeof(E2);
                    hc[i].member = (u64)mq; hc[i].claim = (u64)i;
                }
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        char* d_stage;
        u64 *d_u, *d_img, *d_js, *d_cells;
        try {
            d_stage = ctx->alloc_n<char>(stage_bytes);
            d_u = ctx->alloc_n<u64>(u_total);
            d_img = ctx->alloc_n<u64>(img_total);
            d_js = ctx->alloc_n<u64>(G * Q + G);
            d_cells = ctx->alloc_n<u64>(G);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold a group of " + std::to_string(G) + " openings: lower verify_batch_group (" + e.what() + ")");
        }
        const ObMember* d_mem = reinterpret_cast<const ObMember*>(d_stage + mem_at);
        const unsigned cb = blocks_for(C);
        if (jobs_total * cb > 0x7fffffffull) throw Error(who + ": a group of " + std::to_string(G) + " openings has too many row combinations for one launch: lower verify_batch_group");
        hip_check(hipMemcpyAsync(d_stage, h_stage, stage_bytes, hipMemcpyHostToDevice, st), "upload claims");
        hip_check(hipMemsetAsync(d_cells, 0xff, G * 8, st), "memset");
        size_t nw_total = 0;
        for (const Member& x : mem) nw_total += x.nw;
        ctx->prof_begin(cls, (double)nw_total * C * 8 + (double)u_total * 8);
        k_pcsob_combine<<<(unsigned)(jobs_total * cb), PCS_TPB, 0, st>>>(sh.c, cb, reinterpret_cast<const ObJob*>(d_stage + jobs_at), d_stage, reinterpret_cast<E2*>(d_u));
        ctx->prof_end();
        if (claims_total) {
            ctx->prof_begin(cls, (double)claims_total * C * 16);
            k_pcsob_eval<<<(unsigned)claims_total, PCS_TPB, 0, st>>>(reinterpret_cast<const ObClaim*>(d_stage + claims_at), sh.c, reinterpret_cast<const E2*>(d_u), d_stage, d_cells);
            ctx->prof_end();
        }
        ctx->prof_begin(cls, (double)u_total * 16);
        k_pcsob_emit<<<(unsigned)std::min<size_t>(blocks_for(u_total), 4096), PCS_TPB, 0, st>>>(d_mem, (unsigned)G, u_total, d_u, d_img);
        ctx->prof_end();
        hip_check(hipMemcpyAsync(h_out + hu_at, d_u, u_total * 8, hipMemcpyDeviceToHost, st), "download combinations");
        hip_check(hipMemcpyAsync(h_out + hcell_at, d_cells, G * 8, hipMemcpyDeviceToHost, st), "download evaluation checks");
        hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
        hip_check(hipGetLastError(), (who + ": launch").c_str());
        const double t2 = omp_get_wtime();
        // the host's share: every member's u_i into its transcript, its column indices out of it, one member a thread
        hj.assign(G * Q + G, 0);
        size_t active = 0;
        for (size_t m = 0; m < G; m++) {
            mem[m].refused = h_cells[m] != PCSV_NONE;
            hj[G * Q + m] = mem[m].refused ? 0 : 1;
            active += mem[m].refused ? 0 : 1;
        }
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            if (x.refused) continue;
            try {
                absorb_words(x.tr, h_u + x.u, x.u_words);
                const std::vector<size_t> js = squeeze_indices(x.tr, N, Q);
                for (size_t q = 0; q < Q; q++) hj[(size_t)mq * Q + q] = js[q];
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        const double t3 = omp_get_wtime();
        if (active) {
            if (Q) {
                hip_check(hipMemcpyAsync(d_js, hj.data(), hj.size() * 8, hipMemcpyHostToDevice, st), "upload column indices");
                ctx->prof_begin(cls, (double)active * Q * R * 16);
                k_pcsob_gather<<<blocks_for(G * Q * R), PCS_TPB, 0, st>>>(d_mem, G, Q, R, N, q_words, d_js, d_img);
                ctx->prof_end();
            }
            hip_check(hipMemcpyAsync(h_img, d_img, img_total * 8, hipMemcpyDeviceToHost, st), "download openings");
            hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
            hip_check(hipGetLastError(), (who + ": launch").c_str());
        }
        ctx->prof_collect();
        const double t4 = omp_get_wtime();
        // the siblings from each handle's tree into the gaps; a refused member's reason
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                Opened& out = res[x.idx];
                const Commitment& cm = *items[x.idx].cm;
                if (x.refused) {
                    const size_t i = (size_t)h_cells[mq];
                    out.refused = true;
                    out.reason = std::string(single) + ": claim " + std::to_string(i) + ": the value is not the evaluation of table " + std::to_string((*items[x.idx].claims)[i].table) +
                                 " at the point";
                    continue;
                }
                const uint8_t* image = h_img + 8 * x.img;
                out.bytes.assign(image, image + x.len);
                for (size_t q = 0; q < Q; q++) {
                    uint8_t* sib = out.bytes.data() + 8 * (x.u_words + q * q_words + R);
                    size_t idx = (size_t)hj[(size_t)mq * Q + q];
                    for (int l = 0; l < depth; l++, idx >>= 1) memcpy(sib + 32 * l, cm.node(l, idx ^ 1), 32);
                }
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        if (times)
            fprintf(stderr, "[hg pcs] open group %zu of %zu members: transcripts and weights %.2f ms, combine, checks and u back %.2f, hash %.2f, gather and images back %.2f, "
                            "siblings %.2f\n", g, G, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (omp_get_wtime() - t4) * 1e3);
    }
    return res;
}

}  // namespace pcs
}  // namespace hg
