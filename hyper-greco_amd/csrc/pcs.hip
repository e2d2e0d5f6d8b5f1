// Device form of the polynomial commitment (pcs.hpp): rows staged into the zero-padded 4C-stride matrix and encoded by the batched
// NTT, one Keccak-f[1600] state per thread for the column hashes and the tree, the E x F row combinations of an opening through
// the deferred-reduction accumulators, a gather of the opened columns. The handle owns the raw and the encoded matrix in HBM.
// The verifier of an opening reuses the encoding and the leaf hash and adds five kernels of its own.
// Every step has one kernel, written for a group of members and driven by a member or job table (the descriptors of pcs_flow.hpp,
// which both fields share); the forms for a run launch it once over a group, whose matrices lie in one allocation that its handles
// share, and the forms for one launch it over a group of one.
// The host flows of the verifiers, the batch opener, the batch committer, combine_device and columns_device are the templates of
// pcs_flow.hpp, written once for both fields; this file gives them GlPcs, the Goldilocks policy: the types, the transcript calls, the
// texts and one launch function per kernel step. commit_device and commit_device_values keep a host flow of their own.
// A commitment to tables that lie in HBM (commit_tables_enqueue: hg_secrets_commit_values, the encryption pipeline) stages them with one
// kernel of its own and goes on with the encoding, the leaf hash and the tree of commit_device.
// The statement digest of a bound proof (hg.h: "Bound proofs") lives here as well: its leaves are hashed by a kernel of the same
// thread-a-sponge form as the column hashes, its levels are the commitment's.
// The prover's side of a folded opening (pcs.hpp FoldSource) is here too: the kernel that builds g, the round kernels of the reduction
// sum-check - written for a group of members, the single call a group of one - with the host driver of one opening, FoldDev, and the
// helpers that open_folded_batch_flow of pcs_flow.hpp (a run, both fields) takes through GlPcs; the device verifiers of folded openings
// are verify_folded_flow and verify_batch_flow of pcs_flow.hpp.
#include <omp.h>
#include "pcs.hpp"
#include "prover.hpp"
#include "gl_wide.hpp"
#include "pcs_keccak.hpp"
#include "verifier_batch.hpp"
#include "pcs_flow.hpp"

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

// ---- the statement digest (pcs.hpp DigestMember; hg.h states the tree): the leaf kernel for a group of G members of one parameter
// set. Word w < 2kn of a member is coefficient w & (n-1) of modulus (w mod kn) >> log2 n of a (w < kn) or of ct0.
struct DigestShape {
    int log2_n, log2_k, log2_leaf, log2_leaves;   // a leaf: 2^log2_leaf = min(128, 2kn) words; 2^log2_leaves leaves a member
    u64 half[HG_MAX_K];                            // (q_i - 1) / 2
};
constexpr int DIGEST_TPB = 64;   // a member has 2kn / 128 leaves (8192 at n=32768 k=16): small workgroups reach more compute units
// Word w of member M as the signed value the digest hashes (two's complement). Compact: the staged word itself. Laid out: coefficient
// j of a_i is word n-1-j of input 3+i, of ct0_i word 2n-2-j of block i of ct0is; a field word v stands for v if v <= (p-1)/2, else
// for -(p-v) = v + 2^32 - 1 mod 2^64. bad: v is not below p or |value| is above (q_i-1)/2
template <bool LAID>
__device__ __forceinline__ u64 digest_word(const DigestMember* __restrict__ M, const DigestShape& S, size_t w, bool& bad) {
    const size_t kn = (size_t)1 << (S.log2_n + S.log2_k), n = (size_t)1 << S.log2_n;
    const bool c = w >= kn;
    const size_t r = c ? w - kn : w;
    if constexpr (!LAID) return (c ? M->ct0 : M->a[0])[r];
    const size_t i = r >> S.log2_n, j = r & (n - 1);
    const u64 v = c ? M->ct0[(i << (S.log2_n + 1)) + (2 * n - 2 - j)] : M->a[i][n - 1 - j];
    const bool neg = v > (GL_P - 1) / 2;
    const u64 mag = neg ? GL_P - v : v;
    bad |= v >= GL_P || mag > S.half[i];
    return neg ? v + 0xFFFFFFFFull : v;
}
// The 17 message words of sponge block b of leaf j into nx: message word 0 is LE64(2), word 1 + t is word j 2^log2_leaf + t of the
// member, word 2^log2_leaf + 1 the first padding byte; every index of nx is a compile-time constant
template <bool LAID>
__device__ __forceinline__ void digest_block(const DigestMember* __restrict__ M, const DigestShape& S, size_t j, size_t b, u64 (&nx)[RATE_WORDS], bool& bad) {
    const size_t words = ((size_t)1 << S.log2_leaf) + 1, first = j << S.log2_leaf;
#pragma unroll
    for (int i = 0; i < RATE_WORDS; i++) {
        const size_t idx = b * RATE_WORDS + i;
        u64 w = 0;
        if (idx == 0) w = 2;
        else if (idx < words) w = digest_word<LAID>(M, S, first + idx - 1, bad);
        else if (idx == words) w = 0x01;
        nx[i] = w;
    }
}
// One thread per (member m, leaf j), id = m 2^log2_leaves + j: Keccak256(LE64(2) || the leaf's words) into leaf j of the member's tree
// at trees + m tree_words. The state stays in registers; the words of the next sponge block are loaded ahead of the permutation of
// this one, so that their latency passes under it. A lane reads its leaf's 1 KiB with 8-byte loads at a lane stride of 1 KiB: eight
// whole 128-byte lines that no other lane touches, each fetched from HBM once and found in the cache by the loads that follow. LAID:
// a member whose word is not a signed value in range sets its flag.
template <bool LAID>
__device__ __forceinline__ void digest_leaf(const DigestMember* __restrict__ M, const DigestShape& S, size_t j, u64 (&a)[25], bool& bad) {
    const size_t blocks = (((size_t)1 << S.log2_leaf) + 1) / RATE_WORDS + 1;   // the last block holds the rest (possibly nothing) and the padding
    u64 nx[RATE_WORDS];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    digest_block<LAID>(M, S, j, 0, nx, bad);
    for (size_t b = 0; b < blocks; b++) {
#pragma unroll
        for (int i = 0; i < RATE_WORDS; i++) a[i] ^= nx[i];
        if (b + 1 < blocks) digest_block<LAID>(M, S, j, b + 1, nx, bad);
        else a[RATE_WORDS - 1] ^= 0x8000000000000000ull;
        keccak_f(a);
    }
}
template <bool LAID>
__global__ __launch_bounds__(DIGEST_TPB) void k_instance_digest_leaves(const DigestMember* __restrict__ mem, const DigestShape S, size_t G, u64* __restrict__ trees,
                                                                      size_t tree_words, unsigned* __restrict__ flags) {
    const size_t id = (size_t)blockIdx.x * DIGEST_TPB + threadIdx.x;
    if (id >= G << S.log2_leaves) return;
    const size_t m = id >> S.log2_leaves, j = id & (((size_t)1 << S.log2_leaves) - 1);
    bool bad = false;
    u64 a[25];
    digest_leaf<LAID>(mem + m, S, j, a, bad);
    u64* out = trees + m * tree_words + 4 * j;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
    if (LAID && bad) atomicOr(flags + m, 1u);
}

// The digest of a bound batch (verifier_batch.hip: a slice of a staged set; hg_instance_digest_group). The members are read where the
// batch staged them: member m's 2kn signed words - a, then ct0 - at set + m stride, the compact read without a descriptor table. One
// workgroup of DIGEST_TPB = 64 threads per (member, block of 64 leaves): thread t hashes leaf 64 b + t as k_instance_digest_leaves
// does (digest_leaf: the state in registers, the next sponge block loaded under the permutation of this one), puts its four words into
// LDS, and the workgroup folds its min(64, leaves) leaves to one node there - the levels one behind the other as in a tree buffer,
// 4 (64 + 32 + .. + 1) words = 4064 bytes, one merkle_node a thread and one barrier a level, six levels at most. Node b of member m goes
// to nodes + m tree_words + 4 b: the root where a member has at most 64 leaves (one leaf: that leaf), else leaf b of the small tree that
// merkle_levels_device_batch finishes. leaves = 2^log2_leaves is a power of two, so a workgroup's leaf count is one as well.
constexpr int DIGEST_FOLD_WORDS = 4 * (2 * DIGEST_TPB - 1);
__global__ __launch_bounds__(DIGEST_TPB) void k_instance_digest_group(const u64* __restrict__ set, size_t stride, const DigestShape S, u64* __restrict__ nodes,
                                                                     size_t tree_words) {
    __shared__ u64 fold[DIGEST_FOLD_WORDS];
    const size_t leaves = (size_t)1 << S.log2_leaves, per = leaves > DIGEST_TPB ? leaves / DIGEST_TPB : 1;   // workgroups a member
    const size_t m = blockIdx.x / per, b = blockIdx.x - m * per, j = b * DIGEST_TPB + threadIdx.x;
    const size_t mine = leaves < DIGEST_TPB ? leaves : DIGEST_TPB;                                           // leaves of this workgroup
    if (threadIdx.x < mine) {   // (j < leaves: every word read lies inside the member)
        DigestMember M;
        M.a[0] = set + m * stride;
        M.ct0 = M.a[0] + ((size_t)1 << (S.log2_n + S.log2_k));
        bool bad = false;
        u64 a[25];
        digest_leaf<false>(&M, S, j, a, bad);
        u64* leaf = fold + 4 * threadIdx.x;
        leaf[0] = a[0]; leaf[1] = a[1]; leaf[2] = a[2]; leaf[3] = a[3];
    }
    __syncthreads();
    u64* below = fold;
    for (size_t count = mine / 2; count >= 1; count >>= 1) {
        u64* here = below + 8 * count;   // `below` has 2 * count nodes of 4 words
        if (threadIdx.x < count) merkle_node(below, here, threadIdx.x);
        __syncthreads();
        below = here;
    }
    if (threadIdx.x < 4) nodes[m * tree_words + 4 * b + threadIdx.x] = below[threadIdx.x];
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
// from the shape, from the host's masked j_q or from table offsets the entry point validated. The descriptors (VbMember, VbGroup,
// CombineDesc) and the result cells are those of pcs_flow.hpp; a row element is a word, so the offsets in Row units are word offsets.

// Big-endian words of an opening -> native words; blockIdx.y = the member, its words grid-strided over blockIdx.x. Word i < u_words is
// coordinate i & 1 of element i >> 1 of the u vectors: kept in u (as E2) and scattered into row 2 * (i >> (c+1)) + (i & 1) of the
// member's rows of the matrix the NTT encodes (zeroed beforehand). The others are the Q * R column words, query q at word
// u_words + q * q_stride. cells[3m] = the lowest byte offset, within its opening, of a word that is not below p.
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
        if (i >= u_words) { const size_t k = i - u_words, q = k / R; at = u_words + q * g.q_stride + (k - q * R); }
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
    const u64* sib = set + M.proof + u_words + q * g.q_stride + g.R;
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
// member where its matrix, its u vectors and its opening image lie (ObJob, ObClaim, ObMember of pcs_flow.hpp). Every grid is
// one-dimensional.

// Row combinations: u[u_at + j] = sum_{r < nrows} w[r] * src[r][j] for the job of the block, a thread owns column j. Block b serves job
// b / cb, columns (b % cb) PCS_TPB .. ; the weights are uniform over the workgroup.
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_combine(int c, unsigned cb, const ObJob<u64>* __restrict__ jobs, const char* __restrict__ stage, E2* __restrict__ u) {
    const size_t C = (size_t)1 << c;
    const unsigned jq = blockIdx.x / cb;
    const size_t j = (size_t)(blockIdx.x - jq * cb) * PCS_TPB + threadIdx.x;
    if (j >= C) return;
    const ObJob<u64> job = jobs[jq];
    u[job.u_at + j] = dot_chunked(job.src + j, c, reinterpret_cast<const E2*>(stage + job.w_at), job.nrows);
}
// One workgroup per (member, claim): <u_i, eq(z_i[..c])> == y_i; cells[member] = its lowest failing claim
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_eval(const ObClaim* __restrict__ claims, int c, const E2* __restrict__ u, const char* __restrict__ stage,
                                                        u64* __restrict__ cells) {
    const ObClaim cl = claims[blockIdx.x];
    if (eval_differs(u + cl.u_at, reinterpret_cast<const E2*>(stage + cl.z_at), reinterpret_cast<const E2*>(stage + cl.y_at), c)) cell_min(cells + cl.member, cl.claim);
}
// Word i of the group's u vectors, big-endian, into its member's image: the member is the last one whose u offset is <= i
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_emit(const ObMember<u64>* __restrict__ mem, unsigned G, size_t total, const u64* __restrict__ u, u64* __restrict__ img) {
    for (size_t i = (size_t)blockIdx.x * PCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * PCS_TPB) {
        unsigned lo = 0, hi = G;
        while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].u <= i) lo = mid; else hi = mid; }
        img[mem[lo].img + (i - mem[lo].u)] = __builtin_bswap64(u[i]);
    }
}
// One thread per (member m, query q, row r), id = (m Q + q) R + r: M_m[r][j_q] big-endian at its place in the member's image.
// js[m Q + q] = j_q (masked by the host); js[G Q + m] != 0: the member takes part (it was not refused)
__global__ __launch_bounds__(PCS_TPB) void k_pcsob_gather(const ObMember<u64>* __restrict__ mem, size_t G, size_t Q, size_t R, size_t N, size_t q_words,
                                                          const u64* __restrict__ js, u64* __restrict__ img) {
    const size_t id = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (id >= G * Q * R) return;
    const size_t m = id / (Q * R), k = id - m * Q * R, q = k / R, r = k - q * R;
    if (!js[G * Q + m]) return;
    const ObMember<u64> M = mem[m];
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

// ---- the statement digest: host side
static DigestShape digest_shape(const Params& p) {
    DigestShape S;
    S.log2_n = p.n_log2;
    S.log2_k = p.log2k;
    S.log2_leaf = std::min(7, p.n_log2 + p.log2k + 1);
    static_assert(DIGEST_LEAF_WORDS == 128, "2^7 words a full leaf");
    S.log2_leaves = p.n_log2 + p.log2k + 1 - S.log2_leaf;
    for (int i = 0; i < HG_MAX_K; i++) S.half[i] = i < p.k ? (p.raw.qis[i] - 1) / 2 : 0;
    return S;
}

// the subtree nodes of a member and the levels above them: 8 words a node of the lowest level, as in every tree buffer
static size_t digest_group_per(const DigestShape& S) { return std::max<size_t>(1, ((size_t)1 << S.log2_leaves) / DIGEST_TPB); }
size_t instance_digest_group_words(const Params& p) { return 8 * digest_group_per(digest_shape(p)); }

void instance_digest_group_enqueue(hg_ctx* ctx, hipStream_t st, const Params& p, const u64* d_set, size_t G, u64* d_nodes, uint8_t* h_roots) {
    if (!G) return;
    const DigestShape S = digest_shape(p);
    const size_t per = digest_group_per(S), tree_words = 8 * per, stride = (size_t)2 << (p.n_log2 + p.log2k);
    hipStream_t prof_was = ctx->prof_stream;
    ctx->prof_stream = st;
    ctx->prof_begin(ctx->prof_class("instance_digest_group", false), (double)G * (8.0 * stride + 32 * per + (per > 1 ? 96.0 * per : 0)));
    k_instance_digest_group<<<(unsigned)(G * per), DIGEST_TPB, 0, st>>>(d_set, stride, S, d_nodes, tree_words);
    if (per > 1) merkle_levels_device_batch(st, d_nodes, tree_words, per, G);
    ctx->prof_end();
    ctx->prof_stream = prof_was;
    // the root is the last node of a member's small tree: word 4 (2 per - 2)
    hip_check(hipMemcpy2DAsync(h_roots, 32, d_nodes + 4 * (2 * per - 2), tree_words * 8, 32, G, hipMemcpyDeviceToHost, st), "instance digest: download the roots");
}

void instance_digest_enqueue(hg_ctx* ctx, hipStream_t st, const Params& p, bool laid, const DigestMember* mem, size_t G, uint8_t* roots, unsigned* flags) {
    if (!G) return;
    const DigestShape S = digest_shape(p);
    const size_t leaves = (size_t)1 << S.log2_leaves, tree_words = 8 * leaves, bytes = G * sizeof(DigestMember), need = (bytes + 15) & ~(size_t)15;
    if (ctx->stage_used + need > ctx->stage_cap) throw Error("the staging buffer cannot hold the members of the digest");
    DigestMember* h_mem = reinterpret_cast<DigestMember*>(ctx->h_stage + ctx->stage_used);
    ctx->stage_used += need;
    memcpy(h_mem, mem, bytes);
    DigestMember* d_mem = ctx->alloc_n<DigestMember>(G);
    u64* d_trees = ctx->alloc_n<u64>(G * tree_words);
    unsigned* d_flags = ctx->alloc_n<unsigned>(G + 4);
    hip_check(hipMemcpyAsync(d_mem, h_mem, bytes, hipMemcpyHostToDevice, st), "instance digest: upload the members");
    if (laid) hip_check(hipMemsetAsync(d_flags, 0, G * sizeof(unsigned), st), "memset");
    hipStream_t prof_was = ctx->prof_stream;
    ctx->prof_stream = st;
    const unsigned grid = (unsigned)(((G << S.log2_leaves) + DIGEST_TPB - 1) / DIGEST_TPB);
    ctx->prof_begin(ctx->prof_class("instance_digest_leaves", false), (double)G * (((size_t)16 << (p.n_log2 + p.log2k)) + 32 * leaves));
    if (laid) k_instance_digest_leaves<true><<<grid, DIGEST_TPB, 0, st>>>(d_mem, S, G, d_trees, tree_words, d_flags);
    else k_instance_digest_leaves<false><<<grid, DIGEST_TPB, 0, st>>>(d_mem, S, G, d_trees, tree_words, d_flags);
    ctx->prof_end();
    if (leaves > 1) {
        ctx->prof_begin(ctx->prof_class("instance_digest_tree", false), (double)G * leaves * 96);
        merkle_levels_device_batch(st, d_trees, tree_words, leaves, G);
        ctx->prof_end();
    }
    ctx->prof_stream = prof_was;
    // the root is the last node of a tree: word 4 (2 leaves - 2)
    hip_check(hipMemcpy2DAsync(roots, 32, d_trees + 4 * (2 * leaves - 2), tree_words * 8, 32, G, hipMemcpyDeviceToHost, st), "instance digest: download the roots");
    if (laid && flags) hip_check(hipMemcpyAsync(flags, d_flags, G * sizeof(unsigned), hipMemcpyDeviceToHost, st), "instance digest: download the flags");
}

void instance_digest_device(hg_ctx* ctx, const Params& p, const std::vector<const Instance*>& insts, uint8_t* out) {
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    Drain drain{st};   // (the instances are the caller's: every way out waits for their uploads)
    const size_t G = insts.size(), kn = (size_t)p.k * p.PZ();
    std::vector<DigestMember> mem(G);
    u64* d_words = ctx->alloc_n<u64>(G * 2 * kn);
    for (size_t m = 0; m < G; m++) {
        if (insts[m]->a.size() != kn || insts[m]->ct0.size() != kn) throw Error("an instance does not hold k * n coefficients a table");
        memset(&mem[m], 0, sizeof(DigestMember));
        u64* at = d_words + m * 2 * kn;
        hip_check(hipMemcpyAsync(at, insts[m]->a.data(), kn * 8, hipMemcpyHostToDevice, st), "instance digest: upload the instance");
        hip_check(hipMemcpyAsync(at + kn, insts[m]->ct0.data(), kn * 8, hipMemcpyHostToDevice, st), "instance digest: upload the instance");
        mem[m].a[0] = at;
        mem[m].ct0 = at + kn;
    }
    std::vector<uint8_t> roots(32 * G);
    instance_digest_enqueue(ctx, st, p, false, mem.data(), G, roots.data(), nullptr);
    hip_check(hipStreamSynchronize(st), "instance digest: sync");
    hip_check(hipGetLastError(), "instance digest: launch");
    ctx->prof_collect();
    memcpy(out, roots.data(), roots.size());
}

void instance_digest_values(hg_ctx* ctx, const Params& p, const DigestMember& mem, uint8_t out[32]) {
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    Drain drain{st};
    uint8_t root[32];
    unsigned flag = 0;
    instance_digest_enqueue(ctx, st, p, true, &mem, 1, root, &flag);
    hip_check(hipStreamSynchronize(st), "instance digest: sync");
    hip_check(hipGetLastError(), "instance digest: launch");
    ctx->prof_collect();
    if (flag) throw Error("a word of ais or ct0is is not a signed value in [-(q_i-1)/2, (q_i-1)/2]");
    memcpy(out, root, 32);
}

Commitment* commit_device_values(hg_ctx* ctx, const Shape& sh, const u64* const* d_tables, DigestJob* dg) {
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
    Drain drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
    Drain drain2{dg ? ctx->stream2 : st};   // (the digest's stream as well, where one is used)
    if (dg) {   // the second stream starts behind whatever the first one holds by now, not behind the commit
        hip_check(hipEventRecord(ctx->ev_fork, st), "fork");
        hip_check(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0), "fork wait");
    }
    ctx->prof_stream = st;
    commit_tables_enqueue(st, sh, d_tables, cm->d_rows, cm->d_M, scratch, W, d_tree, d_flag, ctx, ctx->prof_class("pcs_commit_values", false));
    if (dg) {   // the statement digest of the same values object, beside the commit's kernels: both are enqueued ahead of the first copy back
        dg->flag = 0;
        instance_digest_enqueue(ctx, ctx->stream2, *dg->p, true, &dg->mem, 1, dg->digest, &dg->flag);
    }
    cm->tree.resize(32 * (2 * N - 1));
    hip_check(hipMemcpyAsync(cm->tree.data(), d_tree, cm->tree.size(), hipMemcpyDeviceToHost, st), "download tree");
    hip_check(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st), "download flag");
    hip_check(hipStreamSynchronize(st), "sync");
    if (dg) hip_check(hipStreamSynchronize(ctx->stream2), "sync (statement digest)");
    hip_check(hipGetLastError(), "launch");
    ctx->prof_collect();
    if (flag) throw Error("a table holds a word that is not below p");
    return cm.release();
}

// ---- the reduction sum-check of a folded opening (pcs.hpp FoldSource; hg.h "Folded openings"): the prover's table-sized work.
// The raw rows of a handle are its tables, contiguous in table order: table t starts at word s_t = off_t C. g lies in an E array parallel
// to them. Round 0 reads the rows as they are; the kernel of round j >= 1 folds every live table and its g by r_{j-1} into buffers of
// half the size and forms round j's sums from the folded entries while it holds them, so a table is read once and written once a round.
// After j folds table t lies at entry s_t >> j of its buffer: two live tables never overlap there, since s_t' >= s_t + 2^{v_t} and
// 2^{v_t - j} is whole. The two buffer pairs alternate; the rows are never written. A table of two entries is folded to its two scalars
// T_t(rho[..v_t)) and g_t(rho[..v_t)) - the first is Y_t - which go to the host with the round's sums; from then on the table is host
// arithmetic. Hand-off: the sums of a round (48 bytes) and the scalars of the tables that retired come back with ONE SYNCHRONISATION A
// ROUND (the challenge of round j is hashed from round j's sums, so V round trips are inherent; the rounds on small tables are
// single-workgroup launches). Every round runs on the device: there is no host finish.
// Geometry: blockIdx.y = a live table, its units grid-strided over blockIdx.x; at most fold_max_blocks() workgroups in all. A thread
// keeps the three sums unreduced (gl_wide.hpp), restarted every WFLUSH_TRIPS units, reduces them once, then the wave adds by lane
// exchange and the workgroup through 192 bytes of LDS; one small workgroup adds the workgroups' partials. Field addition is exact: the
// order changes no byte.
constexpr int FOLD_TPB = 256;
constexpr unsigned FOLD_MAX_BLOCKS = 2048;
// HG_PCS_FOLD_BLOCKS (tests set it): another bound on the workgroups of a launch, so that a thread's units cross WFLUSH_TRIPS at a small size
static unsigned fold_max_blocks() {
    const char* e = getenv("HG_PCS_FOLD_BLOCKS");
    const long v = e && *e ? atol(e) : (long)FOLD_MAX_BLOCKS;
    return (unsigned)std::max(1L, std::min(65535L, v));
}
struct FoldClaim { u64 lo_at, hi_at; u32 lo_bits, pad; };   // its two factor tables (elements of its member's staged factors): eq(z, x) = lo[x & (2^lo_bits - 1)] hi[x >> lo_bits]
// What a shape fixes for the g kernel of every member: the tables of two entries or more (the kernel's table numbers) and the one-word
// tables, whose word goes to the scalars as it is
struct FoldGTables {
    u32 nt, n1;
    u32 lg[MAX_TABLES], id1[MAX_TABLES];          // v_t; the number t of a one-word table
    u64 at[MAX_TABLES], at1[MAX_TABLES];          // s_t; where a one-word table lies in the rows
};
// A member's block of the g kernel's staged copy (byte offsets): claim0[nt + 1] (the claims of kernel table t are claim0[t] .. claim0[t+1]
// of its list: members differ in their claim counts, and a table may have none), its FoldClaim list, its factor tables
struct FoldGMember { u64 claim0_at, claims_at, fac_at, pad; };
struct FoldTables {
    u32 nt, vec;                                  // vec: every `in` of the rows is even, a pair of words is one 16-byte load
    u32 lg[MAX_TABLES], id[MAX_TABLES];           // log2 of a live table's entries at the input; its number t
    u64 in[MAX_TABLES], out[MAX_TABLES];          // where it lies in the input and where it goes in the output (entries)
};
// What differs by member (blockIdx.z) of a launch: where its raw rows lie (a handle may live in any slab), its challenge, and a fixed
// stride into the group's g, buffer pairs and scalars. A group of one - the single call - carries its row base and its challenge in
// the kernel arguments (rows == null, r == null): its launches need no table and no upload.
struct FoldMembers {
    const u64* const* rows;
    const u64* rows0;
    const E2* r;
    E2 r0;
    u64 g_stride, in_stride, out_stride, scal_stride;   // entries from a member to the next: g, the input pair, the output pair, the scalars
};
__device__ __forceinline__ const u64* fold_rows(const FoldMembers& M) { return M.rows ? M.rows[blockIdx.z] : M.rows0; }
__device__ __forceinline__ E2 ld_e2(const E2* p) { const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p); return e2(v.x, v.y); }
__device__ __forceinline__ void st_e2(E2* p, E2 v) { *reinterpret_cast<ulonglong2*>(p) = make_ulonglong2(v.c0, v.c1); }
__device__ __forceinline__ void ld_pair(const u64* p, bool vec, u64& a, u64& b) {
    if (vec) { const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p); a = v.x; b = v.y; }
    else { a = p[0]; b = p[1]; }
}
// g_t[x] = sum_{i on t} beta^i eq(z_i, x), every entry written once: a thread owns entry x and walks the table's claims, each a product of
// two staged factors (beta^i lies in the low one). stage: G FoldGMember, then the members' blocks. The first workgroup of a member
// also copies the words of its one-word tables to scal[2 t].
__global__ __launch_bounds__(FOLD_TPB) void k_pcsfold_g(const FoldGTables A, const FoldMembers M, const char* __restrict__ stage, E2* __restrict__ g, E2* __restrict__ scal) {
    const unsigned t = blockIdx.y;
    if (blockIdx.x == 0 && t == 0 && threadIdx.x < A.n1)
        st_e2(scal + (size_t)blockIdx.z * M.scal_stride + 2 * A.id1[threadIdx.x], e2(fold_rows(M)[A.at1[threadIdx.x]], 0));
    if (t >= A.nt) return;
    const size_t len = (size_t)1 << A.lg[t];
    const FoldGMember D = reinterpret_cast<const FoldGMember*>(stage)[blockIdx.z];
    const u32* claim0 = reinterpret_cast<const u32*>(stage + D.claim0_at);
    const FoldClaim* cl = reinterpret_cast<const FoldClaim*>(stage + D.claims_at);
    const E2* fac = reinterpret_cast<const E2*>(stage + D.fac_at);
    const unsigned first = claim0[t], last = claim0[t + 1];
    E2* G = g + (size_t)blockIdx.z * M.g_stride + A.at[t];
    for (size_t x = (size_t)blockIdx.x * FOLD_TPB + threadIdx.x; x < len; x += (size_t)gridDim.x * FOLD_TPB) {
        WE2 acc = we2_zero();
        E2 sum = e2_zero();
        int trips = 0;
        for (unsigned i = first; i < last; i++) {
            const FoldClaim d = cl[i];
            we2_mac(acc, ld_e2(fac + d.lo_at + (x & (((size_t)1 << d.lo_bits) - 1))), ld_e2(fac + d.hi_at + (x >> d.lo_bits)));
            if (++trips == WFLUSH_TRIPS) { sum = e2_add(sum, we2_reduce(acc)); acc = we2_zero(); trips = 0; }
        }
        st_e2(G + x, e2_add(sum, we2_reduce(acc)));
    }
}
// the three sums of a thread -> those of its workgroup at out[3 b .. 3 b + 3), b = its number in the grid (members outermost); every thread calls it
__device__ __forceinline__ void fold_block_sums(E2 (&s)[3], E2* __restrict__ out) {
    __shared__ E2 part[FOLD_TPB / 64][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
        for (int m = 32; m >= 1; m >>= 1)
            s[k] = e2_add(s[k], e2((u64)__shfl_xor((unsigned long long)s[k].c0, m, 64), (u64)__shfl_xor((unsigned long long)s[k].c1, m, 64)));
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) part[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        E2 v = part[0][threadIdx.x];
        for (int w = 1; w < FOLD_TPB / 64; w++) v = e2_add(v, part[w][threadIdx.x]);
        out[3 * (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) + threadIdx.x] = v;
    }
}
// Round 0: nothing to fold, the table entries are base-field words. A unit is a pair (T0, T1), (g0, g1):
// s(0) += g0 T0, s(1) += g1 T1, c2 += (g1 - g0) (T1 - T0), an E x F product each
__global__ __launch_bounds__(FOLD_TPB) void k_pcsfold_round0(const FoldTables A, const FoldMembers M, const E2* __restrict__ g, E2* __restrict__ partial) {
    const unsigned t = blockIdx.y;
    const size_t pairs = (size_t)1 << (A.lg[t] - 1);
    const u64* T = fold_rows(M) + A.in[t];
    const E2* G = g + (size_t)blockIdx.z * M.g_stride + A.in[t];
    W2 a = w2_zero(), b = w2_zero(), c = w2_zero();
    int trips = 0;
    for (size_t u = (size_t)blockIdx.x * FOLD_TPB + threadIdx.x; u < pairs; u += (size_t)gridDim.x * FOLD_TPB) {
        u64 t0, t1;
        ld_pair(T + 2 * u, A.vec, t0, t1);
        const E2 g0 = ld_e2(G + 2 * u), g1 = ld_e2(G + 2 * u + 1);
        w2_mac_f(a, g0, t0);
        w2_mac_f(b, g1, t1);
        w2_mac_f(c, e2_sub(g1, g0), gl_sub(t1, t0));
        if (++trips == WFLUSH_TRIPS) { a = w2_from(w2_reduce(a)); b = w2_from(w2_reduce(b)); c = w2_from(w2_reduce(c)); trips = 0; }
    }
    E2 s[3] = {w2_reduce(a), w2_reduce(b), w2_reduce(c)};
    fold_block_sums(s, partial);
}
// Round j >= 1. A unit is four adjacent entries of T and of g: folded by r = r_{j-1} into two of each, which are stored and enter the sums
// of round j as E x E products. BASE (round 1): the entries of T are the words of the raw rows and gin is g (in_stride = g_stride). A
// table of two entries is folded into its two scalars at scal[2 id], scal[2 id + 1] of its member by one thread and enters no sum.
template <bool BASE>
__global__ __launch_bounds__(FOLD_TPB) void k_pcsfold_round(const FoldTables A, const FoldMembers M, const E2* __restrict__ tin, const E2* __restrict__ gin,
                                                            E2* __restrict__ tout, E2* __restrict__ gout, E2* __restrict__ scal, E2* __restrict__ partial) {
    const unsigned t = blockIdx.y, lg = A.lg[t];
    const FoldR f = fold_r(M.r ? M.r[blockIdx.z] : M.r0);
    const size_t in_at = (size_t)blockIdx.z * M.in_stride + A.in[t];
    const u64* rows = BASE ? fold_rows(M) + A.in[t] : nullptr;
    const E2* G = gin + in_at;
    // T[2i] + r (T[2i+1] - T[2i])
    auto fold_t = [&](size_t i) {
        if constexpr (BASE) {
            u64 t0, t1;
            ld_pair(rows + 2 * i, A.vec, t0, t1);
            const u64 d = gl_sub(t1, t0);
            return e2(wreduce(wacc_mul_init(t0, f.r0, d)), gl_mul(f.r1, d));
        } else {
            const E2 t0 = ld_e2(tin + in_at + 2 * i);
            return e2_fold_wide(t0, e2_sub(ld_e2(tin + in_at + 2 * i + 1), t0), f);
        }
    };
    auto fold_g = [&](size_t i) {
        const E2 g0 = ld_e2(G + 2 * i);
        return e2_fold_wide(g0, e2_sub(ld_e2(G + 2 * i + 1), g0), f);
    };
    WE2 a = we2_zero(), b = we2_zero(), c = we2_zero();
    E2 s[3] = {e2_zero(), e2_zero(), e2_zero()};
    if (lg == 1) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            E2* sc = scal + (size_t)blockIdx.z * M.scal_stride + 2 * A.id[t];
            st_e2(sc, fold_t(0));
            st_e2(sc + 1, fold_g(0));
        }
    } else {
        const size_t units = (size_t)1 << (lg - 2), out_at = (size_t)blockIdx.z * M.out_stride + A.out[t];
        E2* To = tout + out_at;
        E2* Go = gout + out_at;
        int trips = 0;
        for (size_t u = (size_t)blockIdx.x * FOLD_TPB + threadIdx.x; u < units; u += (size_t)gridDim.x * FOLD_TPB) {
            const E2 t0 = fold_t(2 * u), t1 = fold_t(2 * u + 1), g0 = fold_g(2 * u), g1 = fold_g(2 * u + 1);
            st_e2(To + 2 * u, t0);
            st_e2(To + 2 * u + 1, t1);
            st_e2(Go + 2 * u, g0);
            st_e2(Go + 2 * u + 1, g1);
            we2_mac(a, g0, t0);
            we2_mac(b, g1, t1);
            we2_mac(c, e2_sub(g1, g0), e2_sub(t1, t0));
            if (++trips == WFLUSH_TRIPS) {
                s[0] = e2_add(s[0], we2_reduce(a)); s[1] = e2_add(s[1], we2_reduce(b)); s[2] = e2_add(s[2], we2_reduce(c));
                a = we2_zero(); b = we2_zero(); c = we2_zero();
                trips = 0;
            }
        }
    }
    s[0] = e2_add(s[0], we2_reduce(a)); s[1] = e2_add(s[1], we2_reduce(b)); s[2] = e2_add(s[2], we2_reduce(c));
    fold_block_sums(s, partial);
}
// one workgroup a member (blockIdx.x): out[3 member + k] = sum_b partial[3 (member blocks + b) + k]
__global__ __launch_bounds__(FOLD_TPB) void k_pcsfold_sum(const E2* __restrict__ partial, size_t blocks, E2* __restrict__ out) {
    const E2* mine = partial + 3 * blocks * blockIdx.x;
    E2 s[3] = {e2_zero(), e2_zero(), e2_zero()};
    for (size_t b = threadIdx.x; b < blocks; b += FOLD_TPB)
        for (int k = 0; k < 3; k++) s[k] = e2_add(s[k], ld_e2(mine + 3 * b + k));
    fold_block_sums(s, out);
}

// ---- what the single call (FoldDev) and the pass over a group (open_folded_device_batch) share on the host: the geometry a shape
// fixes, a member's block of the g kernel's staged copy, the launches of the g kernel and of a round
static FoldGTables fold_g_tables(const Shape& sh, size_t* max_len) {
    FoldGTables A;
    memset(&A, 0, sizeof(A));
    *max_len = 1;
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t v = (size_t)sh.nvars[t], at = sh.off[t] << sh.c;
        if (v == 0) { A.id1[A.n1] = (u32)t; A.at1[A.n1] = (u64)at; A.n1++; continue; }   // a scalar from the start: T_t() is the word, g_t() = sum beta^i
        A.lg[A.nt] = (u32)v;
        A.at[A.nt] = (u64)at;
        A.nt++;
        *max_len = std::max(*max_len, (size_t)1 << v);
    }
    return A;
}
// the bytes of a member's block, a multiple of 16
static size_t fold_gblock_bytes(const Shape& sh, const FoldGTables& A, const std::vector<Claim>& claims) {
    size_t nc = 0, fac = 0;
    for (const Claim& cl : claims) {
        const size_t v = (size_t)sh.nvars[cl.table], lo_bits = (v + 1) / 2;
        if (v == 0) continue;
        nc++;
        fac += ((size_t)1 << lo_bits) + ((size_t)1 << (v - lo_bits));
    }
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    return up((A.nt + 1) * sizeof(u32)) + up(nc * sizeof(FoldClaim)) + fac * sizeof(E2);
}
// writes the block at byte `at` (a multiple of 16) of the staged copy and its descriptor; G1[t] = g_t() of the one-word tables
static void fold_gblock_fill(char* stage, FoldGMember& d, size_t at, const Shape& sh, const FoldGTables& A, const std::vector<Claim>& claims, const std::vector<E2>& bpow,
                             std::vector<E2>& G1) {
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t nc = 0;
    for (const Claim& cl : claims) nc += sh.nvars[cl.table] != 0;
    d.claim0_at = at;
    d.claims_at = d.claim0_at + up((A.nt + 1) * sizeof(u32));
    d.fac_at = d.claims_at + up(nc * sizeof(FoldClaim));
    d.pad = 0;
    u32* claim0 = reinterpret_cast<u32*>(stage + d.claim0_at);
    FoldClaim* list = reinterpret_cast<FoldClaim*>(stage + d.claims_at);
    E2* fac = reinterpret_cast<E2*>(stage + d.fac_at);
    size_t k = 0, f = 0, kt = 0;   // claims and factors written; the kernel's table number
    claim0[0] = 0;
    G1.assign(sh.nvars.size(), e2_zero());
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t v = (size_t)sh.nvars[t], lo_bits = (v + 1) / 2;
        for (size_t i = 0; i < claims.size(); i++) {
            if (claims[i].table != t) continue;
            if (v == 0) { G1[t] = e2_add(G1[t], bpow[i]); continue; }
            std::vector<E2> lo = eq_table(claims[i].point.data(), lo_bits);
            const std::vector<E2> hi = eq_table(claims[i].point.data() + lo_bits, v - lo_bits);
            for (E2& x : lo) x = e2_mul(x, bpow[i]);
            list[k++] = FoldClaim{(u64)f, (u64)(f + lo.size()), (u32)lo_bits, 0};
            memcpy(fac + f, lo.data(), lo.size() * sizeof(E2));
            memcpy(fac + f + lo.size(), hi.data(), hi.size() * sizeof(E2));
            f += lo.size() + hi.size();
        }
        if (v != 0) claim0[++kt] = (u32)k;
    }
}
// the workgroups a table of a launch over nt tables of G members whose largest has `units` units: max_blocks bounds the launch as a whole
static unsigned fold_blocks_of(unsigned max_blocks, size_t units, size_t nt, size_t G) {
    const size_t cap = std::max<size_t>(1, max_blocks / (nt * G));
    return (unsigned)std::max<size_t>(1, std::min(cap, (units + FOLD_TPB - 1) / FOLD_TPB));
}
// the tables live in step j and where they lie; retire: one of them is folded to its scalars; units: those of the largest; entries: in all
static FoldTables fold_tables(const Shape& sh, size_t j, bool* retire, size_t* max_units, size_t* entries) {
    FoldTables A;
    memset(&A, 0, sizeof(A));
    A.vec = sh.c >= 1;
    *retire = false;
    *max_units = 1;
    *entries = 0;
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t v = (size_t)sh.nvars[t], at = sh.off[t] << sh.c;
        if (v == 0 || v < j) continue;   // a scalar already
        const size_t lg = j == 0 ? v : v - (j - 1);
        A.lg[A.nt] = (u32)lg;
        A.id[A.nt] = (u32)t;
        A.in[A.nt] = j == 0 ? at : at >> (j - 1);
        A.out[A.nt] = at >> j;
        A.nt++;
        *retire |= j > 0 && lg == 1;
        *max_units = std::max(*max_units, j == 0 ? (size_t)1 << (lg - 1) : lg == 1 ? 1 : (size_t)1 << (lg - 2));
        *entries += (size_t)1 << lg;
    }
    return A;
}
// the arena buffers of G reductions: g (16 bytes a table entry), the two buffer pairs (a half and a quarter of that for T and for g
// each, member after member), the partials, the sums and the scalars
struct FoldBufs {
    E2 *g, *t[2], *gg[2], *scal, *partial, *sums;
    size_t stride[2];   // entries a member of pair 0 and of pair 1
};
static FoldBufs fold_alloc(hg_ctx* ctx, const Shape& sh, size_t G, unsigned max_blocks) {
    const size_t W = sh.R << sh.c, m = sh.nvars.size();
    FoldBufs b;
    b.stride[0] = W / 2 + 1;
    b.stride[1] = W / 4 + 1;
    b.g = ctx->alloc_n<E2>(G * W);
    for (int p = 0; p < 2; p++) {
        b.t[p] = ctx->alloc_n<E2>(G * b.stride[p]);
        b.gg[p] = ctx->alloc_n<E2>(G * b.stride[p]);
    }
    b.scal = ctx->alloc_n<E2>(G * 2 * m);
    b.partial = ctx->alloc_n<E2>(3 * ((size_t)max_blocks + MAX_TABLES * G));
    b.sums = ctx->alloc_n<E2>(3 * G);
    return b;
}
// the launch of step j over G members (A.nt >= 1) and, `sums`, of the workgroup a member that adds its partials
static void fold_launch(hipStream_t st, unsigned max_blocks, const Shape& sh, size_t j, const FoldTables& A, size_t max_units, size_t G, FoldMembers M, const FoldBufs& b,
                        bool sums) {
    const size_t W = sh.R << sh.c;
    const dim3 grid(fold_blocks_of(max_blocks, max_units, A.nt, G), A.nt, (unsigned)G);
    M.g_stride = W;
    M.scal_stride = 2 * sh.nvars.size();
    M.in_stride = j <= 1 ? W : b.stride[j & 1];
    M.out_stride = j == 0 ? 0 : b.stride[(j - 1) & 1];
    if (j == 0) k_pcsfold_round0<<<grid, FOLD_TPB, 0, st>>>(A, M, b.g, b.partial);
    else if (j == 1) k_pcsfold_round<true><<<grid, FOLD_TPB, 0, st>>>(A, M, nullptr, b.g, b.t[0], b.gg[0], b.scal, b.partial);
    else k_pcsfold_round<false><<<grid, FOLD_TPB, 0, st>>>(A, M, b.t[j & 1], b.gg[j & 1], b.t[(j - 1) & 1], b.gg[(j - 1) & 1], b.scal, b.partial);
    if (sums) k_pcsfold_sum<<<(unsigned)G, FOLD_TPB, 0, st>>>(b.partial, (size_t)grid.x * grid.y, b.sums);
}
// the bytes step j moves over `entries` table entries: round 0 reads 8 + 16 an entry, round 1 reads them and writes 16 + 16 for every
// two, a later round reads 32 and writes 16
static double fold_step_bytes(size_t j, size_t entries) { return (double)entries * (j == 0 ? 24 : j == 1 ? 40 : 48); }

// The device form of FoldSource: a group of one through the kernels above. Scratch from the context's arena (reset here; the handle's
// matrices are its own).
struct FoldDev : FoldSource {
    const Commitment& cm;
    hg_ctx* ctx;
    hipStream_t st;
    int cls;
    size_t n_claims;
    unsigned max_blocks;
    FoldBufs buf;
    FoldMembers mem;
    bool one_word;          // the shape has one-word tables: their words come back with step 0
    std::vector<E2> h_scal, G1;
    E2 h_sums[3];

    FoldDev(const Commitment& cm_, const std::vector<Claim>& claims, const std::vector<E2>& bpow) : cm(cm_), ctx(cm_.ctx), n_claims(claims.size()) {
        const Shape& sh = cm.sh;
        const size_t m = sh.nvars.size(), W = sh.R << sh.c;
        hip_check(hipSetDevice(ctx->device), "hipSetDevice");
        ctx->arena_reset();
        st = ctx->stream;
        cls = ctx->prof_class("pcs_fold", false);
        ctx->prof_stream = st;
        max_blocks = fold_max_blocks();
        T.assign(m, e2_zero());
        G.assign(m, e2_zero());
        h_scal.assign(2 * m, e2_zero());
        size_t max_len;
        const FoldGTables A = fold_g_tables(sh, &max_len);
        one_word = A.n1 != 0;
        memset(&mem, 0, sizeof(mem));
        mem.rows0 = cm.d_rows;
        mem.g_stride = W;
        mem.scal_stride = 2 * m;
        std::vector<char> stage(sizeof(FoldGMember) + fold_gblock_bytes(sh, A, claims) + 16);
        static_assert(sizeof(FoldGMember) % 16 == 0, "a member's block starts at a multiple of 16");
        FoldGMember d;
        fold_gblock_fill(stage.data(), d, sizeof(FoldGMember), sh, A, claims, bpow, G1);
        memcpy(stage.data(), &d, sizeof(d));
        try {
            buf = fold_alloc(ctx, sh, 1, max_blocks);
        } catch (const std::exception& e) {
            throw Error(std::string("the context's arena cannot hold the reduction (") + e.what() + ")");
        }
        char* d_stage = ctx->alloc_n<char>(stage.size());
        hip_check(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload factor tables");
        ctx->prof_begin(cls, (double)W * 16 + (double)stage.size());
        k_pcsfold_g<<<dim3(fold_blocks_of(max_blocks, max_len, std::max<size_t>(A.nt, 1), 1), std::max<unsigned>(A.nt, 1)), FOLD_TPB, 0, st>>>(A, mem, d_stage, buf.g, buf.scal);
        ctx->prof_end();
        hip_check(hipStreamSynchronize(st), "hg_pcs_open_folded: sync");   // (the staged copy is a local)
        hip_check(hipGetLastError(), "hg_pcs_open_folded: launch");
    }
    void step(size_t j, E2 r, E2 s[3]) override {
        const Shape& sh = cm.sh;
        const size_t m = sh.nvars.size(), V = fold_rounds(sh);
        bool retire;
        size_t max_units, entries;
        const FoldTables A = fold_tables(sh, j, &retire, &max_units, &entries);
        retire |= j == 0 && one_word;
        if (s) s[0] = s[1] = s[2] = e2_zero();
        if (!A.nt && !retire) return;
        ctx->prof_stream = st;
        if (A.nt) {
            mem.r0 = r;
            ctx->prof_begin(cls, fold_step_bytes(j, entries));
            fold_launch(st, max_blocks, sh, j, A, max_units, 1, mem, buf, s != nullptr);
            ctx->prof_end();
            if (s) hip_check(hipMemcpyAsync(h_sums, buf.sums, sizeof(h_sums), hipMemcpyDeviceToHost, st), "download the round's sums");
        }
        if (retire) hip_check(hipMemcpyAsync(h_scal.data(), buf.scal, 2 * m * sizeof(E2), hipMemcpyDeviceToHost, st), "download the retired tables' scalars");
        hip_check(hipStreamSynchronize(st), "hg_pcs_open_folded: sync");
        hip_check(hipGetLastError(), "hg_pcs_open_folded: launch");
        ctx->prof_collect();
        if (s && A.nt) memcpy(s, h_sums, sizeof(h_sums));
        for (size_t t = 0; t < m; t++) {
            if (j == 0 && sh.nvars[t] == 0) { T[t] = h_scal[2 * t]; G[t] = G1[t]; }
            if (j > 0 && (size_t)sh.nvars[t] == j) { T[t] = h_scal[2 * t]; G[t] = h_scal[2 * t + 1]; }
        }
        if (j == V && hg_debug("plan"))   // (read at every call: the tests switch it per case)
            fprintf(stderr, "[hg plan] pcsfold V=%zu dev_rounds=%zu host_rounds=0 tables=%zu claims=%zu\n", V, V, m, n_claims);
    }
};
std::unique_ptr<FoldSource> fold_source_device(const Commitment& cm, const std::vector<Claim>& claims, const std::vector<E2>& bpow) {
    return std::unique_ptr<FoldSource>(new FoldDev(cm, claims, bpow));
}

// ---- the Goldilocks policy of the flows of pcs_flow.hpp. A row element is one word, an element of u and a weight an E2: a u vector
// is encoded as two rows (c0, c1) and a row offset in Row units is a word offset.
struct GlPcs {
    typedef u64 Row;
    typedef E2 W;
    typedef pcs::Claim Claim;
    typedef CombineJob Job;
    typedef pcs::VerifyItem VerifyItem;
    typedef pcs::OpenItem OpenItem;
    static constexpr size_t U_ROWS = 2, ALIGN = 16, TPB = PCS_TPB;
    static constexpr Field FIELD = GOLDILOCKS;
    static constexpr bool LEAF_AFTER_DOTS = false;
    static constexpr const char *CLS_VERIFY = "pcs_verify", *CLS_VERIFY_BATCH = "pcs_verify_batch", *CLS_OPEN_BATCH = "pcs_open_batch", *CLS_COMMIT_BATCH = "pcs_commit_batch",
                                *CLS_COMBINE = nullptr;
    static constexpr const char *VERIFY_NAME = "hg_pcs_verify_device", *OPEN_NAME = "hg_pcs_open", *TIMES_TAG = "", *NOT_BELOW = "a table holds a word that is not below p";
    static size_t opening_bytes(const Shape& sh, size_t n, size_t Q) { return pcs::opening_bytes(sh, n, Q); }
    // the folded opening (verify_folded_flow)
    static constexpr const char* VERIFY_FOLDED_NAME = "hg_pcs_verify_folded_device";
    static size_t folded_header_bytes(const Shape& sh) { return pcs::folded_header_bytes(sh); }
    static size_t folded_opening_bytes(const Shape& sh, size_t Q) { return pcs::folded_opening_bytes(sh, Q); }
    static FoldedHeader folded_header(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof) {
        return pcs::folded_header(sh, root, claims, Q, proof);
    }
    // the transcript
    static FsTranscript start_transcript(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q) { return pcs::start_transcript(sh, root, claims, Q); }
    static std::vector<E2> rho_powers(FsTranscript& tr, size_t R) { return pcs::rho_powers(tr.squeeze(), R); }
    static std::vector<E2> eq_table(const E2* pt, size_t n) { return pcs::eq_table(pt, n); }
    static void store_low(E2* dst, const E2* pt, int c) { memcpy(dst, pt, (size_t)c * sizeof(E2)); }
    static void absorb_opening(FsTranscript& tr, const uint8_t* proof, size_t n_u) {   // the u_i as the opening holds them: big-endian words
        std::vector<u64> words(2 * n_u);
        for (size_t i = 0; i < words.size(); i++) { u64 v; memcpy(&v, proof + 8 * i, 8); words[i] = __builtin_bswap64(v); }
        absorb_words(tr, words.data(), words.size());
    }
    static void absorb_u(FsTranscript& tr, const u64* words, size_t n_words) { absorb_words(tr, words, n_words); }
    static std::vector<size_t> squeeze_indices(FsTranscript& tr, size_t N, size_t Q) { return pcs::squeeze_indices(tr, N, Q); }
    // limits and sizes
    static bool ntt_needs_tmp(int depth) { return depth >= 8 && depth <= 16; }   // ntt_batch: the scratch of its four-step path
    static size_t dots_max_rows(size_t) { return ~(size_t)0; }                   // k_pcsvb_dots takes flat ids: no limit of its own
    static constexpr size_t COMMIT_BUDGET = VB_PCS_BUDGET, NTT_TMP = 0;          // the committer encodes a whole group at once, through a scratch of its size
    // what a member of the committer takes: its rows and encoded rows in the slab; the NTT scratch and its tree in the arena
    static size_t commit_member_bytes(size_t R, size_t C, size_t N) { return 8 * (R * C + 2 * R * N + 8 * N) + 4; }
    static void slab_spare(hg_ctx*, Slab&, size_t) {}   // every group's slab comes from the runtime and goes back to it

    // the steps of the committer
    static void stage(hg_ctx* ctx, int cls, hipStream_t st, size_t G, size_t R, int c, const u64*, u64* rows, u64* M, unsigned* flags) {
        const size_t C = (size_t)1 << c, N = (size_t)4 << c;
        ctx->prof_begin(cls, (double)G * R * (C + N) * 8);
        k_pcsb_stage<<<dim3((unsigned)std::min<size_t>(blocks_for(R * N), (4096 + G - 1) / G), (unsigned)G), PCS_TPB, 0, st>>>(rows, M, R, c, flags);   // about 4096 workgroups in all; G in the grid's y: cut_groups keeps it at VB_MAX_GROUP = 64 or below
        ctx->prof_end();
    }
    // the powers of the root and the encoding of `rows` rows, rows_a_call at a time
    static void ntt(hg_ctx* ctx, int cls, hipStream_t st, u64* a, u64* scratch, u64* W, int depth, size_t rows, size_t rows_a_call) {
        const size_t N = (size_t)1 << depth;
        ctx->prof_begin(cls, (double)rows * N * 32);
        dev::powers_table(st, W, root_of_unity(depth), N);
        for (size_t r0 = 0; r0 < rows; r0 += rows_a_call) dev::ntt_batch(st, a + r0 * N, depth, std::min(rows_a_call, rows - r0), W, 1, scratch);
        ctx->prof_end();
    }
    static void leaf_hash(hg_ctx* ctx, int cls, hipStream_t st, const u64* M, size_t G, int depth, size_t R, u64* trees, size_t tree_words) {
        ctx->prof_begin(cls, (double)(G << depth) * R * 8);
        k_pcsb_leaf_hash<<<blocks_for(G << depth), PCS_TPB, 0, st>>>(M, G, depth, R, trees, tree_words);
        ctx->prof_end();
    }
    // the steps of the verifiers
    static void canon(hg_ctx* ctx, int cls, hipStream_t st, unsigned cap, const u64* set, const VbMember* mem, const VbGroup& g, size_t u_total, size_t unit_max, u64* u,
                      u64* cols, u64* enc, u64* cells) {
        ctx->prof_begin(cls, (double)(u_total + g.G * g.Q * g.R) * 24);
        k_pcsvb_canon<<<dim3((unsigned)std::min<size_t>(blocks_for(unit_max), cap), (unsigned)g.G), PCS_TPB, 0, st>>>(set, mem, g, u, cols, enc, cells);
        ctx->prof_end();
    }
    static void eval(hg_ctx* ctx, int cls, hipStream_t st, const VbMember* mem, const VbGroup& g, size_t claims, const u64* u, const char* stage, u64* cells) {
        ctx->prof_begin(cls, (double)(claims << g.c) * 16);
        k_pcsvb_eval<<<(unsigned)claims, PCS_TPB, 0, st>>>(mem, (unsigned)g.G, g.c, u, stage, cells);
        ctx->prof_end();
    }
    static void leaf(hg_ctx* ctx, int cls, hipStream_t st, const VbMember* mem, const VbGroup& g, const u64* cols, u64* leaves) {
        ctx->prof_begin(cls, (double)g.G * g.Q * g.R * 8);
        k_pcsvb_leaf<<<blocks_for(g.G * g.Q), PCS_TPB, 0, st>>>(mem, g, cols, leaves);
        ctx->prof_end();
    }
    static void dots(hg_ctx* ctx, int cls, hipStream_t st, const VbMember* mem, const VbGroup& g, size_t jobs, size_t nw, const u64* cols, const char* stage, E2* s) {
        ctx->prof_begin(cls, (double)g.Q * nw * 24);
        k_pcsvb_dots<<<blocks_for(g.Q * jobs), PCS_TPB, 0, st>>>(mem, g, g.Q * jobs, cols, stage, s);
        ctx->prof_end();
    }
    static void query(hg_ctx* ctx, int cls, hipStream_t st, const u64* set, const VbMember* mem, const VbGroup& g, size_t jobs, const u64* leaves, const E2* s, const u64* enc,
                      const u64* js, const char* stage, u64* cells) {
        ctx->prof_begin(cls, (double)g.G * g.Q * 32.0 * g.depth + (double)g.Q * jobs * 48.0);
        k_pcsvb_query<<<blocks_for(g.G * g.Q), PCS_TPB, 0, st>>>(set, mem, g, leaves, s, enc, js, stage, cells);
        ctx->prof_end();
    }
    // the steps of the openers; cls < 0: not profiled (combine_device)
    static void combine(hg_ctx* ctx, int cls, hipStream_t st, int c, size_t jobs, size_t nw, size_t u_words, const ObJob<u64>* job, const char* stage, E2* u) {
        const size_t C = (size_t)1 << c;
        const unsigned cb = blocks_for(C);
        if (cls >= 0) ctx->prof_begin(cls, (double)nw * C * 8 + (double)u_words * 8);
        k_pcsob_combine<<<(unsigned)(jobs * cb), PCS_TPB, 0, st>>>(c, cb, job, stage, u);
        if (cls >= 0) ctx->prof_end();
    }
    static void ob_eval(hg_ctx* ctx, int cls, hipStream_t st, const ObClaim* claim, size_t claims, int c, const E2* u, const char* stage, u64* cells) {
        ctx->prof_begin(cls, (double)(claims << c) * 16);
        k_pcsob_eval<<<(unsigned)claims, PCS_TPB, 0, st>>>(claim, c, u, stage, cells);
        ctx->prof_end();
    }
    static void emit(hg_ctx* ctx, int cls, hipStream_t st, const ObMember<u64>* mem, size_t G, size_t u_words, const u64* u, u64* img) {
        ctx->prof_begin(cls, (double)u_words * 16);
        k_pcsob_emit<<<(unsigned)std::min<size_t>(blocks_for(u_words), 4096), PCS_TPB, 0, st>>>(mem, (unsigned)G, u_words, u, img);
        ctx->prof_end();
    }
    static void gather(hg_ctx* ctx, int cls, hipStream_t st, const ObMember<u64>* mem, size_t G, size_t Q, size_t R, size_t N, size_t q_words, size_t active, const u64* js,
                       u64* img) {
        ctx->prof_begin(cls, (double)active * Q * R * 16);
        k_pcsob_gather<<<blocks_for(G * Q * R), PCS_TPB, 0, st>>>(mem, G, Q, R, N, q_words, js, img);
        ctx->prof_end();
    }
    static void gather_one(hipStream_t st, const u64* M, size_t N, size_t R, size_t Q, const u64* js, u64* cols) {
        k_pcs_gather<<<dim3(blocks_for(R), (unsigned)Q), PCS_TPB, 0, st>>>(M, N, R, js, cols);
    }
    // the reduction of a run of folded openings (open_folded_batch_flow): the kernels and helpers of FoldDev over a group; a challenge
    // goes up as it is
    typedef pcs::FoldProver FoldProver;
    typedef pcs::FoldGTables FoldGTables;
    typedef pcs::FoldGMember FoldGMember;
    typedef pcs::FoldTables FoldTables;
    typedef pcs::FoldMembers FoldMembers;
    typedef pcs::FoldBufs FoldBufs;
    typedef E2 FoldChal;
    static constexpr const char *CLS_FOLD_BATCH = "pcs_fold_batch", *PLAN_FOLD_BATCH = "pcsfoldb";
    static unsigned fold_max_blocks() { return pcs::fold_max_blocks(); }
    static FoldGTables fold_g_tables(const Shape& sh, size_t* max_len) { return pcs::fold_g_tables(sh, max_len); }
    static size_t fold_gblock_bytes(const Shape& sh, const FoldGTables& A, const std::vector<Claim>& claims) { return pcs::fold_gblock_bytes(sh, A, claims); }
    static void fold_gblock_fill(char* stage, FoldGMember& d, size_t at, const Shape& sh, const FoldGTables& A, const std::vector<Claim>& claims, const std::vector<E2>& bpow,
                                 std::vector<E2>& G1) {
        pcs::fold_gblock_fill(stage, d, at, sh, A, claims, bpow, G1);
    }
    static FoldBufs fold_alloc(hg_ctx* ctx, const Shape& sh, size_t G, unsigned max_blocks) { return pcs::fold_alloc(ctx, sh, G, max_blocks); }
    static FoldTables fold_tables(const Shape& sh, size_t j, bool* retire, size_t* max_units, size_t* entries) { return pcs::fold_tables(sh, j, retire, max_units, entries); }
    static E2 fold_chal(E2 r) { return r; }
    static FoldMembers fold_members(const Shape& sh, const u64* const* rows, const E2* r) {
        FoldMembers M;
        memset(&M, 0, sizeof(M));
        M.rows = rows;
        M.r = r;
        M.g_stride = sh.R << sh.c;
        M.scal_stride = 2 * sh.nvars.size();
        return M;
    }
    static void fold_g_launch(hipStream_t st, unsigned max_blocks, const FoldGTables& A, size_t max_len, size_t G, const FoldMembers& M, const char* d_stage, const FoldBufs& b) {
        k_pcsfold_g<<<dim3(fold_blocks_of(max_blocks, max_len, std::max<size_t>(A.nt, 1), G), std::max<unsigned>(A.nt, 1), (unsigned)G), FOLD_TPB, 0, st>>>(A, M, d_stage, b.g, b.scal);
    }
    static void fold_launch(hipStream_t st, unsigned max_blocks, const Shape& sh, size_t j, const FoldTables& A, size_t max_units, size_t G, const FoldMembers& M, const FoldBufs& b,
                            bool sums) {
        pcs::fold_launch(st, max_blocks, sh, j, A, max_units, G, M, b, sums);
    }
    static double fold_step_bytes(size_t j, size_t entries) { return pcs::fold_step_bytes(j, entries); }
};

void combine_device(const Commitment& cm, const std::vector<CombineJob>& jobs, E2* u) { combine_flow<GlPcs>(cm, jobs, u); }
void columns_device(const Commitment& cm, const std::vector<size_t>& js, u64* cols) { columns_flow<GlPcs>(cm, js, cols); }
std::string verify_device(hg_ctx* ctx, const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    return verify_flow<GlPcs>(ctx, sh, root, claims, Q, proof, len);
}
// the device verifier of a folded opening: verify_folded_flow of pcs_flow.hpp
std::string verify_folded_device(hg_ctx* ctx, const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    return verify_folded_flow<GlPcs>(ctx, sh, root, claims, Q, proof, len);
}
std::vector<std::string> verify_device_batch(const char* who, hg_ctx* ctx, const Shape& sh, const std::vector<VerifyItem>& items, size_t Q) {
    return verify_batch_flow<GlPcs>(who, ctx, sh, items, Q);
}
std::vector<Commitment*> commit_device_batch(const char* who, hg_ctx* ctx, const Shape& sh, const u64* const* tables, size_t n) {
    return commit_batch_flow<GlPcs>(who, ctx, sh, tables, n, false);
}
std::vector<Opened> open_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<OpenItem>& items, size_t Q) {
    return open_batch_flow<GlPcs>(who, single, ctx, items, Q);
}

std::vector<std::string> verify_folded_device_batch(const char* who, hg_ctx* ctx, const Shape& sh, const std::vector<VerifyItem>& items, size_t Q) {
    return verify_batch_flow<GlPcs>(who, ctx, sh, items, Q, true);
}

// hg_pcs_open_folded_batch: open_folded_batch_flow of pcs_flow.hpp over the kernels and helpers of the reduction above
std::vector<Opened> open_folded_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<OpenItem>& items, size_t Q) {
    return open_folded_batch_flow<GlPcs>(who, single, ctx, items, Q);
}

}  // namespace pcs
}  // namespace hg
