// Device form of the polynomial commitment (pcs.hpp): rows staged into the zero-padded 4C-stride matrix and encoded by the batched
// NTT, one Keccak-f[1600] state per thread for the column hashes and the tree, the E x F row combinations of an opening through
// the deferred-reduction accumulators, a gather of the opened columns. The handle owns the raw and the encoded matrix in HBM.
#include "pcs.hpp"
#include "prover.hpp"
#include "gl_wide.hpp"

namespace hg {
namespace pcs {

constexpr int PCS_TPB = 256;

// ---- Keccak-f[1600], the whole state in registers: 24 rounds unrolled, every lane index a compile-time constant (a run-time index
// would put the state into scratch memory)
__device__ constexpr u64 KRC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
__device__ constexpr int KROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // rho offsets, lane x + 5y
__device__ __forceinline__ u64 krotl(u64 v, int s) { return s ? (v << s) | (v >> (64 - s)) : v; }
__device__ __forceinline__ void keccak_f(u64 (&a)[25]) {
#pragma unroll
    for (int rd = 0; rd < 24; rd++) {
        u64 c[5], d[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ krotl(c[(x + 1) % 5], 1);
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] ^= d[i % 5];
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = krotl(a[x + 5 * y], KROT[x + 5 * y]);
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= KRC[rd];
    }
}
constexpr int RATE_WORDS = 17;   // Keccak-256: 136 bytes

// M[r][j] = j < C ? rows[r][j] : 0 ahead of the encoding; a word that is not below p sets *flag
__global__ __launch_bounds__(PCS_TPB) void k_pcs_stage(const u64* __restrict__ rows, u64* __restrict__ M, size_t R, int c, unsigned* __restrict__ flag) {
    const size_t total = R << (c + 2);
    const size_t C = (size_t)1 << c, Nm = ((size_t)4 << c) - 1;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * PCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * PCS_TPB) {
        const size_t r = i >> (c + 2), j = i & Nm;
        u64 v = 0;
        if (j < C) { v = rows[(r << c) + j]; bad |= v >= GL_P; }
        M[i] = v;
    }
    if (bad) atomicOr(flag, 1u);
}

// One thread per column j of the encoded matrix: Keccak256(LE64(0) || M[0][j] || .. || M[R-1][j]) -> leaves[j]. A wavefront reads
// 64 adjacent words of a row at a time. 17 message words per permutation, the prefix word first; padding 0x01 .. 0x80.
__global__ __launch_bounds__(PCS_TPB) void k_pcs_leaf_hash(const u64* __restrict__ M, size_t N, size_t R, u64* __restrict__ leaves) {
    const size_t j = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (j >= N) return;
    u64 a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    const size_t words = R + 1;                       // message words, the prefix included
    const size_t blocks = words / RATE_WORDS + 1;     // the last block holds the rest (possibly nothing) and the padding
    const u64* col = M + j;
    for (size_t b = 0; b < blocks; b++) {
        const size_t base = b * RATE_WORDS;
#pragma unroll
        for (int i = 0; i < RATE_WORDS; i++) {
            const size_t idx = base + i;              // word 0 is LE64(0), word idx >= 1 is M[idx - 1][j]
            u64 w = 0;
            if (idx >= 1 && idx < words) w = col[(idx - 1) * N];
            if (idx == words) w = 0x01;
            a[i] ^= w;
        }
        if (b + 1 == blocks) a[RATE_WORDS - 1] ^= 0x8000000000000000ull;
        keccak_f(a);
    }
    u64* out = leaves + 4 * j;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}

__device__ __forceinline__ void merkle_node(const u64* below, u64* here, size_t i) {
    u64 a[25];
    const u64* in = below + 8 * i;   // left || right
    a[0] = 1;
#pragma unroll
    for (int k = 0; k < 8; k++) a[1 + k] = in[k];
    a[9] = 0x01;
#pragma unroll
    for (int k = 10; k < 25; k++) a[k] = 0;
    a[RATE_WORDS - 1] = 0x8000000000000000ull;
    keccak_f(a);
    u64* out = here + 4 * i;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}
// One level of the tree: node i of `here` = Keccak256(LE64(1) || nodes 2i and 2i + 1 of `below`), one permutation a node
__global__ __launch_bounds__(PCS_TPB) void k_pcs_merkle(const u64* __restrict__ below, u64* __restrict__ here, size_t count) {
    const size_t i = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (i < count) merkle_node(below, here, i);
}
// The levels from `count` (<= PCS_TPB) nodes up to the root in one workgroup; the levels lie one behind the other in the tree buffer
__global__ __launch_bounds__(PCS_TPB) void k_pcs_merkle_top(u64* below, size_t count) {
    while (count >= 1) {
        u64* here = below + 8 * count;   // `below` has 2 * count nodes of 4 words
        if (threadIdx.x < count) merkle_node(below, here, threadIdx.x);
        __syncthreads();
        below = here;
        count >>= 1;
    }
}

// Row combinations of an opening. Job q (blockIdx.y): u_q[j] = sum_{r < nrows} w[woff + r] * rows[row0 + r][j]; a thread owns column
// j. The weights are uniform over the workgroup. Products go into two column accumulators (c0 and c1 of the weight) that are
// reduced every COMBINE_CHUNK rows: the carry counters of gl_wide.hpp stay below 2^8 for up to 127 products.
struct CombineDesc { u64 row0, nrows, woff; };
constexpr int COMBINE_CHUNK = 64;
__global__ __launch_bounds__(PCS_TPB) void k_pcs_combine(const u64* __restrict__ rows, int c, const CombineDesc* __restrict__ jobs, const E2* __restrict__ w,
                                                         E2* __restrict__ u) {
    const size_t C = (size_t)1 << c;
    const size_t j = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (j >= C) return;
    const CombineDesc job = jobs[blockIdx.y];
    const u64* src = rows + (job.row0 << c) + j;
    const E2* wq = w + job.woff;
    u64 s0 = 0, s1 = 0;
    for (u64 r0 = 0; r0 < job.nrows; r0 += COMBINE_CHUNK) {
        const u64 r1 = r0 + COMBINE_CHUNK < job.nrows ? r0 + COMBINE_CHUNK : job.nrows;
        WAcc A = wacc_zero(), B = wacc_zero();
        for (u64 r = r0; r < r1; r++) {
            const u64 x = src[r << c];
            const E2 wr = wq[r];
            wmac2(A, x, wr.c0, B, x, wr.c1);
        }
        s0 = gl_add(s0, wreduce(A));
        s1 = gl_add(s1, wreduce(B));
    }
    u[(size_t)blockIdx.y * C + j] = e2(s0, s1);
}

// cols[q][r] = M[r][js[q]]
__global__ __launch_bounds__(PCS_TPB) void k_pcs_gather(const u64* __restrict__ M, size_t N, size_t R, const u64* __restrict__ js, u64* __restrict__ cols) {
    const size_t r = (size_t)blockIdx.x * PCS_TPB + threadIdx.x;
    if (r >= R) return;
    cols[(size_t)blockIdx.y * R + r] = M[r * N + js[blockIdx.y]];
}

Commitment::~Commitment() {
    if (d_rows) (void)hipFree(d_rows);
    if (d_M) (void)hipFree(d_M);
}

static unsigned blocks_for(size_t n) { return (unsigned)((n + PCS_TPB - 1) / PCS_TPB); }

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
    k_pcs_stage<<<(unsigned)std::min<size_t>(blocks_for(R * N), 4096), PCS_TPB, 0, st>>>(cm->d_rows, cm->d_M, R, sh.c, d_flag);
    dev::powers_table(st, W, root_of_unity(log2n), N);
    dev::ntt_batch(st, cm->d_M, log2n, R, W, 1, scratch);
    k_pcs_leaf_hash<<<blocks_for(N), PCS_TPB, 0, st>>>(cm->d_M, N, R, d_tree);
    u64* below = d_tree;
    size_t count = N / 2;
    for (; count > (size_t)PCS_TPB; count >>= 1) {
        k_pcs_merkle<<<blocks_for(count), PCS_TPB, 0, st>>>(below, below + 8 * count, count);
        below += 8 * count;
    }
    k_pcs_merkle_top<<<1, PCS_TPB, 0, st>>>(below, count);
    cm->tree.resize(32 * (2 * N - 1));
    unsigned flag = 0;
    hip_check(hipMemcpyAsync(cm->tree.data(), d_tree, cm->tree.size(), hipMemcpyDeviceToHost, st), "download tree");
    hip_check(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st), "download flag");
    hip_check(hipStreamSynchronize(st), "hg_pcs_commit: sync");
    hip_check(hipGetLastError(), "hg_pcs_commit: launch");
    if (flag) throw Error("hg_pcs_commit: a table holds a word that is not below p");
    return cm.release();
}

void combine_device(const Commitment& cm, const std::vector<CombineJob>& jobs, E2* u) {
    hg_ctx* ctx = cm.ctx;
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t C = cm.sh.C(), nj = jobs.size();
    if (nj > 65535) throw Error("hg_pcs_open: more than 65534 claims");
    // descriptors and weights in one staged copy
    size_t nw = 0;
    for (const CombineJob& j : jobs) nw += j.nrows;
    const size_t desc_bytes = (nj * sizeof(CombineDesc) + 15) & ~(size_t)15;
    std::vector<char> stage(desc_bytes + nw * sizeof(E2));
    CombineDesc* hd = reinterpret_cast<CombineDesc*>(stage.data());
    E2* hw = reinterpret_cast<E2*>(stage.data() + desc_bytes);
    size_t off = 0;
    for (size_t q = 0; q < nj; q++) {
        hd[q].row0 = jobs[q].row0; hd[q].nrows = jobs[q].nrows; hd[q].woff = off;
        memcpy(hw + off, jobs[q].w.data(), jobs[q].nrows * sizeof(E2));
        off += jobs[q].nrows;
    }
    char* d_stage = ctx->alloc_n<char>(stage.size());
    E2* d_u = ctx->alloc_n<E2>(nj * C);
    hip_check(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload weights");
    k_pcs_combine<<<dim3(blocks_for(C), (unsigned)nj), PCS_TPB, 0, st>>>(cm.d_rows, cm.sh.c, reinterpret_cast<const CombineDesc*>(d_stage),
                                                                         reinterpret_cast<const E2*>(d_stage + desc_bytes), d_u);
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

}  // namespace pcs
}  // namespace hg
