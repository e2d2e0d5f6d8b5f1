// Device form of the polynomial commitment over bn256::Fr (pcs_bn254.hpp), part of bn254.hip. Rows and the encoded matrix lie in
// HBM as canonical plain words (4 an element): the transform is linear and its twiddle products are Montgomery products with
// Montgomery-form powers of w, so plain words go through ntt_batch_dev and come out plain - no conversion pass on either NTT path,
// and the leaf hash and the column gather read the matrix as it is. Keccak and the tree are those of the Goldilocks form
// (pcs_keccak.hpp, pcs::merkle_levels_device): a node is 32 bytes in either field.

constexpr int BNPCS_TPB = 256;
static unsigned bnpcs_blocks(size_t n) { return (unsigned)((n + BNPCS_TPB - 1) / BNPCS_TPB); }

// rows[i] = the signed lift of witness word i (canonical): the secrets wrapper uploads 8 bytes an element
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_lift(const u64* __restrict__ words, Fr* __restrict__ rows, size_t n) {
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * BNPCS_TPB) lz_gstore(rows + i, fr_lift_signed_canon(words[i]));
}
// M[r][j] = j < C ? rows[r][j] : 0 ahead of the encoding; an element that is not below r sets *flag
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_stage(const Fr* __restrict__ rows, Fr* __restrict__ M, size_t R, int c, unsigned* __restrict__ flag) {
    const size_t total = R << (c + 2);
    const size_t C = (size_t)1 << c, Nm = ((size_t)4 << c) - 1;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * BNPCS_TPB) {
        const size_t r = i >> (c + 2), j = i & Nm;
        Fr v = fr_zero();
        if (j < C) { v = lz_gload(rows + (r << c) + j); bad |= fr_geq_p(v); }
        lz_gstore(M + i, v);
    }
    if (bad) atomicOr(flag, 1u);
}

// One thread per column j of the encoded matrix: leaves[j] = Keccak256(LE64(0) || repr(M[0][j]) || .. || repr(M[R-1][j])). The
// message is 4R + 1 words, the prefix first; 17 words per permutation; padding 0x01 .. 0x80 (in one word when they meet). Message
// word w >= 1 is word (w - 1) & 3 of element (w - 1) >> 2: the address is computed, the lane of the state it goes to is a
// compile-time constant. A wavefront reads 64 adjacent elements of a row; the four words of an element come from one 32-byte sector.
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_leaf_hash(const Fr* __restrict__ M, size_t N, size_t R, u64* __restrict__ leaves) {
    const size_t j = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (j >= N) return;
    const u64* __restrict__ col = reinterpret_cast<const u64*>(M + j);
    const size_t stride = 4 * N;                      // words between the rows
    u64 a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = 0;
    const size_t words = 4 * R + 1;
    const size_t blocks = words / pcs::RATE_WORDS + 1;     // the last block holds the rest (possibly nothing) and the padding
    for (size_t b = 0; b < blocks; b++) {
        const size_t base = b * pcs::RATE_WORDS;
#pragma unroll
        for (int i = 0; i < pcs::RATE_WORDS; i++) {
            const size_t idx = base + i;
            u64 w = 0;
            if (idx >= 1 && idx < words) w = col[((idx - 1) >> 2) * stride + ((idx - 1) & 3)];
            if (idx == words) w = 0x01;
            a[i] ^= w;
        }
        if (b + 1 == blocks) a[pcs::RATE_WORDS - 1] ^= 0x8000000000000000ull;
        pcs::keccak_f(a);
    }
    u64* out = leaves + 4 * j;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}

// w += a * b for a weight b whose eight 32-bit limbs are wave-uniform (held in SGPRs: one constant-bus operand per multiply-add)
__device__ __forceinline__ void bnpcs_mac_uniform(WCol& w, const Fr& a, const u32 (&bl)[8]) {
    u32 al[8];
#pragma unroll
    for (int i = 0; i < 4; i++) { al[2 * i] = (u32)a.l[i]; al[2 * i + 1] = (u32)(a.l[i] >> 32); }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        BN_WIDE_ROW4S(w.C[i], w.C[i + 1], w.C[i + 2], w.C[i + 3], w.T[i], w.T[i + 1], w.T[i + 2], w.T[i + 3], al[i], bl[0], bl[1], bl[2], bl[3]);
        BN_WIDE_ROW4S(w.C[i + 4], w.C[i + 5], w.C[i + 6], w.C[i + 7], w.T[i + 4], w.T[i + 5], w.T[i + 6], w.T[i + 7], al[i], bl[4], bl[5], bl[6], bl[7]);
    }
}
// Row combinations of an opening. Job q (blockIdx.y): u_q[j] = sum_{r < nrows} w[woff + r] * rows[row0 + r][j]; a thread owns column j,
// the weight is uniform over the workgroup. Products of a canonical element and a Montgomery-form weight go into the column
// accumulators and are reduced every BNPCS_CHUNK rows by lz_reduce, which takes a value below 2^12 p^2: both factors are below
// p, so a chunk sums to less than BNPCS_CHUNK p^2 and any BNPCS_CHUNK <= 4096 = 2^12 is inside the bound. 1024 is chosen: a
// quarter of the bound (also inside wcol_reduce's 2^10 r^2), and the reduction is already 1/1024 of the multiply-adds. The carry
// counters (32 bits, at most one carry a multiply-add, 16 multiply-adds a column and product) are nowhere near their range.
struct BnPcsDesc { u64 row0, nrows, woff; };
constexpr int BNPCS_CHUNK = 1024;
static_assert(BNPCS_CHUNK <= 4096, "lz_reduce takes a value below 2^12 p^2");
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_combine(const Fr* __restrict__ rows, int c, const BnPcsDesc* __restrict__ jobs, const Fr* __restrict__ w,
                                                             Fr* __restrict__ u) {
    const size_t C = (size_t)1 << c;
    const size_t j = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (j >= C) return;
    const BnPcsDesc job = jobs[blockIdx.y];
    const Fr* src = rows + (job.row0 << c) + j;
    const u32* wq = reinterpret_cast<const u32*>(w + job.woff);
    Fr s = fr_zero();
    for (u64 r0 = 0; r0 < job.nrows; r0 += BNPCS_CHUNK) {
        const u64 r1 = r0 + BNPCS_CHUNK < job.nrows ? r0 + BNPCS_CHUNK : job.nrows;
        WCol A = wcol_zero();
        for (u64 r = r0; r < r1; r++) {
            const Fr x = lz_gload(src + (r << c));
            u32 bl[8];
#pragma unroll
            for (int k = 0; k < 8; k++) bl[k] = __builtin_amdgcn_readfirstlane(wq[8 * r + k]);
            bnpcs_mac_uniform(A, x, bl);
        }
        s = lz_add(s, lz_reduce(A));
    }
    lz_gstore(u + (size_t)blockIdx.y * C + j, lz_canon(s));
}

// cols[q][r] = M[r][js[q]]
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_gather(const Fr* __restrict__ M, size_t N, size_t R, const u64* __restrict__ js, Fr* __restrict__ cols) {
    const size_t r = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (r >= R) return;
    lz_gstore(cols + (size_t)blockIdx.y * R + r, lz_gload(M + r * N + js[blockIdx.y]));
}

// One stream, one synchronisation. The NTT temporary (the size of the encoded matrix) and the uploaded witness words live in the
// context's arena and go back to it with the next arena_reset; the handle owns the raw rows and the encoded matrix.
pcs::Commitment* pcs_commit_device(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tables, bool words) {
    const std::string me(who);
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    std::unique_ptr<pcs::Commitment> cm(new pcs::Commitment());
    cm->field = pcs::BN254;
    cm->sh = sh;
    cm->ctx = ctx;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int log2n = sh.depth();
    if (R > 65535) throw Error(me + ": more than 65535 rows (choose a larger log2_row)");
    hipc(hipMalloc((void**)&cm->d_rows, R * C * sizeof(Fr)), "hipMalloc(pcs rows)");
    hipc(hipMalloc((void**)&cm->d_M, R * N * sizeof(Fr)), "hipMalloc(pcs encoded matrix)");
    Fr* d_rows = reinterpret_cast<Fr*>(cm->d_rows);
    Fr* d_M = reinterpret_cast<Fr*>(cm->d_M);
    Fr* tmp = ctx->alloc_n<Fr>(R * N);
    Fr* W = ctx->alloc_n<Fr>(N);
    u64* d_tree = ctx->alloc_n<u64>(4 * 2 * N);
    unsigned* d_flag = ctx->alloc_n<unsigned>(4);
    u64* d_words = words ? ctx->alloc_n<u64>(R * C) : nullptr;
    const int c_stage = ctx->prof_class("pcs_bn254_stage", false), c_ntt = ctx->prof_class("pcs_bn254_ntt", false), c_leaf = ctx->prof_class("pcs_bn254_leaf", false),
              c_tree = ctx->prof_class("pcs_bn254_tree", false);
    ctx->prof_stream = st;
    struct Drain {   // an error between the first enqueue and the synchronisation must not leave copies of the caller's tables behind
        hipStream_t st; bool armed = true;
        ~Drain() { if (armed) (void)hipStreamSynchronize(st); }
    } drain{st};
    hipc(hipMemsetAsync(d_flag, 0, 16, st), "memset");
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t len = (size_t)1 << sh.nvars[t];
        if (words) hipc(hipMemcpyAsync(d_words + sh.off[t] * C, tables[t], len * 8, hipMemcpyHostToDevice, st), "upload tables");
        else hipc(hipMemcpyAsync(d_rows + sh.off[t] * C, tables[t], len * sizeof(Fr), hipMemcpyHostToDevice, st), "upload tables");
    }
    ctx->prof_begin(c_stage, (double)R * C * (words ? 40 : 0) + (double)R * C * 32 + (double)R * N * 32);
    if (words) k_bnpcs_lift<<<(unsigned)std::min<size_t>(bnpcs_blocks(R * C), 4096), BNPCS_TPB, 0, st>>>(d_words, d_rows, R * C);
    k_bnpcs_stage<<<(unsigned)std::min<size_t>(bnpcs_blocks(R * N), 4096), BNPCS_TPB, 0, st>>>(d_rows, d_M, R, sh.c, d_flag);
    ctx->prof_end();
    ctx->prof_begin(c_ntt, (double)R * N * 32 * 4);
    k_bn_powers<<<bnpcs_blocks(N), 256, 0, st>>>(W, fr_root_of_unity(log2n), N);
    ntt_batch_dev(st, d_M, tmp, W, log2n, R, nullptr);
    ctx->prof_end();
    ctx->prof_begin(c_leaf, (double)R * N * 32);
    k_bnpcs_leaf_hash<<<bnpcs_blocks(N), BNPCS_TPB, 0, st>>>(d_M, N, R, d_tree);
    ctx->prof_end();
    ctx->prof_begin(c_tree, (double)N * 96);
    pcs::merkle_levels_device(st, d_tree, N);
    ctx->prof_end();
    cm->tree.resize(32 * (2 * N - 1));
    unsigned flag = 0;
    hipc(hipMemcpyAsync(cm->tree.data(), d_tree, cm->tree.size(), hipMemcpyDeviceToHost, st), "download tree");
    hipc(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st), "download flag");
    const hipError_t synced = hipStreamSynchronize(st);
    drain.armed = false;
    hipc(synced, (me + ": sync").c_str());
    hipc(hipGetLastError(), (me + ": launch").c_str());
    ctx->prof_collect();
    if (flag) throw Error(me + ": a table holds an element that is not below r");
    return cm.release();
}

void pcs_combine_device(const pcs::Commitment& cm, const std::vector<PcsJob>& jobs, Fr* u) {
    hg_ctx* ctx = cm.ctx;
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t C = cm.sh.C(), nj = jobs.size();
    if (nj > 65535) throw Error("hg_pcs_open_bn254: more than 65534 claims");
    // descriptors and weights in one staged copy
    size_t nw = 0;
    for (const PcsJob& j : jobs) nw += j.nrows;
    const size_t desc_bytes = (nj * sizeof(BnPcsDesc) + 31) & ~(size_t)31;
    std::vector<char> stage(desc_bytes + nw * sizeof(Fr));
    BnPcsDesc* hd = reinterpret_cast<BnPcsDesc*>(stage.data());
    char* hw = stage.data() + desc_bytes;
    size_t off = 0;
    for (size_t q = 0; q < nj; q++) {
        hd[q].row0 = jobs[q].row0; hd[q].nrows = jobs[q].nrows; hd[q].woff = off;
        memcpy(hw + off * sizeof(Fr), jobs[q].w.data(), jobs[q].nrows * sizeof(Fr));
        off += jobs[q].nrows;
    }
    char* d_stage = ctx->alloc_n<char>(stage.size());
    Fr* d_u = ctx->alloc_n<Fr>(nj * C);
    const int cls = ctx->prof_class("pcs_bn254_combine", false);
    ctx->prof_stream = st;
    hipc(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload weights");
    ctx->prof_begin(cls, (double)nw * C * 32);
    k_bnpcs_combine<<<dim3(bnpcs_blocks(C), (unsigned)nj), BNPCS_TPB, 0, st>>>(reinterpret_cast<const Fr*>(cm.d_rows), cm.sh.c, reinterpret_cast<const BnPcsDesc*>(d_stage),
                                                                               reinterpret_cast<const Fr*>(d_stage + desc_bytes), d_u);
    ctx->prof_end();
    hipc(hipMemcpyAsync(u, d_u, nj * C * sizeof(Fr), hipMemcpyDeviceToHost, st), "download combinations");
    hipc(hipStreamSynchronize(st), "hg_pcs_open_bn254: sync");
    hipc(hipGetLastError(), "hg_pcs_open_bn254: launch");
    ctx->prof_collect();
}

void pcs_columns_device(const pcs::Commitment& cm, const std::vector<size_t>& js, Fr* cols) {
    hg_ctx* ctx = cm.ctx;
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    const size_t N = cm.sh.N(), R = cm.sh.R, Q = js.size();
    if (Q > 65535) throw Error("hg_pcs_open_bn254: more than 65535 queries on the device");
    std::vector<u64> hj(js.begin(), js.end());
    u64* d_js = ctx->alloc_n<u64>(Q);
    Fr* d_cols = ctx->alloc_n<Fr>(Q * R);
    hipc(hipMemcpyAsync(d_js, hj.data(), Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
    k_bnpcs_gather<<<dim3(bnpcs_blocks(R), (unsigned)Q), BNPCS_TPB, 0, st>>>(reinterpret_cast<const Fr*>(cm.d_M), N, R, d_js, d_cols);
    hipc(hipMemcpyAsync(cols, d_cols, Q * R * sizeof(Fr), hipMemcpyDeviceToHost, st), "download columns");
    hipc(hipStreamSynchronize(st), "hg_pcs_open_bn254: sync");
    hipc(hipGetLastError(), "hg_pcs_open_bn254: launch");
}
