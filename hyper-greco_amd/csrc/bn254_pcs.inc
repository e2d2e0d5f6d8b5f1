// Device form of the polynomial commitment over bn256::Fr (pcs_bn254.hpp), part of bn254.hip. Rows and the encoded matrix lie in
// HBM as canonical plain words (4 an element): the transform is linear and its twiddle products are Montgomery products with
// Montgomery-form powers of w, so plain words go through ntt_batch_dev and come out plain - no conversion pass on either NTT path,
// and the leaf hash and the column gather read the matrix as it is. Keccak and the tree are those of the Goldilocks form
// (pcs_keccak.hpp, pcs::merkle_levels_device): a node is 32 bytes in either field.
// The verifier of an opening reuses the encoding, the leaf sponge and the accumulators and adds five kernels.
// Every step has one kernel, written for a group of members and driven by a member or job table (the descriptors of pcs_flow.hpp,
// which both fields share); the forms for a run launch it once over a group, whose matrices lie in one allocation that its handles
// share, and the forms for one launch it over a group of one.
// The host flows of the verifiers, the batch opener, the batch committer, pcs_combine_device and pcs_columns_device are the templates
// of pcs_flow.hpp, written once for both fields; this file gives them BnPcs, the BN254 policy: the types, the transcript calls, the
// texts and one launch function per kernel step. pcs_commit_device and pcs_commit_words_enqueue keep a host flow of their own.
// The prover's side of a folded opening (pcs_bn254.hpp PcsFoldSource) is at the end: the kernel that builds g, the round kernels of the
// reduction sum-check - written for a group of members, the single call a group of one - their host driver for one opening,
// BnFoldDev, and BnFoldPcs, through which open_folded_batch_flow of pcs_flow.hpp drives them for a run.

constexpr int BNPCS_TPB = 256;
static unsigned bnpcs_blocks(size_t n) { return (unsigned)((n + BNPCS_TPB - 1) / BNPCS_TPB); }

// rows[i] = the signed lift of witness word i (canonical): the secrets wrapper uploads 8 bytes an element
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_lift(const u64* __restrict__ words, Fr* __restrict__ rows, size_t n) {
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * BNPCS_TPB) lz_gstore(rows + i, fr_lift_signed_canon(words[i]));
}
// ---- the kernels of a commitment, written for a group of G members of one shape (pcs_commit_device_batch); one commitment is a
// group of one. Member m's raw rows lie at rows + m R C, its encoded rows at M + m R N and its tree at trees + m tree_words.
// blockIdx.y = the member, its elements grid-strided over blockIdx.x: M[r][j] = j < C ? rows[r][j] : 0 ahead of the encoding; an
// element that is not below r (all four limbs compared) sets the member's flag
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsb_stage(const Fr* __restrict__ rows, Fr* __restrict__ M, size_t R, int c, unsigned* __restrict__ flags) {
    const size_t total = R << (c + 2);
    const size_t C = (size_t)1 << c, Nm = ((size_t)4 << c) - 1;
    const Fr* src = rows + (((size_t)blockIdx.y * R) << c);
    Fr* dst = M + (size_t)blockIdx.y * total;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * BNPCS_TPB) {
        const size_t r = i >> (c + 2), j = i & Nm;
        Fr v = fr_zero();
        if (j < C) { v = lz_gload(src + (r << c) + j); bad |= fr_geq_p(v); }
        lz_gstore(dst + i, v);
    }
    if (bad) atomicOr(flags + blockIdx.y, 1u);
}

// The sponge of a leaf: a = the state after Keccak256(LE64(0) || repr(e_0) || .. || repr(e_{R-1})), element r at col + r * stride
// (words). The message is 4R + 1 words, the prefix first; 17 words per permutation; padding 0x01 .. 0x80 (in one word when they
// meet). Message word w >= 1 is word (w - 1) & 3 of element (w - 1) >> 2: the address is computed, the lane of the state it goes
// to is a compile-time constant.
__device__ __forceinline__ void bnpcs_leaf_absorb(const u64* __restrict__ col, size_t stride, size_t R, u64 (&a)[25]) {
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
}
// One thread per (member m, column j) of the encoded matrices (N = 2^depth columns), id = m N + j: the leaf hash of the member's
// M[0][j] .. M[R-1][j] into the leaves of its own tree. A wavefront reads 64 adjacent elements of a row; the four words of an element
// come from one 32-byte sector. A member's columns may begin inside a wavefront (N < 64): every address comes from the thread's own
// m and j.
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsb_leaf_hash(const Fr* __restrict__ M, size_t G, int depth, size_t R, u64* __restrict__ trees, size_t tree_words) {
    const size_t id = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (id >= G << depth) return;
    const size_t N = (size_t)1 << depth, m = id >> depth, j = id & (N - 1);
    u64 a[25];
    bnpcs_leaf_absorb(reinterpret_cast<const u64*>(M + m * R * N + j), 4 * N, R, a);   // 4N words between the rows
    u64* out = trees + m * tree_words + 4 * j;
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
// sum_{r < nrows} w[r] * src[r << shift], canonical, for weights that are uniform over the wavefront (their limbs go through
// readfirstlane). Products of a canonical element and a Montgomery-form weight go into the column accumulators and are reduced
// every BNPCS_CHUNK rows by lz_reduce, which takes a value below 2^12 p^2: both factors are below p, so a chunk sums to less than
// BNPCS_CHUNK p^2 and any BNPCS_CHUNK <= 4096 = 2^12 is inside the bound. 1024 is chosen: a quarter of the bound (also inside
// wcol_reduce's 2^10 r^2), and the reduction is already 1/1024 of the multiply-adds. The carry counters (32 bits, at most one carry
// a multiply-add, 16 multiply-adds a column and product) are nowhere near their range.
constexpr int BNPCS_CHUNK = 1024;
static_assert(BNPCS_CHUNK <= 4096, "lz_reduce takes a value below 2^12 p^2");
__device__ __forceinline__ Fr bnpcs_dot_chunked(const Fr* __restrict__ src, int shift, const Fr* __restrict__ w, u64 nrows) {
    const u32* wq = reinterpret_cast<const u32*>(w);
    Fr s = fr_zero();
    for (u64 r0 = 0; r0 < nrows; r0 += BNPCS_CHUNK) {
        const u64 r1 = r0 + BNPCS_CHUNK < nrows ? r0 + BNPCS_CHUNK : nrows;
        WCol A = wcol_zero();
        for (u64 r = r0; r < r1; r++) {
            const Fr x = lz_gload(src + (r << shift));
            u32 bl[8];
#pragma unroll
            for (int k = 0; k < 8; k++) bl[k] = __builtin_amdgcn_readfirstlane(wq[8 * r + k]);
            bnpcs_mac_uniform(A, x, bl);
        }
        s = lz_add(s, lz_reduce(A));
    }
    return lz_canon(s);
}

// cols[q][r] = M[r][js[q]]
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_gather(const Fr* __restrict__ M, size_t N, size_t R, const u64* __restrict__ js, Fr* __restrict__ cols) {
    const size_t r = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (r >= R) return;
    lz_gstore(cols + (size_t)blockIdx.y * R + r, lz_gload(M + r * N + js[blockIdx.y]));
}

// ---- the kernels of the verifier, written for a group of G openings of one shape and one Q (pcs_verify_device_batch); one opening
// (pcs_verify_device) is a group of one, its device copy the set. What differs by member (its claim count, where its opening, u,
// columns, encoded rows, jobs and weights lie) is read from its descriptor, never derived from a flat id, and no member's range is
// assumed to start at a workgroup. Every block of the staged copy starts at a multiple of 32 bytes (lz_gload reads 16-byte halves).
// A word of an opening only ever becomes a number; every index below comes from the shape, from the host's masked j_q or from table
// offsets the entry point validated. The descriptors (VbMember, VbGroup, CombineDesc) and the result cells are those of
// pcs_flow.hpp; a row element is an Fr, so the offsets in Row units are element offsets.
using pcs::CombineDesc;
using pcs::VbMember;
using pcs::VbGroup;
using pcs::ObClaim;
typedef pcs::ObJob<Fr> ObJob;
typedef pcs::ObMember<Fr> ObMember;

// 32 big-endian bytes of an opening -> 4 native limbs (limb w = the byte-swapped word 3 - w); blockIdx.y = the member, its elements
// grid-strided over blockIdx.x. Element i < u_el is element i & (C - 1) of u vector i >> c: kept in u and scattered into row i >> c
// of the member's rows of the matrix the NTT encodes (zeroed beforehand). The others are the Q * R column elements, query q at
// element u_el + q * q_stride. cells[3m] = the lowest byte offset, within its opening, of an element that is not below r (all four limbs
// compared). Elements stay plain words: no Montgomery conversion (ntt_batch_dev keeps the form).
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_canon(const u64* __restrict__ set, const VbMember* __restrict__ mem, VbGroup g, Fr* __restrict__ u,
                                                             Fr* __restrict__ cols, Fr* __restrict__ enc, u64* __restrict__ cells) {
    const VbMember M = mem[blockIdx.y];
    const int c = g.c;
    const size_t Q = g.Q, R = g.R, u_el = (M.n + 1) << c, total = u_el + Q * R, Cm = ((size_t)1 << c) - 1;
    const u64* proof = set + M.proof;
    Fr* mu = u + M.u;
    Fr* mcols = cols + M.cols;
    Fr* menc = enc + (M.enc_row << (c + 2));
    u64 bad = pcs::PCSV_NONE;
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * BNPCS_TPB) {
        size_t at = i;
        if (i >= u_el) { const size_t k = i - u_el, q = k / R; at = u_el + q * g.q_stride + (k - q * R); }
        const u64* p = proof + 4 * at;
        const Fr v = fr_make(__builtin_bswap64(p[3]), __builtin_bswap64(p[2]), __builtin_bswap64(p[1]), __builtin_bswap64(p[0]));
        if (fr_geq_p(v) && 32 * at < bad) bad = 32 * at;
        if (i < u_el) {
            lz_gstore(mu + i, v);
            lz_gstore(menc + ((i >> c) << (c + 2)) + (i & Cm), v);
        } else {
            lz_gstore(mcols + (i - u_el), v);
        }
    }
    if (bad != pcs::PCSV_NONE) pcs::cell_min(cells + 3 * blockIdx.y, bad);
}

// <ui, eq(z[..c])> != y, by one workgroup; the answer is thread 0's. z holds the c low coordinates of the point in Montgomery form,
// so a factor of eq(z, x) = prod_b (x_b ? z_b : 1 - z_b) is in Montgomery form and factor x plain element is the plain product. The
// factors are formed per entry: a thread keeps the one of the low eight bits of x, which its entries share.
__device__ __forceinline__ bool bnpcs_eval_differs(const Fr* __restrict__ ui, const Fr* __restrict__ z, const Fr* __restrict__ y, int c) {
    __shared__ Fr part[BNPCS_TPB];
    const size_t C = (size_t)1 << c;
    const int lob = c < 8 ? c : 8;
    Fr f = fr_one_mont();
    for (int b = 0; b < lob; b++) { const Fr zb = lz_gload(z + b); f = fr_mul(f, (threadIdx.x >> b) & 1 ? zb : fr_sub(fr_one_mont(), zb)); }
    Fr s = fr_zero();
    for (size_t x = threadIdx.x; x < C; x += BNPCS_TPB) {
        Fr gq = f;
        for (int b = 8; b < c; b++) { const Fr zb = lz_gload(z + b); gq = fr_mul(gq, (x >> b) & 1 ? zb : fr_sub(fr_one_mont(), zb)); }
        s = fr_add(s, fr_mul(lz_gload(ui + x), gq));
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = BNPCS_TPB / 2; h >= 1; h >>= 1) {
        if (threadIdx.x < h) part[threadIdx.x] = fr_add(part[threadIdx.x], part[threadIdx.x + h]);
        __syncthreads();
    }
    return threadIdx.x == 0 && !fr_eq(part[0], lz_gload(y));
}
// <u_i, eq(z_i[..c])> == y_i, one workgroup per (member, claim): block b belongs to the last member whose claim0 is <= b (a member
// without claims owns no block). cells[3m + 1] = the member's lowest failing claim.
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_eval(const VbMember* __restrict__ mem, unsigned G, int c, const Fr* __restrict__ u, const char* __restrict__ stage,
                                                            u64* __restrict__ cells) {
    unsigned lo = 0, hi = G;
    while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].claim0 <= blockIdx.x) lo = mid; else hi = mid; }
    const VbMember M = mem[lo];
    const size_t i = blockIdx.x - M.claim0;
    if (i >= M.n) return;   // (uniform over the workgroup; the grid has exactly the claims of the group)
    if (bnpcs_eval_differs(u + M.u + ((i + 1) << c), reinterpret_cast<const Fr*>(stage + M.z_at) + i * (size_t)c, reinterpret_cast<const Fr*>(stage + M.y_at) + i, c))
        pcs::cell_min(cells + 3 * lo + 1, (u64)i);
}

// One thread per (member m, query q), id = m Q + q: the leaf hash of its R column elements (contiguous: 4 words between them) -> leaves[id]
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_leaf(const VbMember* __restrict__ mem, VbGroup g, const Fr* __restrict__ cols, u64* __restrict__ leaves) {
    const size_t id = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (id >= g.G * g.Q) return;
    const size_t m = id / g.Q, q = id - m * g.Q;
    u64 a[25];
    bnpcs_leaf_absorb(reinterpret_cast<const u64*>(cols + mem[m].cols + q * g.R), 4, g.R, a);
    u64* out = leaves + 4 * id;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}

// Column inner products of every member: s[global job][q] = sum_{r < nrows} w[woff + r] * col_q[row0 + r], canonical. Job 0 of a
// member is the proximity combination (rho^r over the whole column), job 1 + i claim i's (eq(z_i[c..]) over the rows of its table).
// The weight limbs go through readfirstlane and so must be the same for every lane of a wavefront. A flat id Q job + q would let a
// wavefront straddle two jobs whenever Q is no multiple of 64, so the job is fixed per workgroup instead: a one-dimensional grid of
// bq * jobs_total workgroups, bq = the workgroups Q threads take (no y extent: the jobs of a group can pass 65535); workgroup b
// works on global job b / bq, queries (b % bq) TPB .. . The member is the last one whose job0 is <= the job. A column element that
// passed k_bnpcsvb_canon is below r and the weight is a residue, which is bnpcs_dot_chunked's bound. (An element that did not pass
// only makes this sum meaningless, and cells[3m] decides ahead of whatever reads it.)
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_dots(const VbMember* __restrict__ mem, VbGroup g, unsigned bq, const Fr* __restrict__ cols,
                                                            const char* __restrict__ stage, Fr* __restrict__ s) {
    const size_t gjob = blockIdx.x / bq;
    const size_t q = (size_t)(blockIdx.x % bq) * BNPCS_TPB + threadIdx.x;
    if (q >= g.Q) return;
    unsigned lo = 0, hi = (unsigned)g.G;
    while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].job0 <= gjob) lo = mid; else hi = mid; }
    const VbMember M = mem[lo];
    const CombineDesc job = reinterpret_cast<const CombineDesc*>(stage + M.jobs_at)[gjob - M.job0];
    lz_gstore(s + gjob * g.Q + q, bnpcs_dot_chunked(cols + M.cols + q * g.R + job.row0, 0, reinterpret_cast<const Fr*>(stage + M.w_at) + job.woff, job.nrows));
}

// One thread per (member m, query q), id = m Q + q, once the host has every member's column indices (js[id]): the path from the leaf
// hash over the c+2 siblings (32 raw bytes each behind the query's column elements) against the member's root, then s[job 0][q]
// against Enc(u_0)[j_q], then s[job 1 + i][q] against Enc(u_i)[j_q]. cells[3m + 2] = the member's lowest q (n_m + 2) + kind that
// failed: kind 0 the path, 1 proximity, 2 + i claim i.
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_query(const u64* __restrict__ set, const VbMember* __restrict__ mem, VbGroup g, const u64* __restrict__ leaves,
                                                             const Fr* __restrict__ s, const Fr* __restrict__ enc, const u64* __restrict__ js,
                                                             const char* __restrict__ stage, u64* __restrict__ cells) {
    const size_t id = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (id >= g.G * g.Q) return;
    const size_t m = id / g.Q, q = id - m * g.Q;
    const VbMember M = mem[m];
    const int depth = g.depth;
    const size_t N = (size_t)1 << depth, j = js[id], n = M.n, u_el = (n + 1) << g.c;
    const u64* sib = set + M.proof + 4 * (u_el + q * g.q_stride + g.R);
    const u64* root = reinterpret_cast<const u64*>(stage + M.root_at);
    u64 h[4] = {leaves[4 * id], leaves[4 * id + 1], leaves[4 * id + 2], leaves[4 * id + 3]};
    pcs::merkle_climb(h, sib, j, depth);
    u64* cell = cells + 3 * m + 2;
    const size_t key = q * (n + 2);
    if (h[0] != root[0] || h[1] != root[1] || h[2] != root[2] || h[3] != root[3]) { pcs::cell_min(cell, key); return; }
    const Fr* sq = s + M.job0 * g.Q + q;
    const Fr* menc = enc + (M.enc_row << depth) + j;
    for (size_t i = 0; i <= n; i++)
        if (!fr_eq(lz_gload(sq + i * g.Q), lz_gload(menc + i * N))) { pcs::cell_min(cell, key + 1 + i); return; }
}

// ---- the kernels of the prover's side of an opening, written for a group of items (pcs_open_device_batch); the row combinations of
// one opening (pcs_combine_device) are a job table of their own. What differs by item lies in three flat tables of the staged copy:
// a job a row combination (the proximity combination and one a claim, every member's behind the other), a claim an evaluation
// check, a member where its matrix, its u vectors and its opening image lie (ObJob, ObClaim, ObMember of pcs_flow.hpp; the low
// coordinates in Montgomery form). Every block of the staged copy starts at a multiple of 32 bytes (lz_gload reads 16-byte halves).
// Every grid is one-dimensional.

// Row combinations: u[u_at + j] = sum_{r < nrows} w[r] * src[r][j] for the job of the workgroup, a thread owns column j. Workgroup b
// serves job b / cb alone, columns (b % cb) BNPCS_TPB .. - the weight limbs go through readfirstlane, so every lane of a wavefront
// must be on one job
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_combine(int c, unsigned cb, const ObJob* __restrict__ jobs, const char* __restrict__ stage, Fr* __restrict__ u) {
    const size_t C = (size_t)1 << c;
    const unsigned jq = blockIdx.x / cb;
    const size_t j = (size_t)(blockIdx.x - jq * cb) * BNPCS_TPB + threadIdx.x;
    if (j >= C) return;
    const ObJob job = jobs[jq];
    lz_gstore(u + job.u_at + j, bnpcs_dot_chunked(job.src + j, c, reinterpret_cast<const Fr*>(stage + job.w_at), job.nrows));
}
// One workgroup per (member, claim): <u_i, eq(z_i[..c])> == y_i; cells[member] = its lowest failing claim
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_eval(const ObClaim* __restrict__ claims, int c, const Fr* __restrict__ u, const char* __restrict__ stage,
                                                            u64* __restrict__ cells) {
    const ObClaim cl = claims[blockIdx.x];
    if (bnpcs_eval_differs(u + cl.u_at, reinterpret_cast<const Fr*>(stage + cl.z_at), reinterpret_cast<const Fr*>(stage + cl.y_at), c)) pcs::cell_min(cells + cl.member, cl.claim);
}
// Word i of the group's u vectors into its member's image, an element as 32 bytes big-endian: word w of the image's element is the
// byte-swapped limb 3 - w. The member is the last one whose u offset is <= i (offsets are multiples of 4: an element never straddles)
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_emit(const ObMember* __restrict__ mem, unsigned G, size_t total, const u64* __restrict__ u, u64* __restrict__ img) {
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * BNPCS_TPB) {
        unsigned lo = 0, hi = G;
        while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].u <= i) lo = mid; else hi = mid; }
        img[mem[lo].img + (i - mem[lo].u)] = __builtin_bswap64(u[i ^ 3]);
    }
}
// One thread per (member m, query q, row r), id = (m Q + q) R + r: M_m[r][j_q] big-endian at its place in the member's image.
// js[m Q + q] = j_q (masked by the host); js[G Q + m] != 0: the member takes part (it was not refused)
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_gather(const ObMember* __restrict__ mem, size_t G, size_t Q, size_t R, size_t N, size_t q_words,
                                                              const u64* __restrict__ js, u64* __restrict__ img) {
    const size_t id = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (id >= G * Q * R) return;
    const size_t m = id / (Q * R), k = id - m * Q * R, q = k / R, r = k - q * R;
    if (!js[G * Q + m]) return;
    const ObMember M = mem[m];
    const Fr v = lz_gload(M.M + r * N + js[m * Q + q]);
    u64* out = img + M.img + M.u_words + q * q_words + 4 * r;
    out[0] = __builtin_bswap64(v.l[3]); out[1] = __builtin_bswap64(v.l[2]); out[2] = __builtin_bswap64(v.l[1]); out[3] = __builtin_bswap64(v.l[0]);
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
    Drain drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
    hipc(hipMemsetAsync(d_flag, 0, 16, st), "memset");
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t len = (size_t)1 << sh.nvars[t];
        if (words) hipc(hipMemcpyAsync(d_words + sh.off[t] * C, tables[t], len * 8, hipMemcpyHostToDevice, st), "upload tables");
        else hipc(hipMemcpyAsync(d_rows + sh.off[t] * C, tables[t], len * sizeof(Fr), hipMemcpyHostToDevice, st), "upload tables");
    }
    ctx->prof_begin(c_stage, (double)R * C * (words ? 40 : 0) + (double)R * C * 32 + (double)R * N * 32);
    if (words) k_bnpcs_lift<<<(unsigned)std::min<size_t>(bnpcs_blocks(R * C), 4096), BNPCS_TPB, 0, st>>>(d_words, d_rows, R * C);
    k_bnpcsb_stage<<<(unsigned)std::min<size_t>(bnpcs_blocks(R * N), 4096), BNPCS_TPB, 0, st>>>(d_rows, d_M, R, sh.c, d_flag);
    ctx->prof_end();
    ctx->prof_begin(c_ntt, (double)R * N * 32 * 4);
    k_bn_powers<<<bnpcs_blocks(N), 256, 0, st>>>(W, fr_root_of_unity(log2n), N);
    ntt_batch_dev(st, d_M, tmp, W, log2n, R, nullptr);
    ctx->prof_end();
    ctx->prof_begin(c_leaf, (double)R * N * 32);
    k_bnpcsb_leaf_hash<<<bnpcs_blocks(N), BNPCS_TPB, 0, st>>>(d_M, 1, log2n, R, d_tree, 8 * N);
    ctx->prof_end();
    ctx->prof_begin(c_tree, (double)N * 96);
    pcs::merkle_levels_device(st, d_tree, N);
    ctx->prof_end();
    cm->tree.resize(32 * (2 * N - 1));
    unsigned flag = 0;
    hipc(hipMemcpyAsync(cm->tree.data(), d_tree, cm->tree.size(), hipMemcpyDeviceToHost, st), "download tree");
    hipc(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st), "download flag");
    hipc(hipStreamSynchronize(st), (me + ": sync").c_str());
    hipc(hipGetLastError(), (me + ": launch").c_str());
    ctx->prof_collect();
    if (flag) throw Error(me + ": a table holds an element that is not below r");
    return cm.release();
}

// ---- a commitment to witness words that lie in HBM already (pcs_commit_words_enqueue: the encryption pipeline): k_bnpcs_lift and
// k_bnpcsb_stage in one pass over the source tables, pcs::k_pcs_stage_tables over Fr. A thread moves a unit of two words (one 16-byte
// load); a row has U = C / 2 units; 2^lanes_log2 = min(BNPCS_TPB, U) threads work on a row, so a workgroup holds
// BNPCS_TPB >> lanes_log2 rows at a time, and a row of more than BNPCS_TPB units is walked in U >> lanes_log2 steps of which every
// workgroup of the row takes `split`-th part. The table of a row is looked up once a row from the descriptor in the kernel
// arguments. Per unit: the word test, the signed lift of both words, the two canonical elements (64 bytes) into the raw row and
// into the row of M, and twelve 16-byte zero stores into the 3C elements of padding behind them, unit-strided, so that the lanes
// of a wavefront write adjacent 16 bytes there and adjacent elements elsewhere. 16 bytes in and 320 out a unit (the two-kernel path: 80 in, 320 out); no LDS.
struct BnStageWords {
    const u64* src[pcs::MAX_TABLES];
    unsigned off[pcs::MAX_TABLES + 1];   // first row of table t; off[nt] = R
    unsigned nt;
};
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcs_stage_words(const BnStageWords T, Fr* __restrict__ rows, Fr* __restrict__ M, int c, int lanes_log2, int split_log2,
                                                                 unsigned* __restrict__ flag) {
    const int u_log2 = c - 1;                                  // log2 of the units in a row
    const int steps_log2 = u_log2 - lanes_log2 - split_log2;   // steps a workgroup walks along its row(s)
    const size_t R = T.off[T.nt];
    const unsigned lane = threadIdx.x & ((1u << lanes_log2) - 1), sub = threadIdx.x >> lanes_log2, rpb = BNPCS_TPB >> lanes_log2;
    const size_t groups = (R + rpb - 1) / rpb, items = groups << split_log2;
    const size_t U = (size_t)1 << u_log2;
    const lz_u32x4 zero = {0, 0, 0, 0};
    bool bad = false;
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const size_t r = (item >> split_log2) * rpb + sub, part = item & (((size_t)1 << split_log2) - 1);
        if (r >= R) continue;
        unsigned t = 0;
        while (t + 1 < T.nt && T.off[t + 1] <= r) t++;
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(T.src[t] + ((r - T.off[t]) << c));
        Fr* drow = rows + (r << c);
        Fr* mrow = M + (r << (c + 2));
        __attribute__((address_space(1))) lz_u32x4* pad = (__attribute__((address_space(1))) lz_u32x4*)(mrow + 2 * U);   // 3C elements = 12 U units of 16 bytes
        for (size_t s = 0; s < ((size_t)1 << steps_log2); s++) {
            const size_t u = (((part << steps_log2) + s) << lanes_log2) + lane;
            const ulonglong2 v = src[u];
            bad |= v.x >= GL_P || v.y >= GL_P;
            const Fr a = fr_lift_signed_canon(v.x), b = fr_lift_signed_canon(v.y);
            lz_gstore(drow + 2 * u, a);
            lz_gstore(drow + 2 * u + 1, b);
            lz_gstore(mrow + 2 * u, a);
            lz_gstore(mrow + 2 * u + 1, b);
#pragma unroll
            for (int q = 0; q < 12; q++) pad[(size_t)q * U + u] = zero;
        }
    }
    if (bad) atomicOr(flag, 1u);
}

void pcs_commit_words_enqueue(hipStream_t st, const pcs::Shape& sh, const u64* const* d_tables, Fr* d_rows, Fr* d_M, Fr* tmp, Fr* W, u64* d_tree, unsigned* d_flag) {
    const size_t N = sh.N(), R = sh.R, nt = sh.nvars.size();
    const int log2n = sh.depth();
    bool fits = nt <= (size_t)pcs::MAX_TABLES && R <= 65535 && sh.c >= 1 && ((uintptr_t)d_rows & 15) == 0 && ((uintptr_t)d_M & 15) == 0;
    BnStageWords T;
    for (size_t t = 0; fits && t < nt; t++) {
        T.src[t] = d_tables[t];
        T.off[t] = (unsigned)sh.off[t];
        fits = ((uintptr_t)d_tables[t] & 15) == 0;
    }
    if (!fits) throw Error("pcs_commit_words_enqueue: a shape or an alignment the staging kernel does not take");
    T.off[nt] = (unsigned)R;
    T.nt = (unsigned)nt;
    const int u_log2 = sh.c - 1, lanes_log2 = std::min(u_log2, 8);
    static_assert(BNPCS_TPB == 256, "2^8 threads a workgroup");
    const size_t groups = (R + (BNPCS_TPB >> lanes_log2) - 1) / (BNPCS_TPB >> lanes_log2);
    int split_log2 = 0;   // the workgroups of a row: enough of them for about 2048 in all
    while (split_log2 < u_log2 - lanes_log2 && (groups << split_log2) < 2048) split_log2++;
    const unsigned grid = (unsigned)std::min<size_t>(groups << split_log2, (size_t)1 << 20);
    hipc(hipMemsetAsync(d_flag, 0, 4, st), "memset");
    k_bnpcs_stage_words<<<grid, BNPCS_TPB, 0, st>>>(T, d_rows, d_M, sh.c, lanes_log2, split_log2, d_flag);
    k_bn_powers<<<bnpcs_blocks(N), 256, 0, st>>>(W, fr_root_of_unity(log2n), N);
    ntt_batch_dev(st, d_M, tmp, W, log2n, R, nullptr);
    k_bnpcsb_leaf_hash<<<bnpcs_blocks(N), BNPCS_TPB, 0, st>>>(d_M, 1, log2n, R, d_tree, 8 * N);
    pcs::merkle_levels_device(st, d_tree, N);
}

// ---- the BN254 policy of the flows of pcs_flow.hpp. A row element, an element of u and a weight are an Fr each: a u vector is encoded
// as one row. Weights and low coordinates go into the staged copy in Montgomery form.
struct BnPcs {
    typedef Fr Row;
    typedef Fr W;
    typedef PcsClaim Claim;
    typedef PcsJob Job;
    typedef bn::VerifyItem VerifyItem;
    typedef PcsOpenItem OpenItem;
    static constexpr size_t U_ROWS = 1, ALIGN = 32, TPB = BNPCS_TPB;
    static constexpr pcs::Field FIELD = pcs::BN254;
    // The leaf sponge (serial: 4R + 1 words a thread, Q threads a member) is the longest of the index-free kernels and goes last among
    // them, so the two verdicts that need no index and the inner products never wait behind it; the host's own hash of the u_i covers it.
    static constexpr bool LEAF_AFTER_DOTS = true;
    static constexpr const char *CLS_VERIFY = "pcs_bn254_verify", *CLS_VERIFY_BATCH = "pcs_bn254_verify_batch", *CLS_OPEN_BATCH = "pcs_bn254_open_batch",
                                *CLS_COMMIT_BATCH = "pcs_bn254_commit_batch", *CLS_COMBINE = "pcs_bn254_combine";
    static constexpr const char *VERIFY_NAME = "hg_pcs_verify_device_bn254", *OPEN_NAME = "hg_pcs_open_bn254", *TIMES_TAG = "bn254 ",
                                *NOT_BELOW = "a table holds an element that is not below r";
    static size_t opening_bytes(const pcs::Shape& sh, size_t n, size_t Q) { return pcs_opening_bytes(sh, n, Q); }
    // the folded opening (verify_folded_flow)
    static constexpr const char* VERIFY_FOLDED_NAME = "hg_pcs_verify_folded_device_bn254";
    static size_t folded_header_bytes(const pcs::Shape& sh) { return pcs_folded_header_bytes(sh); }
    static size_t folded_opening_bytes(const pcs::Shape& sh, size_t Q) { return pcs_folded_opening_bytes(sh, Q); }
    static PcsFoldedHeader folded_header(const pcs::Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof) {
        return pcs_folded_header(sh, root, claims, Q, proof);
    }
    // the transcript
    static FsTranscript start_transcript(const pcs::Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q) { return pcs_start_transcript(sh, root, claims, Q); }
    static std::vector<Fr> rho_powers(FsTranscript& tr, size_t R) { return pcs_rho_powers(pcs_squeeze(tr), R); }
    static std::vector<Fr> eq_table(const Fr* pt, size_t n) { return pcs_eq_table(pt, n); }
    static void store_low(Fr* dst, const Fr* pt, int c) { for (int b = 0; b < c; b++) dst[b] = fr_to_mont(pt[b]); }
    static void absorb_opening(FsTranscript& tr, const uint8_t* proof, size_t n_u) {   // the u_i as the opening holds them: 32 bytes big-endian
        std::vector<Fr> u(n_u);
        for (size_t i = 0; i < n_u; i++) u[i] = pcs_read_be32(proof + 32 * i);
        pcs_absorb(tr, u.data(), n_u);
    }
    static void absorb_u(FsTranscript& tr, const u64* words, size_t n_words) { pcs_absorb(tr, reinterpret_cast<const Fr*>(words), n_words / 4); }
    static std::vector<size_t> squeeze_indices(FsTranscript& tr, size_t N, size_t Q) { return pcs_squeeze_indices(tr, N, Q); }
    // limits and sizes
    static bool ntt_needs_tmp(int) { return true; }   // ntt_batch_dev goes through a temporary on either path
    // k_bnpcsvb_dots: bq workgroups a job (a member's jobs are its rows) in one x extent, and a launch takes fewer than 2^32 threads.
    // One member is at most 4097 jobs of 256 workgroups, far inside it.
    static size_t dots_max_rows(size_t Q) { return (((size_t)1 << 32) / BNPCS_TPB - 1) / bnpcs_blocks(Q); }
    // the committer's temporary is one slice's: at least one member, else what fits in here (the slices follow each other on the
    // stream, so the temporary does not grow with the group)
    static constexpr size_t COMMIT_BUDGET = VB_PCS_COMMIT_BUDGET_BN254, NTT_TMP = (size_t)256 << 20;
    static size_t commit_member_bytes(size_t R, size_t C, size_t N) { return sizeof(Fr) * (R * C + R * N); }   // its rows and encoded rows in the slab
    // a freed group's allocation, if the context holds one that fits (pcs::SlabSpares); the slab goes back there with its last handle
    static void slab_spare(hg_ctx* ctx, pcs::Slab& slab, size_t bytes) {
        slab.home = batch_bufs(ctx)->slabs;
        slab.p = slab.home->take(bytes, &slab.bytes);
    }

    // the steps of the committer; words != null: witness words, lifted into the raw rows first
    static void stage(hg_ctx* ctx, int cls, hipStream_t st, size_t G, size_t R, int c, const u64* words, Fr* rows, Fr* M, unsigned* flags) {
        const size_t C = (size_t)1 << c, N = (size_t)4 << c;
        ctx->prof_begin(cls, (double)G * R * C * (words ? 40 : 0) + (double)G * R * (C + N) * 32);
        if (words) k_bnpcs_lift<<<(unsigned)std::min<size_t>(bnpcs_blocks(G * R * C), 4096), BNPCS_TPB, 0, st>>>(words, rows, G * R * C);
        k_bnpcsb_stage<<<dim3((unsigned)std::min<size_t>(bnpcs_blocks(R * N), (4096 + G - 1) / G), (unsigned)G), BNPCS_TPB, 0, st>>>(rows, M, R, c, flags);   // about 4096 workgroups in all; G in the grid's y: cut_groups keeps it at VB_MAX_GROUP = 64 or below
        ctx->prof_end();
    }
    // the powers of the root and the encoding of `rows` rows, rows_a_call at a time through one temporary
    static void ntt(hg_ctx* ctx, int cls, hipStream_t st, Fr* a, Fr* tmp, Fr* W, int depth, size_t rows, size_t rows_a_call) {
        const size_t N = (size_t)1 << depth;
        ctx->prof_begin(cls, (double)rows * N * 32 * 4);
        k_bn_powers<<<bnpcs_blocks(N), 256, 0, st>>>(W, fr_root_of_unity(depth), N);
        for (size_t r0 = 0; r0 < rows; r0 += rows_a_call) ntt_batch_dev(st, a + r0 * N, tmp, W, depth, std::min(rows_a_call, rows - r0), nullptr);
        ctx->prof_end();
    }
    static void leaf_hash(hg_ctx* ctx, int cls, hipStream_t st, const Fr* M, size_t G, int depth, size_t R, u64* trees, size_t tree_words) {
        ctx->prof_begin(cls, (double)(G << depth) * R * 32);
        k_bnpcsb_leaf_hash<<<bnpcs_blocks(G << depth), BNPCS_TPB, 0, st>>>(M, G, depth, R, trees, tree_words);
        ctx->prof_end();
    }
    // the steps of the verifiers
    static void canon(hg_ctx* ctx, int cls, hipStream_t st, unsigned cap, const u64* set, const VbMember* mem, const VbGroup& g, size_t u_total, size_t unit_max, Fr* u, Fr* cols,
                      Fr* enc, u64* cells) {
        ctx->prof_begin(cls, (double)(u_total + g.G * g.Q * g.R) * 64 + (double)u_total * 32);
        k_bnpcsvb_canon<<<dim3((unsigned)std::min<size_t>(bnpcs_blocks(unit_max), cap), (unsigned)g.G), BNPCS_TPB, 0, st>>>(set, mem, g, u, cols, enc, cells);
        ctx->prof_end();
    }
    static void eval(hg_ctx* ctx, int cls, hipStream_t st, const VbMember* mem, const VbGroup& g, size_t claims, const Fr* u, const char* stage, u64* cells) {
        ctx->prof_begin(cls, (double)(claims << g.c) * 32);
        k_bnpcsvb_eval<<<(unsigned)claims, BNPCS_TPB, 0, st>>>(mem, (unsigned)g.G, g.c, u, stage, cells);
        ctx->prof_end();
    }
    static void leaf(hg_ctx* ctx, int cls, hipStream_t st, const VbMember* mem, const VbGroup& g, const Fr* cols, u64* leaves) {
        ctx->prof_begin(cls, (double)g.G * g.Q * g.R * 32);
        k_bnpcsvb_leaf<<<bnpcs_blocks(g.G * g.Q), BNPCS_TPB, 0, st>>>(mem, g, cols, leaves);
        ctx->prof_end();
    }
    static void dots(hg_ctx* ctx, int cls, hipStream_t st, const VbMember* mem, const VbGroup& g, size_t jobs, size_t nw, const Fr* cols, const char* stage, Fr* s) {
        const size_t bq = bnpcs_blocks(g.Q);   // the workgroups of a job
        ctx->prof_begin(cls, (double)g.Q * nw * 64);
        k_bnpcsvb_dots<<<(unsigned)(bq * jobs), BNPCS_TPB, 0, st>>>(mem, g, (unsigned)bq, cols, stage, s);
        ctx->prof_end();
    }
    static void query(hg_ctx* ctx, int cls, hipStream_t st, const u64* set, const VbMember* mem, const VbGroup& g, size_t jobs, const u64* leaves, const Fr* s, const Fr* enc,
                      const u64* js, const char* stage, u64* cells) {
        ctx->prof_begin(cls, (double)g.G * g.Q * 32.0 * g.depth + (double)g.Q * jobs * 64.0);
        k_bnpcsvb_query<<<bnpcs_blocks(g.G * g.Q), BNPCS_TPB, 0, st>>>(set, mem, g, leaves, s, enc, js, stage, cells);
        ctx->prof_end();
    }
    // the steps of the openers
    static void combine(hg_ctx* ctx, int cls, hipStream_t st, int c, size_t jobs, size_t nw, size_t u_words, const ObJob* job, const char* stage, Fr* u) {
        const size_t C = (size_t)1 << c;
        const unsigned cb = bnpcs_blocks(C);
        ctx->prof_begin(cls, (double)nw * C * 32 + (double)u_words * 8);
        k_bnpcsob_combine<<<(unsigned)(jobs * cb), BNPCS_TPB, 0, st>>>(c, cb, job, stage, u);
        ctx->prof_end();
    }
    static void ob_eval(hg_ctx* ctx, int cls, hipStream_t st, const ObClaim* claim, size_t claims, int c, const Fr* u, const char* stage, u64* cells) {
        ctx->prof_begin(cls, (double)(claims << c) * 32);
        k_bnpcsob_eval<<<(unsigned)claims, BNPCS_TPB, 0, st>>>(claim, c, u, stage, cells);
        ctx->prof_end();
    }
    static void emit(hg_ctx* ctx, int cls, hipStream_t st, const ObMember* mem, size_t G, size_t u_words, const u64* u, u64* img) {
        ctx->prof_begin(cls, (double)u_words * 16);
        k_bnpcsob_emit<<<(unsigned)std::min<size_t>(bnpcs_blocks(u_words), 4096), BNPCS_TPB, 0, st>>>(mem, (unsigned)G, u_words, u, img);
        ctx->prof_end();
    }
    static void gather(hg_ctx* ctx, int cls, hipStream_t st, const ObMember* mem, size_t G, size_t Q, size_t R, size_t N, size_t q_words, size_t active, const u64* js, u64* img) {
        ctx->prof_begin(cls, (double)active * Q * R * 64);
        k_bnpcsob_gather<<<bnpcs_blocks(G * Q * R), BNPCS_TPB, 0, st>>>(mem, G, Q, R, N, q_words, js, img);
        ctx->prof_end();
    }
    static void gather_one(hipStream_t st, const Fr* M, size_t N, size_t R, size_t Q, const u64* js, Fr* cols) {
        k_bnpcs_gather<<<dim3(bnpcs_blocks(R), (unsigned)Q), BNPCS_TPB, 0, st>>>(M, N, R, js, cols);
    }
};

void pcs_combine_device(const pcs::Commitment& cm, const std::vector<PcsJob>& jobs, Fr* u) { pcs::combine_flow<BnPcs>(cm, jobs, u); }
void pcs_columns_device(const pcs::Commitment& cm, const std::vector<size_t>& js, Fr* cols) { pcs::columns_flow<BnPcs>(cm, js, cols); }
std::string pcs_verify_device(hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    return pcs::verify_flow<BnPcs>(ctx, sh, root, claims, Q, proof, len);
}
std::vector<std::string> pcs_verify_device_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<VerifyItem>& items, size_t Q) {
    return pcs::verify_batch_flow<BnPcs>(who, ctx, sh, items, Q);
}
std::vector<pcs::Commitment*> pcs_commit_device_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tables, size_t n, bool words) {
    return pcs::commit_batch_flow<BnPcs>(who, ctx, sh, tables, n, words);
}
std::vector<pcs::Opened> pcs_open_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q) {
    return pcs::open_batch_flow<BnPcs>(who, single, ctx, items, Q);
}
std::string pcs_verify_folded_device(hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    return pcs::verify_folded_flow<BnPcs>(ctx, sh, root, claims, Q, proof, len);
}

// ---- the reduction sum-check of a folded opening (pcs_bn254.hpp PcsFoldSource; hg.h "Folded openings over BN254"): the prover's
// table-sized work, the structure of FoldDev in pcs.hip over Fr. The raw rows of a handle are its tables, contiguous in table order:
// table t starts at element s_t = off_t C, plain canonical words that are never written. g lies in an Fr array parallel to them, in
// Montgomery form. Round 0 reads both as they are; the kernel of round j >= 1 folds every live table and its g by r_{j-1} into buffers of
// half the size and forms round j's sums from the folded entries while it holds them. After j folds table t lies at entry s_t >> j of
// its buffer (two live tables never overlap there); the two buffer pairs alternate. A fold x + r d is lz_fold with the launch's
// fold_consts(r) (r in Montgomery form): the constants are r 2^(32 i) as plain integers, so a plain table stays plain and g stays in
// Montgomery form; a Montgomery reduction of a product g T is the plain value. A table of two entries is folded to its two scalars, which go
// to the host with the round's sums: ONE SYNCHRONISATION A ROUND (the challenge of round j is hashed from round j's sums). Every round
// runs on the device.
// Numbers: the buffers hold loose residues in [0, 2p); what reaches the host - the three sums, the retired scalars (the first of which
// is Y_t) - is canonical (lz_canon), so the device's bytes are the host's. A thread keeps the three sums as unreduced column
// accumulators and restarts them every BNFOLD_TRIPS units: lz_reduce takes a value below 2^12 p^2. The largest product of a unit is
// the c2 term, two lz_sub results in (0, 4p): below 16 p^2 (g T of loose residues is below 4 p^2), so an interval of up to 256 units is
// inside the bound. 64 is chosen: a quarter of that, the reductions are already 1/64 of the multiply-adds, and a test crosses it twice
// with one workgroup a table at 2^17 entries. The g builder multiplies two canonical staged factors (below p^2 a product) and
// restarts every BNFOLD_G_TRIPS = 1024 claims, a quarter of its bound of 4096.
// Geometry: blockIdx.z = the member of a group (the single call is a group of one), blockIdx.y = a live table, its units grid-strided over
// blockIdx.x; at most HG_PCS_FOLD_BLOCKS (2048) workgroups in all, but at least one a table and member.
constexpr int BNFOLD_TPB = 256;
constexpr unsigned BNFOLD_MAX_BLOCKS = 2048;
constexpr int BNFOLD_TRIPS = 64, BNFOLD_G_TRIPS = 1024;
static_assert(BNFOLD_TRIPS <= 64 && BNFOLD_TRIPS * 16 <= 4096, "lz_reduce takes a value below 2^12 p^2; a unit adds less than 16 p^2 to a sum");
static_assert(BNFOLD_G_TRIPS <= 4096, "lz_reduce takes a value below 2^12 p^2; a claim adds less than p^2");
static unsigned bnfold_max_blocks() {   // HG_PCS_FOLD_BLOCKS (tests set it): another bound on the workgroups of a launch
    const char* e = getenv("HG_PCS_FOLD_BLOCKS");
    const long v = e && *e ? atol(e) : (long)BNFOLD_MAX_BLOCKS;
    return (unsigned)std::max(1L, std::min(65535L, v));
}
struct BnFoldClaim { u64 lo_at, hi_at; u32 lo_bits, pad; };   // its two factor tables (elements of its member's staged factors): eq(z, x) = lo[x & (2^lo_bits - 1)] hi[x >> lo_bits]
// What a shape fixes for the g kernel of every member: the tables of two entries or more (the kernel's table numbers) and the
// one-element tables, whose element goes to the scalars as it is
struct BnFoldGTables {
    u32 nt, n1;
    u32 lg[pcs::MAX_TABLES], id1[pcs::MAX_TABLES];          // v_t; the number t of a one-element table
    u64 at[pcs::MAX_TABLES], at1[pcs::MAX_TABLES];          // s_t; where a one-element table lies in the rows
};
// A member's block of the g kernel's staged copy (byte offsets, multiples of 32): claim0[nt + 1] (the claims of kernel table t are
// claim0[t] .. claim0[t+1] of its list: members differ in their claim counts, and a table may have none), its BnFoldClaim list, its
// factor tables
struct BnFoldGMember { u64 claim0_at, claims_at, fac_at, pad; };
struct BnFoldTables {
    u32 nt, pad;
    u32 lg[pcs::MAX_TABLES], id[pcs::MAX_TABLES];           // log2 of a live table's entries at the input; its number t
    u64 in[pcs::MAX_TABLES], out[pcs::MAX_TABLES];          // where it lies in the input and where it goes in the output (entries)
};
// What differs by member (blockIdx.z) of a launch: where its raw rows lie (a handle may live in any slab, and may appear twice), the
// fold constants of its challenge, and a fixed stride into the group's g, buffer pairs and scalars. A group of one - the single call -
// carries its row base and its fold constants in the kernel arguments (rows == null, fk == null): its launches need no table and no
// upload.
struct BnFoldMembers {
    const Fr* const* rows;
    const Fr* rows0;
    const FoldK* fk;
    FoldK fk0;
    u64 g_stride, in_stride, out_stride, scal_stride;   // entries from a member to the next: g, the input pair, the output pair, the scalars
};
__device__ __forceinline__ const Fr* bnfold_rows(const BnFoldMembers& M) { return M.rows ? M.rows[blockIdx.z] : M.rows0; }
// g_t[x] = sum_{i on t} beta^i eq(z_i, x), every entry written once: a thread owns entry x and walks the table's claims, each a product of
// two staged factors (Montgomery form, canonical; beta^i lies in the low one). Loose on the way out. stage: G BnFoldGMember, then the
// members' blocks. The first workgroup of a member also copies the elements of its one-element tables (canonical, as the rows hold
// them) to scal[2 t].
__global__ __launch_bounds__(BNFOLD_TPB) void k_bnpcsfold_g(const BnFoldGTables A, const BnFoldMembers M, const char* __restrict__ stage, Fr* __restrict__ g,
                                                            Fr* __restrict__ scal) {
    const unsigned t = blockIdx.y;
    if (blockIdx.x == 0 && t == 0 && threadIdx.x == 0)
        for (unsigned i = 0; i < A.n1; i++) lz_gstore(scal + (size_t)blockIdx.z * M.scal_stride + 2 * A.id1[i], lz_gload(bnfold_rows(M) + A.at1[i]));
    if (t >= A.nt) return;
    const size_t len = (size_t)1 << A.lg[t];
    const BnFoldGMember D = reinterpret_cast<const BnFoldGMember*>(stage)[blockIdx.z];
    const u32* claim0 = reinterpret_cast<const u32*>(stage + D.claim0_at);
    const BnFoldClaim* cl = reinterpret_cast<const BnFoldClaim*>(stage + D.claims_at);
    const Fr* fac = reinterpret_cast<const Fr*>(stage + D.fac_at);
    const unsigned first = claim0[t], last = claim0[t + 1];
    Fr* G = g + (size_t)blockIdx.z * M.g_stride + A.at[t];
    for (size_t x = (size_t)blockIdx.x * BNFOLD_TPB + threadIdx.x; x < len; x += (size_t)gridDim.x * BNFOLD_TPB) {
        WCol acc = wcol_zero();
        Fr sum = fr_zero();
        int trips = 0;
        for (unsigned i = first; i < last; i++) {
            const BnFoldClaim d = cl[i];
            wcol_mac(acc, lz_gload(fac + d.lo_at + (x & (((size_t)1 << d.lo_bits) - 1))), lz_gload(fac + d.hi_at + (x >> d.lo_bits)));
            if (++trips == BNFOLD_G_TRIPS) { sum = lz_add(sum, lz_reduce(acc)); acc = wcol_zero(); trips = 0; }
        }
        lz_gstore(G + x, lz_add(sum, lz_reduce(acc)));
    }
}
// the three sums of a thread (loose) -> those of its workgroup at out[3 b .. 3 b + 3), b = its number in the grid (members outermost),
// canonical if `canon`; every thread calls it
__device__ __forceinline__ void bnfold_block_sums(const Fr (&s)[3], Fr* __restrict__ out, bool canon) {
    __shared__ Fr part[3][BNFOLD_TPB];
#pragma unroll
    for (int k = 0; k < 3; k++) part[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int h = BNFOLD_TPB / 2; h >= 1; h >>= 1) {
        if (threadIdx.x < h)
            for (int k = 0; k < 3; k++) part[k][threadIdx.x] = lz_add(part[k][threadIdx.x], part[k][threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x < 3) {
        const Fr v = part[threadIdx.x][0];
        lz_gstore(out + 3 * (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) + threadIdx.x, canon ? lz_canon(v) : v);
    }
}
// the accumulators of a unit's three products, restarted every BNFOLD_TRIPS units into the loose sums s
struct BnFoldAcc {
    WCol a, b, c;
    int trips;
};
__device__ __forceinline__ void bnfold_acc_unit(BnFoldAcc& w, Fr (&s)[3], const Fr& t0, const Fr& t1, const Fr& g0, const Fr& g1) {
    wcol_mac(w.a, g0, t0);
    wcol_mac(w.b, g1, t1);
    wcol_mac(w.c, lz_sub(g1, g0), lz_sub(t1, t0));
    if (++w.trips == BNFOLD_TRIPS) {
        s[0] = lz_add(s[0], lz_reduce(w.a)); s[1] = lz_add(s[1], lz_reduce(w.b)); s[2] = lz_add(s[2], lz_reduce(w.c));
        w.a = wcol_zero(); w.b = wcol_zero(); w.c = wcol_zero();
        w.trips = 0;
    }
}
__device__ __forceinline__ void bnfold_acc_finish(BnFoldAcc& w, Fr (&s)[3]) {
    s[0] = lz_add(s[0], lz_reduce(w.a)); s[1] = lz_add(s[1], lz_reduce(w.b)); s[2] = lz_add(s[2], lz_reduce(w.c));
}
// Round 0: nothing to fold. A unit is a pair (T0, T1) of the raw rows, (g0, g1) of g:
// s(0) += g0 T0, s(1) += g1 T1, c2 += (g1 - g0) (T1 - T0)
__global__ __launch_bounds__(BNFOLD_TPB) void k_bnpcsfold_round0(const BnFoldTables A, const BnFoldMembers M, const Fr* __restrict__ g, Fr* __restrict__ partial) {
    const unsigned t = blockIdx.y;
    const size_t pairs = (size_t)1 << (A.lg[t] - 1);
    const Fr* T = bnfold_rows(M) + A.in[t];
    const Fr* G = g + (size_t)blockIdx.z * M.g_stride + A.in[t];
    BnFoldAcc w{wcol_zero(), wcol_zero(), wcol_zero(), 0};
    Fr s[3] = {fr_zero(), fr_zero(), fr_zero()};
    for (size_t u = (size_t)blockIdx.x * BNFOLD_TPB + threadIdx.x; u < pairs; u += (size_t)gridDim.x * BNFOLD_TPB)
        bnfold_acc_unit(w, s, lz_gload(T + 2 * u), lz_gload(T + 2 * u + 1), lz_gload(G + 2 * u), lz_gload(G + 2 * u + 1));
    bnfold_acc_finish(w, s);
    bnfold_block_sums(s, partial, false);
}
// Round j >= 1. A unit is four adjacent entries of T and of g: folded by the member's r_{j-1} (its fold_consts) into two of each,
// which are stored and enter the sums of round j while they are in registers. Round 1 (tin == null) reads T from the member's raw
// rows and gin is g (in_stride = g_stride), later rounds read the other buffer pair. A table of two entries is folded into its two
// scalars at scal[2 id], scal[2 id + 1] of its member (canonical) by one thread and enters no sum.
// The 64 fold constants stay in SGPRs for the whole kernel in either instantiation. GROUP: the member's set is read from the table
// at blockIdx.z, an index that is uniform over the wavefront, so the reads are scalar loads (lz_load_k's readfirstlane folds away).
// !GROUP, the single call: the set comes with the kernel arguments and there is one member, as before the kernels took a group. Two
// instantiations, not one kernel that chooses at run time: merging the two sources after a branch cost the allocator its SGPRs
// (the constants were spilled to VGPR lanes and read back in the loop).
template <bool GROUP>
__global__ __launch_bounds__(BNFOLD_TPB) void k_bnpcsfold_round(const BnFoldTables A, const BnFoldMembers M, const Fr* __restrict__ tin, const Fr* __restrict__ gin,
                                                                Fr* __restrict__ tout, Fr* __restrict__ gout, Fr* __restrict__ scal, Fr* __restrict__ partial) {
    const unsigned t = blockIdx.y, lg = A.lg[t];
    const size_t z = GROUP ? blockIdx.z : 0;
    LzK fk;
    if constexpr (GROUP) {
        fk = lz_load_k(M.fk[z].k);
    } else {
#pragma unroll
        for (int i = 0; i < 64; i++) fk.k[i] = M.fk0.k[i];
    }
    const size_t in_at = z * M.in_stride + A.in[t];
    const Fr* T = tin ? tin + in_at : (GROUP ? M.rows[z] : M.rows0) + A.in[t];
    const Fr* G = gin + in_at;
    // X[2i] + r (X[2i+1] - X[2i])
    auto fold = [&](const Fr* X, size_t i) {
        const Fr x0 = lz_gload(X + 2 * i);
        return lz_fold(x0, lz_sub(lz_gload(X + 2 * i + 1), x0), fk.k);
    };
    BnFoldAcc w{wcol_zero(), wcol_zero(), wcol_zero(), 0};
    Fr s[3] = {fr_zero(), fr_zero(), fr_zero()};
    if (lg == 1) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            Fr* sc = scal + z * M.scal_stride + 2 * A.id[t];
            lz_gstore(sc, lz_canon(fold(T, 0)));
            lz_gstore(sc + 1, lz_canon(fold(G, 0)));
        }
    } else {
        const size_t units = (size_t)1 << (lg - 2), out_at = z * M.out_stride + A.out[t];
        Fr* To = tout + out_at;
        Fr* Go = gout + out_at;
        for (size_t u = (size_t)blockIdx.x * BNFOLD_TPB + threadIdx.x; u < units; u += (size_t)gridDim.x * BNFOLD_TPB) {
            const Fr t0 = fold(T, 2 * u), t1 = fold(T, 2 * u + 1), g0 = fold(G, 2 * u), g1 = fold(G, 2 * u + 1);
            lz_gstore(To + 2 * u, t0);
            lz_gstore(To + 2 * u + 1, t1);
            lz_gstore(Go + 2 * u, g0);
            lz_gstore(Go + 2 * u + 1, g1);
            bnfold_acc_unit(w, s, t0, t1, g0, g1);
        }
    }
    bnfold_acc_finish(w, s);
    bnfold_block_sums(s, partial, false);
}
// one workgroup a member (blockIdx.x): out[3 member + k] = sum_b partial[3 (member blocks + b) + k], canonical
__global__ __launch_bounds__(BNFOLD_TPB) void k_bnpcsfold_sum(const Fr* __restrict__ partial, size_t blocks, Fr* __restrict__ out) {
    const Fr* mine = partial + 3 * blocks * blockIdx.x;
    Fr s[3] = {fr_zero(), fr_zero(), fr_zero()};
    for (size_t b = threadIdx.x; b < blocks; b += BNFOLD_TPB)
        for (int k = 0; k < 3; k++) s[k] = lz_add(s[k], lz_gload(mine + 3 * b + k));
    bnfold_block_sums(s, out, true);
}

// ---- what the single call (BnFoldDev) and the pass over a group (open_folded_batch_flow of pcs_flow.hpp) share on the host: the
// geometry a shape fixes, a member's block of the g kernel's staged copy, the launches of the g kernel and of a round
static BnFoldGTables bnfold_g_tables(const pcs::Shape& sh, size_t* max_len) {
    BnFoldGTables A;
    memset(&A, 0, sizeof(A));
    *max_len = 1;
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t v = (size_t)sh.nvars[t], at = sh.off[t] << sh.c;
        if (v == 0) { A.id1[A.n1] = (u32)t; A.at1[A.n1] = (u64)at; A.n1++; continue; }   // a scalar from the start: T_t() is the element, g_t() = sum beta^i
        A.lg[A.nt] = (u32)v;
        A.at[A.nt] = (u64)at;
        A.nt++;
        *max_len = std::max(*max_len, (size_t)1 << v);
    }
    return A;
}
static size_t bnfold_up(size_t x) { return (x + 31) & ~(size_t)31; }
// the bytes of a member's block, a multiple of 32
static size_t bnfold_gblock_bytes(const pcs::Shape& sh, const BnFoldGTables& A, const std::vector<PcsClaim>& claims) {
    size_t nc = 0, fac = 0;
    for (const PcsClaim& cl : claims) {
        const size_t v = (size_t)sh.nvars[cl.table], lo_bits = (v + 1) / 2;
        if (v == 0) continue;
        nc++;
        fac += ((size_t)1 << lo_bits) + ((size_t)1 << (v - lo_bits));
    }
    return bnfold_up((A.nt + 1) * sizeof(u32)) + bnfold_up(nc * sizeof(BnFoldClaim)) + fac * sizeof(Fr);
}
// writes the block at byte `at` (a multiple of 32) of the staged copy and its descriptor: the claims in table order, per claim the two
// factor tables, beta^i in the low one; G1[t] = g_t() of the one-element tables (Montgomery form)
static void bnfold_gblock_fill(char* stage, BnFoldGMember& d, size_t at, const pcs::Shape& sh, const BnFoldGTables& A, const std::vector<PcsClaim>& claims,
                               const std::vector<Fr>& bpow, std::vector<Fr>& G1) {
    size_t nc = 0;
    for (const PcsClaim& cl : claims) nc += sh.nvars[cl.table] != 0;
    d.claim0_at = at;
    d.claims_at = d.claim0_at + bnfold_up((A.nt + 1) * sizeof(u32));
    d.fac_at = d.claims_at + bnfold_up(nc * sizeof(BnFoldClaim));
    d.pad = 0;
    u32* claim0 = reinterpret_cast<u32*>(stage + d.claim0_at);
    BnFoldClaim* list = reinterpret_cast<BnFoldClaim*>(stage + d.claims_at);
    Fr* fac = reinterpret_cast<Fr*>(stage + d.fac_at);
    size_t k = 0, f = 0, kt = 0;   // claims and factors written; the kernel's table number
    claim0[0] = 0;
    G1.assign(sh.nvars.size(), fr_zero());
    for (size_t t = 0; t < sh.nvars.size(); t++) {
        const size_t v = (size_t)sh.nvars[t], lo_bits = (v + 1) / 2;
        for (size_t i = 0; i < claims.size(); i++) {
            if (claims[i].table != t) continue;
            if (v == 0) { G1[t] = fr_add(G1[t], bpow[i]); continue; }
            std::vector<Fr> lo = pcs_eq_table(claims[i].point.data(), lo_bits);
            const std::vector<Fr> hi = pcs_eq_table(claims[i].point.data() + lo_bits, v - lo_bits);
            for (Fr& x : lo) x = fr_mul(x, bpow[i]);
            list[k++] = BnFoldClaim{(u64)f, (u64)(f + lo.size()), (u32)lo_bits, 0};
            memcpy(fac + f, lo.data(), lo.size() * sizeof(Fr));
            memcpy(fac + f + lo.size(), hi.data(), hi.size() * sizeof(Fr));
            f += lo.size() + hi.size();
        }
        if (v != 0) claim0[++kt] = (u32)k;
    }
}
// the workgroups a table of a launch over nt tables of G members whose largest has `units` units: max_blocks bounds the launch as a
// whole, and a table of a member always gets at least one
static unsigned bnfold_blocks_of(unsigned max_blocks, size_t units, size_t nt, size_t G) {
    const size_t cap = std::max<size_t>(1, max_blocks / (nt * G));
    return (unsigned)std::max<size_t>(1, std::min(cap, (units + BNFOLD_TPB - 1) / BNFOLD_TPB));
}
// the tables live in step j and where they lie; retire: one of them is folded to its scalars; units: those of the largest; entries: in all
static BnFoldTables bnfold_tables(const pcs::Shape& sh, size_t j, bool* retire, size_t* max_units, size_t* entries) {
    BnFoldTables A;
    memset(&A, 0, sizeof(A));
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
// the arena buffers of G reductions: g (32 bytes a table entry), the two buffer pairs (a half and a quarter of that for T and for g
// each, member after member), the partials (3 a workgroup: max_blocks bounds a launch, but a table of a member has at least one), the
// sums and the scalars
struct BnFoldBufs {
    Fr *g, *t[2], *gg[2], *scal, *partial, *sums;
    size_t stride[2];   // entries a member of pair 0 and of pair 1
};
static BnFoldBufs bnfold_alloc(hg_ctx* ctx, const pcs::Shape& sh, size_t G, unsigned max_blocks) {
    const size_t W = sh.R << sh.c, m = sh.nvars.size();
    BnFoldBufs b;
    b.stride[0] = W / 2 + 1;
    b.stride[1] = W / 4 + 1;
    b.g = ctx->alloc_n<Fr>(G * W);
    for (int p = 0; p < 2; p++) {
        b.t[p] = ctx->alloc_n<Fr>(G * b.stride[p]);
        b.gg[p] = ctx->alloc_n<Fr>(G * b.stride[p]);
    }
    b.scal = ctx->alloc_n<Fr>(G * 2 * m);
    b.partial = ctx->alloc_n<Fr>(3 * ((size_t)max_blocks + pcs::MAX_TABLES * G));
    b.sums = ctx->alloc_n<Fr>(3 * G);
    return b;
}
// a member table: rows and fk null for a group of one, which sets rows0 and fk0
static BnFoldMembers bnfold_members(const pcs::Shape& sh, const Fr* const* rows, const FoldK* fk) {
    BnFoldMembers M;
    memset(&M, 0, sizeof(M));
    M.rows = rows;
    M.fk = fk;
    M.g_stride = sh.R << sh.c;
    M.scal_stride = 2 * sh.nvars.size();
    return M;
}
static void bnfold_g_launch(hipStream_t st, unsigned max_blocks, const BnFoldGTables& A, size_t max_len, size_t G, const BnFoldMembers& M, const char* d_stage,
                            const BnFoldBufs& b) {
    const size_t nt = std::max<size_t>(A.nt, 1);   // (a shape of one-element tables alone: the first workgroup of a member copies them)
    k_bnpcsfold_g<<<dim3(bnfold_blocks_of(max_blocks, max_len, nt, G), (unsigned)nt, (unsigned)G), BNFOLD_TPB, 0, st>>>(A, M, d_stage, b.g, b.scal);
}
// the launch of step j over G members (A.nt >= 1) and, `sums`, of the workgroup a member that adds its partials
static void bnfold_launch(hipStream_t st, unsigned max_blocks, const pcs::Shape& sh, size_t j, const BnFoldTables& A, size_t max_units, size_t G, BnFoldMembers M,
                          const BnFoldBufs& b, bool sums) {
    const size_t W = sh.R << sh.c;
    const dim3 grid(bnfold_blocks_of(max_blocks, max_units, A.nt, G), A.nt, (unsigned)G);
    M.in_stride = j <= 1 ? W : b.stride[j & 1];
    M.out_stride = j == 0 ? 0 : b.stride[(j - 1) & 1];
    const Fr *tin = j == 1 ? nullptr : b.t[j & 1], *gin = j == 1 ? b.g : b.gg[j & 1];
    if (j == 0) k_bnpcsfold_round0<<<grid, BNFOLD_TPB, 0, st>>>(A, M, b.g, b.partial);
    else if (M.fk) k_bnpcsfold_round<true><<<grid, BNFOLD_TPB, 0, st>>>(A, M, tin, gin, b.t[(j - 1) & 1], b.gg[(j - 1) & 1], b.scal, b.partial);
    else k_bnpcsfold_round<false><<<grid, BNFOLD_TPB, 0, st>>>(A, M, tin, gin, b.t[(j - 1) & 1], b.gg[(j - 1) & 1], b.scal, b.partial);
    if (sums) k_bnpcsfold_sum<<<(unsigned)G, BNFOLD_TPB, 0, st>>>(b.partial, (size_t)grid.x * grid.y, b.sums);
}
// the bytes step j moves over `entries` table entries: round 0 reads 32 + 32 an entry, a later round reads them and writes 32 + 32 for
// every two
static double bnfold_step_bytes(size_t j, size_t entries) { return (double)entries * (j == 0 ? 64 : 96); }

// The device form of PcsFoldSource: a group of one through the kernels above. Scratch from the context's arena (reset here; the
// handle's matrices are its own).
struct BnFoldDev : PcsFoldSource {
    const pcs::Commitment& cm;
    hg_ctx* ctx;
    hipStream_t st;
    int cls;
    size_t n_claims;
    unsigned max_blocks;
    std::string me;
    BnFoldBufs buf;
    BnFoldMembers mem;
    bool one_element;       // the shape has one-element tables: their elements come back with step 0
    std::vector<Fr> h_scal, G1;
    Fr h_sums[3];

    BnFoldDev(const char* who, const pcs::Commitment& cm_, const std::vector<PcsClaim>& claims, const std::vector<Fr>& bpow)
        : cm(cm_), ctx(cm_.ctx), n_claims(claims.size()), me(who) {
        const pcs::Shape& sh = cm.sh;
        const size_t m = sh.nvars.size(), W = sh.R << sh.c;
        hipc(hipSetDevice(ctx->device), "hipSetDevice");
        ctx->arena_reset();
        st = ctx->stream;
        cls = ctx->prof_class("pcs_fold_bn254", false);
        ctx->prof_stream = st;
        max_blocks = bnfold_max_blocks();
        T.assign(m, fr_zero());
        G.assign(m, fr_zero());
        h_scal.assign(2 * m, fr_zero());
        size_t max_len;
        const BnFoldGTables A = bnfold_g_tables(sh, &max_len);
        one_element = A.n1 != 0;
        mem = bnfold_members(sh, nullptr, nullptr);
        mem.rows0 = reinterpret_cast<const Fr*>(cm.d_rows);
        std::vector<char> stage(sizeof(BnFoldGMember) + bnfold_gblock_bytes(sh, A, claims) + 32);
        static_assert(sizeof(BnFoldGMember) % 32 == 0, "a member's block starts at a multiple of 32");
        BnFoldGMember d;
        bnfold_gblock_fill(stage.data(), d, sizeof(BnFoldGMember), sh, A, claims, bpow, G1);
        memcpy(stage.data(), &d, sizeof(d));
        char* d_stage;
        try {
            buf = bnfold_alloc(ctx, sh, 1, max_blocks);
            d_stage = ctx->alloc_n<char>(stage.size());
        } catch (const std::exception& e) {
            throw Error(std::string("the context's arena cannot hold the reduction (") + e.what() + ")");
        }
        hipc(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload factor tables");
        ctx->prof_begin(cls, (double)W * 32 + (double)stage.size());
        bnfold_g_launch(st, max_blocks, A, max_len, 1, mem, d_stage, buf);
        ctx->prof_end();
        hipc(hipStreamSynchronize(st), (me + ": sync").c_str());   // (the staged copy is a local)
        hipc(hipGetLastError(), (me + ": launch").c_str());
    }
    void step(size_t j, const Fr& r, Fr s[3]) override {
        const pcs::Shape& sh = cm.sh;
        const size_t m = sh.nvars.size(), V = pcs::fold_rounds(sh);
        bool retire;
        size_t max_units, entries;
        const BnFoldTables A = bnfold_tables(sh, j, &retire, &max_units, &entries);
        retire |= j == 0 && one_element;
        if (s) s[0] = s[1] = s[2] = fr_zero();
        if (!A.nt && !retire) return;
        ctx->prof_stream = st;
        if (A.nt) {
            if (j > 0) fold_consts(fr_to_mont(r), &mem.fk0);
            ctx->prof_begin(cls, bnfold_step_bytes(j, entries));
            bnfold_launch(st, max_blocks, sh, j, A, max_units, 1, mem, buf, s != nullptr);
            ctx->prof_end();
            if (s) hipc(hipMemcpyAsync(h_sums, buf.sums, sizeof(h_sums), hipMemcpyDeviceToHost, st), "download the round's sums");
        }
        if (retire) hipc(hipMemcpyAsync(h_scal.data(), buf.scal, 2 * m * sizeof(Fr), hipMemcpyDeviceToHost, st), "download the retired tables' scalars");
        hipc(hipStreamSynchronize(st), (me + ": sync").c_str());
        hipc(hipGetLastError(), (me + ": launch").c_str());
        ctx->prof_collect();
        if (s && A.nt) memcpy(s, h_sums, sizeof(h_sums));
        for (size_t t = 0; t < m; t++) {
            if (j == 0 && sh.nvars[t] == 0) { T[t] = h_scal[2 * t]; G[t] = G1[t]; }
            if (j > 0 && (size_t)sh.nvars[t] == j) { T[t] = h_scal[2 * t]; G[t] = h_scal[2 * t + 1]; }
        }
        if (j == V && hg_debug("plan"))   // (read at every call: the tests switch it per case)
            fprintf(stderr, "[hg plan] bnpcsfold V=%zu dev_rounds=%zu host_rounds=0 tables=%zu claims=%zu\n", V, V, m, n_claims);
    }
};
std::unique_ptr<PcsFoldSource> pcs_fold_source_device(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& claims, const std::vector<Fr>& bpow) {
    return std::unique_ptr<PcsFoldSource>(new BnFoldDev(who, cm, claims, bpow));
}

// ---- the batch forms of the folded openings. The verifier is verify_batch_flow with the member blocks prepared from the folded
// headers; the opener is open_folded_batch_flow over the reduction's kernels and helpers above. A challenge goes up as its 64 fold
// constants (G x 256 bytes a round), which the round kernel reads at blockIdx.z.
struct BnFoldPcs : BnPcs {
    typedef PcsFoldProver FoldProver;
    typedef BnFoldGTables FoldGTables;
    typedef BnFoldGMember FoldGMember;
    typedef BnFoldTables FoldTables;
    typedef BnFoldMembers FoldMembers;
    typedef BnFoldBufs FoldBufs;
    typedef FoldK FoldChal;
    static constexpr const char *CLS_FOLD_BATCH = "pcs_fold_batch_bn254", *PLAN_FOLD_BATCH = "bnpcsfoldb";
    static unsigned fold_max_blocks() { return bnfold_max_blocks(); }
    static FoldGTables fold_g_tables(const pcs::Shape& sh, size_t* max_len) { return bnfold_g_tables(sh, max_len); }
    static size_t fold_gblock_bytes(const pcs::Shape& sh, const FoldGTables& A, const std::vector<PcsClaim>& claims) { return bnfold_gblock_bytes(sh, A, claims); }
    static void fold_gblock_fill(char* stage, FoldGMember& d, size_t at, const pcs::Shape& sh, const FoldGTables& A, const std::vector<PcsClaim>& claims, const std::vector<Fr>& bpow,
                                 std::vector<Fr>& G1) {
        bnfold_gblock_fill(stage, d, at, sh, A, claims, bpow, G1);
    }
    static FoldBufs fold_alloc(hg_ctx* ctx, const pcs::Shape& sh, size_t G, unsigned max_blocks) { return bnfold_alloc(ctx, sh, G, max_blocks); }
    static FoldTables fold_tables(const pcs::Shape& sh, size_t j, bool* retire, size_t* max_units, size_t* entries) { return bnfold_tables(sh, j, retire, max_units, entries); }
    static FoldK fold_chal(const Fr& r) {   // r canonical
        FoldK k;
        fold_consts(fr_to_mont(r), &k);
        return k;
    }
    static FoldMembers fold_members(const pcs::Shape& sh, const Fr* const* rows, const FoldK* fk) { return bnfold_members(sh, rows, fk); }
    static void fold_g_launch(hipStream_t st, unsigned max_blocks, const FoldGTables& A, size_t max_len, size_t G, const FoldMembers& M, const char* d_stage, const FoldBufs& b) {
        bnfold_g_launch(st, max_blocks, A, max_len, G, M, d_stage, b);
    }
    static void fold_launch(hipStream_t st, unsigned max_blocks, const pcs::Shape& sh, size_t j, const FoldTables& A, size_t max_units, size_t G, const FoldMembers& M,
                            const FoldBufs& b, bool sums) {
        bnfold_launch(st, max_blocks, sh, j, A, max_units, G, M, b, sums);
    }
    static double fold_step_bytes(size_t j, size_t entries) { return bnfold_step_bytes(j, entries); }
};
std::vector<std::string> pcs_verify_folded_device_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<VerifyItem>& items, size_t Q) {
    return pcs::verify_batch_flow<BnPcs>(who, ctx, sh, items, Q, true);
}
std::vector<pcs::Opened> pcs_open_folded_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q) {
    return pcs::open_folded_batch_flow<BnFoldPcs>(who, single, ctx, items, Q);
}
