// Device form of the polynomial commitment over bn256::Fr (pcs_bn254.hpp), part of bn254.hip. Rows and the encoded matrix lie in
// HBM as canonical plain words (4 an element): the transform is linear and its twiddle products are Montgomery products with
// Montgomery-form powers of w, so plain words go through ntt_batch_dev and come out plain - no conversion pass on either NTT path,
// and the leaf hash and the column gather read the matrix as it is. Keccak and the tree are those of the Goldilocks form
// (pcs_keccak.hpp, pcs::merkle_levels_device): a node is 32 bytes in either field.
// The verifier of an opening reuses the encoding, the leaf sponge and the accumulators and adds five kernels.
// Every step has one kernel, written for a group of members and driven by a member or job table; the forms for a run
// (pcs_commit_device_batch, pcs_open_device_batch, pcs_verify_device_batch) launch it once over a group, whose matrices lie in one
// allocation that its handles share, and the forms for one (pcs_commit_device, pcs_combine_device, pcs_verify_device) launch it
// over a group of one from a host flow of their own.

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
// offsets the entry point validated. Each result cell holds the lowest offending key (atomicMin), so the reason is the host's also
// where several checks fail at once.
constexpr u64 BNPCSV_NONE = ~(u64)0;   // a cell no thread lowered: nothing failed
__device__ __forceinline__ void bnpcsv_min(u64* cell, u64 v) { atomicMin(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)v); }
struct BnPcsDesc { u64 row0, nrows, woff; };   // a row combination: sum_{r < nrows} w[woff + r] * row_{row0 + r}
struct BnVbMember {
    u64 proof, u, cols, enc_row;               // word offset of its opening in the set; element offsets of its u and columns; its first row of enc
    u64 n, claim0, job0;                       // its claims; the claims and the jobs (claims + 1 each) of the members before it
    u64 root_at, jobs_at, y_at, z_at, w_at;    // byte offsets in the group's staged copy: root, job descriptors, values, low coordinates, weights
};
struct BnVbGroup { u64 G, Q, R, q_el; int c, depth; };

// 32 big-endian bytes of an opening -> 4 native limbs (limb w = the byte-swapped word 3 - w); blockIdx.y = the member, its elements
// grid-strided over blockIdx.x. Element i < u_el is element i & (C - 1) of u vector i >> c: kept in u and scattered into row i >> c
// of the member's rows of the matrix the NTT encodes (zeroed beforehand). The others are the Q * R column elements, query q at
// element u_el + q * q_el. cells[3m] = the lowest byte offset, within its opening, of an element that is not below r (all four limbs
// compared). Elements stay plain words: no Montgomery conversion (ntt_batch_dev keeps the form).
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_canon(const u64* __restrict__ set, const BnVbMember* __restrict__ mem, BnVbGroup g, Fr* __restrict__ u,
                                                             Fr* __restrict__ cols, Fr* __restrict__ enc, u64* __restrict__ cells) {
    const BnVbMember M = mem[blockIdx.y];
    const int c = g.c;
    const size_t Q = g.Q, R = g.R, u_el = (M.n + 1) << c, total = u_el + Q * R, Cm = ((size_t)1 << c) - 1;
    const u64* proof = set + M.proof;
    Fr* mu = u + M.u;
    Fr* mcols = cols + M.cols;
    Fr* menc = enc + (M.enc_row << (c + 2));
    u64 bad = BNPCSV_NONE;
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * BNPCS_TPB) {
        size_t at = i;
        if (i >= u_el) { const size_t k = i - u_el, q = k / R; at = u_el + q * g.q_el + (k - q * R); }
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
    if (bad != BNPCSV_NONE) bnpcsv_min(cells + 3 * blockIdx.y, bad);
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
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_eval(const BnVbMember* __restrict__ mem, unsigned G, int c, const Fr* __restrict__ u, const char* __restrict__ stage,
                                                            u64* __restrict__ cells) {
    unsigned lo = 0, hi = G;
    while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].claim0 <= blockIdx.x) lo = mid; else hi = mid; }
    const BnVbMember M = mem[lo];
    const size_t i = blockIdx.x - M.claim0;
    if (i >= M.n) return;   // (uniform over the workgroup; the grid has exactly the claims of the group)
    if (bnpcs_eval_differs(u + M.u + ((i + 1) << c), reinterpret_cast<const Fr*>(stage + M.z_at) + i * (size_t)c, reinterpret_cast<const Fr*>(stage + M.y_at) + i, c))
        bnpcsv_min(cells + 3 * lo + 1, (u64)i);
}

// One thread per (member m, query q), id = m Q + q: the leaf hash of its R column elements (contiguous: 4 words between them) -> leaves[id]
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_leaf(const BnVbMember* __restrict__ mem, BnVbGroup g, const Fr* __restrict__ cols, u64* __restrict__ leaves) {
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
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_dots(const BnVbMember* __restrict__ mem, BnVbGroup g, unsigned bq, const Fr* __restrict__ cols,
                                                            const char* __restrict__ stage, Fr* __restrict__ s) {
    const size_t gjob = blockIdx.x / bq;
    const size_t q = (size_t)(blockIdx.x % bq) * BNPCS_TPB + threadIdx.x;
    if (q >= g.Q) return;
    unsigned lo = 0, hi = (unsigned)g.G;
    while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].job0 <= gjob) lo = mid; else hi = mid; }
    const BnVbMember M = mem[lo];
    const BnPcsDesc job = reinterpret_cast<const BnPcsDesc*>(stage + M.jobs_at)[gjob - M.job0];
    lz_gstore(s + gjob * g.Q + q, bnpcs_dot_chunked(cols + M.cols + q * g.R + job.row0, 0, reinterpret_cast<const Fr*>(stage + M.w_at) + job.woff, job.nrows));
}

// One thread per (member m, query q), id = m Q + q, once the host has every member's column indices (js[id]): the path from the leaf
// hash over the c+2 siblings (32 raw bytes each behind the query's column elements) against the member's root, then s[job 0][q]
// against Enc(u_0)[j_q], then s[job 1 + i][q] against Enc(u_i)[j_q]. cells[3m + 2] = the member's lowest q (n_m + 2) + kind that
// failed: kind 0 the path, 1 proximity, 2 + i claim i.
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsvb_query(const u64* __restrict__ set, const BnVbMember* __restrict__ mem, BnVbGroup g, const u64* __restrict__ leaves,
                                                             const Fr* __restrict__ s, const Fr* __restrict__ enc, const u64* __restrict__ js,
                                                             const char* __restrict__ stage, u64* __restrict__ cells) {
    const size_t id = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (id >= g.G * g.Q) return;
    const size_t m = id / g.Q, q = id - m * g.Q;
    const BnVbMember M = mem[m];
    const int depth = g.depth;
    const size_t N = (size_t)1 << depth, j = js[id], n = M.n, u_el = (n + 1) << g.c;
    const u64* sib = set + M.proof + 4 * (u_el + q * g.q_el + g.R);
    const u64* root = reinterpret_cast<const u64*>(stage + M.root_at);
    u64 h[4] = {leaves[4 * id], leaves[4 * id + 1], leaves[4 * id + 2], leaves[4 * id + 3]};
    pcs::merkle_climb(h, sib, j, depth);
    u64* cell = cells + 3 * m + 2;
    const size_t key = q * (n + 2);
    if (h[0] != root[0] || h[1] != root[1] || h[2] != root[2] || h[3] != root[3]) { bnpcsv_min(cell, key); return; }
    const Fr* sq = s + M.job0 * g.Q + q;
    const Fr* menc = enc + (M.enc_row << depth) + j;
    for (size_t i = 0; i <= n; i++)
        if (!fr_eq(lz_gload(sq + i * g.Q), lz_gload(menc + i * N))) { bnpcsv_min(cell, key + 1 + i); return; }
}

// ---- the kernels of the prover's side of an opening, written for a group of items (pcs_open_device_batch); the row combinations of
// one opening (pcs_combine_device) are a job table of their own. What differs by item lies in three flat tables of the staged copy:
// a job a row combination (the proximity combination and one a claim, every member's behind the other), a claim an evaluation
// check, a member where its matrix, its u vectors and its opening image lie. Every block of the staged copy starts at a multiple of
// 32 bytes (lz_gload reads 16-byte halves). Every grid is one-dimensional.
struct BnObJob { const Fr* src; u64 nrows, w_at, u_at; };      // its first raw row; the byte offset of its weights in the staged copy; where u goes (elements)
struct BnObClaim { u64 u_at, z_at, y_at, member, claim; };     // its u_i (elements); byte offsets of the low coordinates (Montgomery) and of the value
struct BnObMember { const Fr* M; u64 img, u, u_words; };       // its encoded matrix; word offsets of its image and of its u vectors; 4 C (n + 1)

// Row combinations: u[u_at + j] = sum_{r < nrows} w[r] * src[r][j] for the job of the workgroup, a thread owns column j. Workgroup b
// serves job b / cb alone, columns (b % cb) BNPCS_TPB .. - the weight limbs go through readfirstlane, so every lane of a wavefront
// must be on one job
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_combine(int c, unsigned cb, const BnObJob* __restrict__ jobs, const char* __restrict__ stage, Fr* __restrict__ u) {
    const size_t C = (size_t)1 << c;
    const unsigned jq = blockIdx.x / cb;
    const size_t j = (size_t)(blockIdx.x - jq * cb) * BNPCS_TPB + threadIdx.x;
    if (j >= C) return;
    const BnObJob job = jobs[jq];
    lz_gstore(u + job.u_at + j, bnpcs_dot_chunked(job.src + j, c, reinterpret_cast<const Fr*>(stage + job.w_at), job.nrows));
}
// One workgroup per (member, claim): <u_i, eq(z_i[..c])> == y_i; cells[member] = its lowest failing claim
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_eval(const BnObClaim* __restrict__ claims, int c, const Fr* __restrict__ u, const char* __restrict__ stage,
                                                            u64* __restrict__ cells) {
    const BnObClaim cl = claims[blockIdx.x];
    if (bnpcs_eval_differs(u + cl.u_at, reinterpret_cast<const Fr*>(stage + cl.z_at), reinterpret_cast<const Fr*>(stage + cl.y_at), c)) bnpcsv_min(cells + cl.member, cl.claim);
}
// Word i of the group's u vectors into its member's image, an element as 32 bytes big-endian: word w of the image's element is the
// byte-swapped limb 3 - w. The member is the last one whose u offset is <= i (offsets are multiples of 4: an element never straddles)
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_emit(const BnObMember* __restrict__ mem, unsigned G, size_t total, const u64* __restrict__ u, u64* __restrict__ img) {
    for (size_t i = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * BNPCS_TPB) {
        unsigned lo = 0, hi = G;
        while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (mem[mid].u <= i) lo = mid; else hi = mid; }
        img[mem[lo].img + (i - mem[lo].u)] = __builtin_bswap64(u[i ^ 3]);
    }
}
// One thread per (member m, query q, row r), id = (m Q + q) R + r: M_m[r][j_q] big-endian at its place in the member's image.
// js[m Q + q] = j_q (masked by the host); js[G Q + m] != 0: the member takes part (it was not refused)
__global__ __launch_bounds__(BNPCS_TPB) void k_bnpcsob_gather(const BnObMember* __restrict__ mem, size_t G, size_t Q, size_t R, size_t N, size_t q_words,
                                                              const u64* __restrict__ js, u64* __restrict__ img) {
    const size_t id = (size_t)blockIdx.x * BNPCS_TPB + threadIdx.x;
    if (id >= G * Q * R) return;
    const size_t m = id / (Q * R), k = id - m * Q * R, q = k / R, r = k - q * R;
    if (!js[G * Q + m]) return;
    const BnObMember M = mem[m];
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
    pcs::DrainOne drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
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

void pcs_combine_device(const pcs::Commitment& cm, const std::vector<PcsJob>& jobs, Fr* u) {
    hg_ctx* ctx = cm.ctx;
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t C = cm.sh.C(), nj = jobs.size();
    if (nj > 65535) throw Error("hg_pcs_open_bn254: more than 65534 claims");
    // the job table and the weights in one staged copy; job q's u vector is the q-th
    size_t nw = 0;
    for (const PcsJob& j : jobs) nw += j.nrows;
    const size_t desc_bytes = (nj * sizeof(BnObJob) + 31) & ~(size_t)31;
    std::vector<char> stage(desc_bytes + nw * sizeof(Fr));
    BnObJob* hd = reinterpret_cast<BnObJob*>(stage.data());
    size_t w_at = desc_bytes;
    for (size_t q = 0; q < nj; q++) {
        hd[q].src = reinterpret_cast<const Fr*>(cm.d_rows) + (jobs[q].row0 << cm.sh.c); hd[q].nrows = jobs[q].nrows; hd[q].w_at = w_at; hd[q].u_at = q * C;
        memcpy(stage.data() + w_at, jobs[q].w.data(), jobs[q].nrows * sizeof(Fr));
        w_at += jobs[q].nrows * sizeof(Fr);
    }
    char* d_stage = ctx->alloc_n<char>(stage.size());
    Fr* d_u = ctx->alloc_n<Fr>(nj * C);
    const unsigned cb = bnpcs_blocks(C);   // (at most 2^16 workgroups a job and, by the entry point, MAX_CLAIMS + 1 jobs: inside a grid's x)
    const int cls = ctx->prof_class("pcs_bn254_combine", false);
    ctx->prof_stream = st;
    hipc(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload weights");
    ctx->prof_begin(cls, (double)nw * C * 32);
    k_bnpcsob_combine<<<(unsigned)(nj * cb), BNPCS_TPB, 0, st>>>(cm.sh.c, cb, reinterpret_cast<const BnObJob*>(d_stage), d_stage, d_u);
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

// ---- what the two verifiers share on the host: a member's block of the staged copy and the reading of its three result cells
// the entries of a member's weight tables: R powers of rho, then eq(z_i[c..]) over the rows of every claim's table
static size_t bnpcs_weights_of(const pcs::Shape& sh, const std::vector<PcsClaim>& claims) {
    size_t nw = sh.R;
    for (const PcsClaim& cl : claims) nw += (size_t)1 << (sh.nvars[cl.table] - sh.c);
    return nw;
}
// The block of a member of n claims and nw weights from byte `at` (a multiple of 32) of a staged copy on: root, job descriptors,
// values, the low coordinates of the points, weight tables. Into its descriptor -> the byte behind the block
static size_t bnpcs_block_layout(BnVbMember& d, const pcs::Shape& sh, size_t n, size_t nw, size_t at) {
    d.root_at = at;
    d.jobs_at = d.root_at + 32;
    d.y_at = d.jobs_at + (((n + 1) * sizeof(BnPcsDesc) + 31) & ~(size_t)31);
    d.z_at = d.y_at + n * sizeof(Fr);
    d.w_at = d.z_at + n * (size_t)sh.c * sizeof(Fr);
    return d.w_at + nw * sizeof(Fr);
}
// fills the block (the low coordinates and the weights in Montgomery form) -> the member's transcript, rho squeezed
static FsTranscript bnpcs_block_fill(char* h_stage, const BnVbMember& d, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q) {
    const size_t R = sh.R;
    FsTranscript tr = pcs_start_transcript(sh, root, claims, Q);
    const std::vector<Fr> rho = pcs_rho_powers(pcs_squeeze(tr), R);
    memcpy(h_stage + d.root_at, root, 32);
    BnPcsDesc* hd = reinterpret_cast<BnPcsDesc*>(h_stage + d.jobs_at);
    Fr* hy = reinterpret_cast<Fr*>(h_stage + d.y_at);
    Fr* hz = reinterpret_cast<Fr*>(h_stage + d.z_at);
    Fr* hw = reinterpret_cast<Fr*>(h_stage + d.w_at);
    hd[0].row0 = 0; hd[0].nrows = R; hd[0].woff = 0;
    memcpy(hw, rho.data(), R * sizeof(Fr));
    size_t off = R;
    for (size_t i = 0; i < claims.size(); i++) {
        const PcsClaim& cl = claims[i];
        const std::vector<Fr> w = pcs_eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
        hd[i + 1].row0 = sh.off[cl.table]; hd[i + 1].nrows = w.size(); hd[i + 1].woff = off;
        memcpy(hw + off, w.data(), w.size() * sizeof(Fr));
        off += w.size();
        hy[i] = cl.value;
        for (int b = 0; b < sh.c; b++) hz[i * (size_t)sh.c + b] = fr_to_mont(cl.point[b]);
    }
    return tr;
}
// the host's order: a non-canonical element, the lowest claim whose evaluation fails, the lowest failing query; "" = accepted
static std::string bnpcs_cells_reason(const u64* cells, size_t n) {
    if (cells[0] != BNPCSV_NONE) return pcs::reason_noncanonical((size_t)cells[0]);
    if (cells[1] != BNPCSV_NONE) return pcs::reason_evaluation((size_t)cells[1]);
    if (cells[2] == BNPCSV_NONE) return "";
    const size_t q = (size_t)(cells[2] / (n + 2)), kind = (size_t)(cells[2] % (n + 2));
    return kind == 0 ? pcs::reason_merkle(q) : kind == 1 ? pcs::reason_proximity(q) : pcs::reason_claim(kind - 2, q);
}

// hg_pcs_verify_device_bn254: a group of one member, whose opening in the arena is the set. Everything but the last kernel needs no
// column index, so it is enqueued first and runs while the host hashes the u_i; the indices follow on the same stream, then the
// three result cells come back: one synchronisation. The leaf sponge (serial: 4R + 1 words a thread, Q threads) is the longest of the
// early kernels and goes last among them, so the two verdicts that need no index and the inner products never wait behind it; the
// host's own hash of the u_i covers it.
std::string pcs_verify_device(hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R, n = claims.size();
    const int depth = sh.depth();
    const std::string bad_len = pcs::length_reason(len, pcs_opening_bytes(sh, n, Q));
    if (!bad_len.empty()) return bad_len;
    const size_t u_el = C * (n + 1), q_el = R + (size_t)depth, njobs = n + 1;
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    // the member's descriptor and its block in one staged copy
    const size_t nw = bnpcs_weights_of(sh, claims);
    BnVbMember desc{};   // (every offset into the set and the arena buffers is 0)
    desc.n = n;
    std::vector<char> stage(bnpcs_block_layout(desc, sh, n, nw, sizeof(BnVbMember)));
    static_assert(sizeof(BnVbMember) % 32 == 0, "the block starts at a multiple of 32");
    memcpy(stage.data(), &desc, sizeof(BnVbMember));
    FsTranscript tr = bnpcs_block_fill(stage.data(), desc, sh, root, claims, Q);
    u64 *d_proof, *d_leaves, *d_js, *d_cells;
    Fr *d_u, *d_cols, *d_enc, *d_tmp, *d_W, *d_s;
    char* d_stage;
    try {
        d_proof = ctx->alloc_n<u64>(len / 8);
        d_stage = ctx->alloc_n<char>(stage.size());
        d_u = ctx->alloc_n<Fr>(u_el);
        d_cols = ctx->alloc_n<Fr>(Q * R);
        d_enc = ctx->alloc_n<Fr>(njobs * N);
        d_tmp = ctx->alloc_n<Fr>(njobs * N);
        d_W = ctx->alloc_n<Fr>(N);
        d_leaves = ctx->alloc_n<u64>(4 * Q);
        d_s = ctx->alloc_n<Fr>(Q * njobs);
        d_js = ctx->alloc_n<u64>(Q);
        d_cells = ctx->alloc_n<u64>(4);
    } catch (const std::exception& e) {
        throw Error(std::string("the context's arena cannot hold the opening (") + e.what() + ")");
    }
    pcs::DrainOne drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
    const int cls = ctx->prof_class("pcs_bn254_verify", false);
    ctx->prof_stream = st;
    const BnVbMember* d_mem = reinterpret_cast<const BnVbMember*>(d_stage);
    const BnVbGroup vg{1, (u64)Q, (u64)R, (u64)q_el, sh.c, depth};
    const size_t bq = bnpcs_blocks(Q);   // k_bnpcsvb_dots: the workgroups of a job
    hipc(hipMemcpyAsync(d_proof, proof, len, hipMemcpyHostToDevice, st), "upload opening");
    hipc(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload claims");
    hipc(hipMemsetAsync(d_cells, 0xff, 32, st), "memset");
    hipc(hipMemsetAsync(d_enc, 0, njobs * N * sizeof(Fr), st), "memset");
    ctx->prof_begin(cls, (double)(u_el + Q * R) * 64 + (double)u_el * 32);
    k_bnpcsvb_canon<<<(unsigned)std::min<size_t>(bnpcs_blocks(u_el + Q * R), 4096), BNPCS_TPB, 0, st>>>(d_proof, d_mem, vg, d_u, d_cols, d_enc, d_cells);
    ctx->prof_end();
    if (n) {
        ctx->prof_begin(cls, (double)n * C * 32);
        k_bnpcsvb_eval<<<(unsigned)n, BNPCS_TPB, 0, st>>>(d_mem, 1, sh.c, d_u, d_stage, d_cells);
        ctx->prof_end();
    }
    ctx->prof_begin(cls, (double)njobs * N * 32 * 4);
    k_bn_powers<<<bnpcs_blocks(N), 256, 0, st>>>(d_W, fr_root_of_unity(depth), N);
    ntt_batch_dev(st, d_enc, d_tmp, d_W, depth, njobs, nullptr);
    ctx->prof_end();
    if (Q) {
        ctx->prof_begin(cls, (double)Q * nw * 64);
        k_bnpcsvb_dots<<<(unsigned)(bq * njobs), BNPCS_TPB, 0, st>>>(d_mem, vg, (unsigned)bq, d_cols, d_stage, d_s);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)Q * R * 32);
        k_bnpcsvb_leaf<<<bnpcs_blocks(Q), BNPCS_TPB, 0, st>>>(d_mem, vg, d_cols, d_leaves);
        ctx->prof_end();
    }
    // the host's share, beside the kernels: the u_i into the transcript, the column indices out of it
    {
        std::vector<Fr> u(u_el);
        for (size_t i = 0; i < u_el; i++) u[i] = pcs_read_be32(proof + 32 * i);
        pcs_absorb(tr, u.data(), u_el);
    }
    const std::vector<size_t> js = pcs_squeeze_indices(tr, N, Q);
    const std::vector<u64> hj(js.begin(), js.end());
    if (Q) {
        hipc(hipMemcpyAsync(d_js, hj.data(), Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
        ctx->prof_begin(cls, (double)Q * (32.0 * depth + 64.0 * njobs));
        k_bnpcsvb_query<<<bnpcs_blocks(Q), BNPCS_TPB, 0, st>>>(d_proof, d_mem, vg, d_leaves, d_s, d_enc, d_js, d_stage, d_cells);
        ctx->prof_end();
    }
    u64 cells[4];
    hipc(hipMemcpyAsync(cells, d_cells, 32, hipMemcpyDeviceToHost, st), "download verdict");
    hipc(hipStreamSynchronize(st), "hg_pcs_verify_device_bn254: sync");
    hipc(hipGetLastError(), "hg_pcs_verify_device_bn254: launch");
    ctx->prof_collect();
    return bnpcs_cells_reason(cells, n);
}

// hg_pcs_verify_device_batch_bn254. The items whose length is right are cut into groups (the option verify_batch_group, VB_PCS_BUDGET
// over what a member takes in 32-byte elements, the transforms ntt_batch_dev takes on its four-step path). A group: its openings
// gathered into a page-locked set on the host threads and copied on the upload stream; every member's transcript start, rho powers
// and weight tables written into one staged copy, one member a task; the index-free kernels, one launch each over all members, the
// leaf sponge last among them as in the single call; the members' u_i hashed on the host threads meanwhile; all indices up, the
// query kernel, three cells a member down: one synchronisation a group. The next group's openings are gathered and copied into the
// other set before that synchronisation, under this group's kernels.
std::vector<std::string> pcs_verify_device_batch(const char* who_c, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<VerifyItem>& items, size_t Q) {
    const std::string who(who_c);
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int depth = sh.depth();
    const size_t q_el = R + (size_t)depth;
    const bool four_step = depth >= 8 && depth <= 16;
    std::vector<std::string> why(items.size());
    std::vector<size_t> good;   // the items that reach the device
    for (size_t i = 0; i < items.size(); i++) {
        why[i] = pcs::length_reason(items[i].len, pcs_opening_bytes(sh, items[i].claims->size(), Q));
        if (why[i].empty()) good.push_back(i);
    }
    if (good.empty()) return why;
    // what a member takes: its opening in a set; u, columns, enc rows and as many for the NTT temporary, s (32 bytes an element),
    // leaves and indices in the arena
    auto rows_of = [](size_t n) { return n + 1; };
    auto bytes_of = [&](size_t n, size_t len) { return len + sizeof(Fr) * (C * (n + 1) + Q * R + 2 * rows_of(n) * N + Q * (n + 1)) + 8 * 5 * Q; };
    size_t cap = VB_MAX_GROUP;
    if (ctx->verify_batch_group > 0) cap = std::min<size_t>(cap, (size_t)ctx->verify_batch_group);
    constexpr size_t NTT_ROWS = 65535;   // ntt_batch_dev: the batch is the y extent of its four-step grids
    // k_bnpcsvb_dots: bq workgroups a job (a member's jobs are its rows) in one x extent, and a launch takes fewer than 2^32 threads.
    // One member is at most 4097 jobs of 256 workgroups, far inside it.
    const size_t bq = bnpcs_blocks(Q), DOTS_BLOCKS = (((size_t)1 << 32) / BNPCS_TPB - 1) / bq;
    std::vector<std::pair<size_t, size_t>> groups;   // [first, last) of good
    for (size_t a = 0; a < good.size();) {
        size_t b = a, bytes = 0, rows = 0;
        while (b < good.size() && b - a < cap) {
            const size_t n = items[good[b]].claims->size();
            if (b > a && (bytes + bytes_of(n, items[good[b]].len) > VB_PCS_BUDGET || (four_step && rows + rows_of(n) > NTT_ROWS) || rows + rows_of(n) > DOTS_BLOCKS)) break;
            bytes += bytes_of(n, items[good[b]].len);
            rows += rows_of(n);
            b++;
        }
        groups.push_back({a, b});
        a = b;
    }
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    hipStream_t st = ctx->stream;
    std::vector<u64> hj, cells;   // (declared ahead of the guard: copies of them may be queued when it drains)
    pcs::DrainOne drain_up{B->up}, drain{st};   // (the upload stream as well: no kernel on a set left behind)
    hipc(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());   // (the device pass of hipcc ignores the pragmas)
    const int cls = ctx->prof_class("pcs_bn254_verify_batch", false);
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
        std::vector<BnVbMember> desc(G);
        const std::vector<size_t> poff = proof_offsets(g);
        // the layout of the staged copy: the descriptors, then every member's block, and of the arena buffers
        size_t at = (G * sizeof(BnVbMember) + 31) & ~(size_t)31, u_at = 0, row_at = 0, claim_at = 0;
        for (size_t m = 0; m < G; m++) {
            Member& x = mem[m];
            const VerifyItem& it = items[good[groups[g].first + m]];
            x.idx = good[groups[g].first + m];
            x.n = it.claims->size();
            x.nw = bnpcs_weights_of(sh, *it.claims);
            BnVbMember& d = desc[m];
            d.proof = poff[m]; d.u = u_at; d.cols = m * Q * R; d.enc_row = row_at;
            d.n = x.n; d.claim0 = claim_at; d.job0 = claim_at + m;
            at = bnpcs_block_layout(d, sh, x.n, x.nw, at);
            u_at += C * (x.n + 1);
            row_at += rows_of(x.n);
            claim_at += x.n;
        }
        const size_t stage_bytes = at, u_total = u_at, rows = row_at, claims_total = claim_at, jobs_total = claim_at + G;
        char* h_stage = batch_desc_host(B, stage_bytes);   // (the previous group's copy of it was waited for)
        memcpy(h_stage, desc.data(), G * sizeof(BnVbMember));
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                const VerifyItem& it = items[x.idx];
                x.tr = bnpcs_block_fill(h_stage, desc[mq], sh, it.root, *it.claims, Q);
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        u64 *d_leaves, *d_js, *d_cells;
        Fr *d_u, *d_cols, *d_enc, *d_tmp, *d_W, *d_s;
        char* d_stage;
        try {
            d_stage = ctx->alloc_n<char>(stage_bytes);
            d_u = ctx->alloc_n<Fr>(u_total);
            d_cols = ctx->alloc_n<Fr>(G * Q * R);
            d_enc = ctx->alloc_n<Fr>(rows * N);
            d_tmp = ctx->alloc_n<Fr>(rows * N);
            d_W = ctx->alloc_n<Fr>(N);
            d_leaves = ctx->alloc_n<u64>(4 * G * Q);
            d_s = ctx->alloc_n<Fr>(Q * jobs_total);
            d_js = ctx->alloc_n<u64>(G * Q);
            d_cells = ctx->alloc_n<u64>(3 * G);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold " + (G == 1 ? "the opening at index " + std::to_string(mem[0].idx) : "a group of " + std::to_string(G) + " openings: lower verify_batch_group") +
                        " (" + e.what() + ")");
        }
        const u64* d_set = B->d_in[set];
        const BnVbMember* d_mem = reinterpret_cast<const BnVbMember*>(d_stage);
        const BnVbGroup vg{(u64)G, (u64)Q, (u64)R, (u64)q_el, sh.c, depth};
        size_t el_max = 0, nw_total = 0;
        for (const Member& x : mem) { el_max = std::max(el_max, C * (x.n + 1) + Q * R); nw_total += x.nw; }
        hipc(hipStreamWaitEvent(st, B->ev[set], 0), "hipStreamWaitEvent");   // the set's openings are up
        hipc(hipMemcpyAsync(d_stage, h_stage, stage_bytes, hipMemcpyHostToDevice, st), "upload claims");
        hipc(hipMemsetAsync(d_cells, 0xff, 3 * G * 8, st), "memset");
        hipc(hipMemsetAsync(d_enc, 0, rows * N * sizeof(Fr), st), "memset");
        ctx->prof_begin(cls, (double)(u_total + G * Q * R) * 64 + (double)u_total * 32);
        k_bnpcsvb_canon<<<dim3((unsigned)std::min<size_t>(bnpcs_blocks(el_max), 1024), (unsigned)G), BNPCS_TPB, 0, st>>>(d_set, d_mem, vg, d_u, d_cols, d_enc, d_cells);
        ctx->prof_end();
        if (claims_total) {
            ctx->prof_begin(cls, (double)claims_total * C * 32);
            k_bnpcsvb_eval<<<(unsigned)claims_total, BNPCS_TPB, 0, st>>>(d_mem, (unsigned)G, sh.c, d_u, d_stage, d_cells);
            ctx->prof_end();
        }
        ctx->prof_begin(cls, (double)rows * N * 32 * 4);
        k_bn_powers<<<bnpcs_blocks(N), 256, 0, st>>>(d_W, fr_root_of_unity(depth), N);
        ntt_batch_dev(st, d_enc, d_tmp, d_W, depth, rows, nullptr);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)Q * nw_total * 64);
        k_bnpcsvb_dots<<<(unsigned)(bq * jobs_total), BNPCS_TPB, 0, st>>>(d_mem, vg, (unsigned)bq, d_cols, d_stage, d_s);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * Q * R * 32);
        k_bnpcsvb_leaf<<<bnpcs_blocks(G * Q), BNPCS_TPB, 0, st>>>(d_mem, vg, d_cols, d_leaves);
        ctx->prof_end();
        // the host's share, beside the kernels: every member's u_i into its transcript, its column indices out of it
        const double t2 = omp_get_wtime();
        hj.assign(G * Q, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                const uint8_t* proof = items[x.idx].proof;
                const size_t u_el = C * (x.n + 1);
                std::vector<Fr> u(u_el);
                for (size_t i = 0; i < u_el; i++) u[i] = pcs_read_be32(proof + 32 * i);
                pcs_absorb(x.tr, u.data(), u_el);
                const std::vector<size_t> js = pcs_squeeze_indices(x.tr, N, Q);
                for (size_t q = 0; q < Q; q++) hj[(size_t)mq * Q + q] = js[q];
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        const double t3 = omp_get_wtime();
        hipc(hipMemcpyAsync(d_js, hj.data(), G * Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
        ctx->prof_begin(cls, (double)G * Q * 32.0 * depth + (double)Q * jobs_total * 64.0);
        k_bnpcsvb_query<<<bnpcs_blocks(G * Q), BNPCS_TPB, 0, st>>>(d_set, d_mem, vg, d_leaves, d_s, d_enc, d_js, d_stage, d_cells);
        ctx->prof_end();
        cells.assign(3 * G, 0);
        hipc(hipMemcpyAsync(cells.data(), d_cells, 3 * G * 8, hipMemcpyDeviceToHost, st), "download verdicts");
        const double t4 = omp_get_wtime();
        if (g + 1 < groups.size()) stage(g + 1);   // into the other set, under this group's kernels
        const double t5 = omp_get_wtime();
        hipc(hipStreamSynchronize(st), (who + ": sync").c_str());
        if (times)
            fprintf(stderr, "[hg pcs] group %zu of %zu members: gather and copy of its openings %.2f ms, transcripts and weights %.2f, enqueue %.2f, hash %.2f, "
                            "query enqueue %.2f, next group's gather %.2f, wait %.2f\n", g, G, t_stage * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3,
                    (t5 - t4) * 1e3, (omp_get_wtime() - t5) * 1e3);
        t_stage = t5 - t4;
        hipc(hipGetLastError(), (who + ": launch").c_str());
        ctx->prof_collect();
        for (size_t m = 0; m < G; m++) why[mem[m].idx] = bnpcs_cells_reason(cells.data() + 3 * m, mem[m].n);
    }
    return why;
}

// hg_pcs_commit_batch_bn254. A group: one allocation for its members' raw and encoded rows (a freed group's, where the context
// holds one that fits: pcs::SlabSpares), the tables (or, `words`, the witness
// words, lifted by one k_bnpcs_lift over the group) uploaded straight into it, then k_bnpcsb_stage, the encoding in slices of whole
// members through ONE slice's temporary (the slices follow each other on the stream, so the temporary does not grow with the
// group), the leaf hashes, the tree levels of pcs::merkle_levels_device_batch, one download of all trees and flags, one
// synchronisation.
constexpr size_t BNPCSB_NTT_TMP = (size_t)256 << 20;   // the temporary of one slice: at least one member, else what fits in here
std::vector<pcs::Commitment*> pcs_commit_device_batch(const char* who_c, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tables, size_t n, bool words) {
    const std::string who(who_c);
    const size_t C = sh.C(), N = sh.N(), R = sh.R, nt = sh.nvars.size();
    const int log2n = sh.depth();
    if (R > 65535) throw Error(who + ": more than 65535 rows (choose a larger log2_row)");
    const size_t tree_words = 8 * N;   // 2N nodes of 4 words: the 2N - 1 of a tree and one unused
    const size_t member_bytes = sizeof(Fr) * (R * C + R * N);
    // ntt_batch_dev: the batch is the y extent of its four-step grids, and a slice is at most a group
    const std::vector<std::pair<size_t, size_t>> groups = pcs::cut_groups(ctx, n, [&](size_t) { return member_bytes; }, R, 65535, VB_PCS_COMMIT_BUDGET_BN254);
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    const std::shared_ptr<pcs::SlabSpares> spares = batch_bufs(ctx)->slabs;
    std::vector<std::unique_ptr<pcs::Commitment>> made;
    std::vector<u64> h_out;   // (declared ahead of the guard: a copy into it may be queued when it drains)
    pcs::DrainOne drain{st};
    hipc(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    const int cls = ctx->prof_class("pcs_bn254_commit_batch", false);
    ctx->prof_stream = st;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr
    for (const auto& grp : groups) {
        const double t0 = omp_get_wtime();
        const size_t first = grp.first, G = grp.second - grp.first;
        const size_t slice = std::min(G, std::max<size_t>(1, BNPCSB_NTT_TMP / (R * N * sizeof(Fr))));   // members a slice
        std::shared_ptr<pcs::Slab> slab = std::make_shared<pcs::Slab>();
        slab->home = spares;
        slab->p = spares->take(G * member_bytes, &slab->bytes);   // a freed group's allocation, if the context holds one that fits
        if (!slab->p) {
            hipc(hipMalloc((void**)&slab->p, G * member_bytes), "hipMalloc(pcs rows and encoded matrices of a group)");
            slab->bytes = G * member_bytes;
        }
        Fr* d_rows = reinterpret_cast<Fr*>(slab->p);
        Fr* d_M = d_rows + G * R * C;
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        Fr *tmp, *W;
        u64 *d_out, *d_words = nullptr;
        const size_t out_words = G * tree_words + (G + 1) / 2;   // the trees, then one 32-bit flag a member
        try {
            tmp = ctx->alloc_n<Fr>(slice * R * N);
            W = ctx->alloc_n<Fr>(N);
            d_out = ctx->alloc_n<u64>(out_words);
            if (words) d_words = ctx->alloc_n<u64>(G * R * C);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold a group of " + std::to_string(G) + " commitments: lower verify_batch_group (" + e.what() + ")");
        }
        unsigned* d_flags = reinterpret_cast<unsigned*>(d_out + G * tree_words);
        hipc(hipMemsetAsync(d_flags, 0, ((G + 1) / 2) * 8, st), "memset");
        for (size_t m = 0; m < G; m++)
            for (size_t t = 0; t < nt; t++) {
                const size_t len = (size_t)1 << sh.nvars[t], at = (m * R + sh.off[t]) * C;
                if (words) hipc(hipMemcpyAsync(d_words + at, tables[(first + m) * nt + t], len * 8, hipMemcpyHostToDevice, st), "upload tables");
                else hipc(hipMemcpyAsync(d_rows + at, tables[(first + m) * nt + t], len * sizeof(Fr), hipMemcpyHostToDevice, st), "upload tables");
            }
        const double t2 = omp_get_wtime();
        ctx->prof_begin(cls, (double)G * R * C * (words ? 40 : 0) + (double)G * R * (C + N) * 32);
        if (words) k_bnpcs_lift<<<(unsigned)std::min<size_t>(bnpcs_blocks(G * R * C), 4096), BNPCS_TPB, 0, st>>>(d_words, d_rows, G * R * C);
        k_bnpcsb_stage<<<dim3((unsigned)std::min<size_t>(bnpcs_blocks(R * N), (4096 + G - 1) / G), (unsigned)G), BNPCS_TPB, 0, st>>>(d_rows, d_M, R, sh.c, d_flags);   // about 4096 workgroups in all; G in the grid's y: cut_groups keeps it at VB_MAX_GROUP = 64 or below
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * R * N * 32 * 4);
        k_bn_powers<<<bnpcs_blocks(N), 256, 0, st>>>(W, fr_root_of_unity(log2n), N);
        for (size_t m0 = 0; m0 < G; m0 += slice) ntt_batch_dev(st, d_M + m0 * R * N, tmp, W, log2n, std::min(slice, G - m0) * R, nullptr);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * R * N * 32);
        k_bnpcsb_leaf_hash<<<bnpcs_blocks(G * N), BNPCS_TPB, 0, st>>>(d_M, G, log2n, R, d_out, tree_words);
        ctx->prof_end();
        ctx->prof_begin(cls, (double)G * N * 96);
        pcs::merkle_levels_device_batch(st, d_out, tree_words, N, G);
        ctx->prof_end();
        h_out.resize(out_words);
        hipc(hipMemcpyAsync(h_out.data(), d_out, out_words * 8, hipMemcpyDeviceToHost, st), "download trees and flags");
        const double t3 = omp_get_wtime();
        hipc(hipStreamSynchronize(st), (who + ": sync").c_str());
        const double t4 = omp_get_wtime();
        hipc(hipGetLastError(), (who + ": launch").c_str());
        ctx->prof_collect();
        const unsigned* flags = reinterpret_cast<const unsigned*>(h_out.data() + G * tree_words);
        for (size_t m = 0; m < G; m++)
            if (flags[m]) throw Error(who + ": index " + std::to_string(first + m) + ": a table holds an element that is not below r");
        for (size_t m = 0; m < G; m++) {
            std::unique_ptr<pcs::Commitment> cm(new pcs::Commitment());
            cm->field = pcs::BN254;
            cm->sh = sh;
            cm->ctx = ctx;
            cm->d_rows = reinterpret_cast<u64*>(d_rows + m * R * C);
            cm->d_M = reinterpret_cast<u64*>(d_M + m * R * N);
            cm->owner = slab;
            const uint8_t* tree = reinterpret_cast<const uint8_t*>(h_out.data() + m * tree_words);
            cm->tree.assign(tree, tree + 32 * (2 * N - 1));
            made.push_back(std::move(cm));
        }
        if (times)
            fprintf(stderr, "[hg pcs] bn254 commit group of %zu members (%zu a slice of the encoding): allocation %.2f ms, uploads %.2f, enqueue %.2f, wait %.2f, trees into the handles %.2f\n",
                    G, slice, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (omp_get_wtime() - t4) * 1e3);
    }
    std::vector<pcs::Commitment*> out;
    for (auto& cm : made) out.push_back(cm.release());
    return out;
}

// hg_pcs_open_batch_bn254, pcs::open_device_batch step for step. A group: the host threads write every member's transcript start,
// rho powers, weight tables (Montgomery form) and table entries into one staged copy; the combinations, the evaluation checks and
// the big-endian u vectors run as one launch each; the u vectors and one cell a member come back (first synchronisation); the host
// threads hash each member's u_i, one member a thread; all indices go up, the gather writes the opened columns into the images, the
// images come back (second synchronisation); the host copies the siblings from each handle's tree into the gaps.
std::vector<pcs::Opened> pcs_open_device_batch(const char* who_c, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q) {
    const std::string who(who_c);
    std::vector<pcs::Opened> res(items.size());
    if (items.empty()) return res;
    const pcs::Shape& sh = items[0].cm->sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int depth = sh.depth();
    const size_t q_words = 4 * (R + (size_t)depth);   // a query in the image: R elements and `depth` siblings, 4 words each
    auto align32 = [](size_t x) { return (x + 31) & ~(size_t)31; };
    auto nw_of = [&](const std::vector<PcsClaim>& cl) { size_t nw = R; for (const PcsClaim& x : cl) nw += (size_t)1 << (sh.nvars[x.table] - sh.c); return nw; };
    // what a member takes: its block of the staged copy, its u vectors and its image in the arena, its indices
    auto bytes_of = [&](size_t i) {
        const std::vector<PcsClaim>& cl = *items[i].claims;
        return sizeof(BnObMember) + (cl.size() + 1) * sizeof(BnObJob) + cl.size() * (sizeof(BnObClaim) + (size_t)(sh.c + 1) * sizeof(Fr)) + nw_of(cl) * sizeof(Fr) + 128 +
               sizeof(Fr) * C * (cl.size() + 1) + pcs_opening_bytes(sh, cl.size(), Q) + 8 * Q + 16;
    };
    const std::vector<std::pair<size_t, size_t>> groups = pcs::cut_groups(ctx, items.size(), bytes_of, 0, 0);
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    hipStream_t st = ctx->stream;
    std::vector<u64> hj;   // (declared ahead of the guard: a copy of it may be queued when it drains)
    pcs::DrainOne drain{st};
    hipc(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());   // (the device pass of hipcc ignores the pragmas)
    const int cls = ctx->prof_class("pcs_bn254_open_batch", false);
    ctx->prof_stream = st;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr

    struct Member { size_t idx, n, nw, job0, claim0, y_at, z_at, w_at, img, u, u_words, len; FsTranscript tr; bool refused = false; std::string error; };
    for (size_t g = 0; g < groups.size(); g++) {
        const double t0 = omp_get_wtime();
        const size_t G = groups[g].second - groups[g].first;
        std::vector<Member> mem(G);
        // the layout of the staged copy: the three tables, then every member's values, low coordinates and weights
        size_t jobs_total = 0, claims_total = 0, u_total = 0, img_total = 0;   // u_total, img_total: words
        for (size_t m = 0; m < G; m++) {
            Member& x = mem[m];
            x.idx = groups[g].first + m;
            x.n = items[x.idx].claims->size();
            x.nw = nw_of(*items[x.idx].claims);
            x.job0 = jobs_total; x.claim0 = claims_total; x.u = u_total; x.img = img_total;
            x.u_words = 4 * C * (x.n + 1);
            x.len = pcs_opening_bytes(sh, x.n, Q);
            jobs_total += x.n + 1; claims_total += x.n; u_total += x.u_words; img_total += x.len / 8;
        }
        const size_t mem_at = 0, jobs_at = align32(G * sizeof(BnObMember)), claims_at = jobs_at + align32(jobs_total * sizeof(BnObJob));
        size_t at = claims_at + align32(claims_total * sizeof(BnObClaim));
        for (Member& x : mem) {   // (elements of 32 bytes from a multiple of 32 on)
            x.y_at = at;
            x.z_at = x.y_at + x.n * sizeof(Fr);
            x.w_at = x.z_at + x.n * (size_t)sh.c * sizeof(Fr);
            at = x.w_at + x.nw * sizeof(Fr);
        }
        const size_t stage_bytes = std::max<size_t>(at, 32);
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
                const pcs::Commitment& cm = *items[x.idx].cm;
                const std::vector<PcsClaim>& claims = *items[x.idx].claims;
                const Fr* rows = reinterpret_cast<const Fr*>(cm.d_rows);
                x.tr = pcs_start_transcript(sh, cm.root(), claims, Q);
                const std::vector<Fr> rho = pcs_rho_powers(pcs_squeeze(x.tr), R);
                BnObMember* hm = reinterpret_cast<BnObMember*>(h_stage + mem_at) + mq;
                hm->M = reinterpret_cast<const Fr*>(cm.d_M); hm->img = x.img; hm->u = x.u; hm->u_words = x.u_words;
                BnObJob* hd = reinterpret_cast<BnObJob*>(h_stage + jobs_at) + x.job0;
                BnObClaim* hc = reinterpret_cast<BnObClaim*>(h_stage + claims_at) + x.claim0;
                Fr* hy = reinterpret_cast<Fr*>(h_stage + x.y_at);
                Fr* hz = reinterpret_cast<Fr*>(h_stage + x.z_at);
                Fr* hw = reinterpret_cast<Fr*>(h_stage + x.w_at);
                hd[0].src = rows; hd[0].nrows = R; hd[0].w_at = x.w_at; hd[0].u_at = x.u / 4;
                memcpy(hw, rho.data(), R * sizeof(Fr));
                size_t off = R;
                for (size_t i = 0; i < x.n; i++) {
                    const PcsClaim& cl = claims[i];
                    const std::vector<Fr> w = pcs_eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
                    hd[i + 1].src = rows + (sh.off[cl.table] << sh.c); hd[i + 1].nrows = w.size(); hd[i + 1].w_at = x.w_at + off * sizeof(Fr);
                    hd[i + 1].u_at = x.u / 4 + (i + 1) * C;
                    memcpy(hw + off, w.data(), w.size() * sizeof(Fr));
                    off += w.size();
                    hy[i] = cl.value;
                    for (int b = 0; b < sh.c; b++) hz[i * (size_t)sh.c + b] = fr_to_mont(cl.point[b]);
                    hc[i].u_at = hd[i + 1].u_at; hc[i].z_at = x.z_at + i * (size_t)sh.c * sizeof(Fr); hc[i].y_at = x.y_at + i * sizeof(Fr);
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
        const BnObMember* d_mem = reinterpret_cast<const BnObMember*>(d_stage + mem_at);
        const unsigned cb = bnpcs_blocks(C);
        if (jobs_total * cb > 0x7fffffffull) throw Error(who + ": a group of " + std::to_string(G) + " openings has too many row combinations for one launch: lower verify_batch_group");
        hipc(hipMemcpyAsync(d_stage, h_stage, stage_bytes, hipMemcpyHostToDevice, st), "upload claims");
        hipc(hipMemsetAsync(d_cells, 0xff, G * 8, st), "memset");
        size_t nw_total = 0;
        for (const Member& x : mem) nw_total += x.nw;
        ctx->prof_begin(cls, (double)nw_total * C * 32 + (double)u_total * 8);
        k_bnpcsob_combine<<<(unsigned)(jobs_total * cb), BNPCS_TPB, 0, st>>>(sh.c, cb, reinterpret_cast<const BnObJob*>(d_stage + jobs_at), d_stage, reinterpret_cast<Fr*>(d_u));
        ctx->prof_end();
        if (claims_total) {
            ctx->prof_begin(cls, (double)claims_total * C * 32);
            k_bnpcsob_eval<<<(unsigned)claims_total, BNPCS_TPB, 0, st>>>(reinterpret_cast<const BnObClaim*>(d_stage + claims_at), sh.c, reinterpret_cast<const Fr*>(d_u), d_stage, d_cells);
            ctx->prof_end();
        }
        ctx->prof_begin(cls, (double)u_total * 16);
        k_bnpcsob_emit<<<(unsigned)std::min<size_t>(bnpcs_blocks(u_total), 4096), BNPCS_TPB, 0, st>>>(d_mem, (unsigned)G, u_total, d_u, d_img);
        ctx->prof_end();
        hipc(hipMemcpyAsync(h_out + hu_at, d_u, u_total * 8, hipMemcpyDeviceToHost, st), "download combinations");
        hipc(hipMemcpyAsync(h_out + hcell_at, d_cells, G * 8, hipMemcpyDeviceToHost, st), "download evaluation checks");
        hipc(hipStreamSynchronize(st), (who + ": sync").c_str());
        hipc(hipGetLastError(), (who + ": launch").c_str());
        const double t2 = omp_get_wtime();
        // the host's share: every member's u_i into its transcript, its column indices out of it, one member a thread
        hj.assign(G * Q + G, 0);
        size_t active = 0;
        for (size_t m = 0; m < G; m++) {
            mem[m].refused = h_cells[m] != BNPCSV_NONE;
            hj[G * Q + m] = mem[m].refused ? 0 : 1;
            active += mem[m].refused ? 0 : 1;
        }
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            if (x.refused) continue;
            try {
                pcs_absorb(x.tr, reinterpret_cast<const Fr*>(h_u + x.u), x.u_words / 4);
                const std::vector<size_t> js = pcs_squeeze_indices(x.tr, N, Q);
                for (size_t q = 0; q < Q; q++) hj[(size_t)mq * Q + q] = js[q];
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        const double t3 = omp_get_wtime();
        if (active) {
            if (Q) {
                hipc(hipMemcpyAsync(d_js, hj.data(), hj.size() * 8, hipMemcpyHostToDevice, st), "upload column indices");
                ctx->prof_begin(cls, (double)active * Q * R * 64);
                k_bnpcsob_gather<<<bnpcs_blocks(G * Q * R), BNPCS_TPB, 0, st>>>(d_mem, G, Q, R, N, q_words, d_js, d_img);
                ctx->prof_end();
            }
            hipc(hipMemcpyAsync(h_img, d_img, img_total * 8, hipMemcpyDeviceToHost, st), "download openings");
            hipc(hipStreamSynchronize(st), (who + ": sync").c_str());
            hipc(hipGetLastError(), (who + ": launch").c_str());
        }
        ctx->prof_collect();
        const double t4 = omp_get_wtime();
        // the siblings from each handle's tree into the gaps; a refused member's reason
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                pcs::Opened& out = res[x.idx];
                const pcs::Commitment& cm = *items[x.idx].cm;
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
                    uint8_t* sib = out.bytes.data() + 8 * (x.u_words + q * q_words + 4 * R);
                    size_t idx = (size_t)hj[(size_t)mq * Q + q];
                    for (int l = 0; l < depth; l++, idx >>= 1) memcpy(sib + 32 * l, cm.node(l, idx ^ 1), 32);
                }
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
        if (times)
            fprintf(stderr, "[hg pcs] bn254 open group %zu of %zu members: transcripts and weights %.2f ms, combine, checks and u back %.2f, hash %.2f, gather and images back %.2f, "
                            "siblings %.2f\n", g, G, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (omp_get_wtime() - t4) * 1e3);
    }
    return res;
}
