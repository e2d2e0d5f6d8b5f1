// BfvEncrypt::prove over bn256::Fr (BASELINE config 5 family) - included by bn254.hip (behind its kernels, ahead of its Lasso node), inside namespace hg::bn.
//   witness generation = Circuit::evaluate over Fr   [REF bfv-gkr/src/sk_encryption_circuit.rs:434-442]
//   output claim, gkr::prove_gkr walk                [REF sk_encryption_circuit.rs:444-457]
//   VanillaNode (Libra) / FftNode (zkCNN) claim reductions: external `gkr` crate, conventions G1-G4 / C1-C4 of DESIGN.md 2
//   LassoNode: lasso_prove_bn254 (above)
// Structure: one node at a time on one stream, everything enqueued back to back (the challenges are message-independent and no
// kernel argument depends on a value read back by the host), scalar results in the host-mapped result buffer, one synchronisation
// for all Vanilla / FFT nodes, then the transcript is replayed in protocol order (BnProver); the sum-checks of all nodes run
// round-synchronised in shared launches (prodsum_flush). The circuit wiring (CSR tables in HBM) is shared with the
// Goldilocks prover key - gate constants are non-negative integers in both fields.

struct DevPool {  // device buffers of one prove from the context's bump arena; a node releases its scope when it is done
    hg_ctx* ctx;
    std::vector<std::vector<size_t>> marks;
    explicit DevPool(hg_ctx* c) : ctx(c) { marks.push_back(ctx->arena_mark()); }
    template <typename T> T* get(size_t n) { return static_cast<T*>(ctx->alloc(std::max<size_t>(n, 1) * sizeof(T))); }
    size_t mark() { marks.push_back(ctx->arena_mark()); return marks.size() - 1; }
    void release_from(size_t m) { ctx->arena_rewind(marks.at(m)); marks.resize(m); }
    ~DevPool() { if (!marks.empty()) ctx->arena_rewind(marks[0]); }
};
static unsigned grid_of(size_t n) { return (unsigned)((n + 255) / 256); }

// z held in the Goldilocks form (negative z as p - |z|, |z| < 2^62) -> z in Fr, Montgomery form
__global__ void k_bn_lift_signed(const u64* __restrict__ in, Fr* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 v = in[i];
    out[i] = v < (1ULL << 63) ? fr_to_mont(fr_make(v, 0, 0, 0)) : fr_sub(fr_zero(), fr_to_mont(fr_make(GL_P - v, 0, 0, 0)));
}
__device__ __forceinline__ Fr fr_lift(u64 c) { return fr_to_mont(fr_make(c, 0, 0, 0)); }
// every input table of a witness in one launch (blockIdx.y = table)
struct LiftJobs { const u64* src[64]; Fr* dst[64]; size_t len[64]; int n, pad; };
__global__ __launch_bounds__(256) void k_bn_lift_jobs(LiftJobs J) {
    const u64* __restrict__ in = J.src[blockIdx.y];
    Fr* __restrict__ out = J.dst[blockIdx.y];
    const size_t n = J.len[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const u64 v = in[i];
        out[i] = v < (1ULL << 63) ? fr_to_mont(fr_make(v, 0, 0, 0)) : fr_sub(fr_zero(), fr_to_mont(fr_make(GL_P - v, 0, 0, 0)));
    }
}
// The same for tables that lie in device memory already (hg_prove_encryptions_bn254: the derivation wrote them): a lane reads two words
// as one 16-byte load and writes two whole elements. A zero word - every word the layout pads with, half of most tables - is stored as
// the zero element without the Montgomery product (a wave of padding skips the branch). Tables: 16-byte aligned, even length.
__device__ __forceinline__ Fr fr_lift_signed(u64 v) {
    Fr r = fr_zero();
    if (v) r = v < (1ULL << 63) ? fr_to_mont(fr_make(v, 0, 0, 0)) : fr_sub(fr_zero(), fr_to_mont(fr_make(GL_P - v, 0, 0, 0)));
    return r;
}
__global__ __launch_bounds__(256) void k_bn_lift_pairs(LiftJobs J) {
    const ulonglong2* __restrict__ in = reinterpret_cast<const ulonglong2*>(J.src[blockIdx.y]);
    Fr* __restrict__ out = J.dst[blockIdx.y];
    const size_t half = J.len[blockIdx.y] / 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < half; i += (size_t)gridDim.x * 256) {
        const ulonglong2 v = in[i];
        out[2 * i] = fr_lift_signed(v.x);
        out[2 * i + 1] = fr_lift_signed(v.y);
    }
}

struct BnPtrs { const Fr* p[dev::PS_MAX_PAIRS]; };
// Vanilla node evaluation over Fr (same gate-major wiring as k_gate_eval)
__global__ __launch_bounds__(BN_TPB) void k_bn_gate_eval(dev::EvalNode N, BnPtrs in, Fr* __restrict__ out) {
    const size_t total = (size_t)1 << (N.log2_G + N.log2_R);
    const size_t gmask = ((size_t)1 << N.log2_G) - 1;
    for (size_t idx = (size_t)blockIdx.x * BN_TPB + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BN_TPB) {
        const size_t g = idx & gmask, rep = idx >> N.log2_G;
        Fr acc = fr_zero();
        if (g < N.num_gates) {
            if (N.w0) acc = fr_lift(N.w0[g]);
            if (N.lptr)
                for (u32 e = N.lptr[g]; e < N.lptr[g + 1]; e++) {
                    const Fr x = in.p[N.lin_in[e]][(rep << N.log2_S) + N.lin_j[e]];
                    const u64 c = N.lcoef[e];
                    acc = fr_add(acc, c == 1 ? x : fr_mul(fr_lift(c), x));
                }
            if (N.mptr)
                for (u32 e = N.mptr[g]; e < N.mptr[g + 1]; e++) {
                    const Fr x = in.p[N.mi0[e]][(rep << N.log2_S) + N.mj0[e]];
                    const Fr y = in.p[N.mi1[e]][(rep << N.log2_S) + N.mj1[e]];
                    const u64 c = N.mcoef[e];
                    const Fr pr = fr_mul(x, y);
                    acc = fr_add(acc, c == 1 ? pr : fr_mul(fr_lift(c), pr));
                }
        }
        out[idx] = acc;
    }
}

// in place on `a` (bit-reversed copy in `tmp`, result back in `a`): natural order in and out
static void ntt_dev(hipStream_t st, Fr* a, Fr* tmp, const Fr* W, int log2n, bool inverse, size_t batch) {  // W[i] = w^i, i < n
    const size_t n = (size_t)1 << log2n, total = n * batch;
    if (ntt4_dev(st, a, tmp, W, log2n, inverse, inverse ? fr_inv(fr_small((u64)n)) : fr_one_mont(), batch)) return;
    k_bn_bitrev<<<grid_of(total), 256, 0, st>>>(a, tmp, log2n, total);
    for (int s = 0; s < log2n; s++) k_bn_ntt_stage<<<grid_of(total / 2), 256, 0, st>>>(tmp, W, log2n, s, total / 2);
    if (inverse) k_bn_scale<<<grid_of(total), 256, 0, st>>>(tmp, fr_inv(fr_small((u64)n)), total);
    hipc(hipMemcpyAsync(a, tmp, total * sizeof(Fr), hipMemcpyDeviceToDevice, st), "ntt copy");
}

// the table over m <= 8 variables (at most 256 entries) in one workgroup
struct EqHead { Fr r[8]; };
__global__ __launch_bounds__(256) void k_bn_eq_head(Fr* __restrict__ eq, EqHead h, int m) {
    // entry x = prod_b (x_b ? r_b : 1 - r_b): every thread multiplies its own eight factors as a depth-3 tree (absent variables
    // contribute the factor one, which changes nothing in the field)
    const int x = threadIdx.x;
    if (x >= (1 << m)) return;
    const Fr one = fr_one_mont();
    Fr f[8];
#pragma unroll
    for (int b = 0; b < 8; b++) f[b] = b < m ? ((x >> b) & 1 ? h.r[b] : fr_sub(one, h.r[b])) : one;
    const Fr p01 = fr_mul_wide(f[0], f[1]), p23 = fr_mul_wide(f[2], f[3]), p45 = fr_mul_wide(f[4], f[5]), p67 = fr_mul_wide(f[6], f[7]);
    eq[x] = fr_mul_wide(fr_mul_wide(p01, p23), fr_mul_wide(p45, p67));
}
// eq[x] = lo[x mod 256] * hi[x div 256]: the table over n variables as the outer product of the tables over the low 8 and the
// remaining variables (one product per entry; the same field element as the doubling recursion, products being exact)
__global__ void k_bn_eq_outer(Fr* __restrict__ eq, const Fr* __restrict__ lo, const Fr* __restrict__ hi, size_t total) {
    size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < total) eq[x] = fr_mul_wide(lo[x & 255], hi[x >> 8]);
}
static size_t eq_scratch_len(int n) { return n <= 8 ? 1 : ((size_t)1 << (n - 7)) + 1024; }
// scratch: eq_scratch_len(n) elements
static void build_eq_dev(hipStream_t st, Fr* eq, const Fr* pt_canon, int n, Fr* scratch) {
    if (n <= 8) {
        EqHead h;
        for (int i = 0; i < 8; i++) h.r[i] = i < n ? fr_to_mont(pt_canon[i]) : fr_zero();
        k_bn_eq_head<<<1, 256, 0, st>>>(eq, h, n);
        return;
    }
    Fr* lo = scratch;
    Fr* hi = scratch + 256;
    build_eq_dev(st, lo, pt_canon, 8, nullptr);
    build_eq_dev(st, hi, pt_canon + 8, n - 8, hi + ((size_t)1 << (n - 8)));
    k_bn_eq_outer<<<grid_of((size_t)1 << n), 256, 0, st>>>(eq, lo, hi, (size_t)1 << n);
}

// One round of prove_sum_check for g = sum_i a_i b_i (Libra / zkCNN reductions): tables by pointer (round 0 reads the node
// inputs where they lie), folded tables written contiguously (table t at out + t * half); the dot product over the pairs is
// accumulated unreduced (column accumulators) and reduced once per pair index. blockIdx.z = v: 0 evaluates g(0) and writes the
// folds of the a tables, 1 evaluates g(2) and writes the folds of the b tables (half the dependent chain per thread); small
// rounds deal the pairs round-robin to gy thread groups (see k_bn_gp_round_jobs).
// The same round for many independent sum-checks in one launch (blockIdx.y = job; a job uses gx * gy of the gridDim.x workgroups).
// No node depends on another node's device results (claims carry challenges as points; their values only meet on the host), so
// the rounds of all queued Libra / zkCNN reductions run round-synchronised: launch k is round k of every job.
// (PsJobDev and k_bn_ps_round_jobs live in bn254.hip: the Lasso node's collation sum-check uses them too)
// results of one sum-check in the host-mapped result buffer (canonical): per round g(0), g(2); the 2 npairs fully folded
// values. Valid on the host after the next res_sync; `fin.dev` can be read by later kernels on the stream.
struct PsOut { ResRef sums, fin; int nmain; };   // nmain: rounds done by the shared launches (the tail workgroup does the rest)
struct PsPlan {
    std::vector<const Fr*> a, b;
    int nv;
    std::vector<Fr> rs;  // canonical
    Fr *buf0, *buf1, *part, *tbuf;
    PsOut out;
    bool shared_b = false;   // every pair multiplies the same b table (k_bn_ps_round_jobs)
    size_t win_lo = 0, win_hi = 0;   // single-pair job whose b table is zero outside the entries [win_lo, win_hi) (win_hi = 0: no window)
};
// queue one sum-check: buffers and result slots now, launches in prodsum_flush
static PsOut prodsum_defer(DevPool& pool, std::vector<PsPlan>& queue, const std::vector<const Fr*>& a, const std::vector<const Fr*>& b, int nv,
                           const std::vector<Fr>& rs_canon, size_t win_lo = 0, size_t win_hi = 0) {
    const int npairs = (int)a.size();
    if (npairs < 1 || npairs > dev::PS_MAX_PAIRS || nv < 2 || nv > 32 || b.size() != a.size()) throw Error("bn254 prodsum: bad shape");
    const size_t N = (size_t)1 << nv, ntab = 2 * (size_t)npairs;
    PsPlan p;
    p.a = a; p.b = b; p.nv = nv; p.rs = rs_canon;
    p.buf0 = pool.get<Fr>(ntab * (N / 2));
    p.buf1 = pool.get<Fr>(ntab * std::max<size_t>(N / 4, 1));
    p.part = pool.get<Fr>((size_t)nv * BN_PART_STRIDE * 2);
    p.tbuf = pool.get<Fr>(2 * ntab * (size_t)BN_TAIL_HALF);
    p.out.sums = res_slots(pool.ctx, (size_t)nv * 2);
    p.out.fin = res_slots(pool.ctx, ntab);
    p.out.nmain = ps_nmain(nv);
    p.shared_b = npairs > 1;
    for (int i = 1; i < npairs; i++) p.shared_b = p.shared_b && b[i] == b[0];
    if (npairs == 1 && win_hi > win_lo && win_hi - win_lo < N) {
        // usable when the window stays a run of whole pairs in every shared-launch round (aligned power-of-two slices do)
        bool ok = true;
        for (int rd = 0; rd < p.out.nmain && ok; rd++) {
            const size_t elo = win_lo >> rd, ehi = (win_hi + (((size_t)1 << rd) - 1)) >> rd;
            ok = !(elo & 1) && !(ehi & 1) && ehi > elo;
        }
        if (ok) { p.win_lo = win_lo; p.win_hi = win_hi; }
    }
    queue.push_back(p);
    return p.out;
}
// all queued sum-checks, round-synchronised: one launch per round index, one reduce launch, one launch for all tails.
// `keep`: host staging that must outlive the asynchronous uploads
static void prodsum_flush(hipStream_t st, DevPool& pool, std::vector<PsPlan>& queue, std::vector<std::shared_ptr<void>>& keep) {
    if (queue.empty()) return;
    const size_t nj = queue.size();
    int max_main = 0;
    std::vector<int> nmain(nj);
    for (size_t q = 0; q < nj; q++) {
        const int m = queue[q].out.nmain;
        nmain[q] = m;
        max_main = std::max(max_main, m);
    }
    auto descs = std::make_shared<std::vector<PsJobDev>>();
    auto reds = std::make_shared<std::vector<RedJobDev>>(nj);
    auto tails = std::make_shared<std::vector<TailJobDev>>(nj);
    std::vector<size_t> off(max_main + 1, 0), map_off(max_main, 0);
    std::vector<int> total_blocks(max_main, 0);
    std::vector<unsigned short> jobmap;   // per round: (workgroup >> 4) -> job of the round
    for (int rd = 0; rd < max_main; rd++) {
        off[rd] = descs->size();
        map_off[rd] = jobmap.size();
        for (size_t q = 0; q < nj; q++) {
            const PsPlan& p = queue[q];
            if (rd >= nmain[q]) continue;
            const size_t N = (size_t)1 << p.nv, half = N >> (rd + 1), ntab = 2 * p.a.size();
            PsJobDev d;
            memset(&d, 0, sizeof(d));
            Fr* outb = (rd & 1) ? p.buf1 : p.buf0;          // rounds alternate between the two buffers
            const Fr* inb = (rd & 1) ? p.buf0 : p.buf1;     // previous round's output (rd >= 1)
            for (size_t t = 0; t < ntab; t++) d.t[t] = rd == 0 ? ((t & 1) ? p.b[t / 2] : p.a[t / 2]) : inb + ((t & 1) && p.shared_b ? 1 : t) * (2 * half);
            d.pad = (p.shared_b ? 1 : 0) | (p.shared_b && rd == nmain[q] - 1 ? 2 : 0);
            if (p.win_hi) {
                const size_t elo = p.win_lo >> rd, ehi = (p.win_hi + (((size_t)1 << rd) - 1)) >> rd;
                d.wlo = elo >> 1; d.whi = ehi >> 1;
                d.pad |= 4 | (rd == nmain[q] - 1 ? 8 : 0);
            }
            d.out = outb;
            d.part = p.part + (size_t)rd * BN_PART_STRIDE * 2;
            d.r = fr_to_mont(p.rs[rd]);
            fold_consts(d.r, &d.fk);
            d.half = half;
            d.npairs = (int)p.a.size();
            const RoundGrid g = round_grid(half, d.npairs);
            d.gx = g.gx; d.gy = g.gy;
            (*reds)[q].n[rd] = g.blocks();
            const int wgs = 2 * ((g.blocks() + 7) / 8 * 8);   // both workgroup sets, whole groups of eight (one per XCD)
            d.wg0 = total_blocks[rd];
            total_blocks[rd] += wgs;
            jobmap.insert(jobmap.end(), (size_t)wgs / 16, (unsigned short)(descs->size() - off[rd]));
            descs->push_back(d);
        }
    }
    off[max_main] = descs->size();
    for (size_t q = 0; q < nj; q++) {
        const PsPlan& p = queue[q];
        const size_t N = (size_t)1 << p.nv;
        RedJobDev& r = (*reds)[q];
        r.part = p.part; r.out = p.out.sums.dev; r.nrounds = nmain[q]; r.pad = 0;
        TailJobDev& t = (*tails)[q];
        memset(&t, 0, sizeof(t));
        const int m = nmain[q];
        t.in = ((m - 1) & 1) ? p.buf1 : p.buf0;   // output of the last main round
        t.buf = p.tbuf;
        t.sums_out = p.out.sums.dev + (size_t)m * 2;
        t.fin_out = p.out.fin.dev;
        for (int k = 0; k < BN_TAIL_ROUNDS; k++) t.rs.r[k] = k < p.nv - m ? fr_to_mont(p.rs[m + k]) : fr_zero();
        t.npairs = (int)p.a.size(); t.half0 = (int)(N >> (m + 1)); t.nrounds = p.nv - m;
    }
    {   // the folds' matrices (bn254_mfma.hpp), one per (job, round): built on the device from the descriptors' challenges
        MfA* mfa = pool.get<MfA>(descs->size());
        for (size_t i = 0; i < descs->size(); i++) (*descs)[i].mf = mfa + i;
    }
    if (hg_debug("bnplan")) {   // the descriptors as they are staged, in launch order (read at every call: the tests switch it per case)
        size_t i = 0;
        for (int rd = 0; rd < max_main; rd++)
            for (size_t q = 0; q < nj; q++) {
                if (rd >= nmain[q]) continue;
                const PsJobDev& d = (*descs)[i++];
                const bool mf = d.mf && (d.half & 63) == 0 && (!(d.pad & 4) || ((d.wlo | d.whi) & 63) == 0);   // as k_bn_ps_round_jobs decides
                char win[48] = "-";
                if (d.pad & 4) snprintf(win, sizeof(win), "%llu..%llu", d.wlo, d.whi);
                fprintf(stderr, "[hg bnplan] ps job=%zu rd=%d half=%llu npairs=%d gx=%d gy=%d mf=%d shared=%d rep=%d win=%s zero=%d\n", q, rd, d.half, d.npairs, d.gx, d.gy,
                        mf ? 1 : 0, d.pad & 1, (d.pad >> 1) & 1, win, (d.pad >> 3) & 1);
            }
        for (size_t q = 0; q < nj; q++)
            fprintf(stderr, "[hg bnplan] ps tail job=%zu half0=%d rounds=%d npairs=%d\n", q, (*tails)[q].half0, (*tails)[q].nrounds, (*tails)[q].npairs);
    }
    const PsJobDev* d_descs = bn_stage(pool.ctx, descs->data(), descs->size());
    const unsigned short* d_map = bn_stage(pool.ctx, jobmap.data(), jobmap.size());
    const RedJobDev* d_reds = bn_stage(pool.ctx, reds->data(), nj);
    const TailJobDev* d_tails = bn_stage(pool.ctx, tails->data(), nj);
    bn_flush(pool.ctx, st);
    (void)keep;
    k_bn_mf_consts<PsJobDev><<<(unsigned)descs->size(), 64, 0, st>>>(d_descs);
    for (int rd = 0; rd < max_main; rd++)
        k_bn_ps_round_jobs<<<(unsigned)total_blocks[rd], BN_TPB, 0, st>>>(d_descs + off[rd], d_map + map_off[rd]);
    k_bn_reduce_jobs<<<dim3(32, (unsigned)nj), BN_TPB, 0, st>>>(d_reds, 2);
    k_bn_tail_jobs<BN_PRODSUM><<<(unsigned)nj, 2 * BN_TPB, 0, st>>>(d_tails);
    queue.clear();
}

// hg_prodsum_jobs_bn254: the prover's PRODSUM launches on caller tables, for kernel-level tests. Every job is queued with
// prodsum_defer and the batch is run by ONE prodsum_flush, so it takes the launches a prove takes (jobmap / wg0 packing of jobs of
// different sizes, shared-b and windowed forms, one tail workgroup per job). tables: a_0, b_0, a_1, b_1, .. of every job in job order
// (host, canonical). A job of several pairs whose b pointers are all the same host pointer uploads b once (the shared-b form).
void prodsum_jobs_bn254(hg_ctx* ctx, size_t njobs, const size_t* nv, const size_t* npairs, const u64* const* tables, const size_t* win, size_t chain_skip,
                        u64* sums4, u64* evals4) {
    const char* const who = "hg_prodsum_jobs_bn254: ";
    if (!nv || !npairs || !tables || !win || !sums4 || !evals4) throw Error(std::string(who) + "null argument");
    if (njobs < 1 || njobs > 64) throw Error(std::string(who) + "njobs must be 1 .. 64");
    size_t total_nv = 0;
    for (size_t q = 0; q < njobs; q++) {
        if (nv[q] < 2 || nv[q] > 32) throw Error(std::string(who) + "nv must be 2 .. 32 (job " + std::to_string(q) + ")");
        if (npairs[q] < 1 || npairs[q] > (size_t)dev::PS_MAX_PAIRS) throw Error(std::string(who) + "npairs must be 1 .. " + std::to_string(dev::PS_MAX_PAIRS) + " (job " + std::to_string(q) + ")");
        total_nv += nv[q];
    }
    for (size_t q = 0, t0 = 0; q < njobs; t0 += 2 * npairs[q], q++) {   // everything is checked before anything is uploaded or launched
        const size_t N = (size_t)1 << nv[q], wlo = win[2 * q], whi = win[2 * q + 1];
        const bool windowed = wlo || whi;
        if (windowed && npairs[q] != 1) throw Error(std::string(who) + "a window needs a job of one pair (job " + std::to_string(q) + ")");
        if (windowed && (wlo >= whi || whi > N)) throw Error(std::string(who) + "bad window (job " + std::to_string(q) + ")");
        for (size_t t = 0; t < 2 * npairs[q]; t++) {
            const u64* tab = tables[t0 + t];
            if (!tab) throw Error(std::string(who) + "null table (job " + std::to_string(q) + ")");
            if (t >= 3 && (t & 1) && tab == tables[t0 + 1]) continue;   // the b table of pair 0 again: checked once
            for (size_t i = 0; i < N; i++) {
                Fr v;
                memcpy(v.l, tab + 4 * i, 32);
                if (fr_geq_p(v)) throw Error(std::string(who) + "table entry not below r (job " + std::to_string(q) + ", table " + std::to_string(t) + ")");
                if (windowed && t == 1 && (i < wlo || i >= whi) && (v.l[0] | v.l[1] | v.l[2] | v.l[3]))
                    throw Error(std::string(who) + "b is not zero outside its window (job " + std::to_string(q) + ", entry " + std::to_string(i) + ")");
            }
        }
    }
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    ctx->arena_reset();
    DevPool pool(ctx);
    const std::vector<Fr> chain = challenge_chain_bn254(chain_skip + total_nv);
    std::vector<PsPlan> queue;
    std::vector<PsOut> outs;
    std::vector<std::shared_ptr<void>> keep;
    auto upload = [&](const u64* src, size_t N) {
        Fr* d = pool.get<Fr>(N);
        hipc(hipMemcpyAsync(d, src, N * sizeof(Fr), hipMemcpyHostToDevice, st), "upload table");
        k_bn_to_mont<<<grid_of(N), 256, 0, st>>>(d, N);
        return (const Fr*)d;
    };
    for (size_t q = 0, t0 = 0, c0 = chain_skip; q < njobs; t0 += 2 * npairs[q], c0 += nv[q], q++) {
        const size_t N = (size_t)1 << nv[q], np = npairs[q];
        bool same_b = np > 1;
        for (size_t i = 1; i < np; i++) same_b = same_b && tables[t0 + 2 * i + 1] == tables[t0 + 1];
        std::vector<const Fr*> a(np), b(np);
        for (size_t i = 0; i < np; i++) {
            a[i] = upload(tables[t0 + 2 * i], N);
            b[i] = same_b && i ? b[0] : upload(tables[t0 + 2 * i + 1], N);
        }
        const std::vector<Fr> rs(chain.begin() + c0, chain.begin() + c0 + nv[q]);
        outs.push_back(prodsum_defer(pool, queue, a, b, (int)nv[q], rs, win[2 * q], win[2 * q + 1]));
    }
    prodsum_flush(st, pool, queue, keep);
    res_sync(ctx, st, "hg_prodsum_jobs_bn254: sync");
    for (size_t q = 0; q < njobs; q++) {
        memcpy(sums4, outs[q].sums.host, nv[q] * 2 * sizeof(Fr));
        memcpy(evals4, outs[q].fin.host, 2 * npairs[q] * sizeof(Fr));
        sums4 += nv[q] * 2 * 4; evals4 += 2 * npairs[q] * 4;
    }
}

// sum over reps and constant gates of eqc[rep*G + gate] * c -> per-workgroup partials
__global__ __launch_bounds__(BN_TPB) void k_bn_const_sum(const u32* __restrict__ gate, const u64* __restrict__ coef, size_t nterms, const Fr* __restrict__ eqc,
                                                         int log2_G, int log2_R, Fr* __restrict__ partials) {
    __shared__ Fr sm[BN_TPB];
    const size_t total = nterms << log2_R;
    Fr acc = fr_zero();
    for (size_t idx = (size_t)blockIdx.x * BN_TPB + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BN_TPB) {
        const size_t t = idx % nterms, rep = idx / nterms;
        acc = fr_add(acc, fr_mul(eqc[(rep << log2_G) + gate[t]], fr_lift(coef[t])));
    }
    Fr s = block_sum_fr(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// Libra phase-1 bookkeeping: T[rep*S + x] = sum_lin eqc[rep*G+gate] c + sum_mul eqc[rep*G+gate] c in_other[rep*S + j1]
__global__ __launch_bounds__(BN_TPB) void k_bn_gather_T(dev::CsrLin lin, dev::CsrMul mul, BnPtrs in_vals, const Fr* __restrict__ eqc, int log2_S, int log2_G,
                                                        int log2_R, Fr* __restrict__ T) {
    const size_t total = (size_t)1 << (log2_S + log2_R);
    const size_t smask = ((size_t)1 << log2_S) - 1;
    for (size_t idx = (size_t)blockIdx.x * BN_TPB + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BN_TPB) {
        const size_t x = idx & smask, rep = idx >> log2_S;
        const Fr* eq_rep = eqc + (rep << log2_G);
        Fr acc = fr_zero();
        if (lin.ptr)
            for (u32 e = lin.ptr[x]; e < lin.ptr[x + 1]; e++) {
                const Fr q = eq_rep[lin.gate[e]];
                const u64 c = lin.coef[e];
                acc = fr_add(acc, c == 1 ? q : fr_mul(q, fr_lift(c)));
            }
        if (mul.ptr)
            for (u32 e = mul.ptr[x]; e < mul.ptr[x + 1]; e++) {
                Fr q = eq_rep[mul.gate[e]];
                const u64 c = mul.coef[e];
                if (c != 1) q = fr_mul(q, fr_lift(c));
                acc = fr_add(acc, fr_mul(q, in_vals.p[mul.other_in[e]][(rep << log2_S) + mul.other_j[e]]));
            }
        T[idx] = acc;
    }
}
// Libra phase-2 bookkeeping: B[rep*S + y] = sum_mulR eqc[rep*G+gate] c eqx[rep*S + j0] u[i0]
// u[i0] = in_i0(r_x) is read where phase 1 left it: canonical, at fin[slot[i0]] of the result buffer (no host round trip)
struct BnU { int slot[dev::PS_MAX_PAIRS]; };
__global__ __launch_bounds__(BN_TPB) void k_bn_gather_B(dev::CsrMul m, const Fr* __restrict__ eqc, const Fr* __restrict__ eqx, const Fr* __restrict__ fin,
                                                        BnU us, int arity, int log2_S, int log2_G, int log2_R, Fr* __restrict__ B) {
    __shared__ Fr u_sm[dev::PS_MAX_PAIRS];
    if ((int)threadIdx.x < arity) u_sm[threadIdx.x] = us.slot[threadIdx.x] >= 0 ? fr_to_mont(fin[us.slot[threadIdx.x]]) : fr_zero();
    __syncthreads();
    const size_t total = (size_t)1 << (log2_S + log2_R);
    const size_t smask = ((size_t)1 << log2_S) - 1;
    for (size_t idx = (size_t)blockIdx.x * BN_TPB + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BN_TPB) {
        const size_t y = idx & smask, rep = idx >> log2_S;
        Fr acc = fr_zero();
        for (u32 e = m.ptr[y]; e < m.ptr[y + 1]; e++) {
            Fr q = eqc[(rep << log2_G) + m.gate[e]];
            const u64 c = m.coef[e];
            if (c != 1) q = fr_mul(q, fr_lift(c));
            q = fr_mul(q, eqx[(rep << log2_S) + m.other_j[e]]);
            acc = fr_add(acc, fr_mul(q, u_sm[m.other_in[e]]));
        }
        B[idx] = acc;
    }
}
// zkCNN DFT-row table: F(x) (+)= coef * prod_b (1 + r_b (W[(x << b) mod N] - 1)), W[i] = w^i, coef = alpha * scale. The factor b only
// depends on x mod 2^(L-b): the factors b in [4, 8) and b >= 8 come from two small tables (k_bn_fft_part: 2^(L-4) and 2^(L-8)
// entries), so an output costs 4 direct factors and two lookups - 10 products instead of 32 at L = 16.
struct BnPoint { Fr r[28]; };
__device__ __forceinline__ Fr bn_fft_factor(const Fr* __restrict__ W, size_t N, const Fr& rb, size_t x, int b, const Fr& one) {
    return fr_add(one, fr_mul_wide(rb, fr_sub(W[(x << b) & (N - 1)], one)));
}
// T[y] = prod_{b_lo <= b < b_hi} factor_b(y), y < 2^(L - b_lo)
__global__ void k_bn_fft_part(Fr* __restrict__ T, const Fr* __restrict__ W, int L, BnPoint pt, int b_lo, int b_hi) {
    const size_t N = (size_t)1 << L, n = (size_t)1 << (L - b_lo);
    size_t y = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= n) return;
    const Fr one = fr_one_mont();
    Fr acc = one;
    for (int b = b_lo; b < b_hi; b++) acc = fr_mul_wide(acc, bn_fft_factor(W, N, pt.r[b], y, b, one));
    T[y] = acc;
}

// ---- the same bookkeeping kernels over job arrays: one launch for all nodes (grid.y / blockIdx.x = job) ------------------------
// A prove has ~65 Vanilla / FFT nodes with up to 17 claims each; launched per node and claim their bookkeeping was ~600 launches of
// 5-20 us that the stream ran one after the other (141 single-workgroup k_bn_eq_head alone: 1.6 ms).
struct EqHeadJob { Fr* eq; EqHead h; int m, pad; };
__global__ __launch_bounds__(256) void k_bn_eq_head_jobs(const EqHeadJob* __restrict__ jobs) {
    const EqHeadJob& J = jobs[blockIdx.x];
    const int x = threadIdx.x;
    if (x >= (1 << J.m)) return;
    const Fr one = fr_one_mont();
    Fr f[8];
#pragma unroll
    for (int b = 0; b < 8; b++) f[b] = b < J.m ? ((x >> b) & 1 ? J.h.r[b] : fr_sub(one, J.h.r[b])) : one;
    const Fr p01 = fr_mul_wide(f[0], f[1]), p23 = fr_mul_wide(f[2], f[3]), p45 = fr_mul_wide(f[4], f[5]), p67 = fr_mul_wide(f[6], f[7]);
    J.eq[x] = fr_mul_wide(fr_mul_wide(p01, p23), fr_mul_wide(p45, p67));
}
struct EqOuterJob { Fr* eq; const Fr* lo; const Fr* hi; size_t total; };
__global__ __launch_bounds__(256) void k_bn_eq_outer_jobs(const EqOuterJob* __restrict__ jobs) {
    const EqOuterJob& J = jobs[blockIdx.y];
    for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < J.total; x += (size_t)gridDim.x * 256) J.eq[x] = fr_mul_wide(J.lo[x & 255], J.hi[x >> 8]);
}
// out[i] = sum_a alpha[a] tab[a][i] (the eq tables of a node's claims, G2)
struct CombJob { Fr* out; const Fr* tab[dev::MAX_CLAIMS]; Fr alpha[dev::MAX_CLAIMS]; size_t n; int na, pad; };
__global__ __launch_bounds__(256) void k_bn_comb_jobs(const CombJob* __restrict__ jobs) {
    const CombJob& J = jobs[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < J.n; i += (size_t)gridDim.x * 256) {
        WCol c = wcol_zero();
        for (int a = 0; a < J.na; a++) wcol_mac(c, J.alpha[a], J.tab[a][i]);
        J.out[i] = wcol_reduce(c);
    }
}
struct BnGatherTJob { dev::CsrLin lin; dev::CsrMul mul; BnPtrs in_vals; const Fr* eqc; Fr* T; int log2_S, log2_G, log2_R, pad; };
__global__ __launch_bounds__(BN_TPB) void k_bn_gather_T_jobs(const BnGatherTJob* __restrict__ jobs) {
    const BnGatherTJob& J = jobs[blockIdx.y];
    const size_t total = (size_t)1 << (J.log2_S + J.log2_R);
    const size_t smask = ((size_t)1 << J.log2_S) - 1;
    for (size_t idx = (size_t)blockIdx.x * BN_TPB + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BN_TPB) {
        const size_t x = idx & smask, rep = idx >> J.log2_S;
        const Fr* eq_rep = J.eqc + (rep << J.log2_G);
        Fr acc = fr_zero();
        if (J.lin.ptr)
            for (u32 e = J.lin.ptr[x]; e < J.lin.ptr[x + 1]; e++) {
                const Fr q = eq_rep[J.lin.gate[e]];
                const u64 c = J.lin.coef[e];
                acc = fr_add(acc, c == 1 ? q : fr_mul(q, fr_lift(c)));
            }
        if (J.mul.ptr)
            for (u32 e = J.mul.ptr[x]; e < J.mul.ptr[x + 1]; e++) {
                Fr q = eq_rep[J.mul.gate[e]];
                const u64 c = J.mul.coef[e];
                if (c != 1) q = fr_mul(q, fr_lift(c));
                acc = fr_add(acc, fr_mul(q, J.in_vals.p[J.mul.other_in[e]][(rep << J.log2_S) + J.mul.other_j[e]]));
            }
        J.T[idx] = acc;
    }
}
struct BnGatherBJob { dev::CsrMul m; const Fr* eqc; const Fr* eqx; const Fr* fin; Fr* B; BnU us; int arity, log2_S, log2_G, log2_R; };
__global__ __launch_bounds__(BN_TPB) void k_bn_gather_B_jobs(const BnGatherBJob* __restrict__ jobs) {
    const BnGatherBJob& J = jobs[blockIdx.y];
    __shared__ Fr u_sm[dev::PS_MAX_PAIRS];
    if ((int)threadIdx.x < J.arity) u_sm[threadIdx.x] = J.us.slot[threadIdx.x] >= 0 ? fr_to_mont(J.fin[J.us.slot[threadIdx.x]]) : fr_zero();
    __syncthreads();
    const size_t total = (size_t)1 << (J.log2_S + J.log2_R);
    const size_t smask = ((size_t)1 << J.log2_S) - 1;
    for (size_t idx = (size_t)blockIdx.x * BN_TPB + threadIdx.x; idx < total; idx += (size_t)gridDim.x * BN_TPB) {
        const size_t y = idx & smask, rep = idx >> J.log2_S;
        Fr acc = fr_zero();
        for (u32 e = J.m.ptr[y]; e < J.m.ptr[y + 1]; e++) {
            Fr q = J.eqc[(rep << J.log2_G) + J.m.gate[e]];
            const u64 c = J.m.coef[e];
            if (c != 1) q = fr_mul(q, fr_lift(c));
            q = fr_mul(q, J.eqx[(rep << J.log2_S) + J.m.other_j[e]]);
            acc = fr_add(acc, fr_mul(q, u_sm[J.m.other_in[e]]));
        }
        J.B[idx] = acc;
    }
}
struct FftPartJob { Fr* T; const Fr* W; BnPoint pt; int L, b_lo, b_hi, pad; };
__global__ __launch_bounds__(256) void k_bn_fft_part_jobs(const FftPartJob* __restrict__ jobs) {
    const FftPartJob& J = jobs[blockIdx.y];
    const size_t N = (size_t)1 << J.L, n = (size_t)1 << (J.L - J.b_lo);
    const Fr one = fr_one_mont();
    for (size_t y = (size_t)blockIdx.x * 256 + threadIdx.x; y < n; y += (size_t)gridDim.x * 256) {
        Fr acc = one;
        for (int b = J.b_lo; b < J.b_hi; b++) acc = fr_mul_wide(acc, bn_fft_factor(J.W, N, J.pt.r[b], y, b, one));
        J.T[y] = acc;
    }
}
// F(x) = sum over the node's claims of coef_a * prod_b factor_b(x; r_a): direct factors b < s1, part tables T1 ([s1, s2)), T2 ([s2, L))
struct FftTabClaim { Fr r[4]; Fr coef; const Fr* T1; const Fr* T2; };
struct FftTabJob { Fr* F; const Fr* W; const FftTabClaim* claims; int L, s1, s2, nclaims; };
__global__ __launch_bounds__(256) void k_bn_fft_tab_jobs(const FftTabJob* __restrict__ jobs) {
    const FftTabJob& J = jobs[blockIdx.y];
    const size_t N = (size_t)1 << J.L;
    const Fr one = fr_one_mont();
    for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < N; x += (size_t)gridDim.x * 256) {
        Fr sum = fr_zero();
        for (int a = 0; a < J.nclaims; a++) {
            const FftTabClaim& C = J.claims[a];
            Fr acc = C.coef;
            for (int b = 0; b < J.s1; b++) acc = fr_mul_wide(acc, bn_fft_factor(J.W, N, C.r[b], x, b, one));
            if (C.T1) acc = fr_mul_wide(acc, C.T1[x & (((size_t)1 << (J.L - J.s1)) - 1)]);
            if (C.T2) acc = fr_mul_wide(acc, C.T2[x & (((size_t)1 << (J.L - J.s2)) - 1)]);
            sum = a == 0 ? acc : fr_add(sum, acc);
        }
        J.F[x] = sum;
    }
}
// eq tables queued by level: heads (<= 8 variables) first, then the outer products whose factors are complete
struct EqPlan {
    std::vector<EqHeadJob> heads;
    std::vector<std::vector<EqOuterJob>> outers;   // [level - 1]
    bool empty() const { return heads.empty(); }
    // records build_eq_dev(eq, pt, n, scratch); returns the level of `eq` (0 = a head)
    int add(Fr* eq, const Fr* pt_canon, int n, Fr* scratch) {
        if (n <= 8) {
            EqHeadJob h;
            memset(&h, 0, sizeof(h));
            h.eq = eq; h.m = n;
            for (int i = 0; i < 8; i++) h.h.r[i] = i < n ? fr_to_mont(pt_canon[i]) : fr_zero();
            heads.push_back(h);
            return 0;
        }
        Fr* lo = scratch;
        Fr* hi = scratch + 256;
        add(lo, pt_canon, 8, nullptr);
        const int lh = add(hi, pt_canon + 8, n - 8, hi + ((size_t)1 << (n - 8)));
        const int level = lh + 1;
        if ((int)outers.size() < level) outers.resize(level);
        outers[level - 1].push_back(EqOuterJob{eq, lo, hi, (size_t)1 << n});
        return level;
    }
};
// stages a job array (bn254.hip: bn_stage); the caller flushes once per launch phase, before the first launch that reads it
template <typename J> static const J* upload_jobs(hipStream_t st, DevPool& pool, const std::vector<J>& v, std::vector<std::shared_ptr<void>>& keep) {
    (void)st; (void)keep;
    return bn_stage(pool.ctx, v.data(), v.size());
}
static void eq_plan_flush(hipStream_t st, DevPool& pool, EqPlan& P, std::vector<std::shared_ptr<void>>& keep) {
    if (P.heads.empty()) return;
    const EqHeadJob* d_heads = upload_jobs(st, pool, P.heads, keep);
    std::vector<const EqOuterJob*> d_lev;
    for (auto& lev : P.outers) d_lev.push_back(lev.empty() ? nullptr : upload_jobs(st, pool, lev, keep));
    bn_flush(pool.ctx, st);
    k_bn_eq_head_jobs<<<(unsigned)P.heads.size(), 256, 0, st>>>(d_heads);
    for (size_t q = 0; q < P.outers.size(); q++) {
        auto& lev = P.outers[q];
        if (lev.empty()) continue;
        size_t mx = 0;
        for (auto& j : lev) mx = std::max(mx, j.total);
        k_bn_eq_outer_jobs<<<dim3((unsigned)std::min<size_t>((mx + 255) / 256, 2048), (unsigned)lev.size()), 256, 0, st>>>(d_lev[q]);
    }
    P.heads.clear(); P.outers.clear();
}

// ---- host side of the walk ----------------------------------------------------------------------------------------------------
struct BnChain {  // Keccak256Transcript over Fr (transcript.rs:146-157: nothing is ever absorbed): a window on the process-wide chain
    std::vector<Fr> c;  // canonical
    size_t pos = 0;
    const Fr& at(size_t i) {
        if (c.size() <= i) {
            const size_t have = c.size(), want = std::max(i + 1, have + 2048);
            c.resize(want);
            bn_chain_copy(have, want - have, c.data() + have);
        }
        return c[i];
    }
    Fr next() { return at(pos++); }
    std::vector<Fr> next_n(size_t n) { std::vector<Fr> v(n); for (auto& x : v) x = next(); return v; }
};
struct BnClaim { std::vector<Fr> pt; std::shared_ptr<Fr> val; };  // point canonical; value (Montgomery) known when the transcript is replayed

struct BnValues {
    std::vector<Fr*> node;  // Montgomery tables, one per node
    Fr* ct0is = nullptr;
    std::map<std::pair<int, int>, const Fr*> W;  // (log2n, inverse) -> w^i for i < 2^log2n, shared by the NTTs and the DFT-row tables
};

// Witness generation over Fr = Circuit::evaluate on the device, level by level (Vanilla nodes: gate-major kernel; FFT nodes of one
// level and direction are laid out contiguously and transformed as one batch), as the Goldilocks witness_gen does. Two parts:
//   bn_witness_layout   where every node table lies, and the omega tables (they depend on the key only);
//   bn_witness_enqueue  lift of the input tables, FFT groups, gate maps - launches on the stream passed in and nothing else.
struct BnLayout {
    std::vector<int> level, order;   // `order` keeps a (level, direction, size) group of FFT nodes contiguous in memory
    int maxl = 0;
    size_t total = 0;                // elements of all node tables
    size_t max_grp = 1;              // elements of the largest FFT group: the transforms' scratch
};
// the gate constants must be non-negative integers below 2^63 (they are lifted into Fr as such): a property of the KEY, checked
// once per key - walking the ~10^7 gate terms of the headline circuit on the host took 8 ms of every witness generation
static void bn_check_gate_constants(const hg_pk* pk) {
    static std::mutex mu;
    static std::vector<uint64_t> checked;
    std::lock_guard<std::mutex> lk(mu);
    if (std::find(checked.begin(), checked.end(), pk->serial) != checked.end()) return;
    for (const HNode& n : pk->circuit.nodes) {
        if (n.kind != NK_VANILLA) continue;
        for (auto& t : n.lin) if (t.c >> 63) throw Error("bn254: gate constant is not a non-negative integer below 2^63");
        for (auto& t : n.mul) if (t.c >> 63) throw Error("bn254: gate constant is not a non-negative integer below 2^63");
        for (auto& t : n.w0) if (t.c >> 63) throw Error("bn254: gate constant is not a non-negative integer below 2^63");
    }
    if (checked.size() > 64) checked.clear();
    checked.push_back(pk->serial);
}
// get(n): n elements of device memory (the context arena for one prove, memory of its own for a pipeline). share_w: a table set of the
// same key whose omega tables this one reads too (null: they are built, on `st`)
template <typename Get>
static BnLayout bn_witness_layout(const hg_pk* pk, hipStream_t st, Get&& get, size_t ct0is_len, BnValues& V, const BnValues* share_w = nullptr) {
    const HCircuit& c = pk->circuit;
    BnLayout Y;
    const size_t nn = c.nodes.size();
    Y.level.assign(nn, 0);
    for (int id : c.topo) { for (int pr : c.nodes[id].preds) Y.level[id] = std::max(Y.level[id], Y.level[pr] + 1); Y.maxl = std::max(Y.maxl, Y.level[id]); }
    Y.order.resize(nn);
    for (size_t i = 0; i < nn; i++) Y.order[i] = (int)i;
    auto key = [&](int id) { const HNode& n = c.nodes[id]; return std::make_tuple(n.kind == NK_FFT ? 1 : 0, Y.level[id], n.inverse ? 1 : 0, n.log2_size, id); };
    std::sort(Y.order.begin(), Y.order.end(), [&](int x, int y) { return key(x) < key(y); });
    for (size_t id = 0; id < nn; id++) Y.total += (size_t)1 << c.nodes[id].log2_out();
    Fr* base = get(Y.total);
    V.node.assign(nn, nullptr);
    {
        size_t off = 0;
        for (int id : Y.order) { V.node[id] = base + off; off += (size_t)1 << c.nodes[id].log2_out(); }
    }
    V.ct0is = get(ct0is_len);
    if (share_w) V.W = share_w->W;
    for (size_t id = 0; id < nn; id++) {
        const HNode& n = c.nodes[id];
        if (n.kind != NK_FFT || V.W.count({n.log2_size, (int)n.inverse})) continue;
        if (n.log2_size > 28) throw Error("bn254: two-adicity is 28");
        const size_t N = (size_t)1 << n.log2_size;
        Fr* W = get(N);
        Fr wr = fr_root_of_unity(n.log2_size);
        if (n.inverse) wr = fr_inv(wr);
        k_bn_powers<<<grid_of(N), 256, 0, st>>>(W, wr, N);
        V.W[{n.log2_size, (int)n.inverse}] = W;
    }
    bn_check_gate_constants(pk);
    std::map<std::tuple<int, int, int>, size_t> grp_sz;
    for (size_t id = 0; id < nn; id++)
        if (c.nodes[id].kind == NK_FFT) grp_sz[{Y.level[id], (int)c.nodes[id].inverse, c.nodes[id].log2_size}] += (size_t)1 << c.nodes[id].log2_size;
    for (auto& kv : grp_sz) Y.max_grp = std::max(Y.max_grp, kv.second);
    return Y;
}
// the input tables of a witness as lift jobs, in NodeId order: s, e, k1, ais.., r1is.., r2is (chain_par! sk_encryption_circuit.rs:408),
// then ct0is. src(q, len): where table q lies on the device as u64 words
template <typename Src>
static size_t bn_lift_jobs(const hg_pk* pk, const BnValues& V, Src&& src, LiftJobs& LJ) {
    const HCircuit& c = pk->circuit;
    const Params& p = pk->params;
    const size_t SZ = p.SZ(), k = (size_t)p.k;
    memset(&LJ, 0, sizeof(LJ));
    size_t max_len = 0;
    auto put = [&](size_t len, Fr* dst) {
        if (LJ.n >= 64) throw Error("circuit: more than 64 input tables");
        LJ.src[LJ.n] = src(LJ.n, len); LJ.dst[LJ.n] = dst; LJ.len[LJ.n] = len; LJ.n++;
        max_len = std::max(max_len, len);
    };
    if (c.input_ids.size() != 3 + 2 * k + 1) throw Error("circuit: unexpected input nodes");
    for (size_t q = 0; q < 3 + 2 * k + 1; q++) {
        const int id = c.input_ids[q];
        const size_t len = q < 3 + 2 * k ? SZ : k * p.PZ();
        if (len != (size_t)1 << c.nodes[id].log2_out()) throw Error("circuit: input size mismatch");
        put(len, V.node[id]);
    }
    put(k * SZ, V.ct0is);
    return max_len;
}
// tmp: Y.max_grp elements. pairs: the lift that reads two words per lane (k_bn_lift_pairs: 16-byte aligned tables of even length)
static void bn_witness_enqueue(const hg_pk* pk, const BnLayout& Y, const BnValues& V, const LiftJobs& LJ, size_t max_len, bool pairs, Fr* tmp, hipStream_t st) {
    const HCircuit& c = pk->circuit;
    const size_t nn = c.nodes.size();
    if (pairs) k_bn_lift_pairs<<<dim3((unsigned)std::min<size_t>((max_len / 2 + 255) / 256, 1024), (unsigned)LJ.n), 256, 0, st>>>(LJ);
    else k_bn_lift_jobs<<<dim3((unsigned)std::min<size_t>((max_len + 255) / 256, 1024), (unsigned)LJ.n), 256, 0, st>>>(LJ);
    const std::vector<int>& level = Y.level;
    const std::vector<int>& order = Y.order;
    for (int l = 1; l <= Y.maxl; l++) {
        // FFT groups of this level
        for (size_t q = 0; q < nn;) {
            const int id0 = order[q];
            const HNode& n0 = c.nodes[id0];
            if (n0.kind != NK_FFT || level[id0] != l) { q++; continue; }
            size_t e = q;
            while (e < nn && c.nodes[order[e]].kind == NK_FFT && level[order[e]] == l && c.nodes[order[e]].inverse == n0.inverse &&
                   c.nodes[order[e]].log2_size == n0.log2_size)
                e++;
            const size_t N = (size_t)1 << n0.log2_size;
            NttSrc srcs;
            memset(&srcs, 0, sizeof(srcs));
            for (size_t t = q; t < e && t - q < 64; t++) srcs.p[t - q] = V.node[c.nodes[order[t]].preds[0]];
            const Fr* Wn = V.W.at({n0.log2_size, (int)n0.inverse});
            // the four-step transform reads every input where it lies (no copy into the group's output area first)
            if (!ntt4_dev(st, V.node[id0], tmp, Wn, n0.log2_size, n0.inverse, n0.inverse ? fr_inv(fr_small((u64)N)) : fr_one_mont(), e - q, &srcs)) {
                for (size_t t = q; t < e; t++)
                    hipc(hipMemcpyAsync(V.node[order[t]], V.node[c.nodes[order[t]].preds[0]], N * sizeof(Fr), hipMemcpyDeviceToDevice, st), "copy fft input");
                ntt_dev(st, V.node[id0], tmp, Wn, n0.log2_size, n0.inverse, e - q);
            }
            q = e;
        }
        for (int id : c.topo) {
            const HNode& n = c.nodes[id];
            if (level[id] != l) continue;
            if (n.kind == NK_VANILLA) {
                BnPtrs in;
                memset(&in, 0, sizeof(in));
                if (n.arity > dev::PS_MAX_PAIRS) throw Error("vanilla: arity too large");
                for (int i = 0; i < n.arity; i++) in.p[i] = V.node[n.preds[i]];
                const size_t tot = (size_t)1 << n.log2_out();
                k_bn_gate_eval<<<(unsigned)std::min<size_t>((tot + BN_TPB - 1) / BN_TPB, 4096), BN_TPB, 0, st>>>(pk->node_dev[id].fwd, in, V.node[id]);
            } else if (n.kind == NK_LASSO) {
                hipc(hipMemsetAsync(V.node[id], 0, sizeof(Fr), st), "lasso output");  // LassoNode::evaluate returns [0] (lasso.rs:53-55)
            }
        }
    }
}

// both parts for a host witness, in the context's arena: the tables are uploaded, and the stream is drained before the prover starts
static void bn_witness_gen(hg_ctx* ctx, const hg_pk* pk, const Witness& w, DevPool& pool, BnValues& V) {
    const Params& p = pk->params;
    hipStream_t st = ctx->stream;
    const bool times = hg_times("bn");   // read at every call (host.hpp)
    const double tw0 = wall_ms();
    auto stamp = [&](const char* what) { if (times) fprintf(stderr, "[hg bn] witness %8.3f ms  %s\n", wall_ms() - tw0, what); };
    const BnLayout Y = bn_witness_layout(pk, st, [&](size_t n) { return pool.get<Fr>(n); }, w.ct0is.size(), V);
    stamp("tables laid out, omega tables enqueued");
    const size_t mark = pool.mark();
    // every upload first (a copy from pageable memory makes the host wait for whatever the stream still holds: no kernel may sit
    // between them), then ONE lift launch
    const size_t SZ = p.SZ(), k = (size_t)p.k;
    if (w.r2is.size() != k * p.PZ() || w.ct0is.size() != k * SZ) throw Error("circuit: input size mismatch");
    const size_t n_in = (3 + 2 * k) * SZ + w.r2is.size() + w.ct0is.size();
    u64* stage = pool.get<u64>(n_in);
    size_t soff = 0;
    LiftJobs LJ;
    const size_t max_len = bn_lift_jobs(pk, V, [&](int q, size_t len) {
        const size_t K = (size_t)p.k, x = (size_t)q;
        const u64* h = x == 0 ? w.s.data() : x == 1 ? w.e.data() : x == 2 ? w.k1.data() : x < 3 + K ? &w.ais[(x - 3) * SZ] : x < 3 + 2 * K ? &w.r1is[(x - 3 - K) * SZ]
                       : x == 3 + 2 * K ? w.r2is.data() : w.ct0is.data();
        hipc(hipMemcpyAsync(stage + soff, h, len * 8, hipMemcpyHostToDevice, st), "upload input");
        const u64* d = stage + soff;
        soff += len;
        return d;
    }, LJ);
    stamp("inputs uploaded");
    Fr* tmp = pool.get<Fr>(Y.max_grp);
    bn_witness_enqueue(pk, Y, V, LJ, max_len, false, tmp, st);
    stamp("lift and circuit enqueued");
    hipc(hipStreamSynchronize(st), "bn254 witness generation: sync");
    stamp("drained");
    hipc(hipGetLastError(), "bn254 witness generation: launch");
    pool.release_from(mark);
}

// node values (canonical limbs) for tests: which = 0 the sum node, 1 the Lasso input node, 2 the ct0is table
void circuit_eval_bn254(hg_ctx* ctx, const hg_pk* pk, const Witness& w, int which, std::vector<u64>& out4) {
    if (!pk->ctx) throw Error("hg_circuit_eval_bn254: host-only prover key");
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    DevPool pool(ctx);
    BnValues V;
    bn_witness_gen(ctx, pk, w, pool, V);
    const HCircuit& c = pk->circuit;
    Fr* src;
    size_t n;
    if (which == 0) { src = V.node[c.sum_id]; n = (size_t)1 << c.nodes[c.sum_id].log2_out(); }
    else if (which == 1) { src = V.node[c.lasso_in_id]; n = (size_t)1 << c.nodes[c.lasso_in_id].log2_out(); }
    else if (which == 2) { src = V.ct0is; n = w.ct0is.size(); }
    else throw Error("hg_circuit_eval_bn254: which must be 0 (sum), 1 (lasso input) or 2 (ct0is)");
    k_bn_from_mont<<<grid_of(n), 256, 0, ctx->stream>>>(src, n);
    out4.resize(n * 4);
    hipc(hipMemcpyAsync(out4.data(), src, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream), "copy node values");
    hipc(hipStreamSynchronize(ctx->stream), "sync");
}

// Enqueue-everything / replay-later, as in the Goldilocks prover: the challenges do not depend on the prover's messages, and no
// kernel argument depends on a value the host would have to read back (Libra phase 2 takes u = in(r_x) from the result buffer on
// the device), so the Vanilla / FFT node reductions are enqueued back to back; their round sums and folded values land in the
// host-mapped result buffer and the transcript steps are closures replayed in protocol order after ONE synchronisation. The
// Lasso node keeps its own three synchronisations (lasso_prove_bn254_impl).
struct BnProver {
    hg_ctx* ctx;
    const hg_pk* pk;
    hipStream_t st;
    DevPool pool;
    BnValues V;
    // The Vanilla / FFT node reductions go to the context's second stream; the Lasso node (three host synchronisations of its
    // own, on the first stream) is run after everything else has been enqueued, so the two overlap on the device.
    bool overlap;
    BnProver(hg_ctx* c, const hg_pk* k) : ctx(c), pk(k), st(c->stream), pool(c) {
        static const bool one_stream_env = hg_env_on("HG_ONE_STREAM");
        overlap = !(one_stream_env || c->one_stream);
        if (overlap) st = c->stream2;
    }
    std::map<int, Fr> inv_size;   // 1 / 2^L for the inverse FFT nodes
    std::function<void()> lasso_deferred;
    std::function<void()> lasso_mid;   // the node reductions' launches, enqueued from inside the Lasso node's enqueue (run())
    int lasso_mid_at = 0;
    BnChain chain;
    std::vector<std::vector<BnClaim>> claims;
    std::vector<uint8_t> proof;
    std::vector<std::function<void()>> replay;   // transcript steps in protocol order
    std::vector<PsPlan> ps_queue;                // sum-checks waiting for the next round-synchronised flush
    std::vector<std::function<void()>> second_wave;  // Libra phase-2 bookkeeping: needs the phase-1 values in the result buffer
    // bookkeeping of all nodes, queued by the walk and launched per kind (flush_bookkeeping): eq tables -> claim combinations ->
    // constant sums, Libra gathers, DFT-row part tables -> DFT-row tables
    EqPlan eq_plan;
    std::vector<CombJob> comb_jobs;
    std::vector<std::function<void()>> const_sums;
    std::vector<BnGatherTJob> gatherT_jobs;
    std::vector<BnGatherBJob> gatherB_jobs;
    std::vector<FftPartJob> fft_parts;
    std::vector<FftTabJob> fft_tabs;
    std::vector<std::shared_ptr<std::vector<FftTabClaim>>> fft_claims;   // per fft_tabs entry, uploaded at flush
    template <typename J, typename K> void launch_staged(const J* d, size_t n, K kernel, size_t max_total, int tpb) {
        if (!n) return;
        kernel<<<dim3((unsigned)std::min<size_t>((max_total + tpb - 1) / tpb, 2048), (unsigned)n), tpb, 0, st>>>(d);
    }
    void flush_bookkeeping() {
        eq_plan_flush(st, pool, eq_plan, keep);
        // every job array of this phase is staged first and copied over in one transfer; then one launch per kind
        size_t mx_comb = 0, mx_t = 0, mx_b = 0, mx_part = 0, mx_tab = 0;
        for (auto& j : comb_jobs) mx_comb = std::max(mx_comb, j.n);
        for (auto& j : gatherT_jobs) mx_t = std::max(mx_t, (size_t)1 << (j.log2_S + j.log2_R));
        for (auto& j : gatherB_jobs) mx_b = std::max(mx_b, (size_t)1 << (j.log2_S + j.log2_R));
        for (auto& j : fft_parts) mx_part = std::max(mx_part, (size_t)1 << (j.L - j.b_lo));
        for (size_t q = 0; q < fft_tabs.size(); q++) {
            fft_tabs[q].claims = upload_jobs(st, pool, *fft_claims[q], keep);
            mx_tab = std::max(mx_tab, (size_t)1 << fft_tabs[q].L);
        }
        fft_claims.clear();
        const size_t n_comb = comb_jobs.size(), n_t = gatherT_jobs.size(), n_b = gatherB_jobs.size(), n_part = fft_parts.size(), n_tab = fft_tabs.size();
        const CombJob* d_comb = n_comb ? upload_jobs(st, pool, comb_jobs, keep) : nullptr;
        const BnGatherTJob* d_t = n_t ? upload_jobs(st, pool, gatherT_jobs, keep) : nullptr;
        const BnGatherBJob* d_b = n_b ? upload_jobs(st, pool, gatherB_jobs, keep) : nullptr;
        const FftPartJob* d_part = n_part ? upload_jobs(st, pool, fft_parts, keep) : nullptr;
        const FftTabJob* d_tab = n_tab ? upload_jobs(st, pool, fft_tabs, keep) : nullptr;
        comb_jobs.clear(); gatherT_jobs.clear(); gatherB_jobs.clear(); fft_parts.clear(); fft_tabs.clear();
        bn_flush(ctx, st);
        launch_staged(d_comb, n_comb, k_bn_comb_jobs, mx_comb, 256);
        for (auto& f : const_sums) f();
        const_sums.clear();
        launch_staged(d_t, n_t, k_bn_gather_T_jobs, mx_t, BN_TPB);
        launch_staged(d_b, n_b, k_bn_gather_B_jobs, mx_b, BN_TPB);
        launch_staged(d_part, n_part, k_bn_fft_part_jobs, mx_part, 256);
        launch_staged(d_tab, n_tab, k_bn_fft_tab_jobs, mx_tab, 256);
    }
    std::vector<std::shared_ptr<void>> keep;     // host staging of asynchronous uploads
    std::map<std::vector<u64>, Fr*> eq_shared, fft_shared;   // point (+ size, direction) -> table of a single unit-weight claim
    static bool share_tables() { return true; }
    static std::vector<u64> point_key(const std::vector<Fr>& pt, int n) {
        std::vector<u64> k;
        k.reserve(pt.size() * 4 + 1);
        for (const Fr& x : pt) for (int i = 0; i < 4; i++) k.push_back(((const u64*)&x)[i]);
        k.push_back((u64)n);
        return k;
    }

    static std::shared_ptr<Fr> cell() { return std::make_shared<Fr>(fr_zero()); }
    void write(const Fr& canonical) { write_be32(proof, canonical); }
    // prove_sum_check transcript side: 3 coefficients per round from g(0), g(2); returns the claim after the last round
    Fr replay_prodsum(const PsOut& o, const std::vector<Fr>& rs, Fr claim) {
        for (size_t rd = 0; rd < rs.size(); rd++) {
            Fr cf[4];
            claim = replay_round(&o.sums.host[rd * 2], 2, claim, fr_to_mont(rs[rd]), cf);
            for (int k = 0; k < 3; k++) write(fr_from_mont(cf[k]));
        }
        return claim;
    }
    // G2: alpha per claim when there is more than one (squeezed now, in protocol order)
    std::vector<Fr> alphas(size_t nclaims) {
        std::vector<Fr> alpha(nclaims, fr_one_mont());
        if (nclaims > 1) for (auto& a : alpha) a = fr_to_mont(chain.next());
        return alpha;
    }
    static Fr combined(const std::vector<BnClaim>& cl, const std::vector<Fr>& alpha) {  // replay time: sum_a alpha_a value_a
        Fr v = fr_zero();
        for (size_t a = 0; a < cl.size(); a++) v = fr_add(v, fr_mul(alpha[a], *cl[a].val));
        return v;
    }

    void vanilla_node(int id) {
        const HNode& n = pk->circuit.nodes[id];
        const hg_pk::NodeDev& nd = pk->node_dev[id];
        const int nin = n.log2_sub_in + n.log2_reps, lo = n.log2_out();
        const size_t SR = (size_t)1 << nin, OUT = (size_t)1 << lo;
        const std::vector<BnClaim> cl = claims[id];
        for (auto& c : cl) if ((int)c.pt.size() != lo) throw Error("gkr: claim arity mismatch");
        const std::vector<Fr> alpha = alphas(cl.size());
        // nodes opened at the same point by the same sum-check (every input of a Vanilla node is opened at the node's r_x: the five
        // inputs of the final sum, the eight chunk nodes ...) share one eq table (read-only everywhere)
        Fr* eqc = nullptr;
        if (cl.size() > (size_t)dev::MAX_CLAIMS) throw Error("gkr: too many claims on one node");
        if (cl.size() == 1) {
            const std::vector<u64> key = point_key(cl[0].pt, lo);
            auto hit = share_tables() ? eq_shared.find(key) : eq_shared.end();
            if (hit != eq_shared.end()) eqc = hit->second;
            else {
                eqc = pool.get<Fr>(OUT);
                eq_plan.add(eqc, cl[0].pt.data(), lo, pool.get<Fr>(eq_scratch_len(lo)));
                eq_shared[key] = eqc;
            }
        } else {   // one table per claim (they are built side by side), then eqc = sum_a alpha_a eq_a
            eqc = pool.get<Fr>(OUT);
            CombJob cj;
            memset(&cj, 0, sizeof(cj));
            cj.out = eqc; cj.n = OUT; cj.na = (int)cl.size();
            for (size_t a = 0; a < cl.size(); a++) {
                Fr* tmp = pool.get<Fr>(OUT);
                eq_plan.add(tmp, cl[a].pt.data(), lo, pool.get<Fr>(eq_scratch_len(lo)));
                cj.tab[a] = tmp; cj.alpha[a] = alpha[a];
            }
            comb_jobs.push_back(cj);
        }
        ResRef const_sum{nullptr, nullptr};
        if (nd.nconst) {  // claim -= sum_g eqc[g] * w0_g
            Fr* d_part = pool.get<Fr>(1024);
            const size_t total = nd.nconst << n.log2_reps;
            const int grid = (int)std::min<size_t>((total + BN_TPB - 1) / BN_TPB, 1024);
            const_sum = res_slots(ctx, 1);
            const hg_pk::NodeDev* ndc = &nd;
            const int lso = n.log2_sub_out, lrp = n.log2_reps;
            Fr* cs_dev = const_sum.dev;
            const_sums.push_back([this, ndc, eqc, lso, lrp, d_part, grid, cs_dev] {
                k_bn_const_sum<<<grid, BN_TPB, 0, st>>>(ndc->const_gate, ndc->const_coef, ndc->nconst, eqc, lso, lrp, d_part);
                k_bn_reduce<<<1, BN_TPB, 0, st>>>(d_part, grid, 1, cs_dev);
            });
        }
        std::vector<int> li, ri;
        for (int i = 0; i < n.arity; i++) { if (n.left_use[i]) li.push_back(i); if (n.right_use[i]) ri.push_back(i); }
        if (n.arity > dev::PS_MAX_PAIRS) throw Error("vanilla: arity too large");
        BnPtrs in_vals;
        memset(&in_vals, 0, sizeof(in_vals));
        for (int i = 0; i < n.arity; i++) in_vals.p[i] = V.node[n.preds[i]];
        // phase 1: sum_x sum_i in_i(x) T_i(x)
        std::vector<const Fr*> a, b;
        static const bool use_alias = !hg_env_on("HG_GATHER_CSR");
        for (int i : li) {
            const hg_pk::NodeDev::Seg& sg = nd.seg[i];
            // one unit relay per position: the bookkeeping table IS a slice of the node's eq table (capi.hip: run-length form)
            Fr* T = use_alias && sg.alias ? eqc + sg.alias_off : pool.get<Fr>(SR);
            if (!(use_alias && sg.alias)) {
                BnGatherTJob gj;
                memset(&gj, 0, sizeof(gj));
                gj.lin = nd.lin[i]; gj.mul = nd.mulL[i]; gj.in_vals = in_vals; gj.eqc = eqc; gj.T = T;
                gj.log2_S = n.log2_sub_in; gj.log2_G = n.log2_sub_out; gj.log2_R = n.log2_reps;
                gatherT_jobs.push_back(gj);
            }
            a.push_back(V.node[n.preds[i]]);
            b.push_back(T);
        }
        const std::vector<Fr> rx = chain.next_n(nin);
        size_t wl = 0, wh = 0;
        if (li.size() == 1 && n.log2_reps == 0 && !n.lin.empty() && n.mul.empty() && nd.seg[li[0]].d && !nd.seg[li[0]].alias) { wl = nd.seg[li[0]].win_lo; wh = nd.seg[li[0]].win_hi; }
        const PsOut o1 = prodsum_defer(pool, ps_queue, a, b, nin, rx, wl, wh);
        std::vector<std::shared_ptr<Fr>> ucell, wcell;
        for (size_t q = 0; q < li.size(); q++) {
            ucell.push_back(cell());
            claims[n.preds[li[q]]].push_back(BnClaim{rx, ucell.back()});
        }
        const bool has_mul = !n.mul.empty();
        std::vector<Fr> ry;
        PsOut o2{};
        if (has_mul) {
            if (!n.lin.empty()) throw Error("vanilla: nodes mixing linear and mul gates are not on this path");
            // phase 2: sum_y sum_i in_i(y) B_i(y); the claim carries over from phase 1 (no linear part). Challenges and result
            // slots are taken now, in protocol order; the bookkeeping kernels need u = in(r_x) and run in the second wave.
            ry = chain.next_n(nin);
            std::vector<const Fr*> a2, b2;
            std::vector<Fr*> Bs;
            for (int i : ri) {
                Bs.push_back(pool.get<Fr>(SR));
                a2.push_back(V.node[n.preds[i]]);
                b2.push_back(Bs.back());
            }
            std::vector<PsPlan> own;   // reserve the plan (buffers, slots) now, queue it with the second wave
            o2 = prodsum_defer(pool, own, a2, b2, nin, ry);
            const PsPlan plan2 = own[0];
            Fr* eqx = pool.get<Fr>(SR);
            Fr* eqx_scratch = pool.get<Fr>(eq_scratch_len(nin));
            const hg_pk::NodeDev* ndp = &nd;
            const HNode* np = &n;
            second_wave.push_back([this, eqx, eqx_scratch, rx, nin, li, ri, Bs, ndp, np, eqc, o1, plan2] {   // queues only: run() flushes
                eq_plan.add(eqx, rx.data(), nin, eqx_scratch);
                BnU us;
                for (auto& x : us.slot) x = -1;
                for (size_t q = 0; q < li.size(); q++) us.slot[li[q]] = (int)(2 * q);
                for (size_t q = 0; q < ri.size(); q++) {
                    BnGatherBJob bj;
                    memset(&bj, 0, sizeof(bj));
                    bj.m = ndp->mulR[ri[q]]; bj.eqc = eqc; bj.eqx = eqx; bj.fin = o1.fin.dev; bj.B = Bs[q]; bj.us = us;
                    bj.arity = np->arity; bj.log2_S = np->log2_sub_in; bj.log2_G = np->log2_sub_out; bj.log2_R = np->log2_reps;
                    gatherB_jobs.push_back(bj);
                }
                ps_queue.push_back(plan2);
            });
            for (size_t q = 0; q < ri.size(); q++) {
                wcell.push_back(cell());
                claims[n.preds[ri[q]]].push_back(BnClaim{ry, wcell.back()});
            }
        }
        replay.push_back([this, cl, alpha, const_sum, o1, o2, rx, ry, ucell, wcell, has_mul] {
            Fr claim = combined(cl, alpha);
            if (const_sum.host) claim = fr_sub(claim, fr_to_mont(*const_sum.host));
            const Fr after1 = replay_prodsum(o1, rx, claim);
            for (size_t q = 0; q < ucell.size(); q++) {
                write(o1.fin.host[2 * q]);
                *ucell[q] = fr_to_mont(o1.fin.host[2 * q]);
            }
            if (has_mul) {
                (void)replay_prodsum(o2, ry, after1);
                for (size_t q = 0; q < wcell.size(); q++) {
                    write(o2.fin.host[2 * q]);
                    *wcell[q] = fr_to_mont(o2.fin.host[2 * q]);
                }
            }
        });
    }

    void fft_node(int id) {
        const HNode& n = pk->circuit.nodes[id];
        const int L = n.log2_size;
        if (L > 28) throw Error("bn254: two-adicity is 28");
        const size_t N = (size_t)1 << L;
        const std::vector<BnClaim> cl = claims[id];
        const std::vector<Fr> alpha = alphas(cl.size());
        const Fr* W = V.W.at({L, (int)n.inverse});
        if (n.inverse && !inv_size.count(L)) inv_size[L] = fr_inv(fr_small((u64)N));   // one 254-bit exponentiation per size, not per node
        const Fr scale = n.inverse ? inv_size[L] : fr_one_mont();
        if (cl.size() > (size_t)dev::MAX_CLAIMS) throw Error("gkr: too many claims on one node");
        // (the sixteen inverse-FFT nodes behind sai_par are all opened at sai_par's r_x: one DFT-row table)
        Fr* F = nullptr;
        bool F_shared = false;
        if (cl.size() == 1) {
            std::vector<u64> key = point_key(cl[0].pt, L);
            key.push_back(n.inverse ? 1 : 0);
            auto hit = share_tables() ? fft_shared.find(key) : fft_shared.end();
            if (hit != fft_shared.end()) { F = hit->second; F_shared = true; }
            else { F = pool.get<Fr>(N); fft_shared[key] = F; }
        } else F = pool.get<Fr>(N);
        const int s1 = std::min(4, L), s2 = std::min(8, L);   // direct factors b < s1; tables over [s1, s2) and [s2, L)
        auto tab_claims = std::make_shared<std::vector<FftTabClaim>>();
        for (size_t a = 0; a < cl.size() && !F_shared; a++) {
            if ((int)cl[a].pt.size() != L) throw Error("gkr: claim arity mismatch");
            FftPartJob pj;
            memset(&pj, 0, sizeof(pj));
            for (int b = 0; b < L; b++) pj.pt.r[b] = fr_to_mont(cl[a].pt[b]);
            pj.W = W; pj.L = L;
            FftTabClaim tc;
            memset(&tc, 0, sizeof(tc));
            for (int b = 0; b < s1; b++) tc.r[b] = pj.pt.r[b];
            tc.coef = fr_mul(alpha[a], scale);
            if (s2 > s1) { tc.T1 = pj.T = pool.get<Fr>((size_t)1 << (L - s1)); pj.b_lo = s1; pj.b_hi = s2; fft_parts.push_back(pj); }
            if (L > s2) { tc.T2 = pj.T = pool.get<Fr>((size_t)1 << (L - s2)); pj.b_lo = s2; pj.b_hi = L; fft_parts.push_back(pj); }
            tab_claims->push_back(tc);
        }
        if (!F_shared) {
            FftTabJob tj;
            memset(&tj, 0, sizeof(tj));
            tj.F = F; tj.W = W; tj.L = L; tj.s1 = s1; tj.s2 = s2; tj.nclaims = (int)cl.size();
            fft_tabs.push_back(tj);
            fft_claims.push_back(tab_claims);
        }
        const std::vector<Fr> rx = chain.next_n(L);
        const PsOut o = prodsum_defer(pool, ps_queue, {V.node[n.preds[0]]}, {F}, L, rx);
        std::shared_ptr<Fr> u = cell();
        claims[n.preds[0]].push_back(BnClaim{rx, u});
        replay.push_back([this, cl, alpha, o, rx, u] {
            (void)replay_prodsum(o, rx, combined(cl, alpha));
            write(o.fin.host[0]);
            *u = fr_to_mont(o.fin.host[0]);
        });
    }

    void lasso_node(int id) {
        const HNode& n = pk->circuit.nodes[id];
        const int in_id = n.preds[0];
        const int nu = pk->lasso.nu;
        if (pk->circuit.nodes[in_id].log2_out() != nu) throw Error("lasso: input size != 2^nu");
        auto bytes = std::make_shared<std::vector<uint8_t>>();
        const size_t at = chain.pos;
        BnClaim c;
        c.pt.resize(nu);
        for (int i = 0; i < nu; i++) c.pt[i] = chain.at(at + i);   // the claim point r is the node's first nu challenges (lasso.rs:85,97)
        c.val = cell();                                             // the claimed sum: known once the node has run
        chain.pos += (size_t)nu + nu + 2 + gp_challenges(nu) + gp_challenges(16);
        replay.push_back([this, bytes] { proof.insert(proof.end(), bytes->begin(), bytes->end()); });
        std::shared_ptr<Fr> val = c.val;
        const Fr* d_in = V.node[in_id];
        auto run_node = [this, bytes, at, nu, val, d_in] {
            std::vector<u64> claim4((size_t)(nu + 1) * 4);
            lasso_prove_bn254_impl(ctx, pk, nullptr, d_in, at, *bytes, claim4.data(), lasso_mid ? &lasso_mid : nullptr, lasso_mid_at);   // the input stays in HBM
            for (int i = 0; i < nu; i++) if (memcmp(chain.at(at + i).l, &claim4[4 * i], 32) != 0) throw Error("bn254: lasso claim point is not the challenge run");
            Fr v;
            memcpy(v.l, &claim4[4 * (size_t)nu], 32);
            *val = fr_to_mont(v);
        };
        if (overlap) lasso_deferred = run_node;  // run() starts it once every node reduction is enqueued on the other stream
        else run_node();
        claims[in_id].push_back(c);
    }

    // MLE evaluation by folding, up to ten variables per launch (k_bn_fold_multi); the value lands in a result slot (canonical), read
    // by the replay after the synchronisation
    const Fr* mle_dev(const Fr* table, int nv, const Fr* pt_canon) {
        const ResRef out = res_slots(ctx, 1);
        mle_fold_dev(st, table, nv, pt_canon, [this](size_t n) { return pool.get<Fr>(n); }, out.dev);
        return out.host;
    }

    void run(const Witness& w, double* ms) {
        const double t0 = wall_ms();
        bn_witness_gen(ctx, pk, w, pool, V);
        const double t1 = wall_ms();
        prove_tables();
        if (ms) { ms[0] = t1 - t0; ms[1] = wall_ms() - t1; }
    }
    // The prove on tables it did not build (hg_prove_encryptions_bn254): `filled` lies outside the arena and is complete once `ready` has
    // been reached on the stream that filled it - both prover streams wait for that event on the device, the host does not.
    void run_filled(const BnValues& filled, hipEvent_t ready, double* prove_ms) {
        const double t1 = wall_ms();
        V = filled;
        hipc(hipStreamWaitEvent(ctx->stream, ready, 0), "stream wait");
        if (ctx->stream2 != ctx->stream) hipc(hipStreamWaitEvent(ctx->stream2, ready, 0), "stream wait");
        prove_tables();
        if (prove_ms) *prove_ms = wall_ms() - t1;
    }
    void prove_tables() {
        const HCircuit& c = pk->circuit;
        const Params& p = pk->params;
        const double t1 = wall_ms();
        // "eval output" (sk_encryption_circuit.rs:444-448): point, ct0is MLE value
        const int ov = p.ct0is_log2();
        BnClaim out;
        out.pt = chain.next_n(ov);
        out.val = cell();
        const Fr* out_slot = nullptr;
        claims.assign(c.nodes.size(), {});
        claims[c.lasso_id].push_back(BnClaim{{}, cell()});  // EvalClaim::new(vec![], E::ZERO) (:450)
        claims[c.sum_id].push_back(out);
        for (size_t q = c.topo.size(); q-- > 0;) {            // prove_gkr (:455-457), G1: the walk only queues (no launch yet)
            const int id = c.topo[q];
            switch (c.nodes[id].kind) {
                case NK_INPUT: break;
                case NK_VANILLA: vanilla_node(id); break;
                case NK_FFT: fft_node(id); break;
                case NK_LASSO: lasso_node(id); break;
            }
        }
        // everything the Vanilla / FFT nodes need, on the node stream: output evaluation, bookkeeping, both waves of sum-checks
        const bool times = hg_times("bn");   // read at every call (host.hpp)
        auto stamp = [&](const char* what) { if (times) fprintf(stderr, "[hg bn] %8.3f ms  %s\n", wall_ms() - t1, what); };
        stamp("walk done");
        auto node_launches = [&] {
            stamp("node launches: begin");
            out_slot = mle_dev(V.ct0is, ov, out.pt.data());
            stamp("  output evaluation enqueued");
            flush_bookkeeping();                        // eq tables, claim combinations, constant sums, Libra gathers, DFT-row tables: one launch per kind
            stamp("  bookkeeping 1 enqueued");
            prodsum_flush(st, pool, ps_queue, keep);   // first wave: every FFT / Libra phase-1 reduction, round-synchronised
            stamp("  sum-checks 1 enqueued");
            for (auto& f : second_wave) f();            // Libra phase-2 bookkeeping (queued)
            flush_bookkeeping();
            prodsum_flush(st, pool, ps_queue, keep);
            stamp("node launches: end");
        };
        // Schedule: the Lasso node is the long chain (three quarters of the prove): its enqueue starts first and the node launches are
        // issued from inside it, behind its limb split and counters (the other orders - node reductions first, behind the hashes,
        // behind the last launch - measured the same 14.1-14.7 ms in round 4: both chains are VALU-issue bound)
        if (lasso_deferred) {
            lasso_mid = node_launches;
            lasso_mid_at = 1;
            ctx->arena_skip_to_high();
            lasso_deferred();
        } else {
            node_launches();
            if (lasso_deferred) {
                ctx->arena_skip_to_high();  // scopes released during the walk may still be in use on the other stream: do not recycle them
                lasso_deferred();
            }
        }
        stamp("lasso node returned (its stream is drained, its transcript replayed)");
        res_sync(ctx, st, "hg_prove_bn254: sync");
        stamp("node stream drained");
        *out.val = fr_to_mont(*out_slot);
        for (auto& f : replay) f();
        stamp("replayed");
    }
};

// The BN254 prove runs on its own pair of streams with priorities (Lasso node high, node reductions low): its two halves are both
// ALU-bound and the priority is what keeps the node reductions from slowing the long pole (19.6 ms against 22.0 ms without). The
// Goldilocks prover's streams carry no priority (see hg_create: its cached launch graph replays badly next to a high-priority
// stream). Created on first use; the context's stream pointers are swapped for the duration of the call.
struct BnStreams {
    hg_ctx* ctx;
    hipStream_t s1, s2;
    explicit BnStreams(hg_ctx* c) : ctx(c), s1(c->stream), s2(c->stream2) {
        if (!ctx->bn_stream_hi) {
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || lo == hi) return;   // no priorities here: keep the plain streams
            hipc(hipStreamCreateWithPriority(&ctx->bn_stream_hi, hipStreamNonBlocking, hi), "hipStreamCreate");
            hipc(hipStreamCreateWithPriority(&ctx->bn_stream_lo, hipStreamNonBlocking, lo), "hipStreamCreate");
        }
        hipc(hipStreamSynchronize(s1), "sync"); hipc(hipStreamSynchronize(s2), "sync");
        ctx->stream = ctx->bn_stream_hi; ctx->stream2 = ctx->bn_stream_lo;
    }
    ~BnStreams() {
        if (ctx->stream != s1) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamSynchronize(ctx->stream2); }
        ctx->stream = s1; ctx->stream2 = s2;
    }
};
void prove_bn254(hg_ctx* ctx, const hg_pk* pk, const Witness& w, std::vector<uint8_t>& proof, double* ms) {
    if (!pk->ctx) throw Error("hg_prove_bn254: host-only prover key");
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    BnStreams swap(ctx);
    BnProver P(ctx, pk);
    P.run(w, ms);
    proof = std::move(P.proof);
}
