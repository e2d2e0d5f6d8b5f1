// BfvEncrypt::verify::<Fr, Fr> with the table-sized work on the device [REF bfv-gkr/src/sk_encryption_circuit.rs:462-517, 614-626;
// verify_gkr :509-510; lasso/src/memory_checking/verifier.rs:130-176] - included by bn254.hip behind bn254_gkr.inc, inside namespace
// hg::bn, so that it launches that translation unit's BN254 bookkeeping kernels. The BN254 counterpart of verifier_dev.hip: the walk
// (verifier.cpp, verify_with_backend<BnField>: proof parsing, round-polynomial checks, Lasso scalars) stays on the host and only
// RECORDS the table-sized sums; finish() launches them by kind over job arrays on one stream and synchronises once:
//   eq tables of the claim points and of the sum-check points (offsets into the challenge chain, uploaded once in Montgomery form),
//   the constant-gate sums (k_bn_const_sum), the Libra gathers over the reverse CSR wiring (k_bn_gather_T_jobs / k_bn_gather_B_jobs),
//   the zkCNN DFT-row tables (k_bn_fft_part_jobs / k_bn_fft_tab_jobs), and every dot product of a table with an eq table in two
//   launches (k_bn_vdot_jobs / k_bn_vdot_reduce), the MLE evaluations of the public inputs and of ct0is among them.
// From the ciphertext (hg_verify_public_device_bn254): the public tables stay the compact signed coefficients of hg_instance and
// are evaluated by k_bn_vdot_compact_jobs; the claims on the secret inputs launch nothing and are handed back.
// Mode 0 only (the protocol modes are Goldilocks-only): every evaluation point is a run of the fixed Fr chain (BnChain).

// ---- eq tables from chain offsets ---------------------------------------------------------------------------------------------
// out = sum_a alpha_a eq(point_a, .) over n variables (little-endian: bit b of the index is coordinate b), in two launches. Prep: per
// (table, claim) a low table A over the first min(n, 8) coordinates (2^min(n,8) entries) and a high table B over the others with
// alpha_a folded in (2^(n-8) entries, or the single entry alpha_a), every entry a direct product of its factors (at most 12 at c3).
// Fill: out[x] = sum_a A_a[x mod 256] B_a[x div 256] - the outer product of k_bn_eq_outer_jobs, summed over the claims in one column
// accumulator (one Montgomery reduction per entry, not per claim).
constexpr int VEQ_A = 256;
__host__ __device__ inline size_t veq_stride(int n) { return VEQ_A + ((size_t)1 << (n > 8 ? n - 8 : 0)); }   // A then B, per claim
struct VeqPrep { Fr* ab; size_t point_off, alpha_off; int n, unit; };   // ab: this claim's A (VEQ_A entries) and B
__global__ __launch_bounds__(256) void k_bn_veq_prep(const VeqPrep* __restrict__ jobs, const Fr* __restrict__ chal) {
    const VeqPrep& J = jobs[blockIdx.y];
    const int m = J.n < 8 ? J.n : 8, h = J.n - m;
    const Fr one = fr_one_mont();
    if (blockIdx.x == 0) {   // A
        const int x = threadIdx.x;
        if (x >= (1 << m)) return;
        Fr acc = one;
        for (int b = 0; b < m; b++) { const Fr r = chal[J.point_off + b]; acc = fr_mul_wide(acc, (x >> b) & 1 ? r : fr_sub(one, r)); }
        J.ab[x] = acc;
        return;
    }
    const size_t y = (size_t)(blockIdx.x - 1) * 256 + threadIdx.x;
    if (y >= ((size_t)1 << h)) return;
    Fr acc = J.unit ? one : chal[J.alpha_off];
    for (int b = 0; b < h; b++) { const Fr r = chal[J.point_off + m + b]; acc = fr_mul_wide(acc, (y >> b) & 1 ? r : fr_sub(one, r)); }
    J.ab[VEQ_A + y] = acc;
}
struct VeqFill { Fr* out; const Fr* ab; int n, na; };   // ab: na claims, veq_stride(n) entries each
__global__ __launch_bounds__(256) void k_bn_veq_fill(const VeqFill* __restrict__ jobs) {
    const VeqFill& J = jobs[blockIdx.y];
    const int m = J.n < 8 ? J.n : 8;
    const size_t total = (size_t)1 << J.n, lmask = ((size_t)1 << m) - 1, stride = veq_stride(J.n);
    for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < total; x += (size_t)gridDim.x * 256) {
        WCol w = wcol_zero();
        for (int a = 0; a < J.na; a++) {
            const Fr* ab = J.ab + (size_t)a * stride;
            wcol_mac(w, ab[x & lmask], ab[VEQ_A + (x >> m)]);
        }
        J.out[x] = wcol_reduce(w);   // na <= MAX_CLAIMS = 32 products of canonical residues: < 32 r^2, inside wcol_reduce's 2^10 r^2
    }
}

// ---- dot products ---------------------------------------------------------------------------------------------------------------
// job q: sum_i a_q[i] b_q[i], a an Fr table or a table of small signed integers (the witness form: z >= 0 as z, z < 0 as GL_P - |z|,
// lifted into Fr by the rule of k_bn_lift_jobs), b an eq table. Launch 1 deals every job's entries out in tiles of VD_TILE to a
// flat grid (thousands of workgroups at c3 for 256 CUs, whatever the mix of job sizes); a workgroup writes one partial per tile.
// Launch 2: one workgroup per job adds its tiles' partials into the job's result slot.
// Arithmetic: a thread multiply-accumulates its VD_ITEMS entries into one column accumulator (bn254_wide.hpp) and reduces ONCE:
//   Fr tables:  both operands canonical (< r), so the sum is below VD_ITEMS r^2 = 2^5 r^2 - inside lz_reduce's 2^12 r^2 bound.
//               value(w) R^-1 = sum a~ b~ R^-1 = (sum a b) R: already the Montgomery form of the sum.
//   integers:   |z| < 2^63 times (b~ or r - b~) <= r: below VD_ITEMS 2^63 r; reduce gives sum z b (plain), one fr_to_mont per thread.
constexpr int VD_ITEMS = 32, VD_TILE = 256 * VD_ITEMS;
struct VdotJob { const void* a; const Fr* b; size_t n; Fr* out; int blk0, nblk, a_is_int, pad; };
__device__ __forceinline__ Fr vd_negate_if(const Fr& e, bool neg) {   // neg ? r - e : e, for e in [0, r)
    const u64 P[4] = {FR_P0, FR_P1, FR_P2, FR_P3};
    u64 d[4], borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u64 t = P[i] - e.l[i], b1 = P[i] < e.l[i] ? 1 : 0;
        d[i] = t - borrow;
        borrow = b1 | (t < borrow ? 1 : 0);
    }
    return neg ? fr_make(d[0], d[1], d[2], d[3]) : e;
}
__global__ __launch_bounds__(256) void k_bn_vdot_jobs(const VdotJob* __restrict__ jobs, const int* __restrict__ blk_job, Fr* __restrict__ partials) {
    __shared__ Fr sm[256];
    const VdotJob& J = jobs[blk_job[blockIdx.x]];
    const size_t base = (size_t)(blockIdx.x - J.blk0) * VD_TILE + threadIdx.x, n = J.n;
    const Fr* __restrict__ b = J.b;
    WCol w = wcol_zero();
    Fr s;
    if (J.a_is_int) {
        const u64* __restrict__ a = static_cast<const u64*>(J.a);
        for (int k = 0; k < VD_ITEMS; k++) {
            const size_t i = base + (size_t)k * 256;
            if (i >= n) break;
            const u64 v = a[i];
            const bool neg = v >= (1ULL << 63);
            wcol_mac_u64(w, neg ? GL_P - v : v, vd_negate_if(b[i], neg));
        }
        s = fr_to_mont(lz_canon(lz_reduce(w)));
    } else {
        const Fr* __restrict__ a = static_cast<const Fr*>(J.a);
        for (int k = 0; k < VD_ITEMS; k++) {
            const size_t i = base + (size_t)k * 256;
            if (i >= n) break;
            wcol_mac(w, a[i], b[i]);
        }
        s = lz_canon(lz_reduce(w));
    }
    s = block_sum_fr(s, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_bn_vdot_reduce(const VdotJob* __restrict__ jobs, const Fr* __restrict__ partials) {
    __shared__ Fr sm[256];
    const VdotJob& J = jobs[blockIdx.x];
    Fr a = fr_zero();
    for (int q = threadIdx.x; q < J.nblk; q += 256) a = fr_add(a, partials[(size_t)J.blk0 + q]);
    a = block_sum_fr(a, sm);
    if (threadIdx.x == 0) *J.out = fr_from_mont(a);   // canonical for the host
}

// The MLE evaluations of the public tables from the compact signed coefficients of hg_instance (the Fr counterpart of
// k_vdot_compact_jobs, verifier_dev.hip). A job is nblk blocks of n = 2^log2_n coefficients and of 2n eq entries each; its WORD
// indices t < nblk n are dealt out in tiles of VD_TILE to a flat grid through blk_job, as the jobs of k_bn_vdot_jobs are. Word t is
// block b = t >> log2_n, r = t & (n-1): eq entry b 2n + lo + r meets coefficient n-1-r of block b (ais[i]: one block, lo = 0; ct0is:
// k blocks, lo = n-1), so the 32-byte eq loads of a wavefront are consecutive and the coefficients are read descending over the same
// cache lines. Only the half of each eq table that meets a non-padding word is read. The sign stays in registers: |z| times eq, or
// times r - eq for a negative z; a zero coefficient is skipped.
// Arithmetic: the integer rule of VD_ITEMS above. An instance holds |z| <= (q_i-1)/2 < 2^61 (instance_from_ciphertext), so a thread's
// VD_ITEMS products stay below VD_ITEMS 2^61 r, far inside lz_reduce's 2^12 r^2; one lz_reduce and one fr_to_mont per thread.
// Launch 2 is k_bn_vdot_reduce over a VdotJob per compact job (blk0, nblk = its tiles, out).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 54 VGPRs, no scratch, 8 waves per SIMD.
struct BnCompactDotJob { const int64_t* c; const Fr* eq; u32 log2_n, nblk, lo; int blk0; };
__global__ __launch_bounds__(256) void k_bn_vdot_compact_jobs(const BnCompactDotJob* __restrict__ jobs, const int* __restrict__ blk_job, Fr* __restrict__ partials) {
    __shared__ Fr sm[256];
    const BnCompactDotJob& J = jobs[blk_job[blockIdx.x]];
    const size_t n = (size_t)1 << J.log2_n, total = n * J.nblk;
    const size_t base = (size_t)(blockIdx.x - J.blk0) * VD_TILE + threadIdx.x;
    const int64_t* __restrict__ c = J.c;
    const Fr* __restrict__ eq = J.eq + J.lo;
    WCol w = wcol_zero();
    for (int k = 0; k < VD_ITEMS; k++) {
        const size_t t = base + (size_t)k * 256;
        if (t >= total) break;
        const size_t b = t >> J.log2_n, r = t & (n - 1);
        const int64_t z = c[b * n + (n - 1 - r)];
        if (!z) continue;
        const bool neg = z < 0;
        wcol_mac_u64(w, neg ? (u64)0 - (u64)z : (u64)z, vd_negate_if(eq[b * 2 * n + r], neg));
    }
    Fr s = fr_to_mont(lz_canon(lz_reduce(w)));
    s = block_sum_fr(s, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- the backend ----------------------------------------------------------------------------------------------------------------
struct BnDevBackend : VerifyBackendT<Fr> {
    hg_ctx* ctx;
    const hg_pk* pk;
    hipStream_t st;
    DevPool& pool;
    std::vector<const u64*> d_inputs;
    std::vector<size_t> input_len;
    const u64* d_ct0is = nullptr;
    size_t ct0is_len = 0;
    std::vector<ResRef> slots;        // ticket -> result slot (bn254.hip res_slots: the bound check of the result buffer)
    // the challenge chain on the host (Montgomery), as far as the walk has used it; uploaded once in finish()
    // own_chain (hg_claims_settle_bn254, hg_instance_mle_bn254: the points are the caller's): chm IS the chain, set by the caller
    std::vector<Fr> chm;
    size_t chain_need = 0;
    bool own_chain = false;
    const Fr& chain_at(size_t i) {
        if (own_chain && chm.size() <= i) throw Error("verifier: a job reads past the points it was given");
        if (chm.size() <= i) {
            const size_t have = chm.size(), want = std::max(i + 1, have + 2048);
            chm.resize(want);
            bn_chain_copy(have, want - have, chm.data() + have);
            for (size_t q = have; q < want; q++) chm[q] = fr_to_mont(chm[q]);
        }
        return chm[i];
    }
    void need(size_t end) { chain_need = std::max(chain_need, end); }
    // the node being checked
    int node = -1;
    Fr *eqc = nullptr, *eqx = nullptr, *eqy = nullptr;
    dev::ClaimSet cs;
    size_t u_base = 0;
    // recorded work
    std::vector<VeqPrep> preps;
    std::vector<VeqFill> fills;
    int prep_max_h = 0, fill_max_n = 0;
    std::map<std::pair<size_t, int>, Fr*> eq_cache;   // (chain offset, variables) -> eq table of a single unit-weight point
    struct ConstSum { const hg_pk::NodeDev* nd; const Fr* eqc; int log2_G, log2_R; Fr* out; };
    std::vector<ConstSum> consts;
    std::vector<BnGatherTJob> gts;
    std::vector<BnGatherBJob> gbs;
    size_t gt_max = 0, gb_max = 0;
    std::vector<FftPartJob> fft_parts;
    std::vector<FftTabJob> fft_tabs;
    std::vector<std::vector<FftTabClaim>> fft_claims;   // per fft_tabs entry
    size_t part_max = 0, tab_max = 0;
    std::map<std::pair<int, int>, const Fr*> W;        // (log2 size, inverse) -> w^i
    std::map<int, Fr> inv_size;
    std::vector<VdotJob> dots;
    // hg_verify_public_device_bn254 / hg_instance_mle_bn254: the public tables as compact signed coefficients in HBM (cp set: a of
    // k*n words, ct0 of k*n words); mle_input / mle_ct0is then record compact dot jobs (cdot_slots: what k_bn_vdot_reduce reads)
    const Params* cp = nullptr;
    const int64_t *d_ca = nullptr, *d_cct0 = nullptr;
    std::vector<BnCompactDotJob> cdots;
    std::vector<VdotJob> cdot_slots;
    std::vector<Fr> h_u;                               // the phase-1 evaluations of the Vanilla nodes with a phase 2 (canonical), back to back
    double t_begin = 0;                                // wall_ms() at the start of the verification (HG_TIMES=verify)
    const char* who = "verify_device_bn254";           // the entry the HG_TIMES=verify lines name

    BnDevBackend(hg_ctx* c, const hg_pk* k, DevPool& p) : ctx(c), pk(k), st(c->stream), pool(p) { memset(&cs, 0, sizeof(cs)); }
    int slot() {
        slots.push_back(res_slots(ctx, 1));
        return (int)slots.size() - 1;
    }
    Fr* eq_of(int nvars, const dev::ClaimSet& c) {
        Fr* out = pool.get<Fr>((size_t)1 << nvars);
        const size_t stride = veq_stride(nvars);
        Fr* ab = pool.get<Fr>(stride * (size_t)c.n);
        for (int a = 0; a < c.n; a++) {
            VeqPrep P;
            memset(&P, 0, sizeof(P));
            P.ab = ab + (size_t)a * stride; P.point_off = c.point_off[a]; P.n = nvars; P.unit = c.unit_alpha;
            P.alpha_off = c.alpha_off + a;
            preps.push_back(P);
            need(P.point_off + nvars);
            if (!P.unit) need(P.alpha_off + 1);
        }
        fills.push_back(VeqFill{out, ab, nvars, c.n});
        prep_max_h = std::max(prep_max_h, nvars > 8 ? nvars - 8 : 0);
        fill_max_n = std::max(fill_max_n, nvars);
        return out;
    }
    Fr* eq_single(int nvars, size_t off) {
        auto hit = eq_cache.find({off, nvars});
        if (hit != eq_cache.end()) return hit->second;
        dev::ClaimSet c;
        memset(&c, 0, sizeof(c));
        c.n = 1; c.unit_alpha = 1; c.point_off[0] = off;
        return eq_cache[{off, nvars}] = eq_of(nvars, c);
    }
    int dot(const void* a, bool a_is_int, const Fr* b, size_t n) {
        const int t = slot();
        VdotJob J;
        memset(&J, 0, sizeof(J));
        J.a = a; J.b = b; J.n = n; J.out = slots[t].dev; J.a_is_int = a_is_int ? 1 : 0;
        dots.push_back(J);
        return t;
    }
    const Fr* omega_table(int L, bool inverse) {
        auto hit = W.find({L, (int)inverse});
        if (hit != W.end()) return hit->second;
        if (L > 28) throw Error("bn254: two-adicity is 28");
        const size_t N = (size_t)1 << L;
        Fr* t = pool.get<Fr>(N);
        Fr wr = fr_root_of_unity(L);
        if (inverse) wr = fr_inv(wr);
        k_bn_powers<<<grid_of(N), 256, 0, st>>>(t, wr, N);
        return W[{L, (int)inverse}] = t;
    }

    void begin_node(int id, const ClaimOffs& cl) override {
        node = id;
        const HNode& n = pk->circuit.nodes[id];
        if (cl.point_off.size() > (size_t)dev::MAX_CLAIMS) throw Error("verifier: too many claims on one node");
        memset(&cs, 0, sizeof(cs));
        cs.n = (int)cl.point_off.size();
        cs.unit_alpha = cl.unit ? 1 : 0;
        cs.alpha_off = cl.alpha_off;
        for (int a = 0; a < cs.n; a++) cs.point_off[a] = cl.point_off[a];
        eqc = n.kind == NK_VANILLA ? (cs.n == 1 && cs.unit_alpha ? eq_single(n.log2_out(), cs.point_off[0]) : eq_of(n.log2_out(), cs)) : nullptr;
        eqx = eqy = nullptr;
    }
    int const_sum() override {
        const HNode& n = pk->circuit.nodes[node];
        const int t = slot();
        consts.push_back(ConstSum{&pk->node_dev[node], eqc, n.log2_sub_out, n.log2_reps, slots[t].dev});
        return t;
    }
    void set_x(size_t x_off) override {
        const HNode& n = pk->circuit.nodes[node];
        eqx = eq_single(n.kind == NK_VANILLA ? n.log2_sub_in + n.log2_reps : n.log2_size, x_off);
    }
    std::vector<int> lin_terms() override {
        const HNode& n = pk->circuit.nodes[node];
        const hg_pk::NodeDev& nd = pk->node_dev[node];
        const size_t SR = (size_t)1 << (n.log2_sub_in + n.log2_reps);
        std::vector<int> tk(n.arity, -1);
        for (int i = 0; i < n.arity; i++) {
            if (!n.left_use[i] || !nd.lin[i].ptr) continue;
            Fr* T = pool.get<Fr>(SR);
            BnGatherTJob gj;
            memset(&gj, 0, sizeof(gj));
            gj.lin = nd.lin[i];   // (no mul part: the verifier's linear term has no input tables)
            gj.eqc = eqc; gj.T = T; gj.log2_S = n.log2_sub_in; gj.log2_G = n.log2_sub_out; gj.log2_R = n.log2_reps;
            gts.push_back(gj);
            gt_max = std::max(gt_max, SR);
            tk[i] = dot(T, false, eqx, SR);
        }
        return tk;
    }
    void set_y(size_t y_off, const std::vector<Fr>& u) override {
        const HNode& n = pk->circuit.nodes[node];
        if (n.arity > dev::PS_MAX_PAIRS) throw Error("verifier: arity too large");
        eqy = eq_single(n.log2_sub_in + n.log2_reps, y_off);
        u_base = h_u.size();
        for (const Fr& x : u) h_u.push_back(fr_from_mont(x));   // k_bn_gather_B_jobs reads them canonical, as the prover's result slots
    }
    std::vector<int> mul_terms() override {
        const HNode& n = pk->circuit.nodes[node];
        const hg_pk::NodeDev& nd = pk->node_dev[node];
        const size_t SR = (size_t)1 << (n.log2_sub_in + n.log2_reps);
        std::vector<int> tk(n.arity, -1);
        for (int i = 0; i < n.arity; i++) {
            if (!n.right_use[i] || !nd.mulR[i].ptr) continue;
            Fr* B = pool.get<Fr>(SR);
            BnGatherBJob bj;
            memset(&bj, 0, sizeof(bj));
            bj.m = nd.mulR[i]; bj.eqc = eqc; bj.eqx = eqx; bj.B = B;   // bj.fin: the uploaded evaluations, set in finish()
            for (int q = 0; q < dev::PS_MAX_PAIRS; q++) bj.us.slot[q] = q < n.arity ? (int)(u_base + q) : -1;
            bj.arity = n.arity; bj.log2_S = n.log2_sub_in; bj.log2_G = n.log2_sub_out; bj.log2_R = n.log2_reps;
            gbs.push_back(bj);
            gb_max = std::max(gb_max, SR);
            tk[i] = dot(B, false, eqy, SR);
        }
        return tk;
    }
    int fft_term() override {   // the DFT-row table of bn254_gkr.inc fft_node: direct factors b < s1, part tables over [s1, s2) and [s2, L)
        const HNode& n = pk->circuit.nodes[node];
        const int L = n.log2_size;
        const size_t N = (size_t)1 << L;
        const Fr* Wt = omega_table(L, n.inverse);
        if (n.inverse && !inv_size.count(L)) inv_size[L] = fr_inv(fr_small((u64)N));
        const Fr scale = n.inverse ? inv_size[L] : fr_one_mont();
        const int s1 = std::min(4, L), s2 = std::min(8, L);
        Fr* F = pool.get<Fr>(N);
        std::vector<FftTabClaim> tc_all;
        for (int a = 0; a < cs.n; a++) {
            FftPartJob pj;
            memset(&pj, 0, sizeof(pj));
            for (int b = 0; b < L; b++) pj.pt.r[b] = chain_at(cs.point_off[a] + b);
            pj.W = Wt; pj.L = L;
            FftTabClaim tc;
            memset(&tc, 0, sizeof(tc));
            for (int b = 0; b < s1; b++) tc.r[b] = pj.pt.r[b];
            tc.coef = cs.unit_alpha ? scale : fr_mul(chain_at(cs.alpha_off + a), scale);
            if (s2 > s1) { tc.T1 = pj.T = pool.get<Fr>((size_t)1 << (L - s1)); pj.b_lo = s1; pj.b_hi = s2; fft_parts.push_back(pj); part_max = std::max(part_max, (size_t)1 << (L - s1)); }
            if (L > s2) { tc.T2 = pj.T = pool.get<Fr>((size_t)1 << (L - s2)); pj.b_lo = s2; pj.b_hi = L; fft_parts.push_back(pj); part_max = std::max(part_max, (size_t)1 << (L - s2)); }
            tc_all.push_back(tc);
        }
        FftTabJob tj;
        memset(&tj, 0, sizeof(tj));
        tj.F = F; tj.W = Wt; tj.L = L; tj.s1 = s1; tj.s2 = s2; tj.nclaims = cs.n;
        fft_tabs.push_back(tj);
        fft_claims.push_back(tc_all);
        tab_max = std::max(tab_max, N);
        return dot(F, false, eqx, N);
    }
    void end_node() override { node = -1; }
    int mle_int(const u64* tab, size_t len, size_t point_off, int nvars) {
        if (nvars < 0 || nvars > 40 || ((size_t)1 << nvars) != len) throw Error("verifier: claim point does not fit the input table");
        return dot(tab, true, eq_single(nvars, point_off), len);
    }
    int mle_compact(const int64_t* c, int nblk, size_t lo, size_t point_off, int nvars) {
        int lg = 0;
        while ((1 << lg) < nblk) lg++;
        if (nvars != cp->L + lg) throw Error("verifier: a point of the wrong length for a public table");   // (the job reads nblk * 2n eq entries)
        const int t = slot();
        BnCompactDotJob J;
        memset(&J, 0, sizeof(J));
        J.c = c; J.eq = eq_single(nvars, point_off); J.log2_n = (u32)cp->n_log2; J.nblk = (u32)nblk; J.lo = (u32)lo;
        cdots.push_back(J);
        VdotJob S;
        memset(&S, 0, sizeof(S));
        S.out = slots[t].dev;
        cdot_slots.push_back(S);
        return t;
    }
    int mle_input(size_t k, size_t point_off, int nvars) override {
        if (cp) {
            if (k < 3 || k >= 3 + (size_t)cp->k) throw Error("verifier: input " + std::to_string(k) + " is not a public table");
            return mle_compact(d_ca + (k - 3) * cp->PZ(), 1, 0, point_off, nvars);
        }
        if (k >= d_inputs.size()) throw Error("verifier: no such input table");
        return mle_int(d_inputs[k], input_len[k], point_off, nvars);
    }
    int mle_ct0is(size_t point_off, int nvars) override {
        if (cp) return mle_compact(d_cct0, cp->k, cp->PZ() - 1, point_off, nvars);
        return mle_int(d_ct0is, ct0is_len, point_off, nvars);
    }

    void finish() override {
        const bool times = hg_times("verify");   // read at every call (host.hpp)
        const double t0 = wall_ms();
        if (times) {
            size_t n_fr = 0, n_int = 0;
            for (auto& d : dots) (d.a_is_int ? n_int : n_fr) += d.n;
            fprintf(stderr, "[hg] %s: host walk ended at %.2f ms\n", who, t0 - t_begin);
            hipc(hipStreamSynchronize(st), "sync");
            fprintf(stderr, "[hg] %s: uploads drained %.2f ms after the walk ended; %zu eq tables (%zu claim tables), %zu gathers, %zu + %zu, %zu dots (%zu Fr x Fr entries, %zu integer x Fr entries), %zu compact dots\n",
                    who, wall_ms() - t0, fills.size(), preps.size(), gts.size(), gbs.size(), fft_tabs.size(), dots.size(), n_fr, n_int, cdots.size());
        }
        auto lap = [&](const char* what) { if (times) { hipc(hipStreamSynchronize(st), "sync"); fprintf(stderr, "[hg] %s: %8.2f ms  %s\n", who, wall_ms() - t0, what); } };
        // the chain run the walk used, then every job array, staged side by side and copied over in one transfer (bn_flush)
        if (!own_chain || chain_need) (void)chain_at(chain_need ? chain_need - 1 : 0);
        const Fr* d_chal = bn_stage(ctx, chm.data(), std::max<size_t>(chain_need, 1));
        const VeqPrep* d_prep = preps.empty() ? nullptr : bn_stage(ctx, preps.data(), preps.size());
        const VeqFill* d_fill = fills.empty() ? nullptr : bn_stage(ctx, fills.data(), fills.size());
        const BnGatherTJob* d_gt = gts.empty() ? nullptr : bn_stage(ctx, gts.data(), gts.size());
        if (!gbs.empty()) {
            const Fr* d_u = bn_stage(ctx, h_u.data(), h_u.size());
            for (auto& j : gbs) j.fin = d_u;
        }
        const BnGatherBJob* d_gb = gbs.empty() ? nullptr : bn_stage(ctx, gbs.data(), gbs.size());
        for (size_t q = 0; q < fft_tabs.size(); q++) fft_tabs[q].claims = bn_stage(ctx, fft_claims[q].data(), fft_claims[q].size());
        const FftPartJob* d_part = fft_parts.empty() ? nullptr : bn_stage(ctx, fft_parts.data(), fft_parts.size());
        const FftTabJob* d_tab = fft_tabs.empty() ? nullptr : bn_stage(ctx, fft_tabs.data(), fft_tabs.size());
        std::vector<int> blk_job;
        for (size_t q = 0; q < dots.size(); q++) {
            dots[q].blk0 = (int)blk_job.size();
            dots[q].nblk = (int)((dots[q].n + VD_TILE - 1) / VD_TILE);
            blk_job.insert(blk_job.end(), (size_t)dots[q].nblk, (int)q);
        }
        const VdotJob* d_dots = dots.empty() ? nullptr : bn_stage(ctx, dots.data(), dots.size());
        const int* d_blk_job = blk_job.empty() ? nullptr : bn_stage(ctx, blk_job.data(), blk_job.size());
        std::vector<int> cblk_job;
        for (size_t q = 0; q < cdots.size(); q++) {
            const size_t words = (size_t)cdots[q].nblk << cdots[q].log2_n;
            cdots[q].blk0 = cdot_slots[q].blk0 = (int)cblk_job.size();
            cdot_slots[q].nblk = (int)((words + VD_TILE - 1) / VD_TILE);
            cblk_job.insert(cblk_job.end(), (size_t)cdot_slots[q].nblk, (int)q);
        }
        const BnCompactDotJob* d_cdots = cdots.empty() ? nullptr : bn_stage(ctx, cdots.data(), cdots.size());
        const VdotJob* d_cslots = cdots.empty() ? nullptr : bn_stage(ctx, cdot_slots.data(), cdot_slots.size());
        const int* d_cblk_job = cblk_job.empty() ? nullptr : bn_stage(ctx, cblk_job.data(), cblk_job.size());
        bn_flush(ctx, st);
        lap("descriptors uploaded");
        if (d_prep) {
            k_bn_veq_prep<<<dim3(1 + (unsigned)(((size_t)1 << prep_max_h) + 255) / 256, (unsigned)preps.size()), 256, 0, st>>>(d_prep, d_chal);
            k_bn_veq_fill<<<dim3((unsigned)std::min<size_t>((((size_t)1 << fill_max_n) + 255) / 256, 1024), (unsigned)fills.size()), 256, 0, st>>>(d_fill);
        }
        lap("eq tables");
        if (!consts.empty()) {
            Fr* d_part = pool.get<Fr>(1024);   // one after the other on the stream: one partials buffer serves them all
            for (const ConstSum& c : consts) {
                const size_t total = c.nd->nconst << c.log2_R;
                const int grid = (int)std::max<size_t>(1, std::min<size_t>((total + BN_TPB - 1) / BN_TPB, 1024));
                k_bn_const_sum<<<grid, BN_TPB, 0, st>>>(c.nd->const_gate, c.nd->const_coef, c.nd->nconst, c.eqc, c.log2_G, c.log2_R, d_part);
                k_bn_reduce<<<1, BN_TPB, 0, st>>>(d_part, grid, 1, c.out);
            }
        }
        lap("constant sums");
        if (d_gt) k_bn_gather_T_jobs<<<dim3((unsigned)std::min<size_t>((gt_max + BN_TPB - 1) / BN_TPB, 2048), (unsigned)gts.size()), BN_TPB, 0, st>>>(d_gt);
        lap("phase-1 gathers");
        if (d_part) k_bn_fft_part_jobs<<<dim3((unsigned)std::min<size_t>((part_max + 255) / 256, 2048), (unsigned)fft_parts.size()), 256, 0, st>>>(d_part);
        if (d_tab) k_bn_fft_tab_jobs<<<dim3((unsigned)std::min<size_t>((tab_max + 255) / 256, 2048), (unsigned)fft_tabs.size()), 256, 0, st>>>(d_tab);
        lap("DFT-row tables");
        if (d_gb) k_bn_gather_B_jobs<<<dim3((unsigned)std::min<size_t>((gb_max + BN_TPB - 1) / BN_TPB, 2048), (unsigned)gbs.size()), BN_TPB, 0, st>>>(d_gb);
        lap("phase-2 gathers");
        if (d_dots) {
            Fr* part = pool.get<Fr>(blk_job.size());
            k_bn_vdot_jobs<<<(unsigned)blk_job.size(), 256, 0, st>>>(d_dots, d_blk_job, part);
            k_bn_vdot_reduce<<<(unsigned)dots.size(), 256, 0, st>>>(d_dots, part);
        }
        if (d_cdots) {
            Fr* part = pool.get<Fr>(cblk_job.size());
            k_bn_vdot_compact_jobs<<<(unsigned)cblk_job.size(), 256, 0, st>>>(d_cdots, d_cblk_job, part);
            k_bn_vdot_reduce<<<(unsigned)cdots.size(), 256, 0, st>>>(d_cslots, part);
        }
        lap("dot products");
        res_sync(ctx, st, "verifier: synchronise");
    }
    Fr value(int t) const override { return fr_to_mont(*slots[t].host); }
};

// public inputs and ct0is are uploaded as the integers they are (the dot-product kernel lifts them), the proof is parsed on the host;
// "" = accepted
std::string verify_proof_device_bn254(hg_ctx* ctx, const hg_pk* pk, const Witness& w, const uint8_t* proof, size_t len) {
    if (!pk->ctx) throw Error("hg_verify_device_bn254: host-only prover key");
    const double tv0 = wall_ms();
    struct Total { double t0; ~Total() { if (hg_times("verify")) fprintf(stderr, "[hg] verify_device_bn254: %.2f ms in all\n", wall_ms() - t0); } } total{tv0};
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    DevPool pool(ctx);   // (rewinds the arena on the way out, behind the drain below)
    // Rejection is a normal outcome and leaves kernels and staged copies queued (the walk returns from the middle of the proof), and
    // an hg::Error may leave from any upload: drain the stream on EVERY way out before the caller may reuse the staging buffer and
    // the arena or free the witness whose uploads may still be pending (verifier_dev.hip: the same guard).
    Drain drain{ctx->stream};
    const Params& p = pk->params;
    BnDevBackend D(ctx, pk, pool);
    D.t_begin = tv0;
    const size_t SZ = p.SZ();
    auto up = [&](const u64* src, size_t n) {
        D.input_len.push_back(n);
        u64* d = pool.get<u64>(n);
        hipc(hipMemcpyAsync(d, src, n * 8, hipMemcpyHostToDevice, ctx->stream), "verifier: upload inputs");
        return (const u64*)d;
    };
    D.d_inputs.push_back(up(w.s.data(), SZ));
    D.d_inputs.push_back(up(w.e.data(), SZ));
    D.d_inputs.push_back(up(w.k1.data(), SZ));
    for (int i = 0; i < p.k; i++) D.d_inputs.push_back(up(&w.ais[(size_t)i * SZ], SZ));
    for (int i = 0; i < p.k; i++) D.d_inputs.push_back(up(&w.r1is[(size_t)i * SZ], SZ));
    D.d_inputs.push_back(up(w.r2is.data(), w.r2is.size()));
    D.d_ct0is = up(w.ct0is.data(), w.ct0is.size());
    D.ct0is_len = D.input_len.back();
    D.input_len.pop_back();
    if (hg_times("verify")) fprintf(stderr, "[hg] verify_device_bn254: inputs enqueued at %.2f ms\n", wall_ms() - tv0);
    return verify_proof_with_bn254(D, p, pk->lasso, pk->circuit, proof, len);
}

// ---- hg_verify_public_device_bn254, hg_claims_settle_bn254, hg_instance_mle_bn254 ------------------------------------------------
// (every way out of an entry drains the stream before the staging buffer, the arena or the caller's arrays are reused: see above)
static const int64_t* bn_upload_coeffs(hg_ctx* ctx, DevPool& pool, const std::vector<int64_t>& src) {
    int64_t* d = pool.get<int64_t>(src.size());
    hipc(hipMemcpyAsync(d, src.data(), src.size() * 8, hipMemcpyHostToDevice, ctx->stream), "verifier: upload the instance");
    return d;
}
static Fr fr_from_limbs_mont(const u64* v) { return fr_to_mont(fr_make(v[0], v[1], v[2], v[3])); }

// The public part of the verification on the device: the instance's 2 k n signed words are uploaded as they are (8.4 MB at n=32768
// k=16 against 30.9 MB of laid-out tables), the walk records compact dot jobs for ct0is and the ais claims and NOTHING for the secret
// inputs - their claims come back in `open`, value from the walk and point from the chain. One stream, one synchronisation.
std::string verify_public_device_bn254(hg_ctx* ctx, const hg_pk* pk, const Instance& inst, const uint8_t* proof, size_t len, std::vector<OpenClaimBn>& open) {
    if (!pk->ctx) throw Error("hg_verify_public_device_bn254: host-only prover key");
    const double tv0 = wall_ms();
    struct Total { double t0; ~Total() { if (hg_times("verify")) fprintf(stderr, "[hg] verify_public_device_bn254: %.2f ms in all\n", wall_ms() - t0); } } total{tv0};
    open.clear();
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    DevPool pool(ctx);
    Drain drain{ctx->stream};
    const Params& p = pk->params;
    BnDevBackend D(ctx, pk, pool);
    D.t_begin = tv0;
    D.who = "verify_public_device_bn254";
    D.cp = &p;
    D.d_ca = bn_upload_coeffs(ctx, pool, inst.a);
    D.d_cct0 = bn_upload_coeffs(ctx, pool, inst.ct0);
    VerifyPendingT<Fr> v = verify_walk_bn254(D, p, pk->lasso, pk->circuit, proof, len, true);
    if (!v.live()) return v.reason;
    D.finish();
    std::string why = verify_complete_bn254(v);
    if (why.empty()) for (const auto& cl : v.open) open.push_back(open_claim_bn254(cl));
    return why;
}

// The settle step on the device: the claim points staged as a chain of their own for the eq jobs, each witness table uploaded once
// (as the integers it holds: the integer path of k_bn_vdot_jobs lifts them), one dot product per claim, one synchronisation.
std::string claims_settle_device_bn254(hg_ctx* ctx, const Params& p, const Witness& w, const std::vector<OpenClaimBn>& claims) {
    if (claims.empty()) return "";
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    DevPool pool(ctx);
    Drain drain{ctx->stream};
    BnDevBackend D(ctx, nullptr, pool);
    D.own_chain = true;
    std::map<size_t, const u64*> d_tab;   // one upload per table, however many claims it carries
    std::vector<int> ticket;
    for (const OpenClaimBn& cl : claims) {
        int lg = 0;
        const u64* tab = input_table(p, w, cl.input, &lg);
        const size_t nv = cl.point4.size() / 4;
        if ((size_t)lg != nv) throw Error("hg_claims_settle_bn254: a claim on input " + std::to_string(cl.input) + " has " + std::to_string(nv) + " coordinates, its table " + std::to_string(lg) + " variables");
        auto it = d_tab.find(cl.input);
        if (it == d_tab.end()) {
            u64* d = pool.get<u64>((size_t)1 << lg);
            hipc(hipMemcpyAsync(d, tab, ((size_t)1 << lg) * 8, hipMemcpyHostToDevice, ctx->stream), "hg_claims_settle_bn254: upload inputs");
            it = d_tab.emplace(cl.input, d).first;
        }
        const size_t off = D.chm.size();
        for (size_t j = 0; j < nv; j++) D.chm.push_back(fr_from_limbs_mont(&cl.point4[4 * j]));
        ticket.push_back(D.mle_int(it->second, (size_t)1 << lg, off, lg));
    }
    D.finish();
    long long bad = -1;
    for (size_t i = 0; i < claims.size(); i++)
        if (memcmp(D.slots[ticket[i]].host->l, claims[i].value, 32) != 0 && (bad < 0 || (long long)claims[i].input < bad)) bad = (long long)claims[i].input;
    return bad < 0 ? std::string() : "input claim mismatch at input " + std::to_string(bad);
}

// one eq job and one compact dot job
void instance_mle_device_bn254(hg_ctx* ctx, const Params& p, const Instance& inst, int which, int index, const u64* point4, size_t nvars, u64 out4[4]) {
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    DevPool pool(ctx);
    Drain drain{ctx->stream};
    BnDevBackend D(ctx, nullptr, pool);
    D.own_chain = true;
    D.cp = &p;
    for (size_t j = 0; j < nvars; j++) D.chm.push_back(fr_from_limbs_mont(point4 + 4 * j));
    int t;
    if (which == 0) {
        D.d_ca = bn_upload_coeffs(ctx, pool, inst.a);
        t = D.mle_input(3 + (size_t)index, 0, (int)nvars);
    } else {
        D.d_cct0 = bn_upload_coeffs(ctx, pool, inst.ct0);
        t = D.mle_ct0is(0, (int)nvars);
    }
    D.finish();
    memcpy(out4, D.slots[t].host->l, 32);
}
