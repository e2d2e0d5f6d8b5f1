// hg_verify_device_batch_bn254: BfvEncrypt::verify::<Fr, Fr> of a run of proofs under one key in one device pass per group [REF
// bfv-gkr/src/sk_encryption_circuit.rs:462-517, 614-626] - included by bn254.hip behind bn254_verify.inc, inside namespace hg::bn,
// so that it launches that translation unit's BN254 job kernels. Every proof gets exactly the decision of verify_proof_device_bn254.
// The BN254 counterpart of verifier_batch.hip, in mode 0 only (every evaluation point is a run of the fixed Fr chain). The host side
// of the three steps - recorder, merge, input units, the loop over the groups - is verifier_merge.hpp, shared with Goldilocks; this
// file keeps the group-size rule, the Fr chain in Montgomery form, the lowering of a merged group and the input kernels:
//   1. The walks (verifier.cpp: verify_walk_bn254) run on the host threads, one proof each, against a backend that only RECORDS the
//      calls BnDevBackend makes (no device call, no arena or DevPool allocation: the bump allocator is not thread-safe).
//   2. The jobs of a group are merged. Chain offsets are absolute already, so every eq table, constant-gate sum, Libra phase-1
//      gather, DFT-row table and their dot products - they depend on the key only - are built once per group. Phase-2 gathers (they
//      read the proof's own phase-1 evaluations) and the input evaluations (they read the proof's own witness) are never shared.
//   3. One descriptor copy (the Fr chain in Montgomery form among the descriptors), one launch per kind through the single-proof
//      verifier's kernels, the input evaluations (k_bn_vin_dots), one synchronisation, then every proof's deferred comparisons
//      (verify_complete_bn254) on the host threads.
// The public inputs are the same signed integers in the same layout as over Goldilocks: they are staged and copied by the code of
// the Goldilocks batch (verifier_batch.hpp), so group g+1's copies and walks run while group g's kernels do.
// hg_verify_public_batch_bn254 is the same pass from the ciphertext (the batch form of verify_public_device_bn254, bn254_verify.inc):
// the walks run with public_only, the recording backend in its compact form, each proof's instance is staged as it is (2 k n signed
// words), k_bn_vin_dots<true> evaluates ais and ct0is from them, and the claims on the secret inputs come back from each proof's
// pending state.

// ---- the MLE evaluations of the public inputs -------------------------------------------------------------------------------------
// Work unit: one eq table and the P input tables evaluated at its point (mode 0: the group's tables of one input, so P is the group
// size). A workgroup owns VBN_TILE consecutive entries: it reads its eq tile once into registers and multiply-accumulates it against
// each of the P integer tables, one Montgomery reduction per thread and member, one partial per (member, wave): no barrier, and the
// next member's loads are issued ahead of this member's arithmetic. A second launch adds every member's partials into its result
// slot. HBM traffic: 8 B per input entry plus 32 / P B of eq. Resources (hipcc -Rpass-analysis=kernel-resource-usage): 230 VGPRs,
// no scratch, 2 waves per SIMD.
// Arithmetic (the lift of k_bn_vdot_jobs): an entry v >= 2^63 is the negative integer -(GL_P - v), so the thread accumulates
// (GL_P - v) (r - b~) instead. Each product is below 2^63 r, a thread's VBN_ITEMS = 8 of them below 2^66 r - far inside lz_reduce's
// 2^12 r^2. The reduction gives value R^-1 = sum z b~ R^-1 = sum z b (b~ = b R: the eq table is in Montgomery form): the PLAIN residue
// of the thread's sum, so the partials and the slots are plain residues, canonical for the host without a conversion.
constexpr int VBN_TPB = 256, VBN_ITEMS = 8, VBN_TILE = VBN_TPB * VBN_ITEMS, VBN_WAVES = VBN_TPB / 64;
typedef VinUnitT<Fr> BnVinUnit;   // member p's partial of wave w of workgroup b: part0 + (p * nblk + b) * VBN_WAVES + w

__device__ __forceinline__ Fr vbn_shfl_xor(const Fr& v, int o) {
    Fr t;
#pragma unroll
    for (int i = 0; i < 4; i++) t.l[i] = __shfl_xor(v.l[i], o);
    return t;
}
// COMPACT: k_bn_vin_dots over the compact signed coefficients of public instances (hg_verify_public_batch_bn254; k_bn_vdot_compact_jobs,
// bn254_verify.inc, is the single-proof form and k_vin_dots<true>, verifier_batch.hip, the Goldilocks one). A unit is one eq table
// (Fr, Montgomery form) and the P members' coefficient blocks evaluated at its point (mode 0: the group's tables of one public input,
// so P is the group size). A workgroup owns VBN_TILE consecutive WORD indices t of the non-padding range only (U.n = blocks *
// 2^log2_n of them): with b = t >> log2_n and r = t & (n-1), eq entry b * 2n + lo + r meets coefficient n-1-r of block b, exactly as
// k_bn_vdot_compact_jobs indexes (ais[i]: one block, lo = 0; ct0is: k blocks, lo = n-1). Both addresses of an item come from one
// (t, r) pair (vin_at). The eq tile is loaded once into registers; per member the thread reads its VBN_ITEMS int64 words (descending
// over the same cache lines as the eq loads ascend) and accumulates |z| times eq, or times r - eq for a negative z; a word beyond U.n
// counts as zero. One lz_reduce / lz_canon per thread and member, one partial per (member, wave): no barrier, and the next member's
// loads are issued ahead of this member's arithmetic, as in the plain form. k_bn_vin_reduce adds the partials: with b~ = b R the
// reduction yields plain residues, so the slots are canonical for the host.
// Bound: |z| <= (q_i-1)/2 < 2^61 (hg_instance_from_ciphertext checks the range), each product is below 2^61 r and a thread's
// VBN_ITEMS = 8 of them below 2^64 r - far inside lz_reduce's 2^12 r^2.
// HBM traffic by design: 8 B per coefficient plus 32 / P B of eq, nothing for padding words - the padding half of an eq table is
// never read. Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 248 VGPRs, no scratch, 2 waves per SIMD (the plain
// form: 230 VGPRs).
template <bool COMPACT>
__global__ __launch_bounds__(VBN_TPB) void k_bn_vin_dots(const BnVinUnit* __restrict__ units, const VinMember* __restrict__ members,
                                                         const VinBlock* __restrict__ blocks, Fr* __restrict__ partials) {
    const VinBlock B = blocks[blockIdx.x];
    const BnVinUnit U = units[B.unit];
    const size_t base = (size_t)B.blk * VBN_TILE + threadIdx.x, nm1 = ((size_t)1 << U.log2_n) - 1;
    Fr eq[VBN_ITEMS];
#pragma unroll
    for (int j = 0; j < VBN_ITEMS; j++) {
        const size_t t = base + (size_t)j * VBN_TPB;
        size_t ie, iw;
        vin_at<COMPACT>(t, nm1, U.lo, ie, iw);
        eq[j] = t < U.n ? U.eq[ie] : fr_zero();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 v[VBN_ITEMS];
    auto load = [&](int p, u64* out) {
        const u64* __restrict__ a = members[U.first + p].a;
#pragma unroll
        for (int j = 0; j < VBN_ITEMS; j++) {
            const size_t t = base + (size_t)j * VBN_TPB;
            size_t ie, iw;
            vin_at<COMPACT>(t, nm1, U.lo, ie, iw);
            out[j] = t < U.n ? a[iw] : 0;
        }
    };
    load(0, v);
    for (int p = 0; p < U.P; p++) {
        u64 nx[VBN_ITEMS];
        if (p + 1 < U.P) load(p + 1, nx);   // (the next member's loads are in flight under this member's arithmetic)
        WCol w = wcol_zero();
#pragma unroll
        for (int j = 0; j < VBN_ITEMS; j++) {
            // the word's sign and magnitude: a laid-out entry v >= 2^63 is -(GL_P - v), a compact word is the int64 itself
            const bool neg = v[j] >= (1ULL << 63);
            u64 mag;
            if constexpr (COMPACT) mag = neg ? (u64)0 - v[j] : v[j];
            else mag = neg ? GL_P - v[j] : v[j];
            wcol_mac_u64(w, mag, vd_negate_if(eq[j], neg));
        }
        Fr s = lz_canon(lz_reduce(w));
        for (int o = 32; o > 0; o >>= 1) s = fr_add(s, vbn_shfl_xor(s, o));
        if (lane == 0) partials[U.part0 + ((size_t)p * U.nblk + B.blk) * VBN_WAVES + wave] = s;   // (one partial per wave: no barrier)
#pragma unroll
        for (int j = 0; j < VBN_ITEMS; j++) v[j] = nx[j];
    }
}
// one wave per member: its unit's nblk * VBN_WAVES partials into its slot (canonical)
__global__ __launch_bounds__(64) void k_bn_vin_reduce(const BnVinUnit* __restrict__ units, const VinMember* __restrict__ members,
                                                      const Fr* __restrict__ partials, Fr* __restrict__ res) {
    const VinMember M = members[blockIdx.x];
    const BnVinUnit U = units[M.unit];
    const size_t np = (size_t)U.nblk * VBN_WAVES;
    const Fr* part = partials + U.part0 + (size_t)(blockIdx.x - U.first) * np;
    Fr s = fr_zero();
    for (size_t b = threadIdx.x; b < np; b += 64) s = fr_add(s, part[b]);
    for (int o = 32; o > 0; o >>= 1) s = fr_add(s, vbn_shfl_xor(s, o));
    if (threadIdx.x == 0) res[M.slot] = s;
}

namespace {

// What a batch checks its proofs against: witness handles (hg_verify_device_batch_bn254: ws) or public instances
// (hg_verify_public_batch_bn254: insts, and open[i] receives the claims an accepted proof i leaves on the secret inputs). `who`
// prefixes the error messages.
struct BnBatchSrc {
    const char* who;
    const std::vector<const Witness*>* ws;
    const std::vector<const Instance*>* insts;
    std::vector<std::vector<OpenClaimBn>>* open;
};

void verify_batch_run_bn254(hg_ctx* ctx, const hg_pk* pk, const BnBatchSrc& src, const std::vector<const uint8_t*>& proofs, const std::vector<size_t>& lens,
                            std::vector<std::string>& why) {
    const size_t n = proofs.size();
    const bool pub = src.insts != nullptr;
    const std::string who(src.who);
    why.assign(n, std::string());
    if (pub) src.open->assign(n, std::vector<OpenClaimBn>());
    if (!n) return;
    const bool times = hg_times("verify");
    const double t0 = omp_get_wtime();
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    Drain drain{ctx->stream, B->up};
    hipc(hipStreamSynchronize(ctx->stream), (who + ": synchronise").c_str());   // (the arena is reset below)
    const Params& p = pk->params;
    // one proof's inputs in HBM, in the order of verify_proof_device_bn254: s, e, k1, ais (k), r1is (k), r2is, then ct0is; from the
    // ciphertext: its instance as it is, a then ct0, k n signed words each
    const BatchInputs L(p);
    const size_t kn = L.K * L.PZ, words = pub ? 2 * kn : L.words, in_bytes = words * sizeof(u64);
    size_t G = (size_t)std::max<int64_t>(0, ctx->verify_batch_group);
    if (!G) G = std::min(std::max<size_t>(1, VB_INPUT_BUDGET / in_bytes), VB_MAX_GROUP);
    const size_t ngroups = (n + G - 1) / G;
    const size_t res_cap_fr = ctx->res_cap * sizeof(E2) / sizeof(Fr);   // (result slots hold Fr here: 32 bytes each)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());   // (the device pass of hipcc ignores the pragmas)
    std::vector<Fr> chm;   // the fixed chain in Montgomery form, as far as the walks have used it
    auto chain_upto = [&](size_t end) {
        if (chm.size() >= end) return;
        const size_t have = chm.size();
        chm.resize(end);
        bn_chain_copy(have, end - have, chm.data() + have);
        for (size_t q = have; q < end; q++) chm[q] = fr_to_mont(chm[q]);
    };

    std::vector<std::vector<Walked<Fr>>> groups(ngroups);
    auto stage = [&](size_t g) {
        if (pub) batch_stage_instances(B, (int)(g & 1), *src.insts, g * G, std::min(n, g * G + G), kn, nthr, src.who);
        else batch_stage_inputs(B, (int)(g & 1), *src.ws, g * G, std::min(n, g * G + G), L, nthr, src.who);
    };
    auto walk = [&](size_t g) {
        walk_group(groups[g], g * G, std::min(n, g * G + G), nthr, who, [&](Walked<Fr>& x) {
            x.rec.reset(new RecBackendT<Fr>(pk, pub, true));
            x.pend = verify_walk_bn254(*x.rec, p, pk->lasso, pk->circuit, proofs[x.idx], lens[x.idx], pub);
        });
    };
    // merge group g's jobs and enqueue them; returns the result slots used
    auto launch = [&](size_t g) -> size_t {
        const int s = (int)(g & 1);
        std::vector<Walked<Fr>>& W = groups[g];
        hipStream_t st = ctx->stream;
        ctx->arena_reset();
        // chain offsets are absolute already: every proof reads the fixed chain
        MergedGroup<Fr> M = merge_group(W, false);
        for (Fr& u : M.us) u = fr_from_mont(u);   // canonical: k_bn_gather_B_jobs reads them as the prover's result slots
        const auto& consts = M.consts;
        const auto& lins = M.lins;
        const auto& muls = M.muls;
        const auto& ffts = M.ffts;
        const auto& dots = M.dots;
        const std::vector<Fr>& us = M.us;
        const int nslot = M.nslot;
        const size_t chain_need = M.chain_need;
        typedef RecBackendT<Fr> Rec;
        struct EqG { int n; dev::ClaimSet cs; Fr* out; };
        std::vector<EqG> eqs;
        for (auto& e : M.eqs) eqs.push_back(EqG{e.n, e.cs, nullptr});
        if ((size_t)nslot > res_cap_fr)
            throw Error(who + ": a group needs " + std::to_string(nslot) + " result slots, the context has " + std::to_string(res_cap_fr) +
                        ": lower verify_batch_group");
        // the chain the jobs read: uploaded with the descriptors, exactly as far as the furthest job of the group reads
        chain_upto(chain_need);
        for (auto& e : eqs) {   // (every job reads below chain_need by construction; checked here against what is uploaded)
            for (int a = 0; a < e.cs.n; a++)
                if (e.cs.point_off[a] + (size_t)e.n > chm.size()) throw Error(who + ": verifier: a job reads past the uploaded chain");
            if (!e.cs.unit_alpha && e.cs.alpha_off + (size_t)e.cs.n > chm.size()) throw Error(who + ": verifier: a job reads past the uploaded chain");
        }
        Fr* res = reinterpret_cast<Fr*>(ctx->d_res);
        // device tables (arena) and host descriptors
        std::vector<VeqPrep> preps;
        std::vector<VeqFill> fills;
        int prep_max_h = 0, fill_max_n = 0;
        for (auto& e : eqs) {
            e.out = ctx->alloc_n<Fr>((size_t)1 << e.n);
            const size_t stride = veq_stride(e.n);
            Fr* ab = ctx->alloc_n<Fr>(stride * (size_t)e.cs.n);
            for (int a = 0; a < e.cs.n; a++) {
                VeqPrep P;
                memset(&P, 0, sizeof(P));
                P.ab = ab + (size_t)a * stride; P.point_off = e.cs.point_off[a]; P.n = e.n; P.unit = e.cs.unit_alpha;
                P.alpha_off = e.cs.alpha_off + a;
                preps.push_back(P);
            }
            fills.push_back(VeqFill{e.out, ab, e.n, e.cs.n});
            prep_max_h = std::max(prep_max_h, e.n > 8 ? e.n - 8 : 0);
            fill_max_n = std::max(fill_max_n, e.n);
        }
        std::vector<BnGatherTJob> gts(lins.size());
        std::vector<const Fr*> lin_T(lins.size()), mul_B(muls.size()), fft_F(ffts.size());
        size_t gt_max = 0, gb_max = 0;
        for (size_t i = 0; i < lins.size(); i++) {
            const HNode& nd = pk->circuit.nodes[lins[i].node];
            const size_t SR = (size_t)1 << (nd.log2_sub_in + nd.log2_reps);
            BnGatherTJob& gj = gts[i];
            memset(&gj, 0, sizeof(gj));
            gj.lin = pk->node_dev[lins[i].node].lin[lins[i].in];   // (no mul part: the verifier's linear term has no input tables)
            gj.eqc = eqs[lins[i].eq].out; gj.log2_S = nd.log2_sub_in; gj.log2_G = nd.log2_sub_out; gj.log2_R = nd.log2_reps;
            Fr* T = ctx->alloc_n<Fr>(SR);
            gj.T = T;
            lin_T[i] = T;
            gt_max = std::max(gt_max, SR);
        }
        std::vector<BnGatherBJob> gbs(muls.size());
        for (size_t i = 0; i < muls.size(); i++) {
            const auto& m = muls[i];
            const HNode& nd = pk->circuit.nodes[m.node];
            const size_t SR = (size_t)1 << (nd.log2_sub_in + nd.log2_reps);
            BnGatherBJob& bj = gbs[i];
            memset(&bj, 0, sizeof(bj));
            Fr* Bt = ctx->alloc_n<Fr>(SR);
            bj.m = pk->node_dev[m.node].mulR[m.in]; bj.eqc = eqs[m.eqc].out; bj.eqx = eqs[m.eqx].out; bj.B = Bt;   // bj.fin: set below
            for (int q = 0; q < dev::PS_MAX_PAIRS; q++) bj.us.slot[q] = q < nd.arity ? (int)(m.u_at + q) : -1;
            bj.arity = nd.arity; bj.log2_S = nd.log2_sub_in; bj.log2_G = nd.log2_sub_out; bj.log2_R = nd.log2_reps;
            mul_B[i] = Bt;
            gb_max = std::max(gb_max, SR);
        }
        // the DFT-row tables (bn254_verify.inc fft_term): w^i tables per (size, direction), direct factors b < s1, parts over [s1, s2) and [s2, L)
        std::map<std::pair<int, int>, Fr*> Wt;
        std::vector<FftPartJob> fft_parts;
        std::vector<FftTabJob> fft_tabs;
        std::vector<FftTabClaim> fft_claims;
        std::vector<size_t> claims_at;   // per fft_tabs entry: its first claim in fft_claims
        size_t part_max = 0, tab_max = 0;
        for (size_t i = 0; i < ffts.size(); i++) {
            const HNode& nd = pk->circuit.nodes[ffts[i].node];
            const dev::ClaimSet& c = ffts[i].cs;
            const int L2 = nd.log2_size;
            const size_t N = (size_t)1 << L2;
            Fr*& Wp = Wt[{L2, (int)nd.inverse}];
            if (!Wp) {
                Wp = ctx->alloc_n<Fr>(N);
                Fr wr = fr_root_of_unity(L2);
                if (nd.inverse) wr = fr_inv(wr);
                k_bn_powers<<<grid_of(N), 256, 0, st>>>(Wp, wr, N);
            }
            const Fr scale = nd.inverse ? fr_inv(fr_small((u64)N)) : fr_one_mont();
            const int s1 = std::min(4, L2), s2 = std::min(8, L2);
            claims_at.push_back(fft_claims.size());
            for (int a = 0; a < c.n; a++) {
                FftPartJob pj;
                memset(&pj, 0, sizeof(pj));
                for (int b = 0; b < L2; b++) pj.pt.r[b] = chm[c.point_off[a] + b];
                pj.W = Wp; pj.L = L2;
                FftTabClaim tc;
                memset(&tc, 0, sizeof(tc));
                for (int b = 0; b < s1; b++) tc.r[b] = pj.pt.r[b];
                tc.coef = c.unit_alpha ? scale : fr_mul(chm[c.alpha_off + a], scale);
                if (s2 > s1) { Fr* T = ctx->alloc_n<Fr>((size_t)1 << (L2 - s1)); tc.T1 = pj.T = T; pj.b_lo = s1; pj.b_hi = s2; fft_parts.push_back(pj); part_max = std::max(part_max, (size_t)1 << (L2 - s1)); }
                if (L2 > s2) { Fr* T = ctx->alloc_n<Fr>((size_t)1 << (L2 - s2)); tc.T2 = pj.T = T; pj.b_lo = s2; pj.b_hi = L2; fft_parts.push_back(pj); part_max = std::max(part_max, (size_t)1 << (L2 - s2)); }
                fft_claims.push_back(tc);
            }
            FftTabJob tj;
            memset(&tj, 0, sizeof(tj));
            Fr* F = ctx->alloc_n<Fr>(N);
            tj.F = F; tj.W = Wp; tj.L = L2; tj.s1 = s1; tj.s2 = s2; tj.nclaims = c.n;   // tj.claims: set below
            fft_tabs.push_back(tj);
            fft_F[i] = F;
            tab_max = std::max(tab_max, N);
        }
        std::vector<VdotJob> vdots(dots.size());
        std::vector<int> blk_job;
        for (size_t i = 0; i < dots.size(); i++) {
            const auto& d = dots[i];
            VdotJob& J = vdots[i];
            memset(&J, 0, sizeof(J));
            J.a = d.kind == Rec::D_LIN ? lin_T[d.tab] : d.kind == Rec::D_MUL ? mul_B[d.tab] : fft_F[d.tab];
            J.b = eqs[d.eq].out; J.n = (size_t)1 << eqs[d.eq].n; J.out = res + d.slot; J.a_is_int = 0;
            J.blk0 = (int)blk_job.size();
            J.nblk = (int)((J.n + VD_TILE - 1) / VD_TILE);
            blk_job.insert(blk_job.end(), (size_t)J.nblk, (int)i);
        }
        const VinPlan<Fr> V = vin_units(M, [&](size_t e) { return eqs[e].out; }, B->d_in[s], words, p, pub, VBN_TILE, VBN_WAVES);
        const auto& units = V.units;
        const auto& members = V.members;
        const auto& blocks = V.blocks;
        // the chain, the phase-1 evaluations and every descriptor: one page-locked staging, one copy ahead of the launches
        size_t desc_bytes = 0;
        auto place = [&](size_t bytes) { const size_t o = desc_bytes; desc_bytes += (bytes + 255) & ~(size_t)255; return o; };
        const size_t o_chain = place(chm.size() * sizeof(Fr)), o_us = place(us.size() * sizeof(Fr)), o_prep = place(preps.size() * sizeof(VeqPrep)),
                     o_fill = place(fills.size() * sizeof(VeqFill)), o_gt = place(gts.size() * sizeof(BnGatherTJob)),
                     o_gb = place(gbs.size() * sizeof(BnGatherBJob)), o_part = place(fft_parts.size() * sizeof(FftPartJob)),
                     o_claim = place(fft_claims.size() * sizeof(FftTabClaim)), o_tab = place(fft_tabs.size() * sizeof(FftTabJob)),
                     o_dot = place(vdots.size() * sizeof(VdotJob)), o_bj = place(blk_job.size() * sizeof(int)),
                     o_unit = place(units.size() * sizeof(BnVinUnit)), o_mem = place(members.size() * sizeof(VinMember)),
                     o_blk = place(blocks.size() * sizeof(VinBlock));
        char* d_desc = static_cast<char*>(ctx->alloc(std::max<size_t>(desc_bytes, 1)));
        char* h = batch_desc_host(B, std::max<size_t>(desc_bytes, 1));
        const Fr* d_chal = reinterpret_cast<const Fr*>(d_desc + o_chain);
        for (auto& j : gbs) j.fin = reinterpret_cast<const Fr*>(d_desc + o_us);
        for (size_t q = 0; q < fft_tabs.size(); q++) fft_tabs[q].claims = reinterpret_cast<const FftTabClaim*>(d_desc + o_claim) + claims_at[q];
        auto put = [&](size_t o, const auto& v) { if (!v.empty()) memcpy(h + o, v.data(), v.size() * sizeof(v[0])); };
        put(o_chain, chm); put(o_us, us); put(o_prep, preps); put(o_fill, fills); put(o_gt, gts); put(o_gb, gbs); put(o_part, fft_parts);
        put(o_claim, fft_claims); put(o_tab, fft_tabs); put(o_dot, vdots); put(o_bj, blk_job); put(o_unit, units); put(o_mem, members);
        put(o_blk, blocks);
        if (desc_bytes) hipc(hipMemcpyAsync(d_desc, h, desc_bytes, hipMemcpyHostToDevice, st), (who + ": upload descriptors").c_str());
        // one launch per kind (launchers that index their jobs by gridDim.y: launches of at most VD_MAX_Y jobs)
        auto chunks = [](size_t njobs, auto fn) { for (size_t q0 = 0; q0 < njobs; q0 += VD_MAX_Y) fn(q0, (unsigned)std::min(VD_MAX_Y, njobs - q0)); };
        const auto* d_prep = reinterpret_cast<const VeqPrep*>(d_desc + o_prep);
        const auto* d_fill = reinterpret_cast<const VeqFill*>(d_desc + o_fill);
        chunks(preps.size(), [&](size_t q0, unsigned nq) {
            k_bn_veq_prep<<<dim3(1 + (unsigned)(((size_t)1 << prep_max_h) + 255) / 256, nq), 256, 0, st>>>(d_prep + q0, d_chal);
        });
        chunks(fills.size(), [&](size_t q0, unsigned nq) {
            k_bn_veq_fill<<<dim3((unsigned)std::min<size_t>((((size_t)1 << fill_max_n) + 255) / 256, 1024), nq), 256, 0, st>>>(d_fill + q0);
        });
        if (!consts.empty()) {
            Fr* d_cpart = ctx->alloc_n<Fr>(1024);   // one after the other on the stream: one partials buffer serves them all
            for (const auto& c : consts) {
                const HNode& nd = pk->circuit.nodes[c.node];
                const hg_pk::NodeDev& dv = pk->node_dev[c.node];
                const size_t total = dv.nconst << nd.log2_reps;
                const int grid = (int)std::max<size_t>(1, std::min<size_t>((total + BN_TPB - 1) / BN_TPB, 1024));
                k_bn_const_sum<<<grid, BN_TPB, 0, st>>>(dv.const_gate, dv.const_coef, dv.nconst, eqs[c.eq].out, nd.log2_sub_out, nd.log2_reps, d_cpart);
                k_bn_reduce<<<1, BN_TPB, 0, st>>>(d_cpart, grid, 1, res + c.slot);
            }
        }
        const auto* d_gt = reinterpret_cast<const BnGatherTJob*>(d_desc + o_gt);
        chunks(gts.size(), [&](size_t q0, unsigned nq) {
            k_bn_gather_T_jobs<<<dim3((unsigned)std::min<size_t>((gt_max + BN_TPB - 1) / BN_TPB, 2048), nq), BN_TPB, 0, st>>>(d_gt + q0);
        });
        const auto* d_part = reinterpret_cast<const FftPartJob*>(d_desc + o_part);
        const auto* d_tab = reinterpret_cast<const FftTabJob*>(d_desc + o_tab);
        chunks(fft_parts.size(), [&](size_t q0, unsigned nq) {
            k_bn_fft_part_jobs<<<dim3((unsigned)std::min<size_t>((part_max + 255) / 256, 2048), nq), 256, 0, st>>>(d_part + q0);
        });
        chunks(fft_tabs.size(), [&](size_t q0, unsigned nq) {
            k_bn_fft_tab_jobs<<<dim3((unsigned)std::min<size_t>((tab_max + 255) / 256, 2048), nq), 256, 0, st>>>(d_tab + q0);
        });
        const auto* d_gb = reinterpret_cast<const BnGatherBJob*>(d_desc + o_gb);
        chunks(gbs.size(), [&](size_t q0, unsigned nq) {
            k_bn_gather_B_jobs<<<dim3((unsigned)std::min<size_t>((gb_max + BN_TPB - 1) / BN_TPB, 2048), nq), BN_TPB, 0, st>>>(d_gb + q0);
        });
        if (!vdots.empty()) {   // (a flat grid: blockIdx.x, not y, indexes the tiles)
            Fr* part = ctx->alloc_n<Fr>(blk_job.size());
            const auto* d_dots = reinterpret_cast<const VdotJob*>(d_desc + o_dot);
            k_bn_vdot_jobs<<<(unsigned)blk_job.size(), 256, 0, st>>>(d_dots, reinterpret_cast<const int*>(d_desc + o_bj), part);
            k_bn_vdot_reduce<<<(unsigned)vdots.size(), 256, 0, st>>>(d_dots, part);
        }
        if (!units.empty()) {
            hipc(hipStreamWaitEvent(st, B->ev[s], 0), (who + ": wait for the inputs").c_str());
            Fr* part = ctx->alloc_n<Fr>(V.parts);
            const auto* d_units = reinterpret_cast<const BnVinUnit*>(d_desc + o_unit);
            const auto* d_mem = reinterpret_cast<const VinMember*>(d_desc + o_mem);
            const auto* d_blk = reinterpret_cast<const VinBlock*>(d_desc + o_blk);
            if (pub) k_bn_vin_dots<true><<<(unsigned)blocks.size(), VBN_TPB, 0, st>>>(d_units, d_mem, d_blk, part);
            else k_bn_vin_dots<false><<<(unsigned)blocks.size(), VBN_TPB, 0, st>>>(d_units, d_mem, d_blk, part);
            k_bn_vin_reduce<<<(unsigned)members.size(), 64, 0, st>>>(d_units, d_mem, part, res);
        }
        if (ctx->d_res != ctx->h_res && nslot)
            hipc(hipMemcpyAsync(ctx->h_res, ctx->d_res, (size_t)nslot * sizeof(Fr), hipMemcpyDeviceToHost, st), (who + ": copy results").c_str());
        if (times)
            fprintf(stderr, "[hg] verify_batch_bn254: group %zu (%zu proofs): %zu eq tables, %zu constant sums, %zu + %zu gathers, %zu DFT rows, %zu dots, %zu input evaluations in %zu units (%.1f MB); %d slots\n",
                    g, W.size(), eqs.size(), consts.size(), lins.size(), muls.size(), ffts.size(), dots.size(), members.size(), units.size(), V.bytes / 1e6, nslot);
        return (size_t)nslot;
    };
    auto complete = [&](size_t g) {
        const Fr* h_res = reinterpret_cast<const Fr*>(ctx->h_res);
        complete_group(groups[g], nthr, [&](int slot) { return fr_to_mont(h_res[slot]); }, [&](Walked<Fr>& x) {
            why[x.idx] = verify_complete_bn254(x.pend);
            if (pub && why[x.idx].empty())
                for (const auto& cl : x.pend.open) (*src.open)[x.idx].push_back(open_claim_bn254(cl));
        });
    };
    batch_groups(ctx->stream, who, "verify_batch_bn254", times, t0, n, ngroups, G, stage, walk, launch, complete);
}

}  // namespace

void verify_batch_device_bn254(hg_ctx* ctx, const hg_pk* pk, const std::vector<const Witness*>& ws, const std::vector<const uint8_t*>& proofs,
                               const std::vector<size_t>& lens, std::vector<std::string>& why) {
    verify_batch_run_bn254(ctx, pk, BnBatchSrc{"hg_verify_device_batch_bn254", &ws, nullptr, nullptr}, proofs, lens, why);
}

void verify_public_batch_device_bn254(hg_ctx* ctx, const hg_pk* pk, const std::vector<const Instance*>& insts, const std::vector<const uint8_t*>& proofs,
                                      const std::vector<size_t>& lens, std::vector<std::string>& why, std::vector<std::vector<OpenClaimBn>>& open) {
    verify_batch_run_bn254(ctx, pk, BnBatchSrc{"hg_verify_public_batch_bn254", nullptr, &insts, &open}, proofs, lens, why);
}

// one eq table over the caller's point, then k_bn_vin_dots<true> as ONE unit whose members are the instances' tables
void instance_mle_batch_device_bn254(hg_ctx* ctx, const Params& p, const std::vector<const Instance*>& insts, int which, int index, const u64* point4,
                                     size_t nvars, u64* out4) {
    const size_t np = insts.size();
    if (!np) return;
    const char* who = "hg_instance_mle_batch_bn254";
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    Drain drain{ctx->stream, B->up};
    hipc(hipStreamSynchronize(ctx->stream), "hg_instance_mle_batch_bn254: synchronise");   // (the arena is reset below)
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t n = p.PZ(), kn = (size_t)p.k * n;
    batch_stage_instances(B, 0, insts, 0, np, kn, std::max(1, hg_omp_threads()), who);
    std::vector<Fr> chm(nvars);   // (the point is the whole chain, in Montgomery form)
    for (size_t j = 0; j < nvars; j++) chm[j] = fr_from_limbs_mont(point4 + 4 * j);
    const int nv = (int)nvars;
    Fr* eq = ctx->alloc_n<Fr>((size_t)1 << nv);
    Fr* ab = ctx->alloc_n<Fr>(veq_stride(nv));
    VeqPrep P;
    memset(&P, 0, sizeof(P));
    P.ab = ab; P.n = nv; P.unit = 1;
    const VeqFill F{eq, ab, nv, 1};
    std::vector<std::pair<const u64*, int>> tabs(np);
    for (size_t i = 0; i < np; i++) tabs[i] = {B->d_in[0] + i * 2 * kn + (which ? kn : (size_t)index * n), (int)i};
    VinPlan<Fr> V;
    V.add(eq, which ? kn : n, (u32)p.n_log2, which ? (u32)(n - 1) : 0, tabs, VBN_TILE, VBN_WAVES);
    const BnVinUnit& U = V.units[0];
    const auto& members = V.members;
    const auto& blocks = V.blocks;
    size_t desc_bytes = 0;
    auto place = [&](size_t bytes) { const size_t o = desc_bytes; desc_bytes += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_chain = place(std::max<size_t>(nvars, 1) * sizeof(Fr)), o_prep = place(sizeof(P)), o_fill = place(sizeof(F)), o_unit = place(sizeof(U)),
                 o_mem = place(np * sizeof(VinMember)), o_blk = place(blocks.size() * sizeof(VinBlock));
    char* d_desc = static_cast<char*>(ctx->alloc(desc_bytes));
    char* h = batch_desc_host(B, desc_bytes);
    if (nvars) memcpy(h + o_chain, chm.data(), nvars * sizeof(Fr));
    memcpy(h + o_prep, &P, sizeof(P));
    memcpy(h + o_fill, &F, sizeof(F));
    memcpy(h + o_unit, &U, sizeof(U));
    memcpy(h + o_mem, members.data(), np * sizeof(VinMember));
    memcpy(h + o_blk, blocks.data(), blocks.size() * sizeof(VinBlock));
    hipc(hipMemcpyAsync(d_desc, h, desc_bytes, hipMemcpyHostToDevice, st), "hg_instance_mle_batch_bn254: upload descriptors");
    const size_t high = (size_t)1 << (nv > 8 ? nv - 8 : 0);
    k_bn_veq_prep<<<dim3(1 + (unsigned)((high + 255) / 256), 1), 256, 0, st>>>(reinterpret_cast<const VeqPrep*>(d_desc + o_prep),
                                                                              reinterpret_cast<const Fr*>(d_desc + o_chain));
    k_bn_veq_fill<<<dim3((unsigned)std::min<size_t>((((size_t)1 << nv) + 255) / 256, 1024), 1), 256, 0, st>>>(reinterpret_cast<const VeqFill*>(d_desc + o_fill));
    hipc(hipStreamWaitEvent(st, B->ev[0], 0), "hg_instance_mle_batch_bn254: wait for the instances");
    Fr* res = ctx->alloc_n<Fr>(np);
    Fr* part = ctx->alloc_n<Fr>(V.parts);
    const auto* d_units = reinterpret_cast<const BnVinUnit*>(d_desc + o_unit);
    const auto* d_mem = reinterpret_cast<const VinMember*>(d_desc + o_mem);
    k_bn_vin_dots<true><<<(unsigned)blocks.size(), VBN_TPB, 0, st>>>(d_units, d_mem, reinterpret_cast<const VinBlock*>(d_desc + o_blk), part);
    k_bn_vin_reduce<<<(unsigned)np, 64, 0, st>>>(d_units, d_mem, part, res);
    static_assert(sizeof(Fr) == 4 * sizeof(u64), "an Fr result slot is 4 limbs");
    hipc(hipMemcpyAsync(out4, res, np * sizeof(Fr), hipMemcpyDeviceToHost, st), "hg_instance_mle_batch_bn254: copy results");
    hipc(hipStreamSynchronize(st), "hg_instance_mle_batch_bn254: synchronise");
    hipc(hipGetLastError(), "hg_instance_mle_batch_bn254: kernels");
}
