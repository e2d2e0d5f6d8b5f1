// Part of struct Prover (prover.hip includes this file inside the class body): the Lasso node (LassoNode::prove_claim_reduction, lasso.rs:57-114): limb split, counters, collation sum-check, the two memory-checking grand products (slot form, mirrored top layer, recomputed hashes), openings.

    // ---- Lasso node (lasso.rs:57-114) ------------------------------------------------------------
    struct GpOut { size_t point_off; std::shared_ptr<std::vector<E2>> claims; };  // claims: final per-table claims, valid after replay
    // prove_grand_product (prover.rs:183-266) over nb contiguous tables of `len` base-field values
    // `owner[n]` = rank that runs layer n (n = 0: roots + top evaluations); H may be null when no layer is owned
    int gp_deepest(int nv, const std::vector<int>& owner) const {  // highest tree level this rank needs (layer n reads level nv-1-n)
        int deepest = 0;
        for (int n = 0; n < nv; n++) if (mine(owner[n])) deepest = std::max(deepest, nv - 1 - n);
        return deepest;
    }
    // Joint classes of the read rows of the Lasso top layer (GpHashSrc::slot_of), built with the hash sources in lasso_node
    // (layer 0 = the top layer, rows = the read rows held; layer d >= 1: rows = the read and write rows held, groups of 2^(d+1) segments)
    struct SlotLayer {
        int V = 0, ng = 0, nrows = 0;
        std::vector<uint8_t> slot_of, rep;   // [row * ng + group], [slot * ng + group] (255: no such class there)
        uint8_t* d_slot_of = nullptr; uint8_t* d_rep = nullptr; E2* d_slotw = nullptr; E2* d_ratio = nullptr;
        u64* d_emit = nullptr;               // layer 0: V * ng read masks then V * ng write masks
    };
    struct GpSlots { int V = 0, NP = 0, G = 0 /* read rows held */, seg_shift = 0; std::vector<SlotLayer> layer; } gp_slots;
    // class weights W[v][g] = sum of the members' gamma^b (and W r_0 for the first round's weighted fold), and per row gamma^b / W of
    // its class: what turns a class's folded left table back into the row's (gp_slot_regroup)
    void slot_weights(const SlotLayer& sl, const dev::Powers& pw, E2 r0) {
        const int V = sl.V, ng = sl.ng, R = sl.nrows;
        std::vector<E2> W((size_t)V * ng, e2_zero());
        for (int b = 0; b < R; b++)
            for (int g = 0; g < ng; g++) { E2& w = W[(size_t)sl.slot_of[(size_t)b * ng + g] * ng + g]; w = e2_add(w, pw.v[b]); }
        // one inversion for all of them (a group with fewer classes than V keeps weight zero on the rest)
        std::vector<E2> pre(W.size()), inv(W.size(), e2_zero());
        E2 run_p = e2_one();
        for (size_t q = 0; q < W.size(); q++) { pre[q] = run_p; if (W[q].c0 | W[q].c1) run_p = e2_mul(run_p, W[q]); }
        E2 run_i = e2_inv(run_p);
        for (size_t q = W.size(); q-- > 0;) if (W[q].c0 | W[q].c1) { inv[q] = e2_mul(run_i, pre[q]); run_i = e2_mul(run_i, W[q]); }
        std::vector<E2> slotw(2 * W.size()), ratio((size_t)R * ng);
        for (size_t q = 0; q < W.size(); q++) { slotw[2 * q] = W[q]; slotw[2 * q + 1] = e2_mul(W[q], r0); }
        for (int b = 0; b < R; b++)
            for (int g = 0; g < ng; g++) {
                const size_t q = (size_t)sl.slot_of[(size_t)b * ng + g] * ng + g;
                if (!(W[q].c0 | W[q].c1)) throw Error("grand product: degenerate batching challenge");
                ratio[(size_t)b * ng + g] = e2_mul(pw.v[b], inv[q]);
            }
        upload(sl.d_slotw, slotw.data(), slotw.size() * sizeof(E2), "upload slot weights");
        upload(sl.d_ratio, ratio.data(), ratio.size() * sizeof(E2), "upload slot ratios");
    }
    // lev1 (optional): the first tree level, already produced by the hash kernel.
    // `local` (multi-GPU split by batch item): H holds only the rows of the global pairs listed in `local` (ascending);
    // with p0_only the first of them is pair 0, held only to supply p_0.
    // `hash_src` (device pointer): level 0 is not materialised, the top layer's first round recomputes it (k_gp_first_hash).
    // `emit` > 0: tree levels 1 .. emit are written by the first rounds of the top `emit` layers (their products ARE the next
    // level), which therefore run one after the other before everything else; the remaining small levels follow them.
    GpOut grand_product(const u64* H, size_t len, int nb, const std::vector<int>& owner, const u64* lev1 = nullptr,
                        const std::vector<int>* local = nullptr, bool p0_only = false, const dev::GpHashSrc* hash_src = nullptr, int emit = 0,
                        double hash_fused_bytes = 0, const u64* mirror_c = nullptr) {
        int nv = 0;
        while (((size_t)1 << nv) < len) nv++;
        const int nl = local ? (int)local->size() : nb;  // rows actually held
        std::vector<const u64*> lev(nv, nullptr);
        lev[0] = H;
        const int deepest = gp_deepest(nv, owner);
        if (emit > 0) {
            for (int n = 0; n < nv; n++) if (!mine(owner[n])) throw Error("grand product: level-emitting first rounds need every layer on this rank");
            if (emit > nv - 1 || lev1) throw Error("grand product: bad emit depth");
        } else if (hash_src) throw Error("grand product: recomputed level 0 needs emit >= 1");
        if (lev1 && nv > 1) lev[1] = lev1;
        // buffers of every level this rank needs (host-side bump allocation), then the launches that fill levels > emit
        std::vector<u64*> lev_w(nv, nullptr);
        for (int k = (lev1 && nv > 1) ? 2 : 1; k <= deepest; k++) { lev_w[k] = nl > 0 ? ctx->alloc_n<u64>((size_t)nl * (len >> k)) : nullptr; lev[k] = lev_w[k]; }
        size_t roots = slot(nb), ev0 = slot(2 * (size_t)nb);
        E2* lr = nullptr;
        E2* le = nullptr;
        const bool top_mine = mine(owner[0]) && nl > 0;
        if (top_mine && local) { lr = ctx->alloc_n<E2>(nl); le = ctx->alloc_n<E2>(2 * (size_t)nl); }
        const int first_k = std::max((lev1 && nv > 1) ? 2 : 1, emit + 1);
        auto build = [this, lev, lev_w, len, nl, nb, nv, deepest, first_k, roots, ev0, lr, le, top_mine, local]() {
            for (int k = first_k; k <= deepest; k++) {  // Layer::bottom / Layer::up: w = v_l * v_r on the MSB split
                const size_t in_len = len >> (k - 1);
                if (in_len <= (size_t)dev::PROD_TAIL_LEN && in_len >= 2) {  // the remaining (small) levels in one launch
                    dev::ProdTailOut outs;
                    memset(&outs, 0, sizeof(outs));
                    int nlev = 0;
                    double bytes = 0;
                    for (int kk = k; kk <= deepest; kk++) { outs.p[nlev++] = lev_w[kk]; bytes += (double)nl * (len >> (kk - 1)) * 8.0 * 1.5; }
                    ctx->prof_begin(cls_tree, bytes);
                    if (nl > 0) dev::prod_tail(st, lev[k - 1], (int)in_len, outs, nlev, nl);
                    ctx->prof_end();
                    break;
                }
                // three levels per launch while the third one is still above the tail's size
                if (k + 2 <= deepest && (in_len >> 2) > (size_t)dev::PROD_TAIL_LEN && in_len <= ((size_t)1 << 18)) {
                    ctx->prof_begin(cls_tree, (double)nl * in_len * 8.0 * 1.5 * 1.75);
                    if (nl > 0) dev::prod_level3(st, lev[k - 1], in_len, lev_w[k], lev_w[k + 1], lev_w[k + 2], nl);
                    ctx->prof_end();
                    k += 2;
                    continue;
                }
                ctx->prof_begin(cls_tree, (double)nl * in_len * 8.0 * 1.5);
                if (nl > 0) dev::prod_level(st, lev[k - 1], in_len, lev_w[k], nl);
                ctx->prof_end();
            }
            if (top_mine) {
                if (!local) dev::gp_top(st, lev[nv - 1], nb, d_res() + roots, d_res() + ev0);
                else dev::gp_top(st, lev[nv - 1], nl, lr, le);
            }
        };
        if (emit > 0) st_after_seq.push_back(build);
        else build();
        if (top_mine && local)
            for (int li = p0_only ? 1 : 0; li < nl; li++) {
                int b = (*local)[li];
                scatter.push_back({lr + li, roots + (size_t)b});
                scatter.push_back({le + 2 * li, ev0 + 2 * (size_t)b});
                scatter.push_back({le + 2 * li + 1, ev0 + 2 * (size_t)b + 1});
            }
        auto claims = std::make_shared<std::vector<E2>>(nb);
        mark("grand product: " + std::to_string(nb) + " root products (prover.rs:197-221)");
        push_op([this, roots, nb, claims] {  // root products (prover.rs:197-221)
            for (int b = 0; b < nb; b++) { (*claims)[b] = h_res()[roots + b]; proof.write_e((*claims)[b]); }
        });
        auto layer_down = [this, claims, nb](size_t evals_slot, E2 mu) {  // prover.rs:288-294
            push_op([this, claims, nb, evals_slot, mu] {
                const E2* ev = h_res() + evals_slot;
                for (int b = 0; b < nb; b++) (*claims)[b] = e2_add(ev[2 * b], e2_mul(mu, e2_sub(ev[2 * b + 1], ev[2 * b])));
            });
        };
        GpOut out{0, claims};
        // layer with num_vars 0
        mark("grand product layer 0: v_l, v_r evaluations per tree (prover.rs:257; no sum-check)");
        defer_write_slots(ev0, 2 * (size_t)nb);
        out.point_off = epos();
        layer_down(ev0, squeeze());
        // Claim epilogue on the device (GpClaimEp, kernels.hpp): the tail workgroup that writes a layer's final evaluations also
        // unscales them, completes a mirrored job's write rows, folds them by mu and sums the next layer's claim - the replay then
        // only reads result slots. One rank holding the whole batch only: a sharded rank's evaluations are partial. Layer 0 has no
        // sum-check and stays here; the per-pair claims are written by the LAST layer alone (GpOut::claims), no step reads the others'.
        const bool dev_claims = ctx->gp_claims_device && world == 1 && !local;
        int prev_ep = -1;        // gp_eps entry of the layer above, which still lacks this layer's gamma^b
        int ndev = 0, ndev_mirrored = 0, ndev_slot = 0;
        for (int n = 1; n < nv; n++) {
            int k = nv - 1 - n;
            size_t h = (size_t)1 << n;
            E2 gamma = squeeze();  // prover.rs:238
            dev::Powers pw;
            memset(&pw, 0, sizeof(pw));
            if (nb > dev::PW_MAX) throw Error("grand product: too many batched tables");
            E2 g = e2_one();
            for (int b = 0; b < nb; b++) { pw.v[b] = g; g = e2_mul(g, gamma); }
            Cell claim = cell();
            if (prev_ep >= 0) {   // sum_check_claim, formed by the epilogue of the layer above
                GpEpReq& pe = gp_eps[prev_ep];
                pe.gnext.assign(pw.v, pw.v + nb);
                pe.ep.has_next = 1;
                const size_t ns = pe.ep.next_slot = slot(1);
                push_op([this, ns, claim] { *claim = h_res()[ns]; });
            } else
            push_op([claims, nb, pw, claim] {  // sum_check_claim (prover.rs:281-286)
                E2 c = e2_zero();
                for (int b = 0; b < nb; b++) c = e2_add(c, e2_mul((*claims)[b], pw.v[b]));
                *claim = c;
            });
            size_t evals = slot(2 * (size_t)nb);
            ScHandle sc;
            const size_t jobs_before = st_queue.size();
            StrideArgs sa;   // what every form of the layer's sum-check sets; the forms below add their own
            sa.seq = n >= nv - emit ? nv - n : 0;                           // first round launched alone, deepest layer first
            sa.next_level = sa.seq ? lev_w[k + 1] : nullptr;                  // ... and writes tree level k + 1
            const dev::GpHashSrc* hs = (hash_src && k == 0) ? hash_src : nullptr;
            sa.hash_src = hs;
            if (hs) { sa.fused_bytes = hash_fused_bytes; sa.fused_model_extra = hash_model_extra; sa.hash_reads = hash_design_reads; }
            if (sa.next_level) {   // rows of level k + 1 this first round writes: the next layer's slot rows in slot form, one per row held otherwise
                const bool next_slots = hash_src && !local && k + 1 < (int)gp_slots.layer.size();
                sa.level_design = (double)(next_slots ? gp_slots.layer[k + 1].V : nl) * (double)(len >> (k + 1)) * 8.0;
            }
            const bool mirrored = hs && mirror_c;
            if (mirrored) {
                // Top layer with row b + nb/2 = row b + c for every b < nb/2 (the Lasso write hashes, c = gamma^2): only the read rows
                // are stored and multiplied (StJob::mirror in kernels.hpp). The kernels sum everything but the factor 1 + kappa.
                const int G2 = nb / 2;
                std::vector<int> rows;   // global ids of the read rows held, ascending (row 0 first)
                for (int li = 0; li < nl; li++) { const int b = local ? (*local)[li] : li; if (b < G2) rows.push_back(b); }
                const int R = (int)rows.size();
                for (int li = 0; li < R; li++) if ((local ? (*local)[li] : li) != rows[li]) throw Error("grand product: read rows must come first");
                int nwr = 0;
                for (int li = R; li < nl; li++) {
                    const int b = (local ? (*local)[li] : li) - G2;
                    if (std::find(rows.begin(), rows.end(), b) == rows.end() || (p0_only && b == 0)) throw Error("grand product: write row without its read row");
                    nwr++;
                }
                if (nwr != R - (p0_only ? 1 : 0)) throw Error("grand product: mirrored rows do not pair up");
                if (R > 63 || 2 * R + 1 > dev::PW_MAX) throw Error("grand product: too many mirrored rows");
                const E2 kappa = pw.v[G2], onek = e2_add(e2_one(), kappa);
                if (onek.c0 == 0 && onek.c1 == 0) throw Error("grand product: degenerate batching challenge");
                const E2 kp = e2_mul(kappa, e2_inv(onek));
                dev::Powers pwl;
                memset(&pwl, 0, sizeof(pwl));
                E2 lam = e2_zero();
                for (int li = 0; li < R; li++) { pwl.v[li] = pw.v[rows[li]]; if (!(p0_only && li == 0)) lam = e2_add(lam, pwl.v[li]); }
                const u64 c = *mirror_c;
                MirrorSpec ms;
                ms.k1 = e2_mul_f(kp, c);
                ms.k2 = e2_mul(e2_mul_f(kp, gl_mul(c, c)), lam);
                ms.credit_ntab = 2 * nl;
                E2* fin = ctx->alloc_n<E2>(2 * (size_t)R + 1);
                const bool run = mine(owner[n]) && R > (p0_only ? 1 : 0);
                const bool slotted = !gp_slots.layer.empty();   // (decided with the hash sources, lasso_node)
                if (slotted && (!run || R != gp_slots.G)) throw Error("grand product: the slot plan does not fit the rows held");
                SlotPlan spl;
                if (slotted) {
                    const SlotLayer& sl = gp_slots.layer[0];
                    spl.tail_ntab = 2 * R + 1; spl.d_slot_of = sl.d_slot_of; spl.d_ratio = sl.d_ratio;
                    spl.nrows = R; spl.nslots = sl.V; spl.npairs = sl.ng; spl.max_rd = gp_slots.seg_shift;
                }
                sa.enqueue = run; sa.p0_only = p0_only; sa.mirror = &ms; sa.slots = slotted ? &spl : nullptr;
                sc = sc_stride(dev::SC_GRANDPROD, lev[k], true, h, slotted ? 2 * gp_slots.layer[0].V + 1 : 2 * R + 1, n, pwl, fin, sa);
                sc.scaled = true; sc.scale = onek;
                if (slotted) slot_weights(gp_slots.layer[0], pwl, sc.rs[0]);
                if (run && !dev_claims)   // (the claim epilogue writes the result slots itself)
                    for (int li = p0_only ? 1 : 0; li < R; li++) {
                        scatter.push_back({fin + 2 * li, evals + 2 * (size_t)rows[li]});
                        scatter.push_back({fin + 2 * li + 1, evals + 2 * (size_t)rows[li] + 1});
                    }
            } else if (!local && hash_src && k >= 1 && k < (int)gp_slots.layer.size()) {
                // slot form below the top layer: the input rows are this layer's slot rows (written by the layer above), the tail runs
                // on the 2 nb per-row tables again
                const SlotLayer& sl = gp_slots.layer[k];
                if (sl.nrows != nb || !mine(owner[n]) || !sa.seq) throw Error("grand product: slot form on a partial batch");
                SlotPlan spl;
                spl.tail_ntab = 2 * nb; spl.d_slot_of = sl.d_slot_of; spl.d_ratio = sl.d_ratio;
                spl.nrows = nb; spl.nslots = sl.V; spl.npairs = sl.ng; spl.max_rd = gp_slots.seg_shift;
                spl.job_slotw = sl.d_slotw; spl.job_emit = sl.d_emit;
                sa.model_ntab = 2 * nb; sa.slots = &spl;
                sc = sc_stride(dev::SC_GRANDPROD, lev[k], true, h, 2 * sl.V, n, pw, d_res() + evals, sa);
                slot_weights(sl, pw, sc.rs[0]);
            } else if (!local) {
                sa.enqueue = mine(owner[n]);
                sc = sc_stride(dev::SC_GRANDPROD, lev[k], true, h, 2 * nb, n, pw, d_res() + evals, sa);
            } else {
                // this rank's share of the batch: local pair li is global pair b = local[li], weight gamma^b
                dev::Powers pwl;
                memset(&pwl, 0, sizeof(pwl));
                for (int li = 0; li < nl; li++) pwl.v[li] = pw.v[(*local)[li]];
                E2* fin = nl ? ctx->alloc_n<E2>(2 * (size_t)nl) : nullptr;
                if (hash_src && k >= 1 && k < (int)gp_slots.layer.size()) {   // slot form below the top layer, on the rows this rank holds
                    const SlotLayer& sl = gp_slots.layer[k];
                    if (sl.nrows != nl || !mine(owner[n]) || !sa.seq || nl <= (p0_only ? 1 : 0)) throw Error("grand product: the slot plan does not fit the rows held");
                    SlotPlan spl;
                    spl.tail_ntab = 2 * nl; spl.d_slot_of = sl.d_slot_of; spl.d_ratio = sl.d_ratio;
                    spl.nrows = nl; spl.nslots = sl.V; spl.npairs = sl.ng; spl.max_rd = gp_slots.seg_shift;
                    spl.job_slotw = sl.d_slotw; spl.job_emit = sl.d_emit;
                    sa.p0_only = p0_only; sa.model_ntab = 2 * nl; sa.slots = &spl;
                    sc = sc_stride(dev::SC_GRANDPROD, lev[k], true, h, 2 * sl.V, n, pwl, fin, sa);
                    slot_weights(sl, pwl, sc.rs[0]);
                } else {
                    sa.enqueue = mine(owner[n]) && nl > (p0_only ? 1 : 0); sa.p0_only = p0_only;
                    sc = sc_stride(dev::SC_GRANDPROD, lev[k], true, h, 2 * nl, n, pwl, fin, sa);
                }
                if (mine(owner[n]))
                    for (int li = p0_only ? 1 : 0; li < nl; li++) {
                        int b = (*local)[li];
                        scatter.push_back({fin + 2 * li, evals + 2 * (size_t)b});
                        scatter.push_back({fin + 2 * li + 1, evals + 2 * (size_t)b + 1});
                    }
            }
            mark("grand product layer " + std::to_string(n) + ": sum-check, " + std::to_string(n) + " rounds x 4 coefficients [C1 message format, C2 power order, C3 variable order]");
            defer_sumcheck(sc, 3, claim, nullptr);
            const bool dev_layer = dev_claims && st_queue.size() == jobs_before + 1;   // (queued here: it ends in the tail launch of flush_stride)
            if (!dev_layer) defer_gp_unscale(evals, nb, pw);
            if (mirrored && !dev_layer) {   // the write rows' evaluations: folding is affine with coefficients summing to one, so row + c stays row + c
                const u64 c = *mirror_c;
                const int G2 = nb / 2;
                push_op([this, evals, G2, c] {
                    for (int b = 0; b < G2; b++)
                        for (int t = 0; t < 2; t++) ctx->h_res[evals + 2 * (size_t)(G2 + b) + t] = e2_add_f(ctx->h_res[evals + 2 * (size_t)b + t], c);
                });
            }
            mark("grand product layer " + std::to_string(n) + ": v_l, v_r evaluations per tree (prover.rs:257)");
            defer_write_slots(evals, 2 * (size_t)nb);  // prover.rs:257
            out.point_off = sc.point_off;
            const E2 mu = squeeze();                   // prover.rs:259
            prev_ep = -1;
            if (dev_layer) {
                GpEpReq e;
                memset(&e.ep, 0, sizeof(e.ep));
                e.job = (int)jobs_before;
                e.ep.mu = mu; e.ep.nb = nb; e.ep.evals_slot = evals;
                if (mirrored) { e.ep.nread = nb / 2; e.ep.c = *mirror_c; }
                // gamma^-b: challenge-only, computed during the walk like the host form's (defer_gp_unscale)
                const int nw = mirrored ? nb / 2 : nb;
                e.winv.assign(nw, e2_one());
                if (nw > 1) {
                    if (pw.v[1].c0 == 0 && pw.v[1].c1 == 0) throw Error("grand product: zero batching weight");
                    const E2 ginv = e2_inv(pw.v[1]);
                    E2 w = ginv;
                    for (int b = 1; b < nw; b++) { e.winv[b] = w; w = e2_mul(w, ginv); }
                }
                if (n == nv - 1) {   // the final claims, read by the caller after the replay
                    const size_t cs = e.ep.claims_slot = slot(nb);
                    e.ep.has_claims = 1;
                    push_op([this, claims, nb, cs] { for (int b = 0; b < nb; b++) (*claims)[b] = h_res()[cs + b]; });
                }
                prev_ep = (int)gp_eps.size();
                gp_eps.push_back(std::move(e));
                ndev++;
                if (mirrored) ndev_mirrored++;
                else if (st_queue.back().slot.tail_ntab) ndev_slot++;
            } else layer_down(evals, mu);
        }
        // which sum-check layers' claims the device forms: the mirrored top layer, slot-form layers below it, plain ones (a token of
        // its own: the lines of HG_DEBUG=plan are all numbers and are read as such)
        if (hg_debug("gpclaims"))
            fprintf(stderr, "[hg plan] gpclaims nb=%d layers=%d device=%d mirrored=%d slot=%d plain=%d\n", nb, nv - 1, ndev, ndev_mirrored, ndev_slot,
                    ndev - ndev_mirrored - ndev_slot);
        return out;
    }

    ClaimRef lasso_node(const u64* d_input) {
        // where the node enters the transcript: `ch.pos / 2` extension-field challenges have been squeezed before it (the argument
        // hg_lasso_prove_at takes to reproduce this section on its own)
        mark("lasso node: enters after " + std::to_string(ch.pos / 2) + " squeezed challenges (lasso.rs:57-114)");
        const LassoPlan& lp = pk->lasso;
        const dev::LassoDev& L = pk->lasso_dev;
        const int nu = lp.nu, A = lp.alpha;
        const size_t N = (size_t)1 << nu, M = 65536;
        // What this rank does of the node (single GPU: everything). Sharded over `world` GPUs the whole node is split BY MEMORY:
        // rank r owns the memories gkr_order[i] with gp1_mem_owner[i] == r and runs, for those, their E tables, their share of the
        // claimed sum, of the collation sum-check, of both grand products and of the openings. Every batched sum-check here is
        // linear in its batch items once p_0 is fixed, so every rank also keeps the one table that supplies p_0 (folded, never
        // summed: StJob::p0_only) and the ranks' round sums are partial sums that the exchange adds up.
        const int G = (int)lp.gkr_order.size();
        const bool split = world > 1;
        std::vector<int> local_pairs;  // global pair ids (reads / inits: i, writes / finals: G + i) this rank holds, ascending
        std::vector<int> local_mems;   // memory-GKR indices i it owns
        bool p0_only = false;          // pair 0 of the grand products is held only for p_0
        std::vector<char> own_mem(A, split ? 0 : 1);   // by memory index m
        if (split) {
            for (int i = 0; i < G; i++) if (mine(gp1_mem_owner[i])) { local_mems.push_back(i); own_mem[lp.gkr_order[i]] = 1; }
            p0_only = !mine(gp1_mem_owner[0]);
            if (p0_only) local_pairs.push_back(0);
            for (int i : local_mems) local_pairs.push_back(i);
            for (int i : local_mems) local_pairs.push_back(G + i);
        }
        bool any_gp1 = false;
        for (int n = 0; n < nu; n++) any_gp1 |= mine(gp1_owner[n]);
        const bool any_local = !split || !local_mems.empty();
        const bool do_col = any_local, do_open = any_local, do_gp2 = any_local;
        const bool need_counters = any_gp1 || do_gp2 || do_open;
        const bool need_split = do_col || need_counters;
        // E tables this rank materialises: its own memories, memory 0 (p_0 of the collation sum-check) and memory gkr_order[0] (pair
        // 0 of grand product #1). Row 0 is always memory 0 and the owned memories follow in ascending order, so the collation
        // sum-check's tables are rows [0, ncol) of `ep`.
        dev::EpRows ep_rows = dev::ep_rows_all(A), ep_rows_own = dev::ep_rows_all(A);
        std::vector<int> col_mems;     // memory indices of the collation tables held, table 0 first
        int ep_count = A;
        if (split) {
            for (int m = 0; m < 32; m++) ep_rows.row[m] = ep_rows_own.row[m] = -1;
            col_mems.push_back(0);
            for (int m = 1; m < A; m++) if (own_mem[m]) col_mems.push_back(m);
            ep_count = 0;
            for (int m : col_mems) ep_rows.row[m] = (signed char)ep_count++;
            if (ep_rows.row[lp.gkr_order[0]] < 0) ep_rows.row[lp.gkr_order[0]] = (signed char)ep_count++;
            for (int m = 0; m < A; m++) if (own_mem[m]) ep_rows_own.row[m] = ep_rows.row[m];
        } else for (int m = 0; m < A; m++) col_mems.push_back(m);
        const bool col_p0_only = split && !own_mem[0];
        // Lean form (wherever the hash-free first round is used): the E tables are NOT materialised.
        // E_m[j] = (row j's lookup uses m and limb < cutoff_m) ? limb : 0 is a select on a limb, so the hash round, the claimed sum and
        // the E_m(x) openings recompute it and the limb split writes E_0 (the collation sum-check's p_0 table) and C only.
        bool lean_e = false;
        {
            bool all1 = any_gp1;
            for (int n = 0; n < nu; n++) all1 = all1 && mine(gp1_owner[n]);
            const int nrows_ = split ? (int)local_pairs.size() : 2 * G;
            lean_e = all1 && nu >= 12 && nrows_ > (p0_only ? 1 : 0) && A <= 32;   // (= the condition of emit > 0 below)
        }
        const int ep_count_full = ep_count;   // (what the reference's traffic model writes)
        if (lean_e) {
            for (int m = 0; m < 32; m++) ep_rows.row[m] = ep_rows_own.row[m] = -1;
            ep_rows.row[0] = 0;
            ep_count = 1;
        }
        u32 own_mask = 0;
        for (int m = 0; m < A && m < 32; m++) if (own_mem[m]) own_mask |= 1u << m;
        // polynomialize (lasso.rs:157-250)
        // The limb table (dims[c][j]: limb c of row j) is not written: every reader - counter sorts, hash round / hash tables, openings -
        // takes the limbs from the node input it loads anyway (dev::LimbSrc). HG_LASSO_TABLES=1: the table, as the other provers keep it.
        const bool limbs_in = !lasso_tables() && dev::limbs_from_input_ok(L);
        const dev::LimbSrc limb_src = dev::limb_src(L, d_input);
        u64* dims = nullptr;
        u64* ep = nullptr;
        auto epm = [&](int m) -> const u64* {
            if (ep_rows.row[m] < 0) throw Error("lasso: E table of a memory this rank does not hold");
            return ep + (size_t)ep_rows.row[m] * N;
        };
        if (need_split) {
            if (!limbs_in) dims = ctx->alloc_n<u64>(4 * N);
            // one more row behind the E tables: C = sum_m M^m E_m over this rank's memories - with E_0 all the collation sum-check needs
            ep = ctx->alloc_n<u64>((size_t)(ep_count + 1) * N);
            dev::ColPow cp;
            memset(&cp, 0, sizeof(cp));
            {
                u64 mp = 1;
                for (int m = 0; m < A; m++) { if (own_mem[m]) cp.v[m] = mp; mp = gl_mul(mp, M); }
            }
            // two streams: the limbs first, in their own small launch - the counter sorts (second stream) need nothing else and start
            // while the E tables are still being written
            // (limbs from the input: nothing of the node is ahead of the event - it stays where it is, the counters still wait for it)
            if (fork_recorded) {
                if (!limbs_in) {
                    ctx->prof_begin(cls_aux, (double)N * 8 * (1 + 4));
                    dev::lasso_dims(st, L, d_input, dims);
                    ctx->prof_end();
                }
                hip_check(hipEventRecord(ctx->ev_aux[0], st), "lasso: limbs event");
            }
            const int dim_rows = fork_recorded ? 0 : 4;   // (the reference's traffic model writes the limb table)
            ctx->prof_begin(cls_aux, (double)N * 8 * (1 + (limbs_in ? 0 : dim_rows) + ep_count + 1), (double)N * 8 * (1 + dim_rows + ep_count_full + 1));
            dev::lasso_split(st, L, d_input, fork_recorded ? nullptr : dims, ep, ep_rows, &cp, ep + (size_t)ep_count * N);
            stamp("limb split done");
            ctx->prof_end();
            if (fork_recorded) hip_check(hipEventRecord(ctx->ev_aux[2], st), "lasso: E tables event");
        }
        // MemoryCheckingProver::new (prover.rs:35-89)
        const int nrows = split ? (int)local_pairs.size() : 2 * G;
        // Grand product #1 without hash tables: the top layer's first round recomputes the hashes from dims / read_ts / E and
        // writes tree level 1, the next layers' first rounds write levels 2 .. emit (a fifth level-emitting layer: no gain). Small
        // tables and sharded ranks that do not run every layer take the classic path: hash rows and tree levels materialised.
        constexpr int emit_max = 4;
        bool all_gp1 = any_gp1;
        for (int n = 0; n < nu; n++) all_gp1 = all_gp1 && mine(gp1_owner[n]);
        int emit = 0;
        if (all_gp1 && nu >= 12 && nrows > (p0_only ? 1 : 0))
            for (int n = nu - 1; n >= 12 && emit < emit_max; n--) emit++;   // layers with 2^n >= 4096 entries per table
        // Off the critical path, on the second stream: counter sorts (hidden under the collation sum-check), grand product #2's
        // hashes and tree, the openings (hidden under grand product #1's rounds). Needs the hash-free grand product #1 (the
        // classic path reads read_ts on the main stream right away).
        const bool use_aux = fork_recorded && emit > 0;
        auto aux = [&](const std::function<void()>& fn) { if (use_aux) on_aux(fn); else fn(); };
        // r, claimed sum (lasso.rs:85, 264-269)
        size_t r_off = epos();
        for (int i = 0; i < nu; i++) squeeze();
        // eq(r, .) and the opening point's table below have ONE reader each (the claimed sum, the openings at x): where the reader's
        // launch shape admits it, only their factor tables are built (eq_prep_now) and the reader forms the product per row.
        // HG_LASSO_TABLES=1: the tables, filled and read back.
        E2* eq = nullptr;
        auto eq_table = [&]() -> E2* { if (!eq) eq = ctx->alloc_n<E2>(N); return eq; };
        bool claim_ab = false, open_ab = false;
        size_t claim_slot = slot(1);
        // Stream assignment inside the node (one rank): the main stream goes from the limb split to the first hash round; counters,
        // grand product #2's tree and the opening tables on the second stream; the collation rounds on the third (col_third below).
        // A sharded rank keeps the collation rounds on the main stream ahead of its grand products. (Measured and removed in round 5:
        // the collation sum-check and the claimed sum on the second stream with the counters leading the main one, 3.8-3.9 against
        // 3.55 ms; the collation rounds behind the counters on the second stream, 2.74-2.82 against 2.64 ms; the counters on the
        // main stream, 3.87 against 3.63 ms.)
        // The claimed sum is only a result slot: with two streams it runs on the second one after grand product #2's tree (the main
        // stream goes from the limb split straight into the collation rounds, the second stream is idle at that point anyway).
        const bool claim_late = use_aux;
        auto do_claim = [&] {
            E2* ab = (lean_e && !lasso_tables()) ? eq_prep_now(nu, r_off) : nullptr;
            claim_ab = ab != nullptr;
            if (!ab) eq_now(eq_table(), nu, r_off, nullptr, !use_aux);   // (one stream: the opening point's table takes the buffer later)
            int grid = lean_e ? dev::lasso_claim_in(st, L, ab ? ab : eq, d_input, own_mask, partials, ab != nullptr)
                              : dev::lasso_claim(st, L, eq, ep, ep_rows_own, partials);  // sharded: this rank's memories only (partial sum)
            reduce(grid, 1, claim_slot);
        };
        if (do_col && !claim_late) do_claim();
        Cell claimed = cell();
        mark("lasso: claimed sum (lasso.rs:100-107)");
        push_op([this, claim_slot, claimed] { *claimed = h_res()[claim_slot]; proof.write_e(*claimed); });
        {   // collation sum-check (lasso.rs:271-279): g = poly(0) * sum_i M^i poly(i). Only the SUM enters the round polynomials and the
            // final evaluations are dropped (lasso.rs:97), so the sum-check runs on two tables: E_0 (supplies p_0, not summed) and
            // C = sum_i M^i E_i, written by the limb split (folding is linear: fold(C) = sum_i M^i fold(E_i)). Sharded: every rank's C
            // holds its own memories' terms, the round sums are partial sums.
            dev::Powers pw;
            memset(&pw, 0, sizeof(pw));
            if (A > dev::PW_MAX) throw Error("lasso: too many memories");
            pw.v[0] = e2_one(); pw.v[1] = e2_one();
            const bool col_run = do_col && (int)col_mems.size() > (col_p0_only ? 1 : 0);
            StrideArgs sa;
            sa.enqueue = col_run; sa.p0_only = true; sa.model_ntab = (int)col_mems.size();
            ScHandle sc = sc_stride(dev::SC_COLLATION, ep, true, (size_t)ep_count * N, 2, nu, pw, nullptr, sa);
            mark("lasso: collation sum-check, " + std::to_string(nu) + " rounds x 3 coefficients (lasso.rs:271-279) [C1, C3; poly(0) quirk]");
            defer_sumcheck(sc, 2, claimed, nullptr);
        }
        E2 gamma_e = squeeze(), tau_e = squeeze();  // lasso.rs:99
        u64 gamma = gamma_e.c0, tau = tau_e.c0;     // prover.rs:38-39: base limb 0 only
        // counters: only the memories whose index equals a chunk (dimension) index reach the transcript
        // (lasso.rs:317-319 indexes read_ts/final_cts by chunk index)
        // a rank that only holds a few memories of grand product #1 needs the counters of their chunks only
        // (the chunk of pair 0, and the chunks whose dim / read_ts / final_cts openings it owns: those of its own memories)
        std::vector<char> need_chunk(4, split ? 0 : 1);
        if (split) {
            if (p0_only) need_chunk[lp.gkr_chunk[0]] = 1;
            for (int i : local_mems) need_chunk[lp.gkr_chunk[i]] = 1;
        }
        std::map<int, u64*> read_ts, final_cts;
        // The counters feed grand product #1's first launch; on the second stream they hide under the collation rounds.
        // The collation rounds - 0.2 ms of short launches whose results only the host reads - run on a THIRD stream forked from the main
        // one behind the E tables and joined to it at the end of the prove (one rank): the main stream goes from the limb split
        // straight to the first hash round (which waits for the counters only). 2.574 -> 2.524 ms (96 replays each).
        // (Forked from and joined to the ORIGIN stream of the capture, like the second stream: a stream forked from the second one
        // and joined back into it sent hipStreamEndCapture into an endless recursion on a sharded rank's graph, NOTEBOOK.md.)
        const bool col_third = use_aux && world == 1 && fork_recorded;
        if (col_third) on_col([&] { flush_stride(); });
        else if (use_aux) flush_stride();  // collation rounds first: see below
        bool counters_event_recorded = false;
        if (need_counters) aux([&] {
            if (use_aux) hip_check(hipStreamWaitEvent(st, ctx->ev_aux[0], 0), "lasso: wait for the limb split");
            // all requested chunks in ONE stable sort of (chunk, address) keys
            unsigned mask = 0;
            for (auto& chk : lp.chunks) {
                int c = chk.first;
                if (c < 0 || c >= 4 || !need_chunk[c]) continue;
                mask |= 1u << c;
                read_ts[c] = ctx->alloc_n<u64>(N);
                final_cts[c] = ctx->alloc_n<u64>(M);
            }
            const size_t elems = std::max<size_t>(dev::lasso_counters_all_elems(L, mask), 1);
            size_t tb = dev::lasso_counters_all_temp_bytes(elems);
            void* temp = ctx->alloc(tb);
            u32* keys = ctx->alloc_n<u32>(elems); u32* keys2 = ctx->alloc_n<u32>(elems);
            u32* rows = ctx->alloc_n<u32>(elems); u32* rows2 = ctx->alloc_n<u32>(elems);
            u32* starts = ctx->alloc_n<u32>(4 * 65536 + 1);
            ctx->prof_begin(cls_aux, (double)elems * 40);
            dev::CounterOut co;
            memset(&co, 0, sizeof(co));
            for (int c = 0; c < 4; c++) if ((mask >> c) & 1) { co.read_ts[c] = read_ts[c]; co.final_cts[c] = final_cts[c]; }
            dev::lasso_counters_all(st, L, mask, dims, co, temp, tb, keys, keys2, rows, rows2, starts, limbs_in ? d_input : nullptr);
            ctx->prof_end();
            stamp("counters done");
            if (use_aux) { hip_check(hipEventRecord(ctx->ev_aux[3], st), "lasso: counters event"); counters_event_recorded = true; counters_event_live = true; }
        });
        // the collation rounds are launched now, not with the grand products at the end of the node: the host still has the whole
        // memory-checking bookkeeping to walk (about 0.5 ms) and the main stream would sit idle meanwhile; behind the counters, so
        // that the second stream (grand product #2's tree, openings) can start while they run
        flush_stride();
        const dev::GpHashSrc* d_hash_src = nullptr;
        double hash_build_bytes = 0;
        if (emit > 0) {
            std::vector<dev::GpHashMem> hm;
            auto row_of = [&](int pair) -> int {
                if (!split) return pair;
                for (size_t q = 0; q < local_pairs.size(); q++) if (local_pairs[q] == pair) return (int)q;
                return -1;
            };
            for (int i = 0; i < G; i++) {  // memory-GKR order is chunk-major
                dev::GpHashMem m;
                m.chunk = lp.gkr_chunk[i]; m.rd_row = row_of(i); m.wr_row = row_of(G + i);
                m.mem = lp.gkr_order[i]; m.cutoff = L.mem_cutoff[m.mem];
                if (m.rd_row >= 0 || m.wr_row >= 0) { m.ep = lean_e ? nullptr : epm(lp.gkr_order[i]); hm.push_back(m); }
            }
            dev::GpHashSrc hs;
            memset(&hs, 0, sizeof(hs));
            for (int c = 0; c < 4; c++) { hs.dim[c] = dims ? dims + (size_t)c * N : d_input; hs.ts[c] = read_ts.count(c) ? read_ts[c] : nullptr; }
            if (limbs_in) { hs.input = d_input; hs.limb_sh = 16; memcpy(hs.lookup_mask, L.lookup_mask, sizeof(hs.lookup_mask)); }
            else memset(hs.lookup_mask, 0xFF, sizeof(hs.lookup_mask));
            for (auto& m : hm) if (!hs.ts[m.chunk]) throw Error("lasso: counters of a needed chunk were not computed");
            dev::GpHashMem* d_hm = ctx->alloc_n<dev::GpHashMem>(hm.size());
            upload(d_hm, hm.data(), hm.size() * sizeof(dev::GpHashMem), "upload hash sources");
            hs.mems = d_hm; hs.nmem = (int)hm.size(); hs.gamma = gamma; hs.gamma2 = gl_mul(gamma, gamma); hs.tau = tau;
            hs.seg_shift = L.seg_shift; hs.rows = L.rows; hs.seg_lookup = L.seg_lookup;
            memcpy(hs.lookup_uses, L.lookup_uses, sizeof(hs.lookup_uses));
            hash_recomp = lean_e;
            // Slot form (kernels.hpp, GpHashSrc::slot_of): inside a lookup's row segment the memories it does not use have, per chunk,
            // identical hash rows, and the top layer multiplies segment s with segment s + npairs (Layer::bottom splits a row into
            // halves): memories in the same class in both segments share one table pair until the tables are down to the segment pairs.
            // HG_SLOT_DEPTH = number of slot-form layers (default 4; 0 = the memory form throughout, the path small tables take anyway)
            static const int depth_max = [] { const char* e = getenv("HG_SLOT_DEPTH"); return e && *e ? atoi(e) : 4; }();
            gp_slots = GpSlots();
            const int nvars_top = nu - 1;
            // rows of the grand product as this rank holds them (all of them on one GPU; its own memories' on a sharded rank): reads first
            std::vector<int> rowmem;    // memory-GKR index of row t
            std::vector<char> roww;     // write row?
            if (!split) { for (int t = 0; t < 2 * G; t++) { rowmem.push_back(t % G); roww.push_back(t >= G); } }
            else for (int b : local_pairs) { rowmem.push_back(b % G); roww.push_back(b >= G); }
            const int NL = (int)rowmem.size();
            int R = 0;
            while (R < NL && !roww[R]) R++;
            std::vector<int> read_row_of(G, -1);
            for (int t = 0; t < R; t++) read_row_of[rowmem[t]] = t;
            bool rows_fit = (int)hm.size() == R && R >= 2 && NL <= 64;
            for (int t = 0; t < R && rows_fit; t++) rows_fit = hm[t].rd_row == t;           // (the hash kernel walks hm by read row)
            for (int t = R; t < NL && rows_fit; t++) rows_fit = roww[t] && read_row_of[rowmem[t]] >= 0;
            if (rows_fit && depth_max > 0 && G <= 32 && L.seg_shift >= 9 && nvars_top - 1 > L.seg_shift &&
                ((N / 2) >> L.seg_shift) <= 64 && nvars_top - 1 - slot_tail_h(2 * R + 1, nvars_top) <= L.seg_shift) {
                const int NP = (int)((N / 2) >> L.seg_shift);
                auto cls = [&](int i, int s) -> int {   // class of GKR position i in row segment s: itself where its memory is looked up, else its chunk
                    if (((size_t)s << L.seg_shift) < L.rows && ((L.lookup_uses[lp.seg_lookup[s]] >> lp.gkr_order[i]) & 1)) return 1000 + i;
                    return lp.gkr_chunk[i];
                };
                if (hg_debug("slots"))   // joint classes of deeper layers: layer d multiplies 2^(d+1) segments NP >> d apart
                    for (int d = 0; d < 4 && (NP >> d) >= 1; d++) {
                        const int np = NP >> d, cnt = 2 << d;
                        int vmax = 0;
                        for (int sp = 0; sp < np; sp++) {
                            std::vector<std::vector<int>> keys;
                            for (int i = 0; i < G; i++) {
                                std::vector<int> key;
                                for (int q = 0; q < cnt; q++) key.push_back(cls(i, sp + q * np));
                                if (std::find(keys.begin(), keys.end(), key) == keys.end()) keys.push_back(key);
                            }
                            vmax = std::max(vmax, (int)keys.size());
                        }
                        fprintf(stderr, "[hg slots] layer %d: %d segment groups of %d, at most %d classes of %d memories\n", d, np, cnt, vmax, G);
                    }
                GpSlots& gs = gp_slots;
                gs.NP = NP; gs.G = R; gs.seg_shift = L.seg_shift;
                // layer d multiplies 2^(d+1) segments NP >> d apart: its classes are over those; rows: reads (layer 0), reads then writes
                for (int d = 0; d < std::min(depth_max, emit); d++) {
                    SlotLayer sl;
                    sl.ng = NP >> d; sl.nrows = d == 0 ? R : NL;
                    const int nvars_d = nu - 1 - d;
                    if (sl.ng < 2 || nvars_d - 1 <= L.seg_shift || nvars_d - 1 - slot_tail_h(d == 0 ? 2 * R + 1 : 2 * NL, nvars_d) > L.seg_shift) break;
                    sl.slot_of.assign((size_t)sl.nrows * sl.ng, 0);
                    std::vector<std::vector<int>> reps(sl.ng);
                    for (int g = 0; g < sl.ng; g++) {
                        std::vector<std::vector<int>> keys;
                        for (int b = 0; b < sl.nrows; b++) {
                            std::vector<int> key;
                            if (b == 0) key.push_back(-1);   // row 0 alone: p_0
                            else {
                                key.push_back(roww[b] ? 1 : 0);
                                for (int q = 0; q < (2 << d); q++) key.push_back(cls(rowmem[b], g + q * sl.ng));
                            }
                            int v = -1;
                            for (size_t q = 0; q < keys.size(); q++) if (keys[q] == key) v = (int)q;
                            if (v < 0) { v = (int)keys.size(); keys.push_back(key); reps[g].push_back(b); }
                            sl.slot_of[(size_t)b * sl.ng + g] = (uint8_t)v;
                        }
                        sl.V = std::max(sl.V, (int)keys.size());
                    }
                    if (sl.V >= sl.nrows || sl.V > 64) break;   // (nothing to gain)
                    sl.rep.assign((size_t)sl.V * sl.ng, 255);
                    for (int g = 0; g < sl.ng; g++) for (size_t v = 0; v < reps[g].size(); v++) sl.rep[v * sl.ng + g] = (uint8_t)reps[g][v];
                    gs.layer.push_back(sl);
                }
                // where each layer's first round writes the next tree level: the next layer's slot rows, or the per-memory rows
                for (size_t d = 0; d < gs.layer.size(); d++) {
                    SlotLayer& sl = gs.layer[d];
                    const SlotLayer* nx = d + 1 < gs.layer.size() ? &gs.layer[d + 1] : nullptr;
                    const int T = nx ? nx->V : NL, ngn = sl.ng / 2;
                    std::vector<u64> em((size_t)sl.V * sl.ng * (d == 0 ? 2 : 1), 0);
                    for (int g = 0; g < sl.ng; g++)
                        for (int t = 0; t < T; t++) {
                            const int b = nx ? nx->rep[(size_t)t * ngn + (g % ngn)] : t;   // the row whose values target row t holds there
                            if (b == 255) continue;
                            if (d == 0) {   // (the top layer holds the read rows only: a write row's values come from its read row's class)
                                const int u = sl.slot_of[(size_t)(roww[b] ? read_row_of[rowmem[b]] : b) * sl.ng + g];
                                em[(roww[b] ? (size_t)sl.V * sl.ng : 0) + (size_t)u * sl.ng + g] |= (u64)1 << t;
                            } else em[(size_t)sl.slot_of[(size_t)b * sl.ng + g] * sl.ng + g] |= (u64)1 << t;
                        }
                    sl.d_slot_of = ctx->alloc_n<uint8_t>(sl.slot_of.size());
                    sl.d_rep = ctx->alloc_n<uint8_t>(sl.rep.size());
                    sl.d_slotw = ctx->alloc_n<E2>(2 * (size_t)sl.V * sl.ng);
                    sl.d_ratio = ctx->alloc_n<E2>((size_t)sl.nrows * sl.ng);
                    sl.d_emit = ctx->alloc_n<u64>(em.size());
                    upload(sl.d_slot_of, sl.slot_of.data(), sl.slot_of.size(), "upload slot map");
                    upload(sl.d_rep, sl.rep.data(), sl.rep.size(), "upload slot representatives");
                    upload(sl.d_emit, em.data(), em.size() * sizeof(u64), "upload slot emission masks");
                }
                if (hg_debug("slots")) {
                    std::string vs;
                    for (auto& sl : gs.layer) vs += " " + std::to_string(sl.V) + "/" + std::to_string(sl.nrows);
                    fprintf(stderr, "[hg slots] adopted: %d layers, classes / rows per layer:%s\n", (int)gs.layer.size(), vs.c_str());
                }
                if (!gs.layer.empty()) {
                    const SlotLayer& s0 = gs.layer[0];
                    gs.V = s0.V;
                    hs.slot_of = s0.d_slot_of; hs.rep = s0.d_rep; hs.slotw = s0.d_slotw; hs.npairs = NP; hs.nslots = s0.V;
                    hs.emit_rd = s0.d_emit; hs.emit_wr = s0.d_emit + (size_t)s0.V * s0.ng;
                }
            }
            dev::GpHashSrc* d_hs = ctx->alloc_n<dev::GpHashSrc>(1);
            upload(d_hs, &hs, sizeof(hs), "upload hash sources");
            d_hash_src = d_hs;
            // algorithmic bytes of the hash build this replaces (the accounting of lasso_hash_rw below): dim + read_ts per chunk in
            // use, E read and read / write hash rows written per memory; level 1 is credited by sc_stride (next_level)
            std::vector<char> chunk_used(4, 0);
            for (auto& m : hm) chunk_used[m.chunk] = 1;
            hash_build_bytes = 0;
            for (int c = 0; c < 4; c++) if (chunk_used[c]) hash_build_bytes += (double)N * 8 * 2;
            for (auto& m : hm) hash_build_bytes += (double)N * 8 * ((m.rd_row >= 0) + (m.wr_row >= 0) + (lean_e ? 0 : 1));
            hash_model_extra = lean_e ? (double)N * 8 * (double)hm.size() : 0.0;   // the E reads of the reference's hash build: not streamed here
            // what the kernel really reads: dim + read_ts of every chunk in use, the E tables unless they are recomputed, the row -> lookup map
            hash_design_reads = (lean_e ? 0.0 : (double)N * 8 * (double)hm.size()) + (double)N;
            for (int c = 0; c < 4; c++) if (chunk_used[c]) hash_design_reads += (double)N * 8 * 2;
        }
        u64* H1 = (any_gp1 && !emit) ? ctx->alloc_n<u64>((size_t)nrows * N) : nullptr;
        u64* L1 = (any_gp1 && !emit && gp_deepest(nu, gp1_owner) >= 1) ? ctx->alloc_n<u64>((size_t)nrows * (N / 2)) : nullptr;
        u64* H2 = do_gp2 ? ctx->alloc_n<u64>((size_t)nrows * M) : nullptr;   // sharded: the rows of local_pairs only
        // hash launches are grouped by chunk: the memories of a chunk share the dim / read_ts columns
        struct HashReq { int i; u64 *rd, *wr, *rd1, *wr1; };
        std::vector<HashReq> reqs;
        auto hash_rw = [&](int i, u64* rd, u64* wr, u64* rd1, u64* wr1) { reqs.push_back({i, rd, wr, rd1, wr1}); };
        if (emit > 0) {
            // nothing to hash here
        } else if (any_gp1 && !split) {
            for (int i = 0; i < G; i++)
                hash_rw(i, H1 + (size_t)i * N, H1 + (size_t)(G + i) * N, L1 ? L1 + (size_t)i * (N / 2) : nullptr, L1 ? L1 + (size_t)(G + i) * (N / 2) : nullptr);
        } else if (any_gp1) {
            const int base = p0_only ? 1 : 0, nlm = (int)local_mems.size();
            if (p0_only) {  // table 0 (reads of the first memory) supplies p_0; its write table is not needed here
                u64* junk = ctx->alloc_n<u64>(N + N / 2);
                hash_rw(0, H1, junk, L1 ? L1 : nullptr, L1 ? junk + N : nullptr);
            }
            for (int q = 0; q < nlm; q++)
                hash_rw(local_mems[q], H1 + (size_t)(base + q) * N, H1 + (size_t)(base + nlm + q) * N,
                        L1 ? L1 + (size_t)(base + q) * (N / 2) : nullptr, L1 ? L1 + (size_t)(base + nlm + q) * (N / 2) : nullptr);
        }
        for (int c = 0; c < 4; c++) {
            std::vector<HashReq> of_c;
            for (auto& r : reqs) if (lp.gkr_chunk[r.i] == c) of_c.push_back(r);
            for (size_t o = 0; o < of_c.size(); o += dev::HASH_RW_MAX) {
                const int cnt = (int)std::min<size_t>(dev::HASH_RW_MAX, of_c.size() - o);
                dev::HashRwArgs ha;
                memset(&ha, 0, sizeof(ha));
                for (int q = 0; q < cnt; q++) {
                    const HashReq& r = of_c[o + q];
                    ha.ep[q] = epm(lp.gkr_order[r.i]); ha.rd[q] = r.rd; ha.wr[q] = r.wr; ha.rd1[q] = r.rd1; ha.wr1[q] = r.wr1;
                }
                ctx->prof_begin(cls_hash, (double)N * 8 * (2 + cnt * (L1 ? 4 : 3)));
                dev::lasso_hash_rw(st, N, dims ? dims + (size_t)c * N : nullptr, read_ts[c], ha, cnt, gamma, tau, &limb_src, c);
                ctx->prof_end();
            }
        }
        if (do_gp2) aux([&] {
            if (G > 32) throw Error("lasso: more than 32 memories");
            dev::HashIfArgs ha;
            memset(&ha, 0, sizeof(ha));
            for (int i = 0; i < G; i++) {
                ha.cutoff[i] = (u32)lp.mems[lp.gkr_order[i]].cutoff;
                ha.row_init[i] = split ? -1 : i; ha.row_fin[i] = split ? -1 : G + i;
                if (split)
                    for (size_t q = 0; q < local_pairs.size(); q++) {
                        if (local_pairs[q] == i) ha.row_init[i] = (int)q;
                        if (local_pairs[q] == G + i) ha.row_fin[i] = (int)q;
                    }
                ha.fc[i] = ha.row_fin[i] >= 0 ? final_cts[lp.gkr_chunk[i]] : nullptr;   // (init hashes do not read the counters)
                if (ha.row_fin[i] >= 0 && !ha.fc[i]) throw Error("lasso: counters of a needed chunk were not computed");
            }
            ctx->prof_begin(cls_hash, (double)nrows * M * 8 * 1.5);
            dev::lasso_hash_if(st, ha, G, gamma, tau, H2);
            ctx->prof_end();
        });
        mark("lasso: memory checking, grand product #1 over reads then writes (prover.rs:161-165)");
        // the write hash of a row is its read hash + gamma^2 (prover.rs:44: t + 1): the top layer runs on the read rows only
        constexpr bool use_mirror = true;
        const u64 gamma_sq = gl_mul(gamma, gamma);
        const u64* mirror_c = (emit > 0 && use_mirror) ? &gamma_sq : nullptr;
        GpOut g1 = split ? grand_product(H1, N, 2 * G, gp1_owner, L1, &local_pairs, p0_only, d_hash_src, emit, hash_build_bytes, mirror_c)
                         : grand_product(H1, N, 2 * G, gp1_owner, L1, nullptr, false, d_hash_src, emit, hash_build_bytes, mirror_c);  // reads then writes (prover.rs:161-165)
        mark("lasso: memory checking, grand product #2 over inits then finals (prover.rs:167-171)");
        GpOut g2{0, nullptr};
        aux([&] {   // inits then finals (prover.rs:167-171); its tree on the second stream
            g2 = split ? grand_product(H2, M, 2 * G, std::vector<int>(16, rank), nullptr, &local_pairs, p0_only)
                       : grand_product(H2, M, 2 * G, std::vector<int>(16, rank));
        });
        if (use_aux) {
            // grand product #1's first launch reads the counters, grand product #2's first rounds its tree: the main stream waits
            // for the second one only there, after the collation sum-check has been enqueued
            on_aux([&] { stamp("grand product #2's tree done"); });
            hip_check(hipEventRecord(ctx->ev_aux[1], ctx->stream2), "lasso: aux event");
            on_aux([&] { hip_check(hipStreamWaitEvent(st, ctx->ev_aux[2], 0), "lasso: wait for the E tables"); });   // claimed sum, openings
            // (the claimed sum's launches follow the grand products' below: see the openings)
            hg_ctx* c = ctx;
            // the first launches (the hash-free first round of the top layer, the next layers' level-emitting first rounds) only
            // need the counters; grand product #2's jobs join from the mixed first-round launch on and need its tree
            const bool two_waits = counters_event_recorded;
            st_before_gp = [c, two_waits] { hip_check(hipStreamWaitEvent(c->stream, c->ev_aux[two_waits ? 3 : 1], 0), "lasso: wait for the counters"); };
            if (two_waits) st_before_gp2 = [c] { hip_check(hipStreamWaitEvent(c->stream, c->ev_aux[1], 0), "lasso: wait for grand product #2's tree"); };
        }
        // openings (prover.rs:173-178, mod.rs:80-93). With two streams eq(r, .) may still be in use by the claimed-sum kernel on
        // the main stream, so the openings get their own table.
        // Their launches (and the claimed sum's) are enqueued AFTER the grand products': a replayed launch graph submits its nodes in
        // the order they were recorded, a few microseconds each, so the main stream's first grand-product kernel could not start before
        // everything recorded ahead of it was out - on a sharded rank, whose kernels are short, that left the main stream idle for
        // 100-150 us (scripts/ub/graph_order.hip shows the effect in isolation).
        E2* eqy = do_open ? ctx->alloc_n<E2>(M) : nullptr;
        // every opening at x in one launch, every opening at y in another (dev::dot_eq_many): results land in their wire slots
        dev::DotTabs tx, ty;
        memset(&tx, 0, sizeof(tx)); memset(&ty, 0, sizeof(ty));
        int nx = 0, ny = 0;
        {
        auto add_x = [&](const u64* tab, size_t out_slot) {
            if (nx >= dev::DOT_MAX) throw Error("lasso: too many openings");
            tx.t[nx] = tab; tx.slot[nx] = (int)out_slot; nx++;
        };
        struct ChunkSlots { int c; size_t base, count; };
        std::vector<ChunkSlots> chunk_slots;
        for (auto& chk : lp.chunks) {
            const int c = chk.first;
            // order on the wire: dim(x), read_ts(x), final_cts(y), then E_m(x)
            // sharded: dim(x), read_ts(x), final_cts(y) of a chunk belong to the owner of its first memory, E_m(x) to the owner of m
            const bool own_chunk = do_open && own_mem[chk.second[0]];
            const size_t base_slot = slot(3 + chk.second.size());
            if (own_chunk) {
                if (dims) add_x(dims + (size_t)c * N, base_slot);
                else { if (nx >= dev::DOT_MAX) throw Error("lasso: too many openings"); tx.t[nx] = nullptr; tx.emem[nx] = (signed char)(-1 - c); tx.slot[nx] = (int)base_slot; nx++; }
                add_x(read_ts[c], base_slot + 1);
                ty.t[ny] = final_cts[c]; ty.slot[ny] = (int)(base_slot + 2); ny++;
            }
            for (size_t i = 0; i < chk.second.size(); i++)
                if (do_open && own_mem[chk.second[i]]) {
                    if (lean_e) { if (nx >= dev::DOT_MAX) throw Error("lasso: too many openings"); tx.t[nx] = nullptr; tx.emem[nx] = (signed char)chk.second[i]; tx.slot[nx] = (int)(base_slot + 3 + i); nx++; }
                    else add_x(epm(chk.second[i]), base_slot + 3 + i);
                }
            chunk_slots.push_back({c, base_slot, 3 + chk.second.size()});
        }
        for (auto& cs : chunk_slots) {
            mark("lasso: openings of chunk " + std::to_string(cs.c) + ": dim(x), read_ts(x), final_cts(y), E_m(x) (prover.rs:173-178)");
            defer_write_slots(cs.base, cs.count);
        }
        }
        flush_stride();  // collation + every grand-product layer, round-synchronised
        aux([&] { if (do_col && claim_late) do_claim(); });
        {
            // the openings (two dot-product launches over every opened table: bandwidth) by value, so that they can also run later
            const dev::DotTabs txv = tx, tyv = ty;
            const int nxv = nx, nyv = ny;
            const bool lean_v = lean_e;
            E2* eqy_v = eqy;
            const size_t p1 = g1.point_off, p2 = g2.point_off;
            dev::DotVirt dv;
            memset(&dv, 0, sizeof(dv));
            const bool virt_v = lean_e || limbs_in;   // tables recomputed from the node input among the opened ones
            if (virt_v) {
                dv.input = d_input; dv.seg_lookup = L.seg_lookup; dv.seg_shift = L.seg_shift; dv.rows = L.rows;
                memcpy(dv.lookup_mask, L.lookup_mask, sizeof(dv.lookup_mask)); memcpy(dv.lookup_uses, L.lookup_uses, sizeof(dv.lookup_uses));
                memcpy(dv.mem_dim, L.mem_dim, sizeof(dv.mem_dim)); memcpy(dv.mem_cutoff, L.mem_cutoff, sizeof(dv.mem_cutoff));
            }
            // (dot_eq_many's groups of eight re-read eq per group: where open_x does not take the shape the table is filled)
            open_ab = do_open && lean_e && nx > 0 && !lasso_tables() && nu >= 8 && nu <= 24 && dev::open_x_takes_ab(tx, nx, N, dv);
            // the two eq tables of the opening points are challenges only: built right away on the second stream (beside the first hash
            // round), whatever the place of the dot products - at the end of the second stream they ran alone, 0.05 ms of its length
            E2* eqx_v = nullptr;   // the table, or its factor tables (open_ab)
            aux([&] {
                if (!do_open) return;
                if (open_ab) eqx_v = eq_prep_now(nu, p1);
                else {
                    eqx_v = use_aux ? ctx->alloc_n<E2>(N) : eq_table();  // (one stream: the eq(r,.) table is dead by now)
                    eq_now(eqx_v, nu, p1, nullptr, !use_aux);
                }
                eq_now(eqy_v, 16, p2);
            });
            if (open_ab && !eqx_v) throw Error("lasso: no factor tables for the opening point");
            const bool open_ab_v = open_ab;
            if (use_aux && world == 1) hip_check(hipEventRecord(ctx->ev_aux[4], ctx->stream2), "lasso: opening tables event");
            auto openings = [this, txv, tyv, nxv, nyv, lean_v, virt_v, eqx_v, eqy_v, dv, open_ab_v, N] {
                if (nxv) {
                    int nvirt = 0;
                    for (int t = 0; t < nxv; t++) nvirt += txv.t[t] == nullptr;
                    // (a group of eight re-reads eq; recomputed E tables cost their group one 8-byte input read per entry)
                    ctx->prof_begin(cls_aux, (double)N * (16.0 * ((nxv + 7) / 8) + 8.0 * (nxv - nvirt) + (nvirt ? 8.0 * ((nxv + 7) / 8) : 0.0)),
                                    (double)N * (16.0 * ((nxv + 7) / 8) + 8.0 * nxv));   // (reference model: every opened table is read)
                    if (!(lean_v && dev::open_x(st, eqx_v, txv, nxv, N, partials, d_res(), dv, open_ab_v)))
                        dev::dot_eq_many(st, eqx_v, txv, nxv, N, partials, d_res(), virt_v ? &dv : nullptr);
                    ctx->prof_end();
                }
                if (nyv) dev::dot_eq_many(st, eqy_v, tyv, nyv, M, partials, d_res());
                stamp("claimed sum and openings done");
            };
            // Where the openings' dot products run (the two eq tables above are built right away in every case): behind the node
            // reductions, on THEIR stream (one rank: the third one, which waits for the opening tables of the second; a sharded rank:
            // the second). Since the eq-factored node reductions (round 5) those end 0.25 ms before the grand products do. Measured and
            // removed: right away beside the first hash round (1.846 ms), between the two waves of node reductions (1.864), at the end of
            // the main stream behind the grand products (1.87-1.91; the round-4 default) against 1.83-1.86 ms; a fourth stream for the
            // node reductions alone: 1.85 - a replayed launch graph does not run a fourth branch beside the other three (its first
            // kernel starts 0.6 ms into the prove, with or without GPU_MAX_HW_QUEUES=8).
            if (use_aux && world == 1) {
                late_col.push_back(openings);
            } else if (use_aux) late_aux.push_back(openings);
            else aux(openings);
        }
        // which form each piece took (out_eq: the output claim's table, enqueue_prove - the same rule, stated here). HG_DEBUG=plan,lasso:
        // a token of its own, since the launch-plan lines of HG_DEBUG=plan are all numbers and are read as such
        if (hg_debug("lasso")) {
            const int ov = pk->params.ct0is_log2();
            const bool out_ab = !lasso_tables() && eq_two_launch() && ov >= 8 && ov <= 24;
            fprintf(stderr, "[hg plan] lasso limbs=%s claim_eq=%s open_eq=%s out_eq=%s\n", limbs_in ? "input" : "table", claim_ab ? "factored" : "table",
                    open_ab ? "factored" : "table", out_ab ? "factored" : "table");
        }
        stamp("grand products done");
        return ClaimRef{r_off, nu, claimed};  // (r, claimed_sum) for the single predecessor (lasso.rs:97,113)
    }

