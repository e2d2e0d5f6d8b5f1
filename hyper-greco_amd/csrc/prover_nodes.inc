// Part of struct Prover (prover.hip includes this file inside the class body): the GKR driver (gkr::prove_gkr) - claim combination, Vanilla (Libra) and FFT (zkCNN) node reductions, the streams the node reductions and the Lasso node's side work run on.

    // ---- GKR driver ----------------------------------------------------------------------------
    std::map<std::pair<size_t, int>, E2*> eq_shared;             // (point, variables) -> eq table of a single unit-weight claim
    std::map<std::tuple<size_t, int, int>, E2*> fft_shared;      // (point, log2 size, inverse) -> DFT-row table of a single claim
    static bool share_tables() { return true; }
    std::vector<const u64*> d_vals;               // node values in HBM
    std::vector<std::vector<ClaimRef>> claims;    // per node

    dev::ClaimSet claim_set(const std::vector<ClaimRef>& cl, std::vector<E2>* alphas_host) {
        dev::ClaimSet cs;
        memset(&cs, 0, sizeof(cs));
        if (cl.empty()) throw Error("gkr: node without claim");
        if (cl.size() > (size_t)dev::MAX_CLAIMS) throw Error("gkr: too many claims on one node");
        cs.n = (int)cl.size();
        cs.unit_alpha = cl.size() == 1;
        cs.alpha_off = epos();
        alphas_host->clear();
        if (cl.size() > 1) for (size_t a = 0; a < cl.size(); a++) alphas_host->push_back(squeeze());
        else alphas_host->push_back(e2_one());
        for (size_t a = 0; a < cl.size(); a++) cs.point_off[a] = cl[a].point_off;
        return cs;
    }
    Cell combined_value(const std::vector<ClaimRef>& cl, const std::vector<E2>& alphas) {
        Cell v = cell();
        std::vector<Cell> vals;
        for (auto& c : cl) vals.push_back(c.value);
        push_op([v, vals, alphas] {
            E2 s = e2_zero();
            for (size_t a = 0; a < vals.size(); a++) s = e2_add(s, e2_mul(*vals[a], alphas[a]));
            *v = s;
        });
        return v;
    }

    void vanilla_node(int id) {
        const HNode& n = pk->circuit.nodes[id];
        const hg_pk::NodeDev& nd = pk->node_dev[id];
        const int nin = n.log2_sub_in + n.log2_reps;
        const size_t SR = (size_t)1 << nin;
        std::vector<E2> alphas;
        dev::ClaimSet cs = claim_set(claims[id], &alphas);
        for (auto& c : claims[id]) if (c.len != n.log2_out()) throw Error("gkr: claim arity mismatch");
        Cell claim = combined_value(claims[id], alphas);
        const bool own = mine(node_owner[id]);
        std::vector<int> li, ri;
        for (int i = 0; i < n.arity; i++) { if (n.left_use[i]) li.push_back(i); if (n.right_use[i]) ri.push_back(i); }
        if (n.arity > dev::PS_MAX_PAIRS) throw Error("vanilla: arity too large");
        // phase 1's transcript side, common to both forms below
        auto phase1_steps = [&](const ScHandle& s1, size_t u_base, Cell after1) {
            mark("vanilla node " + std::to_string(id) + ": Libra phase 1 sum-check, " + std::to_string(nin) + " rounds x 3 coefficients [G1 node order, G2 alpha per claim, G3 Libra form]");
            defer_sumcheck(s1, 2, claim, after1);
            for (int i : li) {
                mark("vanilla node " + std::to_string(id) + ": input " + std::to_string(i) + " evaluation at r_x");
                defer_write_slots(u_base + i, 1);
                Cell v = cell();
                size_t sl = u_base + i;
                push_op([this, v, sl] { *v = h_res()[sl]; });
                claims[n.preds[i]].push_back(ClaimRef{s1.point_off, nin, v});
            }
        };
        // Eq-factored form (kernels.hpp PsJob::eq_n; found at setup, hg_pk::NodeDev::EqForm): the node relays aligned blocks, so with
        // ONE claim at z every phase-1 table is kappa_i eq(z', .), z' = (z_0 .. z_(w-1), bits of hib), kappa_i = sum_t coef_t
        // eq(z_(w..); block_t). Neither the node's eq table nor any bookkeeping table is built; additive constants, which are constant
        // over those blocks, leave the claim as a scalar of the challenges.
        const hg_pk::NodeDev::EqForm& ef = nd.eq_form;
        const int eq_tail = ef.ok && cs.n == 1 && ps_eq_on() ? eq_tail_rd((int)li.size(), nin) : -1;
        if (eq_tail >= 0) {
            const u64* chain = challenge_chain(2 * (cs.point_off[0] + n.log2_out()));
            auto zc = [&](int k) { return e2(chain[2 * (cs.point_off[0] + k)], chain[2 * (cs.point_off[0] + k) + 1]); };
            const int hb = n.log2_out() - ef.w;
            auto eq_hi = [&](u32 block) {
                E2 acc = e2_one();
                for (int b = 0; b < hb; b++) acc = e2_mul(acc, (block >> b) & 1 ? zc(ef.w + b) : e2_sub(e2_one(), zc(ef.w + b)));
                return acc;
            };
            if (!ef.consts.empty()) {
                E2 c = e2_zero();
                for (auto& t : ef.consts) c = e2_add(c, e2_mul_f(eq_hi(t.second), t.first));
                push_op([claim, c] { *claim = e2_sub(*claim, c); });
            }
            std::vector<const u64*> a;
            std::vector<E2> kappa;
            std::vector<E2*> fa, fb;
            const size_t u_base = slot(n.arity);
            E2* scratch = own ? ctx->alloc_n<E2>(n.arity) : nullptr;
            for (int i : li) {
                E2 k = e2_zero();
                for (auto& t : ef.terms[i]) k = e2_add(k, e2_mul_f(eq_hi(t.second), t.first));
                a.push_back(d_vals[n.preds[i]]);
                kappa.push_back(k);
                fa.push_back(d_res() + u_base + i);
                fb.push_back(scratch + i);
            }
            std::vector<E2> zp(nin);
            for (int k = 0; k < nin; k++) zp[k] = k < ef.w ? zc(k) : e2((ef.hib >> (k - ef.w)) & 1u, 0);
            ScHandle s1 = sc_prodsum_eq(a, kappa, zp, cs.point_off[0], ef.w, ef.hib, nin, eq_tail, fa, fb, own);
            phase1_steps(s1, u_base, cell());
            return;
        }
        // Nodes that received their only claim from the same sum-check share the point (every input of a Vanilla node is opened at the
        // node's r_x: the five inputs of the final sum, the eight chunk nodes behind the Lasso input ...): one eq table serves them all
        // (read-only everywhere).
        E2* eqc = nullptr;
        if (own) {
            const std::pair<size_t, int> key{cs.point_off[0], n.log2_out()};
            auto hit = cs.n == 1 && share_tables() ? eq_shared.find(key) : eq_shared.end();
            if (hit != eq_shared.end()) eqc = hit->second;
            else {
                eqc = ctx->alloc_n<E2>((size_t)1 << n.log2_out());
                queue_eq(eqc, n.log2_out(), cs);
                if (cs.n == 1) eq_shared[key] = eqc;
            }
        }
        const hg_pk::NodeDev* ndp0 = &nd;
        const HNode* np0 = &n;
        if (nd.nconst) {  // claim -= sum_g eqc[g] * w0_g
            size_t s = slot(1);
            if (own) after_eq.push_back([this, ndp0, np0, eqc, s] {
                int grid = dev::vanilla_const_sum(st, ndp0->const_gate, ndp0->const_coef, ndp0->nconst, eqc, np0->log2_sub_out, np0->log2_reps, partials);
                reduce(grid, 1, s);
            });
            push_op([this, s, claim] { *claim = e2_sub(*claim, h_res()[s]); });
        }
        // phase 1: sum_x sum_i in_i(x) T_i(x)
        dev::GatherT gt;
        memset(&gt, 0, sizeof(gt));
        for (int i = 0; i < n.arity; i++) gt.in_vals[i] = d_vals[n.preds[i]];
        std::vector<const u64*> a;
        std::vector<const E2*> b;
        std::vector<E2*> fa, fb;
        size_t u_base = slot(n.arity);
        E2* scratch = own ? ctx->alloc_n<E2>(n.arity) : nullptr;
        // HG_GATHER_CSR=1: the general (per-term) form for every table
        static const bool use_seg = !hg_env_on("HG_GATHER_CSR");
        for (int i : li) {
            const hg_pk::NodeDev::Seg& sg = nd.seg[i];
            E2* T = nullptr;
            if (own && use_seg && sg.alias) T = eqc + sg.alias_off;   // one unit relay per position: the table is a slice of eqc
            else if (own) T = ctx->alloc_n<E2>(SR);
            gt.lin = nd.lin[i];
            gt.mul = nd.mulL[i];
            // (only a mul part reads the node inputs: a job without one names none, and its table depends on the challenges alone)
            const bool mul_part = gt.mul.ptr != nullptr;
            if (own && use_seg && sg.alias) {
            } else if (own && use_seg && sg.d) {
                dev::GatherSegJob sj;
                memset(&sj, 0, sizeof(sj));
                sj.segs = sg.d; sj.nseg = sg.nseg; sj.eqc = eqc; sj.log2_S = n.log2_sub_in; sj.log2_G = n.log2_sub_out; sj.log2_R = n.log2_reps; sj.T = T;
                if (mul_part) for (int q = 0; q < n.arity; q++) sj.in_vals[q] = gt.in_vals[q];
                gather_seg_queue.push_back(sj);
            } else if (own) {
                dev::GatherT g = gt;
                if (!mul_part) memset(g.in_vals, 0, sizeof(g.in_vals));
                gather_queue.push_back(dev::GatherJob{g, eqc, n.log2_sub_in, n.log2_sub_out, n.log2_reps, T});
            }
            a.push_back(d_vals[n.preds[i]]);
            b.push_back(T);
            fa.push_back(d_res() + u_base + i);
            fb.push_back(scratch + i);
        }
        ScHandle s1 = sc_prodsum(a, b, nin, fa, fb, own);
        Cell after1 = cell();
        phase1_steps(s1, u_base, after1);
        if (!n.mul.empty()) {
            if (!n.lin.empty()) throw Error("vanilla: nodes mixing linear and mul gates are not on this path");
            // phase 2: sum_y sum_i in_i(y) B_i(y), claim carried over from phase 1 (no linear part).
            // Transcript bookkeeping (challenges, slots) happens now, in protocol order; the device work
            // needs u = in(r_x) from phase 1 and is therefore queued for the second wave.
            std::vector<const u64*> a2;
            std::vector<E2*> Bs, fa2, fb2;
            size_t w_base = slot(n.arity);
            for (int i : ri) {
                E2* B = own ? ctx->alloc_n<E2>(SR) : nullptr;
                a2.push_back(d_vals[n.preds[i]]);
                Bs.push_back(B);
                fa2.push_back(d_res() + w_base + i);
                fb2.push_back(scratch + i);
            }
            size_t rx_off = s1.point_off;
            const hg_pk::NodeDev* ndp = &nd;
            const HNode* np = &n;
            // reserve the phase-2 sum-check (challenges + slots) now; attach its tables in the second wave
            ScHandle s2;
            s2.nv = 2; s2.nvars = nin; s2.point_off = epos(); s2.sums_slot = slot((size_t)nin * 2);
            for (int i = 0; i < nin; i++) s2.rs.push_back(squeeze());
            // (eq(r_x, .) depends on challenges only: it joins the FIRST wave's batch of eq tables - the second wave, which sits at the end
            // of the node chain, then starts with its gathers)
            E2* eqx = own ? ctx->alloc_n<E2>(SR) : nullptr;
            if (own) {
                dev::ClaimSet one;
                memset(&one, 0, sizeof(one));
                one.n = 1; one.unit_alpha = 1; one.point_off[0] = rx_off;
                queue_eq(eqx, nin, one);
            }
            // Phase 2 BESIDE phase 1 (round 6): its tables are u = in(r_x) times tables of challenges only when every term of the node
            // has the same left input (the sixteen mul nodes: out = a b), so they are built without u in the FIRST wave, the sum-check joins
            // the first wave's launches and the replay multiplies its round sums by u (ScHandle::scale_cell) - the second wave (a gather,
            // two round launches and a tail at the very end of the node chain: 0.12 ms) is gone. HG_PHASE2_LATE=1: as before.
            static const bool phase2_late = hg_env_on("HG_PHASE2_LATE");
            int left_in = -1;
            bool one_left = !phase2_late;
            for (const MulTerm& t : n.mul) { if (left_in < 0) left_in = (int)t.i0; else if ((int)t.i0 != left_in) one_left = false; }
            if (one_left && left_in >= 0) {
                Cell uc = cell();
                const size_t usl = u_base + (size_t)left_in;
                push_op([this, uc, usl] { *uc = h_res()[usl]; });
                s2.scale_cell = uc;
            }
            const bool early2 = (bool)s2.scale_cell;
            auto phase2_work = [this, ri, Bs, a2, fa2, fb2, ndp, np, eqc, eqx, u_base, nin, s2, early2] {
                for (size_t q = 0; q < ri.size(); q++)  // batched by flush_bookkeeping
                    gatherB_queue.push_back(dev::GatherBJob{ndp->mulR[ri[q]], eqc, eqx, early2 ? nullptr : d_res() + u_base, np->log2_sub_in, np->log2_sub_out, np->log2_reps, Bs[q]});
                const int npairs = (int)ri.size();
                const size_t N = (size_t)1 << nin;
                dev::PsJob J;
                memset(&J, 0, sizeof(J));
                J.npairs = npairs; J.nvars = nin; J.r_off = s2.point_off; J.sums_slot = s2.sums_slot;
                for (int q = 0; q < 2; q++) {
                    J.bufa[q] = ctx->alloc_n<E2>((size_t)npairs * std::max<size_t>(N >> (q + 1), 1));
                    J.bufb[q] = ctx->alloc_n<E2>((size_t)npairs * std::max<size_t>(N >> (q + 1), 1));
                }
                for (int q = 0; q < npairs; q++) { J.a[q] = a2[q]; J.b[q] = Bs[q]; J.fin_a[q] = fa2[q]; J.fin_b[q] = fb2[q]; }
                ps_queue[nin].push_back(J);
            };
            if (own && early2) phase2_work();
            else if (own) second_wave.push_back(phase2_work);
            mark("vanilla node " + std::to_string(id) + ": Libra phase 2 sum-check [G3]");
            defer_sumcheck(s2, 2, after1, nullptr);
            for (int i : ri) {
                mark("vanilla node " + std::to_string(id) + ": input " + std::to_string(i) + " evaluation at r_y");
                defer_write_slots(w_base + i, 1);
                Cell v = cell();
                size_t sl = w_base + i;
                push_op([this, v, sl] { *v = h_res()[sl]; });
                claims[n.preds[i]].push_back(ClaimRef{s2.point_off, nin, v});
            }
        }
    }

    void fft_node(int id) {
        const HNode& n = pk->circuit.nodes[id];
        const int L = n.log2_size;
        const size_t N = (size_t)1 << L;
        std::vector<E2> alphas;
        dev::ClaimSet cs = claim_set(claims[id], &alphas);
        Cell claim = combined_value(claims[id], alphas);
        const bool own = mine(node_owner[id]);
        // (the sixteen inverse-FFT nodes behind sai_par are all opened at sai_par's r_x: one DFT-row table)
        E2* F = nullptr;
        bool F_shared = false;
        if (own) {
            const std::tuple<size_t, int, int> key{claims[id].size() == 1 ? claims[id][0].point_off : (size_t)-1, L, n.inverse ? 1 : 0};
            auto hit = claims[id].size() == 1 && share_tables() ? fft_shared.find(key) : fft_shared.end();
            if (hit != fft_shared.end()) { F = hit->second; F_shared = true; }
            else {
                F = ctx->alloc_n<E2>(N);
                if (claims[id].size() == 1) fft_shared[key] = F;
            }
        }
        const u64* W = (n.inverse ? pk->w_inv : pk->w_fwd).at(L);
        u64 scale = n.inverse ? gl_inv(gl_from_u64(N)) : 1;
        if (own && !F_shared) fft_queue.push_back(dev::FftJob{F, W, scale, L, cs});
        size_t u = slot(1);
        E2* scratch = own ? ctx->alloc_n<E2>(1) : nullptr;
        ScHandle s = sc_prodsum({d_vals[n.preds[0]]}, {F}, L, {d_res() + u}, {scratch}, own);
        mark("fft node " + std::to_string(id) + ": zkCNN sum-check, " + std::to_string(L) + " rounds x 3 coefficients [G3 zkCNN form, G4 root of unity]");
        defer_sumcheck(s, 2, claim, nullptr);
        mark("fft node " + std::to_string(id) + ": input evaluation");
        defer_write_slots(u, 1);
        Cell v = cell();
        push_op([this, v, u] { *v = h_res()[u]; });
        claims[n.preds[0]].push_back(ClaimRef{s.point_off, L, v});
    }

    // The Vanilla / FFT node reductions run on a second stream, concurrently with the Lasso node: they are independent on the
    // device (claim points are challenges) and mostly small launches that leave CUs idle, while the Lasso node's critical
    // path has its own latency-bound stretches (counter sorts, openings, last rounds). The fork point is recorded BEFORE the
    // Lasso node is enqueued (record_fork, at the start of the walk); HG_ONE_STREAM=1 keeps everything on one stream.
    bool fork_recorded = false;
    void record_fork() {
        static const bool one_stream = hg_env_on("HG_ONE_STREAM");
        if (one_stream || ctx->one_stream) return;
        hip_check(hipEventRecord(ctx->ev_fork, ctx->stream), "fork event");   // after the result-buffer clear / ticket reset
        fork_recorded = true;
    }
    // Runs `fn` with the second stream as the enqueue target (work of the Lasso node that is off its critical path: counter
    // sorts, grand product #2's hashes and tree, the openings). One stream only: runs it in place.
    std::vector<std::function<void()>> late_aux;
    std::vector<std::function<void()>> late_col;   // the same, for whichever stream the node reductions run on; needs ev_aux[4]
    bool aux_started = false;
    template <typename Fn> void on_aux(Fn fn) {
        if (!fork_recorded) { fn(); return; }
        hipStream_t s0 = st;
        E2* p0 = partials;
        if (!aux_started) { hip_check(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0), "aux: fork wait"); aux_started = true; }
        st = ctx->stream2; partials = ctx->d_partials2; ctx->prof_stream = st;
        fn();
        st = s0; partials = p0; ctx->prof_stream = s0;
    }
    bool col_pending = false;
    template <typename Fn> void on_col(Fn fn) {   // the collation rounds on their own stream: behind the E tables, joined at the end of the prove
        hipStream_t s0 = st;
        E2* p0 = partials;
        hip_check(hipStreamWaitEvent(ctx->stream_col, ctx->ev_aux[2], 0), "collation: wait for the E tables");
        st = ctx->stream_col; partials = ctx->d_partials3; ctx->prof_stream = st;
        fn();
        hip_check(hipEventRecord(ctx->ev_col, ctx->stream_col), "collation: done event");
        st = s0; partials = p0; ctx->prof_stream = s0;
        col_pending = true;
    }
    std::function<void()> st_before_gp;  // flush_stride runs it once before the first grand-product launch (cross-stream wait)
    std::function<void()> st_before_gp2; // ... and this one once the sequenced first rounds of grand product #1's top layers are out
    // The node reductions on the THIRD stream (the collation rounds' - a few launches at the start of the prove): they then start with
    // the prove instead of behind the Lasso node's second-stream work (counters, grand product #2's tree, opening tables: 0.6 ms),
    // into the idle capacity those latency-bound launches leave.
    bool nodes_on_col = false, counters_event_live = false;   // (the second: ev_aux[3] was recorded by this prove's Lasso node)
    void fork_nodes_stream() {
        if (!fork_recorded) return;
        hip_check(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0), "fork wait");
        if (world == 1 && late_aux.empty()) {
            hip_check(hipStreamWaitEvent(ctx->stream_col, ctx->ev_fork, 0), "fork wait");
            // (behind the counters of the second stream: the first hash round waits for those, and the node reductions' first launches
            // beside them only stretch that wait - 1.79 against 1.81 ms)
            if (counters_event_live) hip_check(hipStreamWaitEvent(ctx->stream_col, ctx->ev_aux[3], 0), "node reductions: wait for the counters");
            st = ctx->stream_col; partials = ctx->d_partials3; ctx->prof_stream = st; forked = true; nodes_on_col = true;
            return;
        }
        st = ctx->stream2; partials = ctx->d_partials2; ctx->prof_stream = st; forked = true;
    }
    void join_sum_stream() {   // the split rounds' sums (flush_stride, mode 2) back into the main stream
        if (ctx->sum_pending) { hip_check(hipStreamWaitEvent(ctx->stream, ctx->ev_sum[1], 0), "split rounds: join wait"); ctx->sum_pending = false; }
    }
    void join_nodes_stream() {
        join_sum_stream();
        if (nodes_on_col) { hip_check(hipEventRecord(ctx->ev_col, ctx->stream_col), "node reductions: done event"); col_pending = true; nodes_on_col = false; }
        if (col_pending) { hip_check(hipStreamWaitEvent(ctx->stream, ctx->ev_col, 0), "collation: join wait"); col_pending = false; }
        if (!forked) return;
        hip_check(hipEventRecord(ctx->ev_join, ctx->stream2), "join event");
        st = ctx->stream; partials = ctx->d_partials; ctx->prof_stream = st;
        hip_check(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0), "join wait");
    }
    void gkr(const ClaimRef& sum_claim) {  // prove_gkr (sk_encryption_circuit.rs:455-457)
        const HCircuit& c = pk->circuit;
        claims.assign(c.nodes.size(), {});
        claims[c.lasso_id].push_back(ClaimRef{epos(), 0, cell()});  // EvalClaim::new(vec![], E::ZERO) (:450)
        claims[c.sum_id].push_back(sum_claim);
        record_fork();
        // nodes whose claims descend from the Lasso node (the node itself and, transitively, its predecessors): their transcript steps
        // wait for the Lasso node's results; every other node's steps can be replayed as soon as the node reductions are done
        std::vector<char> lasso_cone(c.nodes.size(), 0);
        {
            std::vector<int> stack{c.lasso_id};
            lasso_cone[c.lasso_id] = 1;
            while (!stack.empty()) {
                const int u = stack.back(); stack.pop_back();
                for (int pr : c.nodes[u].preds) if (!lasso_cone[pr]) { lasso_cone[pr] = 1; stack.push_back(pr); }
            }
        }
        const bool early_ok = world == 1 && fork_recorded && early_replay_on();
        for (size_t q = c.topo.size(); q-- > 0;) {
            int id = c.topo[q];
            const HNode& n = c.nodes[id];
            cur_early = early_ok && !lasso_cone[id];
            switch (n.kind) {
                case NK_INPUT: break;
                case NK_VANILLA: vanilla_node(id); break;
                case NK_FFT: fft_node(id); break;
                case NK_LASSO: {
                    ClaimRef cr = lasso_node(d_vals[n.preds[0]]);
                    claims[n.preds[0]].push_back(cr);
                    break;
                }
            }
        }
        cur_early = false;
        // The Vanilla / FFT node reductions go to the second stream: they are independent of the Lasso node on the
        // device and consist mostly of small launches that leave CUs idle, so the two streams overlap.
        fork_nodes_stream();
        stamp("node reductions begin");
        flush_bookkeeping();                   // eq tables, constant sums, Libra gathers, DFT-row tables: batched
        stamp("node bookkeeping done");
        flush_prodsum();                       // first wave: every FFT / Libra phase-1 reduction, batched
        stamp("node phase 1 done");

        for (auto& f : second_wave) f();       // Libra phase-2 bookkeeping (needs the phase-1 scalars in HBM)
        second_wave.clear();
        flush_bookkeeping();
        flush_prodsum();
        stamp("node reductions done");
        if (early_ok) {   // every result an early transcript step reads is in the buffer: tell the host (out-of-order replay, see `ops`)
            early_slot = slot(1);
            dev::set_e2(st, d_res() + early_slot, e2(1, 0));
        }
        join_side_streams();
    }
    // The end of a forked walk: what the Lasso node left for the node reductions' stream (its openings), then every side stream
    // joined to the main one. gkr() ends with it, and so do the kernel-level entries (prove_lasso_node, sumcheck_on_tables,
    // grand_product_on_tables), which record the fork as gkr() does and so build the launch plan a prove builds.
    void join_side_streams() {
        for (auto& f : late_aux) f();          // the Lasso node's openings (lasso_node)
        late_aux.clear();
        if (!late_col.empty()) {
            if (st != ctx->stream2) hip_check(hipStreamWaitEvent(st, ctx->ev_aux[4], 0), "openings: wait for the opening tables");
            for (auto& f : late_col) f();
            late_col.clear();
        }
        join_nodes_stream();
    }

