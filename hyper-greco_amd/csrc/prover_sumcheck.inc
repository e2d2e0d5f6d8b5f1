// Part of struct Prover (prover.hip includes this file inside the class body): the sum-check drivers - stride-layout jobs (collation, grand-product layers) and PRODSUM jobs (Libra / zkCNN node reductions, eq-factored or with tables), their round-synchronised launch plans (stride jobs: plan_stride() lists every launch with its items, grid, class and credit, flush_stride() uploads and issues that list; PRODSUM jobs: flush_prodsum(), plan then issue in one function), descriptor uploads, the transcript side of a sum-check - and the batched bookkeeping kernels (eq tables, DFT rows, Libra gathers).

    // ---- sum-check drivers ---------------------------------------------------------------------
    // A sum-check whose remaining work is this small ((table pairs) x (pairs per table) items) finishes all
    // remaining rounds in one single-workgroup launch; anything larger is ALU-bound on a single CU.
    static constexpr size_t TAIL_ITEMS = 4096;   // (the first tail round of such a job does not fit the LDS regions and goes through HBM: still faster than one more launch, 2.93 vs 2.98 ms)

    // Stride-layout sum-checks (collation, every grand-product layer) are queued as jobs and executed by
    // flush_stride() in a round-synchronised schedule (launch k = every job's next round(s)): they are independent on the device.
    // flush_stride() = plan_stride(), which turns the queue into the list of launches and touches no device, stream or profile, then
    // one loop that issues that list entry by entry.
    bool hash_recomp = false;   // the queued hash-source job recomputes its E values (lasso_node: lean form)
    // (the types of the queue and of the plan - StQueued, StrideOpts, StLaunch, StridePlan - are in prover.hip, beside SlotPlan)
    std::vector<StQueued> st_queue;
    std::vector<std::function<void()>> st_after_seq;   // the remaining (small) tree levels, behind the sequenced first rounds (StQueued::seq)
    double hash_design_reads = 0, hash_model_extra = 0;   // lasso_node -> grand_product: StrideArgs::hash_reads / fused_model_extra of the hash-source job
    std::vector<dev::ScatterEnt> scatter;  // locally produced scalars -> global result slots (batch-subset grand products)
    // claim epilogues of the queued grand-product jobs (grand_product, prover_lasso.inc): challenge-only constants, filled during the
    // walk and uploaded with the job descriptors, which a cached launch graph does not repeat
    struct GpEpReq { int job = -1; dev::GpClaimEp ep; std::vector<E2> winv, gnext; };
    std::vector<GpEpReq> gp_eps;

    ScHandle sc_stride(int kind, const void* in, bool base, size_t in_stride, int ntab, int nvars, const dev::Powers& pw, E2* final_out,
                       const StrideArgs& a = StrideArgs()) {
        ScHandle h;
        h.nv = kind == dev::SC_GRANDPROD ? 3 : 2;
        h.nvars = nvars;
        h.point_off = epos();
        h.sums_slot = slot((size_t)nvars * h.nv);
        const size_t N = (size_t)1 << nvars;
        if (!a.enqueue) {  // another rank runs this job: transcript bookkeeping only
            for (int i = 0; i < nvars; i++) h.rs.push_back(squeeze());
            return h;
        }
        dev::StJob J;
        memset(&J, 0, sizeof(J));
        J.in = in; J.in_stride = in_stride;
        J.buf[0] = ctx->alloc_n<E2>((size_t)ntab * std::max<size_t>(N / 2, 1));
        J.buf[1] = ctx->alloc_n<E2>((size_t)ntab * std::max<size_t>(N / 4, 1));
        J.final_out = final_out ? final_out : ctx->alloc_n<E2>(ntab);
        J.kind = kind; J.ntab = ntab; J.nvars = nvars; J.base = base ? 1 : 0; J.p0_only = a.p0_only ? 1 : 0;
        J.r_off = h.point_off; J.sums_slot = h.sums_slot;
        J.next_level = a.next_level; J.hash_src = a.hash_src;
        if (a.mirror) { J.mirror = 1; J.mk1 = a.mirror->k1; J.mk2 = a.mirror->k2; }
        if (a.slots && a.slots->job_slotw) { J.slotw = a.slots->job_slotw; J.emit_mask = a.slots->job_emit; J.slot_ng = a.slots->npairs; J.slot_shift = a.slots->max_rd; }
        memcpy(J.pw, pw.v, sizeof(J.pw));
        for (int i = 0; i < nvars; i++) h.rs.push_back(squeeze());
        if (nvars > 0)  // weight * r_0: the first round stores the weighted fold (kernels.hip)
            for (int i = 0; i < dev::PW_MAX; i++) J.pwr[i] = e2_mul(pw.v[i], h.rs[0]);
        if (nvars > 0) {
            const int credit_ntab = a.mirror ? a.mirror->credit_ntab : (a.model_ntab ? a.model_ntab : ntab);
            // a level-writing first round replaces prod_level on its input level: (nb rows of 2N entries) x 8 B x 1.5 (read +
            // write), as prod_level is credited; the hash-source job's level 1 is credited with its write only, as the hash kernel
            // it replaces was (round-1 accounting: the totals stay comparable)
            const double fused = a.next_level ? (double)(credit_ntab / 2) * (double)(2 * N) * 8.0 * (a.hash_src ? 0.5 : 1.5) : 0.0;
            st_queue.push_back(StQueued{J, a.seq, a.slots ? *a.slots : SlotPlan(), credit_ntab, fused + a.fused_bytes, a.fused_model_extra,
                                        a.next_level ? a.level_design : 0.0, a.hash_src ? a.hash_reads : -1.0});
        }
        return h;
    }

    // half-length (log2) at which a slot-form job's tail starts: what its PER-MEMORY tables allow (HG_TAIL_H does not apply)
    static int slot_tail_h(int tail_ntab, int nvars) { return std::min(dev::st_tail_h(tail_ntab, nvars), nvars - 2); }
    // ---- the plan of a flush: what is launched, in issue order ---------------------------------------------------------------------
    // The switches of a plan are read here and nowhere else: HG_NO_SPLIT once per process, the others at every flush (the tests
    // switch them per case).
    StrideOpts stride_opts() const {
        static const bool no_split = hg_env_on("HG_NO_SPLIT");
        StrideOpts o;
        o.may_split = !no_split && st == ctx->stream && fork_recorded && world == 1;
        o.sums_single = hg_env_on("HG_SUMS_SINGLE");
        o.fold_per_round = hg_env_on("HG_FOLD_ROUNDS");
        o.fold_tile_log2 = dev::ST_FOLD_TILE_LOG2;
        if (const char* e = getenv("HG_FOLD_TILE_LOG2")) { const int v = atoi(e); if (v >= 1 && v <= dev::ST_FOLD_TILE_MAX_LOG2) o.fold_tile_log2 = v; }
        o.tail_whole_rounds = hg_env_on("HG_TAIL_WHOLE_ROUNDS");
        return o;
    }
    // Plans a flush: (kind, base? | fused pair?, h_log2 | tail) -> items (job, where the round reads and writes). Folded tables
    // ping-pong between the job's two buffers; the plan tracks where each job's live tables are. No device, stream or profile call:
    // `alloc_e2` hands out the arena buffers of split rounds' folds and slot-form tails.
    StridePlan plan_stride(const std::vector<StQueued>& Q, const StrideOpts& o, const std::function<E2*(size_t)>& alloc_e2) const {
        constexpr int fuse_min_h = 15;   // fused pairs of rounds from half = 2^15 up (13 until the slot form: 1.96-1.99 against 1.99-2.01 ms; round 5: 13 / 11 / 9 = 1.864 / 1.905 / 1.980 against 1.831)
        constexpr int split_h = 14;      // split rounds from half = 2^14 down (every single-round launch of Ext2 tables: pairs of rounds are fused from 2^15 up; 12 / 10 measured the same)
        StridePlan P;
        const int nj = (int)Q.size();
        for (const StQueued& q : Q) P.jobs.push_back(q.J);
        const std::vector<dev::StJob>& jobs = P.jobs;
        std::vector<const void*> cur_in(nj);
        std::vector<size_t> cur_stride(nj);
        std::vector<int> next_h(nj);  // half-length (log2) of the job's next unscheduled round
        for (int q = 0; q < nj; q++) { cur_in[q] = jobs[q].in; cur_stride[q] = jobs[q].in_stride; next_h[q] = jobs[q].nvars - 1; }
        auto next_out = [&](int q) { return cur_in[q] == (const void*)jobs[q].buf[0] ? jobs[q].buf[1] : jobs[q].buf[0]; };
        // the item of job q's next round (or fused pair of rounds), written to `out`; the job moves on
        auto take = [&](int q, E2* out, int nrounds) {
            dev::StItem it;
            memset(&it, 0, sizeof(it));
            it.job = q; it.h_log2 = next_h[q]; it.in = cur_in[q]; it.in_stride = cur_stride[q]; it.out = out;
            cur_in[q] = out; cur_stride[q] = (size_t)1 << (it.h_log2 - (nrounds - 1)); next_h[q] -= nrounds;
            return it;
        };
        // The rounds with half <= 2^h_small[q] of job q run in ONE single-workgroup launch with the folded tables in LDS (st_tail);
        // how many fit depends on the job's table count (12 rounds for the two collation tables, 6 for a full grand-product layer).
        std::vector<int> h_small(nj);
        for (int q = 0; q < nj; q++) {
            const SlotPlan& sp = Q[q].slot;
            h_small[q] = sp.tail_ntab ? slot_tail_h(sp.tail_ntab, jobs[q].nvars) : dev::st_tail_h(jobs[q].ntab, jobs[q].nvars);
            if (Q[q].seq > 0) h_small[q] = std::min(h_small[q], jobs[q].nvars - 2);   // a sequenced first round has its own kernel
            if (sp.tail_ntab && jobs[q].nvars - 1 - h_small[q] > sp.max_rd) throw Error("slot-form job: the tail starts below the segment pairs");
        }
        // algorithmic bytes of one round of job q (SURVEY.md 8(d)): every live table read once, every folded table written once.
        // model = true: the tables of the reference's batch (a mirrored grand product is modelled with its read AND write tables, the
        // collation sum-check with its alpha tables), false: the tables this implementation streams
        auto round_bytes = [&](int q, int rd, bool model) {
            const dev::StJob& J = jobs[q];
            size_t half = (size_t)1 << (J.nvars - 1 - rd);
            return (double)(model ? Q[q].credit_ntab : J.ntab) * (2.0 * half * ((J.base && rd == 0) ? 8 : 16) + half * 16.0);
        };
        // bytes moved to or from HBM by design (hg_kernel_stat::hbm_bytes): `ntab` tables of round rd read once; the folds of half 2^h written once
        auto reads = [&](int q, int rd, int ntab) { return (double)ntab * 2.0 * (double)((size_t)1 << (jobs[q].nvars - 1 - rd)) * ((jobs[q].base && rd == 0) ? 8 : 16); };
        auto writes = [&](int q, int h) { return (double)jobs[q].ntab * (double)((size_t)1 << h) * 16.0; };
        // a launch of rounds rd .. rd + nrounds - 1: the tables of round rd read (the hash-source job's first round: its integer tables
        // instead), the folds of the last round written, plus the tree level a first round emits
        auto design_bytes = [&](int q, int rd, int nrounds) {
            double b = reads(q, rd, jobs[q].ntab);
            if (rd == 0 && Q[q].hash_reads >= 0) b = Q[q].hash_reads;
            b += writes(q, jobs[q].nvars - 1 - rd - (nrounds - 1));
            if (rd == 0) b += Q[q].level_design;
            return b;
        };
        auto line = [&](int kind, bool base, int nrounds, int mode, bool tail, bool hash, const std::vector<dev::StItem>& its) {
            StLine l{kind, base, nrounds, mode, tail, hash, 0, its.size(), INT_MAX, INT_MIN};
            for (const dev::StItem& it : its) { const int v = tail ? it.nrounds : it.h_log2; l.lo = std::min(l.lo, v); l.hi = std::max(l.hi, v); }
            P.lines.push_back(l);
        };
        auto launch = [](StLaunch::Tag tag, int kind) { StLaunch L; memset(&L, 0, sizeof(L)); L.tag = tag; L.kind = kind; return L; };
        // The launches of one round group: `its` cut at the batch size, each piece with its grid, class and credit - per round, as
        // SURVEY.md 8(d) accounts: a fused launch is credited with both of its rounds although the intermediate folded tables never
        // reach HBM (DESIGN.md 6), a base first round also with the passes it absorbs (the tree level it writes, the hash build).
        // The sums are credited with nothing: their rounds' bytes are the folds'. launched = false: the items only, as a record.
        auto emit = [&](StLaunch::Tag tag, int kind, bool base, int nrounds, int mode, std::vector<dev::StItem>& its, bool launched = true) {
            const size_t batch = tag == StLaunch::Sums && mode == 0 ? (size_t)dev::ST_SUMS_MAX_ITEMS : MAX_BATCH;
            for (size_t at = 0; at < its.size(); at += batch) {
                StLaunch L = launch(tag, kind);
                L.off = P.items.size() + at; L.cnt = (int)std::min<size_t>(batch, its.size() - at);
                L.grid = dev::st_plan_blocks(its.data() + at, L.cnt, nrounds == 2);
                L.base = base; L.mode = mode; L.slot = base && jobs[its[at].job].slotw != nullptr;
                L.cls = tag == StLaunch::Sums ? cls_gp_sums : kind == dev::SC_GRANDPROD ? (base ? cls_gp_base : (nrounds == 2 ? cls_gp_ext2 : cls_gp_ext)) : (base ? cls_col_base : (nrounds == 2 ? cls_col_ext2 : cls_col_ext));
                L.side = tag == StLaunch::Sums; L.first = at == 0; L.last = at + batch >= its.size();
                for (int k = 0; k < L.cnt; k++) {
                    const dev::StItem& it = its[at + k];
                    const int q = it.job, rd = jobs[q].nvars - 1 - it.h_log2;
                    L.design += design_bytes(q, rd, nrounds);
                    if (tag == StLaunch::Sums) continue;
                    for (int r = 0; r < nrounds; r++) { L.bytes += round_bytes(q, rd + r, false); L.model += round_bytes(q, rd + r, true); }
                    if (base && rd == 0) { L.bytes += Q[q].fused_bytes; L.model += Q[q].fused_bytes; }
                }
                if (launched) P.launches.push_back(L);
            }
            P.items.insert(P.items.end(), its.begin(), its.end());
        };
        for (int kind : {dev::SC_COLLATION, dev::SC_GRANDPROD}) {
            int max_h = -1;
            for (auto& J : jobs) if (J.kind == kind) max_h = std::max(max_h, J.nvars - 1);
            if (max_h < 0) continue;
            // sequenced first rounds (each produces the tree level the next one reads), then the remaining tree levels
            if (kind == dev::SC_GRANDPROD) {
                int max_seq = 0;
                for (int q = 0; q < nj; q++) max_seq = std::max(max_seq, Q[q].seq);
                for (int sq = 1; sq <= max_seq; sq++)
                    for (int q = 0; q < nj; q++) {
                        const dev::StJob& J = jobs[q];
                        if (Q[q].seq != sq || J.kind != kind) continue;
                        if (!J.base || next_h[q] <= h_small[q]) throw Error("sequenced first round on a job that has none");
                        std::vector<dev::StItem> one{take(q, J.buf[0], 1)};
                        line(kind, true, 1, 0, false, J.hash_src != nullptr, one);
                        emit(StLaunch::SeqFirst, kind, true, 1, 0, one);
                        if (J.hash_src) {   // ... and what only the reference's traffic model counts of the hash build (E reads)
                            StLaunch& L = P.launches.back();
                            L.hash = true; L.cls = cls_gp_hash; L.model += Q[q].fused_model_extra;
                        }
                    }
                if (max_seq > 0 || !st_after_seq.empty()) {
                    P.lines.push_back(StLine{kind, 0, 0, 0, 0, 0, 1, 0, 0, 0});
                    P.launches.push_back(launch(StLaunch::AfterSeq, kind));
                }
            }
            // the first rounds on base-field rows only read finished tree levels / node tables: one launch for all of them
            {
                std::vector<dev::StItem> all;
                for (int q = 0; q < nj; q++) {
                    const dev::StJob& J = jobs[q];
                    if (J.kind != kind || !J.base || next_h[q] <= h_small[q] || next_h[q] != J.nvars - 1) continue;  // (sequenced jobs are past their first round)
                    all.push_back(take(q, J.buf[0], 1));
                }
                if (!all.empty()) { line(kind, true, 1, 0, false, false, all); emit(StLaunch::First, kind, true, 1, 0, all); }
            }
            // then round-synchronised: launch k runs every job's next round (or, grand product with a long enough table,
            // its next TWO rounds) whatever the sizes; the jobs only depend on their own previous launch
            // Small grand-product rounds are split (round 6): a launch whose items all have half <= 2^split_h runs the FOLDS only, into
            // buffers of the round's own (so that its input outlives the rounds after it); the sums of all such rounds follow in
            // launches of their own on a side stream, beside the remaining fold-only rounds' successor - the tail. HG_NO_SPLIT=1: whole rounds.
            const bool may_split = kind == dev::SC_GRANDPROD && o.may_split;
            std::vector<dev::StItem> split;              // the fold-only rounds' items, in fold order
            std::vector<std::vector<dev::StItem>> runs(nj);   // ... by job
            size_t fold_at = 0;                          // launches ahead of the fold-run launches: all that were planned ahead of the LAST fold-only round
            for (;;) {
                std::vector<dev::StItem> le, l2;
                bool le_small = may_split;
                for (int q = 0; q < nj; q++) {
                    const dev::StJob& J = jobs[q];
                    const int h = next_h[q];
                    if (J.kind != kind || h <= h_small[q]) continue;
                    const bool first = J.nvars - 1 == h;
                    if (first && J.hash_src) throw Error("hash-source job without a sequenced first round");
                    // (fusing the SMALL rounds as well - pairs from 2^12 / 2^11 / 2^10 down - to save launches: 2.10 / 2.19 / 2.22 against 1.79 ms:
                    // the fused kernel walks a job's tables serially per thread and has too few workgroups there; with the table pairs split
                    // over thread groups as the single rounds are, pairs from 2^13 / 2^11 / 2^9: 1.663 / 1.694 / 1.759 against 1.670 - those
                    // rounds are bound by the dependent chain inside a pass, not by the launches)
                    const bool pair = !first && h - 1 > h_small[q] && h >= std::max(dev::ST_STEP2_MIN_H, fuse_min_h);
                    if (!pair && (first || h > split_h)) le_small = false;
                    (pair ? l2 : le).push_back(take(q, first ? J.buf[0] : next_out(q), pair ? 2 : 1));
                }
                if (le.empty() && l2.empty()) break;
                if (!l2.empty()) { line(kind, false, 2, 0, false, false, l2); emit(StLaunch::Step2, kind, false, 2, 0, l2); }
                if (le.empty()) continue;
                if (le_small)
                    for (auto& it : le) {   // (the job already points at it.out: repoint both)
                        it.out = alloc_e2((size_t)jobs[it.job].ntab << it.h_log2);
                        cur_in[it.job] = it.out;
                        split.push_back(it);
                        runs[it.job].push_back(it);
                    }
                line(kind, false, 1, le_small ? 1 : 0, false, false, le);
                emit(StLaunch::Step, kind, false, 1, le_small ? 1 : 0, le, !le_small || o.fold_per_round);
                if (le_small) fold_at = P.launches.size();
            }
            // The fold-only rounds of one job are consecutive rounds, each reading what the one before it wrote: a run, issued as ONE item
            // of a fold-run launch (kernels.hpp: StFoldRun) where the LAST fold-only round stands - every run's input was written by a
            // launch planned ahead of its first fold-only round. A run longer than a tile holds is cut: piece c of every run shares launch c.
            if (!split.empty() && !o.fold_per_round) {
                std::vector<std::vector<dev::StFoldRun>> pieces;   // [c]: piece c of every run that has one
                for (int q = 0; q < nj; q++) {
                    const std::vector<dev::StItem>& run = runs[q];
                    for (size_t k = 1; k < run.size(); k++)
                        if (run[k].h_log2 != run[k - 1].h_log2 - 1 || run[k].in != (const void*)run[k - 1].out || run[k].in_stride != (size_t)1 << run[k - 1].h_log2)
                            throw Error("fold-only rounds of a job that do not follow each other");
                    P.fold_rounds += (int)run.size();
                    P.fold_max_run = std::max(P.fold_max_run, (int)run.size());
                    size_t c = 0;
                    for (size_t pos = 0; pos < run.size(); c++) {
                        dev::StFoldRun F;
                        memset(&F, 0, sizeof(F));
                        F.job = q; F.h0 = run[pos].h_log2; F.in = (const E2*)run[pos].in; F.in_stride = run[pos].in_stride;
                        F.nrounds = (int)std::min<size_t>((size_t)std::min(o.fold_tile_log2, F.h0) + 1, run.size() - pos);
                        for (int k = 0; k < F.nrounds; k++) F.out[k] = run[pos + k].out;
                        if (pieces.size() <= c) pieces.emplace_back();
                        pieces[c].push_back(F);
                        pos += (size_t)F.nrounds;
                    }
                }
                std::vector<StLaunch> fl;
                for (const auto& pc : pieces)
                    for (size_t at = 0; at < pc.size(); at += MAX_BATCH) {
                        StLaunch L = launch(StLaunch::FoldRuns, kind);
                        L.off = P.fold_runs.size(); L.cnt = (int)std::min<size_t>(MAX_BATCH, pc.size() - at);
                        P.fold_runs.insert(P.fold_runs.end(), pc.begin() + at, pc.begin() + at + L.cnt);
                        L.grid = dev::st_plan_fold_blocks(P.fold_runs.data() + L.off, L.cnt, jobs.data(), o.fold_tile_log2);
                        L.cls = cls_gp_ext;
                        for (int k = 0; k < L.cnt; k++) {   // credited round by round as the per-round launches are; by design: the first level read once, every level written once
                            const dev::StFoldRun& F = P.fold_runs[L.off + k];
                            const int rd = jobs[F.job].nvars - 1 - F.h0;
                            L.design += reads(F.job, rd, jobs[F.job].ntab);
                            for (int r = 0; r < F.nrounds; r++) {
                                L.bytes += round_bytes(F.job, rd + r, false); L.model += round_bytes(F.job, rd + r, true);
                                L.design += writes(F.job, F.h0 - r);
                            }
                        }
                        fl.push_back(L);
                    }
                P.launches.insert(P.launches.begin() + fold_at, fl.begin(), fl.end());
                P.fold_launches = (int)fl.size(); P.fold_tile_log2 = o.fold_tile_log2;
            }
            if (!split.empty()) {
                // Rounds (h, h - 1) of one job are summed from round h's input alone (the fused pass folds round h in registers): a third
                // of the reads less - for a job of few table pairs. The fused pass walks a job's pairs serially in every thread, and
                // with many pairs that chain, not the bytes, is what the launch waits for (kernels.hpp: ST_SUMS_PAIR_MAX_NB). A job's
                // rounds follow each other, largest first; a pair is ONE launched item, so none straddles two launches.
                line(kind, false, 1, 2, false, false, split);
                std::vector<dev::StItem> sums;   // what is launched for `split`: job-major, consecutive rounds of a job as one item (st_sums)
                if (!o.sums_single) {
                    std::stable_sort(split.begin(), split.end(), [](const dev::StItem& a, const dev::StItem& b) { return a.job < b.job; });
                    for (size_t k = 0; k < split.size(); k++) {
                        dev::StItem it = split[k];
                        if (k + 1 < split.size() && split[k + 1].job == it.job && split[k + 1].h_log2 == it.h_log2 - 1 && it.h_log2 >= dev::ST_STEP2_MIN_H &&
                            jobs[it.job].ntab / 2 <= dev::ST_SUMS_PAIR_MAX_NB) { it.nrounds = 2; k++; P.n_sum_pairs++; }
                        else P.n_sum_singles++;
                        sums.push_back(it);
                    }
                } else { sums = split; P.n_sum_singles += (int)split.size(); }
                emit(StLaunch::Sums, kind, false, 1, o.sums_single ? 2 : 0, sums);
            }
            // the tail launch: every job's remaining rounds. The grand-product tail folds first and sums once (kernels.hip: k_st_tail<.., FF>)
            const bool tail_ff = kind == dev::SC_GRANDPROD && !o.tail_whole_rounds;
            std::vector<dev::StItem> tail;
            for (int q = 0; q < nj; q++) {
                const dev::StJob& J = jobs[q];
                if (J.kind != kind || next_h[q] < 0) continue;
                const int hs = next_h[q];
                dev::StItem it;
                memset(&it, 0, sizeof(it));
                it.job = q; it.in = cur_in[q]; it.in_stride = cur_stride[q];
                it.rd = J.nvars - 1 - hs; it.nrounds = hs + 1; it.out = J.final_out;
                if (Q[q].slot.tail_ntab) {   // the tail reads the per-memory tables, gathered right before it is launched (Regroup) from cur_in[q]
                    if (cur_stride[q] != (size_t)2 << hs) throw Error("slot-form job: unexpected table length at the tail");
                    it.in = alloc_e2((size_t)Q[q].slot.tail_ntab << (hs + 1)); it.ntab = Q[q].slot.tail_ntab;
                }
                tail.push_back(it);
                next_h[q] = -1;
            }
            if (!tail.empty()) line(kind, false, 0, 0, true, false, tail);
            for (size_t at = 0; at < tail.size(); at += MAX_BATCH) {
                StLaunch R = launch(StLaunch::Regroup, kind), T = launch(StLaunch::Tail, kind);
                R.off = P.regroups.size();
                T.off = P.items.size() + at; T.cnt = (int)std::min<size_t>(MAX_BATCH, tail.size() - at);
                T.cls = cls_tail; T.fold_first = tail_ff;
                for (int k = 0; k < T.cnt; k++) {
                    const dev::StItem& it = tail[at + k];
                    const int h0 = jobs[it.job].nvars - 1 - it.rd, tn = it.ntab > 0 ? it.ntab : jobs[it.job].ntab;
                    for (int r = 0; r < it.nrounds; r++) { T.bytes += round_bytes(it.job, it.rd + r, false); T.model += round_bytes(it.job, it.rd + r, true); }
                    T.design += reads(it.job, it.rd, tn);   // (nothing written)
                    T.table_bytes = std::max(T.table_bytes, dev::st_tail_table_bytes(tn, h0, tail_ff));
                    if (tail_ff && it.nrounds > dev::st_tail_whole_rounds(tn, h0)) P.n_tail_ff++;   // (a tail of one or two whole rounds has nothing to fold first)
                    else if (kind == dev::SC_GRANDPROD) P.n_tail_whole++;
                    if (it.ntab > 0) {   // (a slot-form job: its tables are one round longer than the tail's first half, 2^(h0 + 1))
                        const SlotPlan& sp = Q[it.job].slot;
                        P.regroups.push_back(dev::gp_slot_regroup_job((const E2*)cur_in[it.job], (E2*)it.in, sp.d_slot_of, sp.d_ratio, sp.nrows, sp.nslots, sp.npairs, h0 + 1, (sp.tail_ntab & 1) != 0));
                        R.cnt++;
                        R.rg_max = std::max(R.rg_max, ((size_t)sp.nrows + (sp.tail_ntab & 1)) << (h0 + 1));
                    }
                }
                if (R.cnt) P.launches.push_back(R);
                P.launches.push_back(T);
            }
            P.items.insert(P.items.end(), tail.begin(), tail.end());
        }
        return P;
    }
    void print_stride_plan(const StridePlan& P) const {   // (the tokens are read at every call: the tests switch them per case)
        if (hg_debug("plan"))
            for (const StLine& l : P.lines) {
                if (l.after_seq) { fprintf(stderr, "[hg plan] stride kind=%d after_seq=1\n", l.kind); continue; }
                fprintf(stderr, "[hg plan] stride kind=%d base=%d nrounds=%d mode=%d tail=%d hash=%d items=%zu %s=%d..%d\n", l.kind, l.base, l.nrounds,
                        l.mode, l.tail, l.hash, l.items, l.tail ? "rounds" : "h", l.lo, l.hi);
            }
        if (hg_debug("endgame") && (P.n_tail_ff || P.n_tail_whole || P.n_sum_pairs || P.n_sum_singles))
            fprintf(stderr, "[hg endgame] stride tail_fold_first=%d tail_whole=%d sums_pairs=%d sums_singles=%d\n", P.n_tail_ff, P.n_tail_whole, P.n_sum_pairs, P.n_sum_singles);
        if (hg_debug("folds") && P.fold_launches)   // `rounds` = the items of the plan's mode=1 lines
            fprintf(stderr, "[hg folds] stride launches=%d items=%zu rounds=%d max_run=%d tile_log2=%d\n", P.fold_launches, P.fold_runs.size(), P.fold_rounds, P.fold_max_run, P.fold_tile_log2);
    }
    void flush_stride() {
        if (st_queue.empty()) return;
        const int nj = (int)st_queue.size();
        if (hoist_consts)   // (as in flush_prodsum: the rounds stay recorded)
            for (const StQueued& q : st_queue) {
                const size_t N = (size_t)1 << q.J.nvars;
                kept_writes(crange(q.J.buf[0], (size_t)q.J.ntab * std::max<size_t>(N / 2, 1)));
                kept_writes(crange(q.J.buf[1], (size_t)q.J.ntab * std::max<size_t>(N / 4, 1)));
                kept_writes(crange(q.J.final_out, (size_t)q.J.ntab));
            }
        StridePlan P = plan_stride(st_queue, stride_opts(), [this](size_t n) { return ctx->alloc_n<E2>(n); });
        print_stride_plan(P);
        if (!gp_eps.empty()) {   // the claim epilogues and their weight vectors: one upload each
            std::vector<E2> wts;
            std::vector<dev::GpClaimEp> eps;
            for (const GpEpReq& e : gp_eps) {
                if (e.job < 0 || e.job >= nj || P.jobs[e.job].kind != dev::SC_GRANDPROD) throw Error("grand product: claim epilogue without its job");
                wts.insert(wts.end(), e.winv.begin(), e.winv.end());
                wts.insert(wts.end(), e.gnext.begin(), e.gnext.end());
            }
            E2* d_wts = ctx->alloc_n<E2>(wts.size());
            dev::GpClaimEp* d_eps = ctx->alloc_n<dev::GpClaimEp>(gp_eps.size());
            size_t o = 0;
            for (size_t i = 0; i < gp_eps.size(); i++) {
                dev::GpClaimEp ep = gp_eps[i].ep;
                ep.winv = d_wts + o; o += gp_eps[i].winv.size();
                ep.gnext = d_wts + o; o += gp_eps[i].gnext.size();
                eps.push_back(ep);
                P.jobs[gp_eps[i].job].ep = d_eps + i;
            }
            upload(d_wts, wts.data(), wts.size() * sizeof(E2), "upload claim weights");
            upload(d_eps, eps.data(), eps.size() * sizeof(dev::GpClaimEp), "upload claim epilogues");
            gp_eps.clear();
        }
        dev::StJob* d_jobs = ctx->alloc_n<dev::StJob>(nj);
        upload(d_jobs, P.jobs.data(), (size_t)nj * sizeof(dev::StJob), "upload jobs");
        dev::StItem* d_items = ctx->alloc_n<dev::StItem>(P.items.size());
        upload(d_items, P.items.data(), P.items.size() * sizeof(dev::StItem), "upload step items");
        dev::StFoldRun* d_fold = nullptr;
        if (!P.fold_runs.empty()) {
            d_fold = ctx->alloc_n<dev::StFoldRun>(P.fold_runs.size());
            upload(d_fold, P.fold_runs.data(), P.fold_runs.size() * sizeof(dev::StFoldRun), "upload fold runs");
        }
        for (const StLaunch& L : P.launches) {
            if (L.kind == dev::SC_GRANDPROD && st_before_gp) { stamp("collation done"); st_before_gp(); st_before_gp = nullptr; stamp("grand products may start"); }
            hipStream_t s = L.side ? ctx->stream_sum : st;
            E2* part = L.side ? ctx->d_partials4 : partials;
            switch (L.tag) {
            case StLaunch::AfterSeq:
                for (auto& f : st_after_seq) f();
                st_after_seq.clear();
                if (st_before_gp2) { st_before_gp2(); st_before_gp2 = nullptr; }   // the launches from here on contain grand product #2's jobs
                break;
            case StLaunch::SeqFirst: case StLaunch::First: case StLaunch::Step:
                ctx->prof_begin(L.cls, L.bytes, L.model, L.design);
                if (L.hash) {
                    const int q = P.items[L.off].job;
                    dev::st_first_hash(s, d_jobs + q, d_items + L.off, L.grid, P.jobs[q].mirror != 0, hash_recomp, ctx->d_chal, part, d_res(), st_queue[q].slot.tail_ntab != 0);
                } else dev::st_step(s, L.kind, L.base, d_jobs, d_items + L.off, L.cnt, L.grid, ctx->d_chal, part, d_res(), L.slot, L.mode);
                ctx->prof_end();
                if (L.hash) stamp("first hash round done");
                break;
            case StLaunch::Step2:
                ctx->prof_begin(L.cls, L.bytes, L.model, L.design);
                dev::st_step2(s, L.kind, d_jobs, d_items + L.off, L.cnt, L.grid, ctx->d_chal, part, d_res());
                ctx->prof_end();
                break;
            case StLaunch::FoldRuns:
                ctx->prof_begin(L.cls, L.bytes, L.model, L.design);
                dev::st_fold_runs(s, d_jobs, d_fold + L.off, L.cnt, L.grid, ctx->d_chal);
                ctx->prof_end();
                break;
            case StLaunch::Sums:   // beside whatever the main stream does next, joined at the end of the prove
                if (L.first) {
                    hip_check(hipEventRecord(ctx->ev_sum[0], st), "split rounds: folds done");
                    hip_check(hipStreamWaitEvent(s, ctx->ev_sum[0], 0), "split rounds: wait for the folds");
                }
                ctx->prof_stream = s;
                ctx->prof_begin(L.cls, L.bytes, L.model, L.design);
                if (L.mode == 0) dev::st_sums(s, d_jobs, d_items + L.off, L.cnt, L.grid, ctx->d_chal, part, d_res());
                else dev::st_step(s, L.kind, false, d_jobs, d_items + L.off, L.cnt, L.grid, ctx->d_chal, part, d_res(), false, L.mode);
                ctx->prof_end();
                ctx->prof_stream = st;
                if (L.last) {
                    hip_check(hipEventRecord(ctx->ev_sum[1], s), "split rounds: sums done");
                    ctx->sum_pending = true;
                }
                break;
            case StLaunch::Regroup: {
                dev::SlotRegroupJob* d_rg = ctx->alloc_n<dev::SlotRegroupJob>(L.cnt);
                upload(d_rg, P.regroups.data() + L.off, (size_t)L.cnt * sizeof(dev::SlotRegroupJob), "upload regroup jobs");
                dev::gp_slot_regroup_jobs(s, d_rg, L.cnt, L.rg_max);
                break;
            }
            case StLaunch::Tail:
                ctx->prof_begin(L.cls, L.bytes, L.model, L.design);
                dev::st_tail(s, L.kind, d_jobs, d_items + L.off, L.cnt, L.table_bytes, ctx->d_chal, d_res(), L.fold_first);
                ctx->prof_end();
                break;
            }
        }
        if (st_before_gp) { st_before_gp(); st_before_gp = nullptr; }
        if (st_before_gp2) { st_before_gp2(); st_before_gp2 = nullptr; }
        st_queue.clear();
        for (auto& f : st_after_seq) f();  // (no grand-product job was queued: nothing can depend on these, but keep the order)
        st_after_seq.clear();
        if (!scatter.empty()) {
            dev::ScatterEnt* d = ctx->alloc_n<dev::ScatterEnt>(scatter.size());
            upload(d, scatter.data(), scatter.size() * sizeof(dev::ScatterEnt), "upload scatter list");
            dev::scatter_e2(st, d, scatter.size(), d_res());
            scatter.clear();
        }
    }

    // PRODSUM instances are queued and executed in batches of equal nvars (grid.y = instance): the node
    // reductions have no device-side dependencies on each other, only the transcript order matters.
    std::map<int, std::vector<dev::PsJob>> ps_queue;
    std::vector<std::function<void()>> second_wave;  // device work that needs first-wave results (Libra phase 2)

    ScHandle sc_prodsum(const std::vector<const u64*>& a, const std::vector<const E2*>& b, int nvars,
                        const std::vector<E2*>& fin_a, const std::vector<E2*>& fin_b, bool enqueue = true) {
        ScHandle h;
        h.nv = 2;
        h.nvars = nvars;
        h.point_off = epos();
        h.sums_slot = slot((size_t)nvars * 2);
        if (!enqueue) {
            for (int i = 0; i < nvars; i++) h.rs.push_back(squeeze());
            return h;
        }
        const int np = (int)a.size();
        if (np > dev::PS_MAX_PAIRS) throw Error("prodsum: too many table pairs");
        const size_t N = (size_t)1 << nvars;
        dev::PsJob J;
        memset(&J, 0, sizeof(J));
        J.npairs = np; J.nvars = nvars; J.r_off = h.point_off; J.sums_slot = h.sums_slot;
        for (int q = 0; q < 2; q++) {
            J.bufa[q] = ctx->alloc_n<E2>((size_t)np * std::max<size_t>(N >> (q + 1), 1));
            J.bufb[q] = ctx->alloc_n<E2>((size_t)np * std::max<size_t>(N >> (q + 1), 1));
        }
        for (int i = 0; i < np; i++) { J.a[i] = a[i]; J.b[i] = b[i]; J.fin_a[i] = fin_a[i]; J.fin_b[i] = fin_b[i]; }
        for (int i = 0; i < nvars; i++) h.rs.push_back(squeeze());
        ps_queue[nvars].push_back(J);
        return h;
    }
    // ---- eq-factored PRODSUM jobs (kernels.hpp PsJob::eq_n) ---------------------------------------------------------------
    // HG_NO_PS_EQ=1: every Libra table materialised (the general form, which small or non-affine nodes take anyway)
    static bool ps_eq_on() { static const bool v = !hg_env_on("HG_NO_PS_EQ"); return v; }
    static size_t ps_tail_items() { return std::min<size_t>(TAIL_ITEMS, dev::ps_tail_items_max()); }   // (the tail keeps a job's folds in LDS)
    // first round whose work fits the tail
    static int ps_tail_rd(int npairs, int nvars) {
        const size_t N = (size_t)1 << nvars;
        int rd = 0;
        while (rd < nvars && ((N >> rd) / 2) * (size_t)npairs > ps_tail_items()) rd++;
        return rd;
    }
    // First tail round of an eq-factored job, -1: the job is too small for the form. Every round ahead of the tail runs in a fused
    // pair (the tail may start one round later than TAIL_ITEMS says), the last pair at half >= 2^9, and the table handed to the
    // tail must be one of the point's stored suffix tables.
    static int eq_tail_rd(int npairs, int nvars) {
        if (npairs < 1 || npairs > dev::PS_MAX_PAIRS || nvars > dev::PS_EQ_MAX_VARS) return -1;
        int rd = ps_tail_rd(npairs, nvars);
        if (rd & 1) rd++;
        if (rd < 2 || rd > nvars - 8 || rd < dev::ps_eq_kmin(nvars)) return -1;
        return rd;
    }
    std::vector<E2> eq_scal_host;   // prefactors / kappa of the queued eq-factored jobs (PsJob::eq_scal), one upload per flush
    std::vector<dev::PsEqPoint> eqpt_queue;
    std::map<std::tuple<size_t, int, int, unsigned>, std::pair<E2*, E2*>> eqpt_shared;   // (point, w, nvars, hib) -> the point's (lo, suf) tables
    // g = sum_i a_i(x) kappa_i eq(z', x): zp = z' (host copy of the coordinates), the first w of them the chain run at z_off
    ScHandle sc_prodsum_eq(const std::vector<const u64*>& a, const std::vector<E2>& kappa, const std::vector<E2>& zp, size_t z_off, int w, unsigned hib,
                           int nvars, int tail_rd, const std::vector<E2*>& fin_a, const std::vector<E2*>& fin_b, bool enqueue) {
        ScHandle h;
        h.nv = 2;
        h.nvars = nvars;
        h.point_off = epos();
        h.sums_slot = slot((size_t)nvars * 2);
        for (int i = 0; i < nvars; i++) h.rs.push_back(squeeze());
        if (!enqueue) return h;
        const int np = (int)a.size();
        const size_t N = (size_t)1 << nvars;
        dev::PsJob J;
        memset(&J, 0, sizeof(J));
        J.npairs = np; J.nvars = nvars; J.r_off = h.point_off; J.sums_slot = h.sums_slot;
        J.tail_rd = tail_rd; J.eq_n = np; J.eq_single = np == 1 ? 1 : 0;
        for (int q = 0; q < 2; q++) {
            J.bufa[q] = ctx->alloc_n<E2>((size_t)np * (N >> (q + 1)));
            if (np > 1) J.bufA[q] = ctx->alloc_n<E2>(N >> (q + 1));
        }
        if (np > 1) J.eqA0 = ctx->alloc_n<E2>(N);
        for (int i = 0; i < np; i++) { J.a[i] = a[i]; J.fin_a[i] = fin_a[i]; J.fin_b[i] = fin_b[i]; }
        // prefactors of the rounds ahead of the tail, P at the hand-off, kappa
        std::vector<E2> scal((size_t)2 * nvars + 1 + np + nvars + 4 * (size_t)(tail_rd / 2), e2_zero());
        E2 P = e2_one();
        for (int rd = 0; rd <= tail_rd && rd < nvars; rd++) {
            if (rd == tail_rd) { scal[(size_t)2 * nvars] = P; break; }
            const E2 z = zp[rd], omz = e2_sub(e2_one(), z);
            E2 p0 = e2_mul(P, omz), p2 = e2_mul(P, e2_sub(e2_add(e2_dbl(z), z), e2_one()));
            if (np == 1) { p0 = e2_mul(p0, kappa[0]); p2 = e2_mul(p2, kappa[0]); }
            scal[(size_t)2 * rd] = p0; scal[(size_t)2 * rd + 1] = p2;
            P = e2_mul(P, e2_add(e2_mul(z, h.rs[rd]), e2_mul(omz, e2_sub(e2_one(), h.rs[rd]))));
        }
        for (int i = 0; i < np; i++) scal[(size_t)2 * nvars + 1 + i] = kappa[i];
        for (int k = 0; k < nvars; k++) scal[(size_t)2 * nvars + 1 + np + k] = zp[k];
        for (int rd = 0; rd + 1 < tail_rd; rd += 2) {   // the four-term double fold of the pass at (rd, rd + 1): entry 4j + p, p = b0 + 2 b1
            const E2 ra = h.rs[rd], rb = h.rs[rd + 1], na = e2_sub(e2_one(), ra), nb = e2_sub(e2_one(), rb);
            E2* c = &scal[(size_t)2 * nvars + 1 + np + nvars + 4 * (size_t)(rd / 2)];
            c[0] = e2_mul(na, nb); c[1] = e2_mul(ra, nb); c[2] = e2_mul(na, rb); c[3] = e2_mul(ra, rb);
        }
        // (uploaded by flush_prodsum on the stream the rounds run on - this walk is still enqueueing to the main one; until then
        // eq_scal holds the job's offset into eq_scal_host)
        J.eq_scal = reinterpret_cast<const E2*>(eq_scal_host.size() * sizeof(E2));
        eq_scal_host.insert(eq_scal_host.end(), scal.begin(), scal.end());
        const auto key = std::make_tuple(z_off, w, nvars, hib);
        auto hit = eqpt_shared.find(key);
        if (hit == eqpt_shared.end()) {
            dev::PsEqPoint pt;
            memset(&pt, 0, sizeof(pt));
            pt.point_off = z_off; pt.w = w; pt.nvars = nvars; pt.hib = hib; pt.kmin = dev::ps_eq_kmin(nvars);
            pt.lo = ctx->alloc_n<E2>(dev::ps_eq_lo_entries(nvars));
            pt.suf = ctx->alloc_n<E2>(dev::ps_eq_suf_entries(nvars));
            eqpt_queue.push_back(pt);
            hit = eqpt_shared.emplace(key, std::make_pair(pt.lo, pt.suf)).first;
        }
        J.eq_lo = hit->second.first; J.eq_suf = hit->second.second;
        ps_queue[nvars].push_back(J);
        return h;
    }
    void flush_prodsum() {
        // round-synchronised: launch rd runs round rd of every queued job whatever its size; the last rounds of each
        // job (TAIL_ITEMS work items or fewer) run in one single-workgroup-per-job launch
        std::vector<dev::PsJob> jobs;
        for (auto& kv : ps_queue) { jobs.insert(jobs.end(), kv.second.begin(), kv.second.end()); kv.second.clear(); }
        if (jobs.empty()) return;
        const int nj = (int)jobs.size();
        if (hoist_consts)   // the rounds stay recorded: none of their fold buffers may be a table that was built once
            for (auto& J : jobs) {
                const size_t N = (size_t)1 << J.nvars;
                for (int q = 0; q < 2; q++) {
                    const size_t len = std::max<size_t>(N >> (q + 1), 1);
                    kept_writes(crange(J.bufa[q], (size_t)J.npairs * len));
                    kept_writes(crange(J.bufb[q], (size_t)J.npairs * len));
                    kept_writes(crange(J.bufA[q], len));
                }
                kept_writes(crange(J.eqA0, N));
            }
        if (hg_debug("eq")) {
            int ne = 0; size_t ee = 0, et = 0;
            for (auto& J : jobs) { const size_t e = (size_t)J.npairs << J.nvars; et += e; if (J.eq_n) { ne++; ee += e; } }
            fprintf(stderr, "[hg eq] %d of %d queued node reductions eq-factored, %zu of %zu table entries\n", ne, nj, ee, et);
        }
        if (!eq_scal_host.empty()) {
            E2* d_scal = ctx->alloc_n<E2>(eq_scal_host.size());
            upload(d_scal, eq_scal_host.data(), eq_scal_host.size() * sizeof(E2), "upload eq-form scalars");
            for (auto& J : jobs) if (J.eq_n) J.eq_scal = d_scal + reinterpret_cast<size_t>(J.eq_scal) / sizeof(E2);
            eq_scal_host.clear();
        }
        for (auto& J : jobs)
            if (!J.eq_n) J.tail_rd = ps_tail_rd(J.npairs, J.nvars);   // (an eq-factored job's was planned when it was queued: eq_tail_rd)
        auto round_bytes = [&](const dev::PsJob& J, int rd) {
            size_t half = ((size_t)1 << J.nvars) >> (rd + 1);
            if (J.eq_n && rd < J.tail_rd)   // no b tables; the folded A beside the a_i (formed in round 0, not read)
                return (double)J.npairs * (2.0 * half * (rd == 0 ? 8 : 16) + half * 16.0) + (J.eq_single ? 0.0 : (rd == 0 ? 0.0 : 2.0 * half * 16) + half * 16.0);
            return (double)J.npairs * (2.0 * half * ((rd == 0 ? 8 : 16) + 16) + half * 32.0);
        };
        // plan every step first (step s = every job's next round, or its next two rounds when its table is long
        // enough), upload all items in one copy, then launch; the host tracks each job's ping-pong buffer
        constexpr int ps_fuse_min_h = 9;   // fused pairs from half = 2^9 (11 until the node reductions moved to the third stream: 1.92-1.94 against 1.96 ms)
        // ... and in bytes moved to or from HBM by design: a pass reads its tables once and writes the folds of its LAST round
        auto design_bytes = [&](const dev::PsJob& J, int rd, int nrounds) {
            const size_t half = ((size_t)1 << J.nvars) >> (rd + 1), out = half >> (nrounds - 1);
            const double ea = rd == 0 ? 8 : 16;
            if (J.eq_n) return (double)J.npairs * (2.0 * half * ea + out * 16.0) + (J.eq_single ? 0.0 : 2.0 * half * 16.0 + out * 16.0);
            return (double)J.npairs * (2.0 * half * (ea + 16) + out * 32.0);
        };
        struct PsLaunch { bool two, eq; int cnt, grid; size_t off; double bytes, design; };
        std::vector<PsLaunch> launches;
        std::vector<dev::PsItem> all_items;
        std::vector<int> next_rd(nj, 0), cur_buf(nj, -1);
        for (;;) {
            std::vector<dev::PsItem> one, two, two_eq;   // (eq-factored jobs have a kernel of their own)
            for (int q = 0; q < nj; q++) {
                const dev::PsJob& J = jobs[q];
                const int rd = next_rd[q];
                if (rd >= J.tail_rd) continue;
                const int h = J.nvars - 1 - rd;
                const bool pair = J.eq_n ? true : rd + 1 < J.tail_rd && h >= std::max(9, ps_fuse_min_h);
                dev::PsItem it;
                memset(&it, 0, sizeof(it));
                it.job = q; it.rd = rd; it.in_buf = cur_buf[q]; it.out_buf = cur_buf[q] == 1 ? 0 : 1;
                if (cur_buf[q] < 0) it.out_buf = pair ? 1 : 0;  // sizes: bufa[0] holds N/2 entries per table, bufa[1] N/4
                if (J.eq_n && rd + 2 >= J.tail_rd) it.pad = 1;   // (PS_EQ_OUT_TAIL: this pass writes the layout the tail reads)
                (J.eq_n ? two_eq : pair ? two : one).push_back(it);
                next_rd[q] = rd + (pair ? 2 : 1);
                cur_buf[q] = it.out_buf;
            }
            if (one.empty() && two.empty() && two_eq.empty()) break;
            for (int kind = 0; kind < 3; kind++) {   // the eq-factored jobs first: the largest tables of the first wave
                std::vector<dev::PsItem>& items = kind == 0 ? two_eq : kind == 1 ? one : two;
                const bool fused = kind != 1;
                for (size_t o = 0; o < items.size(); o += MAX_BATCH) {
                    const int cnt = (int)std::min<size_t>(MAX_BATCH, items.size() - o);
                    const int grid = dev::ps_plan_blocks(items.data() + o, cnt, jobs.data(), fused);
                    double bytes = 0, design = 0;
                    for (int q = 0; q < cnt; q++) {
                        for (int k = 0; k <= (fused ? 1 : 0); k++) bytes += round_bytes(jobs[items[o + q].job], items[o + q].rd + k);
                        design += design_bytes(jobs[items[o + q].job], items[o + q].rd, fused ? 2 : 1);
                    }
                    launches.push_back({fused, kind == 0, cnt, grid, all_items.size(), bytes, design});
                    all_items.insert(all_items.end(), items.begin() + o, items.begin() + o + cnt);
                }
            }
        }
        for (int q = 0; q < nj; q++) jobs[q].tail_buf = cur_buf[q];
        if (hg_debug("plan")) {   // one line per launch, in launch order, then the tail's
            for (const PsLaunch& L : launches) {
                int lo = INT_MAX, hi = INT_MIN;
                std::string hs, gs, ws, ts;
                for (int q = 0; q < L.cnt; q++) {
                    const dev::PsItem& it = all_items[L.off + q];
                    lo = std::min(lo, it.rd); hi = std::max(hi, it.rd);
                    hs += (q ? "," : "") + std::to_string(jobs[it.job].nvars - 1 - it.rd);
                    if (L.eq) {
                        gs += (q ? "," : "") + std::to_string(it.jb_log2);
                        ws += (q ? "," : "") + std::to_string(it.nblk / it.jb_log2);
                        ts += (q ? "," : "") + std::to_string(it.pad);
                    }
                }
                // (an eq-factored launch also shows each item's table groups and the workgroups of one group: ps_plan_blocks)
                fprintf(stderr, "[hg plan] prodsum two=%d eq=%d cnt=%d rd=%d..%d h=[%s]%s\n", L.two ? 1 : 0, L.eq ? 1 : 0, L.cnt, lo, hi, hs.c_str(),
                        L.eq ? (" grp=[" + gs + "] wg=[" + ws + "] out_tail=[" + ts + "]").c_str() : "");
            }
            int lo = INT_MAX, hi = INT_MIN;
            for (auto& J : jobs) { lo = std::min(lo, J.tail_rd); hi = std::max(hi, J.tail_rd); }
            fprintf(stderr, "[hg plan] prodsum tail jobs=%d tail_rd=%d..%d\n", nj, lo, hi);
        }
        dev::PsJob* d_jobs = ctx->alloc_n<dev::PsJob>(nj);
        upload(d_jobs, jobs.data(), (size_t)nj * sizeof(dev::PsJob), "upload jobs");
        {   // A = sum_i kappa_i a_i of the eq-factored jobs with several tables
            std::vector<int> ids;
            size_t max_quads = 0; double ab = 0;
            for (int q = 0; q < nj; q++) if (jobs[q].eq_n > 1) {
                ids.push_back(q);
                const size_t N = (size_t)1 << jobs[q].nvars;
                max_quads = std::max(max_quads, N >> 2);
                ab += (double)N * (8.0 * jobs[q].eq_n + 16.0);
            }
            if (!ids.empty()) {
                int* d_ids = ctx->alloc_n<int>(ids.size());
                upload(d_ids, ids.data(), ids.size() * sizeof(int), "upload eq-form job list");
                ctx->prof_begin(cls_aux, ab);
                dev::ps_eq_A(st, d_jobs, d_ids, (int)ids.size(), max_quads);
                ctx->prof_end();
            }
        }
        if (!all_items.empty()) {
            dev::PsItem* d_items = ctx->alloc_n<dev::PsItem>(all_items.size());
            upload(d_items, all_items.data(), all_items.size() * sizeof(dev::PsItem), "upload items");
            for (auto& L : launches) {
                ctx->prof_begin(L.two ? cls_ps2 : cls_ps, L.bytes, -1.0, L.design);
                dev::ps_round(st, L.two, d_jobs, d_items + L.off, L.cnt, L.grid, ctx->d_chal, partials, d_res(), L.eq);
                ctx->prof_end();
            }
        }
        double tb = 0, td = 0;
        for (auto& J : jobs) {
            for (int rd = J.tail_rd; rd < J.nvars; rd++) tb += round_bytes(J, rd);
            if (J.tail_rd < J.nvars) {   // the tail reads its first round's tables (an eq-factored job: the a tables and a suffix table), the rest runs in LDS
                const size_t half = ((size_t)1 << J.nvars) >> (J.tail_rd + 1);
                td += (double)J.npairs * 2.0 * half * (J.tail_rd == 0 ? 8 : 16) + (J.eq_n ? 2.0 * half * 16 : (double)J.npairs * 2.0 * half * 16);
            }
        }
        ctx->prof_begin(cls_ps_tail, tb, -1.0, td);
        dev::ps_tail(st, d_jobs, nj, ctx->d_chal, d_res());
        ctx->prof_end();
    }
    static constexpr size_t MAX_BATCH = 64;
    // pinned staging for small host->device descriptor copies (kept alive until the final synchronisation)
    // small host->device descriptor copy through the staging buffer, on the current stream
    // Descriptor uploads (jobs, items, hash sources ...). Their contents depend on the key and the share only - the challenges are
    // known up front - so a prove that is being recorded into a launch graph does not record them: they are copied ONCE before the
    // first replay (prove_capture) and stay in the arena, which nothing else touches while the cached graph is valid (arena_epoch).
    // As graph nodes they cost about 5 us each on the stream they sit on, ten to twenty per prove.
    bool defer_uploads = false;
    struct Upload { void* dst; const void* src; size_t bytes; };
    std::vector<Upload> deferred_uploads;
    void upload(void* dst, const void* src, size_t bytes, const char* what) {
        const void* staged = stage(src, bytes);
        if (defer_uploads) { deferred_uploads.push_back(Upload{dst, staged, bytes}); return; }
        hip_check(hipMemcpyAsync(dst, staged, bytes, hipMemcpyHostToDevice, st), what);
    }
    // Challenge-only tables (DESIGN.md 3.7). In mode 0 the challenges are the fixed chain, so a table built from the chain and the
    // key's wiring alone is the same for every witness proven under the key. A prove that is being recorded into a launch graph does
    // not record a launch that reads nothing else and writes such tables only: it is kept as a closure and runs ONCE after the
    // capture (prove_capture), behind the descriptor uploads it reads; its tables stay in the graph's private arena, a pure bump
    // allocation. Whether a launch qualifies is decided from its inputs (const_src), and the address ranges written by hoisted
    // launches are kept: a launch that stays in the graph and writes into one of them ends the capture (plain launches then).
    bool hoist_consts = false;
    struct ConstRange { const char* lo; const char* hi; };
    std::vector<std::function<void(hipStream_t)>> hoisted;
    std::vector<ConstRange> hoisted_ranges, kept_ranges;   // kept: tables written by launches of the same kinds that stay recorded
    std::vector<const void*> key_allocs;  // sorted base addresses of the key's device memory (set with hoist_consts)
    int n_hoisted = 0, n_split = 0;        // launches hoisted; queues flushed as a hoisted and a kept launch
    size_t hoisted_bytes = 0;
    template <typename T> static ConstRange crange(const T* p, size_t n) {
        return ConstRange{reinterpret_cast<const char*>(p), reinterpret_cast<const char*>(p) + n * sizeof(T)};
    }
    bool in_hoisted(ConstRange r) const {
        for (const ConstRange& h : hoisted_ranges) if (r.lo < h.hi && h.lo < r.hi) return true;
        return false;
    }
    // a buffer a hoisted launch may read: absent, the key's, or a table written by an earlier hoisted launch
    bool const_src(const void* p) const {
        if (!p) return true;
        if (std::binary_search(key_allocs.begin(), key_allocs.end(), p, std::less<const void*>())) return true;
        const char* c = static_cast<const char*>(p);
        return in_hoisted(ConstRange{c, c + 1});
    }
    void kept_writes(ConstRange r) const {
        if (hoist_consts && r.lo && r.lo < r.hi && in_hoisted(r)) throw Error("launch graph: a recorded launch writes a table that was built once");
    }
    // `fn(stream)` issues `nlaunch` kernels that write `writes`; constant: every buffer they read passes const_src
    template <typename Fn> void issue_const(bool constant, const std::vector<ConstRange>& writes, int nlaunch, Fn fn) {
        if (!(hoist_consts && constant)) {
            for (const ConstRange& w : writes) { kept_writes(w); if (hoist_consts && w.lo && w.lo < w.hi) kept_ranges.push_back(w); }
            fn(st);
            return;
        }
        for (const ConstRange& w : writes) {
            if (!w.lo || w.lo >= w.hi) continue;
            bool clash = in_hoisted(w);
            for (const ConstRange& k : kept_ranges) clash = clash || (w.lo < k.hi && k.lo < w.hi);
            if (clash) throw Error("launch graph: two launches build one challenge-only table");
            hoisted_ranges.push_back(w);
            hoisted_bytes += (size_t)(w.hi - w.lo);
        }
        hoisted.push_back(fn);
        n_hoisted += nlaunch;
    }
    void* stage(const void* src, size_t bytes) {
        size_t need = (bytes + 63) & ~(size_t)63;
        if (ctx->stage_used + need > ctx->stage_cap) throw Error("staging buffer exhausted");
        void* p = ctx->h_stage + ctx->stage_used;
        ctx->stage_used += need;
        memcpy(p, src, bytes);
        return p;
    }

    // transcript side of prove_sum_check: d+1 coefficients per round, eval(1) derived from the running claim
    void defer_sumcheck(const ScHandle& h, int deg, Cell claim_in, Cell claim_out) {
        push_op([this, h, deg, claim_in, claim_out] {
            E2 claim = *claim_in;
            if (h.scaled)   // mirrored grand product: the kernels summed everything but the common factor 1 + kappa
                for (size_t q = 0; q < (size_t)h.nvars * h.nv; q++) ctx->h_res[h.sums_slot + q] = e2_mul(ctx->h_res[h.sums_slot + q], h.scale);
            if (h.scale_cell) {   // Libra phase 2 of a mul node run in the first wave: its tables lack the factor u = in(r_x) of phase 1
                const E2 u = *h.scale_cell;
                for (size_t q = 0; q < (size_t)h.nvars * h.nv; q++) ctx->h_res[h.sums_slot + q] = e2_mul(ctx->h_res[h.sums_slot + q], u);
            }
            for (int i = 0; i < h.nvars; i++) {
                const E2* s = h_res() + h.sums_slot + (size_t)i * h.nv;
                E2 ev[4], c[4];
                ev[0] = s[0];
                ev[1] = e2_sub(claim, s[0]);
                ev[2] = s[1];
                if (deg == 3) ev[3] = s[2];
                interpolate(ev, deg, c);
                for (int k = 0; k <= deg; k++) proof.write_e(c[k]);
                claim = horner(c, deg, h.rs[i]);
            }
            if (claim_out) *claim_out = claim;
        });
    }
    // the grand-product kernels leave the final LEFT evaluation of pair b multiplied by pw[b] (see kernels.hip)
    void defer_gp_unscale(size_t evals_slot, int nb, const dev::Powers& pw) {
        if (nb < 2) return;
        if (pw.v[1].c0 == 0 && pw.v[1].c1 == 0) throw Error("grand product: zero batching weight");
        // the inverse weights depend on the challenges only: computed here, during the walk (which a cached launch graph does not
        // repeat), not in the replay that every prove runs after its synchronisation
        auto winv = std::make_shared<std::vector<E2>>(nb);
        const E2 ginv = e2_inv(pw.v[1]);  // pw[b] = gamma^b
        E2 w = ginv;
        for (int b = 1; b < nb; b++) { (*winv)[b] = w; w = e2_mul(w, ginv); }
        push_op([this, evals_slot, nb, winv] {
            for (int b = 1; b < nb; b++) ctx->h_res[evals_slot + 2 * b] = e2_mul(ctx->h_res[evals_slot + 2 * b], (*winv)[b]);
        });
    }
    // proof map (HG_PROOF_MAP=<file>): byte offset of every protocol element, for diffing against a proof dumped by the
    // Rust reference (scripts/proof_diff.py) - each label names the convention (DESIGN.md 2) that decides those bytes
    std::vector<std::pair<size_t, std::string>> proof_map;
    void mark(const std::string& label) {
        if (hg_proof_map_path()) push_op([this, label] { proof_map.push_back({proof.bytes.size(), label}); });
    }
    void defer_write_slots(size_t s, size_t n) {
        push_op([this, s, n] { for (size_t i = 0; i < n; i++) proof.write_e(h_res()[s + i]); });
    }

    // ---- batched bookkeeping kernels (eq tables, zkCNN DFT rows, Libra gathers) ------------------------
    std::vector<dev::EqJob> eq_queue;
    std::vector<std::function<void()>> after_eq;  // device work that reads the queued eq tables
    std::vector<dev::GatherJob> gather_queue;
    std::vector<dev::GatherSegJob> gather_seg_queue;
    std::vector<dev::GatherBJob> gatherB_queue;
    std::vector<dev::FftJob> fft_queue;

    // tables an eq job writes: its factor tables and, with `fill`, the table itself
    static void eq_writes(const dev::EqJob& J, bool fill, std::vector<ConstRange>& wr) {
        if (J.ab) wr.push_back(crange(J.ab, (size_t)J.cs.n * dev::eq_ab_entries(J.n)));
        if (fill && J.out) wr.push_back(crange(J.out, (size_t)1 << J.n));
    }
    // `reused`: another launch of this prove fills the same buffer later (never built once)
    void eq_now(E2* out, int n, size_t point_off, const E2* point_dev = nullptr, bool reused = false) {  // single table, launched in place
        dev::EqJob J;
        memset(&J, 0, sizeof(J));
        J.out = out; J.n = n; J.point_dev = point_dev;
        J.cs.n = 1; J.cs.unit_alpha = 1; J.cs.point_off[0] = point_off;
        const bool two = eq_two_launch() && n <= 24;
        dev::EqAbGrid grid{0, 0};
        if (two) { J.ab = ctx->alloc_n<E2>(dev::eq_ab_entries(n)); grid = dev::eq_ab_plan(&J, 1); }
        dev::EqJob* d = ctx->alloc_n<dev::EqJob>(1);
        upload(d, &J, sizeof(J), "upload eq job");
        std::vector<ConstRange> wr;
        eq_writes(J, true, wr);
        const E2* chal = ctx->d_chal;
        ctx->prof_begin(cls_aux, 16.0 * ((size_t)1 << n));
        if (two) issue_const(!point_dev && !reused, wr, 2, [d, grid, chal](hipStream_t s) { dev::eq_jobs_ab(s, d, 1, grid, chal); });
        else issue_const(!point_dev && !reused, wr, 1, [d, n, chal](hipStream_t s) { dev::eq_jobs(s, d, 1, n, chal); });
        ctx->prof_end();
    }
    // The factor tables of the same table alone (k_eq_prep, no fill): for a table with ONE reader that forms A[j & 255] * B[j >> 8] per
    // row itself (dev::eq_jobs_prep). nullptr where that form does not exist (fewer than 8 variables, more than 24): use eq_now.
    E2* eq_prep_now(int n, size_t point_off) {
        if (!eq_two_launch() || n < 8 || n > 24) return nullptr;
        dev::EqJob J;
        memset(&J, 0, sizeof(J));
        J.n = n;
        J.cs.n = 1; J.cs.unit_alpha = 1; J.cs.point_off[0] = point_off;
        J.ab = ctx->alloc_n<E2>(dev::eq_ab_entries(n));
        const dev::EqAbGrid grid = dev::eq_ab_plan(&J, 1);
        dev::EqJob* d = ctx->alloc_n<dev::EqJob>(1);
        upload(d, &J, sizeof(J), "upload eq job");
        std::vector<ConstRange> wr;
        eq_writes(J, false, wr);
        const E2* chal = ctx->d_chal;
        ctx->prof_begin(cls_aux, 16.0 * dev::eq_ab_entries(n), 16.0 * ((size_t)1 << n));   // (reference model: the table is written)
        issue_const(true, wr, 1, [d, grid, chal](hipStream_t s) { dev::eq_jobs_prep(s, d, 1, grid, chal); });
        ctx->prof_end();
        return J.ab;
    }
    // HG_LASSO_TABLES=1: the general form of the Lasso node's single-reader eq tables (and of the output claim's) - filled, then read
    static bool lasso_tables() { static const bool on = hg_env_on("HG_LASSO_TABLES"); return on; }
    std::vector<std::function<void()>> eq_post;  // sums of per-claim eq tables, run right after the eq batch
    // (tables of more than 2^24 entries take the one-launch kernel, whose workgroups rebuild their own low / high factor tables)
    static bool eq_two_launch() { return true; }
    void queue_eq(E2* out, int n, const dev::ClaimSet& cs) {
        dev::EqJob J;
        memset(&J, 0, sizeof(J));
        J.n = n;
        if (eq_two_launch() && n <= 24) {  // all claims in one job: the fill kernel sums them
            J.out = out; J.cs = cs;
            J.ab = ctx->alloc_n<E2>((size_t)cs.n * dev::eq_ab_entries(n));
            eq_queue.push_back(J);
            return;
        }
        if (cs.n == 1) { J.out = out; J.cs = cs; eq_queue.push_back(J); return; }
        // several claims: one job per claim (all of them run in parallel in the batch), then one summing pass
        const size_t N = (size_t)1 << n;
        E2* tmp = ctx->alloc_n<E2>((size_t)cs.n * N);
        for (int a = 0; a < cs.n; a++) {
            J.out = tmp + (size_t)a * N;
            memset(&J.cs, 0, sizeof(J.cs));
            J.cs.n = 1; J.cs.unit_alpha = cs.unit_alpha; J.cs.alpha_off = cs.alpha_off + a; J.cs.point_off[0] = cs.point_off[a];
            eq_queue.push_back(J);
        }
        const int nc = cs.n;
        eq_post.push_back([this, out, tmp, nc, N] {
            issue_const(const_src(tmp), {crange(out, N)}, 1, [out, tmp, nc, N](hipStream_t s) { dev::sum_tables(s, out, tmp, nc, N); });
        });
    }
    template <typename JobT> JobT* put_jobs(const std::vector<JobT>& q) {
        JobT* d = ctx->alloc_n<JobT>(q.size());
        upload(d, q.data(), q.size() * sizeof(JobT), "upload jobs");
        return d;
    }
    // Flushes a queue of table-building jobs: each(part, constant) plans, uploads and issues one part. While a launch graph is
    // recorded, the jobs that read challenge-only inputs (is_const) are one part, built once, and the others stay recorded.
    template <typename JobT, typename Pred, typename Each>
    void flush_jobs(std::vector<JobT>& q, Pred is_const, Each each) {
        if (q.empty()) return;
        std::vector<JobT> c, k;
        if (hoist_consts) for (const JobT& J : q) (is_const(J) ? c : k).push_back(J);
        else k.swap(q);
        q.clear();
        if (!c.empty() && !k.empty()) n_split++;
        if (!c.empty()) each(c, true);
        if (!k.empty()) each(k, false);
    }
    static bool no_in_vals(const u64* const* in_vals) {
        for (int q = 0; q < dev::PS_MAX_PAIRS; q++) if (in_vals[q]) return false;
        return true;
    }
    void flush_bookkeeping() {
        const E2* chal = ctx->d_chal;
        // factor tables of the eq-factored jobs' points: the chain alone
        flush_jobs(eqpt_queue, [](const dev::PsEqPoint&) { return true; }, [&](std::vector<dev::PsEqPoint>& part, bool c) {
            double pb = 0;
            std::vector<ConstRange> wr;
            for (auto& p : part) {
                pb += 16.0 * (dev::ps_eq_lo_entries(p.nvars) + dev::ps_eq_suf_entries(p.nvars));
                wr.push_back(crange(p.lo, dev::ps_eq_lo_entries(p.nvars)));
                wr.push_back(crange(p.suf, dev::ps_eq_suf_entries(p.nvars)));
            }
            dev::PsEqPoint* d = put_jobs(part);
            const int np = (int)part.size();
            if (hg_debug("plan")) fprintf(stderr, "[hg plan] eqprep points=%d\n", np);
            ctx->prof_begin(cls_aux, pb);
            issue_const(c, wr, 1, [d, np, chal](hipStream_t s) { dev::ps_eq_prep(s, d, np, chal); });
            ctx->prof_end();
        });
        // eq tables: a point in the chain (point_dev null) and nothing else
        flush_jobs(eq_queue, [](const dev::EqJob& J) { return J.point_dev == nullptr; }, [&](std::vector<dev::EqJob>& part, bool c) {
            int max_n = 0; double eb = 0;
            bool ab = false, old = false;   // (queue_eq gives every job of a prove the same form)
            std::vector<ConstRange> wr;
            for (auto& J : part) { max_n = std::max(max_n, J.n); eb += 16.0 * ((size_t)1 << J.n); (J.ab ? ab : old) = true; eq_writes(J, true, wr); }
            if (ab && old) throw Error("eq tables: mixed job forms in one batch");
            const int nj = (int)part.size();
            dev::EqAbGrid grid{0, 0};
            if (ab) grid = dev::eq_ab_plan(part.data(), nj);
            if (hg_debug("plan")) fprintf(stderr, "[hg plan] eqtab jobs=%d ab=%d max_n=%d prep=%d fill=%d rows=%d\n", nj, ab ? 1 : 0, max_n, grid.prep, grid.fill, ab ? part[0].rows : 0);
            dev::EqJob* d = put_jobs(part);
            ctx->prof_begin(cls_aux, eb);
            if (ab) issue_const(c, wr, 2, [d, nj, grid, chal](hipStream_t s) { dev::eq_jobs_ab(s, d, nj, grid, chal); });
            else issue_const(c, wr, 1, [d, nj, max_n, chal](hipStream_t s) { dev::eq_jobs(s, d, nj, max_n, chal); });
            ctx->prof_end();
        });
        for (auto& f : eq_post) f();
        eq_post.clear();
        for (auto& f : after_eq) f();
        after_eq.clear();
        // Libra phase-1 tables: the key's wiring and the node's eq table; a mul part reads the node inputs (in_vals)
        flush_jobs(gather_queue, [&](const dev::GatherJob& J) { return no_in_vals(J.g.in_vals) && const_src(J.eqc) && const_src(J.g.lin.ptr) && const_src(J.g.mul.ptr); },
                   [&](std::vector<dev::GatherJob>& part, bool c) {
            size_t max_total = 0; double gb = 0;
            std::vector<ConstRange> wr;
            for (auto& J : part) { size_t t = (size_t)1 << (J.log2_S + J.log2_R); max_total = std::max(max_total, t); gb += 24.0 * t; wr.push_back(crange(J.T, t)); }
            dev::GatherJob* d = put_jobs(part);
            const int nj = (int)part.size();
            ctx->prof_begin(cls_gather, gb);
            issue_const(c, wr, 1, [d, nj, max_total](hipStream_t s) { dev::gather_jobs(s, d, nj, max_total); });
            ctx->prof_end();
        });
        flush_jobs(gather_seg_queue, [&](const dev::GatherSegJob& J) { return no_in_vals(J.in_vals) && const_src(J.eqc) && const_src(J.segs); },
                   [&](std::vector<dev::GatherSegJob>& part, bool c) {
            double sb = 0;
            std::vector<ConstRange> wr;
            for (auto& J : part) { size_t t = (size_t)1 << (J.log2_S + J.log2_R); sb += 16.0 * (J.nseg + 1) * t; wr.push_back(crange(J.T, t)); }
            const int nj = (int)part.size();
            const int grid = dev::gather_seg_plan(part.data(), nj);
            dev::GatherSegJob* d = put_jobs(part);
            ctx->prof_begin(cls_gather, sb);
            issue_const(c, wr, 1, [d, nj, grid](hipStream_t s) { dev::gather_seg_jobs(s, d, nj, grid); });
            ctx->prof_end();
        });
        // Libra phase-2 tables: built without u (the replay applies it) they read the wiring and two eq tables
        flush_jobs(gatherB_queue, [&](const dev::GatherBJob& J) { return J.u == nullptr && const_src(J.eqc) && const_src(J.eqx) && const_src(J.m.ptr); },
                   [&](std::vector<dev::GatherBJob>& part, bool c) {
            size_t maxB = 0; double bb = 0;
            std::vector<ConstRange> wr;
            for (auto& J : part) { size_t t = (size_t)1 << (J.log2_S + J.log2_R); maxB = std::max(maxB, t); bb += 40.0 * t; wr.push_back(crange(J.B, t)); }
            dev::GatherBJob* d = put_jobs(part);
            const int nj = (int)part.size();
            ctx->prof_begin(cls_gather, bb);
            issue_const(c, wr, 1, [d, nj, maxB](hipStream_t s) { dev::gather_B_jobs(s, d, nj, maxB); });
            ctx->prof_end();
        });
        // DFT-row tables: the key's twiddle table and claim points in the chain
        flush_jobs(fft_queue, [&](const dev::FftJob& J) { return const_src(J.W); }, [&](std::vector<dev::FftJob>& part, bool c) {
            int max_L = 0, max_claims = 1; double fb = 0;
            std::vector<ConstRange> wr;
            for (auto& J : part) { max_L = std::max(max_L, J.L); max_claims = std::max(max_claims, J.cs.n); fb += 24.0 * ((size_t)1 << J.L); wr.push_back(crange(J.out, (size_t)1 << J.L)); }
            const size_t tab_entries = part.size() * (size_t)max_claims * (((size_t)1 << max_L) >> 4) + 1;
            E2* fft_tab = ctx->alloc_n<E2>(tab_entries);
            wr.push_back(crange(fft_tab, tab_entries));
            dev::FftJob* d = put_jobs(part);
            const int nj = (int)part.size();
            if (hg_debug("plan")) fprintf(stderr, "[hg plan] fftrows jobs=%d max_L=%d max_claims=%d launches=%d\n", nj, max_L, max_claims, dev::fft_jobs_launches(max_L));
            ctx->prof_begin(cls_aux, fb);
            issue_const(c, wr, dev::fft_jobs_launches(max_L), [d, nj, max_L, max_claims, chal, fft_tab](hipStream_t s) { dev::fft_jobs(s, d, nj, max_L, max_claims, chal, fft_tab); });
            ctx->prof_end();
        });
    }
