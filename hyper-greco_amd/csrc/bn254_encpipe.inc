// hg_prove_encryptions_bn254: BfvEncrypt::prove over bn256::Fr for a run of ENCRYPTIONS - included by bn254.hip behind bn254_gkr.inc,
// inside namespace hg::bn.   [REF scripts/circuit_sk.py:18-140 followed by sk_encryption_circuit.rs:417-460, 614-626]
// Data flow of one item: the compact signed coefficients ((3+k) n words) go up once from pinned staging; k_derive_pack lays s, e, k1,
// ais out as u64 tables and the derivation (integer arithmetic, shared with the Goldilocks pipeline) writes r1is, r2is, ct0is beside
// them; k_bn_lift_pairs lifts all of them into the Montgomery node tables; the FFT groups and gate maps fill the rest. No table visits
// the host between the upload and the prove: the prover's two streams wait for the feed stream's event on the device. The u64 tables
// are also what the handle of the item is copied back from, on a copy stream behind the derivation.
// Nothing of this lies in the context arena (every BN254 prove resets it and DevPool hands it out): two table sets, the omega tables,
// the work buffers and the staging are allocated once per (context, key) and kept until the key changes or the context goes.
struct BnEncPipe {
    uint64_t pk_serial = 0;
    int device = 0;
    hipStream_t feed = nullptr, copy = nullptr;
    std::vector<void*> owned;              // device: node tables + ct0is of both sets, omega tables, FFT scratch
    BnValues V[2];
    BnLayout Y;
    Fr* d_tmp = nullptr;                   // FFT scratch of the feed stream (one: the sets are filled one after the other)
    u64* d_u64[2] = {nullptr, nullptr};    // laid-out s | e | k1 | ais | r1is | r2is | ct0is of one item each
    u64* d_work = nullptr;                 // derivation: X | NTT scratch
    int64_t* d_compact = nullptr;          // (3+k) n
    int64_t* h_compact = nullptr;          // pinned
    u32* d_flags = nullptr;                // 2 x DRV_FLAG_WORDS
    u32* h_flags = nullptr;                // pinned, 2 x DRV_FLAG_WORDS
    u64* h_back[2] = {nullptr, nullptr};   // pinned: the seven tables of one item each (allocated once handles are asked for)
    dev::DeriveArgs A[2];
    LiftJobs LJ[2];
    size_t lift_max_len = 0;
    size_t set_bytes = 0;                  // node tables + ct0is + u64 tables of ONE set
    hipEvent_t ev_t0[2] = {}, ev_t1[2] = {}, ev_derived[2] = {}, ev_flags[2] = {}, ev_copied[2] = {}, ev_ready[2] = {};
    // hg_prove_encryptions_committed_bn254, sized for the shape (c_log2, c_rows) in use: the commit's NTT temporary (R N elements) and
    // Montgomery-form twiddles (N), which both table sets use one after the other on the feed stream; per table set the tree (8 N words)
    // with the flag word behind it, in HBM and in page-locked staging; the commit's timing events and the event of the tree's copy
    int c_log2 = -1;
    size_t c_rows = 0;
    Fr* c_tmp = nullptr;
    Fr* c_W = nullptr;
    u64* c_tree[2] = {nullptr, nullptr};
    u64* h_tree[2] = {nullptr, nullptr};
    hipEvent_t ev_c0[2] = {}, ev_c1[2] = {}, ev_tree[2] = {};
    void commit_bufs_free() {
        if (c_tmp) (void)hipFree(c_tmp);
        if (c_W) (void)hipFree(c_W);
        for (auto& t : c_tree) { if (t) (void)hipFree(t); t = nullptr; }
        for (auto& t : h_tree) { if (t) (void)hipHostFree(t); t = nullptr; }
        c_tmp = c_W = nullptr;
        c_log2 = -1; c_rows = 0;
    }
    ~BnEncPipe() {
        (void)hipSetDevice(device);
        if (feed) { (void)hipStreamSynchronize(feed); (void)hipStreamDestroy(feed); }
        if (copy) { (void)hipStreamSynchronize(copy); (void)hipStreamDestroy(copy); }
        commit_bufs_free();
        for (auto* evs : {ev_c0, ev_c1, ev_tree}) for (int q = 0; q < 2; q++) if (evs[q]) (void)hipEventDestroy(evs[q]);
        for (void* p : owned) (void)hipFree(p);
        for (auto p : d_u64) if (p) (void)hipFree(p);
        if (d_work) (void)hipFree(d_work);
        if (d_compact) (void)hipFree(d_compact);
        if (d_flags) (void)hipFree(d_flags);
        if (h_compact) (void)hipHostFree(h_compact);
        if (h_flags) (void)hipHostFree(h_flags);
        for (auto p : h_back) if (p) (void)hipHostFree(p);
        for (auto* evs : {ev_t0, ev_t1, ev_derived, ev_flags, ev_copied, ev_ready}) for (int q = 0; q < 2; q++) if (evs[q]) (void)hipEventDestroy(evs[q]);
    }
};
void bn_enc_pipe_drop(hg_ctx* ctx) {
    if (!ctx->bn_enc_pipe) return;
    delete static_cast<BnEncPipe*>(ctx->bn_enc_pipe);
    ctx->bn_enc_pipe = nullptr;
}
// The feed stream's priority. The prove runs on a high-priority stream (Lasso node) and a low-priority one (node reductions); the feed
// work is wanted only by the NEXT prove, so it goes below or beside them: DESIGN.md has the measurements. HG_BN_FEED_PRIORITY = high |
// normal | low picks another one for such a measurement (read when the pipeline of a context is created).
static int feed_priority() {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || lo == hi) return 0;
    const char* e = getenv("HG_BN_FEED_PRIORITY");
    const std::string want = e ? e : "low";
    if (want == "high") return hi;
    if (want == "normal") return std::min(std::max(0, hi), lo);
    return lo;
}
static BnEncPipe* bn_enc_pipe_get(hg_ctx* ctx, const hg_pk* pk, const dev::DeriveArgs& plan, bool want_w, const std::string& who) {
    const Params& p = pk->params;
    const HCircuit& c = pk->circuit;
    const size_t SZ = p.SZ(), PZ = p.PZ(), k = (size_t)p.k;
    const size_t u64_words = (3 + 3 * k) * SZ + k * PZ;
    BnEncPipe* E = static_cast<BnEncPipe*>(ctx->bn_enc_pipe);
    if (E && E->pk_serial != pk->serial) { bn_enc_pipe_drop(ctx); E = nullptr; }
    if (!E) {
        if (c.input_ids.size() != 3 + 2 * k + 1) throw Error(who + ": unexpected input nodes");
        std::unique_ptr<BnEncPipe> N(new BnEncPipe());
        N->pk_serial = pk->serial; N->device = ctx->device;
        hipc(hipStreamCreateWithPriority(&N->feed, hipStreamNonBlocking, feed_priority()), "hipStreamCreate");
        hipc(hipStreamCreateWithFlags(&N->copy, hipStreamNonBlocking), "hipStreamCreate");
        size_t fr_elems = 0;
        auto get = [&](size_t n) {
            void* d = nullptr;
            hipc(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(Fr)), "hipMalloc(bn254 node tables)");
            N->owned.push_back(d);
            fr_elems += n;
            return static_cast<Fr*>(d);
        };
        N->Y = bn_witness_layout(pk, N->feed, get, k * SZ, N->V[0]);   // (also the once-per-key check of the gate constants)
        const size_t set_elems = N->Y.total + k * SZ;
        (void)bn_witness_layout(pk, N->feed, get, k * SZ, N->V[1], &N->V[0]);
        N->d_tmp = get(N->Y.max_grp);
        N->set_bytes = set_elems * sizeof(Fr) + u64_words * 8;
        for (auto& u : N->d_u64) hipc(hipMalloc((void**)&u, u64_words * 8), "hipMalloc(laid-out witness tables)");
        hipc(hipMalloc((void**)&N->d_work, 2 * (2 * k + 1) * SZ * 8), "hipMalloc(derivation work buffers)");
        hipc(hipMalloc((void**)&N->d_compact, (3 + k) * PZ * 8), "hipMalloc(compact coefficients)");
        hipc(hipMalloc((void**)&N->d_flags, 2 * dev::DRV_FLAG_WORDS * sizeof(u32)), "hipMalloc(derive flags)");
        hipc(hipHostMalloc((void**)&N->h_compact, (3 + k) * PZ * 8, hipHostMallocDefault), "hipHostMalloc(compact coefficients)");
        hipc(hipHostMalloc((void**)&N->h_flags, 2 * dev::DRV_FLAG_WORDS * sizeof(u32), hipHostMallocDefault), "hipHostMalloc(derive flags)");
        for (int q = 0; q < 2; q++) {
            hipc(hipEventCreate(&N->ev_t0[q]), "hipEventCreate"); hipc(hipEventCreate(&N->ev_t1[q]), "hipEventCreate");
            for (hipEvent_t* ev : {&N->ev_derived[q], &N->ev_flags[q], &N->ev_copied[q], &N->ev_ready[q]}) hipc(hipEventCreateWithFlags(ev, hipEventDisableTiming), "hipEventCreate");
            // the u64 tables of the set in the order of the handle: s | e | k1 | ais | r1is | r2is | ct0is
            u64* u = N->d_u64[q];
            dev::DeriveArgs& a = N->A[q];
            a = plan;
            a.s = u; a.e = u + SZ; a.k1 = u + 2 * SZ;
            for (size_t i = 0; i < k; i++) { a.ais[i] = u + (3 + i) * SZ; a.r1is[i] = u + (3 + k + i) * SZ; }
            a.r2is = u + (3 + 2 * k) * SZ;
            a.ct0is = a.r2is + k * PZ;
            a.X = N->d_work;
            a.flags = N->d_flags + (size_t)q * dev::DRV_FLAG_WORDS;
            // input q of the circuit is table q of that order, ct0is the last one
            N->lift_max_len = bn_lift_jobs(pk, N->V[q], [&](int x, size_t) { return (size_t)x <= 3 + 2 * k ? u + (size_t)x * SZ : a.ct0is; }, N->LJ[q]);
            for (int j = 0; j < N->LJ[q].n; j++)
                if (((uintptr_t)N->LJ[q].src[j] & 15) || (N->LJ[q].len[j] & 1)) throw Error(who + ": an input table is not laid out for 16-byte loads");
        }
        hipc(hipStreamSynchronize(N->feed), "bn254 omega tables");
        if (hg_times("bn"))
            fprintf(stderr, "[hg bn] encryption pipeline: one table set %zu bytes (node tables %zu, ct0is %zu, u64 tables %zu), omega tables + FFT scratch %zu bytes\n",
                    N->set_bytes, N->Y.total * sizeof(Fr), k * SZ * sizeof(Fr), u64_words * 8, (fr_elems - 2 * set_elems) * sizeof(Fr));
        ctx->bn_enc_pipe = E = N.release();
    }
    if (want_w)
        for (auto& b : E->h_back)
            if (!b) hipc(hipHostMalloc((void**)&b, u64_words * 8, hipHostMallocDefault), "hipHostMalloc(witness copy-back staging)");
    return E;
}
// the commit's buffers for shape sh (nothing of an earlier run is in flight: every run drains the two side streams on its way out)
static void bn_enc_pipe_commit_bufs(BnEncPipe* E, const pcs::Shape& sh) {
    for (int q = 0; q < 2; q++) {
        if (E->ev_c0[q]) continue;
        hipc(hipEventCreate(&E->ev_c0[q]), "hipEventCreate"); hipc(hipEventCreate(&E->ev_c1[q]), "hipEventCreate");
        hipc(hipEventCreateWithFlags(&E->ev_tree[q], hipEventDisableTiming), "hipEventCreate");
    }
    if (E->c_log2 == sh.c && E->c_rows == sh.R) return;
    E->commit_bufs_free();
    const size_t N = sh.N(), R = sh.R;
    hipc(hipMalloc((void**)&E->c_tmp, R * N * sizeof(Fr)), "hipMalloc(commit NTT temporary)");
    hipc(hipMalloc((void**)&E->c_W, N * sizeof(Fr)), "hipMalloc(commit twiddles)");
    for (int q = 0; q < 2; q++) {
        hipc(hipMalloc((void**)&E->c_tree[q], (8 * N + 2) * 8), "hipMalloc(commit tree)");
        hipc(hipHostMalloc((void**)&E->h_tree[q], (8 * N + 2) * 8, hipHostMallocDefault), "hipHostMalloc(commit tree staging)");
    }
    E->c_log2 = sh.c; E->c_rows = R;
}

// Schedule, per item i (table set i & 1):
//   host: wait for item i's flag words (its derivation ran under prove i-1) - a refused item is never proven;
//         stage item i+1's coefficients and enqueue, on the feed stream, into the OTHER set (prove i-1, its last reader, has completed):
//         one copy, k_derive_pack, NTTs, derive_mul, derive_combine, [ev_derived] lift, FFT groups, gate maps, [ev_ready]; on the copy
//         stream behind [ev_derived]: the flag words, then the tables of the handle;
//         prove i (its streams wait for ev_ready of set i & 1 on the device), with its own synchronisations and transcript replay:
//         the feed work of item i+1 runs on the device meanwhile.
// With cmt (hg_prove_encryptions_committed_bn254) the fill goes on, still on the feed stream, behind [ev_ready]: [ev_c0] the commit to
// the set's secret u64 tables into the item's slot of its group's allocation (pcs_commit_words_enqueue: the staging kernel that
// lifts, NTT, column hashes, tree) [ev_c1]; on the copy stream behind [ev_c1]: the tree and the flag word into page-locked staging
// [ev_tree]. The commit delays neither [ev_ready] nor the flag words; the refill of the set two items later is behind it on the same
// stream. No stream is added: the Goldilocks pipeline measured a fifth one as slower (prover.hip, above prove_encryptions).
std::vector<EncResult> prove_encryptions_bn254(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                                               const int64_t* const* a, size_t n_enc, bool want_w, double* total_ms, const char* who_c, EncCommit* cmt) {
    hipc(hipSetDevice(ctx->device), "hipSetDevice");
    const double t_all = wall_ms();
    const std::string who(who_c);
    const Params& p = pk->params;
    dev::DeriveArgs plan;
    derive_plan(p, &plan);   // (parameters the derivation cannot serve are an error of the call, before anything is enqueued)
    std::vector<EncResult> out(n_enc);
    if (cmt) { cmt->cms.clear(); cmt->cms.resize(n_enc); cmt->ms.assign(n_enc, 0.0); }
    if (!n_enc) return out;
    const size_t SZ = p.SZ(), PZ = p.PZ(), k = (size_t)p.k;
    BnEncPipe* E = bn_enc_pipe_get(ctx, pk, plan, want_w, who);
    hipStream_t sf = E->feed, sc = E->copy;
    // the commitments' matrices: items in groups cut as pcs_commit_device_batch cuts them (at most 64, the option verify_batch_group,
    // VB_PCS_COMMIT_BUDGET_BN254), a group's in one allocation that its handles share - a freed group's where the context holds one
    // that fits - taken when the group's first item is filled. A slot is taken for good once its item is known to be proven: a refused
    // item's slot is written again by the next item, behind it on the feed stream. (Declared ahead of the guard: it drains before they
    // are freed.)
    struct Slot { std::shared_ptr<pcs::Slab> owner; Fr* rows = nullptr; Fr* M = nullptr; };
    std::vector<Slot> slots(cmt ? n_enc : 0);
    struct { std::shared_ptr<pcs::Slab> owner; Fr* p = nullptr; size_t cap = 0, used = 0; } slab;
    size_t c_member = 0, c_group = 0, c_N = 0;
    const u64* c_tabs[2][pcs::MAX_TABLES];
    std::shared_ptr<pcs::SlabSpares> spares;
    if (cmt) {
        const pcs::Shape& sh = cmt->sh;
        bool fits = sh.R <= 65535 && sh.c >= 1 && sh.nvars.size() == 4 + k;
        for (size_t t = 0; fits && t < 4 + k; t++) fits = ((size_t)1 << sh.nvars[t]) == (t < 3 + k ? SZ : k * PZ);
        if (!fits) throw Error(who + ": the commitment's shape is not that of the secret inputs");
        bn_enc_pipe_commit_bufs(E, sh);
        c_N = sh.N();
        c_member = sh.R * (sh.C() + c_N);   // elements
        const auto groups = pcs::cut_groups(ctx, n_enc, [&](size_t) { return c_member * sizeof(Fr); }, sh.R, 65535, VB_PCS_COMMIT_BUDGET_BN254);
        c_group = groups[0].second - groups[0].first;
        spares = batch_bufs(ctx)->slabs;
        for (int q = 0; q < 2; q++) {   // the tables of hg_secrets_commit_bn254, in its order: s, e, k1, r1is, r2is
            const dev::DeriveArgs& A = E->A[q];
            size_t t = 0;
            c_tabs[q][t++] = A.s; c_tabs[q][t++] = A.e; c_tabs[q][t++] = A.k1;
            for (size_t i = 0; i < k; i++) c_tabs[q][t++] = A.r1is[i];
            c_tabs[q][t++] = A.r2is;
        }
    }
    // whatever happens, nothing of this run is left in flight on the two side streams when the call returns
    struct Drain { hipStream_t a, b; ~Drain() { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); } } drain{sf, sc};
    BnStreams swap(ctx);
    u64* scratch = E->d_work + (2 * k + 1) * SZ;
    auto fill = [&](size_t i, int set) {
        int64_t* h = E->h_compact;   // (its last DMA, item i-1's, is complete: that item's flag words have been waited for)
        par_copy(h, s[i], PZ * 8); par_copy(h + PZ, e[i], PZ * 8); par_copy(h + 2 * PZ, k1[i], PZ * 8); par_copy(h + 3 * PZ, a[i], k * PZ * 8);
        const dev::DeriveArgs& A = E->A[set];
        if (want_w) hipc(hipStreamWaitEvent(sf, E->ev_copied[set], 0), "stream wait");   // (the handle of the set's last item has left its tables)
        hipc(hipEventRecord(E->ev_t0[set], sf), "event record");
        hipc(hipMemcpyAsync(E->d_compact, h, (3 + k) * PZ * 8, hipMemcpyHostToDevice, sf), "upload coefficients");
        derive_enqueue_compact(sf, A, E->d_compact, p.L, pk->w_fwd.at(p.L), pk->w_inv.at(p.L), scratch);
        hipc(hipEventRecord(E->ev_derived[set], sf), "event record");
        bn_witness_enqueue(pk, E->Y, E->V[set], E->LJ[set], E->lift_max_len, true, E->d_tmp, sf);
        hipc(hipGetLastError(), "bn254 witness generation: launch");
        hipc(hipEventRecord(E->ev_t1[set], sf), "event record");
        hipc(hipEventRecord(E->ev_ready[set], sf), "event record");
        hipc(hipStreamWaitEvent(sc, E->ev_derived[set], 0), "stream wait");
        hipc(hipMemcpyAsync(E->h_flags + (size_t)set * dev::DRV_FLAG_WORDS, A.flags, dev::DRV_FLAG_WORDS * sizeof(u32), hipMemcpyDeviceToHost, sc), "download derive flags");
        hipc(hipEventRecord(E->ev_flags[set], sc), "event record");
        if (want_w) {
            hipc(hipMemcpyAsync(E->h_back[set], E->d_u64[set], ((3 + 3 * k) * SZ + k * PZ) * 8, hipMemcpyDeviceToHost, sc), "download witness tables");
            hipc(hipEventRecord(E->ev_copied[set], sc), "event record");
        }
        if (cmt) {   // behind the node tables, so that ev_ready is not held up: the commit to the set's five kinds of secret tables
            const pcs::Shape& sh = cmt->sh;
            if (!slab.owner || slab.used == slab.cap) {
                slab.cap = std::min(c_group, n_enc - i);
                slab.used = 0;
                slab.owner = std::make_shared<pcs::Slab>();
                slab.owner->home = spares;
                const size_t bytes = slab.cap * c_member * sizeof(Fr);
                slab.owner->p = spares->take(bytes, &slab.owner->bytes);   // a freed group's allocation, if the context holds one that fits
                if (!slab.owner->p) {
                    hipc(hipMalloc((void**)&slab.owner->p, bytes), "hipMalloc(pcs rows and encoded matrices of a group)");
                    slab.owner->bytes = bytes;
                }
                slab.p = reinterpret_cast<Fr*>(slab.owner->p);
            }
            Slot& sl = slots[i];
            sl.owner = slab.owner;
            sl.rows = slab.p + slab.used * sh.R * sh.C();
            sl.M = slab.p + slab.cap * sh.R * sh.C() + slab.used * sh.R * c_N;
            u64* tree = E->c_tree[set];
            hipc(hipStreamWaitEvent(sf, E->ev_tree[set], 0), "stream wait");   // (the tree of the set's last item has left the device)
            hipc(hipEventRecord(E->ev_c0[set], sf), "event record");
            pcs_commit_words_enqueue(sf, sh, c_tabs[set], sl.rows, sl.M, E->c_tmp, E->c_W, tree, reinterpret_cast<unsigned*>(tree + 8 * c_N));
            hipc(hipGetLastError(), "bn254 commit from the witness words: launch");
            hipc(hipEventRecord(E->ev_c1[set], sf), "event record");
            hipc(hipStreamWaitEvent(sc, E->ev_c1[set], 0), "stream wait");
            hipc(hipMemcpyAsync(E->h_tree[set], tree, (8 * c_N + 1) * 8, hipMemcpyDeviceToHost, sc), "download tree and flag");
            hipc(hipEventRecord(E->ev_tree[set], sc), "event record");
        }
    };
    // the flag words of item i: "" or the reason it is refused
    auto refusal = [&](size_t i, int set) -> std::string {
        hipc(hipEventSynchronize(E->ev_flags[set]), "wait for the derive flags");
        try {
            derive_check_flags(p, E->h_flags + (size_t)set * dev::DRV_FLAG_WORDS, (who + ": encryption " + std::to_string(i)).c_str());
        } catch (const Error& err) { return err.what(); }
        return "";
    };
    // after prove i has completed: device time of its upload + derivation + lift + evaluation, its handle
    auto collect = [&](size_t i, int set) {
        float ms = 0;
        hipc(hipEventElapsedTime(&ms, E->ev_t0[set], E->ev_t1[set]), "event elapsed");
        out[i].witness_gpu_ms = ms;
        if (cmt) {   // the tree into the handle; the commit's device time counts as the witness's
            hipc(hipEventSynchronize(E->ev_tree[set]), "wait for the commitment's tree");
            const u64* h = E->h_tree[set];
            if ((unsigned)h[8 * c_N]) throw Error(who + ": encryption " + std::to_string(i) + ": a derived table holds a word that is not below p");
            hipc(hipEventElapsedTime(&ms, E->ev_c0[set], E->ev_c1[set]), "event elapsed");
            cmt->ms[i] = ms;
            out[i].witness_gpu_ms += ms;
            std::unique_ptr<pcs::Commitment> cm(new pcs::Commitment());
            cm->field = pcs::BN254;
            cm->sh = cmt->sh;
            cm->ctx = ctx;
            cm->d_rows = reinterpret_cast<u64*>(slots[i].rows);
            cm->d_M = reinterpret_cast<u64*>(slots[i].M);
            cm->owner = slots[i].owner;
            cm->tree.resize(32 * (2 * c_N - 1));
            par_copy(cm->tree.data(), h, cm->tree.size());
            cmt->cms[i] = std::move(cm);
        }
        if (!want_w) return;
        hipc(hipEventSynchronize(E->ev_copied[set]), "wait for the witness copy-back");
        Witness& w = out[i].w;
        const u64* b = E->h_back[set];
        auto take = [&](std::vector<u64>& dst, size_t words) { dst.resize(words); par_copy(dst.data(), b, words * 8); b += words; };
        take(w.s, SZ); take(w.e, SZ); take(w.k1, SZ); take(w.ais, k * SZ); take(w.r1is, k * SZ); take(w.r2is, k * PZ); take(w.ct0is, k * SZ);
    };
    fill(0, 0);
    for (size_t i = 0; i < n_enc; i++) {
        const int cur = (int)(i & 1);
        out[i].reason = refusal(i, cur);
        out[i].refused = !out[i].reason.empty();
        if (cmt && !out[i].refused) slab.used++;   // (the next fill takes the next slot)
        if (i + 1 < n_enc) fill(i + 1, cur ^ 1);
        if (out[i].refused) continue;   // never proven: the tables of this set hold a witness that fails its range checks
        ctx->arena_reset();
        BnProver P(ctx, pk);
        P.run_filled(E->V[cur], E->ev_ready[cur], &out[i].r.prove_ms);
        out[i].r.proof = std::move(P.proof);
        collect(i, cur);
    }
    hipc(hipStreamSynchronize(sf), "feed stream");
    hipc(hipStreamSynchronize(sc), "copy stream");
    if (total_ms) *total_ms = wall_ms() - t_all;
    return out;
}
