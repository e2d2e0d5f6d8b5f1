// The host side of a batched device verification, written once for both fields (verifier_batch.hip instantiates it with E2,
// bn254_verify_batch.inc with bn::Fr): the backend that RECORDS a walk's jobs, the merge of a group's records into the group's jobs,
// the work units of the input evaluations, and the loop over the groups. Everything here handles indices, keys and host vectors;
// what becomes of a group's jobs on the device - tables, descriptors, launches - is each field's lowering, in its own file.
// (No HIP call outside the templates of the group loop and the stream guard: tests/verify_merge_check.cpp runs the recorder and the
// merge on the host alone.)
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <omp.h>
#include <string>
#include <utility>
#include <vector>
#include "kernels.hpp"
#include "prover.hpp"

namespace hg {

// Kernels, descriptor copies and input copies may be queued on any way out of an entry (a rejection, an hg::Error): its streams are
// drained before the caller may reuse the arena and the staging or free a witness, an instance or an opening.
struct Drain {
    hipStream_t a, b = nullptr;
    ~Drain() {
        (void)hipStreamSynchronize(a);
        if (b) (void)hipStreamSynchronize(b);
    }
};

// one proof's public inputs in a set, in the order of the single-proof verifiers: s, e, k1, ais (k), r1is (k), r2is, then ct0is -
// the same signed integers in the same layout over both fields
struct BatchInputs {
    size_t SZ, PZ, K, words;
    explicit BatchInputs(const Params& p) : SZ(p.SZ()), PZ(p.PZ()), K((size_t)p.k), words((3 + 3 * K) * SZ + K * PZ) {}
    size_t offset(int k) const {   // the verifier's input table k (k < 0: ct0is)
        if (k < 0) return (3 + 2 * K) * SZ + K * PZ;
        if ((size_t)k < 3 + 2 * K) return (size_t)k * SZ;   // s, e, k1, then ais and r1is, SZ each
        return (3 + 2 * K) * SZ;                           // r2is
    }
    size_t length(int k) const { return k < 0 ? K * SZ : (size_t)k == 3 + 2 * K ? K * PZ : SZ; }
};

// ---- the recording backend ----------------------------------------------------------------------------------------------------------
// The same calls as DevBackend (verifier_dev.hip) and BnDevBackend (bn254_verify.inc), kept as symbolic jobs: tables are indices into
// the proof's own lists, chain offsets are local to the proof's chain, tickets are local result slots. value() reads the slots the
// batch copied back, in the form the walk computes in (E2; Fr in Montgomery form).
// fr_checks: what only BnDevBackend refuses - an arity its phase-2 gather cannot hold, a DFT beyond Fr's two-adicity, a claim point
// that does not fit its input table - is refused here too, with its texts, where that backend refuses it.
template <class F> struct RecBackendT : VerifyBackendT<F> {
    typedef typename VerifyBackendT<F>::ClaimOffs ClaimOffs;
    const hg_pk* pk;
    BatchInputs L;
    struct Eq { int nvars; dev::ClaimSet cs; };
    struct Const { int node, eqc, slot; };
    struct Lin { int node, in, eqc; };
    struct Mul { int node, in, eqc, eqx; size_t u_at; };
    struct Fft { int node; dev::ClaimSet cs; };
    enum { D_LIN, D_MUL, D_FFT };
    struct Dot { int kind, tab, eq, slot; };
    struct In { int k, eq, slot; };   // k < 0: ct0is
    std::vector<Eq> eqs;
    std::vector<Const> consts;
    std::vector<Lin> lins;
    std::vector<Mul> muls;
    std::vector<Fft> ffts;
    std::vector<Dot> dots;
    std::vector<In> ins;
    std::vector<F> us;             // phase-1 evaluations of the Vanilla nodes with a phase 2, back to back, as the walk has them
    size_t chain_need = 0;         // one past the last chain entry a job reads
    int nslots = 0;
    std::vector<F> res;            // the results, filled after the group's synchronisation
    int node = -1, eqc = -1, eqx = -1, eqy = -1;
    size_t u_at = 0;
    dev::ClaimSet cs;

    // the public forms (the counterpart of DevBackend::cp): the public tables are compact signed coefficients, mle_input for inputs
    // 3 .. 3+k-1 and mle_ct0is record compact input jobs, any other input is refused
    const Params* cp = nullptr;
    bool fr_checks;

    RecBackendT(const hg_pk* k, bool compact, bool fr_checks_) : pk(k), L(k->params), cp(compact ? &k->params : nullptr), fr_checks(fr_checks_) {
        memset(&cs, 0, sizeof(cs));
    }
    int slot() { return nslots++; }
    void reads_chain(const dev::ClaimSet& c, int nvars) {
        for (int a = 0; a < c.n; a++) chain_need = std::max(chain_need, c.point_off[a] + (size_t)nvars);
        if (!c.unit_alpha) chain_need = std::max(chain_need, c.alpha_off + (size_t)c.n);
    }
    int eq_of(int nvars, const dev::ClaimSet& c) {
        reads_chain(c, nvars);
        eqs.push_back(Eq{nvars, c});
        return (int)eqs.size() - 1;
    }
    int eq_single(int nvars, size_t off) {
        dev::ClaimSet c;
        memset(&c, 0, sizeof(c));
        c.n = 1; c.unit_alpha = 1; c.point_off[0] = off;
        return eq_of(nvars, c);
    }
    int dot(int kind, int tab, int eq) { const int t = slot(); dots.push_back(Dot{kind, tab, eq, t}); return t; }
    int in_job(int k, size_t point_off, int nvars) { const int t = slot(); ins.push_back(In{k, eq_single(nvars, point_off), t}); return t; }

    void begin_node(int id, const ClaimOffs& cl) override {
        node = id;
        const HNode& n = pk->circuit.nodes[id];
        if (cl.point_off.size() > (size_t)dev::MAX_CLAIMS) throw Error("verifier: too many claims on one node");
        memset(&cs, 0, sizeof(cs));
        cs.n = (int)cl.point_off.size();
        cs.unit_alpha = cl.unit ? 1 : 0;
        cs.alpha_off = cl.alpha_off;
        for (int a = 0; a < cs.n; a++) cs.point_off[a] = cl.point_off[a];
        eqc = n.kind == NK_VANILLA ? eq_of(n.log2_out(), cs) : -1;
        eqx = eqy = -1;
    }
    int const_sum() override { const int t = slot(); consts.push_back(Const{node, eqc, t}); return t; }
    void set_x(size_t x_off) override {
        const HNode& n = pk->circuit.nodes[node];
        eqx = eq_single(n.kind == NK_VANILLA ? n.log2_sub_in + n.log2_reps : n.log2_size, x_off);
    }
    std::vector<int> lin_terms() override {
        const HNode& n = pk->circuit.nodes[node];
        const hg_pk::NodeDev& nd = pk->node_dev[node];
        std::vector<int> tk(n.arity, -1);
        for (int i = 0; i < n.arity; i++) {
            if (!n.left_use[i] || !nd.lin[i].ptr) continue;
            lins.push_back(Lin{node, i, eqc});
            tk[i] = dot(D_LIN, (int)lins.size() - 1, eqx);
        }
        return tk;
    }
    void set_y(size_t y_off, const std::vector<F>& u) override {
        const HNode& n = pk->circuit.nodes[node];
        if (fr_checks && n.arity > dev::PS_MAX_PAIRS) throw Error("verifier: arity too large");
        eqy = eq_single(n.log2_sub_in + n.log2_reps, y_off);
        u_at = us.size();
        us.insert(us.end(), u.begin(), u.end());
    }
    std::vector<int> mul_terms() override {
        const HNode& n = pk->circuit.nodes[node];
        const hg_pk::NodeDev& nd = pk->node_dev[node];
        std::vector<int> tk(n.arity, -1);
        for (int i = 0; i < n.arity; i++) {
            if (!n.right_use[i] || !nd.mulR[i].ptr) continue;
            muls.push_back(Mul{node, i, eqc, eqx, u_at});
            tk[i] = dot(D_MUL, (int)muls.size() - 1, eqy);
        }
        return tk;
    }
    int fft_term() override {
        const int L2 = pk->circuit.nodes[node].log2_size;
        if (fr_checks && L2 > 28) throw Error("bn254: two-adicity is 28");
        reads_chain(cs, L2);
        ffts.push_back(Fft{node, cs});
        return dot(D_FFT, (int)ffts.size() - 1, eqx);
    }
    void end_node() override { node = -1; }
    void fits(int k, int nvars) const {
        if (fr_checks && (nvars < 0 || nvars > 40 || ((size_t)1 << nvars) != L.length(k))) throw Error("verifier: claim point does not fit the input table");
    }
    int mle_input(size_t k, size_t point_off, int nvars) override {
        if (cp) {
            if (k < 3 || k >= 3 + (size_t)cp->k) throw Error("verifier: input " + std::to_string(k) + " is not a public table");
            if (nvars != cp->L) throw Error("verifier: a point of the wrong length for a public table");   // (the job reads 2n eq entries)
        } else {
            if (k >= 3 + 2 * L.K + 1) throw Error("verifier: no such input table");
            fits((int)k, nvars);
        }
        return in_job((int)k, point_off, nvars);
    }
    int mle_ct0is(size_t point_off, int nvars) override {
        if (cp) {
            if (nvars != cp->ct0is_log2()) throw Error("verifier: a point of the wrong length for a public table");   // (k * 2n eq entries)
        } else fits(-1, nvars);
        return in_job(-1, point_off, nvars);
    }
    void finish() override { throw Error("verifier: a recording backend is finished by its batch"); }
    F value(int t) const override { return res[t]; }
};

template <class F> struct Walked {   // one proof of a group
    size_t idx;
    std::unique_ptr<RecBackendT<F>> rec;
    VerifyPendingT<F> pend;
    std::string error;                       // an hg::Error of the walk
    std::vector<int> gslot;                  // local slot -> the group's result slot
};

// ---- the merge of a group --------------------------------------------------------------------------------------------------------------
// dedup keys: a job's descriptor with absolute chain offsets
typedef std::vector<u64> Key;
inline void key_cs(Key& k, const dev::ClaimSet& c, size_t base) {
    k.push_back((u64)c.n);
    k.push_back((u64)c.unit_alpha);
    if (!c.unit_alpha) k.push_back(c.alpha_off + base);
    for (int a = 0; a < c.n; a++) k.push_back(c.point_off[a] + base);
}
inline dev::ClaimSet shift_cs(dev::ClaimSet c, size_t base) {
    if (!c.unit_alpha) c.alpha_off += base;
    for (int a = 0; a < c.n; a++) c.point_off[a] += base;
    return c;
}

// a group's jobs: tables are indices into these lists, chain offsets are absolute, slots are the group's result slots
template <class F> struct MergedGroup {
    struct Eq { int n; dev::ClaimSet cs; };
    struct Const { int node, eq, slot; };
    struct Lin { int node, in, eq; };
    struct Mul { int node, in, eqc, eqx; size_t u_at; };   // u_at: its phase-1 evaluations in `us`
    struct Fft { int node; dev::ClaimSet cs; };
    struct Dot { int kind, tab, eq, slot; };               // kind: RecBackendT::D_*, tab: an index into lins, muls or ffts
    struct In { int k, eq, slot; size_t w; };              // input table k (k < 0: ct0is) of the group's proof w
    std::vector<Eq> eqs;
    std::vector<Const> consts;
    std::vector<Lin> lins;
    std::vector<Mul> muls;
    std::vector<Fft> ffts;
    std::vector<Dot> dots;
    std::vector<In> ins;
    std::vector<F> chain;          // own chains: the proofs' chains back to back
    std::vector<F> us;             // the phase-1 evaluations, as the walks hold them
    size_t chain_need = 0;         // one chain for all: one past the last entry a job reads
    int nslot = 0;
};

// Merges the records of a group's proofs, in their order; a proof the walk rejected with no check pending (!pend.live()) contributes
// nothing - its recorded prefix is not launched; one that keeps the checks of the Vanilla nodes it had reached contributes its prefix. Identical eq tables, constant sums, phase-1 gathers, DFT-row tables and their dot products become one job
// and one slot. Phase-2 gathers and their dots (they read the proof's own phase-1 evaluations) and the input jobs (they read the
// proof's own witness or instance) are never shared. own_chains: the jobs read the concatenation of the proofs' own chains
// (pend.chain), each proof's offsets shifted by its base - so two proofs share nothing; else every proof reads one chain at its
// offsets as they are. Sets every merged proof's gslot. The caller has checked that no job reads past its chain.
template <class F> MergedGroup<F> merge_group(std::vector<Walked<F>>& W, bool own_chains) {
    typedef RecBackendT<F> Rec;
    MergedGroup<F> M;
    std::map<Key, int> eq_ix, const_ix, lin_ix, fft_ix, dot_ix;
    auto new_slot = [&] { return M.nslot++; };
    for (size_t w = 0; w < W.size(); w++) {
        Walked<F>& x = W[w];
        if (!x.pend.live()) continue;
        const Rec& R = *x.rec;
        size_t base = 0;
        if (own_chains) {
            base = M.chain.size();
            M.chain.insert(M.chain.end(), x.pend.chain.begin(), x.pend.chain.end());
        } else M.chain_need = std::max(M.chain_need, R.chain_need);
        x.gslot.assign(R.nslots, -1);
        std::vector<int> geq(R.eqs.size());
        for (size_t e = 0; e < R.eqs.size(); e++) {
            Key k{(u64)R.eqs[e].nvars};
            key_cs(k, R.eqs[e].cs, base);
            auto it = eq_ix.find(k);
            if (it == eq_ix.end()) {
                M.eqs.push_back({R.eqs[e].nvars, shift_cs(R.eqs[e].cs, base)});
                it = eq_ix.emplace(k, (int)M.eqs.size() - 1).first;
            }
            geq[e] = it->second;
        }
        for (auto& c : R.consts) {
            Key k{(u64)c.node, (u64)geq[c.eqc]};
            auto it = const_ix.find(k);
            if (it == const_ix.end()) { M.consts.push_back({c.node, geq[c.eqc], new_slot()}); it = const_ix.emplace(k, (int)M.consts.size() - 1).first; }
            x.gslot[c.slot] = M.consts[it->second].slot;
        }
        std::vector<int> glin(R.lins.size()), gmul(R.muls.size()), gfft(R.ffts.size());
        for (size_t i = 0; i < R.lins.size(); i++) {
            const auto& l = R.lins[i];
            Key k{(u64)l.node, (u64)l.in, (u64)geq[l.eqc]};
            auto it = lin_ix.find(k);
            if (it == lin_ix.end()) { M.lins.push_back({l.node, l.in, geq[l.eqc]}); it = lin_ix.emplace(k, (int)M.lins.size() - 1).first; }
            glin[i] = it->second;
        }
        for (size_t i = 0; i < R.muls.size(); i++) {
            const auto& m = R.muls[i];
            M.muls.push_back({m.node, m.in, geq[m.eqc], geq[m.eqx], M.us.size() + m.u_at});
            gmul[i] = (int)M.muls.size() - 1;
        }
        M.us.insert(M.us.end(), R.us.begin(), R.us.end());
        for (size_t i = 0; i < R.ffts.size(); i++) {
            Key k{(u64)R.ffts[i].node};
            key_cs(k, R.ffts[i].cs, base);
            auto it = fft_ix.find(k);
            if (it == fft_ix.end()) { M.ffts.push_back({R.ffts[i].node, shift_cs(R.ffts[i].cs, base)}); it = fft_ix.emplace(k, (int)M.ffts.size() - 1).first; }
            gfft[i] = it->second;
        }
        for (auto& d : R.dots) {
            const int tab = d.kind == Rec::D_LIN ? glin[d.tab] : d.kind == Rec::D_MUL ? gmul[d.tab] : gfft[d.tab];
            if (d.kind == Rec::D_MUL) { M.dots.push_back({d.kind, tab, geq[d.eq], new_slot()}); x.gslot[d.slot] = M.dots.back().slot; continue; }
            Key k{(u64)d.kind, (u64)tab, (u64)geq[d.eq]};
            auto it = dot_ix.find(k);
            if (it == dot_ix.end()) { M.dots.push_back({d.kind, tab, geq[d.eq], new_slot()}); it = dot_ix.emplace(k, (int)M.dots.size() - 1).first; }
            x.gslot[d.slot] = M.dots[it->second].slot;
        }
        for (auto& in : R.ins) {
            const int sl = new_slot();
            M.ins.push_back({in.k, geq[in.eq], sl, w});
            x.gslot[in.slot] = sl;
        }
    }
    return M;
}

// ---- the work units of the input evaluations ------------------------------------------------------------------------------------------
// A unit is one eq table and the P tables evaluated at its point; workgroup b of the unit owns a tile of its n entries and writes
// `per_wg` partials for every member: member p's partial q of workgroup b at part0 + (p * nblk + b) * per_wg + q.
// (log2_n, lo: the compact form only - n is then the count of non-padding words, blocks of 2^log2_n, word lo + r of a block's 2^(log2_n+1) eq entries)
template <class F> struct VinUnitT { const F* eq; size_t n; int first, P, nblk; u32 log2_n; size_t part0; u32 lo, pad; };
struct VinMember { const u64* a; int unit, slot; };
struct VinBlock { int unit, blk; };
// entry t of a unit: where its eq entry (ie) and its word (iw) lie. Compact form: t counts the non-padding words; with nm1 = n - 1,
// b = t >> log2_n and r = t & nm1, eq entry b * 2n + lo + r meets coefficient n-1-r of block b
template <bool COMPACT> __host__ __device__ inline void vin_at(size_t t, size_t nm1, u32 lo, size_t& ie, size_t& iw) {
    if constexpr (COMPACT) {
        const size_t r = t & nm1;
        ie = 2 * (t - r) + lo + r;
        iw = (t - r) + (nm1 - r);
    } else ie = iw = t;
}
template <class F> struct VinPlan {
    std::vector<VinUnitT<F>> units;
    std::vector<VinMember> members;
    std::vector<VinBlock> blocks;
    size_t parts = 0, bytes = 0;   // partials in all; what the dots kernel reads, eq tables and input tables
    // one more unit: `tabs` are its members' tables and result slots
    void add(const F* eq, size_t n, u32 log2_n, u32 lo, const std::vector<std::pair<const u64*, int>>& tabs, size_t tile, int per_wg) {
        VinUnitT<F> U;
        memset(&U, 0, sizeof(U));
        U.eq = eq; U.n = n; U.first = (int)members.size(); U.P = (int)tabs.size(); U.log2_n = log2_n; U.lo = lo;
        U.nblk = (int)((n + tile - 1) / tile); U.part0 = parts;
        parts += (size_t)U.P * U.nblk * per_wg;
        bytes += n * (sizeof(F) + (size_t)U.P * sizeof(u64));
        for (auto& t : tabs) members.push_back(VinMember{t.first, (int)units.size(), t.second});
        for (int b = 0; b < U.nblk; b++) blocks.push_back(VinBlock{(int)units.size(), b});
        units.push_back(U);
    }
};
// The units of a group: the input jobs at one eq table are one unit, in the order of the eq tables - but an ais table and ct0is
// never share one, even at one point: their words sit at other places of the eq table. eq_out(e): eq table e on the device. Proof w's
// inputs lie at set + w * words: laid out as BatchInputs, or, pub, its instance as it is - then a unit covers the non-padding words
// only, n of an ais table, k n of ct0is (the walk checked the eq table's size).
template <class F, class EqOut>
VinPlan<F> vin_units(const MergedGroup<F>& M, EqOut eq_out, const u64* set, size_t words, const Params& p, bool pub, size_t tile, int per_wg) {
    const BatchInputs L(p);
    const size_t kn = L.K * L.PZ;
    std::vector<std::vector<std::pair<const u64*, int>>> by_eq(2 * M.eqs.size());
    for (auto& in : M.ins) {
        const u64* d_in = set + in.w * words;
        if (pub) by_eq[2 * (size_t)in.eq + (in.k < 0)].push_back({d_in + (in.k < 0 ? kn : (size_t)(in.k - 3) * L.PZ), in.slot});
        else by_eq[2 * (size_t)in.eq].push_back({d_in + L.offset(in.k), in.slot});
    }
    VinPlan<F> V;
    for (size_t e2x = 0; e2x < by_eq.size(); e2x++) {
        if (by_eq[e2x].empty()) continue;
        const size_t e = e2x / 2;
        if (pub) V.add(eq_out(e), e2x & 1 ? kn : L.PZ, (u32)p.n_log2, e2x & 1 ? (u32)(L.PZ - 1) : 0, by_eq[e2x], tile, per_wg);
        else V.add(eq_out(e), (size_t)1 << M.eqs[e].n, 0, 0, by_eq[e2x], tile, per_wg);
    }
    return V;
}

// ---- the pass over the groups -----------------------------------------------------------------------------------------------------------
// proofs [i0, i1) walked on the host threads, one each: one(x) makes x.rec and x.pend. The walk opens no OpenMP region of its own,
// so nothing nests. An hg::Error of a walk leaves with its proof's index.
template <class F, class One> void walk_group(std::vector<Walked<F>>& W, size_t i0, size_t i1, [[maybe_unused]] int nthr, const std::string& who, One one) {
    W.resize(i1 - i0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)W.size()))
    for (long long q = 0; q < (long long)W.size(); q++) {
        Walked<F>& x = W[q];
        x.idx = i0 + (size_t)q;
        try { one(x); } catch (const std::exception& e) { x.error = e.what(); }
    }
    for (auto& x : W)
        if (!x.error.empty()) throw Error(who + ": proof " + std::to_string(x.idx) + ": " + x.error);
}
// after the group's synchronisation: every merged proof's results (res(s): group slot s as the walk reads it), then done(x) - the
// deferred comparisons and what the entry hands back - on the host threads
template <class F, class Res, class Done> void complete_group(std::vector<Walked<F>>& W, [[maybe_unused]] int nthr, Res res, Done done) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)W.size()))
    for (long long q = 0; q < (long long)W.size(); q++) {
        Walked<F>& x = W[q];
        if (x.pend.live()) {
            x.rec->res.resize(x.gslot.size());
            for (size_t t = 0; t < x.gslot.size(); t++) x.rec->res[t] = res(x.gslot[t]);
        }
        done(x);
    }
    W.clear();
}
// group g's kernels run under the staging and the walks of group g + 1; HG_TIMES=verify: where the wall clock went, under `label`
template <class Stage, class Walk, class Launch, class Complete>
void batch_groups(hipStream_t st, const std::string& who, const char* label, bool times, double t0, size_t n, size_t ngroups, size_t G, Stage stage, Walk walk,
                  Launch launch, Complete complete) {
    stage(0);
    walk(0);
    double t_walk = omp_get_wtime() - t0, t_sync = 0;
    for (size_t g = 0; g < ngroups; g++) {
        launch(g);
        if (g + 1 < ngroups) { const double tw = omp_get_wtime(); stage(g + 1); walk(g + 1); t_walk += omp_get_wtime() - tw; }
        const double ts = omp_get_wtime();
        hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());
        hip_check(hipGetLastError(), (who + ": kernels").c_str());
        t_sync += omp_get_wtime() - ts;
        complete(g);
    }
    if (times)
        fprintf(stderr, "[hg] %s: %zu proofs in %zu groups of up to %zu: %.2f ms in all (staging and walks %.2f, waiting for the device %.2f)\n", label, n,
                ngroups, G, (omp_get_wtime() - t0) * 1e3, t_walk * 1e3, t_sync * 1e3);
}

}  // namespace hg
