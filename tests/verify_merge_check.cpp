// Host check of csrc/verifier_merge.hpp (compiled and run by tests/test_verify_batch_sharing.py): hand-made records, made through the
// recording backend's own calls, merged as a group - what is shared, what never is, the shift of own chains, a rejected proof, the slots.
// No device call: only the recorder and merge_group are instantiated.
#include <cstdio>
#include <set>
#include "verifier_merge.hpp"

using namespace hg;

// (the one constructor of Params lives in host.cpp, which this program does not link: the same few lines, without the range checks)
hg::Params::Params(const hg_params& p) : raw(p) {
    n_log2 = __builtin_ctz(p.n);
    L = n_log2 + 1;
    k = (int)p.k;
    log2k = __builtin_ctz(p.k);
}

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

typedef RecBackendT<E2> Rec;
typedef VerifyBackendT<E2>::ClaimOffs ClaimOffs;

// a key with three nodes: 0 a Vanilla node of arity 2 whose input 0 has a linear and input 1 a right-operand wiring, 1 an FFT node,
// 2 an input; n = 8, k = 1 (L = 4)
static const u32 some_ptr[1] = {0};
static hg_pk* make_key() {
    hg_params raw;
    memset(&raw, 0, sizeof(raw));
    raw.n = 8; raw.k = 1;
    hg_pk* pk = new hg_pk(raw);
    HNode v;
    v.kind = NK_VANILLA; v.arity = 2; v.log2_sub_in = 2; v.log2_sub_out = 2; v.log2_reps = 1;
    v.left_use = {1, 0}; v.right_use = {0, 1};
    HNode f;
    f.kind = NK_FFT; f.log2_size = 3;
    HNode in;
    in.kind = NK_INPUT; in.log2_size = 4;
    pk->circuit.nodes = {v, f, in};
    pk->node_dev.resize(3);
    pk->node_dev[0].lin.resize(2);
    pk->node_dev[0].mulR.resize(2);
    memset(pk->node_dev[0].lin.data(), 0, 2 * sizeof(dev::CsrLin));
    memset(pk->node_dev[0].mulR.data(), 0, 2 * sizeof(dev::CsrMul));
    pk->node_dev[0].lin[0].ptr = some_ptr;
    pk->node_dev[0].mulR[1].ptr = some_ptr;
    return pk;
}

// one walk's calls: the Vanilla node with two claims (points at `at` and at + 3, alphas at + 6), its constant sum, phase 1 at
// at + 8, phase 2 at at + 11 with evaluations u, then the FFT node with one claim at at + 14 and its point at at + 17, then input 0
// and ct0is at at + 20. Slots in call order: const 0, lin dot 1, mul dot 2, fft dot 3, input 4, ct0is 5; chain_need = at + 24.
static void record(Walked<E2>& x, const hg_pk* pk, size_t at, u64 u0, size_t chain_len) {
    x.rec.reset(new Rec(pk, false, false));
    Rec& R = *x.rec;
    ClaimOffs two;
    two.point_off = {at, at + 3}; two.alpha_off = at + 6; two.unit = false;
    R.begin_node(0, two);
    CHECK(R.const_sum() == 0);
    R.set_x(at + 8);
    const std::vector<int> lt = R.lin_terms();
    CHECK(lt.size() == 2 && lt[0] == 1 && lt[1] == -1);
    R.set_y(at + 11, {e2(u0, 0), e2(u0 + 1, 0)});
    const std::vector<int> mt = R.mul_terms();
    CHECK(mt.size() == 2 && mt[0] == -1 && mt[1] == 2);
    R.end_node();
    ClaimOffs one;
    one.point_off = {at + 14};
    R.begin_node(1, one);
    R.set_x(at + 17);
    CHECK(R.fft_term() == 3);
    R.end_node();
    CHECK(R.mle_input(0, at + 20, 4) == 4);
    CHECK(R.mle_ct0is(at + 20, 4) == 5);
    CHECK(R.nslots == 6 && R.chain_need == at + 24);
    for (size_t i = 0; i < chain_len; i++) x.pend.chain.push_back(e2(1000 * (u0 + 1) + i, 0));
}

static bool all_set(const Walked<E2>& x, int nslot) {
    if (x.gslot.size() != (size_t)x.rec->nslots) return false;
    for (int s : x.gslot)
        if (s < 0 || s >= nslot) return false;
    return true;
}
static size_t distinct(const std::vector<Walked<E2>>& W) {
    std::set<int> s;
    for (auto& x : W) s.insert(x.gslot.begin(), x.gslot.end());
    return s.size();
}

int main() {
    hg_pk* pk = make_key();
    // ---- one chain for all: equal jobs become one, muls and inputs never
    {
        std::vector<Walked<E2>> W(2);
        record(W[0], pk, 0, 7, 0);
        record(W[1], pk, 0, 9, 0);
        const MergedGroup<E2> M = merge_group(W, false);
        // eq tables of one proof: the node's, x, y, the FFT node's x, and ONE for the input point (input 0 and ct0is: same size, same point)
        CHECK(M.eqs.size() == 5 && M.consts.size() == 1 && M.lins.size() == 1 && M.ffts.size() == 1);
        CHECK(M.muls.size() == 2 && M.ins.size() == 4);
        CHECK(M.dots.size() == 4);   // lin, fft, and a mul dot per proof
        CHECK(M.chain.empty() && M.chain_need == 24);
        CHECK(M.us.size() == 4 && M.us[0].c0 == 7 && M.us[2].c0 == 9 && M.muls[0].u_at == 0 && M.muls[1].u_at == 2);
        CHECK(all_set(W[0], M.nslot) && all_set(W[1], M.nslot));
        for (int s : {0, 1, 3}) CHECK(W[0].gslot[s] == W[1].gslot[s]);   // const, lin dot, fft dot: the same slot
        for (int s : {2, 4, 5}) CHECK(W[0].gslot[s] != W[1].gslot[s]);   // mul dot, the inputs: each its own
        CHECK(M.nslot == 9 && distinct(W) == 9);
        // the merge order is the walks': proof 0's slots in call order, then what proof 1 adds
        const int want0[6] = {0, 1, 2, 3, 4, 5}, want1[6] = {0, 1, 6, 3, 7, 8};
        for (int s = 0; s < 6; s++) CHECK(W[0].gslot[s] == want0[s] && W[1].gslot[s] == want1[s]);
        CHECK(M.eqs[0].n == 3 && M.eqs[0].cs.n == 2 && M.eqs[0].cs.point_off[1] == 3 && M.eqs[0].cs.alpha_off == 6);
        CHECK(M.ins[0].w == 0 && M.ins[1].k == -1 && M.ins[2].w == 1 && M.ins[2].eq == M.ins[0].eq);
        CHECK(M.muls[0].eqc == M.muls[1].eqc && M.muls[0].eqx == M.muls[1].eqx && M.dots[1].kind == Rec::D_MUL && M.dots[1].tab == 0 && M.dots[3].kind == Rec::D_MUL && M.dots[3].tab == 1);
    }
    // ---- the same two at other offsets of the one chain share nothing but what does not read it
    {
        std::vector<Walked<E2>> W(2);
        record(W[0], pk, 0, 7, 0);
        record(W[1], pk, 100, 7, 0);
        const MergedGroup<E2> M = merge_group(W, false);
        CHECK(M.eqs.size() == 10 && M.consts.size() == 2 && M.lins.size() == 2 && M.ffts.size() == 2 && M.dots.size() == 6);
        CHECK(M.chain_need == 124 && M.nslot == 12 && distinct(W) == 12);
    }
    // ---- own chains: equal local offsets, shifted by each proof's base - nothing is shared
    {
        std::vector<Walked<E2>> W(3);
        record(W[0], pk, 0, 7, 30);
        record(W[1], pk, 0, 7, 40);
        record(W[2], pk, 0, 7, 30);
        const MergedGroup<E2> M = merge_group(W, true);
        CHECK(M.chain.size() == 100 && M.chain[0].c0 == 8000 && M.chain[30].c0 == 8000 && M.chain[69].c0 == 8039 && M.chain[70].c0 == 8000);
        CHECK(M.eqs.size() == 15 && M.consts.size() == 3 && M.lins.size() == 3 && M.muls.size() == 3 && M.ffts.size() == 3);
        CHECK(M.dots.size() == 9 && M.ins.size() == 6);
        CHECK(M.nslot == 18 && distinct(W) == 18);
        for (auto& x : W) CHECK(all_set(x, M.nslot));
        const size_t base[3] = {0, 30, 70};
        for (int w = 0; w < 3; w++) {
            const auto& e = M.eqs[5 * w];   // the Vanilla node's eq table of proof w
            CHECK(e.cs.n == 2 && e.cs.point_off[0] == base[w] && e.cs.point_off[1] == base[w] + 3 && e.cs.alpha_off == base[w] + 6);
            CHECK(M.eqs[5 * w + 1].cs.unit_alpha == 1 && M.eqs[5 * w + 1].cs.point_off[0] == base[w] + 8);
            CHECK(M.ffts[w].cs.n == 1 && M.ffts[w].cs.point_off[0] == base[w] + 14);
            for (int s = 0; s < 6; s++) CHECK(W[w].gslot[s] == 6 * w + s);
        }
    }
    // ---- a proof the walk rejected contributes nothing, wherever it stands
    for (int pos = 0; pos < 3; pos++) {
        std::vector<Walked<E2>> W(3);
        for (int w = 0; w < 3; w++) record(W[w], pk, 0, 7 + w, 0);
        W[pos].pend.reason = "rejected";
        const MergedGroup<E2> M = merge_group(W, false);
        CHECK(M.eqs.size() == 5 && M.consts.size() == 1 && M.muls.size() == 2 && M.ins.size() == 4 && M.dots.size() == 4 && M.us.size() == 4);
        CHECK(M.nslot == 9 && distinct(W) == 9 && W[pos].gslot.empty());
        const int a = pos == 0 ? 1 : 0, b = pos == 2 ? 1 : 2;   // the two that are merged, in order
        const int want0[6] = {0, 1, 2, 3, 4, 5}, want1[6] = {0, 1, 6, 3, 7, 8};
        for (int s = 0; s < 6; s++) CHECK(W[a].gslot[s] == want0[s] && W[b].gslot[s] == want1[s]);
        for (auto& in : M.ins) CHECK(in.w != (size_t)pos);
        CHECK(M.us[0].c0 == (u64)(7 + a) && M.us[2].c0 == (u64)(7 + b));
    }
    // ---- the checks of one field only, and the public form's
    {
        Rec gl(pk, false, false), fr(pk, false, true), pub(pk, true, true);
        auto thrown = [](auto fn) -> std::string { try { fn(); } catch (const Error& e) { return e.what(); } return ""; };
        CHECK(thrown([&] { gl.mle_input(0, 0, 3); }) == "");
        CHECK(thrown([&] { fr.mle_input(0, 0, 3); }) == "verifier: claim point does not fit the input table");
        CHECK(thrown([&] { fr.mle_input(0, 0, 4); }) == "");
        CHECK(thrown([&] { gl.mle_input(6, 0, 4); }) == "verifier: no such input table");
        CHECK(thrown([&] { fr.mle_input(6, 0, 4); }) == "verifier: no such input table");
        CHECK(thrown([&] { pub.mle_input(0, 0, 4); }) == "verifier: input 0 is not a public table");
        CHECK(thrown([&] { pub.mle_input(3, 0, 3); }) == "verifier: a point of the wrong length for a public table");
        CHECK(thrown([&] { pub.mle_ct0is(0, 5); }) == "verifier: a point of the wrong length for a public table");
        CHECK(thrown([&] { pub.mle_ct0is(0, 4); }) == "" && thrown([&] { pub.mle_input(3, 0, 4); }) == "");
    }
    delete pk;
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
