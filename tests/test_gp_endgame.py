"""The end of the grand products (-m gpu): the fold-first tail (kernels.hip: k_st_tail<.., FF>) and the split rounds' sums taken in
pairs of consecutive rounds from one read (k_st_step2<SUMS>), against the CPU oracle - exact equality on every output.

Every case runs three times in one process: with both switches off, with HG_TAIL_WHOLE_ROUNDS=1 (the tail round by round, as before)
and with HG_SUMS_SINGLE=1 (one sums item per split round, as before); the library reads both at every flush. What ran is read from the
line `[hg endgame] stride tail_fold_first= tail_whole= sums_pairs= sums_singles=` (HG_DEBUG=endgame, csrc/prover_sumcheck.inc) next to
the launch plan (HG_DEBUG=plan), which must stay what test_launch_plans.py asserts whatever the switches say.

Shapes (st_tail_h and the plan words: test_launch_plans.py): the tail of (2, 13, Ext2) holds the most levels in LDS (twelve rounds; the
levels behind the first do not fit beside it, so two rounds run whole), (4, 13, base) and (6, 16, Ext2) fit them beside the first,
(100, 11, base) on edge operands has the widest dot products, (2, 2) and (2, 1) are a two-round and a one-round tail (one round to
fold first, none). Sums: (6, 16, Ext2) folds F14 .. F10 - two pairs and a single; (4, 17, Ext2) F13 .. F11 - a pair and a single;
(48, 11, base) F9 .. F7 - a pair exactly at ST_STEP2_MIN_H = 9 and a single below it, at 24 table pairs, the most that are paired
(kernels.hpp: ST_SUMS_PAIR_MAX_NB; measured, see NOTEBOOK.md); (100, 11, base) F9 .. F6 has 50 table pairs and stays four singles."""
import os
import random

import pytest

import orclib
from orclib import rand_f, edge_f
from hglib import hg
from planlib import plan_lines
from test_launch_plans import sumcheck_case, assert_sumcheck_equal, signature

pytestmark = pytest.mark.gpu

SWITCHES = {"new": {}, "tail_whole": {"HG_TAIL_WHOLE_ROUNDS": "1"}, "sums_single": {"HG_SUMS_SINGLE": "1"}}


@pytest.fixture(scope="module")
def ctx():
    c, c1 = hg.Context(0), hg.Context(0)
    c1.set_option("one_stream", 1)
    yield {"forked": c, "one_stream": c1}
    c.close()
    c1.close()


def run(capfd, monkeypatch, fn, switch, extra=""):
    """fn() under the switch -> (result, plan lines, the endgame line's fields or None, the whole stderr)"""
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HG_DEBUG", "plan,endgame" + extra)
    capfd.readouterr()
    try:
        res = fn()
    finally:
        monkeypatch.delenv("HG_DEBUG")
        for k in SWITCHES[switch]:
            monkeypatch.delenv(k)
    err = capfd.readouterr().err
    eg = plan_lines(err, "endgame")
    tot = None
    if eg:   # (one line per flush that ran a grand-product tail or sums: added up)
        tot = {k: sum(l[k] for l in eg) for k in ("tail_fold_first", "tail_whole", "sums_pairs", "sums_singles")}
    print(switch, signature([l for l in plan_lines(err, "plan") if l["what"] == "stride"]), tot)
    return res, plan_lines(err, "plan"), tot, err


def expect(switch, tot, ff, whole, pairs, singles):
    """the counts with the switches off -> what the line must say under `switch`"""
    if switch == "tail_whole":
        ff, whole = 0, ff + whole
    if switch == "sums_single":
        pairs, singles = 0, 2 * pairs + singles
    if ff + whole + pairs + singles == 0:
        assert tot is None, (switch, tot)
        return
    assert tot == {"tail_fold_first": ff, "tail_whole": whole, "sums_pairs": pairs, "sums_singles": singles}, (switch, tot)


# (kind 1: ntab, nv, base, operands) -> the forked plan, then tail jobs fold-first / whole and sums pairs / singles with the switches off
CASES = {
    (2, 13, False, "rand"): ("S12 T12", 1, 0, 0, 0),
    (4, 13, True, "rand"): ("B12 F11 M11-11x1 T11", 1, 0, 0, 1),
    (6, 16, False, "rand"): ("S15 F14 F13 F12 F11 F10 M10-14x5 T10", 1, 0, 2, 1),
    (4, 17, False, "rand"): ("S16 P15 F13 F12 F11 M11-13x3 T11", 1, 0, 1, 1),
    (100, 11, True, "edge"): ("B10 F9 F8 F7 F6 M6-9x4 T6", 1, 0, 0, 4),   # (50 table pairs: above ST_SUMS_PAIR_MAX_NB, no pair)
    (48, 11, True, "rand"): ("B10 F9 F8 F7 M7-9x3 T7", 1, 0, 1, 1),       # (24 table pairs, the most that are paired: (9, 8) and 7)
    (2, 2, True, "rand"): ("T2", 1, 0, 0, 0),
    (2, 2, False, "rand"): ("T2", 1, 0, 0, 0),
    (2, 1, True, "rand"): ("T1", 0, 1, 0, 0),
    (2, 1, False, "rand"): ("T1", 0, 1, 0, 0),
}


@pytest.mark.parametrize("ntab,nv,base,ops", list(CASES))
def test_tail_and_sums_of_one_job_bit_exact(ctx, capfd, monkeypatch, ntab, nv, base, ops):
    want, ff, whole, pairs, singles = CASES[(ntab, nv, base, ops)]
    args, exp = sumcheck_case(1, ntab, nv, base, edge_f if ops == "edge" else rand_f, 7000 + 1000 + ntab * 10 + nv)
    for switch in SWITCHES:
        got, plan, tot, _ = run(capfd, monkeypatch, lambda: ctx["forked"].sumcheck(*args), switch)
        assert_sumcheck_equal(got, exp, switch)
        assert signature(plan) == want, (switch, signature(plan))
        expect(switch, tot, ff, whole, pairs, singles)


@pytest.mark.parametrize("nb,nv,ops", [(2, 19, "rand"), (2, 19, "edge"), (3, 18, "rand")])
def test_grand_product_layers_of_every_size_in_one_tail_and_one_sums_launch(ctx, capfd, monkeypatch, nb, nv, ops):
    """Every layer (1 .. nv - 1 variables) ends in ONE tail launch, with the claim epilogue; the sums launch mixes sizes. The layer of
    one variable is a one-round tail, every other one folds first."""
    rng = random.Random(100 * nb + nv)
    gen = edge_f if ops == "edge" else rand_f
    tabs = [gen(rng, 1 << nv) for _ in range(nb)]
    skip = rng.randrange(40)
    ref, rclaims, rpoint = orclib.grand_product_f("goldilocks", tabs, skip, threads=4)
    for switch in SWITCHES:
        (proof, claims, point), plan, tot, _ = run(capfd, monkeypatch, lambda: hg.grand_product(ctx["forked"], tabs, skip), switch)
        assert proof == ref, switch
        assert [int(a) | (int(b) << 64) for a, b in claims] == rclaims, switch
        assert [int(a) | (int(b) << 64) for a, b in point] == rpoint, switch
        lines = [l for l in plan if not l.get("after_seq")]
        assert lines[-1]["tail"] == 1 and lines[-1]["items"] == nv - 1 and lines[-1]["rounds"][0] == 1, switch
        sums = [l for l in lines if l["mode"] == 2]
        assert len(sums) == 1 and sums[0]["h"][0] < sums[0]["h"][1], switch
        assert tot is not None, switch
        assert tot["tail_fold_first"] + tot["tail_whole"] == nv - 1 and 2 * tot["sums_pairs"] + tot["sums_singles"] == sums[0]["items"], (switch, tot)
        assert tot["tail_whole"] == (nv - 1 if switch == "tail_whole" else 1), (switch, tot)
        if switch == "sums_single":
            assert tot["sums_pairs"] == 0, tot
        else:
            assert tot["sums_pairs"] >= 2 and tot["sums_singles"] >= 1, (switch, tot)


FIXTURES = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55)]


def test_lasso_node_with_the_mirrored_top_layer_and_regrouped_jobs(ctx, capfd, monkeypatch):
    """The Lasso node at the smallest fixture whose walk adopts slot-form layers (`[hg slots] adopted: k layers`, k >= 1: their tails
    read tables regrouped right ahead of the launch) behind the hash-free first round of the mirrored top layer (H in the plan), on
    the forked and on the one-stream plan."""
    chosen = None
    for n, k, bits in FIXTURES:
        bfv = hg.BfvEncrypt.new(n, k)
        pk = bfv.setup(ctx["forked"])
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        lasso_in, _ = pk.circuit_eval(w)
        _, plan, _, err = run(capfd, monkeypatch, lambda: hg.LassoNode(pk).prove_claim_reduction(ctx["forked"], lasso_in), "new", ",slots")
        adopted = [int(ln.split("adopted:")[1].split()[0]) for ln in err.splitlines() if ln.startswith("[hg slots] adopted:")]
        pk.free()
        if adopted and max(adopted) >= 1 and any(l.get("hash") == 1 for l in plan):
            chosen = (n, k, bits)
            break
    assert chosen, "no fixture adopts slot-form layers"
    n, k, bits = chosen
    print("fixture", chosen)
    bfv = hg.BfvEncrypt.new(n, k)
    ref = None
    for name in ("forked", "one_stream"):
        pk = bfv.setup(ctx[name])
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        lasso_in, _ = pk.circuit_eval(w)
        if ref is None:
            ref = orclib.lasso_prove(orclib.params(n, k), lasso_in, threads=4)
        for switch in SWITCHES:
            (proof, claim), plan, tot, _ = run(capfd, monkeypatch, lambda: hg.LassoNode(pk).prove_claim_reduction(ctx[name], lasso_in), switch)
            assert proof == ref[0] and (claim == ref[1]).all(), (name, switch)
            assert any(l.get("hash") == 1 for l in plan) and any(l.get("tail") == 1 and l["kind"] == 1 for l in plan), (name, switch)
            assert tot is not None, (name, switch)
            if switch == "tail_whole":
                assert tot["tail_fold_first"] == 0 and tot["tail_whole"] >= 1, (name, switch, tot)
            else:
                assert tot["tail_fold_first"] >= 1, (name, switch, tot)
            if name == "one_stream":
                assert tot["sums_pairs"] == tot["sums_singles"] == 0, (name, switch, tot)
            else:
                split = sum(l["items"] for l in plan if l.get("mode") == 2)
                assert split >= 1 and 2 * tot["sums_pairs"] + tot["sums_singles"] == split, (name, switch, tot)
                assert switch != "sums_single" or tot["sums_pairs"] == 0, (name, switch, tot)
        pk.free()
