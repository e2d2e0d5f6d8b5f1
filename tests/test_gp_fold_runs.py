"""The fold-only rounds of the grand products as runs (-m gpu): all fold-only rounds of a job in one item of one launch
(kernels.hip: k_st_fold_runs, kernels.hpp: StFoldRun), against the CPU oracle - exact equality on every output.

Every case runs three times in one process: as runs at the default tile, with HG_FOLD_ROUNDS=1 (one launch per round, as before) and
with a shrunken tile (HG_FOLD_TILE_LOG2: a run longer than a tile of 2^p pair indices holds, p + 1 rounds, is cut into consecutive
launches, and a table has many tiles); the library reads both at every flush. What ran is read from the line
`[hg folds] stride launches= items= rounds= max_run= tile_log2=` (HG_DEBUG=folds, csrc/prover_sumcheck.inc) next to the launch plan
(HG_DEBUG=plan), which must be the same under all three: an `F<h>` word is a round of the fold-run launch. `rounds` must equal the
items of the plan's `F` lines; under HG_FOLD_ROUNDS=1 no such line appears.

Shapes (st_tail_h and the plan words: test_launch_plans.py): see CASES."""
import os
import random

import numpy as np
import pytest

import orclib
from orclib import P, rand_f, edge_f
from hglib import hg
from planlib import plan_lines
from test_launch_plans import sumcheck_case, assert_sumcheck_equal, signature
from test_gp_endgame import FIXTURES

pytestmark = pytest.mark.gpu

DEFAULT_TILE = 9


@pytest.fixture(scope="module")
def ctx():
    c, c1 = hg.Context(0), hg.Context(0)
    c1.set_option("one_stream", 1)
    yield {"forked": c, "one_stream": c1}
    c.close()
    c1.close()


def np_f(rng, n):
    """uniform field elements from a numpy generator seeded by the case's rng (the long tables)"""
    return np.random.default_rng(rng.randrange(1 << 32)).integers(0, P, size=n, dtype=np.uint64)


def run(capfd, monkeypatch, fn, env):
    """fn() under the environment `env` -> (result, stride plan lines, the [hg folds] lines)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("HG_DEBUG", "plan,folds")
    capfd.readouterr()
    try:
        res = fn()
    finally:
        monkeypatch.delenv("HG_DEBUG")
        for k in env:
            monkeypatch.delenv(k)
    err = capfd.readouterr().err
    plan = [l for l in plan_lines(err, "plan") if l["what"] == "stride"]
    folds = plan_lines(err, "folds")
    print(env, signature(plan), [l["line"] for l in folds])
    return res, plan, folds


def settings(tile):
    return {"runs": {}, "per_round": {"HG_FOLD_ROUNDS": "1"}, "tile%d" % tile: {"HG_FOLD_TILE_LOG2": str(tile)}}


def f_items(plan):
    return sum(l["items"] for l in plan if l.get("mode") == 1)


def pieces(hs, tile):
    """launches a run of fold-only rounds at half lengths 2^hs[0], 2^hs[1], .. is cut into: a piece that starts at h holds
    min(tile, h) + 1 rounds (a tile of 2^p pair indices folds p + 1 rounds deep)"""
    n, pos = 0, 0
    while pos < len(hs):
        pos += min(tile, hs[pos]) + 1
        n += 1
    return n


def check_folds(name, folds, plan, tile, launches=None, items=None):
    """the [hg folds] line of ONE flush against its plan"""
    if name == "per_round":
        assert not folds, (name, folds)
        return
    assert len(folds) == 1, (name, folds)
    f = folds[0]
    assert f["what"] == "stride" and f["rounds"] == f_items(plan) and f["tile_log2"] == tile, (name, f)
    if launches is not None:
        assert f["launches"] == launches, (name, f)
    if items is not None:
        assert f["items"] == items, (name, f)


# (ntab, nv, base, operands) -> the fold-only rounds' half lengths (log2), the shrunken tiles to run and the launches each must take
CASES = {
    (4, 13, True, "rand"): ([11], {1: 1}),                       # the shortest run: one round
    (2, 17, True, "rand"): ([13, 12], {1: 1}),                   # behind a fused pair, two tables
    (4, 17, False, "rand"): ([13, 12, 11], {1: 2}),              # behind a fused pair
    (6, 16, False, "rand"): ([14, 13, 12, 11, 10], {1: 3, 3: 2}),   # 32 tiles per table at the default tile
    (48, 11, True, "rand"): ([9, 8, 7], {2: 1}),                 # 24 table pairs
    (100, 11, True, "edge"): ([9, 8, 7, 6], {3: 1}),             # one tile exactly: 2^h0 = P
    (100, 10, True, "rand"): ([8, 7, 6], {1: 2}),                # 2^h0 < P: a workgroup holds a whole table
    (100, 16, True, "np"): ([14, 13, 12, 11, 10, 9, 8, 7, 6], {3: 3}),   # 9 rounds, the workload's longest: ONE launch at the default tile
}
GENS = {"rand": rand_f, "edge": edge_f, "np": np_f}


@pytest.mark.parametrize("ntab,nv,base,ops", list(CASES))
def test_fold_runs_of_one_job_bit_exact(ctx, capfd, monkeypatch, ntab, nv, base, ops):
    hs, tiles = CASES[(ntab, nv, base, ops)]
    args, exp = sumcheck_case(1, ntab, nv, base, GENS[ops], 7000 + 1000 + ntab * 10 + nv)
    sigs = {}
    for tile, launches in tiles.items():
        assert launches == pieces(hs, tile) and pieces(hs, DEFAULT_TILE) == 1
        for name, env in settings(tile).items():
            if name in sigs:
                continue   # (a second shrunken tile: the other two settings ran already)
            got, plan, folds = run(capfd, monkeypatch, lambda: ctx["forked"].sumcheck(*args), env)
            assert_sumcheck_equal(got, exp, name)
            sigs[name] = signature(plan)
            assert [w for w in sigs[name].split() if w[0] == "F"] == ["F%d" % h for h in hs], (name, sigs[name])
            assert f_items(plan) == len(hs), name
            if name == "runs":
                check_folds(name, folds, plan, DEFAULT_TILE, launches=1, items=1)
                assert folds[0]["max_run"] == len(hs), folds
            else:
                check_folds(name, folds, plan, tile, launches=launches)
    assert len(set(sigs.values())) == 1, sigs


@pytest.mark.parametrize("nb,nv,ops", [(2, 19, "rand"), (2, 19, "edge"), (3, 18, "rand")])
def test_grand_product_layers_of_every_size_as_items_of_one_launch(ctx, capfd, monkeypatch, nb, nv, ops):
    """Every layer with a fold-only round is one item of the launch, each with its own run length."""
    rng = random.Random(100 * nb + nv)
    gen = edge_f if ops == "edge" else rand_f
    tabs = [gen(rng, 1 << nv) for _ in range(nb)]
    skip = rng.randrange(40)
    ref, rclaims, rpoint = orclib.grand_product_f("goldilocks", tabs, skip, threads=4)
    sigs = {}
    for name, env in settings(2).items():
        (proof, claims, point), plan, folds = run(capfd, monkeypatch, lambda: hg.grand_product(ctx["forked"], tabs, skip), env)
        assert proof == ref, name
        assert [int(a) | (int(b) << 64) for a, b in claims] == rclaims, name
        assert [int(a) | (int(b) << 64) for a, b in point] == rpoint, name
        sigs[name] = signature(plan)
        fl = [l for l in plan if l.get("mode") == 1]
        assert len(fl) >= 2 and any(l["h"][0] < l["h"][1] for l in fl), name
        # The run of the layer of L variables (2 nb tables; test_launch_plans.py): the tail takes the rounds from h = hs down, the first
        # round is h = L - 1, pairs of rounds are fused while h >= 15, and what is left down to hs + 1 is fold-only.
        hs = 1 + int(np.log2(2560 // (2 * nb)))
        want = []
        for L in range(1, nv):
            h = L - 2
            while h >= 15 and h - 1 > hs:
                h -= 2
            if h > hs:
                want.append(h - hs)
        assert sum(want) == f_items(plan) and len(want) >= 2 and len(set(want)) >= 2, (name, want, f_items(plan))
        if name == "runs":
            check_folds(name, folds, plan, DEFAULT_TILE, launches=1, items=len(want))
            assert folds[0]["max_run"] == max(want), folds
        elif name == "per_round":
            check_folds(name, folds, plan, DEFAULT_TILE)
        else:   # (tile 2: three rounds a piece)
            check_folds(name, folds, plan, 2, launches=max((r + 2) // 3 for r in want), items=sum((r + 2) // 3 for r in want))
    assert len(set(sigs.values())) == 1, sigs


def test_lasso_node_mirrored_top_layer_and_slot_form_jobs(ctx, capfd, monkeypatch):
    """The Lasso node at the smallest fixture whose walk adopts slot-form layers: the mirrored top layer (an odd table count: its S
    table is folded like any other) and slot-form jobs regrouped ahead of the tail, on the forked context; the one-stream plan has no
    fold-only round."""
    chosen = None
    for n, k, bits in FIXTURES:
        bfv = hg.BfvEncrypt.new(n, k)
        pk = bfv.setup(ctx["forked"])
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        lasso_in, _ = pk.circuit_eval(w)
        monkeypatch.setenv("HG_DEBUG", "plan,slots")
        capfd.readouterr()
        try:
            hg.LassoNode(pk).prove_claim_reduction(ctx["forked"], lasso_in)
        finally:
            monkeypatch.delenv("HG_DEBUG")
        err = capfd.readouterr().err
        adopted = [int(ln.split("adopted:")[1].split()[0]) for ln in err.splitlines() if ln.startswith("[hg slots] adopted:")]
        pk.free()
        if adopted and max(adopted) >= 1 and any(l.get("hash") == 1 for l in plan_lines(err, "plan")):
            chosen = (n, k, bits)
            break
    assert chosen, "no fixture adopts slot-form layers"
    n, k, bits = chosen
    print("fixture", chosen)
    bfv = hg.BfvEncrypt.new(n, k)
    ref = None
    for cname in ("forked", "one_stream"):
        pk = bfv.setup(ctx[cname])
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        lasso_in, _ = pk.circuit_eval(w)
        if ref is None:
            ref = orclib.lasso_prove(orclib.params(n, k), lasso_in, threads=4)
        sigs = {}
        for name, env in settings(2).items():
            (proof, claim), plan, folds = run(capfd, monkeypatch, lambda: hg.LassoNode(pk).prove_claim_reduction(ctx[cname], lasso_in), env)
            assert proof == ref[0] and (claim == ref[1]).all(), (cname, name)
            sigs[name] = [l["line"] for l in plan]
            if cname == "one_stream" or name == "per_round":
                assert not folds, (cname, name, folds)
                assert cname == "forked" or f_items(plan) == 0, (cname, name)
            else:
                assert folds and sum(f["rounds"] for f in folds) == f_items(plan) >= 1, (cname, name, folds)   # (one line per flush that issued a run)
                assert all(f["tile_log2"] == (DEFAULT_TILE if name == "runs" else 2) for f in folds), folds
                if name == "runs":
                    assert all(f["launches"] == 1 for f in folds), folds
        assert sigs["runs"] == sigs["per_round"] == sigs["tile2"], cname
        pk.free()


def test_graph_replays_equal_the_walk_with_one_launch_per_round(capfd, monkeypatch):
    """Three proves of one values object at the smallest golden fixture (walk, walk, capture and replay): the bytes of each equal
    the proof walked with HG_FOLD_ROUNDS=1. A context of its own: the graph is recorded with the runs."""
    n, k, bits = FIXTURES[0]
    c = hg.Context(0)
    try:
        bfv = hg.BfvEncrypt.new(n, k)
        pk = bfv.setup(c)
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        vals = hg.witness_gen(c, pk, w)
        out = hg.ProofBuffer()
        c.set_option("graph", 0)
        walked, plan, folds = run(capfd, monkeypatch, lambda: hg.prove_resident(c, pk, vals, out).bytes(), {"HG_FOLD_ROUNDS": "1"})
        c.set_option("graph", 1)
        assert f_items(plan) >= 1 and not folds, folds
        proofs = []
        for i in range(3):
            got, _, folds = run(capfd, monkeypatch, lambda: hg.prove_resident(c, pk, vals, out).bytes(), {})
            proofs.append(got)
            assert i == 2 or folds, i   # (the walks print their flushes; a replay walks nothing)
        assert all(p == walked for p in proofs), [p == walked for p in proofs]
        vals.free()
        pk.free()
    finally:
        c.close()
