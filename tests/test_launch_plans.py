"""Kernel-level sum-check tests that reach every launch path of the two planners and show that it ran (-m gpu).

Each case compares the HIP entry (hg_sumcheck, hg_grand_product, hg_lasso_prove_at) with the CPU oracle, exact equality on every output, and
reads the launch plan the library printed (HG_DEBUG=plan, csrc/prover_sumcheck.inc): a case whose named launch did not occur fails.
The stride-planner cases run on two contexts: the default one builds the forked plan a prove builds (small grand-product rounds split:
folds `mode=1` on the main stream, all their sums in one `mode=2` pass on the sums stream), `one_stream = 1` the unforked plan.

A plan is asserted as its signature, one word per launch in launch order:
  stride   B<h> first round on base-field rows, S<h> whole single round, P<h> fused pair of rounds (h, h - 1), F<h> fold-only round,
           M<lo>-<hi>x<items> the split rounds' sums, T<rounds> the tail (every remaining round in one launch); h = log2 of the half length;
           a launch that mixes jobs of several sizes shows <lo>-<hi>; Lasso node only: H<h> the hash-free first round, A the tree levels
           built between the sequenced first rounds and the rest
  prodsum  S<rd>@<h> single round, P<rd>@<h> fused pair (rd, rd + 1), T<tail_rd> the tail
The shapes are the smallest that reach each path: kernels.hip st_tail_h(ntab, nv) = min(nv - 1, 1 + floor(log2(2560 / ntab))) rounds-in-LDS
limit (11 for two tables, 10 for three or four, 9 for six), fused stride pairs from half = 2^15 behind the first round, split rounds at
half <= 2^14, PRODSUM tail from 4096 (pair, j) items down and fused PRODSUM pairs from half = 2^9."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import orclib
from orclib import P, ptr, rand_f, edge_f, oracle_sumcheck
from hglib import hg
import planlib
from planlib import plan_lines, show_plans   # noqa: F401  (show_plans: the autouse fixture that prints what each test read)

pytestmark = pytest.mark.gpu

PLANS = ("forked", "one_stream")


@pytest.fixture(scope="module")
def ctx():
    """The two contexts every stride-planner case runs on: {"forked": default context, "one_stream": one_stream = 1}."""
    c, c1 = hg.Context(0), hg.Context(0)
    c1.set_option("one_stream", 1)
    yield {"forked": c, "one_stream": c1}
    c.close()
    c1.close()


# ---- the plan lines -----------------------------------------------------------------------------------------------------------

def _rng(lo_hi):
    lo, hi = lo_hi
    return str(lo) if lo == hi else "%d-%d" % (lo, hi)


def signature(plan):
    sig = []
    for l in plan:
        if l["what"] == "prodsum":
            if l["ptail"]:
                sig.append("T" + _rng(l["tail_rd"]))
            else:
                assert l["cnt"] == len(l["h"]) == 1 and l["eq"] == 0, l["line"]   # (one job per call here, never the eq-factored form)
                sig.append("%s%s@%d" % ("P" if l["two"] else "S", _rng(l["rd"]), l["h"][0]))
            continue
        if l.get("after_seq"):
            sig.append("A")
        elif l["tail"]:
            sig.append("T" + _rng(l["rounds"]))
        elif l["mode"] == 2:
            sig.append("M%d-%dx%d" % (l["h"][0], l["h"][1], l["items"]))
        elif l["hash"]:
            sig.append("H" + _rng(l["h"]))
        else:
            assert l["nrounds"] in (1, 2) and not (l["nrounds"] == 2 and (l["base"] or l["mode"])), l["line"]
            sig.append(("P" if l["nrounds"] == 2 else "B" if l["base"] else "F" if l["mode"] == 1 else "S") + _rng(l["h"]))
    return " ".join(sig)


def planned(capfd, monkeypatch, fn, label=""):
    """Runs fn() with HG_DEBUG=plan and returns (its result, the plan lines it printed); the signature is shown next to the label."""
    return planlib.planned(capfd, monkeypatch, fn, label, describe=signature)


# ---- operands -----------------------------------------------------------------------------------------------------------------

def e2_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def sumcheck_case(kind, ntab, nv, base, gen, seed):
    """Tables, powers, claim and chain position of one hg_sumcheck case, and the oracle's outputs (computed once per case)."""
    rng = random.Random(seed)
    N = 1 << nv
    is_base = [i % 2 == 0 for i in range(ntab)] if kind == 2 else [base] * ntab
    tables = [gen(rng, N if b else 2 * N) for b in is_base]
    if kind == 0:
        pw = np.array([[pow(65536, i, P), 0] for i in range(ntab)], dtype=np.uint64)
    elif kind == 1:   # pw[i] = gamma^i in GoldilocksExt2 (X^2 = 7); edge cases: both coordinates of gamma from the pool (not 0: the
        g = (0, 0)    # final evaluations are unscaled by 1 / gamma^i)
        while g == (0, 0):
            g = tuple(int(x) for x in gen(rng, 2)) if gen is edge_f else (rng.randrange(P), rng.randrange(P))
        cur, pws = (1, 0), []
        for _ in range(ntab // 2):
            pws.append(cur)
            cur = e2_mul(cur, g)
        pw = np.array(pws, dtype=np.uint64)
    else:
        pw = np.zeros((0, 2), dtype=np.uint64)
    claim = np.array([rng.randrange(P), rng.randrange(P)], dtype=np.uint64)   # (arbitrary: eval(1) of a round is claim - eval(0))
    skip = rng.randrange(50)
    args = (kind, tables, is_base, pw, claim, skip)
    return args, oracle_sumcheck(*args, threads=4)


def assert_sumcheck_equal(got, exp, what):
    for name, g_, e_ in zip(("msgs", "point", "evals", "sums"), got, exp):
        assert (g_ == e_).all(), (what, name)


# ---- stride planner (collation, grand-product layers): hg_sumcheck kinds 0 and 1 -----------------------------------------------
# (kind, ntab, nv, base) -> the plan on the forked context, the plan with one_stream. Two rows sit one nv above the issue's hand
# derivation, which took st_tail_h one too small: (1, 4, 12, base) and (1, 2, 12, Ext2) go B11 T11 and T12 - no round between the first
# one and the tail, no single round at all - so the split rounds of a short job are asserted at (1, 4, 13) and the one-single-round
# boundary at (1, 2, 13).
STRIDE = {
    # one fused pair at h = 15 on Ext2 input, single rounds below it, tail
    (1, 4, 17, False): ("S16 P15 F13 F12 F11 M11-13x3 T11", "S16 P15 S13 S12 S11 T11"),
    # base first round, then the same fused pair
    (1, 2, 17, True): ("B16 P15 F13 F12 M12-13x2 T12", "B16 P15 S13 S12 T12"),
    # the collation fused pair (never split)
    (0, 3, 17, True): ("B16 P15 S13 S12 S11 T11", "B16 P15 S13 S12 S11 T11"),
    # two fused pairs in sequence
    (1, 2, 19, True): ("B18 P17 P15 F13 F12 M12-13x2 T12", "B18 P17 P15 S13 S12 T12"),
    # no pair: every round behind the first one split / whole
    (1, 6, 16, False): ("S15 F14 F13 F12 F11 F10 M10-14x5 T10", "S15 S14 S13 S12 S11 S10 T10"),
    # split rounds on a short job
    (1, 4, 13, True): ("B12 F11 M11-11x1 T11", "B12 S11 T11"),
    # exactly one single round (the first: never split, never paired), then the tail
    (1, 2, 13, False): ("S12 T12", "S12 T12"),
    # the widest dot products per hypercube point (edge operands only)
    (1, 100, 11, True): ("B10 F9 F8 F7 F6 M6-9x4 T6", "B10 S9 S8 S7 S6 T6"),
    (0, 25, 12, True): ("B11 S10 S9 S8 T8", "B11 S10 S9 S8 T8"),
}
STRIDE_RAND = [k for k in STRIDE if k[1] < 25]
STRIDE_EDGE = [(1, 4, 17, False), (1, 2, 17, True), (0, 3, 17, True), (1, 100, 11, True), (0, 25, 12, True)]


def check_stride_case(ctx, capfd, monkeypatch, key, gen):
    kind, ntab, nv, base = key
    args, exp = sumcheck_case(kind, ntab, nv, base, gen, 7000 + kind * 1000 + ntab * 10 + nv)
    sigs = {}
    for name, want in zip(PLANS, STRIDE[key]):
        got, plan = planned(capfd, monkeypatch, lambda: ctx[name].sumcheck(*args), name)
        assert_sumcheck_equal(got, exp, name)
        assert plan and all(l["what"] == "stride" and l["kind"] == kind for l in plan), name
        sigs[name] = signature(plan)
        assert sigs[name] == want, (name, sigs[name])
    return sigs


@pytest.mark.parametrize("kind,ntab,nv,base", STRIDE_RAND)
def test_stride_planner_paths_bit_exact(ctx, capfd, monkeypatch, kind, ntab, nv, base):
    """Random tables (rand_f) through every path of flush_stride, on the forked and the unforked plan: outputs equal to the oracle's,
    and the plan printed is the one the row names."""
    check_stride_case(ctx, capfd, monkeypatch, (kind, ntab, nv, base), rand_f)


@pytest.mark.parametrize("kind,ntab,nv,base", STRIDE_EDGE)
def test_stride_rounds_on_edge_operands(ctx, capfd, monkeypatch, kind, ntab, nv, base):
    """Every table entry (and gamma) an edge value of the field reductions: in the unfolded first round edge meets edge, which random
    tables with a few edge values sprinkled in never produce. Same paths, same exact comparison."""
    check_stride_case(ctx, capfd, monkeypatch, (kind, ntab, nv, base), edge_f)


# ---- PRODSUM planner: hg_sumcheck kind 2 --------------------------------------------------------------------------------------
PRODSUM = {
    (2, 14): "S0@13 T1",            # tail_rd = 1: one single-round launch on base-field input, then the tail
    (4, 15): "P0@14 S2@12 T3",      # tail_rd = 3: fused pair at rounds 0 and 1, single round 2 on Ext2 input, then the tail
    (54, 9): "S0@8 T1",             # single round below the fuse threshold, 27 pairs
    (64, 10): "P0@9 T2",            # the largest pair count, fused pair exactly at h = 9
    (2, 16): "P0@15 S2@13 T3",      # long tables: fused pair, single round, tail
    (54, 8): "T0",                  # (edge operands only) 27 products per hypercube point, everything in the tail
}


def check_prodsum_case(ctx, capfd, monkeypatch, ntab, nv, gen):
    args, exp = sumcheck_case(2, ntab, nv, None, gen, 9000 + ntab * 10 + nv)
    got, plan = planned(capfd, monkeypatch, lambda: ctx["forked"].sumcheck(*args), "forked")
    assert_sumcheck_equal(got, exp, (ntab, nv))
    assert plan and all(l["what"] == "prodsum" for l in plan)
    assert signature(plan) == PRODSUM[(ntab, nv)], signature(plan)


@pytest.mark.parametrize("ntab,nv", [(2, 14), (4, 15), (54, 9), (64, 10), (2, 16)])
def test_prodsum_planner_paths_bit_exact(ctx, capfd, monkeypatch, ntab, nv):
    """The single-round PRODSUM kernel (ps_round with two == false) on base-field and on folded Ext2 input, beside the fused pair and the tail."""
    check_prodsum_case(ctx, capfd, monkeypatch, ntab, nv, rand_f)


@pytest.mark.parametrize("ntab,nv", [(2, 14), (4, 15), (54, 8)])
def test_prodsum_rounds_on_edge_operands(ctx, capfd, monkeypatch, ntab, nv):
    check_prodsum_case(ctx, capfd, monkeypatch, ntab, nv, edge_f)


# ---- mixed launches: hg_grand_product -----------------------------------------------------------------------------------------
def check_grand_product(ctx, capfd, monkeypatch, nb, nv, gen, plans):
    """All layers (1 .. nv - 1 variables, 2 nb tables each) are queued in one flush: launch k runs every layer's next round(s)."""
    rng = random.Random(100 * nb + nv)
    tabs = [gen(rng, 1 << nv) for _ in range(nb)]
    skip = rng.randrange(40)
    ref, rclaims, rpoint = orclib.grand_product_f("goldilocks", tabs, skip, threads=4)
    out = {}
    for name in plans:
        (proof, claims, point), plan = planned(capfd, monkeypatch, lambda: hg.grand_product(ctx[name], tabs, skip), name)
        assert proof == ref, name
        assert [int(a) | (int(b) << 64) for a, b in claims] == rclaims, name
        assert [int(a) | (int(b) << 64) for a, b in point] == rpoint, name
        assert plan and all(l["what"] == "stride" and l["kind"] == 1 for l in plan), name
        lines = [l for l in plan if not l.get("after_seq")]
        pairs = [l for l in lines if l["nrounds"] == 2]
        assert pairs and all(l["h"][0] >= 15 for l in pairs), name
        # the first-round launch holds every layer above the tail's size, the tail every layer
        assert lines[0]["base"] == 1 and lines[0]["h"][1] == nv - 2 and lines[0]["items"] > 1, name
        assert lines[-1]["tail"] == 1 and lines[-1]["items"] == nv - 1 and lines[-1]["rounds"][0] == 1, name
        folds, sums = [l for l in lines if l["mode"] == 1], [l for l in lines if l["mode"] == 2]
        if name == "forked":
            assert folds and len(sums) == 1 and sums[0]["items"] == sum(l["items"] for l in folds), name
            assert any(l["h"][0] < l["h"][1] for l in folds), name   # a split launch that mixes layers of several sizes
        else:
            assert not folds and not sums, name
        out[name] = pairs
    return out


def test_grand_product_mixed_fused_pairs_and_split_rounds(ctx, capfd, monkeypatch):
    """nb = 2, nv = 19: the layers of 18 and 17 variables share a fused-pair launch (h = 16 and 15). (At nv = 18, the issue's shape,
    only the 17-variable layer has a round behind its first at half >= 2^15: its fused pair is alone in its launch - the case below.)"""
    pairs = check_grand_product(ctx, capfd, monkeypatch, 2, 19, rand_f, PLANS)
    for name in PLANS:
        assert any(l["items"] > 1 and l["h"][0] < l["h"][1] for l in pairs[name]), name


def test_grand_product_three_tables_unforked(ctx, capfd, monkeypatch):
    check_grand_product(ctx, capfd, monkeypatch, 3, 18, rand_f, ("one_stream",))


def test_grand_product_on_edge_operands(ctx, capfd, monkeypatch):
    """nb = 2, nv = 18, every entry an edge value: the 17-variable layer runs on the caller's values themselves (base first round, fused pair)."""
    check_grand_product(ctx, capfd, monkeypatch, 2, 18, edge_f, PLANS)


# ---- the Lasso node on both plans ---------------------------------------------------------------------------------------------
def test_lasso_node_on_the_forked_and_the_unforked_plan(ctx, capfd, monkeypatch):
    n, k, bits = 1024, 1, 27
    bfv = hg.BfvEncrypt.new(n, k)
    p = orclib.params(n, k)
    ref = None
    sigs = {}
    for name in PLANS:
        pk = bfv.setup(ctx[name])
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        lasso_in, _ = pk.circuit_eval(w)
        if ref is None:
            ref = orclib.lasso_prove(p, lasso_in, threads=4)
        (proof, claim), plan = planned(capfd, monkeypatch, lambda: hg.LassoNode(pk).prove_claim_reduction(ctx[name], lasso_in), name)
        assert proof == ref[0] and (claim == ref[1]).all(), name
        assert any(l["what"] == "stride" and l["kind"] == 0 for l in plan) and any(l.get("tail") == 1 and l["kind"] == 1 for l in plan), name
        modes = {l["mode"] for l in plan if "mode" in l}
        assert modes == ({0, 1, 2} if name == "forked" else {0}), (name, modes)
        sigs[name] = [l["line"] for l in plan]
        pk.free()
    assert sigs["forked"] != sigs["one_stream"]


# ---- hg_sumcheck refuses what it cannot do ------------------------------------------------------------------------------------
def raw_sumcheck(c, kind, nv, tables, is_base, pw, npw, claim):
    """hg_sumcheck as the C ABI takes it (no shape derived from the arguments): -> (return code, hg_last_error())."""
    ntab = len(tables)
    tabs = [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
    ptrs = (orclib.u64p * ntab)(*[ptr(t) for t in tabs])
    flags = (C.c_int * len(is_base))(*[int(b) for b in is_base])
    pw = np.ascontiguousarray(pw, dtype=np.uint64).reshape(-1)
    claim = np.ascontiguousarray(claim, dtype=np.uint64)
    d = 3 if kind == 1 else 2
    msgs, point = np.zeros(nv * (d + 1) * 2, dtype=np.uint64), np.zeros(nv * 2, dtype=np.uint64)
    evals, sums = np.zeros(ntab * 2, dtype=np.uint64), np.zeros(nv * d * 2, dtype=np.uint64)
    rc = hg.lib().hg_sumcheck(c.h, kind, nv, ntab, ptrs, flags, ptr(pw) if pw.size else None, npw, ptr(claim), 0,
                              ptr(msgs), ptr(point), ptr(evals), ptr(sums))
    return rc, hg.lib().hg_last_error().decode()


def test_sumcheck_entry_refuses_what_it_cannot_do(ctx, capfd, monkeypatch):
    """Every argument hg_sumcheck used to answer with a wrong result and return code 0: refused on the host (no launch: the plan stays
    empty), and the context proves a valid call afterwards."""
    c = ctx["forked"]
    rng = random.Random(77)
    nv, N = 2, 4
    one = [1, 0]
    ok_claim = [5, 6]

    def base_t(n):
        return [rand_f(rng, N) for _ in range(n)]

    def ext_t(n):
        return [rand_f(rng, 2 * N) for _ in range(n)]

    def pairs_t(n):
        return [rand_f(rng, N if i % 2 == 0 else 2 * N) for i in range(n)]

    def pws(n):
        return [one] * n

    big, bad_e = base_t(2), ext_t(2)
    big[1][3] = P
    bad_e[0][5] = 0xFFFFFFFFFFFFFFFF
    refused = {
        "kind 3": (3, base_t(2), [1, 1], pws(2), 2, ok_claim),
        "kind -1": (-1, base_t(2), [1, 1], pws(2), 2, ok_claim),
        "odd ntab, kind 1": (1, base_t(3), [1, 1, 1], pws(2), 2, ok_claim),
        "odd ntab, kind 2": (2, pairs_t(3), [1, 0, 1], pws(0), 0, ok_claim),
        "npw < ntab, kind 0": (0, base_t(3), [1, 1, 1], pws(2), 2, ok_claim),
        "npw < ntab / 2, kind 1": (1, base_t(4), [1] * 4, pws(1), 1, ok_claim),
        "65 tables, kind 0": (0, base_t(65), [1] * 65, pws(65), 65, ok_claim),
        "65 pairs, kind 1": (1, base_t(130), [1] * 130, pws(65), 65, ok_claim),
        "33 pairs, kind 2": (2, pairs_t(66), [1, 0] * 33, pws(0), 0, ok_claim),
        "mixed fields, kind 0": (0, [base_t(1)[0], ext_t(1)[0]], [1, 0], pws(2), 2, ok_claim),
        "mixed fields, kind 1": (1, [ext_t(1)[0], base_t(1)[0]], [0, 1], pws(1), 1, ok_claim),
        "(ext, base) pair, kind 2": (2, [ext_t(1)[0], base_t(1)[0]], [0, 1], pws(0), 0, ok_claim),
        "base entry = p": (1, big, [1, 1], pws(1), 1, ok_claim),
        "ext entry = 2^64 - 1": (0, bad_e, [0, 0], pws(2), 2, ok_claim),
        "b-table entry = p, kind 2": (2, [base_t(1)[0], np.array([1, P] + [0] * 6, dtype=np.uint64)], [1, 0], pws(0), 0, ok_claim),
        "claim c0 = p": (1, base_t(2), [1, 1], pws(1), 1, [P, 0]),
        "claim c1 = 2^64 - 1": (2, pairs_t(2), [1, 0], pws(0), 0, [0, 0xFFFFFFFFFFFFFFFF]),
        "power c1 = p": (0, base_t(2), [1, 1], [one, [1, P]], 2, ok_claim),
        "power c0 = p + 1, kind 1": (1, base_t(2), [1, 1], [[P + 1, 0]], 1, ok_claim),
    }
    for what, (kind, tables, is_base, pw, npw, claim) in refused.items():
        (rc, err), plan = planned(capfd, monkeypatch, lambda: raw_sumcheck(c, kind, nv, tables, is_base, pw, npw, claim), what)
        assert rc == -1 and "hg_sumcheck" in err, (what, rc, err)
        assert not plan, what
    # the limits themselves are accepted, and the context still answers as the oracle does
    for kind, ntab, base in ((0, 64, True), (1, 128, True), (2, 64, None), (1, 4, False)):
        args, exp = sumcheck_case(kind, ntab, nv, base, rand_f, 500 + kind * 200 + ntab)
        assert_sumcheck_equal(c.sumcheck(*args), exp, (kind, ntab))
