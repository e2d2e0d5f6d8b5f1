"""Kernel-level tests of the BN254 prover's round kernels that reach every launch path of its planners and show that it ran (-m gpu).

hg_prodsum_jobs_bn254 runs the PRODSUM launches of hg_prove_bn254 (prodsum_defer / prodsum_flush in csrc/bn254_gkr.inc: k_bn_ps_round_jobs,
k_bn_reduce_jobs, k_bn_tail_jobs<BN_PRODSUM>), hg_grand_product_bn254 its grand-product launches (grand_product_core / gp_launch_set in
csrc/bn254.hip: the tree kernels, k_bn_gp_round_jobs, k_bn_tail_jobs<BN_GRANDPROD>). Every case demands exact equality with the C++ Fr
oracle (oracle/fr.hpp through orclib.sumcheck_f / grand_product_f, 8 threads) on every output and reads the descriptors the library
staged (HG_DEBUG=bnplan, lines `[hg bnplan] ..`): a case whose named path did not occur fails. pytest -rA shows the lines of every case.

The tables are limb arrays (orclib.rand_fr: random canonical values with every edge of the 256-bit arithmetic planted; orclib.edge_fr:
nothing but edges, so that edge meets edge in the unfolded first round - r - 1, r - 2, the halves of r, the limb boundaries, lifts of
negative integers); one case each also runs on an all-zero a table and on tables whose every entry is r - 1.

The shapes are derived from the planners:
  ps_nmain(nv)          shared rounds until half <= 16 with at most 8 rounds left: 1 for nv <= 6, nv - 5 from nv = 6 on
  round_grid(half, np)  gx = ceil(half / 256), from half = 4096 on ceil(half / 1024) (four j per thread); gy = min(np, 131072 / (256 gx))
  mf                    half a multiple of 64, and so are the bounds of a window
  window rule           lo >> rd and ceil(hi / 2^rd) even in every shared round rd (prodsum_defer)
  round_grid_gp         gx = ceil(half / 256) up to 1024, gy = min(nb, ceil(2048 / workgroups of the whole launch at gy = 1));
                        acc when half > 256 gx, i.e. half >= 2^19; long-row tree kernel for rows of 256 entries and more

Out of scope here: the mirrored and slot forms of the grand product's top layer and the Lasso collation's single-job launch of
k_bn_ps_round_jobs (jobmap == nullptr). They need a proving key and stay covered by the bit-exact whole proofs (test_gpu_parity.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orclib
from orclib import R_BN as R, rand_fr, edge_fr, fr_limbs
from hglib import hg, ROOT

gpu = pytest.mark.gpu
ENTRY = "hg_prodsum_jobs_bn254"


# ---- not gpu ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % ENTRY, hdr)
    assert m, "not declared in include/hg.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "hg_ctx* ctx", "size_t njobs", "const size_t* nv", "const size_t* npairs", "const uint64_t* const* tables", "const size_t* win", "size_t chain_skip",
        "uint64_t* sums4", "uint64_t* evals4"]
    assert ENTRY in hg.EXPORTS and hasattr(hg.lib(), ENTRY)
    r = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % ENTRY, rs)
    assert r, "not mirrored in rust/hg-shim/src/ffi.rs"
    assert [a.split(":", 1)[1].strip() for a in r.group(1).split(",")] == [
        "*mut HgCtx", "usize", "*const usize", "*const usize", "*const *const u64", "*const usize", "usize", "*mut u64", "*mut u64"]


def test_limb_table_helpers():
    """rand_fr / edge_fr give canonical values, plant every edge, and the limb form passes through the packers unchanged."""
    rng = np.random.default_rng(1)
    a = rand_fr(rng, 4096)
    vals = orclib.from_limbs(a.reshape(-1), 4)
    assert a.shape == (4096, 4) and a.dtype == np.uint64 and max(vals) < R
    assert set(orclib.EDGE_POOL_FR) <= set(vals) and len(set(vals)) > 4000
    e = orclib.from_limbs(edge_fr(rng, 4096).reshape(-1), 4)
    assert set(e) == set(orclib.EDGE_POOL_FR)
    assert len(orclib.from_limbs(rand_fr(rng, 4).reshape(-1), 4)) == 4   # (shorter than the pool)
    assert (orclib.to_limbs(a, 4) == orclib.to_limbs(vals, 4)).all()
    assert (hg.Context._fr_pack(a) == hg.Context._fr_pack(vals)).all()
    assert orclib.from_limbs(fr_limbs([R - 1, 1 << 64]).reshape(-1), 4) == [R - 1, 1 << 64]


# ---- the plan lines ------------------------------------------------------------------------------------------------------------
def _val(v):
    if v == "-":
        return None
    if ".." in v:
        lo, hi = v.split("..")
        return (int(lo), int(hi))
    return int(v) if re.fullmatch(r"-?\d+", v) else v


def bnplan_lines(err):
    """The `[hg bnplan]` lines of a captured stderr as dicts: what = "ps" | "gp", sub = None | "tail" | "tree", then the line's fields."""
    out = []
    for ln in err.splitlines():
        if not ln.startswith("[hg bnplan] "):
            continue
        w = ln.split()[2:]
        d = {"what": w[0], "sub": None, "line": ln}
        for tok in w[1:]:
            if "=" in tok:
                k, v = tok.split("=", 1)
                d[k] = _val(v)
            else:
                d["sub"] = tok
        out.append(d)
    return out


def sel(plan, what, sub=None, **kv):
    return [l for l in plan if l["what"] == what and l["sub"] == sub and all(l[k] == v for k, v in kv.items())]


_SEEN = []


@pytest.fixture(autouse=True)
def show_plans():
    """Prints every plan the test read, once it no longer captures (pytest -rA shows them: which launches each row ran)."""
    _SEEN.clear()
    yield
    print("\n".join(_SEEN))


def planned(capfd, monkeypatch, fn, label=""):
    """Runs fn() with HG_DEBUG=bnplan and returns (its result, the plan lines it printed)."""
    monkeypatch.setenv("HG_DEBUG", "bnplan")
    capfd.readouterr()
    try:
        res = fn()
    finally:
        monkeypatch.delenv("HG_DEBUG")
    plan = bnplan_lines(capfd.readouterr().err)
    _SEEN.extend(["-- %s" % label] + [l["line"] for l in plan])
    return res, plan


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


# ---- tables ----------------------------------------------------------------------------------------------------------------------
FILLS = ("random", "edge")


def table(fill, rng, n):
    if fill == "random":
        return rand_fr(rng, n)
    if fill == "edge":
        return edge_fr(rng, n)
    if fill == "edge_nz":   # edges without zero: a grand product's deeper layers stay non-trivial
        pool = fr_limbs([v for v in orclib.EDGE_POOL_FR if v])
        return pool[rng.integers(0, len(pool), size=n)]
    assert fill == "rm1"
    return np.tile(fr_limbs([R - 1]), (n, 1))


def ps_job(fill, rng, nv, npairs, shared=False, win=None, zero_a=False):
    """(tables, window) of one PRODSUM job; shared: one b OBJECT for every pair; win: b zero outside [lo, hi)"""
    n = 1 << nv
    b0 = table(fill, rng, n)
    if win:
        b0[:win[0]] = 0
        b0[win[1]:] = 0
    tabs = []
    for i in range(npairs):
        tabs.append(np.zeros((n, 4), dtype=np.uint64) if zero_a and i == 0 else table(fill, rng, n))
        tabs.append(b0 if shared or i == 0 else table(fill, rng, n))
    return tabs, win


def check_ps(ctx, capfd, monkeypatch, jobs, skip, label):
    """Runs the batch, compares every job's sums and evals with the oracle's at the job's slice of the chain; -> (results, plan)"""
    res, plan = planned(capfd, monkeypatch, lambda: ctx.prodsum_jobs_bn254(jobs, skip), label)
    off = skip
    for q, (tabs, _) in enumerate(jobs):
        nv = len(tabs[0]).bit_length() - 1
        _, _, eevals, esums = orclib.sumcheck_f("bn254", 2, tabs, chain_skip=off, threads=8)
        sums, evals = res[q]
        assert [x for rd in sums for x in rd] == esums, "job %d: round sums" % q
        assert evals == eevals, "job %d: folded values" % q
        off += nv
    assert len(sel(plan, "ps", "tail")) == len(jobs)
    return res, plan


def rounds_of(plan, job=0):
    r = sel(plan, "ps", job=job)
    assert [l["rd"] for l in r] == list(range(len(r))) and r
    return r


def seed(*k):
    return np.random.default_rng([254] + [int(x) for x in k])


# ---- PRODSUM: k_bn_ps_round_jobs, k_bn_reduce_jobs, k_bn_tail_jobs<BN_PRODSUM> ------------------------------------------------------
@gpu
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nv", [2, 3, 4, 5, 6])
def test_ps_lane_fold_rounds_and_every_tail_length(ctx, capfd, monkeypatch, nv, fill):
    """Row 1: one pair, one shared round (half = 2^(nv-1) < 64: the lane-by-lane fold), then the tail from half0 = 1, 2, 4, 8, 16."""
    _, plan = check_ps(ctx, capfd, monkeypatch, [ps_job(fill, seed(1, nv), nv, 1)], 3 + nv, "row 1 nv=%d %s" % (nv, fill))
    r = rounds_of(plan)
    assert len(r) == 1 and r[0]["mf"] == 0 and r[0]["half"] == 1 << (nv - 1) and r[0]["shared"] == 0 and r[0]["win"] is None
    t, = sel(plan, "ps", "tail")
    assert (t["half0"], t["rounds"], t["npairs"]) == (1 << (nv - 2), nv - 1, 1)


@gpu
@pytest.mark.parametrize("fill", FILLS + ("zero_a",))
@pytest.mark.parametrize("npairs", [1, 3])
def test_ps_matrix_core_round_then_lane_round(ctx, capfd, monkeypatch, npairs, fill):
    """Row 2: nv = 7 has two shared rounds, half = 64 (whole waves: the matrix-core fold) and half = 32 (lane by lane). zero_a: the first a
    table is all zero."""
    job = ps_job("random" if fill == "zero_a" else fill, seed(2, npairs), 7, npairs, zero_a=fill == "zero_a")
    _, plan = check_ps(ctx, capfd, monkeypatch, [job], 11, "row 2 npairs=%d %s" % (npairs, fill))
    r = rounds_of(plan)
    assert [(l["half"], l["mf"]) for l in r] == [(64, 1), (32, 0)] and all(l["npairs"] == npairs and l["shared"] == 0 for l in r)
    assert sel(plan, "ps", "tail")[0]["half0"] == 16


@gpu
@pytest.mark.parametrize("fill", FILLS)
def test_ps_several_j_per_thread(ctx, capfd, monkeypatch, fill):
    """Row 3: nv = 13, two pairs: round 0 has half = 4096 on gx = 4 workgroups, four strides of the j loop per thread."""
    _, plan = check_ps(ctx, capfd, monkeypatch, [ps_job(fill, seed(3), 13, 2)], 0, "row 3 " + fill)
    r = rounds_of(plan)
    assert len(r) == 8 and (r[0]["half"], r[0]["gx"], r[0]["mf"]) == (4096, 4, 1) and r[0]["half"] // (256 * r[0]["gx"]) == 4
    assert all(l["half"] // (256 * l["gx"]) <= 1 for l in r[1:])


@gpu
@pytest.mark.parametrize("fill", FILLS)
def test_ps_pairs_dealt_to_fewer_groups(ctx, capfd, monkeypatch, fill):
    """Row 4: nv = 17, 12 pairs: round 0 has half = 2^16 on gx = 64, and 131072 / (256 gx) = 8 groups take the 12 pairs (i += P with
    pairs left over for the first four groups)."""
    _, plan = check_ps(ctx, capfd, monkeypatch, [ps_job(fill, seed(4), 17, 12)], 5, "row 4 " + fill)
    r = rounds_of(plan)
    assert (r[0]["half"], r[0]["gx"], r[0]["gy"], r[0]["npairs"]) == (1 << 16, 64, 8, 12)
    assert any(l["gy"] == 12 for l in r[1:])


@gpu
@pytest.mark.parametrize("nv,npairs,gy0,fill", [(9, 4, 4, "random"), (9, 4, 4, "edge"), (9, 4, 4, "rm1"), (16, 32, 16, "random"), (16, 32, 16, "edge")])
def test_ps_shared_b_and_its_replicated_last_fold(ctx, capfd, monkeypatch, nv, npairs, gy0, fill):
    """Row 5: every pair multiplies the same b (one host pointer): b is folded once per round by the group pi == 0 (gy = 16 < 32 pairs at
    nv = 16) and written once per pair in the last shared round (rep=1), from where the tail reads one b per pair - the evals of every
    pair must be the oracle's. rm1 (small shape): every entry of every table is r - 1."""
    _, plan = check_ps(ctx, capfd, monkeypatch, [ps_job(fill, seed(5, nv), nv, npairs, shared=True)], 2, "row 5 nv=%d %s" % (nv, fill))
    r = rounds_of(plan)
    assert len(r) == nv - 5 and all(l["shared"] == 1 for l in r)
    assert [l["rep"] for l in r] == [0] * (len(r) - 1) + [1]
    assert r[0]["gy"] == gy0 and r[0]["mf"] == 1 and r[-1]["mf"] == 0


@gpu
@pytest.mark.parametrize("fill", FILLS)
def test_ps_tail_two_items_per_thread(ctx, capfd, monkeypatch, fill):
    """Row 6: 32 pairs with their own b tables at nv = 6: the tail starts with half0 npairs = 512 (pair index, pair) items on 256 threads."""
    _, plan = check_ps(ctx, capfd, monkeypatch, [ps_job(fill, seed(6), 6, 32)], 7, "row 6 " + fill)
    t, = sel(plan, "ps", "tail")
    assert t["half0"] * t["npairs"] == 512 and t["rounds"] == 5 and rounds_of(plan)[0]["shared"] == 0


WINDOWS = [   # nv, (lo, hi), the window is used, mf in round 0
    (12, (0, 1024), True, 1), (12, (1024, 2048), True, 1), (12, (3072, 4096), True, 1),   # aligned slices: start, middle, end
    (8, (64, 128), True, 0),      # half = 128 is whole waves but the bounds 32 .. 64 are not: lane by lane
    (8, (4, 12), False, 1),       # lo >> 2 is odd: prodsum_defer drops the window and the job runs the plain form
]


@gpu
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nv,win,used,mf0", WINDOWS)
def test_ps_windowed_b(ctx, capfd, monkeypatch, nv, win, used, mf0, fill):
    """Row 7: one pair whose b is zero outside [lo, hi): no product and no b fold outside the (halving) window, zeros written behind
    the last shared round (zero=1), whose successor - the tail - reads whole tables."""
    _, plan = check_ps(ctx, capfd, monkeypatch, [ps_job(fill, seed(7, nv, win[0]), nv, 1, win=win)], 1, "row 7 nv=%d win=%s %s" % (nv, win, fill))
    r = rounds_of(plan)
    assert len(r) == nv - 5 and r[0]["mf"] == mf0
    if not used:
        assert all(l["win"] is None and l["zero"] == 0 for l in r)
        return
    for l in r:
        assert l["win"] == (win[0] >> (l["rd"] + 1), win[1] >> (l["rd"] + 1)), l["line"]
        assert l["mf"] == int(l["half"] % 64 == 0 and l["win"][0] % 64 == 0 and l["win"][1] % 64 == 0), l["line"]
    assert [l["zero"] for l in r] == [0] * (len(r) - 1) + [1]
    if nv == 12:
        assert r[0]["win"][0] % 64 == 0 and r[0]["win"][1] % 64 == 0 and any(l["mf"] == 0 for l in r)


@gpu
@pytest.mark.parametrize("fill", FILLS)
def test_ps_jobs_of_several_sizes_in_one_flush(ctx, capfd, monkeypatch, fill):
    """Row 8: nv = 2, 7, 10, 13 with 1, 3, 32 (shared b) and 1 (windowed) pairs in one flush: the jobs share the round launches as long
    as they have shared rounds (1, 2, 5, 8 of them: jobmap / wg0 packing). Each job equals the oracle at its slice of the chain and
    equals the same job run alone."""
    rng = seed(8)
    jobs = [ps_job(fill, rng, 2, 1), ps_job(fill, rng, 7, 3), ps_job(fill, rng, 10, 32, shared=True), ps_job(fill, rng, 13, 1, win=(2048, 3072))]
    skip = 4
    res, plan = check_ps(ctx, capfd, monkeypatch, jobs, skip, "row 8 " + fill)
    rounds = [l for l in plan if l["what"] == "ps" and l["sub"] is None]
    for rd, want in enumerate([[0, 1, 2, 3], [1, 2, 3], [2, 3], [2, 3], [2, 3], [3], [3], [3]]):
        assert [l["job"] for l in rounds if l["rd"] == rd] == want
    assert all(l["shared"] == 1 for l in rounds_of(plan, 2)) and all(l["win"] is not None for l in rounds_of(plan, 3))
    off = skip
    for q, job in enumerate(jobs):
        assert ctx.prodsum_jobs_bn254([job], off) == [res[q]], "job %d alone" % q
        off += len(job[0][0]).bit_length() - 1


@gpu
def test_ps_entry_refuses_before_any_launch(ctx, capfd, monkeypatch):
    rng = seed(9)
    ok = ps_job("random", rng, 3, 1)
    two = ps_job("random", rng, 3, 2)
    over = ps_job("random", rng, 3, 1)
    over[0][1][5] = fr_limbs([R])[0]
    outside = ps_job("random", rng, 4, 1, win=(4, 8))
    outside[0][1][9, 0] = 1
    cases = [([], "njobs"), ([ok] * 65, "njobs"), ([ps_job("random", rng, 1, 1)], "nv must be"), ([ps_job("random", rng, 2, 33)], "npairs must be"),
             ([over], "not below r"), ([(two[0], (0, 4))], "one pair"), ([outside], "outside its window")]
    for jobs, what in cases:
        def call():
            with pytest.raises(hg.HgError, match=ENTRY + ".*" + what):
                ctx.prodsum_jobs_bn254(jobs, 0)
        _, plan = planned(capfd, monkeypatch, call, "refused: " + what)
        assert plan == []   # nothing was staged
    # nv = 33: checked ahead of the tables, which are never read
    sz = C.c_size_t * 2
    one = np.zeros(4, dtype=np.uint64)
    ptrs = (orclib.u64p * 2)(orclib.ptr(one), orclib.ptr(one))
    assert hg.lib().hg_prodsum_jobs_bn254(ctx.h, 1, sz(33, 0), sz(1, 0), ptrs, sz(0, 0), 0, orclib.ptr(one), orclib.ptr(one)) == -1
    assert ENTRY in hg.lib().hg_last_error().decode() and "nv must be" in hg.lib().hg_last_error().decode()
    assert ctx.prodsum_jobs_bn254([ok], 0)[0][1] == orclib.sumcheck_f("bn254", 2, ok[0])[2]   # (and the context still works)


# ---- grand product: the tree kernels, k_bn_gp_round_jobs, k_bn_tail_jobs<BN_GRANDPROD> ----------------------------------------------
def check_gp(ctx, capfd, monkeypatch, nb, nv, fill, skip, label):
    rng = seed(10, nb, nv)
    tabs = [table(fill, rng, 1 << nv) for _ in range(nb)]
    (proof, claims, point), plan = planned(capfd, monkeypatch, lambda: ctx.grand_product_bn254(tabs, skip), label)
    eproof, eclaims, epoint = orclib.grand_product_f("bn254", tabs, skip, threads=8)
    assert proof == eproof and claims == eclaims and point == epoint
    # the final claims are the tables' multilinear extensions at the final point (the relation the verifier relies on)
    assert claims == [orclib.mle_eval_f("bn254", t, point) for t in tabs]
    rounds = sel(plan, "gp")
    assert {(l["layer"], l["rd"]) for l in rounds} >= {(n, 0) for n in range(1, nv)} and all(l["mirror"] == 0 for l in rounds)
    return plan


@gpu
@pytest.mark.parametrize("fill", FILLS + ("edge_nz", "rm1"))
def test_gp_several_workgroups_per_job_and_long_row_tree_levels(ctx, capfd, monkeypatch, fill):
    """Row 9: (nb, nv) = (3, 12): round 0 of layers 11 and 10 has half = 1024 and 512, gx = 4 and 2; the rows of tree levels 1 .. 4 have
    2048 .. 256 entries and go through the long-row kernel (k_bn_prod_level_rows), the shorter ones through the single-workgroup kernel."""
    plan = check_gp(ctx, capfd, monkeypatch, 3, 12, fill, 6, "row 9 " + fill)
    assert sel(plan, "gp", rd=0, layer=11)[0]["gx"] == 4 and sel(plan, "gp", rd=0, layer=10)[0]["gx"] == 2
    tree = sel(plan, "gp", "tree")
    assert [(l["level"], l["kernel"]) for l in tree] == [(k, "rows" if k <= 4 else "tail_levels") for k in range(1, 12)]
    assert {l["layer"] for l in sel(plan, "gp", "tail")} == set(range(2, 12))


@gpu
@pytest.mark.parametrize("fill", FILLS)
def test_gp_staging_buffer_refilled_inside_the_loop(ctx, capfd, monkeypatch, fill):
    """Row 10: (50, 16): round 0 of all layers is 135 workgroups at gy = 1, so gy = ceil(2048 / 135) = 16 groups take the 50 pairs: a wave
    has ceil(50 / 16) = 4 (pair, j) items - the two staging buffers are filled ahead of the loop, refilled inside it, and the wait for
    an item with a later one in flight (vmcnt(8)) is taken."""
    plan = check_gp(ctx, capfd, monkeypatch, 50, 16, fill, 0, "row 10 " + fill)
    for layer in (15, 14, 13):
        l, = sel(plan, "gp", rd=0, layer=layer)
        assert l["items"] >= 3 and l["gy"] < l["nb"] == 50, l["line"]
    assert sel(plan, "gp", rd=0, layer=15)[0]["gx"] == 64


@gpu
@pytest.mark.parametrize("fill", FILLS)
def test_gp_running_sums_through_hbm(ctx, capfd, monkeypatch, fill):
    """Row 11: (1, 21): round 0 of layer 20 has half = 2^19 on the largest grid (gx = 1024): two steps of the jw loop per thread, the
    running sums stored after the first and reloaded in the second (GpJobDev::acc). No other round of any layer takes that path."""
    plan = check_gp(ctx, capfd, monkeypatch, 1, 21, fill, 9, "row 11 " + fill)
    acc = [(l["layer"], l["rd"]) for l in sel(plan, "gp") if l["acc"]]
    assert acc == [(20, 0)]
    l, = sel(plan, "gp", rd=0, layer=20)
    assert (l["half"], l["gx"], l["gy"], l["items"]) == (1 << 19, 1024, 1, 2)
