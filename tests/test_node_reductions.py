"""Kernel-level tests of the Vanilla / FFT node reductions (-m gpu): the eq-factored PRODSUM form, mixed PRODSUM flushes, and the
challenge-only tables (eq tables, DFT rows) that feed the plain jobs.

hg_prodsum_jobs runs the prover's own flush (flush_bookkeeping, flush_prodsum) on caller tables; hg_claim_tables_eq / _fft run the
prover's batch of eq-table and DFT-row jobs. Every case compares every output word with the CPU oracle - an eq-factored job against
oracle_sumcheck(2, ..) on the materialised tables b_i = kappa_i eq(z', .) - and reads the launch plan the library printed
(HG_DEBUG=plan): a case whose named launch did not occur fails.

A PRODSUM plan is asserted as its signature, one word per launch in launch order: E<rd>@<h> a pass of the eq-factored kernel (rounds
rd, rd + 1), S<rd>@<h> a single round, P<rd>@<h> a fused pair, T<tail_rd> the tail; h = log2 of the half length, one per item of the
launch (E0@13,15: two jobs share the launch); <lo>-<hi> where the items' rounds differ. An eq-factored launch also prints grp (table
groups per item), wg (workgroups per group) and out_tail (the pass writes the tail's layout).

The shapes are the smallest that reach each edge: eq_tail_rd(npairs, nv) = the first round with npairs * half <= 4096, rounded up to
even, and the form exists for 2 <= tail_rd <= nv - 8 and tail_rd >= ps_eq_kmin(nv) = clamp(nv - 13, 0, 9)."""
import numpy as np
import pytest

import orclib
from orclib import P, rand_f, edge_f
import hglib
from hglib import hg
import planlib
from planlib import show_plans   # noqa: F401  (the autouse fixture that prints what each test read)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain():
    return orclib.e_chain(1024)


# ---- jobs ---------------------------------------------------------------------------------------------------------------------
class Job:
    """One PRODSUM job: a tables (2^nv words each); plain: b tables (flat (c0, c1) pairs); eq-factored: kappa (npairs, 2) and
    point = (z_off, w, hib)."""
    def __init__(self, nv, a, b=None, kappa=None, point=None):
        self.nv, self.a, self.b, self.kappa, self.point = nv, a, b, kappa, point
        self.npairs = len(a)


def plain_job(rng, npairs, nv, gen=rand_f):
    return Job(nv, [gen(rng, 1 << nv) for _ in range(npairs)], b=[gen(rng, 2 << nv) for _ in range(npairs)])


def eq_job(rng, npairs, nv, z_off, w, hib, gen=rand_f):
    # (kappas: edge values with edge tables, else uniform - rand_f would plant its edges over so short an array)
    kappa = edge_f(rng, 2 * npairs) if gen is edge_f else rng.integers(0, P, size=2 * npairs, dtype=np.uint64)
    return Job(nv, [gen(rng, 1 << nv) for _ in range(npairs)], kappa=kappa.reshape(npairs, 2), point=(z_off, w, hib))


def materialised(chain, job):
    """The plain job an eq-factored job stands for."""
    z_off, w, hib = job.point
    return Job(job.nv, job.a, b=orclib.eq_factored_b_tables(chain, z_off, w, hib, job.nv, job.kappa))


def run_jobs(ctx, jobs, skip):
    """-> (rc, [(sums, evals) per job])"""
    tables, eq4, kap = [], [], []
    for j in jobs:
        if j.point is None:
            tables += [t for pair in zip(j.a, j.b) for t in pair]
            eq4 += [0, 0, 0, 0]
        else:
            tables += j.a
            eq4 += [1] + list(j.point)
            kap.append(j.kappa.reshape(-1))
    kappa = np.ascontiguousarray(np.concatenate(kap)) if kap else None
    rc, sums, evals = hglib.raw_prodsum_jobs(ctx, [j.nv for j in jobs], [j.npairs for j in jobs], tables, eq4, kappa, skip)
    out, so, eo = [], 0, 0
    for j in jobs:
        out.append((sums[so:so + 4 * j.nv], evals[eo:eo + 4 * j.npairs]))
        so, eo = so + 4 * j.nv, eo + 4 * j.npairs
    return rc, out


def expected(chain, jobs, skip):
    """Per job the oracle's (sums, evals), each job run on its own with its chain position."""
    out, pos = [], skip
    for j in jobs:
        m = j if j.point is None else materialised(chain, j)
        out.append(orclib.oracle_prodsum(m.a, m.b, pos))
        pos += j.nv
    return out


def assert_jobs_equal(rc, got, exp, what):
    assert rc == 0, (what, hglib.last_error())
    for q, ((gs, ge), (es, ee)) in enumerate(zip(got, exp)):
        assert (gs == es).all(), (what, "job", q, "round sums")
        assert (ge == ee).all(), (what, "job", q, "evaluations")


# ---- the plan lines -----------------------------------------------------------------------------------------------------------
def _rng(lo_hi):
    lo, hi = lo_hi
    return str(lo) if lo == hi else "%d-%d" % (lo, hi)


def signature(plan):
    sig = []
    for l in plan:
        if l["what"] != "prodsum":
            continue
        if l["ptail"]:
            sig.append("T" + _rng(l["tail_rd"]))
            continue
        assert l["cnt"] == len(l["h"]) and (not l["eq"] or l["two"]), l["line"]
        sig.append("%s%s@%s" % ("E" if l["eq"] else "P" if l["two"] else "S", _rng(l["rd"]), ",".join(str(h) for h in l["h"])))
    return " ".join(sig)


def planned(capfd, monkeypatch, fn, label=""):
    return planlib.planned(capfd, monkeypatch, fn, label, describe=signature)


def eq_passes(plan):
    return [l for l in plan if l["what"] == "prodsum" and not l["ptail"] and l["eq"]]


def eq_preps(plan):
    return [l["points"] for l in plan if l["what"] == "eqprep"]


# ---- single eq-factored jobs --------------------------------------------------------------------------------------------------
# (npairs, nv) -> signature, table groups of each pass, workgroups per group of each pass (None: not asserted)
EQ_SINGLE = {
    (1, 14): ("E0@13 T2", [1], None),                 # smallest eq_single job; tail_rd > kmin = 1
    (1, 15): ("E0@14 T2", [1], None),                 # tail_rd == ps_eq_kmin
    (2, 13): ("E0@12 T2", [1], None),                 # smallest job that needs A = sum_i kappa_i a_i (ps_eq_A)
    (32, 10): ("E0@9 T2", [6], [1]),                  # tail_rd == nv - 8: one tile, SUF of one entry, 32 tables in 6 groups
    (27, 12): ("E0@11 E2@9 T4", [5, 5], [4, 1]),      # second pass on folded Ext2 input with one tile; 5 groups; the circuit's widest job
    (16, 11): ("E0@10 T2", [3], [2]),                 # groups of 6, 6 and 4 tables: the last one is short
    (5, 16): ("E0@15 E2@13 E4@11 T6", [1, 1, 1], None),   # three passes: the 4-way layout read twice before the tail layout
    (1, 20): ("E0@19 E2@17 E4@15 E6@13 T8", [1, 1, 1, 1], None),   # kmin = 7; the MID x TOP branch of the point tables
}
EQ_EDGE = [(1, 14), (32, 10), (27, 12)]


def check_eq_job(ctx, chain, capfd, monkeypatch, npairs, nv, w, hib, gen, seed):
    rng = np.random.default_rng(seed)
    z_off, skip = int(rng.integers(0, 200)), int(rng.integers(0, 50))
    job = eq_job(rng, npairs, nv, z_off, w, hib, gen)
    exp = expected(chain, [job], skip)
    (rc, got), plan = planned(capfd, monkeypatch, lambda: run_jobs(ctx, [job], skip), "eq (%d, %d) w=%d hib=%d" % (npairs, nv, w, hib))
    assert_jobs_equal(rc, got, exp, (npairs, nv, w, hib))
    want_sig, want_grp, want_wg = EQ_SINGLE[(npairs, nv)] if (npairs, nv) in EQ_SINGLE else WINDOW_SIG[(npairs, nv)]
    assert signature(plan) == want_sig, signature(plan)
    passes = eq_passes(plan)
    assert eq_preps(plan) == [1] and [l["grp"] for l in passes] == [[g] for g in want_grp], plan
    if want_wg:
        assert [l["wg"] for l in passes] == [[g] for g in want_wg], plan
    assert [l["out_tail"] for l in passes] == [[0]] * (len(passes) - 1) + [[1]], plan   # only the last pass writes the tail's layout
    return got


@pytest.mark.parametrize("npairs,nv", list(EQ_SINGLE))
def test_eq_factored_job_bit_exact(ctx, chain, capfd, monkeypatch, npairs, nv):
    """One eq-factored job with a full-width point (w = nv) on random tables: round sums and a_i(r), b_i(r) equal to the oracle's on the
    materialised tables, and the plan the row names."""
    check_eq_job(ctx, chain, capfd, monkeypatch, npairs, nv, nv, 0, rand_f, 1000 + 40 * npairs + nv)


@pytest.mark.parametrize("npairs,nv", EQ_EDGE)
def test_eq_factored_job_on_edge_operands(ctx, chain, capfd, monkeypatch, npairs, nv):
    """Every table entry and every kappa coordinate an edge value of the field reductions (zero among them)."""
    check_eq_job(ctx, chain, capfd, monkeypatch, npairs, nv, nv, 0, edge_f, 2000 + 40 * npairs + nv)


# ---- windowed points: top coordinates Boolean, the table zero outside block hib ------------------------------------------------------
WINDOW_SIG = {
    (1, 16): ("E0@15 E2@13 T4", [1, 1], None),
}
WINDOW_SHAPES = [(1, 16), (5, 16), (32, 10)]


def windows(nv):
    """(w, hib): one Boolean coordinate; three, block 5; w = 10 with the largest block; w = 3 with mixed bits; w = 0 (kappa a[hib])"""
    mixed = 0x2B5A5A5 & ((1 << (nv - 3)) - 1)
    return [(nv - 1, 1), (nv - 3, 5), (10, (1 << (nv - 10)) - 1), (3, mixed), (0, (0x15C3 * 7) & ((1 << nv) - 1))]


@pytest.mark.parametrize("npairs,nv", WINDOW_SHAPES)
@pytest.mark.parametrize("k", range(5))
def test_eq_factored_job_windowed(ctx, chain, capfd, monkeypatch, npairs, nv, k):
    """b_i(r) = kappa_i eq(z', r) with z' = (chain run of w, bits of hib): tiles outside the block are skipped by the passes (`live`)."""
    w, hib = windows(nv)[k]
    got = check_eq_job(ctx, chain, capfd, monkeypatch, npairs, nv, w, hib, rand_f, 3000 + 100 * k + 3 * npairs + nv)
    if w == 0:   # the job is kappa_i a_i[hib]: nothing but one entry of each table contributes
        assert any(int(x) for x in got[0][0])


# ---- the boundary of the form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npairs,nv", [(1, 13), (2, 12), (32, 9), (27, 11)])
def test_shapes_below_the_eq_factored_form(ctx, chain, capfd, monkeypatch, npairs, nv):
    """One variable below the first four rows of EQ_SINGLE: refused as an eq-factored job (no launch), proven as a plain job on the
    materialised tables."""
    rng = np.random.default_rng(4000 + 40 * npairs + nv)
    job = eq_job(rng, npairs, nv, 17, nv, 0)
    (rc, _), plan = planned(capfd, monkeypatch, lambda: run_jobs(ctx, [job], 3), "refused (%d, %d)" % (npairs, nv))
    assert rc == -1 and "hg_prodsum_jobs" in hglib.last_error() and "does not take the eq-factored form" in hglib.last_error(), hglib.last_error()
    assert not plan
    m = materialised(chain, job)
    exp = expected(chain, [m], 3)
    (rc, got), plan = planned(capfd, monkeypatch, lambda: run_jobs(ctx, [m], 3), "plain (%d, %d)" % (npairs, nv))
    assert_jobs_equal(rc, got, exp, (npairs, nv))
    assert not eq_passes(plan) and not eq_preps(plan) and signature(plan).split()[-1].startswith("T"), plan


# ---- several jobs in one flush --------------------------------------------------------------------------------------------------
def test_shared_and_unshared_points(ctx, chain, capfd, monkeypatch):
    """Two jobs at the same (z_off, w, hib) share one pair of point tables, a third at another z_off has its own: one ps_eq_prep launch
    over two points, and every job equal to its own oracle run."""
    rng = np.random.default_rng(5001)
    jobs = [eq_job(rng, 1, 14, 5, 12, 2), eq_job(rng, 2, 14, 5, 12, 2), eq_job(rng, 1, 14, 40, 12, 2)]
    exp = expected(chain, jobs, 11)
    (rc, got), plan = planned(capfd, monkeypatch, lambda: run_jobs(ctx, jobs, 11), "shared points")
    assert_jobs_equal(rc, got, exp, "shared")
    assert eq_preps(plan) == [2], plan
    assert signature(plan) == "E0@13,13,13 T2", signature(plan)


def test_mixed_flush(ctx, chain, capfd, monkeypatch):
    """Eq-factored and plain jobs of eight sizes in one flush. The flush orders jobs by nv; per step the launches are eq-factored,
    single rounds, fused pairs; the tail launch holds every job (the three smallest run in it alone)."""
    rng = np.random.default_rng(5002)
    jobs = [eq_job(rng, 5, 16, 60, 16, 0), eq_job(rng, 1, 14, 20, 11, 5), plain_job(rng, 2, 15), plain_job(rng, 1, 14), plain_job(rng, 27, 9),
            plain_job(rng, 1, 1), plain_job(rng, 3, 2), plain_job(rng, 2, 3)]
    exp = expected(chain, jobs, 7)
    (rc, got), plan = planned(capfd, monkeypatch, lambda: run_jobs(ctx, jobs, 7), "mixed flush")
    assert_jobs_equal(rc, got, exp, "mixed")
    assert eq_preps(plan) == [2], plan
    # step 0: both eq jobs | (27, 9) and the plain (1, 14) as single rounds | the fused pair of (2, 15); step 1: (5, 16) | round 2 of
    # (2, 15); step 2: (5, 16)
    assert signature(plan) == "E0@13,15 S0@8,13 P0@14 E2@13 S2@12 E4@11 T0-6", signature(plan)
    tail = [l for l in plan if l["what"] == "prodsum" and l["ptail"]]
    assert len(tail) == 1 and tail[0]["jobs"] == len(jobs), plan


def check_batch(ctx, chain, capfd, monkeypatch, nv, want_sig, want_cnt):
    rng = np.random.default_rng(5100 + nv)
    jobs = [plain_job(rng, 1, nv) for _ in range(70)]
    exp = expected(chain, jobs, 0)
    (rc, got), plan = planned(capfd, monkeypatch, lambda: run_jobs(ctx, jobs, 0), "70 jobs of (1, %d)" % nv)
    assert_jobs_equal(rc, got, exp, nv)
    assert signature(plan).split() == want_sig, signature(plan)
    assert [l["cnt"] for l in plan if l["what"] == "prodsum" and not l["ptail"]] == want_cnt, plan
    assert plan[-1]["ptail"] and plan[-1]["jobs"] == 70, plan


def test_step_split_at_64_items(ctx, chain, capfd, monkeypatch):
    """70 plain jobs in one flush: a step is launched as 64 and 6 items. The shape is (1, 14), one variable above the issue's (1, 13):
    a job of one pair and 13 variables brings 4096 items to its first round, which is the tail's limit itself, so it has no step at
    all (the case below; the same boundary as PRODSUM[(2, 14)] = S0@13 T1 in test_launch_plans.py)."""
    check_batch(ctx, chain, capfd, monkeypatch, 14, ["S0@" + ",".join(["13"] * 64), "S0@" + ",".join(["13"] * 6), "T1"], [64, 6])


def test_70_jobs_in_the_tail_alone(ctx, chain, capfd, monkeypatch):
    """70 plain jobs of (1, 13): no step launch, one tail launch of 70 workgroups."""
    check_batch(ctx, chain, capfd, monkeypatch, 13, ["T0"], [])


# ---- hg_prodsum_jobs refuses what it cannot do ---------------------------------------------------------------------------------------
def test_prodsum_jobs_refusals(ctx, chain, capfd, monkeypatch):
    rng = np.random.default_rng(6000)
    a, b = rand_f(rng, 1 << 14), rand_f(rng, 2 << 14)
    kap = rand_f(rng, 2)
    bad_a, bad_b, bad_k = a.copy(), b.copy(), kap.copy()
    bad_a[77], bad_b[2 * 500 + 1], bad_k[1] = P, 0xFFFFFFFFFFFFFFFF, P
    big = 1 << 21
    R = hglib.raw_prodsum_jobs
    refused = {
        "null nv": lambda: R(ctx, None, [1], [a, b], [0] * 4, None, njobs=1),
        "null npairs": lambda: R(ctx, [14], None, [a, b], [0] * 4, None),
        "null tables": lambda: R(ctx, [14], [1], None, [0] * 4, None),
        "null eq4": lambda: R(ctx, [14], [1], [a, b], None, None),
        "null sums": lambda: R(ctx, [14], [1], [a, b], [0] * 4, None, sums=None),
        "null evals": lambda: R(ctx, [14], [1], [a, b], [0] * 4, None, evals=None),
        "null table": lambda: R(ctx, [14], [1], [a, None], [0] * 4, None),
        "null kappa": lambda: R(ctx, [14], [1], [a], [1, 0, 14, 0], None),
        "njobs 0": lambda: R(ctx, [14], [1], [a, b], [0] * 4, None, njobs=0),
        "njobs 129": lambda: R(ctx, [1] * 129, [1] * 129, [a[:2], b[:4]] * 129, [0] * 4 * 129, None),
        "nv 0": lambda: R(ctx, [0], [1], [a, b], [0] * 4, None),
        "nv 27": lambda: R(ctx, [27], [1], [a, b], [0] * 4, None),
        "npairs 0": lambda: R(ctx, [14], [0], [a, b], [0] * 4, None),
        "npairs 33": lambda: R(ctx, [14], [33], [a, b] * 33, [0] * 4, None),
        "form 2": lambda: R(ctx, [14], [1], [a, b], [2, 0, 0, 0], None),
        "table word = p": lambda: R(ctx, [14], [1], [bad_a, b], [0] * 4, None),
        "b word = 2^64 - 1": lambda: R(ctx, [14], [1], [a, bad_b], [0] * 4, None),
        "eq table word = p": lambda: R(ctx, [14], [1], [bad_a], [1, 0, 14, 0], kap),
        "kappa = p": lambda: R(ctx, [14], [1], [a], [1, 0, 14, 0], bad_k),
        "w > nv": lambda: R(ctx, [14], [1], [a], [1, 0, 15, 0], kap),
        "hib = 2^(nv - w)": lambda: R(ctx, [14], [1], [a], [1, 0, 11, 8], kap),
        "hib with w = nv": lambda: R(ctx, [14], [1], [a], [1, 0, 14, 1], kap),
        "z_off out of range": lambda: R(ctx, [14], [1], [a], [1, big, 14, 0], kap),
        "chain_skip out of range": lambda: R(ctx, [14], [1], [a, b], [0] * 4, None, chain_skip=big),
        "second job refused": lambda: R(ctx, [14, 13], [1, 1], [a, b, a[:1 << 13]], [0] * 4 + [1, 0, 13, 0], kap),
    }
    for what, fn in refused.items():
        (rc, _, _), plan = planned(capfd, monkeypatch, fn, what)
        assert rc == -1 and "hg_prodsum_jobs" in hglib.last_error(), (what, rc, hglib.last_error())
        assert not plan, what
    # the limits themselves are accepted: hib = 2^(nv - w) - 1, 128 jobs, 32 pairs, nv = 1
    jobs = [eq_job(rng, 1, 14, 0, 11, 7)] + [plain_job(rng, 1, 1) for _ in range(126)] + [plain_job(rng, 32, 2)]
    rc, got = run_jobs(ctx, jobs, 0)
    assert_jobs_equal(rc, got, expected(chain, jobs, 0), "limits")


# ---- claim tables: sum_a alpha_a eq(r_a, .) ------------------------------------------------------------------------------------------
def claim_offsets(rng, jobs):
    """jobs: [(n, nclaims, unit)] -> flat point offsets, per-job alpha offsets (None: unit weight)"""
    po = [int(x) for _, nc, _ in jobs for x in rng.integers(0, 300, size=nc)]
    al = [None if unit else int(rng.integers(0, 300)) for _, _, unit in jobs]
    return po, al


def eq_plan(plan):
    lines = [l for l in plan if l["what"] == "eqtab"]
    assert len(lines) == 1 and len(plan) == 1, plan
    return lines[0]


def check_eq_tables(ctx, chain, capfd, monkeypatch, jobs, seed, label):
    rng = np.random.default_rng(seed)
    po, al = claim_offsets(rng, jobs)
    (rc, out), plan = planned(capfd, monkeypatch, lambda: hglib.raw_claim_tables_eq(ctx, [j[0] for j in jobs], [j[1] for j in jobs], po, al), label)
    assert rc == 0, hglib.last_error()
    c0 = 0
    for q, (n, nc, _) in enumerate(jobs):
        assert (out[q] == orclib.eq_claims_table(chain, n, po[c0:c0 + nc], al[q])).all(), (label, "job", q, n, nc)
        c0 += nc
    l = eq_plan(plan)
    assert l["jobs"] == len(jobs) and l["ab"] == 1 and l["max_n"] == max(j[0] for j in jobs), l["line"]
    # one prep workgroup per claim and 256 high entries, one fill workgroup per `rows` rows of 256 outputs
    assert l["prep"] == sum(nc * max(1, (1 << max(n - 8, 0)) // 256) for n, nc, _ in jobs), l["line"]
    assert l["fill"] == sum(-(-(1 << max(n - 8, 0)) // l["rows"]) for n, _, _ in jobs), l["line"]
    return l


def test_eq_tables_of_a_batch_of_claims(ctx, chain, capfd, monkeypatch):
    """n below, at and above the 8 low variables of the factor tables, 1 (unit and weighted), 2, 3 and 32 claims, and n = 17 with two
    claims (several prep workgroups per claim), all in one batch: one plan, rows = 1."""
    jobs = [(1, 1, True), (1, 32, False), (7, 2, False), (7, 32, False), (8, 3, False), (8, 1, False), (9, 32, False), (9, 1, True),
            (12, 2, False), (12, 32, False), (12, 3, False), (17, 2, False)]
    l = check_eq_tables(ctx, chain, capfd, monkeypatch, jobs, 7001, "eq tables, mixed batch")
    assert l["rows"] == 1, l["line"]


def test_eq_table_of_2_22_entries(ctx, chain, capfd, monkeypatch):
    """16384 rows: the fill launch walks eight rows per workgroup."""
    l = check_eq_tables(ctx, chain, capfd, monkeypatch, [(22, 1, True)], 7002, "eq table, n = 22")
    assert l["rows"] == 8, l["line"]


def test_eq_tables_with_a_job_shorter_than_a_workgroups_rows(ctx, chain, capfd, monkeypatch):
    """n = 21 beside n = 9: four rows per workgroup, and the small job has two rows in all (the row count clipped per workgroup)."""
    l = check_eq_tables(ctx, chain, capfd, monkeypatch, [(9, 3, False), (21, 1, False)], 7003, "eq tables, n = 9 beside n = 21")
    assert l["rows"] == 4, l["line"]


# ---- claim tables: DFT rows --------------------------------------------------------------------------------------------------------
def check_fft_tables(ctx, chain, capfd, monkeypatch, jobs, seed, label):
    """jobs: [(L, inverse, nclaims, unit)]"""
    rng = np.random.default_rng(seed)
    po, al = claim_offsets(rng, [(L, nc, unit) for L, _, nc, unit in jobs])
    (rc, out), plan = planned(capfd, monkeypatch, lambda: hglib.raw_claim_tables_fft(ctx, [j[0] for j in jobs], [j[1] for j in jobs],
                                                                                      [j[2] for j in jobs], po, al), label)
    assert rc == 0, hglib.last_error()
    c0 = 0
    for q, (L, inv, nc, _) in enumerate(jobs):
        assert (out[q] == orclib.fft_rows_table(chain, L, inv, po[c0:c0 + nc], al[q])).all(), (label, "job", q, L, inv, nc)
        c0 += nc
    assert len(plan) == 1 and plan[0]["what"] == "fftrows", plan
    l = plan[0]
    max_L = max(j[0] for j in jobs)
    assert (l["jobs"], l["max_L"], l["max_claims"], l["launches"]) == (len(jobs), max_L, max(j[2] for j in jobs), 2 if max_L > 4 else 1), l["line"]


@pytest.mark.parametrize("L", [1, 3, 4, 5, 8, 12])
def test_fft_rows_both_directions(ctx, chain, capfd, monkeypatch, L):
    """L below, at and above FFT_SPLIT = 4 (one launch up to 4, the factor tables' launch above); forward and inverse rows with 1, 2
    and 5 claims in one call."""
    jobs = [(L, False, 1, True), (L, True, 1, False), (L, False, 2, False), (L, True, 2, False), (L, False, 5, False), (L, True, 5, False)]
    check_fft_tables(ctx, chain, capfd, monkeypatch, jobs, 8000 + L, "fft rows, L = %d" % L)


def test_fft_rows_of_different_sizes_in_one_call(ctx, chain, capfd, monkeypatch):
    """L = 3 beside 5 and 12: a job without factor tables in a launch that has them, max_claims above two jobs' own counts."""
    check_fft_tables(ctx, chain, capfd, monkeypatch, [(3, False, 5, False), (5, True, 1, True), (12, False, 2, False)], 8100, "fft rows, mixed sizes")


def test_fft_rows_of_2_19_entries(ctx, chain, capfd, monkeypatch):
    """2^19 outputs against 1024 workgroups of 256 threads: the grid-stride loop takes a second trip."""
    check_fft_tables(ctx, chain, capfd, monkeypatch, [(19, True, 1, False)], 8200, "fft rows, L = 19")


def test_claim_tables_refusals(ctx, chain, capfd, monkeypatch):
    E, F = hglib.raw_claim_tables_eq, hglib.raw_claim_tables_fft
    big = 1 << 21
    refused = {
        "eq: njobs 65": lambda: E(ctx, [1] * 65, [1] * 65, [0] * 65, [None] * 65),
        "eq: n 0": lambda: E(ctx, [0], [1], [0], [None]),
        "eq: n 25": lambda: E(ctx, [25], [1], [0], [None], out=[np.zeros((2, 2), dtype=np.uint64)]),
        "eq: nclaims 0": lambda: E(ctx, [4], [0], [0], [5]),
        "eq: nclaims 33": lambda: E(ctx, [4], [33], [0] * 33, [5]),
        "eq: unit weight, two claims": lambda: E(ctx, [4], [2], [0, 9], [None]),
        "eq: point_off out of range": lambda: E(ctx, [4], [1], [big], [None]),
        "eq: alpha_off out of range": lambda: E(ctx, [4], [1], [0], [big]),
        "eq: null output": lambda: E(ctx, [4], [1], [0], [None], out=[None]),
        "fft: njobs 65": lambda: F(ctx, [1] * 65, [0] * 65, [1] * 65, [0] * 65, [None] * 65),
        "fft: L 0": lambda: F(ctx, [0], [0], [1], [0], [None]),
        "fft: L 25": lambda: F(ctx, [25], [0], [1], [0], [None], out=[np.zeros((2, 2), dtype=np.uint64)]),
        "fft: nclaims 33": lambda: F(ctx, [4], [1], [33], [0] * 33, [5]),
        "fft: unit weight, two claims": lambda: F(ctx, [4], [0], [2], [0, 9], [None]),
        "fft: point_off out of range": lambda: F(ctx, [4], [0], [1], [big], [None]),
        "fft: null output": lambda: F(ctx, [4], [0], [1], [0], [None], out=[None]),
    }
    for what, fn in refused.items():
        (rc, _), plan = planned(capfd, monkeypatch, fn, what)
        assert rc == -1 and ("hg_claim_tables_eq" if what.startswith("eq") else "hg_claim_tables_fft") in hglib.last_error(), (what, rc, hglib.last_error())
        assert not plan, what
    rc, out = E(ctx, [4], [1], [3], [None])
    assert rc == 0 and (out[0] == orclib.eq_claims_table(chain, 4, [3], None)).all()
