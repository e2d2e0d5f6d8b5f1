"""Kernel-level tests of the transforms, the fold and the MLE evaluations on every launch path, for both fields (-m gpu).

hg_ntt (kernels.hip: ntt_batch - radix-2 stages in HBM for log2n 1..7 and from 17, the LDS-resident four-step kernels k_ntt4_cols /
k_ntt4_rows for 8..16 with n1 = log2n / 2, n2 = log2n - n1), hg_ntt_bn254 (bn254.hip: ntt4_dev, k_bn_ntt4_cols / k_bn_ntt4_rows, the
same regimes), hg_mle_eval_bn254 (the prover's fold sequence: k_bn_fold_multi binds up to ten variables a launch, in registers for
m > 8 and in an LDS tree below, no launch left with one variable), hg_mle_eval (eq_now, which changes form at 8 variables, and dot_eq,
whose grid is capped at 1024 workgroups: a second trip from nv = 20) and hg_fold (k_fold_table: grid-stride loop from nv = 22).

Every comparison is exact equality on the whole output, on numpy limb arrays at the raw ABI (hglib.raw_*). The references: the C++
oracle's ntt, mle_eval_f and binops (orclib.ntt_f, mle_eval_f, fold_f; pinned in test_oracle_kats.py), and two closed forms that need no
oracle - the transform of an impulse (orclib.ntt_impulse) and the MLE at a point of zeros and ones, which is one table entry. Every
transform and every BN254 evaluation reads the plan line the library printed (HG_DEBUG=plan / bnplan): a case whose named path did not
print fails. pytest -rA shows the lines of every case.

Shapes: the smallest that reach each path, and the boundaries between them (7 | 8, 16 | 17 for the transforms; 8 | 9, 10 | 11, 20 | 21
variables for k_bn_fold_multi). The Goldilocks batch of 17 transforms of 2^17 has 4352 workgroups' worth of butterflies for a grid
capped at 4096: a ragged second trip in k_ntt_stage and in k_ntt_bitrev."""
import numpy as np
import pytest

import orclib
from orclib import P, R_BN as R, rand_f, edge_f, rand_fr, edge_fr, fr_limbs, ntt_f, fold_f, mle_eval_f
from hglib import hg, raw_ntt, raw_mle_eval, raw_fold, last_error
from planlib import planned, show_plans   # noqa: F401  (show_plans: the autouse fixture that prints what each test read)

pytestmark = pytest.mark.gpu

FIELDS = ("goldilocks", "bn254")
GL, BN = FIELDS
TOKEN = {GL: "plan", BN: "bnplan"}
NTT_ENTRY = {GL: "hg_ntt", BN: "hg_ntt_bn254"}
MLE_ENTRY = {GL: "hg_mle_eval", BN: "hg_mle_eval_bn254"}


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def seed(*ids):
    return np.random.default_rng([0x7472616e] + [int(i) for i in ids])


# ---- operands as limbs: (n,) words for goldilocks, (n, 4) for bn254 ---------------------------------------------------------------
def q_of(field):
    return R if field == BN else P


def rand_t(field, rng, n):
    return rand_fr(rng, n) if field == BN else rand_f(rng, n)


def edge_t(field, rng, n):
    return edge_fr(rng, n) if field == BN else edge_f(rng, n)


def const_t(field, vals):
    """a short list of Python ints as limbs"""
    return fr_limbs(vals) if field == BN else np.array(vals, dtype=np.uint64)


def full_t(field, v, n):
    """n copies of the value v"""
    return np.ascontiguousarray(np.repeat(const_t(field, [v]), n, axis=0))


def edge_values(field):
    return orclib.EDGE_POOL_FR if field == BN else orclib.EDGE_POOL


# ---- NTT ---------------------------------------------------------------------------------------------------------------------------
def check_ntt_plan(plan, log2n, batch):
    assert len(plan) == 1, plan
    l = plan[0]
    assert (l["what"], l["log2n"], l["batch"]) == ("ntt", log2n, batch), l["line"]
    if 8 <= log2n <= 16:
        assert (l["path"], l["n1"], l["n2"]) == ("four", log2n // 2, log2n - log2n // 2), l["line"]
    else:
        assert l["path"] == "radix2" and l["grid"] >= 1, l["line"]
    return l


def run_ntt(ctx, capfd, monkeypatch, field, rows, log2n, inverse, label):
    """rows: (batch, N[, 4]) limbs through the entry; checks the return code and the plan line -> (output, plan line)"""
    rows = np.ascontiguousarray(rows)
    batch = rows.shape[0]
    (rc, out), plan = planned(capfd, monkeypatch, lambda: raw_ntt(ctx, field, rows, log2n, inverse, batch),
                              "%s %s log2n=%d batch=%d %s" % (NTT_ENTRY[field], label, log2n, batch, "inverse" if inverse else "forward"), TOKEN[field])
    assert rc == 0, last_error()
    return out, check_ntt_plan(plan, log2n, batch)


def assert_rows(got, want, what):
    """exact equality of every row, naming the first row that differs"""
    for b in range(len(want)):
        assert (got[b] == want[b]).all(), "%s: row %d differs" % (what, b)


@pytest.mark.parametrize("inverse", (False, True), ids=("fwd", "inv"))
@pytest.mark.parametrize("log2n", range(1, 18))
@pytest.mark.parametrize("field", FIELDS)
def test_ntt_every_size(ctx, capfd, monkeypatch, field, log2n, inverse):
    """log2n 1..17, batch 3, random rows: each row equals the oracle's transform of that row; radix2 for 1..7 and 17, four-step between."""
    rng = seed(1, FIELDS.index(field), log2n, inverse)
    N = 1 << log2n
    rows = rand_t(field, rng, 3 * N).reshape((3, N) + ((4,) if field == BN else ()))
    got, _ = run_ntt(ctx, capfd, monkeypatch, field, rows, log2n, inverse, "random")
    assert_rows(got, [ntt_f(field, r, log2n, inverse) for r in rows], "log2n=%d" % log2n)


@pytest.mark.parametrize("inverse", (False, True), ids=("fwd", "inv"))
@pytest.mark.parametrize("log2n", (1, 7, 8, 9, 15, 16, 17))
@pytest.mark.parametrize("field", FIELDS)
def test_ntt_edge_operands(ctx, capfd, monkeypatch, field, log2n, inverse):
    """One batch of four rows: every entry from the edge pool; every entry q - 1; alternating 0, q - 1; q - 1 then zeros."""
    rng = seed(2, FIELDS.index(field), log2n, inverse)
    N, q = 1 << log2n, q_of(field)
    alt = full_t(field, q - 1, N)
    alt[0::2] = 0
    first = full_t(field, 0, N)
    first[0] = const_t(field, [q - 1])[0]
    rows = np.stack([edge_t(field, rng, N), full_t(field, q - 1, N), alt, first])
    got, _ = run_ntt(ctx, capfd, monkeypatch, field, rows, log2n, inverse, "edges")
    assert_rows(got, [ntt_f(field, r, log2n, inverse) for r in rows], "log2n=%d" % log2n)


@pytest.mark.parametrize("inverse", (False, True), ids=("fwd", "inv"))
@pytest.mark.parametrize("log2n", (8, 9, 15, 16, 17))
@pytest.mark.parametrize("field", FIELDS)
def test_ntt_impulses_match_the_closed_form(ctx, capfd, monkeypatch, field, log2n, inverse):
    """c (an edge value) at position j, zero elsewhere -> c w^(jk): positions 0, 1, N2 - 1, N2, N - 1 (N2 = 2^n2 the column count of the
    four-step split) and a random one, in one batch. Pins the index maps of both four-step kernels at both parities of the split
    without the oracle."""
    rng = seed(3, FIELDS.index(field), log2n, inverse)
    N, N2 = 1 << log2n, 1 << (log2n - log2n // 2)
    pos = [0, 1, N2 - 1, N2, N - 1, int(rng.integers(0, N))]
    pool = [v for v in edge_values(field) if v > 1]
    cs = [pool[int(i)] for i in rng.choice(len(pool), size=len(pos), replace=False)]
    rows = np.stack([full_t(field, 0, N) for _ in pos])
    for b, (j, c) in enumerate(zip(pos, cs)):
        rows[b, j] = const_t(field, [c])[0]
    got, _ = run_ntt(ctx, capfd, monkeypatch, field, rows, log2n, inverse, "impulses at %s" % pos)
    assert_rows(got, [orclib.ntt_impulse(field, log2n, j, c, inverse) for j, c in zip(pos, cs)], "log2n=%d positions %s" % (log2n, pos))


# (field, log2n, batch): the headline witness derivation's batch (2k + 1 = 33 transforms of 2^16), many rows of the smallest four-step
# size (the y extent of a one-workgroup grid), and the capped radix-2 grid
BATCH_SHAPES = [(GL, 16, 33), (BN, 16, 33), (GL, 8, 257), (BN, 8, 257), (GL, 17, 17)]


@pytest.mark.parametrize("inverse", (False, True), ids=("fwd", "inv"))
@pytest.mark.parametrize("field,log2n,batch", BATCH_SHAPES, ids=["%s-%d-x%d" % s for s in BATCH_SHAPES])
def test_ntt_batch_shapes(ctx, capfd, monkeypatch, field, log2n, batch, inverse):
    """Every row equals the oracle's. Two rows are identical and one row is zero, so that a wrong row offset is seen."""
    rng = seed(4, FIELDS.index(field), log2n, batch, inverse)
    N = 1 << log2n
    rows = rand_t(field, rng, batch * N).reshape((batch, N) + ((4,) if field == BN else ()))
    twin, zero = batch - 1, batch // 2
    rows[twin] = rows[1]
    rows[zero] = 0
    got, line = run_ntt(ctx, capfd, monkeypatch, field, rows, log2n, inverse, "batch")
    if (field, log2n) == (GL, 17):
        assert line["grid"] == 4096 and batch << (log2n - 1) > 4096 * 256 and (batch << (log2n - 1)) % (4096 * 256) != 0, line["line"]
    want = {}
    for b in range(batch):   # (the twin's reference is computed once)
        want[b] = want[1] if b == twin else ntt_f(field, rows[b], log2n, inverse)
    assert_rows(got, [want[b] for b in range(batch)], "log2n=%d batch=%d" % (log2n, batch))
    assert not got[zero].any() and (got[twin] == got[1]).all()


def tiny(field, n=2):
    return full_t(field, 0, n)


def over(field, n, at, v):
    """a valid random table with the non-canonical value v at `at`"""
    t = rand_t(field, seed(5, n, at), n)
    t[at] = const_t(field, [v])[0] if field == BN else np.uint64(v)
    return t


def ntt_refusals(field):
    """(id, args of raw_ntt behind the context, what hg_last_error says) - one row per refusal of the entry's list in include/hg.h"""
    q, big = q_of(field), 33 if field == GL else 29
    el = (4,) if field == BN else ()
    ok = lambda: rand_t(field, seed(6), 16)   # noqa: E731
    rows = [
        ("null-in", lambda: (None, 4, False, 1, ok()), "null"),
        ("null-out", lambda: (ok(), 4, False, 1, None), "null"),
        ("log2n-0", lambda: (tiny(field), 0, False, 1, tiny(field)), "size out of range"),
        ("log2n-%d" % big, lambda: (tiny(field), big, False, 1, tiny(field)), "size out of range"),   # (buffers that cannot exist: nothing is read first)
        ("batch-0", lambda: (ok(), 4, False, 0, ok()), "empty batch"),
        ("batch-65536-log2n-8", lambda: (np.zeros((65536 << 8,) + el, dtype=np.uint64), 8, False, 65536, np.zeros((65536 << 8,) + el, dtype=np.uint64)), "65535"),
        ("word-eq-q", lambda: (over(field, 16, 5, q), 4, False, 1, ok()), "non-canonical" if field == GL else "not below r"),
        ("last-word-max", lambda: (over(field, 512, 511, (1 << (256 if field == BN else 64)) - 1), 8, True, 2, tiny(field, 512)), "non-canonical" if field == GL else "not below r"),
    ]
    return [pytest.param(field, mk, what, id="%s-%s" % (field, name)) for name, mk, what in rows]


def valid_ntt_still_works(ctx, field):
    rows = rand_t(field, seed(7), 2 * 256).reshape((2, 256) + ((4,) if field == BN else ()))
    rc, out = raw_ntt(ctx, field, rows, 8, True, 2)
    assert rc == 0, last_error()
    assert_rows(out, [ntt_f(field, r, 8, True) for r in rows], "after a refusal")


@pytest.mark.parametrize("field,make,what", ntt_refusals(GL) + ntt_refusals(BN))
def test_ntt_refusals(ctx, capfd, monkeypatch, field, make, what):
    """-1, hg_last_error names the entry and the cause, no plan line (nothing was launched), the output untouched, and the context
    still transforms a valid batch correctly."""
    data, log2n, inverse, batch, out = make()
    before = None if out is None or out.size > 1 << 20 else out.copy()
    (rc, _), plan = planned(capfd, monkeypatch, lambda: raw_ntt(ctx, field, data, log2n, inverse, batch, out), "refused: " + what, TOKEN[field])
    assert rc == -1 and last_error().startswith(NTT_ENTRY[field] + ": ") and what in last_error(), last_error()
    assert plan == []
    assert before is None or (out == before).all()
    valid_ntt_still_works(ctx, field)


@pytest.mark.parametrize("field", FIELDS)
def test_ntt_refuses_a_null_context(field):
    data = rand_t(field, seed(8), 16)
    rc, _ = raw_ntt(None, field, data, 4, False, 1)
    assert rc == -1 and last_error().startswith(NTT_ENTRY[field] + ": "), last_error()


@pytest.mark.parametrize("field", FIELDS)
def test_ntt_batch_65536_on_the_radix2_path_is_accepted(ctx, capfd, monkeypatch, field):
    """The batch the four-step range refuses, at log2n = 1 (radix-2, 131072 elements): accepted and correct. The size-2 transform is
    (a + b, a - b), taken from the oracle's vector add and sub."""
    rng = seed(9, FIELDS.index(field))
    rows = rand_t(field, rng, 2 * 65536).reshape((65536, 2) + ((4,) if field == BN else ()))
    got, _ = run_ntt(ctx, capfd, monkeypatch, field, rows, 1, False, "batch 65536")
    a, b = np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1])
    assert (got[:, 0] == orclib.binop_limbs(field, False, 0, a, b)).all() and (got[:, 1] == orclib.binop_limbs(field, False, 1, a, b)).all()
    assert (got[:3] == np.stack([ntt_f(field, r, 1) for r in rows[:3]])).all()


# ---- MLE evaluation ----------------------------------------------------------------------------------------------------------------
def point_t(field, fill, rng, nv):
    """nv extension elements as limbs: (nv, 2) goldilocks, (nv, 4) bn254"""
    gen = edge_t if fill == "edge" else rand_t
    return gen(field, rng, max(nv, 1))[:nv] if field == BN else gen(field, rng, 2 * max(nv, 1))[:2 * nv].reshape(nv, 2)


def want_m(nv):
    """the variables each k_bn_fold_multi launch binds: up to ten, and no launch left with one"""
    if nv < 2:
        return []
    if nv <= 10:
        return [nv]
    if nv == 11:
        return [9, 2]
    if nv <= 20:
        return [10, nv - 10]
    assert nv == 21
    return [10, 9, 2]


def run_mle(ctx, capfd, monkeypatch, field, table, nv, point, label):
    """-> the value as a Python int (goldilocks: c0 + (c1 << 64), the form mle_eval_f returns); the BN254 entry's plan line is checked"""
    table = np.ascontiguousarray(table)
    point = np.ascontiguousarray(point) if nv else None   # (a null point at nv = 0)
    (rc, out), plan = planned(capfd, monkeypatch, lambda: raw_mle_eval(ctx, field, table, nv, point), "%s %s nv=%d" % (MLE_ENTRY[field], label, nv), TOKEN[field])
    assert rc == 0, last_error()
    if field == BN:
        assert len(plan) == 1 and (plan[0]["what"], plan[0]["nv"], plan[0]["m"]) == ("mle", nv, want_m(nv)), plan
    else:
        assert plan == []
    return orclib.from_limbs(out, len(out))[0]


def mle_case(ctx, capfd, monkeypatch, field, nv, fill):
    rng = seed(10, FIELDS.index(field), nv, fill == "edge")
    table = (edge_t if fill == "edge" else rand_t)(field, rng, 1 << nv)
    point = point_t(field, fill, rng, nv)
    got = run_mle(ctx, capfd, monkeypatch, field, table, nv, point, fill)
    assert got == mle_eval_f(field, table, point if nv else []), (nv, fill)


@pytest.mark.parametrize("nv", range(0, 22))
def test_bn254_mle_eval_runs_the_fold_sequence_of_the_prover(ctx, capfd, monkeypatch, nv):
    """nv 0..21 on a random table and point: the value equals the oracle's and the launches are the prover's - none at 0 and 1, [nv] up
    to 10, [9, 2] at 11, [10, 2] at 12, [10, 10] at 20, [10, 9, 2] at 21."""
    mle_case(ctx, capfd, monkeypatch, BN, nv, "random")


@pytest.mark.parametrize("nv", (2, 8, 9, 10, 11, 21))
def test_bn254_mle_eval_edge_operands(ctx, capfd, monkeypatch, nv):
    """table and point drawn from the edge pool alone: the LDS tree alone (2, 8), the register fold ahead of it (9, 10), chained launches"""
    mle_case(ctx, capfd, monkeypatch, BN, nv, "edge")


@pytest.mark.parametrize("nv", range(0, 21))
def test_mle_eval_every_size(ctx, capfd, monkeypatch, nv):
    """nv 0..20: eq_now changes form at 8 variables; at 20 a workgroup of dot_eq takes a second trip (grid capped at 1024)"""
    mle_case(ctx, capfd, monkeypatch, GL, nv, "random")


@pytest.mark.parametrize("nv", (1, 7, 8, 9, 19, 20))
def test_mle_eval_edge_operands(ctx, capfd, monkeypatch, nv):
    mle_case(ctx, capfd, monkeypatch, GL, nv, "edge")


@pytest.mark.parametrize("field,nv", [(BN, 11), (BN, 21), (GL, 8), (GL, 20)], ids=lambda v: str(v))
def test_mle_eval_at_a_point_of_zeros_and_ones_is_one_table_entry(ctx, capfd, monkeypatch, field, nv):
    """Coordinate i of the point is bit i of the index (lowest variable first, the order of hg_fold): index 0, the last index, a random one."""
    rng = seed(11, FIELDS.index(field), nv)
    table = rand_t(field, rng, 1 << nv)
    for idx in (0, (1 << nv) - 1, int(rng.integers(1, (1 << nv) - 1))):
        point = np.zeros((nv, 4 if field == BN else 2), dtype=np.uint64)
        point[:, 0] = [(idx >> i) & 1 for i in range(nv)]
        got = run_mle(ctx, capfd, monkeypatch, field, table, nv, point, "index %d" % idx)
        assert got == orclib.from_limbs(np.atleast_1d(table[idx]), 4 if field == BN else 1)[0], (nv, idx)


def mle_refusals(field):
    q = q_of(field)
    big = 29 if field == BN else 31
    pt = lambda nv: point_t(field, "random", seed(12), nv)   # noqa: E731
    tab = lambda nv: rand_t(field, seed(13), 1 << nv)   # noqa: E731
    bad_pt = pt(3)
    bad_pt[2, -1 if field == GL else 3] = np.uint64((1 << 64) - 1)   # (goldilocks: the second coordinate; bn254: the top limb)
    noncanon = "non-canonical" if field == GL else "not below r"
    rows = [
        ("null-table", lambda: (None, 3, pt(3), "new"), "null"),
        ("null-point", lambda: (tab(3), 3, None, "new"), "null"),
        ("null-out", lambda: (tab(3), 3, pt(3), None), "null"),
        ("nv-%d" % big, lambda: (tiny(field), big, pt(1), "new"), "size out of range"),
        ("table-eq-q", lambda: (over(field, 8, 7, q), 3, pt(3), "new"), noncanon),
        ("point-over", lambda: (tab(3), 3, bad_pt, "new"), noncanon),
    ]
    return [pytest.param(field, mk, what, id="%s-%s" % (field, name)) for name, mk, what in rows]


@pytest.mark.parametrize("field,make,what", mle_refusals(GL) + mle_refusals(BN))
def test_mle_eval_refusals(ctx, capfd, monkeypatch, field, make, what):
    table, nv, point, out = make()
    (rc, res), plan = planned(capfd, monkeypatch, lambda: raw_mle_eval(ctx, field, table, nv, point, out), "refused: " + what, TOKEN[field])
    assert rc == -1 and last_error().startswith(MLE_ENTRY[field] + ": ") and what in last_error(), last_error()
    assert plan == [] and (res is None or not res.any())
    t, p = rand_t(field, seed(14), 16), point_t(field, "random", seed(15), 4)   # (and the context still evaluates)
    rc, got = raw_mle_eval(ctx, field, t, 4, p)
    assert rc == 0 and orclib.from_limbs(got, len(got))[0] == mle_eval_f(field, t, p), last_error()


def test_bn254_mle_eval_refuses_a_null_context():
    rc, _ = raw_mle_eval(None, BN, rand_fr(seed(16), 4), 2, rand_fr(seed(17), 2))
    assert rc == -1 and last_error().startswith("hg_mle_eval_bn254: "), last_error()


# ---- hg_fold -----------------------------------------------------------------------------------------------------------------------
def fold_rs(rng):
    return [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), tuple(int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64))]


def fold_case(ctx, nv, is_base, fill):
    rng = seed(18, nv, is_base, fill == "edge")
    table = (edge_f if fill == "edge" else rand_f)(rng, (1 if is_base else 2) << nv)
    pairs = table.reshape(-1, 1 if is_base else 2)
    for r in fold_rs(rng):
        r2 = np.array(r, dtype=np.uint64)
        rc, got = raw_fold(ctx, table, nv, is_base, r2)
        assert rc == 0, last_error()
        assert (got == fold_f(GL, table, is_base, r2)).all(), (nv, is_base, fill, r)
        if r in ((0, 0), (1, 0)):   # the even entries, the odd entries: plain numpy
            pick = pairs[r[0]::2]
            assert (got[:, :pick.shape[1]] == pick).all() and (is_base and not got[:, 1].any() or not is_base), (nv, is_base, r)


@pytest.mark.parametrize("is_base", (True, False), ids=("base", "ext2"))
@pytest.mark.parametrize("nv", (1, 2, 9, 21, 22))
def test_fold_every_size(ctx, nv, is_base):
    """Base and Ext2 tables, the whole output against x + r (y - x) of the oracle's binops, r = (0, 0), (1, 0), (0, 1), (p - 1, p - 1)
    and a random pair; nv = 22 is the first size at which a thread of k_fold_table takes a second trip (grid capped at 4096 x 256)."""
    fold_case(ctx, nv, is_base, "random")


@pytest.mark.parametrize("is_base", (True, False), ids=("base", "ext2"))
@pytest.mark.parametrize("nv", (9, 22))
def test_fold_edge_operands(ctx, nv, is_base):
    fold_case(ctx, nv, is_base, "edge")


def fold_refusals():
    tab = lambda n: rand_f(seed(19), n)   # noqa: E731
    r = lambda *v: np.array(v, dtype=np.uint64)   # noqa: E731
    rows = [
        ("null-table", lambda: (None, 3, True, r(1, 2), "new"), "null"),
        ("null-r", lambda: (tab(8), 3, True, None, "new"), "null"),
        ("null-out", lambda: (tab(8), 3, True, r(1, 2), None), "null"),
        ("nv-0", lambda: (tab(2), 0, True, r(1, 2), np.zeros((1, 2), dtype=np.uint64)), "size out of range"),   # (small arrays: nothing is read first)
        ("nv-31", lambda: (tab(2), 31, False, r(1, 2), np.zeros((1, 2), dtype=np.uint64)), "size out of range"),
        ("base-word-eq-p", lambda: (over(GL, 8, 7, P), 3, True, r(1, 2), "new"), "non-canonical"),
        ("ext2-last-word-max", lambda: (over(GL, 16, 15, (1 << 64) - 1), 3, False, r(1, 2), "new"), "non-canonical"),
        ("r-c0-eq-p", lambda: (tab(8), 3, True, r(P, 0), "new"), "non-canonical"),
        ("r-c1-max", lambda: (tab(8), 3, True, r(0, (1 << 64) - 1), "new"), "non-canonical"),
    ]
    return [pytest.param(mk, what, id=name) for name, mk, what in rows]


@pytest.mark.parametrize("make,what", fold_refusals())
def test_fold_refusals(ctx, make, what):
    table, nv, is_base, r, out = make()
    rc, res = raw_fold(ctx, table, nv, is_base, r, out)
    assert rc == -1 and last_error().startswith("hg_fold: ") and what in last_error(), last_error()
    assert res is None or not res.any()
    t, r2 = rand_f(seed(20), 16), np.array([3, 5], dtype=np.uint64)   # (and the context still folds)
    rc, got = raw_fold(ctx, t, 4, True, r2)
    assert rc == 0 and (got == fold_f(GL, t, True, r2)).all(), last_error()
