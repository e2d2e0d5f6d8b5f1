"""Eq-weighted dot products and collation rounds with unreduced sums (-m gpu): exact equality everywhere.

The openings at x (k_open_x), the Lasso node's claimed sum (k_lasso_claim_in), the output claim's dot product (k_dot_eq_ab) and the
collation rounds (sc_round_body<SC_COLLATION> in its base-field first round and in the tail, k_col_step2) keep their sums in column
accumulators (csrc/gl_wide.hpp: WAcc / W2, and the narrow WNar for 16-bit multiplicands) and reduce once; loops of unbounded length
reduce and restart every WFLUSH_TRIPS = 16 trips. Field arithmetic is exact, so every byte stays what the reduce-every-product form
gave: the oracle's. k_dot_eq was measured in that form and keeps the reduced one; its cases below stay, the size derived
from the restart interval included - they hold for either form."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import orclib
from orclib import P, oracle_sumcheck
from hglib import hg, ROOT
from test_lasso_limbs import node_reference, golden, run_node, check_default_forms, lasso_lines

pytestmark = pytest.mark.gpu

PLANS = ("forked", "one_stream")
FIXTURES = [(1024, 1, 27), (4096, 2, 55)]
WFLUSH_TRIPS = 16            # csrc/gl_wide.hpp
TPB, MAX_BLOCKS = 256, 1024  # csrc/kernels.hip: grid_for


@pytest.fixture(scope="module")
def ctx():
    c, c1 = hg.Context(0), hg.Context(0)
    c1.set_option("one_stream", 1)
    yield {"forked": c, "one_stream": c1}
    c.close()
    c1.close()


# ---- 1. the Lasso node alone: claimed sum, openings at x and y, every collation round ---------------------------------------------
@pytest.mark.parametrize("n,k,bits", FIXTURES)
def test_lasso_node_default_forms(ctx, capfd, monkeypatch, n, k, bits):
    """The smallest fixtures that run k_open_x with factor tables and the slot-form hash round; forked and one-stream context."""
    _, lasso_in, ref = node_reference(n, k, bits)
    bfv = hg.BfvEncrypt.new(n, k)
    for name in PLANS:
        pk = bfv.setup(ctx[name])
        proof, claim, line, _ = run_node(ctx[name], pk, lasso_in, capfd, monkeypatch)
        pk.free()
        assert proof == ref[0] and (claim == ref[1]).all(), name
        check_default_forms(line)


_CHILD = (
    "import hashlib, sys; sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)\n"
    "import numpy as np\n"
    "from hglib import hg\n"
    "bfv = hg.BfvEncrypt.new(%(n)d, %(k)d)\n"
    "for one in (0, 1):\n"
    "    ctx = hg.Context(0)\n"
    "    if one: ctx.set_option('one_stream', 1)\n"
    "    pk = bfv.setup(ctx)\n"
    "    lasso_in, _ = pk.circuit_eval(bfv.get_inputs(%(golden)r))\n"
    "    proof, claim = hg.LassoNode(pk).prove_claim_reduction(ctx, lasso_in)\n"
    "    print('NODE', one, hashlib.sha256(proof).hexdigest(), hashlib.sha256(np.ascontiguousarray(claim, dtype=np.uint64).tobytes()).hexdigest())\n"
    "    pk.free(); ctx.close()\n"
    "print('CHILD OK')\n"
)


@pytest.mark.parametrize("n,k,bits", FIXTURES)
def test_lasso_node_with_tables(n, k, bits):
    """HG_LASSO_TABLES=1 in a child process (the switch is read once): k_open_x<false> and k_lasso_claim_in<false> read eq tables."""
    _, _, ref = node_reference(n, k, bits)
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), n=n, k=k, golden=golden(n, k, bits))
    env = dict(os.environ, HG_DEBUG="plan,lasso", HG_LASSO_TABLES="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    lines = lasso_lines(r.stderr)
    assert len(lines) == 2, r.stderr[-2000:]
    for line in lines:
        assert line == {"limbs": "table", "claim_eq": "table", "open_eq": "table", "out_eq": "table"}, line
    want = (hashlib.sha256(ref[0]).hexdigest(), hashlib.sha256(np.ascontiguousarray(ref[1], dtype=np.uint64).tobytes()).hexdigest())
    nodes = [tuple(l.split()[2:]) for l in r.stdout.splitlines() if l.startswith("NODE ")]
    assert nodes == [want] * 2, nodes


# ---- 2. collation at its edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [True, False], ids=["u64", "ext2"])
@pytest.mark.parametrize("nv", [6, 10, 14])
@pytest.mark.parametrize("ntab", [2, 5])
@pytest.mark.parametrize("fill", ["pm1", "random"])
def test_collation_edges(ctx, fill, ntab, nv, base):
    """kind 0 through hg_sumcheck against orc_sumcheck: every entry p - 1 (the largest products an accumulator sees) and random
    full-range residues; nv = 6 is the tail alone, 10 and 14 launch rounds first (the two-round pass among them); base-field tables
    take the u64 first round, Ext2 tables the Ext2 one."""
    N = 1 << nv
    size = N if base else 2 * N
    rng = np.random.default_rng(1000 * nv + 10 * ntab + int(base))
    if fill == "pm1":
        tables = [np.full(size, P - 1, dtype=np.uint64) for _ in range(ntab)]
    else:
        tables = [rng.integers(0, P, size=size, dtype=np.uint64) for _ in range(ntab)]
    pw = np.array([[pow(65536, i, P), 0] for i in range(ntab)], dtype=np.uint64)
    claim = rng.integers(0, P, size=2, dtype=np.uint64)
    skip = int(rng.integers(0, 50))
    c = ctx["forked"]
    got = c.sumcheck(0, tables, [base] * ntab, pw, claim, skip)
    exp = oracle_sumcheck(0, tables, [base] * ntab, pw, claim, skip)
    for name, g_, e_ in zip(("msgs", "point", "evals", "sums"), got, exp):
        assert (g_ == e_).all(), name


# ---- 3. hg_mle_eval: k_dot_eq<false> with closed-form expectations -----------------------------------------------------------------
def flush_nv():
    """Smallest nv at which a thread of k_dot_eq<false> would restart column accumulators at least twice INSIDE its loop (and add to
    the restarted ones afterwards): the even-length branch takes two entries per trip on grid_for(2^nv / 2) = min(1024, 2^nv / 512)
    workgroups of 256 threads, so a thread makes 2^nv / (2 * 256 * 1024) = 2^(nv - 19) trips once the grid is full. The restart fires
    after trips 16, 32, ...: more than 2 * 16 trips need 2^(nv - 19) >= 64, nv = 25 (64 trips per thread, restarts after 16, 32, 48, 64)."""
    nv = 1
    while (1 << nv) // (2 * TPB * min(MAX_BLOCKS, max(1, (1 << nv) // (2 * TPB)))) <= 2 * WFLUSH_TRIPS:
        nv += 1
    return nv


def test_flush_nv_derivation():
    assert flush_nv() == 25 and (1 << 25) // (2 * TPB * MAX_BLOCKS) == 64


def points(nv, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, P, size=2 * nv, dtype=np.uint64), np.full(2 * nv, P - 1, dtype=np.uint64)]


@pytest.mark.parametrize("nv", [1, 8, 12, flush_nv()])
def test_mle_eval_closed_forms(ctx, nv):
    """eq(point, .) sums to one, so the table identically p - 1 evaluates to p - 1 at any point; the table j -> bit b of j is the
    multilinear polynomial x_b and evaluates to coordinate b of the point (coordinate i belongs to bit i of the index). Random point and
    the point whose coordinates are all p - 1; b = 0 and b = nv - 1. nv = 25: see flush_nv (64 trips per thread)."""
    c = ctx["forked"]
    N = 1 << nv
    full = np.full(N, P - 1, dtype=np.uint64)
    idx = np.arange(N, dtype=np.uint64)
    for pt in points(nv, 77 + nv):
        got = c.mle_eval(full, pt)
        assert (int(got[0]), int(got[1])) == (P - 1, 0), nv
        for b in sorted({0, nv - 1}):
            got = c.mle_eval((idx >> np.uint64(b)) & np.uint64(1), pt)
            assert (int(got[0]), int(got[1])) == (int(pt[2 * b]), int(pt[2 * b + 1])), (nv, b)


def e2_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def test_mle_eval_random_table_against_python_integers(ctx):
    nv = 12
    rng = np.random.default_rng(4242)
    tab = rng.integers(0, P, size=1 << nv, dtype=np.uint64)
    pt = rng.integers(0, P, size=2 * nv, dtype=np.uint64)
    eq = [(1, 0)]
    for i in range(nv):   # coordinate i belongs to bit i of the index
        r = (int(pt[2 * i]), int(pt[2 * i + 1]))
        one_minus = ((1 - r[0]) % P, (-r[1]) % P)
        eq = [e2_mul(e, one_minus) for e in eq] + [e2_mul(e, r) for e in eq]
    exp = [0, 0]
    for e, t in zip(eq, tab.tolist()):
        exp[0] += e[0] * t
        exp[1] += e[1] * t
    got = ctx["forked"].mle_eval(tab, pt)
    assert (int(got[0]), int(got[1])) == (exp[0] % P, exp[1] % P)


# ---- 4. the narrow accumulator at its documented bound -----------------------------------------------------------------------------
def top_input():
    """The (1024, 1) node input with EVERY row below `rows` at the largest value valid for its lookup: each limb at 0xFFFF where mask
    and cutoff allow, else at min(cutoff - 1, what the mask leaves of the limb) - the largest 16-bit multiplicands in every row."""
    p, lasso_in, _ = node_reference(1024, 1, 27)
    Pl = orclib.lasso_polys(p, lasso_in)
    _, lookups = orclib.lasso_layout(p)
    bits = [int(l.split(":")[1]) for l in lookups]
    rows, row_lookup = Pl["rows"], Pl["row_lookup"]
    tops = []
    for l in range(len(bits)):
        mask, v = (1 << bits[l]) - 1, 0
        for m in Pl["lookup_mems"][l]:
            c = Pl["mem_dim"][m]
            v |= min(Pl["mem_cutoff"][m] - 1, (mask >> (16 * c)) & 0xFFFF) << (16 * c)
        assert v & ~mask == 0
        tops.append(v)
    x = np.array(lasso_in)
    x[:rows] = np.array([tops[l] for l in row_lookup[:rows]], dtype=np.uint64)
    assert any((t >> (16 * c)) & 0xFFFF == 0xFFFF for t in tops for c in range(4))   # the bound itself is among the limbs
    return p, x


@pytest.mark.parametrize("which", ["top", "pm1"])
def test_largest_limbs(ctx, capfd, monkeypatch, which):
    """`top`: see top_input. `pm1`: every row p - 1 = 0xFFFFFFFF00000001, out of range for the lookups like the junk case of
    test_gpu_parity.py - the limb columns, which know no cutoff, multiply by 0xFFFF in every row. Both: the oracle's bytes."""
    p, lasso_in, _ = node_reference(1024, 1, 27)
    x = top_input()[1] if which == "top" else np.full(lasso_in.size, P - 1, dtype=np.uint64)
    want = orclib.lasso_prove(p, x, threads=4)
    bfv = hg.BfvEncrypt.new(1024, 1)
    for name in PLANS:
        pk = bfv.setup(ctx[name])
        proof, claim, line, _ = run_node(ctx[name], pk, x, capfd, monkeypatch)
        pk.free()
        assert proof == want[0] and (claim == want[1]).all(), name
        check_default_forms(line)
