"""The Lasso node's limbs and single-reader eq tables formed where they are consumed (-m gpu): exact equality with the CPU oracle.

The mode-0 prover does not write the limb table: counter sorts, hash round, hash tables and openings take limb c of row j from the node
input (csrc/kernels.hip: limb_word / limb_of). And it builds only the FACTOR tables of three eq tables that have one reader each -
eq(r, .) of the claimed sum, the table of the openings at x, the output claim's - whose reader forms eq[j] = A[j & 255] * B[j >> 8] per
row (k_lasso_claim_in, k_open_x, k_dot_eq_ab). HG_LASSO_TABLES=1 writes and reads the tables instead. Which form each piece took is one
line on stderr under HG_DEBUG=plan,lasso (`[hg plan] lasso limbs=input|table claim_eq=factored|table open_eq=.. out_eq=..`; a token of
its own: the launch-plan lines of HG_DEBUG=plan are all numbers and tests/test_launch_plans.py reads them as such).

Hash kernel per case, from HG_DEBUG=slots (asserted below): n=1024 k=1 (nu = 14, segments of 2^11 rows) is already the smallest fixture
that runs the SLOT form of the hash-free first round (`[hg slots] adopted: <layers >= 1>`), and so does n=4096 k=2; the MEMORY form
runs in the child-process case with HG_SLOT_DEPTH=0 at n=1024 k=1 (no slot layer adopted)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import orclib
from hglib import hg, ROOT

pytestmark = pytest.mark.gpu

PLANS = ("forked", "one_stream")
FIXTURES = [(1024, 1, 27), (4096, 2, 55)]
FORMS = ("factored", "table")


@pytest.fixture(scope="module")
def ctx():
    c, c1 = hg.Context(0), hg.Context(0)
    c1.set_option("one_stream", 1)
    yield {"forked": c, "one_stream": c1}
    c.close()
    c1.close()


def golden(n, k, bits):
    return os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json")


_REF = {}


def node_reference(n, k, bits):
    """(Lasso node input, the oracle's proof and claim) of a fixture: computed once, shared, never written to."""
    key = (n, k, bits)
    if key not in _REF:
        p = orclib.params(n, k)
        lasso_in, _, _ = orclib.circuit_eval(p, orclib.fixture_inputs(n, k, bits))
        lasso_in.setflags(write=False)
        _REF[key] = (p, lasso_in, orclib.lasso_prove(p, lasso_in, threads=4))
    return _REF[key]


def slot_layers(err):
    """Number of slot-form layers the node adopted (0: the memory form of the hash-free first round)."""
    got = [int(l.split()[3]) for l in err.splitlines() if l.startswith("[hg slots] adopted:")]
    return got[-1] if got else 0


def lasso_lines(err):
    out = []
    for ln in err.splitlines():
        if ln.startswith("[hg plan] lasso "):
            out.append(dict(tok.split("=", 1) for tok in ln.split()[3:]))
    return out


def run_node(c, pk, lasso_in, capfd, monkeypatch):
    """One hg_lasso_prove_at with the form line and the slot report: -> (proof, claim, form line, slot form adopted?)."""
    monkeypatch.setenv("HG_DEBUG", "plan,lasso,slots")
    capfd.readouterr()
    try:
        proof, claim = hg.LassoNode(pk).prove_claim_reduction(c, np.array(lasso_in))
    finally:
        monkeypatch.delenv("HG_DEBUG")
    err = capfd.readouterr().err
    lines = lasso_lines(err)
    assert len(lines) == 1, err[-2000:]
    print(lines[0])
    return proof, claim, lines[0], slot_layers(err) >= 1


def check_default_forms(line):
    assert set(line) == {"limbs", "claim_eq", "open_eq", "out_eq"}, line
    assert line["limbs"] == "input" and all(line[f] in FORMS for f in ("claim_eq", "open_eq", "out_eq")), line
    # the claimed sum's workgroups always walk whole rows of 256 and the output claim has 2^11 entries and more here: factored wherever
    # the factor tables exist; the openings' launch shape decides for itself (open_x_takes_ab) and the line says how
    assert line["claim_eq"] == "factored" and line["out_eq"] == "factored", line


@pytest.mark.parametrize("n,k,bits", FIXTURES)
def test_node_with_factored_eq_on_both_plans(ctx, capfd, monkeypatch, n, k, bits):
    """Default forms on the forked and the one-stream context: proof and claim are the oracle's; both fixtures run the slot-form hash
    kernel (the memory form: test_general_forms_behind_the_switches with HG_SLOT_DEPTH=0)."""
    p, lasso_in, ref = node_reference(n, k, bits)
    bfv = hg.BfvEncrypt.new(n, k)
    for name in PLANS:
        pk = bfv.setup(ctx[name])
        proof, claim, line, slot = run_node(ctx[name], pk, lasso_in, capfd, monkeypatch)
        pk.free()
        assert proof == ref[0] and (claim == ref[1]).all(), name
        check_default_forms(line)
        assert slot, name


_CHILD = (
    "import hashlib, os, sys; sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)\n"
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
    "    proof, _ = bfv.prove(ctx, pk, bfv.get_inputs(%(golden)r))\n"
    "    print('PROVE', one, hashlib.sha256(proof).hexdigest())\n"
    "    pk.free(); ctx.close()\n"
    "print('CHILD OK')\n"
)

_PROOF = {}


def prove_reference(n, k, bits):
    key = (n, k, bits)
    if key not in _PROOF:
        _PROOF[key] = orclib.prove(orclib.params(n, k), orclib.fixture_inputs(n, k, bits), threads=4)[0]
    return _PROOF[key]


@pytest.mark.parametrize("n,k,bits,switch", [(1024, 1, 27, "HG_LASSO_TABLES=1"), (4096, 2, 55, "HG_LASSO_TABLES=1"), (1024, 1, 27, "HG_SLOT_DEPTH=0")])
def test_general_forms_behind_the_switches(n, k, bits, switch):
    """Child process (the switches are read once). HG_LASSO_TABLES=1: every piece reports `table`. HG_SLOT_DEPTH=0: the default forms
    beside the memory-form hash kernel. In both the node's bytes and a whole proof's (the output claim's table is outside the node) are
    the oracle's on both plans."""
    _, _, ref = node_reference(n, k, bits)
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), n=n, k=k, golden=golden(n, k, bits))
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HG_DEBUG="plan,lasso,slots", **{name: value}), cwd=ROOT)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    lines = lasso_lines(r.stderr)
    assert len(lines) == 4, r.stderr[-2000:]   # per plan: the node alone, the node inside the prove
    for line in lines:
        if name == "HG_LASSO_TABLES":
            assert line == {"limbs": "table", "claim_eq": "table", "open_eq": "table", "out_eq": "table"}, line
        else:
            check_default_forms(line)
    assert (slot_layers(r.stderr) >= 1) == (name != "HG_SLOT_DEPTH"), r.stderr[-2000:]
    want_node = (hashlib.sha256(ref[0]).hexdigest(), hashlib.sha256(np.ascontiguousarray(ref[1], dtype=np.uint64).tobytes()).hexdigest())
    want_proof = hashlib.sha256(prove_reference(n, k, bits)).hexdigest()
    nodes = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("NODE ")]
    proves = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("PROVE ")]
    assert [tuple(x[1:]) for x in nodes] == [want_node] * 2, nodes
    assert [x[1] for x in proves] == [want_proof] * 2, proves


def test_whole_prove_with_factored_output_claim(ctx):
    """bfv.prove at both fixtures with the default forms (the output claim's dot product reads the factor tables): the oracle's bytes."""
    for n, k, bits in FIXTURES:
        bfv = hg.BfvEncrypt.new(n, k)
        for name in PLANS:
            pk = bfv.setup(ctx[name])
            proof, _ = bfv.prove(ctx[name], pk, bfv.get_inputs(golden(n, k, bits)))
            pk.free()
            assert proof == prove_reference(n, k, bits), (n, k, name)


# ---- rows where the limb logic can go wrong --------------------------------------------------------------------------------------
def crafted_input():
    """The (1024, 1) node input with chosen rows overwritten by values that stay valid for their lookup: no bit outside the lookup's
    mask, every limb below the cutoff of its memory. Masks, cutoffs and the row -> lookup map are the oracle's own (orclib.lasso_layout
    gives each lookup's bit count and memories, orclib.lasso_polys each memory's limb and cutoff and every row's lookup)."""
    p, lasso_in, ref = node_reference(1024, 1, 27)
    P = orclib.lasso_polys(p, lasso_in)
    _, lookups = orclib.lasso_layout(p)
    bits = [int(l.split(":")[1]) for l in lookups]
    rows, row_lookup = P["rows"], P["row_lookup"]
    N = 1 << P["nu"]
    assert rows < N and all(b < 64 for b in bits)   # (rows beyond `rows` are padding; every mask is narrower than 64 bits)

    def top(l):   # the largest valid value of lookup l: every limb at min(cutoff - 1, what the mask leaves of the limb)
        mask, v = (1 << bits[l]) - 1, 0
        for m in P["lookup_mems"][l]:
            c = P["mem_dim"][m]
            v |= min(P["mem_cutoff"][m] - 1, (mask >> (16 * c)) & 0xFFFF) << (16 * c)
        assert v & ~mask == 0
        return v

    starts = [0] + [j for j in range(1, rows) if row_lookup[j] != row_lookup[j - 1]]   # first rows of the lookups' segments
    assert len(starts) >= 3
    x = np.array(lasso_in)
    s1, s2 = starts[1], starts[2]
    x[0:3] = 0                                             # all-zero rows (also the first row of a lookup)
    x[5:9] = top(row_lookup[5])                            # every limb at cutoff - 1, four rows running: read counters 0 .. 3
    for j in range(s1 - 3, s1 + 3):                        # one value on both sides of a segment boundary, valid for both lookups
        x[j] = 1
    x[s2] = top(row_lookup[s2])                            # first row of a lookup (mask narrower than 64 bits)
    x[s2 + 1:s2 + 4] = top(row_lookup[s2]) >> 1 if top(row_lookup[s2]) > 1 else 0
    x[rows - 1] = top(row_lookup[rows - 1])                # the last row below `rows`
    x[rows - 2] = 0
    for j in list(range(0, 9)) + list(range(s1 - 3, s1 + 3)) + list(range(s2, s2 + 4)) + [rows - 2, rows - 1]:
        l = row_lookup[j]
        v = int(x[j])
        assert v & ~((1 << bits[l]) - 1) == 0, j
        for m in P["lookup_mems"][l]:
            assert (v >> (16 * P["mem_dim"][m])) & 0xFFFF < P["mem_cutoff"][m], (j, m)
    return p, x, ref


def test_crafted_rows(ctx, capfd, monkeypatch):
    """All-zero rows, limbs at cutoff - 1, a value repeated in consecutive rows and across a segment boundary, the last row below `rows`
    and the first row of a lookup: the oracle accepts the input (and verifies its own proof of it), its proof differs from the fixture's,
    and the device's is the same on both plans."""
    p, x, ref = crafted_input()
    want = orclib.lasso_prove(p, x, threads=4)          # (CPU only up to here)
    assert want[0] != ref[0]
    ok, err = orclib.lasso_verify(p, want[0])
    assert ok, err
    bfv = hg.BfvEncrypt.new(1024, 1)
    for name in PLANS:
        pk = bfv.setup(ctx[name])
        proof, claim, line, _ = run_node(ctx[name], pk, x, capfd, monkeypatch)
        pk.free()
        assert proof == want[0] and (claim == want[1]).all(), name
        check_default_forms(line)


# ---- a whole prove through the cached graph --------------------------------------------------------------------------------------
def test_resident_proves_and_graph_replay_with_a_second_witness(ctx):
    """n=4096 k=2: three proves of one values object (walk, walk, capture), then a replay after hg_witness_gen_into with a second
    witness - the launch graph holds the factor-table launches and the unchanged events. Every proof is the oracle's for its witness."""
    c = ctx["forked"]
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(c)
    p = orclib.params(4096, 2)
    w1 = hg.Witness.synthetic(bfv.params, 0x4c494d4253 + 1)
    w2 = hg.Witness.synthetic(bfv.params, 0x4c494d4253 + 2)
    ref1, _ = orclib.prove(p, orclib.Inputs(w1.arrays()), threads=4)
    ref2, _ = orclib.prove(p, orclib.Inputs(w2.arrays()), threads=4)
    assert ref1 != ref2
    vals = hg.witness_gen(c, pk, w1)
    out = hg.ProofBuffer()
    for i in range(3):
        assert hg.prove_resident(c, pk, vals, out).bytes() == ref1, i
    hg.witness_gen_into(c, pk, w2, vals)
    assert hg.prove_resident(c, pk, vals, out).bytes() == ref2
    hg.witness_gen_into(c, pk, w1, vals)
    assert hg.prove_resident(c, pk, vals, out).bytes() == ref1
    vals.free()
    pk.free()
