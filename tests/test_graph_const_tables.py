"""Launch graphs build challenge-only tables once. In mode 0 the challenges are a fixed chain, so the eq tables, DFT-row
tables and Libra tables without a mul part depend on the chain and the prover key alone: the launches that build them are left out of
the recorded graph and run once after the capture. What can go wrong is a table that does depend on the witness being built once
(stale from the first refill on) or a table built once being overwritten by a launch that stays in the graph (wrong from the second
replay on) - so every test here proves several DIFFERENT witnesses through one graph and compares with the walked proofs.
`HG_DEBUG=plan,consts` reports, per capture, the launches hoisted, the kernel launches recorded and the bytes built once."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import orclib
from hglib import hg, ROOT

pytestmark = pytest.mark.gpu

ORDER = (0, 1, 2, 1, 0, 2)   # refills of one values object: proves 1 and 2 walk, 3 captures and replays, 4 to 6 replay
SIZES = [(1024, 1), (4096, 2)]   # the smallest built-in set; several claims per node, alpha combinations, slot-form and mirrored layers


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ctx):
    """Per size, made once and left unchanged: the key, three synthetic witnesses and their walked proofs (graph off)."""
    made = {}

    def get(n, k):
        if (n, k) not in made:
            bfv = hg.BfvEncrypt.new(n, k)
            pk = bfv.setup(ctx)
            ws = [hg.Witness.synthetic(bfv.params, 0xC0575 + 16 * n + i) for i in range(3)]
            out = hg.ProofBuffer()
            walked = []
            ctx.set_option("graph", 0)
            try:
                for w in ws:
                    v = hg.witness_gen(ctx, pk, w)
                    walked.append(hg.prove_resident(ctx, pk, v, out).bytes())
                    v.free()
            finally:
                ctx.set_option("graph", 1)
            assert len(set(walked)) == 3
            made[(n, k)] = (bfv, pk, ws, walked)
        return made[(n, k)]

    yield get
    for _, pk, _, _ in made.values():
        pk.free()


def consts_lines(err):
    """The `[hg plan] consts key=value ...` lines of a captured stderr, one dict of ints per capture."""
    out = []
    for l in err.splitlines():
        if l.startswith("[hg plan] consts "):
            out.append({k: int(v) for k, v in (f.split("=") for f in l.split()[3:])})
    return out


def through_one_graph(ctx, pk, ws, order=ORDER):
    """One values object refilled in `order`, proven after every refill -> the proofs."""
    out = hg.ProofBuffer()
    vals = hg.witness_gen(ctx, pk, ws[order[0]])
    proofs = []
    try:
        for i, wi in enumerate(order):
            if i:
                hg.witness_gen_into(ctx, pk, ws[wi], vals)
            proofs.append(hg.prove_resident(ctx, pk, vals, out).bytes())
    finally:
        vals.free()
    return proofs


def reported(capfd, monkeypatch, fn):
    """fn() with the report switched on -> (its result, the consts lines)."""
    monkeypatch.setenv("HG_DEBUG", "plan,consts")
    capfd.readouterr()
    try:
        res = fn()
    finally:
        monkeypatch.delenv("HG_DEBUG")
    return res, consts_lines(capfd.readouterr().err)


@pytest.mark.parametrize("n,k", SIZES)
def test_replays_after_refills_give_the_walked_proofs(ctx, keys, capfd, monkeypatch, n, k):
    """Stale tables: four replays of one graph over three witnesses, each the walked proof of its witness."""
    _, pk, ws, walked = keys(n, k)
    proofs, rep = reported(capfd, monkeypatch, lambda: through_one_graph(ctx, pk, ws))
    for i, wi in enumerate(ORDER):
        assert proofs[i] == walked[wi], (n, k, i, wi)
    assert len(rep) == 1 and rep[0]["hoisted"] > 0 and rep[0]["bytes"] > 0, rep   # one capture, and it left launches out


@pytest.mark.parametrize("n,k", SIZES)
def test_both_settings_give_the_same_bytes_and_the_report_adds_up(ctx, keys, capfd, monkeypatch, n, k):
    _, pk, ws, walked = keys(n, k)
    got = {}
    try:
        for on in (0, 1):
            ctx.set_option("graph_const_tables", on)
            got[on] = reported(capfd, monkeypatch, lambda: through_one_graph(ctx, pk, ws))
    finally:
        ctx.set_option("graph_const_tables", 1)
    assert got[0][0] == got[1][0] == [walked[wi] for wi in ORDER]
    (r0,), (r1,) = got[0][1], got[1][1]
    assert r0["hoisted"] == 0 and r0["bytes"] == 0 and r0["split"] == 0, r0
    assert r1["hoisted"] > 0 and r1["bytes"] > 0, r1
    # every hoisted launch is one launch fewer in the graph; a queue flushed as a hoisted and a kept launch adds one
    assert r1["kept"] == r0["kept"] - r1["hoisted"] + r1["split"], (r0, r1)


def test_golden_witness_through_a_graph_equals_its_digest(ctx, keys, capfd, monkeypatch):
    n, k, bits = 4096, 2, 55
    bfv, pk, _, _ = keys(n, k)
    w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
    gold = json.load(open(os.path.join(orclib.GOLDEN, "oracle_proof_digests.json")))[f"{n}_{k}"]
    proofs, rep = reported(capfd, monkeypatch, lambda: [bfv.prove(ctx, pk, w)[0] for _ in range(4)])   # walk, walk, capture + replay, replay
    for i, proof in enumerate(proofs):
        assert len(proof) == gold["len"] and hashlib.sha256(proof).hexdigest() == gold["sha256"], i
    assert len(rep) <= 1 and all(r["hoisted"] > 0 for r in rep), rep   # (no line: an earlier test left the context's graph for this key)


def test_graph_recorded_by_warmup_proves_a_real_witness(keys, capfd, monkeypatch):
    """hg_warmup records the graph on the zero witness; the tables built once then must serve a real one."""
    n, k = 4096, 2
    bfv, _, ws, walked = keys(n, k)
    c = hg.Context(0)   # a context of its own: nothing recorded for it yet
    try:
        pk = bfv.setup(c)
        _, rep = reported(capfd, monkeypatch, lambda: bfv.warmup(c, pk))
        assert len(rep) == 1 and rep[0]["hoisted"] > 0, rep
        for wi in (1, 0):
            assert bfv.prove(c, pk, ws[wi])[0] == walked[wi], wi
        pk.free()
    finally:
        c.close()


@pytest.mark.parametrize("switch", ["HG_GATHER_CSR=1", "HG_PHASE2_LATE=1"])
def test_general_forms_keep_their_witness_dependent_launches(switch):
    """The per-term gathers (more jobs with a mul part) and Libra phase 2 in the second wave (a device u): those launches read the
    witness and must stay in the graph (child process: the library reads the switches once)."""
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import __graft_entry__ as entry\n"
        "hg = entry.load_package()\n"
        "ctx = hg.Context(0); bfv = hg.BfvEncrypt.new(4096, 2); pk = bfv.setup(ctx)\n"
        "ws = [hg.Witness.synthetic(bfv.params, 0xC0575 + i) for i in range(3)]\n"
        "out = hg.ProofBuffer(); walked = []\n"
        "ctx.set_option('graph', 0)\n"
        "for w in ws:\n"
        "    v = hg.witness_gen(ctx, pk, w); walked.append(hg.prove_resident(ctx, pk, v, out).bytes()); v.free()\n"
        "ctx.set_option('graph', 1)\n"
        "assert len(set(walked)) == 3\n"
        "vals = hg.witness_gen(ctx, pk, ws[0])\n"
        "for i, wi in enumerate(%r):\n"
        "    if i: hg.witness_gen_into(ctx, pk, ws[wi], vals)\n"
        "    assert hg.prove_resident(ctx, pk, vals, out).bytes() == walked[wi], (i, wi)\n"
        "print('CONSTS OK')\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), ORDER)
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, HG_DEBUG="plan,consts", **{name: value}))
    assert r.returncode == 0 and "CONSTS OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    rep = consts_lines(r.stderr)
    assert len(rep) == 1 and rep[0]["hoisted"] > 0 and rep[0]["kept"] > 0, rep
