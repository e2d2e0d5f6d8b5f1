"""The claim epilogue of the grand-product tail kernel (k_st_tail<SC_GRANDPROD>, GpClaimEp in kernels.hpp): the workgroup that writes a
layer's final evaluations also unscales them, completes a mirrored job's write rows, folds them by mu (layer_down) and sums the next
layer's claim, and the transcript replay only reads result slots. The context option gp_claims_device = 0 keeps all of that in the
replay. Both forms must give the oracle's bytes, and `HG_DEBUG=plan,gpclaims` must show which one ran."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import orclib
from orclib import P, rand_f
from hglib import hg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def claim_lines(err):
    """The `[hg plan] gpclaims key=value ...` lines of a captured stderr, one dict of ints per grand product."""
    out = []
    for l in err.splitlines():
        if l.startswith("[hg plan] gpclaims "):
            out.append({k: int(v) for k, v in (f.split("=") for f in l.split()[3:])})
    return out


def with_claims(capfd, monkeypatch, ctx, on, fn):
    """fn() with the option set to `on` and the report switched on -> (its result, the report lines)."""
    ctx.set_option("gp_claims_device", on)
    monkeypatch.setenv("HG_DEBUG", "plan,gpclaims")
    capfd.readouterr()
    try:
        res = fn()
    finally:
        monkeypatch.delenv("HG_DEBUG")
        ctx.set_option("gp_claims_device", 1)
    return res, claim_lines(capfd.readouterr().err)


# nb = 1: nothing to unscale; 3: odd; 65: more pairs than a wave. nv = 8: layers of every tail length; nv = 2: a single sum-check layer.
@pytest.mark.parametrize("nv", [8, 2])
@pytest.mark.parametrize("nb", [1, 2, 3, 65])
def test_grand_product_entry_with_and_without_the_epilogue(ctx, capfd, monkeypatch, nb, nv):
    rng = random.Random(1000 * nb + nv)
    tabs = [rand_f(rng, 1 << nv) for _ in range(nb)]
    for t in tabs:   # the edge operands 0 and p - 1 in every table, whatever rand_f planted
        a, b = rng.sample(range(1 << nv), 2)
        t[a], t[b] = 0, P - 1
    skip = rng.randrange(40)
    ref, rclaims, rpoint = orclib.grand_product_f("goldilocks", [[int(v) for v in t] for t in tabs], skip, threads=4)
    for on in (1, 0):
        (proof, claims, point), rep = with_claims(capfd, monkeypatch, ctx, on, lambda: hg.grand_product(ctx, tabs, skip))
        assert proof == ref, (on, nb, nv)
        assert [int(a) | (int(b) << 64) for a, b in claims] == rclaims, (on, nb, nv)
        assert [int(a) | (int(b) << 64) for a, b in point] == rpoint, (on, nb, nv)
        # every sum-check layer (nv - 1 of them: layer 0 has none) took the form asked for
        assert rep == [dict(nb=nb, layers=nv - 1, device=(nv - 1) * on, mirrored=0, slot=0, plain=(nv - 1) * on)], (on, rep)


def test_full_proof_equals_the_golden_digest_on_both_paths(ctx, capfd, monkeypatch):
    """n=4096 k=2 (nu = 16): the lean, slot-form, mirrored top layers of the headline size run here."""
    n, k, bits = 4096, 2, 55
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
    gold = json.load(open(os.path.join(orclib.GOLDEN, "oracle_proof_digests.json")))[f"{n}_{k}"]
    proofs = {}
    for on in (1, 0):
        (proof, _), rep = with_claims(capfd, monkeypatch, ctx, on, lambda: bfv.prove(ctx, pk, w))
        assert len(proof) == gold["len"] and hashlib.sha256(proof).hexdigest() == gold["sha256"], on
        proofs[on] = proof
        assert len(rep) == 2, rep                          # grand product #1 (reads, writes), #2 (inits, finals)
        g1, g2 = rep
        assert g1["layers"] == 15 and g2["layers"] == 15 and g1["nb"] == g2["nb"], rep
        if on:
            assert g1["device"] == 15 and g1["mirrored"] == 1 and g1["slot"] >= 1 and g1["plain"] >= 1, rep
            assert g1["mirrored"] + g1["slot"] + g1["plain"] == 15, rep
            assert g2 == dict(nb=g2["nb"], layers=15, device=15, mirrored=0, slot=0, plain=15), rep
        else:
            assert g1["device"] == 0 and g2["device"] == 0, rep
            assert g1["mirrored"] + g1["slot"] + g1["plain"] + g2["plain"] == 0, rep
    assert proofs[1] == proofs[0]
    pk.free()


def test_cached_graph_replays_the_epilogue_for_another_witness(ctx):
    """Three proves of two witnesses through one values object: walk, walk, capture + replay. The epilogue's constants are challenges
    only, so the graph recorded for one witness proves the other: each proof equals the walked proof of its witness."""
    n, k = 4096, 2
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0x6701 + i) for i in range(2)]
    out = hg.ProofBuffer()
    walked = []
    ctx.set_option("graph", 0)
    try:
        for w in ws:
            v = hg.witness_gen(ctx, pk, w)
            walked.append(hg.prove_resident(ctx, pk, v, out).bytes())
            ctx.set_option("gp_claims_device", 0)          # ... and the replay's own arithmetic agrees
            assert hg.prove_resident(ctx, pk, v, out).bytes() == walked[-1]
            ctx.set_option("gp_claims_device", 1)
            v.free()
    finally:
        ctx.set_option("graph", 1)
        ctx.set_option("gp_claims_device", 1)
    assert walked[0] != walked[1]
    vals = hg.witness_gen(ctx, pk, ws[0])
    for i, wi in enumerate((0, 1, 0, 1)):                  # the third prove captures and replays, the fourth replays
        if i:
            hg.witness_gen_into(ctx, pk, ws[wi], vals)
        assert hg.prove_resident(ctx, pk, vals, out).bytes() == walked[wi], i
    vals.free()
    pk.free()
