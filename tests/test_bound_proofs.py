"""hg_prove_committed_mode / hg_verify_public_bound / hg_verify_public_bound_device: GKR proofs whose transcript starts from the key's
parameters, the digest of the public instance and the root of the commitment to the secret inputs. A bound proof verifies against
exactly that root, that instance and that mode; everything the unbound entries compute stays as it was."""
import numpy as np
import pytest

import orclib
from hglib import hg

Q2 = orclib.constants(4096, 2)["qis"]
SHAPES = [(1024, 1), (1024, 2)]


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


_CASES = {}


def case(ctx, n, k):
    """per shape: device key, a synthetic witness, its resident values and instance, and per mode one bound proof with its commitment
    (made once, never changed)"""
    if (n, k) not in _CASES:
        bfv = hg.BfvEncrypt(hg.params_builtin(n, k) if k == 1 else hg.params_derive(n, k, Q2, 65537))
        pk = bfv.setup(ctx)
        w = hg.Witness.synthetic(bfv.params, 0xb0d + n + k)
        vals = hg.witness_gen(ctx, pk, w)
        c = dict(bfv=bfv, pk=pk, w=w, vals=vals, inst=hg.Instance.from_witness(w), bound={})
        for mode in (1, 3):
            out, cm = hg.prove_committed_mode(ctx, pk, vals, hg.ProofBuffer(), mode)
            c["bound"][mode] = (out.bytes(), cm)
        _CASES[(n, k)] = c
    return _CASES[(n, k)]


def both(ctx, c, proof, root, mode, inst=None):
    """the host and the device verifier on the same input: they must agree on decision, reason and claims"""
    inst = inst or c["inst"]
    h = hg.verify_public_bound(c["pk"], inst, proof, root, mode)
    d = hg.verify_public_bound(c["pk"], inst, proof, root, mode, ctx=ctx, device=True)
    assert h[:2] == d[:2], (h[:2], d[:2])
    if h[0]:
        assert h[2].as_tuples() == d[2].as_tuples()
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("mode", [1, 3])
def test_round_trip(ctx, n, k, mode):
    c = case(ctx, n, k)
    proof, cm = c["bound"][mode]
    ok, why, cl = both(ctx, c, proof, cm.root, mode)
    assert ok, why
    assert cl.n == hg.pk_claim_shape(c["pk"])[0]
    opening = cm.open_claims(c["bfv"].params, cl)
    assert hg.claims_verify(c["bfv"].params, cm.root, cl, opening) == (True, "")
    # handle and root are those of hg_secrets_commit_values on the same values
    plain = hg.Commitment.from_values(ctx, c["pk"], c["vals"])
    assert plain.root == cm.root and plain.log2_row == cm.log2_row
    assert plain.open_claims(c["bfv"].params, cl) == opening
    assert hg.values_instance_digest(ctx, c["pk"], c["vals"]) == hg.instance_digest(c["inst"])


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", SHAPES)
def test_binding(ctx, n, k):
    c = case(ctx, n, k)
    proof, cm = c["bound"][3]
    # another root: one byte flipped (first, last)
    for at in (0, 31):
        root = bytearray(cm.root)
        root[at] ^= 1
        ok, why, _ = both(ctx, c, proof, bytes(root), 3)
        assert not ok and why
    # another instance: one coefficient of a changed to another in-range value (first word, last word)
    a, ct0 = c["inst"].coeffs()
    for at in (0, a.size - 1):
        a2 = a.copy()
        a2[at] = 1 if a2[at] != 1 else 2
        ok, why, _ = both(ctx, c, proof, cm.root, 3, hg.Instance.from_ciphertext(c["bfv"].params, a2, ct0))
        assert not ok and why
    # another mode
    ok, why, _ = both(ctx, c, proof, cm.root, 1)
    assert not ok and why
    ok, why, _ = both(ctx, c, c["bound"][1][0], c["bound"][1][1].root, 3)
    assert not ok and why
    # an unbound proof of the same values against the bound verifiers, and the bound proof against the unbound ones
    for mode in (1, 3):
        unbound = hg.prove_resident_mode(ctx, c["pk"], c["vals"], hg.ProofBuffer(), mode).bytes()
        assert hg.verify_public(c["pk"], c["inst"], unbound, mode)[0]
        ok, why, _ = both(ctx, c, unbound, cm.root, mode)
        assert not ok and why
        h = hg.verify_public(c["pk"], c["inst"], c["bound"][mode][0], mode)
        d = hg.verify_public(c["pk"], c["inst"], c["bound"][mode][0], mode, ctx=ctx, device=True)
        assert not h[0] and h[1] and h[:2] == d[:2]


@pytest.mark.gpu
def test_nothing_else_moved(ctx):
    c = case(ctx, 1024, 1)
    for mode in (1, 3):
        before = hg.prove_resident_mode(ctx, c["pk"], c["vals"], hg.ProofBuffer(), mode).bytes()
        want = orclib.prove_f("goldilocks", orclib.params(1024, 1), orclib.Inputs(c["w"].arrays()), threads=8, mode=mode)[0]
        assert before == want   # the oracle's bytes: an empty seed leaves every proof byte as it is
        out, cm = hg.prove_committed_mode(ctx, c["pk"], c["vals"], hg.ProofBuffer(), mode)
        assert out.bytes() == c["bound"][mode][0] and cm.root == c["bound"][mode][1].root   # deterministic
        assert hg.prove_resident_mode(ctx, c["pk"], c["vals"], hg.ProofBuffer(), mode).bytes() == before
    mode0 = hg.prove_resident(ctx, c["pk"], c["vals"], hg.ProofBuffer()).bytes()
    assert hg.verify_public(c["pk"], c["inst"], mode0, 0)[0]


@pytest.mark.gpu
def test_errors_leave_no_handle(ctx):
    c = case(ctx, 1024, 1)
    small = hg.ProofBuffer(cap=64)
    with pytest.raises(hg.HgError, match=r"^hg_prove_committed_mode: proof buffer too small"):
        hg.prove_committed_mode(ctx, c["pk"], c["vals"], small, 3)
    assert small.len.value > 64   # the need is reported
    with pytest.raises(hg.HgError, match=r"^hg_prove_committed_mode: .*log2_row"):
        hg.prove_committed_mode(ctx, c["pk"], c["vals"], hg.ProofBuffer(), 3, log2_row=25)
    with pytest.raises(hg.HgError, match=r"^hg_prove_committed_mode: binding needs the absorbing transcript \(mode bit 1\)$"):
        hg.prove_committed_mode(ctx, c["pk"], c["vals"], hg.ProofBuffer(), 2)
    for rank in (0, 1):   # a rank's share is refused: an input the call reads is not resident, or the prover sees whose tables they are
        share = hg.witness_gen_shard(ctx, c["pk"], c["w"], rank, 2)
        with pytest.raises(hg.HgError, match=r"^hg_prove_committed_mode: .*(not resident|of rank)"):
            hg.prove_committed_mode(ctx, c["pk"], share, hg.ProofBuffer(), 3)
        share.free()
    # a values object refilled in place (hg_witness_gen_into) proves the new witness
    w2 = hg.Witness.synthetic(c["bfv"].params, 0xb0d + 99)
    vals2 = hg.witness_gen(ctx, c["pk"], c["w"])
    hg.witness_gen_into(ctx, c["pk"], w2, vals2)
    out, cm = hg.prove_committed_mode(ctx, c["pk"], vals2, hg.ProofBuffer(), 3)
    inst2 = hg.Instance.from_witness(w2)
    assert hg.verify_public_bound(c["pk"], inst2, out.bytes(), cm.root, 3)[0]
    assert not hg.verify_public_bound(c["pk"], c["inst"], out.bytes(), cm.root, 3)[0]
    vals2.free()


@pytest.mark.gpu
def test_full_size_once(ctx):
    """n=32768 k=16, mode 3: prove, both verifiers, open, verify"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x8000 + 17)
    vals = hg.witness_gen(ctx, pk, w)
    inst = hg.Instance.from_witness(w)
    out, cm = hg.prove_committed_mode(ctx, pk, vals, hg.ProofBuffer(cap=1 << 25), 3)
    proof = out.bytes()
    assert hg.values_instance_digest(ctx, pk, vals) == hg.instance_digest(inst) == hg.instance_digest(inst, ctx)
    c = dict(pk=pk, inst=inst)
    ok, why, cl = both(ctx, c, proof, cm.root, 3)
    assert ok, why
    assert cl.n == 47
    opening = cm.open_claims(bfv.params, cl)
    assert hg.claims_verify(bfv.params, cm.root, cl, opening) == (True, "")
    root = bytearray(cm.root)
    root[7] ^= 0x10
    assert not both(ctx, c, proof, bytes(root), 3)[0]
    vals.free()
    pk.free()
