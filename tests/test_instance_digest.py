"""hg_instance_digest / hg_instance_digest_batch / hg_values_instance_digest / hg_bound_seed: the statement digest of a public instance
(the Keccak tree include/hg.h fixes byte for byte) and the bytes a bound transcript starts from. The yardstick is a recomputation in
Python with the oracle's Keccak-256; the device, batch and laid-out forms must give the host form's bytes."""
import ctypes as C
import os
import random
import re
import struct

import numpy as np
import pytest

import orclib
from hglib import hg, ROOT, have_gpu

NEW = ["hg_instance_digest", "hg_instance_digest_batch", "hg_values_instance_digest", "hg_bound_seed", "hg_prove_committed_mode", "hg_verify_public_bound",
       "hg_verify_public_bound_device"]
Q1 = orclib.constants(1024, 1)["qis"]
Q2 = orclib.constants(4096, 2)["qis"]
# (n, k, moduli or None for the built-in set): 64 words = one short leaf, 128 = exactly one full leaf, 256 = two leaves (a | ct0), the
# built-in (1024, 1) = 16 leaves, a derived (1024, 2) = 32 leaves with a modulus boundary inside each table
SETS = [(32, 1, Q1), (64, 1, Q1), (64, 2, Q2), (1024, 1, None), (1024, 2, Q2)]


def params_of(n, k, qis):
    return hg.params_builtin(n, k) if qis is None else hg.params_derive(n, k, qis, 65537)


def edge_instance(params, seed):
    """random in-range coefficients with 0, -1, +(q_i-1)/2 and -(q_i-1)/2 on the first and last word of every leaf and modulus block"""
    n, k = params.n, params.k
    rng = random.Random(seed)
    B = min(128, 2 * k * n)
    out = []
    turn = 0
    for _ in range(2):
        t = np.zeros(k * n, dtype=np.int64)
        for i in range(k):
            half = (params.qis[i] - 1) // 2
            t[i * n:(i + 1) * n] = [rng.randint(-half, half) for _ in range(n)]
            edges = [0, -1, half, -half]
            marks = {0, n - 1} | {j for j in range(n) if (i * n + j) % B in (0, B - 1)}
            for j in sorted(marks):
                t[i * n + j] = edges[turn % 4]
                turn += 1
        out.append(t)
    return out


def py_digest(a, ct0):
    """the definition of include/hg.h, written out independently of the library"""
    words = [int(x) for x in a] + [int(x) for x in ct0]
    B = min(128, len(words))
    level = [orclib.keccak256(struct.pack("<Q", 2) + b"".join(struct.pack("<q", w) for w in words[j * B:(j + 1) * B])) for j in range(len(words) // B)]
    while len(level) > 1:
        level = [orclib.keccak256(struct.pack("<Q", 1) + level[2 * i] + level[2 * i + 1]) for i in range(len(level) // 2)]
    return level[0]


_CASES = {}


def case(n, k, qis):
    """per parameter set: the edge instance, its handle and the Python digest (computed once, never changed)"""
    if (n, k) not in _CASES:
        params = params_of(n, k, qis)
        a, ct0 = edge_instance(params, 0xd16e57 + n + k)
        _CASES[(n, k)] = dict(params=params, a=a, ct0=ct0, inst=hg.Instance.from_ciphertext(params, a, ct0), want=py_digest(a, ct0))
    return _CASES[(n, k)]


def _last():
    return hg.lib().hg_last_error().decode()


# ---- not GPU ----------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    for py in ("instance_digest", "instance_digest_batch", "values_instance_digest", "bound_seed", "prove_committed_mode", "verify_public_bound"):
        assert callable(getattr(hg, py)), py


@pytest.mark.parametrize("n,k,qis", SETS)
def test_host_digest_equals_the_definition(n, k, qis):
    c = case(n, k, qis)
    assert len(c["want"]) == 32
    assert hg.instance_digest(c["inst"]) == c["want"]


@pytest.mark.parametrize("n,k,qis", SETS)
def test_digest_depends_on_every_part_of_the_instance(n, k, qis):
    c = case(n, k, qis)
    params, a, ct0 = c["params"], c["a"], c["ct0"]
    seen = {c["want"]}
    for tab, at in ((0, 0), (0, k * n - 1), (1, 0), (1, k * n - 1), (0, k * n // 2)):
        t = [a.copy(), ct0.copy()]
        t[tab][at] = 1 if t[tab][at] != 1 else 2   # another in-range value
        d = hg.instance_digest(hg.Instance.from_ciphertext(params, t[0], t[1]))
        assert d == py_digest(t[0], t[1]) and d not in seen, (tab, at)
        seen.add(d)
    swapped = hg.instance_digest(hg.Instance.from_ciphertext(params, ct0, a))
    assert swapped == py_digest(ct0, a) and swapped not in seen


def py_seed(params, mode, digest, root):
    return (b"hg-gkr-bound-1" + struct.pack("<II", params.n, params.k) + b"".join(struct.pack("<Q", params.qis[i]) for i in range(params.k)) + struct.pack("<I", mode)
            + digest + root)


@pytest.mark.parametrize("n,k,qis", [(1024, 1, None), (1024, 2, Q2)])
def test_bound_seed_is_the_documented_byte_string(n, k, qis):
    c = case(n, k, qis)
    root = bytes(range(100, 132))
    for mode in (1, 3):
        got = hg.bound_seed(c["params"], mode, c["want"], root)
        assert got == py_seed(c["params"], mode, c["want"], root) and len(got) == 90 + 8 * k
    for mode in (0, 2):
        with pytest.raises(hg.HgError, match=r"^hg_bound_seed: binding needs the absorbing transcript \(mode bit 1\)$"):
            hg.bound_seed(c["params"], mode, c["want"], root)


def test_bad_arguments_are_errors_that_begin_with_the_function():
    c = case(1024, 1, None)
    L, inst, params = hg.lib(), c["inst"], c["params"]
    out, n = (C.c_uint8 * 256)(), C.c_size_t(7)
    d, r = c["want"], bytes(32)

    def fails(name, *args):
        assert getattr(L, name)(*args) == -1, (name, args)
        assert _last().startswith(name + ": "), (name, _last())
        return _last()
    fails("hg_instance_digest", None, None, out)
    fails("hg_instance_digest", None, inst.h, None)
    hs = (C.c_void_p * 2)(inst.h, inst.h)
    assert "no context" in fails("hg_instance_digest_batch", None, hs, 2, out)
    fails("hg_instance_digest_batch", None, None, 2, out)
    fails("hg_instance_digest_batch", None, hs, 2, None)
    assert L.hg_instance_digest_batch(None, None, 0, None) == 0   # an empty run
    fails("hg_values_instance_digest", None, None, None, out)
    pk = hg.BfvEncrypt(params).setup(None)
    assert "no context" in fails("hg_values_instance_digest", None, pk.h, inst.h, out)   # (the stand-in for the values is never read: no context)
    for args in ((None, 3, d, r, out, 256, C.byref(n)), (C.byref(params), 3, None, r, out, 256, C.byref(n)), (C.byref(params), 3, d, None, out, 256, C.byref(n)),
                 (C.byref(params), 3, d, r, out, 256, None), (C.byref(params), 4, d, r, out, 256, C.byref(n)), (C.byref(params), -1, d, r, out, 256, C.byref(n)),
                 (C.byref(params), 3, d, r, None, 256, C.byref(n)), (C.byref(params), 3, d, r, out, 97, C.byref(n))):
        fails("hg_bound_seed", *args)
    assert n.value == 98   # the length is reported when the room is too small
    bad = hg.HgParams()
    bad.n, bad.k = 1000, 1
    fails("hg_bound_seed", C.byref(bad), 3, d, r, out, 256, C.byref(n))
    # the prover: the mode rule comes first, then the checks of hg_secrets_commit_values
    ln, h, root = C.c_size_t(0), C.c_void_p(5), (C.c_uint8 * 32)()
    for mode in (0, 2):
        assert fails("hg_prove_committed_mode", None, None, None, mode, 0, out, 256, C.byref(ln), C.byref(h), root, None).endswith("binding needs the absorbing transcript (mode bit 1)")
        assert h.value is None
    fails("hg_prove_committed_mode", None, None, None, 5, 0, out, 256, C.byref(ln), C.byref(h), root, None)
    assert "null argument" in fails("hg_prove_committed_mode", None, None, None, 3, 0, out, 256, C.byref(ln), C.byref(h), root, None)
    assert "no context" in fails("hg_prove_committed_mode", None, pk.h, inst.h, 3, 0, out, 256, C.byref(ln), C.byref(h), root, None)
    # the verifiers
    nc, nco = hg.pk_claim_shape(pk)
    claims, pts = (hg.HgInputClaim * nc)(), np.zeros(2 * nco, dtype=np.uint64)
    proof = b"\0" * 64
    good = (pk.h, inst.h, 3, r, proof, len(proof), claims, nc, hg._ptr(pts), nco, C.byref(n))

    def sub(i, v):
        return good[:i] + (v,) + good[i + 1:]
    other = hg.Instance.from_witness(hg.Witness.synthetic(hg.params_builtin(2048, 1), 5))
    for args in (sub(0, None), sub(1, None), sub(3, None), sub(4, None), sub(10, None), sub(2, 4), sub(2, -1), sub(2, 0), sub(2, 2), sub(7, nc - 1), sub(9, nco - 1), sub(1, other.h)):
        n.value = 7
        why = fails("hg_verify_public_bound", *args)
        assert args[10] is None or n.value == 0
        if args[2] in (0, 2):
            assert why == "hg_verify_public_bound: binding needs the absorbing transcript (mode bit 1)"
        fails("hg_verify_public_bound_device", None, *args)   # no context
    assert L.hg_verify_public_bound(*good) == 1   # well-formed arguments, a proof that is none: a decision, not an error
    if have_gpu():
        ctx = hg.Context(0)
        try:
            fails("hg_verify_public_bound_device", ctx.h, *good)      # a host-only key
            fails("hg_values_instance_digest", ctx.h, pk.h, inst.h, out)   # (the key is tested ahead of the values)
            other_inst = case(64, 1, Q1)["inst"]
            mixed = (C.c_void_p * 2)(inst.h, other_inst.h)
            assert "mixed parameters" in fails("hg_instance_digest_batch", ctx.h, mixed, 2, out)
            holes = (C.c_void_p * 2)(inst.h, None)
            fails("hg_instance_digest_batch", ctx.h, holes, 2, out)
        finally:
            ctx.close()
    pk.free()


def test_unbound_oracle_proof_is_rejected_by_the_bound_verifier():
    """the CPU oracle's mode-3 proof of the fixture is accepted by hg_verify_public and - being unbound - rejected by hg_verify_public_bound"""
    bfv = hg.BfvEncrypt.new(1024, 1)
    w = bfv.get_inputs(os.path.join(orclib.GOLDEN, "sk_enc_1024_1x27_65537.json"))
    proof = orclib.prove_f("goldilocks", orclib.params(1024, 1), orclib.Inputs(w.arrays()), threads=8, mode=3)[0]
    pk, inst = bfv.setup(None), hg.Instance.from_witness(w)
    assert hg.verify_public(pk, inst, proof, 3)[0]
    root = hg.Commitment.secrets(None, bfv.params, w).root
    ok, why, cl = hg.verify_public_bound(pk, inst, proof, root, 3)
    assert not ok and why and cl is None
    pk.free()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,qis", SETS)
def test_device_and_batch_digests_equal_the_host_form(ctx, n, k, qis):
    c = case(n, k, qis)
    assert hg.instance_digest(c["inst"], ctx) == c["want"]
    assert hg.instance_digest_batch(ctx, [c["inst"]]) == [c["want"]]
    # three different members through one launch: the member stride
    others = []
    for s in (1, 2):
        a, ct0 = edge_instance(c["params"], 0xbeef + s)
        others.append((hg.Instance.from_ciphertext(c["params"], a, ct0), py_digest(a, ct0)))
    got = hg.instance_digest_batch(ctx, [others[0][0], c["inst"], others[1][0]])
    assert got == [others[0][1], c["want"], others[1][1]] and len(set(got)) == 3
    assert hg.instance_digest_batch(ctx, []) == []


def laid_out_case(ctx, n, k, qis, w=None):
    bfv = hg.BfvEncrypt(params_of(n, k, qis))
    pk = bfv.setup(ctx)
    w = w or hg.Witness.synthetic(bfv.params, 0x1a1d + k)
    return bfv, pk, w, hg.witness_gen(ctx, pk, w)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,qis,fixture", [(1024, 1, None, True), (1024, 2, Q2, False)])
def test_laid_out_digest_equals_the_host_form(ctx, n, k, qis, fixture):
    w = hg.BfvEncrypt.new(n, k).get_inputs(os.path.join(orclib.GOLDEN, "sk_enc_1024_1x27_65537.json")) if fixture else None
    bfv, pk, w, vals = laid_out_case(ctx, n, k, qis, w)
    inst = hg.Instance.from_witness(w)
    want = py_digest(*inst.coeffs())
    assert hg.instance_digest(inst) == want
    assert hg.values_instance_digest(ctx, pk, vals) == want
    assert hg.instance_digest(inst, ctx) == want
    vals.free()
    pk.free()


@pytest.mark.gpu
def test_laid_out_digest_refuses_what_is_not_an_instance(ctx):
    bfv, pk, w, vals = laid_out_case(ctx, 1024, 2, Q2)
    n, half1 = 1024, (Q2[1] - 1) // 2
    # values of another key
    pk2 = bfv.setup(ctx)
    with pytest.raises(hg.HgError, match=r"^hg_values_instance_digest: .*another prover key"):
        hg.values_instance_digest(ctx, pk2, vals)
    pk2.free()
    # a word out of range: coefficient 0 of a_1 (word n-1 of its table) one above (q_1 - 1) / 2, then the largest "positive" word
    for word in (half1 + 1, hg.P // 2):
        d = {f: v.copy() for f, v in w.arrays().items()}
        d["ais"][2 * n + n - 1] = word
        hg.witness_gen_into(ctx, pk, hg.Witness.from_arrays(bfv.params, d), vals)
        with pytest.raises(hg.HgError, match=r"^hg_values_instance_digest: .*not a signed value"):
            hg.values_instance_digest(ctx, pk, vals)
    d = {f: v.copy() for f, v in w.arrays().items()}
    d["ct0is"][2 * n + 2 * n - 2] = hg.P - half1 - 1   # coefficient 0 of ct0_1 one below -(q_1 - 1) / 2
    hg.witness_gen_into(ctx, pk, hg.Witness.from_arrays(bfv.params, d), vals)
    with pytest.raises(hg.HgError, match=r"^hg_values_instance_digest: .*not a signed value"):
        hg.values_instance_digest(ctx, pk, vals)
    hg.witness_gen_into(ctx, pk, w, vals)   # ... and the same tables with the witness back in them are digested again
    assert hg.values_instance_digest(ctx, pk, vals) == hg.instance_digest(hg.Instance.from_witness(w))
    vals.free()
    # a rank's share: some public input is resident on one of the two ranks only
    seen = []
    for rank in (0, 1):
        share = hg.witness_gen_shard(ctx, pk, w, rank, 2)
        try:
            hg.values_instance_digest(ctx, pk, share)
            seen.append("")
        except hg.HgError as e:
            assert str(e).startswith("hg_values_instance_digest: ") and "not resident" in str(e)
            seen.append(str(e))
        share.free()
    assert any(seen)
    pk.free()
