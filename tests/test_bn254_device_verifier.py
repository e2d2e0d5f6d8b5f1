"""hg_verify_device_bn254: BfvEncrypt::verify over bn256::Fr with the table-sized work on the device (bn254_verify.inc). The host
verifier hg_verify_bn254 is the yardstick: every proof, tampered or not, gets the same accept / reject decision from both."""
import ctypes as C
import os
import random
import re
import statistics
import time

import pytest

import orclib
from orclib import P
from hglib import hg, ROOT, have_gpu


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hg.h")).read()
    assert re.search(r"int\s+hg_verify_device_bn254\s*\(\s*hg_ctx\s*\*\s*ctx\s*,\s*const\s+hg_pk\s*\*\s*pk\s*,\s*const\s+hg_witness\s*\*\s*w\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*proof\s*,\s*size_t\s+len\s*\)\s*;", hdr)
    assert "hg_verify_device_bn254" in hg.EXPORTS
    assert hasattr(hg.lib(), "hg_verify_device_bn254")
    assert "hg_verify_device_bn254" in open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()


def test_host_only_key_or_null_context_is_an_error_naming_the_function():
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(None)   # host-only key
    w = hg.Witness.synthetic(bfv.params, 7)
    L = hg.lib()
    L.hg_verify_device_bn254.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.hg_verify_device_bn254.restype = C.c_int
    proof = bytes(32 * 64)
    assert L.hg_verify_device_bn254(None, pk.h, w.h, proof, len(proof)) == -1
    assert "hg_verify_device_bn254" in L.hg_last_error().decode()
    with pytest.raises(hg.HgError, match="hg_verify_device_bn254"):
        hg.verify_device_bn254(None, pk, w, proof)
    if have_gpu():   # a device context with a host-only key: still an error
        ctx = hg.Context(0)
        try:
            with pytest.raises(hg.HgError, match="hg_verify_device_bn254"):
                hg.verify_device_bn254(ctx, pk, w, proof)
        finally:
            ctx.close()
    pk.free()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def _same_decision(ctx, pk, w, proof):
    dh = hg.verify_bn254(pk, w, proof)[0]
    dd = hg.verify_device_bn254(ctx, pk, w, proof)[0]
    assert dh == dd, (dh, dd)
    return dd


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2), (32768, 16)])
def test_device_verifier_bn254_agrees_with_the_host_verifier(ctx, n, k):
    """The proof of hg_prove_bn254 is accepted by the device and the host verifier (and by the oracle's at n=1024); another witness
    is rejected; tampered proofs (bit flips, non-canonical elements, truncation, a trailing element) get the same decision from both."""
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x6e3 + n)
    w2 = hg.Witness.synthetic(bfv.params, 0x6e4 + n)
    proof, _, _ = ctx.prove_bn254(pk, w, cap=1 << 25)
    ok, why = hg.verify_device_bn254(ctx, pk, w, proof)
    assert ok, why
    assert hg.verify_bn254(pk, w, proof) == (True, "")
    if n == 1024:
        ok, err = orclib.verify_f("bn254", orclib.params(n, k), orclib.Inputs(w.arrays()), proof, threads=8)
        assert ok, err
    # a proof checked against another witness: the input claims fail
    ok2, why2 = hg.verify_device_bn254(ctx, pk, w2, proof)
    assert not ok2 and why2
    assert not hg.verify_bn254(pk, w2, proof)[0]
    if n == 32768:   # median of 5 after a warm-up, beside the host verifier in the same process
        td, th = [], []
        for i in range(6):
            t0 = time.perf_counter(); hg.verify_device_bn254(ctx, pk, w, proof); t1 = time.perf_counter()
            if i: td.append((t1 - t0) * 1e3)
        for i in range(2):
            t0 = time.perf_counter(); hg.verify_bn254(pk, w, proof); th.append((time.perf_counter() - t0) * 1e3)
        print("n=%d k=%d: hg_verify_device_bn254 %.2f ms (median of 5), hg_verify_bn254 (host) %.1f ms" % (n, k, statistics.median(td), min(th)))
    nel = len(proof) // 32
    rng = random.Random(0xb254 + n)
    # (position, xor mask) or (element, None) = the element's top byte set to 0xff (not a canonical residue)
    muts = [(0, 1), (31, 1), (32 * (nel // 3) + 31, 4), (len(proof) // 2 + 31, 1), (nel // 4, None), (32 * (nel - 2) + 31, 2),
            (len(proof) - 1, 1), (32 * (nel // 5) + 17, 8)]
    muts += [(rng.randrange(len(proof)), 1 << rng.randrange(8)) for _ in range(2 if n == 32768 else 4)]
    if n < 32768:
        muts += [(rng.randrange(nel), None), (32 * rng.randrange(nel) + 31, 1 << rng.randrange(8)),
                 (32 * rng.randrange(nel), 0x80), (32 * (nel - 1), 0xff)]
    assert len(muts) >= (8 if n == 32768 else 14)
    for pos, mask in muts:   # (every element of the stream is bound: tests/test_proof_binding.py)
        bad = bytearray(proof)
        if mask is None:
            bad[32 * pos] = 0xff
        else:
            bad[pos] ^= mask
        assert not _same_decision(ctx, pk, w, bytes(bad)), (pos, mask)
    assert not _same_decision(ctx, pk, w, proof[:len(proof) // 2])   # truncated
    _same_decision(ctx, pk, w, proof[:-32])
    assert _same_decision(ctx, pk, w, proof + bytes(32))               # a trailing zero element is ignored, as by the host verifier
    assert hg.verify_device_bn254(ctx, pk, w, proof) == (True, "")     # and the context is still good
    pk.free()


def _tampered_witness(bfv, kind):
    """A synthetic n=1024 witness made invalid: "range" = an error coefficient outside its range-check bound (the Lasso lookup then
    returns the wrong sub-table value); "relation" = one ct0 coefficient changed (the circuit relation fails)."""
    d = {f: a.copy() for f, a in hg.Witness.synthetic(bfv.params, 4242).arrays().items()}
    if kind == "range":
        d["e"][5] = 1000          # e_bound = 19
    else:
        d["ct0is"][7] = (int(d["ct0is"][7]) + 1) % P
    return hg.Witness.from_arrays(bfv.params, d)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["range", "relation"])
def test_device_verifier_bn254_rejects_invalid_witness_proofs(ctx, kind):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    w = _tampered_witness(bfv, kind)
    proof, _, _ = ctx.prove_bn254(pk, w)
    ok_h, _ = hg.verify_bn254(pk, w, proof)
    ok_d, why = hg.verify_device_bn254(ctx, pk, w, proof)
    assert not ok_h and not ok_d and why
    pk.free()


@pytest.mark.gpu
def test_device_verifier_bn254_leaves_a_shared_context_undisturbed(ctx):
    """One context: graph-replayed Goldilocks resident proves, BN254 proves, BN254 device verifies and Goldilocks device verifies,
    interleaved. Every proof stays byte-identical to the one made before the first BN254 device verify; every verifier accepts."""
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(ctx)
    w_gl = hg.Witness.synthetic(bfv.params, 0x5151)
    w_bn = hg.Witness.synthetic(bfv.params, 0x5152)
    vals = hg.witness_gen(ctx, pk, w_gl)
    out = hg.ProofBuffer()
    gl = [hg.prove_resident(ctx, pk, vals, out).bytes() for _ in range(4)]   # from the third on: the recorded launch graph
    assert gl[0] == gl[1] == gl[2] == gl[3]
    gl0 = gl[0]
    bn0, _, _ = ctx.prove_bn254(pk, w_bn)
    assert hg.verify_bn254(pk, w_bn, bn0) == (True, "")
    assert hg.verify_device(ctx, pk, w_gl, gl0) == (True, "")
    for i in range(3):
        assert hg.prove_resident(ctx, pk, vals, out).bytes() == gl0, i
        assert ctx.prove_bn254(pk, w_bn)[0] == bn0, i
        assert hg.verify_device_bn254(ctx, pk, w_bn, bn0) == (True, ""), i
        assert hg.verify_device(ctx, pk, w_gl, gl0) == (True, ""), i
        assert hg.prove_resident(ctx, pk, vals, out).bytes() == gl0, i
    assert hg.prove_resident(ctx, pk, vals, out).bytes() == gl0
    assert hg.verify(pk, w_gl, gl0) == (True, "")
    vals.free()
    pk.free()
