"""hg_verify_device_batch: a run of proofs under one key verified in device passes of a group of proofs each (verifier_batch.hip).
The single-proof entry is the yardstick: every (witness, proof) pair of a batch gets the decision and the reason string that
hg_verify_device_mode gives it alone (and the decision of hg_verify_mode on the host)."""
import ctypes as C
import os
import random
import re

import pytest

import orclib
from hglib import hg, ROOT, have_gpu

ENTRY = "hg_verify_device_batch"
CAP = 256


def _entry():
    f = getattr(hg.lib(), ENTRY)
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int,
                  C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    f.restype = C.c_int
    return f


def _single(ctx, pk, w, proof, mode):
    ok, why = hg.verify_device(ctx, pk, w, proof, mode=mode)
    return ok, why


def _batch_matches_singles(ctx, pk, ws, proofs, mode, host=True):
    got = hg.verify_device_batch(ctx, pk, ws, proofs, mode=mode)
    assert len(got) == len(proofs)
    for i, (w, p) in enumerate(zip(ws, proofs)):
        want = _single(ctx, pk, w, p, mode)
        assert got[i] == want, (mode, i, got[i], want)
        if host:
            assert hg.verify(pk, w, p, mode=mode)[0] == want[0], (mode, i)
    return got


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hg.h")).read()
    assert re.search(r"int\s+hg_verify_device_batch\s*\(\s*hg_ctx\s*\*\s*ctx\s*,\s*const\s+hg_pk\s*\*\s*pk\s*,\s*const\s+hg_witness\s*\*\s*const\s*\*\s*ws\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*const\s*\*\s*proofs\s*,\s*const\s+size_t\s*\*\s*lens\s*,\s*size_t\s+n\s*,\s*int\s+mode\s*,"
                     r"\s*int\s*\*\s*results\s*,\s*char\s*\*\s*reasons\s*,\s*size_t\s+reason_cap\s*\)\s*;", hdr)
    assert '"verify_batch_group"' in hdr
    assert ENTRY in hg.EXPORTS
    assert hasattr(hg.lib(), ENTRY)
    assert re.search(r"pub fn hg_verify_device_batch\(", open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read())


def _raw_call(ctx_h, pk_h, ws, proofs, mode, n=None, results=True):
    n = len(proofs) if n is None else n
    W = (C.c_void_p * max(len(ws), 1))(*ws)
    P = (C.c_char_p * max(len(proofs), 1))(*proofs)
    N = (C.c_size_t * max(len(proofs), 1))(*[len(p) if p else 0 for p in proofs])
    R = (C.c_int * max(n, 1))(*([7] * max(n, 1)))
    reasons = C.create_string_buffer(b"\x55" * (max(n, 1) * CAP), max(n, 1) * CAP)
    rc = _entry()(ctx_h, pk_h, W, P, N, n, mode, R if results else None, reasons, CAP)
    return rc, list(R), reasons.raw


def test_bad_arguments_are_errors_naming_the_function():
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(None)   # host-only key
    w = hg.Witness.synthetic(bfv.params, 12)
    proof = bytes(16 * 64)
    for mode in (0, 3, -1, 4):
        rc, _, _ = _raw_call(None, pk.h, [w.h.value], [proof], mode)
        assert rc == -1 and ENTRY in hg.lib().hg_last_error().decode(), mode
        with pytest.raises(hg.HgError, match=ENTRY):
            hg.verify_device_batch(None, pk, [w], [proof], mode=mode)
    assert _entry()(None, None, None, None, None, 1, 0, None, None, 0) == -1
    assert ENTRY in hg.lib().hg_last_error().decode()
    if have_gpu():
        ctx = hg.Context(0)
        try:
            rc, _, _ = _raw_call(ctx.h, pk.h, [w.h.value], [proof], 0)   # a device context with a host-only key
            assert rc == -1 and ENTRY in hg.lib().hg_last_error().decode()
            pkd = bfv.setup(ctx)
            try:
                for mode in (-1, 4, 7):   # a device key: only the mode is wrong
                    rc, _, _ = _raw_call(ctx.h, pkd.h, [w.h.value], [proof], mode)
                    msg = hg.lib().hg_last_error().decode()
                    assert rc == -1 and ENTRY in msg and "mode" in msg, (mode, msg)
                for args in (([None], [proof]), ([w.h.value], [None])):   # a null element
                    rc, _, _ = _raw_call(ctx.h, pkd.h, *args, 0)
                    assert rc == -1 and ENTRY in hg.lib().hg_last_error().decode()
                rc, _, _ = _raw_call(ctx.h, pkd.h, [w.h.value], [proof], 0, results=False)   # null results
                assert rc == -1 and ENTRY in hg.lib().hg_last_error().decode()
                other = hg.Witness.synthetic(hg.BfvEncrypt.new(2048, 1).params, 3)   # a witness of another parameter set
                rc, _, _ = _raw_call(ctx.h, pkd.h, [w.h.value, other.h.value], [proof, proof], 0)
                assert rc == -1 and ENTRY in hg.lib().hg_last_error().decode()
            finally:
                pkd.free()
        finally:
            ctx.close()
    pk.free()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def _tampered(proof, seed):
    """one flipped byte at several positions, half the bytes, all but the last 16"""
    rng = random.Random(seed)
    L = len(proof)
    out = []
    for pos in (0, L // 7, L // 3, L // 2, 2 * L // 3, L - 40, L - 1, rng.randrange(L)):
        bad = bytearray(proof)
        bad[pos] ^= 1 << rng.randrange(8)
        out.append(bytes(bad))
    return out + [proof[:L // 2], proof[:-16]]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_batch_matches_the_single_proof_verifier(ctx, n, k, mode):
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xb00 + 16 * n + 4 * mode + i) for i in range(2)]
    honest = [bfv.prove(ctx, pk, w, mode=mode)[0] for w in ws]
    bad = _tampered(honest[0], n + mode)
    proofs = [honest[0]] + bad[:5] + [honest[1]] + bad[5:]
    wits = [ws[0]] * 6 + [ws[1]] + [ws[0]] * (len(bad) - 5)
    got = _batch_matches_singles(ctx, pk, wits, proofs, mode)
    assert got[0] == (True, "") and got[6] == (True, "")
    assert [i for i, (ok, _) in enumerate(got) if ok] == [0, 6]   # every tampered proof is rejected (tests/test_proof_binding.py: every element is bound)
    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_no_cross_wiring_between_the_proofs_of_a_batch(ctx, mode):
    """Mode 0 shares every table that depends on the key only: a witness's input evaluations must never be shared."""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xc00 + 8 * mode + i) for i in range(4)]
    ps = [bfv.prove(ctx, pk, w, mode=mode)[0] for w in ws]
    wits = [ws[(i + 1) % 4] for i in range(4)] + ws + [ws[2], ws[2]]
    proofs = ps + ps + [ps[2], ps[2]]
    got = _batch_matches_singles(ctx, pk, wits, proofs, mode, host=False)
    for i in range(4):
        ok, why = got[i]
        assert not ok and (why.startswith("input claim mismatch") or why.startswith("InvalidSumCheck")), (i, why)
        assert got[4 + i] == (True, ""), i
    assert got[8] == got[9] == (True, "")
    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_group_boundaries_do_not_change_the_results(ctx, mode):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xd00 + 8 * mode + i) for i in range(8)]
    ps = [bfv.prove(ctx, pk, w, mode=mode)[0] for w in ws]
    ps[0] = ps[0][:len(ps[0]) // 2]
    ps[7] = _tampered(ps[7], 2)[2]
    wits = list(ws)
    wits[6] = ws[5]                         # (a mismatched pair in the last group too)
    one = hg.verify_device_batch(ctx, pk, wits, ps, mode=mode)
    try:
        ctx.set_option("verify_batch_group", 3)
        three = hg.verify_device_batch(ctx, pk, wits, ps, mode=mode)
    finally:
        ctx.set_option("verify_batch_group", 0)
    assert three == one
    assert not one[0][0] and not one[6][0] and all(one[i][0] for i in (1, 2, 3, 4, 5)), one   # (proof 7: as the single call decides)
    for i, (w, p) in enumerate(zip(wits, ps)):
        assert one[i] == _single(ctx, pk, w, p, mode), i
    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_headline_size_batch_of_eight(ctx, mode):
    n, k = 32768, 16
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0x8000 + 16 + 32 * mode + i) for i in range(8)]
    ps = [bfv.prove(ctx, pk, w, cap=1 << 25, mode=mode)[0] for w in ws]
    L = len(ps[0])
    bad = bytearray(ps[2])
    bad[L // 3] ^= 4
    ps[2] = bytes(bad)
    ps[5] = ps[5][:L // 2]
    got = _batch_matches_singles(ctx, pk, ws, ps, mode, host=False)
    assert [ok for i, (ok, _) in enumerate(got) if i != 2] == [True, True, True, True, False, True, True], got   # (proof 2: as the single call decides)
    pk.free()


@pytest.mark.gpu
def test_the_context_stays_usable(ctx):
    """A batch uses the arena, the result buffer and a stream of its own: resident proves around it (the later ones replays of the
    recorded launch graph) stay byte-identical, and hg_verify_device still accepts afterwards."""
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0xe00)
    vals = hg.witness_gen(ctx, pk, w)
    out = hg.ProofBuffer()
    first = [hg.prove_resident(ctx, pk, vals, out).bytes() for _ in range(3)]
    assert first[0] == first[1] == first[2]
    p3 = bfv.prove(ctx, pk, w, mode=3)[0]
    for mode, p in ((0, first[0]), (3, p3)):
        assert hg.verify_device_batch(ctx, pk, [w, w], [p, p[:-16]], mode=mode)[0] == (True, "")
        assert hg.prove_resident(ctx, pk, vals, out).bytes() == first[0], mode
        assert hg.verify_device(ctx, pk, w, first[0]) == (True, "")
        assert hg.verify_device(ctx, pk, w, p3, mode=3) == (True, "")
    vals.free()
    pk.free()


@pytest.mark.gpu
def test_an_empty_batch_returns_0_and_writes_nothing(ctx):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    for mode in (0, 3):
        rc, res, reasons = _raw_call(ctx.h, pk.h, [], [], mode, n=0)
        assert rc == 0
        assert res == [7] and reasons == b"\x55" * CAP
        assert hg.verify_device_batch(ctx, pk, [], [], mode=mode) == []
    pk.free()
