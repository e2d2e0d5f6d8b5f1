"""hg_verify_device_mode: the device verifier (verifier_dev.hip) in the protocol modes of hg_prove_mode / hg_verify_mode. The host
verifier hg_verify_mode is the yardstick: every proof, honest or tampered, checked in any mode, gets the same accept / reject
decision from both; mode 0 through the new entry is hg_verify_device."""
import ctypes as C
import os
import random
import re
import statistics
import subprocess
import sys
import time

import pytest

import orclib
from hglib import hg, ROOT, have_gpu

ENTRY = "hg_verify_device_mode"


def _entry():
    L = hg.lib()
    f = getattr(L, ENTRY)
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    f.restype = C.c_int
    return f


def _dev(ctx, pk, w, proof, mode):
    """hg_verify_device_mode itself (mode 0 included): True / False, an error raises."""
    rc = _entry()(ctx.h, pk.h, w.h, mode, proof, len(proof))
    if rc < 0:
        raise hg.HgError(hg.lib().hg_last_error().decode())
    return rc == 0


def _same_decision(ctx, pk, w, proof, mode):
    dh = hg.verify(pk, w, proof, mode=mode)[0]
    dd = _dev(ctx, pk, w, proof, mode)
    assert dh == dd, (mode, dh, dd)
    return dd


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hg.h")).read()
    assert re.search(r"int\s+hg_verify_device_mode\s*\(\s*hg_ctx\s*\*\s*ctx\s*,\s*const\s+hg_pk\s*\*\s*pk\s*,\s*const\s+hg_witness\s*\*\s*w\s*,"
                     r"\s*int\s+mode\s*,\s*const\s+uint8_t\s*\*\s*proof\s*,\s*size_t\s+len\s*\)\s*;", hdr)
    assert ENTRY in hg.EXPORTS
    assert hasattr(hg.lib(), ENTRY)
    assert re.search(r"pub fn hg_verify_device_mode\(", open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read())


def test_bad_arguments_are_errors_naming_the_function():
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(None)   # host-only key
    w = hg.Witness.synthetic(bfv.params, 11)
    f = _entry()
    proof = bytes(16 * 64)
    for mode in (0, 1, 2, 3, -1, 4, 7):
        assert f(None, pk.h, w.h, mode, proof, len(proof)) == -1, mode
        assert ENTRY in hg.lib().hg_last_error().decode(), mode
    for mode in (1, 3, -1, 4, 7):
        with pytest.raises(hg.HgError, match=ENTRY):
            hg.verify_device(None, pk, w, proof, mode=mode)
    assert f(None, None, None, 3, None, 0) == -1
    assert ENTRY in hg.lib().hg_last_error().decode()
    if have_gpu():
        ctx = hg.Context(0)
        try:
            for mode in (0, 3):   # a device context with a host-only key
                assert f(ctx.h, pk.h, w.h, mode, proof, len(proof)) == -1, mode
                assert ENTRY in hg.lib().hg_last_error().decode()
                with pytest.raises(hg.HgError, match=ENTRY):
                    hg.verify_device(ctx, pk, w, proof, mode=mode or 1)
            pkd = bfv.setup(ctx)   # a device key: only the mode is wrong
            try:
                for mode in (-1, 4, 7):
                    assert f(ctx.h, pkd.h, w.h, mode, proof, len(proof)) == -1, mode
                    msg = hg.lib().hg_last_error().decode()
                    assert ENTRY in msg and "mode" in msg, msg
                    with pytest.raises(hg.HgError, match=ENTRY):
                        hg.verify_device(ctx, pkd, w, proof, mode=mode)
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


def _flips(proof, n):
    """(position, mask): the positions of test_device_verifier_agrees_with_the_host_verifier plus random ones."""
    rng = random.Random(0x5eed + n)
    L = len(proof)
    pos = [0, 8, L // 5, L // 3, L // 2, 2 * L // 3, L - 40, L - 1]
    pos += [rng.randrange(L) for _ in range(6)]
    return [(p, 1 << rng.randrange(8)) for p in pos]


FIX = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", FIX)
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_device_verifier_in_a_protocol_mode_agrees_with_hg_verify_mode(ctx, n, k, bits, mode):
    """An honest mode-m proof (the oracle's bytes in that mode) is accepted by hg_verify_device_mode and hg_verify_mode; bit flips,
    another witness and truncation get the same decision from both; checked in every other mode m' the decision is again the same,
    and a rejection wherever the transcript bit (1) differs."""
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
    proof, _ = bfv.prove(ctx, pk, w, mode=mode)
    ref, _ = orclib.prove_f("goldilocks", orclib.params(n, k), orclib.Inputs(w.arrays()), threads=8, mode=mode)
    assert proof == ref
    assert hg.verify_device(ctx, pk, w, proof, mode=mode) == (True, "")
    assert hg.verify(pk, w, proof, mode=mode) == (True, "")
    # tampering
    flips = _flips(proof, n)
    assert len(flips) >= 12
    for pos, mask in flips:   # (every element of the stream is bound: tests/test_proof_binding.py)
        bad = bytearray(proof)
        bad[pos] ^= mask
        assert not _same_decision(ctx, pk, w, bytes(bad), mode), (pos, mask)
    w2 = hg.Witness.synthetic(bfv.params, 0x77 + n + mode)
    assert not _same_decision(ctx, pk, w2, proof, mode)                       # another witness
    assert not _same_decision(ctx, pk, w, proof[:len(proof) // 2], mode)      # truncated
    _same_decision(ctx, pk, w, proof[:-16], mode)
    # the modes are not interchangeable
    for other in range(4):
        if other == mode:
            continue
        d = _same_decision(ctx, pk, w, proof, other)
        if (other ^ mode) & 1:
            assert not d, (mode, other)
    assert hg.verify_device(ctx, pk, w, proof, mode=mode) == (True, "")      # and the context is still good
    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
def test_mode_0_through_the_new_entry_is_hg_verify_device(ctx, n, k):
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x300 + n)
    proof, _ = bfv.prove(ctx, pk, w)
    assert _dev(ctx, pk, w, proof, 0) and hg.verify_device(ctx, pk, w, proof) == (True, "")
    for pos, mask in _flips(proof, n):
        bad = bytearray(proof)
        bad[pos] ^= mask
        assert not hg.verify_device(ctx, pk, w, bytes(bad))[0] and not _dev(ctx, pk, w, bytes(bad), 0), pos
    w2 = hg.Witness.synthetic(bfv.params, 0x301 + n)
    assert not _dev(ctx, pk, w2, proof, 0) and not hg.verify_device(ctx, pk, w2, proof)[0]
    pk.free()


@pytest.mark.gpu
def test_a_sound_mode_verification_leaves_the_fixed_chain_alone(ctx):
    """The walk's own challenges are staged into the arena, never over the context's fixed chain: mode-0 proves around a mode-3
    device verification (the later ones replays of the recorded launch graph) stay byte-identical, and every verifier accepts."""
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x4c4b)
    p3, _ = bfv.prove(ctx, pk, w, mode=3)
    first = [bfv.prove(ctx, pk, w)[0] for _ in range(3)]
    assert first[0] == first[1] == first[2]
    p0 = first[0]
    for i in range(2):
        assert hg.verify_device(ctx, pk, w, p3, mode=3) == (True, ""), i
        again, _ = bfv.prove(ctx, pk, w)
        assert again == p0, i
        assert hg.verify_device(ctx, pk, w, p0) == (True, ""), i
        assert _dev(ctx, pk, w, again, 0), i
    assert hg.verify(pk, w, p0) == (True, "")
    assert hg.verify(pk, w, p3, mode=3) == (True, "")
    pk.free()


@pytest.mark.gpu
def test_headline_size_mode_3_device_faster_than_host(ctx):
    n, k = 32768, 16
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x8000 + 16)
    proof, _ = bfv.prove(ctx, pk, w, cap=1 << 25, mode=3)
    assert hg.verify_device(ctx, pk, w, proof, mode=3) == (True, "")
    assert hg.verify(pk, w, proof, mode=3) == (True, "")
    for pos in (len(proof) // 8 + 7, 7 * len(proof) // 8 + 7):   # first and last quarter
        bad = bytearray(proof)
        bad[pos] ^= 0x10
        assert not _same_decision(ctx, pk, w, bytes(bad), 3), pos
    times = {}
    for name, fn in (("device mode 3", lambda: hg.verify_device(ctx, pk, w, proof, mode=3)),
                     ("host mode 3", lambda: hg.verify(pk, w, proof, mode=3))):
        t = []
        for i in range(6):   # a warm-up, then five
            t0 = time.perf_counter()
            assert fn()[0]
            if i:
                t.append((time.perf_counter() - t0) * 1e3)
        times[name] = statistics.median(t)
    print("n=%d k=%d: hg_verify_device_mode(3) %.2f ms, hg_verify_mode(3) (host) %.1f ms (median of 5)" % (n, k, times["device mode 3"], times["host mode 3"]))
    assert times["device mode 3"] < times["host mode 3"], times
    pk.free()


_SHARDED = r"""
import sys, threading
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
hg = entry.load_package()
n, k, world, mode = 1024, 1, 2, 3
bfv = hg.BfvEncrypt.new(n, k)
w = hg.Witness.synthetic(bfv.params, 0x5a4d)
group = hg.Group.local(world)
results, errs = [None] * world, []
def run(r):
    try:
        c = hg.Context(0)
        pk = bfv.setup(c)
        v = hg.witness_gen(c, pk, w)
        out = hg.ProofBuffer()
        hg.prove_resident_mode_sharded(c, pk, v, out, mode, r, group)
        results[r] = out.bytes()
        v.free(); pk.free(); c.close()
    except Exception as e:
        errs.append((r, repr(e)))
ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
for t in ts: t.start()
for t in ts: t.join(300)
assert not errs, errs
assert results[0] is not None and results[0] == results[1]
c = hg.Context(0); pk = bfv.setup(c)
single, _ = bfv.prove(c, pk, w, mode=mode)
assert results[0] == single
assert hg.verify_device(c, pk, w, results[0], mode=mode) == (True, "")
assert hg.verify(pk, w, results[0], mode=mode) == (True, "")
pk.free(); c.close()
print("SHARDED VERIFY OK")
"""


@pytest.mark.gpu
def test_sharded_proof_is_accepted_by_the_device_verifier():
    """A two-rank proof from hg_prove_resident_mode_sharded (hg_group_local(2), one device) is the single-rank proof and is accepted
    (in a child process, as the sharded prover's own tests run it)."""
    code = _SHARDED % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=ROOT)
    assert r.returncode == 0 and "SHARDED VERIFY OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
