"""hg_verify_device_batch_bn254: a run of BN254 proofs under one key verified in device passes of a group of proofs each
(bn254_verify_batch.inc). The single-proof entry is the yardstick: every (witness, proof) pair of a batch gets the decision and the
reason string that hg_verify_device_bn254 gives it alone (and the decision of hg_verify_bn254 on the host)."""
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

ENTRY = "hg_verify_device_batch_bn254"
CAP = 256


def _entry():
    f = getattr(hg.lib(), ENTRY)
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                  C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    f.restype = C.c_int
    return f


def _raw_call(ctx_h, pk_h, ws, proofs, n=None, results=True):
    n = len(proofs) if n is None else n
    W = (C.c_void_p * max(len(ws), 1))(*ws)
    Pp = (C.c_char_p * max(len(proofs), 1))(*proofs)
    N = (C.c_size_t * max(len(proofs), 1))(*[len(p) if p else 0 for p in proofs])
    R = (C.c_int * max(n, 1))(*([7] * max(n, 1)))
    reasons = C.create_string_buffer(b"\x55" * (max(n, 1) * CAP), max(n, 1) * CAP)
    rc = _entry()(ctx_h, pk_h, W, Pp, N, n, R if results else None, reasons, CAP)
    return rc, list(R), reasons.raw


def _batch_matches_singles(ctx, pk, ws, proofs, host=True):
    got = hg.verify_device_batch_bn254(ctx, pk, ws, proofs)
    assert len(got) == len(proofs)
    for i, (w, p) in enumerate(zip(ws, proofs)):
        want = hg.verify_device_bn254(ctx, pk, w, p)
        assert got[i] == want, (i, got[i], want)
        if host:
            assert hg.verify_bn254(pk, w, p)[0] == want[0], i
    return got


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hg.h")).read()
    assert re.search(r"int\s+hg_verify_device_batch_bn254\s*\(\s*hg_ctx\s*\*\s*ctx\s*,\s*const\s+hg_pk\s*\*\s*pk\s*,"
                     r"\s*const\s+hg_witness\s*\*\s*const\s*\*\s*ws\s*,\s*const\s+uint8_t\s*\*\s*const\s*\*\s*proofs\s*,"
                     r"\s*const\s+size_t\s*\*\s*lens\s*,\s*size_t\s+n\s*,\s*int\s*\*\s*results\s*,\s*char\s*\*\s*reasons\s*,"
                     r"\s*size_t\s+reason_cap\s*\)\s*;", hdr)
    assert re.search(r'"verify_batch_group"[^/]*hg_verify_device_batch_bn254', hdr)
    assert ENTRY in hg.EXPORTS
    assert hasattr(hg.lib(), ENTRY)
    assert re.search(r"pub fn hg_verify_device_batch_bn254\(", open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read())


def test_bad_arguments_are_errors_naming_the_function():
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(None)   # host-only key
    w = hg.Witness.synthetic(bfv.params, 12)
    proof = bytes(32 * 64)
    rc, _, _ = _raw_call(None, pk.h, [w.h.value], [proof])   # a null context
    assert rc == -1 and hg.lib().hg_last_error().decode().startswith(ENTRY)
    with pytest.raises(hg.HgError, match=ENTRY):
        hg.verify_device_batch_bn254(None, pk, [w], [proof])
    assert _entry()(None, None, None, None, None, 1, None, None, 0) == -1
    assert hg.lib().hg_last_error().decode().startswith(ENTRY)
    if have_gpu():
        ctx = hg.Context(0)
        try:
            rc, _, _ = _raw_call(ctx.h, pk.h, [w.h.value], [proof])   # a device context with a host-only key
            assert rc == -1 and hg.lib().hg_last_error().decode().startswith(ENTRY)
            with pytest.raises(hg.HgError, match=ENTRY):
                hg.verify_device_batch_bn254(ctx, pk, [w], [proof])
            pkd = bfv.setup(ctx)
            try:
                assert _entry()(ctx.h, None, None, None, None, 1, None, None, 0) == -1   # a null key
                assert hg.lib().hg_last_error().decode().startswith(ENTRY)
                for args in (([None], [proof]), ([w.h.value], [None])):   # a null element
                    rc, _, _ = _raw_call(ctx.h, pkd.h, *args)
                    assert rc == -1 and hg.lib().hg_last_error().decode().startswith(ENTRY)
                rc, _, _ = _raw_call(ctx.h, pkd.h, [w.h.value], [proof], results=False)   # null results
                assert rc == -1 and hg.lib().hg_last_error().decode().startswith(ENTRY)
                other = hg.Witness.synthetic(hg.BfvEncrypt.new(2048, 1).params, 3)   # a witness of another parameter set
                rc, _, _ = _raw_call(ctx.h, pkd.h, [w.h.value, other.h.value], [proof, proof])
                assert rc == -1 and hg.lib().hg_last_error().decode().startswith(ENTRY)
                with pytest.raises(hg.HgError, match=ENTRY):
                    hg.verify_device_batch_bn254(ctx, pkd, [w, other], [proof, proof])
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


def _noncanonical(proof, el):
    bad = bytearray(proof)
    bad[32 * el] = 0xff   # (big-endian elements: the top byte set makes it >= r)
    return bytes(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
def test_batch_matches_the_single_proof_verifier(ctx, n, k):
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xb254 + 16 * n + i) for i in range(3)]
    ps = [ctx.prove_bn254(pk, w)[0] for w in ws]
    L = len(ps[0])
    nel = L // 32
    rng = random.Random(n)
    flips = []
    for pos in (31, 32 * (nel // 3) + 31, L // 2 + 31, L - 1):
        bad = bytearray(ps[0])
        bad[pos] ^= 1 << rng.randrange(8)
        flips.append(bytes(bad))
    pairs = [(ws[0], ps[0]), (ws[1], ps[1])] + [(ws[0], b) for b in flips] + [
        (ws[1], _noncanonical(ps[1], nel // 4)),   # a non-canonical element
        (ws[2], ps[2][:L // 2]),                   # truncated
        (ws[2], ps[2] + bytes(32)),                # a trailing zero element (ignored, as by the host verifier)
        (ws[1], ps[0]),                            # checked against another witness
        (ws[2], ps[2])]
    got = _batch_matches_singles(ctx, pk, [w for w, _ in pairs], [p for _, p in pairs])
    assert got[0] == got[1] == got[-1] == (True, "")
    assert [i for i, (ok, _) in enumerate(got) if ok] == [0, 1, 8, 10], got   # the honest pairs and the trailing element; every flip is rejected
    pk.free()


@pytest.mark.gpu
def test_every_input_table_lands_in_its_own_slot(ctx):
    """One entry of exactly one table changed by +1 mod p, for every table kind: the batch gives each altered pair the single entry's
    decision and reason (this pins the staging layout and the input-evaluation slots)."""
    n, k = 4096, 2
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x1b254)
    proof = ctx.prove_bn254(pk, w)[0]
    base = w.arrays()
    SZ = len(base["s"])
    PZ = len(base["r2is"]) // k
    where = [("s", 3), ("e", 11), ("k1", 17), ("ais", 5), ("ais", SZ + 9), ("r1is", SZ + 21), ("r2is", 7), ("r2is", PZ + 2), ("ct0is", SZ + 13)]
    alt = []
    for f, i in where:
        d = {g: a.copy() for g, a in base.items()}
        d[f][i] = (int(d[f][i]) + 1) % P
        alt.append(hg.Witness.from_arrays(bfv.params, d))
    wits = [w] + alt
    got = hg.verify_device_batch_bn254(ctx, pk, wits, [proof] * len(wits))
    assert got[0] == (True, "")
    for j, x in enumerate(alt):
        single = hg.verify_device_bn254(ctx, pk, x, proof)
        assert not single[0], where[j]
        assert got[1 + j] == single, (where[j], got[1 + j], single)
    pk.free()


@pytest.mark.gpu
def test_no_cross_wiring_between_the_proofs_of_a_batch(ctx):
    """Every table that depends on the key only is shared in a group: a witness's input evaluations must never be."""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xc254 + i) for i in range(4)]
    ps = [ctx.prove_bn254(pk, w)[0] for w in ws]
    pairs = [(ws[(i + 1) % 4], ps[i]) for i in range(4)] + [(ws[i], ps[i]) for i in range(4)]   # a permutation, then the matching pairs
    random.Random(7).shuffle(pairs)
    got = _batch_matches_singles(ctx, pk, [w for w, _ in pairs], [p for _, p in pairs], host=False)
    for (w, p), (ok, why) in zip(pairs, got):
        assert ok == (ws.index(w) == ps.index(p)), why
    assert sum(ok for ok, _ in got) == 4
    pk.free()


@pytest.mark.gpu
def test_group_boundaries_do_not_change_the_results(ctx):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xd254 + i) for i in range(7)]
    ps = [ctx.prove_bn254(pk, w)[0] for w in ws]
    ps[0] = ps[0][:len(ps[0]) // 2]
    bad = bytearray(ps[6])
    bad[len(bad) // 3 + 31] ^= 2
    ps[6] = bytes(bad)
    wits = list(ws)
    wits[4] = ws[3]   # (a mismatched pair in a middle group)
    runs = {}
    try:
        for G in (1, 3, 0):
            ctx.set_option("verify_batch_group", G)
            runs[G] = hg.verify_device_batch_bn254(ctx, pk, wits, ps)
    finally:
        ctx.set_option("verify_batch_group", 0)
    assert runs[1] == runs[3] == runs[0]
    one = runs[0]
    assert not one[0][0] and not one[4][0] and all(one[i][0] for i in (1, 2, 3, 5)), one   # (proof 6: as the single call decides)
    for i, (w, p) in enumerate(zip(wits, ps)):
        assert one[i] == hg.verify_device_bn254(ctx, pk, w, p), i
    pk.free()


BN_FIX = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", BN_FIX)
def test_reference_fixtures_are_accepted_in_a_batch(ctx, n, k, bits):
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.from_json_bn254(bfv.params, os.path.join(orclib.GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json"))
    proof = ctx.prove_bn254(pk, w)[0]
    other = hg.Witness.synthetic(bfv.params, 0xf254 + n)
    got = hg.verify_device_batch_bn254(ctx, pk, [w, other, w], [proof, proof, proof[:-32]])
    assert got[0] == (True, "")
    assert got[1] == hg.verify_device_bn254(ctx, pk, other, proof) and not got[1][0]
    assert got[2] == hg.verify_device_bn254(ctx, pk, w, proof[:-32])
    if n == 1024:
        ok, err = orclib.verify_f("bn254", orclib.params(n, k), orclib.Inputs(w.arrays()), proof, threads=8)
        assert ok == got[0][0], err
    pk.free()


@pytest.mark.gpu
def test_headline_size_batch_of_eight(ctx):
    n, k = 32768, 16
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0x8254 + i) for i in range(8)]
    ps = [ctx.prove_bn254(pk, w, cap=1 << 25)[0] for w in ws]
    bad = bytearray(ps[2])
    bad[len(bad) // 3 + 31] ^= 4
    ps[2] = bytes(bad)
    got = _batch_matches_singles(ctx, pk, ws, ps, host=False)
    assert [ok for i, (ok, _) in enumerate(got) if i != 2] == [True] * 7, got   # (proof 2: as the single call decides)
    tb, ts = [], []
    for i in range(4):
        t0 = time.perf_counter()
        hg.verify_device_batch_bn254(ctx, pk, ws, ps)
        t1 = time.perf_counter()
        for w, p in zip(ws, ps):
            hg.verify_device_bn254(ctx, pk, w, p)
        t2 = time.perf_counter()
        if i:
            tb.append((t1 - t0) * 1e3 / 8)
            ts.append((t2 - t1) * 1e3 / 8)
    print("n=%d k=%d, B=8: batch %.3f ms/proof, hg_verify_device_bn254 one by one %.3f ms/proof (median of 3)" % (
        n, k, statistics.median(tb), statistics.median(ts)))
    pk.free()


@pytest.mark.gpu
def test_the_context_stays_usable(ctx):
    """A batch uses the arena, the result buffer and a stream of its own: BN254 proves, the single BN254 device verifier and a
    Goldilocks batch on the same context give the same bytes and decisions after it as before."""
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0xe254)
    w2 = hg.Witness.synthetic(bfv.params, 0xe255)
    pb = ctx.prove_bn254(pk, w)[0]
    pg = bfv.prove(ctx, pk, w)[0]
    before = (hg.verify_device_bn254(ctx, pk, w, pb), hg.verify_device_bn254(ctx, pk, w2, pb),
              hg.verify_device_batch(ctx, pk, [w, w2], [pg, pg]))
    assert before[0] == (True, "") and not before[1][0] and before[2][0] == (True, "") and not before[2][1][0]
    got = hg.verify_device_batch_bn254(ctx, pk, [w, w2, w], [pb, pb, pb[:-32]])
    assert got[0] == (True, "") and got[1] == before[1]
    assert ctx.prove_bn254(pk, w)[0] == pb
    assert bfv.prove(ctx, pk, w)[0] == pg
    after = (hg.verify_device_bn254(ctx, pk, w, pb), hg.verify_device_bn254(ctx, pk, w2, pb),
             hg.verify_device_batch(ctx, pk, [w, w2], [pg, pg]))
    assert after == before
    pk.free()


@pytest.mark.gpu
def test_an_empty_batch_returns_0_and_writes_nothing(ctx):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    rc, res, reasons = _raw_call(ctx.h, pk.h, [], [], n=0)
    assert rc == 0
    assert res == [7] and reasons == b"\x55" * CAP
    assert hg.verify_device_batch_bn254(ctx, pk, [], []) == []
    pk.free()
