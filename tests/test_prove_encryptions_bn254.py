"""hg_prove_encryptions_bn254: a run of encryptions, given as signed polynomials in ascending degree, laid out, derived, lifted into
bn256::Fr, evaluated and proven in one pipeline (the feed of encryption i+1 under the prove of encryption i).

References, none of them the pipeline: hg_prove_bn254 of hg_witness_derive of the laid-out inputs (the path the pipeline must
reproduce byte for byte; tests/test_witness_derive.py and tests/test_gpu_parity.py pin it to the Fr oracle), the verifiers
hg_verify_bn254 / hg_verify_device_bn254, and the reference's JSON witnesses under tests/golden/."""
import ctypes as C
import json
import os
import statistics
import time

import numpy as np
import pytest

from hglib import hg, ROOT

P = hg.P
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55)]      # the three sets that have a bn254 fixture; the smallest with k = 1 and k = 2
INPUTS = ("s", "e", "k1", "ais")
I64_MIN = -(1 << 63)
NAME = "hg_prove_encryptions_bn254"
i64p = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def signed(words):
    """table words -> signed integers (z >= 0 as z, z < 0 as p - |z|)"""
    w = np.asarray(words, dtype=np.uint64)
    neg = w > np.uint64(P // 2)
    out = w.astype(np.int64)          # (values above 2^63 wrap; they are replaced below)
    out[neg] = -((np.uint64(P) - w[neg]).astype(np.int64))
    return out


def polys_of_tables(params, d):
    """the signed ascending polynomials (s, e, k1, a[k][n]) a set of laid-out tables holds"""
    n, k = params.n, params.k
    s = signed(d["s"][:n])[::-1]
    e = signed(d["e"][n - 1:2 * n - 1])[::-1]
    k1 = signed(d["k1"][n - 1:2 * n - 1])[::-1]
    a = np.stack([signed(d["ais"][i * 2 * n:i * 2 * n + n])[::-1] for i in range(k)])
    return tuple(np.ascontiguousarray(x) for x in (s, e, k1, a))


def polys_of_json(path, k):
    """the same straight from a reference JSON: coefficients are decimal strings in DESCENDING degree, negatives as p - |z| (Goldilocks
    files) or r - |z| (bn254 files); the modulus is told apart by size"""
    w = json.load(open(path))
    BN_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

    def sgn(v):
        out = []
        for x in v:
            x = int(x)
            if x > BN_R // 2:
                x -= BN_R
            elif x > P // 2 and x < P:
                x -= P
            out.append(x)
        return np.array(out[::-1], dtype=np.int64)
    return sgn(w["s"]), sgn(w["e"]), sgn(w["k1"]), np.stack([sgn(w["ais"][i]) for i in range(k)])


def same(got, want, fields):
    for f in fields:
        assert got[f].shape == want[f].shape, f
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s differs at %d positions, first %d: %d != %d" % (f, bad.size, bad[0], got[f][bad[0]], want[f][bad[0]])


def synthetic_encs(params, count, salt):
    return [polys_of_tables(params, hg.Witness.synthetic(params, salt + 131 * i + params.n).arrays()) for i in range(count)]


def reference_proofs(ctx, params, pk, encs):
    """hg_prove_bn254 of hg_witness_derive of the laid-out inputs: (proofs, tables of the handles)"""
    out, tabs = [], []
    for enc in encs:
        w = hg.Witness.derive(ctx, params, hg.encryption_layout(params, *enc))
        out.append(ctx.prove_bn254(pk, w)[0])
        tabs.append(w.arrays())
    return out, tabs


def c_columns(encs):
    """the four arrays of polynomial pointers the C entry takes (and the arrays that keep them alive)"""
    arrs = [[np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in enc] for enc in encs]
    return [(i64p * len(encs))(*[x[f].ctypes.data_as(i64p) for x in arrs]) for f in range(4)], arrs


# ---- 1. error surface -----------------------------------------------------------------------------------------------------------------
def test_errors_without_a_device():
    """No context can exist without a device, so every call here ends at the first check (no context): -1 and the function's name,
    whatever else is null and whatever n_enc is; the checks behind it are asserted in test_errors_on_the_device."""
    assert NAME in hg.EXPORTS
    L = hg.lib()
    assert hasattr(L, NAME)
    n, k = 1024, 1
    bfv = hg.BfvEncrypt.new(n, k)
    pk_host = bfv.setup(None)
    enc = (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((k, n), dtype=np.int64))
    with pytest.raises(hg.HgError, match=NAME + ": needs a device context"):
        hg.prove_encryptions_bn254(None, pk_host, [enc])
    with pytest.raises(hg.HgError, match=NAME + ": needs a device context"):
        hg.prove_encryptions_bn254(None, pk_host, [])
    h = (C.c_void_p * 1)(0xDEAD)
    assert L.hg_prove_encryptions_bn254(None, None, None, None, None, None, 1, None, 0, None, None, h, None, 0, None) == -1
    assert NAME in L.hg_last_error().decode() and not h[0]
    pk_host.free()


@pytest.mark.gpu
def test_errors_on_the_device(ctx):
    n, k = 1024, 1
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk, pk_host = bfv.setup(ctx), bfv.setup(None)
    encs = synthetic_encs(params, 3, 0xE0)
    want, _ = reference_proofs(ctx, params, pk, encs)

    def still_proves():
        assert hg.prove_encryptions_bn254(ctx, pk, encs, witnesses=False)[0] == want
    still_proves()
    L = hg.lib()
    with pytest.raises(hg.HgError, match=NAME + ": host-only"):
        hg.prove_encryptions_bn254(ctx, pk_host, encs)
    still_proves()
    with pytest.raises(hg.HgError, match=NAME + ": needs a device context"):
        hg.prove_encryptions_bn254(None, pk, encs)
    proofs, status, why, ws, tm = hg.prove_encryptions_bn254(ctx, pk, [])   # n_enc == 0 returns 0
    assert proofs == [] and status == [] and ws == []
    assert L.hg_prove_encryptions_bn254(ctx.h, pk.h, None, None, None, None, 0, None, 0, None, None, None, None, 0, None) == 0
    assert L.hg_prove_encryptions_bn254(ctx.h, pk.h, None, None, None, None, 1, None, 0, None, None, None, None, 0, None) == -1
    assert NAME + ": null argument" in L.hg_last_error().decode()
    assert L.hg_prove_encryptions_bn254(ctx.h, None, None, None, None, None, 0, None, 0, None, None, None, None, 0, None) == -1
    assert NAME + ": null argument" in L.hg_last_error().decode()
    still_proves()
    # a null polynomial in item 1 names the item
    cols, keep = c_columns(encs)
    cap = 1 << 22
    buf = (C.c_uint8 * (3 * cap))()
    lens, st = (C.c_size_t * 3)(), (C.c_int * 3)()
    for f in range(4):
        holed, keep_holed = c_columns(encs)
        holed[f][1] = None
        args = [holed[g] if g == f else cols[g] for g in range(4)]
        assert L.hg_prove_encryptions_bn254(ctx.h, pk.h, *args, 3, buf, cap, lens, st, None, None, 0, None) == -1
        assert NAME + ": encryption 1: null polynomial" in L.hg_last_error().decode()
    still_proves()
    with pytest.raises(hg.HgError, match=NAME + r": encryption 0: proof buffer too small \(%d bytes\)" % len(want[0])):
        hg.prove_encryptions_bn254(ctx, pk, encs, cap_each=1000)
    still_proves()
    # parameters the derivation cannot serve: an error of the call, not of an item
    bad = hg.params_builtin(n, k)
    bad.qis[0] = int(bad.qis[0]) + 1
    pk_bad = hg.BfvEncrypt(bad).setup(ctx)
    with pytest.raises(hg.HgError, match="even"):
        hg.prove_encryptions_bn254(ctx, pk_bad, encs)
    still_proves()
    pk.free(); pk_host.free(); pk_bad.free()


# ---- 2. byte identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", FIX)
def test_proofs_are_those_of_derive_then_prove(ctx, n, k, bits):
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    run = 5
    encs = synthetic_encs(params, run, 0xC0DE)
    want, tabs = reference_proofs(ctx, params, pk, encs)
    assert len(set(want)) == run                                              # distinct encryptions, distinct proofs
    for call in range(3):
        proofs, status, why, ws, tm = hg.prove_encryptions_bn254(ctx, pk, encs)
        assert status == [0] * run and why == [""] * run, (call, status, why)
        for i in range(run):
            assert proofs[i] == want[i], (call, i, len(proofs[i]), len(want[i]))
            same(ws[i].arrays(), tabs[i], hg.Witness.FIELDS)
        assert tm["total_ms"] > 0 and tm["witness_ms"] > 0 and tm["prove_ms"] > 0
        assert tm["total_ms"] >= tm["prove_ms"]
        assert [tm[f] for f in ("upload_ms", "gpu_ms", "enqueue_ms", "sync_ms", "replay_ms")] == [0.0] * 5
    for length in (1, 2, 3):                                                   # short runs, rotated so that both table sets see other items
        sub = encs[length:] + encs[:length]
        proofs, status, _, ws, _ = hg.prove_encryptions_bn254(ctx, pk, sub[:length], witnesses=False)
        assert status == [0] * length and ws == [None] * length
        assert proofs == (want[length:] + want[:length])[:length], length
    assert hg.prove_encryptions_bn254(ctx, pk, encs[::-1], witnesses=False)[0] == want[::-1]
    pk.free()


# ---- 3. the reference's fixtures fed as encryptions -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", FIX)
def test_fixtures_as_encryptions(ctx, n, k, bits):
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    paths = [os.path.join(GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json"), os.path.join(GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json")]
    refs = [hg.Witness.from_json_bn254(params, paths[0]).arrays(), hg.Witness.from_json(params, paths[1]).arrays()]
    encs = [polys_of_json(q, k) for q in paths]
    proofs, status, why, ws, _ = hg.prove_encryptions_bn254(ctx, pk, encs)
    assert status == [0, 0], why
    assert proofs[0] != proofs[1]
    for i, ref in enumerate(refs):
        same(ws[i].arrays(), ref, hg.Witness.FIELDS)                           # all seven tables, inputs laid out by the device kernel
        ok, reason = hg.verify_bn254(pk, ws[i], proofs[i])
        assert ok, reason
        ok, reason = hg.verify_device_bn254(ctx, pk, ws[i], proofs[i])
        assert ok, reason
        flipped = bytearray(proofs[i])
        flipped[len(flipped) // 2] ^= 1
        assert not hg.verify_bn254(pk, ws[i], bytes(flipped))[0]
    pk.free()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def spoiled(enc, which, modulus, pos, value):
    out = [x.copy() for x in enc]
    if which == 3:
        out[3][modulus][pos] = value
    else:
        out[which][pos] = value
    return tuple(out)


@pytest.mark.gpu
def test_refused_encryptions(ctx):
    n, k = 4096, 2
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    clean = synthetic_encs(params, 6, 0xBAD)
    e_bad = spoiled(clean[1], 1, 0, 17, int(params.e_bound) + 1)
    a_bad = spoiled(clean[4], 3, 1, n - 3, (int(params.qis[1]) + 1) // 2)
    want, _, _, _, _ = hg.prove_encryptions_bn254(ctx, pk, clean)
    assert want == reference_proofs(ctx, params, pk, clean)[0]
    run = [clean[0], e_bad, clean[2], clean[3], a_bad, clean[5]]
    L = hg.lib()
    for call in range(3):
        proofs, status, why, ws, tm = hg.prove_encryptions_bn254(ctx, pk, run)
        assert status == [0, 1, 0, 0, 1, 0], (call, status, why)
        assert NAME + ": encryption 1: table e:" in why[1] and "e_bound" in why[1], why[1]
        assert NAME + ": encryption 4: table ais of modulus 1 " in why[4] and "(q_i-1)/2" in why[4], why[4]
        for i in (1, 4):
            assert proofs[i] is None and ws[i] is None
        for i in (0, 2, 3, 5):
            assert proofs[i] == want[i], (call, i)
            assert why[i] == "" and ws[i] is not None
    # the C entry itself: return value, lens, NULL handles, truncated reasons
    cols, keep = c_columns(run)
    cap, rcap = 1 << 22, 40
    buf = (C.c_uint8 * (6 * cap))()
    lens = (C.c_size_t * 6)(*[7] * 6)
    st = (C.c_int * 6)(*[9] * 6)
    hs = (C.c_void_p * 6)(*[0xDEAD] * 6)
    reasons = C.create_string_buffer(b"\xff" * (6 * rcap), 6 * rcap)
    assert L.hg_prove_encryptions_bn254(ctx.h, pk.h, *cols, 6, buf, cap, lens, st, hs, reasons, rcap, None) == 2
    assert list(st) == [0, 1, 0, 0, 1, 0]
    assert lens[1] == 0 and lens[4] == 0 and not hs[1] and not hs[4]
    assert not any(buf[1 * cap:1 * cap + 4096]) and not any(buf[4 * cap:4 * cap + 4096])       # no proof bytes for a refused item
    for i in (0, 2, 3, 5):
        assert bytes(buf[i * cap:i * cap + lens[i]]) == want[i] and hs[i]
        L.hg_witness_free(C.c_void_p(hs[i]))
        assert reasons.raw[i * rcap:i * rcap + 1] == b"\0"
    for i in (1, 4):                                                           # truncated to reason_cap bytes, NUL included
        assert len(why[i]) > rcap and reasons.raw[i * rcap:(i + 1) * rcap] == why[i].encode()[:rcap - 1] + b"\0"
    # a refused first item, a refused last item, every item refused, other causes
    proofs, status, why, _, _ = hg.prove_encryptions_bn254(ctx, pk, [e_bad, clean[0], clean[2]])
    assert status == [1, 0, 0] and proofs[1:] == [want[0], want[2]] and "table e:" in why[0]
    proofs, status, why, _, _ = hg.prove_encryptions_bn254(ctx, pk, [clean[3], clean[5], a_bad])
    assert status == [0, 0, 1] and proofs[:2] == [want[3], want[5]] and "table ais of modulus 1 " in why[2]
    s_bad = spoiled(clean[2], 0, 0, 0, -(int(params.s_bound) + 1))
    k1_bad = spoiled(clean[2], 2, 0, n - 1, int(params.k1_bound) + 1)
    a0_bad = spoiled(clean[2], 3, 0, 0, I64_MIN)
    proofs, status, why, ws, _ = hg.prove_encryptions_bn254(ctx, pk, [s_bad, k1_bad, a0_bad])
    assert status == [1, 1, 1] and proofs == [None] * 3 and ws == [None] * 3
    assert "table s:" in why[0] and "table k1:" in why[1] and "table ais of modulus 0 " in why[2]
    assert all(NAME + ": encryption %d:" % i in why[i] for i in range(3))
    assert hg.prove_encryptions_bn254(ctx, pk, [e_bad])[1] == [1] and hg.prove_encryptions_bn254(ctx, pk, [clean[5]])[0] == [want[5]]
    pk.free()


# ---- 5. neighbours on the same context ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_neighbours_share_the_context(ctx):
    """The pipeline keeps its tables outside the arena every BN254 prove resets, swaps the context's streams as hg_prove_bn254 does and
    shares the derivation kernels (not their buffers) with the Goldilocks pipeline: none of the neighbours may notice it, nor it them."""
    n, k = 4096, 2
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    fulls = [hg.Witness.synthetic(params, 0x9E16 + 17 * i).arrays() for i in range(3)]
    hws = [hg.Witness.from_arrays(params, f) for f in fulls]
    encs = [polys_of_tables(params, f) for f in fulls]

    def neighbours():
        got = {"prove": [ctx.prove_bn254(pk, w)[0] for w in hws]}
        got["eval"] = [ctx.circuit_eval_bn254(pk, hws[0], which) for which in (0, 2)]
        got["verify"] = [hg.verify_device_bn254(ctx, pk, w, q) for w, q in zip(hws, got["prove"])]
        got["verify_other"] = hg.verify_device_bn254(ctx, pk, hws[1], got["prove"][0])[0]
        got["gl"] = hg.prove_encryptions(ctx, pk, encs, witnesses=False)[0]
        return got
    before = neighbours()
    assert len(set(before["prove"])) == 3 and before["eval"][0] == before["eval"][1]      # (the sum node equals ct0is)
    assert before["verify"] == [(True, "")] * 3 and not before["verify_other"]
    assert before["gl"] == [bfv.prove(ctx, pk, w)[0] for w in hws]
    for rnd in range(3):                                                       # pipeline, neighbours, pipeline, ...: both orders
        proofs, _, _, ws, _ = hg.prove_encryptions_bn254(ctx, pk, encs, witnesses=(rnd != 1))
        assert proofs == before["prove"], rnd
        if rnd != 1:
            for i in range(3):
                same(ws[i].arrays(), fulls[i], hg.Witness.FIELDS)
        assert neighbours() == before, rnd
    assert hg.prove_encryptions_bn254(ctx, pk, encs[::-1])[0] == before["prove"][::-1]
    pk.free()


# ---- 6. timing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_is_not_slower_than_the_serial_loop(ctx):
    """(32768, 16), runs of 8, two warm-up rounds of each form, then 5 rounds alternating in one process, medians. The serial loop is
    what a service writes without this entry: hg_witness_derive on inputs laid out beforehand, then hg_prove_bn254, per item. The
    pipeline is called with ws = NULL. Asserted: equal proofs, and the pipeline is not slower.
    Measured on an MI355X (two runs of this test on one box): serial 11.6-12.2 ms per proof, pipeline 8.83-8.89 ms, ratio 0.73-0.76,
    witness_ms / run 3.4 ms (README.md)."""
    n, k, run = 32768, 16, 8
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    fulls = [hg.Witness.synthetic(params, 0x71AE + 3 * i).arrays() for i in range(run)]
    encs = [polys_of_tables(params, f) for f in fulls]
    laid = [[np.ascontiguousarray(f[g]) for g in INPUTS] for f in fulls]
    ptrs = [[hg._ptr(a) for a in item] for item in laid]
    L = hg.lib()
    L.hg_witness_derive.argtypes = [C.c_void_p, C.POINTER(hg.HgParams)] + [hg.u64p] * 4 + [C.POINTER(C.c_void_p)]
    pp = C.POINTER(i64p)
    L.hg_prove_encryptions_bn254.argtypes = [C.c_void_p, C.c_void_p, pp, pp, pp, pp, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t, C.POINTER(hg.HgTimings)]
    cols, keep = c_columns(encs)
    cap = 1 << 21
    one = (C.c_uint8 * cap)()
    buf = (C.c_uint8 * (run * cap))()
    lens, st, ln, ms2 = (C.c_size_t * run)(), (C.c_int * run)(), C.c_size_t(0), (C.c_double * 2)()

    def serial():
        proofs = []
        t0 = time.perf_counter()
        for item in ptrs:
            h = C.c_void_p()
            assert L.hg_witness_derive(ctx.h, C.byref(params), *item, C.byref(h)) == 0
            assert L.hg_prove_bn254(ctx.h, pk.h, h, one, cap, C.byref(ln), ms2) == 0, L.hg_last_error()
            L.hg_witness_free(h)
            proofs.append(C.string_at(one, ln.value))
        return (time.perf_counter() - t0) * 1e3 / run, proofs

    def pipeline():
        tm = hg.HgTimings()
        t0 = time.perf_counter()
        rc = L.hg_prove_encryptions_bn254(ctx.h, pk.h, *cols, run, buf, cap, lens, st, None, None, 0, C.byref(tm))
        ms = (time.perf_counter() - t0) * 1e3 / run
        assert rc == 0, L.hg_last_error()
        return ms, [C.string_at(C.addressof(buf) + i * cap, lens[i]) for i in range(run)], tm
    for _ in range(2):                                                         # warm-up: table sets, staging, arena, thread pool
        want = serial()[1]
        assert pipeline()[1] == want
    assert len(set(want)) == run
    ts, tp, wit = [], [], []
    for _ in range(5):
        ts.append(serial()[0])
        ms, proofs, tm = pipeline()
        assert proofs == want
        tp.append(ms); wit.append(tm.witness_ms / run)
    ms_serial, ms_pipe = statistics.median(ts), statistics.median(tp)
    print("\nn=%d k=%d run=%d per proof: serial hg_witness_derive + hg_prove_bn254 %.3f ms (%s), hg_prove_encryptions_bn254 %.3f ms (%s), "
          "ratio %.3f, witness_ms/run %.3f ms" % (n, k, run, ms_serial, " ".join("%.3f" % t for t in ts), ms_pipe,
                                                  " ".join("%.3f" % t for t in tp), ms_pipe / ms_serial, statistics.median(wit)))
    assert ms_pipe <= ms_serial, (ms_pipe, ms_serial)
    pk.free()
