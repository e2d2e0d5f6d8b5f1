"""hg_encryption_layout / hg_prove_encryptions: a run of encryptions, given as signed polynomials in ascending degree, laid out,
derived, evaluated and proven in one pipeline (derivation + evaluation of encryption i+1 under the prove of encryption i).

References, none of them the pipeline: the reference's own JSON witnesses under tests/golden/, the host path hg_witness_synthetic,
and hg_prove of hg_witness_derive of the laid-out inputs (the path the pipeline must reproduce byte for byte).

The layout rule exists twice on purpose - hg_encryption_layout on the host, k_derive_pack on the device - and the tests hold one
against the other: the handles the pipeline returns carry the tables the DEVICE laid out."""
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
FIX = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55), (8192, 4, 55)]
BN_FIX = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55)]
SETS = [(1024, 1), (2048, 1), (4096, 2), (8192, 4), (16384, 8), (32768, 16)]
INPUTS = ("s", "e", "k1", "ais")
I64_MIN = -(1 << 63)


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


# ---- 1. layout against the reference's fixtures (no GPU) ------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,k,bits", [("gl", *f) for f in FIX] + [("bn254", *f) for f in BN_FIX])
def test_layout_reproduces_reference_fixture(family, n, k, bits):
    params = hg.params_builtin(n, k)
    if family == "gl":
        path = os.path.join(GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json")
        ref = hg.Witness.from_json(params, path).arrays()
    else:
        path = os.path.join(GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json")
        ref = hg.Witness.from_json_bn254(params, path).arrays()
    s, e, k1, a = polys_of_json(path, k)
    assert s.size == n and e.size == n and k1.size == n and a.shape == (k, n)
    same(hg.encryption_layout(params, s, e, k1, a), ref, INPUTS)


# ---- 2. layout round trip at every built-in set (no GPU) ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", SETS)
def test_layout_round_trip(n, k):
    params = hg.params_builtin(n, k)
    ref = hg.Witness.synthetic(params, 0x1A70 + n).arrays()
    polys = polys_of_tables(params, ref)
    assert any((x < 0).any() for x in polys) and all(x.dtype == np.int64 for x in polys)
    same(hg.encryption_layout(params, *polys), ref, INPUTS)


# ---- 3. layout errors (no GPU) --------------------------------------------------------------------------------------------------------
def test_layout_errors():
    n, k = 1024, 1
    params = hg.params_builtin(n, k)
    L = hg.lib()
    i64p = C.POINTER(C.c_int64)
    L.hg_encryption_layout.argtypes = [C.POINTER(hg.HgParams)] + [i64p] * 4 + [hg.u64p] * 4
    ins = [np.zeros(n, dtype=np.int64) for _ in range(3)] + [np.zeros(k * n, dtype=np.int64)]
    outs = [np.zeros(2 * n, dtype=np.uint64) for _ in range(3)] + [np.zeros(k * 2 * n, dtype=np.uint64)]
    args = [x.ctypes.data_as(i64p) for x in ins] + [hg._ptr(x) for x in outs]
    assert L.hg_encryption_layout(C.byref(params), *args) == 0
    for hole in range(8):
        holed = list(args)
        holed[hole] = None
        assert L.hg_encryption_layout(C.byref(params), *holed) == -1
        assert "hg_encryption_layout: null argument" in L.hg_last_error().decode()
    assert L.hg_encryption_layout(None, *args) == -1
    assert "hg_encryption_layout" in L.hg_last_error().decode()
    for which in range(4):
        bad = [x.copy() for x in ins]
        bad[which][7] = I64_MIN
        with pytest.raises(hg.HgError, match="hg_encryption_layout.*INT64_MIN"):
            hg.encryption_layout(params, *bad)
    # the most negative value that has a magnitude is laid out (bounds are the derivation's business)
    ok = [x.copy() for x in ins]
    ok[1][0] = I64_MIN + 1
    assert int(hg.encryption_layout(params, *ok)["e"][2 * n - 2]) == P - ((1 << 63) - 1)


# ---- 4. pipeline errors (no GPU) ------------------------------------------------------------------------------------------------------
def test_pipeline_errors_without_a_device():
    """No context can exist without a device, so what can be asked here is: a null context is -1 and names the function (whatever
    n_enc is - the order of hg_verify_device_batch's checks); n_enc == 0 returning 0 needs a context and is asserted in
    test_pipeline_errors_on_the_device."""
    n, k = 1024, 1
    bfv = hg.BfvEncrypt.new(n, k)
    pk_host = bfv.setup(None)
    enc = (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((k, n), dtype=np.int64))
    with pytest.raises(hg.HgError, match="hg_prove_encryptions: needs a device context"):
        hg.prove_encryptions(None, pk_host, [enc])
    with pytest.raises(hg.HgError, match="hg_prove_encryptions: needs a device context"):
        hg.prove_encryptions(None, pk_host, [])
    L = hg.lib()
    h = (C.c_void_p * 1)(0xDEAD)
    assert L.hg_prove_encryptions(None, None, None, None, None, None, 1, None, 0, None, None, h, None, 0, None) == -1
    assert "hg_prove_encryptions" in L.hg_last_error().decode() and not h[0]
    assert "hg_prove_encryptions" in hg.EXPORTS and "hg_encryption_layout" in hg.EXPORTS
    pk_host.free()


# =======================================================================================================================================
# GPU
def reference_proofs(ctx, bfv, pk, encs):
    """hg_prove of hg_witness_derive of the laid-out inputs: (proofs, tables of the handles)"""
    out, tabs = [], []
    for enc in encs:
        w = hg.Witness.derive(ctx, bfv.params, hg.encryption_layout(bfv.params, *enc))
        out.append(bfv.prove(ctx, pk, w)[0])
        tabs.append(w.arrays())
    return out, tabs


def synthetic_encs(params, count, salt):
    return [polys_of_tables(params, hg.Witness.synthetic(params, salt + 131 * i + params.n).arrays()) for i in range(count)]


@pytest.mark.gpu
def test_pipeline_errors_on_the_device(ctx):
    n, k = 1024, 1
    bfv = hg.BfvEncrypt.new(n, k)
    pk, pk_host = bfv.setup(ctx), bfv.setup(None)
    enc = synthetic_encs(bfv.params, 1, 0xE0)[0]
    with pytest.raises(hg.HgError, match="hg_prove_encryptions: host-only"):
        hg.prove_encryptions(ctx, pk_host, [enc])
    with pytest.raises(hg.HgError, match="hg_prove_encryptions: needs a device context"):
        hg.prove_encryptions(None, pk, [enc])
    proofs, status, why, ws, tm = hg.prove_encryptions(ctx, pk, [])          # n_enc == 0 returns 0
    assert proofs == [] and status == [] and ws == []
    with pytest.raises(hg.HgError, match="hg_prove_encryptions: encryption 0: proof buffer too small"):
        hg.prove_encryptions(ctx, pk, [enc], cap_each=1000)
    L = hg.lib()
    assert L.hg_prove_encryptions(ctx.h, pk.h, None, None, None, None, 1, None, 0, None, None, None, None, 0, None) == -1
    assert "hg_prove_encryptions: null argument" in L.hg_last_error().decode()
    # parameters the derivation cannot serve: an error of the call, not of an item
    bad = hg.params_builtin(n, k)
    bad.qis[0] = int(bad.qis[0]) + 1
    pk_bad = hg.BfvEncrypt(bad).setup(ctx)
    with pytest.raises(hg.HgError, match="even"):
        hg.prove_encryptions(ctx, pk_bad, [enc])
    want, _ = reference_proofs(ctx, bfv, pk, [enc])
    assert hg.prove_encryptions(ctx, pk, [enc])[0] == want                   # and the context still proves
    pk.free(); pk_host.free(); pk_bad.free()


# ---- 5. byte identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,k", SETS)
def test_proofs_are_those_of_derive_then_prove(ctx, n, k):
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    run = 5 if n <= 8192 else 4
    encs = synthetic_encs(bfv.params, run, 0xC0DE)
    want, tabs = reference_proofs(ctx, bfv, pk, encs)
    assert len(set(want)) == run                                              # distinct encryptions, distinct proofs
    # first call: walked proves and the recording ones; second and third: recorded and replayed launch graphs of both table sets
    for call in range(3):
        proofs, status, why, ws, tm = hg.prove_encryptions(ctx, pk, encs)
        assert status == [0] * run and why == [""] * run, (call, status, why)
        for i in range(run):
            assert proofs[i] == want[i], (call, i, len(proofs[i]), len(want[i]))
            same(ws[i].arrays(), tabs[i], hg.Witness.FIELDS)
        assert tm["total_ms"] > 0 and tm["witness_ms"] > 0 and tm["prove_ms"] > 0 and tm["gpu_ms"] > 0
    for length in (1, 2, 3):                                                   # short runs, rotated so that both table sets see other items
        sub = encs[length:] + encs[:length]
        proofs, status, _, ws, _ = hg.prove_encryptions(ctx, pk, sub[:length], witnesses=False)
        assert status == [0] * length and ws == [None] * length
        assert proofs == (want[length:] + want[:length])[:length], length
    ctx.set_option("graph", 0)
    try:
        proofs, status, _, _, _ = hg.prove_encryptions(ctx, pk, encs)
        assert status == [0] * run and proofs == want
    finally:
        ctx.set_option("graph", 1)
    assert hg.prove_encryptions(ctx, pk, encs[::-1], witnesses=False)[0] == want[::-1]
    pk.free()


# ---- 6. the reference's fixtures fed as encryptions -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", FIX)
def test_fixtures_as_encryptions(ctx, n, k, bits):
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    paths = [os.path.join(GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json")]
    if (n, k, bits) in BN_FIX:
        paths.append(os.path.join(GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json"))
    refs = [hg.Witness.from_json(bfv.params, paths[0]).arrays()] + [hg.Witness.from_json_bn254(bfv.params, q).arrays() for q in paths[1:]]
    encs = [polys_of_json(q, k) for q in paths]
    proofs, status, why, ws, _ = hg.prove_encryptions(ctx, pk, encs)
    assert status == [0] * len(encs), why
    for i, ref in enumerate(refs):
        same(ws[i].arrays(), ref, hg.Witness.FIELDS)                           # all seven tables, inputs laid out by the device kernel
        ok, reason = hg.verify(pk, ws[i], proofs[i])
        assert ok, reason
        ok, reason = hg.verify_device(ctx, pk, ws[i], proofs[i])
        assert ok, reason
        assert proofs[i] == bfv.prove(ctx, pk, hg.Witness.from_arrays(bfv.params, ref))[0]
    pk.free()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
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
    want, _, _, _, _ = hg.prove_encryptions(ctx, pk, clean)
    assert want == reference_proofs(ctx, bfv, pk, clean)[0]
    run = [clean[0], e_bad, clean[2], clean[3], a_bad, clean[5]]
    L = hg.lib()
    for call in range(3):                                                      # walked, recorded and replayed schedules
        proofs, status, why, ws, tm = hg.prove_encryptions(ctx, pk, run)
        assert status == [0, 1, 0, 0, 1, 0], (call, status, why)
        assert "hg_prove_encryptions: encryption 1: table e:" in why[1] and "e_bound" in why[1], why[1]
        assert "hg_prove_encryptions: encryption 4: table ais of modulus 1 " in why[4] and "(q_i-1)/2" in why[4], why[4]
        for i in (1, 4):
            assert proofs[i] is None and ws[i] is None
        for i in (0, 2, 3, 5):
            assert proofs[i] == want[i], (call, i)
            assert why[i] == "" and ws[i] is not None
    # the C entry itself: return value, lens, NULL handles, truncated reasons
    arrs = [[np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in enc] for enc in run]
    i64p = C.POINTER(C.c_int64)
    cols = [(i64p * 6)(*[x[f].ctypes.data_as(i64p) for x in arrs]) for f in range(4)]
    cap = 1 << 20
    buf = (C.c_uint8 * (6 * cap))()
    lens = (C.c_size_t * 6)(*[7] * 6)
    st = (C.c_int * 6)(*[9] * 6)
    hs = (C.c_void_p * 6)(*[0xDEAD] * 6)
    reasons = C.create_string_buffer(6 * 24)
    assert L.hg_prove_encryptions(ctx.h, pk.h, *cols, 6, buf, cap, lens, st, hs, reasons, 24, None) == 2
    assert list(st) == [0, 1, 0, 0, 1, 0]
    assert lens[1] == 0 and lens[4] == 0 and not hs[1] and not hs[4]
    assert not any(buf[1 * cap:1 * cap + 4096]) and not any(buf[4 * cap:4 * cap + 4096])       # no proof bytes for a refused item
    for i in (0, 2, 3, 5):
        assert bytes(buf[i * cap:i * cap + lens[i]]) == want[i] and hs[i]
        L.hg_witness_free(C.c_void_p(hs[i]))
    assert reasons.raw[24:48] == b"hg_prove_encryptions: e\0" and reasons.raw[0:1] == b"\0"
    # a refused first item, a refused last item, every item refused, other causes
    proofs, status, why, _, _ = hg.prove_encryptions(ctx, pk, [e_bad, clean[0], clean[2]])
    assert status == [1, 0, 0] and proofs[1:] == [want[0], want[2]] and "table e:" in why[0]
    proofs, status, why, _, _ = hg.prove_encryptions(ctx, pk, [clean[3], clean[5], a_bad])
    assert status == [0, 0, 1] and proofs[:2] == [want[3], want[5]] and "table ais of modulus 1 " in why[2]
    s_bad = spoiled(clean[2], 0, 0, 0, -(int(params.s_bound) + 1))
    k1_bad = spoiled(clean[2], 2, 0, n - 1, int(params.k1_bound) + 1)
    a0_bad = spoiled(clean[2], 3, 0, 0, I64_MIN)
    proofs, status, why, _, _ = hg.prove_encryptions(ctx, pk, [s_bad, k1_bad, a0_bad])
    assert status == [1, 1, 1] and proofs == [None] * 3
    assert "table s:" in why[0] and "table k1:" in why[1] and "table ais of modulus 0 " in why[2]
    assert hg.prove_encryptions(ctx, pk, [e_bad])[1] == [1] and hg.prove_encryptions(ctx, pk, [clean[5]])[0] == [want[5]]
    pk.free()


# ---- 8. neighbours on the same context ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_neighbours_share_the_context(ctx):
    n, k = 4096, 2
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    fulls = [hg.Witness.synthetic(params, 0x9E16 + 17 * i).arrays() for i in range(5)]
    hws = [hg.Witness.from_arrays(params, f) for f in fulls]
    encs = [polys_of_tables(params, f) for f in fulls]
    vals = hg.witness_gen(ctx, pk, hws[0])
    out = hg.ProofBuffer()

    def neighbours():
        got = {"prove": [bfv.prove(ctx, pk, w)[0] for w in hws], "stream": bfv.prove_stream(ctx, pk, hws)[0], "into": []}
        for f in fulls:
            hg.witness_derive_into(ctx, pk, {g: f[g] for g in INPUTS}, vals)
            got["into"].append(hg.prove_resident(ctx, pk, vals, out).bytes())
        return got
    before = neighbours()
    assert before["prove"] == before["stream"] == before["into"] and len(set(before["prove"])) == 5
    for rnd in range(3):                                                       # pipeline, neighbours, pipeline, ... : both orders, every schedule
        assert hg.prove_encryptions(ctx, pk, encs, witnesses=(rnd != 1))[0] == before["prove"], rnd
        assert neighbours() == before, rnd
    assert hg.prove_encryptions(ctx, pk, encs[::-1])[0] == before["prove"][::-1]
    vals.free()
    pk.free()


# ---- 9. timing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_is_not_slower_than_the_serial_loop(ctx):
    """(32768, 16), runs of 16 after warm-up, the two forms alternating in one process, median of 5 each. The serial loop is what a
    service writes without this entry: hg_witness_derive_into on laid-out inputs, then hg_prove_resident, per item. Neither form is
    asked for host handles (ws = NULL / w = NULL), so both do the same work for the same proofs. Asserted: the pipeline is not slower."""
    n, k, run = 32768, 16, 16
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    fulls = [hg.Witness.synthetic(params, 0x71AE + 3 * i).arrays() for i in range(run)]
    encs = [polys_of_tables(params, f) for f in fulls]
    laid = [[np.ascontiguousarray(f[g]) for g in INPUTS] for f in fulls]
    vals = hg.witness_gen(ctx, pk, hg.Witness.from_arrays(params, fulls[0]))
    out = hg.ProofBuffer()
    L = hg.lib()
    L.hg_witness_derive_into.argtypes = [C.c_void_p, C.c_void_p] + [hg.u64p] * 4 + [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(hg.HgTimings)]
    ptrs = [[hg._ptr(a) for a in item] for item in laid]

    def serial():
        proofs = []
        t0 = time.perf_counter()
        for item in ptrs:
            assert L.hg_witness_derive_into(ctx.h, pk.h, *item, vals.h, None, None) == 0
            hg.prove_resident(ctx, pk, vals, out)
            proofs.append(out.bytes())
        return (time.perf_counter() - t0) * 1e3 / run, proofs

    def pipeline():
        t0 = time.perf_counter()
        proofs, status, _, _, tm = hg.prove_encryptions(ctx, pk, encs, witnesses=False)
        ms = (time.perf_counter() - t0) * 1e3 / run
        assert status == [0] * run
        return ms, proofs, tm
    for _ in range(2):                                                         # warm-up: launch graphs of all three table sets, staging, thread pool
        want = serial()[1]
        assert pipeline()[1] == want
    ts, tp, wit, inner = [], [], [], []
    for _ in range(5):
        ts.append(serial()[0])
        ms, proofs, tm = pipeline()
        assert proofs == want
        tp.append(ms); wit.append(tm["witness_ms"] / run); inner.append(tm["total_ms"] / run)
    ms_serial, ms_pipe = statistics.median(ts), statistics.median(tp)
    print("\nn=%d k=%d run=%d per proof: serial derive_into + prove_resident %.3f ms (%s), hg_prove_encryptions %.3f ms (%s), ratio %.3f, "
          "witness_ms/n %.3f ms, total_ms/n %.3f ms" % (n, k, run, ms_serial, " ".join("%.3f" % t for t in ts), ms_pipe,
                                                       " ".join("%.3f" % t for t in tp), ms_pipe / ms_serial, statistics.median(wit),
                                                       statistics.median(inner)))
    assert ms_pipe <= ms_serial, (ms_pipe, ms_serial)
    vals.free()
    pk.free()
