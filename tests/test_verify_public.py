"""hg_verify_public / hg_claims_settle: the verifier split where the public data ends. The public part decides everything the key,
the proof, a_i and ct0_i decide and returns the claims left on the five secret inputs; the settle step checks those against a
witness handle. hg_verify_mode is the yardstick: the two parts together make its decision for every proof, honest or tampered."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import orclib
from hglib import hg, ROOT, have_gpu

P = hg.P
NEW = ["hg_instance_from_ciphertext", "hg_instance_from_witness", "hg_instance_free", "hg_instance_coeffs", "hg_instance_get", "hg_pk_claim_shape",
       "hg_verify_public", "hg_verify_public_device", "hg_claims_settle", "hg_instance_mle"]
GL_FIXTURES = [("", 1024, 1, 27), ("", 2048, 1, 52), ("", 4096, 2, 55), ("", 8192, 4, 55), ("bn254_", 1024, 1, 27), ("bn254_", 2048, 1, 52), ("bn254_", 4096, 2, 55)]
SHAPES = [(1024, 1, 27), (4096, 2, 55)]


# ---- Python-integer arithmetic of GoldilocksExt2 (X^2 = 7) and the MLE of a table ------------------------------------------------
def e_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def eq_table(pt):
    """eq(pt, x), x_0 the lowest bit of the index"""
    t = [(1, 0)]
    for r in pt:
        hi = [e_mul(v, r) for v in t]
        t = [((v[0] - h[0]) % P, (v[1] - h[1]) % P) for v, h in zip(t, hi)] + hi
    return t


def py_mle(table, pt):
    eq = eq_table(pt)
    assert len(eq) == len(table)
    c0 = c1 = 0
    for v, e in zip(table, eq):
        v = int(v)
        if v:
            c0 += v * e[0]
            c1 += v * e[1]
    return (c0 % P, c1 % P)


def points(nvars, seed):
    """random E points, the all-zero point and the all-ones point"""
    rng = random.Random(seed)
    rnd = [[(rng.randrange(P), rng.randrange(P)) for _ in range(nvars)] for _ in range(2)]
    return rnd + [[(0, 0)] * nvars, [(1, 0)] * nvars]


def flat(pt):
    return np.array([c for x in pt for c in x], dtype=np.uint64)


def unit_point(index, nvars):
    return [((index >> b) & 1, 0) for b in range(nvars)]


def coeffs_of(n, k, arrays):
    """the layout inverted in numpy, written independently of the library: (a, ct0) signed, ascending degree"""
    def signed(words):
        w = words.astype(object)
        return np.array([int(v) if int(v) < P // 2 else int(v) - P for v in w], dtype=np.int64)
    a = np.concatenate([signed(arrays["ais"][i * 2 * n:i * 2 * n + n][::-1]) for i in range(k)])
    ct0 = np.concatenate([signed(arrays["ct0is"][i * 2 * n + n - 1:i * 2 * n + 2 * n - 1][::-1]) for i in range(k)])
    return a, ct0


def load(prefix, n, k, bits):
    bfv = hg.BfvEncrypt.new(n, k)
    path = os.path.join(orclib.GOLDEN, f"{prefix}sk_enc_{n}_{k}x{bits}_65537.json")
    return bfv, (hg.Witness.from_json_bn254(bfv.params, path) if prefix else bfv.get_inputs(path))


_CASES = {}


def case(n, k, bits):
    """per shape: host-only key, fixture witness, its instance and the oracle's proofs in modes 0 and 3 (computed once, never changed)"""
    if (n, k) not in _CASES:
        bfv, w = load("", n, k, bits)
        d = w.arrays()
        proofs = {m: orclib.prove_f("goldilocks", orclib.params(n, k), orclib.Inputs(d), threads=8, mode=m)[0] for m in (0, 3)}
        _CASES[(n, k)] = dict(bfv=bfv, pk=bfv.setup(None), w=w, d=d, inst=hg.Instance.from_witness(w), proofs=proofs)
    return _CASES[(n, k)]


def changed_witness(c, field, index=0):
    d = {f: v.copy() for f, v in c["d"].items()}
    d[field][index] = (int(d[field][index]) + 1) % P
    return hg.Witness.from_arrays(c["bfv"].params, d)


# ---- 1. surface ------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "hg.h")).read()
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert "typedef struct hg_instance hg_instance;" in hdr and re.search(r"typedef struct hg_input_claim \{.*?\} hg_input_claim;", hdr, flags=re.S)
    assert C.sizeof(hg.HgInputClaim) == 32 and "pub struct HgInputClaim" in rs


def _last():
    return hg.lib().hg_last_error().decode()


def test_bad_arguments_are_errors_naming_the_function():
    c = case(1024, 1, 27)
    L, pk, inst, w, params = hg.lib(), c["pk"], c["inst"], c["w"], c["bfv"].params
    proof = c["proofs"][3]
    nc, nco = hg.pk_claim_shape(pk)
    claims, pts, n = (hg.HgInputClaim * nc)(), np.zeros(2 * nco, dtype=np.uint64), C.c_size_t(7)
    tail = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, hg.u64p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.hg_verify_public.argtypes = tail
    L.hg_verify_public_device.argtypes = [C.c_void_p] + tail
    L.hg_claims_settle.argtypes = [C.c_void_p, C.POINTER(hg.HgParams), C.c_void_p, C.c_void_p, C.c_size_t, hg.u64p]
    L.hg_instance_mle.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, hg.u64p, C.c_size_t, hg.u64p]
    L.hg_pk_claim_shape.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.hg_instance_from_ciphertext.argtypes = [C.POINTER(hg.HgParams), hg.i64p, hg.i64p, C.POINTER(C.c_void_p)]
    L.hg_instance_from_witness.argtypes = [C.POINTER(hg.HgParams), C.c_void_p, C.POINTER(C.c_void_p)]
    pp, np_ = hg._ptr(pts), C.byref(n)
    other = hg.Instance.from_witness(hg.Witness.synthetic(hg.params_builtin(2048, 1), 5))   # an instance of other params
    good = (pk.h, inst.h, 3, proof, len(proof), claims, nc, pp, nco, np_)

    def sub(i, v):
        return good[:i] + (v,) + good[i + 1:]
    bad = [sub(0, None), sub(1, None), sub(3, None), sub(9, None), sub(5, None), sub(7, None), sub(2, -1), sub(2, 4), sub(6, nc - 1), sub(8, nco - 1), sub(1, other.h)]
    for args in bad:
        n.value = 7
        assert L.hg_verify_public(*args) == -1, args
        assert "hg_verify_public" in _last() and "device" not in _last()
        assert args[9] is None or n.value == 0
        assert L.hg_verify_public_device(None, *args) == -1      # no context
        assert "hg_verify_public_device" in _last()
    assert L.hg_verify_public(*good) == 0 and n.value == nc
    # the other entries
    a, ct0 = inst.coeffs()
    h = C.c_void_p()
    ia, ic = a.ctypes.data_as(hg.i64p), ct0.ctypes.data_as(hg.i64p)
    for args in ((None, ia, ic, C.byref(h)), (C.byref(params), None, ic, C.byref(h)), (C.byref(params), ia, None, C.byref(h)), (C.byref(params), ia, ic, None)):
        assert L.hg_instance_from_ciphertext(*args) == -1 and "hg_instance_from_ciphertext" in _last()
    for args in ((None, w.h, C.byref(h)), (C.byref(params), None, C.byref(h)), (C.byref(params), w.h, None), (C.byref(hg.params_builtin(2048, 1)), w.h, C.byref(h))):
        assert L.hg_instance_from_witness(*args) == -1 and "hg_instance_from_witness" in _last()
    a_, b_ = C.c_size_t(0), C.c_size_t(0)
    for args in ((None, C.byref(a_), C.byref(b_)), (pk.h, None, C.byref(b_)), (pk.h, C.byref(a_), None)):
        assert L.hg_pk_claim_shape(*args) == -1 and "hg_pk_claim_shape" in _last()
    ok, _, cl = hg.verify_public(pk, inst, proof, 3)
    assert ok
    for args in ((None, None, w.h, cl.claims, cl.n, pp), (None, C.byref(params), None, cl.claims, cl.n, pp), (None, C.byref(params), w.h, None, cl.n, pp),
                 (None, C.byref(params), w.h, cl.claims, cl.n, None), (None, C.byref(hg.params_builtin(2048, 1)), w.h, cl.claims, cl.n, pp)):
        assert L.hg_claims_settle(*args) == -1 and "hg_claims_settle" in _last()
    wrong = (hg.HgInputClaim * 1)()
    wrong[0].input, wrong[0].nvars = 3 + 2 * 1 + 1, 11      # no such input
    assert L.hg_claims_settle(None, C.byref(params), w.h, wrong, 1, pp) == -1 and "hg_claims_settle" in _last()
    wrong[0].input, wrong[0].nvars = 0, 10                   # a point that is not the table's
    assert L.hg_claims_settle(None, C.byref(params), w.h, wrong, 1, pp) == -1 and "hg_claims_settle" in _last()
    out = np.zeros(2, dtype=np.uint64)
    pt = flat(points(11, 1)[0])
    for args in ((None, None, 0, 0, hg._ptr(pt), 11, hg._ptr(out)), (None, inst.h, 0, 0, None, 11, hg._ptr(out)), (None, inst.h, 0, 0, hg._ptr(pt), 11, None),
                 (None, inst.h, 2, 0, hg._ptr(pt), 11, hg._ptr(out)), (None, inst.h, 0, 1, hg._ptr(pt), 11, hg._ptr(out)), (None, inst.h, 0, 0, hg._ptr(pt), 10, hg._ptr(out))):
        assert L.hg_instance_mle(*args) == -1 and "hg_instance_mle" in _last()
    if have_gpu():   # a device context with a host-only key
        ctx = hg.Context(0)
        try:
            assert L.hg_verify_public_device(ctx.h, *good) == -1 and "hg_verify_public_device" in _last()
        finally:
            ctx.close()


# ---- 2. layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix,n,k,bits", GL_FIXTURES)
def test_instance_layout_reproduces_the_fixture_tables(prefix, n, k, bits):
    bfv, w = load(prefix, n, k, bits)
    d = w.arrays()
    from_w = hg.Instance.from_witness(w)
    a, ct0 = from_w.coeffs()
    ra, rct0 = coeffs_of(n, k, d)
    assert (a == ra).all() and (ct0 == rct0).all()
    from_c = hg.Instance.from_ciphertext(bfv.params, a, ct0)
    for inst in (from_w, from_c):
        assert (inst.table(0) == d["ais"]).all() and (inst.table(1) == d["ct0is"]).all()   # word for word
    # the evaluator reads the same layout: unit-vector points pick single words (first / last coefficient, padding on both sides)
    L, lk = n.bit_length(), k.bit_length() - 1
    for i in sorted({0, k - 1}):
        for word in (0, 1, n - 2, n - 1, n, 2 * n - 2, 2 * n - 1):
            got = from_c.mle(None, 0, i, flat(unit_point(word, L)))
            assert (int(got[0]), int(got[1])) == (int(d["ais"][i * 2 * n + word]), 0), (i, word)
            got = from_c.mle(None, 1, 0, flat(unit_point(i * 2 * n + word, L + lk)))
            assert (int(got[0]), int(got[1])) == (int(d["ct0is"][i * 2 * n + word]), 0), (i, word)


def test_coefficient_range_is_enforced():
    bfv = hg.BfvEncrypt.new(4096, 2)
    n, k, q = 4096, 2, [int(x) for x in bfv.params.qis[:2]]
    zero = np.zeros(k * n, dtype=np.int64)
    z = hg.Instance.from_ciphertext(bfv.params, zero, zero)                      # the all-zero polynomial
    assert not z.table(0).any() and not z.table(1).any()
    edge = np.concatenate([np.where(np.arange(n) % 2 == 0, (q[i] - 1) // 2, -((q[i] - 1) // 2)) for i in range(k)]).astype(np.int64)
    e = hg.Instance.from_ciphertext(bfv.params, edge, -edge)                     # +-(q_i-1)/2 everywhere
    assert (e.coeffs()[0] == edge).all() and (e.coeffs()[1] == -edge).all()
    assert int(e.table(0)[n - 1]) == (q[0] - 1) // 2 and int(e.table(1)[2 * n - 2]) == P - (q[0] - 1) // 2
    for tab, name in ((0, "a"), (1, "ct0")):
        for i, j, sign in ((0, 0, 1), (1, n - 1, -1), (1, 17, 1)):
            arrs = [zero.copy(), zero.copy()]
            arrs[tab][i * n + j] = sign * ((q[i] - 1) // 2 + 1)
            with pytest.raises(hg.HgError, match=r"hg_instance_from_ciphertext: %s, modulus %d, coefficient %d\b" % (name, i, j)):
                hg.Instance.from_ciphertext(bfv.params, *arrs)
    # from_witness: a nonzero padding word, a word that is no small signed value
    c = case(1024, 1, 27)
    for field, index in (("ais", 1024), ("ct0is", 0), ("ct0is", 2047)):
        with pytest.raises(hg.HgError, match="hg_instance_from_witness: %s, modulus 0, word %d is padding" % (field, index)):
            hg.Instance.from_witness(changed_witness(c, field, index))
    d = {f: v.copy() for f, v in c["d"].items()}
    d["ais"][5] = 1 << 40
    with pytest.raises(hg.HgError, match="hg_instance_from_witness: ais, modulus 0, word 5 is not a signed value"):
        hg.Instance.from_witness(hg.Witness.from_arrays(c["bfv"].params, d))


# ---- 3. host hg_instance_mle -----------------------------------------------------------------------------------------------------
def mle_cases():
    """(case, which, index, nvars, laid-out table): (1024,1) both tables, (4096,2) ct0is"""
    c1, c2 = case(1024, 1, 27), case(4096, 2, 55)
    return [(c1, 0, 0, 11, c1["d"]["ais"]), (c1, 1, 0, 11, c1["d"]["ct0is"]), (c2, 1, 0, 14, c2["d"]["ct0is"])]


def test_host_instance_mle_is_the_mle_of_the_laid_out_table():
    for c, which, index, nv, table in mle_cases():
        for pt in points(nv, 100 + nv + which):
            got = c["inst"].mle(None, which, index, flat(pt))
            assert (int(got[0]), int(got[1])) == py_mle(table, pt), (which, nv)


# ---- 4. split equivalence --------------------------------------------------------------------------------------------------------
OFFSETS = lambda ln: [0, ln - 1] + [ln * i // 16 for i in range(1, 16)]   # noqa: E731


def split_equivalence(c, mode, proof, public, settle):
    """public(inst, proof) -> (ok, reason, claims); settle(witness, claims) -> (ok, reason). The whole of test 4 for one proof."""
    bfv, pk, w, inst, k = c["bfv"], c["pk"], c["w"], c["inst"], c["bfv"].params.k
    ok, why, cl = public(inst, proof)
    assert ok, why
    nc, nco = hg.pk_claim_shape(pk)
    tup = cl.as_tuples()
    assert cl.n == nc and sum(t[1] for t in tup) == nco
    assert [t[0] for t in tup] == sorted(t[0] for t in tup) and not any(3 <= t[0] < 3 + k for t in tup)
    assert {t[0] for t in tup} == {0, 1, 2, 3 + 2 * k} | {3 + k + i for i in range(k)}     # every secret input carries a claim
    assert settle(w, cl) == (True, "")
    # a changed secret: the instance is unchanged, so the public part still accepts; the settle step rejects with the verifier's text
    for field, name in (("s", 0), ("r2is", 3 + 2 * k)):
        w2 = changed_witness(c, field)
        want = hg.verify(pk, w2, proof, mode=mode)
        assert want == (False, "input claim mismatch at input %d" % name)
        assert settle(w2, cl) == want
    # a changed instance: the public part rejects, for the reason hg_verify_mode gives for the handle rebuilt with the same change
    a, ct0 = inst.coeffs()
    n = bfv.params.n
    for tab, j in ((1, 3), (0, n * k - 2)):
        arrs = [a.copy(), ct0.copy()]
        arrs[tab][j] += 1
        inst2 = hg.Instance.from_ciphertext(bfv.params, *arrs)
        d = {f: v.copy() for f, v in c["d"].items()}
        d["ais"], d["ct0is"] = inst2.table(0), inst2.table(1)
        want = hg.verify(pk, hg.Witness.from_arrays(bfv.params, d), proof, mode=mode)
        got = public(inst2, proof)
        assert not want[0] and got[:2] == want, (tab, got[:2], want)
    # proof tampering: one bit at each fixed offset; (public, then settle) makes the decision of hg_verify_mode
    # and that decision is a rejection: every element of the stream is bound (tests/test_proof_binding.py)
    for at in OFFSETS(len(proof)):
        bad = bytearray(proof)
        bad[at] ^= 0x04
        bad = bytes(bad)
        want = hg.verify(pk, w, bad, mode=mode)[0]
        ok, _, cl2 = public(inst, bad)
        got = ok and settle(w, cl2)[0]
        assert not want and got == want, (mode, at, got, want)


@pytest.mark.parametrize("n,k,bits", SHAPES)
@pytest.mark.parametrize("mode", [0, 3])
def test_public_part_and_settle_step_decide_what_hg_verify_mode_decides(n, k, bits, mode):
    c = case(n, k, bits)
    split_equivalence(c, mode, c["proofs"][mode], lambda inst, proof: hg.verify_public(c["pk"], inst, proof, mode),
                      lambda w, cl: hg.claims_settle(None, c["bfv"].params, w, cl))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_kernel_parity_with_the_host_form_and_hg_mle_eval(ctx):
    """5. the compact dot kernel against the host loop and against hg_mle_eval of the laid-out table; extreme coefficients too"""
    todo = [(c["inst"], which, index, nv, table) for c, which, index, nv, table in mle_cases()]
    bfv = case(4096, 2, 55)["bfv"]
    n, k, q = 4096, 2, [int(x) for x in bfv.params.qis[:2]]
    half = np.concatenate([np.full(n, (q[i] - 1) // 2) for i in range(k)]).astype(np.int64)
    alt = half * np.where(np.arange(k * n) % 2 == 0, 1, -1)
    for a, ct0 in ((half, half), (-half, -half), (alt, -alt)):
        inst = hg.Instance.from_ciphertext(bfv.params, a, ct0)
        todo += [(inst, 0, 1, 13, inst.table(0)[2 * n:]), (inst, 1, 0, 14, inst.table(1))]
    for inst, which, index, nv, table in todo:
        for pt in points(nv, 200 + nv + which):
            dev = inst.mle(ctx, which, index, flat(pt))
            assert (dev == inst.mle(None, which, index, flat(pt))).all(), (which, nv)
            assert (dev == ctx.mle_eval(table, flat(pt))).all(), (which, nv)


def gpu_case(ctx, n, k, seed=None):
    bfv = hg.BfvEncrypt.new(n, k)
    return dict(bfv=bfv, pk=bfv.setup(ctx), w=hg.Witness.synthetic(bfv.params, seed or 0x9b1 + n))


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", SHAPES)
def test_device_form_returns_the_host_forms_decision_claims_and_points(ctx, n, k, bits):
    """6. proofs from hg_prove_mode, modes 0..3: the same decision, claim list and points, bit for bit - accepted and rejected"""
    g = gpu_case(ctx, n, k)
    bfv, pk, w = g["bfv"], g["pk"], g["w"]
    inst = hg.Instance.from_witness(w)
    for mode in range(4):
        proof, _ = bfv.prove(ctx, pk, w, mode=mode)
        host = hg.verify_public(pk, inst, proof, mode)
        dev = hg.verify_public(pk, inst, proof, mode, ctx=ctx, device=True)
        assert host[0] and dev[0], (mode, host[1], dev[1])
        assert dev[2].as_tuples() == host[2].as_tuples(), mode
        assert hg.claims_settle(None, bfv.params, w, dev[2]) == (True, "")
        for at in (len(proof) // 3, len(proof) - 9):
            bad = bytearray(proof)
            bad[at] ^= 0x20
            h, d = hg.verify_public(pk, inst, bytes(bad), mode), hg.verify_public(pk, inst, bytes(bad), mode, ctx=ctx, device=True)
            assert h[:2] == d[:2] and (h[2] is None) == (d[2] is None), (mode, at, h[:2], d[:2])
            if h[0]:
                assert h[2].as_tuples() == d[2].as_tuples()
    pk.free()


@pytest.mark.gpu
def test_device_settle_equals_the_host_settle(ctx):
    """7. on the accepting case and on the changed-s case of test 4"""
    c = case(1024, 1, 27)
    for mode in (0, 3):
        ok, _, cl = hg.verify_public(c["pk"], c["inst"], c["proofs"][mode], mode)
        assert ok
        for w in (c["w"], changed_witness(c, "s"), changed_witness(c, "r1is", 7)):
            host = hg.claims_settle(None, c["bfv"].params, w, cl)
            assert hg.claims_settle(ctx, c["bfv"].params, w, cl) == host
        assert host == (False, "input claim mismatch at input 4")


@pytest.mark.gpu
def test_whole_split_equivalence_through_the_device_entries(ctx):
    """8. test 4 at (1024,1) in mode 3 with hg_verify_public_device and the device settle"""
    c = dict(case(1024, 1, 27))
    c["pk"] = c["bfv"].setup(ctx)
    split_equivalence(c, 3, c["proofs"][3], lambda inst, proof: hg.verify_public(c["pk"], inst, proof, 3, ctx=ctx, device=True),
                      lambda w, cl: hg.claims_settle(ctx, c["bfv"].params, w, cl))
    c["pk"].free()


@pytest.mark.gpu
def test_neighbours_on_the_context_are_undisturbed(ctx):
    """9. around a mode-3 public verification hg_verify_device and hg_prove give what they gave before: the fixed chain is untouched"""
    g = gpu_case(ctx, 4096, 2, seed=0x4c4c)
    bfv, pk, w = g["bfv"], g["pk"], g["w"]
    inst = hg.Instance.from_witness(w)
    p3, _ = bfv.prove(ctx, pk, w, mode=3)
    first = [bfv.prove(ctx, pk, w)[0] for _ in range(3)]
    assert first[0] == first[1] == first[2]
    for i in range(2):
        ok, why, cl = hg.verify_public(pk, inst, p3, 3, ctx=ctx, device=True)
        assert ok, why
        assert hg.claims_settle(ctx, bfv.params, w, cl) == (True, "")
        assert bfv.prove(ctx, pk, w)[0] == first[0], i
        assert hg.verify_device(ctx, pk, w, first[0]) == (True, ""), i
        assert hg.verify_device(ctx, pk, w, p3, mode=3) == (True, ""), i
    ok, why, cl0 = hg.verify_public(pk, inst, first[0], 0, ctx=ctx, device=True)
    assert ok and hg.claims_settle(ctx, bfv.params, w, cl0) == (True, "")
    pk.free()


@pytest.mark.gpu
def test_full_size_mode_3(ctx):
    """10. (32768,16), a synthetic witness: the public device form accepts, the settle accepts, a changed ct0 coefficient is rejected"""
    g = gpu_case(ctx, 32768, 16, seed=0x8000 + 16)
    bfv, pk, w = g["bfv"], g["pk"], g["w"]
    proof, _ = bfv.prove(ctx, pk, w, cap=1 << 25, mode=3)
    inst = hg.Instance.from_witness(w)
    ok, why, cl = hg.verify_public(pk, inst, proof, 3, ctx=ctx, device=True)
    assert ok, why
    assert (cl.n, sum(t[1] for t in cl.as_tuples())) == hg.pk_claim_shape(pk)
    assert hg.claims_settle(ctx, bfv.params, w, cl) == (True, "")
    a, ct0 = inst.coeffs()
    ct0[11 * 32768 + 12345] += 1
    bad = hg.Instance.from_ciphertext(bfv.params, a, ct0)
    assert not hg.verify_public(pk, bad, proof, 3, ctx=ctx, device=True)[0]
    pk.free()
