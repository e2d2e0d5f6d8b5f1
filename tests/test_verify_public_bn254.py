"""hg_verify_public_bn254 / hg_claims_settle_bn254: the verifier split of test_verify_public.py over bn256::Fr. The public part decides
everything the key, the proof, a_i and ct0_i decide and returns the claims left on the five secret inputs (4 canonical limbs per
element); the settle step checks those against a witness handle. hg_verify_bn254 is the yardstick: the two parts together make
its decision for every proof, honest or tampered."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import orclib
from orclib import P, R_BN as R
from hglib import hg, ROOT, have_gpu

NEW = ["hg_verify_public_bn254", "hg_verify_public_device_bn254", "hg_claims_settle_bn254", "hg_instance_mle_bn254"]
SHAPES = [(1024, 1, 27), (4096, 2, 55)]
OFFSETS = lambda ln: [0, ln - 1] + [ln * i // 16 for i in range(1, 16)]   # noqa: E731  (the 17 offsets of test_verify_public.py)


# ---- Python-integer arithmetic mod r and the MLE of a table ---------------------------------------------------------------------------
def fr_of(word):
    """a table word (small signed integer in the Goldilocks form: z < 0 as p - |z|) as an element of Fr"""
    w = int(word)
    return w if w < P // 2 else (w - P) % R


def eq_table(pt):
    """eq(pt, x), x_0 the lowest bit of the index"""
    t = [1]
    for r in pt:
        hi = [v * r % R for v in t]
        t = [(v - h) % R for v, h in zip(t, hi)] + hi
    return t


def py_mle(table, pt):
    eq = eq_table(pt)
    assert len(eq) == len(table)
    return sum(fr_of(v) * e for v, e in zip(table, eq) if int(v)) % R


def points(nvars, seed):
    """two random Fr points, the all-zero point and the all-ones point"""
    rng = random.Random(seed)
    return [[rng.randrange(R) for _ in range(nvars)] for _ in range(2)] + [[0] * nvars, [1] * nvars]


def unit_point(index, nvars):
    return [(index >> b) & 1 for b in range(nvars)]


UNIT_WORDS = lambda n: (0, 1, n - 2, n - 1, n, 2 * n - 2, 2 * n - 1)   # noqa: E731


def limbs(vals):
    return orclib.to_limbs(vals, 4)


_CASES = {}


def case(n, k, bits):
    """per shape: host-only key, the reference's bn254 fixture, its instance and the oracle's proof (computed once, never changed)"""
    if (n, k) not in _CASES:
        bfv = hg.BfvEncrypt.new(n, k)
        w = hg.Witness.from_json_bn254(bfv.params, os.path.join(orclib.GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json"))
        proof = orclib.prove_f("bn254", orclib.params(n, k), orclib.bn254_fixture_inputs(n, k, bits), threads=8)[0]
        _CASES[(n, k)] = dict(bfv=bfv, pk=bfv.setup(None), w=w, d=w.arrays(), inst=hg.Instance.from_witness(w), proof=proof)
    return _CASES[(n, k)]


def changed_witness(c, field, index=0):
    d = {f: v.copy() for f, v in c["d"].items()}
    d[field][index] = (int(d[field][index]) + 1) % P
    return hg.Witness.from_arrays(c["bfv"].params, d)


def _last():
    return hg.lib().hg_last_error().decode()


# ---- 1. surface ------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "hg.h")).read()
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert re.search(r"typedef struct hg_input_claim_bn254 \{.*?\} hg_input_claim_bn254;", hdr, flags=re.S)
    # two u32, one u64 and four u64 limbs: 4 + 4 + 8 + 32 = 48 bytes, no padding (the request for this struct said 56 beside the same
    # four fields; the fields are the ABI, and a C compiler lays them out in 48)
    assert C.sizeof(hg.HgInputClaimBn254) == 48 and "pub struct HgInputClaimBn254" in rs
    fields = re.search(r"typedef struct hg_input_claim_bn254 \{(.*?)\}", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), flags=re.S).group(1).split()
    assert fields == ["uint32_t", "input;", "uint32_t", "nvars;", "uint64_t", "point_off;", "uint64_t", "value[4];"]


# ---- 2. bad arguments ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors_naming_the_function():
    c = case(1024, 1, 27)
    L, pk, inst, w, params, proof = hg.lib(), c["pk"], c["inst"], c["w"], c["bfv"].params, c["proof"]
    nc, nco = hg.pk_claim_shape(pk)
    claims, pts, n = (hg.HgInputClaimBn254 * nc)(), np.zeros(4 * nco, dtype=np.uint64), C.c_size_t(7)
    tail = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, hg.u64p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.hg_verify_public_bn254.argtypes = tail
    L.hg_verify_public_device_bn254.argtypes = [C.c_void_p] + tail
    L.hg_claims_settle_bn254.argtypes = [C.c_void_p, C.POINTER(hg.HgParams), C.c_void_p, C.c_void_p, C.c_size_t, hg.u64p]
    L.hg_instance_mle_bn254.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, hg.u64p, C.c_size_t, hg.u64p]
    pp, np_ = hg._ptr(pts), C.byref(n)
    other = hg.Instance.from_witness(hg.Witness.synthetic(hg.params_builtin(2048, 1), 5))   # an instance of other params
    good = (pk.h, inst.h, proof, len(proof), claims, nc, pp, nco, np_)

    def sub(i, v):
        return good[:i] + (v,) + good[i + 1:]
    bad = [sub(0, None), sub(1, None), sub(2, None), sub(8, None), sub(4, None), sub(6, None), sub(5, nc - 1), sub(7, nco - 1), sub(1, other.h)]
    for args in bad:
        n.value = 7
        assert L.hg_verify_public_bn254(*args) == -1, args
        assert "hg_verify_public_bn254" in _last()
        assert args[8] is None or n.value == 0
        n.value = 7
        assert L.hg_verify_public_device_bn254(None, *args) == -1      # no context
        assert "hg_verify_public_device_bn254" in _last()
        assert args[8] is None or n.value == 0
    n.value = 7
    assert L.hg_verify_public_device_bn254(None, *good) == -1 and "hg_verify_public_device_bn254" in _last() and n.value == 0
    assert L.hg_verify_public_bn254(*good) == 0 and n.value == nc
    # the settle step
    ok, _, cl = hg.verify_public_bn254(pk, inst, proof)
    assert ok
    cp = hg._ptr(cl.points)
    for args in ((None, None, w.h, cl.claims, cl.n, cp), (None, C.byref(params), None, cl.claims, cl.n, cp), (None, C.byref(params), w.h, None, cl.n, cp),
                 (None, C.byref(params), w.h, cl.claims, cl.n, None), (None, C.byref(hg.params_builtin(2048, 1)), w.h, cl.claims, cl.n, cp)):
        assert L.hg_claims_settle_bn254(*args) == -1 and "hg_claims_settle_bn254" in _last()
    wrong = (hg.HgInputClaimBn254 * 1)()
    zeros = np.zeros(4 * 16, dtype=np.uint64)
    wrong[0].input, wrong[0].nvars = 3 + 2 * 1 + 1, 11      # no such input
    assert L.hg_claims_settle_bn254(None, C.byref(params), w.h, wrong, 1, hg._ptr(zeros)) == -1 and "hg_claims_settle_bn254" in _last()
    wrong[0].input, wrong[0].nvars = 0, 10                   # a point that is not the table's
    assert L.hg_claims_settle_bn254(None, C.byref(params), w.h, wrong, 1, hg._ptr(zeros)) == -1 and "hg_claims_settle_bn254" in _last()
    wrong[0].input, wrong[0].nvars = 0, 11
    for v in (R, (1 << 256) - 1):                            # not below r: a coordinate, then the value
        pt = limbs([0] * 10 + [v])
        assert L.hg_claims_settle_bn254(None, C.byref(params), w.h, wrong, 1, hg._ptr(pt)) == -1 and "hg_claims_settle_bn254: non-canonical coordinate" in _last()
        for j in range(4):
            wrong[0].value[j] = int(limbs([v])[j])
        assert L.hg_claims_settle_bn254(None, C.byref(params), w.h, wrong, 1, hg._ptr(zeros)) == -1 and "hg_claims_settle_bn254: non-canonical value" in _last()
        for j in range(4):
            wrong[0].value[j] = 0
    # the evaluator
    out = np.zeros(4, dtype=np.uint64)
    pt = limbs(points(11, 1)[0])
    for args in ((None, None, 0, 0, hg._ptr(pt), 11, hg._ptr(out)), (None, inst.h, 0, 0, None, 11, hg._ptr(out)), (None, inst.h, 0, 0, hg._ptr(pt), 11, None),
                 (None, inst.h, 2, 0, hg._ptr(pt), 11, hg._ptr(out)), (None, inst.h, 0, 1, hg._ptr(pt), 11, hg._ptr(out)), (None, inst.h, 0, 0, hg._ptr(pt), 10, hg._ptr(out)),
                 (None, inst.h, 0, 0, hg._ptr(limbs([1] * 10 + [R])), 11, hg._ptr(out))):
        assert L.hg_instance_mle_bn254(*args) == -1 and "hg_instance_mle_bn254" in _last()
    if have_gpu():   # a device context with a host-only key
        ctx = hg.Context(0)
        try:
            n.value = 7
            assert L.hg_verify_public_device_bn254(ctx.h, *good) == -1 and "hg_verify_public_device_bn254" in _last() and n.value == 0
        finally:
            ctx.close()


# ---- 3. host hg_instance_mle_bn254 -----------------------------------------------------------------------------------------------
def mle_cases():
    """(instance, which, index, nvars, laid-out table, n, k): (1024,1) both tables, (4096,2) ct0is"""
    c1, c2 = case(1024, 1, 27), case(4096, 2, 55)
    return [(c1["inst"], 0, 0, 11, c1["d"]["ais"], 1024, 1), (c1["inst"], 1, 0, 11, c1["d"]["ct0is"], 1024, 1), (c2["inst"], 1, 0, 14, c2["d"]["ct0is"], 4096, 2)]


def unit_words(which, index, n, k):
    """word indices of the unit-vector points: 0, 1, n-2, n-1, n, 2n-2, 2n-1 of the first and the last modulus"""
    if which == 0:
        return list(UNIT_WORDS(n))
    return [i * 2 * n + word for i in sorted({0, k - 1}) for word in UNIT_WORDS(n)]


def test_host_instance_mle_is_the_mle_of_the_laid_out_table():
    for inst, which, index, nv, table, n, k in mle_cases():
        for pt in points(nv, 100 + nv + which):
            assert inst.mle_bn254(None, which, index, pt) == py_mle(table, pt), (which, nv)
        for word in unit_words(which, index, n, k):
            assert inst.mle_bn254(None, which, index, unit_point(word, nv)) == fr_of(table[word]), (which, nv, word)
    # ais of the last modulus at (4096,2): the unit points of its own block
    c2 = case(4096, 2, 55)
    for word in UNIT_WORDS(4096):
        assert c2["inst"].mle_bn254(None, 0, 1, unit_point(word, 13)) == fr_of(c2["d"]["ais"][2 * 4096 + word]), word


# ---- 4. split equivalence --------------------------------------------------------------------------------------------------------
def split_equivalence(c, public, settle):
    """public(inst, proof) -> (ok, reason, claims); settle(witness, claims) -> (ok, reason)"""
    bfv, pk, w, inst, proof, k = c["bfv"], c["pk"], c["w"], c["inst"], c["proof"], c["bfv"].params.k
    assert hg.verify_bn254(pk, w, proof) == (True, "")
    ok, why, cl = public(inst, proof)
    assert ok, why
    nc, nco = hg.pk_claim_shape(pk)
    tup = cl.as_tuples()
    assert cl.n == nc and sum(t[1] for t in tup) == nco
    assert [t[0] for t in tup] == sorted(t[0] for t in tup) and not any(3 <= t[0] < 3 + k for t in tup)
    assert {t[0] for t in tup} == {0, 1, 2, 3 + 2 * k} | {3 + k + i for i in range(k)}     # every secret input carries a claim
    assert all(v < R for t in tup for v in orclib.from_limbs(t[2] + t[3], 4))               # canonical limbs
    assert settle(w, cl) == (True, "")
    # a changed secret: the instance is unchanged, so the public part still accepts; the settle step rejects with the verifier's text
    for field, name in (("s", 0), ("r2is", 3 + 2 * k)):
        w2 = changed_witness(c, field)
        want = hg.verify_bn254(pk, w2, proof)
        assert want == (False, "input claim mismatch at input %d" % name)
        assert settle(w2, cl) == want
    # a changed instance: the public part rejects, for the reason hg_verify_bn254 gives for the handle rebuilt with the same change
    a, ct0 = inst.coeffs()
    n = bfv.params.n
    for tab, j in ((1, 3), (0, n * k - 2)):
        arrs = [a.copy(), ct0.copy()]
        arrs[tab][j] += 1
        inst2 = hg.Instance.from_ciphertext(bfv.params, *arrs)
        d = {f: v.copy() for f, v in c["d"].items()}
        d["ais"], d["ct0is"] = inst2.table(0), inst2.table(1)
        want = hg.verify_bn254(pk, hg.Witness.from_arrays(bfv.params, d), proof)
        got = public(inst2, proof)
        assert not want[0] and got[:2] == want and got[2] is None, (tab, got[:2], want)
    # proof tampering: one bit at each fixed offset, and an element that is no residue; (public, then settle) decides what hg_verify_bn254 decides
    tampered = []
    for at in OFFSETS(len(proof)):
        bad = bytearray(proof)
        bad[at] ^= 0x04
        tampered.append((at, bytes(bad)))
    bad = bytearray(proof)
    bad[32 * (len(proof) // 32 // 4)] = 0xff   # (big-endian elements: the top byte set makes it >= r)
    tampered.append(("non-canonical", bytes(bad)))
    # and that decision is a rejection: every element of the stream is bound (tests/test_proof_binding.py)
    for at, bad in tampered:
        want = hg.verify_bn254(pk, w, bad)
        ok, why, cl2 = public(inst, bad)
        got = ok and settle(w, cl2)[0]
        assert not want[0] and got == want[0], (at, got, why, want)


@pytest.mark.parametrize("n,k,bits", SHAPES)
def test_public_part_and_settle_step_decide_what_hg_verify_bn254_decides(n, k, bits):
    c = case(n, k, bits)
    split_equivalence(c, lambda inst, proof: hg.verify_public_bn254(c["pk"], inst, proof), lambda w, cl: hg.claims_settle_bn254(None, c["bfv"].params, w, cl))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def parity(ctx, inst, which, index, nv, table, n, k, seed):
    """the compact dot kernel against the host loop and against hg_mle_eval_bn254 of the laid-out table (lifted into Fr once)"""
    tab4 = limbs([fr_of(v) for v in table])
    L = hg.lib()
    pts = points(nv, seed) + [unit_point(word, nv) for word in unit_words(which, index, n, k)]
    for pt in pts:
        dev = inst.mle_bn254(ctx, which, index, pt)
        assert dev == inst.mle_bn254(None, which, index, pt), (which, nv)
        out = np.zeros(4, dtype=np.uint64)
        assert L.hg_mle_eval_bn254(ctx.h, hg._ptr(tab4), nv, hg._ptr(limbs(pt)), hg._ptr(out)) == 0, _last()
        assert dev == orclib.from_limbs(out, 4)[0], (which, nv)


@pytest.mark.gpu
def test_kernel_parity_on_the_fixtures(ctx):
    """5a. (1024,1) ais and ct0is: less than one tile; (4096,2) ct0is: one tile that crosses the block boundary"""
    for i, (inst, which, index, nv, table, n, k) in enumerate(mle_cases()):
        parity(ctx, inst, which, index, nv, table, n, k, 200 + i)


@pytest.mark.gpu
def test_kernel_parity_over_several_tiles(ctx):
    """5b. (8192,4) on a synthetic witness: ct0is (four tiles) and ais of the last modulus"""
    n, k = 8192, 4
    w = hg.Witness.synthetic(hg.params_builtin(n, k), 0xb2f4)
    inst = hg.Instance.from_witness(w)
    parity(ctx, inst, 1, 0, 16, inst.table(1), n, k, 210)
    parity(ctx, inst, 0, 3, 14, inst.table(0)[3 * 2 * n:], n, k, 211)


@pytest.mark.gpu
@pytest.mark.parametrize("signs", ["plus", "minus", "alternating"])
def test_kernel_parity_at_the_extreme_coefficients(ctx, signs):
    """5c. (4096,2): every coefficient +(q_i-1)/2, every coefficient -(q_i-1)/2, alternating signs"""
    n, k = 4096, 2
    params = hg.params_builtin(n, k)
    q = [int(x) for x in params.qis[:k]]
    half = np.concatenate([np.full(n, (q[i] - 1) // 2) for i in range(k)]).astype(np.int64)
    alt = half * np.where(np.arange(k * n) % 2 == 0, 1, -1)
    a, ct0 = {"plus": (half, half), "minus": (-half, -half), "alternating": (alt, -alt)}[signs]
    inst = hg.Instance.from_ciphertext(params, a, ct0)
    parity(ctx, inst, 0, 1, 13, inst.table(0)[2 * n:], n, k, 220)
    parity(ctx, inst, 1, 0, 14, inst.table(1), n, k, 221)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", SHAPES)
def test_device_form_returns_the_host_forms_decision_claims_and_points(ctx, n, k, bits):
    """6. proofs from hg_prove_bn254 of a synthetic witness: the same decision, claim list and points, bit for bit - accepted and rejected"""
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x9b1 + n)
    inst = hg.Instance.from_witness(w)
    proof = ctx.prove_bn254(pk, w)[0]
    host = hg.verify_public_bn254(pk, inst, proof)
    dev = hg.verify_public_bn254(pk, inst, proof, ctx=ctx, device=True)
    assert host[0] and dev[0], (host[1], dev[1])
    assert dev[2].as_tuples() == host[2].as_tuples()
    assert hg.claims_settle_bn254(None, bfv.params, w, dev[2]) == (True, "")
    for at in (len(proof) // 3, len(proof) - 9):
        for bit in (0x20, 0x01):
            bad = bytearray(proof)
            bad[at] ^= bit
            h, d = hg.verify_public_bn254(pk, inst, bytes(bad)), hg.verify_public_bn254(pk, inst, bytes(bad), ctx=ctx, device=True)
            assert h[:2] == d[:2] and (h[2] is None) == (d[2] is None), (at, h[:2], d[:2])
            if h[0]:
                assert h[2].as_tuples() == d[2].as_tuples()
    pk.free()


@pytest.mark.gpu
def test_device_settle_equals_the_host_settle(ctx):
    """7. on the accepting case, on a changed s and on a changed r1is word"""
    c = case(1024, 1, 27)
    ok, _, cl = hg.verify_public_bn254(c["pk"], c["inst"], c["proof"])
    assert ok
    for w in (c["w"], changed_witness(c, "s"), changed_witness(c, "r1is", 7)):
        host = hg.claims_settle_bn254(None, c["bfv"].params, w, cl)
        assert hg.claims_settle_bn254(ctx, c["bfv"].params, w, cl) == host
    assert host == (False, "input claim mismatch at input 4")
    assert hg.claims_settle_bn254(ctx, c["bfv"].params, c["w"], cl) == (True, "")


@pytest.mark.gpu
def test_neighbours_on_the_context_are_undisturbed(ctx):
    """8. around two public device verifications and settles hg_prove_bn254, hg_verify_device_bn254 and a Goldilocks prove / verify pair
    give what they gave before"""
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x4c4c)
    inst = hg.Instance.from_witness(w)
    first = ctx.prove_bn254(pk, w)[0]
    gl = bfv.prove(ctx, pk, w)[0]
    assert hg.verify_device(ctx, pk, w, gl) == (True, "")
    for i in range(2):
        ok, why, cl = hg.verify_public_bn254(pk, inst, first, ctx=ctx, device=True)
        assert ok, why
        assert hg.claims_settle_bn254(ctx, bfv.params, w, cl) == (True, "")
        assert ctx.prove_bn254(pk, w)[0] == first, i
        assert hg.verify_device_bn254(ctx, pk, w, first) == (True, ""), i
        assert bfv.prove(ctx, pk, w)[0] == gl, i
        assert hg.verify_device(ctx, pk, w, gl) == (True, ""), i
    pk.free()
