"""hg_verify_public_batch_bn254: a run of (instance, proof) pairs over bn256::Fr under one key verified from the ciphertext in device
passes of a group of proofs each (bn254_verify_batch.inc). The single entry is the yardstick: every pair of a batch gets the
decision, the reason, the claims and the points that hg_verify_public_device_bn254 gives it alone. hg_instance_mle_batch_bn254
exposes the batch's kernel (k_bn_vin_dots<true>) as one work unit."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from hglib import hg, ROOT, have_gpu

P = hg.P
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # the order of bn256::Fr
ENTRY, MLE = "hg_verify_public_batch_bn254", "hg_instance_mle_batch_bn254"
CAP = 256
MLE_ARGTYPES = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.c_int, hg.u64p, C.c_size_t, hg.u64p]


def _last():
    return hg.lib().hg_last_error().decode()


def _entry():
    f = getattr(hg.lib(), ENTRY)
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_int),
                  C.c_void_p, C.c_size_t, hg.u64p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    f.restype = C.c_int
    return f


def limbs(vals):
    return hg.Context._fr_pack(vals)


class Raw:
    """one raw call with every output prefilled with a pattern; `drop` names arguments passed as NULL"""

    def __init__(self, ctx_h, pk, insts, proofs, n=None, drop=(), caps=None, null_pk=False):
        nc, nco = hg.pk_claim_shape(pk)
        self.nc, self.nco = caps or (nc, nco)
        n = len(proofs) if n is None else n
        m = max(n, len(proofs), 1)
        I = (C.c_void_p * m)(*insts)
        Pf = (C.c_char_p * m)(*proofs)
        N = (C.c_size_t * m)(*[len(p) if p else 0 for p in proofs])
        self.res = (C.c_int * m)(*([7] * m))
        self.claims = (C.c_uint8 * (48 * m * max(nc, 1)))(*([0x55] * (48 * m * max(nc, 1))))
        self.points = np.full(4 * m * max(nco, 1), 0x5555, dtype=np.uint64)
        self.counts = (C.c_size_t * m)(*([9] * m))
        self.reasons = C.create_string_buffer(b"\x55" * (m * CAP), m * CAP)
        a = dict(instances=I, proofs=Pf, lens=N, results=self.res, claims=self.claims, points=hg._ptr(self.points), n_claims=self.counts, reasons=self.reasons)
        for d in drop:
            a[d] = None
        self.rc = _entry()(ctx_h, None if null_pk else pk.h, a["instances"], a["proofs"], a["lens"], n, a["results"], a["claims"], self.nc,
                           a["points"], self.nco, a["n_claims"], a["reasons"], CAP)
        self.m = m

    def untouched(self):
        return (list(self.res) == [7] * self.m and list(self.counts) == [9] * self.m and self.reasons.raw == b"\x55" * (self.m * CAP)
                and bytes(self.claims) == b"\x55" * len(self.claims) and (self.points == 0x5555).all())


# ---- Python-integer arithmetic mod r ---------------------------------------------------------------------------------------------
def fr_of(word):
    """a table word (small signed integer in the Goldilocks form: z < 0 as p - |z|) as an element of Fr"""
    w = int(word)
    return w if w < P // 2 else (w - P) % R


def py_mle(table, pt):
    """the MLE of a laid-out table at pt, x_0 the lowest bit of the index"""
    eq = [1]
    for r in pt:
        hi = [v * r % R for v in eq]
        eq = [(v - h) % R for v, h in zip(eq, hi)] + hi
    assert len(eq) == len(table)
    return sum(fr_of(v) * e for v, e in zip(table, eq) if int(v)) % R


def unit_point(index, nvars):
    return [(index >> b) & 1 for b in range(nvars)]


def points(nvars, seed):
    """two random Fr points, the all-zero point and the all-ones point"""
    rng = random.Random(seed)
    return [[rng.randrange(R) for _ in range(nvars)] for _ in range(2)] + [[0] * nvars, [1] * nvars]


def unit_words(which, n, k):
    """(word of the laid-out table, index into the member's k*n coefficients of that table or None for a padding word): words lo and
    lo + n-1 of the first and the last block, and one padding word. Word lo + r of block b holds coefficient n-1-r of block b."""
    if which == 0:
        return [(0, n - 1), (n - 1, 0), (n, None)]
    out = []
    for b in sorted({0, k - 1}):
        out += [(b * 2 * n + n - 1, b * n + n - 1), (b * 2 * n + 2 * n - 2, b * n)]
    return out + [((k - 1) * 2 * n + 2 * n - 1, None)]


def derived_params():
    """(1024,2) with the moduli of the built-in (4096,2) set: ct0is is ONE 2048-word tile that holds both coefficient blocks"""
    return hg.params_derive(1024, 2, [int(q) for q in hg.params_builtin(4096, 2).qis[:2]])


_MEMBERS = {}
FIXTURE_BITS = {(1024, 1): 27, (4096, 2): 55}


def members(key):
    """six per shape: the fixture's instance where one exists (else a second synthetic witness's), a synthetic witness's, +(q_i-1)/2
    everywhere, -(q_i-1)/2 everywhere, alternating signs, all-zero. key: (n, k) of a built-in set, or "derived"."""
    if key not in _MEMBERS:
        params = derived_params() if key == "derived" else hg.params_builtin(*key)
        n, k = int(params.n), int(params.k)
        q = [int(x) for x in params.qis[:k]]
        half = np.concatenate([np.full(n, (q[i] - 1) // 2) for i in range(k)]).astype(np.int64)
        alt = half * np.where(np.arange(k * n) % 2 == 0, 1, -1)
        zero = np.zeros(k * n, dtype=np.int64)
        if key in FIXTURE_BITS:
            first = hg.Witness.from_json(params, os.path.join(ROOT, "tests", "golden", f"sk_enc_{n}_{k}x{FIXTURE_BITS[key]}_65537.json"))
        else:
            first = hg.Witness.synthetic(params, 0x52 + n)
        out = [hg.Instance.from_witness(first), hg.Instance.from_witness(hg.Witness.synthetic(params, 0x51 + n))]
        out += [hg.Instance.from_ciphertext(params, a, c) for a, c in ((half, half), (-half, -half), (alt, -alt), (zero, zero))]
        _MEMBERS[key] = (params, out)
    return _MEMBERS[key]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    """1."""
    raw = open(os.path.join(ROOT, "include", "hg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)

    def pattern(sig):
        sig = sig.split()
        return "".join(re.escape(t) + (r"\s+" if u and t[-1].isalnum() and (u[0].isalnum() or u[0] == "_") else r"\s*") for t, u in zip(sig, sig[1:] + [""]))
    assert re.search(pattern("int hg_verify_public_batch_bn254 ( hg_ctx * ctx , const hg_pk * pk , const void * const * instances , const uint8_t * const * proofs , "
                             "const size_t * lens , size_t n , int * results , void * claims , size_t claim_cap_each , uint64_t * points4 , "
                             "size_t coord_cap_each , size_t * n_claims , char * reasons , size_t reason_cap ) ;"), hdr)
    assert re.search(pattern("int hg_instance_mle_batch_bn254 ( hg_ctx * ctx , const void * const * instances , size_t n , int which , int index , "
                             "const uint64_t * point4 , size_t nvars , uint64_t * out4 ) ;"), hdr)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in (ENTRY, MLE):
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    opt = re.search(r'"verify_batch_group"(.*?)Returns 0', raw, flags=re.S)
    assert opt and re.search(r"\b%s\b" % ENTRY, opt.group(1))
    assert "there is no batched form" not in raw


def test_bad_arguments_are_errors_naming_the_function():
    """2."""
    bfv = hg.BfvEncrypt.new(1024, 1)
    host_pk = bfv.setup(None)
    w = hg.Witness.synthetic(bfv.params, 21)
    inst = hg.Instance.from_witness(w)
    other = hg.Instance.from_witness(hg.Witness.synthetic(hg.params_builtin(2048, 1), 5))
    proof = bytes(32 * 64)
    ih, oh = inst.h.value, other.h.value
    nc, nco = hg.pk_claim_shape(host_pk)
    out = np.full(8, 0x5555, dtype=np.uint64)
    pt = limbs([3] * 11)
    f = getattr(hg.lib(), MLE)
    f.argtypes = MLE_ARGTYPES

    def is_error(r, what, word=None):
        assert r.rc == -1 and _last().startswith(ENTRY) and r.untouched(), (what, r.rc, _last())
        assert word is None or word in _last(), (what, _last())

    def every_case(ctx_h, pk, device):
        """device: a device context with a device key, so that each case is wrong in one thing only"""
        is_error(Raw(ctx_h, pk, [ih], [proof]), "context or key") if not device else None
        for d in ("instances", "proofs", "lens", "results", "n_claims", "claims", "points"):
            is_error(Raw(ctx_h, pk, [ih], [proof], drop=(d,)), "null " + d)
        is_error(Raw(ctx_h, pk, [ih], [proof], null_pk=True), "null key")
        is_error(Raw(ctx_h, pk, [ih, None], [proof, proof]), "null instance", "index 1" if device else None)
        is_error(Raw(ctx_h, pk, [ih, ih], [proof, None]), "null proof", "index 1" if device else None)
        is_error(Raw(ctx_h, pk, [ih], [proof], caps=(nc - 1, nco)), "claim cap", "hg_pk_claim_shape" if device else None)
        is_error(Raw(ctx_h, pk, [ih], [proof], caps=(nc, nco - 1)), "coordinate cap", "hg_pk_claim_shape" if device else None)
        is_error(Raw(ctx_h, pk, [ih, oh, ih], [proof] * 3), "an instance of (2048,1) among (1024,1)", "index 1" if device else None)
        hs = (C.c_void_p * 2)(ih, oh)
        one = (C.c_void_p * 1)(ih)
        bad = [(None, 1, 0, 0, hg._ptr(pt), 11, hg._ptr(out)), (hs, 1, 0, 0, None, 11, hg._ptr(out)), (hs, 1, 0, 0, hg._ptr(pt), 11, None),
               (hs, 2, 0, 0, hg._ptr(pt), 11, hg._ptr(out)), ((C.c_void_p * 2)(ih, None), 2, 0, 0, hg._ptr(pt), 11, hg._ptr(out)),
               (one, 1, 2, 0, hg._ptr(pt), 11, hg._ptr(out)), (one, 1, 0, 1, hg._ptr(pt), 11, hg._ptr(out)), (one, 1, 0, 0, hg._ptr(pt), 10, hg._ptr(out)),
               (one, 1, 0, 0, hg._ptr(limbs([1] * 10 + [R])), 11, hg._ptr(out))]
        for args in bad:
            assert f(ctx_h, *args) == -1 and _last().startswith(MLE), (args[1:4], _last())
            assert (out == 0x5555).all()

    every_case(None, host_pk, False)                      # no context
    with pytest.raises(hg.HgError, match=ENTRY):
        hg.verify_public_batch_bn254(None, host_pk, [inst], [proof])
    with pytest.raises(hg.HgError, match=MLE):
        hg.instance_mle_batch_bn254(None, [inst], 0, 0, [3] * 11)
    if have_gpu():
        ctx = hg.Context(0)
        try:
            every_case(ctx.h, host_pk, False)             # a device context with a host-only key
            with pytest.raises(hg.HgError, match=ENTRY):
                hg.verify_public_batch_bn254(ctx, host_pk, [inst], [proof])
            pk = bfv.setup(ctx)
            try:
                every_case(ctx.h, pk, True)
            finally:
                pk.free()
        finally:
            ctx.close()
    host_pk.free()


def test_the_derived_shape_works_on_the_host():
    """the (1024,2) set of the kernel test: derivation, instances and the host MLE over Fr agree with Python integers"""
    params, all_ = members("derived")
    n, k, nv = 1024, 2, 12
    assert (int(params.n), int(params.k)) == (n, k)
    rng = random.Random(77)
    pt = [rng.randrange(R) for _ in range(nv)]
    for m in all_[:3]:
        table = m.table(1)
        assert len(table) == 1 << nv
        assert m.mle_bn254(None, 1, 0, pt) == py_mle(table, pt)
        _, ct0 = m.coeffs()
        for word, ci in unit_words(1, n, k):
            want = 0 if ci is None else int(ct0[ci]) % R
            assert fr_of(table[word]) == want and m.mle_bn254(None, 1, 0, unit_point(word, nv)) == want, word


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key,which,index", [((1024, 1), 0, 0), ((1024, 1), 1, 0), ("derived", 1, 0), ((4096, 2), 0, 1), ((4096, 2), 1, 0)])
def test_batch_kernel_parity_with_the_host_form_and_hg_mle_eval_bn254(ctx, key, which, index):
    """3. one unit of k_bn_vin_dots<true> with P members: half a tile (1024 words) and lo = n-1; one 2048-word tile that holds both
    blocks of the derived (1024,2) set, the block boundary inside a thread's items; two and four tiles at (4096,2)"""
    params, all_ = members(key)
    n, k = int(params.n), int(params.k)
    nv = n.bit_length() + (k.bit_length() - 1 if which else 0)
    coeffs = [m.coeffs()[which] for m in all_]
    base = 0 if which else index * n                      # (the member's coefficients of this table start here)
    t = all_[1].table(which)                              # one member against hg_mle_eval_bn254: its laid-out table, lifted once
    lifted = limbs([fr_of(v) for v in (t if which else t[index * 2 * n:(index + 1) * 2 * n])])
    pts = [(pt, False, None) for pt in points(nv, 400 + nv + which)] + [(unit_point(word, nv), True, ci) for word, ci in unit_words(which, n, k)]
    for pi, (pt, unit, ci) in enumerate(pts):
        want = [m.mle_bn254(None, which, index, pt) for m in all_]
        if unit:                                          # a padding word gives 0, any other word that member's lifted coefficient
            assert want == [0 if ci is None else int(c[base + ci]) % R for c in coeffs], pi
        out = np.zeros(4, dtype=np.uint64)
        assert hg.lib().hg_mle_eval_bn254(ctx.h, hg._ptr(lifted), nv, hg._ptr(limbs(pt)), hg._ptr(out)) == 0, _last()
        assert hg.Context._fr_unpack(out)[0] == want[1], pi
        for sel in ([pi % 6], [2, 5], [0, 2, 3, 4, 1], list(range(6))):   # P = 1, 2, 5 (permuted), 6: the prefetch, and the last member issuing none
            got = hg.instance_mle_batch_bn254(ctx, [all_[j] for j in sel], which, index, pt)
            assert got == [want[j] for j in sel], (pi, sel)


def single(ctx, pk, inst, proof):
    ok, why, cl = hg.verify_public_bn254(pk, inst, proof, ctx=ctx, device=True)
    return ok, why, (cl.as_tuples() if ok else None)


def batch(ctx, pk, insts, proofs):
    got = hg.verify_public_batch_bn254(ctx, pk, insts, proofs)
    assert len(got) == len(proofs)
    return got, [(ok, why, (cl.as_tuples() if ok else None)) for ok, why, cl in got]


def batch_equals_singles(ctx, pk, insts, proofs, host=False):
    got, flat_ = batch(ctx, pk, insts, proofs)
    for i, (inst, p) in enumerate(zip(insts, proofs)):
        want = single(ctx, pk, inst, p)
        assert flat_[i] == want, (i, flat_[i][:2], want[:2])
        if host:
            ok, why, cl = hg.verify_public_bn254(pk, inst, p)
            assert (ok, why, cl.as_tuples() if ok else None) == want, i
    return got


def tampered(proof):
    """bit-flipped copies at fixed offsets, half the bytes, all but the last 32"""
    L = len(proof)
    out = []
    for pos, bit in ((0, 1), (L // 7, 4), (L // 3, 0x20), (2 * L // 3, 2), (L - 9, 0x80)):
        bad = bytearray(proof)
        bad[pos] ^= bit
        out.append(bytes(bad))
    return out + [proof[:L // 2], proof[:-32]]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
def test_batch_equals_singles(ctx, n, k):
    """4."""
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xb54 + 16 * n + i) for i in range(2)]
    inst = [hg.Instance.from_witness(w) for w in ws]
    honest = [ctx.prove_bn254(pk, w)[0] for w in ws]
    bad = tampered(honest[0])
    proofs = [honest[0]] + bad[:3] + [honest[1]] + bad[3:]
    insts = [inst[0]] * 4 + [inst[1]] + [inst[0]] * (len(bad) - 3)
    wits = [ws[0]] * 4 + [ws[1]] + [ws[0]] * (len(bad) - 3)
    got = batch_equals_singles(ctx, pk, insts, proofs, host=True)
    assert got[0][0] and got[4][0], (got[0][1], got[4][1])
    assert not got[len(proofs) - 2][0]   # (half the bytes)
    for g, w in zip(got, wits):
        if g[0]:
            assert hg.claims_settle_bn254(ctx, bfv.params, w, g[2]) == (True, "")
    pk.free()


@pytest.mark.gpu
def test_no_cross_wiring_between_the_pairs_of_a_batch(ctx):
    """5. the group shares every eq table among its members: a member's coefficients must never meet another member's slot"""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xc54 + i) for i in range(4)]
    inst = [hg.Instance.from_witness(w) for w in ws]
    ps = [ctx.prove_bn254(pk, w)[0] for w in ws]
    insts = [inst[(i + 1) % 4] for i in range(4)] + inst + [inst[2], inst[2]]
    proofs = ps + ps + [ps[2], ps[2]]
    got = batch_equals_singles(ctx, pk, insts, proofs)
    for i in range(4):
        assert not got[i][0] and got[i][1], i
        assert got[4 + i][0], (i, got[4 + i][1])
        assert hg.claims_settle_bn254(ctx, bfv.params, ws[i], got[4 + i][2]) == (True, "")
        assert not hg.claims_settle_bn254(ctx, bfv.params, ws[(i + 1) % 4], got[4 + i][2])[0]
    assert got[8][0] and got[9][0] and got[8][2].as_tuples() == got[9][2].as_tuples() == got[6][2].as_tuples()
    pk.free()


@pytest.mark.gpu
def test_a_changed_coefficient_hits_only_its_member(ctx):
    """6. one ct0 coefficient, one a coefficient of the last modulus"""
    n, k = 4096, 2
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0xf54)
    inst = hg.Instance.from_witness(w)
    proof = ctx.prove_bn254(pk, w)[0]
    a, ct0 = inst.coeffs()
    changed = []
    for tab, j in ((1, 3), (0, k * n - 2)):
        arrs = [a.copy(), ct0.copy()]
        arrs[tab][j] += 1
        changed.append(hg.Instance.from_ciphertext(bfv.params, *arrs))
    insts = [inst, changed[0], inst, changed[1], inst]
    got = batch_equals_singles(ctx, pk, insts, [proof] * 5)
    assert [g[0] for g in got] == [True, False, True, False, True], [g[1] for g in got]
    alone = single(ctx, pk, inst, proof)
    for i in (0, 2, 4):
        assert got[i][2].as_tuples() == alone[2]
    pk.free()


@pytest.mark.gpu
def test_group_boundaries_do_not_change_the_results(ctx):
    """7."""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xd54 + i) for i in range(8)]
    insts = [hg.Instance.from_witness(w) for w in ws]
    ps = [ctx.prove_bn254(pk, w)[0] for w in ws]
    ps[0] = ps[0][:len(ps[0]) // 2]
    insts[6] = insts[5]                      # (a mismatched pair in the last group of three)
    _, one = batch(ctx, pk, insts, ps)
    try:
        ctx.set_option("verify_batch_group", 3)
        _, three = batch(ctx, pk, insts, ps)
    finally:
        ctx.set_option("verify_batch_group", 0)
    assert three == one
    assert [r[0] for r in one] == [False, True, True, True, True, True, False, True], [r[1] for r in one]
    for i, (inst, p) in enumerate(zip(insts, ps)):
        assert one[i] == single(ctx, pk, inst, p), i
    pk.free()


@pytest.mark.gpu
def test_the_context_stays_usable(ctx):
    """8. BN254 proves, the BN254 device verifiers, the Goldilocks public batch and resident Goldilocks proves (the later ones replays
    of the recorded launch graph) give around two batches what they gave before"""
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0xe54)
    inst = hg.Instance.from_witness(w)
    vals = hg.witness_gen(ctx, pk, w)
    out = hg.ProofBuffer()
    first = [hg.prove_resident(ctx, pk, vals, out).bytes() for _ in range(3)]
    assert first[0] == first[1] == first[2]
    pb = ctx.prove_bn254(pk, w)[0]
    before = single(ctx, pk, inst, pb)
    assert before[0], before[1]
    gl_before = hg.verify_public_batch(ctx, pk, [inst, inst], [first[0], first[0][:-16]], 0)
    gl_before = [(ok, why, cl.as_tuples() if ok else None) for ok, why, cl in gl_before]
    assert gl_before[0][0]
    for i in range(2):
        _, got = batch(ctx, pk, [inst, inst], [pb, pb[:-32]])
        assert got[0] == before and got[1] == single(ctx, pk, inst, pb[:-32])
        assert ctx.prove_bn254(pk, w)[0] == pb, i
        assert hg.verify_device_bn254(ctx, pk, w, pb) == (True, ""), i
        assert hg.verify_device_batch_bn254(ctx, pk, [w, w], [pb, pb[:len(pb) // 2]])[0] == (True, ""), i
        gl = hg.verify_public_batch(ctx, pk, [inst, inst], [first[0], first[0][:-16]], 0)
        assert [(ok, why, cl.as_tuples() if ok else None) for ok, why, cl in gl] == gl_before, i
        assert hg.prove_resident(ctx, pk, vals, out).bytes() == first[0], i
    vals.free()
    pk.free()


@pytest.mark.gpu
def test_an_empty_batch_returns_0_and_writes_nothing(ctx):
    """9."""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    r = Raw(ctx.h, pk, [], [], n=0)
    assert r.rc == 0 and r.untouched()
    assert hg.verify_public_batch_bn254(ctx, pk, [], []) == []
    pk.free()


@pytest.mark.gpu
def test_headline_size_batch_of_four(ctx):
    """10. (32768,16): one bit-flipped proof, one instance with a changed ct0 coefficient in modulus 11"""
    n, k = 32768, 16
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0x8054 + i) for i in range(4)]
    insts = [hg.Instance.from_witness(w) for w in ws]
    ps = [ctx.prove_bn254(pk, w, cap=1 << 25)[0] for w in ws]
    bad = bytearray(ps[1])
    bad[len(bad) // 3] ^= 4
    ps[1] = bytes(bad)
    a, ct0 = insts[2].coeffs()
    ct0[11 * n + 12345] += 1
    insts[2] = hg.Instance.from_ciphertext(bfv.params, a, ct0)
    got = batch_equals_singles(ctx, pk, insts, ps)
    assert got[0][0] and got[3][0] and not got[2][0], [g[1] for g in got]   # (proof 1: as the single call decides)
    for i in (0, 3):
        assert hg.claims_settle_bn254(ctx, bfv.params, ws[i], got[i][2]) == (True, "")
    pk.free()
