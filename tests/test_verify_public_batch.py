"""hg_verify_public_batch: a run of (instance, proof) pairs under one key verified from the ciphertext in device passes of a group of
proofs each (verifier_batch.hip). The single entry is the yardstick: every pair of a batch gets the decision, the reason, the
claims and the points that hg_verify_public_device gives it alone. hg_instance_mle_batch exposes the batch's kernel."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from hglib import hg, ROOT, have_gpu

P = hg.P
ENTRY, MLE = "hg_verify_public_batch", "hg_instance_mle_batch"
CAP = 256


def _last():
    return hg.lib().hg_last_error().decode()


def _entry():
    f = getattr(hg.lib(), ENTRY)
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int, C.POINTER(C.c_int),
                  C.c_void_p, C.c_size_t, hg.u64p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    f.restype = C.c_int
    return f


class Raw:
    """one raw call with every output prefilled with a pattern; `drop` names arguments passed as NULL"""

    def __init__(self, ctx_h, pk, insts, proofs, mode, n=None, drop=(), caps=None, null_pk=False):
        nc, nco = hg.pk_claim_shape(pk)
        self.nc, self.nco = caps or (nc, nco)
        n = len(proofs) if n is None else n
        m = max(n, len(proofs), 1)
        I = (C.c_void_p * m)(*insts)
        Pf = (C.c_char_p * m)(*proofs)
        N = (C.c_size_t * m)(*[len(p) if p else 0 for p in proofs])
        self.res = (C.c_int * m)(*([7] * m))
        self.claims = (C.c_uint8 * (32 * m * max(nc, 1)))(*([0x55] * (32 * m * max(nc, 1))))
        self.points = np.full(2 * m * max(nco, 1), 0x5555, dtype=np.uint64)
        self.counts = (C.c_size_t * m)(*([9] * m))
        self.reasons = C.create_string_buffer(b"\x55" * (m * CAP), m * CAP)
        a = dict(instances=I, proofs=Pf, lens=N, results=self.res, claims=self.claims, points=hg._ptr(self.points), n_claims=self.counts, reasons=self.reasons)
        for d in drop:
            a[d] = None
        self.rc = _entry()(ctx_h, None if null_pk else pk.h, a["instances"], a["proofs"], a["lens"], n, mode, a["results"], a["claims"], self.nc,
                           a["points"], self.nco, a["n_claims"], a["reasons"], CAP)
        self.m = m

    def untouched(self):
        return (list(self.res) == [7] * self.m and list(self.counts) == [9] * self.m and self.reasons.raw == b"\x55" * (self.m * CAP)
                and bytes(self.claims) == b"\x55" * len(self.claims) and (self.points == 0x5555).all())


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    sig = ("int hg_verify_public_batch ( hg_ctx * ctx , const hg_pk * pk , const void * const * instances , const uint8_t * const * proofs , "
           "const size_t * lens , size_t n , int mode , int * results , void * claims , size_t claim_cap_each , uint64_t * points , "
           "size_t coord_cap_each , size_t * n_claims , char * reasons , size_t reason_cap ) ;").split()
    pat = "".join(re.escape(t) + (r"\s+" if u and t[-1].isalnum() and (u[0].isalnum() or u[0] == "_") else r"\s*") for t, u in zip(sig, sig[1:] + [""]))
    assert re.search(pat, hdr)
    assert re.search(r"int\s+hg_instance_mle_batch\s*\(\s*hg_ctx\s*\*\s*ctx\s*,\s*const\s+void\s*\*\s*const\s*\*\s*instances\s*,\s*size_t\s+n\s*,\s*int\s+which\s*,"
                     r"\s*int\s+index\s*,\s*const\s+uint64_t\s*\*\s*point\s*,\s*size_t\s+nvars\s*,\s*uint64_t\s*\*\s*out\s*\)\s*;", hdr)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in (ENTRY, MLE):
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    opt = re.search(r'"verify_batch_group"(.*?)Returns 0', open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    assert opt and ENTRY in opt.group(1)


def test_bad_arguments_are_errors_naming_the_function():
    bfv = hg.BfvEncrypt.new(1024, 1)
    host_pk = bfv.setup(None)
    w = hg.Witness.synthetic(bfv.params, 21)
    inst = hg.Instance.from_witness(w)
    other = hg.Instance.from_witness(hg.Witness.synthetic(hg.params_builtin(2048, 1), 5))
    proof = bytes(16 * 64)
    ih, oh = inst.h.value, other.h.value
    nc, nco = hg.pk_claim_shape(host_pk)
    out = np.zeros(4, dtype=np.uint64)
    pt = np.zeros(22, dtype=np.uint64)
    f = getattr(hg.lib(), MLE)
    f.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.c_int, hg.u64p, C.c_size_t, hg.u64p]

    def is_error(r, what, word=None):
        assert r.rc == -1 and ENTRY in _last() and r.untouched(), (what, r.rc, _last())
        assert word is None or word in _last(), (what, _last())

    def every_case(ctx_h, pk, device):
        """device: a device context with a device key, so that each case is wrong in one thing only"""
        is_error(Raw(ctx_h, pk, [ih], [proof], 0), "context or key") if not device else None
        for d in ("instances", "proofs", "lens", "results", "n_claims", "claims", "points"):
            is_error(Raw(ctx_h, pk, [ih], [proof], 0, drop=(d,)), "null " + d)
        is_error(Raw(ctx_h, pk, [ih], [proof], 0, null_pk=True), "null key")
        is_error(Raw(ctx_h, pk, [ih, None], [proof, proof], 0), "null instance", "index 1" if device else None)
        is_error(Raw(ctx_h, pk, [ih, ih], [proof, None], 0), "null proof", "index 1" if device else None)
        for mode in (-1, 4):
            is_error(Raw(ctx_h, pk, [ih], [proof], mode), "mode", "mode" if device else None)
        is_error(Raw(ctx_h, pk, [ih], [proof], 0, caps=(nc - 1, nco)), "claim cap", "hg_pk_claim_shape" if device else None)
        is_error(Raw(ctx_h, pk, [ih], [proof], 0, caps=(nc, nco - 1)), "coordinate cap", "hg_pk_claim_shape" if device else None)
        is_error(Raw(ctx_h, pk, [ih, oh, ih], [proof] * 3, 0), "an instance of (2048,1) among (1024,1)", "index 1" if device else None)
        hs = (C.c_void_p * 2)(ih, oh)
        for args in ((None, 1, 0, 0, hg._ptr(pt), 11, hg._ptr(out)), (hs, 1, 0, 0, None, 11, hg._ptr(out)), (hs, 1, 0, 0, hg._ptr(pt), 11, None),
                     (hs, 2, 0, 0, hg._ptr(pt), 11, hg._ptr(out)), ((C.c_void_p * 2)(ih, None), 2, 0, 0, hg._ptr(pt), 11, hg._ptr(out))):
            assert f(ctx_h, *args) == -1 and MLE in _last(), args[1:4]

    every_case(None, host_pk, False)                      # no context
    for mode in (0, 3):
        with pytest.raises(hg.HgError, match=ENTRY):
            hg.verify_public_batch(None, host_pk, [inst], [proof], mode)
    with pytest.raises(hg.HgError, match=MLE):
        hg.instance_mle_batch(None, [inst], 0, 0, pt)
    if have_gpu():
        ctx = hg.Context(0)
        try:
            every_case(ctx.h, host_pk, False)             # a device context with a host-only key
            pk = bfv.setup(ctx)
            try:
                every_case(ctx.h, pk, True)
            finally:
                pk.free()
        finally:
            ctx.close()
    host_pk.free()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def points(nvars, seed):
    """two random E points, the all-zero point and the all-ones point"""
    rng = random.Random(seed)
    rnd = [[(rng.randrange(P), rng.randrange(P)) for _ in range(nvars)] for _ in range(2)]
    return rnd + [[(0, 0)] * nvars, [(1, 0)] * nvars]


def flat(pt):
    return np.array([c for x in pt for c in x], dtype=np.uint64)


_MEMBERS = {}


def members(n, k):
    """the fixture's instance and a synthetic witness's, +(q_i-1)/2 everywhere, -(q_i-1)/2 everywhere, alternating signs, all-zero"""
    if (n, k) not in _MEMBERS:
        bfv = hg.BfvEncrypt.new(n, k)
        q = [int(x) for x in bfv.params.qis[:k]]
        half = np.concatenate([np.full(n, (q[i] - 1) // 2) for i in range(k)]).astype(np.int64)
        alt = half * np.where(np.arange(k * n) % 2 == 0, 1, -1)
        zero = np.zeros(k * n, dtype=np.int64)
        bits = {(1024, 1): 27, (4096, 2): 55}[(n, k)]
        fixture = bfv.get_inputs(os.path.join(ROOT, "tests", "golden", f"sk_enc_{n}_{k}x{bits}_65537.json"))
        out = [hg.Instance.from_witness(fixture), hg.Instance.from_witness(hg.Witness.synthetic(bfv.params, 0x51 + n))]
        out += [hg.Instance.from_ciphertext(bfv.params, a, c) for a, c in ((half, half), (-half, -half), (alt, -alt), (zero, zero))]
        _MEMBERS[(n, k)] = out
    return _MEMBERS[(n, k)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,which,index", [(1024, 1, 0, 0), (1024, 1, 1, 0), (4096, 2, 0, 1), (4096, 2, 1, 0)])
def test_batch_kernel_parity_with_the_host_form_and_hg_mle_eval(ctx, n, k, which, index):
    """3. one unit of k_vin_dots<true> with P members: half a tile (1024 words), lo = n-1, two coefficient blocks over four tiles"""
    all_ = members(n, k)
    nv = n.bit_length() + (k.bit_length() - 1 if which else 0)
    tables = [(m.table(1) if which else m.table(0)[index * 2 * n:(index + 1) * 2 * n]) for m in all_]
    for pi, pt in enumerate(points(nv, 300 + nv + which)):
        f = flat(pt)
        want = [m.mle(None, which, index, f) for m in all_]
        for j, t in enumerate(tables):
            assert (ctx.mle_eval(t, f) == want[j]).all(), (pi, j)
        for sel in ([pi % 6], [2, 5], [0, 2, 3, 4, 1], list(range(6))):   # P = 1, 2, 5 (odd: both LDS buffers and back), 6
            got = hg.instance_mle_batch(ctx, [all_[j] for j in sel], which, index, f)
            assert got.shape == (len(sel), 2)
            for r, j in enumerate(sel):
                assert (got[r] == want[j]).all(), (pi, sel, j)


def single(ctx, pk, inst, proof, mode):
    ok, why, cl = hg.verify_public(pk, inst, proof, mode, ctx=ctx, device=True)
    return ok, why, (cl.as_tuples() if ok else None)


def batch(ctx, pk, insts, proofs, mode):
    got = hg.verify_public_batch(ctx, pk, insts, proofs, mode)
    assert len(got) == len(proofs)
    return got, [(ok, why, (cl.as_tuples() if ok else None)) for ok, why, cl in got]


def batch_equals_singles(ctx, pk, insts, proofs, mode, host=False):
    got, flat_ = batch(ctx, pk, insts, proofs, mode)
    for i, (inst, p) in enumerate(zip(insts, proofs)):
        want = single(ctx, pk, inst, p, mode)
        assert flat_[i] == want, (mode, i, flat_[i][:2], want[:2])
        if host:
            ok, why, cl = hg.verify_public(pk, inst, p, mode)
            assert (ok, why, cl.as_tuples() if ok else None) == want, (mode, i)
    return got


def tampered(proof):
    """bit-flipped copies at fixed offsets, half the bytes, all but the last 16"""
    L = len(proof)
    out = []
    for pos, bit in ((0, 1), (L // 7, 4), (L // 3, 0x20), (2 * L // 3, 2), (L - 9, 0x80)):
        bad = bytearray(proof)
        bad[pos] ^= bit
        out.append(bytes(bad))
    return out + [proof[:L // 2], proof[:-16]]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_batch_equals_singles(ctx, n, k, mode):
    """4."""
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xb40 + 16 * n + 4 * mode + i) for i in range(2)]
    inst = [hg.Instance.from_witness(w) for w in ws]
    honest = [bfv.prove(ctx, pk, w, mode=mode)[0] for w in ws]
    bad = tampered(honest[0])
    proofs = [honest[0]] + bad[:3] + [honest[1]] + bad[3:]
    insts = [inst[0]] * 4 + [inst[1]] + [inst[0]] * (len(bad) - 3)
    wits = [ws[0]] * 4 + [ws[1]] + [ws[0]] * (len(bad) - 3)
    got = batch_equals_singles(ctx, pk, insts, proofs, mode, host=True)
    assert got[0][0] and got[4][0], (got[0][1], got[4][1])
    assert sum(not g[0] for g in got) >= 1 and not got[len(proofs) - 2][0]   # (half the bytes)
    for g, w in zip(got, wits):
        if g[0]:
            assert hg.claims_settle(ctx, bfv.params, w, g[2]) == (True, "")
    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_no_cross_wiring_between_the_pairs_of_a_batch(ctx, mode):
    """5. mode 0 shares every eq table among the group's members: a member's coefficients must never be"""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xc40 + 8 * mode + i) for i in range(4)]
    inst = [hg.Instance.from_witness(w) for w in ws]
    ps = [bfv.prove(ctx, pk, w, mode=mode)[0] for w in ws]
    insts = [inst[(i + 1) % 4] for i in range(4)] + inst + [inst[2], inst[2]]
    proofs = ps + ps + [ps[2], ps[2]]
    got = batch_equals_singles(ctx, pk, insts, proofs, mode)
    for i in range(4):
        assert not got[i][0] and got[i][1], i
        assert got[4 + i][0], (i, got[4 + i][1])
        assert hg.claims_settle(ctx, bfv.params, ws[i], got[4 + i][2]) == (True, "")
        assert not hg.claims_settle(ctx, bfv.params, ws[(i + 1) % 4], got[4 + i][2])[0]
    assert got[8][0] and got[9][0] and got[8][2].as_tuples() == got[9][2].as_tuples() == got[6][2].as_tuples()
    pk.free()


@pytest.mark.gpu
def test_a_changed_coefficient_hits_only_its_member(ctx):
    """6."""
    n, k, mode = 4096, 2, 3
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0xf40)
    inst = hg.Instance.from_witness(w)
    proof = bfv.prove(ctx, pk, w, mode=mode)[0]
    a, ct0 = inst.coeffs()
    changed = []
    for tab, j in ((1, 3), (0, k * n - 2)):
        arrs = [a.copy(), ct0.copy()]
        arrs[tab][j] += 1
        changed.append(hg.Instance.from_ciphertext(bfv.params, *arrs))
    insts = [inst, changed[0], inst, changed[1], inst]
    got = batch_equals_singles(ctx, pk, insts, [proof] * 5, mode)
    assert [g[0] for g in got] == [True, False, True, False, True], [g[1] for g in got]
    alone = single(ctx, pk, inst, proof, mode)
    for i in (0, 2, 4):
        assert got[i][2].as_tuples() == alone[2]
    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_group_boundaries_do_not_change_the_results(ctx, mode):
    """7."""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0xd40 + 8 * mode + i) for i in range(8)]
    insts = [hg.Instance.from_witness(w) for w in ws]
    ps = [bfv.prove(ctx, pk, w, mode=mode)[0] for w in ws]
    ps[0] = ps[0][:len(ps[0]) // 2]
    insts[6] = insts[5]                      # (a mismatched pair in the last group of three)
    _, one = batch(ctx, pk, insts, ps, mode)
    try:
        ctx.set_option("verify_batch_group", 3)
        _, three = batch(ctx, pk, insts, ps, mode)
    finally:
        ctx.set_option("verify_batch_group", 0)
    assert three == one
    assert [r[0] for r in one] == [False, True, True, True, True, True, False, True], [r[1] for r in one]
    for i, (inst, p) in enumerate(zip(insts, ps)):
        assert one[i] == single(ctx, pk, inst, p, mode), i
    pk.free()


@pytest.mark.gpu
def test_the_context_stays_usable(ctx):
    """8. resident proves around the batches (the later ones replays of the recorded launch graph) stay byte-identical, and the
    other device verifiers give what they gave before"""
    bfv = hg.BfvEncrypt.new(4096, 2)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0xe40)
    inst = hg.Instance.from_witness(w)
    vals = hg.witness_gen(ctx, pk, w)
    out = hg.ProofBuffer()
    first = [hg.prove_resident(ctx, pk, vals, out).bytes() for _ in range(3)]
    assert first[0] == first[1] == first[2]
    p3 = bfv.prove(ctx, pk, w, mode=3)[0]
    before = {m: single(ctx, pk, inst, p, m) for m, p in ((0, first[0]), (3, p3))}
    assert before[0][0] and before[3][0]
    for mode, p in ((0, first[0]), (3, p3)):
        _, got = batch(ctx, pk, [inst, inst], [p, p[:-16]], mode)
        assert got[0] == before[mode]
        assert hg.prove_resident(ctx, pk, vals, out).bytes() == first[0], mode
        assert hg.verify_device(ctx, pk, w, first[0]) == (True, "")
        assert hg.verify_device(ctx, pk, w, p3, mode=3) == (True, "")
        assert single(ctx, pk, inst, p, mode) == before[mode]
        assert hg.verify_device_batch(ctx, pk, [w, w], [p, p[:len(p) // 2]], mode=mode)[0] == (True, "")
        assert hg.prove_resident(ctx, pk, vals, out).bytes() == first[0], mode
    vals.free()
    pk.free()


@pytest.mark.gpu
def test_an_empty_batch_returns_0_and_writes_nothing(ctx):
    """9."""
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    for mode in (0, 3):
        r = Raw(ctx.h, pk, [], [], mode, n=0)
        assert r.rc == 0 and r.untouched()
        assert hg.verify_public_batch(ctx, pk, [], [], mode) == []
    pk.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_headline_size_batch_of_four(ctx, mode):
    """10. (32768,16): one bit-flipped proof, one instance with a changed ct0 coefficient"""
    n, k = 32768, 16
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0x8040 + 32 * mode + i) for i in range(4)]
    insts = [hg.Instance.from_witness(w) for w in ws]
    ps = [bfv.prove(ctx, pk, w, cap=1 << 25, mode=mode)[0] for w in ws]
    bad = bytearray(ps[1])
    bad[len(bad) // 3] ^= 4
    ps[1] = bytes(bad)
    a, ct0 = insts[2].coeffs()
    ct0[11 * n + 12345] += 1
    insts[2] = hg.Instance.from_ciphertext(bfv.params, a, ct0)
    got = batch_equals_singles(ctx, pk, insts, ps, mode)
    assert got[0][0] and got[3][0] and not got[2][0], [g[1] for g in got]   # (proof 1: as the single call decides)
    for i in (0, 3):
        assert hg.claims_settle(ctx, bfv.params, ws[i], got[i][2]) == (True, "")
    pk.free()
