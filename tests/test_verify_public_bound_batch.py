"""hg_verify_public_bound_batch: a run of bound proofs verified in one pass, and hg_instance_digest_group, the digest that pass takes
out of its staged sets (k_instance_digest_group). The single entries are the yardsticks: every item of a batch gets the decision, the
reason, the claims and the points that hg_verify_public_bound_device (and the host form) gives it alone, and every digest is the host
tree's and the Python recomputation's, byte for byte. Nothing here has a tolerance."""
import ctypes as C
import os
import random
import re
import struct

import numpy as np
import pytest

import orclib
from hglib import hg, ROOT, have_gpu

ENTRY, DIGEST = "hg_verify_public_bound_batch", "hg_instance_digest_group"
BINDING = ENTRY + ": binding needs the absorbing transcript (mode bit 1)"
CAP = 256
Q1 = orclib.constants(1024, 1)["qis"]
Q2 = orclib.constants(4096, 2)["qis"]


def _last():
    return hg.lib().hg_last_error().decode()


def params_of(n, k, qis):
    return hg.params_builtin(n, k) if qis is None else hg.params_derive(n, k, qis, 65537)


class Raw:
    """one raw call with every output prefilled with a pattern; `drop` names arguments passed as NULL"""

    def __init__(self, ctx_h, pk, insts, roots, proofs, mode, n=None, drop=(), caps=None, null_pk=False):
        nc, nco = hg.pk_claim_shape(pk)
        self.nc, self.nco = caps or (nc, nco)
        n = len(proofs) if n is None else n
        m = max(n, len(proofs), 1)
        I = (C.c_void_p * m)(*insts)
        R = (C.c_char_p * m)(*roots)
        Pf = (C.c_char_p * m)(*proofs)
        N = (C.c_size_t * m)(*[len(p) if p else 0 for p in proofs])
        self.res = (C.c_int * m)(*([7] * m))
        self.claims = (C.c_uint8 * (32 * m * max(nc, 1)))(*([0x55] * (32 * m * max(nc, 1))))
        self.points = np.full(2 * m * max(nco, 1), 0x5555, dtype=np.uint64)
        self.counts = (C.c_size_t * m)(*([9] * m))
        self.dg = (C.c_uint8 * (32 * m))(*([0x55] * (32 * m)))
        self.reasons = C.create_string_buffer(b"\x55" * (m * CAP), m * CAP)
        a = dict(instances=I, roots=R, proofs=Pf, lens=N, results=self.res, claims=self.claims, points=hg._ptr(self.points), n_claims=self.counts,
                 digests=self.dg, reasons=self.reasons)
        for d in drop:
            a[d] = None
        self.rc = getattr(hg.lib(), ENTRY)(ctx_h, None if null_pk else pk.h, a["instances"], a["roots"], a["proofs"], a["lens"], n, mode, a["results"],
                                           a["claims"], self.nc, a["points"], self.nco, a["n_claims"],
                                           a["digests"], a["reasons"], CAP)
        self.m = m

    def untouched(self):
        return (list(self.res) == [7] * self.m and list(self.counts) == [9] * self.m and self.reasons.raw == b"\x55" * (self.m * CAP)
                and bytes(self.claims) == b"\x55" * len(self.claims) and (self.points == 0x5555).all() and bytes(self.dg) == b"\x55" * (32 * self.m))


# ---- not GPU ----------------------------------------------------------------------------------------------------------------------
def _sig_pattern(text):
    sig = text.split()
    return "".join(re.escape(t) + (r"\s+" if u and t[-1].isalnum() and (u[0].isalnum() or u[0] == "_") else r"\s*") for t, u in zip(sig, sig[1:] + [""]))


def test_entry_points_declared_listed_exported_and_mirrored():
    """1."""
    full = open(os.path.join(ROOT, "include", "hg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", full, flags=re.S)
    assert re.search(_sig_pattern(
        "int hg_verify_public_bound_batch ( hg_ctx * ctx , const hg_pk * pk , const void * const * instances , const uint8_t * const * roots , "
        "const uint8_t * const * proofs , const size_t * lens , size_t n , int mode , int * results , void * claims , size_t claim_cap_each , "
        "uint64_t * points , size_t coord_cap_each , size_t * n_claims , uint8_t * digests , char * reasons , size_t reason_cap ) ;"), hdr)
    assert re.search(_sig_pattern("int hg_instance_digest_group ( hg_ctx * ctx , const void * const * instances , size_t n , uint8_t * out ) ;"), hdr)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in (ENTRY, DIGEST):
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
        assert "`%s(" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), name
    assert callable(hg.verify_public_bound_batch) and callable(hg.instance_digest_group)
    opts = re.search(r"Context options(.*?)Returns 0", full, flags=re.S).group(1)
    assert ENTRY in re.search(r'"verify_batch_group"(.*?)"bound_batch_slice"', opts, flags=re.S).group(1)
    assert re.search(r'"bound_batch_slice"[^"]*' + ENTRY, opts, flags=re.S)


def every_case(ctx_h, pk, device, ih, oh, proof):
    """every bad-argument case of hg_verify_public_batch, the roots and the mode rule; device: a device context with a device key, so
    that each case is wrong in one thing only"""
    nc, nco = hg.pk_claim_shape(pk)
    root = bytes(range(32))

    def is_error(r, what, word=None):
        assert r.rc == -1 and _last().startswith(ENTRY + ": ") and r.untouched(), (what, r.rc, _last())
        assert word is None or word in _last(), (what, _last())

    if not device:
        is_error(Raw(ctx_h, pk, [ih], [root], [proof], 3), "context or key")
    for d in ("instances", "roots", "proofs", "lens", "results", "n_claims", "claims", "points"):
        is_error(Raw(ctx_h, pk, [ih], [root], [proof], 3, drop=(d,)), "null " + d)
    is_error(Raw(ctx_h, pk, [ih], [root], [proof], 3, null_pk=True), "null key")
    is_error(Raw(ctx_h, pk, [ih, None], [root, root], [proof, proof], 3), "null instance", "index 1" if device else None)
    is_error(Raw(ctx_h, pk, [ih, ih], [root, root], [proof, None], 3), "null proof", "index 1" if device else None)
    is_error(Raw(ctx_h, pk, [ih, ih], [root, None], [proof, proof], 3), "null root", "index 1" if device else None)
    for mode in (0, 2):
        r = Raw(ctx_h, pk, [ih], [root], [proof], mode)
        is_error(r, "mode without bit 1")
        assert _last() == BINDING
    for mode in (-1, 4):
        is_error(Raw(ctx_h, pk, [ih], [root], [proof], mode), "mode", "unknown mode bits")
    is_error(Raw(ctx_h, pk, [ih], [root], [proof], 3, caps=(nc - 1, nco)), "claim cap", "hg_pk_claim_shape" if device else None)
    is_error(Raw(ctx_h, pk, [ih], [root], [proof], 3, caps=(nc, nco - 1)), "coordinate cap", "hg_pk_claim_shape" if device else None)
    is_error(Raw(ctx_h, pk, [ih, oh, ih], [root] * 3, [proof] * 3, 3), "an instance of (2048,1) among (1024,1)", "index 1" if device else None)
    # the digest entry: the contract of hg_instance_digest_batch
    f = getattr(hg.lib(), DIGEST)
    out = (C.c_uint8 * 64)(*([0x55] * 64))
    hs = (C.c_void_p * 2)(ih, ih)
    for args in ((None, 2, out), (hs, 2, None), ((C.c_void_p * 2)(ih, None), 2, out), ((C.c_void_p * 2)(ih, oh), 2, out)):
        assert f(ctx_h, *args) == -1 and _last().startswith(DIGEST + ": "), (args[1:], _last())
    if ctx_h is not None:
        assert "mixed parameters" in _last()
    else:
        assert f(None, hs, 2, out) == -1 and _last().startswith(DIGEST + ": ") and "no context" in _last()
    assert f(ctx_h, None, 0, None) == 0 and bytes(out) == b"\x55" * 64


def _bad_argument_fixture():
    bfv = hg.BfvEncrypt.new(1024, 1)
    inst = hg.Instance.from_witness(hg.Witness.synthetic(bfv.params, 21))
    other = hg.Instance.from_witness(hg.Witness.synthetic(hg.params_builtin(2048, 1), 5))
    return bfv, inst, other, bytes(16 * 64)


def test_bad_arguments_are_errors_naming_the_function():
    """2. without a context, and (where a GPU is present) on a device context with a host-only key"""
    bfv, inst, other, proof = _bad_argument_fixture()
    host_pk = bfv.setup(None)
    every_case(None, host_pk, False, inst.h.value, other.h.value, proof)
    for mode in (1, 3):
        with pytest.raises(hg.HgError, match="^" + ENTRY):
            hg.verify_public_bound_batch(None, host_pk, [inst], [bytes(32)], [proof], mode)
    with pytest.raises(hg.HgError, match="^" + re.escape(BINDING) + "$"):
        hg.verify_public_bound_batch(None, host_pk, [inst], [bytes(32)], [proof], 2)
    with pytest.raises(hg.HgError, match="^" + DIGEST):
        hg.instance_digest_group(None, [inst])
    if have_gpu():
        ctx = hg.Context(0)
        try:
            every_case(ctx.h, host_pk, False, inst.h.value, other.h.value, proof)
        finally:
            ctx.close()
    host_pk.free()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def edge_instance(params, seed):
    """random in-range coefficients with 0, -1, +(q_i-1)/2 and -(q_i-1)/2 on the first and last word of every leaf and modulus block"""
    n, k = params.n, params.k
    rng = random.Random(seed)
    B = min(128, 2 * k * n)
    out = []
    turn = 0
    for _ in range(2):
        t = np.zeros(k * n, dtype=np.int64)
        for i in range(k):
            half = (params.qis[i] - 1) // 2
            t[i * n:(i + 1) * n] = [rng.randint(-half, half) for _ in range(n)]
            edges = [0, -1, half, -half]
            marks = {0, n - 1} | {j for j in range(n) if (i * n + j) % B in (0, B - 1)}
            for j in sorted(marks):
                t[i * n + j] = edges[turn % 4]
                turn += 1
        out.append(t)
    return out


def py_digest(a, ct0):
    """the definition of include/hg.h, written out independently of the library"""
    words = [int(x) for x in a] + [int(x) for x in ct0]
    B = min(128, len(words))
    level = [orclib.keccak256(struct.pack("<Q", 2) + b"".join(struct.pack("<q", w) for w in words[j * B:(j + 1) * B])) for j in range(len(words) // B)]
    while len(level) > 1:
        level = [orclib.keccak256(struct.pack("<Q", 1) + level[2 * i] + level[2 * i + 1]) for i in range(len(level) // 2)]
    return level[0]


# (n, k, moduli or None for the built-in set) and the leaves of a member: one short leaf; one full leaf (a single-leaf root); a and ct0
# in separate leaves; a partial workgroup; a modulus boundary inside a table; exactly one full workgroup (the root inside the kernel);
# two workgroups (the second launch with two nodes); a larger second launch
DIGEST_SETS = [(32, 1, Q1, 1), (64, 1, Q1, 1), (64, 2, Q2, 2), (1024, 1, None, 16), (1024, 2, Q2, 32), (2048, 2, Q2, 64), (4096, 2, None, 128), (8192, 2, Q2, 256)]
_MEMBERS = {}


def digest_members(n, k, qis):
    """per parameter set four edge instances with their Python digests (computed once, never changed)"""
    if (n, k) not in _MEMBERS:
        params = params_of(n, k, qis)
        out = []
        for s in range(4):
            a, ct0 = edge_instance(params, 0x6d0 + 16 * n + 4 * k + s)
            out.append((hg.Instance.from_ciphertext(params, a, ct0), py_digest(a, ct0)))
        _MEMBERS[(n, k)] = out
    return _MEMBERS[(n, k)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,qis,leaves", DIGEST_SETS)
def test_group_digest_equals_the_definition_and_the_host_tree(ctx, n, k, qis, leaves):
    """3. 1, 2 and 5 members in a permuted order, one instance twice, in slices of 1, 2 and the default"""
    mem = digest_members(n, k, qis)
    assert 2 * k * n // min(128, 2 * k * n) == leaves
    for inst, want in mem:
        assert len(want) == 32 and hg.instance_digest(inst) == want
    assert len({w for _, w in mem}) == 4
    try:
        for slice_ in (1, 2, 0):
            ctx.set_option("bound_batch_slice", slice_)
            for sel in ([2], [1, 0], [3, 0, 2, 0, 1]):
                got = hg.instance_digest_group(ctx, [mem[j][0] for j in sel])
                assert got == [mem[j][1] for j in sel], (slice_, sel)
    finally:
        ctx.set_option("bound_batch_slice", 0)
    assert hg.instance_digest_group(ctx, []) == []


SHAPES = {(1024, 1): None, (1024, 2): Q2}
_CASES = {}


def case(ctx, n, k, count=2):
    """per shape: device key and `count` synthetic witnesses with their instances and, per mode, their bound proofs and commitments
    (made once, never changed)"""
    c = _CASES.get((n, k))
    if c is None:
        bfv = hg.BfvEncrypt(params_of(n, k, SHAPES[(n, k)]))
        c = _CASES[(n, k)] = dict(bfv=bfv, pk=bfv.setup(ctx), ws=[], insts=[], bound={1: [], 3: []}, unbound={1: [], 3: []})
    while len(c["ws"]) < count:
        w = hg.Witness.synthetic(c["bfv"].params, 0xbb0 + 64 * n + 8 * k + len(c["ws"]))
        vals = hg.witness_gen(ctx, c["pk"], w)
        for mode in (1, 3):
            out, cm = hg.prove_committed_mode(ctx, c["pk"], vals, hg.ProofBuffer(), mode)
            c["bound"][mode].append((out.bytes(), cm))
            c["unbound"][mode].append(hg.prove_resident_mode(ctx, c["pk"], vals, hg.ProofBuffer(), mode).bytes())
        vals.free()
        c["ws"].append(w)
        c["insts"].append(hg.Instance.from_witness(w))
    return c


def flat(got):
    return [(ok, why, (cl.as_tuples() if ok else None)) for ok, why, cl in got]


def single(ctx, pk, inst, root, proof, mode, host=False):
    ok, why, cl = hg.verify_public_bound(pk, inst, proof, root, mode) if host else hg.verify_public_bound(pk, inst, proof, root, mode, ctx=ctx, device=True)
    return ok, why, (cl.as_tuples() if ok else None)


def batch(ctx, pk, insts, roots, proofs, mode):
    got, dg = hg.verify_public_bound_batch(ctx, pk, insts, roots, proofs, mode)
    assert len(got) == len(dg) == len(proofs)
    return got, flat(got), dg


def tampered(proof):
    """bit-flipped copies at fixed offsets, half the bytes, all but the last 16"""
    L = len(proof)
    out = []
    for pos, bit in ((0, 1), (L // 7, 4), (L // 3, 0x20), (2 * L // 3, 2), (L - 9, 0x80)):
        bad = bytearray(proof)
        bad[pos] ^= bit
        out.append(bytes(bad))
    return out + [proof[:L // 2], proof[:-16]]


def flipped(root, at):
    r = bytearray(root)
    r[at] ^= 1
    return bytes(r)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", list(SHAPES))
@pytest.mark.parametrize("mode", [1, 3])
def test_batch_equals_singles(ctx, n, k, mode):
    """4."""
    c = case(ctx, n, k)
    pk, (i0, i1), ws = c["pk"], c["insts"][:2], c["ws"]
    (p0, cm0), (p1, cm1) = c["bound"][mode][:2]
    r0, r1 = cm0.root, cm1.root
    po, cmo = c["bound"][4 - mode][0]
    items = [(i0, r0, p0, ws[0]), (i1, r1, p1, ws[1])]
    items += [(i0, r0, t, None) for t in tampered(p0)]
    items += [(i0, flipped(r0, 0), p0, None), (i0, flipped(r0, 31), p0, None)]
    items += [(i0, r1, p0, None), (i1, r0, p1, None)]               # the roots swapped
    items += [(i1, r0, p0, None), (i0, r1, p1, None)]               # the instances swapped
    items += [(i0, r0, c["unbound"][mode][0], None)]                # an unbound proof of the same values
    items += [(i0, cmo.root, po, None)]                             # a bound proof made in the other mode
    insts, roots, proofs = [x[0] for x in items], [x[1] for x in items], [x[2] for x in items]
    got, flat_, dg = batch(ctx, pk, insts, roots, proofs, mode)
    for i, (inst, root, proof, w) in enumerate(items):
        want = single(ctx, pk, inst, root, proof, mode)
        assert flat_[i] == want, (i, flat_[i][:2], want[:2])
        assert single(ctx, pk, inst, root, proof, mode, host=True) == want, i
        assert dg[i] == hg.instance_digest(inst), i
        if i < 2:
            assert got[i][0], (i, got[i][1])
            assert hg.claims_settle(ctx, c["bfv"].params, w, got[i][2]) == (True, "")
        else:
            assert not got[i][0] and got[i][1] and got[i][2] is None, i


@pytest.mark.gpu
def test_groups_and_slices_do_not_change_the_results(ctx):
    """5."""
    c = case(ctx, 1024, 1, count=8)
    pk, mode = c["pk"], 3
    insts = list(c["insts"][:8])
    proofs = [p for p, _ in c["bound"][mode][:8]]
    roots = [cm.root for _, cm in c["bound"][mode][:8]]
    proofs[0] = proofs[0][:len(proofs[0]) // 2]
    insts[6] = insts[5]
    roots[3] = roots[2]
    runs = []
    try:
        for group in (0, 3):
            for slice_ in (0, 1, 2):
                ctx.set_option("verify_batch_group", group)
                ctx.set_option("bound_batch_slice", slice_)
                _, f, dg = batch(ctx, pk, insts, roots, proofs, mode)
                runs.append((f, dg))
    finally:
        ctx.set_option("verify_batch_group", 0)
        ctx.set_option("bound_batch_slice", 0)
    for r in runs[1:]:
        assert r == runs[0]
    one, dg = runs[0]
    assert [r[0] for r in one] == [False, True, True, False, True, True, False, True], [r[1] for r in one]
    for i in range(8):
        assert one[i] == single(ctx, pk, insts[i], roots[i], proofs[i], mode), i
        assert dg[i] == hg.instance_digest(insts[i]), i


@pytest.mark.gpu
def test_the_whole_no_secret_route_for_a_run(ctx):
    """6."""
    c = case(ctx, 1024, 2, count=3)
    pk, params, mode = c["pk"], c["bfv"].params, 3
    insts = c["insts"][:3]
    proofs = [p for p, _ in c["bound"][mode][:3]]
    cms = [cm for _, cm in c["bound"][mode][:3]]
    roots = [cm.root for cm in cms]
    got, f, _ = batch(ctx, pk, insts, roots, proofs, mode)
    assert all(g[0] for g in got), [g[1] for g in got]
    claims = [g[2] for g in got]
    openings = [cm.open_claims(params, cl) for cm, cl in zip(cms, claims)]
    assert hg.claims_verify_batch(ctx, params, roots, claims, openings) == [(True, "")] * 3
    roots2 = [roots[0], roots[0], roots[2]]
    got2, f2, _ = batch(ctx, pk, insts, roots2, proofs, mode)
    assert not got2[1][0] and got2[1][1] and f2[0] == f[0] and f2[2] == f[2]
    second = hg.claims_verify_batch(ctx, params, roots2, [got2[0][2], None, got2[2][2]], openings)
    assert second[0] == (True, "") and second[2] == (True, "")


@pytest.mark.gpu
def test_errors_on_a_device_context_with_a_device_key(ctx):
    """7."""
    c = case(ctx, 1024, 1)
    _, inst, other, proof = _bad_argument_fixture()
    every_case(ctx.h, c["pk"], True, inst.h.value, other.h.value, proof)


@pytest.mark.gpu
def test_the_context_stays_usable(ctx):
    """8. what ran before gives the same after bound batches that include a rejected item"""
    c = case(ctx, 1024, 2)
    pk, w, inst = c["pk"], c["ws"][0], c["insts"][0]
    vals = hg.witness_gen(ctx, pk, w)
    out = hg.ProofBuffer()
    first = [hg.prove_resident(ctx, pk, vals, out).bytes() for _ in range(3)]
    assert first[0] == first[1] == first[2]
    p3, cm3 = c["bound"][3][0]
    u3 = c["unbound"][3][0]

    def snapshot():
        return dict(
            prove=[hg.prove_resident(ctx, pk, vals, out).bytes() for _ in range(3)],
            pub0=flat(hg.verify_public_batch(ctx, pk, [inst, inst], [first[0], first[0][:-16]], 0)),
            pub3=flat(hg.verify_public_batch(ctx, pk, [inst, inst], [u3, u3[:-16]], 3)),
            bound=single(ctx, pk, inst, cm3.root, p3, 3),
            digests=hg.instance_digest_batch(ctx, c["insts"][:2]),
            dev=hg.verify_device_batch(ctx, pk, [w, w], [u3, u3[:len(u3) // 2]], mode=3))
    before = snapshot()
    assert before["prove"] == first and before["pub0"][0][0] and before["pub3"][0][0] and before["bound"][0] and before["dev"][0] == (True, "")
    assert not before["pub0"][1][0] and not before["pub3"][1][0]
    for _ in range(2):
        got, _, dg = batch(ctx, pk, [inst, inst, c["insts"][1]], [cm3.root, flipped(cm3.root, 5), cm3.root], [p3, p3, p3[:-16]], 3)
        assert [g[0] for g in got] == [True, False, False]
        assert dg == [before["digests"][0], before["digests"][0], before["digests"][1]]
        assert snapshot() == before
    vals.free()


@pytest.mark.gpu
def test_an_empty_run_returns_0_and_writes_nothing(ctx):
    """9."""
    c = case(ctx, 1024, 1)
    for mode in (1, 3):
        r = Raw(ctx.h, c["pk"], [], [], [], mode, n=0)
        assert r.rc == 0 and r.untouched()
        assert hg.verify_public_bound_batch(ctx, c["pk"], [], [], [], mode) == ([], [])


@pytest.mark.gpu
def test_headline_size_run_of_four(ctx):
    """10. (32768,16), mode 3: a bit-flipped proof, a changed ct0 coefficient (another digest), a root with one bit flipped"""
    n, k, mode = 32768, 16, 3
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0x80b0 + i) for i in range(4)]
    insts = [hg.Instance.from_witness(w) for w in ws]
    proofs, cms = [], []
    vals = hg.witness_gen(ctx, pk, ws[0])
    for i, w in enumerate(ws):
        if i:
            hg.witness_gen_into(ctx, pk, w, vals)
        out, cm = hg.prove_committed_mode(ctx, pk, vals, hg.ProofBuffer(cap=1 << 25), mode)
        proofs.append(out.bytes())
        cms.append(cm)
    vals.free()
    roots = [cm.root for cm in cms]
    bad = bytearray(proofs[1])
    bad[len(bad) // 3] ^= 4
    proofs[1] = bytes(bad)
    a, ct0 = insts[2].coeffs()
    ct0[11 * n + 12345] += 1
    insts[2] = hg.Instance.from_ciphertext(bfv.params, a, ct0)
    roots[3] = flipped(roots[3], 17)
    got, f, dg = batch(ctx, pk, insts, roots, proofs, mode)
    for i in range(4):
        assert f[i] == single(ctx, pk, insts[i], roots[i], proofs[i], mode), i
        assert dg[i] == hg.instance_digest(insts[i]), i
    assert got[0][0] and not got[2][0] and not got[3][0], [g[1] for g in got]   # (proof 1: as the single call decides)
    assert dg[2] != hg.instance_digest(hg.Instance.from_witness(ws[2]))
    opening = cms[0].open_claims(bfv.params, got[0][2])
    assert hg.claims_verify(bfv.params, roots[0], got[0][2], opening) == (True, "")
    for cm in cms:
        cm.free()
    pk.free()
