"""hg_pcs_*_bn254 / hg_secrets_commit_bn254 / hg_claims_open_bn254 / hg_claims_verify_bn254: the polynomial commitment over bn256::Fr
that opens the claims hg_verify_public_bn254 leaves on the secret inputs. As in test_pcs.py the yardstick is a restatement of the
scheme of include/hg.h in Python integers (the oracle's Fr NTT and root of unity, the oracle's Keccak-256, the tree, the
transcript, the verifier's checks in their order): roots and openings of the host form are checked against it, the device form
against the host form byte for byte."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import orclib
from orclib import P, R_BN as R
from hglib import hg, ROOT

bn = orclib.bn254()
NEW = ["hg_pcs_commit_bn254", "hg_pcs_open_bn254", "hg_pcs_verify_bn254", "hg_secrets_commit_bn254", "hg_claims_open_bn254", "hg_claims_verify_bn254"]
# two of the C2_SHAPES of test_pcs.py (c = 2, code length 16): a multi-table and a single-table shape
C2_SHAPES = [(15, [5, 4, 3, 2]), (16, [6])]
# c = 2 shapes around the blocks of the leaf hash: a leaf is 4R + 1 message words, the Keccak rate 17 words. R = 4: 17 words, the
# padding alone in a second block; R = 5: 21 words (R = 4 and 5 lie around 4R + 1 = 16); R = 8: 33 = 34 - 1 words, the 0x01 and the
# 0x80 of the padding in the same word
LEAF_SHAPES = [(4, [4]), (5, [4, 2]), (8, [5])]
WRAPPER_SHAPES = [(1024, 1, 27), (4096, 2, 55)]


# ---- the scheme in Python integers -----------------------------------------------------------------------------------------------
def eq_table(pt):
    """eq(pt, x), coordinate i on bit i of x"""
    t = [1]
    for r in pt:
        hi = [v * r % R for v in t]
        t = [(v - h) % R for v, h in zip(t, hi)] + hi
    return t


def dot(ws, xs):
    return sum(w * int(x) for w, x in zip(ws, xs)) % R


def encode(row, c):
    """Enc: the oracle's size-4C NTT of the zero-padded row, natural order"""
    return bn.ntt([int(x) for x in row] + [0] * (3 << c))


def repr_(x):
    return int(x).to_bytes(32, "little")


def be32(x):
    return int(x).to_bytes(32, "big")


def le64(x):
    return int(x).to_bytes(8, "little")


class PyCommit:
    def __init__(self, tables, c):
        self.c, self.nvars = c, [len(t).bit_length() - 1 for t in tables]
        self.rows, self.off = [], []
        for t in tables:
            self.off.append(len(self.rows))
            self.rows += [[int(x) for x in t[r << c:(r + 1) << c]] for r in range(len(t) >> c)]
        self.M = [encode(r, c) for r in self.rows]
        leaves = [orclib.keccak256(le64(0) + b"".join(repr_(m[j]) for m in self.M)) for j in range(4 << c)]
        self.levels = [leaves]
        while len(self.levels[-1]) > 1:
            lo = self.levels[-1]
            self.levels.append([orclib.keccak256(le64(1) + lo[2 * i] + lo[2 * i + 1]) for i in range(len(lo) // 2)])
        self.root = self.levels[-1][0]


class PyTranscript:
    def __init__(self, root, c, nvars, Q, claims):
        le32 = lambda x: int(x).to_bytes(4, "little")   # noqa: E731
        self.pending = b"hg-pcs-bn254-1" + root + le32(c) + le32(len(nvars)) + b"".join(le32(v) for v in nvars) + le32(Q) + le32(len(claims))
        for t, pt, val in claims:
            self.pending += le32(t) + b"".join(repr_(x) for x in pt) + repr_(val)

    def squeeze(self):
        self.pending = orclib.keccak256(self.pending)
        return int.from_bytes(self.pending, "little") % R

    def absorb(self, x):
        self.pending += repr_(x)


def opening_len(nvars, c, n, Q):
    return 32 * (1 << c) * (n + 1) + Q * (32 * sum(1 << (v - c) for v in nvars) + 32 * (c + 2))


def py_verify(root, nvars, c, claims, Q, proof):
    """the verifier of include/hg.h, checks in the documented order; "" or the documented reason"""
    Cn, N, Rn, n = 1 << c, 4 << c, sum(1 << (v - c) for v in nvars), len(claims)
    off = [sum(1 << (v - c) for v in nvars[:t]) for t in range(len(nvars))]
    if len(proof) != opening_len(nvars, c, n, Q):
        return "pcs: the opening has %d bytes, %d expected" % (len(proof), opening_len(nvars, c, n, Q))
    elem = lambda at: int.from_bytes(proof[at:at + 32], "big")   # noqa: E731
    qb = 32 * Rn + 32 * (c + 2)
    for at in [32 * i for i in range(Cn * (n + 1))] + [32 * Cn * (n + 1) + q * qb + 32 * r for q in range(Q) for r in range(Rn)]:
        if elem(at) >= R:
            return "pcs: non-canonical word at byte %d" % at
    u = [[elem(32 * (i * Cn + j)) for j in range(Cn)] for i in range(n + 1)]
    for i, (t, pt, val) in enumerate(claims):
        if dot(eq_table(pt[:c]), u[i + 1]) != val:
            return "pcs: evaluation mismatch at claim %d" % i
    tr = PyTranscript(root, c, nvars, Q, claims)
    rho = tr.squeeze()
    for ui in u:
        for x in ui:
            tr.absorb(x)
    js = [(tr.squeeze() & 0xFFFFFFFFFFFFFFFF) & (N - 1) for _ in range(Q)]
    rho_pw = [pow(rho, r, R) for r in range(Rn)]
    enc = [encode(ui, c) for ui in u]
    for q in range(Q):
        base = 32 * Cn * (n + 1) + q * qb
        col = [elem(base + 32 * r) for r in range(Rn)]
        h, idx = orclib.keccak256(le64(0) + b"".join(repr_(x) for x in col)), js[q]
        for lv in range(c + 2):
            sib = proof[base + 32 * Rn + 32 * lv:base + 32 * Rn + 32 * (lv + 1)]
            h = orclib.keccak256(le64(1) + (sib + h if idx & 1 else h + sib))
            idx >>= 1
        if h != root:
            return "pcs: Merkle path mismatch at query %d" % q
        if dot(rho_pw, col) != enc[0][js[q]]:
            return "pcs: proximity mismatch at query %d" % q
        for i, (t, pt, _) in enumerate(claims):
            w = eq_table(pt[c:])
            if dot(w, col[off[t]:off[t] + len(w)]) != enc[i + 1][js[q]]:
                return "pcs: claim %d inconsistent at query %d" % (i, q)
    return ""


def py_mle(table, pt):
    return bn.mle_eval([int(x) for x in table], pt)


# ---- cases (computed once, never changed) ----------------------------------------------------------------------------------------
EDGE = [0, 1, R - 1, R - 2, (1 << 64) - 1, 1 << 64, (1 << 192) - 1, 1 << 253, (R - 1) // 2, (R + 1) // 2]


def make_tables(nvars, seed, edge=True):
    """random elements; the edge elements occur (0, 1, r-1, r-2 and limb boundaries)"""
    rng = random.Random(seed)
    out = []
    for v in nvars:
        t = [rng.randrange(R) for _ in range(1 << v)]
        if edge:
            for e in EDGE[:4] if v < 4 else EDGE:
                t[rng.randrange(len(t))] = e
        out.append(t)
    if edge:   # whatever the draws above overwrote
        for i, e in enumerate(EDGE[:4]):
            out[0][i % len(out[0])] = e
    return out


def make_claims(tables, n, seed):
    """n claims, claim i on table i mod m, at random points with the table's value: [(table, point, value)]"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        t = i % len(tables)
        pt = [rng.randrange(R) for _ in range(len(tables[t]).bit_length() - 1)]
        out.append((t, pt, py_mle(tables[t], pt)))
    return out


_C2 = {}


def c2_case(Rn):
    """per c = 2 shape: tables, the Python commitment, the host commitment and its openings (3 claims, Q = 5; no claim, Q = 1)"""
    if Rn not in _C2:
        nvars = dict(C2_SHAPES + LEAF_SHAPES)[Rn]
        tables = make_tables(nvars, 0xb9c5 + Rn)
        cm = hg.Commitment.commit_bn254(None, tables, log2_row=2)
        claims = make_claims(tables, 3, 77 + Rn)
        _C2[Rn] = dict(nvars=nvars, tables=tables, py=PyCommit(tables, 2), cm=cm, claims=claims, open35=cm.open(claims, 5), open01=cm.open([], 1))
    return _C2[Rn]


def _last():
    return hg.lib().hg_last_error().decode()


# ---- 1. surface ------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name


# ---- 2. the root -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rn,nvars", C2_SHAPES + LEAF_SHAPES)
def test_root_against_an_independent_recomputation(Rn, nvars):
    c = c2_case(Rn)
    assert len(c["py"].rows) == Rn
    assert c["cm"].root == c["py"].root
    assert c["cm"].field == "bn254" and c["cm"].nvars == nvars
    pool = set(x for t in c["tables"] for x in t)
    assert {0, 1, R - 1, R - 2} <= pool      # the edge elements occur


# ---- 3. openings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rn,nvars", C2_SHAPES)
def test_host_openings_are_accepted_by_an_independent_verifier(Rn, nvars):
    c = c2_case(Rn)
    for claims, Q, proof in ((c["claims"], 5, c["open35"]), ([], 1, c["open01"])):
        assert len(proof) == opening_len(nvars, 2, len(claims), Q) == hg.pcs_opening_bytes_bn254(nvars, len(claims), Q, 2)
        assert py_verify(c["py"].root, nvars, 2, claims, Q, proof) == ""
        assert hg.pcs_verify_bn254(c["cm"].root, nvars, claims, proof, Q, 2) == (True, "")
    # u_0, the opened column and the siblings of the opening are the Python commitment's
    py, proof = c["py"], c["open01"]
    tr = PyTranscript(py.root, 2, nvars, 1, [])
    rho = tr.squeeze()
    u0 = [dot([pow(rho, r, R) for r in range(Rn)], [row[j] for row in py.rows]) for j in range(4)]
    assert proof[:128] == b"".join(be32(x) for x in u0)
    for x in u0:
        tr.absorb(x)
    j = tr.squeeze() & 15
    assert proof[128:128 + 32 * Rn] == b"".join(be32(m[j]) for m in py.M)
    assert proof[128 + 32 * Rn:] == b"".join(py.levels[lv][(j >> lv) ^ 1] for lv in range(4))


# ---- 4. tampering ----------------------------------------------------------------------------------------------------------------
def test_tampered_openings_are_rejected_with_the_documented_reason():
    Rn, c = 15, c2_case(15)
    nvars, claims, proof, root = c["nvars"], c["claims"], c["open35"], c["cm"].root
    n, Q, Cn = 3, 5, 4
    qb, cols_at = 32 * Rn + 32 * 4, 32 * Cn * (n + 1)
    path0 = {"pcs: Merkle path mismatch at query 0", "pcs: proximity mismatch at query 0"}   # the indices move with the transcript

    def check(root_, claims_, proof_, allowed):
        ok, why = hg.pcs_verify_bn254(root_, nvars, claims_, proof_, Q, 2)
        assert not ok and why in allowed, (why, allowed)
        assert why == py_verify(root_, nvars, 2, claims_, Q, proof_)

    def flip(at, mask=0x01):
        b = bytearray(proof)
        b[at] ^= mask
        return bytes(b)

    check(root, claims, flip(32 * 2 + 31), path0)                                                       # u_0: every later challenge changes
    for i in range(n):
        check(root, claims, flip(32 * Cn * (i + 1) + 32 + 31), {"pcs: evaluation mismatch at claim %d" % i})   # u_i
    for q in (0, 3):
        check(root, claims, flip(cols_at + q * qb + 32 * 5 + 31), {"pcs: Merkle path mismatch at query %d" % q})     # a column element
        check(root, claims, flip(cols_at + q * qb + 32 * Rn + 32 * 2 + 9), {"pcs: Merkle path mismatch at query %d" % q})   # a sibling
    for i in range(n):                                                                                   # a wrong value at the verifier
        bad = [(t, pt, (v + 1) % R if k == i else v) for k, (t, pt, v) in enumerate(claims)]
        check(root, bad, proof, {"pcs: evaluation mismatch at claim %d" % i})
    for coord, allowed in ((0, {"pcs: evaluation mismatch at claim 0"}), (2, path0)):                    # a changed coordinate: below c / from c on
        t, pt, v = claims[0]
        bad = list(claims)
        bad[0] = (t, pt[:coord] + [(pt[coord] + 1) % R] + pt[coord + 1:], v)
        check(root, bad, proof, allowed)
    check(bytes([root[0] ^ 1]) + root[1:], claims, proof, {"pcs: Merkle path mismatch at query 0"})      # a wrong root
    want = len(proof)
    check(root, claims, proof + b"\0", {"pcs: the opening has %d bytes, %d expected" % (want + 1, want)})   # a wrong length
    check(root, claims, proof[:-1], {"pcs: the opening has %d bytes, %d expected" % (want - 1, want)})
    # an element set to r, in a u_i (ahead of the evaluation check it would also fail) and in a column: the byte is the element's first
    for at in (32 * Cn + 32, cols_at + qb + 32 * 2):
        bad = proof[:at] + be32(R) + proof[at + 32:]
        check(root, claims, bad, {"pcs: non-canonical word at byte %d" % at})
    bad = proof[:32] + b"\xff" * 32 + proof[64:]
    check(root, claims, bad, {"pcs: non-canonical word at byte 32"})
    # two at once: the order decides (the lower offset; a non-canonical element ahead of a wrong value)
    both = proof[:cols_at + 32] + be32(R) + proof[cols_at + 64:]
    both = both[:64] + be32(R + 1) + both[96:]
    check(root, claims, both, {"pcs: non-canonical word at byte 64"})
    wrong = [(t, pt, (v + 1) % R) for t, pt, v in claims]
    check(root, wrong, proof[:cols_at + 32] + be32(R) + proof[cols_at + 64:], {"pcs: non-canonical word at byte %d" % (cols_at + 32)})
    check(root, wrong, flip(cols_at + 31), {"pcs: evaluation mismatch at claim 0"})                      # ahead of query 0's path


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_a_wrong_value_is_refused_by_the_prover_naming_the_claim():
    c = c2_case(15)
    bad = list(c["claims"])
    t, pt, v = bad[1]
    bad[1] = (t, pt, (v + 1) % R)
    with pytest.raises(hg.HgError, match=r"hg_pcs_open_bn254: claim 1\b"):
        c["cm"].open(bad, 5)
    assert c["cm"].open(c["claims"], 5) == c["open35"]     # the handle still opens


def test_bad_arguments_are_errors_naming_the_function():
    L = hg._pcs_protos()
    c = c2_case(15)
    nvars, cm = c["nvars"], c["cm"]
    tabs = [hg.Context._fr_pack(t) for t in c["tables"]]
    ptrs = (hg.u64p * 4)(*[hg._ptr(t) for t in tabs])
    nv = (C.c_uint32 * 4)(*nvars)
    h, root = C.c_void_p(), (C.c_uint8 * 32)()
    # c > v_t, null arguments, no table, too many tables, a null table
    for args in ((None, ptrs, nv, 4, 3, C.byref(h), root), (None, None, nv, 4, 2, C.byref(h), root), (None, ptrs, None, 4, 2, C.byref(h), root),
                 (None, ptrs, nv, 4, 2, None, root), (None, ptrs, nv, 4, 2, C.byref(h), None), (None, ptrs, nv, 0, 2, C.byref(h), root),
                 (None, ptrs, nv, 65, 2, C.byref(h), root), (None, ptrs, nv, 4, 25, C.byref(h), root),
                 (None, (hg.u64p * 4)(ptrs[0], None, ptrs[2], ptrs[3]), nv, 4, 2, C.byref(h), root)):
        assert L.hg_pcs_commit_bn254(*args) == -1 and "hg_pcs_commit_bn254" in _last(), args
        assert not h.value
    bad = [list(t) for t in c["tables"]]
    bad[2][3] = R                                                # an element that is not below r
    with pytest.raises(hg.HgError, match="hg_pcs_commit_bn254: a table holds an element that is not below r"):
        hg.Commitment.commit_bn254(None, bad, 2)
    table, pts, vals = hg._pcs_claim_arrays_bn254(c["claims"])
    buf, ln = (C.c_uint8 * len(c["open35"]))(), C.c_size_t(0)
    good = (None, cm.h, table, hg._ptr(pts), hg._ptr(vals), 3, 5, buf, len(buf), C.byref(ln))

    def sub(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    far = (C.c_uint32 * 3)(0, 4, 2)                              # a table index out of range
    big = pts.copy()
    big[4:8] = hg.Context._fr_pack([R])                          # a non-canonical coordinate
    bigv = vals.copy()
    bigv[0:4] = hg.Context._fr_pack([R])                         # a non-canonical value
    # a Goldilocks handle
    gl = hg.Commitment.commit(None, [np.arange(1 << v, dtype=np.uint64) for v in nvars], 2)
    for args in (sub(good, 1, None), sub(good, 2, None), sub(good, 3, None), sub(good, 4, None), sub(good, 7, None), sub(good, 9, None), sub(good, 2, far),
                 sub(good, 3, hg._ptr(big)), sub(good, 4, hg._ptr(bigv)), sub(good, 8, len(buf) - 1), sub(good, 6, 1 << 20), sub(good, 1, gl.h)):
        assert L.hg_pcs_open_bn254(*args) == -1 and "hg_pcs_open_bn254" in _last(), args
    assert L.hg_pcs_open_bn254(*good) == 0 and bytes(buf) == c["open35"]
    # a BN254 handle into the Goldilocks entries
    gbuf = (C.c_uint8 * 4096)()
    assert L.hg_pcs_open(None, cm.h, None, None, None, 0, 1, gbuf, 4096, C.byref(ln)) == -1 and "hg_pcs_open" in _last() and "BN254" in _last()
    assert L.hg_pcs_open(None, gl.h, None, None, None, 0, 1, gbuf, 4096, C.byref(ln)) == 0     # its own handle still opens
    # hg_pcs_free takes both
    gl.free()
    extra = hg.Commitment.commit_bn254(None, c["tables"], 2)
    extra.free()
    assert extra.h is None and gl.h is None
    proof = c["open35"]
    vgood = (cm.root, nv, 4, 2, table, hg._ptr(pts), hg._ptr(vals), 3, 5, proof, len(proof))
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 4, None), sub(vgood, 5, None), sub(vgood, 6, None), sub(vgood, 9, None), sub(vgood, 4, far),
                 sub(vgood, 3, 3), sub(vgood, 2, 0), sub(vgood, 2, 65), sub(vgood, 5, hg._ptr(big)), sub(vgood, 6, hg._ptr(bigv)), sub(vgood, 8, 1 << 20)):
        assert L.hg_pcs_verify_bn254(*args) == -1 and "hg_pcs_verify_bn254" in _last(), args
    assert L.hg_pcs_verify_bn254(*vgood) == 0
    # the wrappers
    w = wrapper_case(1024, 1, 27)
    params, scm, cl = w["bfv"].params, w["cm"], w["claims"]
    obuf, oln = (C.c_uint8 * len(w["opening"]))(), C.c_size_t(0)
    for args in ((None, None, w["w"].h, 0, C.byref(h), root), (None, C.byref(params), None, 0, C.byref(h), root), (None, C.byref(params), w["w"].h, 0, None, root),
                 (None, C.byref(params), w["w"].h, 0, C.byref(h), None), (None, C.byref(params), w["w"].h, 11, C.byref(h), root),
                 (None, C.byref(hg.params_builtin(2048, 1)), w["w"].h, 0, C.byref(h), root)):
        assert L.hg_secrets_commit_bn254(*args) == -1 and "hg_secrets_commit_bn254" in _last(), args
    ogood = (None, C.byref(params), scm.h, cl.claims, cl.n, hg._ptr(cl.points), 0, obuf, len(obuf), C.byref(oln))
    vgood = (C.byref(params), scm.root, 0, cl.claims, cl.n, hg._ptr(cl.points), 0, w["opening"], len(w["opening"]))
    public = (hg.HgInputClaimBn254 * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3                                          # a claim on ais[0]: settled inside hg_verify_public_bn254, never opened
    short = (hg.HgInputClaimBn254 * cl.n)(*cl.claims[:cl.n])
    short[0].nvars -= 1
    glsec = hg.Commitment.secrets(None, params, w["w"])          # the Goldilocks commitment of the same witness
    for args in (sub(ogood, 1, None), sub(ogood, 2, None), sub(ogood, 3, None), sub(ogood, 5, None), sub(ogood, 7, None), sub(ogood, 9, None), sub(ogood, 3, public),
                 sub(ogood, 3, short), sub(ogood, 2, cm.h), sub(ogood, 2, glsec.h), sub(ogood, 1, C.byref(hg.params_builtin(2048, 1)))):
        assert L.hg_claims_open_bn254(*args) == -1 and "hg_claims_open_bn254" in _last(), args
    assert L.hg_claims_open_bn254(*ogood) == 0 and bytes(obuf) == w["opening"]
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 3, None), sub(vgood, 5, None), sub(vgood, 7, None), sub(vgood, 3, public), sub(vgood, 3, short),
                 sub(vgood, 2, 12)):
        assert L.hg_claims_verify_bn254(*args) == -1 and "hg_claims_verify_bn254" in _last(), args
    assert L.hg_claims_verify_bn254(*vgood) == 0


# ---- 6. the wrappers over the secret inputs --------------------------------------------------------------------------------------
_WRAP = {}


def wrapper_case(n, k, bits):
    """per shape: the reference's bn254 fixture as a witness, the oracle's proof (the way test_verify_public_bn254.py obtains it on the
    CPU), the claims hg_verify_public_bn254 leaves, the host commitment and its opening (defaults)"""
    if (n, k) not in _WRAP:
        bfv = hg.BfvEncrypt.new(n, k)
        w = hg.Witness.from_json_bn254(bfv.params, os.path.join(orclib.GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json"))
        proof = orclib.prove_f("bn254", orclib.params(n, k), orclib.bn254_fixture_inputs(n, k, bits), threads=8)[0]
        pk = bfv.setup(None)
        ok, why, claims = hg.verify_public_bn254(pk, hg.Instance.from_witness(w), proof)
        assert ok, why
        cm = hg.Commitment.secrets_bn254(None, bfv.params, w)
        _WRAP[(n, k)] = dict(bfv=bfv, pk=pk, w=w, d=w.arrays(), proof=proof, claims=claims, cm=cm, opening=cm.open_claims(bfv.params, claims))
    return _WRAP[(n, k)]


def fr_of(word):
    """the signed lift of a witness word: below 2^63 itself, else r - (p - word)"""
    w = int(word)
    return w if w < (1 << 63) else R - (P - w)


@pytest.mark.parametrize("n,k,bits", WRAPPER_SHAPES)
def test_claims_of_hg_verify_public_bn254_are_opened_and_verified(n, k, bits):
    c = wrapper_case(n, k, bits)
    params, cl = c["bfv"].params, c["claims"]
    lg = n.bit_length() - 1
    nvars = [lg + 1] * (3 + k) + [lg + k.bit_length() - 1]
    assert c["cm"].nvars == nvars and cl.n > 0
    assert len(c["opening"]) == hg.pcs_opening_bytes_bn254(nvars, cl.n) == opening_len(nvars, hg.pcs_row_log2(nvars), cl.n, 241)
    assert hg.claims_verify_bn254(params, c["cm"].root, cl, c["opening"]) == (True, "")
    assert hg.claims_settle_bn254(None, params, c["w"], cl) == (True, "")
    # the same bytes through the generic layer: the lifted tables in input order, ids mapped 0 1 2 -> 0 1 2, 3+k+i -> 3+i, 3+2k -> 3+k
    sz = 2 * n
    words = [c["d"]["s"], c["d"]["e"], c["d"]["k1"]] + [c["d"]["r1is"][i * sz:(i + 1) * sz] for i in range(k)] + [c["d"]["r2is"]]
    assert any(int(x) >= (1 << 63) for t in words for x in t)            # negative words occur
    generic = hg.Commitment.commit_bn254(None, [[fr_of(x) for x in t] for t in words])
    assert generic.root == c["cm"].root
    mapped = [(i if i < 3 else i - k, list(hg.Context._fr_unpack(np.array(pt, dtype=np.uint64))), hg.Context._fr_unpack(np.array(v, dtype=np.uint64))[0])
              for i, _, pt, v in cl.as_tuples()]
    assert generic.open(mapped) == c["opening"]
    assert hg.pcs_verify_bn254(generic.root, nvars, mapped, c["opening"]) == (True, "")
    # a flipped byte in the last sibling
    bad = bytearray(c["opening"])
    bad[-1] ^= 1
    assert hg.claims_verify_bn254(params, c["cm"].root, cl, bytes(bad)) == (False, "pcs: Merkle path mismatch at query 240")


@pytest.mark.parametrize("n,k,bits", WRAPPER_SHAPES)
def test_an_opening_from_another_witness_does_not_verify(n, k, bits):
    """one changed word of s: hg_claims_open_bn254 refuses (a claim on s is no longer the table's value), or the opening is rejected
    against the honest root; hg_claims_settle_bn254 on the same claims and witness decides the same way"""
    c = wrapper_case(n, k, bits)
    d = {f: v.copy() for f, v in c["d"].items()}
    d["s"][0] = (int(d["s"][0]) + 1) % P
    other_w = hg.Witness.from_arrays(c["bfv"].params, d)
    other = hg.Commitment.secrets_bn254(None, c["bfv"].params, other_w)
    assert other.root != c["cm"].root
    assert hg.claims_settle_bn254(None, c["bfv"].params, other_w, c["claims"])[0] is False
    try:
        forged = other.open_claims(c["bfv"].params, c["claims"])
    except hg.HgError as e:
        assert re.search(r"hg_claims_open_bn254: claim \d+\b", str(e))
        return
    ok, why = hg.claims_verify_bn254(c["bfv"].params, c["cm"].root, c["claims"], forged)
    assert not ok and why.startswith("pcs: ")


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def device_equals_host(ctx, tables, log2_row, seed, n_claims=3):
    host = hg.Commitment.commit_bn254(None, tables, log2_row)
    dev = hg.Commitment.commit_bn254(ctx, tables, log2_row)
    assert dev.root == host.root
    claims = make_claims(tables, n_claims, seed)
    for cl, Q in ((claims, 5), ([], 1)):
        proof = dev.open(cl, Q)
        assert proof == host.open(cl, Q)
        assert hg.pcs_verify_bn254(host.root, host.nvars, cl, proof, Q, log2_row) == (True, "")
    return host, dev


@pytest.mark.gpu
@pytest.mark.parametrize("Rn,nvars", C2_SHAPES + LEAF_SHAPES)
def test_device_form_equals_the_host_form_radix2_path(ctx, Rn, nvars):
    """log2n = 4, below the four-step range; R = 4, 5, 8, 15, 16: the leaf hash with the padding alone in a block, in one word, apart"""
    c = c2_case(Rn)
    dev = hg.Commitment.commit_bn254(ctx, c["tables"], 2)
    assert dev.root == c["cm"].root == c["py"].root
    assert dev.open(c["claims"], 5) == c["open35"] and dev.open([], 1) == c["open01"]


@pytest.mark.gpu
@pytest.mark.parametrize("nvars", [[8, 7, 6], [11]])
def test_device_form_equals_the_host_form_four_step_path(ctx, nvars):
    """c = 6: the encoding is the LDS four-step NTT of size 256, the first of its range; R = 7 and R = 32"""
    device_equals_host(ctx, make_tables(nvars, 0xb6c6 + len(nvars)), 6, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [14, 15])
def test_device_form_at_the_upper_edge_of_the_four_step_range(ctx, nv):
    """one row of 2^nv elements: log2n = 16 is the last four-step size, log2n = 17 takes the radix-2 stages above it (4 MB encoded)"""
    device_equals_host(ctx, make_tables([nv], 0xb7c7 + nv), nv, 6, n_claims=1)


@pytest.mark.gpu
def test_combine_across_its_reduction_chunk_with_the_largest_elements(ctx):
    """one table of 2^13 elements in rows of 4: 2048 rows, two reduction chunks of 1024; every element r - 1; one claim, whose value is
    r - 1 at every point (the eq weights sum to one)"""
    table = np.tile(hg.Context._fr_pack([R - 1]), 1 << 13)
    host = hg.Commitment.commit_bn254(None, [table], 2)
    dev = hg.Commitment.commit_bn254(ctx, [table], 2)
    assert dev.root == host.root
    rng = random.Random(0xc0b1)
    claims = [(0, [rng.randrange(R) for _ in range(13)], R - 1)]
    proof = dev.open(claims, 3)
    assert proof == host.open(claims, 3)
    assert hg.pcs_verify_bn254(host.root, [13], claims, proof, 3, 2) == (True, "")


@pytest.mark.gpu
def test_a_non_canonical_element_is_refused_by_the_device_form(ctx):
    bad = make_tables([6, 2], 3)
    bad[0][63] = R
    texts = []
    for c in (ctx, None):
        with pytest.raises(hg.HgError) as e:
            hg.Commitment.commit_bn254(c, bad, 2)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "hg_pcs_commit_bn254" in texts[0]
    host = hg.Commitment.commit_bn254(None, make_tables([6, 2], 3), 2)
    with pytest.raises(hg.HgError, match="hg_pcs_open_bn254"):       # a host-form handle opened with a context
        hg._check(hg._pcs_protos().hg_pcs_open_bn254(ctx.h, host.h, None, None, None, 0, 1, (C.c_uint8 * 8192)(), 8192, C.byref(C.c_size_t(0))))


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", WRAPPER_SHAPES)
def test_wrappers_on_the_device_equal_the_host_form(ctx, n, k, bits):
    c = wrapper_case(n, k, bits)
    dev = hg.Commitment.secrets_bn254(ctx, c["bfv"].params, c["w"])
    assert dev.root == c["cm"].root
    opening = dev.open_claims(c["bfv"].params, c["claims"])
    assert opening == c["opening"]
    assert hg.claims_verify_bn254(c["bfv"].params, dev.root, c["claims"], opening) == (True, "")


@pytest.mark.gpu
def test_headline_size_once(ctx):
    """(32768,16), a synthetic witness, the claims of hg_verify_public_device_bn254 on its hg_prove_bn254 proof: c = 11, R = 864, four-step
    NTT of 2^13"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x8000 + 16)
    proof = ctx.prove_bn254(pk, w, cap=1 << 25)[0]
    ok, why, cl = hg.verify_public_bn254(pk, hg.Instance.from_witness(w), proof, ctx=ctx, device=True)
    assert ok, why
    dev = hg.Commitment.secrets_bn254(ctx, bfv.params, w)
    assert dev.log2_row == 11
    opening = dev.open_claims(bfv.params, cl)
    assert len(opening) == hg.pcs_opening_bytes_bn254(dev.nvars, cl.n) == 32 * 2048 * (cl.n + 1) + 241 * (32 * 864 + 32 * 13)
    assert hg.claims_verify_bn254(bfv.params, dev.root, cl, opening) == (True, "")
    assert hg.Commitment.secrets_bn254(None, bfv.params, w).root == dev.root
    pk.free()
