"""hg_pcs_* / hg_secrets_commit / hg_claims_open / hg_claims_verify: the polynomial commitment that opens the claims hg_verify_public
leaves on the secret inputs. The yardstick is a restatement of the scheme of include/hg.h in Python integers (direct DFT with the
oracle's root of unity, the oracle's Keccak-256, the tree, the transcript, the verifier's checks in their order): roots and openings
of the host form are checked against it, the device form against the host form byte for byte."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import orclib
from hglib import hg, ROOT

P = hg.P
NEW = ["hg_pcs_commit", "hg_pcs_free", "hg_pcs_open", "hg_pcs_verify", "hg_secrets_commit", "hg_claims_open", "hg_claims_verify"]
# c = 2 (code length 16); the hashed column is 1 + R words and the Keccak rate 17 words, so R = 15, 16, 17, 33 straddle one and two blocks
C2_SHAPES = [(15, [5, 4, 3, 2]), (16, [6]), (17, [6, 2]), (33, [7, 2])]
WRAPPER_SHAPES = [(1024, 1, 27), (4096, 2, 55)]


# ---- the scheme in Python integers -----------------------------------------------------------------------------------------------
def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def eq_table(pt):
    """eq(pt, x), coordinate i on bit i of x"""
    t = [(1, 0)]
    for r in pt:
        hi = [e_mul(v, r) for v in t]
        t = [((v[0] - h[0]) % P, (v[1] - h[1]) % P) for v, h in zip(t, hi)] + hi
    return t


def e_dot_f(ws, xs):
    c0 = c1 = 0
    for w, x in zip(ws, xs):
        c0 += w[0] * int(x)
        c1 += w[1] * int(x)
    return (c0 % P, c1 % P)


def e_dot(a, b):
    s = (0, 0)
    for x, y in zip(a, b):
        s = e_add(s, e_mul(x, y))
    return s


_DFT = {}


def encode(row, c):
    """Enc: the size-4C DFT of the zero-padded row, natural order (only the C non-zero inputs are summed)"""
    n = 4 << c
    if c not in _DFT:
        w = orclib.root_of_unity_f("goldilocks", c + 2)
        pw = [pow(w, i, P) for i in range(n)]
        _DFT[c] = [[pw[(j * k) % n] for j in range(1 << c)] for k in range(n)]
    return [sum(m * int(x) for m, x in zip(line, row)) % P for line in _DFT[c]]


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
        leaves = [orclib.keccak256(le64(0) + b"".join(le64(m[j]) for m in self.M)) for j in range(4 << c)]
        self.levels = [leaves]
        while len(self.levels[-1]) > 1:
            lo = self.levels[-1]
            self.levels.append([orclib.keccak256(le64(1) + lo[2 * i] + lo[2 * i + 1]) for i in range(len(lo) // 2)])
        self.root = self.levels[-1][0]


class PyTranscript:
    def __init__(self, root, c, nvars, Q, claims):
        le32 = lambda x: int(x).to_bytes(4, "little")   # noqa: E731
        self.pending = b"hg-pcs-1" + root + le32(c) + le32(len(nvars)) + b"".join(le32(v) for v in nvars) + le32(Q) + le32(len(claims))
        for t, pt, val in claims:
            self.pending += le32(t) + b"".join(le64(x) for x in pt) + le64(val[0]) + le64(val[1])

    def squeeze_f(self):
        self.pending = orclib.keccak256(self.pending)
        return int.from_bytes(self.pending, "little") % P

    def squeeze(self):
        a = self.squeeze_f()
        return (a, self.squeeze_f())

    def absorb(self, x):
        self.pending += le64(x)


def opening_len(nvars, c, n, Q):
    return 16 * (1 << c) * (n + 1) + Q * (8 * sum(1 << (v - c) for v in nvars) + 32 * (c + 2))


def py_verify(root, nvars, c, claims, Q, proof):
    """the verifier of include/hg.h, checks in the documented order; "" or the documented reason"""
    Cn, N, R, n = 1 << c, 4 << c, sum(1 << (v - c) for v in nvars), len(claims)
    off = [sum(1 << (v - c) for v in nvars[:t]) for t in range(len(nvars))]
    if len(proof) != opening_len(nvars, c, n, Q):
        return "pcs: the opening has %d bytes, %d expected" % (len(proof), opening_len(nvars, c, n, Q))
    word = lambda at: int.from_bytes(proof[at:at + 8], "big")   # noqa: E731
    qb = 8 * R + 32 * (c + 2)
    for at in [8 * i for i in range(2 * Cn * (n + 1))] + [16 * Cn * (n + 1) + q * qb + 8 * r for q in range(Q) for r in range(R)]:
        if word(at) >= P:
            return "pcs: non-canonical word at byte %d" % at
    u = [[(word(16 * (i * Cn + j)), word(16 * (i * Cn + j) + 8)) for j in range(Cn)] for i in range(n + 1)]
    pts = [[(pt[2 * i], pt[2 * i + 1]) for i in range(len(pt) // 2)] for _, pt, _ in claims]
    for i, (t, _, val) in enumerate(claims):
        if e_dot(u[i + 1], eq_table(pts[i][:c])) != tuple(val):
            return "pcs: evaluation mismatch at claim %d" % i
    tr = PyTranscript(root, c, nvars, Q, claims)
    rho = tr.squeeze()
    for ui in u:
        for x in ui:
            tr.absorb(x[0])
            tr.absorb(x[1])
    js = [tr.squeeze_f() & (N - 1) for _ in range(Q)]
    rho_pw = [(1, 0)]
    for _ in range(R - 1):
        rho_pw.append(e_mul(rho_pw[-1], rho))
    enc = [(encode([x[0] for x in ui], c), encode([x[1] for x in ui], c)) for ui in u]
    for q in range(Q):
        base = 16 * Cn * (n + 1) + q * qb
        col = [word(base + 8 * r) for r in range(R)]
        h, idx = orclib.keccak256(le64(0) + b"".join(le64(x) for x in col)), js[q]
        for lv in range(c + 2):
            sib = proof[base + 8 * R + 32 * lv:base + 8 * R + 32 * (lv + 1)]
            h = orclib.keccak256(le64(1) + (sib + h if idx & 1 else h + sib))
            idx >>= 1
        if h != root:
            return "pcs: Merkle path mismatch at query %d" % q
        if e_dot_f(rho_pw, col) != (enc[0][0][js[q]], enc[0][1][js[q]]):
            return "pcs: proximity mismatch at query %d" % q
        for i, (t, _, _) in enumerate(claims):
            w = eq_table(pts[i][c:])
            if e_dot_f(w, col[off[t]:off[t] + len(w)]) != (enc[i + 1][0][js[q]], enc[i + 1][1][js[q]]):
                return "pcs: claim %d inconsistent at query %d" % (i, q)
    return ""


def py_mle(table, pt):
    return e_dot_f(eq_table(pt), table)


# ---- cases (computed once, never changed) ----------------------------------------------------------------------------------------
def make_tables(nvars, seed):
    rng = random.Random(seed)
    return [orclib.edge_f(rng, 1 << v) for v in nvars]


def make_claims(tables, n, seed):
    """n claims, claim i on table i mod m, at random E points with the table's value: [(table, point words, (v0, v1))]"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        t = i % len(tables)
        nv = tables[t].size.bit_length() - 1
        pt = [(rng.randrange(P), rng.randrange(P)) for _ in range(nv)]
        out.append((t, [x for p in pt for x in p], py_mle(tables[t], pt)))
    return out


_C2 = {}


def c2_case(R):
    """per c = 2 shape: tables, the Python commitment, the host commitment and its openings (3 claims, Q = 5; no claim, Q = 1)"""
    if R not in _C2:
        nvars = dict(C2_SHAPES)[R]
        tables = make_tables(nvars, 0x9c5 + R)
        cm = hg.Commitment.commit(None, tables, log2_row=2)
        claims = make_claims(tables, 3, 77 + R)
        _C2[R] = dict(nvars=nvars, tables=tables, py=PyCommit(tables, 2), cm=cm, claims=claims, open35=cm.open(claims, 5), open01=cm.open([], 1))
    return _C2[R]


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
@pytest.mark.parametrize("R,nvars", C2_SHAPES)
def test_root_against_an_independent_recomputation(R, nvars):
    c = c2_case(R)
    assert len(c["py"].rows) == R
    assert c["cm"].root == c["py"].root
    pool = set(int(x) for t in c["tables"] for x in t)
    assert {0, P - 1, P - 2, 1} <= pool      # the edge words occur


# ---- 3. openings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,nvars", C2_SHAPES)
def test_host_openings_are_accepted_by_an_independent_verifier(R, nvars):
    c = c2_case(R)
    for claims, Q, proof in ((c["claims"], 5, c["open35"]), ([], 1, c["open01"])):
        assert len(proof) == opening_len(nvars, 2, len(claims), Q) == hg.pcs_opening_bytes(nvars, len(claims), Q, 2)
        assert py_verify(c["py"].root, nvars, 2, claims, Q, proof) == ""
        assert hg.pcs_verify(c["cm"].root, nvars, claims, proof, Q, 2) == (True, "")
    # the siblings of the opening are the Python tree's
    py, proof = c["py"], c["open01"]
    tr = PyTranscript(py.root, 2, nvars, 1, [])
    rho = tr.squeeze()
    u0 = [e_dot_f([pw for pw in _powers(rho, R)], [row[j] for row in py.rows]) for j in range(4)]
    assert proof[:64] == b"".join(x.to_bytes(8, "big") for e in u0 for x in e)
    for e in u0:
        tr.absorb(e[0])
        tr.absorb(e[1])
    j = tr.squeeze_f() & 15
    assert proof[64:64 + 8 * R] == b"".join(m[j].to_bytes(8, "big") for m in py.M)
    assert proof[64 + 8 * R:] == b"".join(py.levels[lv][(j >> lv) ^ 1] for lv in range(4))


def _powers(rho, n):
    out = [(1, 0)]
    for _ in range(n - 1):
        out.append(e_mul(out[-1], rho))
    return out


# ---- 4. tampering ----------------------------------------------------------------------------------------------------------------
def test_tampered_openings_are_rejected_with_the_documented_reason():
    R, c = 17, c2_case(17)
    nvars, claims, proof, root = c["nvars"], c["claims"], c["open35"], c["cm"].root
    n, Q, Cn = 3, 5, 4
    qb, cols_at = 8 * R + 32 * 4, 16 * Cn * (n + 1)
    path0 = {"pcs: Merkle path mismatch at query 0", "pcs: proximity mismatch at query 0"}   # the indices move with the transcript

    def check(root_, claims_, proof_, allowed):
        ok, why = hg.pcs_verify(root_, nvars, claims_, proof_, Q, 2)
        assert not ok and why in allowed, (why, allowed)
        assert why == py_verify(root_, nvars, 2, claims_, Q, proof_)

    def flip(at, mask=0x01):
        b = bytearray(proof)
        b[at] ^= mask
        return bytes(b)

    check(root, claims, flip(16 * 2 + 7), path0)                                                        # u_0: every later challenge changes
    for i in range(n):
        check(root, claims, flip(16 * Cn * (i + 1) + 16 + 15), {"pcs: evaluation mismatch at claim %d" % i})   # u_i
    for q in (0, 3):
        check(root, claims, flip(cols_at + q * qb + 8 * 5 + 7), {"pcs: Merkle path mismatch at query %d" % q})     # a column word
        check(root, claims, flip(cols_at + q * qb + 8 * R + 32 * 2 + 9), {"pcs: Merkle path mismatch at query %d" % q})   # a sibling
    for i in range(n):                                                                                   # a changed value
        bad = [(t, pt, ((v[0] + 1) % P, v[1]) if k == i else v) for k, (t, pt, v) in enumerate(claims)]
        check(root, bad, proof, {"pcs: evaluation mismatch at claim %d" % i})
    for coord, allowed in ((0, {"pcs: evaluation mismatch at claim 0"}), (2, path0)):                    # a changed coordinate: below c / from c on
        t, pt, v = claims[0]
        bad = list(claims)
        bad[0] = (t, pt[:2 * coord] + [(pt[2 * coord] + 1) % P] + pt[2 * coord + 1:], v)
        check(root, bad, proof, allowed)
    check(bytes([root[0] ^ 1]) + root[1:], claims, proof, {"pcs: Merkle path mismatch at query 0"})      # a changed root
    want = len(proof)
    check(root, claims, proof + b"\0", {"pcs: the opening has %d bytes, %d expected" % (want + 1, want)})
    check(root, claims, proof[:-1], {"pcs: the opening has %d bytes, %d expected" % (want - 1, want)})
    # a word >= p, in an element (ahead of the evaluation check it would also fail) and in a column
    for at in (16 * Cn + 16, cols_at + qb + 8 * 2):
        bad = proof[:at] + (P).to_bytes(8, "big") + proof[at + 8:]
        check(root, claims, bad, {"pcs: non-canonical word at byte %d" % at})
    bad = proof[:8] + b"\xff" * 8 + proof[16:]
    check(root, claims, bad, {"pcs: non-canonical word at byte 8"})


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_a_wrong_value_is_refused_by_the_prover_naming_the_claim():
    c = c2_case(15)
    bad = list(c["claims"])
    t, pt, v = bad[1]
    bad[1] = (t, pt, (v[0], (v[1] + 1) % P))
    with pytest.raises(hg.HgError, match=r"hg_pcs_open: claim 1\b"):
        c["cm"].open(bad, 5)
    assert c["cm"].open(c["claims"], 5) == c["open35"]     # the handle still opens


def test_bad_arguments_are_errors_naming_the_function():
    L = hg._pcs_protos()
    c = c2_case(15)
    nvars, tables, cm = c["nvars"], c["tables"], c["cm"]
    ptrs = (hg.u64p * 4)(*[hg._ptr(t) for t in tables])
    nv = (C.c_uint32 * 4)(*nvars)
    h, root = C.c_void_p(), (C.c_uint8 * 32)()
    # c > v_t, null arguments, a null table, no table
    for args in ((None, ptrs, nv, 4, 3, C.byref(h), root), (None, None, nv, 4, 2, C.byref(h), root), (None, ptrs, None, 4, 2, C.byref(h), root),
                 (None, ptrs, nv, 4, 2, None, root), (None, ptrs, nv, 4, 2, C.byref(h), None), (None, ptrs, nv, 0, 2, C.byref(h), root),
                 (None, (hg.u64p * 4)(ptrs[0], None, ptrs[2], ptrs[3]), nv, 4, 2, C.byref(h), root)):
        assert L.hg_pcs_commit(*args) == -1 and "hg_pcs_commit" in _last(), args
        assert not h.value
    bad = [t.copy() for t in tables]
    bad[2][3] = P                                                # a word that is not below p
    with pytest.raises(hg.HgError, match="hg_pcs_commit"):
        hg.Commitment.commit(None, bad, 2)
    table, pts, vals = hg._pcs_claim_arrays(c["claims"])
    buf, ln = (C.c_uint8 * len(c["open35"]))(), C.c_size_t(0)
    good = (None, cm.h, table, hg._ptr(pts), hg._ptr(vals), 3, 5, buf, len(buf), C.byref(ln))

    def sub(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    far = (C.c_uint32 * 3)(0, 4, 2)                              # a table index out of range
    big = pts.copy()
    big[1] = P                                                   # a non-canonical coordinate
    for args in (sub(good, 1, None), sub(good, 2, None), sub(good, 3, None), sub(good, 4, None), sub(good, 7, None), sub(good, 9, None), sub(good, 2, far),
                 sub(good, 3, hg._ptr(big)), sub(good, 8, len(buf) - 1), sub(good, 6, 1 << 20)):
        assert L.hg_pcs_open(*args) == -1 and "hg_pcs_open" in _last(), args
    assert L.hg_pcs_open(*good) == 0 and bytes(buf) == c["open35"]
    proof = c["open35"]
    vgood = (cm.root, nv, 4, 2, table, hg._ptr(pts), hg._ptr(vals), 3, 5, proof, len(proof))
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 4, None), sub(vgood, 5, None), sub(vgood, 6, None), sub(vgood, 9, None), sub(vgood, 4, far),
                 sub(vgood, 3, 3), sub(vgood, 2, 0), sub(vgood, 2, 65), sub(vgood, 5, hg._ptr(big)), sub(vgood, 8, 1 << 20)):
        assert L.hg_pcs_verify(*args) == -1 and "hg_pcs_verify" in _last(), args
    assert L.hg_pcs_verify(*vgood) == 0
    # the wrappers
    w = wrapper_case(1024, 1, 27)
    params, scm, cl = w["bfv"].params, w["cm"], w["claims"]
    obuf, oln = (C.c_uint8 * len(w["opening"]))(), C.c_size_t(0)
    for args in ((None, None, w["w"].h, 0, C.byref(h), root), (None, C.byref(params), None, 0, C.byref(h), root), (None, C.byref(params), w["w"].h, 0, None, root),
                 (None, C.byref(params), w["w"].h, 0, C.byref(h), None), (None, C.byref(params), w["w"].h, 11, C.byref(h), root),
                 (None, C.byref(hg.params_builtin(2048, 1)), w["w"].h, 0, C.byref(h), root)):
        assert L.hg_secrets_commit(*args) == -1 and "hg_secrets_commit" in _last(), args
    ogood = (None, C.byref(params), scm.h, cl.claims, cl.n, hg._ptr(cl.points), 0, obuf, len(obuf), C.byref(oln))
    vgood = (C.byref(params), scm.root, 0, cl.claims, cl.n, hg._ptr(cl.points), 0, w["opening"], len(w["opening"]))
    public = (hg.HgInputClaim * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3                                          # a claim on ais[0]: settled inside hg_verify_public, never opened
    short = (hg.HgInputClaim * cl.n)(*cl.claims[:cl.n])
    short[0].nvars -= 1
    for args in (sub(ogood, 1, None), sub(ogood, 2, None), sub(ogood, 3, None), sub(ogood, 5, None), sub(ogood, 7, None), sub(ogood, 9, None), sub(ogood, 3, public),
                 sub(ogood, 3, short), sub(ogood, 2, cm.h), sub(ogood, 1, C.byref(hg.params_builtin(2048, 1)))):
        assert L.hg_claims_open(*args) == -1 and "hg_claims_open" in _last(), args
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 3, None), sub(vgood, 5, None), sub(vgood, 7, None), sub(vgood, 3, public), sub(vgood, 3, short),
                 sub(vgood, 2, 12)):
        assert L.hg_claims_verify(*args) == -1 and "hg_claims_verify" in _last(), args
    assert L.hg_claims_verify(*vgood) == 0


# ---- 6. the wrappers over the secret inputs --------------------------------------------------------------------------------------
_WRAP = {}


def wrapper_case(n, k, bits):
    """per shape: fixture witness, the oracle's mode-3 proof, the claims hg_verify_public leaves, host commitment and opening (defaults)"""
    if (n, k) not in _WRAP:
        bfv = hg.BfvEncrypt.new(n, k)
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        d = w.arrays()
        proof = orclib.prove_f("goldilocks", orclib.params(n, k), orclib.Inputs(d), threads=8, mode=3)[0]
        pk = bfv.setup(None)
        ok, why, claims = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 3)
        assert ok, why
        cm = hg.Commitment.secrets(None, bfv.params, w)
        _WRAP[(n, k)] = dict(bfv=bfv, pk=pk, w=w, d=d, proof=proof, claims=claims, cm=cm, opening=cm.open_claims(bfv.params, claims))
    return _WRAP[(n, k)]


@pytest.mark.parametrize("n,k,bits", WRAPPER_SHAPES)
def test_claims_of_hg_verify_public_are_opened_and_verified(n, k, bits):
    c = wrapper_case(n, k, bits)
    params, cl = c["bfv"].params, c["claims"]
    lg = n.bit_length() - 1
    nvars = [lg + 1] * (3 + k) + [lg + k.bit_length() - 1]
    assert c["cm"].nvars == nvars
    assert len(c["opening"]) == hg.pcs_opening_bytes(nvars, cl.n) == opening_len(nvars, hg.pcs_row_log2(nvars), cl.n, 241)
    assert hg.claims_verify(params, c["cm"].root, cl, c["opening"]) == (True, "")
    assert hg.claims_settle(None, params, c["w"], cl) == (True, "")
    # the same bytes through the generic layer: tables in input order, ids mapped 0 1 2 -> 0 1 2, 3+k+i -> 3+i, 3+2k -> 3+k
    sz = 2 * n
    tables = [c["d"]["s"], c["d"]["e"], c["d"]["k1"]] + [c["d"]["r1is"][i * sz:(i + 1) * sz] for i in range(k)] + [c["d"]["r2is"]]
    generic = hg.Commitment.commit(None, tables)
    assert generic.root == c["cm"].root
    mapped = [(i if i < 3 else i - k, list(pt), v) for i, _, pt, v in cl.as_tuples()]
    assert generic.open(mapped) == c["opening"]
    # a flipped byte in the last sibling
    bad = bytearray(c["opening"])
    bad[-1] ^= 1
    assert hg.claims_verify(params, c["cm"].root, cl, bytes(bad)) == (False, "pcs: Merkle path mismatch at query 240")


@pytest.mark.parametrize("n,k,bits", WRAPPER_SHAPES)
def test_an_opening_from_another_witness_does_not_verify(n, k, bits):
    """one changed word of s: hg_claims_open refuses (a claim on s is no longer the table's value), or the opening is rejected
    against the honest root"""
    c = wrapper_case(n, k, bits)
    d = {f: v.copy() for f, v in c["d"].items()}
    d["s"][0] = (int(d["s"][0]) + 1) % P
    other = hg.Commitment.secrets(None, c["bfv"].params, hg.Witness.from_arrays(c["bfv"].params, d))
    assert other.root != c["cm"].root
    try:
        forged = other.open_claims(c["bfv"].params, c["claims"])
    except hg.HgError as e:
        assert re.search(r"hg_claims_open: claim \d+\b", str(e))
        return
    ok, why = hg.claims_verify(c["bfv"].params, c["cm"].root, c["claims"], forged)
    assert not ok and why.startswith("pcs: ")


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def device_equals_host(ctx, tables, log2_row, seed):
    host = hg.Commitment.commit(None, tables, log2_row)
    dev = hg.Commitment.commit(ctx, tables, log2_row)
    assert dev.root == host.root
    claims = make_claims(tables, 3, seed)
    for cl, Q in ((claims, 5), ([], 1)):
        proof = dev.open(cl, Q)
        assert proof == host.open(cl, Q)
        assert hg.pcs_verify(host.root, host.nvars, cl, proof, Q, log2_row) == (True, "")
    return host, dev


@pytest.mark.gpu
@pytest.mark.parametrize("R,nvars", C2_SHAPES)
def test_device_form_equals_the_host_form_radix2_path(ctx, R, nvars):
    c = c2_case(R)
    dev = hg.Commitment.commit(ctx, c["tables"], 2)
    assert dev.root == c["cm"].root == c["py"].root
    assert dev.open(c["claims"], 5) == c["open35"] and dev.open([], 1) == c["open01"]


@pytest.mark.gpu
@pytest.mark.parametrize("nvars", [[8, 7, 6], [11]])
def test_device_form_equals_the_host_form_four_step_path(ctx, nvars):
    """c = 6: the encoding is the LDS four-step NTT of size 256; R = 7 (one Keccak block) and R = 32 (two)"""
    device_equals_host(ctx, make_tables(nvars, 0x6c6 + len(nvars)), 6, 5)


@pytest.mark.gpu
def test_a_non_canonical_word_is_refused_by_the_device_form(ctx):
    bad = make_tables([6, 2], 3)
    bad[0][63] = P
    with pytest.raises(hg.HgError, match="hg_pcs_commit"):
        hg.Commitment.commit(ctx, bad, 2)
    host = hg.Commitment.commit(None, make_tables([6, 2], 3), 2)
    with pytest.raises(hg.HgError, match="hg_pcs_open"):       # a host-form handle opened with a context
        hg._check(hg._pcs_protos().hg_pcs_open(ctx.h, host.h, None, None, None, 0, 1, (C.c_uint8 * 4096)(), 4096, C.byref(C.c_size_t(0))))


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
def test_wrappers_on_the_device_equal_the_host_form(ctx, n, k):
    bfv = hg.BfvEncrypt.new(n, k)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x9c5 + n)
    proof, _ = bfv.prove(ctx, pk, w, mode=3)
    ok, why, cl = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 3, ctx=ctx, device=True)
    assert ok, why
    host, dev = hg.Commitment.secrets(None, bfv.params, w), hg.Commitment.secrets(ctx, bfv.params, w)
    assert dev.root == host.root
    opening = dev.open_claims(bfv.params, cl)
    assert opening == host.open_claims(bfv.params, cl)
    assert len(opening) == hg.pcs_opening_bytes(host.nvars, cl.n)
    assert hg.claims_verify(bfv.params, host.root, cl, opening) == (True, "")
    pk.free()


@pytest.mark.gpu
def test_headline_size_once(ctx):
    """(32768,16), a synthetic witness, the 47 claims of hg_verify_public_device on its proof: c = 11, R = 864, four-step NTT of 2^13"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x8000 + 16)
    proof, _ = bfv.prove(ctx, pk, w, cap=1 << 25)
    ok, why, cl = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 0, ctx=ctx, device=True)
    assert ok, why
    assert cl.n == 47
    dev = hg.Commitment.secrets(ctx, bfv.params, w)
    assert dev.log2_row == 11
    opening = dev.open_claims(bfv.params, cl)
    assert len(opening) == hg.pcs_opening_bytes(dev.nvars, 47) == 16 * 2048 * 48 + 241 * (8 * 864 + 32 * 13)
    assert hg.claims_verify(bfv.params, dev.root, cl, opening) == (True, "")
    assert hg.Commitment.secrets(None, bfv.params, w).root == dev.root
    pk.free()


def signed(words):
    w = np.asarray(words, dtype=np.uint64)
    out = w.astype(np.int64)
    neg = w > np.uint64(P // 2)
    out[neg] = -((np.uint64(P) - w[neg]).astype(np.int64))
    return out


@pytest.mark.gpu
def test_end_to_end_on_the_device(ctx):
    """hg_prove_encryptions of two encryptions -> hg_verify_public_device -> hg_secrets_commit -> hg_claims_open -> hg_claims_verify"""
    n, k = 1024, 1
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    encs = []
    for seed in (21, 22):
        d = hg.Witness.synthetic(bfv.params, seed).arrays()
        encs.append((signed(d["s"][:n])[::-1], signed(d["e"][n - 1:2 * n - 1])[::-1], signed(d["k1"][n - 1:2 * n - 1])[::-1], signed(d["ais"][:n])[::-1].reshape(1, n)))
    proofs, status, why, ws, _ = hg.prove_encryptions(ctx, pk, encs)
    assert status == [0, 0], why
    roots, claims, openings = [], [], []
    for i in range(2):
        ok, reason, cl = hg.verify_public(pk, hg.Instance.from_witness(ws[i]), proofs[i], 0, ctx=ctx, device=True)
        assert ok, reason
        cm = hg.Commitment.secrets(ctx, bfv.params, ws[i])
        roots.append(cm.root)
        claims.append(cl)
        openings.append(cm.open_claims(bfv.params, cl))
        assert hg.claims_verify(bfv.params, cm.root, cl, openings[i]) == (True, "")
    assert roots[0] != roots[1]
    ok, reason = hg.claims_verify(bfv.params, roots[1], claims[0], openings[0])
    assert not ok and reason.startswith("pcs: ")
    pk.free()
