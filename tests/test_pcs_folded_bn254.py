"""hg_pcs_open_folded_bn254 / hg_pcs_verify_folded_bn254 / hg_pcs_verify_folded_device_bn254 and the hg_claims_*_folded_bn254 wrappers:
the folded openings of test_pcs_folded.py over bn256::Fr. The yardstick is py_verify_folded_bn254, the verifier of the section "Folded
openings over BN254" of include/hg.h restated in Python integers (its own transcript with the new tag, the rounds, the final
evaluation, the combined row, the queries; the code and the tree as test_pcs_bn254.py restates them): host openings must be accepted by
it, every tampered input must get the same documented reason from it and from the C verifier, the device forms must equal the host
forms byte for byte and reason for reason."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import orclib
from hglib import hg, ROOT
from test_pcs_bn254 import R, PyCommit, dot, encode, eq_table, make_tables, py_mle, py_verify, repr_, wrapper_case

NEW = ["hg_pcs_open_folded_bn254", "hg_pcs_verify_folded_bn254", "hg_pcs_verify_folded_device_bn254", "hg_claims_open_folded_bn254", "hg_claims_verify_folded_bn254",
       "hg_claims_verify_folded_device_bn254"]
Q = 5
# name -> (nvars, c, the tables of the claims): the shapes of test_pcs_folded.py. unequal: tables of unequal size (the (1 - X) tail), table 2
# without a claim and a single row (v_t = c), two claims on tables 0 and 1. single: one table, one row, one claim. mid: three sizes
SHAPES = {"unequal": ([4, 3, 2, 4], 2, [0, 1, 1, 3, 0]), "single": ([3], 3, [0]), "mid": ([8, 7, 6], 4, [0, 1, 2, 0])}
# larger ones for the device form: the four-step NTT sizes, more than one workgroup a table in the first rounds
DEVICE_SHAPES = dict(SHAPES, eleven=([11], 5, [0, 0, 0]), twelve=([12, 12, 9], 6, [0, 1, 2, 1, 0]))
ROUND = "pcs: fold round %d does not match the running claim"
FINAL = "pcs: fold final evaluation mismatch"
EVAL0 = "pcs: evaluation mismatch at claim 0"


def claims_on(tables, which, seed):
    """one claim per entry of `which` (a table index) at a random point with the table's value: [(table, point, value)]"""
    rng = random.Random(seed)
    out = []
    for t in which:
        pt = [rng.randrange(R) for _ in range(len(tables[t]).bit_length() - 1)]
        out.append((t, pt, py_mle(tables[t], pt)))
    return out


def folded_len(nvars, c, Qn):
    return 32 * (3 * max(nvars) + len(nvars)) + 64 * (1 << c) + Qn * (32 * sum(1 << (v - c) for v in nvars) + 32 * (c + 2))


class FoldTranscript:
    """the absorbing transcript of a folded BN254 opening: "hg-pcs-bn254-fold-1", then what "hg-pcs-bn254-1" appends after its tag"""

    def __init__(self, root, c, nvars, Qn, claims):
        le32 = lambda x: int(x).to_bytes(4, "little")   # noqa: E731
        self.pending = b"hg-pcs-bn254-fold-1" + root + le32(c) + le32(len(nvars)) + b"".join(le32(v) for v in nvars) + le32(Qn) + le32(len(claims))
        for t, pt, val in claims:
            self.pending += le32(t) + b"".join(repr_(x) for x in pt) + repr_(val)

    def squeeze(self):
        self.pending = orclib.keccak256(self.pending)
        return int.from_bytes(self.pending, "little") % R

    def absorb(self, x):
        self.pending += repr_(x)


def py_verify_folded_bn254(root, nvars, c, claims, Qn, proof):
    """the verifier of "Folded openings over BN254" in include/hg.h, checks in the documented order; "" or the documented reason"""
    Cn, N, m, V, n = 1 << c, 4 << c, len(nvars), max(nvars), len(claims)
    Rn = sum(1 << (v - c) for v in nvars)
    off = [sum(1 << (v - c) for v in nvars[:t]) for t in range(m)]
    hb, qb = 32 * (3 * V + m), 32 * Rn + 32 * (c + 2)
    # 1. the exact length
    if len(proof) != folded_len(nvars, c, Qn):
        return "pcs: the opening has %d bytes, %d expected" % (len(proof), folded_len(nvars, c, Qn))
    # 2. every element below r, the lowest offset: the header, then u, then the columns query by query
    elem = lambda at: int.from_bytes(proof[at:at + 32], "big")   # noqa: E731
    cols_at = hb + 64 * Cn
    for at in [32 * i for i in range(cols_at // 32)] + [cols_at + q * qb + 32 * r for q in range(Qn) for r in range(Rn)]:
        if elem(at) >= R:
            return "pcs: non-canonical word at byte %d" % at
    tr = FoldTranscript(root, c, nvars, Qn, claims)
    beta = tr.squeeze()
    bpow = [pow(beta, i, R) for i in range(n)]
    claim = sum(b * val for b, (_, _, val) in zip(bpow, claims)) % R
    # 3. the rounds
    rho = []
    for j in range(V):
        c0, c1, c2 = (elem(32 * (3 * j + k)) for k in range(3))
        if (2 * c0 + c1 + c2) % R != claim:
            return ROUND % j
        for x in (c0, c1, c2):
            tr.absorb(x)
        r = tr.squeeze()
        rho.append(r)
        claim = (c0 + r * (c1 + r * c2)) % R
    # 4. the final evaluation
    Y = [elem(32 * (3 * V + t)) for t in range(m)]
    for y in Y:
        tr.absorb(y)
    fin = 0
    for t in range(m):
        g = 0
        for i, (ti, pt, _) in enumerate(claims):
            if ti == t:
                e = bpow[i]
                for z, r in zip(pt, rho):     # eq(z, r) = z r + (1 - z)(1 - r) per coordinate
                    e = e * (z * r + (1 - z) * (1 - r)) % R
                g += e
        term = Y[t] * g
        for j in range(nvars[t], V):
            term = term * (1 - rho[j]) % R
        fin = (fin + term) % R
    if fin != claim:
        return FINAL
    # 5. the combined row at rho[..c)
    delta = tr.squeeze()
    rho_p = tr.squeeze()
    u = [[elem(hb + 32 * (i * Cn + j)) for j in range(Cn)] for i in range(2)]
    dpow = [pow(delta, t, R) for t in range(m)]
    if dot(eq_table(rho[:c]), u[1]) != dot(dpow, Y):
        return EVAL0
    for ui in u:
        for x in ui:
            tr.absorb(x)
    js = [(tr.squeeze() & 0xFFFFFFFFFFFFFFFF) & (N - 1) for _ in range(Qn)]
    # 6. the queries
    rho_pw = [pow(rho_p, r, R) for r in range(Rn)]
    w = [None] * Rn
    for t in range(m):
        for r, e in enumerate(eq_table(rho[c:nvars[t]])):
            w[off[t] + r] = dpow[t] * e % R
    enc = [encode(ui, c) for ui in u]
    for q in range(Qn):
        base = cols_at + q * qb
        col = [elem(base + 32 * r) for r in range(Rn)]
        h, idx = orclib.keccak256((0).to_bytes(8, "little") + b"".join(repr_(x) for x in col)), js[q]
        for lv in range(c + 2):
            sib = proof[base + 32 * Rn + 32 * lv:base + 32 * Rn + 32 * (lv + 1)]
            h = orclib.keccak256((1).to_bytes(8, "little") + (sib + h if idx & 1 else h + sib))
            idx >>= 1
        if h != root:
            return "pcs: Merkle path mismatch at query %d" % q
        if dot(rho_pw, col) != enc[0][js[q]]:
            return "pcs: proximity mismatch at query %d" % q
        if dot(w, col) != enc[1][js[q]]:
            return "pcs: claim 0 inconsistent at query %d" % q
    return ""


# ---- cases (computed once, never changed) ----------------------------------------------------------------------------------------
_CASES = {}


def case(name):
    """per shape: tables, claims, the host commitment, its folded opening"""
    if name not in _CASES:
        nvars, c, which = DEVICE_SHAPES[name]
        tables = make_tables(nvars, 0xf01d + len(name))
        cm = hg.Commitment.commit_bn254(None, tables, log2_row=c)
        claims = claims_on(tables, which, 31 + len(name))
        _CASES[name] = dict(nvars=nvars, c=c, tables=tables, cm=cm, claims=claims, proof=cm.open_folded(claims, Q))
    return _CASES[name]


def py_root(name):
    c = case(name)
    if "py" not in c:
        c["py"] = PyCommit(c["tables"], c["c"])
    return c["py"].root


def _last():
    return hg.lib().hg_last_error().decode()


_TAMPER = {}


def tamper_set(name):
    """[(label, root, claims, proof, allowed reasons)] for one shape, made once"""
    if name in _TAMPER:
        return _TAMPER[name]
    c = case(name)
    nvars, cc, claims, proof, root = c["nvars"], c["c"], c["claims"], c["proof"], c["cm"].root
    Cn, m, V = 1 << cc, len(nvars), max(nvars)
    Rn = sum(1 << (v - cc) for v in nvars)
    hb, qb = 32 * (3 * V + m), 32 * Rn + 32 * (cc + 2)
    cols_at = hb + 64 * Cn
    path0 = {"pcs: Merkle path mismatch at query 0", "pcs: proximity mismatch at query 0"}   # the indices move with the transcript
    early = {ROUND % 0, ROUND % 1}   # with one claim S = y whatever beta is: round 0 still holds, round 1 does not

    def flip(at, src=proof):
        """one bit of one byte changed: the byte at `at`, or in a field element (every use but the siblings') the first bit from there on,
        going round the element, that leaves it below r (byte 0 of a big-endian element stays at most 0x30)"""
        b = bytearray(src)
        if at >= cols_at and (at - cols_at) % qb >= 32 * Rn:
            b[at] ^= 0x01
            return bytes(b)
        e0 = at & ~31
        for k in range(32):
            for bit in range(8):
                b[e0:e0 + 32] = src[e0:e0 + 32]
                b[e0 + (at - e0 + k) % 32] ^= 1 << bit
                if int.from_bytes(b[e0:e0 + 32], "big") < R:
                    assert b[e0] <= 0x30
                    return bytes(b)
        raise AssertionError("no canonical neighbour")

    def setr(at, src=proof):
        return src[:at] + R.to_bytes(32, "big") + src[at + 32:]

    out = []
    for k in range(3):                                                         # c0 of round 0, c1 of round 1, c2 of the last round
        j = (0, 1, V - 1)[k]
        out.append(("c%d of round %d" % (k, j), root, claims, flip(32 * (3 * j + k) + 31), {ROUND % j}))
    out.append(("Y_0", root, claims, flip(32 * 3 * V + 31), {FINAL}))
    if name == "unequal":                                                      # g_2 = 0: the final evaluation holds, the combined row's value does not
        out.append(("Y of the claimless table", root, claims, flip(32 * (3 * V + 2) + 31), {EVAL0}))
    out.append(("u_0", root, claims, flip(hb + 32 + 31), path0))
    out.append(("u_1", root, claims, flip(hb + 32 * Cn + 32 + 31), {EVAL0}))
    for q in (0, 3):
        out.append(("column element, query %d" % q, root, claims, flip(cols_at + q * qb + 32 * (Rn - 1) + 31), {"pcs: Merkle path mismatch at query %d" % q}))
        out.append(("sibling, query %d" % q, root, claims, flip(cols_at + q * qb + 32 * Rn + 32 + 9), {"pcs: Merkle path mismatch at query %d" % q}))
    for label, at in (("header", 32 * 3 * V), ("first header element", 0), ("u", hb + 32 * Cn), ("column", cols_at + qb + 32 * (Rn - 1))):
        out.append(("r in the " + label, root, claims, setr(at), {"pcs: non-canonical word at byte %d" % at}))
    want = len(proof)
    out.append(("extended", root, claims, proof + b"\0", {"pcs: the opening has %d bytes, %d expected" % (want + 1, want)}))
    out.append(("truncated", root, claims, proof[:-1], {"pcs: the opening has %d bytes, %d expected" % (want - 1, want)}))
    t, pt, v = claims[0]
    out.append(("claim value", root, [(t, pt, (v + 1) % R)] + claims[1:], proof, {ROUND % 0}))
    out.append(("claim point", root, [(t, [(pt[0] + 1) % R] + pt[1:], v)] + claims[1:], proof, early))
    out.append(("root", bytes([root[0] ^ 1]) + root[1:], claims, proof, early))
    # two failures at once: the order of the checks decides
    out.append(("column r and round 1", root, claims, setr(cols_at + 32 * (Rn - 1), flip(32 * 3 + 31)), {"pcs: non-canonical word at byte %d" % (cols_at + 32 * (Rn - 1))}))
    out.append(("round 0 and u_1", root, claims, flip(hb + 32 * Cn + 31, flip(31)), {ROUND % 0}))
    out.append(("u_1 and a sibling", root, claims, flip(hb + 32 * Cn + 31, flip(cols_at + 32 * Rn + 3)), {EVAL0}))
    _TAMPER[name] = out
    return out


# ---- 1. surface ------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name


# ---- 2. host openings ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_openings_have_the_documented_length_and_are_accepted(name):
    c = case(name)
    nvars, cc = c["nvars"], c["c"]
    assert c["cm"].root == py_root(name)
    assert {0, 1, R - 1, R - 2} <= set(x for t in c["tables"] for x in t)      # the edge elements occur
    assert len(c["proof"]) == folded_len(nvars, cc, Q) == hg.pcs_folded_opening_bytes_bn254(nvars, Q, cc)
    assert py_verify_folded_bn254(c["cm"].root, nvars, cc, c["claims"], Q, c["proof"]) == ""
    assert hg.pcs_verify_folded_bn254(c["cm"].root, nvars, c["claims"], c["proof"], Q, cc) == (True, "")
    # the length does not grow with the claims
    assert len(c["cm"].open_folded(c["claims"] + c["claims"][:1], Q)) == len(c["proof"])


def test_a_table_of_one_element_is_a_scalar_from_the_start():
    nvars = [2, 0]
    tables = make_tables(nvars, 0x51)
    cm = hg.Commitment.commit_bn254(None, tables, log2_row=0)
    assert cm.log2_row == 0
    claims = claims_on(tables, [1, 0, 1], 3)
    proof = cm.open_folded(claims, Q)
    assert len(proof) == folded_len(nvars, 0, Q)
    assert py_verify_folded_bn254(cm.root, nvars, 0, claims, Q, proof) == ""
    assert hg.pcs_verify_folded_bn254(cm.root, nvars, claims, proof, Q, 0) == (True, "")


# ---- 3. tampering ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tampered_openings_get_the_documented_reason_from_both_verifiers(name):
    c = case(name)
    for label, root, claims, proof, allowed in tamper_set(name):
        ok, why = hg.pcs_verify_folded_bn254(root, c["nvars"], claims, proof, Q, c["c"])
        assert not ok and why in allowed, (label, why, allowed)
        assert why == py_verify_folded_bn254(root, c["nvars"], c["c"], claims, Q, proof), label


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------
def test_a_wrong_value_is_refused_by_the_prover_naming_the_claim_and_the_function():
    c = case("unequal")
    for i in (2, 4):
        bad = list(c["claims"])
        t, pt, v = bad[i]
        bad[i] = (t, pt, (v + 1) % R)
        with pytest.raises(hg.HgError, match=r"hg_pcs_open_folded_bn254: claim %d: the value is not the evaluation of table %d at the point" % (i, t)):
            c["cm"].open_folded(bad, Q)
    bad = [(t, pt, (v + 1) % R) for t, pt, v in c["claims"]]                      # every value wrong: the lowest is named
    with pytest.raises(hg.HgError, match=r"hg_pcs_open_folded_bn254: claim 0\b"):
        c["cm"].open_folded(bad, Q)
    assert c["cm"].open_folded(c["claims"], Q) == c["proof"]                      # the handle still opens


def folded_wrapper(n, k, bits):
    if (n, k) not in _FOLDED_WRAP:
        w = wrapper_case(n, k, bits)
        _FOLDED_WRAP[(n, k)] = w["cm"].open_claims_folded(w["bfv"].params, w["claims"])
    return _FOLDED_WRAP[(n, k)]


_FOLDED_WRAP = {}


def test_bad_arguments_are_errors_naming_the_function():
    L = hg.lib()
    c = case("unequal")
    nvars, cm, proof = c["nvars"], c["cm"], c["proof"]
    nv = (C.c_uint32 * 4)(*nvars)
    table, pts, vals = hg._pcs_claim_arrays_bn254(c["claims"])
    n = len(c["claims"])
    buf, ln = (C.c_uint8 * len(proof))(), C.c_size_t(0)
    good = (None, cm.h, table, hg._ptr(pts), hg._ptr(vals), n, Q, buf, len(buf), C.byref(ln))

    def sub(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    far = (C.c_uint32 * n)(0, 4, 1, 3, 0)                          # a table index out of range
    big = pts.copy()
    big[4:8] = hg.Context._fr_pack([R])                            # a non-canonical coordinate
    bigv = vals.copy()
    bigv[0:4] = hg.Context._fr_pack([R])                           # a non-canonical value
    for args in (sub(good, 1, None), sub(good, 2, None), sub(good, 3, None), sub(good, 4, None), sub(good, 7, None), sub(good, 9, None), sub(good, 2, far),
                 sub(good, 3, hg._ptr(big)), sub(good, 4, hg._ptr(bigv)), sub(good, 6, 1 << 20)):
        assert L.hg_pcs_open_folded_bn254(*args) == -1 and "hg_pcs_open_folded_bn254" in _last(), args
    assert L.hg_pcs_open_folded_bn254(*sub(good, 5, 0)) == -1 and _last() == "hg_pcs_open_folded_bn254: a folded opening needs a claim"
    ln.value = 0
    assert L.hg_pcs_open_folded_bn254(*sub(good, 8, len(buf) - 1)) == -1 and "hg_pcs_open_folded_bn254" in _last() and ln.value == len(proof)   # *len reports the need
    assert L.hg_pcs_open_folded_bn254(*good) == 0 and bytes(buf) == proof and ln.value == len(proof)
    vgood = (cm.root, nv, 4, 2, table, hg._ptr(pts), hg._ptr(vals), n, Q, proof, len(proof))
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 4, None), sub(vgood, 5, None), sub(vgood, 6, None), sub(vgood, 9, None), sub(vgood, 4, far),
                 sub(vgood, 3, 3), sub(vgood, 2, 0), sub(vgood, 2, 65), sub(vgood, 5, hg._ptr(big)), sub(vgood, 6, hg._ptr(bigv)), sub(vgood, 8, 1 << 20)):
        assert L.hg_pcs_verify_folded_bn254(*args) == -1 and "hg_pcs_verify_folded_bn254" in _last(), args
    assert L.hg_pcs_verify_folded_bn254(*sub(vgood, 7, 0)) == -1 and _last() == "hg_pcs_verify_folded_bn254: a folded opening needs a claim"
    assert L.hg_pcs_verify_folded_bn254(*vgood) == 0
    assert L.hg_pcs_verify_folded_device_bn254(None, *vgood) == -1 and _last() == "hg_pcs_verify_folded_device_bn254: no context"
    # a Goldilocks handle; the Goldilocks entry keeps refusing a BN254 handle
    gl = hg.Commitment.commit(None, [np.arange(1 << v, dtype=np.uint64) for v in nvars], 2)
    assert L.hg_pcs_open_folded_bn254(*sub(good, 1, gl.h)) == -1 and "hg_pcs_open_folded_bn254" in _last() and "Goldilocks" in _last()
    assert L.hg_pcs_open_folded(*sub(good, 1, cm.h)) == -1 and "hg_pcs_open_folded" in _last() and "BN254" in _last()
    # the wrappers
    w = wrapper_case(1024, 1, 27)
    params, scm, cl = w["bfv"].params, w["cm"], w["claims"]
    cap = hg.pcs_folded_opening_bytes_bn254(scm.nvars)
    obuf, oln = (C.c_uint8 * cap)(), C.c_size_t(0)
    ogood = (None, C.byref(params), scm.h, cl.claims, cl.n, hg._ptr(cl.points), 0, obuf, cap, C.byref(oln))
    public = (hg.HgInputClaimBn254 * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3                                            # a claim on ais[0]: settled inside hg_verify_public_bn254, never opened
    glsec = hg.Commitment.secrets(None, params, w["w"])            # the Goldilocks commitment of the same witness
    for args in (sub(ogood, 1, None), sub(ogood, 2, None), sub(ogood, 3, None), sub(ogood, 5, None), sub(ogood, 7, None), sub(ogood, 9, None), sub(ogood, 3, public),
                 sub(ogood, 2, cm.h), sub(ogood, 2, glsec.h), sub(ogood, 4, 0), sub(ogood, 1, C.byref(hg.params_builtin(2048, 1)))):
        assert L.hg_claims_open_folded_bn254(*args) == -1 and "hg_claims_open_folded_bn254" in _last(), args
    opening = folded_wrapper(1024, 1, 27)
    assert L.hg_claims_open_folded_bn254(*ogood) == 0 and bytes(obuf) == opening
    vgood = (C.byref(params), scm.root, 0, cl.claims, cl.n, hg._ptr(cl.points), 0, opening, len(opening))
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 3, None), sub(vgood, 5, None), sub(vgood, 7, None), sub(vgood, 3, public), sub(vgood, 2, 12),
                 sub(vgood, 4, 0)):
        assert L.hg_claims_verify_folded_bn254(*args) == -1 and "hg_claims_verify_folded_bn254" in _last(), args
    assert L.hg_claims_verify_folded_bn254(*vgood) == 0
    assert L.hg_claims_verify_folded_device_bn254(None, *vgood) == -1 and _last() == "hg_claims_verify_folded_device_bn254: no context"


# ---- 5. layouts ------------------------------------------------------------------------------------------------------------------
def test_the_two_forms_of_opening_reject_each_other():
    """by the length rule or by the first check that reads the other layout, never a crash"""
    for name in sorted(SHAPES):
        c = case(name)
        nvars, cc, claims, root = c["nvars"], c["c"], c["claims"], c["cm"].root
        plain = c["cm"].open(claims, Q)
        ok, why = hg.pcs_verify_folded_bn254(root, nvars, claims, plain, Q, cc)
        assert not ok and why == py_verify_folded_bn254(root, nvars, cc, claims, Q, plain) and why.startswith("pcs: "), why
        ok, why = hg.pcs_verify_bn254(root, nvars, claims, c["proof"], Q, cc)
        assert not ok and why == py_verify(root, nvars, cc, claims, Q, c["proof"]) and why.startswith("pcs: "), why


# ---- 6. the wrappers over the secret inputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,bits", [(1024, 1, 27), (4096, 2, 55)])
def test_claims_of_hg_verify_public_bn254_are_opened_folded_and_verified(n, k, bits):
    c = wrapper_case(n, k, bits)
    params, cl = c["bfv"].params, c["claims"]
    opening = folded_wrapper(n, k, bits)
    nvars = c["cm"].nvars
    assert len(opening) == hg.pcs_folded_opening_bytes_bn254(nvars) == folded_len(nvars, hg.pcs_row_log2(nvars), 241) < len(c["opening"])
    assert hg.claims_verify_folded_bn254(params, c["cm"].root, cl, opening) == (True, "")
    assert hg.claims_verify_bn254(params, c["cm"].root, cl, opening)[0] is False
    # the same bytes through the generic layer
    mapped = [(i if i < 3 else i - k, list(hg.Context._fr_unpack(np.array(pt, dtype=np.uint64))), hg.Context._fr_unpack(np.array(v, dtype=np.uint64))[0])
              for i, _, pt, v in cl.as_tuples()]
    assert hg.pcs_verify_folded_bn254(c["cm"].root, nvars, mapped, opening) == (True, "")
    bad = bytearray(opening)
    bad[-1] ^= 1                                                   # the last sibling
    assert hg.claims_verify_folded_bn254(params, c["cm"].root, cl, bytes(bad)) == (False, "pcs: Merkle path mismatch at query 240")
    # an opening made from another witness: refused by the prover, or rejected against the honest root
    d = {f: v.copy() for f, v in c["d"].items()}
    d["s"][0] = (int(d["s"][0]) + 1) % orclib.P
    other = hg.Commitment.secrets_bn254(None, params, hg.Witness.from_arrays(params, d))
    try:
        forged = other.open_claims_folded(params, cl)
    except hg.HgError as e:
        assert re.search(r"hg_claims_open_folded_bn254: claim \d+\b", str(e))
        return
    ok, why = hg.claims_verify_folded_bn254(params, c["cm"].root, cl, forged)
    assert not ok and why.startswith("pcs: ")


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEVICE_SHAPES))
def test_device_form_equals_the_host_form(ctx, name):
    c = case(name)
    dev = hg.Commitment.commit_bn254(ctx, c["tables"], c["c"])
    assert dev.root == c["cm"].root
    assert dev.open_folded(c["claims"], Q) == c["proof"]
    assert hg.pcs_verify_folded_bn254(dev.root, c["nvars"], c["claims"], c["proof"], Q, c["c"], ctx=ctx) == (True, "")
    bad = list(c["claims"])
    t, pt, v = bad[-1]
    bad[-1] = (t, pt, (v + 1) % R)
    with pytest.raises(hg.HgError, match=r"hg_pcs_open_folded_bn254: claim %d\b" % (len(bad) - 1)):
        dev.open_folded(bad, Q)
    assert dev.open(c["claims"], Q) == c["cm"].open(c["claims"], Q)              # the raw rows are as they were


# A launch of the reduction has at most 2048 workgroups of 256 threads (HG_PCS_FOLD_BLOCKS lowers the bound), so on the shapes above a
# thread makes at most 8 trips. The round kernels restart their unreduced sums every 64 units (BNFOLD_TRIPS). With one workgroup a
# table, a table of 2^17 entries has 2^16 pairs in round 0: 2^16 / 256 = 256 trips a thread, four restarts; round 1 has 2^15 units of
# four entries: 128 trips, two restarts. v = 16 would give 64 trips in round 1, a single restart, so v = 17 is the smallest. The second
# table (2^14) makes the launch one over two tables of unequal size. The g builder restarts every 1024 claims of a table
# (BNFOLD_G_TRIPS): a second, tiny shape [6] carries 2100 claims on its one table, two restarts. The plan line shows that the rounds
# ran on the device.
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import test_pcs_folded_bn254 as T
from hglib import hg
ctx = hg.Context(0)
nvars, c = [17, 14], 8
tables = T.make_tables(nvars, 0xb17)
claims = T.claims_on(tables, [0, 1, 0], 8)
host = hg.Commitment.commit_bn254(None, tables, c)
dev = hg.Commitment.commit_bn254(ctx, tables, c)
assert dev.root == host.root
proof = dev.open_folded(claims, 5)
assert proof == host.open_folded(claims, 5)
assert hg.pcs_verify_folded_bn254(host.root, nvars, claims, proof, 5, c) == (True, "")
assert hg.pcs_verify_folded_bn254(host.root, nvars, claims, proof, 5, c, ctx=ctx) == (True, "")
print("FOLD OK")
nvars, c = [6], 3
tables = T.make_tables(nvars, 0xb06)
claims = T.claims_on(tables, [0] * 2100, 9)
host = hg.Commitment.commit_bn254(None, tables, c)
dev = hg.Commitment.commit_bn254(ctx, tables, c)
proof = dev.open_folded(claims, 5)
assert proof == host.open_folded(claims, 5)
assert hg.pcs_verify_folded_bn254(host.root, nvars, claims, proof, 5, c) == (True, "")
assert hg.pcs_verify_folded_bn254(host.root, nvars, claims, proof, 5, c, ctx=ctx) == (True, "")
print("G OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["1", "2048"])
def test_long_accumulations_and_the_plan_line(blocks):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, HG_DEBUG="plan", HG_PCS_FOLD_BLOCKS=blocks))
    assert r.returncode == 0 and "FOLD OK" in r.stdout and "G OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    plan = re.findall(r"\[hg plan\] bnpcsfold V=(\d+) dev_rounds=(\d+) host_rounds=(\d+) tables=(\d+) claims=(\d+)", r.stderr)
    assert plan == [("17", "17", "0", "2", "3"), ("6", "6", "0", "1", "2100")], r.stderr[-2000:]


@pytest.mark.gpu
def test_device_verifier_gives_the_host_decision_and_reason(ctx):
    c = case("unequal")
    for label, root, claims, proof, _ in tamper_set("unequal"):
        assert hg.pcs_verify_folded_bn254(root, c["nvars"], claims, proof, Q, c["c"], ctx=ctx) == hg.pcs_verify_folded_bn254(root, c["nvars"], claims, proof, Q, c["c"]), label
    plain = c["cm"].open(c["claims"], Q)
    assert hg.pcs_verify_folded_bn254(c["cm"].root, c["nvars"], c["claims"], plain, Q, c["c"], ctx=ctx) == hg.pcs_verify_folded_bn254(c["cm"].root, c["nvars"], c["claims"], plain, Q, c["c"])
    # through the claims wrapper at (1024, 1)
    w = wrapper_case(1024, 1, 27)
    params, cl, opening = w["bfv"].params, w["claims"], folded_wrapper(1024, 1, 27)
    assert hg.claims_verify_folded_bn254(params, w["cm"].root, cl, opening, ctx=ctx) == (True, "")
    dev = hg.Commitment.secrets_bn254(ctx, params, w["w"])
    assert dev.open_claims_folded(params, cl) == opening
    V, m = max(w["cm"].nvars), len(w["cm"].nvars)
    hb = 32 * (3 * V + m)
    for at in (31, 32 * 3 * V + 31, hb + 32 + 31, hb + 32 * (1 << dev.log2_row) + 31, len(opening) - 1):   # round 0, Y_0, u_0, u_1, the last sibling
        bad = bytearray(opening)
        bad[at] ^= 1
        h = hg.claims_verify_folded_bn254(params, w["cm"].root, cl, bytes(bad))
        assert not h[0] and hg.claims_verify_folded_bn254(params, w["cm"].root, cl, bytes(bad), ctx=ctx) == h, at


@pytest.mark.gpu
def test_headline_size_once(ctx):
    """n=32768 k=16: the 47 claims of a hg_prove_bn254 proof opened folded from the handle of hg_secrets_commit_bn254"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x8000 + 16)
    proof = ctx.prove_bn254(pk, w, cap=1 << 25)[0]
    ok, why, cl = hg.verify_public_bn254(pk, hg.Instance.from_witness(w), proof, ctx=ctx, device=True)
    assert ok, why
    assert cl.n == 47
    cm = hg.Commitment.secrets_bn254(ctx, bfv.params, w)
    opening = cm.open_claims_folded(bfv.params, cl)
    assert len(opening) == 6896960 == hg.pcs_folded_opening_bytes_bn254(cm.nvars)
    assert hg.claims_verify_folded_bn254(bfv.params, cm.root, cl, opening) == (True, "")
    assert hg.claims_verify_folded_bn254(bfv.params, cm.root, cl, opening, ctx=ctx) == (True, "")
    root = bytearray(cm.root)
    root[7] ^= 0x10
    h = hg.claims_verify_folded_bn254(bfv.params, bytes(root), cl, opening)
    assert not h[0] and hg.claims_verify_folded_bn254(bfv.params, bytes(root), cl, opening, ctx=ctx) == h
    pk.free()
