"""hg_pcs_open_folded / hg_pcs_verify_folded / hg_pcs_verify_folded_device and the hg_claims_*_folded wrappers: all claims of an opening
reduced to one point by a sum-check over the committed tables. The yardstick is py_verify_folded, the verifier of the section "Folded
openings" of include/hg.h restated in Python integers (its own transcript, rounds, final evaluation, combined row; the code and the tree
as test_pcs.py restates them): host openings must be accepted by it, every tampered input must get the same documented reason from it
and from the C verifier, the device forms must equal the host forms byte for byte and reason for reason."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

import orclib
from hglib import hg, ROOT
from test_pcs import P, PyCommit, e_add, e_dot, e_dot_f, e_mul, encode, eq_table, le64, make_tables, py_mle, py_verify, wrapper_case

NEW = ["hg_pcs_open_folded", "hg_pcs_verify_folded", "hg_pcs_verify_folded_device", "hg_claims_open_folded", "hg_claims_verify_folded", "hg_claims_verify_folded_device"]
Q = 5
# name -> (nvars, c, the tables of the claims). unequal: tables of unequal size (the (1 - X) tail), table 2 without a claim and a single
# row (v_t = c), two claims on tables 0 and 1. single: one table, one row, one claim. mid: three sizes, every table claimed
SHAPES = {"unequal": ([4, 3, 2, 4], 2, [0, 1, 1, 3, 0]), "single": ([3], 3, [0]), "mid": ([8, 7, 6], 4, [0, 1, 2, 0])}
# larger ones for the device form: the four-step NTT sizes of test_pcs.py, more than one workgroup a table in the first rounds
DEVICE_SHAPES = dict(SHAPES, eleven=([11], 5, [0, 0, 0]), twelve=([12, 12, 9], 6, [0, 1, 2, 1, 0]))
ROUND = "pcs: fold round %d does not match the running claim"
FINAL = "pcs: fold final evaluation mismatch"


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


ONE = (1, 0)


def claims_on(tables, which, seed):
    """one claim per entry of `which` (a table index) at a random E point with the table's value: [(table, point words, (v0, v1))]"""
    rng = random.Random(seed)
    out = []
    for t in which:
        pt = [(rng.randrange(P), rng.randrange(P)) for _ in range(tables[t].size.bit_length() - 1)]
        out.append((t, [x for p in pt for x in p], py_mle(tables[t], pt)))
    return out


def folded_len(nvars, c, Qn):
    return 16 * (3 * max(nvars) + len(nvars)) + 32 * (1 << c) + Qn * (8 * sum(1 << (v - c) for v in nvars) + 32 * (c + 2))


class FoldTranscript:
    """the absorbing transcript of a folded opening: "hg-pcs-fold-1", then what "hg-pcs-1" appends after its tag"""

    def __init__(self, root, c, nvars, Qn, claims):
        le32 = lambda x: int(x).to_bytes(4, "little")   # noqa: E731
        self.pending = b"hg-pcs-fold-1" + root + le32(c) + le32(len(nvars)) + b"".join(le32(v) for v in nvars) + le32(Qn) + le32(len(claims))
        for t, pt, val in claims:
            self.pending += le32(t) + b"".join(le64(x) for x in pt) + le64(val[0]) + le64(val[1])

    def squeeze_f(self):
        self.pending = orclib.keccak256(self.pending)
        return int.from_bytes(self.pending, "little") % P

    def squeeze(self):
        a = self.squeeze_f()
        return (a, self.squeeze_f())

    def absorb_e(self, x):
        self.pending += le64(x[0]) + le64(x[1])


def py_verify_folded(root, nvars, c, claims, Qn, proof):
    """the verifier of "Folded openings" in include/hg.h, checks in the documented order; "" or the documented reason"""
    Cn, N, m, V, n = 1 << c, 4 << c, len(nvars), max(nvars), len(claims)
    R = sum(1 << (v - c) for v in nvars)
    off = [sum(1 << (v - c) for v in nvars[:t]) for t in range(m)]
    hb, qb = 16 * (3 * V + m), 8 * R + 32 * (c + 2)
    # 1. the exact length
    if len(proof) != folded_len(nvars, c, Qn):
        return "pcs: the opening has %d bytes, %d expected" % (len(proof), folded_len(nvars, c, Qn))
    # 2. every element and column word below p, the lowest offset
    word = lambda at: int.from_bytes(proof[at:at + 8], "big")   # noqa: E731
    elem = lambda at: (word(at), word(at + 8))                   # noqa: E731
    cols_at = hb + 32 * Cn
    for at in [8 * i for i in range((hb + 32 * Cn) // 8)] + [cols_at + q * qb + 8 * r for q in range(Qn) for r in range(R)]:
        if word(at) >= P:
            return "pcs: non-canonical word at byte %d" % at
    pts = [[(pt[2 * i], pt[2 * i + 1]) for i in range(len(pt) // 2)] for _, pt, _ in claims]
    tr = FoldTranscript(root, c, nvars, Qn, claims)
    beta = tr.squeeze()
    bpow = [ONE]
    for _ in range(n - 1):
        bpow.append(e_mul(bpow[-1], beta))
    claim = (0, 0)
    for b, (_, _, val) in zip(bpow, claims):
        claim = e_add(claim, e_mul(b, tuple(val)))
    # 3. the rounds
    rho = []
    for j in range(V):
        c0, c1, c2 = (elem(16 * (3 * j + k)) for k in range(3))
        if e_add(e_add(c0, c0), e_add(c1, c2)) != claim:
            return ROUND % j
        for x in (c0, c1, c2):
            tr.absorb_e(x)
        r = tr.squeeze()
        rho.append(r)
        claim = e_add(c0, e_mul(r, e_add(c1, e_mul(r, c2))))
    # 4. the final evaluation
    Y = [elem(16 * (3 * V + t)) for t in range(m)]
    for y in Y:
        tr.absorb_e(y)
    fin = (0, 0)
    for t in range(m):
        g = (0, 0)
        for i, (ti, _, _) in enumerate(claims):
            if ti == t:
                e = bpow[i]
                for z, r in zip(pts[i], rho):     # eq(z, r) = z r + (1 - z)(1 - r) per coordinate
                    e = e_mul(e, e_add(e_mul(z, r), e_mul(e_sub(ONE, z), e_sub(ONE, r))))
                g = e_add(g, e)
        term = e_mul(Y[t], g)
        for j in range(nvars[t], V):
            term = e_mul(term, e_sub(ONE, rho[j]))
        fin = e_add(fin, term)
    if fin != claim:
        return FINAL
    # 5. the combined row at rho[..c)
    delta = tr.squeeze()
    rho_p = tr.squeeze()
    u = [[elem(hb + 16 * (i * Cn + j)) for j in range(Cn)] for i in range(2)]
    dpow = [ONE]
    for _ in range(m - 1):
        dpow.append(e_mul(dpow[-1], delta))
    y = (0, 0)
    for d, yt in zip(dpow, Y):
        y = e_add(y, e_mul(d, yt))
    if e_dot(u[1], eq_table(rho[:c])) != y:
        return "pcs: evaluation mismatch at claim 0"
    for ui in u:
        for x in ui:
            tr.absorb_e(x)
    js = [tr.squeeze_f() & (N - 1) for _ in range(Qn)]
    # 6. the queries
    rho_pw = [ONE]
    for _ in range(R - 1):
        rho_pw.append(e_mul(rho_pw[-1], rho_p))
    w = [None] * R
    for t in range(m):
        for r, e in enumerate(eq_table(rho[c:nvars[t]])):
            w[off[t] + r] = e_mul(dpow[t], e)
    enc = [(encode([x[0] for x in ui], c), encode([x[1] for x in ui], c)) for ui in u]
    for q in range(Qn):
        base = cols_at + q * qb
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
        if e_dot_f(w, col) != (enc[1][0][js[q]], enc[1][1][js[q]]):
            return "pcs: claim 0 inconsistent at query %d" % q
    return ""


# ---- cases (computed once, never changed) ----------------------------------------------------------------------------------------
_CASES = {}


def case(name):
    """per shape: tables, claims, the host commitment, its folded opening, the Python commitment"""
    if name not in _CASES:
        nvars, c, which = DEVICE_SHAPES[name]
        tables = make_tables(nvars, 0xf01d + len(name))
        cm = hg.Commitment.commit(None, tables, log2_row=c)
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
    R = sum(1 << (v - cc) for v in nvars)
    hb, qb = 16 * (3 * V + m), 8 * R + 32 * (cc + 2)
    cols_at = hb + 32 * Cn
    path0 = {"pcs: Merkle path mismatch at query 0", "pcs: proximity mismatch at query 0"}   # the indices move with the transcript
    early = {ROUND % 0, ROUND % 1}   # with one claim S = y whatever beta is: round 0 still holds, round 1 does not

    def flip(at, src=proof):
        """one bit of one byte changed: the byte at `at`, or in a field word (every use but the siblings') the first bit from there on, going
        round the word, that leaves it below p"""
        b = bytearray(src)
        if at >= cols_at and (at - cols_at) % qb >= 8 * R:
            b[at] ^= 0x01
            return bytes(b)
        w0 = at & ~7
        for k in range(8):
            for bit in range(8):
                b[w0:w0 + 8] = src[w0:w0 + 8]
                b[w0 + (at - w0 + k) % 8] ^= 1 << bit
                if int.from_bytes(b[w0:w0 + 8], "big") < P:
                    return bytes(b)
        raise AssertionError("no canonical neighbour")

    def setp(at, src=proof):
        return src[:at] + P.to_bytes(8, "big") + src[at + 8:]

    out = []
    for k in range(3):                                                         # c0 of round 0, c1 of round 1, c2 of the last round
        j = (0, 1, V - 1)[k]
        out.append(("c%d of round %d" % (k, j), root, claims, flip(16 * (3 * j + k) + 7), {ROUND % j}))
    out.append(("Y_0", root, claims, flip(16 * 3 * V + 15), {FINAL}))
    if name == "unequal":                                                      # g_2 = 0: the final evaluation holds, the combined row's value does not
        out.append(("Y of the claimless table", root, claims, flip(16 * (3 * V + 2) + 7), {"pcs: evaluation mismatch at claim 0"}))
    out.append(("u_0", root, claims, flip(hb + 16 + 7), path0))
    out.append(("u_1", root, claims, flip(hb + 16 * Cn + 16 + 15), {"pcs: evaluation mismatch at claim 0"}))
    for q in (0, 3):
        out.append(("column word, query %d" % q, root, claims, flip(cols_at + q * qb + 8 * (R - 1) + 7), {"pcs: Merkle path mismatch at query %d" % q}))
        out.append(("sibling, query %d" % q, root, claims, flip(cols_at + q * qb + 8 * R + 32 + 9), {"pcs: Merkle path mismatch at query %d" % q}))
    for label, at in (("header", 16 * (3 * V) + 8), ("first header word", 0), ("u", hb + 16 * Cn + 8), ("column", cols_at + qb + 8 * (R - 1))):
        out.append(("p in the " + label, root, claims, setp(at), {"pcs: non-canonical word at byte %d" % at}))
    want = len(proof)
    out.append(("extended", root, claims, proof + b"\0", {"pcs: the opening has %d bytes, %d expected" % (want + 1, want)}))
    out.append(("truncated", root, claims, proof[:-1], {"pcs: the opening has %d bytes, %d expected" % (want - 1, want)}))
    t, pt, v = claims[0]
    out.append(("claim value", root, [(t, pt, ((v[0] + 1) % P, v[1]))] + claims[1:], proof, {ROUND % 0}))
    out.append(("claim point", root, [(t, [(pt[0] + 1) % P] + pt[1:], v)] + claims[1:], proof, early))
    out.append(("root", bytes([root[0] ^ 1]) + root[1:], claims, proof, early))
    # two failures at once: the order of the checks decides
    out.append(("column p and round 1", root, claims, setp(cols_at + 8 * (R - 1), flip(16 * 3 + 7)), {"pcs: non-canonical word at byte %d" % (cols_at + 8 * (R - 1))}))
    out.append(("round 0 and u_1", root, claims, flip(hb + 16 * Cn + 15, flip(7)), {ROUND % 0}))
    out.append(("u_1 and a sibling", root, claims, flip(hb + 16 * Cn + 15, flip(cols_at + 8 * R + 3)), {"pcs: evaluation mismatch at claim 0"}))
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
    assert len(c["proof"]) == folded_len(nvars, cc, Q) == hg.pcs_folded_opening_bytes(nvars, Q, cc)
    assert py_verify_folded(c["cm"].root, nvars, cc, c["claims"], Q, c["proof"]) == ""
    assert hg.pcs_verify_folded(c["cm"].root, nvars, c["claims"], c["proof"], Q, cc) == (True, "")
    # the length does not grow with the claims
    assert len(c["cm"].open_folded(c["claims"] + c["claims"][:1], Q)) == len(c["proof"])


def test_a_table_of_one_word_is_a_scalar_from_the_start():
    nvars = [2, 0]
    tables = make_tables(nvars, 0x51)
    cm = hg.Commitment.commit(None, tables, log2_row=0)
    assert cm.log2_row == 0
    claims = claims_on(tables, [1, 0, 1], 3)
    proof = cm.open_folded(claims, Q)
    assert len(proof) == folded_len(nvars, 0, Q)
    assert py_verify_folded(cm.root, nvars, 0, claims, Q, proof) == ""
    assert hg.pcs_verify_folded(cm.root, nvars, claims, proof, Q, 0) == (True, "")


# ---- 3. tampering ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tampered_openings_get_the_documented_reason_from_both_verifiers(name):
    c = case(name)
    for label, root, claims, proof, allowed in tamper_set(name):
        ok, why = hg.pcs_verify_folded(root, c["nvars"], claims, proof, Q, c["c"])
        assert not ok and why in allowed, (label, why, allowed)
        assert why == py_verify_folded(root, c["nvars"], c["c"], claims, Q, proof), label


# ---- 4. errors -------------------------------------------------------------------------------------------------------------------
def test_a_wrong_value_is_refused_by_the_prover_naming_the_claim_and_the_function():
    c = case("unequal")
    for i in (2, 4):
        bad = list(c["claims"])
        t, pt, v = bad[i]
        bad[i] = (t, pt, (v[0], (v[1] + 1) % P))
        with pytest.raises(hg.HgError, match=r"hg_pcs_open_folded: claim %d: the value is not the evaluation of table %d at the point" % (i, t)):
            c["cm"].open_folded(bad, Q)
    bad = [(t, pt, ((v[0] + 1) % P, v[1])) for t, pt, v in c["claims"]]          # every value wrong: the lowest is named
    with pytest.raises(hg.HgError, match=r"hg_pcs_open_folded: claim 0\b"):
        c["cm"].open_folded(bad, Q)
    assert c["cm"].open_folded(c["claims"], Q) == c["proof"]                      # the handle still opens


def test_bad_arguments_are_errors_naming_the_function():
    L = hg.lib()
    c = case("unequal")
    nvars, cm, proof = c["nvars"], c["cm"], c["proof"]
    nv = (C.c_uint32 * 4)(*nvars)
    table, pts, vals = hg._pcs_claim_arrays(c["claims"])
    n = len(c["claims"])
    buf, ln = (C.c_uint8 * len(proof))(), C.c_size_t(0)
    good = (None, cm.h, table, hg._ptr(pts), hg._ptr(vals), n, Q, buf, len(buf), C.byref(ln))

    def sub(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    far = (C.c_uint32 * n)(0, 4, 1, 3, 0)                          # a table index out of range
    big = pts.copy()
    big[1] = P                                                     # a non-canonical coordinate
    for args in (sub(good, 1, None), sub(good, 2, None), sub(good, 3, None), sub(good, 4, None), sub(good, 7, None), sub(good, 9, None), sub(good, 2, far),
                 sub(good, 3, hg._ptr(big)), sub(good, 6, 1 << 20)):
        assert L.hg_pcs_open_folded(*args) == -1 and "hg_pcs_open_folded" in _last(), args
    assert L.hg_pcs_open_folded(*sub(good, 5, 0)) == -1 and _last() == "hg_pcs_open_folded: a folded opening needs a claim"
    ln.value = 0
    assert L.hg_pcs_open_folded(*sub(good, 8, len(buf) - 1)) == -1 and "hg_pcs_open_folded" in _last() and ln.value == len(proof)   # *len reports the need
    assert L.hg_pcs_open_folded(*good) == 0 and bytes(buf) == proof and ln.value == len(proof)
    vgood = (cm.root, nv, 4, 2, table, hg._ptr(pts), hg._ptr(vals), n, Q, proof, len(proof))
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 4, None), sub(vgood, 5, None), sub(vgood, 6, None), sub(vgood, 9, None), sub(vgood, 4, far),
                 sub(vgood, 3, 3), sub(vgood, 2, 0), sub(vgood, 2, 65), sub(vgood, 5, hg._ptr(big)), sub(vgood, 8, 1 << 20)):
        assert L.hg_pcs_verify_folded(*args) == -1 and "hg_pcs_verify_folded" in _last(), args
    assert L.hg_pcs_verify_folded(*sub(vgood, 7, 0)) == -1 and _last() == "hg_pcs_verify_folded: a folded opening needs a claim"
    assert L.hg_pcs_verify_folded(*vgood) == 0
    assert L.hg_pcs_verify_folded_device(None, *vgood) == -1 and _last() == "hg_pcs_verify_folded_device: no context"
    # a BN254 handle
    bn = hg.Commitment.commit_bn254(None, [[1, 2, 3, 4]], 1)
    assert L.hg_pcs_open_folded(*sub(good, 1, bn.h)) == -1 and "hg_pcs_open_folded" in _last() and "BN254" in _last()
    # the wrappers
    w = wrapper_case(1024, 1, 27)
    params, scm, cl = w["bfv"].params, w["cm"], w["claims"]
    cap = hg.pcs_folded_opening_bytes(scm.nvars)
    obuf, oln = (C.c_uint8 * cap)(), C.c_size_t(0)
    ogood = (None, C.byref(params), scm.h, cl.claims, cl.n, hg._ptr(cl.points), 0, obuf, cap, C.byref(oln))
    public = (hg.HgInputClaim * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3                                            # a claim on ais[0]: settled inside hg_verify_public, never opened
    for args in (sub(ogood, 1, None), sub(ogood, 2, None), sub(ogood, 3, None), sub(ogood, 5, None), sub(ogood, 7, None), sub(ogood, 9, None), sub(ogood, 3, public),
                 sub(ogood, 2, cm.h), sub(ogood, 4, 0), sub(ogood, 1, C.byref(hg.params_builtin(2048, 1)))):
        assert L.hg_claims_open_folded(*args) == -1 and "hg_claims_open_folded" in _last(), args
    opening = folded_wrapper(1024, 1, 27)
    vgood = (C.byref(params), scm.root, 0, cl.claims, cl.n, hg._ptr(cl.points), 0, opening, len(opening))
    for args in (sub(vgood, 0, None), sub(vgood, 1, None), sub(vgood, 3, None), sub(vgood, 5, None), sub(vgood, 7, None), sub(vgood, 3, public), sub(vgood, 2, 12),
                 sub(vgood, 4, 0)):
        assert L.hg_claims_verify_folded(*args) == -1 and "hg_claims_verify_folded" in _last(), args
    assert L.hg_claims_verify_folded(*vgood) == 0
    assert L.hg_claims_verify_folded_device(None, *vgood) == -1 and _last() == "hg_claims_verify_folded_device: no context"


def test_the_two_forms_of_opening_reject_each_other():
    """by the length rule or by the first check that reads the other layout, never a crash"""
    for name in sorted(SHAPES):
        c = case(name)
        nvars, cc, claims, root = c["nvars"], c["c"], c["claims"], c["cm"].root
        plain = c["cm"].open(claims, Q)
        ok, why = hg.pcs_verify_folded(root, nvars, claims, plain, Q, cc)
        assert not ok and why == py_verify_folded(root, nvars, cc, claims, Q, plain) and why.startswith("pcs: "), why
        ok, why = hg.pcs_verify(root, nvars, claims, c["proof"], Q, cc)
        assert not ok and why == py_verify(root, nvars, cc, claims, Q, c["proof"]) and why.startswith("pcs: "), why


# ---- 5. the wrappers over the secret inputs --------------------------------------------------------------------------------------
_FOLDED_WRAP = {}


def folded_wrapper(n, k, bits):
    if (n, k) not in _FOLDED_WRAP:
        w = wrapper_case(n, k, bits)
        _FOLDED_WRAP[(n, k)] = w["cm"].open_claims_folded(w["bfv"].params, w["claims"])
    return _FOLDED_WRAP[(n, k)]


@pytest.mark.parametrize("n,k,bits", [(1024, 1, 27), (4096, 2, 55)])
def test_claims_of_hg_verify_public_are_opened_folded_and_verified(n, k, bits):
    c = wrapper_case(n, k, bits)
    params, cl = c["bfv"].params, c["claims"]
    opening = folded_wrapper(n, k, bits)
    nvars = c["cm"].nvars
    assert len(opening) == hg.pcs_folded_opening_bytes(nvars) == folded_len(nvars, hg.pcs_row_log2(nvars), 241) < len(c["opening"])
    assert hg.claims_verify_folded(params, c["cm"].root, cl, opening) == (True, "")
    assert hg.claims_verify(params, c["cm"].root, cl, opening)[0] is False
    # the same bytes through the generic layer
    mapped = [(i if i < 3 else i - k, list(pt), v) for i, _, pt, v in cl.as_tuples()]
    assert hg.pcs_verify_folded(c["cm"].root, nvars, mapped, opening) == (True, "")
    bad = bytearray(opening)
    bad[-1] ^= 1                                                   # the last sibling
    assert hg.claims_verify_folded(params, c["cm"].root, cl, bytes(bad)) == (False, "pcs: Merkle path mismatch at query 240")
    # an opening made from another witness: refused by the prover, or rejected against the honest root
    d = {f: v.copy() for f, v in c["d"].items()}
    d["s"][0] = (int(d["s"][0]) + 1) % P
    other = hg.Commitment.secrets(None, params, hg.Witness.from_arrays(params, d))
    try:
        forged = other.open_claims_folded(params, cl)
    except hg.HgError as e:
        assert re.search(r"hg_claims_open_folded: claim \d+\b", str(e))
        return
    ok, why = hg.claims_verify_folded(params, c["cm"].root, cl, forged)
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
    dev = hg.Commitment.commit(ctx, c["tables"], c["c"])
    assert dev.root == c["cm"].root
    assert dev.open_folded(c["claims"], Q) == c["proof"]
    assert hg.pcs_verify_folded(dev.root, c["nvars"], c["claims"], c["proof"], Q, c["c"], ctx=ctx) == (True, "")
    bad = list(c["claims"])
    t, pt, v = bad[-1]
    bad[-1] = (t, pt, ((v[0] + 1) % P, v[1]))
    with pytest.raises(hg.HgError, match=r"hg_pcs_open_folded: claim %d\b" % (len(bad) - 1)):
        dev.open_folded(bad, Q)
    assert dev.open(c["claims"], Q) == c["cm"].open(c["claims"], Q)              # the raw rows are as they were


# A launch of the reduction has at most 2048 workgroups (HG_PCS_FOLD_BLOCKS lowers the bound), so on the shapes above a thread makes at
# most 8 trips. With one workgroup a table, a table of 2^16 entries gives 128 trips in round 0, 64 in round 1 and 32, 16 in the two
# rounds after it: the unreduced sums restart (WFLUSH_TRIPS = 16) in all three kernels; 20 claims on one table restart those of the g
# kernel. The plan line shows that the rounds ran on the device.
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import test_pcs_folded as T
from hglib import hg
nvars, c = [16, 13], 7
tables = T.make_tables(nvars, 0xb16)
claims = T.claims_on(tables, [0] * 20 + [1], 8)
host = hg.Commitment.commit(None, tables, c)
ctx = hg.Context(0)
dev = hg.Commitment.commit(ctx, tables, c)
assert dev.root == host.root
proof = dev.open_folded(claims, 5)
assert proof == host.open_folded(claims, 5)
assert hg.pcs_verify_folded(host.root, nvars, claims, proof, 5, c) == (True, "")
assert hg.pcs_verify_folded(host.root, nvars, claims, proof, 5, c, ctx=ctx) == (True, "")
print("FOLD OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["1", "2048"])
def test_long_accumulations_and_the_plan_line(blocks):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, HG_DEBUG="plan", HG_PCS_FOLD_BLOCKS=blocks))
    assert r.returncode == 0 and "FOLD OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    plan = re.findall(r"\[hg plan\] pcsfold V=(\d+) dev_rounds=(\d+) host_rounds=(\d+) tables=(\d+) claims=(\d+)", r.stderr)
    assert plan == [("16", "16", "0", "2", "21")], r.stderr[-2000:]


@pytest.mark.gpu
def test_device_verifier_gives_the_host_decision_and_reason(ctx):
    c = case("unequal")
    for label, root, claims, proof, _ in tamper_set("unequal"):
        assert hg.pcs_verify_folded(root, c["nvars"], claims, proof, Q, c["c"], ctx=ctx) == hg.pcs_verify_folded(root, c["nvars"], claims, proof, Q, c["c"]), label
    plain = c["cm"].open(c["claims"], Q)
    assert hg.pcs_verify_folded(c["cm"].root, c["nvars"], c["claims"], plain, Q, c["c"], ctx=ctx) == hg.pcs_verify_folded(c["cm"].root, c["nvars"], c["claims"], plain, Q, c["c"])
    # through the claims wrapper at (1024, 1)
    w = wrapper_case(1024, 1, 27)
    params, cl, opening = w["bfv"].params, w["claims"], folded_wrapper(1024, 1, 27)
    assert hg.claims_verify_folded(params, w["cm"].root, cl, opening, ctx=ctx) == (True, "")
    dev = hg.Commitment.secrets(ctx, params, w["w"])
    assert dev.open_claims_folded(params, cl) == opening
    V, m = max(w["cm"].nvars), len(w["cm"].nvars)
    hb = 16 * (3 * V + m)
    for at in (7, 16 * 3 * V + 15, hb + 16 + 7, hb + 16 * (1 << dev.log2_row) + 15, len(opening) - 1):
        bad = bytearray(opening)
        bad[at] ^= 1
        h = hg.claims_verify_folded(params, w["cm"].root, cl, bytes(bad))
        assert not h[0] and hg.claims_verify_folded(params, w["cm"].root, cl, bytes(bad), ctx=ctx) == h, at


@pytest.mark.gpu
def test_headline_size_once(ctx):
    """n=32768 k=16: the 47 claims of a bound proof opened folded from the handle of hg_prove_committed_mode"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x8000 + 17)
    vals = hg.witness_gen(ctx, pk, w)
    out, cm = hg.prove_committed_mode(ctx, pk, vals, hg.ProofBuffer(cap=1 << 25), 3)
    ok, why, cl = hg.verify_public_bound(pk, hg.Instance.from_witness(w), out.bytes(), cm.root, 3, ctx=ctx, device=True)
    assert ok, why
    assert cl.n == 47
    opening = cm.open_claims_folded(bfv.params, cl)
    assert len(opening) == 1832816 == hg.pcs_folded_opening_bytes(cm.nvars)
    assert hg.claims_verify_folded(bfv.params, cm.root, cl, opening) == (True, "")
    assert hg.claims_verify_folded(bfv.params, cm.root, cl, opening, ctx=ctx) == (True, "")
    root = bytearray(cm.root)
    root[7] ^= 0x10
    h = hg.claims_verify_folded(bfv.params, bytes(root), cl, opening)
    assert not h[0] and hg.claims_verify_folded(bfv.params, bytes(root), cl, opening, ctx=ctx) == h
    vals.free()
    pk.free()
