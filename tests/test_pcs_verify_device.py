"""hg_pcs_verify_device / hg_claims_verify_device: the opening verifier on a context. The yardstick is the host verifier: on every input
the device form's (decision, reason) equals hg_pcs_verify's, which tests/test_pcs.py holds against the Python restatement (py_verify).
Honest openings on both encoding paths, the tampering matrix, wrong but transcript-consistent openings built by a Python prover (the
two reasons a flipped byte cannot reach) and pairs of faults, where the host's order decides which one is reported."""
import ctypes as C
import os
import re

import pytest

import test_pcs as tp
from hglib import hg, ROOT

P = hg.P
NEW = ["hg_pcs_verify_device", "hg_claims_verify_device"]


def _last():
    return hg.lib().hg_last_error().decode()


def flip(proof, at, mask=0x01):
    b = bytearray(proof)
    b[at] ^= mask
    return bytes(b)


def put_p(proof, at):
    return proof[:at] + P.to_bytes(8, "big") + proof[at + 8:]


# ---- the prover of include/hg.h in Python integers, with a handle on u ----------------------------------------------------------
def py_open(py, claims, Q, which=None, delta=None):
    """The opening of `claims` against the Python commitment. which / delta: vector `which` of u_0 (proximity), u_1 .. u_n (claim
    which - 1) has `delta` (C elements) added BEFORE it enters the transcript, and a claim's value is recomputed from its changed
    vector, so the opening is wrong but consistent with its own transcript. -> (bytes, the claims as opened, the column indices)"""
    c, nvars = py.c, py.nvars
    Cn, N, R = 1 << c, 4 << c, len(py.rows)
    claims = list(claims)
    us = [None]
    for k, (t, pt, val) in enumerate(claims):
        pts = [(pt[2 * i], pt[2 * i + 1]) for i in range(len(pt) // 2)]
        w = tp.eq_table(pts[c:])
        u = [tp.e_dot_f(w, [py.rows[py.off[t] + r][j] for r in range(len(w))]) for j in range(Cn)]
        if which == k + 1:
            u = [tp.e_add(a, b) for a, b in zip(u, delta)]
            claims[k] = (t, pt, tp.e_dot(u, tp.eq_table(pts[:c])))
        us.append(u)
    tr = tp.PyTranscript(py.root, c, nvars, Q, claims)
    rho = tr.squeeze()
    pw = tp._powers(rho, R)
    us[0] = [tp.e_dot_f(pw, [row[j] for row in py.rows]) for j in range(Cn)]
    if which == 0:
        us[0] = [tp.e_add(a, b) for a, b in zip(us[0], delta)]
    out = b""
    for u in us:
        for x in u:
            out += x[0].to_bytes(8, "big") + x[1].to_bytes(8, "big")
            tr.absorb(x[0])
            tr.absorb(x[1])
    js = [tr.squeeze_f() & (N - 1) for _ in range(Q)]
    for j in js:
        out += b"".join(m[j].to_bytes(8, "big") for m in py.M)
        out += b"".join(py.levels[lv][(j >> lv) ^ 1] for lv in range(c + 2))
    return out, claims, js


_FORGED = {}


def forged_case(kind):
    """R = 17, c = 2, Q = 5: "proximity": u_0 + e; "claim": the vector of claim 2 + e with the value recomputed. e has one non-zero
    element, so Enc(e) vanishes nowhere and the first query is the one that fails."""
    if kind not in _FORGED:
        c = tp.c2_case(17)
        e = [(0, 0), (3, 5), (0, 0), (0, 0)]
        proof, claims, js = py_open(c["py"], c["claims"], 5, 0 if kind == "proximity" else 3, e)
        want = "pcs: proximity mismatch at query 0" if kind == "proximity" else "pcs: claim 2 inconsistent at query 0"
        _FORGED[kind] = dict(proof=proof, claims=claims, want=want)
    return _FORGED[kind]


# ---- not gpu ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name


def test_no_context_and_bad_arguments_are_errors_naming_the_function():
    L = hg._pcs_protos()
    c = tp.c2_case(15)
    nv = (C.c_uint32 * 4)(*c["nvars"])
    table, pts, vals = hg._pcs_claim_arrays(c["claims"])
    proof = c["open35"]
    good = (None, c["cm"].root, nv, 4, 2, table, hg._ptr(pts), hg._ptr(vals), 3, 5, proof, len(proof))

    def sub(args, i, v):
        return args[:i] + (v,) + args[i + 1:]
    assert L.hg_pcs_verify_device(*good) == -1 and _last() == "hg_pcs_verify_device: no context"
    far = (C.c_uint32 * 3)(0, 4, 2)                              # a table index out of range
    big = pts.copy()
    big[1] = P                                                   # a non-canonical coordinate
    for args, text in ((sub(good, 1, None), "null argument"), (sub(good, 2, None), "null argument"), (sub(good, 5, far), "names table 4"),
                       (sub(good, 6, hg._ptr(big)), "non-canonical coordinate"), (sub(good, 4, 3), "log2_row"), (sub(good, 9, 1 << 20), "queries")):
        assert L.hg_pcs_verify_device(*args) == -1, args
        assert _last().startswith("hg_pcs_verify_device: ") and text in _last(), _last()
    with pytest.raises(hg.HgError, match="hg_pcs_verify_device: no context"):
        hg.pcs_verify(c["cm"].root, c["nvars"], c["claims"], proof, 5, 2, ctx=type("NoCtx", (), {"h": None})())
    # the wrapper
    w = tp.wrapper_case(1024, 1, 27)
    params, cl = w["bfv"].params, w["claims"]
    vgood = (None, C.byref(params), w["cm"].root, 0, cl.claims, cl.n, hg._ptr(cl.points), 0, w["opening"], len(w["opening"]))
    assert L.hg_claims_verify_device(*vgood) == -1 and _last() == "hg_claims_verify_device: no context"
    public = (hg.HgInputClaim * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3                                          # a claim on ais[0]
    for args in (sub(vgood, 1, None), sub(vgood, 2, None), sub(vgood, 4, None), sub(vgood, 4, public), sub(vgood, 3, 12)):
        assert L.hg_claims_verify_device(*args) == -1 and _last().startswith("hg_claims_verify_device: ") and "no context" not in _last(), _last()


@pytest.mark.parametrize("kind", ["proximity", "claim"])
def test_transcript_consistent_wrong_openings_reach_the_two_late_reasons_on_the_host(kind):
    """what the device form is compared with in the GPU case below: the host verifier and py_verify give the intended text"""
    c, f = tp.c2_case(17), forged_case(kind)
    assert tp.py_verify(c["py"].root, c["nvars"], 2, f["claims"], 5, f["proof"]) == f["want"]
    assert hg.pcs_verify(c["cm"].root, c["nvars"], f["claims"], f["proof"], 5, 2) == (False, f["want"])
    honest, claims, _ = py_open(c["py"], c["claims"], 5)
    assert honest == c["open35"] and claims == c["claims"]      # the Python prover is the library's


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def both(ctx, root, nvars, claims, proof, Q, c):
    """(decision, reason) of the host form, after asserting the device form's is the same"""
    host = hg.pcs_verify(root, nvars, claims, proof, Q, c)
    dev = hg.pcs_verify(root, nvars, claims, proof, Q, c, ctx=ctx)
    assert dev == host, (dev, host)
    return host


@pytest.mark.gpu
@pytest.mark.parametrize("R,nvars", tp.C2_SHAPES)
def test_honest_openings_radix2_path(ctx, R, nvars):
    c = tp.c2_case(R)
    assert both(ctx, c["cm"].root, nvars, c["claims"], c["open35"], 5, 2) == (True, "")
    assert both(ctx, c["cm"].root, nvars, [], c["open01"], 1, 2) == (True, "")


@pytest.mark.gpu
@pytest.mark.parametrize("nvars", [[8, 7, 6], [11]])
def test_honest_openings_four_step_path(ctx, nvars):
    """c = 6: Enc(u_i) is the LDS four-step NTT of size 256"""
    assert hg.pcs_row_log2(nvars, 6) == 6 and 8 <= 6 + 2 <= 16
    tables = tp.make_tables(nvars, 0x6c6 + len(nvars))
    cm = hg.Commitment.commit(None, tables, 6)
    claims = tp.make_claims(tables, 4, 5)
    proof = cm.open(claims)
    assert len(proof) == hg.pcs_opening_bytes(nvars, 4, 0, 6)
    assert both(ctx, cm.root, nvars, claims, proof, 0, 6) == (True, "")
    assert both(ctx, cm.root, nvars, claims, flip(proof, 16 * 64 * 2 + 3), 0, 6) == (False, "pcs: evaluation mismatch at claim 1")


@pytest.mark.gpu
def test_chunk_and_workgroup_boundaries(ctx):
    """R = 129: a weight table of 128 entries is two whole reduction chunks, the column's 129 three; 130 hashed words are 8 Keccak
    blocks; Q = 257 is one query past a workgroup, with duplicate indices at code length 16"""
    nvars, Q = [9, 2], 257
    tables = tp.make_tables(nvars, 0x129)
    cm = hg.Commitment.commit(None, tables, 2)
    claims = tp.make_claims(tables, 2, 9)
    proof = cm.open(claims, Q)
    R, qb, cols_at = 129, 8 * 129 + 32 * 4, 16 * 4 * 3
    assert len(proof) == cols_at + Q * qb
    assert both(ctx, cm.root, nvars, claims, proof, Q, 2) == (True, "")
    assert both(ctx, cm.root, nvars, claims, flip(proof, cols_at + 256 * qb + 8 * (R - 1) + 7), Q, 2) == (False, "pcs: Merkle path mismatch at query 256")


@pytest.mark.gpu
def test_the_tampering_matrix(ctx):
    R, c = 17, tp.c2_case(17)
    nvars, claims, proof, root = c["nvars"], c["claims"], c["open35"], c["cm"].root
    n, Q, Cn = 3, 5, 4
    qb, cols_at = 8 * R + 32 * 4, 16 * Cn * (n + 1)
    path0 = {"pcs: Merkle path mismatch at query 0", "pcs: proximity mismatch at query 0"}   # the indices move with the transcript

    def check(root_, claims_, proof_, allowed):
        ok, why = both(ctx, root_, nvars, claims_, proof_, Q, 2)
        assert not ok and why in allowed, (why, allowed)
        assert why == tp.py_verify(root_, nvars, 2, claims_, Q, proof_)

    check(root, claims, flip(proof, 16 * 2 + 7), path0)                                                       # u_0
    for i in range(n):
        check(root, claims, flip(proof, 16 * Cn * (i + 1) + 16 + 15), {"pcs: evaluation mismatch at claim %d" % i})   # u_i
    for q in (0, 3):
        check(root, claims, flip(proof, cols_at + q * qb + 8 * 5 + 7), {"pcs: Merkle path mismatch at query %d" % q})            # a column word
        check(root, claims, flip(proof, cols_at + q * qb + 8 * R + 32 * 2 + 9), {"pcs: Merkle path mismatch at query %d" % q})   # a sibling
    for i in range(n):                                                                                         # a changed value
        bad = [(t, pt, ((v[0] + 1) % P, v[1]) if k == i else v) for k, (t, pt, v) in enumerate(claims)]
        check(root, bad, proof, {"pcs: evaluation mismatch at claim %d" % i})
    for coord, allowed in ((0, {"pcs: evaluation mismatch at claim 0"}), (2, path0)):                          # a coordinate below c / from c on
        t, pt, v = claims[0]
        bad = list(claims)
        bad[0] = (t, pt[:2 * coord] + [(pt[2 * coord] + 1) % P] + pt[2 * coord + 1:], v)
        check(root, bad, proof, allowed)
    check(bytes([root[0] ^ 1]) + root[1:], claims, proof, {"pcs: Merkle path mismatch at query 0"})            # a changed root
    want = len(proof)
    check(root, claims, proof + b"\0", {"pcs: the opening has %d bytes, %d expected" % (want + 1, want)})
    check(root, claims, proof[:-1], {"pcs: the opening has %d bytes, %d expected" % (want - 1, want)})
    for at in (16 * Cn + 16, cols_at + qb + 8 * 2):                                                            # a word = p: element, column
        check(root, claims, put_p(proof, at), {"pcs: non-canonical word at byte %d" % at})
    check(root, claims, proof[:8] + b"\xff" * 8 + proof[16:], {"pcs: non-canonical word at byte 8"})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["proximity", "claim"])
def test_the_two_reasons_flips_cannot_reach(ctx, kind):
    c, f = tp.c2_case(17), forged_case(kind)
    assert both(ctx, c["cm"].root, c["nvars"], f["claims"], f["proof"], 5, 2) == (False, f["want"])


@pytest.mark.gpu
def test_order_with_several_faults(ctx):
    R, c = 17, tp.c2_case(17)
    nvars, root = c["nvars"], c["cm"].root
    claims = tp.make_claims(c["tables"], 4, 0x66)
    n, Q, Cn = 4, 5, 4
    proof = c["cm"].open(claims, Q)
    qb, cols_at = 8 * R + 32 * 4, 16 * Cn * (n + 1)
    assert both(ctx, root, nvars, claims, proof, Q, 2) == (True, "")
    u_at = lambda i: 16 * Cn * (i + 1) + 16 + 15        # noqa: E731  a byte of claim i's vector
    sib_at = lambda q: cols_at + q * qb + 8 * R + 32 + 9   # noqa: E731
    # a sibling at query 1, a column word at query 3
    bad = flip(flip(proof, sib_at(1)), cols_at + 3 * qb + 8 * 4 + 7)
    assert both(ctx, root, nvars, claims, bad, Q, 2) == (False, "pcs: Merkle path mismatch at query 1")
    # a word = p in a column of query 2, a flipped u_1
    at = cols_at + 2 * qb + 8 * 6
    bad = flip(put_p(proof, at), u_at(1))
    assert both(ctx, root, nvars, claims, bad, Q, 2) == (False, "pcs: non-canonical word at byte %d" % at)
    # u_3 and u_1
    bad = flip(flip(proof, u_at(3)), u_at(1))
    assert both(ctx, root, nvars, claims, bad, Q, 2) == (False, "pcs: evaluation mismatch at claim 1")
    # the value of claim 0 and a sibling
    t, pt, v = claims[0]
    wrong = [(t, pt, ((v[0] + 1) % P, v[1]))] + claims[1:]
    assert both(ctx, root, nvars, wrong, flip(proof, sib_at(0)), Q, 2) == (False, "pcs: evaluation mismatch at claim 0")


def wrapper_inputs(ctx, bfv, pk, seed):
    w = hg.Witness.synthetic(bfv.params, seed)
    proof, _ = bfv.prove(ctx, pk, w, mode=3)
    ok, why, cl = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 3, ctx=ctx, device=True)
    assert ok, why
    cm = hg.Commitment.secrets(ctx, bfv.params, w)
    return cl, cm, cm.open_claims(bfv.params, cl)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
def test_wrappers(ctx, n, k):
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    cl, cm, opening = wrapper_inputs(ctx, bfv, pk, 0x9c5 + n)
    assert hg.claims_verify(bfv.params, cm.root, cl, opening) == (True, "")
    assert hg.claims_verify(bfv.params, cm.root, cl, opening, ctx=ctx) == (True, "")
    # the opening of another witness (of its own claims: the same count, so the same length)
    cl2, cm2, opening2 = wrapper_inputs(ctx, bfv, pk, 0x1c5 + n)
    assert cm2.root != cm.root and len(opening2) == len(opening)
    host = hg.claims_verify(bfv.params, cm.root, cl, opening2)
    assert not host[0] and host[1].startswith("pcs: ")
    assert hg.claims_verify(bfv.params, cm.root, cl, opening2, ctx=ctx) == host
    # a claim on a public input
    public = (hg.HgInputClaim * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3
    with pytest.raises(hg.HgError, match=r"hg_claims_verify_device: claim 0 is on input 3"):
        hg.claims_verify(bfv.params, cm.root, hg.InputClaims(public, cl.n, cl.points), opening, ctx=ctx)
    pk.free()


@pytest.mark.gpu
def test_headline_size_once(ctx):
    """(32768,16): 47 claims, c = 11, R = 864, 241 queries: the four-step NTT of 2^13 over 96 rows, 51 Keccak blocks a column"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x8000 + 16)
    proof, _ = bfv.prove(ctx, pk, w, cap=1 << 25)
    ok, why, cl = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 0, ctx=ctx, device=True)
    assert ok, why
    cm = hg.Commitment.secrets(ctx, bfv.params, w)
    assert cm.log2_row == 11 and cl.n == 47
    opening = cm.open_claims(bfv.params, cl)
    assert hg.claims_verify(bfv.params, cm.root, cl, opening, ctx=ctx) == (True, "")
    cols_at, qb = 16 * 2048 * 48, 8 * 864 + 32 * 13
    bad = flip(opening, cols_at + 200 * qb + 8 * 863 + 2)
    host = hg.claims_verify(bfv.params, cm.root, cl, bad)
    assert host == (False, "pcs: Merkle path mismatch at query 200")
    assert hg.claims_verify(bfv.params, cm.root, cl, bad, ctx=ctx) == host
    pk.free()


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    c = tp.c2_case(17)
    ctx.profile(2)
    ctx.profile_reset()
    try:
        assert hg.pcs_verify(c["cm"].root, c["nvars"], c["claims"], c["open35"], 5, 2, ctx=ctx) == (True, "")
        stat = [s for s in ctx.profile_get() if s["name"] == "pcs_verify"]
    finally:
        ctx.profile(0)
    assert len(stat) == 1 and stat[0]["launches"] >= 6 and stat[0]["total_ms"] > 0
