"""hg_pcs_verify_device_bn254 / hg_claims_verify_device_bn254: the verifier of a BN254 opening on a context. The yardstick is the host
verifier: on every input the device form's (decision, reason) equals hg_pcs_verify_bn254's, which tests/test_pcs_bn254.py holds against
the Python restatement (py_verify); at the c = 2 sizes py_verify is compared here as well. Honest openings on both encoding paths and
around the reduction chunk, the tampering matrix, canonicity over all four limbs, wrong but transcript-consistent openings built by a
Python prover (the two reasons a flipped byte cannot reach) and pairs of faults, where the host's order decides which is reported."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import test_pcs_bn254 as tb
from test_pcs_bn254 import R
from hglib import hg, ROOT

NEW = ["hg_pcs_verify_device_bn254", "hg_claims_verify_device_bn254"]
be32 = tb.be32


def _last():
    return hg.lib().hg_last_error().decode()


def flip(proof, at, mask=0x01):
    b = bytearray(proof)
    b[at] ^= mask
    return bytes(b)


def put(proof, at, value):
    """the 32-byte element at byte `at` replaced by `value` (any integer below 2^256)"""
    return proof[:at] + be32(value) + proof[at + 32:]


# ---- the prover of include/hg.h in Python integers, with a handle on u ----------------------------------------------------------
def py_open(py, claims, Q, which=None, delta=None):
    """The opening of `claims` against the Python commitment. which / delta: vector `which` of u_0 (proximity), u_1 .. u_n (claim
    which - 1) has `delta` (C elements) added BEFORE it enters the transcript, and a claim's value is recomputed from its changed
    vector, so the opening is wrong but consistent with its own transcript. -> (bytes, the claims as opened, the column indices)"""
    c, nvars = py.c, py.nvars
    Cn, N, Rn = 1 << c, 4 << c, len(py.rows)
    claims = list(claims)
    us = [None]
    for k, (t, pt, val) in enumerate(claims):
        w = tb.eq_table(pt[c:])
        u = [tb.dot(w, [py.rows[py.off[t] + r][j] for r in range(len(w))]) for j in range(Cn)]
        if which == k + 1:
            u = [(a + b) % R for a, b in zip(u, delta)]
            claims[k] = (t, pt, tb.dot(tb.eq_table(pt[:c]), u))
        us.append(u)
    tr = tb.PyTranscript(py.root, c, nvars, Q, claims)
    rho = tr.squeeze()
    us[0] = [tb.dot([pow(rho, r, R) for r in range(Rn)], [row[j] for row in py.rows]) for j in range(Cn)]
    if which == 0:
        us[0] = [(a + b) % R for a, b in zip(us[0], delta)]
    out = b""
    for u in us:
        for x in u:
            out += be32(x)
            tr.absorb(x)
    js = [(tr.squeeze() & 0xFFFFFFFFFFFFFFFF) & (N - 1) for _ in range(Q)]
    for j in js:
        out += b"".join(be32(m[j]) for m in py.M)
        out += b"".join(py.levels[lv][(j >> lv) ^ 1] for lv in range(c + 2))
    return out, claims, js


_FORGED = {}


def forged_case(kind):
    """R = 15, c = 2, Q = 5: "proximity": u_0 + e; "claim": the vector of claim 2 + e with the value recomputed. e has one non-zero
    element, so Enc(e) vanishes nowhere and the first query is the one that fails."""
    if kind not in _FORGED:
        c = tb.c2_case(15)
        e = [0, (3 << 200) + 5, 0, 0]
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


def sub(args, i, v):
    return args[:i] + (v,) + args[i + 1:]


def test_no_context_and_bad_arguments_of_the_raw_entry():
    L = hg._pcs_protos()
    c = tb.c2_case(15)
    nv = (C.c_uint32 * 4)(*c["nvars"])
    table, pts, vals = hg._pcs_claim_arrays_bn254(c["claims"])
    proof = c["open35"]
    good = (None, c["cm"].root, nv, 4, 2, table, hg._ptr(pts), hg._ptr(vals), 3, 5, proof, len(proof))
    assert L.hg_pcs_verify_device_bn254(*good) == -1 and _last() == "hg_pcs_verify_device_bn254: no context"
    far = (C.c_uint32 * 3)(0, 4, 2)                              # a table index out of range
    big = pts.copy()
    big[4:8] = hg.Context._fr_pack([R])                          # a coordinate equal to r
    for args, text in ((sub(good, 1, None), "null argument"), (sub(good, 2, None), "null argument"), (sub(good, 5, far), "names table 4"),
                       (sub(good, 6, hg._ptr(big)), "non-canonical coordinate"), (sub(good, 4, 3), "log2_row"), (sub(good, 9, 1 << 20), "queries")):
        assert L.hg_pcs_verify_device_bn254(*args) == -1, args
        assert _last().startswith("hg_pcs_verify_device_bn254: ") and text in _last(), _last()
    with pytest.raises(hg.HgError, match="hg_pcs_verify_device_bn254: no context"):
        hg.pcs_verify_bn254(c["cm"].root, c["nvars"], c["claims"], proof, 5, 2, ctx=type("NoCtx", (), {"h": None})())
    assert L.hg_pcs_verify_bn254(*good[1:]) == 0                 # the same arguments are the host form's


def test_no_context_and_bad_arguments_of_the_wrapper():
    L = hg._pcs_protos()
    w = tb.wrapper_case(1024, 1, 27)
    params, cl = w["bfv"].params, w["claims"]
    vgood = (None, C.byref(params), w["cm"].root, 0, cl.claims, cl.n, hg._ptr(cl.points), 0, w["opening"], len(w["opening"]))
    assert L.hg_claims_verify_device_bn254(*vgood) == -1 and _last() == "hg_claims_verify_device_bn254: no context"
    public = (hg.HgInputClaimBn254 * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3                                          # a claim on ais[0]
    for args in (sub(vgood, 1, None), sub(vgood, 2, None), sub(vgood, 4, None), sub(vgood, 4, public), sub(vgood, 3, 12)):
        assert L.hg_claims_verify_device_bn254(*args) == -1 and _last().startswith("hg_claims_verify_device_bn254: ") and "no context" not in _last(), _last()


def test_the_python_prover_is_the_librarys():
    c = tb.c2_case(15)
    honest, claims, _ = py_open(c["py"], c["claims"], 5)
    assert honest == c["open35"] and claims == c["claims"]


@pytest.mark.parametrize("kind", ["proximity", "claim"])
def test_transcript_consistent_wrong_openings_reach_the_two_late_reasons_on_the_host(kind):
    """what the device form is compared with in the GPU case below: the host verifier and py_verify give the intended text"""
    c, f = tb.c2_case(15), forged_case(kind)
    assert tb.py_verify(c["py"].root, c["nvars"], 2, f["claims"], 5, f["proof"]) == f["want"]
    assert hg.pcs_verify_bn254(c["cm"].root, c["nvars"], f["claims"], f["proof"], 5, 2) == (False, f["want"])


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def both(ctx, root, nvars, claims, proof, Q, c):
    """(decision, reason) of the host form, after asserting the device form's is the same"""
    host = hg.pcs_verify_bn254(root, nvars, claims, proof, Q, c)
    dev = hg.pcs_verify_bn254(root, nvars, claims, proof, Q, c, ctx=ctx)
    assert dev == host, (dev, host)
    return host


@pytest.mark.gpu
@pytest.mark.parametrize("Rn", [4, 5, 8, 15, 16])
def test_honest_openings_radix2_path(ctx, Rn):
    """log2n = 4; 4R + 1 hashed words: the padding alone in a block (R = 4), in one word (R = 8), apart (R = 5, 15, 16)"""
    c = tb.c2_case(Rn)
    assert both(ctx, c["cm"].root, c["nvars"], c["claims"], c["open35"], 5, 2) == (True, "")
    assert both(ctx, c["cm"].root, c["nvars"], [], c["open01"], 1, 2) == (True, "")
    assert tb.py_verify(c["py"].root, c["nvars"], 2, c["claims"], 5, c["open35"]) == ""


@pytest.mark.gpu
@pytest.mark.parametrize("nvars", [[8, 7, 6], [11]])
def test_honest_openings_four_step_path(ctx, nvars):
    """c = 6: Enc(u_i) is the LDS four-step NTT of size 256; 241 indices below 256 repeat"""
    assert hg.pcs_row_log2(nvars, 6) == 6 and 8 <= 6 + 2 <= 16
    tables = tb.make_tables(nvars, 0xd6c6 + len(nvars))
    cm = hg.Commitment.commit_bn254(None, tables, 6)
    claims = tb.make_claims(tables, 4, 5)
    proof = cm.open(claims)
    assert len(proof) == hg.pcs_opening_bytes_bn254(nvars, 4, 0, 6)
    assert both(ctx, cm.root, nvars, claims, proof, 0, 6) == (True, "")
    assert both(ctx, cm.root, nvars, claims, flip(proof, 32 * 64 * 2 + 31), 0, 6) == (False, "pcs: evaluation mismatch at claim 1")   # a byte of u_2


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [14, 15])
def test_the_upper_edge_of_the_four_step_range(ctx, nv):
    """one row of 2^nv elements: log2n = 16 is the last four-step size, log2n = 17 takes the radix-2 stages above it"""
    tables = tb.make_tables([nv], 0xd7c7 + nv)
    cm = hg.Commitment.commit_bn254(None, tables, nv)
    claims = tb.make_claims(tables, 1, 6)
    proof = cm.open(claims, 6)
    assert both(ctx, cm.root, [nv], claims, proof, 6, nv) == (True, "")
    assert both(ctx, cm.root, [nv], claims, flip(proof, 32 * ((1 << nv) + 5) + 31), 6, nv) == (False, "pcs: evaluation mismatch at claim 0")


def last_column_element(nvars, c, n, Q):
    """the byte offset of the last column element of the last query"""
    Rn = sum(1 << (v - c) for v in nvars)
    return 32 * (1 << c) * (n + 1) + (Q - 1) * (32 * Rn + 32 * (c + 2)) + 32 * (Rn - 1)


@pytest.mark.gpu
def test_one_row_past_a_reduction_chunk(ctx):
    """nvars [12, 2] at c = 2: R = 1025, the column's inner product is one row past a chunk of 1024, claim 0's exactly one chunk.
    Acceptance needs every inner product to equal the encoded u: a dropped or doubled row rejects."""
    nvars, Q = [12, 2], 3
    tables = tb.make_tables(nvars, 0xd025)
    cm = hg.Commitment.commit_bn254(None, tables, 2)
    claims = tb.make_claims(tables, 2, 11)
    proof = cm.open(claims, Q)
    assert both(ctx, cm.root, nvars, claims, proof, Q, 2) == (True, "")
    bad = flip(proof, last_column_element(nvars, 2, 2, Q) + 31)
    assert both(ctx, cm.root, nvars, claims, bad, Q, 2) == (False, "pcs: Merkle path mismatch at query 2")


@pytest.mark.gpu
def test_two_reduction_chunks_of_the_largest_elements(ctx):
    """nvars [13] at c = 2, every element r - 1: R = 2048, two whole chunks for the column's job and for the claim's"""
    table = np.tile(hg.Context._fr_pack([R - 1]), 1 << 13)
    cm = hg.Commitment.commit_bn254(None, [table], 2)
    rng = random.Random(0xc0b2)
    claims = [(0, [rng.randrange(R) for _ in range(13)], R - 1)]   # the eq weights sum to one
    proof = cm.open(claims, 3)
    assert both(ctx, cm.root, [13], claims, proof, 3, 2) == (True, "")
    bad = flip(proof, last_column_element([13], 2, 1, 3) + 31)
    assert both(ctx, cm.root, [13], claims, bad, 3, 2) == (False, "pcs: Merkle path mismatch at query 2")


@pytest.mark.gpu
def test_one_query_past_a_workgroup(ctx):
    """R = 129, Q = 257: one query past a workgroup of 256, with duplicate indices at code length 16. The single entry launches the
    inner-product kernel of the batch form: two workgroups a job here, and Q no multiple of 64 (every weight table is a part of one
    reduction chunk of 1024 rows at this R; two whole chunks with two workgroups a job are the case below)"""
    nvars, Q = [9, 2], 257
    tables = tb.make_tables(nvars, 0xd129)
    cm = hg.Commitment.commit_bn254(None, tables, 2)
    claims = tb.make_claims(tables, 2, 9)
    proof = cm.open(claims, Q)
    Rn, qb, cols_at = 129, 32 * 129 + 32 * 4, 32 * 4 * 3
    assert len(proof) == cols_at + Q * qb
    assert both(ctx, cm.root, nvars, claims, proof, Q, 2) == (True, "")
    assert both(ctx, cm.root, nvars, claims, flip(proof, cols_at + 256 * qb + 32 * (Rn - 1) + 31), Q, 2) == (False, "pcs: Merkle path mismatch at query 256")


@pytest.mark.gpu
def test_two_workgroups_a_job_over_two_reduction_chunks(ctx):
    """nvars [13] at c = 2, Q = 257: R = 2048, so the column's job and the claim's are two whole chunks of 1024 rows each, and every
    job takes two workgroups, the second with one query"""
    nvars, Q = [13], 257
    tables = tb.make_tables(nvars, 0xd257)
    cm = hg.Commitment.commit_bn254(None, tables, 2)
    claims = tb.make_claims(tables, 1, 13)
    proof = cm.open(claims, Q)
    assert both(ctx, cm.root, nvars, claims, proof, Q, 2) == (True, "")
    bad = flip(proof, last_column_element(nvars, 2, 1, Q) + 31)
    assert both(ctx, cm.root, nvars, claims, bad, Q, 2) == (False, "pcs: Merkle path mismatch at query 256")


def checker(ctx, nvars, Q):
    def check(root_, claims_, proof_, allowed):
        ok, why = both(ctx, root_, nvars, claims_, proof_, Q, 2)
        assert not ok and why in allowed, (why, allowed)
        assert why == tb.py_verify(root_, nvars, 2, claims_, Q, proof_)
    return check


@pytest.mark.gpu
def test_the_tampering_matrix(ctx):
    Rn, c = 15, tb.c2_case(15)
    nvars, claims, proof, root = c["nvars"], c["claims"], c["open35"], c["cm"].root
    n, Q, Cn = 3, 5, 4
    qb, cols_at = 32 * Rn + 32 * 4, 32 * Cn * (n + 1)
    path0 = {"pcs: Merkle path mismatch at query 0", "pcs: proximity mismatch at query 0"}   # the indices move with the transcript
    check = checker(ctx, nvars, Q)
    check(root, claims, flip(proof, 32 * 2 + 31), path0)                                                          # u_0
    for i in range(n):
        check(root, claims, flip(proof, 32 * Cn * (i + 1) + 32 + 31), {"pcs: evaluation mismatch at claim %d" % i})   # u_i
    for q in (0, 3):
        check(root, claims, flip(proof, cols_at + q * qb + 32 * 5 + 31), {"pcs: Merkle path mismatch at query %d" % q})            # a column element
        check(root, claims, flip(proof, cols_at + q * qb + 32 * Rn + 32 * 2 + 9), {"pcs: Merkle path mismatch at query %d" % q})   # a sibling
    for i in range(n):                                                                                             # a changed value
        bad = [(t, pt, (v + 1) % R if k == i else v) for k, (t, pt, v) in enumerate(claims)]
        check(root, bad, proof, {"pcs: evaluation mismatch at claim %d" % i})
    for coord, allowed in ((0, {"pcs: evaluation mismatch at claim 0"}), (2, path0)):                              # a coordinate below c / from c on
        t, pt, v = claims[0]
        bad = list(claims)
        bad[0] = (t, pt[:coord] + [(pt[coord] + 1) % R] + pt[coord + 1:], v)
        check(root, bad, proof, allowed)
    check(bytes([root[0] ^ 1]) + root[1:], claims, proof, {"pcs: Merkle path mismatch at query 0"})                # a changed root
    want = len(proof)
    check(root, claims, proof + b"\0", {"pcs: the opening has %d bytes, %d expected" % (want + 1, want)})
    check(root, claims, proof[:-1], {"pcs: the opening has %d bytes, %d expected" % (want - 1, want)})


@pytest.mark.gpu
def test_canonicity_is_decided_over_all_four_limbs(ctx):
    Rn, c = 15, tb.c2_case(15)
    nvars, claims, proof, root = c["nvars"], c["claims"], c["open35"], c["cm"].root
    n, Q, Cn = 3, 5, 4
    qb, cols_at = 32 * Rn + 32 * 4, 32 * Cn * (n + 1)
    check = checker(ctx, nvars, Q)
    u_at, col_at = 32 * Cn * 2 + 32, cols_at + 3 * qb + 32 * 7      # an element of u_2, a column element of query 3
    for value in (R, R + 1, (1 << 256) - 1):
        for at in (u_at, col_at):
            check(root, claims, put(proof, at, value), {"pcs: non-canonical word at byte %d" % at})
    # the top limb below r's, the three lower limbs all ones: below r, so it fails later, with the host's reason
    low_ones = (((R >> 192) - 1) << 192) | ((1 << 192) - 1)
    assert low_ones < R
    check(root, claims, put(proof, u_at, low_ones), {"pcs: evaluation mismatch at claim 1"})
    check(root, claims, put(proof, col_at, low_ones), {"pcs: Merkle path mismatch at query 3"})
    # the top limb equal to r's and a lower limb above r's: not below r
    check(root, claims, put(proof, col_at, R + (1 << 64)), {"pcs: non-canonical word at byte %d" % col_at})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["proximity", "claim"])
def test_the_two_reasons_flips_cannot_reach(ctx, kind):
    c, f = tb.c2_case(15), forged_case(kind)
    assert both(ctx, c["cm"].root, c["nvars"], f["claims"], f["proof"], 5, 2) == (False, f["want"])


@pytest.mark.gpu
def test_order_with_several_faults(ctx):
    Rn, c = 15, tb.c2_case(15)
    nvars, root = c["nvars"], c["cm"].root
    claims = tb.make_claims(c["tables"], 4, 0x66)
    n, Q, Cn = 4, 5, 4
    proof = c["cm"].open(claims, Q)
    qb, cols_at = 32 * Rn + 32 * 4, 32 * Cn * (n + 1)
    assert both(ctx, root, nvars, claims, proof, Q, 2) == (True, "")
    u_at = lambda i: 32 * Cn * (i + 1) + 32 + 31        # noqa: E731  a byte of claim i's vector
    sib_at = lambda q: cols_at + q * qb + 32 * Rn + 32 + 9   # noqa: E731
    # a sibling at query 1, a column element at query 3
    bad = flip(flip(proof, sib_at(1)), cols_at + 3 * qb + 32 * 4 + 31)
    assert both(ctx, root, nvars, claims, bad, Q, 2) == (False, "pcs: Merkle path mismatch at query 1")
    # an element = r in a column of query 2, a flipped u_1
    at = cols_at + 2 * qb + 32 * 6
    bad = flip(put(proof, at, R), u_at(1))
    assert both(ctx, root, nvars, claims, bad, Q, 2) == (False, "pcs: non-canonical word at byte %d" % at)
    # u_3 and u_1
    bad = flip(flip(proof, u_at(3)), u_at(1))
    assert both(ctx, root, nvars, claims, bad, Q, 2) == (False, "pcs: evaluation mismatch at claim 1")
    # the value of claim 0 and a sibling
    t, pt, v = claims[0]
    wrong = [(t, pt, (v + 1) % R)] + claims[1:]
    assert both(ctx, root, nvars, wrong, flip(proof, sib_at(0)), Q, 2) == (False, "pcs: evaluation mismatch at claim 0")


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,bits", tb.WRAPPER_SHAPES)
def test_wrappers(ctx, n, k, bits):
    w = tb.wrapper_case(n, k, bits)
    params, cl, cm, opening = w["bfv"].params, w["claims"], w["cm"], w["opening"]
    assert hg.claims_verify_bn254(params, cm.root, cl, opening) == (True, "")
    assert hg.claims_verify_bn254(params, cm.root, cl, opening, ctx=ctx) == (True, "")
    # the opening of another witness (of its own claims: the same count, so the same length)
    pk = w["bfv"].setup(ctx)
    w2 = hg.Witness.synthetic(params, 0x1c5 + n)
    ok, why, cl2 = hg.verify_public_bn254(pk, hg.Instance.from_witness(w2), ctx.prove_bn254(pk, w2)[0], ctx=ctx, device=True)
    assert ok, why
    cm2 = hg.Commitment.secrets_bn254(ctx, params, w2)
    opening2 = cm2.open_claims(params, cl2)
    assert cm2.root != cm.root and len(opening2) == len(opening)
    host = hg.claims_verify_bn254(params, cm.root, cl, opening2)
    assert not host[0] and host[1].startswith("pcs: ")
    assert hg.claims_verify_bn254(params, cm.root, cl, opening2, ctx=ctx) == host
    # a claim on a public input
    public = (hg.HgInputClaimBn254 * cl.n)(*cl.claims[:cl.n])
    public[0].input = 3
    with pytest.raises(hg.HgError, match=r"hg_claims_verify_device_bn254: claim 0 is on input 3"):
        hg.claims_verify_bn254(params, cm.root, hg.InputClaimsBn254(public, cl.n, cl.points), opening, ctx=ctx)
    pk.free()


@pytest.mark.gpu
def test_headline_size_once(ctx):
    """(32768,16): c = 11, R = 864, 241 queries: the four-step NTT of 2^13 over n + 1 rows, 204 Keccak blocks a column"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk, w = bfv.setup(ctx), hg.Witness.synthetic(bfv.params, 0x8000 + 16)
    proof = ctx.prove_bn254(pk, w, cap=1 << 25)[0]
    ok, why, cl = hg.verify_public_bn254(pk, hg.Instance.from_witness(w), proof, ctx=ctx, device=True)
    assert ok, why
    assert cl.n == hg.pk_claim_shape(pk)[0]
    cm = hg.Commitment.secrets_bn254(ctx, bfv.params, w)
    assert cm.log2_row == 11
    opening = cm.open_claims(bfv.params, cl)
    cols_at, qb = 32 * 2048 * (cl.n + 1), 32 * 864 + 32 * 13
    assert len(opening) == cols_at + 241 * qb
    assert hg.claims_verify_bn254(bfv.params, cm.root, cl, opening, ctx=ctx) == (True, "")
    bad = flip(opening, cols_at + 200 * qb + 32 * 863 + 31)
    host = hg.claims_verify_bn254(bfv.params, cm.root, cl, bad)
    assert host == (False, "pcs: Merkle path mismatch at query 200")
    assert hg.claims_verify_bn254(bfv.params, cm.root, cl, bad, ctx=ctx) == host
    pk.free()


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    c = tb.c2_case(15)
    ctx.profile(2)
    ctx.profile_reset()
    try:
        assert hg.pcs_verify_bn254(c["cm"].root, c["nvars"], c["claims"], c["open35"], 5, 2, ctx=ctx) == (True, "")
        stat = [s for s in ctx.profile_get() if s["name"] == "pcs_bn254_verify"]
    finally:
        ctx.profile(0)
    assert len(stat) == 1 and stat[0]["launches"] >= 6 and stat[0]["total_ms"] > 0
