"""hg_pcs_verify_device_batch_bn254 / hg_claims_verify_batch_bn254: a run of BN254 openings verified in device passes of a group each.
The yardstick of every case is the host verifier (hg.pcs_verify_bn254 / hg.claims_verify_bn254 without a context) on that item alone,
compared exactly on decision and reason string. Every commitment and opening of the small cases is made by the host form."""
import ctypes as C
import os
import re

import pytest

import test_pcs_bn254 as tb
import test_pcs_verify_device_bn254 as tv
from test_pcs_bn254 import R
from hglib import hg, ROOT

GENERIC, WRAPPER = "hg_pcs_verify_device_batch_bn254", "hg_claims_verify_batch_bn254"
SENTINEL = 0x5a


def _last():
    return hg.lib().hg_last_error().decode()


# ---- not gpu ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in (GENERIC, WRAPPER):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name


class Outputs:
    """results and reasons filled with a sentinel byte, and whether they still hold it"""

    def __init__(self, n, cap=64):
        self.res = (C.c_int * max(n, 1))()
        self.reasons = C.create_string_buffer(max(n, 1) * cap)
        self.cap = cap
        C.memset(self.res, SENTINEL, C.sizeof(self.res))
        C.memset(self.reasons, SENTINEL, C.sizeof(self.reasons))

    def untouched(self):
        return bytes(self.res) == bytes([SENTINEL]) * C.sizeof(self.res) and self.reasons.raw == bytes([SENTINEL]) * C.sizeof(self.reasons)


def generic_args(items, nvars, log2_row, Q):
    """items: [(root, claims, proof)] -> the named arguments of hg_pcs_verify_device_batch_bn254 (ctx None) and what keeps them alive"""
    n = len(items)
    m = max(n, 1)
    arrays = [hg._pcs_claim_arrays_bn254(cl) for _, cl, _ in items]
    a = dict(ctx=None, roots=(C.c_char_p * m)(*[bytes(r) for r, _, _ in items]), nvars=(C.c_uint32 * len(nvars))(*nvars), n_tables=len(nvars), log2_row=log2_row,
             tables=(hg.u32p * m)(*[C.cast(x[0], hg.u32p) for x in arrays]), points=(hg.u64p * m)(*[hg._ptr(x[1]) for x in arrays]),
             values=(hg.u64p * m)(*[hg._ptr(x[2]) for x in arrays]), n_claims=(C.c_size_t * m)(*[len(cl) for _, cl, _ in items]), n_queries=Q,
             proofs=(C.c_char_p * m)(*[bytes(p) for _, _, p in items]), lens=(C.c_size_t * m)(*[len(p) for _, _, p in items]), n=n)
    return a, arrays


def call_generic(a, out):
    return hg.lib().hg_pcs_verify_device_batch_bn254(a["ctx"], a["roots"], a["nvars"], a["n_tables"], a["log2_row"], a["tables"], a["points"], a["values"], a["n_claims"],
                                                     a["n_queries"], a["proofs"], a["lens"], a["n"], out.res, out.reasons, out.cap)


def test_generic_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    c = tb.c2_case(15)
    nvars = c["nvars"]
    items = [(c["cm"].root, c["claims"], c["open35"])] * 3
    good, keep = generic_args(items, nvars, 2, 5)
    out = Outputs(3)
    assert call_generic(good, out) == -1 and _last() == GENERIC + ": no context" and out.untouched()

    held = [keep]

    def bad_item(claims):
        """the run with item 2's claims replaced"""
        held.append(generic_args(items[:2] + [(c["cm"].root, claims, c["open35"])], nvars, 2, 5))
        return held[-1]

    t, pt, v = c["claims"][0]
    cases = []
    for name in ("roots", "nvars", "n_claims", "proofs", "lens"):
        cases.append((dict(good, **{name: None}), "null argument", None))
    roots = (C.c_char_p * 3)(bytes(c["cm"].root), bytes(c["cm"].root), None)
    cases.append((dict(good, roots=roots), "null argument", 2))
    tables = (hg.u32p * 3)(good["tables"][0], good["tables"][1], None)
    cases.append((dict(good, tables=tables), "null argument", 2))
    cases.append((dict(good, nvars=(C.c_uint32 * 4)(5, 4, 3, 31)), "", None))                       # a shape outside the limits
    cases.append((dict(good, log2_row=3), "log2_row", None))                                         # log2_row above a table's variables
    cases.append((dict(good, n_queries=1 << 20), "queries", None))
    cases.append((dict(good, n_claims=(C.c_size_t * 3)(3, 3, 4097)), "more than 4096 claims", 2))
    cases.append((bad_item([(4, pt, v)] + c["claims"][1:])[0], "names table 4", 2))
    cases.append((bad_item([(t, [R] + pt[1:], v)] + c["claims"][1:])[0], "non-canonical coordinate", 2))   # a coordinate equal to r
    cases.append((bad_item([(t, pt, R)] + c["claims"][1:])[0], "non-canonical value", 2))                  # a value equal to r
    for args, text, index in cases:
        out = Outputs(3)
        assert call_generic(args, out) == -1, text
        assert _last().startswith(GENERIC + ": ") and text in _last() and "no context" not in _last(), _last()
        if index is not None:
            assert "index %d" % index in _last(), _last()
        assert out.untouched(), text
    # results is an argument too
    assert hg.lib().hg_pcs_verify_device_batch_bn254(None, good["roots"], good["nvars"], 4, 2, good["tables"], good["points"], good["values"], good["n_claims"], 5,
                                                     good["proofs"], good["lens"], 3, None, None, 0) == -1 and "null argument" in _last()
    # n == 0
    empty, _ = generic_args([], nvars, 2, 5)
    out = Outputs(1)
    assert call_generic(empty, out) == 0 and out.untouched()
    with pytest.raises(hg.HgError, match=GENERIC + ": no context"):
        hg.pcs_verify_batch_bn254(None, [c["cm"].root], nvars, [c["claims"]], [c["open35"]], 5, 2)
    assert hg.pcs_verify_batch_bn254(None, [], nvars, [], [], 5, 2) == []
    del held


def call_wrapper(a, out):
    return hg.lib().hg_claims_verify_batch_bn254(a["ctx"], a["params"], a["roots"], a["log2_row"], a["claims"], a["claim_cap_each"], a["points"], a["coord_cap_each"],
                                                 a["n_claims"], a["n_queries"], a["openings"], a["lens"], a["n"], out.res, out.reasons, out.cap)


def test_wrapper_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    w = tb.wrapper_case(1024, 1, 27)
    params, cl, k = w["bfv"].params, w["claims"], 1
    claims, nc1, points, nco1, counts = hg._claims_batch_arrays([cl, cl, cl], hg.InputClaimsBn254)
    assert isinstance(claims[0], hg.HgInputClaimBn254) and points.size == 4 * 3 * nco1
    good = dict(ctx=None, params=C.byref(params), roots=(C.c_char_p * 3)(*[bytes(w["cm"].root)] * 3), log2_row=0, claims=claims, claim_cap_each=nc1, points=hg._ptr(points),
                coord_cap_each=nco1, n_claims=counts, n_queries=0, openings=(C.c_char_p * 3)(*[bytes(w["opening"])] * 3), lens=(C.c_size_t * 3)(*[len(w["opening"])] * 3), n=3)
    out = Outputs(3)
    assert call_wrapper(good, out) == -1 and _last() == WRAPPER + ": no context" and out.untouched()

    def changed(field, value):
        """the run with claim 0 of item 2 changed"""
        other = (hg.HgInputClaimBn254 * len(claims))(*claims)
        setattr(other[2 * nc1], field, value)
        return dict(good, claims=other)

    cases = [(dict(good, **{name: None}), "null argument", None) for name in ("params", "roots", "claims", "points", "n_claims", "openings", "lens")]
    cases.append((dict(good, roots=(C.c_char_p * 3)(bytes(w["cm"].root), bytes(w["cm"].root), None)), "null argument", 2))
    cases.append((dict(good, log2_row=12), "log2_row", None))
    cases.append((dict(good, n_queries=1 << 20), "queries", None))
    cases.append((changed("input", 3), "is on input 3", 2))                      # a public input
    cases.append((changed("input", 3 + 2 * k + 1), "is on input %d" % (4 + 2 * k), 2))   # past 3 + 2k
    cases.append((changed("nvars", int(claims[2 * nc1].nvars) - 1), "coordinates", 2))
    cases.append((dict(good, n_claims=(C.c_size_t * 3)(counts[0], counts[1], nc1 + 1)), "claims in a block of", 2))
    for args, text, index in cases:
        out = Outputs(3)
        assert call_wrapper(args, out) == -1, text
        assert _last().startswith(WRAPPER + ": ") and text in _last() and "no context" not in _last(), _last()
        if index is not None:
            assert "index %d" % index in _last(), _last()
        assert out.untouched(), text
    out = Outputs(1)
    assert call_wrapper(dict(good, n=0), out) == 0 and out.untouched()
    with pytest.raises(hg.HgError, match=WRAPPER + ": no context"):
        hg.claims_verify_batch_bn254(None, params, [w["cm"].root], [cl], [w["opening"]])


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def host_of(items, nvars, Q, c):
    return [hg.pcs_verify_bn254(root, nvars, claims, proof, Q, c) for root, claims, proof in items]


def run(ctx, items, nvars, Q, c, reason_cap=256):
    return hg.pcs_verify_batch_bn254(ctx, [r for r, _, _ in items], nvars, [cl for _, cl, _ in items], [p for _, _, p in items], Q, c, reason_cap)


def own_item(nvars, c, n_claims, Q, seed):
    """an item with its own tables and root: (root, claims, the honest opening)"""
    tables = tb.make_tables(nvars, seed)
    cm = hg.Commitment.commit_bn254(None, tables, c)
    claims = tb.make_claims(tables, n_claims, seed + 1)
    return cm.root, claims, cm.open(claims, Q)


_MIXED = {}


def mixed_run():
    """The shape of tb.c2_case(15): [5, 4, 3, 2], c = 2 (R = 15), Q = 5. Eleven items, (tampered, honest form, the host's results of
    the tampered run), computed once. With Q = 5 and one to five jobs a member, 64 consecutive flat ids Q * job + q span several jobs
    and members."""
    if not _MIXED:
        c15 = tb.c2_case(15)
        nvars, Rn, Q, Cn = c15["nvars"], 15, 5, 4
        qb = 32 * Rn + 32 * 4
        counts = [3, 2, 4, 1, 0, 3, 2, 1, 4]
        honest = [own_item(nvars, 2, n, Q, 0xb00 + 16 * i) for i, n in enumerate(counts)]
        cols_at = lambda n: 32 * Cn * (n + 1)   # noqa: E731
        bad = list(honest)

        def tamper(i, fn):
            root, claims, proof = honest[i]
            bad[i] = fn(root, claims, proof, cols_at(len(claims)))
        tamper(1, lambda r, cl, p, ca: (r, cl, tv.flip(p, 32 * 2 + 31)))                         # u_0
        tamper(2, lambda r, cl, p, ca: (r, cl, tv.flip(p, 32 * Cn * 3 + 32 + 31)))               # u_3 (claim 2)
        tamper(3, lambda r, cl, p, ca: (r, cl, tv.flip(p, ca + 3 * qb + 32 * 5 + 31)))           # a column element of query 3
        tamper(4, lambda r, cl, p, ca: (r, cl, tv.flip(p, ca + 2 * qb + 32 * Rn + 32 * 2 + 9)))  # a sibling of query 2
        tamper(5, lambda r, cl, p, ca: (r, cl, tv.put(p, 32 * Cn + 32, R)))                      # an element = r in u_1
        tamper(6, lambda r, cl, p, ca: (r, cl, tv.put(p, ca + qb + 32 * 2, R)))                  # ... in a column of query 1
        tamper(7, lambda r, cl, p, ca: (r, cl, p + b"\0"))                                       # one byte too long
        tamper(8, lambda r, cl, p, ca: (bytes([r[0] ^ 1]) + r[1:], cl, p))                       # a changed root
        for kind in ("proximity", "claim"):                                                      # the transcript-consistent forgeries
            f = tv.forged_case(kind)
            bad.append((c15["cm"].root, f["claims"], f["proof"]))
            honest.append((c15["cm"].root, c15["claims"], c15["open35"]))
        _MIXED.update(nvars=nvars, Q=Q, bad=bad, honest=honest, host=host_of(bad, nvars, Q, 2))
    return _MIXED


@pytest.mark.gpu
def test_mixed_run_radix2_path(ctx):
    m = mixed_run()
    host = m["host"]
    assert len(host) == 11 and {len(cl) for _, cl, _ in m["bad"]} == {0, 1, 2, 3, 4} and len({r for r, _, _ in m["honest"][:9]}) == 9
    assert host[0] == (True, "") and not any(ok for ok, _ in host[1:])
    assert host[2][1] == "pcs: evaluation mismatch at claim 2" and host[3][1] == "pcs: Merkle path mismatch at query 3" and host[4][1] == "pcs: Merkle path mismatch at query 2"
    assert host[5][1] == "pcs: non-canonical word at byte %d" % (32 * 4 + 32) and host[6][1].startswith("pcs: non-canonical word") and "bytes" in host[7][1]
    assert host[9][1] == tv.forged_case("proximity")["want"] and host[10][1] == tv.forged_case("claim")["want"]
    assert len({why for _, why in host}) >= 8                       # the reasons differ: a result in the wrong slot would show
    assert run(ctx, m["bad"], m["nvars"], m["Q"], 2) == host
    a, keep = generic_args(m["bad"], m["nvars"], 2, m["Q"])         # the return value is the number of rejections
    out = Outputs(len(host), 256)
    assert call_generic(dict(a, ctx=ctx.h), out) == sum(1 for ok, _ in host if not ok) == 10
    assert [out.res[i] for i in range(len(host))] == [0] + [1] * 10
    assert out.reasons.raw[:256].split(b"\0", 1)[0] == b"" and out.reasons.raw[256:512].split(b"\0", 1)[0].decode() == host[1][1]
    del keep


@pytest.mark.gpu
def test_reasons_are_truncated_and_may_be_null(ctx):
    m = mixed_run()
    a, keep = generic_args(m["bad"], m["nvars"], 2, m["Q"])
    out = Outputs(len(m["bad"]), 8)
    assert call_generic(dict(a, ctx=ctx.h), out) == 10
    raw = out.reasons.raw
    assert [raw[8 * i:8 * i + 8].split(b"\0", 1)[0].decode() for i in range(len(m["bad"]))] == [why[:7] for _, why in m["host"]]
    res = (C.c_int * len(m["bad"]))()
    assert hg.lib().hg_pcs_verify_device_batch_bn254(ctx.h, a["roots"], a["nvars"], a["n_tables"], 2, a["tables"], a["points"], a["values"], a["n_claims"], m["Q"],
                                                     a["proofs"], a["lens"], a["n"], res, None, 0) == 10
    assert list(res) == [0] + [1] * 10
    del keep


@pytest.mark.gpu
def test_order_within_an_item(ctx):
    """two faults in one item, honest neighbours: the host's order decides which is reported"""
    c = tb.c2_case(15)
    nvars, root, Rn, Q, Cn, n = c["nvars"], c["cm"].root, 15, 5, 4, 4
    claims = tb.make_claims(c["tables"], n, 0x66)
    proof = c["cm"].open(claims, Q)
    qb, cols_at = 32 * Rn + 32 * 4, 32 * Cn * (n + 1)
    at = cols_at + 2 * qb + 32 * 6
    r_and_u1 = (root, claims, tv.flip(tv.put(proof, at, R), 32 * Cn * 2 + 32 + 31))
    t, pt, v = claims[0]
    value_and_sibling = (root, [(t, pt, (v + 1) % R)] + claims[1:], tv.flip(proof, cols_at + 32 * Rn + 32 + 9))
    neighbour = own_item(nvars, 2, 2, Q, 0xc40)
    items = [neighbour, r_and_u1, (root, claims, proof), value_and_sibling, neighbour]
    host = host_of(items, nvars, Q, 2)
    assert host == [(True, ""), (False, "pcs: non-canonical word at byte %d" % at), (True, ""), (False, "pcs: evaluation mismatch at claim 0"), (True, "")]
    assert run(ctx, items, nvars, Q, 2) == host


@pytest.mark.gpu
def test_canonicity_over_all_four_limbs_in_a_member_other_than_0(ctx):
    """an element that is not below r in member 1 of three, differing from r in each limb in turn: the offset is the member's own"""
    m = mixed_run()
    nvars, Q, Rn, Cn = m["nvars"], m["Q"], 15, 4
    root, claims, proof = m["honest"][2]                 # 4 claims; the members around it have 3 and 1
    qb, cols_at = 32 * Rn + 32 * 4, 32 * Cn * (len(claims) + 1)
    u_at, col_at = 32 * Cn * 2 + 32, cols_at + 3 * qb + 32 * 7      # an element of u_2, a column element of query 3
    for value in (R, R + (1 << 64), R + (1 << 192), (1 << 256) - 1):
        for at in (u_at, col_at):
            items = [m["honest"][0], (root, claims, tv.put(proof, at, value)), m["honest"][3]]
            host = host_of(items, nvars, Q, 2)
            assert host == [(True, ""), (False, "pcs: non-canonical word at byte %d" % at), (True, "")]
            assert run(ctx, items, nvars, Q, 2) == host, (hex(value), at)


@pytest.mark.gpu
def test_isolation(ctx):
    """each tampered item replaced in turn by its honest form: the others keep their results; one honest opening four times"""
    m = mixed_run()
    for i in range(1, len(m["bad"])):
        items = list(m["bad"])
        items[i] = m["honest"][i]
        want = list(m["host"])
        want[i] = (True, "")
        assert run(ctx, items, m["nvars"], m["Q"], 2) == want, i
    assert run(ctx, [m["honest"][0]] * 4, m["nvars"], m["Q"], 2) == [(True, "")] * 4


@pytest.mark.gpu
def test_grouping(ctx):
    m = mixed_run()
    items = [m["bad"][0], m["bad"][2], m["bad"][9], m["honest"][3], m["bad"][6]]   # groups of 2: a rejection in each of (0,1) (2,3) (4)
    host = host_of(items, m["nvars"], m["Q"], 2)
    assert [ok for ok, _ in host] == [True, False, False, True, False]
    try:
        for G in (0, 2, 1):
            ctx.set_option("verify_batch_group", G)
            assert run(ctx, items, m["nvars"], m["Q"], 2) == host, G
    finally:
        ctx.set_option("verify_batch_group", 0)


@pytest.mark.gpu
def test_four_step_path(ctx):
    """c = 6: Enc(u_i) is the LDS four-step NTT of size 256, one batch over the 5 + 1 + 3 rows of the three members"""
    nvars = [8, 7, 6]
    items = [own_item(nvars, 6, n, 0, 0xd00 + 16 * i) for i, n in enumerate((4, 0, 2))]
    root, claims, proof = items[0]
    assert len(proof) == hg.pcs_opening_bytes_bn254(nvars, 4, 0, 6)
    items[0] = (root, claims, tv.flip(proof, 32 * 64 * 2 + 31))     # a byte of u_2
    host = host_of(items, nvars, 0, 6)
    assert host == [(False, "pcs: evaluation mismatch at claim 1"), (True, ""), (True, "")]
    assert run(ctx, items, nvars, 0, 6) == host


@pytest.mark.gpu
def test_boundaries(ctx):
    """R = 129, Q = 257: member 1 starts at thread 257 of the per-query kernels and every job takes two workgroups of the inner
    products, the second with one active lane; member 1's last query is the faulty one"""
    nvars, Q = [9, 2], 257
    items = [own_item(nvars, 2, 2, Q, 0xe00 + 16 * i) for i in range(2)]
    root, claims, proof = items[1]
    items[1] = (root, claims, tv.flip(proof, tv.last_column_element(nvars, 2, 2, Q) + 31))
    want = [(True, ""), (False, "pcs: Merkle path mismatch at query 256")]
    assert host_of(items, nvars, Q, 2) == want
    assert run(ctx, items, nvars, Q, 2) == want


@pytest.mark.gpu
def test_one_row_past_a_reduction_chunk(ctx):
    """nvars [12, 2] at c = 2: R = 1025 = BNPCS_CHUNK + 1. Acceptance needs every inner product to equal the encoded u: a dropped or
    doubled row rejects."""
    nvars, Q = [12, 2], 3
    items = [own_item(nvars, 2, 2, Q, 0xf00 + 16 * i) for i in range(2)]
    assert host_of(items, nvars, Q, 2) == [(True, ""), (True, "")]
    assert run(ctx, items, nvars, Q, 2) == [(True, ""), (True, "")]
    root, claims, proof = items[1]
    items[1] = (root, claims, tv.flip(proof, tv.last_column_element(nvars, 2, 2, Q) + 31))
    want = [(True, ""), (False, "pcs: Merkle path mismatch at query 2")]
    assert host_of(items, nvars, Q, 2) == want
    assert run(ctx, items, nvars, Q, 2) == want


def proven(ctx, bfv, pk, seeds, cap=1 << 24):
    """witnesses of the seeds proven over BN254 and publicly verified as a batch: (witnesses, the claims per item)"""
    ws = [hg.Witness.synthetic(bfv.params, s) for s in seeds]
    proofs = [ctx.prove_bn254(pk, w, cap=cap)[0] for w in ws]
    got = hg.verify_public_batch_bn254(ctx, pk, [hg.Instance.from_witness(w) for w in ws], proofs)
    assert all(ok for ok, _, _ in got), got
    return ws, [cl for _, _, cl in got]


@pytest.mark.gpu
def test_wrapper(ctx):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    ws, cls = proven(ctx, bfv, pk, (0xa11, 0xa12, 0xa13))
    cms = [hg.Commitment.secrets_bn254(ctx, bfv.params, w) for w in ws]
    roots = [cm.root for cm in cms]
    openings = [cm.open_claims(bfv.params, cl) for cm, cl in zip(cms, cls)]
    assert hg.claims_verify_batch_bn254(ctx, bfv.params, roots, cls, openings) == [(True, "")] * 3
    swapped = [openings[1], openings[0], openings[2]]
    host = [hg.claims_verify_bn254(bfv.params, r, cl, o) for r, cl, o in zip(roots, cls, swapped)]
    assert [ok for ok, _ in host] == [False, False, True]
    assert hg.claims_verify_batch_bn254(ctx, bfv.params, roots, cls, swapped) == host
    public = (hg.HgInputClaimBn254 * cls[1].n)(*cls[1].claims[:cls[1].n])
    public[0].input = 3
    with pytest.raises(hg.HgError, match=WRAPPER + r": index 1: claim 0 is on input 3"):
        hg.claims_verify_batch_bn254(ctx, bfv.params, roots, [cls[0], hg.InputClaimsBn254(public, cls[1].n, cls[1].points), cls[2]], openings)
    pk.free()


@pytest.mark.gpu
def test_headline_shape_once(ctx):
    """(32768,16), the headline set itself: 47 claims, c = 11, R = 864, 241 queries, two members: one four-step NTT of 2^13 over 96 rows"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk = bfv.setup(ctx)
    ws, cls = proven(ctx, bfv, pk, (0x8000 + 16, 0x8000 + 17), cap=1 << 25)
    cms = [hg.Commitment.secrets_bn254(ctx, bfv.params, w) for w in ws]
    assert cms[0].log2_row == 11 and cls[0].n == cls[1].n == 47
    roots = [cm.root for cm in cms]
    openings = [cm.open_claims(bfv.params, cl) for cm, cl in zip(cms, cls)]
    cols_at, qb = 32 * 2048 * 48, 32 * 864 + 32 * 13
    assert len(openings[1]) == cols_at + 241 * qb
    openings[1] = tv.flip(openings[1], cols_at + 200 * qb + 32 * 863 + 31)
    host = [hg.claims_verify_bn254(bfv.params, r, cl, o) for r, cl, o in zip(roots, cls, openings)]
    assert host == [(True, ""), (False, "pcs: Merkle path mismatch at query 200")]
    assert hg.claims_verify_batch_bn254(ctx, bfv.params, roots, cls, openings) == host
    pk.free()


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    m = mixed_run()
    ctx.profile(2)
    ctx.profile_reset()
    try:
        assert run(ctx, m["bad"], m["nvars"], m["Q"], 2) == m["host"]
        stat = [s for s in ctx.profile_get(256) if s["name"] == "pcs_bn254_verify_batch"]
    finally:
        ctx.profile(0)
    assert len(stat) == 1 and stat[0]["launches"] >= 6 and stat[0]["total_ms"] > 0
