"""hg_pcs_open_batch_bn254 / hg_claims_open_batch_bn254: a run of BN254 openings made in device passes of a group of items each. The
yardstick for the bytes is the host form (hg.Commitment.commit_bn254(None, ..) and its .open) on that item alone; for a refused
item's text it is the single device call (Commitment.open on a device handle), whose error the slot must repeat exactly."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import test_pcs as tp
import test_pcs_bn254 as tb
from orclib import R_BN as R
from hglib import hg, ROOT

GENERIC, WRAPPER = "hg_pcs_open_batch_bn254", "hg_claims_open_batch_bn254"
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
    """openings, lengths, status and reasons filled with a sentinel byte, and whether they still hold it"""

    def __init__(self, n, cap_each, reason_cap=64):
        m = max(n, 1)
        self.n, self.cap_each, self.reason_cap = n, cap_each, reason_cap
        self.buf = np.full(m * max(cap_each, 1), SENTINEL, dtype=np.uint8)
        self.lens, self.status = (C.c_size_t * m)(), (C.c_int * m)()
        self.reasons = C.create_string_buffer(m * reason_cap)
        for x in (self.lens, self.status, self.reasons):
            C.memset(x, SENTINEL, C.sizeof(x))

    def slot(self, i):
        return self.buf[i * self.cap_each:(i + 1) * self.cap_each].tobytes()

    def reason(self, i):
        return self.reasons.raw[i * self.reason_cap:(i + 1) * self.reason_cap].split(b"\0", 1)[0].decode()

    def untouched(self):
        return (self.buf == SENTINEL).all() and all(bytes(x) == bytes([SENTINEL]) * C.sizeof(x) for x in (self.lens, self.status)) and \
            self.reasons.raw == bytes([SENTINEL]) * C.sizeof(self.reasons)


def generic_args(items, Q):
    """items: [(Commitment, claims)] -> the named arguments of hg_pcs_open_batch_bn254 (ctx None) and what keeps them alive"""
    m = max(len(items), 1)
    arrays = [hg._pcs_claim_arrays_bn254(cl) for _, cl in items]
    a = dict(ctx=None, commitments=(C.c_void_p * m)(*[cm.h for cm, _ in items]), tables=(hg.u32p * m)(*[C.cast(x[0], hg.u32p) for x in arrays]),
             points=(hg.u64p * m)(*[hg._ptr(x[1]) for x in arrays]), values=(hg.u64p * m)(*[hg._ptr(x[2]) for x in arrays]),
             n_claims=(C.c_size_t * m)(*[len(cl) for _, cl in items]), n_queries=Q, n=len(items))
    return a, arrays


def call_generic(a, out, **over):
    o = dict(openings=out.buf.ctypes.data_as(hg.u8p), lens=out.lens, status=out.status, reasons=out.reasons, cap_each=out.cap_each, reason_cap=out.reason_cap)
    o.update(over)
    return hg.lib().hg_pcs_open_batch_bn254(a["ctx"], a["commitments"], a["tables"], a["points"], a["values"], a["n_claims"], a["n_queries"], a["n"], o["openings"],
                                            o["cap_each"], o["lens"], o["status"], o["reasons"], o["reason_cap"])


def goldilocks_host_handle():
    return hg.Commitment.commit(None, [np.arange(8, dtype=np.uint64), np.arange(4, dtype=np.uint64)], 2)


def test_generic_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    c = tb.c2_case(15)
    # host-form handles are all a machine without a device has, and each is an error: the faults below lie at index 0, ahead of it
    items = [(c["cm"], c["claims"])] * 3
    good, keep = generic_args(items, 5)
    cap = len(c["open35"])
    cases = [(good, {}, "the commitment was made by the host form", 0)]
    gl = goldilocks_host_handle()
    mixed = (C.c_void_p * 3)(gl.h, c["cm"].h, c["cm"].h)
    cases.append((dict(good, commitments=mixed), {}, "the commitment is over Goldilocks: open it with hg_pcs_open_batch", 0))
    cases.append((dict(good, commitments=(C.c_void_p * 3)(None, c["cm"].h, c["cm"].h)), {}, "null argument", 0))
    cases.append((dict(good, tables=(hg.u32p * 3)(None, good["tables"][1], good["tables"][2])), {}, "null argument", 0))
    cases.append((dict(good, values=None), {}, "null argument", 0))
    for name in ("commitments", "n_claims"):
        cases.append((dict(good, **{name: None}), {}, "null argument", None))
    for name in ("openings", "lens", "status"):
        cases.append((good, {name: None}, "null argument", None))
    cases.append((dict(good, n_queries=1 << 20), {}, "queries", None))
    for args, over, text, index in cases:
        out = Outputs(3, cap)
        assert call_generic(args, out, **over) == -1, text
        assert _last().startswith(GENERIC + ": ") and text in _last() and "no context" not in _last(), _last()
        if index is not None:
            assert "index %d" % index in _last(), _last()
        assert out.untouched(), text
    out = Outputs(1, cap)
    assert call_generic(dict(good, n=0), out) == 0 and out.untouched()
    assert hg.pcs_open_batch_bn254(None, [], []) == []
    with pytest.raises(hg.HgError, match=GENERIC + ": index 0: the commitment was made by the host form"):
        hg.pcs_open_batch_bn254(None, [c["cm"]], [c["claims"]], 5)
    del keep


def call_wrapper(a, out, **over):
    o = dict(openings=out.buf.ctypes.data_as(hg.u8p), lens=out.lens, status=out.status, reasons=out.reasons, cap_each=out.cap_each, reason_cap=out.reason_cap)
    o.update(over)
    return hg.lib().hg_claims_open_batch_bn254(a["ctx"], a["params"], a["commitments"], a["claims"], a["claim_cap_each"], a["points"], a["coord_cap_each"], a["n_claims"],
                                               a["n_queries"], a["n"], o["openings"], o["cap_each"], o["lens"], o["status"], o["reasons"], o["reason_cap"])


def test_wrapper_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    w = tb.wrapper_case(1024, 1, 27)
    params, cl = w["bfv"].params, w["claims"]
    claims, nc1, points, nco1, counts = hg._claims_batch_arrays([cl, cl, cl], hg.InputClaimsBn254)
    good = dict(ctx=None, params=C.byref(params), commitments=(C.c_void_p * 3)(*[w["cm"].h] * 3), claims=claims, claim_cap_each=nc1, points=hg._ptr(points),
                coord_cap_each=nco1, n_claims=counts, n_queries=0, n=3)
    cap = len(w["opening"])
    gl = goldilocks_host_handle()
    cases = [(good, {}, "the commitment was made by the host form", 0)]
    cases.append((dict(good, commitments=(C.c_void_p * 3)(gl.h, w["cm"].h, w["cm"].h)), {}, "the commitment is over Goldilocks: open it with hg_claims_open_batch", 0))
    cases.append((dict(good, commitments=(C.c_void_p * 3)(None, w["cm"].h, w["cm"].h)), {}, "null argument", 0))
    cases.append((dict(good, claims=None), {}, "null argument", 0))
    cases.append((dict(good, points=None), {}, "null argument", 0))
    for name in ("params", "commitments", "n_claims"):
        cases.append((dict(good, **{name: None}), {}, "null argument", None))
    for name in ("openings", "lens", "status"):
        cases.append((good, {name: None}, "null argument", None))
    cases.append((dict(good, n_queries=1 << 20), {}, "queries", None))
    for args, over, text, index in cases:
        out = Outputs(3, cap)
        assert call_wrapper(args, out, **over) == -1, text
        assert _last().startswith(WRAPPER + ": ") and text in _last() and "no context" not in _last(), _last()
        if index is not None:
            assert "index %d" % index in _last(), _last()
        assert out.untouched(), text
    out = Outputs(1, cap)
    assert call_wrapper(dict(good, n=0), out) == 0 and out.untouched()
    assert hg.claims_open_batch_bn254(None, params, [], []) == []


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def wrong(claims, i):
    """claim i with its value raised by one"""
    t, pt, v = claims[i]
    return claims[:i] + [(t, pt, (v + 1) % R)] + claims[i + 1:]


_MIXED = {}


def mixed_run(ctx):
    """Shape [6, 2], c = 2 (R = 17), Q = 5: five members with their own tables and 0 .. 4 claims; the host form's commitments and
    openings, the device handles (made as one batch), and the run with members 1 and 3 made faulty. Computed once."""
    if not _MIXED:
        nvars, Q, counts = [6, 2], 5, [0, 3, 1, 4, 2]
        tables = [tb.make_tables(nvars, 0xf00 + 16 * i) for i in range(5)]
        host = [hg.Commitment.commit_bn254(None, t, 2) for t in tables]
        claims = [tb.make_claims(t, n, 0xf08 + 16 * i) for i, (t, n) in enumerate(zip(tables, counts))]
        dev = hg.Commitment.commit_batch_bn254(ctx, tables, 2)
        faulty = list(claims)
        faulty[1] = wrong(claims[1], 2)
        faulty[3] = wrong(wrong(claims[3], 3), 0)
        _MIXED.update(nvars=nvars, Q=Q, tables=tables, host=host, dev=dev, claims=claims, faulty=faulty, want=[h.open(cl, Q) for h, cl in zip(host, claims)])
    return _MIXED


def single_text(cm, claims, Q):
    """what the single device call leaves in hg_last_error for these claims"""
    with pytest.raises(hg.HgError) as e:
        cm.open(claims, Q)
    return str(e.value)


@pytest.mark.gpu
def test_mixed_run(ctx):
    m = mixed_run(ctx)
    assert sorted(len(cl) for cl in m["claims"]) == [0, 1, 2, 3, 4] and len(set(m["want"])) == 5
    assert [cm.root for cm in m["dev"]] == [h.root for h in m["host"]]
    assert hg.pcs_open_batch_bn254(ctx, m["dev"], m["claims"], m["Q"]) == [(b, "") for b in m["want"]]
    a, keep = generic_args(list(zip(m["dev"], m["claims"])), m["Q"])
    cap = max(len(b) for b in m["want"]) + 24
    out = Outputs(5, cap, 256)
    assert call_generic(dict(a, ctx=ctx.h), out) == 0
    assert list(out.status) == [0] * 5 and list(out.lens) == [len(b) for b in m["want"]]
    for i, b in enumerate(m["want"]):
        assert out.slot(i) == b + bytes([SENTINEL]) * (cap - len(b)) and out.reason(i) == "", i
    # handles of single commits open to the same bytes in the same run
    singles = [hg.Commitment.commit_bn254(ctx, t, 2) for t in m["tables"][:2]]
    assert hg.pcs_open_batch_bn254(ctx, singles + m["dev"][2:], m["claims"], m["Q"]) == [(b, "") for b in m["want"]]
    del keep


@pytest.mark.gpu
def test_refusal(ctx):
    m = mixed_run(ctx)
    Q = m["Q"]
    texts = {i: single_text(m["dev"][i], m["faulty"][i], Q) for i in (1, 3)}
    assert texts[1] == "hg_pcs_open_bn254: claim 2: the value is not the evaluation of table 0 at the point"
    assert texts[3] == "hg_pcs_open_bn254: claim 0: the value is not the evaluation of table 0 at the point"      # the lowest failing claim
    want = [(b, "") for b in m["want"]]
    want[1], want[3] = (None, texts[1]), (None, texts[3])
    assert hg.pcs_open_batch_bn254(ctx, m["dev"], m["faulty"], Q) == want
    a, keep = generic_args(list(zip(m["dev"], m["faulty"])), Q)
    cap = max(len(b) for b in m["want"])
    for reason_cap, reasons in ((256, True), (8, True), (0, False)):
        out = Outputs(5, cap, max(reason_cap, 1))
        over = {} if reasons else dict(reasons=None, reason_cap=0)
        assert call_generic(dict(a, ctx=ctx.h), out, **over) == 2
        assert list(out.status) == [0, 1, 0, 1, 0] and list(out.lens) == [len(m["want"][0]), 0, len(m["want"][2]), 0, len(m["want"][4])]
        for i in (1, 3):
            assert out.slot(i) == bytes([SENTINEL]) * cap, i                                               # a refused item's buffer is untouched
        for i in (0, 2, 4):
            assert out.slot(i)[:len(m["want"][i])] == m["want"][i], i
        if reasons:
            assert [out.reason(i) for i in range(5)] == [w[1][:reason_cap - 1] for w in want]
        else:
            assert out.reasons.raw == bytes([SENTINEL]) * C.sizeof(out.reasons)
    # each faulty item replaced in turn by its honest form: only that item changes
    for i in (1, 3):
        claims = list(m["faulty"])
        claims[i] = m["claims"][i]
        w = list(want)
        w[i] = (m["want"][i], "")
        assert hg.pcs_open_batch_bn254(ctx, m["dev"], claims, Q) == w, i
    del keep


@pytest.mark.gpu
def test_combine_across_its_reduction_chunk_with_the_largest_elements(ctx):
    """one table of 2^13 elements in rows of 4: 2048 rows, two reduction chunks of 1024; every element r - 1; the claim's value is
    r - 1 at every point (the eq weights sum to one). Two members, the second with the claim and without"""
    table = np.tile(hg.Context._fr_pack([R - 1]), 1 << 13)
    host = hg.Commitment.commit_bn254(None, [table], 2)
    dev = hg.Commitment.commit_batch_bn254(ctx, [[table], [table]], 2)
    assert [cm.root for cm in dev] == [host.root] * 2
    rng = random.Random(0xc0b2)
    claims = [[(0, [rng.randrange(R) for _ in range(13)], R - 1)], []]
    got = hg.pcs_open_batch_bn254(ctx, dev, claims, 3)
    assert got == [(host.open(cl, 3), "") for cl in claims]
    assert hg.pcs_verify_bn254(host.root, [13], claims[0], got[0][0], 3, 2) == (True, "")


@pytest.mark.gpu
def test_eval_over_the_high_coordinates(ctx):
    """[10], c = 9: one row of 512 elements; the evaluation check folds coordinate 8 per entry beside the eight a thread keeps"""
    tables = [tb.make_tables([10], 0xc90 + 16 * i) for i in range(2)]
    host = [hg.Commitment.commit_bn254(None, t, 9) for t in tables]
    dev = hg.Commitment.commit_batch_bn254(ctx, tables, 9)
    claims = [tb.make_claims(t, 2, 0xc98 + 16 * i) for i, t in enumerate(tables)]
    assert hg.pcs_open_batch_bn254(ctx, dev, claims, 4) == [(h.open(cl, 4), "") for h, cl in zip(host, claims)]
    faulty = [claims[0], wrong(claims[1], 1)]
    assert hg.pcs_open_batch_bn254(ctx, dev, faulty, 4) == [(host[0].open(claims[0], 4), ""), (None, single_text(dev[1], faulty[1], 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [257, 0])
def test_boundaries(ctx, Q):
    """R = 17; Q = 257: a member's gather starts inside a workgroup (257 * 17 is no multiple of 256); Q = 0: the default 241. One
    handle four times with different claims."""
    m = mixed_run(ctx)
    host, dev, claims = m["host"][1:3], m["dev"][1:3], m["claims"][1:3]
    assert hg.pcs_open_batch_bn254(ctx, dev, claims, Q) == [(h.open(cl, Q), "") for h, cl in zip(host, claims)]
    four = [claims[0], [], claims[0][1:], claims[0][:1]]
    assert hg.pcs_open_batch_bn254(ctx, [dev[0]] * 4, four, Q) == [(host[0].open(cl, Q), "") for cl in four]


@pytest.mark.gpu
def test_c6_with_claims_on_all_three_tables(ctx):
    nvars = [8, 7, 6]
    tables = [tb.make_tables(nvars, 0xd40 + 16 * i) for i in range(3)]
    host = [hg.Commitment.commit_bn254(None, t, 6) for t in tables]
    dev = hg.Commitment.commit_batch_bn254(ctx, tables, 6)
    claims = [tb.make_claims(t, n, 0xd48 + 16 * i) for i, (t, n) in enumerate(zip(tables, (4, 3, 0)))]
    assert {t for t, _, _ in claims[0]} == {0, 1, 2}
    assert hg.pcs_open_batch_bn254(ctx, dev, claims, 9) == [(h.open(cl, 9), "") for h, cl in zip(host, claims)]
    faulty = [claims[0], wrong(claims[1], 1), claims[2]]
    got = hg.pcs_open_batch_bn254(ctx, dev, faulty, 9)
    assert got[1] == (None, single_text(dev[1], faulty[1], 9)) and got[0] == (host[0].open(claims[0], 9), "") and got[2] == (host[2].open([], 9), "")


@pytest.mark.gpu
def test_grouping(ctx):
    m = mixed_run(ctx)
    want = [(b, "") for b in m["want"]]
    want[1], want[3] = (None, single_text(m["dev"][1], m["faulty"][1], m["Q"])), (None, single_text(m["dev"][3], m["faulty"][3], m["Q"]))
    try:
        for G in (0, 2, 1):
            ctx.set_option("verify_batch_group", G)
            assert hg.pcs_open_batch_bn254(ctx, m["dev"], m["faulty"], m["Q"]) == want, G
    finally:
        ctx.set_option("verify_batch_group", 0)


@pytest.mark.gpu
def test_errors_of_the_call_that_need_a_device_handle(ctx):
    m = mixed_run(ctx)
    Q, dev, claims = m["Q"], m["dev"], m["claims"]
    items = list(zip(dev[:3], claims[:3]))
    good, keep = generic_args(items, Q)
    good = dict(good, ctx=ctx.h)
    cap = max(len(b) for b in m["want"][:3])
    held = [keep]

    def with_item(i, cm, cl):
        held.append(generic_args(items[:i] + [(cm, cl)] + items[i + 1:], Q))
        return dict(held[-1][0], ctx=ctx.h)

    t, pt, v = claims[1][0]
    other_shape = hg.Commitment.commit_bn254(ctx, tb.c2_case(15)["tables"], 2)
    goldilocks = hg.Commitment.commit(ctx, tp.make_tables(m["nvars"], 0xa70), 2)
    other = hg.Context(0)
    try:
        elsewhere = hg.Commitment.commit_bn254(other, m["tables"][2], 2)
        cases = [(dict(good, ctx=None), {}, "no context", None),
                 (with_item(2, m["host"][2], claims[2]), {}, "the commitment was made by the host form", 2),
                 (with_item(1, goldilocks, []), {}, "the commitment is over Goldilocks: open it with hg_pcs_open_batch", 1),
                 (with_item(2, other_shape, []), {}, "shape", 2),
                 (with_item(2, elsewhere, claims[2]), {}, "another context", 2),
                 (with_item(1, dev[1], [(2, pt, v)] + claims[1][1:]), {}, "names table 2", 1),
                 (with_item(1, dev[1], [(t, [R] + pt[1:], v)] + claims[1][1:]), {}, "non-canonical coordinate", 1),
                 (with_item(1, dev[1], [(t, pt, R)] + claims[1][1:]), {}, "non-canonical value", 1),
                 (dict(good, n_claims=(C.c_size_t * 3)(0, 4097, 1)), {}, "more than 4096 claims", 1),
                 (good, dict(cap_each=cap - 1), "%d bytes" % cap, None)]
        for args, over, text, index in cases:
            out = Outputs(3, cap)
            assert call_generic(args, out, **over) == -1, text
            assert _last().startswith(GENERIC + ": ") and text in _last(), _last()
            if index is not None:
                assert "index %d" % index in _last(), _last()
            assert out.untouched(), text
        assert call_generic(dict(good, ctx=None), Outputs(3, cap)) == -1 and _last() == GENERIC + ": no context"
        elsewhere.free()
    finally:
        other.close()
    out = Outputs(3, cap)
    assert call_generic(good, out) == 0 and [out.slot(i)[:out.lens[i]] for i in range(3)] == m["want"][:3]    # the context still works
    del held


@pytest.mark.gpu
def test_wrapper_end_to_end(ctx):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    params = bfv.params
    ws = [hg.Witness.synthetic(params, s) for s in (0xb11, 0xb12, 0xb13)]
    proofs = [ctx.prove_bn254(pk, w)[0] for w in ws]
    got = hg.verify_public_batch_bn254(ctx, pk, [hg.Instance.from_witness(w) for w in ws], proofs)
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    cms = hg.Commitment.secrets_batch_bn254(ctx, params, ws)
    roots = [cm.root for cm in cms]
    opened = hg.claims_open_batch_bn254(ctx, params, cms, cls)
    assert all(b is not None and why == "" for b, why in opened)
    openings = [b for b, _ in opened]
    assert hg.claims_verify_batch_bn254(ctx, params, roots, cls, openings) == [(True, "")] * 3
    for w, cm, cl, o in zip(ws, cms, cls, openings):
        one = hg.Commitment.secrets_bn254(None, params, w)                                                 # the host form of the single call
        assert one.root == cm.root and one.open_claims(params, cl) == o and cm.open_claims(params, cl) == o
    # an item without claims opens to the proximity-only opening; a wrong value is refused with hg_claims_open_bn254's text
    spoiled = (hg.HgInputClaimBn254 * cls[2].n)(*cls[2].claims[:cls[2].n])
    spoiled[1].value[0] = spoiled[1].value[0] ^ 1
    bad = hg.InputClaimsBn254(spoiled, cls[2].n, cls[2].points)
    with pytest.raises(hg.HgError) as e:
        cms[2].open_claims(params, bad)
    assert str(e.value).startswith("hg_claims_open_bn254: claim 1: the value is not the evaluation")
    got = hg.claims_open_batch_bn254(ctx, params, cms, [cls[0], None, bad])
    assert got == [(openings[0], ""), (cms[1].open([]), ""), (None, str(e.value))]
    generic = hg.Commitment.commit_bn254(ctx, tb.c2_case(15)["tables"], 2)
    with pytest.raises(hg.HgError, match=WRAPPER + r": index 2: the commitment's shape differs"):
        hg.claims_open_batch_bn254(ctx, params, cms[:2] + [generic], cls)
    with pytest.raises(hg.HgError, match=WRAPPER + r": index 0: the commitment is not hg_secrets_commit_bn254's for these parameters"):
        hg.claims_open_batch_bn254(ctx, params, [generic], [None])
    pk.free()


@pytest.mark.gpu
def test_headline_shape_once(ctx):
    """(32768,16): c = 11, R = 864, 241 queries, two members"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk = bfv.setup(ctx)
    params = bfv.params
    ws = [hg.Witness.synthetic(params, s) for s in (0x8000 + 26, 0x8000 + 27)]
    proofs = [ctx.prove_bn254(pk, w, cap=1 << 25)[0] for w in ws]
    got = hg.verify_public_batch_bn254(ctx, pk, [hg.Instance.from_witness(w) for w in ws], proofs)
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    cms = hg.Commitment.secrets_batch_bn254(ctx, params, ws)
    assert cms[0].log2_row == 11 and cls[0].n == cls[1].n > 0
    # (226 MB of encoded rows a member: the group's encoding runs as two slices through one member's temporary)
    assert [cm.root for cm in cms] == [hg.Commitment.secrets_bn254(ctx, params, w).root for w in ws]
    opened = hg.claims_open_batch_bn254(ctx, params, cms, cls)
    assert [why for _, why in opened] == ["", ""]
    for cm, cl, (b, _) in zip(cms, cls, opened):
        assert len(b) == hg.pcs_opening_bytes_bn254(cm.nvars, cl.n) == 32 * 2048 * (cl.n + 1) + 241 * (32 * 864 + 32 * 13)
        assert hg.claims_verify_bn254(params, cm.root, cl, b) == (True, "")
    pk.free()


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    m = mixed_run(ctx)
    ctx.profile(2)
    ctx.profile_reset()
    try:
        assert hg.pcs_open_batch_bn254(ctx, m["dev"], m["claims"], m["Q"]) == [(b, "") for b in m["want"]]
        stat = [s for s in ctx.profile_get(256) if s["name"] == "pcs_bn254_open_batch"]
    finally:
        ctx.profile(0)
    assert len(stat) == 1 and stat[0]["launches"] >= 4 and stat[0]["total_ms"] > 0
