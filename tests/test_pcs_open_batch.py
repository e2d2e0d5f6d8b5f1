"""hg_pcs_open_batch / hg_claims_open_batch: a run of openings made in device passes of a group of items each. The yardstick for the
bytes is the host form (hg.Commitment.commit(None, ..) and its .open) on that item alone; for a refused item's text it is the single
device call (Commitment.open on a device handle), whose error the slot must repeat exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_pcs as tp
from hglib import hg, ROOT

P = hg.P
GENERIC, WRAPPER = "hg_pcs_open_batch", "hg_claims_open_batch"
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
    """items: [(Commitment, claims)] -> the named arguments of hg_pcs_open_batch (ctx None) and what keeps them alive"""
    m = max(len(items), 1)
    arrays = [hg._pcs_claim_arrays(cl) for _, cl in items]
    a = dict(ctx=None, commitments=(C.c_void_p * m)(*[cm.h for cm, _ in items]), tables=(hg.u32p * m)(*[C.cast(x[0], hg.u32p) for x in arrays]),
             points=(hg.u64p * m)(*[hg._ptr(x[1]) for x in arrays]), values=(hg.u64p * m)(*[hg._ptr(x[2]) for x in arrays]),
             n_claims=(C.c_size_t * m)(*[len(cl) for _, cl in items]), n_queries=Q, n=len(items))
    return a, arrays


def call_generic(a, out, **over):
    o = dict(openings=out.buf.ctypes.data_as(hg.u8p), lens=out.lens, status=out.status, reasons=out.reasons, cap_each=out.cap_each, reason_cap=out.reason_cap)
    o.update(over)
    return hg.lib().hg_pcs_open_batch(a["ctx"], a["commitments"], a["tables"], a["points"], a["values"], a["n_claims"], a["n_queries"], a["n"], o["openings"], o["cap_each"],
                                      o["lens"], o["status"], o["reasons"], o["reason_cap"])


def bn254_host_handle():
    return hg.Commitment.commit_bn254(None, [[1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11, 12]], 2)


def test_generic_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    c = tp.c2_case(15)
    # host-form handles are all a machine without a device has, and each is an error: the faults below lie at index 0, ahead of it
    items = [(c["cm"], c["claims"])] * 3
    good, keep = generic_args(items, 5)
    cap = len(c["open35"])
    cases = [(good, {}, "the commitment was made by the host form", 0)]
    bn = bn254_host_handle()
    mixed = (C.c_void_p * 3)(bn.h, c["cm"].h, c["cm"].h)
    cases.append((dict(good, commitments=mixed), {}, "the commitment is over BN254", 0))
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
    assert hg.pcs_open_batch(None, [], []) == []
    with pytest.raises(hg.HgError, match=GENERIC + ": index 0: the commitment was made by the host form"):
        hg.pcs_open_batch(None, [c["cm"]], [c["claims"]], 5)
    del keep


def call_wrapper(a, out, **over):
    o = dict(openings=out.buf.ctypes.data_as(hg.u8p), lens=out.lens, status=out.status, reasons=out.reasons, cap_each=out.cap_each, reason_cap=out.reason_cap)
    o.update(over)
    return hg.lib().hg_claims_open_batch(a["ctx"], a["params"], a["commitments"], a["claims"], a["claim_cap_each"], a["points"], a["coord_cap_each"], a["n_claims"],
                                         a["n_queries"], a["n"], o["openings"], o["cap_each"], o["lens"], o["status"], o["reasons"], o["reason_cap"])


def test_wrapper_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    w = tp.wrapper_case(1024, 1, 27)
    params, cl = w["bfv"].params, w["claims"]
    claims, nc1, points, nco1, counts = hg._claims_batch_arrays([cl, cl, cl])
    good = dict(ctx=None, params=C.byref(params), commitments=(C.c_void_p * 3)(*[w["cm"].h] * 3), claims=claims, claim_cap_each=nc1, points=hg._ptr(points),
                coord_cap_each=nco1, n_claims=counts, n_queries=0, n=3)
    cap = len(w["opening"])
    bn = bn254_host_handle()
    cases = [(good, {}, "the commitment was made by the host form", 0)]
    cases.append((dict(good, commitments=(C.c_void_p * 3)(bn.h, w["cm"].h, w["cm"].h)), {}, "the commitment is over BN254", 0))
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
    assert hg.claims_open_batch(None, params, [], []) == []


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def wrong(claims, i):
    """claim i with its value's first word raised by one"""
    t, pt, v = claims[i]
    return claims[:i] + [(t, pt, ((v[0] + 1) % P, v[1]))] + claims[i + 1:]


_MIXED = {}


def mixed_run(ctx):
    """Shape [6, 2], c = 2 (R = 17), Q = 5: five members with their own tables and 0 .. 4 claims; the host form's commitments and
    openings, the device handles (made as one batch), and the run with members 1 and 3 made faulty. Computed once."""
    if not _MIXED:
        nvars, Q, counts = [6, 2], 5, [0, 3, 1, 4, 2]
        tables = [tp.make_tables(nvars, 0xf00 + 16 * i) for i in range(5)]
        host = [hg.Commitment.commit(None, t, 2) for t in tables]
        claims = [tp.make_claims(t, n, 0xf08 + 16 * i) for i, (t, n) in enumerate(zip(tables, counts))]
        dev = hg.Commitment.commit_batch(ctx, tables, 2)
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
    assert hg.pcs_open_batch(ctx, m["dev"], m["claims"], m["Q"]) == [(b, "") for b in m["want"]]
    a, keep = generic_args(list(zip(m["dev"], m["claims"])), m["Q"])
    cap = max(len(b) for b in m["want"]) + 24
    out = Outputs(5, cap, 256)
    assert call_generic(dict(a, ctx=ctx.h), out) == 0
    assert list(out.status) == [0] * 5 and list(out.lens) == [len(b) for b in m["want"]]
    for i, b in enumerate(m["want"]):
        assert out.slot(i) == b + bytes([SENTINEL]) * (cap - len(b)) and out.reason(i) == "", i
    # handles of single commits open to the same bytes in the same run
    singles = [hg.Commitment.commit(ctx, t, 2) for t in m["tables"][:2]]
    assert hg.pcs_open_batch(ctx, singles + m["dev"][2:], m["claims"], m["Q"]) == [(b, "") for b in m["want"]]
    del keep


@pytest.mark.gpu
def test_refusal(ctx):
    m = mixed_run(ctx)
    Q = m["Q"]
    texts = {i: single_text(m["dev"][i], m["faulty"][i], Q) for i in (1, 3)}
    assert texts[1] == "hg_pcs_open: claim 2: the value is not the evaluation of table 0 at the point"
    assert texts[3] == "hg_pcs_open: claim 0: the value is not the evaluation of table 0 at the point"      # the lowest failing claim
    want = [(b, "") for b in m["want"]]
    want[1], want[3] = (None, texts[1]), (None, texts[3])
    assert hg.pcs_open_batch(ctx, m["dev"], m["faulty"], Q) == want
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
        assert hg.pcs_open_batch(ctx, m["dev"], claims, Q) == w, i
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [257, 0])
def test_boundaries(ctx, Q):
    """R = 129 (three reduction chunks); Q = 257: a member's gather starts inside a workgroup; Q = 0: the default 241. One handle four
    times with different claims."""
    nvars = [9, 2]
    tables = [tp.make_tables(nvars, 0xe40 + 16 * i) for i in range(2)]
    host = [hg.Commitment.commit(None, t, 2) for t in tables]
    dev = hg.Commitment.commit_batch(ctx, tables, 2)
    claims = [tp.make_claims(t, 2, 0xe48 + 16 * i) for i, t in enumerate(tables)]
    assert hg.pcs_open_batch(ctx, dev, claims, Q) == [(h.open(cl, Q), "") for h, cl in zip(host, claims)]
    four = [claims[0], [], claims[0][1:], claims[0][:1]]
    assert hg.pcs_open_batch(ctx, [dev[0]] * 4, four, Q) == [(host[0].open(cl, Q), "") for cl in four]


@pytest.mark.gpu
def test_c6_with_claims_on_all_three_tables(ctx):
    nvars = [8, 7, 6]
    tables = [tp.make_tables(nvars, 0xd40 + 16 * i) for i in range(3)]
    host = [hg.Commitment.commit(None, t, 6) for t in tables]
    dev = hg.Commitment.commit_batch(ctx, tables, 6)
    claims = [tp.make_claims(t, n, 0xd48 + 16 * i) for i, (t, n) in enumerate(zip(tables, (4, 3, 0)))]
    assert {t for t, _, _ in claims[0]} == {0, 1, 2}
    assert hg.pcs_open_batch(ctx, dev, claims, 9) == [(h.open(cl, 9), "") for h, cl in zip(host, claims)]
    faulty = [claims[0], wrong(claims[1], 1), claims[2]]
    got = hg.pcs_open_batch(ctx, dev, faulty, 9)
    assert got[1] == (None, single_text(dev[1], faulty[1], 9)) and got[0] == (host[0].open(claims[0], 9), "") and got[2] == (host[2].open([], 9), "")


@pytest.mark.gpu
def test_grouping(ctx):
    m = mixed_run(ctx)
    want = hg.pcs_open_batch(ctx, m["dev"], m["faulty"], m["Q"])
    assert [b is None for b, _ in want] == [False, True, False, True, False]
    try:
        for G in (2, 1):
            ctx.set_option("verify_batch_group", G)
            assert hg.pcs_open_batch(ctx, m["dev"], m["faulty"], m["Q"]) == want, G
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
    other_shape = hg.Commitment.commit(ctx, tp.c2_case(15)["tables"], 2)
    other = hg.Context(0)
    try:
        elsewhere = hg.Commitment.commit(other, m["tables"][2], 2)
        cases = [(dict(good, ctx=None), {}, "no context", None),
                 (with_item(2, other_shape, []), {}, "shape", 2),
                 (with_item(2, elsewhere, claims[2]), {}, "another context", 2),
                 (with_item(1, dev[1], [(2, pt, v)] + claims[1][1:]), {}, "names table 2", 1),
                 (with_item(1, dev[1], [(t, [P] + pt[1:], v)] + claims[1][1:]), {}, "non-canonical coordinate", 1),
                 (with_item(1, dev[1], [(t, pt, (v[0], P))] + claims[1][1:]), {}, "non-canonical value", 1),
                 (dict(good, n_claims=(C.c_size_t * 3)(0, 4097, 1)), {}, "more than 4096 claims", 1),
                 (good, dict(cap_each=cap - 8), "%d bytes" % cap, None)]
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
    proofs = [bfv.prove(ctx, pk, w, mode=3)[0] for w in ws]
    got = hg.verify_public_batch(ctx, pk, [hg.Instance.from_witness(w) for w in ws], proofs, 3)
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    cms = hg.Commitment.secrets_batch(ctx, params, ws)
    roots = [cm.root for cm in cms]
    opened = hg.claims_open_batch(ctx, params, cms, cls)
    assert all(b is not None and why == "" for b, why in opened)
    openings = [b for b, _ in opened]
    assert hg.claims_verify_batch(ctx, params, roots, cls, openings) == [(True, "")] * 3
    for w, cm, cl, o in zip(ws, cms, cls, openings):
        assert hg.claims_verify(params, cm.root, cl, o) == (True, "")
        one = hg.Commitment.secrets(ctx, params, w)
        assert one.root == cm.root and one.open_claims(params, cl) == o
    # an item without claims opens to the proximity-only opening; a wrong value is refused with hg_claims_open's text
    spoiled = (hg.HgInputClaim * cls[2].n)(*cls[2].claims[:cls[2].n])
    spoiled[1].value[0] = (spoiled[1].value[0] + 1) % P
    bad = hg.InputClaims(spoiled, cls[2].n, cls[2].points)
    with pytest.raises(hg.HgError) as e:
        cms[2].open_claims(params, bad)
    assert str(e.value).startswith("hg_claims_open: claim 1: the value is not the evaluation")
    got = hg.claims_open_batch(ctx, params, cms, [cls[0], None, bad])
    assert got == [(openings[0], ""), (cms[1].open([]), ""), (None, str(e.value))]
    assert hg.claims_verify(params, roots[1], hg.InputClaims((hg.HgInputClaim * 1)(), 0, np.zeros(1, dtype=np.uint64)), got[1][0]) == (True, "")
    public = (hg.HgInputClaim * cls[1].n)(*cls[1].claims[:cls[1].n])
    public[0].input = 3
    with pytest.raises(hg.HgError, match=WRAPPER + r": index 1: claim 0 is on input 3"):
        hg.claims_open_batch(ctx, params, cms, [cls[0], hg.InputClaims(public, cls[1].n, cls[1].points), cls[2]])
    generic = hg.Commitment.commit(ctx, tp.c2_case(15)["tables"], 2)
    with pytest.raises(hg.HgError, match=WRAPPER + r": index 2: the commitment's shape differs"):
        hg.claims_open_batch(ctx, params, cms[:2] + [generic], cls)
    with pytest.raises(hg.HgError, match=WRAPPER + r": index 0: the commitment is not hg_secrets_commit's for these parameters"):
        hg.claims_open_batch(ctx, params, [generic], [None])
    pk.free()


@pytest.mark.gpu
def test_headline_shape_once(ctx):
    """(32768,16): 47 claims, c = 11, R = 864, 241 queries, two members"""
    bfv = hg.BfvEncrypt.new(32768, 16)
    pk = bfv.setup(ctx)
    params = bfv.params
    ws = [hg.Witness.synthetic(params, s) for s in (0x8000 + 26, 0x8000 + 27)]
    proofs = [bfv.prove(ctx, pk, w, cap=1 << 25, mode=0)[0] for w in ws]
    got = hg.verify_public_batch(ctx, pk, [hg.Instance.from_witness(w) for w in ws], proofs, 0)
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    cms = hg.Commitment.secrets_batch(ctx, params, ws)
    assert cms[0].log2_row == 11 and cls[0].n == cls[1].n == 47
    singles = [hg.Commitment.secrets(ctx, params, w) for w in ws]
    assert [cm.root for cm in cms] == [cm.root for cm in singles]
    opened = hg.claims_open_batch(ctx, params, cms, cls)
    assert [why for _, why in opened] == ["", ""]
    for one, cl, (b, _) in zip(singles, cls, opened):
        assert b == one.open_claims(params, cl)
    assert hg.claims_verify_batch(ctx, params, [cm.root for cm in cms], cls, [b for b, _ in opened]) == [(True, "")] * 2
    pk.free()


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    m = mixed_run(ctx)
    ctx.profile(2)
    ctx.profile_reset()
    try:
        assert hg.pcs_open_batch(ctx, m["dev"], m["claims"], m["Q"]) == [(b, "") for b in m["want"]]
        stat = [s for s in ctx.profile_get(256) if s["name"] == "pcs_open_batch"]
    finally:
        ctx.profile(0)
    assert len(stat) == 1 and stat[0]["launches"] >= 4 and stat[0]["total_ms"] > 0
