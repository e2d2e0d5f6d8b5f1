"""hg_pcs_open_folded_batch_bn254 / hg_claims_open_folded_batch_bn254 / hg_pcs_verify_folded_device_batch_bn254 /
hg_claims_verify_folded_batch_bn254: folded BN254 openings opened and verified for a run in device passes of a group each. The
yardstick of every opening is the single call (Commitment.open_folded on the same device handle) and the host form on a host
commitment of the same tables, byte for byte, with py_verify_folded_bn254 of test_pcs_folded_bn254.py accepting it; the yardstick of
every decision is the host verifier hg.pcs_verify_folded_bn254 on that item alone, compared exactly on decision and reason string.
Q = 5 throughout."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_pcs_bn254 as tb
import test_pcs_folded_bn254 as tf
import test_pcs_open_batch_bn254 as tob
import test_pcs_verify_batch_bn254 as tvb
from hglib import hg, ROOT
from orclib import R_BN as R
from test_pcs_folded_bn254 import claims_on, py_verify_folded_bn254
from test_pcs_bn254 import make_tables

Q = 5
OPEN, OPEN_W = "hg_pcs_open_folded_batch_bn254", "hg_claims_open_folded_batch_bn254"
VERIFY, VERIFY_W = "hg_pcs_verify_folded_device_batch_bn254", "hg_claims_verify_folded_batch_bn254"
NEED = "a folded opening needs a claim"
SENTINEL = tob.SENTINEL


def _last():
    return hg.lib().hg_last_error().decode()


def call_open(a, out, **over):
    o = dict(openings=out.buf.ctypes.data_as(hg.u8p), lens=out.lens, status=out.status, reasons=out.reasons, cap_each=out.cap_each, reason_cap=out.reason_cap)
    o.update(over)
    return hg.lib().hg_pcs_open_folded_batch_bn254(a["ctx"], a["commitments"], a["tables"], a["points"], a["values"], a["n_claims"], a["n_queries"], a["n"], o["openings"],
                                                   o["cap_each"], o["lens"], o["status"], o["reasons"], o["reason_cap"])


def call_open_w(a, out):
    return hg.lib().hg_claims_open_folded_batch_bn254(a["ctx"], a["params"], a["commitments"], a["claims"], a["claim_cap_each"], a["points"], a["coord_cap_each"], a["n_claims"],
                                                      a["n_queries"], a["n"], out.buf.ctypes.data_as(hg.u8p), out.cap_each, out.lens, out.status, out.reasons, out.reason_cap)


def call_verify(a, out):
    return hg.lib().hg_pcs_verify_folded_device_batch_bn254(a["ctx"], a["roots"], a["nvars"], a["n_tables"], a["log2_row"], a["tables"], a["points"], a["values"],
                                                            a["n_claims"], a["n_queries"], a["proofs"], a["lens"], a["n"], out.res, out.reasons, out.cap)


def call_verify_w(a, out):
    return hg.lib().hg_claims_verify_folded_batch_bn254(a["ctx"], a["params"], a["roots"], a["log2_row"], a["claims"], a["claim_cap_each"], a["points"], a["coord_cap_each"],
                                                        a["n_claims"], a["n_queries"], a["openings"], a["lens"], a["n"], out.res, out.reasons, out.cap)


# ---- not gpu ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in (OPEN, OPEN_W, VERIFY, VERIFY_W):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name
    for name in ("pcs_open_folded_batch_bn254", "claims_open_folded_batch_bn254", "pcs_verify_folded_batch_bn254", "claims_verify_folded_batch_bn254"):
        assert callable(getattr(hg, name)), name


def _wrapper_runs(n):
    """the arguments of the two wrapper entries for a run of n copies of the (1024, 1) wrapper case"""
    w = tb.wrapper_case(1024, 1, 27)
    params, cl = w["bfv"].params, w["claims"]
    opening = tf.folded_wrapper(1024, 1, 27)
    m = max(n, 1)
    claims, nc1, points, nco1, counts = hg._claims_batch_arrays([cl] * m, hg.InputClaimsBn254)
    base = dict(ctx=None, params=C.byref(params), log2_row=0, claims=claims, claim_cap_each=nc1, points=hg._ptr(points), coord_cap_each=nco1, n_claims=counts, n_queries=0, n=n)
    opn = dict(base, commitments=(C.c_void_p * m)(*[w["cm"].h] * m))
    ver = dict(base, roots=(C.c_char_p * m)(*[bytes(w["cm"].root)] * m), openings=(C.c_char_p * m)(*[bytes(opening)] * m), lens=(C.c_size_t * m)(*[len(opening)] * m))
    return w, opening, opn, ver, (claims, points, counts)


def test_n_zero_returns_zero_and_writes_nothing():
    c = tf.case("unequal")
    out = tob.Outputs(1, 64)
    a, keep = tob.generic_args([], Q)
    assert call_open(a, out) == 0 and out.untouched()
    out = tvb.Outputs(1)
    a, keep2 = tvb.generic_args([], c["nvars"], c["c"], Q)
    assert call_verify(a, out) == 0 and out.untouched()
    w, opening, opn, ver, keep3 = _wrapper_runs(0)
    out = tob.Outputs(1, 64)
    assert call_open_w(opn, out) == 0 and out.untouched()
    out = tvb.Outputs(1)
    assert call_verify_w(ver, out) == 0 and out.untouched()
    assert hg.pcs_open_folded_batch_bn254(None, [], []) == [] and hg.claims_open_folded_batch_bn254(None, w["bfv"].params, [], []) == []
    assert hg.pcs_verify_folded_batch_bn254(None, [], c["nvars"], [], [], Q, c["c"]) == []
    assert hg.claims_verify_folded_batch_bn254(None, w["bfv"].params, [], [], []) == []
    del keep, keep2, keep3


def test_no_context_comes_after_the_argument_checks_of_every_item():
    """The verify entries need no handle, so a machine without a device reaches every argument check of item 1 and the `no context`
    behind them. (The open entries stop at item 0's host-form handle there - see the next test; their checks of the claims, of an item
    without a claim and of cap_each are in test_errors_of_the_open_entries_that_need_a_device_handle.)"""
    c = tf.case("unequal")
    nvars, cc, claims, proof, root = c["nvars"], c["c"], c["claims"], c["proof"], c["cm"].root
    held = []

    def run(claims1):
        held.append(tvb.generic_args([(root, claims, proof), (root, claims1, proof)], nvars, cc, Q))
        return held[-1][0]

    out = tvb.Outputs(2)
    assert call_verify(run(claims), out) == -1 and _last() == VERIFY + ": no context" and out.untouched()
    t, pt, v = claims[0]
    for bad, text in (([(4, pt, v)] + claims[1:], "names table 4"), ([(t, [R] + pt[1:], v)] + claims[1:], "non-canonical coordinate"), ([], NEED)):
        out = tvb.Outputs(2)
        assert call_verify(run(bad), out) == -1
        assert _last().startswith(VERIFY + ": index 1: ") and text in _last() and "no context" not in _last(), _last()
        assert out.untouched(), text
    assert call_verify(run([]), tvb.Outputs(2)) == -1 and _last() == VERIFY + ": index 1: " + NEED
    with pytest.raises(hg.HgError, match="^" + VERIFY + ": no context$"):
        hg.pcs_verify_folded_batch_bn254(None, [root], nvars, [claims], [proof], Q, cc)
    # the wrapper: the same order; an item without claims is no error of the call there (it is rejected on the device pass's side), so
    # with everything else in order the call gets as far as the missing context
    w, opening, opn, ver, keep = _wrapper_runs(2)
    out = tvb.Outputs(2)
    assert call_verify_w(ver, out) == -1 and _last() == VERIFY_W + ": no context" and out.untouched()
    other = (hg.HgInputClaimBn254 * len(keep[0]))(*keep[0])
    other[ver["claim_cap_each"]].input = 3                        # claim 0 of item 1 on a public input
    assert call_verify_w(dict(ver, claims=other), out) == -1 and _last().startswith(VERIFY_W + ": index 1: ") and "is on input 3" in _last() and out.untouched()
    assert call_verify_w(dict(ver, n_claims=(C.c_size_t * 2)(keep[2][0], 0)), out) == -1 and _last() == VERIFY_W + ": no context" and out.untouched()
    del held


def test_a_host_form_handle_is_an_error_naming_the_index():
    c = tf.case("unequal")
    a, keep = tob.generic_args([(c["cm"], c["claims"])] * 2, Q)
    cap = len(c["proof"])
    out = tob.Outputs(2, cap)
    assert call_open(a, out) == -1 and _last() == OPEN + ": index 0: the commitment was made by the host form: a run is opened on device commitments only" and out.untouched()
    with pytest.raises(hg.HgError, match=OPEN + ": index 0: the commitment was made by the host form"):
        hg.pcs_open_folded_batch_bn254(None, [c["cm"]], [c["claims"]], Q)
    w, opening, opn, ver, keep2 = _wrapper_runs(2)
    out = tob.Outputs(2, len(opening))
    assert call_open_w(opn, out) == -1 and _last().startswith(OPEN_W + ": index 0: the commitment was made by the host form") and out.untouched()
    del keep, keep2


def test_a_goldilocks_handle_gets_the_other_fields_text():
    c = tf.case("unequal")
    gl = hg.Commitment.commit(None, [np.arange(1 << v, dtype=np.uint64) for v in c["nvars"]], c["c"])
    a, keep = tob.generic_args([(c["cm"], c["claims"])] * 2, Q)
    out = tob.Outputs(2, len(c["proof"]))
    assert call_open(dict(a, commitments=(C.c_void_p * 2)(gl.h, c["cm"].h)), out) == -1
    assert _last() == OPEN + ": index 0: the commitment is over Goldilocks: open it with hg_pcs_open_folded_batch" and out.untouched()
    w, opening, opn, ver, keep2 = _wrapper_runs(2)
    glsec = hg.Commitment.secrets(None, w["bfv"].params, w["w"])
    out = tob.Outputs(2, len(opening))
    assert call_open_w(dict(opn, commitments=(C.c_void_p * 2)(glsec.h, w["cm"].h)), out) == -1
    assert _last() == OPEN_W + ": index 0: the commitment is over Goldilocks: open it with hg_claims_open_folded_batch" and out.untouched()
    del keep, keep2


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def run_of(ctx, nvars, c, seeds, which_lists, same_as=None):
    """members with their own tables (one seed each) and claim lists: host commitments, device handles, claims. same_as: {i: j} makes
    member i use member j's tables and handle"""
    same_as = same_as or {}
    tables = [make_tables(nvars, s) for s in seeds]
    for i, j in same_as.items():
        tables[i] = tables[j]
    host = [hg.Commitment.commit_bn254(None, t, log2_row=c) for t in tables]
    dev = [hg.Commitment.commit_bn254(ctx, t, c) for t in tables]
    for i, j in same_as.items():
        host[i], dev[i] = host[j], dev[j]
    claims = [claims_on(t, which, 0x70 + 5 * i) for i, (t, which) in enumerate(zip(tables, which_lists))]
    return tables, host, dev, claims


@pytest.mark.gpu
def test_bytes_equal_the_single_call_and_the_host_form(ctx):
    nvars, c = [4, 3, 2, 4], 2
    which = [[0, 1, 1, 3, 0], [2], [3, 3, 3, 3, 3, 3], [0, 1, 2, 3], [1, 0, 3]]
    tables, host, dev, claims = run_of(ctx, nvars, c, [0xa0 + i for i in range(5)], which, same_as={4: 1})
    want = [h.open_folded(cl, Q) for h, cl in zip(host, claims)]
    assert len(set(want)) == 5
    got = hg.pcs_open_folded_batch_bn254(ctx, dev, claims, Q)
    assert [why for _, why in got] == [""] * 5 and all(b is not None for b, _ in got)
    for i, (b, _) in enumerate(got):
        assert b == dev[i].open_folded(claims[i], Q), i
        assert b == want[i], i
        assert py_verify_folded_bn254(host[i].root, nvars, c, claims[i], Q, b) == "", i
    try:
        ctx.set_option("verify_batch_group", 2)                       # groups of 2, 2, 1
        assert hg.pcs_open_folded_batch_bn254(ctx, dev, claims, Q) == [(b, "") for b in want]
    finally:
        ctx.set_option("verify_batch_group", 0)


@pytest.mark.gpu
def test_a_table_that_is_a_scalar_from_the_start(ctx):
    nvars = [2, 0]
    tables = [make_tables(nvars, 0x51 + i) for i in range(3)]
    host = [hg.Commitment.commit_bn254(None, t, log2_row=0) for t in tables]
    dev = [hg.Commitment.commit_bn254(ctx, t, 0) for t in tables]
    assert dev[0].log2_row == 0
    claims = [claims_on(t, which, 3 + i) for i, (t, which) in enumerate(zip(tables, ([1, 0, 1], [0], [1])))]
    want = [h.open_folded(cl, Q) for h, cl in zip(host, claims)]
    assert hg.pcs_open_folded_batch_bn254(ctx, dev, claims, Q) == [(b, "") for b in want]
    assert [d.open_folded(cl, Q) for d, cl in zip(dev, claims)] == want   # the single call, which now fetches the element with step 0


@pytest.mark.gpu
def test_tables_that_retire_in_different_rounds(ctx):
    nvars, c = [12, 12, 9], 6
    tables, host, dev, claims = run_of(ctx, nvars, c, [0xc0, 0xc1, 0xc2], [[0, 1, 2, 1, 0], [2, 2], [1, 0]])
    assert hg.pcs_open_folded_batch_bn254(ctx, dev, claims, Q) == [(h.open_folded(cl, Q), "") for h, cl in zip(host, claims)]


@pytest.mark.gpu
def test_a_refused_member_in_the_middle(ctx):
    nvars, c = [8, 7, 6], 4
    tables, host, dev, claims = run_of(ctx, nvars, c, [0xd0 + i for i in range(4)], [[0, 1, 2, 0]] * 4)
    bad = list(claims[2])
    for i in (1, 3):                                                  # claim 1 of 4 raised by one, and the last claim wrong as well
        t, pt, v = bad[i]
        bad[i] = (t, pt, (v + 1) % R)
    with pytest.raises(hg.HgError) as e:
        dev[2].open_folded(bad, Q)
    text = str(e.value)
    assert text == "hg_pcs_open_folded_bn254: claim 1: the value is not the evaluation of table 1 at the point"
    run = claims[:2] + [bad] + claims[3:]
    want = [h.open_folded(cl, Q) for h, cl in zip(host, claims)]
    a, keep = tob.generic_args(list(zip(dev, run)), Q)
    cap = len(want[0]) + 24
    out = tob.Outputs(4, cap, 256)
    assert call_open(dict(a, ctx=ctx.h), out) == 1
    assert list(out.status) == [0, 0, 1, 0] and list(out.lens) == [len(want[0]), len(want[1]), 0, len(want[3])]
    assert out.slot(2) == bytes([SENTINEL]) * cap and out.reason(2) == text
    for i in (0, 1, 3):
        assert out.slot(i) == want[i] + bytes([SENTINEL]) * (cap - len(want[i])) and out.reason(i) == "", i
        assert want[i] == dev[i].open_folded(claims[i], Q), i
    assert hg.pcs_open_folded_batch_bn254(ctx, dev, run, Q) == [(want[0], ""), (want[1], ""), (None, text), (want[3], "")]
    for d, h, cl in zip(dev, host, claims):
        assert d.open(cl, Q) == h.open(cl, Q)                         # the raw rows were not written
    del keep


@pytest.mark.gpu
def test_errors_of_the_open_entries_that_need_a_device_handle(ctx):
    """what a machine without a device cannot reach: the checks behind the handle's"""
    nvars, c = [4, 3, 2, 4], 2
    tables, host, dev, claims = run_of(ctx, nvars, c, [0xe0, 0xe1], [[0, 1, 1, 3, 0], [2, 3]])
    cap = hg.pcs_folded_opening_bytes_bn254(nvars, Q, c)
    held = []

    def run(claims1, **over):
        held.append(tob.generic_args([(dev[0], claims[0]), (dev[1], claims1)], Q))
        return {**held[-1][0], "ctx": ctx.h, **over}

    t, pt, v = claims[1][0]
    cases = [(run(claims[1], ctx=None), {}, OPEN + ": no context"),
             (run([(4, pt, v)] + claims[1][1:], ctx=None), {}, "index 1: claim 0 names table 4"),
             (run([(t, [R] + pt[1:], v)] + claims[1][1:], ctx=None), {}, "index 1: claim 0: non-canonical coordinate"),
             (run([], ctx=None), {}, OPEN + ": index 1: " + NEED),
             (run(claims[1], ctx=None), dict(cap_each=cap - 32), "%d bytes" % cap),
             (run(claims[1]), dict(cap_each=cap - 32), "%d bytes" % cap)]
    for args, over, text in cases:
        out = tob.Outputs(2, cap)
        assert call_open(args, out, **over) == -1, text
        assert _last().startswith(OPEN + ": ") and text in _last(), (_last(), text)
        assert ("no context" in _last()) == (text == OPEN + ": no context"), _last()
        assert out.untouched(), text
    out = tob.Outputs(2, cap)
    assert call_open(run(claims[1]), out) == 0 and [out.slot(i)[:out.lens[i]] for i in range(2)] == [h.open_folded(cl, Q) for h, cl in zip(host, claims)]
    del held


# With one workgroup a table and member (HG_PCS_FOLD_BLOCKS=1: the bound holds for the launch as a whole, and a table of a member gets at
# least one workgroup), the table of 2^17 entries gives a thread 256 trips in round 0, 128 in round 1 and 64 in round 2, so the unreduced
# sums restart (BNFOLD_TRIPS = 64) in both round kernels of the group form, with every member folding by its own constants. Three claims
# on the large table, as the single test gives the g builder. The plan line counts the launches of the round kernels and the
# synchronisations that fetch sums or scalars for the whole group: V + 1 = 18 each, whatever the number of members.
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import test_pcs_folded_bn254 as T
from hglib import hg
nvars, c = [17, 14], 8
tables = [T.make_tables(nvars, 0xb17 + i) for i in range(3)]
claims = [T.claims_on(t, which, 8 + i) for i, (t, which) in enumerate(zip(tables, ([0, 1, 0], [1, 0], [0, 0, 1])))]
host = [hg.Commitment.commit_bn254(None, t, c) for t in tables]
ctx = hg.Context(0)
dev = hg.Commitment.commit_batch_bn254(ctx, tables, c)
got = hg.pcs_open_folded_batch_bn254(ctx, dev, claims, 3)
for i in range(3):
    assert got[i] == (host[i].open_folded(claims[i], 3), ""), i
print("FOLD BATCH OK")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["1", "2048"])
def test_long_accumulations_and_the_plan_line(blocks):
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, HG_DEBUG="plan", HG_PCS_FOLD_BLOCKS=blocks))
    assert r.returncode == 0 and "FOLD BATCH OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    plan = re.findall(r"\[hg plan\] bnpcsfoldb (.*)", r.stderr)
    assert plan == ["members=3 V=17 round_launches=18 round_syncs=18 tables=2 claims=8"], r.stderr[-2000:]


def verifier_items():
    """the tamper set of the single test with the untampered opening at two positions and an unfolded opening of the same claims"""
    c = tf.case("unequal")
    items = [(root, claims, proof) for _, root, claims, proof, _ in tf.tamper_set("unequal")]
    labels = [label for label, _, _, _, _ in tf.tamper_set("unequal")]
    items[3:3] = [(c["cm"].root, c["claims"], c["proof"])]
    items.append((c["cm"].root, c["claims"], c["proof"]))
    items.append((c["cm"].root, c["claims"], c["cm"].open(c["claims"], Q)))      # an unfolded opening of the same claims
    labels = labels[:3] + ["untampered"] + labels[3:] + ["untampered", "unfolded"]
    want = [hg.pcs_verify_folded_bn254(root, c["nvars"], claims, proof, Q, c["c"]) for root, claims, proof in items]
    return c, items, labels, want


def test_the_verifier_items_cover_at_least_ten_reasons():
    """(no device: the count is the host verifier's alone)"""
    c, items, labels, want = verifier_items()
    accepted = [i for i, (ok, _) in enumerate(want) if ok]
    assert accepted == [3, len(items) - 2] and all(why for ok, why in want if not ok)
    assert len({why for _, why in want}) >= 10


@pytest.mark.gpu
def test_verifier_gives_the_hosts_decision_and_reason_item_by_item(ctx):
    c, items, labels, want = verifier_items()
    nvars, cc = c["nvars"], c["c"]
    accepted = [i for i, (ok, _) in enumerate(want) if ok]
    roots, cls, proofs = [list(x) for x in zip(*items)]
    for group in (0, 3):
        try:
            ctx.set_option("verify_batch_group", group)
            got = hg.pcs_verify_folded_batch_bn254(ctx, roots, nvars, cls, proofs, Q, cc)
        finally:
            ctx.set_option("verify_batch_group", 0)
        for i, label in enumerate(labels):
            assert got[i] == want[i], (group, label, got[i], want[i])
    a, keep = tvb.generic_args(items, nvars, cc, Q)
    out = tvb.Outputs(len(items), 128)
    assert call_verify(dict(a, ctx=ctx.h), out) == len(items) - 2 and [out.res[i] for i in accepted] == [0, 0]
    del keep


@pytest.mark.gpu
def test_wrappers_end_to_end(ctx):
    bfv = hg.BfvEncrypt.new(1024, 1)
    pk = bfv.setup(ctx)
    params = bfv.params
    ws = [hg.Witness.synthetic(params, s) for s in (0xf11, 0xf12, 0xf13)]
    cms = hg.Commitment.secrets_batch_bn254(ctx, params, ws)
    roots = [cm.root for cm in cms]
    proofs = [ctx.prove_bn254(pk, w)[0] for w in ws]
    insts = [hg.Instance.from_witness(w) for w in ws]
    got = hg.verify_public_batch_bn254(ctx, pk, insts, proofs)
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    opened = hg.claims_open_folded_batch_bn254(ctx, params, cms, cls)
    assert opened == [(cm.open_claims_folded(params, cl), "") for cm, cl in zip(cms, cls)]
    openings = [b for b, _ in opened]
    assert len(openings[0]) == hg.pcs_folded_opening_bytes_bn254(cms[0].nvars)
    assert hg.claims_verify_folded_batch_bn254(ctx, params, roots, cls, openings) == [(True, "")] * 3
    V, m = max(cms[0].nvars), len(cms[0].nvars)
    hb = 32 * (3 * V + m)
    for at in (31, hb + 32 + 31, len(openings[1]) - 1):
        bad = bytearray(openings[1])
        bad[at] ^= 1
        h = hg.claims_verify_folded_bn254(params, roots[1], cls[1], bytes(bad))
        assert not h[0]
        assert hg.claims_verify_folded_batch_bn254(ctx, params, roots, cls, [openings[0], bytes(bad), openings[2]]) == [(True, ""), h, (True, "")], at
    # a proof the public batch verifier rejected: its arrays pass through unchanged. The verifier rejects that item - not an error of
    # the call; the opener, which cannot open nothing, names it
    spoiled = bytearray(proofs[1])
    spoiled[40] ^= 1
    got = hg.verify_public_batch_bn254(ctx, pk, insts, [proofs[0], bytes(spoiled), proofs[2]])
    assert [ok for ok, _, _ in got] == [True, False, True] and got[1][2] is None
    through = [cl for _, _, cl in got]
    assert hg.claims_verify_folded_batch_bn254(ctx, params, roots, through, openings) == [(True, ""), (False, VERIFY_W + ": " + NEED), (True, "")]
    with pytest.raises(hg.HgError, match=OPEN_W + ": index 1: " + NEED):
        hg.claims_open_folded_batch_bn254(ctx, params, cms, through)
    pk.free()


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    nvars, c = [8, 7, 6], 4
    tables, host, dev, claims = run_of(ctx, nvars, c, [0xd0, 0xd1], [[0, 1, 2, 0]] * 2)
    ctx.profile(2)
    ctx.profile_reset()
    try:
        assert all(b is not None for b, _ in hg.pcs_open_folded_batch_bn254(ctx, dev, claims, Q))
        stat = [s for s in ctx.profile_get(256) if s["name"] == "pcs_fold_batch_bn254"]
    finally:
        ctx.profile(0)
    # the g kernel, V + 1 = 9 steps, the two combinations and the gather
    assert len(stat) == 1 and stat[0]["launches"] >= 9 + 3 and stat[0]["total_ms"] > 0
