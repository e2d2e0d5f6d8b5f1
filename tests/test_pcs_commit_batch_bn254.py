"""hg_pcs_commit_batch_bn254 / hg_secrets_commit_batch_bn254: a run of BN254 commitments made in device passes of a group of members
each. The yardstick of every case is the host form on that member alone (hg.Commitment.commit_bn254(None, ..) and its .open): the
root is compared exactly, and the tree and the encoded matrix through an opening with enough queries to reach every column with its
whole path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_pcs_bn254 as tb
from orclib import R_BN as R
from hglib import hg, ROOT

GENERIC, WRAPPER = "hg_pcs_commit_batch_bn254", "hg_secrets_commit_batch_bn254"
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
    """handles and roots filled with a sentinel byte, and whether they still hold it"""

    def __init__(self, n):
        self.handles = (C.c_void_p * max(n, 1))()
        self.roots = (C.c_uint8 * (32 * max(n, 1)))()
        C.memset(self.handles, SENTINEL, C.sizeof(self.handles))
        C.memset(self.roots, SENTINEL, C.sizeof(self.roots))

    def untouched(self):
        return bytes(self.handles) == bytes([SENTINEL]) * C.sizeof(self.handles) and bytes(self.roots) == bytes([SENTINEL]) * C.sizeof(self.roots)


def generic_args(tables_list, log2_row):
    """the named arguments of hg_pcs_commit_batch_bn254 (ctx None) and what keeps them alive; an element is 4 words"""
    tabs = [[hg._fr_table(t) for t in tables] for tables in tables_list]
    nvars = [(t.size // 4).bit_length() - 1 for t in tabs[0]]
    rows = [(hg.u64p * len(nvars))(*[hg._ptr(t) for t in tables]) for tables in tabs]
    ptrs = (C.POINTER(hg.u64p) * len(tabs))(*[C.cast(r, C.POINTER(hg.u64p)) for r in rows])
    return dict(ctx=None, tables=ptrs, nvars=(C.c_uint32 * len(nvars))(*nvars), n_tables=len(nvars), log2_row=log2_row, n=len(tabs)), (tabs, rows)


def call_generic(a, out, handles=True, roots=True):
    return hg.lib().hg_pcs_commit_batch_bn254(a["ctx"], a["tables"], a["nvars"], a["n_tables"], a["log2_row"], a["n"], out.handles if handles else None,
                                              out.roots if roots else None)


def members(nvars, count, seed):
    return [tb.make_tables(nvars, seed + 16 * i) for i in range(count)]


def test_generic_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    nvars = dict(tb.C2_SHAPES)[15]
    run = members(nvars, 3, 0x1c00)
    good, keep = generic_args(run, 2)
    out = Outputs(3)
    assert call_generic(good, out) == -1 and _last() == GENERIC + ": no context" and out.untouched()

    cases = [(dict(good, tables=None), "null argument", None), (dict(good, nvars=None), "null argument", None)]
    no_member = (C.POINTER(hg.u64p) * 3)(good["tables"][0], good["tables"][1], None)
    cases.append((dict(good, tables=no_member), "null argument", 2))
    row = (hg.u64p * 4)(keep[1][2][0], None, keep[1][2][2], keep[1][2][3])
    no_table = (C.POINTER(hg.u64p) * 3)(good["tables"][0], good["tables"][1], C.cast(row, C.POINTER(hg.u64p)))
    cases.append((dict(good, tables=no_table), "null table 1", 2))
    cases.append((dict(good, nvars=(C.c_uint32 * 4)(5, 4, 3, 31)), "", None))       # a shape outside the limits of hg_pcs_commit_bn254
    cases.append((dict(good, log2_row=3), "log2_row", None))                         # log2_row above a table's variables
    cases.append((dict(good, n_tables=65), "tables", None))
    for args, text, index in cases:
        out = Outputs(3)
        assert call_generic(args, out) == -1, text
        assert _last().startswith(GENERIC + ": ") and text in _last() and "no context" not in _last(), _last()
        if index is not None:
            assert "index %d" % index in _last(), _last()
        assert out.untouched(), text
    for kw in (dict(handles=False), dict(roots=False)):                              # the outputs are arguments too
        out = Outputs(3)
        assert call_generic(good, out, **kw) == -1 and "null argument" in _last() and out.untouched()
    # 65536 rows in a member: one table of 2^17 elements in rows of 2
    big, keep_big = generic_args([[np.zeros(4 << 17, dtype=np.uint64)]] * 2, 1)
    out = Outputs(2)
    assert call_generic(big, out) == -1 and _last().startswith(GENERIC + ": more than 65535 rows") and out.untouched()
    # n == 0
    out = Outputs(1)
    assert call_generic(dict(good, n=0), out) == 0 and out.untouched()
    assert hg.Commitment.commit_batch_bn254(None, [], 2) == []
    with pytest.raises(hg.HgError, match="^" + GENERIC + ": no context$"):
        hg.Commitment.commit_batch_bn254(None, run, 2)
    del keep, keep_big


def call_wrapper(a, out):
    return hg.lib().hg_secrets_commit_batch_bn254(a["ctx"], a["params"], a["ws"], a["n"], a["log2_row"], a["handles"] if "handles" in a else out.handles,
                                                  a["roots"] if "roots" in a else out.roots)


def test_wrapper_entry_errors_of_the_call_write_nothing_and_name_function_and_index():
    params, other = hg.params_builtin(1024, 1), hg.params_builtin(2048, 1)
    ws = [hg.Witness.synthetic(params, 0x51 + i) for i in range(3)]
    alien = hg.Witness.synthetic(other, 0x77)
    good = dict(ctx=None, params=C.byref(params), ws=(C.c_void_p * 3)(*[w.h for w in ws]), n=3, log2_row=0)
    out = Outputs(3)
    assert call_wrapper(good, out) == -1 and _last() == WRAPPER + ": no context" and out.untouched()
    cases = [(dict(good, **{name: None}), "null argument", None) for name in ("params", "ws", "handles", "roots")]
    cases.append((dict(good, ws=(C.c_void_p * 3)(ws[0].h, ws[1].h, None)), "null argument", 2))
    cases.append((dict(good, ws=(C.c_void_p * 3)(ws[0].h, alien.h, ws[2].h)), "the witness was built for other parameters", 1))
    cases.append((dict(good, log2_row=12), "log2_row", None))
    for args, text, index in cases:
        out = Outputs(3)
        assert call_wrapper(args, out) == -1, text
        assert _last().startswith(WRAPPER + ": ") and text in _last() and "no context" not in _last(), _last()
        if index is not None:
            assert "index %d" % index in _last(), _last()
        assert out.untouched(), text
    out = Outputs(1)
    assert call_wrapper(dict(good, n=0), out) == 0 and out.untouched()
    assert hg.Commitment.secrets_batch_bn254(None, params, []) == []
    with pytest.raises(hg.HgError, match="^" + WRAPPER + ": no context$"):
        hg.Commitment.secrets_batch_bn254(None, params, ws)


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def every_column(N):
    """queries enough that every one of N columns is opened, with its whole path, but for a chance below N exp(-16)"""
    return 16 * N


def check_members(ctx, run, c, cms, n_claims=3):
    """every batch-made handle against the host form of its member: the root, and - through one opening that reaches every column
    with its path - the encoded matrix and the tree"""
    nvars = [len(t).bit_length() - 1 for t in run[0]]
    Q = every_column(4 << c)
    assert len(cms) == len(run)
    for i, (tables, cm) in enumerate(zip(run, cms)):
        host = hg.Commitment.commit_bn254(None, tables, c)
        assert cm.root == host.root and cm.nvars == nvars and cm.log2_row == c and cm.field == "bn254", i
        claims = tb.make_claims(tables, n_claims, 0x330 + i)
        assert cm.open(claims, Q) == host.open(claims, Q), i


@pytest.mark.gpu
@pytest.mark.parametrize("Rn", [Rn for Rn, _ in tb.C2_SHAPES + tb.LEAF_SHAPES])
def test_c2_shapes(ctx, Rn):
    """c = 2 (N = 16, the radix-2 NTT), R = 4, 5, 8, 15, 16: the leaf sponge with the padding alone in a block, in one word, apart; member
    0 is test_pcs_bn254's case; with N = 16 member 1's columns begin inside a wavefront"""
    case = tb.c2_case(Rn)
    run = [case["tables"]] + members(case["nvars"], 2, 0x2c00 + Rn)
    cms = hg.Commitment.commit_batch_bn254(ctx, run, 2)
    assert cms[0].root == case["cm"].root == case["py"].root and len({cm.root for cm in cms}) == 3
    assert cms[0].open(case["claims"], 5) == case["open35"]
    check_members(ctx, run, 2, cms)


@pytest.mark.gpu
def test_tree_levels(ctx):
    """N = 1024, R = 3: the first level (512 nodes a member) is the per-level kernel, the rest one workgroup a member"""
    run = members([9, 8], 3, 0x3c00)
    check_members(ctx, run, 8, hg.Commitment.commit_batch_bn254(ctx, run, 8), n_claims=2)


@pytest.mark.gpu
def test_four_step_ntt(ctx):
    """c = 6: the LDS four-step NTT of size 256 in one batch over the 7 rows of each of three members"""
    run = members([8, 7, 6], 3, 0x4c00)
    check_members(ctx, run, 6, hg.Commitment.commit_batch_bn254(ctx, run, 6))


@pytest.mark.gpu
def test_boundaries(ctx):
    """R = 129: 4 R + 1 = 517 message words, 31 sponge blocks a column"""
    run = members([9, 2], 2, 0x5c00)
    check_members(ctx, run, 2, hg.Commitment.commit_batch_bn254(ctx, run, 2), n_claims=2)


@pytest.mark.gpu
def test_an_element_that_is_not_below_r(ctx):
    nvars = dict(tb.C2_SHAPES)[15]
    run = members(nvars, 3, 0x6c00)
    bad = [[list(t) for t in tables] for tables in run]
    bad[1][0][29] = R
    bad[2][1][1] = R + (5 << 192)                                                    # the lowest member at fault is named
    a, keep = generic_args(bad, 2)
    out = Outputs(3)
    assert call_generic(dict(a, ctx=ctx.h), out) == -1
    assert _last() == GENERIC + ": index 1: a table holds an element that is not below r" and out.untouched()
    with pytest.raises(hg.HgError, match=GENERIC + ": index 1: "):
        hg.Commitment.commit_batch_bn254(ctx, bad, 2)
    check_members(ctx, run, 2, hg.Commitment.commit_batch_bn254(ctx, run, 2))        # the next call on the context works
    del keep


@pytest.mark.gpu
def test_freeing_the_handles_of_a_group_in_any_order(ctx):
    nvars = dict(tb.C2_SHAPES)[16]
    run = members(nvars, 4, 0x7c00)
    cms = hg.Commitment.commit_batch_bn254(ctx, run, 2)
    host = [hg.Commitment.commit_bn254(None, t, 2) for t in run]
    claims = [tb.make_claims(t, 2, 0x440 + i) for i, t in enumerate(run)]
    cms[2].free()
    assert cms[0].open(claims[0], 7) == host[0].open(claims[0], 7)
    cms[0].free()
    cms[3].free()
    assert cms[1].open(claims[1], every_column(16)) == host[1].open(claims[1], every_column(16))
    again = hg.Commitment.commit_batch_bn254(ctx, run[:2], 2)                        # a new group beside the survivor
    assert cms[1].open(claims[1], 7) == host[1].open(claims[1], 7) and again[1].root == host[1].root
    cms[1].free()
    # the context keeps the freed group's allocation for its next groups: one of the same size, then a smaller one in the larger spare
    check_members(ctx, run, 2, hg.Commitment.commit_batch_bn254(ctx, run, 2), n_claims=1)
    check_members(ctx, run[2:], 2, hg.Commitment.commit_batch_bn254(ctx, run[2:], 2), n_claims=1)


@pytest.mark.gpu
def test_handles_may_outlive_their_context():
    """a group's allocation goes when its last handle is freed, also after the context (whose spare allocations are gone by then)"""
    other = hg.Context(0)
    run = members(dict(tb.C2_SHAPES)[16], 2, 0xac00)
    cms = hg.Commitment.commit_batch_bn254(other, run, 2)
    assert [cm.root for cm in cms] == [hg.Commitment.commit_bn254(None, t, 2).root for t in run]
    cms[0].free()
    other.close()
    cms[1].free()


@pytest.mark.gpu
def test_grouping(ctx):
    nvars = dict(tb.C2_SHAPES)[15]
    run = members(nvars, 5, 0x8c00)
    want = [hg.Commitment.commit_bn254(None, t, 2).root for t in run]
    try:
        for G in (0, 2, 1):
            ctx.set_option("verify_batch_group", G)
            cms = hg.Commitment.commit_batch_bn254(ctx, run, 2)
            assert [cm.root for cm in cms] == want, G
            check_members(ctx, run[3:], 2, cms[3:], n_claims=1)
    finally:
        ctx.set_option("verify_batch_group", 0)


@pytest.mark.gpu
def test_secrets_batch_gives_the_single_call_s_handles(ctx):
    """the signed lift of the witness words (words at or above 2^63 occur) by the batched kernel"""
    params = hg.params_builtin(1024, 1)
    ws = [hg.Witness.synthetic(params, 0x61 + i) for i in range(3)]
    assert all(any(int(x) >= (1 << 63) for x in w.arrays()["e"]) for w in ws)
    cms = hg.Commitment.secrets_batch_bn254(ctx, params, ws)
    for w, cm in zip(ws, cms):
        host = hg.Commitment.secrets_bn254(None, params, w)
        assert cm.root == host.root == hg.Commitment.secrets_bn254(ctx, params, w).root and cm.nvars == host.nvars and cm.field == "bn254"
        assert cm.open([], 64) == host.open([], 64)


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    run = members(dict(tb.C2_SHAPES)[15], 3, 0x9c00)
    ctx.profile(2)
    ctx.profile_reset()
    try:
        cms = hg.Commitment.commit_batch_bn254(ctx, run, 2)
        stat = [s for s in ctx.profile_get(256) if s["name"] == "pcs_bn254_commit_batch"]
    finally:
        ctx.profile(0)
    assert len(cms) == 3 and len(stat) == 1 and stat[0]["launches"] >= 4 and stat[0]["total_ms"] > 0
