"""hg_secrets_commit_values / hg_prove_encryptions_committed: the commitment to the five secret inputs made from the node tables in HBM,
by one call on a values object or inside the encryption pipeline.

The yardstick everywhere is the host form: hg.Commitment.secrets(None, params, w, log2_row) on the witness of the item and .open(..) on
it. Roots are compared exactly; trees and encoded matrices through an opening of six claims (one on each kind of table, two on r2is)
with Q = 4N queries, enough to reach every column with its whole path but for a chance below N exp(-4) a column.

Shapes, none of them the workload's:
  (1024,1) log2_row 0   c = 7, N = 512, R = 72: LDS four-step NTT; the tree wholly in the top kernel
  (1024,1) log2_row 2   N = 16, R = 2304: radix-2 NTT in HBM, 2304 rows
  (1024,1) log2_row 1   C = 2: the narrowest row the 16-byte path takes
  (1024,1) log2_row 10  the smallest table's variables: every table one or two rows
  (4096,2) log2_row 0   c = 8, N = 1024: one per-level tree launch below the top kernel; two r1is tables; r2is with P+1 variables
  derived (1024,2)      k = 2 with the smallest tables"""
import ctypes as C
import os
import random
import re
import statistics
import time

import numpy as np
import pytest

import test_pcs as tp
import test_prove_encryptions as tpe
from hglib import hg, ROOT

P = hg.P
VALUES, PIPE = "hg_secrets_commit_values", "hg_prove_encryptions_committed"
SENTINEL = 0x5a
DERIVED = "derived"
SHAPES = [((1024, 1), 0), ((1024, 1), 2), ((1024, 1), 1), ((1024, 1), 10), ((4096, 2), 0), (DERIVED, 0)]
IDS = ["%s-row%d" % (k if k == DERIVED else "%dx%d" % k, r) for k, r in SHAPES]


def _last():
    return hg.lib().hg_last_error().decode()


def params_of(key):
    if key == DERIVED:
        return hg.params_derive(1024, 2, [int(q) for q in hg.params_builtin(4096, 2).qis[:2]])
    return hg.params_builtin(*key)


def secret_tables(params, d):
    """the tables of hg_secrets_commit in its order, from a witness's arrays"""
    sz = 2 * params.n
    return [d["s"], d["e"], d["k1"]] + [d["r1is"][i * sz:(i + 1) * sz] for i in range(params.k)] + [d["r2is"]]


def kind_claims(params, d, seed):
    """six claims at random E points: s, e, k1, the last r1is table, r2is twice"""
    tables = secret_tables(params, d)
    k = params.k
    rng = random.Random(seed)
    out = []
    for t in (0, 1, 2, 3 + k - 1, 3 + k, 3 + k):
        nv = tables[t].size.bit_length() - 1
        pt = [(rng.randrange(P), rng.randrange(P)) for _ in range(nv)]
        out.append((t, [x for p in pt for x in p], tp.py_mle(tables[t], pt)))
    return out


_HOST = {}


def host_case(params, d, log2_row, tag):
    """per (tag, log2_row), computed once and never changed: the host commitment to the witness with arrays d, six claims, Q = 4N and
    the host opening"""
    key = (tag, log2_row)
    if key not in _HOST:
        w = hg.Witness.from_arrays(params, d)
        cm = hg.Commitment.secrets(None, params, w, log2_row)
        claims = kind_claims(params, d, 0x6c1 + len(_HOST))
        Q = 4 * (4 << cm.log2_row)
        _HOST[key] = dict(w=w, cm=cm, claims=claims, Q=Q, opening=cm.open(claims, Q))
    return _HOST[key]


def same_as_host(cm, case):
    assert cm.root == case["cm"].root
    assert cm.nvars == case["cm"].nvars and cm.log2_row == case["cm"].log2_row
    assert cm.open(case["claims"], case["Q"]) == case["opening"]


def zero_enc(n, k):
    return (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((k, n), dtype=np.int64))


def raw_pipeline(ctx_h, pk_h, run, log2_row, cap, reason_cap=0, ws=False):
    """the C entry on sentinel-filled outputs: (return value, dict of the outputs)"""
    n = len(run)
    arrs = [[np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in enc] for enc in run]
    cols = [(hg.i64p * max(n, 1))(*[x[f].ctypes.data_as(hg.i64p) for x in arrs]) for f in range(4)]
    o = dict(buf=(C.c_uint8 * (max(n, 1) * max(cap, 1)))(), lens=(C.c_size_t * max(n, 1))(*[7] * max(n, 1)), st=(C.c_int * max(n, 1))(*[9] * max(n, 1)),
             cms=(C.c_void_p * max(n, 1))(), roots=(C.c_uint8 * (32 * max(n, 1)))(), hs=(C.c_void_p * max(n, 1))() if ws else None,
             reasons=C.create_string_buffer(max(n, 1) * reason_cap) if reason_cap else None, keep=arrs)
    C.memset(o["cms"], SENTINEL, C.sizeof(o["cms"]))
    C.memset(o["roots"], SENTINEL, C.sizeof(o["roots"]))
    rc = hg.lib().hg_prove_encryptions_committed(ctx_h, pk_h, *cols, n, log2_row, o["buf"], cap, o["lens"], o["st"], o["cms"], o["roots"], o["hs"], o["reasons"],
                                                 reason_cap, None)
    return rc, o


# ---- not gpu ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    for name in (VALUES, PIPE):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in hg.EXPORTS and hasattr(hg.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rs), name


def test_without_a_context():
    n, k = 1024, 1
    bfv = hg.BfvEncrypt.new(n, k)
    pk_host = bfv.setup(None)
    for run in ([], [zero_enc(n, k)], [zero_enc(n, k)] * 3):
        with pytest.raises(hg.HgError, match="^" + PIPE + ": needs a device context"):
            hg.prove_encryptions_committed(None, pk_host, run)
        rc, o = raw_pipeline(None, pk_host.h, run, 0, 1 << 10)
        assert rc == -1 and _last().startswith(PIPE + ": needs a device context")
        assert not any(o["cms"][i] for i in range(len(run)))                        # every handle slot is NULL after an error of the call
    # with a null context no hg_values can exist: the null argument is reported first
    h, root = C.c_void_p(0xDEAD), (C.c_uint8 * 32)()
    assert hg.lib().hg_secrets_commit_values(None, pk_host.h, None, 0, C.byref(h), root) == -1
    assert _last() == VALUES + ": null argument" and not h.value
    with pytest.raises(hg.HgError, match="^" + VALUES + ": null argument$"):
        hg.Commitment.from_values(None, pk_host, None)
    pk_host.free()


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


_KEYS = {}


def key_case(ctx, key):
    """per parameter set, once: the key on the module's context and two synthetic witnesses"""
    if key not in _KEYS:
        params = params_of(key)
        bfv = hg.BfvEncrypt(params)
        ds = [hg.Witness.synthetic(params, 0xC0117 + 7 * i + params.n).arrays() for i in range(2)]
        _KEYS[key] = dict(params=params, bfv=bfv, pk=bfv.setup(ctx), ds=ds)
    return _KEYS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("key,log2_row", SHAPES, ids=IDS)
def test_commit_from_resident_values(ctx, key, log2_row):
    kc = key_case(ctx, key)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, d, log2_row, (key, i)) for i, d in enumerate(kc["ds"])]
    if (key, log2_row) == ((1024, 1), 0):
        assert cases[0]["cm"].log2_row == 7 and cases[0]["cm"].nvars == [11] * 4 + [10]
    v = hg.witness_gen(ctx, pk, cases[0]["w"])
    cm = hg.Commitment.from_values(ctx, pk, v, log2_row)
    same_as_host(cm, cases[0])
    assert hg.pcs_verify(cm.root, cm.nvars, cases[0]["claims"], cases[0]["opening"], cases[0]["Q"], log2_row) == (True, "")
    # the handle owns its rows: a refill of the values leaves it alone, and a new call commits to the new tables
    hg.witness_gen_into(ctx, pk, cases[1]["w"], v)
    other = hg.Commitment.from_values(ctx, pk, v, log2_row)
    assert other.root == cases[1]["cm"].root != cm.root
    assert cm.open(cases[0]["claims"], cases[0]["Q"]) == cases[0]["opening"]
    same_as_host(other, cases[1])
    v.free()
    assert cm.open(cases[0]["claims"], 5) == cases[0]["cm"].open(cases[0]["claims"], 5)


@pytest.mark.gpu
def test_claims_of_verify_public_open_against_a_values_handle(ctx):
    kc = key_case(ctx, (1024, 1))
    params, pk, bfv = kc["params"], kc["pk"], kc["bfv"]
    w = hg.Witness.from_arrays(params, kc["ds"][0])
    proof, _ = bfv.prove(ctx, pk, w)
    ok, why, cl = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 0, ctx=ctx, device=True)
    assert ok, why
    v = hg.witness_gen(ctx, pk, w)
    cm = hg.Commitment.from_values(ctx, pk, v)
    host = hg.Commitment.secrets(None, params, w)
    opening = cm.open_claims(params, cl)
    assert cm.root == host.root and opening == host.open_claims(params, cl)
    assert hg.claims_verify(params, cm.root, cl, opening) == (True, "")
    v.free()


@pytest.mark.gpu
def test_the_launches_are_a_profiler_class(ctx):
    kc = key_case(ctx, (1024, 1))
    v = hg.witness_gen(ctx, kc["pk"], hg.Witness.from_arrays(kc["params"], kc["ds"][0]))
    ctx.profile(2)
    ctx.profile_reset()
    try:
        cm = hg.Commitment.from_values(ctx, kc["pk"], v)
        stat = [s for s in ctx.profile_get(256) if s["name"] == "pcs_commit_values"]
    finally:
        ctx.profile(0)
    assert cm.root == host_case(kc["params"], kc["ds"][0], 0, ((1024, 1), 0))["cm"].root
    assert len(stat) == 1 and stat[0]["launches"] >= 4 and stat[0]["total_ms"] > 0
    v.free()


@pytest.mark.gpu
def test_errors_of_commit_from_values(ctx):
    kc = key_case(ctx, (1024, 1))
    params, pk, bfv = kc["params"], kc["pk"], kc["bfv"]
    case = host_case(params, kc["ds"][0], 0, ((1024, 1), 0))
    v = hg.witness_gen(ctx, pk, case["w"])
    pk_host, pk_other = bfv.setup(None), bfv.setup(ctx)
    L = hg.lib()

    def refused(key, values, log2_row, text):
        h, root = C.c_void_p(0xDEAD), (C.c_uint8 * 32)()
        assert L.hg_secrets_commit_values(ctx.h, key.h if key else None, values.h if values else None, log2_row, C.byref(h), root) == -1
        assert _last().startswith(VALUES + ": ") and re.search(text, _last()), _last()
        assert not h.value
        assert hg.Commitment.from_values(ctx, pk, v).root == case["cm"].root        # the context still commits
    refused(None, v, 0, "null argument")
    refused(pk, None, 0, "null argument")
    refused(pk_host, v, 0, "host-only")
    refused(pk_other, v, 0, "another prover key")
    refused(pk, v, 11, "log2_row")                                                  # above P = 10, the variables of r2is
    h = C.c_void_p(0xDEAD)
    assert L.hg_secrets_commit_values(ctx.h, pk.h, v.h, 0, C.byref(h), None) == -1 and _last() == VALUES + ": null argument" and not h.value
    assert L.hg_secrets_commit_values(None, pk.h, v.h, 0, C.byref(h), (C.c_uint8 * 32)()) == -1 and _last() == VALUES + ": no context"
    # a rank's share of hg_witness_gen_shard holds the tables the rank reads: where a secret input is among the others the call is
    # refused and names it; a share that happens to hold all five kinds commits like any values object. Which shares lack one follows
    # from the dealing of the nodes: of the shares below at least one must
    lacking = 0
    for rank, world in ((0, 2), (1, 2), (1, 4), (3, 4)):
        shard = hg.witness_gen_shard(ctx, pk, case["w"], rank, world)
        if shard.info()["resident_tables"] == shard.info()["tables"]:
            assert hg.Commitment.from_values(ctx, pk, shard).root == case["cm"].root
        else:
            h, root = C.c_void_p(0xDEAD), (C.c_uint8 * 32)()
            rc = L.hg_secrets_commit_values(ctx.h, pk.h, shard.h, 0, C.byref(h), root)
            if rc == 0:                                                             # (it lacks only tables that are not committed to)
                assert bytes(root) == case["cm"].root
                L.hg_pcs_free(h)
            else:
                assert rc == -1 and re.match(VALUES + r": input (0|1|2|4|5) is not resident", _last()) and not h.value, _last()
                lacking += 1
        shard.free()
    assert lacking >= 1
    same_as_host(hg.Commitment.from_values(ctx, pk, v), case)
    v.free(); pk_host.free(); pk_other.free()


def pipeline_case(ctx, key, count, salt):
    """a run of encryptions with, per item, the proof and the derived witness's arrays of derive-then-prove"""
    kc = key_case(ctx, key)
    encs = tpe.synthetic_encs(kc["params"], count, salt)
    want, tabs = tpe.reference_proofs(ctx, kc["bfv"], kc["pk"], encs)
    return kc, encs, want, tabs


def check_run(out, want, cases, opened=True):
    proofs, status, why, cms, roots, ws, tm = out
    n = len(want)
    assert status == [0] * n and why == [""] * n, (status, why)
    assert proofs == want
    assert roots == [c["cm"].root for c in cases] and [cm.root for cm in cms] == roots
    if opened:
        for cm, case in zip(cms, cases):
            same_as_host(cm, case)
    assert tm["total_ms"] > 0 and tm["witness_ms"] >= tm["upload_ms"] > 0 and tm["prove_ms"] > 0 and tm["gpu_ms"] > 0
    return cms


@pytest.mark.gpu
@pytest.mark.parametrize("key,other_row", [((1024, 1), 2), ((4096, 2), 3), (DERIVED, 9)], ids=["1024x1", "4096x2", "derived"])
def test_pipeline_handles_are_those_of_the_host_form(ctx, key, other_row):
    run = 5
    kc, encs, want, tabs = pipeline_case(ctx, key, run, 0xC0DE)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, tabs[i], 0, (key, "pipe", i)) for i in range(run)]
    assert hg.prove_encryptions(ctx, pk, encs, witnesses=False)[0] == want
    for call in range(3):                                                          # walked, recorded and replayed schedules
        check_run(hg.prove_encryptions_committed(ctx, pk, encs), want, cases, opened=(call != 1))
    ctx.set_option("graph", 0)
    try:
        check_run(hg.prove_encryptions_committed(ctx, pk, encs), want, cases)
    finally:
        ctx.set_option("graph", 1)
    for length in (1, 2, 3):                                                       # short runs, rotated so that both table sets see other items
        sub, subwant, subcases = (x[length:] + x[:length] for x in (encs, want, cases))
        check_run(hg.prove_encryptions_committed(ctx, pk, sub[:length]), subwant[:length], subcases[:length])
    out = hg.prove_encryptions_committed(ctx, pk, encs, witnesses=True)
    check_run(out, want, cases, opened=False)
    for i in range(run):
        tpe.same(out[5][i].arrays(), tabs[i], hg.Witness.FIELDS)
    rowcases = [host_case(params, tabs[i], other_row, (key, "pipe", i)) for i in range(2)]
    check_run(hg.prove_encryptions_committed(ctx, pk, encs[:2], log2_row=other_row), want[:2], rowcases)
    assert hg.prove_encryptions_committed(ctx, pk, [])[:6] == ([], [], [], [], [], [])           # n_enc == 0 returns 0
    with pytest.raises(hg.HgError, match="^" + PIPE + ": .*log2_row"):
        hg.prove_encryptions_committed(ctx, pk, encs[:1], log2_row=14)
    check_run(hg.prove_encryptions_committed(ctx, pk, encs[:1]), want[:1], cases[:1])


@pytest.mark.gpu
def test_refused_items(ctx):
    key, n = (4096, 2), 4096
    kc, clean, want, tabs = pipeline_case(ctx, key, 6, 0xBAD)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, tabs[i], 0, (key, "refused", i)) for i in range(6)]
    e_bad = tpe.spoiled(clean[1], 1, 0, 17, int(params.e_bound) + 1)
    a_bad = tpe.spoiled(clean[4], 3, 1, n - 3, (int(params.qis[1]) + 1) // 2)
    run = [clean[0], e_bad, clean[2], clean[3], a_bad, clean[5]]
    zero = bytes(32)
    for call in range(3):
        proofs, status, why, cms, roots, ws, tm = hg.prove_encryptions_committed(ctx, pk, run)
        assert status == [0, 1, 0, 0, 1, 0], (call, status, why)
        assert why[1].startswith(PIPE + ": encryption 1: table e:") and why[4].startswith(PIPE + ": encryption 4: table ais of modulus 1 ")
        for i in (1, 4):
            assert proofs[i] is None and cms[i] is None and roots[i] == zero
        for i in (0, 2, 3, 5):
            assert proofs[i] == want[i] and roots[i] == cases[i]["cm"].root and why[i] == ""
            same_as_host(cms[i], cases[i])
    # the C entry itself on sentinel-filled outputs
    cap = 1 << 20
    rc, o = raw_pipeline(ctx.h, pk.h, run, 0, cap, reason_cap=40)
    assert rc == 2 and list(o["st"]) == [0, 1, 0, 0, 1, 0]
    for i in (1, 4):
        assert not o["cms"][i] and bytes(o["roots"][32 * i:32 * i + 32]) == zero and o["lens"][i] == 0
    for i in (0, 2, 3, 5):
        assert bytes(o["buf"][i * cap:i * cap + o["lens"][i]]) == want[i] and bytes(o["roots"][32 * i:32 * i + 32]) == cases[i]["cm"].root
        cm = hg.Commitment(C.c_void_p(o["cms"][i]), cases[i]["cm"].root, ctx, cases[i]["cm"].nvars, cases[i]["cm"].log2_row)
        assert cm.open(cases[i]["claims"], 9) == cases[i]["cm"].open(cases[i]["claims"], 9)
        cm.free()
    assert o["reasons"].raw[40:80] == (PIPE + ": encryption 1: table e:")[:39].encode() + b"\0" and o["reasons"].raw[0:1] == b"\0"
    # a refused first item, a refused last item, every item refused
    proofs, status, _, cms, roots, _, _ = hg.prove_encryptions_committed(ctx, pk, [e_bad, clean[0], clean[2]])
    assert status == [1, 0, 0] and proofs[1:] == [want[0], want[2]] and cms[0] is None and roots == [zero, cases[0]["cm"].root, cases[2]["cm"].root]
    same_as_host(cms[1], cases[0]); same_as_host(cms[2], cases[2])
    proofs, status, _, cms, roots, _, _ = hg.prove_encryptions_committed(ctx, pk, [clean[3], clean[5], a_bad])
    assert status == [0, 0, 1] and proofs[:2] == [want[3], want[5]] and cms[2] is None and roots == [cases[3]["cm"].root, cases[5]["cm"].root, zero]
    same_as_host(cms[0], cases[3]); same_as_host(cms[1], cases[5])
    proofs, status, _, cms, roots, _, tm = hg.prove_encryptions_committed(ctx, pk, [e_bad, a_bad, e_bad])
    assert status == [1, 1, 1] and proofs == [None] * 3 and cms == [None] * 3 and roots == [zero] * 3 and tm["upload_ms"] == 0
    check_run(hg.prove_encryptions_committed(ctx, pk, clean[:2]), want[:2], cases[:2])


@pytest.mark.gpu
def test_ownership(ctx):
    key = (1024, 1)
    kc, encs, want, tabs = pipeline_case(ctx, key, 5, 0xC0DE)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, tabs[i], 0, (key, "pipe", i)) for i in range(5)]
    for order in ([4, 3, 2, 1, 0], [1, 3, 0, 4, 2]):                                # in reverse, interleaved
        cms = hg.prove_encryptions_committed(ctx, pk, encs)[3]
        alive = set(range(5))
        for i in order:
            cms[i].free()
            alive.discard(i)
            for j in alive:
                same_as_host(cms[j], cases[j])
    check_run(hg.prove_encryptions_committed(ctx, pk, encs), want, cases)         # every handle of the runs above is freed
    # a handle of the pipeline and one of hg_secrets_commit_values in one open batch
    proof, _ = kc["bfv"].prove(ctx, pk, cases[0]["w"])
    got = hg.verify_public_batch(ctx, pk, [hg.Instance.from_witness(cases[i]["w"]) for i in (0, 1)], [want[0], want[1]], 0)
    assert proof == want[0] and all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    piped = hg.prove_encryptions_committed(ctx, pk, encs[:1])[3][0]
    v = hg.witness_gen(ctx, pk, cases[1]["w"])
    single = hg.Commitment.from_values(ctx, pk, v)
    opened = hg.claims_open_batch(ctx, params, [piped, single], cls)
    assert opened == [(piped.open_claims(params, cls[0]), ""), (single.open_claims(params, cls[1]), "")]
    assert [b for b, _ in opened] == [cases[i]["cm"].open_claims(params, cls[i]) for i in (0, 1)]
    v.free()


@pytest.mark.gpu
def test_neighbours_share_the_context(ctx):
    key = (4096, 2)
    kc, encs, want, tabs = pipeline_case(ctx, key, 4, 0x9E16)
    params, pk, bfv = kc["params"], kc["pk"], kc["bfv"]
    cases = [host_case(params, tabs[i], 0, (key, "nb", i)) for i in range(4)]
    hws = [c["w"] for c in cases]
    roots = [c["cm"].root for c in cases]

    def neighbours():
        batch = hg.Commitment.secrets_batch(ctx, params, hws)
        return {"prove": [bfv.prove(ctx, pk, w)[0] for w in hws], "stream": bfv.prove_stream(ctx, pk, hws)[0],
                "pipe": hg.prove_encryptions(ctx, pk, encs, witnesses=False)[0], "roots": [cm.root for cm in batch],
                "open": batch[3].open(cases[3]["claims"], 9)}
    before = neighbours()
    assert before["prove"] == before["stream"] == before["pipe"] == want and before["roots"] == roots
    for rnd in range(3):                                                           # committed run, neighbours, committed run, ...
        check_run(hg.prove_encryptions_committed(ctx, pk, encs), want, cases, opened=(rnd == 2))
        assert neighbours() == before, rnd
    # another key on the same context: the pipeline's buffers are rebuilt for it, and again for the first key
    k2, encs2, want2, tabs2 = pipeline_case(ctx, (1024, 1), 3, 0xC0DE)
    cases2 = [host_case(k2["params"], tabs2[i], 0, ((1024, 1), "pipe", i)) for i in range(3)]
    check_run(hg.prove_encryptions_committed(ctx, k2["pk"], encs2), want2, cases2)
    check_run(hg.prove_encryptions_committed(ctx, pk, encs[::-1]), want[::-1], cases[::-1])


@pytest.mark.gpu
def test_end_to_end(ctx):
    """committed pipeline -> publish proof and root -> hg_verify_public_batch on the ciphertexts -> hg_claims_open_batch on the handles ->
    hg_claims_verify_batch against the roots"""
    key = (1024, 1)
    kc, encs, want, tabs = pipeline_case(ctx, key, 3, 0xC0DE)
    params, pk = kc["params"], kc["pk"]
    proofs, status, _, cms, roots, _, _ = hg.prove_encryptions_committed(ctx, pk, encs)
    assert status == [0] * 3 and len(set(roots)) == 3
    insts = []
    for i in range(3):                                                             # what a verifier holds: a and ct0
        a, ct0 = hg.Instance.from_witness(hg.Witness.from_arrays(params, tabs[i])).coeffs()
        assert (a.reshape(params.k, params.n) == encs[i][3]).all()
        insts.append(hg.Instance.from_ciphertext(params, a, ct0))
    got = hg.verify_public_batch(ctx, pk, insts, proofs, 0)
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    opened = hg.claims_open_batch(ctx, params, cms, cls)
    assert all(b is not None and why == "" for b, why in opened)
    openings = [b for b, _ in opened]
    assert hg.claims_verify_batch(ctx, params, roots, cls, openings) == [(True, "")] * 3
    swapped = [roots[1], roots[0], roots[2]]
    res = hg.claims_verify_batch(ctx, params, swapped, cls, openings)
    assert res[2] == (True, "") and res[0] == res[1] == (False, "pcs: Merkle path mismatch at query 0"), res


@pytest.mark.gpu
def test_committed_pipeline_is_not_slower_than_prove_then_commit(ctx):
    """(32768, 16), runs of 8 after warm-up, the two forms alternating in one process, median of 5 each. Leg A: the committed pipeline
    without host handles, its commitments freed. Leg B, what a service writes without it: hg_prove_encryptions with host handles, then
    hg_secrets_commit_batch on them, handles and commitments freed. A does a strict subset of B's device work and none of its host
    round trip. Asserted: A is not slower than B."""
    n, k, run = 32768, 16, 8
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    encs = [tpe.polys_of_tables(params, hg.Witness.synthetic(params, 0x71AE + 3 * i).arrays()) for i in range(run)]

    def leg_a():
        t0 = time.perf_counter()
        proofs, status, _, cms, roots, _, tm = hg.prove_encryptions_committed(ctx, pk, encs, cap_each=1 << 22)
        for cm in cms:
            cm.free()
        ms = (time.perf_counter() - t0) * 1e3 / run
        assert status == [0] * run
        return ms, proofs, roots, tm

    def leg_b():
        t0 = time.perf_counter()
        proofs, status, _, ws, tm = hg.prove_encryptions(ctx, pk, encs, cap_each=1 << 22, witnesses=True)
        cms = hg.Commitment.secrets_batch(ctx, params, ws)
        roots = [cm.root for cm in cms]
        for cm in cms:
            cm.free()
        del ws[:]
        ms = (time.perf_counter() - t0) * 1e3 / run
        assert status == [0] * run
        return ms, proofs, roots, tm
    for _ in range(2):                                                         # warm-up: the launch graphs, staging, slabs, thread pool
        _, want, want_roots, _ = leg_b()
        _, proofs, roots, _ = leg_a()
        assert proofs == want and roots == want_roots
    ta, tb, commit, gpu, gpu_b = [], [], [], [], []
    for _ in range(5):
        ms, proofs, roots, tm = leg_b()
        assert proofs == want and roots == want_roots
        tb.append(ms); gpu_b.append(tm["gpu_ms"] / run)
        ms, proofs, roots, tm = leg_a()
        assert proofs == want and roots == want_roots
        ta.append(ms); commit.append(tm["upload_ms"] / run); gpu.append(tm["gpu_ms"] / run)
    ms_a, ms_b = statistics.median(ta), statistics.median(tb)
    print("\nn=%d k=%d run=%d per item: committed pipeline %.3f ms (%s), prove_encryptions + secrets_commit_batch %.3f ms (%s), ratio %.3f, "
          "commit device time %.3f ms, gpu_ms/n %.3f (beside the commit) against %.3f (alone)"
          % (n, k, run, ms_a, " ".join("%.3f" % t for t in ta), ms_b, " ".join("%.3f" % t for t in tb), ms_a / ms_b, statistics.median(commit),
             statistics.median(gpu), statistics.median(gpu_b)))
    assert ms_a <= ms_b, (ms_a, ms_b)
    pk.free()
