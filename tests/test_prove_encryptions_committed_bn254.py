"""hg_prove_encryptions_committed_bn254: the BN254 encryption pipeline that also commits to the five secret inputs of every item, from
the laid-out u64 tables in HBM (bn::pcs_commit_words_enqueue: k_bnpcs_stage_words lifts and stages in one pass).

The yardstick is never the pipeline: hg.Commitment.secrets_bn254(None, params, w, log2_row) (the host form) on the witness of the item
and .open(..) on it; hg.prove_encryptions_bn254(..) for the proof bytes. Roots are compared exactly on every call (every column of M
enters the root); once per item and shape an opening of six claims (one on each kind of table, two on r2is, at random Fr points)
with Q = 4N queries is compared byte for byte with the host opening, which shows that the handle's rows and matrix in HBM are what
was hashed; elsewhere a short opening (Q = 9).

Shapes, none of them the workload's:
  (1024,1) log2_row 0   c = 7, N = 512, R = 72: four-step LDS NTT; the tree wholly in the top kernel
  (1024,1) log2_row 2   N = 16, R = 2304: radix-2 stages, many rows
  (1024,1) log2_row 1   C = 2: the narrowest row (one 16-byte unit a row)
  (1024,1) log2_row 10  every table one or two rows
  (4096,2) log2_row 0   c = 8, N = 1024: a per-level tree launch; two r1is tables; r2is with P+1 variables
  derived (1024,2)      k = 2 with the smallest tables"""
import ctypes as C
import os
import random
import re
import statistics
import time

import pytest

import test_pcs_bn254 as tpn
import test_prove_encryptions_bn254 as tpb
import test_prove_encryptions_committed as tpc
from hglib import hg, ROOT

R = tpn.R
PIPE, PLAIN, GL_PIPE = "hg_prove_encryptions_committed_bn254", "hg_prove_encryptions_bn254", "hg_prove_encryptions_committed"
SENTINEL = 0x5a
DERIVED = tpc.DERIVED
ROWS = {(1024, 1): (0, 2, 1, 10), (4096, 2): (0,), DERIVED: (0,)}
ZERO = bytes(32)


def _last():
    return hg.lib().hg_last_error().decode()


def kind_claims(params, d, seed):
    """six claims at random Fr points: s, e, k1, the last r1is table, r2is twice; the values from the signed lift of the words"""
    tables = tpc.secret_tables(params, d)
    k = params.k
    rng = random.Random(seed)
    lifted = {}
    out = []
    for t in (0, 1, 2, 3 + k - 1, 3 + k, 3 + k):
        if t not in lifted:
            lifted[t] = [tpn.fr_of(x) for x in tables[t]]
        pt = [rng.randrange(R) for _ in range(tables[t].size.bit_length() - 1)]
        out.append((t, pt, tpn.py_mle(lifted[t], pt)))
    return out


_HOST = {}


def host_case(params, d, log2_row, tag):
    """per (tag, log2_row), computed once and never changed: the host commitment to the witness with arrays d, six claims, Q = 4N, the
    host opening and a short one (Q = 9)"""
    key = (tag, log2_row)
    if key not in _HOST:
        w = hg.Witness.from_arrays(params, d)
        cm = hg.Commitment.secrets_bn254(None, params, w, log2_row)
        claims = kind_claims(params, d, 0xb6c1 + len(_HOST))
        Q = 4 * (4 << cm.log2_row)
        _HOST[key] = dict(w=w, cm=cm, claims=claims, Q=Q, opening=cm.open(claims, Q), short=cm.open(claims, 9))
    return _HOST[key]


def same_as_host(cm, case, full=True):
    assert cm.field == "bn254" and cm.root == case["cm"].root
    assert cm.nvars == case["cm"].nvars and cm.log2_row == case["cm"].log2_row
    if full:
        assert cm.open(case["claims"], case["Q"]) == case["opening"]
    else:
        assert cm.open(case["claims"], 9) == case["short"]


def raw_pipeline(ctx_h, pk_h, run, log2_row, cap, reason_cap=0, ws=False):
    """the C entry on sentinel-filled outputs: (return value, dict of the outputs)"""
    n = len(run)
    cols, keep = tpb.c_columns(run) if n else ([(hg.i64p * 1)() for _ in range(4)], None)
    o = dict(buf=(C.c_uint8 * (max(n, 1) * max(cap, 1)))(), lens=(C.c_size_t * max(n, 1))(*[7] * max(n, 1)), st=(C.c_int * max(n, 1))(*[9] * max(n, 1)),
             cms=(C.c_void_p * max(n, 1))(), roots=(C.c_uint8 * (32 * max(n, 1)))(), hs=(C.c_void_p * max(n, 1))() if ws else None,
             reasons=C.create_string_buffer(max(n, 1) * reason_cap) if reason_cap else None, keep=keep)
    C.memset(o["cms"], SENTINEL, C.sizeof(o["cms"]))
    C.memset(o["roots"], SENTINEL, C.sizeof(o["roots"]))
    rc = getattr(hg.lib(), PIPE)(ctx_h, pk_h, *cols, n, log2_row, o["buf"], cap, o["lens"], o["st"], o["cms"], o["roots"], o["hs"], o["reasons"], reason_cap, None)
    return rc, o


# ---- not gpu ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_listed_exported_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hg.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "hg-shim", "src", "ffi.rs")).read()
    assert re.search(r"\b%s\s*\(" % PIPE, hdr)
    assert PIPE in hg.EXPORTS and hasattr(hg.lib(), PIPE)
    assert re.search(r"pub fn %s\(" % PIPE, rs)
    assert callable(hg.prove_encryptions_committed_bn254)


def test_without_a_context():
    n, k = 1024, 1
    bfv = hg.BfvEncrypt.new(n, k)
    pk_host = bfv.setup(None)
    for run in ([], [tpc.zero_enc(n, k)], [tpc.zero_enc(n, k)] * 3):
        with pytest.raises(hg.HgError, match="^" + PIPE + ": needs a device context"):
            hg.prove_encryptions_committed_bn254(None, pk_host, run)
        rc, o = raw_pipeline(None, pk_host.h, run, 0, 1 << 10)
        assert rc == -1 and _last().startswith(PIPE + ": needs a device context")
        assert not any(o["cms"][i] for i in range(len(run)))                        # every handle slot is NULL after an error of the call
    pk_host.free()


# ---- gpu -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


_KEYS = {}


def key_case(ctx, key):
    """per parameter set, once: the key on the module's context"""
    if key not in _KEYS:
        params = tpc.params_of(key)
        bfv = hg.BfvEncrypt(params)
        _KEYS[key] = dict(params=params, bfv=bfv, pk=bfv.setup(ctx))
    return _KEYS[key]


_RUNS = {}


def pipeline_case(ctx, key, count, salt):
    """per (key, count, salt), once: a run of encryptions with, per item, the proof of hg_prove_encryptions_bn254 and the arrays of the
    witness hg_witness_derive gives for it"""
    kc = key_case(ctx, key)
    if (key, count, salt) not in _RUNS:
        encs = tpb.synthetic_encs(kc["params"], count, salt)
        want, status, why, ws, _ = hg.prove_encryptions_bn254(ctx, kc["pk"], encs, witnesses=False)
        assert status == [0] * count, why
        tabs = [hg.Witness.derive(ctx, kc["params"], hg.encryption_layout(kc["params"], *enc)).arrays() for enc in encs]
        _RUNS[(key, count, salt)] = (encs, want, tabs)
    return (kc,) + _RUNS[(key, count, salt)]


def check_run(out, want, cases, full=False):
    proofs, status, why, cms, roots, ws, tm = out
    n = len(want)
    assert status == [0] * n and why == [""] * n, (status, why)
    assert proofs == want
    assert roots == [c["cm"].root for c in cases] and [cm.root for cm in cms] == roots
    for cm, case in zip(cms, cases):
        same_as_host(cm, case, full)
    assert tm["total_ms"] > 0 and tm["witness_ms"] >= tm["upload_ms"] > 0 and tm["prove_ms"] > 0       # the commit ran
    assert [tm[f] for f in ("gpu_ms", "enqueue_ms", "sync_ms", "replay_ms")] == [0.0] * 4
    return cms


@pytest.mark.gpu
@pytest.mark.parametrize("key,other_row", [((1024, 1), 2), ((4096, 2), 3), (DERIVED, 9)], ids=["1024x1", "4096x2", "derived"])
def test_pipeline_handles_are_those_of_the_host_form(ctx, key, other_row):
    run = 5
    kc, encs, want, tabs = pipeline_case(ctx, key, run, 0xC0DE)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, tabs[i], 0, (key, "pipe", i)) for i in range(run)]
    if key == (1024, 1):
        assert cases[0]["cm"].log2_row == 7 and cases[0]["cm"].nvars == [11] * 4 + [10]
    for call in range(3):                                                          # three successive calls; the full opening once per item and shape
        check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs), want, cases, full=(call == 0))
    for length in (1, 2, 3):                                                       # short runs, rotated so that both table sets see other items
        sub, subwant, subcases = (x[length:] + x[:length] for x in (encs, want, cases))
        check_run(hg.prove_encryptions_committed_bn254(ctx, pk, sub[:length]), subwant[:length], subcases[:length])
    out = hg.prove_encryptions_committed_bn254(ctx, pk, encs, witnesses=True)
    check_run(out, want, cases)
    plain = hg.prove_encryptions_bn254(ctx, pk, encs, witnesses=True)
    for i in range(run):
        tpb.same(out[5][i].arrays(), tabs[i], hg.Witness.FIELDS)
        tpb.same(out[5][i].arrays(), plain[3][i].arrays(), hg.Witness.FIELDS)
    rowcases = [host_case(params, tabs[i], other_row, (key, "pipe", i)) for i in range(2)]        # a second log2_row: the commit buffers are rebuilt
    check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs[:2], log2_row=other_row), want[:2], rowcases, full=True)
    assert hg.prove_encryptions_committed_bn254(ctx, pk, [])[:6] == ([], [], [], [], [], [])   # n_enc == 0 returns 0
    with pytest.raises(hg.HgError, match="^" + PIPE + ": .*log2_row"):
        hg.prove_encryptions_committed_bn254(ctx, pk, encs[:1], log2_row=14)
    check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs[:1]), want[:1], cases[:1])


@pytest.mark.gpu
@pytest.mark.parametrize("log2_row", ROWS[(1024, 1)][1:])
def test_other_row_lengths(ctx, log2_row):
    key = (1024, 1)
    kc, encs, want, tabs = pipeline_case(ctx, key, 5, 0xC0DE)
    cases = [host_case(kc["params"], tabs[i], log2_row, (key, "pipe", i)) for i in range(3)]
    if log2_row == 2:
        assert cases[0]["cm"].log2_row == 2 and cases[0]["Q"] == 64
    check_run(hg.prove_encryptions_committed_bn254(ctx, kc["pk"], encs[:3], log2_row=log2_row), want[:3], cases, full=True)


@pytest.mark.gpu
def test_refused_items(ctx):
    key, n = (4096, 2), 4096
    kc, clean, want, tabs = pipeline_case(ctx, key, 6, 0xBAD)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, tabs[i], 0, (key, "refused", i)) for i in range(6)]
    e_bad = tpb.spoiled(clean[1], 1, 0, 17, int(params.e_bound) + 1)
    a_bad = tpb.spoiled(clean[4], 3, 1, n - 3, (int(params.qis[1]) + 1) // 2)
    run = [clean[0], e_bad, clean[2], clean[3], a_bad, clean[5]]
    for call in range(3):
        proofs, status, why, cms, roots, ws, tm = hg.prove_encryptions_committed_bn254(ctx, pk, run)
        assert status == [0, 1, 0, 0, 1, 0], (call, status, why)
        assert why[1].startswith(PIPE + ": encryption 1: table e:") and why[4].startswith(PIPE + ": encryption 4: table ais of modulus 1 ")
        for i in (1, 4):
            assert proofs[i] is None and cms[i] is None and roots[i] == ZERO
        for i in (0, 2, 3, 5):
            assert proofs[i] == want[i] and roots[i] == cases[i]["cm"].root and why[i] == ""
            same_as_host(cms[i], cases[i], full=(call == 0))
    # the C entry itself on sentinel-filled outputs
    cap = 1 << 22
    rc, o = raw_pipeline(ctx.h, pk.h, run, 0, cap, reason_cap=40)
    assert rc == 2 and list(o["st"]) == [0, 1, 0, 0, 1, 0]
    for i in (1, 4):
        assert not o["cms"][i] and bytes(o["roots"][32 * i:32 * i + 32]) == ZERO and o["lens"][i] == 0
    for i in (0, 2, 3, 5):
        assert bytes(o["buf"][i * cap:i * cap + o["lens"][i]]) == want[i] and bytes(o["roots"][32 * i:32 * i + 32]) == cases[i]["cm"].root
        cm = hg.Commitment(C.c_void_p(o["cms"][i]), cases[i]["cm"].root, ctx, cases[i]["cm"].nvars, cases[i]["cm"].log2_row, "bn254")
        same_as_host(cm, cases[i], full=False)
        cm.free()
    assert o["reasons"].raw[40:80] == (PIPE + ": encryption 1: table e:")[:39].encode() + b"\0" and o["reasons"].raw[0:1] == b"\0"
    # a refused first item, a refused last item, every item refused, and a clean run behind it
    proofs, status, _, cms, roots, _, _ = hg.prove_encryptions_committed_bn254(ctx, pk, [e_bad, clean[0], clean[2]])
    assert status == [1, 0, 0] and proofs[1:] == [want[0], want[2]] and cms[0] is None and roots == [ZERO, cases[0]["cm"].root, cases[2]["cm"].root]
    same_as_host(cms[1], cases[0], full=False); same_as_host(cms[2], cases[2], full=False)
    proofs, status, _, cms, roots, _, _ = hg.prove_encryptions_committed_bn254(ctx, pk, [clean[3], clean[5], a_bad])
    assert status == [0, 0, 1] and proofs[:2] == [want[3], want[5]] and cms[2] is None and roots == [cases[3]["cm"].root, cases[5]["cm"].root, ZERO]
    same_as_host(cms[0], cases[3], full=False); same_as_host(cms[1], cases[5], full=False)
    proofs, status, _, cms, roots, _, tm = hg.prove_encryptions_committed_bn254(ctx, pk, [e_bad, a_bad, e_bad])
    assert status == [1, 1, 1] and proofs == [None] * 3 and cms == [None] * 3 and roots == [ZERO] * 3 and tm["upload_ms"] == 0
    check_run(hg.prove_encryptions_committed_bn254(ctx, pk, clean[:2]), want[:2], cases[:2])


@pytest.mark.gpu
def test_ownership(ctx):
    key = (1024, 1)
    kc, encs, want, tabs = pipeline_case(ctx, key, 5, 0xC0DE)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, tabs[i], 0, (key, "pipe", i)) for i in range(5)]
    for order in ([4, 3, 2, 1, 0], [1, 3, 0, 4, 2]):                                # in reverse, interleaved
        cms = hg.prove_encryptions_committed_bn254(ctx, pk, encs)[3]
        alive = set(range(5))
        for i in order:
            cms[i].free()
            alive.discard(i)
            for j in alive:
                same_as_host(cms[j], cases[j], full=False)
    check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs), want, cases)   # every handle of the runs above is freed
    # a handle of the pipeline and one of hg_secrets_commit_bn254(ctx, ..) in one open batch
    got = hg.verify_public_batch_bn254(ctx, pk, [hg.Instance.from_witness(cases[i]["w"]) for i in (0, 1)], [want[0], want[1]])
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    piped = hg.prove_encryptions_committed_bn254(ctx, pk, encs[:1])[3][0]
    single = hg.Commitment.secrets_bn254(ctx, params, cases[1]["w"])
    opened = hg.claims_open_batch_bn254(ctx, params, [piped, single], cls)
    assert opened == [(piped.open_claims(params, cls[0]), ""), (single.open_claims(params, cls[1]), "")]
    assert [b for b, _ in opened] == [cases[i]["cm"].open_claims(params, cls[i]) for i in (0, 1)]


@pytest.mark.gpu
def test_groups_follow_the_option(ctx):
    """verify_batch_group = 2: a run of 5 lies in three group allocations (2, 2, 1); with item 1 refused its slot, the last of the
    first group, is written again by item 2, and the next group begins at item 3"""
    key = (1024, 1)
    kc, encs, want, tabs = pipeline_case(ctx, key, 5, 0xC0DE)
    params, pk = kc["params"], kc["pk"]
    cases = [host_case(params, tabs[i], 0, (key, "pipe", i)) for i in range(5)]
    bad = tpb.spoiled(encs[1], 1, 0, 17, int(params.e_bound) + 1)
    ctx.set_option("verify_batch_group", 2)
    try:
        cms = check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs), want, cases)
        for i in (0, 2, 4, 1):                                                     # a handle of each group outlives the others of its group
            cms[i].free()
        same_as_host(cms[3], cases[3], full=False)
        proofs, status, _, cms, roots, _, _ = hg.prove_encryptions_committed_bn254(ctx, pk, [encs[0], bad] + encs[2:])
        assert status == [0, 1, 0, 0, 0] and cms[1] is None and roots[1] == ZERO
        for i in (0, 2, 3, 4):
            assert proofs[i] == want[i]
            same_as_host(cms[i], cases[i], full=False)
    finally:
        ctx.set_option("verify_batch_group", 0)
    check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs), want, cases)


@pytest.mark.gpu
def test_neighbours_share_the_context(ctx):
    key = (4096, 2)
    kc, encs, want, tabs = pipeline_case(ctx, key, 4, 0x9E16)
    params, pk, bfv = kc["params"], kc["pk"], kc["bfv"]
    cases = [host_case(params, tabs[i], 0, (key, "nb", i)) for i in range(4)]
    hws = [c["w"] for c in cases]
    roots = [c["cm"].root for c in cases]

    def neighbours():
        batch = hg.Commitment.secrets_batch_bn254(ctx, params, hws)
        gl = hg.prove_encryptions_committed(ctx, pk, encs)
        return {"prove": [ctx.prove_bn254(pk, w)[0] for w in hws], "pipe": hg.prove_encryptions_bn254(ctx, pk, encs, witnesses=False)[0],
                "roots": [cm.root for cm in batch], "open": batch[3].open(cases[3]["claims"], 9), "gl": (gl[0], gl[4])}
    before = neighbours()
    assert before["prove"] == before["pipe"] == want and before["roots"] == roots and before["open"] == cases[3]["short"]
    assert before["gl"][0] == [bfv.prove(ctx, pk, w)[0] for w in hws]
    assert before["gl"][1] == [hg.Commitment.secrets(None, params, w).root for w in hws]
    for rnd in range(3):                                                           # committed run, neighbours, committed run, ...
        check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs), want, cases, full=(rnd == 2))
        assert neighbours() == before, rnd
    # another key on the same context: the pipeline's buffers are rebuilt for it, and again for the first key
    k2, encs2, want2, tabs2 = pipeline_case(ctx, (1024, 1), 5, 0xC0DE)
    cases2 = [host_case(k2["params"], tabs2[i], 0, ((1024, 1), "pipe", i)) for i in range(3)]
    check_run(hg.prove_encryptions_committed_bn254(ctx, k2["pk"], encs2[:3]), want2[:3], cases2)
    check_run(hg.prove_encryptions_committed_bn254(ctx, pk, encs[::-1]), want[::-1], cases[::-1])


@pytest.mark.gpu
def test_end_to_end(ctx):
    """committed pipeline with ws = NULL -> publish proof and root -> hg_verify_public_batch_bn254 on instances built from a and ct0 ->
    hg_claims_open_batch_bn254 on the handles -> hg_claims_verify_batch_bn254 against the roots"""
    key = (1024, 1)
    kc, encs, want, tabs = pipeline_case(ctx, key, 5, 0xC0DE)
    params, pk = kc["params"], kc["pk"]
    encs, tabs = encs[:3], tabs[:3]
    proofs, status, _, cms, roots, ws, _ = hg.prove_encryptions_committed_bn254(ctx, pk, encs)
    assert status == [0] * 3 and len(set(roots)) == 3 and ws == [None] * 3
    insts = []
    for i in range(3):                                                             # what a verifier holds: a and ct0
        a, ct0 = hg.Instance.from_witness(hg.Witness.from_arrays(params, tabs[i])).coeffs()
        assert (a.reshape(params.k, params.n) == encs[i][3]).all()
        insts.append(hg.Instance.from_ciphertext(params, a, ct0))
    got = hg.verify_public_batch_bn254(ctx, pk, insts, proofs)
    assert all(ok for ok, _, _ in got), got
    cls = [cl for _, _, cl in got]
    opened = hg.claims_open_batch_bn254(ctx, params, cms, cls)
    assert all(b is not None and why == "" for b, why in opened)
    openings = [b for b, _ in opened]
    assert hg.claims_verify_batch_bn254(ctx, params, roots, cls, openings) == [(True, "")] * 3
    swapped = [roots[1], roots[0], roots[2]]
    res = hg.claims_verify_batch_bn254(ctx, params, swapped, cls, openings)
    assert res[2] == (True, "") and res[0] == res[1] == (False, "pcs: Merkle path mismatch at query 0"), res


@pytest.mark.gpu
def test_committed_pipeline_is_not_slower_than_prove_then_commit(ctx):
    """(32768, 16), runs of 8 after two warm-up rounds, the two forms alternating in one process, median of 5 each. Leg A: the committed
    pipeline with ws = NULL, its commitments freed. Leg B, the route without it: hg_prove_encryptions_bn254 with host handles, then
    hg_secrets_commit_batch_bn254 on them, all freed. A does none of B's copy-back and upload and commits under the proves, not behind
    them. Asserted: equal proofs and roots, and A is not slower than B.
    Measured on an MI355X (two runs of this test): A 11.54 / 10.80 ms an item, B 14.96 / 12.36 ms, ratio 0.77 / 0.87; the commit's
    device time 4.8 ms an item beside the proves, the proving span 10.2-10.5 ms against 8.4-8.7 (README.md)."""
    n, k, run = 32768, 16, 8
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    encs = [tpb.polys_of_tables(params, hg.Witness.synthetic(params, 0x71AE + 3 * i).arrays()) for i in range(run)]

    def leg_a():
        t0 = time.perf_counter()
        proofs, status, _, cms, roots, _, tm = hg.prove_encryptions_committed_bn254(ctx, pk, encs, cap_each=1 << 21)
        for cm in cms:
            cm.free()
        ms = (time.perf_counter() - t0) * 1e3 / run
        assert status == [0] * run
        return ms, proofs, roots, tm

    def leg_b():
        t0 = time.perf_counter()
        proofs, status, _, ws, tm = hg.prove_encryptions_bn254(ctx, pk, encs, cap_each=1 << 21, witnesses=True)
        cms = hg.Commitment.secrets_batch_bn254(ctx, params, ws)
        roots = [cm.root for cm in cms]
        for cm in cms:
            cm.free()
        del ws[:]
        ms = (time.perf_counter() - t0) * 1e3 / run
        assert status == [0] * run
        return ms, proofs, roots, tm
    for _ in range(2):                                                         # warm-up: table sets, staging, slabs, commit buffers, thread pool
        _, want, want_roots, _ = leg_b()
        _, proofs, roots, _ = leg_a()
        assert proofs == want and roots == want_roots
    ta, tb, commit, prove_a, prove_b = [], [], [], [], []
    for _ in range(5):
        ms, proofs, roots, tm = leg_b()
        assert proofs == want and roots == want_roots
        tb.append(ms); prove_b.append(tm["prove_ms"] / run)
        ms, proofs, roots, tm = leg_a()
        assert proofs == want and roots == want_roots
        ta.append(ms); commit.append(tm["upload_ms"] / run); prove_a.append(tm["prove_ms"] / run)
    ms_a, ms_b = statistics.median(ta), statistics.median(tb)
    print("\nn=%d k=%d run=%d per item: committed pipeline %.3f ms (%s), prove_encryptions_bn254 + secrets_commit_batch_bn254 %.3f ms (%s), ratio %.3f, "
          "commit device time %.3f ms, prove_ms/n %.3f (beside the commit) against %.3f (alone)"
          % (n, k, run, ms_a, " ".join("%.3f" % t for t in ta), ms_b, " ".join("%.3f" % t for t in tb), ms_a / ms_b, statistics.median(commit),
             statistics.median(prove_a), statistics.median(prove_b)))
    assert ms_a <= ms_b, (ms_a, ms_b)
    pk.free()
