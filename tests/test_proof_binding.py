"""Every element of a proof is bound, on every verifier form. The sets of proof_binding_sets.py - each 8-byte word (each 32-byte
element over BN254) in turn replaced by v + 1, truncations, elements that are no residues, trailing bytes - and single changed entries
of the witness tables go through the host verifiers, the independent oracle and every device form, single and batch. The host forms
must reject everything but the trailing bytes; the device forms must decide what the host decides, and a batch must give each member
what the single call gives it, whatever stands beside it in its group.

What this shows and what it does not: a single changed word that also trips a check the walk makes while it reads the proof (a round
polynomial, an unmatched output, a memory hash) is rejected before a deferred ticket is compared. The sweep therefore pins the
DECISION for every element; it exercises the deferred comparisons (verifier.cpp: vanilla_dev, fft_dev, the input claims) only where
nothing inline fails first - the last nodes of the walk, and the changed table entries, whose only failing check is a deferred one.
What no single-word change can reach stays unchecked here as in the verifiers: trailing bytes, and the final evaluations the
reference discards (the collation sum-check's and every grand-product layer's)."""
import os
import time

import pytest

import orclib
import proof_binding_sets as B
from proof_binding_sets import GL, BN
from hglib import hg

MODES = [0, 1, 2, 3]
CALL = 256   # words per batch call: with the honest proof 257 members, four full groups of 64 and a group of one


def where(rows, i, field=GL):
    """names element i for a failure message: its byte offset and, with a proof map, the protocol element (the BN254 stream holds the
    same elements in the same order, 32 bytes for 16)"""
    nb = B.element(field)[0]
    return "element %d (byte %d)%s" % (i, i * nb, ": " + B.label_at(rows, i * 16 if field == BN else i * 8) if rows else "")


def assert_binds(ref, field, rows=None):
    """the contract of a host form: every word, truncation and non-residue rejected with a text of its kind, the trailing bytes ignored"""
    for i, (ok, why) in enumerate(ref["words"]):
        assert not ok and why in B.NINE, (where(rows, i, field), ok, why)
    assert ref["truncations"] == [(False, B.END_OF_STREAM)] * len(ref["truncations"])
    assert ref["noncanonical"] == [(False, B.INVALID_ELEMENT)] * 14
    assert ref["trailing"] == [(True, ""), (True, "")]


# ---- 1. CPU: the host reference itself ---------------------------------------------------------------------------------------------
def test_sets_are_what_they_are_said_to_be():
    proof = B.proof_of(B.case(), GL, 0)
    assert len(proof) == 33936 and B.n_words(proof) == 4242
    assert sum(a != b for a, b in zip(B.word(proof, 7), proof)) >= 1 and B.word(proof, 7)[:56] == proof[:56] and B.word(proof, 7)[64:] == proof[64:]
    wrap = B.with_element(proof, 5, B.P - 1)
    assert B.word(wrap, 5)[40:48] == bytes(8)                                   # (p - 1) + 1 wraps to zero
    lens = B.truncation_lengths(proof)
    assert len(lens) == 271 and {0, 1, 7, 9, 128, len(proof) - 8, len(proof) - 1} <= set(lens) and max(lens) < len(proof)
    assert B.noncanonical_at(proof) == [0, 1, 2, 3, 2121, 4240, 4241] and len(B.noncanonical(proof)) == 14
    assert B.noncanonical(proof)[0][:8] == B.P.to_bytes(8, "big") and B.noncanonical(proof)[-1][-8:] == b"\xff" * 8
    assert [len(p) - len(proof) for p in B.trailing(proof)] == [1, 8]
    assert B.entries(2048) == [0, 1, 255, 256, 511, 512, 1023, 1024, 2047] and B.entries(1024) == [0, 1, 255, 256, 511, 512, 1023]
    pb = B.proof_of(B.case(), BN, 0)
    assert B.n_words(pb, BN) == 2121 and len(B.word(pb, 3, BN)) == len(pb) and B.noncanonical(pb, BN)[1][:32] == b"\xff" * 32


@pytest.mark.parametrize("mode", MODES)
def test_host_verifier_binds_every_element(mode):
    """hg_verify / hg_verify_mode on the oracle's proof of the (1024, 1, 27) fixture: 4242 words, 271 truncations, 14 non-residues
    rejected, the two trailing variants accepted; in mode 0 every one of the nine checks is the first to fail for some word"""
    ref = B.reference(GL, mode)
    assert len(ref["words"]) == 4242
    assert_binds(ref, GL)
    if mode == 0:
        assert {why for _, why in ref["words"]} == set(B.NINE)


@pytest.mark.parametrize("mode", MODES)
def test_public_host_form_answers_as_the_host_verifier(mode):
    """hg_verify_public: the same (ok, reason) on every member of every set"""
    c, ref = B.case(), B.reference(GL, mode)
    proof = B.proof_of(c, GL, mode)
    for name in B.SETS:
        for i, p in enumerate(B.members(name, proof)):
            assert B.host_public(c, GL, mode, p) == ref[name][i], (mode, name, i)


@pytest.mark.parametrize("mode", MODES)
def test_oracle_decides_as_the_host_verifier(mode):
    """the independent verifier (oracle/) on S(mode): every word whose host reason is not the round check's, plus every 16th word.
    Decisions only: the oracle words the round check differently."""
    c, ref = B.case(), B.reference(GL, mode)
    proof = B.proof_of(c, GL, mode)
    S = B.subset(ref["words"])
    assert 450 <= len(S) <= 600
    for i in S:
        ok, _ = orclib.verify_f(GL, c["orc_params"], c["orc_inputs"], B.word(proof, i), threads=8, mode=mode)
        assert ok == ref["words"][i][0], (mode, i)
    for p, want in zip(B.trailing(proof) + B.truncations(proof)[::16], ref["trailing"] + ref["truncations"][::16]):
        assert orclib.verify_f(GL, c["orc_params"], c["orc_inputs"], p, threads=8, mode=mode)[0] == want[0], (mode, len(p))


def test_bn254_host_verifier_binds_every_element():
    """hg_verify_bn254: 2121 elements; element e fails the check that the Goldilocks mode-0 proof fails for the c0 word of its element e"""
    ref = B.reference(BN, 0)
    assert len(ref["words"]) == 2121
    assert_binds(ref, BN)
    gl = B.reference(GL, 0)["words"]
    for e, got in enumerate(ref["words"]):
        assert got == gl[2 * e], (e, got, gl[2 * e])


def test_bn254_public_host_form_answers_as_the_host_verifier_on_every_element():
    c, ref = B.case(), B.reference(BN, 0)
    for e, p in enumerate(B.words(B.proof_of(c, BN, 0), BN)):
        assert B.host_public(c, BN, 0, p) == ref["words"][e], e


def test_bn254_public_host_form_answers_as_the_host_verifier_on_the_other_sets():
    c, ref = B.case(), B.reference(BN, 0)
    proof = B.proof_of(c, BN, 0)
    for name in B.SETS[1:]:
        for i, p in enumerate(B.members(name, proof, BN)):
            assert B.host_public(c, BN, 0, p) == ref[name][i], (name, i)


_VARIANTS = []


def witness_variants():
    """[(table, index, the text a verifier owes it, witness handle)]: one entry of one of the seven tables + 1 mod p (made once)"""
    if not _VARIANTS:
        c = B.case()
        for t, name in enumerate(B.TABLES):
            for j in B.entries(c["d"][name].size):
                d = {f: v.copy() for f, v in c["d"].items()}
                d[name][j] = (int(d[name][j]) + 1) % B.P
                # ct0is is the output claim: it enters the first round of the output node
                _VARIANTS.append((name, j, B.ROUND if name == "ct0is" else B.INPUT_CLAIM % t, hg.Witness.from_arrays(c["bfv"].params, d)))
    return _VARIANTS


def test_host_verifier_names_the_table_of_a_single_changed_entry():
    """the honest mode-3 proof against a witness with one changed entry, at the first, second and last index and either side of
    every power of two from 256 up"""
    c = B.case()
    var = witness_variants()
    assert len(var) == sum(len(B.entries(c["d"][t].size)) for t in B.TABLES) >= 7 * 7
    p3, pb = B.proof_of(c, GL, 3), B.proof_of(c, BN, 0)
    for name, j, want, w2 in var:
        assert hg.verify(c["pk"], w2, p3, mode=3) == (False, want), (name, j)
        assert hg.verify_bn254(c["pk"], w2, pb) == (False, want), (name, j)


_INSTANCES = []


def instance_variants():
    """[(table, index, instance)]: one coefficient of a or of ct0 + 1"""
    if not _INSTANCES:
        c = B.case()
        a, ct0 = c["inst"].coeffs()
        for tab in (0, 1):
            for j in B.entries(a.size):
                arrs = [a.copy(), ct0.copy()]
                arrs[tab][j] += 1
                _INSTANCES.append((("a", "ct0")[tab], j, hg.Instance.from_ciphertext(c["bfv"].params, *arrs)))
    return _INSTANCES


def test_public_host_form_names_the_table_of_a_single_changed_coefficient():
    c = B.case()
    for name, j, inst in instance_variants():
        want = (False, B.INPUT_CLAIM % 3 if name == "a" else B.ROUND)
        for mode in (0, 3):
            assert hg.verify_public(c["pk"], inst, B.proof_of(c, GL, mode), mode)[:2] == want, (name, j, mode)
        assert hg.verify_public_bn254(c["pk"], inst, B.proof_of(c, BN, 0))[:2] == want, (name, j)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    """a context; per shape (see shape) a device key of the case and the proof map of its mode-0 proof"""
    ctx = hg.Context(0)
    d = dict(ctx=ctx, forms={}, shapes={})
    yield d
    for s in d["shapes"].values():
        s["pk"].free()
    ctx.close()


def shape(dev, tmp_path_factory, n=B.FIXTURE[0], k=B.FIXTURE[1], bits=B.FIXTURE[2]):
    if (n, k) not in dev["shapes"]:
        c = B.case(n, k, bits)
        pk = c["bfv"].setup(dev["ctx"])
        mp = str(tmp_path_factory.mktemp("map") / "map.tsv")
        os.environ["HG_PROOF_MAP"] = mp
        try:
            p0, _ = c["bfv"].prove(dev["ctx"], pk, c["w"])
        finally:
            del os.environ["HG_PROOF_MAP"]
        assert p0 == B.proof_of(c, GL, 0)
        rows = B.read_map(mp)
        assert rows[0][0] == 0 and rows[-1] == (len(p0), "end of proof")
        dev["shapes"][(n, k)] = dict(c=c, pk=pk, rows=rows)
    return dev["shapes"][(n, k)]


class Form:
    """one verifier form in one mode on one shape: batch(proofs) and single(proof) -> (ok, reason), the honest proof, and the host
    form that is its reference. host_reason: include/hg.h promises the host's reason too (the public forms); the forms that take a
    witness promise the decision."""

    def __init__(self, name, field, mode, proof, batch, single, host, host_reason, rows):
        self.name, self.field, self.mode, self.proof, self.batch, self.single, self.host, self.host_reason, self.rows = \
            name, field, mode, proof, batch, single, host, host_reason, rows
        self.singles = {}

    def single_word(self, i):
        if i not in self.singles:
            self.singles[i] = self.single(B.word(self.proof, i, self.field))
        return self.singles[i]


FORMS = ["device", "public", "bound", "device_bn254", "public_bn254"]
BATCH_CASES = [("device", m) for m in MODES] + [("public", m) for m in MODES] + [("bound", 1), ("bound", 3), ("device_bn254", 0), ("public_bn254", 0)]


def form(dev, tmp_path_factory, name, mode, n=B.FIXTURE[0], k=B.FIXTURE[1], bits=B.FIXTURE[2]):
    key = (name, mode, n, k)
    if key in dev["forms"]:
        return dev["forms"][key]
    s = shape(dev, tmp_path_factory, n, k, bits)
    ctx, pk, c, rows = dev["ctx"], s["pk"], s["c"], s["rows"]
    w, inst, bfv = c["w"], c["inst"], c["bfv"]
    field = BN if name.endswith("bn254") else GL
    if name == "bound":   # a bound proof needs the device prover; its reference is the host form of the same entry
        vals = hg.witness_gen(ctx, pk, w)
        out, cm = hg.prove_committed_mode(ctx, pk, vals, hg.ProofBuffer(), mode)
        vals.free()
        proof, root = out.bytes(), cm.root
        cm.free()
        assert len(proof) == len(B.proof_of(c, GL, mode))
    else:   # the device prover returns the oracle's bytes
        proof = ctx.prove_bn254(pk, w)[0] if field == BN else bfv.prove(ctx, pk, w, mode=mode)[0]
        assert proof == B.proof_of(c, field, mode), (name, mode)
    if name == "device":
        f = Form(name, field, mode, proof, lambda ps: hg.verify_device_batch(ctx, pk, [w] * len(ps), ps, mode=mode),
                 lambda p: hg.verify_device(ctx, pk, w, p, mode=mode), lambda p: hg.verify(c["pk"], w, p, mode=mode), False, rows)
    elif name == "public":
        f = Form(name, field, mode, proof, lambda ps: [r[:2] for r in hg.verify_public_batch(ctx, pk, [inst] * len(ps), ps, mode)],
                 lambda p: hg.verify_public(pk, inst, p, mode, ctx=ctx, device=True)[:2], lambda p: hg.verify(c["pk"], w, p, mode=mode), True, rows)
    elif name == "bound":
        f = Form(name, field, mode, proof, lambda ps: [r[:2] for r in hg.verify_public_bound_batch(ctx, pk, [inst] * len(ps), [root] * len(ps), ps, mode)[0]],
                 lambda p: hg.verify_public_bound(pk, inst, p, root, mode, ctx=ctx, device=True)[:2],
                 lambda p: hg.verify_public_bound(c["pk"], inst, p, root, mode)[:2], True, rows)
    elif name == "device_bn254":
        f = Form(name, field, mode, proof, lambda ps: hg.verify_device_batch_bn254(ctx, pk, [w] * len(ps), ps),
                 lambda p: hg.verify_device_bn254(ctx, pk, w, p), lambda p: hg.verify_bn254(c["pk"], w, p), False, rows)
    else:
        f = Form(name, field, mode, proof, lambda ps: [r[:2] for r in hg.verify_public_batch_bn254(ctx, pk, [inst] * len(ps), ps)],
                 lambda p: hg.verify_public_bn254(pk, inst, p, ctx=ctx, device=True)[:2], lambda p: hg.verify_bn254(c["pk"], w, p), True, rows)
    dev["forms"][key] = f
    return f


def reference_of(f):
    """the host answers for the form's proof, shared: the unbound forms of one (field, mode) have the same proof and the same
    reference (hg_verify_public answers as hg_verify_mode: the CPU tests above)"""
    key = ("bound", f.mode) if f.name == "bound" else (f.field, f.mode)
    return B.reference(f.field, f.mode, verify=f.host, key=key, proof=f.proof)


def call_with_honest(f, ci, idx):
    """one batch call: the words `idx` with the honest proof at a position that moves with the call index (the first call puts it
    last in the first group). Returns (position of the honest proof, results of the words in order)."""
    ps = [B.word(f.proof, i, f.field) for i in idx]
    pos = (63 + 65 * ci) % (len(ps) + 1)
    ps.insert(pos, f.proof)
    got = f.batch(ps)
    assert len(got) == len(ps)
    assert got[pos] == (True, ""), (f.name, f.mode, "the honest proof at position %d of call %d" % (pos, ci), got[pos])
    return pos, got[:pos] + got[pos + 1:]


def check_members(f, idx, got, ref_words):
    for i, g in zip(idx, got):
        want = ref_words[i]
        assert not g[0] and g[0] == want[0], (f.name, f.mode, where(f.rows, i, f.field), g, want)
        if f.host_reason:
            assert g == want, (f.name, f.mode, where(f.rows, i, f.field), g, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", BATCH_CASES)
def test_batch_form_binds_every_element(dev, tmp_path_factory, name, mode):
    """2. the whole word set in calls of 256 plus the honest proof, the last call ragged; every word rejected as the host rejects it,
    with the single call's reason on S(mode) (and the host's everywhere, where the header promises it); one call of mixed lengths;
    one call in groups of 3"""
    t0 = time.perf_counter()
    f = form(dev, tmp_path_factory, name, mode)
    ref = reference_of(f)
    for name_ in B.SETS:   # (a set is swept when it is first asked for)
        ref[name_]
    t_ref = time.perf_counter() - t0
    if name == "bound":   # (the unbound host forms: the CPU tests) a perturbed word the host form accepts is a finding of its own
        assert_binds(ref, f.field, f.rows)
    nw = B.n_words(f.proof, f.field)
    assert nw == len(ref["words"])
    by_word = [None] * nw
    calls = [list(range(a, min(a + CALL, nw))) for a in range(0, nw, CALL)]
    for ci, idx in enumerate(calls):
        _, got = call_with_honest(f, ci, idx)
        check_members(f, idx, got, ref["words"])
        for i, g in zip(idx, got):
            by_word[i] = g
    t_batch = time.perf_counter() - t0 - t_ref
    # "exactly the decision of the single call" and its reason
    S = B.subset(ref["words"])
    for i in S:
        assert by_word[i] == f.single_word(i), (name, mode, where(f.rows, i, f.field), by_word[i], f.single_word(i))
    t_single = time.perf_counter() - t0 - t_ref - t_batch
    # members of different lengths in one group: every truncation, non-residue and trailing variant, an honest proof after every 16th
    mixed, want = [], []
    for k, (p, r) in enumerate((p, r) for s in B.SETS[1:] for p, r in zip(B.members(s, f.proof, f.field), ref[s])):
        mixed.append(p), want.append(r)
        if k % 16 == 15:
            mixed.append(f.proof), want.append((True, ""))
    assert f.batch(mixed) == want
    # the group size does not matter (the ragged call again, in groups of 3)
    if mode in (0, 3):
        ctx = dev["ctx"]
        try:
            ctx.set_option("verify_batch_group", 3)
            _, got3 = call_with_honest(f, len(calls) - 1, calls[-1])
        finally:
            ctx.set_option("verify_batch_group", 0)
        assert got3 == [by_word[i] for i in calls[-1]]
    print("%s mode %d: host reference %.1f s, %d batch calls %.1f s, %d single calls %.1f s, all %.1f s"
          % (name, mode, t_ref, len(calls), t_batch, len(S), t_single, time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", BATCH_CASES)
def test_single_call_form_decides_as_the_host(dev, tmp_path_factory, name, mode):
    """3. hg_verify_device(_mode), hg_verify_public_device, hg_verify_public_bound_device and the two BN254 forms on S(mode). The
    decision is the host's. The reason is the host's where the header promises it; hg_verify_device(_mode) promises the decision, and
    its walk defers the table-sized checks, so its reason may differ in one way only: the host names a deferred check (a final
    evaluation, an input claim) and the device an inline one that the same word trips later in the stream. (A walk that rejects
    while it reads keeps the checks of the Vanilla nodes it had reached pending - verifier.cpp, walk_with_backend - so the count
    printed here is 0 today; before that the public forms answered 20 to 34 words of a mode with the later round check's text.)"""
    f = form(dev, tmp_path_factory, name, mode)
    ref = reference_of(f)
    differing = 0
    for i in B.subset(ref["words"]):
        got, want = f.single_word(i), ref["words"][i]
        assert got[0] == want[0] and not got[0], (name, mode, where(f.rows, i, f.field), got, want)
        if got != want:
            differing += 1
            assert not f.host_reason and B.deferred_text(want[1]) and B.inline_text(got[1]), (name, mode, where(f.rows, i, f.field), got, want)
    for s in B.SETS[1:]:
        step = 16 if s == "truncations" else 1
        for p, want in zip(list(B.members(s, f.proof, f.field))[::step], ref[s][::step]):
            assert f.single(p) == want, (name, mode, s, len(p))
    print("%s mode %d: the single call's reason differs from the host's on %d words of S" % (name, mode, differing))


# ---- 4. single entries -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
def test_device_forms_name_the_table_of_a_single_changed_entry(dev, tmp_path_factory, mode):
    """one entry of one table changed: the only failing check is a deferred one. hg_verify_device(_mode) and one hg_verify_device_batch
    call - every variant a member of its own, an honest pair before each, so that variants stand last in their groups - give the
    host's text with the right input index."""
    f = form(dev, tmp_path_factory, "device", mode)
    s = shape(dev, tmp_path_factory)
    ctx, pk, w = dev["ctx"], s["pk"], s["c"]["w"]
    var = witness_variants()
    for name, j, want, w2 in var:
        assert hg.verify_device(ctx, pk, w2, f.proof, mode=mode) == (False, want), (name, j)
    ws = [x for v in var for x in (w, v[3])]
    got = hg.verify_device_batch(ctx, pk, ws, [f.proof] * len(ws), mode=mode)
    assert got == [x for v in var for x in ((True, ""), (False, v[2]))]
    assert len(got) > 64 and not got[63][0] and not got[-1][0]   # (the last members of the first and of the last group)


@pytest.mark.gpu
def test_bn254_batch_form_names_the_table_of_a_single_changed_entry(dev, tmp_path_factory):
    f = form(dev, tmp_path_factory, "device_bn254", 0)
    s = shape(dev, tmp_path_factory)
    ctx, pk, w = dev["ctx"], s["pk"], s["c"]["w"]
    var = witness_variants()
    ws = [x for v in var for x in (w, v[3])]
    got = hg.verify_device_batch_bn254(ctx, pk, ws, [f.proof] * len(ws))
    assert got == [x for v in var for x in ((True, ""), (False, v[2]))]
    for name, j, want, w2 in [v for v in var if v[1] == 0 or v[1] == s["c"]["d"][v[0]].size - 1]:   # (the single call at the first and last index of each table)
        assert hg.verify_device_bn254(ctx, pk, w2, f.proof) == (False, want), (name, j)


@pytest.mark.gpu
def test_public_device_forms_name_the_table_of_a_single_changed_coefficient(dev, tmp_path_factory):
    """a[j] + 1 and ct0[j] + 1: the batch forms and the device single calls answer as the host form does on the same instance"""
    s = shape(dev, tmp_path_factory)
    ctx, pk, c = dev["ctx"], s["pk"], s["c"]
    var = instance_variants()
    insts = [x for v in var for x in (c["inst"], v[2])]
    for mode in (0, 3):
        proof = form(dev, tmp_path_factory, "public", mode).proof
        want = [hg.verify_public(c["pk"], i, proof, mode)[:2] for i in insts]
        assert want == [x for v in var for x in ((True, ""), (False, B.INPUT_CLAIM % 3 if v[0] == "a" else B.ROUND))]
        assert [r[:2] for r in hg.verify_public_batch(ctx, pk, insts, [proof] * len(insts), mode)] == want, mode
        assert [hg.verify_public(pk, i, proof, mode, ctx=ctx, device=True)[:2] for i in insts] == want, mode
    pb = form(dev, tmp_path_factory, "public_bn254", 0).proof
    want = [hg.verify_public_bn254(c["pk"], i, pb)[:2] for i in insts]
    assert [ok for ok, _ in want] == [True, False] * len(var)
    assert [r[:2] for r in hg.verify_public_batch_bn254(ctx, pk, insts, [pb] * len(insts))] == want
    assert [hg.verify_public_bn254(pk, i, pb, ctx=ctx, device=True)[:2] for i in insts] == want


# ---- 5. the smallest shape with two moduli and two r2is chunks ---------------------------------------------------------------------
SECOND = (4096, 2, 55)
_SECOND_REF = {}


PARTS = 3   # the host takes 4 ms a word at this shape: a case sweeps a third of the words


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("name,mode", [("device", 0), ("device", 3), ("public", 0), ("public", 3), ("bound", 3)])
def test_batch_form_binds_the_elements_of_the_second_shape(dev, tmp_path_factory, name, mode, part):
    """5. (4096, 2, 55), batch forms. The words come from the proof map: every word that is not a sum-check's round polynomial (root
    products, v_l / v_r evaluations, the claimed sum, the openings, the input evaluations) and every 16th of the rest; a case takes
    one of PARTS consecutive ranges of them. The host answers are computed once per (host form, mode, part)."""
    t0 = time.perf_counter()
    f = form(dev, tmp_path_factory, name, mode, *SECOND)
    every = B.map_subset(f.rows, f.proof)
    labels = {B.label_at(f.rows, 8 * i) for i in every}
    for kind in ("root products", "v_l, v_r", "claimed sum", "openings", "input evaluation", "evaluation at r_x", "evaluation at r_y"):
        assert any(kind in l for l in labels), kind
    assert all(i in every for i in range(0, B.n_words(f.proof), 16))
    which = every[part * len(every) // PARTS:(part + 1) * len(every) // PARTS]
    key = ("bound" if name == "bound" else GL, mode, part)
    if key not in _SECOND_REF:
        _SECOND_REF[key] = {i: f.host(B.word(f.proof, i)) for i in which}
    ref = _SECOND_REF[key]
    t_ref = time.perf_counter() - t0
    for i in which:
        assert not ref[i][0] and ref[i][1] in B.NINE, (name, mode, where(f.rows, i), ref[i])
    calls = [which[a:a + CALL] for a in range(0, len(which), CALL)]
    for ci, idx in enumerate(calls):
        _, got = call_with_honest(f, ci, idx)
        check_members(f, idx, got, ref)
    print("%s mode %d at (4096, 2), part %d: %d of %d words, host reference %.1f s, %d batch calls %.1f s"
          % (name, mode, part, len(which), len(every), t_ref, len(calls), time.perf_counter() - t0 - t_ref))
