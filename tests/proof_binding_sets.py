"""What tests/test_proof_binding.py shares between its CPU and GPU tests: the perturbation sets of a proof and of a witness table, the
(1024, 1, 27) case with the oracle's proofs, and the host verifiers' answers to every member of every set - computed once per
(field, mode), kept here, never changed, and used by the GPU tests as their reference."""
import bisect
import os

import orclib
from hglib import hg

P, R_BN = orclib.P, orclib.R_BN
GL, BN = "goldilocks", "bn254"
FIXTURE = (1024, 1, 27)
TABLES = ["s", "e", "k1", "ais", "r1is", "r2is", "ct0is"]   # the seven witness tables, in the order of the input indices at k = 1

ROUND = "InvalidSumCheck: round polynomial does not match the running claim"
UNMATCHED = "InvalidSumCheck: unmatched sum check output"
HASHES = ["memory check: %s hash mismatch" % h for h in ("read", "write", "init", "final")]
FINALS = ["vanilla node: final evaluation mismatch", "vanilla node: phase-2 final evaluation mismatch", "fft node: final evaluation mismatch"]
NINE = [ROUND, UNMATCHED] + HASHES + FINALS
END_OF_STREAM, INVALID_ELEMENT = "proof: unexpected end of stream", "proof: invalid field element"
INPUT_CLAIM = "input claim mismatch at input %d"


def deferred_text(why):
    """a check the device walk defers to a ticket (verifier.cpp: vanilla_dev, fft_dev, the input claims)"""
    return why in FINALS or why.startswith("input claim mismatch at input ")


def inline_text(why):
    """a check the device walk makes while it reads the proof"""
    return why in (ROUND, UNMATCHED) or why in HASHES or why.startswith("proof: ")


# ---- perturbation sets ------------------------------------------------------------------------------------------------------------
def element(field):
    """(bytes, modulus) of what a proof stream is made of: a big-endian u64 word, or a 32-byte Fr element"""
    return (32, R_BN) if field == BN else (8, P)


def with_element(proof, i, value, field=GL):
    nb, _ = element(field)
    return proof[:i * nb] + value.to_bytes(nb, "big") + proof[(i + 1) * nb:]


def word(proof, i, field=GL):
    """element i replaced by (v + 1) mod the field's modulus"""
    nb, mod = element(field)
    return with_element(proof, i, (int.from_bytes(proof[i * nb:(i + 1) * nb], "big") + 1) % mod, field)


def n_words(proof, field=GL):
    return len(proof) // element(field)[0]


def words(proof, field=GL, which=None):
    """every element in turn (or the indices of `which`): a generator, a whole set is 4242 proofs"""
    return (word(proof, i, field) for i in (range(n_words(proof, field)) if which is None else which))


def truncation_lengths(proof):
    L = len(proof)
    return sorted({0, 1, 7, 9, L - 8, L - 1} | set(range(0, L, 128)))


def truncations(proof):
    return [proof[:n] for n in truncation_lengths(proof)]


def noncanonical_at(proof, field=GL):
    last = n_words(proof, field) - 1
    return [0, 1, 2, 3, (last + 1) // 2, last - 1, last]


def noncanonical(proof, field=GL):
    nb, mod = element(field)
    return [with_element(proof, i, v, field) for i in noncanonical_at(proof, field) for v in (mod, (1 << (8 * nb)) - 1)]


def trailing(proof):
    """the only two variants a verifier must accept (include/hg.h: trailing bytes are ignored)"""
    return [proof + b"\0", proof + bytes(8)]


def entries(size):
    """flat indices either side of a workgroup's and a tile's edge"""
    at = {0, 1, size - 1}
    j = 256
    while j < size:
        at |= {j - 1, j}
        j *= 2
    return sorted(at)


SETS = ("words", "truncations", "noncanonical", "trailing")


def members(name, proof, field=GL):
    return {"words": lambda: words(proof, field), "truncations": lambda: truncations(proof), "noncanonical": lambda: noncanonical(proof, field),
            "trailing": lambda: trailing(proof)}[name]()


# ---- the case and the host reference ----------------------------------------------------------------------------------------------
_CASES = {}
_REF = {}


def case(n=FIXTURE[0], k=FIXTURE[1], bits=FIXTURE[2]):
    """per shape: a host-only key, the fixture witness with its tables and its instance; proofs are added by proof_of"""
    if (n, k) not in _CASES:
        bfv = hg.BfvEncrypt.new(n, k)
        w = bfv.get_inputs(os.path.join(orclib.GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json"))
        d = w.arrays()
        _CASES[(n, k)] = dict(n=n, k=k, bfv=bfv, pk=bfv.setup(None), w=w, d=d, inst=hg.Instance.from_witness(w), orc_params=orclib.params(n, k),
                              orc_inputs=orclib.Inputs(d), proofs={})
    return _CASES[(n, k)]


def proof_of(c, field, mode):
    """the oracle's proof of the case's witness (orclib.prove_f)"""
    if (field, mode) not in c["proofs"]:
        c["proofs"][(field, mode)] = orclib.prove_f(field, c["orc_params"], c["orc_inputs"], threads=8, mode=mode)[0]
    return c["proofs"][(field, mode)]


def host_verify(c, field, mode, proof):
    return hg.verify_bn254(c["pk"], c["w"], proof) if field == BN else hg.verify(c["pk"], c["w"], proof, mode=mode)


def host_public(c, field, mode, proof):
    got = hg.verify_public_bn254(c["pk"], c["inst"], proof) if field == BN else hg.verify_public(c["pk"], c["inst"], proof, mode)
    return got[:2]


class _Answers(dict):
    """{set name: [(ok, reason)]}: a set is swept when it is first asked for, and kept"""

    def __init__(self, verify, proof, field):
        super().__init__()
        self.verify, self.proof, self.field = verify, proof, field

    def __missing__(self, name):
        self[name] = [self.verify(p) for p in members(name, self.proof, self.field)]
        return self[name]


def reference(field, mode, verify=None, key=None, proof=None):
    """{set name: [(ok, reason)]} of the host verifier on every member of a set, computed once per key and set. The default is hg_verify /
    hg_verify_mode / hg_verify_bn254 on the (1024, 1, 27) case; another host form (a bound proof's) passes its own verify(proof),
    proof and key."""
    key = key or (field, mode)
    if key not in _REF:
        c = case()
        _REF[key] = _Answers(verify or (lambda p: host_verify(c, field, mode, p)), proof or proof_of(c, field, mode), field)
    return _REF[key]


def subset(ref_words):
    """S: every word whose host reason is not the round-polynomial text, plus every 16th word"""
    return [i for i, (_, why) in enumerate(ref_words) if why != ROUND or i % 16 == 0]


# ---- the proof map: which protocol element a byte belongs to ---------------------------------------------------------------------
def read_map(path):
    """[(byte offset, label)] of a map written by a prove under HG_PROOF_MAP"""
    rows = [l.rstrip("\n").split("\t", 1) for l in open(path)]
    return [(int(o), label) for o, label in rows]


def label_at(rows, byte):
    """the label of the last entry at or before `byte` (several entries may share an offset: the last one names the bytes)"""
    return rows[bisect.bisect_right([o for o, _ in rows], byte) - 1][1]


def map_subset(rows, proof):
    """word indices: every word under a label that is not a sum-check's rounds, plus every 16th word"""
    return [i for i in range(len(proof) // 8) if "sum-check" not in label_at(rows, 8 * i) or i % 16 == 0]
