"""What a group of the batch verifiers shares (csrc/verifier_merge.hpp: merge_group). The other batch tests compare decisions; these
pin the merge itself: on the host, through hand-made records (verify_merge_check.cpp), and on the device, through the census line
every group prints under HG_TIMES=verify - one proof against three proofs in one group, for every batch entry over both fields."""
import os
import re
import subprocess
import sys

import pytest

from hglib import ROOT

CENSUS = re.compile(r"\[hg\] (verify_batch\w*): group (\d+) \((\d+) proofs\): (\d+) eq tables, (\d+) constant sums, (\d+) \+ (\d+) gathers, (\d+) DFT rows, "
                    r"(\d+) dots, (\d+) input evaluations in (\d+) units \([0-9.]+ MB\); (\d+) slots")
FIELDS = ("eqs", "consts", "gathers1", "gathers2", "dft", "dots", "inputs", "units", "slots")


def test_merge_of_hand_made_records_on_the_host(tmp_path):
    """csrc/verifier_merge.hpp on the host: records made through RecBackendT's own calls, merged with one chain for all and with own
    chains, a rejected proof at every position, the slot numbers and every proof's gslot."""
    exe = str(tmp_path / "verify_merge_check")
    src = os.path.join(ROOT, "tests", "verify_merge_check.cpp")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-x", "hip", "--cuda-host-only", src, "-o", exe,
                           "-I", os.path.join(ROOT, "hyper-greco_amd", "csrc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


# n=1024 k=1, three synthetic witnesses and their proofs as tests/test_device_verifier_batch.py makes them; every entry once on one
# proof and once on three (one group: the default group size is far above three). A line "CALL <name> <proofs>" ahead of each call.
CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import __graft_entry__ as entry
hg = entry.load_package()
field = %(field)r
ctx = hg.Context(0)
bfv = hg.BfvEncrypt.new(1024, 1)
pk = bfv.setup(ctx)
ws = [hg.Witness.synthetic(bfv.params, 0x5a0 + i) for i in range(3)]
insts = [hg.Instance.from_witness(w) for w in ws]
def call(name, fn, *lists):
    for m in (1, 3):
        print("CALL %%s %%d" %% (name, m), file=sys.stderr, flush=True)
        got = fn(*[l[:m] for l in lists])
        assert len(got) == m and all(g[0] for g in got), (name, m, [g[:2] for g in got])
if field == "bn254":
    ps = [ctx.prove_bn254(pk, w)[0] for w in ws]
    call("device0", lambda w, p: hg.verify_device_batch_bn254(ctx, pk, w, p), ws, ps)
    call("public0", lambda i, p: hg.verify_public_batch_bn254(ctx, pk, i, p), insts, ps)
else:
    for mode in (0, 3):
        ps = [bfv.prove(ctx, pk, w, mode=mode)[0] for w in ws]
        call("device%%d" %% mode, lambda w, p: hg.verify_device_batch(ctx, pk, w, p, mode=mode), ws, ps)
        call("public%%d" %% mode, lambda i, p: hg.verify_public_batch(ctx, pk, i, p, mode=mode), insts, ps)
    ps, roots = [], []
    for w in ws:
        vals = hg.witness_gen(ctx, pk, w)
        out, cm = hg.prove_committed_mode(ctx, pk, vals, hg.ProofBuffer(), 3)
        ps.append(out.bytes()); roots.append(cm.root)
        vals.free()
    call("bound3", lambda i, r, p: hg.verify_public_bound_batch(ctx, pk, i, r, p, 3)[0], insts, roots, ps)
print("RAN")
"""


def census(field):
    """{(entry, proofs): the counts of its one group} and the label the lines carry"""
    code = CHILD % dict(root=ROOT, field=field)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, HG_TIMES="verify"), cwd=ROOT)
    assert r.returncode == 0 and "RAN" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    out, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("CALL "):
            cur = (line.split()[1], int(line.split()[2]))
            continue
        m = CENSUS.match(line)
        if m:
            assert cur is not None and cur not in out, line            # one group per call
            assert m.group(1) == ("verify_batch_bn254" if field == "bn254" else "verify_batch"), line
            assert int(m.group(2)) == 0 and int(m.group(3)) == cur[1], line
            out[cur] = dict(zip(FIELDS, (int(x) for x in m.groups()[3:])))
    return out


def shared_in_mode_0(one, three):
    """every proof reads the one fixed chain at the same offsets: what depends on the key only is built once, what reads a proof's
    own evaluations or its own inputs once per proof"""
    for f in ("eqs", "consts", "gathers1", "dft", "units"):
        assert three[f] == one[f], (f, one, three)
    for f in ("gathers2", "inputs"):
        assert three[f] == 3 * one[f] and one[f] > 0, (f, one, three)
    assert three["dots"] == one["dots"] + 2 * one["gathers2"], (one, three)       # a phase-2 gather's dot is its own, the others are shared
    assert three["slots"] == one["slots"] + 2 * (one["gathers2"] + one["inputs"]), (one, three)


def nothing_shared(one, three):
    """own chains: three proofs are three times one proof"""
    assert one["eqs"] > 0 and one["gathers2"] > 0 and one["inputs"] > 0, one
    for f in FIELDS:
        assert three[f] == 3 * one[f], (f, one, three)


@pytest.mark.gpu
def test_goldilocks_groups_share_what_the_merge_says():
    c = census("goldilocks")
    assert sorted(c) == sorted((e, m) for e in ("device0", "public0", "device3", "public3", "bound3") for m in (1, 3)), sorted(c)
    for e in ("device0", "public0"):
        shared_in_mode_0(c[(e, 1)], c[(e, 3)])
    for e in ("device3", "public3", "bound3"):
        nothing_shared(c[(e, 1)], c[(e, 3)])


@pytest.mark.gpu
def test_bn254_groups_share_what_the_merge_says():
    c = census("bn254")
    assert sorted(c) == sorted((e, m) for e in ("device0", "public0") for m in (1, 3)), sorted(c)
    for e in ("device0", "public0"):
        shared_in_mode_0(c[(e, 1)], c[(e, 3)])
