#!/usr/bin/env python3
"""Per-proof time of hg_verify_public_bound_batch against its two yardsticks, and the device time of its digest against the existing one.
Two steps, each a child process of its own under its own time limit (the parent never opens the GPU; a step that fails or runs out of
time ends the script):
  legs    mode 3, distinct synthetic witnesses, each proven bound (hg_prove_committed_mode) and unbound (hg_prove_resident_mode). For
          each run length B of --batch, three legs ALTERNATED in one process (a, b, c, a, b, c, ..) after a warm-up call of each:
          (a) hg_verify_public_bound_batch on the B bound proofs, (b) the same triples through hg_verify_public_bound_device one by one,
          (c) hg_verify_public_batch on the unbound mode-3 proofs of the same witnesses - (c) shows what binding costs in a run.
          Medians and ranges of --reps runs, per proof; (a) is never measured against itself.
  digest  through hg_profile: the device time of class instance_digest_group (hg_instance_digest_group) against instance_digest_leaves +
          instance_digest_tree (hg_instance_digest_batch) for the member counts of --members, median of --reps calls after a warm-up of
          each, alternated; for the largest count also with one slice holding every member.
Usage: verify_bound_batch_times.py [n k] [--batch 16,64] [--members 4,64] [--reps 5] [--limit SECONDS]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = 3
DISTINCT = 16


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def fmt(x):
    return "%.3f [%.3f .. %.3f]" % (statistics.median(x), min(x), max(x))


def setup(a):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    hg = entry.load_package()
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    return hg, ctx, bfv


def step_legs(a):
    hg, ctx, bfv = setup(a)
    pk = bfv.setup(ctx)
    batches = [int(b) for b in a.batch.split(",")]
    nw = min(DISTINCT, max(batches))
    ws = [hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n + i) for i in range(nw)]
    insts = [hg.Instance.from_witness(w) for w in ws]
    bound, unbound, cms = [], [], []
    vals = hg.witness_gen(ctx, pk, ws[0])
    for i, w in enumerate(ws):
        if i:
            hg.witness_gen_into(ctx, pk, w, vals)
        out, cm = hg.prove_committed_mode(ctx, pk, vals, hg.ProofBuffer(cap=1 << 25), MODE)
        bound.append(out.bytes())
        cms.append(cm)
        unbound.append(hg.prove_resident_mode(ctx, pk, vals, hg.ProofBuffer(cap=1 << 25), MODE).bytes())
    vals.free()
    roots = [cm.root for cm in cms]
    for cm in cms:
        cm.free()
    print("n=%d k=%d mode %d, %d distinct witnesses, per proof, one process; %d alternating runs of (a) hg_verify_public_bound_batch, (b) "
          "hg_verify_public_bound_device one by one, (c) hg_verify_public_batch on unbound proofs, after a warm-up call of each: median [min .. max] ms"
          % (a.n, a.k, MODE, nw, a.reps))
    for B in batches:
        I, R, Pb, Pu = ([x[i % nw] for i in range(B)] for x in (insts, roots, bound, unbound))

        def leg_a():
            got, _ = hg.verify_public_bound_batch(ctx, pk, I, R, Pb, MODE)
            assert all(ok for ok, _, _ in got), got

        def leg_b():
            for inst, root, p in zip(I, R, Pb):
                ok, why, _ = hg.verify_public_bound(pk, inst, p, root, MODE, ctx=ctx, device=True)
                assert ok, why

        def leg_c():
            got = hg.verify_public_batch(ctx, pk, I, Pu, MODE)
            assert all(ok for ok, _, _ in got), got
        legs = (leg_a, leg_b, leg_c)
        for f in legs:
            f()
        t = [[], [], []]
        for _ in range(a.reps):
            for j, f in enumerate(legs):
                t[j].append(timed(f) / B)
        med = [statistics.median(x) for x in t]
        print("B=%3d: %s; a/b %.2f, range of (a) %s range of (b); a - c %+.3f ms (a/c %.2f)" % (
            B, "; ".join("(%s) %s" % ("abc"[j], fmt(t[j])) for j in range(3)), med[0] / med[1], "below" if max(t[0]) < min(t[1]) else "NOT below",
            med[0] - med[2], med[0] / med[2]))
        sys.stdout.flush()
    os.environ["HG_TIMES"] = "verify"
    Bm = max(batches)
    print("B=%d with HG_TIMES=verify: the bound batch, then the unbound one" % Bm, file=sys.stderr)
    hg.verify_public_bound_batch(ctx, pk, [insts[i % nw] for i in range(Bm)], [roots[i % nw] for i in range(Bm)], [bound[i % nw] for i in range(Bm)], MODE)
    hg.verify_public_batch(ctx, pk, [insts[i % nw] for i in range(Bm)], [unbound[i % nw] for i in range(Bm)], MODE)
    del os.environ["HG_TIMES"]
    pk.free()
    ctx.close()


def step_digest(a):
    hg, ctx, bfv = setup(a)
    counts = [int(m) for m in a.members.split(",")]
    nw = min(DISTINCT, max(counts))
    insts = [hg.Instance.from_witness(hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n + i)) for i in range(nw)]
    ctx.profile(2)

    def device_ms(fn, classes):
        ctx.profile_reset()
        fn()
        st = {s["name"]: s for s in ctx.profile_get(512)}
        return sum(st[c]["total_ms"] for c in classes if c in st), sum(st[c]["launches"] for c in classes if c in st)
    print("n=%d k=%d: device time (hg_profile) of the statement digests of G members, ms a call: median [min .. max] of %d alternating calls after a warm-up of each"
          % (a.n, a.k, a.reps))
    for G in counts:
        I = [insts[i % nw] for i in range(G)]
        want = hg.instance_digest_batch(ctx, I)
        legs = [("instance_digest_group, default slices", 0, lambda: hg.instance_digest_group(ctx, I), ("instance_digest_group",)),
                ("instance_digest_leaves + instance_digest_tree", 0, lambda: hg.instance_digest_batch(ctx, I), ("instance_digest_leaves", "instance_digest_tree"))]
        if G == max(counts):
            legs.append(("instance_digest_group, one slice of %d" % G, G, lambda: hg.instance_digest_group(ctx, I), ("instance_digest_group",)))
        t, launches = [[] for _ in legs], [0] * len(legs)
        for rep in range(a.reps + 1):
            for j, (_, slice_, fn, classes) in enumerate(legs):
                ctx.set_option("bound_batch_slice", slice_)
                assert fn() == want if rep == 0 else True
                ms, launches[j] = device_ms(fn, classes)
                if rep:
                    t[j].append(ms)
        ctx.set_option("bound_batch_slice", 0)
        for j, (name, _, _, _) in enumerate(legs):
            print("G=%3d: %-48s %s ms in %d profiled intervals (%.4f ms a member)" % (G, name, fmt(t[j]), launches[j], statistics.median(t[j]) / G))
        sys.stdout.flush()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=32768)
    ap.add_argument("k", type=int, nargs="?", default=16)
    ap.add_argument("--batch", default="16,64")
    ap.add_argument("--members", default="4,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--step", choices=("legs", "digest"))
    a = ap.parse_args()
    if a.step:
        return {"legs": step_legs, "digest": step_digest}[a.step](a)
    for step in ("legs", "digest"):
        cmd = [sys.executable, os.path.abspath(__file__), str(a.n), str(a.k), "--batch", a.batch, "--members", a.members, "--reps", str(a.reps), "--step", step]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit("step %s ran past its limit of %d s" % (step, a.limit))
        if rc != 0:
            sys.exit("step %s ended with status %d" % (step, rc))


if __name__ == "__main__":
    main()
