#!/usr/bin/env python3
"""What binding a proof to its statement costs, bound against unbound, legs alternated in one process:

  prover    A  hg_prove_committed_mode: commitment, statement digest and the seeded round-by-round prove in one call
            B  hg_secrets_commit_values followed by hg_prove_resident_mode: the same artefacts, the proof unbound
  verifier  A  hg_verify_public_bound_device
            B  hg_verify_public_device on B's proof
  kernel    the digest kernel's own time and the tree levels' from hg_profile (classes instance_digest_leaves, instance_digest_tree),
            for the compact read (hg_instance_digest) and the laid-out read (hg_values_instance_digest), in a phase of its own

Both provers must give the same root, and each proof must verify where it belongs and nowhere else (asserted before anything is
timed). Printed: median and range of every leg, the differences A - B, and the host tree's time for comparison.

Usage: python scripts/prove_bound_times.py [n k] [--mode 3] [--reps 5] [--log2-row 0]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

hg = load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=32768)
    ap.add_argument("k", nargs="?", type=int, default=16)
    ap.add_argument("--mode", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2-row", type=int, default=0)
    args = ap.parse_args()
    mode = args.mode
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(args.n, args.k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x71AE)
    vals = hg.witness_gen(ctx, pk, w)
    inst = hg.Instance.from_witness(w)
    buf = hg.ProofBuffer(cap=1 << 25)

    def prove_a():
        t0 = time.perf_counter()
        out, cm = hg.prove_committed_mode(ctx, pk, vals, buf, mode, args.log2_row)
        ms = (time.perf_counter() - t0) * 1e3
        proof, root, commit_ms = out.bytes(), cm.root, out.timings()["upload_ms"]
        cm.free()
        return ms, proof, root, commit_ms

    def prove_b():
        t0 = time.perf_counter()
        cm = hg.Commitment.from_values(ctx, pk, vals, args.log2_row)
        t1 = time.perf_counter()
        hg.prove_resident_mode(ctx, pk, vals, buf, mode)
        ms = (time.perf_counter() - t0) * 1e3
        proof, root = buf.bytes(), cm.root
        cm.free()
        return ms, proof, root, (t1 - t0) * 1e3

    def verify_a(proof, root):
        t0 = time.perf_counter()
        ok, why, _ = hg.verify_public_bound(pk, inst, proof, root, mode, ctx=ctx, device=True)
        return (time.perf_counter() - t0) * 1e3, ok, why

    def verify_b(proof):
        t0 = time.perf_counter()
        ok, why, _ = hg.verify_public(pk, inst, proof, mode, ctx=ctx, device=True)
        return (time.perf_counter() - t0) * 1e3, ok, why

    for _ in range(2):   # warm-up: arena, staging, thread pool
        _, bound, root, _ = prove_a()
        _, unbound, root_b, _ = prove_b()
        assert root == root_b, "the two provers commit to different roots"
        assert verify_a(bound, root)[1] and verify_b(unbound)[1]
        assert not verify_a(unbound, root)[1] and not verify_b(bound)[1]
    pa, pb, ca, cb, va, vb = [], [], [], [], [], []
    for _ in range(args.reps):
        ms, proof, r, c_ms = prove_a()
        assert proof == bound and r == root
        pa.append(ms); ca.append(c_ms)
        ms, proof, r, c_ms = prove_b()
        assert proof == unbound and r == root
        pb.append(ms); cb.append(c_ms)
        ms, ok, why = verify_a(bound, root)
        assert ok, why
        va.append(ms)
        ms, ok, why = verify_b(unbound)
        assert ok, why
        vb.append(ms)
    med = statistics.median

    def line(name, t):
        return "  %-44s %9.3f ms (%.3f .. %.3f)" % (name, med(t), min(t), max(t))
    print("n=%d k=%d mode %d, median of %d (min .. max):" % (args.n, args.k, mode, args.reps))
    print(line("prover A  hg_prove_committed_mode", pa))
    print(line("prover B  commit_values + prove_resident_mode", pb) + "   A - B = %+.3f ms (%+.2f %%)" % (med(pa) - med(pb), 100 * (med(pa) / med(pb) - 1)))
    print(line("  commit + digest inside A (host clock)", ca))
    print(line("  commit inside B (host clock)", cb))
    print(line("verifier A  hg_verify_public_bound_device", va))
    print(line("verifier B  hg_verify_public_device", vb) + "   A - B = %+.3f ms (%+.2f %%)" % (med(va) - med(vb), 100 * (med(va) / med(vb) - 1)))

    # the digest alone: device time of its launches from the profiler, wall clock of the three forms
    want = hg.instance_digest(inst)
    ctx.profile(2)
    for name, call in (("compact (hg_instance_digest on the context)", lambda: hg.instance_digest(inst, ctx)),
                       ("laid out (hg_values_instance_digest)", lambda: hg.values_instance_digest(ctx, pk, vals))):
        assert call() == want
        ctx.profile_reset()
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        st = {s["name"]: s for s in ctx.profile_get(64)}
        leaves, tree = st["instance_digest_leaves"], st.get("instance_digest_tree")
        print("  digest, %-44s leaf kernel %.4f ms a launch (%.1f GB/s), tree levels %.4f ms; the call %.3f ms (%.3f .. %.3f)" % (
            name, leaves["total_ms"] / leaves["launches"], leaves["algo_bytes"] / leaves["launches"] / (leaves["total_ms"] / leaves["launches"]) / 1e6,
            tree["total_ms"] / tree["launches"] if tree and tree["launches"] else 0.0, med(wall), min(wall), max(wall)))
    ctx.profile(0)
    host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        hg.instance_digest(inst)
        host.append((time.perf_counter() - t0) * 1e3)
    print(line("digest, host tree (hg_instance_digest, no context)", host))
    vals.free()
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
