#!/usr/bin/env python3
"""Per-item wall clock of proof + commitment for a run of encryptions, two ways, alternated in one process:

  A  hg_prove_encryptions_committed(.., ws = NULL): the commit inside the pipeline, from the node tables; handles freed after each call
  B  hg_prove_encryptions(.., ws) followed by hg_secrets_commit_batch on the returned handles; handles and witnesses freed

Both must give identical proofs and roots (asserted before anything is timed). Printed per run length: median and range per item of
both legs, their ratio, and for leg A the commit's device time per item (timings.upload_ms / n) and gpu_ms / n beside leg B's gpu_ms / n
(the prove's device time with and without a commit running beside it).

--bn254 runs the same legs over the BN254 entries: A hg_prove_encryptions_committed_bn254(.., ws = NULL), B hg_prove_encryptions_bn254(.., ws)
followed by hg_secrets_commit_batch_bn254, and hg_prove_encryptions_bn254(.., ws = NULL) alone. That path has no gpu_ms; prove_ms / n (the
proving spans, wall clock) stands in its place.

Usage: python scripts/prove_committed_times.py [n k] [--runs 16,64] [--reps 5] [--log2-row 0] [--bn254]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

hg = load_package()
P = hg.P


def signed(words):
    w = np.asarray(words, dtype=np.uint64)
    neg = w > np.uint64(P // 2)
    out = w.astype(np.int64)
    out[neg] = -((np.uint64(P) - w[neg]).astype(np.int64))
    return out


def encryption_of(params, d):
    """the signed ascending polynomials (s, e, k1, a[k][n]) a set of laid-out tables holds"""
    n, k = params.n, params.k
    s = signed(d["s"][:n])[::-1]
    e = signed(d["e"][n - 1:2 * n - 1])[::-1]
    k1 = signed(d["k1"][n - 1:2 * n - 1])[::-1]
    a = np.stack([signed(d["ais"][i * 2 * n:i * 2 * n + n])[::-1] for i in range(k)])
    return tuple(np.ascontiguousarray(x) for x in (s, e, k1, a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=32768)
    ap.add_argument("k", nargs="?", type=int, default=16)
    ap.add_argument("--runs", default="16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2-row", type=int, default=0)
    ap.add_argument("--bn254", action="store_true")
    args = ap.parse_args()
    if args.bn254:
        committed, plain, commit_batch, dev, sfx = hg.prove_encryptions_committed_bn254, hg.prove_encryptions_bn254, hg.Commitment.secrets_batch_bn254, "prove_ms", "_bn254"
    else:
        committed, plain, commit_batch, dev, sfx = hg.prove_encryptions_committed, hg.prove_encryptions, hg.Commitment.secrets_batch, "gpu_ms", ""
    runs = [int(x) for x in args.runs.split(",")]
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(args.n, args.k)
    params = bfv.params
    pk = bfv.setup(ctx)
    pool = [encryption_of(params, hg.Witness.synthetic(params, 0x71AE + 3 * i).arrays()) for i in range(min(max(runs), 16))]
    cap = 1 << 22

    for run in runs:
        encs = [pool[i % len(pool)] for i in range(run)]

        def leg_a():
            t0 = time.perf_counter()
            proofs, status, _, cms, roots, _, tm = committed(ctx, pk, encs, log2_row=args.log2_row, cap_each=cap)
            for cm in cms:
                cm.free()
            ms = (time.perf_counter() - t0) * 1e3 / run
            assert status == [0] * run
            return ms, proofs, roots, tm

        def leg_b():
            t0 = time.perf_counter()
            proofs, status, _, ws, tm = plain(ctx, pk, encs, cap_each=cap, witnesses=True)
            cms = commit_batch(ctx, params, ws, args.log2_row)
            roots = [cm.root for cm in cms]
            for cm in cms:
                cm.free()
            del ws[:]
            ms = (time.perf_counter() - t0) * 1e3 / run
            assert status == [0] * run
            return ms, proofs, roots, tm

        def alone():   # the pipeline without commitments and without handles: what the commit is enqueued beside
            t0 = time.perf_counter()
            proofs, status, _, _, tm = plain(ctx, pk, encs, cap_each=cap, witnesses=False)
            return (time.perf_counter() - t0) * 1e3 / run, proofs, tm

        for _ in range(2):   # warm-up: launch graphs, staging, group allocations, thread pool
            _, want, want_roots, _ = leg_b()
            _, proofs, roots, _ = leg_a()
            assert proofs == want and roots == want_roots, "the two legs differ"
            assert alone()[1] == want
        ta, tb, tc, commit, gpu_a, gpu_b, gpu_c, wit = [], [], [], [], [], [], [], []
        for _ in range(args.reps):
            ms, proofs, tm = alone()
            assert proofs == want
            tc.append(ms); gpu_c.append(tm[dev] / run)
            ms, proofs, roots, tm = leg_b()
            assert proofs == want and roots == want_roots
            tb.append(ms); gpu_b.append(tm[dev] / run)
            ms, proofs, roots, tm = leg_a()
            assert proofs == want and roots == want_roots
            ta.append(ms); commit.append(tm["upload_ms"] / run); gpu_a.append(tm[dev] / run); wit.append(tm["witness_ms"] / run)
        med = statistics.median
        print("n=%d k=%d run=%d%s, per item, median of %d (min .. max):" % (args.n, args.k, run, " over bn256::Fr" if args.bn254 else "", args.reps))
        print("  A committed pipeline          %.3f ms (%.3f .. %.3f)" % (med(ta), min(ta), max(ta)))
        print("  B prove, then commit batch    %.3f ms (%.3f .. %.3f)   A / B = %.3f" % (med(tb), min(tb), max(tb), med(ta) / med(tb)))
        print("  A commit device time          %.3f ms; derivation + evaluation + commit %.3f ms" % (med(commit), med(wit)))
        print("  hg_prove_encryptions%s alone    %.3f ms (%.3f .. %.3f), no commitment, no handles" % (sfx, med(tc), min(tc), max(tc)))
        print("  %s / n                    A %.3f ms beside the commit, B %.3f ms, hg_prove_encryptions%s alone %.3f ms" % (dev, med(gpu_a), med(gpu_b), sfx, med(gpu_c)))
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
