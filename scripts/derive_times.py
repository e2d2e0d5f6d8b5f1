#!/usr/bin/env python3
"""Times of the witness derivation, one process, after a warm-up: median wall time of hg_witness_derive, of hg_witness_derive_into
(with its device time from HIP events) and of the host computation they replace (hg_witness_synthetic: the same rule, schoolbook
on the host threads the process was granted). The three are interleaved rep by rep; every derived witness is compared with the host's.
Usage: derive_times.py [n k] [--reps 7]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

hg = entry.load_package()
INPUTS = ("s", "e", "k1", "ais")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=32768)
    ap.add_argument("k", type=int, nargs="?", default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    pk = bfv.setup(ctx)
    seeds = [0x4752454330 + a.n + i for i in range(a.reps + 1)]
    full = hg.Witness.synthetic(bfv.params, seeds[0]).arrays()
    vals = hg.witness_gen(ctx, pk, hg.Witness.from_arrays(bfv.params, full))
    d = {f: full[f] for f in INPUTS}
    for _ in range(2):                                      # warm-up: arena, code objects
        hg.Witness.derive(ctx, bfv.params, d)
        hg.witness_derive_into(ctx, pk, d, vals)
    t_host, t_derive, t_into, t_into_gpu = [], [], [], []
    for seed in seeds[1:]:
        t0 = time.perf_counter()
        w = hg.Witness.synthetic(bfv.params, seed)
        t_host.append((time.perf_counter() - t0) * 1e3)
        full = w.arrays()
        d = {f: full[f] for f in INPUTS}
        t0 = time.perf_counter()
        got = hg.Witness.derive(ctx, bfv.params, d)
        t_derive.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        got2 = hg.witness_derive_into(ctx, pk, d, vals)
        t_into.append((time.perf_counter() - t0) * 1e3)
        t_into_gpu.append(vals.timings["gpu_ms"])
        for g in (got.arrays(), got2.arrays()):
            assert all((g[f] == full[f]).all() for f in hg.Witness.FIELDS), "derived witness differs from the host's"

    def line(name, t):
        print("%-46s median %9.3f ms   (%s)" % (name, statistics.median(t), " ".join("%.2f" % x for x in t)))
    print("n=%d k=%d, %d reps interleaved after a warm-up, one process, %s host threads" % (a.n, a.k, a.reps, os.environ.get("OMP_NUM_THREADS", "default")))
    line("hg_witness_synthetic (host, the path replaced)", t_host)
    line("hg_witness_derive (wall)", t_derive)
    line("hg_witness_derive_into (wall)", t_into)
    line("hg_witness_derive_into (device, HIP events)", t_into_gpu)
    vals.free()
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
