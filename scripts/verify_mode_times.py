#!/usr/bin/env python3
"""Device and host verification times of one proof per mode, in one process: hg_verify_device_mode and hg_verify_mode on a
synthetic witness's hg_prove_mode proof (hg_prove in mode 0), median of --reps after a warm-up, then one device verification per
mode with HG_TIMES=verify (its laps go to stderr).
  --trace: prove in mode 3, pause, then ONE device verification in mode 3 and nothing else (run it under rocprofv3 --kernel-trace;
           scripts/trace_after_gap.py then keeps the dispatches behind the pause).
Usage: verify_mode_times.py [n k] [--modes 0,3] [--reps 5] [--trace]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

hg = entry.load_package()


def median_ms(fn, reps):
    t = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        ok, why = fn()
        assert ok, why
        if i:
            t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=32768)
    ap.add_argument("k", type=int, nargs="?", default=16)
    ap.add_argument("--modes", default="0,3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n)
    if a.trace:
        proof, _ = bfv.prove(ctx, pk, w, cap=1 << 25, mode=3)
        time.sleep(3.0)   # (longer than any idle stretch of setup, witness generation and prove)
        ok, why = hg.verify_device(ctx, pk, w, proof, mode=3)
        assert ok, why
        print("n=%d k=%d: one mode-3 device verification of a %d-byte proof" % (a.n, a.k, len(proof)))
    else:
        print("n=%d k=%d, median of %d after a warm-up, one process" % (a.n, a.k, a.reps))
        for mode in [int(m) for m in a.modes.split(",")]:
            proof, tm = bfv.prove(ctx, pk, w, cap=1 << 25, mode=mode)
            dev, dl = median_ms(lambda: hg.verify_device(ctx, pk, w, proof, mode=mode), a.reps)
            host, hl = median_ms(lambda: hg.verify(pk, w, proof, mode=mode), a.reps)
            print("mode %d: proof %d bytes, prove %.1f ms; device %.2f ms (%s); host %.1f ms (%s)" % (
                mode, len(proof), tm["prove_ms"], dev, " ".join("%.2f" % x for x in dl), host, " ".join("%.1f" % x for x in hl)))
            sys.stdout.flush()
            os.environ["HG_TIMES"] = "verify"
            print("mode %d with HG_TIMES=verify:" % mode, file=sys.stderr)
            assert hg.verify_device(ctx, pk, w, proof, mode=mode)[0]
            del os.environ["HG_TIMES"]
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
