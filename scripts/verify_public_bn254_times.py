#!/usr/bin/env python3
"""Times of the BN254 verification from the ciphertext against the device verifier that takes the witness, in one process: three legs
ALTERNATED on one hg_prove_bn254 proof of a synthetic witness, after one warm-up call of each leg, --reps timed calls each:
  public   hg_verify_public_device_bn254 (instance uploaded, claims handed back)
  full     hg_verify_device_bn254 on the same proof and witness (the baseline, same run)
  settle   hg_claims_settle_bn254 with a context, on the claims of the public leg
Prints median and range per leg and whether the whole range of `public` lies below the whole range of `full`; then one call of
`public` and of `full` with HG_TIMES=verify (their laps go to stderr).
Usage: verify_public_bn254_times.py [n k] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

hg = entry.load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=32768)
    ap.add_argument("k", type=int, nargs="?", default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n)
    inst = hg.Instance.from_witness(w)
    proof = ctx.prove_bn254(pk, w, cap=1 << 26)[0]
    ok, why, claims = hg.verify_public_bn254(pk, inst, proof, ctx=ctx, device=True)
    assert ok, why
    legs = [("public", lambda: hg.verify_public_bn254(pk, inst, proof, ctx=ctx, device=True)[:2]),
            ("full", lambda: hg.verify_device_bn254(ctx, pk, w, proof)),
            ("settle", lambda: hg.claims_settle_bn254(ctx, bfv.params, w, claims))]
    times = {name: [] for name, _ in legs}
    for rep in range(a.reps + 1):   # rep 0: the warm-up call of each leg
        for name, fn in legs:
            t0 = time.perf_counter()
            ok, why = fn()
            dt = (time.perf_counter() - t0) * 1e3
            assert ok, (name, why)
            if rep:
                times[name].append(dt)
    print("n=%d k=%d, bn254 proof %d bytes, %d claims; legs alternated, %d timed calls each after one warm-up call, one process" % (
        a.n, a.k, len(proof), claims.n, a.reps))
    for name, _ in legs:
        t = times[name]
        print("%-6s median %.2f ms, range %.2f .. %.2f ms (%s)" % (name, statistics.median(t), min(t), max(t), " ".join("%.2f" % x for x in t)))
    pub, full = times["public"], times["full"]
    if max(pub) < min(full):
        print("public is faster than full: its whole range lies below the baseline's")
    elif min(pub) > max(full):
        print("public is SLOWER than full: its whole range lies above the baseline's")
    else:
        print("public and full overlap: no difference shown")
    sys.stdout.flush()
    os.environ["HG_TIMES"] = "verify"
    for name, fn in legs[:2]:
        print("%s with HG_TIMES=verify:" % name, file=sys.stderr)
        assert fn()[0]
    del os.environ["HG_TIMES"]
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
