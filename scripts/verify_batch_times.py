#!/usr/bin/env python3
"""Per-proof time of hg_verify_device_batch against the same proofs through hg_verify_device (hg_verify_device_mode in modes 1-3)
one by one, in one process. For each mode: up to 16 synthetic witnesses and their proofs of that mode (a batch of B > 16 cycles
through them); for each B of --batch, a warm-up batch call of B proofs, then the median of --reps batch calls divided by B, and
next to it the median of --reps one-by-one passes over the same B proofs divided by B. Every decision is checked (all accepted).
  --field bn254: the same for hg_verify_device_batch_bn254 against hg_verify_device_bn254 (proofs of hg_prove_bn254, mode 0 only).
  --trace: prove 16 proofs in mode 3 (bn254: mode 0), pause, then ONE batch call of those 16 and nothing else (run it under rocprofv3
           --kernel-trace --stats; scripts/trace_after_gap.py then keeps the dispatches behind the pause).
  --public: hg_verify_public_batch, three legs per proof over the same B pairs, their runs ALTERNATED (a, b, c, a, b, c, ..) after a
           warm-up call of each: (a) the batch from the ciphertext, (b) the same pairs through hg_verify_public_device one by one,
           (c) hg_verify_device_batch on the same proofs with the witness handles. Medians and ranges of --reps runs, a/b, and
           whether the whole range of (a) lies below the whole range of (b). With --trace: one public batch of 16 in mode 3.
           With --field bn254: (a) hg_verify_public_batch_bn254, (b) hg_verify_public_device_bn254 one by one, (c)
           hg_verify_device_batch_bn254 on the witnesses of the same pairs (mode 0 only; --trace: one public batch of 16).
Usage: verify_batch_times.py [n k] [--field goldilocks|bn254] [--public] [--modes 0,3] [--batch 1,4,16,64] [--reps 5] [--trace]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

hg = entry.load_package()
DISTINCT = 16


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=32768)
    ap.add_argument("k", type=int, nargs="?", default=16)
    ap.add_argument("--modes", default="0,3")
    ap.add_argument("--batch", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--field", choices=("goldilocks", "bn254"), default="goldilocks")
    ap.add_argument("--public", action="store_true")
    a = ap.parse_args()
    bn = a.field == "bn254"
    if bn:
        a.modes = "0"

    def prove(w, mode):
        return ctx.prove_bn254(pk, w, cap=1 << 25)[0] if bn else bfv.prove(ctx, pk, w, cap=1 << 25, mode=mode)[0]

    def verify_batch(W, P, mode):
        return hg.verify_device_batch_bn254(ctx, pk, W, P) if bn else hg.verify_device_batch(ctx, pk, W, P, mode=mode)

    def verify_one(w, p, mode):
        return hg.verify_device_bn254(ctx, pk, w, p) if bn else hg.verify_device(ctx, pk, w, p, mode=mode)

    def public_batch(I, P, mode):
        return hg.verify_public_batch_bn254(ctx, pk, I, P) if bn else hg.verify_public_batch(ctx, pk, I, P, mode)

    def public_one(inst, p, mode):
        return hg.verify_public_bn254(pk, inst, p, ctx=ctx, device=True) if bn else hg.verify_public(pk, inst, p, mode, ctx=ctx, device=True)
    names = (("hg_verify_public_batch_bn254", "hg_verify_public_device_bn254", "hg_verify_device_batch_bn254") if bn else
             ("hg_verify_public_batch", "hg_verify_public_device", "hg_verify_device_batch"))
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    pk = bfv.setup(ctx)
    batches = [int(b) for b in a.batch.split(",")]
    nw = DISTINCT if a.trace else min(DISTINCT, max(batches))
    ws = [hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n + i) for i in range(nw)]
    insts = [hg.Instance.from_witness(w) for w in ws] if a.public else None
    if a.trace:
        mode = 0 if bn else 3
        ps = [prove(w, mode) for w in ws]
        time.sleep(3.0)   # (longer than any idle stretch of setup, witness generation and prove)
        got = public_batch(insts, ps, mode) if a.public else verify_batch(ws, ps, mode)
        assert all(g[0] for g in got), got
        print("n=%d k=%d %s: one mode-%d %sbatch of %d proofs of %d bytes" % (a.n, a.k, a.field, mode, "public " if a.public else "", len(ps), len(ps[0])))
    elif a.public:
        print("n=%d k=%d, %d distinct witnesses, per proof, one process; %d alternating runs of (a) %s, (b) %s one "
              "by one, (c) %s, after a warm-up call of each: median [min .. max]" % ((a.n, a.k, nw, a.reps) + names))
        for mode in [int(m) for m in a.modes.split(",")]:
            ps = [prove(w, mode) for w in ws]
            for B in batches:
                W, I, P = ([x[i % nw] for i in range(B)] for x in (ws, insts, ps))

                def leg_a():
                    got = public_batch(I, P, mode)
                    assert all(ok for ok, _, _ in got), got

                def leg_b():
                    for inst, p in zip(I, P):
                        ok, why, _ = public_one(inst, p, mode)
                        assert ok, why

                def leg_c():
                    got = verify_batch(W, P, mode)
                    assert all(ok for ok, _ in got), got
                legs = (leg_a, leg_b, leg_c)
                for f in legs:
                    f()
                t = [[], [], []]
                for _ in range(a.reps):
                    for j, f in enumerate(legs):
                        t[j].append(timed(f) / B)
                med = [statistics.median(x) for x in t]
                print("mode %d B=%3d: %s; a/b %.2f; range of (a) %s range of (b); a/c %.2f" % (
                    mode, B, "; ".join("(%s) %.3f [%.3f .. %.3f]" % ("abc"[j], med[j], min(t[j]), max(t[j])) for j in range(3)), med[0] / med[1],
                    "below" if max(t[0]) < min(t[1]) else "NOT below", med[0] / med[2]))
                sys.stdout.flush()
            os.environ["HG_TIMES"] = "verify"
            Bm = max(batches)
            print("mode %d, B=%d with HG_TIMES=verify: the public batch, then %s" % (mode, Bm, names[2]), file=sys.stderr)
            public_batch([insts[i % nw] for i in range(Bm)], [ps[i % nw] for i in range(Bm)], mode)
            verify_batch([ws[i % nw] for i in range(Bm)], [ps[i % nw] for i in range(Bm)], mode)
            del os.environ["HG_TIMES"]
    else:
        print("n=%d k=%d %s, %d distinct witnesses, median of %d after a warm-up, per proof, one process" % (a.n, a.k, a.field, nw, a.reps))
        for mode in [int(m) for m in a.modes.split(",")]:
            ps = [prove(w, mode) for w in ws]
            for B in batches:
                W = [ws[i % nw] for i in range(B)]
                P = [ps[i % nw] for i in range(B)]

                def batch():
                    got = verify_batch(W, P, mode)
                    assert all(ok for ok, _ in got), got

                def singles():
                    for w, p in zip(W, P):
                        ok, why = verify_one(w, p, mode)
                        assert ok, why
                batch()
                tb = [timed(batch) / B for _ in range(a.reps)]
                singles()
                ts = [timed(singles) / B for _ in range(a.reps)]
                mb, ms = statistics.median(tb), statistics.median(ts)
                print("mode %d B=%3d: batch %.3f ms/proof (%s); one by one %.3f ms/proof (%s); ratio %.2f" % (
                    mode, B, mb, " ".join("%.3f" % x for x in tb), ms, " ".join("%.3f" % x for x in ts), mb / ms))
                sys.stdout.flush()
            os.environ["HG_TIMES"] = "verify"
            print("mode %d, B=%d with HG_TIMES=verify:" % (mode, max(batches)), file=sys.stderr)
            verify_batch([ws[i % nw] for i in range(max(batches))], [ps[i % nw] for i in range(max(batches))], mode)
            del os.environ["HG_TIMES"]
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
