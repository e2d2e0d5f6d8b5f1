#!/usr/bin/env python3
"""Times of hg_claims_verify_batch against hg_claims_verify_device one by one, in one process. B distinct synthetic witnesses are each
proven, publicly verified (hg_verify_public_batch), committed (hg_secrets_commit on the context) and opened once, outside the timed
region. Per batch size two legs are ALTERNATED, after one warm-up call of each, --reps timed calls each, both through the C entries
on argument arrays built beforehand:
  batch       one hg_claims_verify_batch over the B openings
  one_by_one  hg_claims_verify_device over the same openings, one call each
Prints per-opening wall clock (median and range) per leg and whether the whole range of the batch leg lies below the other's.
--profile: instead of the timed legs, one call of each leg per batch size under hg_profile level 2: the kernel time of the classes
pcs_verify_batch (per group) and pcs_verify (per opening). HG_TIMES=pcs in the environment prints where a group's wall clock goes.
--bn254: the same comparison over bn256::Fr (hg_prove_bn254, hg_verify_public_batch_bn254, hg_secrets_commit_bn254,
hg_claims_verify_batch_bn254 against hg_claims_verify_device_bn254; classes pcs_bn254_verify_batch and pcs_bn254_verify), and the
profiled calls follow the timed legs in the same process.
Usage: pcs_verify_batch_times.py [n k] [--verify-batch 1,16,64] [--reps 5] [--profile] [--bn254]"""
import argparse
import ctypes as C
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
    ap.add_argument("--verify-batch", default="1,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--bn254", action="store_true")
    a = ap.parse_args()
    F = hg.InputClaimsBn254 if a.bn254 else hg.InputClaims
    classes = ("pcs_bn254_verify", "pcs_bn254_verify_batch") if a.bn254 else ("pcs_verify", "pcs_verify_batch")
    sizes = [int(x) for x in a.verify_batch.split(",")]
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n + i) for i in range(max(sizes))]
    insts = [hg.Instance.from_witness(w) for w in ws]
    if a.bn254:
        got = hg.verify_public_batch_bn254(ctx, pk, insts, [ctx.prove_bn254(pk, w, cap=1 << 25)[0] for w in ws])
    else:
        got = hg.verify_public_batch(ctx, pk, insts, [bfv.prove(ctx, pk, w, cap=1 << 25)[0] for w in ws], 0)
    assert all(ok for ok, _, _ in got)
    cls = [cl for _, _, cl in got]
    roots, openings = [], []
    for w, cl in zip(ws, cls):
        cm = (hg.Commitment.secrets_bn254 if a.bn254 else hg.Commitment.secrets)(ctx, bfv.params, w)
        roots.append(cm.root)
        openings.append(cm.open_claims(bfv.params, cl))
        cm.free()
    L = hg.lib()
    batch_entry, single_entry = getattr(L, "hg_claims_verify_batch" + F.SFX), getattr(L, "hg_claims_verify_device" + F.SFX)
    print("%s n=%d k=%d: %d claims an opening, 241 queries, %d bytes an opening" % ("bn254" if a.bn254 else "goldilocks", a.n, a.k, cls[0].n, len(openings[0])))
    for B in sizes:
        claims, nc1, points, nco1, counts = hg._claims_batch_arrays(cls[:B], F)
        rs = (C.c_char_p * B)(*roots[:B])
        ps = (C.c_char_p * B)(*openings[:B])
        lens = (C.c_size_t * B)(*[len(o) for o in openings[:B]])
        res = (C.c_int * B)()
        reasons = C.create_string_buffer(B * 256)

        def batch():
            assert batch_entry(ctx.h, C.byref(bfv.params), rs, 0, claims, nc1, hg._ptr(points), nco1, counts, 0, ps, lens, B, res, reasons, 256) == 0, hg.lib().hg_last_error()

        def one_by_one():
            for i in range(B):
                cl = cls[i]
                assert single_entry(ctx.h, C.byref(bfv.params), roots[i], 0, cl.claims, cl.n, hg._ptr(cl.points), 0, openings[i], len(openings[i])) == 0

        legs = [("batch", batch), ("one_by_one", one_by_one)]

        def profiled():
            ctx.profile(2)
            for name, fn in legs:
                fn()
                ctx.profile_reset()
                fn()
                for st in ctx.profile_get(256):
                    if st["name"] in classes and st["launches"]:
                        print("B=%-3d %-11s class %-23s %4d launches %8.3f ms in all, %.3f ms an opening" % (B, name, st["name"], st["launches"], st["total_ms"], st["total_ms"] / B))
            ctx.profile(0)

        if a.profile:
            profiled()
            continue
        times = {name: [] for name, _ in legs}
        for rep in range(a.reps + 1):   # rep 0: the warm-up call of each leg
            for name, fn in legs:
                t0 = time.perf_counter()
                fn()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3 / B)
        for name, _ in legs:
            t = times[name]
            print("B=%-3d %-11s per opening: median %.3f ms, range %.3f .. %.3f ms (%s)" % (B, name, statistics.median(t), min(t), max(t), " ".join("%.3f" % x for x in t)))
        b, o = times["batch"], times["one_by_one"]
        print("B=%-3d %s" % (B, "the batch leg's whole range lies below the one-by-one leg's" if max(b) < min(o) else
                             "the batch leg's whole range lies ABOVE the one-by-one leg's" if min(b) > max(o) else "the ranges overlap: no difference shown"))
        if a.bn254:
            profiled()
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
