#!/usr/bin/env python3
"""Times of the prover's two commitment steps as a run against one by one, in one process. B distinct synthetic witnesses are each
proven and publicly verified (hg_verify_public_batch) outside the timed region. Per batch size two pairs of legs are ALTERNATED,
after one warm-up call of each, --reps timed calls each, all through the C entries on argument arrays built beforehand:
  commit_batch       one hg_secrets_commit_batch over the B witnesses          commit_one_by_one  hg_secrets_commit, one call each
  open_batch         one hg_claims_open_batch over the B commitments           open_one_by_one    hg_claims_open, one call each
The handles a commit leg makes are freed inside the leg (as a caller of either form must; the share of hg_pcs_free is printed
beside it); the open legs run on commitments made once by hg_secrets_commit_batch. Prints per-item wall clock (median and range) per leg and whether the whole range of the batch leg
lies below the other's. One more call of each leg follows under hg_profile level 2: the kernel time of the classes pcs_commit_batch
and pcs_open_batch. HG_TIMES=pcs in the environment prints where a group's wall clock goes (the allocation's share of a commit group
among it) and what an open run costs around its passes. --bn254 times the same legs over bn256::Fr (hg_secrets_commit_batch_bn254 / hg_claims_open_batch_bn254 against
hg_secrets_commit_bn254 / hg_claims_open_bn254, on hg_prove_bn254 proofs; classes pcs_bn254_commit_batch and pcs_bn254_open_batch).
--group 4,8,16 repeats every batch size under each value of the context option verify_batch_group (0: the default).
Usage: pcs_prove_batch_times.py [n k] [--bn254] [--batch 1,16,64] [--group 0] [--reps 5]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

hg = entry.load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=32768)
    ap.add_argument("k", type=int, nargs="?", default=16)
    ap.add_argument("--batch", default="1,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bn254", action="store_true")
    ap.add_argument("--group", default="0")
    a = ap.parse_args()
    sizes = [int(x) for x in a.batch.split(",")]
    sfx, F = ("_bn254", hg.InputClaimsBn254) if a.bn254 else ("", hg.InputClaims)
    classes = ("pcs_bn254_commit_batch", "pcs_bn254_open_batch") if a.bn254 else ("pcs_commit_batch", "pcs_open_batch")
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    params = bfv.params
    pk = bfv.setup(ctx)
    ws = [hg.Witness.synthetic(params, 0x4752454330 + a.n + i) for i in range(max(sizes))]
    insts = [hg.Instance.from_witness(w) for w in ws]
    if a.bn254:
        got = hg.verify_public_batch_bn254(ctx, pk, insts, [ctx.prove_bn254(pk, w, cap=1 << 25)[0] for w in ws])
    else:
        got = hg.verify_public_batch(ctx, pk, insts, [bfv.prove(ctx, pk, w, cap=1 << 25)[0] for w in ws], 0)
    assert all(ok for ok, _, _ in got)
    cls = [cl for _, _, cl in got]
    L = hg.lib()
    commit_batch_fn, commit_fn = getattr(L, "hg_secrets_commit_batch" + sfx), getattr(L, "hg_secrets_commit" + sfx)
    open_batch_fn, open_fn = getattr(L, "hg_claims_open_batch" + sfx), getattr(L, "hg_claims_open" + sfx)
    held = (hg.Commitment.secrets_batch_bn254 if a.bn254 else hg.Commitment.secrets_batch)(ctx, params, ws)   # what the open legs run on
    cap = (hg.pcs_opening_bytes_bn254 if a.bn254 else hg.pcs_opening_bytes)(held[0].nvars, max(cl.n for cl in cls), 0, held[0].log2_row)
    print("%s n=%d k=%d: %d claims an item, 241 queries, %d bytes an opening" % ("bn254" if a.bn254 else "goldilocks", a.n, a.k, cls[0].n, cap))
    for group, B in [(int(g), B) for g in a.group.split(",") for B in sizes]:
        ctx.set_option("verify_batch_group", group)
        if a.group != "0":
            print("verify_batch_group = %d" % group, flush=True)
        wh = (C.c_void_p * B)(*[w.h for w in ws[:B]])
        hs, roots = (C.c_void_p * B)(), (C.c_uint8 * (32 * B))()
        claims, nc1, points, nco1, counts = hg._claims_batch_arrays(cls[:B], F)
        cms = (C.c_void_p * B)(*[cm.h for cm in held[:B]])
        buf = np.zeros(B * cap, dtype=np.uint8)
        out = buf.ctypes.data_as(hg.u8p)
        lens, status, one_len = (C.c_size_t * B)(), (C.c_int * B)(), C.c_size_t(0)

        freeing = {"commit_batch": [], "commit_one_by_one": []}   # the share of hg_pcs_free in a commit leg, ms per item

        def commit_batch():
            assert commit_batch_fn(ctx.h, C.byref(params), wh, B, 0, hs, roots) == 0, L.hg_last_error()
            t0 = time.perf_counter()
            for i in range(B):
                L.hg_pcs_free(hs[i])
            freeing["commit_batch"].append((time.perf_counter() - t0) * 1e3 / B)

        def commit_one_by_one():
            h, root = C.c_void_p(), (C.c_uint8 * 32)()
            spent = 0.0
            for i in range(B):
                assert commit_fn(ctx.h, C.byref(params), wh[i], 0, C.byref(h), root) == 0, L.hg_last_error()
                t0 = time.perf_counter()
                L.hg_pcs_free(h)
                spent += time.perf_counter() - t0
            freeing["commit_one_by_one"].append(spent * 1e3 / B)

        def open_batch():
            assert open_batch_fn(ctx.h, C.byref(params), cms, claims, nc1, hg._ptr(points), nco1, counts, 0, B, out, cap, lens, status, None, 0) == 0, L.hg_last_error()

        def open_one_by_one():
            for i in range(B):
                cl = cls[i]
                assert open_fn(ctx.h, C.byref(params), cms[i], cl.claims, cl.n, hg._ptr(cl.points), 0, out, cap, C.byref(one_len)) == 0, L.hg_last_error()

        for pair in ((("commit_batch", commit_batch), ("commit_one_by_one", commit_one_by_one)), (("open_batch", open_batch), ("open_one_by_one", open_one_by_one))):
            times = {name: [] for name, _ in pair}
            for rep in range(a.reps + 1):   # rep 0: the warm-up call of each leg
                for name, fn in pair:
                    t0 = time.perf_counter()
                    fn()
                    if rep:
                        times[name].append((time.perf_counter() - t0) * 1e3 / B)
            for name, _ in pair:
                t = times[name]
                print("B=%-3d %-17s per item: median %.3f ms, range %.3f .. %.3f ms (%s)" % (B, name, statistics.median(t), min(t), max(t), " ".join("%.3f" % x for x in t)), flush=True)
                if name in freeing:
                    f = freeing[name][1:1 + a.reps]
                    print("B=%-3d %-17s of which hg_pcs_free: median %.3f ms, range %.3f .. %.3f ms" % (B, name, statistics.median(f), min(f), max(f)), flush=True)
            b, o = times[pair[0][0]], times[pair[1][0]]
            print("B=%-3d %s: %s" % (B, pair[0][0], "the batch leg's whole range lies below the one-by-one leg's" if max(b) < min(o) else
                                     "the batch leg's whole range lies ABOVE the one-by-one leg's" if min(b) > max(o) else "the ranges overlap: no difference shown"), flush=True)
        ctx.profile(2)
        for name, fn in (("commit_batch", commit_batch), ("open_batch", open_batch)):
            ctx.profile_reset()
            fn()
            for st in ctx.profile_get(256):
                if st["name"] in classes and st["launches"]:
                    print("B=%-3d %-17s class %-22s %4d launches %8.3f ms in all, %.3f ms an item" % (B, name, st["name"], st["launches"], st["total_ms"], st["total_ms"] / B), flush=True)
        ctx.profile(0)
    ctx.set_option("verify_batch_group", 0)
    for cm in held:
        cm.free()
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
