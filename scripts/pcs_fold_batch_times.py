#!/usr/bin/env python3
"""Times of folded openings as a run against one by one, in one process. B distinct synthetic witnesses are each proven and publicly
verified (hg_verify_public_batch) and committed (hg_secrets_commit_batch) outside the timed region. Per batch size the legs of a step
are ALTERNATED, after one warm-up call of each, --reps timed calls each, all through the C entries on argument arrays built beforehand:
  open_folded_batch      one hg_claims_open_folded_batch over the B commitments
  open_folded_one_by_one hg_claims_open_folded, one call each, on the same handles
  open_batch             one hg_claims_open_batch (the unfolded opening, for context)
  verify_folded_batch      one hg_claims_verify_folded_batch over the B folded openings
  verify_folded_one_by_one hg_claims_verify_folded_device, one call each
  verify_batch             one hg_claims_verify_batch over the B unfolded openings (for context)
Prints per-item wall clock (median and range) per leg and whether the whole range of the folded batch leg lies below the one-by-one
leg's. One more call of each batch leg follows under hg_profile level 2: the kernel time of the classes pcs_fold_batch, pcs_open_batch
and pcs_verify_batch (over BN254: pcs_fold_batch_bn254, pcs_bn254_open_batch, pcs_bn254_verify_batch), and one more folded open with
HG_DEBUG=plan and HG_TIMES=pcs set for that call alone: the group sizes the budget gave and where a group's wall clock goes, on stderr.
--bn254: the same legs through the _bn254 entries (hg_prove_bn254, hg_verify_public_batch_bn254, hg_secrets_commit_batch_bn254).
Usage: pcs_fold_batch_times.py [n k] [--batch 1,16,64] [--reps 5] [--bn254]"""
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
    a = ap.parse_args()
    sfx = "_bn254" if a.bn254 else ""
    sizes = [int(x) for x in a.batch.split(",")]
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

    def entry_of(name):   # the C entry of this field
        return getattr(L, name + sfx)

    F = hg.InputClaimsBn254 if a.bn254 else hg.InputClaims
    held = (hg.Commitment.secrets_batch_bn254 if a.bn254 else hg.Commitment.secrets_batch)(ctx, params, ws)
    nvars, c = held[0].nvars, held[0].log2_row
    if a.bn254:
        fcap, cap = hg.pcs_folded_opening_bytes_bn254(nvars, 0, c), hg.pcs_opening_bytes_bn254(nvars, max(cl.n for cl in cls), 0, c)
    else:
        fcap, cap = hg.pcs_folded_opening_bytes(nvars, 0, c), hg.pcs_opening_bytes(nvars, max(cl.n for cl in cls), 0, c)
    print("%s n=%d k=%d: %d claims an item, 241 queries, %d bytes a folded opening, %d an unfolded one" % ("bn254" if a.bn254 else "goldilocks", a.n, a.k, cls[0].n, fcap, cap))
    # the openings the verify legs run on, made once
    folded = (hg.claims_open_folded_batch_bn254 if a.bn254 else hg.claims_open_folded_batch)(ctx, params, held, cls)
    plain = (hg.claims_open_batch_bn254 if a.bn254 else hg.claims_open_batch)(ctx, params, held, cls)
    assert all(why == "" for _, why in folded + plain)
    assert folded[0][0] == held[0].open_claims_folded(params, cls[0])
    for B in sizes:
        claims, nc1, points, nco1, counts = hg._claims_batch_arrays(cls[:B], F)
        cms = (C.c_void_p * B)(*[cm.h for cm in held[:B]])
        root = [bytes(cm.root) for cm in held[:B]]
        roots = (C.c_char_p * B)(*root)
        buf = np.zeros(B * cap, dtype=np.uint8)
        out = buf.ctypes.data_as(hg.u8p)
        lens, status, one_len, res = (C.c_size_t * B)(), (C.c_int * B)(), C.c_size_t(0), (C.c_int * B)()
        fo = (C.c_char_p * B)(*[b for b, _ in folded[:B]])
        fl = (C.c_size_t * B)(*[len(b) for b, _ in folded[:B]])
        po = (C.c_char_p * B)(*[b for b, _ in plain[:B]])
        pl = (C.c_size_t * B)(*[len(b) for b, _ in plain[:B]])
        head = (ctx.h, C.byref(params))
        block = (claims, nc1, hg._ptr(points), nco1, counts, 0)

        def open_folded_batch():
            assert entry_of("hg_claims_open_folded_batch")(*head, cms, *block, B, out, fcap, lens, status, None, 0) == 0, L.hg_last_error()

        def open_folded_one_by_one():
            for i in range(B):
                assert entry_of("hg_claims_open_folded")(*head, cms[i], cls[i].claims, cls[i].n, hg._ptr(cls[i].points), 0, out, fcap, C.byref(one_len)) == 0, L.hg_last_error()

        def open_batch():
            assert entry_of("hg_claims_open_batch")(*head, cms, *block, B, out, cap, lens, status, None, 0) == 0, L.hg_last_error()

        def verify_folded_batch():
            assert entry_of("hg_claims_verify_folded_batch")(*head, roots, 0, *block, fo, fl, B, res, None, 0) == 0, L.hg_last_error()

        def verify_folded_one_by_one():
            for i in range(B):
                assert entry_of("hg_claims_verify_folded_device")(*head, root[i], 0, cls[i].claims, cls[i].n, hg._ptr(cls[i].points), 0, folded[i][0], fl[i]) == 0, L.hg_last_error()

        def verify_batch():
            assert entry_of("hg_claims_verify_batch")(*head, roots, 0, *block, po, pl, B, res, None, 0) == 0, L.hg_last_error()

        steps = ((("open_folded_batch", open_folded_batch), ("open_folded_one_by_one", open_folded_one_by_one), ("open_batch", open_batch)),
                 (("verify_folded_batch", verify_folded_batch), ("verify_folded_one_by_one", verify_folded_one_by_one), ("verify_batch", verify_batch)))
        for legs in steps:
            times = {name: [] for name, _ in legs}
            for rep in range(a.reps + 1):   # rep 0: the warm-up call of each leg
                for name, fn in legs:
                    t0 = time.perf_counter()
                    fn()
                    if rep:
                        times[name].append((time.perf_counter() - t0) * 1e3 / B)
            for name, _ in legs:
                t = times[name]
                print("B=%-3d %-24s per item: median %.3f ms, range %.3f .. %.3f ms (%s)" % (B, name, statistics.median(t), min(t), max(t), " ".join("%.3f" % x for x in t)), flush=True)
            b, o = times[legs[0][0]], times[legs[1][0]]
            print("B=%-3d %s: %s" % (B, legs[0][0], "the batch leg's whole range lies below the one-by-one leg's" if max(b) < min(o) else
                                     "the batch leg's whole range lies ABOVE the one-by-one leg's" if min(b) > max(o) else "the ranges overlap: no difference shown"), flush=True)
        ctx.profile(2)
        for name, fn in (("open_folded_batch", open_folded_batch), ("open_batch", open_batch), ("verify_folded_batch", verify_folded_batch), ("verify_batch", verify_batch)):
            ctx.profile_reset()
            fn()
            for st in ctx.profile_get(256):
                if st["name"] in (("pcs_fold_batch_bn254", "pcs_bn254_open_batch", "pcs_bn254_verify_batch") if a.bn254 else ("pcs_fold_batch", "pcs_open_batch", "pcs_verify_batch")) and \
                        st["launches"]:
                    print("B=%-3d %-24s class %-18s %4d launches %8.3f ms in all, %.3f ms an item" % (B, name, st["name"], st["launches"], st["total_ms"], st["total_ms"] / B), flush=True)
        ctx.profile(0)
        before = {k: os.environ.get(k) for k in ("HG_DEBUG", "HG_TIMES")}
        os.environ.update(HG_DEBUG="plan", HG_TIMES="pcs")   # (read at every call) the groups of this run and their breakdown, on stderr
        print("B=%-3d one folded open with HG_DEBUG=plan HG_TIMES=pcs:" % B, file=sys.stderr, flush=True)
        open_folded_batch()
        for k, v in before.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    for cm in held:
        cm.free()
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
