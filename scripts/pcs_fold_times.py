#!/usr/bin/env python3
"""Times of the folded opening against the unfolded one over the secret inputs, in one process: the legs ALTERNATED on one synthetic
witness and the claims hg_verify_public_device leaves on its hg_prove proof, device commitment, after one warm-up call of each leg,
--reps timed calls each:
  open / open_folded                  hg_claims_open / hg_claims_open_folded of those claims (default 241 queries)
  verify_dev / verify_dev_folded      hg_claims_verify_device / hg_claims_verify_folded_device of the opening: the whole call, upload included
  verify_host / verify_host_folded    hg_claims_verify / hg_claims_verify_folded
Prints the bytes of both openings, median and range per leg, per pair whether the whole range of the folded form lies below that of the
unfolded form, then the kernel time of one more folded open under hg_profile (class pcs_fold: the g table, the rounds, their sums).
--bn254: the same legs over bn256::Fr - the claims of hg_verify_public_device_bn254 on an hg_prove_bn254 proof, the hg_claims_*_bn254
entries, class pcs_fold_bn254.
Usage: pcs_fold_times.py [n k] [--reps 5] [--bn254]"""
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
    ap.add_argument("--bn254", action="store_true")
    a = ap.parse_args()
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n)
    if a.bn254:
        proof = ctx.prove_bn254(pk, w, cap=1 << 25)[0]
        ok, why, claims = hg.verify_public_bn254(pk, hg.Instance.from_witness(w), proof, ctx=ctx, device=True)
        cm = hg.Commitment.secrets_bn254(ctx, bfv.params, w) if ok else None
        verify, verify_folded, cls = hg.claims_verify_bn254, hg.claims_verify_folded_bn254, "pcs_fold_bn254"
    else:
        proof, _ = bfv.prove(ctx, pk, w, cap=1 << 25)
        ok, why, claims = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 0, ctx=ctx, device=True)
        cm = hg.Commitment.secrets(ctx, bfv.params, w) if ok else None
        verify, verify_folded, cls = hg.claims_verify, hg.claims_verify_folded, "pcs_fold"
    assert ok, why
    params, root = bfv.params, cm.root
    plain, folded = cm.open_claims(params, claims), cm.open_claims_folded(params, claims)
    pairs = [("open", lambda: cm.open_claims(params, claims), lambda: cm.open_claims_folded(params, claims)),
             ("verify_dev", lambda: verify(params, root, claims, plain, ctx=ctx), lambda: verify_folded(params, root, claims, folded, ctx=ctx)),
             ("verify_host", lambda: verify(params, root, claims, plain), lambda: verify_folded(params, root, claims, folded))]
    legs = [(name + sfx, fn) for name, f0, f1 in pairs for sfx, fn in (("", f0), ("_folded", f1))]
    times = {name: [] for name, _ in legs}
    for rep in range(a.reps + 1):   # rep 0: the warm-up call of each leg
        for name, fn in legs:
            t0 = time.perf_counter()
            out = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if name.startswith("verify"):
                assert out == (True, ""), out
            else:
                assert out == (folded if name.endswith("_folded") else plain)
            if rep:
                times[name].append(dt)
    print("%sn=%d k=%d: %d tables, log2_row %d, %d rows; %d claims, 241 queries, opening %d bytes, folded %d bytes; legs alternated, %d timed calls each after "
          "one warm-up call, one process" % ("bn254 " if a.bn254 else "", a.n, a.k, len(cm.nvars), cm.log2_row, sum(1 << (v - cm.log2_row) for v in cm.nvars), claims.n, len(plain), len(folded), a.reps))
    for name, _ in legs:
        t = times[name]
        print("%-19s median %.2f ms, range %.2f .. %.2f ms (%s)" % (name, statistics.median(t), min(t), max(t), " ".join("%.2f" % x for x in t)))
    for name, _, _ in pairs:
        new, old = times[name + "_folded"], times[name]
        if max(new) < min(old):
            print("%s_folded is faster than %s: its whole range lies below the unfolded form's" % (name, name))
        elif min(new) > max(old):
            print("%s_folded is SLOWER than %s: its whole range lies above the unfolded form's" % (name, name))
        else:
            print("%s_folded and %s overlap: no difference shown" % (name, name))
    ctx.profile(2)   # one more folded open with every launch class timed by events
    ctx.profile_reset()
    assert cm.open_claims_folded(params, claims) == folded
    for st in ctx.profile_get(256):
        if st["name"] == cls:
            print("%-14s %3d launches %8.3f ms  %7.1f MB by the algorithm" % (st["name"], st["launches"], st["total_ms"], st["algo_bytes"] / 1e6))
    ctx.profile(0)
    cm.free()
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
