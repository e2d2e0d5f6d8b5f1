#!/usr/bin/env python3
"""Times of the polynomial commitment over the secret inputs, device form against host form (ctx == NULL), in one process: the legs
ALTERNATED on one synthetic witness and the claims hg_verify_public_device leaves on its hg_prove proof, after one warm-up call of
each leg, --reps timed calls each:
  commit_dev / commit_host   hg_secrets_commit with a context / without (upload or copy of the tables, encoding, column hashes, tree)
  open_dev / open_host       hg_claims_open of those claims on the commitment of that form (default 241 queries)
  verify_dev / verify_host   hg_claims_verify_device / hg_claims_verify of the opening: the whole call, upload included
Prints the opening's bytes, median and range per leg, and for the commit and the verify pair (over BN254 the open pair too) whether the
whole range of the device form lies below that of the host form.
--field bn254 times the BN254 commitment on the claims hg_verify_public_device_bn254 leaves on an hg_prove_bn254 proof: the same three
pairs (verify_dev is hg_claims_verify_device_bn254), then one more device commit, open and verification under hg_profile for the kernel
time by class.
Usage: pcs_times.py [n k] [--reps 5] [--field goldilocks|bn254]"""
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
    ap.add_argument("--field", choices=["goldilocks", "bn254"], default="goldilocks")
    a = ap.parse_args()
    bn = a.field == "bn254"
    ctx = hg.Context(0)
    bfv = hg.BfvEncrypt.new(a.n, a.k)
    pk = bfv.setup(ctx)
    w = hg.Witness.synthetic(bfv.params, 0x4752454330 + a.n)
    if bn:
        proof = ctx.prove_bn254(pk, w, cap=1 << 25)[0]
        ok, why, claims = hg.verify_public_bn254(pk, hg.Instance.from_witness(w), proof, ctx=ctx, device=True)
    else:
        proof, _ = bfv.prove(ctx, pk, w, cap=1 << 25)
        ok, why, claims = hg.verify_public(pk, hg.Instance.from_witness(w), proof, 0, ctx=ctx, device=True)
    assert ok, why
    secrets = hg.Commitment.secrets_bn254 if bn else hg.Commitment.secrets
    verify = hg.claims_verify_bn254 if bn else hg.claims_verify
    held = {"dev": secrets(ctx, bfv.params, w), "host": secrets(None, bfv.params, w)}
    assert held["dev"].root == held["host"].root
    opening = held["dev"].open_claims(bfv.params, claims)
    assert opening == held["host"].open_claims(bfv.params, claims)

    def commit(form):
        held[form].free()
        held[form] = secrets(ctx if form == "dev" else None, bfv.params, w)

    legs = [("commit_dev", lambda: commit("dev")), ("commit_host", lambda: commit("host")),
            ("open_dev", lambda: held["dev"].open_claims(bfv.params, claims)), ("open_host", lambda: held["host"].open_claims(bfv.params, claims)),
            ("verify_dev", lambda: verify(bfv.params, held["host"].root, claims, opening, ctx=ctx)),
            ("verify_host", lambda: verify(bfv.params, held["host"].root, claims, opening))]
    times = {name: [] for name, _ in legs}
    for rep in range(a.reps + 1):   # rep 0: the warm-up call of each leg
        for name, fn in legs:
            t0 = time.perf_counter()
            out = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if name.startswith("verify"):
                assert out == (True, ""), out
            if rep:
                times[name].append(dt)
    c = held["dev"]
    print("field %s" % a.field)
    print("n=%d k=%d: %d tables, log2_row %d, %d rows, code length %d; %d claims, 241 queries, opening %d bytes; legs alternated, %d timed calls each "
          "after one warm-up call, one process" % (a.n, a.k, len(c.nvars), c.log2_row, sum(1 << (v - c.log2_row) for v in c.nvars), 4 << c.log2_row, claims.n,
                                                   len(opening), a.reps))
    for name, _ in legs:
        t = times[name]
        print("%-11s median %.2f ms, range %.2f .. %.2f ms (%s)" % (name, statistics.median(t), min(t), max(t), " ".join("%.2f" % x for x in t)))
    for leg in ("commit", "open", "verify") if bn else ("commit", "verify"):
        dev, host = times[leg + "_dev"], times[leg + "_host"]
        if max(dev) < min(host):
            print("%s_dev is faster than %s_host: its whole range lies below the host form's" % (leg, leg))
        elif min(dev) > max(host):
            print("%s_dev is SLOWER than %s_host: its whole range lies above the host form's" % (leg, leg))
        else:
            print("%s_dev and %s_host overlap: no difference shown" % (leg, leg))
    if bn:   # one more device commit, open and verification with every launch class timed by events
        ctx.profile(2)
        ctx.profile_reset()
        commit("dev")
        held["dev"].open_claims(bfv.params, claims)
        assert verify(bfv.params, held["host"].root, claims, opening, ctx=ctx) == (True, "")
        for st in ctx.profile_get(256):
            if st["name"].startswith("pcs_bn254"):
                print("%-18s %2d launches %8.3f ms  %7.1f MB by the algorithm" % (st["name"], st["launches"], st["total_ms"], st["algo_bytes"] / 1e6))
        ctx.profile(0)
    for h in held.values():
        h.free()
    pk.free()
    ctx.close()


if __name__ == "__main__":
    main()
