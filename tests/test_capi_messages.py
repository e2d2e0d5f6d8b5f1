"""The argument checks of the two-field C ABI layer (capi.hip: the verifier batches, hg_verify_public*, hg_claims_settle*,
hg_instance_mle*, and the commitment layer hg_pcs_open* .. hg_claims_verify*), pinned row by row: for a table of bad and edge
calls the return code, the full hg_last_error() text where the code is non-zero, whether outputs prefilled with a pattern were left
alone, and a digest of those outputs. tests/golden/capi_messages.json holds what the library gave when the table was recorded;
the test replays the table and compares for equality. Checks, their order and their messages are part of the interface.

Recording (only ever against a library whose behaviour is the one to pin): HG_CAPI_RECORD=<file> python tests/test_capi_messages.py [cpu|gpu]
writes the rows of that part."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from hglib import hg, ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_messages.json")
P = hg.P
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # the order of bn256::Fr
MAX_CLAIMS, MAX_QUERIES = 4096, 65536
PAT = b"\x55"
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int

_L = None


def L():
    """a handle of the library of its own: the prototypes below are this test's, whatever the package assigns"""
    global _L
    if _L is None:
        hg.lib()
        _L = C.CDLL(hg._LIB_PATH)
        _L.hg_last_error.restype = C.c_char_p
    return _L


def call(name, types, *args):
    f = getattr(L(), name)
    f.argtypes, f.restype = list(types), C.c_int
    return f(*args)


class Out:
    """an output prefilled with the pattern; handle: the function that frees the handles (void*) the call may set here, which are
    recorded as set / null / untouched, and freed"""

    def __init__(self, nbytes, handle=None):
        self.n, self.handle = max(int(nbytes), 1), handle
        self.buf = (C.c_uint8 * self.n).from_buffer_copy(PAT * self.n)

    def untouched(self):
        return bytes(self.buf) == PAT * self.n

    def digest_bytes(self):
        if not self.handle or self.untouched():
            return bytes(self.buf)
        hs = C.cast(self.buf, C.POINTER(C.c_void_p))[:self.n // 8]
        for h in hs:
            if h:
                f = getattr(L(), self.handle)
                f.argtypes, f.restype = [vp], None
                f(h)
        return b",".join(b"handle set" if h else b"handle null" for h in hs)


def row(rc, outs, counts=False):
    """counts: the entry returns how many items it rejected or refused, and only a negative code leaves a text for hg_last_error()"""
    r = {"rc": rc}
    if rc < 0 or (rc != 0 and not counts):
        r["error"] = L().hg_last_error().decode()
    r["untouched"] = all(o.untouched() for o in outs)
    r["outputs"] = hashlib.sha256(b"|".join(o.digest_bytes() for o in outs)).hexdigest()[:16]
    return r


class Field:
    def __init__(self, bn):
        self.bn, self.W, self.sfx = bn, 4 if bn else 2, "_bn254" if bn else ""
        self.claim_bytes = 16 + 8 * self.W

    def words(self, v):
        """a small non-negative integer, or None for a non-canonical element, as the words that cross the ABI"""
        if v is None:
            v = R if self.bn else P          # (Goldilocks: first word p, second 0)
        return [(v >> (64 * i)) & (2**64 - 1) for i in range(self.W)] if self.bn else [v, 0]

    def lift(self, word):
        """a table word as an element: over Fr by the signed rule"""
        w = int(word)
        return w if not self.bn or w < P // 2 else (w - P) % R

    def flat(self, elems):
        return np.array([x for e in elems for x in self.words(e)] or [0], dtype=np.uint64)

    def claims(self, cl):
        """[(input, nvars, point_off, value)] -> bytes of an hg_input_claim array"""
        b = b""
        for inp, nv, off, val in cl:
            b += np.array([inp, nv], dtype=np.uint32).tobytes() + np.array([off] + self.words(val), dtype=np.uint64).tobytes()
        return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")


GL, BN = Field(False), Field(True)


def arr(t, vals):
    return (t * max(len(vals), 1))(*vals)


def drop(a, names):
    for d in names:
        assert d in a, d
        a[d] = None
    return a


class Env:
    """n = 1024, k = 1: a witness, its instance, the same of (2048, 1), a host-only key; with a device: two contexts, a device key,
    one proof per field"""

    def __init__(self, gpu):
        self.bfv = hg.BfvEncrypt.new(1024, 1)
        self.params, self.other_params = self.bfv.params, hg.params_builtin(2048, 1)
        self.k, self.nv = 1, 11                              # 11 variables: s, e, k1, ais[0], r1is[0] (2n words); r2is has 10, ct0is 11
        self.w, self.w_other = hg.Witness.synthetic(self.params, 0xca91), hg.Witness.synthetic(self.other_params, 0xca92)
        self.inst, self.inst_other = hg.Instance.from_witness(self.w), hg.Instance.from_witness(self.w_other)
        self.host_pk = self.bfv.setup(None)
        self.nc, self.nco = hg.pk_claim_shape(self.host_pk)
        self.s0 = int(self.w.arrays()["s"][0])
        self.garbage = bytes(range(256)) * 16
        self.ctx = self.ctx2 = self.pk = None
        self.proofs = {False: self.garbage, True: self.garbage}
        self.real = False
        if gpu:
            self.ctx, self.ctx2 = hg.Context(0), hg.Context(0)
            self.pk = self.bfv.setup(self.ctx)
            self.proofs = {False: self.bfv.prove(self.ctx, self.pk, self.w)[0], True: self.ctx.prove_bn254(self.pk, self.w)[0]}
            self.real = True
        self._cm = {}

    def close(self):
        for cm in self._cm.values():
            call("hg_pcs_free", [vp], cm)
        if self.pk:
            self.pk.free()
        self.host_pk.free()
        for c in (self.ctx, self.ctx2):
            if c:
                c.close()

    def h(self, ctx):
        return ctx.h if ctx is not None else None

    # commitments, made once: ("tables" | "secrets", field, context)
    TABLE_NVARS = [4, 5]

    def commitment(self, kind, F, ctx=None):
        key = (kind, F.bn, id(ctx) if ctx is not None else 0)
        if key not in self._cm:
            h, root = C.c_void_p(), (C.c_uint8 * 32)()
            if kind == "tables":
                tabs = [F.flat([(7 * i + 3 * t) % 1000 for i in range(1 << v)]) if F.bn else np.array([(7 * i + 3 * t) % 1000 for i in range(1 << v)], dtype=np.uint64)
                        for t, v in enumerate(self.TABLE_NVARS)]
                self._keep = getattr(self, "_keep", []) + tabs
                rc = call("hg_pcs_commit" + F.sfx, [vp, vp, vp, sz, sz, vp, vp], self.h(ctx), arr(C.c_void_p, [t.ctypes.data for t in tabs]),
                          arr(C.c_uint32, self.TABLE_NVARS), 2, 2, C.byref(h), root)
            else:
                rc = call("hg_secrets_commit" + F.sfx, [vp, vp, vp, sz, vp, vp], self.h(ctx), C.byref(self.params), self.w.h, 0, C.byref(h), root)
            assert rc == 0, L().hg_last_error()
            self._cm[key] = h.value
            self._cm_root = getattr(self, "_cm_root", {})
            self._cm_root[key] = bytes(root)
        return self._cm[key], self._cm_root[key]

    def table_value(self, t):
        return (3 * t) % 1000                                # word 0 of table t: its MLE at the all-zero point


# ---- the entry families: each takes the good arguments, changed by keyword, and returns a row -------------------------------------
def verify_device_batch(E, F, ctx, pk, hs=None, proofs=None, n=None, mode=0, rcap=64, nulls=()):
    hs = [E.w.h.value] * 2 if hs is None else hs
    proofs = [E.proofs[F.bn], E.garbage] if proofs is None else proofs
    n = len(proofs) if n is None else n
    m = max(len(proofs), 1)
    res, reasons = Out(4 * m), Out(m * rcap)
    a = drop(dict(ws=arr(C.c_void_p, hs), proofs=arr(C.c_char_p, proofs), lens=arr(C.c_size_t, [len(p) if p else 0 for p in proofs]), results=res.buf,
                  reasons=reasons.buf), nulls)
    mid = ([ci], [mode]) if not F.bn else ([], [])
    rc = call("hg_verify_device_batch" + F.sfx, [vp, vp, vp, vp, vp, sz] + mid[0] + [vp, vp, sz],
              E.h(ctx), pk.h if pk else None, a["ws"], a["proofs"], a["lens"], n, *mid[1], a["results"], a["reasons"], rcap)
    return row(rc, [res, reasons], counts=True)


def verify_public(E, F, device, ctx, pk, inst="own", mode=0, proof=None, caps=None, nulls=()):
    proof = E.proofs[F.bn] if proof is None else proof
    nc, nco = caps or (E.nc, E.nco)
    claims, points, cnt = Out(E.nc * F.claim_bytes), Out(E.nco * 8 * F.W), Out(8)
    a = drop(dict(instance=E.inst.h if inst == "own" else inst, proof=proof, claims=claims.buf, points=points.buf, n_claims=cnt.buf), nulls)
    mid = ([ci], [mode]) if not F.bn else ([], [])
    head = ([vp], [E.h(ctx)]) if device else ([], [])
    rc = call("hg_verify_public" + ("_device" if device else "") + F.sfx, head[0] + [vp, vp] + mid[0] + [C.c_char_p, sz, vp, sz, vp, sz, vp],
              *head[1], pk.h if pk else None, a["instance"], *mid[1], a["proof"], len(proof), a["claims"], nc, a["points"], nco, a["n_claims"])
    return row(rc, [claims, points, cnt])


def verify_public_batch(E, F, ctx, pk, hs=None, proofs=None, n=None, mode=0, caps=None, rcap=64, nulls=()):
    hs = [E.inst.h.value] * 2 if hs is None else hs
    proofs = [E.proofs[F.bn], E.garbage] if proofs is None else proofs
    n = len(proofs) if n is None else n
    m = max(len(proofs), 1)
    nc, nco = caps or (E.nc, E.nco)
    res, claims, points, cnt, reasons = Out(4 * m), Out(m * E.nc * F.claim_bytes), Out(m * E.nco * 8 * F.W), Out(8 * m), Out(m * rcap)
    a = drop(dict(instances=arr(C.c_void_p, hs), proofs=arr(C.c_char_p, proofs), lens=arr(C.c_size_t, [len(p) if p else 0 for p in proofs]), results=res.buf,
                  claims=claims.buf, points=points.buf, n_claims=cnt.buf, reasons=reasons.buf), nulls)
    mid = ([ci], [mode]) if not F.bn else ([], [])
    rc = call("hg_verify_public_batch" + F.sfx, [vp, vp, vp, vp, vp, sz] + mid[0] + [vp, vp, sz, vp, sz, vp, vp, sz],
              E.h(ctx), pk.h if pk else None, a["instances"], a["proofs"], a["lens"], n, *mid[1], a["results"], a["claims"], nc, a["points"], nco,
              a["n_claims"], a["reasons"], rcap)
    return row(rc, [res, claims, points, cnt, reasons], counts=True)


def good_claim(E, F, value=...):
    """input 0 (s) at the all-zero point is word 0 of the table; value None: a non-canonical one"""
    return [(0, E.nv, 0, F.lift(E.s0) if value is ... else value)], [0] * E.nv


def claims_settle(E, F, ctx, params="own", w="own", cl=None, pts=None, n=None, nulls=()):
    c0, p0 = good_claim(E, F)
    cl, pts = c0 if cl is None else cl, p0 if pts is None else pts
    points = F.flat(pts)
    a = drop(dict(params=C.byref(E.params) if params == "own" else params, w=E.w.h if w == "own" else w, claims=F.claims(cl), points=points.ctypes.data), nulls)
    rc = call("hg_claims_settle" + F.sfx, [vp, vp, vp, vp, sz, vp], E.h(ctx), a["params"], a["w"], a["claims"], len(cl) if n is None else n, a["points"])
    return row(rc, [])


def instance_mle(E, F, ctx, which=0, index=0, pts=None, nvars=None, nulls=()):
    pts = [5] * E.nv if pts is None else pts
    point, out = F.flat(pts), Out(8 * F.W)
    a = drop(dict(instance=E.inst.h, point=point.ctypes.data, out=out.buf), nulls)
    rc = call("hg_instance_mle" + F.sfx, [vp, vp, ci, ci, vp, sz, vp], E.h(ctx), a["instance"], which, index, a["point"], len(pts) if nvars is None else nvars, a["out"])
    return row(rc, [out])


def instance_mle_batch(E, F, ctx, hs=None, n=None, which=0, index=0, pts=None, nvars=None, nulls=()):
    hs = [E.inst.h.value] * 2 if hs is None else hs
    pts = [5] * E.nv if pts is None else pts
    point, out = F.flat(pts), Out(8 * F.W * max(len(hs), 1))
    a = drop(dict(instances=arr(C.c_void_p, hs), point=point.ctypes.data, out=out.buf), nulls)
    rc = call("hg_instance_mle_batch" + F.sfx, [vp, vp, sz, ci, ci, vp, sz, vp], E.h(ctx), a["instances"], len(hs) if n is None else n, which, index, a["point"],
              len(pts) if nvars is None else nvars, a["out"])
    return row(rc, [out])


def table_claims(E, F, cl):
    """[(table, point elements, value)] -> the three arrays"""
    return arr(C.c_uint32, [c[0] for c in cl]), F.flat([x for c in cl for x in c[1]]), F.flat([c[2] for c in cl])


def good_table_claims(E):
    return [(t, [0] * v, E.table_value(t)) for t, v in enumerate(E.TABLE_NVARS)]


def pcs_open(E, F, ctx, cm, cl=None, n=None, nq=3, cap=1 << 16, nulls=()):
    cl = good_table_claims(E) if cl is None else cl
    table, pts, vals = table_claims(E, F, cl)
    proof, ln = Out(cap), Out(8)
    a = drop(dict(commitment=cm, table=table, points=pts.ctypes.data, values=vals.ctypes.data, proof=proof.buf, len=ln.buf), nulls)
    rc = call("hg_pcs_open" + F.sfx, [vp, vp, vp, vp, vp, sz, sz, vp, sz, vp], E.h(ctx), a["commitment"], a["table"], a["points"], a["values"],
              len(cl) if n is None else n, nq, a["proof"], cap, a["len"])
    r = row(rc, [proof, ln])
    r["_bytes"] = bytes(proof.buf)[:int.from_bytes(bytes(ln.buf), "little")] if rc == 0 else b""
    return r


def pcs_verify(E, F, device, ctx, root, proof, nvars=None, n_tables=None, log2_row=2, cl=None, n=None, nq=3, nulls=()):
    cl = good_table_claims(E) if cl is None else cl
    nvars = E.TABLE_NVARS if nvars is None else nvars
    table, pts, vals = table_claims(E, F, cl)
    a = drop(dict(root=root, nvars=arr(C.c_uint32, nvars), table=table, points=pts.ctypes.data, values=vals.ctypes.data, proof=proof), nulls)
    head = ([vp], [E.h(ctx)]) if device else ([], [])
    rc = call("hg_pcs_verify" + ("_device" if device else "") + F.sfx, head[0] + [C.c_char_p, vp, sz, sz, vp, vp, vp, sz, sz, C.c_char_p, sz],
              *head[1], a["root"], a["nvars"], len(nvars) if n_tables is None else n_tables, log2_row, a["table"], a["points"], a["values"],
              len(cl) if n is None else n, nq, a["proof"], len(proof))
    return row(rc, [])


def secrets_commit(E, F, ctx, params="own", w="own", log2_row=0, nulls=()):
    cm, root = Out(8, handle="hg_pcs_free"), Out(32)
    a = drop(dict(params=C.byref(E.params) if params == "own" else params, w=E.w.h if w == "own" else w, commitment=cm.buf, root=root.buf), nulls)
    rc = call("hg_secrets_commit" + F.sfx, [vp, vp, vp, sz, vp, vp], E.h(ctx), a["params"], a["w"], log2_row, a["commitment"], a["root"])
    return row(rc, [cm, root])


def claims_open(E, F, ctx, cm, params="own", cl=None, pts=None, n=None, nq=3, cap=1 << 17, nulls=()):
    c0, p0 = good_claim(E, F)
    cl, pts = c0 if cl is None else cl, p0 if pts is None else pts
    points = F.flat(pts)
    opening, ln = Out(cap), Out(8)
    a = drop(dict(params=C.byref(E.params) if params == "own" else params, commitment=cm, claims=F.claims(cl), points=points.ctypes.data, opening=opening.buf,
                  len=ln.buf), nulls)
    rc = call("hg_claims_open" + F.sfx, [vp, vp, vp, vp, sz, vp, sz, vp, sz, vp], E.h(ctx), a["params"], a["commitment"], a["claims"], len(cl) if n is None else n,
              a["points"], nq, a["opening"], cap, a["len"])
    r = row(rc, [opening, ln])
    r["_bytes"] = bytes(opening.buf)[:int.from_bytes(bytes(ln.buf), "little")] if rc == 0 else b""
    return r


def claims_verify(E, F, device, ctx, root, opening, params="own", log2_row=0, cl=None, pts=None, n=None, nq=3, nulls=()):
    c0, p0 = good_claim(E, F)
    cl, pts = c0 if cl is None else cl, p0 if pts is None else pts
    points = F.flat(pts)
    a = drop(dict(params=C.byref(E.params) if params == "own" else params, root=root, claims=F.claims(cl), points=points.ctypes.data, opening=opening), nulls)
    head = ([vp], [E.h(ctx)]) if device else ([], [])
    rc = call("hg_claims_verify" + ("_device" if device else "") + F.sfx, head[0] + [vp, C.c_char_p, sz, vp, sz, vp, sz, C.c_char_p, sz],
              *head[1], a["params"], a["root"], log2_row, a["claims"], len(cl) if n is None else n, a["points"], nq, a["opening"], len(opening))
    return row(rc, [])


def prove_encryptions(E, F, ctx, pk, n=2, cap=None, rcap=64, null_poly=False, ws=True, nulls=()):
    """n encryptions under the key: signed polynomials of small coefficients; timings are not asked for"""
    N, m = int(E.params.n), max(n, 1)
    polys = [np.array([(i % 3) - 1 for i in range(N)], dtype=np.int64), np.array([(i % 5) - 2 for i in range(N)], dtype=np.int64),
             np.array([i % 7 for i in range(N)], dtype=np.int64), np.array([(i * 31) % 1000 for i in range(E.k * N)], dtype=np.int64)]
    cols = [arr(C.c_void_p, [x.ctypes.data] * m) for x in polys]
    if null_poly:
        cols[2][m - 1] = None
    cap = len(E.proofs[F.bn]) + 64 if cap is None else cap
    proofs, lens, status, hs, reasons = Out(m * cap), Out(8 * m), Out(4 * m), Out(8 * m, handle="hg_witness_free"), Out(m * rcap)
    a = drop(dict(s=cols[0], e=cols[1], k1=cols[2], a=cols[3], proofs=proofs.buf, lens=lens.buf, status=status.buf, ws=hs.buf if ws else None, reasons=reasons.buf), nulls)
    rc = call("hg_prove_encryptions" + F.sfx, [vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, vp], E.h(ctx), pk.h if pk else None, a["s"], a["e"], a["k1"], a["a"], n,
              a["proofs"], cap, a["lens"], a["status"], a["ws"], a["reasons"], rcap, None)
    return row(rc, [proofs, lens, status, hs, reasons], counts=True)


# ---- the table -------------------------------------------------------------------------------------------------------------------
def table(E, gpu):
    """[(row id, row)]: the CPU part needs no device (host forms, and every check that fires before the context is used); the GPU
    part has a live context, a device key and one real proof per field"""
    rows = []

    def add(name, thunk):
        r = thunk()                                          # (at once: the thunks close over the loop's variables)
        r.pop("_bytes", None)
        rows.append((name, r))

    for F in (GL, BN):
        own, oth = E.inst.h.value, E.inst_other.h.value
        wo, wt = E.w.h.value, E.w_other.h.value
        vdb, vpub, vpb, st, mle, mleb = ("hg_verify_device_batch", "hg_verify_public", "hg_verify_public_batch", "hg_claims_settle", "hg_instance_mle",
                                          "hg_instance_mle_batch")
        po, pv, sc, co, cv = "hg_pcs_open", "hg_pcs_verify", "hg_secrets_commit", "hg_claims_open", "hg_claims_verify"
        s = F.sfx
        two_claims = [(0, E.nv, 0, F.lift(E.s0)), (1, E.nv, E.nv, 1)]
        many = [(0, [], 0)] * (MAX_CLAIMS + 1)
        many_in = [(0, E.nv, 0, 0)] * (MAX_CLAIMS + 1)
        if not gpu:
            hp = E.host_pk
            add(f"{vdb}{s}: no context", lambda F=F: verify_device_batch(E, F, None, hp))
            add(f"{vdb}{s}: no context, n == 0", lambda F=F: verify_device_batch(E, F, None, hp, hs=[], proofs=[]))
            add(f"{vpb}{s}: no context", lambda F=F: verify_public_batch(E, F, None, hp))
            add(f"{vpb}{s}: no context, n == 0", lambda F=F: verify_public_batch(E, F, None, hp, hs=[], proofs=[]))
            add(f"{mleb}{s}: no context", lambda F=F: instance_mle_batch(E, F, None))
            add(f"hg_prove_encryptions{s}: no context", lambda F=F: prove_encryptions(E, F, None, hp, cap=64))
            add(f"hg_prove_encryptions{s}: no context, no key, no arrays", lambda F=F: prove_encryptions(E, F, None, None, cap=64, nulls=("s", "proofs", "status")))
            add(f"{vpub}_device{s}: no context", lambda F=F: verify_public(E, F, True, None, hp))
            add(f"{vpub}_device{s}: null n_claims and no context", lambda F=F: verify_public(E, F, True, None, hp, nulls=("n_claims",)))
            # hg_verify_public*: the host walk
            add(f"{vpub}{s}: null key", lambda F=F: verify_public(E, F, False, None, None))
            for d in ("instance", "proof", "n_claims", "claims", "points"):
                add(f"{vpub}{s}: null {d}", lambda F=F, d=d: verify_public(E, F, False, None, hp, nulls=(d,)))
            if not F.bn:
                add(f"{vpub}: mode 4", lambda F=F: verify_public(E, F, False, None, hp, mode=4))
                add(f"{vpub}: mode -1", lambda F=F: verify_public(E, F, False, None, hp, mode=-1))
                add(f"{vpub}: mode 3, a proof that is not one", lambda F=F: verify_public(E, F, False, None, hp, mode=3))
            add(f"{vpub}{s}: instance of other parameters", lambda F=F: verify_public(E, F, False, None, hp, inst=E.inst_other.h))
            add(f"{vpub}{s}: claim capacity one too small", lambda F=F: verify_public(E, F, False, None, hp, caps=(E.nc - 1, E.nco)))
            add(f"{vpub}{s}: coordinate capacity one too small", lambda F=F: verify_public(E, F, False, None, hp, caps=(E.nc, E.nco - 1)))
            add(f"{vpub}{s}: a proof that is not one", lambda F=F: verify_public(E, F, False, None, hp))
            add(f"{vpub}{s}: an empty proof", lambda F=F: verify_public(E, F, False, None, hp, proof=b""))
        ctxs = [None] if not gpu else [E.ctx]
        for ctx in ctxs:
            # hg_claims_settle*, hg_instance_mle*: host form without a context, device form with one
            where = "device" if ctx else "host"
            add(f"{st}{s} ({where}): a claim that holds", lambda F=F, ctx=ctx: claims_settle(E, F, ctx))
            add(f"{st}{s} ({where}): a claim with another value", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=good_claim(E, F, 12345)[0]))
            add(f"{st}{s} ({where}): two claims", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=two_claims, pts=[0] * E.nv + [1] * E.nv))
            add(f"{st}{s} ({where}): n == 0 and no arrays", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=[], nulls=("claims", "points")))
            for d in ("params", "w", "claims", "points"):
                add(f"{st}{s} ({where}): null {d}", lambda F=F, ctx=ctx, d=d: claims_settle(E, F, ctx, nulls=(d,)))
            add(f"{st}{s} ({where}): witness of other parameters", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, w=E.w_other.h))
            add(f"{st}{s} ({where}): parameters other than the witness's", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, params=C.byref(E.other_params)))
            add(f"{st}{s} ({where}): input id 3 + 2k + 1", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=[(3 + 2 * E.k + 1, E.nv, 0, 0)]))
            add(f"{st}{s} ({where}): input id 3 + 2k (r2is) with the variables of s", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=[(3 + 2 * E.k, E.nv, 0, 0)]))
            add(f"{st}{s} ({where}): nvars 41", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=[(0, 41, 0, 0)], pts=[0] * 41))
            add(f"{st}{s} ({where}): nvars 41 on a bad input id", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=[(99, 41, 0, 0)], pts=[0] * 41))
            add(f"{st}{s} ({where}): non-canonical coordinate", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, pts=[0] * (E.nv - 1) + [None]))
            add(f"{st}{s} ({where}): non-canonical value", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=good_claim(E, F, None)[0]))
            add(f"{st}{s} ({where}): non-canonical coordinate and value", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=good_claim(E, F, None)[0], pts=[None] + [0] * (E.nv - 1)))
            add(f"{st}{s} ({where}): bad second claim", lambda F=F, ctx=ctx: claims_settle(E, F, ctx, cl=[two_claims[0], (7, E.nv, E.nv, 1)], pts=[0] * (2 * E.nv)))
            add(f"{mle}{s} ({where}): ais[0]", lambda F=F, ctx=ctx: instance_mle(E, F, ctx))
            add(f"{mle}{s} ({where}): ct0is", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, which=1, index=9))
            add(f"{mle}{s} ({where}): ais[0] at a 0/1 point", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, pts=[1, 0] * 5 + [1]))
            for d in ("instance", "point", "out"):
                add(f"{mle}{s} ({where}): null {d}", lambda F=F, ctx=ctx, d=d: instance_mle(E, F, ctx, nulls=(d,)))
            add(f"{mle}{s} ({where}): selector 2", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, which=2))
            add(f"{mle}{s} ({where}): selector -1", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, which=-1))
            add(f"{mle}{s} ({where}): modulus index k", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, index=E.k))
            add(f"{mle}{s} ({where}): modulus index -1", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, index=-1))
            add(f"{mle}{s} ({where}): one variable short", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, pts=[5] * (E.nv - 1)))
            add(f"{mle}{s} ({where}): one variable more, ct0is", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, which=1, pts=[5] * (E.nv + 1)))
            add(f"{mle}{s} ({where}): selector 2 and one variable short", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, which=2, pts=[5] * (E.nv - 1)))
            add(f"{mle}{s} ({where}): non-canonical coordinate", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, pts=[5] * (E.nv - 1) + [None]))
            add(f"{mle}{s} ({where}): one variable short and non-canonical", lambda F=F, ctx=ctx: instance_mle(E, F, ctx, pts=[5] * (E.nv - 2) + [None]))

            # the commitment layer: host form without a context, device form with one
            def opened(F=F, ctx=ctx):
                cm, root = E.commitment("tables", F, ctx)
                return root, pcs_open(E, F, ctx, cm)["_bytes"]

            def sopened(F=F, ctx=ctx):
                cm, root = E.commitment("secrets", F, ctx)
                return root, claims_open(E, F, ctx, cm)["_bytes"]

            def tampered(b):
                return b[:40] + bytes([b[40] ^ 1]) + b[41:]
            cmt = lambda F=F, ctx=ctx: E.commitment("tables", F, ctx)[0]      # noqa: E731
            cms = lambda F=F, ctx=ctx: E.commitment("secrets", F, ctx)[0]     # noqa: E731
            other_field = BN if not F.bn else GL
            add(f"{po}{s} ({where}): two claims that hold", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt()))
            add(f"{po}{s} ({where}): no claims", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cl=[], nulls=("table", "points", "values")))
            add(f"{po}{s} ({where}): default queries", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), nq=0))
            add(f"{po}{s} ({where}): a claim that does not hold", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cl=[(0, [0] * 4, 77)]))
            for d in ("commitment", "proof", "len", "table", "points", "values"):
                add(f"{po}{s} ({where}): null {d}", lambda F=F, ctx=ctx, d=d: pcs_open(E, F, ctx, cmt(), nulls=(d,)))
            add(f"{po}{s} ({where}): commitment of the other field", lambda F=F, ctx=ctx, G=other_field: pcs_open(E, F, ctx, E.commitment("tables", G, ctx)[0]))
            add(f"{po}{s} ({where}): MAX_CLAIMS + 1 claims", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cl=many))
            add(f"{po}{s} ({where}): table index out of range", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cl=[good_table_claims(E)[0], (2, [], 0)]))
            add(f"{po}{s} ({where}): non-canonical coordinate", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cl=[(0, [0, 0, None, 0], 0)]))
            add(f"{po}{s} ({where}): non-canonical value", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cl=[(0, [0] * 4, None)]))
            add(f"{po}{s} ({where}): non-canonical value in claim 1 and MAX_QUERIES + 1", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cl=[good_table_claims(E)[0], (1, [0] * 5, None)], nq=MAX_QUERIES + 1))
            add(f"{po}{s} ({where}): MAX_QUERIES + 1 queries", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), nq=MAX_QUERIES + 1))
            add(f"{po}{s} ({where}): buffer one byte short", lambda F=F, ctx=ctx: pcs_open(E, F, ctx, cmt(), cap=len(opened(F, ctx)[1]) - 1))
            add(f"{pv}{s} ({where}): an opening that verifies", lambda F=F, ctx=ctx: pcs_verify(E, F, False, None, *opened(F, ctx)))
            add(f"{pv}{s} ({where}): a tampered opening", lambda F=F, ctx=ctx: pcs_verify(E, F, False, None, opened(F, ctx)[0], tampered(opened(F, ctx)[1])))
            add(f"{pv}{s} ({where}): another root", lambda F=F, ctx=ctx: pcs_verify(E, F, False, None, bytes(32), opened(F, ctx)[1]))
            if not ctx:
                g = b"\x01" * 64
                for d in ("root", "nvars", "proof", "table", "points", "values"):
                    add(f"{pv}{s}: null {d}", lambda F=F, d=d: pcs_verify(E, F, False, None, bytes(32), g, nulls=(d,)))
                add(f"{pv}{s}: no tables", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, n_tables=0))
                add(f"{pv}{s}: log2_row above a table", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, log2_row=5))
                add(f"{pv}{s}: MAX_CLAIMS + 1 claims", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, cl=many))
                add(f"{pv}{s}: table index out of range", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, cl=[(2, [], 0)]))
                add(f"{pv}{s}: non-canonical coordinate", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, cl=[(1, [None] + [0] * 4, 0)]))
                add(f"{pv}{s}: non-canonical value", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, cl=[(1, [0] * 5, None)]))
                add(f"{pv}{s}: MAX_QUERIES + 1 queries", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, nq=MAX_QUERIES + 1))
                add(f"{pv}{s}: bad shape and bad claim", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g, log2_row=5, cl=[(2, [], 0)]))
                add(f"{pv}{s}: an opening of the wrong length", lambda F=F: pcs_verify(E, F, False, None, bytes(32), g))
                add(f"{pv}{s}: an empty opening, null", lambda F=F: pcs_verify(E, F, False, None, bytes(32), b"", nulls=("proof",)))
            add(f"{sc}{s} ({where}): the five secret inputs", lambda F=F, ctx=ctx: secrets_commit(E, F, ctx))
            add(f"{sc}{s} ({where}): log2_row 4", lambda F=F, ctx=ctx: secrets_commit(E, F, ctx, log2_row=4))
            for d in ("params", "w", "commitment", "root"):
                add(f"{sc}{s} ({where}): null {d}", lambda F=F, ctx=ctx, d=d: secrets_commit(E, F, ctx, nulls=(d,)))
            add(f"{sc}{s} ({where}): witness of other parameters", lambda F=F, ctx=ctx: secrets_commit(E, F, ctx, w=E.w_other.h))
            add(f"{sc}{s} ({where}): log2_row above the variables of r2is", lambda F=F, ctx=ctx: secrets_commit(E, F, ctx, log2_row=11))
            add(f"{sc}{s} ({where}): log2_row 40", lambda F=F, ctx=ctx: secrets_commit(E, F, ctx, log2_row=40))
            add(f"{co}{s} ({where}): a claim that holds", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms()))
            add(f"{co}{s} ({where}): no claims", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=[], nulls=("claims", "points")))
            add(f"{co}{s} ({where}): a claim that does not hold", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=good_claim(E, F, 12345)[0]))
            for d in ("params", "commitment", "opening", "len", "claims", "points"):
                add(f"{co}{s} ({where}): null {d}", lambda F=F, ctx=ctx, d=d: claims_open(E, F, ctx, cms(), nulls=(d,)))
            add(f"{co}{s} ({where}): commitment of the other field", lambda F=F, ctx=ctx, G=other_field: claims_open(E, F, ctx, E.commitment("secrets", G, ctx)[0]))
            add(f"{co}{s} ({where}): a commitment that is not hg_secrets_commit's", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cmt()))
            add(f"{co}{s} ({where}): parameters other than the commitment's", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), params=C.byref(E.other_params)))
            add(f"{co}{s} ({where}): MAX_CLAIMS + 1 claims", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=many_in))
            add(f"{co}{s} ({where}): input 3, a public input", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=[(3, E.nv, 0, 0)]))
            add(f"{co}{s} ({where}): input id 3 + 2k + 1", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=[(3 + 2 * E.k + 1, E.nv, 0, 0)]))
            add(f"{co}{s} ({where}): r1is[0] and r2is, claims that do not hold", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=[(3 + E.k, E.nv, 0, 1), (3 + 2 * E.k, E.nv - 1, E.nv, 1)], pts=[0] * (2 * E.nv - 1)))
            add(f"{co}{s} ({where}): a claim with one coordinate too few", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=[(0, E.nv - 1, 0, 0)]))
            add(f"{co}{s} ({where}): r2is with the variables of s, second claim", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=[good_claim(E, F)[0][0], (3 + 2 * E.k, E.nv, 0, 0)]))
            add(f"{co}{s} ({where}): non-canonical coordinate", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), pts=[None] + [0] * (E.nv - 1)))
            add(f"{co}{s} ({where}): non-canonical value", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cl=good_claim(E, F, None)[0]))
            add(f"{co}{s} ({where}): MAX_QUERIES + 1 queries", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), nq=MAX_QUERIES + 1))
            add(f"{co}{s} ({where}): buffer one byte short", lambda F=F, ctx=ctx: claims_open(E, F, ctx, cms(), cap=len(sopened(F, ctx)[1]) - 1))
            add(f"{cv}{s} ({where}): an opening that verifies", lambda F=F, ctx=ctx: claims_verify(E, F, False, None, *sopened(F, ctx)))
            add(f"{cv}{s} ({where}): a tampered opening", lambda F=F, ctx=ctx: claims_verify(E, F, False, None, sopened(F, ctx)[0], tampered(sopened(F, ctx)[1])))
            add(f"{cv}{s} ({where}): another value", lambda F=F, ctx=ctx: claims_verify(E, F, False, None, *sopened(F, ctx), cl=good_claim(E, F, 12345)[0]))
            if not ctx:
                g = b"\x01" * 64
                for d in ("params", "root", "opening", "claims", "points"):
                    add(f"{cv}{s}: null {d}", lambda F=F, d=d: claims_verify(E, F, False, None, bytes(32), g, nulls=(d,)))
                add(f"{cv}{s}: log2_row 11", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, log2_row=11))
                add(f"{cv}{s}: log2_row 11 and a bad input id", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, log2_row=11, cl=[(3, E.nv, 0, 0)]))
                add(f"{cv}{s}: MAX_CLAIMS + 1 claims", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, cl=many_in))
                add(f"{cv}{s}: input 3, a public input", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, cl=[(3, E.nv, 0, 0)]))
                add(f"{cv}{s}: input id 3 + 2k + 1", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, cl=[(3 + 2 * E.k + 1, E.nv, 0, 0)]))
                add(f"{cv}{s}: a claim with one coordinate too few", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, cl=[(1, E.nv - 1, 0, 0)]))
                add(f"{cv}{s}: non-canonical coordinate", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, pts=[0] * (E.nv - 1) + [None]))
                add(f"{cv}{s}: non-canonical value", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, cl=good_claim(E, F, None)[0]))
                add(f"{cv}{s}: MAX_QUERIES + 1 queries", lambda F=F: claims_verify(E, F, False, None, bytes(32), g, nq=MAX_QUERIES + 1))
                add(f"{cv}{s}: an opening of the wrong length", lambda F=F: claims_verify(E, F, False, None, bytes(32), g))
                if not F.bn:   # the device verifiers of openings exist over Goldilocks only; without a context every check ahead of it still fires
                    add(f"{pv}_device: no context", lambda F=F: pcs_verify(E, F, True, None, bytes(32), g))
                    add(f"{pv}_device: no context and a bad claim", lambda F=F: pcs_verify(E, F, True, None, bytes(32), g, cl=[(2, [], 0)]))
                    add(f"{pv}_device: no context and MAX_QUERIES + 1", lambda F=F: pcs_verify(E, F, True, None, bytes(32), g, nq=MAX_QUERIES + 1))
                    add(f"{pv}_device: null root", lambda F=F: pcs_verify(E, F, True, None, bytes(32), g, nulls=("root",)))
                    add(f"{cv}_device: no context", lambda F=F: claims_verify(E, F, True, None, bytes(32), g))
                    add(f"{cv}_device: no context and a bad input id", lambda F=F: claims_verify(E, F, True, None, bytes(32), g, cl=[(3, E.nv, 0, 0)]))
                    add(f"{cv}_device: null params", lambda F=F: claims_verify(E, F, True, None, bytes(32), g, nulls=("params",)))
        if gpu:
            ctx, pk, hp = E.ctx, E.pk, E.host_pk
            good, bad = E.proofs[F.bn], E.garbage
            # a commitment and the context of the call
            add(f"{po}{s}: host commitment, a context passed", lambda F=F: pcs_open(E, F, ctx, E.commitment("tables", F, None)[0]))
            add(f"{po}{s}: device commitment, no context passed", lambda F=F: pcs_open(E, F, None, E.commitment("tables", F, ctx)[0]))
            add(f"{po}{s}: device commitment, another context passed", lambda F=F: pcs_open(E, F, E.ctx2, E.commitment("tables", F, ctx)[0]))
            add(f"{po}{s}: other field and another context", lambda F=F, G=(BN if not F.bn else GL): pcs_open(E, F, E.ctx2, E.commitment("tables", G, ctx)[0]))
            add(f"{co}{s}: host commitment, a context passed", lambda F=F: claims_open(E, F, ctx, E.commitment("secrets", F, None)[0]))
            add(f"{co}{s}: device commitment, no context passed", lambda F=F: claims_open(E, F, None, E.commitment("secrets", F, ctx)[0]))
            add(f"{co}{s}: device commitment, another context passed", lambda F=F: claims_open(E, F, E.ctx2, E.commitment("secrets", F, ctx)[0]))
            add(f"{co}{s}: another context and a bad input id", lambda F=F: claims_open(E, F, E.ctx2, E.commitment("secrets", F, ctx)[0], cl=[(3, E.nv, 0, 0)]))
            if not F.bn:
                def hopened(F=F):
                    return E.commitment("tables", F, None)[1], pcs_open(E, F, None, E.commitment("tables", F, None)[0])["_bytes"]

                def hsopened(F=F):
                    return E.commitment("secrets", F, None)[1], claims_open(E, F, None, E.commitment("secrets", F, None)[0])["_bytes"]
                add(f"{pv}_device: an opening that verifies", lambda F=F: pcs_verify(E, F, True, ctx, *hopened()))
                add(f"{pv}_device: a tampered opening", lambda F=F: pcs_verify(E, F, True, ctx, hopened()[0], hopened()[1][:40] + b"\x99" + hopened()[1][41:]))
                add(f"{pv}_device: an opening of the wrong length", lambda F=F: pcs_verify(E, F, True, ctx, bytes(32), b"\x01" * 64))
                add(f"{pv}_device: non-canonical value", lambda F=F: pcs_verify(E, F, True, ctx, bytes(32), b"\x01" * 64, cl=[(1, [0] * 5, None)]))
                add(f"{cv}_device: an opening that verifies", lambda F=F: claims_verify(E, F, True, ctx, *hsopened()))
                add(f"{cv}_device: another value", lambda F=F: claims_verify(E, F, True, ctx, *hsopened(), cl=good_claim(E, F, 12345)[0]))
                add(f"{cv}_device: an opening of the wrong length", lambda F=F: claims_verify(E, F, True, ctx, bytes(32), b"\x01" * 64))
                add(f"{cv}_device: a claim with one coordinate too few", lambda F=F: claims_verify(E, F, True, ctx, bytes(32), b"\x01" * 64, cl=[(1, E.nv - 1, 0, 0)]))
            pe = "hg_prove_encryptions" + s
            add(f"{pe}: two encryptions", lambda F=F: prove_encryptions(E, F, ctx, pk))
            add(f"{pe}: one encryption, reason_cap 8, no witness handles", lambda F=F: prove_encryptions(E, F, ctx, pk, n=1, rcap=8, ws=False))
            add(f"{pe}: n == 0 and no arrays", lambda F=F: prove_encryptions(E, F, ctx, pk, n=0, nulls=("s", "e", "k1", "a", "proofs", "lens", "status", "reasons")))
            add(f"{pe}: null key", lambda F=F: prove_encryptions(E, F, ctx, None))
            add(f"{pe}: host-only key", lambda F=F: prove_encryptions(E, F, ctx, hp))
            for d in ("s", "e", "k1", "a", "proofs", "lens", "status"):
                add(f"{pe}: null {d}", lambda F=F, d=d: prove_encryptions(E, F, ctx, pk, nulls=(d,)))
            add(f"{pe}: null polynomial in encryption 1", lambda F=F: prove_encryptions(E, F, ctx, pk, null_poly=True))
            add(f"{pe}: proof buffer too small", lambda F=F: prove_encryptions(E, F, ctx, pk, cap=64))
            # hg_verify_device_batch*
            add(f"{vdb}{s}: a proof and a proof that is not one", lambda F=F: verify_device_batch(E, F, ctx, pk))
            add(f"{vdb}{s}: reason_cap 8", lambda F=F: verify_device_batch(E, F, ctx, pk, rcap=8))
            add(f"{vdb}{s}: reason_cap 1", lambda F=F: verify_device_batch(E, F, ctx, pk, rcap=1))
            add(f"{vdb}{s}: reason_cap 0", lambda F=F: verify_device_batch(E, F, ctx, pk, rcap=0))
            add(f"{vdb}{s}: no reasons", lambda F=F: verify_device_batch(E, F, ctx, pk, nulls=("reasons",)))
            add(f"{vdb}{s}: n == 0", lambda F=F: verify_device_batch(E, F, ctx, pk, hs=[], proofs=[]))
            add(f"{vdb}{s}: n == 0 and no arrays", lambda F=F: verify_device_batch(E, F, ctx, pk, hs=[], proofs=[], nulls=("ws", "proofs", "lens", "results")))
            add(f"{vdb}{s}: null key", lambda F=F: verify_device_batch(E, F, ctx, None))
            add(f"{vdb}{s}: host-only key", lambda F=F: verify_device_batch(E, F, ctx, hp))
            add(f"{vdb}{s}: host-only key and null results", lambda F=F: verify_device_batch(E, F, ctx, hp, nulls=("results",)))
            for d in ("ws", "proofs", "lens", "results"):
                add(f"{vdb}{s}: null {d}", lambda F=F, d=d: verify_device_batch(E, F, ctx, pk, nulls=(d,)))
            add(f"{vdb}{s}: null witness at index 1", lambda F=F: verify_device_batch(E, F, ctx, pk, hs=[wo, None]))
            add(f"{vdb}{s}: null proof at index 1", lambda F=F: verify_device_batch(E, F, ctx, pk, proofs=[good, None]))
            add(f"{vdb}{s}: witness of other parameters at index 1", lambda F=F: verify_device_batch(E, F, ctx, pk, hs=[wo, wt]))
            if not F.bn:
                add(f"{vdb}: mode 4", lambda F=F: verify_device_batch(E, F, ctx, pk, mode=4))
                add(f"{vdb}: mode 4 and a host-only key", lambda F=F: verify_device_batch(E, F, ctx, hp, mode=4))
                add(f"{vdb}: mode 4 and a null witness", lambda F=F: verify_device_batch(E, F, ctx, pk, hs=[wo, None], mode=4))
                add(f"{vdb}: mode 4, n == 0", lambda F=F: verify_device_batch(E, F, ctx, pk, hs=[], proofs=[], mode=4))
                add(f"{vdb}: mode 3, proofs of mode 0", lambda F=F: verify_device_batch(E, F, ctx, pk, mode=3))
            # hg_verify_public*, host walk and device walk on a real proof
            for device in (False, True):
                nm = f"{vpub}{'_device' if device else ''}{s}"
                c = ctx if device else None
                add(f"{nm}: a proof", lambda F=F, device=device, c=c: verify_public(E, F, device, c, pk))
                add(f"{nm}: a proof cut short", lambda F=F, device=device, c=c: verify_public(E, F, device, c, pk, proof=good[:-16]))
                add(f"{nm}: a proof for another instance", lambda F=F, device=device, c=c: verify_public(E, F, device, c, pk, inst=hg_other_instance(E).h))
            nm = f"{vpub}_device{s}"
            add(f"{nm}: host-only key", lambda F=F: verify_public(E, F, True, ctx, hp))
            add(f"{nm}: null key", lambda F=F: verify_public(E, F, True, ctx, None))
            add(f"{nm}: no context, device key", lambda F=F: verify_public(E, F, True, None, pk))
            for d in ("instance", "proof", "n_claims", "claims", "points"):
                add(f"{nm}: null {d}", lambda F=F, d=d: verify_public(E, F, True, ctx, pk, nulls=(d,)))
            if not F.bn:
                add(f"{nm}: mode 4", lambda F=F: verify_public(E, F, True, ctx, pk, mode=4))
                add(f"{nm}: mode 1, a proof of mode 0", lambda F=F: verify_public(E, F, True, ctx, pk, mode=1))
            add(f"{nm}: instance of other parameters", lambda F=F: verify_public(E, F, True, ctx, pk, inst=E.inst_other.h))
            add(f"{nm}: claim capacity one too small", lambda F=F: verify_public(E, F, True, ctx, pk, caps=(E.nc - 1, E.nco)))
            add(f"{nm}: coordinate capacity one too small", lambda F=F: verify_public(E, F, True, ctx, pk, caps=(E.nc, E.nco - 1)))
            add(f"{nm}: a proof that is not one", lambda F=F: verify_public(E, F, True, ctx, pk, proof=bad))
            # hg_verify_public_batch*
            add(f"{vpb}{s}: a proof and a proof that is not one", lambda F=F: verify_public_batch(E, F, ctx, pk))
            add(f"{vpb}{s}: two proofs", lambda F=F: verify_public_batch(E, F, ctx, pk, proofs=[good, good]))
            add(f"{vpb}{s}: reason_cap 8", lambda F=F: verify_public_batch(E, F, ctx, pk, rcap=8))
            add(f"{vpb}{s}: reason_cap 0", lambda F=F: verify_public_batch(E, F, ctx, pk, rcap=0))
            add(f"{vpb}{s}: no reasons", lambda F=F: verify_public_batch(E, F, ctx, pk, nulls=("reasons",)))
            add(f"{vpb}{s}: n == 0", lambda F=F: verify_public_batch(E, F, ctx, pk, hs=[], proofs=[]))
            add(f"{vpb}{s}: n == 0, no arrays, no room", lambda F=F: verify_public_batch(E, F, ctx, pk, hs=[], proofs=[], caps=(0, 0), nulls=("instances", "proofs", "lens", "results", "n_claims", "claims", "points")))
            add(f"{vpb}{s}: null key", lambda F=F: verify_public_batch(E, F, ctx, None))
            add(f"{vpb}{s}: host-only key", lambda F=F: verify_public_batch(E, F, ctx, hp))
            add(f"{vpb}{s}: host-only key and null results", lambda F=F: verify_public_batch(E, F, ctx, hp, nulls=("results",)))
            for d in ("instances", "proofs", "lens", "results", "n_claims", "claims", "points"):
                add(f"{vpb}{s}: null {d}", lambda F=F, d=d: verify_public_batch(E, F, ctx, pk, nulls=(d,)))
            add(f"{vpb}{s}: null instance at index 1", lambda F=F: verify_public_batch(E, F, ctx, pk, hs=[own, None]))
            add(f"{vpb}{s}: null proof at index 1", lambda F=F: verify_public_batch(E, F, ctx, pk, proofs=[good, None]))
            add(f"{vpb}{s}: instance of other parameters at index 1", lambda F=F: verify_public_batch(E, F, ctx, pk, hs=[own, oth]))
            add(f"{vpb}{s}: claim capacity one too small", lambda F=F: verify_public_batch(E, F, ctx, pk, caps=(E.nc - 1, E.nco)))
            add(f"{vpb}{s}: coordinate capacity one too small", lambda F=F: verify_public_batch(E, F, ctx, pk, caps=(E.nc, E.nco - 1)))
            add(f"{vpb}{s}: capacity too small and a null instance", lambda F=F: verify_public_batch(E, F, ctx, pk, hs=[own, None], caps=(E.nc - 1, E.nco)))
            if not F.bn:
                add(f"{vpb}: mode 4", lambda F=F: verify_public_batch(E, F, ctx, pk, mode=4))
                add(f"{vpb}: mode 4 and room too small", lambda F=F: verify_public_batch(E, F, ctx, pk, mode=4, caps=(E.nc - 1, E.nco)))
                add(f"{vpb}: mode 4, n == 0", lambda F=F: verify_public_batch(E, F, ctx, pk, hs=[], proofs=[], mode=4))
                add(f"{vpb}: mode 2, proofs of mode 0", lambda F=F: verify_public_batch(E, F, ctx, pk, mode=2))
            # hg_instance_mle_batch*
            add(f"{mleb}{s}: two instances, ais[0]", lambda F=F: instance_mle_batch(E, F, ctx))
            add(f"{mleb}{s}: one instance, ct0is", lambda F=F: instance_mle_batch(E, F, ctx, hs=[own], which=1))
            add(f"{mleb}{s}: n == 0", lambda F=F: instance_mle_batch(E, F, ctx, n=0))
            add(f"{mleb}{s}: n == 0, selector 2", lambda F=F: instance_mle_batch(E, F, ctx, n=0, which=2))
            for d in ("instances", "point", "out"):
                add(f"{mleb}{s}: null {d}", lambda F=F, d=d: instance_mle_batch(E, F, ctx, nulls=(d,)))
            add(f"{mleb}{s}: null instance at index 1", lambda F=F: instance_mle_batch(E, F, ctx, hs=[own, None]))
            add(f"{mleb}{s}: instance of other parameters at index 1", lambda F=F: instance_mle_batch(E, F, ctx, hs=[own, oth]))
            add(f"{mleb}{s}: other parameters at index 1 and selector 2", lambda F=F: instance_mle_batch(E, F, ctx, hs=[own, oth], which=2))
            add(f"{mleb}{s}: selector 2", lambda F=F: instance_mle_batch(E, F, ctx, which=2))
            add(f"{mleb}{s}: modulus index k", lambda F=F: instance_mle_batch(E, F, ctx, index=E.k))
            add(f"{mleb}{s}: one variable short", lambda F=F: instance_mle_batch(E, F, ctx, pts=[5] * (E.nv - 1)))
            add(f"{mleb}{s}: non-canonical coordinate", lambda F=F: instance_mle_batch(E, F, ctx, pts=[5] * (E.nv - 1) + [None]))
            add(f"{mleb}{s}: one variable short and non-canonical", lambda F=F: instance_mle_batch(E, F, ctx, pts=[5] * (E.nv - 2) + [None]))
    return rows


_OTHER = {}


def hg_other_instance(E):
    """an instance of the same parameters from another witness"""
    if "i" not in _OTHER:
        _OTHER["i"] = hg.Instance.from_witness(hg.Witness.synthetic(E.params, 0xca93))
    return _OTHER["i"]


def run(part):
    E = Env(part == "gpu")
    try:
        out = {}
        for name, r in table(E, part == "gpu"):
            assert name not in out, name
            out[name] = r
        return out
    finally:
        _OTHER.clear()
        E.close()


def replay(part):
    want = json.load(open(GOLDEN))[part]
    got = run(part)
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_rows_that_need_no_device():
    replay("cpu")


@pytest.mark.gpu
def test_rows_with_a_live_context():
    replay("gpu")


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "cpu"
    rows = run(part)
    json.dump({part: rows}, open(os.environ["HG_CAPI_RECORD"], "w"), indent=0, sort_keys=True)
    print(part, len(rows), "rows")
