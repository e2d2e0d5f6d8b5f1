"""ctypes bindings to oracle/liboracle.so — the CPU oracle (test infrastructure only)."""
import os as _os
# Two OpenMP runtimes share a test process (libgomp behind the oracle, libomp behind the product library); with the default
# active wait policy their idle teams spin against each other and the oracle gets SLOWER with more threads. Read at load time.
_os.environ.setdefault("OMP_WAIT_POLICY", "passive")
import ctypes as C
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0xFFFFFFFF00000001
GOLDEN = os.path.join(ROOT, "tests", "golden")

u64p = C.POINTER(C.c_uint64)


class OrcParams(C.Structure):
    _fields_ = [("n", C.c_uint64), ("k", C.c_uint64), ("s_bound", C.c_uint64), ("e_bound", C.c_uint64),
                ("k1_bound", C.c_uint64), ("r1_bounds", u64p), ("r2_bounds", u64p), ("qis", u64p), ("k0is", u64p)]


class OrcInputs(C.Structure):
    _fields_ = [(f, u64p) for f in ("s", "e", "k1", "ais", "r1is", "r2is", "ct0is")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, "oracle", "liboracle.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
        _lib = C.CDLL(so)
        _lib.orc_root_of_unity.restype = C.c_uint64
        _lib.orc_subtable_cutoff.restype = C.c_uint64
    return _lib


def ptr(a):
    return a.ctypes.data_as(u64p)


# ---- kernel-level sum-check helpers shared by test_gpu_parity.py and test_launch_plans.py ----------------------------------
def rand_f(rng, n):
    """n random canonical words with the edges planted; rng: random.Random, or a numpy Generator (long tables: no Python loop)"""
    edge = [0, 1, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000]
    if isinstance(rng, np.random.Generator):
        v = rng.integers(0, P, size=n, dtype=np.uint64)
        k = min(n, len(edge))
        v[rng.choice(n, size=k, replace=False)] = np.array(edge[:k], dtype=np.uint64)
        return v
    v = [rng.randrange(P) for _ in range(n)]
    for i, e in enumerate(edge[:n]):
        v[rng.randrange(n)] = e
    return np.array(v, dtype=np.uint64)


# Every entry an edge of the Goldilocks reductions, so that edge meets edge in the unfolded first round: small values, p - 1 (zero low
# word), p - 2, the 2^32 boundary, the largest canonical value with all four 16-bit quarters set, 2^63, and the two halves of p.
EDGE_POOL = [0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0x100000001, 0xFFFFFFFEFFFFFFFF, 1 << 63, (P - 1) // 2, (P + 1) // 2]


def edge_f(rng, n):
    if isinstance(rng, np.random.Generator):
        return np.array(EDGE_POOL, dtype=np.uint64)[rng.integers(0, len(EDGE_POOL), size=n)]
    return np.array(rng.choices(EDGE_POOL, k=n), dtype=np.uint64)


def oracle_sumcheck(kind, tables, is_base, pw, claim, chain_skip=0, threads=4):
    ntab = len(tables)
    nv = int(np.log2(tables[0].size if is_base[0] else tables[0].size // 2))
    d = 3 if kind == 1 else 2
    tabs = [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
    ptrs = (u64p * ntab)(*[ptr(t) for t in tabs])
    flags = (C.c_int * ntab)(*[int(b) for b in is_base])
    pw = np.ascontiguousarray(pw, dtype=np.uint64).reshape(-1)
    claim = np.ascontiguousarray(claim, dtype=np.uint64)
    msgs = np.zeros(nv * (d + 1) * 2, dtype=np.uint64)
    point = np.zeros(nv * 2, dtype=np.uint64)
    evals = np.zeros(ntab * 2, dtype=np.uint64)
    sums = np.zeros(nv * d * 2, dtype=np.uint64)
    lib().orc_sumcheck(kind, C.c_size_t(nv), C.c_size_t(ntab), ptrs, flags, ptr(pw), C.c_size_t(pw.size // 2), ptr(claim),
                       C.c_size_t(chain_skip), threads, ptr(msgs), ptr(point), ptr(evals), ptr(sums))
    return msgs, point, evals, sums


def constants(n, k):
    return json.load(open(os.path.join(GOLDEN, "constants.json")))[f"{n}_{k}"]


class Params:
    """Keeps the numpy arrays alive next to the ctypes struct."""

    def __init__(self, c):
        self.c = c
        self.n, self.k = c["n"], c["k"]
        self.L = self.n.bit_length()  # log2(n) + 1
        self.arrs = {f: np.array(c[f], dtype=np.uint64) for f in ("r1_bounds", "r2_bounds", "qis", "k0is")}
        self.struct = OrcParams(c["n"], c["k"], c["s_bound"], c["e_bound"], c["k1_bound"],
                                *(ptr(self.arrs[f]) for f in ("r1_bounds", "r2_bounds", "qis", "k0is")))


def params(n, k):
    return Params(constants(n, k))


def layout_inputs(n, k, w):
    """Python restatement of get_inputs / Poly::{new,new_padded,new_shifted}
    [REF sk_encryption_circuit.rs:365-415, poly.rs:12-44] for cross-checking the product's loader."""
    L = n.bit_length()
    SZ = 1 << L

    def arr(x):
        return np.array([int(v) for v in x], dtype=np.uint64)

    def padded(x):
        a = np.zeros(SZ, dtype=np.uint64)
        a[:len(x)] = arr(x)
        return a

    def shifted(x, size):
        pad = max(size - len(x), 0)
        v = np.concatenate([np.zeros(pad, dtype=np.uint64), arr(x)])
        npow = 1 << (size - 1).bit_length()
        out = np.zeros(npow, dtype=np.uint64)
        out[:len(v)] = v
        return out

    d = {}
    d["s"] = padded(w["s"])
    d["e"] = shifted(w["e"], SZ - 1)
    d["k1"] = shifted(w["k1"], SZ - 1)
    d["ais"] = np.concatenate([padded(w["ais"][z]) for z in range(k)])
    d["r1is"] = np.concatenate([padded(w["r1is"][z]) for z in range(k)])
    d["r2is"] = np.concatenate([np.concatenate([arr(w["r2is"][z]), np.zeros(1, dtype=np.uint64)]) for z in range(k)])
    ct = []
    for z in range(k):
        c = shifted(w["ct0is"][z], SZ)
        ct.append(np.concatenate([c[1:], np.zeros(1, dtype=np.uint64)]))
    d["ct0is"] = np.concatenate(ct)
    return d


class Inputs:
    def __init__(self, d):
        self.d = {k: np.ascontiguousarray(v, dtype=np.uint64) for k, v in d.items()}
        self.struct = OrcInputs(*(ptr(self.d[f]) for f in ("s", "e", "k1", "ais", "r1is", "r2is", "ct0is")))


def fixture_inputs(n, k, bits):
    w = json.load(open(os.path.join(GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json")))
    return Inputs(layout_inputs(n, k, w))


def _err():
    return C.create_string_buffer(512)


def prove(p, inp, threads=1, cap=1 << 24):
    buf = (C.c_uint8 * cap)()
    ln = C.c_size_t(0)
    tm = (C.c_double * 2)()
    err = _err()
    rc = lib().orc_prove(C.byref(p.struct), C.byref(inp.struct), threads, buf, C.c_size_t(cap), C.byref(ln), tm, err, C.c_size_t(512))
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return bytes(buf[:ln.value]), (tm[0], tm[1])


def verify(p, inp, proof, threads=1):
    err = _err()
    rc = lib().orc_verify(C.byref(p.struct), C.byref(inp.struct), threads, proof, C.c_size_t(len(proof)), err, C.c_size_t(512))
    return rc == 0, err.value.decode()


def circuit_eval(p, inp):
    info = (C.c_uint64 * 3)()
    err = _err()
    lib().orc_circuit_eval(C.byref(p.struct), C.byref(inp.struct), None, C.c_size_t(0), None, info, err, C.c_size_t(512))
    nu = info[0]
    lasso_in = np.zeros(1 << nu, dtype=np.uint64)
    sum_out = np.zeros(p.k << p.L, dtype=np.uint64)
    rc = lib().orc_circuit_eval(C.byref(p.struct), C.byref(inp.struct), ptr(lasso_in), C.c_size_t(lasso_in.size), ptr(sum_out), info, err, C.c_size_t(512))
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return lasso_in, sum_out, dict(nu=int(info[0]), num_nodes=int(info[1]), rows=int(info[2]))


def lasso_prove(p, lasso_in, threads=1, cap=1 << 24):
    buf = (C.c_uint8 * cap)()
    ln = C.c_size_t(0)
    nu = int(np.log2(lasso_in.size))
    claim = np.zeros(2 * nu + 2, dtype=np.uint64)
    err = _err()
    rc = lib().orc_lasso_prove(C.byref(p.struct), ptr(lasso_in), threads, buf, C.c_size_t(cap), C.byref(ln), ptr(claim), err, C.c_size_t(512))
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return bytes(buf[:ln.value]), claim


def lasso_verify(p, proof):
    err = _err()
    rc = lib().orc_lasso_verify(C.byref(p.struct), proof, C.c_size_t(len(proof)), err, C.c_size_t(512))
    return rc == 0, err.value.decode()


def lasso_layout(p):
    buf = C.create_string_buffer(1 << 16)
    n = lib().orc_lasso_layout(C.byref(p.struct), buf, C.c_size_t(1 << 16))
    assert n > 0
    mems, lk = buf.value.decode().split("|")
    return mems.split(","), lk.split(";")


def keccak256(data: bytes) -> bytes:
    """Keccak-256 of the C oracle (pinned by the reference's chain KATs in test_oracle_kats.py)."""
    import ctypes
    buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    out = (ctypes.c_uint8 * 32)()
    lib().orc_keccak256(buf, ctypes.c_size_t(len(data)), out)
    return bytes(out)


def bn254():
    """The BN254 Python oracle (oracle/bn254.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("oracle_bn254", os.path.join(ROOT, "oracle", "bn254.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def bn254_gkr():
    """The BN254 whole-proof Python oracle (oracle/bn254_gkr.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("oracle_bn254_gkr", os.path.join(ROOT, "oracle", "bn254_gkr.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def bn254_lasso_fns(p):
    """(prove, verify) callbacks for bn254_gkr.prove / .verify: the Lasso node of oracle/bn254.py on the C oracle's integer tables."""
    import numpy as np
    bn = bn254()
    state = {}

    def prove_fn(vin, ch):
        P = lasso_polys(p, np.array(vin, dtype=np.uint64))
        state["P"] = P
        els, r, v = bn.lasso_prove(P, ch)
        return els, r, v, bn.lasso_challenge_count(P["nu"])

    def verify_fn(els, ch, layout=None):
        P = layout or state["P"]
        r, v, pos = bn.lasso_verify(els, P["nu"], P["mem_dim"], P["mem_cutoff"], ch, partial=True)
        return r, v, pos, bn.lasso_challenge_count(P["nu"])

    return prove_fn, verify_fn


def lasso_polys(p, lasso_in):
    """Integer tables of the Lasso node from the C oracle (orc_lasso_polys) as Python lists, plus lookup_mems."""
    import ctypes as C
    import numpy as np
    L = lib()
    nu, A, rows = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    err = C.create_string_buffer(256)
    lin = np.ascontiguousarray(lasso_in, dtype=np.uint64)
    u64p, u8p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    L.orc_lasso_polys.argtypes = [C.c_void_p, u64p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), u64p, u64p, u64p,
                                  u64p, u8p, i32p, u64p, C.c_char_p, C.c_size_t]
    pp = C.cast(C.byref(p.struct), C.c_void_p)
    assert L.orc_lasso_polys(pp, ptr(lin), C.byref(nu), C.byref(A), C.byref(rows), None, None, None, None, None, None, None, err, 256) == 0, err.value
    N = 1 << nu.value
    dims = np.zeros(4 * N, dtype=np.uint64); rd = np.zeros(A.value * N, dtype=np.uint64)
    fin = np.zeros(A.value * 65536, dtype=np.uint64); ep = np.zeros(A.value * N, dtype=np.uint64)
    rl = np.zeros(N, dtype=np.uint8); md = np.zeros(A.value, dtype=np.int32); mc = np.zeros(A.value, dtype=np.uint64)
    assert L.orc_lasso_polys(pp, ptr(lin), C.byref(nu), C.byref(A), C.byref(rows), ptr(dims), ptr(rd), ptr(fin), ptr(ep),
                             rl.ctypes.data_as(u8p), md.ctypes.data_as(i32p), ptr(mc), err, 256) == 0, err.value
    _, lookups = lasso_layout(p)
    lookup_mems = [[int(x) for x in l.split(":")[2].split("/")] for l in lookups]
    a = A.value
    return dict(nu=nu.value, A=a, rows=rows.value,
                dims=[dims[c * N:(c + 1) * N].tolist() for c in range(4)],
                read_cts=[rd[m * N:(m + 1) * N].tolist() for m in range(a)],
                final_cts=[fin[m * 65536:(m + 1) * 65536].tolist() for m in range(a)],
                e_polys=[ep[m * N:(m + 1) * N].tolist() for m in range(a)],
                row_lookup=rl.tolist(), mem_dim=md.tolist(), mem_cutoff=mc.tolist(), lookup_mems=lookup_mems)


# ---- the C++ oracle over bn256::Fr (oracle/fr.hpp: symbols orcbn_*) and the protocol modes of both field builds -------------
R_BN = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MODE_ABSORB, MODE_EXT_MEMCHECK = 1, 2


def _sym(field, name):
    return getattr(lib(), ("orcbn_" if field == "bn254" else "orc_") + name)


def limbs_of(field):
    return (4, 4) if field == "bn254" else (1, 2)


def to_limbs(vals, nl):
    """Python integers -> canonical little-endian u64 limbs (nl per element); an (n, nl) uint64 array holds the limbs already."""
    if nl == 1 and isinstance(vals, np.ndarray):   # (long Goldilocks tables: already in that form)
        return np.ascontiguousarray(vals, dtype=np.uint64)
    if isinstance(vals, np.ndarray) and vals.ndim == 2:   # (long bn254 tables: rand_fr / edge_fr)
        assert vals.shape[1] == nl and vals.dtype == np.uint64, (vals.shape, vals.dtype)
        return np.ascontiguousarray(vals).reshape(-1)
    a = np.zeros(len(vals) * nl, dtype=np.uint64)
    for i, v in enumerate(vals):
        for j in range(nl):
            a[i * nl + j] = (int(v) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return a


def from_limbs(a, nl):
    a = [int(x) for x in a]
    return [sum(a[i * nl + j] << (64 * j) for j in range(nl)) for i in range(len(a) // nl)]


def f_binop(field, op, a, b):
    nl = limbs_of(field)[0]
    out = np.zeros(len(a) * nl, dtype=np.uint64)
    _sym(field, "f_binop")(op, C.c_size_t(len(a)), ptr(to_limbs(a, nl)), ptr(to_limbs(b, nl)), ptr(out))
    return from_limbs(out, nl)


def challenge_chain(field, n):
    nl = limbs_of(field)[0]
    out = np.zeros(n * nl, dtype=np.uint64)
    _sym(field, "challenge_chain")(C.c_size_t(n), ptr(out))
    return from_limbs(out, nl)


def wire_roundtrip(field, vals):
    nl = limbs_of(field)[0]
    buf = (C.c_uint8 * (len(vals) * 8 * nl))()
    back = np.zeros(len(vals) * nl, dtype=np.uint64)
    f = _sym(field, "wire_roundtrip")
    f.restype = C.c_size_t
    n = f(C.c_size_t(len(vals)), ptr(to_limbs(vals, nl)), buf, ptr(back))
    return bytes(buf[:n]), from_limbs(back, nl)


def root_of_unity_f(field, log2n):
    nl = limbs_of(field)[0]
    out = np.zeros(nl, dtype=np.uint64)
    _sym(field, "root_of_unity_limbs")(C.c_size_t(log2n), ptr(out))
    return from_limbs(out, nl)[0]


def prove_f(field, p, inp, threads=1, mode=0, cap=1 << 25):
    """BfvEncrypt::prove of the C++ oracle over `field` ("goldilocks" | "bn254"); inp holds Goldilocks-form tables."""
    buf = (C.c_uint8 * cap)()
    ln = C.c_size_t(0)
    tm = (C.c_double * 2)()
    err = _err()
    rc = _sym(field, "prove_mode")(C.byref(p.struct), C.byref(inp.struct), threads, mode, buf, C.c_size_t(cap), C.byref(ln), tm, err, C.c_size_t(512))
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return bytes(buf[:ln.value]), (tm[0], tm[1])


def verify_f(field, p, inp, proof, threads=1, mode=0):
    err = _err()
    rc = _sym(field, "verify_mode")(C.byref(p.struct), C.byref(inp.struct), threads, mode, proof, C.c_size_t(len(proof)), err, C.c_size_t(512))
    return rc == 0, err.value.decode()


def lasso_prove_f(field, p, lasso_in_ints, threads=1, mode=0, chain_skip=0, cap=1 << 25):
    """Lasso node of the C++ oracle over `field` on a table of Python integers / numpy u64 (2^nu entries)."""
    fl, el = limbs_of(field)
    nu = int(len(lasso_in_ints)).bit_length() - 1
    lin = to_limbs(lasso_in_ints, fl) if fl > 1 else np.ascontiguousarray(lasso_in_ints, dtype=np.uint64)
    buf = (C.c_uint8 * cap)()
    ln = C.c_size_t(0)
    claim = np.zeros((nu + 1) * el, dtype=np.uint64)
    err = _err()
    rc = _sym(field, "lasso_prove_mode")(C.byref(p.struct), ptr(lin), threads, mode, C.c_size_t(chain_skip), buf, C.c_size_t(cap), C.byref(ln), ptr(claim),
                                        err, C.c_size_t(512))
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return bytes(buf[:ln.value]), from_limbs(claim, el) if field == "bn254" else claim


def lasso_verify_f(field, p, proof, mode=0):
    err = _err()
    rc = _sym(field, "lasso_verify_mode")(C.byref(p.struct), mode, proof, C.c_size_t(len(proof)), err, C.c_size_t(512))
    return rc == 0, err.value.decode()


def grand_product_f(field, tabs, chain_skip=0, threads=1, cap=1 << 24):
    """prove_grand_product of the C++ oracle on nb base-field tables (lists of Python ints); -> (proof bytes, claims, point)."""
    fl, el = limbs_of(field)
    nb, ln_ = len(tabs), len(tabs[0])
    nv = ln_.bit_length() - 1
    arrs = [to_limbs(t, fl) for t in tabs]
    ptrs = (u64p * nb)(*[ptr(a) for a in arrs])
    buf = (C.c_uint8 * cap)()
    ln = C.c_size_t(0)
    claims = np.zeros(nb * el, dtype=np.uint64)
    point = np.zeros(nv * el, dtype=np.uint64)
    err = _err()
    rc = _sym(field, "grand_product")(C.c_size_t(nb), C.c_size_t(ln_), ptrs, C.c_size_t(chain_skip), threads, buf, C.c_size_t(cap), C.byref(ln),
                                     ptr(claims), ptr(point), err, C.c_size_t(512))
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return bytes(buf[:ln.value]), from_limbs(claims, el), from_limbs(point, el)


def sumcheck_f(field, kind, tabs, pw=(), claim=0, chain_skip=0, threads=1):
    """prove_sum_check of the C++ oracle over `field` on base-field tables (lists of Python ints or limb arrays), kind 0 collation,
    1 grand product, 2 prodsum; pw, claim: Python ints. -> (msgs, point, evals, sums) as flat lists of ints (sums: the true round
    sums at 0, 2[, 3], which do not depend on the claim)."""
    fl, el = limbs_of(field)
    ntab = len(tabs)
    nv = (len(tabs[0]) - 1).bit_length()
    d = 3 if kind == 1 else 2
    arrs = [to_limbs(t, fl) for t in tabs]
    ptrs = (u64p * ntab)(*[ptr(a) for a in arrs])
    flags = (C.c_int * ntab)(*([1] * ntab))
    ppw = to_limbs(list(pw), el) if len(pw) else np.zeros(el, dtype=np.uint64)
    pcl = to_limbs([claim], el)
    msgs = np.zeros(max(nv * (d + 1), 1) * el, dtype=np.uint64)
    point = np.zeros(max(nv, 1) * el, dtype=np.uint64)
    evals = np.zeros(ntab * el, dtype=np.uint64)
    sums = np.zeros(max(nv * d, 1) * el, dtype=np.uint64)
    _sym(field, "sumcheck")(kind, C.c_size_t(nv), C.c_size_t(ntab), ptrs, flags, ptr(ppw), C.c_size_t(len(pw)), ptr(pcl), C.c_size_t(chain_skip), threads,
                            ptr(msgs), ptr(point), ptr(evals), ptr(sums))
    return from_limbs(msgs, el)[:nv * (d + 1)], from_limbs(point, el)[:nv], from_limbs(evals, el), from_limbs(sums, el)[:nv * d]


def mle_eval_f(field, table, point):
    """BoxMultilinearPoly::evaluate of the C++ oracle: a base-field table (Python ints or a limb array) at a point of Python ints."""
    fl, el = limbs_of(field)
    nv = (len(table) - 1).bit_length()
    out = np.zeros(el, dtype=np.uint64)
    pt = to_limbs(point if isinstance(point, np.ndarray) else list(point), el) if len(point) else np.zeros(el, dtype=np.uint64)   # ((nv, el) limbs as they are)
    _sym(field, "mle_eval_f")(ptr(to_limbs(table, fl)), C.c_size_t(nv), ptr(pt), ptr(out))
    return from_limbs(out, el)[0]


# ---- transforms and folds on limb arrays (tests/test_transform_paths.py; pinned in tests/test_oracle_kats.py) ---------------------
def ntt_f(field, limbs, log2n, inverse=False):
    """ntt of the C++ oracle on one row: 2^log2n elements as limbs ((N,) words for goldilocks, (N, 4) for bn254) -> the same shape"""
    a = np.ascontiguousarray(limbs, dtype=np.uint64)
    assert a.size == limbs_of(field)[0] << log2n, (a.shape, log2n)
    out = np.zeros_like(a)
    _sym(field, "ntt")(ptr(a), C.c_size_t(log2n), 1 if inverse else 0, ptr(out))
    return out


def binop_limbs(field, ext, op, a, b):
    """f_binop (ext = False) / e_binop of the C++ oracle on limb arrays of equal shape; op: 0 add, 1 sub, 2 mul"""
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    nl = limbs_of(field)[1 if ext else 0]
    assert a.shape == b.shape and a.size % nl == 0
    out = np.zeros_like(a)
    _sym(field, "e_binop" if ext else "f_binop")(op, C.c_size_t(a.size // nl), ptr(a), ptr(b), ptr(out))
    return out


def fold_f(field, table, is_base, r):
    """fix_var on the lowest variable, out[j] = x + r (y - x) with x = T[2j], y = T[2j + 1], from the oracle's binops. table: 2^nv
    base-field elements (is_base) or extension elements as limbs, r: one extension element as limbs -> (2^(nv-1), e_limbs)"""
    fl, el = limbs_of(field)
    t = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, fl if is_base else el)
    x, y = np.ascontiguousarray(t[0::2]), np.ascontiguousarray(t[1::2])
    if is_base:   # y - x in the base field, then both lifted (the higher coordinate zero)
        d, xe = np.zeros((len(x), el), dtype=np.uint64), np.zeros((len(x), el), dtype=np.uint64)
        d[:, :fl] = binop_limbs(field, False, 1, y, x)
        xe[:, :fl] = x
    else:
        d, xe = binop_limbs(field, True, 1, y, x), x
    rr = np.ascontiguousarray(np.broadcast_to(np.asarray(r, dtype=np.uint64).reshape(1, el), (len(x), el)))
    return binop_limbs(field, True, 0, xe, binop_limbs(field, True, 2, rr, d))


def field_modulus(field):
    return R_BN if field == "bn254" else P


def ints_to_limbs(vals, nl):
    """Python ints -> (n, nl) limbs ((n,) for nl = 1) through their bytes (long lists: no per-limb Python loop)"""
    a = np.frombuffer(b"".join(int(v).to_bytes(8 * nl, "little") for v in vals), dtype=np.uint64).copy()
    return a if nl == 1 else a.reshape(-1, nl)


def ntt_impulse(field, log2n, j, c, inverse=False):
    """The transform of the row that holds c at position j and zero elsewhere, without the oracle's ntt: out[k] = c w^(jk), filled by a
    running product with g = w^j in Python integers (the inverse: w^-1 and the factor 1 / N). -> limbs, the shape ntt_f returns"""
    q, N = field_modulus(field), 1 << log2n
    w = root_of_unity_f(field, log2n)
    if inverse:
        w, c = pow(w, q - 2, q), c * pow(N, q - 2, q) % q
    g, v, out = pow(w, j, q), c % q, []
    for _ in range(N):
        out.append(v)
        v = v * g % q
    return ints_to_limbs(out, limbs_of(field)[0])


# ---- long bn254 tables as (n, 4) uint64 limb arrays: no Python loop over the elements ---------------------------------------------
# Every edge of the 256-bit arithmetic: the small values, r - 1 and r - 2 (the largest canonical values), the two halves of r, the
# limb boundaries 2^64 - 1, 2^64, 2^128 + 5, the top bit 2^253, and r - k for small k (the lifts of negative integers).
EDGE_POOL_FR = [0, 1, 2, R_BN - 1, R_BN - 2, (R_BN - 1) // 2, (R_BN + 1) // 2, (1 << 64) - 1, 1 << 64, (1 << 128) + 5, 1 << 253] + \
               [R_BN - k for k in (3, 4, 7, 19, 255, 65537)]


def fr_limbs(vals):
    """Python ints (a short list) -> (n, 4) uint64 limbs"""
    return to_limbs(list(vals), 4).reshape(-1, 4)


def rand_fr(rng, n):
    """n random canonical bn254 elements as (n, 4) limbs (rng: numpy Generator). The top limb is drawn below the top limb of r, which
    makes every value canonical by construction; every edge of EDGE_POOL_FR is planted at a random position (the first n of them in
    a table shorter than the pool)."""
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R_BN >> 192, size=n, dtype=np.uint64)
    pool = fr_limbs(EDGE_POOL_FR)[:n]
    a[rng.choice(n, size=len(pool), replace=False)] = pool
    return a


def edge_fr(rng, n):
    """n elements, every one drawn from EDGE_POOL_FR, so that edge meets edge in the unfolded first round"""
    return fr_limbs(EDGE_POOL_FR)[rng.integers(0, len(EDGE_POOL_FR), size=n)]


def gl_form(v):
    """A small signed integer given as an Fr element (negatives as r - |z|) -> its Goldilocks residue (p - |z|)."""
    v = int(v)
    return v if v <= R_BN // 2 else P - (R_BN - v)


def bn254_fixture_inputs(n=1024, k=1, bits=27):
    """The reference's bn254 fixture laid out by get_inputs, as Goldilocks-form tables (what the C surface takes)."""
    w = json.load(open(os.path.join(GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json")))
    conv = {}
    for f in ("s", "e", "k1"):
        conv[f] = [gl_form(x) for x in w[f]]
    for f in ("ais", "r1is", "r2is", "ct0is"):
        conv[f] = [[gl_form(x) for x in row] for row in w[f]]
    return Inputs(layout_inputs(n, k, conv))


def elems_be(proof, nbytes):
    return [int.from_bytes(proof[i:i + nbytes], "big") for i in range(0, len(proof), nbytes)]


# ---- node reductions and claim tables (tests/test_node_reductions.py; pinned in tests/test_oracle_kats.py) ----------------------------
# Goldilocks only. Extension elements are (c0, c1) rows of uint64; every table operation is an O(N) call of the oracle's binops.
def e_chain(n):
    """The first n E challenges as an (n, 2) limb array (E challenge i = base challenges 2i, 2i + 1)."""
    return np.array(challenge_chain("goldilocks", 2 * n), dtype=np.uint64).reshape(n, 2)


def _e_rows(v, n):
    """One extension element broadcast to n rows."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.uint64).reshape(1, 2), (n, 2)))


def e_scale(table, v):
    """table (n, 2) times the extension element v"""
    return binop_limbs("goldilocks", True, 2, table, _e_rows(v, len(table)))


def eq_table_limbs(point):
    """eq(point, .) over len(point) variables, coordinate i on bit i of the index, by doubling: the half with bit i set is t z_i, the
    other half t - t z_i. point: (k, 2) limbs -> (2^k, 2)"""
    t = np.array([[1, 0]], dtype=np.uint64)
    for z in np.asarray(point, dtype=np.uint64).reshape(-1, 2):
        hi = e_scale(t, z)
        t = np.concatenate([binop_limbs("goldilocks", True, 1, t, hi), hi])
    return t


def windowed_point(chain, z_off, w, hib, nv):
    """z' of an eq-factored job: the chain run (z_off .. z_off + w), then the bits of hib (lowest first) as field elements. -> (nv, 2)"""
    z = np.zeros((nv, 2), dtype=np.uint64)
    z[:w] = chain[z_off:z_off + w]
    for k in range(w, nv):
        z[k, 0] = (hib >> (k - w)) & 1
    return z


def eq_factored_b_tables(chain, z_off, w, hib, nv, kappas):
    """The tables an eq-factored job stands for, materialised: b_i = kappa_i eq(z', .), each as the flat (2 * 2^nv,) array a plain job takes."""
    eq = eq_table_limbs(windowed_point(chain, z_off, w, hib, nv))
    return [e_scale(eq, k).reshape(-1) for k in np.asarray(kappas, dtype=np.uint64).reshape(-1, 2)]


def eq_claims_table(chain, n, point_offs, alpha_off):
    """sum_a alpha_a eq(r_a, .): r_a = chain[point_offs[a] .. + n), alpha_a = chain[alpha_off + a] (alpha_off None: one claim, weight 1)"""
    acc = None
    for a, po in enumerate(point_offs):
        t = eq_table_limbs(chain[po:po + n])
        if alpha_off is not None:
            t = e_scale(t, chain[alpha_off + a])
        acc = t if acc is None else binop_limbs("goldilocks", True, 0, acc, t)
    return acc


def powers_limbs(w, n_log2):
    """w^0 .. w^(2^n_log2 - 1) as words, by doubling (the upper half is the lower half times w^(half))"""
    t = np.array([1], dtype=np.uint64)
    for k in range(n_log2):
        step = np.full(len(t), pow(w, 1 << k, P), dtype=np.uint64)
        t = np.concatenate([t, binop_limbs("goldilocks", False, 2, t, step)])
    return t


def fft_rows_table(chain, L, inverse, point_offs, alpha_off):
    """The DFT-row table of an FFT node: F(x) = scale sum_a alpha_a prod_b (1 + r_{a,b} (W[(x 2^b) mod N] - 1)), W the powers of the
    2^L-th root of unity (inverse: of its inverse, scale = 1 / N, else 1); claims as in eq_claims_table. -> (2^L, 2)"""
    N = 1 << L
    w = root_of_unity_f("goldilocks", L)
    scale = 1
    if inverse:
        w, scale = pow(w, P - 2, P), pow(N, P - 2, P)
    W = powers_limbs(w, L)
    wm1 = binop_limbs("goldilocks", False, 1, W, np.ones(N, dtype=np.uint64))   # W - 1
    x = np.arange(N, dtype=np.uint64)
    one = _e_rows([1, 0], N)
    acc = None
    for a, po in enumerate(point_offs):
        p = _e_rows([scale, 0], N)
        if alpha_off is not None:
            p = e_scale(p, chain[alpha_off + a])
        for b in range(L):
            d = np.zeros((N, 2), dtype=np.uint64)
            d[:, 0] = wm1[(x << np.uint64(b)) & np.uint64(N - 1)]
            p = binop_limbs("goldilocks", True, 2, p, binop_limbs("goldilocks", True, 0, one, e_scale(d, chain[po + b])))
        acc = p if acc is None else binop_limbs("goldilocks", True, 0, acc, p)
    return acc


def oracle_prodsum(a_tables, b_tables, chain_skip, threads=4):
    """oracle_sumcheck(2, ..) on the pairs (a_i, b_i) with the job's chain position -> (sums nv x (g(0), g(2)), evals (a_0(r), b_0(r), ..)),
    both as flat word arrays, the layout hg_prodsum_jobs returns per job"""
    tabs, flags = [], []
    for a, b in zip(a_tables, b_tables):
        tabs += [a, b]
        flags += [True, False]
    _, _, evals, sums = oracle_sumcheck(2, tabs, flags, np.zeros((0, 2), dtype=np.uint64), np.array([3, 4], dtype=np.uint64), chain_skip, threads=threads)
    return sums, evals
