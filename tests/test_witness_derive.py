"""hg_witness_derive / hg_witness_derive_into: the witness of a BFV secret-key encryption (ct0is, r2is, r1is) derived on the device
from what the encryptor holds (s, e, k1, ais).

References, none of them this library's derive path: the reference's own JSON witnesses under tests/golden/ (written by its
scripts/circuit_sk.py), the host path hg_witness_synthetic, and a restatement of the rule in Python integers kept in this file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hglib import hg, ROOT

P = hg.P
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55), (8192, 4, 55)]
BN_FIX = [(1024, 1, 27), (2048, 1, 52), (4096, 2, 55)]
SETS = [(1024, 1), (2048, 1), (4096, 2), (8192, 4), (16384, 8), (32768, 16)]
INPUTS = ("s", "e", "k1", "ais")
T = 65537


@pytest.fixture(scope="module")
def ctx():
    c = hg.Context(0)
    yield c
    c.close()


def same_tables(got, want):
    for f in hg.Witness.FIELDS:
        assert got[f].shape == want[f].shape, f
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, "%s differs at %d positions, first %d: %d != %d" % (f, bad.size, bad[0], got[f][bad[0]], want[f][bad[0]])


# ---- the rule in Python integers (ISSUE: ascending degree, signed; [REF scripts/circuit_sk.py:18-140]) --------------------------------
def cmod(z, q):
    r = z % q
    return r - q if r > (q - 1) // 2 else r


def product_over_z(a, s):
    """a * s over Z: a as three signed 21-bit limbs (|a| < 2^63), each convolved in int64 (|sums| <= n 2^21), recombined as ints"""
    sgn = np.array([-1 if x < 0 else 1 for x in a], dtype=np.int64)
    mag = [abs(x) for x in a]
    sa = np.array(s, dtype=np.int64)
    out = None
    for limb in range(3):
        part = sgn * np.array([(m >> (21 * limb)) & 0x1FFFFF for m in mag], dtype=np.int64)
        c = np.convolve(part, sa).astype(object) * (1 << (21 * limb))
        out = c if out is None else out + c
    return [int(x) for x in out]


def derive_rule(n, q, k0, s, e, k1, a):
    h = product_over_z(a, s) + [0]                     # degree <= 2n-2, h[2n-1] = 0
    for j in range(n):
        h[j] += e[j] + k0 * k1[j]
    ct0 = [cmod(h[j] - h[j + n], q) for j in range(n)]
    r2 = [cmod(-h[j + n], q) for j in range(n - 1)]
    r1 = []
    for j in range(2 * n - 1):
        jj = j % n
        d = (ct0[j] if j < n else 0) - h[j] - (r2[jj] if jj + 1 < n else 0)
        assert d % q == 0
        r1.append(d // q)
    return ct0, r2, r1


def enc(z):
    return z if z >= 0 else P - (-z)


def table(coeffs, size, top):
    """descending-degree layout: coefficient j at position top - j, zeros elsewhere"""
    t = np.zeros(size, dtype=np.uint64)
    for j, c in enumerate(coeffs):
        t[top - j] = enc(c)
    return t


def lay_out_inputs(n, s, e, k1, ais):
    return {"s": table(s, 2 * n, n - 1), "e": table(e, 2 * n, 2 * n - 2), "k1": table(k1, 2 * n, 2 * n - 2),
            "ais": np.concatenate([table(a, 2 * n, n - 1) for a in ais])}


def restated(params, s, e, k1, ais):
    """(all seven tables by the rule, the derived tables that leave their bound in params)"""
    n, k = params.n, params.k
    d = lay_out_inputs(n, s, e, k1, ais)
    r1t, r2t, ctt, out_of_bound = [], [], [], set()
    for i in range(k):
        q, k0 = int(params.qis[i]), int(params.k0is[i])
        ct0, r2, r1 = derive_rule(n, q, k0, s, e, k1, ais[i])
        if max(abs(x) for x in r1) > int(params.r1_bounds[i]):
            out_of_bound.add("r1is")
        # (the circuit range-checks every r2_i chunk with R2_BOUND_0, so the bound that counts is the smaller of the two)
        if max(abs(x) for x in r2) > min(int(params.r2_bounds[i]), int(params.r2_bounds[0])):
            out_of_bound.add("r2is")
        ctt.append(table(ct0, 2 * n, 2 * n - 2)); r1t.append(table(r1, 2 * n, 2 * n - 2)); r2t.append(table(r2, n, n - 2))
    d["r1is"], d["r2is"], d["ct0is"] = np.concatenate(r1t), np.concatenate(r2t), np.concatenate(ctt)
    return d, out_of_bound


def test_restatement_reproduces_a_reference_fixture():
    """the Python restatement itself against a file the reference wrote (no GPU): it is the judge of test 3"""
    import json
    n, k = 1024, 1
    w = json.load(open(os.path.join(GOLDEN, "sk_enc_1024_1x27_65537.json")))
    sgn = lambda v: [int(x) if int(x) < P // 2 else int(x) - P for x in v][::-1]
    params = hg.params_builtin(n, k)
    d, oob = restated(params, sgn(w["s"]), sgn(w["e"]), sgn(w["k1"]), [sgn(w["ais"][0])])
    assert not oob
    same_tables(d, hg.Witness.from_json(params, os.path.join(GOLDEN, "sk_enc_1024_1x27_65537.json")).arrays())


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family,n,k,bits", [("gl", *f) for f in FIX] + [("bn254", *f) for f in BN_FIX])
def test_derive_reproduces_reference_fixture(ctx, family, n, k, bits):
    params = hg.params_builtin(n, k)
    if family == "gl":
        ref = hg.Witness.from_json(params, os.path.join(GOLDEN, f"sk_enc_{n}_{k}x{bits}_65537.json")).arrays()
    else:
        ref = hg.Witness.from_json_bn254(params, os.path.join(GOLDEN, f"bn254_sk_enc_{n}_{k}x{bits}_65537.json")).arrays()
    got = hg.Witness.derive(ctx, params, {f: ref[f] for f in INPUTS}).arrays()
    same_tables(got, ref)


# ---- 2. the host path at every built-in size ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,k", SETS)
def test_derive_equals_host_path(ctx, n, k):
    params = hg.params_builtin(n, k)
    for seed in (0x5EED0 + n, 0xD371 + 7 * n):
        ref = hg.Witness.synthetic(params, seed).arrays()
        got = hg.Witness.derive(ctx, params, {f: ref[f] for f in INPUTS}).arrays()
        same_tables(got, ref)


# ---- 3. extremes, judged by the restatement ----------------------------------------------------------------------------------------
def extreme_cases(n, params):
    half = [(int(params.qis[i]) - 1) // 2 for i in range(params.k)]
    kb = (T - 1) // 2
    alt = [1 if j % 2 == 0 else -1 for j in range(n)]
    return {
        "a=+half s=+1 e=+19 k1=+kb": ([1] * n, [19] * n, [kb] * n, [[h] * n for h in half]),
        "a=-half s=alt e=-19 k1=-kb": (alt, [-19] * n, [-kb] * n, [[-h] * n for h in half]),
        "a=+half s=alt e=+19 k1=-kb": (alt, [19] * n, [-kb] * n, [[h] * n for h in half]),
        "a=-half s=+1 e=-19 k1=+kb": ([1] * n, [-19] * n, [kb] * n, [[-h] * n for h in half]),
        "zero secrets": ([0] * n, [0] * n, [0] * n, [[h if j % 3 else -h for j in range(n)] for h in half]),
        "all zero": ([0] * n, [0] * n, [0] * n, [[0] * n for _ in half]),
    }


def run_extremes(ctx, params):
    n = params.n
    verdicts = {}
    for name, (s, e, k1, ais) in extreme_cases(n, params).items():
        want, oob = restated(params, s, e, k1, ais)
        d = {f: want[f] for f in INPUTS}
        if oob:
            with pytest.raises(hg.HgError) as ei:
                hg.Witness.derive(ctx, params, d)
            assert any(t in str(ei.value) for t in oob), (name, oob, str(ei.value))
            assert "bound" in str(ei.value), str(ei.value)
        else:
            same_tables(hg.Witness.derive(ctx, params, d).arrays(), want)
        verdicts[name] = sorted(oob)
    print("n=%d k=%d: %s" % (n, params.k, verdicts))
    return verdicts


@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(1024, 1), (4096, 2)])
def test_derive_extremes_builtin(ctx, n, k):
    run_extremes(ctx, hg.params_builtin(n, k))


@pytest.mark.gpu
def test_derive_extremes_59_bit_modulus(ctx):
    q = (1 << 59) - 55
    assert q % 2 == 1 and q % T != 0 and q.bit_length() == 59
    run_extremes(ctx, hg.params_derive(32768, 1, [q]))


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_derive_refusals(ctx):
    n, k = 1024, 1
    params = hg.params_builtin(n, k)
    ref = hg.Witness.from_json(params, os.path.join(GOLDEN, "sk_enc_1024_1x27_65537.json")).arrays()
    good = {f: ref[f] for f in INPUTS}
    half = (int(params.qis[0]) - 1) // 2

    def changed(f, pos, word):
        d = {g: good[g].copy() for g in INPUTS}
        d[f][pos] = word
        return d
    cases = [
        (changed("s", 5, 2), r"table s: .*s_bound"),
        (changed("s", 5, P - 2), r"table s: .*s_bound"),
        (changed("e", n + 3, 20), r"table e: .*e_bound"),
        (changed("k1", n + 9, P - 32769), r"table k1: .*k1_bound"),
        (changed("ais", 3, half + 1), r"table ais of modulus 0 .*\(q_i-1\)/2"),
        (changed("ais", 3, P - half - 1), r"table ais of modulus 0 .*\(q_i-1\)/2"),
        (changed("s", 0, P), r"table s: non-canonical"),
        (changed("ais", n - 1, 2 ** 64 - 1), r"table ais of modulus 0 .*non-canonical"),
        (changed("e", 0, 1), r"table e: .*pads"),
    ]
    for d, pattern in cases:
        with pytest.raises(hg.HgError, match=pattern):
            hg.Witness.derive(ctx, params, d)
    assert np.array_equal(hg.Witness.derive(ctx, params, good).arrays()["r1is"], ref["r1is"])   # (and the good input still derives)
    # no context
    with pytest.raises(hg.HgError, match="needs a device context"):
        hg.Witness.derive(None, params, good)
    # null pointers: the C entry directly
    L = hg.lib()
    ptrs = [hg._ptr(good[f]) for f in INPUTS]
    for hole in range(4):
        h = C.c_void_p(0xDEAD)
        args = list(ptrs)
        args[hole] = None
        assert L.hg_witness_derive(ctx.h, C.byref(params), *args, C.byref(h)) == -1
        assert "null argument" in L.hg_last_error().decode() and not h.value
    assert L.hg_witness_derive(ctx.h, None, *ptrs, C.byref(C.c_void_p())) == -1
    assert L.hg_witness_derive(ctx.h, C.byref(params), *ptrs, None) == -1
    # even modulus / parameters outside the exactness argument
    bad = hg.params_builtin(n, k)
    bad.qis[0] = int(params.qis[0]) + 1
    with pytest.raises(hg.HgError, match="even"):
        hg.Witness.derive(ctx, bad, good)
    # the fused entry: host-only key, no context, a bad coefficient (no handle, error names the cause)
    bfv = hg.BfvEncrypt.new(n, k)
    pk = bfv.setup(ctx)
    pk_host = bfv.setup(None)
    vals = hg.witness_gen(ctx, pk, hg.Witness.from_arrays(params, ref))
    with pytest.raises(hg.HgError, match="host-only"):
        hg.witness_derive_into(ctx, pk_host, good, vals)
    with pytest.raises(hg.HgError, match="needs a device context"):
        hg.witness_derive_into(None, pk, good, vals)
    with pytest.raises(hg.HgError, match=r"table e: .*e_bound"):
        hg.witness_derive_into(ctx, pk, changed("e", n + 3, 20), vals)
    hw = hg.witness_derive_into(ctx, pk, good, vals)           # the values object is still usable afterwards
    same_tables(hw.arrays(), ref)
    vals.free(); pk.free(); pk_host.free()


# ---- 5. the fused path -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,k", [(4096, 2), (32768, 16)])
def test_derive_into_proves_like_the_full_witness(ctx, n, k):
    bfv = hg.BfvEncrypt.new(n, k)
    params = bfv.params
    pk = bfv.setup(ctx)
    fulls = [hg.Witness.synthetic(params, 0xFA5E + 31 * i + n).arrays() for i in range(4)]
    vals = hg.witness_gen(ctx, pk, hg.Witness.from_arrays(params, fulls[0]))
    out = hg.ProofBuffer()
    # input NodeIds in configure's order: s, e, k1 = 0, 1, 2; two Vanilla nodes; ais = 5 ..; r1is = 5 + k ..; one Vanilla node; r2is
    node_of = {"s": [0], "e": [1], "k1": [2], "ais": [5 + i for i in range(k)], "r1is": [5 + k + i for i in range(k)], "r2is": [6 + 2 * k]}
    proofs = []
    for rnd, full in enumerate(fulls[1:] + fulls[:1]):            # three refills with other secrets, then the first one again
        hw = hg.witness_derive_into(ctx, pk, {f: full[f] for f in INPUTS}, vals)
        got = hg.prove_resident(ctx, pk, vals, out).bytes()
        want, _ = bfv.prove(ctx, pk, hg.Witness.from_arrays(params, full))
        assert got == want, (rnd, len(got), len(want))
        same_tables(hw.arrays(), full)
        ok, why = hg.verify(pk, hw, got)
        assert ok, why
        ok, why = hg.verify_device(ctx, pk, hw, got)
        assert ok, why
        for f, ids in node_of.items():
            assert np.array_equal(np.concatenate([vals.node(ctx, i) for i in ids]), full[f]), (rnd, f)
        assert vals.timings["gpu_ms"] > 0 and vals.timings["total_ms"] >= vals.timings["gpu_ms"] * 0.5
        proofs.append(got)
    assert len(set(proofs)) == 4
    assert not hg.verify_device(ctx, pk, hg.Witness.from_arrays(params, fulls[1]), proofs[-1])[0]
    vals.free()
    pk.free()


# ---- 6. host side ------------------------------------------------------------------------------------------------------------------
def test_derive_without_a_context_is_an_error():
    params = hg.params_builtin(1024, 1)
    d = {"s": np.zeros(2048, dtype=np.uint64), "e": np.zeros(2048, dtype=np.uint64), "k1": np.zeros(2048, dtype=np.uint64),
         "ais": np.zeros(2048, dtype=np.uint64)}
    with pytest.raises(hg.HgError, match="no HIP device|needs a device context"):
        hg.Witness.derive(None, params, d)
    L = hg.lib()
    L.hg_witness_derive_into.argtypes = [C.c_void_p, C.c_void_p] + [hg.u64p] * 4 + [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]
    h = C.c_void_p(1)
    assert L.hg_witness_derive_into(None, None, *[hg._ptr(d[f]) for f in INPUTS], None, C.byref(h), None) == -1
    assert "needs a device context" in L.hg_last_error().decode() and not h.value


def test_derive_arithmetic_against_int128_division(tmp_path):
    """csrc/derive_math.hpp on the host (the same lines the combine kernel runs): remainder through the precomputed reciprocal,
    centred residue and exact quotient against __int128 division - random and edge operands, moduli of 2 to 61 bits."""
    exe = str(tmp_path / "derive_math_check")
    src = os.path.join(ROOT, "tests", "derive_math_check.cpp")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-x", "hip", "--cuda-host-only", src, "-o", exe,
                           "-I", os.path.join(ROOT, "hyper-greco_amd", "csrc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
