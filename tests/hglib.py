"""Loads the product package (hyper-greco_amd/, C ABI over libhypergreco.so) for the tests."""
import ctypes as _C
import os
import sys

import numpy as _np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

hg = entry.load_package()


def have_gpu():
    try:
        return hg.lib().hg_device_count() > 0
    except Exception:
        return False


# ---- the kernel-level entries at their raw ABI, on numpy limb arrays (tests/test_transform_paths.py): every helper returns the entry's
# return code next to its output, takes None for a null pointer, and converts nothing -------------------------------------------------
def last_error():
    return hg.lib().hg_last_error().decode()


def _p(a):
    return None if a is None else hg._ptr(a)


def _h(ctx):
    return None if ctx is None else ctx.h


def raw_ntt(ctx, field, data, log2n, inverse, batch, out="same"):
    """hg_ntt / hg_ntt_bn254 on `data` (batch rows of 2^log2n elements as limbs) -> (rc, out); out: an array, None, or one like data"""
    if isinstance(out, str):
        out = _np.zeros_like(data)
    f = hg.lib().hg_ntt_bn254 if field == "bn254" else hg.lib().hg_ntt
    return f(_h(ctx), _p(data), log2n, 1 if inverse else 0, batch, _p(out)), out


def raw_mle_eval(ctx, field, table, nv, point, out="new"):
    """hg_mle_eval / hg_mle_eval_bn254: table 2^nv base-field elements, point nv extension elements, as limbs -> (rc, out limbs)"""
    if isinstance(out, str):
        out = _np.zeros(4 if field == "bn254" else 2, dtype=_np.uint64)
    f = hg.lib().hg_mle_eval_bn254 if field == "bn254" else hg.lib().hg_mle_eval
    return f(_h(ctx), _p(table), nv, _p(point), _p(out)), out


def raw_fold(ctx, table, nv, is_base, r, out="new"):
    """hg_fold: table 2^nv words (is_base) or (c0, c1) pairs, r two words -> (rc, out as (2^(nv-1), 2))"""
    if isinstance(out, str):
        out = _np.zeros((1 << max(nv, 1) >> 1, 2), dtype=_np.uint64)
    L = hg.lib()
    L.hg_fold.argtypes = [_C.c_void_p, hg.u64p, _C.c_size_t, _C.c_int, hg.u64p, hg.u64p]
    return L.hg_fold(_h(ctx), _p(table), nv, 1 if is_base else 0, _p(r), _p(out)), out


def _sz(vals):
    return (_C.c_size_t * max(len(vals), 1))(*[int(v) for v in vals])


def _ptrs(arrs):
    return (hg.u64p * max(len(arrs), 1))(*[_p(a) for a in arrs])


def raw_prodsum_jobs(ctx, nv, npairs, tables, eq4, kappa, chain_skip=0, sums="new", evals="new", njobs=None):
    """hg_prodsum_jobs (njobs: len(nv) unless given): nv, npairs per job; tables the flat list of every job's tables; eq4 the flat (form, z_off, w, hib) words; kappa
    the eq-factored jobs' kappas as one limb array (or None) -> (rc, sums, evals), the outputs as flat word arrays over all jobs"""
    if isinstance(sums, str):
        sums = _np.zeros(max(4 * sum(nv or [0]), 1), dtype=_np.uint64)
    if isinstance(evals, str):
        evals = _np.zeros(max(4 * sum(npairs or [0]), 1), dtype=_np.uint64)
    rc = hg.lib().hg_prodsum_jobs(_h(ctx), len(nv) if njobs is None else njobs, None if nv is None else _sz(nv), None if npairs is None else _sz(npairs),
                                  None if tables is None else _ptrs(tables), None if eq4 is None else _sz(eq4), _p(kappa), chain_skip, _p(sums), _p(evals))
    return rc, sums, evals


def raw_claim_tables_eq(ctx, n, nclaims, point_off, alpha_off, out="new"):
    """hg_claim_tables_eq: per job n and nclaims, point_off flat over all claims, alpha_off per job (None: unit weight) -> (rc, tables)"""
    if isinstance(out, str):
        out = [_np.zeros((1 << k, 2), dtype=_np.uint64) for k in n]
    al = [(1 << 64) - 1 if a is None else a for a in alpha_off]
    return hg.lib().hg_claim_tables_eq(_h(ctx), len(n), _sz(n), _sz(nclaims), _sz(point_off), _sz(al), _ptrs(out)), out


def raw_claim_tables_fft(ctx, L, inverse, nclaims, point_off, alpha_off, out="new"):
    """hg_claim_tables_fft: per job L, direction and nclaims; offsets as in raw_claim_tables_eq -> (rc, tables)"""
    if isinstance(out, str):
        out = [_np.zeros((1 << k, 2), dtype=_np.uint64) for k in L]
    al = [(1 << 64) - 1 if a is None else a for a in alpha_off]
    inv = (_C.c_int * max(len(L), 1))(*[int(bool(i)) for i in inverse])
    return hg.lib().hg_claim_tables_fft(_h(ctx), len(L), _sz(L), inv, _sz(nclaims), _sz(point_off), _sz(al), _ptrs(out)), out
