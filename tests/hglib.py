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
