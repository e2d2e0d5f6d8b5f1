"""hyper-greco-amd: MI355X-native GKR prover for the BFV secret-key-encryption circuit.

Python host mirror of the reference's `bfv-gkr` API for this path (same names and argument meaning):
`BfvEncrypt.new(k) / setup / get_inputs / prove` [REF bfv-gkr/src/sk_encryption_circuit.rs:300-460] and
`LassoNode.prove_claim_reduction` [REF lasso/src/lasso.rs:57-114], over the C ABI of `include/hg.h`
(libhypergreco.so: hand-written HIP kernels for gfx950). There is no CPU fallback: without a HIP
device `Context()` raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("HG_LIB") or os.path.join(_HERE, "libhypergreco.so")  # HG_LIB: an experimental build (scripts/build_variant.sh)
HG_MAX_K = 16
P = 0xFFFFFFFF00000001

u64p = C.POINTER(C.c_uint64)
i64p = C.POINTER(C.c_int64)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)


class HgParams(C.Structure):
    _fields_ = [("n", C.c_uint32), ("k", C.c_uint32), ("s_bound", C.c_uint64), ("e_bound", C.c_uint64),
                ("k1_bound", C.c_uint64), ("r1_bounds", C.c_uint64 * HG_MAX_K), ("r2_bounds", C.c_uint64 * HG_MAX_K),
                ("qis", C.c_uint64 * HG_MAX_K), ("k0is", C.c_uint64 * HG_MAX_K)]


class HgTimings(C.Structure):
    _fields_ = [("witness_ms", C.c_double), ("upload_ms", C.c_double), ("prove_ms", C.c_double), ("gpu_ms", C.c_double),
                ("total_ms", C.c_double), ("enqueue_ms", C.c_double), ("sync_ms", C.c_double), ("replay_ms", C.c_double)]


class HgKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double), ("algo_bytes", C.c_double), ("model_bytes", C.c_double), ("hbm_bytes", C.c_double)]


class HgInputClaim(C.Structure):
    """hg_input_claim: a claim hg_verify_public leaves on a secret input (point_off counts coordinates of the points array)."""
    _fields_ = [("input", C.c_uint32), ("nvars", C.c_uint32), ("point_off", C.c_uint64), ("value", C.c_uint64 * 2)]


class HgInputClaimBn254(C.Structure):
    """hg_input_claim_bn254: a claim hg_verify_public_bn254 leaves on a secret input (4 canonical limbs per element)."""
    _fields_ = [("input", C.c_uint32), ("nvars", C.c_uint32), ("point_off", C.c_uint64), ("value", C.c_uint64 * 4)]


EXPORTS = [
    "hg_last_error", "hg_device_count", "hg_create", "hg_destroy", "hg_set_option", "hg_params_builtin", "hg_params_derive", "hg_grand_product", "hg_fold", "hg_setup", "hg_pk_free",
    "hg_pk_lasso_layout", "hg_pk_info", "hg_pk_node_eq_form", "hg_witness_from_json", "hg_witness_synthetic", "hg_witness_from_arrays", "hg_witness_derive", "hg_witness_derive_into",
    "hg_witness_get", "hg_witness_free", "hg_prove", "hg_warmup", "hg_prove_stream", "hg_encryption_layout", "hg_prove_encryptions", "hg_verify", "hg_verify_device", "hg_verify_device_mode", "hg_verify_device_batch",
    "hg_instance_from_ciphertext", "hg_instance_from_witness", "hg_instance_free", "hg_instance_coeffs", "hg_instance_get", "hg_pk_claim_shape", "hg_verify_public", "hg_verify_public_device", "hg_verify_public_batch", "hg_claims_settle", "hg_instance_mle", "hg_instance_mle_batch",
    "hg_pcs_commit", "hg_pcs_free", "hg_pcs_open", "hg_pcs_verify", "hg_secrets_commit", "hg_claims_open", "hg_claims_verify",
    "hg_pcs_verify_device", "hg_claims_verify_device", "hg_pcs_verify_device_batch", "hg_claims_verify_batch",
    "hg_pcs_commit_batch", "hg_secrets_commit_batch", "hg_pcs_open_batch", "hg_claims_open_batch",
    "hg_pcs_open_folded", "hg_pcs_verify_folded", "hg_pcs_verify_folded_device", "hg_claims_open_folded", "hg_claims_verify_folded", "hg_claims_verify_folded_device",
    "hg_pcs_open_folded_batch", "hg_claims_open_folded_batch", "hg_pcs_verify_folded_device_batch", "hg_claims_verify_folded_batch",
    "hg_secrets_commit_values", "hg_prove_encryptions_committed", "hg_prove_encryptions_committed_bn254",
    "hg_instance_digest", "hg_instance_digest_batch", "hg_values_instance_digest", "hg_bound_seed", "hg_prove_committed_mode", "hg_verify_public_bound", "hg_verify_public_bound_device",
    "hg_verify_public_bound_batch", "hg_instance_digest_group",
    "hg_pcs_commit_bn254", "hg_pcs_open_bn254", "hg_pcs_verify_bn254", "hg_secrets_commit_bn254", "hg_claims_open_bn254", "hg_claims_verify_bn254",
    "hg_pcs_verify_device_bn254", "hg_claims_verify_device_bn254", "hg_pcs_verify_device_batch_bn254", "hg_claims_verify_batch_bn254",
    "hg_pcs_open_folded_bn254", "hg_pcs_verify_folded_bn254", "hg_pcs_verify_folded_device_bn254", "hg_claims_open_folded_bn254", "hg_claims_verify_folded_bn254",
    "hg_claims_verify_folded_device_bn254",
    "hg_pcs_open_folded_batch_bn254", "hg_claims_open_folded_batch_bn254", "hg_pcs_verify_folded_device_batch_bn254", "hg_claims_verify_folded_batch_bn254",
    "hg_pcs_commit_batch_bn254", "hg_secrets_commit_batch_bn254", "hg_pcs_open_batch_bn254", "hg_claims_open_batch_bn254",
    "hg_prove_mode", "hg_prove_resident_mode", "hg_verify_mode", "hg_group_local", "hg_group_external", "hg_group_free", "hg_prove_resident_mode_sharded", "hg_witness_gen", "hg_witness_gen_into", "hg_witness_gen_shard", "hg_values_info", "hg_values_peak_bytes", "hg_values_free", "hg_values_get", "hg_comm_unique_id", "hg_comm_init", "hg_comm_destroy", "hg_comm_count", "hg_comm_selftest", "hg_prove_sharded", "hg_prove_shard_begin", "hg_prove_shard_combine", "hg_prove_shard_finish", "hg_shard_combine_host", "hg_prove_resident", "hg_circuit_eval", "hg_lasso_prove", "hg_lasso_prove_at", "hg_lasso_num_challenges", "hg_sumcheck", "hg_prodsum_jobs", "hg_claim_tables_eq", "hg_claim_tables_fft", "hg_mle_eval",
    "hg_ntt", "hg_challenges", "hg_challenges_bn254", "hg_bn254_field_op", "hg_sumcheck_bn254", "hg_prodsum_jobs_bn254", "hg_grand_product_bn254", "hg_lasso_prove_bn254", "hg_witness_from_json_bn254", "hg_circuit_eval_bn254", "hg_prove_bn254", "hg_verify_bn254", "hg_verify_device_bn254", "hg_verify_device_batch_bn254", "hg_verify_public_bn254", "hg_verify_public_device_bn254", "hg_verify_public_batch_bn254", "hg_claims_settle_bn254", "hg_instance_mle_bn254", "hg_instance_mle_batch_bn254", "hg_prove_encryptions_bn254", "hg_mle_eval_bn254", "hg_ntt_bn254", "hg_profile", "hg_profile_select", "hg_profile_reset", "hg_profile_get",
]


def build(force=False):
    """Compiles csrc/ for gfx950 into libhypergreco.so (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "clean"])
    subprocess.check_call(["make", "-C", src, "-j4"])
    return _LIB_PATH


def _two_field_protos(L):
    """the verifier, instance and commitment entries: the two fields have the same C types (an element is 2 or 4 words behind a
    pointer); the Goldilocks entries with protocol modes take an int where marked"""
    vp, sz, ci, cp, szp = C.c_void_p, C.c_size_t, C.c_int, C.c_char_p, C.POINTER(C.c_size_t)
    L.hg_verify_mode.argtypes = [vp, vp, ci, cp, sz]
    L.hg_verify_device.argtypes = L.hg_verify_device_bn254.argtypes = [vp, vp, vp, cp, sz]
    L.hg_verify_device_mode.argtypes = [vp, vp, vp, ci, cp, sz]
    L.hg_instance_from_ciphertext.argtypes = [C.POINTER(HgParams), i64p, i64p, C.POINTER(vp)]
    L.hg_instance_from_witness.argtypes = [C.POINTER(HgParams), vp, C.POINTER(vp)]
    L.hg_instance_coeffs.argtypes = [vp, i64p, i64p]
    L.hg_instance_get.argtypes, L.hg_instance_get.restype = [vp, ci, u64p, sz], C.c_int64
    L.hg_instance_free.argtypes = [vp]
    L.hg_pk_claim_shape.argtypes = [vp, szp, szp]
    batch = [vp, vp, C.POINTER(vp), C.POINTER(cp), szp, sz]          # ctx, key, handles, proofs, lengths, n
    room = [vp, sz, u64p, sz, szp]                                    # claims, their capacity, points, their capacity, claims written
    for sfx, mode in (("", [ci]), ("_bn254", [])):
        getattr(L, "hg_verify_device_batch" + sfx).argtypes = batch + mode + [C.POINTER(ci), cp, sz]
        getattr(L, "hg_verify_public_batch" + sfx).argtypes = batch + mode + [C.POINTER(ci)] + room + [cp, sz]
        getattr(L, "hg_verify_public" + sfx).argtypes = [vp, vp] + mode + [cp, sz] + room
        getattr(L, "hg_verify_public_device" + sfx).argtypes = [vp, vp, vp] + mode + [cp, sz] + room
        getattr(L, "hg_claims_settle" + sfx).argtypes = [vp, C.POINTER(HgParams), vp, vp, sz, u64p]
        getattr(L, "hg_instance_mle" + sfx).argtypes = [vp, vp, ci, ci, u64p, sz, u64p]
        getattr(L, "hg_instance_mle_batch" + sfx).argtypes = [vp, C.POINTER(vp), sz, ci, ci, u64p, sz, u64p]
        getattr(L, "hg_pcs_commit" + sfx).argtypes = [vp, C.POINTER(u64p), u32p, sz, sz, C.POINTER(vp), u8p]
        getattr(L, "hg_pcs_open" + sfx).argtypes = [vp, vp, u32p, u64p, u64p, sz, sz, u8p, sz, szp]
        getattr(L, "hg_pcs_verify" + sfx).argtypes = [cp, u32p, sz, sz, u32p, u64p, u64p, sz, sz, cp, sz]
        getattr(L, "hg_secrets_commit" + sfx).argtypes = [vp, C.POINTER(HgParams), vp, sz, C.POINTER(vp), u8p]
        getattr(L, "hg_claims_open" + sfx).argtypes = [vp, C.POINTER(HgParams), vp, vp, sz, u64p, sz, u8p, sz, szp]
        getattr(L, "hg_claims_verify" + sfx).argtypes = [C.POINTER(HgParams), cp, sz, vp, sz, u64p, sz, cp, sz]
        getattr(L, "hg_pcs_verify_device" + sfx).argtypes = [vp] + getattr(L, "hg_pcs_verify" + sfx).argtypes
        getattr(L, "hg_claims_verify_device" + sfx).argtypes = [vp] + getattr(L, "hg_claims_verify" + sfx).argtypes
    for sfx in ("", "_bn254"):   # the folded forms take what the unfolded ones take
        for name in ("hg_pcs_open", "hg_pcs_verify", "hg_claims_open", "hg_claims_verify", "hg_pcs_verify_device", "hg_claims_verify_device"):
            folded = name.replace("_device", "") + "_folded" + ("_device" if name.endswith("_device") else "") + sfx
            getattr(L, folded).argtypes = getattr(L, name + sfx).argtypes
    L.hg_pcs_free.argtypes, L.hg_pcs_free.restype = [vp], None
    tail = [szp, sz, C.POINTER(cp), szp, sz, C.POINTER(ci), cp, sz]   # claim counts, n_queries, openings, lengths, n, results, reasons, reason_cap
    L.hg_pcs_verify_device_batch.argtypes = L.hg_pcs_verify_device_batch_bn254.argtypes = [vp, C.POINTER(cp), u32p, sz, sz, C.POINTER(u32p), C.POINTER(u64p), C.POINTER(u64p)] + tail
    L.hg_claims_verify_batch.argtypes = L.hg_claims_verify_batch_bn254.argtypes = [vp, C.POINTER(HgParams), C.POINTER(cp), sz, vp, sz, u64p, sz] + tail
    L.hg_pcs_commit_batch.argtypes = L.hg_pcs_commit_batch_bn254.argtypes = [vp, C.POINTER(C.POINTER(u64p)), u32p, sz, sz, sz, C.POINTER(vp), u8p]
    L.hg_secrets_commit_batch.argtypes = L.hg_secrets_commit_batch_bn254.argtypes = [vp, C.POINTER(HgParams), C.POINTER(vp), sz, sz, C.POINTER(vp), u8p]
    L.hg_secrets_commit_values.argtypes = [vp, vp, vp, sz, C.POINTER(vp), u8p]   # ctx, key, values, log2_row, handle out, root out
    # bound proofs: a 32-byte root or digest goes in as bytes and comes out through a u8 array
    L.hg_instance_digest.argtypes = [vp, vp, u8p]
    L.hg_instance_digest_batch.argtypes = [vp, C.POINTER(vp), sz, u8p]
    L.hg_values_instance_digest.argtypes = [vp, vp, vp, u8p]
    L.hg_bound_seed.argtypes = [C.POINTER(HgParams), ci, cp, cp, u8p, sz, szp]
    L.hg_prove_committed_mode.argtypes = [vp, vp, vp, ci, sz, vp, sz, szp, C.POINTER(vp), u8p, C.POINTER(HgTimings)]
    L.hg_verify_public_bound.argtypes = [vp, vp, ci, cp, cp, sz] + room
    L.hg_verify_public_bound_device.argtypes = [vp, vp, vp, ci, cp, cp, sz] + room
    L.hg_verify_public_bound_batch.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(cp), C.POINTER(cp), szp, sz, ci, C.POINTER(ci)] + room + [u8p, cp, sz]
    L.hg_instance_digest_group.argtypes = [vp, C.POINTER(vp), sz, u8p]
    pp = C.POINTER(i64p)
    L.hg_prove_encryptions_committed.argtypes = L.hg_prove_encryptions_committed_bn254.argtypes = [
        vp, vp, pp, pp, pp, pp, sz, sz, vp, sz, szp, C.POINTER(ci), C.POINTER(vp), u8p, C.POINTER(vp), cp, sz, C.POINTER(HgTimings)]
    opened = [szp, sz, sz, u8p, sz, szp, C.POINTER(ci), cp, sz]   # claim counts, n_queries, n, openings, cap_each, lengths, status, reasons, reason_cap
    L.hg_pcs_open_batch.argtypes = L.hg_pcs_open_batch_bn254.argtypes = [vp, C.POINTER(vp), C.POINTER(u32p), C.POINTER(u64p), C.POINTER(u64p)] + opened
    L.hg_claims_open_batch.argtypes = L.hg_claims_open_batch_bn254.argtypes = [vp, C.POINTER(HgParams), C.POINTER(vp), vp, sz, u64p, sz] + opened
    # the batch forms of the folded openings take what the unfolded batch forms take
    L.hg_pcs_open_folded_batch.argtypes, L.hg_claims_open_folded_batch.argtypes = L.hg_pcs_open_batch.argtypes, L.hg_claims_open_batch.argtypes
    L.hg_pcs_verify_folded_device_batch.argtypes, L.hg_claims_verify_folded_batch.argtypes = L.hg_pcs_verify_device_batch.argtypes, L.hg_claims_verify_batch.argtypes
    L.hg_pcs_open_folded_batch_bn254.argtypes, L.hg_claims_open_folded_batch_bn254.argtypes = L.hg_pcs_open_batch.argtypes, L.hg_claims_open_batch.argtypes
    L.hg_pcs_verify_folded_device_batch_bn254.argtypes, L.hg_claims_verify_folded_batch_bn254.argtypes = L.hg_pcs_verify_device_batch.argtypes, L.hg_claims_verify_batch.argtypes


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} is missing: run __graft_entry__.build() (the HIP extension is required)")
        L = C.CDLL(_LIB_PATH)
        L.hg_last_error.restype = C.c_char_p
        L.hg_create.restype = C.c_void_p
        L.hg_create.argtypes = [C.c_int]
        L.hg_destroy.argtypes = [C.c_void_p]
        L.hg_setup.argtypes = [C.c_void_p, C.POINTER(HgParams), C.POINTER(C.c_void_p)]
        L.hg_pk_free.argtypes = [C.c_void_p]
        L.hg_pk_lasso_layout.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.hg_pk_info.argtypes = [C.c_void_p, u64p]
        L.hg_witness_from_json.argtypes = [C.POINTER(HgParams), C.c_char_p, C.POINTER(C.c_void_p)]
        L.hg_witness_synthetic.argtypes = [C.POINTER(HgParams), C.c_uint64, C.POINTER(C.c_void_p)]
        L.hg_witness_from_arrays.argtypes = [C.POINTER(HgParams)] + [u64p] * 7 + [C.POINTER(C.c_void_p)]
        L.hg_witness_get.restype = C.c_int64
        L.hg_witness_get.argtypes = [C.c_void_p, C.c_int, u64p, C.c_size_t]
        L.hg_witness_free.argtypes = [C.c_void_p]
        L.hg_prove.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
        L.hg_witness_gen.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(HgTimings)]
        L.hg_witness_gen_into.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(HgTimings)]
        L.hg_values_free.argtypes = [C.c_void_p]
        L.hg_values_get.restype = C.c_int64
        L.hg_values_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int, u64p, C.c_size_t]
        L.hg_prove_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
        L.hg_prove_shard_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(u64p), C.POINTER(C.c_size_t)]
        L.hg_prove_shard_combine.argtypes = [C.c_void_p, u64p, C.c_int, C.c_size_t]
        L.hg_prove_shard_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
        L.hg_verify.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.hg_verify_bn254.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.hg_circuit_eval.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_size_t, u64p, C.c_size_t]
        L.hg_lasso_prove.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), u64p]
        L.hg_lasso_prove_at.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), u64p]
        L.hg_sumcheck.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(u64p), C.POINTER(C.c_int), u64p, C.c_size_t,
                                  u64p, C.c_size_t, u64p, u64p, u64p, u64p]
        L.hg_prodsum_jobs.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(u64p), C.POINTER(C.c_size_t),
                                      u64p, C.c_size_t, u64p, u64p]
        L.hg_claim_tables_eq.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_size_t), C.POINTER(u64p)]
        L.hg_claim_tables_fft.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(u64p)]
        L.hg_mle_eval.argtypes = [C.c_void_p, u64p, C.c_size_t, u64p, u64p]
        L.hg_ntt.argtypes = [C.c_void_p, u64p, C.c_size_t, C.c_int, C.c_size_t, u64p]
        L.hg_challenges.argtypes = [C.c_size_t, u64p]
        L.hg_challenges_bn254.argtypes = [C.c_size_t, u64p]
        L.hg_bn254_field_op.argtypes = [C.c_void_p, C.c_int, C.c_size_t, u64p, u64p, u64p]
        L.hg_sumcheck_bn254.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(u64p), u64p, C.c_size_t, u64p, C.c_size_t,
                                        u64p, u64p, u64p, u64p]
        L.hg_prodsum_jobs_bn254.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(u64p), C.POINTER(C.c_size_t),
                                            C.c_size_t, u64p, u64p]
        L.hg_grand_product_bn254.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(u64p), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t,
                                             C.POINTER(C.c_size_t), u64p, u64p]
        L.hg_lasso_prove_bn254.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), u64p]
        L.hg_mle_eval_bn254.argtypes = [C.c_void_p, u64p, C.c_size_t, u64p, u64p]
        L.hg_witness_from_json_bn254.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
        L.hg_circuit_eval_bn254.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, u64p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.hg_prove_bn254.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double)]
        L.hg_ntt_bn254.argtypes = [C.c_void_p, u64p, C.c_size_t, C.c_int, C.c_size_t, u64p]
        L.hg_profile.argtypes = [C.c_void_p, C.c_int]
        L.hg_profile_select.argtypes = [C.c_void_p, C.c_char_p]
        L.hg_profile_reset.argtypes = [C.c_void_p]
        L.hg_profile_get.argtypes = [C.c_void_p, C.POINTER(HgKernelStat), C.c_int]
        _two_field_protos(L)
        _lib = L
    return _lib


class HgError(RuntimeError):
    pass


def _check(rc):
    if rc is None or (isinstance(rc, int) and rc < 0):
        raise HgError(lib().hg_last_error().decode())
    return rc


def _ptr(a):
    return a.ctypes.data_as(u64p)


def params_builtin(n, k):
    p = HgParams()
    _check(lib().hg_params_builtin(n, k, C.byref(p)))
    return p


def challenges(n):
    out = np.zeros(n, dtype=np.uint64)
    _check(lib().hg_challenges(n, _ptr(out)))
    return out


class Context:
    """One per GPU (hg_ctx): HIP stream, workspace arena, challenge chain in HBM."""

    def __init__(self, device=0):
        h = lib().hg_create(device)
        if not h:
            raise HgError(lib().hg_last_error().decode())
        self.h = C.c_void_p(h)

    def close(self):
        if self.h:
            lib().hg_destroy(self.h)
            self.h = None

    def set_option(self, name, value):
        """hg_set_option: "one_stream" (1 = no cross-stream overlap, for per-kernel timings), "gp_claims_device" (0 = the grand
        products' layer claims in the transcript replay instead of the tail kernel), ... (include/hg.h)."""
        L = lib()
        L.hg_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        if L.hg_set_option(self.h, name.encode(), int(value)) != 0:
            raise HgError(L.hg_last_error().decode())

    def profile(self, level):
        lib().hg_profile(self.h, level)

    def profile_select(self, name):
        _check(lib().hg_profile_select(self.h, name.encode()))

    def profile_reset(self):
        lib().hg_profile_reset(self.h)

    def profile_get(self, cap=32):
        arr = (HgKernelStat * cap)()
        n = lib().hg_profile_get(self.h, arr, cap)
        return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), total_ms=arr[i].total_ms, algo_bytes=arr[i].algo_bytes, model_bytes=arr[i].model_bytes, hbm_bytes=arr[i].hbm_bytes)
                for i in range(n)]

    # ---- BN254 slice: elements are Python ints at this level, 4 little-endian u64 limbs at the C ABI; a long table may be given as
    # the limbs themselves, an (n, 4) uint64 array, which is passed on as it is
    @staticmethod
    def _fr_pack(vals):
        if isinstance(vals, np.ndarray) and vals.ndim == 2:
            if vals.shape[1] != 4 or vals.dtype != np.uint64:
                raise ValueError("a limb table is an (n, 4) uint64 array")
            return np.ascontiguousarray(vals).reshape(-1)
        a = np.zeros((len(vals), 4), dtype=np.uint64)
        for i, v in enumerate(vals):
            for k in range(4):
                a[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
        return a.reshape(-1)

    @staticmethod
    def _fr_unpack(a):
        a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
        return [sum(int(a[i, k]) << (64 * k) for k in range(4)) for i in range(a.shape[0])]

    def bn254_field_op(self, op, a, b):
        pa, pb = self._fr_pack(a), self._fr_pack(b)
        out = np.zeros_like(pa)
        _check(lib().hg_bn254_field_op(self.h, op, len(a), _ptr(pa), _ptr(pb), _ptr(out)))
        return self._fr_unpack(out)

    def grand_product_bn254(self, tables, chain_skip=0):
        """prove_grand_product over bn256::Fr: (proof bytes, final claims, point)."""
        nb, ln = len(tables), len(tables[0])
        nv = ln.bit_length() - 1
        packed = [self._fr_pack(t) for t in tables]
        ptrs = (u64p * nb)(*[_ptr(t) for t in packed])
        cap = 32 * (nb + sum(4 * n + 2 * nb for n in range(nv)) + 2 * nb + 64)
        buf = (C.c_uint8 * cap)()
        ln_out = C.c_size_t(0)
        claims = np.zeros(nb * 4, dtype=np.uint64)
        point = np.zeros(max(nv, 1) * 4, dtype=np.uint64)
        _check(lib().hg_grand_product_bn254(self.h, nb, ln, ptrs, chain_skip, buf, cap, C.byref(ln_out), _ptr(claims), _ptr(point)))
        return C.string_at(buf, ln_out.value), self._fr_unpack(claims), self._fr_unpack(point)[:nv]

    def lasso_prove_bn254(self, pk, lasso_in, chain_skip=0, cap=1 << 22):
        """LassoNode::prove_claim_reduction over bn256::Fr on a table of small integers: (proof bytes, r, claimed sum)."""
        n = len(lasso_in)
        nu = n.bit_length() - 1
        packed = self._fr_pack(lasso_in)
        buf = (C.c_uint8 * cap)()
        ln = C.c_size_t(0)
        claim = np.zeros((nu + 1) * 4, dtype=np.uint64)
        _check(lib().hg_lasso_prove_bn254(self.h, pk.h, _ptr(packed), chain_skip, buf, cap, C.byref(ln), _ptr(claim)))
        vals = self._fr_unpack(claim)
        return C.string_at(buf, ln.value), vals[:nu], vals[nu]

    def circuit_eval_bn254(self, pk, witness, which):
        """Circuit::evaluate over bn256::Fr: which = 0 the sum node, 1 the Lasso input node, 2 the ct0is table (Python ints)."""
        n = C.c_size_t(0)
        cap = 1 << (pk.params.n.bit_length() + 6)
        out = np.zeros(cap * 4, dtype=np.uint64)
        _check(lib().hg_circuit_eval_bn254(self.h, pk.h, witness.h, which, _ptr(out), cap, C.byref(n)))
        return self._fr_unpack(out[:n.value * 4])

    def prove_bn254(self, pk, witness, cap=1 << 24):
        """BfvEncrypt::prove over bn256::Fr: (proof bytes, witness-generation ms, prove ms)."""
        buf = (C.c_uint8 * cap)()
        ln = C.c_size_t(0)
        ms = (C.c_double * 2)()
        _check(lib().hg_prove_bn254(self.h, pk.h, witness.h, buf, cap, C.byref(ln), ms))
        return C.string_at(buf, ln.value), ms[0], ms[1]

    def mle_eval_bn254(self, table, point):
        nv = (len(table) - 1).bit_length()
        pt, pp = self._fr_pack(table), self._fr_pack(point) if len(point) else np.zeros(4, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().hg_mle_eval_bn254(self.h, _ptr(pt), nv, _ptr(pp), _ptr(out)))
        return self._fr_unpack(out)[0]

    def ntt_bn254(self, rows, inverse=False):
        """rows: list of equal-length lists (a batch of transforms)."""
        n = len(rows[0])
        flat = self._fr_pack([v for r in rows for v in r])
        out = np.zeros_like(flat)
        _check(lib().hg_ntt_bn254(self.h, _ptr(flat), n.bit_length() - 1, 1 if inverse else 0, len(rows), _ptr(out)))
        vals = self._fr_unpack(out)
        return [vals[i * n:(i + 1) * n] for i in range(len(rows))]

    def sumcheck_bn254(self, kind, tables, pw, claim, chain_skip=0):
        """gkr::sum_check::prove_sum_check over bn256::Fr: (msgs, point, evals, sums) as lists of ints."""
        ntab = len(tables)
        nv = (len(tables[0]) - 1).bit_length()
        d = 3 if kind == 1 else 2
        packed = [self._fr_pack(t) for t in tables]
        ptrs = (u64p * ntab)(*[_ptr(t) for t in packed])
        ppw = self._fr_pack(pw) if len(pw) else np.zeros(4, dtype=np.uint64)
        pcl = self._fr_pack([claim])
        msgs = np.zeros(max(nv * (d + 1), 1) * 4, dtype=np.uint64)
        point = np.zeros(max(nv, 1) * 4, dtype=np.uint64)
        evals = np.zeros(ntab * 4, dtype=np.uint64)
        sums = np.zeros(max(nv * d, 1) * 4, dtype=np.uint64)
        _check(lib().hg_sumcheck_bn254(self.h, kind, nv, ntab, ptrs, _ptr(ppw), len(pw), _ptr(pcl), chain_skip, _ptr(msgs), _ptr(point),
                                       _ptr(evals), _ptr(sums)))
        m = self._fr_unpack(msgs)[: nv * (d + 1)]
        return ([m[i * (d + 1):(i + 1) * (d + 1)] for i in range(nv)], self._fr_unpack(point)[:nv], self._fr_unpack(evals),
                [self._fr_unpack(sums)[i * d:(i + 1) * d] for i in range(nv)])

    def prodsum_jobs_bn254(self, jobs, chain_skip=0):
        """hg_prodsum_jobs_bn254: the prover's PRODSUM launches on a batch of jobs, one flush. jobs: [(tables, window)] with tables =
        [a_0, b_0, a_1, b_1, ..] (lists of ints or (n, 4) limb arrays; the same OBJECT in several places is uploaded from one
        pointer, which is what selects the shared-b form) and window = (lo, hi) or None. -> per job (sums [[g(0), g(2)]] per round,
        evals [2 npairs]) as ints."""
        packed = {}

        def pk(t):
            if id(t) not in packed:
                packed[id(t)] = self._fr_pack(t)
            return packed[id(t)]
        nj = len(jobs)
        nvs = [(len(tabs[0]) - 1).bit_length() if len(tabs) else 0 for tabs, _ in jobs]
        nps = [len(tabs) // 2 for tabs, _ in jobs]
        flat = [pk(t) for tabs, _ in jobs for t in tabs]
        ptrs = (u64p * max(len(flat), 1))(*[_ptr(t) for t in flat])
        sz = C.c_size_t * max(nj, 1)
        win = (C.c_size_t * max(2 * nj, 1))(*[int(x) for _, w in jobs for x in (w or (0, 0))])
        sums = np.zeros(max(2 * sum(nvs), 1) * 4, dtype=np.uint64)
        evals = np.zeros(max(2 * sum(nps), 1) * 4, dtype=np.uint64)
        _check(lib().hg_prodsum_jobs_bn254(self.h, nj, sz(*nvs), sz(*nps), ptrs, win, chain_skip, _ptr(sums), _ptr(evals)))
        s, e, out, so, eo = self._fr_unpack(sums), self._fr_unpack(evals), [], 0, 0
        for nv, np_ in zip(nvs, nps):
            out.append(([s[so + 2 * i:so + 2 * i + 2] for i in range(nv)], e[eo:eo + 2 * np_]))
            so, eo = so + 2 * nv, eo + 2 * np_
        return out

    # kernel-level entry points (parity tests)
    def sumcheck(self, kind, tables, is_base, pw, claim, chain_skip=0):
        ntab = len(tables)
        nv = int(np.log2(tables[0].size if is_base[0] else tables[0].size // 2))
        d = 3 if kind == 1 else 2
        tabs = [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
        ptrs = (u64p * ntab)(*[_ptr(t) for t in tabs])
        flags = (C.c_int * ntab)(*[int(b) for b in is_base])
        pw = np.ascontiguousarray(pw, dtype=np.uint64).reshape(-1)
        claim = np.ascontiguousarray(claim, dtype=np.uint64)
        msgs = np.zeros(nv * (d + 1) * 2, dtype=np.uint64)
        point = np.zeros(nv * 2, dtype=np.uint64)
        evals = np.zeros(ntab * 2, dtype=np.uint64)
        sums = np.zeros(nv * d * 2, dtype=np.uint64)
        _check(lib().hg_sumcheck(self.h, kind, nv, ntab, ptrs, flags, _ptr(pw), pw.size // 2, _ptr(claim), chain_skip,
                                 _ptr(msgs), _ptr(point), _ptr(evals), _ptr(sums)))
        return msgs, point, evals, sums

    def mle_eval(self, table, point):
        table = np.ascontiguousarray(table, dtype=np.uint64)
        point = np.ascontiguousarray(point, dtype=np.uint64)
        out = np.zeros(2, dtype=np.uint64)
        _check(lib().hg_mle_eval(self.h, _ptr(table), point.size // 2, _ptr(point), _ptr(out)))
        return out

    def ntt(self, data, log2n, inverse=False, batch=1):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        out = np.zeros_like(data)
        _check(lib().hg_ntt(self.h, _ptr(data), log2n, int(inverse), batch, _ptr(out)))
        return out


class Witness:
    """BfvSkEncryptArgs after get_inputs [REF sk_encryption_circuit.rs:64-73, 365-415]."""
    FIELDS = ["s", "e", "k1", "ais", "r1is", "r2is", "ct0is"]

    def __init__(self, handle, params):
        self.h = handle
        self.params = params

    @classmethod
    def from_json(cls, params, path):
        h = C.c_void_p()
        _check(lib().hg_witness_from_json(C.byref(params), path.encode(), C.byref(h)))
        return cls(h, params)

    @classmethod
    def from_json_bn254(cls, params, path):
        """One of the reference's bn254 fixtures (elements of bn256::Fr holding small signed integers)."""
        h = C.c_void_p()
        _check(lib().hg_witness_from_json_bn254(C.byref(params), path.encode(), C.byref(h)))
        return cls(h, params)

    @classmethod
    def synthetic(cls, params, seed):
        h = C.c_void_p()
        _check(lib().hg_witness_synthetic(C.byref(params), seed, C.byref(h)))
        return cls(h, params)

    @classmethod
    def from_arrays(cls, params, d):
        h = C.c_void_p()
        arrs = [np.ascontiguousarray(d[f], dtype=np.uint64) for f in cls.FIELDS]
        _check(lib().hg_witness_from_arrays(C.byref(params), *[_ptr(a) for a in arrs], C.byref(h)))
        return cls(h, params)

    @staticmethod
    def _derive_inputs(params, d):
        arrs = [np.ascontiguousarray(d[f], dtype=np.uint64) for f in ("s", "e", "k1", "ais")]
        sz = 2 * params.n
        if [a.size for a in arrs] != [sz, sz, sz, params.k * sz]:
            raise ValueError("derive: s, e, k1 hold 2n words and ais k * 2n")
        return arrs

    @classmethod
    def derive(cls, ctx, params, d):
        """hg_witness_derive: ct0is, r2is, r1is from the laid-out tables d['s'], d['e'], d['k1'], d['ais'] on the device."""
        h = C.c_void_p()
        arrs = cls._derive_inputs(params, d)
        L = lib()
        L.hg_witness_derive.argtypes = [C.c_void_p, C.POINTER(HgParams)] + [u64p] * 4 + [C.POINTER(C.c_void_p)]
        _check(L.hg_witness_derive(ctx.h if ctx is not None else None, C.byref(params), *[_ptr(a) for a in arrs], C.byref(h)))
        return cls(h, params)

    def arrays(self):
        out = {}
        for i, f in enumerate(self.FIELDS):
            n = lib().hg_witness_get(self.h, i, None, 0)
            a = np.zeros(n, dtype=np.uint64)
            lib().hg_witness_get(self.h, i, _ptr(a), n)
            out[f] = a
        return out

    def __del__(self):
        try:
            if self.h:
                lib().hg_witness_free(self.h)
                self.h = None
        except Exception:
            pass


class ProverKey:
    def __init__(self, handle, params):
        self.h = handle
        self.params = params
        info = (C.c_uint64 * 6)()
        lib().hg_pk_info(self.h, info)
        self.nu, self.num_nodes, self.rows, self.alpha, self.lasso_in_id, self.sum_id = (int(x) for x in info)

    def lasso_layout(self):
        buf = C.create_string_buffer(1 << 16)
        _check(lib().hg_pk_lasso_layout(self.h, buf, 1 << 16))
        mems, lk = buf.value.decode().split("|")
        return mems.split(","), lk.split(";")

    def node_eq_form(self, node):
        """hg_pk_node_eq_form: how setup classified a node - dict(kind, eq_form, block_log2, window, terms, in_log2)."""
        out = (C.c_int64 * 6)()
        L = lib()
        L.hg_pk_node_eq_form.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        _check(L.hg_pk_node_eq_form(self.h, int(node), out))
        return {"kind": ("input", "vanilla", "fft", "lasso")[int(out[0])], "eq_form": bool(out[1]), "block_log2": int(out[2]), "window": int(out[3]),
                "terms": int(out[4]), "in_log2": int(out[5])}

    def circuit_eval(self, w):
        lasso_in = np.zeros(1 << self.nu, dtype=np.uint64)
        sum_out = np.zeros(self.params.k * 2 * self.params.n, dtype=np.uint64)
        _check(lib().hg_circuit_eval(self.h, w.h, _ptr(lasso_in), lasso_in.size, _ptr(sum_out), sum_out.size))
        return lasso_in, sum_out

    def free(self):
        if self.h:
            lib().hg_pk_free(self.h)
            self.h = None


class BfvEncrypt:
    """Mirror of `BfvEncrypt::<Params, K>` [REF sk_encryption_circuit.rs:300-523]."""

    def __init__(self, n, k=None):  # = BfvEncrypt::<SkEnc{n}_{k}x.._65537, k>::new(k); or BfvEncrypt(params) with a derived HgParams
        self.params = n if isinstance(n, HgParams) else params_builtin(n, k)

    @classmethod
    def new(cls, n, k):
        return cls(n, k)

    def setup(self, ctx):  # -> (pk); the verifier key of the reference is the same preprocessing
        h = C.c_void_p()
        _check(lib().hg_setup(ctx.h if ctx is not None else None, C.byref(self.params), C.byref(h)))
        return ProverKey(h, self.params)

    def warmup(self, ctx, pk):
        """hg_warmup: context-owned tables, witness staging and the recorded launch graph ahead of the first prove; returns the ms it took."""
        L = lib()
        L.hg_warmup.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.hg_warmup.restype = C.c_int
        ms = C.c_double(0)
        _check(L.hg_warmup(ctx.h, pk.h, C.byref(ms)))
        return ms.value

    def get_inputs(self, path):
        return Witness.from_json(self.params, path)

    def prove(self, ctx, pk, witness, cap=1 << 24, mode=0):
        """BfvEncrypt::prove; mode != 0: hg_prove_mode (bit 0 absorbing transcript, bit 1 extension-field memory checking)."""
        buf = (C.c_uint8 * cap)()
        ln = C.c_size_t(0)
        tm = HgTimings()
        L = lib()
        if mode:
            L.hg_prove_mode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
            _check(L.hg_prove_mode(ctx.h, pk.h, witness.h, mode, buf, cap, C.byref(ln), C.byref(tm)))
        else:
            _check(L.hg_prove(ctx.h, pk.h, witness.h, buf, cap, C.byref(ln), C.byref(tm)))
        return C.string_at(buf, ln.value), {f: getattr(tm, f) for f, _ in HgTimings._fields_}

    def prove_stream(self, ctx, pk, witnesses, cap_each=1 << 20):
        """hg_prove_stream: BfvEncrypt::prove for a run of witnesses, witness i+1's upload + evaluate under witness i's prove."""
        n = len(witnesses)
        L = lib()
        L.hg_prove_stream.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
        L.hg_prove_stream.restype = C.c_int
        hs = (C.c_void_p * max(n, 1))(*[w.h for w in witnesses])
        buf = (C.c_uint8 * (cap_each * max(n, 1)))()
        lens = (C.c_size_t * max(n, 1))()
        tm = HgTimings()
        _check(L.hg_prove_stream(ctx.h, pk.h, hs, n, buf, cap_each, lens, C.byref(tm)))
        raw = memoryview(buf)
        proofs = [bytes(raw[i * cap_each:i * cap_each + lens[i]]) for i in range(n)]
        return proofs, {f: getattr(tm, f) for f, _ in HgTimings._fields_}


class ResidentValues:
    """circuit.evaluate() output kept in HBM (hg_values)."""

    def __init__(self, handle, timings):
        self.h = handle
        self.timings = timings

    def node(self, ctx, node_id):
        n = lib().hg_values_get(ctx.h, self.h, node_id, None, 0)
        if n < 0:
            raise HgError(lib().hg_last_error().decode())
        a = np.zeros(n, dtype=np.uint64)
        lib().hg_values_get(ctx.h, self.h, node_id, _ptr(a), n)
        return a

    def info(self):
        """hg_values_info: resident bytes, bytes of the full table set, resident tables, tables."""
        out = (C.c_uint64 * 4)()
        L = lib()
        L.hg_values_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _check(L.hg_values_info(self.h, out))
        L.hg_values_peak_bytes.argtypes = [C.c_void_p]
        L.hg_values_peak_bytes.restype = C.c_int64
        return {"resident_bytes": int(out[0]), "full_bytes": int(out[1]), "resident_tables": int(out[2]), "tables": int(out[3]),
                "peak_bytes": int(L.hg_values_peak_bytes(self.h))}

    def free(self):
        if self.h:
            lib().hg_values_free(self.h)
            self.h = None


def witness_gen(ctx, pk, witness):
    h = C.c_void_p()
    tm = HgTimings()
    _check(lib().hg_witness_gen(ctx.h, pk.h, witness.h, C.byref(h), C.byref(tm)))
    return ResidentValues(h, {f: getattr(tm, f) for f, _ in HgTimings._fields_})


def witness_gen_shard(ctx, pk, witness, rank, world):
    """hg_witness_gen_shard: circuit.evaluate() keeping only the tables rank `rank` of a `world`-GPU proof reads."""
    h = C.c_void_p()
    tm = HgTimings()
    L = lib()
    L.hg_witness_gen_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(HgTimings)]
    _check(L.hg_witness_gen_shard(ctx.h, pk.h, witness.h, rank, world, C.byref(h), C.byref(tm)))
    return ResidentValues(h, {f: getattr(tm, f) for f, _ in HgTimings._fields_})


def witness_gen_into(ctx, pk, witness, values):
    """hg_witness_gen_into: circuit.evaluate() of another witness into the SAME resident tables (the launch graph recorded for
    `values` stays valid)."""
    tm = HgTimings()
    _check(lib().hg_witness_gen_into(ctx.h, pk.h, witness.h, values.h, C.byref(tm)))
    values.timings = {f: getattr(tm, f) for f, _ in HgTimings._fields_}
    return values


def witness_derive_into(ctx, pk, d, values):
    """hg_witness_derive_into: derives the witness of d['s'], d['e'], d['k1'], d['ais'] straight into the resident tables of `values`
    and evaluates the circuit behind it; returns the host handle (Witness). values.timings holds total_ms and gpu_ms."""
    h = C.c_void_p()
    tm = HgTimings()
    arrs = Witness._derive_inputs(pk.params, d)
    L = lib()
    L.hg_witness_derive_into.argtypes = [C.c_void_p, C.c_void_p] + [u64p] * 4 + [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(HgTimings)]
    _check(L.hg_witness_derive_into(ctx.h if ctx is not None else None, pk.h, *[_ptr(a) for a in arrs], values.h, C.byref(h), C.byref(tm)))
    values.timings = {f: getattr(tm, f) for f, _ in HgTimings._fields_}
    return Witness(h, pk.params)


def _encryption_arrays(params, s, e, k1, a):
    n, k = params.n, params.k
    arrs = [np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in (s, e, k1, a)]
    if [x.size for x in arrs] != [n, n, n, k * n]:
        raise ValueError("encryption: s, e, k1 hold n signed coefficients (ascending degree) and a holds k * n")
    return arrs


def encryption_layout(params, s, e, k1, a):
    """hg_encryption_layout: the laid-out tables {'s', 'e', 'k1', 'ais'} (what Witness.derive takes) of the signed polynomials
    s, e, k1 (n coefficients, ascending degree) and a (k x n, one row per modulus). Host only."""
    arrs = _encryption_arrays(params, s, e, k1, a)
    sz = 2 * params.n
    out = [np.zeros(sz, dtype=np.uint64) for _ in range(3)] + [np.zeros(params.k * sz, dtype=np.uint64)]
    L = lib()
    L.hg_encryption_layout.argtypes = [C.POINTER(HgParams)] + [i64p] * 4 + [u64p] * 4
    L.hg_encryption_layout.restype = C.c_int
    _check(L.hg_encryption_layout(C.byref(params), *[x.ctypes.data_as(i64p) for x in arrs], *[_ptr(x) for x in out]))
    return dict(zip(("s", "e", "k1", "ais"), out))


def prove_encryptions(ctx, pk, encs, cap_each=1 << 20, witnesses=True, reason_cap=256):
    """hg_prove_encryptions: encs = a run of (s, e, k1, a) signed polynomials (ascending degree; a: k x n). Derivation + evaluation
    of encryption i+1 run under the prove of encryption i. Returns (proofs, statuses, reasons, witnesses, timings): proofs[i] the
    bytes (None when refused), statuses[i] 0 proven / 1 refused, reasons[i] the refusal's text, witnesses[i] the Witness handle of a
    proven item (None when refused or witnesses=False)."""
    return _prove_encryptions(lib().hg_prove_encryptions, ctx, pk, encs, cap_each, witnesses, reason_cap)


def prove_encryptions_bn254(ctx, pk, encs, cap_each=1 << 24, witnesses=True, reason_cap=256):
    """hg_prove_encryptions_bn254: prove_encryptions over bn256::Fr (proofs of 32-byte big-endian elements, each the bytes
    Context.prove_bn254 gives for Witness.derive of the laid-out encryption). Same arguments, same 5-tuple."""
    return _prove_encryptions(lib().hg_prove_encryptions_bn254, ctx, pk, encs, cap_each, witnesses, reason_cap)


def prove_encryptions_committed(ctx, pk, encs, log2_row=0, cap_each=1 << 20, witnesses=False, reason_cap=256):
    """hg_prove_encryptions_committed: prove_encryptions with a device Commitment to the five secret inputs of every proven item
    (what Commitment.from_values gives for its tables), made inside the pipeline. Returns (proofs, statuses, reasons, commitments,
    roots, witnesses, timings): commitments[i] is None and roots[i] 32 zero bytes for a refused item; timings["upload_ms"] is the
    commits' device time."""
    return _prove_encryptions_committed("goldilocks", ctx, pk, encs, log2_row, cap_each, witnesses, reason_cap)


def prove_encryptions_committed_bn254(ctx, pk, encs, log2_row=0, cap_each=1 << 24, witnesses=False, reason_cap=256):
    """hg_prove_encryptions_committed_bn254: prove_encryptions_bn254 with a BN254 device Commitment to the five secret inputs of every
    proven item (what Commitment.secrets_bn254 gives for the item's witness), made inside the pipeline from the tables in HBM. The
    7-tuple of prove_encryptions_committed; the commitments have field "bn254"."""
    return _prove_encryptions_committed("bn254", ctx, pk, encs, log2_row, cap_each, witnesses, reason_cap)


def _prove_encryptions_committed(field, ctx, pk, encs, log2_row, cap_each, witnesses, reason_cap):
    fn = lib().hg_prove_encryptions_committed_bn254 if field == "bn254" else lib().hg_prove_encryptions_committed
    n = len(encs)
    arrs = [_encryption_arrays(pk.params, *enc) for enc in encs]
    cols = [(i64p * max(n, 1))(*[x[f].ctypes.data_as(i64p) for x in arrs]) for f in range(4)]
    buf = (C.c_uint8 * (cap_each * max(n, 1)))()
    lens = (C.c_size_t * max(n, 1))()
    status = (C.c_int * max(n, 1))()
    cms = (C.c_void_p * max(n, 1))()
    rts = (C.c_uint8 * (32 * max(n, 1)))()
    hs = (C.c_void_p * max(n, 1))() if witnesses else None
    reasons = C.create_string_buffer(max(n, 1) * reason_cap)
    tm = HgTimings()
    rc = fn(_h(ctx), pk.h, *cols, n, log2_row, buf, cap_each, lens, status, cms, rts, hs, reasons, reason_cap, C.byref(tm))
    if rc < 0:
        raise HgError(lib().hg_last_error().decode())
    raw, rr = memoryview(buf), reasons.raw
    proofs = [None if status[i] else bytes(raw[i * cap_each:i * cap_each + lens[i]]) for i in range(n)]
    why = [rr[i * reason_cap:(i + 1) * reason_cap].split(b"\0", 1)[0].decode() for i in range(n)]
    ws = [Witness(C.c_void_p(hs[i]), pk.params) if witnesses and hs[i] else None for i in range(n)]
    nvars = _secrets_nvars(pk.params)
    c = pcs_row_log2(nvars, log2_row)
    roots = [bytes(rts[32 * i:32 * i + 32]) for i in range(n)]
    commitments = [Commitment(C.c_void_p(cms[i]), roots[i], ctx, nvars, c, field) if cms[i] else None for i in range(n)]
    return proofs, [int(status[i]) for i in range(n)], why, commitments, roots, ws, {f: getattr(tm, f) for f, _ in HgTimings._fields_}


def _secrets_nvars(params):
    """the variables of the tables of hg_secrets_commit: s, e, k1, r1is[0..k-1], r2is"""
    lg = params.n.bit_length() - 1
    return [lg + 1] * (3 + params.k) + [lg + params.k.bit_length() - 1]


def _prove_encryptions(fn, ctx, pk, encs, cap_each, witnesses, reason_cap):
    n = len(encs)
    arrs = [_encryption_arrays(pk.params, *enc) for enc in encs]
    pp = C.POINTER(i64p)
    fn.argtypes = [C.c_void_p, C.c_void_p, pp, pp, pp, pp, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                   C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t, C.POINTER(HgTimings)]
    fn.restype = C.c_int
    cols = [(i64p * max(n, 1))(*[x[f].ctypes.data_as(i64p) for x in arrs]) for f in range(4)]
    buf = (C.c_uint8 * (cap_each * max(n, 1)))()
    lens = (C.c_size_t * max(n, 1))()
    status = (C.c_int * max(n, 1))()
    hs = (C.c_void_p * max(n, 1))() if witnesses else None
    reasons = C.create_string_buffer(max(n, 1) * reason_cap)
    tm = HgTimings()
    rc = fn(ctx.h if ctx is not None else None, pk.h, *cols, n, buf, cap_each, lens, status, hs, reasons, reason_cap, C.byref(tm))
    if rc < 0:
        raise HgError(lib().hg_last_error().decode())
    raw, rr = memoryview(buf), reasons.raw
    proofs = [None if status[i] else bytes(raw[i * cap_each:i * cap_each + lens[i]]) for i in range(n)]
    why = [rr[i * reason_cap:(i + 1) * reason_cap].split(b"\0", 1)[0].decode() for i in range(n)]
    ws = [Witness(C.c_void_p(hs[i]), pk.params) if witnesses and hs[i] else None for i in range(n)]
    return proofs, [int(status[i]) for i in range(n)], why, ws, {f: getattr(tm, f) for f, _ in HgTimings._fields_}


class ProofBuffer:
    """Reusable output buffer so the timed loop does no Python-side allocation."""

    def __init__(self, cap=1 << 22):
        self.cap = cap
        self.buf = (C.c_uint8 * cap)()
        self.len = C.c_size_t(0)
        self.tm = HgTimings()

    def bytes(self):
        return C.string_at(self.buf, self.len.value)

    def timings(self):
        return {f: getattr(self.tm, f) for f, _ in HgTimings._fields_}


def prove_resident(ctx, pk, values, out):
    _check(lib().hg_prove_resident(ctx.h, pk.h, values.h, out.buf, out.cap, C.byref(out.len), C.byref(out.tm)))
    return out


def prove_resident_mode(ctx, pk, values, out, mode):
    """hg_prove_resident_mode: the round-by-round prover of the f-4 protocol modes on resident node tables."""
    L = lib()
    L.hg_prove_resident_mode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
    _check(L.hg_prove_resident_mode(ctx.h, pk.h, values.h, mode, out.buf, out.cap, C.byref(out.len), C.byref(out.tm)))
    return out


REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t)


class Group:
    """hg_group: the ranks of a sharded round-by-round prove. Group.local(world): ranks are threads of this process. Group.external(fn,
    world): fn(words: numpy u64 view) adds the ranks' words lane-wise mod p IN PLACE (an all-gather + modular sum, say)."""

    def __init__(self, h, world, keep=None):
        self.h, self.world, self._keep = h, world, keep

    @classmethod
    def local(cls, world):
        L = lib()
        L.hg_group_local.restype = C.c_void_p
        L.hg_group_local.argtypes = [C.c_int]
        h = L.hg_group_local(world)
        if not h:
            raise HgError(lib().hg_last_error().decode())
        return cls(h, world)

    @classmethod
    def external(cls, fn, world):
        L = lib()

        def tramp(_user, words, n):
            try:
                fn(np.ctypeslib.as_array(words, shape=(n,)))
                return 0
            except Exception:   # the library turns a non-zero return into an error of the prove
                import traceback
                traceback.print_exc()
                return -1

        cb = REDUCE_FN(tramp)
        L.hg_group_external.restype = C.c_void_p
        L.hg_group_external.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        h = L.hg_group_external(C.cast(cb, C.c_void_p), None, world)
        if not h:
            raise HgError(lib().hg_last_error().decode())
        return cls(h, world, keep=cb)

    def __del__(self):
        try:
            if self.h:
                lib().hg_group_free.argtypes = [C.c_void_p]
                lib().hg_group_free(self.h)
                self.h = None
        except Exception:
            pass


def prove_resident_mode_sharded(ctx, pk, values, out, mode, rank, group):
    """hg_prove_resident_mode_sharded: this rank's run of the round-by-round prover, one all-reduce per sum-check round through `group`."""
    L = lib()
    L.hg_prove_resident_mode_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
    _check(L.hg_prove_resident_mode_sharded(ctx.h, pk.h, values.h, mode, rank, group.h, out.buf, out.cap, C.byref(out.len), C.byref(out.tm)))
    return out


def prove_shard_begin(ctx, pk, values, rank, world):
    """This rank's share of ONE proof; returns a numpy view (u64) of the partial result buffer, to be all-gathered
    across ranks and handed to prove_shard_combine before prove_shard_finish."""
    ptr = u64p()
    n = C.c_size_t(0)
    _check(lib().hg_prove_shard_begin(ctx.h, pk.h, values.h, rank, world, C.byref(ptr), C.byref(n)))
    return np.ctypeslib.as_array(ptr, shape=(n.value,))


def prove_shard_combine(ctx, gathered, world):
    """gathered: the ranks' partial buffers (world x n u64, rank-major); installs their lane-wise sum mod p."""
    gathered = np.ascontiguousarray(gathered, dtype=np.uint64).reshape(-1)
    _check(lib().hg_prove_shard_combine(ctx.h, _ptr(gathered), world, gathered.size // world))


def shard_combine_host(gathered):
    """hg_shard_combine_host: [world, n] canonical u64 lanes -> lane-wise sum mod p (host only, no device needed)."""
    a = np.ascontiguousarray(gathered, dtype=np.uint64)
    world, n = a.shape
    out = np.zeros(n, dtype=np.uint64)
    L = lib()
    L.hg_shard_combine_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    _check(L.hg_shard_combine_host(_ptr(a), world, n, _ptr(out)))
    return out


def prove_shard_finish(ctx, out):
    _check(lib().hg_prove_shard_finish(ctx.h, out.buf, out.cap, C.byref(out.len), C.byref(out.tm)))
    return out


def params_derive(n, k, qis, t=65537):
    """hg_params_derive: the constants emitter of scripts/circuit_sk.py:422-439 for ring degree n and moduli qis."""
    p = HgParams()
    arr = (C.c_uint64 * len(qis))(*qis)
    L = lib()
    L.hg_params_derive.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(HgParams)]
    _check(L.hg_params_derive(n, k, arr, t, C.byref(p)))
    return p


def grand_product(ctx, tables, chain_skip=0, cap=1 << 22):
    """hg_grand_product: prove_grand_product on base-field tables (numpy u64); -> (proof bytes, claims (nb x 2), point (nv x 2))."""
    nb, ln = len(tables), tables[0].size
    nv = ln.bit_length() - 1
    tabs = [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
    ptrs = (u64p * nb)(*[_ptr(t) for t in tabs])
    buf = (C.c_uint8 * cap)()
    n = C.c_size_t(0)
    claims = np.zeros(2 * nb, dtype=np.uint64)
    point = np.zeros(2 * nv, dtype=np.uint64)
    L = lib()
    L.hg_grand_product.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), u64p, u64p]
    _check(L.hg_grand_product(ctx.h, nb, ln, ptrs, chain_skip, buf, cap, C.byref(n), _ptr(claims), _ptr(point)))
    return C.string_at(buf, n.value), claims.reshape(nb, 2), point.reshape(nv, 2)


def fold(ctx, table, is_base, r):
    """hg_fold: fix_var on the lowest variable; table: numpy u64 (2^nv base values or 2^nv (c0, c1) pairs flattened)."""
    t = np.ascontiguousarray(table, dtype=np.uint64)
    n_el = t.size if is_base else t.size // 2
    nv = n_el.bit_length() - 1
    out = np.zeros(n_el, dtype=np.uint64)  # 2^(nv-1) pairs
    rr = (C.c_uint64 * 2)(int(r[0]), int(r[1]))
    L = lib()
    L.hg_fold.argtypes = [C.c_void_p, u64p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64), u64p]
    _check(L.hg_fold(ctx.h, _ptr(t), nv, 1 if is_base else 0, rr, _ptr(out)))
    return out.reshape(-1, 2)


def device_count():
    """hg_device_count: HIP devices visible to this process (0 without a GPU)."""
    return int(lib().hg_device_count())


def comm_unique_id():
    """hg_comm_unique_id: the 128-byte RCCL id rank 0 shares with the other ranks."""
    buf = (C.c_uint8 * 128)()
    _check(lib().hg_comm_unique_id(buf))
    return bytes(buf)


def comm_init(ctx, uid, rank, world):
    """hg_comm_init (collective): RCCL communicator of this rank's context."""
    buf = (C.c_uint8 * 128).from_buffer_copy(uid)
    L = lib()
    L.hg_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    _check(L.hg_comm_init(ctx.h, buf, rank, world))


def comm_count(ctx):
    """hg_comm_count: ranks of the context's RCCL communicator (ncclCommCount)."""
    L = lib()
    n = C.c_int(0)
    L.hg_comm_count.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    _check(L.hg_comm_count(ctx.h, C.byref(n)))
    return n.value


def comm_selftest(ctx, rank_buffers):
    """hg_comm_selftest: rank_buffers [world, n] u64 canonical lanes -> lane-wise sum mod p through the split / combine kernels."""
    a = np.ascontiguousarray(rank_buffers, dtype=np.uint64)
    world, n = a.shape
    out = np.zeros(n, dtype=np.uint64)
    L = lib()
    L.hg_comm_selftest.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    _check(L.hg_comm_selftest(ctx.h, _ptr(a), world, n, _ptr(out)))
    return out


def comm_destroy(ctx):
    L = lib()
    L.hg_comm_destroy.argtypes = [C.c_void_p]
    _check(L.hg_comm_destroy(ctx.h))


def prove_sharded(ctx, pk, values, out):
    """hg_prove_sharded (collective): this rank's share of ONE proof + the RCCL all-reduce inside the library + replay."""
    L = lib()
    L.hg_prove_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HgTimings)]
    _check(L.hg_prove_sharded(ctx.h, pk.h, values.h, out.buf, out.cap, C.byref(out.len), C.byref(out.tm)))
    return out


def challenges_bn254(n):
    """First n Fiat-Shamir challenges over bn256::Fr (host)."""
    out = np.zeros(n * 4, dtype=np.uint64)
    _check(lib().hg_challenges_bn254(n, _ptr(out)))
    return Context._fr_unpack(out)


def _decision(rc):
    """the tail of every verifier call: (accepted, reason); a negative status is an HgError"""
    if rc < 0:
        raise HgError(lib().hg_last_error().decode())
    return rc == 0, ("" if rc == 0 else lib().hg_last_error().decode())


def _h(ctx):
    return ctx.h if ctx is not None else None


def verify(pk, witness, proof, mode=0):
    """BfvEncrypt::verify [REF sk_encryption_circuit.rs:462-517]: (accepted, reason). mode: see hg_verify_mode."""
    L = lib()
    return _decision(L.hg_verify_mode(pk.h, witness.h, mode, proof, len(proof)) if mode else L.hg_verify(pk.h, witness.h, proof, len(proof)))


def verify_bn254(pk, witness, proof):
    """BfvEncrypt::verify over bn256::Fr [REF sk_encryption_circuit.rs:462-517, 614-626]: (accepted, reason)."""
    return _decision(lib().hg_verify_bn254(pk.h, witness.h, proof, len(proof)))


def verify_device(ctx, pk, witness, proof, mode=0):
    """hg_verify_device: BfvEncrypt::verify with the table-sized work on the device: (accepted, reason). mode != 0:
    hg_verify_device_mode (the mode bits of hg_verify_mode)."""
    L = lib()
    if mode:
        return _decision(L.hg_verify_device_mode(_h(ctx), pk.h, witness.h, mode, proof, len(proof)))
    return _decision(L.hg_verify_device(ctx.h, pk.h, witness.h, proof, len(proof)))


def verify_device_bn254(ctx, pk, witness, proof):
    """hg_verify_device_bn254: BfvEncrypt::verify over bn256::Fr with the table-sized work on the device: (accepted, reason)."""
    return _decision(lib().hg_verify_device_bn254(_h(ctx), pk.h, witness.h, proof, len(proof)))


def _verify_batch(fn, ctx, pk, handles, proofs, extra_args, reason_cap, outputs=()):
    """One call of a batch entry: fn(ctx, pk, handles, proofs, lens, n, *extra_args, results, *outputs, reasons, reason_cap).
    Returns [(accepted, reason)], one per proof."""
    n = len(proofs)
    m = max(n, 1)
    hs = (C.c_void_p * m)(*[x.h.value for x in handles])
    ps = (C.c_char_p * m)(*[bytes(p) for p in proofs])
    lens = (C.c_size_t * m)(*[len(p) for p in proofs])
    res = (C.c_int * m)()
    reasons = C.create_string_buffer(m * reason_cap)
    if fn(_h(ctx), pk.h, hs, ps, lens, n, *extra_args, res, *outputs, reasons, reason_cap) < 0:
        raise HgError(lib().hg_last_error().decode())
    raw = reasons.raw
    return [(res[i] == 0, raw[i * reason_cap:(i + 1) * reason_cap].split(b"\0", 1)[0].decode()) for i in range(n)]


def verify_device_batch(ctx, pk, witnesses, proofs, mode=0, reason_cap=256):
    """hg_verify_device_batch: proof i against witnesses[i] in `mode`, the run verified in device passes of a group of proofs each:
    a list of (accepted, reason), one per proof, the decisions of verify_device(ctx, pk, witnesses[i], proofs[i], mode)."""
    if len(witnesses) != len(proofs):
        raise ValueError("verify_device_batch: one witness per proof")
    return _verify_batch(lib().hg_verify_device_batch, ctx, pk, witnesses, proofs, (mode,), reason_cap)


def verify_device_batch_bn254(ctx, pk, witnesses, proofs, reason_cap=256):
    """hg_verify_device_batch_bn254: BN254 proof i against witnesses[i], the run verified in device passes of a group of proofs each:
    a list of (accepted, reason), one per proof, the decisions of verify_device_bn254(ctx, pk, witnesses[i], proofs[i])."""
    if len(witnesses) != len(proofs):
        raise ValueError("verify_device_batch_bn254: one witness per proof")
    return _verify_batch(lib().hg_verify_device_batch_bn254, ctx, pk, witnesses, proofs, (), reason_cap)


class InputClaims:
    """What verify_public leaves open: `claims` (a ctypes array of HgInputClaim) and `points` (u64, two words per coordinate)."""
    WORDS, STRUCT, SFX = 2, HgInputClaim, ""     # how an element crosses the ABI; the entries of this field are hg_<name> + SFX

    def __init__(self, claims, n, points):
        self.claims, self.n, self.points = claims, n, points

    def as_tuples(self):
        """[(input, nvars, point words, value words)]: the whole content, for comparisons."""
        W = self.WORDS
        return [(int(c.input), int(c.nvars), tuple(int(x) for x in self.points[W * c.point_off:W * (c.point_off + c.nvars)]), tuple(int(x) for x in c.value))
                for c in self.claims[:self.n]]


class InputClaimsBn254(InputClaims):
    """What verify_public_bn254 leaves open: `claims` (a ctypes array of HgInputClaimBn254) and `points` (u64, four limbs per coordinate)."""
    WORDS, STRUCT, SFX = 4, HgInputClaimBn254, "_bn254"


def _pack(F, elems):
    """elements of field F as ABI words: u64 words as they are (Goldilocks), Python ints below r as 4 limbs each (BN254)"""
    return Context._fr_pack(elems) if F is InputClaimsBn254 else np.ascontiguousarray(elems, dtype=np.uint64).reshape(-1)


class Instance:
    """hg_instance: the public instance of one encryption - a_i and ct0_i as signed coefficients (k x n, ascending degree)."""

    def __init__(self, handle, params):
        self.h = handle
        self.params = params

    @classmethod
    def from_ciphertext(cls, params, a, ct0):
        """hg_instance_from_ciphertext: every coefficient in [-(q_i-1)/2, (q_i-1)/2], else HgError naming table, modulus, index."""
        kn = params.k * params.n
        arrs = [np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in (a, ct0)]
        if [x.size for x in arrs] != [kn, kn]:
            raise ValueError("instance: a and ct0 hold k * n signed coefficients each")
        h = C.c_void_p()
        _check(lib().hg_instance_from_ciphertext(C.byref(params), arrs[0].ctypes.data_as(i64p), arrs[1].ctypes.data_as(i64p), C.byref(h)))
        return cls(h, params)

    @classmethod
    def from_witness(cls, witness):
        """hg_instance_from_witness: the layout of the handle's ais and ct0is tables inverted."""
        h = C.c_void_p()
        _check(lib().hg_instance_from_witness(C.byref(witness.params), witness.h, C.byref(h)))
        return cls(h, witness.params)

    def coeffs(self):
        """hg_instance_coeffs: (a, ct0) as int64 arrays of k * n coefficients."""
        kn = self.params.k * self.params.n
        a, ct0 = np.zeros(kn, dtype=np.int64), np.zeros(kn, dtype=np.int64)
        _check(lib().hg_instance_coeffs(self.h, a.ctypes.data_as(i64p), ct0.ctypes.data_as(i64p)))
        return a, ct0

    def table(self, which):
        """hg_instance_get: the laid-out ais (which 0) or ct0is (which 1) table, as Witness.arrays() holds it."""
        L = lib()
        n = _check(L.hg_instance_get(self.h, which, None, 0))
        out = np.zeros(n, dtype=np.uint64)
        _check(L.hg_instance_get(self.h, which, _ptr(out), n))
        return out

    def _mle(self, F, ctx, which, index, point):
        pt = _pack(F, point)
        out = np.zeros(F.WORDS, dtype=np.uint64)
        _check(getattr(lib(), "hg_instance_mle" + F.SFX)(_h(ctx), self.h, which, index, _ptr(pt), pt.size // F.WORDS, _ptr(out)))
        return out

    def mle(self, ctx, which, index, point):
        """hg_instance_mle: the MLE of ais[index] (which 0) or ct0is (which 1) at an E point (u64 pairs); ctx None: host loop."""
        return self._mle(InputClaims, ctx, which, index, point)

    def mle_bn254(self, ctx, which, index, point):
        """hg_instance_mle_bn254: the MLE of ais[index] (which 0) or ct0is (which 1) at an Fr point (Python ints below r) as a
        Python int; ctx None: host loop, else the compact dot kernel over Fr."""
        return Context._fr_unpack(self._mle(InputClaimsBn254, ctx, which, index, point))[0]

    def __del__(self):
        try:
            if self.h:
                lib().hg_instance_free(self.h)
                self.h = None
        except Exception:
            pass


def pk_claim_shape(pk):
    """hg_pk_claim_shape: (claims on secret inputs a proof of this key leaves, their coordinates in all)."""
    a, b = C.c_size_t(0), C.c_size_t(0)
    _check(lib().hg_pk_claim_shape(pk.h, C.byref(a), C.byref(b)))
    return a.value, b.value


def _verify_public(F, pk, instance, proof, mode_args, ctx, device):
    nc, nco = pk_claim_shape(pk)
    claims = (F.STRUCT * max(nc, 1))()
    points = np.zeros(F.WORDS * max(nco, 1), dtype=np.uint64)
    n = C.c_size_t(0)
    args = (pk.h, instance.h, *mode_args, proof, len(proof), claims, nc, _ptr(points), nco, C.byref(n))
    L = lib()
    ok, why = _decision(getattr(L, "hg_verify_public_device" + F.SFX)(_h(ctx), *args) if device else getattr(L, "hg_verify_public" + F.SFX)(*args))
    return ok, why, (F(claims, n.value, points) if ok else None)


def verify_public(pk, instance, proof, mode=0, ctx=None, device=False):
    """hg_verify_public (device=True: hg_verify_public_device on ctx): the part of BfvEncrypt::verify that the key, the proof, a_i
    and ct0_i decide. Returns (accepted, reason, InputClaims or None): the claims left on the secret inputs, for claims_settle."""
    return _verify_public(InputClaims, pk, instance, proof, (mode,), ctx, device)


def verify_public_bound(pk, instance, proof, root, mode=3, ctx=None, device=False):
    """hg_verify_public_bound (device=True: hg_verify_public_bound_device on ctx): verify_public for a proof of prove_committed_mode,
    whose transcript starts from the key's parameters, the digest of `instance` and `root`, the 32-byte root of the commitment to the
    secret inputs. Returns (accepted, reason, InputClaims or None); HgError for mode 0 or 2."""
    nc, nco = pk_claim_shape(pk)
    claims = (HgInputClaim * max(nc, 1))()
    points = np.zeros(2 * max(nco, 1), dtype=np.uint64)
    n = C.c_size_t(0)
    args = (pk.h, instance.h, mode, root, proof, len(proof), claims, nc, _ptr(points), nco, C.byref(n))
    L = lib()
    ok, why = _decision(L.hg_verify_public_bound_device(_h(ctx), *args) if device else L.hg_verify_public_bound(*args))
    return ok, why, (InputClaims(claims, n.value, points) if ok else None)


def instance_digest(instance, ctx=None):
    """hg_instance_digest: the 32-byte statement digest of an Instance (the Keccak tree of include/hg.h over its 2kn signed words);
    ctx None: the host tree, else the digest kernel."""
    out = (C.c_uint8 * 32)()
    _check(lib().hg_instance_digest(_h(ctx), instance.h, out))
    return bytes(out)


def instance_digest_batch(ctx, instances):
    """hg_instance_digest_batch: the digests of a run of Instances of one parameter set, one launch over all of them."""
    n = len(instances)
    hs = (C.c_void_p * max(n, 1))(*[i.h for i in instances])
    out = (C.c_uint8 * (32 * max(n, 1)))()
    _check(lib().hg_instance_digest_batch(_h(ctx), hs, n, out))
    return [bytes(out[32 * i:32 * (i + 1)]) for i in range(n)]


def instance_digest_group(ctx, instances):
    """hg_instance_digest_group: the digests of a run of Instances of one parameter set as verify_public_bound_batch computes them:
    staged in slices (context option "bound_batch_slice") and hashed out of the staged set."""
    n = len(instances)
    hs = (C.c_void_p * max(n, 1))(*[i.h for i in instances])
    out = (C.c_uint8 * (32 * max(n, 1)))()
    _check(lib().hg_instance_digest_group(_h(ctx), hs, n, out))
    return [bytes(out[32 * i:32 * (i + 1)]) for i in range(n)]


def verify_public_bound_batch(ctx, pk, instances, roots, proofs, mode=3, reason_cap=256):
    """hg_verify_public_bound_batch: bound proof i against instances[i] and the 32-byte roots[i] in `mode` (1 or 3), the run verified
    in device passes of a group of proofs each. Returns (results, digests): results as verify_public_batch returns them - what
    verify_public_bound(pk, instances[i], proofs[i], roots[i], mode, ctx, device=True) returns for that pair alone -, digests the
    statement digest of every instance as the device computed it, rejected items included."""
    if not len(instances) == len(roots) == len(proofs):
        raise ValueError("verify_public_bound_batch: one instance and one root per proof")
    nc, nco = pk_claim_shape(pk)
    n = len(proofs)
    m, nc1, nco1 = max(n, 1), max(nc, 1), max(nco, 1)
    hs = (C.c_void_p * m)(*[x.h.value for x in instances])
    rs = (C.c_char_p * m)(*[bytes(r) for r in roots])
    ps = (C.c_char_p * m)(*[bytes(p) for p in proofs])
    lens = (C.c_size_t * m)(*[len(p) for p in proofs])
    res = (C.c_int * m)()
    claims = (HgInputClaim * (m * nc1))()
    points = np.zeros(2 * m * nco1, dtype=np.uint64)
    counts = (C.c_size_t * m)()
    dg = (C.c_uint8 * (32 * m))()
    reasons = C.create_string_buffer(m * reason_cap)
    if lib().hg_verify_public_bound_batch(_h(ctx), pk.h, hs, rs, ps, lens, n, mode, res, claims, nc1, _ptr(points), nco1, counts, dg, reasons, reason_cap) < 0:
        raise HgError(lib().hg_last_error().decode())
    raw = reasons.raw
    out = []
    for i in range(n):
        ok = res[i] == 0
        cl = InputClaims((HgInputClaim * nc1)(*claims[i * nc1:(i + 1) * nc1]), counts[i], points[2 * i * nco1:2 * (i + 1) * nco1].copy()) if ok else None
        out.append((ok, raw[i * reason_cap:(i + 1) * reason_cap].split(b"\0", 1)[0].decode(), cl))
    return out, [bytes(dg[32 * i:32 * (i + 1)]) for i in range(n)]


def values_instance_digest(ctx, pk, values):
    """hg_values_instance_digest: the same digest read from the resident ais and ct0is tables of a ResidentValues of this key."""
    out = (C.c_uint8 * 32)()
    _check(lib().hg_values_instance_digest(_h(ctx), pk.h, values.h if values is not None else None, out))
    return bytes(out)


def bound_seed(params, mode, digest, root):
    """hg_bound_seed: the bytes a bound transcript starts from."""
    out, n = (C.c_uint8 * 256)(), C.c_size_t(0)
    _check(lib().hg_bound_seed(C.byref(params), mode, digest, root, out, 256, C.byref(n)))
    return bytes(out[:n.value])


def prove_committed_mode(ctx, pk, values, out, mode=3, log2_row=0):
    """hg_prove_committed_mode: commits to the secret inputs of a ResidentValues (the Commitment of Commitment.from_values), digests
    its public tables and proves in `mode` (1 or 3) on the transcript seeded with both. Returns (out, Commitment)."""
    h, root = C.c_void_p(), (C.c_uint8 * 32)()
    _check(lib().hg_prove_committed_mode(_h(ctx), pk.h, values.h if values is not None else None, mode, log2_row, out.buf, out.cap, C.byref(out.len), C.byref(h), root,
                                         C.byref(out.tm)))
    nvars = _secrets_nvars(pk.params)
    return out, Commitment(h, bytes(root), ctx, nvars, pcs_row_log2(nvars, log2_row))


def verify_public_bn254(pk, instance, proof, ctx=None, device=False):
    """hg_verify_public_bn254 (device=True: hg_verify_public_device_bn254 on ctx): the part of BfvEncrypt::verify over bn256::Fr that
    the key, the proof, a_i and ct0_i decide. Returns (accepted, reason, InputClaimsBn254 or None), for claims_settle_bn254."""
    return _verify_public(InputClaimsBn254, pk, instance, proof, (), ctx, device)


def _verify_public_batch(F, ctx, pk, instances, proofs, mode_args, reason_cap):
    name = "verify_public_batch" + F.SFX
    if len(instances) != len(proofs):
        raise ValueError(name + ": one instance per proof")
    nc, nco = pk_claim_shape(pk)
    m, nc1, nco1 = max(len(proofs), 1), max(nc, 1), max(nco, 1)
    claims = (F.STRUCT * (m * nc1))()
    points = np.zeros(F.WORDS * m * nco1, dtype=np.uint64)
    counts = (C.c_size_t * m)()
    got = _verify_batch(getattr(lib(), "hg_" + name), ctx, pk, instances, proofs, mode_args, reason_cap, (claims, nc1, _ptr(points), nco1, counts))
    return [(ok, why, F((F.STRUCT * nc1)(*claims[i * nc1:(i + 1) * nc1]), counts[i], points[F.WORDS * i * nco1:F.WORDS * (i + 1) * nco1].copy()) if ok else None)
            for i, (ok, why) in enumerate(got)]


def verify_public_batch(ctx, pk, instances, proofs, mode=0, reason_cap=256):
    """hg_verify_public_batch: proof i against instances[i] in `mode`, the run verified in device passes of a group of proofs each:
    a list of (accepted, reason, InputClaims or None), one per proof: what verify_public(pk, instances[i], proofs[i], mode, ctx,
    device=True) returns for that pair alone."""
    return _verify_public_batch(InputClaims, ctx, pk, instances, proofs, (mode,), reason_cap)


def verify_public_batch_bn254(ctx, pk, instances, proofs, reason_cap=256):
    """hg_verify_public_batch_bn254: BN254 proof i against instances[i], the run verified in device passes of a group of proofs each:
    a list of (accepted, reason, InputClaimsBn254 or None), one per proof: what verify_public_bn254(pk, instances[i], proofs[i], ctx,
    device=True) returns for that pair alone."""
    return _verify_public_batch(InputClaimsBn254, ctx, pk, instances, proofs, (), reason_cap)


def _instance_mle_batch(F, ctx, instances, which, index, point):
    pt = _pack(F, point)
    n = len(instances)
    out = np.zeros(F.WORDS * max(n, 1), dtype=np.uint64)
    hs = (C.c_void_p * max(n, 1))(*[x.h.value for x in instances])
    _check(getattr(lib(), "hg_instance_mle_batch" + F.SFX)(_h(ctx), hs, n, which, index, _ptr(pt), pt.size // F.WORDS, _ptr(out)))
    return out[:F.WORDS * n]


def instance_mle_batch(ctx, instances, which, index, point):
    """hg_instance_mle_batch: the MLE of ais[index] (which 0) or ct0is (which 1) of every instance at ONE E point (u64 pairs),
    through the kernel of hg_verify_public_batch as one work unit: an (n, 2) array. Device only."""
    return _instance_mle_batch(InputClaims, ctx, instances, which, index, point).reshape(len(instances), 2)


def instance_mle_batch_bn254(ctx, instances, which, index, point):
    """hg_instance_mle_batch_bn254: the MLE of ais[index] (which 0) or ct0is (which 1) of every instance at ONE Fr point (Python ints
    below r), through the kernel of hg_verify_public_batch_bn254 as one work unit: a list of Python ints. Device only."""
    return Context._fr_unpack(_instance_mle_batch(InputClaimsBn254, ctx, instances, which, index, point))


def _claims_settle(fn, ctx, params, witness, claims):
    return _decision(fn(_h(ctx), C.byref(params), witness.h, claims.claims, claims.n, _ptr(claims.points)))


def claims_settle(ctx, params, witness, claims):
    """hg_claims_settle: every claim of an InputClaims against the witness handle (ctx None: host): (accepted, reason)."""
    return _claims_settle(lib().hg_claims_settle, ctx, params, witness, claims)


def claims_settle_bn254(ctx, params, witness, claims):
    """hg_claims_settle_bn254: every claim of an InputClaimsBn254 against the witness handle (ctx None: host): (accepted, reason)."""
    return _claims_settle(lib().hg_claims_settle_bn254, ctx, params, witness, claims)


PCS_DEFAULT_QUERIES = 241


def pcs_row_log2(nvars, log2_row=0):
    """The row length an hg_pcs_* call uses: log2_row, or for 0 min(min v_t, ceil(log2(sum 2^v_t) / 2))."""
    if log2_row:
        return log2_row
    total, c = sum(1 << v for v in nvars), 0
    while (1 << (2 * c)) < total:
        c += 1
    return min(c, min(nvars))


def _opening_bytes(elem_bytes, word_bytes, nvars, n_claims, n_queries, log2_row):
    c = pcs_row_log2(nvars, log2_row)
    rows = sum(1 << (v - c) for v in nvars)
    return elem_bytes * (1 << c) * (n_claims + 1) + (n_queries or PCS_DEFAULT_QUERIES) * (word_bytes * rows + 32 * (c + 2))


def pcs_opening_bytes(nvars, n_claims, n_queries=0, log2_row=0):
    """16 C (n+1) + Q (8 R + 32 (c+2)): the exact length of an opening."""
    return _opening_bytes(16, 8, nvars, n_claims, n_queries, log2_row)


def pcs_opening_bytes_bn254(nvars, n_claims, n_queries=0, log2_row=0):
    """32 C (n+1) + Q (32 R + 32 (c+2)): the exact length of an opening over BN254."""
    return _opening_bytes(32, 32, nvars, n_claims, n_queries, log2_row)


def pcs_folded_opening_bytes(nvars, n_queries=0, log2_row=0):
    """16 (3 V + m) + 32 C + Q (8 R + 32 (c+2)): the exact length of a folded opening, whatever the number of claims."""
    return 16 * (3 * max(nvars) + len(nvars)) + pcs_opening_bytes(nvars, 1, n_queries, log2_row)


def pcs_folded_opening_bytes_bn254(nvars, n_queries=0, log2_row=0):
    """32 (3 V + m) + 64 C + Q (32 R + 32 (c+2)): the exact length of a folded opening over BN254, whatever the number of claims."""
    return 32 * (3 * max(nvars) + len(nvars)) + pcs_opening_bytes_bn254(nvars, 1, n_queries, log2_row)


def _pcs_protos():
    """the library: the prototypes of the commitment entries are assigned with the others when it is loaded"""
    return lib()


def _pcs_claim_arrays(claims):
    """claims: [(table, point words (2 per coordinate), (v0, v1))] -> ctypes / numpy arguments"""
    n = len(claims)
    table = (C.c_uint32 * max(n, 1))(*[int(c[0]) for c in claims])
    pts = np.array([int(x) for c in claims for x in c[1]] or [0], dtype=np.uint64)
    vals = np.array([int(x) for c in claims for x in c[2]] or [0], dtype=np.uint64)
    return table, pts, vals


def _pcs_claim_arrays_bn254(claims):
    """claims: [(table, point (Python ints below r), value)] -> ctypes / numpy arguments, 4 limbs per element"""
    n = len(claims)
    table = (C.c_uint32 * max(n, 1))(*[int(c[0]) for c in claims])
    pts = Context._fr_pack([x for c in claims for x in c[1]] or [0])
    vals = Context._fr_pack([c[2] for c in claims] or [0])
    return table, pts, vals


def _fr_table(t):
    """a table of Fr elements as 4 little-endian u64 limbs each: a u64 array of limbs as it is, anything else as Python ints"""
    if isinstance(t, np.ndarray) and t.dtype == np.uint64:
        return np.ascontiguousarray(t).reshape(-1)
    return Context._fr_pack(t)


class Commitment:
    """hg_pcs_commit / hg_secrets_commit and their _bn254 forms: the handle of a polynomial commitment (host form: ctx None) and its
    32-byte root. field is "goldilocks" or "bn254"; open and open_claims call the entry of the handle's field."""

    def __init__(self, handle, root, ctx, nvars, log2_row, field="goldilocks"):
        self.h, self.root, self.ctx, self.nvars, self.log2_row, self.field = handle, root, ctx, list(nvars), log2_row, field

    @classmethod
    def _commit(cls, field, ctx, tabs, words, log2_row):
        nvars = [(t.size // words).bit_length() - 1 for t in tabs]
        ptrs = (u64p * len(tabs))(*[_ptr(t) for t in tabs])
        nv = (C.c_uint32 * len(tabs))(*nvars)
        h, root = C.c_void_p(), (C.c_uint8 * 32)()
        fn = lib().hg_pcs_commit_bn254 if field == "bn254" else lib().hg_pcs_commit
        _check(fn(_h(ctx), ptrs, nv, len(tabs), log2_row, C.byref(h), root))
        return cls(h, bytes(root), ctx, nvars, pcs_row_log2(nvars, log2_row), field)

    @classmethod
    def _secrets(cls, field, ctx, params, witness, log2_row):
        h, root = C.c_void_p(), (C.c_uint8 * 32)()
        fn = lib().hg_secrets_commit_bn254 if field == "bn254" else lib().hg_secrets_commit
        _check(fn(_h(ctx), C.byref(params), witness.h, log2_row, C.byref(h), root))
        lg = params.n.bit_length() - 1
        nvars = [lg + 1] * (3 + params.k) + [lg + params.k.bit_length() - 1]
        return cls(h, bytes(root), ctx, nvars, pcs_row_log2(nvars, log2_row), field)

    @classmethod
    def commit_bn254(cls, ctx, tables, log2_row=0):
        """hg_pcs_commit_bn254. tables: per table 2^v_t elements, Python ints below r or a numpy u64 array of 4 limbs each."""
        return cls._commit("bn254", ctx, [_fr_table(t) for t in tables], 4, log2_row)

    @classmethod
    def secrets_bn254(cls, ctx, params, witness, log2_row=0):
        """hg_secrets_commit_bn254: the five secret inputs of a witness handle, every word lifted into Fr by the signed rule."""
        return cls._secrets("bn254", ctx, params, witness, log2_row)

    @classmethod
    def commit(cls, ctx, tables, log2_row=0):
        """tables: numpy u64 arrays of 2^v_t canonical words."""
        return cls._commit("goldilocks", ctx, [np.ascontiguousarray(t, dtype=np.uint64) for t in tables], 1, log2_row)

    @classmethod
    def secrets(cls, ctx, params, witness, log2_row=0):
        """hg_secrets_commit: the five secret inputs of a witness handle (tables s, e, k1, r1is[0..k-1], r2is)."""
        return cls._secrets("goldilocks", ctx, params, witness, log2_row)

    @classmethod
    def from_values(cls, ctx, pk, values, log2_row=0):
        """hg_secrets_commit_values: the device Commitment of secrets(ctx, ..) to the five secret inputs where witness_gen left them
        in HBM (a ResidentValues of this key and context that holds every table)."""
        h, root = C.c_void_p(), (C.c_uint8 * 32)()
        _check(lib().hg_secrets_commit_values(_h(ctx), pk.h, values.h if values is not None else None, log2_row, C.byref(h), root))
        nvars = _secrets_nvars(pk.params)
        return cls(h, bytes(root), ctx, nvars, pcs_row_log2(nvars, log2_row))

    @classmethod
    def _batch(cls, call, ctx, n, nvars, log2_row, field="goldilocks"):
        """call(handles, roots) of a commit batch entry of `field` -> the n Commitments"""
        hs, roots = (C.c_void_p * max(n, 1))(), (C.c_uint8 * (32 * max(n, 1)))()
        _check(call(hs, roots))
        c = pcs_row_log2(nvars, log2_row)
        return [cls(C.c_void_p(hs[i]), bytes(roots[32 * i:32 * i + 32]), ctx, nvars, c, field) for i in range(n)]

    @classmethod
    def _commit_batch(cls, field, ctx, tabs, words, log2_row):
        n = len(tabs)
        if not n:   # (no member, no shape to pass)
            return []
        nvars = [(t.size // words).bit_length() - 1 for t in tabs[0]]
        if any([(t.size // words).bit_length() - 1 for t in tables] != nvars for tables in tabs):
            raise ValueError("commit_batch: every member has the tables of one shape")
        rows = [(u64p * len(nvars))(*[_ptr(t) for t in tables]) for tables in tabs]
        ptrs = (C.POINTER(u64p) * max(n, 1))(*[C.cast(r, C.POINTER(u64p)) for r in rows])
        nv = (C.c_uint32 * len(nvars))(*nvars)
        fn = lib().hg_pcs_commit_batch_bn254 if field == "bn254" else lib().hg_pcs_commit_batch
        return cls._batch(lambda hs, roots: fn(_h(ctx), ptrs, nv, len(nvars), log2_row, n, hs, roots), ctx, n, nvars, log2_row, field)

    @classmethod
    def _secrets_batch(cls, field, ctx, params, witnesses, log2_row):
        n = len(witnesses)
        ws = (C.c_void_p * max(n, 1))(*[w.h for w in witnesses])
        lg = params.n.bit_length() - 1
        nvars = [lg + 1] * (3 + params.k) + [lg + params.k.bit_length() - 1]
        fn = lib().hg_secrets_commit_batch_bn254 if field == "bn254" else lib().hg_secrets_commit_batch
        return cls._batch(lambda hs, roots: fn(_h(ctx), C.byref(params), ws, n, log2_row, hs, roots), ctx, n, nvars, log2_row, field)

    @classmethod
    def commit_batch(cls, ctx, tables_list, log2_row=0):
        """hg_pcs_commit_batch: one device Commitment per entry of tables_list (each as commit takes it), all of one shape, their
        matrices encoded and hashed in device passes of a group of members each."""
        return cls._commit_batch("goldilocks", ctx, [[np.ascontiguousarray(t, dtype=np.uint64) for t in tables] for tables in tables_list], 1, log2_row)

    @classmethod
    def secrets_batch(cls, ctx, params, witnesses, log2_row=0):
        """hg_secrets_commit_batch: one device Commitment to the five secret inputs of every witness handle."""
        return cls._secrets_batch("goldilocks", ctx, params, witnesses, log2_row)

    @classmethod
    def commit_batch_bn254(cls, ctx, tables_list, log2_row=0):
        """hg_pcs_commit_batch_bn254: commit_batch over bn256::Fr, each member's tables as commit_bn254 takes them; the handles are
        BN254 handles."""
        return cls._commit_batch("bn254", ctx, [[_fr_table(t) for t in tables] for tables in tables_list], 4, log2_row)

    @classmethod
    def secrets_batch_bn254(cls, ctx, params, witnesses, log2_row=0):
        """hg_secrets_commit_batch_bn254: one device BN254 Commitment to the five secret inputs of every witness handle, every word
        lifted into Fr by the signed rule."""
        return cls._secrets_batch("bn254", ctx, params, witnesses, log2_row)

    def _open(self, entry, head, n_claims, tail, n_queries, folded=False):
        """entry(ctx, *head, n_claims, *tail, n_queries, buffer, its size, length out) of the handle's field -> the opening bytes"""
        bn = self.field == "bn254"
        if folded:
            entry, cap = entry + "_folded", (pcs_folded_opening_bytes_bn254 if bn else pcs_folded_opening_bytes)(self.nvars, n_queries, self.log2_row)
        else:
            cap = (pcs_opening_bytes_bn254 if bn else pcs_opening_bytes)(self.nvars, n_claims, n_queries, self.log2_row)
        buf, ln = (C.c_uint8 * cap)(), C.c_size_t(0)
        _check(getattr(lib(), entry + ("_bn254" if bn else ""))(_h(self.ctx), *head, n_claims, *tail, n_queries, buf, cap, C.byref(ln)))
        return bytes(memoryview(buf)[:ln.value])

    def open(self, claims, n_queries=0):
        """hg_pcs_open: claims = [(table, point words, (v0, v1))] -> the opening bytes. On a BN254 handle hg_pcs_open_bn254:
        claims = [(table, point (Python ints below r), value)]."""
        table, pts, vals = (_pcs_claim_arrays_bn254 if self.field == "bn254" else _pcs_claim_arrays)(claims)
        return self._open("hg_pcs_open", (self.h, table, _ptr(pts), _ptr(vals)), len(claims), (), n_queries)

    def open_claims(self, params, claims, n_queries=0):
        """hg_claims_open: the opening of an InputClaims (what verify_public returns) against a Commitment.secrets handle. On a BN254
        handle hg_claims_open_bn254 of an InputClaimsBn254 (what verify_public_bn254 returns)."""
        return self._open("hg_claims_open", (C.byref(params), self.h, claims.claims), claims.n, (_ptr(claims.points),), n_queries)

    def open_folded(self, claims, n_queries=0):
        """hg_pcs_open_folded, on a BN254 handle hg_pcs_open_folded_bn254: open's claims (at least one) -> a folded opening, whose
        length does not grow with the claims."""
        table, pts, vals = (_pcs_claim_arrays_bn254 if self.field == "bn254" else _pcs_claim_arrays)(claims)
        return self._open("hg_pcs_open", (self.h, table, _ptr(pts), _ptr(vals)), len(claims), (), n_queries, folded=True)

    def open_claims_folded(self, params, claims, n_queries=0):
        """hg_claims_open_folded, on a BN254 handle hg_claims_open_folded_bn254: open_claims as a folded opening."""
        return self._open("hg_claims_open", (C.byref(params), self.h, claims.claims), claims.n, (_ptr(claims.points),), n_queries, folded=True)

    def free(self):
        if self.h:
            lib().hg_pcs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _open_batch(call, cms, counts, n_queries, reason_cap, opening_bytes=pcs_opening_bytes):
    """One call of an open batch entry: call(handles, counts, n_queries, n, openings, cap_each, lens, status, reasons, reason_cap) ->
    [(the opening bytes or None, reason)]; opening_bytes sizes the buffers (pcs_opening_bytes_bn254 for the BN254 entries)"""
    n = len(cms)
    m = max(n, 1)
    cap = max([opening_bytes(cm.nvars, k, n_queries, cm.log2_row) for cm, k in zip(cms, counts)] + [8])
    hs = (C.c_void_p * m)(*[cm.h for cm in cms])
    nc = (C.c_size_t * m)(*counts)
    buf = np.zeros(m * cap, dtype=np.uint8)
    lens, status = (C.c_size_t * m)(), (C.c_int * m)()
    reasons = C.create_string_buffer(m * reason_cap)
    _check(call(hs, nc, n_queries, n, buf.ctypes.data_as(u8p), cap, lens, status, reasons, reason_cap))
    raw = reasons.raw
    return [(None if status[i] else buf[i * cap:i * cap + lens[i]].tobytes(), raw[i * reason_cap:(i + 1) * reason_cap].split(b"\0", 1)[0].decode()) for i in range(n)]


def _pcs_open_batch_of(sfx, arrays_of, opening_bytes, ctx, cms, claims_list, n_queries, reason_cap, entry="hg_pcs_open_batch"):
    """hg_pcs_open_batch + sfx (or the `entry` of its argument list) on claim lists that arrays_of turns into (table, points, values)"""
    if len(cms) != len(claims_list):
        raise ValueError(f"pcs_open_batch{sfx}: one claim list per commitment")
    m = max(len(cms), 1)
    arrays = [arrays_of(c) for c in claims_list]
    tabs = (u32p * m)(*[C.cast(a[0], u32p) for a in arrays])
    pts = (u64p * m)(*[_ptr(a[1]) for a in arrays])
    vals = (u64p * m)(*[_ptr(a[2]) for a in arrays])
    fn = getattr(lib(), entry + sfx)
    return _open_batch(lambda hs, nc, *rest: fn(_h(ctx), hs, tabs, pts, vals, nc, *rest), cms, [len(c) for c in claims_list], n_queries, reason_cap, opening_bytes)


def _claims_open_batch_of(F, opening_bytes, ctx, params, cms, claims_list, n_queries, reason_cap, entry="hg_claims_open_batch"):
    """hg_claims_open_batch of field F (or the `entry` of its argument list)"""
    if len(cms) != len(claims_list):
        raise ValueError(f"claims_open_batch{F.SFX}: one {F.__name__} per commitment")
    claims, nc1, points, nco1, counts = _claims_batch_arrays(claims_list, F)
    fn = getattr(lib(), entry + F.SFX)
    return _open_batch(lambda hs, nc, *rest: fn(_h(ctx), C.byref(params), hs, claims, nc1, _ptr(points), nco1, nc, *rest), cms, list(counts)[:len(cms)], n_queries, reason_cap,
                       opening_bytes)


def pcs_open_batch(ctx, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_pcs_open_batch: claims_list[i] (claims as Commitment.open takes them; an empty list is allowed) opened against the device
    Commitment cms[i], all of one shape: [(bytes or None, reason)] - the bytes of cms[i].open(claims_list[i]), or None and the text of
    its error where a value is not the evaluation."""
    return _pcs_open_batch_of("", _pcs_claim_arrays, pcs_opening_bytes, ctx, cms, claims_list, n_queries, reason_cap)


def claims_open_batch(ctx, params, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_claims_open_batch: the InputClaims claims_list[i] (what verify_public_batch returns; None stands for no claims) opened
    against the Commitment.secrets / secrets_batch handle cms[i]: [(bytes or None, reason)]."""
    return _claims_open_batch_of(InputClaims, pcs_opening_bytes, ctx, params, cms, claims_list, n_queries, reason_cap)


def _folded_bytes(nvars, n_claims, n_queries, log2_row):
    """pcs_folded_opening_bytes with the argument list of pcs_opening_bytes: the length does not depend on the claims"""
    return pcs_folded_opening_bytes(nvars, n_queries, log2_row)


def pcs_open_folded_batch(ctx, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_pcs_open_folded_batch: pcs_open_batch for folded openings (every claim list holds a claim): [(bytes or None, reason)] - the
    bytes of cms[i].open_folded(claims_list[i]), or None and the text of its error where a value is not the evaluation."""
    return _pcs_open_batch_of("", _pcs_claim_arrays, _folded_bytes, ctx, cms, claims_list, n_queries, reason_cap, "hg_pcs_open_folded_batch")


def claims_open_folded_batch(ctx, params, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_claims_open_folded_batch: claims_open_batch for folded openings: [(bytes or None, reason)] - the bytes of
    cms[i].open_claims_folded(params, claims_list[i])."""
    return _claims_open_batch_of(InputClaims, _folded_bytes, ctx, params, cms, claims_list, n_queries, reason_cap, "hg_claims_open_folded_batch")


def pcs_open_batch_bn254(ctx, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_pcs_open_batch_bn254: pcs_open_batch over bn256::Fr on device BN254 Commitments, claims as Commitment.open takes them on a
    BN254 handle: [(bytes or None, reason)] - the bytes of cms[i].open(claims_list[i]), or None and the text of its error."""
    return _pcs_open_batch_of("_bn254", _pcs_claim_arrays_bn254, pcs_opening_bytes_bn254, ctx, cms, claims_list, n_queries, reason_cap)


def claims_open_batch_bn254(ctx, params, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_claims_open_batch_bn254: the InputClaimsBn254 claims_list[i] (what verify_public_batch_bn254 returns; None stands for no
    claims) opened against the Commitment.secrets_bn254 / secrets_batch_bn254 handle cms[i]: [(bytes or None, reason)]."""
    return _claims_open_batch_of(InputClaimsBn254, pcs_opening_bytes_bn254, ctx, params, cms, claims_list, n_queries, reason_cap)


def _folded_bytes_bn254(nvars, n_claims, n_queries, log2_row):
    """pcs_folded_opening_bytes_bn254 with the argument list of pcs_opening_bytes_bn254"""
    return pcs_folded_opening_bytes_bn254(nvars, n_queries, log2_row)


def pcs_open_folded_batch_bn254(ctx, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_pcs_open_folded_batch_bn254: pcs_open_batch_bn254 for folded openings (every claim list holds a claim): [(bytes or None,
    reason)] - the bytes of cms[i].open_folded(claims_list[i]), or None and the text of its error where a value is not the evaluation."""
    return _pcs_open_batch_of("_bn254", _pcs_claim_arrays_bn254, _folded_bytes_bn254, ctx, cms, claims_list, n_queries, reason_cap, "hg_pcs_open_folded_batch")


def claims_open_folded_batch_bn254(ctx, params, cms, claims_list, n_queries=0, reason_cap=256):
    """hg_claims_open_folded_batch_bn254: claims_open_batch_bn254 for folded openings: [(bytes or None, reason)] - the bytes of
    cms[i].open_claims_folded(params, claims_list[i])."""
    return _claims_open_batch_of(InputClaimsBn254, _folded_bytes_bn254, ctx, params, cms, claims_list, n_queries, reason_cap, "hg_claims_open_folded_batch")


def _pcs_verify(sfx, arrays, root, nvars, claims, proof, n_queries, log2_row, ctx, form=""):
    """form "_folded": the folded verifiers"""
    nv = (C.c_uint32 * len(nvars))(*nvars)
    table, pts, vals = arrays(claims)
    args = (bytes(root), nv, len(nvars), log2_row, table, _ptr(pts), _ptr(vals), len(claims), n_queries, bytes(proof), len(proof))
    L = lib()
    return _decision(getattr(L, "hg_pcs_verify" + form + sfx)(*args) if ctx is None else getattr(L, "hg_pcs_verify" + form + "_device" + sfx)(ctx.h, *args))


def _claims_verify(sfx, params, root, claims, opening, n_queries, log2_row, ctx, form=""):
    args = (C.byref(params), bytes(root), log2_row, claims.claims, claims.n, _ptr(claims.points), n_queries, bytes(opening), len(opening))
    L = lib()
    return _decision(getattr(L, "hg_claims_verify" + form + sfx)(*args) if ctx is None else getattr(L, "hg_claims_verify" + form + "_device" + sfx)(ctx.h, *args))


def pcs_verify(root, nvars, claims, proof, n_queries=0, log2_row=0, ctx=None):
    """hg_pcs_verify, with a context hg_pcs_verify_device: (accepted, reason). claims as Commitment.open takes them."""
    return _pcs_verify("", _pcs_claim_arrays, root, nvars, claims, proof, n_queries, log2_row, ctx)


def claims_verify(params, root, claims, opening, n_queries=0, log2_row=0, ctx=None):
    """hg_claims_verify, with a context hg_claims_verify_device: an InputClaims against the root of hg_secrets_commit: (accepted, reason)."""
    return _claims_verify("", params, root, claims, opening, n_queries, log2_row, ctx)


def pcs_verify_folded(root, nvars, claims, proof, n_queries=0, log2_row=0, ctx=None):
    """hg_pcs_verify_folded, with a context hg_pcs_verify_folded_device: (accepted, reason) for a folded opening."""
    return _pcs_verify("", _pcs_claim_arrays, root, nvars, claims, proof, n_queries, log2_row, ctx, "_folded")


def claims_verify_folded(params, root, claims, opening, n_queries=0, log2_row=0, ctx=None):
    """hg_claims_verify_folded, with a context hg_claims_verify_folded_device: claims_verify for a folded opening."""
    return _claims_verify("", params, root, claims, opening, n_queries, log2_row, ctx, "_folded")


def _pcs_verify_batch(call, roots, proofs, reason_cap):
    """One call of a batch entry of the commitment: call(roots, proofs, lens, n, results, reasons, reason_cap) -> [(accepted, reason)]"""
    n = len(proofs)
    m = max(n, 1)
    rs = (C.c_char_p * m)(*[bytes(r) for r in roots])
    ps = (C.c_char_p * m)(*[bytes(p) for p in proofs])
    lens = (C.c_size_t * m)(*[len(p) for p in proofs])
    res = (C.c_int * m)()
    reasons = C.create_string_buffer(m * reason_cap)
    if call(rs, ps, lens, n, res, reasons, reason_cap) < 0:
        raise HgError(lib().hg_last_error().decode())
    raw = reasons.raw
    return [(res[i] == 0, raw[i * reason_cap:(i + 1) * reason_cap].split(b"\0", 1)[0].decode()) for i in range(n)]


def _pcs_verify_batch_of(sfx, arrays_of, ctx, roots, nvars, claims_list, proofs, n_queries, log2_row, reason_cap, entry="hg_pcs_verify_device_batch"):
    """hg_pcs_verify_device_batch + sfx (or the `entry` of its argument list) on claim lists that arrays_of turns into (table, points, values)"""
    if not (len(roots) == len(claims_list) == len(proofs)):
        raise ValueError(f"pcs_verify_batch{sfx}: one root and one claim list per opening")
    m = max(len(proofs), 1)
    nv = (C.c_uint32 * len(nvars))(*nvars)
    arrays = [arrays_of(c) for c in claims_list]
    tabs = (u32p * m)(*[C.cast(a[0], u32p) for a in arrays])
    pts = (u64p * m)(*[_ptr(a[1]) for a in arrays])
    vals = (u64p * m)(*[_ptr(a[2]) for a in arrays])
    counts = (C.c_size_t * m)(*[len(c) for c in claims_list])
    fn = getattr(lib(), entry + sfx)
    return _pcs_verify_batch(lambda rs, ps, lens, n, res, reasons, cap: fn(_h(ctx), rs, nv, len(nvars), log2_row, tabs, pts, vals, counts, n_queries, ps, lens, n,
                                                                            res, reasons, cap), roots, proofs, reason_cap)


def pcs_verify_batch(ctx, roots, nvars, claims_list, proofs, n_queries=0, log2_row=0, reason_cap=256):
    """hg_pcs_verify_device_batch: opening i against roots[i] and claims_list[i] (claims as Commitment.open takes them; an empty list
    is allowed), every item of the shape nvars: a list of (accepted, reason), the decisions of pcs_verify for each item alone."""
    return _pcs_verify_batch_of("", _pcs_claim_arrays, ctx, roots, nvars, claims_list, proofs, n_queries, log2_row, reason_cap)


def _claims_batch_arrays(claims_list, F=InputClaims):
    """a list of InputClaims of field F (None: no claims) in the layout hg_verify_public_batch and its _bn254 form write: (claims,
    claim_cap_each, points, coord_cap_each, counts); point_off counts from the item's own block"""
    W = F.WORDS
    m = max(len(claims_list), 1)
    held = [c for c in claims_list if c is not None]
    nc1 = max([c.n for c in held] + [1])
    nco1 = max([sum(int(x.nvars) for x in c.claims[:c.n]) for c in held] + [1])
    claims = (F.STRUCT * (m * nc1))()
    points = np.zeros(W * m * nco1, dtype=np.uint64)
    counts = (C.c_size_t * m)()
    for i, c in enumerate(claims_list):
        if c is None:
            continue
        counts[i], off = c.n, 0
        for j in range(c.n):
            src, dst = c.claims[j], claims[i * nc1 + j]
            dst.input, dst.nvars, dst.point_off = src.input, src.nvars, off
            for w in range(W):
                dst.value[w] = src.value[w]
            points[W * (i * nco1 + off):W * (i * nco1 + off + src.nvars)] = c.points[W * src.point_off:W * (src.point_off + src.nvars)]
            off += src.nvars
    return claims, nc1, points, nco1, counts


def _claims_verify_batch_of(F, ctx, params, roots, claims_list, openings, n_queries, log2_row, reason_cap, entry="hg_claims_verify_batch"):
    """hg_claims_verify_batch of field F (or the `entry` of its argument list)"""
    if not (len(roots) == len(claims_list) == len(openings)):
        raise ValueError(f"claims_verify_batch{F.SFX}: one root and one {F.__name__} per opening")
    claims, nc1, points, nco1, counts = _claims_batch_arrays(claims_list, F)
    fn = getattr(lib(), entry + F.SFX)
    return _pcs_verify_batch(lambda rs, ps, lens, n, res, reasons, cap: fn(_h(ctx), C.byref(params), rs, log2_row, claims, nc1, _ptr(points), nco1, counts, n_queries,
                                                                            ps, lens, n, res, reasons, cap), roots, openings, reason_cap)


def claims_verify_batch(ctx, params, roots, claims_list, openings, n_queries=0, log2_row=0, reason_cap=256):
    """hg_claims_verify_batch: opening i against roots[i] and the InputClaims claims_list[i] (what verify_public_batch returns; None
    stands for no claims), packed into the layout hg_verify_public_batch writes: a list of (accepted, reason), the decisions of
    claims_verify for each item alone."""
    return _claims_verify_batch_of(InputClaims, ctx, params, roots, claims_list, openings, n_queries, log2_row, reason_cap)


def pcs_verify_folded_batch(ctx, roots, nvars, claims_list, proofs, n_queries=0, log2_row=0, reason_cap=256):
    """hg_pcs_verify_folded_device_batch: pcs_verify_batch for folded openings (every claim list holds a claim): a list of (accepted,
    reason), the decisions of pcs_verify_folded for each item alone."""
    return _pcs_verify_batch_of("", _pcs_claim_arrays, ctx, roots, nvars, claims_list, proofs, n_queries, log2_row, reason_cap, "hg_pcs_verify_folded_device_batch")


def claims_verify_folded_batch(ctx, params, roots, claims_list, openings, n_queries=0, log2_row=0, reason_cap=256):
    """hg_claims_verify_folded_batch: claims_verify_batch for folded openings: a list of (accepted, reason), the decisions of
    claims_verify_folded for each item alone; an item without claims (None) is rejected, not an error."""
    return _claims_verify_batch_of(InputClaims, ctx, params, roots, claims_list, openings, n_queries, log2_row, reason_cap, "hg_claims_verify_folded_batch")


def pcs_verify_batch_bn254(ctx, roots, nvars, claims_list, proofs, n_queries=0, log2_row=0, reason_cap=256):
    """hg_pcs_verify_device_batch_bn254: pcs_verify_batch over bn256::Fr, claims as Commitment.open takes them on a BN254 handle: a
    list of (accepted, reason), the decisions of pcs_verify_bn254 for each item alone."""
    return _pcs_verify_batch_of("_bn254", _pcs_claim_arrays_bn254, ctx, roots, nvars, claims_list, proofs, n_queries, log2_row, reason_cap)


def claims_verify_batch_bn254(ctx, params, roots, claims_list, openings, n_queries=0, log2_row=0, reason_cap=256):
    """hg_claims_verify_batch_bn254: claims_verify_batch on InputClaimsBn254 objects (what verify_public_batch_bn254 returns; None
    stands for no claims): a list of (accepted, reason), the decisions of claims_verify_bn254 for each item alone."""
    return _claims_verify_batch_of(InputClaimsBn254, ctx, params, roots, claims_list, openings, n_queries, log2_row, reason_cap)


def pcs_verify_folded_batch_bn254(ctx, roots, nvars, claims_list, proofs, n_queries=0, log2_row=0, reason_cap=256):
    """hg_pcs_verify_folded_device_batch_bn254: pcs_verify_batch_bn254 for folded openings (every claim list holds a claim): a list of
    (accepted, reason), the decisions of pcs_verify_folded_bn254 for each item alone."""
    return _pcs_verify_batch_of("_bn254", _pcs_claim_arrays_bn254, ctx, roots, nvars, claims_list, proofs, n_queries, log2_row, reason_cap, "hg_pcs_verify_folded_device_batch")


def claims_verify_folded_batch_bn254(ctx, params, roots, claims_list, openings, n_queries=0, log2_row=0, reason_cap=256):
    """hg_claims_verify_folded_batch_bn254: claims_verify_batch_bn254 for folded openings: a list of (accepted, reason), the decisions
    of claims_verify_folded_bn254 for each item alone; an item without claims (None) is rejected, not an error."""
    return _claims_verify_batch_of(InputClaimsBn254, ctx, params, roots, claims_list, openings, n_queries, log2_row, reason_cap, "hg_claims_verify_folded_batch")


def pcs_verify_bn254(root, nvars, claims, proof, n_queries=0, log2_row=0, ctx=None):
    """hg_pcs_verify_bn254, with a context hg_pcs_verify_device_bn254: (accepted, reason). claims as Commitment.open takes them on a
    BN254 handle."""
    return _pcs_verify("_bn254", _pcs_claim_arrays_bn254, root, nvars, claims, proof, n_queries, log2_row, ctx)


def claims_verify_bn254(params, root, claims, opening, n_queries=0, log2_row=0, ctx=None):
    """hg_claims_verify_bn254, with a context hg_claims_verify_device_bn254: an InputClaimsBn254 against the root of
    hg_secrets_commit_bn254: (accepted, reason)."""
    return _claims_verify("_bn254", params, root, claims, opening, n_queries, log2_row, ctx)


def pcs_verify_folded_bn254(root, nvars, claims, proof, n_queries=0, log2_row=0, ctx=None):
    """hg_pcs_verify_folded_bn254, with a context hg_pcs_verify_folded_device_bn254: (accepted, reason) for a folded BN254 opening."""
    return _pcs_verify("_bn254", _pcs_claim_arrays_bn254, root, nvars, claims, proof, n_queries, log2_row, ctx, "_folded")


def claims_verify_folded_bn254(params, root, claims, opening, n_queries=0, log2_row=0, ctx=None):
    """hg_claims_verify_folded_bn254, with a context hg_claims_verify_folded_device_bn254: claims_verify_bn254 for a folded opening."""
    return _claims_verify("_bn254", params, root, claims, opening, n_queries, log2_row, ctx, "_folded")


class LassoNode:
    """Mirror of `LassoNode<F, E, 4, 65536>` as a gkr Node [REF lasso/src/lasso.rs:32-140]."""

    def __init__(self, pk):
        self.pk = pk

    def prove_claim_reduction(self, ctx, inputs, cap=1 << 24, chain_skip=0):
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        assert inputs.size == 1 << self.pk.nu
        buf = (C.c_uint8 * cap)()
        ln = C.c_size_t(0)
        claim = np.zeros(2 * self.pk.nu + 2, dtype=np.uint64)
        _check(lib().hg_lasso_prove_at(ctx.h, self.pk.h, _ptr(inputs), chain_skip, buf, cap, C.byref(ln), _ptr(claim)))
        return bytes(buf[:ln.value]), claim
