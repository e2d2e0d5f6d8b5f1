/* hyper-greco-amd: C ABI of the MI355X-native GKR prover for the BFV secret-key-encryption circuit.
 *
 * This is the drop-in boundary: plain C, caller-owned buffers, `int` status
 * (0 = OK, negative = error, text via hg_last_error()). Field elements cross the boundary as
 * canonical little-endian u64 limbs (Goldilocks: 1 limb; GoldilocksExt2: 2 limbs [c0, c1]); proof
 * bytes use the reference wire format (canonical repr, big-endian, ext = bases in order)
 * [REF bfv-gkr/src/transcript.rs:183-195].
 *
 * Each entry point names the reference interface it replaces. The Rust-side binding a maintainer
 * would add is shown in INTEGRATION.md.
 */
#ifndef HG_H
#define HG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_MAX_K 16

typedef struct hg_ctx hg_ctx;         /* one per GPU: stream, workspace arena, cached challenge chain */
typedef struct hg_pk hg_pk;           /* prover key = LassoPreprocessing + circuit wiring, device resident */
typedef struct hg_witness hg_witness; /* BfvSkEncryptArgs after get_inputs(): laid-out field tables (host) */
typedef struct hg_values hg_values;   /* circuit.evaluate() result: every node's table, resident in HBM */
typedef struct hg_group hg_group;     /* the ranks of a sharded round-by-round prove: who adds the partial round sums */
typedef struct hg_instance hg_instance; /* the public instance of one encryption: a_i and ct0_i, host. Crosses the ABI as void* */

/* Per-parameter-set constants [REF bfv-gkr/src/constants/mod.rs:16-35, constants/sk_enc_constants_*.rs] */
typedef struct hg_params {
    uint32_t n;        /* ring degree N */
    uint32_t k;        /* number of CRT moduli (const generic K) */
    uint64_t s_bound, e_bound, k1_bound;
    uint64_t r1_bounds[HG_MAX_K], r2_bounds[HG_MAX_K];
    uint64_t qis[HG_MAX_K], k0is[HG_MAX_K];
} hg_params;

typedef struct hg_timings {
    double witness_ms; /* "wintess gen" span: circuit.evaluate + output claim [REF sk_encryption_circuit.rs:439-453] */
    double upload_ms;  /* host -> HBM copy of node values (not part of any reference span) */
    double prove_ms;   /* "GKR prove" span [REF sk_encryption_circuit.rs:455-457]: HIP events on the prover stream,
                          node values resident in HBM at start; wall clock from the
                          first launch to the assembled proof bytes (includes host launch + transcript replay) */
    double gpu_ms;     /* the same span measured with HIP events on the prover stream (device time only) */
    double total_ms;   /* wall clock of the whole hg_prove call */
    double enqueue_ms; /* host time spent walking the protocol and launching (part of prove_ms) */
    double sync_ms;    /* host wait for the stream after the last launch (part of prove_ms) */
    double replay_ms;  /* host transcript replay: interpolation, claim chaining, proof bytes (part of prove_ms) */
} hg_timings;

/* Per-kernel-class profile (HIP events recorded on the prover stream around every launch of the class). */
typedef struct hg_kernel_stat {
    char name[48];
    uint64_t launches;
    double total_ms;
    double algo_bytes; /* algorithmic bytes over all launches: tables read once + folded tables written once */
    double model_bytes; /* the same launches in the traffic model of the REFERENCE's algorithm: larger than algo_bytes
                           where an algebraic shortcut avoids tables (mirrored grand product, two-table collation sum-check) */
    double hbm_bytes;   /* what the launches move to or from HBM BY DESIGN: every table a launch reads and every table it writes, once -
                           nothing for tables that are recomputed and never stored (the hash rows of the first grand-product round), for
                           the intermediate folds of a two-round launch, or for rounds that run inside LDS */
} hg_kernel_stat;

const char* hg_last_error(void);
int hg_device_count(void);

/* = nothing in the reference (single-process rayon); one ctx per device, calls on a ctx are serialised by the caller */
hg_ctx* hg_create(int device_id);
void hg_destroy(hg_ctx* ctx);

/* Context options (nothing in the reference: its only knob is the rayon pool). name:
 *   "one_stream"  value != 0: every launch on one stream (the default overlaps the Vanilla / FFT node reductions, the counter
 *                 sorts and the openings with the Lasso node's critical path on a second stream); used to time kernels in isolation
 *   "graph"       value == 0: never replay a cached launch graph (default: after two ordinary resident proves of the same key and
 *                 values object the third is captured into a hipGraph and later ones replay it - the launch sequence depends on
 *                 addresses only, because every challenge is known up front; a values object refilled by hg_witness_gen_into
 *                 keeps its graph; up to HG_GRAPH_ENTRIES (8) graphs per context, each with a private workspace)
 *   "gp_claims_device"  value == 0: the grand products' layer claims (unscaled evaluations, the mu fold, the next layer's claim) are
 *                 formed by the transcript replay on the host (default 1: by the tail kernel that writes the layer's evaluations;
 *                 a sharded rank, the sound modes and BN254 always use the host form). Same proof bytes; a change drops the
 *                 context's cached launch graphs
 *   "graph_const_tables"  value == 0: a launch graph records every launch of the prove (default 1: the launches that build tables
 *                 of the challenge chain and the prover key alone - eq and DFT-row tables, Libra tables without a mul part - run
 *                 once after the capture and are not part of the replays; one rank, mode 0). Same proof bytes; a change drops
 *                 the context's cached launch graphs
 *   "verify_batch_group"  the most proofs one device pass of hg_verify_device_batch, hg_verify_device_batch_bn254,
 *                 hg_verify_public_batch, hg_verify_public_bound_batch or hg_verify_public_batch_bn254 holds (and
 *                 hg_instance_digest_group stages), and the most openings one of
 *                 hg_pcs_verify_device_batch, hg_claims_verify_batch, hg_pcs_verify_device_batch_bn254 or
 *                 hg_claims_verify_batch_bn254, the most members one device pass of hg_pcs_commit_batch, hg_secrets_commit_batch,
 *                 hg_pcs_commit_batch_bn254 or hg_secrets_commit_batch_bn254 encodes and the most items one of hg_pcs_open_batch,
 *                 hg_claims_open_batch, hg_pcs_open_batch_bn254, hg_claims_open_batch_bn254, hg_pcs_open_folded_batch,
 *                 hg_claims_open_folded_batch, hg_pcs_open_folded_batch_bn254 or hg_claims_open_folded_batch_bn254 opens (default 0:
 *                 sized from the memory budget, at most 64)
 *   "bound_batch_slice"  the members of a group that hg_verify_public_bound_batch and hg_instance_digest_group gather, copy and
 *                 digest at a time (default 0: as many as fit in 32 MiB of instance words, at least one: 4 at n=32768 k=16); a
 *                 slice's copy and digests run under the gather of the next one. Results do not depend on it
 * Returns 0, or -1 for an unknown name. */
int hg_set_option(hg_ctx* ctx, const char* name, int64_t value);

/* = `type Params = constants::SkEnc{N}_{K}x{bits}_65537` [REF bfv-gkr/src/test.rs:8] */
int hg_params_builtin(uint32_t n, uint32_t k, hg_params* out);

/* = the constants emitter of scripts/circuit_sk.py [REF scripts/circuit_sk.py:80, 249, 296-297, 334-337, 422-439]: a parameter set
 *   for ring degree n, k CRT moduli qis[] and plaintext modulus t, so that (n, k) can be swept beyond the six shipped sets.
 *   S_BOUND = 1, E_BOUND = 19, K1_BOUND = (t-1)/2, K0_i = (-t)^-1 mod q_i, R2_BOUND_i = int((q_i - 1) / 2) and
 *   R1_BOUND_i = int((int((q_i-1)/2) (n+2) + 19 + int((t-1)/2) K0_i) / q_i), with the script's float semantics of "/" reproduced
 *   (that is why shipped R2 bounds are doubles rounded to 53 bits). n must be a power of two, k one of 1, 2, 4, 8, 16. */
int hg_params_derive(uint32_t n, uint32_t k, const uint64_t* qis, uint64_t t, hg_params* out);

/* = BfvEncrypt::setup -> LassoPreprocessing::preprocess::<4, 65536> [REF sk_encryption_circuit.rs:319-349, lasso.rs:527-627]
 *   plus BfvEncrypt::configure (circuit wiring) [REF sk_encryption_circuit.rs:351-363, 86-293], done once. */
int hg_setup(hg_ctx* ctx, const hg_params* params, hg_pk** pk); /* ctx == NULL: host-only key (layout / circuit_eval) */
void hg_pk_free(hg_pk* pk);
/* Lasso memory map as text "subtable@dim,...|lookup:bits:m/m;..." (for tests) */
int hg_pk_lasso_layout(const hg_pk* pk, char* out, size_t cap);
/* [nu, num_nodes, rows, alpha, NodeId of lasso_inputs_batched, NodeId of sum] */
int hg_pk_info(const hg_pk* pk, uint64_t out[6]);
/* How hg_setup classified one node of the circuit (for tests; host-only keys too): [kind (0 input, 1 Vanilla, 2 FFT, 3 Lasso),
 * eq-factored form found (every Libra phase-1 table of the node is a constant times an eq table: VanillaNode wirings that relay aligned
 * blocks, sk_encryption_circuit.rs:97-285), log2 of the relayed block, index of the input window, number of (coefficient, gate block)
 * terms, log2 of the input size]. Whether a prove uses the form also depends on the node having ONE claim and on its size. */
int hg_pk_node_eq_form(const hg_pk* pk, int node, int64_t out[6]);

/* = serde_json::from_str::<BfvSkEncryptArgs> + BfvEncrypt::get_inputs / Poly::{new,new_padded,new_shifted}
 *   [REF bfv-gkr/src/test.rs:21-33, sk_encryption_circuit.rs:365-415, poly.rs:12-44] */
int hg_witness_from_json(const hg_params* params, const char* path, hg_witness** w);
/* Replaces scripts/circuit_sk.py (offline witness generator) with a seeded synthetic BFV sk-encryption
 * [REF scripts/circuit_sk.py:18-140, scripts/utils.py:4-18]; needed because the n=32768 fixture is a missing blob. */
int hg_witness_synthetic(const hg_params* params, uint64_t seed, hg_witness** w);   /* caller-supplied secrets: hg_witness_derive */
/* Already laid-out tables: s,e,k1: 2^L; ais,r1is: k*2^L; r2is: k*2^P; ct0is: k*2^L (L = log2 n + 1, P = log2 n) */
int hg_witness_from_arrays(const hg_params* params, const uint64_t* s, const uint64_t* e, const uint64_t* k1,
                           const uint64_t* ais, const uint64_t* r1is, const uint64_t* r2is, const uint64_t* ct0is,
                           hg_witness** w);
/* = the witness half of scripts/circuit_sk.py for secrets the CALLER holds [REF scripts/circuit_sk.py:18-140], on the device: from
 *   the laid-out tables s, e, k1 (2^L each) and ais (k*2^L) of hg_witness_from_arrays it derives ct0is, r2is and r1is - per modulus
 *   h = a_i s + e + k0_i k1 over Z (2k+1 Goldilocks NTTs of size 2n on 32-bit halves of a_i), ct0_i = h mod (X^n + 1, q_i) centred,
 *   r2_i = cmod(-h[j+n], q_i), r1_i = (ct0_i - h - r2_i (X^n + 1)) / q_i - and returns the handle hg_witness_from_arrays would
 *   return for all seven tables. Needs a device context; never falls back to the host.
 *   Errors (-1, text in hg_last_error, *w = NULL): null argument; no context; a word >= p; a coefficient of s / e / k1 outside
 *   s_bound / e_bound / k1_bound, of a_i outside [-(q_i-1)/2, (q_i-1)/2], or a nonzero word where the layout pads; a derived r1_i /
 *   r2_i coefficient outside its bound in params (table and modulus are named: such a witness cannot be proven, its Lasso lookups
 *   fail); an even q_i, q_i >= 2^62, or parameters for which the products are not exact below p/2 or h leaves the 128-bit reduction. */
int hg_witness_derive(hg_ctx* ctx, const hg_params* params, const uint64_t* s, const uint64_t* e, const uint64_t* k1,
                      const uint64_t* ais, hg_witness** w);
/* which: 0 s, 1 e, 2 k1, 3 ais, 4 r1is, 5 r2is, 6 ct0is. Returns the element count (copies min(count, cap)). */
int64_t hg_witness_get(const hg_witness* w, int which, uint64_t* out, size_t cap);
void hg_witness_free(hg_witness* w);

/* = BfvEncrypt::prove [REF sk_encryption_circuit.rs:417-460]. Fails (never falls back to a CPU path)
 *   when no HIP device is available. */
int hg_prove(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, uint8_t* proof, size_t cap, size_t* len,
             hg_timings* timings);

/* Makes the FIRST hg_prove of a key a warm one - what a drop-in BfvEncrypt::setup calls right after hg_setup [REF the caller's sequence
 *   bfv-gkr/src/test.rs:31-44: setup, then ONE prove per witness]: allocates the context-owned node tables and the page-locked witness
 *   staging, proves an all-zero witness until the launch graph of those tables is recorded (two protocol walks and the capture; nothing
 *   of it depends on table contents), so that the first real hg_prove refills the tables in place and replays the graph. *ms (may be
 *   NULL): the time it took. Optional: without it the first two hg_prove calls of a key walk the protocol and the third records. */
int hg_warmup(hg_ctx* ctx, const hg_pk* pk, double* ms);

/* hg_prove for a run of `n` witnesses under one key, pipelined [REF: the loop a caller of BfvEncrypt::prove writes; the only
 *   in-tree caller is the test macro bfv-gkr/src/test.rs:31-44, one witness per call - the reference has no batch entry]: upload + circuit.evaluate of witness i+1 run on a third stream into a second set of node
 *   tables while witness i is proven. Proof i is written at proofs + i*cap_each, its length to lens[i]; each proof is byte-identical
 *   to hg_prove's for that witness. timings (may be NULL): total_ms = wall clock of the whole run, prove_ms / gpu_ms = sums over
 *   the proofs. The first proofs of a context + key walk the protocol (the launch graph of a table set is recorded on its third
 *   prove); after that a proof costs about max(prove, upload + evaluate). */
int hg_prove_stream(hg_ctx* ctx, const hg_pk* pk, const hg_witness* const* ws, size_t n, uint8_t* proofs, size_t cap_each,
                    size_t* lens, hg_timings* timings);

/* = BfvEncrypt::get_inputs / Poly::{new_padded, new_shifted} [REF sk_encryption_circuit.rs:365-415, poly.rs:20-44] for the four
 *   polynomials an encryptor holds, as SIGNED coefficients in ASCENDING degree: s, e, k1: n coefficients; a: k*n (modulus-major).
 *   Writes the laid-out tables hg_witness_derive / hg_witness_from_arrays take (s_t, e_t, k1_t: 2^L words, ais_t: k*2^L): coefficient
 *   j of s and of a_i at word n-1-j, of e and k1 at word 2n-2-j, every other word zero, a negative z as p - |z| [REF scripts/utils.py:
 *   4-18]. Host only, no context. Bounds are not checked here (the derivation checks them); INT64_MIN or a null argument: -1. */
int hg_encryption_layout(const hg_params* params, const int64_t* s, const int64_t* e, const int64_t* k1, const int64_t* a,
                         uint64_t* s_t, uint64_t* e_t, uint64_t* k1_t, uint64_t* ais_t);
/* hg_witness_derive and hg_prove for a run of n_enc ENCRYPTIONS under one key, pipelined [REF scripts/circuit_sk.py:18-140 followed by
 *   sk_encryption_circuit.rs:417-460; the loop a proving service writes around them - the reference has no batch entry]: s[i], e[i],
 *   k1[i] (n each) and a[i] (k*n) are the signed ascending polynomials of hg_encryption_layout. They cross the bus as they are
 *   ((3+k) n words, a quarter of the laid-out tables); one kernel lays the tables out on the device, checks every coefficient and
 *   feeds the derivation; derivation and circuit.evaluate of encryption i+1 run on a third stream, in buffers of their own, into a
 *   second set of node tables while encryption i is proven. Proof i is written at proofs + i*cap_each, its length to lens[i], and is
 *   byte-identical to hg_prove of hg_witness_derive of the laid-out inputs. ws (may be NULL): ws[i] = the handle hg_witness_derive
 *   would return (all seven tables; the caller frees it).
 *   status[i] = 0 proven, 1 REFUSED: a check of hg_witness_derive failed (a coefficient of s / e / k1 outside its bound, of a_i outside
 *   [-(q_i-1)/2, (q_i-1)/2], a derived r1_i / r2_i outside its bound, an inexact quotient). A refused encryption is never proven:
 *   lens[i] = 0, ws[i] = NULL, no proof bytes; reasons (may be NULL) receives at reasons + i*reason_cap the text that names table,
 *   modulus and cause, NUL-terminated and truncated to reason_cap bytes ("" when proven). The run continues; the other proofs are
 *   what they would be without the refused item.
 *   Returns the number of refused encryptions (>= 0; n_enc == 0 returns 0), or -1 on an error of the call: a null argument, no
 *   context, a host-only key, a proof larger than cap_each, parameters the derivation cannot serve (hg_witness_derive's last error
 *   class). hg_last_error names the function and, where it applies, the index.
 *   timings (may be NULL): total_ms = wall clock of the run; prove_ms / gpu_ms / replay_ms = sums over the proven items; witness_ms =
 *   sum over the proven items of the device time of upload + derivation + evaluation (HIP events on the stream they run on).
 *   The first proofs of a context + key walk the protocol one after the other (the launch graph of a table set is recorded on its
 *   third prove, as in hg_prove_stream); after that a proof costs about max(prove, derive + evaluate). */
int hg_prove_encryptions(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                         const int64_t* const* a, size_t n_enc, uint8_t* proofs, size_t cap_each, size_t* lens, int* status,
                         hg_witness** ws, char* reasons, size_t reason_cap, hg_timings* timings);

/* = BfvEncrypt::verify [REF sk_encryption_circuit.rs:462-517] (host-side, like the reference's): the witness handle
 *   supplies the public inputs and ct0is. Returns 0 = accepted, 1 = rejected (reason via hg_last_error), < 0 = error.
 *   Works with a host-only key (hg_setup(NULL, ..)).
 *   NOTE: "accepted" means what the reference's verifier means, which is NOT soundness: the challenges are a fixed Keccak chain
 *   independent of the proof bytes, gamma / tau are truncated to one base limb, the collation sum-check's final evaluation, the
 *   final evaluation of every grand-product layer's sum-check (verify_grand_product discards it and keeps the point) and
 *   the multiset relation init * write == read * final between the two grand products are never checked, trailing bytes are
 *   ignored. hg_verify_mode(.., 3, ..) closes the first two. Every single element of the stream is bound all the same: a proof
 *   with one element changed is rejected in every mode (tests/test_proof_binding.py). */
int hg_verify(const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len);
/* The same check with the table-sized work on the device [REF sk_encryption_circuit.rs:462-517; lasso/src/memory_checking/verifier.rs:
 * 130-176]: the host parses the proof and checks the round polynomials and the Lasso scalars; the eq tables, the wiring-predicate
 * sums of the Vanilla nodes, the DFT rows of the FFT nodes and the MLE evaluations of the public inputs run as kernels (one stream,
 * one synchronisation). Same return values, the same accept / reject decisions and the same reasons as hg_verify (a proof rejected
 * while it is read still has the checks of the Vanilla nodes read so far evaluated: hg_verify makes those first); Goldilocks, mode 0
 * (the protocol modes: hg_verify_device_mode). */
int hg_verify_device(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len);
/* hg_verify_device in a protocol mode (the mode bits of hg_prove_mode / hg_verify_mode below, 0 to 3), Goldilocks only. Mode 0 is
 * hg_verify_device; modes 1 to 3 make the same accept / reject decision as hg_verify_mode in the same mode. The walk records the
 * challenges it squeezes (with bit 1 they depend on the proof bytes) and the kernels read that record, staged into the context's
 * arena; the fixed chain the mode-0 prover reads is left as it is. Of the gaps listed at hg_verify, bit 1 closes the first (the
 * challenges bind every element read), bit 2 the second (gamma, tau in E); mode 3 closes both. The collation sum-check's final
 * evaluation, the final evaluation of every grand-product layer's sum-check, the multiset relation and trailing bytes stay
 * unchecked in every mode. Needs a device context and a device key
 * (hg_setup(ctx, ..)). Returns 0 accept, 1 reject (reason in hg_last_error), -1 error: a null argument, a host-only key, or a mode
 * outside 0..3. */
int hg_verify_device_mode(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int mode, const uint8_t* proof, size_t len);
/* hg_verify_device_mode for a run of n proofs under one key: proof i (proofs[i], lens[i]) is checked against witness ws[i] in
 * `mode` (0..3). results[i] = 0 accepted / 1 rejected, exactly the decision hg_verify_device_mode makes for that pair.
 * reasons (may be NULL): proof i's rejection reason, NUL-terminated and truncated to reason_cap bytes, at reasons + i*reason_cap
 * ("" when accepted). Returns the number of rejected proofs (>= 0), or -1 on an error (hg_last_error names the function and,
 * for an error inside one proof's check, its index). n == 0 returns 0.
 * The walks run on the host threads, the table-sized work of a group of proofs (context option "verify_batch_group") in one
 * launch per kind, tables that depend on the key only built once per group; the inputs of the next group are copied meanwhile. */
int hg_verify_device_batch(hg_ctx* ctx, const hg_pk* pk, const hg_witness* const* ws, const uint8_t* const* proofs,
                           const size_t* lens, size_t n, int mode, int* results, char* reasons, size_t reason_cap);

/* ---- Verification from the ciphertext: the verifier split where the public data ends ------------------------------------------
 * Every verifier above takes an hg_witness, as the reference's verify evaluates EVERY input polynomial at the claim points GKR
 * leaves [REF sk_encryption_circuit.rs:462-517; izip_eq!(inputs, input_claims) :512-516]; five of those seven tables (s, e, k1,
 * r1is, r2is) are the encryptor's secrets. A recipient holds the ciphertext (ct0_i, a_i) and the proof. The entries below decide
 * everything those and the key decide - the output claim, every node reduction, the Lasso scalars, the input claims on the ais
 * tables - and hand back what is left, the claims (input, point, value) on the five secret inputs: what a commitment layer would
 * open (the reference's PCS type parameter is dead): hg_claims_open / hg_claims_verify below. hg_claims_settle checks such claims against a witness handle,
 * which is the reference's contract again: hg_verify_public followed by hg_claims_settle decides what hg_verify_mode decides.
 * Goldilocks, modes 0..3, one proof per call (hg_verify_public_batch: a run of them in one device pass). Over bn256::Fr:
 * hg_verify_public_bn254 and its neighbours, below hg_verify_device_batch_bn254; the instance handle and hg_pk_claim_shape serve
 * both fields (an instance holds signed integers, the claim shape depends on the wiring only).
 * The instance handle (hg_instance*) and the claim array (hg_input_claim*) cross the ABI as void pointers. */
typedef struct hg_input_claim {
    uint32_t input;      /* chain_par! order [REF sk_encryption_circuit.rs:476-481]: 0 s, 1 e, 2 k1, 3+k+i r1is[i], 3+2k r2is (never 3..3+k-1: the claims on ais are settled inside) */
    uint32_t nvars;
    uint64_t point_off;  /* coordinates points[2*point_off .. 2*(point_off+nvars)), (c0, c1) each */
    uint64_t value[2];
} hg_input_claim;

/* = the public half of BfvSkEncryptArgs [REF sk_encryption_circuit.rs:64-73: ais, ct0is] as a recipient holds it. a, ct0: k*n SIGNED
 *   coefficients each, modulus-major, ASCENDING degree (the convention of hg_encryption_layout). Laid out as get_inputs does
 *   [REF sk_encryption_circuit.rs:365-415]: coefficient j of a_i at word n-1-j of ais[i] [REF poly.rs:20-28], of ct0_i at word 2n-2-j of
 *   modulus i's 2n-word block of ct0is (new_shifted to 2^L, the first word dropped, a zero pushed [REF :393-396]), a negative z as
 *   p - |z| [REF scripts/utils.py:4-18]. Every coefficient must lie in [-(q_i-1)/2, (q_i-1)/2], else -1 naming table, modulus and
 *   index. Host only. *out: an hg_instance*. */
int hg_instance_from_ciphertext(const hg_params* params, const int64_t* a, const int64_t* ct0, void** out);
/* The same from a handle: the layout of tables 3 (ais) and 6 (ct0is) inverted. -1 if a padding word is nonzero or a word is not a
 * signed value in that range. */
int hg_instance_from_witness(const hg_params* params, const hg_witness* w, void** out);
void hg_instance_free(void* instance);
/* copies the coefficients back out: a and ct0 receive k*n signed words each, as hg_instance_from_ciphertext takes them */
int hg_instance_coeffs(const void* instance, int64_t* a, int64_t* ct0);
/* the laid-out table the instance stands for, as hg_witness_get returns it: which 0 ais, 1 ct0is (k*2^L words each). Returns the
 * element count (copies min(count, cap)); -1 for a null handle or another selector. */
int64_t hg_instance_get(const void* instance, int which, uint64_t* out, size_t cap);

/* key-only: how many claims on secret inputs a proof of this key leaves, and their coordinates in all (host-only keys too) */
int hg_pk_claim_shape(const hg_pk* pk, size_t* n_claims, size_t* n_coords);

/* = BfvEncrypt::verify [REF sk_encryption_circuit.rs:462-517] up to the point where it needs a secret: the walk of hg_verify_mode in
 *   `mode` (0..3) with ct0is and the ais tables evaluated from the instance's compact coefficients; a claim on any other input is
 *   not evaluated but written out. instance: an hg_instance*; claims: room for claim_cap hg_input_claim; points: room for coord_cap
 *   coordinates (2 words each). Returns 0 accept (claims and points filled, *n_claims set), 1 reject (reason in hg_last_error,
 *   *n_claims = 0; the reasons are hg_verify_mode's), -1 error: a null argument, a mode outside 0..3, claim_cap or coord_cap below
 *   hg_pk_claim_shape, an instance of other parameters; the device form also: no context, a host-only key.
 *   Claim order: inputs ascending, within one input the order in which the walk pushes them; the same for both forms. Points are
 *   always written out as values (in mode 0 they are runs of the fixed chain; the caller still receives the values).
 *   hg_verify_public is the host form (works with hg_setup(NULL, ..)). hg_verify_public_device runs the table-sized work as
 *   hg_verify_device_mode does, with the instance uploaded as it is (2 k n words: 8 MB at n=32768 k=16 against the 22 MB of laid-out
 *   tables) and the MLE evaluations of ais and ct0is in one kernel that reads the signed words and the half of each eq table that
 *   meets a non-padding word; the secret inputs launch nothing. Same decisions, claims and points as the host form, bit for bit. */
int hg_verify_public(const hg_pk* pk, const void* instance, int mode, const uint8_t* proof, size_t len, void* claims, size_t claim_cap,
                     uint64_t* points, size_t coord_cap, size_t* n_claims);
int hg_verify_public_device(hg_ctx* ctx, const hg_pk* pk, const void* instance, int mode, const uint8_t* proof, size_t len, void* claims,
                            size_t claim_cap, uint64_t* points, size_t coord_cap, size_t* n_claims);

/* hg_verify_public_device for a run of n proofs under one key: proof i (proofs[i], lens[i]) is checked against instances[i] (an
 *   hg_instance* of the key's parameters) in `mode` (0..3). Device only. results[i] = 0 accepted / 1 rejected, exactly the decision
 *   hg_verify_public_device makes for that pair alone; reasons (may be NULL): at reasons + i*reason_cap the text that call leaves in
 *   hg_last_error, NUL-terminated and truncated to reason_cap bytes ("" when accepted). An accepted proof i writes its claims at
 *   (hg_input_claim*)claims + i*claim_cap_each and its points at points + 2*i*coord_cap_each, point_off relative to that proof's own
 *   block, and n_claims[i] = the claim count: claim order, values and points are bit for bit those of the single call. A rejected
 *   proof gets n_claims[i] = 0. Returns the number of rejected proofs (>= 0); n == 0 returns 0 and writes nothing; -1 on an error of
 *   the call, which writes no output either (hg_last_error names the function and, where it applies, the index): a null argument or
 *   a null element, no context, a host-only key, a mode outside 0..3, claim_cap_each or coord_cap_each below hg_pk_claim_shape, an
 *   instance of other parameters.
 *   The pass is hg_verify_device_batch's - walks on the host threads, a group of proofs (context option "verify_batch_group", at
 *   most 64) in one launch per kind, key-only tables built once per group, the next group's copies under this group's kernels -
 *   with each proof's instance staged as it is (2 k n signed words) and ais / ct0is evaluated from them by one kernel per group
 *   that reads the non-padding half of each eq table once for all the group's members; the secret inputs launch nothing. */
int hg_verify_public_batch(hg_ctx* ctx, const hg_pk* pk, const void* const* instances, const uint8_t* const* proofs,
                           const size_t* lens, size_t n, int mode, int* results, void* claims, size_t claim_cap_each,
                           uint64_t* points, size_t coord_cap_each, size_t* n_claims, char* reasons, size_t reason_cap);

/* = izip_eq!(inputs, input_claims) [REF sk_encryption_circuit.rs:512-516] for the n claims of an hg_input_claim array: table `input`
 *   of w (any input 0 .. 3+2k) at the point == value, for every claim. ctx == NULL: host; with a context: one batch of eq tables and
 *   dot products on the device, one synchronisation. Returns 0, 1 ("input claim mismatch at input K", the lowest failing K: the
 *   verifiers' text) or -1 (a null argument, a handle of other parameters, no such input, nvars that is not the table's). */
int hg_claims_settle(hg_ctx* ctx, const hg_params* params, const hg_witness* w, const void* claims, size_t n, const uint64_t* points);

/* part exposed for parity tests: the MLE of one laid-out public table at an E point, computed from the compact coefficients
 * (ctx == NULL: host loop; else the kernel of hg_verify_public_device). which 0: ais[index] (L vars); 1: ct0is, the whole table
 * (L + log2 k vars, index ignored). */
int hg_instance_mle(hg_ctx* ctx, const void* instance, int which, int index, const uint64_t* point, size_t nvars, uint64_t out2[2]);
/* the same for the kernel of hg_verify_public_batch: the table (which / index as above) of n instances of one parameter set at ONE
 * shared point, as one work unit of that kernel with n members; out receives 2 words per instance. Device only. Returns 0, or -1
 * for a null argument or element, no context, or instances of mixed parameters. */
int hg_instance_mle_batch(hg_ctx* ctx, const void* const* instances, size_t n, int which, int index, const uint64_t* point,
                          size_t nvars, uint64_t* out);

/* ---- Polynomial commitment: what opens the claims hg_verify_public leaves ------------------------------------------------------
 * The reference names MultilinearBrakedown<F, Keccak256, BrakedownSpec6> as its Pcs type parameter
 * [REF sk_encryption_circuit.rs:543-550] and never calls it. This is that layer for Goldilocks: a multilinear
 * commitment of the Brakedown / Ligero shape with the reference's hash, Keccak-256. Two things differ from the type the reference
 * names: the linear code is Reed-Solomon of rate 1/4 (the NTT of the zero-padded row; Brakedown's argument needs a linear code, not
 * the expander code of BrakedownSpec6), and evaluation points are E = GoldilocksExt2 points. Not zero knowledge: an opening
 * reveals linear combinations and whole encoded columns of the tables. A proof of
 * hg_prove_committed_mode absorbs the root into the GKR transcript ahead of the first challenge ("Bound proofs" below); the other
 * provers do not.
 *
 * The scheme. Coordinate i of a point belongs to bit i of the table index (the convention of hg_mle_eval and hg_claims_settle).
 *   Rows.   Tables T_0 .. T_{m-1}, table t of 2^{v_t} canonical words. Row length C = 2^c (c = log2_row, c <= v_t for every t).
 *           Table t gives 2^{v_t - c} rows, row r = T_t[r C .. (r+1) C); the rows of all tables are stacked in table order, R rows
 *           in all; off_t = the first row of table t.
 *   Code.   Enc(row) = the forward NTT of size N = 4C of the row zero-padded to 4C words, natural order, root root_of_unity(c+2):
 *           what hg_ntt(.., log2n = c+2, inverse = 0, ..) computes. On an E vector Enc acts on the c0 and the c1 coordinates apart.
 *   Tree.   leaf_j = Keccak256(LE64(0) || LE64(M[0][j]) || .. || LE64(M[R-1][j])), j < 4C, M[r] = Enc(row_r); an inner node is
 *           Keccak256(LE64(1) || left || right); the commitment is the 32-byte root. Keccak-256 with the original padding.
 *   Opening of n claims (t_i, z_i in E^{v_{t_i}}, y_i) with Q = n_queries:
 *     1. an absorbing transcript (mode bit 1 above) whose hash state starts as the ASCII bytes "hg-pcs-1", the root, then as 4-byte
 *        little-endian c, m, v_0 .. v_{m-1}, Q, n, then per claim t_i (4-byte LE), the point's words and the value's two words (8-byte LE);
 *     2. rho = a squeezed E challenge; u_0[j] = sum_{r<R} rho^r row_r[j], j < C (the proximity combination);
 *     3. per claim w_i = eq(z_i[c..]) (2^{v_t - c} entries) and u_i[j] = sum_r w_i[r] row_{off_t + r}[j];
 *     4. u_0, u_1 .. u_n are written (big-endian, as every proof element) and absorbed;
 *     5. Q column indices j_q = (a squeezed base-field challenge) & (4C - 1), duplicates kept;
 *     6. per query the R column words M[.][j_q] (8-byte big-endian) and the c+2 siblings bottom-up (32 raw bytes each).
 *     Length: exactly 16 C (n+1) + Q (8 R + 32 (c+2)) bytes.
 *   Verification (hg_pcs_verify on the host, hg_pcs_verify_device on a context), in this order, the first failure is the reason in hg_last_error:
 *     1. the exact length ("pcs: the opening has .. bytes, .. expected");  2. every element and column word below p ("pcs:
 *     non-canonical word at byte ..");  3. <u_i, eq(z_i[..c])> == y_i, claims ascending ("pcs: evaluation mismatch at claim i");
 *     4. per query, ascending: leaf hash and path reach the root ("pcs: Merkle path mismatch at query q"), sum_r rho^r col[r] ==
 *     Enc(u_0)[j_q] ("pcs: proximity mismatch at query q"), per claim sum_r w_i[r] col[off_t + r] == Enc(u_i)[j_q] ("pcs: claim i
 *     inconsistent at query q").
 *   Parameters, plain arguments on every side (the verifier passes what it requires): n_queries = 0 means 241 =
 *     ceil(100 / log2(4/3)), the (3/4)^Q term of the unique-decoding analysis at rate 1/4 with proximity parameter d/3 - no more is
 *     claimed; at most 65536. log2_row = 0 means min(min_t v_t, ceil(log2(sum_t 2^{v_t}) / 2)); at most 24. m <= 64, v_t <= 30,
 *     n <= 4096.
 * Contracts: 0, 1 = rejected with the reason (the verifiers only), -1 with text in hg_last_error that names the function. The
 * commitment handle crosses as void*.
 *
 * hg_pcs_commit: the generic layer on caller tables (tables[t]: 2^{nvars[t]} host words). ctx == NULL: the host form; with a
 *   context the device form - rows staged and encoded in HBM by the batched NTT, one Keccak-f[1600] state per thread for the
 *   column hashes and for every tree node, one synchronisation; the handle then owns the raw and the encoded matrix in HBM (14 MB +
 *   57 MB for the secrets of n=32768 k=16 at c=11) and a host copy of the tree. Both forms give the same root. -1: a null argument
 *   or table, a shape outside the limits, log2_row above a table's variables, a word that is not below p, more than 65535 rows on
 *   the device.
 * hg_pcs_open: points = the claims' points one behind the other, 2 words per coordinate, nvars[table[i]] coordinates for claim i;
 *   values: 2 words per claim. ctx must be the context the commitment was made on (NULL for the host form). The device form runs
 *   the row combinations as one launch (weights built on the host, staged in one copy) and gathers the opened columns with
 *   another; the column indices depend on the u_i through the transcript, so it synchronises twice. Same bytes as the host form.
 *   n_claims == 0 is allowed: the proximity test alone. *len = the opening's length, also when cap is too small (-1). -1 also: a
 *   null argument, a table index out of range, a non-canonical coordinate or value, and - naming the claim - a value that is not
 *   <u_i, eq(z_i[..c])>: the prover holds u_i, so the check is free.
 * hg_pcs_verify: host only, no context. -1: a null argument, a shape or a count outside the limits, a table index out of range, a
 *   non-canonical coordinate or value.
 * hg_pcs_verify_device: hg_pcs_verify with the table-sized work on the context's stream; the decision and the reason are the host
 *   verifier's on every input, also where several checks fail at once (the order above decides). The opening is uploaded as it
 *   is; kernels byte-swap and range-check its words, check the evaluations, encode the u_i with the batched NTT, hash the opened
 *   columns and form their inner products while the host hashes the u_i into the transcript; the Q column indices follow on the
 *   same stream and a last kernel walks the paths and compares; three result words come back: one synchronisation. -1 as
 *   hg_pcs_verify (naming this function), for a null context (".. : no context"), and if the context's arena cannot hold the
 *   opening. It uses the context's arena like a prove: not concurrently with another call on the same context.
 * hg_secrets_commit: hg_pcs_commit of the five secret inputs of a witness handle, tables in input order s, e, k1, r1is[0] ..
 *   r1is[k-1], r2is: m = k+4, variables L, L, L, L x k, P + log2 k (L = log2 n + 1, P = log2 n).
 * hg_claims_open / hg_claims_verify: hg_pcs_open / hg_pcs_verify for an hg_input_claim array exactly as hg_verify_public* returns
 *   it (claims, n, points). Input ids map to tables 0, 1, 2 -> 0, 1, 2; 3+k+i -> 3+i; 3+2k -> 3+k; a claim on input 3 .. 3+k-1 (the
 *   public ais) or past 3+2k is an error (-1), so is a claim whose nvars is not its input's. The commitment is one hg_secrets_commit
 *   or hg_secrets_commit_batch made, or hg_secrets_commit_values / hg_prove_encryptions_committed. hg_verify_public followed by
 *   hg_claims_verify against a root the encryptor published is a verification that needs no secret. hg_claims_verify_device is
 *   hg_pcs_verify_device under the same mapping. */
int hg_pcs_commit(hg_ctx* ctx, const uint64_t* const* tables, const uint32_t* nvars, size_t n_tables, size_t log2_row, void** commitment,
                  uint8_t root[32]);
void hg_pcs_free(void* commitment);
int hg_pcs_open(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims,
                size_t n_queries, uint8_t* proof, size_t cap, size_t* len);
int hg_pcs_verify(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points,
                  const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len);
int hg_pcs_verify_device(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table,
                         const uint64_t* points, const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len);
int hg_secrets_commit(hg_ctx* ctx, const hg_params* params, const hg_witness* w, size_t log2_row, void** commitment, uint8_t root[32]);
int hg_claims_open(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points,
                   size_t n_queries, uint8_t* opening, size_t cap, size_t* len);
int hg_claims_verify(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points,
                     size_t n_queries, const uint8_t* opening, size_t len);
int hg_claims_verify_device(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n,
                            const uint64_t* points, size_t n_queries, const uint8_t* opening, size_t len);

/* ---- Folded openings: all claims reduced to one point by a sum-check ------------------------------------------------------------
 * An opening above carries one combined row u_i a claim. All claims of one proof are claims on tables of the same commitment, so the
 * usual multi-point batch opening of multilinear commitments applies: a sum-check over the committed tables reduces the n claims to
 * one value Y_t a table at the prefixes of a single point rho, and because those points share their low c coordinates the m values
 * are opened by ONE combined row. A folded opening carries two rows (proximity and combined) and 3 V + m field elements whatever n
 * is: 1 832 816 bytes against 3 338 912 for the 47 claims of n=32768 k=16, and the transcript hashes 64 KB of u instead of 1.5 MB.
 * A second set of entries with its own transcript tag; hg_pcs_open and its neighbours, their bytes and "hg-pcs-1" are unchanged.
 *
 * The scheme, in the notation of the section above; V = max_t v_t, n >= 1 claims (t_i, z_i, y_i), challenges are E elements.
 *   Transcript. Absorbing; its hash state starts as the 13 ASCII bytes "hg-pcs-fold-1" followed by exactly what "hg-pcs-1" appends
 *     after its tag: the root, c, m, v_0 .. v_{m-1}, Q, n (4-byte LE), per claim t_i, the point's words and the value's words. Every
 *     element written below is absorbed (its two words, 8-byte LE, c0 first) and appears in the opening big-endian.
 *   1. beta = a squeezed E challenge. S = sum_i beta^i y_i. For every table g_t(x) = sum_{i: t_i = t} beta^i eq(z_i, x) on v_t
 *      variables (zero for a table without a claim): sum_t sum_x g_t(x) T_t(x) = S.
 *   2. V rounds, the lowest variable first; folding by r is hg_fold's T'[j] = T[2j] + r (T[2j+1] - T[2j]). In round j the prover
 *      writes the coefficients c0, c1, c2 of s_j(X) = sum_t s_{j,t}(X), then r_j is squeezed. For v_t > j, s_{j,t}(X) = sum_{x'}
 *      g_t^(j)(X, x') T_t^(j)(X, x') over the tables folded by r_0 .. r_{j-1}. For v_t <= j, s_{j,t}(X) = K_t prod_{v_t <= j' < j}
 *      (1 - r_j') (1 - X) with K_t = g_t(rho[..v_t)) T_t(rho[..v_t)): a table that has run out of variables counts as extended by zero
 *      over the remaining ones. rho = (r_0 .. r_{V-1}).
 *   3. The prover writes Y_t = T_t(rho[0..v_t)), t = 0 .. m-1.
 *   4. delta, then rho' are squeezed. u_0[j] = sum_{r<R} rho'^r row_r[j]; u_1[j] = sum_t delta^t sum_{r < 2^{v_t-c}}
 *      eq(rho[c..v_t))[r] row_{off_t+r}[j]. u_0, then u_1 are written.
 *   5. Q column indices and 6. per query the R column words and the c+2 siblings, exactly as in "hg-pcs-1".
 *   Layout: a header of 16 (3 V + m) bytes - the round coefficients, then the Y_t - followed by a body that has exactly the layout of
 *     an "hg-pcs-1" opening with one claim: u_0, u_1, Q x (8 R + 32 (c+2)). Length: exactly 16 (3 V + m) + 32 C + Q (8 R + 32 (c+2)).
 *   Verification (hg_pcs_verify_folded on the host, hg_pcs_verify_folded_device on a context), in this order, the first failure is
 *     the reason:  1. the exact length ("pcs: the opening has .. bytes, .. expected", with the folded length);  2. every element and
 *     column word below p ("pcs: non-canonical word at byte ..", the lowest offset, counted from the start of the folded opening);
 *     3. for j ascending 2 c0 + c1 + c2 == claim_j, claim_0 = S, claim_{j+1} = s_j(r_j) ("pcs: fold round j does not match the
 *     running claim");  4. claim_V == sum_t Y_t g_t(rho[..v_t)) prod_{j >= v_t} (1 - rho_j), g_t evaluated from the claims in n V
 *     products ("pcs: fold final evaluation mismatch");  5. <u_1, eq(rho[..c))> == sum_t delta^t Y_t ("pcs: evaluation mismatch at
 *     claim 0");  6. per query, ascending: the Merkle path, proximity, then sum_t delta^t sum_r eq(rho[c..v_t))[r] col[off_t + r] ==
 *     Enc(u_1)[j_q] ("pcs: claim 0 inconsistent at query q"), the first two with the texts of hg_pcs_verify.
 *   Soundness is the beta and delta combinations plus the sum-check over E, on top of what the opening above claims; no more is
 *   claimed. Still not zero knowledge.
 * Contracts are those of the unfolded entries unless stated. The forms for a run are hg_pcs_open_folded_batch,
 * hg_claims_open_folded_batch, hg_pcs_verify_folded_device_batch and hg_claims_verify_folded_batch, below the single calls;
 * hg_prove_encryptions_committed does not fold. The forms over bn256::Fr are hg_pcs_open_folded_bn254 and its neighbours ("Folded
 * openings over BN254" below): single calls only.
 * hg_pcs_open_folded: hg_pcs_open's arguments. n_claims == 0 is -1 ("<function>: a folded opening needs a claim"; the proximity
 *   test alone is hg_pcs_open). *len = the length also when cap is too small. A value that is not its table's evaluation is refused
 *   with hg_pcs_open's text under this name, naming the lowest failing claim: the prover sees that round 0's s(0) + s(1) is not S
 *   and only then evaluates the claims one by one. A BN254 handle (open it with hg_pcs_open_folded_bn254) or a handle of another context is -1. The host form (ctx == NULL)
 *   is the byte reference. The device form builds g in HBM (16 bytes a table entry, 28 MB at n=32768 k=16) with one kernel from
 *   per-claim factor tables staged in one copy, then runs one launch a round on the context's stream with scratch from its arena:
 *   every live table pair is folded by the previous challenge and enters the round's sums in the same pass (round 0 reads the
 *   handle's raw rows, which are never written); the three sums come back once a round (one synchronisation a round), a table that
 *   has run out of variables continues as two scalars on the host, the Y_t come out of the last fold. u_0 and u_1 are two row
 *   combinations of R rows through hg_pcs_open's kernel, the columns through its gather. Profiler class pcs_fold. Not concurrently
 *   with another call on the same context.
 * hg_pcs_verify_folded: hg_pcs_verify's arguments and -1 cases, and n_claims == 0 as above. Host only.
 * hg_pcs_verify_folded_device: the same decision and reason on every input, also where several checks fail at once (a non-canonical
 *   column word together with a failing round reports the word). The header's checks are host scalar work; the body goes through
 *   the kernels of hg_pcs_verify_device as an opening of one claim that starts behind the header.
 * hg_claims_open_folded / hg_claims_verify_folded / hg_claims_verify_folded_device: the same under the mapping of hg_claims_open /
 *   hg_claims_verify, on an hg_input_claim array as hg_verify_public* returns it. */
int hg_pcs_open_folded(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points, const uint64_t* values, size_t n_claims,
                       size_t n_queries, uint8_t* proof, size_t cap, size_t* len);
int hg_pcs_verify_folded(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table, const uint64_t* points,
                         const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len);
int hg_pcs_verify_folded_device(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table,
                                const uint64_t* points, const uint64_t* values, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len);
int hg_claims_open_folded(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points,
                          size_t n_queries, uint8_t* opening, size_t cap, size_t* len);
int hg_claims_verify_folded(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n, const uint64_t* points,
                            size_t n_queries, const uint8_t* opening, size_t len);
int hg_claims_verify_folded_device(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n,
                                   const uint64_t* points, size_t n_queries, const uint8_t* opening, size_t len);

/* hg_pcs_open_folded_batch / hg_claims_open_folded_batch: hg_pcs_open_folded / hg_claims_open_folded for a run, with the argument lists
 *   and the outputs of hg_pcs_open_batch / hg_claims_open_batch (declared with the batch forms of commit and open, below). Item i opens
 *   its own claims, n_claims[i] >= 1, against commitments[i]; all handles are Goldilocks device handles of this context and of one
 *   shape, a handle may appear twice; one n_queries for the run. Opening i is byte for byte what hg_pcs_open_folded returns for that
 *   item alone - so also what the host form gives on a host commitment of the same tables. n == 0 returns 0 and writes nothing.
 *   status[i] = 0 opened; 1 REFUSED: lens[i] = 0, the item's buffer untouched, the reason slot holds exactly the text
 *   hg_pcs_open_folded (hg_claims_open_folded) leaves for that item, the single entry's name and the lowest failing claim. The run
 *   continues after a refusal and the other items' bytes are what they would be without the refused item. Returns the number of
 *   refused items.
 *   -1, nothing written, the text beginning with this function's name and giving "index i" where an item is at fault, every item
 *   checked before anything is enqueued: the cases of hg_pcs_open_batch, and an item without a claim ("<function>: index i: a folded
 *   opening needs a claim"); "<function>: no context" after the argument checks; cap_each below the folded length (the text gives the
 *   bytes needed).
 *   The pass: groups of at most 64 or "verify_batch_group" members within 2 GiB of scratch - a member takes its g (16 bytes a table
 *   entry), the two buffer pairs of the rounds (24 bytes a table entry), its staged claims and its image: about 71 MB at n=32768 k=16, 29
 *   members a group (a run of 64 ran as 3 groups: DESIGN.md 6). Per group the host threads start every
 *   member's transcript and write its claim rows and factor tables into one staged copy, one member a task; one launch builds all
 *   members' g and copies the words of one-word tables to the scalars; then every step of the reduction is ONE launch over all
 *   members (the member is the grid's third dimension; its raw rows through a table of G pointers, its challenge from an array of G
 *   elements that is uploaded once a round), one workgroup a member adds its partial sums, the 3 G sums and the scalars of the tables
 *   that retire come back in one copy each, and ONE synchronisation serves the group: V + 1 launches of the round kernels and V + 1
 *   synchronisations a group, whatever its size. The single call runs the same kernels as a group of one, with its row base and its
 *   challenge in the kernel arguments. A member whose running claim is not met is refused; it rides on in the launches, its results
 *   ignored (its buffers are its own). The lowest failing claim of the refused members comes from the combine and evaluation kernels
 *   of hg_pcs_open_batch over their claims, one cell a member; a refused member of which no claim fails is -1 (internal). u_0 and u_1
 *   are two jobs a member through the combine kernel, the u vectors come back, the host threads hash them and squeeze the indices,
 *   the gather writes the columns into images whose body starts behind the header; the host writes header, u vectors and siblings.
 *   Profiler class pcs_fold_batch; HG_TIMES=pcs prints a line a group; HG_DEBUG=plan prints "[hg plan] pcsfoldb members=.. V=..
 *   round_launches=.. round_syncs=.. tables=.. claims=.." a group. Not concurrently with another call on the same context.
 * hg_pcs_verify_folded_device_batch / hg_claims_verify_folded_batch: hg_pcs_verify_folded_device / hg_claims_verify_folded_device for a
 *   run, with the argument lists and the outputs of hg_pcs_verify_device_batch / hg_claims_verify_batch. results[i] and the reason are
 *   exactly what hg_pcs_verify_folded_device (so hg_pcs_verify_folded) gives for that item alone, also where several checks fail at
 *   once; byte offsets count from the start of the item's folded opening; a wrong length is rejected per item and never reaches the
 *   device. The order of reasons is the single call's: the length; a non-canonical header word (host); a non-canonical body word;
 *   the header's rounds and final evaluation; the body's checks. Returns the number of rejected items. -1 as
 *   hg_pcs_verify_device_batch, and in hg_pcs_verify_folded_device_batch an item with n_claims[i] == 0 ("<function>: index i: a folded
 *   opening needs a claim"). THE ONE EXCEPTION: hg_claims_verify_folded_batch gives an item with n_claims[i] == 0 - a proof the public
 *   batch verifier rejected - results[i] = 1 with the reason "hg_claims_verify_folded_batch: a folded opening needs a claim", so that a
 *   service can pass the arrays of hg_verify_public_batch through unchanged; such an item never reaches the device.
 *   The pass is hg_pcs_verify_device_batch's: per group the host threads run the header of every member (the claims' hash, the round
 *   checks, g_t from n V products) and write its block of the staged copy as that of an opening of one claim that starts behind the
 *   header - what hg_pcs_verify_folded_device writes for its one member; the index-free kernels run once over the group, the host
 *   threads hash each member's 2 C elements of u meanwhile, one copy of indices, the query kernel, the cells back: one synchronisation
 *   a group, the next group's openings gathered and copied meanwhile. A member whose header holds a word that is not canonical rides
 *   along on a block of zeros. No kernel of its own. Profiler class pcs_verify_batch. */
int hg_pcs_open_folded_batch(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points,
                             const uint64_t* const* values, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each,
                             size_t* lens, int* status, char* reasons, size_t reason_cap);
int hg_claims_open_folded_batch(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each,
                                const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings,
                                size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap);
int hg_pcs_verify_folded_device_batch(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row,
                                      const uint32_t* const* tables, const uint64_t* const* points, const uint64_t* const* values, const size_t* n_claims,
                                      size_t n_queries, const uint8_t* const* proofs, const size_t* lens, size_t n, int* results, char* reasons,
                                      size_t reason_cap);
int hg_claims_verify_folded_batch(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims,
                                  size_t claim_cap_each, const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries,
                                  const uint8_t* const* openings, const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap);

/* hg_pcs_verify_device_batch: hg_pcs_verify_device for a run of n openings of ONE shape (nvars, n_tables, log2_row) and one n_queries.
 *   Item i has its own root roots[i] (32 bytes), its own claims - n_claims[i] of them, 0 allowed; tables[i], points[i], values[i]
 *   laid out as hg_pcs_verify_device takes them, and may be NULL where n_claims[i] == 0 - and its opening proofs[i] of lens[i] bytes.
 *   results[i] = 0 accepted / 1 rejected; reasons may be NULL, else the slot at reasons + i*reason_cap receives the item's reason,
 *   NUL-terminated and cut to reason_cap bytes, "" where it is accepted. Decision and reason are exactly hg_pcs_verify_device's (so
 *   hg_pcs_verify's) for that item alone, also where several checks fail at once and for a wrong length, which is rejected per item
 *   and never reaches the device; byte offsets in reasons count from the item's own opening. Returns the number of rejected items;
 *   n == 0 returns 0 and writes nothing.
 *   The pass: the items whose length is right are cut into groups - at most 64 or the context option "verify_batch_group", a byte
 *   budget of 2 GiB (an item takes about 19 MB at n=32768 k=16), and the 65535 rows the batched NTT takes at once. Per group the
 *   host threads gather the openings into a page-locked set (copied on the context's upload stream) and write every member's
 *   transcript start, rho powers and eq weight tables into one staged copy; the kernels of hg_pcs_verify_device then run once over all
 *   members, driven by a member descriptor table - one workgroup per (member, claim), one thread per (member, query) and per (member,
 *   query, job), one batched NTT over all members' u rows - while the host threads hash each member's u_i into its transcript; one
 *   copy of all column indices, one query kernel, three result words a member: one synchronisation a group. The next group's
 *   openings are gathered and copied under the kernels of the current one.
 *   -1 (nothing is written; hg_last_error begins with the function's name and gives "index i" where an item is at fault; every
 *   item's arguments are checked before anything is enqueued): a null argument or null element, a shape, log2_row or n_queries
 *   outside the limits of hg_pcs_verify, n_claims[i] above 4096, a table index out of range, a non-canonical coordinate or value, a
 *   null context ("hg_pcs_verify_device_batch: no context"), a group the context's arena cannot hold. It uses the context's arena
 *   and batch buffers: not concurrently with another call on the same context.
 * hg_claims_verify_batch: the same pass under the mapping of hg_claims_verify_device (input ids to tables, the shape from params),
 *   on the claim and point arrays exactly as hg_verify_public_batch writes them: item i's claims at (hg_input_claim*)claims +
 *   i*claim_cap_each, its points at points + 2*i*coord_cap_each with point_off relative to its own block, its count n_claims[i]. An
 *   item with n_claims[i] == 0 (a proof hg_verify_public_batch rejected, say) is verified as the single call verifies zero claims:
 *   the proximity test, with its length rule. -1 also, naming the index: a claim on a public input or on an input past 3+2k, a
 *   wrong nvars, a count above claim_cap_each, a point outside the item's block. */
int hg_pcs_verify_device_batch(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row,
                               const uint32_t* const* tables, const uint64_t* const* points, const uint64_t* const* values,
                               const size_t* n_claims, size_t n_queries, const uint8_t* const* proofs, const size_t* lens, size_t n,
                               int* results, char* reasons, size_t reason_cap);
int hg_claims_verify_batch(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims,
                           size_t claim_cap_each, const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries,
                           const uint8_t* const* openings, const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap);

/* hg_pcs_commit_batch: hg_pcs_commit on a context for a run of n members of ONE shape (nvars, n_tables, log2_row); tables[i][t] = table
 *   t of member i. Member i receives the handle commitments[i] and its root at roots + 32 i. Each handle is what hg_pcs_commit on the
 *   same context returns for that member - the same root, the same host copy of the tree, the raw and the encoded matrix in HBM - and
 *   hg_pcs_open, hg_claims_open, hg_pcs_open_batch and hg_pcs_free take it. Device only. Returns 0; n == 0 returns 0 and writes nothing.
 *   The pass: the members are cut into groups - at most 64 or the context option "verify_batch_group", a byte budget of 2 GiB (a
 *   member takes 128 MB at n=32768 k=16: its rows, its encoded rows and the NTT scratch), and the 65535 rows the batched NTT takes at
 *   once. A group's rows and encoded rows live in ONE allocation (member stride R C and R N words); the tables are uploaded straight
 *   into it; staging with the range check (one flag a member), one batched NTT over all G R rows, the column hashes (one thread per
 *   member and column), the tree levels (one thread per member and node, the levels of at most 256 nodes in one workgroup a member)
 *   each run as one launch over the group; one download fetches all trees and flags: one synchronisation a group. A member's handle
 *   points into the group's allocation and shares its ownership: THE MEMORY RETURNS WHEN THE LAST HANDLE OF THE GROUP IS FREED.
 *   -1 (nothing is written and no handle survives; hg_last_error begins with the function's name and gives "index i" where a member
 *   is at fault): a null argument or null element, a shape outside the limits of hg_pcs_commit, more than 65535 rows in a member, a
 *   word that is not below p (the lowest such member is named), a null context ("hg_pcs_commit_batch: no context", reported after the
 *   argument checks), a group the arena cannot hold. It uses the context's arena like a prove: not concurrently with another call
 *   on the same context.
 * hg_secrets_commit_batch: the same pass on the five secret inputs of the witness handles ws[0 .. n-1] (tables as hg_secrets_commit
 *   orders them). -1 also, naming the index: a witness built for other parameters.
 * hg_pcs_open_batch: hg_pcs_open for a run of n items with one n_queries. Item i opens its own claims (n_claims[i] of them, 0 allowed;
 *   tables[i], points[i], values[i] as hg_pcs_open takes them, NULL allowed where n_claims[i] == 0) against commitments[i]. Every
 *   handle is a Goldilocks device handle of this context and all have one shape; a handle may appear more than once. Opening i is
 *   written at openings + i*cap_each and its length to lens[i]: byte for byte what hg_pcs_open gives for that item alone (and what
 *   the host form gives on a host commitment of the same tables). status[i] = 0 opened; 1 REFUSED - a value is not the evaluation of
 *   its table at the point: lens[i] = 0, the item's buffer is untouched, and the slot at reasons + i*reason_cap holds the text
 *   hg_pcs_open leaves in hg_last_error for that item (the lowest failing claim), NUL-terminated and cut to reason_cap; "" where the
 *   item is opened; reasons may be NULL. The run continues, the other items are what they are without the refused one. Returns the
 *   number of refused items; n == 0 returns 0 and writes nothing.
 *   The pass, per group (at most 64 or "verify_batch_group" items, the 2 GiB budget): the host threads write every member's
 *   transcript start, rho powers, weight tables eq(z[c..]) and the job, claim and member tables into one staged copy; the row
 *   combinations run as one launch driven by the job table, a second checks <u_i, eq(z_i[..c])> == y_i per (member, claim) with one
 *   cell a member for its lowest failing claim, a third writes the u vectors big-endian into the members' opening images; the u
 *   vectors and the cells come back into page-locked memory (first synchronisation); the host threads absorb each member's u_i and
 *   squeeze its indices, one member a thread; one copy uploads all indices, a gather writes the opened columns big-endian into the
 *   images of the members that were not refused, the images come back (second synchronisation); the host copies the siblings from
 *   each handle's tree. Two synchronisations a group, as hg_pcs_open has per item.
 *   -1 (nothing is written; hg_last_error begins with the function's name and gives "index i" where an item is at fault; every item
 *   is checked before anything is enqueued): a null argument or element, a host-form handle, a BN254 handle, a handle of another
 *   context, handles of different shapes, a table index out of range, a non-canonical coordinate or value, more than 4096 claims,
 *   n_queries above the limit, cap_each below the largest opening of the run (the text gives the bytes needed), a null context
 *   ("hg_pcs_open_batch: no context", after the argument checks), a group the arena cannot hold. It uses the context's arena and
 *   batch buffers: not concurrently with another call on the same context.
 * hg_claims_open_batch: the same pass under the mapping of hg_claims_open, on the claim and point arrays exactly as
 *   hg_verify_public_batch writes them (item i's claims at (hg_input_claim*)claims + i*claim_cap_each, its points at points +
 *   2*i*coord_cap_each with point_off relative to its own block, its count n_claims[i]); a refused item's text is hg_claims_open's.
 *   -1 also, naming the index: the mapping errors of hg_claims_verify_batch and a commitment that is not hg_secrets_commit's for
 *   these parameters. The BN254 forms of these four entries are declared with the other _bn254 entries of the commitment, below. */
int hg_pcs_commit_batch(hg_ctx* ctx, const uint64_t* const* const* tables, const uint32_t* nvars, size_t n_tables, size_t log2_row, size_t n,
                        void** commitments, uint8_t* roots);
int hg_secrets_commit_batch(hg_ctx* ctx, const hg_params* params, const hg_witness* const* ws, size_t n, size_t log2_row, void** commitments,
                            uint8_t* roots);
int hg_pcs_open_batch(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points,
                      const uint64_t* const* values, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each,
                      size_t* lens, int* status, char* reasons, size_t reason_cap);
int hg_claims_open_batch(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each,
                         const uint64_t* points, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings,
                         size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap);

/* hg_secrets_commit_values: hg_secrets_commit on a context, taken from where the tables lie in HBM: inputs 0, 1, 2, 3+k .. 3+2k-1 and
 *   3+2k of v (s, e, k1, r1is[i], r2is), an hg_values of hg_witness_gen / hg_witness_gen_into / hg_witness_derive_into for this key on
 *   this context. The handle is a Goldilocks device handle of ctx (hg_claims_open, hg_claims_open_batch, hg_pcs_open, hg_pcs_open_batch
 *   and hg_pcs_free take it); its root and every opening made from it are byte for byte those of the host form of hg_secrets_commit on
 *   the witness whose tables v holds. The handle owns copies of the rows: v may be refilled or freed afterwards.
 *   One kernel reads every word of the k+4 tables once (16 bytes a thread where a row has two words or more) and writes it into the
 *   handle's raw rows and into the zero-padded rows of the matrix to encode, with the padding and the range check; the batched NTT,
 *   the column hashes and the tree follow as in hg_pcs_commit: nothing crosses the bus but the tree. The context's stream, its arena
 *   for the scratch, one synchronisation: not concurrently with another call on the same context. Profiler class pcs_commit_values.
 *   *commitment = NULL first. -1, hg_last_error beginning with the function's name, in this order: a null argument (pk, v,
 *   commitment, root); a null context (".. : no context"); a host-only key; values of another key or of another context; a rank's
 *   share of hg_witness_gen_shard, in which a secret input is not resident (the input is named); a log2_row outside the limits of
 *   hg_pcs_commit or above the smallest table; more than 65535 rows; a word that is not below p.
 * hg_prove_encryptions_committed: hg_prove_encryptions that also commits to every item's secret inputs, inside the pipeline.
 *   Everything hg_prove_encryptions does and returns, with its checks in its order under this function's name (a refusal's text reads
 *   "hg_prove_encryptions_committed: encryption i: .."); proof i is byte-identical to hg_prove_encryptions's. commitments and roots
 *   are required when n_enc > 0: commitments[i] is what hg_secrets_commit_values(.., log2_row, ..) gives for item i's tables, the 32
 *   bytes at roots + 32 i are its root. A refused item gets commitments[i] = NULL and 32 zero bytes. ws may be NULL, and the entry is
 *   made to be called that way: the seven tables then never visit the host.
 *   The commit of item i is enqueued on the third stream behind the item's derivation and evaluation, so it runs under the prove of
 *   the item before (and of item i) and does not delay the event that prove i waits for; its tree comes back on the copy stream
 *   into page-locked staging and enters the handle once prove i has completed. The NTT scratch, the twiddles and the tree buffers
 *   belong to the pipeline, not to the arena. The raw and encoded rows of the items lie in group allocations - at most 64 items or
 *   the 2 GiB budget of hg_pcs_commit_batch, allocated when a group's first item is filled - that the group's handles share: THE
 *   MEMORY RETURNS WHEN THE LAST HANDLE OF THE GROUP IS FREED. The commit is outside the launch graph of a table set: the walked,
 *   recording and replayed schedules and option "graph" = 0 give the same handles.
 *   All commitments[i] are NULL at entry, as ws[i]. Returns the number of refused encryptions (n_enc == 0 returns 0) or -1, after
 *   which no handle is alive: the errors of hg_prove_encryptions (commitments and roots count among the null arguments); then, ahead
 *   of anything enqueued, the log2_row errors of hg_secrets_commit_values and more than 65535 rows; a derived table holding a word
 *   that is not below p (".. encryption i: a derived table holds a word that is not below p"), which a correct derivation never gives.
 *   timings: the fields of hg_prove_encryptions; witness_ms includes the commits' device time; upload_ms = the sum over the proven
 *   items of the commit's device time alone (HIP events on the stream it runs on). Goldilocks, mode 0. */
int hg_secrets_commit_values(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, size_t log2_row, void** commitment, uint8_t root[32]);
int hg_prove_encryptions_committed(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                                   const int64_t* const* a, size_t n_enc, size_t log2_row, uint8_t* proofs, size_t cap_each, size_t* lens,
                                   int* status, void** commitments, uint8_t* roots, hg_witness** ws, char* reasons, size_t reason_cap,
                                   hg_timings* timings);

/* The same pair in a protocol mode that FIXES the reference's two known soundness gaps. mode bits:
 *   1  absorbing transcript: write_felt / read_felt also hash the element - the rule of the in-tree plonkish-trait writer of
 *      the same struct [REF bfv-gkr/src/transcript.rs:205-208, 224-233]; the gkr-trait writer the prover uses does not
 *      [REF :146-157, 180-196], which leaves every challenge independent of the proof;
 *   2  extension-field memory checking: gamma, tau are used as E elements, not truncated to base limb 0
 *      [REF lasso/src/memory_checking/prover.rs:36-39; README.md:108 "Known issues"].
 * mode 0 = hg_prove / hg_verify (the reference as it is, bit-exact). Other modes are Goldilocks only and run the round-by-round
 * prover: the device hands every round's sums to the host transcript through a pinned mailbox and spins on the challenge (no
 * stream synchronisation inside a sum-check); timings->sync_ms then holds the NUMBER of stream synchronisations and
 * timings->enqueue_ms the number of mailbox round trips. HG_SEQ_NO_MAIL=1 restores one synchronisation per round. */
int hg_prove_mode(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int mode, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings);
int hg_prove_resident_mode(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int mode, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings);
int hg_verify_mode(const hg_pk* pk, const hg_witness* w, int mode, const uint8_t* proof, size_t len);

/* ---- Bound proofs: the GKR transcript starts from the statement -----------------------------------------------------------------
 * With the absorbing transcript (mode bit 1) the challenges depend on the proof bytes. In a BOUND proof they also depend on what the
 * proof is about and on what its claims are opened against: the transcript's hash state starts, instead of empty, as
 *     "hg-gkr-bound-1" (14 ASCII bytes) || LE32(n) || LE32(k) || LE64(qis[0]) .. LE64(qis[k-1]) || LE32(mode) || digest || root
 * (hg_bound_seed), digest = the statement digest of the public instance below, root = the 32-byte root of the commitment to the five
 * secret inputs (hg_secrets_commit*). Nothing else changes: a bound transcript is the absorbing transcript with that start, on the
 * prover's side and on the verifier's. mode is 1 or 3; for mode 0 or 2 every entry of this section returns -1 with the text
 * "<function>: binding needs the absorbing transcript (mode bit 1)" (a mode outside 0..3: "<function>: unknown mode bits").
 * Goldilocks; hg_verify_public_bound_batch verifies a run of bound proofs in one pass. Still open: BN254 has no protocol modes and
 * stays unbound; the hg_prove_encryptions_committed pipeline is mode 0 and stays unbound; the sharded prover is unbound; nothing here
 * is zero knowledge.
 *
 * The statement digest. The instance is read as 2 k n signed 64-bit words, two's complement, little-endian: the k n words of a, then
 *   those of ct0, each modulus-major in ascending degree (what hg_instance_from_ciphertext takes). Leaf width B = min(128, 2 k n)
 *   words; leaf_j = Keccak256(LE64(2) || words[j B .. (j+1) B)), j < 2 k n / B; an inner node is the commitment's,
 *   Keccak256(LE64(1) || left || right); the digest is the root of the (full binary) tree, with one leaf that leaf. Keccak-256 with
 *   the original padding. The prefix 2 keeps these leaves apart from the commitment's leaves (prefix 0) and nodes (prefix 1).
 * hg_instance_digest: ctx == NULL: the host tree, the leaves dealt to the host threads. With a context: the instance is uploaded as
 *   it is and hashed by one kernel, one thread per leaf with the Keccak-f[1600] state in registers, the levels above by the tree
 *   kernels of the commitment; one synchronisation. Same 32 bytes. -1: a null argument.
 * hg_instance_digest_batch: device only; the n instances (one parameter set) go through ONE launch of that kernel as n members; out
 *   receives 32 bytes an instance. n == 0 returns 0. -1: a null argument or element, no context, instances of mixed parameters.
 * hg_values_instance_digest: device only; the same 32 bytes from the resident tables of a full hg_values of this key and context (the
 *   laid-out read: coefficient j of a_i is word n-1-j of input 3+i, of ct0_i word 2n-2-j of block i of ct0is; a field word w stands
 *   for w if w <= (p-1)/2, else for -(p-w)). Padding words are not read. -1, in this order: a null argument; no context; a host-only
 *   key; values of another key or context; a rank's share of hg_witness_gen_shard, in which an input (or ct0is) is not resident; a
 *   word that is not a signed value in [-(q_i-1)/2, (q_i-1)/2].
 * hg_bound_seed: the byte string above into out (90 + 8 k bytes); *len = its length, also when cap is too small (-1). -1 also:
 *   a null argument, the mode rule, parameters hg_setup would not take.
 * hg_prove_committed_mode: on a full resident hg_values - of hg_witness_gen, hg_witness_gen_into or hg_witness_derive_into -, in one call:
 *   the commitment of hg_secrets_commit_values(ctx, pk, v, log2_row, ..) - handle and root byte for byte that call's; hg_claims_open
 *   takes the handle -, the statement digest from the same resident tables (the digest kernel on the context's second stream, beside
 *   the commit's kernels and waited for together with them), the seed, and the round-by-round prover of hg_prove_resident_mode on
 *   the seeded transcript. No table crosses the bus: only the commitment's tree and the 32 digest bytes come back. -1, in this
 *   order, after which no handle is alive (*commitment = NULL): the mode rule; the errors of hg_secrets_commit_values under this
 *   function's name; a null proof or len; the errors of hg_prove_resident_mode; a proof buffer that is too small (*len = the need).
 *   timings: the fields of hg_prove_resident_mode, upload_ms = the commit and the digest (host clock).
 * hg_verify_public_bound / hg_verify_public_bound_device: hg_verify_public / hg_verify_public_device for a bound proof, with the
 *   root the encryptor published as one more argument. The host form computes the digest with the host tree; the device form with
 *   the kernel, from the instance words it uploads anyway, and waits for the 32 bytes ahead of the walk's first squeeze (one
 *   synchronisation more than the unbound form). Decisions, claims, points and reasons are otherwise those of the unbound entries; -1
 *   also for a null root and by the mode rule. A proof made for another root, another instance or another mode, and an unbound
 *   proof, are rejected: their challenges differ from the first one on. hg_verify_public_bound followed by hg_claims_verify against
 *   the same root is a verification that needs no secret in which neither the commitment nor the ciphertext can be chosen after the
 *   challenges.
 * hg_verify_public_bound_batch: hg_verify_public_bound_device for a run of n pairs under one key: proof i (proofs[i], lens[i]) is
 *   checked against instances[i], roots[i] (32 bytes; the array hg_claims_verify_batch takes) and `mode` (1 or 3). Goldilocks, device
 *   only. results, reasons, claims, points and n_claims follow hg_verify_public_batch in layout and meaning; for every pair the
 *   decision, the reason text, the claims and the points are bit for bit those of hg_verify_public_bound_device on that pair alone
 *   (and so those of hg_verify_public_bound). digests (may be NULL): 32 bytes an item, the statement digest of instances[i] as the
 *   device computed it - for accepted and rejected items alike, it depends on the instance only. Returns the number of rejected
 *   proofs; n == 0 returns 0 and writes nothing; -1, after which nothing is written and hg_last_error begins with the function's
 *   name (and gives "index i" where an item is at fault): everything hg_verify_public_batch returns -1 for, a null roots or
 *   roots[i], and - checked first - the mode rule above.
 *   The pass is hg_verify_public_batch's with the digests ordered in. A group's instances are staged in slices (context option
 *   "bound_batch_slice"): the host threads gather a slice, its copy goes on the upload stream, one kernel behind it hashes the
 *   slice's members out of the staged set - one workgroup of 64 threads per (member, 64 leaves), a thread a leaf with the state in
 *   registers, the workgroup's leaves folded to one node in LDS; members of more than 64 leaves finish with the commitment's tree
 *   kernels over those nodes - and the 32-byte roots come back into a page-locked block of the batch; all of it in the batch's own
 *   buffers, without the context's arena or staging buffer. The walks of a group wait for its digests (one event a group, under the
 *   kernels of the group before), build each item's seed and go on as the unbound pass does.
 * hg_instance_digest_group: part exposed for parity tests: the digests of n instances of one parameter set computed exactly as
 *   hg_verify_public_bound_batch computes them - gathered into the batch's page-locked sets in slices, copied on the upload stream,
 *   hashed by that kernel out of the staged set. out receives 32 bytes an instance: hg_instance_digest's. The contract of
 *   hg_instance_digest_batch: device only, n == 0 returns 0, -1 for a null argument or element, no context, mixed parameters. */
int hg_instance_digest(hg_ctx* ctx, const void* instance, uint8_t out32[32]);
int hg_instance_digest_batch(hg_ctx* ctx, const void* const* instances, size_t n, uint8_t* out);
int hg_instance_digest_group(hg_ctx* ctx, const void* const* instances, size_t n, uint8_t* out);
int hg_values_instance_digest(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, uint8_t out32[32]);
int hg_bound_seed(const hg_params* params, int mode, const uint8_t digest32[32], const uint8_t root32[32], uint8_t* out, size_t cap, size_t* len);
int hg_prove_committed_mode(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int mode, size_t log2_row, uint8_t* proof, size_t cap, size_t* len,
                            void** commitment, uint8_t root[32], hg_timings* timings);
int hg_verify_public_bound(const hg_pk* pk, const void* instance, int mode, const uint8_t root[32], const uint8_t* proof, size_t len, void* claims,
                           size_t claim_cap, uint64_t* points, size_t coord_cap, size_t* n_claims);
int hg_verify_public_bound_device(hg_ctx* ctx, const hg_pk* pk, const void* instance, int mode, const uint8_t root[32], const uint8_t* proof, size_t len,
                                  void* claims, size_t claim_cap, uint64_t* points, size_t coord_cap, size_t* n_claims);
int hg_verify_public_bound_batch(hg_ctx* ctx, const hg_pk* pk, const void* const* instances, const uint8_t* const* roots,
                                 const uint8_t* const* proofs, const size_t* lens, size_t n, int mode, int* results,
                                 void* claims, size_t claim_cap_each, uint64_t* points, size_t coord_cap_each,
                                 size_t* n_claims, uint8_t* digests, char* reasons, size_t reason_cap);

/* The round-by-round prover (modes 1-3) on several ranks, with ONE all-reduce per sum-check round: the exchange pattern an absorbing
 * transcript leaves [REF bfv-gkr/src/transcript.rs:205-208, 224-233: every round's message is hashed before the next challenge is
 * squeezed], SURVEY 8(e)'s conservative form of the north_star partition. Every rank holds the whole witness (hg_witness_gen) and runs
 * the whole protocol; inside every round kernel rank r evaluates the hypercube sums of the tiles t = r (mod world) only - the
 * prove_sum_check work of [REF lasso/src/lasso.rs:278-279; memory_checking/prover.rs:242-252] split along the hypercube - and folds
 * everything; the group adds the ranks' partial sums (at most six canonical Goldilocks words, lane-wise mod p), after which every
 * rank's transcript absorbs the same message and squeezes the same challenge. Rounds finished on the host and the scalar steps between
 * sum-checks are replicated. Every rank returns the same proof, byte for byte the one hg_prove_resident_mode gives.
 *   hg_group_local(world)    ranks are threads of this process, one context each (any devices): barrier + modular sum in memory;
 *   hg_group_external(fn, user, world)   fn = int (*)(void* user, uint64_t* words, size_t n): adds `words` over the ranks in place
 *                            (e.g. an all-gather over torch.distributed / MPI followed by the modular sum) and returns 0.
 * In this form a round kernel is launched only after the challenge of the round before has been posted (the single-rank prover
 * launches ahead and lets the kernel wait on the device): no kernel ever waits for the host, so ranks may share a device or a
 * hardware queue (ranks as threads of one process in the tests) without waiting for each other's waiting kernels.
 * timings->replay_ms holds the number of all-reduces of the proof. Mode 0 shards through hg_prove_sharded (one all-reduce per proof).
 * WITHOUT replicating the witness (round 6): when `v` is a rank's share (hg_witness_gen_shard: the Lasso node's input and the inputs of
 * the node reductions the rank owns, chains dealt by CRT modulus as in mode 0), a Vanilla / FFT node's reduction runs on its owner
 * alone - every tile of its round kernels, the rounds finished on the host - and the other ranks launch nothing for it: they join the
 * same all-reduces with zeros (one per device round; one of up to 144 words for the rounds the owner's host finished; one for the final
 * evaluations), absorb the same messages and squeeze the same challenges. The Lasso node keeps the tile-split form. Same proof bytes. */
hg_group* hg_group_local(int world);
hg_group* hg_group_external(void* reduce_fn, void* user, int world);
void hg_group_free(hg_group* g);
int hg_prove_resident_mode_sharded(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int mode, int rank, hg_group* group, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings);

/* The two halves of hg_prove, split where the reference splits its spans:
 *   hg_witness_gen   = "wintess gen": circuit.evaluate(inputs) [REF sk_encryption_circuit.rs:439-442] ON THE DEVICE: the
 *                      3+2k+1 input tables are uploaded, the 2k+1 size-2^L NTTs (FFT -> pointwise mul -> IFFT) and
 *                      the Vanilla gate maps run as HIP kernels; every node table stays resident in HBM;
 *   hg_prove_resident = "eval output" + "GKR prove" [REF sk_encryption_circuit.rs:444-457] on resident tables.
 * bench.py times hg_prove_resident (inputs already in HBM when the timed region starts). */
int hg_witness_gen(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, hg_values** out, hg_timings* timings);
/* The same into an EXISTING values object (of the same key and context): no allocation, every table keeps its address. This is the
 * steady state of a prover that receives a new witness per proof, as the reference's caller does [REF bfv-gkr/src/test.rs:37-38]: the
 * launch graph the library recorded for `v` (hg_set_option "graph") stays valid, because the launch sequence of a prove depends on
 * addresses only - the next hg_prove_resident(v) replays it on the new witness. hg_prove does this internally with a values
 * object owned by the context. */
int hg_witness_gen_into(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, hg_values* v, hg_timings* timings);
/* hg_witness_derive and hg_witness_gen_into in one: the steady state of a proving service that receives encryptions, not witnesses
 * [REF scripts/circuit_sk.py:18-140 followed by sk_encryption_circuit.rs:439-442]. s, e, k1, ais are uploaded into the input tables
 * of `v` (a full values object of this key and context, from hg_witness_gen), the derivation kernels write r1is, r2is and ct0is
 * straight into its tables - they do not visit the host on the way to the prover - and the circuit is evaluated behind them on the
 * same stream. `v` keeps its addresses, so the launch graph recorded for it proves the new witness. *w (w may be NULL) receives
 * the host handle the verifiers need for ct0is; its copy back runs beside the evaluation. timings (may be NULL): total_ms =
 * witness_ms = wall clock of the call, gpu_ms = HIP events around uploads, derivation and evaluation on the prover stream.
 * Errors as hg_witness_derive, plus a host-only key or a rank's share as `v`; after a failed check (-1) no handle is produced and the
 * CONTENTS of `v` are clobbered (it stays valid for the next hg_witness_gen_into / hg_witness_derive_into). */
int hg_witness_derive_into(hg_ctx* ctx, const hg_pk* pk, const uint64_t* s, const uint64_t* e, const uint64_t* k1,
                           const uint64_t* ais, hg_values* v, hg_witness** w, hg_timings* timings);
/* The same for ONE rank of a proof sharded over `world` GPUs (BASELINE config 4): only the node tables the rank's share reads stay
 * resident - the Lasso node's input, the inputs of the Vanilla / FFT node reductions the planner deals to it, ct0is on the rank that
 * evaluates the output claim; the per-modulus objects a rank does not own [REF sk_encryption_circuit.rs:122-128, 245-260] are released.
 * Only the cone of those tables is ever evaluated (the per-modulus chains of the moduli the rank owns, not the whole circuit), into
 * subset tables the object keeps, so hg_witness_gen_into refills it without allocating (hg_values_peak_bytes: tables + cone).
 * The result proves through hg_prove_sharded / hg_prove_shard_begin with the same (rank, world) only. */
int hg_witness_gen_shard(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int rank, int world, hg_values** out, hg_timings* timings);
/* [resident bytes, bytes of the full set of node tables, resident tables, tables] */
int hg_values_info(const hg_values* v, uint64_t out[4]);
/* Device bytes the object holds in all: its resident tables plus, for a rank's share (hg_witness_gen_shard), the subset tables its
 * refills evaluate into - the cone of nodes the resident tables are computed from, never the whole circuit. -1 for a null handle. */
int64_t hg_values_peak_bytes(const hg_values* v);
void hg_values_free(hg_values* v);
/* copies node `node`'s table (NodeId order of configure) back to the host; returns its element count */
int64_t hg_values_get(hg_ctx* ctx, const hg_values* v, int node, uint64_t* out, size_t cap);
int hg_prove_resident(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, uint8_t* proof, size_t cap, size_t* len,
                      hg_timings* timings);

/* ONE proof sharded over `world` GPUs (one process per GPU, same witness resident on each). Every rank walks the whole
 * protocol but runs only the device jobs it owns; the largest part, grand product #1 of the Lasso node, is split by
 * memory (batch item), so its round sums are PARTIAL sums on every rank. `*partial` (pinned host memory owned by the
 * context, *n_u64 lanes of canonical field elements) holds this rank's share of the scalar results, zeros elsewhere.
 * The caller all-gathers the ranks' buffers (RCCL) and hands them to hg_prove_shard_combine, which installs their
 * lane-wise sum mod p; hg_prove_shard_finish then replays the transcript — every rank obtains the identical bytes.
 * One all-gather per proof is the only exchange. world == 1 degenerates to hg_prove_resident. */
int hg_prove_shard_begin(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, int rank, int world, uint64_t** partial,
                         size_t* n_u64);
int hg_prove_shard_combine(hg_ctx* ctx, const uint64_t* gathered /* world x n_u64, rank-major */, int world, size_t n_u64);
int hg_prove_shard_finish(hg_ctx* ctx, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings);
/* the arithmetic of hg_prove_shard_combine alone, host only (no context, no device): out[i] = sum over ranks of gathered[r][i] mod p;
 * non-canonical lanes are an error. What a caller-side exchange (any byte transport) computes between _begin and _finish. */
int hg_shard_combine_host(const uint64_t* gathered /* world x n_u64, rank-major */, int world, size_t n_u64, uint64_t* out);

/* The same with the exchange INSIDE the library: one process per GPU, each with its own context and a copy of the resident
 * witness; one RCCL all-reduce per proof (each 64-bit lane as two 32-bit halves in 64-bit lanes, ncclSum, folded back mod p on
 * the device; no host staging), enqueued on the prover stream behind the rank's last kernel. Nothing in the reference
 * corresponds (single-process rayon); BASELINE config 4.
 *   hg_comm_unique_id: rank 0 obtains the 128-byte RCCL id and hands it to the other ranks out of band (any byte channel);
 *   hg_comm_init:      collective over all `world` ranks (ncclCommInitRank); world == 1 is allowed (single-rank communicator);
 *   hg_prove_sharded:  collective; every rank returns the identical proof bytes. */
int hg_comm_unique_id(uint8_t out[128]);
int hg_comm_init(hg_ctx* ctx, const uint8_t id[128], int rank, int world);
int hg_comm_destroy(hg_ctx* ctx);
/* number of ranks of the context's communicator as RCCL reports it (ncclCommCount); 0 without a communicator */
int hg_comm_count(hg_ctx* ctx, int* ranks);
/* The arithmetic of the exchange without a communicator (a one-GPU box cannot form one of more than one rank): `world` rank
 * buffers of n_u64 canonical lanes (host, rank-major) are split into 32-bit halves on the device, added lane-wise as plain 64-bit
 * integers - what ncclAllReduce(ncclUint64, ncclSum) does - and folded back mod p; out[n_u64] = lane-wise sum mod p. */
int hg_comm_selftest(hg_ctx* ctx, const uint64_t* rank_buffers, int world, size_t n_u64, uint64_t* out);
int hg_prove_sharded(hg_ctx* ctx, const hg_pk* pk, const hg_values* v, uint8_t* proof, size_t cap, size_t* len, hg_timings* timings);

/* = circuit.evaluate (host part of witness generation) [REF sk_encryption_circuit.rs:442]:
 *   copies out the Lasso node's input table (2^nu) and the `sum` node output (k*2^L). Host only. */
int hg_circuit_eval(const hg_pk* pk, const hg_witness* w, uint64_t* lasso_in, size_t lasso_cap, uint64_t* sum_out,
                    size_t sum_cap);

/* = <LassoNode as gkr::circuit::node::Node>::prove_claim_reduction [REF lasso/src/lasso.rs:57-114] on a fresh
 *   transcript. lasso_in: host table of 2^nu field elements. claim_out: nu E coordinates then the value. */
int hg_lasso_prove(hg_ctx* ctx, const hg_pk* pk, const uint64_t* lasso_in, uint8_t* proof, size_t cap, size_t* len,
                   uint64_t* claim_out);
/* The same, entered inside a larger transcript: `chain_skip` E challenges have already been squeezed by the caller
 * (what a Rust `impl Node` shim passes: the position of its `&mut dyn TranscriptWrite` in the challenge chain). */
/* Launch plan: the node runs as it does inside hg_prove - the fork recorded ahead of it, counters, grand product #2's tree and the
 * openings on the side streams, the small grand-product rounds split, every side stream joined before the results are read. With
 * hg_set_option(ctx, "one_stream", 1) it runs the unforked plan, every launch on the main stream. The bytes are the same. */
int hg_lasso_prove_at(hg_ctx* ctx, const hg_pk* pk, const uint64_t* lasso_in, size_t chain_skip, uint8_t* proof, size_t cap,
                      size_t* len, uint64_t* claim_out);

/* Number of E challenges the Lasso node squeezes (nu for r, nu collation rounds, gamma / tau, both grand products:
 * SURVEY.md appendix C). A caller that replays the node's bytes into its own transcript (the Rust `impl Node` shim)
 * advances its challenge position by this much. */
int hg_lasso_num_challenges(const hg_pk* pk, size_t* n_e);

/* = gkr::sum_check::prove_sum_check [REF call sites lasso.rs:278-279, prover.rs:242-252] on caller tables.
 *   kind: 0 collation g = p0*sum M^i p_i, 1 grand product g = p0*sum gam^i p_2i p_2i+1, 2 sum of pair products.
 *   tables[i]: host pointer, 2^nv u64 (is_base) or 2^nv (c0,c1) pairs. The challenge chain starts after
 *   `chain_skip` E challenges. Outputs: msgs nv*(d+1) E, point nv E, evals ntab E, sums nv*d E (raw per-round sums).
 *   Refused with -1 (hg_last_error names hg_sumcheck), checked on the host before anything is launched: kind outside 0..2; an odd
 *   ntab in kinds 1 and 2; npw < ntab (kind 0) or npw < ntab/2 (kind 1; kind 2 reads no powers); more tables than the kernels carry
 *   powers or pairs for - ntab > 64 (kind 0), ntab/2 > 64 (kind 1), ntab/2 > 32 (kind 2); tables of mixed fields in kinds 0 and 1,
 *   anything but (base, ext) pairs in kind 2; a table entry, power or claim coordinate >= p (values are canonical everywhere).
 *   Launch plan: kinds 0 and 1 record the fork as hg_prove does, so a grand product's small rounds (half <= 2^14, behind the first
 *   round) are split - folds on the main stream, their sums in one pass on a side stream that is joined before the results are
 *   read. hg_set_option(ctx, "one_stream", 1) selects the unforked plan (whole rounds, one stream). HG_DEBUG=plan prints either. */
int hg_sumcheck(hg_ctx* ctx, int kind, size_t nv, size_t ntab, const uint64_t* const* tables, const int* is_base,
                const uint64_t* pw, size_t npw, const uint64_t* claim2, size_t chain_skip, uint64_t* msgs,
                uint64_t* point, uint64_t* evals, uint64_t* sums);

/* The prover's own PRODSUM flush (the Vanilla / FFT node reductions of hg_prove) on caller tables, for kernel-level tests; the
 *   Goldilocks counterpart of hg_prodsum_jobs_bn254, with its conventions. Job q is a sum-check over 2^nv[q] entries with npairs[q]
 *   pairs; all jobs go through one prover, one bookkeeping flush and ONE round-synchronised PRODSUM flush, so jobs of different sizes
 *   and forms share the step launches and the tail launch exactly as in a prove. Job q takes its nv[q] round challenges from the
 *   chain at chain_skip + sum_{q' < q} nv[q'] (E challenges).
 *   eq4[4q .. 4q+3] = (form, z_off, w, hib):
 *     form 0, plain: g = sum_i a_i b_i on tables a_i (2^nv words) and b_i (2^nv (c0, c1) pairs); tables holds a_0, b_0, a_1, b_1, ..;
 *       the other three words are not read.
 *     form 1, eq-factored: every b_i = kappa_i eq(z', .) with z' = (chain[z_off .. z_off + w), bits of hib, lowest first) - a table
 *       that is zero outside block hib of 2^w entries - and no b table exists before the tail; tables holds a_0, a_1, .. only, and
 *       kappa2 the job's npairs (c0, c1) pairs (the eq-factored jobs' kappas, concatenated in job order; may be null without such a
 *       job). The job is queued with the first tail round the prover plans for its shape. HG_NO_PS_EQ is not read here.
 *   sums2: per job nv[q] x (g(0), g(2)) raw round sums, concatenated; evals2: per job the 2 npairs[q] folded values (a_0(r), b_0(r),
 *   a_1(r), ..), concatenated - b_i(r) = kappa_i eq(z', r) for an eq-factored job.
 *   HG_DEBUG=plan prints `[hg plan] eqprep points=..` (the point tables' launch), one `[hg plan] prodsum two= eq= cnt= rd= h=[..]` line
 *   per step launch (an eq-factored launch adds grp=[..] table groups, wg=[..] workgroups per group and out_tail=[..] per item) and the
 *   `prodsum tail jobs= tail_rd=` line.
 *   -1 before any launch (hg_last_error names hg_prodsum_jobs) for: a null argument; njobs outside 1..128; nv outside 1..26; npairs
 *   outside 1..32; a form above 1; a table word or a kappa coordinate >= p (the points' coordinates come from the chain); w > nv;
 *   hib >= 2^(nv - w); chain_skip or z_off above 2^20; an eq-factored job whose shape does not take the form (the message says
 *   "does not take the eq-factored form": fewer than two rounds ahead of the tail, or a last pass below 2^9 pairs). */
int hg_prodsum_jobs(hg_ctx* ctx, size_t njobs, const size_t* nv, const size_t* npairs, const uint64_t* const* tables, const size_t* eq4,
                    const uint64_t* kappa2, size_t chain_skip, uint64_t* sums2, uint64_t* evals2);
/* The challenge-only tables of a batch of claims as the prover builds them for the plain node reductions, for kernel-level tests:
 *   all jobs of a call are queued as a node queues them and run in ONE bookkeeping flush. Claim a of job q has its point at
 *   chain[point_off[c0 + a] ..] (c0 = sum_{q' < q} nclaims[q'], E challenges) and the weight chain[alpha_off[q] + a];
 *   alpha_off[q] = SIZE_MAX: unit weight, one claim only. out[q]: host, 2^n[q] (2^L[q]) (c0, c1) pairs.
 *   hg_claim_tables_eq: out[q] = sum_a alpha_a eq(r_a, .) over n[q] variables (coordinate i belongs to bit i of the index): one plan,
 *     one factor-table launch and one fill launch for the batch (`[hg plan] eqtab jobs= ab= max_n= prep= fill= rows=`). n <= 24: the
 *     one-launch form the prover keeps for larger tables (with its summing pass) is not reachable here - no parameter set builds
 *     such a table.
 *   hg_claim_tables_fft: the DFT-row tables of FFT nodes, out[q][x] = scale sum_a alpha_a prod_b (1 + r_{a,b} (W[(x 2^b) mod N] - 1)),
 *     N = 2^L[q], W the powers of the N-th root of unity of hg_ntt (inverse[q]: of its inverse, and scale = 1 / N, else 1): one call
 *     of the batch kernel for all jobs (`[hg plan] fftrows jobs= max_L= max_claims= launches=`).
 *   -1 before any launch (hg_last_error names the entry) for: a null argument or output; njobs outside 1..64; n or L outside 1..24;
 *   nclaims outside 1..32; a unit weight with several claims; point_off or alpha_off above 2^20. */
int hg_claim_tables_eq(hg_ctx* ctx, size_t njobs, const size_t* n, const size_t* nclaims, const size_t* point_off, const size_t* alpha_off,
                       uint64_t* const* out);
int hg_claim_tables_fft(hg_ctx* ctx, size_t njobs, const size_t* L, const int* inverse, const size_t* nclaims, const size_t* point_off,
                        const size_t* alpha_off, uint64_t* const* out);

/* = prove_grand_product [REF lasso/src/memory_checking/prover.rs:183-266] on nb <= 128 host tables of len = 2^nv base-field values: product
 *   tree on the MSB split, root products, per layer the batched degree-3 sum-check, 2 nb evaluations and the mu fold. The transcript
 *   starts after `chain_skip` E challenges. claims2: nb final claims (E), point2: nv coordinates (E). (Goldilocks counterpart of
 *   hg_grand_product_bn254)
 *   Launch plan: as in hg_prove - the fork is recorded ahead of the layers, whose small rounds are split (folds on the main stream,
 *   sums on a side stream joined before the results are read); hg_set_option(ctx, "one_stream", 1): whole rounds on one stream. */
int hg_grand_product(hg_ctx* ctx, size_t nb, size_t len, const uint64_t* const* tables, size_t chain_skip, uint8_t* proof, size_t cap,
                     size_t* proof_len, uint64_t* claims2, uint64_t* point2);
/* = BoxMultilinearPoly::fix_var on the lowest variable (inside gkr::sum_check::prove_sum_check; SURVEY.md 8(c) convention C3):
 *   out[j] = T[2j] + r (T[2j+1] - T[2j]), j < 2^(nv-1). table: 2^nv base values (is_base) or (c0, c1) pairs; out: 2^(nv-1) pairs.
 *   Refused with -1 (hg_last_error names hg_fold), checked on the host before anything is launched: a null argument; nv outside
 *   1..30 (checked before the table is read); a table word or a coordinate of r that is >= p. */
int hg_fold(hg_ctx* ctx, const uint64_t* table, size_t nv, int is_base, const uint64_t r2[2], uint64_t* out);

/* = BoxMultilinearPoly::evaluate [REF call sites memory_checking/mod.rs:80-93, sk_encryption_circuit.rs:446]
 *   on a host table of 2^nv base-field values at an E point (point: nv (c0, c1) pairs, lowest variable first; may be null at nv = 0).
 *   Refused with -1 (hg_last_error names hg_mle_eval), checked on the host before anything is launched: a null argument; nv > 30
 *   (checked before the table is read); a table word or a point coordinate that is >= p. */
int hg_mle_eval(hg_ctx* ctx, const uint64_t* table, size_t nv, const uint64_t* point, uint64_t out2[2]);

/* = FftNode evaluate (size-2^log2n NTT, natural order in/out) [REF sk_encryption_circuit.rs:224,249,251]. Device.
 *   in, out: batch rows of 2^log2n canonical words. 8 <= log2n <= 16 runs the LDS-resident four-step kernels (2^n1 x 2^n2,
 *   n1 = log2n / 2), every other size radix-2 stages in HBM.
 *   Refused with -1 (hg_last_error names hg_ntt), checked on the host before anything is launched: a null argument; log2n outside
 *   1..32; batch == 0; batch > 65535 when 8 <= log2n <= 16 (the four-step grids carry the batch in their y extent); a batch whose
 *   byte count does not fit size_t - all of these before `in` is read; an input word >= p.
 *   HG_DEBUG=plan prints the path taken, one line per call: `[hg plan] ntt log2n=.. batch=.. path=four n1=.. n2=..` or
 *   `[hg plan] ntt log2n=.. batch=.. path=radix2 grid=..` (grid: workgroups of a stage launch; the bit reversal has twice as many). */
int hg_ntt(hg_ctx* ctx, const uint64_t* in, size_t log2n, int inverse, size_t batch, uint64_t* out);

/* Fiat-Shamir challenge chain [REF bfv-gkr/src/transcript.rs:146-157,198-203]: first n base-field challenges. */
int hg_challenges(size_t n, uint64_t* out);

/* ---- BN254 (BASELINE config 5): the same path over halo2curves bn256::Fr (F = E = Fr) ---------------------------------
 * Elements cross the boundary as 4 canonical little-endian u64 limbs (non-Montgomery). The extension field of the
 * reference's bn254 tests is the field itself [REF sk_encryption_circuit.rs:614-626: (Fr, Fr)], so a challenge is one
 * element. hg_prove_bn254 is the whole BfvEncrypt::prove over Fr; the entry points before it expose its parts for parity tests. */
/* = Keccak256Transcript::squeeze_challenge over Fr: c_j = LE(Keccak^j("")) mod r [REF transcript.rs:146-157,198-203]; n x 4 limbs */
int hg_challenges_bn254(size_t n, uint64_t* out4);
/* device field arithmetic on n element pairs: op 0 add, 1 sub, 2 mul, 3 mul through the column accumulators, 4 a b + a a + b b
 * through one deferred reduction (known-answer tests of the Montgomery kernels; operands and results canonical, converted inside).
 * ops 5 .. 9: the branch-free loose forms the hot kernels use (bn254_lazy.hpp) on RAW 256-bit operands, results as canonical
 * residues: 5 a b R^-1 (any operands), 6 a + r b R^-1 with r = 2^200 + 12345 (a < 2p), 7 a + b, 8 a - b (a, b < 2p),
 * 9 (a b + a a + b b + (a - b + 2p) b) R^-1 through one reduction (a, b < 2p); R = 2^256. */
int hg_bn254_field_op(hg_ctx* ctx, int op, size_t n, const uint64_t* a4, const uint64_t* b4, uint64_t* out4);
/* = gkr::sum_check::prove_sum_check over Fr on caller tables, same shapes and conventions as hg_sumcheck
 *   [REF call sites lasso.rs:278-279, prover.rs:242-252]. tables[i]: host pointer, 2^nv elements (4 limbs each).
 *   Outputs: msgs nv*(d+1), point nv, evals ntab, sums nv*d elements.
 *   Its round kernel (k_bn_round, with k_bn_reduce) is a plain form of the three shapes that nothing else launches: it is NOT one of
 *   the kernels hg_prove_bn254 runs. Those are reached through hg_prodsum_jobs_bn254 (PRODSUM) and hg_grand_product_bn254. */
int hg_sumcheck_bn254(hg_ctx* ctx, int kind, size_t nv, size_t ntab, const uint64_t* const* tables, const uint64_t* pw4, size_t npw,
                      const uint64_t* claim4, size_t chain_skip, uint64_t* msgs, uint64_t* point, uint64_t* evals, uint64_t* sums);
/* The prover's own PRODSUM launches (the Libra / zkCNN node reductions of hg_prove_bn254) on caller tables, for kernel-level tests:
 *   job q is the sum-check of g = sum_i a_i b_i over 2^nv[q] entries with npairs[q] pairs; every job is queued and the batch runs as
 *   ONE round-synchronised flush - the shared round launches over jobs of different sizes, one reduce launch, one tail workgroup per job.
 *   tables: a_0, b_0, a_1, b_1, .. of every job, in job order (host pointers, 2^nv[q] canonical elements each). A job of more than one
 *   pair whose b pointers are all the SAME host pointer uploads b once and takes the shared-b form. win[2q], win[2q+1]: b of job q is
 *   zero outside the entries [lo, hi) ((0, 0): no window; needs npairs[q] == 1, and the entries outside are checked to be zero); a
 *   window that is not a run of whole pairs in every shared round is dropped and the job runs the plain form. Job q takes its nv[q]
 *   round challenges from the chain at chain_skip + sum_{q' < q} nv[q'].
 *   sums4: per job nv[q] x (g(0), g(2)), concatenated; evals4: per job the 2 npairs[q] folded values (a_0, b_0, a_1, ..), concatenated.
 *   HG_DEBUG=bnplan prints the staged descriptors (`[hg bnplan] ps ..`; `gp ..` for hg_grand_product_bn254): which form each round took.
 *   -1 before any launch for: njobs outside 1..64, nv outside 2..32, npairs outside 1..32, an element >= r, a window on a job of
 *   several pairs, a non-zero entry outside a window. */
int hg_prodsum_jobs_bn254(hg_ctx* ctx, size_t njobs, const size_t* nv, const size_t* npairs, const uint64_t* const* tables, const size_t* win,
                          size_t chain_skip, uint64_t* sums4, uint64_t* evals4);

/* = prove_grand_product over Fr [REF lasso/src/memory_checking/prover.rs:183-266]: nb tables of len = 2^nv elements; product tree on
 *   the MSB split, root products, per layer a degree-3 sum-check with g = poly(0) * sum_b gamma^b v_l,b v_r,b, 2 nb evaluations and the
 *   mu fold. proof: 32-byte big-endian canonical elements [REF transcript.rs:183-189]. claims4: nb final claims, point4: nv coordinates. */
int hg_grand_product_bn254(hg_ctx* ctx, size_t nb, size_t len, const uint64_t* const* tables, size_t chain_skip, uint8_t* proof, size_t cap,
                           size_t* proof_len, uint64_t* claims4, uint64_t* point4);
/* = <LassoNode as Node>::prove_claim_reduction over Fr [REF lasso/src/lasso.rs:57-114]: the same node as hg_lasso_prove_at, for the
 *   bn254 test family. lasso_in4: 2^nu elements (4 limbs each; range-shifted values, i.e. below 2^64). The limb split and the
 *   counters are integer kernels shared with the Goldilocks path; claimed sum, collation sum-check, multiset hashes, both grand
 *   products and the openings run over Fr. proof: 32-byte big-endian elements. claim_out4: nu coordinates of r, then the claimed sum. */
int hg_lasso_prove_bn254(hg_ctx* ctx, const hg_pk* pk, const uint64_t* lasso_in4, size_t chain_skip, uint8_t* proof, size_t cap, size_t* len,
                         uint64_t* claim_out4);
/* = BoxMultilinearPoly::evaluate over Fr [REF memory_checking/mod.rs:80-93]: table of 2^nv elements at a point of nv elements,
 *   lowest variable first. Runs the fold sequence of hg_prove_bn254's own evaluation: up to ten variables bound per launch, no launch
 *   left with a single one (11 variables: 9 then 2); nv < 2 without such a launch.
 *   Refused with -1 (hg_last_error names hg_mle_eval_bn254), checked on the host before anything is launched: a null context or
 *   pointer (point4 may be null at nv = 0); nv > 28 (checked before the table is read); a table or point element >= r.
 *   HG_DEBUG=bnplan prints `[hg bnplan] mle nv=.. m=[..]`: the variables bound by each launch, in order (m=[] for nv < 2). */
int hg_mle_eval_bn254(hg_ctx* ctx, const uint64_t* table4, size_t nv, const uint64_t* point4, uint64_t out4[4]);
/* = FftNode evaluate over Fr [REF sk_encryption_circuit.rs:224,249,251]: size-2^log2n NTT with the root of unity
 *   7^((r-1)/2^log2n) (halo2curves ROOT_OF_UNITY, two-adicity 28), natural order in / out; inverse scales by 1/n.
 *   8 <= log2n <= 16 runs the LDS-resident four-step kernels (n1 = log2n / 2), every other size radix-2 stages in HBM.
 *   Refused with -1 (hg_last_error names hg_ntt_bn254), checked on the host before anything is launched: a null context or pointer;
 *   log2n outside 1..28; batch == 0; batch > 65535 when 8 <= log2n <= 16; a batch whose byte count does not fit size_t - all of
 *   these before in4 is read; an element >= r.
 *   HG_DEBUG=bnplan prints the path taken: `[hg bnplan] ntt log2n=.. batch=.. path=four n1=.. n2=..` or `.. path=radix2 grid=..`
 *   (grid: workgroups of a stage launch). */
int hg_ntt_bn254(hg_ctx* ctx, const uint64_t* in4, size_t log2n, int inverse, size_t batch, uint64_t* out4);

/* = BfvSkEncryptArgs from one of the reference's bn254 fixtures [REF bfv-gkr/src/data/bn254/ *.json, sk_encryption_circuit.rs:365-415]:
 *   coefficients are bn256::Fr elements (negatives as r - |z|). Every coefficient of a valid witness is a small signed integer, which
 *   is what the handle stores (an element that is not an integer below 2^62 in magnitude is rejected); the same handle type as
 *   hg_witness_from_json / hg_witness_synthetic, so those witnesses can be proven over Fr as well. */
int hg_witness_from_json_bn254(const hg_params* params, const char* path, hg_witness** out);
/* = Circuit::evaluate over Fr on the device [REF sk_encryption_circuit.rs:434-442]; returns one table as canonical limbs:
 *   which = 0 the `sum` node (must equal ct0is), 1 the Lasso input node, 2 the ct0is table as laid out by get_inputs */
int hg_circuit_eval_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, int which, uint64_t* out4, size_t cap_elems, size_t* n_elems);
/* = BfvEncrypt::<_, 1>::prove::<Fr, Fr> [REF sk_encryption_circuit.rs:417-460, 614-626]: witness generation, output claim, the
 *   prove_gkr walk (Libra / zkCNN / Lasso node reductions) over bn256::Fr. proof: 32-byte big-endian elements
 *   [REF transcript.rs:183-189]. ms2 (may be null): witness generation and proving wall time in ms. */
int hg_prove_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, uint8_t* proof, size_t cap, size_t* len, double* ms2);
/* = BfvEncrypt::verify::<Fr, Fr> [REF sk_encryption_circuit.rs:462-517]: host side (no device needed; pk may come from
 *   hg_setup(NULL, ..)). Returns 0 accept, 1 reject (reason in hg_last_error), -1 error. */
int hg_verify_bn254(const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len);
/* The same check with the table-sized work on the device [REF sk_encryption_circuit.rs:462-517, 614-626; lasso/src/memory_checking/
 * verifier.rs:130-176]: the host parses the proof and checks the round polynomials and the Lasso scalars; the eq tables, the
 * wiring-predicate sums of the Vanilla nodes, the DFT rows of the FFT nodes and the MLE evaluations of the public inputs run as
 * kernels over bn256::Fr (one stream, one synchronisation). Needs a device context and a device key (hg_setup(ctx, ..)). Same return
 * values and the same accept / reject decisions as hg_verify_bn254; mode 0 only. */
int hg_verify_device_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* w, const uint8_t* proof, size_t len);
/* hg_verify_device_bn254 for a run of n proofs under one key: the contract of hg_verify_device_batch without a mode (BN254 is mode 0
 * only). results[i] = 0 accepted / 1 rejected, exactly the decision hg_verify_device_bn254 (and hg_verify_bn254) makes for
 * (ws[i], proofs[i]); reasons (may be NULL) receives the reason that call leaves in hg_last_error, NUL-terminated and truncated to
 * reason_cap bytes, at reasons + i*reason_cap ("" when accepted). Returns the number of rejected proofs (>= 0), or -1 on an error
 * (hg_last_error names the function and, for an error inside one proof's check, its index). n == 0 returns 0. Needs a device
 * context and a device key. The walks run on the host threads; the table-sized work of a group of proofs (context option
 * "verify_batch_group") runs in one launch per kind, tables that depend on the key only built once per group; the inputs of the
 * next group are copied meanwhile. */
int hg_verify_device_batch_bn254(hg_ctx* ctx, const hg_pk* pk, const hg_witness* const* ws, const uint8_t* const* proofs,
                                 const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap);

/* ---- Verification from the ciphertext over bn256::Fr: the counterparts of hg_verify_public, hg_verify_public_device,
 * hg_claims_settle and hg_instance_mle (above), with the same contracts, return values and error rules. BN254 is mode 0 only: no
 * entry takes a mode. An element crosses the ABI as 4 canonical little-endian u64 limbs. The instance is the field-independent
 * hg_instance* of hg_instance_from_ciphertext / hg_instance_from_witness, the claim counts are hg_pk_claim_shape's; instance and
 * claim array (hg_input_claim_bn254*) cross as void pointers. hg_verify_public_bn254 followed by hg_claims_settle_bn254 decides
 * what hg_verify_bn254 decides. One proof per call; hg_verify_public_batch_bn254 (below) verifies a run of them in one device pass. */
typedef struct hg_input_claim_bn254 {
    uint32_t input;      /* as hg_input_claim: 0 s, 1 e, 2 k1, 3+k+i r1is[i], 3+2k r2is (never 3..3+k-1) */
    uint32_t nvars;
    uint64_t point_off;  /* coordinates points4[4*point_off .. 4*(point_off+nvars)), 4 limbs each */
    uint64_t value[4];
} hg_input_claim_bn254;

/* = BfvEncrypt::verify::<Fr, Fr> [REF sk_encryption_circuit.rs:462-517, 614-626] up to the point where it needs a secret: the walk
 *   of hg_verify_bn254 with ct0is and the ais tables evaluated from the instance's compact coefficients (a negative z counts as
 *   r - |z|); a claim on any other input is not evaluated but written out. claims: room for claim_cap hg_input_claim_bn254; points4:
 *   room for coord_cap coordinates (4 words each). Returns 0 accept (claims and points filled, *n_claims set), 1 reject (reason in
 *   hg_last_error, *n_claims = 0; the reasons are hg_verify_bn254's), -1 error: a null argument, claim_cap or coord_cap below
 *   hg_pk_claim_shape, an instance of other parameters; the device form also: no context, a host-only key.
 *   Claim order: inputs ascending, within one input the order in which the walk pushes them; the same for both forms. Points are
 *   written out as values.
 *   hg_verify_public_bn254 is the host form (works with hg_setup(NULL, ..)). hg_verify_public_device_bn254 runs the table-sized
 *   work as hg_verify_device_bn254 does (one stream, one synchronisation), with the instance uploaded as it is (2 k n signed words:
 *   8.4 MB at n=32768 k=16, and no witness table) and the MLE evaluations of ais and ct0is in one kernel over Fr that reads the signed
 *   words and the half of each eq table that meets a non-padding word; the secret inputs launch nothing. Same decisions, claims and
 *   points as the host form, bit for bit. */
int hg_verify_public_bn254(const hg_pk* pk, const void* instance, const uint8_t* proof, size_t len, void* claims, size_t claim_cap,
                           uint64_t* points4, size_t coord_cap, size_t* n_claims);
int hg_verify_public_device_bn254(hg_ctx* ctx, const hg_pk* pk, const void* instance, const uint8_t* proof, size_t len, void* claims,
                                  size_t claim_cap, uint64_t* points4, size_t coord_cap, size_t* n_claims);
/* = izip_eq!(inputs, input_claims) [REF sk_encryption_circuit.rs:512-516] over Fr for the n claims of an hg_input_claim_bn254 array:
 *   table `input` of w (any input 0 .. 3+2k) at the point == value, for every claim. ctx == NULL: host; with a context: the points
 *   staged as a chain of their own, each table uploaded once, one batch of eq tables and dot products, one synchronisation. Returns
 *   0, 1 ("input claim mismatch at input K", the lowest failing K: the verifiers' text) or -1 (a null argument, a handle of other
 *   parameters, no such input, nvars that is not the table's, a coordinate or value that is not below r). */
int hg_claims_settle_bn254(hg_ctx* ctx, const hg_params* params, const hg_witness* w, const void* claims, size_t n, const uint64_t* points4);
/* part exposed for parity tests: the MLE of one laid-out public table at an Fr point, computed from the compact coefficients
 * (ctx == NULL: host loop; else the kernel of hg_verify_public_device_bn254). which 0: ais[index] (L vars); 1: ct0is, the whole
 * table (L + log2 k vars, index ignored). out4: canonical limbs. -1 for a null argument, another selector or modulus, nvars that is
 * not the table's, a coordinate that is not below r. */
int hg_instance_mle_bn254(hg_ctx* ctx, const void* instance, int which, int index, const uint64_t* point4, size_t nvars, uint64_t out4[4]);

/* hg_verify_public_device_bn254 for a run of n proofs under one key: the contract of hg_verify_public_batch without a mode (BN254 is
 *   mode 0 only), with the element conventions of hg_verify_public_device_bn254. Proof i (proofs[i], lens[i]) is checked against
 *   instances[i] (an hg_instance* of the key's parameters). Device only. results[i] = 0 accepted / 1 rejected, exactly the decision
 *   hg_verify_public_device_bn254 makes for that pair alone; reasons (may be NULL): at reasons + i*reason_cap the text that call leaves
 *   in hg_last_error, NUL-terminated and truncated to reason_cap bytes ("" when accepted). An accepted proof i writes its claims at
 *   (hg_input_claim_bn254*)claims + i*claim_cap_each and its points at points4 + 4*i*coord_cap_each, point_off relative to that
 *   proof's own block, and n_claims[i] = the claim count: claim order, values and points are bit for bit those of the single call. A
 *   rejected proof gets n_claims[i] = 0. Returns the number of rejected proofs (>= 0); n == 0 returns 0 and writes nothing; -1 on an
 *   error of the call, which writes no output either (hg_last_error begins with the function's name and gives "index i" where an
 *   element is at fault): no context, a host-only key, a null argument or a null element, claim_cap_each or coord_cap_each below
 *   hg_pk_claim_shape, an instance of other parameters.
 *   The pass is hg_verify_device_batch_bn254's - walks on the host threads, a group of proofs (context option "verify_batch_group",
 *   at most 64) in one launch per kind, key-only tables built once per group, the next group's copies under this group's kernels -
 *   with each proof's instance staged as it is (2 k n signed words: 8.4 MB at n=32768 k=16 against 30.9 MB of witness tables) and
 *   ais / ct0is evaluated from them by one kernel over Fr per group that reads the non-padding half of each eq table once for all
 *   the group's members; the secret inputs launch nothing. */
int hg_verify_public_batch_bn254(hg_ctx* ctx, const hg_pk* pk, const void* const* instances, const uint8_t* const* proofs,
                                 const size_t* lens, size_t n, int* results, void* claims, size_t claim_cap_each,
                                 uint64_t* points4, size_t coord_cap_each, size_t* n_claims, char* reasons, size_t reason_cap);
/* hg_instance_mle_bn254 for the kernel of hg_verify_public_batch_bn254: the table (which / index as above) of n instances of one
 * parameter set at ONE shared point of 4-limb coordinates below r, as one work unit of that kernel with n members; out4 receives 4
 * canonical limbs per instance. Device only. Returns 0, or -1 for a null argument or element, no context, instances of mixed
 * parameters, another selector or modulus, nvars that is not the table's, a coordinate that is not below r. */
int hg_instance_mle_batch_bn254(hg_ctx* ctx, const void* const* instances, size_t n, int which, int index,
                                const uint64_t* point4, size_t nvars, uint64_t* out4);

/* ---- Polynomial commitment over bn256::Fr: what opens the claims hg_verify_public_bn254 leaves --------------------------------------
 * The scheme of the Goldilocks block above (hg_pcs_commit ..) with F = E = Fr (r = the order of bn256's scalar field). Shape rules,
 * limits, the log2_row = 0 rule, n_queries = 0 -> 241 and the 65535-row cap of the device commit are unchanged; the 241 is the same
 * (3/4)^Q term, and with a 254-bit field ONE rho is enough for the combination's own error - no more is claimed. Not zero knowledge;
 * BN254 has no protocol modes, so no BN254 proof absorbs the root ("Bound proofs" above is Goldilocks only). An element crosses the ABI as 4 canonical little-endian u64 limbs, as
 * everywhere in the BN254 entries. repr(x) below is the 32-byte little-endian canonical, non-Montgomery form (halo2curves to_repr).
 *   Rows.   Table t has 2^{v_t} elements and is cut into rows of C = 2^c elements; rows are stacked in table order (R rows, off_t).
 *   Code.   Enc(row) = the forward NTT of size N = 4C of the row zero-padded to 4C elements, natural order, root of unity
 *           7^((r-1)/2^(c+2)): what hg_ntt_bn254(.., log2n = c+2, inverse = 0, ..) computes.
 *   Tree.   leaf_j = Keccak256(LE64(0) || repr(M[0][j]) || .. || repr(M[R-1][j])), j < 4C, M[r] = Enc(row_r); an inner node is
 *           Keccak256(LE64(1) || left || right), as above; the commitment is the 32-byte root.
 *   Transcript. Absorbing: the hash state starts as the ASCII bytes "hg-pcs-bn254-1", the root, then as 4-byte little-endian c, m,
 *           v_0 .. v_{m-1}, Q, n, then per claim t_i (4-byte LE), repr of every coordinate of the point, repr of the value. A
 *           challenge: h = Keccak256(state); the challenge is LE(h) mod r; the state becomes h (what is absorbed later is appended
 *           to it). With nothing absorbed this is the chain of hg_challenges_bn254.
 *   Opening of n claims (t_i, z_i in Fr^{v_{t_i}}, y_i) with Q = n_queries:
 *     1. rho = one squeezed element; u_0[j] = sum_{r<R} rho^r row_r[j], j < C;
 *     2. per claim w_i = eq(z_i[c..]) and u_i[j] = sum_r w_i[r] row_{off_t + r}[j];
 *     3. u_0, u_1 .. u_n are written as 32-byte big-endian elements (as every BN254 proof element) and absorbed as repr;
 *     4. Q column indices j_q = (the low 64 bits of a squeezed canonical element) & (4C - 1), duplicates kept;
 *     5. per query the R column elements M[.][j_q] (32-byte big-endian), then the c+2 siblings bottom-up (32 raw bytes each).
 *     Length: exactly 32 C (n+1) + Q (32 R + 32 (c+2)) bytes.
 *   Verification (hg_pcs_verify_bn254 on the host, hg_pcs_verify_device_bn254 on a context): the order of checks and the reason strings of hg_pcs_verify - length; every element
 *     below r ("pcs: non-canonical word at byte B", B = the offset of the first byte of the first element that is not below r, the
 *     u_i first, then the columns query by query); <u_i, eq(z_i[..c])> == y_i; per query the path, the proximity combination against
 *     Enc(u_0)[j_q], every claim's combination against Enc(u_i)[j_q].
 * Contracts as above: 0, 1 = rejected with the reason in hg_last_error (the verifiers only), -1 with text that names the function.
 * A handle carries its field: hg_pcs_free frees a handle of either; a Goldilocks handle given to hg_pcs_open_bn254 /
 * hg_claims_open_bn254 is an error (-1), and so is a BN254 handle given to hg_pcs_open / hg_claims_open.
 *
 * hg_pcs_commit_bn254: tables4[t] = 2^{nvars[t]} elements of 4 limbs. ctx == NULL: the host form (radix-2 NTT and hashes on the
 *   host's threads); with a context the device form on one stream with one synchronisation: the tables are uploaded as they are, a
 *   kernel writes the zero-padded 4C-stride matrix, the batched Fr NTT encodes it in place (four-step in LDS for 8 <= c+2 <= 16,
 *   radix-2 stages otherwise), one thread per column hashes it with the Keccak state in registers, the tree is built by the kernels
 *   of hg_pcs_commit. The encoded matrix stays in HBM as canonical plain limbs; the handle owns it and the raw rows (57 MB + 227 MB
 *   for the secrets of n=32768 k=16 at c=11) and a host copy of the tree; the NTT temporary is the context's arena. Both forms give
 *   the same root. -1: a null argument or table, a shape outside the limits, an element that is not below r (the same text in both
 *   forms), more than 65535 rows on the device.
 * hg_pcs_open_bn254: points4 = the claims' points one behind the other, 4 limbs per coordinate; values4: 4 limbs per claim. ctx
 *   must be the context the commitment was made on (NULL for the host form). The device form runs the row combinations as one
 *   launch and gathers the opened columns with another; it synchronises twice, as hg_pcs_open. Same bytes as the host form. -1 as
 *   hg_pcs_open, and for a handle over Goldilocks.
 * hg_pcs_verify_bn254: host only, no context. -1 as hg_pcs_verify.
 * hg_pcs_verify_device_bn254: hg_pcs_verify_bn254 with the table-sized work on the context's stream; the decision and the reason
 *   are the host verifier's on every input, also where several checks fail at once (the order above decides: length, the first
 *   element not below r, the lowest claim whose evaluation fails, the lowest query and within it path, proximity, claims
 *   ascending). The opening is uploaded as it is; kernels byte-swap its elements into 4 limbs and compare each with r, check the
 *   evaluations, encode the u_i with the batched Fr NTT, form the inner products of the opened columns and hash them while the host
 *   hashes the u_i into the transcript; the Q column indices follow on the same stream and a last kernel walks the paths and
 *   compares; three result words come back: one synchronisation. -1 as hg_pcs_verify_bn254 (naming this function), for a null
 *   context (".. : no context"), and if the context's arena cannot hold the opening. It uses the context's arena like a prove: not
 *   concurrently with another call on the same context.
 * hg_secrets_commit_bn254: hg_pcs_commit_bn254 of the five secret inputs of a witness handle, tables in input order and with the
 *   variable counts of hg_secrets_commit; every u64 word of the handle is lifted into Fr by the signed rule - a word below 2^63 is
 *   itself, any other is r - (p_goldilocks - word) - which is the table hg_claims_settle_bn254 evaluates. The device form uploads
 *   the words (a quarter of the bytes) and lifts them by a kernel.
 * hg_claims_open_bn254 / hg_claims_verify_bn254: hg_pcs_open_bn254 / hg_pcs_verify_bn254 for an hg_input_claim_bn254 array and
 *   points4 exactly as hg_verify_public_bn254 / hg_verify_public_batch_bn254 return them, with the input-to-table mapping and the -1
 *   cases of hg_claims_open / hg_claims_verify. hg_verify_public_bn254 followed by hg_claims_verify_bn254 against a root the
 *   encryptor published is a BN254 verification that needs no secret. hg_claims_verify_device_bn254 is
 *   hg_pcs_verify_device_bn254 under the same mapping. hg_claims_open_bn254 takes a commitment hg_secrets_commit_bn254 or
 *   hg_secrets_commit_batch_bn254 made, or hg_prove_encryptions_committed_bn254. */
int hg_pcs_commit_bn254(hg_ctx* ctx, const uint64_t* const* tables4, const uint32_t* nvars, size_t n_tables, size_t log2_row,
                        void** commitment, uint8_t root[32]);
int hg_pcs_open_bn254(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points4, const uint64_t* values4,
                      size_t n_claims, size_t n_queries, uint8_t* proof, size_t cap, size_t* len);
int hg_pcs_verify_bn254(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table,
                        const uint64_t* points4, const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len);
int hg_pcs_verify_device_bn254(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table,
                               const uint64_t* points4, const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof,
                               size_t len);
int hg_secrets_commit_bn254(hg_ctx* ctx, const hg_params* params, const hg_witness* w, size_t log2_row, void** commitment, uint8_t root[32]);
int hg_claims_open_bn254(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n,
                         const uint64_t* points4, size_t n_queries, uint8_t* opening, size_t cap, size_t* len);
int hg_claims_verify_bn254(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n,
                           const uint64_t* points4, size_t n_queries, const uint8_t* opening, size_t len);
int hg_claims_verify_device_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n,
                                  const uint64_t* points4, size_t n_queries, const uint8_t* opening, size_t len);

/* ---- Folded openings over BN254: "Folded openings" above with F = E = Fr ---------------------------------------------------------
 * The six folded entries over bn256::Fr, with the element conventions of the BN254 commitment above: 4 canonical little-endian limbs
 * across the ABI, 32-byte big-endian elements in the opening, repr absorbed, claims as hg_input_claim_bn254 with points4. An element is
 * four times a Goldilocks word, so folding saves most here: for the 47 claims of n=32768 k=16 (m = 20, V = 19, c = 11, C = 2048,
 * R = 864, Q = 241) a folded opening is 2464 + 131072 + 6763424 = 6 896 960 bytes against 9 909 152, the transcript hashes 128 KB of u
 * instead of 3.1 MB, and prover and verifiers form 2 row combinations instead of 48.
 *
 * The scheme; V = max_t v_t, n >= 1 claims (t_i, z_i, y_i); one squeezed element is one challenge, there is no extension field.
 *   Transcript. That of "hg-pcs-bn254-1": absorbing, challenge = LE(Keccak256(state)) mod r, the state becomes the hash. It starts as
 *     the 19 ASCII bytes "hg-pcs-bn254-fold-1" followed by exactly what "hg-pcs-bn254-1" appends after its tag: the root, c, m,
 *     v_0 .. v_{m-1}, Q, n (4-byte LE), per claim t_i (4-byte LE), repr of the point's coordinates and of the value. Every element
 *     written below is absorbed as repr (32 bytes little-endian, canonical) and appears in the opening as 32 bytes big-endian.
 *   1. beta is squeezed. S = sum_i beta^i y_i. For every table g_t(x) = sum_{i: t_i = t} beta^i eq(z_i, x) on v_t variables (zero for
 *      a table without a claim): sum_t sum_x g_t(x) T_t(x) = S.
 *   2. V rounds, the lowest variable first; folding by r is T'[j] = T[2j] + r (T[2j+1] - T[2j]). In round j the prover writes the
 *      coefficients c0, c1, c2 of s_j(X) = sum_t s_{j,t}(X), then r_j is squeezed. For v_t > j, s_{j,t}(X) = sum_{x'} g_t^(j)(X, x')
 *      T_t^(j)(X, x') over the tables folded by r_0 .. r_{j-1}. For v_t <= j, s_{j,t}(X) = K_t prod_{v_t <= j' < j} (1 - r_j') (1 - X)
 *      with K_t = g_t(rho[..v_t)) T_t(rho[..v_t)). rho = (r_0 .. r_{V-1}).
 *   3. The prover writes Y_t = T_t(rho[0..v_t)), t = 0 .. m-1.
 *   4. delta, then rho' are squeezed. u_0[j] = sum_{r<R} rho'^r row_r[j]; u_1[j] = sum_t delta^t sum_{r < 2^{v_t-c}}
 *      eq(rho[c..v_t))[r] row_{off_t+r}[j]. u_0, then u_1 are written.
 *   5. Q column indices, each the low 64 bits of a squeezed element & (4C - 1), and 6. per query the R column elements and the c+2
 *      siblings, exactly as in "hg-pcs-bn254-1".
 *   Layout: a header of 32 (3 V + m) bytes - the round coefficients, then the Y_t - followed by a body that has exactly the layout of
 *     an "hg-pcs-bn254-1" opening of one claim: u_0, u_1, Q x (32 R + 32 (c+2)). Length: exactly 32 (3 V + m) + 64 C + Q (32 R + 32 (c+2)).
 *   Verification (hg_pcs_verify_folded_bn254 on the host, hg_pcs_verify_folded_device_bn254 on a context), in this order, the first
 *     failure is the reason:  1. the exact length ("pcs: the opening has .. bytes, .. expected", with the folded length);  2. every
 *     element below r ("pcs: non-canonical word at byte B", B = the offset of the first byte of the first element that is not below
 *     r, counted from the start of the folded opening: the header first, then u, then the columns query by query);  3. for j
 *     ascending 2 c0 + c1 + c2 == claim_j, claim_0 = S, claim_{j+1} = s_j(r_j) ("pcs: fold round j does not match the running
 *     claim");  4. claim_V == sum_t Y_t g_t(rho[..v_t)) prod_{j >= v_t} (1 - rho_j) ("pcs: fold final evaluation mismatch");
 *     5. <u_1, eq(rho[..c))> == sum_t delta^t Y_t ("pcs: evaluation mismatch at claim 0");  6. per query, ascending: the Merkle path,
 *     proximity, then the combined claim ("pcs: claim 0 inconsistent at query q"), the first two with the texts of hg_pcs_verify_bn254.
 *   Soundness is what "Folded openings" claims, over Fr. Still not zero knowledge.
 * Contracts are those of the Goldilocks folded entries. The forms for a run are hg_pcs_open_folded_batch_bn254,
 * hg_claims_open_folded_batch_bn254, hg_pcs_verify_folded_device_batch_bn254 and hg_claims_verify_folded_batch_bn254, below the single
 * calls; hg_prove_encryptions_committed_bn254 does not fold. hg_pcs_open and its BN254 neighbours, their bytes and "hg-pcs-bn254-1" are unchanged.
 * hg_pcs_open_folded_bn254: hg_pcs_open_bn254's arguments. n_claims == 0 is -1 ("<function>: a folded opening needs a claim").
 *   *len = the length also when cap is too small. A value that is not its table's evaluation is refused with hg_pcs_open_bn254's text
 *   under this name, naming the lowest failing claim. A Goldilocks handle or a handle of another context is -1. The host form
 *   (ctx == NULL) is the byte reference. The device form builds g in HBM beside the handle's raw rows (Montgomery form, 32 bytes a
 *   table entry, 57 MB at n=32768 k=16) with one kernel from per-claim factor tables staged in one copy, then runs one launch a round
 *   over all live tables on the context's stream with scratch from its arena ("the context's arena cannot hold the reduction" when
 *   it does not fit): four adjacent entries of a table and of g are folded by the previous challenge into two of each and enter the
 *   round's sums in the same pass (round 0 reads the raw rows, which are never written); the three sums come back once a round (one
 *   synchronisation a round), a table of two entries retires into two scalars, a table of one element is a scalar from the start.
 *   Everything that reaches the host is canonical, so device bytes equal host bytes. u_0 and u_1 are two row combinations of R rows
 *   through hg_pcs_open_bn254's kernel, the columns through its gather. Profiler class pcs_fold_bn254. HG_PCS_FOLD_BLOCKS bounds the
 *   workgroups of a launch as it does over Goldilocks. Not concurrently with another call on the same context.
 * hg_pcs_verify_folded_bn254: hg_pcs_verify_bn254's arguments and -1 cases, and n_claims == 0 as above. Host only.
 * hg_pcs_verify_folded_device_bn254: the same decision and reason on every input, also where several checks fail at once (a
 *   non-canonical body element together with a failing round reports the element). ctx == NULL is -1 ("<function>: no context").
 *   The header's checks are host scalar work; the body goes through the kernels of hg_pcs_verify_device_bn254 as an opening of one
 *   claim that starts behind the header.
 * hg_claims_open_folded_bn254 / hg_claims_verify_folded_bn254 / hg_claims_verify_folded_device_bn254: the same under the mapping and
 *   the -1 cases of hg_claims_open_bn254 / hg_claims_verify_bn254, on an hg_input_claim_bn254 array as hg_verify_public_bn254 returns it. */
int hg_pcs_open_folded_bn254(hg_ctx* ctx, const void* commitment, const uint32_t* table, const uint64_t* points4, const uint64_t* values4,
                             size_t n_claims, size_t n_queries, uint8_t* proof, size_t cap, size_t* len);
int hg_pcs_verify_folded_bn254(const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table,
                               const uint64_t* points4, const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len);
int hg_pcs_verify_folded_device_bn254(hg_ctx* ctx, const uint8_t root[32], const uint32_t* nvars, size_t n_tables, size_t log2_row, const uint32_t* table,
                                      const uint64_t* points4, const uint64_t* values4, size_t n_claims, size_t n_queries, const uint8_t* proof, size_t len);
int hg_claims_open_folded_bn254(hg_ctx* ctx, const hg_params* params, const void* commitment, const void* claims, size_t n, const uint64_t* points4,
                                size_t n_queries, uint8_t* opening, size_t cap, size_t* len);
int hg_claims_verify_folded_bn254(const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n,
                                  const uint64_t* points4, size_t n_queries, const uint8_t* opening, size_t len);
int hg_claims_verify_folded_device_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t root[32], size_t log2_row, const void* claims, size_t n,
                                         const uint64_t* points4, size_t n_queries, const uint8_t* opening, size_t len);

/* hg_pcs_open_folded_batch_bn254 / hg_claims_open_folded_batch_bn254: hg_pcs_open_folded_bn254 / hg_claims_open_folded_bn254 for a run,
 *   with the argument lists and the outputs of hg_pcs_open_batch_bn254 / hg_claims_open_batch_bn254 (declared with the BN254 batch
 *   forms of commit and open, below). Item i opens its own claims, n_claims[i] >= 1, against commitments[i]; all handles are BN254
 *   device handles of this context and of one shape, a handle may appear twice; one n_queries for the run. Opening i is byte for byte
 *   what hg_pcs_open_folded_bn254 returns for that item alone - so also what the host form gives on a host commitment of the same
 *   tables. n == 0 returns 0 and writes nothing.
 *   status[i] = 0 opened; 1 REFUSED: lens[i] = 0, the item's buffer untouched, the reason slot holds exactly the text
 *   hg_pcs_open_folded_bn254 (hg_claims_open_folded_bn254) leaves for that item, the single entry's name and the lowest failing claim.
 *   The run continues after a refusal and the other items' bytes are what they would be without the refused item. Returns the number
 *   of refused items.
 *   -1, nothing written, the text beginning with this function's name and giving "index i" where an item is at fault, every item
 *   checked before anything is enqueued: the cases of hg_pcs_open_batch_bn254 (a Goldilocks handle: "the commitment is over
 *   Goldilocks: open it with <this function without _bn254>"), and an item without a claim ("<function>: index i: a folded opening
 *   needs a claim"); "<function>: no context" after the argument checks; cap_each below the folded length (the text gives the bytes
 *   needed).
 *   The pass is hg_pcs_open_folded_batch's, one host flow for both fields: groups of at most 64 or "verify_batch_group" members
 *   within 2 GiB of scratch - a member takes its g (32 bytes a table entry), the two buffer pairs of the rounds (48 bytes a table
 *   entry), its staged claims and its image: about 149 MB at n=32768 k=16, 14 members a group (a run of 64 ran as 5 groups:
 *   DESIGN.md 6; "the context's arena cannot hold a group of G reductions: lower verify_batch_group" when the arena is smaller). Per group the host threads start every
 *   member's transcript and write its claim rows and factor tables into one staged copy, one member a task; one launch builds all
 *   members' g and copies the elements of one-element tables to the scalars; then every step of the reduction is ONE launch over all
 *   members (the member is the grid's third dimension; its raw rows through a table of G pointers, the 64 fold constants of its
 *   challenge - 256 bytes, computed by the host - from an array of G sets that is uploaded once a round and read at the member's
 *   index, which is uniform over a wavefront, so the constants stay in scalar registers), one workgroup a member adds its partial
 *   sums, the 3 G sums and the scalars of the tables that retire come back in one copy each, canonical, and ONE synchronisation
 *   serves the group: V + 1 launches of the round kernels and V + 1 synchronisations a group, whatever its size. The single call runs
 *   the same kernels as a group of one, with its row base and its fold constants in the kernel arguments. A member whose running
 *   claim is not met is refused; it rides on in the launches, its results ignored (its buffers are its own; raw rows are never
 *   written). The lowest failing claim of the refused members comes from the combine and evaluation kernels of
 *   hg_pcs_open_batch_bn254 over their claims, one cell a member; a refused member of which no claim fails is -1 (internal). u_0 and
 *   u_1 are two jobs a member through the combine kernel, the u vectors come back (128 KB a member where the unfolded batch hashes
 *   3.1 MB), the host threads hash them and squeeze the indices, the gather writes the columns into images whose body starts behind
 *   the header; the host writes header, u vectors and siblings. Profiler class pcs_fold_batch_bn254; HG_TIMES=pcs prints a line a
 *   group; HG_DEBUG=plan prints "[hg plan] bnpcsfoldb members=.. V=.. round_launches=.. round_syncs=.. tables=.. claims=.." a group.
 *   HG_PCS_FOLD_BLOCKS bounds the workgroups of a launch as a whole; a table of a member always has at least one. Not concurrently
 *   with another call on the same context.
 * hg_pcs_verify_folded_device_batch_bn254 / hg_claims_verify_folded_batch_bn254: hg_pcs_verify_folded_device_bn254 /
 *   hg_claims_verify_folded_device_bn254 for a run, with the argument lists and the outputs of hg_pcs_verify_device_batch_bn254 /
 *   hg_claims_verify_batch_bn254. results[i] and the reason are exactly what hg_pcs_verify_folded_device_bn254 (so
 *   hg_pcs_verify_folded_bn254) gives for that item alone, also where several checks fail at once; byte offsets count from the start
 *   of the item's folded opening; a wrong length is rejected per item and never reaches the device. The order of reasons is the
 *   single call's: the length; a header element that is not below r (host); a body element that is not below r; the header's rounds
 *   and final evaluation; the body's checks. Returns the number of rejected items. -1 as hg_pcs_verify_device_batch_bn254, and in
 *   hg_pcs_verify_folded_device_batch_bn254 an item with n_claims[i] == 0 ("<function>: index i: a folded opening needs a claim").
 *   THE ONE EXCEPTION: hg_claims_verify_folded_batch_bn254 gives an item with n_claims[i] == 0 - a proof the public batch verifier
 *   rejected - results[i] = 1 with the reason "hg_claims_verify_folded_batch_bn254: a folded opening needs a claim", so that a
 *   service can pass the arrays of hg_verify_public_batch_bn254 through unchanged; such an item never reaches the device.
 *   The pass is hg_pcs_verify_device_batch_bn254's: per group the host threads run the header of every member and write its block of
 *   the staged copy as that of an opening of one claim that starts behind the header - what hg_pcs_verify_folded_device_bn254
 *   writes for its one member; the index-free kernels run once over the group, the host threads hash each member's 2 C elements of u
 *   meanwhile, one copy of indices, the query kernel, the cells back: one synchronisation a group. A member whose header holds an
 *   element that is not below r rides along on a block of zeros and gets the header's reason. No kernel of its own. Profiler class
 *   pcs_bn254_verify_batch. */
int hg_pcs_open_folded_batch_bn254(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points4,
                                   const uint64_t* const* values4, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings,
                                   size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap);
int hg_claims_open_folded_batch_bn254(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each,
                                      const uint64_t* points4, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n,
                                      uint8_t* openings, size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap);
int hg_pcs_verify_folded_device_batch_bn254(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row,
                                            const uint32_t* const* tables, const uint64_t* const* points4, const uint64_t* const* values4,
                                            const size_t* n_claims, size_t n_queries, const uint8_t* const* proofs, const size_t* lens, size_t n,
                                            int* results, char* reasons, size_t reason_cap);
int hg_claims_verify_folded_batch_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims,
                                        size_t claim_cap_each, const uint64_t* points4, size_t coord_cap_each, const size_t* n_claims,
                                        size_t n_queries, const uint8_t* const* openings, const size_t* lens, size_t n, int* results, char* reasons,
                                        size_t reason_cap);

/* hg_pcs_verify_device_batch_bn254 / hg_claims_verify_batch_bn254: hg_pcs_verify_device_batch / hg_claims_verify_batch over bn256::Fr,
 *   the same contract word for word with a coordinate or value of 4 canonical limbs: a run of n openings of ONE shape and one
 *   n_queries, item i with its own root, claims (0 allowed) and opening; results[i] and the reason slot at reasons + i*reason_cap
 *   (reasons may be NULL) are exactly what hg_pcs_verify_device_bn254 - so hg_pcs_verify_bn254 - gives for that item alone, also
 *   where several checks fail at once and for a wrong length, which is rejected per item and never reaches the device; byte offsets
 *   in reasons count from the item's own opening. Returns the number of rejected items; n == 0 returns 0 and writes nothing.
 *   claims is an hg_input_claim_bn254 array and points4 is laid out exactly as hg_verify_public_batch_bn254 writes them: item i's
 *   claims at (hg_input_claim_bn254*)claims + i*claim_cap_each, its points at points4 + 4*i*coord_cap_each with point_off relative
 *   to its own block.
 *   The pass is the Goldilocks one over 32-byte elements: groups of at most 64 or "verify_batch_group" members, the 2 GiB budget (a
 *   member takes about 45 MB at n=32768 k=16, so 64 of them run as groups of 47 and 17), the 65535 transforms the batched Fr NTT takes at
 *   once and the threads of one launch of the inner products; the kernels of hg_pcs_verify_device_bn254 once over all members,
 *   the inner products with one job per workgroup; one synchronisation a group.
 *   -1 (nothing is written; hg_last_error begins with the function's name and gives "index i" where an item is at fault; every
 *   item is checked before anything is enqueued): the cases of the Goldilocks pair, with an element that is not below r in place
 *   of a word that is not below p, and "<function>: no context" for a null context, after the argument checks. */
int hg_pcs_verify_device_batch_bn254(hg_ctx* ctx, const uint8_t* const* roots, const uint32_t* nvars, size_t n_tables, size_t log2_row,
                                     const uint32_t* const* tables, const uint64_t* const* points4, const uint64_t* const* values4,
                                     const size_t* n_claims, size_t n_queries, const uint8_t* const* proofs, const size_t* lens, size_t n,
                                     int* results, char* reasons, size_t reason_cap);
int hg_claims_verify_batch_bn254(hg_ctx* ctx, const hg_params* params, const uint8_t* const* roots, size_t log2_row, const void* claims,
                                 size_t claim_cap_each, const uint64_t* points4, size_t coord_cap_each, const size_t* n_claims, size_t n_queries,
                                 const uint8_t* const* openings, const size_t* lens, size_t n, int* results, char* reasons, size_t reason_cap);

/* hg_pcs_commit_batch_bn254 / hg_secrets_commit_batch_bn254 / hg_pcs_open_batch_bn254 / hg_claims_open_batch_bn254: hg_pcs_commit_batch,
 *   hg_secrets_commit_batch, hg_pcs_open_batch and hg_claims_open_batch over bn256::Fr, each with the argument list of its Goldilocks
 *   sibling and its contract word for word, Fr standing for the Goldilocks field: tables4, points4 and values4 hold 4 canonical
 *   little-endian words an element, claims is an hg_input_claim_bn254 array and points4 is laid out exactly as
 *   hg_verify_public_batch_bn254 writes them (item i's claims at (hg_input_claim_bn254*)claims + i*claim_cap_each, its points at
 *   points4 + 4*i*coord_cap_each with point_off relative to its own block). Device only. Every handle is byte for byte what
 *   hg_pcs_commit_bn254 / hg_secrets_commit_bn254 on the same context gives for that member alone (the same root, tree and matrices;
 *   hg_pcs_open_bn254, hg_claims_open_bn254, the open batch and hg_pcs_free take it), except that a group's matrices share one
 *   allocation: THE MEMORY RETURNS WHEN THE LAST HANDLE OF THE GROUP IS FREED. Every opening is byte for byte what hg_pcs_open_bn254 /
 *   hg_claims_open_bn254 gives for that item alone; the open pair also takes the handles of hg_prove_encryptions_committed_bn254,
 *   mixed with the others in one call. The commit pair returns 0, the open pair the number of refused items; n == 0
 *   returns 0 and writes nothing. What differs from the Goldilocks contract:
 *   - a refused open item (status[i] = 1, lens[i] = 0, its buffer untouched) carries the text hg_pcs_open_bn254 / hg_claims_open_bn254
 *     leaves in hg_last_error for it, the lowest failing claim;
 *   - a member whose table holds an element that is not below r (all four limbs compared) is named as "<entry>: index i: a table holds
 *     an element that is not below r", the lowest such member; hg_secrets_commit_batch_bn254 lifts the 8-byte witness words into Fr on
 *     the device by the signed rule of hg_secrets_commit_bn254, so a quarter of the bytes is uploaded;
 *   - a Goldilocks handle is refused with "the commitment is over Goldilocks: open it with hg_pcs_open_batch" (hg_claims_open_batch
 *     for the wrapper).
 *   The commit pass: groups of at most 64 or "verify_batch_group" members, a byte budget of its own over the members' raw and encoded
 *   rows (4.25 GiB; a member takes 283 MB at n=32768 k=16: 16 members a group) and the 65535 rows the batched Fr NTT takes at once. A
 *   group's rows lie in one allocation. An allocation of gigabytes costs between 0.3 ms and 1.4 s on the device, so the context
 *   KEEPS the allocations of groups whose handles were all freed, up to 4.25 GiB in all (the oldest goes first), and the next group
 *   takes one that holds it and is at most twice as large; hg_destroy frees them, and a handle may still be freed after it. Staging with the range check (one flag a member), the encoding in slices of whole members
 *   through one slice's NTT temporary (so the temporary does not grow with the group), the leaf sponges (one thread per member and
 *   column) and the tree levels of the Goldilocks batch (a node is 32 bytes in either field) each run once over the group; one
 *   download, one synchronisation a group.
 *   The open pass is hg_pcs_open_batch's step for step over 32-byte elements: the weights in Montgomery form, the row combinations on
 *   the deferred-reduction accumulators with one job per workgroup (their weights are wave-uniform scalar operands), elements
 *   written into the images as 32 bytes big-endian; two synchronisations a group.
 *   -1 (nothing is written; hg_last_error begins with the function's name and gives "index i" where a member or item is at fault):
 *   the cases of the Goldilocks entries, "<function>: no context" for a null context after the argument checks. */
int hg_pcs_commit_batch_bn254(hg_ctx* ctx, const uint64_t* const* const* tables4, const uint32_t* nvars, size_t n_tables, size_t log2_row, size_t n,
                              void** commitments, uint8_t* roots);
int hg_secrets_commit_batch_bn254(hg_ctx* ctx, const hg_params* params, const hg_witness* const* ws, size_t n, size_t log2_row, void** commitments,
                                  uint8_t* roots);
int hg_pcs_open_batch_bn254(hg_ctx* ctx, const void* const* commitments, const uint32_t* const* tables, const uint64_t* const* points4,
                            const uint64_t* const* values4, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings, size_t cap_each,
                            size_t* lens, int* status, char* reasons, size_t reason_cap);
int hg_claims_open_batch_bn254(hg_ctx* ctx, const hg_params* params, const void* const* commitments, const void* claims, size_t claim_cap_each,
                               const uint64_t* points4, size_t coord_cap_each, const size_t* n_claims, size_t n_queries, size_t n, uint8_t* openings,
                               size_t cap_each, size_t* lens, int* status, char* reasons, size_t reason_cap);

/* hg_witness_derive and hg_prove_bn254 for a run of n_enc ENCRYPTIONS under one key, pipelined: hg_prove_encryptions over bn256::Fr
 *   [REF scripts/circuit_sk.py:18-140 followed by sk_encryption_circuit.rs:417-460, 614-626; the loop a proving service writes around
 *   them - the reference has no batch entry]. The contract is that of hg_prove_encryptions: s[i], e[i], k1[i] (n each) and a[i] (k*n)
 *   are the signed ascending polynomials of hg_encryption_layout and cross the bus as they are ((3+k) n words); one kernel lays the
 *   tables out on the device and checks every coefficient, the derivation writes r1is, r2is and ct0is beside them, one launch lifts
 *   all of them into Fr and the circuit is evaluated over Fr - all of it for encryption i+1 on a stream of its own, into a second
 *   set of node tables, while encryption i is proven; no table visits the host on the way to the prover. Proof i is written at
 *   proofs + i*cap_each (32-byte big-endian elements), its length to lens[i], and is byte-identical to hg_prove_bn254 of
 *   hg_witness_derive of the laid-out inputs. ws (may be NULL): ws[i] = the handle hg_witness_derive would return (all seven tables;
 *   the caller frees it), usable with hg_verify_bn254 and hg_verify_device[_batch]_bn254.
 *   status[i] = 0 proven, 1 REFUSED (a check of hg_witness_derive failed); a refused encryption is never proven: lens[i] = 0,
 *   ws[i] = NULL, no proof bytes; reasons (may be NULL) receives at reasons + i*reason_cap the text that names table, modulus and
 *   cause, NUL-terminated and truncated to reason_cap bytes ("" when proven). The run continues; the other proofs are what they would
 *   be without the refused item.
 *   Returns the number of refused encryptions (>= 0; n_enc == 0 returns 0), or -1 on an error of the call: a null argument, no
 *   context, a host-only key, a proof larger than cap_each, parameters the derivation cannot serve, a key with a gate constant that
 *   is not below 2^63 (it could not be lifted into Fr). hg_last_error names the function and, where it applies, the index.
 *   timings (may be NULL): total_ms = wall clock of the run; prove_ms = sum of the proving spans of the proven items (wall clock,
 *   from the first launch of a prove to its replayed transcript); witness_ms = sum over the proven items of the device time of
 *   upload + derivation + lift + evaluation (HIP events on the stream they run on). upload_ms, gpu_ms, enqueue_ms, sync_ms and
 *   replay_ms have no meaning on this path and are 0.
 * hg_prove_encryptions_committed_bn254: hg_prove_encryptions_bn254 that also commits to every item's secret inputs, inside the
 *   pipeline - hg_prove_encryptions_committed over bn256::Fr, with its argument list. Everything hg_prove_encryptions_bn254 does and
 *   returns, with its checks in its order under this function's name (a refusal's text reads
 *   "hg_prove_encryptions_committed_bn254: encryption i: .."); proof i is byte-identical to hg_prove_encryptions_bn254's.
 *   commitments and roots are required when n_enc > 0: commitments[i] is a BN254 device handle of ctx (hg_claims_open_bn254,
 *   hg_claims_open_batch_bn254, hg_pcs_open_bn254, hg_pcs_open_batch_bn254 and hg_pcs_free take it); its root, the 32 bytes at
 *   roots + 32 i, and every opening made from it are byte for byte those of the host form hg_secrets_commit_bn254(NULL, params, w_i,
 *   log2_row, ..) on the witness hg_witness_derive gives for item i: the tables in the order of hg_secrets_commit, the words lifted
 *   by the signed rule of hg_secrets_commit_bn254. A refused item gets commitments[i] = NULL and 32 zero bytes. ws may be NULL, and
 *   the entry is made to be called that way: then no table visits the host.
 *   The commit of item i starts from the laid-out u64 tables of its table set in HBM: one kernel reads every word once, lifts it and
 *   writes the canonical 32-byte element into the handle's raw row and into the zero-padded row to encode (8 bytes in and 160 out an
 *   element); the batched Fr NTT, the leaf sponges and the tree follow as in hg_pcs_commit_bn254: nothing crosses the bus but the
 *   tree. It is enqueued on the feed stream behind the item's node tables, so it runs under the prove of the item before (and of
 *   item i) and delays neither the event that prove i waits for nor the flag words; the refill of the set two items later is behind
 *   it on the same stream. The tree and the flag word come back on the copy stream into page-locked staging, one per set, and
 *   enter the handle once prove i has completed. The commit of an item is enqueued before it is known whether the item is refused;
 *   a refused item's slot is written again by the next item. The Montgomery-form twiddles, the NTT temporary (rows x code length
 *   elements: 227 MB at n=32768 k=16) and the two tree buffers belong to the pipeline, not to the arena (every BN254 prove resets
 *   it); they are sized for the shape in use and rebuilt when it changes. The raw and encoded rows of the items lie in group
 *   allocations, cut as hg_pcs_commit_batch_bn254 cuts its groups - at most 64 items, "verify_batch_group", its 4.25 GiB budget -
 *   and taken when a group's first item is filled, from the allocations the context keeps of freed groups where one fits; the
 *   group's handles share it: THE MEMORY RETURNS WHEN THE LAST HANDLE OF THE GROUP IS FREED (to the context, as for the batch entries).
 *   All commitments[i] are NULL at entry, as ws[i]. Returns the number of refused encryptions (n_enc == 0 returns 0) or -1, after
 *   which no handle is alive, in this order: the errors of hg_prove_encryptions_bn254 (commitments and roots count among the null
 *   arguments); then, ahead of anything enqueued, the log2_row errors of hg_pcs_commit for the shape of the secrets (outside the
 *   limits, above the smallest table) and ".. more than 65535 rows (choose a larger log2_row)" (the batched Fr NTT takes so many
 *   at once); during the run a derived word that is not below the Goldilocks p (".. encryption i: a derived table holds a word
 *   that is not below p"; the signed lift is only defined for such words), which a correct derivation never gives.
 *   timings: the fields of hg_prove_encryptions_bn254; witness_ms includes the commits' device time; upload_ms = the sum over the
 *   proven items of the commit's device time alone (HIP events on the stream it runs on). */
int hg_prove_encryptions_bn254(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                               const int64_t* const* a, size_t n_enc, uint8_t* proofs, size_t cap_each, size_t* lens, int* status,
                               hg_witness** ws, char* reasons, size_t reason_cap, hg_timings* timings);
int hg_prove_encryptions_committed_bn254(hg_ctx* ctx, const hg_pk* pk, const int64_t* const* s, const int64_t* const* e, const int64_t* const* k1,
                                         const int64_t* const* a, size_t n_enc, size_t log2_row, uint8_t* proofs, size_t cap_each, size_t* lens,
                                         int* status, void** commitments, uint8_t* roots, hg_witness** ws, char* reasons, size_t reason_cap,
                                         hg_timings* timings);

/* profiling: level 0 off, 1 = events around the selected kernel class only, 2 = every class */
int hg_profile(hg_ctx* ctx, int level);
/* selects the class that level 1 times (a name hg_profile_get reported); returns 0, or -1 if there is no such class */
int hg_profile_select(hg_ctx* ctx, const char* name);
int hg_profile_reset(hg_ctx* ctx);
int hg_profile_get(hg_ctx* ctx, hg_kernel_stat* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
