// The polynomial commitment of pcs.hpp over bn256::Fr (F = E = Fr): what opens the claims hg_verify_public_bn254 leaves on the secret
// inputs. Same scheme, shape rules and limits; an element is 32 bytes. What differs (include/hg.h states it in full): the code is
// the Fr NTT of size 4C with the root of hg_ntt_bn254; a leaf hashes LE64(0) and the 32-byte little-endian canonical elements of a
// column; the transcript starts as "hg-pcs-bn254-1", absorbs elements as those 32 bytes, and a challenge is LE(hash) mod r (the rule
// of hg_challenges_bn254 over the absorbed bytes), one element for rho; elements cross the opening as 32 bytes big-endian.
//
// A handle is the pcs::Commitment of pcs.hpp with field == BN254: rows, M, d_rows, d_M hold 4 canonical (non-Montgomery) words an
// element, so the leaf hash and the column gather read them as they are. Weights (powers of rho, eq tables) are in Montgomery
// form, so a Montgomery product weight x element is the plain product.
#pragma once
#include "pcs.hpp"
#include "bn254_field.hpp"

namespace hg {
namespace bn {

inline size_t pcs_opening_bytes(const pcs::Shape& sh, size_t n_claims, size_t Q) { return 32 * sh.C() * (n_claims + 1) + Q * (32 * sh.R + 32 * (size_t)sh.depth()); }

struct PcsClaim { size_t table; std::vector<Fr> point; Fr value; };   // canonical elements

// `who`: the entry point an Error names. words == false: tables[t] = 2^{v_t} elements of 4 canonical words (an element that is not
// below r is an Error); words == true: tables[t] = 2^{v_t} witness words, lifted by the signed rule of fr_lift_signed (a word below
// 2^63 is itself, any other is r - (p_goldilocks - word)) - on the device by a kernel, so a quarter of the bytes is uploaded.
pcs::Commitment* pcs_commit_host(const char* who, const pcs::Shape& sh, const u64* const* tables, bool words);
// bn254_pcs.inc (part of bn254.hip): rows staged, encoded by the batched NTT, hashed, the tree by the kernels of pcs.hip; one synchronisation
pcs::Commitment* pcs_commit_device(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tables, bool words);
// hg_pcs_commit_batch_bn254 (bn254_pcs.inc): n members of one shape, tables[i * m + t] = table t of member i (`words` as above), in
// device passes of a group of members each: every handle is what pcs_commit_device gives for that member, except that a group's
// matrices share one allocation (pcs::Commitment::owner). A group is cut by the option verify_batch_group, VB_PCS_COMMIT_BUDGET_BN254
// over the members' raw and encoded rows and the 65535 rows of ntt_batch_dev; the NTT temporary is one slice's. Throws an Error
// naming `who` (and "index i" for a member's element that is not below r); no handle survives an error
std::vector<pcs::Commitment*> pcs_commit_device_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const u64* const* tables, size_t n, bool words);

// One row combination of an opening: u[j] = sum_{r < nrows} w[r] * row_{row0 + r}[j]; w in Montgomery form, u canonical
struct PcsJob { size_t row0, nrows; std::vector<Fr> w; };
void pcs_combine_host(const pcs::Commitment& cm, const std::vector<PcsJob>& jobs, Fr* u);        // u: jobs.size() x C
void pcs_columns_host(const pcs::Commitment& cm, const std::vector<size_t>& js, Fr* cols);       // cols: js.size() x R
void pcs_combine_device(const pcs::Commitment& cm, const std::vector<PcsJob>& jobs, Fr* u);
void pcs_columns_device(const pcs::Commitment& cm, const std::vector<size_t>& js, Fr* cols);

// hg_pcs_open_bn254: the opening bytes; an Error (naming `who` and the claim) if a value is not <u_i, eq(z_i[..c])>. Transcript and
// byte layout are here for both forms: device bytes equal host bytes by construction
std::vector<uint8_t> pcs_open(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& claims, size_t Q);
// hg_pcs_open_batch_bn254 (bn254_pcs.inc): item i's claims opened against its own device commitment (one shape, one context, one Q)
// in device passes of a group of items each. refused: a value is not the evaluation (reason = pcs_open's error text under the name
// `single`, the lowest failing claim; bytes empty); else bytes = what pcs_open gives for the item alone. Throws an Error naming `who`
struct PcsOpenItem { const pcs::Commitment* cm; const std::vector<PcsClaim>* claims; };
std::vector<pcs::Opened> pcs_open_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q);
// hg_pcs_verify_bn254: "" = accepted, else the reason (the strings and the order of pcs::verify)
std::string pcs_verify(const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len);
// hg_pcs_verify_device_bn254 (bn254_pcs.inc): the same decision and the same reason with the table-sized work on the context's
// stream; the Fiat-Shamir hash over the u_i stays on the host and runs beside the kernels. Throws an Error if the arena cannot hold
// the opening
std::string pcs_verify_device(hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len);
// hg_pcs_verify_device_batch_bn254 (bn254_pcs.inc): a run of openings of one shape and one Q, each with its own root and claims, in
// device passes of a group of openings each; why[i] is what pcs_verify_device returns for item i alone. Throws an Error naming
// `who` if the arena cannot hold a group
struct VerifyItem { const uint8_t* root; const std::vector<PcsClaim>* claims; const uint8_t* proof; size_t len; };
std::vector<std::string> pcs_verify_device_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<VerifyItem>& items, size_t Q);

// ---- folded openings (hg.h "Folded openings over BN254"): the folded openings of pcs.hpp with F = E = Fr. The header is 3 coefficients a
// round, V = max_t v_t rounds, then the m values Y_t, 32 bytes big-endian each; the body is that of an opening of one claim.
inline size_t pcs_folded_header_bytes(const pcs::Shape& sh) { return 32 * (3 * pcs::fold_rounds(sh) + sh.nvars.size()); }
inline size_t pcs_folded_opening_bytes(const pcs::Shape& sh, size_t Q) { return pcs_folded_header_bytes(sh) + pcs_opening_bytes(sh, 1, Q); }
// The prover's side of the reduction: pcs::FoldSource over Fr. r is the canonical challenge of round j - 1; T[t] (plain) and G[t]
// (Montgomery form) are canonical once table t has retired; s = the three sums as plain canonical elements
struct PcsFoldSource {
    std::vector<Fr> T, G;
    virtual void step(size_t j, const Fr& r, Fr s[3]) = 0;
    virtual ~PcsFoldSource() {}
};
// bpow[i] = beta^i in Montgomery form. The host form reads cm.rows; the device form (bn254_pcs.inc) builds g and runs every round on the
// context's stream (`who` names the entry in the texts of its device calls)
std::unique_ptr<PcsFoldSource> pcs_fold_source_host(const pcs::Commitment& cm, const std::vector<PcsClaim>& claims, const std::vector<Fr>& bpow);
std::unique_ptr<PcsFoldSource> pcs_fold_source_device(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& claims, const std::vector<Fr>& bpow);
// The prover's arithmetic of one reduction, which pcs_open_folded and the batch form (bn254_pcs.inc) share: pcs::FoldProver over Fr. The
// transcript, the running claim (plain) and the factors prod (1 - r_j') of the retired tables (Montgomery form). T, G are a
// PcsFoldSource's, or what a group pass brought back for the member.
struct PcsFoldProver {
    FsTranscript tr;
    std::vector<Fr> bpow, tail, rho;   // bpow, tail in Montgomery form; rho canonical
    Fr claim, r;                       // r: the canonical challenge the next step folds by (zero ahead of round 0)
    PcsFoldProver(const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q);
    // round j < V from the sums of step(j): false, with nothing written, if they do not meet the running claim (a value is wrong); else
    // c0, c1, c2 are written and r = rho[j] is squeezed
    bool round(const pcs::Shape& sh, size_t j, const Fr s[3], const std::vector<Fr>& T, const std::vector<Fr>& G);
    // after step(V): false if the final evaluation misses the claim; else the Y_t are written
    bool finish(const pcs::Shape& sh, const std::vector<Fr>& T, const std::vector<Fr>& G);
    // delta and rho' squeezed -> the two row combinations of the body: the R powers of rho', the combined weights
    std::vector<PcsJob> body_jobs(const pcs::Shape& sh);
    // the u vectors (canonical) behind the header and into the transcript
    void write_u(const Fr* u, size_t n);
};
// hg_pcs_open_folded_bn254: the opening bytes; an Error naming `who` if there is no claim and - naming the lowest failing claim - if a
// value is not its table's evaluation
std::vector<uint8_t> pcs_open_folded(const char* who, const pcs::Commitment& cm, const std::vector<PcsClaim>& claims, size_t Q);
// hg_pcs_open_folded_batch_bn254 (bn254_pcs.inc): pcs_open_device_batch for folded openings (every item has a claim): a group's reductions
// run as one launch a round over all members, with one synchronisation a round. refused / bytes as there, the reason is
// pcs_open_folded's under `single`
std::vector<pcs::Opened> pcs_open_folded_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<PcsOpenItem>& items, size_t Q);
// hg_pcs_verify_folded_device_batch_bn254 (bn254_pcs.inc): pcs_verify_device_batch for folded openings: why[i] is what
// pcs_verify_folded_device returns for item i alone; the headers on the host threads, the bodies through pcs_verify_device_batch's pass
// as openings of one claim
std::vector<std::string> pcs_verify_folded_device_batch(const char* who, hg_ctx* ctx, const pcs::Shape& sh, const std::vector<VerifyItem>& items, size_t Q);
// hg_pcs_verify_folded_bn254: "" = accepted, else the reason
std::string pcs_verify_folded(const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len);
// hg_pcs_verify_folded_device_bn254 (bn254_pcs.inc): the same decision and reason; the header on the host, the body through
// pcs_verify_device's kernels
std::string pcs_verify_folded_device(hg_ctx* ctx, const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof, size_t len);
// What the two folded verifiers share (pcs::FoldedHeader over Fr): rho_pw and w in Montgomery form, lo and y canonical
struct PcsFoldedHeader {
    size_t noncanonical = ~(size_t)0;
    std::string reason;
    FsTranscript tr;
    std::vector<Fr> rho_pw, w, lo;
    Fr y;
};
PcsFoldedHeader pcs_folded_header(const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const uint8_t* proof);

// ---- what the opening and both forms of the verifier share (pcs_bn254.cpp): the transcript up to the column indices, the weights
// tag: "hg-pcs-bn254-1", or "hg-pcs-bn254-fold-1" for a folded opening
FsTranscript pcs_start_transcript(const pcs::Shape& sh, const uint8_t root[32], const std::vector<PcsClaim>& claims, size_t Q, const char* tag = "hg-pcs-bn254-1");
Fr pcs_squeeze(FsTranscript& tr);                                                    // a challenge, canonical (rho is the first)
std::vector<Fr> pcs_rho_powers(const Fr& rho_canon, size_t R);                       // rho^r, r < R, Montgomery form
void pcs_absorb(FsTranscript& tr, const Fr* x, size_t count);                        // canonical elements as their 32 bytes
std::vector<size_t> pcs_squeeze_indices(FsTranscript& tr, size_t N, size_t Q);       // j_q = a squeezed element's low word & (N - 1)
std::vector<Fr> pcs_eq_table(const Fr* pt_canon, size_t n);                          // Montgomery form; coordinate i belongs to bit i
Fr pcs_read_be32(const uint8_t* p);                                                  // an element of the opening as it is read

// the signed lift of a witness word, canonical (host side of fr_lift_signed)
BN_HD Fr fr_lift_signed_canon(u64 v) { return v < (1ULL << 63) ? fr_make(v, 0, 0, 0) : fr_sub(fr_zero(), fr_make(0xFFFFFFFF00000001ULL - v, 0, 0, 0)); }

// bn254.hip: `batch` transforms of size 2^log2n in place on device pointers, natural order in and out, through tmp (same size).
// W[i] = w^i in Montgomery form, i < 2^log2n. 8 <= log2n <= 16: the four-step LDS kernels (batch <= 65535, the grid's y), any other
// size: bit reversal and radix-2 stages. scale (null: none) is multiplied on by a Montgomery product on the way out. The transform
// is linear and every twiddle product is a Montgomery product with a Montgomery-form power of w, so elements keep the form they
// came in: Montgomery in, Montgomery out; canonical plain words in, canonical plain words out.
void ntt_batch_dev(hipStream_t st, Fr* a, Fr* tmp, const Fr* W, int log2n, size_t batch, const Fr* scale);

// bn254_pcs.inc: pcs::commit_tables_enqueue over Fr - the whole commit of pcs_commit_device(.., words = true) to m tables of witness
// words that lie in HBM (d_tables[t]: table t, 2^{v_t} words, 16-byte aligned), enqueued on st: nothing is synchronised and the
// context's arena is not touched. The caller supplies d_rows (R C elements), d_M (R N), the NTT temporary (R N), W (N: filled here
// with the Montgomery-form powers of the root), the tree buffer (8 N words: the levels one behind the other) and one flag word,
// which is set if a word is not below the Goldilocks p (the signed lift is defined for such words only). One kernel,
// k_bnpcs_stage_words, reads every word once, lifts it and writes the raw row and the zero-padded row of M. Needs c >= 1 and
// R <= 65535 (ntt_batch_dev)
void pcs_commit_words_enqueue(hipStream_t st, const pcs::Shape& sh, const u64* const* d_tables, Fr* d_rows, Fr* d_M, Fr* tmp, Fr* W, u64* d_tree, unsigned* d_flag);

}  // namespace bn
}  // namespace hg
