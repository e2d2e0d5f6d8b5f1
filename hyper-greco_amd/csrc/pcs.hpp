// Multilinear polynomial commitment of the Brakedown / Ligero shape over Goldilocks: the layer that opens the claims
// hg_verify_public leaves on the secret inputs. The reference names MultilinearBrakedown<F, Keccak256, BrakedownSpec6> as its Pcs type
// parameter [REF bfv-gkr/src/sk_encryption_circuit.rs:543-550] and never uses it. What differs here: the linear code
// is Reed-Solomon of rate 1/4 (the forward NTT of the zero-padded row: Goldilocks has the two-adicity, Brakedown's argument only
// needs linearity), not the expander code of BrakedownSpec6; and evaluation points are E = GoldilocksExt2 points.
//
// Scheme (include/hg.h states it in full). Tables T_0 .. T_{m-1} of 2^{v_t} canonical words are cut into rows of C = 2^c words
// and stacked in table order (R rows, off_t = first row of table t). Enc(row) = NTT_{4C}(row || 0). Leaf j of the Keccak-256
// Merkle tree hashes LE64(0) || column j of the encoded matrix; an inner node hashes LE64(1) || left || right. An opening of n
// claims carries u_0 = sum_r rho^r row_r, u_i = sum_r eq(z_i[c..])[r] row_{off_t + r} and Q opened columns with their paths.
#pragma once
#include <memory>
#include <string>
#include <vector>
#include "host.hpp"

struct hg_ctx;

namespace hg {
namespace pcs {

constexpr int MAX_TABLES = 64, MAX_NVARS = 30, MAX_LOG2_ROW = 24;
constexpr size_t MAX_CLAIMS = 4096, MAX_QUERIES = 65536;
constexpr size_t DEFAULT_QUERIES = 241;   // ceil(100 / log2(4/3)): the (3/4)^Q term at rate 1/4, proximity parameter d/3

struct Shape {
    int c = 0;                   // log2 of the row length
    std::vector<int> nvars;      // v_t
    std::vector<size_t> off;     // first row of table t
    size_t R = 0;                // rows in all
    size_t C() const { return (size_t)1 << c; }
    size_t N() const { return (size_t)4 << c; }   // code length
    int depth() const { return c + 2; }
};
// log2_row == 0 selects min(min_t v_t, ceil(log2(sum_t 2^{v_t}) / 2)); an Error naming `who` for a shape outside the limits above
// or c > v_t
Shape make_shape(const char* who, const uint32_t* nvars, size_t n_tables, size_t log2_row);
inline size_t opening_bytes(const Shape& sh, size_t n_claims, size_t Q) { return 16 * sh.C() * (n_claims + 1) + Q * (8 * sh.R + 32 * (size_t)sh.depth()); }

struct Claim { size_t table; std::vector<E2> point; E2 value; };

// One handle for both forms and both fields. The tree is always on the host: level l (0 = leaves) starts at node 2N - (2N >> l),
// 32 bytes a node.
enum Field { GOLDILOCKS = 0, BN254 = 1 };   // BN254 (pcs_bn254.hpp): an element is 4 canonical little-endian words in rows, M, d_rows, d_M
struct Commitment {
    Field field = GOLDILOCKS;
    Shape sh;
    hg_ctx* ctx = nullptr;          // null: host form
    std::vector<u64> rows, M;       // host form: R x C raw rows, R x 4C encoded rows
    u64* d_rows = nullptr;          // device form: the same two matrices in HBM, owned unless `owner` is set
    u64* d_M = nullptr;
    std::shared_ptr<void> owner;    // a handle of commit_device_batch: d_rows and d_M point into its group's slab, freed with the last handle
    std::vector<uint8_t> tree;
    const uint8_t* root() const { return tree.data() + 32 * (2 * sh.N() - 2); }
    const uint8_t* node(int level, size_t i) const { return tree.data() + 32 * (2 * sh.N() - ((2 * sh.N()) >> level) + i); }
    ~Commitment();
};

// the Keccak-256 calls of the tree
void leaf_hash(const u64* words, size_t R, uint8_t out[32]);                      // Keccak256(LE64(0) || LE64(words[0]) || ...)
void node_hash(const uint8_t* left, const uint8_t* right, uint8_t out[32]);       // Keccak256(LE64(1) || left || right)
std::vector<E2> eq_table(const E2* pt, size_t n);                                 // coordinate i belongs to bit i of the index

// ---- host form (pcs.cpp)
Commitment* commit_host(const Shape& sh, const u64* const* tables);
// ---- device form (pcs.hip): rows staged and encoded in HBM, column hashes and the tree by kernels, one synchronisation
Commitment* commit_device(hg_ctx* ctx, const Shape& sh, const u64* const* tables);
// hg_pcs_commit_batch (pcs.hip): n members of one shape, tables[i * m + t] = table t of member i, in device passes of a group of
// members each: every handle is what commit_device gives for that member, except that a group's matrices share one allocation.
// Throws an Error naming `who` (and "index i" for a member's word that is not below p); no handle survives an error
std::vector<Commitment*> commit_device_batch(const char* who, hg_ctx* ctx, const Shape& sh, const u64* const* tables, size_t n);
// The whole commit to m tables that lie in HBM (d_tables[t]: table t, 2^{v_t} words), enqueued on st: nothing is synchronised and
// the context's arena is not touched. The caller supplies d_rows (R C words), d_M (R N), the NTT scratch (R N), W (N), the tree
// buffer (8 N words: the levels one behind the other) and one flag word, which is set if a word is not below p. Rows of two words or
// more are moved 16 bytes at a time when every table, d_rows and d_M are 16-byte aligned. prof (may be null): the context whose
// profiler class cls the launches are counted in (its prof_stream must be st)
void commit_tables_enqueue(hipStream_t st, const Shape& sh, const u64* const* d_tables, u64* d_rows, u64* d_M, u64* scratch, u64* W, u64* d_tree, unsigned* d_flag,
                           hg_ctx* prof = nullptr, int cls = -1);
// ---- the statement digest on the device (pcs.hip; hg.h states the tree, instance_digest_host is its host form). One kernel hashes
// the leaves of a group of members of one parameter set, one thread per (member, leaf); the levels above are the commitment's
// (merkle_levels_device_batch). A member is where its words lie: compact (an hg_instance as it is uploaded: a[0] = the k n signed
// words of a, ct0 = those of ct0) or laid out (the resident tables of an hg_values: a[i] = input 3+i, ct0 = ct0is).
struct DigestMember { const u64* a[HG_MAX_K]; const u64* ct0; };
struct DigestJob {   // the laid-out digest of one values object beside a commit (commit_device_values): in mem, out digest and flag
    const Params* p;
    DigestMember mem;
    uint8_t digest[32];
    unsigned flag;   // != 0: a word of ais or ct0is is not a signed value in [-(q_i-1)/2, (q_i-1)/2]
};
// Enqueues on st the digests of G members (host copies of their descriptors in mem; staged through the context's pinned buffer into its
// arena, which is not reset) and the copies of the G roots to roots (32 bytes each) and, laid out, of the G flag words to flags
// (flags may be null for compact members). Nothing is synchronised: roots and flags are valid once st has been. The launches are
// counted in the profiler classes instance_digest_leaves and instance_digest_tree (the context's prof_stream is st for their duration).
void instance_digest_enqueue(hg_ctx* ctx, hipStream_t st, const Params& p, bool laid, const DigestMember* mem, size_t G, uint8_t* roots, unsigned* flags);
// The digest of a bound batch (hg_verify_public_bound_batch, hg_instance_digest_group): G members that lie back to back as the batch
// staged them, member m's 2kn signed words at d_set + 2kn m, hashed by k_instance_digest_group - no descriptor table, neither the
// context's arena nor its staging buffer. The caller owns the scratch: d_nodes, instance_digest_group_words(p) words a member (the
// nodes of its blocks of 64 leaves and the levels above them: 8 KB at n=32768 k=16), and h_roots, 32 page-locked bytes a member, valid
// once st has been waited for. Two launches where a member has more than 64 leaves, else one; nothing is synchronised. Counted in the
// profiler class instance_digest_group (the context's prof_stream is st for their duration).
size_t instance_digest_group_words(const Params& p);
void instance_digest_group_enqueue(hg_ctx* ctx, hipStream_t st, const Params& p, const u64* d_set, size_t G, u64* d_nodes, uint8_t* h_roots);
// hg_instance_digest with a context and hg_instance_digest_batch: every instance uploaded as it is, one launch over all of them, one
// synchronisation; out: 32 bytes an instance
void instance_digest_device(hg_ctx* ctx, const Params& p, const std::vector<const Instance*>& insts, uint8_t* out);
// hg_values_instance_digest: the laid-out read; throws if a word is not a signed value in range
void instance_digest_values(hg_ctx* ctx, const Params& p, const DigestMember& mem, uint8_t out[32]);

// hg_secrets_commit_values: commit_tables_enqueue on the context's stream, the scratch from its arena, one synchronisation; the handle
// owns d_rows and d_M. Its errors do not carry a name. dg (hg_prove_committed_mode, may be null): the statement digest of the same
// values object as well, enqueued on the context's second stream beside the commit's kernels and waited for with them; the caller
// reads dg->flag
Commitment* commit_device_values(hg_ctx* ctx, const Shape& sh, const u64* const* d_tables, DigestJob* dg = nullptr);
// an allocation of `bytes` that lives until the last copy of the returned owner is dropped (Commitment::owner of handles whose
// matrices are laid into it by the caller)
std::shared_ptr<void> slab_alloc(size_t bytes, u64** p);
// the levels above the 4C leaf hashes at d_tree (4 words a node, the levels one behind the other), enqueued on st; nodes are 32 bytes
// in either field
void merkle_levels_device(hipStream_t st, u64* d_tree, size_t N);
// the same for the G trees of a group, tree m at d_trees + m tree_words: one launch a level over all members
void merkle_levels_device_batch(hipStream_t st, u64* d_trees, size_t tree_words, size_t N, size_t G);

// One row combination of an opening: u[j] = sum_{r < nrows} w[r] * row_{row0 + r}[j]
struct CombineJob { size_t row0, nrows; std::vector<E2> w; };
void combine_host(const Commitment& cm, const std::vector<CombineJob>& jobs, E2* u);                 // u: jobs.size() x C
void columns_host(const Commitment& cm, const std::vector<size_t>& js, u64* cols);                   // cols: js.size() x R
void combine_device(const Commitment& cm, const std::vector<CombineJob>& jobs, E2* u);
void columns_device(const Commitment& cm, const std::vector<size_t>& js, u64* cols);

// hg_pcs_open: the opening bytes; an Error (naming `who` and the claim) if a value is not <u_i, eq(z_i[..c])>
std::vector<uint8_t> open(const char* who, const Commitment& cm, const std::vector<Claim>& claims, size_t Q);
// hg_pcs_open_batch (pcs.hip): item i's claims opened against its own device commitment (one shape, one context, one Q) in device
// passes of a group of items each. refused: a value is not the evaluation (reason = open's error text under the name `single`, the
// lowest failing claim; bytes empty); else bytes = what open gives for the item alone. Throws an Error naming `who`
struct OpenItem { const Commitment* cm; const std::vector<Claim>* claims; };
struct Opened { bool refused = false; std::string reason; std::vector<uint8_t> bytes; };
std::vector<Opened> open_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<OpenItem>& items, size_t Q);
// hg_pcs_verify: "" = accepted, else the reason
std::string verify(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len);
// hg_pcs_verify_device (pcs.hip): the same decision and the same reason with the table-sized work on the context's stream; the
// Fiat-Shamir hash over the u_i stays on the host and runs beside the kernels. Throws an Error if the arena cannot hold the opening
std::string verify_device(hg_ctx* ctx, const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len);
// hg_pcs_verify_device_batch (pcs.hip): a run of openings of one shape and one Q, each with its own root and claims, in device passes
// of a group of openings each; why[i] is what verify_device returns for item i alone. Throws an Error
// naming `who` if the arena cannot hold a group
struct VerifyItem { const uint8_t* root; const std::vector<Claim>* claims; const uint8_t* proof; size_t len; };
std::vector<std::string> verify_device_batch(const char* who, hg_ctx* ctx, const Shape& sh, const std::vector<VerifyItem>& items, size_t Q);

// ---- folded openings (hg.h "Folded openings"): a sum-check over the committed tables reduces the n claims to one value Y_t a table at
// the prefixes of one point, which one combined row opens. The opening is a header - 3 coefficients a round, V = max_t v_t rounds,
// then the m values Y_t - followed by the body of an opening of one claim. The forms over bn256::Fr: pcs_bn254.hpp.
inline size_t fold_rounds(const Shape& sh) { int V = 0; for (int v : sh.nvars) V = v > V ? v : V; return (size_t)V; }
inline size_t folded_header_bytes(const Shape& sh) { return 16 * (3 * fold_rounds(sh) + sh.nvars.size()); }
inline size_t folded_opening_bytes(const Shape& sh, size_t Q) { return folded_header_bytes(sh) + opening_bytes(sh, 1, Q); }
// The prover's side of the reduction, one object an opening. step(j, r, s), j = 0 .. V in turn: the tables still live are folded by r
// (the challenge of round j - 1; j = 0 folds nothing); a table left with one entry retires - T[t] and G[t] receive the entries of T_t and
// g_t, the evaluations at rho[..v_t) - and for j < V s = the sums over the tables that stay live of g(0,x') T(0,x'), of g(1,x') T(1,x')
// and of (g(1,x') - g(0,x')) (T(1,x') - T(0,x')): s_j's value at 0, its value at 1 and its coefficient c2, without the retired tables.
struct FoldSource {
    std::vector<E2> T, G;   // per table, valid once it has retired (v_t <= j after step j)
    virtual void step(size_t j, E2 r, E2 s[3]) = 0;
    virtual ~FoldSource() {}
};
// bpow[i] = beta^i. The host form reads cm.rows; the device form (pcs.hip) builds g and runs every round on the context's stream
std::unique_ptr<FoldSource> fold_source_host(const Commitment& cm, const std::vector<Claim>& claims, const std::vector<E2>& bpow);
std::unique_ptr<FoldSource> fold_source_device(const Commitment& cm, const std::vector<Claim>& claims, const std::vector<E2>& bpow);
// The prover's arithmetic of one reduction, which open_folded and the batch form (pcs.hip) share: the transcript, the running claim and
// the factors prod (1 - r_j') of the retired tables. T, G are a FoldSource's, or what a group pass brought back for the member.
struct FoldProver {
    FsTranscript tr;
    std::vector<E2> bpow, tail, rho;
    E2 claim, r;   // r: the challenge the next step folds by (zero ahead of round 0)
    FoldProver(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q);
    // round j < V from the sums of step(j): false, with nothing written, if they do not meet the running claim (a value is wrong); else
    // c0, c1, c2 are written and r = rho[j] is squeezed
    bool round(const Shape& sh, size_t j, const E2 s[3], const std::vector<E2>& T, const std::vector<E2>& G);
    // after step(V): false if the final evaluation misses the claim; else the Y_t are written
    bool finish(const Shape& sh, const std::vector<E2>& T, const std::vector<E2>& G);
    // delta and rho' squeezed -> the two row combinations of the body: the R powers of rho', the combined weights
    std::vector<CombineJob> body_jobs(const Shape& sh);
    // the u vectors behind the header and into the transcript
    void write_u(const E2* u, size_t n);
};
// hg_pcs_open_folded: the opening bytes; an Error naming `who` if there is no claim and - naming the lowest failing claim - if a value
// is not its table's evaluation (round 0 shows that one is wrong, the claims are then evaluated one by one)
std::vector<uint8_t> open_folded(const char* who, const Commitment& cm, const std::vector<Claim>& claims, size_t Q);
// hg_pcs_open_folded_batch (pcs.hip): open_device_batch for folded openings (every item has a claim): a group's reductions run as one
// launch a round over all members, with one synchronisation a round. refused / bytes as there, the reason is open_folded's under `single`
std::vector<Opened> open_folded_device_batch(const char* who, const char* single, hg_ctx* ctx, const std::vector<OpenItem>& items, size_t Q);
// hg_pcs_verify_folded_device_batch (pcs.hip): verify_device_batch for folded openings: why[i] is what verify_folded_device returns for
// item i alone; the headers on the host threads, the bodies through verify_device_batch's pass as openings of one claim
std::vector<std::string> verify_folded_device_batch(const char* who, hg_ctx* ctx, const Shape& sh, const std::vector<VerifyItem>& items, size_t Q);
// hg_pcs_verify_folded: "" = accepted, else the reason
std::string verify_folded(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len);
// hg_pcs_verify_folded_device (pcs.hip, verify_folded_flow of pcs_flow.hpp): the same decision and reason; the header on the host, the body through
// verify_device's kernels
std::string verify_folded_device(hg_ctx* ctx, const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof, size_t len);
// What the two folded verifiers share: everything the header decides. The header's words are read (`noncanonical`: the lowest byte
// offset of one that is not below p, else ~0; the walk then stops), the rounds and the final evaluation checked (`reason`: the first
// that fails, the walk goes on regardless so that the body's challenges exist) and the body's one claim formed: the transcript with
// delta and rho squeezed, the R powers of rho, the combined weights over all R rows, the value sum_t delta^t Y_t and the point rho[..c)
struct FoldedHeader {
    size_t noncanonical = ~(size_t)0;
    std::string reason;
    FsTranscript tr;
    std::vector<E2> rho_pw, w, lo;
    E2 y;
};
FoldedHeader folded_header(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const uint8_t* proof);

// ---- what both forms of the verifier share (pcs.cpp): the length check, the transcript up to the column indices, the reasons
std::string length_reason(const Shape& sh, size_t n_claims, size_t Q, size_t len);   // "" if the length is the opening's
std::string length_reason(size_t len, size_t want);                                   // the same for a length worked out by the caller
// tag: "hg-pcs-1", or "hg-pcs-fold-1" for a folded opening
FsTranscript start_transcript(const Shape& sh, const uint8_t root[32], const std::vector<Claim>& claims, size_t Q, const char* tag = "hg-pcs-1");
std::vector<E2> rho_powers(E2 rho, size_t R);
void absorb_words(FsTranscript& tr, const u64* words, size_t count);                 // the u_i as read: c0, c1 of every element
std::vector<size_t> squeeze_indices(FsTranscript& tr, size_t N, size_t Q);           // j_q = a squeezed word & (N - 1)
std::string reason_noncanonical(size_t byte);
std::string reason_evaluation(size_t claim);
std::string reason_merkle(size_t query);
std::string reason_proximity(size_t query);
std::string reason_claim(size_t claim, size_t query);

}  // namespace pcs
}  // namespace hg
