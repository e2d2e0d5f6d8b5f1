// What the batched device verifiers share (verifier_batch.hip: hg_verify_device_batch and hg_verify_public_batch over Goldilocks;
// bn254_verify_batch.inc: hg_verify_device_batch_bn254 over bn256::Fr): the context's input sets and upload stream, the layout of one proof's public inputs
// in a set, the default group size, and the staging of a group's inputs.
#pragma once
#include <string>
#include <vector>
#include "kernels.hpp"
#include "prover.hpp"

namespace hg {

// the context's batch buffers: two sets of a group's public inputs (page-locked and in HBM) and the stream that copies them
struct VerifyBatchBufs {
    hipStream_t up = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};   // the copies of set s are done
    bool recorded[2] = {false, false};
    u64* h_in[2] = {nullptr, nullptr};
    u64* d_in[2] = {nullptr, nullptr};
    size_t words[2] = {0, 0};
    char* h_desc = nullptr;                  // page-locked descriptor staging of one group
    size_t desc_cap = 0;
    char* h_out = nullptr;                   // page-locked results of one group (hg_pcs_open_batch: the u vectors and the opening images)
    size_t out_cap = 0;
};
VerifyBatchBufs* batch_bufs(hg_ctx* ctx);
// the page-locked descriptor staging, grown to `bytes` (call it only after the previous group's copy has been waited for)
char* batch_desc_host(VerifyBatchBufs* B, size_t bytes);
// the page-locked result buffer, grown to `bytes` (call it only when no copy into it is in flight)
char* batch_out_host(VerifyBatchBufs* B, size_t bytes);

// one proof's public inputs in a set, in the order of the single-proof verifiers: s, e, k1, ais (k), r1is (k), r2is, then ct0is -
// the same signed integers in the same layout over both fields
struct BatchInputs {
    size_t SZ, PZ, K, words;
    explicit BatchInputs(const Params& p) : SZ(p.SZ()), PZ(p.PZ()), K((size_t)p.k), words((3 + 3 * K) * SZ + K * PZ) {}
    size_t offset(int k) const {   // the verifier's input table k (k < 0: ct0is)
        if (k < 0) return (3 + 2 * K) * SZ + K * PZ;
        if ((size_t)k < 3 + 2 * K) return (size_t)k * SZ;   // s, e, k1, then ais and r1is, SZ each
        return (3 + 2 * K) * SZ;                           // r2is
    }
    size_t length(int k) const { return k < 0 ? K * SZ : (size_t)k == 3 + 2 * K ? K * PZ : SZ; }
};

// budget of one group: its inputs in one set (and, in modes 1-3 of the Goldilocks batch, each proof's own node tables in the arena:
// about five times its inputs, 0.13 GB at n=32768 k=16)
constexpr size_t VB_INPUT_BUDGET = (size_t)1 << 30, VB_TABLE_BUDGET = (size_t)4 << 30;
constexpr size_t VB_MAX_GROUP = 64;
// hg_pcs_verify_device_batch: what the members of one group may take in all - each one's opening in a set and its u, columns,
// encoded rows and NTT scratch in the arena (about 19 MB a member at n=32768 k=16: opening 3.3, u 1.5, columns 1.7, enc and the
// scratch 6.3 each; 64 members: 1.2 GB). hg_pcs_verify_device_batch_bn254 counts its members' bytes against the same budget, 32 bytes an
// element (about 45 MB a member at that size: 47 members a group)
constexpr size_t VB_PCS_BUDGET = (size_t)2 << 30;

// dedup keys of the group merge: a job's descriptor with absolute chain offsets
typedef std::vector<u64> Key;
inline void key_cs(Key& k, const dev::ClaimSet& c, size_t base) {
    k.push_back((u64)c.n);
    k.push_back((u64)c.unit_alpha);
    if (!c.unit_alpha) k.push_back(c.alpha_off + base);
    for (int a = 0; a < c.n; a++) k.push_back(c.point_off[a] + base);
}

// gathers the inputs of proofs [i0, i1) into page-locked set `set` on the host threads (at most nthr) and copies them on the
// upload stream; the set's event marks the copy. `who` prefixes the error messages.
void batch_stage_inputs(VerifyBatchBufs* B, int set, const std::vector<const Witness*>& ws, size_t i0, size_t i1, const BatchInputs& L,
                        int nthr, const char* who);

// the same for the public instances of proofs [i0, i1) (hg_verify_public_batch): each as it is, a then ct0, kn = k * n signed words each
void batch_stage_instances(VerifyBatchBufs* B, int set, const std::vector<const Instance*>& insts, size_t i0, size_t i1, size_t kn, int nthr,
                           const char* who);

// the same for a run of byte strings (hg_pcs_verify_device_batch: the openings of a group): blob i, a whole number of words, lands at
// word word_off[i] of the set, which holds total_words
struct BatchBlob { const uint8_t* p; size_t bytes; size_t word_off; };
void batch_stage_blobs(VerifyBatchBufs* B, int set, const std::vector<BatchBlob>& blobs, size_t total_words, int nthr, const char* who);

}  // namespace hg
