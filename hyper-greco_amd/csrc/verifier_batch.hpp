// What the batched device verifiers share (verifier_batch.hip: hg_verify_device_batch and hg_verify_public_batch over Goldilocks;
// bn254_verify_batch.inc: hg_verify_device_batch_bn254 over bn256::Fr): the context's input sets and upload stream, the default
// group size and the staging of a group's inputs here; the recorder, the group merge, the input units, the loop over the groups, the
// layout of one proof's public inputs in a set and the stream guard of every device entry in verifier_merge.hpp.
#pragma once
#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include "kernels.hpp"
#include "prover.hpp"
#include "verifier_merge.hpp"

namespace hg {

namespace pcs { struct SlabSpares; }

// the context's batch buffers: two sets of a group's public inputs (page-locked and in HBM) and the stream that copies them
struct VerifyBatchBufs {
    hipStream_t up = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};   // the copies of set s are done
    bool recorded[2] = {false, false};
    u64* h_in[2] = {nullptr, nullptr};
    u64* d_in[2] = {nullptr, nullptr};
    size_t words[2] = {0, 0};
    // hg_verify_public_bound_batch: the statement digests of the set's members, hashed out of d_in[s] on the upload stream
    u64* d_dg[2] = {nullptr, nullptr};       // each member's subtree nodes and the levels above them (pcs::instance_digest_group_words a member)
    size_t dg_words[2] = {0, 0};
    uint8_t* h_dg[2] = {nullptr, nullptr};   // page-locked: 32 bytes a member, the digests as they come back
    size_t dg_cap[2] = {0, 0};               // members h_dg[s] holds
    hipEvent_t ev_dg[2] = {nullptr, nullptr};   // the digests of set s are back
    char* h_desc = nullptr;                  // page-locked descriptor staging of one group
    size_t desc_cap = 0;
    char* h_out = nullptr;                   // page-locked results of one group (hg_pcs_open_batch: the u vectors and the opening images)
    size_t out_cap = 0;
    std::shared_ptr<pcs::SlabSpares> slabs;  // hg_pcs_commit_batch_bn254: the allocations of groups whose handles were all freed, kept for the next groups
};
VerifyBatchBufs* batch_bufs(hg_ctx* ctx);
// the page-locked descriptor staging, grown to `bytes` (call it only after the previous group's copy has been waited for)
char* batch_desc_host(VerifyBatchBufs* B, size_t bytes);
// the page-locked result buffer, grown to `bytes` (call it only when no copy into it is in flight)
char* batch_out_host(VerifyBatchBufs* B, size_t bytes);

// budget of one group: its inputs in one set (and, in modes 1-3 of the Goldilocks batch, each proof's own node tables in the arena:
// about five times its inputs, 0.13 GB at n=32768 k=16)
constexpr size_t VB_INPUT_BUDGET = (size_t)1 << 30, VB_TABLE_BUDGET = (size_t)4 << 30;
constexpr size_t VB_MAX_GROUP = 64;
// hg_pcs_verify_device_batch: what the members of one group may take in all - each one's opening in a set and its u, columns,
// encoded rows and NTT scratch in the arena (about 19 MB a member at n=32768 k=16: opening 3.3, u 1.5, columns 1.7, enc and the
// scratch 6.3 each; 64 members: 1.2 GB). hg_pcs_verify_device_batch_bn254 counts its members' bytes against the same budget, 32 bytes an
// element (about 45 MB a member at that size: 47 members a group)
constexpr size_t VB_PCS_BUDGET = (size_t)2 << 30;
// hg_pcs_commit_batch_bn254: what the raw and the encoded rows of one group may take in all (283 MB a member at n=32768 k=16: 16
// members a group). The NTT temporary does not count: it is one slice's, whatever the group. Measured at that size in runs of 16
// with groups of 4 / 8 / 16: 1.73 / 1.37 / 1.29 ms of kernel time an item; the context keeps freed group allocations
// up to the same number of bytes (SlabSpares below)
constexpr size_t VB_PCS_COMMIT_BUDGET_BN254 = (size_t)17 << 28;

namespace pcs {
// What the batch forms of commit and open share over both fields (pcs.hip, bn254_pcs.inc)
// The allocations of groups whose last handle was freed, kept by the context (VerifyBatchBufs) for its next groups: a hipMalloc of
// gigabytes costs anything between 0.3 ms and 1.4 s, whatever was freed just before. At most `cap` bytes are kept, the oldest
// going first. A slab holds a reference, so a handle may outlive its context: once closed, everything is freed as it comes back.
struct SlabSpares {
    std::mutex mu;
    std::vector<std::pair<u64*, size_t>> spare;   // (allocation, its bytes), oldest first
    size_t cap = 0;
    bool closed = false;
    u64* take(size_t need, size_t* bytes);        // the smallest spare of at least `need` and at most twice as many bytes, or null
    void give(u64* p, size_t bytes);
    void close();                                 // hg_destroy
};
struct Slab {   // a group's raw and encoded rows; its members' handles share it
    u64* p = nullptr;
    size_t bytes = 0;
    std::shared_ptr<SlabSpares> home;             // where p goes when the last handle is freed (null: back to the runtime)
    ~Slab() {
        if (!p) return;
        if (home) home->give(p, bytes); else (void)hipFree(p);
    }
};
// [first, last) of a run cut into groups: at most VB_MAX_GROUP or the option, `bytes_of(i)` summed within `budget`, `rows_each` a
// member summed within max_rows; a group holds at least one member
template <class BytesOf>
std::vector<std::pair<size_t, size_t>> cut_groups(hg_ctx* ctx, size_t n, BytesOf bytes_of, size_t rows_each, size_t max_rows, size_t budget = VB_PCS_BUDGET) {
    size_t cap = VB_MAX_GROUP;
    if (ctx->verify_batch_group > 0) cap = std::min<size_t>(cap, (size_t)ctx->verify_batch_group);
    std::vector<std::pair<size_t, size_t>> groups;
    for (size_t a = 0; a < n;) {
        size_t b = a, bytes = 0;
        while (b < n && b - a < cap) {
            if (b > a && (bytes + bytes_of(b) > budget || (b - a + 1) * rows_each > max_rows)) break;
            bytes += bytes_of(b);
            b++;
        }
        groups.push_back({a, b});
        a = b;
    }
    return groups;
}
}  // namespace pcs

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
