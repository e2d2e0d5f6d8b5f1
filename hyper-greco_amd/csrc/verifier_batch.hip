// hg_verify_device_batch: BfvEncrypt::verify of a run of proofs under one key in one device pass per group [REF
// bfv-gkr/src/sk_encryption_circuit.rs:462-517]. Every proof gets exactly the decision of verify_proof_device (verifier_dev.hip).
//   1. The walks (verifier.cpp: verify_walk) run on the host threads, one proof each, against a backend that only RECORDS its jobs
//      symbolically (no device call, no arena allocation: the bump allocator is not thread-safe). The walk opens no OpenMP region of
//      its own, so nothing nests.
//   2. The jobs of a group are merged. Chain offsets are made absolute - mode 0 reads the context's fixed chain, modes 1-3 the
//      concatenation of the proofs' own chains, each proof's offsets shifted by its base - and identical tables are built once:
//      in mode 0 every eq table, constant-gate sum, Libra gather, DFT-row table and their dot products are the same for every
//      proof (they depend on the key only), so a group pays for them once. Phase-2 gathers (they read the proof's own phase-1
//      evaluations) and the input evaluations (they read the proof's own witness) are never shared.
//   3. One allocation, one descriptor copy, one launch per kind (the launchers of the single-proof verifier), one synchronisation,
//      then every proof's deferred comparisons (verify_complete) on the host threads.
// The public inputs are gathered by host threads into page-locked memory and copied on a stream of their own: group g+1's copies
// and walks run while group g's kernels do.
// hg_verify_public_batch is the same pass from the ciphertext (the batch form of verify_public_device, verifier_dev.hip): the walks
// run with public_only, the recording backend in its compact form, each proof's instance is staged as it is (2 k n signed words),
// k_vin_dots<true> evaluates ais and ct0is from them, and the claims on the secret inputs come back from each proof's pending state.
// hg_verify_public_bound_batch is that pass for bound proofs (the batch form of verify_public_device with a root): a third source kind
// of verify_batch_run. A group's instances are staged in slices, each slice's statement digests are taken out of the staged set on the
// upload stream, in the batch's own buffers (batch_stage_instances_bound), and a group's walks wait for its digests before they start
// from bound_seed; launch and complete are the unbound ones.
// What of this is the same over BN254 - the recording backend, the merge of step 2, the work units of the input evaluations and the
// loop over the groups - is verifier_merge.hpp. This file keeps what is Goldilocks': the group-size rule, the chain a group reads
// (the context's, or the proofs' own), the lowering of a merged group into tables, descriptors and launches, and the input kernels.
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <omp.h>
#include "verifier_batch.hpp"
#include "gl_wide.hpp"
#include "pcs.hpp"

namespace hg {
namespace {

// ---- the MLE evaluations of the public inputs -------------------------------------------------------------------------------------
// Work unit: one eq table and the P input tables evaluated at its point (mode 0: the group's tables of one input; modes 1-3: one).
// A workgroup owns VB_TILE consecutive entries: it reads its eq tile once into registers and multiply-accumulates it against each
// of the P tables, eight products per accumulator before one reduction (gl_wide.hpp), one partial per (member, workgroup). A second
// launch adds every member's partials into its result slot. HBM traffic: 8 B per input entry plus 16 / P B of eq.
constexpr int VB_TPB = 256, VB_ITEMS = 8, VB_TILE = VB_TPB * VB_ITEMS;
typedef VinUnitT<E2> VinUnit;   // member p's partial of workgroup b: part0 + p * nblk + b

// COMPACT: k_vin_dots over the compact signed coefficients of public instances (hg_verify_public_batch; CompactDotJob, prover.hpp, is
// the single-proof form). A unit is one eq table and the P members' coefficient blocks evaluated at its point (mode 0: the group's
// tables of one public input; modes 1-3: one). A workgroup owns VB_TILE consecutive WORD indices t of the non-padding range only
// (U.n = blocks * 2^log2_n of them): with b = t >> log2_n and r = t & (n-1), eq entry b * 2n + lo + r meets coefficient n-1-r of
// block b (vin_at), exactly as k_vdot_compact_jobs indexes (ais[i]: one block, lo = 0; ct0is: k blocks, lo = n-1). The eq tile is loaded
// once into registers; per member the eight int64 words are read (descending over the same cache lines as the eq loads ascend) and
// the sign becomes the field element in registers, a negative z being GL_P - |z|. Accumulator bound: the plain form's, eight products of
// canonical operands per accumulator before one reduction - |z| <= (q_i-1)/2 < 2^61 (hg_instance_from_ciphertext checks the range),
// so the lifted word is canonical, and the eq entries are. One partial per (member, workgroup); k_vin_reduce adds them. HBM traffic
// by design: 8 B per coefficient plus 16 / P B of eq, nothing for padding words - the padding half of an eq table is never read.
template <bool COMPACT>
__global__ __launch_bounds__(VB_TPB) void k_vin_dots(const VinUnit* __restrict__ units, const VinMember* __restrict__ members,
                                                     const VinBlock* __restrict__ blocks, E2* __restrict__ partials) {
    __shared__ E2 sm[2][VB_TPB / 64];
    const VinBlock B = blocks[blockIdx.x];
    const VinUnit U = units[B.unit];
    const size_t base = (size_t)B.blk * VB_TILE + threadIdx.x, nm1 = ((size_t)1 << U.log2_n) - 1;
    E2 eq[VB_ITEMS];
#pragma unroll
    for (int j = 0; j < VB_ITEMS; j++) {
        const size_t t = base + (size_t)j * VB_TPB;
        size_t ie, iw;
        vin_at<COMPACT>(t, nm1, U.lo, ie, iw);
        eq[j] = t < U.n ? U.eq[ie] : e2_zero();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = 0; p < U.P; p++) {
        const u64* __restrict__ a = members[U.first + p].a;
        u64 v[VB_ITEMS];
#pragma unroll
        for (int j = 0; j < VB_ITEMS; j++) {
            const size_t t = base + (size_t)j * VB_TPB;
            size_t ie, iw;
            vin_at<COMPACT>(t, nm1, U.lo, ie, iw);
            v[j] = t < U.n ? a[iw] : 0;
            if constexpr (COMPACT) {
                const int64_t z = (int64_t)v[j];
                v[j] = z >= 0 ? (u64)z : GL_P - (u64)(-z);
            }
        }
        WAcc c0 = wacc_zero(), c1 = wacc_zero();
#pragma unroll
        for (int j = 0; j < VB_ITEMS; j++) wmac2(c0, eq[j].c0, v[j], c1, eq[j].c1, v[j]);
        E2 s = e2(wreduce(c0), wreduce(c1));
        for (int o = 32; o > 0; o >>= 1) {
            E2 t;
            t.c0 = __shfl_xor(s.c0, o);
            t.c1 = __shfl_xor(s.c1, o);
            s = e2_add(s, t);
        }
        // (two LDS buffers: member p + 1 writes the other one, and thread 0 has read this one before the next barrier)
        if (lane == 0) sm[p & 1][wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            E2 t = sm[p & 1][0];
            for (int w = 1; w < VB_TPB / 64; w++) t = e2_add(t, sm[p & 1][w]);
            partials[U.part0 + (size_t)p * U.nblk + B.blk] = t;
        }
    }
}
// one wave per member: its unit's nblk partials into its slot
__global__ __launch_bounds__(64) void k_vin_reduce(const VinUnit* __restrict__ units, const VinMember* __restrict__ members,
                                                   const E2* __restrict__ partials, E2* __restrict__ res) {
    const VinMember M = members[blockIdx.x];
    const VinUnit U = units[M.unit];
    const E2* part = partials + U.part0 + (size_t)(blockIdx.x - U.first) * U.nblk;
    E2 s = e2_zero();
    for (int b = threadIdx.x; b < U.nblk; b += 64) s = e2_add(s, part[b]);
    for (int o = 32; o > 0; o >>= 1) {
        E2 t;
        t.c0 = __shfl_xor(s.c0, o);
        t.c1 = __shfl_xor(s.c1, o);
        s = e2_add(s, t);
    }
    if (threadIdx.x == 0) res[M.slot] = s;
}

}  // namespace

VerifyBatchBufs* batch_bufs(hg_ctx* ctx) {
    if (!ctx->verify_batch) {
        auto* b = new VerifyBatchBufs();
        ctx->verify_batch = b;
        b->slabs = std::make_shared<pcs::SlabSpares>();
        b->slabs->cap = VB_PCS_COMMIT_BUDGET_BN254;
        hip_check(hipStreamCreateWithFlags(&b->up, hipStreamNonBlocking), "hipStreamCreate(batch uploads)");
        for (auto& e : b->ev) hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate(batch uploads)");
        for (auto& e : b->ev_dg) hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate(batch digests)");
    }
    return static_cast<VerifyBatchBufs*>(ctx->verify_batch);
}

namespace pcs {
u64* SlabSpares::take(size_t need, size_t* bytes) {
    std::lock_guard<std::mutex> lock(mu);
    size_t best = spare.size();
    for (size_t i = 0; i < spare.size(); i++)
        if (spare[i].second >= need && spare[i].second / 2 <= need && (best == spare.size() || spare[i].second < spare[best].second)) best = i;
    if (best == spare.size()) return nullptr;
    u64* p = spare[best].first;
    *bytes = spare[best].second;
    spare.erase(spare.begin() + best);
    return p;
}
void SlabSpares::give(u64* p, size_t bytes) {
    std::lock_guard<std::mutex> lock(mu);
    if (closed || bytes > cap) { (void)hipFree(p); return; }
    spare.push_back({p, bytes});
    size_t total = 0;
    for (const auto& s : spare) total += s.second;
    while (total > cap) {
        total -= spare.front().second;
        (void)hipFree(spare.front().first);
        spare.erase(spare.begin());
    }
}
void SlabSpares::close() {
    std::lock_guard<std::mutex> lock(mu);
    closed = true;
    for (const auto& s : spare) (void)hipFree(s.first);
    spare.clear();
}
}  // namespace pcs

char* batch_desc_host(VerifyBatchBufs* B, size_t bytes) {
    if (bytes > B->desc_cap) {
        if (B->h_desc) (void)hipHostFree(B->h_desc);
        B->h_desc = nullptr;
        B->desc_cap = 0;
        hip_check(hipHostMalloc((void**)&B->h_desc, bytes, hipHostMallocDefault), "hipHostMalloc(batch descriptors)");
        B->desc_cap = bytes;
    }
    return B->h_desc;
}

char* batch_out_host(VerifyBatchBufs* B, size_t bytes) {
    if (bytes > B->out_cap) {
        if (B->h_out) (void)hipHostFree(B->h_out);
        B->h_out = nullptr;
        B->out_cap = 0;
        hip_check(hipHostMalloc((void**)&B->h_out, bytes, hipHostMallocDefault), "hipHostMalloc(batch results)");
        B->out_cap = bytes;
    }
    return B->h_out;
}

namespace {
// set s free again (its last copy waited for) and grown to `total` words
void stage_set(VerifyBatchBufs* B, int s, size_t total, const std::string& w) {
    if (B->recorded[s]) hip_check(hipEventSynchronize(B->ev[s]), (w + ": input set reuse").c_str());
    if (B->words[s] < total) {
        if (B->h_in[s]) { (void)hipHostFree(B->h_in[s]); B->h_in[s] = nullptr; }
        if (B->d_in[s]) { (void)hipFree(B->d_in[s]); B->d_in[s] = nullptr; }
        B->words[s] = 0;
        hip_check(hipHostMalloc((void**)&B->h_in[s], total * sizeof(u64), hipHostMallocDefault), "hipHostMalloc(batch inputs)");
        hip_check(hipMalloc((void**)&B->d_in[s], total * sizeof(u64)), "hipMalloc(batch inputs)");
        B->words[s] = total;
    }
}
// the gather of a set in pieces of 2 MB on the host threads, then its copy on the upload stream
struct Piece { u64* dst; const u64* src; size_t n; };
void stage_table(std::vector<Piece>& pieces, u64*& dst, const u64* src, size_t n) {
    constexpr size_t PIECE = (size_t)1 << 18;   // 2 MB
    for (size_t o = 0; o < n; o += PIECE) pieces.push_back(Piece{dst + o, src + o, std::min(PIECE, n - o)});
    dst += n;
}
void stage_gather(const std::vector<Piece>& pieces, [[maybe_unused]] int nthr) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)pieces.size()))
    for (long long q = 0; q < (long long)pieces.size(); q++) memcpy(pieces[q].dst, pieces[q].src, pieces[q].n * sizeof(u64));
}
void stage_copy(VerifyBatchBufs* B, int s, const std::vector<Piece>& pieces, size_t total, int nthr, const std::string& w) {
    stage_gather(pieces, nthr);
    hip_check(hipMemcpyAsync(B->d_in[s], B->h_in[s], total * sizeof(u64), hipMemcpyHostToDevice, B->up), (w + ": upload inputs").c_str());
    hip_check(hipEventRecord(B->ev[s], B->up), "hipEventRecord");
    B->recorded[s] = true;
}
}  // namespace

void batch_stage_inputs(VerifyBatchBufs* B, int s, const std::vector<const Witness*>& ws, size_t i0, size_t i1, const BatchInputs& L,
                        int nthr, const char* who) {
    const size_t np = i1 - i0, words = L.words, SZ = L.SZ, PZ = L.PZ, K = L.K;
    const std::string w(who);
    stage_set(B, s, np * words, w);
    std::vector<Piece> pieces;
    for (size_t i = i0; i < i1; i++) {
        const Witness& x = *ws[i];
        u64* dst = B->h_in[s] + (i - i0) * words;
        const std::pair<const u64*, size_t> tabs[] = {{x.s.data(), SZ}, {x.e.data(), SZ}, {x.k1.data(), SZ}, {x.ais.data(), K * SZ},
                                                      {x.r1is.data(), K * SZ}, {x.r2is.data(), K * PZ}, {x.ct0is.data(), K * SZ}};
        for (auto& t : tabs) stage_table(pieces, dst, t.first, t.second);
    }
    stage_copy(B, s, pieces, np * words, nthr, w);
}

void batch_stage_instances(VerifyBatchBufs* B, int s, const std::vector<const Instance*>& insts, size_t i0, size_t i1, size_t kn, int nthr,
                           const char* who) {
    const size_t np = i1 - i0;
    const std::string w(who);
    stage_set(B, s, np * 2 * kn, w);
    std::vector<Piece> pieces;
    for (size_t i = i0; i < i1; i++) {
        const Instance& x = *insts[i];
        u64* dst = B->h_in[s] + (i - i0) * 2 * kn;
        stage_table(pieces, dst, reinterpret_cast<const u64*>(x.a.data()), kn);
        stage_table(pieces, dst, reinterpret_cast<const u64*>(x.ct0.data()), kn);
    }
    stage_copy(B, s, pieces, np * 2 * kn, nthr, w);
}

// batch_stage_instances for the bound pass (hg_verify_public_bound_batch, hg_instance_digest_group), in slices of `slice` members: the
// host threads gather a slice, its copy is enqueued on the upload stream, the statement digests of its members behind the copy
// (pcs::instance_digest_group_enqueue: read out of d_in[s], the nodes in d_dg[s]) and the copy of their 32-byte roots into h_dg[s] behind
// those - so copies and digests run under the gather of the next slice, and nothing of it touches the context's arena or staging
// buffer. The set's event is recorded behind the last slice as ever (stage_set waits for it before the set, its node words and its
// digest block are reused or grown), ev_dg[s] at the same place: the digests of the set are back.
namespace {
void batch_stage_instances_bound(hg_ctx* ctx, VerifyBatchBufs* B, int s, const Params& p, const std::vector<const Instance*>& insts, size_t i0, size_t i1,
                                 size_t kn, size_t slice, int nthr, const char* who) {
    const size_t np = i1 - i0, dgw = pcs::instance_digest_group_words(p);
    const std::string w(who);
    stage_set(B, s, np * 2 * kn, w);
    if (B->dg_words[s] < np * dgw) {
        if (B->d_dg[s]) { (void)hipFree(B->d_dg[s]); B->d_dg[s] = nullptr; }
        B->dg_words[s] = 0;
        hip_check(hipMalloc((void**)&B->d_dg[s], np * dgw * sizeof(u64)), "hipMalloc(batch digests)");
        B->dg_words[s] = np * dgw;
    }
    if (B->dg_cap[s] < np) {
        if (B->h_dg[s]) { (void)hipHostFree(B->h_dg[s]); B->h_dg[s] = nullptr; }
        B->dg_cap[s] = 0;
        hip_check(hipHostMalloc((void**)&B->h_dg[s], 32 * np, hipHostMallocDefault), "hipHostMalloc(batch digests)");
        B->dg_cap[s] = np;
    }
    for (size_t a = 0; a < np; a += slice) {
        const size_t b = std::min(np, a + slice);
        std::vector<Piece> pieces;
        for (size_t m = a; m < b; m++) {
            const Instance& x = *insts[i0 + m];
            u64* dst = B->h_in[s] + m * 2 * kn;
            stage_table(pieces, dst, reinterpret_cast<const u64*>(x.a.data()), kn);
            stage_table(pieces, dst, reinterpret_cast<const u64*>(x.ct0.data()), kn);
        }
        stage_gather(pieces, nthr);
        hip_check(hipMemcpyAsync(B->d_in[s] + a * 2 * kn, B->h_in[s] + a * 2 * kn, (b - a) * 2 * kn * sizeof(u64), hipMemcpyHostToDevice, B->up),
                  (w + ": upload inputs").c_str());
        pcs::instance_digest_group_enqueue(ctx, B->up, p, B->d_in[s] + a * 2 * kn, b - a, B->d_dg[s] + a * dgw, B->h_dg[s] + 32 * a);
    }
    hip_check(hipEventRecord(B->ev[s], B->up), "hipEventRecord");
    B->recorded[s] = true;
    hip_check(hipEventRecord(B->ev_dg[s], B->up), "hipEventRecord");
}
// members a slice: the option, else what fits in 32 MiB of instance words, at least one (4 at n=32768 k=16)
size_t bound_slice(const hg_ctx* ctx, size_t kn) {
    if (ctx->bound_batch_slice > 0) return (size_t)ctx->bound_batch_slice;
    return std::max<size_t>(1, ((size_t)32 << 20) / (2 * kn * sizeof(u64)));
}
}  // namespace

void batch_stage_blobs(VerifyBatchBufs* B, int s, const std::vector<BatchBlob>& blobs, size_t total_words, [[maybe_unused]] int nthr, const char* who) {
    const std::string w(who);
    stage_set(B, s, std::max<size_t>(total_words, 1), w);
    constexpr size_t PIECE = (size_t)2 << 20;
    struct BytePiece { char* dst; const uint8_t* src; size_t n; };
    std::vector<BytePiece> pieces;
    for (const BatchBlob& b : blobs)
        for (size_t o = 0; o < b.bytes; o += PIECE) pieces.push_back(BytePiece{reinterpret_cast<char*>(B->h_in[s] + b.word_off) + o, b.p + o, std::min(PIECE, b.bytes - o)});
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::max(1, std::min<int>(nthr, (int)pieces.size())))
    for (long long q = 0; q < (long long)pieces.size(); q++) memcpy(pieces[q].dst, pieces[q].src, pieces[q].n);
    if (total_words) hip_check(hipMemcpyAsync(B->d_in[s], B->h_in[s], total_words * sizeof(u64), hipMemcpyHostToDevice, B->up), (w + ": upload openings").c_str());
    hip_check(hipEventRecord(B->ev[s], B->up), "hipEventRecord");
    B->recorded[s] = true;
}

void verify_batch_drop(hg_ctx* ctx) {
    if (!ctx->verify_batch) return;
    auto* b = static_cast<VerifyBatchBufs*>(ctx->verify_batch);
    if (b->up) { (void)hipStreamSynchronize(b->up); (void)hipStreamDestroy(b->up); }
    for (auto e : b->ev) if (e) (void)hipEventDestroy(e);
    for (auto e : b->ev_dg) if (e) (void)hipEventDestroy(e);
    for (auto p : b->h_in) if (p) (void)hipHostFree(p);
    for (auto p : b->d_in) if (p) (void)hipFree(p);
    for (auto p : b->h_dg) if (p) (void)hipHostFree(p);
    for (auto p : b->d_dg) if (p) (void)hipFree(p);
    if (b->h_desc) (void)hipHostFree(b->h_desc);
    if (b->h_out) (void)hipHostFree(b->h_out);
    if (b->slabs) b->slabs->close();
    delete b;
    ctx->verify_batch = nullptr;
}

namespace {
// the MLE evaluations of the inputs: one partial per (member, workgroup), then every member's partials into its slot
void vin_launch(hipStream_t st, bool compact, const VinUnit* units, const VinMember* members, size_t nmembers, const VinBlock* blocks, size_t nblocks,
                E2* part, E2* res) {
    if (compact) k_vin_dots<true><<<(unsigned)nblocks, VB_TPB, 0, st>>>(units, members, blocks, part);
    else k_vin_dots<false><<<(unsigned)nblocks, VB_TPB, 0, st>>>(units, members, blocks, part);
    k_vin_reduce<<<(unsigned)nmembers, 64, 0, st>>>(units, members, part, res);
}

// What a batch checks its proofs against: witness handles (hg_verify_device_batch: ws) or public instances (hg_verify_public_batch:
// insts, and open[i] receives the claims an accepted proof i leaves on the secret inputs). `who` prefixes the error messages.
// roots (hg_verify_public_bound_batch, else null): the proofs are bound ones - proof i's transcript starts from bound_seed over the
// statement digest of insts[i], taken from the staged set, and roots[i]; digests receives the 32 bytes of every item.
struct BatchSrc {
    const char* who;
    const std::vector<const Witness*>* ws;
    const std::vector<const Instance*>* insts;
    std::vector<std::vector<OpenClaim>>* open;
    const std::vector<const uint8_t*>* roots = nullptr;
    std::vector<uint8_t>* digests = nullptr;
};

void verify_batch_run(hg_ctx* ctx, const hg_pk* pk, const BatchSrc& src, const std::vector<const uint8_t*>& proofs, const std::vector<size_t>& lens, int mode,
                      std::vector<std::string>& why) {
    const size_t n = proofs.size();
    const bool pub = src.insts != nullptr, bound = src.roots != nullptr;
    const std::string who(src.who);
    why.assign(n, std::string());
    if (pub) src.open->assign(n, std::vector<OpenClaim>());
    if (bound) src.digests->assign(32 * n, 0);
    if (!n) return;
    const bool times = hg_times("verify");
    const double t0 = omp_get_wtime();
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    Drain drain{ctx->stream, B->up};
    hip_check(hipStreamSynchronize(ctx->stream), (who + ": synchronise").c_str());   // (the arena is reset below)
    ctx->ensure_chain(16384);
    const Params& p = pk->params;
    // one proof's inputs in HBM, in the order of verify_proof_device: s, e, k1, ais (k), r1is (k), r2is, then ct0is; from the
    // ciphertext: its instance as it is, a then ct0, k n signed words each (the node tables of modes 1-3 are as large either way)
    const BatchInputs L(p);
    const size_t kn = L.K * L.PZ, words = pub ? 2 * kn : L.words;
    const size_t in_bytes = L.words * sizeof(u64);
    size_t G = (size_t)std::max<int64_t>(0, ctx->verify_batch_group);
    if (!G) {
        G = std::max<size_t>(1, VB_INPUT_BUDGET / (words * sizeof(u64)));
        if (mode != 0) G = std::min(G, std::max<size_t>(1, VB_TABLE_BUDGET / (5 * in_bytes)));
        G = std::min(G, VB_MAX_GROUP);
    }
    const size_t ngroups = (n + G - 1) / G;
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());   // (the device pass of hipcc ignores the pragmas)

    std::vector<std::vector<Walked<E2>>> groups(ngroups);
    // stage group g: gather its inputs into page-locked set g & 1 (host threads), copy them on the upload stream
    auto stage = [&](size_t g) {
        if (bound) batch_stage_instances_bound(ctx, B, (int)(g & 1), p, *src.insts, g * G, std::min(n, g * G + G), kn, bound_slice(ctx, kn), nthr, src.who);
        else if (pub) batch_stage_instances(B, (int)(g & 1), *src.insts, g * G, std::min(n, g * G + G), kn, nthr, src.who);
        else batch_stage_inputs(B, (int)(g & 1), *src.ws, g * G, std::min(n, g * G + G), L, nthr, src.who);
    };
    // walk group g on the host threads (a bound walk cannot squeeze its first challenge before its digest is back: wait for the set's)
    auto walk = [&](size_t g) {
        const size_t i0 = g * G, i1 = std::min(n, i0 + G);
        const uint8_t* dg = nullptr;
        if (bound) {
            hip_check(hipEventSynchronize(B->ev_dg[g & 1]), (who + ": the statement digests").c_str());
            dg = B->h_dg[g & 1];
            memcpy(src.digests->data() + 32 * i0, dg, 32 * (i1 - i0));
        }
        walk_group(groups[g], i0, i1, nthr, who, [&](Walked<E2>& x) {
            x.rec.reset(new RecBackendT<E2>(pk, pub, false));
            std::vector<uint8_t> seed;
            if (bound) seed = bound_seed(p.raw, mode, dg + 32 * (x.idx - i0), (*src.roots)[x.idx]);
            x.pend = verify_walk(*x.rec, p, pk->lasso, pk->circuit, proofs[x.idx], lens[x.idx], mode, pub, bound ? &seed : nullptr);
        });
    };
    // merge group g's jobs and enqueue them; returns the result slots used
    auto launch = [&](size_t g) -> size_t {
        const int s = (int)(g & 1);
        std::vector<Walked<E2>>& W = groups[g];
        hipStream_t st = ctx->stream;
        ctx->arena_reset();
        // mode 0 reads the context's fixed chain, modes 1-3 the concatenation of the proofs' own chains
        for (auto& x : W) {
            if (!x.pend.live()) continue;
            if (mode != 0 && x.rec->chain_need > x.pend.chain.size())
                throw Error(who + ": proof " + std::to_string(x.idx) + ": verifier: a job reads past the challenges the walk squeezed");
            if (mode == 0 && x.rec->chain_need > ctx->chal_e) throw Error(who + ": proof " + std::to_string(x.idx) + ": verifier: a job reads past the fixed chain");
        }
        const MergedGroup<E2> M = merge_group(W, mode != 0);
        const auto& consts = M.consts;
        const auto& lins = M.lins;
        const auto& muls = M.muls;
        const auto& ffts = M.ffts;
        const auto& dots = M.dots;
        const std::vector<E2>& chain = M.chain;
        const std::vector<E2>& us = M.us;
        const int nslot = M.nslot;
        typedef RecBackendT<E2> Rec;
        std::vector<dev::EqJob> eqs(M.eqs.size());
        int eq_max_n = 0, fft_max_L = 0, fft_max_claims = 0;
        size_t gt_max = 0, gb_max = 0;
        for (size_t e = 0; e < eqs.size(); e++) {
            memset(&eqs[e], 0, sizeof(eqs[e]));
            eqs[e].n = M.eqs[e].n; eqs[e].cs = M.eqs[e].cs;
            eq_max_n = std::max(eq_max_n, eqs[e].n);
        }
        for (auto& f : ffts) {
            fft_max_L = std::max(fft_max_L, pk->circuit.nodes[f.node].log2_size);
            fft_max_claims = std::max(fft_max_claims, f.cs.n);
        }
        if ((size_t)nslot > ctx->res_cap)
            throw Error(who + ": a group needs " + std::to_string(nslot) + " result slots, the context has " + std::to_string(ctx->res_cap) + ": lower verify_batch_group");
        // device tables (arena)
        for (auto& J : eqs) J.out = ctx->alloc_n<E2>((size_t)1 << J.n);
        std::vector<dev::GatherJob> gts(lins.size());
        std::vector<E2*> lin_T(lins.size()), mul_B(muls.size()), fft_F(ffts.size());
        for (size_t i = 0; i < lins.size(); i++) {
            const HNode& nd = pk->circuit.nodes[lins[i].node];
            const size_t SR = (size_t)1 << (nd.log2_sub_in + nd.log2_reps);
            dev::GatherJob& gj = gts[i];
            memset(&gj, 0, sizeof(gj));
            gj.g.lin = pk->node_dev[lins[i].node].lin[lins[i].in];
            gj.eqc = eqs[lins[i].eq].out; gj.log2_S = nd.log2_sub_in; gj.log2_G = nd.log2_sub_out; gj.log2_R = nd.log2_reps;
            gj.T = lin_T[i] = ctx->alloc_n<E2>(SR);
            gt_max = std::max(gt_max, SR);
        }
        std::vector<dev::FftJob> fjs(ffts.size());
        for (size_t i = 0; i < ffts.size(); i++) {
            const HNode& nd = pk->circuit.nodes[ffts[i].node];
            const int L = nd.log2_size;
            const size_t N = (size_t)1 << L;
            fjs[i] = dev::FftJob{fft_F[i] = ctx->alloc_n<E2>(N), (nd.inverse ? pk->w_inv : pk->w_fwd).at(L), nd.inverse ? gl_inv(gl_from_u64(N)) : 1, L, ffts[i].cs};
        }
        // the descriptors, the walks' chains and phase-1 evaluations: one page-locked staging, one copy ahead of the launches
        const VinPlan<E2> V = vin_units(M, [&](size_t e) { return eqs[e].out; }, B->d_in[s], words, p, pub, VB_TILE, 1);
        const auto& units = V.units;
        const auto& members = V.members;
        const auto& blocks = V.blocks;
        size_t desc_bytes = 0;
        auto place = [&](size_t bytes) { const size_t o = desc_bytes; desc_bytes += (bytes + 255) & ~(size_t)255; return o; };
        const size_t o_chain = place(chain.size() * sizeof(E2)), o_us = place(us.size() * sizeof(E2)), o_eq = place(eqs.size() * sizeof(dev::EqJob)),
                     o_gt = place(gts.size() * sizeof(dev::GatherJob)), o_gb = place(muls.size() * sizeof(dev::GatherBJob)),
                     o_fft = place(fjs.size() * sizeof(dev::FftJob)), o_dot = place(dots.size() * sizeof(DotJob)),
                     o_unit = place(units.size() * sizeof(VinUnit)), o_mem = place(members.size() * sizeof(VinMember)),
                     o_blk = place(blocks.size() * sizeof(VinBlock));
        char* d_desc = static_cast<char*>(ctx->alloc(desc_bytes));
        char* h = batch_desc_host(B, desc_bytes);
        const E2* chal = mode != 0 ? reinterpret_cast<const E2*>(d_desc + o_chain) : ctx->d_chal;
        const E2* d_us = reinterpret_cast<const E2*>(d_desc + o_us);
        if (!chain.empty()) memcpy(h + o_chain, chain.data(), chain.size() * sizeof(E2));
        if (!us.empty()) memcpy(h + o_us, us.data(), us.size() * sizeof(E2));
        if (!eqs.empty()) memcpy(h + o_eq, eqs.data(), eqs.size() * sizeof(dev::EqJob));
        if (!gts.empty()) memcpy(h + o_gt, gts.data(), gts.size() * sizeof(dev::GatherJob));
        for (size_t i = 0; i < muls.size(); i++) {
            const auto& m = muls[i];
            const HNode& nd = pk->circuit.nodes[m.node];
            const size_t SR = (size_t)1 << (nd.log2_sub_in + nd.log2_reps);
            mul_B[i] = ctx->alloc_n<E2>(SR);
            gb_max = std::max(gb_max, SR);
            const dev::GatherBJob J{pk->node_dev[m.node].mulR[m.in], eqs[m.eqc].out, eqs[m.eqx].out, d_us + m.u_at, nd.log2_sub_in, nd.log2_sub_out, nd.log2_reps, mul_B[i]};
            memcpy(h + o_gb + i * sizeof(dev::GatherBJob), &J, sizeof(J));
        }
        if (!fjs.empty()) memcpy(h + o_fft, fjs.data(), fjs.size() * sizeof(dev::FftJob));
        for (size_t i = 0; i < dots.size(); i++) {
            const auto& d = dots[i];
            const E2* a = d.kind == Rec::D_LIN ? lin_T[d.tab] : d.kind == Rec::D_MUL ? mul_B[d.tab] : fft_F[d.tab];
            const DotJob J{a, eqs[d.eq].out, (size_t)1 << eqs[d.eq].n, d.slot, 0};
            memcpy(h + o_dot + i * sizeof(DotJob), &J, sizeof(J));
        }
        if (!units.empty()) {
            memcpy(h + o_unit, units.data(), units.size() * sizeof(VinUnit));
            memcpy(h + o_mem, members.data(), members.size() * sizeof(VinMember));
            memcpy(h + o_blk, blocks.data(), blocks.size() * sizeof(VinBlock));
        }
        if (desc_bytes) hip_check(hipMemcpyAsync(d_desc, h, desc_bytes, hipMemcpyHostToDevice, st), (who + ": upload descriptors").c_str());
        // one launch per kind (the job index is gridDim.y: launches of at most VD_MAX_Y jobs)
        auto chunks = [](size_t njobs, size_t per, auto fn) { for (size_t q0 = 0; q0 < njobs; q0 += per) fn(q0, std::min(per, njobs - q0)); };
        const auto* d_eqs = reinterpret_cast<const dev::EqJob*>(d_desc + o_eq);
        chunks(eqs.size(), VD_MAX_Y, [&](size_t q0, size_t nq) { dev::eq_jobs(st, d_eqs + q0, (int)nq, eq_max_n, chal); });
        for (const auto& c : consts) {
            const HNode& nd = pk->circuit.nodes[c.node];
            const hg_pk::NodeDev& dv = pk->node_dev[c.node];
            const int grid = dev::vanilla_const_sum(st, dv.const_gate, dv.const_coef, dv.nconst, eqs[c.eq].out, nd.log2_sub_out, nd.log2_reps, ctx->d_partials);
            dev::reduce_partials(st, ctx->d_partials, grid, 1, ctx->d_res + c.slot);
        }
        const auto* d_gts = reinterpret_cast<const dev::GatherJob*>(d_desc + o_gt);
        chunks(gts.size(), VD_MAX_Y, [&](size_t q0, size_t nq) { dev::gather_jobs(st, d_gts + q0, (int)nq, gt_max); });
        if (!fjs.empty()) {
            const size_t per = VD_MAX_Y / (size_t)fft_max_claims;   // (k_fft_tab: gridDim.y = jobs * claims)
            E2* tab = ctx->alloc_n<E2>(std::min(per, fjs.size()) * (size_t)fft_max_claims * ((size_t)1 << (fft_max_L > 4 ? fft_max_L - 4 : 0)) + 1);
            const auto* d_ffts = reinterpret_cast<const dev::FftJob*>(d_desc + o_fft);
            chunks(fjs.size(), per, [&](size_t q0, size_t nq) { dev::fft_jobs(st, d_ffts + q0, (int)nq, fft_max_L, fft_max_claims, chal, tab); });
        }
        const auto* d_gbs = reinterpret_cast<const dev::GatherBJob*>(d_desc + o_gb);
        chunks(muls.size(), VD_MAX_Y, [&](size_t q0, size_t nq) { dev::gather_B_jobs(st, d_gbs + q0, (int)nq, gb_max); });
        if (!dots.empty()) vdot_jobs(st, reinterpret_cast<const DotJob*>(d_desc + o_dot), dots.size(), ctx->alloc_n<E2>(dots.size() * (size_t)VD_BLOCKS), ctx->d_res);
        if (!units.empty()) {
            hip_check(hipStreamWaitEvent(st, B->ev[s], 0), (who + ": wait for the inputs").c_str());
            vin_launch(st, pub, reinterpret_cast<const VinUnit*>(d_desc + o_unit), reinterpret_cast<const VinMember*>(d_desc + o_mem), members.size(),
                       reinterpret_cast<const VinBlock*>(d_desc + o_blk), blocks.size(), ctx->alloc_n<E2>(V.parts), ctx->d_res);
        }
        if (ctx->d_res != ctx->h_res && nslot)
            hip_check(hipMemcpyAsync(ctx->h_res, ctx->d_res, (size_t)nslot * sizeof(E2), hipMemcpyDeviceToHost, st), (who + ": copy results").c_str());
        if (times)
            fprintf(stderr, "[hg] verify_batch: group %zu (%zu proofs): %zu eq tables, %zu constant sums, %zu + %zu gathers, %zu DFT rows, %zu dots, %zu input evaluations in %zu units (%.1f MB); %d slots\n",
                    g, W.size(), eqs.size(), consts.size(), lins.size(), muls.size(), ffts.size(), dots.size(), members.size(), units.size(), V.bytes / 1e6, nslot);
        return (size_t)nslot;
    };
    auto complete = [&](size_t g) {
        complete_group(groups[g], nthr, [&](int slot) { return ctx->h_res[slot]; }, [&](Walked<E2>& x) {
            why[x.idx] = verify_complete(x.pend);
            if (pub && why[x.idx].empty()) (*src.open)[x.idx] = std::move(x.pend.open);
        });
        if (bound && g + 1 == ngroups) ctx->prof_collect();   // (the last digests were waited for by the last walk, ahead of the last synchronisation)
    };
    batch_groups(ctx->stream, who, "verify_batch", times, t0, n, ngroups, G, stage, walk, launch, complete);
}

}  // namespace

void verify_batch_device(hg_ctx* ctx, const hg_pk* pk, const std::vector<const Witness*>& ws, const std::vector<const uint8_t*>& proofs,
                         const std::vector<size_t>& lens, int mode, std::vector<std::string>& why) {
    verify_batch_run(ctx, pk, BatchSrc{"hg_verify_device_batch", &ws, nullptr, nullptr}, proofs, lens, mode, why);
}

void verify_public_batch_device(hg_ctx* ctx, const hg_pk* pk, const std::vector<const Instance*>& insts, const std::vector<const uint8_t*>& proofs,
                                const std::vector<size_t>& lens, int mode, std::vector<std::string>& why, std::vector<std::vector<OpenClaim>>& open) {
    verify_batch_run(ctx, pk, BatchSrc{"hg_verify_public_batch", nullptr, &insts, &open}, proofs, lens, mode, why);
}

void verify_public_bound_batch_device(hg_ctx* ctx, const hg_pk* pk, const std::vector<const Instance*>& insts, const std::vector<const uint8_t*>& roots,
                                      const std::vector<const uint8_t*>& proofs, const std::vector<size_t>& lens, int mode, std::vector<std::string>& why,
                                      std::vector<std::vector<OpenClaim>>& open, std::vector<uint8_t>& digests) {
    verify_batch_run(ctx, pk, BatchSrc{"hg_verify_public_bound_batch", nullptr, &insts, &open, &roots, &digests}, proofs, lens, mode, why);
}

// the staging of the bound pass without its walks: groups as that pass cuts them by the option and the input budget, group g in set
// g & 1, its digests fetched once group g + 1 is enqueued
void instance_digest_group_device(hg_ctx* ctx, const Params& p, const std::vector<const Instance*>& insts, uint8_t* out) {
    const size_t n = insts.size(), kn = (size_t)p.k * p.PZ();
    if (!n) return;
    const char* who = "hg_instance_digest_group";
    for (const Instance* x : insts)
        if (x->a.size() != kn || x->ct0.size() != kn) throw Error("an instance does not hold k * n coefficients a table");
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    Drain drain{ctx->stream, B->up};
    size_t G = (size_t)std::max<int64_t>(0, ctx->verify_batch_group);
    if (!G) G = std::min(VB_MAX_GROUP, std::max<size_t>(1, VB_INPUT_BUDGET / (2 * kn * sizeof(u64))));
    const size_t ngroups = (n + G - 1) / G;
    const int nthr = std::max(1, hg_omp_threads());
    auto fetch = [&](size_t g) {
        hip_check(hipEventSynchronize(B->ev_dg[g & 1]), "hg_instance_digest_group: the statement digests");
        memcpy(out + 32 * g * G, B->h_dg[g & 1], 32 * (std::min(n, g * G + G) - g * G));
    };
    for (size_t g = 0; g < ngroups; g++) {
        batch_stage_instances_bound(ctx, B, (int)(g & 1), p, insts, g * G, std::min(n, g * G + G), kn, bound_slice(ctx, kn), nthr, who);
        if (g) fetch(g - 1);
    }
    fetch(ngroups - 1);
    hip_check(hipStreamSynchronize(B->up), "hg_instance_digest_group: synchronise");
    hip_check(hipGetLastError(), "hg_instance_digest_group: kernels");
    ctx->prof_collect();
}

// one eq job, then k_vin_dots<true> as ONE unit whose members are the instances' tables
void instance_mle_batch_device(hg_ctx* ctx, const Params& p, const std::vector<const Instance*>& insts, int which, int index, const std::vector<E2>& pt, E2* out) {
    const size_t np = insts.size();
    if (!np) return;
    const char* who = "hg_instance_mle_batch";
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    Drain drain{ctx->stream, B->up};
    hip_check(hipStreamSynchronize(ctx->stream), "hg_instance_mle_batch: synchronise");   // (the arena is reset below)
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t n = p.PZ(), kn = (size_t)p.k * n;
    batch_stage_instances(B, 0, insts, 0, np, kn, std::max(1, hg_omp_threads()), who);
    dev::EqJob J;
    memset(&J, 0, sizeof(J));
    J.n = (int)pt.size(); J.cs.n = 1; J.cs.unit_alpha = 1;   // (point_off[0] = 0: the point is the whole chain)
    J.out = ctx->alloc_n<E2>((size_t)1 << J.n);
    std::vector<std::pair<const u64*, int>> tabs(np);
    for (size_t i = 0; i < np; i++) tabs[i] = {B->d_in[0] + i * 2 * kn + (which ? kn : (size_t)index * n), (int)i};
    VinPlan<E2> V;
    V.add(J.out, which ? kn : n, (u32)p.n_log2, which ? (u32)(n - 1) : 0, tabs, VB_TILE, 1);
    const VinUnit& U = V.units[0];
    const auto& members = V.members;
    const auto& blocks = V.blocks;
    size_t desc_bytes = 0;
    auto place = [&](size_t bytes) { const size_t o = desc_bytes; desc_bytes += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_chain = place(pt.size() * sizeof(E2)), o_eq = place(sizeof(J)), o_unit = place(sizeof(U)), o_mem = place(np * sizeof(VinMember)),
                 o_blk = place(blocks.size() * sizeof(VinBlock));
    char* d_desc = static_cast<char*>(ctx->alloc(desc_bytes));
    char* h = batch_desc_host(B, desc_bytes);
    if (!pt.empty()) memcpy(h + o_chain, pt.data(), pt.size() * sizeof(E2));
    memcpy(h + o_eq, &J, sizeof(J));
    memcpy(h + o_unit, &U, sizeof(U));
    memcpy(h + o_mem, members.data(), np * sizeof(VinMember));
    memcpy(h + o_blk, blocks.data(), blocks.size() * sizeof(VinBlock));
    hip_check(hipMemcpyAsync(d_desc, h, desc_bytes, hipMemcpyHostToDevice, st), "hg_instance_mle_batch: upload descriptors");
    dev::eq_jobs(st, reinterpret_cast<const dev::EqJob*>(d_desc + o_eq), 1, J.n, reinterpret_cast<const E2*>(d_desc + o_chain));
    hip_check(hipStreamWaitEvent(st, B->ev[0], 0), "hg_instance_mle_batch: wait for the instances");
    E2* res = ctx->alloc_n<E2>(np);
    vin_launch(st, true, reinterpret_cast<const VinUnit*>(d_desc + o_unit), reinterpret_cast<const VinMember*>(d_desc + o_mem), np,
               reinterpret_cast<const VinBlock*>(d_desc + o_blk), blocks.size(), ctx->alloc_n<E2>(V.parts), res);
    hip_check(hipMemcpyAsync(out, res, np * sizeof(E2), hipMemcpyDeviceToHost, st), "hg_instance_mle_batch: copy results");
    hip_check(hipStreamSynchronize(st), "hg_instance_mle_batch: synchronise");
    hip_check(hipGetLastError(), "hg_instance_mle_batch: kernels");
}

}  // namespace hg
