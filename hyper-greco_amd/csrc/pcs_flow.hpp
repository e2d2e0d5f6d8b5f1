// What the device forms of the polynomial commitment share over both fields (pcs.hip over Goldilocks, bn254_pcs.inc over bn256::Fr):
// the descriptors their kernels read and the host flows, written once as templates over a field policy F (pcs::GlPcs, bn::BnPcs).
// The kernels stay per field. A policy names the field's types (Row: an element of a row, of the encoded matrix and of a column; W: an
// element of u and of a weight table), its sizes, its transcript calls, its profiler classes and texts, and has one static launch
// function per kernel step, which holds the profiler's byte formula, the grid and the launch. A flow decides what is staged where,
// what is enqueued in which order and what the host does meanwhile; it never names a kernel.
#pragma once
#include <omp.h>
#include <cstdio>
#include <cstring>
#include "pcs.hpp"
#include "prover.hpp"
#include "verifier_batch.hpp"

namespace hg {
namespace pcs {

// ---- the descriptors. A result cell holds the lowest offending key (atomicMin), so the reason is the host's also where several
// checks fail at once.
constexpr u64 PCSV_NONE = ~(u64)0;   // a cell no thread lowered: nothing failed
__device__ __forceinline__ void cell_min(u64* cell, u64 v) { atomicMin(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)v); }
struct CombineDesc { u64 row0, nrows, woff; };   // a row combination: sum_{r < nrows} w[woff + r] * row_{row0 + r}
struct VbMember {
    u64 proof, u, cols, enc_row;               // word offset of its opening in the set; offsets of its u and columns in Row units; its first row of enc
    u64 n, claim0, job0;                       // its claims; the claims and the jobs (claims + 1 each) of the members before it
    u64 root_at, jobs_at, y_at, z_at, w_at;    // byte offsets in the group's staged copy: root, job descriptors, values, low coordinates, weights
};
struct VbGroup { u64 G, Q, R, q_stride; int c, depth; };   // q_stride: from one query of an opening to the next, in Row units
template <class Row> struct ObJob { const Row* src; u64 nrows, w_at, u_at; };   // its first raw row; the byte offset of its weights in the staged copy; where u goes (elements)
struct ObClaim { u64 u_at, z_at, y_at, member, claim; };                        // its u_i (elements); byte offsets of the low coordinates and of the value
template <class Row> struct ObMember { const Row* M; u64 img, u, u_words; };    // its encoded matrix; word offsets of its image and of its u vectors; the words of its u vectors

// ---- what the two verifiers share on the host: a member's block of the staged copy and the reading of its three result cells
template <class F> size_t align_up(size_t x) { return (x + F::ALIGN - 1) & ~(size_t)(F::ALIGN - 1); }
// a query of an opening in Row units: its R column elements and the 32-byte siblings of its path
template <class F> size_t query_stride(const Shape& sh) { return sh.R + (size_t)sh.depth() * (32 / sizeof(typename F::Row)); }
// the entries of a member's weight tables: R powers of rho, then eq(z_i[c..]) over the rows of every claim's table
template <class F> size_t weights_of(const Shape& sh, const std::vector<typename F::Claim>& claims) {
    size_t nw = sh.R;
    for (const typename F::Claim& cl : claims) nw += (size_t)1 << (sh.nvars[cl.table] - sh.c);
    return nw;
}
// The block of a member of n claims and nw weights from byte `at` (a multiple of F::ALIGN) of a staged copy on: root, job
// descriptors, values, the low coordinates of the points, weight tables. Into its descriptor -> the byte behind the block
template <class F> size_t member_block_layout(VbMember& d, const Shape& sh, size_t n, size_t nw, size_t at) {
    typedef typename F::W W;
    d.root_at = at;
    d.jobs_at = d.root_at + 32;
    d.y_at = d.jobs_at + align_up<F>((n + 1) * sizeof(CombineDesc));
    d.z_at = d.y_at + n * sizeof(W);
    d.w_at = d.z_at + n * (size_t)sh.c * sizeof(W);
    return d.w_at + nw * sizeof(W);
}
// fills the block (low coordinates and weights in the form the field's kernels take) -> the member's transcript, rho squeezed
template <class F> FsTranscript member_block_fill(char* h_stage, const VbMember& d, const Shape& sh, const uint8_t root[32], const std::vector<typename F::Claim>& claims, size_t Q) {
    typedef typename F::W W;
    const size_t R = sh.R;
    FsTranscript tr = F::start_transcript(sh, root, claims, Q);
    const std::vector<W> rho = F::rho_powers(tr, R);
    memcpy(h_stage + d.root_at, root, 32);
    CombineDesc* hd = reinterpret_cast<CombineDesc*>(h_stage + d.jobs_at);
    W* hy = reinterpret_cast<W*>(h_stage + d.y_at);
    W* hz = reinterpret_cast<W*>(h_stage + d.z_at);
    W* hw = reinterpret_cast<W*>(h_stage + d.w_at);
    hd[0].row0 = 0; hd[0].nrows = R; hd[0].woff = 0;
    memcpy(hw, rho.data(), R * sizeof(W));
    size_t off = R;
    for (size_t i = 0; i < claims.size(); i++) {
        const typename F::Claim& cl = claims[i];
        const std::vector<W> w = F::eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
        hd[i + 1].row0 = sh.off[cl.table]; hd[i + 1].nrows = w.size(); hd[i + 1].woff = off;
        memcpy(hw + off, w.data(), w.size() * sizeof(W));
        off += w.size();
        hy[i] = cl.value;
        F::store_low(hz + i * (size_t)sh.c, cl.point.data(), sh.c);
    }
    return tr;
}
// the host's order: a non-canonical element, the lowest claim whose evaluation fails, the lowest failing query; "" = accepted
inline std::string cells_reason(const u64* cells, size_t n) {
    if (cells[0] != PCSV_NONE) return reason_noncanonical((size_t)cells[0]);
    if (cells[1] != PCSV_NONE) return reason_evaluation((size_t)cells[1]);
    if (cells[2] == PCSV_NONE) return "";
    const size_t q = (size_t)(cells[2] / (n + 2)), kind = (size_t)(cells[2] % (n + 2));
    return kind == 0 ? reason_merkle(q) : kind == 1 ? reason_proximity(q) : reason_claim(kind - 2, q);
}

// the arena buffers of a group of openings under verification, and what its members take in all (u_total, unit_max: Row units)
template <class F> struct VerifyDev {
    char* stage;
    typename F::Row *u, *cols, *enc, *tmp = nullptr, *W;
    u64 *leaves, *js, *cells;
    typename F::W* s;
};
struct VerifyTotals { size_t G, u_total, unit_max, rows, claims, jobs, nw; };
template <class F> VerifyDev<F> verify_alloc(hg_ctx* ctx, const Shape& sh, size_t Q, size_t stage_bytes, const VerifyTotals& t, size_t n_cells) {
    typedef typename F::Row Row;
    const size_t N = sh.N();
    VerifyDev<F> d;
    d.stage = ctx->alloc_n<char>(stage_bytes);
    d.u = ctx->alloc_n<Row>(t.u_total);
    d.cols = ctx->alloc_n<Row>(t.G * Q * sh.R);
    d.enc = ctx->alloc_n<Row>(t.rows * N);
    if (F::ntt_needs_tmp(sh.depth())) d.tmp = ctx->alloc_n<Row>(t.rows * N);
    d.W = ctx->alloc_n<Row>(N);
    d.leaves = ctx->alloc_n<u64>(4 * t.G * Q);
    d.s = ctx->alloc_n<typename F::W>(Q * t.jobs);
    d.js = ctx->alloc_n<u64>(t.G * Q);
    d.cells = ctx->alloc_n<u64>(n_cells);
    return d;
}
// Everything of a group that needs no column index, behind the uploads of its openings and of its staged copy: it runs while the
// host hashes the u_i. The order of the leaf sponge and the inner products is the field's.
template <class F> void verify_enqueue(hg_ctx* ctx, int cls, hipStream_t st, unsigned canon_cap, const u64* d_set, const VerifyDev<F>& d, const VbGroup& vg, const VerifyTotals& t,
                                       size_t n_cells) {
    const VbMember* d_mem = reinterpret_cast<const VbMember*>(d.stage);
    hip_check(hipMemsetAsync(d.cells, 0xff, n_cells * 8, st), "memset");
    hip_check(hipMemsetAsync(d.enc, 0, (t.rows << vg.depth) * sizeof(typename F::Row), st), "memset");
    F::canon(ctx, cls, st, canon_cap, d_set, d_mem, vg, t.u_total, t.unit_max, d.u, d.cols, d.enc, d.cells);
    if (t.claims) F::eval(ctx, cls, st, d_mem, vg, t.claims, d.u, d.stage, d.cells);
    F::ntt(ctx, cls, st, d.enc, d.tmp, d.W, vg.depth, t.rows, t.rows);
    if (!F::LEAF_AFTER_DOTS) F::leaf(ctx, cls, st, d_mem, vg, d.cols, d.leaves);
    F::dots(ctx, cls, st, d_mem, vg, t.jobs, t.nw, d.cols, d.stage, d.s);
    if (F::LEAF_AFTER_DOTS) F::leaf(ctx, cls, st, d_mem, vg, d.cols, d.leaves);
}
// the column indices of every member up, the query kernel behind them
template <class F> void verify_enqueue_query(hg_ctx* ctx, int cls, hipStream_t st, const u64* d_set, const VerifyDev<F>& d, const VbGroup& vg, const VerifyTotals& t, const u64* hj) {
    hip_check(hipMemcpyAsync(d.js, hj, t.G * vg.Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
    F::query(ctx, cls, st, d_set, reinterpret_cast<const VbMember*>(d.stage), vg, t.jobs, d.leaves, d.s, d.enc, d.js, d.stage, d.cells);
}

// The device verifier of one opening: a group of one member, whose opening in the arena is the set. Everything but the last kernel
// needs no column index, so it is enqueued first and runs while the host hashes the u_i; the indices follow on the same stream, then
// the three result cells come back: one synchronisation.
template <class F>
std::string verify_flow(hg_ctx* ctx, const Shape& sh, const uint8_t root[32], const std::vector<typename F::Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), N = sh.N(), n = claims.size();
    const std::string who(F::VERIFY_NAME);
    const std::string bad_len = length_reason(len, F::opening_bytes(sh, n, Q));
    if (!bad_len.empty()) return bad_len;
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    // the member's descriptor and its block in one staged copy
    const size_t nw = weights_of<F>(sh, claims), u_units = F::U_ROWS * C * (n + 1);
    const VerifyTotals t{1, u_units, u_units + Q * sh.R, F::U_ROWS * (n + 1), n, n + 1, nw};
    VbMember desc{};   // (every offset into the set and the arena buffers is 0)
    desc.n = n;
    std::vector<char> stage(member_block_layout<F>(desc, sh, n, nw, sizeof(VbMember)));
    static_assert(sizeof(VbMember) % F::ALIGN == 0, "the block starts at a multiple of the alignment");
    memcpy(stage.data(), &desc, sizeof(VbMember));
    FsTranscript tr = member_block_fill<F>(stage.data(), desc, sh, root, claims, Q);
    u64* d_proof;
    VerifyDev<F> d;
    try {
        d_proof = ctx->alloc_n<u64>(len / 8);
        d = verify_alloc<F>(ctx, sh, Q, stage.size(), t, 4);
    } catch (const std::exception& e) {
        throw Error(std::string("the context's arena cannot hold the opening (") + e.what() + ")");
    }
    Drain drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
    const int cls = ctx->prof_class(F::CLS_VERIFY, false);
    ctx->prof_stream = st;
    const VbGroup vg{1, (u64)Q, (u64)sh.R, (u64)query_stride<F>(sh), sh.c, sh.depth()};
    hip_check(hipMemcpyAsync(d_proof, proof, len, hipMemcpyHostToDevice, st), "upload opening");
    hip_check(hipMemcpyAsync(d.stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload claims");
    verify_enqueue<F>(ctx, cls, st, 4096, d_proof, d, vg, t, 4);
    // the host's share, beside the kernels: the u_i into the transcript, the column indices out of it
    F::absorb_opening(tr, proof, C * (n + 1));
    const std::vector<size_t> js = F::squeeze_indices(tr, N, Q);
    const std::vector<u64> hj(js.begin(), js.end());
    verify_enqueue_query<F>(ctx, cls, st, d_proof, d, vg, t, hj.data());
    u64 cells[4];
    hip_check(hipMemcpyAsync(cells, d.cells, 32, hipMemcpyDeviceToHost, st), "download verdict");
    hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
    hip_check(hipGetLastError(), (who + ": launch").c_str());
    ctx->prof_collect();
    return cells_reason(cells, n);
}

// The block of a folded opening's body, whose layout is that of a member of one claim and 2 R weights: the root, two jobs over all R
// rows (the powers of rho', the combined weights), the value sum_t delta^t Y_t and the point rho[..c), all from the header H
template <class F, class Header> void folded_block_fill(char* h_stage, const VbMember& d, const Shape& sh, const uint8_t root[32], const Header& H) {
    typedef typename F::W W;
    const size_t R = sh.R;
    memcpy(h_stage + d.root_at, root, 32);
    CombineDesc* hd = reinterpret_cast<CombineDesc*>(h_stage + d.jobs_at);
    hd[0].row0 = 0; hd[0].nrows = R; hd[0].woff = 0;
    hd[1].row0 = 0; hd[1].nrows = R; hd[1].woff = R;
    memcpy(h_stage + d.y_at, &H.y, sizeof(W));
    if (sh.c) F::store_low(reinterpret_cast<W*>(h_stage + d.z_at), H.lo.data(), sh.c);
    memcpy(h_stage + d.w_at, H.rho_pw.data(), R * sizeof(W));
    memcpy(h_stage + d.w_at + R * sizeof(W), H.w.data(), R * sizeof(W));
}

// The device verifier of a folded opening. The header is host scalar work (the field's folded_header); its body is an opening of one
// claim - all R rows under the combined weights, at rho[..c), with the value sum_t delta^t Y_t - and goes through verify_flow's kernels
// as a group of one member whose opening starts behind the header. The kernels run whatever the header's checks gave: an element of the
// body that is not canonical is reported ahead of a failing round, as the host verifier does.
template <class F>
std::string verify_folded_flow(hg_ctx* ctx, const Shape& sh, const uint8_t root[32], const std::vector<typename F::Claim>& claims, size_t Q, const uint8_t* proof, size_t len) {
    const size_t C = sh.C(), N = sh.N(), R = sh.R, hb = F::folded_header_bytes(sh);
    const std::string who(F::VERIFY_FOLDED_NAME);
    const std::string bad_len = length_reason(len, F::folded_opening_bytes(sh, Q));
    if (!bad_len.empty()) return bad_len;
    auto H = F::folded_header(sh, root, claims, Q, proof);
    if (H.noncanonical != ~(size_t)0) return reason_noncanonical(H.noncanonical);
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t nw = 2 * R, u_units = F::U_ROWS * C * 2;
    const VerifyTotals t{1, u_units, u_units + Q * R, F::U_ROWS * 2, 1, 2, nw};
    VbMember desc{};
    desc.n = 1;
    desc.proof = hb / 8;
    std::vector<char> stage(member_block_layout<F>(desc, sh, 1, nw, sizeof(VbMember)));
    memcpy(stage.data(), &desc, sizeof(VbMember));
    folded_block_fill<F>(stage.data(), desc, sh, root, H);
    u64* d_proof;
    VerifyDev<F> d;
    try {
        d_proof = ctx->alloc_n<u64>(len / 8);
        d = verify_alloc<F>(ctx, sh, Q, stage.size(), t, 4);
    } catch (const std::exception& e) {
        throw Error(std::string("the context's arena cannot hold the opening (") + e.what() + ")");
    }
    Drain drain{st};   // (drains on an error; after the synchronisation below its own is one more, on an idle stream)
    const int cls = ctx->prof_class(F::CLS_VERIFY, false);
    ctx->prof_stream = st;
    const VbGroup vg{1, (u64)Q, (u64)R, (u64)query_stride<F>(sh), sh.c, sh.depth()};
    hip_check(hipMemcpyAsync(d_proof, proof, len, hipMemcpyHostToDevice, st), "upload opening");
    hip_check(hipMemcpyAsync(d.stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload claims");
    verify_enqueue<F>(ctx, cls, st, 4096, d_proof, d, vg, t, 4);
    F::absorb_opening(H.tr, proof + hb, 2 * C);
    const std::vector<size_t> js = F::squeeze_indices(H.tr, N, Q);
    const std::vector<u64> hj(js.begin(), js.end());
    verify_enqueue_query<F>(ctx, cls, st, d_proof, d, vg, t, hj.data());
    u64 cells[4];
    hip_check(hipMemcpyAsync(cells, d.cells, 32, hipMemcpyDeviceToHost, st), "download verdict");
    hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
    hip_check(hipGetLastError(), (who + ": launch").c_str());
    ctx->prof_collect();
    if (cells[0] != PCSV_NONE) return reason_noncanonical(hb + (size_t)cells[0]);
    if (!H.reason.empty()) return H.reason;
    return cells_reason(cells, 1);
}

// The device verifier of a run of openings. The items whose length is right are cut into groups (the option verify_batch_group,
// VB_PCS_BUDGET over what a member takes, the rows the field's NTT takes on its four-step path, the field's limit of one inner-product
// launch). A group: its openings gathered into a page-locked set on the host threads and copied on the upload stream; every member's
// transcript start, rho powers and weight tables written into one staged copy, one member a task; the index-free kernels, one launch
// each over all members; the members' u_i hashed on the host threads meanwhile; all indices up, the query kernel, three cells a
// member down: one synchronisation a group. The next group's openings are gathered and copied into the other set before that
// synchronisation, under this group's kernels.
// `folded`: the items are folded openings. A member's block is then prepared from its header - the field's folded_header on the host
// threads, one member a task - as that of an opening of one claim that starts behind the header (folded_block_fill: what
// verify_folded_flow writes for its one member); everything else is the same pass. A member whose header holds a word that is not
// canonical rides along on a block of zeros and is given the header's reason.
template <class F>
std::vector<std::string> verify_batch_flow(const char* who_c, hg_ctx* ctx, const Shape& sh, const std::vector<typename F::VerifyItem>& items, size_t Q, bool folded = false) {
    typedef typename F::Row Row;
    typedef typename F::W W;
    typedef typename F::VerifyItem Item;
    const std::string who(who_c);
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int depth = sh.depth();
    const bool four_step = depth >= 8 && depth <= 16;
    const size_t hb = folded ? F::folded_header_bytes(sh) : 0;   // where a member's body starts in its opening
    auto claims_of = [&](const Item& it) { return folded ? (size_t)1 : it.claims->size(); };   // the claims of the body
    std::vector<std::string> why(items.size());
    std::vector<size_t> good;   // the items that reach the device
    for (size_t i = 0; i < items.size(); i++) {
        why[i] = length_reason(items[i].len, folded ? F::folded_opening_bytes(sh, Q) : F::opening_bytes(sh, items[i].claims->size(), Q));
        if (why[i].empty()) good.push_back(i);
    }
    if (good.empty()) return why;
    // what a member takes: its opening in a set; u, columns, enc rows (and the NTT's temporary), s, leaves and indices in the arena
    auto rows_of = [](size_t n) { return F::U_ROWS * (n + 1); };
    auto bytes_of = [&](size_t n, size_t len) {
        return len + sizeof(W) * (C + Q) * (n + 1) + sizeof(Row) * (Q * R + rows_of(n) * N * (F::ntt_needs_tmp(depth) ? 2 : 1)) + 8 * 5 * Q;
    };
    size_t cap = VB_MAX_GROUP;
    if (ctx->verify_batch_group > 0) cap = std::min<size_t>(cap, (size_t)ctx->verify_batch_group);
    constexpr size_t NTT_ROWS = 65535;   // the batch is the y extent of the four-step grids
    const size_t dots_rows = F::dots_max_rows(Q);
    std::vector<std::pair<size_t, size_t>> groups;   // [first, last) of good
    for (size_t a = 0; a < good.size();) {
        size_t b = a, bytes = 0, rows = 0;
        while (b < good.size() && b - a < cap) {
            const size_t n = claims_of(items[good[b]]);
            if (b > a && (bytes + bytes_of(n, items[good[b]].len) > VB_PCS_BUDGET || (four_step && rows + rows_of(n) > NTT_ROWS) || rows + rows_of(n) > dots_rows)) break;
            bytes += bytes_of(n, items[good[b]].len);
            rows += rows_of(n);
            b++;
        }
        groups.push_back({a, b});
        a = b;
    }
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    hipStream_t st = ctx->stream;
    std::vector<u64> hj, cells;   // (declared ahead of the guard: copies of them may be queued when it drains)
    Drain drain_up{B->up}, drain{st};   // (the upload stream as well: no kernel on a set left behind)
    hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());        // (the device pass of hipcc ignores the pragmas)
    const int cls = ctx->prof_class(F::CLS_VERIFY_BATCH, false);
    ctx->prof_stream = st;

    typedef decltype(F::folded_header(sh, nullptr, *items[0].claims, Q, nullptr)) Header;
    struct Member { size_t idx, n, nw; FsTranscript tr; std::string error, header_reason; size_t noncanonical = ~(size_t)0; };
    auto rethrow = [&](const std::vector<Member>& mem) {
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
    };
    // the openings of group g into set g & 1, at word offsets that the descriptors repeat
    auto proof_offsets = [&](size_t g) {
        std::vector<size_t> off;
        size_t at = 0;
        for (size_t x = groups[g].first; x < groups[g].second; x++) { off.push_back(at); at += items[good[x]].len / 8; }
        off.push_back(at);
        return off;
    };
    auto stage = [&](size_t g) {
        const std::vector<size_t> off = proof_offsets(g);
        std::vector<BatchBlob> blobs;
        for (size_t x = groups[g].first; x < groups[g].second; x++) blobs.push_back(BatchBlob{items[good[x]].proof, items[good[x]].len, off[x - groups[g].first]});
        batch_stage_blobs(B, (int)(g & 1), blobs, off.back(), nthr, who_c);
    };
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr
    double t_stage = omp_get_wtime();
    stage(0);
    t_stage = omp_get_wtime() - t_stage;
    for (size_t g = 0; g < groups.size(); g++) {
        const double t0 = omp_get_wtime();
        const size_t G = groups[g].second - groups[g].first;
        const int set = (int)(g & 1);
        std::vector<Member> mem(G);
        std::vector<VbMember> desc(G);
        const std::vector<size_t> poff = proof_offsets(g);
        // the layout of the staged copy: the descriptors, then every member's block, and of the arena buffers
        VerifyTotals t{G, 0, 0, 0, 0, 0, 0};
        size_t at = align_up<F>(G * sizeof(VbMember));
        for (size_t m = 0; m < G; m++) {
            Member& x = mem[m];
            const Item& it = items[good[groups[g].first + m]];
            x.idx = good[groups[g].first + m];
            x.n = claims_of(it);
            x.nw = folded ? 2 * R : weights_of<F>(sh, *it.claims);
            VbMember& d = desc[m];
            d.proof = poff[m] + hb / 8; d.u = t.u_total; d.cols = m * Q * R; d.enc_row = t.rows;
            d.n = x.n; d.claim0 = t.claims; d.job0 = t.claims + m;
            at = member_block_layout<F>(d, sh, x.n, x.nw, at);
            const size_t u_units = F::U_ROWS * C * (x.n + 1);
            t.u_total += u_units;
            t.unit_max = std::max(t.unit_max, u_units + Q * R);
            t.rows += rows_of(x.n);
            t.claims += x.n;
            t.nw += x.nw;
        }
        t.jobs = t.claims + G;
        const size_t stage_bytes = at;
        char* h_stage = batch_desc_host(B, stage_bytes);   // (the previous group's copy of it was waited for)
        memcpy(h_stage, desc.data(), G * sizeof(VbMember));
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                const Item& it = items[x.idx];
                if (!folded) { x.tr = member_block_fill<F>(h_stage, desc[mq], sh, it.root, *it.claims, Q); continue; }
                Header H = F::folded_header(sh, it.root, *it.claims, Q, it.proof);
                x.noncanonical = H.noncanonical;
                if (H.noncanonical != ~(size_t)0) { memset(h_stage + desc[mq].root_at, 0, desc[mq].w_at + x.nw * sizeof(W) - desc[mq].root_at); continue; }
                folded_block_fill<F>(h_stage, desc[mq], sh, it.root, H);
                x.header_reason = std::move(H.reason);
                x.tr = std::move(H.tr);
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        rethrow(mem);
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        VerifyDev<F> d;
        try {
            d = verify_alloc<F>(ctx, sh, Q, stage_bytes, t, 3 * G);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold " + (G == 1 ? "the opening at index " + std::to_string(mem[0].idx) : "a group of " + std::to_string(G) + " openings: lower verify_batch_group") +
                        " (" + e.what() + ")");
        }
        const u64* d_set = B->d_in[set];
        const VbGroup vg{(u64)G, (u64)Q, (u64)R, (u64)query_stride<F>(sh), sh.c, depth};
        hip_check(hipStreamWaitEvent(st, B->ev[set], 0), "hipStreamWaitEvent");   // the set's openings are up
        hip_check(hipMemcpyAsync(d.stage, h_stage, stage_bytes, hipMemcpyHostToDevice, st), "upload claims");
        verify_enqueue<F>(ctx, cls, st, 1024, d_set, d, vg, t, 3 * G);
        // the host's share, beside the kernels: every member's u_i into its transcript, its column indices out of it
        const double t2 = omp_get_wtime();
        hj.assign(G * Q, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                if (x.noncanonical != ~(size_t)0) continue;   // (its indices stay 0: its cells are not read)
                F::absorb_opening(x.tr, items[x.idx].proof + hb, C * (x.n + 1));
                const std::vector<size_t> js = F::squeeze_indices(x.tr, N, Q);
                for (size_t q = 0; q < Q; q++) hj[(size_t)mq * Q + q] = js[q];
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        rethrow(mem);
        const double t3 = omp_get_wtime();
        verify_enqueue_query<F>(ctx, cls, st, d_set, d, vg, t, hj.data());
        cells.assign(3 * G, 0);
        hip_check(hipMemcpyAsync(cells.data(), d.cells, 3 * G * 8, hipMemcpyDeviceToHost, st), "download verdicts");
        const double t4 = omp_get_wtime();
        if (g + 1 < groups.size()) stage(g + 1);   // into the other set, under this group's kernels
        const double t5 = omp_get_wtime();
        hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
        if (times)
            fprintf(stderr, "[hg pcs] group %zu of %zu members: gather and copy of its openings %.2f ms, transcripts and weights %.2f, enqueue %.2f, hash %.2f, "
                            "query enqueue %.2f, next group's gather %.2f, wait %.2f\n", g, G, t_stage * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3,
                    (t5 - t4) * 1e3, (omp_get_wtime() - t5) * 1e3);
        t_stage = t5 - t4;
        hip_check(hipGetLastError(), (who + ": launch").c_str());
        ctx->prof_collect();
        for (size_t m = 0; m < G; m++) {
            const Member& x = mem[m];
            const u64* cell = cells.data() + 3 * m;
            // a folded opening in the single call's order: a header word, a body word, the header's checks, the body's
            if (x.noncanonical != ~(size_t)0) why[x.idx] = reason_noncanonical(x.noncanonical);
            else if (folded && cell[0] != PCSV_NONE) why[x.idx] = reason_noncanonical(hb + (size_t)cell[0]);
            else if (!x.header_reason.empty()) why[x.idx] = x.header_reason;
            else why[x.idx] = cells_reason(cell, x.n);
        }
    }
    return why;
}

// The device committer of a run. A group: one allocation for its members' raw and encoded rows (where the field keeps freed ones, a
// spare that fits), the tables uploaded straight into it (or, `words`, the witness words, which the field's stage step lifts), the
// stage kernel, the encoding (all G R rows in one call, or in slices of whole members through one slice's temporary where the field
// sets NTT_TMP), the leaf hashes, the tree levels (per level while a level has more than a workgroup's nodes, then one workgroup a
// member), one download of all trees and flags, one synchronisation.
template <class F>
std::vector<Commitment*> commit_batch_flow(const char* who_c, hg_ctx* ctx, const Shape& sh, const u64* const* tables, size_t n, bool words) {
    typedef typename F::Row Row;
    const std::string who(who_c);
    const size_t C = sh.C(), N = sh.N(), R = sh.R, nt = sh.nvars.size();
    const int log2n = sh.depth();
    if (R > 65535) throw Error(who + ": more than 65535 rows (choose a larger log2_row)");
    const size_t tree_words = 8 * N;   // 2N nodes of 4 words: the 2N - 1 of a tree and one unused
    const size_t member_bytes = F::commit_member_bytes(R, C, N), slab_bytes = sizeof(Row) * (R * C + R * N);
    // the NTT: the batch is the y extent of its four-step grids, and a slice is at most a group
    const std::vector<std::pair<size_t, size_t>> groups = cut_groups(ctx, n, [&](size_t) { return member_bytes; }, R, 65535, F::COMMIT_BUDGET);
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    std::vector<std::unique_ptr<Commitment>> made;
    std::vector<u64> h_out;   // (declared ahead of the guard: a copy into it may be queued when it drains)
    Drain drain{st};
    hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    const int cls = ctx->prof_class(F::CLS_COMMIT_BATCH, false);
    ctx->prof_stream = st;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr
    for (const auto& grp : groups) {
        const double t0 = omp_get_wtime();
        const size_t first = grp.first, G = grp.second - grp.first;
        const size_t slice = F::NTT_TMP ? std::min(G, std::max<size_t>(1, F::NTT_TMP / (R * N * sizeof(Row)))) : G;   // members a call of the NTT
        std::shared_ptr<Slab> slab = std::make_shared<Slab>();
        F::slab_spare(ctx, *slab, G * slab_bytes);   // a freed group's allocation, if the field keeps them and one fits
        if (!slab->p) {
            hip_check(hipMalloc((void**)&slab->p, G * slab_bytes), "hipMalloc(pcs rows and encoded matrices of a group)");
            slab->bytes = G * slab_bytes;
        }
        Row* d_rows = reinterpret_cast<Row*>(slab->p);
        Row* d_M = d_rows + G * R * C;
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        Row *tmp, *W;
        u64 *d_out, *d_words = nullptr;
        const size_t out_words = G * tree_words + (G + 1) / 2;   // the trees, then one 32-bit flag a member
        try {
            tmp = ctx->alloc_n<Row>(slice * R * N);
            W = ctx->alloc_n<Row>(N);
            d_out = ctx->alloc_n<u64>(out_words);
            if (words) d_words = ctx->alloc_n<u64>(G * R * C);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold a group of " + std::to_string(G) + " commitments: lower verify_batch_group (" + e.what() + ")");
        }
        unsigned* d_flags = reinterpret_cast<unsigned*>(d_out + G * tree_words);
        hip_check(hipMemsetAsync(d_flags, 0, ((G + 1) / 2) * 8, st), "memset");
        for (size_t m = 0; m < G; m++)
            for (size_t t = 0; t < nt; t++) {
                const size_t len = (size_t)1 << sh.nvars[t], at = (m * R + sh.off[t]) * C;
                if (words) hip_check(hipMemcpyAsync(d_words + at, tables[(first + m) * nt + t], len * 8, hipMemcpyHostToDevice, st), "upload tables");
                else hip_check(hipMemcpyAsync(d_rows + at, tables[(first + m) * nt + t], len * sizeof(Row), hipMemcpyHostToDevice, st), "upload tables");
            }
        const double t2 = omp_get_wtime();
        F::stage(ctx, cls, st, G, R, sh.c, d_words, d_rows, d_M, d_flags);
        F::ntt(ctx, cls, st, d_M, tmp, W, log2n, G * R, slice * R);
        F::leaf_hash(ctx, cls, st, d_M, G, log2n, R, d_out, tree_words);
        ctx->prof_begin(cls, (double)G * N * 96);
        merkle_levels_device_batch(st, d_out, tree_words, N, G);
        ctx->prof_end();
        h_out.resize(out_words);
        hip_check(hipMemcpyAsync(h_out.data(), d_out, out_words * 8, hipMemcpyDeviceToHost, st), "download trees and flags");
        const double t3 = omp_get_wtime();
        hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
        const double t4 = omp_get_wtime();
        hip_check(hipGetLastError(), (who + ": launch").c_str());
        ctx->prof_collect();
        const unsigned* flags = reinterpret_cast<const unsigned*>(h_out.data() + G * tree_words);
        for (size_t m = 0; m < G; m++)
            if (flags[m]) throw Error(who + ": index " + std::to_string(first + m) + ": " + F::NOT_BELOW);
        for (size_t m = 0; m < G; m++) {
            std::unique_ptr<Commitment> cm(new Commitment());
            cm->field = F::FIELD;
            cm->sh = sh;
            cm->ctx = ctx;
            cm->d_rows = reinterpret_cast<u64*>(d_rows + m * R * C);
            cm->d_M = reinterpret_cast<u64*>(d_M + m * R * N);
            cm->owner = slab;
            const uint8_t* tree = reinterpret_cast<const uint8_t*>(h_out.data() + m * tree_words);
            cm->tree.assign(tree, tree + 32 * (2 * N - 1));
            made.push_back(std::move(cm));
        }
        if (times)
            fprintf(stderr, "[hg pcs] %scommit group of %zu members%s: allocation %.2f ms, uploads %.2f, enqueue %.2f, wait %.2f, trees into the handles %.2f\n", F::TIMES_TAG, G,
                    F::NTT_TMP ? (" (" + std::to_string(slice) + " a slice of the encoding)").c_str() : "", (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3,
                    (omp_get_wtime() - t4) * 1e3);
    }
    std::vector<Commitment*> out;
    for (auto& cm : made) out.push_back(cm.release());
    return out;
}

// The row combinations of one opening: the job table and the weights in one staged copy; job q's u vector is the q-th
template <class F>
void combine_flow(const Commitment& cm, const std::vector<typename F::Job>& jobs, typename F::W* u) {
    typedef typename F::Row Row;
    typedef typename F::W W;
    const std::string who(F::OPEN_NAME);
    hg_ctx* ctx = cm.ctx;
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    ctx->arena_reset();
    hipStream_t st = ctx->stream;
    const size_t C = cm.sh.C(), nj = jobs.size();
    if (nj > 65535) throw Error(who + ": more than 65534 claims");   // (at most 2^16 workgroups a job and, by the entry point, MAX_CLAIMS + 1 jobs: inside a grid's x)
    size_t nw = 0;
    for (const typename F::Job& j : jobs) nw += j.nrows;
    const size_t desc_bytes = align_up<F>(nj * sizeof(ObJob<Row>));
    std::vector<char> stage(desc_bytes + nw * sizeof(W));
    ObJob<Row>* hd = reinterpret_cast<ObJob<Row>*>(stage.data());
    size_t w_at = desc_bytes;
    for (size_t q = 0; q < nj; q++) {
        hd[q].src = reinterpret_cast<const Row*>(cm.d_rows) + (jobs[q].row0 << cm.sh.c); hd[q].nrows = jobs[q].nrows; hd[q].w_at = w_at; hd[q].u_at = q * C;
        memcpy(stage.data() + w_at, jobs[q].w.data(), jobs[q].nrows * sizeof(W));
        w_at += jobs[q].nrows * sizeof(W);
    }
    char* d_stage = ctx->alloc_n<char>(stage.size());
    W* d_u = ctx->alloc_n<W>(nj * C);
    const int cls = F::CLS_COMBINE ? ctx->prof_class(F::CLS_COMBINE, false) : -1;   // (-1: the field does not profile this call)
    ctx->prof_stream = st;
    hip_check(hipMemcpyAsync(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice, st), "upload weights");
    F::combine(ctx, cls, st, cm.sh.c, nj, nw, 0, reinterpret_cast<const ObJob<Row>*>(d_stage), d_stage, d_u);
    hip_check(hipMemcpyAsync(u, d_u, nj * C * sizeof(W), hipMemcpyDeviceToHost, st), "download combinations");
    hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
    hip_check(hipGetLastError(), (who + ": launch").c_str());
    ctx->prof_collect();
}

// The opened columns of one opening: cols[q][r] = M[r][js[q]]
template <class F>
void columns_flow(const Commitment& cm, const std::vector<size_t>& js, typename F::Row* cols) {
    typedef typename F::Row Row;
    const std::string who(F::OPEN_NAME);
    hg_ctx* ctx = cm.ctx;
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t st = ctx->stream;
    const size_t N = cm.sh.N(), R = cm.sh.R, Q = js.size();
    if (Q > 65535) throw Error(who + ": more than 65535 queries on the device");
    std::vector<u64> hj(js.begin(), js.end());
    u64* d_js = ctx->alloc_n<u64>(Q);
    Row* d_cols = ctx->alloc_n<Row>(Q * R);
    hip_check(hipMemcpyAsync(d_js, hj.data(), Q * 8, hipMemcpyHostToDevice, st), "upload column indices");
    F::gather_one(st, reinterpret_cast<const Row*>(cm.d_M), N, R, Q, d_js, d_cols);
    hip_check(hipMemcpyAsync(cols, d_cols, Q * R * sizeof(Row), hipMemcpyDeviceToHost, st), "download columns");
    hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
    hip_check(hipGetLastError(), (who + ": launch").c_str());
}

// The device opener of a run. A group: the host threads write every member's transcript start, rho powers, weight tables and table
// entries into one staged copy; the combinations, the evaluation checks and the big-endian u vectors run as one launch each; the u
// vectors and one cell a member come back (first synchronisation); the host threads hash each member's u_i, one member a thread; all
// indices go up, the gather writes the opened columns into the images, the images come back (second synchronisation); the host
// copies the siblings from each handle's tree into the gaps.
template <class F>
std::vector<Opened> open_batch_flow(const char* who_c, const char* single, hg_ctx* ctx, const std::vector<typename F::OpenItem>& items, size_t Q) {
    typedef typename F::Row Row;
    typedef typename F::W W;
    typedef typename F::Claim Claim;
    constexpr size_t RW = sizeof(Row) / 8, WW = sizeof(W) / 8;   // words of a row element and of a u element
    const std::string who(who_c);
    std::vector<Opened> res(items.size());
    if (items.empty()) return res;
    const Shape& sh = items[0].cm->sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R;
    const int depth = sh.depth();
    const size_t q_words = RW * query_stride<F>(sh);   // a query in the image: R elements and `depth` siblings of 4 words
    // what a member takes: its block of the staged copy, its u vectors and its image in the arena, its indices
    auto bytes_of = [&](size_t i) {
        const std::vector<Claim>& cl = *items[i].claims;
        return sizeof(ObMember<Row>) + (cl.size() + 1) * sizeof(ObJob<Row>) + cl.size() * (sizeof(ObClaim) + (size_t)(sh.c + 1) * sizeof(W)) + weights_of<F>(sh, cl) * sizeof(W) +
               4 * F::ALIGN + sizeof(W) * C * (cl.size() + 1) + F::opening_bytes(sh, cl.size(), Q) + 8 * Q + 16;
    };
    const std::vector<std::pair<size_t, size_t>> groups = cut_groups(ctx, items.size(), bytes_of, 0, 0);
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    hipStream_t st = ctx->stream;
    std::vector<u64> hj;   // (declared ahead of the guard: a copy of it may be queued when it drains)
    Drain drain{st};
    hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());        // (the device pass of hipcc ignores the pragmas)
    const int cls = ctx->prof_class(F::CLS_OPEN_BATCH, false);
    ctx->prof_stream = st;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr

    struct Member { size_t idx, n, nw, job0, claim0, y_at, z_at, w_at, img, u, u_words, len; FsTranscript tr; bool refused = false; std::string error; };
    auto rethrow = [&](const std::vector<Member>& mem) {
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
    };
    for (size_t g = 0; g < groups.size(); g++) {
        const double t0 = omp_get_wtime();
        const size_t G = groups[g].second - groups[g].first;
        std::vector<Member> mem(G);
        // the layout of the staged copy: the three tables, then every member's values, low coordinates and weights
        size_t jobs_total = 0, claims_total = 0, u_total = 0, img_total = 0, nw_total = 0;   // u_total, img_total: words
        for (size_t m = 0; m < G; m++) {
            Member& x = mem[m];
            x.idx = groups[g].first + m;
            x.n = items[x.idx].claims->size();
            x.nw = weights_of<F>(sh, *items[x.idx].claims);
            x.job0 = jobs_total; x.claim0 = claims_total; x.u = u_total; x.img = img_total;
            x.u_words = WW * C * (x.n + 1);
            x.len = F::opening_bytes(sh, x.n, Q);
            jobs_total += x.n + 1; claims_total += x.n; u_total += x.u_words; img_total += x.len / 8; nw_total += x.nw;
        }
        const size_t mem_at = 0, jobs_at = align_up<F>(G * sizeof(ObMember<Row>)), claims_at = jobs_at + align_up<F>(jobs_total * sizeof(ObJob<Row>));
        size_t at = claims_at + align_up<F>(claims_total * sizeof(ObClaim));
        for (Member& x : mem) {
            x.y_at = at;
            x.z_at = x.y_at + x.n * sizeof(W);
            x.w_at = x.z_at + x.n * (size_t)sh.c * sizeof(W);
            at = x.w_at + x.nw * sizeof(W);
        }
        const size_t stage_bytes = std::max<size_t>(at, F::ALIGN);
        char* h_stage = batch_desc_host(B, stage_bytes);   // (the previous group's copy of it was waited for)
        // results of the group, page-locked: the u vectors, the images, one cell a member
        const size_t hu_at = 0, himg_at = u_total * 8, hcell_at = himg_at + img_total * 8;
        char* h_out = batch_out_host(B, hcell_at + G * 8);
        const u64* h_u = reinterpret_cast<const u64*>(h_out + hu_at);
        uint8_t* h_img = reinterpret_cast<uint8_t*>(h_out + himg_at);
        const u64* h_cells = reinterpret_cast<const u64*>(h_out + hcell_at);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                const Commitment& cm = *items[x.idx].cm;
                const std::vector<Claim>& claims = *items[x.idx].claims;
                const Row* rows = reinterpret_cast<const Row*>(cm.d_rows);
                x.tr = F::start_transcript(sh, cm.root(), claims, Q);
                const std::vector<W> rho = F::rho_powers(x.tr, R);
                ObMember<Row>* hm = reinterpret_cast<ObMember<Row>*>(h_stage + mem_at) + mq;
                hm->M = reinterpret_cast<const Row*>(cm.d_M); hm->img = x.img; hm->u = x.u; hm->u_words = x.u_words;
                ObJob<Row>* hd = reinterpret_cast<ObJob<Row>*>(h_stage + jobs_at) + x.job0;
                ObClaim* hc = reinterpret_cast<ObClaim*>(h_stage + claims_at) + x.claim0;
                W* hy = reinterpret_cast<W*>(h_stage + x.y_at);
                W* hz = reinterpret_cast<W*>(h_stage + x.z_at);
                W* hw = reinterpret_cast<W*>(h_stage + x.w_at);
                hd[0].src = rows; hd[0].nrows = R; hd[0].w_at = x.w_at; hd[0].u_at = x.u / WW;
                memcpy(hw, rho.data(), R * sizeof(W));
                size_t off = R;
                for (size_t i = 0; i < x.n; i++) {
                    const Claim& cl = claims[i];
                    const std::vector<W> w = F::eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
                    hd[i + 1].src = rows + (sh.off[cl.table] << sh.c); hd[i + 1].nrows = w.size(); hd[i + 1].w_at = x.w_at + off * sizeof(W);
                    hd[i + 1].u_at = x.u / WW + (i + 1) * C;
                    memcpy(hw + off, w.data(), w.size() * sizeof(W));
                    off += w.size();
                    hy[i] = cl.value;
                    F::store_low(hz + i * (size_t)sh.c, cl.point.data(), sh.c);
                    hc[i].u_at = hd[i + 1].u_at; hc[i].z_at = x.z_at + i * (size_t)sh.c * sizeof(W); hc[i].y_at = x.y_at + i * sizeof(W);
                    hc[i].member = (u64)mq; hc[i].claim = (u64)i;
                }
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        rethrow(mem);
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        char* d_stage;
        u64 *d_u, *d_img, *d_js, *d_cells;
        try {
            d_stage = ctx->alloc_n<char>(stage_bytes);
            d_u = ctx->alloc_n<u64>(u_total);
            d_img = ctx->alloc_n<u64>(img_total);
            d_js = ctx->alloc_n<u64>(G * Q + G);
            d_cells = ctx->alloc_n<u64>(G);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold a group of " + std::to_string(G) + " openings: lower verify_batch_group (" + e.what() + ")");
        }
        const ObMember<Row>* d_mem = reinterpret_cast<const ObMember<Row>*>(d_stage + mem_at);
        if (jobs_total * ((C + F::TPB - 1) / F::TPB) > 0x7fffffffull)   // (a row combination takes a workgroup for every TPB columns)
            throw Error(who + ": a group of " + std::to_string(G) + " openings has too many row combinations for one launch: lower verify_batch_group");
        hip_check(hipMemcpyAsync(d_stage, h_stage, stage_bytes, hipMemcpyHostToDevice, st), "upload claims");
        hip_check(hipMemsetAsync(d_cells, 0xff, G * 8, st), "memset");
        F::combine(ctx, cls, st, sh.c, jobs_total, nw_total, u_total, reinterpret_cast<const ObJob<Row>*>(d_stage + jobs_at), d_stage, reinterpret_cast<W*>(d_u));
        if (claims_total) F::ob_eval(ctx, cls, st, reinterpret_cast<const ObClaim*>(d_stage + claims_at), claims_total, sh.c, reinterpret_cast<const W*>(d_u), d_stage, d_cells);
        F::emit(ctx, cls, st, d_mem, G, u_total, d_u, d_img);
        hip_check(hipMemcpyAsync(h_out + hu_at, d_u, u_total * 8, hipMemcpyDeviceToHost, st), "download combinations");
        hip_check(hipMemcpyAsync(h_out + hcell_at, d_cells, G * 8, hipMemcpyDeviceToHost, st), "download evaluation checks");
        hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
        hip_check(hipGetLastError(), (who + ": launch").c_str());
        const double t2 = omp_get_wtime();
        // the host's share: every member's u_i into its transcript, its column indices out of it, one member a thread
        hj.assign(G * Q + G, 0);
        size_t active = 0;
        for (size_t m = 0; m < G; m++) {
            mem[m].refused = h_cells[m] != PCSV_NONE;
            hj[G * Q + m] = mem[m].refused ? 0 : 1;
            active += mem[m].refused ? 0 : 1;
        }
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            if (x.refused) continue;
            try {
                F::absorb_u(x.tr, h_u + x.u, x.u_words);
                const std::vector<size_t> js = F::squeeze_indices(x.tr, N, Q);
                for (size_t q = 0; q < Q; q++) hj[(size_t)mq * Q + q] = js[q];
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        rethrow(mem);
        const double t3 = omp_get_wtime();
        if (active) {
            hip_check(hipMemcpyAsync(d_js, hj.data(), hj.size() * 8, hipMemcpyHostToDevice, st), "upload column indices");
            F::gather(ctx, cls, st, d_mem, G, Q, R, N, q_words, active, d_js, d_img);
            hip_check(hipMemcpyAsync(h_img, d_img, img_total * 8, hipMemcpyDeviceToHost, st), "download openings");
            hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
            hip_check(hipGetLastError(), (who + ": launch").c_str());
        }
        ctx->prof_collect();
        const double t4 = omp_get_wtime();
        // the siblings from each handle's tree into the gaps; a refused member's reason
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long mq = 0; mq < (long long)G; mq++) {
            Member& x = mem[mq];
            try {
                Opened& out = res[x.idx];
                const Commitment& cm = *items[x.idx].cm;
                if (x.refused) {
                    const size_t i = (size_t)h_cells[mq];
                    out.refused = true;
                    out.reason = std::string(single) + ": claim " + std::to_string(i) + ": the value is not the evaluation of table " + std::to_string((*items[x.idx].claims)[i].table) +
                                 " at the point";
                    continue;
                }
                const uint8_t* image = h_img + 8 * x.img;
                out.bytes.assign(image, image + x.len);
                for (size_t q = 0; q < Q; q++) {
                    uint8_t* sib = out.bytes.data() + 8 * (x.u_words + q * q_words + RW * R);
                    size_t idx = (size_t)hj[(size_t)mq * Q + q];
                    for (int l = 0; l < depth; l++, idx >>= 1) memcpy(sib + 32 * l, cm.node(l, idx ^ 1), 32);
                }
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        rethrow(mem);
        if (times)
            fprintf(stderr, "[hg pcs] %sopen group %zu of %zu members: transcripts and weights %.2f ms, combine, checks and u back %.2f, hash %.2f, gather and images back %.2f, "
                            "siblings %.2f\n", F::TIMES_TAG, g, G, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (omp_get_wtime() - t4) * 1e3);
    }
    return res;
}

// The device opener of a run of folded openings (hg_pcs_open_folded_batch*). A group (cut_groups over what a member takes: its g, its
// two buffer pairs, its blocks of the staged copy and its image): the host threads start every member's transcript and write its claim
// rows and factor tables into one staged copy, one member a task; ONE launch builds all members' g; then, for every step of the
// reduction, ONE launch folds the live tables of all members (the member is the grid's z), one workgroup a member adds its partials,
// the 3 G sums and - where tables retire - the scalars come back in one copy each, and ONE SYNCHRONISATION serves the group; the host
// threads do every member's transcript arithmetic (the field's FoldProver, the single call's) and the G challenges - in the form the
// round kernel takes them, F::FoldChal - go up in one copy ahead of the next launch. A member whose running claim is not met is
// refused: it rides on in the launches - its buffers are its own, so no other member's bytes depend on it - and its results are
// ignored. The tail is open_batch_flow's on two jobs a member: the combinations, the u vectors back, the host threads hash them and
// squeeze the indices, the gather writes the columns into images whose body starts behind the header, the host writes header, u
// vectors and siblings. The lowest failing claim of the refused members comes from the combine and evaluation kernels over their
// claims, one cell a member.
// What the field gives beside the policy of the other flows: FoldProver (round / finish / body_jobs / write_u), the geometry a shape
// fixes (fold_g_tables, fold_tables), a member's block of the g kernel's staged copy (fold_gblock_bytes, fold_gblock_fill), the arena
// buffers (fold_alloc), the member table (fold_members), the launches (fold_g_launch, fold_launch) and their bytes.
template <class F>
std::vector<Opened> open_folded_batch_flow(const char* who_c, const char* single, hg_ctx* ctx, const std::vector<typename F::OpenItem>& items, size_t Q) {
    typedef typename F::Row Row;
    typedef typename F::W W;
    typedef typename F::Claim Claim;
    typedef typename F::FoldProver Prover;
    typedef typename F::FoldChal Chal;
    typedef typename F::FoldGMember GMember;
    constexpr size_t RW = sizeof(Row) / 8, WW = sizeof(W) / 8;   // words of a row element and of a u element
    const std::string who(who_c);
    std::vector<Opened> res(items.size());
    if (items.empty()) return res;
    const Shape& sh = items[0].cm->sh;
    const size_t C = sh.C(), N = sh.N(), R = sh.R, m = sh.nvars.size(), V = fold_rounds(sh), Wd = R << sh.c;
    const int depth = sh.depth();
    const size_t hb = F::folded_header_bytes(sh), len = F::folded_opening_bytes(sh, Q), q_words = RW * query_stride<F>(sh), body_at = hb / 8 + 2 * C * WW;   // (words)
    size_t max_len;
    const typename F::FoldGTables GA = F::fold_g_tables(sh, &max_len);
    const unsigned max_blocks = F::fold_max_blocks();
    // what a member takes: g, the buffer pairs (a half and a quarter of g for T and for g each), its sums, its challenge and its row
    // pointer, its blocks of the staged copy, its u vectors, its image and its indices
    const size_t tail_block = sizeof(ObMember<Row>) + 2 * sizeof(ObJob<Row>) + 2 * R * sizeof(W);
    auto bytes_of = [&](size_t i) {
        return sizeof(W) * (Wd + 2 * (Wd / 2 + 1) + 2 * (Wd / 4 + 1) + 2 * m + 3 + 2 * C) + sizeof(Chal) + sizeof(GMember) + 8 + F::fold_gblock_bytes(sh, GA, *items[i].claims) +
               tail_block + len + 8 * Q + 64;
    };
    const std::vector<std::pair<size_t, size_t>> groups = cut_groups(ctx, items.size(), bytes_of, 0, 0);
    hip_check(hipSetDevice(ctx->device), "hipSetDevice");
    VerifyBatchBufs* B = batch_bufs(ctx);
    hipStream_t st = ctx->stream;
    Drain drain{st};
    hip_check(hipStreamSynchronize(st), (who + ": synchronise").c_str());   // (the arena is reset below)
    [[maybe_unused]] const int nthr = std::max(1, hg_omp_threads());        // (the device pass of hipcc ignores the pragmas)
    const int cls = ctx->prof_class(F::CLS_FOLD_BATCH, false);
    ctx->prof_stream = st;
    const bool times = hg_times("pcs");   // HG_TIMES=pcs: where a group's wall clock goes, on stderr

    struct Member {
        size_t idx, block_at;
        std::unique_ptr<Prover> P;
        std::vector<W> T, Gs, G1;
        bool refused = false;
        size_t failing = 0;
        std::string error;
    };
    auto rethrow = [&](const std::vector<Member>& mem) {
        for (const Member& x : mem)
            if (!x.error.empty()) throw Error(who + ": index " + std::to_string(x.idx) + ": " + x.error);
    };
    for (size_t g = 0; g < groups.size(); g++) {
        const double t0 = omp_get_wtime();
        const size_t G = groups[g].second - groups[g].first;
        std::vector<Member> mem(G);
        // the staged copy: the g kernel's member table, the row pointers, the challenges, the members' blocks; then the tail's member and
        // job tables, its weights, and the indices with the members' flags behind them
        const size_t rows_at = align_up<F>(G * sizeof(GMember)), r_at = rows_at + align_up<F>(G * 8);
        size_t at = r_at + align_up<F>(G * sizeof(Chal)), claims_total = 0;
        for (size_t k = 0; k < G; k++) {
            mem[k].idx = groups[g].first + k;
            mem[k].block_at = at;
            at += F::fold_gblock_bytes(sh, GA, *items[mem[k].idx].claims);
            claims_total += items[mem[k].idx].claims->size();
        }
        const size_t g_bytes = at, tmem_at = at, tjob_at = tmem_at + align_up<F>(G * sizeof(ObMember<Row>)), tw_at = tjob_at + align_up<F>(2 * G * sizeof(ObJob<Row>)),
                     js_at = tw_at + 2 * G * R * sizeof(W), stage_bytes = js_at + (G * Q + G) * 8;
        char* h_stage = batch_desc_host(B, stage_bytes);   // (the previous group's copies of it were waited for)
        // results of the group, page-locked: the sums, the scalars, the u vectors, the images
        const size_t hsum_at = 0, hscal_at = hsum_at + 3 * G * sizeof(W), hu_at = hscal_at + 2 * m * G * sizeof(W), himg_at = hu_at + 2 * C * G * sizeof(W);
        char* h_out = batch_out_host(B, himg_at + G * len);
        const W* h_sums = reinterpret_cast<const W*>(h_out + hsum_at);
        const W* h_scal = reinterpret_cast<const W*>(h_out + hscal_at);
        const W* h_u = reinterpret_cast<const W*>(h_out + hu_at);
        const uint8_t* h_img = reinterpret_cast<const uint8_t*>(h_out + himg_at);
        Chal* h_r = reinterpret_cast<Chal*>(h_stage + r_at);
        u64* h_js = reinterpret_cast<u64*>(h_stage + js_at);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long k = 0; k < (long long)G; k++) {
            Member& x = mem[k];
            try {
                const Commitment& cm = *items[x.idx].cm;
                const std::vector<Claim>& claims = *items[x.idx].claims;
                x.P.reset(new Prover(sh, cm.root(), claims, Q));
                x.T.assign(m, W());
                x.Gs.assign(m, W());
                F::fold_gblock_fill(h_stage, reinterpret_cast<GMember*>(h_stage)[k], x.block_at, sh, GA, claims, x.P->bpow, x.G1);
                reinterpret_cast<const Row**>(h_stage + rows_at)[k] = reinterpret_cast<const Row*>(cm.d_rows);
                h_r[k] = F::fold_chal(x.P->r);
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        rethrow(mem);
        const double t1 = omp_get_wtime();
        ctx->arena_reset();
        char* d_stage;
        typename F::FoldBufs buf;
        W* d_u;
        u64* d_img;
        try {
            d_stage = ctx->alloc_n<char>(stage_bytes);
            buf = F::fold_alloc(ctx, sh, G, max_blocks);
            d_u = ctx->alloc_n<W>(G * 2 * C);
            d_img = ctx->alloc_n<u64>(G * len / 8);
        } catch (const std::exception& e) {
            throw Error(who + ": the context's arena cannot hold a group of " + std::to_string(G) + " reductions: lower verify_batch_group (" + e.what() + ")");
        }
        const typename F::FoldMembers M = F::fold_members(sh, reinterpret_cast<const Row* const*>(d_stage + rows_at), reinterpret_cast<const Chal*>(d_stage + r_at));
        hip_check(hipMemcpyAsync(d_stage, h_stage, g_bytes, hipMemcpyHostToDevice, st), "upload claims");
        ctx->prof_begin(cls, (double)G * Wd * sizeof(W) + (double)g_bytes);
        F::fold_g_launch(st, max_blocks, GA, max_len, G, M, d_stage, buf);
        ctx->prof_end();
        // the steps of the reduction: every member is in the same one at the same time
        size_t round_launches = 0, round_syncs = 0;
        double t_host = 0;
        for (size_t j = 0; j <= V; j++) {
            bool retire;
            size_t max_units, entries;
            const typename F::FoldTables A = F::fold_tables(sh, j, &retire, &max_units, &entries);
            retire |= j == 0 && GA.n1 != 0;   // the elements of the one-element tables come back with step 0
            if (A.nt) {
                if (j > 0) hip_check(hipMemcpyAsync(d_stage + r_at, h_r, G * sizeof(Chal), hipMemcpyHostToDevice, st), "upload the round's challenges");
                ctx->prof_begin(cls, (double)G * F::fold_step_bytes(j, entries));
                F::fold_launch(st, max_blocks, sh, j, A, max_units, G, M, buf, j < V);
                ctx->prof_end();
                round_launches++;
                if (j < V) hip_check(hipMemcpyAsync(h_out + hsum_at, buf.sums, 3 * G * sizeof(W), hipMemcpyDeviceToHost, st), "download the round's sums");
            }
            if (retire) hip_check(hipMemcpyAsync(h_out + hscal_at, buf.scal, 2 * m * G * sizeof(W), hipMemcpyDeviceToHost, st), "download the retired tables' scalars");
            if (A.nt || retire) {
                hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
                hip_check(hipGetLastError(), (who + ": launch").c_str());
                round_syncs++;
            }
            const double th = omp_get_wtime();
#pragma omp parallel for schedule(static) num_threads(std::min<int>(nthr, (int)G))
            for (long long k = 0; k < (long long)G; k++) {
                Member& x = mem[k];
                if (x.refused) continue;
                try {
                    const W* sc = h_scal + 2 * m * (size_t)k;
                    for (size_t t = 0; t < m; t++) {
                        if (j == 0 && sh.nvars[t] == 0) { x.T[t] = sc[2 * t]; x.Gs[t] = x.G1[t]; }
                        if (j > 0 && (size_t)sh.nvars[t] == j) { x.T[t] = sc[2 * t]; x.Gs[t] = sc[2 * t + 1]; }
                    }
                    W s[3] = {W(), W(), W()};
                    if (A.nt && j < V) memcpy(s, h_sums + 3 * (size_t)k, sizeof(s));
                    x.refused = j < V ? !x.P->round(sh, j, s, x.T, x.Gs) : !x.P->finish(sh, x.T, x.Gs);
                    h_r[k] = F::fold_chal(x.P->r);
                } catch (const std::exception& e) { x.error = e.what(); }
            }
            rethrow(mem);
            t_host += omp_get_wtime() - th;
        }
        ctx->prof_collect();
        if (hg_debug("plan"))   // (read at every call: the tests switch it per case)
            fprintf(stderr, "[hg plan] %s members=%zu V=%zu round_launches=%zu round_syncs=%zu tables=%zu claims=%zu\n", F::PLAN_FOLD_BATCH, G, V, round_launches, round_syncs, m,
                    claims_total);
        const double t2 = omp_get_wtime();
        // the refused members: their claims through the row combinations and the evaluation checks, the lowest failing one in a cell a member
        std::vector<size_t> bad;
        for (size_t k = 0; k < G; k++)
            if (mem[k].refused) bad.push_back(k);
        if (!bad.empty()) {
            size_t nc = 0, nw = 0;
            for (size_t k : bad) {
                nc += items[mem[k].idx].claims->size();
                nw += weights_of<F>(sh, *items[mem[k].idx].claims) - R;
            }
            const size_t rc_at = align_up<F>(nc * sizeof(ObJob<Row>)), ry_at = rc_at + align_up<F>(nc * sizeof(ObClaim)), rz_at = ry_at + nc * sizeof(W),
                         rw_at = rz_at + nc * (size_t)sh.c * sizeof(W);
            std::vector<char> rs(rw_at + nw * sizeof(W) + F::ALIGN);
            ObJob<Row>* hd = reinterpret_cast<ObJob<Row>*>(rs.data());
            ObClaim* hc = reinterpret_cast<ObClaim*>(rs.data() + rc_at);
            W* hy = reinterpret_cast<W*>(rs.data() + ry_at);
            W* hz = reinterpret_cast<W*>(rs.data() + rz_at);
            W* hw = reinterpret_cast<W*>(rs.data() + rw_at);
            size_t q = 0, off = 0;
            for (size_t b = 0; b < bad.size(); b++) {
                const Commitment& cm = *items[mem[bad[b]].idx].cm;
                const std::vector<Claim>& claims = *items[mem[bad[b]].idx].claims;
                for (size_t i = 0; i < claims.size(); i++, q++) {
                    const Claim& cl = claims[i];
                    const std::vector<W> w = F::eq_table(cl.point.data() + sh.c, (size_t)(sh.nvars[cl.table] - sh.c));
                    hd[q].src = reinterpret_cast<const Row*>(cm.d_rows) + (sh.off[cl.table] << sh.c); hd[q].nrows = w.size(); hd[q].w_at = rw_at + off * sizeof(W); hd[q].u_at = q * C;
                    memcpy(hw + off, w.data(), w.size() * sizeof(W));
                    off += w.size();
                    hy[q] = cl.value;
                    F::store_low(hz + q * (size_t)sh.c, cl.point.data(), sh.c);
                    hc[q].u_at = q * C; hc[q].z_at = rz_at + q * (size_t)sh.c * sizeof(W); hc[q].y_at = ry_at + q * sizeof(W); hc[q].member = (u64)b; hc[q].claim = (u64)i;
                }
            }
            char* d_rs;
            W* d_ru;
            u64* d_cells;
            try {
                d_rs = ctx->alloc_n<char>(rs.size());
                d_ru = ctx->alloc_n<W>(nc * C);
                d_cells = ctx->alloc_n<u64>(bad.size());
            } catch (const std::exception& e) {
                throw Error(who + ": the context's arena cannot hold the claims of the refused members: lower verify_batch_group (" + e.what() + ")");
            }
            if (nc * ((C + F::TPB - 1) / F::TPB) > 0x7fffffffull) throw Error(who + ": the refused members have too many claims for one launch: lower verify_batch_group");
            std::vector<u64> cells(bad.size());
            hip_check(hipMemcpyAsync(d_rs, rs.data(), rs.size(), hipMemcpyHostToDevice, st), "upload claims");
            hip_check(hipMemsetAsync(d_cells, 0xff, bad.size() * 8, st), "memset");
            F::combine(ctx, cls, st, sh.c, nc, nw, 0, reinterpret_cast<const ObJob<Row>*>(d_rs), d_rs, d_ru);
            F::ob_eval(ctx, cls, st, reinterpret_cast<const ObClaim*>(d_rs + rc_at), nc, sh.c, d_ru, d_rs, d_cells);
            hip_check(hipMemcpyAsync(cells.data(), d_cells, bad.size() * 8, hipMemcpyDeviceToHost, st), "download evaluation checks");
            hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());   // (the staged copy and the cells are locals)
            hip_check(hipGetLastError(), (who + ": launch").c_str());
            for (size_t b = 0; b < bad.size(); b++) {
                if (cells[b] == PCSV_NONE) throw Error(who + ": index " + std::to_string(mem[bad[b]].idx) + ": internal: the reduction does not meet its claim");
                mem[bad[b]].failing = (size_t)cells[b];
            }
        }
        const size_t active = G - bad.size();
        const double t3 = omp_get_wtime();
        if (active) {
            // the tail: two row combinations a member that was not refused
            ObMember<Row>* hm = reinterpret_cast<ObMember<Row>*>(h_stage + tmem_at);
            ObJob<Row>* hd = reinterpret_cast<ObJob<Row>*>(h_stage + tjob_at);
            std::vector<size_t> live;
            for (size_t k = 0; k < G; k++)
                if (!mem[k].refused) live.push_back(k);
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
            for (long long k = 0; k < (long long)G; k++) {
                Member& x = mem[k];
                try {
                    const Commitment& cm = *items[x.idx].cm;
                    hm[k].M = reinterpret_cast<const Row*>(cm.d_M); hm[k].img = (size_t)k * (len / 8); hm[k].u = 0; hm[k].u_words = body_at;
                    h_js[G * Q + k] = x.refused ? 0 : 1;
                    if (x.refused) continue;
                    const size_t a = std::lower_bound(live.begin(), live.end(), (size_t)k) - live.begin();   // its number among the members that go on
                    const auto jobs = x.P->body_jobs(sh);
                    for (size_t i = 0; i < 2; i++) {
                        ObJob<Row>& d = hd[2 * a + i];
                        d.src = reinterpret_cast<const Row*>(cm.d_rows); d.nrows = R; d.w_at = tw_at + (2 * (size_t)k + i) * R * sizeof(W); d.u_at = (2 * (size_t)k + i) * C;
                        memcpy(h_stage + d.w_at, jobs[i].w.data(), R * sizeof(W));
                    }
                } catch (const std::exception& e) { x.error = e.what(); }
            }
            rethrow(mem);
            hip_check(hipMemcpyAsync(d_stage + tmem_at, h_stage + tmem_at, js_at - tmem_at, hipMemcpyHostToDevice, st), "upload weights");
            F::combine(ctx, cls, st, sh.c, 2 * active, 2 * active * R, 0, reinterpret_cast<const ObJob<Row>*>(d_stage + tjob_at), d_stage, d_u);
            hip_check(hipMemcpyAsync(h_out + hu_at, d_u, G * 2 * C * sizeof(W), hipMemcpyDeviceToHost, st), "download combinations");
            hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
            hip_check(hipGetLastError(), (who + ": launch").c_str());
        }
        const double t4 = omp_get_wtime();
        if (active) {
            // the host's share: every member's u vectors into its transcript (and behind its header), its column indices out of it
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
            for (long long k = 0; k < (long long)G; k++) {
                Member& x = mem[k];
                for (size_t q = 0; q < Q; q++) h_js[(size_t)k * Q + q] = 0;
                if (x.refused) continue;
                try {
                    x.P->write_u(h_u + 2 * C * (size_t)k, 2 * C);
                    const std::vector<size_t> js = F::squeeze_indices(x.P->tr, N, Q);
                    for (size_t q = 0; q < Q; q++) h_js[(size_t)k * Q + q] = js[q];
                } catch (const std::exception& e) { x.error = e.what(); }
            }
            rethrow(mem);
        }
        const double t5 = omp_get_wtime();
        if (active) {
            hip_check(hipMemcpyAsync(d_stage + js_at, h_js, (G * Q + G) * 8, hipMemcpyHostToDevice, st), "upload column indices");
            F::gather(ctx, cls, st, reinterpret_cast<const ObMember<Row>*>(d_stage + tmem_at), G, Q, R, N, q_words, active, reinterpret_cast<const u64*>(d_stage + js_at), d_img);
            hip_check(hipMemcpyAsync(h_out + himg_at, d_img, G * len, hipMemcpyDeviceToHost, st), "download openings");
            hip_check(hipStreamSynchronize(st), (who + ": sync").c_str());
            hip_check(hipGetLastError(), (who + ": launch").c_str());
        }
        ctx->prof_collect();
        const double t6 = omp_get_wtime();
        // header and u vectors from each transcript, the siblings from each handle's tree into the gaps; a refused member's reason
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::min<int>(nthr, (int)G))
        for (long long k = 0; k < (long long)G; k++) {
            Member& x = mem[k];
            try {
                Opened& out = res[x.idx];
                const Commitment& cm = *items[x.idx].cm;
                if (x.refused) {
                    out.refused = true;
                    out.reason = std::string(single) + ": claim " + std::to_string(x.failing) + ": the value is not the evaluation of table " +
                                 std::to_string((*items[x.idx].claims)[x.failing].table) + " at the point";
                    continue;
                }
                const std::vector<uint8_t>& head = x.P->tr.bytes;
                if (head.size() != 8 * body_at) throw Error("internal: opening length");
                const uint8_t* image = h_img + (size_t)k * len;
                out.bytes.assign(image, image + len);
                memcpy(out.bytes.data(), head.data(), head.size());
                for (size_t q = 0; q < Q; q++) {
                    uint8_t* sib = out.bytes.data() + 8 * (body_at + q * q_words + RW * R);
                    size_t idx = (size_t)h_js[(size_t)k * Q + q];
                    for (int l = 0; l < depth; l++, idx >>= 1) memcpy(sib + 32 * l, cm.node(l, idx ^ 1), 32);
                }
            } catch (const std::exception& e) { x.error = e.what(); }
        }
        rethrow(mem);
        if (times)
            fprintf(stderr, "[hg pcs] %sfolded open group %zu of %zu members: transcripts and factor tables %.2f ms, g and %zu rounds %.2f (host arithmetic %.2f), refusals %.2f, "
                            "combine and u back %.2f, hash %.2f, gather and images back %.2f, header and siblings %.2f\n", F::TIMES_TAG, g, G, (t1 - t0) * 1e3, V, (t2 - t1) * 1e3,
                    t_host * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3, (t6 - t5) * 1e3, (omp_get_wtime() - t6) * 1e3);
    }
    return res;
}

}  // namespace pcs
}  // namespace hg
