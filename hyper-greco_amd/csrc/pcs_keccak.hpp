// Keccak-f[1600] on the device with the whole state in registers, the inner node of the commitment's Merkle tree and the climb of an
// opened column's path: shared by the column-hash, tree and query kernels of both fields (pcs.hip: Goldilocks words, bn254_pcs.inc: 32-byte Fr elements; a node is 32 bytes
// either way).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace hg {
namespace pcs {

typedef uint64_t u64;

// ---- Keccak-f[1600], the whole state in registers: 24 rounds unrolled, every lane index a compile-time constant (a run-time index
// would put the state into scratch memory)
__device__ constexpr u64 KRC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
__device__ constexpr int KROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // rho offsets, lane x + 5y
__device__ __forceinline__ u64 krotl(u64 v, int s) { return s ? (v << s) | (v >> (64 - s)) : v; }
__device__ __forceinline__ void keccak_f(u64 (&a)[25]) {
#pragma unroll
    for (int rd = 0; rd < 24; rd++) {
        u64 c[5], d[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ krotl(c[(x + 1) % 5], 1);
#pragma unroll
        for (int i = 0; i < 25; i++) a[i] ^= d[i % 5];
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = krotl(a[x + 5 * y], KROT[x + 5 * y]);
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= KRC[rd];
    }
}
constexpr int RATE_WORDS = 17;   // Keccak-256: 136 bytes

__device__ __forceinline__ void merkle_node(const u64* below, u64* here, size_t i) {
    u64 a[25];
    const u64* in = below + 8 * i;   // left || right
    a[0] = 1;
#pragma unroll
    for (int k = 0; k < 8; k++) a[1 + k] = in[k];
    a[9] = 0x01;
#pragma unroll
    for (int k = 10; k < 25; k++) a[k] = 0;
    a[RATE_WORDS - 1] = 0x8000000000000000ull;
    keccak_f(a);
    u64* out = here + 4 * i;
    out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
}
// The path of column j from its leaf hash h up to the root, which replaces h: level l's sibling is the 4 words at sib + 4l, and
// bit l of j says on which side it lies
__device__ __forceinline__ void merkle_climb(u64 (&h)[4], const u64* __restrict__ sib, size_t j, int depth) {
    for (int l = 0; l < depth; l++) {
        const bool right = (j >> l) & 1;   // this node is the right child
        const u64 t0 = sib[4 * l], t1 = sib[4 * l + 1], t2 = sib[4 * l + 2], t3 = sib[4 * l + 3];
        u64 a[25];
        a[0] = 1;
        a[1] = right ? t0 : h[0]; a[2] = right ? t1 : h[1]; a[3] = right ? t2 : h[2]; a[4] = right ? t3 : h[3];
        a[5] = right ? h[0] : t0; a[6] = right ? h[1] : t1; a[7] = right ? h[2] : t2; a[8] = right ? h[3] : t3;
        a[9] = 0x01;
#pragma unroll
        for (int k = 10; k < 25; k++) a[k] = 0;
        a[RATE_WORDS - 1] = 0x8000000000000000ull;
        keccak_f(a);
        h[0] = a[0]; h[1] = a[1]; h[2] = a[2]; h[3] = a[3];
    }
}

}  // namespace pcs
}  // namespace hg
