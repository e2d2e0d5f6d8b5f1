// Integer arithmetic of the witness derivation (hg_witness_derive: kernels.hip k_derive_*, host glue in prover.hip), shared by the
// gfx950 kernels and the host so that the same lines can be checked on a CPU build: signed 128-bit values in two limbs, the
// remainder of such a value by a CRT modulus through a precomputed reciprocal (no 128-bit division on the device), the exact
// quotient by an odd modulus through its inverse mod 2^64.
// The rule itself [REF scripts/circuit_sk.py:18-140] is restated in host.cpp above witness_synthetic.
#pragma once
#include "gl_field.hpp"

namespace hg {
namespace drv {

HG_HD u64 mulhi64(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}

struct S128 { u64 lo; int64_t hi; };   // two's complement, hi holds the sign

HG_HD S128 s128(int64_t x) { return S128{(u64)x, x >> 63}; }
HG_HD S128 s128_add(S128 a, S128 b) {
    u64 lo = a.lo + b.lo;
    return S128{lo, (int64_t)((u64)a.hi + (u64)b.hi + (lo < a.lo ? 1 : 0))};
}
HG_HD S128 s128_neg(S128 a) {
    u64 lo = ~a.lo + 1;
    return S128{lo, (int64_t)(~(u64)a.hi + (lo == 0 ? 1 : 0))};
}
HG_HD S128 s128_sub(S128 a, S128 b) { return s128_add(a, s128_neg(b)); }
HG_HD S128 s128_shl32(int64_t x) { return S128{(u64)x << 32, x >> 32}; }   // x * 2^32 (an arithmetic shift keeps the sign)
HG_HD S128 s128_mul(int64_t x, u64 m) {                                     // x * m, |x| m < 2^127
    const u64 a = x < 0 ? (u64)0 - (u64)x : (u64)x;
    S128 r{a * m, (int64_t)mulhi64(a, m)};
    return x < 0 ? s128_neg(r) : r;
}
HG_HD bool s128_eq(S128 a, S128 b) { return a.lo == b.lo && a.hi == b.hi; }

// A signed coefficient as the tables hold it: z >= 0 as z, z < 0 as p - |z| (utils.py:4-18). |z| < 2^63.
HG_HD int64_t gl_signed(u64 w) { return w > (GL_P >> 1) ? -(int64_t)(GL_P - w) : (int64_t)w; }
HG_HD u64 gl_assign(int64_t z) { return z >= 0 ? (u64)z : GL_P - ((u64)0 - (u64)z); }

// One CRT modulus as the kernels read it. d = q << sh has its top bit set; v = floor((2^128 - 1) / d) - 2^64 is the reciprocal of
// Moeller and Granlund, "Improved division by invariant integers" (IEEE Trans. Computers 60(2), 2011), algorithm 4.
struct Modulus { u64 q, d, v, qinv, half; int sh; };   // qinv = q^-1 mod 2^64 (q odd); half = (q - 1) / 2

// z mod q for z >= 0 with (z << sh) >> 64 < d (derive_plan in prover.hip checks that bound for every value the combine
// step forms, and refuses a q of 62 bits or more, so 2 <= sh <= 63 and no shift below is by 64)
HG_HD u64 mod_u128(u64 hi, u64 lo, const Modulus& m) {
    const u64 u1 = (hi << m.sh) | (lo >> (64 - m.sh)), u0 = lo << m.sh;
    u64 q0 = m.v * u1, q1 = mulhi64(m.v, u1);
    q0 += u0;
    q1 += u1 + (q0 < u0 ? 1 : 0) + 1;
    u64 r = u0 - q1 * m.d;
    if (r > q0) r += m.d;
    if (r >= m.d) r -= m.d;
    return r >> m.sh;
}
// cmod(z, q): the residue of z in [-(q-1)/2, (q-1)/2]
HG_HD int64_t centre_mod(S128 z, const Modulus& m) {
    const bool neg = z.hi < 0;
    if (neg) z = s128_neg(z);
    u64 r = mod_u128((u64)z.hi, z.lo, m);
    if (neg && r) r = m.q - r;
    return r > m.half ? (int64_t)r - (int64_t)m.q : (int64_t)r;
}
// z / q for a z that q divides and a quotient below 2^63 in magnitude: the low word times q^-1 mod 2^64; *exact = the product gives z back
HG_HD int64_t exact_quotient(S128 z, const Modulus& m, bool* exact) {
    const int64_t t = (int64_t)(z.lo * m.qinv);
    *exact = s128_eq(s128_mul(t, m.q), z);
    return t;
}

}  // namespace drv
}  // namespace hg
