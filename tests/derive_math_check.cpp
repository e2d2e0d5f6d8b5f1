// Host check of csrc/derive_math.hpp (compiled and run by tests/test_witness_derive.py): the two-limb signed arithmetic, the remainder
// through the precomputed reciprocal, the centred residue and the exact quotient against __int128 arithmetic.
#include <cstdio>
#include <cstdlib>
#include "derive_math.hpp"

using namespace hg;
using namespace hg::drv;
typedef __int128 i128;
typedef unsigned __int128 u128;

static u64 rng_state = 0x9E3779B97F4A7C15ULL;
static u64 rnd() {
    u64 z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static Modulus modulus(u64 q) {
    Modulus m;
    m.q = q; m.sh = __builtin_clzll(q); m.d = q << m.sh;
    m.v = (u64)(~(u128)0 / m.d - ((u128)1 << 64));
    m.qinv = q;
    for (int it = 0; it < 5; it++) m.qinv *= 2 - q * m.qinv;
    m.half = (q - 1) / 2;
    return m;
}
static S128 from(i128 z) { return S128{(u64)z, (int64_t)(z >> 64)}; }
static i128 to(S128 z) { return ((i128)z.hi << 64) | (i128)(u128)z.lo; }
static i128 cmod_ref(i128 z, i128 q) {
    i128 r = z % q;
    if (r < 0) r += q;
    if (r > (q - 1) / 2) r -= q;
    return r;
}
static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 10) printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void check_value(i128 z, const Modulus& m) {
    const i128 q = (i128)m.q;
    CHECK((i128)centre_mod(from(z), m) == cmod_ref(z, q));
    if (z >= 0) CHECK(mod_u128((u64)(z >> 64), (u64)z, m) == (u64)(z % q));
    CHECK(to(s128_neg(from(z))) == -z);
}

int main() {
    const u64 fixed[] = {3, 5, 82638181ULL, (1ULL << 27) - 39, (1ULL << 52) - 47, (1ULL << 55) - 55, (1ULL << 59) - 55, (1ULL << 61) - 1, (1ULL << 62) - 57};
    for (int t = 0; t < 200; t++) {
        u64 q = t < 9 ? fixed[t] : ((rnd() >> (2 + rnd() % 60)) | 1);
        if (q < 3) q = 3;
        const Modulus m = modulus(q);
        CHECK(m.sh >= 2 && m.q * m.qinv == 1);
        // the largest z the precondition (z << sh) >> 64 < d admits
        const u128 zmax = (((u128)m.d << 64) >> m.sh) - 1;
        const i128 half = (i128)m.half;
        const i128 edges[] = {0, 1, -1, half, half + 1, -half, -half - 1, (i128)q, -(i128)q, (i128)q * 7 + half, (i128)q * 7 + half + 1,
                              -((i128)q * 7 + half), -((i128)q * 7 + half + 1), (i128)(zmax >> 1), -(i128)(zmax >> 1), (i128)((zmax >> 1) - q)};
        for (i128 z : edges) check_value(z, m);
        for (int r = 0; r < 2000; r++) {
            u128 z = (((u128)rnd() << 64) | rnd()) % ((zmax >> 1) + 1);
            z >>= rnd() % 100;
            check_value((r & 1) ? -(i128)z : (i128)z, m);
            // exact quotient: t * q for |t| < 2^62, and a neighbour that q does not divide
            const int64_t tq = (int64_t)(rnd() >> (2 + rnd() % 60)) * ((r & 2) ? -1 : 1);
            bool ex = false;
            CHECK(exact_quotient(from((i128)tq * q), m, &ex) == tq && ex);
            exact_quotient(from((i128)tq * q + 1), m, &ex);
            CHECK(!ex);
            // two-limb helpers
            const int64_t x = (int64_t)rnd() >> (rnd() % 40), y = (int64_t)rnd() >> (rnd() % 40);
            CHECK(to(s128_add(s128(x), s128(y))) == (i128)x + y);
            CHECK(to(s128_sub(s128_shl32(x >> 20), s128(y))) == (i128)(x >> 20) * ((i128)1 << 32) - y);
            CHECK(to(s128_mul(x >> 2, q)) == (i128)(x >> 2) * q);
        }
    }
    for (int r = 0; r < 1000; r++) {
        const int64_t z = (int64_t)(rnd() >> 2) * ((r & 1) ? -1 : 1);
        CHECK(gl_signed(gl_assign(z)) == z && gl_assign(z) < GL_P);
    }
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
