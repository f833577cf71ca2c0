// The rollout's RANDOM NUMBERS: a counter-based generator and a triple of standard normals that the host repeats bit for bit
// (action_motion.py: philox4x32_10, normal3).  No state: every draw is a pure function of a 64-bit key and a 128-bit counter, so a
// robot's draws depend on nothing but what names them -- not on the lane it runs in, the robots run beside it or the order of ticks.
//
//   philox4x32_10   Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the
//                   Random123 constants; integer arithmetic only.
//   normal3         Box-Muller on one block w0..w3:  u = (2 w0 + 1) / 2^33 in (0, 1),  r = sqrt(-2 ln u),  phi = 2 pi w1 / 2^32,
//                   z0 = r cos phi, z1 = r sin phi;  the second pair of words gives z2 = r' cos phi'.  |z| <= sqrt(66 ln 2) = 6.76.
//   normal4         all four values of a block, z3 = r' sin phi', with the fourth counter word as a stream (action_motion.py: normal4)
// The device's log and sincos are not correctly rounded and differ from the host's, so both are written out here in add, multiply,
// divide and square root, every one rounded on its own (__dmul_rn and its relatives: no contraction into an fma) and in the order
// written:
//   ln_rn           x = m 2^e by bit operations, m in [sqrt(1/2), sqrt(2)) so that ln m has no cancellation against e ln 2 near x = 1;
//                   ln m = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716: the series to s^25 / 25 (truncation < 2e-20 relative)
//   sincos_turn_rn  of 2 pi w / 2^32: the quadrant from the top two bits, the rest r folded onto [0, 2^29] (r -> 2^30 - r swaps sine
//                   and cosine) in integers, so the polynomial's argument a = r' (2 pi / 2^32) <= pi / 4 carries one rounding; Taylor
//                   to a^19 / 19! and a^20 / 20! (truncation < 1e-19 / 4e-21 relative).  Exact zeros where the angle's sine or cosine
//                   is zero, and a relative error of a few ulp right beside them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace irlosc {

__device__ __forceinline__ void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ln x for a positive, finite, normal x
__device__ __forceinline__ double ln_rn(double x) {
    constexpr double SQRT2 = 1.4142135623730951, LN2 = 0.6931471805599453;
    const uint64_t bits = (uint64_t)__double_as_longlong(x);
    int e = (int)((bits >> 52) & 0x7ffu) - 1023;
    double m = __longlong_as_double((long long)((bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull));      // [1, 2)
    if (m >= SQRT2) { m = __dmul_rn(m, 0.5); e += 1; }
    const double s = __ddiv_rn(__dsub_rn(m, 1.0), __dadd_rn(m, 1.0));
    const double s2 = __dmul_rn(s, s);
    double p = 1.0 / 25.0;
#pragma unroll
    for (int k = 23; k >= 1; k -= 2) p = __dadd_rn(__dmul_rn(p, s2), 1.0 / (double)k);
    return __dadd_rn(__dmul_rn((double)e, LN2), __dmul_rn(__dmul_rn(2.0, s), p));
}

// a * (1 - a^2/3! + ... - a^18/19!) and 1 - a^2/2! + ... + a^20/20! for a in [0, pi/4]
__device__ __forceinline__ void sincos_poly_rn(double a, double* sn, double* cs) {
    constexpr double F[21] = {1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0, 39916800.0, 479001600.0,
                              6227020800.0, 87178291200.0, 1307674368000.0, 20922789888000.0, 355687428096000.0, 6402373705728000.0,
                              121645100408832000.0, 2432902008176640000.0};      // n!, each exact in a double
    const double a2 = __dmul_rn(a, a);
    double ps = -1.0 / F[19], pc = 1.0 / F[20];
#pragma unroll
    for (int k = 17; k >= 1; k -= 2) ps = __dadd_rn(__dmul_rn(ps, a2), ((k & 2) ? -1.0 : 1.0) / F[k]);
#pragma unroll
    for (int k = 18; k >= 0; k -= 2) pc = __dadd_rn(__dmul_rn(pc, a2), ((k & 2) ? -1.0 : 1.0) / F[k]);
    *sn = __dmul_rn(a, ps);
    *cs = pc;
}

// sine and cosine of 2 pi w / 2^32
__device__ __forceinline__ void sincos_turn_rn(uint32_t w, double* sn, double* cs) {
    constexpr double K = 6.283185307179586 / 4294967296.0;      // 2 pi / 2^32 (a power of two: exact scaling of the rounded 2 pi)
    const uint32_t quad = w >> 30, r = w & 0x3fffffffu;
    const bool fold = r > 0x20000000u;
    double s, c;
    sincos_poly_rn(__dmul_rn((double)(fold ? 0x40000000u - r : r), K), &s, &c);
    if (fold) { const double t = s; s = c; c = t; }
    *sn = quad == 0 ? s : quad == 1 ? c : quad == 2 ? -s : -c;
    *cs = quad == 0 ? c : quad == 1 ? -s : quad == 2 ? -c : s;
}

// Three standard normals of block (robot, draw, action, 0) under key `seed`
__device__ __forceinline__ void normal3(uint64_t seed, uint32_t robot, uint32_t draw, uint32_t action, double z[3]) {
    const uint32_t ctr[4] = {robot, draw, action, 0u}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    constexpr double INV33 = 1.0 / 8589934592.0;                // 2^-33
    double s, c;
    const double u0 = __dmul_rn(__dadd_rn(__dmul_rn(2.0, (double)w[0]), 1.0), INV33);      // (every step exact: 33 bits)
    const double r0 = __dsqrt_rn(__dmul_rn(-2.0, ln_rn(u0)));
    sincos_turn_rn(w[1], &s, &c);
    z[0] = __dmul_rn(r0, c);
    z[1] = __dmul_rn(r0, s);
    const double u1 = __dmul_rn(__dadd_rn(__dmul_rn(2.0, (double)w[2]), 1.0), INV33);
    const double r1 = __dsqrt_rn(__dmul_rn(-2.0, ln_rn(u1)));
    sincos_turn_rn(w[3], &s, &c);
    z[2] = __dmul_rn(r1, c);
}

// One Box-Muller pair on the words (wa, wb) of a block: *zc = r cos phi, *zs = r sin phi -- normal3's steps, both values kept
__device__ __forceinline__ void normal_pair(uint32_t wa, uint32_t wb, double* zc, double* zs) {
    constexpr double INV33 = 1.0 / 8589934592.0;                // 2^-33
    double s, c;
    const double u = __dmul_rn(__dadd_rn(__dmul_rn(2.0, (double)wa), 1.0), INV33);
    const double r = __dsqrt_rn(__dmul_rn(-2.0, ln_rn(u)));
    sincos_turn_rn(wb, &s, &c);
    *zc = __dmul_rn(r, c);
    *zs = __dmul_rn(r, s);
}

// Four standard normals of block (robot, draw, block, stream) under key `seed`: both word pairs of the block, z0 = r0 cos, z1 = r0 sin,
// z2 = r1 cos, z3 = r1 sin.  The fourth counter word names a STREAM: normal3 is stream 0 (its three values are z0, z1, z2 of this block),
// the policy's Gaussian head draws on stream 1 (osc_policy.hpp), so the two never meet under one seed.
__device__ __forceinline__ void normal4(uint64_t seed, uint32_t robot, uint32_t draw, uint32_t block, uint32_t stream, double z[4]) {
    const uint32_t ctr[4] = {robot, draw, block, stream}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    normal_pair(w[0], w[1], &z[0], &z[1]);
    normal_pair(w[2], w[3], &z[2], &z[3]);
}

}  // namespace irlosc
