// java.util.Random (JDK specification): the 48-bit LCG the reference draws every phantom, bead and ray from.  One statement of the
// recipe for the host walks (phantom.hip, mvsim_beads_random_points) and the device tracers (aberrations.hip); plain C++, so the
// known answers of tests/golden/jdk_vectors.json check it without a GPU.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define MVSIM_JR_FN __host__ __device__ __forceinline__
#else
#define MVSIM_JR_FN inline
#endif

namespace mvsim {

constexpr uint64_t JR_MASK = (1ULL << 48) - 1, JR_A = 0x5DEECE66DULL, JR_C = 0xBULL;

struct JRandom {
    uint64_t s;                       // the scrambled seed as the JDK keeps it (48 bits)
    MVSIM_JR_FN int32_t next(int bits)
    {
        s = (s * JR_A + JR_C) & JR_MASK;
        return (int32_t)((int64_t)s >> (48 - bits));
    }
    MVSIM_JR_FN int32_t next_int(int32_t bound)
    {
        int32_t r = next(31);
        const int32_t m = bound - 1;
        if ((bound & m) == 0) return (int32_t)(((int64_t)bound * (int64_t)r) >> 31);
        for (int32_t u = r; (int32_t)((uint32_t)u - (uint32_t)(r = u % bound) + (uint32_t)m) < 0; u = next(31)) {}
        return r;
    }
    MVSIM_JR_FN double next_double()
    {
        const int64_t hi = (int64_t)next(26) << 27;
        return (double)(hi + next(27)) * 0x1.0p-53;
    }
};

// the state after k steps from s: s * a^k + c (a^(k-1) + ... + 1)  (mod 2^48), composing the affine map with itself by squaring
MVSIM_JR_FN uint64_t jr_jump(uint64_t s, uint64_t k)
{
    uint64_t A = 1, C = 0, a = JR_A, c = JR_C;
    while (k) {
        if (k & 1) { A = (A * a) & JR_MASK; C = (C * a + c) & JR_MASK; }
        c = ((a + 1) * c) & JR_MASK;
        a = (a * a) & JR_MASK;
        k >>= 1;
    }
    return (s * A + C) & JR_MASK;
}

// ---- nextGaussian() and Collections.shuffle: host only ------------------------------------------------------------------------
// StrictMath.log is fdlibm's __ieee754_log (e_log.c, Sun's freely redistributable algorithm), restated: a platform log differs from it
// in the last bit for about three arguments in a hundred, and nextGaussian() is specified through StrictMath.
inline double jr_from_bits(uint64_t b) { double d; std::memcpy(&d, &b, sizeof d); return d; }
inline uint64_t jr_to_bits(double d) { uint64_t b; std::memcpy(&b, &d, sizeof b); return b; }

inline double jr_strict_log(double x)
{
    const double ln2_hi = jr_from_bits(0x3fe62e42fee00000ULL), ln2_lo = jr_from_bits(0x3dea39ef35793c76ULL),
                 two54 = jr_from_bits(0x4350000000000000ULL), Lg1 = jr_from_bits(0x3FE5555555555593ULL),
                 Lg2 = jr_from_bits(0x3FD999999997FA04ULL), Lg3 = jr_from_bits(0x3FD2492494229359ULL),
                 Lg4 = jr_from_bits(0x3FCC71C51D8E78AFULL), Lg5 = jr_from_bits(0x3FC7466496CB03DEULL),
                 Lg6 = jr_from_bits(0x3FC39A09D078C69FULL), Lg7 = jr_from_bits(0x3FC2F112DF3E5244ULL);
    uint64_t bits = jr_to_bits(x);
    int32_t hx = (int32_t)(bits >> 32);
    const uint32_t lx = (uint32_t)bits;
    int32_t k = 0;
    if (hx < 0x00100000) {                                   // x < 2^-1022
        if (((hx & 0x7fffffff) | lx) == 0) return -HUGE_VAL; // log(+-0) = -inf
        if (hx < 0) return std::nan("");                     // log(-#) = NaN
        k -= 54;
        x *= two54;                                          // subnormal: scale up
        bits = jr_to_bits(x);
        hx = (int32_t)(bits >> 32);
    }
    if (hx >= 0x7ff00000) return x + x;
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    int32_t i = (hx + 0x95f64) & 0x100000;
    x = jr_from_bits(((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (bits & 0xffffffffULL));   // normalise x or x / 2
    k += i >> 20;
    const double f = x - 1.0;
    if ((0x000fffff & (2 + hx)) < 3) {                       // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            const double dk = (double)k;
            return dk * ln2_hi + dk * ln2_lo;
        }
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        if (k == 0) return f - R;
        const double dk = (double)k;
        return dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f), dk = (double)k, z = s * s, w = z * z;
    i = hx - 0x6147a;
    const int32_t j = 0x6b851 - hx;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6)), t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    i |= j;
    const double R = t2 + t1;
    if (i > 0) {
        const double hfsq = 0.5 * f * f;
        if (k == 0) return f - (hfsq - s * (hfsq + R));
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    if (k == 0) return f - s * (f - R);
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// Random.nextGaussian(): the polar method of the JDK specification.  `pending` is the cached second value (NaN: none).
inline double jr_next_gaussian(JRandom& rnd, double& pending)
{
    if (pending == pending) {
        const double g = pending;
        pending = std::nan("");
        return g;
    }
    double v1, v2, s;
    do {
        v1 = 2 * rnd.next_double() - 1;
        v2 = 2 * rnd.next_double() - 1;
        s = v1 * v1 + v2 * v2;
    } while (s >= 1 || s == 0);
    const double multiplier = std::sqrt(-2 * jr_strict_log(s) / s);
    pending = v2 * multiplier;
    return v1 * multiplier;
}

// Collections.shuffle(list, rnd): for i = size; i > 1; i--: swap(i - 1, rnd.nextInt(i))
inline void jr_shuffle(JRandom& rnd, int32_t* list, int32_t size)
{
    for (int32_t i = size; i > 1; --i) {
        const int32_t j = rnd.next_int(i), t = list[i - 1];
        list[i - 1] = list[j];
        list[j] = t;
    }
}

}  // namespace mvsim
