// The arithmetic of one voxel of the extractSlices / poissonProcess stage, stated once: for the device (every sampler kernel, through
// poisson_dev.h) and for a host compiler (tests/c_abi/poisson_recipe_main.cpp holds it to the oracle on a CPU).  Replaces
// uncommons/PoissonGenerator.java:95-109 + java.util.Random, which cost ~lambda+1 Math.log calls per voxel on one strictly
// sequential stream.
//
// Generator : Philox4x32-10, key = 64-bit seed
// Sampler   : lambda < 10  -> inversion by sequential search on a 32-bit uniform; the 4 voxels of
//                             group index>>2 share ONE Philox block, ctr = (index>>2, stream, 0)         (group_block / group_word)
//             lambda >= 10 -> Hoermann's PTRS transformed rejection on 32-bit uniforms; attempt 0 of the
//                             voxel pair index>>1 shares one block, ctr = (index>>1, stream, 1)          (pair_block / pair_words);
//                             retries take two attempts per block, ctr = (index, stream, 2 + (a-1)/2)   (ptrs_retry_words)
// All accept/reject arithmetic is IEEE +,-,*,/,sqrt,fma on doubles plus the bit-defined log/exp
// below (built with -ffp-contract=off), so a CPU implementation of the same recipe gives
// identical counts.  The one place single precision decides anything is ptrs_screen, and it answers only where the fp64 test
// is certain to agree.
//
// No HIP include on the host: MVSIM_RECIPE_FN is the functions' qualifier, MVSIM_RECIPE_TABLE the tables' storage, the bit casts go
// through the HIP intrinsics or __builtin_memcpy, __logf is logf there, and the unroll pragmas (MVSIM_RECIPE_UNROLL) are empty.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MVSIM_RECIPE_FN __device__ __forceinline__
#define MVSIM_RECIPE_TABLE __device__ const
#define MVSIM_RECIPE_LOGF(x) __logf(x)
#define MVSIM_RECIPE_UNROLL _Pragma("unroll")
#define MVSIM_RECIPE_NO_UNROLL _Pragma("unroll 1")
#else
#include <cmath>
#define MVSIM_RECIPE_FN static inline
#define MVSIM_RECIPE_TABLE static const
#define MVSIM_RECIPE_LOGF(x) logf(x)
#define MVSIM_RECIPE_UNROLL
#define MVSIM_RECIPE_NO_UNROLL
#endif

namespace mvsim {

MVSIM_RECIPE_FN uint64_t recipe_bits(double d)
{
#if defined(__HIPCC__)
    return (uint64_t)__double_as_longlong(d);
#else
    uint64_t u;
    __builtin_memcpy(&u, &d, 8);
    return u;
#endif
}

MVSIM_RECIPE_FN double recipe_double(uint64_t u)
{
#if defined(__HIPCC__)
    return __longlong_as_double((long long)u);
#else
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
#endif
}

struct Philox4 {
    uint32_t x, y, z, w;
};

MVSIM_RECIPE_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
MVSIM_RECIPE_UNROLL
    for (int r = 0; r < 10; ++r) {
        // one 32x32 -> 64 multiply per product (v_mad_u64_u32) instead of separate mul_hi / mul_lo
        const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0;
        const uint32_t n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

// ---- which word of which block belongs to voxel `index`: these helpers are the only places that know the counters
// Inversion regime: the block of group index >> 2, and the voxel's word of it (word index & 3).
MVSIM_RECIPE_FN Philox4 group_block(uint64_t index, uint32_t stream, uint32_t k0, uint32_t k1)
{
    const uint64_t g = index >> 2;
    return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), stream, 0u, k0, k1);
}

MVSIM_RECIPE_FN uint32_t group_word(Philox4 r, uint64_t index)
{
    const uint32_t c = (uint32_t)index & 3u;
    return c == 0u ? r.x : (c == 1u ? r.y : (c == 2u ? r.z : r.w));
}

// PTRS attempt 0: the block of pair index >> 1, and the voxel's two words of it (words 2 * (index & 1), + 1).
MVSIM_RECIPE_FN Philox4 pair_block(uint64_t index, uint32_t stream, uint32_t k0, uint32_t k1)
{
    const uint64_t pr = index >> 1;
    return philox4x32_10((uint32_t)pr, (uint32_t)(pr >> 32), stream, 1u, k0, k1);
}

MVSIM_RECIPE_FN void pair_words(Philox4 r, uint64_t index, uint32_t& w0, uint32_t& w1)
{
    const bool odd = (index & 1u) != 0u;
    w0 = odd ? r.z : r.x;
    w1 = odd ? r.w : r.y;
}

// Random words of retry attempt a >= 1 of voxel `index`.
MVSIM_RECIPE_FN void ptrs_retry_words(uint64_t index, uint32_t attempt, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t& w0,
                                      uint32_t& w1)
{
    const Philox4 r = philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), stream, 2u + (attempt - 1u) / 2u, k0, k1);
    const bool second = ((attempt - 1u) & 1u) != 0u;
    w0 = second ? r.z : r.x;
    w1 = second ? r.w : r.y;
}

MVSIM_RECIPE_FN double u32_open(uint32_t w) { return ((double)w + 0.5) * 0x1.0p-32; }

// log(x), x > 0: fdlibm-style reduction to [sqrt(1/2), sqrt(2)), degree-14 odd polynomial.
MVSIM_RECIPE_FN double det_log(double x)
{
    if (!(x > 0.0)) return -1.0e300;
    uint64_t u = recipe_bits(x);
    int e = (int)(u >> 52) - 1023;
    if (e == -1023) {
        x = x * 0x1.0p54;
        u = recipe_bits(x);
        e = (int)(u >> 52) - 1023 - 54;
    }
    u = (u & 0x000FFFFFFFFFFFFFULL) | 0x3FF0000000000000ULL;
    double m = recipe_double(u);
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    const double dk = (double)e;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

// exp(-lambda), 0 < lambda < 10, division free: 2^k * sum_{n<=13} r^n / n!  (Horner, explicit FMAs)
MVSIM_RECIPE_FN double det_exp_neg(double lambda)
{
    const double x = -lambda;
    const double kf = floor(x * 1.44269504088896338700e+00 + 0.5);
    const double r = (x - kf * 6.93147180369123816490e-01) - kf * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return p * recipe_double((uint64_t)((int)kf + 1023) << 52);
}

// log(k!) : table to 16, Stirling series beyond.
MVSIM_RECIPE_TABLE double kLogFact[17] = {
    0.0, 0.0, 0.6931471805599453, 1.791759469228055, 3.1780538303479458, 4.787491742782046, 6.579251212010101,
    8.525161361065415, 10.60460290274525, 12.801827480081469, 15.104412573075516, 17.502307845873887,
    19.987214495661885, 22.552163853123425, 25.19122118273868, 27.89927138384089, 30.671860106080672};

// (`lf`: where the table is read from -- the resolver keeps a copy in LDS: a dependent GLOBAL load inside its divergent attempt costs every
// lane of the wave a trip to the cache)
MVSIM_RECIPE_FN double det_lgamma_int(long long k, const double* lf = kLogFact)
{
    if (k <= 16) return lf[k < 0 ? 0 : k];
    const double x = (double)k + 1.0;
    const double ix = 1.0 / x;
    const double ix2 = ix * ix;
    const double ser = ix * (8.3333333333333333e-02 + ix2 * (-2.7777777777777778e-03 + ix2 * (7.9365079365079365e-04 + ix2 * -5.9523809523809524e-04)));
    return ((x - 0.5) * det_log(x) - x) + 0.9189385332046727 + ser;
}

// 1/k, k = 0..63 (k = 0 unused), correctly rounded at compile time
MVSIM_RECIPE_TABLE double kInvK[64] = {
    0.0,       1.0 / 1,  1.0 / 2,  1.0 / 3,  1.0 / 4,  1.0 / 5,  1.0 / 6,  1.0 / 7,  1.0 / 8,  1.0 / 9,  1.0 / 10,
    1.0 / 11,  1.0 / 12, 1.0 / 13, 1.0 / 14, 1.0 / 15, 1.0 / 16, 1.0 / 17, 1.0 / 18, 1.0 / 19, 1.0 / 20, 1.0 / 21,
    1.0 / 22,  1.0 / 23, 1.0 / 24, 1.0 / 25, 1.0 / 26, 1.0 / 27, 1.0 / 28, 1.0 / 29, 1.0 / 30, 1.0 / 31, 1.0 / 32,
    1.0 / 33,  1.0 / 34, 1.0 / 35, 1.0 / 36, 1.0 / 37, 1.0 / 38, 1.0 / 39, 1.0 / 40, 1.0 / 41, 1.0 / 42, 1.0 / 43,
    1.0 / 44,  1.0 / 45, 1.0 / 46, 1.0 / 47, 1.0 / 48, 1.0 / 49, 1.0 / 50, 1.0 / 51, 1.0 / 52, 1.0 / 53, 1.0 / 54,
    1.0 / 55,  1.0 / 56, 1.0 / 57, 1.0 / 58, 1.0 / 59, 1.0 / 60, 1.0 / 61, 1.0 / 62, 1.0 / 63};

// Inversion by sequential search for 0 < lambda < 10 on the 32-bit word `w` of the group block.
MVSIM_RECIPE_FN float poisson_small(double lambda, uint32_t w, const double* invk = kInvK)
{
    const double u = ((double)w + 0.5) * 0x1.0p-32;
    double p = det_exp_neg(lambda);
    double F = p;
    int k = 0;
    while (u >= F && k < 63) {
        k += 1;
        p = (p * lambda) * invk[k];
        F = F + p;
    }
    return (float)k;
}

// An integer-valued double (a floor: the count PTRS proposes) as float: THE conversion of a count.  The oracle's (float)(int64_t)d rounds
// that integer to the nearest float, and so does (float)d -- the same value for every |d| < 2^63, and the oracle returns int64_t, so
// nothing beyond that is defined -- in ONE conversion; f64 -> i64 -> f32 has no instruction of its own and costs ~16 per value (two per
// pair in every PTRS trip of phase 1: 4 % of its vector instructions).
MVSIM_RECIPE_FN float count_as_float(double d) { return (float)d; }

constexpr uint32_t kPtrsMaxAttempts = 60000u;   // cap (never reached in practice: p ~ 0.1^k); then floor(lambda)

// ---- Hoermann PTRS for lambda >= 10 on 32-bit uniforms, split into pieces so that every driver executes exactly the same arithmetic.
struct PtrsSetup {
    double b, a, bm2, vrq, bm34, ianum;
};

MVSIM_RECIPE_FN PtrsSetup ptrs_setup(double lambda)
{
    PtrsSetup s;
    const double slam = sqrt(lambda);
    s.b = 0.931 + 2.53 * slam;
    s.a = -0.059 + 0.02483 * s.b;
    s.bm2 = s.b - 2.0;
    s.vrq = 0.9277 * s.bm2 - 3.6224;        // V <= vr  <=>  V*(b-2) <= 0.9277*(b-2) - 3.6224
    s.bm34 = s.b - 3.4;
    s.ianum = 1.1239 * s.bm34 + 1.1328;      // invalpha = ianum / bm34
    return s;
}

// One attempt's squeeze.  Returns 0: accepted (kd is the sample), 1: rejected, 2: needs the exact test.
MVSIM_RECIPE_FN int ptrs_fast(const PtrsSetup& s, double lambda, uint32_t w0, uint32_t w1, double& us, double& V, double& kd)
{
    const double U = u32_open(w0) - 0.5;
    V = u32_open(w1);
    us = 0.5 - fabs(U);
    kd = floor((2.0 * s.a / us + s.b) * U + lambda + 0.43);
    if (us >= 0.07 && V * s.bm2 <= s.vrq) return 0;
    if (kd < 0.0 || (us < 0.013 && V > us)) return 1;
    return 2;
}

// The exact acceptance test of one attempt.
MVSIM_RECIPE_FN bool ptrs_exact(const PtrsSetup& s, double lambda, double us, double V, double kd, double& loglam, bool& have_loglam,
                                const double* lf = kLogFact)
{
    const double us2 = us * us;
    const double lhs = det_log((V * us2 * s.ianum) / (s.bm34 * (s.a + s.b * us2)));
    if (!have_loglam) { loglam = det_log(lambda); have_loglam = true; }
    const double rhs = (-lambda + kd * loglam) - det_lgamma_int((long long)kd, lf);
    return lhs <= rhs;
}

// fp32 screening of the exact test.  D = lhs - rhs is re-derived in a cancellation-free form (valid for k >= 16,
// Stirling branch):  with t = (k+1-lambda)/lambda,
//     rhs = lambda*g(t) + log1p(t) - log(k+1)/2 - log(2 pi)/2 - ser(k+1),   g(t) = t - (1+t) log1p(t) = -t^2/2 + t^3/6 - ...
// so every term is O(1..50) and single precision is accurate to ~1e-5 absolute.  Returns +1 (surely accept),
// -1 (surely reject) or 0 (too close to call: run the bit-defined fp64 test).  Pure optimisation: whenever it
// answers, the answer equals the fp64 decision (margin >= 100x the error bound), so counts are unchanged.
// The promise needs the fp64 test itself to be that accurate: its rhs sums terms of magnitude ~lambda log(lambda), so its own rounding
// grows like ~4 * 2^-53 * lambda log(lambda) -- 7e-8 at lambda = 1e7 (the margin to eps stays ~300x), but 1e-5 at 1e9 and 1e-2 at 1e12,
// where the screen's cancellation-free D and the fp64 decision part.  Above kScreenMaxLambda the fp64 test always decides.
constexpr double kScreenMaxLambda = 1.0e7;
MVSIM_RECIPE_FN int ptrs_screen(const PtrsSetup& s, double lambda, double us, double V, double kd, const double* lf = kLogFact)
{
    if (!(lambda < kScreenMaxLambda)) return 0;
    const float lam = (float)lambda;
    if (kd <= 16.0) {
        // table branch of log(k!): -lambda + k log(lambda) - log(k!) has terms of magnitude <= ~100 here
        // (lambda < ~60 for such k to be proposed at all), so single precision is good to ~1e-5 absolute
        if (lambda > 64.0) return 0;
        const float usq = (float)us * (float)us;
        const float q0 = ((float)V * usq * (float)s.ianum) / ((float)s.bm34 * ((float)s.a + (float)s.b * usq));
        const float kf = (float)kd;
        const float ll = MVSIM_RECIPE_LOGF(lam);
        const float d0 = MVSIM_RECIPE_LOGF(q0) - ((kf * ll - lam) - (float)lf[(int)kd]);
        const float e0 = 1.0e-4f + 4.0e-6f * (kf * ll + lam);
        return d0 < -e0 ? 1 : (d0 > e0 ? -1 : 0);
    }
    const float x = (float)kd + 1.0f;
    const float t = (float)((kd + 1.0 - lambda) / lambda);          // formed in double: no cancellation error
    const float usf = (float)us;
    const float us2 = usf * usf;
    const float q = ((float)V * us2 * (float)s.ianum) / ((float)s.bm34 * ((float)s.a + (float)s.b * us2));
    const float lhs = MVSIM_RECIPE_LOGF(q);
    float lg;                                                         // lambda * g(t) + log1p(t)
    if (fabsf(t) < 0.25f) {
        // g(t) = sum_{n>=2} (-1)^(n-1) t^n / (n (n-1));  log1p(t) = sum_{n>=1} (-1)^(n-1) t^n / n
        float g = 1.0f / 156.0f;                                      // n = 13
        g = fmaf(g, -t, 1.0f / 132.0f);
        g = fmaf(g, -t, 1.0f / 110.0f);
        g = fmaf(g, -t, 1.0f / 90.0f);
        g = fmaf(g, -t, 1.0f / 72.0f);
        g = fmaf(g, -t, 1.0f / 56.0f);
        g = fmaf(g, -t, 1.0f / 42.0f);
        g = fmaf(g, -t, 1.0f / 30.0f);
        g = fmaf(g, -t, 1.0f / 20.0f);
        g = fmaf(g, -t, 1.0f / 12.0f);
        g = fmaf(g, -t, 1.0f / 6.0f);
        g = fmaf(g, -t, 1.0f / 2.0f);
        g = -g * t * t;
        lg = lam * g + MVSIM_RECIPE_LOGF(1.0f + t);
    } else {
        const float l1p = MVSIM_RECIPE_LOGF(1.0f + t);
        lg = lam * (t - (1.0f + t) * l1p) + l1p;
    }
    const float ix = 1.0f / x;
    const float ix2 = ix * ix;
    const float ser = ix * (8.3333333e-02f + ix2 * (-2.7777778e-03f + ix2 * 7.9365079e-04f));
    const float lx = MVSIM_RECIPE_LOGF(x);
    const float rhs = lg - 0.5f * lx - 0.9189385f - ser;
    const float d = lhs - rhs;
    // error budget: each term carries <= ~3 ulp of single precision relative to its own magnitude (q: 5 roundings,
    // series: fma chain, v_log_f32: 1 ulp), i.e. <= 4e-7 * (|lhs| + |lg| + lx + 1); the margin below is >= 10x that.
    const float eps = 2.0e-5f + 4.0e-6f * (fabsf(lhs) + fabsf(lg) + lx);
    if (d < -eps) return 1;
    if (d > eps) return -1;
    return 0;
}

// One attempt of one voxel from its two random words: THE accept/reject of the recipe.  Returns true when the voxel is resolved.
MVSIM_RECIPE_FN bool ptrs_step_words(double lambda, uint32_t w0, uint32_t w1, float& res, const double* lf = kLogFact)
{
    const PtrsSetup s = ptrs_setup(lambda);
    double us, V, kd;
    const int st = ptrs_fast(s, lambda, w0, w1, us, V, kd);
    if (st == 1) return false;
#ifndef MVSIM_EXP_NOEXACT
    if (st == 2) {
        const int sc = ptrs_screen(s, lambda, us, V, kd, lf);
        if (sc < 0) return false;
        if (sc == 0) {
            double loglam = 0.0;
            bool have = false;
            if (!ptrs_exact(s, lambda, us, V, kd, loglam, have, lf)) return false;
        }
    }
#endif
    res = count_as_float(kd);
    return true;
}

// Attempt `att` of voxel `index`: the words of the attempt, its accept/reject, the cap.  (w0, w1): the attempt-0 words (pair_words) when
// att == 0; a retry draws its own into them.
MVSIM_RECIPE_FN bool ptrs_attempt(double lambda, uint32_t att, uint32_t& w0, uint32_t& w1, uint32_t k0, uint32_t k1, uint32_t stream,
                                  uint64_t index, float& res)
{
    if (att >= kPtrsMaxAttempts) {
        res = (float)(long long)lambda;         // lambda is no integer: truncated as the oracle's (int64_t)lambda, then rounded
        return true;
    }
    if (att != 0u) ptrs_retry_words(index, att, k0, k1, stream, w0, w1);
    return ptrs_step_words(lambda, w0, w1, res);
}

// Counter sampler v3 for one voxel, attempt by attempt from its own random words.
// lambda <= 0 or NaN -> 0 (the reference's loop does not terminate there; documented deviation Q9).
MVSIM_RECIPE_FN float poisson_voxel(double lambda, uint32_t k0, uint32_t k1, uint32_t stream, uint64_t index)
{
    if (!(lambda > 0.0)) return 0.0f;
    if (lambda < 10.0) {
        const Philox4 r = group_block(index, stream, k0, k1);
        return poisson_small(lambda, group_word(r, index));
    }
    const Philox4 r = pair_block(index, stream, k0, k1);
    uint32_t w0, w1;
    pair_words(r, index, w0, w1);
    float val = 0.f;
MVSIM_RECIPE_NO_UNROLL
    for (uint32_t att = 0u;; ++att)
        if (ptrs_attempt(lambda, att, w0, w1, k0, k1, stream, index, val)) return val;
}

// Four voxels index4 .. index4+3 (index4 % 4 == 0) sharing their group block and their two pair blocks: out[c] = poisson_voxel(lam[c],
// ..., index4 + c).  The attempt-0 squeeze of every bright voxel runs first, with all lanes busy; the voxels it does not settle (the
// exact test and / or retries, ~14 %) then take one attempt per trip, one voxel at a time, from attempt 0 again (ptrs_attempt: the same
// squeeze, now followed by the screen and the exact test), so the divergent code runs per pending voxel and not once per voxel slot.
MVSIM_RECIPE_FN void poisson_counter4(const double lam[4], uint32_t k0, uint32_t k1, uint32_t stream, uint64_t index4, float out[4])
{
    bool small_any = false;
MVSIM_RECIPE_UNROLL
    for (int c = 0; c < 4; ++c) {
        out[c] = 0.f;
        small_any |= lam[c] > 0.0 && lam[c] < 10.0;
    }
    if (small_any) {
        const Philox4 r = group_block(index4, stream, k0, k1);
MVSIM_RECIPE_UNROLL
        for (int c = 0; c < 4; ++c)
            if (lam[c] > 0.0 && lam[c] < 10.0) out[c] = poisson_small(lam[c], group_word(r, index4 + (uint64_t)c));
    }
    uint32_t pend = 0u, w0[4] = {0u, 0u, 0u, 0u}, w1[4] = {0u, 0u, 0u, 0u};      // bit c: voxel c unresolved; its attempt-0 words
MVSIM_RECIPE_UNROLL
    for (int h = 0; h < 2; ++h)
        if (lam[2 * h] >= 10.0 || lam[2 * h + 1] >= 10.0) {
            const Philox4 r = pair_block(index4 + 2u * (uint64_t)h, stream, k0, k1);
MVSIM_RECIPE_UNROLL
            for (int c = 2 * h; c < 2 * h + 2; ++c)
                if (lam[c] >= 10.0) {
                    pair_words(r, index4 + (uint64_t)c, w0[c], w1[c]);
                    double us, V, kd;
                    if (ptrs_fast(ptrs_setup(lam[c]), lam[c], w0[c], w1[c], us, V, kd) == 0) out[c] = count_as_float(kd);
                    else pend |= 1u << c;
                }
        }
    uint32_t att = 0u;                                                         // of the lowest pending voxel
    while (pend != 0u) {
        const int v = __builtin_ffs((int)pend) - 1;
        const double l = v == 0 ? lam[0] : (v == 1 ? lam[1] : (v == 2 ? lam[2] : lam[3]));
        uint32_t a0 = v == 0 ? w0[0] : (v == 1 ? w0[1] : (v == 2 ? w0[2] : w0[3]));
        uint32_t a1 = v == 0 ? w1[0] : (v == 1 ? w1[1] : (v == 2 ? w1[2] : w1[3]));
        float res = 0.f;
        if (ptrs_attempt(l, att, a0, a1, k0, k1, stream, index4 + (uint64_t)v, res)) {
            if (v == 0) out[0] = res; else if (v == 1) out[1] = res; else if (v == 2) out[2] = res; else out[3] = res;
            pend &= pend - 1u;
            att = 0u;
        } else {
            att += 1u;
        }
    }
}

// Tools.adjustImage on one voxel: (float)(v * corr), then + minValue as a second float rounding (Tools.java:150-155)
MVSIM_RECIPE_FN float adjust_one(float v, double corr, float min_value)
{
    const float t = (float)((double)v * corr);  // pass 1, Tools.java:150-151
    return t + min_value;                       // pass 2, Tools.java:154-155 (second rounding, Q6)
}

}  // namespace mvsim
