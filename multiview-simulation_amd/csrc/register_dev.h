// The arithmetic of the bead registration that the device kernels (register.hip) and the host (mvsim_fit_affine in api_register.cpp)
// share, stated once: squared distances, the rank triples, the descriptor distance, the sums of the affine fit and its solve, the
// residual, a hypothesis's draw.  mvsim.h states the recipe; every + - * / sqrt here is an operation of its own (the build has
// -ffp-contract=off).  Plain C++ outside hipcc.
#pragma once

#include "jrandom.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MVSIM_REG_FN __host__ __device__ __forceinline__
#else
#define MVSIM_REG_FN inline
#endif

namespace mvsim {

constexpr int REG_FIT_CHUNK = 256;                       // MVSIM_REG_FIT_CHUNK
constexpr int REG_MAX_K = 5, REG_MAX_SUBSETS = 10;
constexpr int REG_EMPTY = 0x7fffffff;                    // the index of an empty slot: sorts behind every point at d2 = +inf
constexpr int REG_MAX_DRAWS = 32;

MVSIM_REG_FN double reg_nan() { return __builtin_nan(""); }
MVSIM_REG_FN double reg_inf() { return __builtin_inf(); }
MVSIM_REG_FN bool reg_finite(double v) { return v - v == 0.0; }
MVSIM_REG_FN bool reg_finite3(double x, double y, double z) { return reg_finite(x) && reg_finite(y) && reg_finite(z); }

MVSIM_REG_FN double reg_d2(double ax, double ay, double az, double bx, double by, double bz)
{
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// (value, index) as a total order; no NaN reaches it
MVSIM_REG_FN bool reg_less(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }

MVSIM_REG_FN int reg_subset_count(int K) { return K * (K - 1) * (K - 2) / 6; }

// rank triple s of K neighbours, lexicographic
MVSIM_REG_FN void reg_subset(int K, int s, int t[3])
{
    int at = 0;
    for (int i = 0; i < K - 2; ++i)
        for (int j = i + 1; j < K - 1; ++j)
            for (int k = j + 1; k < K; ++k) {
                if (at == s) { t[0] = i; t[1] = j; t[2] = k; }
                ++at;
            }
}

MVSIM_REG_FN double reg_desc_dist(const double* u, const double* w)
{
    const double e0 = u[0] - w[0], e1 = u[1] - w[1], e2 = u[2] - w[2], e3 = u[3] - w[3], e4 = u[4] - w[4], e5 = u[5] - w[5];
    return ((((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3) + e4 * e4) + e5 * e5;
}

// ---- step 4: the sums, one pair (p = pq[0..2] -> q = pq[3..5]) at a time ------------------------------------------------------------
MVSIM_REG_FN void reg_acc_centroid(double acc[6], const double pq[6])
{
    for (int t = 0; t < 6; ++t) acc[t] = acc[t] + pq[t];
}

// acc: xx xy xz yy yz zz of p', then c00 c01 c02 c10 .. c22 of q' p'^T
MVSIM_REG_FN void reg_acc_moments(double acc[15], const double pq[6], const double cen[6])
{
    const double px = pq[0] - cen[0], py = pq[1] - cen[1], pz = pq[2] - cen[2];
    const double qx = pq[3] - cen[3], qy = pq[4] - cen[4], qz = pq[5] - cen[5];
    acc[0] = acc[0] + px * px; acc[1] = acc[1] + px * py; acc[2] = acc[2] + px * pz;
    acc[3] = acc[3] + py * py; acc[4] = acc[4] + py * pz; acc[5] = acc[5] + pz * pz;
    acc[6] = acc[6] + qx * px; acc[7] = acc[7] + qx * py; acc[8] = acc[8] + qx * pz;
    acc[9] = acc[9] + qy * px; acc[10] = acc[10] + qy * py; acc[11] = acc[11] + qy * pz;
    acc[12] = acc[12] + qz * px; acc[13] = acc[13] + qz * py; acc[14] = acc[14] + qz * pz;
}

MVSIM_REG_FN void reg_centroid(const double sum[6], long long n, double cen[6])
{
    const double dn = (double)n;
    for (int t = 0; t < 6; ++t) cen[t] = sum[t] / dn;
}

// A = C Sm^-1, t = cq - A cp; false: no model (m untouched)
MVSIM_REG_FN bool reg_solve(const double cen[6], const double mom[15], double m[12])
{
    const double m00 = mom[0], m01 = mom[1], m02 = mom[2], m10 = mom[1], m11 = mom[3], m12 = mom[4], m20 = mom[2], m21 = mom[4], m22 = mom[5];
    const double det = m00 * m11 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20 - m00 * m12 * m21 - m01 * m10 * m22;
    if (det == 0.0 || !reg_finite(det)) return false;
    const double idet = 1.0 / det;
    double inv[3][3];
    inv[0][0] = (m11 * m22 - m12 * m21) * idet; inv[0][1] = (m02 * m21 - m01 * m22) * idet; inv[0][2] = (m01 * m12 - m02 * m11) * idet;
    inv[1][0] = (m12 * m20 - m10 * m22) * idet; inv[1][1] = (m00 * m22 - m02 * m20) * idet; inv[1][2] = (m02 * m10 - m00 * m12) * idet;
    inv[2][0] = (m10 * m21 - m11 * m20) * idet; inv[2][1] = (m01 * m20 - m00 * m21) * idet; inv[2][2] = (m00 * m11 - m01 * m10) * idet;
    for (int r = 0; r < 3; ++r) {
        const double* c = mom + 6 + 3 * r;
        double a[3];
        for (int k = 0; k < 3; ++k) a[k] = (c[0] * inv[0][k] + c[1] * inv[1][k]) + c[2] * inv[2][k];
        m[4 * r + 0] = a[0]; m[4 * r + 1] = a[1]; m[4 * r + 2] = a[2];
        m[4 * r + 3] = cen[3 + r] - ((a[0] * cen[0] + a[1] * cen[1]) + a[2] * cen[2]);
    }
    return true;
}

// The fit as ONE walk: `items` slots in ascending candidate order; slot k is candidate items.index(k), taken if items.selected(k),
// its pair read by items.load(k, pq).  What the host and a hypothesis run (the refit kernel gives every chunk a thread of its own and
// adds the chunks' sums in the same order).
template <class Items> MVSIM_REG_FN bool reg_fit_walk(const Items& items, double m[12])
{
    const int slots = items.count();
    double total[15], chunk[15], cen[6], pq[6];
    long long n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int terms = pass == 0 ? 6 : 15;
        for (int t = 0; t < terms; ++t) { total[t] = 0.0; chunk[t] = 0.0; }
        int cur = -1;
        for (int k = 0; k < slots; ++k) {
            if (!items.selected(k)) continue;
            const int c = items.index(k) / REG_FIT_CHUNK;
            if (c != cur) {
                for (int t = 0; t < terms; ++t) { total[t] = total[t] + chunk[t]; chunk[t] = 0.0; }
                cur = c;
            }
            items.load(k, pq);
            if (pass == 0) { reg_acc_centroid(chunk, pq); ++n; }
            else reg_acc_moments(chunk, pq, cen);
        }
        for (int t = 0; t < terms; ++t) total[t] = total[t] + chunk[t];
        if (pass == 0) {
            if (n < 4) return false;
            reg_centroid(total, n, cen);
        }
    }
    return reg_solve(cen, total, m);
}

// e2 of one pair under a model
MVSIM_REG_FN double reg_residual2(const double m[12], const double pq[6])
{
    const double ex = (((m[0] * pq[0] + m[1] * pq[1]) + m[2] * pq[2]) + m[3]) - pq[3];
    const double ey = (((m[4] * pq[0] + m[5] * pq[1]) + m[6] * pq[2]) + m[7]) - pq[4];
    const double ez = (((m[8] * pq[0] + m[9] * pq[1]) + m[10] * pq[2]) + m[11]) - pq[5];
    return (ex * ex + ey * ey) + ez * ez;
}

// hypothesis h: 4 distinct indices below M from java.util.Random(seed + h), sorted ascending; false: void
MVSIM_REG_FN bool reg_draw4(long long seed, long long h, int M, int idx[4])
{
    JRandom rnd{(((uint64_t)seed + (uint64_t)h) ^ JR_A) & JR_MASK};     // the sum wraps as a Java long does
    int have = 0;
    for (int draw = 0; draw < REG_MAX_DRAWS && have < 4; ++draw) {
        const int v = rnd.next_int(M);
        bool fresh = true;
        for (int k = 0; k < have; ++k) fresh = fresh && idx[k] != v;
        if (fresh) idx[have++] = v;
    }
    if (have < 4) return false;
    for (int i = 1; i < 4; ++i)
        for (int j = i; j > 0 && idx[j - 1] > idx[j]; --j) { const int t = idx[j - 1]; idx[j - 1] = idx[j]; idx[j] = t; }
    return true;
}

// four pairs in registers as the items of reg_fit_walk
struct RegFour {
    int idx[4];
    double pq[4][6];
    MVSIM_REG_FN int count() const { return 4; }
    MVSIM_REG_FN int index(int k) const { return idx[k]; }
    MVSIM_REG_FN bool selected(int) const { return true; }
    MVSIM_REG_FN void load(int k, double out[6]) const { for (int t = 0; t < 6; ++t) out[t] = pq[k][t]; }
};

}  // namespace mvsim
