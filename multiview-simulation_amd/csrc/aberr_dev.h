// Device functions the ray tracers share (aberrations.hip: refract3d, projectToCamera; raytrace.hip: caller-supplied rays): the
// interpolating accessor, the Hessian by the reference's moves, the largest eigenpair, one move's refraction, and the ray starts of
// the two reference families.  Every function is the reference's arithmetic with its rounding points (the build compiles with
// -ffp-contract=off); the units that include this header must produce the same bits from it.
#pragma once

#include "common.h"
#include "jrandom.h"

#include <cmath>

namespace mvsim {

namespace {

// ---- the interpolating accessor (ImgLib2 NLinearInterpolator over Views.extendMirrorSingle) ---------------------------------
__device__ __forceinline__ int mirror_single(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    const int period = 2 * n - 2;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

struct Accessor {
    const float* img;
    int nx, ny, nz;
    double px, py, pz;      // the real position
    int tx, ty, tz;         // the lower-corner tap
    __device__ __forceinline__ void set(double x, double y, double z)
    {
        px = x; py = y; pz = z;
        tx = (int)floor(x); ty = (int)floor(y); tz = (int)floor(z);
    }
    template <int D> __device__ __forceinline__ void fwd()
    {
        if (D == 0) { px += 1.0; tx += 1; } else if (D == 1) { py += 1.0; ty += 1; } else { pz += 1.0; tz += 1; }
    }
    template <int D> __device__ __forceinline__ void bck()
    {
        if (D == 0) { px -= 1.0; tx -= 1; } else if (D == 1) { py -= 1.0; ty -= 1; } else { pz -= 1.0; tz -= 1; }
    }
    __device__ __forceinline__ void move(double dx, double dy, double dz)
    {
        px += dx; tx = (int)floor(px);
        py += dy; ty = (int)floor(py);
        pz += dz; tz = (int)floor(pz);
    }
    __device__ __forceinline__ float tap(int x, int y, int z) const
    {
        return img[(long long)mirror_single(x, nx) + (long long)nx * ((long long)mirror_single(y, ny) + (long long)ny * mirror_single(z, nz))];
    }
    // taps in Gray-code order, each (float)(v * w) with the weight product in fp64, float accumulation
    __device__ __forceinline__ float get() const
    {
        const double w0 = px - (double)tx, w1 = py - (double)ty, w2 = pz - (double)tz;
        const double w0n = 1.0 - w0, w1n = 1.0 - w1, w2n = 1.0 - w2;
        const int x0 = mirror_single(tx, nx), x1 = mirror_single(tx + 1, nx);
        const long long y0 = (long long)nx * mirror_single(ty, ny), y1 = (long long)nx * mirror_single(ty + 1, ny);
        const long long z0 = (long long)nx * ny * mirror_single(tz, nz), z1 = (long long)nx * ny * mirror_single(tz + 1, nz);
        float s = (float)((double)img[x0 + y0 + z0] * (w0n * w1n * w2n));
        s += (float)((double)img[x1 + y0 + z0] * (w0 * w1n * w2n));
        s += (float)((double)img[x1 + y1 + z0] * (w0 * w1 * w2n));
        s += (float)((double)img[x0 + y1 + z0] * (w0n * w1 * w2n));
        s += (float)((double)img[x0 + y1 + z1] * (w0n * w1 * w2));
        s += (float)((double)img[x1 + y1 + z1] * (w0 * w1 * w2));
        s += (float)((double)img[x1 + y0 + z1] * (w0 * w1n * w2));
        s += (float)((double)img[x0 + y0 + z1] * (w0n * w1n * w2));
        return s;
    }
};

// ---- Hessian.computeHessianMatrix3D (:155-278) by the reference's moves -----------------------------------------------------
template <int D> __device__ __forceinline__ double hess_second(Accessor& a, double temp)
{
    a.fwd<D>();
    double h = (double)a.get();
    h -= temp;
    a.bck<D>();
    a.bck<D>();
    h += (double)a.get();
    a.fwd<D>();
    return h;
}

template <int U, int V> __device__ __forceinline__ double hess_mixed(Accessor& a)
{
    a.fwd<U>(); a.fwd<V>();
    const double p = (double)a.get();
    a.bck<U>(); a.bck<U>();
    const double q = (double)a.get();
    a.fwd<U>(); a.fwd<U>(); a.bck<V>(); a.bck<V>();
    const double r = (double)a.get();
    a.bck<U>(); a.bck<U>();
    const double s = (double)a.get();
    a.fwd<U>(); a.fwd<V>();
    return ((p - q) / 2 - (r - s) / 2) / 2;
}

// m = {xx, yy, zz, xy, xz, yz}
__device__ __forceinline__ void hessian_by_moves(Accessor& a, double m[6])
{
    const double temp = (double)(2 * a.get());
    m[0] = hess_second<0>(a, temp);
    m[1] = hess_second<1>(a, temp);
    m[2] = hess_second<2>(a, temp);
    m[3] = hess_mixed<0, 1>(a);
    m[4] = hess_mixed<0, 2>(a);
    m[5] = hess_mixed<1, 2>(a);
}

// ---- Hessian.computeLargestEigenVectorAndValue3d (:110-147): JAMA's symmetric path for n = 3 ---------------------------------
__device__ __forceinline__ double jama_hypot(double a, double b)
{
    double r;
    if (fabs(a) > fabs(b)) { r = b / a; r = fabs(a) * sqrt(1 + r * r); }
    else if (b != 0) { r = a / b; r = fabs(b) * sqrt(1 + r * r); }
    else r = 0.0;
    return r;
}

constexpr int QL_MAX_SWEEPS = 64;     // JAMA has no limit; a matrix of finite entries converges in a handful of sweeps

// m = {xx, yy, zz, xy, xz, yz}; returns the eigenvalue of largest magnitude (first wins on ties, eigenvalues ascending) and its
// eigenvector with the sign the decomposition gives it
__device__ double largest_eigenpair(const double m[6], double vec[3])
{
    constexpr int N = 3;
    double V[N][N] = {{m[0], m[3], m[4]}, {m[3], m[1], m[5]}, {m[4], m[5], m[2]}};
    double d[N], e[N];
    // tred2
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] = V[N - 1][j];
#pragma unroll
    for (int i = N - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) scale = scale + fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
#pragma unroll
            for (int j = 0; j < i; ++j) { d[j] = V[i - 1][j]; V[i][j] = 0.0; V[j][i] = 0.0; }
        } else {
#pragma unroll
            for (int k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
            double f = d[i - 1];
            double g = sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h = h - f * g;
            d[i - 1] = f - g;
#pragma unroll
            for (int j = 0; j < i; ++j) e[j] = 0.0;
#pragma unroll
            for (int j = 0; j < i; ++j) {
                f = d[j];
                V[j][i] = f;
                g = e[j] + V[j][j] * f;
#pragma unroll
                for (int k = j + 1; k <= i - 1; ++k) { g += V[k][j] * d[k]; e[k] += V[k][j] * f; }
                e[j] = g;
            }
            f = 0.0;
#pragma unroll
            for (int j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
            const double hh = f / (h + h);
#pragma unroll
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
#pragma unroll
            for (int j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
#pragma unroll
                for (int k = j; k <= i - 1; ++k) V[k][j] -= (f * e[k] + g * d[k]);
                d[j] = V[i - 1][j];
                V[i][j] = 0.0;
            }
        }
        d[i] = h;
    }
#pragma unroll
    for (int i = 0; i < N - 1; ++i) {
        V[N - 1][i] = V[i][i];
        V[i][i] = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
#pragma unroll
            for (int k = 0; k <= i; ++k) d[k] = V[k][i + 1] / h;
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double g = 0.0;
#pragma unroll
                for (int k = 0; k <= i; ++k) g += V[k][i + 1] * V[k][j];
#pragma unroll
                for (int k = 0; k <= i; ++k) V[k][j] -= g * d[k];
            }
        }
#pragma unroll
        for (int k = 0; k <= i; ++k) V[k][i + 1] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) { d[j] = V[N - 1][j]; V[N - 1][j] = 0.0; }
    V[N - 1][N - 1] = 1.0;
    e[0] = 0.0;

    // tql2
#pragma unroll
    for (int i = 1; i < N; ++i) e[i - 1] = e[i];
    e[N - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = 0x1.0p-52;
#pragma unroll
    for (int l = 0; l < N; ++l) {
        const double t = fabs(d[l]) + fabs(e[l]);
        tst1 = tst1 > t ? tst1 : t;
        int mm = l;
#pragma unroll
        for (int q = l; q < N; ++q)               // while (m < n) { if (|e[m]| <= eps tst1) break; m++; }; e[n-1] == 0 ends it
            if (mm == q && !(fabs(e[q]) <= eps * tst1)) mm = q + 1;
        if (mm > N - 1) mm = N - 1;               // only a NaN reaches this: e[n-1] == 0 passes the test otherwise
        if (mm > l) {
            int iter = 0;
            do {
                iter = iter + 1;
                double g = d[l];
                double p = (d[l + 1 < N ? l + 1 : l] - g) / (2.0 * e[l]);
                double r = jama_hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1 < N ? l + 1 : l] = e[l] * (p + r);
                const double dl1 = d[l + 1 < N ? l + 1 : l];
                double h = g - d[l];
#pragma unroll
                for (int i = l + 2; i < N; ++i) d[i] -= h;
                f = f + h;
                p = mm == 2 ? d[2] : d[1];
                double c = 1.0, c2 = c, c3 = c;
                const double el1 = e[l + 1 < N ? l + 1 : l];
                double s = 0.0, s2 = 0.0;
#pragma unroll
                for (int i = N - 2; i >= l; --i) {
                    if (i > mm - 1) continue;
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = jama_hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        h = V[k][i + 1];
                        V[k][i + 1] = s * V[k][i] + c * h;
                        V[k][i] = c * V[k][i] - s * h;
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (fabs(e[l]) > eps * tst1 && iter < QL_MAX_SWEEPS);
        }
        d[l] = d[l] + f;
        e[l] = 0.0;
    }
    // ascending order, columns swapped with their values
#pragma unroll
    for (int i = 0; i < N - 1; ++i) {
        int k = i;
        double p = d[i];
#pragma unroll
        for (int j = i + 1; j < N; ++j)
            if (d[j] < p) { k = j; p = d[j]; }
        if (k != i) {
#pragma unroll
            for (int j = i + 1; j < N; ++j)
                if (j == k) {
                    d[j] = d[i];
#pragma unroll
                    for (int r = 0; r < N; ++r) { const double t = V[r][i]; V[r][i] = V[r][j]; V[r][j] = t; }
                }
            d[i] = p;
        }
    }
    int idx = 0;
    double best = d[0];
#pragma unroll
    for (int i = 1; i < N; ++i)
        if (fabs(d[i]) > fabs(best)) { best = d[i]; idx = i; }
#pragma unroll
    for (int r = 0; r < N; ++r) vec[r] = idx == 0 ? V[r][0] : (idx == 1 ? V[r][1] : V[r][2]);
    return best;
}

// ---- Raytrace ---------------------------------------------------------------------------------------------------------------
constexpr double HALF_PI = 1.5707963267948966;      // Math.PI / 2

__device__ __forceinline__ void norm3(double v[3])
{
    const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
}

// Raytrace.reflect (:32-40): i - 2 (i . n) n with the products in the reference's order
__device__ __forceinline__ void reflect3(const double i[3], const double n[3], double r[3])
{
    const double dot = i[0] * n[0] + i[1] * n[1] + i[2] * n[2];
    r[0] = i[0] - 2 * dot * n[0];
    r[1] = i[1] - 2 * dot * n[1];
    r[2] = i[2] - 2 * dot * n[2];
}

// One move's refraction (SimulateMultiViewAberrations.java:155-214 and :331-378): the Hessian of the index volume at pos, and where
// its largest eigenvalue exceeds evThreshold in magnitude (0.01 in every reference loop), Snell's law across the plane its
// eigenvector is normal to.  REFLECT: on total reflection the ray takes Raytrace.reflect (the line the reference has commented
// out) instead of keeping its direction.
template <bool REFLECT = false>
__device__ __forceinline__ void refract_step(Accessor& ri, const double pos[3], double vec[3], double nA, double nB, double evThreshold)
{
    double m[6], en[3];
    ri.set(pos[0], pos[1], pos[2]);
    hessian_by_moves(ri, m);
    const double ev = largest_eigenpair(m, en);
    if (fabs(ev) > evThreshold) {
        ri.set(pos[0], pos[1], pos[2]);
        ri.move(-vec[0], -vec[1], -vec[2]);
        const double i0 = (double)ri.get();
        ri.move(2 * vec[0], 2 * vec[1], 2 * vec[2]);
        const double i1 = (double)ri.get();
        const double n0 = (nB - nA) * i0 + nA;
        const double n1 = (nB - nA) * i1 + nA;
        // Raytrace.incidentAngle (:75-93), quirk kept: the normal is flipped and the angle reduced by pi / 2 (not mirrored)
        double thetaI = acos((en[0] * vec[0] + en[1] * vec[1] + en[2] * vec[2]) /
                             (sqrt(en[0] * en[0] + en[1] * en[1] + en[2] * en[2]) * sqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2])));
        if (thetaI >= HALF_PI) {
            en[0] *= -1; en[1] *= -1; en[2] *= -1;
            thetaI -= HALF_PI;
        }
        // Raytrace.refract (:42-59); total reflection (NaN): the ray keeps its direction
        const double deltaN = n0 / n1;
        const double thetaT = asin(deltaN * sin(thetaI));
        double t[3] = {vec[0], vec[1], vec[2]};
        if (thetaT == thetaT) {
            const double cosThetaI = cos(thetaI);
            const double sinThetaT = sin(thetaT);
            const double k = deltaN * cosThetaI - sqrt(1 - sinThetaT * sinThetaT);
            t[0] = deltaN * vec[0] - en[0] * k;
            t[1] = deltaN * vec[1] - en[1] * k;
            t[2] = deltaN * vec[2] - en[2] * k;
        } else if (REFLECT) {
            reflect3(vec, en, t);
        }
        norm3(t);
        vec[0] = t[0]; vec[1] = t[1]; vec[2] = t[2];
    }
}

__device__ __forceinline__ bool inside3(const double p[3], int nx, int ny, int nz)
{
    return !(p[0] < 0.0 || p[0] > (double)(nx - 1) || p[1] < 0.0 || p[1] > (double)(ny - 1) || p[2] < 0.0 || p[2] > (double)(nz - 1));
}

// ---- ray starts -------------------------------------------------------------------------------------------------------------
struct SheetParams {
    unsigned long long state;     // java.util.Random state in front of ray 0
    double a, b, c;               // Lightsheet: a x x + b x + c
    int    illum, z;
};

// refract3d :309-319: ray i consumes draws 3i .. 3i + 2 of nextDouble(), two generator steps each
__device__ __forceinline__ void sheet_ray_start(const SheetParams& sp, long long ray, int nx, int ny, double pos[3], double vec[3])
{
    JRandom rnd{jr_jump(sp.state, 6ULL * (unsigned long long)ray)};
    pos[0] = rnd.next_double() * (double)(nx - 1);
    pos[1] = sp.illum ? (double)(ny - 1) : 0.0;
    const double th = sp.a * pos[0] * pos[0] + sp.b * pos[0] + sp.c;
    pos[2] = (double)sp.z + (rnd.next_double() * th) - th / 2.0;
    vec[0] = (rnd.next_double() - 0.5) / 5;
    vec[1] = sp.illum ? -1.0 : 1.0;
    vec[2] = 0.0;
    norm3(vec);
}

// projectToCamera :137-143: ray (pixel p, i) consumes draws 2 (rays p + i) ..; start z = 1, direction +z
__device__ __forceinline__ void camera_ray_start(unsigned long long state, long long ray, int px, int py, double pos[3], double vec[3])
{
    JRandom rnd{jr_jump(state, 4ULL * (unsigned long long)ray)};
    pos[0] = (double)px + (rnd.next_double() - 0.5);
    pos[1] = (double)py + (rnd.next_double() - 0.5);
    pos[2] = 1.0;
    vec[0] = 0.0; vec[1] = 0.0; vec[2] = 1.0;
}

}  // namespace

}  // namespace mvsim
