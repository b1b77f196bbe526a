/* Sequential restatement of the refraction simulator (SimulateMultiViewAberrations, Hessian, Raytrace, Lightsheet,
 * VolumeInjection) for the tests: one ray after the other, a literal java.util.Random, fp64 where the reference computes in
 * double and float where it stores floats.  Built by tests/aberrations_restatement.py with gcc -O2 -ffp-contract=off.
 *
 * The five libm functions the reference reaches (acos, asin, sin, cos, exp) go through wrappers, so that the tests can run
 * the same code with every libm result moved by one ulp, alternating up and down ("the twin"), and see how far that carries.
 *
 * Third-party semantics restated from the published algorithms:
 *   ImgLib2 NLinearInterpolator over extendMirrorSingle: the accessor keeps an fp64 position and the integer position of its
 *     lower-corner tap; setPosition / move(distance) set the tap to floor(position), fwd / bck move both by one; the weights
 *     are position - tap per axis; taps in Gray-code order, each (float)(v * w), float accumulation.
 *   JAMA EigenvalueDecomposition of a symmetric matrix: tred2 + tql2 (EISPACK), eigenvalues ascending.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define HALF_PI 1.5707963267948966 /* Math.PI / 2 */
static int g_twin = 0;
static uint64_t g_calls = 0;

static double bend(double r)
{
    if (!g_twin || r != r) return r;
    return nextafter(r, (g_calls++ & 1) ? INFINITY : -INFINITY);
}
static double m_acos(double x) { return bend(acos(x)); }
static double m_asin(double x) { return bend(asin(x)); }
static double m_sin(double x) { return bend(sin(x)); }
static double m_cos(double x) { return bend(cos(x)); }
static double m_exp(double x) { return bend(exp(x)); }

void rs_set_twin(int on) { g_twin = on; g_calls = 0; }

/* ---- java.util.Random ------------------------------------------------------------------------------------------------- */
static int32_t jr_next(uint64_t* s, int bits)
{
    *s = (*s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
    return (int32_t)((int64_t)*s >> (48 - bits));
}
static double jr_double(uint64_t* s)
{
    const int64_t hi = (int64_t)jr_next(s, 26) << 27;
    return (double)(hi + jr_next(s, 27)) * 0x1.0p-53;
}

/* ---- the interpolating accessor ---------------------------------------------------------------------------------------- */
typedef struct { const float* img; int64_t dim[3]; double p[3]; int64_t t[3]; } acc_t;

static int64_t mirror(int64_t i, int64_t n)
{
    const int64_t period = 2 * n - 2;
    if (i >= 0 && i < n) return i;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}
static float tap(const acc_t* a, int64_t x, int64_t y, int64_t z)
{
    x = mirror(x, a->dim[0]); y = mirror(y, a->dim[1]); z = mirror(z, a->dim[2]);
    return a->img[x + a->dim[0] * (y + a->dim[1] * z)];
}
static void acc_set(acc_t* a, const double p[3])
{
    for (int d = 0; d < 3; ++d) { a->p[d] = p[d]; a->t[d] = (int64_t)floor(p[d]); }
}
static void acc_fwd(acc_t* a, int d) { a->p[d] += 1.0; a->t[d] += 1; }
static void acc_bck(acc_t* a, int d) { a->p[d] -= 1.0; a->t[d] -= 1; }
static void acc_move(acc_t* a, double dist, int d) { a->p[d] += dist; a->t[d] = (int64_t)floor(a->p[d]); }
static float acc_get(const acc_t* a)
{
    const int64_t x = a->t[0], y = a->t[1], z = a->t[2];
    const double w0 = a->p[0] - (double)x, w1 = a->p[1] - (double)y, w2 = a->p[2] - (double)z;
    const double w0n = 1.0 - w0, w1n = 1.0 - w1, w2n = 1.0 - w2;
    float s = (float)((double)tap(a, x, y, z) * (w0n * w1n * w2n));
    s += (float)((double)tap(a, x + 1, y, z) * (w0 * w1n * w2n));
    s += (float)((double)tap(a, x + 1, y + 1, z) * (w0 * w1 * w2n));
    s += (float)((double)tap(a, x, y + 1, z) * (w0n * w1 * w2n));
    s += (float)((double)tap(a, x, y + 1, z + 1) * (w0n * w1 * w2));
    s += (float)((double)tap(a, x + 1, y + 1, z + 1) * (w0 * w1 * w2));
    s += (float)((double)tap(a, x + 1, y, z + 1) * (w0 * w1n * w2));
    s += (float)((double)tap(a, x, y, z + 1) * (w0n * w1n * w2));
    return s;
}

/* ---- Hessian by moves of the accessor ---------------------------------------------------------------------------------- */
static double second(acc_t* a, int d, double temp)
{
    double h;
    acc_fwd(a, d);
    h = acc_get(a);
    h -= temp;
    acc_bck(a, d);
    acc_bck(a, d);
    h += acc_get(a);
    acc_fwd(a, d);
    return h;
}
static double mixed(acc_t* a, int u, int v)
{
    double p, q, r, s;
    acc_fwd(a, u); acc_fwd(a, v);
    p = acc_get(a);
    acc_bck(a, u); acc_bck(a, u);
    q = acc_get(a);
    acc_fwd(a, u); acc_fwd(a, u); acc_bck(a, v); acc_bck(a, v);
    r = acc_get(a);
    acc_bck(a, u); acc_bck(a, u);
    s = acc_get(a);
    acc_fwd(a, u); acc_fwd(a, v);
    return ((p - q) / 2 - (r - s) / 2) / 2;
}
static void hessian(acc_t* a, double m[9])
{
    const double temp = 2 * acc_get(a);
    m[0] = second(a, 0, temp);
    m[4] = second(a, 1, temp);
    m[8] = second(a, 2, temp);
    m[1] = m[3] = mixed(a, 0, 1);
    m[2] = m[6] = mixed(a, 0, 2);
    m[5] = m[7] = mixed(a, 1, 2);
}

/* ---- symmetric 3 x 3 eigen-decomposition: Householder tridiagonalisation, then implicit QL ------------------------------ */
static double hyp(double a, double b)
{
    double r;
    if (fabs(a) > fabs(b)) { r = b / a; r = fabs(a) * sqrt(1 + r * r); }
    else if (b != 0) { r = a / b; r = fabs(b) * sqrt(1 + r * r); }
    else r = 0.0;
    return r;
}

#define N 3
#define QL_MAX_SWEEPS 64
static void eig_sym(const double A[9], double d[N], double V[N][N])
{
    double e[N];
    int i, j, k, l;
    for (i = 0; i < N; ++i) for (j = 0; j < N; ++j) V[i][j] = A[3 * i + j];
    for (j = 0; j < N; ++j) d[j] = V[N - 1][j];
    for (i = N - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (k = 0; k < i; ++k) scale = scale + fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (j = 0; j < i; ++j) { d[j] = V[i - 1][j]; V[i][j] = 0.0; V[j][i] = 0.0; }
        } else {
            double f, g, hh;
            for (k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
            f = d[i - 1];
            g = sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h = h - f * g;
            d[i - 1] = f - g;
            for (j = 0; j < i; ++j) e[j] = 0.0;
            for (j = 0; j < i; ++j) {
                f = d[j];
                V[j][i] = f;
                g = e[j] + V[j][j] * f;
                for (k = j + 1; k <= i - 1; ++k) { g += V[k][j] * d[k]; e[k] += V[k][j] * f; }
                e[j] = g;
            }
            f = 0.0;
            for (j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
            hh = f / (h + h);
            for (j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
                for (k = j; k <= i - 1; ++k) V[k][j] -= (f * e[k] + g * d[k]);
                d[j] = V[i - 1][j];
                V[i][j] = 0.0;
            }
        }
        d[i] = h;
    }
    for (i = 0; i < N - 1; ++i) {
        double h;
        V[N - 1][i] = V[i][i];
        V[i][i] = 1.0;
        h = d[i + 1];
        if (h != 0.0) {
            for (k = 0; k <= i; ++k) d[k] = V[k][i + 1] / h;
            for (j = 0; j <= i; ++j) {
                double g = 0.0;
                for (k = 0; k <= i; ++k) g += V[k][i + 1] * V[k][j];
                for (k = 0; k <= i; ++k) V[k][j] -= g * d[k];
            }
        }
        for (k = 0; k <= i; ++k) V[k][i + 1] = 0.0;
    }
    for (j = 0; j < N; ++j) { d[j] = V[N - 1][j]; V[N - 1][j] = 0.0; }
    V[N - 1][N - 1] = 1.0;
    e[0] = 0.0;

    for (i = 1; i < N; ++i) e[i - 1] = e[i];
    e[N - 1] = 0.0;
    {
        double f = 0.0, tst1 = 0.0;
        const double eps = 0x1.0p-52;
        for (l = 0; l < N; ++l) {
            int m = l;
            const double t = fabs(d[l]) + fabs(e[l]);
            tst1 = tst1 > t ? tst1 : t;
            while (m < N) {
                if (fabs(e[m]) <= eps * tst1) break;
                m++;
            }
            if (m > l) {
                int iter = 0;
                do {
                    double g = d[l], p = (d[l + 1] - g) / (2.0 * e[l]), r = hyp(p, 1.0);
                    double dl1, h, c = 1.0, c2 = 1.0, c3 = 1.0, el1, s = 0.0, s2 = 0.0;
                    iter = iter + 1;
                    if (p < 0) r = -r;
                    d[l] = e[l] / (p + r);
                    d[l + 1] = e[l] * (p + r);
                    dl1 = d[l + 1];
                    h = g - d[l];
                    for (i = l + 2; i < N; ++i) d[i] -= h;
                    f = f + h;
                    p = d[m];
                    el1 = e[l + 1];
                    for (i = m - 1; i >= l; --i) {
                        c3 = c2;
                        c2 = c;
                        s2 = s;
                        g = c * e[i];
                        h = c * p;
                        r = hyp(p, e[i]);
                        e[i + 1] = s * r;
                        s = e[i] / r;
                        c = p / r;
                        p = c * d[i] - s * g;
                        d[i + 1] = h + s * (c * g + s * d[i]);
                        for (k = 0; k < N; ++k) {
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
    }
    for (i = 0; i < N - 1; ++i) {
        double p = d[i];
        k = i;
        for (j = i + 1; j < N; ++j) if (d[j] < p) { k = j; p = d[j]; }
        if (k != i) {
            d[k] = d[i];
            d[i] = p;
            for (j = 0; j < N; ++j) { p = V[j][i]; V[j][i] = V[j][k]; V[j][k] = p; }
        }
    }
}

double rs_largest_eigen(const double A[9], double vec[3])
{
    double d[N], V[N][N], best;
    int idx = 0, i;
    eig_sym(A, d, V);
    best = d[0];
    for (i = 1; i < N; ++i) if (fabs(d[i]) > fabs(best)) { best = d[i]; idx = i; }
    vec[0] = V[0][idx]; vec[1] = V[1][idx]; vec[2] = V[2][idx];
    return best;
}

void rs_eig_all(const double A[9], double d[3], double V[9])
{
    double W[N][N];
    eig_sym(A, d, W);
    memcpy(V, W, sizeof(W));
}

void rs_hessian_at(const float* img, const int64_t dim[3], const double* xyz, int64_t n, double* matrix9, double* vec3, double* val)
{
    acc_t a;
    a.img = img; memcpy(a.dim, dim, sizeof(a.dim));
    for (int64_t i = 0; i < n; ++i) {
        acc_set(&a, xyz + 3 * i);
        hessian(&a, matrix9 + 9 * i);
        val[i] = rs_largest_eigen(matrix9 + 9 * i, vec3 + 3 * i);
    }
}

/* Hessian.largestEigenVector without its Gauss3 blur: integer positions through the mirror */
void rs_hessian_images(const float* img, const int64_t dim[3], float* eigval, float* eigvec)
{
    acc_t a;
    const int64_t nvox = dim[0] * dim[1] * dim[2];
    a.img = img; memcpy(a.dim, dim, sizeof(a.dim));
    for (int64_t z = 0; z < dim[2]; ++z)
        for (int64_t y = 0; y < dim[1]; ++y)
            for (int64_t x = 0; x < dim[0]; ++x) {
                double m[9], v[3], ev;
                const double temp = 2 * tap(&a, x, y, z);
                const int64_t i = x + dim[0] * (y + dim[1] * z);
#define T(dx, dy, dz) ((double)tap(&a, x + (dx), y + (dy), z + (dz)))
                m[0] = T(1, 0, 0); m[0] -= temp; m[0] += T(-1, 0, 0);
                m[4] = T(0, 1, 0); m[4] -= temp; m[4] += T(0, -1, 0);
                m[8] = T(0, 0, 1); m[8] -= temp; m[8] += T(0, 0, -1);
                m[1] = m[3] = ((T(1, 1, 0) - T(-1, 1, 0)) / 2 - (T(1, -1, 0) - T(-1, -1, 0)) / 2) / 2;
                m[2] = m[6] = ((T(1, 0, 1) - T(-1, 0, 1)) / 2 - (T(1, 0, -1) - T(-1, 0, -1)) / 2) / 2;
                m[5] = m[7] = ((T(0, 1, 1) - T(0, -1, 1)) / 2 - (T(0, 1, -1) - T(0, -1, -1)) / 2) / 2;
#undef T
                ev = rs_largest_eigen(m, v);
                eigval[i] = (float)ev;
                eigvec[i] = (float)v[0];
                eigvec[i + nvox] = (float)v[1];
                eigvec[i + 2 * nvox] = (float)v[2];
            }
}

/* ---- Raytrace ---------------------------------------------------------------------------------------------------------- */
void rs_reflect(const double i[3], const double n[3], double r[3])
{
    const double dotP = i[0] * n[0] + i[1] * n[1] + i[2] * n[2];
    for (int d = 0; d < 3; ++d) r[d] = i[d] - 2 * dotP * n[d];
}
void rs_norm(double v[3])
{
    const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
}
double rs_incident_angle(const double i[3], double n[3])
{
    double thetaI = m_acos((n[0] * i[0] + n[1] * i[1] + n[2] * i[2]) /
                           (sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) * sqrt(i[0] * i[0] + i[1] * i[1] + i[2] * i[2])));
    if (thetaI >= HALF_PI) {
        n[0] *= -1; n[1] *= -1; n[2] *= -1;
        thetaI -= HALF_PI;
    }
    return thetaI;
}
double rs_refract(const double i[3], const double n[3], double n0, double n1, double thetaI, double t[3])
{
    const double deltaN = n0 / n1;
    const double thetaT = m_asin(deltaN * m_sin(thetaI));
    double cosThetaI, sinThetaT;
    if (thetaT != thetaT) return thetaT;
    cosThetaI = m_cos(thetaI);
    sinThetaT = m_sin(thetaT);
    for (int d = 0; d < 3; ++d) t[d] = deltaN * i[d] - n[d] * (deltaN * cosThetaI - sqrt(1 - sinThetaT * sinThetaT));
    return thetaT;
}

/* ---- Lightsheet -------------------------------------------------------------------------------------------------------- */
int rs_lightsheet_fit(double center, double thickness_center, double length, double thickness_edges, double abc[3])
{
    const double px[3] = {center, center - length / 2, center + length / 2};
    const double py[3] = {thickness_center, thickness_edges, thickness_edges};
    double m[9] = {0}, t[3] = {0}, inv[9], det;
    for (int k = 0; k < 3; ++k) {
        const double x = px[k], y = py[k], xx = x * x, xxx = xx * x;
        m[0] += xx * xx; m[1] += xxx; m[2] += xx;
        m[3] += xxx; m[4] += xx; m[5] += x;
        m[6] += xx; m[7] += x; m[8] += 1;
        t[0] += xx * y; t[1] += x * y; t[2] += y;
    }
    det = m[0] * m[4] * m[8] + m[3] * m[7] * m[2] + m[6] * m[1] * m[5] - m[2] * m[4] * m[6] - m[5] * m[7] * m[0] - m[8] * m[1] * m[3];
    if (det == 0) { abc[0] = abc[1] = abc[2] = 0; return -1; }
    inv[0] = (m[4] * m[8] - m[5] * m[7]) / det; inv[1] = (m[2] * m[7] - m[1] * m[8]) / det; inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    inv[3] = (m[5] * m[6] - m[3] * m[8]) / det; inv[4] = (m[0] * m[8] - m[2] * m[6]) / det; inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    inv[6] = (m[3] * m[7] - m[4] * m[6]) / det; inv[7] = (m[1] * m[6] - m[0] * m[7]) / det; inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    for (int r = 0; r < 3; ++r) abc[r] = inv[3 * r] * t[0] + inv[3 * r + 1] * t[1] + inv[3 * r + 2] * t[2];
    return 0;
}

/* ---- VolumeInjection --------------------------------------------------------------------------------------------------- */
static int diameter(double sigma)
{
    int s;
    if (!(sigma > 0)) return 3;
    s = 2 * (int)(3 * sigma + 0.5) + 1;
    return s > 3 ? s : 3;
}
static int64_t jround(double x)
{
    const double f = floor(x);
    return (int64_t)f + ((x - f) >= 0.5 ? 1 : 0);
}
static double gauss(double loc, int64_t cur, double tss)
{
    const double x = loc - (double)cur;
    return m_exp(-(x * x) / tss);
}
typedef struct { float *image, *weight; int64_t dim[3]; int size[3]; double tss[3]; double sum_weights; int num_pixels; } inj_t;

static void inj_init(inj_t* v, float* image, float* weight, const int64_t dim[3], const double sigma[3])
{
    v->image = image; v->weight = weight;
    memcpy(v->dim, dim, sizeof(v->dim));
    for (int d = 0; d < 3; ++d) {
        if (sigma[d] == 0) { v->size[d] = 1; v->tss[d] = 1; }
        else { v->size[d] = diameter(sigma[d]); v->tss[d] = 2 * sigma[d] * sigma[d]; }
    }
    v->sum_weights = 0; v->num_pixels = 0;
    {
        int64_t mn[3];
        for (int d = 0; d < 3; ++d) mn[d] = jround(0.0) - v->size[d] / 2;
        for (int64_t z = mn[2]; z < mn[2] + v->size[2]; ++z)
            for (int64_t y = mn[1]; y < mn[1] + v->size[1]; ++y)
                for (int64_t x = mn[0]; x < mn[0] + v->size[0]; ++x) {
                    double value = 1;
                    value *= gauss(0, x, v->tss[0]);
                    value *= gauss(0, y, v->tss[1]);
                    value *= gauss(0, z, v->tss[2]);
                    v->sum_weights += value;
                    ++v->num_pixels;
                }
    }
}
static void inj_add(inj_t* v, double intensity, const double loc[3])
{
    int64_t mn[3];
    for (int d = 0; d < 3; ++d) mn[d] = jround(loc[d]) - v->size[d] / 2;
    for (int64_t z = mn[2]; z < mn[2] + v->size[2]; ++z)
        for (int64_t y = mn[1]; y < mn[1] + v->size[1]; ++y)
            for (int64_t x = mn[0]; x < mn[0] + v->size[0]; ++x) {
                double value = 1;
                int64_t i;
                if (x < 0 || y < 0 || z < 0 || x >= v->dim[0] || y >= v->dim[1] || z >= v->dim[2]) continue;   /* extendZero */
                value *= gauss(loc[0], x, v->tss[0]);
                value *= gauss(loc[1], y, v->tss[1]);
                value *= gauss(loc[2], z, v->tss[2]);
                i = x + v->dim[0] * (y + v->dim[1] * z);
                v->image[i] = v->image[i] + (float)(value * intensity);
                v->weight[i] = v->weight[i] + (float)value;
            }
}

void rs_inject_info(const double sigma[3], int size[3], double* sum_weights, int* num_pixels)
{
    inj_t v;
    const int64_t dim[3] = {1, 1, 1};
    inj_init(&v, 0, 0, dim, sigma);
    memcpy(size, v.size, sizeof(v.size));
    *sum_weights = v.sum_weights;
    *num_pixels = v.num_pixels;
}

void rs_inject(float* image, float* weight, const int64_t dim[3], const double sigma[3], const double* xyz, const double* intensity,
               int64_t n, int normalized)
{
    inj_t v;
    inj_init(&v, image, weight, dim, sigma);
    for (int64_t i = 0; i < n; ++i) inj_add(&v, normalized ? intensity[i] / v.sum_weights : intensity[i], xyz + 3 * i);
}

void rs_normalize(const float* image, const float* weight, int64_t n, float* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = weight[i] > 1.0f ? image[i] / weight[i] : image[i];
}

void rs_project(const float* image, const float* weight, const int64_t dim[3], float* proj)
{
    for (int64_t y = 0; y < dim[1]; ++y)
        for (int64_t x = 0; x < dim[0]; ++x) {
            double sum = 0, count = 0;
            for (int64_t z = 0; z < dim[2]; ++z) {
                const int64_t i = x + dim[0] * (y + dim[1] * z);
                if (image[i] > 0) {
                    sum += image[i] * weight[i];          /* float product, as the reference's float * float */
                    count += weight[i];
                }
            }
            proj[x + dim[0] * y] = (float)(sum / count);
        }
}

/* ---- the tracers ------------------------------------------------------------------------------------------------------- */
static int inside(const double p[3], const int64_t dim[3])
{
    for (int d = 0; d < 3; ++d)
        if (p[d] < 0 || p[d] > (double)(dim[d] - 1)) return 0;
    return 1;
}
static uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001B3ULL; }

/* one move's refraction: updates the ray vector; *dec collects the decisions taken */
static void bend_ray(acc_t* ri, const double pos[3], double vec[3], double nA, double nB, uint64_t* dec)
{
    double m[9], ev3[3], ev;
    acc_set(ri, pos);
    hessian(ri, m);
    ev = rs_largest_eigen(m, ev3);
    *dec = mix(*dec, fabs(ev) > 0.01);
    if (fabs(ev) > 0.01) {
        double i0, i1, n0, n1, thetaI, thetaT, t[3];
        acc_set(ri, pos);
        acc_move(ri, -vec[0], 0); acc_move(ri, -vec[1], 1); acc_move(ri, -vec[2], 2);
        i0 = acc_get(ri);
        acc_move(ri, 2 * vec[0], 0); acc_move(ri, 2 * vec[1], 1); acc_move(ri, 2 * vec[2], 2);
        i1 = acc_get(ri);
        n0 = (nB - nA) * i0 + nA;
        n1 = (nB - nA) * i1 + nA;
        thetaI = m_acos((ev3[0] * vec[0] + ev3[1] * vec[1] + ev3[2] * vec[2]) /
                        (sqrt(ev3[0] * ev3[0] + ev3[1] * ev3[1] + ev3[2] * ev3[2]) * sqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2])));
        *dec = mix(*dec, 2 + (thetaI >= HALF_PI));
        if (thetaI >= HALF_PI) {
            ev3[0] *= -1; ev3[1] *= -1; ev3[2] *= -1;
            thetaI -= HALF_PI;
        }
        thetaT = rs_refract(vec, ev3, n0, n1, thetaI, t);
        *dec = mix(*dec, 4 + (thetaT != thetaT));
        if (thetaT != thetaT) { t[0] = vec[0]; t[1] = vec[1]; t[2] = vec[2]; }
        rs_norm(t);
        vec[0] = t[0]; vec[1] = t[1]; vec[2] = t[2];
    }
}

void rs_refract3d_ray_starts(uint64_t* rnd_state, const int64_t dim[3], int illum, int z, const double abc[3], int64_t n, double* pos3,
                             double* dir3)
{
    for (int64_t i = 0; i < n; ++i) {
        double* p = pos3 + 3 * i;
        double* v = dir3 + 3 * i;
        double th;
        p[0] = jr_double(rnd_state) * (double)(dim[0] - 1);
        p[1] = illum ? (int)dim[1] - 1 : 0;
        th = abc[0] * p[0] * p[0] + abc[1] * p[0] + abc[2];
        p[2] = z + (jr_double(rnd_state) * th) - th / 2.0;
        v[0] = (jr_double(rnd_state) - 0.5) / 5;
        v[1] = illum ? -1 : 1;
        v[2] = 0;
        rs_norm(v);
    }
}

/* refract3d (:261-401).  steps_xyz / steps_val / moves / decisions may be null; returns the number of steps.  inject = 0 traces only. */
int64_t rs_refract3d(const float* img, const float* ri_img, const int64_t dim[3], int illum, int z, double ls_middle, double ls_edge,
                     double ri, int64_t num_rays, uint64_t* rnd_state, float* image, float* weight, double* steps_xyz, float* steps_val,
                     int32_t* moves_out, uint64_t* decisions, int inject)
{
    acc_t aim, ari;
    inj_t inj;
    const double sigma[3] = {0.5, 0.5, 0.5};
    const double nA = 1.00, nB = ri;
    double abc[3];
    const int64_t max_moves = dim[2];
    int64_t nsteps = 0;
    aim.img = img; memcpy(aim.dim, dim, sizeof(aim.dim));
    ari.img = ri_img; memcpy(ari.dim, dim, sizeof(ari.dim));
    inj_init(&inj, image, weight, dim, sigma);
    if (rs_lightsheet_fit(dim[0] / 2.0, ls_middle, (double)dim[0], ls_edge, abc) != 0) return -1;
    for (int64_t i = 0; i < num_rays; ++i) {
        double pos[3], vec[3];
        int moves = 0;
        uint64_t dec = 0xCBF29CE484222325ULL;
        rs_refract3d_ray_starts(rnd_state, dim, illum, z, abc, 1, pos, vec);
        while (inside(pos, dim) && moves < max_moves) {
            float value;
            ++moves;
            acc_set(&aim, pos);
            value = acc_get(&aim);
            bend_ray(&ari, pos, vec, nA, nB, &dec);
            if (inject) inj_add(&inj, (double)value / inj.sum_weights, pos);
            for (int d = 0; d < 3; ++d) dec = mix(dec, (uint64_t)jround(pos[d]));
            if (steps_xyz) { steps_xyz[3 * nsteps] = pos[0]; steps_xyz[3 * nsteps + 1] = pos[1]; steps_xyz[3 * nsteps + 2] = pos[2]; }
            if (steps_val) steps_val[nsteps] = value;
            ++nsteps;
            pos[0] += vec[0]; pos[1] += vec[1]; pos[2] += vec[2];
        }
        if (moves_out) moves_out[i] = moves;
        if (decisions) decisions[i] = dec;
    }
    return nsteps;
}

void rs_camera_ray_starts(uint64_t* rnd_state, const int64_t dim[3], int rays_per_pixel, double* pos3)
{
    int64_t k = 0;
    for (int64_t y = 0; y < dim[1]; ++y)
        for (int64_t x = 0; x < dim[0]; ++x)
            for (int i = 0; i < rays_per_pixel; ++i, ++k) {
                pos3[3 * k] = (int)x + (jr_double(rnd_state) - 0.5);
                pos3[3 * k + 1] = (int)y + (jr_double(rnd_state) - 0.5);
                pos3[3 * k + 2] = 1;
            }
}

/* projectToCamera (:89-254); moves_out / decisions per ray (pixel-major), may be null */
void rs_project_to_camera(const float* ri_img, const float* refr, const int64_t dim[3], int current_z, int rays_per_pixel,
                          uint64_t* rnd_state, float* proj, int32_t* moves_out, uint64_t* decisions)
{
    acc_t ari, aref;
    const double nA = 1.00, nB = 1.01;
    const double sigma = 4.0, two_sq_sigma = 2 * sigma * sigma;
    const int64_t max_moves = dim[2];
    int64_t k = 0;
    ari.img = ri_img; memcpy(ari.dim, dim, sizeof(ari.dim));
    aref.img = refr; memcpy(aref.dim, dim, sizeof(aref.dim));
    for (int64_t y = 0; y < dim[1]; ++y)
        for (int64_t x = 0; x < dim[0]; ++x) {
            double avg = 0;
            for (int i = 0; i < rays_per_pixel; ++i, ++k) {
                double pos[3], vec[3] = {0, 0, 1}, signal = 0;
                int moves = 0;
                uint64_t dec = 0xCBF29CE484222325ULL;
                pos[0] = (int)x + (jr_double(rnd_state) - 0.5);
                pos[1] = (int)y + (jr_double(rnd_state) - 0.5);
                pos[2] = 1;
                while (inside(pos, dim) && moves < max_moves) {
                    double zo;
                    ++moves;
                    bend_ray(&ari, pos, vec, nA, nB, &dec);
                    acc_set(&aref, pos);
                    zo = fabs(pos[2] - current_z);
                    signal += acc_get(&aref) * m_exp(-(zo * zo) / two_sq_sigma);
                    pos[0] += vec[0]; pos[1] += vec[1]; pos[2] += vec[2];
                }
                avg += signal;
                if (moves_out) moves_out[k] = moves;
                if (decisions) decisions[k] = dec;
            }
            proj[x + dim[0] * y] = (float)(avg / 10.0);
        }
}
