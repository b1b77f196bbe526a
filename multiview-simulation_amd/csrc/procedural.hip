// The procedural phantom of HypersphereCollectionRealRandomAccessible.main (:199-286): a Perlin field
// (PerlinNoiseRealRandomAccessible), sets of spheres (HypersphereCollectionRealRandomAccessible) and rejection sampling against
// either (PointRejectionSampling).  Everything is fp64 on the vector units, one operation per rounding (the build compiles with
// -ffp-contract=off), so that a literal restatement on any IEEE machine gives the same bits.
//
//   Perlin   PerlinNoiseRealRandomAccess.get() (:127-160) operation by operation; the one deliberate difference is the smoothstep
//            weight, Math.pow(p, 3) * (10 - 15 p + 6 Math.pow(p, 2)) evaluated as (p p p) (10 - 15 p + 6 (p p)).  One lane per voxel,
//            x fastest; the gradient table and the permutation are staged in LDS once per block.
//   spheres  the value of the lowest-index sphere with sqrt(dx dx + dy dy + dz dz) <= radius, else the background.  The test is
//            made without a square root per voxel: sqrt is correctly rounded and monotone, so for every radius there is one largest
//            double T with sqrt(T) <= radius, found once per sphere (k_sph_prep), and sqrt(d) <= radius  <=>  d <= T.
//            The raster goes through the brick binner (bricks.h), culling with each sphere's own radius: every brick's list in
//            ascending sphere index, which one block per brick streams through LDS; a lane stops at its first containing sphere, the
//            block leaves the list once every lane has one.  Calls whose pairs exceed the option "beads_pair_cap" run in sphere
//            ranges; a bit mask of the voxels that earlier ranges own keeps a later range from replacing them.
//   sampler  one lane per trial: trial t starts at jr_jump(state, 8 t) (four nextDouble() of two steps each, accepted or not),
//            evaluates the density with the device functions of the `at` kernels, and a hipcub scan compacts the accepted trials in
//            trial order.
#include "bricks.h"
#include "jrandom.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace mvsim {

namespace {

constexpr int VPL = 8;                      // voxels per lane of the Perlin raster

struct SphRec {
    double c[3];
    double t;               // the largest d with sqrt(d) <= radius (NaN: never)
    float  v;
    int    pad;
};

struct Box3 {
    long long o[3];         // origin of the raster
    int       n[3];         // its extent
};

struct Interval3 {
    double mn[3], mx[3];
};

// ---- Perlin ------------------------------------------------------------------------------------------------------------------
// Math.min(1, Math.max(sstep, 0)) for the values that reach it (NaN stays NaN)
__device__ __forceinline__ double clamp01(double s)
{
    s = s > 0.0 ? s : (s != s ? s : 0.0);
    return s < 1.0 ? s : (s != s ? s : 1.0);
}

__device__ __forceinline__ double smoothstep(double a1, double a2, double p)
{
    const double s = clamp01((p * p * p) * (10.0 - 15.0 * p + 6.0 * (p * p)));      // :205-207, products for Math.pow
    return (1.0 - s) * a1 + s * a2;
}

// PerlinNoiseRealRandomAccess.get() (:127-160); grad (n x 3) and perm (n) in LDS
__device__ double perlin_value(const PerlinParams& P, const double* grad, const int* perm, const double pos[3])
{
    double pg[3];
    int pi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float a = (float)(pos[d] / P.scale[d]), b = (float)P.ext[d];
        float mod = fmodf(a, b);                                                      // fFloorMod (:248-252): Java's float %
        mod = mod < 0.0f ? mod + b : mod;
        pg[d] = (double)mod;
        pi[d] = pg[d] == pg[d] ? (int)floor(pg[d]) : 0;                               // (int) of NaN is 0 in Java
    }
    double dots[8], offs[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int off[3] = {i / 4, (i % 4) / 2, i % 2};                               // neighborOffsets (:230-245)
        double dist[3];
        int cp = 1, idx = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            int np = pi[d] + off[d];
            dist[d] = pg[d] - (double)np;                                             // before the wrap
            np = np % P.ext[d];
            idx += np * cp;                                                           // flatIndex (:218-228) as written
            cp += cp * P.ext[d];
        }
        if (i == 0) { offs[0] = dist[0]; offs[1] = dist[1]; offs[2] = dist[2]; }
        const double* g = grad + 3 * perm[idx % P.nvec];
        double dot = 0.0;
#pragma unroll
        for (int d = 0; d < 3; ++d) dot += g[d] * dist[d];
        dots[i] = dot;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) dots[i] = smoothstep(dots[2 * i], dots[2 * i + 1], offs[2]);      // interpolateSmoothstep (:184-201)
    dots[0] = smoothstep(dots[0], dots[1], offs[1]);
    dots[1] = smoothstep(dots[2], dots[3], offs[1]);
    return smoothstep(dots[0], dots[1], offs[0]);
}

// the field as its readers see it: the raw fp64 value, or -- SimpleCalculated's lambda (:221-223) over the FloatType the Perlin
// accessible stores its value in -- (float)value > threshold ? 1 : 0
__device__ __forceinline__ double perlin_field(const PerlinParams& P, const double* grad, const int* perm, const double pos[3])
{
    const double v = perlin_value(P, grad, perm, pos);
    if (P.threshold != P.threshold) return v;
    return (double)(float)v > P.threshold ? 1.0 : 0.0;
}

__device__ __forceinline__ void perlin_stage(const PerlinParams& P, const double* __restrict__ grad, const int* __restrict__ perm,
                                             double* s_grad, int* s_perm)
{
    for (int i = threadIdx.x; i < 3 * P.nvec; i += blockDim.x) s_grad[i] = grad[i];
    for (int i = threadIdx.x; i < P.nvec; i += blockDim.x) s_perm[i] = perm[i];
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_perlin_raster(PerlinParams P, const double* __restrict__ grad, const int* __restrict__ perm,
                                                       Box3 bx, float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_grad = s_dyn;
    int* s_perm = reinterpret_cast<int*>(s_dyn + 3 * P.nvec);
    perlin_stage(P, grad, perm, s_grad, s_perm);
    const long long n = (long long)bx.n[0] * bx.n[1] * bx.n[2];
    const long long first = (long long)blockIdx.x * (256 * VPL) + threadIdx.x;
    for (int k = 0; k < VPL; ++k) {
        const long long i = first + 256LL * k;
        if (i >= n) return;
        const long long yz = i / bx.n[0];
        const int x = (int)(i - yz * bx.n[0]);
        const long long z = yz / bx.n[1];
        const int y = (int)(yz - z * bx.n[1]);
        const double pos[3] = {(double)(bx.o[0] + x), (double)(bx.o[1] + y), (double)(bx.o[2] + z)};
        out[i] = (float)perlin_field(P, s_grad, s_perm, pos);
    }
}

__global__ __launch_bounds__(256) void k_perlin_at(PerlinParams P, const double* __restrict__ grad, const int* __restrict__ perm,
                                                   const double* __restrict__ xyz, long long n, double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_grad = s_dyn;
    int* s_perm = reinterpret_cast<int*>(s_dyn + 3 * P.nvec);
    perlin_stage(P, grad, perm, s_grad, s_perm);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double pos[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    out[i] = perlin_field(P, s_grad, s_perm, pos);
}

// ---- spheres -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double next_up(double t) { return __longlong_as_double(__double_as_longlong(t) + 1); }      // t >= +0, finite
__device__ __forceinline__ double next_down(double t) { return __longlong_as_double(__double_as_longlong(t) - 1); }   // t > +0

__global__ __launch_bounds__(256) void k_sph_prep(const double* __restrict__ centres, const double* __restrict__ radii,
                                                  const float* __restrict__ values, long long n, SphRec* __restrict__ recs)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double r = radii[i];                                 // >= 0, may be +inf (checked by the caller)
    double t = r * r;
    if (t < INFINITY || r < INFINITY) {
        if (!(t < INFINITY)) t = DBL_MAX;
        for (int k = 0; k < 8 && t > 0.0 && sqrt(t) > r; ++k) t = next_down(t);
        for (int k = 0; k < 8 && t < DBL_MAX && sqrt(next_up(t)) <= r; ++k) t = next_up(t);
    }
    SphRec s;
    s.c[0] = centres[3 * i]; s.c[1] = centres[3 * i + 1]; s.c[2] = centres[3 * i + 2];
    s.t = t;
    s.v = values[i];
    s.pad = 0;
    recs[i] = s;
}

// The bricks a sphere can reach: its box with one voxel to spare per side (the rounded distance of a voxel just outside the real
// box can still compare <= radius), clipped to the raster.  The host sizes the sphere ranges with the same function.
__host__ __device__ inline uint32_t sph_box(const double c[3], double r, const Box3& bx, int lo[3], int hi[3])
{
    for (int d = 0; d < 3; ++d) {
        double a = floor(c[d] - r) - 1.0 - (double)bx.o[d], b = ceil(c[d] + r) + 1.0 - (double)bx.o[d];
        a = a > 0.0 ? a : 0.0;
        b = b < (double)(bx.n[d] - 1) ? b : (double)(bx.n[d] - 1);
        if (!(a <= b)) { lo[d] = 1; hi[d] = 0; continue; }
        lo[d] = (int)a;
        hi[d] = (int)b;
    }
    return bricks_overlapped(lo, hi);
}

__global__ __launch_bounds__(256) void k_sph_cull(const double* __restrict__ centres, const double* __restrict__ radii, long long first,
                                                  long long count, Box3 bx, uint32_t* __restrict__ counts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double c[3] = {centres[3 * (first + i)], centres[3 * (first + i) + 1], centres[3 * (first + i) + 2]};
    int lo[3], hi[3];
    counts[i] = sph_box(c, radii[first + i], bx, lo, hi);
}

__global__ __launch_bounds__(256) void k_sph_emit(const double* __restrict__ centres, const double* __restrict__ radii, long long first,
                                                  long long count, Box3 bx, const uint32_t* __restrict__ counts,
                                                  const uint32_t* __restrict__ offs, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                  BrickGrid grid)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count || counts[i] == 0) return;
    const double c[3] = {centres[3 * (first + i)], centres[3 * (first + i) + 1], centres[3 * (first + i) + 2]};
    int lo[3], hi[3];
    sph_box(c, radii[first + i], bx, lo, hi);
    brick_emit(lo, hi, grid, 0u, (uint32_t)i, offs[i], keys, vals);      // the index within the range: ascending with the sphere index
}

// Math.max(float, float): NaN if either is NaN, +0 above -0
__device__ __forceinline__ float java_max_f(float a, float b)
{
    if (a != a) return a;
    if (a == 0.0f && b == 0.0f) return __float_as_uint(a) == 0u ? a : b;
    return a >= b ? a : b;                                     // b NaN: b
}

__global__ __launch_bounds__(256) void k_sph_render(const SphRec* __restrict__ recs, const uint32_t* __restrict__ vals,
                                                    const uint32_t* __restrict__ starts, float* __restrict__ out,
                                                    unsigned short* __restrict__ owned, Box3 bx, BrickGrid grid, float background,
                                                    int combine, int first_piece, int last_piece)
{
    __shared__ double s_c[CH][4];
    __shared__ float s_v[CH];

    const int nx = bx.n[0], ny = bx.n[1], nz = bx.n[2];
    const uint32_t brick = blockIdx.x;
    const BrickLane f = brick_lane(brick, grid, nx, ny);
    const int bzi = f.bzi, bz0 = f.bz0, x = f.x, y = f.y, tid = threadIdx.x;
    const bool inxy = f.inxy;
    const long long row = f.row, base = f.base;
    const long long oidx = inxy ? base + row * bzi : 0;        // the lane's word of the ownership mask
    const int nk = inxy ? min(BZ, nz - bz0) : 0;
    const uint32_t valid = (1u << nk) - 1u;
    const uint32_t have = (first_piece || !inxy) ? 0u : (uint32_t)owned[oidx];
    uint32_t found = have;
    float val[BZ];
#pragma unroll
    for (int k = 0; k < BZ; ++k) val[k] = background;
    const double px = (double)(bx.o[0] + x), py = (double)(bx.o[1] + y), pz0 = (double)(bx.o[2] + bz0);

    const uint32_t s = starts[brick], e = starts[brick + 1];
    for (uint32_t c0 = s; c0 < e; c0 += CH) {
        const int m = (int)min((uint32_t)CH, e - c0);
        if (tid < m) {
            const SphRec r = recs[vals[c0 + tid]];
            s_c[tid][0] = r.c[0]; s_c[tid][1] = r.c[1]; s_c[tid][2] = r.c[2]; s_c[tid][3] = r.t;
            s_v[tid] = r.v;
        }
        __syncthreads();
        if ((found & valid) != valid)
            for (int c = 0; c < m; ++c) {
                const double dx = px - s_c[c][0], dy = py - s_c[c][1], t = s_c[c][3];
                const double dxy = dx * dx + dy * dy;          // Util.distance: the squares summed x, y, z from 0.0
                if (!(dxy <= t)) continue;                     // adding dz dz never lowers the rounded sum
                const double cz = s_c[c][2];
                const float v = s_v[c];
#pragma unroll
                for (int k = 0; k < BZ; ++k) {
                    const double dz = (pz0 + (double)k) - cz;
                    if (!((found >> k) & 1u) && dxy + dz * dz <= t) { found |= 1u << k; val[k] = v; }
                }
            }
        if (__syncthreads_and((found & valid) == valid)) break;   // also the barrier in front of the next chunk's stores
    }
    if (!inxy) return;
    const uint32_t newly = found & ~have & valid;
#pragma unroll
    for (int k = 0; k < BZ; ++k) {
        if (k >= nk) break;
        const long long idx = base + row * (bz0 + k);
        if ((newly >> k) & 1u) out[idx] = combine ? java_max_f(out[idx], val[k]) : val[k];
        else if (last_piece && !((found >> k) & 1u)) {
            if (!combine) out[idx] = background;
            else {
                const float o = out[idx], mx = java_max_f(o, background);
                if (__float_as_uint(mx) != __float_as_uint(o)) out[idx] = mx;
            }
        }
    }
    if (!last_piece) owned[oidx] = (unsigned short)(found & valid);
}

// the value of the lowest-index sphere that contains the position, for every lane of the block at once: the set streams through
// LDS in chunks, a lane stops at its first sphere, the block at the chunk after which every lane has one
__device__ float spheres_first(const SphRec* __restrict__ recs, long long n, float background, const double pos[3], bool active)
{
    __shared__ double s_c[CH][4];
    __shared__ float s_v[CH];
    float v = background;
    bool found = !active;
    for (long long c0 = 0; c0 < n; c0 += CH) {
        const int m = (int)min((long long)CH, n - c0);
        if ((int)threadIdx.x < m) {
            const SphRec r = recs[c0 + threadIdx.x];
            s_c[threadIdx.x][0] = r.c[0]; s_c[threadIdx.x][1] = r.c[1]; s_c[threadIdx.x][2] = r.c[2]; s_c[threadIdx.x][3] = r.t;
            s_v[threadIdx.x] = r.v;
        }
        __syncthreads();
        if (!found)
            for (int c = 0; c < m; ++c) {
                const double dx = pos[0] - s_c[c][0], dy = pos[1] - s_c[c][1], dz = pos[2] - s_c[c][2];
                if ((dx * dx + dy * dy) + dz * dz <= s_c[c][3]) { v = s_v[c]; found = true; break; }
            }
        if (__syncthreads_and(found)) break;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_spheres_at(const SphRec* __restrict__ recs, long long nsph, float background,
                                                    const double* __restrict__ xyz, long long n, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool active = i < n;
    const double pos[3] = {active ? xyz[3 * i] : 0.0, active ? xyz[3 * i + 1] : 0.0, active ? xyz[3 * i + 2] : 0.0};
    const float v = spheres_first(recs, nsph, background, pos, active);
    if (active) out[i] = v;
}

// ---- rejection sampling ------------------------------------------------------------------------------------------------------
// PointRejectionSampling.sampleRealPoints (:42-53), trial t0 + i per lane.  The density is what RealType.getRealDouble() returns for
// the FloatType the accessibles hold: the float value, widened.
template <int KIND>
__global__ __launch_bounds__(256) void k_sample(uint64_t state, long long t0, int count, Interval3 iv, PerlinParams P,
                                                const double* __restrict__ grad, const int* __restrict__ perm,
                                                const SphRec* __restrict__ recs, long long nsph, float background,
                                                uint32_t* __restrict__ flags, double* __restrict__ pos_out)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_grad = s_dyn;
    int* s_perm = reinterpret_cast<int*>(s_dyn + 3 * P.nvec);
    if (KIND == 0) perlin_stage(P, grad, perm, s_grad, s_perm);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool active = i < count;
    JRandom r{jr_jump(state, 8ULL * (uint64_t)(t0 + (active ? i : 0)))};
    double pos[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) pos[d] = iv.mn[d] + r.next_double() * (iv.mx[d] - iv.mn[d]);
    const double p = r.next_double();
    double dens;
    if (KIND == 0) dens = (double)(float)perlin_field(P, s_grad, s_perm, pos);
    else dens = (double)spheres_first(recs, nsph, background, pos, active);
    if (!active) return;
    flags[i] = p < dens ? 1u : 0u;
    pos_out[3 * i] = pos[0]; pos_out[3 * i + 1] = pos[1]; pos_out[3 * i + 2] = pos[2];
}

// accepted trials to their slots, in trial order; res[0] = accepted in this batch, res[1] = the trial that filled the last slot
__global__ __launch_bounds__(256) void k_sample_compact(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                                                        const double* __restrict__ pos, int count, long long t0, long long have,
                                                        long long want, double* __restrict__ out, long long* __restrict__ res)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if (i == count - 1) res[0] = (long long)offs[i] + flags[i];
    if (!flags[i]) return;
    const long long slot = have + offs[i];
    if (slot >= want) return;
    out[3 * slot] = pos[3 * i]; out[3 * slot + 1] = pos[3 * i + 1]; out[3 * slot + 2] = pos[3 * i + 2];
    if (slot == want - 1) res[1] = t0 + i;
}

size_t perlin_lds(int nvec) { return (size_t)nvec * (3 * sizeof(double) + sizeof(int)); }

}  // namespace

int perlin_upload(mvsim_ctx* ctx, const mvsim_perlin* p, PerlinDev* dev)
{
    const size_t gb = (size_t)p->n_vectors * 3 * sizeof(double), pb = (size_t)p->n_vectors * sizeof(int32_t);
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));            // an earlier call's kernels may still read the tables
    MVSIM_TRY(ctx->proc_buf[0].reserve(gb + pb));
    MVSIM_HIP(hipMemcpy(ctx->proc_buf[0].p, p->gradients, gb, hipMemcpyHostToDevice));
    MVSIM_HIP(hipMemcpy((char*)ctx->proc_buf[0].p + gb, p->permutation, pb, hipMemcpyHostToDevice));
    for (int d = 0; d < 3; ++d) { dev->P.scale[d] = p->scales[d]; dev->P.ext[d] = p->loop_extents[d]; }
    dev->P.nvec = p->n_vectors;
    dev->P.threshold = p->threshold;
    dev->grad = ctx->proc_buf[0].as<double>();
    dev->perm = reinterpret_cast<const int32_t*>((char*)ctx->proc_buf[0].p + gb);
    return MVSIM_OK;
}

int perlin_at_dev(mvsim_ctx* ctx, const PerlinDev& pd, const double* xyz, int64_t n, double* out)
{
    if (n == 0) return MVSIM_OK;
    hipLaunchKernelGGL(k_perlin_at, dim3((unsigned)((n + 255) / 256)), dim3(256), perlin_lds(pd.P.nvec), ctx->stream, pd.P, pd.grad,
                       pd.perm, xyz, (long long)n, out);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int perlin_raster_dev(mvsim_ctx* ctx, const PerlinDev& pd, const int64_t origin[3], const int64_t dim[3], float* out)
{
    Box3 bx;
    for (int d = 0; d < 3; ++d) { bx.o[d] = origin[d]; bx.n[d] = (int)dim[d]; }
    const long long n = dim[0] * dim[1] * dim[2];
    hipLaunchKernelGGL(k_perlin_raster, dim3((unsigned)((n + 256 * VPL - 1) / (256 * VPL))), dim3(256), perlin_lds(pd.P.nvec), ctx->stream,
                       pd.P, pd.grad, pd.perm, bx, out);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int spheres_upload(mvsim_ctx* ctx, const mvsim_sphere_set* s, SpheresDev* dev)
{
    const size_t n = (size_t)s->n;
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    MVSIM_TRY(ctx->proc_buf[1].reserve(std::max<size_t>(16, n * (4 * sizeof(double) + sizeof(float)))));
    MVSIM_TRY(ctx->proc_buf[2].reserve(std::max<size_t>(16, n * sizeof(SphRec))));
    double* c = ctx->proc_buf[1].as<double>();
    double* r = c + 3 * n;
    float* v = reinterpret_cast<float*>(r + n);
    if (n > 0) {
        MVSIM_HIP(hipMemcpy(c, s->centres, n * 3 * sizeof(double), hipMemcpyHostToDevice));
        MVSIM_HIP(hipMemcpy(r, s->radii, n * sizeof(double), hipMemcpyHostToDevice));
        MVSIM_HIP(hipMemcpy(v, s->values, n * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_sph_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, c, r, v, (long long)n,
                           ctx->proc_buf[2].as<SphRec>());
        MVSIM_HIP(hipGetLastError());
    }
    dev->centres = c;
    dev->radii = r;
    dev->recs = ctx->proc_buf[2].p;
    dev->n = s->n;
    dev->background = s->background;
    return MVSIM_OK;
}

int spheres_at_dev(mvsim_ctx* ctx, const SpheresDev& sd, const double* xyz, int64_t n, float* out)
{
    if (n == 0) return MVSIM_OK;
    hipLaunchKernelGGL(k_spheres_at, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const SphRec*)sd.recs, (long long)sd.n,
                       sd.background, xyz, (long long)n, out);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int spheres_raster_dev(mvsim_ctx* ctx, const mvsim_sphere_set* s, const SpheresDev& sd, const int64_t origin[3], const int64_t dim[3],
                       int combine, float* out)
{
    Box3 bx;
    for (int d = 0; d < 3; ++d) { bx.o[d] = origin[d]; bx.n[d] = (int)dim[d]; }
    BrickGrid grid;
    MVSIM_TRY(brick_grid(dim, "sphere raster", &grid));
    // sphere ranges of at most `cap` pairs (one sphere alone may exceed it: it cannot be divided)
    const long long cap = ctx->opt.beads_pair_cap;
    std::vector<long long> first{0};
    long long pairs = 0, max_pairs = 0, max_count = 1;
    for (int64_t i = 0; i < s->n; ++i) {
        int lo[3], hi[3];
        const long long c = sph_box(s->centres + 3 * i, s->radii[i], bx, lo, hi);
        if (pairs > 0 && pairs + c > cap) {
            first.push_back(i);
            pairs = 0;
        }
        pairs += c;
        max_pairs = std::max(max_pairs, pairs);
    }
    first.push_back(s->n);
    const size_t npieces = first.size() - 1;
    for (size_t p = 0; p < npieces; ++p) max_count = std::max(max_count, first[p + 1] - first[p]);
    const long long max_slots = max_pairs + 1;
    BrickBins bins;
    MVSIM_TRY(bins.reserve(ctx->stream, max_count, max_slots, grid.nb, ctx->proc_buf[3], ctx->proc_buf[4], ctx->proc_buf[5], ctx->proc_buf[6],
                           "invalid argument: sphere raster: a range of %lld pairs"));
    unsigned short* owned = nullptr;
    if (npieces > 1) {
        MVSIM_TRY(ctx->proc_buf[7].reserve((size_t)(dim[0] * dim[1]) * (size_t)grid.nbz * sizeof(unsigned short)));
        owned = ctx->proc_buf[7].as<unsigned short>();
    }
    for (size_t p = 0; p < npieces; ++p) {
        const long long a = first[p], count = first[p + 1] - a;
        long long slots = 1;
        for (long long i = a; i < a + count; ++i) {
            int lo[3], hi[3];
            slots += sph_box(s->centres + 3 * i, s->radii[i], bx, lo, hi);
        }
        const dim3 gb((unsigned)((count + 255) / 256));
        if (count > 0) {
            hipLaunchKernelGGL(k_sph_cull, gb, dim3(256), 0, ctx->stream, sd.centres, sd.radii, a, count, bx, bins.counts);
            MVSIM_HIP(hipGetLastError());
            MVSIM_TRY(bins.scan(ctx->stream, count));
            hipLaunchKernelGGL(k_sph_emit, gb, dim3(256), 0, ctx->stream, sd.centres, sd.radii, a, count, bx, bins.counts, bins.offs, bins.keys[0],
                               bins.vals[0], grid);
            MVSIM_HIP(hipGetLastError());
        }
        MVSIM_TRY(bins.finish(ctx->stream, count, slots, grid.nb));
        hipLaunchKernelGGL(k_sph_render, dim3(grid.nb), dim3(256), 0, ctx->stream, (const SphRec*)sd.recs + a, bins.vals[1], bins.starts, out,
                           owned, bx, grid, sd.background, combine, p == 0 ? 1 : 0, p + 1 == npieces ? 1 : 0);
        MVSIM_HIP(hipGetLastError());
    }
    return MVSIM_OK;
}

int rejection_sample_dev(mvsim_ctx* ctx, uint64_t state, const double rmin[3], const double rmax[3], int64_t n_samples, const PerlinDev* pd,
                         const SpheresDev* sd, int64_t max_trials, double* xyz_out, int64_t* n_trials)
{
    *n_trials = 0;
    if (n_samples == 0) return MVSIM_OK;
    long long batch = ctx->opt.reject_batch;
    if (batch == 0) batch = std::min<long long>(1 << 20, std::max<long long>(4096, 4 * n_samples));
    size_t scan_tmp = 0;
    MVSIM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)batch, ctx->stream));
    MVSIM_TRY(ctx->proc_buf[6].reserve(std::max<size_t>(16, scan_tmp)));
    MVSIM_TRY(ctx->proc_buf[8].reserve((size_t)(2 * batch) * sizeof(uint32_t) + 2 * sizeof(long long)));
    MVSIM_TRY(ctx->proc_buf[9].reserve((size_t)(3 * batch + 3 * n_samples) * sizeof(double)));
    long long* res = ctx->proc_buf[8].as<long long>();                   // [accepted in the batch, trial of the last slot]
    uint32_t* flags = reinterpret_cast<uint32_t*>(res + 2);
    uint32_t* offs = flags + batch;
    double* pos = ctx->proc_buf[9].as<double>();
    double* out = pos + 3 * batch;
    Interval3 iv;
    for (int d = 0; d < 3; ++d) { iv.mn[d] = rmin[d]; iv.mx[d] = rmax[d]; }
    PerlinParams none = {};
    none.nvec = 0;
    long long have = 0, t0 = 0, host_res[2] = {0, -1};
    while (have < n_samples) {
        if (t0 >= max_trials) {
            set_error("invalid argument: rejection sampling: %lld of %lld samples after max_trials = %lld trials", have, (long long)n_samples,
                      (long long)max_trials);
            return MVSIM_EINVAL;
        }
        const int count = (int)std::min<long long>(batch, max_trials - t0);
        const dim3 grid((unsigned)((count + 255) / 256));
        if (pd)
            hipLaunchKernelGGL(k_sample<0>, grid, dim3(256), perlin_lds(pd->P.nvec), ctx->stream, state, t0, count, iv, pd->P, pd->grad, pd->perm,
                               (const SphRec*)nullptr, 0LL, 0.0f, flags, pos);
        else
            hipLaunchKernelGGL(k_sample<1>, grid, dim3(256), 0, ctx->stream, state, t0, count, iv, none, (const double*)nullptr,
                               (const int*)nullptr, (const SphRec*)sd->recs, (long long)sd->n, sd->background, flags, pos);
        MVSIM_HIP(hipGetLastError());
        size_t t = ctx->proc_buf[6].bytes;
        MVSIM_HIP(hipcub::DeviceScan::ExclusiveSum(ctx->proc_buf[6].p, t, flags, offs, count, ctx->stream));
        hipLaunchKernelGGL(k_sample_compact, grid, dim3(256), 0, ctx->stream, flags, offs, pos, count, t0, have, (long long)n_samples, out, res);
        MVSIM_HIP(hipGetLastError());
        MVSIM_HIP(hipMemcpyAsync(host_res, res, sizeof(host_res), hipMemcpyDeviceToHost, ctx->stream));
        MVSIM_HIP(hipStreamSynchronize(ctx->stream));
        have += host_res[0];
        t0 += count;
    }
    MVSIM_HIP(hipMemcpyAsync(xyz_out, out, (size_t)n_samples * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    *n_trials = host_res[1] + 1;
    return MVSIM_OK;
}

}  // namespace mvsim
