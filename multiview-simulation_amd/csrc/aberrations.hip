// The refraction simulator (SimulateMultiViewAberrations.java): light-sheet rays refracted through a refractive-index volume and
// injected as Gaussians (refract3d, :261-401), camera rays summing the refracted volume (projectToCamera, :89-254), and the pieces
// they are made of (Hessian.java, raytracing/Raytrace.java, VolumeInjection.java).
//
//   ray step   one __device__ function for both tracers, with the reference's rounding points (the build compiles with
//              -ffp-contract=off): the n-linear sampler over a mirrored volume as an ACCESSOR that is moved -- an fp64 position plus
//              the integer position of its lower-corner tap; setPosition / move(distance) put the tap at floor(position), fwd / bck
//              move both by one, the weights are position - tap, so (p + 1) - 1 enters the weights as the reference computes it --,
//              the Hessian by the reference's literal sequence of moves (Hessian.java:155-278), the largest eigenpair by Householder
//              tridiagonalisation and implicit QL (EISPACK tred2 / tql2 as JAMA runs them for a symmetric matrix; + - * / sqrt only),
//              Snell refraction (Raytrace.java:42-93; acos, asin, sin, cos of the device library).
//   starts     ray i takes its draws of the caller's java.util.Random by jumping the 48-bit generator ahead (a^k and
//              c (a^k - 1) / (a - 1) mod 2^48 by squaring): ray starts are bit-exact whatever the launch shape.
//   refract3d  one ray per lane writes a step record (x, y, z, valueIm) per move at slot ray * maxMoves + move and its move count;
//              an exclusive scan over the counts compacts the records into the step LIST in ray order, then move order.
//   injection  VolumeInjection.addGaussian in list order into image and weight.  Float addition does not associate, so nothing is
//              scattered with atomics: the brick binner (bricks.h) gives every brick its steps in list order, and one block per
//              brick adds them, every voxel owned by one lane.  Lists whose pairs exceed the option "beads_pair_cap" run in ranges,
//              each continuing from the image and weight the previous one left: the same sequential sum.
//   shared     the device functions of the ray step and the starts live in aberr_dev.h; raytrace.hip traces caller-supplied rays
//              with them and owns the tail of a ray range (StepRanges: scan, compaction, step list, injection).
//   camera     one block per camera pixel, lanes over the pixel's rays; the per-ray fp64 signals go to LDS and ONE lane adds them in
//              ray order (avgValue, :242).
#include "aberr_dev.h"
#include "bricks.h"
#include "jrandom.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mvsim {

namespace {

__global__ __launch_bounds__(256) void k_ray_starts(SheetParams sp, int camera, int rays_per_pixel, int nx, int ny, long long n,
                                                    double* __restrict__ pos3, double* __restrict__ dir3)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double p[3], v[3];
    if (camera) {
        const long long pix = i / rays_per_pixel;
        camera_ray_start(sp.state, i, (int)(pix % nx), (int)(pix / nx), p, v);
    } else {
        sheet_ray_start(sp, i, nx, ny, p, v);
    }
    for (int d = 0; d < 3; ++d) {
        pos3[3 * i + d] = p[d];
        if (dir3) dir3[3 * i + d] = v[d];
    }
}

// ---- refract3d: trace -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_refract3d_trace(const float* __restrict__ img, const float* __restrict__ ri_img, int nx, int ny,
                                                        int nz, SheetParams sp, double nB, long long ray0, int nrays, int max_moves,
                                                        double* __restrict__ slot_xyz, float* __restrict__ slot_val,
                                                        int* __restrict__ moves_out)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= nrays) return;
    double pos[3], vec[3];
    sheet_ray_start(sp, ray0 + r, nx, ny, pos, vec);
    Accessor aim{img, nx, ny, nz, 0, 0, 0, 0, 0, 0}, ari{ri_img, nx, ny, nz, 0, 0, 0, 0, 0, 0};
    int moves = 0;
    const long long base = (long long)r * max_moves;
    while (inside3(pos, nx, ny, nz) && moves < max_moves) {
        aim.set(pos[0], pos[1], pos[2]);
        const float value = aim.get();
        const double at[3] = {pos[0], pos[1], pos[2]};
        refract_step(ari, pos, vec, 1.00, nB, 0.01);
        double* q = slot_xyz + 3 * (base + moves);
        q[0] = at[0]; q[1] = at[1]; q[2] = at[2];
        slot_val[base + moves] = value;
        ++moves;
        pos[0] += vec[0]; pos[1] += vec[1]; pos[2] += vec[2];
    }
    moves_out[r] = moves;
}

// ---- projectToCamera --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_project_to_camera(const float* __restrict__ ri_img, const float* __restrict__ refr, int nx, int ny,
                                                           int nz, int current_z, int rays_per_pixel, unsigned long long state,
                                                           float* __restrict__ proj)
{
    extern __shared__ double s_signal[];
    const int pix = blockIdx.x;
    const int px = pix % nx, py = pix / nx;
    const int max_moves = nz;
    const double two_sq_sigma = 2 * 4.0 * 4.0;
    Accessor ari{ri_img, nx, ny, nz, 0, 0, 0, 0, 0, 0}, aref{refr, nx, ny, nz, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < rays_per_pixel; i += 256) {
        double pos[3], vec[3], signal = 0.0;
        camera_ray_start(state, (long long)pix * rays_per_pixel + i, px, py, pos, vec);
        int moves = 0;
        while (inside3(pos, nx, ny, nz) && moves < max_moves) {
            ++moves;
            const double at[3] = {pos[0], pos[1], pos[2]};
            refract_step(ari, pos, vec, 1.00, 1.01, 0.01);                     // nB = 1.01 whatever ri is (:117)
            aref.set(at[0], at[1], at[2]);
            const double zo = fabs(at[2] - (double)current_z);
            signal += (double)aref.get() * exp(-(zo * zo) / two_sq_sigma);
            pos[0] += vec[0]; pos[1] += vec[1]; pos[2] += vec[2];
        }
        s_signal[i] = signal;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double avg = 0.0;
        for (int i = 0; i < rays_per_pixel; ++i) avg += s_signal[i];
        proj[pix] = (float)(avg / 10.0);
    }
}

// ---- Hessian at positions / over the image ----------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hessian_at(const float* __restrict__ img, int nx, int ny, int nz, const double* __restrict__ xyz,
                                                   long long n, double* __restrict__ matrix9, double* __restrict__ vec3,
                                                   double* __restrict__ val)
{
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Accessor a{img, nx, ny, nz, 0, 0, 0, 0, 0, 0};
    a.set(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    double m[6], v[3];
    hessian_by_moves(a, m);
    const double ev = largest_eigenpair(m, v);
    double* q = matrix9 + 9 * i;
    q[0] = m[0]; q[1] = m[3]; q[2] = m[4];
    q[3] = m[3]; q[4] = m[1]; q[5] = m[5];
    q[6] = m[4]; q[7] = m[5]; q[8] = m[2];
    vec3[3 * i] = v[0]; vec3[3 * i + 1] = v[1]; vec3[3 * i + 2] = v[2];
    val[i] = ev;
}

// Hessian.largestEigenVector (:69-99) without its blur: integer positions through the mirror, over `planes` planes from z0 on (the
// outputs hold those planes alone; eigvec may be null)
__global__ __launch_bounds__(64) void k_hessian_images(const float* __restrict__ img, int nx, int ny, int nz, int z0, int planes,
                                                       float* __restrict__ eigval, float* __restrict__ eigvec)
{
    const long long nvox = (long long)nx * ny * planes;
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= nvox) return;
    const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = z0 + (int)(i / ((long long)nx * ny));
    Accessor a{img, nx, ny, nz, 0, 0, 0, 0, 0, 0};
    const double temp = (double)(2 * a.tap(x, y, z));
    double m[6], v[3];
    m[0] = (double)a.tap(x + 1, y, z); m[0] -= temp; m[0] += (double)a.tap(x - 1, y, z);
    m[1] = (double)a.tap(x, y + 1, z); m[1] -= temp; m[1] += (double)a.tap(x, y - 1, z);
    m[2] = (double)a.tap(x, y, z + 1); m[2] -= temp; m[2] += (double)a.tap(x, y, z - 1);
    m[3] = (((double)a.tap(x + 1, y + 1, z) - (double)a.tap(x - 1, y + 1, z)) / 2 -
            ((double)a.tap(x + 1, y - 1, z) - (double)a.tap(x - 1, y - 1, z)) / 2) / 2;
    m[4] = (((double)a.tap(x + 1, y, z + 1) - (double)a.tap(x - 1, y, z + 1)) / 2 -
            ((double)a.tap(x + 1, y, z - 1) - (double)a.tap(x - 1, y, z - 1)) / 2) / 2;
    m[5] = (((double)a.tap(x, y + 1, z + 1) - (double)a.tap(x, y - 1, z + 1)) / 2 -
            ((double)a.tap(x, y + 1, z - 1) - (double)a.tap(x, y - 1, z - 1)) / 2) / 2;
    const double ev = largest_eigenpair(m, v);
    eigval[i] = (float)ev;
    if (!eigvec) return;
    eigvec[i] = (float)v[0];
    eigvec[i + nvox] = (float)v[1];
    eigvec[i + 2 * nvox] = (float)v[2];
}

// ---- VolumeInjection: normalize (:115-135), project (:199-232) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_volume_normalize(const float* __restrict__ image, const float* __restrict__ weight, long long n,
                                                          float* __restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float w = weight[i], v = image[i];
        out[i] = w > 1.0f ? v / w : v;
    }
}

__global__ __launch_bounds__(256) void k_volume_project(const float* __restrict__ image, const float* __restrict__ weight, int nx, int ny,
                                                        int nz, float* __restrict__ proj)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x, plane = (long long)nx * ny;
    if (p >= plane) return;
    double sum = 0.0, count = 0.0;
    for (int z = 0; z < nz; ++z) {
        const float v = image[p + plane * z], w = weight[p + plane * z];
        if (v > 0) {
            sum += (double)(v * w);       // float * float, widened afterwards (:223)
            count += (double)w;
        }
    }
    proj[p] = (float)(sum / count);       // an empty column: 0 / 0 = NaN, as the reference
}

// ---- VolumeInjection.addGaussian (:175-197) in list order -------------------------------------------------------------------
struct InjRec {
    double loc[3];
    double inten;
    int    lo[3], hi[3];    // box clipped to the image, inclusive
};

__global__ __launch_bounds__(256) void k_inject_cull(const double* __restrict__ xyz, const double* __restrict__ inten, const float* __restrict__ val,
                                                     double sumw, long long n, InjRec* __restrict__ recs, uint32_t* __restrict__ counts, int nx,
                                                     int ny, int nz, int s0, int s1, int s2)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int dim[3] = {nx, ny, nz}, size[3] = {s0, s1, s2};
    InjRec r;
    double v = val ? (double)val[i] : inten[i];
    if (sumw != 0.0) v = v / sumw;                               // addNormalizedGaussian (:168-173)
    r.inten = v;
    for (int d = 0; d < 3; ++d) {
        const double p = xyz[3 * i + d];
        r.loc[d] = p;
        r.lo[d] = 1; r.hi[d] = 0;
        if (!(fabs(p) < 1.0e9)) continue;                        // nowhere near the image (or NaN): every write is dropped
        const long long lo = java_round_d(p) - size[d] / 2;      // getCursor (:147-160)
        const long long hi = lo + size[d] - 1;
        r.lo[d] = (int)(lo < 0 ? 0 : lo);
        r.hi[d] = (int)(hi > dim[d] - 1 ? dim[d] - 1 : hi);
    }
    const uint32_t cnt = bricks_overlapped(r.lo, r.hi);
    if (cnt == 0) { r.lo[0] = 1; r.hi[0] = 0; }
    recs[i] = r;
    counts[i] = cnt;
}

__global__ __launch_bounds__(256) void k_inject_emit(const InjRec* __restrict__ recs, const uint32_t* __restrict__ counts,
                                                     const uint32_t* __restrict__ offs, long long n, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ vals, BrickGrid grid)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || counts[i] == 0) return;
    const InjRec r = recs[i];
    brick_emit(r.lo, r.hi, grid, 0u, (uint32_t)i, offs[i], keys, vals);
}

// one block per brick: image and weight of its voxels continue from what they hold, step after step in list order
__global__ __launch_bounds__(256) void k_inject_render(const InjRec* __restrict__ recs, const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ starts, float* __restrict__ image, float* __restrict__ weight,
                                                       int nx, int ny, int nz, BrickGrid grid, double t0, double t1, double t2)
{
    __shared__ double s_tab[CH][NTAB];
    __shared__ double s_loc[CH][3], s_int[CH];
    __shared__ int s_lo[CH][3], s_hi[CH][3];

    const uint32_t brick = blockIdx.x;
    const uint32_t s = starts[brick], e = starts[brick + 1];
    if (s == e) return;                                 // nothing lands here: the voxels stay as they are
    const BrickLane f = brick_lane(brick, grid, nx, ny);
    const int bz0 = f.bz0, xl = f.xl, yl = f.yl, x = f.x, y = f.y, tid = threadIdx.x;
    const bool inxy = f.inxy;
    const long long row = f.row, base = f.base;

    float acc_i[BZ], acc_w[BZ];
#pragma unroll
    for (int k = 0; k < BZ; ++k) {
        const int z = bz0 + k;
        const bool in = inxy && z < nz;
        acc_i[k] = in ? image[base + row * z] : 0.0f;
        acc_w[k] = in ? weight[base + row * z] : 0.0f;
    }
    const double tss[3] = {t0, t1, t2};
    for (uint32_t c0 = s; c0 < e; c0 += CH) {
        const int m = (int)min((uint32_t)CH, e - c0);
        __syncthreads();                                // the previous chunk's tables have been read
        if (tid < m) {
            const InjRec r = recs[vals[c0 + tid]];
            for (int d = 0; d < 3; ++d) { s_loc[tid][d] = r.loc[d]; s_lo[tid][d] = r.lo[d]; s_hi[tid][d] = r.hi[d]; }
            s_int[tid] = r.inten;
        }
        __syncthreads();
        brick_fill_tables(m, f, tss, s_tab, s_loc, s_lo, s_hi);      // getGaussValue (:162-166)
        __syncthreads();
        for (int c = 0; c < m; ++c) {
            if (x < s_lo[c][0] || x > s_hi[c][0] || y < s_lo[c][1] || y > s_hi[c][1]) continue;
            const int zl = s_lo[c][2] - bz0, zh = s_hi[c][2] - bz0;
            const double exy = (1 * s_tab[c][xl]) * s_tab[c][BX + yl];
            const double inten = s_int[c];
#pragma unroll
            for (int k = 0; k < BZ; ++k)
                if (k >= zl && k <= zh) {
                    const double value = exy * s_tab[c][BX + BY + k];
                    acc_i[k] = acc_i[k] + (float)(value * inten);        // :194
                    acc_w[k] = acc_w[k] + (float)value;                  // :195
                }
        }
    }
    if (!inxy) return;
#pragma unroll
    for (int k = 0; k < BZ; ++k) {
        const int z = bz0 + k;
        if (z >= nz) break;
        image[base + row * z] = acc_i[k];
        weight[base + row * z] = acc_w[k];
    }
}

}  // namespace

// VolumeInjection's constructor (:56-72) for sigma > 0
void aberr_inject_geometry(const double sigma[3], int size[3], double tss[3])
{
    for (int d = 0; d < 3; ++d) {
        size[d] = suggested_kernel_diameter(sigma[d]);
        tss[d] = 2 * sigma[d] * sigma[d];
    }
}

// xyz (3 doubles per step) with either inten (doubles) or val (floats), all on the device; sumw != 0 divides every intensity by it
int aberr_inject_dev(mvsim_ctx* ctx, float* image, float* weight, const int64_t dim[3], const double sigma[3], const double* xyz,
                     const double* inten, const float* val, int64_t n, double sumw)
{
    if (n == 0) return MVSIM_OK;
    int size[3];
    double tss[3];
    aberr_inject_geometry(sigma, size, tss);
    BrickGrid grid;
    MVSIM_TRY(brick_grid(dim, "volume injection", &grid));
    const int64_t per_item = bricks_spanned(size, dim, grid);
    const int64_t cap = ctx->opt.beads_pair_cap;
    const int64_t per_range = std::max<int64_t>(1, std::min<int64_t>(cap / per_item, ((int64_t)1 << 31) / per_item - 1));
    const int64_t max_items = std::min(n, per_range), max_slots = max_items * per_item + 1;

    Scratch ws;
    BrickBins bins;                              // per_range keeps a range's slots below 2^31: the refusal is never reached
    MVSIM_TRY(bins.reserve(ctx->stream, max_items, max_slots, grid.nb, ws.b[1], ws.b[2], ws.b[3], ws.b[4],
                           "invalid argument: volume injection: a range of %lld pairs"));
    MVSIM_TRY(ws.b[0].reserve((size_t)max_items * sizeof(InjRec)));
    InjRec* recs = ws.b[0].as<InjRec>();

    for (int64_t first = 0; first < n; first += per_range) {
        const int64_t cnt = std::min(per_range, n - first), slots = cnt * per_item + 1;
        const unsigned blocks = (unsigned)((cnt + 255) / 256);
        hipLaunchKernelGGL(k_inject_cull, dim3(blocks), dim3(256), 0, ctx->stream, xyz + 3 * first, inten ? inten + first : nullptr,
                           val ? val + first : nullptr, sumw, (long long)cnt, recs, bins.counts, (int)dim[0], (int)dim[1], (int)dim[2], size[0],
                           size[1], size[2]);
        MVSIM_HIP(hipGetLastError());
        MVSIM_TRY(bins.scan(ctx->stream, cnt));
        hipLaunchKernelGGL(k_inject_emit, dim3(blocks), dim3(256), 0, ctx->stream, recs, bins.counts, bins.offs, (long long)cnt, bins.keys[0],
                           bins.vals[0], grid);
        MVSIM_HIP(hipGetLastError());
        MVSIM_TRY(bins.finish(ctx->stream, cnt, slots, grid.nb));
        hipLaunchKernelGGL(k_inject_render, dim3(grid.nb), dim3(256), 0, ctx->stream, recs, bins.vals[1], bins.starts, image, weight,
                           (int)dim[0], (int)dim[1], (int)dim[2], grid, tss[0], tss[1], tss[2]);
        MVSIM_HIP(hipGetLastError());
    }
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));          // the workspaces go away with this call
    return MVSIM_OK;
}

// refract3d on device volumes; image and weight are ADDED to (the caller zeroes them for the reference's result).  steps: host buffers
// or null.  Rays run in ranges whose step records and pairs fit the option "beads_pair_cap".
int aberr_refract3d_dev(mvsim_ctx* ctx, const float* img, const float* ri_img, const int64_t dim[3], int illum, int z, const double abc[3],
                        double ri, int64_t num_rays, uint64_t state, float* image, float* weight, double sumw, mvsim_ray_steps* steps)
{
    const double sigma[3] = {0.5, 0.5, 0.5};                                                       // :280
    const int max_moves = (int)dim[2];                                                            // :304
    if (steps) steps->n = 0;
    StepRanges sr;
    MVSIM_TRY(sr.reserve(ctx, num_rays, max_moves));
    SheetParams sp{state & JR_MASK, abc[0], abc[1], abc[2], illum ? 1 : 0, z};

    for (int64_t r0 = 0; r0 < num_rays; r0 += sr.rays_per_range) {
        const int nr = (int)std::min(sr.rays_per_range, num_rays - r0);
        hipLaunchKernelGGL(k_refract3d_trace, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, ctx->stream, img, ri_img, (int)dim[0], (int)dim[1],
                           (int)dim[2], sp, ri, (long long)r0, nr, max_moves, sr.slot_xyz, sr.slot_val, sr.moves);
        MVSIM_HIP(hipGetLastError());
        MVSIM_TRY(sr.finish(ctx, "refract3d", r0, nr, dim, sigma, sumw, image, weight, steps));
    }
    return MVSIM_OK;
}

int aberr_project_to_camera_dev(mvsim_ctx* ctx, const float* ri_img, const float* refr, const int64_t dim[3], int current_z,
                                int rays_per_pixel, uint64_t state, float* proj)
{
    const size_t lds = (size_t)rays_per_pixel * sizeof(double);
    hipLaunchKernelGGL(k_project_to_camera, dim3((unsigned)(dim[0] * dim[1])), dim3(256), lds, ctx->stream, ri_img, refr, (int)dim[0],
                       (int)dim[1], (int)dim[2], current_z, rays_per_pixel, (unsigned long long)(state & JR_MASK), proj);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// camera = 0: refract3d's starts (pos3 and dir3); 1: projectToCamera's (pos3; dir3 may be null).  Host outputs.
int aberr_ray_starts(mvsim_ctx* ctx, uint64_t state, const int64_t dim[3], int camera, int illum, int z, const double abc[3],
                     int rays_per_pixel, int64_t n, double* pos3, double* dir3)
{
    if (n == 0) return MVSIM_OK;
    Scratch ws;
    MVSIM_TRY(ws.b[0].reserve((size_t)n * 3 * sizeof(double)));
    if (dir3) MVSIM_TRY(ws.b[1].reserve((size_t)n * 3 * sizeof(double)));
    SheetParams sp{state & JR_MASK, abc ? abc[0] : 0.0, abc ? abc[1] : 0.0, abc ? abc[2] : 0.0, illum ? 1 : 0, z};
    hipLaunchKernelGGL(k_ray_starts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, sp, camera, rays_per_pixel, (int)dim[0],
                       (int)dim[1], (long long)n, ws.b[0].as<double>(), dir3 ? ws.b[1].as<double>() : nullptr);
    MVSIM_HIP(hipGetLastError());
    MVSIM_HIP(hipMemcpyAsync(pos3, ws.b[0].p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (dir3) MVSIM_HIP(hipMemcpyAsync(dir3, ws.b[1].p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

// img on the device; positions and results on the host
int aberr_hessian_at_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const double* xyz, int64_t n, double* matrix9, double* eigvec3,
                         double* eigval)
{
    if (n == 0) return MVSIM_OK;
    Scratch ws;
    MVSIM_TRY(ws.b[0].reserve((size_t)n * 3 * sizeof(double)));
    MVSIM_TRY(ws.b[1].reserve((size_t)n * 13 * sizeof(double)));
    double* out = ws.b[1].as<double>();
    MVSIM_HIP(hipMemcpyAsync(ws.b[0].p, xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_hessian_at, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, img, (int)dim[0], (int)dim[1], (int)dim[2],
                       ws.b[0].as<double>(), (long long)n, out, out + 9 * n, out + 12 * n);
    MVSIM_HIP(hipGetLastError());
    if (matrix9) MVSIM_HIP(hipMemcpyAsync(matrix9, out, (size_t)n * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (eigvec3) MVSIM_HIP(hipMemcpyAsync(eigvec3, out + 9 * n, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (eigval) MVSIM_HIP(hipMemcpyAsync(eigval, out + 12 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

// planes z0 .. z0 + planes - 1 of the Hessian images into outputs of `planes` planes (eigvec: 3 x planes, may be null)
int aberr_hessian_images_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], int z0, int planes, float* eigval, float* eigvec)
{
    const int64_t n = dim[0] * dim[1] * planes;
    hipLaunchKernelGGL(k_hessian_images, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, img, (int)dim[0], (int)dim[1], (int)dim[2],
                       z0, planes, eigval, eigvec);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int aberr_normalize_dev(mvsim_ctx* ctx, const float* image, const float* weight, int64_t n, float* out)
{
    hipLaunchKernelGGL(k_volume_normalize, dim3((unsigned)std::min<int64_t>(8192, (n + 255) / 256)), dim3(256), 0, ctx->stream, image, weight,
                       (long long)n, out);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int aberr_project_dev(mvsim_ctx* ctx, const float* image, const float* weight, const int64_t dim[3], float* proj)
{
    hipLaunchKernelGGL(k_volume_project, dim3((unsigned)((dim[0] * dim[1] + 255) / 256)), dim3(256), 0, ctx->stream, image, weight,
                       (int)dim[0], (int)dim[1], (int)dim[2], proj);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
