// The ray sandbox (raytracing/RayTracingTest.java) and the general tracer under it: rays whose starts and directions the CALLER
// supplies, refracted through an index volume by the same move as refract3d and projectToCamera (aberr_dev.h: refract_step), their
// steps injected as Gaussians by the same brick-sorted injection (aberrations.hip: aberr_inject_dev).
//
//   trace      one ray per lane, one wave per block, as k_refract3d_trace.  Per move the ray carries a value -- the interpolated sample
//              of an image volume, else its own intensity, else a constant --, takes refract_step with the caller's linear index map
//              n = (n_b - n_a) sample + n_a and eigenvalue threshold, and writes the step record at ray * max_moves + move.  Total
//              reflection is a policy (template parameter): keep the direction (every reference loop) or Raytrace.reflect (:32-40, the
//              line the reference has commented out).  max_moves is always finite: a ray that never leaves is counted, not waited for.
//   ranges     rays run in ranges whose slot buffer holds at most 2^25 step records (option "beads_pair_cap" lowers it); every range
//              compacts its records and continues the injection from what the previous one left.  StepRanges is that workspace and
//              tail, for this tracer and for refract3d (aberrations.hip).
//   starts     the sandbox's bundle (:110-123), every ray jumping the caller's java.util.Random ahead, and its grid (:334-344).
//   scene      Raytrace.drawSimpleImage (:96-128), the wedge.
#include "aberr_dev.h"
#include "common.h"
#include "jrandom.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace mvsim {

namespace {

struct TraceArgs {
    double n_a, n_b, ev_threshold;
    float  constant_value;
    int    max_moves, normalize_dirs;
};

template <bool REFLECT>
__global__ __launch_bounds__(64) void k_trace_rays(const float* __restrict__ img, const float* __restrict__ ri_img, int nx, int ny, int nz,
                                                   const double* __restrict__ pos3, const double* __restrict__ dir3,
                                                   const float* __restrict__ intensity, TraceArgs ta, int nrays,
                                                   double* __restrict__ slot_xyz, float* __restrict__ slot_val, int* __restrict__ moves_out,
                                                   double* __restrict__ end_pos3, double* __restrict__ end_dir3, int* __restrict__ n_capped)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= nrays) return;
    double pos[3] = {pos3[3 * (long long)r], pos3[3 * (long long)r + 1], pos3[3 * (long long)r + 2]};
    double vec[3] = {dir3[3 * (long long)r], dir3[3 * (long long)r + 1], dir3[3 * (long long)r + 2]};
    if (ta.normalize_dirs) norm3(vec);
    Accessor aim{img, nx, ny, nz, 0, 0, 0, 0, 0, 0}, ari{ri_img, nx, ny, nz, 0, 0, 0, 0, 0, 0};
    const float own = intensity ? intensity[r] : ta.constant_value;
    int moves = 0;
    const long long base = (long long)r * ta.max_moves;
    while (inside3(pos, nx, ny, nz) && moves < ta.max_moves) {
        float value = own;
        if (img) {
            aim.set(pos[0], pos[1], pos[2]);
            value = aim.get();
        }
        const double at[3] = {pos[0], pos[1], pos[2]};
        refract_step<REFLECT>(ari, pos, vec, ta.n_a, ta.n_b, ta.ev_threshold);
        double* q = slot_xyz + 3 * (base + moves);
        q[0] = at[0]; q[1] = at[1]; q[2] = at[2];
        slot_val[base + moves] = value;
        ++moves;
        pos[0] += vec[0]; pos[1] += vec[1]; pos[2] += vec[2];
    }
    moves_out[r] = moves;
    for (int d = 0; d < 3; ++d) {
        end_pos3[3 * (long long)r + d] = pos[d];
        end_dir3[3 * (long long)r + d] = vec[d];
    }
    if (inside3(pos, nx, ny, nz)) atomicAdd(n_capped, 1);      // still inside: max_moves ended it (an integer count: order-free)
}

// RayTracingTest.drawMultipleRays :110-123: ray n consumes draws 2n, 2n + 1 of nextDouble(), two generator steps each
__global__ __launch_bounds__(256) void k_sandbox_ray_starts(unsigned long long state, int x, int z, int ny, long long n,
                                                            double* __restrict__ pos3, double* __restrict__ dir3)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    JRandom rnd{jr_jump(state, 4ULL * (unsigned long long)i)};
    double v[3] = {0, -1, 0};
    norm3(v);
    pos3[3 * i] = (double)x + rnd.next_double() - 0.5;
    pos3[3 * i + 1] = (double)(ny - 1);
    pos3[3 * i + 2] = (double)z + rnd.next_double() - 0.5;
    dir3[3 * i] = v[0]; dir3[3 * i + 1] = v[1]; dir3[3 * i + 2] = v[2];
}

// RayTracingTest.drawRays :334-344: x = spacing, 2 spacing, .. <= Nx (x = Nx is a ray that is not inside), y = Ny - 25
__global__ __launch_bounds__(256) void k_grid_ray_starts(int spacing, int z, int ny, long long n, double* __restrict__ pos3,
                                                         double* __restrict__ dir3)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v[3] = {0, -1, 0};
    norm3(v);
    pos3[3 * i] = (double)((i + 1) * spacing);
    pos3[3 * i + 1] = (double)(ny - 25);
    pos3[3 * i + 2] = (double)z;
    dir3[3 * i] = v[0]; dir3[3 * i + 1] = v[1]; dir3[3 * i + 2] = v[2];
}

// Raytrace.drawSimpleImage :96-128
__global__ __launch_bounds__(256) void k_draw_simple_image(float* __restrict__ out, int nx, int ny, long long nvox, float low, float high)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % nx), y = (int)((i / nx) % ny);
        const bool all = x < nx / 2 ? x > y : nx - x > y;
        out[i] = all ? high : low;
    }
}

// the step list: slot records (ray * maxMoves + move) compacted in ray order, then move order
__global__ __launch_bounds__(256) void k_compact_steps(const double* __restrict__ slot_xyz, const float* __restrict__ slot_val,
                                                       const int* __restrict__ moves, const int* __restrict__ offs, int nrays, int max_moves,
                                                       double* __restrict__ xyz, float* __restrict__ val)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= (long long)nrays * max_moves) return;
    const int r = (int)(s / max_moves), mv = (int)(s - (long long)r * max_moves);
    if (mv >= moves[r]) return;
    const long long o = (long long)offs[r] + mv;
    xyz[3 * o] = slot_xyz[3 * s]; xyz[3 * o + 1] = slot_xyz[3 * s + 1]; xyz[3 * o + 2] = slot_xyz[3 * s + 2];
    val[o] = slot_val[s];
}

}  // namespace

// The step records one range of rays may fill (refract3d: max_moves = Nz, :304), at least one ray
int64_t trace_rays_per_range(int64_t pair_cap, int64_t max_moves)
{
    const int64_t cap_steps = std::max<int64_t>(max_moves, std::min<int64_t>(pair_cap / 8, (int64_t)1 << 25));
    return std::max<int64_t>(1, cap_steps / max_moves);
}

int StepRanges::reserve(mvsim_ctx* ctx, int64_t nrays, int max_moves_)
{
    max_moves = max_moves_;
    rays_per_range = trace_rays_per_range(ctx->opt.beads_pair_cap, max_moves);
    max_rays = std::min(std::max<int64_t>(nrays, 1), rays_per_range);
    const int64_t max_slots = max_rays * max_moves;
    size_t scan_tmp = 0;
    MVSIM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (int*)nullptr, (int*)nullptr, (int)max_rays, ctx->stream));
    MVSIM_TRY(ws.b[0].reserve((size_t)max_slots * 3 * sizeof(double)));
    MVSIM_TRY(ws.b[1].reserve((size_t)max_slots * sizeof(float)));
    MVSIM_TRY(ws.b[2].reserve((size_t)max_rays * 2 * sizeof(int)));
    MVSIM_TRY(ws.b[3].reserve((size_t)max_slots * 3 * sizeof(double)));
    MVSIM_TRY(ws.b[4].reserve((size_t)max_slots * sizeof(float)));
    MVSIM_TRY(ws.b[5].reserve(std::max<size_t>(16, scan_tmp)));
    slot_xyz = ws.b[0].as<double>();
    slot_val = ws.b[1].as<float>();
    moves = ws.b[2].as<int>();
    offs = moves + max_rays;
    xyz = ws.b[3].as<double>();
    val = ws.b[4].as<float>();
    return MVSIM_OK;
}

int StepRanges::finish(mvsim_ctx* ctx, const char* who, int64_t r0, int nr, const int64_t dim[3], const double sigma[3], double sumw, float* image,
                       float* weight, mvsim_ray_steps* steps)
{
    size_t t = ws.b[5].bytes;
    MVSIM_HIP(hipcub::DeviceScan::ExclusiveSum(ws.b[5].p, t, moves, offs, nr, ctx->stream));
    hipLaunchKernelGGL(k_compact_steps, dim3((unsigned)(((long long)nr * max_moves + 255) / 256)), dim3(256), 0, ctx->stream, slot_xyz,
                       slot_val, moves, offs, nr, max_moves, xyz, val);
    MVSIM_HIP(hipGetLastError());
    int last[2];
    MVSIM_HIP(hipMemcpyAsync(&last[0], moves + nr - 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipMemcpyAsync(&last[1], offs + nr - 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t nsteps = (int64_t)last[0] + last[1];
    if (steps) {
        if (steps->n + nsteps > steps->capacity) {
            set_error("invalid argument: %s: the step list needs more than its capacity of %lld steps", who, (long long)steps->capacity);
            return MVSIM_EINVAL;
        }
        if (steps->xyz) MVSIM_HIP(hipMemcpyAsync(steps->xyz + 3 * steps->n, xyz, (size_t)nsteps * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (steps->value) MVSIM_HIP(hipMemcpyAsync(steps->value + steps->n, val, (size_t)nsteps * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (steps->moves) MVSIM_HIP(hipMemcpyAsync(steps->moves + r0, moves, (size_t)nr * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        steps->n += nsteps;
    }
    if (image && weight) MVSIM_TRY(aberr_inject_dev(ctx, image, weight, dim, sigma, xyz, nullptr, val, nsteps, sumw));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

// Device volumes (img may be null); pos3, dir3, intensity (may be null) and every output list on the host.  image and weight are ADDED
// to.  end_pos3, end_dir3, n_capped and steps may be null.
int trace_rays_dev(mvsim_ctx* ctx, const float* ri_img, const float* img, const int64_t dim[3], const double* pos3, const double* dir3,
                   const float* intensity, int64_t n, const mvsim_trace_params* tp, double sumw, float* image, float* weight,
                   mvsim_ray_steps* steps, double* end_pos3, double* end_dir3, int64_t* n_capped)
{
    if (steps) steps->n = 0;
    if (n_capped) *n_capped = 0;
    if (n == 0) return MVSIM_OK;
    const int max_moves = (int)tp->max_moves;
    StepRanges sr;
    MVSIM_TRY(sr.reserve(ctx, n, max_moves));
    const int64_t max_rays = sr.max_rays;
    Scratch ws;
    MVSIM_TRY(ws.b[0].reserve((size_t)n * 6 * sizeof(double)));           // starts: [pos3][dir3] of every ray
    MVSIM_TRY(ws.b[1].reserve((size_t)max_rays * 6 * sizeof(double)));    // ends of one range
    if (intensity) MVSIM_TRY(ws.b[2].reserve((size_t)n * sizeof(float)));
    MVSIM_TRY(ws.b[3].reserve(sizeof(int)));
    double* d_pos = ws.b[0].as<double>();
    double* d_dir = d_pos + 3 * n;
    double* d_end = ws.b[1].as<double>();
    float* d_int = intensity ? ws.b[2].as<float>() : nullptr;
    int* capped = ws.b[3].as<int>();
    MVSIM_HIP(hipMemcpyAsync(d_pos, pos3, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MVSIM_HIP(hipMemcpyAsync(d_dir, dir3, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (intensity) MVSIM_HIP(hipMemcpyAsync(d_int, intensity, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    MVSIM_HIP(hipMemsetAsync(capped, 0, sizeof(int), ctx->stream));
    const TraceArgs ta{tp->n_a, tp->n_b, tp->ev_threshold, (float)tp->constant_value, max_moves, tp->normalize_dirs ? 1 : 0};
    const double sigma[3] = {tp->sigma[0], tp->sigma[1], tp->sigma[2]};

    for (int64_t r0 = 0; r0 < n; r0 += sr.rays_per_range) {
        const int nr = (int)std::min(sr.rays_per_range, n - r0);
        auto kernel = tp->total_reflection == MVSIM_TRACE_REFLECT ? k_trace_rays<true> : k_trace_rays<false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, ctx->stream, img, ri_img, (int)dim[0], (int)dim[1],
                           (int)dim[2], d_pos + 3 * r0, d_dir + 3 * r0, d_int ? d_int + r0 : nullptr, ta, nr, sr.slot_xyz, sr.slot_val, sr.moves,
                           d_end, d_end + 3 * max_rays, capped);
        MVSIM_HIP(hipGetLastError());
        if (end_pos3) MVSIM_HIP(hipMemcpyAsync(end_pos3 + 3 * r0, d_end, (size_t)nr * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (end_dir3) MVSIM_HIP(hipMemcpyAsync(end_dir3 + 3 * r0, d_end + 3 * max_rays, (size_t)nr * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MVSIM_TRY(sr.finish(ctx, "trace_rays", r0, nr, dim, sigma, sumw, image, weight, steps));
    }
    int nc = 0;
    MVSIM_HIP(hipMemcpyAsync(&nc, capped, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    if (n_capped) *n_capped = nc;
    return MVSIM_OK;
}

// bundle = 1: the sandbox's random bundle around (x, z) (state: the caller's java.util.Random); 0: the grid (x is the spacing).  Host outputs.
int trace_ray_starts(mvsim_ctx* ctx, int bundle, uint64_t state, const int64_t dim[3], int x, int z, int64_t n, double* pos3, double* dir3)
{
    if (n == 0) return MVSIM_OK;
    Scratch ws;
    MVSIM_TRY(ws.b[0].reserve((size_t)n * 6 * sizeof(double)));
    double* p = ws.b[0].as<double>();
    const dim3 grid((unsigned)((n + 255) / 256));
    if (bundle)
        hipLaunchKernelGGL(k_sandbox_ray_starts, grid, dim3(256), 0, ctx->stream, (unsigned long long)(state & JR_MASK), x, z, (int)dim[1],
                           (long long)n, p, p + 3 * n);
    else
        hipLaunchKernelGGL(k_grid_ray_starts, grid, dim3(256), 0, ctx->stream, x, z, (int)dim[1], (long long)n, p, p + 3 * n);
    MVSIM_HIP(hipGetLastError());
    MVSIM_HIP(hipMemcpyAsync(pos3, p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipMemcpyAsync(dir3, p + 3 * n, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

int draw_simple_image_dev(mvsim_ctx* ctx, float* out, const int64_t dim[3], float low, float high)
{
    const int64_t n = dim[0] * dim[1] * dim[2];
    hipLaunchKernelGGL(k_draw_simple_image, dim3((unsigned)std::min<int64_t>(8192, (n + 255) / 256)), dim3(256), 0, ctx->stream, out,
                       (int)dim[0], (int)dim[1], (long long)n, low, high);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
