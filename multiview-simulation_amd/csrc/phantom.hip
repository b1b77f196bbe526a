// Ground-truth phantom of SimulateMultiViewDataset (SimulateMultiViewDataset.java:366-522): the step in front of
// the per-view path.
//
//   drawSpheres   :436-522  walk the voxels of one large sphere; per voxel draw radius = rnd.nextInt(10*scale)+1 and
//                           a double; one voxel in (7*scale)^3 (by a rounding test on that double) becomes the centre
//                           of a small sphere whose voxels are max-composited with a second random intensity.
//   downSample2x  :394-424  n-linear samples at 2l + 0.5 (all eight weights 1/8), dims N/2 - 1.
//
// Split between host and GPU.  The random stream is ONE sequential java.util.Random shared by all voxels of the large
// sphere (3 LCG steps per voxel, 5 where a sphere is drawn), so the walk that decides which voxels become centres
// is replayed on the host (~0.1 s for the reference's 580^3 canvas: 31 M voxels) in the HyperSphereCursor's raster
// order; what it produces is a list of (centre, radius, value).  Math.max makes the compositing order-free, so the
// ~11 000 spheres (~10^8 voxel updates) are splatted on the GPU with one atomic max per voxel, and the 2x
// down-sampling is a streaming kernel.  Option sphere_walk = device resolves the same walk on the GPU instead (sphere_walk.h,
// sphere_walk.hip: 1.6 ms against 90 ms at 580^3); multiSpheres of the refraction simulator (below) does so by default.
//
// Sphere geometry (ImgLib2 HyperSphereCursor, restated from the published algorithm): z in [cz-R, cz+R],
// r1 = floor(sqrt(R^2 - dz^2)), y in [cy-r1, cy+r1], r0 = floor(sqrt(r1^2 - dy^2)), x in [cx-r0, cx+r0]
// (nested truncated radii, x fastest).  (long)Math.sqrt of an exact integer equals the integer floor square root,
// which is what isqrt() computes without floating-point rounding questions.
#include "common.h"
#include "jrandom.h"

#include <cmath>
#include <vector>

namespace mvsim {

namespace {

inline int64_t isqrt_host(int64_t v)
{
    int64_t r = (int64_t)std::sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

}  // namespace

// device-side item = the C ABI's mvsim_sphere (centre, radius, value)
struct SphereItem {
    int cx, cy, cz, r;
    float v;
};
static_assert(sizeof(SphereItem) == sizeof(mvsim_sphere), "SphereItem must mirror mvsim_sphere");

__device__ __forceinline__ int isqrt_dev(int v)
{
    int r = (int)sqrtf((float)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// max-composite that is valid for any mix of signs (integer order of IEEE floats)
__device__ __forceinline__ void atomic_max_float(float* p, float v)
{
    if (v >= 0.f) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned int*>(p), __float_as_uint(v));
}

// one block per (sphere, z slice of the sphere); lanes over the (2r+1)^2 candidates of the slice
__global__ __launch_bounds__(256) void k_splat_spheres(float* __restrict__ img, int nx, int ny, int nz,
                                                       const SphereItem* __restrict__ items)
{
    const SphereItem it = items[blockIdx.x];
    const int dz = (int)blockIdx.y - it.r;
    if (dz > it.r) return;
    const int r1 = isqrt_dev(it.r * it.r - dz * dz);
    const int w = 2 * r1 + 1;
    const int z = it.cz + dz;
    if (z < 0 || z >= nz) return;
    for (int e = threadIdx.x; e < w * w; e += 256) {
        const int dy = e / w - r1, dx = e % w - r1;
        const int r0 = isqrt_dev(r1 * r1 - dy * dy);
        if (dx < -r0 || dx > r0) continue;
        const int x = it.cx + dx, y = it.cy + dy;
        if (x < 0 || x >= nx || y < 0 || y >= ny) continue;      // validated on the host; belt and braces
        atomic_max_float(img + (x + (long long)nx * (y + (long long)ny * z)), it.v);
    }
}

// SMVD:394-424.  All eight n-linear weights are 0.5^3: each tap (float)(v * 0.125), float accumulation in the
// interpolator's Gray-code order 000,100,110,010,011,111,101,001 (x is the first digit).
__global__ __launch_bounds__(256) void k_downsample2x(const float* __restrict__ in, float* __restrict__ out, int nx,
                                                      int ny, int ox, int oy, int oz)
{
    const long long total = (long long)ox * oy * oz;
    const long long nthreads = (long long)gridDim.x * 256;
    const long long row = nx, plane = (long long)nx * ny;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += nthreads) {
        const int x = (int)(o % ox);
        const long long t = o / ox;
        const int y = (int)(t % oy), z = (int)(t / oy);
        const float* p = in + 2 * x + row * (2 * y) + plane * (2 * z);
        const double w = 0.5 * 0.5 * 0.5;
        float acc = (float)((double)p[0] * w);
        acc += (float)((double)p[1] * w);
        acc += (float)((double)p[1 + row] * w);
        acc += (float)((double)p[row] * w);
        acc += (float)((double)p[row + plane] * w);
        acc += (float)((double)p[1 + row + plane] * w);
        acc += (float)((double)p[1 + plane] * w);
        acc += (float)((double)p[plane] * w);
        out[o] = acc;
    }
}

int launch_downsample2x(hipStream_t s, const float* in, const int64_t dim[3], float* out)
{
    const int ox = (int)(dim[0] / 2 - 1), oy = (int)(dim[1] / 2 - 1), oz = (int)(dim[2] / 2 - 1);
    const long long total = (long long)ox * oy * oz;
    long long want = (total + 255) / 256;
    const int blocks = (int)(want < 1 ? 1 : (want > 16384 ? 16384 : want));
    hipLaunchKernelGGL(k_downsample2x, dim3(blocks), dim3(256), 0, s, in, out, (int)dim[0], (int)dim[1], ox, oy, oz);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

namespace {

// voxels of the large sphere of radius R (HyperSphereCursor geometry)
int64_t sphere_voxels(int64_t R)
{
    int64_t n = 0;
    for (int64_t dz = -R; dz <= R; ++dz) {
        const int64_t r1 = isqrt_host(R * R - dz * dz);
        for (int64_t dy = -r1; dy <= r1; ++dy) n += 2 * isqrt_host(r1 * r1 - dy * dy) + 1;
    }
    return n;
}

// The accepted voxels of the walk over the n voxels of the large sphere, in visit order: on the device where the context asks for it
// and the device walk vouches for the case, else the serial walk (sphere_walk = device_only: an error instead, so that a test can tell
// the two apart).  *state: the generator, advanced on success.
int walk_entries(mvsim_ctx* ctx, bool on_device, int64_t n, const WalkRule& rule, uint64_t* state, std::vector<WalkEntry>* entries)
{
    if (on_device) {
        bool done = false;
        uint64_t end_state = *state;
        MVSIM_TRY(sphere_walk_dev(ctx, *state, n, rule, entries, &end_state, &done));
        if (done) { *state = end_state; return MVSIM_OK; }
        if (ctx->opt.sphere_walk == 2) {
            set_error("sphere_walk=device_only: the device walk does not vouch for this case (%lld voxels)", (long long)n);
            return MVSIM_EINVAL;
        }
    }
    entries->clear();
    uint64_t s = *state;
    for (int64_t i = 0; i < n; ++i) {
        const WalkVoxel v = walk_voxel(s, rule);
        if (v.accepted) entries->push_back(WalkEntry{i, v.raw, 0, v.value});
        for (int k = 0; k < v.steps; ++k) s = (s * JR_A + JR_C) & JR_MASK;
    }
    *state = s;
    return MVSIM_OK;
}

// ordinals (ascending) -> offsets from the centre of the large sphere, in the raster order of the cursor (z, then y, then x fastest)
void ordinals_to_offsets(int64_t R, const std::vector<WalkEntry>& entries, std::vector<std::array<int64_t, 3>>* off)
{
    off->resize(entries.size());
    size_t at = 0;
    int64_t first = 0;                                             // ordinal of the first voxel of the current row
    for (int64_t dz = -R; dz <= R && at < entries.size(); ++dz) {
        const int64_t r1 = isqrt_host(R * R - dz * dz);
        for (int64_t dy = -r1; dy <= r1 && at < entries.size(); ++dy) {
            const int64_t r0 = isqrt_host(r1 * r1 - dy * dy), len = 2 * r0 + 1;
            for (; at < entries.size() && entries[at].ordinal < first + len; ++at) (*off)[at] = {entries[at].ordinal - first - r0, dy, dz};
            first += len;
        }
    }
}

}  // namespace

// drawSpheres on a device image.  rnd_state: the 48-bit state of the caller's java.util.Random, advanced exactly
// as the reference advances it.
int draw_spheres_dev(mvsim_ctx* ctx, float* img, const int64_t dim[3], double min_value, double max_value, int scale,
                     int half_pixel_offset, uint64_t* rnd_state, int64_t* n_spheres)
{
    int64_t c[3], min_size = dim[0];
    for (int d = 0; d < 3; ++d) {
        c[d] = dim[d] / 2;
        if (dim[d] < min_size) min_size = dim[d];
    }
    const int max_radius = 10 * scale;
    const int64_t R = min_size / 2 - 47 * (int64_t)scale - 1;
    if (R < 0) {
        set_error("drawSpheres: image too small for scale %d (large-sphere radius %lld)", scale, (long long)R);
        return MVSIM_EINVAL;
    }
    int64_t modulus = 1;
    for (int d = 0; d < 3; ++d) modulus *= 7 * (int64_t)scale;

    std::vector<SphereItem> items;
    const int off_xy = half_pixel_offset ? 1 : 0;
    if (ctx->opt.sphere_walk >= 1) {                               // option sphere_walk = device: the walk of sphere_walk.hip
        const WalkRule rule{max_radius, SW_RULE_DRAW, modulus};
        uint64_t state = *rnd_state & JR_MASK;
        std::vector<WalkEntry> entries;
        std::vector<std::array<int64_t, 3>> off;
        MVSIM_TRY(walk_entries(ctx, true, sphere_voxels(R), rule, &state, &entries));
        ordinals_to_offsets(R, entries, &off);
        items.resize(entries.size());
        for (size_t i = 0; i < entries.size(); ++i) {
            const double value = entries[i].value * (max_value - min_value) + min_value;
            SphereItem& it = items[i];
            it.cx = (int)(c[0] + off[i][0] + off_xy); it.cy = (int)(c[1] + off[i][1] + off_xy); it.cz = (int)(c[2] + off[i][2]);
            it.r = entries[i].raw + 1; it.v = (float)value;
        }
        // splat_spheres_dev rejects a sphere that leaves the image before anything is written; the generator moves on success only
        MVSIM_TRY(splat_spheres_dev(ctx, img, dim, reinterpret_cast<const mvsim_sphere*>(items.data()), (int64_t)items.size()));
        *rnd_state = state;
        if (n_spheres) *n_spheres = (int64_t)items.size();
        return MVSIM_OK;
    }
    JRandom rnd{*rnd_state & JR_MASK};
    for (int64_t dz = -R; dz <= R; ++dz) {
        const int64_t r1 = isqrt_host(R * R - dz * dz);
        for (int64_t dy = -r1; dy <= r1; ++dy) {
            const int64_t r0 = isqrt_host(r1 * r1 - dy * dy);
            for (int64_t dx = -r0; dx <= r0; ++dx) {
                const int radius = rnd.next_int(max_radius) + 1;
                const double rv = rnd.next_double();
                const int64_t rounded = (int64_t)std::floor(rv * 10000 + 0.5);     // Math.round
                if (rounded % modulus != 0) continue;
                const double value = rnd.next_double() * (max_value - min_value) + min_value;
                SphereItem it;
                it.cx = (int)(c[0] + dx + off_xy); it.cy = (int)(c[1] + dy + off_xy); it.cz = (int)(c[2] + dz);
                it.r = radius; it.v = (float)value;
                if (it.cx - radius < 0 || it.cy - radius < 0 || it.cz - radius < 0 || it.cx + radius >= dim[0] ||
                    it.cy + radius >= dim[1] || it.cz + radius >= dim[2]) {
                    set_error("drawSpheres: a small sphere leaves the image (the reference throws here)");
                    return MVSIM_EINVAL;
                }
                items.push_back(it);
            }
        }
    }
    *rnd_state = rnd.s;
    if (n_spheres) *n_spheres = (int64_t)items.size();
    return splat_spheres_dev(ctx, img, dim, reinterpret_cast<const mvsim_sphere*>(items.data()), (int64_t)items.size());
}

// Max-compositing of a list of small spheres (the GPU half of drawSpheres; also the entry point for hosts that walk
// the large sphere themselves with their own java.util.Random, mvsim_splat_spheres).
int splat_spheres_dev(mvsim_ctx* ctx, float* img, const int64_t dim[3], const mvsim_sphere* spheres, int64_t n)
{
    if (n <= 0) return MVSIM_OK;
    int max_radius = 0;
    for (int64_t i = 0; i < n; ++i) {
        const mvsim_sphere& q = spheres[i];
        if (q.radius < 0 || q.radius > 4096) { set_error("invalid argument: sphere %lld has radius %d", (long long)i, q.radius); return MVSIM_EINVAL; }
        if (q.cx - q.radius < 0 || q.cy - q.radius < 0 || q.cz - q.radius < 0 || (int64_t)q.cx + q.radius >= dim[0] ||
            (int64_t)q.cy + q.radius >= dim[1] || (int64_t)q.cz + q.radius >= dim[2]) {
            set_error("drawSpheres: a small sphere leaves the image (the reference throws here)");
            return MVSIM_EINVAL;
        }
        if (q.radius > max_radius) max_radius = q.radius;
    }
    MVSIM_TRY(ctx->sphere_list.reserve((size_t)n * sizeof(SphereItem)));
    // the list lives in pageable host memory: a synchronous copy (the host walk dominates anyway)
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    MVSIM_HIP(hipMemcpy(ctx->sphere_list.p, spheres, (size_t)n * sizeof(SphereItem), hipMemcpyHostToDevice));
    // Math.max( value, existing ) stores (float)value when value > existing: with monotonic rounding that is the
    // float max of (float)value and existing
    const int64_t chunk = 32768;        // grid.x limit is far away; chunking only bounds a single launch
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t m = n - i0 < chunk ? n - i0 : chunk;
        hipLaunchKernelGGL(k_splat_spheres, dim3((unsigned)m, (unsigned)(2 * max_radius + 1)), dim3(256), 0, ctx->stream,
                           img, (int)dim[0], (int)dim[1], (int)dim[2], ctx->sphere_list.as<SphereItem>() + i0);
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ---- the phantom of the refraction simulator: SimulateMultiViewAberrations.simulate (SMVA:408-440) --------------------------------
// SMVA:425-426: voxel i, x fastest, becomes (float)Math.max(0, t + (nextDouble() - 0.5) / 10).  Two steps of the generator per voxel: a
// lane jumps once to 2 * (its first voxel) and steps over NOISE_PER_LANE consecutive voxels.
constexpr int NOISE_PER_LANE = 8;
__global__ __launch_bounds__(256) void k_ri_noise(float* __restrict__ ri, long long n, uint64_t state)
{
    const long long groups = (n + NOISE_PER_LANE - 1) / NOISE_PER_LANE, nthreads = (long long)gridDim.x * 256;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += nthreads) {
        const long long i0 = g * NOISE_PER_LANE, i1 = i0 + NOISE_PER_LANE < n ? i0 + NOISE_PER_LANE : n;
        JRandom rnd{jr_jump(state, 2 * (uint64_t)i0)};
        for (long long i = i0; i < i1; ++i) {
            const double v = (double)ri[i] + (rnd.next_double() - 0.5) / 10;
            ri[i] = (float)(v > 0.0 ? v : (v != v ? v : 0.0));                     // Math.max(0, v): NaN stays NaN, -0.0 becomes 0.0
        }
    }
}

int ri_noise_dev(mvsim_ctx* ctx, float* ri, int64_t n, uint64_t state)
{
    if (n <= 0) return MVSIM_OK;
    const long long want = ((n + NOISE_PER_LANE - 1) / NOISE_PER_LANE + 255) / 256;
    hipLaunchKernelGGL(k_ri_noise, dim3((unsigned)(want > 65536 ? 65536 : want)), dim3(256), 0, ctx->stream, ri, (long long)n, state);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// SMVA:575-576 in front of the compositing: a covered voxel of the index volume that holds exactly 5.0 takes the sphere's value instead
// of the maximum.  Every such voxel gets -inf here, so that the atomic max that follows replaces it; every writer stores the same bits.
// Geometry as k_splat_spheres.
__global__ __launch_bounds__(256) void k_mark_spheres(float* __restrict__ ri, int nx, int ny, int nz, const SphereItem* __restrict__ items)
{
    const SphereItem it = items[blockIdx.x];
    const int dz = (int)blockIdx.y - it.r;
    if (dz > it.r) return;
    const int r1 = isqrt_dev(it.r * it.r - dz * dz);
    const int w = 2 * r1 + 1;
    const int z = it.cz + dz;
    if (z < 0 || z >= nz) return;
    for (int e = threadIdx.x; e < w * w; e += 256) {
        const int dy = e / w - r1, dx = e % w - r1;
        const int r0 = isqrt_dev(r1 * r1 - dy * dy);
        if (dx < -r0 || dx > r0) continue;
        const int x = it.cx + dx, y = it.cy + dy;
        if (x < 0 || x >= nx || y < 0 || y >= ny) continue;
        float* p = ri + (x + (long long)nx * (y + (long long)ny * z));
        if (__float_as_uint(*p) == 0x40a00000u) *p = __uint_as_float(0xff800000u);
    }
}

// multiSpheres (SMVA:474-586) with the ranges the reference hard-codes, {0.5, 1.0} for the image and {1.0, 1.1} for the index volume (its
// min == max branches are dead code and not offered).  One walk, two item lists: the image is max-composited; the index volume is marked
// (k_mark_spheres), then max-composited -- after the first replacement a voxel holds a value in [1.0, 1.1] and can never equal 5.0 again,
// so the outcome does not depend on the order of the spheres.
int multi_spheres_dev(mvsim_ctx* ctx, float* img, float* ri, const int64_t dim[3], int scale, uint64_t* rnd_state, int64_t* n_spheres)
{
    int64_t c[3], min_size = dim[0];
    for (int d = 0; d < 3; ++d) {
        c[d] = dim[d] / 2;
        if (dim[d] < min_size) min_size = dim[d];
    }
    const int max_radius = 10 * scale;
    const int64_t R = min_size / 2 - 47 * (int64_t)scale - 1;
    if (R < 0) {
        set_error("multiSpheres: image too small for scale %d (large-sphere radius %lld)", scale, (long long)R);
        return MVSIM_EINVAL;
    }
    const WalkRule rule{max_radius, SW_RULE_MULTI, 1};
    uint64_t state = *rnd_state & JR_MASK;
    std::vector<WalkEntry> entries;
    std::vector<std::array<int64_t, 3>> off;
    MVSIM_TRY(walk_entries(ctx, ctx->opt.sphere_walk != 0, sphere_voxels(R), rule, &state, &entries));
    ordinals_to_offsets(R, entries, &off);
    const size_t n = entries.size();
    std::vector<SphereItem> items(2 * n);                          // [image items][index-volume items]
    int biggest = 0;
    for (size_t i = 0; i < n; ++i) {
        SphereItem& im = items[i];
        im.cx = (int)(c[0] + off[i][0]); im.cy = (int)(c[1] + off[i][1]); im.cz = (int)(c[2] + off[i][2]);
        im.r = std::max(entries[i].raw + 1, max_radius - 1);                        // SMVA:546
        im.v = (float)(entries[i].value * (1.0 - 0.5) + 0.5);                      // :563
        items[n + i] = im;
        items[n + i].v = (float)(entries[i].value * (1.1 - 1.0) + 1.0);            // :562
        if (im.cx - im.r < 0 || im.cy - im.r < 0 || im.cz - im.r < 0 || im.cx + im.r >= dim[0] || im.cy + im.r >= dim[1] ||
            im.cz + im.r >= dim[2]) {
            set_error("multiSpheres: a small sphere leaves the image (the reference throws here)");
            return MVSIM_EINVAL;
        }
        biggest = std::max(biggest, im.r);
    }
    *rnd_state = state;
    if (n_spheres) *n_spheres = (int64_t)n;
    if (n == 0) return MVSIM_OK;
    MVSIM_TRY(ctx->sphere_list.reserve(2 * n * sizeof(SphereItem)));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));                  // pageable source, as in splat_spheres_dev
    MVSIM_HIP(hipMemcpy(ctx->sphere_list.p, items.data(), 2 * n * sizeof(SphereItem), hipMemcpyHostToDevice));
    const SphereItem* d_im = ctx->sphere_list.as<SphereItem>();
    const SphereItem* d_ri = d_im + n;
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    const size_t chunk = 32768;
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const dim3 grid((unsigned)std::min(chunk, n - i0), (unsigned)(2 * biggest + 1));
        hipLaunchKernelGGL(k_splat_spheres, grid, dim3(256), 0, ctx->stream, img, nx, ny, nz, d_im + i0);
        hipLaunchKernelGGL(k_mark_spheres, grid, dim3(256), 0, ctx->stream, ri, nx, ny, nz, d_ri + i0);
    }
    for (size_t i0 = 0; i0 < n; i0 += chunk)                        // after EVERY sphere has marked
        hipLaunchKernelGGL(k_splat_spheres, dim3((unsigned)std::min(chunk, n - i0), (unsigned)(2 * biggest + 1)), dim3(256), 0, ctx->stream, ri,
                           nx, ny, nz, d_ri + i0);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
