// The kernels of the bead detector (gfx950, wave64; api_detect.cpp drives them; mvsim.h and DESIGN.md section 17 state the recipe):
//   k_dog_xy    one plane tile of DOG_TILE_X x DOG_TILE_Y voxels per block: the tile and the halo of the larger radius are staged in
//               LDS through the mirror (uint16 widened on load), the x pass and then the y pass run out of LDS for BOTH tap sets,
//               and the two half-blurred volumes are written -- the source crosses HBM once for both sigmas.
//   k_dog_z     one DOG_TILE_X x DOG_TILE_Z tile of an (x, z) slice per block: both half-blurred volumes staged with the z halo, the
//               z pass for both, and only D = G1 - G2 is written -- the two blurred volumes never exist as finished volumes.
//   k_peaks_*   one block per PEAK_BLOCK_VOX consecutive voxels, twice: k_peaks_count evaluates the rule, counts and keeps every wave's
//               ballot; behind an exclusive scan of the counts (hipcub) k_peaks_emit writes the list in index order from the ballots
//               and their prefixes.  No atomics: the list's order is the voxels' order.
//   k_localise  one lane per listed peak: the fp64 quadratic fit and its moves.
// Every product and every sum of a blur is a float operation of its own, in ascending tap order (the build has -ffp-contract=off);
// 16-byte loads and stores where the operand is 16-byte aligned and Nx is a multiple of 4 (8-byte loads for uint16), scalar otherwise.
#include "common.h"
#include "detect.h"

#include <hipcub/hipcub.hpp>

namespace mvsim {

namespace {

constexpr int TAP_PITCH = MVSIM_DOG_MAX_TAPS + 1;    // 64 floats per tap set in LDS

// mirror-single: period 2 n - 2, folded as often as needed (n >= 2)
__device__ __forceinline__ int dog_fold(int i, int n)
{
    const int p = 2 * n - 2;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

__device__ __forceinline__ float dog_load(const float* p) { return *p; }
__device__ __forceinline__ float dog_load(const uint16_t* p) { return (float)*p; }
__device__ __forceinline__ float4 dog_load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 dog_load4(const uint16_t* p)
{
    const ushort4 v = *reinterpret_cast<const ushort4*>(p);
    return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}

// acc = t[0] v_0, then acc = acc + t[j] v_j: s points at the sample of tap 0, consecutive taps are `pitch` floats apart
__device__ __forceinline__ float dog_taps_sum(const float* t, int d, const float* s, int pitch)
{
    float acc = t[0] * s[0];
    for (int j = 1; j < d; ++j) {
        const float prod = t[j] * s[j * pitch];
        acc = acc + prod;
    }
    return acc;
}

// the same for 4 neighbouring columns at once: s is 16-byte aligned, consecutive taps are one tile row (DOG_TILE_X floats) apart, one
// 16-byte LDS read per tap
__device__ __forceinline__ void dog_taps_sum4(const float* t, int d, const float* s, float acc[4])
{
    const float4 v0 = *reinterpret_cast<const float4*>(s);
    acc[0] = t[0] * v0.x; acc[1] = t[0] * v0.y; acc[2] = t[0] * v0.z; acc[3] = t[0] * v0.w;
    for (int j = 1; j < d; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(s + j * DOG_TILE_X);
        const float tj = t[j];
        const float p0 = tj * v.x, p1 = tj * v.y, p2 = tj * v.z, p3 = tj * v.w;
        acc[0] = acc[0] + p0; acc[1] = acc[1] + p1; acc[2] = acc[2] + p2; acc[3] = acc[3] + p3;
    }
}

// LDS (floats): [4 tap sets: x1 x2 y1 y2][stage: SH rows of SW][x-blurred set 1: SH rows of 64][x-blurred set 2]
// SW = 64 + 2 rx, SH = 16 + 2 ry with rx, ry the larger radius of the two sets along x and y
template <class SRC, bool VEC>
__global__ __launch_bounds__(256) void k_dog_xy(const SRC* __restrict__ src, float* __restrict__ h1, float* __restrict__ h2, int nx, int ny,
                                                DogTaps T, int rx, int ry)
{
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x;
    const int SW = DOG_TILE_X + 2 * rx, SH = DOG_TILE_Y + 2 * ry;
    float* tp = lds;
    float* stage = lds + 4 * TAP_PITCH;
    float* xb1 = stage + SH * SW;
    float* xb2 = xb1 + SH * DOG_TILE_X;
    const int x0 = blockIdx.x * DOG_TILE_X, y0 = blockIdx.y * DOG_TILE_Y;
    const long long plane = (long long)blockIdx.z * ny * nx;

    {   // 4 x 64 taps: thread tid copies tap tid & 63 of set tid >> 6
        const int set = tid >> 6, j = tid & 63;
        tp[tid] = T.t[set & 1][set >> 1][j];
    }
    const bool full_x = x0 + DOG_TILE_X <= nx;
    if (VEC && full_x) {
        // the tile's own columns as 4-voxel groups, the halo columns one by one
        for (int idx = tid; idx < SH * (DOG_TILE_X / 4); idx += 256) {
            const int row = idx >> 4, cg = idx & 15;
            const int gy = dog_fold(y0 - ry + row, ny);
            const float4 v = dog_load4(src + plane + (long long)gy * nx + x0 + 4 * cg);
            float* d = stage + row * SW + rx + 4 * cg;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        const int hw = 2 * rx;
        for (int idx = tid; idx < SH * hw; idx += 256) {
            const int row = idx / hw, h = idx - row * hw;
            const int col = h < rx ? h : h + DOG_TILE_X;
            const int gy = dog_fold(y0 - ry + row, ny), gx = dog_fold(x0 - rx + col, nx);
            stage[row * SW + col] = dog_load(src + plane + (long long)gy * nx + gx);
        }
    } else {
        for (int idx = tid; idx < SH * SW; idx += 256) {
            const int row = idx / SW, col = idx - row * SW;
            const int gy = dog_fold(y0 - ry + row, ny), gx = dog_fold(x0 - rx + col, nx);
            stage[idx] = dog_load(src + plane + (long long)gy * nx + gx);
        }
    }
    __syncthreads();

    // x pass: every staged row, both sets off ONE walk over the wider set's window -- each sample is read once, and each set still
    // sums its own taps in ascending order from its own first product (the narrower set's window is the middle of the wider one's)
    {
        const int r1x = T.r[0][0], r2x = T.r[1][0];
        const bool wide1 = r1x >= r2x;                   // uniform
        const float* tw = wide1 ? tp : tp + TAP_PITCH;
        const float* tn = wide1 ? tp + TAP_PITCH : tp;
        float* xw = wide1 ? xb1 : xb2;
        float* xn = wide1 ? xb2 : xb1;
        const int dn = 2 * (wide1 ? r2x : r1x) + 1, o = rx - (dn >> 1), dw = 2 * rx + 1;
        for (int idx = tid; idx < SH * DOG_TILE_X; idx += 256) {
            const int row = idx >> 6, c = idx & 63;
            const float* s = stage + row * SW + c;       // s[j]: the sample of the wider set's tap j
            float v = s[0];
            float aw = tw[0] * v, an = tn[0] * v;        // an: kept only where the windows start together (o == 0)
            int j = 1;
            for (; j < o; ++j) aw = aw + tw[j] * s[j];
            if (o > 0) {
                v = s[o];
                aw = aw + tw[o] * v;
                an = tn[0] * v;
                j = o + 1;
            }
            for (; j < o + dn; ++j) {
                v = s[j];
                const float pw = tw[j] * v, pn = tn[j - o] * v;
                aw = aw + pw;
                an = an + pn;
            }
            for (; j < dw; ++j) aw = aw + tw[j] * s[j];
            xw[idx] = aw;
            xn[idx] = an;
        }
    }
    __syncthreads();

    // y pass: 4 consecutive columns of one row per thread
    const int r1y = T.r[0][1], r2y = T.r[1][1];
    const int cg = tid & 15, row = tid >> 4;
    const int x = x0 + 4 * cg, y = y0 + row;
    if (y >= ny || x >= nx) return;
    float o1[4], o2[4];
    dog_taps_sum4(tp + 2 * TAP_PITCH, 2 * r1y + 1, xb1 + (row + ry - r1y) * DOG_TILE_X + 4 * cg, o1);
    dog_taps_sum4(tp + 3 * TAP_PITCH, 2 * r2y + 1, xb2 + (row + ry - r2y) * DOG_TILE_X + 4 * cg, o2);
    const long long at = plane + (long long)y * nx + x;
    if ((nx & 3) == 0) {                                 // the workspaces are 16-byte aligned: whole groups, aligned
        *reinterpret_cast<float4*>(h1 + at) = make_float4(o1[0], o1[1], o1[2], o1[3]);
        *reinterpret_cast<float4*>(h2 + at) = make_float4(o2[0], o2[1], o2[2], o2[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < nx) { h1[at + k] = o1[k]; h2[at + k] = o2[k]; }
    }
}

// LDS (floats): [2 tap sets: z1 z2][half-blurred set 1: SZ rows of 64][set 2]; SZ = 32 + 2 rz, rz the larger z radius
template <bool VEC>
__global__ __launch_bounds__(256) void k_dog_z(const float* __restrict__ h1, const float* __restrict__ h2, float* __restrict__ dog, int nx,
                                               int ny, int nz, DogTaps T, int rz)
{
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x;
    const int SZ = DOG_TILE_Z + 2 * rz;
    float* tp = lds;
    float* s1 = lds + 2 * TAP_PITCH;
    float* s2 = s1 + SZ * DOG_TILE_X;
    const int x0 = blockIdx.x * DOG_TILE_X, y = blockIdx.y, z0 = blockIdx.z * DOG_TILE_Z;
    const long long row_at = (long long)y * nx, plane_pitch = (long long)ny * nx;

    if (tid < 128) tp[tid] = T.t[tid >> 6][2][tid & 63];
    const bool vec_in = (nx & 3) == 0;                   // the workspaces are 16-byte aligned
    for (int idx = tid; idx < SZ * (DOG_TILE_X / 4); idx += 256) {
        const int row = idx >> 4, cg = idx & 15;
        const int gz = dog_fold(z0 - rz + row, nz);
        const int x = x0 + 4 * cg;
        const long long at = (long long)gz * plane_pitch + row_at + x;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (x < nx) {
            if (vec_in) {
                a = *reinterpret_cast<const float4*>(h1 + at);
                b = *reinterpret_cast<const float4*>(h2 + at);
            } else {
                a.x = h1[at]; b.x = h2[at];
                if (x + 1 < nx) { a.y = h1[at + 1]; b.y = h2[at + 1]; }
                if (x + 2 < nx) { a.z = h1[at + 2]; b.z = h2[at + 2]; }
                if (x + 3 < nx) { a.w = h1[at + 3]; b.w = h2[at + 3]; }
            }
        }
        *reinterpret_cast<float4*>(s1 + row * DOG_TILE_X + 4 * cg) = a;
        *reinterpret_cast<float4*>(s2 + row * DOG_TILE_X + 4 * cg) = b;
    }
    __syncthreads();

    const int r1z = T.r[0][2], r2z = T.r[1][2];
    const int cg = tid & 15, x = x0 + 4 * cg;
    if (x >= nx) return;
#pragma unroll
    for (int pass = 0; pass < DOG_TILE_Z / 16; ++pass) {
        const int zz = (tid >> 4) + 16 * pass, z = z0 + zz;
        if (z >= nz) break;
        float g1[4], g2[4], d[4];
        dog_taps_sum4(tp, 2 * r1z + 1, s1 + (zz + rz - r1z) * DOG_TILE_X + 4 * cg, g1);
        dog_taps_sum4(tp + TAP_PITCH, 2 * r2z + 1, s2 + (zz + rz - r2z) * DOG_TILE_X + 4 * cg, g2);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = g1[k] - g2[k];
        const long long at = (long long)z * plane_pitch + row_at + x;
        if (VEC) {
            *reinterpret_cast<float4*>(dog + at) = make_float4(d[0], d[1], d[2], d[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < nx) dog[at + k] = d[k];
        }
    }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <class SRC>
int launch_dog_xy(mvsim_ctx* ctx, const SRC* src, const int64_t dim[3], const DogTaps& T, float* h1, float* h2)
{
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    const int rx = std::max(T.r[0][0], T.r[1][0]), ry = std::max(T.r[0][1], T.r[1][1]);
    const int SW = DOG_TILE_X + 2 * rx, SH = DOG_TILE_Y + 2 * ry;
    const size_t lds = (size_t)(4 * TAP_PITCH + SH * SW + 2 * SH * DOG_TILE_X) * sizeof(float);
    const bool vec = (nx & 3) == 0 && aligned_to(src, 4 * sizeof(SRC));
    const dim3 grid((unsigned)((nx + DOG_TILE_X - 1) / DOG_TILE_X), (unsigned)((ny + DOG_TILE_Y - 1) / DOG_TILE_Y), (unsigned)nz);
    if (vec) {
        MVSIM_TRY(ensure_lds_attr(ctx, reinterpret_cast<const void*>(k_dog_xy<SRC, true>), lds));
        hipLaunchKernelGGL((k_dog_xy<SRC, true>), grid, dim3(256), lds, ctx->stream, src, h1, h2, nx, ny, T, rx, ry);
    } else {
        MVSIM_TRY(ensure_lds_attr(ctx, reinterpret_cast<const void*>(k_dog_xy<SRC, false>), lds));
        hipLaunchKernelGGL((k_dog_xy<SRC, false>), grid, dim3(256), lds, ctx->stream, src, h1, h2, nx, ny, T, rx, ry);
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace

int launch_dog(mvsim_ctx* ctx, const void* img, int src_type, const int64_t dim[3], const DogTaps& T, float* half1, float* half2, float* dog)
{
    if (ctx->opt.dog_pass != 2) {
        if (src_type == MVSIM_SRC_U16) MVSIM_TRY(launch_dog_xy(ctx, reinterpret_cast<const uint16_t*>(img), dim, T, half1, half2));
        else MVSIM_TRY(launch_dog_xy(ctx, reinterpret_cast<const float*>(img), dim, T, half1, half2));
    }
    if (ctx->opt.dog_pass == 1) return MVSIM_OK;
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    const int rz = std::max(T.r[0][2], T.r[1][2]);
    const size_t lds = (size_t)(2 * TAP_PITCH + 2 * (DOG_TILE_Z + 2 * rz) * DOG_TILE_X) * sizeof(float);
    const dim3 grid((unsigned)((nx + DOG_TILE_X - 1) / DOG_TILE_X), (unsigned)ny, (unsigned)((nz + DOG_TILE_Z - 1) / DOG_TILE_Z));
    if ((nx & 3) == 0 && aligned_to(dog, 16))
        hipLaunchKernelGGL(k_dog_z<true>, grid, dim3(256), lds, ctx->stream, half1, half2, dog, nx, ny, nz, T, rz);
    else
        hipLaunchKernelGGL(k_dog_z<false>, grid, dim3(256), lds, ctx->stream, half1, half2, dog, nx, ny, nz, T, rz);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ---- peaks -----------------------------------------------------------------------------------------------------------------------
namespace {

// step 4 of the recipe for the voxel of linear index idx < n whose value v has been read already
__device__ __forceinline__ bool dog_is_peak(const float* __restrict__ D, int nx, int ny, int nz, long long idx, float v, float threshold)
{
    // the threshold first: all but a few voxels end here, before any division
    if (!(v > threshold)) return false;
    const long long plane = (long long)nx * ny;
    int x, y, z;
    if (plane * nz <= 0x7fffffffLL) {                    // uniform: 32-bit divisions where the volume allows them
        const unsigned i = (unsigned)idx, pl = (unsigned)plane;
        const unsigned zz = i / pl, r = i - zz * pl, yy = r / (unsigned)nx;
        z = (int)zz; y = (int)yy; x = (int)(r - yy * (unsigned)nx);
    } else {
        z = (int)(idx / plane);
        const long long in_plane = idx - (long long)z * plane;
        y = (int)(in_plane / nx);
        x = (int)(in_plane - (long long)y * nx);
    }
    if (x < 1 || x > nx - 2 || y < 1 || y > ny - 2 || z < 1 || z > nz - 2) return false;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const long long off = dx + (long long)nx * dy + plane * dz;
                if (off < 0) { if (!(v > D[idx + off])) return false; }
                else if (off > 0) { if (!(v >= D[idx + off])) return false; }
            }
    return true;
}

// A block takes PEAK_BLOCK_VOX consecutive voxels as PEAK_TRIPS trips of 256: voxel base + 256 trip + tid, so that (trip, wave, lane)
// order is index order.  The counting pass evaluates the rule -- all of a thread's values loaded up front -- and leaves every wave's
// ballot in `masks` (one 64-bit word per 64 voxels); the emitting pass, behind the scan of the counts, reads the words back.
constexpr int PEAK_TRIPS = PEAK_BLOCK_VOX / 256;
constexpr int PEAK_WORDS = PEAK_BLOCK_VOX / 64;          // ballot words of a block: [trip][wave]

__global__ __launch_bounds__(256) void k_peaks_count(const float* __restrict__ D, int nx, int ny, int nz, long long n, float threshold,
                                                     long long* __restrict__ counts, unsigned long long* __restrict__ masks)
{
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long base = (long long)blockIdx.x * PEAK_BLOCK_VOX;
    float v[PEAK_TRIPS];
#pragma unroll
    for (int it = 0; it < PEAK_TRIPS; ++it) {
        const long long idx = base + it * 256 + tid;
        v[it] = idx < n ? D[idx] : 0.0f;
    }
    int count = 0;
#pragma unroll
    for (int it = 0; it < PEAK_TRIPS; ++it) {
        const long long idx = base + it * 256 + tid;
        const bool p = idx < n && dog_is_peak(D, nx, ny, nz, idx, v[it], threshold);
        const unsigned long long mask = __ballot(p);
        if (lane == 0) masks[(long long)blockIdx.x * PEAK_WORDS + it * 4 + wave] = mask;
        count += __popcll(mask);
    }
    if (lane == 0) wave_count[wave] = count;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

__global__ __launch_bounds__(256) void k_peaks_emit(const unsigned long long* __restrict__ masks, const long long* __restrict__ counts,
                                                    const long long* __restrict__ offsets, long long capacity,
                                                    long long* __restrict__ voxels, long long* __restrict__ n_found)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long base = (long long)blockIdx.x * PEAK_BLOCK_VOX;
    const long long first = offsets[blockIdx.x];
    if (tid == 0 && blockIdx.x == gridDim.x - 1) *n_found = first + counts[blockIdx.x];
    if (counts[blockIdx.x] == 0) return;                 // uniform
    const unsigned long long* words = masks + (long long)blockIdx.x * PEAK_WORDS;
    int running = 0;
#pragma unroll
    for (int it = 0; it < PEAK_TRIPS; ++it) {
        int before = 0, all = 0;
        unsigned long long mine = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned long long m = words[it * 4 + w];
            const int c = __popcll(m);
            before += w < wave ? c : 0;
            all += c;
            if (w == wave) mine = m;
        }
        if ((mine >> lane) & 1ull) {
            const long long at = first + running + before + __popcll(mine & ((1ull << lane) - 1ull));
            if (at < capacity) voxels[at] = base + it * 256 + tid;
        }
        running += all;
    }
}

}  // namespace

int64_t peak_blocks(int64_t n) { return (n + PEAK_BLOCK_VOX - 1) / PEAK_BLOCK_VOX; }

size_t peaks_counts_bytes(int64_t n) { return (size_t)peak_blocks(n) * (2 + PEAK_WORDS) * sizeof(int64_t); }

size_t peaks_scan_bytes(int64_t n)
{
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (long long*)nullptr, (long long*)nullptr, (int)peak_blocks(n), (hipStream_t) nullptr);
    return std::max<size_t>(bytes, 256);
}

int launch_find_peaks(hipStream_t s, const float* vol, const int64_t dim[3], float threshold, int64_t capacity, int64_t* voxels,
                      int64_t* n_found, int64_t* counts, void* scan_tmp, size_t scan_bytes)
{
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    const long long n = (long long)nx * ny * nz;
    const int nb = (int)peak_blocks(n);
    long long* cnt = reinterpret_cast<long long*>(counts);
    long long* off = cnt + nb;
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(off + nb);
    hipLaunchKernelGGL(k_peaks_count, dim3(nb), dim3(256), 0, s, vol, nx, ny, nz, n, threshold, cnt, masks);
    MVSIM_HIP(hipGetLastError());
    MVSIM_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, cnt, off, nb, s));
    hipLaunchKernelGGL(k_peaks_emit, dim3(nb), dim3(256), 0, s, (const unsigned long long*)masks, (const long long*)cnt, (const long long*)off,
                       (long long)capacity, reinterpret_cast<long long*>(voxels), reinterpret_cast<long long*>(n_found));
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ---- localisation ----------------------------------------------------------------------------------------------------------------
namespace {

struct DogFit {
    double g[3], o[3], c;
    bool   singular;
};

// step 5 of the recipe at the interior voxel idx; the operation order is the header's
__device__ __forceinline__ DogFit dog_fit(const float* __restrict__ D, const long long st[3], long long idx)
{
    DogFit f;
    f.c = (double)D[idx];
    double h[3][3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double p = (double)D[idx + st[d]], m = (double)D[idx - st[d]];
        f.g[d] = (p - m) / 2.0;
        h[d][d] = (p - 2.0 * f.c) + m;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int e = d + 1; e < 3; ++e) {
            const double pp = (double)D[idx + st[d] + st[e]], mp = (double)D[idx - st[d] + st[e]];
            const double pm = (double)D[idx + st[d] - st[e]], mm = (double)D[idx - st[d] - st[e]];
            h[d][e] = h[e][d] = (((pp - mp) - pm) + mm) / 4.0;
        }
    const double m00 = h[0][0], m01 = h[0][1], m02 = h[0][2], m10 = h[1][0], m11 = h[1][1], m12 = h[1][2], m20 = h[2][0], m21 = h[2][1],
                 m22 = h[2][2];
    const double det = m00 * m11 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20 - m00 * m12 * m21 - m01 * m10 * m22;
    f.singular = det == 0.0 || !isfinite(det);
    f.o[0] = f.o[1] = f.o[2] = 0.0;
    if (f.singular) return f;
    const double idet = 1.0 / det;
    const double i00 = (m11 * m22 - m12 * m21) * idet, i01 = (m02 * m21 - m01 * m22) * idet, i02 = (m01 * m12 - m02 * m11) * idet;
    const double i10 = (m12 * m20 - m10 * m22) * idet, i11 = (m00 * m22 - m02 * m20) * idet, i12 = (m02 * m10 - m00 * m12) * idet;
    const double i20 = (m10 * m21 - m11 * m20) * idet, i21 = (m01 * m20 - m00 * m21) * idet, i22 = (m00 * m11 - m01 * m10) * idet;
    const double ox = -((i00 * f.g[0] + i01 * f.g[1]) + i02 * f.g[2]);
    const double oy = -((i10 * f.g[0] + i11 * f.g[1]) + i12 * f.g[2]);
    const double oz = -((i20 * f.g[0] + i21 * f.g[1]) + i22 * f.g[2]);
    if (!isfinite(ox) || !isfinite(oy) || !isfinite(oz)) { f.singular = true; return f; }
    f.o[0] = ox; f.o[1] = oy; f.o[2] = oz;
    return f;
}

__global__ __launch_bounds__(256) void k_localise(const float* __restrict__ D, int nx, int ny, int nz, const long long* __restrict__ voxels,
                                                  const long long* __restrict__ n_found, long long capacity, int max_moves,
                                                  mvsim_peak* __restrict__ peaks)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long listed = *n_found < capacity ? *n_found : capacity;
    if (i >= listed) return;
    const long long plane = (long long)nx * ny, total = plane * nz;
    const long long v = voxels[i];
    const int N[3] = {nx, ny, nz};
    const long long st[3] = {1, nx, plane};
    int b[3] = {0, 0, 0};
    bool inside = v >= 0 && v < total;
    if (inside) {
        b[2] = (int)(v / plane);
        const long long in_plane = v - (long long)b[2] * plane;
        b[1] = (int)(in_plane / nx);
        b[0] = (int)(in_plane - (long long)b[1] * nx);
        for (int d = 0; d < 3; ++d) inside = inside && b[d] >= 1 && b[d] <= N[d] - 2;
    }
    mvsim_peak out;
    if (!inside) {
        out.pos[0] = (double)b[0]; out.pos[1] = (double)b[1]; out.pos[2] = (double)b[2];
        out.value = 0.0f; out.flags = MVSIM_PEAK_OUTSIDE; out.voxel = v;
        peaks[i] = out;
        return;
    }
    int moved[3] = {0, 0, 0};
    int moves = 0, flags = 0;
    long long idx = v;
    DogFit f;
    for (;;) {
        f = dog_fit(D, st, idx);
        flags = f.singular ? MVSIM_PEAK_SINGULAR : 0;
        int step[3] = {0, 0, 0};
        bool any = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (!(fabs(f.o[d]) > 0.5)) continue;
            const int dir = f.o[d] > 0.0 ? 1 : -1;
            const int nb = b[d] + dir;
            if (nb < 1 || nb > N[d] - 2) continue;
            if (moved[d] == -dir) { flags |= MVSIM_PEAK_FROZEN; continue; }
            step[d] = dir;
            any = true;
        }
        if (!any) break;
        if (moves >= max_moves) { flags |= MVSIM_PEAK_CAPPED; break; }
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (step[d] != 0) { b[d] += step[d]; idx += step[d] * st[d]; moved[d] = step[d]; }
        moves += 1;
    }
    out.pos[0] = (double)b[0] + f.o[0];
    out.pos[1] = (double)b[1] + f.o[1];
    out.pos[2] = (double)b[2] + f.o[2];
    out.value = (float)(f.c + 0.5 * ((f.g[0] * f.o[0] + f.g[1] * f.o[1]) + f.g[2] * f.o[2]));
    out.flags = flags;
    out.voxel = idx;
    peaks[i] = out;
}

}  // namespace

int launch_localise(hipStream_t s, const float* vol, const int64_t dim[3], const int64_t* voxels, const int64_t* n_found, int64_t capacity,
                    int max_moves, mvsim_peak* peaks)
{
    const int64_t blocks = (capacity + 255) / 256;
    hipLaunchKernelGGL(k_localise, dim3((unsigned)blocks), dim3(256), 0, s, vol, (int)dim[0], (int)dim[1], (int)dim[2],
                       reinterpret_cast<const long long*>(voxels), reinterpret_cast<const long long*>(n_found), (long long)capacity, max_moves,
                       peaks);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
