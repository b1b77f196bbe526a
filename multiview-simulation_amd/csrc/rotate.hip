// rotateAroundAxis and attenuate3d of the per-view path (gfx950, wave64): the two stage operators and their fused forms.
// All are HBM- or latency-bound; design notes and algorithmic bytes per voxel are in DESIGN.md.  The arithmetic of the
// rotation about x and of the attenuation is stated once, in rotate_dev.h; the kernels here differ in who computes a row's
// geometry and in how the loads are issued.  (The third fused form, with the convolution's x transform: rotate_fft.hip.)
#include "common.h"

namespace mvsim {

// ------------------------------------------------------------------------------------------------
// rotateAroundAxis (SimulateMultiViewDataset.java:104-135)
// out[l] = trilinear(in zero-extended, Minv * l); ImgLib2 NLinearInterpolator arithmetic: weights
// in double, each tap rounded (float)(v * w), float accumulation in Gray-code tap order.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tap0(const float* __restrict__ in, int nx, int ny, int nz, long long x,
                                      long long y, long long z)
{
    if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return 0.0f;
    return in[x + (long long)nx * (y + (long long)ny * z)];
}

__global__ __launch_bounds__(256) void k_rotate_generic(const float* __restrict__ in, float* __restrict__ out,
                                                        int nx, int ny, int nz, Affine a)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int z = blockIdx.z;
    if (x >= nx) return;
    const double l0 = (double)x, l1 = (double)y, l2 = (double)z;
    const double px = l0 * a.m[0] + l1 * a.m[1] + l2 * a.m[2] + a.m[3];
    const double py = l0 * a.m[4] + l1 * a.m[5] + l2 * a.m[6] + a.m[7];
    const double pz = l0 * a.m[8] + l1 * a.m[9] + l2 * a.m[10] + a.m[11];
    const double fx = floor(px), fy = floor(py), fz = floor(pz);
    float acc = 0.0f;
    // whole 2x2x2 support outside the volume -> exact zero (also keeps the long long casts safe)
    if (fx >= -1.0 && fy >= -1.0 && fz >= -1.0 && fx < (double)nx && fy < (double)ny && fz < (double)nz) {
        const long long sx = (long long)fx, sy = (long long)fy, sz = (long long)fz;
        const double w0 = px - fx, w1 = py - fy, w2 = pz - fz;
        const double w0n = 1.0 - w0, w1n = 1.0 - w1, w2n = 1.0 - w2;
        acc = (float)((double)tap0(in, nx, ny, nz, sx, sy, sz) * (w0n * w1n * w2n));
        acc += (float)((double)tap0(in, nx, ny, nz, sx + 1, sy, sz) * (w0 * w1n * w2n));
        acc += (float)((double)tap0(in, nx, ny, nz, sx + 1, sy + 1, sz) * (w0 * w1 * w2n));
        acc += (float)((double)tap0(in, nx, ny, nz, sx, sy + 1, sz) * (w0n * w1 * w2n));
        acc += (float)((double)tap0(in, nx, ny, nz, sx, sy + 1, sz + 1) * (w0n * w1 * w2));
        acc += (float)((double)tap0(in, nx, ny, nz, sx + 1, sy + 1, sz + 1) * (w0 * w1 * w2));
        acc += (float)((double)tap0(in, nx, ny, nz, sx + 1, sy, sz + 1) * (w0 * w1n * w2));
        acc += (float)((double)tap0(in, nx, ny, nz, sx, sy, sz + 1) * (w0n * w1n * w2));
    }
    out[x + (long long)nx * (y + (long long)ny * z)] = acc;
}

// Rotation about x: an output x-row reads 4 source rows at the same x with wave-uniform weights (rotate_dev.h).
// 4 voxels per lane (16-B loads/stores), ROT_ROWS consecutive output rows per block with all 4*ROT_ROWS row loads
// issued before the first blend.
constexpr int ROT_ROWS = 4;

__global__ __launch_bounds__(128) void k_rotate_axis0_v4(const float* __restrict__ in, float* __restrict__ out,
                                                         int nx, int ny, int nz, Affine a)
{
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int y0 = blockIdx.y * ROT_ROWS;
    const int z = blockIdx.z;
    if (x4 >= nx) return;
    const long long row = (long long)nx;
    const long long row_b = row * 4, plane_b = row_b * ny;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v00[ROT_ROWS], v10[ROT_ROWS], v11[ROT_ROWS], v01[ROT_ROWS];
    RowGeo g[ROT_ROWS];
#pragma unroll
    for (int r = 0; r < ROT_ROWS; ++r) {
        const int y = y0 + r;
        g[r] = row_geometry(a, y, (double)z, ny, nz, row);
        v00[r] = v10[r] = v11[r] = v01[r] = zero;
        const int kind = g[r].kind;
        if (y < ny && kind != 0) {
            const char* __restrict__ p00 = reinterpret_cast<const char*>(in + x4) + g[r].off00;
            if (tap_inside(kind, 0)) v00[r] = *reinterpret_cast<const float4*>(p00);
            if (tap_inside(kind, 1)) v10[r] = *reinterpret_cast<const float4*>(p00 + row_b);
            if (tap_inside(kind, 2)) v11[r] = *reinterpret_cast<const float4*>(p00 + row_b + plane_b);
            if (tap_inside(kind, 3)) v01[r] = *reinterpret_cast<const float4*>(p00 + plane_b);
        }
    }
#pragma unroll
    for (int r = 0; r < ROT_ROWS; ++r) {
        const int y = y0 + r;
        if (y >= ny) break;
        float4 o;
        o.x = blend4(v00[r].x, v10[r].x, v11[r].x, v01[r].x, g[r]);
        o.y = blend4(v00[r].y, v10[r].y, v11[r].y, v01[r].y, g[r]);
        o.z = blend4(v00[r].z, v10[r].z, v11[r].z, v01[r].z, g[r]);
        o.w = blend4(v00[r].w, v10[r].w, v11[r].w, v01[r].w, g[r]);
        *reinterpret_cast<float4*>(out + x4 + (long long)nx * (y + (long long)ny * z)) = o;
    }
}

int launch_rotate(hipStream_t s, const float* in, float* out, const int64_t dim[3], const Affine& inv)
{
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    const bool aligned = (nx % 4 == 0) && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16 == 0);
    if (affine_is_x_rotation(inv) && aligned) {
        const int threads = 128;
        dim3 grid((nx / 4 + threads - 1) / threads, (ny + ROT_ROWS - 1) / ROT_ROWS, nz);
        hipLaunchKernelGGL(k_rotate_axis0_v4, grid, dim3(threads), 0, s, in, out, nx, ny, nz, inv);
    } else {
        const int threads = 256;
        dim3 grid((nx + threads - 1) / threads, ny, nz);
        hipLaunchKernelGGL(k_rotate_generic, grid, dim3(threads), 0, s, in, out, nx, ny, nz, inv);
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ------------------------------------------------------------------------------------------------
// attenuate3d (SimulateMultiViewDataset.java:318-364).  One (x,z) column per lane, lanes along x
// (coalesced 256-B rows per wave per y step), serial fp64 recurrence from y = Ny-1 downwards:
//   phi = v*delta*n ; n = max(n - phi, 0) ; out = (float)(v*n)
// `steps` = Nx (the reference loops dimension(0) times, Q1); rows below stay zero.
// ------------------------------------------------------------------------------------------------
template <int U>
__global__ __launch_bounds__(64) void k_attenuate(const float* __restrict__ in, float* __restrict__ out, int nx,
                                                  int ny, int steps, double delta)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int z = blockIdx.y;
    if (x >= nx) return;
    const long long plane = (long long)nx * ny;
    const float* __restrict__ pin = in + plane * z + x;
    float* __restrict__ pout = out + plane * z + x;
    double n = 1.0;
    int y = ny - 1;
    int left = steps;
    while (left >= U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = pin[(long long)(y - u) * nx];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float o = attenuate_step(n, v[u], delta);
            pout[(long long)(y - u) * nx] = o;
        }
        y -= U;
        left -= U;
    }
    for (; left > 0; --left, --y) {
        const float o = attenuate_step(n, pin[(long long)y * nx], delta);
        pout[(long long)y * nx] = o;
    }
    for (; y >= 0; --y) pout[(long long)y * nx] = 0.0f;
}

// ------------------------------------------------------------------------------------------------
// attenuate3d as a wavefront-level prefix scan (option attenuate=scan; north_star's formulation).  In exact arithmetic
// the recurrence n <- max(n - v delta n, 0) is n_k = PROD_{j<=k} max(1 - v_j delta, 0): lanes run ALONG the illumination
// axis (64 consecutive y per wave), every lane forms its factor, an inclusive product scan across the wave (6 shuffle
// steps in fp64) gives the prefix products, and the product of the chunk carries into the next 64 rows.  Tiles of
// 64 (y) x 64 (x) go through LDS so that HBM sees whole rows although lanes walk columns.  This re-associates the fp64
// roundings of the reference's serial loop: results agree with k_attenuate to ~1e-15 relative in n, i.e. the float outputs
// are identical except where v*n falls within that distance of a rounding boundary (measured: < 1e-6 of the voxels, by one
// ulp).  Parallelism comes from y as well as from (x, z): the form for thin volumes; the serial kernels, which are
// bit-exact against the oracle, stay the default.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_attenuate_scan(const float* __restrict__ in, float* __restrict__ out, int nx, int ny,
                                                        int steps, double delta)
{
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, z = blockIdx.y;
    const long long plane = (long long)nx * ny;
    const float* __restrict__ pin = in + plane * z;
    float* __restrict__ pout = out + plane * z;
    const bool xin = x0 + lane < nx;
    double carry[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) carry[i] = 1.0;
    for (int j0 = 0; j0 < steps; j0 += 64) {
        // rows y = ny - 1 - (j0 + r), r = 0..63: wave w brings in rows 16 w .. 16 w + 15, lanes along x
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int r = wave * 16 + rr;
            float v = 0.f;
            if (j0 + r < steps && xin) v = pin[(long long)(ny - 1 - (j0 + r)) * nx + x0 + lane];
            tile[r][lane] = v;
        }
        __syncthreads();
        const bool live = j0 + lane < steps;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = wave * 16 + i;
            const double dv = (double)tile[lane][c];
            double p = live ? fmax(1.0 - dv * delta, 0.0) : 1.0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const double t = __shfl_up(p, d, 64);
                if (lane >= d) p *= t;
            }
            const double n = carry[i] * p;
            tile[lane][c] = (float)(dv * n);
            carry[i] = carry[i] * __shfl(p, 63, 64);
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int r = wave * 16 + rr;
            if (j0 + r < steps && xin) pout[(long long)(ny - 1 - (j0 + r)) * nx + x0 + lane] = tile[r][lane];
        }
        __syncthreads();
    }
    // rows the reference never visits (Ny > Nx): the attenuated image stays zero there
    for (int yy = ny - 1 - steps - wave; yy >= 0; yy -= 4)
        if (xin) pout[(long long)yy * nx + x0 + lane] = 0.f;
}

int launch_attenuate_scan(hipStream_t s, const float* in, float* out, const int64_t dim[3], double delta)
{
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    dim3 grid((nx + 63) / 64, nz);
    hipLaunchKernelGGL(k_attenuate_scan, grid, dim3(256), 0, s, in, out, nx, ny, nx, delta);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_attenuate(hipStream_t s, const float* in, float* out, const int64_t dim[3], double delta)
{
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    dim3 grid((nx + 63) / 64, nz);
    hipLaunchKernelGGL(k_attenuate<16>, grid, dim3(64), 0, s, in, out, nx, ny, nx, delta);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ------------------------------------------------------------------------------------------------
// Fused rotate (about x) + attenuate for the per-view pipeline: a lane owns one (x,z) column and walks y from Ny-1
// downwards; every step blends the 4 source rows exactly as k_rotate_axis0_v4 does and feeds the value straight into
// the attenuation recurrence, so `rot` never makes the round trip through HBM (saves 8 N bytes per view).  Same
// arithmetic, same order => bit-identical to the two separate kernels.  rot_out may be null.
// Here every lane recomputes the row geometry (option fused_rotate=lane, kept for A/B runs).
// ------------------------------------------------------------------------------------------------
template <int U, bool WRITE_ROT>
__global__ __launch_bounds__(64) void k_rotate_attenuate_axis0(const float* __restrict__ in, float* __restrict__ rot_out,
                                                               float* __restrict__ att_out, int nx, int ny, int nz,
                                                               int steps, Affine a, double delta, int z_off)
{
    // blockIdx.y counts the planes of the OUTPUT buffers, which start at plane z_off of the view (z-slab tiling; 0
    // for a whole view); the source volume is always the whole ground truth
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int z = blockIdx.y + z_off;
    if (x >= nx) return;
    const long long row = (long long)nx;
    const long long plane = row * ny;
    float* __restrict__ patt = att_out + plane * blockIdx.y + x;
    float* __restrict__ prot = WRITE_ROT ? rot_out + plane * blockIdx.y + x : nullptr;
    const double l2 = (double)z;
    double n = 1.0;
    int y = ny - 1;
    int left = steps;
    while (left > 0) {
        float v00[U], v10[U], v11[U], v01[U];
        RowGeo g[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < left) {
                g[u] = row_geometry(a, y - u, l2, ny, nz, row);
                load_taps_masked(in, g[u], g[u].kind, true, x, row, plane, v00[u], v10[u], v11[u], v01[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < left) {
                const int yy = y - u;
                const float r = blend4(v00[u], v10[u], v11[u], v01[u], g[u]);
                if (WRITE_ROT) prot[(long long)yy * nx] = r;
                patt[(long long)yy * nx] = attenuate_step(n, r, delta);
            }
        }
        y -= U;
        left -= U;
    }
    // rows the reference never visits (Ny > Nx): attenuated image stays zero; rot still needs its values
    for (int yy = ny - 1 - steps; yy >= 0; --yy) {
        patt[(long long)yy * nx] = 0.f;
        if (WRITE_ROT) prot[(long long)yy * nx] = rot_value(in, a, x, yy, l2, nx, ny, nz);
    }
}

// ------------------------------------------------------------------------------------------------
// Same arithmetic, different decomposition (the production form): the geometry of an output row (y, z) -- the two
// source rows, the four fp64 weights -- is the same for every x, and the scalar unit has no fp64, so the kernel
// above spends half of its vector instructions recomputing wave-uniform values in every lane.  Here a block covers
// the WHOLE x extent of one plane (up to 16 waves), the threads first compute the geometry of the rows of a chunk
// once, one row per thread, into an LDS table, and every lane then fetches a row's entry with same-address (broadcast)
// LDS reads while it walks y.  The element offset of the first source row and the row class come back to the scalar
// unit through v_readfirstlane, so the four row loads and the stores use scalar base addresses and the lane's
// constant x offset.  Row classes: 0 = no tap inside the volume (output is +0, attenuation state unchanged -- what the
// generic arithmetic produces for four zero taps), 1 = all four source rows inside, 2 = some inside (per-tap mask).
// Rounding points unchanged => bit-identical to k_rotate_axis0_v4 + k_attenuate and to the kernel above.
// ------------------------------------------------------------------------------------------------
constexpr int GEO_CHUNK = 512;  // rows per LDS table (24 KB)

template <int U, bool WRITE_ROT>
__global__ __launch_bounds__(1024) void k_rotate_attenuate_axis0_lds(const float* __restrict__ in, float* __restrict__ rot_out,
                                                                     float* __restrict__ att_out, int nx, int ny, int nz,
                                                                     int steps, Affine a, double delta, int z_off, int z_cnt,
                                                                     const Affine* __restrict__ atab, long long view_stride)
{
    __shared__ RowGeo geo[GEO_CHUNK];
    __shared__ int bclass[GEO_CHUNK / U];
    if (atab) {
        // stacked views of ONE ground truth (mvsim_simulate_views_dev): blockIdx.z names the view -- its inverse model from the table,
        // its planes `view_stride` voxels further on in the outputs
        a = atab[blockIdx.z];
        att_out += (long long)blockIdx.z * view_stride;
        if (WRITE_ROT) rot_out += (long long)blockIdx.z * view_stride;
    }
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    // Plane order: consecutive block ids go to different XCDs (round-robin dispatch, for speed only), and the output
    // planes z and z + 1 read the same source rows; giving every XCD a contiguous slab of planes keeps that reuse inside
    // one L2 (otherwise each source row is fetched from HBM by two XCDs: measured 1.07 GB instead of 0.54 GB of reads).
    const int slab = (gridDim.y + 7) / 8;
    const int zl = (int)(blockIdx.y % 8u) * slab + (int)(blockIdx.y / 8u);
    if (zl >= z_cnt) return;                          // whole block: uniform
    const int z = zl + z_off;
    const bool active = x < nx;                       // no early exit past this point: every thread takes part in the barriers
    const long long row = (long long)nx;
    const long long plane = row * ny;
    const long long out_plane = plane * zl;           // output buffers start at plane z_off of the view
    const double l2 = (double)z;
    // byte-addressed views for the straight-line path: scalar 64-bit bases plus one 32-bit per-lane offset
    const char* __restrict__ in_b = reinterpret_cast<const char*>(in);
    const long long row_b = row * 4, plane_b = plane * 4;
    const unsigned xoff = (unsigned)(active ? x : nx - 1) * 4u;
    double n = 1.0;
    for (int c0 = 0; c0 < steps; c0 += GEO_CHUNK) {
        const int cnt = min(GEO_CHUNK, steps - c0);
        if (c0 > 0) __syncthreads();                  // the previous chunk's readers are done
        fill_row_tables<U>(geo, bclass, a, l2, ny, nz, row, c0, cnt, (int)threadIdx.x, (int)blockDim.x);
        __syncthreads();
        for (int r0 = 0; r0 < cnt; r0 += U) {
            const int cls = __builtin_amdgcn_readfirstlane(bclass[r0 / U]);
            const int y0 = ny - 1 - (c0 + r0);                        // rows y0, y0 - 1, ..., y0 - U + 1
            if (cls == 1) {
                // straight-line: U offsets from the table, U x 4 row loads, then the U dependent steps
                long long offs[U];
#pragma unroll
                for (int u = 0; u < U; ++u) offs[u] = geo[r0 + u].off00;
                float v00[U], v10[U], v11[U], v01[U];
#pragma unroll
                for (int u = 0; u < U; ++u) issue_row_loads(in_b, offs[u], row_b, plane_b, xoff, v00[u], v10[u], v11[u], v01[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float r = blend4(v00[u], v10[u], v11[u], v01[u], geo[r0 + u]);
                    const float v = attenuate_step(n, r, delta);
                    if (active) {
                        const long long ob = (out_plane + (long long)(y0 - u) * row) * 4;                    // scalar
                        if (WRITE_ROT) *reinterpret_cast<float*>(reinterpret_cast<char*>(rot_out) + ob + xoff) = r;
                        *reinterpret_cast<float*>(reinterpret_cast<char*>(att_out) + ob + xoff) = v;
                    }
                }
            } else if (cls == 0) {
                // four zero taps per row: r = +0, n = max(n - 0 * delta * n, 0) = n, out = (float)(0 * n) = +0
                if (active) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const long long o = out_plane + (long long)(y0 - u) * row;
                        if (WRITE_ROT) rot_out[o + x] = 0.f;
                        att_out[o + x] = 0.f;
                    }
                }
            } else {
                for (int u = 0; u < U && r0 + u < cnt; ++u) {
                    const RowGeo* g = &geo[r0 + u];
                    const int kind = __builtin_amdgcn_readfirstlane(g->kind);
                    const long long o = out_plane + (long long)(y0 - u) * row;
                    float r = 0.f, v = 0.f;
                    if (kind != 0) {            // (a row of kind 0 leaves the attenuation state alone)
                        float a00, a10, a11, a01;
                        load_taps_masked(in, *g, kind, active, x, row, plane, a00, a10, a11, a01);
                        r = blend4(a00, a10, a11, a01, *g);
                        v = attenuate_step(n, r, delta);
                    }
                    if (active) {
                        att_out[o + x] = v;
                        if (WRITE_ROT) rot_out[o + x] = r;
                    }
                }
            }
        }
    }
    // rows the reference never visits (Ny > Nx): attenuated image stays zero; rot still needs its values
    for (int yy = ny - 1 - steps; yy >= 0; --yy) {
        if (!active) break;
        att_out[out_plane + (long long)yy * row + x] = 0.f;
        if (WRITE_ROT) rot_out[out_plane + (long long)yy * row + x] = rot_value(in, a, x, yy, l2, nx, ny, nz);
    }
}

// The LDS-table kernel: one block per plane and 1024-column stripe -- nx / 64 waves (at most 16) share one geometry table.
// Planes [z_begin, z_begin + z_count) of one view (atab null, inverse model `inv`), or all planes of `nviews` stacked views
// whose inverse models are in the device table `atab` (blockIdx.z = view).
static void launch_lds(hipStream_t s, const float* in, float* rot_or_null, float* att, const int64_t dim[3], const Affine& inv,
                       double delta, int z_begin, int z_count, const Affine* atab, int nviews)
{
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    const int waves = (nx + 63) / 64 < 16 ? (nx + 63) / 64 : 16;
    dim3 grid_l((nx + waves * 64 - 1) / (waves * 64), (z_count + 7) / 8 * 8, nviews), block_l(waves * 64);
    const long long view_stride = atab ? (long long)nx * ny * nz : 0ll;
    if (rot_or_null)
        hipLaunchKernelGGL((k_rotate_attenuate_axis0_lds<8, true>), grid_l, block_l, 0, s, in, rot_or_null, att, nx, ny, nz, nx, inv, delta, z_begin, z_count,
                           atab, view_stride);
    else
        hipLaunchKernelGGL((k_rotate_attenuate_axis0_lds<8, false>), grid_l, block_l, 0, s, in, rot_or_null, att, nx, ny, nz, nx, inv, delta, z_begin, z_count,
                           atab, view_stride);
}

// returns MVSIM_OK and sets *fused = false when the fast-path conditions do not hold (caller runs the two kernels)
int launch_rotate_attenuate(hipStream_t s, const float* in, float* rot_or_null, float* att, const int64_t dim[3],
                            const Affine& inv, double delta, int fused_mode, bool* fused)
{
    return launch_rotate_attenuate_planes(s, in, rot_or_null, att, dim, inv, delta, 0, (int)dim[2], fused_mode, fused);
}

// planes [z_begin, z_begin + z_count) of the view into buffers that start at plane z_begin
int launch_rotate_attenuate_planes(hipStream_t s, const float* in, float* rot_or_null, float* att, const int64_t dim[3],
                                   const Affine& inv, double delta, int z_begin, int z_count, int fused_mode, bool* fused)
{
    const int nx = (int)dim[0], ny = (int)dim[1], nz = (int)dim[2];
    // fused_mode: 0 separate kernels, 1 geometry table in LDS, 2 every lane recomputes the row geometry, 3 = 1 when the
    // columns fill the chip (>= 2 waves per SIMD), else 0
    // (the separate rotate is only fast in its 16-byte form: Nx % 4 == 0, aligned rows; the generic one is 3x slower than
    // the fused kernel -- the reference's own 289^3 volume: 0.38 ms against 0.10 ms)
    if (fused_mode == 3) {
        const bool vec4 = nx % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(att)) % 16 == 0);
        fused_mode = ((int64_t)nx * z_count >= 131072 || !vec4) ? 1 : 0;
    }
    *fused = affine_is_x_rotation(inv) && fused_mode != 0;
    if (!*fused) return MVSIM_OK;
    if (fused_mode == 1) {
        launch_lds(s, in, rot_or_null, att, dim, inv, delta, z_begin, z_count, nullptr, 1);
        MVSIM_HIP(hipGetLastError());
        return MVSIM_OK;
    }
    dim3 grid((nx + 63) / 64, z_count);
    if (rot_or_null)
        hipLaunchKernelGGL((k_rotate_attenuate_axis0<8, true>), grid, dim3(64), 0, s, in, rot_or_null, att, nx, ny, nz, nx, inv, delta, z_begin);
    else
        hipLaunchKernelGGL((k_rotate_attenuate_axis0<8, false>), grid, dim3(64), 0, s, in, rot_or_null, att, nx, ny, nz, nx, inv, delta, z_begin);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// `nviews` views of one ground truth (rotation about x each, inverse models in the device table `atab`) into the stacked attenuated
// volumes att[v][Nz][Ny][Nx]: ONE launch whose grid carries the view index, so that views too small to fill the chip fill it
// together -- a 128^3 view is 256 waves of serial latency, eight of them are two waves per SIMD.
int launch_rotate_attenuate_views(hipStream_t s, const float* in, float* att, const int64_t dim[3], const Affine* atab, int nviews, double delta)
{
    launch_lds(s, in, nullptr, att, dim, Affine{}, delta, 0, (int)dim[2], atab, nviews);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
