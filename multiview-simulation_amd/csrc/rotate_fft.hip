// Rotate (about x) + attenuate + the x transform of the convolution as ONE kernel: the attenuated volume never makes its
// round trip through HBM (SimulateMultiViewDataset.java:570-580 -- rotateAroundAxis, attenuate3d, and the first pass of
// convolve's FFT).  The rotate+attenuate kernel (rotate.hip: k_rotate_attenuate_axis0_lds) already holds complete x rows
// of the attenuated plane, one value per lane, while it walks y; pass A of the hand-written convolution
// (fft_passes.hip: k_fft_x_r2c) transforms exactly those rows.  Here a block -- all the x columns of one plane -- walks
// y in batches of U = 8 rows: every lane blends, attenuates (rotate_dev.h: same arithmetic, same order: `att`, and `rot`, stay
// bit-identical and are still written when the caller asks for them) and drops its value into an LDS row with the
// mirror halo of the padded row; after one barrier each wave owns a row end to end -- packed real FFT of M = Px/2
// points, half-spectrum post-processing, 16-byte stores into the spectrum buffer -- while the row buffers are double
// buffered, so that the faster waves already walk the next batch.  Saves 8 N bytes of HBM traffic per view and a launch;
// the spectrum is bit-identical to pass A's (same plan, same twiddles, same post-processing on the same values).
#include "common.h"
#include "fft_dev.h"
#include "rotate_rounds.h"

#include <type_traits>

namespace mvsim {
namespace fft {

// rows per LDS geometry table: 512 (24 KB) for blocks of up to 8 waves, 128 for the 16-wave blocks of rows longer than 512
// voxels, whose double-buffered 16-row transform rounds take 144 KB of the CU's 160
constexpr int geo_chunk_f(int G) { return G == 1 ? 512 : 128; }
constexpr int UF = 8;
// rows of the NEXT batch requested before this batch's transforms (their latency would hide behind the FFTs).  Measured at
// 512^3: 0 -> 0.43 ms, 2 -> 0.46 ms, 4 -> 0.46 ms (128 VGPRs, 4 spilled), also with the LDS-only round barrier that lets loads
// stay in flight across it (0.40 against 0.42 ms): the kernel is not waiting for these loads -- no prefetch in the product build.
#ifndef MVSIM_ROTFFT_PREFETCH
#define MVSIM_ROTFFT_PREFETCH 0
#endif

// Dynamic LDS of both kernels, G batches per transform round (the role-split kernel: G = 1):
// [2][G * U][M + 1] round buffers, [M] plan twiddles, [M + 1] post-processing twiddles (each rounded up to 2 float2: the
// geometry table behind them is 16-byte aligned), the geometry and class tables of a chunk (rotate_dev.h), the row masks
// [2][G][16 waves] (bit u set = the wave's 64 columns of row u of that batch hold a non-zero value), the plane flag's word (of 4),
// the plane's Ny data bits of the row-bit record (row_bits.h: ROW_BITS_MAX_WORDS words, bit y = row y was stored)
constexpr size_t rot_fftx_lds_bytes(int M, int G)
{
    return (size_t)(2 * G * UF * (M + 1) + M + (M & 1) + (M + 1) + ((M + 1) & 1)) * sizeof(float2) + (size_t)geo_chunk_f(G) * sizeof(RowGeo) +
           (size_t)(geo_chunk_f(G) / UF) * sizeof(int) + (size_t)(2 * G * 16 + 4 + ROW_BITS_MAX_WORDS) * sizeof(unsigned int);
}

// Plane order.  Consecutive block ids go to different XCDs (round-robin dispatch, for speed only) and planes z, z + 1 read
// the same source rows, so every XCD gets contiguous runs of planes -- TWO runs half a volume apart: the work of a plane
// follows its content (empty rows skip the fp64 blends and the transforms), all blocks are resident at once (two per
// CU), and a specimen in the middle of the volume would otherwise put all the dense planes on two XCDs
// (measured 0.40 -> 0.36 ms at 512^3 on the sphere phantom).
// -> the plane's index in this launch (rows of `dst`, planes of rot_out / att_out, plane_nz); the plane of the rotated volume is
// z_first + that index -- a z slab of a tiled view (mvsim_view_slab_*: planes z_first .. z_first + nzl - 1) computes its own planes only
__device__ __forceinline__ int rot_fftx_plane()
{
    const int slab = (gridDim.x + 7) / 8;
    const int hs = slab / 2, jb = (int)(blockIdx.x / 8u), kb = (int)(blockIdx.x % 8u);
    return (hs > 0 && slab == 2 * hs) ? ((jb < hs) ? kb * hs + jb : (int)gridDim.x / 2 + kb * hs + (jb - hs)) : kb * slab + jb;
}

// What a lane of a walking wave knows about its column x of plane zl.
struct WalkLane {
    int       x;
    bool      active;              // x < nx: the other lanes walk along (barriers, ballots) and store nothing
    unsigned  xoff;                // the column's byte offset within a row; lanes beyond nx read the last column
    long long row, plane;          // voxels per row, per plane
    long long out_plane;           // the plane's first voxel in rot_out / att_out
    // where the lane's value goes in the padded row besides position x: its mirror image right of the row, its mirror image at
    // the end of the padded row (one reflection each: kx <= nx is guaranteed by the launcher; -1: none); the zero gap between them
    int       pos_r, pos_l, gap_lo, gap_len;
};

__device__ __forceinline__ WalkLane walk_lane(const RotFftArgs& p, int x, int zl, int Px)
{
    WalkLane L;
    const int nx = p.nx;
    L.x = x;
    L.active = x < nx;
    L.xoff = (unsigned)(L.active ? x : nx - 1) * 4u;
    L.row = (long long)nx;
    L.plane = L.row * p.ny;
    L.out_plane = L.plane * zl;
    L.pos_r = (L.active && x >= nx - 1 - p.halo_r && x <= nx - 2) ? 2 * nx - 2 - x : -1;
    L.pos_l = (L.active && x >= 1 && x <= p.halo_l) ? Px - x : -1;
    L.gap_lo = nx + p.halo_r;
    L.gap_len = Px - p.halo_l - L.gap_lo;
    return L;
}

// row y of the plane's values through byte addresses: a scalar base plus the lane's constant offset
__device__ __forceinline__ void store_rot_att(const RotFftArgs& p, const WalkLane& L, int y, float r, float att)
{
    const long long ob = (L.out_plane + (long long)y * L.row) * 4;
    if (p.rot_out) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.rot_out) + ob + L.xoff) = r;
    if (p.att_out) *reinterpret_cast<float*>(reinterpret_cast<char*>(p.att_out) + ob + L.xoff) = att;
}

// A class-0 batch, rows y0, y0 - 1, ...: four zero taps per row: rot = +0, the attenuation state is unchanged, att = +0
template <int U>
__device__ __forceinline__ void store_zero_batch(const RotFftArgs& p, const WalkLane& L, int y0)
{
    if (L.active) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long o = L.out_plane + (long long)(y0 - u) * L.row;
            if (p.rot_out) p.rot_out[o + L.x] = 0.f;
            if (p.att_out) p.att_out[o + L.x] = 0.f;
        }
    }
}

// One row (y) of a class-1 batch from its four loaded taps -> the attenuated value.
template <bool WRITE_OUT>
__device__ __forceinline__ float walk_row_loaded(const RotFftArgs& p, const WalkLane& L, const RowGeo& g, int y, float v00, float v10,
                                                 float v11, float v01, double& n)
{
#ifdef MVSIM_EXP_ROTFFT_NOBLEND
    const unsigned bits = 0u;
#else
    const unsigned bits = __float_as_uint(v00) | __float_as_uint(v10) | __float_as_uint(v11) | __float_as_uint(v01);
#endif
    // four zero taps in EVERY lane of the wave (empty space): rot = +0, the attenuation state does not move
    // (n - 0 delta n = n), att = +0 -- what the arithmetic below gives, without the fp64 blends.  Wave-uniform.
    if (__builtin_amdgcn_ballot_w64((bits << 1) != 0u) == 0ull) {
        if (WRITE_OUT && L.active) store_rot_att(p, L, y, 0.f, 0.f);
        return 0.f;
    }
    const float r = blend4(v00, v10, v11, v01, g);
    const float att = attenuate_step(n, r, p.delta);
    if (WRITE_OUT && L.active) store_rot_att(p, L, y, r, att);
    return att;
}

// One row (y) of a mixed batch, every tap under the mask of the row's kind -> the attenuated value.
template <bool WRITE_OUT>
__device__ __forceinline__ float walk_row_masked(const RotFftArgs& p, const WalkLane& L, const RowGeo& g, int y, double& n)
{
    const int kind = __builtin_amdgcn_readfirstlane(g.kind);
    const long long o = L.out_plane + (long long)y * L.row;
    float r = 0.f, att = 0.f;
    if (kind != 0) {
        float a00, a10, a11, a01;
        load_taps_masked(p.in, g, kind, L.active, L.x, L.row, L.plane, a00, a10, a11, a01);
        r = blend4(a00, a10, a11, a01, g);
        att = attenuate_step(n, r, p.delta);
    }
    if (WRITE_OUT && L.active) {
        if (p.rot_out) p.rot_out[o + L.x] = r;
        if (p.att_out) p.att_out[o + L.x] = att;
    }
    return att;
}

// bit u set = the calling wave's columns of row u of the batch hold a non-zero value
template <int U>
__device__ __forceinline__ unsigned int batch_rowmask(const WalkLane& L, const float (&val)[U])
{
    unsigned int rowmask = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (__builtin_amdgcn_ballot_w64(L.active && (__float_as_uint(val[u]) << 1) != 0u) != 0ull) rowmask |= 1u << u;
    return rowmask;
}

// the batch's rows into a round buffer (rows of LP float2) as the padded real rows pass A would read: position x, the two
// mirror images, the gap (shared by the `nthreads` walking threads)
template <int U>
__device__ __forceinline__ void write_batch_rows(float* __restrict__ rb, int LP, const WalkLane& L, const float (&val)[U], int nthreads)
{
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float* __restrict__ rr = rb + (size_t)u * 2 * LP;
        if (L.active) rr[L.x] = val[u];
        if (L.pos_r >= 0) rr[L.pos_r] = val[u];
        if (L.pos_l >= 0) rr[L.pos_l] = val[u];
        for (int gpos = L.x; gpos < L.gap_len; gpos += nthreads) rr[L.gap_lo + gpos] = 0.f;
    }
}

// row yy of the rows the reference never visits (Ny > Nx): the attenuated image stays zero there; rot still has its values
template <bool WRITE_OUT>
__device__ __forceinline__ void store_unvisited_row(const RotFftArgs& p, const WalkLane& L, int yy, double l2)
{
    if (WRITE_OUT && L.active) {
        if (p.att_out) p.att_out[L.out_plane + (long long)yy * L.row + L.x] = 0.f;
        if (p.rot_out) p.rot_out[L.out_plane + (long long)yy * L.row + L.x] = rot_value(p.in, p.a, L.x, yy, l2, p.nx, p.ny, p.nz);
    }
}

__device__ __forceinline__ float2* spectrum_row(const RotFftArgs& p, int zl, int y) { return p.dst + ((long long)zl * p.py + y) * p.hxp; }

// one transformed row (M complex values in wbuf) -> its half spectrum in drow: k_fft_x_r2c's post-processing
template <int M>
__device__ __forceinline__ void rot_post_store(const float2* wbuf, const float2* twx_l, float2* __restrict__ drow, int hxp, int lane)
{
    constexpr int HQ = M / 4;
#pragma unroll 1
    for (int q = lane; q < HQ; q += 64) {
        float2 lo[2], hi[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * q + h;
            const float2 zk = wbuf[k];
            const float2 zm = cconj(wbuf[k == 0 ? 0 : M - k]);
            const float2 sm = cadd(zk, zm), d = csub(zk, zm);
            const float2 wd = cmul(twx_l[k], d);
            const float2 t = make_float2(wd.y, -wd.x);
            lo[h] = cadd(sm, t);
            hi[h] = cconj(csub(sm, t));
        }
        *reinterpret_cast<float4*>(drow + 2 * q) = make_float4(lo[0].x, lo[0].y, lo[1].x, lo[1].y);
        *reinterpret_cast<Pair16*>(drow + M - 2 * q - 1) = Pair16{hi[1].x, hi[1].y, hi[0].x, hi[0].y};
    }
    const int nmid = M - 4 * HQ + 1;
    const int ntail = nmid + (hxp - M - 1);
    for (int u = lane; u < ntail; u += 64) {
        if (u < nmid) {
            const int k = 2 * HQ + u;
            const float2 zk = wbuf[k == M ? 0 : k];
            const float2 zm = cconj(wbuf[k == 0 ? 0 : M - k]);
            const float2 sm = cadd(zk, zm), d = csub(zk, zm);
            const float2 wd = cmul(twx_l[k], d);
            drow[k] = cadd(sm, make_float2(wd.y, -wd.x));
        } else {
            drow[M + 1 + (u - nmid)] = make_float2(0.f, 0.f);
        }
    }
}

// Row y of the plane, owned by the calling wave: transform, post-process to the half spectrum, store.  A row without a single
// non-zero voxel (everything outside the specimen: well over half the rows of a sphere phantom) has the zero spectrum: no
// transform, sixteen-byte zero stores.  Exact, not an approximation.
// With the row-bit record (p.rowbits; `dbits`: the block's data bits in LDS) a stored row sets its bit and a zero row stores NOTHING:
// pass B reads the bits instead of the zeros.
template <class PLAN>
__device__ __forceinline__ void spectrum_row_store(const RotFftArgs& p, int zl, int y, bool nonzero, float2* wbuf, const float2* tw,
                                                   const float2* twx_l, int lane, unsigned int* dbits)
{
    if (nonzero) {
        PLAN::template run<1>(wbuf, tw, lane);
        rot_post_store<PLAN::len>(wbuf, twx_l, spectrum_row(p, zl, y), p.hxp, lane);
        if (p.rowbits && lane == 0) atomicOr(dbits + (y >> 5), 1u << (y & 31));
    } else if (!p.rowbits) {
        float4* __restrict__ drow = reinterpret_cast<float4*>(spectrum_row(p, zl, y));
        for (int i = lane; i < p.hxp / 2; i += 64) drow[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// G: batches of U rows per transform round.  One wave transforms one row, so a block of up to 8 waves transforms after every
// batch (G = 1); a 16-wave block (rows of 513 .. 1024 voxels) collects two batches first (G = 2), or half its waves would
// sit out every transform.
template <class PLAN, bool WRITE_OUT, int G>
__global__ __launch_bounds__(1024) void k_rotate_attenuate_fftx(RotFftArgs p)
{
    constexpr int M = PLAN::len, LP = M + 1, U = UF, GEO_CHUNK_F = geo_chunk_f(G);
    extern __shared__ __align__(16) float2 lds[];                 // rot_fftx_lds_bytes
    float2* rowbuf = lds;
    float2* tw = lds + 2 * G * U * LP;
    float2* twx_l = tw + M + (M & 1);
    RowGeo* geo = reinterpret_cast<RowGeo*>(twx_l + (M + 1) + ((M + 1) & 1));
    int* bclass = reinterpret_cast<int*>(geo + GEO_CHUNK_F);
    unsigned int* wmask = reinterpret_cast<unsigned int*>(bclass + GEO_CHUNK_F / U);
    unsigned int* dbits = wmask + 2 * G * 16 + 4;                 // the rows of the plane that were stored, bit y
    const int ny = p.ny, steps = p.steps;
    const int x = threadIdx.x;
    const int lane = x & 63, wave = __builtin_amdgcn_readfirstlane(x >> 6), nwaves = (int)blockDim.x >> 6;
    const int zl = rot_fftx_plane();
    if (zl >= p.nzl) return;                                      // whole block: uniform
    if (x < ROW_BITS_MAX_WORDS) dbits[x] = 0u;                    // (in front of the chunk loop's first barrier)
    const double l2 = (double)(p.z_first + zl);
    const WalkLane L = walk_lane(p, x, zl, 2 * M);
    const char* __restrict__ in_b = reinterpret_cast<const char*>(p.in);
    const long long row_b = L.row * 4, plane_b = L.plane * 4;
    for (int i = x; i < M; i += (int)blockDim.x) tw[i] = p.twg[i];
    for (int i = x; i <= M; i += (int)blockDim.x) twx_l[i] = p.twx[i];

    double n = 1.0;
    unsigned int plane_any = 0u;                                  // this wave's columns: any non-zero attenuated value in the plane so far
    int buf = 0;
    int fill = 0;                                                 // batches waiting in the current round buffer (block-uniform)
    int ysub[G], nsub[G];                                         // first row (y) and row count of each of them
    // one barrier per round: the rows are complete; every wave transforms its share; the other buffer takes the next round
    // (a wave reaches the NEXT round's barrier only after its transforms of this one, so two buffers suffice)
    auto flush_round = [&]() {
        // LDS-only barrier: __syncthreads() is a workgroup-scope fence as well and drains vmcnt, i.e. it would wait for every
        // global store of the previous round's spectra (and for the next batch's rows, were they requested ahead) before the
        // waves may meet.  What the round hands over travels through LDS alone: the wave's own ds_writes are complete
        // (lgkmcnt(0)), then the barrier; global loads and stores stay in flight across it.
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        for (int j = wave; j < fill * U; j += nwaves) {
            const int sub = j / U, u = j - sub * U;
            if (u < nsub[sub]) {
                unsigned int any = 0u;
                for (int w = 0; w < nwaves; ++w) any |= wmask[(buf * G + sub) * 16 + w];
#ifdef MVSIM_EXP_ROTFFT_NOFFT
                any = 0u;
#endif
                spectrum_row_store<PLAN>(p, zl, ysub[sub] - u, (__builtin_amdgcn_readfirstlane(any) >> u) & 1u,
                                         rowbuf + (((size_t)buf * G + sub) * U + u) * LP, tw, twx_l, lane, dbits);
            }
        }
        buf ^= 1;
        fill = 0;
    };
    float pv00[U], pv10[U], pv11[U], pv01[U];                     // source rows of a class-1 batch (see issue_loads)
    bool have_pref = false;                                       // block-uniform
    // straight-line loads of a batch whose rows all have their four taps inside the volume
    constexpr int UPRE = MVSIM_ROTFFT_PREFETCH;                  // rows of the next batch requested ahead (registers are the limit)
    auto issue_loads = [&](int r0n, auto lo_c, auto hi_c) {
#pragma unroll
        for (int u = decltype(lo_c)::value; u < decltype(hi_c)::value; ++u)
            issue_row_loads(in_b, geo[r0n + u].off00, row_b, plane_b, L.xoff, pv00[u], pv10[u], pv11[u], pv01[u]);
    };
    for (int c0 = 0; c0 < steps; c0 += GEO_CHUNK_F) {
        const int cnt = min(GEO_CHUNK_F, steps - c0);
        __syncthreads();                                          // the previous chunk's readers are done (and tw is staged)
        fill_row_tables<U>(geo, bclass, p.a, l2, ny, p.nz, L.row, c0, cnt, x, (int)blockDim.x);
        __syncthreads();
        have_pref = false;
        for (int r0 = 0; r0 < cnt; r0 += U) {
            const int cls = __builtin_amdgcn_readfirstlane(bclass[r0 / U]);
            const int y0 = ny - 1 - (c0 + r0);                    // rows y0, y0 - 1, ..., y0 - U + 1
            const int nrows = min(U, cnt - r0);
            if (cls == 0) {
                if (WRITE_OUT) store_zero_batch<U>(p, L, y0);
                for (int j = wave; j < U; j += nwaves) spectrum_row_store<PLAN>(p, zl, y0 - j, false, nullptr, tw, twx_l, lane, dbits);   // zero rows, zero spectra
                continue;
            }
            float val[U];
            if (cls == 1) {
                // the batch's 4 U source rows: already in flight when the previous batch asked for them before its transforms
                if (!have_pref) issue_loads(r0, std::integral_constant<int, 0>{}, std::integral_constant<int, UPRE>{});
                issue_loads(r0, std::integral_constant<int, UPRE>{}, std::integral_constant<int, U>{});
#pragma unroll
                for (int u = 0; u < U; ++u) val[u] = walk_row_loaded<WRITE_OUT>(p, L, geo[r0 + u], y0 - u, pv00[u], pv10[u], pv11[u], pv01[u], n);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) val[u] = u < nrows ? walk_row_masked<WRITE_OUT>(p, L, geo[r0 + u], y0 - u, n) : 0.f;
            }
            const unsigned int rowmask = batch_rowmask<U>(L, val);
            if (lane == 0) wmask[(buf * G + fill) * 16 + wave] = rowmask;
            plane_any |= rowmask;
            write_batch_rows<U>(reinterpret_cast<float*>(rowbuf + ((size_t)buf * G + fill) * U * LP), LP, L, val, (int)blockDim.x);
            ysub[fill] = y0;
            nsub[fill] = nrows;
            fill += 1;
            // the next batch's rows are requested BEFORE this batch's transforms: their latency hides behind the FFTs
            have_pref = r0 + U < cnt && __builtin_amdgcn_readfirstlane(bclass[r0 / U + 1]) == 1;
            if (have_pref) issue_loads(r0 + U, std::integral_constant<int, 0>{}, std::integral_constant<int, UPRE>{});
            if (fill == G) flush_round();
        }
        if (fill > 0) flush_round();                              // before the geometry table (and with it nothing the round needs) moves on
    }
    // The row-bit record: every stored row's bit is in LDS once the block has met -- at an LDS-only barrier that every wave reaches
    // whatever its plane holds (p.rowbits is a kernel argument); one wave expands the Ny bits and stores the record
    if (p.rowbits) {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (wave == 0) write_row_bits(dbits, p.rowbits + (long long)zl * row_bits_words(p.py), ny, p.ky, p.py, lane);
    }
    // Planes that stay empty (a specimen in empty space: a third of the planes of the sphere phantom) need no convolution passes at
    // all: their spectrum is exactly zero.  The passes skip what these flags call empty (custom_fft_convolve_slab, ConvTail::plane_nz).
    if (p.plane_nz) write_plane_flag(wmask + 2 * G * 16, plane_any, x, lane, p.plane_nz + zl);
    for (int yy = ny - 1 - steps; yy >= 0; --yy) {
        store_unvisited_row<WRITE_OUT>(p, L, yy, l2);
        if ((ny - 1 - steps - yy) % nwaves == wave) spectrum_row_store<PLAN>(p, zl, yy, false, nullptr, tw, twx_l, lane, dbits);
    }
}

// ---------------------------------------------------------------------------------- walkers and transformers
// The same kernel with its waves split by role, for rows of up to 512 voxels.  W = ceil(nx / 64) WALKER waves do what every
// wave above does up to the LDS row write (table, loads, zero test, blends, recurrence, rot / att stores, row masks) and never
// transform; ROLE_T extra TRANSFORMER waves own every store into the spectrum: the transforms of the non-zero rows (each wave
// takes U / ROLE_T adjacent rows of a round, one after the other) and the zero rows.  The hand-over is the one above: two
// round buffers, one LDS-only barrier per round that every wave of the block executes; after barrier r the transformers read
// buffer r % 2 while the walkers fill the other one.  Nobody polls anything.  Both roles take the rounds from rot_rounds_next
// (rotate_rounds.h), which sees block-uniform data only, so they meet at the same barriers by construction.
// A round lasts as long as the slower role.  Two transformers (four rows each per round) are slower than the walkers and the
// kernel with them (0.42 ms at 512^3 against 0.36 for the kernel above); four keep up (0.33), and ahead of the walkers on
// their SIMD (s_setprio 1: 0.305; 2 and 3 the same) -- profiles/rotate_roles_ab.txt.  Rows through the plan's multi-row form
// (two per call) need more registers than the budget has and lose (0.44).
// Registers: two blocks per CU must stay resident, i.e. (8 + ROLE_T) / 2 waves per SIMD -- 80 VGPRs with four transformers.
// What held 113 in the kernel above was the chunk loop around the batch loop, not the batch: see the kernel body.
#ifndef MVSIM_ROTFFT_ROLE_WAVES
#define MVSIM_ROTFFT_ROLE_WAVES 4
#endif
constexpr int ROLE_T = MVSIM_ROTFFT_ROLE_WAVES;
static_assert(ROLE_T == 2 || ROLE_T == 4, "transformer waves per block");
static_assert(UF == ROT_ROUND_ROWS && UF % ROLE_T == 0, "round geometry");
// half lengths the role-split kernel is instantiated for: what rows of up to 512 voxels reach with PSFs of up to 64 taps
constexpr bool rot_fftx_roles_len_ok(int len) { return rot_fftx_len_ok(len) && len <= 288; }

template <class PLAN, bool WRITE_OUT, int T>
__global__ __launch_bounds__((8 + T) * 64, (8 + T) / 2) void k_rotate_attenuate_fftx_roles(RotFftArgs p)
{
    constexpr int M = PLAN::len, LP = M + 1, U = UF, GEO_CHUNK_F = geo_chunk_f(1), RW = rot_round_group(T);
    extern __shared__ __align__(16) float2 lds[];                 // rot_fftx_lds_bytes(M, 1): the layout of the G = 1 instance above
    float2* rowbuf = lds;
    float2* tw = lds + 2 * U * LP;
    float2* twx_l = tw + M + (M & 1);
    RowGeo* geo = reinterpret_cast<RowGeo*>(twx_l + (M + 1) + ((M + 1) & 1));
    int* bclass = reinterpret_cast<int*>(geo + GEO_CHUNK_F);
    unsigned int* wmask = reinterpret_cast<unsigned int*>(bclass + GEO_CHUNK_F / U);
    unsigned int* dbits = wmask + 2 * 16 + 4;                     // the rows of the plane that were stored, bit y
    const int ny = p.ny, steps = p.steps;
    const int x = threadIdx.x;
    const int lane = x & 63, wave = __builtin_amdgcn_readfirstlane(x >> 6);
    const int nwalk = ((int)blockDim.x >> 6) - T, walk_threads = nwalk * 64;
    const bool walker = wave < nwalk;                             // wave-uniform: a scalar branch
    const int tr = wave - nwalk;                                  // which transformer (walkers: negative)
    const int zl = rot_fftx_plane();
    if (zl >= p.nzl) return;                                      // whole block: uniform
    if (x < ROW_BITS_MAX_WORDS) dbits[x] = 0u;                    // (in front of the barriers around the table fill)
    const double l2 = (double)(p.z_first + zl);
    const WalkLane L = walk_lane(p, x, zl, 2 * M);                // (transformer lanes: x >= 64 nwalk >= nx, never active)
    const char* __restrict__ in_b = reinterpret_cast<const char*>(p.in);
    // the lane's four taps of a row as 32-bit byte offsets against the row's scalar base (the launcher checks the range)
    const unsigned o10 = L.xoff + (unsigned)(L.row * 4), o01 = L.xoff + (unsigned)(L.plane * 4), o11 = o10 + (unsigned)(L.plane * 4);
    for (int i = x; i < M; i += (int)blockDim.x) tw[i] = p.twg[i];
    for (int i = x; i <= M; i += (int)blockDim.x) twx_l[i] = p.twx[i];

    // the round barrier of k_rotate_attenuate_fftx: LDS only, global loads and stores stay in flight across it
    auto round_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    auto cls_of = [&](int b) { return __builtin_amdgcn_readfirstlane(bclass[b]); };

    double n = 1.0;
    unsigned int plane_any = 0u;
    // ONE geometry chunk: the launcher takes this instance for walks of up to GEO_CHUNK_F rows only (steps = nx <= 512), and the
    // walker's state -- the attenuation, the loads in flight -- is then not alive across a chunk loop around both roles' code
    // (four transformers, 80-VGPR budget: with that loop 92 .. 104 bytes of scratch per lane, without it 75 .. 80 VGPRs and none)
    const int cnt = steps;
    __syncthreads();                                              // tw and twx_l are staged
    fill_row_tables<U>(geo, bclass, p.a, l2, ny, p.nz, L.row, 0, cnt, x, (int)blockDim.x);
    __syncthreads();
    RotRounds rounds = rot_rounds_begin(cnt, 0);
    RotBatch b;
    if (!walker) {
        // ------------------------------------------------------------------ transformer: everything that writes the spectrum
        __builtin_amdgcn_s_setprio(1);                        // ahead of the walkers: the round waits for the slower role
        while (rot_rounds_next(rounds, cls_of, b)) {
            const int y0 = ny - 1 - b.r0;
            if (b.cls == 0) {
                for (int j = tr; j < U; j += T) spectrum_row_store<PLAN>(p, zl, y0 - j, false, nullptr, tw, twx_l, lane, dbits);
                continue;
            }
            round_barrier();                                  // round b.buf is complete
            unsigned int any = 0u;
            for (int w = 0; w < nwalk; ++w) any |= wmask[b.buf * 16 + w];
#ifdef MVSIM_EXP_ROTFFT_NOFFT
            any = 0u;
#endif
            any = __builtin_amdgcn_readfirstlane(any);
            // this wave's RW adjacent rows
#pragma unroll 1
            for (int u = tr * RW; u < (tr + 1) * RW && u < b.nrows; ++u)
                spectrum_row_store<PLAN>(p, zl, y0 - u, (any >> u) & 1u, rowbuf + ((size_t)b.buf * U + u) * LP, tw, twx_l, lane, dbits);
        }
    } else {
        // ------------------------------------------------------------------ walker: one batch, one round buffer, one barrier
        while (rot_rounds_next(rounds, cls_of, b)) {
            const int r0 = b.r0, y0 = ny - 1 - r0;
            if (b.cls == 0) {
                if (WRITE_OUT) store_zero_batch<U>(p, L, y0);
                continue;
            }
            float val[U];
            if (b.cls == 1) {
                // straight-line loads of the batch's 4 U source rows
                float pv00[U], pv10[U], pv11[U], pv01[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const char* __restrict__ p00 = scalar_row_base(in_b, geo[r0 + u].off00);
                    pv00[u] = *reinterpret_cast<const float*>(p00 + L.xoff);
                    pv10[u] = *reinterpret_cast<const float*>(p00 + o10);
                    pv11[u] = *reinterpret_cast<const float*>(p00 + o11);
                    pv01[u] = *reinterpret_cast<const float*>(p00 + o01);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) val[u] = walk_row_loaded<WRITE_OUT>(p, L, geo[r0 + u], y0 - u, pv00[u], pv10[u], pv11[u], pv01[u], n);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) val[u] = u < b.nrows ? walk_row_masked<WRITE_OUT>(p, L, geo[r0 + u], y0 - u, n) : 0.f;
            }
            const unsigned int rowmask = batch_rowmask<U>(L, val);
            if (lane == 0) wmask[b.buf * 16 + wave] = rowmask;
            plane_any |= rowmask;
            write_batch_rows<U>(reinterpret_cast<float*>(rowbuf + (size_t)b.buf * U * LP), LP, L, val, walk_threads);
            round_barrier();                                  // hands buffer b.buf to the transformers
        }
    }
    // The row-bit record: the transformers have ORed the bits of the rows they stored into LDS.  The block meets ONCE MORE, at an
    // LDS-only barrier outside the enumeration of rot_rounds_next, which every wave of both roles reaches whatever its plane holds
    // (p.rowbits is a kernel argument: the number of barriers stays a function of block-uniform data only); one wave expands the Ny
    // bits and stores the record
    if (p.rowbits) {
        round_barrier();
        if (wave == 0) write_row_bits(dbits, p.rowbits + (long long)zl * row_bits_words(p.py), ny, p.ky, p.py, lane);
    }
    if (p.plane_nz) write_plane_flag(wmask + 2 * 16, plane_any, x, lane, p.plane_nz + zl);   // the walkers know; every wave meets at the barriers
    // the rows the reference never visits: zero spectra are the transformers'
    for (int yy = ny - 1 - steps; yy >= 0; --yy) {
        store_unvisited_row<WRITE_OUT>(p, L, yy, l2);
        if (!walker && (ny - 1 - steps - yy) % T == tr) spectrum_row_store<PLAN>(p, zl, yy, false, nullptr, tw, twx_l, lane, dbits);
    }
}

template <class PLAN>
static int launch_rot_fftx_t(mvsim_ctx* ctx, const RotFftArgs& a, bool write_out, bool roles)
{
    constexpr int M = PLAN::len;
    const int waves = (a.nx + 63) / 64;
    const int G = waves > 8 ? 2 : 1;
    if constexpr (rot_fftx_roles_len_ok(M)) {
        // walkers + transformers: rows of up to 512 voxels whose four taps lie within 32-bit byte offsets of a row's base
        if (roles && waves <= 8 && a.steps <= geo_chunk_f(1) && ((int64_t)a.nx * a.ny + 2 * (int64_t)a.nx) * 4 < (int64_t)1 << 32) {
            const size_t lds = rot_fftx_lds_bytes(M, 1);
            dim3 grid((unsigned)((a.nzl + 7) / 8 * 8)), block((unsigned)((waves + ROLE_T) * 64));
            if (write_out) {
                MVSIM_TRY(ensure_lds_attr(ctx, reinterpret_cast<const void*>(k_rotate_attenuate_fftx_roles<PLAN, true, ROLE_T>), lds));
                hipLaunchKernelGGL((k_rotate_attenuate_fftx_roles<PLAN, true, ROLE_T>), grid, block, lds, ctx->stream, a);
            } else {
                MVSIM_TRY(ensure_lds_attr(ctx, reinterpret_cast<const void*>(k_rotate_attenuate_fftx_roles<PLAN, false, ROLE_T>), lds));
                hipLaunchKernelGGL((k_rotate_attenuate_fftx_roles<PLAN, false, ROLE_T>), grid, block, lds, ctx->stream, a);
            }
            MVSIM_HIP(hipGetLastError());
            return MVSIM_OK;
        }
    }
    const size_t lds = rot_fftx_lds_bytes(M, G);
    if (lds > 160 * 1024) { set_error("fused rotate + x transform: %zu bytes of LDS", lds); return MVSIM_EINVAL; }
    dim3 grid((unsigned)((a.nzl + 7) / 8 * 8)), block((unsigned)(waves * 64));
#define MVSIM_RF(W_, G_)                                                                                            \
    do {                                                                                                            \
        MVSIM_TRY(ensure_lds_attr(ctx, reinterpret_cast<const void*>(k_rotate_attenuate_fftx<PLAN, W_, G_>), lds)); \
        hipLaunchKernelGGL((k_rotate_attenuate_fftx<PLAN, W_, G_>), grid, block, lds, ctx->stream, a);              \
    } while (0)
    if constexpr (M >= 280) {                                     // rows of more than 512 voxels: padded half length >= 280
        if (G == 2) {
            if (write_out) MVSIM_RF(true, 2); else MVSIM_RF(false, 2);
            MVSIM_HIP(hipGetLastError());
            return MVSIM_OK;
        }
    }
    if (G == 2) { set_error("fused rotate + x transform: no 16-wave instance for half length %d", M); return MVSIM_EINVAL; }
    if (write_out) MVSIM_RF(true, 1); else MVSIM_RF(false, 1);
#undef MVSIM_RF
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

template <int LL, int... Rs>
static int launch_rot_fftx_pick(mvsim_ctx* ctx, const RotFftArgs& a, bool write_out, bool roles)
{
    if constexpr (rot_fftx_len_ok(LL)) return launch_rot_fftx_t<Plan<LL, Rs...>>(ctx, a, write_out, roles);
    set_error("fused rotate + x transform: half length %d is not instantiated", LL);
    return MVSIM_EINVAL;
}

int launch_rot_fftx(mvsim_ctx* ctx, int M, const RotFftArgs& a, bool write_out, bool roles)
{
    switch (M) {
#define X(LL, ...) case LL: return launch_rot_fftx_pick<LL, __VA_ARGS__>(ctx, a, write_out, roles);
        MVSIM_FFT_SIZES(X)
#undef X
    }
    set_error("fused rotate + x transform: no plan for half length %d", M);
    return MVSIM_EINVAL;
}

}  // namespace fft
}  // namespace mvsim
