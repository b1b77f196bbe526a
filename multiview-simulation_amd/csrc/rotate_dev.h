// The ONE statement of the arithmetic of rotateAroundAxis about x followed by attenuate3d
// (SimulateMultiViewDataset.java:104-135, 318-364), as every rotate kernel walks it: rotate.hip and rotate_fft.hip.
//
// The inverse model of a rotation about x has row 0 = (1, 0, 0, 0) exactly (affine_is_x_rotation), so the output row (y, z)
// reads four source rows at the same x with weights that do not depend on x.  The written evaluation order IS the contract
// (the build has -ffp-contract=off): `0.0 * m[4] + l1 * m[5] + l2 * m[6] + m[7]` (l0 * m4 with m4 == 0 contributes +0 exactly),
// the `1.0 * w1n * w2n` weights of ImgLib2's NLinearInterpolator in double, every tap rounded (float)(v * w), float
// accumulation in Gray-code tap order 00, 10, 11, 01, and the fp64 recurrence n = max(n - v delta n, 0), out = (float)(v n).
// Nothing here may be simplified.  The header compiles for the device and for a plain host compiler
// (tests/c_abi/row_geometry_main.cpp runs it against the oracle on the CPU).
#pragma once

#include <math.h>

#include "row_bits.h"

#if defined(__HIPCC__)
#define MVSIM_ROT_FN __host__ __device__ __forceinline__
#else
#define MVSIM_ROT_FN inline __attribute__((always_inline))
#endif

namespace mvsim {

struct Affine {
    double m[12];
};

// The geometry of an output row (yy, z): the same for every x of the row.
struct __attribute__((aligned(16))) RowGeo {
    double    w00, w10, w11, w01;
    long long off00;            // byte offset of source row (sy, sz), x = 0; only meaningful for the taps that are inside
    int       kind;             // low byte: 0 none, 1 all four taps inside, 2 partial; bits 8..11 = inside(00, 10, 11, 01)
    int       pad;
};

// l2 = (double)z; row = nx as a 64-bit count of voxels
MVSIM_ROT_FN RowGeo row_geometry(const Affine& a, int yy, double l2, int ny, int nz, long long row)
{
    const double l1 = (double)yy;
    const double py = 0.0 * a.m[4] + l1 * a.m[5] + l2 * a.m[6] + a.m[7];
    const double pz = 0.0 * a.m[8] + l1 * a.m[9] + l2 * a.m[10] + a.m[11];
    const double fy = floor(py), fz = floor(pz);
    RowGeo g;
    g.w00 = g.w10 = g.w11 = g.w01 = 0.0;
    g.off00 = 0;
    g.kind = 0;
    g.pad = 0;
    // whole 2x2 support outside the volume -> exact zero (also keeps the int casts safe)
    if (fy >= -1.0 && fz >= -1.0 && fy < (double)ny && fz < (double)nz) {
        const int sy = (int)fy, sz = (int)fz;
        const double w1 = py - fy, w2 = pz - fz;
        const double w1n = 1.0 - w1, w2n = 1.0 - w2;
        g.w00 = 1.0 * w1n * w2n; g.w10 = 1.0 * w1 * w2n; g.w11 = 1.0 * w1 * w2; g.w01 = 1.0 * w1n * w2;
        const bool ya = sy >= 0, yb = sy + 1 < ny, za = sz >= 0, zb = sz + 1 < nz;
        g.off00 = row * (sy + (long long)ny * sz) * 4;          // BYTE offset
        const int m = ((ya && za) ? 1 : 0) | ((yb && za) ? 2 : 0) | ((yb && zb) ? 4 : 0) | ((ya && zb) ? 8 : 0);
        g.kind = (m == 15 ? 1 : (m == 0 ? 0 : 2)) | (m << 8);
    }
    return g;
}

// which of the taps 00, 10, 11, 01 of a row of this kind lie inside the volume (tap = 0..3 in that order)
MVSIM_ROT_FN bool tap_inside(int kind, int tap) { return (kind & ((1 << tap) << 8)) != 0; }
// 0, 1 or 2: see RowGeo
MVSIM_ROT_FN int row_class(int kind) { return kind & 0xff; }

MVSIM_ROT_FN float blend4(float v00, float v10, float v11, float v01, const RowGeo& g)
{
    float r = (float)((double)v00 * g.w00);
    r += (float)((double)v10 * g.w10);
    r += (float)((double)v11 * g.w11);
    r += (float)((double)v01 * g.w01);
    return r;
}

// one step of attenuate3d: n is the column's state, r the voxel; returns the attenuated voxel
MVSIM_ROT_FN float attenuate_step(double& n, float r, double delta)
{
    const double d = (double)r;
    n = fmax(n - d * delta * n, 0.0);
    return (float)(d * n);
}

// The four taps of a row at column x, a tap outside the volume (or of a lane that is not `active`) reading as +0.  `kind` is
// g.kind, handed in separately so that a kernel may pass it from a scalar register.  plane = nx * ny voxels.
MVSIM_ROT_FN void load_taps_masked(const float* in, const RowGeo& g, int kind, bool active, int x, long long row, long long plane,
                                   float& a00, float& a10, float& a11, float& a01)
{
    const float* __restrict__ p00 = reinterpret_cast<const float*>(reinterpret_cast<const char*>(in) + g.off00);
    a00 = (active && tap_inside(kind, 0)) ? p00[x] : 0.f;
    a10 = (active && tap_inside(kind, 1)) ? p00[row + x] : 0.f;
    a11 = (active && tap_inside(kind, 2)) ? p00[row + plane + x] : 0.f;
    a01 = (active && tap_inside(kind, 3)) ? p00[plane + x] : 0.f;
}

// The rotated voxel (x, yy, z) from scratch: what the rows the attenuation never visits (Ny > Nx) still need in `rot`.
MVSIM_ROT_FN float rot_value(const float* in, const Affine& a, int x, int yy, double l2, int nx, int ny, int nz)
{
    const long long row = (long long)nx;
    const RowGeo g = row_geometry(a, yy, l2, ny, nz, row);
    float a00, a10, a11, a01;
    load_taps_masked(in, g, g.kind, g.kind != 0, x, row, row * ny, a00, a10, a11, a01);
    return blend4(a00, a10, a11, a01, g);
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------- device only
// The table form of the walk: the threads of a block compute the geometry of `cnt` rows (row r of the chunk is
// yy = ny - 1 - (c0 + r)) once, one row per thread, into an LDS table, then the class of every batch of U rows:
// 1 = all rows have their four taps inside (straight-line code), 0 = all rows are outside (zeros), 2 = mixed or
// incomplete batch (per-tap mask).  The caller brackets the call with its own barriers (the previous chunk's readers are
// done before it; the tables are complete after it).
template <int U>
__device__ __forceinline__ void fill_row_tables(RowGeo* geo, int* bclass, const Affine& a, double l2, int ny, int nz, long long row,
                                                int c0, int cnt, int tid, int nthreads)
{
    for (int r = tid; r < cnt; r += nthreads) geo[r] = row_geometry(a, ny - 1 - (c0 + r), l2, ny, nz, row);
    __syncthreads();
    for (int bq = tid; bq < (cnt + U - 1) / U; bq += nthreads) {
        bool all1 = true, all0 = true;
        for (int u = 0; u < U; ++u) {
            const int r = bq * U + u;
            if (r < cnt) {
                const int k = row_class(geo[r].kind);
                all1 = all1 && k == 1;
                all0 = all0 && k == 0;
            } else {
                all1 = false;
                all0 = false;
            }
        }
        bclass[bq] = all1 ? 1 : (all0 ? 0 : 2);
    }
}

// The address of source row (sy, sz) as a scalar: the table's byte offset comes back through v_readfirstlane, so the row's
// loads use a scalar base and the lane's constant byte offset.
__device__ __forceinline__ const char* scalar_row_base(const char* in_b, long long off00)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)off00);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)off00 >> 32));
    return in_b + (long long)(((unsigned long long)hi << 32) | lo);
}

// The four loads of a row whose taps are all inside (row_b, plane_b: bytes per row and per plane; xoff: the lane's byte
// offset -- lanes beyond nx read the last column, only their stores are masked).
__device__ __forceinline__ void issue_row_loads(const char* in_b, long long off00, long long row_b, long long plane_b, unsigned xoff,
                                                float& v00, float& v10, float& v11, float& v01)
{
    const char* __restrict__ p00 = scalar_row_base(in_b, off00);
    v00 = *reinterpret_cast<const float*>(p00 + xoff);
    v10 = *reinterpret_cast<const float*>(p00 + row_b + xoff);
    v11 = *reinterpret_cast<const float*>(p00 + row_b + plane_b + xoff);
    v01 = *reinterpret_cast<const float*>(p00 + plane_b + xoff);
}

// "does this block's plane hold a non-zero attenuated voxel" into *flag (0 or 1: nothing has to be cleared beforehand).
// plane_any: the calling wave's own finding; blk_any: one LDS word.  Every thread of the block calls.
__device__ __forceinline__ void write_plane_flag(unsigned int* blk_any, unsigned int plane_any, int tid, int lane, int* flag)
{
    __syncthreads();                                          // (also: every earlier reader of the LDS around blk_any is done)
    if (tid == 0) *blk_any = 0u;
    __syncthreads();
    if (lane == 0 && plane_any != 0u) atomicOr(blk_any, 1u);
    __syncthreads();
    if (tid == 0) *flag = (int)*blk_any;
}

// The plane's row-bit record (row_bits.h) from the block's Ny data bits in LDS (`data`: ROW_BITS_MAX_WORDS words; whoever owned a
// stored row has ORed its bit in, and the block has met at a barrier since).  ONE wave calls: 64 padded positions per ballot, two
// words per trip, ordinary vector stores; the whole record on every launch, an empty plane's included.
__device__ __forceinline__ void write_row_bits(const unsigned int* data, unsigned int* __restrict__ rec, int ny, int ky, int py, int lane)
{
    const int words = fft::row_bits_words(py);
    for (int w0 = 0; w0 < words; w0 += 2) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(fft::row_bits_padded_bit(data, 32 * w0 + lane, ny, ky, py));
        if (lane < 2 && w0 + lane < words) rec[w0 + lane] = (unsigned int)(m >> (32 * lane));
    }
}
#endif

}  // namespace mvsim
