// What the translation units of the hand-written FFT convolution share on the host side: the argument structs of their kernels, the
// constants of the spectrum's layout, and the entry points by which the driver (fft_driver.hip) reaches the kernels of fft_passes.hip
// (y / z line transforms and x passes) and zconv.hip (direct z pass).  The device-side building blocks and the one list of
// lengths are fft_dev.h.
#pragma once
#include "fft_dev.h"

namespace mvsim {
struct PItem;               // poisson_dev.h (the fused tail's work items; only fft_passes.hip needs the definition)
namespace fft {

// ---------------------------------------------------------------------------------- y / z line transforms (fft_passes.hip)
// CONVZ: the z pass as FFT -> product -> inverse FFT on a spectrum WITHOUT z padding (the geometry of the direct z pass): the
// mirrored halo planes are read from their mirror images through the index map, and the PSF's z spectrum is never stored --
// every block transforms the Kz taps of its own 16 lines first and keeps the result in registers for the product.
enum Mode { FWD = 0, INV = 1, CONV = 2, CONVZ = 3 };

struct LinesArgs {
    const float2* src;      // element (line c, position n) of tile (bx, by): src[by*src_outer + n'*src_es + bx*NL + c]
    float2*       dst;
    const float2* spec;     // CONV: PSF spectrum, same tiling
    const float2* tw;
    long long     src_es, src_outer, dst_es, dst_outer, spec_es, spec_outer;
    DimMap        lmap;     // SPARSE: position n reads source position map_src(lmap, n) (or zero)
    int           gap_lo, gap_hi;   // positions n in [gap_lo, gap_hi) are structurally zero: not loaded (gap_hi <= gap_lo: none)
    int           outer_skip_lo, outer_skip_len;   // outer index by >= outer_skip_lo is shifted by outer_skip_len (skipped planes)
    int           store_limit;      // > 0: positions n >= store_limit are never read downstream and are not stored
    int           dst_tile_major;   // FWD: store tile (bx,by) as NL contiguous lines of L: dst[((by*gridDim.x+bx)*NL + c)*L + n]
    // z-blocked layout of the spectrum between passes B, C' and D (0: off): position n of a line sits at
    // (n >> ZBS) * blk + (n & (ZB - 1)) * es -- ZB rows of every plane stay together, so that the z pass, which walks the
    // planes of ONE row, finds them ZB * Hxp elements apart instead of a whole plane apart (see line_off)
    long long     src_blk, dst_blk;
    int           src_mirror;       // != 0 (non-SPARSE): position n reads source position map_src(lmap, n) -- the mirrored halo rows
                                    // of the padded image are the rows themselves, read twice instead of transformed twice
    // planes known to be empty (null: none): a block whose outer index names an empty plane has nothing to read and -- because every
    // reader of its output asks the same flags -- nothing to write.  Outer index k = plane k * nz_stride of the flag array
    // (Pass B behind the fused rotate kernel: that kernel may have left the rows without a non-zero voxel UNWRITTEN -- stale bytes of an
    // earlier view.  Whoever reads its output must ask `rowbits` below as well as these flags.)
    const int*    nzflags;
    int           nz_stride;
    // blocked OUTER addressing (0: linear): outer index by sits at (by >> ZBS) * oblk + (by & (ZB - 1)) * outer -- the z-blocked
    // spectrum layout seen from a pass whose lines run along z (CONVZ)
    long long     src_oblk, dst_oblk;
    // CONVZ: the PSF's (x, y) spectrum, Kz planes in the z-blocked layout of the direct z pass (ZConvArgs::taps); pmap embeds tap
    // t at position (t - Kz / 2) mod L; adjustImage's sum from this pass's output as in k_zconv (null: not wanted)
    const float2* taps;
    long long     taps_es, taps_oblk, taps_outer;
    DimMap        pmap;
    const double2* wx;
    const double2* wy;
    double*       sum_partial;
    int           pair_tiles;       // 8-column tiles: the two tiles of a 128-byte line on one XCD (see k_fft_lines; exp bit 4 clears it)
    // FWD, not SPARSE (pass B): the row-bit record of the fused rotate kernel (row_bits.h; null: every row was written).  Outer index
    // `by` finds its plane's bits at rowbits + by * rowbits_stride; position n of the line is loaded iff bit n is set and is +0
    // otherwise -- the rotate kernel has not written that row.  Lengths with row_bits_len_ok only (launch_lines checks).
    const unsigned int* rowbits;
    int           rowbits_stride;
};

#ifndef MVSIM_ZBS
#define MVSIM_ZBS 4
#endif
constexpr int ZBS = MVSIM_ZBS, ZB = 1 << ZBS;        // rows per block of the z-blocked layout
constexpr int NZ_EXT = 96;                          // mirrored planes the flag bit string holds in front of plane 0 (>= Kz - 1 + tap padding)

__device__ __forceinline__ int mirror_index(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// A tile row that is not wanted, loaded all the same from an address that is certainly mapped and cleared to +0 bits: an AND, not a
// select -- a select whose operand is a load is turned back into a branch around the load (zconv.hip; k_fft_lines' masked form)
__device__ __forceinline__ float4 keep4(float4 t, bool keep)
{
    const unsigned int m = keep ? 0xFFFFFFFFu : 0u;
    return make_float4(__uint_as_float(__float_as_uint(t.x) & m), __uint_as_float(__float_as_uint(t.y) & m),
                       __uint_as_float(__float_as_uint(t.z) & m), __uint_as_float(__float_as_uint(t.w) & m));
}

__device__ __forceinline__ long long line_off(int n, long long es, long long blk)
{
    return blk ? (long long)(n >> ZBS) * blk + (long long)(n & (ZB - 1)) * es : (long long)n * es;
}

// ---------------------------------------------------------------------------------- x passes (fft_passes.hip)
// Pass E's fused tail (k_fft_x_c2r<FUSE>): what the epilogue needs to adjust, extract and sample the rows it produces
struct C2RFuse {
    const double* scal;           // scal[1] = adjustImage's factor
    float         min_value;
    float*        con;            // adjusted volume, rows as this pass produces them (null: not wanted)
    float*        acq;            // acquisition [planes][ny][nx]
    int           acq_every;      // plane k of this pass is acquired iff k % acq_every == 0, as acquisition plane k / acq_every
    int           idx_zstride;    // plane k of this pass is plane k * idx_zstride of the source volume (RNG counter)
    int           noise;
    double        mul;
    uint32_t      k0, k1, stream;
    PItem*        queue;          // per-block segments of `segcap` items
    unsigned int* qcount;
    unsigned int  segcap;
};

// planes of pass E's input known to be empty (pass D has not written them): plane k of this pass is plane k * stride of the
// dilated flag array (null: none).  sparse: the mode bit of the sparse tail (ConvTail::sparse) -- the rows of those planes are not
// stored either (k_fft_x_c2r_sparse); 0: they are stored as zeros
struct C2REmpty {
    const int* flags;
    int        stride;
    int        sparse;
};

// ---------------------------------------------------------------------------------- direct z pass (zconv.hip)
// (MVSIM_EXP_NLZ = 32 -- 256-byte rows -- measured 0.35 ms with 160-output tiles, 0.42 ms with 112-output tiles, against 0.32 ms)
#ifndef MVSIM_EXP_NLZ
#define MVSIM_EXP_NLZ 16
#endif
#ifndef MVSIM_ZNIT
#define MVSIM_ZNIT 9
#endif
// tile: NLZ columns, a lane computes ZU consecutive outputs of its line, taps in chunks of ZJ, blocks of ZT threads
constexpr int NLZ = MVSIM_EXP_NLZ, ZU = 16, ZJ = 8, ZT = 256;
constexpr int ZRPI = ZT / (NLZ / 2);             // rows per staging iteration (NLZ / 2 lanes of 16 B per row)
constexpr int ZNIT = MVSIM_ZNIT;                 // staged rows <= ZNIT * ZRPI (zconv_chunk keeps the tile below that)

struct ZConvArgs {
    const float2* src;      // z-blocked (see below)
    float2*       dst;      // z-blocked
    const float2* taps;     // z-blocked as well, Kz planes: (ky >> ZBS) * taps_blk + t * zs + (ky & (ZB-1)) * Hxp + kx
    // src and dst in the z-blocked layout (LinesArgs::src_blk): element (z, ky, kx) at (ky >> ZBS) * blk + z * zs + (ky & (ZB-1)) * Hxp + kx
    long long     src_blk, dst_blk, taps_blk, zs;
    int           hxp, nz, kz, c, zc;   // nz: output planes; zc: outputs per tile along z (multiple of ZU)
    // z-slab tiling: the mirror boundary acts on the GLOBAL plane index; src holds the global planes from z_in0 on,
    // dst plane 0 is global plane z_out0 (whole volume: nz_global = nz, both offsets 0)
    int           nz_global, z_in0, z_out0;
    // adjustImage's sum taken from the spectrum side (null: not wanted).  The sum of the cropped convolved volume is a
    // linear functional of this pass's output: sum = scale * SUM_{z, ky, kx <= M} Re( F[z][ky][kx] * wx[kx] * wy[ky] ) with
    // wx[kx] = c(kx) * SUM_{x < Nx} e^{+2 pi i kx x / Px} (c = 1 for kx = 0 and M, else 2: Hermitian half), wy[ky] alike
    // without c.  One partial (double) per block.
    const double2* wx;
    const double2* wy;
    double*       sum_partial;
    // planes of the input known to be empty (pass B has not even written them; null: none): their rows are not loaded, and a tile
    // whose rows are all empty computes and stores nothing (pass D skips its planes on the same flags)
    // bit i = plane mirror(i - NZ_EXT) is non-empty: the flags as a bit string that already holds the mirrored halo on both sides, so
    // that the planes a tile reaches are ONE run of bits (k_plane_flags_finish); null: every plane is read
    const unsigned int* nzbits;
    // k_zconv_strided only: outputs are the planes k * stride (the compact planes extractSlices reads); LDS rows reserved for the tile
    int           stride, frows;
    // tiles: nch chunks along z x nkxb groups of NLZ columns x py rows, on a 1-D grid (zconv_tile)
    int           nch, nkxb, py, plain_order;
    // stacked views (mvsim_simulate_views_dev; blockIdx.y = view): view v finds its planes, its outputs and the taps of ITS PSF that
    // many elements further on, and its partial sums behind those of the views before it
    long long     src_view, dst_view, taps_view;
};

template <class K> static int set_lds(mvsim_ctx* ctx, K kernel, size_t bytes)
{
    return ensure_lds_attr(ctx, reinterpret_cast<const void*>(kernel), bytes);
}

// ---------------------------------------------------------------------------------- entry points
// fft_passes.hip: lines of L points (a length of MVSIM_FFT_SIZES, else MVSIM_EINVAL) on a grid of tiles x nouter blocks; whether lines of
// 2 LH points can run as two transforms of LH points (k_fft_lines_split is instantiated for LH)
int  launch_lines(mvsim_ctx* ctx, int L, int mode, bool sparse, const LinesArgs& a, int tiles, int nouter);
bool lines_split_exists(int LH);
// ... and passes A and E with the half length M
int  launch_r2c(mvsim_ctx* ctx, int M, const float* src, const SrcMap& map, float2* dst, const float2* tw, const float2* twx, int hxp,
                long long rows);
int  launch_c2r(mvsim_ctx* ctx, int M, const float2* srcc, float* out, const float2* tw, const float2* twx, int hxp, int py, int nx, int ny,
                long long rows, float scale, double* partial, int* nblocks, const C2RFuse* fuse, const C2REmpty& em);
// zconv.hip
int       zconv_chunk(int nz, int kz);
long long zconv_blocks(const ZConvArgs& a, int py, int cols = 0);
int       zconv_strided_chunk(int nz, int kz, int s, bool force, int* frows_out, size_t* lds_out);
int       launch_zconv(mvsim_ctx* ctx, const ZConvArgs& args, int py, int views = 1);
int       launch_zconv_strided(mvsim_ctx* ctx, const ZConvArgs& args, int py, size_t lds, int views = 1);

}  // namespace fft

// fft_driver.hip: the device twiddle table of a length (kind 0: the per-pass table of its plan; kind 1: plain exp(-2 pi i k / L))
int ensure_twiddles(mvsim_ctx* ctx, int L, int kind, const float2** out);

}  // namespace mvsim
