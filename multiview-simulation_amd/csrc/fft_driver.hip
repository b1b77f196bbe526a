// Hand-written LDS-tiled FFT convolution for gfx950 (the production path of
// SimulateMultiViewDataset.convolve, :253-264, for padded sizes of the form 2^a 3^b).
//
// A 3-D real convolution is five streaming passes over one half-spectrum buffer F
// (complex float, [Pz][Py][Hxp], Hxp = Px/2+1 rounded up to the tile width):
//   A  x: mirror-pad on the fly + real->complex FFT along x          read 4N      write C
//   B  y: complex FFT along y, in place                               read C       write C
//   C  z: FFT along z, multiply by the PSF spectrum, inverse FFT z    read C (+G)  write C
//   D  y: inverse FFT along y, in place                               read C       write C
//   E  x: complex->real FFT along x + crop + 1/P^3 + block sums       read C       write 4N
// Each pass stages a tile of NL lines in LDS (line = the FFT axis, contiguous in LDS; NL adjacent
// kx columns = 128 B contiguous in HBM).  Every wave then OWNS whole lines of the tile and runs the
// mixed-radix Stockham passes on them with register butterflies; because LDS operations of one wave
// execute in issue order, the passes need no workgroup barrier at all -- the waves of a block run
// decoupled and hide each other's LDS latency.  Block barriers remain only around the transposed
// staging (and around the spectrum product of pass C).  Twiddles come from a host-computed (double
// precision, rounded once) table staged in LDS.  Inverse transforms use conj(FFT(conj(.))).
//
// This file is the host side: the table of lengths, the plan (conv_plan), the twiddle and weight caches and the driver.  The kernels
// live in fft_passes.hip (the transforms along x, y and z) and zconv.hip (direct z pass) and are reached through fft_host.h.
#include "fft_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace mvsim {
namespace fft {

#ifndef MVSIM_ZINLINE_MIN_KZ
#define MVSIM_ZINLINE_MIN_KZ 48           // measured (profiles/r04_zpass_sweep.txt): see custom_fft_convolve_slab
#endif

// Empty-plane bookkeeping for the convolution passes (one small block per view).  flags[z] = 1 where the fused rotate kernel found a
// non-zero voxel in plane z.  dil[z] = 1 iff any plane the z pass's Kz taps reach from output plane z -- z + c - t, t = 0 .. kz - 1,
// mirror-single at the faces -- is non-empty (passes D and E).  bits: bit i = flags[mirror(i - NZ_EXT)] (pass C').
__global__ __launch_bounds__(1024) void k_plane_flags_finish(const int* __restrict__ flags, int n, int kz, int c, unsigned int* __restrict__ bits,
                                                             int nwords, int* __restrict__ dil, int* __restrict__ empty_hint)
{
    // the flags once through LDS (volumes of up to 16384 planes; beyond that straight from memory): every thread then reads up to 64 of them
    __shared__ unsigned char sf[16384];
    __shared__ int cnt, cnt_dil;
    const int t = threadIdx.x;
    const bool in_lds = n <= 16384;
    if (t == 0) { cnt = 0; cnt_dil = 0; }
    __syncthreads();
    int mine = 0;
    for (int z = t; z < n; z += 1024) {
        const int f = flags[z] != 0;
        if (in_lds) sf[z] = (unsigned char)f;
        mine += !f;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (t == 0 && empty_hint) *empty_hint = cnt;          // how many planes are empty: a hint for the host (page-locked), see rotate_attenuate_fftx
    auto flag = [&](int z) { return in_lds ? (int)sf[z] : (flags[z] != 0 ? 1 : 0); };
    // (one reflection covers every index asked for here unless the PSF is deeper than the volume: the general form only then)
    auto mir = [&](int i) {
        int j = i < 0 ? -i : i;
        if (j >= n) j = 2 * n - 2 - j;
        return (j >= 0 && j < n) ? j : mirror_index(i, n);
    };
    // one bit per lane, 64 bits per ballot: two words of the bit string per wave and trip
    for (int i0 = 0; i0 < nwords * 32; i0 += 1024) {
        const int i = i0 + t;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(i < nwords * 32 && flag(mir(i - NZ_EXT)) != 0);
        if ((t & 63) == 0) {
            if (i / 32 < nwords) bits[i / 32] = (unsigned int)m;
            if (i / 32 + 1 < nwords) bits[i / 32 + 1] = (unsigned int)(m >> 32);
        }
    }
    int mine_dil = 0;
    for (int z = t; z < n; z += 1024) {
        int any = 0;
        for (int tt = 0; tt < kz; ++tt) any |= flag(mir(z + c - tt));
        dil[z] = any;
        mine_dil += !any;
    }
    if (empty_hint) {
        // (statistics only: how many planes of the z pass's OUTPUT are empty -- what passes D and E skip; mvsim_get_plane_stats)
        if (mine_dil) atomicAdd(&cnt_dil, mine_dil);
        __syncthreads();
        if (t == 0) { empty_hint[1] = cnt_dil; empty_hint[2] = n; }
    }
}

// scal[0] = factor * sum of the partials; with corr_n > 0 also adjustImage's factor scal[1] = (target - min) / (scal[0] / n)
// (Tools.java:146-147: the subtraction in float, the rest in double) -- one launch less per view than a separate kernel.
__global__ __launch_bounds__(1024) void k_reduce_partials(const double* __restrict__ partial, long long count,
                                                          double* __restrict__ scal, double factor, long long corr_n,
                                                          float min_value, float target)
{
    __shared__ double sh[16];
    partial += (long long)blockIdx.x * count;             // stacked views: block v reduces view v's partials into its own pair
    scal += 2 * blockIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    long long i = threadIdx.x;
    for (; i + 3 * 1024 < count; i += 4 * 1024) {
        a0 += partial[i];
        a1 += partial[i + 1024];
        a2 += partial[i + 2 * 1024];
        a3 += partial[i + 3 * 1024];
    }
    for (; i < count; i += 1024) a0 += partial[i];
    double acc = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += sh[w];
        const double sum = t * factor;
        scal[0] = sum;
        if (corr_n > 0) scal[1] = (double)(target - min_value) / (sum / (double)corr_n);
    }
}

// ---------------------------------------------------------------------------------- the length table
// One entry per length of MVSIM_FFT_SIZES, ascending: everything the host asks about a length.  (What is launched for a length is
// picked from the same list in the unit that holds the kernels: launch_lines, launch_r2c, launch_c2r.)
struct LenEntry {
    int len, nrad, rad[5];
    int nl;                 // Cfg<len>::NL: lines per tile of the y and z passes
    int nlx;                // CfgX<len>::NL: rows per block of the x passes with this HALF length (the fused tail's queue segments are per block)
};

static constexpr LenEntry kLens[] = {
#define X(L, ...) {L, (int)(sizeof((int[]){__VA_ARGS__}) / sizeof(int)), {__VA_ARGS__}, Cfg<L>::NL, CfgX<L>::NL},
    MVSIM_FFT_SIZES(X)
#undef X
};

// the smallest table length >= need (null past the table), and the entry of length L itself
static const LenEntry* pick_len(int64_t need)
{
    const LenEntry* e = std::lower_bound(std::begin(kLens), std::end(kLens), need, [](const LenEntry& x, int64_t v) { return x.len < v; });
    return e == std::end(kLens) ? nullptr : e;
}
static const LenEntry* find_len(int L)
{
    const LenEntry* e = pick_len(L);
    return e && e->len == L ? e : nullptr;
}

static int lines_per_tile(int L) { const LenEntry* e = find_len(L); return e ? e->nl : 16; }
}  // namespace fft

// Padded sizes for the custom path, or false if some dimension has no supported size.
bool custom_fft_sizes(const int64_t dim[3], const int64_t kdim[3], int64_t P[3], const Options& opt)
{
    if (opt.rocfft) return false;
    for (int d = 0; d < 3; ++d) {                                  // x: twice the half length M
        const int64_t need = dim[d] + kdim[d] - 1;
        const fft::LenEntry* e = fft::pick_len(d == 0 ? (need + 1) / 2 : need);
        if (!e) return false;
        P[d] = d == 0 ? 2 * (int64_t)e->len : e->len;
    }
    return true;
}

// The one place the geometry of the hand-written convolution is derived (ConvPlan, common.h).
bool conv_plan(const int64_t dim[3], const int64_t kdim[3], const Options& opt, ConvPlan* pl)
{
    using namespace fft;
    if (!custom_fft_sizes(dim, kdim, pl->P, opt)) return false;
    for (int d = 0; d < 3; ++d) { pl->n[d] = (int)dim[d]; pl->k[d] = (int)kdim[d]; }
    pl->px = (int)pl->P[0]; pl->py = (int)pl->P[1]; pl->pz = (int)pl->P[2]; pl->M = pl->px / 2;
    pl->tile_y = lines_per_tile(pl->py); pl->tile_z = lines_per_tile(pl->pz);
    const int ny = pl->n[1], ky = pl->k[1], kz = pl->k[2];
    pl->zdirect = opt.zpass == 2 ? false : kz <= 64;
    pl->ymirror = pl->zdirect && ny > 1 && ky / 2 < ny && ky - 1 - ky / 2 < ny;   // one reflection reaches every halo row
    pl->early = pl->zdirect && opt.early_sum;
    // measured (profiles/r04_zpass_sweep.txt, see zpass_inline): deep PSFs on z lengths of 512 .. 576
    pl->zinline_auto = opt.zpass == 0 && kz >= MVSIM_ZINLINE_MIN_KZ && pl->pz >= 512 && pl->tile_z == 16;
    const int tw_max = std::max(pl->tile_y, pl->zdirect ? NLZ : pl->tile_z);
    pl->hxp = (pl->M + 1 + tw_max - 1) / tw_max * tw_max;
    pl->pyb = (pl->py + ZB - 1) / ZB * ZB;
    pl->e_rows = find_len(pl->M)->nlx;
    return true;
}

// kind 0: per-pass transform table of the plan for length L (see wpasses); kind 1: plain exp(-2 pi i k / L),
// k = 0..L (the real<->complex post/pre-processing of the x passes).
int ensure_twiddles(mvsim_ctx* ctx, int L, int kind, const float2** out)
{
    const int key = L * 2 + kind;
    auto it = ctx->twiddles.find(key);
    if (it != ctx->twiddles.end()) { *out = reinterpret_cast<const float2*>(it->second); return MVSIM_OK; }
    std::vector<float2> h((size_t)L + 1, make_float2(0.f, 0.f));
    if (kind == 1) {
        for (int k = 0; k <= L; ++k) {
            const double a = -2.0 * M_PI * (double)k / (double)L;
            h[k] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    } else {
        const fft::LenEntry* pd = fft::find_len(L);
        if (!pd) { set_error("custom FFT: no plan for length %d", L); return MVSIM_EINVAL; }
        int P = 1, off = 0;
        for (int i = 0; i < pd->nrad; ++i) {
            const int R = pd->rad[i];
            if (P > 1) {
                for (int r = 1; r < R; ++r)
                    for (int k = 0; k < P; ++k) {
                        const double a = -2.0 * M_PI * (double)r * (double)k / ((double)P * (double)R);
                        h[(size_t)off + (size_t)(r - 1) * P + k] = make_float2((float)std::cos(a), (float)std::sin(a));
                    }
                off += (R - 1) * P;
            }
            P *= R;
        }
    }
    void* d = nullptr;
    MVSIM_HIP(hipMalloc(&d, h.size() * sizeof(float2)));
    // synchronous copy from a temporary: happens once per length per context
    hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); set_error("twiddle upload failed: %s", hipGetErrorString(e)); return MVSIM_EHIP; }
    ctx->twiddles[key] = d;
    *out = reinterpret_cast<const float2*>(d);
    return MVSIM_OK;
}

// Weights of the early sum (see ZConvArgs): w[k] = c(k) * SUM_{n < N} e^{+2 pi i k n / P}, k < len; c(k) = 1 unless `half`,
// where c = 1 for k = 0 and k = P/2, 2 for 0 < k < P/2 and 0 beyond (the half spectrum's padding columns).  Built on the
// host in double from an exact P-entry table of e^{2 pi i j / P} (the angle index k n mod P is integer arithmetic).
static int ensure_box_weights(mvsim_ctx* ctx, int N, int P, int len, bool half, const double2** out)
{
    char key[64];
    snprintf(key, sizeof(key), "%d/%d/%d/%d", N, P, len, half ? 1 : 0);
    auto it = ctx->box_weights.find(key);
    if (it != ctx->box_weights.end()) { *out = reinterpret_cast<const double2*>(it->second); return MVSIM_OK; }
    std::vector<double> ct((size_t)P), st((size_t)P);
    for (int j = 0; j < P; ++j) {
        const double a = 2.0 * M_PI * (double)j / (double)P;
        ct[j] = std::cos(a); st[j] = std::sin(a);
    }
    std::vector<double2> h((size_t)len, make_double2(0.0, 0.0));
    for (int k = 0; k < len; ++k) {
        if (half && k > P / 2) break;
        if (!half && k >= P) break;
        long double re = 0.0L, im = 0.0L;
        for (int n = 0; n < N; ++n) {
            const int j = (int)(((long long)k * n) % P);
            re += ct[j]; im += st[j];
        }
        const double c = half ? ((k == 0 || 2 * k == P) ? 1.0 : 2.0) : 1.0;
        h[k] = make_double2(c * (double)re, c * (double)im);
    }
    void* d = nullptr;
    MVSIM_HIP(hipMalloc(&d, h.size() * sizeof(double2)));
    hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); set_error("weight upload failed: %s", hipGetErrorString(e)); return MVSIM_EHIP; }
    ctx->box_weights[key] = d;
    *out = reinterpret_cast<const double2*>(d);
    return MVSIM_OK;
}

// The plan of the fused tail: pass E blocks own queue segments that can hold every voxel of their rows (QueueLayout without the header:
// there may be more than POISSON_MAX_BLOCKS of them), and the resolver counts the RNG in source planes, whichever planes pass E wrote.
static bool fused_tail_of(const ConvPlan& pl, int inc, bool con_wanted, ExtractPlan* fp)
{
    if (!pl.early || (pl.n[0] & 3) != 0) return false;
    const int64_t dim[3] = {pl.n[0], pl.n[1], pl.n[2]};
    const long long nk = con_wanted ? pl.n[2] : (pl.n[2] - 1) / inc + 1;
    const long long rows = pl.n[1] * nk;
    if (rows * pl.n[0] >= (1ll << 32)) return false;               // work items carry the output position in 32 bits
    *fp = ExtractPlan{};
    fp->geom = ExtractGeom::compact(dim, inc);                     // (the acquisition's planes, whichever planes pass E walks)
    fp->kernel = EXTRACT_FUSED_TAIL; fp->share = 16;
    fp->blocks = (int)((rows + pl.e_rows - 1) / pl.e_rows);
    fp->segcap = fp->full_items = (unsigned int)(pl.e_rows * pl.n[0]);
    fp->layout = QueueLayout(fp->blocks, fp->segcap, false);
    return true;
}

bool fused_tail_geometry(const int64_t dim[3], const int64_t kdim[3], int inc, bool con_wanted, const Options& opt, ExtractPlan* fp)
{
    ConvPlan pl;
    return conv_plan(dim, kdim, opt, &pl) && fused_tail_of(pl, inc, con_wanted, fp);
}

size_t fused_tail_queue_bytes(const int64_t dim[3], const int64_t kdim[3], int inc, bool con_wanted, const Options& opt)
{
    ExtractPlan fp{};
    return fused_tail_geometry(dim, kdim, inc, con_wanted, opt, &fp) ? fp.layout.total_bytes : 0;
}

void custom_fft_release(mvsim_ctx* ctx)
{
    for (auto& kv : ctx->twiddles) (void)hipFree(kv.second);
    ctx->twiddles.clear();
    for (auto& kv : ctx->box_weights) (void)hipFree(kv.second);
    ctx->box_weights.clear();
    ctx->partials_z.release();
    ctx->cfft_f.release();
    ctx->cfft_g.release();
    ctx->cfft_g1.release();
    ctx->cfft_g2.release();
}

// {Px, Py, Pz, Hxp, direct z pass?} of the hand-written path for this volume / PSF (what the passes move through HBM)
bool custom_fft_geometry(const int64_t dim[3], const int64_t kdim[3], int64_t g[5], const Options& opt)
{
    ConvPlan pl;
    if (!conv_plan(dim, kdim, opt, &pl)) return false;
    g[0] = pl.px; g[1] = pl.py; g[2] = pl.zdirect ? pl.n[2] : pl.pz; g[3] = pl.hxp; g[4] = pl.zdirect ? 1 : 0;
    return true;
}

// What custom_fft_convolve_slab settles for the z pass of a whole view whose tail asks for the planes k * inc (the same expressions:
// ConvRun::zstride, zs_chunk, zinline; ZConvArgs::zc, and the tile counts of zconv_grid)
bool custom_zpass_geometry(const int64_t dim[3], const int64_t kdim[3], int inc, int64_t g[4], const Options& o)
{
    using namespace fft;
    ConvPlan pl;
    if (inc < 1 || !conv_plan(dim, kdim, o, &pl) || !pl.zdirect) return false;
    const int nz = pl.n[2], kz = pl.k[2];
    const int zstride = (pl.early && inc > 1) ? inc : 1;
    int frows = 0;
    size_t lds = 0;
    const int zs_chunk = (zstride > 1 && o.zconv_strided && o.zpass != 3) ? zconv_strided_chunk(nz, kz, zstride, (o.exp & 2) != 0, &frows, &lds) : 0;
    if (zs_chunk == 0 && (o.zpass == 3 || pl.zinline_auto)) return false;
    const int zc = zs_chunk > 0 ? zs_chunk : zconv_chunk(nz, kz);
    g[0] = zs_chunk > 0 ? zstride : 0; g[1] = zc; g[2] = (nz + zc - 1) / zc; g[3] = pl.hxp / NLZ;
    return true;
}

bool custom_fft_batchable(const mvsim_ctx* ctx, const int64_t dim[3], const int64_t kdim[3])
{
    const Options& o = ctx->opt;
    ConvPlan pl;
    return conv_plan(dim, kdim, o, &pl) && pl.early && !o.fuse_tail && o.zpass != 3 && !pl.zinline_auto && pl.ymirror;
}

// Rotate (about x) + attenuate + pass A as one kernel (rotate_fft.hip) when the view's geometry allows it: the attenuated
// volume then never crosses HBM unless the caller asked for it.  *done = false: nothing was enqueued, the caller runs the
// separate kernels.  On success the context's spectrum buffer F holds what pass A would have written for `att`, and the
// convolution is told so through ConvTail::x_done.
// z_first / nzl: the planes of the rotated volume to compute (a z slab of a tiled view: its own planes and the halo the PSF reaches;
// nzl < 0: all of them).  F then holds those planes from index 0, as pass A leaves them for custom_fft_convolve_slab.
int rotate_attenuate_fftx(mvsim_ctx* ctx, const float* gt, float* rot_or_null, float* att_or_null, const int64_t dim[3],
                          const int64_t kdim[3], const Affine& inv, double delta, bool* done, const int** plane_nz, int z_first, int nzl,
                          const unsigned int** row_bits)
{
    using namespace fft;
    *done = false;
    if (plane_nz) *plane_nz = nullptr;
    if (row_bits) *row_bits = nullptr;
    if (ctx->opt.fused_fftx == 0) return MVSIM_OK;
    if (!affine_is_x_rotation(inv)) return MVSIM_OK;
    ConvPlan pl;
    if (!conv_plan(dim, kdim, ctx->opt, &pl)) return MVSIM_OK;
    const int nx = pl.n[0], ny = pl.n[1], nz = pl.n[2], kx = pl.k[0];
    if (nzl < 0) { z_first = 0; nzl = nz; }
    if (z_first < 0 || nzl < 1 || z_first + nzl > nz) return MVSIM_OK;
    // pass B must be reading the mirrored halo rows from their mirror images (pass A then transforms the Ny rows of a plane
    // only -- what this kernel produces), the padded x row must be one reflection deep, one block must span the row
    if (!pl.ymirror || nx > 1024 || nx < 64 || kx > nx || nx > ny) return MVSIM_OK;
    const int px = pl.px, py = pl.py, M = pl.M, hxp = pl.hxp;
    if (!rot_fftx_len_ok(M)) return MVSIM_OK;
    // auto: from two waves per SIMD of columns up (below that the kernel is a handful of serial waves, like its parent)
    if (ctx->opt.fused_fftx == 2 && (int64_t)nx * nzl < 131072) return MVSIM_OK;
    // the driver finds the spectrum in F and must not move it: it checks its own size against this one (ConvTail::x_done)
    const size_t cbytes = pl.spectrum_bytes(nzl, 0, 0, 1);
    MVSIM_TRY(ctx->cfft_f.reserve(cbytes));
    MVSIM_TRY(ctx->cfft_g.reserve(cbytes));
    const float2 *tw_m, *tw_px;
    MVSIM_TRY(ensure_twiddles(ctx, M, 0, &tw_m));
    MVSIM_TRY(ensure_twiddles(ctx, px, 1, &tw_px));
    RotFftArgs a{};
    a.in = gt; a.rot_out = rot_or_null; a.att_out = att_or_null; a.dst = ctx->cfft_f.as<float2>();
    a.twg = tw_m; a.twx = tw_px;
    a.nx = nx; a.ny = ny; a.nz = nz; a.steps = nx;                     // Q1: attenuate3d walks dimension(0) steps along y
    a.z_first = z_first; a.nzl = nzl;
    a.hxp = hxp; a.py = py;
    a.halo_r = kx / 2; a.halo_l = kx - 1 - kx / 2;
    a.a = inv; a.delta = delta;
    // The flags cost a volume WITHOUT empty planes about 1.5 % of a view (a scalar load in front of every block's tile loads, the bit
    // strings of the z pass): the last flagged view says how many planes were empty (a page-locked word the device writes, read here
    // without waiting -- a hint, nothing depends on its being current), and while that was none only every sixteenth view carries
    // flags, to notice when the data change.  Results are the same with and without flags.
    bool want_flags = plane_nz && ctx->opt.skip_empty && nzl == nz;     // (a slab keeps the unflagged passes)
    if (want_flags) {
        if (!ctx->empty_hint) {
            MVSIM_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->empty_hint), 4 * sizeof(int), hipHostMallocDefault));
            ctx->empty_hint[0] = -1; ctx->empty_hint[1] = -1; ctx->empty_hint[2] = 0; ctx->empty_hint[3] = 0;
        }
        const int hint = *reinterpret_cast<volatile int*>(ctx->empty_hint);
        if (hint == 0 && ctx->views_since_flags < 15) { want_flags = false; ctx->views_since_flags += 1; }
        else ctx->views_since_flags = 0;
    }
    if (want_flags) {
        // Beside the flags, the row-bit records (row_bits.h; option skip_rows): the kernel then stores no row without a non-zero voxel
        // and pass B -- k_fft_lines<FWD> of py points on this view's whole spectrum, nothing else -- reads the bits.  Not where pass B
        // takes the split long-line form, which does not read them.
        const bool want_rows = row_bits && ctx->opt.skip_rows && pl.zdirect && row_bits_len_ok(py) && !(py % 2 == 0 && lines_split_exists(py / 2));
        const size_t flag_bytes = ((size_t)(3 * nz + 1024) * sizeof(int) + 255) & ~(size_t)255;   // flags, the dilated flags, the flag bit string
        MVSIM_TRY(ctx->plane_flags.reserve(flag_bytes + (want_rows ? row_bits_bytes(py, nz) : 0)));
        a.plane_nz = ctx->plane_flags.as<int>();
        *plane_nz = a.plane_nz;
        if (want_rows) {
            a.rowbits = reinterpret_cast<unsigned int*>(ctx->plane_flags.as<char>() + flag_bytes);
            a.ky = pl.k[1];
            *row_bits = a.rowbits;
        }
    }
    MVSIM_TRY(launch_rot_fftx(ctx, M, a, rot_or_null != nullptr || att_or_null != nullptr, ctx->opt.fused_fftx >= 2));
    *done = true;
    return MVSIM_OK;
}

// ---------------------------------------------------------------------------------- the driver
namespace fft {
// What one call has settled before it enqueues anything, for the stages below.
struct ConvRun {
    const ConvPlan& pl;
    SlabRange slab;                 // nz_in: planes the image spectrum holds when zdirect; nz_out: planes that leave the z pass
    bool is_slab;
    long long plane;                // elements of a plane of the plane-major spectrum: hxp * py
    int V, zstride;                 // stacked views; passes D and E produce the planes k * zstride only
    int nzp;                        // plane pitch of a view in the z pass's output: its planes k * zstride at multiples of zstride of the stacked index
    int nk;                         // planes 0, zstride, 2 zstride, ... of every stacked view: what passes D and E see
    int zs_chunk, zs_frows;         // k_zconv_strided's tile (chunk 0: this call keeps k_zconv)
    size_t zs_lds;
    bool zinline;                   // the z pass as FFT -> product -> inverse FFT per tile (CONVZ)
    long long corr_n;               // adjustImage's factor rides in the reduction of the sum (0: not asked for)
    float corr_min, corr_target;
    const float2 *tw_m, *tw_px, *tw_py, *tw_pz;
    float2 *F, *G, *G1, *G2;
    double* scal;
    const int *pnz, *pnz_dil;       // planes the fused rotate kernel found empty (null: no flags): raw, dilated by the taps' reach,
    const unsigned int* pnz_bits;   // and as the z pass's bit string
    const unsigned int* rowbits;    // the rotate kernel's row-bit record (null: it wrote every row): pass B's
};

// compact PSF intermediates: G1 [kz][ky][hxp] (x transformed), G2 [kz][py][hxp] (x,y transformed), G the full spectrum (FFT z pass only)
static int psf_passes(mvsim_ctx* ctx, const ConvRun& r, const float* psf)
{
    const ConvPlan& pl = r.pl;
    const int kx = pl.k[0], ky = pl.k[1], kz = pl.k[2], hxp = pl.hxp, V = r.V;
    SrcMap m{};
    m.x = DimMap{kx, pl.px, kx - kx / 2, kx / 2, 1, kx / 2};   // embed along x with wrap-around
    m.y = DimMap{ky, ky, ky, 0, 1, 0};                         // compact: identity
    m.z = DimMap{kz * V, kz * V, kz * V, 0, 1, 0};             // (stacked PSFs: V x Kz planes of taps)
    MVSIM_TRY(launch_r2c(ctx, pl.M, psf, m, r.G1, r.tw_m, r.tw_px, hxp, (long long)ky * kz * V));
    LinesArgs a{};
    a.src = r.G1; a.dst = r.G2; a.spec = nullptr; a.tw = r.tw_py;
    a.src_es = hxp; a.src_outer = (long long)hxp * ky;          // per kz plane
    a.dst_es = hxp; a.dst_outer = r.plane;
    if (pl.zdirect) { a.dst_outer = (long long)ZB * hxp; a.dst_blk = (long long)kz * V * ZB * hxp; }   // the z pass reads its taps z-blocked
    a.lmap = DimMap{ky, pl.py, ky - ky / 2, ky / 2, 1, ky / 2};
    MVSIM_TRY(launch_lines(ctx, pl.py, FWD, true, a, hxp / pl.tile_y, kz * V));
    if (pl.zdirect) return MVSIM_OK;
    LinesArgs c{};
    c.src = r.G2; c.dst = r.G; c.spec = nullptr; c.tw = r.tw_pz;
    c.src_es = r.plane; c.src_outer = hxp;                         // per ky row
    c.dst_es = r.plane; c.dst_outer = hxp;
    c.lmap = DimMap{kz, pl.pz, kz - kz / 2, kz / 2, 1, kz / 2};
    c.dst_tile_major = 1;                                         // consumed line by line in pass C
    return launch_lines(ctx, pl.pz, FWD, true, c, hxp / pl.tile_z, pl.py);
}

// ---- PSF spectrum.  The embedded kernel is zero outside Kx*Ky*Kz taps, so the x pass runs on the
//      Ky*Kz non-zero rows only, the y pass on the Kz non-zero planes only (sparse loads), and the z
//      pass expands Kz planes to the full spectrum.
// It depends on nothing the image passes A and B produce and is a handful of small launches, so it runs on the
// context's side stream beside them (fork here, join before the z pass reads G2 / G: ctx->psf_on_side).
// Only where it pays: the fork and the join cost ~10 us of cross-stream dependency, more than the spectrum of a small view.
//
// entry (psf_cache.h; null: no cache for this call): r.G2 is the entry's buffer.  A filled entry holds the very bytes the two passes would
// write (same taps, same geometry, same kernels): nothing is launched, and no fork is recorded for the PSF -- only the one
// k_plane_flags_finish needs on the side stream when this view carries flags (flags_follow).  An entry that is not filled gets the passes'
// output instead of ctx->cfft_g2.  Its buffer may be an evicted entry's, which the PREVIOUS view's z pass may still be reading on the
// main stream: the passes write it on the side stream behind ev_fork, recorded here on the main stream, that is behind that z pass --
// or on the main stream itself.  Stream order protects the slot; keep the fork in front of anything that writes an entry.
static int psf_spectrum(mvsim_ctx* ctx, const ConvRun& r, const float* psf, PsfCache::Entry* entry, bool flags_follow)
{
    hipStream_t s = ctx->stream;
    const bool hit = entry && entry->filled;
    const bool side = ctx->opt.psf_overlap && (int64_t)r.pl.n[0] * r.pl.n[1] * r.pl.n[2] >= (int64_t)1 << 24 && (!hit || flags_follow);
    ctx->psf_on_side = side;
    if (side) {
        if (!ctx->side_stream) {
            MVSIM_HIP(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
            MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
            MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        }
        MVSIM_HIP(hipEventRecord(ctx->ev_fork, s));
        MVSIM_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
        if (hit) return MVSIM_OK;                       // (plane_flags_setup records the join behind its kernel)
        ctx->stream = ctx->side_stream;                 // the launch helpers enqueue on ctx->stream
    }
    if (hit) return MVSIM_OK;
    ev_begin(ctx, ST_PSF);
    const int rc = psf_passes(ctx, r, psf);
    ev_end(ctx, ST_PSF);
    if (entry && rc == MVSIM_OK) entry->filled = true;
    if (side) {
        // always joined, also after a failed launch: a stream capture must not end with the side stream dangling
        ctx->stream = s;
        MVSIM_HIP(hipEventRecord(ctx->ev_join, ctx->side_stream));
    }
    return rc;
}

// Pass A.  Direct z pass: no z padding (k_zconv mirrors through an index map), and the mirrored halo rows along y are copies of rows
// pass A transforms anyway, so it transforms the Ny rows of a r.plane only and pass B reads the halo positions from their mirror
// images (same bytes, from L2).
static int pass_a(mvsim_ctx* ctx, const ConvRun& r, const float* img)
{
    const ConvPlan& pl = r.pl;
    const int planes = r.slab.nz_in * r.V;
    SrcMap m{};
    DimMap* dm[3] = {&m.x, &m.y, &m.z};
    for (int d = 0; d < 3; ++d) *dm[d] = DimMap{pl.n[d], (int)pl.P[d], pl.n[d] + pl.k[d] / 2, pl.k[d] - 1 - pl.k[d] / 2, 0, 0};
    if (pl.zdirect) m.z = DimMap{planes, planes, planes, 0, 0, 0};
    if (pl.ymirror) { m.y = DimMap{pl.n[1], pl.py, pl.n[1], 0, 0, 0}; m.enum_y = pl.n[1]; }   // ... and visits no other row
    const long long rows = pl.zdirect ? (long long)(pl.ymirror ? pl.n[1] : pl.py) * planes : (long long)pl.py * pl.pz;
    ev_begin(ctx, ST_PASS_A);
    MVSIM_TRY(launch_r2c(ctx, pl.M, img, m, r.F, r.tw_m, r.tw_px, pl.hxp, rows));
    ev_end(ctx, ST_PASS_A);
    return MVSIM_OK;
}

// Planes the fused rotate kernel found empty: B skips them, C' does not load them and skips tiles made of nothing else, D and E
// skip the planes whose taps reach nothing but empty planes (exact: their spectra are zero) -- a specimen in empty space.
// ctx->plane_flags = [flags (nz)][dilated (nz)][bit string (nwords)] (rotate_attenuate_fftx reserves all three)
static int plane_flags_setup(mvsim_ctx* ctx, ConvRun& r, const int* pnz)
{
    const int nz = r.pl.n[2], kz = r.pl.k[2];
    int* base = ctx->plane_flags.as<int>();
    const int nwords = (nz + 2 * NZ_EXT + 64 + 31) / 32 + ZNIT + 2;
    // one block, ~9 us: beside pass B on the side stream when there is one (pass B reads the raw flags; the bit string and the
    // dilated flags are for passes C', D and E, behind the join)
    const bool side = ctx->psf_on_side;
    hipLaunchKernelGGL(k_plane_flags_finish, dim3(1), dim3(1024), 0, side ? ctx->side_stream : ctx->stream, pnz, nz, kz, kz / 2,
                       reinterpret_cast<unsigned int*>(base + 2 * nz), nwords, base + nz, ctx->empty_hint);
    MVSIM_HIP(hipGetLastError());
    if (side) MVSIM_HIP(hipEventRecord(ctx->ev_join, ctx->side_stream));
    r.pnz = pnz;
    r.pnz_dil = base + nz;
    r.pnz_bits = reinterpret_cast<const unsigned int*>(base + 2 * nz);
    return MVSIM_OK;
}

// Pass B: F -> F in place, or (direct z pass) out of place into the z-blocked layout the z pass reads and writes:
// G[(ky >> ZBS)][z][ky & (ZB-1)][kx].
// Zero gap of the padded volume: y in [Ny + cy, Py - lefty), z in [Nz + cz, Pz - leftz).  Pass A does not transform (or write) rows
// there, pass B skips the gap planes and does not load gap rows, pass C does not load gap planes.
static int pass_b(mvsim_ctx* ctx, const ConvRun& r)
{
    const ConvPlan& pl = r.pl;
    const int hxp = pl.hxp, ny = pl.n[1], ky = pl.k[1], kz = pl.k[2];
    LinesArgs b{};
    b.src = r.F; b.dst = r.F; b.tw = r.tw_py; b.src_es = b.dst_es = hxp; b.src_outer = b.dst_outer = r.plane;
    b.lmap = DimMap{0, 0, 0, 0, 1, 0};
    if (pl.ymirror) { b.lmap = DimMap{ny, pl.py, ny + ky / 2, ky - 1 - ky / 2, 0, 0}; b.src_mirror = 1; }
    b.gap_lo = ny + ky / 2; b.gap_hi = pl.py - (ky - 1 - ky / 2);
    if (pl.zdirect) {
        b.outer_skip_lo = 1 << 30;
        b.dst = r.G; b.dst_outer = (long long)ZB * hxp; b.dst_blk = (long long)r.slab.nz_in * r.V * ZB * hxp;
    } else {
        b.outer_skip_lo = pl.n[2] + kz / 2;
        b.outer_skip_len = std::max(0, pl.pz - (kz - 1 - kz / 2) - b.outer_skip_lo);
    }
    if (r.pnz) { b.nzflags = r.pnz; b.nz_stride = 1; }
    // the rotate kernel of this view produced the row-bit record, i.e. left the rows whose bit is clear unwritten: read the bits
    // (with or without the plane flags -- an empty plane's bits are all clear)
    if (r.rowbits) { b.rowbits = r.rowbits; b.rowbits_stride = row_bits_words(pl.py); }
    ev_begin(ctx, ST_PASS_B);
    MVSIM_TRY(launch_lines(ctx, pl.py, FWD, false, b, hxp / pl.tile_y, pl.zdirect ? r.slab.nz_in * r.V : pl.pz - b.outer_skip_len));
    ev_end(ctx, ST_PASS_B);
    return MVSIM_OK;
}

// The z pass on the unpadded spectrum as FFT -> product -> inverse FFT with the PSF's z spectrum computed per tile (CONVZ): from
// MVSIM_ZINLINE_MIN_KZ taps up the Kz-tap direct convolution is bound by its FMAs and this form by HBM.
// Measured, whole views with 31 x 31 x Kz PSFs (profiles/r04_zpass_sweep.txt): 2048 x 2048 x 512 (padded z length 576: tiles of 16
// lines, 128-byte rows) -- pass C 8.1 ms whatever Kz against 8.1 / 9.0 / 10.2 ms for the direct form at Kz = 41 / 51 / 63; 1024^3
// (length 1120: tiles of 8 lines, 64-byte rows, one line per wave) -- 5.6 ms against 3.9 / 4.4 / 4.9 ms.  Hence auto = deep PSFs on
// z lengths of 512 .. 576 (the sizes measured to win; ConvPlan::zinline_auto); everything else keeps the direct form unless asked.
// Compact planes: the direct form computes 1 / zstride of the planes (k_zconv_strided) and is then ahead of this one at every depth.
// G (z-blocked) -> F (z-blocked).
static int zpass_inline(mvsim_ctx* ctx, const ConvRun& r)
{
    const ConvPlan& pl = r.pl;
    const int nz = pl.n[2], kz = pl.k[2], pz = pl.pz, hxp = pl.hxp;
    LinesArgs c{};
    c.src = r.G; c.dst = r.F; c.tw = r.tw_pz;
    c.src_es = c.dst_es = (long long)ZB * hxp; c.src_outer = c.dst_outer = hxp;
    c.src_oblk = (long long)r.slab.nz_in * ZB * hxp; c.dst_oblk = (long long)r.slab.nz_out * ZB * hxp;
    c.lmap = DimMap{nz, pz, nz + kz / 2, kz - 1 - kz / 2, 0, 0};
    c.src_mirror = 1;
    c.gap_lo = nz + kz / 2; c.gap_hi = pz - (kz - 1 - kz / 2);
    c.outer_skip_lo = 1 << 30;
    c.store_limit = nz;
    c.taps = r.G2; c.taps_es = (long long)ZB * hxp; c.taps_outer = hxp; c.taps_oblk = (long long)kz * ZB * hxp;
    c.pmap = DimMap{kz, pz, kz - kz / 2, kz / 2, 1, kz / 2};
    const float scale_f = (float)(0.25 / ((double)pl.px * (double)pl.py * (double)pz));
    const long long zblocks = (long long)(hxp / pl.tile_z) * pl.py;
    if (pl.early) {
        MVSIM_TRY(ensure_box_weights(ctx, pl.n[0], pl.px, hxp, true, &c.wx));
        MVSIM_TRY(ensure_box_weights(ctx, pl.n[1], pl.py, pl.py, false, &c.wy));
        MVSIM_TRY(ctx->partials_z.reserve((size_t)zblocks * sizeof(double)));
        c.sum_partial = ctx->partials_z.as<double>();
    }
    MVSIM_TRY(launch_lines(ctx, pz, CONVZ, false, c, hxp / pl.tile_z, pl.py));
    if (pl.early) {
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, ctx->stream, c.sum_partial, zblocks, r.scal, (double)scale_f,
                           r.corr_n, r.corr_min, r.corr_target);
        MVSIM_HIP(hipGetLastError());
    }
    return MVSIM_OK;
}

// The direct z pass, every r.plane (k_zconv) or the planes k * zstride only (k_zconv_strided): G (z-blocked) -> F (z-blocked)
static int zpass_direct(mvsim_ctx* ctx, const ConvRun& r)
{
    const ConvPlan& pl = r.pl;
    const int kz = pl.k[2], hxp = pl.hxp, V = r.V;
    ZConvArgs z{};
    z.src = r.G; z.dst = r.F; z.taps = r.G2; z.hxp = hxp; z.nz = r.slab.nz_out; z.kz = kz; z.c = kz / 2;
    z.zs = (long long)ZB * hxp; z.src_blk = (long long)r.slab.nz_in * V * ZB * hxp; z.dst_blk = (long long)r.nzp * V * ZB * hxp;
    z.taps_blk = (long long)kz * V * ZB * hxp;
    z.src_view = (long long)r.slab.nz_in * z.zs; z.dst_view = (long long)r.nzp * z.zs; z.taps_view = (long long)kz * z.zs;
    z.nz_global = pl.n[2]; z.z_in0 = r.slab.z_in0; z.z_out0 = r.slab.z_out0;
    z.zc = r.zs_chunk > 0 ? r.zs_chunk : zconv_chunk(r.slab.nz_out, kz);
    z.stride = r.zs_chunk > 0 ? r.zstride : 1; z.frows = r.zs_frows;
    z.nzbits = r.pnz_bits;
    const float scale_f = (float)(0.25 / ((double)pl.px * (double)pl.py));
    long long zblocks = 0;
    if (pl.early) {
        MVSIM_TRY(ensure_box_weights(ctx, pl.n[0], pl.px, hxp, true, &z.wx));
        MVSIM_TRY(ensure_box_weights(ctx, pl.n[1], pl.py, pl.py, false, &z.wy));
        zblocks = zconv_blocks(z, pl.py);
        MVSIM_TRY(ctx->partials_z.reserve((size_t)zblocks * V * sizeof(double)));
        z.sum_partial = ctx->partials_z.as<double>();
    }
    if (r.zs_chunk > 0) MVSIM_TRY(launch_zconv_strided(ctx, z, pl.py, r.zs_lds, V));
    else MVSIM_TRY(launch_zconv(ctx, z, pl.py, V));
    if (pl.early) {
        // same factor pass E applies to every voxel (a float), so that the two sums estimate the same quantity
        hipLaunchKernelGGL(k_reduce_partials, dim3(V), dim3(1024), 0, ctx->stream, z.sum_partial, zblocks, r.scal, (double)scale_f,
                           r.corr_n, r.corr_min, r.corr_target);
        MVSIM_HIP(hipGetLastError());
    }
    return MVSIM_OK;
}

// The z pass on the z-padded spectrum: FFT, product with the PSF's spectrum G, inverse FFT, in place in F
static int zpass_fft(mvsim_ctx* ctx, const ConvRun& r)
{
    const ConvPlan& pl = r.pl;
    const int nz = pl.n[2], kz = pl.k[2], hxp = pl.hxp;
    LinesArgs c{};
    c.src = r.F; c.dst = r.F; c.spec = r.G; c.tw = r.tw_pz;
    c.src_es = c.dst_es = c.spec_es = r.plane; c.src_outer = c.dst_outer = c.spec_outer = hxp;
    c.lmap = DimMap{0, 0, 0, 0, 1, 0};
    c.gap_lo = nz + kz / 2; c.gap_hi = pl.pz - (kz - 1 - kz / 2);
    c.outer_skip_lo = 1 << 30;
    c.store_limit = nz;                                           // pass D only reads planes z < Nz
    return launch_lines(ctx, pl.pz, CONV, false, c, hxp / pl.tile_z, pl.py);
}

// Pass D: the planes k * zstride, from F (z-blocked after a direct or inline z pass) into `dst` (plane-major)
static int pass_d(mvsim_ctx* ctx, const ConvRun& r, float2* dst)
{
    const ConvPlan& pl = r.pl;
    const int hxp = pl.hxp;
    LinesArgs d{};
    d.src = r.F; d.dst = dst; d.tw = r.tw_py; d.src_es = d.dst_es = hxp;
    d.src_outer = d.dst_outer = r.plane * r.zstride;
    if (pl.zdirect) { d.src_outer = (long long)ZB * hxp * r.zstride; d.src_blk = (long long)r.nzp * r.V * ZB * hxp; }
    d.lmap = DimMap{0, 0, 0, 0, 1, 0};
    d.outer_skip_lo = 1 << 30;
    d.store_limit = pl.n[1];                                      // pass E only reads rows y < Ny
    if (r.pnz) { d.nzflags = r.pnz_dil; d.nz_stride = r.zstride; }
    ev_begin(ctx, ST_PASS_D);
    MVSIM_TRY(launch_lines(ctx, pl.py, INV, false, d, hxp / pl.tile_y, r.nk));
    ev_end(ctx, ST_PASS_D);
    return MVSIM_OK;
}

// Fused tail: what pass E needs to adjust, extract and sample.  adjustImage's factor must exist before pass E runs:
// (target - min) / (sum / n) from the early sum.
static int fused_tail_args(mvsim_ctx* ctx, const ConvRun& r, const ConvTail& tail, const ExtractPlan& fp, C2RFuse* fz)
{
    if (!tail.corr_done) {
        ev_begin(ctx, ST_ADJUST);
        MVSIM_TRY(launch_adjust_corr(ctx->stream, r.scal, (int64_t)r.pl.n[0] * r.pl.n[1] * r.pl.n[2], tail.min_value, tail.target_average));
        ev_end(ctx, ST_ADJUST);
    }
    fz->scal = r.scal; fz->min_value = tail.min_value; fz->con = tail.con_adj; fz->acq = tail.acq;
    fz->acq_every = tail.con_adj ? tail.inc : 1; fz->idx_zstride = r.zstride; fz->noise = tail.noise ? 1 : 0;
    fz->mul = tail.mul; fz->k0 = (uint32_t)tail.seed; fz->k1 = (uint32_t)(tail.seed >> 32); fz->stream = tail.stream;
    if (tail.noise) {
        if (ctx->pqueue.bytes < fp.layout.total_bytes) {
            set_error("fused tail: queue workspace not reserved");
            return MVSIM_EINVAL;
        }
        const QueueLayout::Region q = fp.layout.region(ctx->pqueue.p);
        fz->qcount = q.counts; fz->queue = reinterpret_cast<PItem*>(q.items);
        fz->segcap = fp.segcap;
    }
    return MVSIM_OK;
}
}  // namespace fft

int custom_fft_convolve(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* psf,
                        const int64_t kdim[3], float* out, ConvTail* tail)
{
    const SlabRange whole{0, (int)dim[2], 0, (int)dim[2]};
    return custom_fft_convolve_slab(ctx, img, dim, psf, kdim, whole, out, tail);
}

// Decide; PSF spectrum; image: A, B, C (with product), D, E.
int custom_fft_convolve_slab(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* psf,
                             const int64_t kdim[3], const SlabRange& slab, float* out, ConvTail* tail)
{
    using namespace fft;
    ConvPlan pl;
    if (!conv_plan(dim, kdim, ctx->opt, &pl)) { set_error("custom FFT: no hand-written size for this volume / PSF"); return MVSIM_EINVAL; }
    const Options& o = ctx->opt;
    const int kz = pl.k[2];
    ConvRun r{pl, slab};
    r.plane = (long long)pl.hxp * pl.py;
    r.is_slab = slab.nz_in != pl.n[2] || slab.nz_out != pl.n[2];
    // stacked views (ConvTail::views = V > 1; the caller has asked custom_fft_batchable): `img` holds V attenuated volumes back to back,
    // `psf` V PSFs, `out` receives V convolved volumes (compact planes: V x nk), the context's scalar pairs 0 .. V-1 the sums and factors.
    // Passes A, B, D, E and the PSF's passes work on planes (rows) and simply see V x as many; the z pass carries the view in its grid.
    r.V = (tail && tail->views > 1) ? tail->views : 1;
    // with the sum known before passes D and E (early), they only have to produce the planes extractSlices reads
    // (a z slab may ask for it too: its first output plane is then a multiple of the stride -- the caller's promise -- so that the planes
    // k * zstride of the SLAB are planes k' * zstride of the view)
    r.zstride = (tail && pl.early && tail->zstride > 1 && (!r.is_slab || slab.z_out0 % tail->zstride == 0)) ? tail->zstride : 1;
    // fused tail: pass E adjusts, extracts and samples (needs the sum first, whole rows of float4 groups, aligned outputs)
    ExtractPlan fp{};
    const bool fuse = tail && tail->want_fuse && !r.is_slab && tail->acq &&
                      fused_tail_of(pl, tail->inc, tail->con_adj != nullptr, &fp) &&
                      ((reinterpret_cast<uintptr_t>(tail->acq) | reinterpret_cast<uintptr_t>(tail->con_adj)) & 15) == 0;
    if (fuse) r.zstride = tail->con_adj ? 1 : tail->inc;
    if (tail) { tail->zstride = r.zstride; tail->fused = fuse; tail->fused_blocks = fp.blocks; tail->fused_segcap = fp.segcap; }
    // adjustImage's factor rides in the reduction of the sum when the caller described it (a view; not the stage operator)
    r.corr_n = (tail && tail->corr_n > 0 && !r.is_slab) ? tail->corr_n : 0;
    r.corr_min = tail ? tail->min_value : 0.f; r.corr_target = tail ? tail->target_average : 1.f;
    if (tail) tail->corr_done = r.corr_n > 0;
    const bool x_done = tail && tail->x_done;
    if (r.is_slab && !pl.zdirect) {
        set_error("z-slab tiling needs the direct z pass (PSF depth %d > 64 or option fft_zpass=fft)", kz);
        return MVSIM_EINVAL;
    }
    if (r.V > 1 && (r.is_slab || !pl.early || fuse || x_done || tail->plane_nz)) {
        set_error("stacked views need the direct z pass with the early sum on whole views");
        return MVSIM_EINVAL;
    }
    const int nkv = (r.slab.nz_out - 1) / r.zstride + 1;            // planes per view that leave passes D and E
    r.nzp = r.V > 1 ? nkv * r.zstride : r.slab.nz_out;
    r.nk = nkv * r.V;                                               // (FFT z pass: whole views only, nzo = Nz; planes z >= Nz are never read)
    const size_t cbytes = pl.spectrum_bytes(r.slab.nz_in, r.slab.nz_out, r.nzp, r.V);
    const long long rows_out_early = (long long)pl.n[1] * r.slab.nz_out * r.V;
    // the fused rotate + attenuate + x transform has left the spectrum of the attenuated rows in F already (a slab's: its nz_in input
    // planes -- the slab and its halo -- from plane 0): F must stay where it is
    if (x_done && cbytes > ctx->cfft_f.bytes) {
        set_error("custom FFT: the spectrum needs %zu bytes, the fused x transform left it in %zu", cbytes, ctx->cfft_f.bytes);
        return MVSIM_EINVAL;
    }
    if (!x_done) MVSIM_TRY(ctx->cfft_f.reserve(cbytes));
    MVSIM_TRY(ctx->cfft_g.reserve(cbytes));
    r.zs_chunk = (pl.zdirect && r.zstride > 1 && o.zconv_strided && o.zpass != 3)
                     ? zconv_strided_chunk(slab.nz_out, kz, r.zstride, (o.exp & 2) != 0, &r.zs_frows, &r.zs_lds) : 0;
    r.zinline = pl.zdirect && !r.is_slab && r.zs_chunk == 0 && r.V == 1 && (o.zpass == 3 || pl.zinline_auto);
    // The cache entry psf_prepare settled for this call (it is this call's alone: taken off the context here).  Used by whole single
    // views on the direct z pass, for the very taps `psf` points at and a G2 of this plan's size; anything else -- stacked views, a z slab,
    // the inline FFT z pass -- transforms `psf` into the context's own G2 as ever (the taps in an entry are valid device memory either way).
    const size_t g2_bytes = (size_t)r.V * pl.hxp * pl.pyb * kz * sizeof(float2);
    PsfCache::Entry* pe = ctx->psf_entry;
    ctx->psf_entry = nullptr;
    if (pe && !(r.V == 1 && !r.is_slab && pl.zdirect && !r.zinline && psf == pe->psf && pe->g2_bytes == g2_bytes)) pe = nullptr;
    if (!(pe && pe->filled)) MVSIM_TRY(ctx->cfft_g1.reserve((size_t)r.V * pl.hxp * pl.k[1] * kz * sizeof(float2)));
    if (!pe) MVSIM_TRY(ctx->cfft_g2.reserve(g2_bytes));
    MVSIM_TRY(ctx->partials.reserve(PARTIALS_BYTES));
    MVSIM_TRY(ctx->partials_e.reserve((size_t)((rows_out_early + 3) / 4 + 16) * sizeof(double)));
    r.scal = scal_of(ctx);
    MVSIM_TRY(ensure_twiddles(ctx, pl.M, 0, &r.tw_m));
    MVSIM_TRY(ensure_twiddles(ctx, pl.px, 1, &r.tw_px));
    MVSIM_TRY(ensure_twiddles(ctx, pl.py, 0, &r.tw_py));
    if (!pl.zdirect || r.zinline) MVSIM_TRY(ensure_twiddles(ctx, pl.pz, 0, &r.tw_pz));
    r.F = ctx->cfft_f.as<float2>(); r.G = ctx->cfft_g.as<float2>();
    r.G1 = ctx->cfft_g1.as<float2>(); r.G2 = pe ? static_cast<float2*>(pe->g2) : ctx->cfft_g2.as<float2>();
    hipStream_t s = ctx->stream;

    const bool flags_follow = x_done && tail->plane_nz && !r.zinline && !r.is_slab && !fuse;   // plane_flags_setup, below
    MVSIM_TRY(psf_spectrum(ctx, r, psf, pe, flags_follow));

    ev_begin(ctx, ST_CONVOLVE);
    if (x_done) {
        if (!pl.ymirror || r.V != 1) { set_error("x_done without the geometry of the fused x transform"); return MVSIM_EINVAL; }
        if (tail->row_bits) {
            if (r.is_slab || !pl.zdirect) { set_error("row bits on a view pass B cannot read them for"); return MVSIM_EINVAL; }
            r.rowbits = tail->row_bits;
        }
    } else {
        MVSIM_TRY(pass_a(ctx, r, img));
    }
    if (flags_follow) MVSIM_TRY(plane_flags_setup(ctx, r, tail->plane_nz));
    MVSIM_TRY(pass_b(ctx, r));
    if (ctx->psf_on_side) MVSIM_HIP(hipStreamWaitEvent(s, ctx->ev_join, 0));    // the z pass reads the PSF spectrum
    ev_begin(ctx, ST_PASS_C);
    if (r.zinline) MVSIM_TRY(zpass_inline(ctx, r));
    else if (pl.zdirect) MVSIM_TRY(zpass_direct(ctx, r));
    else MVSIM_TRY(zpass_fft(ctx, r));
    ev_end(ctx, ST_PASS_C);
    float2* Fz = pl.zdirect ? r.G : r.F;                            // where pass D leaves the z-convolved spectrum for pass E
    MVSIM_TRY(pass_d(ctx, r, Fz));
    C2RFuse fz{};
    if (fuse) MVSIM_TRY(fused_tail_args(ctx, r, *tail, fp, &fz));
    ev_begin(ctx, ST_PASS_E);
    // both half spectra carry the factor 2 left in by pass A (see k_fft_x_r2c): 2 * 2 = 4
    const float scale = (float)(0.25 / ((double)pl.px * (double)pl.py * ((pl.zdirect && !r.zinline) ? 1.0 : (double)pl.pz)));
    int nblk = 0;
    // The sparse tail (option skip_tail; extract_plan.h: tail_sparse_ok): this view carries plane flags, and the caller vouches that
    // `out` is a workspace nobody but its flagged queue sampler reads -- pass E then stores nothing into the planes k whose dilated
    // flag k * zstride is clear.  Handed over through the tail: the flags the sampler reads are the words pass E read.
    // (r.pnz_dil already says: x_done, a whole single view, skip_empty, not the inline z pass, not the fused tail)
    const bool sparse = tail_sparse_ok(tail && tail->want_sparse, r.pnz_dil != nullptr, fuse) && r.V == 1 && !r.is_slab;
    if (tail) { tail->sparse = sparse; tail->sparse_flags = sparse ? r.pnz_dil : nullptr; tail->sparse_stride = sparse ? r.zstride : 0; }
    MVSIM_TRY(launch_c2r(ctx, pl.M, Fz, out, r.tw_m, r.tw_px, pl.hxp, pl.py * r.zstride, pl.n[0], pl.n[1], (long long)pl.n[1] * r.nk, scale,
                         pl.early ? nullptr : ctx->partials_e.as<double>(), &nblk, fuse ? &fz : nullptr,
                         C2REmpty{r.pnz_dil, r.zstride, sparse ? 1 : 0}));
    if (fuse && nblk != fp.blocks) { set_error("fused tail: block count mismatch"); return MVSIM_EINVAL; }
    if (!pl.early) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(1024), 0, s, ctx->partials_e.as<double>(), (long long)nblk, r.scal, 1.0,
                                      r.corr_n, r.corr_min, r.corr_target);
    MVSIM_HIP(hipGetLastError());
    ev_end(ctx, ST_PASS_E);
    if (fuse && tail->noise) {
        ev_end(ctx, ST_CONVOLVE);
        ev_begin(ctx, ST_EXTRACT);
        ExtractOps ops;
        ops.out = tail->acq; ops.queue_ws = ctx->pqueue.p; ops.mul = tail->mul; ops.seed = tail->seed; ops.stream = tail->stream;
        MVSIM_TRY(launch_resolve(s, fp, ops));
        ev_end(ctx, ST_EXTRACT);
        return MVSIM_OK;
    }
    ev_end(ctx, ST_CONVOLVE);
    return MVSIM_OK;
}

}  // namespace mvsim
