// The transform passes of the hand-written FFT convolution (fft_driver.hip has the overview), instantiated for every length of
// MVSIM_FFT_SIZES: the y / z line transforms k_fft_lines and k_fft_lines_split (passes B, C, D) and the x passes k_fft_x_r2c and
// k_fft_x_c2r (A, E; with the fused tail, hence the sampler's device code), with their launchers.
// The line and the x kernels stay in ONE translation unit on purpose.  From 1024 points up both run one line per wave and so share
// the instantiation wpasses<L, L + 1, 1, ...>, to which they pass different LDS addresses of the twiddle table.  Compiled apart, every
// caller in a unit passes the same address, the compiler propagates it into wpasses before it inlines, and all 84 kernels of those
// lengths come out with another instruction stream -- k_fft_lines_split<1080> and <1120> (the 2160- and 2240-point y passes) with
// two spilled registers (tools/isa_compare.py, profiles/fft_split_isa.txt).
#include "fft_host.h"
#include "poisson_dev.h"

namespace mvsim {
namespace fft {

#if defined(MVSIM_DEV_ATTRIBUTION) && defined(MVSIM_EXP_LINES_STAMPS)
// Attribution build only (tools/lines_timeline.py): shader-clock stamps of the phases of every block of the image's y passes --
// [mode FWD / INV][block][8]: start, loads requested, loads arrived, tile staged (barrier), this wave's transform done, barrier, stores
// requested.  The last launch of each mode stays in the buffer.
constexpr int STAMP_BLOCKS = 1 << 20;
__device__ unsigned long long g_line_stamps[2][STAMP_BLOCKS][8];
#define MVSIM_STAMP(k)                                                                                                       \
    do {                                                                                                                     \
        if (!SPARSE && (MODE == FWD || MODE == INV) && threadIdx.x == 0) {                                                   \
            const unsigned long long sb_ = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;                          \
            if (sb_ < (unsigned long long)STAMP_BLOCKS) g_line_stamps[MODE == INV][sb_][k] = __builtin_amdgcn_s_memtime();   \
        }                                                                                                                    \
    } while (0)
#else
#define MVSIM_STAMP(k) do { } while (0)
#endif

// Pass B's rows whose row bit is clear (k_fft_lines): 0 = a branch around the load, 1 = the load from the tile's base under a mask
// (keep4).  Both built and measured at 512^3 (profiles/row_bits_ab.txt); the product build keeps the branch.
#ifndef MVSIM_ROWBITS_MASKED
#define MVSIM_ROWBITS_MASKED 0
#endif

// where outer index `by` (a plane, or a row of the z-blocked layout seen from a pass along z: oblk != 0, see LinesArgs::src_oblk) starts
__device__ __forceinline__ long long outer_off(int by, long long outer, long long oblk)
{
    return oblk ? (long long)(by >> ZBS) * oblk + (long long)(by & (ZB - 1)) * outer : (long long)by * outer;
}

// second launch bound: as many blocks as the LDS lets a CU hold (two, or one for the long lines) must stay resident
// (w = blocks*T/256 waves per SIMD, rounded up) -- the register budget follows from that
template <int L> constexpr int lines_blocks_per_cu() { return 2 * Cfg<L>::LDS <= 160 * 1024 ? 2 : 1; }
template <class PLAN, int MODE, bool SPARSE>
__global__ __launch_bounds__(Cfg<PLAN::len>::T, (lines_blocks_per_cu<PLAN::len>() * Cfg<PLAN::len>::T + 255) / 256)
void k_fft_lines(LinesArgs p)
{
    constexpr int L = PLAN::len;
    using C = Cfg<L>;
    constexpr int NL = C::NL, LP = C::LP, T = C::T, LW = C::LW, NW = C::NW;
    constexpr int LPR = NL / 2;             // lanes per position: one float4 = two adjacent columns
    constexpr int ROWS = T / LPR;
    constexpr int NIT = (L + ROWS - 1) / ROWS;
    extern __shared__ __align__(16) float2 lds[];
    float2* buf = lds;
    float2* tw = lds + NL * LP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c2 = (tid % LPR) * 2;
    const int r0 = tid / LPR;
    float2* wbuf = buf + wave * LW * LP;    // the lines this wave transforms
    // all global loads of the tile are issued before anything waits
    // Which tile this block takes.  Tiles of 8 columns (the long lines: L > 576) move 64-BYTE row segments, i.e. two neighbouring tiles
    // share every 128-byte line they read and write.  In plain grid order those two blocks have consecutive ids, which the dispatcher
    // hands to DIFFERENT XCDs: both L2s fetch the whole line for their half (measured at 1024^3, profiles/r05_pmc_hbm_traffic_1024.txt
    // and tools/microbench/fetch_calib.hip: passes B and D read 2.0-2.1 x the bytes they need, TCC_EA0_RDREQ_128B = 2 per line, every
    // half-line write misses).  So the pair goes to ONE XCD, one directly behind the other in that XCD's dispatch order (ids b and
    // b + 8): the second half hits the line the first one brought in, and the two half-line writes meet in one L2 before they leave.
    int tile_x = (int)blockIdx.x, tile_o = (int)blockIdx.y;
    if constexpr (NL * sizeof(float2) < 128) {
        const unsigned nt = gridDim.x, total = nt * gridDim.y, b = blockIdx.y * nt + blockIdx.x;
        if ((nt & 1u) == 0 && b < (total & ~15u) && p.pair_tiles) {
            const unsigned xcd = b & 7u, slot = b >> 3;
            const unsigned lin = ((((slot >> 1) << 3) + xcd) << 1) | (slot & 1u);
            tile_x = (int)(lin % nt); tile_o = (int)(lin / nt);
        }
    }
    MVSIM_STAMP(0);
    const int by = tile_o >= p.outer_skip_lo ? tile_o + p.outer_skip_len : tile_o;
    // Pass B behind the fused rotate kernel: the plane's row-bit record (row_bits.h), block-uniform loads requested in front of the
    // plane flag so that one wait covers both -- no second trip to memory in front of the tile loads.  Row n = r0 + it * ROWS: with
    // ROWS a multiple of 32 the words of iteration `it` are static and the bit is r0's; shorter tiles ask per row (below).
    // null: every row was written -- the block takes the loop every other instance has, and no scalar load stands in front of its
    // tile loads unless there are plane flags: a volume without empty rows pays one branch per block.  Only this instance has any of it.
    constexpr bool ROWBITS = MODE == FWD && !SPARSE && row_bits_len_ok(L);
    constexpr int RB_WPI = ROWS >= 32 ? ROWS / 32 : 1;            // words of the record per load iteration
    constexpr int RB_N = (ROWBITS && ROWS >= 32) ? NIT * RB_WPI : 1;
    unsigned int rb[RB_N];
    const unsigned int* rec = nullptr;
    if constexpr (ROWBITS) {
        const int* const nzf = p.nzflags;
        const unsigned int* const rbp = p.rowbits;
        if (rbp) {
            // No branch between the two loads -- behind one the compiler waits for the flag before it asks for the record: without
            // flags the record's first word stands in and is not looked at.
            rec = rbp + (long long)by * p.rowbits_stride;
            const int flag = *(nzf ? nzf + by * p.nz_stride : reinterpret_cast<const int*>(rbp));
            if constexpr (ROWS >= 32) {
#pragma unroll
                for (int i = 0; i < RB_N; ++i) rb[i] = i < row_bits_words(L) ? rec[i] : 0u;
            }
            if (nzf && flag == 0) return;                         // an empty plane: as below
        } else if (nzf) {
            if (nzf[by * p.nz_stride] == 0) return;
        }
    } else if (p.nzflags) {
        // block-uniform (one scalar load): nothing of an empty plane is read, transformed or stored -- its readers skip it on the
        // same flags.  Pass B: flags of the input planes; pass D: the dilated flags (a plane of the z pass's output is empty iff
        // every plane its Kz taps reach is), outer index k = plane k * nz_stride
        if (p.nzflags[by * p.nz_stride] == 0) return;
    }
    const float2* sbase = p.src + outer_off(by, p.src_outer, p.src_oblk) + (long long)tile_x * NL + c2;
    float4 vp[MODE == CONVZ ? NIT : 1];
    if (MODE == CONVZ) {
        const float2* tbase = p.taps + outer_off(by, p.taps_outer, p.taps_oblk) + (long long)tile_x * NL + c2;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int n = r0 + it * ROWS;
            vp[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((L % ROWS == 0) || n < L) {
                const int t = map_src(p.pmap, n);
                if (t >= 0) vp[it] = *reinterpret_cast<const float4*>(tbase + (long long)t * p.taps_es);
            }
        }
    }
    float4 v[NIT];
    bool under_bits = false;                                      // (block-uniform; constant false in every other instance)
    if constexpr (ROWBITS) {
        if (rec) {
            // The tile under the row bits: a row is loaded iff its bit is set and is +0 bits otherwise -- it was never written, and its
            // (stale) line is not brought in.  The record's gap bits and the bits from Py on are clear: no other test.
            under_bits = true;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int n = r0 + it * ROWS;
                bool keep;
                if constexpr (ROWS >= 32) {
                    unsigned int w = rb[it * RB_WPI];
                    if constexpr (RB_WPI > 1) {
                        const int sel = __builtin_amdgcn_readfirstlane(r0 >> 5);           // wave-uniform: a wave's rows share a word
#pragma unroll
                        for (int k = 1; k < RB_WPI; ++k) w = sel == k ? rb[it * RB_WPI + k] : w;
                    }
                    keep = (w >> (r0 & 31)) & 1u;
                } else {
                    keep = n < L && ((rec[n >> 5] >> (n & 31)) & 1u);
                }
                const int sn = keep ? (p.src_mirror ? map_src(p.lmap, n) : n) : 0;
#if MVSIM_ROWBITS_MASKED
                // (the z pass's form: every load unconditional, an unwanted row from the tile's base -- certainly mapped -- and cleared)
                v[it] = keep4(*reinterpret_cast<const float4*>(sbase + line_off(sn, p.src_es, p.src_blk)), keep);
#else
                v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (keep) v[it] = *reinterpret_cast<const float4*>(sbase + line_off(sn, p.src_es, p.src_blk));
#endif
            }
        }
    }
    if (!under_bits) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int n = r0 + it * ROWS;
        v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((L % ROWS == 0) || n < L) {
            if (SPARSE) {
                const int sn = map_src(p.lmap, n);
                if (sn >= 0) v[it] = *reinterpret_cast<const float4*>(sbase + sn * p.src_es);
            } else if (n < p.gap_lo || n >= p.gap_hi) {
                // (the compiler waits for the tile's FIRST row before it requests the second -- the merge of loaded and zero registers behind
                // this branch costs it a register copy --; without the branch, all rows requested at once, passes B and D measured the same)
                const int sn = p.src_mirror ? map_src(p.lmap, n) : n;
                v[it] = *reinterpret_cast<const float4*>(sbase + line_off(sn, p.src_es, p.src_blk));
            }
        }
    }
    }
    MVSIM_STAMP(1);
    for (int i = tid; i < L; i += T) tw[i] = p.tw[i];
    MVSIM_STAMP(2);                                             // (behind the wait for the twiddles, i.e. for every load before them)
    constexpr int R1 = PLAN::R1, IT1 = (LW * (L / R1) + 63) / 64;
    float2 ps[MODE == CONVZ ? IT1 : 1][MODE == CONVZ ? R1 : 1];
    if constexpr (MODE == CONVZ) {
        // the PSF's z lines of this tile: taps into the (zeroed) lines, transform, keep the spectrum as the product's operands
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int n = r0 + it * ROWS;
            if ((L % ROWS == 0) || n < L) {
                buf[c2 * LP + n] = make_float2(vp[it].x, vp[it].y);
                buf[(c2 + 1) * LP + n] = make_float2(vp[it].z, vp[it].w);
            }
        }
        __syncthreads();
        PLAN::template run<LW>(wbuf, tw, lane);
        PLAN::template capture_first_pass<LW, IT1>(wbuf, lane, ps);
        __syncthreads();                                  // every wave has read its PSF lines: the image tile may overwrite them
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int n = r0 + it * ROWS;
        if ((L % ROWS == 0) || n < L) {
            float2 a = make_float2(v[it].x, v[it].y), b = make_float2(v[it].z, v[it].w);
            if (MODE == INV) { a = cconj(a); b = cconj(b); }
            buf[c2 * LP + n] = a;
            buf[(c2 + 1) * LP + n] = b;
        }
    }
    __syncthreads();
    MVSIM_STAMP(3);
    PLAN::template run<LW>(wbuf, tw, lane);
    MVSIM_STAMP(4);
    if (MODE == CONV) {
        // x PSF spectrum, conjugate, transform again (inverse = conj FFT conj).  The spectrum is stored tile-major
        // (each line contiguous), so the wave that owns a line streams its spectrum line straight into the first
        // radix pass of the second transform: no barrier, no extra trip through LDS.
        const float2* gl = p.spec + (((long long)tile_o * gridDim.x + tile_x) * NL + (long long)wave * LW) * L;
        PLAN::template run_op<LW>(wbuf, tw, lane, LoadMulConj{gl, L});
    }
    if constexpr (MODE == CONVZ) PLAN::template run_op<LW>(wbuf, tw, lane, LoadMulConjReg<IT1, R1>{ps});
    if (MODE == FWD && p.dst_tile_major) {
        // wave-private store: every line of the tile contiguous (consumed by LoadMulConj above)
        float2* gl = p.dst + (((long long)tile_o * gridDim.x + tile_x) * NL + (long long)wave * LW) * L;
#pragma unroll
        for (int j = 0; j < LW; ++j)
            for (int n2 = lane * 2; n2 < L; n2 += 128) {
                const float2 a = wbuf[j * LP + n2], b = wbuf[j * LP + n2 + 1];
                *reinterpret_cast<float4*>(gl + j * L + n2) = make_float4(a.x, a.y, b.x, b.y);
            }
        return;
    }
    __syncthreads();
    MVSIM_STAMP(5);
    float2* dbase = p.dst + outer_off(by, p.dst_outer, p.dst_oblk) + (long long)tile_x * NL + c2;
    const int nstore = p.store_limit > 0 ? p.store_limit : L;
    float2 sa = make_float2(0.f, 0.f), sb = make_float2(0.f, 0.f);       // CONVZ: this thread's share of its two lines' sums over z
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int n = r0 + it * ROWS;
        if (((L % ROWS == 0) || n < L) && n < nstore) {
            float2 a = buf[c2 * LP + n], b = buf[(c2 + 1) * LP + n];
            if (MODE != FWD) { a = cconj(a); b = cconj(b); }
            *reinterpret_cast<float4*>(dbase + line_off(n, p.dst_es, p.dst_blk)) = make_float4(a.x, a.y, b.x, b.y);
            if (MODE == CONVZ) { sa = cadd(sa, a); sb = cadd(sb, b); }
        }
    }
    MVSIM_STAMP(6);
    if constexpr (MODE == CONVZ) {
        if (p.sum_partial) {
            // adjustImage's sum from the spectrum side, as k_zconv's epilogue: SUM_z of every line (fp32 over a thread's <= NIT rows,
            // double from there on), weighted with wx[kx] * wy[ky], one double per block
            __syncthreads();                              // everybody has read its outputs: the tile serves as scratch
            float2* red = buf;                            // [ROWS][NL]
            red[r0 * NL + c2] = sa;
            red[r0 * NL + c2 + 1] = sb;
            __syncthreads();
            double t = 0.0;
            if (tid < NL) {
                double sre = 0.0, sim = 0.0;
                for (int r = 0; r < ROWS; ++r) { const float2 q = red[r * NL + tid]; sre += (double)q.x; sim += (double)q.y; }
                const double2 a = p.wx[tile_x * NL + tid], b = p.wy[by];
                const double wr = a.x * b.x - a.y * b.y, wi = a.x * b.y + a.y * b.x;
                t = sre * wr - sim * wi;                  // Re( s * W )
            }
            if (wave == 0) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
                if (lane == 0) p.sum_partial[(long long)tile_o * gridDim.x + tile_x] = t;
            }
        }
    }
}

// The image's y passes on lines that leave a CU room for ONE tile (L >= 1280: 8 lines x (L + 1) x 8 B > 80 KB; configs[4]'s 2160-point lines),
// round 6 -- instantiated for L = 2048, 2160 and 2240 (split_half_ok).  With one block per CU nothing overlaps: the block clock stamps (profiles/r06_lines_timeline.txt) show a 2160-point block alive for
// 60 k ticks of which 32 k are its loads, 20 k its transform and the barrier behind it, 5 k its stores -- HBM idles while it transforms, the
// SIMDs idle while it loads (2.6 TB/s per pass against 4.4 at 1080 points, where two blocks interleave).  Here the FIRST radix-2 stage of a
// decimation-in-frequency transform runs in REGISTERS as the rows arrive -- a lane loads rows n and n + L/2 of its two columns,
//     e[n] = x[n] + x[n + L/2],   o[n] = (x[n] - x[n + L/2]) w_L^n      (X[2k] = FFT_{L/2}(e)[k],  X[2k + 1] = FFT_{L/2}(o)[k])
// -- and the two half-length transforms pass through an 8-line LDS tile of L/2 points one after the other: e is staged, transformed with the
// half length's own plan and stored to the even rows; then o (kept in registers meanwhile: 36 VGPRs at 2160 points) to the odd rows.  Half
// the LDS: TWO blocks per CU, as on the 1080-point lines.  Same result as the L-point plan up to rounding (another factorisation: 2 x the
// half plan instead of the table's radices for L; measured 2-4e-7 of the range apart, tests/test_gpu_parity.py); option exp bit 8 keeps the
// one-block form for A/B runs.  tw2 = exp(-2 pi i n / L), n < L/2 (ensure_twiddles kind 1); p.tw = the HALF plan's pass table.
template <class PLANH, int MODE>
__global__ __launch_bounds__(Cfg<PLANH::len>::T, (2 * Cfg<PLANH::len>::T + 255) / 256)
void k_fft_lines_split(LinesArgs p, const float2* __restrict__ tw2)
{
    static_assert(MODE == FWD || MODE == INV, "the image's y passes");
    constexpr int LH = PLANH::len;
    using C = Cfg<LH>;
    constexpr int NL = C::NL, LP = C::LP, T = C::T, LW = C::LW;
    static_assert(2 * C::LDS <= 160 * 1024, "tiles of the half length, two per CU");
    constexpr int LPR = NL / 2;             // lanes per position: one float4 = two adjacent columns
    constexpr int ROWS = T / LPR;
    constexpr int NIT = (LH + ROWS - 1) / ROWS;
    extern __shared__ __align__(16) float2 lds[];
    float2* buf = lds;
    float2* tw = lds + NL * LP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c2 = (tid % LPR) * 2;
    const int r0 = tid / LPR;
    float2* wbuf = buf + wave * LW * LP;
    // 8-column tiles: the two tiles of a 128-byte line on one XCD, one behind the other in its dispatch order (k_fft_lines' tile pick, line
    // for line; kept as a copy: as a __forceinline__ helper it changed the code of both kernels, tools/isa_compare.py)
    int tile_x = (int)blockIdx.x, tile_o = (int)blockIdx.y;
    if constexpr (NL * sizeof(float2) < 128) {
        const unsigned nt = gridDim.x, total = nt * gridDim.y, b = blockIdx.y * nt + blockIdx.x;
        if ((nt & 1u) == 0 && b < (total & ~15u) && p.pair_tiles) {
            const unsigned xcd = b & 7u, slot = b >> 3;
            const unsigned lin = ((((slot >> 1) << 3) + xcd) << 1) | (slot & 1u);
            tile_x = (int)(lin % nt); tile_o = (int)(lin / nt);
        }
    }
    const int by = tile_o >= p.outer_skip_lo ? tile_o + p.outer_skip_len : tile_o;
    if (p.nzflags) {
        if (p.nzflags[by * p.nz_stride] == 0) return;              // an empty plane (block-uniform): see k_fft_lines
    }
    const float2* sbase = p.src + outer_off(by, p.src_outer, p.src_oblk) + (long long)tile_x * NL + c2;
    // position `pos` of the padded line, this lane's two columns.  The mirrored halo rows (pass B behind the fused rotate kernel) by ONE
    // reflection -- the launcher takes this kernel only where the halo is shorter than the image --: map_src's general path (a modulo)
    // costs the 18 address computations of a lane registers they do not have
    const int mir_n = p.src_mirror ? p.lmap.n : (1 << 30), mir_a = p.src_mirror ? p.lmap.a : (1 << 30), mir_P = p.lmap.P, mir_b = p.lmap.b;
    auto row = [&](int pos) -> float4 {
        if (pos >= p.gap_lo && pos < p.gap_hi) return make_float4(0.f, 0.f, 0.f, 0.f);
        int sn = pos;
        if (pos >= mir_a) {                                        // (never without src_mirror)
            if (pos < mir_P - mir_b) return make_float4(0.f, 0.f, 0.f, 0.f);
            sn = pos - mir_P;
        }
        sn = sn < 0 ? -sn : sn;
        sn = sn >= mir_n ? 2 * mir_n - 2 - sn : sn;
        return *reinterpret_cast<const float4*>(sbase + line_off(sn, p.src_es, p.src_blk));
    };
    float4 lo[NIT], hi[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int n = r0 + it * ROWS;
        lo[it] = hi[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((LH % ROWS == 0) || n < LH) {
            lo[it] = row(n);
            hi[it] = row(n + LH);
        }
    }
    // the first stage's twiddles w_L^n pass through the LDS region of the half plan's table, which takes their place before the first
    // transform (registers: the 72 of the tile's rows leave no room for 18 more across the loads)
    for (int i = tid; i < LH; i += T) tw[i] = tw2[i];
    __syncthreads();
    // first stage in registers: lo <- e, hi <- o (inverse transform: conj FFT conj, as everywhere)
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int n = r0 + it * ROWS;
        const float2 w = tw[((LH % ROWS == 0) || n < LH) ? n : 0];
        float2 a0 = make_float2(lo[it].x, lo[it].y), a1 = make_float2(lo[it].z, lo[it].w);
        float2 b0 = make_float2(hi[it].x, hi[it].y), b1 = make_float2(hi[it].z, hi[it].w);
        if (MODE == INV) { a0 = cconj(a0); a1 = cconj(a1); b0 = cconj(b0); b1 = cconj(b1); }
        const float2 e0 = cadd(a0, b0), e1 = cadd(a1, b1);
        const float2 o0 = cmul(csub(a0, b0), w), o1 = cmul(csub(a1, b1), w);
        lo[it] = make_float4(e0.x, e0.y, e1.x, e1.y);
        hi[it] = make_float4(o0.x, o0.y, o1.x, o1.y);
    }
    __syncthreads();                                                // every lane has read its twiddles: the plan's table takes the region
    for (int i = tid; i < LH; i += T) tw[i] = p.tw[i];
    float2* dbase = p.dst + outer_off(by, p.dst_outer, p.dst_oblk) + (long long)tile_x * NL + c2;
    const int nstore = p.store_limit > 0 ? p.store_limit : 2 * LH;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int n = r0 + it * ROWS;
            if ((LH % ROWS == 0) || n < LH) {
                const float4 v = h == 0 ? lo[it] : hi[it];
                buf[c2 * LP + n] = make_float2(v.x, v.y);
                buf[(c2 + 1) * LP + n] = make_float2(v.z, v.w);
            }
        }
        __syncthreads();
        // a wave's lines one at a time: with the odd half pinned in registers a two-line transform (its butterflies' operands side by
        // side) does not fit the 128 VGPRs of two blocks per CU; one line after the other costs the same pass iterations (60 .. 180
        // butterflies of a 540-point line fill the 64 lanes as well as 120 .. 360 of two)
#pragma unroll 1
        for (int j = 0; j < LW; ++j) PLANH::template run<1>(wbuf + j * LP, tw, lane);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = r0 + it * ROWS, n = 2 * k + h;            // output k of this half is row 2 k + h of the line
            if (((LH % ROWS == 0) || k < LH) && n < nstore) {
                float2 a = buf[c2 * LP + k], b = buf[(c2 + 1) * LP + k];
                if (MODE != FWD) { a = cconj(a); b = cconj(b); }
                *reinterpret_cast<float4*>(dbase + line_off(n, p.dst_es, p.dst_blk)) = make_float4(a.x, a.y, b.x, b.y);
            }
        }
        if (h == 0) __syncthreads();                                // the odd half overwrites the tile
    }
}
template <class PLAN>
static int launch_lines_t(mvsim_ctx* ctx, int mode, bool sparse, const LinesArgs& a, int tiles, int nouter)
{
    hipStream_t s = ctx->stream;
    using C = Cfg<PLAN::len>;
    dim3 grid(tiles, nouter), block(C::T);
#define MVSIM_LL(MODE_, SP_)                                                                 \
    do {                                                                                     \
        MVSIM_TRY(set_lds(ctx, k_fft_lines<PLAN, MODE_, SP_>, C::LDS));                           \
        hipLaunchKernelGGL((k_fft_lines<PLAN, MODE_, SP_>), grid, block, C::LDS, s, a);      \
    } while (0)
    if (mode == FWD && sparse) MVSIM_LL(FWD, true);
    else if (mode == FWD) MVSIM_LL(FWD, false);
    else if (mode == INV) MVSIM_LL(INV, false);
    else if (mode == CONVZ) MVSIM_LL(CONVZ, false);
    else MVSIM_LL(CONV, false);
#undef MVSIM_LL
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}
// the half-length plans k_fft_lines_split is instantiated for: 2 LH is a table length whose own tile leaves a CU room for one block only,
// and the 8-line tile of LH points fits twice
// (... and whose blocks are eight waves: measured, profiles/r06_split_ab.txt -- 2160 = 2 x 1080 and 2048 = 2 x 1024 gain
// 15-25 % per pass; 1792 = 2 x 896, four waves of two lines with 112 registers of rows per lane, loses in pass B what it gains in pass D).
// The same form would serve the lines of 1024 .. 1152 points for another reason -- their halves (512 .. 576 points) take SIXTEEN-column
// tiles: 128-byte rows in every load and store, two blocks per CU either way -- and was built and run for them (the kernel below takes
// 16-column half tiles as it stands: WIDE in the launcher; same tests, green).  It is NOT instantiated there: with two lines
// per wave the compiler does not fit the 72 registers of a lane's rows, their addresses and the pinned odd half into the 128 of two blocks
// per CU (104-228 bytes of scratch in every variant tried: all rows at once, groups of three with the even half written to LDS at once,
// one-reflection addressing), spills rows as they arrive -- i.e. waits for them one by one -- and pass B at 1024^3 takes 2.66 instead
// of 1.66 ms (profiles/r06_split_ab.txt).
template <int LH> constexpr bool split_half_ok()
{
    return Cfg<LH>::NL == 8 && Cfg<LH>::T == 512 && 2 * Cfg<LH>::LDS <= 160 * 1024 && 2 * Cfg<2 * LH>::LDS > 160 * 1024;
}

template <int LH, int... Rs>
static int launch_lines_split_t(mvsim_ctx* ctx, int mode, const LinesArgs& a, const float2* tw2, int tiles, int nouter)
{
    using PLANH = Plan<LH, Rs...>;
    using C = Cfg<LH>;
    // `tiles` counts tiles of the whole length's width (8 columns); the half length's tiles may be 16 wide
    constexpr int WIDE = C::NL / Cfg<2 * LH>::NL;
    if (tiles % WIDE) { set_error("custom FFT: %d tiles of 8 columns do not pair up", tiles); return MVSIM_EINVAL; }
    dim3 grid(tiles / WIDE, nouter), block(C::T);
    if (mode == FWD) {
        MVSIM_TRY(set_lds(ctx, k_fft_lines_split<PLANH, FWD>, C::LDS));
        hipLaunchKernelGGL((k_fft_lines_split<PLANH, FWD>), grid, block, C::LDS, ctx->stream, a, tw2);
    } else {
        MVSIM_TRY(set_lds(ctx, k_fft_lines_split<PLANH, INV>, C::LDS));
        hipLaunchKernelGGL((k_fft_lines_split<PLANH, INV>), grid, block, C::LDS, ctx->stream, a, tw2);
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// The launchers of a length, from the one list of lengths (null: not a length of the list; lines_split: lines of 2 L points as two
// transforms of this length, null where k_fft_lines_split is not instantiated)
using LinesFn = int (*)(mvsim_ctx*, int mode, bool sparse, const LinesArgs&, int tiles, int nouter);
using LinesSplitFn = int (*)(mvsim_ctx*, int mode, const LinesArgs&, const float2* tw2, int tiles, int nouter);

template <int LH, int... Rs> constexpr LinesSplitFn lines_split_of()
{
    if constexpr (LH >= 1024 && LH <= 1120 && split_half_ok<LH>()) return &launch_lines_split_t<LH, Rs...>;
    else return nullptr;
}

static LinesFn lines_fn(int L)
{
    switch (L) {
#define X(L_, ...) case L_: return &launch_lines_t<Plan<L_, __VA_ARGS__>>;
    MVSIM_FFT_SIZES(X)
#undef X
    default: return nullptr;
    }
}

static LinesSplitFn lines_split_fn(int LH)
{
    switch (LH) {
#define X(L_, ...) case L_: return lines_split_of<L_, __VA_ARGS__>();
    MVSIM_FFT_SIZES(X)
#undef X
    default: return nullptr;
    }
}

bool lines_split_exists(int LH) { return lines_split_fn(LH) != nullptr; }

int launch_lines(mvsim_ctx* s, int L, int mode, bool sparse, const LinesArgs& a0, int tiles, int nouter)
{
    const LinesFn lines = lines_fn(L);
    if (!lines) { set_error("custom FFT: unsupported length %d", L); return MVSIM_EINVAL; }
    LinesArgs a = a0;
    a.pair_tiles = (s->opt.exp & 4) ? 0 : 1;              // exp bit 4: 8-column tiles in plain grid order (A/B, tools/ab_env.sh)
    // lines of one block per CU: the image's y passes as two half-length transforms (k_fft_lines_split) unless exp bit 8 asks for the
    // one-block form; the PSF's sparse passes and the z-pass forms keep k_fft_lines
    // the row-bit record is read by k_fft_lines<FWD, not sparse> alone: whoever set it must get that kernel or an error, never a
    // kernel that reads the unwritten rows
    if (a.rowbits && (mode != FWD || sparse || !row_bits_len_ok(L) || a.rowbits_stride != row_bits_words(L))) {
        set_error("custom FFT: row bits on a pass that does not read them (length %d, mode %d)", L, mode);
        return MVSIM_EINVAL;
    }
    const LinesSplitFn split = (L % 2 || a.rowbits) ? nullptr : lines_split_fn(L / 2);
    if ((mode == FWD || mode == INV) && !sparse && !a.dst_tile_major && !(s->opt.exp & 8) && split && tiles % 2 == 0 &&
        (!a.src_mirror || (a.lmap.mode == 0 && a.lmap.b < a.lmap.n && a.lmap.a - a.lmap.n < a.lmap.n))) {
        const float2* tw2 = nullptr;
        MVSIM_TRY(ensure_twiddles(s, L / 2, 0, &a.tw));
        MVSIM_TRY(ensure_twiddles(s, L, 1, &tw2));
        return split(s, mode, a, tw2, tiles, nouter);
    }
    return lines(s, mode, sparse, a, tiles, nouter);
}

// ---------------------------------------------------------------------------------- x passes
// A: rows of the (virtually) padded real volume -> half spectrum along x.  M = Px/2.
// Each wave owns LW rows end to end (load, transform, post-process, store): no block barrier after the
// twiddle table is staged.  Lanes run along x with 16-B loads / stores; dst row pitch hxp (complex).
template <class PLAN>
__global__ __launch_bounds__(CfgX<PLAN::len>::T) void k_fft_x_r2c(const float* __restrict__ src, SrcMap map,
                                                                 float2* __restrict__ dst,
                                                                 const float2* __restrict__ twg,
                                                                 const float2* __restrict__ twx, int hxp,
                                                                 long long rows)
{
    constexpr int M = PLAN::len;
    using C = CfgX<M>;
    constexpr int NR = C::NL, LP = C::LP, T = C::T, LW = C::LW;
    constexpr int PAIRS = (M + 1) / 2;               // lanes needed for one row (2 complex = 4 floats per lane)
    extern __shared__ __align__(16) float2 lds[];
    float2* tw = lds + NR * LP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2* wbuf = lds + wave * LW * LP;
    const long long row0 = (long long)blockIdx.x * NR + wave * LW;

    const int nxs = map.x.n;
    const bool fast_x = (nxs & 3) == 0 && map.x.mode == 0;     // 16-B aligned interior loads
    // row offsets of the wave's LW rows (wave-uniform)
    long long offs[LW], drows[LW];                    // source offset (-1: zero row) and destination row of the wave's rows
#pragma unroll
    for (int j = 0; j < LW; ++j) {
        const long long row = row0 + j;
        offs[j] = -1;
        drows[j] = row;
        if (row < rows) {
            const unsigned py = (unsigned)(map.enum_y ? map.enum_y : map.y.P);
            const unsigned urow = (unsigned)row;      // rows = Py*Pz < 2^31
            const int z = (int)(urow / py), y = (int)(urow - (unsigned)z * py);
            const int sy = map_src(map.y, y), sz = map_src(map.z, z);
            if (sy >= 0 && sz >= 0) offs[j] = (long long)nxs * (sy + (long long)map.y.n * sz);
            drows[j] = (long long)z * map.y.P + y;
        }
    }
    // rows in the zero gap of the padded volume are never read by pass B/C (they skip the gap): if none of the
    // wave's rows carries data the wave only has to keep the block barrier company
    bool any_row = false;
#pragma unroll
    for (int j = 0; j < LW; ++j) any_row |= offs[j] >= 0;
    if (!any_row && map.x.mode == 0) {
        for (int i = tid; i < M; i += T) tw[i] = twg[i];
        __syncthreads();
        return;
    }
    // (row, lane-pair) items flattened over the wave's rows: every load iteration has all 64 lanes busy
    constexpr int LITEMS = LW * PAIRS;
    constexpr int LIT = (LITEMS + 63) / 64;
    float4 v[LIT];
#pragma unroll
    for (int it = 0; it < LIT; ++it) {
        const int e = lane + it * 64;
        const int j = e / PAIRS, q = e - j * PAIRS;   // floats 4q .. 4q+3 of padded row j
        long long off = -1;
#pragma unroll
        for (int jj = 0; jj < LW; ++jj) off = (j == jj) ? offs[jj] : off;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (off >= 0 && e < LITEMS) {
            const float* __restrict__ srow = src + off;
            if (fast_x && 4 * q + 3 < nxs) {
                t = *reinterpret_cast<const float4*>(srow + 4 * q);
            } else {
                const int s0 = map_src(map.x, 4 * q), s1 = map_src(map.x, 4 * q + 1);
                const int s2 = map_src(map.x, 4 * q + 2), s3 = map_src(map.x, 4 * q + 3);
                t.x = s0 >= 0 ? srow[s0] : 0.f;
                t.y = s1 >= 0 ? srow[s1] : 0.f;
                t.z = s2 >= 0 ? srow[s2] : 0.f;
                t.w = s3 >= 0 ? srow[s3] : 0.f;
            }
        }
        v[it] = t;
    }
    for (int i = tid; i < M; i += T) tw[i] = twg[i];
#pragma unroll
    for (int it = 0; it < LIT; ++it) {
        const int e = lane + it * 64;
        if (e < LITEMS) {
            const int j = e / PAIRS, q = e - j * PAIRS;
            wbuf[j * LP + 2 * q] = make_float2(v[it].x, v[it].y);
            if (2 * q + 1 < M) wbuf[j * LP + 2 * q + 1] = make_float2(v[it].z, v[it].w);
        }
    }
    __syncthreads();                                  // twiddle table complete (rows are wave-private)
    PLAN::template run<LW>(wbuf, tw, lane);
    // Post-process to the half spectrum, in symmetric pairs.  With s = Z[k] + conj Z[M-k], d = Z[k] - conj Z[M-k],
    // t = -i w_P^k d:   2 X[k] = s + t,   2 X[M-k] = conj(s - t).   The factor 2 is NOT divided out here: image and
    // PSF spectra both carry it and pass E folds the exact power of two into its final scale.
    // Item (row j, q) owns k = 2q, 2q+1 (one 16-B store) and the mirrored M-2q, M-2q-1 (two 8-B stores); items are
    // flattened over the wave's rows so that all lanes stay busy.
    constexpr int HQ = M / 4;
    constexpr int PITEMS = LW * HQ;
#pragma unroll 1
    for (int e = lane; e < PITEMS; e += 64) {
        const int j = e / HQ, q = e - j * HQ;
        const long long row = row0 + j;
        if (row >= rows) continue;
        long long drw = drows[0];
#pragma unroll
        for (int jj = 1; jj < LW; ++jj) drw = (j == jj) ? drows[jj] : drw;
        float2* __restrict__ drow = dst + drw * hxp;
        const float2* __restrict__ zrow = wbuf + j * LP;
        float2 lo[2], hi[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * q + h;
            const float2 zk = zrow[k];
            const float2 zm = cconj(zrow[k == 0 ? 0 : M - k]);
            const float2 sm = cadd(zk, zm), d = csub(zk, zm);
            const float2 wd = cmul(twx[k], d);
            const float2 t = make_float2(wd.y, -wd.x);                 // -i * w^k * d
            lo[h] = cadd(sm, t);
            hi[h] = cconj(csub(sm, t));                                 // element M-k (k = 0: element M)
        }
        *reinterpret_cast<float4*>(drow + 2 * q) = make_float4(lo[0].x, lo[0].y, lo[1].x, lo[1].y);
        // the mirrored pair is adjacent too (elements M-2q-1, M-2q): one 16-byte store at 8-byte alignment
        *reinterpret_cast<Pair16*>(drow + M - 2 * q - 1) = Pair16{hi[1].x, hi[1].y, hi[0].x, hi[0].y};
    }
    // per row: the middle elements not covered by the pairs (k = M/2 when M % 4 == 0) and the zero padding up
    // to hxp; flattened over rows as well
    const int nmid = M - 4 * HQ + 1;
    const int ntail = nmid + (hxp - M - 1);
    for (int e = lane; e < LW * ntail; e += 64) {
        const int j = e / ntail, u = e - j * ntail;
        const long long row = row0 + j;
        if (row >= rows) continue;
        long long drw = drows[0];
#pragma unroll
        for (int jj = 1; jj < LW; ++jj) drw = (j == jj) ? drows[jj] : drw;
        float2* __restrict__ drow = dst + drw * hxp;
        const float2* __restrict__ zrow = wbuf + j * LP;
        if (u < nmid) {
            const int k = 2 * HQ + u;
            const float2 zk = zrow[k == M ? 0 : k];
            const float2 zm = cconj(zrow[k == 0 ? 0 : M - k]);
            const float2 sm = cadd(zk, zm), d = csub(zk, zm);
            const float2 wd = cmul(twx[k], d);
            drow[k] = cadd(sm, make_float2(wd.y, -wd.x));
        } else {
            drow[M + 1 + (u - nmid)] = make_float2(0.f, 0.f);
        }
    }
}

// E: half spectrum rows -> real rows, cropped to nx, scaled; one partial sum (double) per block.
// Wave-private rows as in pass A; rows are processed in batches of RB to bound register use.
// FUSE: the rows do not go to HBM as the convolved volume; the epilogue applies adjustImage (the mean is known from the
// z pass), stores the adjusted row only if the caller wants the volume, and turns the rows of acquired planes into the
// acquisition: a copy (no noise) or phase 1 of the Poisson sampler (poisson_phase1; the rest is queued for
// k_poisson_resolve).  Saves the 8 N bytes of the convolved volume's round trip and a launch.
// SPARSE (the sparse tail, C2REmpty::sparse; never with FUSE): a row of an empty plane is not stored at all -- the sampler behind this
// pass carries the same flags and does not read it (ConvTail::sparse) -- and a block whose rows all lie in empty planes returns before
// it has requested anything but the flags.  The mode is a template argument by way of the plan's type, k_fft_x_c2r<SparseTail<PLAN>, false>:
// the instances without it keep their symbols and, line for line, their code (a third template parameter renames every instance, and a
// body shared through a device function changed the schedule of all of them).
template <class P> struct SparseTail : P {};
template <class P> struct is_sparse_tail { static constexpr bool value = false; };
template <class P> struct is_sparse_tail<SparseTail<P>> { static constexpr bool value = true; };

template <class PLAN, bool FUSE>
__global__ __launch_bounds__(CfgX<PLAN::len>::T) void k_fft_x_c2r(const float2* __restrict__ srcc,
                                                                 float* __restrict__ out,
                                                                 const float2* __restrict__ twg,
                                                                 const float2* __restrict__ twx, int hxp, int py,
                                                                 int nx, int ny, long long rows, float scale,
                                                                 double* __restrict__ partial, C2RFuse f, C2REmpty em)
{
    constexpr bool SPARSE = is_sparse_tail<PLAN>::value;
    static_assert(!(FUSE && SPARSE), "the fused tail stores no convolved volume");
    constexpr int M = PLAN::len;
    using C = CfgX<M>;
    constexpr int NR = C::NL, LP = C::LP, T = C::T, LW = C::LW, NW = C::NW;
    extern __shared__ __align__(16) float2 lds[];
    float2* tw = lds + NR * LP;
    double* red = reinterpret_cast<double*>(lds + NR * LP + M);              // NW doubles
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (SPARSE) {
        // The block's rows lie in planes zb0 .. zb1 (rows = Ny * planes < 2^31).  Up to two planes, both empty (block-uniform, two
        // scalar loads): nothing to store, and nothing waits at the barrier below because nobody gets there.  Blocks of more than two
        // planes (Ny < the block's rows / 2) decide wave by wave, further down.
        const unsigned rb0 = blockIdx.x * (unsigned)NR;
        const unsigned rb1 = (rb0 + (unsigned)NR < (unsigned)rows ? rb0 + (unsigned)NR : (unsigned)rows) - 1u;
        const int zb0 = (int)(rb0 / (unsigned)ny), zb1 = (int)(rb1 / (unsigned)ny);
        if (zb1 - zb0 <= 1 && (em.flags[zb0 * em.stride] | em.flags[zb1 * em.stride]) == 0) {
            if (partial != nullptr && tid == 0) partial[blockIdx.x] = 0.0;   // (a sum taken here: this block's share of it)
            return;
        }
    }
    float2* wbuf = lds + wave * LW * LP;
    // FUSE: behind the 32 doubles of `red`: the append counter (64 bits) and the two refusal counters, then one P1Scratch per wave
    unsigned long long* qctr = reinterpret_cast<unsigned long long*>(red + 32);
    unsigned int* qovf = reinterpret_cast<unsigned int*>(red + 33);
    constexpr size_t SCR_OFF = ((size_t)(NR * LP + M) * sizeof(float2) + 34 * sizeof(double) + 15) & ~(size_t)15;
    P1Scratch* scratch = reinterpret_cast<P1Scratch*>(reinterpret_cast<char*>(lds) + SCR_OFF);
    if (FUSE) p1_frame_zero(qctr, qovf);                                     // (the barrier behind the twiddle table comes before any append)
    // Every global load of the wave -- its share of the transform's twiddle table, the plane flags of its rows, the rows themselves and
    // the post-processing twiddles of its items -- is requested before anything waits: requested where they are used, they made a chain
    // of five dependent round trips to the caches in a block that lives for a few microseconds.
    constexpr int TWN = (M + T - 1) / T;
    float2 twreg[TWN];
#pragma unroll
    for (int n = 0; n < TWN; ++n) { const int i = tid + n * T; twreg[n] = i < M ? twg[i] : make_float2(0.f, 0.f); }
    const long long row0 = (long long)blockIdx.x * NR + wave * LW;           // output rows (y < ny, z < nz)

    // Pre-process in symmetric pairs.  With A = X[k], B = conj X[M-k], s = A + B, d = A - B, t = i w_P^{-k} d:
    //   Z[k] = s + t,  Z[M-k] = conj(s - t);  the inverse FFT runs as conj(FFT(conj Z)), so conj(Z) is staged:
    //   buf[k] = conj(s + t),  buf[M-k] = s - t.
    // Item (row j, q) owns k = 2q, 2q+1 (one 16-B load) and the mirrored M-2q, M-2q-1 (two 8-B loads), q < M/4;
    // items are flattened over the wave's rows so that every iteration has all 64 lanes busy.
    constexpr int HQ = M / 4;
    constexpr int ITEMS = LW * HQ;
    constexpr int HIT = (ITEMS + 63) / 64;
    long long offs[LW];
    int rowflag[LW];                                  // the plane flag of each of the wave's rows, all requested before the first is looked at
    int zrow_[LW];
#pragma unroll
    for (int j = 0; j < LW; ++j) {
        const long long row = row0 + j;
        const bool live = row < rows;
        const unsigned urow = live ? (unsigned)row : 0u;             // rows = Ny*Nz < 2^31
        const int z = (int)(urow / (unsigned)ny), y = (int)(urow - (unsigned)z * (unsigned)ny);
        offs[j] = live ? ((long long)z * py + y) * hxp : -1;
        zrow_[j] = __builtin_amdgcn_readfirstlane(z);                // (a wave's rows are wave-uniform)
        rowflag[j] = 1;
    }
    if (em.flags) {
        // scalar loads without a branch between them: they leave together
#pragma unroll
        for (int j = 0; j < LW; ++j) rowflag[j] = em.flags[zrow_[j] * em.stride];
    }
    // a row of an empty plane is a row of zeros -- not read (nobody wrote it), transformed to zeros
#pragma unroll
    for (int j = 0; j < LW; ++j)
        if (rowflag[j] == 0) offs[j] = -1;
    // SPARSE: ... and not stored either (bit j: row j of this wave lies in an empty plane; wave-uniform)
    static_assert(LW <= 32, "one bit per row of a wave");
    unsigned int unstored = 0u;
    if (SPARSE) {
#pragma unroll
        for (int j = 0; j < LW; ++j) unstored |= (rowflag[j] == 0 ? 1u : 0u) << j;
    }
    // every row of this wave lies in an empty plane (wave-uniform): nothing to read or transform, its outputs are zeros
    bool wave_empty = !FUSE && em.flags != nullptr;
#pragma unroll
    for (int j = 0; j < LW; ++j) wave_empty = wave_empty && (offs[j] < 0);
    constexpr int NMID = M - 4 * HQ + 1;             // middle elements not covered by the pairs (k = M/2 when M % 4 == 0)
    static_assert(LW * NMID <= 64, "one lane per middle element");
    if (!wave_empty) {
    float4 xa[HIT], xw[HIT];                          // X[2q], X[2q+1] and the twiddles w^{2q}, w^{2q+1} of the item
    Pair16 xb[HIT];                                   // X[M-2q-1], X[M-2q]: adjacent too, one 16-byte load at 8-byte alignment
    bool live_item[HIT];
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int e = lane + it * 64;
        const int j = e / HQ, q = e - j * HQ;
        long long off = -1;
#pragma unroll
        for (int jj = 0; jj < LW; ++jj) off = (j == jj) ? offs[jj] : off;
        // no branch around the loads (a merge of loaded and zero registers behind one made the compiler wait for the data at once): a
        // dead item -- a row of an empty plane, a lane beyond the items -- reads the first elements of the buffer and is zeroed below
        const bool item = off >= 0 && e < ITEMS;
        live_item[it] = item;
        const int ql = item ? q : 0;
        const float2* __restrict__ sp = srcc + (item ? off : 0);
        xw[it] = *reinterpret_cast<const float4*>(twx + 2 * (e < ITEMS ? q : 0));
        xa[it] = *reinterpret_cast<const float4*>(sp + 2 * ql);      // X[2q], X[2q+1]
        xb[it] = *reinterpret_cast<const Pair16*>(sp + M - 2 * ql - 1);
    }
    // ... and the middle elements, one per lane
    const int mj = lane / NMID, mk = 2 * HQ + (lane - mj * NMID);
    const bool mid = lane < LW * NMID && mk < M;
    long long moff = -1;
#pragma unroll
    for (int jj = 0; jj < LW; ++jj) moff = (mj == jj) ? offs[jj] : moff;
    const bool mid_row = mid && moff >= 0;
    const int mkl = mid_row ? mk : 0;                                 // (no branch around these loads either)
    const float2* __restrict__ msp = srcc + (mid_row ? moff : 0);
    const float2 ma = msp[mkl], mb = msp[M - mkl], mw = twx[mkl];
    // the transform's twiddles go to LDS now that everything is under way (the barrier below covers them)
#pragma unroll
    for (int n = 0; n < TWN; ++n) { const int i = tid + n * T; if (i < M) tw[i] = twreg[n]; }
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
        const int e = lane + it * 64;
        if (e < ITEMS) {
            const int j = e / HQ, q = e - j * HQ;
            float2* zrow = wbuf + j * LP;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = 2 * q + h;
                float2 a = h == 0 ? make_float2(xa[it].x, xa[it].y) : make_float2(xa[it].z, xa[it].w);
                float2 b = cconj(h == 0 ? make_float2(xb[it].c, xb[it].d) : make_float2(xb[it].a, xb[it].b));
                if (!live_item[it]) { a = make_float2(0.f, 0.f); b = make_float2(0.f, 0.f); }
                const float2 sm = cadd(a, b), d = csub(a, b);
                const float2 wk = h == 0 ? make_float2(xw[it].x, xw[it].y) : make_float2(xw[it].z, xw[it].w);
                const float2 wd = cmul(cconj(wk), d);                       // w^{-k} d
                const float2 t = make_float2(-wd.y, wd.x);                  // i w^{-k} d
                zrow[k] = cconj(cadd(sm, t));                               // dead rows were loaded as zeros
                if (k > 0) zrow[M - k] = csub(sm, t);
            }
        }
    }
    if (mid) {
        float2 zk = make_float2(0.f, 0.f);
        if (mid_row) {
            const float2 a = ma, b = cconj(mb);
            const float2 sm = cadd(a, b), d = csub(a, b);
            const float2 wd = cmul(cconj(mw), d);
            zk = cconj(cadd(sm, make_float2(-wd.y, wd.x)));
        }
        wbuf[mj * LP + mk] = zk;
    }
    } else {
#pragma unroll
        for (int n = 0; n < TWN; ++n) { const int i = tid + n * T; if (i < M) tw[i] = twreg[n]; }
    }
    __syncthreads();                                  // twiddle table complete (rows are wave-private)
    if (!wave_empty) PLAN::template run<LW>(wbuf, tw, lane);
    // z[n] = conj(buf[n]) = x[2n] + i x[2n+1]; lane q writes x[4q..4q+3]
    if (FUSE) {
        // nx % 4 == 0 and 16-byte aligned outputs are guaranteed by the launcher
        const double corr = f.scal[1];
        const P1Args pa = p1_frame_args(f.mul, f.k0, f.k1, f.stream, f.queue, f.segcap, qctr, qovf);
        const int nq4 = nx >> 2;
        for (int j = 0; j < LW; ++j) {
            const long long row = row0 + j;
            if (row >= rows) break;                                          // wave-uniform
            const unsigned urow = (unsigned)row;
            const int k = (int)(urow / (unsigned)ny), y = (int)(urow - (unsigned)k * (unsigned)ny);
            const bool acquired = (k % f.acq_every) == 0;
            const float2* __restrict__ zrow = wbuf + j * LP;
            const unsigned long long idx_row = (unsigned long long)nx * ((unsigned long long)y + (unsigned long long)ny * ((unsigned long long)k * (unsigned long long)f.idx_zstride));
            const unsigned long long acq_row = (unsigned long long)nx * ((unsigned long long)y + (unsigned long long)ny * (unsigned long long)(k / f.acq_every));
            for (int q0 = 0; q0 < nq4; q0 += 64) {                           // uniform trip count: phase 1 needs every lane
                const int q = q0 + lane;
                const bool valid = q < nq4;
                float vv[4] = {0.f, 0.f, 0.f, 0.f};
                if (valid) {
                    const float2 z0 = zrow[2 * q];
                    const float2 z1 = (2 * q + 1 < M) ? zrow[2 * q + 1] : make_float2(0.f, 0.f);
                    vv[0] = adjust_one(z0.x * scale, corr, f.min_value);
                    vv[1] = adjust_one(-z0.y * scale, corr, f.min_value);
                    vv[2] = adjust_one(z1.x * scale, corr, f.min_value);
                    vv[3] = adjust_one(-z1.y * scale, corr, f.min_value);
                    if (f.con) *reinterpret_cast<float4*>(f.con + row * nx + 4 * q) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                }
                if (acquired) {
                    float ov[4] = {vv[0], vv[1], vv[2], vv[3]};
                    if (f.noise)
                        poisson_phase1<false>(vv, valid, idx_row + 4ull * (unsigned long long)q, acq_row + 4ull * (unsigned long long)q, pa,
                                       &scratch[wave], lane, ov);
                    if (valid) *reinterpret_cast<float4*>(f.acq + acq_row + 4 * q) = make_float4(ov[0], ov[1], ov[2], ov[3]);
                }
            }
        }
        p1_frame_close<false>(f.qcount, qctr, qovf, f.segcap, f.noise);          // no header by design; no queue without noise (qcount is null then)
        return;
    }
    double acc = 0.0;
    const bool vec_out = (nx & 3) == 0;
    const bool want_sum = partial != nullptr;             // null: adjustImage's sum came from the z pass (early sum)
    for (int j = 0; j < LW; ++j) {
        const long long row = row0 + j;
        if (row >= rows) break;
        if (SPARSE && ((unstored >> j) & 1u) != 0u) continue;
        float* __restrict__ o = out + row * nx;
        if (wave_empty) {
            if (vec_out) for (int q = lane; 4 * q < nx; q += 64) *reinterpret_cast<float4*>(o + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
            else for (int q = lane; q < nx; q += 64) o[q] = 0.f;
            continue;
        }
        const float2* __restrict__ zrow = wbuf + j * LP;
        for (int q = lane; 4 * q < nx; q += 64) {
            const float2 z0 = zrow[2 * q];
            const float2 z1 = (2 * q + 1 < M) ? zrow[2 * q + 1] : make_float2(0.f, 0.f);
            const float x0 = z0.x * scale, x1 = -z0.y * scale, x2 = z1.x * scale, x3 = -z1.y * scale;
            if (vec_out) {
                *reinterpret_cast<float4*>(o + 4 * q) = make_float4(x0, x1, x2, x3);
                if (want_sum) acc += ((double)x0 + (double)x1) + ((double)x2 + (double)x3);
            } else {
                o[4 * q] = x0; acc += (double)x0;
                if (4 * q + 1 < nx) { o[4 * q + 1] = x1; acc += (double)x1; }
                if (4 * q + 2 < nx) { o[4 * q + 2] = x2; acc += (double)x2; }
                if (4 * q + 3 < nx) { o[4 * q + 3] = x3; acc += (double)x3; }
            }
        }
    }
    if (!want_sum) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int w = 0; w < NW; ++w) sum += red[w];
        partial[blockIdx.x] = sum;
    }
}

template <class PLAN>
static int launch_r2c_t(mvsim_ctx* ctx, const float* src, const SrcMap& map, float2* dst, const float2* tw,
                        const float2* twx, int hxp, long long rows)
{
    using C = CfgX<PLAN::len>;
    hipStream_t s = ctx->stream;
    const long long blocks = (rows + C::NL - 1) / C::NL;
    MVSIM_TRY(set_lds(ctx, k_fft_x_r2c<PLAN>, C::LDS));
    hipLaunchKernelGGL((k_fft_x_r2c<PLAN>), dim3((unsigned)blocks), dim3(C::T), C::LDS, s, src, map, dst, tw, twx, hxp, rows);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

template <class PLAN>
static int launch_c2r_t(mvsim_ctx* ctx, const float2* srcc, float* out, const float2* tw, const float2* twx, int hxp,
                        int py, int nx, int ny, long long rows, float scale, double* partial, int* nblocks, const C2RFuse* fuse,
                        const C2REmpty& em)
{
    using C = CfgX<PLAN::len>;
    const long long groups = (rows + C::NL - 1) / C::NL;
    const int blocks = (int)groups;
    *nblocks = blocks;
    hipStream_t s = ctx->stream;
    if (fuse) {
        const size_t lds = C::LDS + 32 + (size_t)C::NW * sizeof(P1Scratch);
        MVSIM_TRY(set_lds(ctx, k_fft_x_c2r<PLAN, true>, lds));
        hipLaunchKernelGGL((k_fft_x_c2r<PLAN, true>), dim3((unsigned)blocks), dim3(C::T), lds, s, srcc, out, tw, twx, hxp, py, nx, ny,
                           rows, scale, partial, *fuse, em);
    } else if (em.sparse) {
        if (!em.flags) { set_error("pass E: sparse mode without plane flags"); return MVSIM_EINVAL; }
        MVSIM_TRY(set_lds(ctx, k_fft_x_c2r<SparseTail<PLAN>, false>, C::LDS));
        hipLaunchKernelGGL((k_fft_x_c2r<SparseTail<PLAN>, false>), dim3((unsigned)blocks), dim3(C::T), C::LDS, s, srcc, out, tw, twx, hxp, py, nx, ny,
                           rows, scale, partial, C2RFuse{}, em);
    } else {
        MVSIM_TRY(set_lds(ctx, k_fft_x_c2r<PLAN, false>, C::LDS));
        hipLaunchKernelGGL((k_fft_x_c2r<PLAN, false>), dim3((unsigned)blocks), dim3(C::T), C::LDS, s, srcc, out, tw, twx, hxp, py, nx, ny,
                           rows, scale, partial, C2RFuse{}, em);
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// the launchers of a half length, from the one list of lengths
int launch_r2c(mvsim_ctx* ctx, int M, const float* src, const SrcMap& map, float2* dst, const float2* tw, const float2* twx, int hxp,
               long long rows)
{
    switch (M) {
#define X(L_, ...) case L_: return launch_r2c_t<Plan<L_, __VA_ARGS__>>(ctx, src, map, dst, tw, twx, hxp, rows);
    MVSIM_FFT_SIZES(X)
#undef X
    default: set_error("custom FFT: unsupported length %d", M); return MVSIM_EINVAL;
    }
}

int launch_c2r(mvsim_ctx* ctx, int M, const float2* srcc, float* out, const float2* tw, const float2* twx, int hxp, int py, int nx, int ny,
               long long rows, float scale, double* partial, int* nblocks, const C2RFuse* fuse, const C2REmpty& em)
{
    switch (M) {
#define X(L_, ...) \
    case L_: return launch_c2r_t<Plan<L_, __VA_ARGS__>>(ctx, srcc, out, tw, twx, hxp, py, nx, ny, rows, scale, partial, nblocks, fuse, em);
    MVSIM_FFT_SIZES(X)
#undef X
    default: set_error("custom FFT: unsupported length %d", M); return MVSIM_EINVAL;
    }
}

}  // namespace fft
}  // namespace mvsim

#if defined(MVSIM_DEV_ATTRIBUTION) && defined(MVSIM_EXP_LINES_STAMPS)
// attribution build only: the stamps of blocks [0, nblocks) of mode `inv` (see g_line_stamps), 8 words per block
extern "C" int mvsim_dev_read_line_stamps(int inv, unsigned long long* out, size_t nblocks)
{
    if (nblocks > (size_t)mvsim::fft::STAMP_BLOCKS) nblocks = (size_t)mvsim::fft::STAMP_BLOCKS;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mvsim::fft::g_line_stamps), nblocks * 8 * sizeof(unsigned long long),
                                    (size_t)(inv ? 1 : 0) * mvsim::fft::STAMP_BLOCKS * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}
#endif
