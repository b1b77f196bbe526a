// Bead images of SimulateBeads / SimulateBeads2 (SimulateBeads.java:97-205): every bead adds a Gaussian, sampled over a box
// of getSuggestedKernelDiameter(sigma) * 2 voxels per axis, to a float image -- one float addition per voxel and bead, in list
// order.  The order is part of the result (float addition does not associate), so the GPU form never scatters with atomics:
//
//   cull   one thread per (view, bead): the view's 3x4 matrix in fp64 (((x m00 + y m01) + z m02) + m03, no fused multiply-add:
//          the build compiles with -ffp-contract=off), isInsideAdjust (:120-130), the box with Java's Math.round (:178-184)
//          clipped to the image (Views.extendZero drops the writes outside it), and the number of bricks the box overlaps
//   bin    the brick binner (bricks.h) with one job per view of a chunk, keys = job-in-chunk * bricks + brick: every brick's
//          list in ascending bead order
//   render one block per brick, every voxel written exactly once (empty bricks included): the brick's beads pass through LDS
//          in chunks as per-axis factor tables exp(-(x*x) / two_sq_sigma) over the brick's extent -- +0.0 outside the bead's
//          box, which adds +0.0f to an accumulator that is never -0 and so changes nothing -- and every lane accumulates
//          acc = acc + (float)((ex * ey) * ez) * 1000.0f over its voxels in bead order; float and / or uint16 out
//
// The per-voxel sum is therefore the reference's sum bit for bit, given the same fp64 exp (device exp and a host libm may
// differ by one ulp on rare arguments).  Float denormals are kept (the build does not flush them).  Calls whose pairs would
// exceed the option "beads_pair_cap" run in chunks of whole views, or of bead ranges of one view: a range after the first
// continues from the float image the previous range left, which is the same sequential sum.
#include "bricks.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace mvsim {

namespace {

struct BeadJob {
    double    m[12];
    long long p_first;      // first point of the job in the uploaded list
    long long count;        // its beads
    long long bead_base;    // first per-bead record of the job within its chunk
    float*    out_f32;      // float image written (null: none)
    uint16_t* out_u16;      // uint16 image written (null: none)
    const float* init;      // the float image a previous bead range of the same view left (null: start from 0)
    int       has_m;        // 0: identity (renderPoints of lists that are already transformed)
    int       pad;
};

struct BeadRec {
    double loc[3];          // location after isInsideAdjust
    int    lo[3], hi[3];    // box clipped to the image, inclusive (lo > hi: nothing to add)
};

// Math.round(float) -> int (NaN -> 0, saturating), then UnsignedShortType.set(int): the low 16 bits
__device__ __forceinline__ uint16_t java_round_u16(float x)
{
    if (x != x) return 0;
    const float f = floorf(x);
    double r = (double)f + ((x - f) >= 0.5f ? 1.0 : 0.0);
    r = r > 2147483647.0 ? 2147483647.0 : (r < -2147483648.0 ? -2147483648.0 : r);
    return (uint16_t)(unsigned int)(int)r;
}

__global__ __launch_bounds__(256) void k_beads_cull(const double* __restrict__ pts, const BeadJob* __restrict__ jobs,
                                                    BeadRec* __restrict__ recs, uint32_t* __restrict__ counts, int nx, int ny,
                                                    int nz, double min0, double min1, double min2, int s0, int s1, int s2)
{
    const BeadJob& jb = jobs[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= jb.count) return;
    const double* q = pts + 3 * (jb.p_first + i);
    double p[3] = {q[0], q[1], q[2]};
    if (jb.has_m) {
        const double* m = jb.m;
        const double x = p[0], y = p[1], z = p[2];
        p[0] = ((x * m[0] + y * m[1]) + z * m[2]) + m[3];
        p[1] = ((x * m[4] + y * m[5]) + z * m[6]) + m[7];
        p[2] = ((x * m[8] + y * m[9]) + z * m[10]) + m[11];
    }
    const int dim[3] = {nx, ny, nz}, size[3] = {s0, s1, s2};
    const double mn[3] = {min0, min1, min2};
    BeadRec r;
    bool keep = true;
    for (int d = 0; d < 3; ++d) {
        p[d] -= mn[d];
        // interval.dimension(d) - 1 == max - min == the image's extent; a NaN coordinate is dropped (see mvsim.h)
        if (!(p[d] >= 0.0) || p[d] > (double)dim[d]) { keep = false; break; }
    }
    for (int d = 0; d < 3; ++d) { r.loc[d] = p[d]; r.lo[d] = 1; r.hi[d] = 0; }
    if (keep)
        for (int d = 0; d < 3; ++d) {
            const long long lo = (long long)(int)java_round_d(p[d]) - size[d] / 2;
            const long long hi = lo + size[d] - 1;
            r.lo[d] = (int)(lo < 0 ? 0 : lo);
            r.hi[d] = (int)(hi > dim[d] - 1 ? dim[d] - 1 : hi);
        }
    recs[jb.bead_base + i] = r;
    counts[jb.bead_base + i] = bricks_overlapped(r.lo, r.hi);
}

// every bead writes its (brick, bead) pairs at its scanned slot: keys = job-in-chunk * bricks + brick, values = bead record
__global__ __launch_bounds__(256) void k_beads_emit(const BeadJob* __restrict__ jobs, const BeadRec* __restrict__ recs,
                                                    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offs,
                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, BrickGrid grid)
{
    const BeadJob& jb = jobs[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= jb.count) return;
    const uint32_t g = (uint32_t)(jb.bead_base + i);
    if (counts[g] == 0) return;
    const BeadRec r = recs[g];
    brick_emit(r.lo, r.hi, grid, (uint32_t)blockIdx.y * grid.nb, g, offs[g], keys, vals);
}

__global__ __launch_bounds__(256) void k_beads_render(const BeadJob* __restrict__ jobs, const BeadRec* __restrict__ recs,
                                                      const uint32_t* __restrict__ vals, const uint32_t* __restrict__ starts,
                                                      int nx, int ny, int nz, BrickGrid grid, double t0, double t1, double t2)
{
    __shared__ double s_tab[CH][NTAB];
    __shared__ double s_loc[CH][3];
    __shared__ int s_lo[CH][3], s_hi[CH][3];

    const BeadJob& jb = jobs[blockIdx.y];
    const uint32_t brick = blockIdx.x;
    const BrickLane f = brick_lane(brick, grid, nx, ny);
    const int bz0 = f.bz0, xl = f.xl, yl = f.yl, tid = threadIdx.x;
    const bool inxy = f.inxy;
    const long long row = f.row, base = f.base;

    float acc[BZ];
#pragma unroll
    for (int k = 0; k < BZ; ++k) {
        const int z = bz0 + k;
        acc[k] = (jb.init && inxy && z < nz) ? jb.init[base + row * z] : 0.0f;
    }

    const uint32_t key = blockIdx.y * grid.nb + brick;
    const uint32_t s = starts[key], e = starts[key + 1];
    const double tss[3] = {t0, t1, t2};
    for (uint32_t c0 = s; c0 < e; c0 += CH) {
        const int m = (int)min((uint32_t)CH, e - c0);
        __syncthreads();                               // the previous chunk's tables have been read
        if (tid < m) {
            const BeadRec r = recs[vals[c0 + tid]];
            for (int d = 0; d < 3; ++d) { s_loc[tid][d] = r.loc[d]; s_lo[tid][d] = r.lo[d]; s_hi[tid][d] = r.hi[d]; }
        }
        __syncthreads();
        brick_fill_tables(m, f, tss, s_tab, s_loc, s_lo, s_hi);     // SimulateBeads.java:199-200
        __syncthreads();
        for (int c = 0; c < m; ++c) {
            const int zl = s_lo[c][2] - bz0, zh = s_hi[c][2] - bz0;
            const double exy = s_tab[c][xl] * s_tab[c][BX + yl];
#pragma unroll
            for (int k = 0; k < BZ; ++k)
                if (k >= zl && k <= zh) acc[k] = acc[k] + (float)(exy * s_tab[c][BX + BY + k]) * 1000.0f;   // :203
        }
    }
    if (!inxy) return;
#pragma unroll
    for (int k = 0; k < BZ; ++k) {
        const int z = bz0 + k;
        if (z >= nz) break;
        const long long idx = base + row * z;
        if (jb.out_f32) jb.out_f32[idx] = acc[k];
        if (jb.out_u16) jb.out_u16[idx] = java_round_u16(acc[k]);
    }
}

// LegacySimulatedBeadsImgLoader.normalize (:120-136): float min / max with `v < min` / `v > max` (NaN never taken), then
// (v - min) / (max - min) in float.  Min and max do not depend on the order of the comparisons.
constexpr int NORM_BLOCKS = 1024;

__device__ __forceinline__ void minmax_block(float& mn, float& mx, float* smn, float* smx)
{
    const int tid = threadIdx.x;
    smn[tid] = mn;
    smx[tid] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            if (smn[tid + w] < smn[tid]) smn[tid] = smn[tid + w];
            if (smx[tid + w] > smx[tid]) smx[tid] = smx[tid + w];
        }
        __syncthreads();
    }
    mn = smn[0];
    mx = smx[0];
}

__global__ __launch_bounds__(256) void k_minmax(const float* __restrict__ img, long long n, float* __restrict__ part)
{
    __shared__ float smn[256], smx[256];
    float mn = FLT_MAX, mx = -FLT_MAX;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = img[i];
        if (v < mn) mn = v;
        if (v > mx) mx = v;
    }
    minmax_block(mn, mx, smn, smx);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = mn; part[2 * blockIdx.x + 1] = mx; }
}

__global__ __launch_bounds__(256) void k_minmax_final(float* __restrict__ part, int nparts)
{
    __shared__ float smn[256], smx[256];
    float mn = FLT_MAX, mx = -FLT_MAX;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        if (part[2 * i] < mn) mn = part[2 * i];
        if (part[2 * i + 1] > mx) mx = part[2 * i + 1];
    }
    minmax_block(mn, mx, smn, smx);
    __syncthreads();
    if (threadIdx.x == 0) { part[2 * nparts] = mn; part[2 * nparts + 1] = mx; }
}

__global__ __launch_bounds__(256) void k_norm_apply(float* __restrict__ img, long long n, const float* __restrict__ mm)
{
    const float mn = mm[0], range = mm[1] - mm[0];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        img[i] = (img[i] - mn) / range;
}

struct Piece {
    int       view;
    long long first, count;   // bead range within the view's list
    bool      first_piece, last_piece;
};

}  // namespace

void beads_release(mvsim_ctx* ctx)
{
    for (DevBuf& b : ctx->beads_buf) b.release();
}

int render_beads_dev(mvsim_ctx* ctx, const double* xyz, const int64_t* view_offsets, int64_t n, const double* m12, int nviews,
                     const int64_t dim[3], const int64_t imin[3], const double sigma[3], float* const* out_f32,
                     uint16_t* const* out_u16)
{
    BrickGrid grid;
    MVSIM_TRY(brick_grid(dim, "renderBeads", &grid));
    const uint64_t nb = grid.nb;
    int size[3];
    for (int d = 0; d < 3; ++d) size[d] = suggested_kernel_diameter(sigma[d]) * 2;    // SimulateBeads.java:180
    const int64_t per_bead = bricks_spanned(size, dim, grid);

    // bead ranges of the views, then pieces of at most `cap` pairs, packed into chunks
    std::vector<long long> vfirst(nviews), vcount(nviews);
    for (int v = 0; v < nviews; ++v) {
        vfirst[v] = view_offsets ? view_offsets[v] : 0;
        vcount[v] = view_offsets ? view_offsets[v + 1] - view_offsets[v] : n;
    }
    const long long cap = ctx->opt.beads_pair_cap;
    const long long per_piece = std::max<long long>(1, cap / per_bead);
    std::vector<Piece> pieces;
    for (int v = 0; v < nviews; ++v) {
        long long a = 0;
        do {
            const long long c = std::min(per_piece, vcount[v] - a);
            pieces.push_back({v, a, c, a == 0, a + c >= vcount[v]});
            a += c;
        } while (a < vcount[v]);
    }
    bool scratch = false;
    for (const Piece& p : pieces)
        if (!(p.first_piece && p.last_piece) && !out_f32) scratch = true;
        else if (!(p.first_piece && p.last_piece) && !out_f32[p.view]) scratch = true;
    float* scratch_f32 = nullptr;
    if (scratch) {
        MVSIM_TRY(ctx->beads_buf[7].reserve((size_t)(dim[0] * dim[1] * dim[2]) * sizeof(float)));
        scratch_f32 = ctx->beads_buf[7].as<float>();
    }

    std::vector<BeadJob> jobs(pieces.size());
    std::vector<size_t> chunk_begin;             // chunk c = jobs [chunk_begin[c], chunk_begin[c + 1])
    {
        long long beads = 0;
        bool uses_scratch = false;
        std::vector<int> views_in;
        const uint64_t max_jobs = std::min<uint64_t>(1024, (((uint64_t)1 << 32) - 2) / nb);
        for (size_t i = 0; i < pieces.size(); ++i) {
            const Piece& p = pieces[i];
            const bool split = !(p.first_piece && p.last_piece);
            float* target = (out_f32 && out_f32[p.view]) ? out_f32[p.view] : (split ? scratch_f32 : nullptr);
            const bool needs_scratch = split && target == scratch_f32;
            const bool fits = chunk_begin.empty() ? false
                              : (beads + p.count) * per_bead <= cap && (!needs_scratch || !uses_scratch) &&
                                std::find(views_in.begin(), views_in.end(), p.view) == views_in.end() &&
                                (uint64_t)(i - chunk_begin.back()) < max_jobs;
            if (!fits) {
                chunk_begin.push_back(i);
                beads = 0;
                uses_scratch = false;
                views_in.clear();
            }
            BeadJob& j = jobs[i];
            if (m12) { for (int k = 0; k < 12; ++k) j.m[k] = m12[12 * p.view + k]; j.has_m = 1; }
            else { for (int k = 0; k < 12; ++k) j.m[k] = 0.0; j.has_m = 0; }
            j.p_first = vfirst[p.view] + p.first;
            j.count = p.count;
            j.bead_base = beads;
            j.init = p.first_piece ? nullptr : target;
            j.out_f32 = p.last_piece ? (out_f32 ? out_f32[p.view] : nullptr) : target;
            j.out_u16 = p.last_piece && out_u16 ? out_u16[p.view] : nullptr;
            j.pad = 0;
            beads += p.count;
            uses_scratch = uses_scratch || needs_scratch;
            views_in.push_back(p.view);
        }
        chunk_begin.push_back(pieces.size());
    }

    // workspace for the largest chunk
    long long max_beads = 1, max_slots = 1, max_keys = 1;
    const size_t nchunks = chunk_begin.size() - 1;
    for (size_t c = 0; c < nchunks; ++c) {
        long long beads = 0;
        for (size_t i = chunk_begin[c]; i < chunk_begin[c + 1]; ++i) beads += jobs[i].count;
        max_beads = std::max(max_beads, beads);
        max_slots = std::max(max_slots, beads * per_bead + 1);
        max_keys = std::max(max_keys, (long long)((chunk_begin[c + 1] - chunk_begin[c]) * nb));
    }
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));          // the workspaces may still be read by an earlier call's kernels
    BrickBins bins;
    MVSIM_TRY(bins.reserve(ctx->stream, max_beads, max_slots, max_keys, ctx->beads_buf[3], ctx->beads_buf[4], ctx->beads_buf[5], ctx->beads_buf[6],
                           "invalid argument: renderBeads: a chunk of %lld pairs (option beads_pair_cap)"));
    MVSIM_TRY(ctx->beads_buf[0].reserve(std::max<size_t>(1, (size_t)n * 3 * sizeof(double))));
    MVSIM_TRY(ctx->beads_buf[1].reserve(jobs.size() * sizeof(BeadJob)));
    MVSIM_TRY(ctx->beads_buf[2].reserve((size_t)max_beads * sizeof(BeadRec)));
    // pageable sources: synchronous copies (the caller may free its lists as soon as the call returns)
    if (n > 0) MVSIM_HIP(hipMemcpy(ctx->beads_buf[0].p, xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice));
    MVSIM_HIP(hipMemcpy(ctx->beads_buf[1].p, jobs.data(), jobs.size() * sizeof(BeadJob), hipMemcpyHostToDevice));

    const double* pts = ctx->beads_buf[0].as<double>();
    BeadRec* recs = ctx->beads_buf[2].as<BeadRec>();
    const double two_sq[3] = {2 * sigma[0] * sigma[0], 2 * sigma[1] * sigma[1], 2 * sigma[2] * sigma[2]};   // :183
    for (size_t c = 0; c < nchunks; ++c) {
        const size_t j0 = chunk_begin[c], nj = chunk_begin[c + 1] - j0;
        const BeadJob* jd = ctx->beads_buf[1].as<BeadJob>() + j0;
        long long beads = 0, most = 1;
        for (size_t i = j0; i < j0 + nj; ++i) { beads += jobs[i].count; most = std::max(most, jobs[i].count); }
        const long long slots = beads * per_bead + 1;
        const uint32_t nkeys = (uint32_t)(nj * nb);
        const dim3 gb((unsigned)((most + 255) / 256), (unsigned)nj);
        if (beads > 0) {
            hipLaunchKernelGGL(k_beads_cull, gb, dim3(256), 0, ctx->stream, pts, jd, recs, bins.counts, (int)dim[0], (int)dim[1], (int)dim[2],
                               (double)imin[0], (double)imin[1], (double)imin[2], size[0], size[1], size[2]);
            MVSIM_HIP(hipGetLastError());
            MVSIM_TRY(bins.scan(ctx->stream, beads));
            hipLaunchKernelGGL(k_beads_emit, gb, dim3(256), 0, ctx->stream, jd, recs, bins.counts, bins.offs, bins.keys[0], bins.vals[0], grid);
            MVSIM_HIP(hipGetLastError());
        }
        MVSIM_TRY(bins.finish(ctx->stream, beads, slots, nkeys));
        hipLaunchKernelGGL(k_beads_render, dim3((unsigned)nb, (unsigned)nj), dim3(256), 0, ctx->stream, jd, recs, bins.vals[1], bins.starts,
                           (int)dim[0], (int)dim[1], (int)dim[2], grid, two_sq[0], two_sq[1], two_sq[2]);
        MVSIM_HIP(hipGetLastError());
    }
    return MVSIM_OK;
}

int beads_normalize_dev(mvsim_ctx* ctx, float* img, int64_t n)
{
    MVSIM_TRY(ctx->beads_buf[6].reserve(std::max<size_t>(ctx->beads_buf[6].bytes, (2 * NORM_BLOCKS + 2) * sizeof(float))));
    float* part = ctx->beads_buf[6].as<float>();
    const int blocks = (int)std::min<int64_t>(NORM_BLOCKS, (n + 255) / 256);
    hipLaunchKernelGGL(k_minmax, dim3(blocks), dim3(256), 0, ctx->stream, img, (long long)n, part);
    hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(256), 0, ctx->stream, part, blocks);
    hipLaunchKernelGGL(k_norm_apply, dim3(std::min<int64_t>(8192, (n + 255) / 256)), dim3(256), 0, ctx->stream, img, (long long)n,
                       part + 2 * blocks);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
