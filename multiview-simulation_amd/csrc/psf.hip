// The kernels of the PSF extraction (gfx950, wave64; api_psf.cpp drives them; mvsim.h and DESIGN.md section 20 state the recipe):
//   k_psf_select   one wave of PSF_QUERIES bead lanes per block: the corner test with the block-uniform inverse, then the crowding
//                  rule as an all-pairs pass with the list staged through LDS PSF_SELECT_TILE points at a time.  A bead's byte depends
//                  on the list alone, never on which block owns it.
//   k_psf_count    one block counts the status bytes (integers: any order) and writes the record.
//   k_psf_gather   grid (tap tiles x bead chunks), lanes along the tap index (kx fastest).  The bead loop is uniform over the block --
//                  status byte and position come from block-uniform addresses, an unused bead costs one branch --, a lane keeps its
//                  tap's offset in registers for the whole chunk, adds in list order and writes ONE fp64 partial per (chunk, tap).
//   k_psf_reduce   adds the chunks' partials ascending, a lane per tap.
//   k_psf_finish   one block: the minimum under (value, index), the two-level tap sum (a thread per chunk of 256 taps, thread 0 adds
//                  the chunks' sums ascending), the normalised PSF and the record.
//   k_psf_use      the inliers of a registration scattered into a use-mask: plain stores of the same value.
// No atomics, no scratch.  Every kernel inverts the matrix itself (psf_dev.h: a few dozen operations), so no stage depends on a table
// another stage wrote; nothing here is read back by the host.
#include "psf.h"
#include "psf_dev.h"

namespace mvsim {

namespace {

__device__ __forceinline__ long long psf_count(const PsfList& L)
{
    const long long n = *L.n_dev;
    return n < 0 ? 0 : (n < L.capacity ? n : L.capacity);
}

__device__ __forceinline__ const double* psf_point(const PsfList& L, long long i) { return reinterpret_cast<const double*>(L.pos + i * L.stride); }

// step 1 as every kernel takes it; false: singular
__device__ __forceinline__ bool psf_inverse(const PsfMatrix& M, double inv[12])
{
    double m[12];
    for (int k = 0; k < 12; ++k) { m[k] = M.m_dev ? M.m_dev[k] : M.m[k]; inv[k] = 0.0; }
    return psf_invert((M.m_dev || M.given) ? m : nullptr, inv);
}

__global__ __launch_bounds__(PSF_QUERIES) void k_psf_select(PsfList L, const unsigned char* __restrict__ use, PsfMatrix M, PsfJob job,
                                                            unsigned char* __restrict__ status)
{
    __shared__ double sx[PSF_SELECT_TILE], sy[PSF_SELECT_TILE], sz[PSF_SELECT_TILE];
    const int tid = threadIdx.x;
    const int n = (int)psf_count(L);
    if ((int)blockIdx.x * PSF_QUERIES >= n) return;      // uniform
    double inv[12];
    if (!psf_inverse(M, inv)) return;                    // uniform: singular, no byte is written
    const int q = blockIdx.x * PSF_QUERIES + tid;
    const bool have = q < n;
    double p[3] = {0.0, 0.0, 0.0};
    if (have) { const double* g = psf_point(L, q); p[0] = g[0]; p[1] = g[1]; p[2] = g[2]; }
    bool crowded = false;
    if (job.crowding) {
        for (int base = 0; base < n; base += PSF_SELECT_TILE) {
            __syncthreads();
            for (int jj = tid; jj < PSF_SELECT_TILE; jj += PSF_QUERIES) {
                const int j = base + jj;
                double x[3] = {0.0, 0.0, 0.0};
                if (j < n) { const double* g = psf_point(L, j); x[0] = g[0]; x[1] = g[1]; x[2] = g[2]; }
                // a point that is not listed or not finite is staged as NaN: no comparison with it holds, so it crowds nobody -- and
                // the loop below has no branch
                const bool ok = j < n && psf_finite3(x);
                sx[jj] = ok ? x[0] : (double)NAN; sy[jj] = x[1]; sz[jj] = x[2];
            }
            __syncthreads();
#pragma unroll 8
            for (int jj = 0; jj < PSF_SELECT_TILE; ++jj)
                crowded = crowded || (base + jj != q && psf_crowds(p[0], p[1], p[2], sx[jj], sy[jj], sz[jj], job.min_separation));
        }
    }
    if (!have) return;
    int st = MVSIM_PSF_USED;
    if (!psf_finite3(p)) st = MVSIM_PSF_NONFINITE;
    else if (use && use[q] == 0) st = MVSIM_PSF_MASKED;
    else if (psf_outside(inv, job.kdim, job.dim, p)) st = MVSIM_PSF_OUTSIDE;
    else if (crowded) st = MVSIM_PSF_CROWDED;
    status[q] = (unsigned char)st;
}

__global__ __launch_bounds__(256) void k_psf_count(PsfList L, PsfMatrix M, const unsigned char* __restrict__ status,
                                                   mvsim_psf_result* __restrict__ result)
{
    __shared__ int cnt[5][256];
    const int tid = threadIdx.x;
    const int n = (int)psf_count(L);
    double inv[12];
    const bool ok = psf_inverse(M, inv);
    int c[5] = {0, 0, 0, 0, 0};
    if (ok)
        for (int i = tid; i < n; i += 256) {
            const int st = status[i];
            if (st >= 0 && st < 5) c[st] += 1;
        }
    for (int k = 0; k < 5; ++k) cnt[k][tid] = c[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
            for (int k = 0; k < 5; ++k) cnt[k][tid] += cnt[k][tid + w];
        __syncthreads();
    }
    if (tid != 0) return;
    result->minimum = 0.0;
    result->sum = 0.0;
    result->n_listed = n;
    result->n_used = cnt[MVSIM_PSF_USED][0];
    result->n_nonfinite = cnt[MVSIM_PSF_NONFINITE][0];
    result->n_masked = cnt[MVSIM_PSF_MASKED][0];
    result->n_outside = cnt[MVSIM_PSF_OUTSIDE][0];
    result->n_crowded = cnt[MVSIM_PSF_CROWDED][0];
    result->flags = ok ? 0 : MVSIM_PSF_SINGULAR;
    result->pad = 0;
}

template <bool U16> __device__ __forceinline__ double psf_load(const void* src, long long i)
{
    if (U16) return (double)(float)static_cast<const uint16_t*>(src)[i];
    return (double)static_cast<const float*>(src)[i];
}

template <bool U16>
__global__ __launch_bounds__(PSF_TAPS) void k_psf_gather(const void* __restrict__ img, PsfList L, const unsigned char* __restrict__ status,
                                                         PsfMatrix M, PsfJob job, double* __restrict__ partials)
{
    const long long n = psf_count(L);
    const long long i0 = (long long)blockIdx.y * PSF_CHUNK;
    if (i0 >= n) return;                                 // uniform: the reduce kernel reads the chunks below ceil(n / PSF_CHUNK) only
    double inv[12];
    if (!psf_inverse(M, inv)) return;                    // uniform: singular, the reduce kernel writes the zeros
    const long long taps = job.kdim[0] * job.kdim[1] * job.kdim[2];
    const long long t = (long long)blockIdx.x * PSF_TAPS + threadIdx.x;
    const bool mine = t < taps;
    const long long tt = mine ? t : 0;
    const long long kx = tt % job.kdim[0], ky = (tt / job.kdim[0]) % job.kdim[1], kz = tt / (job.kdim[0] * job.kdim[1]);
    const double jx = (double)(kx - job.kdim[0] / 2), jy = (double)(ky - job.kdim[1] / 2), jz = (double)(kz - job.kdim[2] / 2);
    const double dx = psf_delta(inv, jx, jy, jz), dy = psf_delta(inv + 4, jx, jy, jz), dz = psf_delta(inv + 8, jx, jy, jz);
    const long long Nx = job.dim[0], Ny = job.dim[1], Nz = job.dim[2];
    const double tx = (double)(Nx - 1), ty = (double)(Ny - 1), tz = (double)(Nz - 1);
    const long long i1 = i0 + PSF_CHUNK < n ? i0 + PSF_CHUNK : n;
    double acc = 0.0;
    for (long long i = i0; i < i1; ++i) {
        if (status[i] != MVSIM_PSF_USED) continue;       // uniform
        const double* g = psf_point(L, i);
        // the clamp also keeps a NaN (a caller's own status bytes may admit anything) inside the volume
        const double px = psf_clamp(g[0] + dx, tx), py = psf_clamp(g[1] + dy, ty), pz = psf_clamp(g[2] + dz, tz);
        const double fx = floor(px), fy = floor(py), fz = floor(pz);
        const double ux = px - fx, uy = py - fy, uz = pz - fz;
        const long long x0 = (long long)fx, y0 = (long long)fy, z0 = (long long)fz;
        const long long x1 = x0 + 1 < Nx ? x0 + 1 : Nx - 1, y1 = y0 + 1 < Ny ? y0 + 1 : Ny - 1, z1 = z0 + 1 < Nz ? z0 + 1 : Nz - 1;
        const long long r00 = Nx * (y0 + Ny * z0), r10 = Nx * (y1 + Ny * z0), r01 = Nx * (y0 + Ny * z1), r11 = Nx * (y1 + Ny * z1);
        const double v000 = psf_load<U16>(img, r00 + x0), v100 = psf_load<U16>(img, r00 + x1);
        const double v010 = psf_load<U16>(img, r10 + x0), v110 = psf_load<U16>(img, r10 + x1);
        const double v001 = psf_load<U16>(img, r01 + x0), v101 = psf_load<U16>(img, r01 + x1);
        const double v011 = psf_load<U16>(img, r11 + x0), v111 = psf_load<U16>(img, r11 + x1);
        const double c00 = v000 + ux * (v100 - v000), c10 = v010 + ux * (v110 - v010);
        const double c01 = v001 + ux * (v101 - v001), c11 = v011 + ux * (v111 - v011);
        const double c0 = c00 + uy * (c10 - c00), c1 = c01 + uy * (c11 - c01);
        const float s_f = (float)(c0 + uz * (c1 - c0));
        acc = acc + (double)s_f;
    }
    if (mine) partials[(long long)blockIdx.y * taps + t] = acc;
}

__global__ __launch_bounds__(256) void k_psf_reduce(PsfList L, PsfMatrix M, long long taps, const double* __restrict__ partials,
                                                    double* __restrict__ totals)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= taps) return;
    const long long n = psf_count(L);
    double inv[12];
    const long long chunks = psf_inverse(M, inv) ? (n + PSF_CHUNK - 1) / PSF_CHUNK : 0;
    double total = 0.0;
    for (long long c = 0; c < chunks; ++c) total = total + partials[c * taps + t];
    totals[t] = total;
}

__global__ __launch_bounds__(PSF_FINISH_THREADS) void k_psf_finish(const double* __restrict__ totals, PsfJob job, float* __restrict__ psf,
                                                                    mvsim_psf_result* __restrict__ result)
{
    __shared__ double sv[PSF_FINISH_THREADS];
    __shared__ long long si[PSF_FINISH_THREADS];
    __shared__ double s_sum;
    const int tid = threadIdx.x;
    const long long taps = job.kdim[0] * job.kdim[1] * job.kdim[2];
    const long long n_used = result->n_used;
    const int flags = result->flags;
    __syncthreads();                                     // every thread has read the record before thread 0 writes it
    if ((flags & MVSIM_PSF_SINGULAR) || n_used <= 0) {
        for (long long t = tid; t < taps; t += PSF_FINISH_THREADS) psf[t] = 0.0f;
        if (tid == 0) {
            result->minimum = 0.0;
            result->sum = 0.0;
            result->flags = (flags & MVSIM_PSF_SINGULAR) ? flags : (flags | MVSIM_PSF_NO_BEADS);
        }
        return;
    }
    const double den = (double)n_used;
    const long long t0 = (long long)tid * PSF_CHUNK, t1 = t0 + PSF_CHUNK < taps ? t0 + PSF_CHUNK : taps;   // this thread's chunk of taps

    double bv = (double)INFINITY;
    long long bt = 0x7fffffffffffffffLL;
    for (long long t = t0; t < t1; ++t) {
        const double mean = totals[t] / den;
        if (psf_min_less(mean, t, bv, bt)) { bv = mean; bt = t; }
    }
    sv[tid] = bv; si[tid] = bt;
    __syncthreads();
    for (int w = PSF_FINISH_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w && psf_min_less(sv[tid + w], si[tid + w], sv[tid], si[tid])) { sv[tid] = sv[tid + w]; si[tid] = si[tid + w]; }
        __syncthreads();
    }
    const double b = sv[0];
    __syncthreads();

    double s = 0.0;
    for (long long t = t0; t < t1; ++t) {
        const double mean = totals[t] / den;
        s = s + (job.subtract_min ? mean - b : mean);
    }
    sv[tid] = s;
    __syncthreads();
    if (tid == 0) {
        const long long chunks = (taps + PSF_CHUNK - 1) / PSF_CHUNK;
        double S = 0.0;
        for (long long c = 0; c < chunks; ++c) S = S + sv[c];
        s_sum = S;
    }
    __syncthreads();
    const double S = s_sum;
    const bool scale = job.normalize && S > 0.0 && fuse_finite(S);
    for (long long t = tid; t < taps; t += PSF_FINISH_THREADS) {
        const double mean = totals[t] / den;
        const double v = job.subtract_min ? mean - b : mean;
        psf[t] = scale ? (float)(v / S) : (float)v;
    }
    if (tid == 0) {
        result->minimum = b;
        result->sum = S;
        result->flags = (job.normalize && !scale) ? (flags | MVSIM_PSF_FLAT) : flags;
    }
}

__global__ __launch_bounds__(256) void k_psf_use(const mvsim_match* __restrict__ cand, const long long* __restrict__ n_cand, long long capacity,
                                                 const unsigned char* __restrict__ mask, int side, long long n_points,
                                                 unsigned char* __restrict__ use)
{
    const long long nc = *n_cand;
    const long long n = nc < 0 ? 0 : (nc < capacity ? nc : capacity);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (mask && mask[i] != 1) return;
    const long long at = side ? cand[i].b : cand[i].a;
    if (at >= 0 && at < n_points) use[at] = 1;
}

}  // namespace

int launch_psf_select(hipStream_t s, const PsfList& L, const unsigned char* use, const PsfMatrix& M, const PsfJob& job, unsigned char* status,
                      mvsim_psf_result* result)
{
    const dim3 grid((unsigned)((L.capacity + PSF_QUERIES - 1) / PSF_QUERIES));
    hipLaunchKernelGGL(k_psf_select, grid, dim3(PSF_QUERIES), 0, s, L, use, M, job, status);
    MVSIM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_psf_count, dim3(1), dim3(256), 0, s, L, M, status, result);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_psf_gather(hipStream_t s, const void* img, const PsfList& L, const unsigned char* status, const PsfMatrix& M, const PsfJob& job,
                      double* partials, double* totals)
{
    const long long taps = job.kdim[0] * job.kdim[1] * job.kdim[2];
    const dim3 grid((unsigned)((taps + PSF_TAPS - 1) / PSF_TAPS), (unsigned)((L.capacity + PSF_CHUNK - 1) / PSF_CHUNK));
    if (job.src_type == MVSIM_SRC_U16) hipLaunchKernelGGL(k_psf_gather<true>, grid, dim3(PSF_TAPS), 0, s, img, L, status, M, job, partials);
    else hipLaunchKernelGGL(k_psf_gather<false>, grid, dim3(PSF_TAPS), 0, s, img, L, status, M, job, partials);
    MVSIM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_psf_reduce, dim3((unsigned)((taps + 255) / 256)), dim3(256), 0, s, L, M, taps, partials, totals);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_psf_finish(hipStream_t s, const double* totals, const PsfJob& job, float* psf, mvsim_psf_result* result)
{
    hipLaunchKernelGGL(k_psf_finish, dim3(1), dim3(PSF_FINISH_THREADS), 0, s, totals, job, psf, result);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_psf_use_from_matches(hipStream_t s, const mvsim_match* cand, const long long* n_cand, long long capacity, const unsigned char* mask,
                                int side, long long n_points, unsigned char* use)
{
    MVSIM_HIP(hipMemsetAsync(use, 0, (size_t)n_points, s));
    hipLaunchKernelGGL(k_psf_use, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, s, cand, n_cand, capacity, mask, side, n_points, use);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
