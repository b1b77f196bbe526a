// The two elementwise kernels of the multi-view Richardson-Lucy deconvolution (gfx950, wave64; api_decon.cpp drives them between the two
// convolutions of a view-iteration): the ratio phi / max(blurred, eps) and the multiplicative update with its floor, Tikhonov term and
// weight blend.  Both are HBM-bound (12 and 16 bytes per voxel): 16-byte loads and stores over the body that is 16-byte aligned for
// EVERY operand, scalar code for the head and the tail -- or for everything where the operands' alignments differ.  Every step of the
// arithmetic is rounded on its own (the build has -ffp-contract=off); DESIGN.md section 16 states the recipe.
#include "common.h"
#include "decon.h"

namespace mvsim {

namespace {

// voxels [0, head) and [tail, n) are scalar, [head, tail) are (tail - head) / 4 aligned float4s
struct DeconSplit {
    long long head, nvec, tail;
};

inline DeconSplit decon_split(int64_t n, std::initializer_list<const void*> ptrs)
{
    uintptr_t first = 0;
    bool have = false, same = true;
    for (const void* p : ptrs) {
        if (!p) continue;
        const uintptr_t m = reinterpret_cast<uintptr_t>(p) & 15;
        if (!have) { first = m; have = true; }
        else if (m != first) same = false;
    }
    DeconSplit s;
    if (!same || (first & 3) != 0) { s.head = n; s.nvec = 0; s.tail = n; return s; }
    s.head = std::min<long long>(n, (long long)(((16 - first) & 15) >> 2));
    s.nvec = (n - s.head) >> 2;
    s.tail = s.head + 4 * s.nvec;
    return s;
}

inline int decon_blocks(int64_t n)
{
    const int64_t b = (n + DECON_BLOCK_ELEMS - 1) / DECON_BLOCK_ELEMS;
    return (int)std::max<int64_t>(1, std::min<int64_t>(b, DECON_MAX_BLOCKS));
}

}  // namespace

// ---- r = phi / fmaxf(b, eps): one IEEE division; fmaxf returns eps for a NaN b ------------------------------------------------------
__device__ __forceinline__ float decon_ratio_one(float phi, float b, float eps) { return phi / fmaxf(b, eps); }

__global__ __launch_bounds__(256) void k_decon_ratio(const float* phi, const float* b, float* r, long long n, long long head,
                                                     long long nvec, long long tail, float eps)
{
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * 256;
    // r may be b: every voxel is read and written by the same thread, the read first
    const float4* phi4 = reinterpret_cast<const float4*>(phi + head);
    const float4* b4 = reinterpret_cast<const float4*>(b + head);
    float4* r4 = reinterpret_cast<float4*>(r + head);
    for (long long i = tid; i < nvec; i += nthreads) {
        const float4 p = phi4[i], q = b4[i];
        float4 o;
        o.x = decon_ratio_one(p.x, q.x, eps);
        o.y = decon_ratio_one(p.y, q.y, eps);
        o.z = decon_ratio_one(p.z, q.z, eps);
        o.w = decon_ratio_one(p.w, q.w, eps);
        r4[i] = o;
    }
    for (long long i = tid; i < head; i += nthreads) r[i] = decon_ratio_one(phi[i], b[i], eps);
    for (long long i = tail + tid; i < n; i += nthreads) r[i] = decon_ratio_one(phi[i], b[i], eps);
}

int launch_decon_ratio(hipStream_t s, const float* phi, const float* b, int64_t n, float eps, float* r)
{
    const DeconSplit sp = decon_split(n, {phi, b, r});
    hipLaunchKernelGGL(k_decon_ratio, dim3(decon_blocks(n)), dim3(256), 0, s, phi, b, r, (long long)n, sp.head, sp.nvec, sp.tail, eps);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ---- the update ------------------------------------------------------------------------------------------------------------------
struct DeconAcc {            // what one thread has seen: combined in a fixed order, so the three results repeat bit for bit
    double    sum;
    long long floored;
    float     maxc;
};

template <bool STATS>
__device__ __forceinline__ float decon_update_one(float psi, float c, bool has_w, float w, float min_value, double lambda,
                                                  double two_lambda, DeconAcc& acc)
{
    float v = psi * c;
    if (lambda > 0.0) v = (float)((sqrt(1.0 + two_lambda * (double)v) - 1.0) / lambda);
    const bool fl = !(v >= min_value);               // NaN or below the floor
    if (fl) v = min_value;
    if (has_w) {
        const float d = v - psi;
        const float t = w * d;
        v = psi + t;
    }
    if (STATS) {
        acc.sum += (double)v;
        acc.floored += fl ? 1 : 0;
        acc.maxc = fmaxf(acc.maxc, fabsf(v - psi));  // fmaxf drops a NaN difference
    }
    return v;
}

template <bool STATS>
__global__ __launch_bounds__(256) void k_decon_update(float* psi, const float* c, const float* w, long long n, long long head,
                                                      long long nvec, long long tail, float min_value, double lambda,
                                                      DeconPartial* partial)
{
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * 256;
    const double two_lambda = 2.0 * lambda;
    DeconAcc acc = {0.0, 0, 0.0f};
    float4* psi4 = reinterpret_cast<float4*>(psi + head);
    const float4* c4 = reinterpret_cast<const float4*>(c + head);
    const bool has_w = w != nullptr;
    const float4* w4 = reinterpret_cast<const float4*>(has_w ? w + head : nullptr);
    for (long long i = tid; i < nvec; i += nthreads) {
        const float4 p = psi4[i], q = c4[i];
        const float4 u = has_w ? w4[i] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        float4 o;
        o.x = decon_update_one<STATS>(p.x, q.x, has_w, u.x, min_value, lambda, two_lambda, acc);
        o.y = decon_update_one<STATS>(p.y, q.y, has_w, u.y, min_value, lambda, two_lambda, acc);
        o.z = decon_update_one<STATS>(p.z, q.z, has_w, u.z, min_value, lambda, two_lambda, acc);
        o.w = decon_update_one<STATS>(p.w, q.w, has_w, u.w, min_value, lambda, two_lambda, acc);
        psi4[i] = o;
    }
    for (long long i = tid; i < head; i += nthreads)
        psi[i] = decon_update_one<STATS>(psi[i], c[i], has_w, has_w ? w[i] : 1.0f, min_value, lambda, two_lambda, acc);
    for (long long i = tail + tid; i < n; i += nthreads)
        psi[i] = decon_update_one<STATS>(psi[i], c[i], has_w, has_w ? w[i] : 1.0f, min_value, lambda, two_lambda, acc);
    if (STATS) {
        // lanes of a wave, then the four waves, always in this order; the block's slot is its own
        __shared__ DeconAcc sh[4];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            acc.sum += __shfl_down(acc.sum, off, 64);
            acc.floored += __shfl_down(acc.floored, off, 64);
            acc.maxc = fmaxf(acc.maxc, __shfl_down(acc.maxc, off, 64));
        }
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            DeconPartial out;
            out.sum = (sh[0].sum + sh[1].sum) + (sh[2].sum + sh[3].sum);
            out.floored = (sh[0].floored + sh[1].floored) + (sh[2].floored + sh[3].floored);
            out.maxc = fmaxf(fmaxf(sh[0].maxc, sh[1].maxc), fmaxf(sh[2].maxc, sh[3].maxc));
            out.pad = 0.0f;
            partial[blockIdx.x] = out;
        }
    }
}

// one block over the per-block slots, in slot order per thread and the same tree as above
__global__ __launch_bounds__(256) void k_decon_stat_final(const DeconPartial* partial, int count, mvsim_decon_stat* stat)
{
    DeconAcc acc = {0.0, 0, 0.0f};
    for (int i = threadIdx.x; i < count; i += 256) {
        const DeconPartial p = partial[i];
        acc.sum += p.sum;
        acc.floored += p.floored;
        acc.maxc = fmaxf(acc.maxc, p.maxc);
    }
    __shared__ DeconAcc sh[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.sum += __shfl_down(acc.sum, off, 64);
        acc.floored += __shfl_down(acc.floored, off, 64);
        acc.maxc = fmaxf(acc.maxc, __shfl_down(acc.maxc, off, 64));
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        stat->sum_psi = (sh[0].sum + sh[1].sum) + (sh[2].sum + sh[3].sum);
        stat->max_change = fmaxf(fmaxf(sh[0].maxc, sh[1].maxc), fmaxf(sh[2].maxc, sh[3].maxc));
        stat->n_floored = (int64_t)((sh[0].floored + sh[1].floored) + (sh[2].floored + sh[3].floored));
    }
}

int launch_decon_update(hipStream_t s, float* psi, const float* c, const float* w, int64_t n, float min_value, double lambda,
                        DeconPartial* partial, mvsim_decon_stat* stat_dev)
{
    const DeconSplit sp = decon_split(n, {psi, c, w});   // a null w takes no part in the alignment rule
    const int blocks = decon_blocks(n);
    if (stat_dev) {
        hipLaunchKernelGGL(k_decon_update<true>, dim3(blocks), dim3(256), 0, s, psi, c, w, (long long)n, sp.head, sp.nvec, sp.tail, min_value,
                           lambda, partial);
        hipLaunchKernelGGL(k_decon_stat_final, dim3(1), dim3(256), 0, s, partial, blocks, stat_dev);
    } else {
        hipLaunchKernelGGL(k_decon_update<false>, dim3(blocks), dim3(256), 0, s, psi, c, w, (long long)n, sp.head, sp.nvec, sp.tail, min_value,
                           lambda, (DeconPartial*)nullptr);
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ---- the start value: a constant, or the mean over views of each view's mean (fp64 sums of launch_sum), floored ------------------------
__global__ __launch_bounds__(256) void k_decon_fill(float* psi, long long n, const double* sums, int n_views, float constant, float min_value)
{
    float v = constant;
    if (sums) {
        double m = 0.0;
        for (int k = 0; k < n_views; ++k) m += sums[k] / (double)n;
        v = (float)(m / (double)n_views);
    }
    if (!(v >= min_value)) v = min_value;
    const long long nthreads = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) psi[i] = v;
}

int launch_decon_fill(hipStream_t s, float* psi, int64_t n, const double* sums_dev_or_null, int n_views, float constant, float min_value)
{
    hipLaunchKernelGGL(k_decon_fill, dim3(decon_blocks(n)), dim3(256), 0, s, psi, (long long)n, sums_dev_or_null, n_views, constant, min_value);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
