// The small streaming stage operators of the per-view path (gfx950, wave64): sum/adjust, norm, the 16-bit pack of
// acquisitions, makeIsotropic, weight image, weights (rotate and attenuate: rotate.hip; slice extraction + Poisson:
// extract.hip).  All are HBM-bound; design notes and algorithmic bytes per voxel are in DESIGN.md.
#include "common.h"
#include "poisson_recipe.h"

namespace mvsim {

// ------------------------------------------------------------------------------------------------
// Sum (Tools.sumImage, Tools.java:124-132; mpicbg RealSum ~ exact-to-double): per-thread double
// accumulation, wave shuffle + LDS block tree, fixed-order final pass => deterministic.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ double block_sum_256(double v)
{
    __shared__ double sh[4];
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = ((sh[0] + sh[1]) + (sh[2] + sh[3]));
    __syncthreads();
    return r;  // valid in thread 0
}

__global__ __launch_bounds__(256) void k_sum_partial(const float* __restrict__ in, long long n,
                                                     double* __restrict__ partial)
{
    double acc = 0.0;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * 256;
    const long long n4 = ((reinterpret_cast<uintptr_t>(in) & 15) == 0) ? (n >> 2) : 0;
    const float4* in4 = reinterpret_cast<const float4*>(in);
    for (long long i = tid; i < n4; i += nthreads) {
        const float4 v = in4[i];
        acc += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
    for (long long i = (n4 << 2) + tid; i < n; i += nthreads) acc += (double)in[i];
    const double b = block_sum_256(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void k_sum_final(const double* __restrict__ partial, int count,
                                                   double* __restrict__ scal)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) acc += partial[i];
    const double b = block_sum_256(acc);
    if (threadIdx.x == 0) scal[0] = b;
}

int launch_sum(hipStream_t s, const float* in, int64_t n, double* partial, double* scal)
{
    int blocks = (int)((n / 4 + 255) / 256);
    if (blocks < 1) blocks = 1;
    if (blocks > SUM_BLOCKS) blocks = SUM_BLOCKS;
    hipLaunchKernelGGL(k_sum_partial, dim3(blocks), dim3(256), 0, s, in, (long long)n, partial);
    hipLaunchKernelGGL(k_sum_final, dim3(1), dim3(256), 0, s, partial, blocks, scal);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// adjustImage (Tools.java:143-159): corr = (double)(target - min) / (sum / n)
__global__ void k_adjust_corr(double* scal, long long n, float min_value, float target)
{
    const double avg = scal[0] / (double)n;
    scal[1] = (double)(target - min_value) / avg;
}

int launch_adjust_corr(hipStream_t s, double* scal, int64_t n, float min_value, float target)
{
    hipLaunchKernelGGL(k_adjust_corr, dim3(1), dim3(1), 0, s, scal, (long long)n, min_value, target);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

__global__ __launch_bounds__(256) void k_adjust_apply(float* __restrict__ img, long long n,
                                                      const double* __restrict__ scal, float min_value)
{
    const double corr = scal[1];
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nthreads = (long long)gridDim.x * 256;
    const long long n4 = ((reinterpret_cast<uintptr_t>(img) & 15) == 0) ? (n >> 2) : 0;
    float4* img4 = reinterpret_cast<float4*>(img);
    for (long long i = tid; i < n4; i += nthreads) {
        float4 v = img4[i];
        v.x = adjust_one(v.x, corr, min_value);
        v.y = adjust_one(v.y, corr, min_value);
        v.z = adjust_one(v.z, corr, min_value);
        v.w = adjust_one(v.w, corr, min_value);
        img4[i] = v;
    }
    for (long long i = (n4 << 2) + tid; i < n; i += nthreads) img[i] = adjust_one(img[i], corr, min_value);
}

int launch_adjust_apply(hipStream_t s, float* img, int64_t n, const double* scal, float min_value)
{
    int blocks = (int)((n / 4 + 255) / 256);
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_adjust_apply, dim3(blocks), dim3(256), 0, s, img, (long long)n, scal, min_value);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// normImage (Tools.java:112-118): img <- (float)((double)img / sum)
__global__ __launch_bounds__(256) void k_norm_apply(float* __restrict__ img, long long n,
                                                    const double* __restrict__ scal)
{
    const double sum = scal[0];
    const long long nthreads = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads)
        img[i] = (float)((double)img[i] / sum);
}

int launch_norm_apply(hipStream_t s, float* img, int64_t n, const double* scal)
{
    int blocks = (int)((n + 255) / 256);
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_norm_apply, dim3(blocks), dim3(256), 0, s, img, (long long)n, scal);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ------------------------------------------------------------------------------------------------
// Acquisitions cross PCIe as 16-bit counts (host-buffer views): Tools.poissonProcess stores raw Poisson COUNTS as floats
// (Tools.java:84), so a view's acquisition is integer-valued and -- at the reference's SNRs -- far below 65 536.  out16[i] = (uint16) in[i];
// *flag is raised when any value does not survive the round trip (a count beyond 65 535, a non-integer because the view was
// simulated without noise, a NaN): the host then fetches the float32 buffer instead.  Exact: counts are integers.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_u16(const float* __restrict__ in, unsigned short* __restrict__ out16, long long n,
                                                  unsigned int* __restrict__ flag)
{
    const long long nthreads = (long long)gridDim.x * 256;
    const long long n8 = n >> 3;
    bool bad = false;
    const float4* __restrict__ in4 = reinterpret_cast<const float4*>(in);
    uint4* __restrict__ out8 = reinterpret_cast<uint4*>(out16);
    auto cvt = [&](float v) -> unsigned int {
        const unsigned int u = (unsigned int)fminf(fmaxf(v, 0.f), 65535.f);
        bad |= __float_as_uint((float)u) != __float_as_uint(v);      // bit patterns: -0.0f does not pass for +0.0f
        return u;
    };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += nthreads) {
        const float4 a = in4[2 * i], b = in4[2 * i + 1];
        uint4 o;
        o.x = cvt(a.x) | (cvt(a.y) << 16); o.y = cvt(a.z) | (cvt(a.w) << 16);
        o.z = cvt(b.x) | (cvt(b.y) << 16); o.w = cvt(b.z) | (cvt(b.w) << 16);
        out8[i] = o;
    }
    for (long long i = (n8 << 3) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) out16[i] = (unsigned short)cvt(in[i]);
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// in: n floats (16-byte aligned), out16: n uint16 (16-byte aligned); *flag must be zero before the launch
int launch_pack_u16(hipStream_t s, const float* in, unsigned short* out16, int64_t n, unsigned int* flag)
{
    long long want = ((n >> 3) + 255) / 256;
    const int blocks = (int)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
    hipLaunchKernelGGL(k_pack_u16, dim3(blocks), dim3(256), 0, s, in, out16, (long long)n, flag);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ------------------------------------------------------------------------------------------------
// makeIsotropic (SimulateMultiViewDataset.java:144-171): z = (float)l / (float)inc (Q4), x and y
// integral => the 8-tap interpolator degenerates to two planes (weights of the x+1 / y+1 taps
// are exactly 0); mirror-single extension along z.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long mirror1(long long i, long long n)
{
    if (n == 1) return 0;
    const long long p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// One output plane per blockIdx.y: the plane's z geometry (the float division of Q4, the two source planes, their weights) is the
// same for every voxel of it -- computed once per thread from the block index instead of per voxel with a 64-bit division and two
// 64-bit modulos (0.51 -> 0.2 ms at 512^3); VEC: 16-byte rows (plane % 4 == 0, aligned buffers).  Same arithmetic per voxel.
template <bool VEC>
__global__ __launch_bounds__(256) void k_make_isotropic(const float* __restrict__ in, float* __restrict__ out,
                                                        long long plane, long long nz, long long onz, int inc)
{
    const long long z = blockIdx.y;
    const double pz = (double)((float)z / (float)inc);
    const double fz = floor(pz);
    const double w2 = pz - fz, w2n = 1.0 - w2;
    const long long z0 = mirror1((long long)fz, nz), z1 = mirror1((long long)fz + 1, nz);
    const double wa = 1.0 * 1.0 * w2n, wb = 1.0 * 1.0 * w2;
    // tap order 000 ... 001: only 000 (w = 1*1*w2n) and 001 (w = 1*1*w2) carry weight
    const long long nthreads = (long long)gridDim.x * 256;
    if (VEC) {
        const float4* __restrict__ a4 = reinterpret_cast<const float4*>(in + z0 * plane);
        const float4* __restrict__ b4 = reinterpret_cast<const float4*>(in + z1 * plane);
        float4* __restrict__ o4 = reinterpret_cast<float4*>(out + z * plane);
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < plane / 4; i += nthreads) {
            const float4 a = a4[i], b = b4[i];
            float4 r;
            r.x = (float)((double)a.x * wa); r.x += (float)((double)b.x * wb);
            r.y = (float)((double)a.y * wa); r.y += (float)((double)b.y * wb);
            r.z = (float)((double)a.z * wa); r.z += (float)((double)b.z * wb);
            r.w = (float)((double)a.w * wa); r.w += (float)((double)b.w * wb);
            o4[i] = r;
        }
    } else {
        const float* __restrict__ a = in + z0 * plane;
        const float* __restrict__ b = in + z1 * plane;
        float* __restrict__ o = out + z * plane;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < plane; i += nthreads) {
            float acc = (float)((double)a[i] * wa);
            acc += (float)((double)b[i] * wb);
            o[i] = acc;
        }
    }
}

int launch_make_isotropic(hipStream_t s, const float* in, float* out, const int64_t dim[3], int inc)
{
    const long long plane = (long long)dim[0] * dim[1];
    const long long onz = (dim[2] - 1) * inc + 1;
    if (onz > 65535) { set_error("makeIsotropic: %lld output planes exceed one launch", onz); return MVSIM_EINVAL; }
    const bool vec = plane % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long long per = vec ? plane / 4 : plane;
    long long want = (per + 255) / 256;
    const unsigned bx = (unsigned)(want < 1 ? 1 : (want > 64 ? 64 : want));
    if (vec) hipLaunchKernelGGL(k_make_isotropic<true>, dim3(bx, (unsigned)onz), dim3(256), 0, s, in, out, plane, (long long)dim[2], onz, inc);
    else hipLaunchKernelGGL(k_make_isotropic<false>, dim3(bx, (unsigned)onz), dim3(256), 0, s, in, out, plane, (long long)dim[2], onz, inc);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// computeWeightImage (SimulateMultiViewDataset.java:280-316): cosine ramp along y.
__global__ __launch_bounds__(256) void k_weight_image(float* __restrict__ out, int nx, int ny, long long total)
{
    const long long nthreads = (long long)gridDim.x * 256;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += nthreads) {
        const int y = (int)((o / nx) % ny);
        const int l = ny - y - 1;
        float value;
        if (l < ny / 2) value = 1.0f;
        else if (l > ny / 2 + 40) value = 0.0f;
        else {
            const double pos = ((double)(l - ny / 2) / 40.0) * 3.141592653589793;
            value = (float)((cos(pos) + 1.0) / 2.0);
        }
        out[o] = value;
    }
}

int launch_weight_image(hipStream_t s, float* out, const int64_t dim[3])
{
    const long long total = (long long)dim[0] * dim[1] * dim[2];
    long long want = (total + 255) / 256;
    int blocks = (int)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
    hipLaunchKernelGGL(k_weight_image, dim3(blocks), dim3(256), 0, s, out, (int)dim[0], (int)dim[1], total);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

// ------------------------------------------------------------------------------------------------
// Cross-view weight normalisation (SimulateMultiViewDataset.java:615-640): per voxel, float sum over the
// views in view order; zero sum -> all zero, else w <- min(1, osem * (w / sum)).
// ------------------------------------------------------------------------------------------------
struct ViewPtrs {
    float* p[MVSIM_MAX_VIEWS];
};

template <bool HAVE_SUM, bool WRITE_SUM_ONLY>
__global__ __launch_bounds__(256) void k_weights(ViewPtrs vp, int nv, long long n, const float* __restrict__ sum_in,
                                                 float* __restrict__ sum_out, float osem)
{
    const long long nthreads = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += nthreads) {
        float sum;
        if (HAVE_SUM) {
            sum = sum_in[i];
        } else {
            sum = 0.0f;
            for (int v = 0; v < nv; ++v) sum += vp.p[v][i];
        }
        if (WRITE_SUM_ONLY) { sum_out[i] = sum; continue; }
        for (int v = 0; v < nv; ++v) {
            float w = 0.0f;
            if (sum != 0.0f) w = fminf(1.0f, osem * (vp.p[v][i] / sum));
            vp.p[v][i] = w;
        }
    }
}

int launch_weights(hipStream_t s, float* const* views, int nv, int64_t n, const float* sum_in, float* sum_out,
                   float osem, bool sum_only)
{
    ViewPtrs vp;
    for (int v = 0; v < MVSIM_MAX_VIEWS; ++v) vp.p[v] = v < nv ? views[v] : nullptr;
    long long want = (n + 255) / 256;
    int blocks = (int)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
    if (sum_only)
        hipLaunchKernelGGL((k_weights<false, true>), dim3(blocks), dim3(256), 0, s, vp, nv, (long long)n, sum_in, sum_out, osem);
    else if (sum_in)
        hipLaunchKernelGGL((k_weights<true, false>), dim3(blocks), dim3(256), 0, s, vp, nv, (long long)n, sum_in, sum_out, osem);
    else
        hipLaunchKernelGGL((k_weights<false, false>), dim3(blocks), dim3(256), 0, s, vp, nv, (long long)n, sum_in, sum_out, osem);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
