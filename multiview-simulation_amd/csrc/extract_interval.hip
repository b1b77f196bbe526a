// extractSlices over an Interval of a volume that stays on the device (gfx950, wave64): Views.zeroMin(Views.interval(con, min, max)) of
// SimulateTileStitching.java:131-189 without the crop ever existing.  The tile's rows are narrower than the volume's, so the kernels here
// differ from those of extract.hip in ONE thing, the source address: output positions and RNG counters are those of the contiguous zero-min
// tile, and everything behind phase 1 -- k_poisson_resolve, k_poisson_refused, which see only output positions and tile-local counters --
// runs on the queue unchanged (launch_resolve).  Plan: interval_plan.h; design notes: DESIGN.md 14.
#include "common.h"
#include "poisson_dev.h"

namespace mvsim {

// One voxel per lane: the bit-exact copy (snr < 0), and the sampler where extract_plan gives no queue (share 0, 2^32 voxels or more).
// Consecutive lanes read consecutive x of a row; the row starts are not 16-byte aligned, so neither form here loads wider than a float.
template <bool NOISE>
__global__ __launch_bounds__(256) void k_extract_interval(const IntervalView* __restrict__ vt, long long tx, long long plane, long long nzo, int inc,
                                                          double mul)
{
    const IntervalView e = vt[blockIdx.y];
    const long long total = plane * nzo;
    const long long nthreads = (long long)gridDim.x * 256;
    const bool small32 = total < (1ll << 32);
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += nthreads) {
        long long k, i, y;
        if (small32) {
            k = (long long)((unsigned)o / (unsigned)plane); i = o - k * plane;
            y = (long long)((unsigned)i / (unsigned)tx);
        } else {
            k = o / plane; i = o - k * plane;
            y = i / tx;
        }
        const long long x = i - y * tx;
        float v = e.in[k * inc * e.plane_pitch + y * e.row_pitch + x];
        if (NOISE) v = poisson_counter((double)v * mul, e.k0, e.k1, e.stream, (unsigned long long)(k * inc * plane + i));
        e.out[o] = v;
    }
}

// Phase 1 of the two-launch sampler, the walk of k_extract_noise2_any (extract.hip) on the zero-min tile: a wave slot is 64 consecutive
// Philox groups of ONE acquired tile plane (plane = tx * ty voxels), so a wave's outputs stay consecutive and a group never straddles a
// plane.  It may straddle a row end (tx % 4 != 0) or several rows (tx < 4): tile-local i gives y = i / tx, x = i - y * tx for the group's
// first voxel inside the plane -- one 32-bit division by the wave-uniform tx per lane (plane < 2^32 where a queue is planned) -- and a carry
// takes the other components across row ends.  Offsets into the volume are 64-bit.
template <bool CHECKED>
__global__ __launch_bounds__(256) void k_extract_interval_noise2(const IntervalView* __restrict__ vt, unsigned int tx, long long plane, long long nzo,
                                                                 int inc, double mul, unsigned int segcap, long long slots_per_plane)
{
    const IntervalView e = vt[blockIdx.y];
    __shared__ unsigned long long qctr;
    __shared__ unsigned int qovf[2];
    __shared__ P1Scratch scratch[4];
    if (threadIdx.x == 0) { qctr = 0ull; qovf[0] = 0u; qovf[1] = 0u; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    P1Args pa;
    pa.mul = mul; pa.mulf = (float)mul; pa.k0 = e.k0; pa.k1 = e.k1; pa.stream = e.stream;
    pa.seg = reinterpret_cast<PItem*>(e.queue) + (unsigned long long)blockIdx.x * segcap; pa.segcap = segcap; pa.ctr = &qctr; pa.ovf = qovf;
    const long long slots = slots_per_plane * nzo;        // wave slots: 64 groups each
    for (long long sl = (long long)blockIdx.x * 4 + wave; sl < slots; sl += (long long)gridDim.x * 4) {
        const long long k = sl / slots_per_plane, jb = sl - k * slots_per_plane;
        const unsigned long long ibase = (unsigned long long)(k * inc) * (unsigned long long)plane;        // tile-local RNG index of the plane's voxel 0
        const unsigned long long g = (ibase >> 2) + (unsigned long long)(jb * 64 + lane);                  // this lane's Philox group
        const long long i0 = (long long)(4ull * g - ibase);                                               // its first voxel inside the plane (may be < 0)
        const float* __restrict__ src = e.in + k * inc * e.plane_pitch;
        // (x, y) of the group's first voxel inside the plane; a lane past the plane's end divides too and reads nothing
        const unsigned int ifirst = (unsigned int)(i0 < 0 ? 0 : i0);
        unsigned int y = ifirst / tx, x = ifirst - y * tx;
        float vv[4];
        bool any = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long i = i0 + c;
            const bool ok = i >= 0 && i < plane;
            float v = 0.f;
            if (ok) {
                v = src[(long long)y * e.row_pitch + x];
                if (++x == tx) { x = 0u; ++y; }
            }
            vv[c] = v;
            any |= ok;
        }
        float ov[4];
        // (output position of component 0: negative for a plane's first group when the plane starts inside it, as in k_extract_noise2_any)
        poisson_phase1<CHECKED>(vv, any, 4ull * g, (unsigned long long)(k * plane + i0), pa, &scratch[wave], lane, ov);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long long i = i0 + c;
            if (i >= 0 && i < plane) e.out[k * plane + i] = ov[c];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        p1_publish(e.qcount + (size_t)QCOUNT_WORDS * blockIdx.x, qctr, qovf);
        if (blockIdx.x == 0) p1_publish_header(e.qcount, gridDim.x, segcap);
    }
}

int launch_extract_interval(hipStream_t s, const IntervalPlan& pl, const IntervalView* vt, const ExtractView* rvt, int njobs, bool noise, double mul)
{
    const ExtractPlan& xp = pl.xp;
    const ExtractGeom& g = xp.geom;
    const dim3 grid(xp.blocks, (unsigned)njobs), block(256);
    if (xp.kernel == EXTRACT_K_NOISE2_ANY) {
        if (xp.checked)
            hipLaunchKernelGGL((k_extract_interval_noise2<true>), grid, block, 0, s, vt, (unsigned int)pl.ig.tile[0], g.plane, g.nzo, g.inc, mul, xp.segcap,
                               xp.slots_per_plane);
        else
            hipLaunchKernelGGL((k_extract_interval_noise2<false>), grid, block, 0, s, vt, (unsigned int)pl.ig.tile[0], g.plane, g.nzo, g.inc, mul, xp.segcap,
                               xp.slots_per_plane);
        // the resolver and the walk over refused voxels, on the jobs' queues: out, queue, counts and keys from the table
        ExtractOps r;
        r.vt = rvt; r.nviews = njobs; r.noise = true; r.mul = mul;
        return launch_resolve(s, xp, r);
    }
    if (xp.kernel != EXTRACT_K_SCALAR) { set_error("interval launch: a plan of kernel %d", xp.kernel); return MVSIM_EINVAL; }
    if (noise) hipLaunchKernelGGL((k_extract_interval<true>), grid, block, 0, s, vt, (long long)pl.ig.tile[0], g.plane, g.nzo, g.inc, mul);
    else hipLaunchKernelGGL((k_extract_interval<false>), grid, block, 0, s, vt, (long long)pl.ig.tile[0], g.plane, g.nzo, g.inc, mul);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
