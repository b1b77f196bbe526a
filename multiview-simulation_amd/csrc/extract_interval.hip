// extractSlices over an Interval of a volume that stays on the device (gfx950, wave64): Views.zeroMin(Views.interval(con, min, max)) of
// SimulateTileStitching.java:131-189 without the crop ever existing.  The tile's rows are narrower than the volume's, so the kernels here
// differ from those of extract.hip in ONE thing, the source address (phase 1: the pitched fetch of the group walk both files share,
// poisson_dev.h): output positions and RNG counters are those of the contiguous zero-min
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
        if (NOISE) v = poisson_voxel((double)v * mul, e.k0, e.k1, e.stream, (unsigned long long)(k * inc * plane + i));
        e.out[o] = v;
    }
}

// Phase 1 of the two-launch sampler: the group-by-group walk of poisson_dev.h (group_walk_phase1, the one k_extract_noise2_any runs) on
// the zero-min tile -- a wave slot is 64 consecutive Philox groups of ONE acquired tile plane (plane = tx * ty voxels) -- with the pitched
// fetch (FetchPitched: the rows of the volume the tile is cut from); tile-local RNG counters, no adjust.
template <bool CHECKED>
__global__ __launch_bounds__(256) void k_extract_interval_noise2(const IntervalView* __restrict__ vt, unsigned int tx, long long plane, long long nzo,
                                                                 int inc, double mul, unsigned int segcap, long long slots_per_plane)
{
    const IntervalView e = vt[blockIdx.y];
    __shared__ unsigned long long qctr;
    __shared__ unsigned int qovf[2];
    __shared__ P1Scratch scratch[4];
    p1_frame_open(&qctr, qovf);
    const P1Args pa = p1_frame_args(mul, e.k0, e.k1, e.stream, reinterpret_cast<PItem*>(e.queue), segcap, &qctr, qovf);
    const FetchPitched fetch{e.in, inc, e.plane_pitch, e.row_pitch, tx};
    group_walk_phase1<CHECKED>(fetch, e.out, plane, nzo, inc, 0ull, slots_per_plane, pa, scratch);
    p1_frame_close<true>(e.qcount, &qctr, qovf, segcap);
}

int launch_extract_interval(hipStream_t s, const IntervalPlan& pl, const IntervalView* vt, const ExtractView* rvt, int njobs, bool noise, double mul)
{
    const ExtractPlan& xp = pl.xp;
    const ExtractGeom& g = xp.geom;
    const dim3 grid(xp.blocks, (unsigned)njobs), block(256);
    if (xp.kernel == EXTRACT_K_NOISE2_ANY) {
        dispatch1(xp.checked, [&](auto C) {
            hipLaunchKernelGGL((k_extract_interval_noise2<decltype(C)::value>), grid, block, 0, s, vt, (unsigned int)pl.ig.tile[0], g.plane, g.nzo, g.inc,
                               mul, xp.segcap, xp.slots_per_plane);
        });
        // the resolver and the walk over refused voxels, on the jobs' queues: out, queue, counts and keys from the table
        ExtractOps r;
        r.vt = rvt; r.nviews = njobs; r.noise = true; r.mul = mul;
        return launch_resolve(s, xp, r);
    }
    if (xp.kernel != EXTRACT_K_SCALAR) { set_error("interval launch: a plan of kernel %d", xp.kernel); return MVSIM_EINVAL; }
    dispatch1(noise, [&](auto N) {
        hipLaunchKernelGGL((k_extract_interval<decltype(N)::value>), grid, block, 0, s, vt, (long long)pl.ig.tile[0], g.plane, g.nzo, g.inc, mul);
    });
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
