// The extract + Poisson stage (gfx950, wave64): extractSlices with adjustImage on the fly and the two-launch Poisson sampler -- the four
// kernels of phase 1, the resolver, the walk over what full segments refused -- and the one launcher that runs an ExtractPlan
// (extract_plan.h).  The arithmetic of a voxel: poisson_recipe.h; phase 1, its block frame, the group walk and the resolver's loop:
// poisson_dev.h; design notes: DESIGN.md 4.4.
#include <vector>

#include "common.h"
#include "poisson_dev.h"

namespace mvsim {

// Stacked views (vt != null, blockIdx.y = view): the view's operands from the device table, over the kernel's own.  One helper per
// operand set; without a table the operands stay what the kernel was launched with.
__device__ __forceinline__ void view_operands(const ExtractView* __restrict__ vt, const float* __restrict__& in, float* __restrict__& out,
                                              const double* __restrict__& scal, uint32_t& k0, uint32_t& k1, uint32_t& stream)
{
    if (vt) { const ExtractView e = vt[blockIdx.y]; in = e.in; out = e.out; scal = e.scal; k0 = e.k0; k1 = e.k1; stream = e.stream; }
}

__device__ __forceinline__ void view_operands(const ExtractView* __restrict__ vt, const float* __restrict__& in, float* __restrict__& out,
                                              const double* __restrict__& scal, uint32_t& k0, uint32_t& k1, uint32_t& stream,
                                              PItem* __restrict__& queue, unsigned int* __restrict__& qcount)
{
    if (vt) {
        const ExtractView e = vt[blockIdx.y];
        in = e.in; out = e.out; scal = e.scal; k0 = e.k0; k1 = e.k1; stream = e.stream;
        queue = reinterpret_cast<PItem*>(e.queue); qcount = e.qcount;
    }
}

// The ResolveJob set.  QUEUE == false: k_poisson_refused, which reads no queue, does not take the field.
template <bool QUEUE>
__device__ __forceinline__ void view_job(const ExtractView* __restrict__ vt, ResolveJob& job)
{
    if (vt) {
        const ExtractView e = vt[blockIdx.y];
        job.out = e.out; job.qcount = e.qcount; job.k0 = e.k0; job.k1 = e.k1; job.stream = e.stream;
        if (QUEUE) job.queue = reinterpret_cast<const PItem*>(e.queue);
    }
}

// ------------------------------------------------------------------------------------------------
// extractSlices + adjust + Poisson (SimulateMultiViewDataset.java:195-251, Tools.java:73-86):
// out[x,y,k] = f(in[x,y,k*inc]);  ADJUST applies the two adjustImage passes on the fly (fused
// path: the scaled volume is never materialised); NOISE draws Poisson((double)v * mul).
// ------------------------------------------------------------------------------------------------
template <bool ADJUST, bool NOISE>
__global__ __launch_bounds__(256) void k_extract(const float* __restrict__ in, float* __restrict__ out,
                                                 long long plane, long long nzo, int inc, int idx_inc,
                                                 const double* __restrict__ scal, float min_value, double mul,
                                                 uint32_t k0, uint32_t k1, uint32_t stream,
                                                 unsigned long long index_offset, const ExtractView* __restrict__ vt)
{
    view_operands(vt, in, out, scal, k0, k1, stream);
    double corr = 1.0;
    if (ADJUST) corr = scal[1];
    const long long total = plane * nzo;
    const long long nthreads = (long long)gridDim.x * 256;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += nthreads) {
        const long long k = o / plane;
        const long long i = o - k * plane;
        const long long src = k * inc * plane + i;
        float v = in[src];
        if (ADJUST) v = adjust_one(v, corr, min_value);
        if (NOISE) v = poisson_voxel((double)v * mul, k0, k1, stream, index_offset + (unsigned long long)(k * idx_inc * plane + i));
        out[o] = v;
    }
}

// Vector form: 4 consecutive voxels per lane (16-B loads/stores); the lane's 4 voxels are exactly one
// Philox group.  Requires plane % 4 == 0, index_offset % 4 == 0 and 16-B aligned buffers.
template <bool ADJUST, bool NOISE>
__global__ __launch_bounds__(256) void k_extract4(const float* __restrict__ in, float* __restrict__ out,
                                                  long long plane4, long long nzo, int inc, int idx_inc,
                                                  const double* __restrict__ scal, float min_value, double mul,
                                                  uint32_t k0, uint32_t k1, uint32_t stream,
                                                  unsigned long long index_offset, const ExtractView* __restrict__ vt)
{
    view_operands(vt, in, out, scal, k0, k1, stream);
    double corr = 1.0;
    if (ADJUST) corr = scal[1];
    const long long total4 = plane4 * nzo;
    const long long nthreads = (long long)gridDim.x * 256;
    const float4* __restrict__ in4 = reinterpret_cast<const float4*>(in);
    float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
    const bool small32 = total4 < (1ll << 32);
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total4; o += nthreads) {
        long long src4 = o, idx4 = o;                 // where the voxels are read / what the RNG counter says they are
        if (inc != 1 || idx_inc != 1) {
            const long long k = small32 ? (long long)((unsigned)o / (unsigned)plane4) : o / plane4;
            src4 = k * inc * plane4 + (o - k * plane4);
            idx4 = k * idx_inc * plane4 + (o - k * plane4);
        }
        float4 v = in4[src4];
        if (ADJUST) {
            v.x = adjust_one(v.x, corr, min_value);
            v.y = adjust_one(v.y, corr, min_value);
            v.z = adjust_one(v.z, corr, min_value);
            v.w = adjust_one(v.w, corr, min_value);
        }
        if (NOISE) {
            const double lam[4] = {(double)v.x * mul, (double)v.y * mul, (double)v.z * mul, (double)v.w * mul};
            float cnt[4];
            poisson_counter4(lam, k0, k1, stream, index_offset + 4ull * (unsigned long long)idx4, cnt);
            v = make_float4(cnt[0], cnt[1], cnt[2], cnt[3]);
        }
        out4[o] = v;
    }
}

// Noise form for production sizes, two launches.
//   k_extract4_noise2: every lane busy -- adjust, then phase 1 of the sampler (poisson_dev.h: poisson_phase1): the
//                      "count is 0" shortcut of the low-lambda inversion, and the attempt-0 squeeze of PTRS run densely
//                      over the wave's bright voxels (ballot compaction into a wave-private LDS list).  The ~1/3 of
//                      bright voxels that still need the exact test or a retry, and the few low-lambda voxels whose
//                      count may be >= 1, are appended to a work queue in HBM (per-block segments, LDS append counters:
//                      one global counter would serialise at ~88 atomics/us chip-wide; bright items grow from the front
//                      of the segment, inversion items from its back).
//   k_poisson_resolve: one queue item per lane, looped until resolved; no LDS, no barriers, full occupancy, and
//                      every lane starts with real work -- the divergent fp64 code (logs, divisions) no longer
//                      runs once per voxel slot with 1-in-7 lanes active.
// Same arithmetic per (voxel, attempt) as poisson_voxel: bit-identical counts.
template <bool ADJUST, bool CHECKED>
__global__ __launch_bounds__(256) void k_extract4_noise2(const float* __restrict__ in, float* __restrict__ out,
                                                         long long plane4, long long nzo, int inc, int idx_inc,
                                                         const double* __restrict__ scal, float min_value, double mul,
                                                         uint32_t k0, uint32_t k1, uint32_t stream,
                                                         unsigned long long index_offset, PItem* __restrict__ queue,
                                                         unsigned int* __restrict__ qcount, unsigned int segcap,
                                                         const ExtractView* __restrict__ vt)
{
    view_operands(vt, in, out, scal, k0, k1, stream, queue, qcount);
    __shared__ unsigned long long qctr;
    __shared__ unsigned int qovf[2];
    __shared__ P1Scratch scratch[4];
    p1_frame_open(&qctr, qovf);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const P1Args pa = p1_frame_args(mul, k0, k1, stream, queue, segcap, &qctr, qovf);
    double corr = 1.0;
    if (ADJUST) corr = scal[1];
    const long long total4 = plane4 * nzo;
    const long long nthreads = (long long)gridDim.x * 256;
    const float4* __restrict__ in4 = reinterpret_cast<const float4*>(in);
    float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
    const bool small32 = total4 < (1ll << 32);
    // the trip count is uniform per wave (lanes past the end carry invalid voxels): ballots need every lane
    const long long wave_first = (long long)blockIdx.x * 256 + wave * 64;
    for (long long o0 = wave_first; o0 < total4; o0 += nthreads) {
        const long long o = o0 + lane;
        const bool valid = o < total4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        long long src4 = o, idx4 = o;                 // where the voxels are read / what the RNG counter says they are
        if (valid) {
            if (inc != 1 || idx_inc != 1) {
                const long long k = small32 ? (long long)((unsigned)o / (unsigned)plane4) : o / plane4;
                src4 = k * inc * plane4 + (o - k * plane4);
                idx4 = k * idx_inc * plane4 + (o - k * plane4);
            }
            v = in4[src4];
            if (ADJUST) {
                v.x = adjust_one(v.x, corr, min_value);
                v.y = adjust_one(v.y, corr, min_value);
                v.z = adjust_one(v.z, corr, min_value);
                v.w = adjust_one(v.w, corr, min_value);
            }
        }
        const float vv[4] = {v.x, v.y, v.z, v.w};
        float ov[4];
        poisson_phase1<CHECKED>(vv, valid, index_offset + 4ull * (unsigned long long)idx4, 4ull * (unsigned long long)o, pa, &scratch[wave], lane, ov);
        if (valid) out4[o] = make_float4(ov[0], ov[1], ov[2], ov[3]);
    }
    p1_frame_close<true>(qcount, &qctr, qovf, segcap);
}

// The same two-launch sampler for planes that are no multiple of four voxels (the reference's own 289^3 run: 83 521 voxels per
// plane) or buffers that are not 16-byte aligned: the group-by-group walk of poisson_dev.h (group_walk_phase1) over contiguous planes
// (scalar loads and stores under a mask; the components outside the plane enter phase 1 as zeros, which it ignores).  Same arithmetic
// per (voxel, attempt) as every other form: bit-identical counts.
template <bool ADJUST, bool CHECKED>
__global__ __launch_bounds__(256) void k_extract_noise2_any(const float* __restrict__ in, float* __restrict__ out,
                                                            long long plane, long long nzo, int inc, int idx_inc,
                                                            const double* __restrict__ scal, float min_value, double mul,
                                                            uint32_t k0, uint32_t k1, uint32_t stream,
                                                            unsigned long long index_offset, PItem* __restrict__ queue,
                                                            unsigned int* __restrict__ qcount, unsigned int segcap,
                                                            long long slots_per_plane, const ExtractView* __restrict__ vt)
{
    view_operands(vt, in, out, scal, k0, k1, stream, queue, qcount);
    __shared__ unsigned long long qctr;
    __shared__ unsigned int qovf[2];
    __shared__ P1Scratch scratch[4];
    p1_frame_open(&qctr, qovf);
    const P1Args pa = p1_frame_args(mul, k0, k1, stream, queue, segcap, &qctr, qovf);
    const FetchContiguous<ADJUST> fetch{in, inc, ADJUST ? scal[1] : 1.0, min_value};
    group_walk_phase1<CHECKED>(fetch, out, plane, nzo, idx_inc, index_offset, slots_per_plane, pa, scratch);
    p1_frame_close<true>(qcount, &qctr, qovf, segcap);
}

// Phase 1 behind a sparse tail (ExtractOps::empty_flags; extract_plan.h): the two kernels above for a buffer whose empty planes pass E has
// not stored.  Kernels of their own -- the mode is not an argument of the unflagged ones, whose code stays what it was -- for single
// views that are adjusted on the fly (the buffer is the context's workspace), planes of at least 256 voxels and fewer than 2^32 outputs
// (every queue launch).  flags[j * fstride] is the flag of plane j of `in`.
//
// k_extract4_noise2_sparse: a slot is 64 consecutive float4 groups, of plane k from lane 0 and of plane k + 1 from lane `first` on
// (first >= 64: one plane; a plane holds at least 64 groups, so never a third).  Where the slot starts -- plane k, group rem of it --
// is carried from trip to trip in scalar registers: the grid stride is dq planes and dr groups.  The flags of the wave's next 32 trips
// are ONE per-lane load and a ballot (tail_mask_ask: before the first voxel load, and again every 32 trips): a trip shifts the mask and
// tests a bit -- no flag load, no flag register and no clamp in the loop.
//   ALIGNED (planes of a multiple of 64 groups; the launcher picks the instance from the plan): a slot lies in ONE plane and no slot is
//     cut by the end of the output -- no second plane, no per-lane flag, no `valid` mask; the lane's address is a scalar base + lane.
//   else the per-lane form: the lanes from `first` on ask the mask's second half, a lane of an empty plane does not read -- its four
//     voxels are the plane's one value -- and lanes past the end of the output are masked out.
//   * the slot lies in one empty plane of regime 0 or 1: poisson_phase1_empty -- no read, no adjust, no regime test per voxel;
//   * else the ordinary phase 1 (regime 2, a caller with a large min_value: on the constant, still without a read).
// What the trip loop carries in scalar registers: the slot's first group, its plane and place in it, the mask, the trip count.  The
// products with inc / index_inc are formed per trip on the scalar unit.  profiles/tail_walk_isa.txt: the aligned instance spills as
// many scalars as the unflagged kernel and reloads none of them on the path a trip takes.
template <bool ALIGNED>
__device__ __forceinline__ unsigned long long tail_mask_load(const int* __restrict__ flags, long long fstep, unsigned int o0, unsigned int lane,
                                                             unsigned int step, unsigned int p4, unsigned int total4, unsigned int klast)
{
    const TailAsk a = tail_mask_ask(o0, lane, step, p4, total4, klast);
    int f = 0;
    if (a.ask && !(ALIGNED && lane >= TAIL_MASK_TRIPS)) f = flags[(long long)a.k * fstep];
    return __ballot(f != 0);
}

template <bool CHECKED, bool ALIGNED>
__global__ __launch_bounds__(256) void k_extract4_noise2_sparse(const float* __restrict__ in, float* __restrict__ out,
                                                                long long plane4, long long nzo, int inc, int idx_inc,
                                                                const double* __restrict__ scal, float min_value, double mul,
                                                                uint32_t k0, uint32_t k1, uint32_t stream,
                                                                unsigned long long index_offset, PItem* __restrict__ queue,
                                                                unsigned int* __restrict__ qcount, unsigned int segcap,
                                                                const int* __restrict__ flags, int fstride)
{
    __shared__ unsigned long long qctr;
    __shared__ unsigned int qovf[2];
    __shared__ P1Scratch scratch[4];
    p1_frame_open(&qctr, qovf);
    const unsigned int lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const P1Args pa = p1_frame_args(mul, k0, k1, stream, queue, segcap, &qctr, qovf);
    const double corr = scal[1];
    const P1Empty pe = p1_empty_of(corr, min_value, pa);
    const float4* __restrict__ in4 = reinterpret_cast<const float4*>(in);
    float4* __restrict__ out4 = reinterpret_cast<float4*>(out);
    const unsigned int p4 = (unsigned int)plane4, total4 = (unsigned int)(plane4 * nzo), step = gridDim.x * 256u;   // (outputs < 2^32)
    const unsigned int klast = (unsigned int)nzo - 1u;
    const long long fstep = (long long)inc * fstride;                  // flag index per output plane
    unsigned int o0 = blockIdx.x * 256u + (unsigned int)wave * 64u;
    TailSlot sl = tail_slot_at(o0, p4);
    const unsigned int dq = step / p4, dr = step - dq * p4;
    unsigned long long mask = 0ull;
    for (unsigned int trip = 0u; o0 < total4; ++trip) {
        if (tail_mask_refill(trip)) mask = tail_mask_load<ALIGNED>(flags, fstep, o0, lane, step, p4, total4, klast);   // wave-uniform
        const bool fa = tail_mask_first(mask);
        // the slot's first group in the buffer and on the RNG counter (scalar; the lane adds itself)
        const unsigned long long sbase = (unsigned long long)(sl.k * (unsigned int)inc) * p4 + sl.rem;
        const unsigned long long ibase = (unsigned long long)(sl.k * (unsigned int)idx_inc) * p4 + sl.rem;
        float ov[4];
        if (ALIGNED) {
            const unsigned long long index4 = index_offset + 4ull * (ibase + lane), o4 = 4ull * (unsigned long long)(o0 + lane);
            if (!fa && pe.cls != 2) {                                        // wave-uniform
                poisson_phase1_empty<CHECKED>(pe, 15u, index4, o4, pa, ov);
            } else {
                float4 v = make_float4(pe.v, pe.v, pe.v, pe.v);
                if (fa) {                                                    // wave-uniform: the whole slot reads, or none of it
                    v = (in4 + sbase)[lane];
                    v.x = adjust_one(v.x, corr, min_value);
                    v.y = adjust_one(v.y, corr, min_value);
                    v.z = adjust_one(v.z, corr, min_value);
                    v.w = adjust_one(v.w, corr, min_value);
                }
                const float vv[4] = {v.x, v.y, v.z, v.w};
                poisson_phase1<CHECKED>(vv, true, index4, o4, pa, &scratch[wave], (int)lane, ov);
            }
            (out4 + o0)[lane] = make_float4(ov[0], ov[1], ov[2], ov[3]);
        } else {
            const unsigned int o = o0 + lane;
            const bool valid = o < total4;
            if (tail_slot_first(sl, p4) >= 64u && !fa && pe.cls != 2) {      // wave-uniform
                poisson_phase1_empty<CHECKED>(pe, valid ? 15u : 0u, index_offset + 4ull * (ibase + lane), 4ull * (unsigned long long)o, pa, ov);
            } else {
                // past the plane boundary the planes in between come on top (tail_lane's k * inc * p4 + within, without a 64-bit
                // multiplication per lane)
                const bool second = lane >= tail_slot_first(sl, p4);
                const bool empty = !(second ? tail_mask_second(mask) : fa);
                const unsigned long long sskip = (unsigned long long)(unsigned int)(inc - 1) * p4, iskip = (unsigned long long)(unsigned int)(idx_inc - 1) * p4;
                const unsigned long long src4 = sbase + lane + (second ? sskip : 0ull);
                const unsigned long long idx4 = ibase + lane + (second ? iskip : 0ull);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid) {
                    if (empty) {
                        v = make_float4(pe.v, pe.v, pe.v, pe.v);
                    } else {
                        v = in4[src4];
                        v.x = adjust_one(v.x, corr, min_value);
                        v.y = adjust_one(v.y, corr, min_value);
                        v.z = adjust_one(v.z, corr, min_value);
                        v.w = adjust_one(v.w, corr, min_value);
                    }
                }
                const float vv[4] = {v.x, v.y, v.z, v.w};
                poisson_phase1<CHECKED>(vv, valid, index_offset + 4ull * idx4, 4ull * (unsigned long long)o, pa, &scratch[wave], (int)lane, ov);
            }
            if (valid) out4[o] = make_float4(ov[0], ov[1], ov[2], ov[3]);
        }
        o0 += step; sl = tail_slot_next(sl, dq, dr, p4); mask = tail_mask_next(mask);
    }
    p1_frame_close<true>(qcount, &qctr, qovf, segcap);
}

template <bool CHECKED>
__global__ __launch_bounds__(256) void k_extract_noise2_any_sparse(const float* __restrict__ in, float* __restrict__ out,
                                                                   long long plane, long long nzo, int inc, int idx_inc,
                                                                   const double* __restrict__ scal, float min_value, double mul,
                                                                   uint32_t k0, uint32_t k1, uint32_t stream,
                                                                   unsigned long long index_offset, PItem* __restrict__ queue,
                                                                   unsigned int* __restrict__ qcount, unsigned int segcap,
                                                                   long long slots_per_plane, const int* __restrict__ flags, int fstride)
{
    __shared__ unsigned long long qctr;
    __shared__ unsigned int qovf[2];
    __shared__ P1Scratch scratch[4];
    p1_frame_open(&qctr, qovf);
    const P1Args pa = p1_frame_args(mul, k0, k1, stream, queue, segcap, &qctr, qovf);
    const double corr = scal[1];
    const FetchContiguous<true> fetch{in, inc, corr, min_value};
    group_walk_phase1_sparse<CHECKED>(fetch, p1_empty_of(corr, min_value, pa), flags, (long long)inc * fstride, out, plane, nzo, idx_inc,
                                      index_offset, slots_per_plane, pa, scratch);
    p1_frame_close<true>(qcount, &qctr, qovf, segcap);
}

// One block per queue segment (same grid as k_extract4_noise2; the grid-stride walk of that kernel spreads the
// bright voxels evenly over the segments).
__global__ __launch_bounds__(256) void k_poisson_resolve(ResolveJob job, const ExtractView* __restrict__ vt)
{
    view_job<true>(vt, job);
    __shared__ unsigned int ticket;
    __shared__ double tab[RESOLVE_TAB];
    resolve_segment_body(job, (long long)blockIdx.x, (int)threadIdx.x, &ticket, tab);
}

// Queues whose segments hold a SHARE of their blocks' voxels (poisson_queue_share < 16): the voxels a full segment refused, sampled
// where they stand.  A kernel of its own so that this divergent fp64 code costs neither phase 1 nor the resolver a register; its blocks
// return at once unless the resolver has recorded a refusal in the queue's header -- on the bench's volumes, always.
constexpr int REFUSED_BLOCKS = 2048;
constexpr unsigned int REFUSED_LIST = 4096;                // positions the block gathers before it samples them (16 KB of LDS)
__global__ __launch_bounds__(256) void k_poisson_refused(ResolveJob job, int segments, unsigned int full_items, unsigned int* hint,
                                                         const ExtractView* __restrict__ vt)
{
    view_job<false>(vt, job);                                         // (its queue is not read here)
    if (job.qcount[QCOUNT_HEADER + 2] == 0u) return;                 // no block of this view was refused anything (the resolver's word)
    __shared__ unsigned int list[REFUSED_LIST];
    __shared__ unsigned int count;
    const int t = (int)threadIdx.x;
    if (t == 0) count = 0u;
    __syncthreads();
    // refused voxels are a few per cent of a block's voxels, scattered: sampled where the walk finds them, one lane in twenty would work.
    // So the walk only gathers positions, and the list is sampled whenever another trip (1024 candidates) might not fit: all lanes busy.
    auto flush = [&]() {
        __syncthreads();                                              // the list is complete
        const unsigned int m = count;
        for (unsigned int i = (unsigned int)t; i < m; i += 256u) {
            const unsigned int o = list[i];
            job.out[o] = poisson_voxel((double)-job.out[o] * job.mul, job.k0, job.k1, job.stream, resolve_index_of(job, o));
        }
        __syncthreads();                                              // every lane has read `count` and its entries
        if (t == 0) count = 0u;
        __syncthreads();
    };
    unsigned int need = 0u;                                           // sixteenths of its voxels the fullest of this block's segments had pending
    for (int seg = (int)blockIdx.x; seg < segments; seg += (int)gridDim.x) {
        const unsigned int* qc = job.qcount + (size_t)QCOUNT_WORDS * seg;
        if (qc[2] == 0u) continue;                                    // block-uniform
        const unsigned int sixteenths = (unsigned int)((16ull * (qc[0] + qc[1] + qc[2]) + full_items - 1u) / full_items);
        need = sixteenths > need ? sixteenths : need;
        for (long long trip = 0;; ++trip) {
            if (!refused_collect(job, seg, trip, t, segments, list, &count)) break;      // block-uniform
            __syncthreads();
            const unsigned int gathered = count;                      // the same for every lane: read between two barriers
            __syncthreads();
            if (gathered + 1024u > REFUSED_LIST) flush();             // the next trip adds up to 1024 positions
        }
    }
    flush();
    // what a context on the automatic share builds its next queue with (api.cpp: queue_mode_next reads the word without synchronising)
    if (t == 0 && hint && need != 0u) __hip_atomic_fetch_max(hint, need > 16u ? 16u : need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The second launch of the sampler: one block per queue segment, and behind it -- where the segments can refuse (pl.checked) -- the walk
// over what they refused.  The fused tail of the convolution, whose pass E has run phase 1, ends here too.
int launch_resolve(hipStream_t s, const ExtractPlan& pl, const ExtractOps& o)
{
    const ExtractGeom& g = pl.geom;
    const unsigned gy = o.nviews > 0 ? (unsigned)o.nviews : 1u;
    const QueueLayout::Region q = pl.layout.region(o.queue_ws);
    const bool any = pl.kernel == EXTRACT_K_NOISE2_ANY;
    // how phase 1 walked the volume (ResolveJob): float4 groups, or wave slots of slots_per_plane per plane
    const long long walk_n = pl.kernel == EXTRACT_K_NOISE2 ? g.plane * g.nzo / 4 : (any ? pl.slots_per_plane * g.nzo : 0);
    const ResolveJob job{o.out, reinterpret_cast<const PItem*>(q.items), q.counts, pl.segcap, o.mul, (uint32_t)o.seed, (uint32_t)(o.seed >> 32), o.stream,
                         (unsigned int)g.plane, (unsigned int)g.index_inc, (unsigned long long)g.index_offset, pl.checked ? (any ? 2 : 1) : 0,
                         walk_n, any ? pl.slots_per_plane : 0};
    hipLaunchKernelGGL(k_poisson_resolve, dim3(pl.blocks, gy), dim3(256), 0, s, job, o.vt);
    if (job.walk != 0)
        hipLaunchKernelGGL(k_poisson_refused, dim3(pl.blocks < REFUSED_BLOCKS ? pl.blocks : REFUSED_BLOCKS, gy), dim3(256), 0, s, job, pl.blocks,
                           pl.full_items, pl.hint, o.vt);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_extract(hipStream_t s, const ExtractPlan& pl, const ExtractOps& o)
{
    const ExtractGeom& g = pl.geom;
    const dim3 grid(pl.blocks, o.nviews > 0 ? (unsigned)o.nviews : 1u), block(256);
    const float* in = o.in ? o.in + g.in_offset : nullptr;
    const uint32_t k0 = (uint32_t)o.seed, k1 = (uint32_t)(o.seed >> 32);
    const unsigned long long offset = g.index_offset;
    const bool queued = pl.kernel == EXTRACT_K_NOISE2 || pl.kernel == EXTRACT_K_NOISE2_ANY;
    if (o.empty_flags && !(queued && o.adjust && o.nviews == 0 && g.in_offset == 0 && g.plane >= TAIL_SPARSE_MIN_PLANE && o.empty_stride >= 1)) {
        // the buffer has holes only a flagged queue sampler knows about: no other form may read it
        set_error("extract: a sparse tail needs one of the two queue samplers on a single adjusted view");
        return MVSIM_EINVAL;
    }
    if (queued && o.empty_flags) {
        const QueueLayout::Region q = pl.layout.region(o.queue_ws);
        PItem* queue = reinterpret_cast<PItem*>(q.items);
        dispatch2(pl.checked, tail_walk_aligned((unsigned int)(g.plane / 4)), [&](auto C, auto A) {
            if (pl.kernel == EXTRACT_K_NOISE2)
                hipLaunchKernelGGL((k_extract4_noise2_sparse<decltype(C)::value, decltype(A)::value>), grid, block, 0, s, in, o.out, g.plane / 4, g.nzo, g.inc, g.index_inc,
                                   o.scal, o.min_value, o.mul, k0, k1, o.stream, offset, queue, q.counts, pl.segcap, o.empty_flags, o.empty_stride);
            else
                hipLaunchKernelGGL((k_extract_noise2_any_sparse<decltype(C)::value>), grid, block, 0, s, in, o.out, g.plane, g.nzo, g.inc, g.index_inc,
                                   o.scal, o.min_value, o.mul, k0, k1, o.stream, offset, queue, q.counts, pl.segcap, pl.slots_per_plane,
                                   o.empty_flags, o.empty_stride);
        });
        return launch_resolve(s, pl, o);
    }
    if (queued) {
        const QueueLayout::Region q = pl.layout.region(o.queue_ws);
        PItem* queue = reinterpret_cast<PItem*>(q.items);
        dispatch2(o.adjust, pl.checked, [&](auto A, auto C) {
            if (pl.kernel == EXTRACT_K_NOISE2)
                hipLaunchKernelGGL((k_extract4_noise2<decltype(A)::value, decltype(C)::value>), grid, block, 0, s, in, o.out, g.plane / 4, g.nzo, g.inc,
                                   g.index_inc, o.scal, o.min_value, o.mul, k0, k1, o.stream, offset, queue, q.counts, pl.segcap, o.vt);
            else       // planes that are no multiple of four voxels / unaligned buffers: the same two launches, group by group
                hipLaunchKernelGGL((k_extract_noise2_any<decltype(A)::value, decltype(C)::value>), grid, block, 0, s, in, o.out, g.plane, g.nzo, g.inc,
                                   g.index_inc, o.scal, o.min_value, o.mul, k0, k1, o.stream, offset, queue, q.counts, pl.segcap, pl.slots_per_plane, o.vt);
        });
        return launch_resolve(s, pl, o);
    }
    dispatch2(o.adjust, o.noise, [&](auto A, auto N) {
        if (pl.kernel == EXTRACT_K_VEC)
            hipLaunchKernelGGL((k_extract4<decltype(A)::value, decltype(N)::value>), grid, block, 0, s, in, o.out, g.plane / 4, g.nzo, g.inc, g.index_inc,
                               o.scal, o.min_value, o.mul, k0, k1, o.stream, offset, o.vt);
        else
            hipLaunchKernelGGL((k_extract<decltype(A)::value, decltype(N)::value>), grid, block, 0, s, in, o.out, g.plane, g.nzo, g.inc, g.index_inc,
                               o.scal, o.min_value, o.mul, k0, k1, o.stream, offset, o.vt);
    });
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

void extract_path(const int64_t dim[3], int inc, int index_inc, uint64_t index_offset, bool aligned16, int qshare, int64_t path[4])
{
    ExtractGeom g = ExtractGeom::strided(dim, inc);
    if (index_inc > 0) g.index_inc = index_inc;
    g.index_offset = index_offset;
    const ExtractPlan pl = extract_plan(g, aligned16, true, QueueMode{qshare, nullptr});
    path[0] = pl.kernel; path[1] = pl.checked ? 1 : 0; path[2] = pl.blocks; path[3] = pl.segcap;
}

// What the last two-launch sampler that used this workspace queued (mvsim_get_queue_stats): {items a segment holds, bright items,
// inversion items, voxels refused and sampled in place, pending voxels of the fullest block}.  The caller has synchronised the stream.
int poisson_queue_read_stats(const void* queue_ws, size_t bytes, long long stats[5])
{
    stats[0] = stats[1] = stats[2] = stats[3] = stats[4] = 0;
    if (!queue_ws || bytes < QueueLayout(0, 0, true).total_bytes) return MVSIM_OK;   // not a queue of the two-launch sampler
    std::vector<unsigned int> h((size_t)QCOUNT_HEADER + 2);
    MVSIM_HIP(hipMemcpy(h.data(), queue_ws, h.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    const unsigned int blocks = h[QCOUNT_HEADER] <= (unsigned int)POISSON_MAX_BLOCKS ? h[QCOUNT_HEADER] : 0u;
    stats[0] = h[(size_t)QCOUNT_HEADER + 1];
    stats[1] = stats[2] = stats[3] = stats[4] = 0;
    for (unsigned int b = 0; b < blocks; ++b) {
        const long long f = h[(size_t)QCOUNT_WORDS * b], k = h[(size_t)QCOUNT_WORDS * b + 1], r = h[(size_t)QCOUNT_WORDS * b + 2];
        stats[1] += f;
        stats[2] += k;
        stats[3] += r;
        if (f + k + r > stats[4]) stats[4] = f + k + r;     // what the fullest block had to settle: the segment size that refuses nothing
    }
    return MVSIM_OK;
}

}  // namespace mvsim
