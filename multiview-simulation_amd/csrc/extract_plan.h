// The host-side plan of the extract + Poisson stage: which planes one launch reads and on which RNG counters (ExtractGeom), where a queue
// workspace keeps its counts and its segments (QueueLayout), and the sampler form, grid and queue geometry that follow (ExtractPlan).
// extract_plan() derives them and nothing else does: the launcher (extract.hip), the stage function (api.cpp: extract_stage),
// mvsim_extract_path and the fused tail read them.  Plain C++, no HIP include (tests/c_abi/extract_plan_main.cpp: g++ alone).
#pragma once

#include <cstddef>
#include <cstdint>

namespace mvsim {

// The count array in front of a queue's segments: per block three words -- items at the front, items at the back, voxels that found
// the segment full -- for up to POISSON_MAX_BLOCKS blocks, then a header the first block of phase 1 writes: {blocks, items per segment}
// (what mvsim_get_queue_stats reads) and the resolver completes: {.., .., 1 if any block refused a voxel} (what k_poisson_refused reads).
constexpr int QCOUNT_WORDS = 3;
constexpr int POISSON_MAX_BLOCKS = 256 * 64;
constexpr int QCOUNT_HEADER = QCOUNT_WORDS * POISSON_MAX_BLOCKS;        // word index of the header
constexpr size_t PITEM_BYTES = 16;                                      // one work item (poisson_dev.h: PItem)

// The sampler form: path = {EXTRACT_K_*, segments can refuse, blocks, items per segment} (mvsim_extract_path, mvsim_get_extract_path)
enum { EXTRACT_K_SCALAR = 0, EXTRACT_K_VEC = 1, EXTRACT_K_NOISE2 = 2, EXTRACT_K_NOISE2_ANY = 3, EXTRACT_FUSED_TAIL = 4,
       EXTRACT_K_INTERVAL = 5 };   // 5: an interval launch (interval_plan.h), reported by mvsim_get_extract_path only

// How the stage samples.  share 0: one launch, no work queue.  1..16: work queue whose per-block segments hold that many sixteenths
// of the block's voxels.  QUEUE_SHARE_AUTO + L (L = 0..16): the library's choice -- every voxel for queues of up to 64 MiB, else
// max(QUEUE_SHARE_START, L) sixteenths, L being what this context's views have needed so far (api.cpp: queue_mode_next).
constexpr int QUEUE_SHARE_AUTO = 32;
constexpr int QUEUE_SHARE_START = 5;
struct QueueMode {
    int           share = 0;
    unsigned int* hint  = nullptr;  // page-locked word k_poisson_refused raises to the sixteenths the fullest refused block would have needed
};

// What one launch acquires: output plane k (0 <= k < nzo) is the buffer's plane in_offset / plane + k * inc, and its voxel i draws on
// RNG counter index_offset + k * index_inc * plane + i -- the plane's place in the SOURCE volume, wherever the buffer keeps it.
struct ExtractGeom {
    long long plane;              // voxels per plane
    long long nzo;                // acquired planes (0: an empty slab)
    int       inc;                // plane stride of the reads
    int       index_inc;          // plane stride of the RNG counter
    uint64_t  index_offset;       // counter of the first voxel read
    long long in_offset;          // the first voxel read, relative to the buffer

    // every inc-th plane of a whole volume of dim[2] planes
    static ExtractGeom strided(const int64_t dim[3], int inc) { return {(long long)dim[0] * dim[1], (long long)((dim[2] - 1) / inc + 1), inc, inc, 0, 0}; }
    // the buffer holds the planes k * inc of that volume alone, in order: read every plane, count the RNG in source planes
    static ExtractGeom compact(const int64_t dim[3], int inc) { ExtractGeom g = strided(dim, inc); g.inc = 1; return g; }
    // the acquired planes k, z0 <= k * inc < z1, of a buffer that holds the planes [z0, z1) of the volume -- or, compact (z0 is a
    // multiple of inc), the planes z0 + k * inc alone
    static ExtractGeom slab(const int64_t dim[3], int inc, int64_t z0, int64_t z1, bool compact)
    {
        const long long plane = (long long)dim[0] * dim[1];
        const int64_t k0 = (z0 + inc - 1) / inc, k1 = (z1 + inc - 1) / inc;
        const int64_t first = k0 * inc;                           // global index of the first acquired source plane
        return {plane, (long long)(k1 > k0 ? k1 - k0 : 0), compact ? 1 : inc, inc, (uint64_t)(first * plane), compact ? 0 : plane * (first - z0)};
    }
};

// Where a queue workspace keeps its counts and where its segments start: [counts][segments], the only place that knows.  fixed_header:
// the count array is QCOUNT_HEADER words and the header behind it, whatever `blocks` is (the stage's own queues: at most
// POISSON_MAX_BLOCKS blocks).  Else three words per block, rounded up to 256 bytes, and NO header: the fused tail of the convolution,
// whose pass E may have more blocks than that -- mvsim_get_queue_stats finds no block count behind such a view.
struct QueueLayout {
    size_t counts_bytes = 0;      // the segments start here (16-byte aligned)
    size_t total_bytes  = 0;
    constexpr QueueLayout() = default;
    constexpr QueueLayout(long long blocks, unsigned int segcap, bool fixed_header)
        : counts_bytes(fixed_header ? (size_t)QCOUNT_HEADER * sizeof(unsigned int) + 256
                                    : (((size_t)QCOUNT_WORDS * (size_t)blocks * sizeof(unsigned int) + 255) & ~(size_t)255)),
          total_bytes(counts_bytes + (size_t)blocks * segcap * PITEM_BYTES) {}
    size_t view_stride() const { return (total_bytes + 255) & ~(size_t)255; }   // stacked views: one region per view
    struct Region { unsigned int* counts; void* items; };
    // the counts and the segments of the workspace at `ws` (null: no queue) -- of its region `view`
    Region region(void* ws, int view = 0) const
    {
        char* p = ws ? static_cast<char*>(ws) + (size_t)view * view_stride() : nullptr;
        return {reinterpret_cast<unsigned int*>(p), p ? p + counts_bytes : nullptr};
    }
};
static_assert(QueueLayout(1, 0, true).counts_bytes % 256 == 0, "the segments start 16-byte aligned");

struct ExtractPlan {
    ExtractGeom  geom;
    int          kernel;          // EXTRACT_K_*
    bool         checked;         // segments that can fill up (share < 16): the appends look before they write, a third kernel samples the refused
    int          blocks;          // grid of the kernel (and of the resolver: one block per segment)
    unsigned int segcap;          // items per segment (0: no queue)
    unsigned int full_items;      // ... of a segment that holds every voxel of its block (what k_poisson_refused measures a block's need by)
    long long    slots_per_plane; // EXTRACT_K_NOISE2_ANY: wave slots per plane
    int          share;           // sixteenths the queue is built with (0: no queue asked for)
    QueueLayout  layout;          // the workspace a sampled launch reserves
    unsigned int* hint;           // QueueMode::hint of the context that planned it
};

// the share a queue of n_out voxels is built with.  Auto: what the context has learned its views need, from QUEUE_SHARE_START sixteenths up
// (at 512^3 and the bench's SNR the sphere phantom's fullest block has 14 % of its voxels pending, that of a volume without an empty voxel
// 68 %: profiles/r05_queue_share.txt), but small queues (<= 64 MiB at full size: up to 160^3 acquired
// voxels) are not worth the extra launch that looks for refused voxels
inline int share_for(long long n_out, int share)
{
    if (share >= QUEUE_SHARE_AUTO) {
        const int learned = share - QUEUE_SHARE_AUTO;
        return n_out <= (4ll << 20) ? 16 : (learned >= 16 ? 16 : (learned > QUEUE_SHARE_START ? learned : QUEUE_SHARE_START));
    }
    return share >= 16 ? 16 : (share < 1 ? 1 : share);
}

inline unsigned int segment_share(long long worst, int share)
{
    if (share >= 16) return (unsigned int)worst;
    long long c = (worst * (share < 1 ? 1 : share) + 15) / 16;
    c = (c + 63) & ~63ll;                                   // at least one wave of items, whole waves after that
    return (unsigned int)(c < worst ? c : worst);
}

struct QueueGeom { int blocks; long long worst, slots_per_plane; };   // worst: voxels a block walks, the segment that refuses nothing
inline int queue_blocks(long long want) { return (int)(want < 1 ? 1 : (want > POISSON_MAX_BLOCKS ? POISSON_MAX_BLOCKS : want)); }
// Work-queue geometry of the vector form for n_out output voxels: `blocks` blocks of 256 lanes x 4 voxels walk the volume with a grid
// stride; each owns a segment of `share` sixteenths of its voxels (16: every voxel, 16 B per output voxel of HBM workspace and no
// refusals; less: what does not fit is sampled in place, poisson_dev.h).  Worst case every voxel of the block: the squeeze accepts
// only ~35 % at lambda = 10.
inline QueueGeom queue_geom_vec(long long n_out)
{
    const int b = queue_blocks((n_out / 4 + 255) / 256);
    const long long iters = (n_out / 4 + (long long)b * 256 - 1) / ((long long)b * 256);
    return {b, iters * 1024, 0};
}
// The same group by group (k_extract_noise2_any): a wave slot is 64 Philox groups of ONE plane (a plane of `plane` voxels that starts
// anywhere inside a group touches up to plane / 4 + 1 of them, rounded up to whole slots), `blocks` blocks of four waves walk the slots
// with a grid stride, and a block's segment holds `share` sixteenths of the voxels of its trips.
inline QueueGeom queue_geom_any(long long plane, long long nzo)
{
    const long long spp = ((plane + 3) / 4 + 1 + 63) / 64, slots = spp * nzo;
    const int b = queue_blocks((slots + 3) / 4);
    const long long trips = (slots + (long long)b * 4 - 1) / ((long long)b * 4);
    return {b, trips * 1024, spp};
}

// aligned16: both buffers (plus in_offset) allow 16-byte accesses; noise: the launch samples; mode: the context's queue setting.
inline ExtractPlan extract_plan(const ExtractGeom& g, bool aligned16, bool noise, QueueMode mode)
{
    ExtractPlan p{};
    p.geom = g; p.hint = mode.hint;
    const long long plane = g.plane, total = g.plane * g.nzo;
    p.share = noise && mode.share != 0 ? share_for(total, mode.share) : 0;
    // phase 1 hands a slot's RNG counters across lanes as 32-bit offsets from lane 0's (poisson_phase1): a vector slot is 256
    // consecutive outputs, and planes smaller than that put several plane boundaries -- each a jump of (index_inc - 1) planes of
    // counter -- into one slot; all of them together must stay below 2^31 (double: the product may exceed 64 bits)
    const double crossings = (double)((255 + plane - 1) / plane);
    // ... and a work item carries its output position (and the resolver the plane) in 32 bits
    const bool use_queue = p.share != 0 && crossings * (double)(g.index_inc - 1) * (double)plane < 2147483648.0 && total < (1ll << 32) &&
                           plane < (1ll << 32);
    const bool vec = (plane % 4 == 0) && (g.index_offset % 4 == 0) && aligned16;
    const QueueGeom qv = queue_geom_vec(total), qa = queue_geom_any(plane, g.nzo);
    p.checked = use_queue && p.share < 16;
    if (use_queue) {
        const QueueGeom& q = vec ? qv : qa;
        p.kernel = vec ? EXTRACT_K_NOISE2 : EXTRACT_K_NOISE2_ANY;
        p.blocks = q.blocks; p.slots_per_plane = q.slots_per_plane;
        p.segcap = segment_share(q.worst, p.share); p.full_items = (unsigned int)q.worst;
    } else {
        const long long want = vec ? (total / 4 + 255) / 256 : (total + 255) / 256, cap = vec ? 256 * 64 : 256 * 32;
        p.kernel = vec ? EXTRACT_K_VEC : EXTRACT_K_SCALAR;
        p.blocks = (int)(want < 1 ? 1 : (want > cap ? cap : want));
    }
    if (noise) {
        // the larger of the two queue forms, whichever kernel takes this launch -- and the smallest queue where none does: a grow-only
        // workspace must not depend on one call's pointer alignment
        const int s = share_for(total, mode.share);
        const QueueLayout lv(qv.blocks, segment_share(qv.worst, s), true), la(qa.blocks, segment_share(qa.worst, s), true);
        p.layout = la.total_bytes > lv.total_bytes ? la : lv;
    }
    return p;
}

// ---- The sparse tail (option skip_tail).  Behind a flagged view (the fused rotate kernel's plane flags, dilated by the reach of the
// PSF's z taps) a plane of the convolved volume whose flag is clear is exactly zero: pass E does not store it and phase 1 of the queue
// samplers does not read it -- every voxel of it has the one value adjust_one(+0, corr, min_value).  The buffer between the two then
// has holes, so the mode is taken only where the one reader of the buffer is known, BEFORE pass E is enqueued, to be a flagged sampler.
// The caller's half (view_enqueue): the option, the convolved volume not requested -- the buffer is the context's own workspace --, and
// the launch behind the convolution one of the two queue samplers ...
inline bool tail_sparse_caller(bool skip_tail, bool con_requested, bool queue_sampler) { return skip_tail && !con_requested && queue_sampler; }
// ... the driver's half: the view carries dilated flags (x_done, a whole single view, skip_empty, not the inline z pass) and pass E
// does not run the fused tail
inline bool tail_sparse_ok(bool caller_half, bool has_flags, bool fused_tail) { return caller_half && has_flags && !fused_tail; }

// phase 1 tells a slot's planes apart by ONE plane boundary (the vector form: 64 float4 groups per slot), so a plane holds at least a slot
constexpr long long TAIL_SPARSE_MIN_PLANE = 256;
// "one of the two queue samplers" for an acquisition of every inc-th plane of `dim`, whichever of the two geometries the convolution
// leaves (compact planes or all of them) and whatever the buffers' alignment: known from the sizes and the context's queue setting alone
inline bool tail_queue_sampler(const int64_t dim[3], int inc, bool noise, QueueMode mode)
{
    if (!noise || (long long)dim[0] * dim[1] < TAIL_SPARSE_MIN_PLANE) return false;
    for (int compact = 0; compact < 2; ++compact)
        for (int aligned = 0; aligned < 2; ++aligned) {
            const int k = extract_plan(compact ? ExtractGeom::compact(dim, inc) : ExtractGeom::strided(dim, inc), aligned != 0, true, mode).kernel;
            if (k != EXTRACT_K_NOISE2 && k != EXTRACT_K_NOISE2_ANY) return false;
        }
    return true;
}

// Which flag stands for which plane.  Pass E produces the planes j = 0 .. nk-1 of the buffer; plane j is source plane j * zstride, the
// index of its dilated flag (zstride: ConvTail::sparse_stride).  Output plane k of the sampler reads buffer plane k * g.inc (whole
// views: in_offset = 0), hence flag k * g.inc * zstride: source plane k * inc for both ExtractGeom::strided (g.inc = inc, zstride = 1)
// and ::compact (g.inc = 1, zstride = inc).
inline long long tail_flag_of_buffer_plane(long long j, int zstride) { return j * zstride; }
inline long long tail_flag_of_output(const ExtractGeom& g, long long k, int zstride) { return tail_flag_of_buffer_plane(k * g.inc, zstride); }

// The vector form's walk behind a sparse tail (k_extract4_noise2_sparse; constexpr: host and device).  A wave slot is 64 consecutive
// float4 groups of the output from group o0 on; p4 groups make a plane (p4 >= 64, outputs < 2^32).  The slot starts in plane k at
// group rem of it and the grid stride is dq planes and dr groups, so the next slot follows without a division.
struct TailSlot { unsigned int k, rem; };
constexpr TailSlot tail_slot_at(unsigned int o0, unsigned int p4) { return TailSlot{o0 / p4, o0 - (o0 / p4) * p4}; }
constexpr TailSlot tail_slot_next(TailSlot s, unsigned int dq, unsigned int dr, unsigned int p4)
{
    return s.rem + dr >= p4 ? TailSlot{s.k + dq + 1u, s.rem + dr - p4} : TailSlot{s.k + dq, s.rem + dr};
}
// groups of plane k from lane 0 on (>= 64: the slot lies in one plane); from that lane on the groups are of plane k + 1 -- never of a third
constexpr unsigned int tail_slot_first(TailSlot s, unsigned int p4) { return p4 - s.rem; }
struct TailLane { unsigned int k, within; bool second; };   // a lane's group: its plane, its place in it, whether it is past the boundary
constexpr TailLane tail_lane(TailSlot s, unsigned int lane, unsigned int p4)
{
    return lane >= tail_slot_first(s, p4) ? TailLane{s.k + 1u, lane - tail_slot_first(s, p4), true} : TailLane{s.k, s.rem + lane, false};
}
// p4 a multiple of 64 (every power-of-two plane, the flagship's): a wave's slots start on multiples of 64 groups, so none straddles a
// plane and none is cut by the end of the output -- the kernel instance without a second plane, per-lane flags or a `valid` lane mask
constexpr bool tail_walk_aligned(unsigned int p4) { return p4 % 64u == 0u; }

// The flags of a wave's trips as a bit mask, asked for once per TAIL_MASK_TRIPS trips and not once per trip.  Trip t of the wave is the
// slot at group o0 + t * step.  From the slot at o0 on, lane l of the wave asks for ONE flag: lanes 0..31 that of the plane the slot of
// trip l starts in, lanes 32..63 that of the plane behind it for trip l - 32 -- the second plane of a straddling slot, clamped to the last
// plane as a slot at the end of the output has none -- and lanes whose trip lies past the end ask for nothing: their bit is clear.  The
// wave's ballot over "flag set" is the mask: bit t the first plane of trip t, bit 32 + t its second.  One load instruction per wave
// and refill, no flag register carried from trip to trip; the one division per lane is per refill too.
constexpr unsigned int TAIL_MASK_TRIPS = 32;
struct TailAsk { bool ask; unsigned int k; };               // whether the lane loads a flag, and of which output plane
constexpr TailAsk tail_mask_ask(unsigned int o0, unsigned int lane, unsigned int step, unsigned int p4, unsigned int total4, unsigned int klast)
{
    // (outputs < 2^32: total4 < 2^30, and step <= POISSON_MAX_BLOCKS * 256 = 2^22 -- no sum here reaches 2^32)
    const unsigned int o = o0 + (lane % TAIL_MASK_TRIPS) * step, k = o / p4;
    return o < total4 ? TailAsk{true, (lane >= TAIL_MASK_TRIPS && k < klast) ? k + 1u : k} : TailAsk{false, 0u};
}
constexpr bool tail_mask_refill(unsigned int trip) { return trip % TAIL_MASK_TRIPS == 0u; }       // the mask is used up (or was never loaded)
constexpr bool tail_mask_first(unsigned long long m) { return (m & 1ull) != 0ull; }               // this trip's first plane is non-empty
constexpr bool tail_mask_second(unsigned long long m) { return ((m >> TAIL_MASK_TRIPS) & 1ull) != 0ull; }
constexpr unsigned long long tail_mask_next(unsigned long long m) { return (m >> 1) & ~(1ull << (TAIL_MASK_TRIPS - 1u)); }   // both halves move on one trip
// trips of the wave whose first slot starts at o0 (what the walk `for (; o0 < total4; o0 += step)` makes)
constexpr unsigned int tail_trips(unsigned int o0, unsigned int total4, unsigned int step) { return o0 < total4 ? (total4 - o0 - 1u) / step + 1u : 0u; }

}  // namespace mvsim
