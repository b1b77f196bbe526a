// The sequential java.util.Random walk of drawSpheres / multiSpheres resolved on the device (sphere_walk.h states the problem and
// holds every statement that decides a result; this file distributes them).
//
//   k_walk_events   one block per chunk of SW_CHUNK stream positions.  A lane jumps once to the state of its first position and
//                   steps over its 16 consecutive positions with the next five states in registers; per position "if a voxel
//                   started here" (walk_code).  The positions whose step is not 3 are compacted, in order, into the chunk's event
//                   list, and lanes 0 .. SW_ENTRIES - 1 resolve the orbit through the chunk for their entry offset (walk_resolve).
//   k_walk_scan     one block composes the chunk maps: every lane a contiguous run of chunks for all entry offsets, lane 0 the 256 run
//                   maps, then every lane its run again with the true entry -- per chunk the entry offset, the ordinal of its first
//                   voxel and the index of its first accepted voxel; the lane that meets voxel n - 1 writes the summary.
//   k_walk_emit     one lane per chunk follows the true orbit through the event list and writes the accepted voxels: ordinal, raw
//                   nextInt value and the second double, recomputed from the position by one jump.
//
// The host reads the summary between scan and emit (it sizes the entry list), so the call costs two synchronisations.
#include "common.h"
#include "sphere_walk.h"

namespace mvsim {

namespace {

struct WalkSummary {
    int32_t fail, reached;
    int64_t final_chunk, n_entries, end_pos;
};

constexpr int SW_THREADS = 256, SW_PER_LANE = SW_CHUNK / SW_THREADS;
static_assert(SW_PER_LANE * SW_THREADS == SW_CHUNK && SW_PER_LANE % 4 == 0, "a lane walks a multiple of four positions");
static_assert(SW_ENTRIES == 8 && SW_CHUNK <= SW_MAX_CHUNK && SW_MAX_EVENTS <= 4095, "the packed chunk map");

__device__ __forceinline__ uint64_t lcg_step(uint64_t s) { return (s * JR_A + JR_C) & JR_MASK; }

__global__ __launch_bounds__(SW_THREADS) void k_walk_events(uint64_t s0, WalkRule rule, uint32_t* __restrict__ events,
                                                            uint32_t* __restrict__ nevents, uint32_t* __restrict__ maps)
{
    __shared__ int scan[SW_THREADS];
    __shared__ uint32_t ev[SW_MAX_EVENTS];
    const int tid = threadIdx.x;
    const size_t chunk = blockIdx.x;
    const uint64_t base = jr_jump(s0, (uint64_t)chunk * SW_CHUNK);           // uniform over the block
    uint64_t w[6];
    w[0] = jr_jump(base, (uint64_t)(tid * SW_PER_LANE));
#pragma unroll
    for (int i = 1; i < 6; ++i) w[i] = lcg_step(w[i - 1]);
    uint32_t codes[SW_PER_LANE / 4];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < SW_PER_LANE; ++j) {
        const uint32_t c = walk_code(w, rule);
        if (j % 4 == 0) codes[j / 4] = c;
        else codes[j / 4] |= c << (8 * (j % 4));
        mine += c != 3u;
#pragma unroll
        for (int i = 0; i < 5; ++i) w[i] = w[i + 1];
        w[5] = lcg_step(w[5]);
    }
    // exclusive prefix of the event counts over the block (lane order is position order)
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < SW_THREADS; d <<= 1) {
        const int add = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const int total = scan[SW_THREADS - 1];
    int at = scan[tid] - mine;
    if (mine) {
#pragma unroll
        for (int j = 0; j < SW_PER_LANE; ++j) {
            const uint32_t c = (codes[j / 4] >> (8 * (j % 4))) & 0xffu;
            if (c != 3u) {
                if (at < SW_MAX_EVENTS) ev[at] = walk_event(tid * SW_PER_LANE + j, c);
                at += 1;
            }
        }
    }
    __syncthreads();
    const int nev = total < SW_MAX_EVENTS ? total : SW_MAX_EVENTS;
    if (tid < nev) events[chunk * SW_MAX_EVENTS + tid] = ev[tid];
    if (tid == 0) nevents[chunk] = (uint32_t)nev;
    if (tid < SW_ENTRIES) maps[chunk * SW_ENTRIES + tid] = walk_resolve(ev, nev, SW_CHUNK, tid, SW_ENTRIES, total > SW_MAX_EVENTS).pack();
}

// mp[i] without indexing registers dynamically
__device__ __forceinline__ uint32_t pick8(const uint32_t mp[8], int i)
{
    uint32_t r = mp[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) r = i == k ? mp[k] : r;
    return r;
}

__global__ __launch_bounds__(SW_THREADS) void k_walk_scan(const uint32_t* __restrict__ maps, const uint32_t* __restrict__ events,
                                                          const uint32_t* __restrict__ nevents, long long nchunks, long long n_total,
                                                          int32_t* __restrict__ entry, int64_t* __restrict__ vbase, int64_t* __restrict__ abase,
                                                          WalkSummary* __restrict__ summary)
{
    __shared__ int64_t run_count[SW_THREADS][SW_ENTRIES], run_acc[SW_THREADS][SW_ENTRIES];
    __shared__ uint8_t run_exit[SW_THREADS][SW_ENTRIES], run_fail[SW_THREADS][SW_ENTRIES];
    __shared__ int64_t start_v[SW_THREADS], start_a[SW_THREADS];
    __shared__ int start_e[SW_THREADS], start_fail[SW_THREADS];
    const int tid = threadIdx.x;
    const long long seg = (nchunks + SW_THREADS - 1) / SW_THREADS;
    const long long c0 = tid * seg < nchunks ? tid * seg : nchunks, c1 = c0 + seg < nchunks ? c0 + seg : nchunks;
    const uint4* maps4 = reinterpret_cast<const uint4*>(maps);
    {
        WalkMap cur[SW_ENTRIES];
#pragma unroll
        for (int e = 0; e < SW_ENTRIES; ++e) { cur[e].exit = e; cur[e].fail = 0; cur[e].count = 0; cur[e].accepted = 0; }
        for (long long c = c0; c < c1; ++c) {
            const uint4 lo = maps4[2 * c], hi = maps4[2 * c + 1];
            const uint32_t mp[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int e = 0; e < SW_ENTRIES; ++e) cur[e] = walk_compose(cur[e], WalkMap::unpack(pick8(mp, cur[e].exit)));
        }
#pragma unroll
        for (int e = 0; e < SW_ENTRIES; ++e) {
            run_count[tid][e] = cur[e].count; run_acc[tid][e] = cur[e].accepted;
            run_exit[tid][e] = (uint8_t)cur[e].exit; run_fail[tid][e] = (uint8_t)cur[e].fail;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int e = 0, fail = 0;
        int64_t v = 0, a = 0;
        for (int t = 0; t < SW_THREADS; ++t) {
            start_e[t] = e; start_fail[t] = fail; start_v[t] = v; start_a[t] = a;
            v += run_count[t][e]; a += run_acc[t][e]; fail |= run_fail[t][e];
            e = run_exit[t][e];
        }
    }
    __syncthreads();
    int e = start_e[tid], fail = start_fail[tid];
    int64_t v = start_v[tid], a = start_a[tid];
    for (long long c = c0; c < c1; ++c) {
        entry[c] = e; vbase[c] = v; abase[c] = a;
        const WalkMap m = WalkMap::unpack(maps[c * SW_ENTRIES + e]);
        fail |= m.fail;
        if (v < n_total && v + m.count >= n_total) {               // voxel n_total - 1 starts in this chunk: exactly one lane gets here
            int64_t end = -1, found = 0;
            (void)walk_chunk(events + (size_t)c * SW_MAX_EVENTS, (int)nevents[c], SW_CHUNK, e, v, n_total, &end,
                             [&](int64_t, int) { found += 1; });
            summary->fail = fail | (end < 0 ? 1 : 0);
            summary->final_chunk = c;
            summary->n_entries = a + found;
            summary->end_pos = c * SW_CHUNK + end;
            summary->reached = 1;
        }
        v += m.count; a += m.accepted; e = m.exit;
    }
}

__global__ __launch_bounds__(SW_THREADS) void k_walk_emit(uint64_t s0, WalkRule rule, const uint32_t* __restrict__ events,
                                                          const uint32_t* __restrict__ nevents, const int32_t* __restrict__ entry,
                                                          const int64_t* __restrict__ vbase, const int64_t* __restrict__ abase,
                                                          long long nchunks_used, long long n_total, long long capacity,
                                                          WalkEntry* __restrict__ out)
{
    const long long c = (long long)blockIdx.x * SW_THREADS + threadIdx.x;
    if (c >= nchunks_used) return;
    int64_t at = abase[c], end;
    (void)walk_chunk(events + (size_t)c * SW_MAX_EVENTS, (int)nevents[c], SW_CHUNK, entry[c], vbase[c], n_total, &end, [&](int64_t ordinal, int q) {
        const WalkVoxel vx = walk_voxel(jr_jump(s0, (uint64_t)(c * SW_CHUNK + q)), rule);
        if (at < capacity) {
            WalkEntry w;
            w.ordinal = ordinal; w.raw = vx.raw; w.pad = 0; w.value = vx.value;
            out[at] = w;
        }
        at += 1;
    });
}

}  // namespace

// The accepted voxels of a walk over n voxels from `state`, in visit order, and the state the walk ends in.  *done = false: the device
// walk does not vouch for this case (sphere_walk.h: fail, or voxel n - 1 not reached, or too many chunks for one launch) -- nothing has
// been written, the caller walks on the host.
int sphere_walk_dev(mvsim_ctx* ctx, uint64_t state, int64_t n, const WalkRule& rule, std::vector<WalkEntry>* entries, uint64_t* end_state,
                    bool* done)
{
    *done = false;
    entries->clear();
    if (n <= 0) { *end_state = state; *done = true; return MVSIM_OK; }
    if (n > ((int64_t)1 << 40)) return MVSIM_OK;
    const int64_t nchunks = (walk_cover(n) + SW_CHUNK - 1) / SW_CHUNK;
    if (nchunks >= ((int64_t)1 << 31) - 1) return MVSIM_OK;
    DevBuf* b = ctx->walk_buf;
    MVSIM_TRY(b[0].reserve((size_t)nchunks * SW_MAX_EVENTS * sizeof(uint32_t)));
    MVSIM_TRY(b[1].reserve((size_t)nchunks * (SW_ENTRIES + 1) * sizeof(uint32_t)));                        // maps, then the event counts
    MVSIM_TRY(b[2].reserve(256 + (size_t)nchunks * (2 * sizeof(int64_t) + sizeof(int32_t))));              // summary, vbase, abase, entry
    uint32_t *events = b[0].as<uint32_t>(), *maps = b[1].as<uint32_t>(), *nevents = maps + (size_t)nchunks * SW_ENTRIES;
    WalkSummary* summary = b[2].as<WalkSummary>();
    int64_t* vbase = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(b[2].p) + 256);
    int64_t* abase = vbase + nchunks;
    int32_t* entry = reinterpret_cast<int32_t*>(abase + nchunks);
    MVSIM_HIP(hipMemsetAsync(summary, 0, sizeof(WalkSummary), ctx->stream));
    hipLaunchKernelGGL(k_walk_events, dim3((unsigned)nchunks), dim3(SW_THREADS), 0, ctx->stream, state, rule, events, nevents, maps);
    hipLaunchKernelGGL(k_walk_scan, dim3(1), dim3(SW_THREADS), 0, ctx->stream, maps, events, nevents, (long long)nchunks, (long long)n, entry,
                       vbase, abase, summary);
    MVSIM_HIP(hipGetLastError());
    WalkSummary sum;
    MVSIM_HIP(hipMemcpyAsync(&sum, summary, sizeof sum, hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    if (sum.fail || !sum.reached || sum.final_chunk < 0 || sum.final_chunk >= nchunks || sum.n_entries < 0 || sum.n_entries > n) return MVSIM_OK;
    if (sum.n_entries > 0) {
        MVSIM_TRY(b[3].reserve((size_t)sum.n_entries * sizeof(WalkEntry)));
        const long long used = sum.final_chunk + 1;
        hipLaunchKernelGGL(k_walk_emit, dim3((unsigned)((used + SW_THREADS - 1) / SW_THREADS)), dim3(SW_THREADS), 0, ctx->stream, state, rule, events,
                           nevents, entry, vbase, abase, used, (long long)n, (long long)sum.n_entries, b[3].as<WalkEntry>());
        MVSIM_HIP(hipGetLastError());
        entries->resize((size_t)sum.n_entries);
        MVSIM_HIP(hipMemcpyAsync(entries->data(), b[3].p, (size_t)sum.n_entries * sizeof(WalkEntry), hipMemcpyDeviceToHost, ctx->stream));
        MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    }
    *end_state = jr_jump(state, (uint64_t)sum.end_pos);
    *done = true;
    return MVSIM_OK;
}

}  // namespace mvsim
