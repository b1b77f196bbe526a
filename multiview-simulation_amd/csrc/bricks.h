// The brick binner of the three renderers whose result depends on the order of their items and that therefore never scatter with
// atomics: the bead images (beads.hip), the sphere raster (procedural.hip) and VolumeInjection (aberrations.hip).  DESIGN.md, "The
// brick binner", has the argument; the steps are
//
//   cull    the consumer's kernel: the clipped inclusive box of every item and bricks_overlapped() of it into counts
//   scan    BrickBins::scan: exclusive sum of the counts, every item's first slot
//   emit    the consumer's kernel calls brick_emit(): (key base + brick, value) pairs at the item's slots, in item order
//   finish  BrickBins::finish: k_brick_pad gives the slots behind the last pair a key beyond every brick, a stable LSD radix sort
//           by key (hipcub) leaves every brick's list in item order, k_brick_starts finds each key's first pair by binary search
//   render  the consumer's kernel, one block of 256 lanes per brick: brick_lane() is the lane's place in the brick, the list goes
//           through LDS in chunks of CH (brick_fill_tables() for the two Gaussian renderers)
//
// Keys are job * bricks + brick: one call bins `jobs` lists over the same grid at once (the bead renderer's views; one job elsewhere).
#pragma once

#include "common.h"

#include <hipcub/hipcub.hpp>

namespace mvsim {

namespace {

constexpr int BX = 32, BY = 8, BZ = 16;     // brick: two 32-voxel rows per wave, four waves, 16 planes per lane
constexpr int CH = 32;                      // items per LDS chunk
constexpr int NTAB = BX + BY + BZ;          // entries of one item's per-axis factor tables

struct BrickGrid {
    int      nbx, nby, nbz;
    uint32_t nb;
};

// the grid over an image of dim voxels; refuses an image whose brick indices would not leave keys a spare bit
inline int brick_grid(const int64_t dim[3], const char* who, BrickGrid* g)
{
    g->nbx = (int)((dim[0] + BX - 1) / BX);
    g->nby = (int)((dim[1] + BY - 1) / BY);
    g->nbz = (int)((dim[2] + BZ - 1) / BZ);
    const uint64_t nb = (uint64_t)g->nbx * g->nby * g->nbz;
    if (nb >= ((uint64_t)1 << 31)) {
        set_error("invalid argument: %s: image of %llu bricks", who, (unsigned long long)nb);
        return MVSIM_EINVAL;
    }
    g->nb = (uint32_t)nb;
    return MVSIM_OK;
}

// the bricks a clipped inclusive box lo..hi overlaps (lo > hi along any axis: none)
__host__ __device__ inline uint32_t bricks_overlapped(const int lo[3], const int hi[3])
{
    const int bs[3] = {BX, BY, BZ};
    uint32_t cnt = 1;
    for (int d = 0; d < 3; ++d) cnt = lo[d] > hi[d] ? 0u : cnt * (uint32_t)(hi[d] / bs[d] - lo[d] / bs[d] + 1);
    return cnt;
}

// the most bricks a box of `size` voxels per axis, placed anywhere and clipped to the image, can overlap: what one item may emit
inline int64_t bricks_spanned(const int size[3], const int64_t dim[3], const BrickGrid& g)
{
    const int bs[3] = {BX, BY, BZ};
    const int64_t nbd[3] = {g.nbx, g.nby, g.nbz};
    int64_t per_item = 1;
    for (int d = 0; d < 3; ++d) {
        const int64_t len = std::min<int64_t>(size[d], dim[d]), k = (len + bs[d] - 2) / bs[d] + 1;
        per_item *= k < nbd[d] ? k : nbd[d];
    }
    return per_item;
}

// Java Math.round(double) for the finite values that reach it here: floor, plus one when the fraction is >= 0.5 (x - floor(x)
// is exact), so -2.5 -> -2 and 0.49999999999999994 -> 0 as on Java 7 and later.
__device__ __forceinline__ long long java_round_d(double x)
{
    const double f = floor(x);
    return (long long)f + ((x - f) >= 0.5 ? 1 : 0);
}

// an item's (key, value) pairs from its scanned slot `o` on, bricks in z, y, x order
__device__ __forceinline__ void brick_emit(const int lo[3], const int hi[3], const BrickGrid& g, uint32_t key_base, uint32_t val, uint32_t o,
                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    for (int bz = lo[2] / BZ; bz <= hi[2] / BZ; ++bz)
        for (int by = lo[1] / BY; by <= hi[1] / BY; ++by)
            for (int bx = lo[0] / BX; bx <= hi[0] / BX; ++bx) {
                keys[o] = key_base + (uint32_t)(bx + g.nbx * (by + g.nby * bz));
                vals[o] = val;
                ++o;
            }
}

// slots past the last pair: a key beyond every brick, so that they sort to the end
__global__ __launch_bounds__(256) void k_brick_pad(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offs, long long items,
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, long long slots, uint32_t pad_key)
{
    const long long total = items > 0 ? (long long)offs[items - 1] + counts[items - 1] : 0;
    for (long long i = total + (long long)blockIdx.x * 256 + threadIdx.x; i < slots; i += (long long)gridDim.x * 256) {
        keys[i] = pad_key;
        vals[i] = 0u;
    }
}

// starts[k] = first sorted pair of key k (k = 0 .. nkeys; starts[nkeys] = number of pairs)
__global__ __launch_bounds__(256) void k_brick_starts(const uint32_t* __restrict__ keys, long long slots, uint32_t* __restrict__ starts,
                                                      uint32_t nkeys)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k > (long long)nkeys) return;
    long long lo = 0, hi = slots;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    starts[k] = (uint32_t)lo;
}

// The binning workspace of one call, carved from the consumer's own buffers, and the launches around the consumer's cull and emit:
//   reserve();  per chunk:  [cull -> counts;  scan(items);  emit -> keys[0], vals[0]  -- skipped for an empty chunk]  finish()
// after which vals[1] holds the values sorted by key and starts[k] .. starts[k + 1] is the list of key k.
struct BrickBins {
    uint32_t *counts = nullptr, *offs = nullptr, *starts = nullptr, *keys[2] = {}, *vals[2] = {};
    DevBuf*   tmp = nullptr;                 // scan / sort temp storage
    long long max_items = 0, max_slots = 0;

    // index: counts | offs | starts; refusal: the consumer's message for more items or slots than hipcub's int counts hold
    int reserve(hipStream_t s, long long items, long long slots, long long nkeys, DevBuf& index, DevBuf& kbuf, DevBuf& vbuf, DevBuf& tbuf,
                const char* refusal)
    {
        if (slots >= ((long long)1 << 31) || items >= ((long long)1 << 31)) {
            set_error(refusal, slots);
            return MVSIM_EINVAL;
        }
        size_t scan_tmp = 0, sort_tmp = 0;
        MVSIM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)items, s));
        MVSIM_TRY(sort(s, nullptr, sort_tmp, (int)slots, 32));
        MVSIM_TRY(index.reserve((size_t)(2 * items + nkeys + 1) * sizeof(uint32_t)));
        MVSIM_TRY(kbuf.reserve((size_t)(2 * slots) * sizeof(uint32_t)));
        MVSIM_TRY(vbuf.reserve((size_t)(2 * slots) * sizeof(uint32_t)));
        MVSIM_TRY(tbuf.reserve(std::max<size_t>(16, std::max(scan_tmp, sort_tmp))));
        max_items = items;
        max_slots = slots;
        counts = index.as<uint32_t>();
        offs = counts + items;
        starts = offs + items;
        keys[0] = kbuf.as<uint32_t>(); keys[1] = keys[0] + slots;
        vals[0] = vbuf.as<uint32_t>(); vals[1] = vals[0] + slots;
        tmp = &tbuf;
        return MVSIM_OK;
    }

    int scan(hipStream_t s, long long items)
    {
        size_t t = tmp->bytes;
        MVSIM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp->p, t, counts, offs, (int)items, s));
        return MVSIM_OK;
    }

    // slots = the chunk's bound on its pairs + 1: at least one padded slot, so the sort never sees an empty input
    int finish(hipStream_t s, long long items, long long slots, uint32_t nkeys)
    {
        const long long pad_blocks = std::min<long long>(4096, (slots + 255) / 256);
        hipLaunchKernelGGL(k_brick_pad, dim3((unsigned)pad_blocks), dim3(256), 0, s, counts, offs, items, keys[0], vals[0], slots, nkeys);
        MVSIM_HIP(hipGetLastError());
        int end_bit = 1;                     // the bits of the pad key, the largest key there is
        while (end_bit < 32 && ((uint64_t)nkeys >> end_bit) != 0) ++end_bit;
        size_t t = tmp->bytes;
        MVSIM_TRY(sort(s, tmp->p, t, (int)slots, end_bit));
        hipLaunchKernelGGL(k_brick_starts, dim3((unsigned)(((long long)nkeys + 1 + 255) / 256)), dim3(256), 0, s, keys[1], slots, starts, nkeys);
        MVSIM_HIP(hipGetLastError());
        return MVSIM_OK;
    }

private:
    // the size query (storage null) and the sort itself
    int sort(hipStream_t s, void* storage, size_t& bytes, int slots, int end_bit)
    {
        MVSIM_HIP(hipcub::DeviceRadixSort::SortPairs(storage, bytes, (const uint32_t*)keys[0], keys[1], (const uint32_t*)vals[0], vals[1], slots, 0,
                                                     end_bit, s));
        return MVSIM_OK;
    }
};

// ---- the render kernels' frame: 256 lanes, lane = (xl, yl) of the brick's 32 x 8 columns, BZ voxels per lane ---------------------
struct BrickLane {
    int       bx0, by0, bzi, bz0;            // the brick's first voxel; bzi = its index along z
    int       xl, yl, x, y;
    bool      inxy;                          // the lane's column lies inside the image
    long long row, base;                     // voxels per plane; the column's voxel in plane 0 (0 outside the image)
};

__device__ __forceinline__ BrickLane brick_lane(uint32_t brick, const BrickGrid& g, int nx, int ny)
{
    BrickLane f;
    f.bx0 = (int)(brick % (uint32_t)g.nbx) * BX;
    f.by0 = (int)((brick / (uint32_t)g.nbx) % (uint32_t)g.nby) * BY;
    f.bzi = (int)(brick / ((uint32_t)g.nbx * (uint32_t)g.nby));
    f.bz0 = f.bzi * BZ;
    f.xl = threadIdx.x & 31;                 // lanes 0-31 / 32-63 of a wave: two rows
    f.yl = threadIdx.x >> 5;
    f.x = f.bx0 + f.xl;
    f.y = f.by0 + f.yl;
    f.inxy = f.x < nx && f.y < ny;
    f.row = (long long)nx * ny;
    f.base = f.inxy ? (long long)f.x + (long long)nx * f.y : 0;
    return f;
}

// the per-axis factor tables of a chunk of m Gaussians over the brick's extent: exp(-(d * d) / tss) inside the item's box, +0.0 outside
__device__ __forceinline__ void brick_fill_tables(int m, const BrickLane& f, const double tss[3], double (*s_tab)[NTAB], const double (*s_loc)[3],
                                                  const int (*s_lo)[3], const int (*s_hi)[3])
{
    for (int t = threadIdx.x; t < m * NTAB; t += 256) {
        const int c = t / NTAB, i = t - c * NTAB;
        const int d = i < BX ? 0 : (i < BX + BY ? 1 : 2);
        const int pos = d == 0 ? f.bx0 + i : (d == 1 ? f.by0 + i - BX : f.bz0 + i - BX - BY);
        double v = 0.0;
        if (pos >= s_lo[c][d] && pos <= s_hi[c][d]) {
            const double xd = s_loc[c][d] - (double)pos;
            v = exp(-(xd * xd) / tss[d]);
        }
        s_tab[c][i] = v;
    }
}

}  // namespace

}  // namespace mvsim
