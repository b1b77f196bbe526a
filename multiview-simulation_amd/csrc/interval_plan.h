// The host-side plan of extractSlices over an Interval of a volume that stays on the device -- Views.zeroMin(Views.interval(con, min, max))
// of SimulateTileStitching.java:131-189: the tile's geometry inside the volume and its validation (IntervalGeom), the sampler form, grid and
// queue geometry of one launch (IntervalPlan: an ExtractPlan of the zero-min tile, extract_plan.h), which jobs of a call share launches,
// and the reference's two tile intervals (tile_interval).  Plain C++, no HIP include (tests/c_abi/interval_plan_main.cpp: g++ alone).
#pragma once

#include <cmath>

#include "extract_plan.h"

namespace mvsim {

// What one interval job reads: tile voxel (x, y, k) is the volume's voxel in_offset + x + row_pitch * y + plane_pitch * k * inc, and its RNG
// counter its index in the ZERO-MIN tile, x + tile[0] * (y + tile[1] * k * inc) -- the interval is treated as zero-min, so a
// tile's counts are those of mvsim_extract_slices on the cropped tile.
struct IntervalGeom {
    int64_t   tile[3];            // max - min + 1
    int       inc;
    long long row_pitch;          // dim[0]
    long long plane_pitch;        // dim[0] * dim[1]
    long long in_offset;          // the min corner, in voxels from the volume's first (64-bit: 2048 x 2048 x 512 and beyond)
    long long nzo() const { return (long long)((tile[2] - 1) / inc + 1); }
    long long n_out() const { return (long long)tile[0] * tile[1] * nzo(); }
    // the zero-min tile as the extract stage sees a volume: every inc-th plane, counters from 0
    ExtractGeom tile_geom() const { ExtractGeom g = ExtractGeom::strided(tile, inc); g.in_offset = in_offset; return g; }
};

// The geometry of the interval [mn, mx] (inclusive corners) of a volume of dim voxels; null, or what is wrong with it.  The limits on dim
// are those of every stage operator (api_internal.h: check_dim).
inline const char* interval_geom(const int64_t dim[3], const int64_t mn[3], const int64_t mx[3], int inc, IntervalGeom* g)
{
    if (!dim || !mn || !mx || !g) return "null pointer";
    if (inc < 1) return "inc must be >= 1";
    if (dim[0] < 1 || dim[1] < 1 || dim[2] < 1) return "dimensions must be >= 1";
    if (dim[0] > 65535 * 4 || dim[1] > 65535 || dim[2] > 65535) return "dimension too large for one launch";
    for (int d = 0; d < 3; ++d) {
        if (mn[d] > mx[d]) return "interval: min > max";
        if (mn[d] < 0 || mx[d] >= dim[d]) return "interval leaves the volume";
        g->tile[d] = mx[d] - mn[d] + 1;
    }
    g->inc = inc;
    g->row_pitch = (long long)dim[0];
    g->plane_pitch = (long long)dim[0] * dim[1];
    g->in_offset = (long long)mn[0] + g->row_pitch * mn[1] + g->plane_pitch * mn[2];
    return nullptr;
}

// One launch (per sampler stage) of interval jobs: the plan of the zero-min tile.  xp.kernel says what runs -- EXTRACT_K_NOISE2_ANY: phase 1
// group by group (k_extract_interval_noise2) and the resolver on its queue; EXTRACT_K_SCALAR: one voxel per lane (k_extract_interval; the
// copy, and the sampler where extract_plan gives no queue) --; mvsim_get_extract_path reports both as EXTRACT_K_INTERVAL.
struct IntervalPlan {
    IntervalGeom ig;
    ExtractPlan  xp;
};
// (aligned16 = false: a tile's rows start anywhere, the vector forms never apply)
inline IntervalPlan interval_plan(const IntervalGeom& ig, bool noise, QueueMode mode) { return {ig, extract_plan(ig.tile_geom(), false, noise, mode)}; }

// Jobs share launches (blockIdx.y = job) when everything the resolver takes from its ONE ResolveJob is the same for them: the tile's size,
// the plane stride and the factor lambda = v * mul, i.e. the snr (its bits; copies among themselves).  Their volumes, corners, seeds and
// streams may differ: those come from the per-job tables.
struct IntervalKey {
    int64_t  tile[3];
    int      inc;
    bool     noise;
    uint32_t snr_bits;
    bool operator==(const IntervalKey& o) const
    {
        return tile[0] == o.tile[0] && tile[1] == o.tile[1] && tile[2] == o.tile[2] && inc == o.inc && noise == o.noise && (!noise || snr_bits == o.snr_bits);
    }
};

// SimulateTileStitching.java:119-121, 214-234 with its quirks: overlap_d = (int)Math.round(dim_d * ratio_d / 2); tile 0 is
// [0, dim_d / 2 + overlap_d]; tile 1 is [dim_0 / 2 - overlap_d, dim_d - 1] -- dimension(0) in EVERY dimension, as the reference has it.
// Nothing is validated here: a ratio of 1 gives a tile 0 that leaves the volume, and extracting it is refused.
inline void tile_interval(const int64_t dim[3], const double ratio[3], int tile, int64_t mn[3], int64_t mx[3], int64_t overlap[3])
{
    for (int d = 0; d < 3; ++d) {
        const int ov = (int)(long long)std::floor((double)dim[d] * ratio[d] / 2 + 0.5);      // Math.round(double): floor(x + 1/2)
        overlap[d] = ov;
        mn[d] = 0; mx[d] = dim[d] - 1;
        if (tile == 0) mx[d] = (int)dim[d] / 2 + ov;
        else mn[d] = (int)dim[0] / 2 - ov;
    }
}

}  // namespace mvsim
