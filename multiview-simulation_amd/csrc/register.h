// What register.hip (the kernels of the bead registration: neighbours, descriptors, matching, RANSAC, refit) and api_register.cpp
// (its driver) share.
#pragma once

#include "common.h"

namespace mvsim {

// launch geometry (mvsim_match_geometry reports it).  A block of the two all-pairs kernels is ONE wave of REG_QUERIES query lanes;
// k_knn stages REG_KNN_TILE candidate points per round in LDS, k_match REG_MATCH_TILE points of B with all their descriptors.  The
// other list is split over blockIdx.y so that small lists still fill the chip: with Q query blocks and T tiles,
// splits = min(T, max(1, ceil(REG_SPLIT_TARGET / Q))).  The RANSAC kernel stages REG_RANSAC_TILE candidate pairs per round.
constexpr int REG_QUERIES = 64, REG_KNN_TILE = 64, REG_MATCH_TILE = 32, REG_RANSAC_TILE = 256, REG_SPLIT_TARGET = 1024;

struct RegSplit { int qblocks, tiles, splits, tiles_per_split; };
inline RegSplit reg_split(int64_t queries, int64_t points, int tile)
{
    RegSplit g;
    g.qblocks = (int)((queries + REG_QUERIES - 1) / REG_QUERIES);
    g.tiles = (int)((points + tile - 1) / tile);
    const int want = std::min(g.tiles, std::max(1, (REG_SPLIT_TARGET + g.qblocks - 1) / g.qblocks));
    g.tiles_per_split = (g.tiles + want - 1) / want;
    g.splits = (g.tiles + g.tiles_per_split - 1) / g.tiles_per_split;
    return g;
}

struct RegList {                 // a point list as the kernels take it
    const char*      pos;        // 3 doubles at `stride` bytes
    long long        stride;
    const long long* n_dev;
    long long        capacity;
};

// step 1.  part_d2 / part_idx: splits x capacity x K partial entries
int launch_knn(hipStream_t s, const RegList& L, int K, const RegSplit& g, double* part_d2, int* part_idx, int32_t* idx, double* d2);
// step 2.  counts into *n_described
int launch_descriptors(hipStream_t s, const RegList& L, int K, const int32_t* idx, double* desc, long long* n_described);
// step 3.  part: splits x (capacity_a x S) partial top-2 entries (RegTop2); best: capacity_a records
struct RegTop2 { double v1, v2; int b1, b2; };
int launch_match(hipStream_t s, const double* desc_a, const long long* n_a, long long cap_a, const double* desc_b, const long long* n_b,
                 long long cap_b, int K, double ratio2, const RegSplit& g, RegTop2* part, mvsim_match* best, long long capacity,
                 mvsim_match* candidates, long long* n_candidates);
// steps 5 and 6.  pq: 6 doubles per candidate; key: one 64-bit word; mask: one byte per candidate (the caller's or a workspace)
struct RegRansac {
    double    eps2, min_inlier_ratio;
    long long seed;
    int       hypotheses, max_refits, min_inliers;
};
int launch_ransac(hipStream_t s, const RegList& A, const RegList& B, const mvsim_match* cand, const long long* n_cand, long long capacity,
                  const RegRansac& R, double* pq, unsigned long long* key, unsigned char* mask, mvsim_registration* result);
// n_a, n_b of the result from the two counts of step 2
int launch_set_counts(hipStream_t s, const long long* n_desc_a, const long long* n_desc_b, mvsim_registration* result);

}  // namespace mvsim
