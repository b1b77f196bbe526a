// What fuse.hip (the kernels of the view fusion: prepare, resample + blend) and api_fuse.cpp (its driver) share.
#pragma once

#include "common.h"

namespace mvsim {

// launch geometry (mvsim_fusion_geometry reports it).  A block of FUSE_BX * FUSE_BY threads owns a brick of FUSE_BX x FUSE_BY x FUSE_BZ
// output voxels: one wave per output row, lanes along x, every thread walks the brick's FUSE_BZ planes.  At most FUSE_MAX_BLOCKS blocks
// are launched; the bricks (x fastest) are cut into 8 consecutive runs, one per XCD, and the blocks of an XCD walk its run.
constexpr int FUSE_BX = 64, FUSE_BY = 4, FUSE_BZ = 4, FUSE_XCDS = 8, FUSE_MAX_BLOCKS = 4096;
constexpr int FUSE_PREPARE_BATCH = 16;                   // views one prepare launch takes in its kernel arguments

struct FuseViewRec {             // one view as the fuse kernel reads it (context workspace, written by the prepare kernel)
    double      inv[12];         // step 1; unspecified when singular
    const void* src;
    long long   dim[3];
    float*      aligned;         // aligned mode: the view's two outputs, either may be null
    float*      weight;
    int         singular, pad;
};

struct FuseViewArg {             // one view as the prepare kernel takes it, by value
    const void*   src;
    long long     dim[3];
    const double* m_dev;         // non-null: the matrix is read from device memory
    double        m[12];
    float*        aligned;
    float*        weight;
};
struct FusePrepareArgs { FuseViewArg v[FUSE_PREPARE_BATCH]; };

struct FuseJob {
    long long out_min[3], out_dim[3];
    double    blend[3];
    float     background;
    int       src_type, n_views;
};

// views [first, first + n) of a call into recs (and status, when given)
int launch_fuse_prepare(hipStream_t s, const FusePrepareArgs& a, int first, int n, FuseViewRec* recs, int32_t* status_or_null);
// fused != null: steps 2-6 into fused (and sum_weights); else step 7 into every record's aligned / weight
int launch_fuse(hipStream_t s, const FuseJob& job, const FuseViewRec* recs, float* fused, float* sum_weights);

}  // namespace mvsim
