// What deconvolve.hip (the elementwise kernels of the multi-view deconvolution) and api_decon.cpp (its driver) share.
#pragma once

#include "common.h"

namespace mvsim {

// launch geometry of the elementwise kernels: at most DECON_MAX_BLOCKS blocks of 256 threads, each taking DECON_BLOCK_ELEMS voxels per
// trip of its grid-stride loop (mvsim_decon_geometry reports the two)
constexpr int DECON_MAX_BLOCKS = 2048;
constexpr int DECON_BLOCK_ELEMS = 256 * 4;

struct DeconPartial {        // a block's share of the update's statistics, in the block's own slot
    double    sum;
    long long floored;
    float     maxc, pad;
};

// ratio may be blurred (in place); any alignment, any n >= 1
int launch_decon_ratio(hipStream_t s, const float* phi, const float* blurred, int64_t n, float eps, float* ratio);
// step 4 of the recipe in place on psi; w may be null.  stat_dev non-null: the statistics of this step into *stat_dev (device memory)
// through `partial` (DECON_MAX_BLOCKS slots)
int launch_decon_update(hipStream_t s, float* psi, const float* corr, const float* w, int64_t n, float min_value, double lambda,
                        DeconPartial* partial, mvsim_decon_stat* stat_dev);
// psi = max(min_value, constant), or -- sums_dev non-null -- max(min_value, (float)(mean over views of sums_dev[v] / n))
int launch_decon_fill(hipStream_t s, float* psi, int64_t n, const double* sums_dev_or_null, int n_views, float constant, float min_value);
// the correlation kernel of the recipe: out[j] = psf[K - 1 - j] per axis behind one leading zero on every axis of even extent
void decon_flip_psf_host(const float* psf, const int64_t kdim[3], float* out, int64_t out_kdim[3]);

}  // namespace mvsim
