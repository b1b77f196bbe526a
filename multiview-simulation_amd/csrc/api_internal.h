// What the translation units of the C ABI share: api.cpp (context, options, memory, stage operators on device buffers, queries),
// api_view.cpp (the per-view pipeline on device buffers), api_host.cpp (host-buffer entry points), api_sims.cpp (phantom, bead and
// refraction-simulator wrappers), api_decon.cpp (the multi-view deconvolution), api_detect.cpp (the bead detector), api_register.cpp (the bead
// registration), api_fuse.cpp (the view fusion), api_psf.cpp (the PSF extraction).  Host orchestration only.
#pragma once

#include "common.h"
#include "host_pool.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mvsim {

// every entry point starts here: the device, and a pending tail ordered in front of what the call enqueues (api.cpp)
int set_device(mvsim_ctx* ctx, bool keep_tail = false);
// The one way to a context's extract + Poisson stage (api.cpp): the queue mode of this launch, its plan, the queue workspace, the launch
// between the stage's markers on ctx->stream, the form taken left in ctx->extract_path; ops.queue_ws is the stage's to fill.  In two steps
// where the plan is needed first: stacked views (the queue regions of their table; views_aligned16 = every view's buffers), view_enqueue.
int extract_stage_plan(mvsim_ctx* ctx, const ExtractGeom& g, const ExtractOps& ops, ExtractPlan* pl, bool views_aligned16 = false);
int extract_stage_run(mvsim_ctx* ctx, const ExtractPlan& pl, ExtractOps& ops);
// known before the convolution is enqueued: the launch behind it will be one of the two queue samplers (extract_plan.h: tail_queue_sampler)
bool extract_stage_queued(mvsim_ctx* ctx, const int64_t dim[3], int inc, bool noise);
int extract_stage(mvsim_ctx* ctx, const ExtractGeom& g, ExtractOps& ops);
// extractSlices over intervals of device volumes (api.cpp): the jobs checked against everything mvsim_extract_intervals* refuses but the
// outputs (geoms: one per job), and the launches of checked jobs into DEVICE outputs, asynchronous on ctx->stream
int interval_jobs_check(const mvsim_interval_job* jobs, int n, std::vector<IntervalGeom>* geoms);
int extract_intervals_enqueue(mvsim_ctx* ctx, const mvsim_interval_job* jobs, const std::vector<IntervalGeom>& geoms, float* const* out_dev);
int host_threads_of(const mvsim_ctx* ctx);
void psf_normalise_host(float* psf_host, int64_t n);
// cacheable: the call is a whole single view that may take its PSF's spectrum from the context's cache (psf_cache.h) -- then a PSF the
// context has seen is not uploaded, and ctx->psf_entry tells the convolution that follows; otherwise ctx->psf_dev receives the taps
int psf_prepare(mvsim_ctx* ctx, float* psf_host, const int64_t kdim[3], const int64_t dim[3], bool cacheable);
int convolve_dev_impl(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const int64_t kdim[3], int method, float* out,
                      ConvTail* tail = nullptr);
// the same convolution with an explicit device PSF (convolve_dev_impl: the context's own, or its cache entry's); neither method caches by
// the PSF's ADDRESS -- the cache is keyed by the taps themselves
int convolve_with_psf(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* psf_dev, const int64_t kdim[3], int method,
                      float* out, ConvTail* tail = nullptr);
void view_graphs_release(mvsim_ctx* ctx);                 // api_view.cpp
void async_release(mvsim_ctx* ctx);                       // api_host.cpp
// host buffer <-> workspace on the context's stream (api_host.cpp); down() returns with the data on the host
int up(mvsim_ctx* ctx, DevBuf& b, const float* h, size_t bytes);
int down(mvsim_ctx* ctx, float* h, const void* d, size_t bytes);

inline int check_dim(const int64_t dim[3])
{
    MVSIM_CHECK_ARG(dim != nullptr, "dim is null");
    MVSIM_CHECK_ARG(dim[0] >= 1 && dim[1] >= 1 && dim[2] >= 1, "dimensions must be >= 1");
    MVSIM_CHECK_ARG(dim[0] <= 65535 * 4 && dim[1] <= 65535 && dim[2] <= 65535, "dimension too large for one launch");
    return MVSIM_OK;
}

inline int64_t nvox(const int64_t dim[3]) { return dim[0] * dim[1] * dim[2]; }

inline int pick_method(int method, const int64_t kdim[3])
{
    if (method == 1 || method == 2) return method;
    // direct stencil costs 2*K^3 flop/voxel; measured at 512^3 (tools/stencil_bench.py, profiles/r03_stencil_bench.txt): 3^3
    // 0.67x the FFT passes' time, 5^3 1.06x, 7^3 1.76x -- the FFT path takes over between 4 and 5 taps per axis
    return (kdim[0] * kdim[1] * kdim[2] <= 4 * 4 * 4) ? 2 : 1;
}

inline int scal_ptr(mvsim_ctx* ctx, double** partial, double** scal)
{
    MVSIM_TRY(ctx->partials.reserve(PARTIALS_BYTES));
    *partial = ctx->partials.as<double>();
    *scal = scal_of(ctx);
    return MVSIM_OK;
}

// The host slabs of the *_zslabs entry points belong to the caller again when the call returns -- on EVERY path: copies from
// page-locked slabs are truly asynchronous, so an error return must not leave one in flight.
struct SyncOnExit {
    mvsim_ctx* c;
    ~SyncOnExit() { if (c && c->stream) (void)hipStreamSynchronize(c->stream); }
};
struct StreamSwap {               // enqueue on another stream for a scope; the context's stream comes back on every exit path
    mvsim_ctx* c;
    hipStream_t saved;
    StreamSwap(mvsim_ctx* ctx, hipStream_t s) : c(ctx), saved(ctx->stream) { ctx->stream = s; }
    ~StreamSwap() { c->stream = saved; }
};

}  // namespace mvsim
