// C ABI of libmvsim, part 5: the multi-view deconvolution (mvsim.h states the recipe) -- per view and iteration two convolutions of the
// library with an explicit device PSF (convolve_with_psf) and the two elementwise kernels of deconvolve.hip between and behind them.
// Host orchestration only; everything is enqueued on the context's stream.
#include "api_internal.h"
#include "decon.h"

namespace mvsim {

void decon_flip_psf_host(const float* psf, const int64_t kdim[3], float* out, int64_t out_kdim[3])
{
    int64_t lead[3];
    for (int d = 0; d < 3; ++d) { lead[d] = (kdim[d] & 1) ? 0 : 1; out_kdim[d] = kdim[d] + lead[d]; }
    std::fill(out, out + out_kdim[0] * out_kdim[1] * out_kdim[2], 0.0f);
    for (int64_t z = 0; z < kdim[2]; ++z)
        for (int64_t y = 0; y < kdim[1]; ++y)
            for (int64_t x = 0; x < kdim[0]; ++x)
                out[(lead[0] + x) + out_kdim[0] * ((lead[1] + y) + out_kdim[1] * (lead[2] + z))] =
                    psf[(kdim[0] - 1 - x) + kdim[0] * ((kdim[1] - 1 - y) + kdim[1] * (kdim[2] - 1 - z))];
}

namespace {

constexpr size_t PSF_ALIGN = 64;     // floats: every prepared PSF starts on a 256-byte boundary of the context's buffer

inline size_t psf_round(int64_t n) { return ((size_t)n + PSF_ALIGN - 1) / PSF_ALIGN * PSF_ALIGN; }

inline bool overlaps(const void* a, const void* b, size_t bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

// the layout of decon_stat: [DECON_MAX_BLOCKS partials][MVSIM_MAX_VIEWS view sums][the statistics of every step]
constexpr size_t STAT_OFF_SUMS = (size_t)DECON_MAX_BLOCKS * sizeof(DeconPartial);
constexpr size_t STAT_OFF_STEPS = STAT_OFF_SUMS + (size_t)MVSIM_MAX_VIEWS * sizeof(double);

int stat_reserve(mvsim_ctx* ctx, size_t steps)
{
    return ctx->decon_stat.reserve(STAT_OFF_STEPS + steps * sizeof(mvsim_decon_stat));
}
inline DeconPartial* stat_partials(mvsim_ctx* ctx) { return ctx->decon_stat.as<DeconPartial>(); }
inline double* stat_sums(mvsim_ctx* ctx) { return reinterpret_cast<double*>(ctx->decon_stat.as<char>() + STAT_OFF_SUMS); }
inline mvsim_decon_stat* stat_steps(mvsim_ctx* ctx) { return reinterpret_cast<mvsim_decon_stat*>(ctx->decon_stat.as<char>() + STAT_OFF_STEPS); }

int check_params(const mvsim_decon_params* p)
{
    MVSIM_CHECK_ARG(p != nullptr, "deconvolve: params is null");
    MVSIM_CHECK_ARG(p->iterations >= 1, "deconvolve: iterations must be >= 1");
    MVSIM_CHECK_ARG(p->method >= 0 && p->method <= 2, "deconvolve: method must be 0, 1 or 2");
    MVSIM_CHECK_ARG(p->init_from_psi == 0 || p->init_from_psi == 1, "deconvolve: init_from_psi must be 0 or 1");
    MVSIM_CHECK_ARG(p->eps > 0.0f, "deconvolve: eps must be > 0");
    MVSIM_CHECK_ARG(p->min_value > 0.0f, "deconvolve: min_value must be > 0");
    MVSIM_CHECK_ARG(p->lambda >= 0.0, "deconvolve: lambda must be >= 0");
    return MVSIM_OK;
}

// everything mvsim_deconvolve* refuses that does not depend on where the volumes live
int check_args(const float* const* views, const float* const* weights, const float* const* psf_host, const int64_t* kdims, int n_views,
               const int64_t dim[3], const mvsim_decon_params* p, const float* psi)
{
    MVSIM_CHECK_ARG(n_views >= 1 && n_views <= MVSIM_MAX_VIEWS, "deconvolve: n_views must be in [1, MVSIM_MAX_VIEWS]");
    MVSIM_TRY(check_params(p));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(views && psf_host && kdims && psi, "deconvolve: null pointer");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    for (int v = 0; v < n_views; ++v) {
        MVSIM_CHECK_ARG(views[v] != nullptr, "deconvolve: null view pointer");
        MVSIM_CHECK_ARG(!weights || weights[v] != nullptr, "deconvolve: null weight pointer (weights: all views or none)");
        MVSIM_CHECK_ARG(psf_host[v] != nullptr, "deconvolve: null psf pointer");
        const int64_t* k = kdims + 3 * v;
        MVSIM_CHECK_ARG(k[0] >= 1 && k[1] >= 1 && k[2] >= 1, "deconvolve: psf dimensions must be >= 1");
        MVSIM_CHECK_ARG(k[0] <= 65535 && k[1] <= 65535 && k[2] <= 65535, "deconvolve: psf dimension too large");
        MVSIM_CHECK_ARG(!overlaps(psi, views[v], bytes), "deconvolve: psi overlaps a view");
        MVSIM_CHECK_ARG(!weights || !overlaps(psi, weights[v], bytes), "deconvolve: psi overlaps a weight");
    }
    return MVSIM_OK;
}

struct PsfSlot {
    size_t  off_p, off_f;     // floats into decon_psf: the normalised PSF and its flipped twin
    int64_t kf[3];            // the twin's extents
};

// copies, normalises and flips every PSF on the host and uploads all 2 V of them in one transfer
int upload_psfs(mvsim_ctx* ctx, const float* const* psf_host, const int64_t* kdims, int n_views, std::vector<PsfSlot>* slots)
{
    slots->resize((size_t)n_views);
    size_t total = 0;
    for (int v = 0; v < n_views; ++v) {
        const int64_t* k = kdims + 3 * v;
        PsfSlot& sl = (*slots)[(size_t)v];
        for (int d = 0; d < 3; ++d) sl.kf[d] = k[d] | 1;
        sl.off_p = total; total += psf_round(k[0] * k[1] * k[2]);
        sl.off_f = total; total += psf_round(sl.kf[0] * sl.kf[1] * sl.kf[2]);
    }
    MVSIM_TRY(ctx->decon_psf.reserve(total * sizeof(float)));
    int slot = 0;
    MVSIM_TRY(ctx->pinned.acquire(total * sizeof(float), &slot));
    float* h = reinterpret_cast<float*>(ctx->pinned.p[slot]);
    std::memset(h, 0, total * sizeof(float));
    for (int v = 0; v < n_views; ++v) {
        const int64_t* k = kdims + 3 * v;
        const PsfSlot& sl = (*slots)[(size_t)v];
        const int64_t n = k[0] * k[1] * k[2];
        std::memcpy(h + sl.off_p, psf_host[v], (size_t)n * sizeof(float));
        psf_normalise_host(h + sl.off_p, n);
        int64_t kf[3];
        decon_flip_psf_host(h + sl.off_p, k, h + sl.off_f, kf);
    }
    MVSIM_HIP(hipMemcpyAsync(ctx->decon_psf.p, h, total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    MVSIM_HIP(hipEventRecord(ctx->pinned.ev[slot], ctx->stream));
    ctx->pinned.busy[slot] = true;
    return MVSIM_OK;
}

// the loop over iterations and views on device volumes; arguments checked by the caller.  stats_dev_out: true when the steps' statistics
// lie in stat_steps(ctx) behind what this enqueued
int deconvolve_enqueue(mvsim_ctx* ctx, const float* const* views, const float* const* weights, const float* const* psf_host,
                       const int64_t* kdims, int n_views, const int64_t dim[3], const mvsim_decon_params& p, float* psi, bool want_stats)
{
    const int64_t n = nvox(dim);
    const size_t bytes = (size_t)n * sizeof(float);
    std::vector<PsfSlot> slots;
    MVSIM_TRY(upload_psfs(ctx, psf_host, kdims, n_views, &slots));
    MVSIM_TRY(ctx->decon_work[0].reserve(bytes));
    MVSIM_TRY(ctx->decon_work[1].reserve(bytes));
    MVSIM_TRY(stat_reserve(ctx, want_stats ? (size_t)p.iterations * n_views : 0));
    float* work_b = ctx->decon_work[0].as<float>();
    float* work_c = ctx->decon_work[1].as<float>();
    const float* psfs = ctx->decon_psf.as<float>();

    if (!p.init_from_psi) {
        if (p.init_value > 0.0f) {
            MVSIM_TRY(launch_decon_fill(ctx->stream, psi, n, nullptr, n_views, p.init_value, p.min_value));
        } else {
            double *partial, *scal;
            MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
            for (int v = 0; v < n_views; ++v) MVSIM_TRY(launch_sum(ctx->stream, views[v], n, partial, stat_sums(ctx) + v));
            MVSIM_TRY(launch_decon_fill(ctx->stream, psi, n, stat_sums(ctx), n_views, 0.0f, p.min_value));
        }
    }
    for (int it = 0; it < p.iterations; ++it)
        for (int v = 0; v < n_views; ++v) {
            const PsfSlot& sl = slots[(size_t)v];
            MVSIM_TRY(convolve_with_psf(ctx, psi, dim, psfs + sl.off_p, kdims + 3 * v, p.method, work_b));
            MVSIM_TRY(launch_decon_ratio(ctx->stream, views[v], work_b, n, p.eps, work_b));
            MVSIM_TRY(convolve_with_psf(ctx, work_b, dim, psfs + sl.off_f, sl.kf, p.method, work_c));
            mvsim_decon_stat* st = want_stats ? stat_steps(ctx) + ((size_t)it * n_views + v) : nullptr;
            MVSIM_TRY(launch_decon_update(ctx->stream, psi, work_c, weights ? weights[v] : nullptr, n, p.min_value, p.lambda,
                                          stat_partials(ctx), st));
        }
    return MVSIM_OK;
}

}  // namespace

}  // namespace mvsim

using namespace mvsim;

extern "C" {

void mvsim_decon_params_default(mvsim_decon_params* p)
{
    if (!p) return;
    p->iterations = 10; p->method = 0; p->init_from_psi = 0; p->init_value = 0.0f; p->min_value = 0.0001f; p->eps = 1e-6f; p->lambda = 0.0;
}

int mvsim_decon_flip_psf(const float* psf, const int64_t kdim[3], float* out, int64_t out_kdim[3])
{
    if (!psf || !kdim || !out || !out_kdim) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    MVSIM_CHECK_ARG(kdim[0] >= 1 && kdim[1] >= 1 && kdim[2] >= 1, "psf dimensions must be >= 1");
    decon_flip_psf_host(psf, kdim, out, out_kdim);
    return MVSIM_OK;
}

int mvsim_decon_geometry(int64_t out[2])
{
    if (!out) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    out[0] = DECON_MAX_BLOCKS; out[1] = DECON_BLOCK_ELEMS;
    return MVSIM_OK;
}

int mvsim_decon_ratio_dev(mvsim_ctx* ctx, const float* phi, const float* blurred, int64_t n, float eps, float* ratio)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(phi && blurred && ratio && n >= 1, "null buffer or empty image");
    MVSIM_CHECK_ARG(eps > 0.0f, "eps must be > 0");
    return launch_decon_ratio(ctx->stream, phi, blurred, n, eps, ratio);
}

int mvsim_decon_update_dev(mvsim_ctx* ctx, float* psi, const float* corr, const float* weight_or_null, int64_t n, float min_value,
                           double lambda, mvsim_decon_stat* stat_host_or_null)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(psi && corr && n >= 1, "null buffer or empty image");
    MVSIM_CHECK_ARG(min_value > 0.0f, "min_value must be > 0");
    MVSIM_CHECK_ARG(lambda >= 0.0, "lambda must be >= 0");
    if (!stat_host_or_null) return launch_decon_update(ctx->stream, psi, corr, weight_or_null, n, min_value, lambda, nullptr, nullptr);
    MVSIM_TRY(stat_reserve(ctx, 1));
    MVSIM_TRY(launch_decon_update(ctx->stream, psi, corr, weight_or_null, n, min_value, lambda, stat_partials(ctx), stat_steps(ctx)));
    MVSIM_HIP(hipMemcpyAsync(stat_host_or_null, stat_steps(ctx), sizeof(mvsim_decon_stat), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

int mvsim_deconvolve_dev(mvsim_ctx* ctx, const float* const* views_dev, const float* const* weights_dev_or_null,
                         const float* const* psf_host, const int64_t* kdims, int n_views, const int64_t dim[3],
                         const mvsim_decon_params* params, float* psi_dev, mvsim_decon_stat* stats_or_null)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_args(views_dev, weights_dev_or_null, psf_host, kdims, n_views, dim, params, psi_dev));
    MVSIM_TRY(deconvolve_enqueue(ctx, views_dev, weights_dev_or_null, psf_host, kdims, n_views, dim, *params, psi_dev, stats_or_null != nullptr));
    if (stats_or_null) {
        MVSIM_HIP(hipMemcpyAsync(stats_or_null, stat_steps(ctx), (size_t)params->iterations * n_views * sizeof(mvsim_decon_stat),
                                 hipMemcpyDeviceToHost, ctx->stream));
        MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MVSIM_OK;
}

int mvsim_deconvolve(mvsim_ctx* ctx, const float* const* views, const float* const* weights_or_null, const float* const* psf_host,
                     const int64_t* kdims, int n_views, const int64_t dim[3], const mvsim_decon_params* params, float* psi,
                     mvsim_decon_stat* stats_or_null)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_args(views, weights_or_null, psf_host, kdims, n_views, dim, params, psi));
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    // device twins of the caller's volumes, for this call only: V views, V weights, the estimate
    const int nw = weights_or_null ? n_views : 0;
    std::vector<DevBuf> bufs((size_t)(n_views + nw + 1));
    std::vector<const float*> dv((size_t)n_views), dw((size_t)nw);
    int rc = MVSIM_OK;
    for (int v = 0; v < n_views && rc == MVSIM_OK; ++v) {
        rc = up(ctx, bufs[(size_t)v], views[v], bytes);
        dv[(size_t)v] = bufs[(size_t)v].as<float>();
    }
    for (int v = 0; v < nw && rc == MVSIM_OK; ++v) {
        rc = up(ctx, bufs[(size_t)(n_views + v)], weights_or_null[v], bytes);
        dw[(size_t)v] = bufs[(size_t)(n_views + v)].as<float>();
    }
    DevBuf& dpsi = bufs.back();
    if (rc == MVSIM_OK) rc = params->init_from_psi ? up(ctx, dpsi, psi, bytes) : dpsi.reserve(bytes);
    if (rc == MVSIM_OK)
        rc = mvsim_deconvolve_dev(ctx, dv.data(), nw ? dw.data() : nullptr, psf_host, kdims, n_views, dim, params, dpsi.as<float>(), stats_or_null);
    if (rc == MVSIM_OK) rc = down(ctx, psi, dpsi.p, bytes);
    (void)hipStreamSynchronize(ctx->stream);
    for (DevBuf& b : bufs) b.release();
    return rc;
}

}  // extern "C"
