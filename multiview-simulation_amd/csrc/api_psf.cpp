// C ABI of libmvsim, part 9: the PSF extraction (mvsim.h states the recipe) -- the beads of one view averaged into that view's PSF in
// the output frame.  Host orchestration only: the argument checks, the launches of psf.hip on the context's stream, and the host
// helpers that restate steps 1-3 and 6 with the arithmetic of psf_dev.h; no _dev entry point reads anything back, so detection,
// registration, extraction and deconvolution chain without a synchronisation.
// Every argument is checked before the context is touched, so each refusal can be reached without a device.
#include "api_internal.h"
#include "psf.h"
#include "psf_dev.h"

#include <limits>
#include <vector>

namespace mvsim {

namespace {

int check_params(const mvsim_psf_params* p)
{
    MVSIM_CHECK_ARG(p != nullptr, "psf: null pointer");
    for (int d = 0; d < 3; ++d) {
        MVSIM_CHECK_ARG(p->kdim[d] >= 1 && p->kdim[d] <= MVSIM_PSF_MAX_DIM && (p->kdim[d] & 1) == 1,
                        "psf: kdim entries must be odd and in [1, MVSIM_PSF_MAX_DIM]");
        MVSIM_CHECK_ARG(std::isfinite(p->min_separation[d]) && p->min_separation[d] >= 0.0, "psf: min_separation must be finite and >= 0");
    }
    MVSIM_CHECK_ARG(p->src_type == MVSIM_SRC_F32 || p->src_type == MVSIM_SRC_U16, "psf: src_type must be MVSIM_SRC_F32 or MVSIM_SRC_U16");
    return MVSIM_OK;
}

int check_image_dim(const int64_t dim[3])
{
    MVSIM_CHECK_ARG(dim != nullptr, "psf: null pointer");
    for (int d = 0; d < 3; ++d) MVSIM_CHECK_ARG(dim[d] >= 1 && dim[d] < ((int64_t)1 << 31), "psf: every extent must be >= 1");
    MVSIM_CHECK_ARG(nvox(dim) < ((int64_t)1 << 40), "psf: image too large");
    return MVSIM_OK;
}

int check_list(const void* pos, int64_t stride, const void* n_dev, int64_t capacity)
{
    MVSIM_CHECK_ARG(pos && n_dev, "psf: null pointer");
    MVSIM_CHECK_ARG(stride >= 24 && stride % 8 == 0, "psf: stride must be >= 24 and a multiple of 8");
    MVSIM_CHECK_ARG(capacity >= 1 && capacity <= MVSIM_PSF_MAX_POINTS, "psf: capacity must be in [1, MVSIM_PSF_MAX_POINTS]");
    return MVSIM_OK;
}

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const char *a0 = static_cast<const char*>(a), *b0 = static_cast<const char*>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

int64_t taps_of(const mvsim_psf_params& p) { return p.kdim[0] * p.kdim[1] * p.kdim[2]; }

PsfJob job_of(const int64_t dim[3], const mvsim_psf_params& p)
{
    PsfJob j;
    for (int d = 0; d < 3; ++d) { j.dim[d] = dim ? dim[d] : 1; j.kdim[d] = p.kdim[d]; j.min_separation[d] = p.min_separation[d]; }
    j.src_type = p.src_type;
    j.subtract_min = p.subtract_min != 0;
    j.normalize = p.normalize != 0;
    j.crowding = p.min_separation[0] != 0.0 || p.min_separation[1] != 0.0 || p.min_separation[2] != 0.0;
    return j;
}

PsfMatrix matrix_of(const double* m, const double* m_dev)
{
    PsfMatrix M;
    std::memset(&M, 0, sizeof(M));
    M.m_dev = m_dev;
    if (m) { std::memcpy(M.m, m, sizeof(M.m)); M.given = 1; }
    return M;
}

PsfList list_of(const void* pos, int64_t stride, const int64_t* n_dev, int64_t capacity)
{
    PsfList L;
    L.pos = static_cast<const char*>(pos);
    L.stride = stride;
    L.n_dev = reinterpret_cast<const long long*>(n_dev);
    L.capacity = capacity;
    return L;
}

// the workspace of steps 4 and 5: per-chunk partial sums (and, for the whole call, the totals)
int reserve_gather(mvsim_ctx* ctx, int64_t capacity, int64_t taps, bool totals)
{
    const int64_t chunks = (capacity + PSF_CHUNK - 1) / PSF_CHUNK;
    MVSIM_TRY(ctx->psfx_buf[0].reserve((size_t)(chunks * taps) * sizeof(double)));
    if (totals) MVSIM_TRY(ctx->psfx_buf[1].reserve((size_t)taps * sizeof(double)));
    return MVSIM_OK;
}

void record_clear(mvsim_psf_result* r, int64_t n)
{
    std::memset(r, 0, sizeof(*r));
    r->n_listed = n;
}

}  // namespace

}  // namespace mvsim

using namespace mvsim;

extern "C" {

void mvsim_psf_params_default(mvsim_psf_params* p)
{
    if (!p) return;
    for (int d = 0; d < 3; ++d) { p->kdim[d] = 15; p->min_separation[d] = 15.0; }
    p->src_type = MVSIM_SRC_F32;
    p->subtract_min = 1;
    p->normalize = 1;
    p->pad = 0;
}

int mvsim_psf_offsets(const double* m_or_null, const int64_t kdim[3], double* offsets, int* singular)
{
    MVSIM_CHECK_ARG(kdim && offsets && singular, "psf_offsets: null pointer");
    for (int d = 0; d < 3; ++d)
        MVSIM_CHECK_ARG(kdim[d] >= 1 && kdim[d] <= MVSIM_PSF_MAX_DIM && (kdim[d] & 1) == 1,
                        "psf_offsets: kdim entries must be odd and in [1, MVSIM_PSF_MAX_DIM]");
    double inv[12];
    *singular = psf_invert(m_or_null, inv) ? 0 : 1;
    if (*singular) return MVSIM_OK;
    int64_t t = 0;
    for (int64_t kz = 0; kz < kdim[2]; ++kz)
        for (int64_t ky = 0; ky < kdim[1]; ++ky)
            for (int64_t kx = 0; kx < kdim[0]; ++kx, ++t) {
                const double jx = (double)(kx - kdim[0] / 2), jy = (double)(ky - kdim[1] / 2), jz = (double)(kz - kdim[2] / 2);
                for (int r = 0; r < 3; ++r) offsets[3 * t + r] = psf_delta(inv + 4 * r, jx, jy, jz);
            }
    return MVSIM_OK;
}

int mvsim_psf_select(const void* pos, int64_t stride, int64_t n, const unsigned char* use_or_null, const double* m_or_null,
                     const int64_t dim[3], const mvsim_psf_params* params, unsigned char* status, mvsim_psf_result* result)
{
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(check_image_dim(dim));
    MVSIM_CHECK_ARG(result != nullptr && (n == 0 || (pos && status)), "psf_select: null pointer");
    MVSIM_CHECK_ARG(stride >= 24 && stride % 8 == 0, "psf: stride must be >= 24 and a multiple of 8");
    MVSIM_CHECK_ARG(n >= 0 && n <= MVSIM_PSF_MAX_POINTS, "psf_select: n must be in [0, MVSIM_PSF_MAX_POINTS]");
    const PsfJob job = job_of(dim, *params);
    record_clear(result, n);
    double inv[12];
    if (!psf_invert(m_or_null, inv)) { result->flags = MVSIM_PSF_SINGULAR; return MVSIM_OK; }
    auto point = [&](int64_t i) { return reinterpret_cast<const double*>(static_cast<const char*>(pos) + i * stride); };
    std::vector<unsigned char> finite((size_t)n);
    for (int64_t i = 0; i < n; ++i) finite[(size_t)i] = psf_finite3(point(i)) ? 1 : 0;
    for (int64_t i = 0; i < n; ++i) {
        const double* p = point(i);
        int st = MVSIM_PSF_USED;
        if (!finite[(size_t)i]) st = MVSIM_PSF_NONFINITE;
        else if (use_or_null && use_or_null[i] == 0) st = MVSIM_PSF_MASKED;
        else if (psf_outside(inv, job.kdim, job.dim, p)) st = MVSIM_PSF_OUTSIDE;
        else if (job.crowding) {
            for (int64_t j = 0; j < n && st == MVSIM_PSF_USED; ++j) {
                if (j == i || !finite[(size_t)j]) continue;
                const double* o = point(j);
                if (psf_crowds(p[0], p[1], p[2], o[0], o[1], o[2], job.min_separation)) st = MVSIM_PSF_CROWDED;
            }
        }
        status[i] = (unsigned char)st;
        int64_t* counts[5] = {&result->n_used, &result->n_nonfinite, &result->n_masked, &result->n_outside, &result->n_crowded};
        *counts[st] += 1;
    }
    return MVSIM_OK;
}

int mvsim_psf_finish(const double* totals, const mvsim_psf_params* params, float* psf, mvsim_psf_result* result)
{
    MVSIM_TRY(check_params(params));
    MVSIM_CHECK_ARG(totals && psf && result, "psf_finish: null pointer");
    const int64_t taps = taps_of(*params);
    const bool singular = (result->flags & MVSIM_PSF_SINGULAR) != 0;
    if (singular || result->n_used <= 0) {
        for (int64_t t = 0; t < taps; ++t) psf[t] = 0.0f;
        result->minimum = 0.0;
        result->sum = 0.0;
        if (!singular) result->flags |= MVSIM_PSF_NO_BEADS;
        return MVSIM_OK;
    }
    const double den = (double)result->n_used;
    double b = std::numeric_limits<double>::infinity();
    for (int64_t t = 0; t < taps; ++t) {
        const double mean = totals[t] / den;
        if (mean < b) b = mean;
    }
    double S = 0.0;
    for (int64_t t0 = 0; t0 < taps; t0 += PSF_CHUNK) {
        double s = 0.0;
        for (int64_t t = t0; t < std::min<int64_t>(t0 + PSF_CHUNK, taps); ++t) {
            const double mean = totals[t] / den;
            s = s + (params->subtract_min ? mean - b : mean);
        }
        S = S + s;
    }
    const bool scale = params->normalize && S > 0.0 && fuse_finite(S);
    for (int64_t t = 0; t < taps; ++t) {
        const double mean = totals[t] / den;
        const double v = params->subtract_min ? mean - b : mean;
        psf[t] = scale ? (float)(v / S) : (float)v;
    }
    result->minimum = b;
    result->sum = S;
    if (params->normalize && !scale) result->flags |= MVSIM_PSF_FLAT;
    return MVSIM_OK;
}

int mvsim_psf_geometry(int64_t out[4])
{
    MVSIM_CHECK_ARG(out != nullptr, "null pointer");
    out[0] = PSF_CHUNK; out[1] = PSF_TAPS; out[2] = PSF_SELECT_TILE; out[3] = PSF_MAX_BLOCKS;
    return MVSIM_OK;
}

int mvsim_psf_select_dev(mvsim_ctx* ctx, const void* pos_dev, int64_t stride, const int64_t* n_dev, int64_t capacity,
                         const unsigned char* use_dev_or_null, const double* m_or_null, const double* m_dev_or_null, const int64_t dim[3],
                         const mvsim_psf_params* params, unsigned char* status_dev, mvsim_psf_result* result_dev)
{
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(check_image_dim(dim));
    MVSIM_TRY(check_list(pos_dev, stride, n_dev, capacity));
    MVSIM_CHECK_ARG(status_dev && result_dev, "psf: null pointer");
    MVSIM_CHECK_ARG(!(m_or_null && m_dev_or_null), "psf: m and m_dev exclude each other");
    MVSIM_TRY(set_device(ctx));
    return launch_psf_select(ctx->stream, list_of(pos_dev, stride, n_dev, capacity), use_dev_or_null, matrix_of(m_or_null, m_dev_or_null),
                             job_of(dim, *params), status_dev, result_dev);
}

int mvsim_psf_gather_dev(mvsim_ctx* ctx, const void* img_dev, const int64_t dim[3], const void* pos_dev, int64_t stride,
                         const int64_t* n_dev, int64_t capacity, const unsigned char* status_dev, const double* m_or_null,
                         const double* m_dev_or_null, const mvsim_psf_params* params, double* totals_dev)
{
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(check_image_dim(dim));
    MVSIM_TRY(check_list(pos_dev, stride, n_dev, capacity));
    MVSIM_CHECK_ARG(img_dev && status_dev && totals_dev, "psf: null pointer");
    MVSIM_CHECK_ARG(!(m_or_null && m_dev_or_null), "psf: m and m_dev exclude each other");
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(reserve_gather(ctx, capacity, taps_of(*params), false));
    return launch_psf_gather(ctx->stream, img_dev, list_of(pos_dev, stride, n_dev, capacity), status_dev, matrix_of(m_or_null, m_dev_or_null),
                             job_of(dim, *params), ctx->psfx_buf[0].as<double>(), totals_dev);
}

int mvsim_psf_finish_dev(mvsim_ctx* ctx, const double* totals_dev, const mvsim_psf_params* params, float* psf_dev,
                         mvsim_psf_result* result_dev)
{
    MVSIM_TRY(check_params(params));
    MVSIM_CHECK_ARG(totals_dev && psf_dev && result_dev, "psf: null pointer");
    MVSIM_TRY(set_device(ctx));
    return launch_psf_finish(ctx->stream, totals_dev, job_of(nullptr, *params), psf_dev, result_dev);
}

int mvsim_psf_use_from_matches_dev(mvsim_ctx* ctx, const mvsim_match* candidates_dev, const int64_t* n_candidates_dev, int64_t capacity,
                                   const unsigned char* mask_dev_or_null, int side, int64_t n_points_capacity, unsigned char* use_dev)
{
    MVSIM_CHECK_ARG(candidates_dev && n_candidates_dev && use_dev, "psf_use_from_matches: null pointer");
    MVSIM_CHECK_ARG(capacity >= 1 && capacity <= MVSIM_PSF_MAX_POINTS, "psf_use_from_matches: capacity must be in [1, MVSIM_PSF_MAX_POINTS]");
    MVSIM_CHECK_ARG(n_points_capacity >= 1 && n_points_capacity <= MVSIM_PSF_MAX_POINTS,
                    "psf_use_from_matches: n_points_capacity must be in [1, MVSIM_PSF_MAX_POINTS]");
    MVSIM_CHECK_ARG(side == 0 || side == 1, "psf_use_from_matches: side must be 0 or 1");
    MVSIM_TRY(set_device(ctx));
    return launch_psf_use_from_matches(ctx->stream, candidates_dev, reinterpret_cast<const long long*>(n_candidates_dev), capacity,
                                       mask_dev_or_null, side, n_points_capacity, use_dev);
}

int mvsim_extract_psf_dev(mvsim_ctx* ctx, const void* img_dev, const int64_t dim[3], const void* pos_dev, int64_t stride,
                          const int64_t* n_dev, int64_t capacity, const unsigned char* use_dev_or_null, const double* m_or_null,
                          const double* m_dev_or_null, const mvsim_psf_params* params, float* psf_dev, mvsim_psf_result* result_dev,
                          unsigned char* status_dev_or_null)
{
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(check_image_dim(dim));
    MVSIM_TRY(check_list(pos_dev, stride, n_dev, capacity));
    MVSIM_CHECK_ARG(img_dev && psf_dev && result_dev, "psf: null pointer");
    MVSIM_CHECK_ARG(!(m_or_null && m_dev_or_null), "psf: m and m_dev exclude each other");
    const int64_t taps = taps_of(*params);
    MVSIM_CHECK_ARG(!overlaps(psf_dev, (size_t)taps * sizeof(float), img_dev, (size_t)nvox(dim) * (params->src_type == MVSIM_SRC_U16 ? 2 : 4)),
                    "psf: psf_dev overlaps the image");
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(reserve_gather(ctx, capacity, taps, true));
    unsigned char* status = status_dev_or_null;
    if (!status) {
        MVSIM_TRY(ctx->psfx_buf[2].reserve((size_t)capacity));
        status = ctx->psfx_buf[2].as<unsigned char>();
    }
    const PsfList L = list_of(pos_dev, stride, n_dev, capacity);
    const PsfMatrix M = matrix_of(m_or_null, m_dev_or_null);
    const PsfJob job = job_of(dim, *params);
    double* totals = ctx->psfx_buf[1].as<double>();
    MVSIM_TRY(launch_psf_select(ctx->stream, L, use_dev_or_null, M, job, status, result_dev));
    MVSIM_TRY(launch_psf_gather(ctx->stream, img_dev, L, status, M, job, ctx->psfx_buf[0].as<double>(), totals));
    return launch_psf_finish(ctx->stream, totals, job, psf_dev, result_dev);
}

int mvsim_extract_psf(mvsim_ctx* ctx, const void* img, const int64_t dim[3], const void* pos, int64_t stride, int64_t n,
                      const unsigned char* use_or_null, const double* m_or_null, const mvsim_psf_params* params, float* psf,
                      mvsim_psf_result* result, unsigned char* status_or_null)
{
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(check_image_dim(dim));
    MVSIM_CHECK_ARG(img && psf && result && (n == 0 || pos), "psf: null pointer");
    MVSIM_CHECK_ARG(stride >= 24 && stride % 8 == 0, "psf: stride must be >= 24 and a multiple of 8");
    MVSIM_CHECK_ARG(n >= 0 && n <= MVSIM_PSF_MAX_POINTS, "psf: n must be in [0, MVSIM_PSF_MAX_POINTS]");
    const int64_t taps = taps_of(*params);
    const size_t img_bytes = (size_t)nvox(dim) * (params->src_type == MVSIM_SRC_U16 ? 2 : 4);
    MVSIM_CHECK_ARG(!overlaps(psf, (size_t)taps * sizeof(float), img, img_bytes), "psf: psf overlaps the image");
    MVSIM_TRY(set_device(ctx));
    const int64_t capacity = std::max<int64_t>(n, 1);
    const size_t pos_bytes = n > 0 ? (size_t)((n - 1) * stride + 24) : 0;
    // one device block for everything but the image: [positions][n][record][use][status], each part 8-aligned
    const size_t o_n = (size_t)capacity * (size_t)stride, o_rec = o_n + 8, o_use = o_rec + sizeof(mvsim_psf_result);
    const size_t o_status = o_use + (((size_t)capacity + 7) & ~(size_t)7), block_bytes = o_status + (size_t)capacity;
    DevBuf image, block, out;
    int rc = up(ctx, image, static_cast<const float*>(img), img_bytes);
    if (rc == MVSIM_OK) rc = block.reserve(block_bytes);
    if (rc == MVSIM_OK) rc = out.reserve((size_t)taps * sizeof(float));
    char* base = block.as<char>();
    auto copy_up = [&](size_t at, const void* h, size_t bytes) {
        if (rc != MVSIM_OK || bytes == 0) return;
        if (hipMemcpyAsync(base + at, h, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { set_error("psf: upload failed"); rc = MVSIM_EHIP; }
    };
    const int64_t n_host = n;
    copy_up(0, pos, pos_bytes);
    copy_up(o_n, &n_host, sizeof(n_host));
    if (use_or_null) copy_up(o_use, use_or_null, (size_t)n);
    if (rc == MVSIM_OK)
        rc = mvsim_extract_psf_dev(ctx, image.p, dim, base, stride, reinterpret_cast<const int64_t*>(base + o_n), capacity,
                                   use_or_null ? reinterpret_cast<const unsigned char*>(base + o_use) : nullptr, m_or_null, nullptr, params,
                                   out.as<float>(), reinterpret_cast<mvsim_psf_result*>(base + o_rec),
                                   reinterpret_cast<unsigned char*>(base + o_status));
    if (rc == MVSIM_OK) rc = down(ctx, psf, out.p, (size_t)taps * sizeof(float));
    if (rc == MVSIM_OK) rc = down(ctx, reinterpret_cast<float*>(result), base + o_rec, sizeof(mvsim_psf_result));
    if (rc == MVSIM_OK && status_or_null && n > 0 && !(result->flags & MVSIM_PSF_SINGULAR))
        rc = down(ctx, reinterpret_cast<float*>(status_or_null), base + o_status, (size_t)n);
    (void)hipStreamSynchronize(ctx->stream);
    for (DevBuf* b : {&image, &block, &out}) b->release();
    return rc;
}

}  // extern "C"
