// C ABI of libmvsim, part 8: the view fusion (mvsim.h states the recipe) -- every view resampled through its affine into one output
// interval, blended into one volume or handed back aligned with its weights.  Host orchestration only: the argument checks, the prepare
// launches that invert the matrices on the device, the launch of fuse.hip on the context's stream; no entry point reads anything back,
// so registration and fusion chain without a synchronisation.
// Every argument is checked before the context is touched, so each refusal can be reached without a device.
#include "api_internal.h"
#include "fuse.h"
#include "fuse_dev.h"

#include <vector>

namespace mvsim {

namespace {

size_t src_bytes(const mvsim_fuse_view& v, int src_type) { return (size_t)nvox(v.dim) * (src_type == MVSIM_SRC_U16 ? 2 : 4); }

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const char *a0 = static_cast<const char*>(a), *b0 = static_cast<const char*>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

int check_job(const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3], const mvsim_fuse_params* p,
              bool host_matrices_only)
{
    MVSIM_CHECK_ARG(views && out_min && out_dim && p, "fuse: null pointer");
    MVSIM_CHECK_ARG(n_views >= 1 && n_views <= MVSIM_MAX_VIEWS, "fuse: n_views must be in [1, MVSIM_MAX_VIEWS]");
    MVSIM_CHECK_ARG(p->src_type == MVSIM_SRC_F32 || p->src_type == MVSIM_SRC_U16, "fuse: src_type must be MVSIM_SRC_F32 or MVSIM_SRC_U16");
    for (int d = 0; d < 3; ++d) {
        MVSIM_CHECK_ARG(std::isfinite(p->blend[d]) && p->blend[d] >= 0.0, "fuse: blend must be finite and >= 0");
        MVSIM_CHECK_ARG(out_dim[d] >= 1, "fuse: out_dim entries must be >= 1");
        MVSIM_CHECK_ARG(out_dim[d] < ((int64_t)1 << 31) && out_min[d] > -((int64_t)1 << 52) && out_min[d] < ((int64_t)1 << 52),
                        "fuse: output interval too large");
    }
    MVSIM_CHECK_ARG(nvox(out_dim) < ((int64_t)1 << 40), "fuse: output interval too large");
    for (int v = 0; v < n_views; ++v) {
        MVSIM_CHECK_ARG(views[v].src != nullptr, "fuse: null source");
        for (int d = 0; d < 3; ++d) MVSIM_CHECK_ARG(views[v].dim[d] >= 1 && views[v].dim[d] < ((int64_t)1 << 31), "fuse: every extent must be >= 1");
        MVSIM_CHECK_ARG(nvox(views[v].dim) < ((int64_t)1 << 40), "fuse: view too large");
        MVSIM_CHECK_ARG(!host_matrices_only || views[v].m_dev == nullptr, "fuse: m_dev must be null with host buffers");
    }
    return MVSIM_OK;
}

int check_output(const void* out, const mvsim_fuse_view* views, int n_views, const int64_t out_dim[3], int src_type)
{
    if (!out) return MVSIM_OK;
    for (int v = 0; v < n_views; ++v)
        MVSIM_CHECK_ARG(!overlaps(out, (size_t)nvox(out_dim) * sizeof(float), views[v].src, src_bytes(views[v], src_type)),
                        "fuse: an output overlaps a source");
    return MVSIM_OK;
}

FuseJob job_of(const int64_t out_min[3], const int64_t out_dim[3], const mvsim_fuse_params& p, int n_views)
{
    FuseJob j;
    for (int d = 0; d < 3; ++d) { j.out_min[d] = out_min[d]; j.out_dim[d] = out_dim[d]; j.blend[d] = p.blend[d]; }
    j.background = p.background;
    j.src_type = p.src_type;
    j.n_views = n_views;
    return j;
}

// the prepare launches of a checked call and the fuse launch behind them
int enqueue(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
            const mvsim_fuse_params& p, float* fused, float* sum_weights, float* const* aligned, float* const* weights, int32_t* status)
{
    MVSIM_TRY(ctx->fuse_buf.reserve((size_t)MVSIM_MAX_VIEWS * sizeof(FuseViewRec)));
    FuseViewRec* recs = ctx->fuse_buf.as<FuseViewRec>();
    for (int first = 0; first < n_views; first += FUSE_PREPARE_BATCH) {
        const int n = std::min(FUSE_PREPARE_BATCH, n_views - first);
        FusePrepareArgs a;
        std::memset(&a, 0, sizeof(a));
        for (int t = 0; t < n; ++t) {
            const mvsim_fuse_view& v = views[first + t];
            FuseViewArg& o = a.v[t];
            o.src = v.src;
            for (int d = 0; d < 3; ++d) o.dim[d] = v.dim[d];
            o.m_dev = v.m_dev;
            std::memcpy(o.m, v.m, sizeof(o.m));
            o.aligned = aligned ? aligned[first + t] : nullptr;
            o.weight = weights ? weights[first + t] : nullptr;
        }
        MVSIM_TRY(launch_fuse_prepare(ctx->stream, a, first, n, recs, status));
    }
    return launch_fuse(ctx->stream, job_of(out_min, out_dim, p, n_views), recs, fused, sum_weights);
}

// the sources of a host call into device twins; dev: the views with the twins as sources
int upload_views(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, int src_type, std::vector<DevBuf>* twins,
                 std::vector<mvsim_fuse_view>* dev)
{
    twins->resize((size_t)n_views);
    dev->assign(views, views + n_views);
    for (int v = 0; v < n_views; ++v) {
        MVSIM_TRY(up(ctx, (*twins)[(size_t)v], static_cast<const float*>(views[v].src), src_bytes(views[v], src_type)));
        (*dev)[(size_t)v].src = (*twins)[(size_t)v].p;
    }
    return MVSIM_OK;
}

}  // namespace

}  // namespace mvsim

using namespace mvsim;

extern "C" {

void mvsim_fuse_params_default(mvsim_fuse_params* p)
{
    if (!p) return;
    p->blend[0] = p->blend[1] = p->blend[2] = 8.0;
    p->background = 0.0f;
    p->src_type = MVSIM_SRC_F32;
}

int mvsim_fuse_invert(const double m[12], double inv[12], int* singular)
{
    MVSIM_CHECK_ARG(m && inv && singular, "fuse_invert: null pointer");
    double out[12];
    *singular = fuse_invert(m, out) ? 0 : 1;
    if (!*singular) std::memcpy(inv, out, sizeof(out));
    return MVSIM_OK;
}

int mvsim_fusion_bounds(const double* m, const int64_t* dims, int n_views, int intersection, int64_t out_min[3], int64_t out_dim[3])
{
    MVSIM_CHECK_ARG(m && dims && out_min && out_dim, "fusion_bounds: null pointer");
    MVSIM_CHECK_ARG(n_views >= 1 && n_views <= MVSIM_MAX_VIEWS, "fusion_bounds: n_views must be in [1, MVSIM_MAX_VIEWS]");
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int v = 0; v < n_views; ++v) {
        const double* mv = m + 12 * v;
        const int64_t* N = dims + 3 * v;
        MVSIM_CHECK_ARG(N[0] >= 1 && N[1] >= 1 && N[2] >= 1, "fusion_bounds: every extent must be >= 1");
        double vlo[3], vhi[3];
        for (int c = 0; c < 8; ++c) {
            const double x = (c & 1) ? (double)(N[0] - 1) : 0.0, y = (c & 2) ? (double)(N[1] - 1) : 0.0, z = (c & 4) ? (double)(N[2] - 1) : 0.0;
            for (int r = 0; r < 3; ++r) {
                const double q = ((mv[4 * r] * x + mv[4 * r + 1] * y) + mv[4 * r + 2] * z) + mv[4 * r + 3];
                MVSIM_CHECK_ARG(std::isfinite(q) && std::fabs(q) < 4.0e15, "fusion_bounds: a corner is not finite");
                if (c == 0 || q < vlo[r]) vlo[r] = q;
                if (c == 0 || q > vhi[r]) vhi[r] = q;
            }
        }
        for (int r = 0; r < 3; ++r) {
            const double f = std::floor(vlo[r]), c = std::ceil(vhi[r]);
            if (v == 0) { lo[r] = f; hi[r] = c; }
            else if (intersection) { lo[r] = std::max(lo[r], f); hi[r] = std::min(hi[r], c); }
            else { lo[r] = std::min(lo[r], f); hi[r] = std::max(hi[r], c); }
        }
    }
    for (int r = 0; r < 3; ++r) MVSIM_CHECK_ARG(lo[r] <= hi[r], "fusion_bounds: the intersection is empty");
    for (int r = 0; r < 3; ++r) { out_min[r] = (int64_t)lo[r]; out_dim[r] = (int64_t)hi[r] - (int64_t)lo[r] + 1; }
    return MVSIM_OK;
}

int mvsim_fusion_psf_matrix(const double m[12], const int64_t kdim[3], const int64_t out_kdim[3], double out[12])
{
    MVSIM_CHECK_ARG(m && kdim && out_kdim && out, "fusion_psf_matrix: null pointer");
    for (int d = 0; d < 3; ++d) MVSIM_CHECK_ARG(kdim[d] >= 1 && out_kdim[d] >= 1, "fusion_psf_matrix: every extent must be >= 1");
    const double cx = (double)(kdim[0] / 2), cy = (double)(kdim[1] / 2), cz = (double)(kdim[2] / 2);
    double res[12];
    for (int r = 0; r < 3; ++r) {
        const double* a = m + 4 * r;
        res[4 * r] = a[0]; res[4 * r + 1] = a[1]; res[4 * r + 2] = a[2];
        res[4 * r + 3] = (double)(out_kdim[r] / 2) - ((a[0] * cx + a[1] * cy) + a[2] * cz);
    }
    std::memcpy(out, res, sizeof(res));
    return MVSIM_OK;
}

int mvsim_fusion_geometry(int64_t out[4])
{
    MVSIM_CHECK_ARG(out != nullptr, "null pointer");
    out[0] = FUSE_BX; out[1] = FUSE_BY; out[2] = FUSE_BZ; out[3] = FUSE_MAX_BLOCKS;
    return MVSIM_OK;
}

int mvsim_fuse_views_dev(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                         const mvsim_fuse_params* params, float* fused_dev, float* sum_weights_dev_or_null, int32_t* status_dev_or_null)
{
    MVSIM_TRY(check_job(views, n_views, out_min, out_dim, params, false));
    MVSIM_CHECK_ARG(fused_dev != nullptr, "fuse: null pointer");
    MVSIM_TRY(check_output(fused_dev, views, n_views, out_dim, params->src_type));
    MVSIM_TRY(check_output(sum_weights_dev_or_null, views, n_views, out_dim, params->src_type));
    MVSIM_TRY(set_device(ctx));
    return enqueue(ctx, views, n_views, out_min, out_dim, *params, fused_dev, sum_weights_dev_or_null, nullptr, nullptr, status_dev_or_null);
}

int mvsim_align_views_dev(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                          const mvsim_fuse_params* params, float* const* aligned_dev, float* const* weights_dev_or_null,
                          int32_t* status_dev_or_null)
{
    MVSIM_TRY(check_job(views, n_views, out_min, out_dim, params, false));
    MVSIM_CHECK_ARG(aligned_dev != nullptr, "fuse: null pointer");
    for (int v = 0; v < n_views; ++v) {
        MVSIM_TRY(check_output(aligned_dev[v], views, n_views, out_dim, params->src_type));
        if (weights_dev_or_null) MVSIM_TRY(check_output(weights_dev_or_null[v], views, n_views, out_dim, params->src_type));
    }
    MVSIM_TRY(set_device(ctx));
    return enqueue(ctx, views, n_views, out_min, out_dim, *params, nullptr, nullptr, aligned_dev, weights_dev_or_null, status_dev_or_null);
}

int mvsim_fuse_views(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                     const mvsim_fuse_params* params, float* fused, float* sum_weights_or_null, int32_t* status_or_null)
{
    MVSIM_TRY(check_job(views, n_views, out_min, out_dim, params, true));
    MVSIM_CHECK_ARG(fused != nullptr, "fuse: null pointer");
    MVSIM_TRY(check_output(fused, views, n_views, out_dim, params->src_type));
    MVSIM_TRY(check_output(sum_weights_or_null, views, n_views, out_dim, params->src_type));
    MVSIM_TRY(set_device(ctx));
    const size_t bytes = (size_t)nvox(out_dim) * sizeof(float), status_bytes = (size_t)n_views * sizeof(int32_t);
    std::vector<DevBuf> twins;
    std::vector<mvsim_fuse_view> dev;
    DevBuf out, sum, st;
    int rc = upload_views(ctx, views, n_views, params->src_type, &twins, &dev);
    if (rc == MVSIM_OK) rc = out.reserve(bytes);
    if (rc == MVSIM_OK && sum_weights_or_null) rc = sum.reserve(bytes);
    if (rc == MVSIM_OK && status_or_null) rc = st.reserve(status_bytes);
    if (rc == MVSIM_OK)
        rc = enqueue(ctx, dev.data(), n_views, out_min, out_dim, *params, out.as<float>(), sum.as<float>(), nullptr, nullptr, st.as<int32_t>());
    if (rc == MVSIM_OK) rc = down(ctx, fused, out.p, bytes);
    if (rc == MVSIM_OK && sum_weights_or_null) rc = down(ctx, sum_weights_or_null, sum.p, bytes);
    if (rc == MVSIM_OK && status_or_null) rc = down(ctx, reinterpret_cast<float*>(status_or_null), st.p, status_bytes);
    (void)hipStreamSynchronize(ctx->stream);
    for (DevBuf& b : twins) b.release();
    for (DevBuf* b : {&out, &sum, &st}) b->release();
    return rc;
}

int mvsim_align_views(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                      const mvsim_fuse_params* params, float* const* aligned, float* const* weights_or_null, int32_t* status_or_null)
{
    MVSIM_TRY(check_job(views, n_views, out_min, out_dim, params, true));
    MVSIM_CHECK_ARG(aligned != nullptr, "fuse: null pointer");
    for (int v = 0; v < n_views; ++v) {
        MVSIM_TRY(check_output(aligned[v], views, n_views, out_dim, params->src_type));
        if (weights_or_null) MVSIM_TRY(check_output(weights_or_null[v], views, n_views, out_dim, params->src_type));
    }
    MVSIM_TRY(set_device(ctx));
    const size_t bytes = (size_t)nvox(out_dim) * sizeof(float), status_bytes = (size_t)n_views * sizeof(int32_t);
    std::vector<DevBuf> twins, outs((size_t)2 * n_views);
    std::vector<mvsim_fuse_view> dev;
    std::vector<float*> al((size_t)n_views, nullptr), wt((size_t)n_views, nullptr);
    DevBuf st;
    int rc = upload_views(ctx, views, n_views, params->src_type, &twins, &dev);
    for (int v = 0; v < n_views && rc == MVSIM_OK; ++v) {
        if (aligned[v]) { rc = outs[(size_t)2 * v].reserve(bytes); al[(size_t)v] = outs[(size_t)2 * v].as<float>(); }
        if (rc == MVSIM_OK && weights_or_null && weights_or_null[v]) {
            rc = outs[(size_t)2 * v + 1].reserve(bytes);
            wt[(size_t)v] = outs[(size_t)2 * v + 1].as<float>();
        }
    }
    if (rc == MVSIM_OK && status_or_null) rc = st.reserve(status_bytes);
    if (rc == MVSIM_OK)
        rc = enqueue(ctx, dev.data(), n_views, out_min, out_dim, *params, nullptr, nullptr, al.data(), wt.data(), st.as<int32_t>());
    for (int v = 0; v < n_views && rc == MVSIM_OK; ++v) {
        if (al[(size_t)v]) rc = down(ctx, aligned[v], al[(size_t)v], bytes);
        if (rc == MVSIM_OK && wt[(size_t)v]) rc = down(ctx, weights_or_null[v], wt[(size_t)v], bytes);
    }
    if (rc == MVSIM_OK && status_or_null) rc = down(ctx, reinterpret_cast<float*>(status_or_null), st.p, status_bytes);
    (void)hipStreamSynchronize(ctx->stream);
    for (DevBuf& b : twins) b.release();
    for (DevBuf& b : outs) b.release();
    st.release();
    return rc;
}

}  // extern "C"
