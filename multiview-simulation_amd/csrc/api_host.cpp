// C ABI of libmvsim, part 3: every entry point that takes and returns HOST buffers (the JNI boundary) -- the stage wrappers,
// mvsim_simulate_view, the pipelined path (mvsim_simulate_view_async / mvsim_wait), mvsim_simulate_views and the *_zslabs forms.
#include "api_internal.h"

using namespace mvsim;

// ---- the 16-bit acquisition transfer (CountsStaging, common.h) -----------------------------------------------------------------
int CountsStaging::reserve(const long long* counts, int views)
{
    count.assign(counts, counts + views);
    packed.assign((size_t)views, 0);
    body.assign((size_t)views + 1, 0);
    for (int v = 0; v < views; ++v) body[(size_t)v + 1] = body[(size_t)v] + (((size_t)counts[v] * sizeof(unsigned short) + 255) & ~(size_t)255);
    const size_t need = body[(size_t)views] + (((size_t)views * sizeof(unsigned int) + 255) & ~(size_t)255);
    MVSIM_TRY(dev.reserve(need));
    if (host_bytes < need) {
        if (host) { (void)hipHostFree(host); host = nullptr; host_bytes = 0; }
        MVSIM_HIP(hipHostMalloc(&host, need, hipHostMallocDefault));
        host_bytes = need;
    }
    return MVSIM_OK;
}

int CountsStaging::pack(hipStream_t s, int view, const float* src)
{
    unsigned int* flags = reinterpret_cast<unsigned int*>(dev.as<char>() + body.back());
    if (std::find(packed.begin(), packed.end(), 1) == packed.end()) MVSIM_HIP(hipMemsetAsync(flags, 0, count.size() * sizeof(unsigned int), s));
    packed[(size_t)view] = 1;
    return launch_pack_u16(s, src, reinterpret_cast<unsigned short*>(dev.as<char>() + body[(size_t)view]), count[(size_t)view], flags + view);
}

int CountsStaging::fetch(hipStream_t s)
{
    MVSIM_HIP(hipMemcpyAsync(host, dev.p, body.back() + count.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    return MVSIM_OK;
}

int CountsStaging::land(mvsim_ctx* ctx, const float* const* src_dev, float* const* dst_host)
{
    const char* h = reinterpret_cast<const char*>(host);
    std::vector<WidenJob> arrays;
    for (size_t v = 0; v < packed.size(); ++v) {
        if (!packed[v]) continue;
        packed[v] = 0;
        ctx->u16_views += 1;
        if (reinterpret_cast<const unsigned int*>(h + body.back())[v] != 0u) {      // a value beyond 65 535, or no integer: float32 after all
            ctx->u16_fallbacks += 1;
            MVSIM_HIP(hipMemcpy(dst_host[v], src_dev[v], (size_t)count[v] * sizeof(float), hipMemcpyDeviceToHost));
            continue;
        }
        arrays.push_back(WidenJob{reinterpret_cast<const unsigned short*>(h + body[v]), dst_host[v], count[v]});
    }
    widen_u16_chunked(arrays, host_threads_of(ctx));
    return MVSIM_OK;
}

void CountsStaging::release()
{
    dev.release();
    if (host) (void)hipHostFree(host);
    host = nullptr; host_bytes = 0;
    packed.clear();
}

// ---- host buffer <-> workspace ------------------------------------------------------------------------------------------------
int mvsim::up(mvsim_ctx* ctx, DevBuf& b, const float* h, size_t bytes)
{
    MVSIM_TRY(b.reserve(bytes));
    MVSIM_HIP(hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return MVSIM_OK;
}
int mvsim::down(mvsim_ctx* ctx, float* h, const void* d, size_t bytes)
{
    MVSIM_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

// Download of an acquisition that holds Poisson COUNTS (sampled: snr >= 0) through the 16-bit transfer.  Synchronous, like down().
// Small outputs are not worth the extra launch.
static int down_counts(mvsim_ctx* ctx, float* h, const float* d, int64_t n, bool sampled)
{
    if (!sampled || ctx->opt.acq_u16 == 0 || n < ((int64_t)1 << 20) || (reinterpret_cast<uintptr_t>(d) & 15) != 0)
        return down(ctx, h, d, (size_t)n * sizeof(float));
    CountsStaging& st = ctx->sync_counts;
    const long long count = n;
    MVSIM_TRY(st.reserve(&count, 1));
    MVSIM_TRY(st.pack(ctx->stream, 0, d));
    MVSIM_TRY(st.fetch(ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return st.land(ctx, &d, &h);
}

// ---- pipelined host-buffer views: the slots ---------------------------------------------------------------
static int async_setup(mvsim_ctx* ctx)
{
    if (ctx->async_ready) return MVSIM_OK;
    MVSIM_HIP(hipStreamCreateWithFlags(&ctx->h2d_stream, hipStreamNonBlocking));
    MVSIM_HIP(hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking));
    for (int s = 0; s < mvsim_ctx::ASYNC_SLOTS; ++s) {
        MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_h2d[s], hipEventDisableTiming));
        MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_compute[s], hipEventDisableTiming));
        MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_d2h[s], hipEventDisableTiming));
    }
    MVSIM_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->async_corr), mvsim_ctx::ASYNC_SLOTS * sizeof(double), hipHostMallocDefault));
    ctx->async_ready = true;
    return MVSIM_OK;
}

// The slot's view has landed: its download is through, its adjustImage factor is kept for mvsim_wait, and 16-bit counts become the
// caller's float32 acquisition (or the float32 buffer is fetched after all).  Nothing to do for a slot that has no view in flight.
static int async_collect(mvsim_ctx* ctx, int s)
{
    if (!ctx->async_inflight[s]) return MVSIM_OK;
    MVSIM_HIP(hipEventSynchronize(ctx->ev_d2h[s]));
    ctx->async_inflight[s] = false;
    ctx->async_corr_done[ctx->async_ticket[s] % mvsim_ctx::ASYNC_HISTORY] = ctx->async_corr[s];
    const float* src = ctx->async_acq[s].as<float>();
    return ctx->async_counts[s].land(ctx, &src, &ctx->async_out_acq[s]);
}

void mvsim::async_release(mvsim_ctx* ctx)
{
    if (!ctx->async_ready) return;
    (void)hipStreamSynchronize(ctx->h2d_stream);
    (void)hipStreamSynchronize(ctx->d2h_stream);
    for (int s = 0; s < mvsim_ctx::ASYNC_SLOTS; ++s) {
        (void)async_collect(ctx, s);                          // views nobody waited for still owe their caller the widened counts
        (void)hipEventDestroy(ctx->ev_h2d[s]); (void)hipEventDestroy(ctx->ev_compute[s]); (void)hipEventDestroy(ctx->ev_d2h[s]);
        ctx->async_gt[s].release(); ctx->async_acq[s].release(); ctx->async_counts[s].release();
        ctx->async_inflight[s] = false; ctx->async_gt_src[s] = nullptr;
    }
    (void)hipStreamDestroy(ctx->h2d_stream);
    (void)hipStreamDestroy(ctx->d2h_stream);
    (void)hipHostFree(ctx->async_corr);
    ctx->async_corr = nullptr;
    ctx->async_ready = false;
}

extern "C" {

int mvsim_rotate_around_axis(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int axis, int degrees, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out, "null buffer");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, in, bytes));
    MVSIM_TRY(ctx->vol_b.reserve(bytes));
    MVSIM_TRY(mvsim_rotate_around_axis_dev(ctx, ctx->vol_a.as<float>(), dim, axis, degrees, ctx->vol_b.as<float>()));
    return down(ctx, out, ctx->vol_b.p, bytes);
}

int mvsim_attenuate3d(mvsim_ctx* ctx, const float* in, const int64_t dim[3], double delta, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out, "null buffer");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, in, bytes));
    MVSIM_TRY(ctx->vol_b.reserve(bytes));
    MVSIM_TRY(mvsim_attenuate3d_dev(ctx, ctx->vol_a.as<float>(), dim, delta, ctx->vol_b.as<float>()));
    return down(ctx, out, ctx->vol_b.p, bytes);
}

int mvsim_norm_image(mvsim_ctx* ctx, float* img, int64_t n)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(img && n >= 1, "null buffer or empty image");
    const size_t bytes = (size_t)n * sizeof(float);
    double *partial, *scal;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(launch_sum(ctx->stream, ctx->vol_a.as<float>(), n, partial, scal));
    MVSIM_TRY(launch_norm_apply(ctx->stream, ctx->vol_a.as<float>(), n, scal));
    return down(ctx, img, ctx->vol_a.p, bytes);
}

int mvsim_convolve(mvsim_ctx* ctx, const float* img, const int64_t dim[3], float* psf, const int64_t kdim[3],
                   int method, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(img && out, "null buffer");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(ctx->vol_b.reserve(bytes));
    MVSIM_TRY(mvsim_convolve_dev(ctx, ctx->vol_a.as<float>(), dim, psf, kdim, method, ctx->vol_b.as<float>()));
    return down(ctx, out, ctx->vol_b.p, bytes);
}

int mvsim_adjust_image(mvsim_ctx* ctx, float* img, int64_t n, float min_value, float target_average, double* correction)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(img && n >= 1, "null buffer or empty image");
    const size_t bytes = (size_t)n * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(mvsim_adjust_image_dev(ctx, ctx->vol_a.as<float>(), n, min_value, target_average, correction));
    return down(ctx, img, ctx->vol_a.p, bytes);
}

int mvsim_extract_slices(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float snr, uint64_t seed,
                         uint32_t stream, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out, "null buffer");
    MVSIM_CHECK_ARG(inc >= 1, "inc must be >= 1");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    const size_t obytes = (size_t)(dim[0] * dim[1] * mvsim_extract_nz(dim[2], inc)) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, in, bytes));
    MVSIM_TRY(ctx->out_buf.reserve(obytes));
    MVSIM_TRY(mvsim_extract_slices_dev(ctx, ctx->vol_a.as<float>(), dim, inc, snr, seed, stream, ctx->out_buf.as<float>()));
    return down_counts(ctx, out, ctx->out_buf.as<float>(), (int64_t)(obytes / sizeof(float)), snr >= 0.0f);
}

// Volumes on the DEVICE, tiles on the HOST: the tiles are staged side by side in the context's output workspace; the sampled ones of 2^20
// values and more cross PCIe as 16-bit counts in ONE transfer (down_counts' staging and its float32 fallback), the others as they are.
int mvsim_extract_intervals(mvsim_ctx* ctx, const mvsim_interval_job* jobs, int n, float* const* out_host)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(out_host != nullptr, "interval jobs: null pointer");
    std::vector<IntervalGeom> geoms;
    MVSIM_TRY(interval_jobs_check(jobs, n, &geoms));
    std::vector<size_t> off((size_t)n + 1, 0);
    for (int j = 0; j < n; ++j) {
        MVSIM_CHECK_ARG(out_host[j] != nullptr, "interval jobs: null output");
        off[(size_t)j + 1] = off[(size_t)j] + (((size_t)geoms[(size_t)j].n_out() * sizeof(float) + 255) & ~(size_t)255);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out_host[j]), o1 = o0 + (uintptr_t)geoms[(size_t)j].n_out() * sizeof(float);
        for (int w = 0; w < j; ++w) {
            const uintptr_t p0 = reinterpret_cast<uintptr_t>(out_host[w]), p1 = p0 + (uintptr_t)geoms[(size_t)w].n_out() * sizeof(float);
            MVSIM_CHECK_ARG(!(o0 < p1 && p0 < o1), "interval jobs: outputs overlap each other");
        }
    }
    MVSIM_TRY(ctx->out_buf.reserve(off[(size_t)n]));
    std::vector<float*> dev((size_t)n);
    for (int j = 0; j < n; ++j) dev[(size_t)j] = reinterpret_cast<float*>(ctx->out_buf.as<char>() + off[(size_t)j]);
    MVSIM_TRY(extract_intervals_enqueue(ctx, jobs, geoms, dev.data()));
    std::vector<long long> counts;                    // the outputs that cross as 16-bit counts, and where they come from / go to
    std::vector<const float*> src16;
    std::vector<float*> dst16;
    for (int j = 0; j < n; ++j) {
        const long long c = geoms[(size_t)j].n_out();
        if (jobs[j].snr >= 0.0f && ctx->opt.acq_u16 != 0 && c >= (1ll << 20)) {
            counts.push_back(c); src16.push_back(dev[(size_t)j]); dst16.push_back(out_host[j]);
        } else {
            MVSIM_HIP(hipMemcpyAsync(out_host[j], dev[(size_t)j], (size_t)c * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    SyncOnExit sync{ctx};                             // the host outputs are the caller's again on every path
    if (counts.empty()) { MVSIM_HIP(hipStreamSynchronize(ctx->stream)); return MVSIM_OK; }
    CountsStaging& st = ctx->sync_counts;
    MVSIM_TRY(st.reserve(counts.data(), (int)counts.size()));
    for (size_t v = 0; v < counts.size(); ++v) MVSIM_TRY(st.pack(ctx->stream, (int)v, src16[v]));
    MVSIM_TRY(st.fetch(ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return st.land(ctx, src16.data(), dst16.data());
}

int mvsim_poisson_process(mvsim_ctx* ctx, float* img, int64_t n, double snr, uint64_t seed, uint32_t stream,
                          uint64_t index_offset)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(img && n >= 1, "null buffer or empty image");
    const size_t bytes = (size_t)n * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(ctx->out_buf.reserve(bytes));
    const int64_t dim[3] = {n, 1, 1};
    ExtractGeom g = ExtractGeom::strided(dim, 1);
    g.index_offset = index_offset;
    ExtractOps ops;
    ops.in = ctx->vol_a.as<float>(); ops.out = ctx->out_buf.as<float>();
    ops.noise = true; ops.mul = mvsim_poisson_mul(snr); ops.seed = seed; ops.stream = stream;
    MVSIM_TRY(extract_stage(ctx, g, ops));
    return down_counts(ctx, img, ctx->out_buf.as<float>(), n, true);
}

int mvsim_make_isotropic(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out, "null buffer");
    MVSIM_CHECK_ARG(inc >= 1, "inc must be >= 1");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    const size_t obytes = (size_t)(dim[0] * dim[1] * mvsim_isotropic_nz(dim[2], inc)) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, in, bytes));
    MVSIM_TRY(ctx->out_buf.reserve(obytes));
    MVSIM_TRY(mvsim_make_isotropic_dev(ctx, ctx->vol_a.as<float>(), dim, inc, ctx->out_buf.as<float>()));
    return down(ctx, out, ctx->out_buf.p, obytes);
}

int mvsim_compute_weight_image(mvsim_ctx* ctx, const int64_t dim[3], float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(out, "null buffer");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(ctx->vol_a.reserve(bytes));
    MVSIM_TRY(mvsim_compute_weight_image_dev(ctx, dim, ctx->vol_a.as<float>()));
    return down(ctx, out, ctx->vol_a.p, bytes);
}

int mvsim_simulate_view(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* psf_host, const int64_t kdim[3],
                        const mvsim_view_params* p, const mvsim_view_outputs* o, double* correction)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(gt && p && o && o->acq, "null pointer (outputs.acq is required)");
    MVSIM_CHECK_ARG(p->inc >= 1, "inc must be >= 1");
    const int64_t n = nvox(dim);
    const size_t vbytes = (size_t)n * sizeof(float);
    const size_t obytes = (size_t)(dim[0] * dim[1] * mvsim_extract_nz(dim[2], p->inc)) * sizeof(float);
    // ground truth goes to its own buffer; requested intermediates get device twins (kept by the context: a driver
    // that calls this once per view must not pay a 0.5 GB hipMalloc/hipFree pair per buffer and call)
    DevBuf &gt_d = ctx->host_gt, &rot_d = ctx->host_rot, &att_d = ctx->host_att, &con_d = ctx->host_con;
    int rc = up(ctx, gt_d, gt, vbytes);
    mvsim_view_outputs dev = {nullptr, nullptr, nullptr, nullptr};
    if (rc == MVSIM_OK && o->rot) { rc = rot_d.reserve(vbytes); dev.rot = rot_d.as<float>(); }
    if (rc == MVSIM_OK && o->att) { rc = att_d.reserve(vbytes); dev.att = att_d.as<float>(); }
    if (rc == MVSIM_OK && o->con) { rc = con_d.reserve(vbytes); dev.con = con_d.as<float>(); }
    if (rc == MVSIM_OK) rc = ctx->out_buf.reserve(obytes);
    dev.acq = ctx->out_buf.as<float>();
    if (rc == MVSIM_OK) rc = mvsim_simulate_view_dev(ctx, gt_d.as<float>(), dim, psf_host, kdim, p, &dev, correction);
    if (rc == MVSIM_OK) rc = join_tail(ctx);                // the copies below read what the tail writes
    if (rc == MVSIM_OK && o->rot) rc = down(ctx, o->rot, dev.rot, vbytes);
    if (rc == MVSIM_OK && o->att) rc = down(ctx, o->att, dev.att, vbytes);
    if (rc == MVSIM_OK && o->con) rc = down(ctx, o->con, dev.con, vbytes);
    if (rc == MVSIM_OK) rc = down_counts(ctx, o->acq, dev.acq, (int64_t)(obytes / sizeof(float)), p->snr >= 0.0f);
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int mvsim_simulate_view_async(mvsim_ctx* ctx, const float* gt, uint64_t gt_generation, const int64_t dim[3], float* psf_host,
                              const int64_t kdim[3], const mvsim_view_params* p, const mvsim_view_outputs* o, int64_t* ticket)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(gt && p && o && o->acq && ticket, "null pointer (outputs.acq and ticket are required)");
    MVSIM_CHECK_ARG(p->inc >= 1, "inc must be >= 1");
    MVSIM_TRY(async_setup(ctx));
    const int64_t n = nvox(dim);
    const size_t vbytes = (size_t)n * sizeof(float);
    const size_t obytes = (size_t)(dim[0] * dim[1] * mvsim_extract_nz(dim[2], p->inc)) * sizeof(float);
    const long long k = ctx->async_next;
    const int s = (int)(k % mvsim_ctx::ASYNC_SLOTS);
    // the staging set is free once its previous view has landed on the host
    MVSIM_TRY(async_collect(ctx, s));
    const bool wants_twins = o->rot || o->att || o->con;
    // counts as uint16 over PCIe: sampled views only (a view without noise holds reals), 16-byte rows for the packer
    const long long n_out = (long long)(obytes / sizeof(float));
    const bool as_u16 = ctx->opt.acq_u16 != 0 && p->snr >= 0.0f;
    CountsStaging& counts = ctx->async_counts[s];
    MVSIM_TRY(counts.reserve(&n_out, as_u16 ? 1 : 0));        // (no view: mvsim_wait finds nothing to widen)
    mvsim_view_outputs dev = {nullptr, nullptr, nullptr, nullptr};
    {
        // the staging buffer may move when a later view is larger: what it held is gone then, whatever the caller's pointer
        // and generation say; a view of another size never matches the cached upload either
        const void* before = ctx->async_gt[s].p;
        MVSIM_TRY(ctx->async_gt[s].reserve(vbytes));
        if (ctx->async_gt[s].p != before || ctx->async_gt_bytes[s] != vbytes) ctx->async_gt_src[s] = nullptr;
    }
    MVSIM_TRY(ctx->async_acq[s].reserve(obytes));
    if (o->rot) { MVSIM_TRY(ctx->host_rot.reserve(vbytes)); dev.rot = ctx->host_rot.as<float>(); }
    if (o->att) { MVSIM_TRY(ctx->host_att.reserve(vbytes)); dev.att = ctx->host_att.as<float>(); }
    if (o->con) { MVSIM_TRY(ctx->host_con.reserve(vbytes)); dev.con = ctx->host_con.as<float>(); }
    dev.acq = ctx->async_acq[s].as<float>();
    // upload: only when this staging set does not hold this ground truth already; the copy must not overtake the
    // view that last read the set (ev_compute)
    if (ctx->async_gt_src[s] != gt || ctx->async_gt_gen[s] != gt_generation) {
        if (k >= mvsim_ctx::ASYNC_SLOTS) MVSIM_HIP(hipStreamWaitEvent(ctx->h2d_stream, ctx->ev_compute[s], 0));
        MVSIM_HIP(hipMemcpyAsync(ctx->async_gt[s].p, gt, vbytes, hipMemcpyHostToDevice, ctx->h2d_stream));
        MVSIM_HIP(hipEventRecord(ctx->ev_h2d[s], ctx->h2d_stream));
        MVSIM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_h2d[s], 0));
        ctx->async_gt_src[s] = gt;
        ctx->async_gt_gen[s] = gt_generation;
        ctx->async_gt_bytes[s] = vbytes;
    }
    // compute: the acquisition buffer of the set is free (waited for above); the single-buffered intermediates are free
    // once the neighbour's downloads are through
    if (wants_twins || ctx->async_twins_busy) {
        for (int q = 0; q < mvsim_ctx::ASYNC_SLOTS; ++q)
            if (ctx->async_inflight[q]) MVSIM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_d2h[q], 0));
    }
    int rc = mvsim_simulate_view_dev(ctx, ctx->async_gt[s].as<float>(), dim, psf_host, kdim, p, &dev, nullptr);
    if (rc == MVSIM_OK) rc = join_tail(ctx);                // the copies below read what the tail writes
    if (rc != MVSIM_OK) { ctx->async_gt_src[s] = nullptr; return rc; }
    {
        double *partial, *scal;
        MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
        MVSIM_HIP(hipMemcpyAsync(&ctx->async_corr[s], scal + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (as_u16) MVSIM_TRY(counts.pack(ctx->stream, 0, dev.acq));
    MVSIM_HIP(hipEventRecord(ctx->ev_compute[s], ctx->stream));
    // download
    MVSIM_HIP(hipStreamWaitEvent(ctx->d2h_stream, ctx->ev_compute[s], 0));
    if (o->rot) MVSIM_HIP(hipMemcpyAsync(o->rot, dev.rot, vbytes, hipMemcpyDeviceToHost, ctx->d2h_stream));
    if (o->att) MVSIM_HIP(hipMemcpyAsync(o->att, dev.att, vbytes, hipMemcpyDeviceToHost, ctx->d2h_stream));
    if (o->con) MVSIM_HIP(hipMemcpyAsync(o->con, dev.con, vbytes, hipMemcpyDeviceToHost, ctx->d2h_stream));
    if (as_u16) MVSIM_TRY(counts.fetch(ctx->d2h_stream));
    else MVSIM_HIP(hipMemcpyAsync(o->acq, dev.acq, obytes, hipMemcpyDeviceToHost, ctx->d2h_stream));
    MVSIM_HIP(hipEventRecord(ctx->ev_d2h[s], ctx->d2h_stream));
    ctx->async_out_acq[s] = o->acq;
    ctx->async_inflight[s] = true;
    ctx->async_ticket[s] = k;
    ctx->async_twins_busy = wants_twins;
    ctx->async_next = k + 1;
    *ticket = (int64_t)k;
    return MVSIM_OK;
}

int mvsim_wait(mvsim_ctx* ctx, int64_t ticket, double* correction)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(ctx->async_ready && ticket >= 0 && ticket < ctx->async_next, "no such ticket");
    MVSIM_CHECK_ARG(ticket + mvsim_ctx::ASYNC_HISTORY > ctx->async_next, "ticket too old");
    const int s = (int)(ticket % mvsim_ctx::ASYNC_SLOTS);
    if (ctx->async_ticket[s] == ticket) MVSIM_TRY(async_collect(ctx, s));
    // otherwise the view has landed already: a later call on the same staging set, or an earlier wait, saw to that
    if (correction) *correction = ctx->async_corr_done[ticket % mvsim_ctx::ASYNC_HISTORY];
    return MVSIM_OK;
}

// Host buffers in and out for the stacked / side-by-side views of mvsim_simulate_views_dev: the ground truth goes up once, the V views
// run in one call, and the acquisitions come back together -- as uint16 counts where the views are sampled (one transfer of half the
// bytes, widened by the host threads), as float32 for a view that holds a value beyond 65 535 or was simulated without noise.
int mvsim_simulate_views(mvsim_ctx* ctx, const float* gt_host, const int64_t dim[3], float* const* psf_host, const int64_t kdim[3],
                         const mvsim_view_params* params, float* const* acq_host, int n_views)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(gt_host && psf_host && kdim && params && acq_host, "null pointer");
    MVSIM_CHECK_ARG(n_views >= 0 && n_views <= MVSIM_MAX_VIEWS, "n_views must be in [0, MVSIM_MAX_VIEWS]");
    if (n_views == 0) return MVSIM_OK;
    SyncOnExit sync{ctx};
    // views of the pipelined entry point that are still in flight own the 16-bit staging this call is about to use: land them first
    if (ctx->async_ready)
        for (int q = 0; q < mvsim_ctx::ASYNC_SLOTS; ++q) MVSIM_TRY(async_collect(ctx, q));
    const int64_t n = nvox(dim), plane = dim[0] * dim[1];
    // per-view acquisition sizes (the spacing may differ from view to view), 256-byte aligned slots
    std::vector<size_t> off((size_t)n_views + 1, 0);
    std::vector<long long> cnt((size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        MVSIM_CHECK_ARG(acq_host[v] != nullptr && params[v].inc >= 1, "null acquisition buffer or inc < 1");
        cnt[(size_t)v] = plane * mvsim_extract_nz(dim[2], params[v].inc);
        off[(size_t)v + 1] = off[(size_t)v] + (((size_t)cnt[(size_t)v] * sizeof(float) + 255) & ~(size_t)255);
    }
    MVSIM_TRY(up(ctx, ctx->host_gt, gt_host, (size_t)n * sizeof(float)));
    MVSIM_TRY(ctx->out_buf.reserve(off[(size_t)n_views]));
    std::vector<mvsim_view_outputs> outs((size_t)n_views, mvsim_view_outputs{nullptr, nullptr, nullptr, nullptr});
    std::vector<const float*> acq_dev((size_t)n_views);
    for (int v = 0; v < n_views; ++v) acq_dev[(size_t)v] = outs[(size_t)v].acq = reinterpret_cast<float*>(ctx->out_buf.as<char>() + off[(size_t)v]);
    MVSIM_TRY(mvsim_simulate_views_dev(ctx, ctx->host_gt.as<float>(), dim, psf_host, kdim, params, outs.data(), n_views));
    MVSIM_TRY(set_device(ctx));
    // pack the sampled views, fetch everything that was packed in ONE transfer (+ the flags), widen; float32 for the rest.
    // The synchronous staging (down_counts' own): mvsim_destroy / mvsim_release_caches free it whether or not the pipelined
    // entry points ever set their slots up (the async slots leaked from a context that only came through here)
    CountsStaging& counts = ctx->sync_counts;
    auto as16 = [&](int v) { return ctx->opt.acq_u16 != 0 && params[v].snr >= 0.0f; };
    bool any16 = false;
    for (int v = 0; v < n_views; ++v) any16 = any16 || as16(v);
    if (any16) {
        MVSIM_TRY(counts.reserve(cnt.data(), n_views));
        for (int v = 0; v < n_views; ++v)
            if (as16(v)) MVSIM_TRY(counts.pack(ctx->stream, v, acq_dev[(size_t)v]));
        MVSIM_TRY(counts.fetch(ctx->stream));
    }
    for (int v = 0; v < n_views; ++v)
        if (!as16(v)) MVSIM_HIP(hipMemcpyAsync(acq_host[v], acq_dev[(size_t)v], (size_t)cnt[(size_t)v] * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    if (any16) MVSIM_TRY(counts.land(ctx, acq_dev.data(), acq_host));
    return MVSIM_OK;
}

// ---- per-stage operators on host buffers given as z slabs (volumes beyond one 2 GiB direct buffer) --------------------
namespace {
struct SlabList {
    const void* const* ptr;
    const int64_t*     nz;
    int                count;
};
int check_slabs(const SlabList& l, int64_t planes, const char* what)
{
    if (!l.ptr || !l.nz || l.count < 1) { set_error("invalid argument: %s slab list is empty", what); return MVSIM_EINVAL; }
    int64_t z = 0;
    for (int i = 0; i < l.count; ++i) {
        if (!l.ptr[i] || l.nz[i] < 1) { set_error("invalid argument: %s slab %d is empty", what, i); return MVSIM_EINVAL; }
        z += l.nz[i];
    }
    if (z != planes) { set_error("invalid argument: %s slabs hold %lld planes, expected %lld", what, (long long)z, (long long)planes); return MVSIM_EINVAL; }
    return MVSIM_OK;
}
int upload_slabs(mvsim_ctx* ctx, const SlabList& l, int64_t plane, float* dev)
{
    int64_t z = 0;
    for (int i = 0; i < l.count; ++i) {
        MVSIM_HIP(hipMemcpyAsync(dev + plane * z, l.ptr[i], (size_t)(plane * l.nz[i]) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        z += l.nz[i];
    }
    return MVSIM_OK;
}
int download_slabs(mvsim_ctx* ctx, const SlabList& l, int64_t plane, const float* dev, const char* what = "")
{
    int rc = MVSIM_OK;
    int64_t z = 0;
    for (int i = 0; i < l.count && rc == MVSIM_OK; ++i) {
        if (hipMemcpyAsync(const_cast<void*>(l.ptr[i]), dev + plane * z, (size_t)(plane * l.nz[i]) * sizeof(float), hipMemcpyDeviceToHost,
                           ctx->stream) != hipSuccess) { set_error("download of %sslab %d failed", what, i); rc = MVSIM_EHIP; }
        z += l.nz[i];
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == MVSIM_OK) { set_error("stream synchronise failed"); rc = MVSIM_EHIP; }
    return rc;
}
// stage the input slabs in vol_a, make room for `out_planes` planes in vol_b
int slabs_in(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_nz, int n_in, const int64_t dim[3], float* const* out_slabs,
             const int64_t* out_nz, int n_out, int64_t out_planes, SlabList* in, SlabList* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    *in = SlabList{reinterpret_cast<const void* const*>(in_slabs), in_nz, n_in};
    *out = SlabList{reinterpret_cast<const void* const*>(out_slabs), out_nz, n_out};
    MVSIM_TRY(check_slabs(*in, dim[2], "input"));
    MVSIM_TRY(check_slabs(*out, out_planes, "output"));
    const int64_t plane = dim[0] * dim[1];
    MVSIM_TRY(ctx->vol_a.reserve((size_t)(plane * dim[2]) * sizeof(float)));
    MVSIM_TRY(ctx->vol_b.reserve((size_t)(plane * out_planes) * sizeof(float)));
    return upload_slabs(ctx, *in, plane, ctx->vol_a.as<float>());
}
}  // namespace

int mvsim_simulate_view_zslabs(mvsim_ctx* ctx, const float* const* gt_slabs, const int64_t* gt_slab_nz, int n_gt_slabs,
                               const int64_t dim[3], float* psf_host, const int64_t kdim[3], const mvsim_view_params* p,
                               float* const* acq_slabs, const int64_t* acq_slab_nz, int n_acq_slabs, double* correction)
{
    MVSIM_TRY(set_device(ctx));
    SyncOnExit sync{ctx};
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(gt_slabs && gt_slab_nz && acq_slabs && acq_slab_nz && p, "null pointer");
    MVSIM_CHECK_ARG(n_gt_slabs >= 1 && n_acq_slabs >= 1 && p->inc >= 1, "slab counts and inc must be >= 1");
    const int64_t plane = dim[0] * dim[1];
    const int64_t nzo = mvsim_extract_nz(dim[2], p->inc);
    int64_t zs = 0, za = 0;
    for (int i = 0; i < n_gt_slabs; ++i) { MVSIM_CHECK_ARG(gt_slabs[i] && gt_slab_nz[i] >= 1, "empty ground-truth slab"); zs += gt_slab_nz[i]; }
    for (int j = 0; j < n_acq_slabs; ++j) { MVSIM_CHECK_ARG(acq_slabs[j] && acq_slab_nz[j] >= 1, "empty acquisition slab"); za += acq_slab_nz[j]; }
    MVSIM_CHECK_ARG(zs == dim[2], "ground-truth slabs must add up to dim[2] planes");
    MVSIM_CHECK_ARG(za == nzo, "acquisition slabs must add up to mvsim_extract_nz(dim[2], inc) planes");
    MVSIM_TRY(ctx->host_gt.reserve((size_t)(plane * dim[2]) * sizeof(float)));
    MVSIM_TRY(ctx->out_buf.reserve((size_t)(plane * nzo) * sizeof(float)));
    MVSIM_TRY(upload_slabs(ctx, SlabList{reinterpret_cast<const void* const*>(gt_slabs), gt_slab_nz, n_gt_slabs}, plane, ctx->host_gt.as<float>()));
    mvsim_view_outputs dev = {nullptr, nullptr, nullptr, ctx->out_buf.as<float>()};
    MVSIM_TRY(mvsim_simulate_view_dev(ctx, ctx->host_gt.as<float>(), dim, psf_host, kdim, p, &dev, correction));
    MVSIM_TRY(join_tail(ctx));                              // the copies below read what the tail writes
    return download_slabs(ctx, SlabList{reinterpret_cast<const void* const*>(acq_slabs), acq_slab_nz, n_acq_slabs}, plane, dev.acq, "acquisition ");
}

int mvsim_rotate_around_axis_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                                    int axis, int degrees, float* const* out_slabs, const int64_t* out_slab_nz, int n_out)
{
    SlabList in, out;
    SyncOnExit sync{ctx};
    MVSIM_TRY(slabs_in(ctx, in_slabs, in_slab_nz, n_in, dim, out_slabs, out_slab_nz, n_out, dim ? dim[2] : 0, &in, &out));
    MVSIM_TRY(mvsim_rotate_around_axis_dev(ctx, ctx->vol_a.as<float>(), dim, axis, degrees, ctx->vol_b.as<float>()));
    return download_slabs(ctx, out, dim[0] * dim[1], ctx->vol_b.as<float>());
}

int mvsim_attenuate3d_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                             double delta, float* const* out_slabs, const int64_t* out_slab_nz, int n_out)
{
    SlabList in, out;
    SyncOnExit sync{ctx};
    MVSIM_TRY(slabs_in(ctx, in_slabs, in_slab_nz, n_in, dim, out_slabs, out_slab_nz, n_out, dim ? dim[2] : 0, &in, &out));
    MVSIM_TRY(mvsim_attenuate3d_dev(ctx, ctx->vol_a.as<float>(), dim, delta, ctx->vol_b.as<float>()));
    return download_slabs(ctx, out, dim[0] * dim[1], ctx->vol_b.as<float>());
}

int mvsim_convolve_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                          float* psf, const int64_t kdim[3], int method, float* const* out_slabs, const int64_t* out_slab_nz, int n_out)
{
    SlabList in, out;
    SyncOnExit sync{ctx};
    MVSIM_TRY(slabs_in(ctx, in_slabs, in_slab_nz, n_in, dim, out_slabs, out_slab_nz, n_out, dim ? dim[2] : 0, &in, &out));
    MVSIM_TRY(mvsim_convolve_dev(ctx, ctx->vol_a.as<float>(), dim, psf, kdim, method, ctx->vol_b.as<float>()));
    return download_slabs(ctx, out, dim[0] * dim[1], ctx->vol_b.as<float>());
}

int mvsim_extract_slices_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                                int inc, float snr, uint64_t seed, uint32_t stream, float* const* out_slabs, const int64_t* out_slab_nz,
                                int n_out)
{
    MVSIM_CHECK_ARG(inc >= 1, "inc must be >= 1");
    SlabList in, out;
    SyncOnExit sync{ctx};
    MVSIM_TRY(slabs_in(ctx, in_slabs, in_slab_nz, n_in, dim, out_slabs, out_slab_nz, n_out, dim ? mvsim_extract_nz(dim[2], inc) : 0, &in, &out));
    MVSIM_TRY(mvsim_extract_slices_dev(ctx, ctx->vol_a.as<float>(), dim, inc, snr, seed, stream, ctx->vol_b.as<float>()));
    MVSIM_TRY(join_tail(ctx));
    return download_slabs(ctx, out, dim[0] * dim[1], ctx->vol_b.as<float>());
}

}  // extern "C"
