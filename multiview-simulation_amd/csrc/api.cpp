// C ABI of libmvsim (include/mvsim.h), part 1: errors, options, context lifetime, memory, the stage operators on device buffers
// and the statistics / geometry / timing queries.  The per-view pipeline is api_view.cpp, the host-buffer entry points are
// api_host.cpp, the phantom / bead / refraction-simulator wrappers api_sims.cpp.  Host orchestration only -- every voxel of
// arithmetic happens in the HIP kernels (rotate.hip, kernels.hip, extract.hip, fftconv.hip, stencil.hip).
#include "api_internal.h"

#include <cstdlib>
#include <mutex>
#include <thread>

namespace mvsim {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- run-time switches ------------------------------------------------------------------------------
int parse_option(Options& o, const char* name, const char* value)
{
    if (!name || !value) return MVSIM_EINVAL;
    const std::string n(name), v(value);
    // the value as one of a list of words: the setting that word stands for (untouched when the word is not on the list)
    auto word = [&](std::initializer_list<std::pair<const char*, int>> words, auto* dst) {
        for (const auto& w : words)
            if (v == w.first) { *dst = w.second; return MVSIM_OK; }
        return MVSIM_EINVAL;
    };
    auto flag = [&](bool* dst) { return word({{"1", 1}, {"on", 1}, {"true", 1}, {"0", 0}, {"off", 0}, {"false", 0}}, dst); };
    // a decimal number of at most `digits` digits, lo <= k <= hi; "auto" = when_auto where the option has such a value
    auto number = [&](size_t digits, long long lo, long long hi, auto* dst, int when_auto = -1) {
        if (when_auto >= 0 && v == "auto") { *dst = when_auto; return MVSIM_OK; }
        if (v.empty() || v.size() > digits || v.find_first_not_of("0123456789") != std::string::npos) return MVSIM_EINVAL;
        const long long k = atoll(v.c_str());
        if (k < lo || k > hi) return MVSIM_EINVAL;
        *dst = k;
        return MVSIM_OK;
    };
    if (n == "fft_zpass") return word({{"auto", 0}, {"direct", 1}, {"fft", 2}, {"inline", 3}}, &o.zpass);
    if (n == "fft_backend") return word({{"custom", 0}, {"auto", 0}, {"rocfft", 1}}, &o.rocfft);
    if (n == "fused_rotate") return word({{"1", 1}, {"on", 1}, {"lds", 1}, {"0", 0}, {"off", 0}, {"2", 2}, {"lane", 2}, {"3", 3}, {"auto", 3}}, &o.fused_rotate);
    if (n == "poisson_queue") return word({{"1", 1}, {"on", 1}, {"0", 0}, {"off", 0}}, &o.poisson_queue);
    if (n == "poisson_queue_share") return number(2, 1, 16, &o.poisson_queue_share, 0);   // sixteenths of a block's voxels per queue segment
    if (n == "attenuate") return word({{"serial", 0}, {"scan", 1}}, &o.attenuate_scan);
    if (n == "early_sum") return flag(&o.early_sum);
    if (n == "zconv_strided") return flag(&o.zconv_strided);
    if (n == "exp") return number(2, 0, 15, &o.exp);                                  // A/B bits of tools/ and the tests (common.h)
    if (n == "beads_pair_cap") return number(10, 1024, 1LL << 31, &o.beads_pair_cap);  // pairs per chunk of the bead renderer
    if (n == "reject_batch") return number(7, 1, 1LL << 20, &o.reject_batch, 0);      // trials per launch of the rejection sampler
    if (n == "dog_pass") return word({{"both", 0}, {"xy", 1}, {"z", 2}}, &o.dog_pass);
    if (n == "sphere_walk") return word({{"host", 0}, {"device", 1}, {"device_only", 2}, {"auto", -1}}, &o.sphere_walk);   // who walks the large sphere's random stream
    if (n == "fuse_tail") return flag(&o.fuse_tail);
    if (n == "psf_overlap") return flag(&o.psf_overlap);
    if (n == "fused_fftx") return word({{"auto", 2}, {"1", 1}, {"on", 1}, {"0", 0}, {"off", 0}, {"roles", 3}}, &o.fused_fftx);
    if (n == "tail_overlap") return word({{"0", 0}, {"off", 0}, {"1", 1}, {"on", 1}, {"own", 1}, {"2", 2}, {"any", 2}}, &o.tail_overlap);
    if (n == "acq_transfer") return word({{"auto", 1}, {"u16", 1}, {"f32", 0}}, &o.acq_u16);
    if (n == "host_threads") return number(3, 1, 256, &o.host_threads, 0);
    if (n == "view_batch") return word({{"auto", 2}, {"1", 1}, {"on", 1}, {"0", 0}, {"off", 0}}, &o.view_batch);
    if (n == "view_lanes") return number(2, 1, MVSIM_MAX_VIEWS, &o.view_lanes, 0);
    if (n == "graph") { bool g = false; const int rc = flag(&g); o.graph = g ? 1 : 0; return rc; }
    if (n == "broadcast") {
        int how = 0;
        if (word({{"scatter_allgather", 0}, {"auto", 0}, {"ring", 1}, {"peer_copy", 2}, {"pipelined", 3}}, &how) != MVSIM_OK) return MVSIM_EINVAL;
        o.bcast_ring = how == 1; o.bcast_peer_copy = how == 2; o.bcast_pipelined = how == 3;
        return MVSIM_OK;
    }
    if (n == "skip_empty") return flag(&o.skip_empty);
    if (n == "skip_rows") return flag(&o.skip_rows);
    if (n == "skip_tail") return flag(&o.skip_tail);
    if (n == "psf_cache") return number(7, 0, 1 << 20, &o.psf_cache);                 // MiB of PSF spectra kept by content; 0: off
    if (n == "fft_pad") {
        long long a = 0, b = 0, c = 0;
        if (v == "auto" || v.empty()) { o.fft_pad[0] = o.fft_pad[1] = o.fft_pad[2] = 0; return MVSIM_OK; }
        if (sscanf(v.c_str(), "%lld,%lld,%lld", &a, &b, &c) != 3 || a < 0 || b < 0 || c < 0) return MVSIM_EINVAL;
        o.fft_pad[0] = a; o.fft_pad[1] = b; o.fft_pad[2] = c;
        return MVSIM_OK;
    }
    return MVSIM_EINVAL;
}

// Process defaults, read from the environment exactly once (MVSIM_FFT_ZPASS=fft|direct, MVSIM_FFT_BACKEND=rocfft,
// MVSIM_FFT_PAD=px,py,pz, MVSIM_NO_FUSED_ROTATE, MVSIM_POISSON_NOQUEUE, MVSIM_NO_EARLY_SUM, MVSIM_GRAPH).
const Options& env_options()
{
    static Options o;
    static std::once_flag once;
    std::call_once(once, [] {
        if (const char* e = getenv("MVSIM_FFT_ZPASS")) (void)parse_option(o, "fft_zpass", e);
        if (const char* e = getenv("MVSIM_FFT_BACKEND")) (void)parse_option(o, "fft_backend", e);
        if (const char* e = getenv("MVSIM_FFT_PAD")) (void)parse_option(o, "fft_pad", e);
        if (getenv("MVSIM_NO_FUSED_ROTATE")) o.fused_rotate = 0;
        if (getenv("MVSIM_POISSON_NOQUEUE")) o.poisson_queue = 0;
        if (getenv("MVSIM_NO_EARLY_SUM")) o.early_sum = false;
        if (getenv("MVSIM_NO_FUSE_TAIL")) o.fuse_tail = false;
        if (const char* e = getenv("MVSIM_GRAPH")) (void)parse_option(o, "graph", e);
        if (const char* e = getenv("MVSIM_BROADCAST")) (void)parse_option(o, "broadcast", e);
        // MVSIM_OPTIONS="name=value;name=value": any option by its mvsim_set_option name (experiments, A/B runs)
        if (const char* e = getenv("MVSIM_OPTIONS")) {
            std::string all(e);
            size_t pos = 0;
            while (pos < all.size()) {
                size_t end = all.find(';', pos);
                if (end == std::string::npos) end = all.size();
                const std::string kv = all.substr(pos, end - pos);
                const size_t eq = kv.find('=');
                if (eq != std::string::npos) (void)parse_option(o, kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str());
                pos = end + 1;
            }
        }
    });
    return o;
}

int ensure_lds_attr(mvsim_ctx* ctx, const void* kernel, size_t bytes)
{
    if (bytes <= 64 * 1024) return MVSIM_OK;
    if (bytes > 160 * 1024) { set_error("kernel needs %zu bytes of LDS (> 160 KiB)", bytes); return MVSIM_EINVAL; }
    if (ctx->lds_attr_set.count(kernel)) return MVSIM_OK;
    MVSIM_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ctx->lds_attr_set.insert(kernel);
    return MVSIM_OK;
}

// Bumped whenever a workspace moves or goes away: captured view graphs hold raw workspace addresses and must not be
// replayed across such a change (view_graph_launch compares the epoch it captured under).
int DevBuf::reserve(size_t need)
{
    if (need <= bytes) return MVSIM_OK;
    if (epoch) *epoch += 1;
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess) {
        p = nullptr;
        set_error("hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
        return MVSIM_ENOMEM;
    }
    bytes = need;
    return MVSIM_OK;
}

void DevBuf::release()
{
    if (p && epoch) *epoch += 1;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

int PinnedRing::acquire(size_t need, int* slot)
{
    const int i = next;
    next = (next + 1) % SLOTS;
    if (busy[i]) { MVSIM_HIP(hipEventSynchronize(ev[i])); busy[i] = false; }
    if (!ev[i]) MVSIM_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    if (bytes[i] < need) {
        if (p[i]) { (void)hipHostFree(p[i]); p[i] = nullptr; bytes[i] = 0; }
        MVSIM_HIP(hipHostMalloc(&p[i], need, hipHostMallocDefault));
        bytes[i] = need;
    }
    *slot = i;
    return MVSIM_OK;
}

void PinnedRing::release_all()
{
    for (int i = 0; i < SLOTS; ++i) {
        if (busy[i]) (void)hipEventSynchronize(ev[i]);
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (p[i]) (void)hipHostFree(p[i]);
        p[i] = nullptr; bytes[i] = 0; ev[i] = nullptr; busy[i] = false;
    }
}

// ---- affine model (mpicbg AffineModel3D semantics; SimulateMultiViewDataset.java:80-102) -------
static void ident(double m[12])
{
    for (int i = 0; i < 12; ++i) m[i] = 0.0;
    m[0] = m[5] = m[10] = 1.0;
}

// a <- b o a
static void pre_concat(double a[12], const double b[12])
{
    double r[12];
    for (int i = 0; i < 3; ++i) {
        const double* bi = b + 4 * i;
        for (int j = 0; j < 3; ++j) r[4 * i + j] = bi[0] * a[j] + bi[1] * a[4 + j] + bi[2] * a[8 + j];
        r[4 * i + 3] = bi[0] * a[3] + bi[1] * a[7] + bi[2] * a[11] + bi[3];
    }
    std::memcpy(a, r, sizeof(r));
}

void axis_rotation_host(const int64_t dim[3], int axis, int degrees, double m[12])
{
    // centre = (max - min) / 2 in integer arithmetic (SMVD:84-86)
    double c[3];
    for (int d = 0; d < 3; ++d) c[d] = (double)((dim[d] - 1) / 2);
    // (float)Math.toRadians(degrees) (SMVD:90)
    const double theta = (double)(float)((double)degrees * 0.017453292519943295);
    const double co = std::cos(theta), si = std::sin(theta);
    double t1[12], rot[12], t2[12];
    ident(t1); ident(rot); ident(t2);
    t1[3] = -c[0]; t1[7] = -c[1]; t1[11] = -c[2];
    t2[3] = c[0];  t2[7] = c[1];  t2[11] = c[2];
    switch (axis) {
        case 0:  rot[5] = co; rot[6] = -si; rot[9] = si;  rot[10] = co; break;
        case 1:  rot[0] = co; rot[2] = si;  rot[8] = -si; rot[10] = co; break;
        default: rot[0] = co; rot[1] = -si; rot[4] = si;  rot[5] = co;  break;
    }
    pre_concat(t1, rot);   // SMVD:98
    pre_concat(t1, t2);    // SMVD:99
    std::memcpy(m, t1, 12 * sizeof(double));
}

void affine_invert_host(const double m[12], double v[12])
{
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double det = a * e * i + d * h * c + g * b * f - c * e * g - f * h * a - i * b * d;
    v[0] = (e * i - f * h) / det;  v[1] = (c * h - b * i) / det;  v[2] = (b * f - c * e) / det;
    v[4] = (f * g - d * i) / det;  v[5] = (a * i - c * g) / det;  v[6] = (c * d - a * f) / det;
    v[8] = (d * h - e * g) / det;  v[9] = (b * g - a * h) / det;  v[10] = (a * e - b * d) / det;
    v[3]  = -v[0] * m[3] - v[1] * m[7] - v[2] * m[11];
    v[7]  = -v[4] * m[3] - v[5] * m[7] - v[6] * m[11];
    v[11] = -v[8] * m[3] - v[9] * m[7] - v[10] * m[11];
}

int join_tail(mvsim_ctx* ctx)
{
    if (ctx && ctx->tail_pending) {
        MVSIM_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_tail, 0));
        ctx->tail_pending = false;
    }
    return MVSIM_OK;
}

// every entry point starts here: the device, and a pending tail ordered in front of what the call enqueues
int set_device(mvsim_ctx* ctx, bool keep_tail)
{
    MVSIM_CHECK_ARG(ctx != nullptr, "ctx is null");
    ev_rebalance(ctx);
    MVSIM_HIP(hipSetDevice(ctx->device));
    if (!keep_tail) MVSIM_TRY(join_tail(ctx));
    return MVSIM_OK;
}

// The queue share of the context's next sampled view (QueueMode).  Option given: that.  Auto: what this context's views have needed so
// far -- k_poisson_refused leaves the sixteenths the fullest refused segment would have needed in a page-locked word, read here without
// synchronising: a view whose segments refuse voxels still gives the right counts (slower), and the views after it get the larger queue.
static int queue_mode_next(mvsim_ctx* ctx, QueueMode* qm)
{
    qm->share = 0; qm->hint = nullptr;
    if (ctx->opt.poisson_queue != 1) return MVSIM_OK;
    if (ctx->opt.poisson_queue_share > 0) { qm->share = ctx->opt.poisson_queue_share; return MVSIM_OK; }
    const unsigned int seen = *reinterpret_cast<volatile unsigned int*>(ctx->queue_hint);
    if ((int)seen >= ctx->queue_share_learned && seen != 0u) ctx->queue_share_learned = seen >= 15u ? 16 : (int)seen + 1;   // one sixteenth of headroom
    qm->share = QUEUE_SHARE_AUTO + ctx->queue_share_learned;
    qm->hint = ctx->queue_hint;
    return MVSIM_OK;
}

int extract_stage_plan(mvsim_ctx* ctx, const ExtractGeom& g, const ExtractOps& ops, ExtractPlan* pl, bool views_aligned16)
{
    const bool aligned16 = ops.nviews > 0 ? views_aligned16 : (reinterpret_cast<uintptr_t>(ops.in + g.in_offset) | reinterpret_cast<uintptr_t>(ops.out)) % 16 == 0;
    QueueMode qm;
    MVSIM_TRY(queue_mode_next(ctx, &qm));                 // (whether or not the launch samples: the learned share follows the hint word)
    *pl = extract_plan(g, aligned16, ops.noise, qm);
    if (ops.noise) MVSIM_TRY(ctx->pqueue.reserve(ops.nviews > 0 ? pl->layout.view_stride() * (size_t)ops.nviews : pl->layout.total_bytes));
    return MVSIM_OK;
}

// Will the launch behind a view's convolution be one of the two queue samplers, whichever planes the convolution leaves?  (The caller's
// half of the sparse tail's condition -- extract_plan.h: tail_queue_sampler -- from the sizes and the context's queue setting alone.)
bool extract_stage_queued(mvsim_ctx* ctx, const int64_t dim[3], int inc, bool noise)
{
    QueueMode qm;
    if (queue_mode_next(ctx, &qm) != MVSIM_OK) return false;
    return tail_queue_sampler(dim, inc, noise, qm);
}

int extract_stage_run(mvsim_ctx* ctx, const ExtractPlan& pl, ExtractOps& ops)
{
    if (ops.nviews == 0) ops.queue_ws = ops.noise ? ctx->pqueue.p : nullptr;
    ev_begin(ctx, ST_EXTRACT);
    MVSIM_TRY(launch_extract(ctx->stream, pl, ops));
    ev_end(ctx, ST_EXTRACT);
    const int64_t path[5] = {pl.kernel, pl.checked ? 1 : 0, pl.blocks, pl.segcap, ops.nviews > 0 ? ops.nviews : 1};
    std::memcpy(ctx->extract_path, path, sizeof(path));
    ctx->tail_path[0] = ops.empty_flags ? 1 : 0; ctx->tail_path[1] = ops.empty_flags ? ops.empty_stride : 0;
    return MVSIM_OK;
}

int extract_stage(mvsim_ctx* ctx, const ExtractGeom& g, ExtractOps& ops)
{
    ExtractPlan pl;
    MVSIM_TRY(extract_stage_plan(ctx, g, ops, &pl));
    return extract_stage_run(ctx, pl, ops);
}

// ---- extractSlices over intervals of device volumes (interval_plan.h, extract_interval.hip) ----------------------------------------
int interval_jobs_check(const mvsim_interval_job* jobs, int n, std::vector<IntervalGeom>* geoms)
{
    MVSIM_CHECK_ARG(jobs != nullptr, "interval jobs: null pointer");
    MVSIM_CHECK_ARG(n >= 1 && n <= MVSIM_MAX_VIEWS, "interval jobs: n must be in [1, MVSIM_MAX_VIEWS]");
    geoms->resize((size_t)n);
    for (int j = 0; j < n; ++j) {
        if (!jobs[j].in) { set_error("invalid argument: interval job %d: null volume", j); return MVSIM_EINVAL; }
        if (const char* why = interval_geom(jobs[j].dim, jobs[j].min, jobs[j].max, jobs[j].inc, &(*geoms)[(size_t)j])) {
            set_error("invalid argument: interval job %d: %s", j, why);
            return MVSIM_EINVAL;
        }
    }
    return MVSIM_OK;
}

static IntervalKey interval_key(const mvsim_interval_job& job, const IntervalGeom& g)
{
    IntervalKey k{{g.tile[0], g.tile[1], g.tile[2]}, g.inc, job.snr >= 0.0f, 0u};
    std::memcpy(&k.snr_bits, &job.snr, sizeof(k.snr_bits));
    return k;
}

// Jobs of one IntervalKey share their launches, the groups follow one another on the stream in the order of their first jobs.  One table
// upload and one queue workspace for the call: a group's queue regions are free again when the next group's phase 1 starts (stream order).
int extract_intervals_enqueue(mvsim_ctx* ctx, const mvsim_interval_job* jobs, const std::vector<IntervalGeom>& geoms, float* const* out_dev)
{
    const int n = (int)geoms.size();
    QueueMode qm;
    MVSIM_TRY(queue_mode_next(ctx, &qm));
    struct Group { IntervalPlan pl; std::vector<int> members; bool noise; double mul; };
    std::vector<Group> groups;
    std::vector<IntervalKey> keys;
    size_t queue_bytes = 0;
    for (int j = 0; j < n; ++j) {
        const IntervalKey key = interval_key(jobs[j], geoms[(size_t)j]);
        size_t gi = 0;
        while (gi < keys.size() && !(keys[gi] == key)) ++gi;
        if (gi == keys.size()) {
            keys.push_back(key);
            groups.push_back(Group{interval_plan(geoms[(size_t)j], key.noise, qm), {}, key.noise, mvsim_poisson_mul((double)jobs[j].snr)});
        }
        groups[gi].members.push_back(j);
    }
    for (const Group& g : groups)
        if (g.noise) queue_bytes = std::max(queue_bytes, g.pl.xp.layout.view_stride() * g.members.size());
    if (queue_bytes) MVSIM_TRY(ctx->pqueue.reserve(queue_bytes));
    const size_t off_r = ((size_t)n * sizeof(IntervalView) + 255) & ~(size_t)255, up_bytes = off_r + (size_t)n * sizeof(ExtractView);
    MVSIM_TRY(ctx->interval_tab.reserve(up_bytes));
    int slot = 0;
    MVSIM_TRY(ctx->pinned.acquire(up_bytes, &slot));
    char* hp = reinterpret_cast<char*>(ctx->pinned.p[slot]);
    char* dp = ctx->interval_tab.as<char>();
    IntervalView* vtab = reinterpret_cast<IntervalView*>(hp);
    ExtractView* rtab = reinterpret_cast<ExtractView*>(hp + off_r);
    int row = 0;
    for (const Group& g : groups)
        for (size_t m = 0; m < g.members.size(); ++m, ++row) {
            const int j = g.members[m];
            const IntervalGeom& ig = geoms[(size_t)j];
            const QueueLayout::Region q = g.pl.xp.layout.region(g.noise ? ctx->pqueue.p : nullptr, (int)m);
            vtab[row] = IntervalView{jobs[j].in + ig.in_offset, out_dev[j], q.items, q.counts, (uint32_t)jobs[j].seed, (uint32_t)(jobs[j].seed >> 32),
                                     jobs[j].stream, 0u, ig.row_pitch, ig.plane_pitch};
            rtab[row] = ExtractView{nullptr, out_dev[j], nullptr, q.items, q.counts, (uint32_t)jobs[j].seed, (uint32_t)(jobs[j].seed >> 32), jobs[j].stream, 0u};
        }
    MVSIM_HIP(hipMemcpyAsync(dp, hp, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    MVSIM_HIP(hipEventRecord(ctx->pinned.ev[slot], ctx->stream));
    ctx->pinned.busy[slot] = true;
    ev_begin(ctx, ST_EXTRACT);
    row = 0;
    for (const Group& g : groups) {
        const int m = (int)g.members.size();
        MVSIM_TRY(launch_extract_interval(ctx->stream, g.pl, reinterpret_cast<const IntervalView*>(dp) + row, reinterpret_cast<const ExtractView*>(dp + off_r) + row,
                                          m, g.noise, g.mul));
        const int64_t path[5] = {EXTRACT_K_INTERVAL, g.pl.xp.checked ? 1 : 0, g.pl.xp.blocks, g.pl.xp.segcap, m};
        std::memcpy(ctx->extract_path, path, sizeof(path));
        row += m;
    }
    ev_end(ctx, ST_EXTRACT);
    return MVSIM_OK;
}

// Tools.normImage on the host (Tools.java:112-132), in place (Q5): double sum, (float)(v / sum).
void psf_normalise_host(float* psf_host, int64_t n)
{
    // pairwise (cascade) double summation: same order of magnitude of error as mpicbg RealSum.  A binary counter of
    // partial sums (level l holds the sum of 2^l consecutive elements); aligned blocks of 16 enter it at level 4 with
    // their balanced tree written out -- the same additions in the same association as 16 single pushes (IEEE addition is
    // commutative), several times faster: this loop is on the host path of every view (29 791 taps for a 31^3 PSF).
    double lvl[64]; bool used[64] = {};
    int64_t i = 0;
    for (; i + 16 <= n; i += 16) {
        const float* q = psf_host + i;
        double t[8];
        for (int k = 0; k < 8; ++k) t[k] = (double)q[2 * k] + (double)q[2 * k + 1];
        double s = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
        int l = 4;
        while (used[l]) { used[l] = false; s += lvl[l]; ++l; }
        used[l] = true; lvl[l] = s;
    }
    for (; i < n; ++i) {
        double s = (double)psf_host[i];
        int l = 0;
        while (used[l]) { used[l] = false; s += lvl[l]; ++l; }
        used[l] = true; lvl[l] = s;
    }
    double sum = 0.0;
    for (int l = 0; l < 64; ++l) if (used[l]) sum += lvl[l];
    for (int64_t i = 0; i < n; ++i) psf_host[i] = (float)((double)psf_host[i] / sum);
}

int host_threads_of(const mvsim_ctx* ctx)            // ctx may be null: the process-wide default
{
    if (ctx && ctx->opt.host_threads > 0) return ctx->opt.host_threads;
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(16u, hw ? hw : 1u));
}

static void* psf_cache_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
static void psf_cache_free(void* p) { (void)hipFree(p); }     // (waits for the device: nothing still reads what an eviction frees)

// The cache entry of this normalised PSF for the convolution that follows, or null: the view uploads into ctx->psf_dev and
// transforms its PSF as ever.  *fresh: the entry is new, its device PSF is still to be uploaded.
static PsfCache::Entry* psf_cache_entry(mvsim_ctx* ctx, const float* psf_host, const int64_t kdim[3], const int64_t dim[3], bool* fresh)
{
    const Options& o = ctx->opt;
    *fresh = false;
    if (o.psf_cache <= 0 || !dim) return nullptr;
    if (o.graph) return nullptr;                                      // a captured graph holds pointers: G2 must stay ctx->cfft_g2
    ConvPlan pl;
    if (!conv_plan(dim, kdim, o, &pl)) return nullptr;                // rocFFT: another spectrum altogether
    if (!pl.zdirect || o.zpass == 3 || pl.zinline_auto) return nullptr;   // the padded and the inline FFT z pass read G2 in forms of their own
    PsfKey key{};
    for (int d = 0; d < 3; ++d) key.kdim[d] = kdim[d];
    key.px = pl.px; key.py = pl.py; key.pyb = pl.pyb; key.hxp = pl.hxp; key.zdirect = 1; key.tile_y = pl.tile_y; key.views = 1;
    const size_t n = (size_t)(kdim[0] * kdim[1] * kdim[2]);
    ctx->psf_cache.configure(psf_cache_alloc, psf_cache_free);
    if (PsfCache::Entry* e = ctx->psf_cache.find(key, psf_host, n)) return e;
    *fresh = true;
    // as much of G2 as the driver reserves for one view (fft_driver.hip: custom_fft_convolve_slab)
    return ctx->psf_cache.insert(key, psf_host, n, (size_t)pl.hxp * pl.pyb * pl.k[2] * sizeof(float2), (size_t)o.psf_cache << 20);
}

// Normalise the PSF on the host exactly as Tools.normImage does, in place (Q5), then place it in device memory -- unless the context
// holds the spectrum of these very taps already (cacheable: the caller is a whole single view on the hand-written FFT and needs
// ctx->psf_dev for nothing but the spectrum): then nothing is copied and nothing enqueued.
int psf_prepare(mvsim_ctx* ctx, float* psf_host, const int64_t kdim[3], const int64_t dim[3], bool cacheable)
{
    MVSIM_CHECK_ARG(psf_host != nullptr && kdim != nullptr, "psf is null");
    MVSIM_CHECK_ARG(kdim[0] >= 1 && kdim[1] >= 1 && kdim[2] >= 1, "psf dimensions must be >= 1");
    const int64_t n = kdim[0] * kdim[1] * kdim[2];
    psf_normalise_host(psf_host, n);
    ctx->psf_entry = nullptr;
    void* dst = nullptr;
    PsfCache::Entry* fresh_entry = nullptr;
    if (cacheable) {
        bool fresh = false;
        PsfCache::Entry* e = psf_cache_entry(ctx, psf_host, kdim, dim, &fresh);
        if (e && !fresh) { ctx->psf_entry = e; return MVSIM_OK; }     // a hit: its taps are on the device, behind their upload in stream order
        if (e) { dst = e->psf; fresh_entry = e; }
    }
    if (!dst) {
        MVSIM_TRY(ctx->psf_dev.reserve((size_t)n * sizeof(float)));
        dst = ctx->psf_dev.p;
    }
    // (a new entry that took over an evicted one's buffers: their last readers were that entry's PSF passes, joined to this stream since)
    int slot = 0;
    int rc = ctx->pinned.acquire((size_t)n * sizeof(float), &slot);
    if (rc == MVSIM_OK) {
        std::memcpy(ctx->pinned.p[slot], psf_host, (size_t)n * sizeof(float));
        if (hipMemcpyAsync(dst, ctx->pinned.p[slot], (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipEventRecord(ctx->pinned.ev[slot], ctx->stream) != hipSuccess) {
            set_error("PSF upload failed: %s", hipGetErrorString(hipGetLastError()));
            rc = MVSIM_EHIP;
        } else {
            ctx->pinned.busy[slot] = true;
        }
    }
    if (rc != MVSIM_OK) {
        if (fresh_entry) ctx->psf_cache.discard(fresh_entry);
        return rc;
    }
    ctx->psf_entry = fresh_entry;
    return MVSIM_OK;
}

int convolve_with_psf(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* psf_dev, const int64_t kdim[3], int method,
                      float* out, ConvTail* tail)
{
    MVSIM_CHECK_ARG(img != out, "convolve cannot run in place");
    if (pick_method(method, kdim) == 2) {
        if (tail) { tail->zstride = 1; tail->corr_done = false; }
        ev_begin(ctx, ST_CONVOLVE);
        MVSIM_TRY(launch_stencil(ctx, img, dim, psf_dev, kdim, out));
        ev_end(ctx, ST_CONVOLVE);
        return MVSIM_OK;
    }
    return fft_convolve(ctx, img, dim, psf_dev, kdim, out, tail);
}

int convolve_dev_impl(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const int64_t kdim[3], int method, float* out,
                      ConvTail* tail)
{
    // (a cached PSF's taps live in its entry; the driver takes the entry itself from ctx->psf_entry)
    const float* psf = ctx->psf_entry ? static_cast<const float*>(ctx->psf_entry->psf) : ctx->psf_dev.as<float>();
    return convolve_with_psf(ctx, img, dim, psf, kdim, method, out, tail);
}

}  // namespace mvsim

using namespace mvsim;

extern "C" {

const char* mvsim_version(void) { return "mvsim 0.1.0 (gfx950)"; }
const char* mvsim_last_error(void) { return g_err; }

int mvsim_device_count(int* count)
{
    MVSIM_CHECK_ARG(count != nullptr, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return MVSIM_ENODEV; }
    *count = n;
    return MVSIM_OK;
}

int mvsim_create(int device, mvsim_ctx** out)
{
    MVSIM_CHECK_ARG(out != nullptr, "ctx out pointer is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available (libmvsim has no CPU fallback)");
        return MVSIM_ENODEV;
    }
    MVSIM_CHECK_ARG(device >= 0 && device < n, "device index out of range");
    MVSIM_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MVSIM_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libmvsim is built for gfx950 only", device, prop.gcnArchName);
        return MVSIM_ENODEV;
    }
    mvsim_ctx* ctx = new (std::nothrow) mvsim_ctx();
    if (!ctx) { set_error("out of host memory"); return MVSIM_ENOMEM; }
    ctx->device = device;
    ctx->num_cu = prop.multiProcessorCount;
    ctx->opt = env_options();
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); delete ctx; return MVSIM_EHIP; }
    ctx->stream = ctx->own_stream;
    // (here and not at the first sampled view: that one may be inside a stream capture)
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->queue_hint), 4 * sizeof(unsigned int), hipHostMallocDefault) != hipSuccess) {
        set_error("hipHostMalloc failed");
        (void)hipStreamDestroy(ctx->own_stream);
        delete ctx;
        return MVSIM_EHIP;
    }
    ctx->queue_hint[0] = ctx->queue_hint[1] = ctx->queue_hint[2] = ctx->queue_hint[3] = 0u;
    *out = ctx;
    return MVSIM_OK;
}

int mvsim_destroy(mvsim_ctx* ctx)
{
    if (!ctx) return MVSIM_OK;
    (void)hipSetDevice(ctx->device);
    (void)join_tail(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    for (mvsim_ctx* l : ctx->lanes) (void)mvsim_destroy(l);
    ctx->lanes.clear();
    for (hipEvent_t e : ctx->lane_done) (void)hipEventDestroy(e);
    ctx->lane_done.clear();
    if (ctx->ev_lane_fork) { (void)hipEventDestroy(ctx->ev_lane_fork); ctx->ev_lane_fork = nullptr; }
    mvsim_comm_destroy(ctx);
    async_release(ctx);
    view_graphs_release(ctx);
    fft_release(ctx);                                     // plans, twiddles, weights; its workspaces are on the list like all others
    ctx->each_workspace([](DevBuf& b, int) { b.release(); });
    ctx->psf_cache.clear();
    for (CountsStaging* c : {&ctx->sync_counts, &ctx->async_counts[0], &ctx->async_counts[1]}) c->release();
    ctx->pinned.release_all();
    if (ctx->ev_created)
        for (int k = 0; k < mvsim_ctx::TIMING_SLOTS; ++k)
            for (int s = 0; s < ST_COUNT; ++s) { (void)hipEventDestroy(ctx->evr[k][s][0]); (void)hipEventDestroy(ctx->evr[k][s][1]); }
    if (ctx->tail_stream) { (void)hipStreamSynchronize(ctx->tail_stream); (void)hipStreamDestroy(ctx->tail_stream); (void)hipEventDestroy(ctx->ev_tail_fork); (void)hipEventDestroy(ctx->ev_tail); }
    if (ctx->side_stream) { (void)hipStreamDestroy(ctx->side_stream); (void)hipEventDestroy(ctx->ev_fork); (void)hipEventDestroy(ctx->ev_join); }
    if (ctx->empty_hint) (void)hipHostFree(ctx->empty_hint);
    if (ctx->queue_hint) (void)hipHostFree(ctx->queue_hint);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return MVSIM_OK;
}

int mvsim_set_stream(mvsim_ctx* ctx, void* hip_stream)
{
    MVSIM_TRY(set_device(ctx));
    ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return MVSIM_OK;
}

int mvsim_join(mvsim_ctx* ctx)
{
    return set_device(ctx);                              // joins a pending tail; nothing else to do
}

int mvsim_set_option(mvsim_ctx* ctx, const char* name, const char* value)
{
    MVSIM_CHECK_ARG(ctx != nullptr, "ctx is null");
    if (parse_option(ctx->opt, name, value) != MVSIM_OK) {
        set_error("invalid argument: option %s = %s", name ? name : "(null)", value ? value : "(null)");
        return MVSIM_EINVAL;
    }
    return MVSIM_OK;
}

int mvsim_synchronize(mvsim_ctx* ctx)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

int mvsim_release_caches(mvsim_ctx* ctx)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    for (mvsim_ctx* l : ctx->lanes) MVSIM_TRY(mvsim_release_caches(l));
    MVSIM_HIP(hipSetDevice(ctx->device));
    async_release(ctx);
    view_graphs_release(ctx);                             // captured launches point into the workspaces released below
    fft_release(ctx);
    ctx->each_workspace([](DevBuf& b, int traits) { if (!(traits & WS_KEPT)) b.release(); });
    ctx->psf_cache.clear();                               // (its counters of hits, misses and evictions stay)
    ctx->psf_entry = nullptr;
    ctx->weight_dim[0] = 0;
    // the page-locked twins too, whether or not the pipelined entry points ever set their slots up
    for (CountsStaging* c : {&ctx->sync_counts, &ctx->async_counts[0], &ctx->async_counts[1]}) c->release();
    return MVSIM_OK;
}

// Host-to-host copy on the library's host threads (the JNI shim's bulk copies between a Java heap array and a page-locked staging
// block: one JVM thread moves 0.54 GB in 16 ms into a live array and in 79 ms into a fresh one -- first-touch page faults --,
// profiles/r05_slab_copy.txt; several threads fault and copy in parallel).  ctx may be null: the process-wide default thread count.
int mvsim_host_copy(mvsim_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return MVSIM_OK;
    if (!dst || !src) { set_error("invalid argument: host_copy with a null pointer"); return MVSIM_EINVAL; }
    const size_t chunk = (size_t)4 << 20;
    const int threads = host_threads_of(ctx);
    if (bytes <= chunk || threads <= 1) { std::memmove(dst, src, bytes); return MVSIM_OK; }
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst), sr = reinterpret_cast<uintptr_t>(src);
    if (d < sr + bytes && sr < d + bytes) { std::memmove(dst, src, bytes); return MVSIM_OK; }      // overlapping ranges: one ordered move
    HostPool::get().run((int)((bytes + chunk - 1) / chunk), threads, [&](int c) {
        const size_t a = (size_t)c * chunk, n = std::min(chunk, bytes - a);
        std::memcpy(static_cast<char*>(dst) + a, static_cast<const char*>(src) + a, n);
    });
    return MVSIM_OK;
}

int mvsim_dev_alloc(mvsim_ctx* ctx, size_t bytes, void** dptr)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(dptr != nullptr, "dptr is null");
    *dptr = nullptr;
    if (bytes == 0) return MVSIM_OK;
    MVSIM_HIP(hipMalloc(dptr, bytes));
    return MVSIM_OK;
}

int mvsim_dev_free(mvsim_ctx* ctx, void* dptr)
{
    MVSIM_TRY(set_device(ctx));
    if (dptr && ctx->peer_copy) {
        // peers' IPC mappings registered for this allocation must not outlive it (mvsim_comm_register_volume)
        void* base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, dptr) == hipSuccess) comm_forget_range(ctx, base, size);
        else comm_forget_range(ctx, dptr, 0);
    }
    if (dptr) MVSIM_HIP(hipFree(dptr));
    return MVSIM_OK;
}

// Page-locked host memory: copies between it and HBM run at PCIe speed instead of through the runtime's staging of
// pageable memory.  The JNI shim wraps such blocks in direct ByteBuffers (NewDirectByteBuffer), numpy wraps them through
// the buffer protocol.
int mvsim_host_alloc(mvsim_ctx* ctx, size_t bytes, void** hptr)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(hptr != nullptr, "hptr is null");
    *hptr = nullptr;
    if (bytes == 0) return MVSIM_OK;
    hipError_t e = hipHostMalloc(hptr, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MVSIM_ENOMEM : MVSIM_EHIP;
    }
    return MVSIM_OK;
}

int mvsim_host_free(mvsim_ctx* ctx, void* hptr)
{
    if (ctx) {                                         // ctx may be NULL: blocks can outlive their context
        MVSIM_TRY(set_device(ctx));
        // a block that comes back from the allocator at the same address is a different ground truth
        for (int s = 0; s < mvsim_ctx::ASYNC_SLOTS; ++s)
            if (hptr && ctx->async_gt_src[s] == hptr) ctx->async_gt_src[s] = nullptr;
    }
    if (hptr) MVSIM_HIP(hipHostFree(hptr));
    return MVSIM_OK;
}

int mvsim_upload(mvsim_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes)
{
    MVSIM_TRY(set_device(ctx));
    if (bytes == 0) return MVSIM_OK;
    MVSIM_CHECK_ARG(dst_dev && src_host, "null pointer");
    MVSIM_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

int mvsim_dev_memset(mvsim_ctx* ctx, void* dptr, int value, size_t bytes)
{
    MVSIM_TRY(set_device(ctx));
    if (bytes == 0) return MVSIM_OK;
    MVSIM_CHECK_ARG(dptr != nullptr, "null pointer");
    MVSIM_HIP(hipMemsetAsync(dptr, value, bytes, ctx->stream));
    return MVSIM_OK;
}

int mvsim_download(mvsim_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes)
{
    MVSIM_TRY(set_device(ctx));
    if (bytes == 0) return MVSIM_OK;
    MVSIM_CHECK_ARG(dst_host && src_dev, "null pointer");
    MVSIM_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

// ---- host helpers ---------------------------------------------------------------------------------
int mvsim_axis_rotation(const int64_t dim[3], int axis, int degrees, double m[12])
{
    MVSIM_CHECK_ARG(dim && m, "null pointer");
    MVSIM_CHECK_ARG(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
    axis_rotation_host(dim, axis, degrees, m);
    return MVSIM_OK;
}

int64_t mvsim_extract_nz(int64_t nz, int inc) { return inc < 1 ? -1 : (nz - 1) / inc + 1; }
int64_t mvsim_isotropic_nz(int64_t nz_acq, int inc) { return inc < 1 ? -1 : (nz_acq - 1) * inc + 1; }
double  mvsim_poisson_mul(double snr) { return std::pow(snr / std::sqrt(5.0), 2.0); }

void mvsim_view_params_default(mvsim_view_params* p)
{
    if (!p) return;
    p->axis = 0; p->degrees = 15; p->delta = (double)0.01f /* `final float attenuation = 0.01f` widened, SMVD:533,573 */; p->min_value = 0.0001f; p->target_average = 1.0f;
    p->inc = 3; p->snr = 25.0f; p->seed = 464232194ULL; p->stream = 0; p->conv_method = 0;
}

// ---- device-resident stage operators --------------------------------------------------------------
int mvsim_rotate_around_axis_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int axis, int degrees,
                                 float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out && in != out, "null or aliased buffers");
    MVSIM_CHECK_ARG(axis >= 0 && axis <= 2, "axis must be 0, 1 or 2");
    double m[12];
    Affine inv;
    axis_rotation_host(dim, axis, degrees, m);
    affine_invert_host(m, inv.m);
    ev_begin(ctx, ST_ROTATE);
    MVSIM_TRY(launch_rotate(ctx->stream, in, out, dim, inv));
    ev_end(ctx, ST_ROTATE);
    return MVSIM_OK;
}

int mvsim_attenuate3d_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], double delta, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out && in != out, "null or aliased buffers");
    MVSIM_CHECK_ARG(dim[0] <= dim[1], "attenuate3d: Nx > Ny walks outside the interval in the reference (steps = dimension(0))");
    ev_begin(ctx, ST_ATTENUATE);
    if (ctx->opt.attenuate_scan) MVSIM_TRY(launch_attenuate_scan(ctx->stream, in, out, dim, delta));
    else MVSIM_TRY(launch_attenuate(ctx->stream, in, out, dim, delta));
    ev_end(ctx, ST_ATTENUATE);
    return MVSIM_OK;
}

int mvsim_convolve_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], float* psf_host,
                       const int64_t kdim[3], int method, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(img && out, "null buffer");
    MVSIM_CHECK_ARG(method >= 0 && method <= 2, "method must be 0, 1 or 2");
    MVSIM_TRY(psf_prepare(ctx, psf_host, kdim, dim, false));           // the stage operator: not a view, no PSF cache
    return convolve_dev_impl(ctx, img, dim, kdim, method, out);
}

int mvsim_adjust_image_dev(mvsim_ctx* ctx, float* img, int64_t n, float min_value, float target_average,
                           double* correction)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(img && n >= 1, "null buffer or empty image");
    double *partial, *scal;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
    ev_begin(ctx, ST_ADJUST);
    MVSIM_TRY(launch_sum(ctx->stream, img, n, partial, scal));
    MVSIM_TRY(launch_adjust_corr(ctx->stream, scal, n, min_value, target_average));
    MVSIM_TRY(launch_adjust_apply(ctx->stream, img, n, scal, min_value));
    ev_end(ctx, ST_ADJUST);
    if (correction) {
        MVSIM_HIP(hipMemcpyAsync(correction, scal + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MVSIM_OK;
}

int mvsim_extract_slices_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float snr,
                             uint64_t seed, uint32_t stream, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out, "null buffer");
    MVSIM_CHECK_ARG(inc >= 1, "inc must be >= 1");
    ExtractOps ops;
    ops.in = in; ops.out = out;
    ops.noise = snr >= 0.0f;   // SMVD:211
    ops.mul = mvsim_poisson_mul((double)snr); ops.seed = seed; ops.stream = stream;
    return extract_stage(ctx, ExtractGeom::strided(dim, inc), ops);
}

int mvsim_interval_out_dim(const mvsim_interval_job* job, int64_t out_dim[3])
{
    if (!job || !out_dim) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    IntervalGeom g;
    if (const char* why = interval_geom(job->dim, job->min, job->max, job->inc, &g)) { set_error("invalid argument: %s", why); return MVSIM_EINVAL; }
    out_dim[0] = g.tile[0]; out_dim[1] = g.tile[1]; out_dim[2] = g.nzo();
    return MVSIM_OK;
}

int mvsim_tile_interval(const int64_t dim[3], const double overlap_ratio[3], int tile, int64_t min[3], int64_t max[3], int64_t overlap[3])
{
    if (!dim || !overlap_ratio || !min || !max || !overlap) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(tile == 0 || tile == 1, "tile must be 0 or 1");
    tile_interval(dim, overlap_ratio, tile, min, max, overlap);
    return MVSIM_OK;
}

int mvsim_extract_intervals_dev(mvsim_ctx* ctx, const mvsim_interval_job* jobs, int n, float* const* out_dev)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(out_dev != nullptr, "interval jobs: null pointer");
    std::vector<IntervalGeom> geoms;
    MVSIM_TRY(interval_jobs_check(jobs, n, &geoms));
    // an output must not meet another output or any job's volume: the jobs of a launch run side by side
    for (int j = 0; j < n; ++j) {
        MVSIM_CHECK_ARG(out_dev[j] != nullptr, "interval jobs: null output");
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out_dev[j]), o1 = o0 + (uintptr_t)geoms[(size_t)j].n_out() * sizeof(float);
        for (int w = 0; w < n; ++w) {
            const uintptr_t v0 = reinterpret_cast<uintptr_t>(jobs[w].in), v1 = v0 + (uintptr_t)nvox(jobs[w].dim) * sizeof(float);
            const uintptr_t p0 = reinterpret_cast<uintptr_t>(out_dev[w]), p1 = p0 + (uintptr_t)geoms[(size_t)w].n_out() * sizeof(float);
            MVSIM_CHECK_ARG(!(o0 < v1 && v0 < o1), "interval jobs: an output overlaps a job's volume");
            MVSIM_CHECK_ARG(w <= j || !out_dev[w] || !(o0 < p1 && p0 < o1), "interval jobs: outputs overlap each other");
        }
    }
    return extract_intervals_enqueue(ctx, jobs, geoms, out_dev);
}

int mvsim_make_isotropic_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out, "null buffer");
    MVSIM_CHECK_ARG(inc >= 1, "inc must be >= 1");
    return launch_make_isotropic(ctx->stream, in, out, dim, inc);
}

int mvsim_compute_weight_image_dev(mvsim_ctx* ctx, const int64_t dim[3], float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(out, "null buffer");
    return launch_weight_image(ctx->stream, out, dim);
}

// ---- cross-view weight normalisation -------------------------------------------------------------------
static int views_args(mvsim_ctx* ctx, const float* const* vols, int n_views, int64_t n, bool out_ok)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(vols && out_ok && n >= 1, "null pointer or empty image");
    MVSIM_CHECK_ARG(n_views >= 1 && n_views <= MVSIM_MAX_VIEWS, "n_views must be in [1, MVSIM_MAX_VIEWS]");
    for (int v = 0; v < n_views; ++v) MVSIM_CHECK_ARG(vols[v] != nullptr, "null view pointer");
    return MVSIM_OK;
}

int mvsim_sum_views_dev(mvsim_ctx* ctx, const float* const* vols, int n_views, int64_t n, float* out)
{
    MVSIM_TRY(views_args(ctx, vols, n_views, n, out != nullptr));
    return launch_weights(ctx->stream, const_cast<float* const*>(vols), n_views, n, nullptr, out, 0.0f, true);
}

int mvsim_normalize_weights_dev(mvsim_ctx* ctx, float* const* weights, int n_views, int64_t n, const float* sum_or_null,
                                float osem)
{
    MVSIM_TRY(views_args(ctx, weights, n_views, n, true));
    return launch_weights(ctx->stream, weights, n_views, n, sum_or_null, nullptr, osem, false);
}

int mvsim_normalize_weights(mvsim_ctx* ctx, float* const* weights, int n_views, int64_t n, float osem)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(weights && n >= 1, "null pointer or empty image");
    MVSIM_CHECK_ARG(n_views >= 1 && n_views <= MVSIM_MAX_VIEWS, "n_views must be in [1, MVSIM_MAX_VIEWS]");
    const size_t bytes = (size_t)n * sizeof(float);
    std::vector<DevBuf> bufs((size_t)n_views);
    std::vector<float*> dptr((size_t)n_views);
    int rc = MVSIM_OK;
    for (int v = 0; v < n_views && rc == MVSIM_OK; ++v) {
        if (!weights[v]) { set_error("invalid argument: null view pointer"); rc = MVSIM_EINVAL; break; }
        rc = bufs[v].reserve(bytes);
        if (rc == MVSIM_OK && hipMemcpyAsync(bufs[v].p, weights[v], bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            set_error("upload of view %d failed", v); rc = MVSIM_EHIP;
        }
        dptr[v] = bufs[v].as<float>();
    }
    if (rc == MVSIM_OK) rc = launch_weights(ctx->stream, dptr.data(), n_views, n, nullptr, nullptr, osem, false);
    for (int v = 0; v < n_views && rc == MVSIM_OK; ++v)
        if (hipMemcpyAsync(weights[v], bufs[v].p, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
            set_error("download of view %d failed", v); rc = MVSIM_EHIP;
        }
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& b : bufs) b.release();
    return rc;
}

int mvsim_get_plane_stats(mvsim_ctx* ctx, int64_t stats[3])
{
    MVSIM_CHECK_ARG(ctx != nullptr && stats != nullptr, "null pointer");
    stats[0] = stats[1] = stats[2] = 0;
    if (ctx->empty_hint && ctx->empty_hint[0] >= 0) {
        const volatile int* h = ctx->empty_hint;
        stats[0] = h[2]; stats[1] = h[0]; stats[2] = h[1] >= 0 ? h[1] : 0;
    }
    return MVSIM_OK;
}

int mvsim_get_queue_stats(mvsim_ctx* ctx, int64_t stats[6])
{
    MVSIM_CHECK_ARG(ctx != nullptr && stats != nullptr, "null pointer");
    for (int i = 0; i < 6; ++i) stats[i] = 0;
    stats[0] = (int64_t)ctx->pqueue.bytes;
    if (!ctx->pqueue.p) return MVSIM_OK;
    MVSIM_TRY(mvsim_synchronize(ctx));
    long long q[5] = {0, 0, 0, 0, 0};
    MVSIM_TRY(poisson_queue_read_stats(ctx->pqueue.p, ctx->pqueue.bytes, q));
    for (int i = 0; i < 5; ++i) stats[1 + i] = q[i];
    return MVSIM_OK;
}

int mvsim_get_transfer_stats(mvsim_ctx* ctx, int64_t* views_as_u16, int64_t* fallbacks)
{
    MVSIM_CHECK_ARG(ctx != nullptr, "ctx is null");
    if (views_as_u16) *views_as_u16 = ctx->u16_views;
    if (fallbacks) *fallbacks = ctx->u16_fallbacks;
    return MVSIM_OK;
}

int mvsim_stencil_geometry(const int64_t kdim[3], int64_t geometry[5])
{
    if (!kdim || !geometry) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    if (!stencil_chunk_geometry(kdim, geometry)) {
        set_error("direct stencil: PSF outside 1..64 taps per axis");
        return MVSIM_EINVAL;
    }
    return MVSIM_OK;
}

int mvsim_extract_path(const int64_t dim[3], int inc, int index_inc, uint64_t index_offset, int aligned16, int queue_share, int64_t path[4])
{
    if (!dim || !path) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(inc >= 1 && index_inc >= 0, "inc must be >= 1 and index_inc >= 0");
    MVSIM_CHECK_ARG(0 <= queue_share && queue_share <= 16, "queue_share must be 0 (no queue) or 1..16 sixteenths");
    extract_path(dim, inc, index_inc, index_offset, aligned16 != 0, queue_share, path);
    return MVSIM_OK;
}

int mvsim_get_extract_path(mvsim_ctx* ctx, int64_t path[5])
{
    MVSIM_CHECK_ARG(ctx != nullptr && path != nullptr, "null pointer");
    std::memcpy(path, ctx->extract_path, sizeof(ctx->extract_path));
    return MVSIM_OK;
}

int mvsim_get_tail_path(mvsim_ctx* ctx, int64_t out[2])
{
    MVSIM_CHECK_ARG(ctx != nullptr && out != nullptr, "null pointer");
    out[0] = ctx->tail_path[0]; out[1] = ctx->tail_path[1];
    return MVSIM_OK;
}

int mvsim_get_psf_cache_stats(mvsim_ctx* ctx, int64_t out[4])
{
    MVSIM_CHECK_ARG(ctx != nullptr && out != nullptr, "null pointer");
    const PsfCache::Stats& st = ctx->psf_cache.stats();
    out[0] = st.hits; out[1] = st.misses; out[2] = st.evictions; out[3] = st.bytes;
    return MVSIM_OK;
}

int mvsim_fused_tail_geometry(mvsim_ctx* ctx, const int64_t dim[3], const int64_t kdim[3], int inc, int want_con, int64_t out[2])
{
    MVSIM_CHECK_ARG(ctx != nullptr && dim && kdim && out, "null pointer");
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(inc >= 1, "inc must be >= 1");
    ExtractPlan fp{};
    // what view_enqueue asks of a noisy view before it offers the convolution its tail
    if (!ctx->opt.fuse_tail || ctx->opt.poisson_queue != 1 || !fused_tail_geometry(dim, kdim, inc, want_con != 0, ctx->opt, &fp)) {
        set_error("this view would not take the fused tail");
        return MVSIM_EINVAL;
    }
    out[0] = fp.blocks; out[1] = fp.segcap;
    return MVSIM_OK;
}

int mvsim_fft_geometry(const int64_t dim[3], const int64_t kdim[3], int64_t geometry[5])
{
    if (!dim || !kdim || !geometry) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    MVSIM_TRY(check_dim(dim));
    if (!custom_fft_geometry(dim, kdim, geometry, env_options())) {
        set_error("no hand-written FFT size for this volume / PSF");
        return MVSIM_EINVAL;
    }
    return MVSIM_OK;
}

int mvsim_zpass_geometry(const int64_t dim[3], const int64_t kdim[3], int inc, int64_t out[4])
{
    if (!dim || !kdim || !out) { set_error("invalid argument: null pointer"); return MVSIM_EINVAL; }
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(inc >= 1, "inc must be >= 1");
    if (!custom_zpass_geometry(dim, kdim, inc, out, env_options())) {
        set_error("this view's z pass is not the direct convolution");
        return MVSIM_EINVAL;
    }
    return MVSIM_OK;
}

// ---- timings ---------------------------------------------------------------------------------------
int mvsim_enable_timing(mvsim_ctx* ctx, int enable)
{
    MVSIM_TRY(set_device(ctx));
    if (enable && !ctx->ev_created) {
        for (int k = 0; k < mvsim_ctx::TIMING_SLOTS; ++k)
            for (int s = 0; s < ST_COUNT; ++s) {
                MVSIM_HIP(hipEventCreate(&ctx->evr[k][s][0]));
                MVSIM_HIP(hipEventCreate(&ctx->evr[k][s][1]));
            }
        ctx->ev_created = true;
    }
    ctx->timing = enable != 0;
    ctx->ev_cur = 0;
    ctx->ev_calls = 0;
    for (int s = 0; s < ST_COUNT; ++s) ctx->ev_used[0][s] = false;
    return MVSIM_OK;
}

// Averages over the calls recorded since timing was enabled or last read (at most the last TIMING_SLOTS calls).
int mvsim_get_timings(mvsim_ctx* ctx, mvsim_timings* t)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(t != nullptr, "timings pointer is null");
    MVSIM_CHECK_ARG(ctx->ev_created, "timing was never enabled");
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    double sum[ST_COUNT] = {};
    int cnt[ST_COUNT] = {};
    const long long calls = ctx->ev_calls == 0 ? 1 : ctx->ev_calls;    // stage operators outside simulate_view use slot 0
    const int nslots = (int)(calls < mvsim_ctx::TIMING_SLOTS ? calls : mvsim_ctx::TIMING_SLOTS);
    for (int j = 0; j < nslots; ++j) {
        const int k = ((ctx->ev_cur - j) % mvsim_ctx::TIMING_SLOTS + mvsim_ctx::TIMING_SLOTS) % mvsim_ctx::TIMING_SLOTS;
        for (int s = 0; s < ST_COUNT; ++s) {
            if (!ctx->ev_used[k][s]) continue;
            float ms = 0.f;
            MVSIM_HIP(hipEventElapsedTime(&ms, ctx->evr[k][s][0], ctx->evr[k][s][1]));
            sum[s] += ms;
            cnt[s] += 1;
            ctx->ev_used[k][s] = false;
        }
    }
    float ms[ST_COUNT];
    float total = 0.f;
    for (int s = 0; s < ST_COUNT; ++s) {
        ms[s] = cnt[s] ? (float)(sum[s] / cnt[s]) : 0.f;
        // views whose PSF spectrum came from the cache recorded no PSF stage: the average is over every convolution all the same
        if (s == ST_PSF && cnt[ST_CONVOLVE] > cnt[s]) ms[s] = (float)(sum[s] / cnt[ST_CONVOLVE]);
        // a PSF spectrum that ran on the side stream overlaps passes A and B: it is part of convolve_ms, not a stage of its own
        if (s == ST_PSF && ctx->psf_on_side) ms[s] = 0.f;
        if (s < ST_PASS_A) total += ms[s];              // the passes are nested inside ST_CONVOLVE
    }
    t->rotate_ms = ms[ST_ROTATE]; t->attenuate_ms = ms[ST_ATTENUATE]; t->psf_ms = ms[ST_PSF];
    t->convolve_ms = ms[ST_CONVOLVE]; t->adjust_ms = ms[ST_ADJUST]; t->extract_ms = ms[ST_EXTRACT];
    t->total_ms = total;
    t->pass_a_ms = ms[ST_PASS_A]; t->pass_b_ms = ms[ST_PASS_B]; t->pass_c_ms = ms[ST_PASS_C];
    t->pass_d_ms = ms[ST_PASS_D]; t->pass_e_ms = ms[ST_PASS_E];
    ctx->last = *t;
    ctx->ev_cur = 0;
    ctx->ev_calls = 0;
    return MVSIM_OK;
}

}  // extern "C"
