// C ABI of libmvsim, part 2: the fused per-view pipeline on device buffers -- view_enqueue and its hipGraph cache, lanes and stacked
// views, main's whole iteration, and the z-slab tiling of one view.
#include "api_internal.h"

using namespace mvsim;

void mvsim::view_graphs_release(mvsim_ctx* ctx)
{
    for (auto& g : ctx->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    ctx->graphs.clear();
    ctx->graph_seen.clear();
}

extern "C" {

// ---- fused per-view pipeline ------------------------------------------------------------------------
// Everything a view enqueues on the context stream behind the PSF upload: kernel launches only (no allocation once the
// workspaces have their size, no host synchronisation) -- which is what makes it capturable into a hipGraph.
static bool ranges_meet(const void* a, size_t abytes, const char* lo, const char* hi)
{
    const char* p = reinterpret_cast<const char*>(a);
    return a && lo && p < hi && lo < p + abytes;
}

// overlap_ok: the tail (extract + Poisson) may stay pending on the tail stream when the call returns (join_tail)
static int view_enqueue(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], const int64_t kdim[3], const mvsim_view_params* p,
                        const mvsim_view_outputs* o, bool overlap_ok = false)
{
    const int64_t n = nvox(dim);
    const size_t vbytes = (size_t)n * sizeof(float);
    float* rot = o->rot;
    float* att = o->att;
    float* con = o->con;
    // (the attenuated volume gets its scratch only where a kernel writes it: behind the fused rotate + attenuate + x transform
    // nothing does, and a 512^3 / 1024^3 view keeps 0.5 / 4 GiB of HBM it would never touch)
    if (ctx->tail_pending) {
        // the previous view's tail still writes its acquisition and reads its convolved volume: this view's first stage
        // may run beside it only if it touches neither
        bool meet = false;
        for (int r = 0; r < 2; ++r)
            meet = meet || ranges_meet(gt, vbytes, ctx->tail_lo[r], ctx->tail_hi[r]) || ranges_meet(rot, vbytes, ctx->tail_lo[r], ctx->tail_hi[r]) ||
                   ranges_meet(att, vbytes, ctx->tail_lo[r], ctx->tail_hi[r]);
        if (meet) MVSIM_TRY(join_tail(ctx));
    }

    double m[12];
    Affine inv;
    axis_rotation_host(dim, p->axis, p->degrees, m);
    affine_invert_host(m, inv.m);
    // rotation about x: rotate and attenuate run as one kernel and `rot` is written only when requested
    bool fused = false;
    // ... and when the FFT passes follow, their x transform rides in the same kernel: `att` leaves the chip only if asked for
    bool x_done = false;
    const int* plane_nz = nullptr;
    const unsigned int* row_bits = nullptr;
    ev_begin(ctx, ST_ROTATE);
    if (pick_method(p->conv_method, kdim) == 1)
        MVSIM_TRY(rotate_attenuate_fftx(ctx, gt, rot, o->att, dim, kdim, inv, p->delta, &x_done, &plane_nz, 0, -1, &row_bits));
    fused = x_done;
    if (!x_done) {
        if (!att) { MVSIM_TRY(ctx->vol_b.reserve(vbytes)); att = ctx->vol_b.as<float>(); }
        MVSIM_TRY(launch_rotate_attenuate(ctx->stream, gt, rot, att, dim, inv, p->delta, ctx->opt.fused_rotate, &fused));
    }
    if (!fused) {
        MVSIM_TRY(join_tail(ctx));                      // the rotation scratch is the buffer a pending tail reads
        if (!rot) { MVSIM_TRY(ctx->vol_a.reserve(vbytes)); rot = ctx->vol_a.as<float>(); }
        MVSIM_TRY(launch_rotate(ctx->stream, gt, rot, dim, inv));
    }
    ev_end(ctx, ST_ROTATE);
    // everything below reuses the workspaces of the previous view
    MVSIM_TRY(join_tail(ctx));
    if (!fused) {
        ev_begin(ctx, ST_ATTENUATE);
        MVSIM_TRY(launch_attenuate(ctx->stream, rot, att, dim, p->delta));
        ev_end(ctx, ST_ATTENUATE);
    }
    if (!con) { MVSIM_TRY(ctx->vol_a.reserve(vbytes)); con = ctx->vol_a.as<float>(); }   // vol_a: rot scratch is dead by now

    double *partial, *scal;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
    const int method = pick_method(p->conv_method, kdim);
    const bool materialise = o->con != nullptr;
    const bool noise = p->snr >= 0.0f;
    // only every inc-th plane is acquired: when the adjusted volume itself is not asked for, the last two passes of the
    // convolution need not produce the other planes (the convolution says whether it could honour that)
    ConvTail tail;
    tail.zstride = (!materialise && p->inc > 1 && (!noise || ctx->opt.poisson_queue == 1)) ? p->inc : 1;
    tail.corr_n = n; tail.min_value = p->min_value; tail.target_average = p->target_average;
    tail.x_done = x_done;
    tail.plane_nz = x_done ? plane_nz : nullptr;
    tail.row_bits = x_done ? row_bits : nullptr;
    // the sparse tail, the caller's half (extract_plan.h): `con` is the context's workspace, which nothing but this view's sampler reads,
    // and that sampler will be one of the two that take the flags -- settled here, on the host, before pass E is enqueued
    tail.want_sparse = tail.plane_nz != nullptr &&
                       tail_sparse_caller(ctx->opt.skip_tail, materialise, extract_stage_queued(ctx, dim, p->inc, noise));
    if (method == 1 && ctx->opt.fuse_tail && (!noise || ctx->opt.poisson_queue == 1)) {
        const size_t qb = noise ? fused_tail_queue_bytes(dim, kdim, p->inc, materialise, ctx->opt) : 0;
        if (!noise || qb > 0) {
            if (qb) MVSIM_TRY(ctx->pqueue.reserve(qb));
            tail.want_fuse = true;
            tail.min_value = p->min_value; tail.target_average = p->target_average;
            tail.con_adj = materialise ? con : nullptr;
            tail.acq = o->acq; tail.inc = p->inc; tail.noise = noise;
            tail.mul = mvsim_poisson_mul((double)p->snr); tail.seed = p->seed; tail.stream = p->stream;
        }
    }
    MVSIM_TRY(convolve_dev_impl(ctx, att, dim, kdim, method, con, &tail));
    if (tail.fused) {                  // pass E adjusted, extracted and sampled (phase 1); the resolver is enqueued behind it
        const int64_t fused[5] = {EXTRACT_FUSED_TAIL, 0, tail.fused_blocks, noise ? (int64_t)tail.fused_segcap : 0, 1};
        std::memcpy(ctx->extract_path, fused, sizeof(fused));
        ctx->tail_path[0] = ctx->tail_path[1] = 0;
        return MVSIM_OK;
    }
    if (tail.sparse && (materialise || method != 1)) { set_error("sparse tail behind a view that did not ask for it"); return MVSIM_EINVAL; }

    ev_begin(ctx, ST_ADJUST);
    if (method == 2) MVSIM_TRY(launch_sum(ctx->stream, con, n, partial, scal));   // FFT path sums in its crop epilogue
    if (!tail.corr_done) MVSIM_TRY(launch_adjust_corr(ctx->stream, scal, n, p->min_value, p->target_average));
    if (materialise) MVSIM_TRY(launch_adjust_apply(ctx->stream, con, n, scal, p->min_value));
    ev_end(ctx, ST_ADJUST);

    const int64_t n_out = dim[0] * dim[1] * mvsim_extract_nz(dim[2], p->inc);
    ExtractOps ops;
    ops.in = con; ops.out = o->acq; ops.scal = scal;
    ops.min_value = p->min_value; ops.noise = noise; ops.mul = mvsim_poisson_mul((double)p->snr); ops.seed = p->seed; ops.stream = p->stream;
    ops.adjust = !materialise;             // a materialised volume is adjusted already
    // a sparse tail: `con` has holes where these flags are clear, and launch_extract refuses every form but the two that read them.
    // The flag words belong to this view until the next view's rotate kernel rewrites them; that kernel is enqueued behind this
    // tail -- same stream, or joined (below: a sparse tail never stays pending on the tail stream)
    if (tail.sparse) { ops.empty_flags = tail.sparse_flags; ops.empty_stride = tail.sparse_stride; }
    // compact: `con` holds the acquired planes only (read in order, the RNG counted in source planes).  The queue grows here, before the tail forks
    ExtractPlan xpl;
    MVSIM_TRY(extract_stage_plan(ctx, tail.zstride > 1 ? ExtractGeom::compact(dim, p->inc) : ExtractGeom::strided(dim, p->inc), ops, &xpl));
    // The tail runs on a stream of its own and is joined by whatever the context does next (join_tail): the next view's
    // rotate+attenuate leaves most of the chip idle and runs beside it.
    // (not beside the fused rotate + attenuate + x transform of the next view: that kernel is bound by vector issue like the
    // sampler itself, and the two together measured slower than one after the other -- 17.6 against 17.2 ms per 8 views)
    if (x_done) overlap_ok = false;
    // (a sparse tail implies x_done today.  Should the line above ever go: the pending tail would be reading ctx->plane_flags while the
    // next view's rotate kernel rewrites them, and join_tail's ranges do not cover that workspace)
    if (tail.sparse) overlap_ok = false;
    hipStream_t tail_on = ctx->stream;
    if (overlap_ok) {
        if (!ctx->tail_stream) {
            MVSIM_HIP(hipStreamCreateWithFlags(&ctx->tail_stream, hipStreamNonBlocking));
            MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_tail_fork, hipEventDisableTiming));
            MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_tail, hipEventDisableTiming));
        }
        MVSIM_HIP(hipEventRecord(ctx->ev_tail_fork, ctx->stream));
        MVSIM_HIP(hipStreamWaitEvent(ctx->tail_stream, ctx->ev_tail_fork, 0));
        tail_on = ctx->tail_stream;
    }
    StreamSwap swap(ctx, tail_on);
    MVSIM_TRY(extract_stage_run(ctx, xpl, ops));
    if (overlap_ok) {
        MVSIM_HIP(hipEventRecord(ctx->ev_tail, ctx->tail_stream));
        ctx->tail_pending = true;
        ctx->tail_lo[0] = reinterpret_cast<const char*>(o->acq); ctx->tail_hi[0] = ctx->tail_lo[0] + (size_t)n_out * sizeof(float);
        ctx->tail_lo[1] = reinterpret_cast<const char*>(con);    ctx->tail_hi[1] = ctx->tail_lo[1] + vbytes;
    }
    return MVSIM_OK;
}


// hipGraph replay of a view (option "graph"): host launch cost is what bounds small volumes (130 us to issue the 14
// launches of a 128^3 view against ~0.1 ms of device time).  A captured view bakes in its pointers and by-value
// parameters (affine model of the angle, seed, stream id), so the cache is keyed by ALL of them: the first call with a key
// runs eagerly (workspaces, twiddles), the second is captured and instantiated, later ones replay.  The PSF upload stays
// outside the graph (its pinned staging slot changes from call to call).
static std::string view_graph_key(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], const int64_t kdim[3],
                                  const mvsim_view_params* p, const mvsim_view_outputs* o)
{
    std::string k;
    auto add = [&](const void* ptr, size_t bytes) { k.append(reinterpret_cast<const char*>(ptr), bytes); };
    add(&gt, sizeof(gt)); add(dim, 3 * sizeof(int64_t)); add(kdim, 3 * sizeof(int64_t));
    // field by field: the struct has padding bytes
    add(&p->axis, sizeof(p->axis)); add(&p->degrees, sizeof(p->degrees)); add(&p->delta, sizeof(p->delta));
    add(&p->min_value, sizeof(p->min_value)); add(&p->target_average, sizeof(p->target_average)); add(&p->inc, sizeof(p->inc));
    add(&p->snr, sizeof(p->snr)); add(&p->seed, sizeof(p->seed)); add(&p->stream, sizeof(p->stream));
    add(&p->conv_method, sizeof(p->conv_method));
    add(&o->rot, sizeof(o->rot)); add(&o->att, sizeof(o->att)); add(&o->con, sizeof(o->con)); add(&o->acq, sizeof(o->acq));
    add(&ctx->stream, sizeof(ctx->stream));
    const Options& q = ctx->opt;
    const int oo[16] = {q.zpass, q.rocfft ? 1 : 0, q.fused_rotate, q.poisson_queue, q.early_sum ? 1 : 0, q.fuse_tail ? 1 : 0, q.psf_overlap ? 1 : 0,
                        q.attenuate_scan ? 1 : 0, q.fused_fftx, q.zconv_strided ? 1 : 0, q.skip_empty ? 1 : 0, q.exp, q.poisson_queue_share, ctx->queue_share_learned,
                        q.skip_rows ? 1 : 0, q.skip_tail ? 1 : 0};
    add(oo, sizeof(oo));
    add(q.fft_pad, sizeof(q.fft_pad));
    return k;
}

static int view_graph_launch(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], const int64_t kdim[3], const mvsim_view_params* p,
                             const mvsim_view_outputs* o)
{
    const std::string key = view_graph_key(ctx, gt, dim, kdim, p, o);
    ctx->graph_tick += 1;
    const unsigned long long epoch = ctx->alloc_epoch;
    if (ctx->graph_epoch != epoch) {
        // some workspace was (re)allocated since the graphs were captured: their baked-in addresses may be stale
        for (auto& g : ctx->graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
        ctx->graphs.clear();
        ctx->graph_epoch = epoch;
    }
    for (auto& g : ctx->graphs)
        if (g.key == key) {
            g.last_use = ctx->graph_tick;
            MVSIM_HIP(hipGraphLaunch(g.exec, ctx->stream));
            return MVSIM_OK;
        }
    if (!ctx->graph_seen.count(key)) {
        // first sight: run eagerly (this is also what sizes every workspace and table the capture must not allocate)
        if (ctx->graph_seen.size() > 4096) ctx->graph_seen.clear();
        ctx->graph_seen.insert(key);
        return view_enqueue(ctx, gt, dim, kdim, p, o);
    }
    MVSIM_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
    const int rc = view_enqueue(ctx, gt, dim, kdim, p, o);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
    if (rc != MVSIM_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ctx->alloc_epoch != epoch) {
        // an allocation slipped into the capture (a workspace grew): do not keep this graph; run the view eagerly
        if (graph) (void)hipGraphDestroy(graph);
        return view_enqueue(ctx, gt, dim, kdim, p, o);
    }
    if (e != hipSuccess || !graph) { set_error("hipStreamEndCapture failed: %s", hipGetErrorString(e)); return MVSIM_EHIP; }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (ei != hipSuccess) { (void)hipGraphDestroy(graph); set_error("hipGraphInstantiate failed: %s", hipGetErrorString(ei)); return MVSIM_EHIP; }
    if (ctx->graphs.size() >= 32) {                       // evict the least recently used
        size_t victim = 0;
        for (size_t i = 1; i < ctx->graphs.size(); ++i) if (ctx->graphs[i].last_use < ctx->graphs[victim].last_use) victim = i;
        (void)hipGraphExecDestroy(ctx->graphs[victim].exec);
        (void)hipGraphDestroy(ctx->graphs[victim].graph);
        ctx->graphs.erase(ctx->graphs.begin() + (long)victim);
    }
    ctx->graphs.push_back(mvsim_ctx::ViewGraph{key, graph, exec, ctx->graph_tick});
    MVSIM_HIP(hipGraphLaunch(exec, ctx->stream));
    return MVSIM_OK;
}

// keep_psf_dev: the caller reads ctx->psf_dev behind the view (main's iteration: view_psf), so the view uploads its PSF whatever the cache holds
static int simulate_view_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* psf_host, const int64_t kdim[3],
                             const mvsim_view_params* p, const mvsim_view_outputs* o, double* correction, bool keep_psf_dev)
{
    MVSIM_TRY(set_device(ctx, /*keep_tail=*/true));
    // The previous view's tail may stay in flight beside this view's first stage, and this view's tail behind the call,
    // where nothing but this library can observe the difference: the context's own stream, no host-visible result, no graph.
    const bool overlap = ctx->opt.tail_overlap != 0 && (ctx->opt.tail_overlap == 2 || ctx->stream == ctx->own_stream) &&
                         !ctx->opt.graph && !correction && dim &&
                         dim[0] > 0 && dim[1] > 0 && dim[2] > 0 && dim[0] * dim[1] * dim[2] >= ((int64_t)1 << 24);
    if (!overlap) MVSIM_TRY(join_tail(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(gt && p && o, "null pointer");
    MVSIM_CHECK_ARG(o->acq != nullptr, "outputs.acq is required");
    MVSIM_CHECK_ARG(p->axis >= 0 && p->axis <= 2, "axis must be 0, 1 or 2");
    MVSIM_CHECK_ARG(p->inc >= 1, "inc must be >= 1");
    MVSIM_CHECK_ARG(p->conv_method >= 0 && p->conv_method <= 2, "conv_method must be 0, 1 or 2");
    MVSIM_CHECK_ARG(dim[0] <= dim[1], "attenuate3d: Nx > Ny walks outside the interval in the reference");
    ev_next(ctx);
    // (conv_method 2, the stencil, has no spectrum)
    MVSIM_TRY(psf_prepare(ctx, psf_host, kdim, dim, !keep_psf_dev && kdim && pick_method(p->conv_method, kdim) == 1));
    // a view replays from a graph when asked to, unless stage events are being recorded (they would be captured too) or
    // the convolution would go through rocFFT (library calls inside a capture are not ours to vouch for)
    int64_t P[3];
    const bool capturable = pick_method(p->conv_method, kdim) == 2 || custom_fft_sizes(dim, kdim, P, ctx->opt);
    if (ctx->opt.graph && !ctx->timing && capturable) MVSIM_TRY(view_graph_launch(ctx, gt, dim, kdim, p, o));
    else MVSIM_TRY(view_enqueue(ctx, gt, dim, kdim, p, o, overlap));
    if (correction) {
        double *partial, *scal;
        MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
        MVSIM_HIP(hipMemcpyAsync(correction, scal + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MVSIM_OK;
}

int mvsim_simulate_view_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* psf_host,
                            const int64_t kdim[3], const mvsim_view_params* p, const mvsim_view_outputs* o,
                            double* correction)
{
    return simulate_view_dev(ctx, gt, dim, psf_host, kdim, p, o, correction, false);
}

// How many views of this size run side by side on LANES -- the form for views that cannot be stacked (an adjusted volume requested,
// another spacing per view, ...).  A view is a chain of ~12 dependent launches that each leave CUs idle below ~2^24 voxels, so two to
// four chains side by side hide part of each other's latency; beyond that the host's launch rate is the bound (~75 us per view), and
// from 289^3 up lanes LOSE (kernels that each fill the CUs run one after the other anyway, and their working sets evict each other).
// Measured (profiles/r05_small_views.txt): 64^3 3.4 -> 4.5 Gvoxel/s and 128^3 16.7 -> 25.0 with four lanes, 256^3 41 -> 49 with two
// (37 with four), 289^3 48 -> 24 with four: DESIGN 4.8.
static int pick_view_lanes(const mvsim_ctx* ctx, const int64_t dim[3], int n_views)
{
    int lanes = ctx->opt.view_lanes;
    if (lanes <= 0) {
        const int64_t n = dim[0] * dim[1] * dim[2];
        lanes = n <= ((int64_t)1 << 22) ? 4 : n <= ((int64_t)1 << 24) ? 2 : 1;
    }
    return std::max(1, std::min(lanes, n_views));
}

// ---- stacked views: ONE launch per stage for all V views ------------------------------------------------------------------
// A view below ~2^26 voxels is a chain of a dozen dependent launches that each leave most of the chip idle (128^3: a few hundred
// blocks per launch and ~10 us per link of the chain; 289^3: the rotate + attenuate kernel is 1 300 waves of serial latency), and the
// host needs ~5 us per launch on top.  The views of `main`'s loop are independent and alike (SimulateMultiViewDataset.java:567-585:
// same volume, same PSF size, same spacing), so their kernels take the view as one more grid dimension: the attenuated volumes, the
// spectra, the PSFs' taps and the convolved planes of the V views lie back to back in the workspaces, the passes that work on planes
// or rows (A, B, D, E, the PSF's own) simply see V times as many, and the kernels with per-view operands -- rotate + attenuate (the
// view's inverse model), the z pass (its taps, its sum), extract + Poisson (its acquisition, RNG key, adjustImage factor) -- read them
// from small device tables.  Every voxel goes through the same arithmetic in the same order as in a single view: bit-identical.
static bool views_batchable(const mvsim_ctx* ctx, const int64_t dim[3], const int64_t kdim[3], const mvsim_view_params* params,
                            const mvsim_view_outputs* outs, int n_views)
{
    if (n_views < 2 || ctx->opt.view_batch == 0 || ctx->opt.graph || ctx->opt.rocfft) return false;
    const int64_t n = nvox(dim);
    if (ctx->opt.view_batch == 2 && n > ((int64_t)1 << 26)) return false;            // auto: views that fill the chip by themselves stay single
    if ((size_t)n * n_views * sizeof(float) > ((size_t)24 << 30)) return false;      // the stacked workspaces are ~6 x this
    const mvsim_view_params& p0 = params[0];
    if (pick_method(p0.conv_method, kdim) != 1 || !custom_fft_batchable(ctx, dim, kdim)) return false;
    const bool noise = p0.snr >= 0.0f;
    if (noise && ctx->opt.poisson_queue != 1) return false;
    for (int v = 0; v < n_views; ++v) {
        const mvsim_view_params& p = params[v];
        if (p.axis != 0 || p.delta != p0.delta || p.inc != p0.inc || p.snr != p0.snr || p.min_value != p0.min_value ||
            p.target_average != p0.target_average || pick_method(p.conv_method, kdim) != 1)
            return false;
        if (outs[v].rot || outs[v].att || outs[v].con) return false;                   // intermediates on request: the single-view path
        double m[12];
        Affine inv;
        axis_rotation_host(dim, 0, p.degrees, m);
        affine_invert_host(m, inv.m);
        if (!affine_is_x_rotation(inv)) return false;
    }
    return true;
}

static int views_enqueue_batched(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* const* psf_host, const int64_t kdim[3],
                                 const mvsim_view_params* params, const mvsim_view_outputs* outs, int V)
{
    const int64_t n = nvox(dim), k3 = kdim[0] * kdim[1] * kdim[2];
    const mvsim_view_params& p0 = params[0];
    const bool noise = p0.snr >= 0.0f;
    const int64_t nzo = mvsim_extract_nz(dim[2], p0.inc), plane_vox = dim[0] * dim[1];
    ev_next(ctx);
    ctx->psf_entry = nullptr;                              // stacked views: V PSFs in one G2, no PSF cache
    // one upload for everything the views bring: [V inverse models][V extract tables][V normalised PSFs]
    const size_t tab_a = (size_t)V * sizeof(Affine), tab_e = (size_t)V * sizeof(ExtractView);
    const size_t off_e = (tab_a + 255) & ~(size_t)255, off_p = (off_e + tab_e + 255) & ~(size_t)255;
    const size_t up_bytes = off_p + (size_t)V * k3 * sizeof(float);
    MVSIM_TRY(ctx->view_tab.reserve(up_bytes));
    MVSIM_TRY(ctx->vol_b.reserve((size_t)V * n * sizeof(float)));                       // att[v]
    const int zstride = p0.inc > 1 ? p0.inc : 1;                                        // (as view_enqueue: only the planes extractSlices reads)
    const int64_t con_planes = zstride > 1 ? nzo : dim[2];
    MVSIM_TRY(ctx->vol_a.reserve((size_t)V * plane_vox * con_planes * sizeof(float)));  // con[v]
    float* con = ctx->vol_a.as<float>();
    bool vec_all = true;
    for (int v = 0; v < V; ++v)
        vec_all = vec_all && ((reinterpret_cast<uintptr_t>(con + (size_t)v * plane_vox * con_planes) | reinterpret_cast<uintptr_t>(outs[v].acq)) % 16 == 0);
    ExtractPlan xpl;                                                                    // `con` holds the acquired planes only where zstride > 1
    ExtractOps xops;
    xops.nviews = V; xops.adjust = true; xops.min_value = p0.min_value; xops.noise = noise; xops.mul = mvsim_poisson_mul((double)p0.snr);
    MVSIM_TRY(extract_stage_plan(ctx, zstride > 1 ? ExtractGeom::compact(dim, p0.inc) : ExtractGeom::strided(dim, p0.inc), xops, &xpl, vec_all));
    double *partial, *scal0;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal0));
    int slot = 0;
    MVSIM_TRY(ctx->pinned.acquire(up_bytes, &slot));
    char* hp = reinterpret_cast<char*>(ctx->pinned.p[slot]);
    char* dp = ctx->view_tab.as<char>();
    Affine* atab = reinterpret_cast<Affine*>(hp);
    ExtractView* etab = reinterpret_cast<ExtractView*>(hp + off_e);
    for (int v = 0; v < V; ++v) {
        double m[12];
        axis_rotation_host(dim, 0, params[v].degrees, m);
        affine_invert_host(m, atab[v].m);
        ExtractView& e = etab[v];
        e.in = con + (size_t)v * plane_vox * con_planes;
        e.out = outs[v].acq;
        e.scal = scal_of(ctx, v);
        const QueueLayout::Region q = xpl.layout.region(noise ? ctx->pqueue.p : nullptr, v);
        e.queue = q.items; e.qcount = q.counts;
        e.k0 = (uint32_t)params[v].seed; e.k1 = (uint32_t)(params[v].seed >> 32); e.stream = params[v].stream; e.pad = 0;
    }
    // Tools.normImage of the V PSFs (in place, Q5) and their copy into the upload block: one host thread per view -- a 51^3 stack is 0.13 ms of
    // summation and division, and nothing reaches the GPU before the last of them is done
    //  -- unless two views name the same (or overlapping) PSF memory, e.g. `[psf] * 8`: n sequential calls normalise that buffer n
    // times one after the other, and so does this: in view order on the calling thread, each view taking the taps as they are at its turn
    auto psf_stage = [&](int v) {
        psf_normalise_host(psf_host[v], k3);
        std::memcpy(hp + off_p + (size_t)v * k3 * sizeof(float), psf_host[v], (size_t)k3 * sizeof(float));
    };
    bool psf_aliased = false;
    for (int v = 0; v < V && !psf_aliased; ++v)
        for (int w = v + 1; w < V; ++w) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(psf_host[v]), b = reinterpret_cast<uintptr_t>(psf_host[w]);
            const uintptr_t len = (uintptr_t)k3 * sizeof(float);
            if (a < b + len && b < a + len) { psf_aliased = true; break; }
        }
    if (psf_aliased) for (int v = 0; v < V; ++v) psf_stage(v);
    else HostPool::get().run(V, host_threads_of(ctx), psf_stage);
    MVSIM_HIP(hipMemcpyAsync(dp, hp, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    MVSIM_HIP(hipEventRecord(ctx->pinned.ev[slot], ctx->stream));
    ctx->pinned.busy[slot] = true;

    ev_begin(ctx, ST_ROTATE);
    MVSIM_TRY(launch_rotate_attenuate_views(ctx->stream, gt, ctx->vol_b.as<float>(), dim, reinterpret_cast<const Affine*>(dp), V, p0.delta));
    ev_end(ctx, ST_ROTATE);

    ConvTail tail;
    tail.views = V;
    tail.zstride = zstride;
    tail.corr_n = n; tail.min_value = p0.min_value; tail.target_average = p0.target_average;
    int64_t P[3];
    if (!custom_fft_sizes(dim, kdim, P, ctx->opt)) { set_error("stacked views: no hand-written FFT size"); return MVSIM_EINVAL; }
    MVSIM_TRY(custom_fft_convolve(ctx, ctx->vol_b.as<float>(), dim, reinterpret_cast<const float*>(dp + off_p), kdim, con, &tail));
    if (!tail.corr_done || tail.zstride != zstride) { set_error("stacked views: the convolution did not deliver the factors / planes asked for"); return MVSIM_EHIP; }

    xops.vt = reinterpret_cast<const ExtractView*>(dp + off_e);
    return extract_stage_run(ctx, xpl, xops);
}

int mvsim_simulate_views_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* const* psf_host, const int64_t kdim[3],
                             const mvsim_view_params* params, const mvsim_view_outputs* outs, int n_views)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(gt && psf_host && kdim && params && outs, "null pointer");
    MVSIM_CHECK_ARG(n_views >= 0 && n_views <= MVSIM_MAX_VIEWS, "n_views must be in [0, MVSIM_MAX_VIEWS]");
    MVSIM_CHECK_ARG(!ctx->is_lane, "a lane context cannot fan out itself");
    const int64_t n = nvox(dim);
    const size_t vbytes = (size_t)n * sizeof(float);
    for (int v = 0; v < n_views; ++v) {
        const mvsim_view_params* p = &params[v];
        MVSIM_CHECK_ARG(psf_host[v] != nullptr, "null PSF");
        MVSIM_CHECK_ARG(outs[v].acq != nullptr, "outputs.acq is required");
        MVSIM_CHECK_ARG(p->axis >= 0 && p->axis <= 2, "axis must be 0, 1 or 2");
        MVSIM_CHECK_ARG(p->inc >= 1, "inc must be >= 1");
        MVSIM_CHECK_ARG(p->conv_method >= 0 && p->conv_method <= 2, "conv_method must be 0, 1 or 2");
    }
    MVSIM_CHECK_ARG(dim[0] <= dim[1], "attenuate3d: Nx > Ny walks outside the interval in the reference");
    // views that run side by side must not write what another one reads or writes (sequential calls would order them)
    {
        struct Range { const char* lo; const char* hi; };
        std::vector<Range> w;
        for (int v = 0; v < n_views; ++v) {
            const size_t abytes = (size_t)(dim[0] * dim[1] * mvsim_extract_nz(dim[2], params[v].inc)) * sizeof(float);
            const float* ptr[4] = {outs[v].rot, outs[v].att, outs[v].con, outs[v].acq};
            for (int a = 0; a < 4; ++a)
                if (ptr[a]) w.push_back(Range{reinterpret_cast<const char*>(ptr[a]), reinterpret_cast<const char*>(ptr[a]) + (a == 3 ? abytes : vbytes)});
        }
        bool meet = false;
        for (size_t i = 0; i < w.size() && !meet; ++i) {
            meet = ranges_meet(gt, vbytes, w[i].lo, w[i].hi);
            for (size_t j = i + 1; j < w.size() && !meet; ++j) meet = w[i].lo < w[j].hi && w[j].lo < w[i].hi;
        }
        MVSIM_CHECK_ARG(!meet, "simulate_views: output buffers overlap each other or the ground truth");
    }
    if (views_batchable(ctx, dim, kdim, params, outs, n_views)) {
        const int rc = views_enqueue_batched(ctx, gt, dim, psf_host, kdim, params, outs, n_views);
        ev_rebalance(ctx);
        return rc;
    }
    const int nl = pick_view_lanes(ctx, dim, n_views);
    if (nl <= 1) {
        for (int v = 0; v < n_views; ++v) MVSIM_TRY(mvsim_simulate_view_dev(ctx, gt, dim, psf_host[v], kdim, &params[v], &outs[v], nullptr));
        return MVSIM_OK;
    }
    while ((int)ctx->lanes.size() < nl) {
        // the event first: lanes and lane_done grow together or not at all
        hipEvent_t e = nullptr;
        MVSIM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        mvsim_ctx* lane = nullptr;
        const int lrc = mvsim_create(ctx->device, &lane);
        if (lrc != MVSIM_OK) { (void)hipEventDestroy(e); return lrc; }
        lane->is_lane = true;
        ctx->lanes.push_back(lane);
        ctx->lane_done.push_back(e);
    }
    if (!ctx->ev_lane_fork) MVSIM_HIP(hipEventCreateWithFlags(&ctx->ev_lane_fork, hipEventDisableTiming));
    // fork: nothing a lane enqueues may overtake what this context's stream holds (the ground truth's producer, say)
    MVSIM_HIP(hipEventRecord(ctx->ev_lane_fork, ctx->stream));
    for (int l = 0; l < nl; ++l) {
        mvsim_ctx* lane = ctx->lanes[(size_t)l];
        lane->opt = ctx->opt;
        lane->opt.tail_overlap = 0; lane->opt.graph = 0; lane->opt.view_lanes = 1;
        MVSIM_HIP(hipStreamWaitEvent(lane->stream, ctx->ev_lane_fork, 0));
    }
    int rc = MVSIM_OK;
    for (int v = 0; v < n_views && rc == MVSIM_OK; ++v) {
        mvsim_ctx* lane = ctx->lanes[(size_t)(v % nl)];
        rc = psf_prepare(lane, psf_host[v], kdim, dim, false);        // lanes: small views side by side, each lane a context of its own -- no PSF cache
        if (rc == MVSIM_OK) rc = view_enqueue(lane, gt, dim, kdim, &params[v], &outs[v], false);
        ev_rebalance(lane);
    }
    // join -- also after a failure: whatever was enqueued is ordered in front of this context's next work
    for (int l = 0; l < nl; ++l) {
        mvsim_ctx* lane = ctx->lanes[(size_t)l];
        if (hipEventRecord(ctx->lane_done[(size_t)l], lane->stream) != hipSuccess ||
            hipStreamWaitEvent(ctx->stream, ctx->lane_done[(size_t)l], 0) != hipSuccess) {
            if (rc == MVSIM_OK) { set_error("simulate_views: joining lane %d failed", l); rc = MVSIM_EHIP; }
        }
    }
    return rc;
}

int mvsim_simulate_iteration_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* psf_host, const int64_t kdim[3],
                                 const mvsim_view_params* p, int back_degrees, const mvsim_view_outputs* o,
                                 const mvsim_iteration_outputs* more)
{
    MVSIM_CHECK_ARG(ctx && more, "null pointer");
    MVSIM_TRY(simulate_view_dev(ctx, gt, dim, psf_host, kdim, p, o, nullptr, more->view_psf != nullptr));
    MVSIM_TRY(set_device(ctx));                            // the rest reads the acquisition: a pending tail runs first
    Affine inv;
    double m[12];
    if (more->iso || more->view) {
        const int64_t adim[3] = {dim[0], dim[1], mvsim_extract_nz(dim[2], p->inc)};
        const int64_t idim[3] = {dim[0], dim[1], mvsim_isotropic_nz(adim[2], p->inc)};
        float* iso = more->iso;
        if (!iso) { MVSIM_TRY(ctx->vol_c.reserve((size_t)(idim[0] * idim[1] * idim[2]) * sizeof(float))); iso = ctx->vol_c.as<float>(); }
        MVSIM_CHECK_ARG(iso != more->view, "iso and view must be different buffers");
        MVSIM_TRY(launch_make_isotropic(ctx->stream, o->acq, iso, adim, p->inc));
        if (more->view) {
            axis_rotation_host(idim, p->axis, back_degrees, m);
            affine_invert_host(m, inv.m);
            MVSIM_TRY(launch_rotate(ctx->stream, iso, more->view, idim, inv));
        }
    }
    if (more->view_weights) {
        if (ctx->weight_dim[0] != dim[0] || ctx->weight_dim[1] != dim[1] || ctx->weight_dim[2] != dim[2] || !ctx->weight_img.p) {
            MVSIM_TRY(ctx->weight_img.reserve((size_t)nvox(dim) * sizeof(float)));
            MVSIM_TRY(launch_weight_image(ctx->stream, ctx->weight_img.as<float>(), dim));
            for (int d = 0; d < 3; ++d) ctx->weight_dim[d] = dim[d];
        }
        axis_rotation_host(dim, p->axis, back_degrees, m);
        affine_invert_host(m, inv.m);
        MVSIM_TRY(launch_rotate(ctx->stream, ctx->weight_img.as<float>(), more->view_weights, dim, inv));
    }
    if (more->view_psf) {
        // psf_dev holds the normalised PSF this view was convolved with (psf_prepare)
        axis_rotation_host(kdim, p->axis, back_degrees, m);
        affine_invert_host(m, inv.m);
        MVSIM_TRY(launch_rotate(ctx->stream, ctx->psf_dev.as<float>(), more->view_psf, kdim, inv));
    }
    return MVSIM_OK;
}

// ---- z-slab tiling of one view (BASELINE configs[3]/[4]) ------------------------------------------------
int mvsim_slab_range(int64_t nz, int nranks, int rank, int64_t* z0, int64_t* z1)
{
    if (nz < 1 || nranks < 1 || rank < 0 || rank >= nranks || !z0 || !z1) {
        set_error("invalid argument: slab range");
        return MVSIM_EINVAL;
    }
    *z0 = nz * rank / nranks;
    *z1 = nz * (rank + 1) / nranks;
    return MVSIM_OK;
}

// rotate + attenuate the slab's planes and the halo the PSF reaches, convolve the slab; the slab's share of adjustImage's sum is left in
// the context's scalar slot (device).  Nothing here waits for the device.
static int slab_convolve_enqueue(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* psf_host,
                                 const int64_t kdim[3], const mvsim_view_params* p, int64_t z0, int64_t z1)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(gt && p, "null pointer");
    MVSIM_CHECK_ARG(p->axis == 0, "slab tiling supports rotation about x (axis 0)");
    MVSIM_CHECK_ARG(dim[0] <= dim[1], "attenuate3d: Nx > Ny walks outside the interval in the reference");
    MVSIM_CHECK_ARG(0 <= z0 && z0 < z1 && z1 <= dim[2], "slab must satisfy 0 <= z0 < z1 <= Nz");
    MVSIM_CHECK_ARG(kdim && kdim[2] >= 1 && kdim[2] <= 64, "slab tiling needs a PSF depth <= 64 (direct z pass)");
    const int64_t nz = dim[2], kz = kdim[2], c = kz / 2, hl = kz - 1 - c;
    // planes the taps of the slab's outputs reach: [z0 - hl, z1 - 1 + c], folded back at the global faces
    int64_t za = z0 - hl, zb = z1 + c;                     // [za, zb)
    if (za < 0) { zb = std::max<int64_t>(zb, std::min<int64_t>(nz, -za + 1)); za = 0; }
    if (zb > nz) { za = std::min<int64_t>(za, std::max<int64_t>(0, 2 * nz - 1 - zb)); zb = nz; }
    int64_t P[3];
    if (!custom_fft_sizes(dim, kdim, P, ctx->opt)) {
        set_error("slab tiling: no hand-written FFT size for this volume / PSF");
        return MVSIM_EINVAL;
    }
    const size_t pbytes = (size_t)dim[0] * dim[1] * sizeof(float);
    MVSIM_TRY(ctx->vol_a.reserve(pbytes * (size_t)(z1 - z0)));
    MVSIM_TRY(psf_prepare(ctx, psf_host, kdim, dim, false));          // a z slab: not a whole view, no PSF cache
    double m[12];
    Affine inv;
    axis_rotation_host(dim, p->axis, p->degrees, m);
    affine_invert_host(m, inv.m);
    // (round 6) the slab's planes through the fused rotate + attenuate + x-transform kernel, as an untiled view's: the attenuated planes
    // never cross HBM (z_first = za, zb - za planes; F holds them from plane 0, where pass B of the slab's convolution expects them)
    bool x_done = false;
    ev_begin(ctx, ST_ROTATE);
    MVSIM_TRY(rotate_attenuate_fftx(ctx, gt, nullptr, nullptr, dim, kdim, inv, p->delta, &x_done, nullptr, (int)za, (int)(zb - za)));
    if (!x_done) {
        MVSIM_TRY(ctx->vol_b.reserve(pbytes * (size_t)(zb - za)));
        bool fused = false;
        MVSIM_TRY(launch_rotate_attenuate_planes(ctx->stream, gt, nullptr, ctx->vol_b.as<float>(), dim, inv, p->delta,
                                                 (int)za, (int)(zb - za), ctx->opt.fused_rotate == 2 ? 2 : 1, &fused));   // planes [za, zb) exist only fused
        if (!fused) {
            set_error("slab tiling needs the fused rotate+attenuate kernel");
            return MVSIM_EINVAL;
        }
    }
    ev_end(ctx, ST_ROTATE);
    const SlabRange slab{(int)za, (int)(zb - za), (int)z0, (int)(z1 - z0)};
    // a slab that starts at a multiple of the view's spacing convolves along z -- and sends through passes D and E -- only the planes
    // extractSlices reads, like an untiled compact view (the sum over ALL of the slab's planes comes from the z pass's input rows)
    ConvTail tail;
    tail.zstride = (p->inc > 1 && z0 % p->inc == 0) ? p->inc : 1;
    tail.x_done = x_done;
    ctx->slab_z0 = ctx->slab_z1 = -1;
    MVSIM_TRY(custom_fft_convolve_slab(ctx, x_done ? nullptr : ctx->vol_b.as<float>(), dim, ctx->psf_dev.as<float>(), kdim, slab,
                                       ctx->vol_a.as<float>(), &tail));
    ctx->slab_z0 = z0; ctx->slab_z1 = z1; ctx->slab_zstride = tail.zstride;
    return MVSIM_OK;
}

int mvsim_view_slab_convolve_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* psf_host,
                                 const int64_t kdim[3], const mvsim_view_params* p, int64_t z0, int64_t z1,
                                 double* slab_sum)
{
    MVSIM_CHECK_ARG(ctx != nullptr && slab_sum != nullptr, "null pointer");
    MVSIM_TRY(slab_convolve_enqueue(ctx, gt, dim, psf_host, kdim, p, z0, z1));
    double *partial, *scal;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
    MVSIM_HIP(hipMemcpyAsync(slab_sum, scal, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

// adjust with the sum the context's scalar slot holds (the view's, once reduced), extract, Poisson: the slab's acquired planes
static int slab_finish_enqueue(mvsim_ctx* ctx, const int64_t dim[3], const mvsim_view_params* p, int64_t z0, int64_t z1, float* acq,
                               int64_t* n_planes)
{
    double *partial, *scal;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
    MVSIM_TRY(launch_adjust_corr(ctx->stream, scal, nvox(dim), p->min_value, p->target_average));
    // compact slab: vol_a holds the planes z0 + k * inc alone, in order (z0 is a multiple of inc)
    const ExtractGeom g = ExtractGeom::slab(dim, p->inc, z0, z1, ctx->slab_zstride > 1);
    if (n_planes) *n_planes = g.nzo;
    if (g.nzo == 0) return MVSIM_OK;
    ExtractOps ops;
    ops.in = ctx->vol_a.as<float>(); ops.out = acq; ops.scal = scal;
    ops.adjust = true; ops.min_value = p->min_value; ops.noise = p->snr >= 0.0f; ops.mul = mvsim_poisson_mul((double)p->snr);
    ops.seed = p->seed; ops.stream = p->stream;
    return extract_stage(ctx, g, ops);
}

int mvsim_view_slab_finish_dev(mvsim_ctx* ctx, const int64_t dim[3], const mvsim_view_params* p, int64_t z0,
                               int64_t z1, double total_sum, float* acq, int64_t* n_planes)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(p && acq, "null pointer");
    MVSIM_CHECK_ARG(0 <= z0 && z0 < z1 && z1 <= dim[2], "slab must satisfy 0 <= z0 < z1 <= Nz");
    MVSIM_CHECK_ARG(p->inc >= 1, "inc must be >= 1");
    const int64_t plane = dim[0] * dim[1];
    MVSIM_CHECK_ARG(ctx->slab_z0 == z0 && ctx->slab_z1 == z1 && ctx->vol_a.bytes >= (size_t)(plane * (z1 - z0)) * sizeof(float),
                    "no convolved slab [z0, z1) in this context (mvsim_view_slab_convolve_dev first)");
    MVSIM_CHECK_ARG(ctx->slab_zstride == 1 || ctx->slab_zstride == p->inc, "the slab was convolved for another spacing");
    double *partial, *scal;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
    MVSIM_HIP(hipMemcpyAsync(scal, &total_sum, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));          // total_sum lives on the caller's stack
    return slab_finish_enqueue(ctx, dim, p, z0, z1, acq, n_planes);
}

// One tiled view's slab in ONE call, nothing through the host (round 6): the slab's share of adjustImage's sum stays on the device, is
// reduced over the ranks in place -- on THIS context's stream, by the communicator of `comm_ctx` (null: this context's own; a context
// without one, or a job of one rank, reduces nothing) -- and the adjusted, extracted, sampled planes follow behind it.  Asynchronous.
int mvsim_view_slab_dev(mvsim_ctx* ctx, mvsim_ctx* comm_ctx, const float* gt, const int64_t dim[3], float* psf_host,
                        const int64_t kdim[3], const mvsim_view_params* p, int64_t z0, int64_t z1, float* acq, int64_t* n_planes)
{
    MVSIM_CHECK_ARG(ctx != nullptr && p != nullptr && acq != nullptr, "null pointer");
    MVSIM_CHECK_ARG(p->inc >= 1, "inc must be >= 1");
    MVSIM_TRY(slab_convolve_enqueue(ctx, gt, dim, psf_host, kdim, p, z0, z1));
    double *partial, *scal;
    MVSIM_TRY(scal_ptr(ctx, &partial, &scal));
    mvsim_ctx* cc = comm_ctx ? comm_ctx : ctx;
    MVSIM_CHECK_ARG(cc->device == ctx->device, "the communicator's context lives on another device");
    MVSIM_TRY(comm_allreduce_f64_on_stream(cc, scal, ctx->stream));
    return slab_finish_enqueue(ctx, dim, p, z0, z1, acq, n_planes);
}

}  // extern "C"
