// Internal declarations shared by the libmvsim translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>
#include <roctracer/roctx.h>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <type_traits>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/mvsim.h"
#include "extract_plan.h"
#include "interval_plan.h"
#include "psf_cache.h"
#include "rotate_dev.h"
#include "sphere_walk.h"

// Attribution switches (tools/attribute_flags.sh, attribute_valu.sh, attribution_run.sh: builds that compile a part of a kernel's work
// OUT -- and with it the correctness of the results -- to see what that part costs; the figures are in profiles/r04_attribution.txt).
// They exist only in a build that defines MVSIM_DEV_ATTRIBUTION, which multiview-simulation_amd/build.py never does: in the product
// build none of the names below can be defined, whatever MVSIM_EXTRA_CFLAGS carries.
#ifndef MVSIM_DEV_ATTRIBUTION
#undef MVSIM_EXP_ROTFFT_NOFFT
#undef MVSIM_EXP_ROTFFT_NOBLEND
#undef MVSIM_EXP_NOEXACT
#undef MVSIM_EXP_NOPHILOX
#undef MVSIM_EXP_NOSMALLPUSH
#undef MVSIM_EXP_NOBRIGHT
#undef MVSIM_P1_F64
#undef MVSIM_EXP_NLZ
#undef MVSIM_EXP_LINES_STAMPS
#endif

namespace mvsim {

void set_error(const char* fmt, ...);

#define MVSIM_HIP(expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            mvsim::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,   \
                             __LINE__);                                                         \
            return (e_ == hipErrorOutOfMemory) ? MVSIM_ENOMEM : MVSIM_EHIP;                     \
        }                                                                                       \
    } while (0)

#define MVSIM_FFT(expr)                                                                         \
    do {                                                                                        \
        rocfft_status s_ = (expr);                                                              \
        if (s_ != rocfft_status_success) {                                                      \
            mvsim::set_error("%s failed: rocfft status %d (%s:%d)", #expr, (int)s_, __FILE__,   \
                             __LINE__);                                                         \
            return MVSIM_EFFT;                                                                  \
        }                                                                                       \
    } while (0)

#define MVSIM_TRY(expr)                                                                         \
    do {                                                                                        \
        int rc_ = (expr);                                                                       \
        if (rc_ != MVSIM_OK) return rc_;                                                        \
    } while (0)

#define MVSIM_CHECK_ARG(cond, msg)                                                              \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            mvsim::set_error("invalid argument: %s", msg);                                      \
            return MVSIM_EINVAL;                                                                \
        }                                                                                       \
    } while (0)

// Grow-only device buffer (steady state: no hipMalloc on the hot path).
struct DevBuf {
    void*  p     = nullptr;
    size_t bytes = 0;
    // allocation epoch of the owning context (null for buffers that belong to no context): bumped whenever this buffer
    // moves or goes away, so that the context's captured view graphs -- which hold raw workspace addresses -- are dropped.
    // Per context, not per process: another thread's context growing a workspace must not cost this one its graphs.
    unsigned long long* epoch = nullptr;
    int    reserve(size_t need);
    void   release();
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// device buffers that live for one call
struct Scratch {
    DevBuf b[12];
    ~Scratch() { for (DevBuf& x : b) x.release(); }
};

// Util.getSuggestedKernelDiameter (ImgLib2, recalled): max(3, 2 * (int)(3 sigma + 0.5) + 1) for sigma > 0, else 3
inline int suggested_kernel_diameter(double sigma)
{
    if (!(sigma > 0)) return 3;
    const int s = 2 * (int)(3 * sigma + 0.5) + 1;
    return s > 3 ? s : 3;
}

// struct Affine: rotate_dev.h.  A rotation about x (the only axis SimulateMultiViewDataset.main uses, :557,:570,:591): the
// inverse model has row 0 = (1,0,0,0) exactly and no x term in rows 1 and 2 -- what every row-walking rotate kernel requires
inline bool affine_is_x_rotation(const Affine& a)
{
    return a.m[0] == 1.0 && a.m[1] == 0.0 && a.m[2] == 0.0 && a.m[3] == 0.0 && a.m[4] == 0.0 && a.m[8] == 0.0;
}

struct FftPlan {
    int64_t      P[3]      = {0, 0, 0};
    rocfft_plan  fwd       = nullptr;   // real P^3 -> complex (Px/2+1) Py Pz
    rocfft_plan  inv       = nullptr;   // complex -> real
    rocfft_execution_info info = nullptr;
    size_t       work_bytes = 0;
};

// Small ring of pinned host buffers for asynchronous H2D copies of PSFs (the caller's buffer may be
// pageable and may be reused as soon as the call returns).
struct PinnedRing {
    static constexpr int SLOTS = 4;
    void*      p[SLOTS]     = {};
    size_t     bytes[SLOTS] = {};
    hipEvent_t ev[SLOTS]    = {};
    bool       busy[SLOTS]  = {};
    int        next         = 0;
    int  acquire(size_t need, int* slot);   // waits for the slot's previous copy if still in flight
    void release_all();
};

// The 16-bit transfer of acquisitions (option acq_transfer): Poisson counts (Tools.java:84 stores them as floats) are packed to uint16 on
// the device, cross PCIe as half the bytes and are widened into the caller's buffers by the host threads -- or fetched as float32 after
// all where the device flags a value that does not survive the round trip.  One device buffer [body of view 0][body of view 1] ...
// [one flag word per view] (bodies padded to 256 bytes) and its page-locked twin; reserve -> pack per view -> fetch -> land
// (api_host.cpp).  Every step is enqueued on the stream the caller names; land() expects that stream's work to have completed.
struct CountsStaging {
    DevBuf dev;
    void*  host       = nullptr;       // page-locked twin
    size_t host_bytes = 0;
    std::vector<long long> count;      // values per view of the current call
    std::vector<size_t>    body;       // byte offset of each view's body; body[views]: the flag words
    std::vector<char>      packed;     // views pack() was called for since reserve()
    int  reserve(const long long* counts, int views);
    int  pack(hipStream_t s, int view, const float* src);          // the first pack() of a call clears the flags
    int  fetch(hipStream_t s);                                     // ONE transfer: every body and the flags
    // every packed view: flag test, statistics, float32 fallback from src_dev[view], or widening into dst_host[view] (one pool job)
    int  land(mvsim_ctx* ctx, const float* const* src_dev, float* const* dst_host);
    void release();
};

// Run-time switches of a context.  Defaults come from the environment, read ONCE per process (env_options); the tests
// reach every code path through mvsim_set_option.  Nothing on a launch path calls getenv.
struct Options {
    int     zpass = 0;                 // z pass of the hand-written convolution: 0 auto, 1 direct Kz-tap convolution (Kz <= 64), 2 FFT on a
                                       // z-padded spectrum, 3 FFT inline: no z padding, mirrored planes through the index map, the PSF's z
                                       // spectrum computed per tile (k_fft_lines<CONVZ>); auto: inline from MVSIM_ZINLINE_MIN_KZ taps up, else direct
    bool    rocfft = false;            // library fallback instead of the hand-written passes
    int     fused_rotate = 3;          // rotate+attenuate as one kernel when the rotation is about x: 0 off, 1 row geometry
                                       // shared through LDS, 2 recomputed per lane (kept for A/B runs), 3 auto (production):
                                       // 1 when the view has >= 2 waves per SIMD of columns to walk or the separate rotate
                                       // cannot use 16-byte rows (Nx % 4 != 0), else 0 -- one lane walks
                                       // one (x, z) column, so a 128^3 view is 256 waves of serial latency (measured 30 us
                                       // against 20 us for the two kernels; break-even at 256^3)
    int     fused_fftx = 2;            // rotate + attenuate + the convolution's x transform as ONE kernel in the per-view pipeline
                                       // (rotate_fft.hip; `att` crosses HBM only when requested): 0 off, 1 whenever the geometry
                                       // allows (every wave walks and transforms), 2 auto (production): from 131072 columns up, like
                                       // fused_rotate, with the block's waves split into walkers and transformers where rows have at most
                                       // 512 voxels, 3 "roles": that kernel whenever the geometry allows
    bool    attenuate_scan = false;    // attenuate3d (stage operator) as a wavefront prefix scan along y: re-associates the
                                       // fp64 products (float outputs differ from the serial walk by one ulp on < 1e-6 of the voxels)
    int     poisson_queue = 1;         // 1: two-launch Poisson (streaming kernel with wave-level compaction + work-queue
                                       // resolver, production), 0: one kernel
    int     poisson_queue_share = 16;  // sixteenths of a block's voxels its queue segment holds.  16 (default): every voxel, 16 B per acquired
                                       // voxel (2.25 GiB at 512^3, 34 GB at 2048^2 x 512), nothing is ever refused and phase 1 appends without
                                       // looking.  1..15: smaller segments; the appends check for room (+0.03 ms per 512^3 view) and what a full
                                       // segment refuses is sampled where it stands by a third kernel, same counts (k_poisson_refused).  0 =
                                       // "auto": 16 for queues of up to 64 MiB, else 5 (0.70 GiB at 512^3) and growing to what the context's
                                       // views turn out to need (the phantom: 3, a volume without an empty voxel: 12)
    bool    early_sum = true;          // adjustImage's sum from the spectrum side (pass C epilogue) so that pass E can adjust
    int     exp = 0;                   // experiment bits for A/B runs on one box (tools/): 1 = z pass tiles in plain grid order, 2 = k_zconv_strided wherever its
                                       // geometry allows (without the cost rule of zconv_strided_chunk), 4 = the 8-column tiles of the long y / z lines
                                       // in plain grid order (the two tiles of a 128-byte line on different XCDs, as before round 6),
                                       // 8 = the image's y passes on lines of one block per CU (L >= 1280) as ONE transform (k_fft_lines) instead of two half-length phases (k_fft_lines_split)
    bool    zconv_strided = true;      // views that only return the acquisition (compact planes, inc > 1): the direct z pass computes the
                                       // planes k * inc alone (k_zconv_strided: 1 / inc of the taps' work) and takes adjustImage's sum from
                                       // its INPUT rows (the sum over all planes is a linear functional of them); 0: every plane, as round 3
    bool    psf_overlap = true;        // PSF spectrum on the context's side stream, concurrent with passes A and B (views of
                                       // >= 2^24 voxels; +1 % views/s at 512^3).  On by default since round 3 (bit-identical, tested);
                                       // overlapped kernels share the chip, so their own durations in a profile no longer add up to
                                       // the stage time: profiles and bench.py's roofline leg switch both overlaps off
    int     tail_overlap = 1;          // extract + Poisson of a view concurrent with the next view's rotate+attenuate (device
                                       // views of >= 2^24 voxels; measured +0..6 % views/s at 512^3 depending on the box -- the two
                                       // stages then share the chip, so their own HIP-event times grow while the convolution
                                       // between them is undisturbed): 0 off, 1 on the context's own stream only (nothing outside
                                       // the library can observe the difference), 2 also on a caller's stream (the caller
                                       // calls mvsim_join / any entry point before its stream touches the outputs)
    bool    fuse_tail = false;         // adjust + extract + Poisson phase 1 in the epilogue of the convolution's last pass: saves
                                       // the 8 N bytes of the convolved volume's round trip, but the merged kernel is bound by
                                       // vector issue (0.61 ms against 0.25 + 0.36 ms for pass E and the streaming Poisson kernel
                                       // at 512^3): measured neutral to slightly slower, so off by default
    int     graph = 0;                 // replay simulate_view_dev from a captured hipGraph (small, launch-bound volumes)
    int     acq_u16 = 1;               // host-buffer views (mvsim_simulate_view_async): the acquisition crosses PCIe as uint16 counts when the
                                       // view is sampled (snr >= 0), widened on the host; automatic float32 fallback per view.  0: always float32
    int     host_threads = 0;          // threads of the host-side widening (0 = auto: min(16, hardware threads))
    int     view_lanes = 0;            // mvsim_simulate_views_dev: views in flight side by side (0 = auto: from the size of a view)
    int     view_batch = 2;            // mvsim_simulate_views_dev: the views STACKED -- one launch per stage for all of them (api_view.cpp:
                                       // views_enqueue_batched): 0 never, 1 whenever the views allow it, 2 auto (views of <= 2^26 voxels)
    bool    bcast_ring = false;        // ground-truth broadcast as one ncclBroadcast instead of scatter + all-gather
    bool    bcast_peer_copy = false;   // ... or as copy-engine transfers between IPC-mapped buffers (comm.cpp: bcast_peer_copy)
    bool    bcast_pipelined = false;   // ... or the pipelined form: the root scatters the WHOLE volume as nranks - 1 chunks while the peers all-gather
                                       // the pieces that have arrived among themselves (mvsim_comm_broadcast_plan; comm.cpp: bcast_pipelined)
    int64_t fft_pad[3] = {0, 0, 0};    // explicit padded sizes on the rocFFT path (0: choose)
    bool    skip_empty = true;         // convolution passes skip planes the fused rotate kernel found empty (exact; option for A/B runs)
    bool    skip_rows = true;          // ... and, where those flags are in use, the rotate kernel does not store the rows without a non-zero
                                       // voxel and pass B does not read them (row_bits.h; exact; option for A/B runs)
    int     psf_cache = 1024;          // MiB of device memory for PSF spectra kept by content (psf_cache.h): a whole single view on the direct
                                       // z pass whose normalised PSF and geometry the context has seen uploads nothing and launches neither PSF pass
                                       // (exact: the same G2 bytes).  0: off -- every view uploads and transforms its PSF
    bool    skip_tail = true;          // ... and pass E does not store, nor phase 1 of the queue samplers read, the planes whose dilated flag is
                                       // clear (extract_plan.h: tail_sparse_ok; exact; option for A/B runs)
    int64_t beads_pair_cap = (int64_t)1 << 28;   // bead renderer and volume injection: (brick, item) pairs one chunk may bin; larger calls run in chunks (beads.hip, aberrations.hip)
    int64_t reject_batch = 0;          // rejection sampler: trials per launch (0 = auto: 4 per wanted sample, 4096 .. 2^20) (procedural.hip)
    int     dog_pass = 0;              // the DoG kernels a call launches (detect.hip): 0 both, 1 the xy kernel alone, 2 the z kernel alone -- for
                                       // timing one kernel kind (tools/bench_detect.py); only 0 leaves a valid D
    int     sphere_walk = -1;          // the java.util.Random walk over the large sphere: 0 on the host, 1 on the device (sphere_walk.hip; the host
                                       // walk where the device walk does not vouch for a case; 2: MVSIM_EINVAL there), -1 = each call's default: drawSpheres host, multiSpheres device
};
const Options& env_options();
int parse_option(Options& o, const char* name, const char* value);   // MVSIM_OK / MVSIM_EINVAL

// ST_PASS_*: the five passes of the hand-written convolution, nested inside ST_CONVOLVE (not part of the stage sum)
enum Stage { ST_ROTATE = 0, ST_ATTENUATE, ST_PSF, ST_CONVOLVE, ST_ADJUST, ST_EXTRACT, ST_PASS_A, ST_PASS_B, ST_PASS_C, ST_PASS_D,
             ST_PASS_E, ST_COUNT };

}  // namespace mvsim

struct mvsim_ctx {
    mvsim_ctx();
    mvsim_ctx(const mvsim_ctx&) = delete;
    mvsim_ctx& operator=(const mvsim_ctx&) = delete;
    template <class F> void each_workspace(F&& f);   // f(DevBuf&, traits) for every device workspace of the context (below)
    unsigned long long alloc_epoch = 1;     // see DevBuf::epoch
    int         roctx_depth = 0;            // stage ranges open on this context (rebalanced by every entry point after an error return)
    int         device     = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream     = nullptr;
    int         num_cu     = 256;

    // workspaces
    mvsim::DevBuf vol_a, vol_b, vol_c;      // N-sized float staging for host entry points / fused path
    mvsim::DevBuf out_buf;                  // extract output staging
    mvsim::DevBuf psf_dev;                  // K^3 floats
    mvsim::PsfCache psf_cache;              // PSF spectra by content (option psf_cache); its entries are written and read on this context's
                                            // main and side streams only
    mvsim::PsfCache::Entry* psf_entry = nullptr;   // the entry psf_prepare settled for the convolution that follows it (null: ctx->psf_dev)
    mvsim::DevBuf view_tab;                 // stacked views: [inverse models][extract tables][PSFs] of the current batch
    mvsim::DevBuf interval_tab;             // interval jobs of the current call: [IntervalView table][ExtractView table] (extract_interval.hip)
    mvsim::DevBuf stencil_psf;              // direct stencil: PSF reversed along x, rows zero-padded to 4 taps
    mvsim::PinnedRing pinned;
    mvsim::DevBuf fft_real;                 // P^3 floats
    mvsim::DevBuf fft_spec_img, fft_spec_psf;
    mvsim::DevBuf fft_work;
    mvsim::DevBuf pqueue;                   // Poisson work queue: [count][items]
    mvsim::DevBuf sphere_list;              // phantom generator: (centre, radius, value) items
    mvsim::DevBuf beads_buf[8];             // bead renderer (beads.hip): points, jobs, per-bead records, pair keys / values, sort temp, scratch
    mvsim::DevBuf proc_buf[10];             // procedural phantom (procedural.hip): Perlin tables, sphere lists and records, counts, pair keys / values,
                                            // scan / sort temp, ownership mask, sampler flags and positions
    mvsim::DevBuf walk_buf[4];              // device walk (sphere_walk.hip): event lists, chunk maps, scan results, accepted voxels
    mvsim::DevBuf plane_flags;              // per-plane non-zero flags of the current view (rotate_fft.hip -> the convolution passes)
    int*          empty_hint = nullptr;     // page-locked word the device writes: empty planes of the last view that carried flags (-1: none yet)
    unsigned int* queue_hint = nullptr;     // page-locked word the device raises: sixteenths of a block's voxels the fullest refused queue segment needed
    int           queue_share_learned = 0;  // ... as the host has seen it so far (auto share: queue_mode_next)
    int64_t       extract_path[5] = {-1, 0, 0, 0, 0};   // the sampler form of the last extract this context enqueued (mvsim_get_extract_path)
    int64_t       tail_path[2] = {0, 0};    // {the last view's tail ran in sparse mode, its flag stride} (mvsim_get_tail_path)
    int           views_since_flags = 0;    // views run WITHOUT flags since (a volume without empty planes pays nothing for the bookkeeping)
    mvsim::DevBuf weight_img;               // computeWeightImage of the last volume size (mvsim_simulate_iteration_dev)
    mvsim::DevBuf decon_work[2];            // multi-view deconvolution (api_decon.cpp): the blurred estimate / ratio, and the correlation
    mvsim::DevBuf decon_psf;                // ... every view's normalised PSF and its flipped twin, uploaded once per call
    mvsim::DevBuf decon_stat;               // ... per-block partials, per-view sums and the statistics of every step of a call
    mvsim::DevBuf detect_buf[6];            // bead detector (api_detect.cpp): the two half-blurred volumes, D, the peak list, block counts + offsets + ballots, scan temp
    mvsim::DevBuf register_buf[4];          // bead registration (api_register.cpp): the stages' lists of one whole call, split partials, per-point bests, RANSAC pairs + key + mask
    mvsim::DevBuf fuse_buf;                 // view fusion (api_fuse.cpp): the views' inverted matrices, sources and outputs of the current call
    mvsim::DevBuf psfx_buf[3];              // PSF extraction (api_psf.cpp): per-chunk partial sums, per-tap totals, status bytes
    int64_t       weight_dim[3] = {0, 0, 0};
    mvsim::DevBuf host_gt, host_rot, host_att, host_con;   // device twins of the host-buffer simulate_view (grow-only)
    mvsim::DevBuf partials;                 // doubles: block partial sums + [sum, corr]
    mvsim::DevBuf partials_e;               // per-block sums of the c2r/crop pass
    mvsim::DevBuf cfft_f, cfft_g;           // custom FFT: image / PSF half spectra [Pz][Py][Hxp]
    mvsim::DevBuf cfft_g1, cfft_g2;         // compact PSF intermediates [Kz][Ky][Hxp], [Kz][Py][Hxp]
    mvsim::Options opt;
    std::unordered_set<const void*> lds_attr_set;   // kernels whose dynamic-LDS limit has been raised on this device
    std::map<std::string, void*> box_weights;   // early-sum weights (fft_driver.hip: ensure_box_weights)
    mvsim::DevBuf partials_z;               // per-block sums of the z pass
    std::map<int, void*> twiddles;          // 2*length + kind -> device twiddle table (fft_driver.hip: ensure_twiddles)
    std::map<std::string, mvsim::FftPlan> plans;
    bool   fft_ready = false;

    // timing: a ring of event sets, one set per stage-operator / simulate_view call, so that a host can time
    // many asynchronous calls and read the averages once (mvsim_get_timings)
    static constexpr int TIMING_SLOTS = 64;
    bool       timing = false;
    hipEvent_t evr[TIMING_SLOTS][mvsim::ST_COUNT][2] = {};
    bool       ev_used[TIMING_SLOTS][mvsim::ST_COUNT] = {};
    int        ev_cur = 0;          // slot being recorded
    long long  ev_calls = 0;        // slots started since timing was enabled / last read
    bool       ev_created = false;
    mvsim_timings last = {};

    // pipelined host-buffer views (mvsim_simulate_view_async): upload(v+1) || compute(v) || download(v-1)
    static constexpr int ASYNC_SLOTS = 2, ASYNC_HISTORY = 8;
    double     async_corr_done[ASYNC_HISTORY] = {};   // adjustImage factors of the views that have landed
    hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
    // the PSF's (x,y) spectrum is independent of the image passes A and B: it runs on a side stream beside them
    hipStream_t side_stream = nullptr;
    hipEvent_t  ev_fork = nullptr, ev_join = nullptr;
    bool        psf_on_side = false;          // last convolution: PSF spectrum overlapped (its time is inside passes A/B)
    // extract + Poisson of view v ("the tail") on a stream of its own, so that the next view's rotate+attenuate -- a
    // latency-bound kernel that leaves most of the chip idle -- runs beside it.  While tail_pending, the tail's outputs are
    // NOT yet ordered on ctx->stream: join_tail() restores that and every entry point does it first (set_device).
    hipStream_t tail_stream = nullptr;
    hipEvent_t  ev_tail_fork = nullptr, ev_tail = nullptr;
    bool        tail_pending = false;
    const char *tail_lo[2] = {nullptr, nullptr}, *tail_hi[2] = {nullptr, nullptr};   // byte ranges the pending tail writes / reads
    mvsim::DevBuf async_gt[ASYNC_SLOTS], async_acq[ASYNC_SLOTS];
    // acquisitions cross PCIe as 16-bit counts: one staging per pipelined slot (landed by mvsim_wait), one for the synchronous
    // host-buffer entry points (down_counts, mvsim_simulate_views)
    mvsim::CountsStaging async_counts[ASYNC_SLOTS], sync_counts;
    float*     async_out_acq[ASYNC_SLOTS] = {};   // the caller's acquisition buffer of the slot's view
    long long  u16_views = 0, u16_fallbacks = 0;  // statistics (mvsim_get_transfer_stats)
    hipEvent_t ev_h2d[ASYNC_SLOTS] = {}, ev_compute[ASYNC_SLOTS] = {}, ev_d2h[ASYNC_SLOTS] = {};
    bool       async_inflight[ASYNC_SLOTS] = {};
    long long  async_ticket[ASYNC_SLOTS] = {};
    double*    async_corr = nullptr;          // pinned: one double per slot
    const void* async_gt_src[ASYNC_SLOTS] = {};   // host ground truth a slot holds (identity + generation: re-upload skipped)
    unsigned long long async_gt_gen[ASYNC_SLOTS] = {};
    size_t     async_gt_bytes[ASYNC_SLOTS] = {};  // bytes of that upload (a view of another size never reuses it)
    long long  async_next = 0;
    bool       async_ready = false;
    bool       async_twins_busy = false;      // the single-buffered rot/att/con twins are being downloaded

    // hipGraph replay of views (option "graph"): cache keyed by every pointer and parameter of the view
    struct ViewGraph {
        std::string    key;
        hipGraph_t     graph;
        hipGraphExec_t exec;
        unsigned long long last_use;
    };
    std::vector<ViewGraph> graphs;
    std::unordered_set<std::string> graph_seen;
    unsigned long long graph_tick = 0, graph_epoch = 0;

    // mvsim_simulate_views_dev: views that cannot fill the chip one at a time run side by side on LANES -- child contexts of this
    // one (own stream, own workspaces, same device and options), forked from and joined to this context's stream by events
    std::vector<mvsim_ctx*> lanes;
    std::vector<hipEvent_t> lane_done;
    hipEvent_t  ev_lane_fork = nullptr;
    bool        is_lane = false;

    // z-slab tiling: what mvsim_view_slab_convolve_dev left in vol_a for mvsim_view_slab_finish_dev -- the slab's planes [z0, z1), or only
    // the planes k * slab_zstride of it (compact, slab_zstride > 1: the slab starts at a multiple of the view's spacing)
    int64_t slab_z0 = -1, slab_z1 = -1;
    int     slab_zstride = 1;

    // RCCL
    void* comm = nullptr;
    void* peer_copy = nullptr;             // broadcast=peer_copy: IPC maps, copy streams (comm.cpp)
    int   nranks = 1, rank = 0;
};

// Every device workspace a context owns -- the ONE list: the constructor (allocation epoch), mvsim_destroy and mvsim_release_caches
// are written against it.  Traits say where the three have always differed:
//   WS_KEPT      partials, partials_e: mvsim_release_caches keeps them (the fixed-size scalar / partial-sum slots of PARTIALS_BYTES and
//                SUM_BLOCKS doubles, no cache that grows with a volume); mvsim_destroy frees them like everything else.
//   WS_NO_EPOCH  beads_buf, proc_buf, walk_buf: carry no allocation epoch -- no captured view graph holds an address inside the bead
//                renderer's, the procedural phantom's or the device walk's buffers.
enum { WS_KEPT = 1, WS_NO_EPOCH = 2 };
template <class F> inline void mvsim_ctx::each_workspace(F&& f)
{
    for (mvsim::DevBuf* b : {&vol_a, &vol_b, &vol_c, &out_buf, &psf_dev, &stencil_psf, &fft_real, &fft_spec_img, &fft_spec_psf, &fft_work,
                             &pqueue, &view_tab, &interval_tab, &sphere_list, &weight_img, &plane_flags, &host_gt, &host_rot, &host_att, &host_con, &cfft_f, &cfft_g,
                             &cfft_g1, &cfft_g2, &partials_z, &async_gt[0], &async_gt[1], &async_acq[0], &async_acq[1], &async_counts[0].dev,
                             &async_counts[1].dev, &sync_counts.dev, &decon_work[0], &decon_work[1], &decon_psf, &decon_stat, &fuse_buf})
        f(*b, 0);
    f(partials, WS_KEPT);
    f(partials_e, WS_KEPT);
    for (mvsim::DevBuf& b : detect_buf) f(b, 0);
    for (mvsim::DevBuf& b : register_buf) f(b, 0);
    for (mvsim::DevBuf& b : psfx_buf) f(b, 0);
    for (mvsim::DevBuf& b : beads_buf) f(b, WS_NO_EPOCH);
    for (mvsim::DevBuf& b : proc_buf) f(b, WS_NO_EPOCH);
    for (mvsim::DevBuf& b : walk_buf) f(b, WS_NO_EPOCH);
}

inline mvsim_ctx::mvsim_ctx()
{
    each_workspace([this](mvsim::DevBuf& b, int traits) { if (!(traits & WS_NO_EPOCH)) b.epoch = &alloc_epoch; });
}

namespace mvsim {

// ---- kernel launchers (each enqueues on `s`, returns MVSIM_* status) ----------------------------
int launch_rotate(hipStream_t s, const float* in, float* out, const int64_t dim[3], const Affine& inv);
int launch_attenuate(hipStream_t s, const float* in, float* out, const int64_t dim[3], double delta);
int launch_attenuate_scan(hipStream_t s, const float* in, float* out, const int64_t dim[3], double delta);
int launch_rotate_attenuate(hipStream_t s, const float* in, float* rot_or_null, float* att, const int64_t dim[3],
                            const Affine& inv, double delta, int fused_mode, bool* fused);
int launch_rotate_attenuate_planes(hipStream_t s, const float* in, float* rot_or_null, float* att, const int64_t dim[3],
                                   const Affine& inv, double delta, int z_begin, int z_count, int fused_mode, bool* fused);
// sum -> scal[0]; partial workspace must hold >= SUM_BLOCKS doubles
constexpr int SUM_BLOCKS = 2048;
int launch_sum(hipStream_t s, const float* in, int64_t n, double* partial, double* scal);
// scal[1] = (double)(target - min) / (scal[0] / n)
int launch_adjust_corr(hipStream_t s, double* scal, int64_t n, float min_value, float target);
int launch_adjust_apply(hipStream_t s, float* img, int64_t n, const double* scal, float min_value);
int launch_norm_apply(hipStream_t s, float* img, int64_t n, const double* scal);
// ---- extract (+ adjust using scal[1]) (+ Poisson): extract.hip runs what extract_plan.h plans
struct ExtractView {              // per-view operands of the extract + Poisson kernels (device table)
    const float*  in;             // the view's convolved planes
    float*        out;            // its acquisition
    const double* scal;           // its [sum, adjustImage factor]
    void*         queue;          // its Poisson work-queue segments (PItem) ...
    unsigned int* qcount;         // ... and their counters
    uint32_t      k0, k1, stream, pad;
};
struct ExtractOps {               // the operands of one launch_extract
    const float*  in = nullptr;   // the buffer the planes are read from (ExtractGeom::in_offset voxels in), the acquisition, the
    float*        out = nullptr;  // [sum, adjustImage factor] pair and the queue workspace (QueueLayout) ...
    const double* scal = nullptr;
    void*         queue_ws = nullptr;
    const ExtractView* vt = nullptr;   // ... or those of `nviews` stacked views, with their RNG keys, from a device table (blockIdx.y = view)
    int           nviews = 0;
    bool          adjust = false, noise = false;
    float         min_value = 0.f;
    double        mul = 0.0;
    uint64_t      seed = 0;       // the RNG key and stream of the launch
    uint32_t      stream = 0;
    // sparse tail (ConvTail::sparse): pass E has NOT written the planes of `in` whose flag is clear -- plane j of the buffer is flag
    // empty_flags[j * empty_stride], so output plane k reads flag k * ExtractGeom::inc * empty_stride (extract_plan.h:
    // tail_flag_of_output) -- and phase 1 must not read them.  Only the two queue samplers take it; launch_extract refuses every other form
    const int*    empty_flags = nullptr;
    int           empty_stride = 0;
};
int launch_extract(hipStream_t s, const ExtractPlan& pl, const ExtractOps& o);
int launch_resolve(hipStream_t s, const ExtractPlan& pl, const ExtractOps& o);   // the sampler's second launch alone (the fused tail)
// run-time flags -> a kernel's template arguments (the launchers of extract.hip and extract_interval.hip)
template <class F> inline void dispatch1(bool a, F&& f)
{
    if (a) f(std::true_type{}); else f(std::false_type{});
}
template <class F> inline void dispatch2(bool a, bool b, F&& f)
{
    dispatch1(a, [&](auto A) { dispatch1(b, [&](auto B) { f(A, B); }); });
}
// mvsim_extract_path: the plan of nzo = (dim[2] - 1) / inc + 1 acquired planes as path = {EXTRACT_K_*, segments can refuse, blocks, items
// per segment}.  index_inc: 0 = inc; qshare: 0 = no work queue, else 1..16 sixteenths.
void extract_path(const int64_t dim[3], int inc, int index_inc, uint64_t index_offset, bool aligned16, int qshare, int64_t path[4]);
int poisson_queue_read_stats(const void* queue_ws, size_t bytes, long long stats[5]);
// ---- extractSlices over intervals of device volumes (extract_interval.hip runs what interval_plan.h plans)
struct IntervalView {             // per-job operands of the interval kernels (device table, blockIdx.y = job): ExtractView's idea, plus the
    const float*  in;             // pitches of the volume the tile is cut from.  in: the interval's MIN corner
    float*        out;            // the contiguous zero-min tile
    void*         queue;          // the job's Poisson work-queue segments (PItem) ...
    unsigned int* qcount;         // ... and their counters
    uint32_t      k0, k1, stream, pad;
    long long     row_pitch, plane_pitch;   // voxels from one row / plane of the volume to the next
};
// One launch per sampler stage for `njobs` jobs of one IntervalPlan.  vt: their IntervalView table; rvt: the same jobs as the resolver's
// table (out, queue, qcount, keys; sampled launches with a queue only) -- both on the device.
int launch_extract_interval(hipStream_t s, const IntervalPlan& pl, const IntervalView* vt, const ExtractView* rvt, int njobs, bool noise, double mul);
// ---- stacked views (mvsim_simulate_views_dev): one launch per stage for V views of one ground truth; blockIdx.y / .z = view
int launch_rotate_attenuate_views(hipStream_t s, const float* in, float* att, const int64_t dim[3], const Affine* atab_dev, int nviews, double delta);
int launch_pack_u16(hipStream_t s, const float* in, unsigned short* out16, int64_t n, unsigned int* flag);
int launch_make_isotropic(hipStream_t s, const float* in, float* out, const int64_t dim[3], int inc);
// phantom generator (phantom.hip)
int launch_downsample2x(hipStream_t s, const float* in, const int64_t dim[3], float* out);
int draw_spheres_dev(mvsim_ctx* ctx, float* img, const int64_t dim[3], double min_value, double max_value, int scale,
                     int half_pixel_offset, uint64_t* rnd_state, int64_t* n_spheres);
int splat_spheres_dev(mvsim_ctx* ctx, float* img, const int64_t dim[3], const mvsim_sphere* spheres, int64_t n);
// the refraction simulator's phantom (phantom.hip): noise on the index volume, multiSpheres on image and index volume
int ri_noise_dev(mvsim_ctx* ctx, float* ri, int64_t n, uint64_t state);
int multi_spheres_dev(mvsim_ctx* ctx, float* img, float* ri, const int64_t dim[3], int scale, uint64_t* rnd_state, int64_t* n_spheres);
// the walk over n voxels resolved on the device (sphere_walk.hip); *done = false: not vouched for, walk on the host
int sphere_walk_dev(mvsim_ctx* ctx, uint64_t state, int64_t n, const WalkRule& rule, std::vector<WalkEntry>* entries, uint64_t* end_state,
                    bool* done);
// SimulateBeads.renderPoints on device outputs (beads.hip); arguments validated by the caller (api_sims.cpp)
int render_beads_dev(mvsim_ctx* ctx, const double* xyz, const int64_t* view_offsets, int64_t n, const double* m12, int nviews,
                     const int64_t dim[3], const int64_t imin[3], const double sigma[3], float* const* out_f32, uint16_t* const* out_u16);
int beads_normalize_dev(mvsim_ctx* ctx, float* img, int64_t n);
void beads_release(mvsim_ctx* ctx);
// the procedural phantom (procedural.hip); arguments validated by the caller (api_sims.cpp).  *_upload puts the host tables of a field
// on the device (synchronous); the launches that follow are asynchronous on the context's stream.
struct PerlinParams {
    double scale[3];
    int    ext[3];
    int    nvec;
    double threshold;       // NaN: the raw value
};
struct PerlinDev {
    PerlinParams   P;
    const double*  grad;    // device: n x 3
    const int32_t* perm;    // device: n
};
struct SpheresDev {
    const double* centres;  // device: n x 3
    const double* radii;    // device: n
    const void*   recs;     // device: per-sphere records of procedural.hip
    int64_t       n;
    float         background;
};
constexpr int PERLIN_MAX_VECTORS = 1536;   // 28 bytes of LDS per vector: 42 KiB
int perlin_upload(mvsim_ctx* ctx, const mvsim_perlin* p, PerlinDev* dev);
int perlin_at_dev(mvsim_ctx* ctx, const PerlinDev& pd, const double* xyz, int64_t n, double* out);
int perlin_raster_dev(mvsim_ctx* ctx, const PerlinDev& pd, const int64_t origin[3], const int64_t dim[3], float* out);
int spheres_upload(mvsim_ctx* ctx, const mvsim_sphere_set* s, SpheresDev* dev);
int spheres_at_dev(mvsim_ctx* ctx, const SpheresDev& sd, const double* xyz, int64_t n, float* out);
int spheres_raster_dev(mvsim_ctx* ctx, const mvsim_sphere_set* s, const SpheresDev& sd, const int64_t origin[3], const int64_t dim[3],
                       int combine, float* out);
int rejection_sample_dev(mvsim_ctx* ctx, uint64_t state, const double rmin[3], const double rmax[3], int64_t n_samples, const PerlinDev* pd,
                         const SpheresDev* sd, int64_t max_trials, double* xyz_out, int64_t* n_trials);
// the refraction simulator (aberrations.hip); arguments validated by the caller (api_sims.cpp), volumes on the device
void aberr_inject_geometry(const double sigma[3], int size[3], double tss[3]);
int aberr_inject_dev(mvsim_ctx* ctx, float* image, float* weight, const int64_t dim[3], const double sigma[3], const double* xyz,
                     const double* inten, const float* val, int64_t n, double sumw);
int aberr_refract3d_dev(mvsim_ctx* ctx, const float* img, const float* ri_img, const int64_t dim[3], int illum, int z, const double abc[3],
                        double ri, int64_t num_rays, uint64_t state, float* image, float* weight, double sumw, mvsim_ray_steps* steps);
int aberr_project_to_camera_dev(mvsim_ctx* ctx, const float* ri_img, const float* refr, const int64_t dim[3], int current_z,
                                int rays_per_pixel, uint64_t state, float* proj);
int aberr_ray_starts(mvsim_ctx* ctx, uint64_t state, const int64_t dim[3], int camera, int illum, int z, const double abc[3],
                     int rays_per_pixel, int64_t n, double* pos3, double* dir3);
int aberr_hessian_at_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const double* xyz, int64_t n, double* matrix9,
                         double* eigvec3, double* eigval);
int aberr_hessian_images_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], int z0, int planes, float* eigval, float* eigvec);
// raytrace.hip
int64_t trace_rays_per_range(int64_t pair_cap, int64_t max_moves);
// The step-range workspace of the two tracers (trace_rays_dev, aberr_refract3d_dev): rays run in ranges of rays_per_range; a trace
// kernel fills slot_xyz / slot_val (record of ray r, move m at r * max_moves + m) and moves for the nr rays of a range from r0 on, and
// finish() scans the moves, compacts the records into xyz / val, appends them to `steps` (null: not wanted; `who` names the caller in
// the capacity refusal), injects them into image and weight (null: no injection) and synchronises.
struct StepRanges {
    Scratch ws;
    int64_t rays_per_range = 0, max_rays = 0;
    int     max_moves = 0;
    double *slot_xyz = nullptr, *xyz = nullptr;
    float  *slot_val = nullptr, *val = nullptr;
    int    *moves = nullptr, *offs = nullptr;
    int reserve(mvsim_ctx* ctx, int64_t nrays, int max_moves);
    int finish(mvsim_ctx* ctx, const char* who, int64_t r0, int nr, const int64_t dim[3], const double sigma[3], double sumw, float* image,
               float* weight, mvsim_ray_steps* steps);
};
int trace_rays_dev(mvsim_ctx* ctx, const float* ri_img, const float* img, const int64_t dim[3], const double* pos3, const double* dir3,
                   const float* intensity, int64_t n, const mvsim_trace_params* tp, double sumw, float* image, float* weight,
                   mvsim_ray_steps* steps, double* end_pos3, double* end_dir3, int64_t* n_capped);
int trace_ray_starts(mvsim_ctx* ctx, int bundle, uint64_t state, const int64_t dim[3], int x, int z, int64_t n, double* pos3, double* dir3);
int draw_simple_image_dev(mvsim_ctx* ctx, float* out, const int64_t dim[3], float low, float high);
int aberr_normalize_dev(mvsim_ctx* ctx, const float* image, const float* weight, int64_t n, float* out);
int aberr_project_dev(mvsim_ctx* ctx, const float* image, const float* weight, const int64_t dim[3], float* proj);
int launch_weight_image(hipStream_t s, float* out, const int64_t dim[3]);
int launch_weights(hipStream_t s, float* const* views, int nv, int64_t n, const float* sum_in, float* sum_out,
                   float osem, bool sum_only);

// FFT convolution pieces
int launch_pad_mirror(hipStream_t s, const float* img, const int64_t dim[3], const int64_t kdim[3],
                      float* padded, const int64_t P[3]);
int launch_psf_embed(hipStream_t s, const float* psf, const int64_t kdim[3], float* padded, const int64_t P[3]);
int launch_cmul(hipStream_t s, float2* f, const float2* g, int64_t n);
// out = crop(real) * scale; also accumulates block partial sums -> partial (SUM_BLOCKS doubles) and scal[0]
int launch_crop_scale_sum(hipStream_t s, const float* real, const int64_t P[3], float* out,
                          const int64_t dim[3], float scale, double* partial, double* scal);
int launch_stencil(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* psf,
                   const int64_t kdim[3], float* out);
bool stencil_chunk_geometry(const int64_t kdim[3], int64_t out[5]);
// raise a kernel's dynamic-LDS limit once per context (hipFuncSetAttribute is not free on a launch path)
int ensure_lds_attr(mvsim_ctx* ctx, const void* kernel, size_t bytes);

// What the caller would like the tail of the convolution to do beyond "write the convolved volume"; every request is
// optional for the implementation, which reports back what it did.
struct ConvTail {
    // in: `img` / `psf` / `out` hold this many views stacked back to back (mvsim_simulate_views_dev; the caller has checked
    // custom_fft_batchable): one launch per pass for all of them, sums and factors in the context's scalar pairs 0 .. views-1
    int views = 1;
    // in: produce only the planes k * zstride (the planes extractSlices will read) into a COMPACT out[nk][Ny][Nx].
    // Possible when adjustImage's sum comes from the spectrum side (early sum); out: the stride actually applied (1 = full).
    int zstride = 1;
    // in: the caller would like the last pass to adjust (Tools.adjustImage), extract (every inc-th plane) and run phase 1 of
    // the Poisson sampler itself instead of writing the convolved volume: everything below describes that request.
    bool     want_fuse = false;
    float    min_value = 0.f, target_average = 1.f;
    float*   con_adj = nullptr;        // adjusted volume (all planes) if the caller wants it, else null
    float*   acq = nullptr;            // acquisition
    int      inc = 1;
    bool     noise = false;
    double   mul = 0.0;
    uint64_t seed = 0;
    uint32_t stream = 0;
    // out: true when the convolution did all of that (sum, factor in the context's scalar slots; acquisition complete), and the
    // blocks and items per segment of the queue pass E filled
    bool     fused = false;
    long long    fused_blocks = 0;
    unsigned int fused_segcap = 0;
    // in: pass A has run already -- the context's spectrum buffer holds the x transform of the image rows (fused rotate +
    // attenuate + x transform, rotate_fft.hip); `img` is not read
    bool     x_done = false;
    // in: voxels of the view (> 0: compute adjustImage's factor from min_value / target_average together with the sum);
    // out: corr_done = the factor is in the context's scalar slot, no separate k_adjust_corr needed
    long long corr_n = 0;
    bool      corr_done = false;
    // in (with x_done): per-plane flags the fused rotate kernel has set (1 = the attenuated plane holds a non-zero voxel; device
    // array of dim[2] ints): passes B .. E skip the planes whose inputs are all empty -- exact, their spectra are zero
    const int* plane_nz = nullptr;
    // in (with x_done): the row-bit record of the fused rotate kernel (row_bits.h; device array, dim[2] records of row_bits_words(Py)
    // words).  Non-null means that kernel has NOT written the rows whose bit is clear: pass B must read the bits, whatever else the
    // convolution decides
    const unsigned int* row_bits = nullptr;
    // in: the caller's half of the sparse-tail condition (extract_plan.h: tail_sparse_ok) -- option skip_tail, `out` is the context's
    // own workspace, and the launch behind the convolution will be one of the two queue samplers whichever stride is applied.
    // out: sparse = pass E has left the planes k of `out` with sparse_flags[k * sparse_stride] == 0 UNWRITTEN (stale bytes of
    // earlier views): nothing but a sampler launch of this view that carries the flags (ExtractOps::empty_flags) may read `out`.
    // The flag words are the dilated flags of ctx->plane_flags, which the NEXT view's rotate kernel rewrites: the sampler has to be
    // enqueued in front of it, on the same stream or joined (view_enqueue: a sparse tail never stays pending)
    bool       want_sparse = false;
    bool       sparse = false;
    const int* sparse_flags = nullptr;
    int        sparse_stride = 0;
};
// bytes of queue workspace the fused tail needs for this geometry (0: the geometry has no fused tail)
size_t fused_tail_queue_bytes(const int64_t dim[3], const int64_t kdim[3], int inc, bool con_wanted, const Options& opt);
int comm_allreduce_f64_on_stream(mvsim_ctx* cc, double* value_dev, hipStream_t s);      // comm.cpp
int rotate_attenuate_fftx(mvsim_ctx* ctx, const float* gt, float* rot_or_null, float* att_or_null, const int64_t dim[3],
                          const int64_t kdim[3], const Affine& inv, double delta, bool* done, const int** plane_nz = nullptr,
                          int z_first = 0, int nzl = -1, const unsigned int** row_bits = nullptr);
int fft_convolve(mvsim_ctx* ctx, const float* img_dev, const int64_t dim[3], const float* psf_dev,
                 const int64_t kdim[3], float* out_dev, ConvTail* tail);
void fft_release(mvsim_ctx* ctx);
void choose_padded(const int64_t dim[3], const int64_t kdim[3], int64_t P[3], const Options& opt);
// hand-written LDS FFT path (fft_driver.hip; its kernels: fft_passes.hip, zconv.hip)
bool custom_fft_sizes(const int64_t dim[3], const int64_t kdim[3], int64_t P[3], const Options& opt);
// orders a pending tail (extract + Poisson of the last view, on the tail stream) in front of whatever is enqueued on
// ctx->stream next
int  join_tail(mvsim_ctx* ctx);
// The geometry of one hand-written convolution, everything that follows from (dim, kdim, options) alone: conv_plan() derives it (false
// where custom_fft_sizes is) and nothing else does -- the fused rotate + x transform, the stacked-view test, the fused tail and the driver read it.
struct ConvPlan {
    int     n[3], k[3];             // volume and PSF extents
    int64_t P[3];                   // padded lengths (custom_fft_sizes)
    int     px, py, pz, M;          // ... as ints; M = Px / 2, the half length of the x passes
    int     tile_y, tile_z;         // lines per tile of the y and z FFT passes
    bool    zdirect;                // z pass: direct convolution with the Kz taps, unless the PSF is deep or fft_zpass=fft
    bool    ymirror;                // pass A transforms the Ny rows of a plane only, pass B reads the y halo from their mirror images
    bool    early;                  // adjustImage's sum from the z pass instead of pass E
    bool    zinline_auto;           // fft_zpass=auto takes the inline FFT z pass for whole single views
    int     hxp, pyb;               // complex row pitch of the spectrum (M + 1 rounded up to the widest tile); rows of a plane in the z-blocked layout
    int     e_rows;                 // rows per block of pass E
    // bytes of each spectrum buffer, F and G: nz_in planes enter the z pass, nz_out leave it at a pitch of nz_pitch planes per view
    size_t spectrum_bytes(int nz_in, int nz_out, int nz_pitch, int views) const
    {
        const size_t planes = zdirect ? (size_t)views * std::max(nz_in, std::max(nz_out, nz_pitch)) : (size_t)pz;
        return (size_t)hxp * (zdirect ? pyb : py) * planes * sizeof(float2);
    }
};
bool conv_plan(const int64_t dim[3], const int64_t kdim[3], const Options& opt, ConvPlan* pl);
int  custom_fft_convolve(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* psf,
                         const int64_t kdim[3], float* out, ConvTail* tail);
// z-slab form (direct z pass only): `img` holds the planes [z_in0, z_in0 + nz_in) of a volume with dim[2] planes,
// `out` receives the planes [z_out0, z_out0 + nz_out); every plane the Kz taps reach (mirrored at the global faces)
// must lie inside the input range.  The sum left in the context's scalar slot is the sum of the output planes.
struct SlabRange {
    int z_in0, nz_in, z_out0, nz_out;
};
int  custom_fft_convolve_slab(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* psf,
                              const int64_t kdim[3], const SlabRange& slab, float* out, ConvTail* tail);
void custom_fft_release(mvsim_ctx* ctx);
bool custom_fft_geometry(const int64_t dim[3], const int64_t kdim[3], int64_t g[5], const Options& opt);
// {kernel (0: k_zconv, else the stride of k_zconv_strided), zc, nch, nkxb} of the direct z pass of a whole view that returns every inc-th
// plane only (mvsim_zpass_geometry); false where that view's z pass is not the direct convolution
bool custom_zpass_geometry(const int64_t dim[3], const int64_t kdim[3], int inc, int64_t g[4], const Options& opt);
// the plan of the fused tail (pass E adjusts, extracts and samples: blocks, items per segment, queue layout); false when the view would not be fused
bool fused_tail_geometry(const int64_t dim[3], const int64_t kdim[3], int inc, bool con_wanted, const Options& opt, ExtractPlan* fp);
// true when views of this geometry can run stacked through the hand-written passes (ConvTail::views > 1): direct z pass, early sum,
// pass B reading the mirrored y halo from its mirror images, no inline-FFT z pass, no fused tail
bool custom_fft_batchable(const mvsim_ctx* ctx, const int64_t dim[3], const int64_t kdim[3]);

// stage markers: a roctx range per stage (what rocprofv3 --marker-trace / a timeline shows around the launches; the reference
// prints a time stamp per stage, SimulateMultiViewDataset.java:553-590) and, when timing is on, HIP events recorded on the
// stream the kernels run on.  begin/end pairs nest strictly.
inline const char* stage_name(int st)
{
    static const char* const names[ST_COUNT] = {"mvsim:rotate", "mvsim:attenuate", "mvsim:psf_spectrum", "mvsim:convolve", "mvsim:adjust",
                                               "mvsim:extract_poisson", "mvsim:pass_A_x_r2c", "mvsim:pass_B_y_fwd", "mvsim:pass_C_z",
                                               "mvsim:pass_D_y_inv", "mvsim:pass_E_x_c2r"};
    return names[st];
}
inline void ev_begin(mvsim_ctx* ctx, int st)
{
    (void)roctxRangePushA(stage_name(st));
    ctx->roctx_depth += 1;
    if (ctx->timing) (void)hipEventRecord(ctx->evr[ctx->ev_cur][st][0], ctx->stream);
}
inline void ev_end(mvsim_ctx* ctx, int st)
{
    if (ctx->roctx_depth > 0) { (void)roctxRangePop(); ctx->roctx_depth -= 1; }
    if (ctx->timing) {
        (void)hipEventRecord(ctx->evr[ctx->ev_cur][st][1], ctx->stream);
        ctx->ev_used[ctx->ev_cur][st] = true;
    }
}
// An error return between ev_begin and ev_end (MVSIM_TRY / MVSIM_HIP) leaves ranges open: every entry point closes what
// the previous call on this context left behind (set_device), and so does mvsim_destroy.
inline void ev_rebalance(mvsim_ctx* ctx)
{
    while (ctx->roctx_depth > 0) { (void)roctxRangePop(); ctx->roctx_depth -= 1; }
}
// start a new slot (called once per timed call)
inline void ev_next(mvsim_ctx* ctx)
{
    if (!ctx->timing) return;
    if (ctx->ev_calls > 0) ctx->ev_cur = (ctx->ev_cur + 1) % mvsim_ctx::TIMING_SLOTS;
    ctx->ev_calls += 1;
    for (int s = 0; s < ST_COUNT; ++s) ctx->ev_used[ctx->ev_cur][s] = false;
}

// [sum, adjustImage factor] of the current view, behind the block partials; stacked views: one pair per view.  The doubles behind
// the pairs are scratch of the one-double all-reduce (comm.cpp)
constexpr int SCAL_DOUBLES = 2 * MVSIM_MAX_VIEWS;
constexpr size_t PARTIALS_BYTES = (size_t)(SUM_BLOCKS + SCAL_DOUBLES + 8) * sizeof(double);
inline double* scal_of(mvsim_ctx* ctx, int view = 0) { return ctx->partials.as<double>() + SUM_BLOCKS + 2 * view; }

// comm.cpp: a device range is about to go away -- drop the peer mappings registered for it (broadcast=peer_copy)
void comm_forget_range(mvsim_ctx* ctx, const void* p, size_t bytes);

void axis_rotation_host(const int64_t dim[3], int axis, int degrees, double m[12]);
void affine_invert_host(const double m[12], double inv[12]);

}  // namespace mvsim
