// C ABI of libmvsim, part 6: the bead detector (mvsim.h states the recipe) -- difference of Gaussians, its strict local maxima in index
// order, the quadratic sub-voxel fit.  Host orchestration only: taps in fp64, workspaces, launches of detect.hip on the context's stream.
// Every argument is checked before the context is touched, so each refusal can be reached without a device.
#include "api_internal.h"
#include "detect.h"

namespace mvsim {

int dog_taps_host(double sigma, float* taps, int* ntaps)
{
    MVSIM_CHECK_ARG(std::isfinite(sigma) && sigma > 0.0, "dog: sigma must be a positive finite number");
    MVSIM_CHECK_ARG(sigma <= 64.0, "dog: sigma needs more than MVSIM_DOG_MAX_TAPS taps");
    const int d = suggested_kernel_diameter(sigma);
    MVSIM_CHECK_ARG(d <= MVSIM_DOG_MAX_TAPS, "dog: sigma needs more than MVSIM_DOG_MAX_TAPS taps");
    const int r = d / 2;
    double e[MVSIM_DOG_MAX_TAPS];
    double sum = 0.0;
    for (int j = 0; j < d; ++j) {
        const double x = (double)(j - r);
        e[j] = std::exp(-(x * x) / (2.0 * sigma * sigma));
        sum += e[j];
    }
    for (int j = 0; j < d; ++j) taps[j] = (float)(e[j] / sum);
    *ntaps = d;
    return MVSIM_OK;
}

namespace {

enum { DET_HALF1 = 0, DET_HALF2, DET_DOG, DET_LIST, DET_COUNTS, DET_SCAN };

int check_volume(const int64_t dim[3], int min_extent)
{
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(dim[0] >= min_extent && dim[1] >= min_extent && dim[2] >= min_extent, "detect: every extent must be >= 2");
    MVSIM_CHECK_ARG(nvox(dim) < ((int64_t)1 << 40), "detect: volume too large for one launch");
    return MVSIM_OK;
}

int make_taps(const mvsim_dog_params* p, DogTaps* T)
{
    MVSIM_CHECK_ARG(p != nullptr, "dog: params is null");
    std::memset(T, 0, sizeof(*T));
    for (int set = 0; set < 2; ++set)
        for (int d = 0; d < 3; ++d) {
            int n = 0;
            MVSIM_TRY(dog_taps_host(set == 0 ? p->sigma1[d] : p->sigma2[d], T->t[set][d], &n));
            T->r[set][d] = n / 2;
        }
    return MVSIM_OK;
}

int check_src_type(int src_type)
{
    MVSIM_CHECK_ARG(src_type == MVSIM_SRC_F32 || src_type == MVSIM_SRC_U16, "detect: src_type must be MVSIM_SRC_F32 or MVSIM_SRC_U16");
    return MVSIM_OK;
}

int check_peaks_args(float threshold, int64_t capacity)
{
    MVSIM_CHECK_ARG(!std::isnan(threshold), "detect: threshold is NaN");
    MVSIM_CHECK_ARG(capacity >= 1, "detect: capacity must be >= 1");
    MVSIM_CHECK_ARG(capacity <= ((int64_t)1 << 31), "detect: capacity too large for one launch");
    return MVSIM_OK;
}

int dog_enqueue(mvsim_ctx* ctx, const void* img, int src_type, const int64_t dim[3], const DogTaps& T, float* dog)
{
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(ctx->detect_buf[DET_HALF1].reserve(bytes));
    MVSIM_TRY(ctx->detect_buf[DET_HALF2].reserve(bytes));
    return launch_dog(ctx, img, src_type, dim, T, ctx->detect_buf[DET_HALF1].as<float>(), ctx->detect_buf[DET_HALF2].as<float>(), dog);
}

int find_peaks_enqueue(mvsim_ctx* ctx, const float* vol, const int64_t dim[3], float threshold, int64_t capacity, int64_t* voxels,
                       int64_t* n_found)
{
    const int64_t n = nvox(dim);
    const size_t scan_bytes = peaks_scan_bytes(n);
    MVSIM_TRY(ctx->detect_buf[DET_COUNTS].reserve(peaks_counts_bytes(n)));
    MVSIM_TRY(ctx->detect_buf[DET_SCAN].reserve(scan_bytes));
    return launch_find_peaks(ctx->stream, vol, dim, threshold, capacity, voxels, n_found, ctx->detect_buf[DET_COUNTS].as<int64_t>(),
                             ctx->detect_buf[DET_SCAN].p, scan_bytes);
}

int check_detect(const void* img, int src_type, const int64_t dim[3], const mvsim_dog_params* p, int64_t capacity, const void* peaks,
                 const void* n_found, DogTaps* T)
{
    MVSIM_CHECK_ARG(img && peaks && n_found, "detect: null pointer");
    MVSIM_TRY(check_src_type(src_type));
    MVSIM_TRY(check_volume(dim, 2));
    MVSIM_TRY(make_taps(p, T));
    MVSIM_TRY(check_peaks_args(p->threshold, capacity));
    MVSIM_CHECK_ARG(p->max_moves >= 0, "detect: max_moves must be >= 0");
    return MVSIM_OK;
}

}  // namespace

}  // namespace mvsim

using namespace mvsim;

extern "C" {

void mvsim_dog_params_default(mvsim_dog_params* p)
{
    if (!p) return;
    const double s2 = 1.8 * std::pow(2.0, 0.25);
    for (int d = 0; d < 3; ++d) { p->sigma1[d] = 1.8; p->sigma2[d] = s2; }
    p->threshold = 0.008f;
    p->max_moves = 4;
}

int mvsim_dog_taps(double sigma, float* taps, int* ntaps)
{
    MVSIM_CHECK_ARG(taps && ntaps, "dog: null pointer");
    return dog_taps_host(sigma, taps, ntaps);
}

int mvsim_dog_geometry(int64_t out[5])
{
    MVSIM_CHECK_ARG(out != nullptr, "null pointer");
    out[0] = DOG_TILE_X; out[1] = DOG_TILE_Y; out[2] = DOG_TILE_Z; out[3] = DOG_MAX_RADIUS; out[4] = PEAK_BLOCK_VOX;
    return MVSIM_OK;
}

int mvsim_dog_dev(mvsim_ctx* ctx, const void* img_dev, int src_type, const int64_t dim[3], const mvsim_dog_params* params, float* dog_dev)
{
    DogTaps T;
    MVSIM_CHECK_ARG(img_dev && dog_dev, "dog: null pointer");
    MVSIM_TRY(check_src_type(src_type));
    MVSIM_TRY(check_volume(dim, 2));
    MVSIM_TRY(make_taps(params, &T));
    MVSIM_TRY(set_device(ctx));
    return dog_enqueue(ctx, img_dev, src_type, dim, T, dog_dev);
}

int mvsim_find_peaks_dev(mvsim_ctx* ctx, const float* vol_dev, const int64_t dim[3], float threshold, int64_t capacity, int64_t* voxels_dev,
                         int64_t* n_found_dev)
{
    MVSIM_CHECK_ARG(vol_dev && voxels_dev && n_found_dev, "find_peaks: null pointer");
    MVSIM_TRY(check_volume(dim, 1));
    MVSIM_TRY(check_peaks_args(threshold, capacity));
    MVSIM_TRY(set_device(ctx));
    return find_peaks_enqueue(ctx, vol_dev, dim, threshold, capacity, voxels_dev, n_found_dev);
}

int mvsim_localise_peaks_dev(mvsim_ctx* ctx, const float* vol_dev, const int64_t dim[3], const int64_t* voxels_dev, const int64_t* n_found_dev,
                             int64_t capacity, int max_moves, mvsim_peak* peaks_dev)
{
    MVSIM_CHECK_ARG(vol_dev && voxels_dev && n_found_dev && peaks_dev, "localise_peaks: null pointer");
    MVSIM_TRY(check_volume(dim, 1));
    MVSIM_TRY(check_peaks_args(0.0f, capacity));
    MVSIM_CHECK_ARG(max_moves >= 0, "detect: max_moves must be >= 0");
    MVSIM_TRY(set_device(ctx));
    return launch_localise(ctx->stream, vol_dev, dim, voxels_dev, n_found_dev, capacity, max_moves, peaks_dev);
}

int mvsim_detect_beads_dev(mvsim_ctx* ctx, const void* img_dev, int src_type, const int64_t dim[3], const mvsim_dog_params* params,
                           int64_t capacity, mvsim_peak* peaks_dev, int64_t* n_found_dev)
{
    DogTaps T;
    MVSIM_TRY(check_detect(img_dev, src_type, dim, params, capacity, peaks_dev, n_found_dev, &T));
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(ctx->detect_buf[DET_DOG].reserve((size_t)nvox(dim) * sizeof(float)));
    MVSIM_TRY(ctx->detect_buf[DET_LIST].reserve((size_t)capacity * sizeof(int64_t)));
    float* dog = ctx->detect_buf[DET_DOG].as<float>();
    int64_t* list = ctx->detect_buf[DET_LIST].as<int64_t>();
    MVSIM_TRY(dog_enqueue(ctx, img_dev, src_type, dim, T, dog));
    MVSIM_TRY(find_peaks_enqueue(ctx, dog, dim, params->threshold, capacity, list, n_found_dev));
    return launch_localise(ctx->stream, dog, dim, list, n_found_dev, capacity, params->max_moves, peaks_dev);
}

int mvsim_detect_beads(mvsim_ctx* ctx, const void* img, int src_type, const int64_t dim[3], const mvsim_dog_params* params, int64_t capacity,
                       mvsim_peak* peaks, int64_t* n_found)
{
    DogTaps T;
    MVSIM_TRY(check_detect(img, src_type, dim, params, capacity, peaks, n_found, &T));
    MVSIM_TRY(set_device(ctx));
    // device twins for this call only: the image, the peaks and the count behind them
    const size_t img_bytes = (size_t)nvox(dim) * (src_type == MVSIM_SRC_U16 ? sizeof(uint16_t) : sizeof(float));
    const size_t peak_bytes = (size_t)capacity * sizeof(mvsim_peak);
    DevBuf dimg, dpeaks;
    int rc = up(ctx, dimg, reinterpret_cast<const float*>(img), img_bytes);
    if (rc == MVSIM_OK) rc = dpeaks.reserve(peak_bytes + sizeof(int64_t));
    int64_t* dcount = rc == MVSIM_OK ? reinterpret_cast<int64_t*>(dpeaks.as<char>() + peak_bytes) : nullptr;
    if (rc == MVSIM_OK) rc = mvsim_detect_beads_dev(ctx, dimg.p, src_type, dim, params, capacity, dpeaks.as<mvsim_peak>(), dcount);
    if (rc == MVSIM_OK) rc = down(ctx, reinterpret_cast<float*>(n_found), dcount, sizeof(int64_t));
    if (rc == MVSIM_OK) {
        const int64_t listed = std::min<int64_t>(std::max<int64_t>(*n_found, 0), capacity);
        if (listed > 0) rc = down(ctx, reinterpret_cast<float*>(peaks), dpeaks.p, (size_t)listed * sizeof(mvsim_peak));
    }
    (void)hipStreamSynchronize(ctx->stream);
    dimg.release();
    dpeaks.release();
    return rc;
}

}  // extern "C"
