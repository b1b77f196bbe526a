// What detect.hip (the kernels of the bead detector: DoG, peaks, localisation) and api_detect.cpp (its driver) share.
#pragma once

#include "common.h"

namespace mvsim {

// launch geometry (mvsim_dog_geometry reports it): the xy kernel blurs a DOG_TILE_X x DOG_TILE_Y tile of one plane, the z kernel a
// DOG_TILE_X x DOG_TILE_Z tile of one (x, z) slice, both with a halo of the larger radius (at most DOG_MAX_RADIUS) staged in LDS; a
// block of the peaks kernels takes PEAK_BLOCK_VOX consecutive voxels
constexpr int DOG_TILE_X = 64, DOG_TILE_Y = 16, DOG_TILE_Z = 32;
constexpr int DOG_MAX_RADIUS = (MVSIM_DOG_MAX_TAPS - 1) / 2;
constexpr int PEAK_BLOCK_VOX = 256 * 8;

struct DogTaps {             // [set: sigma1, sigma2][axis]; a kernel argument
    int   r[2][3];
    float t[2][3][MVSIM_DOG_MAX_TAPS + 1];
};

// step 1 of the recipe; MVSIM_EINVAL for a sigma that is not a positive finite number or needs more than MVSIM_DOG_MAX_TAPS taps
int dog_taps_host(double sigma, float* taps, int* ntaps);
// steps 2 and 3: img (float or uint16_t, any alignment) -> dog (any alignment) through the two half-blurred volumes half1 / half2
// (16-byte aligned workspaces of the image's size)
int launch_dog(mvsim_ctx* ctx, const void* img, int src_type, const int64_t dim[3], const DogTaps& taps, float* half1, float* half2, float* dog);
// step 4.  counts: peaks_counts_bytes(n) bytes (the per-block counts, their exclusive scan, one ballot word per 64 voxels);
// scan_tmp: peaks_scan_bytes(n) bytes
int64_t peak_blocks(int64_t n);
size_t  peaks_counts_bytes(int64_t n);
size_t  peaks_scan_bytes(int64_t n);
int launch_find_peaks(hipStream_t s, const float* vol, const int64_t dim[3], float threshold, int64_t capacity, int64_t* voxels,
                      int64_t* n_found, int64_t* counts, void* scan_tmp, size_t scan_bytes);
// step 5: `capacity` lanes, the surplus ones exit
int launch_localise(hipStream_t s, const float* vol, const int64_t dim[3], const int64_t* voxels, const int64_t* n_found, int64_t capacity,
                    int max_moves, mvsim_peak* peaks);

}  // namespace mvsim
