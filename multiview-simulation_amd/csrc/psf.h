// What psf.hip (the kernels of the PSF extraction: select, count, gather, reduce, finish, use-mask) and api_psf.cpp (its driver) share.
#pragma once

#include "common.h"

namespace mvsim {

// launch geometry (mvsim_psf_geometry reports it).  The gather kernel's grid is (tap tiles x bead chunks): a block of PSF_TAPS threads
// owns PSF_TAPS consecutive taps (kx fastest) of one chunk of PSF_CHUNK consecutive list indices.  The selection kernel is one wave of
// PSF_QUERIES bead lanes per block, the list staged through LDS PSF_SELECT_TILE points at a time.  The finish kernel is ONE block of
// PSF_FINISH_THREADS threads, a thread per chunk of PSF_CHUNK taps: 63^3 taps are 977 chunks.
constexpr int PSF_CHUNK = MVSIM_PSF_CHUNK, PSF_TAPS = 256, PSF_QUERIES = 64, PSF_SELECT_TILE = 256, PSF_FINISH_THREADS = 1024;
constexpr long long PSF_MAX_TAPS = (long long)MVSIM_PSF_MAX_DIM * MVSIM_PSF_MAX_DIM * MVSIM_PSF_MAX_DIM;
constexpr long long PSF_MAX_BLOCKS = ((PSF_MAX_TAPS + PSF_TAPS - 1) / PSF_TAPS) * (MVSIM_PSF_MAX_POINTS / PSF_CHUNK);
static_assert((PSF_MAX_TAPS + PSF_CHUNK - 1) / PSF_CHUNK <= PSF_FINISH_THREADS, "the finish kernel holds one chunk sum per thread");

struct PsfList {                 // a point list as the kernels take it
    const char*      pos;        // 3 doubles at `stride` bytes
    long long        stride;
    const long long* n_dev;
    long long        capacity;
};

struct PsfMatrix {               // the forward matrix as the kernels take it: from device memory, by value, or the identity
    const double* m_dev;
    double        m[12];
    int           given, pad;    // 0: identity (m_dev null)
};

struct PsfJob {
    long long dim[3], kdim[3];
    double    min_separation[3];
    int       src_type, subtract_min, normalize, crowding;   // crowding: min_separation is not all zero
};

// step 3: status (n bytes) and the record's counts and flags
int launch_psf_select(hipStream_t s, const PsfList& L, const unsigned char* use, const PsfMatrix& M, const PsfJob& job, unsigned char* status,
                      mvsim_psf_result* result);
// steps 4 and 5.  partials: ceil(capacity / PSF_CHUNK) x prod(kdim) doubles
int launch_psf_gather(hipStream_t s, const void* img, const PsfList& L, const unsigned char* status, const PsfMatrix& M, const PsfJob& job,
                      double* partials, double* totals);
// step 6
int launch_psf_finish(hipStream_t s, const double* totals, const PsfJob& job, float* psf, mvsim_psf_result* result);
int launch_psf_use_from_matches(hipStream_t s, const mvsim_match* cand, const long long* n_cand, long long capacity, const unsigned char* mask,
                                int side, long long n_points, unsigned char* use);

}  // namespace mvsim
