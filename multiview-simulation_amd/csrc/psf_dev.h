// The arithmetic of the PSF extraction that the device kernels (psf.hip) and the host helpers (mvsim_psf_offsets, mvsim_psf_select,
// mvsim_psf_finish in api_psf.cpp) share, stated once: the inverse of the matrix's linear part, a tap's offset, the corner test, the
// crowding test of a pair, the order the minimum is taken in.  mvsim.h states the recipe; every + - * / here is an operation of its
// own (the build has -ffp-contract=off).  Plain C++ outside hipcc.
#pragma once

#include "fuse_dev.h"

namespace mvsim {

// step 1: the nine i_rc of [A | 0] into inv[4 r + c] (inv[4 r + 3] is not used); m == nullptr: the identity through the same arithmetic
MVSIM_FUSE_FN bool psf_invert(const double* m, double inv[12])
{
    double a[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a[4 * r + c] = m ? m[4 * r + c] : (r == c ? 1.0 : 0.0);
        a[4 * r + 3] = 0.0;
    }
    return fuse_invert(a, inv);
}

// step 2 for one axis: inv_r = &inv[4 r]
MVSIM_FUSE_FN double psf_delta(const double* inv_r, double jx, double jy, double jz) { return ((inv_r[2] * jz) + inv_r[1] * jy) + inv_r[0] * jx; }

MVSIM_FUSE_FN bool psf_finite3(const double* p) { return fuse_finite(p[0]) && fuse_finite(p[1]) && fuse_finite(p[2]); }

// step 3, OUTSIDE: one of the eight corner taps fails the box on an axis
MVSIM_FUSE_FN bool psf_outside(const double inv[12], const long long kdim[3], const long long dim[3], const double* pos)
{
    bool out = false;
    for (int c = 0; c < 8; ++c) {
        const long long kx = (c & 1) ? kdim[0] - 1 : 0, ky = (c & 2) ? kdim[1] - 1 : 0, kz = (c & 4) ? kdim[2] - 1 : 0;
        const double jx = (double)(kx - kdim[0] / 2), jy = (double)(ky - kdim[1] / 2), jz = (double)(kz - kdim[2] / 2);
        for (int r = 0; r < 3; ++r) {
            const double p = pos[r] + psf_delta(inv + 4 * r, jx, jy, jz);
            out = out || !(0.0 <= p && p <= (double)(dim[r] - 1));
        }
    }
    return out;
}

// step 3, CROWDED, for one other finite point
MVSIM_FUSE_FN bool psf_crowds(double ax, double ay, double az, double bx, double by, double bz, const double sep[3])
{
    return fabs(bx - ax) < sep[0] && fabs(by - ay) < sep[1] && fabs(bz - az) < sep[2];
}

// step 4: the clamp in front of the fusion's sample
MVSIM_FUSE_FN double psf_clamp(double p, double top)
{
    const double q = p > 0.0 ? p : 0.0;
    return q < top ? q : top;
}

// step 6: "ascending t, if mean_t < b" as an order that any reduction tree can apply: the smaller value, the lower index among equals
// (-0.0 and +0.0 are equal); the start (+inf, no index) loses to every smaller value and a NaN never wins
MVSIM_FUSE_FN bool psf_min_less(double v, long long t, double bv, long long bt) { return v < bv || (v == bv && t < bt); }

}  // namespace mvsim
