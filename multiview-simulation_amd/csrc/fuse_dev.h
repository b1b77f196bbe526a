// The arithmetic of the view fusion that the device kernels (fuse.hip) and the host (mvsim_fuse_invert in api_fuse.cpp) share, stated
// once: the inverse of a view's matrix, the row-constant part of an output voxel's position, the border weight.  mvsim.h states the
// recipe; every + - * / here is an operation of its own (the build has -ffp-contract=off).  Plain C++ outside hipcc.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MVSIM_FUSE_FN __host__ __device__ __forceinline__
#else
#define MVSIM_FUSE_FN inline
#endif

namespace mvsim {

MVSIM_FUSE_FN bool fuse_finite(double v) { return v - v == 0.0; }

// step 1: inv = [A^-1 | -A^-1 t] of m = [A | t]; false (inv untouched): an entry is non-finite, or det is zero or non-finite
MVSIM_FUSE_FN bool fuse_invert(const double m[12], double inv[12])
{
    bool finite = true;
    for (int k = 0; k < 12; ++k) finite = finite && fuse_finite(m[k]);
    if (!finite) return false;
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9], m22 = m[10];
    const double det = m00 * m11 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20 - m00 * m12 * m21 - m01 * m10 * m22;
    if (det == 0.0 || !fuse_finite(det)) return false;
    const double idet = 1.0 / det;
    double i[3][3];
    i[0][0] = (m11 * m22 - m12 * m21) * idet; i[0][1] = (m02 * m21 - m01 * m22) * idet; i[0][2] = (m01 * m12 - m02 * m11) * idet;
    i[1][0] = (m12 * m20 - m10 * m22) * idet; i[1][1] = (m00 * m22 - m02 * m20) * idet; i[1][2] = (m02 * m10 - m00 * m12) * idet;
    i[2][0] = (m10 * m21 - m11 * m20) * idet; i[2][1] = (m01 * m20 - m00 * m21) * idet; i[2][2] = (m00 * m11 - m01 * m10) * idet;
    for (int r = 0; r < 3; ++r) {
        inv[4 * r + 0] = i[r][0]; inv[4 * r + 1] = i[r][1]; inv[4 * r + 2] = i[r][2];
        inv[4 * r + 3] = -((i[r][0] * m[3] + i[r][1] * m[7]) + i[r][2] * m[11]);
    }
    return true;
}

// step 2 for one axis: the part that is constant along an output row, and the whole position
MVSIM_FUSE_FN double fuse_row(const double* inv_r, double oy, double oz) { return (inv_r[3] + inv_r[2] * oz) + inv_r[1] * oy; }
MVSIM_FUSE_FN double fuse_pos(const double* inv_r, double ox, double oy, double oz) { return fuse_row(inv_r, oy, oz) + inv_r[0] * ox; }

// step 5 for one axis; p inside [0, top], top = (double)(N - 1)
MVSIM_FUSE_FN double fuse_ramp(double p, double top, double blend)
{
    const double far = top - p;
    const double e = p < far ? p : far;
    if (!(e < blend)) return 1.0;
    const double q = e / blend;
    return (q * q) * (3.0 - 2.0 * q);
}

}  // namespace mvsim
