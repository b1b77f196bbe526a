// The kernels of the view fusion (mvsim.h states the recipe): a prepare kernel that inverts every view's matrix -- given by value or
// read from device memory -- into the context's table, and ONE resample + blend kernel template, specialised on the source type, on
// fused versus aligned output and on whether any blend is non-zero.  fp64 throughout, every operation of its own (fuse_dev.h), no
// atomics, no LDS: a thread owns its output voxels from the first view to the store.
#include "fuse.h"
#include "fuse_dev.h"

namespace mvsim {

namespace {

__global__ __launch_bounds__(64) void k_fuse_prepare(FusePrepareArgs a, int first, int n, FuseViewRec* __restrict__ recs,
                                                     int32_t* __restrict__ status)
{
    const int t = (int)threadIdx.x;
    if (t >= n) return;
    const FuseViewArg& v = a.v[t];
    double m[12], inv[12];
    for (int k = 0; k < 12; ++k) { m[k] = v.m_dev ? v.m_dev[k] : v.m[k]; inv[k] = 0.0; }
    const bool ok = fuse_invert(m, inv);
    FuseViewRec& r = recs[first + t];
    for (int k = 0; k < 12; ++k) r.inv[k] = inv[k];
    r.src = v.src;
    for (int d = 0; d < 3; ++d) r.dim[d] = v.dim[d];
    r.aligned = v.aligned;
    r.weight = v.weight;
    r.singular = ok ? 0 : 1;
    r.pad = 0;
    if (status) status[first + t] = ok ? 0 : MVSIM_FUSE_SINGULAR;
}

template <bool U16> __device__ __forceinline__ double fuse_load(const void* src, long long i)
{
    if (U16) return (double)(float)static_cast<const uint16_t*>(src)[i];
    return (double)static_cast<const float*>(src)[i];
}

// The brick [b0, b0 + B) provably misses the view's box on axis r: all eight transformed corners lie beyond the same face by more than
// a margin that covers the rounding of step 2 (4 operations on terms of magnitude <= mag: a few 1e-16 mag) many times over.  The
// position of a voxel inside the brick is, exactly, a convex combination of the corners'; a NaN compares false and skips nothing.
__device__ __forceinline__ bool fuse_misses(const double* inv, const long long dim[3], const double lo[3], const double hi[3])
{
    bool miss = false;
    for (int r = 0; r < 3; ++r) {
        const double* ir = inv + 4 * r;
        bool below = true, above = true;
        const double top = (double)(dim[r] - 1);
        for (int c = 0; c < 8; ++c) {
            const double ox = (c & 1) ? hi[0] : lo[0], oy = (c & 2) ? hi[1] : lo[1], oz = (c & 4) ? hi[2] : lo[2];
            const double p = fuse_pos(ir, ox, oy, oz);
            const double mag = (fabs(ir[3]) + fabs(ir[2] * oz)) + (fabs(ir[1] * oy) + fabs(ir[0] * ox));
            const double margin = 1.0 + 1e-9 * mag;
            below = below && (p < -margin);
            above = above && (p > top + margin);
        }
        miss = miss || below || above;
    }
    return miss;
}

template <bool U16, bool ALIGNED, bool BLEND>
__global__ __launch_bounds__(FUSE_BX * FUSE_BY) void k_fuse(FuseJob job, const FuseViewRec* __restrict__ recs, float* __restrict__ fused,
                                                            float* __restrict__ sum_weights)
{
    const long long nbx = (job.out_dim[0] + FUSE_BX - 1) / FUSE_BX, nby = (job.out_dim[1] + FUSE_BY - 1) / FUSE_BY;
    const long long nbz = (job.out_dim[2] + FUSE_BZ - 1) / FUSE_BZ;
    const long long bricks = nbx * nby * nbz;
    // blocks b and b + 8 tend to share an XCD (for speed only): XCD x walks the x-th of 8 consecutive runs of bricks, so that the
    // gathers of neighbouring bricks meet in one L2
    const long long run = (bricks + FUSE_XCDS - 1) / FUSE_XCDS;
    const long long xcd = blockIdx.x % FUSE_XCDS, slot = blockIdx.x / FUSE_XCDS, slots = gridDim.x / FUSE_XCDS;
    const int lane = (int)threadIdx.x % FUSE_BX, row = (int)threadIdx.x / FUSE_BX;

    for (long long at = slot; at < run; at += slots) {
        const long long brick = xcd * run + at;
        if (brick >= bricks) break;
        const long long bx = brick % nbx, by = (brick / nbx) % nby, bz = brick / (nbx * nby);
        const long long x = bx * FUSE_BX + lane, y = by * FUSE_BY + row, z0 = bz * FUSE_BZ;
        const bool mine = x < job.out_dim[0] && y < job.out_dim[1];
        const double ox = (double)(job.out_min[0] + x), oy = (double)(job.out_min[1] + y);
        double lo[3], hi[3];
        lo[0] = (double)(job.out_min[0] + bx * FUSE_BX); hi[0] = lo[0] + (double)(FUSE_BX - 1);
        lo[1] = (double)(job.out_min[1] + by * FUSE_BY); hi[1] = lo[1] + (double)(FUSE_BY - 1);
        lo[2] = (double)(job.out_min[2] + z0);           hi[2] = lo[2] + (double)(FUSE_BZ - 1);
        const long long plane = job.out_dim[0] * job.out_dim[1];
        const long long o0 = x + job.out_dim[0] * y + plane * z0;

        double num[FUSE_BZ], den[FUSE_BZ];
#pragma unroll
        for (int k = 0; k < FUSE_BZ; ++k) { num[k] = 0.0; den[k] = 0.0; }

        for (int v = 0; v < job.n_views; ++v) {
            const FuseViewRec& R = recs[v];
            float* const al = ALIGNED ? R.aligned : nullptr;
            float* const wt = ALIGNED ? R.weight : nullptr;
            if (ALIGNED && !al && !wt) continue;
            const bool absent = R.singular != 0 || fuse_misses(R.inv, R.dim, lo, hi);     // uniform over the block
            if (absent) {
                if (ALIGNED && mine) {
#pragma unroll
                    for (int k = 0; k < FUSE_BZ; ++k) {
                        if (z0 + k >= job.out_dim[2]) continue;
                        if (al) al[o0 + plane * k] = 0.0f;
                        if (wt) wt[o0 + plane * k] = 0.0f;
                    }
                }
                continue;
            }
            if (!mine) continue;
            const long long Nx = R.dim[0], Ny = R.dim[1], Nz = R.dim[2];
            const double tx = (double)(Nx - 1), ty = (double)(Ny - 1), tz = (double)(Nz - 1);
            // step 2: the two products that do not depend on z, once per view; the sums keep the stated order
            const double ax = R.inv[0] * ox, ay = R.inv[4] * ox, az = R.inv[8] * ox;
            const double bx1 = R.inv[1] * oy, by1 = R.inv[5] * oy, bz1 = R.inv[9] * oy;
#pragma unroll
            for (int k = 0; k < FUSE_BZ; ++k) {
                if (z0 + k >= job.out_dim[2]) continue;
                const double oz = (double)(job.out_min[2] + z0 + k);
                const double px = ((R.inv[3] + R.inv[2] * oz) + bx1) + ax;
                const double py = ((R.inv[7] + R.inv[6] * oz) + by1) + ay;
                const double pz = ((R.inv[11] + R.inv[10] * oz) + bz1) + az;
                const bool inside = 0.0 <= px && px <= tx && 0.0 <= py && py <= ty && 0.0 <= pz && pz <= tz;
                float s_f = 0.0f;
                double w = 0.0;
                if (inside) {
                    const double fx = floor(px), fy = floor(py), fz = floor(pz);
                    const double ux = px - fx, uy = py - fy, uz = pz - fz;
                    const long long x0 = (long long)fx, y0 = (long long)fy, zz0 = (long long)fz;
                    const long long x1 = x0 + 1 < Nx ? x0 + 1 : Nx - 1, y1 = y0 + 1 < Ny ? y0 + 1 : Ny - 1, z1 = zz0 + 1 < Nz ? zz0 + 1 : Nz - 1;
                    const long long r00 = Nx * (y0 + Ny * zz0), r10 = Nx * (y1 + Ny * zz0), r01 = Nx * (y0 + Ny * z1), r11 = Nx * (y1 + Ny * z1);
                    const double v000 = fuse_load<U16>(R.src, r00 + x0), v100 = fuse_load<U16>(R.src, r00 + x1);
                    const double v010 = fuse_load<U16>(R.src, r10 + x0), v110 = fuse_load<U16>(R.src, r10 + x1);
                    const double v001 = fuse_load<U16>(R.src, r01 + x0), v101 = fuse_load<U16>(R.src, r01 + x1);
                    const double v011 = fuse_load<U16>(R.src, r11 + x0), v111 = fuse_load<U16>(R.src, r11 + x1);
                    const double c00 = v000 + ux * (v100 - v000), c10 = v010 + ux * (v110 - v010);
                    const double c01 = v001 + ux * (v101 - v001), c11 = v011 + ux * (v111 - v011);
                    const double c0 = c00 + uy * (c10 - c00), c1 = c01 + uy * (c11 - c01);
                    s_f = (float)(c0 + uz * (c1 - c0));
                    w = 1.0;
                    if (BLEND) w = (fuse_ramp(px, tx, job.blend[0]) * fuse_ramp(py, ty, job.blend[1])) * fuse_ramp(pz, tz, job.blend[2]);
                }
                if (ALIGNED) {
                    if (al) al[o0 + plane * k] = s_f;
                    if (wt) wt[o0 + plane * k] = (float)w;
                } else if (inside) {
                    num[k] = num[k] + w * (double)s_f;
                    den[k] = den[k] + w;
                }
            }
        }
        if (!ALIGNED && mine) {
#pragma unroll
            for (int k = 0; k < FUSE_BZ; ++k) {
                if (z0 + k >= job.out_dim[2]) continue;
                fused[o0 + plane * k] = den[k] > 0.0 ? (float)(num[k] / den[k]) : job.background;
                if (sum_weights) sum_weights[o0 + plane * k] = (float)den[k];
            }
        }
    }
}

template <bool U16, bool ALIGNED> void fuse_dispatch(hipStream_t s, dim3 grid, bool blend, const FuseJob& job, const FuseViewRec* recs,
                                                     float* fused, float* sum_weights)
{
    const dim3 block(FUSE_BX * FUSE_BY);
    if (blend) hipLaunchKernelGGL((k_fuse<U16, ALIGNED, true>), grid, block, 0, s, job, recs, fused, sum_weights);
    else hipLaunchKernelGGL((k_fuse<U16, ALIGNED, false>), grid, block, 0, s, job, recs, fused, sum_weights);
}

}  // namespace

int launch_fuse_prepare(hipStream_t s, const FusePrepareArgs& a, int first, int n, FuseViewRec* recs, int32_t* status_or_null)
{
    hipLaunchKernelGGL(k_fuse_prepare, dim3(1), dim3(64), 0, s, a, first, n, recs, status_or_null);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_fuse(hipStream_t s, const FuseJob& job, const FuseViewRec* recs, float* fused, float* sum_weights)
{
    const long long bricks = ((job.out_dim[0] + FUSE_BX - 1) / FUSE_BX) * ((job.out_dim[1] + FUSE_BY - 1) / FUSE_BY) *
                             ((job.out_dim[2] + FUSE_BZ - 1) / FUSE_BZ);
    const long long run = (bricks + FUSE_XCDS - 1) / FUSE_XCDS;
    const dim3 grid((unsigned)(std::min<long long>(run, FUSE_MAX_BLOCKS / FUSE_XCDS) * FUSE_XCDS));
    const bool blend = job.blend[0] > 0.0 || job.blend[1] > 0.0 || job.blend[2] > 0.0;
    const bool u16 = job.src_type == MVSIM_SRC_U16;
    if (fused) {
        if (u16) fuse_dispatch<true, false>(s, grid, blend, job, recs, fused, sum_weights);
        else fuse_dispatch<false, false>(s, grid, blend, job, recs, fused, sum_weights);
    } else {
        if (u16) fuse_dispatch<true, true>(s, grid, blend, job, recs, nullptr, nullptr);
        else fuse_dispatch<false, true>(s, grid, blend, job, recs, nullptr, nullptr);
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
