// The kernels of the bead registration (gfx950, wave64; api_register.cpp drives them; mvsim.h and DESIGN.md section 18 state the recipe):
//   k_knn          one wave of REG_QUERIES query lanes per block, the list's points staged through LDS REG_KNN_TILE at a time and read
//                  back as broadcasts; a lane keeps its K best (d2, index) sorted in registers.  blockIdx.y splits the staged range, every
//                  split leaves its K best, k_knn_merge folds them: (d2, index) is a total order, so any split gives the same bits.
//   k_descriptors  one lane per (point, rank triple): six square roots.
//   k_match        the same shape over descriptors: one lane per descriptor of A, REG_MATCH_TILE points of B with all their descriptors
//                  staged per round; a lane keeps its two best B points under (v, index).  k_match_merge folds the S lanes of a point and
//                  the splits (the same point twice keeps its smaller v) and applies the ratio test, k_match_emit lists the candidates in
//                  ascending a: count, scan, emit in one block, no atomics.
//   k_ransac_*     gather the candidates' positions once; one lane per hypothesis, the pairs staged REG_RANSAC_TILE at a time, an integer
//                  atomicMax on (count, ~h) -- order-independent; one persistent block runs every refit round, a thread per chunk of
//                  REG_FIT_CHUNK candidates, and writes the result.  Nothing here is read back by the host.
// All fp64, every product and sum an operation of its own (the build has -ffp-contract=off); register_dev.h holds the arithmetic.
#include "common.h"
#include "register.h"
#include "register_dev.h"

namespace mvsim {

namespace {

__device__ __forceinline__ long long reg_count(const long long* n_dev, long long capacity)
{
    const long long n = *n_dev;
    return n < 0 ? 0 : (n < capacity ? n : capacity);
}

__device__ __forceinline__ const double* reg_point(const RegList& L, long long i)
{
    return reinterpret_cast<const double*>(L.pos + i * L.stride);
}

// keep the K smallest of what has been offered, sorted
template <int K> __device__ __forceinline__ void reg_offer(double (&bd)[K], int (&bi)[K], double d, int j)
{
    if (!reg_less(d, j, bd[K - 1], bi[K - 1])) return;
    bd[K - 1] = d; bi[K - 1] = j;
#pragma unroll
    for (int r = K - 1; r > 0; --r)
        if (reg_less(bd[r], bi[r], bd[r - 1], bi[r - 1])) {
            const double td = bd[r]; bd[r] = bd[r - 1]; bd[r - 1] = td;
            const int ti = bi[r]; bi[r] = bi[r - 1]; bi[r - 1] = ti;
        }
}

template <int K>
__global__ __launch_bounds__(REG_QUERIES) void k_knn(RegList L, int tiles, int tiles_per_split, double* __restrict__ part_d2,
                                                     int* __restrict__ part_idx)
{
    __shared__ double sx[REG_KNN_TILE], sy[REG_KNN_TILE], sz[REG_KNN_TILE];
    __shared__ int sok[REG_KNN_TILE];
    const int tid = threadIdx.x;
    const int n = (int)reg_count(L.n_dev, L.capacity);
    if ((int)blockIdx.x * REG_QUERIES >= n) return;      // uniform
    const int q = blockIdx.x * REG_QUERIES + tid;
    const bool have = q < n;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (have) { const double* p = reg_point(L, q); px = p[0]; py = p[1]; pz = p[2]; }
    const bool mine = have && reg_finite3(px, py, pz);
    double bd[K];
    int bi[K];
#pragma unroll
    for (int r = 0; r < K; ++r) { bd[r] = reg_inf(); bi[r] = REG_EMPTY; }
    const int t0 = blockIdx.y * tiles_per_split, t1 = min(t0 + tiles_per_split, tiles);
    for (int t = t0; t < t1; ++t) {
        const int base = t * REG_KNN_TILE;
        if (base >= n) break;                            // uniform
        __syncthreads();
        for (int jj = tid; jj < REG_KNN_TILE; jj += REG_QUERIES) {
            const int j = base + jj;
            double x = 0.0, y = 0.0, z = 0.0;
            if (j < n) { const double* p = reg_point(L, j); x = p[0]; y = p[1]; z = p[2]; }
            sx[jj] = x; sy[jj] = y; sz[jj] = z;
            sok[jj] = j < n && reg_finite3(x, y, z);
        }
        __syncthreads();
        const int cnt = min(REG_KNN_TILE, n - base);
        for (int jj = 0; jj < cnt; ++jj) {
            if (!sok[jj]) continue;                      // uniform
            const int j = base + jj;
            const double d = reg_d2(px, py, pz, sx[jj], sy[jj], sz[jj]);
            if (mine && j != q) reg_offer<K>(bd, bi, d, j);
        }
    }
    if (!have) return;
    const long long at = ((long long)blockIdx.y * L.capacity + q) * K;
#pragma unroll
    for (int r = 0; r < K; ++r) { part_d2[at + r] = bd[r]; part_idx[at + r] = bi[r]; }
}

// splits that staged nothing (their first point is at or past n) wrote nothing and are not read
template <int K>
__global__ __launch_bounds__(256) void k_knn_merge(const long long* __restrict__ n_dev, long long capacity, int splits, int tiles_per_split,
                                                   const double* __restrict__ part_d2, const int* __restrict__ part_idx,
                                                   int32_t* __restrict__ idx, double* __restrict__ d2)
{
    const int n = (int)reg_count(n_dev, capacity);
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    double bd[K];
    int bi[K];
#pragma unroll
    for (int r = 0; r < K; ++r) { bd[r] = reg_inf(); bi[r] = REG_EMPTY; }
    for (int s = 0; s < splits; ++s) {
        if ((long long)s * tiles_per_split * REG_KNN_TILE >= n) break;
        const long long at = ((long long)s * capacity + q) * K;
#pragma unroll
        for (int r = 0; r < K; ++r) reg_offer<K>(bd, bi, part_d2[at + r], part_idx[at + r]);
    }
#pragma unroll
    for (int r = 0; r < K; ++r) {
        idx[(long long)q * K + r] = bi[r] == REG_EMPTY ? -1 : bi[r];
        d2[(long long)q * K + r] = bd[r];
    }
}

__global__ __launch_bounds__(256) void k_descriptors(RegList L, int K, int S, const int32_t* __restrict__ idx, double* __restrict__ desc)
{
    const int n = (int)reg_count(L.n_dev, L.capacity);
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(g / S), s = (int)(g - (long long)i * S);
    if (i >= n) return;
    double* out = desc + g * 6;
    bool described = true;
    for (int r = 0; r < K; ++r) {
        const int j = idx[(long long)i * K + r];
        described = described && j >= 0 && j < n;        // a caller's index list may hold anything
    }
    if (!described) {
        for (int t = 0; t < 6; ++t) out[t] = reg_nan();
        return;
    }
    int tr[3] = {0, 1, 2};
    reg_subset(K, s, tr);
    const double* p = reg_point(L, i);
    const double* a = reg_point(L, idx[(long long)i * K + tr[0]]);
    const double* b = reg_point(L, idx[(long long)i * K + tr[1]]);
    const double* c = reg_point(L, idx[(long long)i * K + tr[2]]);
    out[0] = sqrt(reg_d2(p[0], p[1], p[2], a[0], a[1], a[2]));
    out[1] = sqrt(reg_d2(p[0], p[1], p[2], b[0], b[1], b[2]));
    out[2] = sqrt(reg_d2(p[0], p[1], p[2], c[0], c[1], c[2]));
    out[3] = sqrt(reg_d2(a[0], a[1], a[2], b[0], b[1], b[2]));
    out[4] = sqrt(reg_d2(a[0], a[1], a[2], c[0], c[1], c[2]));
    out[5] = sqrt(reg_d2(b[0], b[1], b[2], c[0], c[1], c[2]));
}

__global__ __launch_bounds__(256) void k_count_described(const long long* __restrict__ n_dev, long long capacity, int S,
                                                         const double* __restrict__ desc, long long* __restrict__ n_described)
{
    __shared__ int total;
    const int n = (int)reg_count(n_dev, capacity);
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double v = desc[(long long)i * S * 6];
        mine += v == v;
    }
    atomicAdd(&total, mine);                             // integers: any order, one sum
    __syncthreads();
    if (threadIdx.x == 0) *n_described = total;
}

// ---- matching ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void reg_top2_offer(RegTop2& t, double v, int b)
{
    if (b == REG_EMPTY) return;
    if (b == t.b1) { if (v < t.v1) t.v1 = v; return; }
    if (b == t.b2) {
        if (v < t.v2) t.v2 = v;
        if (reg_less(t.v2, t.b2, t.v1, t.b1)) {
            const double tv = t.v1; t.v1 = t.v2; t.v2 = tv;
            const int tb = t.b1; t.b1 = t.b2; t.b2 = tb;
        }
        return;
    }
    if (reg_less(v, b, t.v1, t.b1)) { t.v2 = t.v1; t.b2 = t.b1; t.v1 = v; t.b1 = b; }
    else if (reg_less(v, b, t.v2, t.b2)) { t.v2 = v; t.b2 = b; }
}

template <int S>
__global__ __launch_bounds__(REG_QUERIES) void k_match(const double* __restrict__ desc_a, const long long* __restrict__ n_a_dev, long long cap_a,
                                                       const double* __restrict__ desc_b, const long long* __restrict__ n_b_dev, long long cap_b,
                                                       int tiles, int tiles_per_split, RegTop2* __restrict__ part)
{
    __shared__ double sw[REG_MATCH_TILE * S * 6];
    const int tid = threadIdx.x;
    const int n_a = (int)reg_count(n_a_dev, cap_a), n_b = (int)reg_count(n_b_dev, cap_b);
    const long long lanes = (long long)n_a * S;
    if ((long long)blockIdx.x * REG_QUERIES >= lanes) return;   // uniform
    const long long g = (long long)blockIdx.x * REG_QUERIES + tid;
    const bool have = g < lanes;
    double u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (have)
#pragma unroll
        for (int t = 0; t < 6; ++t) u[t] = desc_a[g * 6 + t];
    const bool mine = have && u[0] == u[0];
    RegTop2 best = {reg_inf(), reg_inf(), REG_EMPTY, REG_EMPTY};
    const int t0 = blockIdx.y * tiles_per_split, t1 = min(t0 + tiles_per_split, tiles);
    for (int t = t0; t < t1; ++t) {
        const int base = t * REG_MATCH_TILE;
        if (base >= n_b) break;                          // uniform
        const int cnt = min(REG_MATCH_TILE, n_b - base);
        __syncthreads();
        for (int k = tid; k < cnt * S * 6; k += REG_QUERIES) sw[k] = desc_b[(long long)base * S * 6 + k];
        __syncthreads();
        for (int bb = 0; bb < cnt; ++bb) {
            const double* w = sw + bb * S * 6;
            if (!(w[0] == w[0])) continue;               // uniform: this point of B has no descriptors
            double v = reg_inf();
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double d = reg_desc_dist(u, w + 6 * s);
                if (d < v) v = d;
            }
            if (mine) reg_top2_offer(best, v, base + bb);
        }
    }
    if (have) part[(long long)blockIdx.y * (cap_a * S) + g] = best;
}

__global__ __launch_bounds__(256) void k_match_merge(const long long* __restrict__ n_a_dev, long long cap_a, const long long* __restrict__ n_b_dev,
                                                     long long cap_b, int S, int splits, int tiles_per_split, const RegTop2* __restrict__ part,
                                                     double ratio2, mvsim_match* __restrict__ best)
{
    const int n_a = (int)reg_count(n_a_dev, cap_a), n_b = (int)reg_count(n_b_dev, cap_b);
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n_a) return;
    RegTop2 t = {reg_inf(), reg_inf(), REG_EMPTY, REG_EMPTY};
    for (int sp = 0; sp < splits; ++sp) {
        if ((long long)sp * tiles_per_split * REG_MATCH_TILE >= n_b) break;
        for (int s = 0; s < S; ++s) {
            const RegTop2 e = part[(long long)sp * (cap_a * S) + (long long)a * S + s];
            reg_top2_offer(t, e.v1, e.b1);
            reg_top2_offer(t, e.v2, e.b2);
        }
    }
    mvsim_match m;
    const bool yes = t.b2 != REG_EMPTY && t.v1 * ratio2 < t.v2;
    m.a = yes ? a : -1;
    m.b = yes ? t.b1 : -1;
    m.v_best = t.v1;
    m.v_second = t.v2;
    best[a] = m;
}

// one block: thread t owns the points [t per, (t + 1) per) -- counts them, the counts are scanned in LDS, and it emits its own in order
__global__ __launch_bounds__(256) void k_match_emit(const long long* __restrict__ n_a_dev, long long cap_a, const mvsim_match* __restrict__ best,
                                                    long long capacity, mvsim_match* __restrict__ candidates, long long* __restrict__ n_candidates)
{
    __shared__ int counts[256];
    const int tid = threadIdx.x;
    const int n_a = (int)reg_count(n_a_dev, cap_a);
    const int per = (n_a + 255) / 256;
    const int first = min(n_a, tid * per), last = min(n_a, first + per);
    int c = 0;
    for (int a = first; a < last; ++a) c += best[a].a >= 0;
    counts[tid] = c;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < tid; ++k) before += counts[k];
    if (tid == 255) *n_candidates = before + c;
    for (int a = first; a < last; ++a) {
        const mvsim_match m = best[a];
        if (m.a < 0) continue;
        if (before < capacity) candidates[before] = m;
        ++before;
    }
}

// ---- RANSAC and refit -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ransac_gather(RegList A, RegList B, const mvsim_match* __restrict__ cand, const long long* __restrict__ n_cand,
                                                       long long capacity, double* __restrict__ pq)
{
    const int M = (int)reg_count(n_cand, capacity);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const long long n_a = reg_count(A.n_dev, A.capacity), n_b = reg_count(B.n_dev, B.capacity);
    const int a = cand[i].a, b = cand[i].b;
    const bool ok = a >= 0 && a < n_a && b >= 0 && b < n_b;
    double* out = pq + (long long)i * 6;
    if (ok) {
        const double* p = reg_point(A, a);
        const double* q = reg_point(B, b);
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = q[0]; out[4] = q[1]; out[5] = q[2];
    } else {
        for (int t = 0; t < 6; ++t) out[t] = reg_nan();
    }
}

// the model of hypothesis h over M >= 4 gathered pairs; false: void or no model
__device__ __forceinline__ bool reg_hypothesis(long long seed, long long h, int M, const double* __restrict__ pq, double m[12])
{
    RegFour four;
    if (!reg_draw4(seed, h, M, four.idx)) return false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int t = 0; t < 6; ++t) four.pq[k][t] = pq[(long long)four.idx[k] * 6 + t];
    return reg_fit_walk(four, m);
}

__global__ __launch_bounds__(REG_QUERIES) void k_ransac_hypotheses(const long long* __restrict__ n_cand, long long capacity, RegRansac R,
                                                                   const double* __restrict__ pq, unsigned long long* __restrict__ key)
{
    __shared__ double spq[REG_RANSAC_TILE * 6];
    const int tid = threadIdx.x;
    const int M = (int)reg_count(n_cand, capacity);
    if (M < 4) return;                                   // uniform
    const int h = blockIdx.x * REG_QUERIES + tid;
    double m[12];
    for (int t = 0; t < 12; ++t) m[t] = reg_nan();
    const bool model = h < R.hypotheses && reg_hypothesis(R.seed, h, M, pq, m);
    int count = 0;
    for (int base = 0; base < M; base += REG_RANSAC_TILE) {
        const int cnt = min(REG_RANSAC_TILE, M - base);
        __syncthreads();
        for (int k = tid; k < cnt * 6; k += REG_QUERIES) spq[k] = pq[(long long)base * 6 + k];
        __syncthreads();
        for (int i = 0; i < cnt; ++i) count += reg_residual2(m, spq + 6 * i) <= R.eps2;
    }
    if (model && count > 0) atomicMax(key, ((unsigned long long)count << 32) | (unsigned long long)(0xffffffffu - (unsigned)h));
}

constexpr int REFIT_THREADS = 256;                       // >= MVSIM_REG_MAX_POINTS / REG_FIT_CHUNK chunks: a thread per chunk

// sums[c][0 .. terms) of chunk c = tid left in LDS by every thread; thread 0 adds them ascending into total[]
__device__ __forceinline__ void reg_add_chunks(double (*sums)[16], int chunks, int terms, double* total)
{
    for (int t = 0; t < terms; ++t) total[t] = 0.0;
    for (int c = 0; c < chunks; ++c)
        for (int t = 0; t < terms; ++t) total[t] = total[t] + sums[c][t];
}

__global__ __launch_bounds__(REFIT_THREADS) void k_ransac_refit(const long long* __restrict__ n_cand, long long capacity, RegRansac R,
                                                                const double* __restrict__ pq, const unsigned long long* __restrict__ key,
                                                                unsigned char* mask, mvsim_registration* __restrict__ result)
{
    __shared__ double sums[REFIT_THREADS][16];
    __shared__ double sh_m[12], sh_cen[6];
    __shared__ int sh_cnt[REFIT_THREADS];
    __shared__ int sh_ok, sh_changed;
    __shared__ long long sh_best;
    const int tid = threadIdx.x;
    const long long total_cand = *n_cand < 0 ? 0 : *n_cand;
    const int M = (int)reg_count(n_cand, capacity);
    const int chunks = (M + REG_FIT_CHUNK - 1) / REG_FIT_CHUNK;
    const int c0 = tid * REG_FIT_CHUNK, c1 = min(M, c0 + REG_FIT_CHUNK);     // this thread's chunk (empty past the last)
    int flags = M < 4 ? MVSIM_REG_FEW_CANDIDATES : 0;
    int refits = 0;

    if (tid == 0) {
        const unsigned long long k = M < 4 ? 0ull : *key;
        const long long count = (long long)(k >> 32), h = (long long)(0xffffffffu - (unsigned)(k & 0xffffffffull));
        sh_ok = 0;
        sh_best = -1;
        double m[12];
        if (count >= 4 && reg_hypothesis(R.seed, h, M, pq, m)) {
            sh_ok = 1;
            sh_best = h;
            for (int t = 0; t < 12; ++t) sh_m[t] = m[t];
        } else {
            for (int t = 0; t < 12; ++t) sh_m[t] = reg_nan();
        }
    }
    __syncthreads();
    const bool have_model = sh_ok != 0;
    if (!have_model) flags |= MVSIM_REG_NO_MODEL;
    for (int i = tid; i < M; i += REFIT_THREADS) mask[i] = have_model && reg_residual2(sh_m, pq + (long long)i * 6) <= R.eps2;
    __syncthreads();

    while (have_model) {                                 // every condition below is uniform
        if (refits == R.max_refits) { flags |= MVSIM_REG_CAPPED; break; }
        // centroids
        {
            double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            int cnt = 0;
            for (int i = c0; i < c1; ++i)
                if (mask[i]) { reg_acc_centroid(acc, pq + (long long)i * 6); ++cnt; }
            for (int t = 0; t < 6; ++t) sums[tid][t] = acc[t];
            sh_cnt[tid] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            double total[6];
            reg_add_chunks(sums, chunks, 6, total);
            long long n = 0;
            for (int c = 0; c < chunks; ++c) n += sh_cnt[c];
            sh_ok = n >= 4;
            if (sh_ok) reg_centroid(total, n, sh_cen);
        }
        __syncthreads();
        if (!sh_ok) { flags |= MVSIM_REG_NO_MODEL; break; }
        // moments
        {
            double acc[15], cen[6];
            for (int t = 0; t < 15; ++t) acc[t] = 0.0;
            for (int t = 0; t < 6; ++t) cen[t] = sh_cen[t];
            for (int i = c0; i < c1; ++i)
                if (mask[i]) reg_acc_moments(acc, pq + (long long)i * 6, cen);
            for (int t = 0; t < 15; ++t) sums[tid][t] = acc[t];
        }
        __syncthreads();
        if (tid == 0) {
            double total[15], m[12];
            reg_add_chunks(sums, chunks, 15, total);
            sh_ok = reg_solve(sh_cen, total, m);
            if (sh_ok)
                for (int t = 0; t < 12; ++t) sh_m[t] = m[t];
            sh_changed = 0;
        }
        __syncthreads();
        if (!sh_ok) { flags |= MVSIM_REG_NO_MODEL; break; }
        refits += 1;
        for (int i = tid; i < M; i += REFIT_THREADS) {
            const unsigned char now = reg_residual2(sh_m, pq + (long long)i * 6) <= R.eps2;
            if (now != mask[i]) { mask[i] = now; sh_changed = 1; }
        }
        __syncthreads();
        const bool changed = sh_changed != 0;
        __syncthreads();                                 // before thread 0 clears it again
        if (!changed) break;
    }

    // the inliers' errors: the sum as every sum of the fit, the maximum in sums[][1]
    {
        double sum = 0.0, mx = 0.0;
        int cnt = 0;
        for (int i = c0; i < c1; ++i)
            if (mask[i]) {
                const double e = sqrt(reg_residual2(sh_m, pq + (long long)i * 6));
                sum = sum + e;
                mx = e > mx ? e : mx;
                ++cnt;
            }
        sums[tid][0] = sum; sums[tid][1] = mx;
        sh_cnt[tid] = cnt;
    }
    __syncthreads();
    if (tid != 0) return;
    double sum = 0.0, mx = 0.0;
    long long n = 0;
    for (int c = 0; c < chunks; ++c) {
        sum = sum + sums[c][0];
        mx = sums[c][1] > mx ? sums[c][1] : mx;
        n += sh_cnt[c];
    }
    if (n < R.min_inliers || (double)n < R.min_inlier_ratio * (double)M) flags |= MVSIM_REG_FEW_INLIERS;
    mvsim_registration out;
    for (int t = 0; t < 12; ++t) out.m[t] = sh_m[t];
    out.mean_error = n > 0 ? sum / (double)n : reg_nan();
    out.max_error = n > 0 ? mx : reg_nan();
    out.n_a = 0; out.n_b = 0;
    out.n_candidates = total_cand;
    out.n_inliers = n;
    out.best_hypothesis = sh_best;
    out.refits = refits;
    out.flags = flags;
    *result = out;
}

__global__ void k_set_counts(const long long* __restrict__ n_desc_a, const long long* __restrict__ n_desc_b, mvsim_registration* __restrict__ result)
{
    result->n_a = *n_desc_a;
    result->n_b = *n_desc_b;
}

}  // namespace

int launch_knn(hipStream_t s, const RegList& L, int K, const RegSplit& g, double* part_d2, int* part_idx, int32_t* idx, double* d2)
{
    const dim3 grid((unsigned)g.qblocks, (unsigned)g.splits), merge((unsigned)((L.capacity + 255) / 256));
    switch (K) {
    case 3:
        hipLaunchKernelGGL(k_knn<3>, grid, dim3(REG_QUERIES), 0, s, L, g.tiles, g.tiles_per_split, part_d2, part_idx);
        hipLaunchKernelGGL(k_knn_merge<3>, merge, dim3(256), 0, s, L.n_dev, L.capacity, g.splits, g.tiles_per_split, (const double*)part_d2,
                           (const int*)part_idx, idx, d2);
        break;
    case 4:
        hipLaunchKernelGGL(k_knn<4>, grid, dim3(REG_QUERIES), 0, s, L, g.tiles, g.tiles_per_split, part_d2, part_idx);
        hipLaunchKernelGGL(k_knn_merge<4>, merge, dim3(256), 0, s, L.n_dev, L.capacity, g.splits, g.tiles_per_split, (const double*)part_d2,
                           (const int*)part_idx, idx, d2);
        break;
    default:
        hipLaunchKernelGGL(k_knn<5>, grid, dim3(REG_QUERIES), 0, s, L, g.tiles, g.tiles_per_split, part_d2, part_idx);
        hipLaunchKernelGGL(k_knn_merge<5>, merge, dim3(256), 0, s, L.n_dev, L.capacity, g.splits, g.tiles_per_split, (const double*)part_d2,
                           (const int*)part_idx, idx, d2);
        break;
    }
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_descriptors(hipStream_t s, const RegList& L, int K, const int32_t* idx, double* desc, long long* n_described)
{
    const int S = reg_subset_count(K);
    const long long lanes = L.capacity * S;
    hipLaunchKernelGGL(k_descriptors, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, L, K, S, idx, desc);
    hipLaunchKernelGGL(k_count_described, dim3(1), dim3(256), 0, s, L.n_dev, L.capacity, S, (const double*)desc, n_described);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_match(hipStream_t s, const double* desc_a, const long long* n_a, long long cap_a, const double* desc_b, const long long* n_b,
                 long long cap_b, int K, double ratio2, const RegSplit& g, RegTop2* part, mvsim_match* best, long long capacity,
                 mvsim_match* candidates, long long* n_candidates)
{
    const int S = reg_subset_count(K);
    const dim3 grid((unsigned)g.qblocks, (unsigned)g.splits);
    switch (S) {
    case 1: hipLaunchKernelGGL(k_match<1>, grid, dim3(REG_QUERIES), 0, s, desc_a, n_a, cap_a, desc_b, n_b, cap_b, g.tiles, g.tiles_per_split, part); break;
    case 4: hipLaunchKernelGGL(k_match<4>, grid, dim3(REG_QUERIES), 0, s, desc_a, n_a, cap_a, desc_b, n_b, cap_b, g.tiles, g.tiles_per_split, part); break;
    default: hipLaunchKernelGGL(k_match<10>, grid, dim3(REG_QUERIES), 0, s, desc_a, n_a, cap_a, desc_b, n_b, cap_b, g.tiles, g.tiles_per_split, part); break;
    }
    hipLaunchKernelGGL(k_match_merge, dim3((unsigned)((cap_a + 255) / 256)), dim3(256), 0, s, n_a, cap_a, n_b, cap_b, S, g.splits, g.tiles_per_split,
                       (const RegTop2*)part, ratio2, best);
    hipLaunchKernelGGL(k_match_emit, dim3(1), dim3(256), 0, s, n_a, cap_a, (const mvsim_match*)best, capacity, candidates, n_candidates);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_ransac(hipStream_t s, const RegList& A, const RegList& B, const mvsim_match* cand, const long long* n_cand, long long capacity,
                  const RegRansac& R, double* pq, unsigned long long* key, unsigned char* mask, mvsim_registration* result)
{
    MVSIM_HIP(hipMemsetAsync(key, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_ransac_gather, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, s, A, B, cand, n_cand, capacity, pq);
    hipLaunchKernelGGL(k_ransac_hypotheses, dim3((unsigned)((R.hypotheses + REG_QUERIES - 1) / REG_QUERIES)), dim3(REG_QUERIES), 0, s, n_cand,
                       capacity, R, (const double*)pq, key);
    hipLaunchKernelGGL(k_ransac_refit, dim3(1), dim3(REFIT_THREADS), 0, s, n_cand, capacity, R, (const double*)pq,
                       (const unsigned long long*)key, mask, result);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

int launch_set_counts(hipStream_t s, const long long* n_desc_a, const long long* n_desc_b, mvsim_registration* result)
{
    hipLaunchKernelGGL(k_set_counts, dim3(1), dim3(1), 0, s, n_desc_a, n_desc_b, result);
    MVSIM_HIP(hipGetLastError());
    return MVSIM_OK;
}

}  // namespace mvsim
