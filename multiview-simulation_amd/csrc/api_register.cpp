// C ABI of libmvsim, part 7: the bead registration (mvsim.h states the recipe) -- nearest neighbours, geometric descriptors, ratio-test
// matching, RANSAC and the affine refit.  Host orchestration only: workspaces, launches of register.hip on the context's stream; no
// entry point reads a count back, so detection and registration chain without a synchronisation.
// Every argument is checked before the context is touched, so each refusal can be reached without a device.
#include "api_internal.h"
#include "register.h"
#include "register_dev.h"

namespace mvsim {

namespace {

enum { REG_STAGES = 0, REG_PARTIALS, REG_BEST, REG_RANSAC };

int check_list(const void* pos, int64_t stride, const void* n_dev, int64_t capacity)
{
    MVSIM_CHECK_ARG(pos && n_dev, "register: null pointer");
    MVSIM_CHECK_ARG(stride >= 24 && stride % 8 == 0, "register: stride must be >= 24 and a multiple of 8");
    MVSIM_CHECK_ARG(capacity >= 1 && capacity <= MVSIM_REG_MAX_POINTS, "register: capacity must be 1 .. MVSIM_REG_MAX_POINTS");
    return MVSIM_OK;
}

int check_redundancy(int redundancy)
{
    MVSIM_CHECK_ARG(redundancy >= 0 && redundancy <= 2, "register: redundancy must be 0 .. 2");
    return MVSIM_OK;
}

int check_ratio(double ratio)
{
    MVSIM_CHECK_ARG(std::isfinite(ratio) && ratio >= 1.0, "register: ratio must be finite and >= 1");
    return MVSIM_OK;
}

int check_params(const mvsim_match_params* p)
{
    MVSIM_CHECK_ARG(p != nullptr, "register: params is null");
    MVSIM_TRY(check_redundancy(p->redundancy));
    MVSIM_TRY(check_ratio(p->ratio));
    MVSIM_CHECK_ARG(std::isfinite(p->max_epsilon) && p->max_epsilon > 0.0, "register: max_epsilon must be finite and > 0");
    MVSIM_CHECK_ARG(std::isfinite(p->min_inlier_ratio), "register: min_inlier_ratio must be finite");
    MVSIM_CHECK_ARG(p->hypotheses >= 1, "register: hypotheses must be >= 1");
    MVSIM_CHECK_ARG(p->max_refits >= 0 && p->max_refits <= MVSIM_REG_MAX_REFITS, "register: max_refits must be 0 .. MVSIM_REG_MAX_REFITS");
    MVSIM_CHECK_ARG(p->min_inliers >= 4, "register: min_inliers must be >= 4");
    return MVSIM_OK;
}

RegList list_of(const void* pos, int64_t stride, const int64_t* n_dev, int64_t capacity)
{
    return RegList{reinterpret_cast<const char*>(pos), (long long)stride, reinterpret_cast<const long long*>(n_dev), (long long)capacity};
}

RegRansac ransac_of(const mvsim_match_params& p)
{
    return RegRansac{p.max_epsilon * p.max_epsilon, p.min_inlier_ratio, (long long)p.seed, p.hypotheses, p.max_refits, p.min_inliers};
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// bytes of split partials: k_knn's K best (d2 then indices) and k_match's two best per lane and split
size_t knn_partial_bytes(int64_t capacity, int K, size_t* d2_bytes)
{
    const RegSplit g = reg_split(capacity, capacity, REG_KNN_TILE);
    const size_t entries = (size_t)g.splits * (size_t)capacity * K;
    *d2_bytes = align256(entries * sizeof(double));
    return *d2_bytes + entries * sizeof(int);
}

size_t match_partial_bytes(int64_t cap_a, int64_t cap_b, int S)
{
    return (size_t)reg_split(cap_a * S, cap_b, REG_MATCH_TILE).splits * (size_t)cap_a * S * sizeof(RegTop2);
}

int knn_enqueue(mvsim_ctx* ctx, const RegList& L, int K, int32_t* idx, double* d2)
{
    const RegSplit g = reg_split(L.capacity, L.capacity, REG_KNN_TILE);
    size_t d2_bytes = 0;
    MVSIM_TRY(ctx->register_buf[REG_PARTIALS].reserve(knn_partial_bytes(L.capacity, K, &d2_bytes)));
    char* base = ctx->register_buf[REG_PARTIALS].as<char>();
    return launch_knn(ctx->stream, L, K, g, reinterpret_cast<double*>(base), reinterpret_cast<int*>(base + d2_bytes), idx, d2);
}

int match_enqueue(mvsim_ctx* ctx, const double* desc_a, const int64_t* n_a, int64_t cap_a, const double* desc_b, const int64_t* n_b,
                  int64_t cap_b, int K, double ratio, int64_t capacity, mvsim_match* cand, int64_t* n_cand)
{
    const int S = reg_subset_count(K);
    const RegSplit g = reg_split(cap_a * S, cap_b, REG_MATCH_TILE);
    MVSIM_TRY(ctx->register_buf[REG_PARTIALS].reserve(match_partial_bytes(cap_a, cap_b, S)));
    MVSIM_TRY(ctx->register_buf[REG_BEST].reserve((size_t)cap_a * sizeof(mvsim_match)));
    return launch_match(ctx->stream, desc_a, reinterpret_cast<const long long*>(n_a), cap_a, desc_b, reinterpret_cast<const long long*>(n_b), cap_b,
                        K, ratio * ratio, g, ctx->register_buf[REG_PARTIALS].as<RegTop2>(), ctx->register_buf[REG_BEST].as<mvsim_match>(),
                        capacity, cand, reinterpret_cast<long long*>(n_cand));
}

int ransac_enqueue(mvsim_ctx* ctx, const RegList& A, const RegList& B, const mvsim_match* cand, const int64_t* n_cand, int64_t capacity,
                   const mvsim_match_params& p, mvsim_registration* result, unsigned char* mask)
{
    const size_t pq_bytes = align256((size_t)capacity * 6 * sizeof(double));
    MVSIM_TRY(ctx->register_buf[REG_RANSAC].reserve(pq_bytes + 256 + (size_t)capacity));
    char* base = ctx->register_buf[REG_RANSAC].as<char>();
    return launch_ransac(ctx->stream, A, B, cand, reinterpret_cast<const long long*>(n_cand), capacity, ransac_of(p),
                         reinterpret_cast<double*>(base), reinterpret_cast<unsigned long long*>(base + pq_bytes),
                         mask ? mask : reinterpret_cast<unsigned char*>(base + pq_bytes + 256), result);
}

// a host block into a workspace of `reserve` bytes on the context's stream (an empty list copies nothing)
int put(mvsim_ctx* ctx, DevBuf& b, const void* h, size_t reserve, size_t bytes)
{
    MVSIM_TRY(b.reserve(reserve));
    if (bytes) MVSIM_HIP(hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return MVSIM_OK;
}

struct HostPairs {               // the items of reg_fit_walk over the caller's arrays
    const double* p;
    const double* q;
    const unsigned char* mask;
    int n;
    int count() const { return n; }
    int index(int k) const { return k; }
    bool selected(int k) const { return !mask || mask[k] != 0; }
    void load(int k, double pq[6]) const
    {
        for (int t = 0; t < 3; ++t) { pq[t] = p[3 * (size_t)k + t]; pq[3 + t] = q[3 * (size_t)k + t]; }
    }
};

}  // namespace

}  // namespace mvsim

using namespace mvsim;

extern "C" {

void mvsim_match_params_default(mvsim_match_params* p)
{
    if (!p) return;
    p->ratio = 3.0;
    p->max_epsilon = 5.0;
    p->min_inlier_ratio = 0.1;
    p->seed = 0;
    p->redundancy = 1;
    p->hypotheses = 10000;
    p->max_refits = 8;
    p->min_inliers = 12;
}

int mvsim_match_geometry(int64_t capacity_a, int64_t capacity_b, int redundancy, int64_t out[8])
{
    MVSIM_CHECK_ARG(out != nullptr, "null pointer");
    MVSIM_CHECK_ARG(capacity_a >= 1 && capacity_a <= MVSIM_REG_MAX_POINTS && capacity_b >= 1 && capacity_b <= MVSIM_REG_MAX_POINTS,
                    "register: capacity must be 1 .. MVSIM_REG_MAX_POINTS");
    MVSIM_TRY(check_redundancy(redundancy));
    const RegSplit k = reg_split(capacity_a, capacity_a, REG_KNN_TILE);
    const RegSplit m = reg_split(capacity_a * reg_subset_count(3 + redundancy), capacity_b, REG_MATCH_TILE);
    out[0] = REG_QUERIES; out[1] = REG_KNN_TILE; out[2] = k.splits; out[3] = k.tiles_per_split;
    out[4] = REG_MATCH_TILE; out[5] = m.splits; out[6] = m.tiles_per_split; out[7] = REG_RANSAC_TILE;
    return MVSIM_OK;
}

int mvsim_descriptor_subsets(int redundancy, int32_t* triples, int* n_subsets)
{
    MVSIM_CHECK_ARG(triples && n_subsets, "register: null pointer");
    MVSIM_TRY(check_redundancy(redundancy));
    const int K = 3 + redundancy, S = reg_subset_count(K);
    for (int s = 0; s < S; ++s) {
        int t[3] = {0, 0, 0};
        reg_subset(K, s, t);
        for (int k = 0; k < 3; ++k) triples[3 * s + k] = t[k];
    }
    *n_subsets = S;
    return MVSIM_OK;
}

int mvsim_fit_affine(const double* p, const double* q, const unsigned char* mask_or_null, int64_t n, double m[12], int* has_model)
{
    MVSIM_CHECK_ARG(p && q && m && has_model, "fit_affine: null pointer");
    MVSIM_CHECK_ARG(n >= 0 && n <= MVSIM_REG_MAX_POINTS, "fit_affine: n must be 0 .. MVSIM_REG_MAX_POINTS");
    const HostPairs items{p, q, mask_or_null, (int)n};
    double out[12];
    *has_model = reg_fit_walk(items, out) ? 1 : 0;
    if (*has_model) std::memcpy(m, out, sizeof(out));
    return MVSIM_OK;
}

int mvsim_knn_dev(mvsim_ctx* ctx, const void* pos_dev, int64_t stride, const int64_t* n_dev, int64_t capacity, int redundancy, int32_t* idx_dev,
                  double* d2_dev)
{
    MVSIM_TRY(check_list(pos_dev, stride, n_dev, capacity));
    MVSIM_CHECK_ARG(idx_dev && d2_dev, "register: null pointer");
    MVSIM_TRY(check_redundancy(redundancy));
    MVSIM_TRY(set_device(ctx));
    return knn_enqueue(ctx, list_of(pos_dev, stride, n_dev, capacity), 3 + redundancy, idx_dev, d2_dev);
}

int mvsim_bead_descriptors_dev(mvsim_ctx* ctx, const void* pos_dev, int64_t stride, const int64_t* n_dev, int64_t capacity, int redundancy,
                               const int32_t* idx_dev, double* desc_dev, int64_t* n_described_dev)
{
    MVSIM_TRY(check_list(pos_dev, stride, n_dev, capacity));
    MVSIM_CHECK_ARG(idx_dev && desc_dev && n_described_dev, "register: null pointer");
    MVSIM_TRY(check_redundancy(redundancy));
    MVSIM_TRY(set_device(ctx));
    return launch_descriptors(ctx->stream, list_of(pos_dev, stride, n_dev, capacity), 3 + redundancy, idx_dev, desc_dev,
                              reinterpret_cast<long long*>(n_described_dev));
}

int mvsim_match_descriptors_dev(mvsim_ctx* ctx, const double* desc_a_dev, const int64_t* n_a_dev, int64_t capacity_a, const double* desc_b_dev,
                                const int64_t* n_b_dev, int64_t capacity_b, int redundancy, double ratio, int64_t capacity,
                                mvsim_match* candidates_dev, int64_t* n_candidates_dev)
{
    MVSIM_TRY(check_list(desc_a_dev, 24, n_a_dev, capacity_a));
    MVSIM_TRY(check_list(desc_b_dev, 24, n_b_dev, capacity_b));
    MVSIM_CHECK_ARG(candidates_dev && n_candidates_dev, "register: null pointer");
    MVSIM_CHECK_ARG(capacity >= 1 && capacity <= MVSIM_REG_MAX_POINTS, "register: capacity must be 1 .. MVSIM_REG_MAX_POINTS");
    MVSIM_TRY(check_redundancy(redundancy));
    MVSIM_TRY(check_ratio(ratio));
    MVSIM_TRY(set_device(ctx));
    return match_enqueue(ctx, desc_a_dev, n_a_dev, capacity_a, desc_b_dev, n_b_dev, capacity_b, 3 + redundancy, ratio, capacity, candidates_dev,
                         n_candidates_dev);
}

int mvsim_ransac_affine_dev(mvsim_ctx* ctx, const void* pos_a_dev, int64_t stride_a, const int64_t* n_a_dev, int64_t capacity_a,
                            const void* pos_b_dev, int64_t stride_b, const int64_t* n_b_dev, int64_t capacity_b,
                            const mvsim_match* candidates_dev, const int64_t* n_candidates_dev, int64_t capacity, const mvsim_match_params* params,
                            mvsim_registration* result_dev, unsigned char* mask_dev_or_null)
{
    MVSIM_TRY(check_list(pos_a_dev, stride_a, n_a_dev, capacity_a));
    MVSIM_TRY(check_list(pos_b_dev, stride_b, n_b_dev, capacity_b));
    MVSIM_CHECK_ARG(candidates_dev && n_candidates_dev && result_dev, "register: null pointer");
    MVSIM_CHECK_ARG(capacity >= 1 && capacity <= MVSIM_REG_MAX_POINTS, "register: capacity must be 1 .. MVSIM_REG_MAX_POINTS");
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(set_device(ctx));
    return ransac_enqueue(ctx, list_of(pos_a_dev, stride_a, n_a_dev, capacity_a), list_of(pos_b_dev, stride_b, n_b_dev, capacity_b), candidates_dev,
                          n_candidates_dev, capacity, *params, result_dev, mask_dev_or_null);
}

int mvsim_register_beads_dev(mvsim_ctx* ctx, const void* pos_a_dev, int64_t stride_a, const int64_t* n_a_dev, int64_t capacity_a,
                             const void* pos_b_dev, int64_t stride_b, const int64_t* n_b_dev, int64_t capacity_b, const mvsim_match_params* params,
                             mvsim_registration* result_dev, mvsim_match* candidates_dev_or_null, unsigned char* mask_dev_or_null)
{
    MVSIM_TRY(check_list(pos_a_dev, stride_a, n_a_dev, capacity_a));
    MVSIM_TRY(check_list(pos_b_dev, stride_b, n_b_dev, capacity_b));
    MVSIM_CHECK_ARG(result_dev != nullptr, "register: null pointer");
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(set_device(ctx));
    // the lists between the stages, carved out of one workspace: per list the neighbours' indices and d2 and the descriptors; the
    // candidates; the three counts
    const int K = 3 + params->redundancy, S = reg_subset_count(K);
    const int64_t cap[2] = {capacity_a, capacity_b};
    size_t off = 0, idx_at[2], d2_at[2], desc_at[2];
    for (int l = 0; l < 2; ++l) {
        idx_at[l] = off;  off += align256((size_t)cap[l] * K * sizeof(int32_t));
        d2_at[l] = off;   off += align256((size_t)cap[l] * K * sizeof(double));
        desc_at[l] = off; off += align256((size_t)cap[l] * S * 6 * sizeof(double));
    }
    const size_t cand_at = off;  off += align256((size_t)capacity_a * sizeof(mvsim_match));
    const size_t counts_at = off; off += 256;
    MVSIM_TRY(ctx->register_buf[REG_STAGES].reserve(off));
    {   // the partials at the largest size of the three launches that share them, before the first: no stage grows them under another
        size_t unused = 0;
        const size_t knn = std::max(knn_partial_bytes(capacity_a, K, &unused), knn_partial_bytes(capacity_b, K, &unused));
        MVSIM_TRY(ctx->register_buf[REG_PARTIALS].reserve(std::max(knn, match_partial_bytes(capacity_a, capacity_b, S))));
    }
    char* base = ctx->register_buf[REG_STAGES].as<char>();
    int64_t* counts = reinterpret_cast<int64_t*>(base + counts_at);            // described in A, described in B, candidates
    const RegList lists[2] = {list_of(pos_a_dev, stride_a, n_a_dev, capacity_a), list_of(pos_b_dev, stride_b, n_b_dev, capacity_b)};
    for (int l = 0; l < 2; ++l) {
        int32_t* idx = reinterpret_cast<int32_t*>(base + idx_at[l]);
        MVSIM_TRY(knn_enqueue(ctx, lists[l], K, idx, reinterpret_cast<double*>(base + d2_at[l])));
        MVSIM_TRY(launch_descriptors(ctx->stream, lists[l], K, idx, reinterpret_cast<double*>(base + desc_at[l]),
                                     reinterpret_cast<long long*>(counts + l)));
    }
    mvsim_match* cand = candidates_dev_or_null ? candidates_dev_or_null : reinterpret_cast<mvsim_match*>(base + cand_at);
    MVSIM_TRY(match_enqueue(ctx, reinterpret_cast<const double*>(base + desc_at[0]), n_a_dev, capacity_a,
                            reinterpret_cast<const double*>(base + desc_at[1]), n_b_dev, capacity_b, K, params->ratio, capacity_a, cand, counts + 2));
    MVSIM_TRY(ransac_enqueue(ctx, lists[0], lists[1], cand, counts + 2, capacity_a, *params, result_dev, mask_dev_or_null));
    return launch_set_counts(ctx->stream, reinterpret_cast<const long long*>(counts), reinterpret_cast<const long long*>(counts + 1), result_dev);
}

int mvsim_register_beads(mvsim_ctx* ctx, const void* pos_a, int64_t stride_a, int64_t n_a, const void* pos_b, int64_t stride_b, int64_t n_b,
                         const mvsim_match_params* params, mvsim_registration* result, mvsim_match* candidates_or_null, unsigned char* mask_or_null)
{
    const int64_t cap_a = std::max<int64_t>(n_a, 1), cap_b = std::max<int64_t>(n_b, 1);
    const int64_t dummy = 0;
    MVSIM_CHECK_ARG(n_a >= 0 && n_b >= 0, "register: n must be >= 0");
    MVSIM_TRY(check_list(pos_a, stride_a, &dummy, cap_a));
    MVSIM_TRY(check_list(pos_b, stride_b, &dummy, cap_b));
    MVSIM_CHECK_ARG(result != nullptr, "register: null pointer");
    MVSIM_TRY(check_params(params));
    MVSIM_TRY(set_device(ctx));
    // device twins for this call only: the two lists, their counts, and the result with the candidates and the mask behind it
    const size_t cand_bytes = align256((size_t)cap_a * sizeof(mvsim_match));
    const int64_t counts[2] = {n_a, n_b};                                      // read by the copy until the call's last synchronise
    DevBuf da, db, dn, dout;
    int rc = put(ctx, da, pos_a, (size_t)cap_a * stride_a, (size_t)n_a * stride_a);
    if (rc == MVSIM_OK) rc = put(ctx, db, pos_b, (size_t)cap_b * stride_b, (size_t)n_b * stride_b);
    if (rc == MVSIM_OK) rc = put(ctx, dn, counts, sizeof(counts), sizeof(counts));
    if (rc == MVSIM_OK) rc = dout.reserve(256 + cand_bytes + (size_t)cap_a);
    char* out = dout.as<char>();
    if (rc == MVSIM_OK)
        rc = mvsim_register_beads_dev(ctx, da.p, stride_a, dn.as<int64_t>(), cap_a, db.p, stride_b, dn.as<int64_t>() + 1, cap_b, params,
                                      reinterpret_cast<mvsim_registration*>(out), reinterpret_cast<mvsim_match*>(out + 256),
                                      reinterpret_cast<unsigned char*>(out + 256 + cand_bytes));
    if (rc == MVSIM_OK) rc = down(ctx, reinterpret_cast<float*>(result), out, sizeof(mvsim_registration));
    if (rc == MVSIM_OK) {
        const size_t listed = (size_t)std::min<int64_t>(std::max<int64_t>(result->n_candidates, 0), cap_a);
        if (listed > 0 && candidates_or_null) rc = down(ctx, reinterpret_cast<float*>(candidates_or_null), out + 256, listed * sizeof(mvsim_match));
        if (rc == MVSIM_OK && listed > 0 && mask_or_null) rc = down(ctx, reinterpret_cast<float*>(mask_or_null), out + 256 + cand_bytes, listed);
    }
    (void)hipStreamSynchronize(ctx->stream);
    for (DevBuf* b : {&da, &db, &dn, &dout}) b->release();
    return rc;
}

}  // extern "C"
