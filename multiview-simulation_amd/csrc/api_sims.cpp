// C ABI of libmvsim, part 4: the simulators around the per-view pipeline -- the sphere phantom (phantom.hip), bead images
// (SimulateBeads / SimulateBeads2, beads.hip) and the refraction simulator (SimulateMultiViewAberrations, aberrations.hip).
// Arguments are checked here, before a device is touched; every check is stated once for a host entry point and its _dev twin.
#include "api_internal.h"
#include "jrandom.h"

using namespace mvsim;

extern "C" {

static int draw_spheres_args(mvsim_ctx* ctx, const float* img, const int64_t dim[3], int scale, const uint64_t* rnd_state)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(img && rnd_state, "null pointer");
    MVSIM_CHECK_ARG(scale >= 1 && scale <= 64, "scale must be in 1..64");
    return MVSIM_OK;
}

int mvsim_draw_spheres_dev(mvsim_ctx* ctx, float* img, const int64_t dim[3], double min_value, double max_value,
                           int scale, int half_pixel_offset, uint64_t* rnd_state, int64_t* n_spheres)
{
    MVSIM_TRY(draw_spheres_args(ctx, img, dim, scale, rnd_state));
    return draw_spheres_dev(ctx, img, dim, min_value, max_value, scale, half_pixel_offset, rnd_state, n_spheres);
}

int mvsim_downsample2x_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out && in != out, "null or aliased buffer");
    MVSIM_CHECK_ARG(dim[0] >= 4 && dim[1] >= 4 && dim[2] >= 4, "downSample2x needs at least 4 samples per dimension");
    return launch_downsample2x(ctx->stream, in, dim, out);
}

int mvsim_draw_spheres(mvsim_ctx* ctx, float* img, const int64_t dim[3], double min_value, double max_value,
                       int scale, int half_pixel_offset, uint64_t* rnd_state, int64_t* n_spheres)
{
    MVSIM_TRY(draw_spheres_args(ctx, img, dim, scale, rnd_state));
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(draw_spheres_dev(ctx, ctx->vol_a.as<float>(), dim, min_value, max_value, scale, half_pixel_offset, rnd_state, n_spheres));
    return down(ctx, img, ctx->vol_a.p, bytes);
}

int mvsim_downsample2x(mvsim_ctx* ctx, const float* in, const int64_t dim[3], float* out)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(in && out, "null buffer");
    MVSIM_CHECK_ARG(dim[0] >= 4 && dim[1] >= 4 && dim[2] >= 4, "downSample2x needs at least 4 samples per dimension");
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    const size_t obytes = (size_t)(dim[0] / 2 - 1) * (size_t)(dim[1] / 2 - 1) * (size_t)(dim[2] / 2 - 1) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, in, bytes));
    MVSIM_TRY(ctx->out_buf.reserve(obytes));
    MVSIM_TRY(mvsim_downsample2x_dev(ctx, ctx->vol_a.as<float>(), dim, ctx->out_buf.as<float>()));
    return down(ctx, out, ctx->out_buf.p, obytes);
}

static int splat_spheres_args(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const mvsim_sphere* spheres, int64_t n)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(img && (spheres || n == 0) && n >= 0, "null pointer or negative count");
    return MVSIM_OK;
}

int mvsim_splat_spheres_dev(mvsim_ctx* ctx, float* img, const int64_t dim[3], const mvsim_sphere* spheres, int64_t n)
{
    MVSIM_TRY(splat_spheres_args(ctx, img, dim, spheres, n));
    return splat_spheres_dev(ctx, img, dim, spheres, n);
}

int mvsim_splat_spheres(mvsim_ctx* ctx, float* img, const int64_t dim[3], const mvsim_sphere* spheres, int64_t n)
{
    MVSIM_TRY(splat_spheres_args(ctx, img, dim, spheres, n));
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(splat_spheres_dev(ctx, ctx->vol_a.as<float>(), dim, spheres, n));
    return down(ctx, img, ctx->vol_a.p, bytes);
}

// ---- the phantom of the refraction simulator: noise on the index volume, multiSpheres (phantom.hip, sphere_walk.hip) ----------------
int mvsim_sphere_walk_geometry(int64_t* chunk_positions, int* max_entry)
{
    MVSIM_CHECK_ARG(chunk_positions && max_entry, "null pointer");
    *chunk_positions = SW_CHUNK;
    *max_entry = SW_ENTRIES;
    return MVSIM_OK;
}

static int ri_noise_args(mvsim_ctx* ctx, const float* ri, int64_t n, const uint64_t* rnd_state)
{
    MVSIM_CHECK_ARG(rnd_state != nullptr, "null rnd_state");
    MVSIM_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 40) && (ri || n == 0), "null volume or count outside 0 .. 2^40");
    return set_device(ctx);
}

int mvsim_ri_noise_dev(mvsim_ctx* ctx, float* ri, int64_t n, uint64_t* rnd_state)
{
    MVSIM_TRY(ri_noise_args(ctx, ri, n, rnd_state));
    MVSIM_TRY(ri_noise_dev(ctx, ri, n, *rnd_state & JR_MASK));
    *rnd_state = jr_jump(*rnd_state & JR_MASK, 2 * (uint64_t)n);
    return MVSIM_OK;
}

int mvsim_ri_noise(mvsim_ctx* ctx, float* ri, int64_t n, uint64_t* rnd_state)
{
    MVSIM_TRY(ri_noise_args(ctx, ri, n, rnd_state));
    if (n > 0) {
        const size_t bytes = (size_t)n * sizeof(float);
        MVSIM_TRY(up(ctx, ctx->vol_a, ri, bytes));
        MVSIM_TRY(ri_noise_dev(ctx, ctx->vol_a.as<float>(), n, *rnd_state & JR_MASK));
        MVSIM_TRY(down(ctx, ri, ctx->vol_a.p, bytes));
    }
    *rnd_state = jr_jump(*rnd_state & JR_MASK, 2 * (uint64_t)n);
    return MVSIM_OK;
}

static int multi_spheres_args(mvsim_ctx* ctx, const float* img, const float* ri, const int64_t dim[3], int scale, const uint64_t* rnd_state)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(check_dim(dim));
    MVSIM_CHECK_ARG(img && ri && img != ri && rnd_state, "null pointer or aliased volumes");
    MVSIM_CHECK_ARG(scale >= 1 && scale <= 64, "scale must be in 1..64");
    return MVSIM_OK;
}

int mvsim_multi_spheres_dev(mvsim_ctx* ctx, float* img, float* ri, const int64_t dim[3], int scale, uint64_t* rnd_state, int64_t* n_spheres)
{
    MVSIM_TRY(multi_spheres_args(ctx, img, ri, dim, scale, rnd_state));
    return multi_spheres_dev(ctx, img, ri, dim, scale, rnd_state, n_spheres);
}

int mvsim_multi_spheres(mvsim_ctx* ctx, float* img, float* ri, const int64_t dim[3], int scale, uint64_t* rnd_state, int64_t* n_spheres)
{
    MVSIM_TRY(multi_spheres_args(ctx, img, ri, dim, scale, rnd_state));
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(up(ctx, ctx->vol_b, ri, bytes));
    MVSIM_TRY(multi_spheres_dev(ctx, ctx->vol_a.as<float>(), ctx->vol_b.as<float>(), dim, scale, rnd_state, n_spheres));
    MVSIM_HIP(hipMemcpyAsync(img, ctx->vol_a.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return down(ctx, ri, ctx->vol_b.p, bytes);
}

// ---- bead images: SimulateBeads / SimulateBeads2 (beads.hip) ----------------------------------------------------------
int mvsim_beads_random_points(uint64_t* rnd_state, int64_t n, const int64_t min[3], const int64_t max[3], double* xyz)
{
    MVSIM_CHECK_ARG(rnd_state && min && max && (xyz || n == 0), "null pointer");
    MVSIM_CHECK_ARG(n >= 0, "negative number of points");
    JRandom rnd{*rnd_state & JR_MASK};
    for (int64_t i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d)                                    // SimulateBeads.java:159-160
            xyz[3 * i + d] = rnd.next_double() * (double)(max[d] - min[d]) + (double)min[d];
    *rnd_state = rnd.s;
    return MVSIM_OK;
}

// the arguments first: their errors need no device
static int beads_check(mvsim_ctx* ctx, const double* xyz, const int64_t* view_offsets, int64_t n, const double* m12, int nviews, const int64_t min[3],
                       const int64_t max[3], const double sigma[3], float* const* out_f32, uint16_t* const* out_u16, int64_t dim[3])
{
    MVSIM_CHECK_ARG(min && max && sigma, "null interval or sigma");
    MVSIM_CHECK_ARG(n >= 0 && (xyz || n == 0), "null point list or negative count");
    MVSIM_CHECK_ARG(nviews >= 1, "renderBeads needs at least one view");
    MVSIM_CHECK_ARG(out_f32 || out_u16, "renderBeads: no output list");
    for (int d = 0; d < 3; ++d) {
        dim[d] = max[d] - min[d];                                      // SimulateBeads.java:105-106: one voxel less than the interval
        MVSIM_CHECK_ARG(dim[d] >= 1, "image dimension (interval max - min) must be >= 1");
        MVSIM_CHECK_ARG(std::isfinite(sigma[d]) && sigma[d] > 0.0, "sigma must be finite and > 0");
        MVSIM_CHECK_ARG(sigma[d] <= 1.0e4, "sigma must be <= 1e4");
    }
    MVSIM_CHECK_ARG(dim[0] <= (1 << 24) && dim[1] <= (1 << 24) && dim[2] <= (1 << 24), "image dimension too large");
    if (view_offsets) {
        MVSIM_CHECK_ARG(view_offsets[0] >= 0 && view_offsets[nviews] <= n, "view_offsets outside the point list");
        for (int v = 0; v < nviews; ++v) MVSIM_CHECK_ARG(view_offsets[v] <= view_offsets[v + 1], "view_offsets must not decrease");
    }
    if (m12)
        for (int64_t k = 0; k < 12 * (int64_t)nviews; ++k) MVSIM_CHECK_ARG(std::isfinite(m12[k]), "transform with a non-finite entry");
    for (int v = 0; v < nviews; ++v)
        MVSIM_CHECK_ARG((!out_f32 || out_f32[v]) && (!out_u16 || out_u16[v]), "renderBeads: null image in an output list");
    return set_device(ctx);
}

int mvsim_render_beads_dev(mvsim_ctx* ctx, const double* xyz, const int64_t* view_offsets, int64_t n, const double* m12, int nviews,
                           const int64_t min[3], const int64_t max[3], const double sigma[3], float* const* out_f32,
                           uint16_t* const* out_u16)
{
    int64_t dim[3];
    MVSIM_TRY(beads_check(ctx, xyz, view_offsets, n, m12, nviews, min, max, sigma, out_f32, out_u16, dim));
    return render_beads_dev(ctx, xyz, view_offsets, n, m12, nviews, dim, min, sigma, out_f32, out_u16);
}

int mvsim_render_beads(mvsim_ctx* ctx, const double* xyz, const int64_t* view_offsets, int64_t n, const double* m12, int nviews,
                       const int64_t min[3], const int64_t max[3], const double sigma[3], float* const* out_f32, uint16_t* const* out_u16)
{
    int64_t dim[3];
    MVSIM_TRY(beads_check(ctx, xyz, view_offsets, n, m12, nviews, min, max, sigma, out_f32, out_u16, dim));
    // device twins of the outputs: every view's float image in vol_a, its uint16 image in vol_b
    const size_t nv = (size_t)(dim[0] * dim[1] * dim[2]);
    std::vector<float*> df(nviews, nullptr);
    std::vector<uint16_t*> du(nviews, nullptr);
    if (out_f32) {
        MVSIM_TRY(ctx->vol_a.reserve(nv * sizeof(float) * nviews));
        for (int v = 0; v < nviews; ++v) df[v] = ctx->vol_a.as<float>() + nv * v;
    }
    if (out_u16) {
        MVSIM_TRY(ctx->vol_b.reserve(nv * sizeof(uint16_t) * nviews));
        for (int v = 0; v < nviews; ++v) du[v] = reinterpret_cast<uint16_t*>(ctx->vol_b.p) + nv * v;
    }
    MVSIM_TRY(render_beads_dev(ctx, xyz, view_offsets, n, m12, nviews, dim, min, sigma, out_f32 ? df.data() : nullptr,
                               out_u16 ? du.data() : nullptr));
    for (int v = 0; v < nviews; ++v) {
        if (out_f32) MVSIM_HIP(hipMemcpyAsync(out_f32[v], df[v], nv * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (out_u16) MVSIM_HIP(hipMemcpyAsync(out_u16[v], du[v], nv * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    MVSIM_HIP(hipStreamSynchronize(ctx->stream));
    return MVSIM_OK;
}

int mvsim_beads_normalize_dev(mvsim_ctx* ctx, float* img, int64_t n)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(img && n >= 1, "null image or empty count");
    return beads_normalize_dev(ctx, img, n);
}

int mvsim_beads_normalize(mvsim_ctx* ctx, float* img, int64_t n)
{
    MVSIM_TRY(set_device(ctx));
    MVSIM_CHECK_ARG(img && n >= 1, "null image or empty count");
    const size_t bytes = (size_t)n * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(beads_normalize_dev(ctx, ctx->vol_a.as<float>(), n));
    return down(ctx, img, ctx->vol_a.p, bytes);
}

// ---- the procedural phantom: Perlin field, sphere sets, rejection sampling (procedural.hip) ---------------------------------
int mvsim_perlin_init(uint64_t* rnd_state, int32_t n_vectors, double* gradients, int32_t* permutation, double* pending_gaussian)
{
    MVSIM_CHECK_ARG(rnd_state && gradients && permutation, "null pointer");
    MVSIM_CHECK_ARG(n_vectors >= 1, "n_vectors must be >= 1");
    JRandom rnd{*rnd_state & JR_MASK};
    double pending = pending_gaussian ? *pending_gaussian : std::nan("");
    for (int32_t i = 0; i < n_vectors; ++i) {                          // PerlinNoiseRealRandomAccessible.java:67-71, :99-111
        double* res = gradients + 3 * (size_t)i;
        double s_sum = 0.0;
        for (int d = 0; d < 3; ++d) {
            res[d] = jr_next_gaussian(rnd, pending);
            s_sum += res[d] * res[d];
        }
        for (int d = 0; d < 3; ++d) res[d] /= std::sqrt(s_sum);
        permutation[i] = i;
    }
    jr_shuffle(rnd, permutation, n_vectors);                           // :72
    *rnd_state = rnd.s;
    if (pending_gaussian) *pending_gaussian = pending;
    return MVSIM_OK;
}

static int perlin_check(const mvsim_perlin* f)
{
    MVSIM_CHECK_ARG(f && f->gradients && f->permutation, "null pointer");
    MVSIM_CHECK_ARG(f->n_vectors >= 1, "n_vectors must be >= 1");
    MVSIM_CHECK_ARG(f->n_vectors <= PERLIN_MAX_VECTORS, "n_vectors too large: the gradient table does not fit into LDS");
    for (int d = 0; d < 3; ++d) {
        MVSIM_CHECK_ARG(f->loop_extents[d] >= 1, "loop extents must be >= 1");
        MVSIM_CHECK_ARG(f->scales[d] != 0.0 && f->scales[d] == f->scales[d], "scale must not be 0 or NaN");
    }
    MVSIM_CHECK_ARG((1 + (int64_t)f->loop_extents[0]) * (1 + (int64_t)f->loop_extents[1]) * (int64_t)f->loop_extents[2] < ((int64_t)1 << 31),
                    "loop extents too large: flatIndex would overflow");
    for (int32_t i = 0; i < f->n_vectors; ++i)
        MVSIM_CHECK_ARG(f->permutation[i] >= 0 && f->permutation[i] < f->n_vectors, "permutation entry outside 0 .. n_vectors - 1");
    return MVSIM_OK;
}

static int spheres_check(const mvsim_sphere_set* s)
{
    MVSIM_CHECK_ARG(s && s->n >= 0 && ((s->centres && s->radii && s->values) || s->n == 0), "null pointer or negative count");
    MVSIM_CHECK_ARG(s->n < ((int64_t)1 << 31), "too many spheres");
    for (int64_t i = 0; i < s->n; ++i) {
        MVSIM_CHECK_ARG(s->radii[i] >= 0.0, "negative (or NaN) radius");
        MVSIM_CHECK_ARG(std::isfinite(s->centres[3 * i]) && std::isfinite(s->centres[3 * i + 1]) && std::isfinite(s->centres[3 * i + 2]),
                        "sphere centre not finite");
    }
    return MVSIM_OK;
}

static int raster_check(const int64_t origin[3], const int64_t dim[3], const float* out)
{
    MVSIM_CHECK_ARG(origin && dim && out, "null pointer");
    MVSIM_CHECK_ARG(dim[0] >= 1 && dim[1] >= 1 && dim[2] >= 1, "dimensions must be >= 1");
    MVSIM_CHECK_ARG(dim[0] <= (1 << 24) && dim[1] <= (1 << 24) && dim[2] <= (1 << 24) && nvox(dim) < ((int64_t)1 << 40), "raster too large");
    for (int d = 0; d < 3; ++d) MVSIM_CHECK_ARG(origin[d] >= -((int64_t)1 << 40) && origin[d] <= ((int64_t)1 << 40), "origin outside +-2^40");
    return MVSIM_OK;
}

static int positions_check(const double* xyz, int64_t n, const void* out, bool host)
{
    MVSIM_CHECK_ARG(n >= 0 && ((xyz && out) || n == 0), "null pointer or negative count");
    if (host)
        for (int64_t i = 0; i < 3 * n; ++i) MVSIM_CHECK_ARG(std::isfinite(xyz[i]), "position not finite");
    return MVSIM_OK;
}

int mvsim_perlin_at_dev(mvsim_ctx* ctx, const mvsim_perlin* field, const double* xyz, int64_t n, double* out)
{
    MVSIM_TRY(perlin_check(field));
    MVSIM_TRY(positions_check(xyz, n, out, false));
    MVSIM_TRY(set_device(ctx));
    PerlinDev pd;
    MVSIM_TRY(perlin_upload(ctx, field, &pd));
    return perlin_at_dev(ctx, pd, xyz, n, out);
}

int mvsim_perlin_at(mvsim_ctx* ctx, const mvsim_perlin* field, const double* xyz, int64_t n, double* out)
{
    MVSIM_TRY(perlin_check(field));
    MVSIM_TRY(positions_check(xyz, n, out, true));
    MVSIM_TRY(set_device(ctx));
    if (n == 0) return MVSIM_OK;
    PerlinDev pd;
    MVSIM_TRY(perlin_upload(ctx, field, &pd));
    MVSIM_TRY(up(ctx, ctx->vol_a, reinterpret_cast<const float*>(xyz), (size_t)n * 3 * sizeof(double)));
    MVSIM_TRY(ctx->vol_b.reserve((size_t)n * sizeof(double)));
    MVSIM_TRY(perlin_at_dev(ctx, pd, ctx->vol_a.as<double>(), n, ctx->vol_b.as<double>()));
    return down(ctx, reinterpret_cast<float*>(out), ctx->vol_b.p, (size_t)n * sizeof(double));
}

int mvsim_perlin_raster_dev(mvsim_ctx* ctx, const mvsim_perlin* field, const int64_t origin[3], const int64_t dim[3], float* out)
{
    MVSIM_TRY(perlin_check(field));
    MVSIM_TRY(raster_check(origin, dim, out));
    MVSIM_TRY(set_device(ctx));
    PerlinDev pd;
    MVSIM_TRY(perlin_upload(ctx, field, &pd));
    return perlin_raster_dev(ctx, pd, origin, dim, out);
}

int mvsim_perlin_raster(mvsim_ctx* ctx, const mvsim_perlin* field, const int64_t origin[3], const int64_t dim[3], float* out)
{
    MVSIM_TRY(perlin_check(field));
    MVSIM_TRY(raster_check(origin, dim, out));
    MVSIM_TRY(set_device(ctx));
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    PerlinDev pd;
    MVSIM_TRY(perlin_upload(ctx, field, &pd));
    MVSIM_TRY(ctx->vol_a.reserve(bytes));
    MVSIM_TRY(perlin_raster_dev(ctx, pd, origin, dim, ctx->vol_a.as<float>()));
    return down(ctx, out, ctx->vol_a.p, bytes);
}

int mvsim_spheres_at_dev(mvsim_ctx* ctx, const mvsim_sphere_set* set, const double* xyz, int64_t n, float* out)
{
    MVSIM_TRY(spheres_check(set));
    MVSIM_TRY(positions_check(xyz, n, out, false));
    MVSIM_TRY(set_device(ctx));
    SpheresDev sd;
    MVSIM_TRY(spheres_upload(ctx, set, &sd));
    return spheres_at_dev(ctx, sd, xyz, n, out);
}

int mvsim_spheres_at(mvsim_ctx* ctx, const mvsim_sphere_set* set, const double* xyz, int64_t n, float* out)
{
    MVSIM_TRY(spheres_check(set));
    MVSIM_TRY(positions_check(xyz, n, out, true));
    MVSIM_TRY(set_device(ctx));
    if (n == 0) return MVSIM_OK;
    SpheresDev sd;
    MVSIM_TRY(spheres_upload(ctx, set, &sd));
    MVSIM_TRY(up(ctx, ctx->vol_a, reinterpret_cast<const float*>(xyz), (size_t)n * 3 * sizeof(double)));
    MVSIM_TRY(ctx->vol_b.reserve((size_t)n * sizeof(float)));
    MVSIM_TRY(spheres_at_dev(ctx, sd, ctx->vol_a.as<double>(), n, ctx->vol_b.as<float>()));
    return down(ctx, out, ctx->vol_b.p, (size_t)n * sizeof(float));
}

static int spheres_raster_args(const mvsim_sphere_set* set, const int64_t origin[3], const int64_t dim[3], int combine, const float* out)
{
    MVSIM_TRY(spheres_check(set));
    MVSIM_TRY(raster_check(origin, dim, out));
    MVSIM_CHECK_ARG(combine == 0 || combine == 1, "combine must be 0 or 1");
    return MVSIM_OK;
}

int mvsim_spheres_raster_dev(mvsim_ctx* ctx, const mvsim_sphere_set* set, const int64_t origin[3], const int64_t dim[3], int combine,
                             float* out)
{
    MVSIM_TRY(spheres_raster_args(set, origin, dim, combine, out));
    MVSIM_TRY(set_device(ctx));
    SpheresDev sd;
    MVSIM_TRY(spheres_upload(ctx, set, &sd));
    return spheres_raster_dev(ctx, set, sd, origin, dim, combine, out);
}

int mvsim_spheres_raster(mvsim_ctx* ctx, const mvsim_sphere_set* set, const int64_t origin[3], const int64_t dim[3], int combine, float* out)
{
    MVSIM_TRY(spheres_raster_args(set, origin, dim, combine, out));
    MVSIM_TRY(set_device(ctx));
    const size_t bytes = (size_t)nvox(dim) * sizeof(float);
    SpheresDev sd;
    MVSIM_TRY(spheres_upload(ctx, set, &sd));
    if (combine) MVSIM_TRY(up(ctx, ctx->vol_a, out, bytes));
    else MVSIM_TRY(ctx->vol_a.reserve(bytes));
    MVSIM_TRY(spheres_raster_dev(ctx, set, sd, origin, dim, combine, ctx->vol_a.as<float>()));
    return down(ctx, out, ctx->vol_a.p, bytes);
}

int mvsim_rejection_sample(mvsim_ctx* ctx, uint64_t* rnd_state, const double rmin[3], const double rmax[3], int64_t n_samples,
                           const mvsim_density* density, int64_t max_trials, double* xyz_out, int64_t* n_trials_out)
{
    MVSIM_CHECK_ARG(rnd_state && rmin && rmax && density && (xyz_out || n_samples == 0), "null pointer");
    MVSIM_CHECK_ARG(n_samples >= 0 && n_samples < ((int64_t)1 << 28), "n_samples must be 0 .. 2^28");
    MVSIM_CHECK_ARG(max_trials >= 0 && max_trials < ((int64_t)1 << 44), "max_trials must be 0 .. 2^44");
    for (int d = 0; d < 3; ++d) MVSIM_CHECK_ARG(std::isfinite(rmin[d]) && std::isfinite(rmax[d]), "interval not finite");
    MVSIM_CHECK_ARG(density->kind == 0 || density->kind == 1, "density kind must be 0 (perlin) or 1 (spheres)");
    if (density->kind == 0) MVSIM_TRY(perlin_check(density->perlin));
    else MVSIM_TRY(spheres_check(density->spheres));
    MVSIM_TRY(set_device(ctx));
    PerlinDev pd;
    SpheresDev sd;
    if (n_samples > 0) {
        if (density->kind == 0) MVSIM_TRY(perlin_upload(ctx, density->perlin, &pd));
        else MVSIM_TRY(spheres_upload(ctx, density->spheres, &sd));
    }
    const uint64_t state = *rnd_state & JR_MASK;
    int64_t trials = 0;
    MVSIM_TRY(rejection_sample_dev(ctx, state, rmin, rmax, n_samples, density->kind == 0 ? &pd : nullptr, density->kind == 1 ? &sd : nullptr,
                                   max_trials, xyz_out, &trials));
    *rnd_state = jr_jump(state, 8 * (uint64_t)trials);
    if (n_trials_out) *n_trials_out = trials;
    return MVSIM_OK;
}

// ---- the refraction simulator: SimulateMultiViewAberrations (aberrations.hip) ---------------------------------------------
int mvsim_lightsheet_fit(double center, double thickness_center, double length, double thickness_edges, double abc[3])
{
    MVSIM_CHECK_ARG(abc != nullptr, "null pointer");
    MVSIM_CHECK_ARG(std::isfinite(center) && std::isfinite(thickness_center) && std::isfinite(length) && std::isfinite(thickness_edges),
                    "light sheet: non-finite argument");
    const double px[3] = {center, center - length / 2, center + length / 2};                    // Lightsheet.java:47-50
    const double py[3] = {thickness_center, thickness_edges, thickness_edges};
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {                                                                 // :90-113
        const double x = px[k], y = py[k], xx = x * x, xxx = xx * x;
        m[0] += xx * xx; m[1] += xxx; m[2] += xx;
        m[3] += xxx; m[4] += xx; m[5] += x;
        m[6] += xx; m[7] += x; m[8] += 1;
        t[0] += xx * y; t[1] += x * y; t[2] += y;
    }
    const double det = m[0] * m[4] * m[8] + m[3] * m[7] * m[2] + m[6] * m[1] * m[5] - m[2] * m[4] * m[6] - m[5] * m[7] * m[0] -
                       m[8] * m[1] * m[3];                                                        // :131-142
    abc[0] = abc[1] = abc[2] = 0;
    MVSIM_CHECK_ARG(det != 0 && std::isfinite(det), "light sheet: cannot invert the matrix of the fit");
    const double inv[9] = {(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                           (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                           (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
    for (int r = 0; r < 3; ++r) abc[r] = inv[3 * r] * t[0] + inv[3 * r + 1] * t[1] + inv[3 * r + 2] * t[2];   // :126-128
    return MVSIM_OK;
}

static int aberr_dim_check(const int64_t dim[3])
{
    MVSIM_CHECK_ARG(dim != nullptr, "null dim");
    for (int d = 0; d < 3; ++d) MVSIM_CHECK_ARG(dim[d] >= 2 && dim[d] <= (1 << 24), "the refraction simulator needs 2 .. 2^24 samples per dimension");
    MVSIM_CHECK_ARG(dim[0] * dim[1] * dim[2] < ((int64_t)1 << 40), "volume too large");
    return MVSIM_OK;
}

static size_t aberr_bytes(const int64_t dim[3]) { return (size_t)(dim[0] * dim[1] * dim[2]) * sizeof(float); }

static int aberr_points_check(const double* xyz, int64_t n, double limit)
{
    MVSIM_CHECK_ARG(n >= 0 && (xyz || n == 0), "null point list or negative count");
    for (int64_t i = 0; i < 3 * n; ++i) MVSIM_CHECK_ARG(std::fabs(xyz[i]) < limit, "position not finite or too far away");   // false for NaN
    return MVSIM_OK;
}

static int hessian_at_args(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const double* xyz, int64_t n)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(img != nullptr, "null image");
    MVSIM_TRY(aberr_points_check(xyz, n, 0x1.0p30));
    return set_device(ctx);
}

int mvsim_hessian_at_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const double* xyz, int64_t n, double* matrix9,
                         double* eigvec3, double* eigval)
{
    MVSIM_TRY(hessian_at_args(ctx, img, dim, xyz, n));
    return aberr_hessian_at_dev(ctx, img, dim, xyz, n, matrix9, eigvec3, eigval);
}

int mvsim_hessian_at(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const double* xyz, int64_t n, double* matrix9, double* eigvec3,
                     double* eigval)
{
    MVSIM_TRY(hessian_at_args(ctx, img, dim, xyz, n));
    MVSIM_TRY(up(ctx, ctx->vol_a, img, aberr_bytes(dim)));
    return aberr_hessian_at_dev(ctx, ctx->vol_a.as<float>(), dim, xyz, n, matrix9, eigvec3, eigval);
}

static int hessian_images_args(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const float* eigval, const float* eigvec)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(img && eigval && eigvec, "null pointer");
    return set_device(ctx);
}

int mvsim_hessian_images_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], float* eigval, float* eigvec)
{
    MVSIM_TRY(hessian_images_args(ctx, img, dim, eigval, eigvec));
    return aberr_hessian_images_dev(ctx, img, dim, 0, (int)dim[2], eigval, eigvec);
}

int mvsim_hessian_images(mvsim_ctx* ctx, const float* img, const int64_t dim[3], float* eigval, float* eigvec)
{
    MVSIM_TRY(hessian_images_args(ctx, img, dim, eigval, eigvec));
    const size_t bytes = aberr_bytes(dim);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(ctx->vol_b.reserve(4 * bytes));
    float* out = ctx->vol_b.as<float>();
    MVSIM_TRY(aberr_hessian_images_dev(ctx, ctx->vol_a.as<float>(), dim, 0, (int)dim[2], out, out + bytes / sizeof(float)));
    MVSIM_HIP(hipMemcpyAsync(eigval, out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return down(ctx, eigvec, out + bytes / sizeof(float), 3 * bytes);
}

// What a call leaves the caller's java.util.Random at: a light-sheet ray takes three nextDouble() (six steps of the generator), a
// camera ray two (four steps), whatever the launch shape traced (aberrations.hip: starts)
static void advance_sheet_rays(uint64_t* rnd_state, int64_t rays) { *rnd_state = jr_jump(*rnd_state & JR_MASK, 6 * (uint64_t)rays); }
static void advance_camera_rays(uint64_t* rnd_state, const int64_t dim[3], int rays_per_pixel)
{
    *rnd_state = jr_jump(*rnd_state & JR_MASK, 4 * (uint64_t)(dim[0] * dim[1]) * (uint64_t)rays_per_pixel);
}

static int rays_per_pixel_check(int rays_per_pixel)
{
    MVSIM_CHECK_ARG(rays_per_pixel >= 1 && rays_per_pixel <= 4096, "rays_per_pixel must be 1 .. 4096");
    return MVSIM_OK;
}

int mvsim_refract3d_ray_starts(mvsim_ctx* ctx, uint64_t* rnd_state, const int64_t dim[3], int illum, int z, const double abc[3], int64_t n,
                               double* pos3, double* dir3)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(rnd_state && abc && n >= 0 && ((pos3 && dir3) || n == 0), "null pointer or negative count");
    MVSIM_CHECK_ARG(std::isfinite(abc[0]) && std::isfinite(abc[1]) && std::isfinite(abc[2]), "light sheet: non-finite coefficient");
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(aberr_ray_starts(ctx, *rnd_state, dim, 0, illum, z, abc, 1, n, pos3, dir3));
    advance_sheet_rays(rnd_state, n);
    return MVSIM_OK;
}

int mvsim_camera_ray_starts(mvsim_ctx* ctx, uint64_t* rnd_state, const int64_t dim[3], int rays_per_pixel, double* pos3)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(rnd_state && pos3, "null pointer");
    MVSIM_TRY(rays_per_pixel_check(rays_per_pixel));
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(aberr_ray_starts(ctx, *rnd_state, dim, 1, 0, 0, nullptr, rays_per_pixel, dim[0] * dim[1] * rays_per_pixel, pos3, nullptr));
    advance_camera_rays(rnd_state, dim, rays_per_pixel);
    return MVSIM_OK;
}

// VolumeInjection's constructor (:74-92): the Gaussian of a point at the origin over its box, summed in cursor order (x fastest)
static double aberr_sum_weights(const double sigma[3], int size[3], int* num_pixels)
{
    double tss[3], sum = 0;
    aberr_inject_geometry(sigma, size, tss);
    int count = 0;
    for (int z = -(size[2] / 2); z < -(size[2] / 2) + size[2]; ++z)
        for (int y = -(size[1] / 2); y < -(size[1] / 2) + size[1]; ++y)
            for (int x = -(size[0] / 2); x < -(size[0] / 2) + size[0]; ++x) {
                const double c[3] = {(double)x, (double)y, (double)z};
                double value = 1;
                for (int d = 0; d < 3; ++d) {
                    const double q = 0.0 - c[d];
                    value *= std::exp(-(q * q) / tss[d]);
                }
                sum += value;
                ++count;
            }
    if (num_pixels) *num_pixels = count;
    return sum;
}

static int aberr_sigma_check(const double sigma[3])
{
    MVSIM_CHECK_ARG(sigma != nullptr, "null sigma");
    for (int d = 0; d < 3; ++d) MVSIM_CHECK_ARG(std::isfinite(sigma[d]) && sigma[d] > 0.0 && sigma[d] <= 1.0e4, "sigma must be finite, > 0 and <= 1e4");
    return MVSIM_OK;
}

int mvsim_volume_inject_info(const double sigma[3], int32_t size[3], double* sum_weights, int32_t* num_pixels)
{
    MVSIM_TRY(aberr_sigma_check(sigma));
    MVSIM_CHECK_ARG(size && sum_weights && num_pixels, "null pointer");
    int s[3], np = 0;
    *sum_weights = aberr_sum_weights(sigma, s, &np);
    for (int d = 0; d < 3; ++d) size[d] = s[d];
    *num_pixels = np;
    return MVSIM_OK;
}

// everything refract3d checks, the light sheet's fit (SMVA:297) and the weight sum of the injected Gaussians (sigma 0.5)
static int refract3d_args(mvsim_ctx* ctx, const float* img, const float* ri_img, const int64_t dim[3], double ls_middle, double ls_edge, double ri,
                          int64_t num_rays, const uint64_t* rnd_state, const float* image, const float* weight, const mvsim_ray_steps* steps,
                          double abc[3], double* sumw)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(rnd_state != nullptr, "null rnd_state");
    MVSIM_CHECK_ARG(num_rays >= 0, "negative number of rays");
    MVSIM_CHECK_ARG(std::isfinite(ls_middle) && std::isfinite(ls_edge) && std::isfinite(ri), "refract3d: non-finite argument");
    MVSIM_CHECK_ARG(!steps || steps->capacity >= 0, "negative step capacity");
    MVSIM_TRY(mvsim_lightsheet_fit(dim[0] / 2.0, ls_middle, (double)dim[0], ls_edge, abc));        // SMVA:297
    MVSIM_CHECK_ARG(img && ri_img && ((image != nullptr) == (weight != nullptr)), "null volume (image and weight go together)");
    MVSIM_TRY(set_device(ctx));
    const double sigma[3] = {0.5, 0.5, 0.5};
    int size[3];
    *sumw = aberr_sum_weights(sigma, size, nullptr);
    return MVSIM_OK;
}

int mvsim_refract3d_dev(mvsim_ctx* ctx, const float* img, const float* ri_img, const int64_t dim[3], int illum, int z, double ls_middle,
                        double ls_edge, double ri, int64_t num_rays, uint64_t* rnd_state, float* image, float* weight, mvsim_ray_steps* steps)
{
    double abc[3], sumw;
    MVSIM_TRY(refract3d_args(ctx, img, ri_img, dim, ls_middle, ls_edge, ri, num_rays, rnd_state, image, weight, steps, abc, &sumw));
    MVSIM_TRY(aberr_refract3d_dev(ctx, img, ri_img, dim, illum, z, abc, ri, num_rays, *rnd_state, image, weight, sumw, steps));
    advance_sheet_rays(rnd_state, num_rays);
    return MVSIM_OK;
}

int mvsim_refract3d(mvsim_ctx* ctx, const float* img, const float* ri_img, const int64_t dim[3], int illum, int z, double ls_middle,
                    double ls_edge, double ri, int64_t num_rays, uint64_t* rnd_state, float* image, float* weight, mvsim_ray_steps* steps)
{
    double abc[3], sumw;
    MVSIM_TRY(refract3d_args(ctx, img, ri_img, dim, ls_middle, ls_edge, ri, num_rays, rnd_state, image, weight, steps, abc, &sumw));
    const size_t bytes = aberr_bytes(dim);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    MVSIM_TRY(up(ctx, ctx->vol_b, ri_img, bytes));
    float* out = nullptr;
    if (image) {
        MVSIM_TRY(ctx->vol_c.reserve(2 * bytes));
        out = ctx->vol_c.as<float>();
        MVSIM_HIP(hipMemsetAsync(out, 0, 2 * bytes, ctx->stream));
    }
    MVSIM_TRY(aberr_refract3d_dev(ctx, ctx->vol_a.as<float>(), ctx->vol_b.as<float>(), dim, illum, z, abc, ri, num_rays, *rnd_state, out,
                                  out ? out + bytes / sizeof(float) : nullptr, sumw, steps));
    advance_sheet_rays(rnd_state, num_rays);
    if (!image) return MVSIM_OK;
    MVSIM_HIP(hipMemcpyAsync(image, out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return down(ctx, weight, out + bytes / sizeof(float), bytes);
}

static int volume_inject_args(mvsim_ctx* ctx, const float* image, const float* weight, const int64_t dim[3], const double sigma[3],
                              const double* xyz, const double* intensity, int64_t n)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_TRY(aberr_sigma_check(sigma));
    MVSIM_TRY(aberr_points_check(xyz, n, INFINITY));
    MVSIM_CHECK_ARG(intensity || n == 0, "null intensity list");
    for (int64_t i = 0; i < n; ++i) MVSIM_CHECK_ARG(std::isfinite(intensity[i]), "intensity not finite");
    MVSIM_CHECK_ARG(image && weight, "null volume");
    return set_device(ctx);
}

int mvsim_volume_inject_dev(mvsim_ctx* ctx, float* image, float* weight, const int64_t dim[3], const double sigma[3], const double* xyz,
                            const double* intensity, int64_t n, int normalized)
{
    MVSIM_TRY(volume_inject_args(ctx, image, weight, dim, sigma, xyz, intensity, n));
    if (n == 0) return MVSIM_OK;
    int size[3];
    const double sumw = normalized ? aberr_sum_weights(sigma, size, nullptr) : 0.0;
    DevBuf pts;
    int rc = pts.reserve((size_t)n * 4 * sizeof(double));
    if (rc == MVSIM_OK) {
        double* d = pts.as<double>();
        hipError_t e = hipMemcpyAsync(d, xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d + 3 * n, intensity, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { set_error("hipMemcpyAsync failed: %s", hipGetErrorString(e)); rc = MVSIM_EHIP; }
        else rc = aberr_inject_dev(ctx, image, weight, dim, sigma, d, d + 3 * n, nullptr, n, sumw);
    }
    (void)hipStreamSynchronize(ctx->stream);
    pts.release();
    return rc;
}

int mvsim_volume_inject(mvsim_ctx* ctx, float* image, float* weight, const int64_t dim[3], const double sigma[3], const double* xyz,
                        const double* intensity, int64_t n, int normalized)
{
    MVSIM_TRY(volume_inject_args(ctx, image, weight, dim, sigma, xyz, intensity, n));
    const size_t bytes = aberr_bytes(dim);
    MVSIM_TRY(up(ctx, ctx->vol_a, image, bytes));
    MVSIM_TRY(up(ctx, ctx->vol_b, weight, bytes));
    MVSIM_TRY(mvsim_volume_inject_dev(ctx, ctx->vol_a.as<float>(), ctx->vol_b.as<float>(), dim, sigma, xyz, intensity, n, normalized));
    MVSIM_HIP(hipMemcpyAsync(image, ctx->vol_a.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return down(ctx, weight, ctx->vol_b.p, bytes);
}

static int volume_normalize_args(mvsim_ctx* ctx, const float* image, const float* weight, int64_t n, const float* out)
{
    MVSIM_CHECK_ARG(image && weight && out && n >= 1, "null volume or empty count");
    return set_device(ctx);
}

int mvsim_volume_normalize_dev(mvsim_ctx* ctx, const float* image, const float* weight, int64_t n, float* out)
{
    MVSIM_TRY(volume_normalize_args(ctx, image, weight, n, out));
    return aberr_normalize_dev(ctx, image, weight, n, out);
}

int mvsim_volume_normalize(mvsim_ctx* ctx, const float* image, const float* weight, int64_t n, float* out)
{
    MVSIM_TRY(volume_normalize_args(ctx, image, weight, n, out));
    const size_t bytes = (size_t)n * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, image, bytes));
    MVSIM_TRY(up(ctx, ctx->vol_b, weight, bytes));
    MVSIM_TRY(ctx->vol_c.reserve(bytes));
    MVSIM_TRY(aberr_normalize_dev(ctx, ctx->vol_a.as<float>(), ctx->vol_b.as<float>(), n, ctx->vol_c.as<float>()));
    return down(ctx, out, ctx->vol_c.p, bytes);
}

static int volume_project_args(mvsim_ctx* ctx, const float* image, const float* weight, const int64_t dim[3], const float* proj)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(image && weight && proj, "null pointer");
    return set_device(ctx);
}

int mvsim_volume_project_dev(mvsim_ctx* ctx, const float* image, const float* weight, const int64_t dim[3], float* proj)
{
    MVSIM_TRY(volume_project_args(ctx, image, weight, dim, proj));
    return aberr_project_dev(ctx, image, weight, dim, proj);
}

int mvsim_volume_project(mvsim_ctx* ctx, const float* image, const float* weight, const int64_t dim[3], float* proj)
{
    MVSIM_TRY(volume_project_args(ctx, image, weight, dim, proj));
    const size_t bytes = aberr_bytes(dim), pbytes = (size_t)(dim[0] * dim[1]) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, image, bytes));
    MVSIM_TRY(up(ctx, ctx->vol_b, weight, bytes));
    MVSIM_TRY(ctx->vol_c.reserve(pbytes));
    MVSIM_TRY(aberr_project_dev(ctx, ctx->vol_a.as<float>(), ctx->vol_b.as<float>(), dim, ctx->vol_c.as<float>()));
    return down(ctx, proj, ctx->vol_c.p, pbytes);
}

static int project_to_camera_args(mvsim_ctx* ctx, const float* ri_img, const float* refr, const int64_t dim[3], int rays_per_pixel,
                                  const uint64_t* rnd_state, const float* proj)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(ri_img && refr && proj && rnd_state, "null pointer");
    MVSIM_TRY(rays_per_pixel_check(rays_per_pixel));
    return set_device(ctx);
}

int mvsim_project_to_camera_dev(mvsim_ctx* ctx, const float* ri_img, const float* refr, const int64_t dim[3], int current_z,
                                int rays_per_pixel, uint64_t* rnd_state, float* proj)
{
    MVSIM_TRY(project_to_camera_args(ctx, ri_img, refr, dim, rays_per_pixel, rnd_state, proj));
    MVSIM_TRY(aberr_project_to_camera_dev(ctx, ri_img, refr, dim, current_z, rays_per_pixel, *rnd_state, proj));
    advance_camera_rays(rnd_state, dim, rays_per_pixel);
    return MVSIM_OK;
}

int mvsim_project_to_camera(mvsim_ctx* ctx, const float* ri_img, const float* refr, const int64_t dim[3], int current_z, int rays_per_pixel,
                            uint64_t* rnd_state, float* proj)
{
    MVSIM_TRY(project_to_camera_args(ctx, ri_img, refr, dim, rays_per_pixel, rnd_state, proj));
    const size_t bytes = aberr_bytes(dim), pbytes = (size_t)(dim[0] * dim[1]) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, ri_img, bytes));
    MVSIM_TRY(up(ctx, ctx->vol_b, refr, bytes));
    MVSIM_TRY(ctx->vol_c.reserve(pbytes));
    MVSIM_TRY(aberr_project_to_camera_dev(ctx, ctx->vol_a.as<float>(), ctx->vol_b.as<float>(), dim, current_z, rays_per_pixel, *rnd_state,
                                          ctx->vol_c.as<float>()));
    advance_camera_rays(rnd_state, dim, rays_per_pixel);
    return down(ctx, proj, ctx->vol_c.p, pbytes);
}

// ---- the ray sandbox (raytracing/RayTracingTest.java) and the general tracer (raytrace.hip) ------------------------------------
int mvsim_trace_params_default(const int64_t dim[3], mvsim_trace_params* params)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(params != nullptr, "null params");
    *params = mvsim_trace_params{};
    params->n_a = 0.0;
    params->n_b = 1.0;
    params->ev_threshold = 0.01;
    params->max_moves = std::min<int64_t>(4 * (dim[0] + dim[1] + dim[2]), (int64_t)1 << 20);
    params->total_reflection = MVSIM_TRACE_KEEP;
    params->normalize_dirs = 0;
    params->constant_value = 1.0;
    params->sigma[0] = params->sigma[1] = params->sigma[2] = 0.5;
    params->normalized = 1;
    return MVSIM_OK;
}

// everything trace_rays checks, and the weight sum of the injected Gaussians (0 when they are not normalized)
static int trace_rays_args(mvsim_ctx* ctx, const float* ri_img, const int64_t dim[3], const double* pos3, const double* dir3,
                           const float* intensity, int64_t n, const mvsim_trace_params* tp, const float* image, const float* weight,
                           const mvsim_ray_steps* steps, double* sumw)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(tp != nullptr, "null params");
    MVSIM_CHECK_ARG(std::isfinite(tp->n_a) && std::isfinite(tp->n_b) && std::isfinite(tp->ev_threshold) && std::isfinite(tp->constant_value),
                    "trace_rays: non-finite parameter");
    MVSIM_CHECK_ARG(std::isfinite((float)tp->constant_value), "trace_rays: constant_value is not a finite float");
    MVSIM_CHECK_ARG(tp->ev_threshold >= 0.0, "trace_rays: ev_threshold must be >= 0");
    MVSIM_CHECK_ARG(tp->max_moves >= 1 && tp->max_moves <= ((int64_t)1 << 20), "trace_rays: max_moves must be 1 .. 2^20");
    MVSIM_CHECK_ARG(tp->total_reflection == MVSIM_TRACE_KEEP || tp->total_reflection == MVSIM_TRACE_REFLECT,
                    "trace_rays: unknown total_reflection policy");
    MVSIM_TRY(aberr_sigma_check(tp->sigma));
    MVSIM_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "trace_rays: 0 .. 2^31 - 1 rays");
    MVSIM_CHECK_ARG((pos3 && dir3) || n == 0, "null ray list");
    MVSIM_TRY(aberr_points_check(pos3, n, 0x1.0p30));
    for (int64_t i = 0; i < 3 * n; ++i) MVSIM_CHECK_ARG(std::fabs(dir3[i]) < 0x1.0p30, "direction not finite or too long");
    if (tp->normalize_dirs)
        for (int64_t i = 0; i < n; ++i)
            MVSIM_CHECK_ARG(dir3[3 * i] != 0.0 || dir3[3 * i + 1] != 0.0 || dir3[3 * i + 2] != 0.0, "a zero direction cannot be normalised");
    if (intensity)
        for (int64_t i = 0; i < n; ++i) MVSIM_CHECK_ARG(std::isfinite(intensity[i]), "intensity not finite");
    MVSIM_CHECK_ARG(!steps || steps->capacity >= 0, "negative step capacity");
    MVSIM_CHECK_ARG(ri_img && ((image != nullptr) == (weight != nullptr)), "null volume (image and weight go together)");
    MVSIM_TRY(set_device(ctx));
    int size[3];
    *sumw = tp->normalized ? aberr_sum_weights(tp->sigma, size, nullptr) : 0.0;
    return MVSIM_OK;
}

int mvsim_trace_rays_dev(mvsim_ctx* ctx, const float* ri_img, const float* img, const int64_t dim[3], const double* pos3, const double* dir3,
                         const float* intensity, int64_t n, const mvsim_trace_params* params, float* image, float* weight,
                         mvsim_ray_steps* steps, double* end_pos3, double* end_dir3, int64_t* n_capped)
{
    double sumw;
    MVSIM_TRY(trace_rays_args(ctx, ri_img, dim, pos3, dir3, intensity, n, params, image, weight, steps, &sumw));
    return trace_rays_dev(ctx, ri_img, img, dim, pos3, dir3, intensity, n, params, sumw, image, weight, steps, end_pos3, end_dir3, n_capped);
}

int mvsim_trace_rays(mvsim_ctx* ctx, const float* ri_img, const float* img, const int64_t dim[3], const double* pos3, const double* dir3,
                     const float* intensity, int64_t n, const mvsim_trace_params* params, float* image, float* weight, mvsim_ray_steps* steps,
                     double* end_pos3, double* end_dir3, int64_t* n_capped)
{
    double sumw;
    MVSIM_TRY(trace_rays_args(ctx, ri_img, dim, pos3, dir3, intensity, n, params, image, weight, steps, &sumw));
    const size_t bytes = aberr_bytes(dim);
    MVSIM_TRY(up(ctx, ctx->vol_b, ri_img, bytes));
    if (img) MVSIM_TRY(up(ctx, ctx->vol_a, img, bytes));
    float* out = nullptr;
    if (image) {
        MVSIM_TRY(ctx->vol_c.reserve(2 * bytes));
        out = ctx->vol_c.as<float>();
        MVSIM_HIP(hipMemsetAsync(out, 0, 2 * bytes, ctx->stream));
    }
    MVSIM_TRY(trace_rays_dev(ctx, ctx->vol_b.as<float>(), img ? ctx->vol_a.as<float>() : nullptr, dim, pos3, dir3, intensity, n, params, sumw,
                             out, out ? out + bytes / sizeof(float) : nullptr, steps, end_pos3, end_dir3, n_capped));
    if (!image) return MVSIM_OK;
    MVSIM_HIP(hipMemcpyAsync(image, out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return down(ctx, weight, out + bytes / sizeof(float), bytes);
}

int mvsim_sandbox_ray_starts(mvsim_ctx* ctx, uint64_t* rnd_state, const int64_t dim[3], int x, int z, int64_t n, double* pos3, double* dir3)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(rnd_state && n >= 0 && ((pos3 && dir3) || n == 0), "null pointer or negative count");
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(trace_ray_starts(ctx, 1, *rnd_state, dim, x, z, n, pos3, dir3));
    *rnd_state = jr_jump(*rnd_state & JR_MASK, 4 * (uint64_t)n);        // two nextDouble() per ray, two generator steps each
    return MVSIM_OK;
}

int mvsim_grid_ray_starts(mvsim_ctx* ctx, const int64_t dim[3], int z, int spacing, int64_t capacity, double* pos3, double* dir3, int64_t* n_out)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(spacing >= 1, "grid: spacing must be >= 1");
    MVSIM_CHECK_ARG(n_out != nullptr && capacity >= 0, "null count or negative capacity");
    const int64_t n = dim[0] / spacing;                                  // x = spacing, 2 spacing, .. <= Nx (RTT:334)
    *n_out = n;
    if (capacity == 0 && !pos3 && !dir3) return MVSIM_OK;
    MVSIM_CHECK_ARG(pos3 && dir3 && capacity >= n, "grid: the ray lists are null or hold fewer rays than the grid has");
    MVSIM_TRY(set_device(ctx));
    return trace_ray_starts(ctx, 0, 0, dim, spacing, z, n, pos3, dir3);
}

int mvsim_draw_simple_image_dev(mvsim_ctx* ctx, float* out, const int64_t dim[3], float low, float high)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(out != nullptr, "null volume");
    MVSIM_CHECK_ARG(std::isfinite(low) && std::isfinite(high), "drawSimpleImage: non-finite value");
    MVSIM_TRY(set_device(ctx));
    return draw_simple_image_dev(ctx, out, dim, low, high);
}

int mvsim_draw_simple_image(mvsim_ctx* ctx, float* out, const int64_t dim[3], float low, float high)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(out != nullptr, "null volume");
    MVSIM_CHECK_ARG(std::isfinite(low) && std::isfinite(high), "drawSimpleImage: non-finite value");
    MVSIM_TRY(set_device(ctx));
    MVSIM_TRY(ctx->vol_a.reserve(aberr_bytes(dim)));
    MVSIM_TRY(draw_simple_image_dev(ctx, ctx->vol_a.as<float>(), dim, low, high));
    return down(ctx, out, ctx->vol_a.p, aberr_bytes(dim));
}

static int hessian_plane_args(mvsim_ctx* ctx, const float* img, const int64_t dim[3], int z, const float* eigval)
{
    MVSIM_TRY(aberr_dim_check(dim));
    MVSIM_CHECK_ARG(img && eigval, "null pointer");
    MVSIM_CHECK_ARG(z >= 0 && z < dim[2], "hessian_plane: z outside the volume");
    return set_device(ctx);
}

int mvsim_hessian_plane_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3], int z, float* eigval, float* eigvec)
{
    MVSIM_TRY(hessian_plane_args(ctx, img, dim, z, eigval));
    return aberr_hessian_images_dev(ctx, img, dim, z, 1, eigval, eigvec);
}

int mvsim_hessian_plane(mvsim_ctx* ctx, const float* img, const int64_t dim[3], int z, float* eigval, float* eigvec)
{
    MVSIM_TRY(hessian_plane_args(ctx, img, dim, z, eigval));
    const size_t pbytes = (size_t)(dim[0] * dim[1]) * sizeof(float);
    MVSIM_TRY(up(ctx, ctx->vol_a, img, aberr_bytes(dim)));
    MVSIM_TRY(ctx->vol_b.reserve(4 * pbytes));
    float* out = ctx->vol_b.as<float>();
    MVSIM_TRY(aberr_hessian_images_dev(ctx, ctx->vol_a.as<float>(), dim, z, 1, out, eigvec ? out + pbytes / sizeof(float) : nullptr));
    if (eigvec) MVSIM_HIP(hipMemcpyAsync(eigvec, out + pbytes / sizeof(float), 3 * pbytes, hipMemcpyDeviceToHost, ctx->stream));
    return down(ctx, eigval, out, pbytes);
}

}  // extern "C"
