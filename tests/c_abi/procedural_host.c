/* Host leg of the procedural phantom's C ABI (include/mvsim.h) for a sanitizer build: mvsim_perlin_init and every argument check
 * of the mvsim_perlin_*, mvsim_spheres_* and mvsim_rejection_sample entry points, called from a consumer compiled with
 * -fsanitize=address,undefined on exactly sized heap blocks.  No context is created: the checks come before a device is touched.
 * Exit code 0 = clean. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mvsim.h"

#define REQUIRE(cond)                                                               \
    do {                                                                            \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main(void)
{
    /* new Random(42): the constructor's 3 n Gaussians and the shuffle, for an even and an odd number of Gaussians */
    const int counts[2] = {100, 7};
    for (int c = 0; c < 2; ++c) {
        const int n = counts[c];
        double* grad = (double*)malloc((size_t)n * 3 * sizeof(double));
        int32_t* perm = (int32_t*)malloc((size_t)n * sizeof(int32_t));
        int* seen = (int*)calloc((size_t)n, sizeof(int));
        uint64_t state = (42ull ^ 0x5DEECE66Dull) & ((1ull << 48) - 1);
        double pending = NAN;
        REQUIRE(mvsim_perlin_init(&state, n, grad, perm, &pending) == MVSIM_OK);
        if (c == 0) REQUIRE(isnan(pending));                           /* 300 Gaussians: none left over */
        else REQUIRE(!isnan(pending));                                 /* 21: the 22nd is cached */
        for (int i = 0; i < n; ++i) {
            const double* g = grad + 3 * i;
            REQUIRE(fabs(g[0] * g[0] + g[1] * g[1] + g[2] * g[2] - 1.0) < 1e-14);
            REQUIRE(perm[i] >= 0 && perm[i] < n && !seen[perm[i]]);
            seen[perm[i]] = 1;
        }
        REQUIRE(mvsim_perlin_init(&state, n, grad, perm, NULL) == MVSIM_OK);   /* no cache handed in or out */
        REQUIRE(mvsim_perlin_init(&state, 0, grad, perm, NULL) == MVSIM_EINVAL && strstr(mvsim_last_error(), "n_vectors"));
        REQUIRE(mvsim_perlin_init(NULL, n, grad, perm, NULL) == MVSIM_EINVAL);
        REQUIRE(mvsim_perlin_init(&state, n, NULL, perm, NULL) == MVSIM_EINVAL);
        REQUIRE(mvsim_perlin_init(&state, n, grad, NULL, NULL) == MVSIM_EINVAL);
        free(grad); free(perm); free(seen);
    }

    const int n = 5;
    double* grad = (double*)calloc((size_t)n * 3, sizeof(double));
    int32_t* perm = (int32_t*)calloc((size_t)n, sizeof(int32_t));
    double* xyz = (double*)calloc(3, sizeof(double));
    double* dout = (double*)calloc(1, sizeof(double));
    float* fout = (float*)calloc(8, sizeof(float));
    int64_t* origin = (int64_t*)calloc(3, sizeof(int64_t));
    int64_t* dim = (int64_t*)malloc(3 * sizeof(int64_t));
    dim[0] = dim[1] = dim[2] = 2;
    mvsim_perlin f;
    memset(&f, 0, sizeof f);
    f.scales[0] = f.scales[1] = f.scales[2] = 2.0;
    f.loop_extents[0] = f.loop_extents[1] = f.loop_extents[2] = 15;
    f.n_vectors = n;
    f.gradients = grad;
    f.permutation = perm;
    f.threshold = NAN;
    /* a well-formed call gets as far as the context */
    REQUIRE(mvsim_perlin_at(NULL, &f, xyz, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "ctx is null"));
    REQUIRE(mvsim_perlin_raster(NULL, &f, origin, dim, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "ctx is null"));
    mvsim_perlin g = f;
    g.n_vectors = 0;
    REQUIRE(mvsim_perlin_at(NULL, &g, xyz, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "n_vectors"));
    g.n_vectors = 100000;
    REQUIRE(mvsim_perlin_raster_dev(NULL, &g, origin, dim, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "LDS"));
    g = f; g.loop_extents[1] = 0;
    REQUIRE(mvsim_perlin_at_dev(NULL, &g, xyz, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "extents"));
    g = f; g.loop_extents[2] = 1 << 30;
    REQUIRE(mvsim_perlin_at(NULL, &g, xyz, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "flatIndex"));
    g = f; g.scales[2] = 0.0;
    REQUIRE(mvsim_perlin_raster(NULL, &g, origin, dim, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "scale"));
    g = f; g.gradients = NULL;
    REQUIRE(mvsim_perlin_at(NULL, &g, xyz, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "null"));
    perm[4] = n;                                                       /* an entry outside the table */
    REQUIRE(mvsim_perlin_at(NULL, &f, xyz, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "permutation"));
    perm[4] = 0;
    REQUIRE(mvsim_perlin_at(NULL, &f, NULL, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "null"));
    xyz[1] = INFINITY;
    REQUIRE(mvsim_perlin_at(NULL, &f, xyz, 1, dout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "finite"));
    xyz[1] = 0.0;
    dim[1] = 0;
    REQUIRE(mvsim_perlin_raster(NULL, &f, origin, dim, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "dimensions"));
    dim[1] = 2;
    REQUIRE(mvsim_perlin_raster(NULL, &f, origin, dim, NULL) == MVSIM_EINVAL && strstr(mvsim_last_error(), "null"));

    double* centres = (double*)calloc(6, sizeof(double));
    double* radii = (double*)calloc(2, sizeof(double));
    float* values = (float*)calloc(2, sizeof(float));
    mvsim_sphere_set s;
    memset(&s, 0, sizeof s);
    s.n = 2; s.centres = centres; s.radii = radii; s.values = values; s.background = 0.0f;
    REQUIRE(mvsim_spheres_at(NULL, &s, xyz, 1, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "ctx is null"));
    REQUIRE(mvsim_spheres_raster(NULL, &s, origin, dim, 1, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "ctx is null"));
    REQUIRE(mvsim_spheres_raster_dev(NULL, &s, origin, dim, 2, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "combine"));
    radii[1] = -1.0;
    REQUIRE(mvsim_spheres_at(NULL, &s, xyz, 1, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "radius"));
    REQUIRE(mvsim_spheres_raster(NULL, &s, origin, dim, 0, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "radius"));
    radii[1] = NAN;
    REQUIRE(mvsim_spheres_at_dev(NULL, &s, xyz, 1, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "radius"));
    radii[1] = 1.0;
    centres[4] = NAN;
    REQUIRE(mvsim_spheres_at(NULL, &s, xyz, 1, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "centre"));
    centres[4] = 0.0;
    s.values = NULL;
    REQUIRE(mvsim_spheres_at(NULL, &s, xyz, 1, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "null"));
    s.values = values;
    s.n = -1;
    REQUIRE(mvsim_spheres_raster(NULL, &s, origin, dim, 0, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "negative"));
    s.n = 2;
    dim[2] = -3;
    REQUIRE(mvsim_spheres_raster(NULL, &s, origin, dim, 0, fout) == MVSIM_EINVAL && strstr(mvsim_last_error(), "dimensions"));
    dim[2] = 2;

    uint64_t state = 12345;
    double* rmin = (double*)calloc(3, sizeof(double));
    double* rmax = (double*)calloc(3, sizeof(double));
    int64_t trials = -1;
    mvsim_density d;
    memset(&d, 0, sizeof d);
    d.kind = 1; d.spheres = &s;
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, 1, &d, 10, xyz, &trials) == MVSIM_EINVAL && strstr(mvsim_last_error(), "ctx is null"));
    REQUIRE(mvsim_rejection_sample(NULL, NULL, rmin, rmax, 1, &d, 10, xyz, &trials) == MVSIM_EINVAL && strstr(mvsim_last_error(), "null"));
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, 1, NULL, 10, xyz, &trials) == MVSIM_EINVAL);
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, 1, &d, 10, NULL, &trials) == MVSIM_EINVAL);
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, -1, &d, 10, xyz, &trials) == MVSIM_EINVAL && strstr(mvsim_last_error(), "n_samples"));
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, 1, &d, -1, xyz, &trials) == MVSIM_EINVAL && strstr(mvsim_last_error(), "max_trials"));
    d.kind = 2;
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, 1, &d, 10, xyz, &trials) == MVSIM_EINVAL && strstr(mvsim_last_error(), "kind"));
    d.kind = 0; d.perlin = NULL;
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, 1, &d, 10, xyz, &trials) == MVSIM_EINVAL && strstr(mvsim_last_error(), "null"));
    d.perlin = &f;
    rmax[0] = INFINITY;
    REQUIRE(mvsim_rejection_sample(NULL, &state, rmin, rmax, 1, &d, 10, xyz, &trials) == MVSIM_EINVAL && strstr(mvsim_last_error(), "interval"));
    REQUIRE(state == 12345 && trials == -1);

    free(grad); free(perm); free(xyz); free(dout); free(fout); free(origin); free(dim); free(centres); free(radii); free(values);
    free(rmin); free(rmax);
    printf("procedural host sanitizer run ok\n");
    return 0;
}
