/* Plain-C consumer of the refraction simulator's entry points (include/mvsim.h): built by tests/test_aberrations.py with
 *     gcc -std=c99 -Iinclude tests/c_abi/aberr.c -Lmultiview-simulation_amd -lmvsim -Wl,-rpath,... -lm
 * Exit codes: 0 ok, 3 no usable GPU, 1 anything else. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mvsim.h"

#define CHECK(call)                                                                      \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != MVSIM_OK) {                                                           \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, mvsim_last_error());           \
            return rc_ == MVSIM_ENODEV ? 3 : 1;                                          \
        }                                                                                \
    } while (0)

int main(void)
{
    const int64_t dim[3] = {20, 16, 12};
    const int64_t n = dim[0] * dim[1] * dim[2];
    const int64_t rays = 64;
    mvsim_ctx* ctx = NULL;
    CHECK(mvsim_create(0, &ctx));

    float* img = (float*)malloc((size_t)n * sizeof(float));
    float* ri = (float*)malloc((size_t)n * sizeof(float));
    float* image = (float*)malloc((size_t)n * sizeof(float));
    float* weight = (float*)malloc((size_t)n * sizeof(float));
    for (int64_t i = 0; i < n; ++i) { img[i] = 1.0f; ri[i] = 0.25f; }

    /* no index contrast: every ray walks straight from y = 0 and carries the image's constant value */
    mvsim_ray_steps steps;
    steps.capacity = rays * dim[2];
    steps.n = 0;
    steps.xyz = (double*)malloc((size_t)steps.capacity * 3 * sizeof(double));
    steps.value = (float*)malloc((size_t)steps.capacity * sizeof(float));
    steps.moves = (int32_t*)malloc((size_t)rays * sizeof(int32_t));
    uint64_t state = (2423ull ^ 0x5DEECE66Dull) & ((1ull << 48) - 1);
    const uint64_t state0 = state;
    CHECK(mvsim_refract3d(ctx, img, ri, dim, 0, 6, 1.0, 3.0, 1.1, rays, &state, image, weight, &steps));
    if (state == state0 || steps.n <= 0 || steps.n > steps.capacity) { fprintf(stderr, "implausible step list (%lld steps)\n", (long long)steps.n); return 1; }
    int64_t total = 0;
    for (int64_t r = 0; r < rays; ++r) {
        if (steps.moves[r] < 1 || steps.moves[r] > dim[2]) { fprintf(stderr, "ray %lld made %d moves\n", (long long)r, steps.moves[r]); return 1; }
        if (steps.xyz[3 * total + 1] != 0.0) { fprintf(stderr, "ray %lld does not start at y = 0\n", (long long)r); return 1; }
        total += steps.moves[r];
    }
    if (total != steps.n) { fprintf(stderr, "move counts add up to %lld, not to %lld steps\n", (long long)total, (long long)steps.n); return 1; }
    double wsum = 0.0, isum = 0.0;
    for (int64_t i = 0; i < steps.n; ++i)
        if (fabs(steps.value[i] - 1.0) > 1e-6) { fprintf(stderr, "step %lld carries %.9g\n", (long long)i, steps.value[i]); return 1; }
    for (int64_t i = 0; i < n; ++i) { wsum += weight[i]; isum += image[i]; }
    if (!(wsum > 0.0) || !(isum > 0.0)) { fprintf(stderr, "nothing was injected\n"); return 1; }

    /* VolumeInjection: one normalised Gaussian in the middle adds up to its intensity */
    const double sigma[3] = {0.5, 0.5, 0.5}, at[3] = {10.0, 8.0, 6.0}, inten[1] = {2.0};
    int32_t size[3], num_pixels = 0;
    double sum_weights = 0.0;
    CHECK(mvsim_volume_inject_info(sigma, size, &sum_weights, &num_pixels));
    if (size[0] != 5 || num_pixels != 125) { fprintf(stderr, "box of %d voxels, %d pixels\n", size[0], num_pixels); return 1; }
    memset(image, 0, (size_t)n * sizeof(float));
    memset(weight, 0, (size_t)n * sizeof(float));
    CHECK(mvsim_volume_inject(ctx, image, weight, dim, sigma, at, inten, 1, 1));
    isum = 0.0; wsum = 0.0;
    for (int64_t i = 0; i < n; ++i) { wsum += weight[i]; isum += image[i]; }
    if (fabs(isum - 2.0) > 1e-5 || fabs(wsum - sum_weights) > 1e-5) { fprintf(stderr, "injected %g with weight %g\n", isum, wsum); return 1; }
    float* proj = (float*)malloc((size_t)(dim[0] * dim[1]) * sizeof(float));
    CHECK(mvsim_volume_project(ctx, image, weight, dim, proj));
    if (!(proj[10 + dim[0] * 8] > 0.0f) || proj[0] == proj[0]) { fprintf(stderr, "projection: %g at the point, %g in an empty column\n", proj[10 + dim[0] * 8], proj[0]); return 1; }

    /* the camera: 5 rays per pixel through the same volumes */
    CHECK(mvsim_project_to_camera(ctx, ri, img, dim, 6, 5, &state, proj));
    if (!(proj[3 + dim[0] * 4] > 0.0f)) { fprintf(stderr, "camera pixel %g\n", proj[3 + dim[0] * 4]); return 1; }

    /* argument errors come back as status codes with a message */
    const double bad_sigma[3] = {0.5, 0.0, 0.5};
    if (mvsim_volume_inject(ctx, image, weight, dim, bad_sigma, at, inten, 1, 0) != MVSIM_EINVAL || strlen(mvsim_last_error()) == 0 ||
        mvsim_refract3d(ctx, img, ri, dim, 0, 6, 1.0, 3.0, 1.1, -1, &state, image, weight, NULL) != MVSIM_EINVAL) {
        fprintf(stderr, "bad arguments were not rejected\n");
        return 1;
    }
    printf("aberrations c abi ok: %lld steps of %lld rays\n", (long long)steps.n, (long long)rays);
    free(img); free(ri); free(image); free(weight); free(proj); free(steps.xyz); free(steps.value); free(steps.moves);
    mvsim_destroy(ctx);
    return 0;
}
