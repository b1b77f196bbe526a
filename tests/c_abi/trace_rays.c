/* Plain-C consumer of the ray sandbox's entry points (include/mvsim.h): built by tests/test_trace_rays.py with
 *     gcc -std=c99 -Iinclude tests/c_abi/trace_rays.c -Lmultiview-simulation_amd -lmvsim -Wl,-rpath,... -lm
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
    const int64_t dim[3] = {40, 48, 6};
    const int64_t n = dim[0] * dim[1] * dim[2];
    mvsim_ctx* ctx = NULL;
    CHECK(mvsim_create(0, &ctx));

    /* the wedge, RayTracingTest.drawRays(wedge, 3, 3): 13 rays from y = 23 down */
    float* wedge = (float*)malloc((size_t)n * sizeof(float));
    float* image = (float*)malloc((size_t)n * sizeof(float));
    float* weight = (float*)malloc((size_t)n * sizeof(float));
    CHECK(mvsim_draw_simple_image(ctx, wedge, dim, 1.0f, 1.33f));
    if (wedge[5 + dim[0] * 2] != 1.33f || wedge[2 + dim[0] * 5] != 1.0f || wedge[38 + dim[0] * 1] != 1.33f) { fprintf(stderr, "not the wedge\n"); return 1; }
    int64_t rays = 0;
    CHECK(mvsim_grid_ray_starts(ctx, dim, 3, 3, 0, NULL, NULL, &rays));
    if (rays != 13) { fprintf(stderr, "%lld rays in the grid\n", (long long)rays); return 1; }
    double* pos = (double*)malloc((size_t)rays * 3 * sizeof(double));
    double* dir = (double*)malloc((size_t)rays * 3 * sizeof(double));
    double* end = (double*)malloc((size_t)rays * 3 * sizeof(double));
    CHECK(mvsim_grid_ray_starts(ctx, dim, 3, 3, rays, pos, dir, &rays));
    if (pos[0] != 3.0 || pos[1] != 23.0 || pos[2] != 3.0 || dir[1] != -1.0) { fprintf(stderr, "grid starts at %g %g %g\n", pos[0], pos[1], pos[2]); return 1; }

    mvsim_trace_params tp;
    CHECK(mvsim_trace_params_default(dim, &tp));
    if (tp.max_moves != 4 * (40 + 48 + 6) || tp.ev_threshold != 0.01 || tp.total_reflection != MVSIM_TRACE_KEEP) { fprintf(stderr, "defaults\n"); return 1; }
    mvsim_ray_steps steps;
    steps.capacity = rays * tp.max_moves;
    steps.n = 0;
    steps.xyz = (double*)malloc((size_t)steps.capacity * 3 * sizeof(double));
    steps.value = (float*)malloc((size_t)steps.capacity * sizeof(float));
    steps.moves = (int32_t*)malloc((size_t)rays * sizeof(int32_t));
    int64_t capped = -1;
    CHECK(mvsim_trace_rays(ctx, wedge, NULL, dim, pos, dir, NULL, rays, &tp, image, weight, &steps, end, NULL, &capped));
    int64_t total = 0;
    for (int64_t r = 0; r < rays; ++r) total += steps.moves[r];
    if (capped != 0 || total != steps.n || steps.n < 13 * 20) { fprintf(stderr, "%lld steps, %lld capped\n", (long long)steps.n, (long long)capped); return 1; }
    for (int64_t i = 0; i < steps.n; ++i)
        if (steps.value[i] != 1.0f) { fprintf(stderr, "step %lld carries %.9g\n", (long long)i, steps.value[i]); return 1; }
    if (end[1] >= 0.0 && end[0] >= 0.0 && end[0] <= 39.0 && end[2] >= 0.0 && end[2] <= 5.0) { fprintf(stderr, "ray 0 ends inside\n"); return 1; }
    double wsum = 0.0;
    for (int64_t i = 0; i < n; ++i) wsum += weight[i];
    if (!(wsum > 0.0)) { fprintf(stderr, "nothing was injected\n"); return 1; }

    /* the bundle advances the caller's generator four steps per ray; a Hessian plane */
    uint64_t state = (234345ull ^ 0x5DEECE66Dull) & ((1ull << 48) - 1);
    const uint64_t state0 = state;
    CHECK(mvsim_sandbox_ray_starts(ctx, &state, dim, 20, 3, rays, pos, dir));
    if (state == state0 || pos[1] != 47.0 || fabs(pos[0] - 20.0) > 0.5) { fprintf(stderr, "bundle starts at %g %g\n", pos[0], pos[1]); return 1; }
    CHECK(mvsim_hessian_plane(ctx, wedge, dim, 3, image, NULL));

    tp.max_moves = 0;
    if (mvsim_trace_rays(ctx, wedge, NULL, dim, pos, dir, NULL, rays, &tp, NULL, NULL, NULL, NULL, NULL, NULL) != MVSIM_EINVAL ||
        strlen(mvsim_last_error()) == 0 || mvsim_grid_ray_starts(ctx, dim, 3, 0, 0, NULL, NULL, &rays) != MVSIM_EINVAL) {
        fprintf(stderr, "bad arguments were not rejected\n");
        return 1;
    }
    printf("trace rays c abi ok: %lld steps\n", (long long)steps.n);
    free(wedge); free(image); free(weight); free(pos); free(dir); free(end); free(steps.xyz); free(steps.value); free(steps.moves);
    mvsim_destroy(ctx);
    return 0;
}
