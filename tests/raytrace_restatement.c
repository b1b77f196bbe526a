/* Sequential restatement of the ray sandbox (raytracing/RayTracingTest.java, Raytrace.drawSimpleImage) and of the general tracer
 * under it, for the tests: one ray after the other.  It includes aberr_restatement.c, so the sampler, the Hessian, the eigenpair,
 * bend_ray, the injection and the twin are the ones refract3d's yardstick uses, unchanged.  Built by tests/raytrace_restatement.py
 * with gcc -O2 -ffp-contract=off.
 */
#include "aberr_restatement.c"

#define RT_KEEP 0
#define RT_REFLECT 1

/* bend_ray with the eigenvalue threshold and the total-reflection policy as arguments; *reflected counts the reflections taken.
 * With (0.01, keep) the generic loop calls bend_ray itself. */
static void bend_ray_policy(acc_t* ri, const double pos[3], double vec[3], double nA, double nB, double threshold, int policy,
                            uint64_t* dec, int64_t* reflected)
{
    double m[9], ev3[3], ev;
    acc_set(ri, pos);
    hessian(ri, m);
    ev = rs_largest_eigen(m, ev3);
    *dec = mix(*dec, fabs(ev) > threshold);
    if (fabs(ev) > threshold) {
        double i0, i1, n0, n1, thetaI, thetaT, t[3];
        acc_set(ri, pos);
        acc_move(ri, -vec[0], 0); acc_move(ri, -vec[1], 1); acc_move(ri, -vec[2], 2);
        i0 = acc_get(ri);
        acc_move(ri, 2 * vec[0], 0); acc_move(ri, 2 * vec[1], 1); acc_move(ri, 2 * vec[2], 2);
        i1 = acc_get(ri);
        n0 = (nB - nA) * i0 + nA;
        n1 = (nB - nA) * i1 + nA;
        thetaI = m_acos((ev3[0] * vec[0] + ev3[1] * vec[1] + ev3[2] * vec[2]) /
                        (sqrt(ev3[0] * ev3[0] + ev3[1] * ev3[1] + ev3[2] * ev3[2]) * sqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2])));
        *dec = mix(*dec, 2 + (thetaI >= HALF_PI));
        if (thetaI >= HALF_PI) {
            ev3[0] *= -1; ev3[1] *= -1; ev3[2] *= -1;
            thetaI -= HALF_PI;
        }
        thetaT = rs_refract(vec, ev3, n0, n1, thetaI, t);
        *dec = mix(*dec, 4 + (thetaT != thetaT));
        if (thetaT != thetaT) {
            if (policy == RT_REFLECT) {
                rs_reflect(vec, ev3, t);                 /* RayTracingTest :164, the commented line */
                ++*reflected;
            } else {
                t[0] = vec[0]; t[1] = vec[1]; t[2] = vec[2];
            }
        }
        rs_norm(t);
        vec[0] = t[0]; vec[1] = t[1]; vec[2] = t[2];
    }
}

/* The general loop.  img (may be null), else intensity (floats, may be null), else constant: the value a ray carries, a float.
 * image / weight are added to when inject != 0.  Per ray: moves, decisions (hash as rs_refract3d), end_pos3, end_dir3; *n_capped:
 * rays still inside after max_moves; *n_reflected: reflections taken.  Every output list may be null.  Returns the number of steps. */
int64_t rs_trace_rays(const float* ri_img, const float* img, const int64_t dim[3], const double* pos3, const double* dir3,
                      const float* intensity, int64_t n, double nA, double nB, double threshold, int64_t max_moves, int policy,
                      int normalize_dirs, double constant_value, const double sigma[3], int normalized, float* image, float* weight,
                      double* steps_xyz, float* steps_val, int32_t* moves_out, uint64_t* decisions, double* end_pos3, double* end_dir3,
                      int64_t* n_capped, int64_t* n_reflected, int inject)
{
    acc_t aim, ari;
    inj_t inj;
    int64_t nsteps = 0, capped = 0, reflected = 0;
    aim.img = img; memcpy(aim.dim, dim, sizeof(aim.dim));
    ari.img = ri_img; memcpy(ari.dim, dim, sizeof(ari.dim));
    inj_init(&inj, image, weight, dim, sigma);
    for (int64_t i = 0; i < n; ++i) {
        double pos[3] = {pos3[3 * i], pos3[3 * i + 1], pos3[3 * i + 2]};
        double vec[3] = {dir3[3 * i], dir3[3 * i + 1], dir3[3 * i + 2]};
        int64_t moves = 0;
        uint64_t dec = 0xCBF29CE484222325ULL;
        if (normalize_dirs) rs_norm(vec);
        while (inside(pos, dim) && moves < max_moves) {
            float value = intensity ? intensity[i] : (float)constant_value;
            ++moves;
            if (img) {
                acc_set(&aim, pos);
                value = acc_get(&aim);
            }
            if (policy == RT_KEEP && threshold == 0.01) bend_ray(&ari, pos, vec, nA, nB, &dec);
            else bend_ray_policy(&ari, pos, vec, nA, nB, threshold, policy, &dec, &reflected);
            if (inject) inj_add(&inj, normalized ? (double)value / inj.sum_weights : (double)value, pos);
            for (int d = 0; d < 3; ++d) dec = mix(dec, (uint64_t)jround(pos[d]));
            if (steps_xyz) { steps_xyz[3 * nsteps] = pos[0]; steps_xyz[3 * nsteps + 1] = pos[1]; steps_xyz[3 * nsteps + 2] = pos[2]; }
            if (steps_val) steps_val[nsteps] = value;
            ++nsteps;
            pos[0] += vec[0]; pos[1] += vec[1]; pos[2] += vec[2];
        }
        if (inside(pos, dim)) ++capped;
        if (moves_out) moves_out[i] = (int32_t)moves;
        if (decisions) decisions[i] = dec;
        for (int d = 0; d < 3; ++d) {
            if (end_pos3) end_pos3[3 * i + d] = pos[d];
            if (end_dir3) end_dir3[3 * i + d] = vec[d];
        }
    }
    if (n_capped) *n_capped = capped;
    if (n_reflected) *n_reflected = reflected;
    return nsteps;
}

/* RayTracingTest.drawMultipleRays :110-123 */
void rs_sandbox_ray_starts(uint64_t* rnd_state, const int64_t dim[3], int x, int z, int64_t n, double* pos3, double* dir3)
{
    for (int64_t i = 0; i < n; ++i) {
        double* p = pos3 + 3 * i;
        double* v = dir3 + 3 * i;
        v[0] = 0; v[1] = -1; v[2] = 0;
        rs_norm(v);
        p[0] = x + jr_double(rnd_state) - 0.5;
        p[1] = (int)dim[1] - 1;
        p[2] = z + jr_double(rnd_state) - 0.5;
    }
}

/* RayTracingTest.drawRays :334-344; returns the number of rays (pos3 / dir3 may be null to count) */
int64_t rs_grid_ray_starts(const int64_t dim[3], int z, int spacing, double* pos3, double* dir3)
{
    int64_t k = 0;
    for (int x = spacing; x <= dim[0]; x += spacing, ++k) {
        if (!pos3) continue;
        dir3[3 * k] = 0; dir3[3 * k + 1] = -1; dir3[3 * k + 2] = 0;
        rs_norm(dir3 + 3 * k);
        pos3[3 * k] = x;
        pos3[3 * k + 1] = (int)dim[1] - 25;
        pos3[3 * k + 2] = z;
    }
    return k;
}

/* Raytrace.drawSimpleImage :96-128 */
void rs_draw_simple_image(float* out, const int64_t dim[3], float low, float high)
{
    for (int64_t z = 0; z < dim[2]; ++z)
        for (int64_t y = 0; y < dim[1]; ++y)
            for (int64_t x = 0; x < dim[0]; ++x) {
                int all;
                if (x < dim[0] / 2) all = x > y;
                else all = dim[0] - x > y;
                out[x + dim[0] * (y + dim[1] * z)] = all ? high : low;
            }
}
