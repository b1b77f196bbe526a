// JNI shim: net.preibisch.simulation.gpu.MvsimNative  ->  C ABI of libmvsim.so (include/mvsim.h).
//
// SOURCE ONLY in this repository (the build image has no JDK / jni.h): this file has never been loaded by a JVM.  What runs here:
// a syntax and type check against the hand-written jni.h subset of tests/jni_stub (tests/test_host_logic.py), and the functions
// below EXECUTED against a fake JNIEnv (tests/jni_fake, tests/test_jni_shim.py): the capacity checks, the exception mapping and,
// on the GPU, results bit-identical to the same calls through the C ABI.  Neither says anything about a real JVM.
// Build on a host with a JDK:
//   g++ -shared -fPIC -std=c++17 -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include
//       mvsim_jni.cpp -L../../multiview-simulation_amd -lmvsim -Wl,-rpath,'$ORIGIN' -o libmvsim_jni.so
//
// Every buffer is a direct java.nio.FloatBuffer: GetDirectBufferAddress gives the host pointer and
// GetDirectBufferCapacity its size in floats, which is checked against the dimensions BEFORE the C ABI sees the
// pointer (wrong dims from Java must become an IllegalArgumentException, not an out-of-bounds hipMemcpy).  Nothing is
// retained after a synchronous call returns; the asynchronous view keeps using its buffers until waitView, which the
// Java side guarantees by holding the staging blocks.  Status codes map to IllegalArgumentException (MVSIM_EINVAL),
// OutOfMemoryError (MVSIM_ENOMEM), RuntimeException (rest).  No JNI call is made with an exception pending.
#include <jni.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "mvsim.h"

namespace {

void throw_new(JNIEnv* env, const char* cls, const char* msg)
{
    if (env->ExceptionCheck()) return;                      // keep the first exception
    jclass c = env->FindClass(cls);
    if (c) env->ThrowNew(c, msg);
}

void throw_for(JNIEnv* env, int status)
{
    if (status == MVSIM_OK) return;
    const char* cls = status == MVSIM_EINVAL   ? "java/lang/IllegalArgumentException"
                      : status == MVSIM_ENOMEM ? "java/lang/OutOfMemoryError"
                                               : "java/lang/RuntimeException";
    throw_new(env, cls, mvsim_last_error());
}

// dims {nx, ny, nz}; ok == false after a pending ArrayIndexOutOfBoundsException or non-positive extents
struct Dim {
    int64_t d[3] = {1, 1, 1};
    bool ok = false;
    Dim(JNIEnv* env, jlongArray a)
    {
        if (!a || env->GetArrayLength(a) < 3) { throw_new(env, "java/lang/IllegalArgumentException", "dims: long[3] expected"); return; }
        jlong tmp[3] = {1, 1, 1};
        env->GetLongArrayRegion(a, 0, 3, tmp);
        if (env->ExceptionCheck()) return;
        if (tmp[0] < 1 || tmp[1] < 1 || tmp[2] < 1) { throw_new(env, "java/lang/IllegalArgumentException", "dims must be >= 1"); return; }
        d[0] = tmp[0]; d[1] = tmp[1]; d[2] = tmp[2];
        ok = true;
    }
    int64_t n() const { return d[0] * d[1] * d[2]; }
};

// host pointer of a direct FloatBuffer holding at least `need` floats; nullptr (+ exception) otherwise.
// optional == true: a null buffer is allowed and gives nullptr without an exception.
float* fptr(JNIEnv* env, jobject buf, int64_t need, const char* what, bool optional = false)
{
    if (env->ExceptionCheck()) return nullptr;              // an earlier argument already failed: no JNI call with that pending
    if (!buf) {
        if (!optional) throw_new(env, "java/lang/IllegalArgumentException", what);
        return nullptr;
    }
    void* p = env->GetDirectBufferAddress(buf);
    const jlong cap = env->GetDirectBufferCapacity(buf);    // in elements of the buffer's type
    if (!p || cap < 0) { throw_new(env, "java/lang/IllegalArgumentException", "a direct FloatBuffer is required"); return nullptr; }
    if (cap < need) { throw_new(env, "java/lang/IllegalArgumentException", what); return nullptr; }
    return static_cast<float*>(p);
}

mvsim_ctx* ctx_of(jlong h) { return reinterpret_cast<mvsim_ctx*>(static_cast<intptr_t>(h)); }
mvsim_group* group_of(jlong h) { return reinterpret_cast<mvsim_group*>(static_cast<intptr_t>(h)); }

void fill_params(mvsim_view_params* p, jint axis, jint degrees, jdouble delta, jfloat min_value, jfloat target, jint inc, jfloat snr,
                 jlong seed, jint stream)
{
    mvsim_view_params_default(p);
    p->axis = axis; p->degrees = degrees; p->delta = delta; p->min_value = min_value; p->target_average = target;
    p->inc = inc; p->snr = snr; p->seed = static_cast<uint64_t>(seed); p->stream = static_cast<uint32_t>(stream);
}

}  // namespace

extern "C" {

#define JNI_FN(name) Java_net_preibisch_simulation_gpu_MvsimNative_##name

JNIEXPORT jlong JNICALL JNI_FN(create)(JNIEnv* env, jclass, jint device)
{
    mvsim_ctx* c = nullptr;
    throw_for(env, mvsim_create(device, &c));
    return static_cast<jlong>(reinterpret_cast<intptr_t>(c));
}

JNIEXPORT void JNICALL JNI_FN(destroy)(JNIEnv*, jclass, jlong h) { mvsim_destroy(ctx_of(h)); }

JNIEXPORT jint JNICALL JNI_FN(deviceCount)(JNIEnv*, jclass)
{
    int n = 0;
    mvsim_device_count(&n);
    return n;
}

JNIEXPORT void JNICALL JNI_FN(rotateAroundAxis)(JNIEnv* env, jclass, jlong h, jobject in, jlongArray dim, jint axis,
                                                jint degrees, jobject out)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* pi = fptr(env, in, d.n(), "rotateAroundAxis: input buffer smaller than the dimensions");
    float* po = fptr(env, out, d.n(), "rotateAroundAxis: output buffer smaller than the dimensions");
    if (!pi || !po) return;
    throw_for(env, mvsim_rotate_around_axis(ctx_of(h), pi, d.d, axis, degrees, po));
}

JNIEXPORT void JNICALL JNI_FN(attenuate3d)(JNIEnv* env, jclass, jlong h, jobject in, jlongArray dim, jdouble delta,
                                           jobject out)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* pi = fptr(env, in, d.n(), "attenuate3d: input buffer smaller than the dimensions");
    float* po = fptr(env, out, d.n(), "attenuate3d: output buffer smaller than the dimensions");
    if (!pi || !po) return;
    throw_for(env, mvsim_attenuate3d(ctx_of(h), pi, d.d, delta, po));
}

JNIEXPORT void JNICALL JNI_FN(normImage)(JNIEnv* env, jclass, jlong h, jobject img, jlong n)
{
    float* p = fptr(env, img, n, "normImage: buffer smaller than n");
    if (!p) return;
    throw_for(env, mvsim_norm_image(ctx_of(h), p, n));
}

JNIEXPORT void JNICALL JNI_FN(convolve)(JNIEnv* env, jclass, jlong h, jobject img, jlongArray dim, jobject psf,
                                        jlongArray kdim, jint method, jobject out)
{
    Dim d(env, dim);
    if (!d.ok) return;
    Dim k(env, kdim);
    if (!k.ok) return;
    float* pi = fptr(env, img, d.n(), "convolve: image buffer smaller than the dimensions");
    float* pp = fptr(env, psf, k.n(), "convolve: PSF buffer smaller than its dimensions");
    float* po = fptr(env, out, d.n(), "convolve: output buffer smaller than the dimensions");
    if (!pi || !pp || !po) return;
    throw_for(env, mvsim_convolve(ctx_of(h), pi, d.d, pp, k.d, method, po));
}

JNIEXPORT jdouble JNICALL JNI_FN(adjustImage)(JNIEnv* env, jclass, jlong h, jobject img, jlong n, jfloat min_value,
                                              jfloat target)
{
    double corr = 0.0;
    float* p = fptr(env, img, n, "adjustImage: buffer smaller than n");
    if (!p) return corr;
    throw_for(env, mvsim_adjust_image(ctx_of(h), p, n, min_value, target, &corr));
    return corr;
}

JNIEXPORT void JNICALL JNI_FN(extractSlices)(JNIEnv* env, jclass, jlong h, jobject in, jlongArray dim, jint inc,
                                             jfloat snr, jlong seed, jint stream, jobject out)
{
    Dim d(env, dim);
    if (!d.ok) return;
    if (inc < 1) { throw_new(env, "java/lang/IllegalArgumentException", "extractSlices: inc must be >= 1"); return; }
    float* pi = fptr(env, in, d.n(), "extractSlices: input buffer smaller than the dimensions");
    float* po = fptr(env, out, d.d[0] * d.d[1] * mvsim_extract_nz(d.d[2], inc), "extractSlices: output buffer smaller than (Nz-1)/inc+1 planes");
    if (!pi || !po) return;
    throw_for(env, mvsim_extract_slices(ctx_of(h), pi, d.d, inc, snr, static_cast<uint64_t>(seed), static_cast<uint32_t>(stream), po));
}

JNIEXPORT void JNICALL JNI_FN(poissonProcess)(JNIEnv* env, jclass, jlong h, jobject img, jlong n, jdouble snr,
                                              jlong seed, jint stream, jlong index_offset)
{
    float* p = fptr(env, img, n, "poissonProcess: buffer smaller than n");
    if (!p) return;
    throw_for(env, mvsim_poisson_process(ctx_of(h), p, n, snr, static_cast<uint64_t>(seed), static_cast<uint32_t>(stream),
                                         static_cast<uint64_t>(index_offset)));
}

JNIEXPORT void JNICALL JNI_FN(makeIsotropic)(JNIEnv* env, jclass, jlong h, jobject in, jlongArray dim, jint inc,
                                             jobject out)
{
    Dim d(env, dim);
    if (!d.ok) return;
    if (inc < 1) { throw_new(env, "java/lang/IllegalArgumentException", "makeIsotropic: inc must be >= 1"); return; }
    float* pi = fptr(env, in, d.n(), "makeIsotropic: input buffer smaller than the dimensions");
    float* po = fptr(env, out, d.d[0] * d.d[1] * mvsim_isotropic_nz(d.d[2], inc), "makeIsotropic: output buffer smaller than (Nz-1)*inc+1 planes");
    if (!pi || !po) return;
    throw_for(env, mvsim_make_isotropic(ctx_of(h), pi, d.d, inc, po));
}

JNIEXPORT void JNICALL JNI_FN(computeWeightImage)(JNIEnv* env, jclass, jlong h, jlongArray dim, jobject out)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* po = fptr(env, out, d.n(), "computeWeightImage: output buffer smaller than the dimensions");
    if (!po) return;
    throw_for(env, mvsim_compute_weight_image(ctx_of(h), d.d, po));
}

JNIEXPORT void JNICALL JNI_FN(axisRotation)(JNIEnv* env, jclass, jlongArray dim, jint axis, jint degrees,
                                            jdoubleArray m12)
{
    Dim d(env, dim);
    if (!d.ok) return;
    if (!m12 || env->GetArrayLength(m12) < 12) { throw_new(env, "java/lang/IllegalArgumentException", "axisRotation: double[12] expected"); return; }
    double m[12];
    const int rc = mvsim_axis_rotation(d.d, axis, degrees, m);
    if (rc != MVSIM_OK) { throw_for(env, rc); return; }
    env->SetDoubleArrayRegion(m12, 0, 12, m);
}

// ---- bead images (mvsim_render_beads) -----------------------------------------------------------------------------------
namespace {
// host pointer of a direct buffer (any element type) holding at least `need` elements; nullptr (+ exception) otherwise
void* any_ptr(JNIEnv* env, jobject buf, int64_t need, const char* what)
{
    if (env->ExceptionCheck()) return nullptr;
    if (!buf) { throw_new(env, "java/lang/IllegalArgumentException", what); return nullptr; }
    void* p = env->GetDirectBufferAddress(buf);
    const jlong cap = env->GetDirectBufferCapacity(buf);
    if (!p || cap < need) { throw_new(env, "java/lang/IllegalArgumentException", what); return nullptr; }
    return p;
}
}  // namespace

JNIEXPORT void JNICALL JNI_FN(renderBeads)(JNIEnv* env, jclass, jlong h, jobject xyz, jlong n, jlongArray view_offsets, jobject m12,
                                           jint nviews, jlongArray interval, jdouble sx, jdouble sy, jdouble sz, jobjectArray out_f32,
                                           jobjectArray out_u16)
{
    if (nviews < 1 || n < 0) { throw_new(env, "java/lang/IllegalArgumentException", "renderBeads: nviews >= 1 and n >= 0 expected"); return; }
    if (!interval || env->GetArrayLength(interval) < 6) { throw_new(env, "java/lang/IllegalArgumentException", "renderBeads: long[6] interval expected"); return; }
    jlong iv[6];
    env->GetLongArrayRegion(interval, 0, 6, iv);
    if (env->ExceptionCheck()) return;
    int64_t mn[3] = {iv[0], iv[1], iv[2]}, mx[3] = {iv[3], iv[4], iv[5]};
    for (int d = 0; d < 3; ++d)
        if (mx[d] - mn[d] < 1) { throw_new(env, "java/lang/IllegalArgumentException", "renderBeads: image dimension (max - min) must be >= 1"); return; }
    const int64_t nv = (mx[0] - mn[0]) * (mx[1] - mn[1]) * (mx[2] - mn[2]);
    const double* pts = nullptr;
    if (n > 0) {
        pts = static_cast<const double*>(any_ptr(env, xyz, 3 * n, "renderBeads: point buffer smaller than 3 n doubles"));
        if (!pts) return;
    }
    std::vector<int64_t> offs;
    if (view_offsets) {
        if (env->GetArrayLength(view_offsets) != nviews + 1) { throw_new(env, "java/lang/IllegalArgumentException", "renderBeads: nviews + 1 offsets expected"); return; }
        offs.resize(static_cast<size_t>(nviews) + 1);
        std::vector<jlong> tmp(offs.size());
        env->GetLongArrayRegion(view_offsets, 0, nviews + 1, tmp.data());
        if (env->ExceptionCheck()) return;
        for (size_t i = 0; i < tmp.size(); ++i) offs[i] = tmp[i];
    }
    const double* m = nullptr;
    if (m12) {
        m = static_cast<const double*>(any_ptr(env, m12, 12 * static_cast<int64_t>(nviews), "renderBeads: matrix buffer smaller than 12 nviews doubles"));
        if (!m) return;
    }
    std::vector<float*> f;
    std::vector<uint16_t*> u;
    for (int k = 0; k < 2; ++k) {
        jobjectArray list = k == 0 ? out_f32 : out_u16;
        if (!list) continue;
        if (env->GetArrayLength(list) != nviews) { throw_new(env, "java/lang/IllegalArgumentException", "renderBeads: one output buffer per view expected"); return; }
        for (jint v = 0; v < nviews; ++v) {
            jobject b = env->GetObjectArrayElement(list, v);
            if (env->ExceptionCheck()) return;
            void* p = any_ptr(env, b, nv, "renderBeads: output buffer smaller than the image");
            if (!p) return;
            if (k == 0) f.push_back(static_cast<float*>(p)); else u.push_back(static_cast<uint16_t*>(p));
        }
    }
    const double sigma[3] = {sx, sy, sz};
    throw_for(env, mvsim_render_beads(ctx_of(h), pts, view_offsets ? offs.data() : nullptr, n, m, nviews, mn, mx, sigma,
                                      out_f32 ? f.data() : nullptr, out_u16 ? u.data() : nullptr));
}

// ---- the refraction simulator (mvsim_refract3d, mvsim_project_to_camera) ------------------------------------------------
namespace {
// the 48-bit java.util.Random state in rnd_state[0]; false (+ exception) when the array is missing
bool state_in(JNIEnv* env, jlongArray rnd_state, const char* what, uint64_t* state)
{
    if (env->ExceptionCheck()) return false;
    if (!rnd_state || env->GetArrayLength(rnd_state) < 1) { throw_new(env, "java/lang/IllegalArgumentException", what); return false; }
    jlong st = 0;
    env->GetLongArrayRegion(rnd_state, 0, 1, &st);
    if (env->ExceptionCheck()) return false;
    *state = static_cast<uint64_t>(st);
    return true;
}
}  // namespace

JNIEXPORT void JNICALL JNI_FN(refract3d)(JNIEnv* env, jclass, jlong h, jobject img, jobject ri_img, jlongArray dim, jboolean illum, jint z,
                                         jdouble ls_middle, jdouble ls_edge, jdouble ri, jlong num_rays, jlongArray rnd_state, jobject image,
                                         jobject weight)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* pi = fptr(env, img, d.n(), "refract3d: image buffer smaller than the dimensions");
    float* pr = fptr(env, ri_img, d.n(), "refract3d: refractive-index buffer smaller than the dimensions");
    float* po = fptr(env, image, d.n(), "refract3d: output image buffer smaller than the dimensions");
    float* pw = fptr(env, weight, d.n(), "refract3d: output weight buffer smaller than the dimensions");
    if (!pi || !pr || !po || !pw) return;
    uint64_t state = 0;
    if (!state_in(env, rnd_state, "refract3d: long[1] state expected", &state)) return;
    const int rc = mvsim_refract3d(ctx_of(h), pi, pr, d.d, illum ? 1 : 0, z, ls_middle, ls_edge, ri, num_rays, &state, po, pw, nullptr);
    if (rc != MVSIM_OK) { throw_for(env, rc); return; }
    const jlong st = static_cast<jlong>(state);
    env->SetLongArrayRegion(rnd_state, 0, 1, &st);
}

JNIEXPORT void JNICALL JNI_FN(projectToCamera)(JNIEnv* env, jclass, jlong h, jobject ri_img, jobject refr, jlongArray dim, jint current_z,
                                               jint rays_per_pixel, jlongArray rnd_state, jobject proj)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* pr = fptr(env, ri_img, d.n(), "projectToCamera: refractive-index buffer smaller than the dimensions");
    float* pf = fptr(env, refr, d.n(), "projectToCamera: refracted-volume buffer smaller than the dimensions");
    float* pp = fptr(env, proj, d.d[0] * d.d[1], "projectToCamera: output buffer smaller than one plane");
    if (!pr || !pf || !pp) return;
    uint64_t state = 0;
    if (!state_in(env, rnd_state, "projectToCamera: long[1] state expected", &state)) return;
    const int rc = mvsim_project_to_camera(ctx_of(h), pr, pf, d.d, current_z, rays_per_pixel, &state, pp);
    if (rc != MVSIM_OK) { throw_for(env, rc); return; }
    const jlong st = static_cast<jlong>(state);
    env->SetLongArrayRegion(rnd_state, 0, 1, &st);
}

// ---- the ray sandbox (mvsim_trace_rays, mvsim_draw_simple_image, mvsim_sandbox_ray_starts) ------------------------------------------
// pos3 / dir3: direct DoubleBuffers of 3 n doubles; img_in and intensity may be null; image and weight are given together or both
// null.  The injection is the sandbox's (sigma 0.5, normalized).  Returns the number of rays still inside after max_moves moves.
JNIEXPORT jlong JNICALL JNI_FN(traceRays)(JNIEnv* env, jclass, jlong h, jobject ri_img, jobject img_in, jlongArray dim, jobject pos3,
                                          jobject dir3, jobject intensity, jlong n, jdouble n_a, jdouble n_b, jdouble ev_threshold,
                                          jlong max_moves, jint total_reflection, jboolean normalize_dirs, jdouble constant_value,
                                          jobject image, jobject weight)
{
    Dim d(env, dim);
    if (!d.ok) return 0;
    if (n < 0) { throw_new(env, "java/lang/IllegalArgumentException", "traceRays: negative number of rays"); return 0; }
    float* pr = fptr(env, ri_img, d.n(), "traceRays: refractive-index buffer smaller than the dimensions");
    if (!pr) return 0;
    float* pi = fptr(env, img_in, d.n(), "traceRays: image buffer smaller than the dimensions", true);
    float* pv = fptr(env, intensity, n, "traceRays: intensity buffer smaller than n floats", true);
    float* po = fptr(env, image, d.n(), "traceRays: output image buffer smaller than the dimensions", true);
    float* pw = fptr(env, weight, d.n(), "traceRays: output weight buffer smaller than the dimensions", true);
    if (env->ExceptionCheck()) return 0;
    const double* pp = nullptr;
    const double* pd = nullptr;
    if (n > 0) {
        pp = static_cast<const double*>(any_ptr(env, pos3, 3 * n, "traceRays: position buffer smaller than 3 n doubles"));
        if (!pp) return 0;
        pd = static_cast<const double*>(any_ptr(env, dir3, 3 * n, "traceRays: direction buffer smaller than 3 n doubles"));
        if (!pd) return 0;
    }
    mvsim_trace_params tp;
    int rc = mvsim_trace_params_default(d.d, &tp);
    if (rc != MVSIM_OK) { throw_for(env, rc); return 0; }
    tp.n_a = n_a; tp.n_b = n_b; tp.ev_threshold = ev_threshold; tp.max_moves = max_moves; tp.total_reflection = total_reflection;
    tp.normalize_dirs = normalize_dirs ? 1 : 0; tp.constant_value = constant_value;
    int64_t capped = 0;
    rc = mvsim_trace_rays(ctx_of(h), pr, pi, d.d, pp, pd, pv, n, &tp, po, pw, nullptr, nullptr, nullptr, &capped);
    if (rc != MVSIM_OK) { throw_for(env, rc); return 0; }
    return static_cast<jlong>(capped);
}

JNIEXPORT void JNICALL JNI_FN(drawSimpleImage)(JNIEnv* env, jclass, jlong h, jobject out, jlongArray dim, jfloat low, jfloat high)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* po = fptr(env, out, d.n(), "drawSimpleImage: buffer smaller than the dimensions");
    if (!po) return;
    throw_for(env, mvsim_draw_simple_image(ctx_of(h), po, d.d, low, high));
}

JNIEXPORT void JNICALL JNI_FN(sandboxRayStarts)(JNIEnv* env, jclass, jlong h, jlongArray rnd_state, jlongArray dim, jint x, jint z, jlong n,
                                                jobject pos3, jobject dir3)
{
    Dim d(env, dim);
    if (!d.ok) return;
    if (n < 0) { throw_new(env, "java/lang/IllegalArgumentException", "sandboxRayStarts: negative number of rays"); return; }
    double* pp = static_cast<double*>(any_ptr(env, pos3, 3 * n, "sandboxRayStarts: position buffer smaller than 3 n doubles"));
    if (!pp) return;
    double* pd = static_cast<double*>(any_ptr(env, dir3, 3 * n, "sandboxRayStarts: direction buffer smaller than 3 n doubles"));
    if (!pd) return;
    uint64_t state = 0;
    if (!state_in(env, rnd_state, "sandboxRayStarts: long[1] state expected", &state)) return;
    const int rc = mvsim_sandbox_ray_starts(ctx_of(h), &state, d.d, x, z, n, pp, pd);
    if (rc != MVSIM_OK) { throw_for(env, rc); return; }
    const jlong st = static_cast<jlong>(state);
    env->SetLongArrayRegion(rnd_state, 0, 1, &st);
}

// ---- per-stage operators with z-slab lists (mvsim_*_zslabs) ----------------------------------------------------------
namespace {
// the host pointers and plane counts of a FloatBuffer[] / long[] pair; every buffer is checked against plane * nz[i] floats
// and the planes against `planes` before the C ABI sees anything.  ok == false: an exception is pending.
struct SlabArgs {
    std::vector<float*>  ptr;
    std::vector<int64_t> nz;
    bool ok = false;
    SlabArgs(JNIEnv* env, jobjectArray bufs, jlongArray counts, int64_t plane, int64_t planes, const char* what)
    {
        if (!bufs || !counts) { throw_new(env, "java/lang/IllegalArgumentException", what); return; }
        const jsize n = env->GetArrayLength(bufs);
        if (n < 1 || env->GetArrayLength(counts) != n) { throw_new(env, "java/lang/IllegalArgumentException", what); return; }
        std::vector<jlong> c(static_cast<size_t>(n));
        env->GetLongArrayRegion(counts, 0, n, c.data());
        if (env->ExceptionCheck()) return;
        int64_t total = 0;
        for (jsize i = 0; i < n; ++i) {
            if (c[i] < 1) { throw_new(env, "java/lang/IllegalArgumentException", what); return; }
            jobject b = env->GetObjectArrayElement(bufs, i);
            if (env->ExceptionCheck()) return;
            float* p = fptr(env, b, plane * c[i], what);
            if (!p) return;
            ptr.push_back(p);
            nz.push_back(c[i]);
            total += c[i];
        }
        if (total != planes) { throw_new(env, "java/lang/IllegalArgumentException", what); return; }
        ok = true;
    }
};
}  // namespace

JNIEXPORT void JNICALL JNI_FN(rotateAroundAxisSlabs)(JNIEnv* env, jclass, jlong h, jobjectArray in, jlongArray in_nz, jlongArray dim,
                                                     jint axis, jint degrees, jobjectArray out, jlongArray out_nz)
{
    Dim d(env, dim);
    if (!d.ok) return;
    SlabArgs si(env, in, in_nz, d.d[0] * d.d[1], d.d[2], "rotateAroundAxis: input slabs do not match the dimensions");
    if (!si.ok) return;
    SlabArgs so(env, out, out_nz, d.d[0] * d.d[1], d.d[2], "rotateAroundAxis: output slabs do not match the dimensions");
    if (!so.ok) return;
    throw_for(env, mvsim_rotate_around_axis_zslabs(ctx_of(h), si.ptr.data(), si.nz.data(), (int)si.ptr.size(), d.d, axis, degrees,
                                                   so.ptr.data(), so.nz.data(), (int)so.ptr.size()));
}

JNIEXPORT void JNICALL JNI_FN(attenuate3dSlabs)(JNIEnv* env, jclass, jlong h, jobjectArray in, jlongArray in_nz, jlongArray dim,
                                                jdouble delta, jobjectArray out, jlongArray out_nz)
{
    Dim d(env, dim);
    if (!d.ok) return;
    SlabArgs si(env, in, in_nz, d.d[0] * d.d[1], d.d[2], "attenuate3d: input slabs do not match the dimensions");
    if (!si.ok) return;
    SlabArgs so(env, out, out_nz, d.d[0] * d.d[1], d.d[2], "attenuate3d: output slabs do not match the dimensions");
    if (!so.ok) return;
    throw_for(env, mvsim_attenuate3d_zslabs(ctx_of(h), si.ptr.data(), si.nz.data(), (int)si.ptr.size(), d.d, delta, so.ptr.data(),
                                            so.nz.data(), (int)so.ptr.size()));
}

JNIEXPORT void JNICALL JNI_FN(convolveSlabs)(JNIEnv* env, jclass, jlong h, jobjectArray in, jlongArray in_nz, jlongArray dim, jobject psf,
                                             jlongArray kdim, jint method, jobjectArray out, jlongArray out_nz)
{
    Dim d(env, dim);
    if (!d.ok) return;
    Dim k(env, kdim);
    if (!k.ok) return;
    float* pp = fptr(env, psf, k.n(), "convolve: PSF buffer smaller than its dimensions");
    if (!pp) return;
    SlabArgs si(env, in, in_nz, d.d[0] * d.d[1], d.d[2], "convolve: input slabs do not match the dimensions");
    if (!si.ok) return;
    SlabArgs so(env, out, out_nz, d.d[0] * d.d[1], d.d[2], "convolve: output slabs do not match the dimensions");
    if (!so.ok) return;
    throw_for(env, mvsim_convolve_zslabs(ctx_of(h), si.ptr.data(), si.nz.data(), (int)si.ptr.size(), d.d, pp, k.d, method, so.ptr.data(),
                                         so.nz.data(), (int)so.ptr.size()));
}

JNIEXPORT void JNICALL JNI_FN(extractSlicesSlabs)(JNIEnv* env, jclass, jlong h, jobjectArray in, jlongArray in_nz, jlongArray dim, jint inc,
                                                  jfloat snr, jlong seed, jint stream, jobjectArray out, jlongArray out_nz)
{
    Dim d(env, dim);
    if (!d.ok) return;
    if (inc < 1) { throw_new(env, "java/lang/IllegalArgumentException", "extractSlices: inc must be >= 1"); return; }
    SlabArgs si(env, in, in_nz, d.d[0] * d.d[1], d.d[2], "extractSlices: input slabs do not match the dimensions");
    if (!si.ok) return;
    SlabArgs so(env, out, out_nz, d.d[0] * d.d[1], mvsim_extract_nz(d.d[2], inc), "extractSlices: output slabs do not hold (Nz-1)/inc+1 planes");
    if (!so.ok) return;
    throw_for(env, mvsim_extract_slices_zslabs(ctx_of(h), si.ptr.data(), si.nz.data(), (int)si.ptr.size(), d.d, inc, snr,
                                               static_cast<uint64_t>(seed), static_cast<uint32_t>(stream), so.ptr.data(), so.nz.data(),
                                               (int)so.ptr.size()));
}

JNIEXPORT jobject JNICALL JNI_FN(allocPinned)(JNIEnv* env, jclass, jlong h, jlong bytes)
{
    void* p = nullptr;
    if (bytes <= 0 || mvsim_host_alloc(ctx_of(h), static_cast<size_t>(bytes), &p) != MVSIM_OK || !p) return nullptr;
    jobject b = env->NewDirectByteBuffer(p, bytes);
    if (!b) (void)mvsim_host_free(nullptr, p);              // the JVM could not wrap it: do not leak the block
    return b;
}

JNIEXPORT void JNICALL JNI_FN(freePinned)(JNIEnv* env, jclass, jobject block)
{
    if (block) (void)mvsim_host_free(nullptr, env->GetDirectBufferAddress(block));
}

// Bulk copies between a Java float[] and a (page-locked) direct block on the library's host threads (mvsim_host_copy).  The array is
// held with GetPrimitiveArrayCritical for the duration of the copy -- the worker threads touch plain memory, never the JNIEnv, and no
// JNI call is made inside the critical region (JNI specification, "GetPrimitiveArrayCritical").  to_array == JNI_TRUE: block -> array
// (Buffers.toImg's copy into the NEW ArrayImg every operator of the reference returns, SimulateMultiViewDataset.java:109,198: the
// threads also take the array's first-touch page faults in parallel); JNI_FALSE: array -> block (Buffers.toBlock / toSlabs).
JNIEXPORT void JNICALL JNI_FN(copyFloats)(JNIEnv* env, jclass, jlong h, jobject block, jlong block_off, jfloatArray array, jint array_off,
                                          jint count, jboolean to_array)
{
    if (count == 0) return;
    if (!array || count < 0 || array_off < 0 || block_off < 0 || (jlong)array_off + count > env->GetArrayLength(array)) {
        throw_new(env, "java/lang/ArrayIndexOutOfBoundsException", "copyFloats: range outside the array");
        return;
    }
    float* b = fptr(env, block, block_off + count, "copyFloats: range outside the block");
    if (!b) return;
    void* a = env->GetPrimitiveArrayCritical(array, nullptr);
    if (!a) { throw_new(env, "java/lang/OutOfMemoryError", "copyFloats: GetPrimitiveArrayCritical"); return; }
    float* arr = static_cast<float*>(a) + array_off;
    const int rc = to_array ? mvsim_host_copy(ctx_of(h), arr, b + block_off, static_cast<size_t>(count) * sizeof(float))
                            : mvsim_host_copy(ctx_of(h), b + block_off, arr, static_cast<size_t>(count) * sizeof(float));
    env->ReleasePrimitiveArrayCritical(array, a, to_array ? 0 : JNI_ABORT);   // array -> block: nothing to write back
    throw_for(env, rc);
}

JNIEXPORT jlong JNICALL JNI_FN(drawSpheres)(JNIEnv* env, jclass, jlong h, jobject img, jlongArray dim, jdouble min_value,
                                            jdouble max_value, jint scale, jboolean half_pixel_offset, jlongArray rnd_state)
{
    Dim d(env, dim);
    if (!d.ok) return 0;
    float* p = fptr(env, img, d.n(), "drawSpheres: buffer smaller than the dimensions");
    if (!p) return 0;
    if (!rnd_state || env->GetArrayLength(rnd_state) < 1) { throw_new(env, "java/lang/IllegalArgumentException", "drawSpheres: long[1] state expected"); return 0; }
    jlong st = 0;
    env->GetLongArrayRegion(rnd_state, 0, 1, &st);
    if (env->ExceptionCheck()) return 0;
    uint64_t state = static_cast<uint64_t>(st);
    int64_t n = 0;
    const int rc = mvsim_draw_spheres(ctx_of(h), p, d.d, min_value, max_value, scale, half_pixel_offset ? 1 : 0, &state, &n);
    if (rc != MVSIM_OK) { throw_for(env, rc); return 0; }
    st = static_cast<jlong>(state);
    env->SetLongArrayRegion(rnd_state, 0, 1, &st);
    return static_cast<jlong>(n);
}

// ---- the refraction simulator's phantom (mvsim_ri_noise, mvsim_multi_spheres): the generator state in and out through long[1] ----
JNIEXPORT void JNICALL JNI_FN(riNoise)(JNIEnv* env, jclass, jlong h, jobject ri, jlong n, jlongArray rnd_state)
{
    if (n < 0) { throw_new(env, "java/lang/IllegalArgumentException", "riNoise: negative count"); return; }
    float* p = fptr(env, ri, n, "riNoise: buffer smaller than the count", n == 0);
    if (!p && n > 0) return;
    uint64_t state = 0;
    if (!state_in(env, rnd_state, "riNoise: long[1] state expected", &state)) return;
    const int rc = mvsim_ri_noise(ctx_of(h), p, n, &state);
    if (rc != MVSIM_OK) { throw_for(env, rc); return; }
    const jlong st = static_cast<jlong>(state);
    env->SetLongArrayRegion(rnd_state, 0, 1, &st);
}

JNIEXPORT jlong JNICALL JNI_FN(multiSpheres)(JNIEnv* env, jclass, jlong h, jobject img, jobject ri, jlongArray dim, jint scale,
                                             jlongArray rnd_state)
{
    Dim d(env, dim);
    if (!d.ok) return 0;
    float* pi = fptr(env, img, d.n(), "multiSpheres: image buffer smaller than the dimensions");
    float* pr = fptr(env, ri, d.n(), "multiSpheres: index buffer smaller than the dimensions");
    if (!pi || !pr) return 0;
    uint64_t state = 0;
    if (!state_in(env, rnd_state, "multiSpheres: long[1] state expected", &state)) return 0;
    int64_t n = 0;
    const int rc = mvsim_multi_spheres(ctx_of(h), pi, pr, d.d, scale, &state, &n);
    if (rc != MVSIM_OK) { throw_for(env, rc); return 0; }
    const jlong st = static_cast<jlong>(state);
    env->SetLongArrayRegion(rnd_state, 0, 1, &st);
    return static_cast<jlong>(n);
}

// out[0] = stream positions per chunk of the device walk, out[1] = entry offsets resolved per chunk
JNIEXPORT void JNICALL JNI_FN(sphereWalkGeometry)(JNIEnv* env, jclass, jlongArray out)
{
    if (!out || env->GetArrayLength(out) < 2) { throw_new(env, "java/lang/IllegalArgumentException", "sphereWalkGeometry: long[2] expected"); return; }
    int64_t chunk = 0;
    int entries = 0;
    const int rc = mvsim_sphere_walk_geometry(&chunk, &entries);
    if (rc != MVSIM_OK) { throw_for(env, rc); return; }
    const jlong v[2] = {static_cast<jlong>(chunk), static_cast<jlong>(entries)};
    env->SetLongArrayRegion(out, 0, 2, v);
}

JNIEXPORT void JNICALL JNI_FN(splatSpheres)(JNIEnv* env, jclass, jlong h, jobject img, jlongArray dim, jintArray geometry,
                                            jfloatArray values)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* p = fptr(env, img, d.n(), "splatSpheres: buffer smaller than the dimensions");
    if (!p) return;
    if (!geometry || !values) { throw_new(env, "java/lang/IllegalArgumentException", "splatSpheres: null sphere list"); return; }
    const jsize n = env->GetArrayLength(values);
    if (env->GetArrayLength(geometry) != 4 * n) { throw_new(env, "java/lang/IllegalArgumentException", "splatSpheres: 4 ints per sphere expected"); return; }
    std::vector<jint> g(static_cast<size_t>(4 * n));
    std::vector<jfloat> v(static_cast<size_t>(n));
    if (n > 0) {
        env->GetIntArrayRegion(geometry, 0, 4 * n, g.data());
        if (env->ExceptionCheck()) return;
        env->GetFloatArrayRegion(values, 0, n, v.data());
        if (env->ExceptionCheck()) return;
    }
    std::vector<mvsim_sphere> s(static_cast<size_t>(n));
    for (jsize i = 0; i < n; ++i) s[i] = mvsim_sphere{g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3], v[i]};
    throw_for(env, mvsim_splat_spheres(ctx_of(h), p, d.d, s.data(), static_cast<int64_t>(n)));
}

JNIEXPORT void JNICALL JNI_FN(downSample2x)(JNIEnv* env, jclass, jlong h, jobject in, jlongArray dim, jobject out)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* pi = fptr(env, in, d.n(), "downSample2x: input buffer smaller than the dimensions");
    const int64_t no = (d.d[0] / 2 - 1) * (d.d[1] / 2 - 1) * (d.d[2] / 2 - 1);
    float* po = fptr(env, out, no > 0 ? no : 0, "downSample2x: output buffer smaller than (N/2-1)^3");
    if (!pi || !po) return;
    throw_for(env, mvsim_downsample2x(ctx_of(h), pi, d.d, po));
}

// ---- volumes that stay on the device, and extractSlices over their intervals (mvsim_dev_alloc / _free / mvsim_upload / mvsim_extract_intervals)
JNIEXPORT jlong JNICALL JNI_FN(devAlloc)(JNIEnv* env, jclass, jlong h, jlong bytes)
{
    if (bytes < 1) { throw_new(env, "java/lang/IllegalArgumentException", "devAlloc: bytes >= 1 expected"); return 0; }
    void* p = nullptr;
    throw_for(env, mvsim_dev_alloc(ctx_of(h), static_cast<size_t>(bytes), &p));
    return static_cast<jlong>(reinterpret_cast<intptr_t>(p));
}

JNIEXPORT void JNICALL JNI_FN(devFree)(JNIEnv* env, jclass, jlong h, jlong dptr)
{
    if (dptr != 0) throw_for(env, mvsim_dev_free(ctx_of(h), reinterpret_cast<void*>(static_cast<intptr_t>(dptr))));
}

JNIEXPORT void JNICALL JNI_FN(uploadFloats)(JNIEnv* env, jclass, jlong h, jlong dptr, jobject src, jlong n)
{
    if (dptr == 0 || n < 1) { throw_new(env, "java/lang/IllegalArgumentException", "uploadFloats: a device pointer and n >= 1 expected"); return; }
    float* p = fptr(env, src, n, "uploadFloats: source buffer smaller than n");
    if (!p) return;
    throw_for(env, mvsim_upload(ctx_of(h), reinterpret_cast<void*>(static_cast<intptr_t>(dptr)), p, static_cast<size_t>(n) * sizeof(float)));
}

// geometry: 10 longs per job {volume (device pointer), Nx, Ny, Nz, min x, y, z, max x, y, z}; inc, snr, seed, stream: one entry per job;
// out: one direct FloatBuffer per job holding the tile, tx * ty * mvsim_extract_nz(tz, inc) floats
JNIEXPORT void JNICALL JNI_FN(extractIntervals)(JNIEnv* env, jclass, jlong h, jlongArray geometry, jintArray inc, jfloatArray snr, jlongArray seed,
                                                jintArray stream, jobjectArray out)
{
    if (!geometry || !inc || !snr || !seed || !stream || !out) { throw_new(env, "java/lang/IllegalArgumentException", "extractIntervals: null array"); return; }
    const jsize n = env->GetArrayLength(out);
    if (n < 1 || n > MVSIM_MAX_VIEWS) { throw_new(env, "java/lang/IllegalArgumentException", "extractIntervals: 1..32 jobs"); return; }
    if (env->GetArrayLength(geometry) != 10 * n || env->GetArrayLength(inc) != n || env->GetArrayLength(snr) != n || env->GetArrayLength(seed) != n ||
        env->GetArrayLength(stream) != n) {
        throw_new(env, "java/lang/IllegalArgumentException", "extractIntervals: 10 geometry entries and one inc, snr, seed and stream per output expected");
        return;
    }
    jlong g[10 * MVSIM_MAX_VIEWS], sd[MVSIM_MAX_VIEWS];
    jint ic[MVSIM_MAX_VIEWS], st[MVSIM_MAX_VIEWS];
    jfloat sn[MVSIM_MAX_VIEWS];
    env->GetLongArrayRegion(geometry, 0, 10 * n, g);
    if (env->ExceptionCheck()) return;
    env->GetIntArrayRegion(inc, 0, n, ic);
    if (env->ExceptionCheck()) return;
    env->GetFloatArrayRegion(snr, 0, n, sn);
    if (env->ExceptionCheck()) return;
    env->GetLongArrayRegion(seed, 0, n, sd);
    if (env->ExceptionCheck()) return;
    env->GetIntArrayRegion(stream, 0, n, st);
    if (env->ExceptionCheck()) return;
    mvsim_interval_job jobs[MVSIM_MAX_VIEWS];
    float* ptr[MVSIM_MAX_VIEWS];
    for (jsize j = 0; j < n; ++j) {
        mvsim_interval_job& job = jobs[j];
        const jlong* q = g + 10 * j;
        job.in = reinterpret_cast<const float*>(static_cast<intptr_t>(q[0]));
        for (int d = 0; d < 3; ++d) { job.dim[d] = q[1 + d]; job.min[d] = q[4 + d]; job.max[d] = q[7 + d]; }
        job.inc = ic[j]; job.snr = sn[j]; job.seed = static_cast<uint64_t>(sd[j]); job.stream = static_cast<uint32_t>(st[j]);
        int64_t od[3];
        if (mvsim_interval_out_dim(&job, od) != MVSIM_OK) { throw_for(env, MVSIM_EINVAL); return; }      // host only: no pointer is touched
        jobject b = env->GetObjectArrayElement(out, j);
        if (env->ExceptionCheck()) return;
        ptr[j] = fptr(env, b, od[0] * od[1] * od[2], "extractIntervals: output buffer smaller than the tile");
        if (!ptr[j]) return;
    }
    throw_for(env, mvsim_extract_intervals(ctx_of(h), jobs, (int)n, ptr));
}

JNIEXPORT void JNICALL JNI_FN(normalizeWeights)(JNIEnv* env, jclass, jlong h, jobjectArray weights, jlong n, jfloat osem)
{
    if (!weights) { throw_new(env, "java/lang/IllegalArgumentException", "normalizeWeights: null list"); return; }
    const jsize nv = env->GetArrayLength(weights);
    if (nv < 1 || nv > MVSIM_MAX_VIEWS) { throw_new(env, "java/lang/IllegalArgumentException", "normalizeWeights: 1..32 views"); return; }
    float* ptr[MVSIM_MAX_VIEWS];
    for (jsize v = 0; v < nv; ++v) {
        jobject b = env->GetObjectArrayElement(weights, v);
        if (env->ExceptionCheck()) return;
        ptr[v] = fptr(env, b, n, "normalizeWeights: view buffer smaller than n");
        if (!ptr[v]) return;
    }
    throw_for(env, mvsim_normalize_weights(ctx_of(h), ptr, (int)nv, n, osem));
}

JNIEXPORT jdouble JNICALL JNI_FN(simulateView)(JNIEnv* env, jclass, jlong h, jobject gt, jlongArray dim, jobject psf,
                                               jlongArray kdim, jint axis, jint degrees, jdouble delta,
                                               jfloat min_value, jfloat target, jint inc, jfloat snr, jlong seed,
                                               jint stream, jobject rot, jobject att, jobject con, jobject acq)
{
    double corr = 0.0;
    Dim d(env, dim);
    if (!d.ok) return corr;
    Dim k(env, kdim);
    if (!k.ok) return corr;
    if (inc < 1) { throw_new(env, "java/lang/IllegalArgumentException", "simulateView: inc must be >= 1"); return corr; }
    float* pg = fptr(env, gt, d.n(), "simulateView: ground-truth buffer smaller than the dimensions");
    float* pp = fptr(env, psf, k.n(), "simulateView: PSF buffer smaller than its dimensions");
    float* pa = fptr(env, acq, d.d[0] * d.d[1] * mvsim_extract_nz(d.d[2], inc), "simulateView: acquisition buffer too small");
    if (!pg || !pp || !pa) return corr;
    mvsim_view_outputs o = {fptr(env, rot, d.n(), "simulateView: rot buffer too small", true), fptr(env, att, d.n(), "simulateView: att buffer too small", true),
                            fptr(env, con, d.n(), "simulateView: con buffer too small", true), pa};
    if (env->ExceptionCheck()) return corr;
    mvsim_view_params p;
    fill_params(&p, axis, degrees, delta, min_value, target, inc, snr, seed, stream);
    throw_for(env, mvsim_simulate_view(ctx_of(h), pg, d.d, pp, k.d, &p, &o, &corr));
    return corr;
}

JNIEXPORT jlong JNICALL JNI_FN(simulateViewAsync)(JNIEnv* env, jclass, jlong h, jobject gt, jlong gt_generation, jlongArray dim,
                                                  jobject psf, jlongArray kdim, jint axis, jint degrees, jdouble delta, jfloat min_value,
                                                  jfloat target, jint inc, jfloat snr, jlong seed, jint stream, jobject acq)
{
    Dim d(env, dim);
    if (!d.ok) return -1;
    Dim k(env, kdim);
    if (!k.ok) return -1;
    if (inc < 1) { throw_new(env, "java/lang/IllegalArgumentException", "simulateViewAsync: inc must be >= 1"); return -1; }
    float* pg = fptr(env, gt, d.n(), "simulateViewAsync: ground-truth buffer smaller than the dimensions");
    float* pp = fptr(env, psf, k.n(), "simulateViewAsync: PSF buffer smaller than its dimensions");
    float* pa = fptr(env, acq, d.d[0] * d.d[1] * mvsim_extract_nz(d.d[2], inc), "simulateViewAsync: acquisition buffer too small");
    if (!pg || !pp || !pa) return -1;
    mvsim_view_params p;
    fill_params(&p, axis, degrees, delta, min_value, target, inc, snr, seed, stream);
    mvsim_view_outputs o = {nullptr, nullptr, nullptr, pa};
    int64_t ticket = -1;
    throw_for(env, mvsim_simulate_view_async(ctx_of(h), pg, static_cast<uint64_t>(gt_generation), d.d, pp, k.d, &p, &o, &ticket));
    return static_cast<jlong>(ticket);
}

JNIEXPORT jdouble JNICALL JNI_FN(waitView)(JNIEnv* env, jclass, jlong h, jlong ticket)
{
    double corr = 0.0;
    throw_for(env, mvsim_wait(ctx_of(h), ticket, &corr));
    return corr;
}

JNIEXPORT void JNICALL JNI_FN(waitViewQuiet)(JNIEnv*, jclass, jlong h, jlong ticket) { (void)mvsim_wait(ctx_of(h), ticket, nullptr); }

// mvsim_simulate_views: V views of one ground truth in one call (host buffers; the library stacks them when they cannot fill the chip
// one at a time and brings the acquisitions back as 16-bit counts)
JNIEXPORT void JNICALL JNI_FN(simulateViewsBatch)(JNIEnv* env, jclass, jlong h, jobject gt, jlongArray dim, jobjectArray psfs, jlongArray kdim,
                                                  jintArray degrees, jdouble delta, jfloat min_value, jfloat target, jint inc, jfloat snr,
                                                  jlongArray seeds, jobjectArray acqs)
{
    Dim d(env, dim);
    if (!d.ok) return;
    Dim k(env, kdim);
    if (!k.ok) return;
    if (inc < 1) { throw_new(env, "java/lang/IllegalArgumentException", "simulateViewsBatch: inc must be >= 1"); return; }
    if (!psfs || !degrees || !seeds || !acqs) { throw_new(env, "java/lang/IllegalArgumentException", "simulateViewsBatch: null argument"); return; }
    const jsize n = env->GetArrayLength(degrees);
    if (env->GetArrayLength(psfs) != n || env->GetArrayLength(seeds) != n || env->GetArrayLength(acqs) != n) {
        throw_new(env, "java/lang/IllegalArgumentException", "simulateViewsBatch: one PSF, seed and acquisition buffer per view");
        return;
    }
    float* pg = fptr(env, gt, d.n(), "simulateViewsBatch: ground-truth buffer smaller than the dimensions");
    if (!pg) return;
    const int64_t acq_floats = d.d[0] * d.d[1] * mvsim_extract_nz(d.d[2], inc);
    std::vector<jint> deg(static_cast<size_t>(n));
    std::vector<jlong> sd(static_cast<size_t>(n));
    if (n > 0) {
        env->GetIntArrayRegion(degrees, 0, n, deg.data());
        if (env->ExceptionCheck()) return;
        env->GetLongArrayRegion(seeds, 0, n, sd.data());
        if (env->ExceptionCheck()) return;
    }
    std::vector<float*> pp(static_cast<size_t>(n)), pa(static_cast<size_t>(n));
    std::vector<mvsim_view_params> par(static_cast<size_t>(n));
    for (jsize v = 0; v < n; ++v) {
        jobject b = env->GetObjectArrayElement(psfs, v);
        if (env->ExceptionCheck()) return;
        pp[v] = fptr(env, b, k.n(), "simulateViewsBatch: PSF buffer smaller than its dimensions");
        jobject a = env->GetObjectArrayElement(acqs, v);
        if (env->ExceptionCheck()) return;
        pa[v] = fptr(env, a, acq_floats, "simulateViewsBatch: acquisition buffer smaller than nx * ny * ((nz - 1) / inc + 1) floats");
        if (!pp[v] || !pa[v]) return;
        fill_params(&par[v], 0, deg[v], delta, min_value, target, inc, snr, sd[v], v);
    }
    throw_for(env, mvsim_simulate_views(ctx_of(h), pg, d.d, pp.data(), k.d, par.data(), pa.data(), (int)n));
}

// mvsim_deconvolve: the multi-view deconvolution on host buffers.  kdims: 3 extents per view; weights: null, or one buffer per view;
// psi: the start estimate where init_from_psi is set, the result always.  Every length and capacity is checked before the C ABI sees a pointer.
JNIEXPORT void JNICALL JNI_FN(deconvolve)(JNIEnv* env, jclass, jlong h, jobjectArray views, jobjectArray weights, jobjectArray psfs,
                                          jlongArray kdims, jlongArray dim, jint iterations, jint method, jboolean init_from_psi,
                                          jfloat init_value, jfloat min_value, jfloat eps, jdouble lambda, jobject psi)
{
    Dim d(env, dim);
    if (!d.ok) return;
    if (!views || !psfs || !kdims) { throw_new(env, "java/lang/IllegalArgumentException", "deconvolve: null argument"); return; }
    const jsize nv = env->GetArrayLength(views);
    if (nv < 1 || nv > MVSIM_MAX_VIEWS) { throw_new(env, "java/lang/IllegalArgumentException", "deconvolve: 1..32 views"); return; }
    if (env->GetArrayLength(psfs) != nv || env->GetArrayLength(kdims) != 3 * nv || (weights && env->GetArrayLength(weights) != nv)) {
        throw_new(env, "java/lang/IllegalArgumentException", "deconvolve: one PSF, three PSF extents and (with weights) one weight buffer per view");
        return;
    }
    jlong kd[3 * MVSIM_MAX_VIEWS];
    env->GetLongArrayRegion(kdims, 0, 3 * nv, kd);
    if (env->ExceptionCheck()) return;
    int64_t k64[3 * MVSIM_MAX_VIEWS];
    const float *pv[MVSIM_MAX_VIEWS], *pw[MVSIM_MAX_VIEWS], *pp[MVSIM_MAX_VIEWS];
    for (jsize v = 0; v < nv; ++v) {
        for (int a = 0; a < 3; ++a) {
            k64[3 * v + a] = kd[3 * v + a];
            if (kd[3 * v + a] < 1 || kd[3 * v + a] > 65535) { throw_new(env, "java/lang/IllegalArgumentException", "deconvolve: PSF extents must be in 1..65535"); return; }
        }
        jobject b = env->GetObjectArrayElement(views, v);
        if (env->ExceptionCheck()) return;
        pv[v] = fptr(env, b, d.n(), "deconvolve: view buffer smaller than the dimensions");
        if (!pv[v]) return;                                 // (no JNI call with that exception pending)
        b = env->GetObjectArrayElement(psfs, v);
        if (env->ExceptionCheck()) return;
        pp[v] = fptr(env, b, k64[3 * v] * k64[3 * v + 1] * k64[3 * v + 2], "deconvolve: PSF buffer smaller than its dimensions");
        if (!pp[v]) return;
        pw[v] = nullptr;
        if (weights) {
            b = env->GetObjectArrayElement(weights, v);
            if (env->ExceptionCheck()) return;
            pw[v] = fptr(env, b, d.n(), "deconvolve: weight buffer smaller than the dimensions");
            if (!pw[v]) return;
        }
    }
    float* ps = fptr(env, psi, d.n(), "deconvolve: estimate buffer smaller than the dimensions");
    if (!ps) return;
    mvsim_decon_params p;
    mvsim_decon_params_default(&p);
    p.iterations = iterations; p.method = method; p.init_from_psi = init_from_psi ? 1 : 0; p.init_value = init_value;
    p.min_value = min_value; p.eps = eps; p.lambda = lambda;
    throw_for(env, mvsim_deconvolve(ctx_of(h), pv, weights ? pw : nullptr, pp, k64, (int)nv, d.d, &p, ps, nullptr));
}

// mvsim_detect_beads: DoG interest points with sub-voxel localisation on a host image.  img: a direct FloatBuffer, or (u16) a direct
// ShortBuffer, of nx * ny * nz elements; peaks: a direct ByteBuffer of at least 40 * capacity bytes that receives min(found, capacity)
// mvsim_peak records {double pos[3]; float value; int flags; long voxel} in native byte order.  Returns the number found.  Every length
// and capacity is checked before the C ABI sees a pointer.
JNIEXPORT jlong JNICALL JNI_FN(detectBeads)(JNIEnv* env, jclass, jlong h, jobject img, jboolean u16, jlongArray dim, jdouble s1x, jdouble s1y,
                                            jdouble s1z, jdouble s2x, jdouble s2y, jdouble s2z, jfloat threshold, jint max_moves,
                                            jlong capacity, jobject peaks)
{
    Dim d(env, dim);
    if (!d.ok) return 0;
    if (capacity < 1 || capacity > (static_cast<jlong>(1) << 31)) {
        throw_new(env, "java/lang/IllegalArgumentException", "detectBeads: capacity must be in 1 .. 2^31");
        return 0;
    }
    mvsim_dog_params p;
    mvsim_dog_params_default(&p);
    p.sigma1[0] = s1x; p.sigma1[1] = s1y; p.sigma1[2] = s1z;
    p.sigma2[0] = s2x; p.sigma2[1] = s2y; p.sigma2[2] = s2z;
    p.threshold = threshold;
    p.max_moves = max_moves;
    const void* src = any_ptr(env, img, d.n(), "detectBeads: image buffer missing or smaller than the dimensions");
    if (!src) return 0;
    void* out = any_ptr(env, peaks, capacity * static_cast<jlong>(sizeof(mvsim_peak)), "detectBeads: peak buffer missing or smaller than 40 * capacity bytes");
    if (!out) return 0;
    int64_t found = 0;
    throw_for(env, mvsim_detect_beads(ctx_of(h), src, u16 ? MVSIM_SRC_U16 : MVSIM_SRC_F32, d.d, &p, capacity, static_cast<mvsim_peak*>(out), &found));
    return static_cast<jlong>(found);
}

// mvsim_register_beads: bead-based registration A -> B of two packed position lists (direct DoubleBuffers of 3 n doubles).  result: a
// direct ByteBuffer of at least 160 bytes that receives one mvsim_registration {double m[12], meanError, maxError; long nA, nB,
// nCandidates, nInliers, bestHypothesis; int refits, flags} in native byte order; candidates (or null): at least 24 * max(nA, 1) bytes
// for the mvsim_match records {int a, b; double vBest, vSecond}; mask (or null): at least max(nA, 1) bytes, one per candidate.  Returns
// the number of candidates.  Every length, null and capacity is checked before the C ABI sees a pointer.
JNIEXPORT jlong JNICALL JNI_FN(registerBeads)(JNIEnv* env, jclass, jlong h, jobject pos_a, jlong n_a, jobject pos_b, jlong n_b, jint redundancy,
                                              jdouble ratio, jdouble max_epsilon, jdouble min_inlier_ratio, jlong seed, jint hypotheses,
                                              jint max_refits, jint min_inliers, jobject result, jobject candidates, jobject mask)
{
    if (n_a < 0 || n_a > MVSIM_REG_MAX_POINTS || n_b < 0 || n_b > MVSIM_REG_MAX_POINTS) {
        throw_new(env, "java/lang/IllegalArgumentException", "registerBeads: list lengths must be in 0 .. 65536");
        return 0;
    }
    const void* pa = any_ptr(env, pos_a, 3 * n_a, "registerBeads: position buffer A missing or smaller than 3 nA doubles");
    if (!pa) return 0;
    const void* pb = any_ptr(env, pos_b, 3 * n_b, "registerBeads: position buffer B missing or smaller than 3 nB doubles");
    if (!pb) return 0;
    void* res = any_ptr(env, result, static_cast<jlong>(sizeof(mvsim_registration)), "registerBeads: result buffer missing or smaller than 160 bytes");
    if (!res) return 0;
    const jlong slots = n_a > 0 ? n_a : 1;
    void* cand = nullptr;
    void* msk = nullptr;
    if (candidates) {
        cand = any_ptr(env, candidates, slots * static_cast<jlong>(sizeof(mvsim_match)), "registerBeads: candidate buffer smaller than 24 * max(nA, 1) bytes");
        if (!cand) return 0;
    }
    if (mask) {
        msk = any_ptr(env, mask, slots, "registerBeads: mask buffer smaller than max(nA, 1) bytes");
        if (!msk) return 0;
    }
    mvsim_match_params p;
    mvsim_match_params_default(&p);
    p.redundancy = redundancy; p.ratio = ratio; p.max_epsilon = max_epsilon; p.min_inlier_ratio = min_inlier_ratio; p.seed = seed;
    p.hypotheses = hypotheses; p.max_refits = max_refits; p.min_inliers = min_inliers;
    mvsim_registration r;
    const int rc = mvsim_register_beads(ctx_of(h), pa, 24, n_a, pb, 24, n_b, &p, &r, static_cast<mvsim_match*>(cand), static_cast<unsigned char*>(msk));
    if (rc != MVSIM_OK) { throw_for(env, rc); return 0; }
    std::memcpy(res, &r, sizeof(r));
    return static_cast<jlong>(r.n_candidates);
}

// ---- view fusion (mvsim_fuse_views, mvsim_align_views) ---------------------------------------------------------------------------
namespace {
// The views of a fusion call: direct Float- or (u16) ShortBuffers of the extents in dims (3 longs per view) with one 3 x 4 matrix each
// in a direct DoubleBuffer of 12 V doubles.  ok == false after an exception.  Every length, null and capacity is checked here.
struct FuseArgs {
    mvsim_fuse_view v[MVSIM_MAX_VIEWS];
    int64_t out_min[3], out_dim[3];
    mvsim_fuse_params p;
    int32_t* status = nullptr;
    jsize n = 0;
    bool ok = false;
    FuseArgs(JNIEnv* env, jobjectArray views, jboolean u16, jlongArray dims, jobject m12, jlongArray omin, jlongArray odim, jdouble bx, jdouble by,
             jdouble bz, jfloat background, jobject status_buf)
    {
        const char* iae = "java/lang/IllegalArgumentException";
        if (!views || !dims || !m12 || !omin || !odim) { throw_new(env, iae, "fuse: null argument"); return; }
        n = env->GetArrayLength(views);
        if (n < 1 || n > MVSIM_MAX_VIEWS) { throw_new(env, iae, "fuse: 1..32 views"); return; }
        if (env->GetArrayLength(dims) != 3 * n) { throw_new(env, iae, "fuse: three extents per view"); return; }
        if (env->GetArrayLength(omin) < 3) { throw_new(env, iae, "fuse: outMin: long[3] expected"); return; }
        Dim od(env, odim);
        if (!od.ok) return;
        jlong mn[3], nd[3 * MVSIM_MAX_VIEWS];
        env->GetLongArrayRegion(omin, 0, 3, mn);
        if (env->ExceptionCheck()) return;
        env->GetLongArrayRegion(dims, 0, 3 * n, nd);
        if (env->ExceptionCheck()) return;
        const double* m = static_cast<const double*>(any_ptr(env, m12, 12 * static_cast<int64_t>(n), "fuse: matrix buffer missing or smaller than 12 doubles per view"));
        if (!m) return;
        for (int a = 0; a < 3; ++a) { out_min[a] = mn[a]; out_dim[a] = od.d[a]; }
        for (jsize k = 0; k < n; ++k) {
            for (int a = 0; a < 3; ++a) {
                if (nd[3 * k + a] < 1 || nd[3 * k + a] > 0x7fffffff) { throw_new(env, iae, "fuse: view extents must be in 1 .. 2^31-1"); return; }
                v[k].dim[a] = nd[3 * k + a];
            }
            jobject b = env->GetObjectArrayElement(views, k);
            if (env->ExceptionCheck()) return;
            v[k].src = any_ptr(env, b, v[k].dim[0] * v[k].dim[1] * v[k].dim[2], "fuse: view buffer missing or smaller than its dimensions");
            if (!v[k].src) return;
            v[k].m_dev = nullptr;
            std::memcpy(v[k].m, m + 12 * k, sizeof(v[k].m));
        }
        if (status_buf) {
            status = static_cast<int32_t*>(any_ptr(env, status_buf, n, "fuse: status buffer smaller than one int per view"));
            if (!status) return;
        }
        mvsim_fuse_params_default(&p);
        p.blend[0] = bx; p.blend[1] = by; p.blend[2] = bz;
        p.background = background;
        p.src_type = u16 ? MVSIM_SRC_U16 : MVSIM_SRC_F32;
        ok = true;
    }
    int64_t out_n() const { return out_dim[0] * out_dim[1] * out_dim[2]; }
};
}  // namespace

// mvsim_fuse_views: the blended average of the views in the interval outMin, outDim.  fused: a direct FloatBuffer of prod(outDim) floats;
// sumWeights (or null): the same; status (or null): a direct IntBuffer of one int per view (MVSIM_FUSE_SINGULAR).
JNIEXPORT void JNICALL JNI_FN(fuseViews)(JNIEnv* env, jclass, jlong h, jobjectArray views, jboolean u16, jlongArray dims, jobject m12,
                                         jlongArray out_min, jlongArray out_dim, jdouble blend_x, jdouble blend_y, jdouble blend_z,
                                         jfloat background, jobject fused, jobject sum_weights, jobject status)
{
    FuseArgs a(env, views, u16, dims, m12, out_min, out_dim, blend_x, blend_y, blend_z, background, status);
    if (!a.ok) return;
    float* out = fptr(env, fused, a.out_n(), "fuseViews: output buffer missing or smaller than the interval");
    if (!out) return;
    float* sw = fptr(env, sum_weights, a.out_n(), "fuseViews: sum-of-weights buffer smaller than the interval", true);
    if (sum_weights && !sw) return;
    throw_for(env, mvsim_fuse_views(ctx_of(h), a.v, static_cast<int>(a.n), a.out_min, a.out_dim, &a.p, out, sw, a.status));
}

// mvsim_align_views: one resampled volume and one weight volume per view.  aligned: direct FloatBuffers of prod(outDim) floats, entries
// may be null; weights: null, or the same.
JNIEXPORT void JNICALL JNI_FN(alignViews)(JNIEnv* env, jclass, jlong h, jobjectArray views, jboolean u16, jlongArray dims, jobject m12,
                                          jlongArray out_min, jlongArray out_dim, jdouble blend_x, jdouble blend_y, jdouble blend_z,
                                          jobjectArray aligned, jobjectArray weights, jobject status)
{
    FuseArgs a(env, views, u16, dims, m12, out_min, out_dim, blend_x, blend_y, blend_z, 0.0f, status);
    if (!a.ok) return;
    if (!aligned || env->GetArrayLength(aligned) != a.n || (weights && env->GetArrayLength(weights) != a.n)) {
        throw_new(env, "java/lang/IllegalArgumentException", "alignViews: one output entry (and, with weights, one weight entry) per view");
        return;
    }
    float *al[MVSIM_MAX_VIEWS], *wt[MVSIM_MAX_VIEWS];
    for (jsize k = 0; k < a.n; ++k) {
        jobject b = env->GetObjectArrayElement(aligned, k);
        if (env->ExceptionCheck()) return;
        al[k] = fptr(env, b, a.out_n(), "alignViews: output buffer smaller than the interval", true);
        if (b && !al[k]) return;
        wt[k] = nullptr;
        if (weights) {
            b = env->GetObjectArrayElement(weights, k);
            if (env->ExceptionCheck()) return;
            wt[k] = fptr(env, b, a.out_n(), "alignViews: weight buffer smaller than the interval", true);
            if (b && !wt[k]) return;
        }
    }
    throw_for(env, mvsim_align_views(ctx_of(h), a.v, static_cast<int>(a.n), a.out_min, a.out_dim, &a.p, al, weights ? wt : nullptr, a.status));
}

// ---- PSF extraction (mvsim_extract_psf) ---------------------------------------------------------------------------------------------
// The PSF of one view from its beads.  img: a direct Float- or (u16) ShortBuffer of prod(dim) voxels; pos: a direct DoubleBuffer of 3 n
// doubles; use (or null): a direct ByteBuffer of n bytes; m12 (or null: the identity): a direct DoubleBuffer of 12 doubles, view -> output
// frame; psf: a direct FloatBuffer of prod(kdim) floats; result: a direct ByteBuffer of at least 72 bytes that receives one
// mvsim_psf_result {double minimum, sum; long nListed, nUsed, nNonfinite, nMasked, nOutside, nCrowded; int flags, pad} in native byte
// order; status (or null): a direct ByteBuffer of max(n, 1) bytes.  Returns the number of beads used.  Every length, null and capacity is
// checked before the C ABI sees a pointer.
JNIEXPORT jlong JNICALL JNI_FN(extractPsf)(JNIEnv* env, jclass, jlong h, jobject img, jboolean u16, jlongArray dim, jobject pos, jlong n,
                                           jobject use, jobject m12, jlongArray kdim, jdouble sep_x, jdouble sep_y, jdouble sep_z,
                                           jboolean subtract_min, jboolean normalize, jobject psf, jobject result, jobject status)
{
    const char* iae = "java/lang/IllegalArgumentException";
    if (n < 0 || n > MVSIM_PSF_MAX_POINTS) { throw_new(env, iae, "extractPsf: the list length must be in 0 .. 65536"); return 0; }
    Dim d(env, dim);
    if (!d.ok) return 0;
    Dim k(env, kdim);
    if (!k.ok) return 0;
    for (int a = 0; a < 3; ++a) {
        if (d.d[a] > 0x7fffffff) { throw_new(env, iae, "extractPsf: image extents must be in 1 .. 2^31-1"); return 0; }
        if (k.d[a] > MVSIM_PSF_MAX_DIM || (k.d[a] & 1) == 0) { throw_new(env, iae, "extractPsf: PSF extents must be odd and in 1 .. 63"); return 0; }
    }
    const void* src = any_ptr(env, img, d.n(), "extractPsf: image buffer missing or smaller than its dimensions");
    if (!src) return 0;
    const void* p = any_ptr(env, pos, 3 * n, "extractPsf: position buffer missing or smaller than 3 n doubles");
    if (!p) return 0;
    const void* u = nullptr;
    if (use) {
        u = any_ptr(env, use, n, "extractPsf: use buffer smaller than n bytes");
        if (!u) return 0;
    }
    const void* m = nullptr;
    if (m12) {
        m = any_ptr(env, m12, 12, "extractPsf: matrix buffer smaller than 12 doubles");
        if (!m) return 0;
    }
    float* out = fptr(env, psf, k.n(), "extractPsf: PSF buffer missing or smaller than its dimensions");
    if (!out) return 0;
    void* res = any_ptr(env, result, static_cast<jlong>(sizeof(mvsim_psf_result)), "extractPsf: result buffer missing or smaller than 72 bytes");
    if (!res) return 0;
    void* st = nullptr;
    if (status) {
        st = any_ptr(env, status, n > 0 ? n : 1, "extractPsf: status buffer smaller than max(n, 1) bytes");
        if (!st) return 0;
    }
    mvsim_psf_params q;
    mvsim_psf_params_default(&q);
    for (int a = 0; a < 3; ++a) q.kdim[a] = k.d[a];
    q.min_separation[0] = sep_x; q.min_separation[1] = sep_y; q.min_separation[2] = sep_z;
    q.src_type = u16 ? MVSIM_SRC_U16 : MVSIM_SRC_F32;
    q.subtract_min = subtract_min ? 1 : 0;
    q.normalize = normalize ? 1 : 0;
    mvsim_psf_result r;
    const int rc = mvsim_extract_psf(ctx_of(h), src, d.d, p, 24, n, static_cast<const unsigned char*>(u), static_cast<const double*>(m), &q, out, &r,
                                     static_cast<unsigned char*>(st));
    if (rc != MVSIM_OK) { throw_for(env, rc); return 0; }
    std::memcpy(res, &r, sizeof(r));
    return static_cast<jlong>(r.n_used);
}

// ---- mvsim_group_* -------------------------------------------------------------------------------------------------
JNIEXPORT jlong JNICALL JNI_FN(groupCreate)(JNIEnv* env, jclass, jint ndev)
{
    mvsim_group* g = nullptr;
    throw_for(env, mvsim_group_create(ndev, nullptr, &g));
    return static_cast<jlong>(reinterpret_cast<intptr_t>(g));
}

JNIEXPORT void JNICALL JNI_FN(groupDestroy)(JNIEnv*, jclass, jlong g) { mvsim_group_destroy(group_of(g)); }

JNIEXPORT void JNICALL JNI_FN(groupBroadcastVolume)(JNIEnv* env, jclass, jlong g, jobject gt, jlongArray dim)
{
    Dim d(env, dim);
    if (!d.ok) return;
    float* p = fptr(env, gt, d.n(), "groupBroadcastVolume: buffer smaller than the dimensions");
    if (!p) return;
    throw_for(env, mvsim_group_broadcast_volume(group_of(g), p, d.d));
}

JNIEXPORT void JNICALL JNI_FN(groupSimulateViews)(JNIEnv* env, jclass, jlong g, jobjectArray psfs, jlongArray kdim, jlongArray dim,
                                                  jintArray degrees, jdouble delta, jfloat min_value, jfloat target, jint inc, jfloat snr,
                                                  jlongArray seeds, jobjectArray acqs)
{
    Dim k(env, kdim);
    if (!k.ok) return;
    Dim d(env, dim);                                       // the dimensions of the broadcast ground truth (GpuGroup keeps them)
    if (!d.ok) return;
    if (inc < 1) { throw_new(env, "java/lang/IllegalArgumentException", "groupSimulateViews: inc must be >= 1"); return; }
    const int64_t acq_floats = d.d[0] * d.d[1] * mvsim_extract_nz(d.d[2], inc);
    if (!psfs || !degrees || !seeds || !acqs) { throw_new(env, "java/lang/IllegalArgumentException", "groupSimulateViews: null argument"); return; }
    const jsize n = env->GetArrayLength(degrees);
    if (env->GetArrayLength(psfs) != n || env->GetArrayLength(seeds) != n || env->GetArrayLength(acqs) != n) {
        throw_new(env, "java/lang/IllegalArgumentException", "groupSimulateViews: one PSF, seed and acquisition buffer per view");
        return;
    }
    std::vector<jint> deg(static_cast<size_t>(n));
    std::vector<jlong> sd(static_cast<size_t>(n));
    if (n > 0) {
        env->GetIntArrayRegion(degrees, 0, n, deg.data());
        if (env->ExceptionCheck()) return;
        env->GetLongArrayRegion(seeds, 0, n, sd.data());
        if (env->ExceptionCheck()) return;
    }
    std::vector<float*> pp(static_cast<size_t>(n)), pa(static_cast<size_t>(n));
    std::vector<mvsim_view_params> par(static_cast<size_t>(n));
    for (jsize v = 0; v < n; ++v) {
        jobject b = env->GetObjectArrayElement(psfs, v);
        if (env->ExceptionCheck()) return;
        pp[v] = fptr(env, b, k.n(), "groupSimulateViews: PSF buffer smaller than its dimensions");
        jobject a = env->GetObjectArrayElement(acqs, v);
        if (env->ExceptionCheck()) return;
        // the C ABI takes no capacity: an undersized direct buffer would take an out-of-bounds copy, so it is refused here
        pa[v] = fptr(env, a, acq_floats, "groupSimulateViews: acquisition buffer smaller than nx * ny * ((nz - 1) / inc + 1) floats");
        if (!pp[v] || !pa[v]) return;
        fill_params(&par[v], 0, deg[v], delta, min_value, target, inc, snr, sd[v], v);
    }
    throw_for(env, mvsim_group_simulate_views(group_of(g), pp.data(), k.d, par.data(), (int)n, pa.data()));
}

}  // extern "C"
