/*
 * mvsim.h -- C ABI of libmvsim.so: MI355X (gfx950) implementation of the per-view
 * acquisition pipeline of net.preibisch.simulation.SimulateMultiViewDataset
 *
 *     rotate -> attenuate -> 3-D PSF convolve -> adjust -> axial slice extraction -> Poisson
 *
 * The reference is pure Java with NO foreign-function interface for this path; each entry
 * point below names the Java static method (file:line in the reference tree) whose body it
 * replaces.  The Java-side binding a maintainer would add (JNI shim + facade with the same
 * signatures) is in java/ and described in INTEGRATION.md.
 *
 *   SMVD  = src/main/java/net/preibisch/simulation/SimulateMultiViewDataset.java
 *   Tools = src/main/java/net/preibisch/simulation/Tools.java
 *
 * Conventions
 *   - all images are IEEE float32, x fastest: index = x + Nx*(y + Ny*z)  (ArrayImg order)
 *   - dim[3] = {Nx, Ny, Nz};  kdim[3] likewise for the PSF
 *   - every function returns 0 (MVSIM_OK) or a negative status; mvsim_last_error() gives the
 *     thread-local message of the last failure.  No C++ exception crosses this boundary.
 *   - "host" entry points: caller owns every buffer, pre-sized; the call is synchronous and
 *     keeps no reference to the pointers afterwards.
 *   - "_dev" entry points: pointers are device (HBM) addresses valid on the context's GPU;
 *     work is enqueued on the context's stream (mvsim_set_stream) and the call returns
 *     without synchronising unless stated.
 *   - a context is bound to one GPU and is NOT thread-safe; use one per host thread.
 *   - there is no CPU fallback: without a usable gfx950 device mvsim_create fails.
 */
#ifndef MVSIM_H
#define MVSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVSIM_OK       0
#define MVSIM_EINVAL  (-1)   /* bad dims / axis / inc / null pointer              */
#define MVSIM_ENOMEM  (-2)   /* device or host allocation failed                  */
#define MVSIM_EHIP    (-3)   /* HIP runtime error                                 */
#define MVSIM_EFFT    (-4)   /* rocFFT error                                      */
#define MVSIM_ERCCL   (-5)   /* RCCL error                                        */
#define MVSIM_ENODEV  (-6)   /* no usable GPU                                     */

typedef struct mvsim_ctx mvsim_ctx;

/* ---- library / context ------------------------------------------------------------ */
const char* mvsim_version(void);
const char* mvsim_last_error(void);
int  mvsim_device_count(int* count);
int  mvsim_create(int device, mvsim_ctx** ctx);
int  mvsim_destroy(mvsim_ctx* ctx);
/* Use a caller-owned hipStream_t (e.g. the host framework's current stream); NULL restores
 * the context's own stream. */
int  mvsim_set_stream(mvsim_ctx* ctx, void* hip_stream);
int  mvsim_synchronize(mvsim_ctx* ctx);
/* Orders everything the context still has in flight on its internal streams (the extract + Poisson tail of the last
 * device view, option "tail_overlap") in front of whatever is enqueued on its stream next; no host synchronisation.  Every
 * entry point does this first, so only a caller that set its OWN stream (mvsim_set_stream), opted in with
 * tail_overlap = any, and enqueues work of its own on that stream needs to call it. */
int  mvsim_join(mvsim_ctx* ctx);
/* Run-time switches of a context (tests and experiments; production needs none).  Defaults come from the environment
 * variables of the same meaning, read once per process: "fft_zpass" = auto|direct|fft (MVSIM_FFT_ZPASS),
 * "fft_backend" = custom|rocfft (MVSIM_FFT_BACKEND), "fft_pad" = "px,py,pz"|auto (MVSIM_FFT_PAD), "fused_rotate" = auto|1|0|2
 * (MVSIM_NO_FUSED_ROTATE; auto = fused from 131072 columns up, separate kernels for small views; 2 = the variant that
 * recomputes the row geometry in every lane), "poisson_queue" = 1|0 (MVSIM_POISSON_NOQUEUE), "early_sum" = 1|0 (MVSIM_NO_EARLY_SUM),
 * "graph" = 0|1 (MVSIM_GRAPH), "broadcast" = scatter_allgather|ring|peer_copy|pipelined (MVSIM_BROADCAST), "psf_overlap" = 1|0 (the PSF's spectrum on a side
 * stream of the context, concurrent with the image passes A and B), "tail_overlap" = 1|0|any (extract + Poisson of a device
 * view concurrent with the next view's rotate+attenuate; 1 = only on the context's own stream, see mvsim_join; both
 * overlaps are on by default -- results are bit-identical to the serial order -- and are switched off for profiles whose
 * per-kernel durations must add up to the stage times), "fuse_tail" = 0|1 (adjust +
 * extract + Poisson phase 1 in the epilogue of the convolution's last pass), "fused_fftx" = auto|1|0|roles (per-view pipeline: rotate + attenuate + the x transform of
 * the FFT convolution as one kernel, so that the attenuated volume crosses HBM only when requested; auto = from 131072
 * columns up, its waves split into walkers and transformers for rows of up to 512 voxels; roles = that kernel whenever
 * the geometry allows; 1 = the kernel whose waves all walk and transform), "attenuate" = serial|scan (mvsim_attenuate3d
 * as a wavefront-level prefix scan along the illumination axis: parallel in y, not bit-identical to the serial walk), "beads_pair_cap" =
 * 1024..2^31 ((brick, bead) pairs the bead renderer bins at once; larger calls run in chunks with identical results; the refraction
 * simulator's injection bins its (brick, step) pairs under the same cap, and so does the sphere raster of the procedural phantom),
 * "reject_batch" = 1..2^20|auto (trials per launch of mvsim_rejection_sample; the result does not depend on it),
 * "sphere_walk" = host|device|device_only|auto (mvsim_draw_spheres, mvsim_multi_spheres: see mvsim_multi_spheres; the result does not depend on it),
 * "dog_pass" = both|xy|z (mvsim_dog_dev: launch only the xy kernel or only the z kernel, for timing a kernel alone; anything but
 * `both` leaves no valid D).
 * MVSIM_OPTIONS="name=value;name=value" sets any of them process-wide.  Unknown names or values: MVSIM_EINVAL. */
int  mvsim_set_option(mvsim_ctx* ctx, const char* name, const char* value);
/* Release cached FFT plans / workspaces / PSF spectra held by the context. */
int  mvsim_release_caches(mvsim_ctx* ctx);

/* ---- device memory (for hosts that keep volumes resident between calls) ------------- */
int  mvsim_dev_alloc(mvsim_ctx* ctx, size_t bytes, void** dptr);
int  mvsim_dev_free(mvsim_ctx* ctx, void* dptr);
int  mvsim_upload(mvsim_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  mvsim_download(mvsim_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* Page-locked host memory for the host-buffer entry points: transfers from/to such blocks run at PCIe speed (the
 * JNI shim hands them to Java as direct ByteBuffers).  Ordinary pageable buffers work everywhere too, just slower. */
int  mvsim_host_alloc(mvsim_ctx* ctx, size_t bytes, void** hptr);
int  mvsim_host_free(mvsim_ctx* ctx_or_null, void* hptr);
/* Host-to-host copy on the library's host threads (option "host_threads"; ctx may be NULL): what the JNI shim uses between a Java heap
 * array held with GetPrimitiveArrayCritical and a page-locked staging block -- the copies of the facade's Buffers.toBlock / toImg
 * (SimulateMultiViewDataset.java:109,198: every operator returns a NEW ArrayImg).  Synchronous; overlapping ranges are moved in order. */
int  mvsim_host_copy(mvsim_ctx* ctx_or_null, void* dst, const void* src, size_t bytes);
/* byte-wise fill, asynchronous on the context stream (e.g. the zero canvas of the phantom generator) */
int  mvsim_dev_memset(mvsim_ctx* ctx, void* dptr, int value, size_t bytes);

/* ---- pure host helpers --------------------------------------------------------------- */
/* SMVD:80-102 axisRotation(Interval,int axis,int degrees): forward model T(+c) R T(-c) as a
 * row-major 3x4 matrix (mpicbg AffineModel3D layout m00..m23).  Zero-min interval assumed. */
int     mvsim_axis_rotation(const int64_t dim[3], int axis, int degrees, double m[12]);
/* (Nz-1)/inc+1, SMVD:197 */
int64_t mvsim_extract_nz(int64_t nz, int inc);
/* (Nz_acq-1)*inc+1, SMVD:146 */
int64_t mvsim_isotropic_nz(int64_t nz_acq, int inc);
/* (SNR/sqrt(5))^2, Tools:76 */
double  mvsim_poisson_mul(double snr);

/* ---- stage operators, host buffers ----------------------------------------------------- */
/* SMVD:104-135 rotateAroundAxis: out[l] = trilinear(in zero-extended, M^-1 l). */
int mvsim_rotate_around_axis(mvsim_ctx* ctx, const float* in, const int64_t dim[3],
                             int axis, int degrees, float* out);
/* SMVD:318-364 attenuate3d: light enters at y = Ny-1; Nx > Ny is rejected (the reference
 * walks dimension(0) steps along y and leaves the interval). */
int mvsim_attenuate3d(mvsim_ctx* ctx, const float* in, const int64_t dim[3], double delta, float* out);
/* Tools:112-118 normImage: img <- (float)(img / sum), in place. */
int mvsim_norm_image(mvsim_ctx* ctx, float* img, int64_t n);
/* SMVD:253-264 convolve(img, psf, service): normalises psf IN PLACE (sum -> 1), then exact
 * linear convolution with mirror-single image boundary, kernel centre kdim/2, no flip.
 * method: 0 = auto (the stencil up to 4 x 4 x 4 taps, where it is measured faster; the FFT passes beyond), 1 = FFT,
 * 2 = direct LDS-tiled stencil (any PSF up to 64 taps per axis; 2 Kx Ky Kz flop per voxel). */
int mvsim_convolve(mvsim_ctx* ctx, const float* img, const int64_t dim[3],
                   float* psf, const int64_t kdim[3], int method, float* out);
/* Tools:143-159 adjustImage: in place; *correction = (target - min) / mean. */
int mvsim_adjust_image(mvsim_ctx* ctx, float* img, int64_t n, float min_value, float target_average,
                       double* correction);
/* SMVD:181-231 extractSlices(img, inc, poissonSNR, rnd): out has mvsim_extract_nz(Nz,inc)
 * planes.  snr < 0 => bit-exact strided copy.  Otherwise per-voxel Poisson(lambda = v * mul)
 * from the counter-based generator keyed by (seed, stream) with counter = source voxel index;
 * the Java facade takes seed = rnd.nextLong(). */
int mvsim_extract_slices(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float snr,
                         uint64_t seed, uint32_t stream, float* out);
/* Tools:73-86 poissonProcess(img, SNR, rnd): in place over n values; counter = index_offset+i. */
int mvsim_poisson_process(mvsim_ctx* ctx, float* img, int64_t n, double snr,
                          uint64_t seed, uint32_t stream, uint64_t index_offset);
/* SMVD:144-171 makeIsotropic: out has mvsim_isotropic_nz(Nz,inc) planes. */
int mvsim_make_isotropic(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float* out);
/* SMVD:280-316 computeWeightImage (the reference ignores its delta argument). */
int mvsim_compute_weight_image(mvsim_ctx* ctx, const int64_t dim[3], float* out);
/* SMVD:436-522 drawSpheres(img, minValue, maxValue, scale, halfPixelOffset, rnd), in place.  rnd_state is the
 * 48-bit state of the caller's java.util.Random ((seed ^ 0x5DEECE66D) & (2^48-1) right after `new Random(seed)`);
 * it is advanced exactly as the reference advances it.  The walk over the large sphere (one shared sequential
 * random stream) runs on the host, the max-compositing of the small spheres on the GPU.  n_spheres may be NULL. */
int mvsim_draw_spheres(mvsim_ctx* ctx, float* img, const int64_t dim[3], double min_value, double max_value,
                       int scale, int half_pixel_offset, uint64_t* rnd_state, int64_t* n_spheres);
/* The GPU half of drawSpheres for hosts that walk the large sphere THEMSELVES with the caller's java.util.Random (any
 * subclass, SimulateTileStitching.java:93,108 passes `new Random(seed)`): max-composite n small spheres -- ImgLib2
 * HyperSphere geometry, nested truncated radii -- into img, in place.  A sphere that leaves the image is rejected
 * (the reference throws there). */
typedef struct mvsim_sphere {
    int32_t cx, cy, cz;       /* centre                                   */
    int32_t radius;           /* rnd.nextInt(10*scale) + 1 (SMVD:468)     */
    float   value;            /* (float) intensity, Math.max-composited   */
} mvsim_sphere;
int mvsim_splat_spheres(mvsim_ctx* ctx, float* img, const int64_t dim[3], const mvsim_sphere* spheres, int64_t n);
int mvsim_splat_spheres_dev(mvsim_ctx* ctx, float* img_dev, const int64_t dim[3], const mvsim_sphere* spheres_host, int64_t n);
/* SMVD:394-424 downSample2x: out has dim[d]/2 - 1 samples per dimension. */
int mvsim_downsample2x(mvsim_ctx* ctx, const float* in, const int64_t dim[3], float* out);

/* ---- bead images: net.preibisch.simulation.SimulateBeads / SimulateBeads2 -------------------------------------------------
 *   SB  = src/main/java/net/preibisch/simulation/SimulateBeads.java
 * SB:151-166 randomPoints(numPoints, range, rnd): for each point, d = 0, 1, 2: rnd.nextDouble() * (max[d] - min[d]) + min[d]
 * (the difference of two longs, as a double).  rnd_state is the 48-bit state of the caller's java.util.Random, advanced
 * exactly as the reference advances it (both bead classes seed `new Random(535)`).  xyz receives n * 3 doubles, x first. */
int mvsim_beads_random_points(uint64_t* rnd_state, int64_t n, const int64_t min[3], const int64_t max[3], double* xyz);
/* SB:97-118 renderPoints + SB:168-205 addGaussian for nviews views in one call.  The image of every view has
 * dim[d] = max[d] - min[d] voxels (one less than the interval, as the reference allocates it; x fastest).
 *   view_offsets == NULL: every view renders the same n points; else view v renders points [view_offsets[v], view_offsets[v+1]).
 *   m12 == NULL: the points as given (renderPoints of lists that are already transformed); else nviews row-major 3x4 matrices
 *   applied first in fp64, ((x m00 + y m01) + z m02) + m03 per row (AffineModel3D / AffineTransform3D.apply).
 * Then isInsideAdjust (SB:120-130: p[d] -= min[d], kept iff 0 <= p[d] <= dim[d]) and, per kept bead IN LIST ORDER, every voxel of
 * its box (getSuggestedKernelDiameter(sigma) * 2 voxels per axis around (int)Math.round(p), clipped to the image) becomes
 * voxel + (float)(prod_d exp(-(x_d * x_d) / (2 sigma_d sigma_d))) * 1000.0f in float: bit for bit the reference's sequential sum.
 * out_f32[v] (float) and / or out_u16[v] (LegacySimulatedBeadsImgLoader.getImage: Math.round(float), then the low 16 bits) receive the
 * images; either list may be NULL, not both.  Deliberate deviations: sigma must be finite and > 0 (the reference would produce NaN
 * or degenerate boxes), and a bead whose transformed coordinates are NaN is dropped (the reference would write NaN over its box).
 * MVSIM_EINVAL also for an image dimension < 1, inconsistent view offsets and matrices with non-finite entries.
 * Host buffers, synchronous. */
int mvsim_render_beads(mvsim_ctx* ctx, const double* xyz, const int64_t* view_offsets, int64_t n, const double* m12, int nviews,
                       const int64_t min[3], const int64_t max[3], const double sigma[3], float* const* out_f32, uint16_t* const* out_u16);
/* The same with DEVICE outputs (the point list, offsets and matrices stay host arrays): returns once the lists are on the device,
 * the kernels run asynchronously on the context stream -- the images can feed the other *_dev entry points directly. */
int mvsim_render_beads_dev(mvsim_ctx* ctx, const double* xyz, const int64_t* view_offsets, int64_t n, const double* m12, int nviews,
                           const int64_t min[3], const int64_t max[3], const double sigma[3], float* const* out_f32,
                           uint16_t* const* out_u16);
/* LegacySimulatedBeadsImgLoader.normalize (:120-136), in place over n floats: float min / max, then (v - min) / (max - min) in
 * float (a constant image gives NaN, as in the reference). */
int mvsim_beads_normalize(mvsim_ctx* ctx, float* img, int64_t n);
int mvsim_beads_normalize_dev(mvsim_ctx* ctx, float* img_dev, int64_t n);

/* ---- the procedural phantom: HypersphereCollectionRealRandomAccessible.main (:199-286) ------------------------------------
 *   PN = src/main/java/net/preibisch/simulation/PerlinNoiseRealRandomAccessible.java, HC = .../HypersphereCollectionRealRandomAccessible.java,
 *   SC = .../SimpleCalculatedRealRandomAccessible.java, PRS = .../PointRejectionSampling.java
 * Three dimensions only.  Positions are 3 doubles, x first; rasters are floats, x fastest, dim = {Nx, Ny, Nz}, the voxel l at the integer
 * position origin + l.  The arithmetic is fp64, one rounding per operation, stated in DESIGN.md section 12: the results equal a literal
 * restatement bit for bit.  The host forms take host buffers and are synchronous; the *_dev forms take DEVICE positions / rasters (the
 * tables and sphere lists stay host arrays, copied before the call returns) and run asynchronously on the context's stream.
 * MVSIM_EINVAL, without touching the GPU, for null pointers, n_vectors < 1 or > 1536 (the tables are staged in LDS), loop extents < 1 or
 * with (1 + e0)(1 + e1) e2 >= 2^31 (PN's flatIndex would overflow), a scale that is 0 or NaN, non-finite positions or centres, a negative
 * or NaN radius, non-positive dims, |origin| > 2^40. */
/* PN:56-73, the constructor: per vector three nextGaussian() (JDK polar method over StrictMath.log = fdlibm, restated), each component
 * divided by Math.sqrt(sSum); then Collections.shuffle of 0 .. n - 1.  rnd_state is the caller's java.util.Random (48 bits), advanced as
 * the reference advances it; *pending_gaussian (may be NULL: none before, dropped after) is the generator's cached second Gaussian,
 * NaN = none, in and out.  Pure host function. */
int mvsim_perlin_init(uint64_t* rnd_state, int32_t n_vectors, double* gradients, int32_t* permutation, double* pending_gaussian);
typedef struct mvsim_perlin {
    double         scales[3];
    int32_t        loop_extents[3];
    int32_t        n_vectors;
    const double*  gradients;       /* n_vectors x 3 */
    const int32_t* permutation;     /* n_vectors, each 0 .. n_vectors - 1 */
    double         threshold;       /* NaN: the raw value; else SC's lambda of HC:221-223 over PN's FloatType: (float)value > threshold ? 1 : 0 */
} mvsim_perlin;
/* PN:127-160 get() at n positions -> n doubles (the raw fp64 value, or 1 / 0 with a threshold). */
int mvsim_perlin_at(mvsim_ctx* ctx, const mvsim_perlin* field, const double* xyz, int64_t n, double* out);
int mvsim_perlin_at_dev(mvsim_ctx* ctx, const mvsim_perlin* field, const double* xyz_dev, int64_t n, double* out_dev);
/* Views.raster of the field: out[l] = (float) of the value at origin + l. */
int mvsim_perlin_raster(mvsim_ctx* ctx, const mvsim_perlin* field, const int64_t origin[3], const int64_t dim[3], float* out);
int mvsim_perlin_raster_dev(mvsim_ctx* ctx, const mvsim_perlin* field, const int64_t origin[3], const int64_t dim[3], float* out_dev);
/* HC:148-177: the value of the LOWEST-INDEX sphere with sqrt(dx dx + dy dy + dz dz) <= radius (ImgLib2's Util.distance: the squares
 * summed x, y, z in fp64), else `background`.  The reference reaches this through a KD-tree search at the largest radius. */
typedef struct mvsim_sphere_set {
    int64_t       n;
    const double* centres;          /* n x 3 */
    const double* radii;            /* n, >= 0 */
    const float*  values;           /* n */
    float         background;
} mvsim_sphere_set;
int mvsim_spheres_at(mvsim_ctx* ctx, const mvsim_sphere_set* set, const double* xyz, int64_t n, float* out);
int mvsim_spheres_at_dev(mvsim_ctx* ctx, const mvsim_sphere_set* set, const double* xyz_dev, int64_t n, float* out_dev);
/* combine = 0: out = value; combine = 1: out = Math.max(out, value), the lambda of HC:265-270 without a temporary volume.  Calls that
 * bin more (brick, sphere) pairs than the option "beads_pair_cap" run in sphere ranges with identical results. */
int mvsim_spheres_raster(mvsim_ctx* ctx, const mvsim_sphere_set* set, const int64_t origin[3], const int64_t dim[3], int combine, float* out);
int mvsim_spheres_raster_dev(mvsim_ctx* ctx, const mvsim_sphere_set* set, const int64_t origin[3], const int64_t dim[3], int combine,
                             float* out_dev);
/* PRS:37-55 sampleRealPoints: per trial pos[d] = rmin[d] + nextDouble() * (rmax[d] - rmin[d]), d = 0, 1, 2, then p = nextDouble(); the
 * trial is accepted if p < density(pos), the density being the FloatType's value as a double ((double)(float) of a raw Perlin value).
 * Every trial takes eight steps of the generator, so the trials are evaluated side by side on the GPU, "reject_batch" = 1..2^20|auto
 * (option) at a time, and the accepted ones compacted in trial order; xyz_out receives the first n_samples, *n_trials_out (may be NULL)
 * the number of trials the reference would have made, and *rnd_state advances by 8 steps per such trial.  More than max_trials trials:
 * MVSIM_EINVAL with *rnd_state untouched (the reference would loop forever on a density that is 0 everywhere). */
typedef struct mvsim_density {
    int32_t                 kind;   /* 0: perlin, 1: spheres */
    const mvsim_perlin*     perlin;
    const mvsim_sphere_set* spheres;
} mvsim_density;
int mvsim_rejection_sample(mvsim_ctx* ctx, uint64_t* rnd_state, const double rmin[3], const double rmax[3], int64_t n_samples,
                           const mvsim_density* density, int64_t max_trials, double* xyz_out, int64_t* n_trials_out);

/* ---- the refraction simulator: net.preibisch.simulation.SimulateMultiViewAberrations --------------------------------------
 *   SMVA = src/main/java/net/preibisch/simulation/SimulateMultiViewAberrations.java, HES = .../Hessian.java,
 *   RAY = .../raytracing/Raytrace.java, LS = .../raytracing/Lightsheet.java, VI = .../VolumeInjection.java
 * Volumes are floats, x fastest, dim = {Nx, Ny, Nz}, every dimension >= 2 (the mirror of Views.extendMirrorSingle needs two samples).
 * Positions and directions are 3 doubles, x first.  The host forms take host buffers and are synchronous; the *_dev forms take DEVICE
 * volumes (lists, scalars and the step list stay host memory).  NaN or infinite scalars and positions: MVSIM_EINVAL; a NaN VOXEL is not
 * looked for and poisons what samples it, as in the reference.
 * What is exact: ray starts, the sampler, the Hessian, the eigenpair, the injection of a given step list, normalize, project.  What is
 * not: everything behind acos / asin / sin / cos (refraction) and exp (Gaussian weights), which the JDK, a host libm and the device
 * library each round within about an ulp, differently.
 * Third-party semantics are restated from the published algorithms and not pinned against the jars: ImgLib2's NLinearInterpolator (an
 * fp64 position and an integer lower-corner tap; setPosition / move(distance) put the tap at floor(position), fwd / bck move both by
 * one; weights = position - tap; Gray-code tap order, (float)(v * w) per tap, float accumulation), JAMA's EigenvalueDecomposition of a
 * symmetric matrix (EISPACK tred2 + tql2, eigenvalues ascending; the QL loop is capped at 64 sweeps where JAMA has no cap). */
/* LS:41-129: a x x + b x + c through (center, thickness_center) and (center -+ length / 2, thickness_edges) by the reference's
 * normal equations and adjugate inverse.  MVSIM_EINVAL when the matrix is singular (the reference throws). */
int mvsim_lightsheet_fit(double center, double thickness_center, double length, double thickness_edges, double abc[3]);
/* HES:155-278 computeHessianMatrix3D on the INTERPOLATED image (RealRandomAccess over the mirrored volume, moved as the reference
 * moves it) at n real positions (|coordinate| < 2^30), and HES:110-147 computeLargestEigenVectorAndValue3d: the eigenvalue of largest
 * magnitude (first wins on ties) and its eigenvector with the decomposition's sign.  matrix9 (n * 9, row-major), eigvec3 (n * 3),
 * eigval (n): host arrays, each may be NULL. */
int mvsim_hessian_at(mvsim_ctx* ctx, const float* img, const int64_t dim[3], const double* xyz, int64_t n, double* matrix9,
                     double* eigvec3, double* eigval);
int mvsim_hessian_at_dev(mvsim_ctx* ctx, const float* img_dev, const int64_t dim[3], const double* xyz, int64_t n, double* matrix9,
                         double* eigvec3, double* eigval);
/* HES:69-99, the loop of largestEigenVector (its Gauss3 blur is the caller's): integer positions through the mirror;
 * eigval[Nz][Ny][Nx] = (float)eigenvalue, eigvec[3][Nz][Ny][Nx] = (float)eigenvector components. */
int mvsim_hessian_images(mvsim_ctx* ctx, const float* img, const int64_t dim[3], float* eigval, float* eigvec);
int mvsim_hessian_images_dev(mvsim_ctx* ctx, const float* img_dev, const int64_t dim[3], float* eigval_dev, float* eigvec_dev);
/* SMVA:305-319: the starts of refract3d's rays, computed on the GPU: ray i consumes draws 3i .. 3i + 2 of nextDouble() of the caller's
 * java.util.Random (48-bit state, see mvsim_draw_spheres), every ray jumping the generator ahead on its own.  x = u * (Nx - 1),
 * y = illum ? Ny - 1 : 0, z = z + u * t - t / 2 with t = Lightsheet.predict(x) (abc from mvsim_lightsheet_fit), direction
 * ((u - 0.5) / 5, illum ? -1 : 1, 0) normalised.  rnd_state is advanced by the 6 n generator steps.  Bit-exact. */
int mvsim_refract3d_ray_starts(mvsim_ctx* ctx, uint64_t* rnd_state, const int64_t dim[3], int illum, int z, const double abc[3], int64_t n,
                               double* pos3, double* dir3);
/* SMVA:137-143: the starts of projectToCamera's rays, pixel-major (x fastest), rays_per_pixel per pixel: (px + (u - 0.5),
 * py + (u - 0.5), 1), direction (0, 0, 1).  pos3 receives Nx * Ny * rays_per_pixel positions; rnd_state advances 4 steps per ray. */
int mvsim_camera_ray_starts(mvsim_ctx* ctx, uint64_t* rnd_state, const int64_t dim[3], int rays_per_pixel, double* pos3);
/* The step list of refract3d: one record per move of every ray, in ray order, then move order -- where the ray stood (before the
 * move) and the image value it carried.  The caller provides host arrays for `capacity` steps (xyz: 3 doubles each) and num_rays
 * move counts; any of the three may be NULL.  n returns the number of steps; more steps than capacity: MVSIM_EINVAL. */
typedef struct mvsim_ray_steps {
    int64_t  capacity;
    int64_t  n;
    double*  xyz;
    float*   value;
    int32_t* moves;
} mvsim_ray_steps;
/* SMVA:261-401 refract3d(imgIn, imgRi, illum, z, lsMiddle, lsEdge, ri) with num_rays rays (the reference: 200 000) drawn from
 * rnd_state (the reference: new Random(2423); advanced by 6 steps per ray).  Each ray moves while it is inside the image
 * (0 <= p <= N - 1) and has made fewer than Nz moves (maxMoves = dimension(2), kept), the light sheet is fitted over Nx
 * (Lightsheet(Nx / 2.0, ls_middle, Nx, ls_edge), kept).  Per move: valueIm = imgIn at the position; Hessian of imgRi and its largest
 * eigenpair; where |eigenvalue| > 0.01, n = (ri - 1) * imgRi + 1 sampled one ray vector behind and ahead, RAY:75-93 incidentAngle
 * (quirk kept: the normal is flipped and pi / 2 SUBTRACTED when thetaI >= pi / 2), RAY:42-59 refract, NaN (total reflection) keeps
 * the direction, then norm; addNormalizedGaussian(valueIm, position) with sigma 0.5 (a box of 5 voxels per axis); position +=
 * direction.  image and weight (both may be NULL to trace only) are OVERWRITTEN with the injection's image and weight volumes,
 * accumulated in float in list order: given the step list, bit for bit the reference's sums.  steps may be NULL. */
int mvsim_refract3d(mvsim_ctx* ctx, const float* img, const float* ri_img, const int64_t dim[3], int illum, int z, double ls_middle,
                    double ls_edge, double ri, int64_t num_rays, uint64_t* rnd_state, float* image, float* weight, mvsim_ray_steps* steps);
/* Device volumes; image_dev and weight_dev are ADDED to (zero them for the reference's result).  Synchronises. */
int mvsim_refract3d_dev(mvsim_ctx* ctx, const float* img_dev, const float* ri_img_dev, const int64_t dim[3], int illum, int z,
                        double ls_middle, double ls_edge, double ri, int64_t num_rays, uint64_t* rnd_state, float* image_dev,
                        float* weight_dev, mvsim_ray_steps* steps);
/* VI:168-197 addGaussian (normalized = 0) / addNormalizedGaussian (1: intensity / sumWeights, VI:74-92 summed on the host in the
 * constructor's cursor order) for n points IN LIST ORDER, in place: over the box Math.round(xyz_d) - size_d / 2 .. + size_d - 1
 * (size = getSuggestedKernelDiameter(sigma)), value = ((1 * ex) * ey) * ez in fp64,
 * image += (float)(value * intensity), weight += (float)value; writes outside the volume are dropped (extendZero).
 * MVSIM_EINVAL: sigma <= 0 or not finite (the reference's sigma == 0, a box of one voxel, is not offered), non-finite positions or
 * intensities. */
int mvsim_volume_inject(mvsim_ctx* ctx, float* image, float* weight, const int64_t dim[3], const double sigma[3], const double* xyz,
                        const double* intensity, int64_t n, int normalized);
int mvsim_volume_inject_dev(mvsim_ctx* ctx, float* image_dev, float* weight_dev, const int64_t dim[3], const double sigma[3],
                            const double* xyz, const double* intensity, int64_t n, int normalized);
/* VI:45-94: the box sizes, sumWeights and numPixels of a VolumeInjection with this sigma (host only). */
int mvsim_volume_inject_info(const double sigma[3], int32_t size[3], double* sum_weights, int32_t* num_pixels);
/* VI:115-135 normalize: out = weight > 1.0f ? image / weight : image over n floats. */
int mvsim_volume_normalize(mvsim_ctx* ctx, const float* image, const float* weight, int64_t n, float* out);
int mvsim_volume_normalize_dev(mvsim_ctx* ctx, const float* image_dev, const float* weight_dev, int64_t n, float* out_dev);
/* VI:199-232 project: per (x, y) the weighted mean along z over the voxels with image > 0 (fp64 sums of the float products);
 * proj[Ny][Nx]; an empty column gives NaN (0 / 0), as the reference. */
int mvsim_volume_project(mvsim_ctx* ctx, const float* image, const float* weight, const int64_t dim[3], float* proj);
int mvsim_volume_project_dev(mvsim_ctx* ctx, const float* image_dev, const float* weight_dev, const int64_t dim[3], float* proj_dev);
/* SMVA:89-254 projectToCamera(imgRi, refr, ri, currentzPlane): rays_per_pixel rays (the reference: 500; 1 .. 4096) per pixel of
 * proj[Ny][Nx], drawn from rnd_state (the reference: the class's Random(464232194); advanced 4 steps per ray), refracted through
 * imgRi as above and summing refr (interpolated) * exp(-dz^2 / (2 * 4^2)), dz = |z - current_z|, per move in fp64; the pixel is
 * (float)(sum over its rays in ray order / 10.0).  Quirks kept: rays start at z = 1, the index contrast is 1.01 whatever ri is
 * (SMVA:117, so the entry point takes no ri), maxMoves = Nz, `inside` is tested against refr (same dim here). */
int mvsim_project_to_camera(mvsim_ctx* ctx, const float* ri_img, const float* refr, const int64_t dim[3], int current_z,
                            int rays_per_pixel, uint64_t* rnd_state, float* proj);
int mvsim_project_to_camera_dev(mvsim_ctx* ctx, const float* ri_img_dev, const float* refr_dev, const int64_t dim[3], int current_z,
                                int rays_per_pixel, uint64_t* rnd_state, float* proj_dev);
/* ---- the ray sandbox: net.preibisch.simulation.raytracing.RayTracingTest, and the general tracer under it -------------------
 *   RTT = .../raytracing/RayTracingTest.java; RAY, HES, VI, SMVA as above.
 * refract3d and projectToCamera launch the two ray families the reference hard-codes; mvsim_trace_rays launches the CALLER's rays
 * through the same move.  What is exact and what is not is as above: starts, the wedge, the Hessian plane and the injection of a
 * given step list are bit-exact; a ray's path is exact until its first refraction and within the libm's ulp afterwards.  On one
 * device, mvsim_trace_rays given refract3d's starts, the map (1, ri), max_moves = Nz and the image as value source returns
 * refract3d's step list, image and weight bit for bit. */
#define MVSIM_TRACE_KEEP    0   /* total reflection: the ray keeps its direction (every loop of the reference) */
#define MVSIM_TRACE_REFLECT 1   /* ... or takes RAY:32-40 reflect (the line RTT:164 has commented out), then norm */
typedef struct mvsim_trace_params {
    double  n_a, n_b;          /* the linear index map n = (n_b - n_a) * sample + n_a: (1, ri) is refract3d, (0, 1) a raw index image */
    double  ev_threshold;      /* a move refracts where |largest eigenvalue| > ev_threshold (0.01 in every reference loop); >= 0 */
    int64_t max_moves;         /* 1 .. 2^20 moves per ray: always finite, so no ray can spin */
    int32_t total_reflection;  /* MVSIM_TRACE_KEEP / MVSIM_TRACE_REFLECT */
    int32_t normalize_dirs;    /* != 0: RAY:66-73 norm applied once to every direction (a zero direction: MVSIM_EINVAL); 0: as given */
    double  constant_value;    /* the value a ray carries when there is neither an image volume nor an intensity list, as a float */
    double  sigma[3];          /* the injected Gaussians (VI): > 0 */
    int32_t normalized;        /* != 0: addNormalizedGaussian (value / sumWeights), 0: addGaussian */
} mvsim_trace_params;
/* The sandbox's settings: (0, 1), 0.01, max_moves = 4 * (Nx + Ny + Nz) (the reference's loops have no cap), keep, directions as
 * given, constant 1.0, sigma 0.5, normalized. */
int mvsim_trace_params_default(const int64_t dim[3], mvsim_trace_params* params);
/* n rays, ray r from pos3[r] along dir3[r] (host lists; |coordinate| < 2^30).  A ray moves while it is inside (0 <= p <= N - 1) and
 * has made fewer than max_moves moves.  Per move: the value it carries is the interpolated sample of img (may be NULL), else
 * intensity[r] (floats, may be NULL), else constant_value -- a float, like the step list's values; Hessian of ri_img and its largest
 * eigenpair; where |eigenvalue| > ev_threshold the refraction of refract3d with the map above and the total-reflection policy; the
 * step record; position += direction.  Outputs, each may be NULL (image and weight go together): image and weight, OVERWRITTEN with
 * the injection of the step list in list order (sigma, normalized); steps (moves: n counts); end_pos3 and end_dir3 (n * 3: where
 * each ray stood when it stopped, outside or at its last allowed move, and the direction it had); n_capped: the rays still inside
 * after max_moves moves.  Rays run in ranges of at most 2^25 step records (option "beads_pair_cap" / 8 lowers it): same bits.
 * MVSIM_EINVAL: non-finite scalars, positions, directions or intensities, max_moves outside 1 .. 2^20, ev_threshold < 0, sigma <= 0,
 * a dimension below 2, a null index volume, a step list that needs more than its capacity. */
int mvsim_trace_rays(mvsim_ctx* ctx, const float* ri_img, const float* img, const int64_t dim[3], const double* pos3, const double* dir3,
                     const float* intensity, int64_t n, const mvsim_trace_params* params, float* image, float* weight,
                     mvsim_ray_steps* steps, double* end_pos3, double* end_dir3, int64_t* n_capped);
/* Device volumes; image_dev and weight_dev are ADDED to (zero them for the sandbox's result).  Synchronises. */
int mvsim_trace_rays_dev(mvsim_ctx* ctx, const float* ri_img_dev, const float* img_dev, const int64_t dim[3], const double* pos3,
                         const double* dir3, const float* intensity, int64_t n, const mvsim_trace_params* params, float* image_dev,
                         float* weight_dev, mvsim_ray_steps* steps, double* end_pos3, double* end_dir3, int64_t* n_capped);
/* RTT:110-123 drawMultipleRays' bundle, computed on the GPU: ray i consumes draws 2i, 2i + 1 of nextDouble() of the caller's
 * java.util.Random (the reference: new Random(234345)): (x + u - 0.5, Ny - 1, z + u - 0.5), direction (0, -1, 0).  rnd_state is
 * advanced by the 4 n generator steps.  Bit-exact. */
int mvsim_sandbox_ray_starts(mvsim_ctx* ctx, uint64_t* rnd_state, const int64_t dim[3], int x, int z, int64_t n, double* pos3,
                             double* dir3);
/* RTT:334-344 drawRays' grid: x = spacing, 2 spacing, .. <= Nx from (x, Ny - 25, z), direction (0, -1, 0).  Returns the number of
 * rays, Nx / spacing, in *n_out; pos3 and dir3 hold `capacity` rays (MVSIM_EINVAL when that is too few; both may be NULL with
 * capacity 0 to ask for the count).  Quirks kept: x = Nx is a ray that is not inside and makes no move; Ny < 25 gives rays that
 * make no move (Ny = 25 starts at y = 0: one move).  spacing >= 1. */
int mvsim_grid_ray_starts(mvsim_ctx* ctx, const int64_t dim[3], int z, int spacing, int64_t capacity, double* pos3, double* dir3,
                          int64_t* n_out);
/* RAY:96-128 drawSimpleImage, the wedge: out = high where (x < Nx / 2 ? x > y : Nx - x > y) (integer division), low elsewhere,
 * for every z.  Bit-exact. */
int mvsim_draw_simple_image(mvsim_ctx* ctx, float* out, const int64_t dim[3], float low, float high);
int mvsim_draw_simple_image_dev(mvsim_ctx* ctx, float* out_dev, const int64_t dim[3], float low, float high);
/* RTT:55-84 hessian(img, z): plane z (0 <= z < Nz) of mvsim_hessian_images alone -- eigval[Ny][Nx], eigvec[3][Ny][Nx] (may be
 * NULL) -- at the cost of one plane.  (The reference returns a copy of img with that plane replaced by eigval.) */
int mvsim_hessian_plane(mvsim_ctx* ctx, const float* img, const int64_t dim[3], int z, float* eigval, float* eigvec);
int mvsim_hessian_plane_dev(mvsim_ctx* ctx, const float* img_dev, const int64_t dim[3], int z, float* eigval_dev, float* eigvec_dev);

/* The simulator's phantom, SMVA:408-440 simulate(rnd, dir): everything behind its Tools.open(dir + "block4.tif") -- a file the reference
 * does not ship; the caller supplies that canvas of refractive indices.
 * SMVA:425-426: voxel i of ri (x fastest, n voxels, n == 0 is legal) becomes (float)Math.max(0, ri[i] + (nextDouble() - 0.5) / 10), in
 * place; voxel i takes draw i of the caller's java.util.Random (see mvsim_draw_spheres), every lane jumping the generator ahead on its
 * own; rnd_state is advanced by the 2 n generator steps.  Bit-exact. */
int mvsim_ri_noise(mvsim_ctx* ctx, float* ri, int64_t n, uint64_t* rnd_state);
int mvsim_ri_noise_dev(mvsim_ctx* ctx, float* ri_dev, int64_t n, uint64_t* rnd_state);
/* SMVA:474-586 multiSpheres(image, ri, scale, rnd), in place on two volumes of the same dimensions, with the ranges the reference
 * hard-codes: {0.5, 1.0} for the image, {1.0, 1.1} for the index volume (its min == max branches never run and are not offered).  The walk
 * is drawSpheres' with a large sphere of radius min(dim) / 2 - 47 scale - 1 about dim / 2, radius = Math.max(nextInt(10 scale) + 1,
 * 10 scale - 1), and one voxel in 100 000 drawn (rv * 100000 < 1).  image: Math.max(value, existing).  ri: a covered voxel that holds
 * exactly 5.0 takes the sphere's value, any other the maximum -- built as two passes in place: every covered voxel equal to 5.0 is set
 * to -infinity, then all spheres are max-composited (the outcome does not depend on the order of the spheres: after the first
 * replacement a voxel holds at most 1.1).  Caveat: a call that fails between the two passes (a HIP error) leaves -infinity in those
 * voxels.  MVSIM_EINVAL, nothing written and rnd_state untouched: the large sphere's radius is negative, or a small sphere leaves the
 * volume (the reference throws there).  n_spheres may be NULL.  Option "sphere_walk" = host|device|device_only|auto: who walks the sequential random
 * stream over the voxels of the large sphere -- the host, one voxel after the other, or the GPU (csrc/sphere_walk.h: the stream cut in chunks, the
 * orbit of voxel starts resolved per chunk and stitched by a scan; the host walk takes over in the cases the device walk does not vouch
 * for; device_only: MVSIM_EINVAL in those cases, for tests).  Same bits either way.  auto (the default): mvsim_draw_spheres on the host, mvsim_multi_spheres on the device. */
int mvsim_multi_spheres(mvsim_ctx* ctx, float* img, float* ri, const int64_t dim[3], int scale, uint64_t* rnd_state, int64_t* n_spheres);
int mvsim_multi_spheres_dev(mvsim_ctx* ctx, float* img_dev, float* ri_dev, const int64_t dim[3], int scale, uint64_t* rnd_state,
                            int64_t* n_spheres);
/* Host only: stream positions per chunk of the device walk and the number of entry offsets resolved per chunk (tests aim at chunk
 * boundaries with these). */
int mvsim_sphere_walk_geometry(int64_t* chunk_positions, int* max_entry);

/* ---- stage operators, device-resident buffers (asynchronous on the context stream) ------ */
/* (mvsim_draw_spheres_dev returns after the host walk; the compositing kernels are asynchronous.) */
int mvsim_draw_spheres_dev(mvsim_ctx* ctx, float* img, const int64_t dim[3], double min_value, double max_value,
                           int scale, int half_pixel_offset, uint64_t* rnd_state, int64_t* n_spheres);
int mvsim_downsample2x_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], float* out);
int mvsim_rotate_around_axis_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3],
                                 int axis, int degrees, float* out);
int mvsim_attenuate3d_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], double delta, float* out);
/* psf_host is normalised in place on the host (it is <= ~1 MB), then uploaded. */
int mvsim_convolve_dev(mvsim_ctx* ctx, const float* img, const int64_t dim[3],
                       float* psf_host, const int64_t kdim[3], int method, float* out);
/* Synchronises (the correction is returned to the host). */
int mvsim_adjust_image_dev(mvsim_ctx* ctx, float* img, int64_t n, float min_value, float target_average,
                           double* correction);
int mvsim_extract_slices_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float snr,
                             uint64_t seed, uint32_t stream, float* out);
int mvsim_make_isotropic_dev(mvsim_ctx* ctx, const float* in, const int64_t dim[3], int inc, float* out);
int mvsim_compute_weight_image_dev(mvsim_ctx* ctx, const int64_t dim[3], float* out);

/* ---- cross-view weight normalisation (after the view loop, SMVD:615-640 and :648-661) ------------------ */
#define MVSIM_MAX_VIEWS 32
/* out[i] = sum over views (float accumulation in view order, starting from 0), SMVD:625-628 / :648-661.
 * vols: HOST array of n_views DEVICE pointers. */
int mvsim_sum_views_dev(mvsim_ctx* ctx, const float* const* vols, int n_views, int64_t n, float* out);
/* In place on every view: sum == 0 -> 0, else min(1, osem * (w / sum)) in float (SMVD:630-639).
 * sum_or_null: per-voxel sum over ALL views (e.g. after mvsim_comm_allreduce_sum when views are sharded over
 * ranks); NULL => summed here over the given views. */
int mvsim_normalize_weights_dev(mvsim_ctx* ctx, float* const* weights, int n_views, int64_t n,
                                const float* sum_or_null, float osem);
/* Host buffers: weights[v] are host pointers of n floats each. */
int mvsim_normalize_weights(mvsim_ctx* ctx, float* const* weights, int n_views, int64_t n, float osem);

/* ---- multi-view deconvolution: the consumer of the simulated dataset ------------------------------------------------------
 * Weighted, sequential (OSEM) multi-view Richardson-Lucy over V views phi_v of one size, optional weights w_v of that size, one
 * PSF P_v per view (each with its own kdim) and an estimate psi.  The reference has no deconvolution; the recipe is this one.
 * With conv(a, P)[i] = sum_k P[k] a_mirror[i - (k - K/2)] the convolution of mvsim_convolve (mirror-single extension, centre K/2,
 * no flip), for iteration = 0 .. T-1 and v = 0 .. V-1 in the order given, psi updated after every view:
 *     b = conv(psi, P_v)
 *     r = phi_v / fmaxf(b, eps)                 one IEEE float division; a NaN b takes eps
 *     c = conv(r, F_v)                          F_v: mvsim_decon_flip_psf(P_v), so that c[i] = sum_k P_v[k] r_mirror[i + (k - K/2)]
 *     n = psi * c                               float
 *     lambda > 0:  n = (float)((sqrt(1.0 + 2.0 * lambda * (double)n) - 1.0) / lambda)        in double
 *     n NaN or n < min_value:  n = min_value
 *     psi = n    without weights,    psi = psi + w_v * (n - psi)    with them (float subtract, multiply, add)
 * Every step is rounded on its own.  The elementwise steps are exact (bit for bit the float32 arithmetic above); the convolutions
 * carry the error of mvsim_convolve (<= 1e-5 of range each).
 * UNLIKE mvsim_convolve, the caller's PSF arrays are NOT written: every PSF is copied and the copy normalised (Tools.normImage).
 * Start value: params.init_from_psi = 1: what psi holds on entry; else init_value > 0: that constant; else the mean over views of
 * each view's mean (fp64 sums), rounded to float; constant and mean are floored at min_value.
 * Device memory beyond the caller's buffers: two volumes of the views' size plus the 2 V prepared PSFs (and what the convolution
 * itself keeps), all context workspaces that mvsim_release_caches frees. */
typedef struct mvsim_decon_params {
    int32_t iterations;      /* >= 1 */
    int32_t method;          /* as mvsim_convolve: 0 auto, 1 FFT, 2 stencil (a flipped PSF of an even 64 has 65 taps: EINVAL) */
    int32_t init_from_psi;   /* 0 | 1 */
    float   init_value;      /* > 0: constant start; <= 0: mean of the views */
    float   min_value;       /* default 1e-4f */
    float   eps;             /* default 1e-6f */
    double  lambda;          /* Tikhonov; default 0 = off */
} mvsim_decon_params;
typedef struct mvsim_decon_stat {
    double  sum_psi;         /* fp64 sum of the new estimate */
    float   max_change;      /* max |psi_new - psi_old| (float subtraction; NaN differences are skipped) */
    int64_t n_floored;       /* voxels whose n was NaN or below min_value */
} mvsim_decon_stat;
void mvsim_decon_params_default(mvsim_decon_params* p);
/* Host only.  out[j] = psf[K-1-j] per axis; an axis of EVEN extent gets one leading zero tap (extent K+1), which puts the centre
 * (K+1)/2 where the correlation needs it.  out holds prod(kdim[d] | 1) floats; out_kdim[d] = kdim[d] | 1. */
int mvsim_decon_flip_psf(const float* psf, const int64_t kdim[3], float* out, int64_t out_kdim[3]);
/* Host only: {most blocks an elementwise kernel launches, voxels a block takes per trip of its grid-stride loop}. */
int mvsim_decon_geometry(int64_t out[2]);
/* The two elementwise steps on device buffers of n floats, any alignment.  ratio may be `blurred` (in place). */
int mvsim_decon_ratio_dev(mvsim_ctx* ctx, const float* phi, const float* blurred, int64_t n, float eps, float* ratio);
/* In place on psi; weight_or_null: device.  stat_host_or_null non-null: the statistics of the step, and the call synchronises.
 * The three values repeat bit for bit from run to run (per-block partials, one fixed-order final reduction, no atomics). */
int mvsim_decon_update_dev(mvsim_ctx* ctx, float* psi, const float* corr, const float* weight_or_null, int64_t n,
                           float min_value, double lambda, mvsim_decon_stat* stat_host_or_null);
/* views_dev, weights_dev_or_null: HOST arrays of n_views DEVICE pointers (weights: all or none); psf_host: HOST arrays of HOST
 * PSFs, kdims: 3 extents per view.  psi_dev must not overlap a view or a weight.  Asynchronous on the context's stream unless
 * stats_or_null is given: iterations * n_views entries, [iteration][view], fetched in ONE download at the end.
 * MVSIM_EINVAL: n_views outside [1, MVSIM_MAX_VIEWS], iterations < 1, a null or mismatched argument, psi aliasing a view or a
 * weight, method outside 0..2, eps <= 0, min_value <= 0, lambda < 0 (NaN included). */
int mvsim_deconvolve_dev(mvsim_ctx* ctx, const float* const* views_dev, const float* const* weights_dev_or_null,
                         const float* const* psf_host, const int64_t* kdims, int n_views, const int64_t dim[3],
                         const mvsim_decon_params* params, float* psi_dev, mvsim_decon_stat* stats_or_null);
/* The same with HOST buffers for views, weights and psi (read only with init_from_psi, always written); synchronous. */
int mvsim_deconvolve(mvsim_ctx* ctx, const float* const* views, const float* const* weights_or_null,
                     const float* const* psf_host, const int64_t* kdims, int n_views, const int64_t dim[3],
                     const mvsim_decon_params* params, float* psi, mvsim_decon_stat* stats_or_null);

/* ---- bead detection: difference-of-Gaussian interest points, sub-voxel localised ------------------------------------------------
 * The consumer of mvsim_render_beads: a DoG volume over a device-resident image, its strict local maxima above a threshold in a
 * deterministic order, and a quadratic sub-voxel fit of every maximum.  The reference has no detector; the recipe is this one, and
 * every arithmetic step is stated so that a literal restatement reproduces the result bit for bit.
 * Volumes are x fastest with dim = {Nx, Ny, Nz}.  The source is float, or uint16_t converted with one (float)v on load.
 * 1. Taps (host, fp64, handed to the kernels as floats).  For a sigma s > 0 the diameter is d = max(3, 2 (int)(3 s + 0.5) + 1) and
 *    r = d / 2;  e[j] = exp(-((j - r) (j - r)) / (2 s s)) for j = 0 .. d-1 with libm exp;  S = e[0] + e[1] + ... in ascending order;
 *    t[j] = (float)(e[j] / S).  A diameter above MVSIM_DOG_MAX_TAPS (63) is MVSIM_EINVAL.
 * 2. Blur: separable, x then y then z, one float result per pass and voxel: acc = t[0] v_0, then acc = acc + t[j] v_j for j
 *    ascending; each product and each sum is its own float operation (no fused multiply-add, the symmetric taps are not folded,
 *    nothing is reordered).  v_j is the sample at index i + j - r through the mirror-single extension of mvsim_convolve: period
 *    2 N - 2, folded as often as needed (m = (i + j - r) mod (2 N - 2), taken non-negative; m >= N reads 2 N - 2 - m), so any
 *    N >= 2 with any legal radius is defined.  Every extent must be >= 2.
 * 3. D = G1 - G2, one float subtraction; G1 is the blur with sigma1[3], G2 the blur with sigma2[3], each per axis (x, y, z).
 *    Bright blobs are maxima of D.
 * 4. Peaks.  A voxel is a peak when it is interior (1 <= x <= Nx-2, likewise y and z; a volume with an extent below 3 has none, no
 *    error), D > threshold, D > each of the 13 neighbours of its 3x3x3 box with a smaller linear index and D >= each of the 13 with
 *    a larger one -- float comparisons, so a NaN at the voxel or at any neighbour yields no peak and a plateau of equal voxels
 *    yields at most one.  The list holds the peaks' linear indices x + Nx (y + Ny z) in ascending order; n_found is the total, and
 *    only the first min(n_found, capacity) entries are written.
 * 5. Localisation: one fp64 computation per listed peak from the float values of D, no fused operations.  At base voxel b, with
 *    p_d = (double)D(b + e_d), m_d = (double)D(b - e_d), c = (double)D(b):
 *        g_d  = (p_d - m_d) / 2.0
 *        H_dd = (p_d - 2.0 * c) + m_d
 *        H_df = (((D(b+e_d+e_f) - D(b-e_d+e_f)) - D(b+e_d-e_f)) + D(b-e_d-e_f)) / 4.0            (each D widened to double first)
 *    With m00 = H_xx, m01 = m10 = H_xy, m02 = m20 = H_xz, m11 = H_yy, m12 = m21 = H_yz, m22 = H_zz, every product chain and every sum
 *    evaluated left to right:
 *        det  = m00*m11*m22 + m01*m12*m20 + m02*m10*m21 - m02*m11*m20 - m00*m12*m21 - m01*m10*m22
 *        idet = 1.0 / det
 *        i00 = (m11*m22 - m12*m21) * idet    i01 = (m02*m21 - m01*m22) * idet    i02 = (m01*m12 - m02*m11) * idet
 *        i10 = (m12*m20 - m10*m22) * idet    i11 = (m00*m22 - m02*m20) * idet    i12 = (m02*m10 - m00*m12) * idet
 *        i20 = (m10*m21 - m11*m20) * idet    i21 = (m01*m20 - m00*m21) * idet    i22 = (m00*m11 - m01*m10) * idet
 *        o_d = -((i_d0 * g_x + i_d1 * g_y) + i_d2 * g_z)
 *    det zero or non-finite, or a non-finite o_d: o = 0 and flag SINGULAR.
 *    Moves: an axis with |o_d| > 0.5 wants to move its base one voxel in the direction of o_d.  The move is refused if it would
 *    leave the interior, and refused with flag FROZEN if the axis has already moved in the opposite direction (the axis keeps its
 *    base and its offset as computed; without this rule a bead centred within ~0.005 of a half voxel oscillates between two bases
 *    and ends a voxel off).  If no move remains the fit is accepted; if moves remain but max_moves rounds are used up it is accepted
 *    with flag CAPPED; otherwise every remaining move is applied at once (one round) and the fit is repeated at the new base.
 *    SINGULAR and FROZEN describe the accepted fit.
 *    Output: pos[d] = (double)b_d + o_d, value = (float)(c + 0.5 * ((g_x*o_x + g_y*o_y) + g_z*o_z)), flags, voxel = the final base. */
#define MVSIM_DOG_MAX_TAPS 63
#define MVSIM_SRC_F32 0
#define MVSIM_SRC_U16 1
#define MVSIM_PEAK_SINGULAR 1
#define MVSIM_PEAK_FROZEN   2
#define MVSIM_PEAK_CAPPED   4
#define MVSIM_PEAK_OUTSIDE  8     /* mvsim_localise_peaks_dev only: the listed voxel is no interior voxel; pos = its coordinates, value 0 */
typedef struct mvsim_dog_params {
    double  sigma1[3];       /* x, y, z; default 1.8 */
    double  sigma2[3];       /* default 1.8 * pow(2.0, 0.25) */
    float   threshold;       /* default 0.008f: the usual proposal for images normalised to [0, 1] (mvsim_beads_normalize) */
    int32_t max_moves;       /* default 4 */
} mvsim_dog_params;
typedef struct mvsim_peak {
    double  pos[3];          /* b + o, x first */
    float   value;
    int32_t flags;           /* MVSIM_PEAK_* */
    int64_t voxel;           /* linear index of the final base voxel */
} mvsim_peak;
void mvsim_dog_params_default(mvsim_dog_params* p);
/* Host only, no context: the taps of step 1.  taps holds MVSIM_DOG_MAX_TAPS floats; *ntaps = d. */
int mvsim_dog_taps(double sigma, float* taps, int* ntaps);
/* Host only: {x extent, y extent of the xy kernel's plane tile, z extent of the z kernel's tile, largest radius (the halo limit),
 * voxels one block of the peaks kernels takes}. */
int mvsim_dog_geometry(int64_t out[5]);
/* Steps 1-3 over a device image of src_type MVSIM_SRC_F32 / MVSIM_SRC_U16 (not written) into dog_dev (floats); any alignment of
 * either.  Only sigma1 and sigma2 of params are read.  Asynchronous on the context's stream, like every _dev call below. */
int mvsim_dog_dev(mvsim_ctx* ctx, const void* img_dev, int src_type, const int64_t dim[3], const mvsim_dog_params* params,
                  float* dog_dev);
/* Step 4 over a device float volume: voxels_dev receives min(n_found, capacity) int64 indices, *n_found_dev (one int64 in DEVICE
 * memory) the total.  No atomics: per-block counts, an exclusive scan, an ordered emit. */
int mvsim_find_peaks_dev(mvsim_ctx* ctx, const float* vol_dev, const int64_t dim[3], float threshold, int64_t capacity,
                         int64_t* voxels_dev, int64_t* n_found_dev);
/* Step 5 for the first min(*n_found_dev, capacity) entries of voxels_dev; peaks_dev entries past that are not written. */
int mvsim_localise_peaks_dev(mvsim_ctx* ctx, const float* vol_dev, const int64_t dim[3], const int64_t* voxels_dev,
                             const int64_t* n_found_dev, int64_t capacity, int max_moves, mvsim_peak* peaks_dev);
/* The whole recipe; D, the list and the half-blurred volumes live in context workspaces that mvsim_release_caches frees.
 * MVSIM_EINVAL: a null pointer, an extent below 2, a sigma <= 0 or non-finite, a diameter above 63, a NaN threshold,
 * capacity <= 0, max_moves < 0, an unknown src_type. */
int mvsim_detect_beads_dev(mvsim_ctx* ctx, const void* img_dev, int src_type, const int64_t dim[3], const mvsim_dog_params* params,
                           int64_t capacity, mvsim_peak* peaks_dev, int64_t* n_found_dev);
/* The same with HOST buffers in and out; synchronous.  peaks holds capacity entries, min(*n_found, capacity) are written. */
int mvsim_detect_beads(mvsim_ctx* ctx, const void* img, int src_type, const int64_t dim[3], const mvsim_dog_params* params,
                       int64_t capacity, mvsim_peak* peaks, int64_t* n_found);

/* ---- bead registration: geometric descriptors, ratio-test matching, RANSAC, affine fit ------------------------------------------
 * The consumer of mvsim_detect_beads: two device-resident lists of positions in two coordinate frames go in, the affine transform
 * from list A to list B comes out.  The reference has no matcher; the recipe is this one, and every arithmetic step is stated so that
 * a literal restatement reproduces the result bit for bit.  All arithmetic is fp64, every + - * / sqrt an operation of its own (no
 * fused multiply-add), sqrt correctly rounded.
 * A point list is n positions of 3 doubles (x, y, z) at a byte stride >= 24 that is a multiple of 8: 24 for a packed array, 40 for
 * the mvsim_peak records of the detector (pos comes first).  n = min(max(*n_dev, 0), capacity) is read from DEVICE memory by the
 * kernels, so detection and registration chain on one stream without a synchronisation; capacity <= MVSIM_REG_MAX_POINTS.  The
 * method is all-pairs.  The squared distance of two points is d2 = (dx*dx + dy*dy) + dz*dz.
 * 1. Neighbours.  K = 3 + redundancy.  For every point whose three coordinates are finite: the K OTHER finite points (by index; an
 *    exact duplicate at d2 = 0 is a neighbour like any other) with the smallest (d2, index), in that order.  A non-finite point is
 *    nobody's neighbour and has no neighbours.  Missing ranks are index -1 with d2 = +inf.  A point with a missing rank has no
 *    descriptors.
 * 2. Descriptors.  The S = C(K, 3) rank triples (i < j < k) in lexicographic order (mvsim_descriptor_subsets; S = 1, 4, 10).  For a
 *    point p and the neighbours a, b, c of a triple the descriptor is the 6 doubles |pa|, |pb|, |pc|, |ab|, |ac|, |bc|, each the sqrt
 *    of a d2.  Descriptor s of point i is at doubles 6 (S i + s) ...; a point without descriptors holds NaN in all of them, and a
 *    point whose FIRST double is NaN counts as having none.
 * 3. Matching A -> B.  The distance of two descriptors u, w is ((((( e0 + e1) + e2) + e3) + e4) + e5) with e_t = (u_t - w_t)*(u_t - w_t).
 *    v(a, b) is the smallest distance over the S x S descriptor pairs of a and b, NaN distances left out, +inf when none is left.
 *    b1 and b2 are the two described points of B with the smallest (v, index).  a yields the candidate (a, b1) when b2 exists and
 *    v(a, b1) * ratio2 < v(a, b2), ratio2 = ratio * ratio computed once on the host.  The candidates are listed in ascending a
 *    (count, scan, emit: no atomics); n_candidates is the total and only the first min(n_candidates, capacity) are written.
 * 4. Affine fit over an ordered selection of candidates (p -> q), candidate i holding p = A[a_i], q = B[b_i].  EVERY sum below is
 *    taken the same way: over chunks of MVSIM_REG_FIT_CHUNK (256) consecutive candidate indices, unselected candidates skipped; a
 *    chunk's sum starts from +0.0 and adds ascending, the total starts from +0.0 and adds the chunks' sums ascending.
 *        n = number selected;  cp = (sum p) / n,  cq = (sum q) / n                    (6 sums, 6 divisions by (double)n)
 *        p' = p - cp, q' = q - cq
 *        Sm = sum p' p'^T: m00 = xx, m01 = m10 = xy, m02 = m20 = xz, m11 = yy, m12 = m21 = yz, m22 = zz       (6 sums of products)
 *        C  = sum q' p'^T: c_rc = sum q'_r p'_c                                                                  (9 sums of products)
 *        det and the inverse i_rc of Sm exactly as step 5 of the detector writes them (adjugate times idet = 1.0 / det)
 *        A_rc = ((c_r0 * i_0c + c_r1 * i_1c) + c_r2 * i_2c)
 *        t_r  = cq_r - ((A_r0 * cp_x + A_r1 * cp_y) + A_r2 * cp_z)
 *    n < 4, or det zero or non-finite: no model.  The model is the 3 x 4 row-major matrix m = [A | t].
 * 5. RANSAC over M = min(n_candidates, capacity) candidates.  M < 4 sets FEW_CANDIDATES.  Hypothesis h = 0 .. hypotheses-1 owns a
 *    java.util.Random(seed + h) and draws nextInt(M) until it holds 4 distinct indices, at most 32 draws, otherwise it is void.  The 4
 *    indices sorted ascending are fitted by step 4.  A candidate is an inlier of a model when e2 <= eps2 with
 *    e_r = (((m_r0 * p_x + m_r1 * p_y) + m_r2 * p_z) + m_r3) - q_r,  e2 = (e_x*e_x + e_y*e_y) + e_z*e_z,  eps2 = max_epsilon * max_epsilon
 *    computed once on the host; a NaN e2 is no inlier, and a candidate whose a or b is no index of its list holds NaN positions.  A
 *    void or model-less hypothesis counts 0.  The best hypothesis has the highest count, ties go to the lowest h.  M < 4 or a best
 *    count below 4: NO_MODEL, m is NaN, best_hypothesis -1, no inliers, and step 6 does not run.
 * 6. Refit.  model = the best hypothesis's, mask = its inliers, refits = 0.  Repeat: if refits == max_refits set CAPPED and stop; fit
 *    the masked candidates by step 4 -- no model: set NO_MODEL, keep the model and stop; refits += 1; take the new model, recompute the
 *    mask; stop when it is the mask of the round before.  n_inliers counts the final mask -- always the inliers of the reported
 *    model --, mean_error is (sum of sqrt(e2) over the inliers, summed as in step 4) / n_inliers, max_error the largest sqrt(e2)
 *    (both NaN without inliers).  FEW_INLIERS when n_inliers < min_inliers or (double)n_inliers < min_inlier_ratio * (double)M; the
 *    matrix is reported all the same. */
#define MVSIM_REG_MAX_POINTS 65536
#define MVSIM_REG_FIT_CHUNK  256
#define MVSIM_REG_MAX_REFITS 4096   /* the refit rounds run inside one kernel: a mask that keeps alternating must end */
#define MVSIM_REG_FEW_CANDIDATES 1
#define MVSIM_REG_NO_MODEL       2
#define MVSIM_REG_CAPPED         4
#define MVSIM_REG_FEW_INLIERS    8
typedef struct mvsim_match_params {
    double  ratio;             /* default 3.0 (a convention); >= 1 */
    double  max_epsilon;       /* default 5.0 voxels; > 0 */
    double  min_inlier_ratio;  /* default 0.1 */
    int64_t seed;              /* default 0: hypothesis h draws from java.util.Random(seed + h) */
    int32_t redundancy;        /* default 1; 0 .. 2 */
    int32_t hypotheses;        /* default 10000; >= 1 */
    int32_t max_refits;        /* default 8; 0 .. MVSIM_REG_MAX_REFITS */
    int32_t min_inliers;       /* default 12; >= 4 */
} mvsim_match_params;          /* 48 bytes */
typedef struct mvsim_match {
    int32_t a, b;              /* indices into list A and list B */
    double  v_best, v_second;  /* v(a, b1), v(a, b2) */
} mvsim_match;                 /* 24 bytes */
typedef struct mvsim_registration {
    double  m[12];             /* 3 x 4 row-major, A -> B: q = m[:, :3] p + m[:, 3] */
    double  mean_error, max_error;   /* over the inliers, voxels */
    int64_t n_a, n_b;          /* points with descriptors (0 from mvsim_ransac_affine_dev, which sees no descriptors) */
    int64_t n_candidates;      /* the total, also beyond the capacity */
    int64_t n_inliers;
    int64_t best_hypothesis;   /* -1: none */
    int32_t refits, flags;     /* MVSIM_REG_* */
} mvsim_registration;          /* 160 bytes */
void mvsim_match_params_default(mvsim_match_params* p);
/* Host only, no context.  The launch geometry for lists of capacity_a and capacity_b points: out = {queries (lanes) per block of the
 * two all-pairs kernels, points per staged tile of k_knn, splits of list A's candidate range for capacity_a, tiles per split;
 * B points per staged tile of k_match, splits of list B for (capacity_a, capacity_b, redundancy), tiles per split; candidates per
 * staged tile of the RANSAC kernel}.  The split rule: with Q blocks of queries and T tiles, splits = min(T, max(1, ceil(1024 / Q))),
 * tiles per split = ceil(T / splits), and only the ceil(T / tiles per split) splits that own a tile are launched.  (d2, index) and
 * (v, index) are total orders, so every split gives the same bits. */
int mvsim_match_geometry(int64_t capacity_a, int64_t capacity_b, int redundancy, int64_t out[8]);
/* Host only: the S = C(3 + redundancy, 3) rank triples of step 2, 3 ints each; *n_subsets = S.  triples holds 30 ints. */
int mvsim_descriptor_subsets(int redundancy, int32_t* triples, int* n_subsets);
/* Host only, no context: step 4 over n pairs p[i] -> q[i] (packed, 3 doubles each) selected by mask (one byte per pair; NULL: all).
 * Returns MVSIM_OK with *has_model = 1 and m filled, or *has_model = 0 and m untouched. */
int mvsim_fit_affine(const double* p, const double* q, const unsigned char* mask_or_null, int64_t n, double m[12], int* has_model);
/* Step 1 on a device list: idx_dev receives K int32 and d2_dev K doubles per point, for the first n points (entries past them are
 * not written).  Asynchronous on the context's stream, like every _dev call below. */
int mvsim_knn_dev(mvsim_ctx* ctx, const void* pos_dev, int64_t stride, const int64_t* n_dev, int64_t capacity, int redundancy,
                  int32_t* idx_dev, double* d2_dev);
/* Step 2 from the positions and the neighbour indices of step 1: 6 S doubles per point for the first n points; *n_described_dev (one
 * int64 in DEVICE memory) the number of points with descriptors. */
int mvsim_bead_descriptors_dev(mvsim_ctx* ctx, const void* pos_dev, int64_t stride, const int64_t* n_dev, int64_t capacity, int redundancy,
                               const int32_t* idx_dev, double* desc_dev, int64_t* n_described_dev);
/* Step 3 over two descriptor arrays as step 2 leaves them: candidates_dev receives min(n_candidates, capacity) records,
 * *n_candidates_dev (one int64 in DEVICE memory) the total.  1 <= capacity <= MVSIM_REG_MAX_POINTS. */
int mvsim_match_descriptors_dev(mvsim_ctx* ctx, const double* desc_a_dev, const int64_t* n_a_dev, int64_t capacity_a,
                                const double* desc_b_dev, const int64_t* n_b_dev, int64_t capacity_b, int redundancy, double ratio,
                                int64_t capacity, mvsim_match* candidates_dev, int64_t* n_candidates_dev);
/* Steps 5 and 6 over any candidate list: result_dev receives one mvsim_registration, mask_dev_or_null one byte per candidate
 * (min(n_candidates, capacity) of them; 1 = inlier).  Of params, redundancy and ratio are checked and not used. */
int mvsim_ransac_affine_dev(mvsim_ctx* ctx, const void* pos_a_dev, int64_t stride_a, const int64_t* n_a_dev, int64_t capacity_a,
                            const void* pos_b_dev, int64_t stride_b, const int64_t* n_b_dev, int64_t capacity_b,
                            const mvsim_match* candidates_dev, const int64_t* n_candidates_dev, int64_t capacity,
                            const mvsim_match_params* params, mvsim_registration* result_dev, unsigned char* mask_dev_or_null);
/* The whole recipe; every intermediate lives in context workspaces that mvsim_release_caches frees.  The candidate list has
 * capacity_a entries (a point of A yields at most one); candidates_dev_or_null receives it (capacity_a records, n_candidates of
 * them written), mask_dev_or_null one byte per candidate.
 * MVSIM_EINVAL: a null pointer, a stride below 24 or no multiple of 8, a capacity <= 0 or above MVSIM_REG_MAX_POINTS, redundancy
 * outside 0 .. 2, ratio, max_epsilon or min_inlier_ratio not finite, ratio < 1, max_epsilon <= 0, hypotheses <= 0, max_refits < 0
 * or above MVSIM_REG_MAX_REFITS, min_inliers < 4. */
int mvsim_register_beads_dev(mvsim_ctx* ctx, const void* pos_a_dev, int64_t stride_a, const int64_t* n_a_dev, int64_t capacity_a,
                             const void* pos_b_dev, int64_t stride_b, const int64_t* n_b_dev, int64_t capacity_b,
                             const mvsim_match_params* params, mvsim_registration* result_dev, mvsim_match* candidates_dev_or_null,
                             unsigned char* mask_dev_or_null);
/* The same with HOST buffers; synchronous.  n_a, n_b >= 0 points; candidates_or_null holds max(n_a, 1) records, mask_or_null as many
 * bytes; min(result->n_candidates, n_a) of each are written. */
int mvsim_register_beads(mvsim_ctx* ctx, const void* pos_a, int64_t stride_a, int64_t n_a, const void* pos_b, int64_t stride_b, int64_t n_b,
                         const mvsim_match_params* params, mvsim_registration* result, mvsim_match* candidates_or_null,
                         unsigned char* mask_or_null);

/* ---- view fusion: affine resampling into one frame, blended average or aligned views ----------------------------------------------
 * The consumer of mvsim_register_beads: V views, each with a forward matrix view -> output frame, are resampled into a caller-chosen
 * output interval and either averaged under smooth border weights (the fused volume) or handed back one by one with their weight
 * volumes (the aligned views, which mvsim_normalize_weights_dev and mvsim_deconvolve_dev take as they are).  The reference has no
 * fusion; the recipe is this one, and every arithmetic step is stated so that a literal restatement reproduces the result bit for bit.
 * Volumes are x fastest with dim = {Nx, Ny, Nz}.  A source is float, or uint16_t widened with one (float)v on load (MVSIM_SRC_F32 /
 * MVSIM_SRC_U16; one type for all views of a call).  All arithmetic below is fp64, every + - * / an operation of its own (no fused
 * multiply-add), every product chain and every sum evaluated as parenthesised.
 * 1. Inverse.  View v has the forward matrix m = [A | t], 3 x 4 row-major (what mvsim_registration.m holds for A -> B).  With
 *    m00 .. m22 = A, det, idet = 1.0 / det and the nine i_rc = (...) * idet are exactly the formulas of step 5 of the detector, and
 *        it_r = -((i_r0 * t_x + i_r1 * t_y) + i_r2 * t_z)
 *    If any of the 12 entries is non-finite, or det is zero or non-finite, the view contributes nothing anywhere (in aligned mode its
 *    outputs are all zero) and its status word is MVSIM_FUSE_SINGULAR; otherwise the status word is 0.
 * 2. Position.  For output voxel l: o_d = (double)(out_min_d + l_d) (out_min may be negative), and
 *        p_r = ((it_r + i_r2 * o_z) + i_r1 * o_y) + i_r0 * o_x
 * 3. Inside.  View v covers the voxel when 0.0 <= p_d && p_d <= (double)(N_d - 1) for all three axes; a NaN is outside.
 * 4. Sample.  f_d = floor(p_d), u_d = p_d - f_d, lo_d = (int64)f_d, hi_d = min(lo_d + 1, N_d - 1).  The eight voxels v_abc (a, b, c in
 *    {0 = lo, 1 = hi} along x, y, z) are widened to double; along x: c_bc = v_0bc + u_x * (v_1bc - v_0bc); along y: c_c = c_0c + u_y *
 *    (c_1c - c_0c); along z: s = c_0 + u_z * (c_1 - c_0); s_f = (float)s.
 * 5. Border weight.  g_d = (double)(N_d - 1) - p_d;  e_d = p_d < g_d ? p_d : g_d;  r_d = 1.0 unless e_d < blend_d, and then
 *    q = e_d / blend_d, r_d = (q * q) * (3.0 - 2.0 * q) (a smoothstep: it restates exactly, the usual cosine does not).
 *    w = (r_x * r_y) * r_z.  blend_d = 0 gives r_d = 1 everywhere inside.
 * 6. Fused volume.  num = den = +0.0; over the views that cover the voxel, in ascending v: num = num + w * (double)s_f, den = den + w.
 *    out = den > 0.0 ? (float)(num / den) : background; the optional second output is (float)den.  Non-finite samples propagate as
 *    the arithmetic gives (0 * inf is NaN).
 * 7. Aligned views.  Per view: aligned_v[l] = inside ? s_f : 0.0f, weight_v[l] = inside ? (float)w : 0.0f.
 * A block may skip a view whose box its brick of output provably misses; the skip never changes a bit. */
#define MVSIM_FUSE_SINGULAR 1
typedef struct mvsim_fuse_params {
    double  blend[3];          /* default 8, 8, 8 voxels (a convention); >= 0 and finite */
    float   background;        /* default 0: where no view has weight */
    int32_t src_type;          /* default MVSIM_SRC_F32 */
} mvsim_fuse_params;           /* 32 bytes */
typedef struct mvsim_fuse_view {
    const void*   src;         /* the view's voxels (DEVICE for the _dev calls, HOST for the others) */
    int64_t       dim[3];
    const double* m_dev;       /* non-null: 12 doubles in DEVICE memory (e.g. &result_dev->m[0]), m is ignored; _dev calls only */
    double        m[12];       /* 3 x 4 row-major, view -> output frame */
} mvsim_fuse_view;             /* 136 bytes */
void mvsim_fuse_params_default(mvsim_fuse_params* p);
/* Host only, no context: step 1.  *singular = 1 and inv untouched, or *singular = 0 and inv = [i | it] as 3 x 4 row-major. */
int mvsim_fuse_invert(const double m[12], double inv[12], int* singular);
/* Host only: the output interval that holds every view (intersection = 0) or that every view covers (intersection = 1), as bounding
 * boxes.  m: 12 doubles per view, dims: 3 extents per view.  The 8 corners {0, N_d - 1} of every view go forward, each coordinate as
 * ((m_r0 * x + m_r1 * y) + m_r2 * z) + m_r3; a view's box is floor of the minima .. ceil of the maxima; out_dim = max - min + 1.
 * MVSIM_EINVAL: an empty intersection, a non-finite corner, n_views outside [1, MVSIM_MAX_VIEWS], an extent < 1. */
int mvsim_fusion_bounds(const double* m, const int64_t* dims, int n_views, int intersection, int64_t out_min[3], int64_t out_dim[3]);
/* Host only: the matrix that brings a view's PSF into the output frame as a small volume of out_kdim: PSF voxel k goes to
 * A (k - c) + c' with c_d = kdim_d / 2, c'_d = out_kdim_d / 2 (integer divisions: the centre mvsim_convolve uses), so
 * out = [A | c' - A c], t_r = (double)c'_r - ((A_r0 * c_x + A_r1 * c_y) + A_r2 * c_z).  mvsim_align_views with blend = 0 on the PSF
 * volume, out_min = 0 and out_dim = out_kdim then resamples it. */
int mvsim_fusion_psf_matrix(const double m[12], const int64_t kdim[3], const int64_t out_kdim[3], double out[12]);
/* Host only: {x, y, z extent of the brick of output a block owns, most blocks a launch has}. */
int mvsim_fusion_geometry(int64_t out[4]);
/* Steps 1-6 on the device.  views: HOST array of n_views records whose src (and m_dev) are DEVICE pointers; fused_dev and
 * sum_weights_dev_or_null: prod(out_dim) floats; status_dev_or_null: n_views int32 in DEVICE memory.  Asynchronous on the context's
 * stream, nothing is read back: a prepare kernel inverts the matrices, host-given and device-given, into a context workspace that
 * mvsim_release_caches frees, so detection -> registration -> fusion chain without a synchronisation.
 * MVSIM_EINVAL, before the context is touched: a null pointer, n_views outside [1, MVSIM_MAX_VIEWS], an extent < 1, an out_dim entry
 * < 1, a blend that is negative or not finite, a src_type outside the two, an output that overlaps a source. */
int mvsim_fuse_views_dev(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                         const mvsim_fuse_params* params, float* fused_dev, float* sum_weights_dev_or_null, int32_t* status_dev_or_null);
/* Steps 1-5 and 7.  aligned_dev: HOST array of n_views DEVICE pointers, entries may be NULL; weights_dev_or_null: the same, or NULL
 * for no weight volume at all. */
int mvsim_align_views_dev(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                          const mvsim_fuse_params* params, float* const* aligned_dev, float* const* weights_dev_or_null,
                          int32_t* status_dev_or_null);
/* The same two with HOST buffers and host matrices only (m_dev must be NULL); synchronous. */
int mvsim_fuse_views(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                     const mvsim_fuse_params* params, float* fused, float* sum_weights_or_null, int32_t* status_or_null);
int mvsim_align_views(mvsim_ctx* ctx, const mvsim_fuse_view* views, int n_views, const int64_t out_min[3], const int64_t out_dim[3],
                      const mvsim_fuse_params* params, float* const* aligned, float* const* weights_or_null, int32_t* status_or_null);

/* ---- PSF extraction: the beads of one view averaged into that view's PSF, in the output frame ------------------------------------
 * The link between mvsim_detect_beads / mvsim_register_beads and mvsim_deconvolve: a device-resident view, its detection list and
 * (optionally) its registration matrix go in, one normalised PSF volume comes out, already in the frame the matrix maps to, so that
 * mvsim_deconvolve_dev takes it as it is.  The reference has no counterpart; the recipe is this one, and every arithmetic step is stated
 * so that a literal restatement reproduces the result bit for bit.
 * Volumes are x fastest with dim = {Nx, Ny, Nz}; the source is float, or uint16_t widened with one (float)v on load.  A point list is
 * as in the registration: 3 doubles at a byte stride >= 24 that is a multiple of 8, n = min(max(*n_dev, 0), capacity) read from DEVICE
 * memory by the kernels, capacity <= MVSIM_PSF_MAX_POINTS.  All arithmetic is fp64 unless it says float, every + - * / an operation of
 * its own (no fused multiply-add), every sum and product evaluated as parenthesised.
 * 1. Inverse.  The forward matrix m = [A | t] (3 x 4 row-major, view -> output frame; NULL: the identity matrix, taken through the
 *    same arithmetic) is given on the host or as 12 doubles in device memory.  Only A is used: the nine i_rc are those of step 1 of
 *    the fusion applied to [A | 0].  If an entry of A is non-finite, or det is zero or non-finite: the flag is MVSIM_PSF_SINGULAR,
 *    n_listed = n, every other count, minimum and sum are 0, the PSF is all +0.0f, the status bytes are not written, nothing else runs.
 * 2. Offsets.  The PSF has odd extents kdim_d, 1 <= kdim_d <= MVSIM_PSF_MAX_DIM, centre c_d = kdim_d / 2.  For tap k:
 *        j_d = (double)(k_d - c_d),   delta_r = ((i_r2 * j_z) + i_r1 * j_y) + i_r0 * j_x
 *    and the sample position of tap k for a bead at pos is p_r = pos_r + delta_r: with the identity, pos + j exactly.
 * 3. Selection.  Every listed bead i < n gets one status byte, the first rule that applies:
 *      MVSIM_PSF_NONFINITE  a coordinate is not finite
 *      MVSIM_PSF_MASKED     a use-mask is given and use[i] == 0
 *      MVSIM_PSF_OUTSIDE    one of the eight corner taps (k_d in {0, kdim_d - 1}) has a p_d that fails
 *                           0.0 <= p_d && p_d <= (double)(N_d - 1)
 *      MVSIM_PSF_CROWDED    min_separation is not all zero and another finite listed point j != i, masked or not, has
 *                           fabs(pos_j,d - pos_i,d) < min_separation_d on all three axes (strict: an exact duplicate crowds both)
 *      MVSIM_PSF_USED       otherwise
 * 4. Sample, for a used bead and any tap: q_d = p_d > 0.0 ? p_d : 0.0, then q_d = q_d < (double)(N_d - 1) ? q_d : (double)(N_d - 1)
 *    (between inside corners a tap leaves the box only by rounding), then step 4 of the fusion on q verbatim: floor, u, lo,
 *    hi = min(lo + 1, N - 1), along x, then y, then z, rounded to float once: s_f.
 * 5. Sum per tap over the used beads, as step 4 of the registration takes its sums: chunks of MVSIM_PSF_CHUNK (256) consecutive list
 *    indices, unused beads skipped; a chunk's sum starts from +0.0 and adds (double)s_f ascending, the total starts from +0.0 and adds
 *    the sums of the ceil(n / 256) chunks ascending.
 * 6. Finish.  Taps are indexed t = k_x + kdim_x * (k_y + kdim_y * k_z).  mean_t = total_t / (double)n_used.  b = +inf, then ascending
 *    t: if mean_t < b then b = mean_t (a NaN is never smaller).  v_t = mean_t - b with subtract_min, else v_t = mean_t.  S is the sum
 *    of v_t, chunked by 256 consecutive tap indices exactly as in step 5.  With normalize and S > 0.0 and S finite:
 *    psf_t = (float)(v_t / S); otherwise psf_t = (float)v_t, and MVSIM_PSF_FLAT is set when normalize was asked for.
 *    n_used == 0: the flag is MVSIM_PSF_NO_BEADS, the PSF is all +0.0f, minimum and sum are 0.
 * The workspace of a call is ceil(capacity / 256) * prod(kdim) doubles of per-chunk partial sums, prod(kdim) doubles of totals and
 * capacity status bytes, in the context (mvsim_release_caches frees them). */
#define MVSIM_PSF_MAX_POINTS MVSIM_REG_MAX_POINTS
#define MVSIM_PSF_MAX_DIM    63
#define MVSIM_PSF_CHUNK      256
#define MVSIM_PSF_USED       0
#define MVSIM_PSF_NONFINITE  1
#define MVSIM_PSF_MASKED     2
#define MVSIM_PSF_OUTSIDE    3
#define MVSIM_PSF_CROWDED    4
#define MVSIM_PSF_SINGULAR   1
#define MVSIM_PSF_NO_BEADS   2
#define MVSIM_PSF_FLAT       4
typedef struct mvsim_psf_params {
    int64_t kdim[3];           /* default 15, 15, 15; odd, 1 .. MVSIM_PSF_MAX_DIM */
    double  min_separation[3]; /* default 15, 15, 15 voxels; >= 0 and finite; all zero: no crowding rule */
    int32_t src_type;          /* default MVSIM_SRC_F32 */
    int32_t subtract_min;      /* default 1 */
    int32_t normalize;         /* default 1 */
    int32_t pad;
} mvsim_psf_params;            /* 64 bytes */
typedef struct mvsim_psf_result {
    double  minimum, sum;      /* b and S of step 6 */
    int64_t n_listed, n_used, n_nonfinite, n_masked, n_outside, n_crowded;
    int32_t flags, pad;        /* MVSIM_PSF_SINGULAR | NO_BEADS | FLAT */
} mvsim_psf_result;            /* 72 bytes */
void mvsim_psf_params_default(mvsim_psf_params* p);
/* Host only, no context: steps 1 and 2.  offsets receives 3 doubles (delta_x, delta_y, delta_z) per tap, taps indexed as in step 6;
 * *singular = 1 leaves offsets untouched.  m_or_null: 12 doubles. */
int mvsim_psf_offsets(const double* m_or_null, const int64_t kdim[3], double* offsets, int* singular);
/* Host only: steps 1 and 3 over a host list of n >= 0 points.  status receives n bytes; result the counts, flags 0 or
 * MVSIM_PSF_SINGULAR, minimum = sum = 0.  Of params, kdim and min_separation are used. */
int mvsim_psf_select(const void* pos, int64_t stride, int64_t n, const unsigned char* use_or_null, const double* m_or_null,
                     const int64_t dim[3], const mvsim_psf_params* params, unsigned char* status, mvsim_psf_result* result);
/* Host only: step 6 over prod(kdim) host totals.  result goes in as the selection left it (n_used and flags are read) and comes out
 * complete; psf receives prod(kdim) floats. */
int mvsim_psf_finish(const double* totals, const mvsim_psf_params* params, float* psf, mvsim_psf_result* result);
/* Host only: {MVSIM_PSF_CHUNK, taps per block of the gather kernel, beads staged per tile of the crowding kernel, most blocks a
 * launch has}. */
int mvsim_psf_geometry(int64_t out[4]);
/* The stages on their own, asynchronous on the context's stream.  Selection: status_dev receives capacity bytes (n of them written),
 * result_dev one record as mvsim_psf_select leaves it.  m_or_null (host) and m_dev_or_null (DEVICE, e.g. &result_dev->m[0] of a
 * registration) exclude each other. */
int mvsim_psf_select_dev(mvsim_ctx* ctx, const void* pos_dev, int64_t stride, const int64_t* n_dev, int64_t capacity,
                         const unsigned char* use_dev_or_null, const double* m_or_null, const double* m_dev_or_null, const int64_t dim[3],
                         const mvsim_psf_params* params, unsigned char* status_dev, mvsim_psf_result* result_dev);
/* Steps 4 and 5 for the beads whose status byte is 0: totals_dev receives prod(kdim) doubles (all +0.0 when the matrix is singular,
 * and then the status bytes are not read). */
int mvsim_psf_gather_dev(mvsim_ctx* ctx, const void* img_dev, const int64_t dim[3], const void* pos_dev, int64_t stride,
                         const int64_t* n_dev, int64_t capacity, const unsigned char* status_dev, const double* m_or_null,
                         const double* m_dev_or_null, const mvsim_psf_params* params, double* totals_dev);
/* Step 6: result_dev goes in as the selection left it and comes out complete; psf_dev receives prod(kdim) floats. */
int mvsim_psf_finish_dev(mvsim_ctx* ctx, const double* totals_dev, const mvsim_psf_params* params, float* psf_dev,
                         mvsim_psf_result* result_dev);
/* The inliers of a registration as a use-mask: use_dev (n_points_capacity bytes) is zeroed, then byte a (side 0) or byte b (side 1)
 * of every candidate i < min(max(*n_candidates_dev, 0), capacity) whose mask byte is 1 -- of every candidate with a NULL mask -- is
 * set to 1; an index outside [0, n_points_capacity) is ignored. */
int mvsim_psf_use_from_matches_dev(mvsim_ctx* ctx, const mvsim_match* candidates_dev, const int64_t* n_candidates_dev, int64_t capacity,
                                   const unsigned char* mask_dev_or_null, int side, int64_t n_points_capacity, unsigned char* use_dev);
/* The whole recipe.  psf_dev: prod(kdim) floats; result_dev: one record; status_dev_or_null: capacity bytes.  Asynchronous on the
 * context's stream, nothing is read back.
 * MVSIM_EINVAL, before the context is touched: a null pointer where one is required, an extent < 1, a kdim entry even, < 1 or above
 * MVSIM_PSF_MAX_DIM, a stride below 24 or no multiple of 8, a capacity <= 0 or above MVSIM_PSF_MAX_POINTS, a min_separation that is
 * negative or not finite, an unknown src_type, both m and m_dev given, a psf_dev that overlaps the image. */
int mvsim_extract_psf_dev(mvsim_ctx* ctx, const void* img_dev, const int64_t dim[3], const void* pos_dev, int64_t stride,
                          const int64_t* n_dev, int64_t capacity, const unsigned char* use_dev_or_null, const double* m_or_null,
                          const double* m_dev_or_null, const mvsim_psf_params* params, float* psf_dev, mvsim_psf_result* result_dev,
                          unsigned char* status_dev_or_null);
/* The same with HOST buffers and a host matrix; synchronous.  n >= 0 points, at most MVSIM_PSF_MAX_POINTS; status_or_null: n bytes. */
int mvsim_extract_psf(mvsim_ctx* ctx, const void* img, const int64_t dim[3], const void* pos, int64_t stride, int64_t n,
                      const unsigned char* use_or_null, const double* m_or_null, const mvsim_psf_params* params, float* psf,
                      mvsim_psf_result* result, unsigned char* status_or_null);

/* ---- extractSlices over Intervals of volumes that stay on the device (SimulateTileStitching.java:131-189) ---------------
 * Views.zeroMin(Views.interval(con, min, max)) run through extractSlices: output voxel (x, y, k) of the contiguous tile
 * tx x ty x mvsim_extract_nz(tz, inc), t_d = max_d - min_d + 1, is f(in[(min_x + x) + Nx ((min_y + y) + Ny (min_z + k inc))]).
 * Its RNG counter is its index in the ZERO-MIN tile, x + tx (y + ty k inc), keyed by (seed, stream): bit for bit what
 * mvsim_extract_slices returns for the cropped tile (the interval is treated as zero-min). */
typedef struct mvsim_interval_job {
    const float* in;          /* DEVICE: the volume the interval is cut from (several jobs may name the same one) */
    int64_t  dim[3];          /* its size */
    int64_t  min[3], max[3];  /* inclusive corners, as an ImgLib2 Interval */
    int32_t  inc;  float snr; /* as mvsim_extract_slices: snr < 0 => copy */
    uint64_t seed; uint32_t stream;
} mvsim_interval_job;
/* out_dim = {tx, ty, mvsim_extract_nz(tz, inc)}.  Host only, no context; MVSIM_EINVAL as the extract calls below. */
int mvsim_interval_out_dim(const mvsim_interval_job* job, int64_t out_dim[3]);
/* 1 <= n <= MVSIM_MAX_VIEWS jobs in one call; out_dev: HOST array of n DEVICE pointers.  Asynchronous on the context's stream.
 * Jobs of equal tile size, inc and snr share their launches (one per sampler stage, blockIdx.y = job), the others follow one
 * another; the results do not depend on it.  MVSIM_EINVAL: null pointer, inc < 1, min_d > max_d, an interval that leaves its
 * volume, outputs that overlap each other or any job's volume, n out of range.  mvsim_get_extract_path reports kernel 5 for
 * an interval launch (the last one of the call; the fifth field: its jobs). */
int mvsim_extract_intervals_dev(mvsim_ctx* ctx, const mvsim_interval_job* jobs, int n, float* const* out_dev);
/* The same with outputs on the HOST (the volumes stay DEVICE pointers); synchronous.  Sampled outputs cross PCIe as the
 * acquisitions of the host-buffer views do: uint16 counts from 2^20 values up, automatic float32 fallback per output
 * (option "acq_transfer", mvsim_get_transfer_stats). */
int mvsim_extract_intervals(mvsim_ctx* ctx, const mvsim_interval_job* jobs, int n, float* const* out_host);
/* The two tiles of SimulateTileStitching (:119-121, :214-234), quirks included: overlap_d = (int)Math.round(dim_d ratio_d / 2);
 * tile 0 = [0, dim_d / 2 + overlap_d], tile 1 = [dim_0 / 2 - overlap_d, dim_d - 1] -- dimension 0 in every dimension, as the
 * reference has it.  Host only; the interval is not validated (a ratio of 1 leaves the volume: the extract calls refuse it). */
int mvsim_tile_interval(const int64_t dim[3], const double overlap_ratio[3], int tile,
                        int64_t min[3], int64_t max[3], int64_t overlap[3]);

/* ---- fused per-view pipeline: loop body SMVD:570-585 -------------------------------------- */
typedef struct mvsim_view_params {
    int32_t  axis;            /* 0 (SMVD:570)                                  */
    int32_t  degrees;         /* angle + angleOffset                           */
    double   delta;           /* attenuation, 0.01 (SMVD:533)                  */
    float    min_value;       /* 1e-4f (SMVD:77)                               */
    float    target_average;  /* 1     (SMVD:78)                               */
    int32_t  inc;             /* lightsheetSpacing (SMVD:532)                  */
    float    snr;             /* poissonSNR, 25 (SMVD:531); < 0 => no noise    */
    uint64_t seed;            /* counter-RNG key; 464232194 (SMVD:76)          */
    uint32_t stream;          /* view index                                    */
    int32_t  conv_method;     /* 0 auto, 1 FFT, 2 direct stencil               */
} mvsim_view_params;

/* Optional intermediate outputs (NULL = not wanted).  acq is required. */
typedef struct mvsim_view_outputs {
    float* rot;   /* Nx*Ny*Nz               (SMVD:570) */
    float* att;   /* Nx*Ny*Nz               (SMVD:573) */
    float* con;   /* Nx*Ny*Nz, adjusted     (SMVD:580-582) */
    float* acq;   /* Nx*Ny*extract_nz       (SMVD:585) */
} mvsim_view_outputs;

void mvsim_view_params_default(mvsim_view_params* p);

/* Device-resident: gt and every non-NULL output are device pointers; psf_host is a host
 * buffer, normalised in place.  Intermediates stay in HBM; nothing is copied to the host
 * except the scalar correction when correction != NULL (which forces a synchronise). */
int mvsim_simulate_view_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3],
                            float* psf_host, const int64_t kdim[3],
                            const mvsim_view_params* params, const mvsim_view_outputs* out,
                            double* correction);
/* The view loop of `main` (SimulateMultiViewDataset.java:567-585) for views that cannot fill the chip one at a time -- the
 * reference's own run is 7 views of a 289^3 volume with 51^3 PSFs (:376-380, :399, :531-548): n_views independent views of ONE
 * ground truth in one call.  psf_host[v] (normalised in place like everywhere else), params[v] and outs[v] describe view v; all
 * views share dim and kdim.  The library runs as many of them side by side as pays for their size (option "view_lanes" =
 * auto|1..32: child contexts of `ctx` on the same device, forked from and joined to ctx's stream, so the call is asynchronous on
 * that stream like mvsim_simulate_view_dev).  Every output is bit-identical to what n_views sequential mvsim_simulate_view_dev
 * calls write -- also when several views name the SAME (or overlapping) PSF memory, e.g. one buffer for all views: such PSFs are
 * normalised one after the other in view order, exactly as sequential calls would (a buffer named n times is normalised n times;
 * distinct buffers are normalised by one host thread each).  Output buffers must not overlap each other or the ground truth
 * (MVSIM_EINVAL). */
int mvsim_simulate_views_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* const* psf_host,
                             const int64_t kdim[3], const mvsim_view_params* params, const mvsim_view_outputs* outs,
                             int n_views);
/* The same with HOST buffers: the ground truth goes up once, the views run in one call (stacked / side by side as above), and the
 * acquisitions -- acq_host[v] of dim[0] * dim[1] * mvsim_extract_nz(dim[2], params[v].inc) floats -- come back together, as uint16 counts
 * over PCIe where the views are sampled (see mvsim_get_transfer_stats).  Synchronous; what a JVM calls for the reference's own run
 * (SimulateMultiViewDataset.java:567-585: seven views of one 289^3 volume). */
int mvsim_simulate_views(mvsim_ctx* ctx, const float* gt_host, const int64_t dim[3], float* const* psf_host,
                         const int64_t kdim[3], const mvsim_view_params* params, float* const* acq_host, int n_views);
/* One whole iteration of `main`'s view loop (SimulateMultiViewDataset.java:567-613), device-resident: the view above
 * (rotate, attenuate, convolve, adjust, extractSlices + Poisson) followed by what the loop does with its results --
 *   iso          = makeIsotropic(acq, inc)                                    (:588)   Nx*Ny*isotropic_nz
 *   view         = rotateAroundAxis(iso, axis, back_degrees)                  (:591)   same size (the reference passes -angle)
 *   view_weights = rotateAroundAxis(computeWeightImage(rot, delta), axis, back_degrees)   (:576,592)   Nx*Ny*Nz
 *   view_psf     = rotateAroundAxis(psf, axis, back_degrees)                  (:593)   Kx*Ky*Kz, the PSF as convolve() left it (normalised, Q5)
 * Every non-NULL member of `more` is a device buffer of that size; `iso` may be NULL with `view` set (library scratch).
 * computeWeightImage depends on the dimensions alone: it is rendered once per context and size and reused.
 * `out->acq` is required; the call is asynchronous on the context's stream. */
typedef struct mvsim_iteration_outputs {
    float* iso;
    float* view;
    float* view_weights;
    float* view_psf;
} mvsim_iteration_outputs;
int mvsim_simulate_iteration_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3],
                                 float* psf_host, const int64_t kdim[3],
                                 const mvsim_view_params* params, int back_degrees,
                                 const mvsim_view_outputs* out, const mvsim_iteration_outputs* more);
/* Host buffers in / out (what the JNI shim calls). */
int mvsim_simulate_view(mvsim_ctx* ctx, const float* gt, const int64_t dim[3],
                        float* psf_host, const int64_t kdim[3],
                        const mvsim_view_params* params, const mvsim_view_outputs* out,
                        double* correction);

/* Pipelined host-buffer views for a caller that loops over views (SMVD:567-613, SimulateTileStitching.java:93-111):
 * the call enqueues  upload(gt) -> view -> download(outputs)  on three HIP streams over two staging sets and returns a
 * ticket at once, so that upload(v+1), compute(v) and download(v-1) overlap; with page-locked buffers (mvsim_host_alloc)
 * a 512^3 view costs one PCIe transfer time instead of the sum of three phases.  gt_host, psf_host and every output
 * buffer must stay valid and untouched until mvsim_wait(ticket) returns; at most two tickets may be outstanding (a
 * third call waits for the oldest).  The ground truth is uploaded again only when its pointer or `gt_generation`
 * differs from what the staging set already holds (pass a new generation after changing the buffer's contents; the
 * view loop of `main` passes the same `rendered` image for every angle).  psf_host is normalised in place before the
 * call returns.  Intermediates (rot/att/con) may be requested; they are single-buffered on the device, so views that ask
 * for them do not overlap with their neighbours' downloads. */
int mvsim_simulate_view_async(mvsim_ctx* ctx, const float* gt_host, uint64_t gt_generation, const int64_t dim[3],
                              float* psf_host, const int64_t kdim[3], const mvsim_view_params* params,
                              const mvsim_view_outputs* out_host, int64_t* ticket);
/* Blocks until the view behind `ticket` has landed in its host buffers; *correction (may be NULL) receives the
 * adjustImage factor.  Tickets may be waited for in any order, each once. */
int mvsim_wait(mvsim_ctx* ctx, int64_t ticket, double* correction);
/* How the acquisitions of mvsim_simulate_view_async crossed PCIe.  Tools.poissonProcess stores Poisson COUNTS as floats
 * (Tools.java:84): a sampled view (snr >= 0) is packed to uint16 on the device, downloaded as half the bytes and widened into the
 * caller's float buffer by mvsim_wait (a few host threads, option "host_threads" = auto|1..256); a view holding a value that does not
 * survive the round trip (a count beyond 65 535) is fetched as float32 after all, automatically.  Exact either way.  Option
 * "acq_transfer" = auto|f32 (f32: never pack).  *views_as_u16: views that took the 16-bit path so far, *fallbacks: how many of them
 * had to be fetched as float32.  Either pointer may be NULL. */
int mvsim_get_transfer_stats(mvsim_ctx* ctx, int64_t* views_as_u16, int64_t* fallbacks);
/* Host buffers given as z slabs: volumes beyond 2^31-1 voxels do not fit one Java array / direct buffer
 * (SimulateMultiViewDataset.java:109 uses ArrayImg and cannot hold them at all), so the ground truth arrives as
 * n_gt_slabs pointers of gt_slab_nz[i] planes each (sum = dim[2]) and the acquisition leaves as n_acq_slabs pointers of
 * acq_slab_nz[j] planes each (sum = mvsim_extract_nz(dim[2], inc)).  Same arithmetic as mvsim_simulate_view. */
int mvsim_simulate_view_zslabs(mvsim_ctx* ctx, const float* const* gt_slabs, const int64_t* gt_slab_nz, int n_gt_slabs,
                               const int64_t dim[3], float* psf_host, const int64_t kdim[3],
                               const mvsim_view_params* params, float* const* acq_slabs, const int64_t* acq_slab_nz,
                               int n_acq_slabs, double* correction);

/* The per-stage operators with HOST buffers given as z slabs: an ArrayImg may hold 2^31-1 voxels (SimulateMultiViewDataset.java:109,
 * :198, :235, :321 create their results with ArrayImgFactory) but one direct ByteBuffer only 2^31-1 BYTES, so the Java facade hands
 * volumes beyond 2^29 voxels over as several page-locked blocks.  in_slabs[i] holds in_slab_nz[i] planes (sum = dim[2]); out_slabs[j]
 * receives out_slab_nz[j] planes (sum = dim[2], or mvsim_extract_nz(dim[2], inc) for extractSlices).  Same arithmetic as the
 * single-buffer entry points (SMVD:104-135, :318-364, :253-264, :181-231). */
int mvsim_rotate_around_axis_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                                    int axis, int degrees, float* const* out_slabs, const int64_t* out_slab_nz, int n_out);
int mvsim_attenuate3d_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                             double delta, float* const* out_slabs, const int64_t* out_slab_nz, int n_out);
int mvsim_convolve_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                          float* psf, const int64_t kdim[3], int method, float* const* out_slabs, const int64_t* out_slab_nz, int n_out);
int mvsim_extract_slices_zslabs(mvsim_ctx* ctx, const float* const* in_slabs, const int64_t* in_slab_nz, int n_in, const int64_t dim[3],
                                int inc, float snr, uint64_t seed, uint32_t stream, float* const* out_slabs, const int64_t* out_slab_nz,
                                int n_out);

/* ---- per-stage device timings of the last simulate_view / stage call (milliseconds) ------ */
typedef struct mvsim_timings {
    /* psf_ms is 0 when the PSF spectrum ran on the context's side stream (option psf_overlap, views of >= 2^24 voxels):
     * it then overlaps passes A and B and its time is part of convolve_ms */
    float rotate_ms, attenuate_ms, psf_ms, convolve_ms, adjust_ms, extract_ms, total_ms;
    /* the passes of the hand-written convolution, nested inside convolve_ms (0 on other paths): x real->complex,
     * y forward, z (direct convolution or FFT + product + inverse FFT), y inverse, x complex->real + crop + sum */
    float pass_a_ms, pass_b_ms, pass_c_ms, pass_d_ms, pass_e_ms;
} mvsim_timings;
/* Geometry of the hand-written convolution for this volume / PSF: {Px, Py, planes of the spectrum, Hxp (complex row
 * pitch), 1 if the z pass is the direct convolution}.  A pass moves 8 * Hxp * Py * planes bytes each way (the x passes
 * 4 N on their real side).  MVSIM_EINVAL when the sizes fall outside the pass table (rocFFT path). */
int mvsim_fft_geometry(const int64_t dim[3], const int64_t kdim[3], int64_t geometry[5]);
/* The direct z pass of a whole view of this volume / PSF that returns its acquisition only (every inc-th plane), under the default
 * options: out = {kernel: 0 = k_zconv, which computes every plane -- else the stride s of k_zconv_strided<s>, which computes the planes
 * k * inc alone --; zc, the outputs of a tile along z; nch, the tiles of a z column; nkxb, the 16-column groups of a spectrum row}.
 * The same figures hold for every view of a stacked call.  Host only, no context.  MVSIM_EINVAL: inc < 1, no hand-written FFT size, or
 * a z pass that is not the direct convolution (more than 64 z taps, fft_zpass = fft, the inline FFT z pass of deep PSFs). */
int mvsim_zpass_geometry(const int64_t dim[3], const int64_t kdim[3], int inc, int64_t out[4]);
/* Geometry of the direct LDS-tiled stencil (method 2) for this PSF: {taps of one x chunk, y taps, z taps of the PSF chunk a
 * tile serves, LDS bytes per block, blocks per CU}.  Any PSF of 1..64 taps per axis is accepted (SimulateMultiViewDataset.java:579
 * loads 51^3 stacks); beyond that MVSIM_EINVAL (use the FFT method). */
int mvsim_stencil_geometry(const int64_t kdim[3], int64_t geometry[5]);
/* The extract + Poisson sampler form one launch takes for nzo = (dim[2] - 1) / inc + 1 acquired planes of dim[0] x dim[1] voxels, the RNG
 * counter of plane k's voxel i being index_offset + k * index_inc * plane + i (index_inc 0: inc).  aligned16: both buffers allow 16-byte
 * accesses; queue_share: 0 = no work queue, else 1..16 sixteenths of a block's voxels its segment holds (the share option resolved; small
 * volumes resolve "auto" to 16).  path = {kernel: 0 one voxel per lane, 1 four voxels per lane, 2 two-launch vector form, 3 two-launch
 * group-by-group form; 1 if queue segments can refuse voxels; blocks; items per segment (0: no queue)}.  Host only, no context. */
int mvsim_extract_path(const int64_t dim[3], int inc, int index_inc, uint64_t index_offset, int aligned16, int queue_share, int64_t path[4]);
/* The sampler form of the last extract + Poisson this context enqueued: {kernel as mvsim_extract_path, or 4 for the fused tail of the
 * convolution, or 5 for an interval launch (mvsim_extract_intervals*: items per segment 0 = one voxel per lane, else the two-launch
 * form); 1 if queue segments can refuse voxels; blocks; items per segment; views or jobs in the launch (> 1: the per-view tables)}.
 * Recorded on the host when the work is enqueued; kernel -1 before the first. */
int mvsim_get_extract_path(mvsim_ctx* ctx, int64_t path[5]);
/* {blocks, items per segment} of the fused tail (the convolution's last pass adjusts, extracts and samples) for a noisy view of this
 * volume / PSF under the context's options, with (want_con) or without the adjusted volume; MVSIM_EINVAL when it would not be fused. */
int mvsim_fused_tail_geometry(mvsim_ctx* ctx, const int64_t dim[3], const int64_t kdim[3], int inc, int want_con, int64_t out[2]);
/* Planes the convolution passes of the last FLAGGED view skipped (option "skip_empty"; exact: the spectrum of an empty attenuated plane
 * is zero): stats = {planes of the view, planes whose attenuated image is empty (pass B does not transform them, the z pass does not
 * read them), planes of the z pass's output that are empty (passes D and E skip them)}.  Read from a page-locked word the device
 * writes, without synchronising: call after the view has completed.  All zero when no view has carried flags yet. */
int mvsim_get_plane_stats(mvsim_ctx* ctx, int64_t stats[3]);
/* Whether the tail of the last view this context enqueued ran in sparse mode (option "skip_tail", default 1; exact): out = {1 if the
 * convolution's last pass stored nothing into the planes of its output that are known to be empty and phase 1 of the Poisson sampler read
 * nothing there, else 0; the plane stride of the flags the two shared (0 outside the mode)}.  The mode needs a flagged view (see
 * mvsim_get_plane_stats), the convolved volume not requested, and a sampled view on the work queue; together with the third figure of
 * mvsim_get_plane_stats it says how many planes were left out.  Recorded on the host when the work is enqueued. */
int mvsim_get_tail_path(mvsim_ctx* ctx, int64_t out[2]);
/* PSF spectra kept by content (option "psf_cache" = MiB of device memory, default 1024; 0 switches it off; exact).  A whole single view
 * on the hand-written FFT with the direct z pass (mvsim_simulate_view_dev and the host / async entry points on top of it) whose
 * NORMALISED PSF and geometry the context has seen before uploads no PSF and launches neither of the PSF's two transform passes: the
 * convolution reads the spectrum the first such view computed.  The PSF is normalised in place on every call all the same.  A lookup
 * is a 64-bit hash and then a comparison of every tap; replacement is least recently used under the cap.  Stacked views, lanes, z
 * slabs, rocFFT, fft_zpass=fft / inline, graph=1, conv_method 2, mvsim_convolve_dev and an iteration that returns view_psf do not use
 * the cache.  out = {hits, misses, evictions, device bytes held} of this context; mvsim_release_caches frees the entries and keeps
 * the three counters.  Recorded on the host when the work is enqueued. */
int mvsim_get_psf_cache_stats(mvsim_ctx* ctx, int64_t out[4]);
/* The work queue of the Poisson sampler (Tools.java:73-86 is one sample per voxel; here the voxels whose sample needs the divergent fp64
 * code wait in per-block segments for a second kernel): stats = {bytes of queue workspace the context holds, items one segment holds,
 * bright items (lambda >= 10) and inversion items (lambda < 10) the context's last sampled view queued -- the first view of a stacked
 * call --, voxels its full segments refused (a third kernel samples them where they stand: same counts, slower), pending voxels (queued
 * or refused) of its fullest block: the segment size that refuses nothing}.
 * Option "poisson_queue_share" = 1..16 fixes the sixteenths of a block's voxels its segment holds (16, the default: 16 bytes per
 * acquired voxel, nothing is ever refused, the fastest).  "auto": 16 for queues of up to 64 MiB; otherwise 5 at first, and after a view
 * whose segments refused voxels the context's later views get what that view would have needed plus one sixteenth (memory for ~2 % of
 * a 512^3 view's time).  Counts are the same for every share.
 * Synchronises the context.  (Zeros after a view that did not go through the two-launch sampler: options "poisson_queue=0", "fuse_tail=1".) */
int mvsim_get_queue_stats(mvsim_ctx* ctx, int64_t stats[6]);
int mvsim_enable_timing(mvsim_ctx* ctx, int enable);
int mvsim_get_timings(mvsim_ctx* ctx, mvsim_timings* t);

/* ---- multi-GPU: one process per GPU, views shard across ranks (RCCL over xGMI) ------------ */
#define MVSIM_UNIQUE_ID_BYTES 128
/* rank 0 creates the id, the host passes the 128 bytes to every rank by any means. */
int mvsim_comm_unique_id(unsigned char id[MVSIM_UNIQUE_ID_BYTES]);
int mvsim_comm_init(mvsim_ctx* ctx, int nranks, int rank, const unsigned char id[MVSIM_UNIQUE_ID_BYTES]);
/* The RCCL this library is bound to in the running process: file path of the shared object that provides ncclGetVersion
 * (a process that loaded PyTorch first holds torch/lib/librccl.so under the same soname) and its version code
 * (major * 10000 + minor * 100 + patch).  Either output may be NULL. */
int mvsim_comm_library_info(char* path, size_t path_capacity, int* version);
/* Broadcast the ground-truth volume (device pointer, count floats) from root; enqueued on
 * the context stream.  The only collective on the path (views are independent, SMVD:567).
 * Default form: scatter (root sends chunk r to rank r, nranks-1 concurrent ncclSend: one per xGMI link) followed by
 * an in-place ncclAllGather, so that all links carry traffic; option "broadcast" = ring selects one ncclBroadcast. */
int mvsim_comm_broadcast_volume(mvsim_ctx* ctx, float* vol_dev, int64_t count, int root);
/* Option "broadcast" = peer_copy moves the chunks of the same scatter + all-gather with the copy engines between the ranks'
 * buffers (IPC-mapped into each other's processes; no RCCL kernels beside the views).  The buffer a rank broadcasts into must have
 * been REGISTERED: a collective -- every rank calls it, in the same order as the other collectives of the communicator, each for
 * its own buffer of >= count floats; it synchronises the context's stream.  A registration is never reused for another buffer:
 * registering again replaces it, mvsim_comm_unregister_volume (local), mvsim_dev_free of the buffer and mvsim_comm_destroy drop
 * it -- LOCALLY: the other ranks keep their mappings of this rank's buffer until THEY unregister, register again or destroy their
 * communicator.  So a registered volume is unregistered (or freed) on EVERY rank before any rank runs another peer_copy broadcast;
 * a broadcast into a registration one rank has already dropped writes through a mapping of freed memory.
 * One process per rank (ranks that share a process use the RCCL forms). */
int mvsim_comm_register_volume(mvsim_ctx* ctx, float* vol_dev, int64_t count);
/* Option "broadcast" = pipelined: scatter + all-gather loads the root's outbound links twice (its scatter chunks, then its own chunk of
 * the all-gather: 2 S / (N b) for a volume of S bytes over links of b bytes/s).  The pipelined form scatters the WHOLE volume as N - 1
 * chunks to the N - 1 peers, piece by piece, and lets the peers all-gather the pieces that have arrived among themselves over the
 * peer<->peer links WHILE the next piece leaves the root: one group of ncclSend / ncclRecv per stage, ~ S / ((N - 1) b) in all (1.3-1.4 ms
 * instead of 2.2 ms for a 512^3 volume on 8 GPUs).  The schedule is a pure function of (nranks, rank, root, count, pieces): this entry point
 * returns it -- ops[i] = {stage, kind (0 send, 1 receive), peer rank, first float, floats} in issue order, *n_ops of them (MVSIM_EINVAL when
 * capacity is too small; ops may be NULL to ask for the count) -- so that a host can check it without a GPU (every send has its receive in
 * the same stage, every rank ends with every float).  The last stage holds the unaligned tail as sends from the root. */
typedef struct mvsim_bcast_op { int32_t stage, kind, peer, pad; int64_t first, count; } mvsim_bcast_op;
int mvsim_comm_broadcast_plan(int nranks, int rank, int root, int64_t count, int pieces, mvsim_bcast_op* ops, int capacity, int* n_ops);
int mvsim_comm_unregister_volume(mvsim_ctx* ctx, const float* vol_dev);
/* In-place sum over ranks (RCCL all-reduce) of a device float buffer: the per-voxel weight sums of SMVD:625-628
 * when the views live on different GPUs.  Summation order differs from the sequential reference (<= 1 ulp). */
int mvsim_comm_allreduce_sum(mvsim_ctx* ctx, float* buf_dev, int64_t count);
/* Sum over ranks of ONE double held on the host (in place; synchronises): the adjustImage sum of a view whose
 * z slabs live on different GPUs. */
int mvsim_comm_allreduce_sum_f64(mvsim_ctx* ctx, double* value_host);
/* The same sum for ONE double that lives on the DEVICE (in place, asynchronous, no host trip): enqueued on `hip_stream` (null: the
 * context's stream), so a caller can order it behind the kernel that produces the value.  What mvsim_view_slab_dev runs between a
 * slab's convolution and its adjust (SimulateMultiViewDataset.java:582: Tools.adjustImage needs the whole view's sum). */
int mvsim_comm_allreduce_sum_f64_dev(mvsim_ctx* ctx, double* value_dev, void* hip_stream);
int mvsim_comm_destroy(mvsim_ctx* ctx);
/* view v of n_views belongs to rank v % nranks; returns how many views `rank` owns and writes
 * their indices (capacity max_out). */
int mvsim_shard_views(int n_views, int nranks, int rank, int* view_idx, int max_out);

/* ---- one PROCESS driving several GPUs (what a JVM host is): a group owns one context per device and an RCCL
 * communicator over them (ncclCommInitAll).  The ground truth goes host -> device 0 -> all devices (scatter +
 * all-gather over xGMI), then view v of SimulateMultiViewDataset.main's loop (:567-613) runs on device v % ndev and
 * its acquisition is copied to acq_host[v]; the call returns when every view has landed.  psf_host[v] is normalised in
 * place like everywhere else.  devices == NULL means 0 .. ndev-1. */
typedef struct mvsim_group mvsim_group;
int        mvsim_group_create(int ndev, const int* devices, mvsim_group** group);
int        mvsim_group_destroy(mvsim_group* group);
int        mvsim_group_size(const mvsim_group* group);
mvsim_ctx* mvsim_group_ctx(mvsim_group* group, int index);
/* gt_host is free for reuse when the call returns (the upload has completed; the collectives behind it may still run). */
int        mvsim_group_broadcast_volume(mvsim_group* group, const float* gt_host, const int64_t dim[3]);
int        mvsim_group_simulate_views(mvsim_group* group, float* const* psf_host, const int64_t kdim[3],
                                      const mvsim_view_params* params, int n_views, float* const* acq_host);

/* ---- z-slab tiling of ONE view across GPUs (BASELINE configs[3]/[4]) ----------------------------
 * For volumes whose views should be split over several GPUs: rank r owns the planes [z0, z1) of the view
 * (mvsim_slab_range gives a balanced partition).  Every rank holds the whole ground truth (broadcast); rotation and
 * attenuation of the slab and of the Kz/2 halo planes the PSF reaches are recomputed locally (attenuation runs along
 * y inside a plane, SMVD:335-359), the mirror boundary acts at the global faces only, and the only exchange is the
 * sum of the convolved voxels that adjustImage needs.  Per view and rank:
 *     mvsim_view_slab_convolve_dev(...,&slab_sum)      rotate, attenuate, convolve the slab (kept in the context)
 *     total = sum of slab_sum over ranks               e.g. mvsim_comm_allreduce_sum_f64
 *     mvsim_view_slab_finish_dev(..., total, acq)      adjust with the global mean, extract, Poisson
 * acq receives the acquired planes k with z0 <= k*inc < z1, in order (*n_planes of them); Poisson counters use the
 * global voxel index, so the tiling is invisible in the counts.  Needs rotation about x (axis 0), the hand-written
 * convolution path and a PSF depth <= 64. */
int mvsim_slab_range(int64_t nz, int nranks, int rank, int64_t* z0, int64_t* z1);
int mvsim_view_slab_convolve_dev(mvsim_ctx* ctx, const float* gt, const int64_t dim[3], float* psf_host,
                                 const int64_t kdim[3], const mvsim_view_params* params, int64_t z0, int64_t z1,
                                 double* slab_sum);
int mvsim_view_slab_finish_dev(mvsim_ctx* ctx, const int64_t dim[3], const mvsim_view_params* params, int64_t z0,
                               int64_t z1, double total_sum, float* acq, int64_t* n_planes);
/* The three steps above as ONE asynchronous call that never leaves the device: the slab's share of the sum stays in HBM, is reduced
 * over the ranks in place by the communicator of `comm_ctx` (null: ctx's own; no communicator or one rank: nothing to reduce) ON
 * ctx's stream, and adjust, extract and Poisson follow behind it.  The loop body tiled is SimulateMultiViewDataset.java:570-585.
 * Same results as the three-step form (the reduction adds the same doubles; RCCL's order over ranks may differ from a host
 * loop's in the last bit of the sum). */
int mvsim_view_slab_dev(mvsim_ctx* ctx, mvsim_ctx* comm_ctx, const float* gt, const int64_t dim[3], float* psf_host,
                        const int64_t kdim[3], const mvsim_view_params* params, int64_t z0, int64_t z1, float* acq,
                        int64_t* n_planes);

#ifdef __cplusplus
}
#endif
#endif /* MVSIM_H */
