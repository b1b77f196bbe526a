package net.preibisch.simulation.gpu;

import java.nio.FloatBuffer;

/**
 * JNI binding of libmvsim.so (C ABI in include/mvsim.h).  One native context per GPU; the context is
 * not thread-safe, so {@link GpuContextPool} hands one to each calling thread.
 *
 * SOURCE ONLY in this repository: the build image has no JDK (no javac, no jni.h); this layer has never been compiled
 * or run.  Compile on a host with a JDK: see INTEGRATION.md.
 */
final class MvsimNative
{
	static { System.loadLibrary( "mvsim_jni" ); }

	private MvsimNative() {}

	static native long create( int device );                          // mvsim_create
	static native void destroy( long ctx );                           // mvsim_destroy
	static native int deviceCount();                                  // mvsim_device_count

	// all buffers are DIRECT FloatBuffers (x fastest); dim = {nx, ny, nz}.  The shim checks every buffer's capacity against
	// the dimensions before it touches the C ABI and throws IllegalArgumentException when one is too small.
	static native void rotateAroundAxis( long ctx, FloatBuffer in, long[] dim, int axis, int degrees, FloatBuffer out );
	static native void attenuate3d( long ctx, FloatBuffer in, long[] dim, double delta, FloatBuffer out );
	static native void normImage( long ctx, FloatBuffer img, long n );
	static native void convolve( long ctx, FloatBuffer img, long[] dim, FloatBuffer psf, long[] kdim, int method, FloatBuffer out );
	static native double adjustImage( long ctx, FloatBuffer img, long n, float minValue, float targetAverage );
	static native void extractSlices( long ctx, FloatBuffer in, long[] dim, int inc, float snr, long seed, int stream, FloatBuffer out );
	static native void poissonProcess( long ctx, FloatBuffer img, long n, double snr, long seed, int stream, long indexOffset );
	static native void makeIsotropic( long ctx, FloatBuffer in, long[] dim, int inc, FloatBuffer out );
	static native void computeWeightImage( long ctx, long[] dim, FloatBuffer out );
	static native void axisRotation( long[] dim, int axis, int degrees, double[] m12 );
	// SimulateBeads.renderPoints for nviews views (mvsim_render_beads): xyz = n * 3 doubles, viewOffsets = nviews + 1 entries or null
	// (every view renders all points), m12 = nviews row-major 3x4 matrices or null (points as given), interval = {min x, y, z, max x, y, z};
	// images of (max - min) voxels per axis; either output list may be null
	static native void renderBeads( long ctx, java.nio.DoubleBuffer xyz, long n, long[] viewOffsets, java.nio.DoubleBuffer m12, int nviews,
			long[] interval, double sigmaX, double sigmaY, double sigmaZ, FloatBuffer[] outF32, java.nio.ShortBuffer[] outU16 );

	// SimulateMultiViewAberrations.refract3d (mvsim_refract3d): numRays rays drawn from rndState[0] (the 48-bit java.util.Random state,
	// advanced on return) through imgRi; image and weight receive the injection's two volumes
	static native void refract3d( long ctx, FloatBuffer imgIn, FloatBuffer imgRi, long[] dim, boolean illum, int z, double lsMiddle,
			double lsEdge, double ri, long numRays, long[] rndState, FloatBuffer image, FloatBuffer weight );
	// SimulateMultiViewAberrations.projectToCamera (mvsim_project_to_camera): proj receives dim[0] * dim[1] floats
	static native void projectToCamera( long ctx, FloatBuffer imgRi, FloatBuffer refr, long[] dim, int currentZ, int raysPerPixel,
			long[] rndState, FloatBuffer proj );

	// the general tracer under RayTracingTest (mvsim_trace_rays): n rays from pos3 along dir3 (3 n doubles each) through imgRi mapped by
	// (nB - nA) * sample + nA; the value carried is imgIn's sample, else intensity (n floats), else constantValue (either may be null);
	// totalReflection 0 keeps the direction, 1 reflects; image and weight (both or neither) receive the sandbox's injection (sigma 0.5,
	// normalized).  Returns the number of rays still inside after maxMoves moves
	static native long traceRays( long ctx, FloatBuffer imgRi, FloatBuffer imgIn, long[] dim, java.nio.DoubleBuffer pos3, java.nio.DoubleBuffer dir3,
			FloatBuffer intensity, long n, double nA, double nB, double evThreshold, long maxMoves, int totalReflection, boolean normalizeDirs,
			double constantValue, FloatBuffer image, FloatBuffer weight );
	// Raytrace.drawSimpleImage (mvsim_draw_simple_image): the wedge
	static native void drawSimpleImage( long ctx, FloatBuffer out, long[] dim, float low, float high );
	// RayTracingTest.drawMultipleRays' bundle (mvsim_sandbox_ray_starts): n starts around (x, Ny - 1, z) drawn from rndState[0], advanced on return
	static native void sandboxRayStarts( long ctx, long[] rndState, long[] dim, int x, int z, long n, java.nio.DoubleBuffer pos3,
			java.nio.DoubleBuffer dir3 );

	// the per-stage operators with volumes as z-slab lists (mvsim_*_zslabs): in[i] holds inNz[i] planes, out[j] receives outNz[j];
	// this is how images beyond one 2 GiB direct buffer (2^29 voxels) cross the boundary -- a 512^3 image is a list of one
	static native void rotateAroundAxisSlabs( long ctx, FloatBuffer[] in, long[] inNz, long[] dim, int axis, int degrees, FloatBuffer[] out, long[] outNz );
	static native void attenuate3dSlabs( long ctx, FloatBuffer[] in, long[] inNz, long[] dim, double delta, FloatBuffer[] out, long[] outNz );
	static native void convolveSlabs( long ctx, FloatBuffer[] in, long[] inNz, long[] dim, FloatBuffer psf, long[] kdim, int method,
			FloatBuffer[] out, long[] outNz );
	static native void extractSlicesSlabs( long ctx, FloatBuffer[] in, long[] inNz, long[] dim, int inc, float snr, long seed, int stream,
			FloatBuffer[] out, long[] outNz );

	/** mvsim_host_alloc wrapped by NewDirectByteBuffer: a page-locked block (null if the allocation fails); freePinned releases it. */
	static native java.nio.ByteBuffer allocPinned( long ctx, long bytes );
	static native void freePinned( java.nio.ByteBuffer block );
	/**
	 * count floats between a direct FloatBuffer (from blockOffset) and a heap array (from arrayOffset) on the library's host threads
	 * (mvsim_host_copy; the array is held with GetPrimitiveArrayCritical meanwhile).  toArray: block -> array, else array -> block.
	 */
	static native void copyFloats( long ctx, java.nio.FloatBuffer block, long blockOffset, float[] array, int arrayOffset, int count, boolean toArray );

	/** drawSpheres (:436-522), in place; rndState[0] is the 48-bit java.util.Random state, advanced on return; returns the sphere count. */
	static native long drawSpheres( long ctx, FloatBuffer img, long[] dim, double minValue, double maxValue, int scale,
			boolean halfPixelOffset, long[] rndState );
	/** The noise on the refractive-index volume (SimulateMultiViewAberrations :425-426) over n floats, in place; rndState as for drawSpheres. */
	static native void riNoise( long ctx, FloatBuffer ri, long n, long[] rndState );
	/** multiSpheres (SimulateMultiViewAberrations :474-586), in place on image and index volume; returns the sphere count. */
	static native long multiSpheres( long ctx, FloatBuffer img, FloatBuffer ri, long[] dim, int scale, long[] rndState );
	/** out[0] = stream positions per chunk of the device walk, out[1] = entry offsets resolved per chunk (mvsim_sphere_walk_geometry). */
	static native void sphereWalkGeometry( long[] out );
	/** mvsim_splat_spheres: geometry ={ cx, cy, cz, radius } per sphere, values = one float per sphere; in place. */
	static native void splatSpheres( long ctx, FloatBuffer img, long[] dim, int[] geometry, float[] values );
	/** downSample2x (:394-424): out has dim/2 - 1 samples per dimension. */
	static native void downSample2x( long ctx, FloatBuffer in, long[] dim, FloatBuffer out );

	// ---- volumes that stay on the device (SimulateTileStitchingGPU) ----
	/** mvsim_dev_alloc: a device pointer as a long; devFree (mvsim_dev_free) releases it, 0 is ignored. */
	static native long devAlloc( long ctx, long bytes );
	static native void devFree( long ctx, long dptr );
	/** mvsim_upload: n floats of a direct buffer to the device pointer; returns when src may be reused. */
	static native void uploadFloats( long ctx, long dptr, FloatBuffer src, long n );
	/**
	 * mvsim_extract_intervals: extractSlices over intervals of DEVICE volumes, all jobs in one call.  geometry holds 10 longs per job
	 * {volume (device pointer), Nx, Ny, Nz, min x, y, z, max x, y, z} (inclusive corners); inc, snr, seed and stream one entry per job;
	 * out[j] receives the zero-min tile, tx * ty * ((tz - 1) / inc + 1) floats.  The shim checks every array length and buffer capacity first.
	 */
	static native void extractIntervals( long ctx, long[] geometry, int[] inc, float[] snr, long[] seed, int[] stream, FloatBuffer[] out );

	/** Cross-view weight normalisation (:615-640), in place on every buffer. */
	static native void normalizeWeights( long ctx, FloatBuffer[] weights, long n, float osem );

	/**
	 * Multi-view deconvolution (mvsim_deconvolve; include/mvsim.h states the recipe): views, weights (null: none) and psfs hold one direct
	 * buffer per view, kdims three PSF extents per view.  psi is read where initFromPsi is set and always receives the estimate.  The
	 * PSF buffers are not written (unlike convolve).  The shim checks every array length and buffer capacity first.
	 */
	static native void deconvolve( long ctx, FloatBuffer[] views, FloatBuffer[] weights, FloatBuffer[] psfs, long[] kdims, long[] dim,
			int iterations, int method, boolean initFromPsi, float initValue, float minValue, float eps, double lambda, FloatBuffer psi );

	/**
	 * Bead detection (mvsim_detect_beads; include/mvsim.h states the recipe): DoG interest points with sub-voxel localisation.  img is a direct
	 * FloatBuffer, or with u16 a direct ShortBuffer, of nx * ny * nz elements; peaks a direct ByteBuffer in native order of at least
	 * 40 * capacity bytes that receives min(found, capacity) records {double x, y, z; float value; int flags; long voxel}.  Returns the
	 * number found.  The shim checks every length and capacity first.
	 */
	static native long detectBeads( long ctx, java.nio.Buffer img, boolean u16, long[] dim, double sigma1X, double sigma1Y, double sigma1Z,
			double sigma2X, double sigma2Y, double sigma2Z, float threshold, int maxMoves, long capacity, java.nio.ByteBuffer peaks );

	/**
	 * Bead registration (mvsim_register_beads; include/mvsim.h states the recipe): geometric descriptors, ratio-test matching, RANSAC and an
	 * affine refit from list A to list B.  posA / posB are direct DoubleBuffers of 3 n doubles (x, y, z per point); result a direct
	 * ByteBuffer in native order of at least 160 bytes that receives {double m[12], meanError, maxError; long nA, nB, nCandidates, nInliers,
	 * bestHypothesis; int refits, flags}; candidates (or null) at least 24 * max(nA, 1) bytes for records {int a, b; double vBest, vSecond};
	 * mask (or null) at least max(nA, 1) bytes, one per candidate.  Returns the number of candidates.  The shim checks every length first.
	 */
	static native long registerBeads( long ctx, java.nio.DoubleBuffer posA, long nA, java.nio.DoubleBuffer posB, long nB, int redundancy,
			double ratio, double maxEpsilon, double minInlierRatio, long seed, int hypotheses, int maxRefits, int minInliers,
			java.nio.ByteBuffer result, java.nio.ByteBuffer candidates, java.nio.ByteBuffer mask );

	/**
	 * View fusion (mvsim_fuse_views; include/mvsim.h states the recipe): every view is resampled through its 3 x 4 matrix view to output
	 * frame into the interval outMin, outDim and averaged under smooth border weights.  views are direct FloatBuffers (or, u16, direct
	 * ShortBuffers) of the extents in dims (3 longs per view); m12 a direct DoubleBuffer of 12 doubles per view; fused a direct
	 * FloatBuffer of prod(outDim) floats; sumWeights (or null) the same; status (or null) a direct IntBuffer of one int per view
	 * (1: the matrix is singular or not finite, the view is absent).  The shim checks every length first.
	 */
	static native void fuseViews( long ctx, java.nio.Buffer[] views, boolean u16, long[] dims, java.nio.DoubleBuffer m12, long[] outMin,
			long[] outDim, double blendX, double blendY, double blendZ, float background, FloatBuffer fused, FloatBuffer sumWeights,
			java.nio.IntBuffer status );

	/**
	 * Aligned views (mvsim_align_views): one resampled volume and one weight volume per view, what normalizeWeights and deconvolve
	 * take.  aligned: direct FloatBuffers of prod(outDim) floats, entries may be null; weights: null, or the same.
	 */
	static native void alignViews( long ctx, java.nio.Buffer[] views, boolean u16, long[] dims, java.nio.DoubleBuffer m12, long[] outMin,
			long[] outDim, double blendX, double blendY, double blendZ, FloatBuffer[] aligned, FloatBuffer[] weights,
			java.nio.IntBuffer status );

	/**
	 * mvsim_extract_psf: the PSF of one view from its beads (include/mvsim.h states the recipe).  img: a direct Float- or (u16)
	 * ShortBuffer of prod(dim) voxels; pos: 3 n doubles; use (or null): n bytes; m12 (or null: the identity): 12 doubles, view to
	 * output frame; psf: prod(kdim) floats; result: at least 72 bytes for one mvsim_psf_result in native byte order; status (or
	 * null): max(n, 1) bytes.  Returns the number of beads used.
	 */
	static native long extractPsf( long ctx, java.nio.Buffer img, boolean u16, long[] dim, java.nio.DoubleBuffer pos, long n,
			java.nio.ByteBuffer use, java.nio.DoubleBuffer m12, long[] kdim, double sepX, double sepY, double sepZ, boolean subtractMin,
			boolean normalize, FloatBuffer psf, java.nio.ByteBuffer result, java.nio.ByteBuffer status );

	/** Fused loop body of SimulateMultiViewDataset.main (:570-585); rot/att/con may be null (then they never leave HBM). */
	static native double simulateView( long ctx, FloatBuffer gt, long[] dim, FloatBuffer psf, long[] kdim,
			int axis, int degrees, double delta, float minValue, float targetAverage, int inc, float snr, long seed, int stream,
			FloatBuffer rot, FloatBuffer att, FloatBuffer con, FloatBuffer acq );

	/** mvsim_simulate_view_async: returns a ticket at once; gt, psf and acq must stay reachable and untouched until waitView. */
	static native long simulateViewAsync( long ctx, FloatBuffer gt, long gtGeneration, long[] dim, FloatBuffer psf, long[] kdim,
			int axis, int degrees, double delta, float minValue, float targetAverage, int inc, float snr, long seed, int stream, FloatBuffer acq );
	/** mvsim_wait: blocks until the view has landed; returns the adjustImage factor. */
	static native double waitView( long ctx, long ticket );
	/** mvsim_wait without exceptions (cleanup paths). */
	static native void waitViewQuiet( long ctx, long ticket );

	// ---- one JVM process driving several GPUs: mvsim_group_* (GpuGroup) ----
	static native long groupCreate( int ndev );
	static native void groupDestroy( long group );
	static native void groupBroadcastVolume( long group, FloatBuffer gt, long[] dim );
	/** dim = the dimensions given to groupBroadcastVolume: the shim checks every acquisition buffer against them */
	/** mvsim_simulate_views: all views of one ground truth in ONE native call (stacked kernels for views that cannot fill the chip) */
	static native void simulateViewsBatch( long ctx, FloatBuffer gt, long[] dim, FloatBuffer[] psfs, long[] kdim, int[] degrees, double delta,
			float minValue, float targetAverage, int inc, float snr, long[] seeds, FloatBuffer[] acqs );

	static native void groupSimulateViews( long group, FloatBuffer[] psfs, long[] kdim, long[] dim, int[] degrees, double delta, float minValue,
			float targetAverage, int inc, float snr, long[] seeds, FloatBuffer[] acqs );
}
