package net.preibisch.simulation.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.DoubleBuffer;
import java.nio.FloatBuffer;

/**
 * The link between {@link InterestPointRegistrationGPU} and {@link MultiViewDeconvolutionGPU}: the beads of one view are averaged into
 * that view's PSF on the GPU (mvsim_extract_psf; include/mvsim.h states the recipe), sampled through the inverse of the view's
 * registration so that the PSF comes out in the output frame.  The reference has no PSF extraction.
 *
 * <pre>
 * final PsfExtractionGPU extraction = new PsfExtractionGPU();
 * extraction.kdim = new long[] { 15, 15, 21 };
 * final float[] psf = extraction.extract( view, dim, positions, null, matrix ).psf;   // matrix: 3 x 4 row-major, view to output, or null
 * </pre>
 *
 * Volumes are x fastest; dim and kdim are { x, y, z }; positions are { x0, y0, z0, x1, ... } in voxels.
 */
public class PsfExtractionGPU
{
	/** status bytes of the listed beads */
	public static final int USED = 0, NONFINITE = 1, MASKED = 2, OUTSIDE = 3, CROWDED = 4;
	/** flags of the result */
	public static final int SINGULAR = 1, NO_BEADS = 2, FLAT = 4;
	/** most beads per call, largest PSF extent */
	public static final int MAX_POINTS = 65536, MAX_DIM = 63;

	public static class Psf
	{
		public float[] psf;
		/** one byte per listed bead: {@link #USED} ... {@link #CROWDED}; all zero when {@link #SINGULAR} is set */
		public byte[] status;
		/** the smallest mean that was subtracted, and the sum the PSF was divided by */
		public double minimum, sum;
		public long nListed, nUsed, nNonfinite, nMasked, nOutside, nCrowded;
		public int flags;
	}

	/** extents of the PSF, odd, at most {@link #MAX_DIM} */
	public long[] kdim = new long[] { 15, 15, 15 };
	/** a bead with another listed bead closer than this on all three axes is left out; all zero: no such rule */
	public double[] minSeparation = new double[] { 15.0, 15.0, 15.0 };
	public boolean subtractMin = true, normalize = true;

	public Psf extract( final float[] view, final long[] dim, final double[] positions, final byte[] use, final double[] matrix )
	{
		if ( view == null || dim == null || dim.length < 3 || positions == null || positions.length % 3 != 0 || kdim == null || kdim.length < 3
				|| minSeparation == null || minSeparation.length < 3 )
			throw new IllegalArgumentException( "a view, its size and a list of positions expected" );
		final int n = positions.length / 3;
		final long voxels = dim[ 0 ] * dim[ 1 ] * dim[ 2 ], taps = kdim[ 0 ] * kdim[ 1 ] * kdim[ 2 ];
		if ( dim[ 0 ] < 1 || dim[ 1 ] < 1 || dim[ 2 ] < 1 || voxels > Integer.MAX_VALUE / 4 || view.length < voxels )
			throw new IllegalArgumentException( "a view of 1 .. 2^29 - 1 voxels, no smaller than its size, expected" );
		if ( n > MAX_POINTS || ( use != null && use.length < n ) || ( matrix != null && matrix.length < 12 ) || taps < 1
				|| taps > ( long ) MAX_DIM * MAX_DIM * MAX_DIM )
			throw new IllegalArgumentException( "at most " + MAX_POINTS + " beads, one use byte each, a 3 x 4 matrix and a PSF of at most 63^3 expected" );
		final FloatBuffer img = direct( 4 * ( int ) voxels ).asFloatBuffer();
		img.put( view, 0, ( int ) voxels );
		final DoubleBuffer pos = direct( 24 * Math.max( n, 1 ) ).asDoubleBuffer();
		pos.put( positions );
		ByteBuffer useBuf = null;
		if ( use != null )
		{
			useBuf = direct( Math.max( n, 1 ) );
			useBuf.put( use, 0, n );
		}
		DoubleBuffer m = null;
		if ( matrix != null )
		{
			m = direct( 96 ).asDoubleBuffer();
			m.put( matrix, 0, 12 );
		}
		final FloatBuffer out = direct( 4 * ( int ) taps ).asFloatBuffer();
		final ByteBuffer result = direct( 72 ), status = direct( Math.max( n, 1 ) );
		MvsimNative.extractPsf( GpuContextPool.get(), img, false, dim, pos, n, useBuf, m, kdim, minSeparation[ 0 ], minSeparation[ 1 ],
				minSeparation[ 2 ], subtractMin, normalize, out, result, status );
		final Psf p = new Psf();
		p.psf = new float[ ( int ) taps ];
		out.get( p.psf );
		p.status = new byte[ n ];
		status.get( p.status );
		p.minimum = result.getDouble( 0 );
		p.sum = result.getDouble( 8 );
		p.nListed = result.getLong( 16 );
		p.nUsed = result.getLong( 24 );
		p.nNonfinite = result.getLong( 32 );
		p.nMasked = result.getLong( 40 );
		p.nOutside = result.getLong( 48 );
		p.nCrowded = result.getLong( 56 );
		p.flags = result.getInt( 64 );
		return p;
	}

	private static ByteBuffer direct( final int bytes )
	{
		return ByteBuffer.allocateDirect( bytes ).order( ByteOrder.nativeOrder() );
	}
}
