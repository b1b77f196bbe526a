package net.preibisch.simulation.gpu;

import java.nio.Buffer;
import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.DoubleBuffer;
import java.nio.FloatBuffer;
import java.nio.IntBuffer;
import java.util.List;

/**
 * The consumer of the transforms that {@link InterestPointRegistrationGPU} returns: every view is resampled through its affine
 * into one output interval on the GPU (mvsim_fuse_views / mvsim_align_views; include/mvsim.h states the recipe) and either averaged
 * under smooth border weights or handed back aligned, with its weight volume -- what {@link MultiViewDeconvolutionGPU} takes.  The
 * reference has no fusion.
 *
 * <pre>
 * final ViewFusionGPU fusion = new ViewFusionGPU();
 * fusion.blend = new double[] { 8, 8, 8 };
 * final float[] fused = fusion.fuse( views, dims, matrices, outMin, outDim ).volume;   // matrices.get( v ): 3 x 4 row-major, view to output
 * </pre>
 *
 * Volumes are x fastest; dims, outMin and outDim are { x, y, z }.
 */
public class ViewFusionGPU
{
	/** status of a view whose matrix is singular or not finite: the view is absent */
	public static final int SINGULAR = 1;
	/** most views per call */
	public static final int MAX_VIEWS = 32;

	public static class Fused
	{
		public float[] volume;
		/** the sum of the views' weights per voxel */
		public float[] sumWeights;
		/** one word per view: 0 or {@link #SINGULAR} */
		public int[] status;
	}

	public static class Aligned
	{
		public float[][] views, weights;
		public int[] status;
	}

	/** width of the smooth ramp from every face of a view, voxels per axis; 0: weight 1 everywhere inside */
	public double[] blend = new double[] { 8.0, 8.0, 8.0 };
	/** value of the fused volume where no view has weight */
	public float background = 0.0f;

	public Fused fuse( final List< float[] > views, final List< long[] > dims, final List< double[] > matrices, final long[] outMin, final long[] outDim )
	{
		final int n = check( views, dims, matrices, outMin, outDim );
		final int voxels = voxels( outDim );
		final FloatBuffer out = floats( voxels ), sum = floats( voxels );
		final IntBuffer status = ByteBuffer.allocateDirect( 4 * n ).order( ByteOrder.nativeOrder() ).asIntBuffer();
		MvsimNative.fuseViews( GpuContextPool.get(), pack( views, dims ), false, flat( dims ), pack( matrices ), outMin, outDim, blend[ 0 ], blend[ 1 ],
				blend[ 2 ], background, out, sum, status );
		final Fused f = new Fused();
		f.volume = new float[ voxels ];
		f.sumWeights = new float[ voxels ];
		f.status = new int[ n ];
		out.get( f.volume );
		sum.get( f.sumWeights );
		status.get( f.status );
		return f;
	}

	public Aligned align( final List< float[] > views, final List< long[] > dims, final List< double[] > matrices, final long[] outMin, final long[] outDim )
	{
		final int n = check( views, dims, matrices, outMin, outDim );
		final int voxels = voxels( outDim );
		final FloatBuffer[] al = new FloatBuffer[ n ], wt = new FloatBuffer[ n ];
		for ( int v = 0; v < n; ++v )
		{
			al[ v ] = floats( voxels );
			wt[ v ] = floats( voxels );
		}
		final IntBuffer status = ByteBuffer.allocateDirect( 4 * n ).order( ByteOrder.nativeOrder() ).asIntBuffer();
		MvsimNative.alignViews( GpuContextPool.get(), pack( views, dims ), false, flat( dims ), pack( matrices ), outMin, outDim, blend[ 0 ], blend[ 1 ],
				blend[ 2 ], al, wt, status );
		final Aligned a = new Aligned();
		a.views = new float[ n ][ voxels ];
		a.weights = new float[ n ][ voxels ];
		a.status = new int[ n ];
		for ( int v = 0; v < n; ++v )
		{
			al[ v ].get( a.views[ v ] );
			wt[ v ].get( a.weights[ v ] );
		}
		status.get( a.status );
		return a;
	}

	private static int check( final List< float[] > views, final List< long[] > dims, final List< double[] > matrices, final long[] outMin, final long[] outDim )
	{
		if ( views == null || dims == null || matrices == null || outMin == null || outDim == null || outMin.length < 3 || outDim.length < 3 )
			throw new IllegalArgumentException( "views, their sizes, their matrices and an output interval expected" );
		final int n = views.size();
		if ( n < 1 || n > MAX_VIEWS || dims.size() != n || matrices.size() != n )
			throw new IllegalArgumentException( "1 .. " + MAX_VIEWS + " views with one size and one matrix each" );
		return n;
	}

	private static int voxels( final long[] d )
	{
		final long v = d[ 0 ] * d[ 1 ] * d[ 2 ];
		if ( d[ 0 ] < 1 || d[ 1 ] < 1 || d[ 2 ] < 1 || v > Integer.MAX_VALUE / 4 )
			throw new IllegalArgumentException( "an interval of 1 .. 2^29 - 1 voxels expected" );
		return ( int ) v;
	}

	private static FloatBuffer floats( final int n )
	{
		return ByteBuffer.allocateDirect( 4 * n ).order( ByteOrder.nativeOrder() ).asFloatBuffer();
	}

	private static Buffer[] pack( final List< float[] > views, final List< long[] > dims )
	{
		final Buffer[] out = new Buffer[ views.size() ];
		for ( int v = 0; v < out.length; ++v )
		{
			final float[] a = views.get( v );
			final long[] d = dims.get( v );
			if ( a == null || d == null || d.length < 3 || a.length < voxels( d ) )
				throw new IllegalArgumentException( "view " + v + " is smaller than its size" );
			final FloatBuffer b = floats( a.length );
			b.put( a );
			b.rewind();
			out[ v ] = b;
		}
		return out;
	}

	private static long[] flat( final List< long[] > dims )
	{
		final long[] out = new long[ 3 * dims.size() ];
		for ( int v = 0; v < dims.size(); ++v )
			System.arraycopy( dims.get( v ), 0, out, 3 * v, 3 );
		return out;
	}

	private static DoubleBuffer pack( final List< double[] > matrices )
	{
		final DoubleBuffer buf = ByteBuffer.allocateDirect( 96 * matrices.size() ).order( ByteOrder.nativeOrder() ).asDoubleBuffer();
		for ( int v = 0; v < matrices.size(); ++v )
		{
			final double[] m = matrices.get( v );
			if ( m == null || m.length < 12 )
				throw new IllegalArgumentException( "every matrix is 3 x 4, row-major" );
			for ( int k = 0; k < 12; ++k )
				buf.put( 12 * v + k, m[ k ] );
		}
		return buf;
	}
}
