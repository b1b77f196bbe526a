package net.preibisch.simulation.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.util.ArrayList;
import java.util.List;

import net.imglib2.RandomAccessibleInterval;
import net.imglib2.type.numeric.real.FloatType;

/**
 * The consumer of the bead images that SimulateBeads and SimulateBeads2 render: difference-of-Gaussian interest points with a
 * quadratic sub-voxel fit, on the GPU (mvsim_detect_beads; include/mvsim.h states the recipe).  The reference has no detector;
 * its imgloader classes hand the bead images to a pipeline that detects beads, matches them across views and registers the views.
 *
 * <pre>
 * final InterestPointDetectionGPU det = new InterestPointDetectionGPU();
 * det.threshold = 5f;
 * final List&lt; InterestPointDetectionGPU.Peak &gt; peaks = det.detect( img );
 * </pre>
 *
 * The detections come in ascending order of their peak voxels.  More than {@link #capacity} detections are counted
 * ({@link #lastFound}) but only the first {@link #capacity} are returned.
 */
public class InterestPointDetectionGPU
{
	/** flags of a detection */
	public static final int SINGULAR = 1, FROZEN = 2, CAPPED = 4;

	/** one detection: the sub-voxel position (x, y, z), the interpolated DoG value, the flags and the final base voxel */
	public static class Peak
	{
		public final double[] pos;
		public final float value;
		public final int flags;
		public final long voxel;

		Peak( final double[] pos, final float value, final int flags, final long voxel )
		{
			this.pos = pos;
			this.value = value;
			this.flags = flags;
			this.voxel = voxel;
		}
	}

	/** the smaller sigma per axis; the larger one is sigma * 2^(1/4) unless {@link #sigma2} is set */
	public double[] sigma = new double[] { 1.8, 1.8, 1.8 };
	/** the larger sigma per axis, or null */
	public double[] sigma2 = null;
	/** the usual proposal for images normalised to [0, 1] */
	public float threshold = 0.008f;
	/** rounds of base-voxel moves of the sub-voxel fit */
	public int maxMoves = 4;
	/** most detections returned by one call */
	public int capacity = 1 << 16;
	/** what the last call found, which may be more than it returned */
	public long lastFound = 0;

	public List< Peak > detect( final RandomAccessibleInterval< FloatType > img )
	{
		if ( sigma == null || sigma.length != 3 || ( sigma2 != null && sigma2.length != 3 ) )
			throw new IllegalArgumentException( "sigma and sigma2 must have three entries (x, y, z)" );
		if ( capacity < 1 )
			throw new IllegalArgumentException( "capacity must be >= 1" );
		final double f = Math.pow( 2.0, 0.25 );
		final double[] s2 = sigma2 != null ? sigma2 : new double[] { sigma[ 0 ] * f, sigma[ 1 ] * f, sigma[ 2 ] * f };
		final long[] d = Buffers.dims( img );
		final ByteBuffer out = ByteBuffer.allocateDirect( 40 * capacity ).order( ByteOrder.nativeOrder() );
		final Buffers.Block b = Buffers.toBlock( img );
		try
		{
			lastFound = MvsimNative.detectBeads( GpuContextPool.get(), b.floats, false, d, sigma[ 0 ], sigma[ 1 ], sigma[ 2 ], s2[ 0 ], s2[ 1 ], s2[ 2 ],
					threshold, maxMoves, capacity, out );
		}
		finally
		{
			b.close();
		}
		final int n = ( int ) Math.min( lastFound, capacity );
		final List< Peak > peaks = new ArrayList<>( n );
		for ( int i = 0; i < n; ++i )
		{
			final int at = 40 * i;
			peaks.add( new Peak( new double[] { out.getDouble( at ), out.getDouble( at + 8 ), out.getDouble( at + 16 ) }, out.getFloat( at + 24 ),
					out.getInt( at + 28 ), out.getLong( at + 32 ) ) );
		}
		return peaks;
	}
}
