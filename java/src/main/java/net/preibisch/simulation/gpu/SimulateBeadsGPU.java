package net.preibisch.simulation.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.DoubleBuffer;
import java.nio.FloatBuffer;
import java.nio.ShortBuffer;
import java.util.ArrayList;
import java.util.List;
import java.util.Random;

import net.imglib2.Interval;
import net.imglib2.img.Img;
import net.imglib2.img.array.ArrayImg;
import net.imglib2.img.array.ArrayImgs;
import net.imglib2.img.basictypeaccess.array.FloatArray;
import net.imglib2.realtransform.AffineTransform3D;
import net.imglib2.type.numeric.integer.UnsignedShortType;
import net.imglib2.type.numeric.real.FloatType;
import net.preibisch.simulation.SimulateBeads;
import net.preibisch.simulation.SimulateMultiViewDataset;
import mpicbg.models.AffineModel3D;

/**
 * GPU form of {@link SimulateBeads} / {@code SimulateBeads2}: the points come from the reference's own
 * {@code SimulateBeads.randomPoints} (same {@code new Random(535)} stream), the transforms are composed by the real ImgLib2 /
 * mpicbg classes inside the JVM, and only the final 3x4 matrices cross to {@code MvsimNative.renderBeads}, which renders every view
 * in one call (beads.hip: binned by brick, summed in bead order, bit for bit the reference's float sums).
 * SOURCE ONLY: never compiled here (no JDK); the native half is exercised through a fake JNIEnv (tests/test_beads_jni.py).
 */
public class SimulateBeadsGPU
{
	final long ctx;

	public SimulateBeadsGPU( final long ctx ) { this.ctx = ctx; }

	/** SimulateBeads.getImgs(): one float image per angle of axisRotation(rangeSimulation, axis, angle). */
	public ArrayList< Img< FloatType > > getImgs( final int[] angles, final int axis, final int numPoints, final Interval rangeSimulation,
			final Interval intervalRender, final double[] sigma )
	{
		final ArrayList< double[] > points = SimulateBeads.randomPoints( numPoints, rangeSimulation, new Random( 535 ) );
		final double[][] m = new double[ angles.length ][];
		for ( int a = 0; a < angles.length; ++a )
		{
			final AffineModel3D t = SimulateMultiViewDataset.axisRotation( rangeSimulation, axis, angles[ a ] );
			m[ a ] = t.getMatrix( null );   // m00 .. m23, row-major
		}
		return render( points, null, m, intervalRender, sigma );
	}

	/** SimulateBeads2.getImg equivalent: the composed transform of one view. */
	public Img< FloatType > getImg( final List< double[] > points, final AffineTransform3D transform, final Interval intervalRender,
			final double[] sigma )
	{
		final double[][] m = { transform.getRowPackedCopy() };
		return render( points, null, m, intervalRender, sigma ).get( 0 );
	}

	/** SimulateBeads.renderPoints(lists, interval, sigma): lists that are already transformed. */
	public ArrayList< Img< FloatType > > renderPoints( final List< ? extends List< double[] > > lists, final Interval interval, final double[] sigma )
	{
		final ArrayList< double[] > all = new ArrayList<>();
		final long[] offsets = new long[ lists.size() + 1 ];
		for ( int v = 0; v < lists.size(); ++v )
		{
			all.addAll( lists.get( v ) );
			offsets[ v + 1 ] = all.size();
		}
		final ArrayList< Img< FloatType > > imgs = render( all, offsets, null, interval, sigma );
		for ( final List< double[] > list : lists )   // isInsideAdjust's side effect on the caller's points
			for ( final double[] p : list )
				for ( int d = 0; d < 3; ++d )
				{
					p[ d ] -= interval.min( d );
					if ( p[ d ] < 0 || p[ d ] > interval.dimension( d ) - 1 )
						break;
				}
		return imgs;
	}

	/** LegacySimulatedBeadsImgLoader2.getImage equivalent: uint16 written by the kernel (Math.round, low 16 bits). */
	public Img< UnsignedShortType > getImage( final List< double[] > points, final AffineTransform3D transform, final Interval intervalRender,
			final double[] sigma )
	{
		final long[] dim = dims( intervalRender );
		final int nv = ( int ) ( dim[ 0 ] * dim[ 1 ] * dim[ 2 ] );
		final ShortBuffer out = ByteBuffer.allocateDirect( 2 * nv ).order( ByteOrder.nativeOrder() ).asShortBuffer();
		MvsimNative.renderBeads( ctx, pointBuffer( points ), points.size(), null, matrixBuffer( new double[][] { transform.getRowPackedCopy() } ), 1,
				interval( intervalRender ), sigma[ 0 ], sigma[ 1 ], sigma[ 2 ], null, new ShortBuffer[] { out } );
		final short[] s = new short[ nv ];
		out.get( s );
		return ArrayImgs.unsignedShorts( s, dim );
	}

	ArrayList< Img< FloatType > > render( final List< double[] > points, final long[] offsets, final double[][] m, final Interval interval,
			final double[] sigma )
	{
		final long[] dim = dims( interval );
		final int nv = ( int ) ( dim[ 0 ] * dim[ 1 ] * dim[ 2 ] );
		final int nviews = m != null ? m.length : offsets.length - 1;
		final FloatBuffer[] out = new FloatBuffer[ nviews ];
		for ( int v = 0; v < nviews; ++v )
			out[ v ] = ByteBuffer.allocateDirect( 4 * nv ).order( ByteOrder.nativeOrder() ).asFloatBuffer();
		MvsimNative.renderBeads( ctx, pointBuffer( points ), points.size(), offsets, m == null ? null : matrixBuffer( m ), nviews,
				interval( interval ), sigma[ 0 ], sigma[ 1 ], sigma[ 2 ], out, null );
		final ArrayList< Img< FloatType > > imgs = new ArrayList<>();
		for ( int v = 0; v < nviews; ++v )
		{
			final float[] f = new float[ nv ];
			out[ v ].get( f );
			final ArrayImg< FloatType, FloatArray > img = ArrayImgs.floats( f, dim );
			imgs.add( img );
		}
		return imgs;
	}

	static long[] dims( final Interval interval )
	{
		// SimulateBeads.java:105-106: one voxel less than the interval per axis
		return new long[] { interval.max( 0 ) - interval.min( 0 ), interval.max( 1 ) - interval.min( 1 ), interval.max( 2 ) - interval.min( 2 ) };
	}

	static long[] interval( final Interval interval )
	{
		return new long[] { interval.min( 0 ), interval.min( 1 ), interval.min( 2 ), interval.max( 0 ), interval.max( 1 ), interval.max( 2 ) };
	}

	static DoubleBuffer pointBuffer( final List< double[] > points )
	{
		final DoubleBuffer b = ByteBuffer.allocateDirect( Math.max( 8, 24 * points.size() ) ).order( ByteOrder.nativeOrder() ).asDoubleBuffer();
		for ( final double[] p : points )
			b.put( p[ 0 ] ).put( p[ 1 ] ).put( p[ 2 ] );
		b.rewind();
		return b;
	}

	static DoubleBuffer matrixBuffer( final double[][] m )
	{
		final DoubleBuffer b = ByteBuffer.allocateDirect( 96 * m.length ).order( ByteOrder.nativeOrder() ).asDoubleBuffer();
		for ( final double[] r : m )
			b.put( r, 0, 12 );
		b.rewind();
		return b;
	}
}
