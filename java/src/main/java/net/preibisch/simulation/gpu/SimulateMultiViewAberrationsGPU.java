package net.preibisch.simulation.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.FloatBuffer;

import net.imglib2.Cursor;
import net.imglib2.RandomAccessibleInterval;
import net.imglib2.img.Img;
import net.imglib2.img.array.ArrayImgs;
import net.imglib2.type.numeric.real.FloatType;
import net.imglib2.util.Pair;
import net.imglib2.util.ValuePair;
import net.imglib2.view.Views;

/**
 * GPU form of {@code SimulateMultiViewAberrations.refract3d}, {@code projectToCamera}, {@code multiSpheres} and
 * {@code simulate( rnd, dir )} (with the canvas of block4.tif passed in): the volumes cross to
 * {@code MvsimNative} as direct buffers, the rays are traced, injected and summed by the kernels of aberrations.hip.  The random
 * streams are the reference's -- {@code new Random(2423)} per refract3d call, one {@code Random(464232194)} shared by the
 * projectToCamera calls of this object -- kept as the 48-bit generator state the native side jumps ahead.
 * SOURCE ONLY: never compiled here (no JDK); the native half is exercised through a fake JNIEnv (tests/test_aberrations_jni.py).
 */
public class SimulateMultiViewAberrationsGPU
{
	static final long MULT = 0x5DEECE66DL, MASK = ( 1L << 48 ) - 1;

	final long ctx;
	final long[] cameraState = { ( 464232194L ^ MULT ) & MASK };   // SimulateMultiViewAberrations.java:78

	public SimulateMultiViewAberrationsGPU( final long ctx ) { this.ctx = ctx; }

	/** refract3d (:261-401): the image and weight volumes of the returned VolumeInjection, 200 000 rays. */
	public Pair< Img< FloatType >, Img< FloatType > > refract3d( final RandomAccessibleInterval< FloatType > imgIn,
			final RandomAccessibleInterval< FloatType > imgRi, final boolean illum, final int z, final double lsMiddle, final double lsEdge,
			final double ri )
	{
		return refract3d( imgIn, imgRi, illum, z, lsMiddle, lsEdge, ri, 200000 );
	}

	public Pair< Img< FloatType >, Img< FloatType > > refract3d( final RandomAccessibleInterval< FloatType > imgIn,
			final RandomAccessibleInterval< FloatType > imgRi, final boolean illum, final int z, final double lsMiddle, final double lsEdge,
			final double ri, final long numRays )
	{
		final long[] dim = dims( imgIn );
		final int n = ( int ) ( dim[ 0 ] * dim[ 1 ] * dim[ 2 ] );
		final FloatBuffer image = direct( n ), weight = direct( n );
		final long[] state = { ( 2423L ^ MULT ) & MASK };            // :305
		MvsimNative.refract3d( ctx, toBuffer( imgIn ), toBuffer( imgRi ), dim, illum, z, lsMiddle, lsEdge, ri, numRays, state, image, weight );
		return new ValuePair<>( toImg( image, dim ), toImg( weight, dim ) );
	}

	/** projectToCamera (:89-254); {@code ri} is accepted and unused, as in the reference (:117). */
	public Img< FloatType > projectToCamera( final RandomAccessibleInterval< FloatType > imgRi, final RandomAccessibleInterval< FloatType > refr,
			final double ri, final int currentzPlane )
	{
		final long[] dim = dims( imgRi );
		final FloatBuffer proj = direct( ( int ) ( dim[ 0 ] * dim[ 1 ] ) );
		MvsimNative.projectToCamera( ctx, toBuffer( imgRi ), toBuffer( refr ), dim, currentzPlane, 500, cameraState, proj );
		return toImg( proj, new long[] { dim[ 0 ], dim[ 1 ] } );
	}

	/**
	 * multiSpheres (:474-586), in place on both images, with the reference's hard-coded ranges.  The generator is a {@link GpuRandom}:
	 * its 48-bit state crosses the boundary, the native library walks the large sphere (on the GPU by default) and hands the state back
	 * advanced exactly as the reference advances its java.util.Random.  Returns the number of small spheres drawn.
	 */
	public long multiSpheres( final Img< FloatType > image, final Img< FloatType > ri, final int scale, final GpuRandom rnd )
	{
		final long[] dim = dims( image );
		final FloatBuffer bi = toBuffer( image ), br = toBuffer( ri );
		final long[] state = { rnd.getState() };
		final long n = MvsimNative.multiSpheres( ctx, bi, br, dim, scale, state );
		rnd.setState( state[ 0 ] );
		copyBack( bi, image );
		copyBack( br, ri );
		return n;
	}

	/**
	 * simulate( rnd, dir ) (:408-440) behind its Tools.open: {@code ri} is the canvas of refractive indices the reference reads from
	 * block4.tif (not shipped; 580^3 there).  Noise on the canvas, multiSpheres on a zero image and the canvas, both down-sampled 2x.
	 */
	public Pair< Img< FloatType >, Img< FloatType > > simulate( final GpuRandom rnd, final RandomAccessibleInterval< FloatType > ri )
	{
		final int scale = 2;
		final long[] dim = dims( ri );
		final int n = ( int ) ( dim[ 0 ] * dim[ 1 ] * dim[ 2 ] );
		final FloatBuffer bi = direct( n ), br = toBuffer( ri );
		final long[] state = { rnd.getState() };
		MvsimNative.riNoise( ctx, br, n, state );
		MvsimNative.multiSpheres( ctx, bi, br, dim, scale, state );
		rnd.setState( state[ 0 ] );
		final long[] o = { dim[ 0 ] / 2 - 1, dim[ 1 ] / 2 - 1, dim[ 2 ] / 2 - 1 };
		final FloatBuffer oi = direct( ( int ) ( o[ 0 ] * o[ 1 ] * o[ 2 ] ) ), or = direct( ( int ) ( o[ 0 ] * o[ 1 ] * o[ 2 ] ) );
		MvsimNative.downSample2x( ctx, bi, dim, oi );
		MvsimNative.downSample2x( ctx, br, dim, or );
		return new ValuePair<>( toImg( oi, o ), toImg( or, o ) );
	}

	static void copyBack( final FloatBuffer b, final Img< FloatType > img )
	{
		b.rewind();
		final Cursor< FloatType > c = Views.flatIterable( img ).cursor();
		while ( c.hasNext() )
			c.next().set( b.get() );
	}

	static long[] dims( final RandomAccessibleInterval< FloatType > img )
	{
		return new long[] { img.dimension( 0 ), img.dimension( 1 ), img.dimension( 2 ) };
	}

	static FloatBuffer direct( final int n )
	{
		return ByteBuffer.allocateDirect( 4 * n ).order( ByteOrder.nativeOrder() ).asFloatBuffer();
	}

	static FloatBuffer toBuffer( final RandomAccessibleInterval< FloatType > img )
	{
		final long[] dim = dims( img );
		final FloatBuffer b = direct( ( int ) ( dim[ 0 ] * dim[ 1 ] * dim[ 2 ] ) );
		final Cursor< FloatType > c = Views.flatIterable( img ).cursor();
		while ( c.hasNext() )
			b.put( c.next().get() );
		b.rewind();
		return b;
	}

	static Img< FloatType > toImg( final FloatBuffer b, final long[] dim )
	{
		final float[] f = new float[ b.capacity() ];
		b.rewind();
		b.get( f );
		return ArrayImgs.floats( f, dim );
	}
}
