package net.preibisch.simulation.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.DoubleBuffer;
import java.nio.FloatBuffer;

import net.imglib2.RandomAccessibleInterval;
import net.imglib2.img.Img;
import net.imglib2.type.numeric.real.FloatType;
import net.imglib2.util.Pair;
import net.imglib2.util.ValuePair;

/**
 * GPU form of {@code raytracing.RayTracingTest.drawRays} and {@code drawMultipleRays}: the ray starts of the reference's loops, traced
 * by the general tracer of raytrace.hip ({@code MvsimNative.traceRays}) through the raw index image (map (0, 1), threshold 0.01, value
 * 1.0, total reflection keeps the direction) and injected with sigma 0.5.  The reference's loops have no move cap; here a ray makes at
 * most 4 (Nx + Ny + Nz) moves, and a ray still inside after that many is an IllegalStateException, because the result would not be
 * the reference's.
 * SOURCE ONLY: never compiled here (no JDK); the native half is exercised through a fake JNIEnv (tests/test_trace_rays_jni.py).
 */
public class RayTracingTestGPU
{
	final long ctx;

	public RayTracingTestGPU( final long ctx ) { this.ctx = ctx; }

	/** drawRays (:308-415): the image and weight volumes of the returned VolumeInjection. */
	public Pair< Img< FloatType >, Img< FloatType > > drawRays( final RandomAccessibleInterval< FloatType > imgIn, final int z, final int spacing )
	{
		if ( spacing < 1 )
			throw new IllegalArgumentException( "spacing must be >= 1" );
		final long[] dim = SimulateMultiViewAberrationsGPU.dims( imgIn );
		final int n = ( int ) ( dim[ 0 ] / spacing );
		final DoubleBuffer pos = direct( 3 * n ), dir = direct( 3 * n );
		for ( int x = spacing; x <= dim[ 0 ]; x += spacing )      // :334-344
		{
			pos.put( x ).put( dim[ 1 ] - 25 ).put( z );
			dir.put( 0 ).put( -1 ).put( 0 );
		}
		return trace( imgIn, dim, pos, dir, n );
	}

	/** drawMultipleRays (:86-194): numRays rays from new Random( 234345 ) around (x, Ny - 1, z). */
	public Pair< Img< FloatType >, Img< FloatType > > drawMultipleRays( final RandomAccessibleInterval< FloatType > imgIn, final int z, final int x,
			final int numRays )
	{
		final long[] dim = SimulateMultiViewAberrationsGPU.dims( imgIn );
		final DoubleBuffer pos = direct( 3 * numRays ), dir = direct( 3 * numRays );
		final long[] state = { ( 234345L ^ SimulateMultiViewAberrationsGPU.MULT ) & SimulateMultiViewAberrationsGPU.MASK };   // :110
		MvsimNative.sandboxRayStarts( ctx, state, dim, x, z, numRays, pos, dir );
		return trace( imgIn, dim, pos, dir, numRays );
	}

	Pair< Img< FloatType >, Img< FloatType > > trace( final RandomAccessibleInterval< FloatType > imgIn, final long[] dim, final DoubleBuffer pos,
			final DoubleBuffer dir, final long n )
	{
		final int nvox = ( int ) ( dim[ 0 ] * dim[ 1 ] * dim[ 2 ] );
		final FloatBuffer image = SimulateMultiViewAberrationsGPU.direct( nvox ), weight = SimulateMultiViewAberrationsGPU.direct( nvox );
		final long maxMoves = 4 * ( dim[ 0 ] + dim[ 1 ] + dim[ 2 ] );
		final long capped = MvsimNative.traceRays( ctx, SimulateMultiViewAberrationsGPU.toBuffer( imgIn ), null, dim, pos, dir, null, n, 0.0, 1.0,
				0.01, maxMoves, 0, false, 1.0, image, weight );
		if ( capped > 0 )
			throw new IllegalStateException( capped + " rays were still inside the image after " + maxMoves + " moves" );
		return new ValuePair<>( SimulateMultiViewAberrationsGPU.toImg( image, dim ), SimulateMultiViewAberrationsGPU.toImg( weight, dim ) );
	}

	static DoubleBuffer direct( final int n )
	{
		return ByteBuffer.allocateDirect( 8 * Math.max( n, 1 ) ).order( ByteOrder.nativeOrder() ).asDoubleBuffer();
	}
}
