package net.preibisch.simulation.gpu;

import java.nio.FloatBuffer;
import java.util.Random;
import java.util.concurrent.ExecutorService;

import net.imglib2.img.Img;
import net.imglib2.type.numeric.real.FloatType;
import net.imglib2.util.Pair;
import net.imglib2.util.ValuePair;

/**
 * Drop-in for net.preibisch.simulation.SimulateTileStitching: the same constructors and the same getNextPair / getCorrectTranslation /
 * getInterval, with the two convolved phantoms kept in HBM.  init runs the facade's operators (simulate, attenuate3d, convolve,
 * adjustImage) and uploads the two volumes once; every getNextPair is then ONE native call, mvsim_extract_intervals with two jobs --
 * Views.zeroMin( Views.interval( con, min, max ) ) through extractSlices without a tile ever being copied on the host.  The tiles'
 * seeds are drawn as the reference draws them: rnd.nextInt() twice, then nextLong() of new Random( seedN ) for a sampled tile.
 *
 * The object owns device memory: close() it (try-with-resources).
 *
 * SOURCE ONLY in this repository (no JDK in the build image): never compiled or run here.  The native half, MvsimNative.extractIntervals,
 * runs against a fake JNIEnv in tests/test_intervals_jni.py.
 */
public class SimulateTileStitchingGPU implements AutoCloseable
{
	final ExecutorService service;
	final int lightsheetSpacing = 3;
	final float attenuation = 0.01f;
	final Random rnd;
	final Img< FloatType > psf;

	boolean halfPixelOffset;
	int[] overlap;
	final long[] dim = new long[ 3 ];
	long[] min, max;
	private long ctx, con, conHalfPixel;

	public SimulateTileStitchingGPU( final Img< FloatType > psf, final boolean halfPixelOffset, final double[] overlapRatio, final ExecutorService service )
	{
		this( psf, null, halfPixelOffset, overlapRatio, service );
	}

	/** psf: what the reference reads with Tools.open( dir + "Angle0.tif", true ); it is normalised in place, as there. */
	public SimulateTileStitchingGPU( final Img< FloatType > psf, final Random rnd, final boolean halfPixelOffset, final double[] overlapRatio,
			final ExecutorService service )
	{
		this.rnd = rnd == null ? new Random( 464232194 ) : rnd;
		this.service = service;
		this.psf = psf;
		init( overlapRatio, halfPixelOffset );
	}

	private long rendered( final boolean half, final int seed )
	{
		final Img< FloatType > groundTruth = SimulateMultiViewDatasetGPU.simulate( half, new Random( seed ) );
		final Img< FloatType > att = SimulateMultiViewDatasetGPU.attenuate3d( groundTruth, attenuation );
		final Img< FloatType > c = SimulateMultiViewDatasetGPU.convolve( att, psf, service );
		ToolsGPU.adjustImage( c, SimulateMultiViewDatasetGPU.minValue, SimulateMultiViewDatasetGPU.avgIntensity );
		c.dimensions( dim );
		final long n = Buffers.size( dim );
		final long d = MvsimNative.devAlloc( ctx, 4 * n );
		try ( Buffers.Block blk = Buffers.toBlock( c ) )
		{
			MvsimNative.uploadFloats( ctx, d, blk.floats, n );
		}
		catch ( final RuntimeException e )
		{
			MvsimNative.devFree( ctx, d );
			throw e;
		}
		return d;
	}

	public void init( final double[] overlapRatio, final boolean halfPixelOffset )
	{
		close();
		this.halfPixelOffset = halfPixelOffset;
		this.ctx = GpuContextPool.get();
		final int seed = rnd.nextInt(); // the same phantom with and without the half-pixel shift
		this.con = rendered( false, seed );
		this.conHalfPixel = rendered( true, seed );

		this.overlap = new int[ 3 ];
		for ( int d = 0; d < 3; ++d )
			this.overlap[ d ] = ( int ) Math.round( dim[ d ] * overlapRatio[ d ] / 2 );
		this.min = new long[ 3 ];
		this.max = new long[ 3 ];
	}

	public Pair< Img< FloatType >, Img< FloatType > > getNextPair( final float snr )
	{
		if ( con == 0 )
			throw new IllegalStateException( "SimulateTileStitchingGPU: closed" );
		final int seed0 = rnd.nextInt();
		final int seed1 = rnd.nextInt();
		final long[] geometry = new long[ 20 ];
		final long[][] out = new long[ 2 ][];
		for ( int tile = 0; tile < 2; ++tile )
		{
			final long[] lo = new long[ 3 ], hi = new long[ 3 ];
			getInterval( lo, hi, tile );
			geometry[ 10 * tile ] = tile == 1 && halfPixelOffset ? conHalfPixel : con;
			for ( int d = 0; d < 3; ++d )
			{
				geometry[ 10 * tile + 1 + d ] = dim[ d ];
				geometry[ 10 * tile + 4 + d ] = lo[ d ];
				geometry[ 10 * tile + 7 + d ] = hi[ d ];
			}
			out[ tile ] = new long[] { hi[ 0 ] - lo[ 0 ] + 1, hi[ 1 ] - lo[ 1 ] + 1, ( hi[ 2 ] - lo[ 2 ] ) / lightsheetSpacing + 1 };
		}
		// as extractSlices draws it: one nextLong() of the tile's own generator, for a sampled tile only
		final long[] seeds = { snr >= 0.0 ? new Random( seed0 ).nextLong() : 0L, snr >= 0.0 ? new Random( seed1 ).nextLong() : 0L };
		try ( Buffers.Block b0 = Buffers.direct( Buffers.size( out[ 0 ] ) ); Buffers.Block b1 = Buffers.direct( Buffers.size( out[ 1 ] ) ) )
		{
			MvsimNative.extractIntervals( ctx, geometry, new int[] { lightsheetSpacing, lightsheetSpacing }, new float[] { snr, snr }, seeds,
					new int[] { 0, 0 }, new FloatBuffer[] { b0.floats, b1.floats } );
			return new ValuePair<>( Buffers.toImg( b0, out[ 0 ] ), Buffers.toImg( b1, out[ 1 ] ) );
		}
	}

	public double[] getCorrectTranslation()
	{
		final double[] translation = new double[ 3 ];
		getInterval( min, max, 1 );
		for ( int d = 0; d < 3; ++d )
			translation[ d ] = min[ d ];
		if ( halfPixelOffset )
		{
			// the right tile's content sits half a pixel further right, so it has to move half a pixel less to the left
			translation[ 0 ] -= 0.5;
			translation[ 1 ] -= 0.5;
		}
		translation[ 2 ] /= lightsheetSpacing;
		return translation;
	}

	/** Inclusive corners of tile 0 / 1 (mvsim_tile_interval): tile 1 starts at dimension( 0 ) / 2 - overlap in EVERY dimension, as the reference has it. */
	protected void getInterval( final long[] min, final long[] max, final int tile )
	{
		for ( int d = 0; d < 3; ++d )
		{
			min[ d ] = 0;
			max[ d ] = dim[ d ] - 1;
			if ( tile == 0 )
				max[ d ] = ( int ) dim[ d ] / 2 + overlap[ d ];
			else
				min[ d ] = ( int ) dim[ 0 ] / 2 - overlap[ d ];
		}
	}

	@Override
	public void close()
	{
		if ( con != 0 )
			MvsimNative.devFree( ctx, con );
		if ( conHalfPixel != 0 )
			MvsimNative.devFree( ctx, conHalfPixel );
		con = conHalfPixel = 0;
	}
}
