package net.preibisch.simulation.gpu;

import java.nio.FloatBuffer;
import java.util.List;

import net.imglib2.RandomAccessibleInterval;
import net.imglib2.img.Img;
import net.imglib2.type.numeric.real.FloatType;

/**
 * The consumer of what SimulateMultiViewDataset.main writes: a weighted, sequential (OSEM) multi-view Richardson-Lucy
 * deconvolution of the aligned views with their PSFs and normalised weights, on the GPU (mvsim_deconvolve; include/mvsim.h
 * states the recipe).  The reference has no deconvolution; its README names the algorithm the dataset is made for.
 *
 * <pre>
 * final MultiViewDeconvolutionGPU d = new MultiViewDeconvolutionGPU();
 * d.iterations = 10;
 * final Img&lt; FloatType &gt; psi = d.run( views, psfs, weights );
 * </pre>
 *
 * Views and weights share one size; every view has a PSF of its own size.  The PSF images are not written: the library
 * normalises copies.
 */
public class MultiViewDeconvolutionGPU
{
	/** iterations over all views, &gt;= 1 */
	public int iterations = 10;
	/** the convolutions: 0 auto, 1 FFT, 2 direct stencil */
	public int method = 0;
	/** &gt; 0: the constant start estimate; &lt;= 0: the mean of the views */
	public float initValue = 0f;
	/** floor of the estimate */
	public float minValue = 0.0001f;
	/** floor of the blurred estimate under the division */
	public float eps = 1e-6f;
	/** Tikhonov weight, 0 = off */
	public double lambda = 0.0;

	/** weights may be null: every view then replaces the estimate */
	public Img< FloatType > run( final List< ? extends RandomAccessibleInterval< FloatType > > views, final List< ? extends RandomAccessibleInterval< FloatType > > psfs,
			final List< ? extends RandomAccessibleInterval< FloatType > > weights )
	{
		return run( views, psfs, weights, null );
	}

	/** start: the estimate to continue from (null: initValue / the mean of the views) */
	public Img< FloatType > run( final List< ? extends RandomAccessibleInterval< FloatType > > views, final List< ? extends RandomAccessibleInterval< FloatType > > psfs,
			final List< ? extends RandomAccessibleInterval< FloatType > > weights, final RandomAccessibleInterval< FloatType > start )
	{
		final int nv = views.size();
		if ( nv < 1 || psfs.size() != nv || ( weights != null && weights.size() != nv ) )
			throw new IllegalArgumentException( "one PSF and (with weights) one weight image per view" );
		final long[] d = Buffers.dims( views.get( 0 ) );
		final long[] kdims = new long[ 3 * nv ];
		final Buffers.Block[] b = new Buffers.Block[ 3 * nv + 1 ];
		try
		{
			final FloatBuffer[] fv = new FloatBuffer[ nv ], fp = new FloatBuffer[ nv ], fw = weights != null ? new FloatBuffer[ nv ] : null;
			for ( int i = 0; i < nv; ++i )
			{
				if ( !java.util.Arrays.equals( Buffers.dims( views.get( i ) ), d ) || ( weights != null && !java.util.Arrays.equals( Buffers.dims( weights.get( i ) ), d ) ) )
					throw new IllegalArgumentException( "all views and weights must have the same size" );
				fv[ i ] = ( b[ i ] = Buffers.toBlock( views.get( i ) ) ).floats;
				fp[ i ] = ( b[ nv + i ] = Buffers.toBlock( psfs.get( i ) ) ).floats;
				if ( weights != null )
					fw[ i ] = ( b[ 2 * nv + i ] = Buffers.toBlock( weights.get( i ) ) ).floats;
				System.arraycopy( Buffers.dims( psfs.get( i ) ), 0, kdims, 3 * i, 3 );
			}
			if ( start != null && !java.util.Arrays.equals( Buffers.dims( start ), d ) )
				throw new IllegalArgumentException( "the start estimate must have the views' size" );
			final Buffers.Block psi = b[ 3 * nv ] = start != null ? Buffers.toBlock( start ) : Buffers.direct( Buffers.size( d ) );
			MvsimNative.deconvolve( GpuContextPool.get(), fv, fw, fp, kdims, d, iterations, method, start != null, initValue, minValue, eps, lambda, psi.floats );
			return Buffers.toImg( psi, d );
		}
		finally
		{
			for ( final Buffers.Block x : b )
				if ( x != null ) x.close();
		}
	}
}
