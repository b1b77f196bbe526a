package net.preibisch.simulation.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.DoubleBuffer;
import java.util.ArrayList;
import java.util.List;

/**
 * The consumer of the detections that {@link InterestPointDetectionGPU} returns: bead-based registration of one view against
 * another on the GPU (mvsim_register_beads; include/mvsim.h states the recipe) -- nearest neighbours, geometric descriptors that
 * are invariant under rigid motion, ratio-test matching, RANSAC over java.util.Random hypotheses and an affine refit.  The
 * reference has no matcher.
 *
 * <pre>
 * final InterestPointRegistrationGPU reg = new InterestPointRegistrationGPU();
 * final InterestPointRegistrationGPU.Result r = reg.register( peaksA, peaksB );
 * if ( ( r.flags &amp; InterestPointRegistrationGPU.NO_MODEL ) == 0 ) use( r.matrix );   // 3 x 4 row-major, A to B
 * </pre>
 */
public class InterestPointRegistrationGPU
{
	/** flags of a result */
	public static final int FEW_CANDIDATES = 1, NO_MODEL = 2, CAPPED = 4, FEW_INLIERS = 8;
	/** most points per list */
	public static final int MAX_POINTS = 65536;

	/** one candidate correspondence and whether the final model keeps it */
	public static class Match
	{
		public final int a, b;
		public final double vBest, vSecond;
		public final boolean inlier;

		Match( final int a, final int b, final double vBest, final double vSecond, final boolean inlier )
		{
			this.a = a;
			this.b = b;
			this.vBest = vBest;
			this.vSecond = vSecond;
			this.inlier = inlier;
		}
	}

	public static class Result
	{
		/** 3 x 4, row-major: q = matrix[:, :3] p + matrix[:, 3] maps list A onto list B */
		public final double[] matrix = new double[ 12 ];
		public double meanError, maxError;
		/** points with descriptors */
		public long nA, nB;
		public long nCandidates, nInliers, bestHypothesis;
		public int refits, flags;
		public final List< Match > candidates = new ArrayList<>();
	}

	/** neighbours beyond three per descriptor set: 0, 1 or 2 */
	public int redundancy = 1;
	/** the second-best descriptor distance must exceed the best one by this factor, squared */
	public double ratio = 3.0;
	/** largest residual of an inlier, voxels */
	public double maxEpsilon = 5.0;
	public double minInlierRatio = 0.1;
	/** hypothesis h draws from new java.util.Random( seed + h ) */
	public long seed = 0;
	public int hypotheses = 10000;
	public int maxRefits = 8;
	public int minInliers = 12;

	/** Positions of both views as (x, y, z) triples. */
	public Result register( final List< double[] > posA, final List< double[] > posB )
	{
		if ( posA == null || posB == null )
			throw new IllegalArgumentException( "two position lists expected" );
		if ( posA.size() > MAX_POINTS || posB.size() > MAX_POINTS )
			throw new IllegalArgumentException( "at most " + MAX_POINTS + " points per list" );
		final DoubleBuffer a = pack( posA ), b = pack( posB );
		final int slots = Math.max( posA.size(), 1 );
		final ByteBuffer res = ByteBuffer.allocateDirect( 160 ).order( ByteOrder.nativeOrder() );
		final ByteBuffer cand = ByteBuffer.allocateDirect( 24 * slots ).order( ByteOrder.nativeOrder() );
		final ByteBuffer mask = ByteBuffer.allocateDirect( slots ).order( ByteOrder.nativeOrder() );
		final long n = MvsimNative.registerBeads( GpuContextPool.get(), a, posA.size(), b, posB.size(), redundancy, ratio, maxEpsilon,
				minInlierRatio, seed, hypotheses, maxRefits, minInliers, res, cand, mask );
		final Result r = new Result();
		for ( int i = 0; i < 12; ++i )
			r.matrix[ i ] = res.getDouble( 8 * i );
		r.meanError = res.getDouble( 96 );
		r.maxError = res.getDouble( 104 );
		r.nA = res.getLong( 112 );
		r.nB = res.getLong( 120 );
		r.nCandidates = res.getLong( 128 );
		r.nInliers = res.getLong( 136 );
		r.bestHypothesis = res.getLong( 144 );
		r.refits = res.getInt( 152 );
		r.flags = res.getInt( 156 );
		final int listed = ( int ) Math.min( n, slots );
		for ( int i = 0; i < listed; ++i )
			r.candidates.add( new Match( cand.getInt( 24 * i ), cand.getInt( 24 * i + 4 ), cand.getDouble( 24 * i + 8 ), cand.getDouble( 24 * i + 16 ),
					mask.get( i ) != 0 ) );
		return r;
	}

	/** The detections of two views, as {@link InterestPointDetectionGPU#detect} returns them. */
	public Result registerPeaks( final List< InterestPointDetectionGPU.Peak > peaksA, final List< InterestPointDetectionGPU.Peak > peaksB )
	{
		final List< double[] > a = new ArrayList<>( peaksA.size() ), b = new ArrayList<>( peaksB.size() );
		for ( final InterestPointDetectionGPU.Peak p : peaksA )
			a.add( p.pos );
		for ( final InterestPointDetectionGPU.Peak p : peaksB )
			b.add( p.pos );
		return register( a, b );
	}

	private static DoubleBuffer pack( final List< double[] > pos )
	{
		final DoubleBuffer buf = ByteBuffer.allocateDirect( 24 * Math.max( pos.size(), 1 ) ).order( ByteOrder.nativeOrder() ).asDoubleBuffer();
		for ( int i = 0; i < pos.size(); ++i )
		{
			final double[] p = pos.get( i );
			if ( p == null || p.length < 3 )
				throw new IllegalArgumentException( "every position needs x, y and z" );
			buf.put( 3 * i, p[ 0 ] ).put( 3 * i + 1, p[ 1 ] ).put( 3 * i + 2, p[ 2 ] );
		}
		return buf;
	}
}
