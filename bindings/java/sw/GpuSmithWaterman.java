package sw ;

import org.apache.spark.api.java.function.PairFlatMapFunction ;
import org.apache.spark.api.java.function.PairFunction ;

import scala.Tuple2 ;
import scala.Tuple3 ;

import java.nio.ByteBuffer ;
import java.nio.charset.StandardCharsets ;
import java.util.ArrayList ;
import java.util.Iterator ;

/**
 * Drop-in replacements for Distribution.MapRef (src/sw/Distribution.java:383-437) that run the matrix fill,
 * tied-maximum search and traceback of every (reference, read) pair on an MI355X through libswmi.so.
 *
 * NOT compiled by this repository's build (no JDK in the build image); see INTEGRATION.md.
 *
 *   mapRDD = listRDD.mapToPair( new MapRef() ) ;                           // reference, Distribution.java:338
 *   mapRDD = listRDD.mapPartitionsToPair( new GpuSmithWaterman.MapPartition() ) ;   // one native call per partition
 *   mapRDD = listRDD.mapToPair( new GpuSmithWaterman.MapRef() ) ;           // per element (simple, slower)
 */
public class GpuSmithWaterman
{
	static { System.loadLibrary( "swmi_jni" ) ; }

	public static final int TIE_SERIAL = 0 ;	// SmithWaterman.GetCellScore order
	public static final int TIE_STRICT = 1 ;	// DistributedSW.GetCellScore order

	static native long nativeCreate( int device ) ;
	static native void nativeDestroy( long ctx ) ;
	static native long nativeAlignBatch( long ctx , int match , int mismatch , int gap , int tieMode , byte[] types ,
			ByteBuffer refBytes , long[] refOff , int nRefs , ByteBuffer readBytes , long[] readOff , int nReads ) ;
	/** affine gaps on the context: alignScores { match , mismatch , gap , gapOpen } -- a gap of length k costs gapOpen + k * gap */
	static native void nativeSetGapOpen( long ctx , int gapOpen ) ;
	/** end-to-end alignment on the context: ALIGN_LOCAL, ALIGN_FIT or ALIGN_GLOBAL (include/swmi.h: option "align_mode") */
	static native void nativeSetAlignMode( long ctx , int alignMode ) ;
	/** reads longer than 1024 bases on the affine kernels: 1 allowed, 0 refused (include/swmi.h: option "long_reads") */
	static native void nativeSetLongReads( long ctx , int longReads ) ;
	/** reads longer than 1024 bases inside a band of this half-width around the diagonal, 0: no band (include/swmi.h: option "band") */
	static native void nativeSetBand( long ctx , int band ) ;
	/** seed extension with ALIGN_GLOBAL: 1 on, 0 off (include/swmi.h: option "extend") */
	static native void nativeSetExtend( long ctx , int extend ) ;
	/** the drop-off threshold of seed extension for reads longer than 1024 bases, 0: off (include/swmi.h: option "xdrop") */
	static native void nativeSetXdrop( long ctx , int xdrop ) ;
	/** the band of a banded seed extension follows the alignment: 1 on, 0 off (include/swmi.h: option "band_adapt") */
	static native void nativeSetBandAdapt( long ctx , int bandAdapt ) ;
	/** two-piece gaps: alignScores { match , mismatch , gap , gapOpen , gap2 , gapOpen2 } -- a gap of length k costs
	 * max( gapOpen + k * gap , gapOpen2 + k * gap2 ) on a global or extend run; gapOpen2 0: off (include/swmi.h: option "gap_open2") */
	static native void nativeSetGap2( long ctx , int gapOpen2 , int gap2 ) ;
	/** alignments as CIGARs: 1 M/I/D, 2 =/X/I/D, 0 off (include/swmi.h: option "cigar") */
	static native void nativeSetCigar( long ctx , int cigar ) ;
	/** fills info = { begin , last row , last column } and returns the CIGAR entries len &lt;&lt; 4 | op of alignment k, from its start */
	static native int[] nativePairCigar( long batch , long pair , long k , int[] info ) ;
	/** the edit distance (SAM's NM) of alignment k: X columns + inserted + deleted bases */
	static native int nativePairNm( long batch , long pair , long k ) ;
	/** the second-best score: the mask half-width in columns, -1 per pair, 0 off (include/swmi.h: option "subopt") */
	static native void nativeSetSubopt( long ctx , int subopt ) ;
	/** { second-best score , the reference column it ends in } of a pair after a run under that option */
	static native int[] nativePairSubopt( long batch , long pair ) ;
	/** the end bonus of extend runs: 1 .. 2^30 the bonus, 0 off (include/swmi.h: option "end_bonus") */
	static native void nativeSetEndBonus( long ctx , int endBonus ) ;
	/** { max score , to-end score , the reference column it ends in , taken to the end ? 1 : 0 } of a pair after a run under that option */
	static native int[] nativePairEndScore( long batch , long pair ) ;
	/** overlap (ends-free) alignment with ALIGN_FIT: 1 on, 0 off (include/swmi.h: option "overlap") */
	static native void nativeSetOverlap( long ctx , int overlap ) ;
	/** the best local hits: the most entries per pair, 0 off (include/swmi.h: option "hits"; needs nativeSetSubopt) */
	static native void nativeSetHits( long ctx , int hits ) ;
	/** { score , read row , reference column } of every hit of a pair after a run under that option, best first */
	static native int[] nativePairHits( long batch , long pair ) ;
	/** substitution scores on the context: alphabet = n ISO-8859-1 symbols, scores = n * n, row = read base; null clears */
	static native void nativeSetScoreMatrix( long ctx , byte[] alphabet , int[] scores ) ;
	/** per-read score profiles on a batch of nativeAlignBatch, and the batch run again under them: alphabet = n ISO-8859-1 symbols,
	 * scores = n entries per read byte in upload order, nRows = the reads' bytes; alphabet null clears ( setReadProfiles ) */
	static native void nativeSetReadProfiles( long ctx , long batch , int match , int mismatch , int gap , int tieMode , byte[] types ,
	                                          byte[] alphabet , int[] scores , long nRows ) ;
	/** a pair list over the sequences: specs = eight ints per pair ( alignPairs ) */
	static native long nativeAlignPairs( long ctx , int match , int mismatch , int gap , int tieMode , byte[] types ,
	                                     ByteBuffer refBytes , long[] refOff , int nRefs , ByteBuffer readBytes , long[] readOff , int nReads , int[] specs ) ;
	static native void nativePairResults( long batch , int[] scores , long[] counts ) ;
	/** fills info = { begin , last row , last column } and returns { refAligned , readAligned } as ISO-8859-1 bytes */
	static native byte[][] nativePairAlignment( long batch , long pair , long k , int[] info ) ;
	static native void nativeFreeBatch( long ctx , long batch ) ;
	static native int nativeRefTotal( long batch , int ref ) ;
	static native long nativeRefSiteCount( long batch , int ref ) ;
	static native byte[][] nativeRefSite( long batch , int ref , long k , int[] begin ) ;
	/** {number of match sites, bytes of all their strings} of the references refLo .. refHi-1 */
	static native long[] nativeRefSitesSizes( long batch , int refLo , int refHi ) ;
	/** MapRef's output of the references refLo .. refHi-1 into the caller's arrays, ONE call (swmi_ref_sites_packed, include/swmi.h) */
	static native void nativeRefSitesPacked( long batch , int refLo , int refHi , int[] totals , long[] degenerate , long[] siteFirst ,
			int[] begins , int[] lens , long[] strOff , byte[] blob ) ;

	/** a native context and the version of the score matrix it holds (0: none set on it yet) */
	private static final class NativeContext
	{
		final long handle ;
		long matrixVersion = 0 ;		// (touched only by the owning thread)
		NativeContext( long handle ) { this.handle = handle ; }
	}

	/** one context per executor thread: MapRef.call runs concurrently on every task thread */
	private static final java.util.concurrent.ConcurrentHashMap<Long,NativeContext> CONTEXTS = new java.util.concurrent.ConcurrentHashMap<Long,NativeContext>() ;
	static
	{
		// executor threads outlive tasks; whatever is still open when the JVM goes down is destroyed here
		Runtime.getRuntime().addShutdownHook( new Thread() { @Override public void run() { releaseAllContexts() ; } } ) ;
	}

	public static final int ALIGN_LOCAL = 0 , ALIGN_FIT = 1 , ALIGN_GLOBAL = 2 ;
	/** what every context aligns end to end from its next batch on (applied next to gapOpen, before every batch) */
	private static volatile int ALIGN_MODE = ALIGN_LOCAL ;

	/**
	 * ALIGN_LOCAL (the default): Smith-Waterman.  ALIGN_FIT: the whole read against any stretch of the reference.  ALIGN_GLOBAL: the
	 * whole read against the whole reference.  Totals may then be zero or negative, and every match site spells the whole read.
	 * For every batch aligned from now on, on every executor thread.
	 */
	public static void setAlignMode( int alignMode )
	{
		if( alignMode != ALIGN_LOCAL && alignMode != ALIGN_FIT && alignMode != ALIGN_GLOBAL )
			throw new IllegalArgumentException( "alignMode must be ALIGN_LOCAL, ALIGN_FIT or ALIGN_GLOBAL: " + alignMode ) ;
		ALIGN_MODE = alignMode ;
	}

	/** whether every context lets the affine kernels take reads longer than 1024 bases (applied next to alignMode, before every batch) */
	private static volatile boolean LONG_READS = false ;

	/**
	 * true: runs on the affine kernels (gapOpen, a score matrix, ALIGN_FIT / ALIGN_GLOBAL) take reads longer than 1024 bases, swept in
	 * strips of 1024 rows; false (the default): such a read is refused.  For every batch aligned from now on, on every executor thread.
	 */
	public static void setLongReads( boolean longReads ) { LONG_READS = longReads ; }

	/** the half-width of the band every context aligns reads longer than 1024 bases in, 0: none (applied next to longReads, before every batch) */
	private static volatile int BAND = 0 ;

	/**
	 * band &gt; 0: a read longer than 1024 bases (setLongReads) is aligned inside the band |j - i| &lt;= band only, rounded outwards to strips
	 * of 1024 rows, on the affine kernels; 0 (the default): no band.  For every batch aligned from now on, on every executor thread.
	 */
	public static void setBand( int band ) { BAND = band ; }

	/** whether every context runs ALIGN_GLOBAL as seed extension (applied next to band, before every batch) */
	private static volatile boolean EXTEND = false ;

	/**
	 * true: with ALIGN_GLOBAL the alignment is anchored at the start of the read and of the reference and ends at the cell with the
	 * best score, the tails left unaligned (seed extension; the total may be zero or negative; for left extension reverse both
	 * sequences); with another align mode the batch is refused.  false (the default): off.  For every batch aligned from now on, on
	 * every executor thread.
	 */
	public static void setExtend( boolean extend ) { EXTEND = extend ; }

	/** the drop-off threshold every context runs seed extension with, 0: none (applied next to extend, before every batch) */
	private static volatile int XDROP = 0 ;

	/**
	 * With setExtend( true ) and setLongReads( true ): the sweep of a read longer than 1024 bases ends behind the first strip of 1024
	 * rows whose last row lies more than xdrop below the best score so far, and the best cell so far is the answer; 0 (the
	 * default): off.  With xdrop &gt; 0 and no seed extension the batch is refused.  For every batch aligned from now on, on every
	 * executor thread.
	 */
	public static void setXdrop( int xdrop ) { XDROP = xdrop ; }

	/** whether every context lets the band of a banded seed extension follow the alignment (applied next to band, before every batch) */
	private static volatile boolean BAND_ADAPT = false ;

	/**
	 * With setBand( w ), setExtend( true ) and setLongReads( true ): the window of every strip of 1024 rows of a read longer than 1024
	 * bases is placed around the column where the row above it scores best, so that w only has to cover the drift inside one
	 * strip; false (the default): the band stays around the main diagonal.  With true and no banded seed extension the batch is
	 * refused.  For every batch aligned from now on, on every executor thread.
	 */
	public static void setBandAdapt( boolean bandAdapt ) { BAND_ADAPT = bandAdapt ; }

	/** the CIGAR payload every context asks its runs for, 0: none (applied next to bandAdapt, before every batch) */
	private static volatile int CIGAR = 0 ;
	public static final int CIGAR_M = 0 , CIGAR_I = 1 , CIGAR_D = 2 , CIGAR_EQ = 7 , CIGAR_X = 8 ;

	/**
	 * 1: the GPU writes every alignment as a run-length CIGAR of M / I / D with its edit distance; 2: of = / X / I / D; 0 (the
	 * default): strings.  Such a run takes the affine kernels; the strings the other methods return stay the same.  For every
	 * batch aligned from now on, on every executor thread.
	 */
	public static void setCigar( int cigar )
	{
		if( cigar < 0 || cigar > 2 ) throw new IllegalArgumentException( "cigar must be 0, 1 or 2: " + cigar ) ;
		CIGAR = cigar ;
	}

	/** the CIGAR of alignment k of a pair of a native batch run under setCigar: entries len &lt;&lt; 4 | op ( CIGAR_M , ... ), from the alignment's start */
	static int[] cigar( long batch , long pair , long k ) { return nativePairCigar( batch , pair , k , null ) ; }
	/** ... and its edit distance */
	static int nm( long batch , long pair , long k ) { return nativePairNm( batch , pair , k ) ; }

	/** the mask half-width of the second-best score every context asks its runs for, 0: none (applied next to cigar, before every batch) */
	private static volatile int SUBOPT = 0 ;
	public static final int SUBOPT_AUTO = -1 ;

	/**
	 * w in 1 .. 2^30: a local run also computes every pair's second-best score, the best score of an alignment that ends more than
	 * w columns away from every column where the best one ends; SUBOPT_AUTO: w = max( m / 2 , 15 ) per pair, m the read's length;
	 * 0 (the default): off.  Such a run takes the affine kernels and ALIGN_LOCAL.  For every batch aligned from now on, on every
	 * executor thread.
	 */
	public static void setSubopt( int w )
	{
		if( w < -1 || w > ( 1 << 30 ) ) throw new IllegalArgumentException( "subopt must be 0, -1 or 1 .. 2^30: " + w ) ;
		SUBOPT = w ;
	}

	/** { second-best score , the reference column it ends in } of a pair of a native batch run under setSubopt ( { 0 , 0 }: none ) */
	static int[] subopt( long batch , long pair ) { return nativePairSubopt( batch , pair ) ; }

	/** the end bonus every context asks its extend runs for, 0: none (applied next to subopt, before every batch) */
	private static volatile int END_BONUS = 0 ;

	/**
	 * b in 1 .. 2^30: an extend run also computes every pair's best score in the read's last row and takes the pair to the end of
	 * the read when that is less than b below the best score anywhere (strictly: toEnd + b > best); 0 (the default): off.  Needs an
	 * extend run without xdrop, band_adapt or two-piece gaps.  For every batch aligned from now on, on every executor thread.
	 */
	public static void setEndBonus( int b )
	{
		if( b < 0 || b > ( 1 << 30 ) ) throw new IllegalArgumentException( "endBonus must be 0 or 1 .. 2^30: " + b ) ;
		END_BONUS = b ;
	}

	/** { max score , to-end score , its reference column , taken to the end ? 1 : 0 } of a pair of a native batch run under setEndBonus */
	static int[] endScore( long batch , long pair ) { return nativePairEndScore( batch , pair ) ; }

	/** whether every context runs ALIGN_FIT as overlap alignment (applied next to END_BONUS, before every batch) */
	private static volatile boolean OVERLAP = false ;

	/**
	 * true: a run with ALIGN_FIT is an overlap (ends-free, dovetail) alignment -- the read's ends are free as well as the
	 * reference's, the alignment ends in the read's last row or the reference's last column and its score may be <= 0.  Needs
	 * ALIGN_FIT without band, extend, two-piece gaps, subopt, hits and endBonus.  For every batch aligned from now on, on every
	 * executor thread.
	 */
	public static void setOverlap( boolean overlap ) { OVERLAP = overlap ; }

	/** the most local hits per pair every context asks its runs for, 0: none (applied next to SUBOPT, before every batch) */
	private static volatile int HITS = 0 ;

	/**
	 * k in 1 .. 16: a run under setSubopt also returns, per pair, up to k local hits -- the best alignment's score and end cell, then the
	 * best scores that end more than the mask half-width away from it and from each other, each with the cell it ends in; 0 (the
	 * default): off.  Needs setSubopt != 0: a batch aligned with hits and without it is refused.  For every batch aligned from now on,
	 * on every executor thread.
	 */
	public static void setHits( int k )
	{
		if( k < 0 || k > 16 ) throw new IllegalArgumentException( "hits must be 0 .. 16: " + k ) ;
		HITS = k ;
	}

	/** { score , read row , reference column } per hit of a pair of a native batch run under setHits, best first (1-based cells) */
	static int[] hits( long batch , long pair ) { return nativePairHits( batch , pair ) ; }

	/**
	 * Per-read score profiles (position-specific scoring matrices; include/swmi.h: swmi_batch_set_read_profiles) on a native batch of
	 * this thread's context, and the batch run again under them: alphabet = the n symbols (ISO-8859-1, distinct ignoring case),
	 * profiles[q][i][c] = the score of position i of read q against reference symbol alphabet[c]; a reference base outside the alphabet
	 * scores mismatch.  alignScores = { match , mismatch , gap }, types and tieMode as the batch was aligned with.  alphabet null
	 * clears the profiles.  The score matrix of setScoreMatrix must not be set at the same time.
	 * PRECONDITION, which neither this method nor the library can check (the library has no query for a batch's reads): profiles has
	 * one entry per read of the batch, in upload order, and profiles[q].length is the length of read q.  The library reads n entries
	 * per read byte of the batch from the flattened array; with fewer rows than that it reads past the array's end.
	 */
	static void setReadProfiles( long ctx , long batch , int[] alignScores , int tieMode , byte[] types , String alphabet , int[][][] profiles )
	{
		if( alphabet == null ) { nativeSetReadProfiles( ctx , batch , alignScores[0] , alignScores[1] , alignScores[2] , tieMode , types , null , null , 0L ) ; return ; }
		int n = alphabet.length() ;
		for( int i = 0 ; i < n ; i++ )
			if( alphabet.charAt(i) > 0xFF )
				throw new IllegalArgumentException( "profile symbol " + i + " is not an ISO-8859-1 character" ) ;
		if( profiles == null ) throw new IllegalArgumentException( "profiles is null" ) ;
		long rows = 0 ;
		for( int[][] p : profiles ) rows += p.length ;
		if( rows * n > Integer.MAX_VALUE ) throw new IllegalArgumentException( "more than 2^31 - 1 profile entries in one batch" ) ;
		int[] flat = new int[(int)( rows * n )] ;
		int at = 0 ;
		for( int q = 0 ; q < profiles.length ; q++ )
			for( int i = 0 ; i < profiles[q].length ; i++ )
			{
				if( profiles[q][i] == null || profiles[q][i].length != n ) throw new IllegalArgumentException( "profile " + q + " row " + i + " needs " + n + " entries" ) ;
				System.arraycopy( profiles[q][i] , 0 , flat , at , n ) ;
				at += n ;
			}
		nativeSetReadProfiles( ctx , batch , alignScores[0] , alignScores[1] , alignScores[2] , tieMode , types ,
		                       alphabet.getBytes( StandardCharsets.ISO_8859_1 ) , flat , rows ) ;
	}

	/** the score matrix every context applies before its next batch: { alphabet , scores } (null: none), and its version */
	private static volatile Object[] MATRIX = null ;
	private static final java.util.concurrent.atomic.AtomicLong MATRIX_VERSION = new java.util.concurrent.atomic.AtomicLong() ;

	/**
	 * Substitution scores for every batch aligned from now on, on every executor thread (include/swmi.h: swmi_set_score_matrix):
	 * alphabet = the n symbols (ISO-8859-1, distinct ignoring case), scores[i][j] = score of read base alphabet[i] against
	 * reference base alphabet[j].  Bases outside the alphabet keep alignScores' match / mismatch.  null clears the matrix.
	 * Symbols must be ISO-8859-1 characters (U+0000..U+00FF): sequences are passed to the library as ISO-8859-1 bytes.
	 */
	public static void setScoreMatrix( String alphabet , int[][] scores )
	{
		if( alphabet == null ) { MATRIX = new Object[] { null , null , Long.valueOf( MATRIX_VERSION.incrementAndGet() ) } ; return ; }
		int n = alphabet.length() ;
		for( int i = 0 ; i < n ; i++ )
			if( alphabet.charAt(i) > 0xFF )
				throw new IllegalArgumentException( "score matrix symbol " + i + " (U+" + Integer.toHexString( alphabet.charAt(i) ).toUpperCase() + ") is not an ISO-8859-1 character" ) ;
		if( scores == null || scores.length != n ) throw new IllegalArgumentException( "scores needs " + n + " rows" ) ;
		int[] flat = new int[n*n] ;
		for( int i = 0 ; i < n ; i++ )
		{
			if( scores[i] == null || scores[i].length != n ) throw new IllegalArgumentException( "row " + i + " needs " + n + " entries" ) ;
			System.arraycopy( scores[i] , 0 , flat , i * n , n ) ;
		}
		MATRIX = new Object[] { alphabet.getBytes( StandardCharsets.ISO_8859_1 ) , flat , Long.valueOf( MATRIX_VERSION.incrementAndGet() ) } ;
	}

	/** the current matrix on this thread's context, if it does not hold it yet (the version lives with the context, so a context
	 *  created after another was destroyed never inherits its state) */
	private static void applyScoreMatrix( NativeContext ctx )
	{
		Object[] m = MATRIX ;
		if( m == null ) return ;
		long ver = ((Long)m[2]).longValue() ;
		if( ctx.matrixVersion == ver ) return ;
		nativeSetScoreMatrix( ctx.handle , (byte[])m[0] , (int[])m[1] ) ;
		ctx.matrixVersion = ver ;
	}

	private static NativeContext context()
	{
		Long tid = Long.valueOf( Thread.currentThread().getId() ) ;
		NativeContext ctx = CONTEXTS.get( tid ) ;
		if( ctx == null )
		{
			int nGpus = Integer.getInteger( "swmi.gpus" , 8 ) ;
			ctx = new NativeContext( nativeCreate( (int)( tid.longValue() % nGpus ) ) ) ;
			CONTEXTS.put( tid , ctx ) ;
		}
		return ctx ;
	}

	/** destroys the calling thread's context (device buffers, HIP stream): call it when a task thread retires */
	public static void releaseThreadContext()
	{
		NativeContext ctx = CONTEXTS.remove( Long.valueOf( Thread.currentThread().getId() ) ) ;
		if( ctx != null ) nativeDestroy( ctx.handle ) ;
	}

	/** destroys every context (no native call may be in flight) */
	public static synchronized void releaseAllContexts()
	{
		for( Long tid : new ArrayList<Long>( CONTEXTS.keySet() ) )
		{
			NativeContext ctx = CONTEXTS.remove( tid ) ;
			if( ctx != null ) nativeDestroy( ctx.handle ) ;
		}
	}

	/** a direct ByteBuffer holds at most Integer.MAX_VALUE bytes: one native call takes at most this many sequence bytes */
	private static final long MAX_BYTES_PER_CALL = 1L << 30 ;
	private static final Tuple2<Integer,String[]> EMPTY_SITE = new Tuple2<Integer,String[]>( Integer.valueOf(0) , new String[]{ "" , "" } ) ;

	/**
	 * Characters above U+00FF cannot be narrowed to ISO-8859-1: map Character.toUpperCase(c) of every distinct
	 * such character of the partition to a free byte value first (the aligned strings come back as bytes of the
	 * sequences as uploaded, so the mapping must be undone on the way out).  DNA/IUPAC input never needs it.
	 */
	private static ByteBuffer pack( java.util.List<String> seqs , long[] off )
	{
		long total = 0 ;
		for( int i = 0 ; i < seqs.size() ; i++ ) { off[i] = total ; total += seqs.get(i).length() ; }
		off[seqs.size()] = total ;
		if( total > Integer.MAX_VALUE )		// (MapPartition never hands over more than MAX_BYTES_PER_CALL of references; reads are one list)
			throw new IllegalArgumentException( "more than 2 GiB of sequence in one native call: " + total ) ;
		ByteBuffer buf = ByteBuffer.allocateDirect( (int) Math.max(total,1L) ) ;
		for( String s : seqs ) buf.put( s.getBytes(StandardCharsets.ISO_8859_1) ) ;
		return buf ;
	}

	/** the scores' optional entries and the class's run options onto a native context, before a native align call */
	private static void applyRunOptions( NativeContext nc , int[] sc )
	{
		long ctx = nc.handle ;
		// alignScores may carry a fourth entry, gapOpen (<= 0): affine gaps; three entries keep the linear scoring
		// ... and a fifth and sixth, gap2 and gapOpen2 (<= 0): two-piece gaps, with ALIGN_GLOBAL
		if( sc.length != 3 && sc.length != 4 && sc.length != 6 ) throw new IllegalArgumentException( "alignScores needs 3, 4 or 6 entries: " + sc.length ) ;
		nativeSetGapOpen( ctx , sc.length >= 4 ? sc[3] : 0 ) ;
		nativeSetGap2( ctx , sc.length == 6 ? sc[5] : 0 , sc.length == 6 ? sc[4] : 0 ) ;
		nativeSetAlignMode( ctx , ALIGN_MODE ) ;
		nativeSetLongReads( ctx , LONG_READS ? 1 : 0 ) ;
		nativeSetBand( ctx , BAND ) ;
		nativeSetExtend( ctx , EXTEND ? 1 : 0 ) ;
		nativeSetXdrop( ctx , XDROP ) ;
		nativeSetBandAdapt( ctx , BAND_ADAPT ? 1 : 0 ) ;
		nativeSetCigar( ctx , CIGAR ) ;
		nativeSetSubopt( ctx , SUBOPT ) ;
		nativeSetHits( ctx , HITS ) ;
		nativeSetEndBonus( ctx , END_BONUS ) ;
		nativeSetOverlap( ctx , OVERLAP ? 1 : 0 ) ;
		applyScoreMatrix( nc ) ;
	}

	/** swmi_pair_spec.flags: both segments of the pair are taken in reverse order ( a left extension ) */
	public static final int SPEC_REVERSE = 1 ;

	/**
	 * swmi_pair_spec.flags: the pair is on the minus strand -- the READ segment is taken reverse-complemented ( IUPAC codes, case
	 * kept, U to A ) on the GPU and the reference segment is untouched; the read is uploaded once for both strands.  Combines with
	 * SPEC_REVERSE : the reference is reversed iff SPEC_REVERSE is set, the read is reversed iff exactly one of the two is set
	 * and complemented iff this one is.  Coordinates stay the segments': column j is reference character refStart + j - 1, or
	 * refStart + refLen - j under SPEC_REVERSE ; row i is read character readStart + i - 1 when the read's order is forward
	 * ( flags 0 or SPEC_REVERSE | SPEC_READ_REVCOMP ) and readStart + readLen - i when it is reversed ( flags SPEC_REVERSE or
	 * SPEC_READ_REVCOMP ).  readAligned holds the complemented characters.
	 */
	public static final int SPEC_READ_REVCOMP = 4 ;

	/**
	 * A PAIR LIST in one native call: what a read mapper has after chaining.  refs / reads are uploaded once; specs holds eight
	 * ints per pair -- { ref , read , refStart , refLen , readStart , readLen , flags , 0 } : indices into refs / reads, the 0-based
	 * start and the length of the two segments ( -1 as a length: to the end of the sequence ) and SPEC_REVERSE in flags for a
	 * left extension ( both segments are taken in reverse order ).  The GPU cuts the segments from the resident sequences.
	 * Returns, per pair in list order, ( score , alignments as ( begin , { refAligned , readAligned } ) ) with coordinates in the
	 * SEGMENTS: column j is reference character refStart + j - 1, or refStart + refLen - j when reversed.  alignScores and
	 * alignTypes are OptAlignments' arrays ( null: the defaults ); the run options set on this class ( setAlignMode, setExtend,
	 * setBand, ... ) apply.
	 */
	public static ArrayList<Tuple2<Integer,ArrayList<Tuple2<Integer,String[]>>>> alignPairs( String[] refs , String[] reads , int[] specs )
	{
		return alignPairs( refs , reads , specs , null , null ) ;
	}
	public static ArrayList<Tuple2<Integer,ArrayList<Tuple2<Integer,String[]>>>> alignPairs( String[] refs , String[] reads , int[] specs , int[] alignScores , char[] alignTypes )
	{
		int[] sc = alignScores != null ? alignScores : new int[]{ 5 , -3 , -4 } ;		// Distribution.java:36-37
		char[] ty = alignTypes != null ? alignTypes : new char[]{ 'a' , 'i' , 'd' , '-' } ;
		if( specs.length % 8 != 0 ) throw new IllegalArgumentException( "specs needs 8 ints per pair: " + specs.length ) ;
		int nPairs = specs.length / 8 ;
		long[] refOff = new long[refs.length+1] , readOff = new long[reads.length+1] ;
		ByteBuffer refBuf = pack( java.util.Arrays.asList(refs) , refOff ) , readBuf = pack( java.util.Arrays.asList(reads) , readOff ) ;
		byte[] types = { (byte)ty[0] , (byte)ty[1] , (byte)ty[2] , (byte)ty[3] } ;
		NativeContext nc = context() ;
		long ctx = nc.handle ;
		applyRunOptions( nc , sc ) ;
		long batch = nativeAlignPairs( ctx , sc[0] , sc[1] , sc[2] , TIE_SERIAL , types , refBuf , refOff , refs.length , readBuf , readOff , reads.length , specs ) ;
		try
		{
			int[] scores = new int[nPairs] ;
			long[] counts = new long[nPairs] ;
			nativePairResults( batch , scores , counts ) ;
			ArrayList<Tuple2<Integer,ArrayList<Tuple2<Integer,String[]>>>> out = new ArrayList<Tuple2<Integer,ArrayList<Tuple2<Integer,String[]>>>>( nPairs ) ;
			int[] info = new int[3] ;
			for( int p = 0 ; p < nPairs ; p++ )
			{
				if( counts[p] > Integer.MAX_VALUE ) throw new IllegalStateException( "pair " + p + " has " + counts[p] + " alignments" ) ;
				ArrayList<Tuple2<Integer,String[]>> alns = new ArrayList<Tuple2<Integer,String[]>>( (int)counts[p] ) ;
				for( long k = 0 ; k < counts[p] ; k++ )
				{
					byte[][] two = nativePairAlignment( batch , p , k , info ) ;
					alns.add( two[0].length == 0 ? EMPTY_SITE : new Tuple2<Integer,String[]>( Integer.valueOf(info[0]) ,
						new String[]{ new String( two[0] , StandardCharsets.ISO_8859_1 ) , new String( two[1] , StandardCharsets.ISO_8859_1 ) } ) ) ;
				}
				out.add( new Tuple2<Integer,ArrayList<Tuple2<Integer,String[]>>>( Integer.valueOf(scores[p]) , alns ) ) ;
			}
			return out ;
		}
		finally { nativeFreeBatch( ctx , batch ) ; }
	}

	/** mapPartitionsToPair variant: the elements of the partition in ONE native call per (at most) 1 GiB of references. */
	public static class MapPartition implements PairFlatMapFunction< Iterator<Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>>> , Integer , Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>> >
	{
		@Override
		public Iterable<Tuple2<Integer,Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>>>> call( Iterator<Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>>> it )
		{
			ArrayList<Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>>> elems = new ArrayList<Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>>>() ;
			while( it.hasNext() ) elems.add( it.next() ) ;
			ArrayList<Tuple2<Integer,Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>>>> out = new ArrayList<Tuple2<Integer,Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>>>>( elems.size() ) ;
			int lo = 0 ;
			while( lo < elems.size() )
			{
				// as many elements as fit one native call
				long bytes = 0 ;
				int hi = lo ;
				while( hi < elems.size() && ( hi == lo || bytes + elems.get(hi)._1()[1].length() <= MAX_BYTES_PER_CALL ) ) { bytes += elems.get(hi)._1()[1].length() ; hi++ ; }
				alignRange( elems , lo , hi , out ) ;
				lo = hi ;
			}
			return out ;
		}

		private static void alignRange( ArrayList<Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>>> elems , int lo , int hi ,
				ArrayList<Tuple2<Integer,Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>>>> out )
		{
			// CombineReadsToRef (Distribution.java:714-724) hands every element the same reads and algoArgs
			ArrayList<String> reads = elems.get(lo)._2() ;
			int[] sc = elems.get(lo)._3()._1() ;
			char[] ty = elems.get(lo)._3()._2() ;
			int n = hi - lo ;
			ArrayList<String> refs = new ArrayList<String>( n ) ;
			for( int e = lo ; e < hi ; e++ ) refs.add( elems.get(e)._1()[1] ) ;

			long[] refOff = new long[n+1] , readOff = new long[reads.size()+1] ;
			ByteBuffer refBuf = pack( refs , refOff ) , readBuf = pack( reads , readOff ) ;
			byte[] types = { (byte)ty[0] , (byte)ty[1] , (byte)ty[2] , (byte)ty[3] } ;

			NativeContext nc = context() ;
			long ctx = nc.handle ;
			applyRunOptions( nc , sc ) ;
			long batch = nativeAlignBatch( ctx , sc[0] , sc[1] , sc[2] , TIE_SERIAL , types , refBuf , refOff , n , readBuf , readOff , reads.size() ) ;
			try
			{
				// everything MapRef returns for these references in TWO native calls: the sizes, then the data
				long[] sizes = nativeRefSitesSizes( batch , 0 , n ) ;
				if( sizes[0] > Integer.MAX_VALUE || sizes[1] > Integer.MAX_VALUE )
					throw new IllegalStateException( "the match sites of one native call do not fit Java arrays: " + sizes[0] + " sites, " + sizes[1] + " bytes" ) ;
				int[] totals = new int[n] , begins = new int[(int)sizes[0]] , lens = new int[(int)sizes[0]] ;
				long[] degenerate = new long[n] , siteFirst = new long[n+1] , strOff = new long[(int)sizes[0]] ;
				byte[] blob = new byte[(int)sizes[1]] ;
				nativeRefSitesPacked( batch , 0 , n , totals , degenerate , siteFirst , begins , lens , strOff , blob ) ;
				for( int r = 0 ; r < n ; r++ )
				{
					long nSites = degenerate[r] + siteFirst[r+1] - siteFirst[r] ;
					if( nSites > Integer.MAX_VALUE ) throw new IllegalStateException( "more match sites than an ArrayList holds: " + nSites ) ;
					ArrayList<Tuple2<Integer,String[]>> sites = new ArrayList<Tuple2<Integer,String[]>>( (int)nSites ) ;
					// a pair whose maximum is 0 yields (0, "", "") for every one of its m*n cells (SmithWaterman.java:154,182-185,378-380):
					// begin 0 sorts them in front of every real site; one shared tuple stands for all of them
					for( long d = 0 ; d < degenerate[r] ; d++ ) sites.add( EMPTY_SITE ) ;
					for( int s = (int)siteFirst[r] ; s < (int)siteFirst[r+1] ; s++ )
					{
						int at = (int)strOff[s] ;
						String[] aligned = { new String( blob , at , lens[s] , StandardCharsets.ISO_8859_1 ) ,
								new String( blob , at + lens[s] , lens[s] , StandardCharsets.ISO_8859_1 ) } ;
						sites.add( new Tuple2<Integer,String[]>( Integer.valueOf(begins[s]) , aligned ) ) ;
					}
					out.add( new Tuple2<Integer,Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>>>( Integer.valueOf(totals[r]) ,
							new Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>>( elems.get(lo+r)._1() , sites ) ) ) ;
				}
			}
			finally { nativeFreeBatch( ctx , batch ) ; }
		}
	}

	/** Same signature as Distribution.MapRef: per-element drop-in. */
	public static class MapRef implements PairFunction< Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>> , Integer , Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>> >
	{
		@Override
		public Tuple2<Integer,Tuple2<String[],ArrayList<Tuple2<Integer,String[]>>>> call( Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>> tuple )
		{
			ArrayList<Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>>> one = new ArrayList<Tuple3<String[],ArrayList<String>,Tuple2<int[],char[]>>>(1) ;
			one.add( tuple ) ;
			return new MapPartition().call( one.iterator() ).iterator().next() ;
		}
	}
}
