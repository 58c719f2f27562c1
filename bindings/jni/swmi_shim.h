/*
 * swmi_shim.h -- the JNI shim's logic without JNI: argument checks + the exact C-ABI call sequence the
 * Java_sw_GpuSmithWaterman_* functions of swmi_jni.c perform.  Plain C99 over include/swmi.h only, so it is compiled
 * and run by the tests (tests/c/shim_kat.c, gcc -std=c99 -Wall -Werror -pedantic) although the build image has no
 * JDK; swmi_jni.c only unwraps JNI types and forwards here.
 *
 * Replaces the per-pair call  new SmithWaterman.OptAlignments().call(seqs, alignScores, alignTypes)
 * at src/sw/Distribution.java:421-422 by ONE native call per partition.
 */
#ifndef SWMI_SHIM_H
#define SWMI_SHIM_H
#include <stddef.h>
#include <stdint.h>
#include "swmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nativeAlignBatch: `types` = the alignTypes characters narrowed to bytes (types_len must be 4); ref_bytes / read_bytes
 * = addresses of the direct ByteBuffers (NULL when the buffer is not direct) and their capacities; ref_off / read_off =
 * the long[n+1] offset arrays.  Returns SWMI_OK and the batch, or a negative swmi_status with a message in err. */
int swmi_shim_align_batch(swmi_ctx *ctx, int32_t match, int32_t mismatch, int32_t gap, int32_t tie_mode,
                          const signed char *types, size_t types_len,
                          const void *ref_bytes, int64_t ref_cap, const int64_t *ref_off, int32_t n_refs,
                          const void *read_bytes, int64_t read_cap, const int64_t *read_off, int32_t n_reads,
                          swmi_batch **out, char *err, size_t err_len);

/* nativeAlignPairs: a PAIR LIST over the sequences (swmi_batch_upload_pairs + swmi_batch_run): `specs` = int[8 * n_pairs], eight
 * ints per pair in the order of swmi_pair_spec -- ref, read, refStart, refLen, readStart, readLen, flags (SWMI_SPEC_REVERSE: both
 * segments reversed, a left extension; SWMI_SPEC_READ_REVCOMP = 4: the pair is on the minus strand, the read segment taken
 * reverse-complemented and the reference untouched; the two combine), 0 -- taken as unsigned, so that -1 as a length is
 * SWMI_SPEC_WHOLE; n_spec_ints = the array's length (a multiple of 8).  The flags are passed through as given.  Coordinates are
 * the segments': column j is reference byte refStart + j - 1, or refStart + refLen - j under REVERSE; row i is read byte
 * readStart + i - 1 when the read's order is forward (flags 0 or 5) and readStart + readLen - i when it is reversed (flags 1 or
 * 4).  The other arguments are nativeAlignBatch's.  Pair k of the batch is spec k: its results are
 * read with swmi_shim_pair_results and swmi_shim_pair_alignment (the swmi_shim_ref_* views need the cross product and fail with
 * SWMI_ERR_UNSUPPORTED). */
int swmi_shim_align_pairs(swmi_ctx *ctx, int32_t match, int32_t mismatch, int32_t gap, int32_t tie_mode,
                          const signed char *types, size_t types_len,
                          const void *ref_bytes, int64_t ref_cap, const int64_t *ref_off, int32_t n_refs,
                          const void *read_bytes, int64_t read_cap, const int64_t *read_off, int32_t n_reads,
                          const int32_t *specs, int64_t n_spec_ints, swmi_batch **out, char *err, size_t err_len);
/* nativePairResults: every pair's score and number of alignments (either array may be NULL); n = the arrays' length, which must
 * be the batch's number of pairs.  nativePairAlignment: alignment k of a pair, as swmi_pair_alignment hands it out; cell[0..1]
 * receive the alignment's last cell (row, column), 1-based in the segments. */
int swmi_shim_pair_results(const swmi_batch *b, int32_t *scores, int64_t *n_alignments, int64_t n, char *err, size_t err_len);
int swmi_shim_pair_alignment(swmi_batch *b, int64_t pair, int64_t k, int32_t *begin, int32_t cell[2], const char **ref_aln,
                             const char **read_aln, uint32_t *len, char *err, size_t err_len);

/* nativeSetGapOpen: affine gaps on this context (swmi_set_option "gap_open"): a gap of length k then costs gap_open + k * gap.
 * gap_open <= 0; 0 (the default) is the linear scoring.  Applies to the batches the context aligns from then on. */
int swmi_shim_set_gap_open(swmi_ctx *ctx, int32_t gap_open, char *err, size_t err_len);
/* nativeSetAlignMode: what the context aligns end to end from then on (swmi_set_option "align_mode"): SWMI_ALIGN_LOCAL (0, the
 * default), SWMI_ALIGN_FIT (1: the whole read against any stretch of the reference) or SWMI_ALIGN_GLOBAL (2: the whole read against
 * the whole reference).  Any other value is SWMI_ERR_INVALID and leaves the context as it was. */
int swmi_shim_set_align_mode(swmi_ctx *ctx, int32_t align_mode, char *err, size_t err_len);
/* nativeSetLongReads: 1 lets the affine kernels take reads longer than 1024 bases from then on (swmi_set_option "long_reads"), 0 (the
 * default) refuses them.  Any other value is SWMI_ERR_INVALID and leaves the context as it was. */
int swmi_shim_set_long_reads(swmi_ctx *ctx, int32_t long_reads, char *err, size_t err_len);
/* nativeSetBand: reads longer than 1024 bases are aligned inside a band of this half-width around the diagonal from then on
 * (swmi_set_option "band"), 0 (the default): no band.  A value outside 0 .. 2^20 is SWMI_ERR_INVALID and leaves the context as it was. */
int swmi_shim_set_band(swmi_ctx *ctx, int32_t band, char *err, size_t err_len);
/* nativeSetExtend: 1 = seed extension from then on (swmi_set_option "extend"): a global run ends at the cell with the best score
 * instead of at (m, n); a run in another align_mode is then refused (SWMI_ERR_UNSUPPORTED).  0 (the default): off.  Any other
 * value is SWMI_ERR_INVALID and leaves the context as it was. */
int swmi_shim_set_extend(swmi_ctx *ctx, int32_t extend, char *err, size_t err_len);
/* nativeSetXdrop: the drop-off threshold of seed extension from then on (swmi_set_option "xdrop"): the sweep of a read longer than
 * 1024 bases ends behind the first strip of 1024 rows whose last row lies more than `xdrop` below the best score so far; a run that
 * is not an extend run is then refused (SWMI_ERR_UNSUPPORTED).  0 (the default): off.  A negative value is SWMI_ERR_INVALID and
 * leaves the context as it was. */
int swmi_shim_set_xdrop(swmi_ctx *ctx, int32_t xdrop, char *err, size_t err_len);
/* nativeSetBandAdapt: 1 = from then on the band of a banded extend run follows the alignment (swmi_set_option "band_adapt"): the
 * window of a strip of 1024 rows is placed around the column where the row above it scores best; a run that is not a banded
 * extend run is then refused (SWMI_ERR_UNSUPPORTED).  0 (the default): off.  Any other value is SWMI_ERR_INVALID and leaves the
 * context as it was. */
int swmi_shim_set_band_adapt(swmi_ctx *ctx, int32_t band_adapt, char *err, size_t err_len);
/* nativeSetGap2: two-piece gaps from then on (swmi_set_option "gap_open2" and "gap2"): with gap_open2 != 0 a gap of length k costs
 * max(gapOpen + k * gap, gap_open2 + k * gap2) on a global or extend run; any other run is then refused (SWMI_ERR_UNSUPPORTED).
 * gap_open2 = 0 (the default): one-piece gaps, gap2 is not read.  A value > 0 is SWMI_ERR_INVALID and leaves the context as it was
 * (both values: gap2 is checked first, and set only with a valid gap_open2). */
int swmi_shim_set_gap2(swmi_ctx *ctx, int32_t gap_open2, int32_t gap2, char *err, size_t err_len);
/* nativeSetCigar: from then on the alignments are returned as CIGARs (swmi_set_option "cigar"): 1 = M / I / D, 2 = '=' / X / I / D,
 * 0 (the default): off.  Any other value is SWMI_ERR_INVALID and leaves the context as it was.
 * nativePairCigar: alignment k of a pair after a run under that option, as swmi_pair_cigar hands it out: *cigar points to *n_cigar
 * entries  len << 4 | op  owned by the batch, *nm is the edit distance, cell[0..1] the alignment's last cell. */
int swmi_shim_set_cigar(swmi_ctx *ctx, int32_t cigar, char *err, size_t err_len);
int swmi_shim_pair_cigar(swmi_batch *b, int64_t pair, int64_t k, int32_t *begin, int32_t cell[2], const uint32_t **cigar,
                         uint32_t *n_cigar, uint32_t *nm, char *err, size_t err_len);

/* nativeSetSubopt: from then on a local run also returns every pair's second-best score (swmi_set_option "subopt"): 1 .. 2^30 = the
 * mask half-width in columns, -1 = max(m / 2, 15) per pair, 0 (the default): off.  Any other value is SWMI_ERR_INVALID and leaves
 * the context as it was.
 * nativePairSubopt: out[0..1] = the pair's second-best score and the reference column it ends in after a run under that option, as
 * swmi_pair_subopt hands them out ((0, 0): none). */
int swmi_shim_set_subopt(swmi_ctx *ctx, int32_t subopt, char *err, size_t err_len);
int swmi_shim_pair_subopt(const swmi_batch *b, int64_t pair, int32_t out[2], char *err, size_t err_len);

/* nativeSetEndBonus: from then on an extend run also returns every pair's best score in the read's last row and takes the pair to the
 * read's end when that is less than the bonus below the best score (swmi_set_option "end_bonus"): 1 .. 2^30 = the bonus, 0 (the
 * default): off.  Any other value is SWMI_ERR_INVALID and leaves the context as it was.
 * nativePairEndScore: out[0..3] = the pair's max_score, end_score and end_col after a run under that option, as swmi_pair_end_score
 * hands them out, and 1 if the pair was taken to the end (SWMI_PAIR_TO_END), else 0. */
int swmi_shim_set_end_bonus(swmi_ctx *ctx, int32_t end_bonus, char *err, size_t err_len);
int swmi_shim_pair_end_score(const swmi_batch *b, int64_t pair, int32_t out[4], char *err, size_t err_len);

/* nativeSetOverlap: 1 = overlap (ends-free) alignment from then on (swmi_set_option "overlap"): a fit run whose read ends are free as
 * well -- the alignment ends in the read's last row or the reference's last column and starts in row 0 or column 0.  Any other run is
 * then refused (SWMI_ERR_UNSUPPORTED).  0 (the default): off.  Any other value is SWMI_ERR_INVALID and leaves the context as it was. */
int swmi_shim_set_overlap(swmi_ctx *ctx, int32_t overlap, char *err, size_t err_len);

/* nativeSetHits: from then on a run under nativeSetSubopt also returns every pair's best local hits with their end cells
 * (swmi_set_option "hits"): 1 .. 16 = the most entries per pair, 0 (the default): off.  Any other value is SWMI_ERR_INVALID and leaves
 * the context as it was.
 * nativePairHits: *n = the pair's count after a run under that option, and out[3 k .. 3 k + 2] = entry k's score, read row and reference
 * column (1-based), as swmi_pair_hits hands them out.  out may be NULL (the count only); cap = the entries out holds, below the count:
 * SWMI_ERR_RANGE. */
int swmi_shim_set_hits(swmi_ctx *ctx, int32_t hits, char *err, size_t err_len);
int swmi_shim_pair_hits(const swmi_batch *b, int64_t pair, int32_t *out, int32_t cap, int32_t *n, char *err, size_t err_len);

/* nativeSetScoreMatrix: a substitution score matrix on this context (swmi_set_score_matrix): `alphabet` = n symbols narrowed to
 * bytes (ISO-8859-1), `scores` = n * n entries, row = read base, column = reference base (n_scores must be n * n).  n = 0 clears
 * it.  Applies to the batches the context aligns from then on (on the affine kernels). */
int swmi_shim_set_score_matrix(swmi_ctx *ctx, const signed char *alphabet, size_t n, const int32_t *scores, size_t n_scores,
                               char *err, size_t err_len);

/* nativeSetReadProfiles: per-read score profiles on a batch nativeAlignBatch returned (swmi_batch_set_read_profiles), and the batch
 * run again under them with the same scores, tie mode and types: `alphabet` = n symbols narrowed to bytes, `scores` = n entries per
 * read byte of the batch in upload order; n_rows = the reads' bytes as the caller uploaded them (readOff[nReads]), and n_scores
 * must be n * n_rows.  n_rows is the CALLER's statement and a precondition: the library has no query for a batch's read bytes, reads
 * n entries per read byte of the batch, and runs past `scores` when n_rows is less than that.  n = 0 clears the profiles and runs the batch without them.  A refused set leaves the batch as it was; a
 * refused run leaves it with the new profiles and without results. */
int swmi_shim_set_read_profiles(swmi_ctx *ctx, swmi_batch *b, int32_t match, int32_t mismatch, int32_t gap, int32_t tie_mode,
                                const signed char *types, size_t types_len, const signed char *alphabet, size_t n,
                                const int32_t *scores, size_t n_scores, int64_t n_rows, char *err, size_t err_len);

/* nativeRefTotal / nativeRefSiteCount / nativeRefSite */
int swmi_shim_ref_total(const swmi_batch *b, int32_t ref, int32_t *total, char *err, size_t err_len);
int swmi_shim_ref_site_count(swmi_batch *b, int32_t ref, int64_t *n, char *err, size_t err_len);
int swmi_shim_ref_site(swmi_batch *b, int32_t ref, int64_t k, int32_t *begin, const char **ref_aln, const char **read_aln,
                       uint32_t *len, char *err, size_t err_len);

/* nativeRefSitesSizes / nativeRefSitesPacked: MapRef's output of the references ref_lo .. ref_hi-1 in ONE call
 * (swmi_ref_sites_packed, include/swmi.h).  The Java side asks for the sizes, allocates its int[] / long[] / byte[] once per
 * partition, and builds every String from a slice of one byte[] -- instead of three JNI calls and two array allocations per
 * match site.  `sizes` receives {number of sites, bytes of all strings}.  Lengths are checked against the arrays' lengths. */
int swmi_shim_ref_sites_sizes(swmi_batch *b, int32_t ref_lo, int32_t ref_hi, int64_t sizes[2], char *err, size_t err_len);
int swmi_shim_ref_sites_packed(swmi_batch *b, int32_t ref_lo, int32_t ref_hi,
                               int32_t *totals, int64_t n_totals, int64_t *degenerate, int64_t n_degenerate,
                               int64_t *site_first, int64_t n_site_first,
                               int32_t *begins, int32_t *lens, int64_t *str_off, int64_t n_sites_cap,
                               signed char *blob, int64_t blob_cap, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif
#endif
