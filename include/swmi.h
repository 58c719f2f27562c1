/*
 * swmi.h -- C ABI of the MI355X-native Smith-Waterman batch aligner (libswmi.so).
 *
 * This is the drop-in boundary for ONE hot path of elizabethfong/SparkSmithWaterman:
 * the matrix fill + tied-maximum search + traceback that
 *     JavaRDD.mapToPair(new MapRef())                 src/sw/Distribution.java:337-338
 *       -> MapRef.call(tuple)                         src/sw/Distribution.java:403-436
 *         -> SmithWaterman.OptAlignments.call(...)    src/sw/SmithWaterman.java:62-92
 * runs once per (reference, read) pair.  The reference has no FFI of its own; the
 * entry points below are what a JNI binding for that seam binds (INTEGRATION.md
 * shows the Java/JNI side).  Plain C types only: pointers, sizes, POD structs.
 *
 * Conventions
 *   - every function returning int returns SWMI_OK (0) or a negative swmi_status;
 *     the message for the last failure on the calling thread: swmi_last_error().
 *   - sequences are byte strings (Java chars narrowed to ISO-8859-1).  Two bases are
 *     equal iff Character.toUpperCase of the two chars is equal, as AlignmentScore
 *     tests (src/sw/SmithWaterman.java:309-318), reproduced exactly for Latin-1.  A JNI
 *     caller holding chars above U+00FF must canonicalise them first.
 *   - a batch is the cross product refs x reads, pair index = ref * n_reads + read:
 *     the order in which MapRef.call loops (Distribution.java:419-426) -- or a pair list
 *     (swmi_batch_upload_pairs), pair index = position in the list.
 *   - a context is bound to one GPU and owns one HIP stream; calls on one context
 *     are serialised internally, use one context per host thread for concurrency
 *     (Spark runs MapRef on every executor thread).
 *   - there is NO CPU fallback: if no gfx950 device / kernel image is usable the
 *     calls fail with SWMI_ERR_NO_DEVICE.
 */
#ifndef SWMI_H
#define SWMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_ABI_VERSION 3

typedef enum swmi_status {
    SWMI_OK               =  0,
    SWMI_ERR_INVALID      = -1,  /* bad argument (null pointer, non-monotone offsets, ...)   */
    SWMI_ERR_NO_DEVICE    = -2,  /* no usable MI355X / HIP runtime error at start-up          */
    SWMI_ERR_HIP          = -3,  /* a HIP call failed; see swmi_last_error()                  */
    SWMI_ERR_NOMEM        = -4,  /* host or device allocation failed                          */
    SWMI_ERR_UNSUPPORTED  = -5,  /* e.g. alignTypes a/i/d not pairwise distinct, len >= 2^30  */
    SWMI_ERR_RANGE        = -6   /* index out of range in an accessor                         */
} swmi_status;

/* What is aligned end to end (swmi_set_option "align_mode"). */
#define SWMI_ALIGN_LOCAL  0  /* Smith-Waterman: any stretch of the read against any stretch of the reference (the default) */
#define SWMI_ALIGN_FIT    1  /* the whole read against any stretch of the reference ("glocal", semi-global)              */
#define SWMI_ALIGN_GLOBAL 2  /* Needleman-Wunsch: the whole read against the whole reference                              */

/* Which reference aligner's tie-breaking is reproduced. */
#define SWMI_TIE_SERIAL 0  /* SmithWaterman.GetCellScore, '>=' chain: a > i > d (SmithWaterman.java:223-249);
                              max cells in row-major order (SmithWaterman.java:157-185)                        */
#define SWMI_TIE_STRICT 1  /* DistributedSW.GetCellScore, '>' chain: d > i > a (DistributedSW.java:305-330);
                              max cells per anti-diagonal, ascending j (DistributedSW.java:209-239), then a
                              stable sort of the alignments by beginning (DistributedSW.java:480)              */

/* alignScores {match, mismatch, gap} and alignTypes {a, i, d, none}: the two arrays
 * OptAlignments.call takes (SmithWaterman.java:47-57); defaults Distribution.java:36-37.
 * Every score sum is a Java int (uint32 wrap-around), for any int32 scores, with one documented deviation: a POSITIVE gap under
 * which some H + gap could pass 2^31 - 1 is SWMI_ERR_UNSUPPORTED before anything is launched.  With s1 the largest and s2 the
 * next smaller positive value among {match, mismatch, gap}, B = 2^31 - 1 and L = the batch's longest read + longest reference,
 * a run needs  min(B, min(L, B / s1) * s1 + min(L, B / s2) * s2) + gap <= B  (integer divisions; the s2 term is 0 without an
 * s2).  gap <= 0 is never refused. */
typedef struct swmi_params {
    int32_t match;       /* default  5 */
    int32_t mismatch;    /* default -3 */
    int32_t gap;         /* default -4 (linear) */
    int32_t tie_mode;    /* SWMI_TIE_SERIAL | SWMI_TIE_STRICT */
    char    types[4];    /* default {'a','i','d','-'}; only used to validate distinctness */
} swmi_params;

typedef struct swmi_ctx    swmi_ctx;     /* per-(thread, device) context                  */
typedef struct swmi_batch  swmi_batch;   /* sequences resident in HBM + device workspaces */

/* ---- library / context --------------------------------------------------------- */
int         swmi_abi_version(void);
const char *swmi_last_error(void);                       /* thread-local, never NULL */
int         swmi_device_count(int *count);
int         swmi_create(int device, swmi_ctx **out);     /* device = HIP ordinal      */
void        swmi_destroy(swmi_ctx *ctx);
void        swmi_default_params(swmi_params *p);

/* Tuning knobs (all optional).  cell_cap: tied-maximum cells kept per pair in the
 * fast path (pairs with more are re-run on the GPU with an exact-size list);
 * max_workspace_bytes: cap on the per-batch workspace arena (larger batches are run in
 * chunks); profiling = 1 brackets every stage with HIP events (sweep, traceback, D2H: three marker packets per run, ~10 us of a
 * 0.17 ms step), 2 only the sweep (two packets; swmi_timing.traceback_ms stays 0), 0 (default) nothing; zero_copy (default 1): kernels
 * write results straight into pinned host memory instead of a D2H copy; device_strings (default 1): the traceback kernels
 * write both aligned strings of every alignment behind its packed ops (from the caller's bytes as uploaded), so the
 * alignment accessors hand out pointers; 0: records carry the 2-bit ops only and the host builds a string when it is asked
 * for (smaller result stream, e.g. when only a few of many alignments will ever be read); mode selects the kernel
 * pipeline -- results are identical in all of them:
 *   1 (default)  the sweep computes scores only, leaves lane-state checkpoints and ONE maximum per
 *                32-step window; the traceback re-sweeps the windows holding the pair's maximum to list
 *                its cells, and the windows each alignment path crosses to get direction bits (into LDS).
 *                Needs mismatch <= 0 and gap <= 0; other scores run as mode 2.
 *   2            as 1, but tied maxima are tracked during the sweep (per-step test + rare handler).
 *   0            the sweep writes the whole 2-bit direction field to HBM and the traceback reads it
 *                (cheaper when most pairs have many tied maxima).  Batches with pairs longer than about
 *                16 k bases (m + n) run as mode 1/2: mode 0's traceback tiles leave too little LDS for them.
 *  -1            the same as 1 (kept for callers that passed "automatic").
 * tb_split: grain of the mode-1 traceback.  0: one workgroup per pair (lists the maximum cells, then up to four waves walk
 *                the alignments, the others re-sweep windows for them) -- best when pairs have one or a few alignments;
 *                1: split -- one wavefront per checkpoint window lists cells, one wavefront per alignment walks; -1
 *                (default): split for launches of fewer than 64 pairs, and for batches of up to 256 pairs in which a sample
 *                of the pairs (aligned once, on the first run of a batch) averages >= auto_ties_x100 / 100 tied maxima
 *                per pair -- periodic references, the reference's own EngineerData sets.
 * resident: -1 (default) pairs whose whole direction field fits 20 KB of LDS and whose reference is at most 8 x the read
 *                (80 bp reads x 400 bp references, the reference's EngineerData shapes) are handled start to finish by one
 *                wavefront -- two sweeps inside LDS, all alignments walked at once, one per lane; 0 never; 1 whenever the
 *                field fits 40 KB.
 * tfused: 1: the usual pair -- fast symbols on both sides, scores within int4, gap < 0, a read of at most 256 bases, a reference
 *                of at most 2560 -- is swept in the TRANSPOSED layout (reference columns on the lanes, the read streaming
 *                through) and traced back in the same launch (sw_tfused_kernel: block tasks and walk items shared by the
 *                wavefronts of a workgroup); 0 or -1 (default): never -- measured slower than the two-kernel pipeline.
 * scores_only (default 0): 1 = the sweep only: every pair's score and MapRef's totals (swmi_pair_score, swmi_ref_total(s),
 *                swmi_stream_totals, swmi_batch_pair_results with n_alignments = NULL); the tied-maximum lists and the alignments
 *                are not computed and their accessors fail.  For a driver that reduces to the winning references first and aligns
 *                only those in full (the reference's driver discards every other reference's alignments, Distribution.java:341-353).
 * stream_keep_records (default 1): 0 = a stream drops every chunk's alignment records once its scores, counts and totals are
 *                taken -- for a driver that reduces to the winning references and aligns those again (Distribution.java:341-353
 *                discards every other reference's alignments too); the alignment accessors of such chunks fail.
 * gap_open (default 0, must be <= 0, else SWMI_ERR_INVALID): affine gaps -- a gap of length k costs gap_open + k * gap (gap is then the
 *                per-base extension).  A run with gap_open != 0 takes the affine kernels (swmi_affine.hip; swmi_batch_mode = 3): the Gotoh
 *                recurrence with the same tie chains, maximum cells and walk order as the linear path.  Bounds:
 *                gap <= 0, |match|, |mismatch|, |gap|, |gap_open| <= 2^20, reads of at most 1024 bases; outside them the run returns
 *                SWMI_ERR_UNSUPPORTED before anything is launched.  scores_only, device_strings, zero_copy, cell_cap, max_workspace_bytes,
 *                arena_words_per_pair and profiling apply to affine runs; mode, tb_split, resident, tfused, col_chunks and debug_* do not.
 * affine: -1 (default) the affine kernels only when gap_open != 0; 1 always, also at gap_open = 0 (where they give the linear results).
 * align_mode (default SWMI_ALIGN_LOCAL; any value but the three is SWMI_ERR_INVALID and leaves the context as it was): SWMI_ALIGN_FIT aligns
 *                the WHOLE read against any stretch of the reference, SWMI_ALIGN_GLOBAL the whole read against the whole reference -- the
 *                Gotoh recurrence of gap_open without the floor at 0, with H(i,0) = gap_open + i * gap and H(0,j) = 0 (fit) or
 *                gap_open + j * gap (global); the pair's score is the maximum of the last read row (fit: every tied column is a maximum
 *                cell, ascending) or H(m,n) (global), and may be zero or negative: SWMI_PAIR_DEGENERATE is never set.  Every alignment spells
 *                the whole read (and, global, the whole reference); `begin` is the 1-based column of the first reference base it consumes
 *                (the end column if it consumes none).  Such a run takes the affine kernels whatever gap_open / affine say (swmi_batch_mode
 *                = 3), with or without a matrix, within the affine bounds; global mode also needs
 *                3 * |gap_open| + (64 * ceil(m / 64) + n) * |gap| <= 2^31 for the longest read m and reference n of the batch, else
 *                SWMI_ERR_UNSUPPORTED before anything is launched.  A pair with an empty side scores 0 with no alignments in every mode.
 *                A run (async runs and stream slots included) takes the value set when it was asked for.
 * long_reads (default 0; any value but 0 and 1 is SWMI_ERR_INVALID and leaves the context as it was): 1 lets a run on the affine kernels
 *                (gap_open, affine, a score matrix, align_mode) take reads of MORE than 1024 bases: such a read is swept in strips of
 *                1024 rows by the same wavefront and walked across the strips; reads of at most 1024 bases in the
 *                same batch take the kernels they take today.  The rule "reads of at most 1024 bases" is then a rule on sums.  With m
 *                the batch's longest read, M = 1024 * ceil(m / 1024) for m > 1024 and 64 * ceil(m / 64) otherwise (the rows a sweep
 *                computes), and S = the largest of |match|, |mismatch|, |gap|, |gap_open| and the |entries| of the score matrix, a run
 *                needs  M * S <= 2^30;  global mode needs 3 * |gap_open| + (M + n) * |gap| <= 2^31 with this M; a pair's direction field
 *                (4 * ceil(m / 1024) * ceil((n + 63) / 8) KiB for m > 1024) must fit max_workspace_bytes; the traceback's bound on a
 *                pair's longest path (587,760 moves) stays.  Outside them SWMI_ERR_UNSUPPORTED before anything is launched.  The other
 *                affine bounds (gap <= 0, |scores| <= 2^20) stay; at S = 2^20 the rule is today's M <= 1024.  With 0 nothing changes:
 *                a read of more than 1024 bases is SWMI_ERR_UNSUPPORTED.  A run (async runs and stream slots included) takes the value
 *                set when it was asked for.
 * band (default 0 = no band and no change; 1 .. 2^20 = the half-width w in columns; any other value is SWMI_ERR_INVALID and leaves the
 *                context as it was): a read of MORE than 1024 bases (so long_reads = 1 is needed for there to be any) is aligned inside
 *                a band around the diagonal j = i only.  The band is a staircase with the sweep's strip height: row i (1-based) is in
 *                strip s = (i - 1) / 1024, and cell (i, j) exists iff  max(1, 1024 s + 1 - w) <= j <= min(n, 1024 (s + 1) + w)  -- every
 *                cell with |j - i| <= w, rounded outwards to strips.  A cell outside does not exist: in local mode its H, E and F read as
 *                0 and it is never a maximum cell; in fit and global mode they read as -infinity.  Inside, everything is as without a
 *                band, in global coordinates; fit mode takes its maximum over the in-band columns of row m; local mode with maximum 0
 *                counts the IN-BAND cells in n_cells.  A pair whose read has at most 1024 bases is computed in full by the kernels it
 *                takes today: cut its reference for the same effect.  A run with band > 0 takes the affine kernels whatever gap_open /
 *                affine say (swmi_batch_mode = 3).  Refused with SWMI_ERR_UNSUPPORTED before anything is launched, for the batch's
 *                longest read m (NS = ceil(m / 1024), M = 1024 NS) and the extreme references: a strip with an empty window
 *                (n < 1024 (NS - 1) + 1 - w); global mode with (m, n) outside the band (n > 1024 NS + w, NS of the shortest long read);
 *                fit and global mode unless  M * S <= 2^29  (S as under long_reads; local mode keeps M * S <= 2^30); global mode unless
 *                3 * |gap_open| + (M + n) * |gap| <= 2^30; a pair whose banded direction field (4 KiB per 8-step block, strip s has
 *                ceil((window + 63) / 8) blocks) is over max_workspace_bytes -- the chunking sees the smaller field, so a pair that did
 *                not fit without a band may fit with one.  scores_only, device_strings, zero_copy, cell_cap and profiling apply as to
 *                any affine run.  A run (async runs and stream slots included) takes the value set when it was asked for (DESIGN.md
 *                section 8f).
 * extend (default 0; any value but 0 and 1 is SWMI_ERR_INVALID and leaves the context as it was): 1 turns a run with align_mode =
 *                SWMI_ALIGN_GLOBAL into SEED EXTENSION (ksw2's extz, BWA-MEM's extension step): the alignment is anchored at the start
 *                of the read and of the reference, runs along the diagonal, and ends at the cell with the best score, the tail of the
 *                read or of the reference left unaligned.  E, F, H, the x bits, the tie chains and the boundaries are global mode's
 *                (H(0,0) = 0, H(0,j) = gap_open + j * gap, H(i,0) = gap_open + i * gap, no floor at 0); the pair's score is the maximum
 *                of H(i,j) over 1 <= i <= m, 1 <= j <= n -- under band, over the in-band cells of a long read -- and every tied cell is
 *                a maximum cell, in local mode's order (serial tie mode row-major; strict per anti-diagonal with ascending j, then
 *                the stable sort by begin), with cell_cap, the exact-size re-run and the other affine options as for local and fit
 *                lists.  Row 0 and column 0 do not compete: the library reports the best NON-EMPTY extension, so the score may be zero
 *                or negative (SWMI_PAIR_DEGENERATE is never set), and a score <= 0 tells the caller that not extending at all (score 0)
 *                is no worse.  The walk is global mode's, started at the maximum cell (i, j): the alignment spells exactly read[:i] and
 *                ref[:j], `begin` is 1, and end_i / end_j of swmi_pair_alignment are the maximum cell.  For LEFT extension reverse both
 *                sequences.  The bounds are global mode's, unchanged (the affine bounds, 3 * |gap_open| + (M + n) * |gap| <= 2^31, under
 *                long_reads M * S <= 2^30, under band M * S <= 2^29 and 3 * |gap_open| + (M + n) * |gap| <= 2^30, no strip with an empty
 *                window), but for one: the end cell is free, so a banded extend run does NOT need (m, n) inside the band and takes a
 *                reference longer than 1024 NS + w.  extend = 1 with any other align_mode is SWMI_ERR_UNSUPPORTED before anything is
 *                launched.  With 0 nothing changes.  A run (async runs and stream slots included) takes the value set when it was asked
 *                for.
 * xdrop (default 0 = off and no change; 1 .. 2^31 - 1 = the threshold X; any other value is SWMI_ERR_INVALID and leaves the context
 *                as it was): the DROP-OFF rule of an extend run (ksw2's zdrop, BWA-MEM's and BLAST's X-drop), at the granularity of the
 *                sweep's strips.  It acts on pairs whose read has MORE than 1024 bases (so long_reads = 1 is needed for there to be
 *                any), with or without band, with or without a score matrix, in both tie modes; a pair whose read has at most 1024
 *                bases is computed in full by the kernels it takes today -- the same rule as for band.  For a read of m > 1024 bases,
 *                NS = ceil(m / 1024) strips with the windows c_lo(s) .. c_hi(s) of option band ((1, n) without one), and
 *                s = 0 .. NS - 2:  best(s) = the maximum of H(i, j) over the existing cells with 1 <= i <= 1024 (s + 1), j >= 1 (the
 *                extend run's running maximum after strip s);  seam(s) = the maximum of H(1024 (s + 1), j) over c_lo(s) <= j <=
 *                c_hi(s).  The sweep stops behind the first strip s* with  best(s*) - seam(s*) > X  (strict; the difference is taken
 *                exactly, not in int32): strips s* + 1 .. are not swept, the pair's score is best(s*), its maximum cells are the
 *                cells of rows i <= 1024 (s* + 1) that tie at it, in extend's order, each walked as extend walks it (begin = 1).
 *                That is the extend result of (ref, read[:1024 (s* + 1)]) under the same band (for s* = 0 without a band: a read of
 *                1024 bases is not banded).  Without such a strip the result is exactly the extend result.  No flag is set: flags
 *                stays 0, and swmi_pair_rows_swept tells a stopped pair.  No gap-length term is added to X as ksw2 adds one to zdrop
 *                (it needs one anchor cell; the maximum here is a list of tied cells).  cell_cap, the exact-size re-run (it stops at
 *                the same strip), scores_only, device_strings and zero_copy apply as to any extend run; the bounds and refusals are
 *                extend's, unchanged -- a strip with an empty window is refused even where a stop would never reach it.  xdrop > 0 on
 *                a run that is not an extend run (align_mode global with extend = 1) is SWMI_ERR_UNSUPPORTED before anything is
 *                launched.  A run (async runs and stream slots included) takes the value set when it was asked for (DESIGN.md
 *                section 8h).
 * band_adapt (default 0 = off and no change; 1 = on; any other value is SWMI_ERR_INVALID and leaves the context as it was): the band
 *                of a banded extend run FOLLOWS THE ALIGNMENT from strip to strip (libgaba's adaptive band, at the granularity of the
 *                sweep's strips), so that the half-width w = band only has to cover the drift inside one strip of 1024 rows, not the
 *                drift over the whole read.  It is an option of a banded extend run -- band > 0, align_mode global, extend = 1: on any
 *                other run (the linear pipeline included) band_adapt = 1 is SWMI_ERR_UNSUPPORTED before anything is launched.  Like band
 *                it acts on pairs whose read has MORE than 1024 bases (so long_reads = 1 is needed for there to be any); a shorter
 *                read is computed in full by the kernels it takes today.  For a read of m > 1024 bases, NS = ceil(m / 1024) strips,
 *                each with a centre, starting from c(-1) = 0:
 *                  c_lo(s) = max(1, c(s - 1) + 1 - w),  c_hi(s) = min(n, c(s - 1) + 1024 + w)     (strip 0: the static window)
 *                  p(s) = the smallest column j in c_lo(s) .. c_hi(s) at which H(1024 (s + 1), j) is largest,  s <= NS - 2
 *                  c(s) = max(c(s - 1), p(s))                                         (the centre never moves left)
 *                Both window ends are non-decreasing in s, a window has at most 1024 + 2 w columns, p(s) lies in the windows of
 *                strips s and s + 1, and no window is empty (c(s) <= n): band's refusal of a strip with an empty window does not
 *                apply, and a reference shorter than the read is taken, its last windows ending at n.  Everything else is band's
 *                contract for an extend run with these windows: a cell outside its strip's window does not exist and reads as
 *                -infinity (also column c_lo - 1 on the row above a strip whose window did not move, c_lo(s + 1) = c_lo(s) > 1); the
 *                score is the maximum over the existing cells; tied cells come in extend's order; the walk is the global walk;
 *                begin = 1.  cell_cap, the exact-size re-run (it places the same windows), scores_only, device_strings and zero_copy
 *                apply as to any extend run.  With xdrop > 0 the drop-off test runs on these windows (seam(s) over c_lo(s) .. c_hi(s))
 *                and comes first: behind a stop no further window is placed.  Bounds, for the batch's longest read (M = 1024 NS) and
 *                longest reference, refused with SWMI_ERR_UNSUPPORTED before anything is launched:  M * S <= 2^29  as under band, and
 *                (2 NS + 1) * |gap_open| + (M + n) * |gap| <= 2^30  in place of band's 3 * |gap_open| + (M + n) * |gap| <= 2^30 (an
 *                existing cell is reached from the boundary by gap moves with two gap openings per strip, not by a diagonal); a
 *                pair's workspace -- NS fields of ceil((min(n, 1024 + 2 w) + 63) / 8) blocks of 4 KiB, whatever the windows turn out to
 *                be, and a table of NS window centres -- must fit max_workspace_bytes.  swmi_pair_band_window tells the windows a
 *                pair's sweep used.  A run (async runs and stream slots included) takes the value set when it was asked for
 *                (DESIGN.md section 8i).
 * gap_open2 (default 0 = off and no change; a value > 0 or < INT32_MIN is SWMI_ERR_INVALID and leaves the context as it was) and
 * gap2 (default 0; a value > 0 or < INT32_MIN is SWMI_ERR_INVALID likewise): TWO-PIECE AFFINE GAPS (minimap2's scoring, ksw2's extd2)
 *                on global and extend runs.  A run is a two-piece run iff gap_open2 != 0; gap2 is then the second piece's per-base
 *                extension, and with gap_open2 = 0 gap2 is not read.  With o1 = gap_open, e1 = gap, o2 = gap_open2, e2 = gap2 a gap
 *                of length k costs  max(o1 + k * e1, o2 + k * e2)  -- piece 1 cheap to open and steep, piece 2 dear to open and flat,
 *                though no order between the pieces is required and o1 = 0 is allowed.  The recurrence is global mode's (no floor at
 *                0) with each gap state twice, p = 1, 2:
 *                  Ep(i,j) = max(H(i,j-1) + op + ep, Ep(i,j-1) + ep),  xEp = 1 iff the extension is strictly better;  Fp, xFp with row i-1
 *                  E = max(E1, E2), pE = 1 iff E2 > E1 (piece 1 wins a tie, in both tie modes);  F, pF likewise
 *                  H from E, F and the diagonal by the two tie chains, unchanged (serial '>=' a > i > d, strict '>' d > i > a)
 *                  H(0,0) = 0,  H(0,j) = max(o1 + j * e1, o2 + j * e2),  H(i,0) the same in i;  the gap states of row 0 and column 0
 *                  are H + op, so that the first real cell opens (x = 0, value H + op + ep)
 *                The walk is the global walk with five states: H reads the direction; a deletion enters E2 iff pE, else E1; an
 *                insertion F2 iff pF, else F1; a gap state stays while its own x bit is set.  An extend run lists its tied maximum
 *                cells in extend's order and walks each.  Scope: align_mode global with and without extend, reads of every length
 *                (long_reads, with and without band), both tie modes; scores_only, device_strings, zero_copy, cell_cap, the exact-size
 *                re-run and chunking under max_workspace_bytes apply as to any global run, and swmi_batch_mode reports 3.  With
 *                gap_open2 != 0 these are SWMI_ERR_UNSUPPORTED before anything is launched: align_mode local or fit; a score matrix;
 *                xdrop > 0; band_adapt = 1.  The bounds are global mode's, read with |gap_open| = max(|o1|, |o2|) and |gap| =
 *                max(|e1|, |e2|); S also covers |o2| and |e2|; |o2|, |e2| <= 2^20 and gap2 <= 0.  A pair's direction field and seam row
 *                are twice the one-piece size (the chunking and the refusal of a pair over max_workspace_bytes see the doubled field).
 *                Unlike gap_open, both are run modes: a run (async runs and stream slots included) takes the values set when it was
 *                asked for.
 * cigar (default 0 = off and no change; 1 = M / I / D; 2 = '=' / X / I / D; any other value is SWMI_ERR_INVALID and leaves the context
 *                as it was): the traceback kernels write every alignment as a run-length CIGAR with its edit distance instead of
 *                strings or packed ops, read with swmi_pair_cigar.  An entry is BAM's,  len << 4 | op  (SWMI_CIGAR_M, _I, _D, _EQ, _X);
 *                I consumes a read base (the column whose reference string has '_'), D a reference base.  Entries run from the START
 *                of the alignment to its end cell: the order of the aligned strings, the reverse of the walk.  Adjacent entries
 *                never have the same op; under cigar = 1 '=' and X merge into M.  Two bases are EQUAL by the library's own rule,
 *                Character.toUpperCase equality on ISO-8859-1 (equal canonical codes), whatever they score: under a score matrix an
 *                identical pair with a negative entry is still '=', a positively scored substitution still X.  nm = X columns +
 *                inserted + deleted bases (SAM's NM), under cigar = 1 too.  len < 2^28 always: an alignment has at most 587,760
 *                columns.  A run with cigar != 0 takes the affine kernels whatever gap_open / affine say (swmi_batch_mode = 3); with
 *                gap_open = 0 it gives the linear pipeline's scores and alignments.  The record payload is then the CIGAR:
 *                device_strings is not read.  scores_only = 1 wins (no records).  Every other accessor works as with device_strings
 *                = 0 -- the host expands the CIGAR where it expanded the ops -- and returns what the same run with cigar = 0 returns,
 *                strings with the caller's original case included.  zero_copy, cell_cap, max_workspace_bytes, arena_words_per_pair,
 *                profiling, every affine option (align_mode, long_reads, band, extend, xdrop, band_adapt, gap_open2 / gap2, a score
 *                matrix), pair lists and streams apply unchanged; the bounds and refusals are those of the affine run it becomes.
 *                A run (async runs and stream slots included) takes the value set when it was asked for.
 * subopt (default 0 = off and no change; 1 .. 2^30 = the mask half-width w in columns; -1 = SWMI_SUBOPT_AUTO, per pair w =
 *                max(floor(m / 2), 15), m the read's length -- SSW's maskLen; any other value is SWMI_ERR_INVALID and leaves the context
 *                as it was): a local run also returns every pair's SECOND-BEST score, the best score of an alignment that ends
 *                somewhere else in the same reference (BWA's score2 / te2 under KSW_XSUBO, SSW's score2 / ref_end2), read with
 *                swmi_pair_subopt.  With s the pair's score: colmax(j) = the maximum of H(i, j) over the existing cells of column j,
 *                1 <= i <= m (under band a cell outside its strip's window does not exist; a column with no existing cell has colmax
 *                0); j* is a maximum column iff colmax(j*) = s -- exactly the columns of the pair's tied maximum cells, whatever
 *                cell_cap is; column j is eligible iff |j - j*| > w for EVERY maximum column (strict, as in SSW); score2 = the largest
 *                colmax over the eligible columns, 0 if there are none; end2 = the smallest eligible column with colmax = score2 if
 *                score2 > 0, else 0.  So 0 <= score2 < s, or both are 0; a degenerate pair (s = 0) and a pair with an empty side give
 *                (0, 0).  The values do not depend on the tie mode, on cell_cap, on chunking, or on whether the pair was re-run.
 *                Scope: align_mode local, with and without a score matrix, both tie modes, reads of every length (long_reads, with
 *                and without band).  A run with subopt != 0 takes the affine kernels whatever gap_open / affine say (swmi_batch_mode =
 *                3); with gap_open = 0 it gives the linear pipeline's scores and alignments.  subopt != 0 with align_mode fit or
 *                global (so also extend, xdrop, band_adapt, gap_open2) is SWMI_ERR_UNSUPPORTED before anything is launched.
 *                scores_only, cigar, device_strings, zero_copy, cell_cap, max_workspace_bytes, profiling, pair lists and streams apply
 *                unchanged, and every other accessor returns what the same run with subopt = 0 returns.  The sweep keeps one row of n
 *                int32 column maxima per pair behind the pair's direction field (charged to max_workspace_bytes with it).  A run
 *                (async runs and stream slots included) takes the value set when it was asked for.
 * hits (default 0 = off and no change; 1 .. 16 = K, the most entries a pair returns; any other value is SWMI_ERR_INVALID and leaves
 *                the context as it was): a run under subopt also returns every pair's K BEST LOCAL HITS WITH THEIR END CELLS, read
 *                with swmi_pair_hits: what a mapper anchors the reverse pass on (SSW's ref_end1 / read_end1, BWA's te / qe), and the
 *                next few peaks for repeats, secondary and supplementary alignments.  hits != 0 needs subopt != 0, which gives the
 *                mask half-width w (fixed, or SWMI_SUBOPT_AUTO per pair); with subopt = 0 the run is SWMI_ERR_UNSUPPORTED before
 *                anything is launched, and so are the runs subopt refuses (fit, global, extend, xdrop, band_adapt, gap_open2).  In
 *                subopt's terms, for a pair with both sides non-empty and score s > 0: row(j) = the smallest row i, 1 <= i <= m,
 *                whose existing cell has H(i, j) = colmax(j).  Entry 0, the primary: score = s, end_j = the smallest maximum column,
 *                end_i = row(end_j).  Entry k, 1 <= k < K: column j is eligible iff |j - c| > w for EVERY maximum column c and for
 *                c = end_j of every entry 1 .. k - 1 (strict, 64-bit arithmetic); score = the largest colmax over the eligible
 *                columns -- if that is 0 the list ends at k entries; end_j = the smallest eligible column that holds it, end_i =
 *                row(end_j).  So entry 1 is exactly (score2, end2) of swmi_pair_subopt, scores do not increase from entry 1 on, and
 *                any two listed columns are more than w apart.  A degenerate pair (s = 0) and a pair with an empty side have 0
 *                entries.  The values do not depend on the tie mode, on cell_cap, on chunking, or on whether the pair was re-run;
 *                swmi_pair_subopt and every other accessor return what the same run with hits = 0 returns.  Everything subopt's
 *                scope names applies unchanged.  The sweep keeps a second row of n int32 per pair behind the row of column maxima
 *                (charged to max_workspace_bytes with it).  A run (async runs and stream slots included) takes the value set when
 *                it was asked for.
 * end_bonus (default 0 = off and no change; 1 .. 2^30 = the bonus b; any other value is SWMI_ERR_INVALID and leaves the context as
 *                it was): an extend run (align_mode global, extend = 1) also returns, per pair, the best score of an extension that
 *                reaches the END OF THE READ, and takes that extension when it is less than b worse than the best one anywhere
 *                (BWA-MEM's gscore / pen_clip, ksw2's mqe / minimap2's end_bonus: no soft clip for one mismatch near the read's end).
 *                For a pair with both sides non-empty: max_score = the maximum of H(i, j) over the existing cells, the score of the
 *                run without the option; end_score = the maximum of H(m, j) over the existing cells of read row m (under band the
 *                columns of the last strip's window of a long read, else 1 .. n; no window is empty, so the row has a cell;
 *                end_score may be <= 0); end_col = the smallest (1-based) column that holds end_score.  The pair is taken TO THE END
 *                iff (int64) end_score + b > (int64) max_score -- strict, minimap2's rule and BWA-MEM's gscore > max - pen_clip.  A
 *                pair taken to the end has the score end_score, exactly one maximum cell (m, end_col) and one alignment, the global
 *                walk from that cell: it spells the whole read and ref[:end_col], begin = 1, end_i = m, end_j = end_col; and
 *                SWMI_PAIR_TO_END is set in the flags of swmi_pair_n_alignments.  One cell is listed, not every tied column, so the
 *                exact-size re-run never applies to such a pair.  A pair not taken returns exactly what the run without the option
 *                returns: score, tied cells in extend's order, flags 0, cell_cap and the re-run.  A pair with an empty side gives
 *                score 0, no alignments and (0, 0, 0).  swmi_pair_end_score reads the three values, max_score whether or not the pair
 *                was taken.  Scope: one-piece extend runs, reads of every length (long_reads, with and without band), with and
 *                without a score matrix, both tie modes; scores_only, cigar, device_strings, zero_copy, cell_cap,
 *                max_workspace_bytes, pair lists and streams apply unchanged.  end_bonus != 0 on a run that is not an extend run
 *                (the linear pipeline included), or with xdrop > 0, band_adapt = 1 or gap_open2 != 0, is SWMI_ERR_UNSUPPORTED before
 *                anything is launched.  The bounds are extend's, unchanged: the comparison is made in 64 bits and no new sum is formed
 *                in int32.  A run (async runs and stream slots included) takes the value set when it was asked for (DESIGN.md
 *                section 8o).
 * overlap (default 0; any value but 0 and 1 is SWMI_ERR_INVALID and leaves the context as it was): 1 turns a run with align_mode =
 *                SWMI_ALIGN_FIT into OVERLAP (ends-free, dovetail) alignment: fit frees the reference's ends, the option frees the
 *                read's as well (parasail's sg; read overlaps, paired-end merging, adapter trimming).  E, F, the x bits and the tie
 *                chains are fit mode's, with no floor at 0.  Boundaries: H(0,j) = 0 for j = 0 .. n and H(i,0) = 0 for i = 1 .. m;
 *                E(i,0) = F(0,j) = -inf.  The score is the maximum of H over the COMPETING cells (m, j), 1 <= j <= n, and (i, n),
 *                1 <= i <= m -- the read's last row and the reference's last column; row 0 and column 0 do not compete, so the score
 *                is that of the best non-empty overlap, may be <= 0 (no overlap worth having) and SWMI_PAIR_DEGENERATE is never
 *                set.  Every competing cell that holds the score is a maximum cell, (m, n) once, in local and extend mode's order
 *                restricted to those cells: row-major in serial tie mode; per anti-diagonal with ascending j in strict mode, then
 *                the stable sort by begin.  cell_cap and the exact-size re-run apply as to fit's list.  The walk starts at a
 *                maximum cell and ends at the first cell of row 0 or column 0, where nothing is appended: the alignment spells
 *                read[i0+1 .. end_i] against ref[j0+1 .. end_j] with i0 = 0 or j0 = 0 -- no inserted read head, no deleted reference
 *                head.  begin is fit's: the column of the first reference base consumed, end_j if the alignment consumes none.  The
 *                read's first base used is end_i - (read bases consumed) + 1, which the strings or the CIGAR give.  A pair with an
 *                empty side scores 0 with no alignments.  Scope: reads of every length (long_reads), with and without a score
 *                matrix, both tie modes; scores_only, cigar, device_strings, zero_copy, cell_cap, max_workspace_bytes, pair lists
 *                (SWMI_SPEC_REVERSE and SWMI_SPEC_READ_REVCOMP included: overlaps between reads of opposite strands), set_pairs and
 *                streams apply as to a fit run.  The run takes the affine kernels whatever gap_open says (swmi_batch_mode 3).
 *                overlap = 1 with another align_mode, or with band != 0, extend, xdrop, band_adapt, gap_open2, subopt, hits or
 *                end_bonus, is SWMI_ERR_UNSUPPORTED before anything is launched.  The bounds are fit's, unchanged.  A run (async
 *                runs and stream slots included) takes the value set when it was asked for.
 * Further knobs: spin_us (how long a run polls its stream before it blocks, default 2000); col_chunks (0 automatic,
 * 1 never, N > 1 force up to N column chunks per pair: a launch of few pairs with long references is swept by several
 * wavefronts per pair -- a read of more than 256 rows by several strip pipelines); debug_strip_spins / debug_reverse_strips (tests of the strip pipeline's give-up path);
 * debug_async_delay_us (0 .. 10^7, default 0: the async worker waits this long before it starts a run -- a test of what a run takes
 * when it is asked for, not when it starts). */
int         swmi_set_option(swmi_ctx *ctx, const char *name, int64_t value);

/* Substitution score matrix.  alphabet: n bytes, 1 <= n <= 64, pairwise distinct after canonicalisation
 * (Character.toUpperCase on ISO-8859-1: 'a' and 'A' are one symbol, and a matrix on 'A' also scores 'a'); scores[i * n + j] is the
 * score of READ base alphabet[i] against REFERENCE base alphabet[j] (row = read, column = reference; asymmetric matrices are
 * allowed).  A cell whose two bases are both in the alphabet takes the matrix entry; any other cell scores as before: match when
 * the bases are equal, else mismatch.  n = 0 (the pointers may be NULL) clears the matrix.  Duplicate symbols, n > 64 or an
 * entry with |entry| > 2^20 return SWMI_ERR_INVALID and leave the context as it was.
 * A run with a matrix takes the affine kernels whatever gap_open / affine say (swmi_batch_mode = 3), with the affine bounds: reads
 * of at most 1024 bases, gap <= 0, |match|, |mismatch|, |gap|, |gap_open| <= 2^20 -- outside them SWMI_ERR_UNSUPPORTED before
 * anything is launched.  A run uses the matrix set when it was asked for (swmi_batch_run, swmi_batch_run_async, swmi_stream_open
 * for all of a stream's chunks); setting another one later does not change it.  Without a matrix nothing changes. */
int         swmi_set_score_matrix(swmi_ctx *ctx, const uint8_t *alphabet, uint32_t n, const int32_t *scores);

/* ---- staged path: upload once, run many times (what bench.py times) ------------- */
/* ref_off/read_off have n+1 entries, off[0] == 0, non-decreasing; lengths < 2^30.  */
int  swmi_batch_upload(swmi_ctx *ctx,
                       const uint8_t *ref_bytes, const uint64_t *ref_off, uint32_t n_refs,
                       const uint8_t *read_bytes, const uint64_t *read_off, uint32_t n_reads,
                       swmi_batch **out);
/* ---- pair lists: chosen segments of uploaded sequences, one batch ------------------ */
/* A mapper's work list is not a cross product but a list of (reference window, read segment) pairs, windows overlapping,
 * the left extension of a seed running over both sequences reversed.  swmi_batch_upload_pairs uploads the SOURCE sequences
 * once (ref_off / read_off as for swmi_batch_upload) and a list of specs; a gfx950 kernel cuts, reverses and encodes the
 * segments from the resident sources.  Pair k of such a batch is spec k, swmi_batch_n_pairs returns
 * n_pairs, and the result of pair k is, bit for bit, what a one-pair batch of swmi_batch_upload returns for the two segments
 * cut -- and under SWMI_SPEC_REVERSE reversed -- by the caller: score, flags, n_alignments, every alignment's begin / end_i /
 * end_j and both strings with the caller's original case, swmi_pair_rows_swept and swmi_pair_band_window, under every option
 * and pipeline the context selects.  The bounds a run checks on "the batch's longest read / reference" are read over the
 * segments.  COORDINATES ARE THE SEGMENT'S: column j (1-based) of pair k is source byte  ref_start + j - 1  of the reference,
 * or  ref_start + ref_len - j  when the pair is reversed; row i maps to the read's bytes in the same way.  A pair with an empty
 * segment scores 0 with no alignments.
 * THE MINUS STRAND: under SWMI_SPEC_READ_REVCOMP the READ segment is taken reverse-complemented and the
 * reference segment is untouched; the caller uploads each read once, for both strands.  The flag combines with
 * SWMI_SPEC_REVERSE.  With R = the REVERSE bit and C = the READ_REVCOMP bit:
 *      reference segment:  byte order reversed iff R,         never complemented
 *      read segment:       byte order reversed iff R xor C,   complemented iff C
 * so REVERSE | READ_REVCOMP is the left extension on the minus strand: the reference reversed, the read complemented in its own
 * order.  Column j is source byte  ref_start + j - 1,  or  ref_start + ref_len - j  under R; row i is read source byte
 * read_start + i - 1  when the read's order is forward (R == C) and  read_start + read_len - i  when it is reversed (R != C).
 * The complement is a 256-entry byte table: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H; S, W and N map to themselves; U maps to A;
 * the same for the lower-case letters, which stay lower-case; every other byte maps to itself.  It is applied BEFORE the
 * canonical codes: the fast path, a score matrix's rows (row = read base), option "cigar" 2's = / X and the read string of an
 * alignment (with its case) all see the complemented base.  The contract above holds with "and reverse-complemented under
 * SWMI_SPEC_READ_REVCOMP" added: pair k gives what a one-pair swmi_batch_upload batch gives for the two transformed segments.
 * Refused with SWMI_ERR_INVALID before anything is uploaded or launched, the message naming the pair: a source index out of
 * range, start + len past the end of the source, a flag bit other than SWMI_SPEC_REVERSE and SWMI_SPEC_READ_REVCOMP (0x2 is undefined), reserved != 0, specs == NULL with
 * n_pairs > 0.  n_pairs >= 2^32 is SWMI_ERR_UNSUPPORTED; the segments' images together are subject to the 16 GiB image rule.
 * n_pairs = 0 is a valid, empty batch.  The MapRef views (swmi_ref_total(s), swmi_ref_n_match_sites, swmi_ref_match_site,
 * swmi_ref_sites_packed) have no meaning without the cross product and return SWMI_ERR_UNSUPPORTED on such a batch. */
#define SWMI_SPEC_REVERSE 0x1u          /* both segments are taken in reverse byte order (left extension); no complement */
#define SWMI_SPEC_READ_REVCOMP 0x4u     /* the pair is on the minus strand: the read segment reverse-complemented, the reference untouched */
#define SWMI_SPEC_WHOLE   0xFFFFFFFFu   /* as ref_len / read_len: from the start given to the end of the source */
typedef struct swmi_pair_spec {         /* 32 bytes */
    uint32_t ref, read;                 /* indices of the uploaded reference / read                      */
    uint32_t ref_start, ref_len;        /* 0-based first byte and length of the reference segment        */
    uint32_t read_start, read_len;
    uint32_t flags;                     /* SWMI_SPEC_REVERSE | SWMI_SPEC_READ_REVCOMP, or 0               */
    uint32_t reserved;                  /* 0                                                             */
} swmi_pair_spec;
int  swmi_batch_upload_pairs(swmi_ctx *ctx,
                             const uint8_t *ref_bytes, const uint64_t *ref_off, uint32_t n_refs,
                             const uint8_t *read_bytes, const uint64_t *read_off, uint32_t n_reads,
                             const swmi_pair_spec *specs, uint64_t n_pairs, swmi_batch **out);
/* Replaces the list on the same resident sources (left extensions, then right extensions; a second round under another
 * band): the old results are dropped and the batch is to be run again.  A refused list leaves the batch as it was.  On a
 * batch made by swmi_batch_upload: SWMI_ERR_INVALID. */
int  swmi_batch_set_pairs(swmi_ctx *ctx, swmi_batch *b, const swmi_pair_spec *specs, uint64_t n_pairs);
/* spec `pair` of the batch, SWMI_SPEC_WHOLE resolved to a length.  On a cross-product batch: SWMI_ERR_INVALID. */
int  swmi_batch_pair_spec(const swmi_batch *b, uint64_t pair, swmi_pair_spec *spec);

/* ---- per-read score profiles (position-specific scoring matrices) ---------------------------------
 * A profile makes the score of a cell depend on the POSITION in the read instead of on the read's letter: a PSSM of a protein
 * search, or the quality-aware penalties of a mapper (a mismatch at a Q2 base costs less than one at a Q40 base).
 * alphabet: n bytes as for swmi_set_score_matrix -- 1 <= n <= 64, pairwise distinct after canonicalisation.  scores: n entries per
 * read byte of the batch, in upload order: the entry of read q, 0-based row i < m_q and symbol c is
 * scores[(read_off[q] + i) * n + c], read_off being the array swmi_batch_upload was given.  The array is copied.  n = 0 (the
 * pointers may be NULL) clears the profiles.  A run of a batch that has profiles scores cell (i, j) of (ref, read q) as
 *      s(i,j) = scores[(read_off[q] + i - 1) * n + class(ref[j-1])]   if the reference byte's canonical code is in the alphabet
 *             = params.mismatch                                       otherwise
 * and everything else is the contract of the run's mode with this s: the recurrences, both tie chains, the order of tied maximum
 * cells, local mode's degenerate maximum 0, the walks and `begin`.  The read's bytes are not read for scoring; they are what the
 * aligned strings show (with case) and what cigar = 2 compares for = / X.  Such a run takes the affine kernels whatever gap_open /
 * affine say (swmi_batch_mode = 3); S of the affine bounds covers the largest |entry|, and the path bound takes the largest entry
 * as it does a matrix's.  Scope: align_mode local, fit and global, extend, overlap, both tie modes, any gap_open <= 0, scores_only,
 * cigar, device_strings, zero_copy, profiling, cell_cap with its exact-size re-run, max_workspace_bytes, swmi_batch_run_async.
 * Setting: duplicate symbols, n > 64, an entry with |entry| > 2^20 or a NULL pointer with n > 0 return SWMI_ERR_INVALID and leave
 * the batch as it was; a batch of swmi_batch_upload_pairs returns SWMI_ERR_UNSUPPORTED (streams make their own chunk batches and
 * take no profiles).  The call takes the context's lock as swmi_batch_set_pairs does; the batch's old results are dropped and the
 * batch is to be run again.  A run takes the profiles set when it was asked for.
 * Running: SWMI_ERR_UNSUPPORTED before anything is launched, the message naming the profile and the other value, for a context
 * score matrix set at the same time, gap_open2, subopt, hits or end_bonus; for a batch whose longest read has more than 1024
 * bases; and for a batch beyond the LDS bound: with m the longest read and M = 64 * ceil(m / 64), M * (n + 1) <= 32768 (every read
 * of up to 1024 bases with n <= 31; n = 64 with reads of up to 448 bases).  band, xdrop and band_adapt act on reads longer than
 * 1024 bases only and keep their rules.  A batch without profiles runs exactly as before. */
int  swmi_batch_set_read_profiles(swmi_ctx *ctx, swmi_batch *b, const uint8_t *alphabet, uint32_t n, const int32_t *scores);

/* Fill + direction field + max-cell lists + device traceback for every pair, then
 * the compact result records device->host.  Synchronous on return. */
int  swmi_batch_run(swmi_ctx *ctx, swmi_batch *b, const swmi_params *p);
void swmi_batch_free(swmi_ctx *ctx, swmi_batch *b);
/* The same run on the context's own host thread: swmi_batch_run_async returns at once, swmi_batch_wait blocks until
 * the run has finished and returns its status (one run in flight per context; results and accessors as after
 * swmi_batch_run, to be used after the wait).  What a Spark task uses to prepare its next partition -- or bench.py's
 * rank to do the previous shard's reduce -- while the GPU works. */
int  swmi_batch_run_async(swmi_ctx *ctx, swmi_batch *b, const swmi_params *p);
int  swmi_batch_wait(swmi_ctx *ctx);

/* Stage timings of the last swmi_batch_run with option "profiling" = 1 (ms, HIP events
 * on the context's stream): fill kernel, traceback kernel, D2H; launches = number of
 * fill launches the figures sum over. */
typedef struct swmi_timing {
    float    fill_ms, traceback_ms, d2h_ms, total_ms;
    uint32_t fill_launches, rerun_pairs;
    uint64_t cells;             /* sum of m*n over the pairs of the run (nominal: a pair that option "xdrop" stopped counts in full) */
    uint64_t dir_bytes;         /* direction-field bytes written                   */
    uint32_t strip_fallbacks;   /* launches repeated with the one-wavefront sweep after the strip pipeline gave up */
    uint32_t col_chunks;        /* column chunks the sweep of the run was split into (0: one sweep per pair): one wavefront each, one strip pipeline each for reads of several strips */
    uint32_t resident_pairs;    /* pairs handled whole by one wavefront with the direction field in LDS             */
    uint32_t tfused_pairs;      /* pairs swept in the transposed layout and traced back by the same wavefront        */
} swmi_timing;
int  swmi_batch_timing(const swmi_batch *b, swmi_timing *t);
/* The kernel pipeline (0, 1 or 2, see swmi_set_option "mode"; 3: the affine kernels, option "gap_open", "align_mode" or a score matrix) the last run
 * of the batch used. */
int  swmi_batch_mode(const swmi_batch *b, int *mode);

/* ---- results of the last run (host memory owned by the batch) ------------------- */
#define SWMI_PAIR_DEGENERATE 0x1u   /* max score 0: every one of the m*n cells is a "max cell" and
                                       yields (0,"","") -- SmithWaterman.java:154,182-185,378-380 */
#define SWMI_PAIR_TO_END     0x2u   /* option "end_bonus": the pair was taken to the read's end -- its score is end_score and its one
                                       alignment ends at (m, end_col) */
uint64_t swmi_batch_n_pairs(const swmi_batch *b);
int      swmi_pair_score(const swmi_batch *b, uint64_t pair, int32_t *score);
int      swmi_pair_n_alignments(const swmi_batch *b, uint64_t pair, uint64_t *n, uint32_t *flags);
/* The read rows the pair's sweep covered: the read's length m for every pair that was not stopped (in every mode, with xdrop = 0
 * too), 1024 (s* + 1) for a pair that option "xdrop" stopped behind strip s*: rows < m is the sign of a stop.  Works under
 * scores_only. */
int      swmi_pair_rows_swept(const swmi_batch *b, uint64_t pair, uint32_t *rows);
/* The window of reference columns *c_lo .. *c_hi (1-based, inclusive; either pointer may be NULL) that the pair's sweep used for
 * strip `strip` of the read (rows 1024 strip + 1 .. 1024 (strip + 1)), after any run: (1, n) for a read of at most 1024 bases or a run
 * without a band; max(1, 1024 strip + 1 - w) .. min(n, 1024 (strip + 1) + w) under option "band"; the window the sweep placed under
 * option "band_adapt".  Works under scores_only.  A strip >= ceil(m / 1024) (>= 1 for m <= 1024), or one that option "xdrop" did not
 * sweep (1024 strip >= swmi_pair_rows_swept), is SWMI_ERR_RANGE. */
int      swmi_pair_band_window(const swmi_batch *b, uint64_t pair, uint32_t strip, uint32_t *c_lo, uint32_t *c_hi);
/* all pairs at once: scores[n] and/or n_alignments[n] (either may be NULL), n = swmi_batch_n_pairs */
int      swmi_batch_pair_results(const swmi_batch *b, int32_t *scores, uint64_t *n_alignments, uint64_t n);
/* k-th alignment of the pair in OptAlignments order.  *ref_aln / *read_aln point to
 * NUL-terminated strings owned by the batch (valid until the next run/free);
 * characters keep the caller's original case, gaps are '_' (SmithWaterman.java:356). */
int      swmi_pair_alignment(swmi_batch *b, uint64_t pair, uint64_t k,
                             int32_t *begin, int32_t *end_i, int32_t *end_j,
                             const char **ref_aln, const char **read_aln, uint32_t *len);
/* Option "cigar": the k-th alignment of the pair as a CIGAR.  *cigar points to *n_cigar entries  len << 4 | op  in the batch's
 * result memory (valid until the next run / free), first entry = start of the alignment; *nm is the edit distance; begin / end_i /
 * end_j as swmi_pair_alignment.  Any output pointer may be NULL.  An alignment of a degenerate local pair gives begin = 0,
 * n_cigar = 0, nm = 0.  k out of range: SWMI_ERR_RANGE.  A batch whose last run had cigar = 0 or scores_only = 1:
 * SWMI_ERR_UNSUPPORTED. */
#define SWMI_CIGAR_M  0u
#define SWMI_CIGAR_I  1u
#define SWMI_CIGAR_D  2u
#define SWMI_CIGAR_EQ 7u
#define SWMI_CIGAR_X  8u
int      swmi_pair_cigar(swmi_batch *b, uint64_t pair, uint64_t k,
                         int32_t *begin, int32_t *end_i, int32_t *end_j,
                         const uint32_t **cigar, uint32_t *n_cigar, uint32_t *nm);

/* Option "subopt": the pair's second-best local score and the (1-based) reference column it ends in, as option "subopt" defines
 * them; (0, 0) when there is none.  Either pointer may be NULL.  Works under scores_only = 1 and on a stream's chunk batches; on a
 * pair list end2 is in the segment's coordinates.  A batch whose last run had subopt = 0: SWMI_ERR_UNSUPPORTED; a pair out of
 * range: SWMI_ERR_RANGE. */
#define SWMI_SUBOPT_AUTO (-1)
int      swmi_pair_subopt(const swmi_batch *b, uint64_t pair, int32_t *score2, uint32_t *end2);
/* all pairs at once: score2[n] and/or end2[n] (either may be NULL), n = swmi_batch_n_pairs */
int      swmi_batch_pair_subopt(const swmi_batch *b, int32_t *score2, uint32_t *end2, uint64_t n);

/* Option "hits": the pair's entries as option "hits" defines them, best first; cells are 1-based (end_i the read row, end_j the
 * reference column), reserved is 0.  *n_hits always receives the pair's count (n_hits may be NULL); hits may be NULL, which asks for the
 * count only; cap below the count: SWMI_ERR_RANGE.  Works under scores_only = 1 and on a stream's chunk batches; on a pair list the cells
 * are in the segments' coordinates.  A batch whose last run had hits = 0: SWMI_ERR_UNSUPPORTED; a pair out of range: SWMI_ERR_RANGE. */
typedef struct swmi_hit { int32_t score; uint32_t end_i, end_j, reserved; } swmi_hit;
int      swmi_pair_hits(const swmi_batch *b, uint64_t pair, swmi_hit *hits, uint32_t cap, uint32_t *n_hits);
/* all pairs at once: n_hits[n] and/or hits[n * cap_per_pair], pair p's entry k at hits[p * cap_per_pair + k], the entries past its count
 * zeroed (either may be NULL); n = swmi_batch_n_pairs.  cap_per_pair below the run's K with hits given: SWMI_ERR_RANGE. */
int      swmi_batch_pair_hits(const swmi_batch *b, swmi_hit *hits, uint32_t cap_per_pair, uint32_t *n_hits, uint64_t n);

/* Option "end_bonus": the pair's max_score, end_score and end_col as that option defines them -- the best score anywhere (reported
 * whether or not the pair was taken to the end: a caller needs it to undo the choice), the best score in read row m and the
 * smallest (1-based) reference column that holds it; (0, 0, 0) for a pair with an empty side.  Every pointer may be NULL.  Works
 * under scores_only = 1 and on a stream's chunk batches; on a pair list end_col is in the segment's coordinates.  A batch whose
 * last run had end_bonus = 0: SWMI_ERR_UNSUPPORTED; a pair out of range: SWMI_ERR_RANGE. */
int      swmi_pair_end_score(const swmi_batch *b, uint64_t pair, int32_t *max_score, int32_t *end_score, uint32_t *end_col);
/* all pairs at once: max_score[n], end_score[n] and/or end_col[n] (each may be NULL), n = swmi_batch_n_pairs */
int      swmi_batch_pair_end_scores(const swmi_batch *b, int32_t *max_score, int32_t *end_score, uint32_t *end_col, uint64_t n);

/* Builds the record index and both strings of EVERY alignment of the batch in one native call (what a caller that
 * consumes all of OptAlignments' output pays); returns the number of alignments (degenerate pairs count m*n) and
 * of characters built. */
int      swmi_batch_materialise_all(swmi_batch *b, uint64_t *n_alignments, uint64_t *n_chars);

/* ---- MapRef view: per reference, over all reads (Distribution.java:403-436) ------ */
/* total = sum over reads of the pair scores (Java int, wrapping) (:424). */
int      swmi_ref_total(const swmi_batch *b, uint32_t ref, int32_t *total);
/* all n_refs totals at once into totals[n_refs] (what the driver's max/top-K reduce consumes, :341-353) */
int      swmi_ref_totals(const swmi_batch *b, int32_t *totals, uint32_t n);
/* matchSites = the reads' alignment lists concatenated in read order (:425), then
 * stably sorted by ascending begin (:428, MatchSiteComp :691-694). */
int      swmi_ref_n_match_sites(swmi_batch *b, uint32_t ref, uint64_t *n);
int      swmi_ref_match_site(swmi_batch *b, uint32_t ref, uint64_t k, int32_t *begin,
                             const char **ref_aln, const char **read_aln, uint32_t *len);

/* MapRef's output for the references ref_lo .. ref_hi-1 in ONE call -- what a per-partition binding hands back
 * (Distribution.java:419-433) instead of three calls per match site.  Per reference r (index r - ref_lo): totals[] (:424),
 * degenerate[] = how many leading (0, "", "") sites it has (pairs whose maximum is 0 contribute m*n each,
 * SmithWaterman.java:154,182-185; they are counted, not listed) and site_first[] .. site_first[+1] = its real match sites in
 * MapRef order (stable sort by begin, :428) within begins[] / lens[] / str_off[]: site s has refAligned at blob + str_off[s]
 * and readAligned at blob + str_off[s] + lens[s], lens[s] bytes each, no terminators.  site_first has ref_hi - ref_lo + 1
 * entries.  *n_sites / *blob_bytes always receive the sizes needed: call with begins = NULL to ask for them, then with
 * buffers of at least that capacity (too small: SWMI_ERR_RANGE).  totals / degenerate / site_first may be NULL. */
int      swmi_ref_sites_packed(swmi_batch *b, uint32_t ref_lo, uint32_t ref_hi,
                               int32_t *totals, uint64_t *degenerate, uint64_t *site_first,
                               int32_t *begins, uint32_t *lens, uint64_t *str_off, uint64_t sites_cap,
                               uint8_t *blob, uint64_t blob_cap, uint64_t *n_sites, uint64_t *blob_bytes);

/* ---- one-shot path: what a per-partition JNI call binds -------------------------- */
/* upload + run; results are read with the accessors above; free with swmi_batch_free. */
int  swmi_align_batch(swmi_ctx *ctx, const swmi_params *p,
                      const uint8_t *ref_bytes, const uint64_t *ref_off, uint32_t n_refs,
                      const uint8_t *read_bytes, const uint64_t *read_off, uint32_t n_reads,
                      swmi_batch **out);

/* ---- streaming: a reference set larger than one batch ------------------------------ */
/* The reference reads a whole FASTA file (InOutOps.GetRefSeqs, InOutOps.java:115-168) and then maps it
 * (Distribution.java:329-338).  A stream aligns the reads given at open against references that arrive in chunks:
 * host threads parse / copy chunk k+1 into pinned memory while `slots` workers (each its own HIP stream and device
 * buffers on the context's GPU) upload the raw bytes, canonicalise them on the GPU, run the full path and keep the
 * results of chunks k, k-1, ...  After swmi_stream_finish every chunk's results are a swmi_batch to which all
 * swmi_pair_* / swmi_ref_* accessors apply (reference indices local to the chunk; swmi_stream_chunk gives the offset).
 * slots = 0 and chunk_bytes = 0 pick the defaults (3 slots, 32 MiB of sequence per chunk). */
typedef struct swmi_stream swmi_stream;
typedef struct swmi_stream_stats {
    double   push_ms;            /* wall time inside swmi_stream_push_file                                  */
    double   parse_ms;           /* summed over the parser threads                                          */
    double   upload_ms, run_ms;  /* summed over the slot workers: H2D + encode, sweep + traceback + results */
    double   gpu_sweep_ms, gpu_traceback_ms;   /* HIP-event times, option "profiling" = 1                   */
    uint64_t bytes, cells;
    uint32_t chunks, pad;
} swmi_stream_stats;
int      swmi_stream_open(swmi_ctx *ctx, const swmi_params *p, const uint8_t *read_bytes, const uint64_t *read_off,
                          uint32_t n_reads, uint32_t slots, uint64_t chunk_bytes, swmi_stream **out);
/* references from memory (copied before the call returns; kept for the alignment strings) */
int      swmi_stream_push(swmi_stream *s, const uint8_t *ref_bytes, const uint64_t *ref_off, uint32_t n_refs);
/* references from a FASTA file with GetRefSeqs' line rules (swmi_io.h), parsed segment-wise by parse_threads host
 * threads (0: 6); the file stays mapped until the stream is closed and a reference's bytes are re-read from it when
 * one of its alignment strings is asked for.  One file per stream. */
int      swmi_stream_push_file(swmi_stream *s, const char *path, const char *delimiter, uint32_t parse_threads);
/* the same for one rank's share of the file: the records of shard `shard` of `n_shards` by the byte-range rule of
 * swmi_io_read_refs_shard (swmi_io.h) -- what a driver that partitions ONE reference file over its ranks pushes, as
 * DistributeReference partitions its reference list over the executors (Distribution.java:329-338).  A shard may hold no
 * record (the stream then has none); the whole-file checks apply on every shard.  (0, 1) is swmi_stream_push_file. */
int      swmi_stream_push_file_shard(swmi_stream *s, const char *path, const char *delimiter, uint32_t parse_threads,
                                     uint32_t shard, uint32_t n_shards);
int      swmi_stream_finish(swmi_stream *s);                  /* blocks until every chunk is done */
uint64_t swmi_stream_n_refs(const swmi_stream *s);
uint32_t swmi_stream_n_chunks(const swmi_stream *s);
int      swmi_stream_chunk(swmi_stream *s, uint32_t k, swmi_batch **batch, uint64_t *first_ref);
int      swmi_stream_totals(const swmi_stream *s, int32_t *totals, uint64_t n);   /* MapRef totals of all references */
int      swmi_stream_metadata(const swmi_stream *s, uint64_t ref, char *buf, size_t cap);
/* file sources: the byte offset in its file of reference `ref`'s metadata line.  With the file's place in the DirectoryCrawler
 * walk this is the order in which the control driver meets the reference (Distribution.java:586-613), which OptSeqsComp's stable
 * sort keeps among equal metadata (:621, :647-666).  SWMI_ERR_INVALID for references pushed from memory. */
int      swmi_stream_ref_pos(const swmi_stream *s, uint64_t ref, uint64_t *pos);
/* the sequence bytes of reference `ref` (GetRefSeqs' concatenated lines, InOutOps.java:127-150) into buf, for a driver that aligns
 * its winning references again after the stream dropped their records (option stream_keep_records = 0): file sources re-read
 * the one record from the mapped file, memory sources copy the bytes kept at push.  *len always receives the size; buf = NULL
 * asks for it only; cap < size is SWMI_ERR_RANGE. */
int      swmi_stream_ref_sequence(const swmi_stream *s, uint64_t ref, uint8_t *buf, uint64_t cap, uint64_t *len);
int      swmi_stream_get_stats(const swmi_stream *s, swmi_stream_stats *st);
void     swmi_stream_close(swmi_stream *s);

#ifdef __cplusplus
}
#endif
#endif /* SWMI_H */
