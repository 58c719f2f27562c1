// swmi_affine.hip -- gfx950 kernels of the affine-gap (Gotoh) path: a gap of length k costs gap_open + k * gap.
//
// Recurrence (DESIGN.md "Affine gaps"; i = read row, j = reference column; o = gap_open <= 0, e = gap <= 0):
//   E(i,j) = max(H(i,j-1) + o + e, E(i,j-1) + e)     deletion state,  xE = 1 iff the extension is strictly better
//   F(i,j) = max(H(i-1,j) + o + e, F(i-1,j) + e)     insertion state, xF likewise
//   H(i,j) = max(0, E, F, H(i-1,j-1) + s(i,j)) with the linear path's tie chains (serial '>=' a > i > d, strict '>' d > i > a)
// E and F are clamped at 0: only positive values ever reach H, the direction or a walked x bit, so no -inf sentinel is needed.
//
// sw_affine_sweep_kernel: ONE WAVEFRONT PER PAIR, the anti-diagonal systolic mapping of the linear sweep.
//   Lane l owns R = ceil(m / 64) consecutive read rows (R = 1..16, m <= 1024) and at step t works on column j = t - l + 1.
//   H and E of its rows stay in registers; H and F of its last row, and the reference base, pass to lane l+1 by DPP
//   (wave_shr:1).  Every cell leaves a 4-bit code in the pair's direction field:
//     bits 0-1  what H(i,j) came from: 0 = H is 0 (the walk stops), 1 = diagonal, 2 = F (insertion), 3 = E (deletion)
//     bit 2     xE(i,j)        bit 3  xF(i,j)
//   8 anti-diagonal steps per dword, laid out [block w][row slot k][lane]: dword (w * R + k) * 64 + lane holds steps
//   t = 8w .. 8w+7 of row i = l * R + k + 1, step t at bits 4 * (t % 8).  Every store writes 256 contiguous bytes.
//   The pair's maximum and its tied cells are tracked as in the linear sweep: a wave-uniform threshold, a cell list capped
//   at cell_cap (more: SWMI_F_CELL_OVF, the host re-runs the pair with an exact-size list).
//
// sw_affine_sweep_matrix_kernel / _wide_kernel: the same sweep with s(i,j) from a substitution score matrix
//   (swmi_set_score_matrix, DESIGN.md "Score matrices").  The workgroup stages two tables in LDS (layout: swmi_aff_mat_words):
//     key[code]   = class(code) * 4 | hi << 16, hi = code when the code is outside the alphabet (class n), else 0x1FF
//     tab[cq * (n+1) + cr]  the matrix, row = read class, column = reference class; row and column n (outside the
//                           alphabet) hold mismatch
//   A lane keeps key-derived words for its rows (q = class * (n+1) * 4 | hi << 16, hi = 0x3FF inside the alphabet) and passes the reference base's key along
//   the wave instead of its code: the cell reads tab at byte offset q.lo + key.lo, and scores match instead when both high
//   halves are equal (the same code outside the alphabet -- today's equality rule).
//
// sw_affine_sweep_{fit,global}[_matrix][_wide]_kernel: the end-to-end modes (option "align_mode", DESIGN.md "End-to-end
//   modes"): the same sweep with MODE = 1 (fit: the whole read against any stretch of the reference) or 2 (global).  No floor
//   at 0 on E, F and H, so the direction is always 1..3; H of a lane's rows starts at the column-0 value o + i*e and E at
//   H(i,0) + o (which gives E(i,1) = H(i,0) + o + e with xE = 0: no -inf needed); lane 0's feed from above is row 0 of the
//   mode (H = 0 in fit mode, o + j*e in global mode; F(0,j) := H(0,j) + o, the same trick).  The maximum is taken over row m
//   only -- one lane, one row slot -- from INT32_MIN up: every column j of row m that ties (fit) or the one cell (m,n) (global).
//   The x bits come from compares: the operands may be negative and their difference need not fit int32.
//
// sw_affine_sweep_long[_fit|_global][_matrix]_kernel: reads longer than 1024 bases (option "long_reads", DESIGN.md "Long
//   reads").  Still one wavefront per pair: the read is swept in ceil(m / 1024) strips of 1024 rows, every strip with R = 16
//   (the last one padded with SWMI_CODE_PAD rows), each strip leaving the field of a (1024, n) pair; the strips' fields are
//   consecutive.  What lane 0 reads from above in strips 1.. is the SEAM: (H, F) of the strip's last row, written by lane 63
//   of the strip above into one row of n pairs per pair in HBM, rewritten in place strip after strip.  The threshold and the
//   cell list live on across the strips; cells carry global row indices.  These kernels return for m <= 1024, the others for
//   m > 1024: the host launches each over the pairs it takes.
//
// sw_affine_traceback_kernel: one wavefront per (pair, slot); slot s walks the pair's maximum cells s, s + S, ...  The walk
//   is the three-state machine of DESIGN.md "Affine gaps"; the field is staged in LDS a tile of consecutive 8-step blocks at a
//   time (a path never moves to a later step), the ops are packed 16 per dword in LDS, and the record goes out through
//   swmi_emit.h with rank SWMI_RANK_BY_CELL (the host orders a pair's records by cell).
// sw_affine_traceback_{fit,global}_kernel: the walk of the end-to-end modes.  It ends at row 0, not at a code 0; at column 0
//   the rest of the read is inserted without touching the field; global mode then deletes the rest of the reference;
//   `begin` follows the moves that consume a reference base.
// sw_affine_traceback_long[_fit|_global]_kernel: the same walks over the strips' fields: row i is in strip (i - 1) / 1024; a
//   step up from a strip's first row goes to lane 63, row slot 15 of the strip above; the LDS tile is keyed by the strip too.
//
// sw_affine_sweep_band[_fit|_global][_matrix]_kernel, sw_affine_traceback_band[_fit|_global]_kernel: the strip kernels under
//   option "band" (half-width w, DESIGN.md "Banded alignment"): strip s sweeps the window of columns swmi_aff_band_lo(s, w) ..
//   swmi_aff_band_hi(s, n, w) only and leaves that window's field; a cell outside the band reads as 0 (local) or
//   SWMI_AFF_BAND_NEG; the walk takes a strip's window origin and block count from (s, n, w).  The half-width is one more
//   scalar kernel argument.
//
// sw_affine_sweep_extend[_matrix][_wide]_kernel, sw_affine_sweep_{long,band}_extend[_matrix]_kernel: seed extension (option
//   "extend" on a global run), MODE = 3: global mode's cells, boundaries and field, bit for bit, with the maximum
//   taken over every cell of rows 1 .. m as in local mode, from INT32_MIN up (the score may be <= 0; there is no degenerate
//   case).  The walk from a maximum cell is global mode's: these runs are traced back by the three global traceback kernels.
//
// sw_affine_sweep_{long,band}_xdrop[_matrix]_kernel: the strip sweeps of an extend run under option "xdrop" (DESIGN.md 8h), XDROP =
//   1: between two strips the wave takes the maximum of H over the seam row and ends the pair when the running maximum lies more
//   than the threshold above it; the PairOut carries the strips swept.  The threshold is one more scalar kernel argument.
//
// sw_affine_sweep_band_adapt[_xdrop][_matrix]_kernel, sw_affine_traceback_band_adapt_global_kernel: the banded strip kernels of an
//   extend run under option "band_adapt" (DESIGN.md 8i), ADAPT = 1: the window of a strip is placed around the column of the seam
//   row's maximum instead of around j = i; the sweep leaves the centres in a table behind the pair's fields, the walk reads them.
//
// sw_affine_sweep2_{global,extend}[_wide]_kernel, sw_affine_sweep2_{long,band}_{global,extend}_kernel,
// sw_affine_traceback2[_long|_band]_global_kernel: global and extend runs under option "gap_open2" (DESIGN.md 8j), TWO = 1: a gap of
//   length k costs max(gap_open + k * gap, gap_open2 + k * gap2).  Two more gap states per cell, a second 4-bit plane in the field
//   (blocks interleave the planes), 16-byte seam entries (H, F1, F2), a walk through five states.
//
// sw_affine_sweep_[long_|band_]subopt[_matrix][_wide]_kernel: the local sweeps under option "subopt" (DESIGN.md 8n), SUBOPT = 1: a running
//   column maximum rides down the wave with its column, and the lane that finishes a column leaves colmax(j) in a row of n int32
//   behind the pair's fields; sw_subopt_kernel (swmi_subopt.hip) turns the row into the pair's second-best score and its end column.
//
// sw_affine_sweep_[long_|band_]hits[_matrix][_wide]_kernel: the local sweeps under options "subopt" and "hits" (DESIGN.md 8p), SUBOPT = 1 and
//   HITS = 1: the smallest row that holds the column maximum rides with it and is left in a second row behind the first;
//   sw_hits_kernel (swmi_subopt.hip) picks the pair's K best separated end cells from the two rows.
//
// sw_affine_sweep_[long_|band_]endb[_matrix][_wide]_kernel: the extend sweeps under option "end_bonus" (DESIGN.md 8o), ENDB = 1: the lane
//   that owns read row m keeps the maximum of H(m, j) and its smallest column, and the wave chooses between the best cell anywhere
//   and the best extension that reaches the read's end where it writes the pair's PairOut.
//
// sw_affine_sweep_[long_]overlap[_matrix][_wide]_kernel, sw_affine_traceback_[long_]overlap_kernel: overlap (ends-free) alignment (option
//   "overlap" on a fit run), MODE = 4: fit mode's cells with column 0 at 0 as well as row 0, the maximum taken over read row
//   m and the last column from INT32_MIN + 1 up (the score may be <= 0; there is no degenerate case), and a walk that ends at the first
//   cell of row 0 or column 0 without a tail.
//
// sw_affine_sweep_[fit_|global_|extend_|overlap_]profile[_wide]_kernel: the short sweeps of a batch with per-read score profiles
//   (swmi_batch_set_read_profiles), PROFILE = 1: s(i,j) is entry [row i][class of the reference base] of the READ's own
//   table -- one row per read position, not per read letter.  The workgroup stages the 256 keys (class * 4), every wavefront its
//   read's table in dynamic LDS (prows rows of n + 1 dwords, column n = mismatch for a reference base outside the alphabet); a lane's
//   row words are the byte offsets of its rows' table rows, and the cell is one LDS read at row word + key, with no select.  The
//   read's bytes are not read.  A list of their own, AFF_PROFILE_SWEEPS (10), and a launcher of their own; the walks are unchanged.
//
// How the 93 kernels of the first four lists are made: two lists, AFF_SWEEPS (72 rows) and AFF_TRACEBACKS (13), name every kernel with its
//   MODE and its flags; the kernel definitions, their parameter lists and the launchers' tables are the lists under a macro each,
//   and the file defines no kernel outside them and the second pair of lists, AFF_OVERLAP_SWEEPS (6) and AFF_OVERLAP_TRACEBACKS (2),
//   which goes through the same macros (the first pair's row counts are pinned by the tests of the modes they hold).
//   A sweep is aff_sweep_entry<RLO, RHI, MODE, F> over one block function
//   (aff_block8), a traceback aff_traceback<MODE, F>, F being the row's flags as one word (AFF_F_ of swmi_launch.h; !LONG is the
//   walk with one strip and !BAND the walk whose windows are the whole reference).  Which combinations may exist is aff_flags_ok
//   there, asserted for every row; the launchers take the run's options as one AffRun and search their table for the run's key.
//   The per-pair sweep is two thin bodies, aff_sweep_pair and aff_sweep_long_pair (the one strip
//   loop, banded or not), over shared pieces: vrows and the cell list as functions of values, the row load, the block store
//   and the epilogue as text (DESIGN.md 8e and 8f say why).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "swmi_device.h"
#include "swmi_emit.h"
#include "swmi_launch.h"
#include "swmi_wave.h"

#define AFF_WAVES 4                    // wavefronts (= pairs) per workgroup of the sweep

// direction codes of the field (bits 0-1)
#define AFF_STOP 0u
#define AFF_DIAG 1u
#define AFF_INS  2u
#define AFF_DEL  3u
// MODE of the sweeps and the traceback (= option "align_mode")
#define AFF_LOCAL  0
#define AFF_FIT    1
#define AFF_GLOBAL 2
// option "extend" (with align_mode global): global mode's cells, local mode's maximum over every cell.  Internal to this file
// and the launchers' tables: the host passes it in place of the align_mode
#define AFF_EXTEND 3
// option "overlap" (with align_mode fit): fit mode's cells without a fixed end -- row 0 AND column 0 are 0, the maximum
// is taken over read row m and the last column, the walk ends at row 0 or column 0.  Internal like AFF_EXTEND
#define AFF_OVERLAP 4
// the modes that sweep global mode's cells (row 0 is o + j*e), and the ones whose maximum is taken over row m alone
#define AFF_ROW0_GAPS(MODE) ((MODE) == AFF_GLOBAL || (MODE) == AFF_EXTEND)
#define AFF_ROW_M_ONLY(MODE) ((MODE) == AFF_FIT || (MODE) == AFF_GLOBAL)
// the modes whose column 0 is o + i*e (local and overlap: 0)
#define AFF_COL0_GAPS(MODE) ((MODE) == AFF_FIT || (MODE) == AFF_GLOBAL || (MODE) == AFF_EXTEND)
// The device templates take MODE and one flags word F (the AFF_F_ bits of swmi_launch.h); each opens with the bits under the
// names its body uses
#define AFF_FLAG_NAMES(F)                                                                                                           \
    [[maybe_unused]] constexpr bool MATRIX = ((F) & AFF_F_MATRIX) != 0, LONG = ((F) & AFF_F_LONG) != 0, BAND = ((F) & AFF_F_BAND) != 0, \
                                    XDROP = ((F) & AFF_F_XDROP) != 0, ADAPT = ((F) & AFF_F_ADAPT) != 0, TWO = ((F) & AFF_F_TWO) != 0, \
                                    SUBOPT = ((F) & AFF_F_SUBOPT) != 0, ENDB = ((F) & AFF_F_ENDB) != 0, HITS = ((F) & AFF_F_HITS) != 0, \
                                    PROFILE = ((F) & AFF_F_PROFILE) != 0;

namespace {

// the score matrix of the matrix sweeps (only their instantiations reference it: the other kernels allocate no LDS)
__shared__ uint32_t aff_mkey[256];
__shared__ int aff_mtab[SWMI_MAT_NN_MAX * SWMI_MAT_NN_MAX];
// the reads' tables of the profile sweeps (PROFILE): dynamic LDS behind aff_mkey, which those sweeps stage too -- one
// table per wavefront, prows rows of pnn dwords each (what the launcher sized the workgroup by); a lane's row words are byte offsets
// from here
extern __shared__ int aff_ptab[];

// the strip sweeps (LONG): lane 0's feed from above and lane 63's hand-over to the next strip
struct AffSeam {
    int h, f;              // lanes 0..7: (H, F) of the row above the strip at the 8 columns lane 0 takes in this block
    int2 *row;             // the pair's seam row: (H, F) per column
    int f2;                // TWO: F2 of that row (f is F1)
    uint32_t cmrs;         // HITS: dwords from an entry of cmrow to the same column's entry of the row of rows (swmi_aff_colmax_stride).  It and
                           //   cmr stand in the struct's two padding words: a struct of more than 64 bytes renames the narrow subopt sweeps' registers
    int4 *row4;            // TWO: the pair's seam row, (H, F1, F2, -) per column: 16-byte entries, one load and one store each
    uint32_t wlane;        // the lane that writes it (63), none in the read's last strip
    uint32_t coff;         // BAND: the columns left of the strip's window (`row` starts at the window, cells are listed with global columns)
    // SUBOPT (option "subopt"; the short sweeps use these three too)
    int cm;                // lanes 0..7: the column maxima the strips above left at the 8 columns lane 0 takes in this block (strip 0, short reads: not read)
    int cmr;               // HITS (option "hits"): lanes 0..7: the rows that hold those maxima (strip 0, short reads: not read)
    int *cmrow;            // the pair's row of column maxima, from the window's first column on
    uint32_t cmlane;       // the lane that holds a column's finished maximum and stores it: 63 in a strip, the owner of the read's last row in a short sweep
    // ENDB (option "end_bonus"; the short sweeps use it too)
    uint32_t elane;        // the lane that owns read row m: (m - 1) / R in a short sweep, the last strip's (m - 1 - 1024 sx) / 16; no lane (0xFFFFFFFF) in the strips above
};

template <int R>
struct AffState {
    int h[R], e[R];        // H and E of the lane's rows at its previous column
    int q[R];              // the rows' base codes (SWMI_CODE_PAD past the read); MATRIX: their score-table row words
    uint32_t acc[R];       // codes of the current 8-step block
    int rb;                // reference base code of the lane's current column; MATRIX: its key word
    int nh_prev;           // lane l-1's last-row H one step ago: the diagonal of row 0
    int f_last;            // F of the lane's last row at its previous column (what lane l+1 reads as F(i-1, j))
    int thr;               // wave-uniform running maximum (starts at 1: a maximum of 0 is the degenerate case)
    uint32_t cnt;          // wave-uniform number of cells equal to thr
    // TWO (two-piece gaps): e and f_last are piece 1's E and F; piece 2's, and the codes of plane 1
    int e2[R];
    uint32_t acc2[R];
    int f2_last;
    int cm;                // SUBOPT: the running maximum of H over the lane's current column, rows 1 .. the lane's last (it travels with the column)
    int eg;                // ENDB: in the lane that owns read row m, the maximum of H(m, j) over the columns it has swept (INT32_MIN before the first)
    uint32_t egc;          // ... and the smallest (global, 1-based) column that holds it
    int cmr;               // HITS: the smallest (global, 1-based) row that holds S.cm, 0 while that is the seed's 0
};

// 8 anti-diagonal steps t0 .. t0+7 (a lane outside its column range keeps its state).  The steps are a loop, not unrolled:
// eight copies of R cells let the scheduler hoist the compares of many cells at once, and their masks spilled the SGPRs.
// AFF_FIT, AFF_GLOBAL: vrows is the row slot of read row m in the lane that owns it, 0xFFFFFFFF in every other lane
// AFF_EXTEND: global mode's cell, then local mode's tied maxima from INT32_MIN up -- vrows is local mode's, so pad rows never
//   compete.  A lane without a cell in this step idles at mrow = INT32_MIN: it passes `mrow >= thr` only while thr is still
//   INT32_MIN, which is before step 0 alone (lane 0's cell (1, 1) -- of the first window under BAND -- raises it there), and it
//   lists nothing even then: a listed cell is inr, inside the read and holds a real H
// AFF_OVERLAP: fit mode's cell and row 0; a cell COMPETES iff it lies on read row m or in the last column.  vrows is
//   local mode's.  Inside the row loop a lane takes, under the one test k < vrows, the maximum of its rows inside the read and H of the
//   last of them (ENDB's hend: no array indexed by a run-time value, no further mask per row); behind the loop mrow is that maximum in
//   the last column, H(m, j) in lane Z.elane, which owns read row m, and INT32_MIN everywhere else.  (Taking the last column's maximum
//   from S.h behind the loop instead, once per lane, was tried: the wide sweep then spills 900 SGPRs and the strip sweep needs 234
//   VGPRs.)  The threshold starts at INT32_MIN + 1, ONE ABOVE what an idle lane holds: a lane without a competing cell never reaches
//   it, however late the first competing cell comes (row m, or column n of strip 0), and that cell -- a real H -- is strictly
//   greater.  The list loop repeats the membership test: a row of the lane that happens to hold the maximum's value but does not
//   compete is not listed
// LONG: one strip of a long read -- lane 0 is fed from Z (every strip, the first one too: its Z holds row 0 of the mode) and lane
// Z.wlane leaves (H, F) of its last row in the seam row
// BAND (with LONG): the strip sweeps a window of the reference -- n is the window's length, columns count from its first one
// TWO (option "gap_open2", global and extend runs): a gap of length k costs max(o + k*e, o2 + k*e2).  Each gap state
//   exists once per piece -- (S.e, S.f_last) piece 1, (S.e2, S.f2_last) piece 2 -- E = max(E1, E2), F = max(F1, F2), piece 1 on a
//   tie, and H is taken from E, F and the diagonal as before.  The cell leaves a second 4-bit code in S.acc2 (plane 1 of the
//   field): bit 0 pE (E is E2), bit 1 pF, bit 2 xE2, bit 3 xF2; plane 0 is the one-piece code with xE1, xF1 in bits 2 and 3.
//   Lane l+1 receives F2 of the last row by one more wave_shr1.  Row 0 is max(o + j*e, o2 + j*e2), F1(0,j) := H + o, F2 := H + o2.
// SUBOPT (option "subopt", local runs): lane l is at column t - l at step t, so a column travels down the wave one lane per
//   step and its running maximum rides along: S.cm = max(what lane l-1 held one step ago, mrow), mrow being the maximum of the
//   lane's rows inside the read at this column (-1 when it has none, or no column).  The move runs every step in every lane.  Lane 0
//   starts a column at 0 (H >= 0) or, in strips 1.., at what the strips above left (Z.cm, loaded as Z.h is).  Lane Z.cmlane holds the
//   finished maximum and stores it into the pair's row, a plain vector store.
// HITS (option "hits", with SUBOPT): the row that holds the column maximum rides with it in S.cmr.  Inside the row loop a
//   strictly greater hv takes the row row0 + k + 1 along with mrow; at the move a lane keeps the shifted pair unless its own mrow is
//   strictly greater.  Rows ascend with slot, lane and strip, so strict compares everywhere leave the SMALLEST row.  The storing lane
//   writes the row Z.cmrs dwords behind the value.  A column whose maximum is 0 keeps the seed's row 0 (it is never reported).
// ENDB (option "end_bonus", extend runs): read row m is slot vrows - 1 of lane Z.elane (vrows is local mode's, so a pad row
//   never owns it).  At every step with a cell that lane takes H of that slot and the column when it is strictly greater than S.eg:
//   its columns ascend, so S.egc ends as the smallest column that holds the maximum.  The slot is picked inside the unrolled row loop,
//   as the k == vrows test of fit mode is -- by the test k < vrows that mrow already makes, the last slot that passes it, so that no
//   further compare mask per row is kept in SGPRs: S.h is never indexed by a run-time value.
template <int R, bool STRICT, int MODE, uint32_t F>
__device__ __forceinline__ void aff_block8(AffState<R> &S, const uint2 rw, const uint32_t t0, const uint32_t lane,
                                           const uint32_t n, const uint32_t row0, const uint32_t vrows,
                                           const int o, const int e, const int vmat, const int vmis,
                                           uint2 *__restrict__ cells, const uint32_t ccap, const AffSeam &Z, const int o2, const int e2) {
    AFF_FLAG_NAMES(F)
    const int oe = o + e;
    const int oe2 = o2 + e2;                                     // (TWO)
#pragma unroll 1
    for (uint32_t s = 0; s < 8; ++s) {
        const uint32_t wsel = s < 4 ? rw.x : rw.y;
        const uint32_t fb = (wsel >> (8u * (s & 3u))) & 0xFFu;
        const int feed = MATRIX || PROFILE ? (int)aff_mkey[fb] : (int)fb;  // (wave-uniform: lane 0's column)
        S.rb = wave_shr1(feed, S.rb);
        int nh, nf;
        int nf2 = 0;                                             // (TWO)
        if constexpr (LONG) {
            nh = wave_shr1(__builtin_amdgcn_readlane(Z.h, (int)s), S.h[R - 1]);
            nf = wave_shr1(__builtin_amdgcn_readlane(Z.f, (int)s), S.f_last);
            if constexpr (TWO) nf2 = wave_shr1(__builtin_amdgcn_readlane(Z.f2, (int)s), S.f2_last);
        } else if constexpr (MODE == AFF_LOCAL) {
            nh = wave_shr1_zero(S.h[R - 1]);
            nf = wave_shr1_zero(S.f_last);
        }
        const uint32_t c0 = t0 + s - lane;                       // column index j - 1 of this lane
        if constexpr (MODE != AFF_LOCAL && !LONG) {
            // lane 0 reads row 0 of the mode: H(0,j) = 0 (fit) or o + j*e (global), F(0,j) := H(0,j) + o
            // (unsigned arithmetic: lane 0 runs up to 70 columns past n, where the value is not used)
            int h0 = AFF_ROW0_GAPS(MODE) ? (int)((uint32_t)o + (c0 + 1u) * (uint32_t)e) : 0;
            if constexpr (TWO) h0 = max(h0, (int)((uint32_t)o2 + (c0 + 1u) * (uint32_t)e2));
            nh = wave_shr1(h0, S.h[R - 1]);
            nf = wave_shr1((int)((uint32_t)h0 + (uint32_t)o), S.f_last);
            if constexpr (TWO) nf2 = wave_shr1((int)((uint32_t)h0 + (uint32_t)o2), S.f2_last);
        }
        const bool inr = c0 < n;
        int mrow = MODE == AFF_LOCAL ? -1 : (MODE == AFF_EXTEND || MODE == AFF_OVERLAP ? INT32_MIN : 0);
        int mrr = 0;                                             // (HITS) the smallest row of the lane that holds mrow
        if (inr) {
            int diag = S.nh_prev, up = nh, fup = nf;
            int fup2 = nf2;                                      // (TWO)
            int hend = INT32_MIN;                                // (ENDB, AFF_OVERLAP) H of the lane's last row inside the read
            uint32_t sh = 4u * s;
            const uint32_t rkey = (uint32_t)S.rb, rlo = rkey & 0xFFFFu;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int left = S.h[k];
                int sv;
                if (MATRIX) {
                    const uint32_t qk = (uint32_t)S.q[k];
                    const int tv = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(aff_mtab) + ((qk & 0xFFFFu) + rlo));
                    sv = (qk ^ rkey) < 0x10000u ? vmat : tv;
                } else if (PROFILE) {
                    // the row's table row at the column of the reference base's class: one LDS read, no select
                    sv = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(aff_ptab) + ((uint32_t)S.q[k] + rkey));
                } else {
                    sv = S.rb == S.q[k] ? vmat : vmis;
                }
                const int dg = diag + sv;
                const int t1 = left + oe, t2 = S.e[k] + e;
                const int u1 = up + oe, u2 = fup + e;
                int en, fn, hv;
                uint32_t code;
                if constexpr (MODE == AFF_LOCAL) {
                    en = max(max(t1, t2), 0);
                    fn = max(max(u1, u2), 0);
                    hv = max(max(en, fn), dg);                   // en, fn >= 0: hv >= 0
                    uint32_t d;
                    if (STRICT) d = hv == 0 ? AFF_STOP : (en == hv ? AFF_DEL : (fn == hv ? AFF_INS : AFF_DIAG));
                    else        d = hv == 0 ? AFF_STOP : (dg == hv ? AFF_DIAG : (fn == hv ? AFF_INS : AFF_DEL));
                    // x bits from the sign of the difference (no compare mask): |values| < 2^30 + 2^21, the difference fits
                    code = d | (((uint32_t)(t1 - t2) >> 31) << 2) | (((uint32_t)(u1 - u2) >> 31) << 3);
                } else if constexpr (TWO) {
                    // en, fn: piece 1's states (what S.e and fup carry on); ev, fv: E and F
                    const int t3 = left + oe2, t4 = S.e2[k] + e2;
                    const int u3 = up + oe2, u4 = fup2 + e2;
                    en = max(t1, t2);
                    fn = max(u1, u2);
                    const int en2 = max(t3, t4), fn2 = max(u3, u4);
                    const int ev = max(en, en2), fv = max(fn, fn2);
                    hv = max(max(ev, fv), dg);
                    uint32_t d;
                    if (STRICT) d = ev == hv ? AFF_DEL : (fv == hv ? AFF_INS : AFF_DIAG);
                    else        d = dg == hv ? AFF_DIAG : (fv == hv ? AFF_INS : AFF_DEL);
                    code = d | (t2 > t1 ? 4u : 0u) | (u2 > u1 ? 8u : 0u);
                    S.acc2[k] |= ((en2 > en ? 1u : 0u) | (fn2 > fn ? 2u : 0u) | (t4 > t3 ? 4u : 0u) | (u4 > u3 ? 8u : 0u)) << sh;
                    S.e2[k] = en2;
                    fup2 = fn2;
                } else {
                    en = max(t1, t2);
                    fn = max(u1, u2);
                    hv = max(max(en, fn), dg);
                    uint32_t d;
                    if (STRICT) d = en == hv ? AFF_DEL : (fn == hv ? AFF_INS : AFF_DIAG);
                    else        d = dg == hv ? AFF_DIAG : (fn == hv ? AFF_INS : AFF_DEL);
                    // x bits from compares: the operands are of either sign here and their difference need not fit int32
                    code = d | (t2 > t1 ? 4u : 0u) | (u2 > u1 ? 8u : 0u);
                }
                S.acc[k] |= code << sh;
                diag = left;
                up = hv;
                fup = fn;
                S.h[k] = hv;
                S.e[k] = en;
                if constexpr (HITS) { if ((uint32_t)k < vrows && hv > mrow) mrr = (int)(row0 + (uint32_t)k + 1u); }
                if constexpr (MODE == AFF_OVERLAP)        { if ((uint32_t)k < vrows) { mrow = max(mrow, hv); hend = hv; } }
                else if constexpr (!AFF_ROW_M_ONLY(MODE)) { if ((uint32_t)k < vrows) mrow = max(mrow, hv); }
                else                                      { if ((uint32_t)k == vrows) mrow = hv; }
                if constexpr (ENDB) { if ((uint32_t)k < vrows) hend = hv; }      // (the test of mrow: the last slot that passes it is vrows - 1)
            }
            if constexpr (ENDB) {
                if (lane == Z.elane && hend > S.eg) { S.eg = hend; S.egc = c0 + 1u + (BAND ? Z.coff : 0u); }
            }
            if constexpr (MODE == AFF_OVERLAP) {
                // left of the last column only read row m competes: one cell, in the lane that owns the row
                if (c0 + 1u != n) mrow = lane == Z.elane ? hend : INT32_MIN;
            }
            S.f_last = fup;
            if constexpr (TWO) S.f2_last = fup2;
            if constexpr (LONG && TWO) { if (lane == Z.wlane) Z.row4[c0] = make_int4(S.h[R - 1], fup, fup2, 0); }
            else if constexpr (LONG) { if (lane == Z.wlane) Z.row[c0] = make_int2(S.h[R - 1], fup); }
        }
        S.nh_prev = nh;
        if constexpr (SUBOPT) {
            // (mrow is -1 in a lane without a column)
            if constexpr (HITS) {
                const int pc = wave_shr1(LONG ? __builtin_amdgcn_readlane(Z.cm, (int)s) : 0, S.cm);
                const int pr = wave_shr1(LONG ? __builtin_amdgcn_readlane(Z.cmr, (int)s) : 0, S.cmr);
                S.cmr = mrow > pc ? mrr : pr;
                S.cm = max(pc, mrow);
                if (inr && lane == Z.cmlane) { Z.cmrow[c0] = S.cm; Z.cmrow[c0 + Z.cmrs] = S.cmr; }
            } else {
            S.cm = max(wave_shr1(LONG ? __builtin_amdgcn_readlane(Z.cm, (int)s) : 0, S.cm), mrow);
            if (inr && lane == Z.cmlane) Z.cmrow[c0] = S.cm;
            }
        }
        if constexpr (AFF_ROW_M_ONLY(MODE)) {
            // row m only: the one lane that owns it, at every column (fit) or at column n (global)
            const bool cand = inr && vrows != 0xFFFFFFFFu && (MODE == AFF_FIT || c0 + 1u == n);
            const uint64_t cm = BALLOT(cand && mrow >= S.thr);
            if (cm != 0ull) {
                const int v = __builtin_amdgcn_readlane(mrow, (int)__builtin_ctzll(cm));
                if (v > S.thr) { S.thr = v; S.cnt = 0u; }
                if (cand && S.cnt < ccap) cells[S.cnt] = make_uint2(row0 + vrows + 1u, c0 + 1u + (BAND ? Z.coff : 0u));
                S.cnt += 1u;
            }
            continue;
        }
        // tied maxima (SmithWaterman.java:176-185): the wave leaves the step only when some lane reached the threshold
        if (BALLOT(mrow >= S.thr) != 0ull) {
            uint64_t gt = BALLOT(mrow > S.thr);
            if (gt) {
                while (gt) {
                    S.thr = __builtin_amdgcn_readlane(mrow, (int)__builtin_ctzll(gt));
                    gt = BALLOT(mrow > S.thr);
                }
                S.cnt = 0;
            }
            // (AFF_OVERLAP) the lane's competing slots are clo .. vrows - 1: every row inside the read in the last column, row m alone in
            // the lane that owns it, none elsewhere -- one unsigned compare per row, where the other modes have k < vrows
            [[maybe_unused]] const uint32_t clo = MODE != AFF_OVERLAP || c0 + 1u == n ? 0u : (lane == Z.elane ? vrows - 1u : vrows);
            [[maybe_unused]] const uint32_t cspan = vrows - clo;
#pragma unroll
            for (int k = 0; k < R; ++k) {
                bool hit;
                if constexpr (MODE == AFF_OVERLAP) hit = inr && (uint32_t)k - clo < cspan && S.h[k] == S.thr;
                else                               hit = inr && (uint32_t)k < vrows && S.h[k] == S.thr;
                const uint64_t hm = BALLOT(hit);
                if (hm) {
                    const uint32_t pos = S.cnt + lanemask_lt_count(hm);
                    if (hit && pos < ccap) cells[pos] = make_uint2(row0 + (uint32_t)k + 1u, c0 + 1u + (BAND ? Z.coff : 0u));
                    S.cnt += (uint32_t)__popcll(hm);
                }
            }
        }
    }
}

// The pieces the sweep of a short read and the strip sweep of a long one share.  They take and return values: a helper that
// is handed a reference to the lane's state changes the register allocation of the sweeps it is inlined into.
// vrows of a lane whose first row is row0 + 1: LOCAL and EXTEND the number of its rows inside the read; fit and global track row m
// alone: its row slot in the lane that owns it, no slot (0xFFFFFFFF) elsewhere
template <int R, int MODE>
__device__ __forceinline__ uint32_t aff_vrows(const uint32_t m, const uint32_t row0) {
    return AFF_ROW_M_ONLY(MODE) ? (m - 1u - row0 < (uint32_t)R ? m - 1u - row0 : 0xFFFFFFFFu)
                             : row0 >= m ? 0u : (m - row0 < (uint32_t)R ? m - row0 : (uint32_t)R);
}

// the pair's cell list and its cap (the exact-size lists of a re-run, else cell_cap cells per pair)
struct AffCells { uint2 *p; uint32_t cap; };
__device__ __forceinline__ AffCells aff_cell_list(const FillArgs &A, const PairDesc pd) {
    const uint64_t cbase = A.cells_off ? A.cells_off[pd.out_id] : (uint64_t)pd.out_id * A.cell_cap;
    const uint32_t ccap = A.cells_cap ? A.cells_cap[pd.out_id] : A.cell_cap;
    return AffCells{A.cells + cbase, ccap};
}

// The two pieces that read or write the lane's state S are shared as TEXT, not as functions.  As an inlined function -- handed
// S, its arrays, a pointer to them, or one row at a time by value -- either one changes the register allocation of the sweeps
// (DESIGN.md 8e); the same statements expanded in place cannot.  Both expect R, MATRIX, MODE, TWO, S, A, o, o2, e2 and the names below.
// AFF_LOAD_ROWS (readw, m, row0, nn): the lane's rows row0 + 1 .. row0 + R (global row indices) -- their base codes, with MATRIX
//   their row words class * (n+1) * 4 | hi << 16 (a read base inside the alphabet takes hi = 0x3FF, never a reference key's;
//   pad rows: class n, hi 0xFFFF) -- and H and E at column 0: 0 (local), else H(i,0) = o + i*e, E(i,0) := H(i,0) + o
//   AFF_OVERLAP: H(i,0) = 0 and the same stand-in, E(i,0) := o
//   TWO: H(i,0) = max(o + i*e, o2 + i*e2), E1(i,0) := H(i,0) + o, E2(i,0) := H(i,0) + o2
//   PROFILE (expects pbase, pnn): the row words are the byte offsets of the rows' table rows in aff_ptab -- dword pbase + row * pnn;
//   a pad row points at the read's row 0 (any valid row: it never competes).  The read's bytes are not read
#define AFF_LOAD_ROWS                                                                                         \
    _Pragma("unroll") for (int k = 0; k < R; ++k) {                                                           \
        const uint32_t row = row0 + (uint32_t)k;                                                              \
        S.q[k] = row < m ? (int)((readw[row >> 2] >> (8u * (row & 3u))) & 0xFFu) : (int)SWMI_CODE_PAD;        \
        if (MATRIX) {                                                                                         \
            const uint32_t key = row < m ? aff_mkey[S.q[k]] : ((nn - 1u) * 4u) | (0xFFFFu << 16);             \
            const uint32_t hi = (key >> 16) == 0x1FFu ? 0x3FFu : key >> 16;                                   \
            S.q[k] = (int)(((key & 0xFFFFu) * nn) | (hi << 16));                                              \
        }                                                                                                     \
        if (PROFILE) S.q[k] = (int)((pbase + (row < m ? row : 0u) * pnn) * 4u);                               \
        if constexpr (MODE == AFF_LOCAL) {                                                                    \
            S.h[k] = 0;                                                                                       \
            S.e[k] = 0;                                                                                       \
        } else if constexpr (MODE == AFF_OVERLAP) {                                                           \
            S.h[k] = 0;                                                                                       \
            S.e[k] = o;                                                                                       \
        } else {                                                                                              \
            S.h[k] = o + (int)(row + 1u) * A.gap;                                                             \
            if constexpr (TWO) S.h[k] = max(S.h[k], o2 + (int)(row + 1u) * e2);                               \
            S.e[k] = S.h[k] + o;                                                                              \
            if constexpr (TWO) S.e2[k] = S.h[k] + o2;                                                         \
        }                                                                                                     \
    }
// AFF_STORE_BLOCK (dir, w, lane): block w of a field, the codes of the lane's R rows, 256 contiguous bytes per row slot
//   TWO: the two planes of a block lie one behind the other -- dword ((w * 2 + plane) * R + k) * 64 + lane
#define AFF_STORE_BLOCK                                                                                       \
    uint32_t *__restrict__ dst = dir + (uint64_t)w * (TWO ? 2 : 1) * R * WAVE + lane;                         \
    _Pragma("unroll") for (int k = 0; k < R; ++k) dst[k * WAVE] = S.acc[k];                                   \
    if constexpr (TWO) { _Pragma("unroll") for (int k = 0; k < R; ++k) dst[(R + k) * WAVE] = S.acc2[k]; }
// AFF_PAIR_OUT(NCELLS, XFLAGS) (lane, pd, ccap): the pair's PairOut.  NCELLS is what the degenerate case counts -- the pair's m * n cells
//   or, under option "band", those inside the band -- and is evaluated in that branch only.  Text as well: as a function that
//   takes the count as a value it changes the short local sweeps, as one that picks it inside the banded local ones
//   XFLAGS: what the sweep reports above the flag bits -- the strips swept of a pair that option "xdrop" stopped
//   (SWMI_F_STRIPS_SHIFT), the constant 0 everywhere else
#define AFF_PAIR_OUT(NCELLS, XFLAGS)                                                                                \
    if (lane == 0) {                                                                                          \
        PairOut po;                                                                                           \
        if (MODE == AFF_LOCAL && S.cnt == 0u) {     /* maximum 0: every cell ties (SmithWaterman.java:154) */ \
            po.score = 0;                                                                                     \
            po.flags = SWMI_F_DEGENERATE;                                                                     \
            po.n_cells = NCELLS;                                                                              \
        } else {                                                                                              \
            po.score = S.thr;                                                                                 \
            po.flags = (S.cnt > ccap ? SWMI_F_CELL_OVF : 0u) | (XFLAGS);                                      \
            po.n_cells = S.cnt;                                                                               \
        }                                                                                                     \
        A.out[pd.out_id] = po;                                                                                \
    }
// AFF_PAIR_OUT_ENDB(ELANE) (lane, pd, m, cells, ccap, endb): the pair's PairOut under option "end_bonus" (DESIGN.md 8o), and its entry of
//   the launch's EndOut array, which lies behind the A.n_out pair outputs.  ELANE (wave-uniform) owns read row m: its (S.eg, S.egc)
//   are (end_score, end_col) -- it has swept at least one column of the row, no window being empty.  The pair is taken to the end iff
//   end_score + endb > max_score, in 64 bits; lane 0 then names (m, end_col) as the pair's one cell.  Every store of the wave's cell
//   list comes before that store in program order, and the wait puts them in memory first: another lane may have written entry 0.
//   A pair that is not taken leaves what AFF_PAIR_OUT leaves (an extend run has no degenerate case).
#define AFF_PAIR_OUT_ENDB(ELANE)                                                                              \
    {                                                                                                         \
        const int eg = __builtin_amdgcn_readlane(S.eg, (int)(ELANE));                                         \
        const uint32_t egc = (uint32_t)__builtin_amdgcn_readlane((int)S.egc, (int)(ELANE));                   \
        if (lane == 0) {                                                                                      \
            PairOut po;                                                                                       \
            EndOut eo;                                                                                        \
            eo.max_score = S.thr; eo.end_score = eg; eo.end_col = egc;                                        \
            if ((int64_t)eg + (int64_t)endb > (int64_t)S.thr) {                                               \
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                                            \
                cells[0] = make_uint2(m, egc);                                                                \
                po.score = eg;                                                                                \
                po.flags = SWMI_F_TO_END;                                                                     \
                po.n_cells = 1ull;                                                                            \
            } else {                                                                                          \
                po.score = S.thr;                                                                             \
                po.flags = S.cnt > ccap ? SWMI_F_CELL_OVF : 0u;                                               \
                po.n_cells = S.cnt;                                                                           \
            }                                                                                                 \
            A.out[pd.out_id] = po;                                                                            \
            reinterpret_cast<EndOut *>(A.out + A.n_out)[pd.out_id] = eo;                                      \
        }                                                                                                     \
    }

// SUBOPT: the row of column maxima lies behind the field; the lane that owns the read's last row, lact - 1 of swmi_aff_blocks, stores
// it -- W is sized for that lane to reach column n
// ENDB: the bonus endb of option "end_bonus"; the lane that owns read row m tracks it, and the choice is made with the PairOut
template <int R, bool STRICT, int MODE, uint32_t F>
__device__ __forceinline__ void aff_sweep_pair(const FillArgs &A, const int o, const PairDesc pd, const uint32_t lane, const uint32_t nn,
                                               const int o2, const int e2, const uint32_t endb, const uint32_t *__restrict__ pimg) {
    AFF_FLAG_NAMES(F)
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    uint32_t *__restrict__ dir = A.dir + pd.dir_off;
    const uint32_t W = swmi_aff_blocks(m, n);
    const uint32_t row0 = lane * R;
    const uint32_t vrows = aff_vrows<R, MODE>(m, row0);
    const AffCells cl = aff_cell_list(A, pd);
    const uint32_t ccap = cl.cap;
    uint2 *__restrict__ cells = cl.p;
    // PROFILE: nn carries the table's row stride n + 1 (low half) and the rows of a wavefront's table (high half); pimg is the
    // profiles' image (AffProfile, swmi_launch.h).  The wavefront stages its read's table, m rows, column n filled with mismatch:
    // entry x = row * pnn + c comes from scores[(row_off + row) * n + c], and x - row is row * n + c.  A read with more rows than
    // the launcher sized the tables for is not swept (it admits none).  The wavefront reads what its own lanes wrote: LDS
    // instructions of one wavefront complete in order, and the fence keeps the compiler from moving a read above the writes.
    [[maybe_unused]] const uint32_t pnn = nn & 0xFFFFu, pbase = (threadIdx.x >> 6) * (nn >> 16) * pnn;
    if constexpr (PROFILE) {
        if (m > (nn >> 16)) {                                    // never seen: the run fails (run_chunk reads the word)
            if (lane == 0 && A.err_host) *A.err_host = 1u;
            return;
        }
        const uint32_t sy = pnn - 1u;
        const uint64_t soff = *reinterpret_cast<const uint64_t *>(pimg + SWMI_PROF_KEY_WORDS);
        const uint64_t roff = reinterpret_cast<const uint64_t *>(pimg + SWMI_PROF_HDR_WORDS)[pd.read_id];
        const int *__restrict__ src = reinterpret_cast<const int *>(pimg) + soff + roff * sy;
        // (row and column of entry x run along with it: one division per lane, and one for the wavefront's step of 64 entries)
        const uint32_t rstep = uni(WAVE / pnn), cstep = uni(WAVE - rstep * pnn);
        uint32_t row = lane / pnn, c = lane - row * pnn;
        for (uint32_t x = lane; x < m * pnn; x += WAVE) {
            aff_ptab[pbase + x] = c == sy ? A.mismatch : src[x - row];
            row += rstep; c += cstep;
            if (c >= pnn) { c -= pnn; row += 1u; }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }

    AffState<R> S;
    AFF_LOAD_ROWS
    S.rb = 0; S.nh_prev = 0; S.f_last = 0;                       // (nh_prev of lane 0: H(0,0) = 0 in every mode)
    if constexpr (TWO) S.f2_last = 0;
    S.thr = MODE == AFF_LOCAL ? 1 : MODE == AFF_OVERLAP ? INT32_MIN + 1 : INT32_MIN; S.cnt = 0;
    AffSeam Zs{};                                                // (SUBOPT, ENDB, AFF_OVERLAP; nothing else reads it in a short sweep)
    if constexpr (MODE == AFF_OVERLAP) Zs.elane = uni((m - 1u) / (uint32_t)R);      // the lane that owns read row m
    if constexpr (SUBOPT) {
        S.cm = 0;
        Zs.cmrow = reinterpret_cast<int *>(dir + (uint64_t)W * R * WAVE);
        Zs.cmlane = (m + (uint32_t)R - 1u) / (uint32_t)R - 1u;
        if constexpr (HITS) { S.cmr = 0; Zs.cmrs = (uint32_t)swmi_aff_colmax_stride(n); }
    }
    if constexpr (ENDB) {
        S.eg = INT32_MIN; S.egc = 0u;
        Zs.elane = uni((m - 1u) / (uint32_t)R);
    }
    for (uint32_t w = 0; w < W; ++w) {
        const uint32_t t0 = 8u * w;
        // lane 0's 8 reference bases (images are padded: the last block may read past the end)
        const uint2 rw = *reinterpret_cast<const uint2 *>(refw + (t0 >> 2));
#pragma unroll
        for (int k = 0; k < R; ++k) S.acc[k] = 0u;
        if constexpr (TWO) {
#pragma unroll
            for (int k = 0; k < R; ++k) S.acc2[k] = 0u;
        }
        aff_block8<R, STRICT, MODE, F>(S, rw, t0, lane, n, row0, vrows, o, A.gap, A.match, A.mismatch, cells, ccap, Zs, o2, e2);
        AFF_STORE_BLOCK
    }
    if constexpr (ENDB) AFF_PAIR_OUT_ENDB(Zs.elane)
    else
    AFF_PAIR_OUT((uint64_t)m * n, 0u)
}

// A read of more than 1024 bases, strip after strip (R = 16 in every strip), over the same pieces as aff_sweep_pair.  Strip sx
// sweeps a WINDOW of columns clo .. chi and leaves the field of a (1024, chi - clo + 1) pair behind the fields of the strips
// above; aff_block8 counts columns from the window's first one.  !BAND: the window is the whole reference -- clo = 1, chi = n,
// the same W blocks in every strip -- and everything that depends on it is a constant that folds away.
// BAND (option "band", half-width wb >= 1): clo, chi = swmi_aff_band_lo / _hi (sx), and
//   - a cell outside the band reads as OUT: 0 in local mode (what the clamps make of -inf), SWMI_AFF_BAND_NEG otherwise
//   - column clo - 1 of the strip's rows is the mode's column 0 when clo = 1, else OUT (H and E)
//   - nh_prev of lane 0, the diagonal of the strip's first row at column clo, is H(1024 sx, clo - 1): the mode's value when
//     clo = 1, else the seam's -- the strip above wrote it, clo(sx) - 1 >= clo(sx - 1)
//   - lane 0's feed from above is the seam up to column chi(sx - 1), the last one the strip above wrote, and OUT beyond: the
//     seam words there are stale (!BAND: every column of the seam is the strip above's)
//   - the reference words are read from byte clo - 1 of the image, which is not 8-aligned: three dwords, two byte-aligns
//   - the strips' fields are of unequal size: the field pointer runs
// The seam row is rewritten IN PLACE.  In strip sx lane 0 is at column clo + t at step t and loads the seam of its block's 8
// columns clo + t0 .. clo + t0 + 7 at the block's first step t0 <= t, so a load at step t touches columns >= clo + t; lane 63 is
// at column clo + t - 63 at step t.  A column is therefore read (by this strip) at least 63 steps before this strip overwrites
// it.  Column clo - 1 (nh_prev) is left of the window and not written by this strip at all.  What strip sx reads, columns
// clo(sx) - 1 .. chi(sx - 1), lies inside clo(sx - 1) .. chi(sx - 1), all written by the strip above, whose stores all precede
// the fence between the strips (clo = 1: columns 1 .. n, and column 0 is the mode's).  Vector loads and stores only: the row is
// rewritten by vector stores of this kernel, which the scalar cache does not see.
// XDROP (option "xdrop", threshold xd >= 1, extend runs only): at the top of strip sx >= 1, behind the same fence,
//   the wave takes the maximum of H over the seam row inside the window of strip sx - 1 -- seam[j - 1].x, 64 columns per step,
//   vector loads for the reason above; lane 63 of strip sx - 1 wrote every one of them before the fence -- and ends the pair
//   when the running maximum S.thr lies more than xd above it: the strips from sx on are not swept, the cell list holds the
//   cells of rows <= 1024 sx, and the PairOut carries sx, the strips swept, above its flag bits.  The comparison is made once per
//   strip on wave-uniform values, in 64 bits.  Nothing enters the block loop.
// ADAPT (option "band_adapt", with BAND and AFF_EXTEND): the window follows a centre, cen = c(sx - 1), 0 for strip
//   0: clo, chi = swmi_aff_adapt_lo / _hi (cen).  At the top of strip sx >= 1, behind the same fence, ONE pass over the seam row
//   inside the window of strip sx - 1 finds the maximum of H there and p, the smallest column that holds it: a lane keeps its
//   first strictly larger value (its columns ascend), the wave takes the maximum and then the smallest column among the lanes
//   that hold it, both through wave_max_i32, so both are wave-uniform.  XDROP's test runs on the same maximum and comes first: a
//   pair it stops places no further window.  Then cen = max(cen, p).  What differs from the static staircase:
//   - the windows are monotone but clo may STAND STILL: clo(sx) = clo(sx - 1) > 1.  Column clo - 1 of the seam row was then not
//     written by the strip above (it lies left of ITS window too), and nh_prev is OUT, not a seam load.  Otherwise clo(sx) - 1 >=
//     clo(sx - 1) as before.  The strip's own column clo - 1 (S.h, S.e) is OUT whenever clo > 1, as under BAND
//   - seam_end is chi(sx - 1) - (clo - 1): lane 0's loads stay inside clo(sx - 1) .. chi(sx - 1), since clo(sx) >= clo(sx - 1)
//   - the in-place argument above is relative to the window's first column and holds as it stands; the pass reads the row
//     before the strip stores anything
//   - every strip's field has the fixed stride swmi_aff_adapt_strip_words: the window is not known before the strip above ends
//   - lane 0 leaves cen in the pair's window table behind the fields (a vector store), for the traceback and the host
// TWO (option "gap_open2"): the seam row carries (H, F1, F2) per column in 16-byte entries (int4, the fourth word
//   unused), so that lane 0's load and lane 63's store stay one instruction each; the pair's seam row is 4 n dwords and starts on
//   a 16-byte boundary (every pair of such a run has a row of that kind).  The in-place argument above counts COLUMNS, not bytes,
//   and an entry is read and written whole: in strip sx lane 0 loads the entries of columns clo + t0 .. clo + t0 + 7 at step t0,
//   lane 63 stores the entry of column clo + t - 63 at step t, so every entry is read at least 63 steps before this strip
//   overwrites it, as it stands for 8-byte entries.  nh_prev reads word x of the entry of column clo - 1.  A strip's field is
//   twice swmi_aff_strip_words of its window; under BAND a cell outside reads SWMI_AFF_BAND_NEG in all five values.
// SUBOPT (option "subopt", local runs): the pair's row of column maxima, n int32 behind the strips' fields, is rewritten IN
//   PLACE strip after strip like the seam row, and the argument above holds word for word: lane 0 loads the row's entries of columns
//   clo + t0 .. clo + t0 + 7 at step t0, lane 63 stores the entry of column clo + t - 63 at step t, behind the same fence.  Lane 63
//   stores in EVERY strip, the last one too.  The row is indexed by the global column: under BAND a column left of a later strip's
//   window keeps what the earlier strips left, and lane 0 starts a column the strips above never reached (beyond seam_end) at 0 --
//   the words there were never written.  Columns right of the last window stay unwritten: readers stop at swmi_aff_colmax_cols.
// ENDB (option "end_bonus", extend runs): read row m lies in the last strip alone, in lane (m - 1 - 1024 (NS - 1)) / 16; the
//   strips above name no owner (Z.elane = 0xFFFFFFFF) and leave (S.eg, S.egc) as they were set before the first.  Under BAND the row's
//   existing cells are the columns of the last strip's window, and the column kept is global (Z.coff).  Nothing is loaded or stored.
// HITS (with SUBOPT): the row of rows lies swmi_aff_colmax_stride(n) dwords behind the row of column maxima and is rewritten
//   in place with it -- the same loads by lanes 0..7 at step t0, the same stores by lane 63 at step t, so an entry of either row is read at
//   least 63 steps before this strip overwrites it.  A strip keeps the row the strips above left unless it holds a strictly greater
//   value: the smallest row survives the seam.
template <bool STRICT, int MODE, uint32_t F>
__device__ __forceinline__ void aff_sweep_long_pair(const FillArgs &A, const int o, const PairDesc pd, const uint32_t lane, const uint32_t nn,
                                                    const uint32_t wb, const uint32_t xd, const int o2, const int e2, const uint32_t endb) {
    AFF_FLAG_NAMES(F)
    constexpr int R = SWMI_AFF_RMAX;
    constexpr int OUT = BAND && MODE != AFF_LOCAL ? SWMI_AFF_BAND_NEG : 0;
    static_assert(!PROFILE, "a long read has no profile sweep: one table per strip is not built");
    [[maybe_unused]] constexpr uint32_t pbase = 0u, pnn = 0u;    // (names of AFF_LOAD_ROWS under PROFILE)
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const uint32_t NS = swmi_aff_strips(m);
    uint32_t W = BAND ? 0u : swmi_aff_strip_blocks(n);           // (BAND: of strip sx, set with its window)
    const AffCells cl = aff_cell_list(A, pd);
    const uint32_t ccap = cl.cap;
    uint2 *__restrict__ cells = cl.p;
    int2 *const seam = reinterpret_cast<int2 *>(A.seam + pd.seam_off);
    int4 *const seam4 = reinterpret_cast<int4 *>(A.seam + pd.seam_off);     // (TWO)
    AffSeam Z;
    Z.row = seam;
    Z.row4 = seam4;
    // SUBOPT: the row of column maxima, behind the last strip's field
    int *const cmbase = SUBOPT ? reinterpret_cast<int *>(A.dir + pd.dir_off + (BAND ? swmi_aff_band_strip_off(NS, n, wb) : (uint64_t)NS * swmi_aff_strip_words(n)))
                               : nullptr;
    if constexpr (SUBOPT) { Z.cmrow = cmbase; Z.cmlane = 63u; }
    if constexpr (HITS) Z.cmrs = (uint32_t)swmi_aff_colmax_stride(n);
    uint32_t *__restrict__ dir = A.dir + pd.dir_off;
    uint64_t inband = 0ull;                                      // BAND: in-band cells with i <= m (the degenerate count)
    uint32_t stopped = 0u;                                       // XDROP: the strips swept of a pair that was stopped, else 0
    uint32_t cen = 0u, plo = 1u, phi = 0u;                       // ADAPT: the centre c(sx - 1); the window of the strip above
    const uint64_t astride = ADAPT ? swmi_aff_adapt_strip_words(n, wb) : 0ull;       // ADAPT: dwords of every strip's field
    uint32_t *const wtab = ADAPT ? A.dir + pd.dir_off + (uint64_t)NS * astride : nullptr;   // ADAPT: the pair's window table

    AffState<R> S;
    S.thr = MODE == AFF_LOCAL ? 1 : MODE == AFF_OVERLAP ? INT32_MIN + 1 : INT32_MIN; S.cnt = 0;       // (wave-uniform: they live on across the strips)
    const uint32_t elast = ENDB || MODE == AFF_OVERLAP ? uni((m - 1u - (NS - 1u) * SWMI_AFF_MAX_READ) / (uint32_t)R) : 0u;      // ENDB: the lane of the last strip that owns read row m
    if constexpr (ENDB) { S.eg = INT32_MIN; S.egc = 0u; }
    for (uint32_t sx = 0; sx < NS; ++sx) {
        const uint32_t row0 = sx * SWMI_AFF_MAX_READ + lane * R;             // global index of the lane's first row, less 1
        const uint32_t vrows = aff_vrows<R, MODE>(m, row0);               // (row m is in the last strip)
        uint32_t clo = 1u, nw = n, seam_end = n;                 // the window's first column and length; the window columns the strip above wrote
        if constexpr (ADAPT) {
            if (sx) {
                // the strip above has written its window of the seam row (the fence of the static sweeps, taken here: the window
                // of this strip hangs on what the pass loads)
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
                // (four loads in flight per lane, as in the XDROP pass; the seam row is indexed by j - 1)
                int bv = INT32_MIN;
                uint32_t bc = 0u;
                uint32_t c = plo - 1u + lane;
                for (; c + 3u * WAVE < phi; c += 4u * WAVE) {
                    const int s0 = seam[c].x, s1 = seam[c + WAVE].x, s2 = seam[c + 2u * WAVE].x, s3 = seam[c + 3u * WAVE].x;
                    if (s0 > bv) { bv = s0; bc = c; }
                    if (s1 > bv) { bv = s1; bc = c + WAVE; }
                    if (s2 > bv) { bv = s2; bc = c + 2u * WAVE; }
                    if (s3 > bv) { bv = s3; bc = c + 3u * WAVE; }
                }
                for (; c < phi; c += WAVE) {
                    const int s0 = seam[c].x;
                    if (s0 > bv) { bv = s0; bc = c; }
                }
                const int smax = wave_max_i32(bv);               // seam(sx - 1): a real H, above INT32_MIN
                if constexpr (XDROP) {
                    if ((int64_t)S.thr - (int64_t)smax > (int64_t)xd) { stopped = sx; break; }
                }
                // p(sx - 1): the smallest column among the lanes that hold the maximum (bc < 2^31: its negative orders them)
                const uint32_t p = (uint32_t)(-wave_max_i32(bv == smax ? -(int)bc : INT32_MIN)) + 1u;
                if (p > cen) cen = p;
            }
            if (lane == 0) wtab[sx] = cen;
            clo = swmi_aff_adapt_lo(cen, wb);
            nw = swmi_aff_adapt_hi(cen, n, wb) - clo + 1u;
            W = swmi_aff_strip_blocks(nw);
            seam_end = sx ? phi - (clo - 1u) : 0u;
        } else if constexpr (BAND) {
            clo = swmi_aff_band_lo(sx, wb);
            nw = swmi_aff_band_hi(sx, n, wb) - clo + 1u;
            W = swmi_aff_strip_blocks(nw);
            seam_end = sx ? swmi_aff_band_hi(sx - 1u, n, wb) - (clo - 1u) : 0u;
            const uint32_t srows = m - sx * SWMI_AFF_MAX_READ < SWMI_AFF_MAX_READ ? m - sx * SWMI_AFF_MAX_READ : SWMI_AFF_MAX_READ;
            inband += (uint64_t)srows * nw;
        }
        AFF_LOAD_ROWS
        if constexpr (BAND) {
            if (clo > 1u) {
#pragma unroll
                for (int k = 0; k < R; ++k) { S.h[k] = OUT; S.e[k] = OUT; }
                if constexpr (TWO) {
#pragma unroll
                    for (int k = 0; k < R; ++k) S.e2[k] = OUT;
                }
            }
        }
        S.rb = 0; S.f_last = 0;
        if constexpr (TWO) S.f2_last = 0;
        if constexpr (SUBOPT) S.cm = 0;
        if constexpr (HITS) S.cmr = 0;
        // nh_prev of lane 0: H(1024 * sx, clo - 1)
        if constexpr (!BAND) S.nh_prev = AFF_COL0_GAPS(MODE) && sx ? o + (int)(sx * SWMI_AFF_MAX_READ) * A.gap : 0;
        if constexpr (!BAND && TWO) { if (sx) S.nh_prev = max(S.nh_prev, o2 + (int)(sx * SWMI_AFF_MAX_READ) * e2); }
        if constexpr (BAND) {
            Z.row = seam + (clo - 1u);
            if constexpr (TWO) Z.row4 = seam4 + (clo - 1u);
            Z.coff = clo - 1u;
            if constexpr (SUBOPT) Z.cmrow = cmbase + (clo - 1u);
        }
        Z.wlane = sx + 1u < NS ? 63u : 0xFFFFFFFFu;
        if constexpr (ENDB || MODE == AFF_OVERLAP) Z.elane = sx + 1u < NS ? 0xFFFFFFFFu : elast;
        if constexpr (!BAND) dir = A.dir + pd.dir_off + (uint64_t)sx * (TWO ? 2u : 1u) * swmi_aff_strip_words(n);
        if constexpr (ADAPT) dir = A.dir + pd.dir_off + (uint64_t)sx * astride;
        // the strip above has written its window of the seam row: its stores are in memory before this strip loads any of it
        if constexpr (!ADAPT) { if (sx) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent"); }
        if constexpr (XDROP && !ADAPT) {
            if (sx) {
                // seam(sx - 1): the maximum of H(1024 sx, j) over the window of strip sx - 1 (the seam row is indexed by j - 1)
                const uint32_t plo = BAND ? swmi_aff_band_lo(sx - 1u, wb) : 1u, phi = BAND ? swmi_aff_band_hi(sx - 1u, n, wb) : n;
                // (four loads in flight per lane: one after the other, a 10 kbp row is 157 round trips to HBM per test)
                int smax = INT32_MIN;
                uint32_t c = plo - 1u + lane;
                for (; c + 3u * WAVE < phi; c += 4u * WAVE) {
                    const int s0 = seam[c].x, s1 = seam[c + WAVE].x, s2 = seam[c + 2u * WAVE].x, s3 = seam[c + 3u * WAVE].x;
                    smax = max(max(smax, max(s0, s1)), max(s2, s3));
                }
                for (; c < phi; c += WAVE) smax = max(smax, seam[c].x);
                smax = wave_max_i32(smax);
                if ((int64_t)S.thr - (int64_t)smax > (int64_t)xd) { stopped = sx; break; }
            }
        }
        if constexpr (BAND) {
            if (clo > 1u) S.nh_prev = !ADAPT || clo > plo ? (TWO ? seam4[clo - 2u].x : seam[clo - 2u].x) : OUT;   // (a vector load, behind the fence; ADAPT: a window that stood still)
            else S.nh_prev = MODE != AFF_LOCAL && sx ? o + (int)(sx * SWMI_AFF_MAX_READ) * A.gap : 0;
            if constexpr (TWO) { if (clo <= 1u && sx) S.nh_prev = max(S.nh_prev, o2 + (int)(sx * SWMI_AFF_MAX_READ) * e2); }
        }
        const uint32_t boff = clo - 1u, bsh = boff & 3u;         // (BAND) the window's first byte of the image
        const uint32_t *__restrict__ refb = refw + (boff >> 2);
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t t0 = 8u * w;
            // lane 0's 8 reference bases, from byte boff + t0 on (the image's padding covers the last block and the third dword)
            uint2 rw;
            if constexpr (BAND) {
                const uint32_t r0 = refb[t0 >> 2], r1 = refb[(t0 >> 2) + 1u], r2 = refb[(t0 >> 2) + 2u];
                rw = make_uint2(__builtin_amdgcn_alignbyte(r1, r0, bsh), __builtin_amdgcn_alignbyte(r2, r1, bsh));
            } else {
                rw = *reinterpret_cast<const uint2 *>(refb + (t0 >> 2));
            }
            // lane 0's feed from above at window columns t0 + 1 .. t0 + 8, one column per lane 0..7: row 0 of the mode (as in
            // aff_block8; strip 0 has clo = 1), below it the seam -- the true F, not the H + o stand-in of row 0
            const uint32_t c = t0 + lane;
            Z.h = AFF_ROW0_GAPS(MODE) ? (int)((uint32_t)o + (c + 1u) * (uint32_t)A.gap) : 0;
            if constexpr (TWO) Z.h = max(Z.h, (int)((uint32_t)o2 + (c + 1u) * (uint32_t)e2));
            Z.f = MODE == AFF_LOCAL ? 0 : (int)((uint32_t)Z.h + (uint32_t)o);
            if constexpr (TWO) {
                Z.f2 = (int)((uint32_t)Z.h + (uint32_t)o2);
                if (sx) {
                    int4 v = make_int4(OUT, OUT, OUT, 0);
                    if (lane < 8u && c < seam_end) v = Z.row4[c];
                    Z.h = v.x; Z.f = v.y; Z.f2 = v.z;
                }
            } else
            if (sx) {
                int2 v = make_int2(OUT, OUT);
                if (lane < 8u && c < seam_end) v = Z.row[c];
                Z.h = v.x; Z.f = v.y;
            }
            if constexpr (SUBOPT) {
                // what the strips above left at lane 0's 8 columns (a vector load, behind the fence); 0 in strip 0 and beyond seam_end
                Z.cm = 0;
                if (sx && lane < 8u && c < seam_end) Z.cm = Z.cmrow[c];
                if constexpr (HITS) {
                    Z.cmr = 0;
                    if (sx && lane < 8u && c < seam_end) Z.cmr = Z.cmrow[c + Z.cmrs];
                }
            }
#pragma unroll
            for (int k = 0; k < R; ++k) S.acc[k] = 0u;
            if constexpr (TWO) {
#pragma unroll
                for (int k = 0; k < R; ++k) S.acc2[k] = 0u;
            }
            aff_block8<R, STRICT, MODE, F>(S, rw, t0, lane, nw, row0, vrows, o, A.gap, A.match, A.mismatch, cells, ccap, Z, o2, e2);
            AFF_STORE_BLOCK
        }
        if constexpr (BAND && !ADAPT) dir += (uint64_t)W * (TWO ? 2 : 1) * R * WAVE;
        if constexpr (ADAPT) { plo = clo; phi = clo + nw - 1u; }
    }
    if constexpr (ENDB) AFF_PAIR_OUT_ENDB(elast)
    else
    AFF_PAIR_OUT(BAND ? inband : (uint64_t)m * n, XDROP ? stopped << SWMI_F_STRIPS_SHIFT : 0u)
}

#undef AFF_LOAD_ROWS
#undef AFF_STORE_BLOCK
#undef AFF_PAIR_OUT
#undef AFF_PAIR_OUT_ENDB

// RLO..RHI: the rows per lane this instantiation of the kernel takes (the others' registers would cap its occupancy)
template <int RLO, int RHI, bool STRICT, int MODE, uint32_t F>
__device__ __forceinline__ void aff_sweep_dispatch(const FillArgs &A, const int o, const PairDesc pd, const uint32_t R, const uint32_t lane,
                                                   const uint32_t nn, const int o2, const int e2, const uint32_t endb,
                                                   const uint32_t *__restrict__ pimg) {
    if constexpr (RLO <= RHI) {
        if (R == (uint32_t)RLO) aff_sweep_pair<RLO, STRICT, MODE, F>(A, o, pd, lane, nn, o2, e2, endb, pimg);
        else aff_sweep_dispatch<RLO + 1, RHI, STRICT, MODE, F>(A, o, pd, R, lane, nn, o2, e2, endb, pimg);
    }
}

// The body of every sweep kernel.  Its arguments are the kernels', in their order, a constant where a kernel has none: o2, e2
// (TWO) the second piece's open and extension; mat, nn (MATRIX) the score matrix image (swmi_aff_mat_words) and its side n + 1;
// wb (BAND) the half-width; xd (XDROP) the threshold; endb (ENDB) the bonus.  LONG: RLO and RHI are not used.  Which flags may
// meet is aff_flags_ok (swmi_launch.h)
// PROFILE (the rows of AFF_PROFILE_SWEEPS): mat is the profiles' image (AffProfile, swmi_launch.h) and nn is
// (n + 1) | rows << 16, rows being the rows of one wavefront's LDS table -- what the launcher sized the workgroup by
template <int RLO, int RHI, int MODE, uint32_t F>
__device__ __forceinline__ void aff_sweep_entry(const FillArgs &A, const int o, const int o2, const int e2, const uint32_t *__restrict__ mat,
                                                const uint32_t nn, const uint32_t wb, const uint32_t xd, const uint32_t endb) {
    static_assert(aff_flags_ok(MODE, F), "no such sweep");
    AFF_FLAG_NAMES(F)
    if (blockIdx.x == 0 && threadIdx.x == 0) A.hdr->reserved = 0ull;      // the traceback's bump allocator
    if (MATRIX) {                                                          // (before any wavefront leaves)
        for (uint32_t x = threadIdx.x; x < 256u; x += WAVE * AFF_WAVES) aff_mkey[x] = mat[x];
        const uint32_t n = nn - 1u;
        for (uint32_t x = threadIdx.x; x < nn * nn; x += WAVE * AFF_WAVES) {
            const uint32_t cq = x / nn, cr = x - cq * nn;
            aff_mtab[x] = (cq == n || cr == n) ? A.mismatch : (int)mat[256u + x];
        }
        __syncthreads();
    }
    if constexpr (PROFILE) {
        // the keys alone are the workgroup's (class * 4, class n outside the alphabet); every wavefront stages its own read's
        // table (aff_sweep_pair).  The workgroup has as many wavefronts as the launcher gave it, 1 .. AFF_WAVES
        for (uint32_t x = threadIdx.x; x < SWMI_PROF_KEY_WORDS; x += blockDim.x) aff_mkey[x] = mat[x];
        __syncthreads();
    }
    const uint32_t pair = blockIdx.x * (PROFILE ? blockDim.x >> 6 : (uint32_t)AFF_WAVES) + (threadIdx.x >> 6);
    if (pair >= A.n_pairs) return;
    const uint32_t lane = threadIdx.x & 63u;
    const PairDesc pd = A.pairs[pair];
    if constexpr (LONG) {
        if (uni(A.reads[pd.read_id].len) <= SWMI_AFF_MAX_READ) return;
        if (A.strict) aff_sweep_long_pair<true, MODE, F>(A, o, pd, lane, nn, wb, xd, o2, e2, endb);
        else          aff_sweep_long_pair<false, MODE, F>(A, o, pd, lane, nn, wb, xd, o2, e2, endb);
        return;
    }
    const uint32_t R = uni(swmi_aff_rows_per_lane(A.reads[pd.read_id].len));
    if (R < (uint32_t)RLO || R > (uint32_t)RHI) return;
    if (A.strict) aff_sweep_dispatch<RLO, RHI, true, MODE, F>(A, o, pd, R, lane, nn, o2, e2, endb, mat);
    else          aff_sweep_dispatch<RLO, RHI, false, MODE, F>(A, o, pd, R, lane, nn, o2, e2, endb, mat);
}

}  // namespace

// THE LIST OF SWEEPS.  One row per kernel: its name, the rows per lane it takes (RLO .. RHI: 1 .. 4 narrow, 5 .. 16 wide; the strip
// sweeps of option "long_reads" have 16 and do not use them), its MODE, and the flags of swmi_launch.h as 0 / 1.  The definitions
// just below and the launcher's table at the end of the file are this list under two macros; DESIGN.md 8q says how to add an option.
//                                                     RLO RHI  MODE     MATRIX LONG BAND XDROP ADAPT TWO SUBOPT ENDB HITS
#define AFF_SWEEPS(X)                                                                                     \
    X(sw_affine_sweep_kernel,                          1,  4, AFF_LOCAL,  0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_wide_kernel,                     5, 16, AFF_LOCAL,  0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_kernel,                    16, 16, AFF_LOCAL,  0, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_matrix_kernel,                   1,  4, AFF_LOCAL,  1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_matrix_wide_kernel,              5, 16, AFF_LOCAL,  1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_matrix_kernel,             16, 16, AFF_LOCAL,  1, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_fit_kernel,                      1,  4, AFF_FIT,    0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_fit_wide_kernel,                 5, 16, AFF_FIT,    0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_fit_kernel,                16, 16, AFF_FIT,    0, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_fit_matrix_kernel,               1,  4, AFF_FIT,    1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_fit_matrix_wide_kernel,          5, 16, AFF_FIT,    1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_fit_matrix_kernel,         16, 16, AFF_FIT,    1, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_global_kernel,                   1,  4, AFF_GLOBAL, 0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_global_wide_kernel,              5, 16, AFF_GLOBAL, 0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_global_kernel,             16, 16, AFF_GLOBAL, 0, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_global_matrix_kernel,            1,  4, AFF_GLOBAL, 1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_global_matrix_wide_kernel,       5, 16, AFF_GLOBAL, 1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_global_matrix_kernel,      16, 16, AFF_GLOBAL, 1, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_kernel,                    16, 16, AFF_LOCAL,  0, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_matrix_kernel,             16, 16, AFF_LOCAL,  1, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_fit_kernel,                16, 16, AFF_FIT,    0, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_fit_matrix_kernel,         16, 16, AFF_FIT,    1, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_global_kernel,             16, 16, AFF_GLOBAL, 0, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_global_matrix_kernel,      16, 16, AFF_GLOBAL, 1, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_extend_kernel,                   1,  4, AFF_EXTEND, 0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_extend_wide_kernel,              5, 16, AFF_EXTEND, 0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_extend_kernel,             16, 16, AFF_EXTEND, 0, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_extend_matrix_kernel,            1,  4, AFF_EXTEND, 1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_extend_matrix_wide_kernel,       5, 16, AFF_EXTEND, 1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_extend_matrix_kernel,      16, 16, AFF_EXTEND, 1, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_extend_kernel,             16, 16, AFF_EXTEND, 0, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_extend_matrix_kernel,      16, 16, AFF_EXTEND, 1, 1, 1, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_xdrop_kernel,              16, 16, AFF_EXTEND, 0, 1, 0, 1, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_xdrop_matrix_kernel,       16, 16, AFF_EXTEND, 1, 1, 0, 1, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_xdrop_kernel,              16, 16, AFF_EXTEND, 0, 1, 1, 1, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_xdrop_matrix_kernel,       16, 16, AFF_EXTEND, 1, 1, 1, 1, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_adapt_kernel,              16, 16, AFF_EXTEND, 0, 1, 1, 0, 1, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_adapt_matrix_kernel,       16, 16, AFF_EXTEND, 1, 1, 1, 0, 1, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_adapt_xdrop_kernel,        16, 16, AFF_EXTEND, 0, 1, 1, 1, 1, 0, 0, 0, 0) \
    X(sw_affine_sweep_band_adapt_xdrop_matrix_kernel, 16, 16, AFF_EXTEND, 1, 1, 1, 1, 1, 0, 0, 0, 0) \
    X(sw_affine_sweep_subopt_kernel,                   1,  4, AFF_LOCAL,  0, 0, 0, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_subopt_wide_kernel,              5, 16, AFF_LOCAL,  0, 0, 0, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_long_subopt_kernel,             16, 16, AFF_LOCAL,  0, 1, 0, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_subopt_matrix_kernel,            1,  4, AFF_LOCAL,  1, 0, 0, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_subopt_matrix_wide_kernel,       5, 16, AFF_LOCAL,  1, 0, 0, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_long_subopt_matrix_kernel,      16, 16, AFF_LOCAL,  1, 1, 0, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_band_subopt_kernel,             16, 16, AFF_LOCAL,  0, 1, 1, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_band_subopt_matrix_kernel,      16, 16, AFF_LOCAL,  1, 1, 1, 0, 0, 0, 1, 0, 0) \
    X(sw_affine_sweep_hits_kernel,                     1,  4, AFF_LOCAL,  0, 0, 0, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_hits_wide_kernel,                5, 16, AFF_LOCAL,  0, 0, 0, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_long_hits_kernel,               16, 16, AFF_LOCAL,  0, 1, 0, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_hits_matrix_kernel,              1,  4, AFF_LOCAL,  1, 0, 0, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_hits_matrix_wide_kernel,         5, 16, AFF_LOCAL,  1, 0, 0, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_long_hits_matrix_kernel,        16, 16, AFF_LOCAL,  1, 1, 0, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_band_hits_kernel,               16, 16, AFF_LOCAL,  0, 1, 1, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_band_hits_matrix_kernel,        16, 16, AFF_LOCAL,  1, 1, 1, 0, 0, 0, 1, 0, 1) \
    X(sw_affine_sweep_endb_kernel,                     1,  4, AFF_EXTEND, 0, 0, 0, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep_endb_wide_kernel,                5, 16, AFF_EXTEND, 0, 0, 0, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep_long_endb_kernel,               16, 16, AFF_EXTEND, 0, 1, 0, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep_endb_matrix_kernel,              1,  4, AFF_EXTEND, 1, 0, 0, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep_endb_matrix_wide_kernel,         5, 16, AFF_EXTEND, 1, 0, 0, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep_long_endb_matrix_kernel,        16, 16, AFF_EXTEND, 1, 1, 0, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep_band_endb_kernel,               16, 16, AFF_EXTEND, 0, 1, 1, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep_band_endb_matrix_kernel,        16, 16, AFF_EXTEND, 1, 1, 1, 0, 0, 0, 0, 1, 0) \
    X(sw_affine_sweep2_global_kernel,                  1,  4, AFF_GLOBAL, 0, 0, 0, 0, 0, 1, 0, 0, 0) \
    X(sw_affine_sweep2_global_wide_kernel,             5, 16, AFF_GLOBAL, 0, 0, 0, 0, 0, 1, 0, 0, 0) \
    X(sw_affine_sweep2_long_global_kernel,            16, 16, AFF_GLOBAL, 0, 1, 0, 0, 0, 1, 0, 0, 0) \
    X(sw_affine_sweep2_band_global_kernel,            16, 16, AFF_GLOBAL, 0, 1, 1, 0, 0, 1, 0, 0, 0) \
    X(sw_affine_sweep2_extend_kernel,                  1,  4, AFF_EXTEND, 0, 0, 0, 0, 0, 1, 0, 0, 0) \
    X(sw_affine_sweep2_extend_wide_kernel,             5, 16, AFF_EXTEND, 0, 0, 0, 0, 0, 1, 0, 0, 0) \
    X(sw_affine_sweep2_long_extend_kernel,            16, 16, AFF_EXTEND, 0, 1, 0, 0, 0, 1, 0, 0, 0) \
    X(sw_affine_sweep2_band_extend_kernel,            16, 16, AFF_EXTEND, 0, 1, 1, 0, 0, 1, 0, 0, 0)
static_assert(SWMI_AFF_RMAX == 16, "the RHI column of the list");
// A kernel's parameters are pieces, one per flag that has any, in this order (TWO and MATRIX never meet): AFF_IF_<flag>(text) is
// the text under a set flag, AFF_SEL_<flag>(a, b) is a under a set flag and b otherwise.
//   const FillArgs A, const int gap_open [, gap_open2, gap2: TWO] [, mat, nn: MATRIX] [, band: BAND] [, xdrop: XDROP] [, end_bonus: ENDB]
#define AFF_IF_0(...)
#define AFF_IF_1(...) __VA_ARGS__
#define AFF_SEL_0(a, b) b
#define AFF_SEL_1(a, b) a
// The MATRIX column of a row of AFF_PROFILE_SWEEPS is 2: the kernel has the matrix sweeps' piece (mat, nn) with the meaning
// aff_sweep_entry gives it under PROFILE, and its flags word is AFF_F_PROFILE in place of AFF_F_MATRIX
#define AFF_IF_2(...) __VA_ARGS__
#define AFF_SEL_2(a, b) a
#define AFF_ROW_FLAGS(MATRIX, LONG, BAND, XDROP, ADAPT, TWO, SUBOPT, ENDB, HITS)                                                              \
    (aff_flags((MATRIX) == 1, LONG, BAND, XDROP, ADAPT, TWO, SUBOPT, ENDB, HITS) | ((MATRIX) == 2 ? AFF_F_PROFILE : 0u))
#define AFF_SWEEP_KERNEL(name, RLO, RHI, MODE, MATRIX, LONG, BAND, XDROP, ADAPT, TWO, SUBOPT, ENDB, HITS)                                    \
    static_assert(aff_flags_ok(MODE, AFF_ROW_FLAGS(MATRIX, LONG, BAND, XDROP, ADAPT, TWO, SUBOPT, ENDB, HITS)), #name);                      \
    extern "C" __global__ void __launch_bounds__(WAVE * AFF_WAVES) name(const FillArgs A, const int gap_open                                  \
            AFF_IF_##TWO(, const int gap_open2, const int gap2) AFF_IF_##MATRIX(, const uint32_t *mat, const uint32_t nn)                    \
            AFF_IF_##BAND(, const uint32_t band) AFF_IF_##XDROP(, const uint32_t xdrop) AFF_IF_##ENDB(, const uint32_t end_bonus)) {         \
        aff_sweep_entry<RLO, RHI, MODE, AFF_ROW_FLAGS(MATRIX, LONG, BAND, XDROP, ADAPT, TWO, SUBOPT, ENDB, HITS)>(                          \
            A, gap_open, AFF_SEL_##TWO(gap_open2, 0), AFF_SEL_##TWO(gap2, 0), AFF_SEL_##MATRIX(mat, nullptr), AFF_SEL_##MATRIX(nn, 0u),      \
            AFF_SEL_##BAND(band, 0u), AFF_SEL_##XDROP(xdrop, 0u), AFF_SEL_##ENDB(end_bonus, 0u));                                            \
    }
AFF_SWEEPS(AFF_SWEEP_KERNEL)
// THE LIST OF OVERLAP SWEEPS (option "overlap", MODE 4): a list of its own behind the first, under the same two macros
#define AFF_OVERLAP_SWEEPS(X)                                                                             \
    X(sw_affine_sweep_overlap_kernel,                  1,  4, AFF_OVERLAP, 0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_overlap_wide_kernel,             5, 16, AFF_OVERLAP, 0, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_overlap_matrix_kernel,           1,  4, AFF_OVERLAP, 1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_overlap_matrix_wide_kernel,      5, 16, AFF_OVERLAP, 1, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_overlap_kernel,            16, 16, AFF_OVERLAP, 0, 1, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_long_overlap_matrix_kernel,     16, 16, AFF_OVERLAP, 1, 1, 0, 0, 0, 0, 0, 0, 0)
AFF_OVERLAP_SWEEPS(AFF_SWEEP_KERNEL)
// THE LIST OF PROFILE SWEEPS (swmi_batch_set_read_profiles): the five modes, narrow and wide, with s(i,j) from the
// read's own table.  A list of its own behind the overlap list, under the same two macros; its rows are in a table of their own
// (aff_profile_sweeps), which swmi_launch_affine_profile_sweep searches by shape and mode
#define AFF_PROFILE_SWEEPS(X)                                                                             \
    X(sw_affine_sweep_profile_kernel,                  1,  4, AFF_LOCAL,   2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_profile_wide_kernel,             5, 16, AFF_LOCAL,   2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_fit_profile_kernel,              1,  4, AFF_FIT,     2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_fit_profile_wide_kernel,         5, 16, AFF_FIT,     2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_global_profile_kernel,           1,  4, AFF_GLOBAL,  2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_global_profile_wide_kernel,      5, 16, AFF_GLOBAL,  2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_extend_profile_kernel,           1,  4, AFF_EXTEND,  2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_extend_profile_wide_kernel,      5, 16, AFF_EXTEND,  2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_overlap_profile_kernel,          1,  4, AFF_OVERLAP, 2, 0, 0, 0, 0, 0, 0, 0, 0) \
    X(sw_affine_sweep_overlap_profile_wide_kernel,     5, 16, AFF_OVERLAP, 2, 0, 0, 0, 0, 0, 0, 0, 0)
AFF_PROFILE_SWEEPS(AFF_SWEEP_KERNEL)
#undef AFF_SWEEP_KERNEL

// ------------------------------------------------------------------------------------------------
// traceback
// ------------------------------------------------------------------------------------------------
// LDS of one wavefront: [tile_words] direction tile | [ops_words] ops, 16 per dword | [SWMI_EMIT_SCRATCH_WORDS] string scratch
// LONG: the pairs of the strip sweeps (reads longer than 1024 bases): R = 16, the field of strip sx at sx * swmi_aff_strip_words(n).
// !LONG: one strip -- sx and tsx stay 0 and fold away.
// BAND (with LONG): the fields of the banded strip sweeps (half-width wb): strip sx holds the window of columns from clo =
//   swmi_aff_band_lo(sx) on -- W blocks at swmi_aff_band_strip_off(sx) -- so step t of cell (i, j) is (j - clo) + lane; a step up
//   across the seam changes clo, chi and W along with the strip.  In local mode a cell outside the window reads as H = 0, so an
//   in-band cell may take its diagonal from one (0 + match): the walk that steps onto a column left of clo or right of chi has
//   reached a cell with H = 0 and ends there, as at column 0, without touching the field -- that cell has no code.  (Left of the
//   window the step index would wrap in lane 0 and name an inactive step of the row elsewhere; right of it it may lie past the
//   strip's blocks.)  Fit and global never get there: an outside value loses every max strictly.
// ADAPT (with BAND, the walk of an extend run under option "band_adapt"): clo, chi and W of strip sx come from the
//   centre the sweep left in the pair's window table (an earlier launch on the same stream wrote it), read at the start cell and
//   on every step up across a seam; the strip's field lies at the fixed stride swmi_aff_adapt_strip_words.  A centre is clamped to
//   n, so that a table entry the sweep never wrote (a corrupted list that names a strip behind an xdrop stop) still gives a window
//   of at most the stride's blocks and the guard w < W keeps the walk inside the pair's field.
// TWO (the walk of a two-piece run, global mode's): a block is 2 R 64 dwords, plane 0 then plane 1, so a tile of
//   consecutive blocks holds both; a strip's field is twice as long.  Five states: H, M, and per piece F and E (AFF_INS / AFF_DEL are
//   piece 1's, AFF_INS2 / AFF_DEL2 piece 2's).  State H reads the direction from plane 0; an insertion enters F2 iff pF (plane 1,
//   bit 1), a deletion E2 iff pE (bit 0); a gap state stays while its own x bit is set -- plane 0 bits 2, 3 for piece 1, plane 1
//   bits 2, 3 for piece 2.  Plane 1 is read only on entering a gap state or in a piece-2 state.  A step up across a seam in
//   state F2 continues in the strip above like any other.
#define AFF_INS2 4u
#define AFF_DEL2 5u
namespace {
// The walks that may exist: modes 0 .. 2 (an extend run is walked by global mode's kernels, so the walk of option "band_adapt" is
// held against the extend sweeps' rule) and 4 (overlap), and the four flags that shape a field
constexpr bool aff_traceback_ok(uint32_t mode, uint32_t f) {
    return (mode <= AFF_GLOBAL || mode == AFF_OVERLAP) && !(f & ~(AFF_F_LONG | AFF_F_BAND | AFF_F_ADAPT | AFF_F_TWO)) &&
           aff_flags_ok((f & AFF_F_ADAPT) && mode == AFF_GLOBAL ? AFF_EXTEND : mode, f);
}
template <int MODE, uint32_t F>
__device__ __forceinline__ void aff_traceback(const TraceArgs A, const uint32_t tile_words, const uint32_t ops_words, const uint32_t cigar,
                                              const uint32_t wb) {
    static_assert(aff_traceback_ok(MODE, F), "no such walk");
    AFF_FLAG_NAMES(F)
    constexpr uint32_t PL = TWO ? 2u : 1u;                        // planes of the field
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = blockIdx.y, nslots = gridDim.y;
    const PairDesc pd = A.pairs[blockIdx.x];
    const PairOut po = A.out[pd.out_id];
    if (A.out_host && slot == 0 && lane == 0) A.out_host[pd.out_id] = po;      // result straight into pinned host memory
    if (po.flags & (SWMI_F_DEGENERATE | SWMI_F_CELL_OVF)) return;
    if (po.n_cells <= slot) return;
    uint32_t *tile = lds;
    uint32_t *ops = lds + tile_words;
    uint32_t *scratch = ops + ops_words;
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t R = LONG ? SWMI_AFF_RMAX : uni(swmi_aff_rows_per_lane(m));
    uint32_t W = uni(LONG ? swmi_aff_strip_blocks(n) : swmi_aff_blocks(m, n));      // (BAND: of strip sx, set with it)
    uint32_t clo = 1u, chi = n;                                   // first and last column of strip sx's window
    const uint32_t blk_words = PL * R * WAVE;                     // dwords of one 8-step block
    const uint32_t NB = tile_words / blk_words;                   // blocks per tile (>= 1: the host sizes the tile)
    const uint32_t max_ops = ops_words * 16u;
    const uint32_t *__restrict__ dir = A.dir + pd.dir_off;
    const uint8_t *__restrict__ raw_ref = A.raw ? A.raw + A.raw_off[pd.ref_id] : nullptr;
    const uint8_t *__restrict__ raw_read = A.raw ? A.raw + A.raw_off[A.raw_reads_at + pd.read_id] : nullptr;
    const uint64_t cbase = A.cells_off ? A.cells_off[pd.out_id] : (uint64_t)pd.out_id * A.cell_cap;
    const uint2 *__restrict__ cells = A.cells + cbase;
    const uint32_t ncell = (uint32_t)po.n_cells;
    uint32_t wlo = 0xFFFFFFFFu, whi = 0u;                         // blocks [wlo, whi) are in the tile
    uint32_t tsx = LONG ? 0xFFFFFFFFu : 0u;                       // ... of this strip
    const uint32_t NS = LONG ? uni(swmi_aff_strips(m)) : 1u;
    const uint64_t astride = ADAPT ? swmi_aff_adapt_strip_words(n, wb) : 0ull;     // ADAPT: dwords of every strip's field
    const uint32_t *const wtab = ADAPT ? dir + (uint64_t)NS * astride : nullptr;    // ADAPT: the pair's window table
// AFF_ADAPT_WINDOW: clo, chi and W of strip sx from the table (text, as the sweeps' shared pieces are: the static walks stay as they
// were).  Only for sx < NS: the step up from row 1 leaves strip 0 for "strip" 0xFFFFFFFF -- the walk ends there, at row 0, and the
// closed forms of the static band are harmless for it, but the table has no such entry to load
#define AFF_ADAPT_WINDOW                                                                                                       \
    {                                                                                                                          \
        if (sx < NS) {                                                                                                         \
            const uint32_t tc = uni(wtab[sx]), cen = tc < n ? tc : n;                                                          \
            clo = swmi_aff_adapt_lo(cen, wb); chi = swmi_aff_adapt_hi(cen, n, wb); W = swmi_aff_strip_blocks(chi - clo + 1u);  \
        }                                                                                                                      \
    }

    for (uint32_t c = slot; c < ncell; c += nslots) {
        const uint32_t ci = uni(cells[c].x), cj = uni(cells[c].y);
        uint32_t i = ci, j = cj;
        uint32_t l = (i - 1u) / R, k = (i - 1u) - l * R;          // (global) lane and row slot of row i
        uint32_t sx = 0u;                                         // its strip, and the lane within it
        if constexpr (LONG) { sx = l / WAVE; l -= sx * WAVE; }
        if constexpr (BAND) {
            if (sx >= NS) sx = NS;                                // (a corrupted list: refused below, and no window is computed for it)
            else if constexpr (ADAPT) AFF_ADAPT_WINDOW
            else { clo = swmi_aff_band_lo(sx, wb); chi = swmi_aff_band_hi(sx, n, wb); W = swmi_aff_band_blocks(sx, n, wb); }
        }
        uint32_t st = 0u;                                         // 0: H, else the state entered (AFF_DIAG / AFF_INS / AFF_DEL)
        uint32_t n_ops = 0, cur = 0;
        int begin = MODE == AFF_LOCAL ? 0 : (int)cj;
        bool ok = true;
        // (AFF_OVERLAP: the walk ends at the first cell of row 0 or column 0 -- local's condition -- with fit's codes and `begin`)
        while (MODE == AFF_LOCAL || MODE == AFF_OVERLAP ? (i != 0u && j != 0u) : (i != 0u)) {
            if (MODE != AFF_LOCAL && MODE != AFF_OVERLAP && j == 0u) {      // the read's head hangs over the reference start: inserted,
                if (n_ops >= max_ops) { ok = false; break; }      // and the field is not touched
                --i;
                cur |= SWMI_DIR_I << (2u * (n_ops & 15u));
                ++n_ops;
                if ((n_ops & 15u) == 0u) { if (lane == 0) ops[(n_ops >> 4) - 1u] = cur; cur = 0u; }
                continue;
            }
            if constexpr (BAND && MODE == AFF_LOCAL) {
                // outside the strip's window: H = 0, the walk ends (only ever reached in state H, by a diagonal step)
                if (sx < NS && (j < clo || j > chi)) { ok = st == 0u; break; }
            }
            const uint32_t t = j - (BAND ? clo : 1u) + l, w = t >> 3;      // (BAND: clo <= j here, or the list is corrupted and w >= W refuses it)
            if (w < wlo || w >= whi || (LONG && sx != tsx)) {     // stage the tile that ends at this block
                if (w >= W || (LONG && sx >= NS)) { ok = false; break; }    // (a corrupted list: never walks off the field)
                WAVE_SYNC();
                wlo = w + 1u >= NB ? w + 1u - NB : 0u;
                whi = w + 1u;
                if constexpr (LONG) tsx = sx;
                const uint32_t *__restrict__ src = dir + (ADAPT ? (uint64_t)sx * astride : BAND ? PL * swmi_aff_band_strip_off(sx, n, wb) : LONG ? (uint64_t)sx * PL * swmi_aff_strip_words(n) : 0ull) +
                                                   (uint64_t)wlo * blk_words;
                const uint32_t words = (whi - wlo) * blk_words;
                for (uint32_t x = lane; x < words; x += WAVE) tile[x] = src[x];
                WAVE_SYNC();
            }
            uint32_t code = uni((tile[((w - wlo) * PL * R + k) * WAVE + l] >> (4u * (t & 7u))) & 15u);
            if (st == 0u) {
                st = code & 3u;
                if (MODE == AFF_LOCAL) { if (st == AFF_STOP) break; }   // H(i, j) == 0: `while (score > 0)` (SmithWaterman.java:380)
                else if (st == AFF_STOP) { ok = false; break; }         // (these sweeps write no code 0: a corrupted field)
                if constexpr (TWO) {
                    if (st != AFF_DIAG) {                               // entering a gap state: which piece (plane 1: pE bit 0, pF bit 1)
                        const uint32_t c2 = uni((tile[(((w - wlo) * PL + 1u) * R + k) * WAVE + l] >> (4u * (t & 7u))) & 15u);
                        if (st == AFF_INS && (c2 & 2u)) { st = AFF_INS2; code = c2; }
                        else if (st == AFF_DEL && (c2 & 1u)) { st = AFF_DEL2; code = c2; }
                    }
                }
            } else if constexpr (TWO) {
                // in a piece-2 state: its x bits are plane 1's
                if (st >= AFF_INS2) code = uni((tile[(((w - wlo) * PL + 1u) * R + k) * WAVE + l] >> (4u * (t & 7u))) & 15u);
            }
            if (n_ops >= max_ops) { ok = false; break; }
            if (MODE == AFF_LOCAL || (st != AFF_INS && (!TWO || st != AFF_INS2))) begin = (int)j;     // (end-to-end: the moves that consume a reference base)
            uint32_t op;
            if (st == AFF_DIAG) {
                op = SWMI_DIR_A;
                st = 0u;
                --i; --j;
            } else if (st == AFF_INS) {
                op = SWMI_DIR_I;
                st = (code & 8u) ? AFF_INS : 0u;
                --i;
            } else if (TWO && st == AFF_INS2) {
                op = SWMI_DIR_I;
                st = (code & 8u) ? AFF_INS2 : 0u;
                --i;
            } else if (TWO && st == AFF_DEL2) {
                op = SWMI_DIR_D;
                st = (code & 4u) ? AFF_DEL2 : 0u;
                --j;
            } else {
                op = SWMI_DIR_D;
                st = (code & 4u) ? AFF_DEL : 0u;
                --j;
            }
            if (op != SWMI_DIR_D) {
                if (k != 0u) --k;
                else if (!LONG || l != 0u) { k = R - 1u; --l; }
                else {                                            // up from a strip's first row: the last row of the strip above
                    k = R - 1u; l = WAVE - 1u; --sx;
                    if constexpr (ADAPT) AFF_ADAPT_WINDOW
                    else if constexpr (BAND) { clo = swmi_aff_band_lo(sx, wb); chi = swmi_aff_band_hi(sx, n, wb); W = swmi_aff_band_blocks(sx, n, wb); }
                }
            }
            cur |= op << (2u * (n_ops & 15u));
            ++n_ops;
            if ((n_ops & 15u) == 0u) { if (lane == 0) ops[(n_ops >> 4) - 1u] = cur; cur = 0u; }
        }
        if (MODE == AFF_GLOBAL) {                                 // row 0: the rest of the reference is deleted
            while (ok && j != 0u) {
                if (n_ops >= max_ops) { ok = false; break; }
                begin = (int)j;
                --j;
                cur |= SWMI_DIR_D << (2u * (n_ops & 15u));
                ++n_ops;
                if ((n_ops & 15u) == 0u) { if (lane == 0) ops[(n_ops >> 4) - 1u] = cur; cur = 0u; }
            }
        }
        if ((n_ops & 15u) != 0u && lane == 0) ops[n_ops >> 4] = cur;
        WAVE_SYNC();
        // the payload: both strings, the packed ops or -- option "cigar", wave-uniform -- the CIGAR, sized by a pass of its own (swmi_emit.h)
        const bool strings = A.raw != nullptr;
        SwmiCigar<SwmiOpsPacked> cg(SwmiOpsPacked{ops}, n_ops, ci, cj, reinterpret_cast<const uint8_t *>(A.seqw + rd.boff),
                                    reinterpret_cast<const uint8_t *>(A.seqw + qd.boff), cigar, lane);
        if (cigar && ok) cg.count();
        const uint32_t words = cigar ? cg.words() : swmi_payload_words(n_ops, strings);
        unsigned long long off;
        uint32_t rslot;
        if (ok && swmi_reserve(A, lane, words, 1u, off, rslot)) {
            uint32_t *dst = A.arena + off;
            if (lane == 0) swmi_write_rec(A, rslot, pd.out_id, SWMI_RANK_BY_CELL, begin, ci, cj, n_ops, off);
            if (cigar) swmi_emit_cigar(dst, cg);
            else if (strings) swmi_emit_strings(dst, SwmiOpsPacked{ops}, n_ops, ci, cj, raw_ref, raw_read, lane, scratch);
            else for (uint32_t x = lane; x < words; x += WAVE) dst[x] = ops[x];
        } else if (lane == 0) {
            atomicOr(&A.out[pd.out_id].flags, SWMI_F_ARENA_OVF);
            if (A.ovf_host) *A.ovf_host = 1u;
        }
        WAVE_SYNC();
    }
}
#undef AFF_ADAPT_WINDOW
}  // namespace
#undef AFF_INS2
#undef AFF_DEL2

// THE LIST OF TRACEBACKS.  One row per kernel: its name, its MODE and the four flags a walk has.  The banded walks take the
// half-width as one more argument, the last.  cigar: the payload kind (0: strings or packed ops, as TraceArgs.raw says; 1, 2: option
// "cigar") -- a runtime value, one kernel for all
//                                                   MODE      LONG BAND ADAPT TWO
#define AFF_TRACEBACKS(X)                                                     \
    X(sw_affine_traceback_kernel,                   AFF_LOCAL,  0, 0, 0, 0) \
    X(sw_affine_traceback_fit_kernel,               AFF_FIT,    0, 0, 0, 0) \
    X(sw_affine_traceback_global_kernel,            AFF_GLOBAL, 0, 0, 0, 0) \
    X(sw_affine_traceback_long_kernel,              AFF_LOCAL,  1, 0, 0, 0) \
    X(sw_affine_traceback_long_fit_kernel,          AFF_FIT,    1, 0, 0, 0) \
    X(sw_affine_traceback_long_global_kernel,       AFF_GLOBAL, 1, 0, 0, 0) \
    X(sw_affine_traceback_band_kernel,              AFF_LOCAL,  1, 1, 0, 0) \
    X(sw_affine_traceback_band_fit_kernel,          AFF_FIT,    1, 1, 0, 0) \
    X(sw_affine_traceback_band_global_kernel,       AFF_GLOBAL, 1, 1, 0, 0) \
    X(sw_affine_traceback_band_adapt_global_kernel, AFF_GLOBAL, 1, 1, 1, 0) \
    X(sw_affine_traceback2_global_kernel,           AFF_GLOBAL, 0, 0, 0, 1) \
    X(sw_affine_traceback2_long_global_kernel,      AFF_GLOBAL, 1, 0, 0, 1) \
    X(sw_affine_traceback2_band_global_kernel,      AFF_GLOBAL, 1, 1, 0, 1)
#define AFF_TB_FLAGS(LONG, BAND, ADAPT, TWO) aff_flags(0, LONG, BAND, 0, ADAPT, TWO, 0, 0, 0)
#define AFF_TRACEBACK_KERNEL(name, MODE, LONG, BAND, ADAPT, TWO)                                                                     \
    static_assert(aff_traceback_ok(MODE, AFF_TB_FLAGS(LONG, BAND, ADAPT, TWO)), #name);                                             \
    extern "C" __global__ void __launch_bounds__(WAVE) name(const TraceArgs A, const uint32_t tile_words, const uint32_t ops_words, \
                                                            const uint32_t cigar AFF_IF_##BAND(, const uint32_t band)) {            \
        aff_traceback<MODE, AFF_TB_FLAGS(LONG, BAND, ADAPT, TWO)>(A, tile_words, ops_words, cigar, AFF_SEL_##BAND(band, 0u));       \
    }
AFF_TRACEBACKS(AFF_TRACEBACK_KERNEL)
// THE LIST OF OVERLAP TRACEBACKS (option "overlap", MODE 4), behind the first as the sweeps' is
#define AFF_OVERLAP_TRACEBACKS(X)                                              \
    X(sw_affine_traceback_overlap_kernel,           AFF_OVERLAP, 0, 0, 0, 0) \
    X(sw_affine_traceback_long_overlap_kernel,      AFF_OVERLAP, 1, 0, 0, 0)
AFF_OVERLAP_TRACEBACKS(AFF_TRACEBACK_KERNEL)
#undef AFF_TRACEBACK_KERNEL

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------
// Both take the run's options as one AffRun and refuse what aff_run_ok refuses (swmi_launch.h, which describes the arguments).
// Each has ONE table, the list above under a macro: a row is the kernel's key (aff_key of its shape, mode and flags), a launch
// stub and the kernel's name.  The stub is a captureless lambda that launches its own kernel with the pieces of AffRun the
// kernel's flags ask for, so every launch is checked against its kernel's parameter list, whatever the signature.  A run's key is
// searched for; no row, no kernel: hipErrorInvalidValue.
static_assert(AFF_EXTEND == 3, "AffRun.mode 3 is the extend run");
static_assert(AFF_OVERLAP == 4, "AffRun.mode 4 is the overlap run");
namespace {
struct AffSweepRow {
    uint32_t key;
    void (*launch)(const FillArgs &a, const AffRun &r, dim3 grid, uint32_t waves, size_t lds, hipStream_t st);
    const char *name;
    const void *kernel;          // for swmi_allow_big_lds (the profile sweeps)
};
// (waves, lds: the wavefronts of a workgroup and its dynamic LDS -- AFF_WAVES and none but for the profile sweeps; the key of a
// profile row is that of the plain sweep of its shape and mode: AFF_F_PROFILE is no part of a key, and the row is in its own table)
#define AFF_SWEEP_ROW(name, RLO, RHI, MODE, MATRIX, LONG, BAND, XDROP, ADAPT, TWO, SUBOPT, ENDB, HITS)                               \
    {aff_key(LONG ? 2u : RLO == 1 ? 0u : 1u, MODE, aff_flags((MATRIX) == 1, LONG, BAND, XDROP, ADAPT, TWO, SUBOPT, ENDB, HITS)),     \
     [](const FillArgs &a, const AffRun &r, dim3 grid, uint32_t waves, size_t lds, hipStream_t st) {                                 \
         hipLaunchKernelGGL(name, grid, dim3(WAVE * waves), lds, st, a, (int)r.gap_open AFF_IF_##TWO(, (int)r.gap_open2, (int)r.gap2) \
                            AFF_IF_##MATRIX(, r.mat, r.nn) AFF_IF_##BAND(, r.band) AFF_IF_##XDROP(, r.xdrop) AFF_IF_##ENDB(, r.end_bonus)); \
     }, #name, reinterpret_cast<const void *>(name)},
const AffSweepRow aff_sweeps[] = {AFF_SWEEPS(AFF_SWEEP_ROW) AFF_OVERLAP_SWEEPS(AFF_SWEEP_ROW)};
const AffSweepRow aff_profile_sweeps[] = {AFF_PROFILE_SWEEPS(AFF_SWEEP_ROW)};
#undef AFF_SWEEP_ROW

struct AffTracebackRow {
    uint32_t key;
    void (*launch)(const TraceArgs &a, const AffRun &r, uint32_t tile_words, uint32_t ops_words, hipStream_t st);
    const char *name;
    const void *kernel;          // for swmi_allow_big_lds
};
#define AFF_TRACEBACK_ROW(name, MODE, LONG, BAND, ADAPT, TWO)                                                                        \
    {aff_key(0u, MODE, AFF_TB_FLAGS(LONG, BAND, ADAPT, TWO)),                                                                        \
     [](const TraceArgs &a, const AffRun &r, uint32_t tile_words, uint32_t ops_words, hipStream_t st) {                              \
         const size_t lds = ((size_t)tile_words + ops_words + SWMI_EMIT_SCRATCH_WORDS) * sizeof(uint32_t);                           \
         hipLaunchKernelGGL(name, dim3(a.n_pairs, SWMI_AFF_TB_SLOTS), dim3(WAVE), lds, st, a, tile_words, ops_words, r.cigar         \
                            AFF_IF_##BAND(, r.band));                                                                                \
     }, #name, reinterpret_cast<const void *>(name)},
const AffTracebackRow aff_tracebacks[] = {AFF_TRACEBACKS(AFF_TRACEBACK_ROW) AFF_OVERLAP_TRACEBACKS(AFF_TRACEBACK_ROW)};
#undef AFF_TRACEBACK_ROW

// The rows of a run's kernels, null where the launchers refuse.  shape: 0 narrow, 1 wide, 2 long.
const AffSweepRow *aff_sweep_row(const AffRun &r, uint32_t long_reads, uint32_t shape) {
    if (!aff_run_ok(r, long_reads)) return nullptr;
    const uint32_t key = aff_key(shape, r.mode, aff_run_flags(r, long_reads));
    for (const AffSweepRow &row : aff_sweeps) if (row.key == key) return &row;
    return nullptr;
}
// The profile sweep of a run whose batch has profiles: the plain one-piece run of a short shape in any of the five
// modes -- no score matrix, none of gap_open2, subopt, hits and end_bonus.  band, xdrop and band_adapt are the long shape's and do
// not count here, as for every short sweep.
const AffSweepRow *aff_profile_sweep_row(const AffRun &r, uint32_t shape) {
    if (!aff_run_ok(r, 0u) || shape > 1u) return nullptr;
    if (r.mat || r.gap_open2 || r.subopt || r.hits || r.end_bonus) return nullptr;
    const uint32_t key = aff_key(shape, r.mode, 0u);
    for (const AffSweepRow &row : aff_profile_sweeps) if (row.key == key) return &row;
    return nullptr;
}
const AffTracebackRow *aff_traceback_row(const AffRun &r, uint32_t long_reads) {
    if (!aff_run_ok(r, long_reads)) return nullptr;
    // an extend run is walked by global mode's kernels: aff_traceback<AFF_GLOBAL, ..> starts at whatever cell the list names and
    // makes no use of its being (m, n)
    const uint32_t mode = r.mode == AFF_EXTEND ? AFF_GLOBAL : r.mode;
    const uint32_t key = aff_key(0u, mode, aff_run_flags(r, long_reads) & (AFF_F_LONG | AFF_F_BAND | AFF_F_ADAPT | AFF_F_TWO));
    for (const AffTracebackRow &row : aff_tracebacks) if (row.key == key) return &row;
    return nullptr;
}
}  // namespace

extern "C" int swmi_affine_run_ok(const AffRun *r, uint32_t long_reads) { return aff_run_ok(*r, long_reads) ? 1 : 0; }
extern "C" const char *swmi_affine_sweep_name(const AffRun *r, uint32_t long_reads, uint32_t shape) {
    const AffSweepRow *row = aff_sweep_row(*r, long_reads, shape);
    return row ? row->name : nullptr;
}
extern "C" const char *swmi_affine_traceback_name(const AffRun *r, uint32_t long_reads) {
    const AffTracebackRow *row = aff_traceback_row(*r, long_reads);
    return row ? row->name : nullptr;
}

extern "C" hipError_t swmi_launch_affine_sweep(const FillArgs *a, const AffRun *r, uint32_t long_reads, uint32_t r_min, uint32_t r_max,
                                               hipStream_t st) {
    if (a->n_pairs == 0) return hipSuccess;
    const dim3 grid((a->n_pairs + AFF_WAVES - 1) / AFF_WAVES);
    const auto sweep = [&](uint32_t shape) {
        const AffSweepRow *row = aff_sweep_row(*r, long_reads, shape);
        if (row) row->launch(*a, *r, grid, AFF_WAVES, 0, st);
        return row != nullptr;
    };
    // the short shape: the narrow and the wide sweep, each only if the launch has pairs for it
    const bool ok = long_reads ? sweep(2u) : (r_min > 4u || sweep(0u)) && (r_max < 5u || sweep(1u));
    return ok ? hipGetLastError() : hipErrorInvalidValue;      // (a launch's own error is what hipGetLastError returns)
}

extern "C" const char *swmi_affine_profile_sweep_name(const AffRun *r, uint32_t shape) {
    const AffSweepRow *row = aff_profile_sweep_row(*r, shape);
    return row ? row->name : nullptr;
}

// A wavefront's table has `rows` rows of n + 1 dwords, rows = 64 * the rows per lane of the longest read the kernel takes in this
// launch (the narrow sweep: at most 4); a workgroup gets as many wavefronts, at most AFF_WAVES, as tables fit the LDS beside the
// 1 KiB of keys.  One table must fit: rows * (n + 1) <= SWMI_PROF_LDS_WORDS, which check_run_params (swmi_run.cpp) has made sure of.
namespace {
// the dwords of one wavefront's table in a launch of that shape whose longest read has r_max rows per lane
inline uint32_t aff_profile_tab_words(uint32_t n, uint32_t r_max, uint32_t shape) {
    return WAVE * (shape == 0u ? std::min(r_max, 4u) : r_max) * (n + 1u);
}
}  // namespace
extern "C" uint32_t swmi_affine_profile_waves(uint32_t n, uint32_t r_max, uint32_t shape) {
    if (n < 1u || n > SWMI_MAT_MAX_SYMBOLS || r_max < 1u || r_max > SWMI_AFF_RMAX || shape > 1u) return 0u;
    const uint32_t tab_words = aff_profile_tab_words(n, r_max, shape);
    if (tab_words > SWMI_PROF_LDS_WORDS) return 0u;
    return std::min<uint32_t>(AFF_WAVES, (SWMI_LDS_BYTES - 4u * SWMI_PROF_KEY_WORDS) / (4u * tab_words));
}

extern "C" hipError_t swmi_launch_affine_profile_sweep(const FillArgs *a, const AffRun *r, const AffProfile *p, uint32_t r_min, uint32_t r_max,
                                                       hipStream_t st) {
    if (a->n_pairs == 0) return hipSuccess;
    if (!p || !p->image || p->n < 1u || p->n > SWMI_MAT_MAX_SYMBOLS || r_max < 1u || r_max > SWMI_AFF_RMAX) return hipErrorInvalidValue;
    // (the dynamic LDS a profile sweep may ask for: the CU's less the kernel's own static 1 KiB of keys -- swmi_allow_big_lds asks
    // for all of it, which a kernel with static LDS is refused)
    static const hipError_t attrs = [] {
        hipError_t e = hipSuccess;
        for (const AffSweepRow &s : aff_profile_sweeps) {
            const hipError_t x = hipFuncSetAttribute(s.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SWMI_LDS_BYTES - 4u * SWMI_PROF_KEY_WORDS));
            if (x != hipSuccess) e = x;
        }
        return e;
    }();
    if (attrs != hipSuccess) return attrs;
    const uint32_t nn = p->n + 1u;
    const auto sweep = [&](uint32_t shape) {
        const AffSweepRow *row = aff_profile_sweep_row(*r, shape);
        const uint32_t tab_words = aff_profile_tab_words(p->n, r_max, shape), rows = tab_words / nn;
        const uint32_t waves = swmi_affine_profile_waves(p->n, r_max, shape);       // (0: the table does not fit)
        if (!row || !waves) return false;
        AffRun pr = *r;
        pr.mat = p->image;
        pr.nn = nn | rows << 16;
        row->launch(*a, pr, dim3((a->n_pairs + waves - 1u) / waves), waves, (size_t)waves * tab_words * 4u, st);
        return true;
    };
    const bool ok = (r_min > 4u || sweep(0u)) && (r_max < 5u || sweep(1u));
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

extern "C" hipError_t swmi_launch_affine_traceback(const TraceArgs *a, const AffRun *r, uint32_t long_reads, uint32_t tile_words,
                                                   uint32_t ops_words, hipStream_t st) {
    if (a->n_pairs == 0) return hipSuccess;
    const AffTracebackRow *row = aff_traceback_row(*r, long_reads);
    if (!row) return hipErrorInvalidValue;
    // (the fields of the two-piece sweeps: the tile holds at least one block of 2 * R * 64 dwords)
    if (r->gap_open2 && tile_words < 2u * SWMI_AFF_RMAX * WAVE) return hipErrorInvalidValue;
    static const bool attrs = [] {
        for (const AffTracebackRow &t : aff_tracebacks) swmi_allow_big_lds(t.kernel);
        return true;
    }();
    (void)attrs;
    row->launch(*a, *r, tile_words, ops_words, st);
    return hipGetLastError();
}
