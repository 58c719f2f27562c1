// swmi_device.h -- structures shared by the host runtime (swmi_host.h and its units) and the gfx950 kernels
// (the swmi_*.hip units).  HBM data layout of one batch:
//
//   seqw   uint32[]   every sequence as a BYTE image: 1 canonical code per base, 4 per dword, image start
//                     16-byte aligned.  Codes: the eight fast symbols A,C,G,T,N,U,R,Y (any case) -> 0,4,...,28 --
//                     the bit offset of the symbol's entry in a row's 8 x int4 score profile: the sweep turns a
//                     code into the one-hot word 1 << code with one SDWA shift and looks the score up with
//                     v_dot8_i32_i4 -- every other (upper-cased) byte value -> a distinct code outside that set.
//                     Each image is followed by SWMI_SEQ_PAD_WORDS zero dwords so a 16-step block may
//                     over-read past the end.
//   refs / reads      SeqDesc per sequence.
//   pairs  PairDesc[] one per (ref, read) pair of the launch (any order; the host sorts by work).
//   dir    uint32[]   direction field, 2 bits per DP cell.  For one pair and one strip of 64*R
//                     read rows it is laid out [w][k][lane]: dword ((w*R + k)*64 + lane) holds the
//                     16 anti-diagonal steps t = 16w .. 16w+15 of row i = strip*64R + lane*R + k + 1,
//                     step t at bits 2*(15 - t%16) (+1), where lane `lane` is at column j = t - lane + 1.
//                     Code: bit0 = alignment chosen, else bit1 = insertion chosen, else deletion.
//                     Every store instruction therefore writes 256 contiguous bytes.
//   cells  uint2[]    per pair, up to cell_cap (i, j) coordinates of the tied maximum cells.
//   out    PairOut[]  per pair score / count / flags.
//   rec_tab AlnRec[]  one entry per alignment, in the order the traceback kernels reserved them;
//   arena  uint32[]   the alignments' variable-length payloads (the two aligned strings, or the packed ops).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SWMI_HD __host__ __device__
#else
#define SWMI_HD
#endif

#define SWMI_SEQ_PAD_WORDS 24u
#define SWMI_RMAX          4          // rows per lane in the widest kernel variant
#ifndef SWMI_CK_BLOCKS
#define SWMI_CK_BLOCKS     2u         // mode 1: a lane-state checkpoint every 2 blocks = 32 anti-diagonal steps
#endif                                 // (-DSWMI_CK_BLOCKS=4u builds the 64-step variant measured in profiles/r02/ck_blocks.md)
#define SWMI_CODE_PAD      0x1FFu     // never equals a base code (codes are 0..255)

// LDS layout constants the host dimensions launches by
#define SWMI_LDS_BYTES (160u * 1024u)     // LDS of a CU = the most one workgroup may ask for
#define SWMI_EMIT_SCRATCH_WORDS 128u      // LDS dwords emit_strings needs: 256 characters of each string
#define SWMI_TB_BLOCKS 16u
#define SWMI_TB_REFWIN_WORDS 96u      // (16*16 + 63) / 4 + slack
#define SWMI_RES_CELL_CAP 128u            // maximum cells a resident pair lists in LDS (sw_resident_pairs_kernel)

// op codes of an alignment record (2 bits per traceback step)
#define SWMI_DIR_D 0u
#define SWMI_DIR_I 1u
#define SWMI_DIR_A 2u

// PairOut.flags
#define SWMI_F_DEGENERATE   0x1u   // max score 0: all m*n cells tie (no alignment records emitted)
#define SWMI_F_CELL_OVF     0x2u   // more tied max cells than cell_cap: host re-runs the pair
#define SWMI_F_ARENA_OVF    0x4u   // a record of this pair did not fit the arena: host grows it, re-runs
#define SWMI_F_DONE         0x8u   // the pair was handled whole by sw_resident_pairs_kernel: the traceback kernels leave it alone
#define SWMI_F_TO_END       0x10u  // option "end_bonus": the pair was taken to the read's end -- its score is end_score, its one cell (m, end_col)
// bits 8-31: the strips swept of a pair whose strip sweep option "xdrop" stopped (>= 1; a read has at most 2^22 strips), 0 for every
// other pair.  Not a flag: no kernel tests it, the traceback kernels copy it to the host with the word, and the host turns it
// into swmi_pair_rows_swept
#define SWMI_F_STRIPS_SHIFT 8u
#define SWMI_F_STRIPS_MASK  0xFFFFFF00u

struct SeqDesc {
    uint32_t len;     // bases
    uint32_t boff;    // dword offset of the byte image in seqw (multiple of 4)
    uint32_t acgt;    // 1 if every base is one of the eight fast symbols (codes 0,4,...,28)
    uint32_t pad;
};

struct PairDesc {
    uint32_t ref_id;
    uint32_t read_id;
    uint32_t out_id;      // index into out[] / cells[] (the pair's position in the batch)
    uint32_t pad;         // flags below (mode 1)
    uint64_t dir_off;     // dword offset of this pair's direction field in dir[]
    uint64_t seam_off;    // dword offset of the strip-seam rows, n+1 int32 per strip (multi-strip pairs only)
};

// PairDesc.pad of a single-strip pair whose sweep is split into column chunks (mode 1): this flag + the number of chunks
#define SWMI_PAD_COLS 0x80000000u
// PairDesc.pad of a pair handled start to finish by sw_resident_pairs_kernel (mode 1, small pairs): every other kernel skips it
#define SWMI_PAD_RESIDENT 0x40000000u

// One column chunk of a pair's mode-1 sweep (sw_sweep_winmax_cols_kernel): the wavefront starts a fresh sweep at
// reference column col0 + 1 (col0 a multiple of 32) -- far enough to the left that every cell from checkpoint window
// g_lo on is exact, because a positive-score path cannot span more columns than that -- and owns the checkpoint
// windows g_lo .. g_hi-1: it writes exactly the checkpoints and window maxima a one-wavefront sweep would have written.
struct ColItem {
    uint32_t pair;        // index into FillArgs.pairs
    uint32_t col0;
    uint32_t g_lo, g_hi;
};

// One wavefront of the strip pipeline (sw_sweep_winmax_strips_kernel): strip `strip` of pair `pair`, for the whole reference
// (col0 = 0, g_lo = 0, g_hi >= the strip's windows) or for ONE COLUMN CHUNK of it -- ColItem's rule holds for every strip as
// long as the seam rows of the halo are swept too: all strips of a chunk start at column col0 + 1 from a zero state, the
// chunk owns the checkpoint windows g_lo .. g_hi-1 of every strip, and strip s runs 64 steps further than strip s+1 (whose
// lane 0 needs the seam that far).  A chunk keeps PRIVATE seam rows for its own strips (its halo values are not exact) and
// writes the columns it owns into the pair's shared seam rows, which the traceback's replay reads.
struct StripItem {
    uint32_t pair, strip;
    uint32_t col0, g_lo, g_hi;
    uint32_t prog;          // index of the first progress slot of this (pair, chunk): + strip
    uint32_t priv_stride;   // dwords per private seam row (0: not chunked, the strips hand over through the shared rows)
    uint32_t pad;
    uint64_t priv_off;      // dword offset of the chunk's private seam rows in seam[]: row s at priv_off + s * priv_stride
};

struct PairOut {
    int32_t  score;
    uint32_t flags;
    uint64_t n_cells;     // number of tied maximum cells (m*n when degenerate)
};

// Option "end_bonus" (DESIGN.md 8o): what the extend sweeps of such a run leave per pair, by out_id, in the result block behind the
// pair outputs -- swmi.h's max_score, end_score and end_col
struct EndOut {
    int32_t  max_score;   // the maximum of H over every existing cell: the score of the run without the option
    int32_t  end_score;   // the maximum of H(m, j) over the existing cells of read row m
    uint32_t end_col;     // the smallest (1-based) column that holds it
};

// One alignment = one entry of the RECORD TABLE (dense, 8 dwords each, in the order the records were reserved) + its payload
// in the arena.  With TraceArgs.raw set: the two aligned strings GetAlignment returns (SmithWaterman.java:418-431), refAligned
// then readAligned, n_ops/4 + 1 dwords each (NUL-terminated, NUL-padded).  Otherwise: ceil(n_ops/16) dwords of 2-bit ops (op t
// of the traceback, first = the max cell, at bits 2*(t%16) of dword t/16), from which the host builds the strings on demand.  The table is what the host indexes: a
// dense array reads at memory bandwidth, where headers scattered through the arena were one dependent cache miss per record
// (0.11 ms per 1161 records of a pinned block the GPU had just written).
struct AlnRec {
    uint32_t out_id;
    uint32_t rank;        // position of the alignment in OptAlignments order
    int32_t  begin;       // GetAlignment's `beginning` (SmithWaterman.java:378-383)
    int32_t  end_i, end_j;
    uint32_t n_ops;
    uint32_t off_lo, off_hi;   // dword offset of the payload in the arena
};
#define SWMI_RECTAB_WORDS 8u

// ONE 64-bit counter reserves both an alignment's payload and its table entry: the low 36 bits count arena dwords (they may
// exceed the capacity: what does not fit is dropped and the host re-runs with the size the counter then shows), the high 28
// bits count records.  One atomic per alignment instead of two: device-scope atomics of every XCD on one line queue up, and
// two per record made the traceback launch 10 us longer (profiles/r03/ab_one_atomic.txt).
struct ArenaHdr {
    unsigned long long reserved;     // n_records << 36 | used_words
    unsigned long long pad;
};
#define SWMI_HDR_WORD_BITS 36u
#define SWMI_HDR_WORD_MASK ((1ull << SWMI_HDR_WORD_BITS) - 1ull)

struct FillArgs {
    const uint32_t *seqw;
    const SeqDesc  *refs;
    const SeqDesc  *reads;
    const PairDesc *pairs;
    uint32_t       *dir;
    int32_t        *seam;
    PairOut        *out;
    uint2          *cells;
    const uint64_t *cells_off;   // per out_id offset into cells[] (null: out_id * cell_cap)
    const uint32_t *cells_cap;   // per out_id capacity        (null: cell_cap)
    ArenaHdr       *hdr;         // zeroed by the fill kernel for the traceback kernel that follows it
    unsigned long long *dbg;     // optional diagnostics: per pair {slow-path entries, s_memtime ticks}
    uint32_t        dbg_thr0;    // diagnostics only: initial threshold (timing runs without the rare path)
    uint32_t        dbg_pad;
    uint32_t        n_pairs;
    uint32_t        cell_cap;
    int32_t         match, mismatch, gap;
    uint32_t        strict;      // tie mode
    uint32_t        mode;        // 0 = direction field in HBM, 1 = checkpoints + window maxima, 2 = checkpoints + event-tracked maxima
    uint32_t        skip_multi;  // mode 1: the pairs of several strips are left to sw_sweep_winmax_strips_kernel
    // mode 1, reads longer than one strip: one wavefront per STRIP, pipelined through the seam rows
    const StripItem *strip_items; // the strips of a (pair, column chunk) consecutive and ascending
    uint32_t       *progress;    // per strip item: 16-step blocks finished (the item's index is PairDesc.pad + strip)
    uint32_t        n_strip_items;
    uint32_t        n_out;       // entries of out[]: the pairs of the whole launch (n_pairs is this kernel's share of them).  Read by the sweeps of
                                 // option "end_bonus" alone: their EndOut array lies behind the pair outputs, at out + n_out
    uint32_t       *err_host;    // host-mapped word, set to 1 when a strip gave up waiting for its producer
    const ColItem  *col_items;   // mode 1: column chunks of single-strip pairs (few pairs, long references)
    uint32_t        n_col_items;
    uint32_t        strip_spins; // spin budget of the strip pipeline before it gives up (0: default)
    uint32_t       *q_reset;     // split traceback: its walk-item counter, zeroed by the sweep kernel (a memset would be one more launch)
};

struct TraceArgs {
    const uint32_t *seqw;
    const SeqDesc  *refs;
    const SeqDesc  *reads;
    const PairDesc *pairs;
    const uint32_t *dir;
    PairOut        *out;
    const uint2    *cells;
    const uint64_t *cells_off;
    const uint32_t *cells_cap;
    ArenaHdr       *hdr;
    uint32_t       *arena;
    uint64_t        arena_cap_words;
    uint32_t        n_pairs;
    uint32_t        cell_cap;
    int32_t         match, mismatch, gap;
    uint32_t        strict;
    uint32_t        lds_words;   // staging words per block for the ops of one alignment
    uint32_t        lds_read_words;   // LDS dwords reserved for the longest read's codes
    unsigned long long *dbg;     // optional diagnostics: per pair {ticks, walk ticks, steps, tiles}
    const int32_t  *seam;        // mode 1: strip seam rows for the replay of multi-strip pairs
    PairOut        *out_host;    // zero-copy results: host-mapped mirror of out[] (written by slot 0 of every pair), or null
    uint32_t       *ovf_host;    // zero-copy results: set to 1 when a record did not fit the (host-mapped) arena
    uint32_t        mode;        // same as FillArgs.mode
    uint32_t        pad2;        // set by the launcher of sw_traceback_winmax_kernel: a second set of window tiles is there (speculative staging)
    // split traceback (mode 1, tie-heavy or tiny batches): sw_detect_windows_kernel lists the maximum cells one wavefront
    // per candidate WINDOW and queues one walk item per cell, sw_walk_items_kernel walks one alignment per wavefront
    const uint32_t *win_off;     // per pair of the launch: index of its first window among all windows (n_pairs + 1 entries)
    uint32_t       *q_count;     // walk items queued
    uint4          *q_items;     // {pair index of the launch, i, j, 0}
    uint32_t        q_cap;
    uint32_t        pad4;
    // the two aligned strings of every alignment, written behind its record (swmi_emit.h): the caller's bytes as uploaded
    const uint8_t  *raw;         // null: records carry the 2-bit ops only and the host builds the strings
    const uint64_t *raw_off;     // byte offsets into raw: n_refs + 1 for the references, then n_reads + 1 for the reads
    uint32_t        raw_reads_at;   // index of the reads' first offset in raw_off (= n_refs + 1)
    uint32_t        rec_tab_cap;    // entries the record table holds
    AlnRec         *rec_tab;        // the record table (host-mapped with zero-copy results)
};

// extra arguments of sw_resident_pairs_kernel (kept out of TraceArgs: the traceback kernels are at their SGPR limit)
struct ResidentArgs {
    const uint32_t *res_items;   // indices into pairs[]: pairs whose whole direction field fits a wavefront's share of LDS
    uint32_t        n_res;
    uint32_t        res_lds_words;   // LDS dwords per wavefront (the largest resident pair of the launch)
    uint32_t        res_cell_cap;    // maximum cells a resident pair may list in LDS (more: SWMI_F_CELL_OVF, re-run by the ordinary path)
    uint32_t        res_ops_words;   // dwords of packed ops a lane can stage (the longest possible path of the launch)
};

// extra arguments of sw_tfused_kernel (swmi_tfused.hip): pairs swept in the transposed layout and traced back by the same wavefront
struct TFusedArgs {
    const uint32_t *items;       // indices into pairs[]
    uint32_t        n_items;
    uint32_t        lds_words;   // LDS dwords per wavefront: tile | cells | staged ops | reference codes | read codes
    uint32_t        tile_words;  // direction tile of one block: ceil((m_max + 63) / 16) * 64 * SWMI_TF_BR
    uint32_t        cell_cap;    // maximum cells a block lists per pass (a block with more is re-swept once per `cell_cap` cells)
    uint32_t        pad0;
    uint32_t        ref_words;   // LDS dwords for the longest reference's codes
    uint32_t        read_words;  // ... and the longest read's
    uint32_t        stage_words; // LDS dwords for the ops of ONE alignment staged one per byte (the longest possible path)
    uint32_t        debug_marks; // diagnostics: workgroup 0 leaves progress marks in the host-mapped result header
    uint32_t        n_helpers;   // wavefronts per workgroup (0..2) beyond the four that sweep: they only take block tasks
};
#define SWMI_TF_HELPERS 2u          // wavefronts per workgroup beyond the four sweepers, at most
#define SWMI_TF_BMAX   40u          // columns per lane of the transposed sweep: references up to 64 * 40 = 2560 bases
#ifndef SWMI_TF_BR
#define SWMI_TF_BR     4u           // columns per lane of a re-swept block: 256 columns (5: 320 columns, fewer walks leave the block, but every
                                    // re-sweep costs 14 % more -- measured 0.166 against 0.149 ms at the headline)
#endif
#define SWMI_TF_MAX_M  256u         // reads up to 256 bases (LDS tile of a block: (m + 63) / 16 KB)
// columns per lane for a reference of n bases (even: the kernel is instantiated for 2, 4, ..., SWMI_TF_BMAX)
SWMI_HD static inline uint32_t swmi_tf_cols_per_lane(uint32_t n) {
    uint32_t b = (n + 63u) / 64u;
    b = (b + 1u) & ~1u;
    return b < 2u ? 2u : b;
}
// dwords of column checkpoints of a pair swept by sw_tfused_kernel: one 64-lane row per step, m + L - 1 <= m + 63 steps
SWMI_HD static inline uint64_t swmi_tf_ck_words(uint32_t m) { return ((uint64_t)m + 64u) * 64u; }

#define SWMI_RANK_BY_CELL 0xFFFFFFFFu   // AlnRec.rank of the split traceback: the host orders a pair's records by (end_i, end_j)
#define SWMI_DETECT_LCAP  64u           // cells one window may hold before the pair is handed to the exact-size re-run

// rows per lane for a read of m bases
SWMI_HD static inline uint32_t swmi_rows_per_lane(uint32_t m) {
    uint32_t r = (m + 63u) / 64u;
    return r < 1u ? 1u : (r > SWMI_RMAX ? SWMI_RMAX : r);
}
// dwords of per-pair workspace.  mode 0: the direction field; mode 1: lane-state checkpoints + one maximum per
// checkpoint window; mode 2: lane-state checkpoints (mode 3, the affine kernels: swmi_aff_pair_dir_words below).
// tfused: the context lets sw_tfused_kernel take pairs (option "tfused" = 1): such a pair keeps its column checkpoints in the
// same region, which must then hold them.
SWMI_HD static inline uint64_t swmi_dir_words(uint32_t m, uint32_t n, uint32_t mode, bool tfused = false) {
    uint32_t R = swmi_rows_per_lane(m);
    uint64_t strips = ((uint64_t)m + 64u * R - 1u) / (64u * R);
    uint64_t wblocks = ((uint64_t)n + 63u + 15u) / 16u;   // T = n + 63 steps at most
    if (mode == 0) return strips * wblocks * R * 64u;
    uint64_t n_ck = (wblocks + SWMI_CK_BLOCKS - 1u) / SWMI_CK_BLOCKS;
    uint64_t words = strips * (n_ck * (R + 2u) * 64u + (mode == 1 ? ((n_ck + 63u) & ~(uint64_t)63u) : 0u));
    if (tfused && mode == 1 && m <= 256u && n <= 64u * 40u && ((uint64_t)m + 64u) * 64u > words) words = ((uint64_t)m + 64u) * 64u;
    return words;
}
// ---- affine gaps (swmi_affine.hip): one wavefront per pair, R = ceil(m / 64) rows per lane, 4-bit codes, 8 steps per dword ----
#define SWMI_AFF_RMAX     16u         // rows per lane of the widest affine sweep: reads of at most 1024 bases
#define SWMI_AFF_MAX_READ (64u * SWMI_AFF_RMAX)
#define SWMI_AFF_TB_SLOTS 4u          // traceback wavefronts per pair: slot s walks the maximum cells s, s + 4, ...
#define SWMI_AFF_TILE_WORDS 4096u     // LDS dwords of a traceback wavefront's direction tile (at least one 8-step block)
SWMI_HD static inline uint32_t swmi_aff_rows_per_lane(uint32_t m) {
    uint32_t r = (m + 63u) / 64u;
    return r < 1u ? 1u : r;
}
// 8-step blocks of a pair's field: T = n + lact - 1 anti-diagonal steps, lact = the lanes that own read rows
SWMI_HD static inline uint32_t swmi_aff_blocks(uint32_t m, uint32_t n) {
    const uint32_t R = swmi_aff_rows_per_lane(m), lact = m ? (m + R - 1u) / R : 1u;
    return (uint32_t)(((uint64_t)n + lact - 1u + 7u) / 8u);
}
// ---- reads longer than SWMI_AFF_MAX_READ (option "long_reads"): swept in strips of 1024 rows, every strip with 16 rows per lane ----
// strips of a read of m bases (the last one padded with SWMI_CODE_PAD rows)
SWMI_HD static inline uint32_t swmi_aff_strips(uint32_t m) { return m ? (m + SWMI_AFF_MAX_READ - 1u) / SWMI_AFF_MAX_READ : 1u; }
// 8-step blocks of ONE strip's field: the field of a (1024, n) pair, all 64 lanes own rows
SWMI_HD static inline uint32_t swmi_aff_strip_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + 63u + 7u) / 8u); }
// dwords of one strip's field: [block][row slot][lane]
SWMI_HD static inline uint64_t swmi_aff_strip_words(uint32_t n) { return (uint64_t)swmi_aff_strip_blocks(n) * SWMI_AFF_RMAX * 64u; }
// ---- option "band" (half-width w >= 1, reads longer than SWMI_AFF_MAX_READ only): strip s sweeps the WINDOW of columns
// swmi_aff_band_lo(s, w) .. swmi_aff_band_hi(s, n, w) -- the band |j - i| <= w rounded outwards to the strip -- and leaves the
// field of a (1024, window length) pair; the strips' fields are consecutive, now of unequal size.  The host refuses a pair with
// an empty window, so lo <= hi holds for every strip a kernel sees. ----
#define SWMI_AFF_BAND_MAX (1u << 20)
// the value of a cell outside the band in fit and global mode: below every real value less three scores, and two more scores
// added to it do not leave int32 (DESIGN.md 8f derives it from the bounds of a banded run): -2^31 + 2^27
#define SWMI_AFF_BAND_NEG (-2013265920)
SWMI_HD static inline uint32_t swmi_aff_band_lo(uint32_t s, uint32_t w) {
    const uint64_t a = (uint64_t)SWMI_AFF_MAX_READ * s;                  // 1024 s + 1 - w, at least 1
    return a > w ? (uint32_t)(a + 1u - w) : 1u;
}
SWMI_HD static inline uint32_t swmi_aff_band_hi(uint32_t s, uint32_t n, uint32_t w) {
    const uint64_t a = (uint64_t)SWMI_AFF_MAX_READ * ((uint64_t)s + 1u) + w;
    return a < n ? (uint32_t)a : n;
}
// 8-step blocks of strip s's field: swmi_aff_strip_blocks of its window
SWMI_HD static inline uint32_t swmi_aff_band_blocks(uint32_t s, uint32_t n, uint32_t w) {
    return swmi_aff_strip_blocks(swmi_aff_band_hi(s, n, w) - swmi_aff_band_lo(s, w) + 1u);
}
// blocks of the strips before strip s, in closed form.  With B(x) = (x + 70) / 8 the blocks of a window of x columns, strips
// below sa = w / 1024 + 1 start at column 1 and strips from sb = the first s with 1024 (s + 1) + w >= n on end at column n:
//   s < sa, s < sb    window 1024 (s + 1) + w    128 (s + 1) + B(w)
//   between the two   window n (sb < sa) or 1024 + 2 w (sa < sb): the same for every such strip
//   s >= sa, s >= sb  window n + w - 1024 s        B(n + w) - 128 s
// (1024 s is a multiple of 8, so it leaves the rounding alone) -- three arithmetic series.
SWMI_HD static inline uint64_t swmi_aff_band_blocks_before(uint32_t s, uint32_t n, uint32_t w) {
    const uint64_t sa = (uint64_t)w / SWMI_AFF_MAX_READ + 1u;
    const uint64_t sb = (uint64_t)n > (uint64_t)SWMI_AFF_MAX_READ + w ? ((uint64_t)n - w + SWMI_AFF_MAX_READ - 1u) / SWMI_AFF_MAX_READ - 1u : 0u;
    const uint64_t p = sa < sb ? sa : sb, q = sa < sb ? sb : sa;
    const uint64_t k1 = s < p ? s : p;
    const uint64_t e2 = s < q ? s : q, k2 = e2 > p ? e2 - p : 0u;
    const uint64_t k3 = s > q ? s - q : 0u;
    const uint64_t mid = sb < sa ? ((uint64_t)n + 70u) / 8u : ((uint64_t)SWMI_AFF_MAX_READ + 2ull * w + 70u) / 8u;
    return 64ull * k1 * (k1 + 1u) + k1 * (((uint64_t)w + 70u) / 8u)
         + k2 * mid
         + k3 * (((uint64_t)n + w + 70u) / 8u) - 64ull * k3 * (2u * q + k3 - 1u);
}
// dword offset of strip s's field in the pair's (s = the pair's strips: the dwords of the whole field)
SWMI_HD static inline uint64_t swmi_aff_band_strip_off(uint32_t s, uint32_t n, uint32_t w) {
    return swmi_aff_band_blocks_before(s, n, w) * SWMI_AFF_RMAX * 64u;
}
// ---- option "gap_open2" (two-piece gaps, global and extend runs): the field has two 4-bit planes, interleaved per
// 8-step block -- dword ((w * 2 + plane) * R + k) * 64 + lane -- so every block, strip and field is twice the one-piece size, and
// the seam row carries (H, F1, F2) per column in 16-byte entries.  A traceback tile must hold one block: 2 * 16 * 64 dwords. ----
static_assert(2u * SWMI_AFF_RMAX * 64u <= SWMI_AFF_TILE_WORDS, "a two-plane block fits the traceback tile");
// ---- option "band_adapt" (with band = w and option "extend"): the window of strip s follows a CENTRE c that the
// sweep takes from the seam row above the strip -- c_lo = max(1, c + 1 - w), c_hi = min(n, c + 1024 + w), 0 <= c <= n; c = 0 is
// strip 0's (static) window.  A window has at most min(n, 1024 + 2 w) columns, and every strip's field gets the blocks of that
// many: a fixed stride, blocks beyond a strip's actual window neither written nor read.  Behind the NS fields the sweep leaves
// the WINDOW TABLE, the centre it used for every strip it swept: what the traceback and swmi_pair_band_window read. ----
SWMI_HD static inline uint32_t swmi_aff_adapt_lo(uint32_t c, uint32_t w) { return c + 1u > w ? c + 1u - w : 1u; }
SWMI_HD static inline uint32_t swmi_aff_adapt_hi(uint32_t c, uint32_t n, uint32_t w) {       // (c <= n; w <= SWMI_AFF_BAND_MAX)
    return n - c > SWMI_AFF_MAX_READ + w ? c + SWMI_AFF_MAX_READ + w : n;
}
// dwords of one strip's field
SWMI_HD static inline uint64_t swmi_aff_adapt_strip_words(uint32_t n, uint32_t w) {
    const uint64_t cols = (uint64_t)SWMI_AFF_MAX_READ + 2ull * w;
    return swmi_aff_strip_words(cols < n ? (uint32_t)cols : n);
}
// ---- a mode-3 pair's workspace under the run's options.  AffGeom holds the options that decide it, and these three functions alone
// choose between the layouts above: an option that changes it is a member and a case here (SchedKey, swmi_host.h, keys on the struct) ----
struct AffGeom {
    uint32_t band;       // option "band": the half-width, 0: none (it shapes the fields of reads longer than SWMI_AFF_MAX_READ only)
    bool adapt, two;     // options "band_adapt" (with band, never with two) and "gap_open2"
    bool subopt;         // option "subopt" (local runs: never with adapt or two): the pair's row of column maxima behind its fields
    bool hits;           // option "hits" (with subopt only): a second row behind that one, the smallest row that holds each column's maximum
    bool operator==(const AffGeom &o) const { return band == o.band && adapt == o.adapt && two == o.two && subopt == o.subopt && hits == o.hits; }
};
// dwords of the pair's direction fields (m > 1024: the strips', consecutive) = where the window table of "band_adapt" or the
// row of column maxima of "subopt" starts
SWMI_HD static inline uint64_t swmi_aff_pair_table_off(uint32_t m, uint32_t n, AffGeom g) {
    const uint64_t planes = g.two ? 2u : 1u, ns = swmi_aff_strips(m);
    if (m <= SWMI_AFF_MAX_READ) return planes * swmi_aff_blocks(m, n) * swmi_aff_rows_per_lane(m) * 64u;
    if (!g.band) return planes * ns * swmi_aff_strip_words(n);                      // every strip the whole reference
    if (g.adapt) return ns * swmi_aff_adapt_strip_words(n, g.band);                 // a fixed stride per strip
    return planes * swmi_aff_band_strip_off((uint32_t)ns, n, g.band);               // the strips' windows: the offset of strip NS
}
// ---- option "subopt" (local runs): behind the fields the sweep leaves colmax(j), the maximum of H over column j, one
// int32 per column j = 1 .. n at dword j - 1, for sw_subopt_kernel.  Under "band" the columns right of the last strip's window are
// never written: the row ends, for every reader, at swmi_aff_colmax_cols. ----
SWMI_HD static inline uint32_t swmi_aff_colmax_cols(uint32_t m, uint32_t n, uint32_t band) {
    return band && m > SWMI_AFF_MAX_READ ? swmi_aff_band_hi(swmi_aff_strips(m) - 1u, n, band) : n;
}
// what sw_subopt_kernel (swmi_subopt.hip) makes of the row, per pair: swmi.h's score2 and end2
struct SuboptOut { int32_t score2; uint32_t end2; };
// ---- option "hits" (with "subopt"): TWO ROWS, not one row of pairs.  The row of column maxima stays where and what it
// is under "subopt" alone; a second row of the same rounded length follows it and holds row(j), the smallest (1-based, global) read row
// with H(i, j) = colmax(j), at dword j - 1.  sw_hits_kernel passes over the values up to 2 K times and reads a row index K times: the
// passes stay dense 4-byte loads, and the sweeps' cmrow pointer and the in-place rewrite serve both rows with one stride.  row(j) is
// meaningful where colmax(j) > 0 (a column of zeros keeps the seed's 0); no other column is ever reported. ----
#define SWMI_HITS_MAX 16u
SWMI_HD static inline uint64_t swmi_aff_colmax_stride(uint32_t n) { return ((uint64_t)n + 63u) & ~63ull; }
// what sw_hits_kernel (swmi_subopt.hip) makes of the two rows, per pair: 1 + K entries of 16 bytes -- entry 0 is (n_hits, 0, 0, 0), entries
// 1 .. n_hits are swmi.h's swmi_hit k - 1, the rest is zero
struct HitEnt { int32_t score; uint32_t end_i, end_j, reserved; };
// what the pair is charged in the launch's `dir` workspace: the fields and, under "band_adapt", the table -- one dword per strip --
// or, under "subopt", the row of column maxima -- one per column, and under "hits" the row of their rows behind it; each rounded to 64
// dwords so that the next pair's field stays 256-byte aligned
SWMI_HD static inline uint64_t swmi_aff_pair_dir_words(uint32_t m, uint32_t n, AffGeom g) {
    return swmi_aff_pair_table_off(m, n, g) + (g.band && g.adapt && m > SWMI_AFF_MAX_READ ? ((uint64_t)swmi_aff_strips(m) + 63u) & ~63ull : 0ull) +
           (g.subopt ? (g.hits ? 2ull : 1ull) * (((uint64_t)n + 63u) & ~63ull) : 0ull);
}
// dwords of the pair's seam row: (H, F) per column, two-piece 16 bytes; ONE row, rewritten in place by every strip but the last
SWMI_HD static inline uint64_t swmi_aff_pair_seam_words(uint32_t m, uint32_t n, AffGeom g) { return m > SWMI_AFF_MAX_READ ? (g.two ? 4ull : 2ull) * n : 0ull; }
// score matrices (swmi_set_score_matrix) on the affine sweeps: at most 64 symbols, plus class n = outside the alphabet.
// Device image: 256 key dwords by base code (class * 4 | hi << 16, hi = the code outside the alphabet, else 0x1FF), then the
// (n+1) x (n+1) int32 scores, row = read class, column = reference class (row and column n are not read: the kernel fills them).
#define SWMI_MAT_MAX_SYMBOLS 64u
#define SWMI_MAT_NN_MAX (SWMI_MAT_MAX_SYMBOLS + 1u)
SWMI_HD static inline uint32_t swmi_aff_mat_words(uint32_t nn) { return 256u + nn * nn; }

// int32 seam rows of a pair whose read spans several strips: one row of n+1 per strip
SWMI_HD static inline uint64_t swmi_seam_words(uint32_t m, uint32_t n) {
    if (m <= 64u * SWMI_RMAX) return 0;
    uint64_t strips = ((uint64_t)m + 64u * SWMI_RMAX - 1u) / (64u * SWMI_RMAX);
    return strips * ((uint64_t)n + 1u);
}
