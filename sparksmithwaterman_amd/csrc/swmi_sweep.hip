// swmi_sweep.hip -- gfx950 (MI355X / CDNA4) sweep kernels of the Smith-Waterman hot path, reached through swmi_launch_fill:
//   sw_fill_kernel                  mode 0: scores + the 2-bit direction field to HBM, tied maxima listed on the way
//   sw_fill_score_kernel            mode 2: scores + lane-state checkpoints, tied maxima listed on the way
//   sw_sweep_winmax_kernel          mode 1 (the default, the headline path): checkpoints + one maximum per checkpoint window
//   sw_sweep_winmax_strips_kernel   mode 1, reads of several strips: one wavefront per (pair, strip)
//   sw_sweep_winmax_cols_kernel     mode 1, long references: one wavefront per column chunk of a pair
//
// Replaces, for a whole batch of (reference, read) pairs at once, what the reference does per pair in
//   ScoreMatrix.call   src/sw/SmithWaterman.java:129-190  (fill, max-cell list)
//   GetCellScore.call  src/sw/SmithWaterman.java:217-252  (cell rule, tie order)   [DistributedSW.java:305-330 for strict]
// (GetAlignment.call, the traceback: swmi_traceback.hip.)
//
// ONE WAVEFRONT (64 lanes) PER PAIR, anti-diagonal systolic sweep.
//   lane l owns R consecutive read rows (i = strip*64R + l*R + k + 1, k < R) and at step t works on
//   reference column j = t - l + 1, so the 64 lanes sit on one anti-diagonal band.  Per step a lane needs
//     W  = its own H of the previous step              (register)
//     N  = lane l-1's bottom-row H of the previous step (one DPP wave_shr:1, no LDS)
//     NW = the N it received one step earlier           (register carry)
//     the reference base of column j                    (flows down the lanes by a second DPP shift;
//                                                        lane 0 is fed from a scalar register)
//   int32 scores live in registers only; nothing but the 2-bit direction field is written to HBM, as
//   256-byte coalesced stores ([w][k][lane] layout, swmi_device.h).  Integer recurrence: no MFMA.
//   Rows beyond 64*R (long reads) are processed strip after strip; the seam row between two strips
//   goes through a small per-pair buffer.
//   Tied maxima: a wave-uniform threshold `thr` (scalar register) holds the running maximum; only when
//   some lane reaches it does the wave leave the hot loop to append (i,j) to the pair's cell list
//   (clearing it on a strict increase, exactly like SmithWaterman.java:176-185).
// The blocks and cell streams all of them are made of: swmi_cells.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdlib.h>
#include "swmi_device.h"
#include "swmi_launch.h"
#include "swmi_cells.h"

typedef uint32_t Words4 __attribute__((ext_vector_type(4)));
typedef const Words4 __attribute__((address_space(4))) *ConstWords4;     // constant address space: uniform loads become s_load

// ------------------------------------------------------------------------------------------------
// fill: one pair, one wavefront.  R rows per lane; ACGT = both sequences made of the eight fast symbols
// (A,C,G,T,N,U,R,Y -- the template parameter kept its first name) and match/mismatch fit a
// signed nibble (profile lookup by v_dot8_i32_i4 instead of compare+select); STRICT = DistributedSW tie order;
// MULTI = more than one strip of 64*R rows (seam rows through memory); MODE = FIELD or SCORE.
// ------------------------------------------------------------------------------------------------
// PIPE (mode 1, MULTI): this wavefront sweeps only strip `my_strip`; the wavefront of strip s-1 runs a few blocks ahead
// and publishes its progress, the one of strip s+1 follows -- a systolic pipeline of strips over wavefronts, so a
// 10 kbp read is swept in about the time of ONE strip instead of 40.
#define SWMI_PIPE_PUBLISH 2u      // blocks between two publications of a strip's progress
template <int R, bool ACGT, bool STRICT, bool MULTI, int MODE, bool PIPE = false>
__device__ __forceinline__ void fill_pair(const FillArgs &A, const PairDesc pd, const uint32_t lane, const uint32_t my_strip = 0u,
                                          const StripItem *item = nullptr) {
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    // PIPE: the geometry in scalar registers, so that the block counter is one and the reference words can come through
    // the scalar cache: a vector load's s_waitcnt vmcnt also waits for every store issued before it, the device-scope seam
    // stores among them
    const uint32_t n_full = PIPE ? uni(rd.len) : rd.len, m = PIPE ? uni(qd.len) : qd.len;
    // PIPE, column chunk (StripItem): the sweep starts at reference column col0 + 1 from a zero state and owns the windows
    // g_lo .. g_hi-1; the whole reference is the chunk {0, 0, all windows}
    const uint32_t col0 = PIPE ? uni(item->col0) : 0u;
    const uint32_t g_lo = PIPE ? uni(item->g_lo) : 0u, g_hi = PIPE ? uni(item->g_hi) : 0xFFFFFFFFu;
    const uint32_t priv_stride = PIPE ? uni(item->priv_stride) : 0u;
    const uint32_t *__restrict__ refw = A.seqw + (PIPE ? uni(rd.boff) + (col0 >> 2) : rd.boff);
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const int match = A.match, mismatch = A.mismatch, gap = A.gap;
    constexpr uint32_t HMODE = MODE == SWMI_MODE_FIELD ? 0u : (MODE == SWMI_MODE_WINMAX ? 1u : 2u);
    const StripGeom G = strip_geom<R>(m, n_full, HMODE);
    int pair_max = 0;        // WINMAX: maximum over the finished windows

    const uint64_t cbase = A.cells_off ? A.cells_off[pd.out_id] : (uint64_t)pd.out_id * A.cell_cap;
    const uint32_t ccap = A.cells_cap ? A.cells_cap[pd.out_id] : A.cell_cap;
    uint2 *__restrict__ cells = A.cells + cbase;

    FillState<R> S;
    S.thr = A.dbg ? (int)A.dbg_thr0 : 1;   // a max of 0 never enters the list: that is the degenerate case
    S.cnt = 0;
    S.ev_prev = 0;
    S.events = 0;
    S.dbg_skip = A.dbg && (A.dbg_pad != 0);
#ifdef SWMI_STRIP_DIAG
    S.dg_pub = 0;
#endif
    const unsigned long long t_start = A.dbg ? __builtin_amdgcn_s_memtime() : 0ull;

    const uint32_t s_begin = PIPE ? my_strip : 0u, s_end = PIPE ? my_strip + 1u : G.n_strips;
    uint32_t *__restrict__ progress = PIPE ? A.progress + uni(item->prog) : nullptr;
    for (uint32_t s = s_begin; s < s_end; ++s) {
        const uint32_t row0 = s * G.rps + lane * R;        // 0-based first row of this lane
        const uint32_t rows_left = m - s * G.rps;
        const uint32_t lact = rows_left >= G.rps ? WAVE : (rows_left + R - 1) / R;   // lanes holding rows
        // columns this strip sweeps (from col0 + 1 on).  A column chunk that is not the pair's last ends after its last
        // window -- 64 steps later per strip below this one, whose lane 0 needs the seam that far -- unless that is past
        // the reference's end
        uint32_t n = n_full - col0;
        bool truncated = false;
        if (PIPE && g_hi < G.n_ck) {
            const uint32_t ext = 16u * SWMI_CK_BLOCKS * g_hi - col0 + WAVE * (G.n_strips - 1u - s);
            if (ext < n) { n = ext; truncated = true; }
        }
        const uint32_t T = truncated ? n : n + lact - 1; // steps of this strip
        const uint32_t lane_eff = lane < lact ? lane : 0x40000000u;   // lanes without rows are never in range
        setup_rows<R, ACGT>(S, readw, row0, m, match, mismatch);
        S.lmax = -1;

        uint32_t *__restrict__ wsp = A.dir + pd.dir_off + s * G.strip_words + lane;   // this strip's workspace
        // WINMAX: one maximum per checkpoint window.  Lanes without rows are left out; the pad rows of the last lane with
        // rows cannot exceed the real cells they derive from (mismatch <= 0 and gap <= 0 are required for this mode), so the
        // pair's maximum is exact and a window can at worst be listed without holding a maximum cell.
        auto close_window = [&](uint32_t g) {
            const int wm = wave_max_i32(lane < lact ? S.lmax : -1);
            if (lane == 0) A.dir[pd.dir_off + s * G.strip_words + G.wmax_off + g] = (uint32_t)wm;
            pair_max = pair_max > wm ? pair_max : wm;
            S.lmax = -1;
        };
        const int32_t *seam_in = nullptr;
        int32_t *seam_out = nullptr;
        int32_t *seam_sh = nullptr;                                   // column chunk: the pair's shared row, for the columns the chunk owns
        if (MULTI) {
            int32_t *sb = A.seam + pd.seam_off;                       // row s = H of the strip's last read row
            seam_in = sb + (uint64_t)(s > 0 ? s - 1 : 0) * (n_full + 1);
            seam_out = sb + (uint64_t)s * (n_full + 1);
            if (PIPE && priv_stride) {
                int32_t *pb = A.seam + item->priv_off;                // the chunk's own rows, indexed by local column
                seam_sh = seam_out + col0;
                seam_in = pb + (uint64_t)(s > 0 ? s - 1 : 0) * priv_stride;
                seam_out = pb + (uint64_t)s * priv_stride;
            }
        }
        const uint32_t step_w = 16u * SWMI_CK_BLOCKS;
        const uint32_t own_lo = step_w * g_lo > col0 ? step_w * g_lo - col0 : 0u;                  // owned local columns: own_lo < c <= own_hi
        const uint32_t own_hi = g_hi < G.n_ck ? step_w * g_hi - col0 : 0xFFFFFFFFu;
        const bool feeds_seam = MULTI && (s + 1 < G.n_strips);
        const bool reads_seam = MULTI && (s > 0);

        const uint32_t nblk = (T + 15u) / 16u;
        const uint4 *__restrict__ refq = reinterpret_cast<const uint4 *>(refw);   // images are 16-byte aligned
        const ConstWords4 refq_s = (ConstWords4)(uintptr_t)refw;                  // the same through the scalar cache (read-only data)
        auto ref_words = [&](uint32_t i) -> uint4 {
            if (PIPE) { const Words4 v = refq_s[i]; return make_uint4(v.x, v.y, v.z, v.w); }
            return refq[i];
        };
        uint4 wnext = ref_words(0u);
        // The seam row above this strip is read in GROUPS of 64 columns (4 blocks): seam_in[64g + 1 + lane], one coalesced
        // load per group, issued one group ahead; a block takes its 16 values (N of lane 0 for its 16 steps) from the
        // group register with one ds_bpermute.
        // PIPE: column c of the seam row is stored by the producer's lane 63 at step c + 62, so the columns of block x are
        // complete when the producer has finished block x + 4; the producer publishes its progress every SWMI_PIPE_PUBLISH
        // blocks and the polled value is kept, so a consumer that is behind does not poll at all (a poll and a wait for
        // the stores' acknowledgements per block: 0.415 ms at 257 x 4000; every 4 blocks, 24 polls per 254 blocks: 0.357;
        // every 2 blocks with the next group asked for 2 blocks ahead instead of 4 costs two strips 2 % and gains a
        // 40-strip pipeline 3 %: profiles/r03/strip_pipeline.md).
        uint32_t nblk_prod = (n_full - col0 + WAVE - 1u + 15u) / 16u;
        if (truncated || (PIPE && g_hi < G.n_ck)) {
            const uint32_t ext_p = 16u * SWMI_CK_BLOCKS * g_hi - col0 + WAVE * (G.n_strips - s);      // (strip s-1's extent)
            if (ext_p < n_full - col0) nblk_prod = ext_p / 16u;
        }
        bool gave_up = false;
        uint32_t prod_seen = 0u;
#ifdef SWMI_STRIP_DIAG
        // -DSWMI_STRIP_DIAG + SWMI_DEBUG_FILL=1: where a strip's wavefront waits (s_memtime ticks, 10 ns)
        unsigned long long dg_poll = 0, dg_grp = 0, dg_polls = 0;
#endif
        auto load_group = [&](uint32_t g) -> int {
            const uint32_t col = 64u * g + 1u + lane;
            if (64u * g >= n) return 0;
            if (PIPE) {
                const uint32_t need = 4u * g + 8u < nblk_prod ? 4u * g + 8u : nblk_prod;
                // the give-up is progress-based: the budget (~60 ms of s_sleep by default) restarts whenever the producer
                // advances, so a slow producer is waited for and only one that does not move at all is abandoned -- the host
                // then re-runs the chunk with the one-wavefront sweep, which needs no other workgroup (swmi_run.cpp)
                const uint32_t budget = A.strip_spins ? A.strip_spins : (1u << 18);
                uint32_t spins = 0;
                SWMI_SD(const unsigned long long dg0 = __builtin_amdgcn_s_memtime(); if (prod_seen < need) dg_polls++;)
                while (prod_seen < need && !gave_up) {
                    const uint32_t p = __builtin_amdgcn_readfirstlane(
                        __hip_atomic_load(progress + (s - 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    if (p != prod_seen) { prod_seen = p; spins = 0; continue; }
                    __builtin_amdgcn_s_sleep(8);
                    if (++spins > budget) {
                        gave_up = true;
                        if (lane == 0 && A.err_host) *A.err_host = 1u;
                    }
                }
                SWMI_SD(dg_poll += __builtin_amdgcn_s_memtime() - dg0;)
            }
            return col <= n ? __hip_atomic_load(seam_in + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        };
        int seam_grp = 0, seam_grp_next = reads_seam ? load_group(0u) : 0;
        for (uint32_t tb = 0; tb < nblk; ++tb) {
            const uint4 w = wnext;                       // base codes of columns 16tb+1 .. 16tb+16
            wnext = ref_words(tb + 1u);                  // prefetch (images are padded)
            const uint32_t t0 = 16u * tb;
            const uint32_t tbg = tb + (col0 >> 4);       // the block's number in the pair's own sweep (col0 is a multiple of 32)
            const uint32_t gw = tbg / SWMI_CK_BLOCKS;    // ... and its window
            if (MODE == SWMI_MODE_WINMAX && (tbg % SWMI_CK_BLOCKS) == 0u && tb > 0u) {
                if (gw > g_lo && gw <= g_hi) close_window(gw - 1u); else S.lmax = -1;
            }
            if ((MODE == SWMI_MODE_SCORE || MODE == SWMI_MODE_WINMAX) && (tbg % SWMI_CK_BLOCKS) == 0u && gw >= g_lo && gw < g_hi) {
                // checkpoint: everything a replay of steps t0.. needs from this lane ([ck][slot][lane], 256 B stores)
                uint32_t *__restrict__ ck = wsp + (uint64_t)gw * (R + 2) * WAVE;
#pragma unroll
                for (int k = 0; k < R; ++k) ck[k * WAVE] = (uint32_t)S.h[k];
                ck[R * WAVE] = (uint32_t)S.nprev;
                ck[(R + 1) * WAVE] = (uint32_t)S.rb;
            }
            if (reads_seam && (tb & 3u) == 0u) {
                SWMI_SD(const unsigned long long dg1 = __builtin_amdgcn_s_memtime();)
                seam_grp = seam_grp_next;
                SWMI_SD(asm volatile("s_waitcnt vmcnt(0)" : "+v"(seam_grp) :: "memory"); dg_grp += __builtin_amdgcn_s_memtime() - dg1;)
            }
            // the next group is asked for two blocks before it is needed, not four: every block of distance is a block a
            // strip trails the one above it, and a 10 kbp read is a pipeline of 40 strips
            if (reads_seam && (tb & 3u) == 2u) seam_grp_next = load_group(tb / 4u + 1u);
            // lanes 0..15: the block's 16 values (0 in every lane of a strip without a seam above it)
            const int seamv = reads_seam ? __builtin_amdgcn_ds_bpermute((int)(((tb & 3u) << 6) + ((lane & 15u) << 2)), seam_grp) : 0;
            const bool steady = (t0 + 1u >= lact) && (t0 + 15u < n);     // (a truncated strip never leaves the reference)
            // progress value p = "blocks 0 .. p-1 are complete", published every SWMI_PIPE_PUBLISH blocks, one block late
            uint32_t *pub_slot = PIPE ? progress + s : nullptr;
            const uint32_t pub_val = (PIPE && feeds_seam && tb > 0u && (tb % SWMI_PIPE_PUBLISH) == 0u) ? tb : 0u;
            if (steady)
                fill_block16<R, ACGT, STRICT, MULTI, false, MODE, PIPE>(S, w, t0, lane, lane_eff, n, m, row0, gap, match, mismatch,
                                                                        seamv, reads_seam, feeds_seam, seam_out, cells, ccap,
                                                                        pub_slot, pub_val, seam_sh, own_lo, own_hi);
            else
                fill_block16<R, ACGT, STRICT, MULTI, true, MODE, PIPE>(S, w, t0, lane, lane_eff, n, m, row0, gap, match, mismatch,
                                                                       seamv, reads_seam, feeds_seam, seam_out, cells, ccap,
                                                                       pub_slot, pub_val, seam_sh, own_lo, own_hi);
            if (PIPE && feeds_seam && tb + 1u == nblk) {
                // the strip is complete once its last seam stores have left the CU (they are device-coherent stores)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) __hip_atomic_store(progress + s, nblk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }

            if (MODE == SWMI_MODE_FIELD) {
                // ---- end of a 16-step block: one coalesced 256 B store per row slot -------------------
                // lanes that finished their last column inside this block still owe the missing shifts
                const int miss = (int)(t0 + 15u) - ((int)(lane + n) - 1);
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    uint32_t v = S.acc[k];
                    if (miss > 0 && miss < 16) v <<= 2 * miss;
                    wsp[((uint64_t)tb * R + k) * WAVE] = v;
                }
            }
        }
        if (MODE == SWMI_MODE_WINMAX) {
            const uint32_t gl = (nblk - 1u + (col0 >> 4)) / SWMI_CK_BLOCKS;
            if (gl >= g_lo && gl < g_hi) close_window(gl);
        }
#ifdef SWMI_STRIP_DIAG
        if (PIPE && A.dbg && lane == 0 && s < 2u) {
            const unsigned long long tot = __builtin_amdgcn_s_memtime() - t_start;
            // strip 0: {lifetime, waiting before publications}; strip 1: {lifetime, polls, waiting in polls, waiting for seam groups}
            A.dbg[2 * pd.out_id + s] = s == 0u ? (tot << 32) | (S.dg_pub & 0xFFFFFFFFull)
                                               : (tot << 40) | ((dg_polls & 0xFFull) << 32) | ((dg_poll & 0xFFFFull) << 16) | (dg_grp & 0xFFFFull);
        }
#endif
        // the tied-maximum test of the strip's last step is still pending (16 steps per block: its H is in S.h)
        if (S.ev_prev != 0) {
            handle_pending<R>(S, S.h, 16u * nblk - 1u, lane_eff, n, row0, m, cells, ccap);
            S.ev_prev = 0;
        }
        if (MULTI) __threadfence();    // seam row of this strip visible before the next strip reads it
    }

    if (PIPE) {
        // combine the strips: one atomicMax each into the record sw_sweep_winmax_kernel zeroed one launch earlier; the
        // traceback kernels complete it (finish_pair).  No fence: see sweep_fast.
        if (lane == 0 && pair_max > 0) atomicMax(&A.out[pd.out_id].score, pair_max);
        return;
    }
    if (lane == 0) {
        PairOut o;
        if (MODE == SWMI_MODE_WINMAX) {
            // the cells holding the maximum are listed by the traceback kernel (n_cells follows there)
            if (pair_max <= 0) { o.score = 0; o.flags = SWMI_F_DEGENERATE; o.n_cells = (uint64_t)m * n_full; }
            else               { o.score = pair_max; o.flags = 0u; o.n_cells = 0; }
        } else if (S.cnt == 0) { o.score = 0; o.flags = SWMI_F_DEGENERATE; o.n_cells = (uint64_t)m * n_full; }
        else            { o.score = S.thr; o.flags = S.cnt > ccap ? SWMI_F_CELL_OVF : 0u; o.n_cells = S.cnt; }
        A.out[pd.out_id] = o;
        if (A.dbg) {
            A.dbg[2 * pd.out_id] = S.events;
            A.dbg[2 * pd.out_id + 1] = __builtin_amdgcn_s_memtime() - t_start;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// mode-1 sweep, fast symbols, one strip (m <= 256): the headline path.  Same results, checkpoints and window maxima
// as fill_pair<..., SWMI_MODE_WINMAX>, from a shorter instruction stream (tools/gen_step.py: 3 VALU per cell, the
// neighbour exchanges folded into DPP arithmetic, 14.5 instructions per step at R = 3 instead of 17.8).
// COLS: this wavefront sweeps only the column chunk `ci` of the pair (swmi_device.h: ColItem).
// ------------------------------------------------------------------------------------------------
template <int R, bool COLS>
__device__ __forceinline__ void sweep_fast(const FillArgs &A, const PairDesc pd, const uint32_t lane, const ColItem ci) {
    // (moving the pair's geometry to scalar registers with readfirstlane makes the block loop scalar, and the sweep 3 % slower:
    // measured, tools/ab_headline.py -- the vector-side loop control overlaps the asm groups better than the scalar one)
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n_full = rd.len, m = qd.len;
    const StripGeom G = strip_geom<R>(m, n_full, 1u);
    const uint32_t col0 = COLS ? ci.col0 : 0u;
    const uint32_t g_lo = COLS ? ci.g_lo : 0u, g_hi = COLS ? ci.g_hi : G.n_ck;
    const bool last = g_hi >= G.n_ck;
    const uint32_t n = (last ? n_full : 16u * SWMI_CK_BLOCKS * g_hi) - col0;   // columns of this wavefront's (virtual) reference
    const uint32_t *__restrict__ refw = A.seqw + rd.boff + (col0 >> 2);
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const uint32_t lact = m >= G.rps ? WAVE : (m + R - 1) / R;           // lanes holding rows
    const uint32_t lane_eff = lane < lact ? lane : 0x40000000u;
    const uint32_t T = n + lact - 1;
    const uint32_t nblk = last ? (T + 15u) / 16u : n / 16u;               // (a chunk that is not the last ends on a window boundary)
    const uint32_t gm = (uint32_t)(-(int64_t)A.gap);                      // mode 1: gap <= 0
    const int one = 1;
    int pair_max = 0;

    const unsigned long long dbg_t0 = A.dbg ? __builtin_amdgcn_s_memtime() : 0ull;
    SweepState<R> S;
    build_profiles<R>(S.q, readw, lane * R, m, A.match, A.mismatch);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        S.h[k] = 0; S.g[k] = 0; S.hp[k] = 0;
    }
    S.lmax = -1;
    const uint4 *__restrict__ refq = reinterpret_cast<const uint4 *>(refw);   // 16-byte aligned: col0 is a multiple of 32
    uint4 wnext = refq[0];
    S.rby = 0;
    S.rbx = wave_shr1((int)(1u << (wnext.x & 31u)), 0);                   // lane 0: column 1; nothing has flowed further yet

    uint32_t *__restrict__ wsp = A.dir + pd.dir_off + lane;
    auto close_window = [&](uint32_t g) {
        const int wm = wave_max_i32(lane < lact ? S.lmax : -1);
        if (lane == 0) A.dir[pd.dir_off + G.wmax_off + g] = (uint32_t)wm;
        pair_max = pair_max > wm ? pair_max : wm;
        S.lmax = -1;
    };
    // The sweep in three parts.  HEAD: the blocks of a chunk's halo (windows before g_lo: no checkpoint, no maximum) and
    // whatever else is not steady; STEADY: the windows from g_lo on whose 32 steps all keep lane 0 inside the reference, one
    // pass of SweepWindowAsm's loop each -- checkpoint, reference loads, steps, window maximum and loop control in one
    // generated statement (tools/gen_step.py); TAIL: the remaining blocks, block by block like the head.
    int steady_max = -1;                                  // per lane: maximum over the steady windows (lanes with rows)
    bool closed = false;                                  // the window before block tb is closed already (by the steady part)
    for (uint32_t tb = 0; tb < nblk; ++tb) {
        const uint32_t tbg = tb + (col0 >> 4);            // the block's number in the pair's own sweep
        if ((tbg % SWMI_CK_BLOCKS) == 0u) {
            const uint32_t g = tbg / SWMI_CK_BLOCKS;
            if (tb > 0u && !closed) {
                if (g > g_lo) close_window(g - 1u); else S.lmax = -1;
            }
            closed = false;
#if !defined(SWMI_NO_ASM) && SWMI_CK_BLOCKS == 2u
            const uint32_t nwin = n > 16u * tb ? (n - 16u * tb) / 32u : 0u;     // windows ahead with 16 * block + 15 < n for both blocks
            if (g >= g_lo && nwin > 0u) {
                // byte offsets from the pair's workspace: the checkpoint of window g (this lane's column of it), the maximum
                // of window g - 1 (stored one pass late; the first pass stores nothing); from the reference image: block tb
                uint32_t cko = (g * (uint32_t)(R + 2) * WAVE + lane) * 4u;
                uint32_t wmo = ((uint32_t)G.wmax_off + g - 1u) * 4u;
                uint32_t rfo = tb * 16u;
                const uint32_t lact_s = uni(lact);
                int wm_last;
                uint32_t wx = wnext.x, wy = wnext.y, wz = wnext.z, ww = wnext.w;
                SweepWindowAsm<R>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, wx, wy, wz, ww, one, gm, S.lmax, wm_last, steady_max,
                                       cko, wmo, rfo, uni64((uint64_t)(uintptr_t)(A.dir + pd.dir_off)), uni64((uint64_t)(uintptr_t)refq),
                                       lact_s >= WAVE ? ~0ull : (1ull << lact_s) - 1ull, uni(nwin - 1u));
                wnext = make_uint4(wx, wy, wz, ww);       // the block after the last steady window
                // the last window's maximum is still one value per lane (already without the lanes that hold no rows)
                const int wm = wave_max_i32(wm_last);
                if (lane == 0) A.dir[pd.dir_off + G.wmax_off + g + nwin - 1u] = (uint32_t)wm;
                tb += 2u * nwin - 1u;
                closed = true;
                continue;
            }
#endif
            if (g >= g_lo) {
                // checkpoint in the layout the replay expects: H of the rows, the N received one step earlier, the
                // reference operand of the last step ([ck][slot][lane], 256 B stores)
                uint32_t *__restrict__ ck = wsp + (uint64_t)g * (R + 2) * WAVE;
#pragma unroll
                for (int k = 0; k < R; ++k) ck[k * WAVE] = (uint32_t)S.h[k];
                ck[R * WAVE] = (uint32_t)wave_shr1_zero(S.g[R - 1]);
                ck[(R + 1) * WAVE] = (uint32_t)S.rby;
            }
        }
        const uint4 w = wnext;                            // base codes of (local) columns 16tb+1 .. 16tb+16
        wnext = refq[tb + 1];                             // prefetch (images are padded)
        const uint32_t t0 = 16u * tb;
#ifndef SWMI_NO_ASM
        if (t0 + 15u < n) {
            // lane 0 stays inside the reference for all 16 steps: nobody has to be masked (a lane that has not started
            // yet computes zeros from its zero operands, lanes without rows compute values nobody reads)
            SweepStep4Asm<R>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.x, w.y, one, gm, S.lmax);
            SweepStep4Asm<R>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.y, w.z, one, gm, S.lmax);
            SweepStep4Asm<R>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.z, w.w, one, gm, S.lmax);
            SweepStep4Asm<R>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.w, wnext.x, one, gm, S.lmax);
        } else
#endif
        {
            sweep_tail_block<R>(S, w, wnext.x, t0, lane_eff, n, one, gm);
        }
    }
    if (!closed) {
        const uint32_t gl = (nblk - 1u + (col0 >> 4)) / SWMI_CK_BLOCKS;
        if (gl >= g_lo) close_window(gl);
    }
    {
        const int sm = wave_max_i32(steady_max);
        pair_max = pair_max > sm ? pair_max : sm;
    }
    if (lane != 0) return;
    if (A.dbg) {      // diagnostics: where the wave ran (HW_ID: wave, SIMD, CU, SE ...) and how long
        A.dbg[2 * pd.out_id] = (unsigned long long)__builtin_amdgcn_s_getreg((4 /*HW_REG_HW_ID*/) | (0 << 6) | (31 << 11)) |
                               ((unsigned long long)__builtin_amdgcn_s_getreg((20 /*HW_REG_XCC_ID*/) | (0 << 6) | (31 << 11)) << 32);
        A.dbg[2 * pd.out_id + 1] = __builtin_amdgcn_s_memtime() - dbg_t0;
    }
    PairOut *o = &A.out[pd.out_id];
    if (COLS) {
        // combine the chunks: ONE atomicMax each (the record was zeroed by sw_sweep_winmax_kernel, one launch earlier) and
        // nothing else -- no completion count, no fence: a fence here writes back the XCD's L2, full of the checkpoints just
        // stored, and cost every chunk's launch ~30 us (profiles/r02/col_chunks.md).  The traceback kernels, one launch
        // later, read the final maximum and mark the pair degenerate when it is 0 (finish_pair).
        if (pair_max > 0) atomicMax(&o->score, pair_max);
        return;
    }
    PairOut v;                 // the cells holding the maximum are listed by the traceback kernel (n_cells follows there)
    if (pair_max <= 0) { v.score = 0; v.flags = SWMI_F_DEGENERATE; v.n_cells = (uint64_t)m * n_full; }
    else               { v.score = pair_max; v.flags = 0u; v.n_cells = 0; }
    *o = v;
}

template <bool COLS>
__device__ __forceinline__ void sweep_fast_dispatch(const FillArgs &A, const PairDesc pd, uint32_t lane, uint32_t m, const ColItem ci) {
    const uint32_t R = swmi_rows_per_lane(m);
    if (R == 1)      sweep_fast<1, COLS>(A, pd, lane, ci);
    else if (R == 2) sweep_fast<2, COLS>(A, pd, lane, ci);
    else if (R == 3) sweep_fast<3, COLS>(A, pd, lane, ci);
    else             sweep_fast<4, COLS>(A, pd, lane, ci);
}

template <bool ACGT, bool STRICT, int MODE>
__device__ __forceinline__ void fill_dispatch(const FillArgs &A, const PairDesc pd, uint32_t lane, uint32_t m) {
    const uint32_t R = swmi_rows_per_lane(m);
    if (R == 1)      fill_pair<1, ACGT, STRICT, false, MODE>(A, pd, lane);
    else if (R == 2) fill_pair<2, ACGT, STRICT, false, MODE>(A, pd, lane);
    else if (R == 3) fill_pair<3, ACGT, STRICT, false, MODE>(A, pd, lane);
    else if (m <= WAVE * SWMI_RMAX) fill_pair<SWMI_RMAX, ACGT, STRICT, false, MODE>(A, pd, lane);
    else             fill_pair<SWMI_RMAX, ACGT, STRICT, true, MODE>(A, pd, lane);
}

template <int MODE>
__device__ __forceinline__ void fill_entry(const FillArgs &A) {
    const uint32_t pair = blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);
    if (pair >= A.n_pairs) return;
    const uint32_t lane = threadIdx.x & 63u;
    if (pair == 0 && lane == 0 && A.hdr) { A.hdr->reserved = 0; A.hdr->pad = 0; }   // arena reset for the traceback kernel that follows
    if (pair == 0 && lane == 0 && A.q_reset) *A.q_reset = 0u;                        // ... and the split traceback's item counter
    const PairDesc pd = A.pairs[pair];
    if (MODE == SWMI_MODE_WINMAX && (pd.pad & SWMI_PAD_RESIDENT)) return;            // sw_resident_pairs_kernel does the whole pair
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    if (MODE == SWMI_MODE_WINMAX && A.skip_multi && qd.len > WAVE * SWMI_RMAX) {
        // swept strip by strip (sw_sweep_winmax_strips_kernel, next launch): start the record its strips complete by atomics
        if (lane == 0) { PairOut z; z.score = 0; z.flags = 0u; z.n_cells = 0; A.out[pd.out_id] = z; }
        return;
    }
    // profile lookup needs both sequences pure ACGT and scores that fit a signed byte
    const bool acgt = rd.acgt && qd.acgt &&
                      SWMI_SCORES_FIT(A);
    if (MODE == SWMI_MODE_WINMAX && qd.len <= WAVE * SWMI_RMAX && (pd.pad & SWMI_PAD_COLS)) {
        // swept chunk by chunk (sw_sweep_winmax_cols_kernel, next launch): start the record its chunks complete by atomics
        if (lane == 0) { PairOut z; z.score = 0; z.flags = 0u; z.n_cells = 0; A.out[pd.out_id] = z; }
        return;
    }
    if (MODE == SWMI_MODE_WINMAX && acgt && qd.len <= WAVE * SWMI_RMAX && A.gap <= 0) {
        sweep_fast_dispatch<false>(A, pd, lane, qd.len, ColItem{0u, 0u, 0u, 0u});
        return;
    }
    if (MODE == SWMI_MODE_SCORE || MODE == SWMI_MODE_WINMAX) {   // scores do not depend on the tie order
        if (acgt) fill_dispatch<true, false, MODE>(A, pd, lane, qd.len);
        else      fill_dispatch<false, false, MODE>(A, pd, lane, qd.len);
    } else if (acgt) {
        if (A.strict) fill_dispatch<true, true, MODE>(A, pd, lane, qd.len);
        else          fill_dispatch<true, false, MODE>(A, pd, lane, qd.len);
    } else {
        if (A.strict) fill_dispatch<false, true, MODE>(A, pd, lane, qd.len);
        else          fill_dispatch<false, false, MODE>(A, pd, lane, qd.len);
    }
}

extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES)
sw_fill_kernel(const FillArgs A) { fill_entry<SWMI_MODE_FIELD>(A); }

extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES)
sw_fill_score_kernel(const FillArgs A) { fill_entry<SWMI_MODE_SCORE>(A); }

// (at most 128 VGPRs -- 14 spills, none in the fast stream: with two batches in flight this kernel's wavefront shares its SIMD
//  with the other batch's traceback wavefronts, 128 VGPRs each: three of them fit beside it, at 137 only two.  Two in flight
//  0.124 -> 0.119 ms per step, one at a time 0.1655 -> 0.167: profiles/r03/ab_sweep_128vgpr_after_lds.txt)
extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES) __attribute__((amdgpu_waves_per_eu(4, 4)))
sw_sweep_winmax_kernel(const FillArgs A) { fill_entry<SWMI_MODE_WINMAX>(A); }

// mode 1, reads of several strips: one wavefront per (pair, strip).  The items are ordered so that a strip's producer
// (the strip above it) sits in the same or an earlier workgroup, i.e. is never dispatched later than its consumer.
extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES)
sw_sweep_winmax_strips_kernel(const FillArgs A) {
    const uint32_t item = blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);
    if (item >= A.n_strip_items) return;
    const uint32_t lane = threadIdx.x & 63u;
    const StripItem *it = A.strip_items + item;
    const PairDesc pd = A.pairs[it->pair];
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const bool acgt = rd.acgt && qd.acgt &&
                      SWMI_SCORES_FIT(A);
    const uint32_t strip = __builtin_amdgcn_readfirstlane(it->strip);     // wave-uniform: "does this strip feed a seam" stays scalar
    if (acgt) fill_pair<SWMI_RMAX, true, false, true, SWMI_MODE_WINMAX, true>(A, pd, lane, strip, it);
    else      fill_pair<SWMI_RMAX, false, false, true, SWMI_MODE_WINMAX, true>(A, pd, lane, strip, it);
}

// mode 1, few pairs with long references: one wavefront per COLUMN CHUNK of a pair (swmi_device.h: ColItem).  The
// chunks of a pair are independent -- each re-derives its left context from a halo no positive-score path can span --
// so a 128 kbp reference against one read is swept by dozens of wavefronts at once instead of one 128 k-step chain.
extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES)
sw_sweep_winmax_cols_kernel(const FillArgs A) {
    const uint32_t item = blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);
    if (item >= A.n_col_items) return;
    const uint32_t lane = threadIdx.x & 63u;
    const ColItem ci = A.col_items[item];
    const PairDesc pd = A.pairs[ci.pair];
    sweep_fast_dispatch<true>(A, pd, lane, A.reads[pd.read_id].len, ci);
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers (the runtime in swmi_run.cpp is plain C++)
// ------------------------------------------------------------------------------------------------
// Small launches: the dispatcher may stack several workgroups on one CU while other CUs stay empty (measured: 250
// workgroups of the 67-VGPR column-chunk kernel ran two to a CU, each wave sharing its SIMD, 1.5x slower per step).  A
// dynamic-LDS request nobody uses caps the workgroups a CU can hold at what an even spread needs, so the launch is dealt
// over all 256 CUs.  SWMI_LDS_SPREAD=0 switches it off.
static size_t spread_lds(uint32_t n_groups) {
    static const int on = getenv("SWMI_LDS_SPREAD") ? atoi(getenv("SWMI_LDS_SPREAD")) : 1;
    if (!on || n_groups == 0 || n_groups > 4u * 256u) return 0;
    const uint32_t per_cu = (n_groups + 255u) / 256u;                      // workgroups a CU must take
    // per_cu fit, per_cu + 1 do not -- and no more than that needs: the rest of the CU's LDS stays free for the kernels of
    // ANOTHER batch in flight on the same GPU (a sweep that reserved the whole 160 KB kept the other batch's traceback
    // workgroups off its CU: 0.130 ms per step with two batches in flight, 0.119 without the reservation)
    return ((size_t)(160u * 1024u) / (per_cu + 1u) / 1024u + 1u) * 1024u;
}

// ev_start / ev_stop (both or none): the launch is ONE kernel and the events take its start and stop times from the dispatch
// itself (hipExtLaunchKernelGGL) -- no marker packets between the kernels of a run, which hipEventRecord would put there
extern "C" hipError_t swmi_launch_fill(const FillArgs *a, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (a->n_pairs == 0) return hipSuccess;
    static const bool attrs = [] {
        swmi_allow_big_lds(sw_fill_kernel); swmi_allow_big_lds(sw_fill_score_kernel); swmi_allow_big_lds(sw_sweep_winmax_kernel);
        swmi_allow_big_lds(sw_sweep_winmax_strips_kernel); swmi_allow_big_lds(sw_sweep_winmax_cols_kernel);
        return true;
    }();
    (void)attrs;
    const dim3 grid((a->n_pairs + FILL_WAVES - 1) / FILL_WAVES), block(WAVE * FILL_WAVES);
    const size_t lds = spread_lds(grid.x);
    if (a->mode == 0)      hipLaunchKernelGGL(sw_fill_kernel, grid, block, lds, st, *a);
    else if (a->mode == 1) {
        if (ev_start && ev_stop && !(a->skip_multi && a->n_strip_items) && !a->n_col_items) {
            hipExtLaunchKernelGGL(sw_sweep_winmax_kernel, grid, block, (uint32_t)lds, st, ev_start, ev_stop, 0u, *a);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(sw_sweep_winmax_kernel, grid, block, a->n_col_items || a->n_strip_items ? 0 : lds, st, *a);
        if (a->skip_multi && a->n_strip_items) {
            const uint32_t g = (a->n_strip_items + FILL_WAVES - 1) / FILL_WAVES;
            hipLaunchKernelGGL(sw_sweep_winmax_strips_kernel, dim3(g), block, spread_lds(g), st, *a);
        }
        if (a->n_col_items) {
            const uint32_t g = (a->n_col_items + FILL_WAVES - 1) / FILL_WAVES;
            hipLaunchKernelGGL(sw_sweep_winmax_cols_kernel, dim3(g), block, spread_lds(g), st, *a);
        }
    }
    else                   hipLaunchKernelGGL(sw_fill_score_kernel, grid, block, lds, st, *a);
    return hipGetLastError();
}
