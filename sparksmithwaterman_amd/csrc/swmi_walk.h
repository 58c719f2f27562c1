// swmi_walk.h -- what the per-pair and the split traceback kernels (swmi_traceback.hip) share: the re-sweep of a
// checkpoint window (replay_*), the listing of a pair's maximum cells (detect_cells) and the walk of its alignments
// (traceback_pair).  Device code only; everything is __forceinline__.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "swmi_device.h"
#include "swmi_emit.h"
#include "swmi_cells.h"

#ifndef SWMI_HELPER_SLEEP
#define SWMI_HELPER_SLEEP 8          // x 64 cycles between two polls of an idle helper wavefront of the traceback (measured: profiles/r02/ab_helper_sleep.txt)
#endif

// ------------------------------------------------------------------------------------------------
// traceback: SWMI_TB_SLOTS wavefronts per pair (slot x walks the tied cells x, x+SLOTS, ...).
//
// The walk is a chain of dependent 2-bit lookups; straight from HBM that is ~1 us per step, and even from
// LDS a one-cell-at-a-time scalar walk costs ~100 instruction issues per step.  So:
//  * the wave brings a TILE of the direction field -- every cell whose anti-diagonal step lies in a window
//    of 16-step blocks, all 64*R row slots of the strip -- into LDS, plus the matching window of reference
//    codes and the whole read.  Mode 0 copies it from the HBM direction field (16 blocks, coalesced 256 B
//    loads, all in flight at once); mode 1 RE-SWEEPS SWMI_CK_BLOCKS blocks from the lane-state checkpoint the
//    score-only fill left behind, this time with the direction bits (the same instruction stream as the
//    mode-0 fill), which is cheaper than having every pair pay 4 more VALU per cell in the fill;
//  * it then advances by RUNS: lane x looks at the cell x steps up the current diagonal, a ballot gives the
//    length of the run of "alignment" moves, a second ballot over per-lane prefix scores finds where the
//    tracked score H(pred) = H - s(ref,read) would reach 0 (`while (score > 0)`, SmithWaterman.java:380), and
//    the whole run is emitted at once.  Gap moves (insertion / deletion) are taken one at a time.
// ------------------------------------------------------------------------------------------------
#define SWMI_TB_SLOTS 4u
#if SWMI_CK_BLOCKS > 2
#define SWMI_TB_WAVES 4u            // (64-step windows: a team's span of 4 windows is what the reference-window staging holds)
#else
#define SWMI_TB_WAVES 8u            // mode 1: most waves per workgroup (= per pair) of the traceback kernel; the launcher picks 4 or 8
#endif

// The same re-sweep for the usual pair (fast symbols, one strip, gap <= 0), from the shorter instruction stream of
// tools/gen_step.py (DirStep4Asm: the 3-VALU cell + two compares feeding v_addc, neighbour exchange inside the arithmetic;
// 25 instructions per step at R = 3 instead of ~30).  No lane is masked: a lane outside its column range computes bits
// nobody reads, and because every step pushes exactly one bit pair the bits of the real steps sit where the walk expects them.
template <int R, bool STRICT>
__device__ __forceinline__ void replay_window_fast(const TraceArgs &A, const PairDesc pd, const uint32_t n, const uint32_t m,
                                                   const uint32_t *__restrict__ refw, const uint32_t *__restrict__ readw,
                                                   const uint32_t wlo, const uint32_t lane, uint32_t *__restrict__ lds_tile) {
    const uint32_t gm = (uint32_t)(-(int64_t)A.gap);
    const int one = 1;
    int h[R], g[R], hp[R], q[R];
    uint32_t acc[R];
    const uint32_t *__restrict__ ck = A.dir + pd.dir_off + (uint64_t)(wlo / SWMI_CK_BLOCKS) * (R + 2) * WAVE + lane;
    build_profiles<R>(q, readw, lane * R, m, A.match, A.mismatch);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        h[k] = (int)ld_l2(ck + k * WAVE);
        hp[k] = (uint32_t)h[k] > gm ? (int)((uint32_t)h[k] - gm) : 0;
        g[k] = 0;
        acc[k] = 0;
    }
    // the checkpoint holds, per lane, the N it received one step earlier (= NW of its row 0 now); the stream takes that value
    // from the lane above, out of its ping-pong set: hand it back up (wave_shl:1)
    const int nprev = (int)ld_l2(ck + R * WAVE);
    g[R - 1] = __builtin_amdgcn_update_dpp(0, nprev, 0x130 /*wave_shl:1*/, 0xf, 0xf, true);
    const int rb_ck = (int)ld_l2(ck + (R + 1) * WAVE);
    const uint32_t lact = m >= WAVE * R ? WAVE : (m + R - 1) / R;
    const uint32_t T = n + lact - 1, nblk = (T + 15u) / 16u;
    const uint4 *__restrict__ refq = reinterpret_cast<const uint4 *>(refw);
    uint4 wv[SWMI_CK_BLOCKS + 1];
#pragma unroll
    for (uint32_t b = 0; b <= SWMI_CK_BLOCKS; ++b) wv[b] = refq[wlo + b];          // images are padded past the last block
    int rbx = wave_shr1((int)(1u << (wv[0].x & 31u)), rb_ck), rby = rb_ck;
#pragma unroll
    for (uint32_t b = 0; b < SWMI_CK_BLOCKS; ++b) {
        if (wlo + b >= nblk) break;
        const uint4 w = wv[b];
        DirStep4Asm<R, STRICT>::run(h, g, hp, acc, q, rbx, rby, w.x, w.y, one, gm);
        DirStep4Asm<R, STRICT>::run(h, g, hp, acc, q, rbx, rby, w.y, w.z, one, gm);
        DirStep4Asm<R, STRICT>::run(h, g, hp, acc, q, rbx, rby, w.z, w.w, one, gm);
        DirStep4Asm<R, STRICT>::run(h, g, hp, acc, q, rbx, rby, w.w, wv[b + 1].x, one, gm);
#pragma unroll
        for (int k = 0; k < R; ++k) lds_tile[(b * R + k) * WAVE + lane] = acc[k];
    }
}

// re-sweep the window of SWMI_CK_BLOCKS blocks that starts at block `wlo` of strip `s` into lds_tile.
// DETECT: also append the window's cells equal to `maxv` to the pair's cell list; returns the new list length.
template <int R, bool ACGT, bool STRICT, bool MULTI, bool DETECT>
__device__ __forceinline__ uint32_t replay_window(const TraceArgs &A, const PairDesc pd, const uint32_t n, const uint32_t m,
                                                  const uint32_t *__restrict__ refw, const uint32_t *__restrict__ readw,
                                                  const StripGeom G, const uint32_t s, const uint32_t wlo,
                                                  const uint32_t lane, uint32_t *__restrict__ lds_tile,
                                                  const int maxv, const uint32_t cnt_in, uint2 *__restrict__ cells, const uint32_t ccap) {
#ifndef SWMI_NO_ASM
    if constexpr (ACGT && !MULTI && !DETECT) {
        if (A.gap <= 0 && s == 0u) {
            replay_window_fast<R, STRICT>(A, pd, n, m, refw, readw, wlo, lane, lds_tile);
            return cnt_in;
        }
    }
#endif
    constexpr int BM = DETECT ? SWMI_MODE_DETECT : SWMI_MODE_REPLAY;
    FillState<R> S;
    S.thr = DETECT ? maxv : 0x7FFFFFFF; S.cnt = cnt_in; S.ev_prev = 0; S.events = 0; S.dbg_skip = false; S.lmax = -1;
    const uint32_t row0 = s * G.rps + lane * R;
    const uint32_t rows_left = m - s * G.rps;
    const uint32_t lact = rows_left >= G.rps ? WAVE : (rows_left + R - 1) / R;
    const uint32_t T = n + lact - 1;
    const uint32_t lane_eff = lane < lact ? lane : 0x40000000u;
    setup_rows<R, ACGT>(S, readw, row0, m, A.match, A.mismatch);
    const uint32_t *__restrict__ ck = A.dir + pd.dir_off + s * G.strip_words +
                                      (uint64_t)(wlo / SWMI_CK_BLOCKS) * (R + 2) * WAVE + lane;
#pragma unroll
    for (int k = 0; k < R; ++k) S.h[k] = (int)ld_l2(ck + k * WAVE);
    S.nprev = (int)ld_l2(ck + R * WAVE);
    S.rb = (int)ld_l2(ck + (R + 1) * WAVE);
    const int32_t *seam_in = nullptr;
    if (MULTI) seam_in = A.seam + pd.seam_off + (uint64_t)(s > 0 ? s - 1 : 0) * (n + 1);
    const bool reads_seam = MULTI && (s > 0);
    const uint32_t nblk = (T + 15u) / 16u;
    const uint4 *__restrict__ refq = reinterpret_cast<const uint4 *>(refw);
    uint4 wv[SWMI_CK_BLOCKS];                                  // the window's base codes: all loads in flight at once
#pragma unroll
    for (uint32_t b = 0; b < SWMI_CK_BLOCKS; ++b) wv[b] = refq[wlo + b];     // images are padded past nblk
#pragma unroll
    for (uint32_t b = 0; b < SWMI_CK_BLOCKS; ++b) {
        const uint32_t tb = wlo + b;
        if (tb >= nblk) break;
        const uint4 w = wv[b];
        const uint32_t t0 = 16u * tb;
        int seamv = 0;
        if (reads_seam) {
            const uint32_t col = t0 + 1u + (lane & 15u);
            seamv = col <= n ? (int)ld_l2((const uint32_t *)seam_in + col) : 0;
        }
        const bool steady = (t0 + 1u >= lact) && (t0 + 15u < n);
        if (steady)
            fill_block16<R, ACGT, STRICT, MULTI, false, BM>(S, w, t0, lane, lane_eff, n, m, row0, A.gap, A.match, A.mismatch,
                                                            seamv, reads_seam, false, nullptr, cells, ccap);
        else
            fill_block16<R, ACGT, STRICT, MULTI, true, BM>(S, w, t0, lane, lane_eff, n, m, row0, A.gap, A.match, A.mismatch,
                                                           seamv, reads_seam, false, nullptr, cells, ccap);
        const int miss = (int)(t0 + 15u) - ((int)(lane + n) - 1);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            uint32_t v = S.acc[k];
            if (miss > 0 && miss < 16) v <<= 2 * miss;
            lds_tile[(b * R + k) * WAVE + lane] = v;
        }
    }
    return S.cnt;
}

template <int R, bool MULTI, bool DETECT>
__device__ __forceinline__ uint32_t replay_dispatch(const TraceArgs &A, const PairDesc pd, uint32_t n, uint32_t m, bool acgt,
                                                    const uint32_t *__restrict__ refw, const uint32_t *__restrict__ readw,
                                                    const StripGeom G, uint32_t s, uint32_t wlo, uint32_t lane, uint32_t *lds_tile,
                                                    int maxv, uint32_t cnt_in, uint2 *__restrict__ cells, uint32_t ccap) {
    if (acgt) {
        if (A.strict) return replay_window<R, true, true, MULTI, DETECT>(A, pd, n, m, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
        else          return replay_window<R, true, false, MULTI, DETECT>(A, pd, n, m, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
    } else {
        if (A.strict) return replay_window<R, false, true, MULTI, DETECT>(A, pd, n, m, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
        else          return replay_window<R, false, false, MULTI, DETECT>(A, pd, n, m, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
    }
}

// A pair swept by several wavefronts (column chunks, strips) reaches the mode-1 traceback with only its maximum combined:
// a maximum of 0 is the degenerate case -- every one of the m*n cells ties (SmithWaterman.java:154,182-185).  (A pair swept
// by one wavefront was marked by it.)  Returns true if `po` was completed here.
__device__ __forceinline__ bool finish_pair(const TraceArgs &A, const PairDesc pd, PairOut &po) {
    if (po.score > 0 || (po.flags & SWMI_F_DEGENERATE)) return false;
    po.score = 0;
    po.flags = SWMI_F_DEGENERATE;
    po.n_cells = (uint64_t)A.reads[pd.read_id].len * A.refs[pd.ref_id].len;
    return true;
}

// true for the pairs the full-featured mode-1 traceback handles: pure ACGT with int8 scores, the serial tie order
__device__ __forceinline__ bool swmi_common_pair(const TraceArgs &A, const SeqDesc rd, const SeqDesc qd) {
    return rd.acgt && qd.acgt && SWMI_SCORES_FIT(A) && !A.strict;
}

// re-sweeps one window.  FULL: any variant (byte alphabet, DistributedSW tie order, several strips); otherwise only the
// common one -- the call sites of the team code are many, and every variant inlined at each of them is what made this
// file take six minutes to compile.
template <int R, bool DETECT, bool FULL = true>
__device__ __forceinline__ uint32_t replay_any(const TraceArgs &A, const PairDesc pd, uint32_t n, uint32_t m, bool acgt,
                                               const uint32_t *__restrict__ refw, const uint32_t *__restrict__ readw,
                                               const StripGeom G, uint32_t s, uint32_t wlo, uint32_t lane, uint32_t *lds_tile,
                                               int maxv, uint32_t cnt_in, uint2 *__restrict__ cells, uint32_t ccap) {
    if constexpr (!FULL) {
        if constexpr (R == SWMI_RMAX) {
            if (m > WAVE * SWMI_RMAX)          // a read of several strips
                return replay_window<R, true, false, true, DETECT>(A, pd, n, m, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
        }
        return replay_window<R, true, false, false, DETECT>(A, pd, n, m, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
    }
    if constexpr (R == SWMI_RMAX) {
        if (m > WAVE * SWMI_RMAX)
            return replay_dispatch<R, true, DETECT>(A, pd, n, m, acgt, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
    }
    return replay_dispatch<R, false, DETECT>(A, pd, n, m, acgt, refw, readw, G, s, wlo, lane, lds_tile, maxv, cnt_in, cells, ccap);
}

// mode 1: list the pair's maximum cells.  The sweep left one maximum per checkpoint window; every window whose
// maximum equals the pair's is re-swept once with the cell test switched on.
template <int R, bool FULL = true>
__device__ __forceinline__ uint32_t detect_cells(const TraceArgs &A, const PairDesc pd, const PairOut po,
                                                 const uint32_t lane, uint32_t *__restrict__ lds_tile) {
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const StripGeom G = strip_geom<R>(m, n, 1u);
    const bool acgt = rd.acgt && qd.acgt && SWMI_SCORES_FIT(A);
    const uint64_t cbase = A.cells_off ? A.cells_off[pd.out_id] : (uint64_t)pd.out_id * A.cell_cap;
    const uint32_t ccap = A.cells_cap ? A.cells_cap[pd.out_id] : A.cell_cap;
    uint2 *__restrict__ cells = const_cast<uint2 *>(A.cells) + cbase;
    uint32_t cnt = 0;
    for (uint32_t s = 0; s < G.n_strips; ++s) {
        const uint32_t *__restrict__ wm = A.dir + pd.dir_off + s * G.strip_words + G.wmax_off;
        for (uint32_t g0 = 0; g0 < G.n_ck; g0 += WAVE) {
            const uint32_t g = g0 + lane;
            const int wv = g < G.n_ck ? (int)wm[g] : -1;
            uint64_t cand = BALLOT(wv == po.score);
            while (cand) {
                const uint32_t gg = g0 + (uint32_t)__builtin_ctzll(cand);
                cand &= cand - 1ull;
                cnt = replay_any<R, true, FULL>(A, pd, n, m, acgt, refw, readw, G, s, gg * SWMI_CK_BLOCKS, lane, lds_tile,
                                          po.score, cnt, cells, ccap);
            }
        }
    }
    return cnt;
}

// COOP (mode 1): the workgroup's waves form `nslots` teams of `ts` waves, one walker (this function) plus ts-1
// helpers (coop_helper below) each.  Instead of re-sweeping one 32-step window at a time, the walker publishes a
// request for up to ts consecutive windows, the team re-sweeps them in parallel into the team's tile, and the walker
// then crosses the whole 32*ts-step span without stopping.  The teams of a workgroup run independently of each other:
// a request is a sequence number in LDS the helpers poll (s_sleep between polls), completion a counter the walker polls;
// there is no workgroup barrier after the cell list.
// shared[]: [0] number of maximum cells, [4+4t ..] team t's request {strip, first block, windows, sequence number
// (~0: the walker is done)}, [20+t] windows team t's helpers have delivered so far.
// Per-pair diagnostics of the traceback (ticks of the walk and of the stagings, iterations, steps: SWMI_DEBUG_FILL=1) are compiled
// in only with -DSWMI_TB_DIAG (make KFLAGS=-DSWMI_TB_DIAG): their counters lived in registers across the whole walk of a kernel
// that sits at its 128-VGPR limit with spills.
#ifdef SWMI_TB_DIAG
#define TB_DBG (A.dbg != nullptr)
#else
#define TB_DBG false
#endif
template <int R, int TMODE, bool COOP, bool FULL = true>
__device__ __forceinline__ void traceback_pair(const TraceArgs &A, const PairDesc pd, const PairOut po,
                                               const uint32_t lane, const uint32_t slot, const uint32_t nslots,
                                               uint32_t *__restrict__ lds, uint32_t *__restrict__ lds_tile,
                                               volatile uint32_t *__restrict__ shared, const uint32_t ts,
                                               uint32_t pre_wlo = 0xFFFFFFFFu, const bool read_staged = false,
                                               const uint4 *__restrict__ one = nullptr, uint32_t *__restrict__ lds_tile_alt = nullptr) {
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const StripGeom G = strip_geom<R>(m, n, A.mode);
    const uint32_t rps = G.rps;
    const uint32_t *__restrict__ dirp = A.dir + pd.dir_off;
    const uint32_t umat = (uint32_t)A.match, umis = (uint32_t)A.mismatch, ugap = (uint32_t)A.gap;
    const int dec0 = A.match > A.mismatch ? A.match : A.mismatch;
    // The walk's shortcuts compare the score with up to 2 gap and 21 alignment moves' worth of these two.  With scores so large
    // that such a product could pass 2^31 both become 2^32 - 1: k moves' worth is then 2^32 - k (mod 2^32, 1 <= k <= 23), above
    // every score in the unsigned compares below, so the shortcuts are off and every move is checked
    // (tests/test_gpu_parity.py::test_scores_that_wrap).
    const bool dec_fits = dec0 <= 0x7FFFFFFF / 23 && A.gap <= 0x7FFFFFFF / 23;
    const uint32_t udec = !dec_fits ? 0xFFFFFFFFu : dec0 > 0 ? (uint32_t)dec0 : 0u;    // the most one alignment move can lower the tracked score
    const uint32_t ugdec = !dec_fits ? 0xFFFFFFFFu : A.gap > 0 ? (uint32_t)A.gap : 0u;  // ... and one gap move
    (void)udec; (void)ugdec;                                  // (the -DSWMI_WALK_CHASE build of the walk does not use them)
    const bool acgt = rd.acgt && qd.acgt && SWMI_SCORES_FIT(A);
    // the caller's own bytes of the two sequences (for the aligned strings; loaded here, long before they are needed)
    const uint8_t *__restrict__ raw_ref = A.raw ? A.raw + A.raw_off[pd.ref_id] : nullptr;
    const uint8_t *__restrict__ raw_read = A.raw ? A.raw + A.raw_off[A.raw_reads_at + pd.read_id] : nullptr;

    // (s_setprio for the walker over the helpers sharing its SIMD: measured, no effect)
    uint32_t *lds_ops = lds;                                   // [A.lds_words]      one op per BYTE, staged per alignment
    uint32_t *lds_read = lds_ops + A.lds_words;                // [A.lds_read_words] the read's codes
    uint32_t *lds_ref = lds_read + A.lds_read_words;           // [SWMI_TB_REFWIN_WORDS]
    uint8_t *ops_b = reinterpret_cast<uint8_t *>(lds_ops);
    const uint8_t *read_b = reinterpret_cast<const uint8_t *>(lds_read);
    const uint8_t *ref_b = reinterpret_cast<const uint8_t *>(lds_ref);
    uint32_t req_seq = 0, req_expected = 0;                    // COOP: requests published / windows expected back so far
    // COOP with a second tile buffer (lds_tile_alt): SPECULATIVE staging.  A path only ever moves towards smaller steps, so
    // the span the walk will need next is the one just before the current one: the team's helpers re-sweep it into the other
    // buffer WHILE the walker walks, and the walker finds it ready when it crosses the boundary (it swaps buffers instead of
    // waiting ~7 k cycles for a re-sweep).  A span whose walk ends early costs the helpers -- otherwise idle -- one re-sweep.
    uint32_t *tile_cur = lds_tile, *tile_alt = lds_tile_alt;
    uint32_t spec_wlo = 0xFFFFFFFFu, spec_hi = 0u, spec_rv0 = 0u, spec_rv1 = 0u;
    auto team_wait = [&]() {                                   // every window requested so far has been delivered
        while (__hip_atomic_load(const_cast<uint32_t *>(&shared[20u + slot]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < req_expected)
            __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    // request {flags: bit 0 = buffer (0: the team's first, 1: its second), bit 1 = the walker takes no window of it, bits 2.. =
    // the strip; first block; windows}; the helpers poll the sequence number (coop_helper)
    auto team_request = [&](uint32_t flags, uint32_t first_block, uint32_t nq, uint32_t delivered) {
        ++req_seq;
        req_expected += delivered;
        if (lane == 0) {
            shared[4u + 4u * slot] = flags; shared[5u + 4u * slot] = first_block; shared[6u + 4u * slot] = nq;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_store(const_cast<uint32_t *>(&shared[7u + 4u * slot]), req_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };

    const unsigned long long tk0 = TB_DBG ? __builtin_amdgcn_s_memtime() : 0ull;
    unsigned long long tk_walk = 0, tk_stage = 0, n_steps = 0, n_iters = 0;
    if (!read_staged)
        for (uint32_t w = lane; w < (m + 3u) / 4u; w += WAVE) lds_read[w] = readw[w];

    const uint64_t cbase = A.cells_off ? A.cells_off[pd.out_id] : (uint64_t)pd.out_id * A.cell_cap;
    const uint32_t ncell = one ? 1u : (uint32_t)po.n_cells;          // `one`: walk just this cell (split traceback)
    const uint2 *__restrict__ cells = A.cells + cbase;

    // The tied cells are processed in list order; `rank` is the position the reference would list the cell
    // at: row-major (SmithWaterman.java:157-185) or per anti-diagonal, ascending j (DistributedSW.java:209-239).
    for (uint32_t base = 0; base < ncell; base += WAVE) {
        const uint32_t idx = base + lane;
        uint2 mine = make_uint2(0, 0);
        if (one) { mine.x = one->y; mine.y = one->z; }
        else if (idx < ncell) { mine.x = ld_l2(&cells[idx].x); mine.y = ld_l2(&cells[idx].y); }
        const uint64_t mykey = A.strict ? (((uint64_t)(mine.x + mine.y) << 32) | mine.y)
                                        : (((uint64_t)mine.x << 32) | mine.y);
        // (a pair with more tied cells than one wave of lanes: every lane comparing its cell with all others is O(cells^2)
        //  global loads per walker -- 1600 cells on a 128 kbp periodic reference -- so the host orders those records by cell)
        uint32_t rank = (one || ncell > WAVE) ? SWMI_RANK_BY_CELL : 0u;
        if (ncell > 1 && ncell <= WAVE) {
            for (uint32_t o = 0; o < ncell; ++o) {
                uint2 c; c.x = ld_l2(&cells[o].x); c.y = ld_l2(&cells[o].y);
                const uint64_t kk = A.strict ? (((uint64_t)(c.x + c.y) << 32) | c.y) : (((uint64_t)c.x << 32) | c.y);
                rank += (kk < mykey) ? 1u : 0u;
            }
        }
        const uint32_t nhere = ncell - base < WAVE ? ncell - base : WAVE;

        for (uint32_t a = slot; a < nhere; a += nslots) {
            const uint32_t ci = __builtin_amdgcn_readlane((int)mine.x, a);
            const uint32_t cj = __builtin_amdgcn_readlane((int)mine.y, a);
            const uint32_t crank = __builtin_amdgcn_readlane((int)rank, a);

            // ---- walk, SmithWaterman.java:380-409; (i, j, score, n_ops, begin) are wave-uniform ----
            uint32_t i = ci, j = cj;
            uint32_t score = (uint32_t)po.score;
            uint32_t n_ops = 0;
            int begin = 0;
            while ((int)score > 0 && i != 0u && j != 0u) {     // (a positive score at row/column 0 cannot happen with consistent
                const unsigned long long ts0 = TB_DBG ? __builtin_amdgcn_s_memtime() : 0ull;
                                                               //  data; the test keeps a corrupted workspace from walking off the matrix)
                // ---- stage the window that holds the current cell's step ----
                const uint32_t s = (i - 1u) / rps;
                int rho = (int)((i - 1u) - s * rps);                               // row slot within the strip
                const uint32_t t_cur = j - 1u + (uint32_t)rho / R;
                const uint32_t whi = t_cur >> 4;
                uint32_t wlo, nb;
                if (TMODE == 0) {
                    wlo = whi >= SWMI_TB_BLOCKS - 1u ? whi - (SWMI_TB_BLOCKS - 1u) : 0u;
                    nb = whi - wlo + 1u;
                } else if (COOP) {
                    const uint32_t wtop = whi - whi % SWMI_CK_BLOCKS;
                    wlo = wtop >= (ts - 1u) * SWMI_CK_BLOCKS ? wtop - (ts - 1u) * SWMI_CK_BLOCKS : 0u;
                    nb = wtop + SWMI_CK_BLOCKS - wlo;
                } else {
                    wlo = whi - whi % SWMI_CK_BLOCKS;                              // windows start at checkpoints
                    nb = SWMI_CK_BLOCKS;
                }
                // COOP: the span the helpers have been re-sweeping since the last staging, if the walk arrived there
                bool use_spec = false;
                if (COOP && spec_wlo != 0xFFFFFFFFu) {
                    const uint32_t wtop = whi - whi % SWMI_CK_BLOCKS;
                    if (s == 0u && wtop + SWMI_CK_BLOCKS == spec_hi) { use_spec = true; wlo = spec_wlo; nb = spec_hi - spec_wlo; }
                }
                // COOP: the span of the first staging was already re-swept while wave 0 listed the maximum cells
                const bool prestaged = TMODE == 1 && pre_wlo == wlo && s == 0u && !use_spec;
                pre_wlo = 0xFFFFFFFFu;
                const int clo = (int)(16u * wlo) - 63;
                const uint32_t cw0 = clo > 0 ? (uint32_t)clo >> 2 : 0u;           // first dword of the reference window
                const uint32_t cw1 = (16u * (wlo + nb) - 1u) >> 2;
                WAVE_SYNC();
                if (use_spec) {
                    const unsigned long long tq0 = TB_DBG ? __builtin_amdgcn_s_memtime() : 0ull;
                    team_wait();
                    if (TB_DBG) tk_walk += (__builtin_amdgcn_s_memtime() - tq0) << 32;
                    uint32_t *t = tile_cur; tile_cur = tile_alt; tile_alt = t;
                    lds_ref[lane] = spec_rv0;
                    if (lane + WAVE < SWMI_TB_REFWIN_WORDS) lds_ref[lane + WAVE] = spec_rv1;
                    WAVE_SYNC();
                } else if (!prestaged) {
                    // the slice of the reference: loads issued now, stored to LDS after the re-sweep (at most 2 dwords per lane)
                    const uint32_t rx0 = cw0 + lane, rx1 = rx0 + WAVE, rlim = (n + 3u) / 4u;
                    const uint32_t rv0 = (rx0 <= cw1 && rx0 < rlim) ? refw[rx0] : 0u;
                    const uint32_t rv1 = (rx1 <= cw1 && rx1 < rlim) ? refw[rx1] : 0u;
                    if (TMODE == 0) {
                        const uint32_t *__restrict__ src = dirp + s * G.strip_words + (uint64_t)wlo * R * WAVE + lane;
                        for (uint32_t x = 0; x < nb * R; ++x) tile_cur[x * WAVE + lane] = src[(uint64_t)x * WAVE];
                    } else {
                        if (COOP) {
                            team_wait();                                           // (a speculative request nobody needs any more)
                            const uint32_t nq = nb / SWMI_CK_BLOCKS;
                            team_request((tile_cur == lds_tile ? 0u : 1u) | (s << 2), wlo, nq, nq - 1u);     // helpers 1 .. nq-1 deliver one window each
                        }
                        (void)replay_any<R, false, FULL>(A, pd, n, m, acgt, refw, readw, G, s, wlo, lane, tile_cur, 0, 0u, nullptr, 0u);
                    }
                    lds_ref[lane] = rv0;
                    if (lane + WAVE < SWMI_TB_REFWIN_WORDS) lds_ref[lane + WAVE] = rv1;
                    if (COOP) {
                        // wait for the helpers' windows
                        const unsigned long long tq0 = TB_DBG ? __builtin_amdgcn_s_memtime() : 0ull;
                        team_wait();
                        if (TB_DBG) tk_walk += (__builtin_amdgcn_s_memtime() - tq0) << 32;     // (waiting counted in the upper half)
                    }
                    WAVE_SYNC();
                }
                spec_wlo = 0xFFFFFFFFu;
                if (COOP && tile_alt != nullptr && ts > 1u && wlo > 0u && s == 0u) {
                    // the helpers start on the span to the left of this one, ts - 1 windows of it, while the walker walks
                    const uint32_t have = wlo / SWMI_CK_BLOCKS, nq = have < ts - 1u ? have : ts - 1u;
                    spec_hi = wlo;
                    spec_wlo = wlo - nq * SWMI_CK_BLOCKS;
                    const int sclo = (int)(16u * spec_wlo) - 63;
                    const uint32_t scw0 = sclo > 0 ? (uint32_t)sclo >> 2 : 0u, scw1 = (16u * spec_hi - 1u) >> 2;
                    const uint32_t rx0 = scw0 + lane, rx1 = rx0 + WAVE, rlim = (n + 3u) / 4u;
                    spec_rv0 = (rx0 <= scw1 && rx0 < rlim) ? refw[rx0] : 0u;      // its slice of the reference: held in registers meanwhile
                    spec_rv1 = (rx1 <= scw1 && rx1 < rlim) ? refw[rx1] : 0u;
                    team_request((tile_alt == lds_tile ? 0u : 1u) | 2u, spec_wlo, nq, nq);
                }
                const int tmin = (int)(16u * wlo);
                const unsigned long long tw0 = TB_DBG ? __builtin_amdgcn_s_memtime() : 0ull;
                if (TB_DBG) { tk_stage += tw0 - ts0; n_iters += 1ull << 32; }      // (stagings counted in the upper half)

#ifdef SWMI_WALK_CHASE
                // (Alternative walk, -DSWMI_WALK_CHASE: measured 0.084 ms against the 0.072 ms of the run-based walk below at the
                //  headline config -- one wave issues an instruction of ANY kind every ~5.6 cycles, so 23 scalar instructions per
                //  path step cost more than 145 instructions per 4.4 steps.  Kept as the simplest correct statement of the walk.)
                // One LDS round trip brings the 8 x 8 NEIGHBOURHOOD up-left of the current cell into the
                // wave: lane (a, b) = (lane >> 3, lane & 7) looks at cell (i - a, j - b) -- its direction bits, whether its two
                // bases match, whether it is staged at all -- and packs that into one word.  The path is then chased through the
                // neighbourhood by SCALAR code, one v_readlane per step (the lane index is the position in the neighbourhood):
                // direction, H(pred) = H - delta (`while (score > 0)`, SmithWaterman.java:380-409), op, next cell -- about 15
                // scalar instructions per path step and no memory access, 7-15 steps per round trip whatever mix of gaps and
                // alignment moves the path is made of.
                for (;;) {
                    if (TB_DBG) ++n_iters;
                    const uint32_t na = lane >> 3, nb = lane & 7u;
                    const int rho_x = rho - (int)na;
                    const uint32_t rx = rho_x > 0 ? (uint32_t)rho_x : 0u;
                    const uint32_t lx = rx / R, kx = rx - lx * R;
                    const uint32_t jj = j - nb;                                    // column of this lane's cell
                    const int tx = (int)jj - 1 + (int)lx;
                    const bool valid = rho_x >= 0 && j > nb && tx >= tmin;         // same strip, inside the matrix, inside the staged span
                    // all three LDS reads are issued together (one latency); lanes without a cell read element 0
                    const uint32_t dw = tile_cur[valid ? (((uint32_t)tx >> 4) - wlo) * (R * WAVE) + kx * WAVE + lx : 0u];
                    const uint32_t rc = ref_b[valid ? (jj - 1u) - 4u * cw0 : 0u];
                    const uint32_t qc = read_b[valid ? i - 1u - na : 0u];
                    const uint32_t d = (dw >> (2u * (15u - ((uint32_t)tx & 15u)))) & 3u;
                    // everything a path step needs from this cell, worked out by its lane: the move (rows, columns), the op, the
                    // score it takes off (:388-406), whether the move leaves the neighbourhood or reaches row / column 0
                    const uint32_t b0 = d & 1u, b1 = (d >> 1) & 1u;                // alignment chosen; else insertion over deletion
                    const uint32_t di = b0 | b1, dj = b0 | (b1 ^ 1u);
                    const uint32_t op = (b0 << 1) | (b1 & (b0 ^ 1u));              // SWMI_DIR_A = 2, _I = 1, _D = 0
                    const int delta = (int)(b0 ? (rc == qc ? umat : umis) : ugap);
                    const uint32_t last = (na + di > 7u || nb + dj > 7u) ? 1u : 0u;
                    const uint32_t edge = (i - na == di || j - nb == dj) ? 1u : 0u;
                    const int ctrl = valid ? (int)(0x80000000u | (edge << 9) | (last << 8) | (op << 4) | (di << 3) | dj) : 0;
                    // (the compiler does not know that i, j and score are the same in every lane: readfirstlane says so, and the
                    //  chase below then compiles to scalar code with scalar branches instead of an exec-masked vector loop)
                    const uint32_t si = uni(i), sj = uni(j);
                    uint32_t sscore = uni(score);
                    uint32_t idx = 0, sh = 0, opsacc = 0, lastc = 0, lastidx = 0;
                    bool done = false;
                    for (;;) {
                        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane(ctrl, (int)idx);
                        if ((int)c >= 0) break;                                     // not staged (or in the strip above): restage from here
                        sscore -= (uint32_t)__builtin_amdgcn_readlane(delta, (int)idx);
                        opsacc |= ((c >> 4) & 3u) << sh;
                        sh += 2u;
                        lastc = c; lastidx = idx;
                        idx += c & 15u;
                        if ((int)sscore <= 0) { done = true; break; }
                        if (c & 0x300u) {                                           // the move left the neighbourhood (at most 15 ops: one word) ...
                            if (c & 0x200u) { sscore = 0; done = true; }            // ... or reached row / column 0 (cannot happen with a positive score on consistent data)
                            break;
                        }
                    }
                    const uint32_t cnt = sh >> 1;
                    const uint32_t ca = cnt ? (lastidx >> 3) + ((lastc >> 3) & 1u) : 0u, cb = cnt ? (lastidx & 7u) + (lastc & 7u) : 0u;
                    score = sscore;
                    if (cnt) begin = (int)(sj - (lastidx & 7u));                    // `beginning = j` of the last cell visited (:383)
                    if (lane < cnt && n_ops + lane < 4u * A.lds_words) ops_b[n_ops + lane] = (uint8_t)((opsacc >> (2u * lane)) & 3u);
                    n_ops += cnt; i = si - ca; j = sj - cb; rho -= (int)ca;
                    if (done || cnt == 0u || rho < 0) break;                        // finished / the current cell needs another window or strip
                }
#else
                // Three diagonals are inspected at once, 21 lanes each: group 0 runs up from the current cell, group 1
                // from the cell above it (where an insertion leads), group 2 from the cell to its left (a deletion).
                // One iteration then takes: [a gap move] + [the run of alignment moves that follows] + [the gap move
                // that ends the run] -- about 4-5 path steps per LDS round trip on gappy paths, 21+ on clean ones.
                for (;;) {
                    if (TB_DBG) ++n_iters;
                    const uint32_t grp = lane / 21u, x = lane - grp * 21u;        // lane 63: grp 3, idle
                    const uint32_t di = grp == 1u ? 1u : 0u, dj = grp == 2u ? 1u : 0u;
                    const int rho_x = rho - (int)di - (int)x;
                    const uint32_t rx = rho_x > 0 ? (uint32_t)rho_x : 0u;
                    const uint32_t lx = rx / R, kx = rx - lx * R;
                    const uint32_t jj = j - dj - x;                                // column of this lane's cell
                    const int tx = (int)jj - 1 + (int)lx;
                    const bool valid = grp < 3u && rho_x >= 0 && j > dj + x && tx >= tmin;
                    // all three LDS reads are issued together (one latency): direction word, reference code, read code.
                    // Lanes without a cell read element 0 instead of branching around the loads.
                    uint32_t dw = tile_cur[valid ? (((uint32_t)tx >> 4) - wlo) * (R * WAVE) + kx * WAVE + lx : 0u];
                    uint32_t rc = ref_b[valid ? (jj - 1u) - 4u * cw0 : 0u];
                    uint32_t qc = read_b[valid ? i - 1u - di - x : 0u];
                    // (all three in flight before anything waits: left alone, the compiler put the direction word's read
                    //  behind the wait for the two codes -- a second LDS round trip in every iteration of the walk)
                    asm volatile("" : "+v"(dw), "+v"(rc), "+v"(qc));
                    const uint32_t d = (dw >> (2u * (15u - ((uint32_t)tx & 15u)))) & 3u;
                    const bool mt = rc == qc;
                    const uint64_t vmask = BALLOT(valid);
                    if (!(vmask & 1ull)) break;                                    // current cell left the window / the strip: restage
                    const uint64_t amask = BALLOT((d & 1u) != 0u) & vmask;       // alignment chosen
                    const uint64_t imask = BALLOT(d == 2u) & vmask;              // insertion chosen (else deletion)
                    const uint64_t mm = BALLOT(mt);
                    {
                        // ---- fast path: [gap move] + [run of alignment moves] + [gap move], taken in one go when the tracked
                        // score provably stays positive throughout (no move lowers it by more than udec / ugdec) and the cell
                        // after the first gap move was inspected.  A positive score also rules out reaching row/column 0.
                        const uint32_t g1 = (uint32_t)(~amask & 1ull);
                        const uint32_t isI1 = (uint32_t)(imask & 1ull);
                        const uint32_t fb = g1 ? (isI1 ? 21u : 42u) : 0u;
                        const uint32_t vb = (uint32_t)(vmask >> fb) & 0x1FFFFFu;
                        const uint32_t frun = (uint32_t)__builtin_ctz(~((uint32_t)(amask >> fb) & 0x1FFFFFu));   // 0..21
                        const uint32_t has3 = (vb >> frun) & 1u;                   // bit 21 is never set
                        if ((!g1 || (vb & 1u)) && score > (g1 + has3) * ugdec + frun * udec) {    // (score > 0 here: an unsigned compare)
                            const uint32_t isI3 = (uint32_t)(imask >> (fb + frun)) & 1u & has3;
                            const uint32_t nm = (uint32_t)__builtin_popcountll(mm & ((((1ull << frun) - 1ull)) << fb));
                            const uint32_t i1 = g1 & isI1, total = g1 + frun + has3;
                            score -= (g1 + has3) * ugap + nm * umat + (frun - nm) * umis;
                            const uint32_t j1 = j - (g1 - i1);                     // column after the first gap move
                            begin = has3 ? (int)(j1 - frun) : (frun ? (int)(j1 - frun + 1u) : (int)j);
                            if (lane < total && n_ops + lane < 4u * A.lds_words)
                                ops_b[n_ops + lane] = (uint8_t)(lane < g1 ? (isI1 ? SWMI_DIR_I : SWMI_DIR_D)
                                                               : lane < g1 + frun ? SWMI_DIR_A : (isI3 ? SWMI_DIR_I : SWMI_DIR_D));
                            n_ops += total;
                            const uint32_t dec_i = i1 + frun + isI3;
                            i -= dec_i; rho -= (int)dec_i;
                            j = j1 - frun - (has3 - isI3);
                            continue;
                        }
                    }
                    bool done = false;
                    uint32_t base = 0;                                             // first lane of the diagonal the run is on
                    if (!(amask & 1ull)) {
                        // ---- the current cell is an insertion or a deletion: H(pred) = H - gap   (:395-406) ----
                        begin = (int)j;                                             // :383
                        score -= ugap;
                        uint32_t op;
                        if (imask & 1ull) { --i; --rho; op = SWMI_DIR_I; base = 21u; } else { --j; op = SWMI_DIR_D; base = 42u; }
                        if (lane == 0 && n_ops < 4u * A.lds_words) ops_b[n_ops] = (uint8_t)op;
                        n_ops += 1u;
                        if ((int)score <= 0) break;
                        if (i == 0 || j == 0) { score = 0; break; }
                        if (rho < 0 || !((vmask >> base) & 1ull)) continue;       // next cell not staged: start over from it
                    }
                    // ---- a run of alignment moves on diagonal `base`: H(i-1,j-1) = H - s(ref[j-1], read[i-1])   (:388-394) ----
                    uint32_t run = (uint32_t)__builtin_ctzll(~((amask >> base) & 0x1FFFFFull));     // 0..21
                    if (run > 0) {
                        const uint64_t range = ((1ull << run) - 1ull) << base;
                        if (score > run * udec) {
                            // no move lowers the score by more than udec: it stays positive through the whole run
                            const uint32_t nm = (uint32_t)__builtin_popcountll(mm & range);
                            score -= nm * umat + (run - nm) * umis;
                        } else {
                            const bool in_run = (range >> lane) & 1ull;
                            const uint32_t cm = lanemask_lt_count(mm & range) + (mt ? 1u : 0u);   // matches among the run's lanes up to this one
                            const uint32_t after = score - (cm * umat + (lane - base + 1u - cm) * umis);   // H after this lane's move
                            const uint64_t z = BALLOT(in_run && (int)after <= 0);
                            if (z) { run = (uint32_t)__builtin_ctzll(z) - base + 1u; done = true; }   // `while (score > 0)` stops there
                            score = (uint32_t)__builtin_amdgcn_readlane((int)after, base + run - 1u);
                        }
                        begin = (int)(j - (run - 1u));
                        if (lane >= base && lane < base + run && n_ops + (lane - base) < 4u * A.lds_words)
                            ops_b[n_ops + (lane - base)] = (uint8_t)SWMI_DIR_A;
                        n_ops += run; i -= run; j -= run; rho -= (int)run;
                        if (done || (int)score <= 0) break;
                        if (i == 0 || j == 0) { score = 0; break; }
                        if (rho < 0) break;                                         // continues in the strip above
                    }
                    // ---- the gap move that ended the run, if that cell was inspected ----
                    const uint32_t nxt = base + run;
                    if (run < 21u && ((vmask >> nxt) & 1ull)) {
                        begin = (int)j;
                        score -= ugap;
                        uint32_t op;
                        if ((imask >> nxt) & 1ull) { --i; --rho; op = SWMI_DIR_I; } else { --j; op = SWMI_DIR_D; }
                        if (lane == 0 && n_ops < 4u * A.lds_words) ops_b[n_ops] = (uint8_t)op;
                        n_ops += 1u;
                        if ((int)score <= 0) break;
                        if (i == 0 || j == 0) { score = 0; break; }
                        if (rho < 0) break;
                    }
                }
#endif
                if (TB_DBG) tk_walk += __builtin_amdgcn_s_memtime() - tw0;
            }
            if (TB_DBG) n_steps += n_ops;
            WAVE_SYNC();

            // ---- the record: a table entry + the payload (ops packed 2 bits each, 16 per dword [+ the two aligned strings]) ----
            const uint32_t opw = A.raw ? 0u : (n_ops + 15u) / 16u;          // (records with strings carry no ops)
            const uint32_t words = swmi_payload_words(n_ops, A.raw != nullptr);
            const SwmiReserve rsv = swmi_reserve_issue(A, lane, words, 1u);
            // while the reservation is on its way: this lane's first dword of packed ops, and the last 256 characters of
            // GetAlignment's two strings (SmithWaterman.java:418-431) from the caller's own bytes.  The walker's current direction
            // tile is free between two walks (a speculative span goes to the other one) and serves as scratch.
            const bool staged = n_ops <= 4u * A.lds_words;
            auto pack16 = [&](uint32_t w) {
                uint32_t packed = 0;
#pragma unroll
                for (uint32_t c = 0; c < 4; ++c) {
                    const uint32_t first = 16u * w + 4u * c;
                    uint32_t x = first < n_ops ? lds_ops[4u * w + c] : 0u;
                    if (first + 4u > n_ops && first < n_ops) x &= (1u << (8u * (n_ops - first))) - 1u;
                    const uint32_t b8 = (x & 3u) | ((x >> 6) & 0xCu) | ((x >> 12) & 0x30u) | ((x >> 18) & 0xC0u);
                    packed |= b8 << (8u * c);
                }
                return packed;
            };
            const uint32_t packed0 = (staged && lane < opw) ? pack16(lane) : 0u;
            SwmiStrings<SwmiOpsPerByte> strs(SwmiOpsPerByte{ops_b}, staged ? n_ops : 0u, ci, cj, raw_ref, raw_read, lane, tile_cur);
            const uint32_t sw = strs.words(), ctop = strs.n_chunks();
            uint32_t wr0 = 0, wq0 = 0;
            if (A.raw && staged) strs.chunk(ctop - 1u, wr0, wq0);
            unsigned long long off;
            uint32_t rslot;
            if (swmi_reserve_finish(A, rsv, words, 1u, off, rslot) && staged) {
                uint32_t *dst = A.arena + off;
                if (lane == 0) swmi_write_rec(A, rslot, pd.out_id, crank, begin, ci, cj, n_ops, off);
                if (lane < opw) dst[lane] = packed0;
                for (uint32_t w = lane + WAVE; w < opw; w += WAVE) dst[w] = pack16(w);
                if (A.raw) {
                    const uint32_t w = 64u * (ctop - 1u) + lane;
                    if (w < sw) { dst[w] = wr0; dst[sw + w] = wq0; }
                    strs.store_from(dst, ctop - 1u);
                }
            } else if (lane == 0) {
                atomicOr(&A.out[pd.out_id].flags, SWMI_F_ARENA_OVF);
                if (A.ovf_host) *A.ovf_host = 1u;
            }
            WAVE_SYNC();
        }
    }
    if (COOP && lane == 0)                                                         // releases this team's helpers
        __hip_atomic_store(const_cast<uint32_t *>(&shared[7u + 4u * slot]), 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (TB_DBG && lane == 0 && slot == 0) {
        A.dbg[4 * pd.out_id] = __builtin_amdgcn_s_memtime() - tk0;
        A.dbg[4 * pd.out_id + 1] = tk_walk;
        A.dbg[4 * pd.out_id + 2] = n_steps | (tk_stage << 16);       // (steps < 65536 in the diagnostics runs)
        A.dbg[4 * pd.out_id + 3] = n_iters;
    }
}
