// swmi_cells.h -- the cell streams and the 16-step block every sweep of the linear-gap kernels is made of.  Instantiated by
// the sweep kernels (swmi_sweep.hip), by the window re-sweeps of the tracebacks (swmi_walk.h) and by the resident kernel
// (swmi_traceback.hip):
//   CellsAsm / CellsRef + fill_block16   the general block: any alphabet, any tie order, strips, direction bits or not
//   SweepStep4Asm / sweep_step_ref       the 3-VALU score-only step of the usual pair (fast symbols, one strip, gap <= 0)
//   StripGeom                            the workspace geometry a sweep and its re-sweeps agree on
// Device code only; everything is __forceinline__ and there is no static LDS, so the unit a kernel is compiled in does not
// change its code.  -DSWMI_NO_ASM selects the plain C++ statements, -DSWMI_STRIP_DIAG the strip pipeline's wait counters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "swmi_device.h"
#include "swmi_wave.h"

// The 8 x int4 score profiles of a lane's R rows (fast symbols): nibble c/4 of row k's profile is the score of the row's base
// against reference symbol c.  The R base codes are loaded FIRST, unconditionally (images are padded), so that the loads are in
// flight together: a load behind each `row < m` test serialised R memory latencies in front of every window re-sweep.
template <int R>
__device__ __forceinline__ void build_profiles(int (&q)[R], const uint32_t *__restrict__ readw, const uint32_t row0, const uint32_t m,
                                               const int match, const int mismatch) {
    uint32_t c[R];
#pragma unroll
    for (int k = 0; k < R; ++k) c[k] = seq_code(readw, row0 + k) & 28u;      // 0, 4, ..., 28
#pragma unroll
    for (int k = 0; k < R; ++k) {
        uint32_t p = (uint32_t)(mismatch & 0xF) * 0x11111111u;
        if (row0 + k < m) p = (p & ~(0xFu << c[k])) | ((uint32_t)(match & 0xF) << c[k]);
        q[k] = (int)p;
    }
}

// ------------------------------------------------------------------------------------------------
// the R cells of one lane in one step (previous column's H in hin, this column's H to hout)
// ------------------------------------------------------------------------------------------------
// the fast cell stream looks scores up in a profile of 8 x int4 (v_dot8_i32_i4): match and mismatch must fit
#define SWMI_SCORES_FIT(A) ((A).match >= -8 && (A).match <= 7 && (A).mismatch >= -8 && (A).mismatch <= 7)

#include "swmi_cells_gen.inc"   // CellsAsm<R, ACGT, STRICT, DIRS>: hand-scheduled instruction stream

// Plain C++ statement of the same update (build with -DSWMI_NO_ASM to A/B against the asm stream).
template <int R, bool ACGT, bool STRICT, bool DIRS>
struct CellsRef {
    static __device__ __forceinline__ void step(const int (&hin)[R], int (&hout)[R], uint32_t (&acc)[R], const int (&q)[R],
                                                int rb, int diag, int up, int gap, int vmat, int vmis) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int left = hin[k];
            int sc;
            if (ACGT) sc = rb ? __builtin_amdgcn_sbfe(q[k], (unsigned)__builtin_ctz((unsigned)rb), 4u) : 0;   // rb = 1 << 4*symbol
            else      sc = (rb == q[k]) ? vmat : vmis;
            const int a = diag + sc;                       // SmithWaterman.java:244 / AlignmentScore :309-318
            const int t2 = (up > left ? up : left) + gap;   // :227, :235 (InsDelScore :277-280)
            int hv = a > t2 ? a : t2;
            hv = hv > 0 ? hv : 0;                           // `int max = 0` :223
            if (DIRS) {
                const bool bi = STRICT ? (up > left) : (up >= left);
                const bool ba = STRICT ? (a > t2) : (a >= t2);
                acc[k] = (acc[k] << 2) | (bi ? 2u : 0u) | (ba ? 1u : 0u);
            }
            diag = left;
            up = hv;
            hout[k] = hv;
        }
    }
};

#ifdef SWMI_NO_ASM
template <int R, bool ACGT, bool STRICT, bool DIRS> using Cells = CellsRef<R, ACGT, STRICT, DIRS>;
#else
template <int R, bool ACGT, bool STRICT, bool DIRS> using Cells = CellsAsm<R, ACGT, STRICT, DIRS>;
#endif

// What a 16-step block does besides the scores:
//   SWMI_MODE_FIELD   sweep, direction bits packed and stored to HBM, tied maxima tracked by events          (mode 0 sweep)
//   SWMI_MODE_SCORE   sweep, scores only (5 VALU per cell) + checkpoints, tied maxima tracked by events      (mode 2 sweep)
//   SWMI_MODE_REPLAY  a checkpoint-to-checkpoint window re-swept, direction bits to LDS, nothing tracked     (mode 1/2 traceback)
//   SWMI_MODE_WINMAX  sweep, scores only + checkpoints; per lane only a running maximum (no compare, no branch,
//                     no cell list): the wave reduces it to ONE maximum per checkpoint window                 (mode 1 sweep)
//   SWMI_MODE_DETECT  a window re-swept like REPLAY that also lists its cells equal to the pair's maximum     (mode 1 traceback)
#define SWMI_MODE_FIELD  0
#define SWMI_MODE_SCORE  1
#define SWMI_MODE_REPLAY 2
#define SWMI_MODE_WINMAX 3
#define SWMI_MODE_DETECT 4

// ------------------------------------------------------------------------------------------------
// rare path: at step t some lane reached the running maximum.  thr / cnt are wave-uniform; they travel
// packed in one 64-bit value.
// ------------------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ unsigned long long
record_max_cells(int h0, int h1, int h2, int h3, uint32_t t, uint32_t lane_eff, uint32_t n, uint32_t row0, uint32_t m,
                 int thr, uint32_t cnt, uint2 *__restrict__ cells, uint32_t ccap) {
    const int hh[4] = {h0, h1, h2, h3};
    const uint32_t c0 = t - lane_eff;                  // column index j-1 the lane worked on at step t
    const bool active = c0 < n;
    int v[R];
    int cand = -1;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        v[k] = (active && row0 + k < m) ? hh[k] : -1;   // rows past the read and lanes off their range never count
        cand = cand > v[k] ? cand : v[k];
    }
    if (BALLOT(cand >= thr) == 0) return ((unsigned long long)(uint32_t)thr << 32) | cnt;   // stale trigger
    // strict increase: climb to the wave's maximum by lane hops (no reduction network needed: few lanes exceed)
    uint64_t gt = BALLOT(cand > thr);
    while (gt) {                                        // SmithWaterman.java:176-181
        thr = __builtin_amdgcn_readlane(cand, (int)__builtin_ctzll(gt));
        cnt = 0;
        gt = BALLOT(cand > thr);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const bool hit = v[k] == thr;                   // :182-185
        const uint64_t hm = BALLOT(hit);
        if (hm) {
            const uint32_t pos = cnt + lanemask_lt_count(hm);
            if (hit && pos < ccap) cells[pos] = make_uint2(row0 + k + 1, c0 + 1u);
            cnt += (uint32_t)__popcll(hm);
        }
    }
    return ((unsigned long long)(uint32_t)thr << 32) | cnt;
}

// ------------------------------------------------------------------------------------------------
// sweep state of one wavefront
// ------------------------------------------------------------------------------------------------
#ifdef SWMI_STRIP_DIAG
#define SWMI_SD(...) __VA_ARGS__
#else
#define SWMI_SD(...)
#endif
template <int R>
struct FillState {
    int h[R];            // H of the lane's rows: read by even steps of a block, written by odd ones
    int g[R];            // ... and the other way round (ping-pong, see fill_block16)
    uint32_t acc[R];     // direction bits of the last <= 16 steps
    int q[R];            // ACGT (= fast symbols): the row's 8 x int4 score profile; else the read's base code
    int nprev, rb;
    int thr;             // wave-uniform running maximum
    uint32_t cnt;        // wave-uniform number of cells equal to thr
    uint64_t ev_prev;    // lanes whose previous step reached thr (handled one step late, see below)
    int lmax;            // WINMAX: this lane's maximum H since the last checkpoint
    uint32_t events;     // slow-path entries (diagnostics only)
    bool dbg_skip;       // diagnostics only
#ifdef SWMI_STRIP_DIAG
    unsigned long long dg_pub;    // ticks spent waiting before progress publications
#endif
};

// read-side operands of this lane's rows, and a zero H column
template <int R, bool ACGT>
__device__ __forceinline__ void setup_rows(FillState<R> &S, const uint32_t *__restrict__ readw, uint32_t row0, uint32_t m,
                                           int match, int mismatch) {
    if (ACGT) {
        build_profiles<R>(S.q, readw, row0, m, match, mismatch);      // 8 signed score nibbles indexed by the reference code
    } else {
        uint32_t c[R];
#pragma unroll
        for (int k = 0; k < R; ++k) c[k] = seq_code(readw, row0 + k);
#pragma unroll
        for (int k = 0; k < R; ++k) S.q[k] = row0 + k < m ? (int)c[k] : (int)SWMI_CODE_PAD;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        S.h[k] = 0;
        S.g[k] = 0;
        S.acc[k] = 0;
    }
    S.nprev = 0;                                     // N received one step earlier = NW of this step
    S.rb = 0;                                        // reference base operand of this lane's current column
}

template <int R>
__device__ __forceinline__ void handle_pending(FillState<R> &S, const int (&hv)[R], uint32_t t, uint32_t lane_eff,
                                               uint32_t n, uint32_t row0, uint32_t m, uint2 *__restrict__ cells, uint32_t ccap) {
    if (S.dbg_skip) {          // diagnostics: price of the branch alone (results are wrong in this mode)
        S.events++;
        S.thr += 1;
        return;
    }
    const unsigned long long tc = record_max_cells<R>(
        hv[0], R > 1 ? hv[R > 1 ? 1 : 0] : 0, R > 2 ? hv[R > 2 ? 2 : 0] : 0, R > 3 ? hv[R > 3 ? 3 : 0] : 0,
        t, lane_eff, n, row0, m, S.thr, S.cnt, cells, ccap);
    S.events++;
    S.thr = __builtin_amdgcn_readfirstlane((int)(tc >> 32));
    S.cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tc);
}

// acc with lane `l` (0..15, a constant after unrolling) replaced by the scalar v
__device__ __forceinline__ int writelane_const(int acc, const int v, const uint32_t l) {
#define SWMI_WL(L) case L: asm("v_writelane_b32 %0, %1, " #L : "+v"(acc) : "s"(v)); break;
    switch (l) {
    SWMI_WL(0) SWMI_WL(1) SWMI_WL(2) SWMI_WL(3) SWMI_WL(4) SWMI_WL(5) SWMI_WL(6) SWMI_WL(7)
    SWMI_WL(8) SWMI_WL(9) SWMI_WL(10) SWMI_WL(11) SWMI_WL(12) SWMI_WL(13) SWMI_WL(14) SWMI_WL(15)
    }
#undef SWMI_WL
    return acc;
}

// 16 anti-diagonal steps t = t0 .. t0+15.  PRED: lanes may be outside their column range (ramp-up /
// ramp-down blocks); otherwise every lane below `lact` is inside it for all 16 steps.
//
// The H registers ping-pong between S.h (read by even steps) and S.g (read by odd steps), so after step t
// the values of step t-1 are still there.  That lets the tied-maximum test of step t-1 -- a compare into
// an SGPR pair -- be branched on one step later, when its result has long arrived, instead of stalling the
// wave on a VALU->scalar-branch dependency every step (measured: 57 of 197 cycles per step).
template <int R, bool ACGT, bool STRICT, bool MULTI, bool PRED, int MODE, bool PIPE = false>
__device__ __forceinline__ void fill_block16(FillState<R> &S, const uint4 w, const uint32_t t0,
                                             const uint32_t lane, const uint32_t lane_eff,
                                             const uint32_t n, const uint32_t m, const uint32_t row0,
                                             const int gap, const int vmat, const int vmis,
                                             const int seamv, const bool reads_seam, const bool feeds_seam,
                                             int32_t *__restrict__ seam_out,
                                             uint2 *__restrict__ cells, const uint32_t ccap,
                                             uint32_t *pub_slot = nullptr, const uint32_t pub_val = 0u,
                                             int32_t *__restrict__ seam_sh = nullptr, const uint32_t own_lo = 0u, const uint32_t own_hi = 0u) {
    constexpr bool DIRS = MODE == SWMI_MODE_FIELD || MODE == SWMI_MODE_REPLAY || MODE == SWMI_MODE_DETECT;
    constexpr bool TRACK = MODE == SWMI_MODE_FIELD || MODE == SWMI_MODE_SCORE;     // deferred tied-maximum events
    constexpr bool LMAX = MODE == SWMI_MODE_WINMAX;                                  // per-lane running maximum only
    constexpr bool DETECT = MODE == SWMI_MODE_DETECT;                                // list the cells equal to S.thr
    constexpr bool FEEDS = MODE == SWMI_MODE_FIELD || MODE == SWMI_MODE_SCORE || MODE == SWMI_MODE_WINMAX;   // sweep (writes seam rows)
    using C = Cells<R, ACGT, DIRS ? STRICT : false, DIRS>;
    int seam_acc = 0;
    // PIPE: "the blocks before this one are complete" (pub_val) is published as late as possible before this block's own
    // seam stores: the wait then covers stores that were issued a block ago, not a moment ago
    auto publish = [&]() {
        if (PIPE && pub_val) {
            SWMI_SD(const unsigned long long dg2 = __builtin_amdgcn_s_memtime();)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            SWMI_SD(S.dg_pub += __builtin_amdgcn_s_memtime() - dg2;)
            if (lane == 0) __hip_atomic_store(pub_slot, pub_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    if (PRED) publish();
#pragma unroll
    for (uint32_t s = 0; s < 16; ++s) {
        const int (&hin)[R] = (s & 1u) ? S.g : S.h;
        int (&hout)[R] = (s & 1u) ? S.h : S.g;
        const uint32_t wsel = s < 4 ? w.x : s < 8 ? w.y : s < 12 ? w.z : w.w;
        // base code of column t0+s+1 (lane 0).  ACGT: codes are 0, 4, ..., 28 and travel down the lanes ONE-HOT
        // (1 << code) so that one v_dot8_i32_i4 with the row's score profile yields NW + s(ref, read); the SDWA byte
        // select makes extract + shift a single instruction.
        int feed;
        if (ACGT) {
            switch (s & 3u) {
            case 0:  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(feed) : "v"(wsel), "v"(1)); break;
            case 1:  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(feed) : "v"(wsel), "v"(1)); break;
            case 2:  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(feed) : "v"(wsel), "v"(1)); break;
            default: asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(feed) : "v"(wsel), "v"(1)); break;
            }
        } else {
            feed = (int)((wsel >> (8u * (s & 3u))) & 0xFFu);
        }
        S.rb = wave_shr1(feed, S.rb);
        int nin;
        if (MULTI) {
            // seamv is 0 in every lane of a strip with no seam above it: no branch on reads_seam (it cost an exec-masked
            // branch per step, 9 instructions where 3 do)
            nin = wave_shr1(__builtin_amdgcn_readlane(seamv, s), hin[R - 1]);
        } else {
            nin = wave_shr1_zero(hin[R - 1]);
        }
        int mrow = -1;
        if (PRED) {
            const uint32_t c0 = t0 + s - lane_eff;                         // column index j-1 of this lane
            if (c0 < n) {
                C::step(hin, hout, S.acc, S.q, S.rb, S.nprev, nin, gap, vmat, vmis);
                if (TRACK || DETECT) {
                    mrow = hout[0];
#pragma unroll
                    for (int k = 1; k < R; ++k) mrow = mrow > hout[k] ? mrow : hout[k];
                }
                if (LMAX) {
#pragma unroll
                    for (int k = 0; k < R; ++k) S.lmax = S.lmax > hout[k] ? S.lmax : hout[k];
                }
                if (MULTI && FEEDS && feeds_seam && lane == WAVE - 1) {
                    if (PIPE) __hip_atomic_store(seam_out + c0 + 1, hout[R - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else      seam_out[c0 + 1] = hout[R - 1];
                    if (PIPE && seam_sh && c0 + 1u > own_lo && c0 + 1u <= own_hi) seam_sh[c0 + 1] = hout[R - 1];   // (column chunk: the columns it owns)
                }
            } else {
#pragma unroll
                for (int k = 0; k < R; ++k) hout[k] = hin[k];             // a lane off its range keeps its state
            }
        } else {
            C::step(hin, hout, S.acc, S.q, S.rb, S.nprev, nin, gap, vmat, vmis);
            if (TRACK || DETECT) {
                mrow = hout[0];
#pragma unroll
                for (int k = 1; k < R; ++k) mrow = mrow > hout[k] ? mrow : hout[k];
            }
            if (LMAX) {
                if (R == 3) {
                    // 6 new values per two steps = three v_max3: the last row of an even step waits for the odd one
                    // (its register is still live there thanks to the ping-pong)
                    if (s & 1u) {
                        int x = S.lmax > hin[2] ? S.lmax : hin[2];  x = x > hout[0] ? x : hout[0];
                        x = x > hout[1] ? x : hout[1];              S.lmax = x > hout[2] ? x : hout[2];
                    } else {
                        const int x = S.lmax > hout[0] ? S.lmax : hout[0];
                        S.lmax = x > hout[1] ? x : hout[1];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < R; ++k) S.lmax = S.lmax > hout[k] ? S.lmax : hout[k];
                }
            }
            // seam row: lane 63's last row of this step goes to lane s of seam_acc (v_readlane + v_writelane); one 64-byte
            // store per block below instead of an exec-masked branch, a 64-bit address and a one-lane store per step
            if (MULTI && FEEDS) seam_acc = writelane_const(seam_acc, __builtin_amdgcn_readlane(hout[R - 1], WAVE - 1), s);
        }
        S.nprev = nin;
        if (DETECT) {
            // replay of a window that holds the pair's maximum: list its cells equal to it (immediate branch: 32 steps only)
            if (BALLOT(mrow >= S.thr) != 0) {
                const uint32_t c0d = t0 + s - lane_eff;
                const bool act = c0d < n;
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    const bool hit = act && (row0 + k < m) && (hout[k] == S.thr);      // SmithWaterman.java:182-185
                    const uint64_t hm = BALLOT(hit);
                    if (hm) {
                        const uint32_t pos = S.cnt + lanemask_lt_count(hm);
                        if (hit && pos < ccap) cells[pos] = make_uint2(row0 + k + 1, c0d + 1u);
                        S.cnt += (uint32_t)__popcll(hm);
                    }
                }
            }
        }
        if (TRACK) {
            const uint64_t ev = BALLOT(mrow >= S.thr);      // all 64 lanes vote: thr / cnt stay wave-uniform
            if (__builtin_expect(S.ev_prev != 0, 0))                           // step t0+s-1, values still in hin
                handle_pending<R>(S, hin, t0 + s - 1u, lane_eff, n, row0, m, cells, ccap);
            S.ev_prev = ev;
        }
    }
    if (!PRED) publish();
    if (MULTI && FEEDS && !PRED && feeds_seam && lane < 16u) {
        // a steady block of a strip that feeds a seam has all 64 lanes on rows: lane 63 was on column t0 + s - 62 (1-based)
        // at step s.  PIPE: another wavefront (possibly on another XCD) is already reading this row: device-coherent store
        const uint32_t col = t0 - (WAVE - 2u) + lane;
        int32_t *dst = seam_out + col;
        if (PIPE) __hip_atomic_store(dst, seam_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else      *dst = seam_acc;
        if (PIPE && seam_sh && col > own_lo && col <= own_hi) seam_sh[col] = seam_acc;
    }
}

// geometry shared by the sweep and its replay
struct StripGeom {
    uint32_t rps, n_strips, wblocks, n_ck;
    uint64_t strip_words;        // dwords of workspace per strip
    uint64_t wmax_off;           // mode 1: offset of the strip's per-window maxima inside its workspace
};
// hmode = the pipeline the host selected: 0 direction field, 1 checkpoints + window maxima, 2 checkpoints only
template <int R>
__device__ __forceinline__ StripGeom strip_geom(uint32_t m, uint32_t n, uint32_t hmode) {
    StripGeom g;
    g.rps = WAVE * R;
    g.n_strips = (m + g.rps - 1) / g.rps;
    g.wblocks = (n + 63u + 15u) / 16u;                       // 16-step blocks reserved per strip
    g.n_ck = (g.wblocks + SWMI_CK_BLOCKS - 1u) / SWMI_CK_BLOCKS;
    g.wmax_off = (uint64_t)g.n_ck * (R + 2) * WAVE;
    g.strip_words = hmode == 0 ? (uint64_t)g.wblocks * R * WAVE
                               : g.wmax_off + (hmode == 1 ? (uint64_t)((g.n_ck + 63u) & ~63u) : 0u);
    return g;
}

// ------------------------------------------------------------------------------------------------
// the score-only step of the usual pair (tools/gen_step.py): state, plain statement, masked last blocks.  The sweep
// that runs it is sweep_fast (swmi_sweep.hip); the resident kernel (swmi_traceback.hip) runs it too.
// ------------------------------------------------------------------------------------------------
#include "swmi_step_gen.inc"   // SweepStep4Asm<R>: four steps per asm statement

template <int R>
struct SweepState {
    int h[R], g[R];      // H of the lane's rows: h is read by even steps and written by odd ones, g the other way round
    int hp[R];           // max(H + gap, 0) of the same rows, updated in place
    int q[R];            // the row's 8 x int4 score profile
    int rbx, rby;        // one-hot reference symbol: rbx is what an even step consumes (it prepares rby for the odd one)
    int lmax;            // this lane's maximum H since the last window boundary
};

// plain statement of one step of SweepStep4Asm::run.  Used for the blocks in which some lane has run past the last column
// (`in_range` false: the lane keeps its state), and for every block when built with -DSWMI_NO_ASM.
template <int R>
__device__ __forceinline__ void sweep_step_ref(const int (&hin)[R], int (&hout)[R], int (&hp)[R], const int (&q)[R],
                                               const int rb, int &rbn, const uint32_t feed_code, const uint32_t gm,
                                               int &lm, const bool in_range) {
    const int nw = wave_shr1_zero(hout[R - 1]);      // lane l-1's bottom row two steps ago = NW of row 0 (lane 0: 0)
    const int upp = wave_shr1_zero(hp[R - 1]);       // max(N + gap, 0) of row 0 (lane 0: 0)
    if (in_range) {
        int diag = nw, up = upp;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int a = __builtin_amdgcn_sdot8(q[k], rb, diag, false);    // SmithWaterman.java:244 (AlignmentScore :309-318)
            diag = hin[k];
            int hv = a > up ? a : up;                                         // :227-240: max(W + gap, N + gap, 0) is max(hp, hp)
            hv = hv > hp[k] ? hv : hp[k];
            hout[k] = hv;
            hp[k] = (uint32_t)hv > gm ? (int)((uint32_t)hv - gm) : 0;
            up = hp[k];
            lm = lm > hv ? lm : hv;
        }
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k) hout[k] = hin[k];
    }
    rbn = wave_shr1((int)(1u << (feed_code & 31u)), rb);
}

// 16 steps of a block in which some lane runs past the last column.  Such a lane goes on computing -- nobody reads its values:
// the lane below it took what it needed one step earlier -- but its window maximum must not see them: SweepStepTailAsm updates
// the maximum under a lane mask.  (-DSWMI_NO_ASM: the plain statement, which also leaves such a lane's state alone.)
template <int R>
__device__ __forceinline__ void sweep_tail_block(SweepState<R> &S, const uint4 w, const uint32_t wnext_x, const uint32_t t0,
                                                 const uint32_t lane_eff, const uint32_t n, const int one, const uint32_t gm) {
#ifndef SWMI_NO_ASM
    const uint32_t c = t0 - lane_eff;              // column index (0-based) of this lane at step t0; lanes without rows: far outside
    SweepStepTailAsm<R, 0>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.x, w.y, one, gm, S.lmax, c + 0u, n);
    SweepStepTailAsm<R, 1>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.x, w.y, one, gm, S.lmax, c + 1u, n);
    SweepStepTailAsm<R, 2>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.x, w.y, one, gm, S.lmax, c + 2u, n);
    SweepStepTailAsm<R, 3>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.x, w.y, one, gm, S.lmax, c + 3u, n);
    SweepStepTailAsm<R, 0>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.y, w.z, one, gm, S.lmax, c + 4u, n);
    SweepStepTailAsm<R, 1>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.y, w.z, one, gm, S.lmax, c + 5u, n);
    SweepStepTailAsm<R, 2>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.y, w.z, one, gm, S.lmax, c + 6u, n);
    SweepStepTailAsm<R, 3>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.y, w.z, one, gm, S.lmax, c + 7u, n);
    SweepStepTailAsm<R, 0>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.z, w.w, one, gm, S.lmax, c + 8u, n);
    SweepStepTailAsm<R, 1>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.z, w.w, one, gm, S.lmax, c + 9u, n);
    SweepStepTailAsm<R, 2>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.z, w.w, one, gm, S.lmax, c + 10u, n);
    SweepStepTailAsm<R, 3>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.z, w.w, one, gm, S.lmax, c + 11u, n);
    SweepStepTailAsm<R, 0>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.w, wnext_x, one, gm, S.lmax, c + 12u, n);
    SweepStepTailAsm<R, 1>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.w, wnext_x, one, gm, S.lmax, c + 13u, n);
    SweepStepTailAsm<R, 2>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.w, wnext_x, one, gm, S.lmax, c + 14u, n);
    SweepStepTailAsm<R, 3>::run(S.h, S.g, S.hp, S.q, S.rbx, S.rby, w.w, wnext_x, one, gm, S.lmax, c + 15u, n);
#else
#pragma unroll
    for (uint32_t s = 0; s < 16; ++s) {
        const uint32_t s1 = s + 1u;
        const uint32_t wf = s1 < 4 ? w.x : s1 < 8 ? w.y : s1 < 12 ? w.z : s1 < 16 ? w.w : wnext_x;
        const uint32_t code = (wf >> (8u * (s1 & 3u))) & 0xFFu;
        const bool in_range = (t0 + s - lane_eff) < n;
        if (s & 1u) sweep_step_ref<R>(S.g, S.h, S.hp, S.q, S.rby, S.rbx, code, gm, S.lmax, in_range);
        else        sweep_step_ref<R>(S.h, S.g, S.hp, S.q, S.rbx, S.rby, code, gm, S.lmax, in_range);
    }
#endif
}

// 4 wavefronts per workgroup, one pair each: the 4 waves of a workgroup land on the 4 SIMDs of a CU, so a
// grid of n_pairs/4 workgroups spreads evenly over the SIMDs.
#define FILL_WAVES 4
