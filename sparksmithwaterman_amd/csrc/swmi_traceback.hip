// swmi_traceback.hip -- gfx950 (MI355X / CDNA4) traceback kernels of the Smith-Waterman hot path and the launchers that
// reach them:
//   swmi_launch_traceback         one workgroup or one wavefront per pair
//     sw_traceback_winmax_kernel    mode 1 (the default, the headline path): one workgroup per pair lists the maximum cells
//                                   from the sweep's window maxima, then walks the alignments in teams of wavefronts (COOP)
//     sw_traceback_kernel           mode 0: walks through the direction field the sweep stored to HBM
//     sw_traceback_replay_kernel    mode 2: walks through checkpoint windows re-swept one at a time
//   swmi_launch_traceback_split   mode 1, few pairs or many tied maxima per pair
//     sw_detect_windows_kernel      one wavefront per checkpoint window: lists the maximum cells, queues one walk item per cell
//     sw_walk_items_kernel          a fixed grid of wavefronts shares the queue, one alignment per wavefront
//   swmi_launch_resident          mode 1, small pairs
//     sw_resident_pairs_kernel      sweep, cell list and all walks of a pair by one wavefront, its direction field in LDS
//
// Replaces GetAlignment.call  src/sw/SmithWaterman.java:354-436 for a whole batch at once (the resident kernel also
// ScoreMatrix.call :129-190).
//
// The walk: one wavefront per alignment; orders the tied cells as the reference would list
//   them, walks each path through the direction field while tracking the score arithmetically
//   (H(pred) = H - delta, so `while (score > 0)` of SmithWaterman.java:380 needs no score matrix),
//   stages the 2-bit ops in LDS and appends one variable-length record per alignment to an arena.
// The re-sweep of a window and the walk itself: swmi_walk.h; the blocks and cell streams: swmi_cells.h.
//
// These six kernels stay in ONE unit on purpose: the code the compiler emits for sw_traceback_winmax_kernel (register
// allocation, spills) and for sw_resident_pairs_kernel depends on which other kernels of the unit instantiate the shared
// templates, and in what order -- measured, profiles/r09/kernel_split.md.  The sweep kernels (swmi_sweep.hip) do not take part.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdlib.h>
#include "swmi_device.h"
#include "swmi_emit.h"
#include "swmi_launch.h"
#include "swmi_walk.h"

// The helper side of COOP: wave `wave` >= nw serves team (wave - nw) % nw as its window number 1 + (wave - nw) / nw.
template <int R>
__device__ __forceinline__ void coop_helper(const TraceArgs &A, const PairDesc pd, const uint32_t lane, const uint32_t wave,
                                            const uint32_t nw, const uint32_t ts, const uint32_t n_waves_all,
                                            uint32_t *__restrict__ tiles, volatile uint32_t *__restrict__ shared) {
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const StripGeom G = strip_geom<R>(m, n, 1u);
    const bool acgt = rd.acgt && qd.acgt && SWMI_SCORES_FIT(A);
    const uint32_t team = (wave - nw) % nw, q = 1u + (wave - nw) / nw;
    uint32_t last = 0;
    for (;;) {
        uint32_t seq;
        while ((seq = __hip_atomic_load(const_cast<uint32_t *>(&shared[7u + 4u * team]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == last)
            __builtin_amdgcn_s_sleep(SWMI_HELPER_SLEEP);
        if (seq == 0xFFFFFFFFu) break;
        last = seq;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // request: flags bit 0 = the team's second buffer, bit 1 = speculative (the walker takes no window: helper q takes window
        // q-1), bits 2.. = the strip
        const uint32_t flags = shared[4u + 4u * team], wlo = shared[5u + 4u * team], nq = shared[6u + 4u * team];
        const uint32_t s = flags >> 2;
        const uint32_t win = (flags & 2u) ? q - 1u : q;
        if (q < ts && win < nq) {
            uint32_t *__restrict__ base = ((flags & 1u) ? tiles + n_waves_all * (SWMI_CK_BLOCKS * SWMI_RMAX * WAVE) : tiles) +
                                          team * ts * (SWMI_CK_BLOCKS * SWMI_RMAX * WAVE);
            (void)replay_any<R, false, false>(A, pd, n, m, acgt, refw, readw, G, s, wlo + win * SWMI_CK_BLOCKS, lane,
                                       base + win * SWMI_CK_BLOCKS * R * WAVE, 0, 0u, nullptr, 0u);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) atomicAdd(const_cast<uint32_t *>(&shared[20u + team]), 1u);
        }
    }
}

// 4 wavefronts per workgroup (one pair each, like the sweep) so that the walks of slot 0 -- one per pair -- land
// one per SIMD; the extra slots' few walks fall where they may.
template <int TMODE>
__device__ __forceinline__ void traceback_entry(const TraceArgs &A, uint32_t *lds_all) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t pair = blockIdx.x * FILL_WAVES + wave;
    if (pair >= A.n_pairs) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = blockIdx.y;
    uint32_t *tb_lds = lds_all + wave * (A.lds_words + A.lds_read_words + SWMI_TB_REFWIN_WORDS +
                                         (TMODE == 0 ? SWMI_TB_BLOCKS : SWMI_CK_BLOCKS) * SWMI_RMAX * WAVE);
    uint32_t *tile = tb_lds + A.lds_words + A.lds_read_words + SWMI_TB_REFWIN_WORDS;
    const PairDesc pd = A.pairs[pair];
    const PairOut po = A.out[pd.out_id];
    if (A.out_host && slot == 0 && lane == 0) A.out_host[pd.out_id] = po;      // result straight into pinned host memory
    if (po.flags & (SWMI_F_DEGENERATE | SWMI_F_CELL_OVF)) return;
    if (po.n_cells <= slot) return;
    const uint32_t R = swmi_rows_per_lane(A.reads[pd.read_id].len);
    if (R == 1)      traceback_pair<1, TMODE, false>(A, pd, po, lane, slot, SWMI_TB_SLOTS, tb_lds, tile, nullptr, 1u);
    else if (R == 2) traceback_pair<2, TMODE, false>(A, pd, po, lane, slot, SWMI_TB_SLOTS, tb_lds, tile, nullptr, 1u);
    else if (R == 3) traceback_pair<3, TMODE, false>(A, pd, po, lane, slot, SWMI_TB_SLOTS, tb_lds, tile, nullptr, 1u);
    else             traceback_pair<4, TMODE, false>(A, pd, po, lane, slot, SWMI_TB_SLOTS, tb_lds, tile, nullptr, 1u);
}

// mode 1, before the walks: the pair's maximum cells are listed, and the first span of each walk is prepared at the
// same time.  The sweep left one maximum per checkpoint window; a window whose maximum equals the pair's is a candidate.
//   * one candidate (the usual case): wave 0 re-sweeps it with the cell test on, the other waves re-sweep the windows
//     below it, so the span a single alignment's walk starts in is complete when the cell list is;
//   * 2..4 candidates: wave w re-sweeps candidate w (cells into its own quarter of the pair's cell list), the remaining
//     waves the windows below their team's candidate.  If every candidate holds exactly ONE maximum cell the quarters
//     are compacted and walker w starts in its own window; otherwise the generic path below runs;
//   * generic: wave 0 re-sweeps all candidates one after the other (detect_cells).
// On return the workgroup has passed a barrier, shared[0] = number of cells, shared[3] = 1 if every walker's first span
// is staged; the return value is this wave's first staged block (~0: none).  shared[24..27] / [28..31]: per candidate
// cell count / first staged block.
template <int R>
__device__ __forceinline__ uint32_t winmax_detect(const TraceArgs &A, const PairDesc pd, PairOut &po, const uint32_t lane,
                                                  const uint32_t wave, const uint32_t n_waves, const uint32_t ccap,
                                                  uint32_t *__restrict__ tiles, uint32_t *__restrict__ walker_lds,
                                                  const uint32_t per_walker, volatile uint32_t *__restrict__ shared) {
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const bool acgt = rd.acgt && qd.acgt && SWMI_SCORES_FIT(A);
    const StripGeom G = strip_geom<R>(m, n, 1u);
    constexpr uint32_t WIN_WORDS = SWMI_CK_BLOCKS * SWMI_RMAX * WAVE;
    uint32_t ncand = 0, gc[SWMI_TB_SLOTS] = {0u, 0u, 0u, 0u};
    if (G.n_strips == 1u) {
        const uint32_t *__restrict__ wm = A.dir + pd.dir_off + G.wmax_off;
        for (uint32_t g0 = 0; g0 < G.n_ck; g0 += WAVE) {
            const uint32_t g = g0 + lane;
            const int wv = g < G.n_ck ? (int)wm[g] : -1;
            uint64_t cand = BALLOT(wv == po.score);
            while (cand) {
                const uint32_t gg = g0 + (uint32_t)__builtin_ctzll(cand);
                cand &= cand - 1ull;
                if (ncand == 0u) gc[0] = gg; else if (ncand == 1u) gc[1] = gg; else if (ncand == 2u) gc[2] = gg; else if (ncand == 3u) gc[3] = gg;
                ++ncand;
            }
        }
    }
    auto stage_ref = [&](uint32_t *__restrict__ dst, uint32_t wlo, uint32_t nwin) {
        const int clo = (int)(16u * wlo) - 63;
        const uint32_t cw0 = clo > 0 ? (uint32_t)clo >> 2 : 0u;
        const uint32_t cw1 = (16u * (wlo + nwin * SWMI_CK_BLOCKS) - 1u) >> 2;
        for (uint32_t x = cw0 + lane; x <= cw1 && x < (n + 3u) / 4u; x += WAVE) dst[x - cw0] = refw[x];
    };
    auto publish = [&](uint32_t cnt, uint32_t staged) {      // wave 0, after the cells are listed
        if (lane == 0) {
            po.n_cells = cnt;
            if (cnt > ccap) po.flags |= SWMI_F_CELL_OVF;
            A.out[pd.out_id] = po;
            if (A.out_host) A.out_host[pd.out_id] = po;
            shared[0] = cnt;
            shared[3] = staged;
        }
        if (lane < SWMI_TB_SLOTS) { shared[7u + 4u * lane] = 0u; shared[20u + lane] = 0u; }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the cell list has left the CU before the others read it
    };
    const uint64_t cbase = A.cells_off ? A.cells_off[pd.out_id] : (uint64_t)pd.out_id * A.cell_cap;
    uint2 *__restrict__ cells = const_cast<uint2 *>(A.cells) + cbase;

    const uint32_t seg = ccap / SWMI_TB_SLOTS;
    if (ncand >= 2u && ncand <= SWMI_TB_SLOTS && ncand <= n_waves && seg >= 1u) {
        const uint32_t nw = ncand, ts = n_waves / nw;
        if (wave < nw) {
            const uint32_t g = wave == 0u ? gc[0] : wave == 1u ? gc[1] : wave == 2u ? gc[2] : gc[3];
            const uint32_t nq0 = g + 1u < ts ? g + 1u : ts;
            const uint32_t wlo0 = (g + 1u - nq0) * SWMI_CK_BLOCKS;
            uint32_t *my = walker_lds + wave * per_walker;
            for (uint32_t w = lane; w < (m + 3u) / 4u; w += WAVE) my[A.lds_words + w] = readw[w];
            stage_ref(my + A.lds_words + A.lds_read_words, wlo0, nq0);
            const uint32_t c = replay_any<R, true, false>(A, pd, n, m, acgt, refw, readw, G, 0u, g * SWMI_CK_BLOCKS, lane,
                                                   tiles + wave * ts * WIN_WORDS + (nq0 - 1u) * SWMI_CK_BLOCKS * R * WAVE,
                                                   po.score, 0u, cells + wave * seg, seg);
            if (lane == 0) { shared[24u + wave] = c; shared[28u + wave] = wlo0; }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            const uint32_t team = (wave - nw) % nw, q = 1u + (wave - nw) / nw;
            const uint32_t g = team == 0u ? gc[0] : team == 1u ? gc[1] : team == 2u ? gc[2] : gc[3];
            const uint32_t nq0 = g + 1u < ts ? g + 1u : ts;
            if (q < nq0)
                (void)replay_any<R, false, false>(A, pd, n, m, acgt, refw, readw, G, 0u, (g - q) * SWMI_CK_BLOCKS, lane,
                                           tiles + team * ts * WIN_WORDS + (nq0 - 1u - q) * SWMI_CK_BLOCKS * R * WAVE,
                                           0, 0u, nullptr, 0u);
        }
        __syncthreads();
        bool one_each = true;
        for (uint32_t w = 0; w < nw; ++w) one_each = one_each && shared[24u + w] == 1u;
        if (one_each) {
            if (wave == 0) {
                uint2 c = make_uint2(0, 0);
                if (lane < nw) { c.x = ld_l2(&cells[lane * seg].x); c.y = ld_l2(&cells[lane * seg].y); }
                if (lane < nw) cells[lane] = c;
                publish(nw, 1u);
            }
            __syncthreads();
            return wave < nw ? shared[28u + wave] : 0xFFFFFFFFu;
        }
        __syncthreads();                                     // everybody has read the counts before wave 0 reuses shared[]
    }

    const bool pre = ncand == 1u;
    const uint32_t nq0 = gc[0] + 1u < n_waves ? gc[0] + 1u : n_waves;             // windows of the span that ends with window gc[0]
    const uint32_t wlo0 = (gc[0] + 1u - nq0) * SWMI_CK_BLOCKS;
    if (wave == 0) {
        if (n_waves == 1u) {                                 // nobody else to do it
            for (uint32_t w = lane; w < (m + 3u) / 4u; w += WAVE) walker_lds[A.lds_words + w] = readw[w];
            if (pre) stage_ref(walker_lds + A.lds_words + A.lds_read_words, wlo0, nq0);
        }
        const uint32_t cnt = detect_cells<R, false>(A, pd, po, lane, pre ? tiles + (nq0 - 1u) * SWMI_CK_BLOCKS * R * WAVE : tiles);
        publish(cnt, (pre && cnt == 1u) ? 1u : 0u);       // (the candidate's window doubles as the first window of the walk)
    } else {
        // the read's codes for the walkers: wave w fills walker w's copy, the last wave also walker 0's
        if (wave < SWMI_TB_SLOTS)
            for (uint32_t w = lane; w < (m + 3u) / 4u; w += WAVE) walker_lds[wave * per_walker + A.lds_words + w] = readw[w];
        if (wave == n_waves - 1u)
            for (uint32_t w = lane; w < (m + 3u) / 4u; w += WAVE) walker_lds[A.lds_words + w] = readw[w];
        if (pre) {
            if (wave < nq0)
                (void)replay_any<R, false, false>(A, pd, n, m, acgt, refw, readw, G, 0u, wlo0 + (wave - 1u) * SWMI_CK_BLOCKS, lane,
                                           tiles + (wave - 1u) * SWMI_CK_BLOCKS * R * WAVE, 0, 0u, nullptr, 0u);
            if (wave == n_waves - 1u) stage_ref(walker_lds + A.lds_words + A.lds_read_words, wlo0, nq0);
        }
    }
    __syncthreads();
    return (pre && wave == 0) ? wlo0 : 0xFFFFFFFFu;
}

// mode 1: one workgroup of SWMI_TB_WAVES waves = ONE pair.  Wave 0 first lists the maximum cells (detect_cells),
// the workgroup meets at a barrier, then min(cells, 4) waves walk the alignments and the others help them.
// (4 waves per SIMD = at most 128 VGPRs: at the headline the 1000 workgroups of four waves must ALL be resident, or the launch
//  grows a second round of workgroups -- at 130 VGPRs it took 0.092 ms instead of 0.073)
extern "C" __global__ void __launch_bounds__(WAVE * SWMI_TB_WAVES) __attribute__((amdgpu_waves_per_eu(4, 4)))
sw_traceback_winmax_kernel(const TraceArgs A) {
    extern __shared__ uint32_t wm_lds[];
    const uint32_t pair = blockIdx.x;
    if (pair >= A.n_pairs) return;
    // (rotating the walker role over the hardware waves, in case wave w always landed on SIMD w, changes nothing)
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const PairDesc pd = A.pairs[pair];
    PairOut po = A.out[pd.out_id];
    if (finish_pair(A, pd, po) && wave == 0 && lane == 0) A.out[pd.out_id] = po;
    if (po.flags & (SWMI_F_DEGENERATE | SWMI_F_DONE)) {      // (DONE: sw_resident_pairs_kernel did the whole pair) same decision in every wave: nobody waits at the barrier
        if (A.out_host && wave == 0 && lane == 0) A.out_host[pd.out_id] = po;
        return;
    }
    // LDS: [32 shared words][tiles: one window per wave][per walker: ops staging, read codes, reference window]
    const uint32_t n_waves = blockDim.x >> 6;
    const uint32_t per_walker = A.lds_words + A.lds_read_words + SWMI_TB_REFWIN_WORDS;
    constexpr uint32_t WIN_WORDS = SWMI_CK_BLOCKS * SWMI_RMAX * WAVE;
    uint32_t *shared = wm_lds;
    uint32_t *tiles = wm_lds + 32;
    const uint32_t R = swmi_rows_per_lane(A.reads[pd.read_id].len);
    const uint32_t ccap = A.cells_cap ? A.cells_cap[pd.out_id] : A.cell_cap;
    // (A.pad2: the launcher reserved a SECOND set of window tiles for speculative staging -- traceback_pair)
    const uint32_t tile_sets = A.pad2 ? 2u : 1u;
    uint32_t *tiles2 = A.pad2 ? tiles + n_waves * WIN_WORDS : nullptr;
    uint32_t *walker_lds0 = tiles + tile_sets * n_waves * WIN_WORDS;
    if (!swmi_common_pair(A, A.refs[pd.ref_id], A.reads[pd.read_id])) {
        // a byte alphabet, the DistributedSW tie order or a read of several strips: the plain scheme -- wave 0 lists the
        // cells, then up to four independent walkers, one window at a time -- with every kernel variant available
        if (wave == 0) {
            uint32_t c;
            if (R == 1)      c = detect_cells<1>(A, pd, po, lane, tiles);
            else if (R == 2) c = detect_cells<2>(A, pd, po, lane, tiles);
            else if (R == 3) c = detect_cells<3>(A, pd, po, lane, tiles);
            else             c = detect_cells<4>(A, pd, po, lane, tiles);
            if (lane == 0) {
                po.n_cells = c;
                if (c > ccap) po.flags |= SWMI_F_CELL_OVF;
                A.out[pd.out_id] = po;
                if (A.out_host) A.out_host[pd.out_id] = po;
                shared[0] = c;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the cell list has left the CU before the others read it
        }
        __syncthreads();
        const uint32_t c = shared[0];
        uint32_t nwr = c < SWMI_TB_SLOTS ? c : SWMI_TB_SLOTS;
        if (nwr > n_waves) nwr = n_waves;
        if (c > ccap || wave >= nwr) return;
        po.n_cells = c;
        uint32_t *lds = walker_lds0 + wave * per_walker;
        uint32_t *tile = tiles + wave * WIN_WORDS;
        if (R == 1)      traceback_pair<1, 1, false>(A, pd, po, lane, wave, nwr, lds, tile, nullptr, 1u);
        else if (R == 2) traceback_pair<2, 1, false>(A, pd, po, lane, wave, nwr, lds, tile, nullptr, 1u);
        else if (R == 3) traceback_pair<3, 1, false>(A, pd, po, lane, wave, nwr, lds, tile, nullptr, 1u);
        else             traceback_pair<4, 1, false>(A, pd, po, lane, wave, nwr, lds, tile, nullptr, 1u);
        return;
    }
    uint32_t pre_wlo;
    if (R == 1)      pre_wlo = winmax_detect<1>(A, pd, po, lane, wave, n_waves, ccap, tiles, walker_lds0, per_walker, shared);
    else if (R == 2) pre_wlo = winmax_detect<2>(A, pd, po, lane, wave, n_waves, ccap, tiles, walker_lds0, per_walker, shared);
    else if (R == 3) pre_wlo = winmax_detect<3>(A, pd, po, lane, wave, n_waves, ccap, tiles, walker_lds0, per_walker, shared);
    else             pre_wlo = winmax_detect<4>(A, pd, po, lane, wave, n_waves, ccap, tiles, walker_lds0, per_walker, shared);
    const uint32_t cnt = shared[0];                                    // (winmax_detect ends with a barrier)
    if (shared[3] != 1u) pre_wlo = 0xFFFFFFFFu;                        // no staged first spans
    if (cnt > ccap || cnt == 0u) return;
    po.n_cells = cnt;
    uint32_t nw = cnt < SWMI_TB_SLOTS ? cnt : SWMI_TB_SLOTS;           // walkers = teams
    if (nw > n_waves) nw = n_waves;                                    // (a one-wave workgroup walks its alignments one after the other)
    const uint32_t ts = n_waves / nw;                                  // waves (= windows per round) per team
    if (ts == 1u) {
        // no helpers to share the re-sweeps with: the walkers run independently, one window at a time
        if (wave >= nw) return;
        uint32_t *lds = walker_lds0 + wave * per_walker;
        uint32_t *tile = tiles + wave * WIN_WORDS;
        if (R == 1)      traceback_pair<1, 1, false, false>(A, pd, po, lane, wave, nw, lds, tile, nullptr, 1u, pre_wlo, true);
        else if (R == 2) traceback_pair<2, 1, false, false>(A, pd, po, lane, wave, nw, lds, tile, nullptr, 1u, pre_wlo, true);
        else if (R == 3) traceback_pair<3, 1, false, false>(A, pd, po, lane, wave, nw, lds, tile, nullptr, 1u, pre_wlo, true);
        else             traceback_pair<4, 1, false, false>(A, pd, po, lane, wave, nw, lds, tile, nullptr, 1u, pre_wlo, true);
        return;
    }
    if (wave < nw) {
        uint32_t *lds = walker_lds0 + wave * per_walker;
        uint32_t *tile = tiles + wave * ts * WIN_WORDS;
        uint32_t *tile2 = tiles2 ? tiles2 + wave * ts * WIN_WORDS : nullptr;
        if (R == 1)      traceback_pair<1, 1, true, false>(A, pd, po, lane, wave, nw, lds, tile, shared, ts, pre_wlo, true, nullptr, tile2);
        else if (R == 2) traceback_pair<2, 1, true, false>(A, pd, po, lane, wave, nw, lds, tile, shared, ts, pre_wlo, true, nullptr, tile2);
        else if (R == 3) traceback_pair<3, 1, true, false>(A, pd, po, lane, wave, nw, lds, tile, shared, ts, pre_wlo, true, nullptr, tile2);
        else             traceback_pair<4, 1, true, false>(A, pd, po, lane, wave, nw, lds, tile, shared, ts, pre_wlo, true, nullptr, tile2);
    } else {
        if (R == 1)      coop_helper<1>(A, pd, lane, wave, nw, ts, n_waves, tiles, shared);
        else if (R == 2) coop_helper<2>(A, pd, lane, wave, nw, ts, n_waves, tiles, shared);
        else if (R == 3) coop_helper<3>(A, pd, lane, wave, nw, ts, n_waves, tiles, shared);
        else             coop_helper<4>(A, pd, lane, wave, nw, ts, n_waves, tiles, shared);
    }
}

extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES)
sw_traceback_kernel(const TraceArgs A) {
    extern __shared__ uint32_t tb_lds[];
    traceback_entry<0>(A, tb_lds);
}

extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES)
sw_traceback_replay_kernel(const TraceArgs A) {
    extern __shared__ uint32_t tb_lds[];
    traceback_entry<1>(A, tb_lds);
}

// ------------------------------------------------------------------------------------------------
// split traceback (mode 1): for batches whose pairs carry many tied maxima (periodic references: the reference's own
// EngineerData sets, one tied maximum per period) or that have few pairs, one workgroup per pair is the wrong grain --
// a 128 kbp periodic reference against one read is ONE pair with 1600 alignments.  Here the grain is the window and
// the alignment:
//   sw_detect_windows_kernel  one wavefront per checkpoint window of every pair: a window whose maximum equals the
//                             pair's is re-swept with the cell test on; its cells go to the pair's list (slots reserved
//                             by one atomicAdd, any order: the host orders a pair's records by cell) and one walk item
//                             per cell to a global queue;
//   sw_walk_items_kernel      a fixed grid of wavefronts shares the queue (item w, w + W, ...): one alignment per
//                             wavefront, windows re-swept one at a time.
// ------------------------------------------------------------------------------------------------
#define SWMI_SPLIT_WAVES 4u

extern "C" __global__ void __launch_bounds__(WAVE * SWMI_SPLIT_WAVES)
sw_detect_windows_kernel(const TraceArgs A) {
    extern __shared__ uint32_t dw_lds[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t item = blockIdx.x * SWMI_SPLIT_WAVES + wave;
    const uint32_t n_items = A.win_off[A.n_pairs];
    if (item >= n_items) return;
    // the pair this window belongs to: last p with win_off[p] <= item
    uint32_t lo = 0, hi = A.n_pairs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.win_off[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t pair = lo, wloc = item - A.win_off[pair];
    const PairDesc pd = A.pairs[pair];
    PairOut po = A.out[pd.out_id];
    if (finish_pair(A, pd, po) && wloc == 0u && lane == 0) A.out[pd.out_id] = po;     // (window 0's wave completes the record)
    if (po.flags & (SWMI_F_DEGENERATE | SWMI_F_DONE)) return;                          // (DONE: sw_resident_pairs_kernel did the whole pair)
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t R = swmi_rows_per_lane(m);
    const uint64_t wblocks = ((uint64_t)n + 63u + 15u) / 16u;
    const uint32_t n_ck = (uint32_t)((wblocks + SWMI_CK_BLOCKS - 1u) / SWMI_CK_BLOCKS);
    const uint32_t strip = wloc / n_ck, g = wloc - strip * n_ck;
    const uint64_t wmax_off = (uint64_t)n_ck * (R + 2) * WAVE;
    const uint64_t strip_words = wmax_off + (uint64_t)((n_ck + 63u) & ~63u);
    if ((int)A.dir[pd.dir_off + strip * strip_words + wmax_off + g] != po.score) return;

    // this wave's scratch: the re-swept window (direction bits nobody reads here) and the cells it finds
    constexpr uint32_t WIN_WORDS = SWMI_CK_BLOCKS * SWMI_RMAX * WAVE;
    uint32_t *tile = dw_lds + wave * (WIN_WORDS + 2u * SWMI_DETECT_LCAP);
    uint2 *found = reinterpret_cast<uint2 *>(tile + WIN_WORDS);
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const bool acgt = rd.acgt && qd.acgt && SWMI_SCORES_FIT(A);
    uint32_t cnt;
    if (R == 1)      { const StripGeom G = strip_geom<1>(m, n, 1u); cnt = replay_any<1, true>(A, pd, n, m, acgt, refw, readw, G, strip, g * SWMI_CK_BLOCKS, lane, tile, po.score, 0u, found, SWMI_DETECT_LCAP); }
    else if (R == 2) { const StripGeom G = strip_geom<2>(m, n, 1u); cnt = replay_any<2, true>(A, pd, n, m, acgt, refw, readw, G, strip, g * SWMI_CK_BLOCKS, lane, tile, po.score, 0u, found, SWMI_DETECT_LCAP); }
    else if (R == 3) { const StripGeom G = strip_geom<3>(m, n, 1u); cnt = replay_any<3, true>(A, pd, n, m, acgt, refw, readw, G, strip, g * SWMI_CK_BLOCKS, lane, tile, po.score, 0u, found, SWMI_DETECT_LCAP); }
    else             { const StripGeom G = strip_geom<4>(m, n, 1u); cnt = replay_any<4, true>(A, pd, n, m, acgt, refw, readw, G, strip, g * SWMI_CK_BLOCKS, lane, tile, po.score, 0u, found, SWMI_DETECT_LCAP); }
    if (cnt == 0u) return;                                   // (pad rows can make a window's maximum a value no real cell holds)
    WAVE_SYNC();
    const uint64_t cbase = A.cells_off ? A.cells_off[pd.out_id] : (uint64_t)pd.out_id * A.cell_cap;
    const uint32_t ccap = A.cells_cap ? A.cells_cap[pd.out_id] : A.cell_cap;
    unsigned long long base = 0;
    uint32_t qbase = 0;
    const uint32_t have = cnt < SWMI_DETECT_LCAP ? cnt : SWMI_DETECT_LCAP;
    if (lane == 0) {
        base = atomicAdd((unsigned long long *)&A.out[pd.out_id].n_cells, (unsigned long long)cnt);
        const bool fits = cnt <= SWMI_DETECT_LCAP && base + cnt <= (unsigned long long)ccap;
        if (fits) {
            qbase = atomicAdd(A.q_count, have);
            if (qbase + have > A.q_cap) qbase = 0xFFFFFFFFu;
        } else {
            qbase = 0xFFFFFFFFu;
        }
        if (qbase == 0xFFFFFFFFu) atomicOr(&A.out[pd.out_id].flags, SWMI_F_CELL_OVF);     // the host re-runs the pair with exact sizes
    }
    base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    qbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)qbase);
    if (qbase == 0xFFFFFFFFu) return;
    uint2 *__restrict__ cells = const_cast<uint2 *>(A.cells) + cbase;
    for (uint32_t c = lane; c < have; c += WAVE) {
        const uint2 cell = found[c];
        cells[base + c] = cell;
        A.q_items[qbase + c] = make_uint4(pair, cell.x, cell.y, 0u);
    }
}

extern "C" __global__ void __launch_bounds__(WAVE * SWMI_SPLIT_WAVES)
sw_walk_items_kernel(const TraceArgs A) {
    extern __shared__ uint32_t wi_lds[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * SWMI_SPLIT_WAVES + wave, n_waves = gridDim.x * SWMI_SPLIT_WAVES;
    // zero-copy results: the pair outputs are final (the detect kernel ended one launch ago)
    if (A.out_host)
        for (uint32_t p = gw * WAVE + lane; p < A.n_pairs; p += n_waves * WAVE) A.out_host[p] = A.out[p];
    uint32_t n_items = *A.q_count;
    if (n_items > A.q_cap) n_items = A.q_cap;
    constexpr uint32_t WIN_WORDS = SWMI_CK_BLOCKS * SWMI_RMAX * WAVE;
    const uint32_t per_wave = A.lds_words + A.lds_read_words + SWMI_TB_REFWIN_WORDS + WIN_WORDS;
    uint32_t *lds = wi_lds + wave * per_wave;
    uint32_t *tile = lds + A.lds_words + A.lds_read_words + SWMI_TB_REFWIN_WORDS;
    for (uint32_t it = gw; it < n_items; it += n_waves) {
        const uint4 item = A.q_items[it];
        const PairDesc pd = A.pairs[item.x];
        PairOut po = A.out[pd.out_id];
        if (po.flags & (SWMI_F_DEGENERATE | SWMI_F_CELL_OVF)) continue;         // (an overflowed pair is re-run as a whole)
        const uint32_t R = swmi_rows_per_lane(A.reads[pd.read_id].len);
        if (R == 1)      traceback_pair<1, 1, false>(A, pd, po, lane, 0u, 1u, lds, tile, nullptr, 1u, 0xFFFFFFFFu, false, &item);
        else if (R == 2) traceback_pair<2, 1, false>(A, pd, po, lane, 0u, 1u, lds, tile, nullptr, 1u, 0xFFFFFFFFu, false, &item);
        else if (R == 3) traceback_pair<3, 1, false>(A, pd, po, lane, 0u, 1u, lds, tile, nullptr, 1u, 0xFFFFFFFFu, false, &item);
        else             traceback_pair<4, 1, false>(A, pd, po, lane, 0u, 1u, lds, tile, nullptr, 1u, 0xFFFFFFFFu, false, &item);
        WAVE_SYNC();
    }
}

extern "C" hipError_t swmi_launch_traceback_split(const TraceArgs *a, uint32_t n_windows, hipStream_t st) {
    if (a->n_pairs == 0) return hipSuccess;
    const size_t win = (size_t)SWMI_CK_BLOCKS * SWMI_RMAX * WAVE;
    const size_t det_words = SWMI_SPLIT_WAVES * (win + 2u * SWMI_DETECT_LCAP);
    if (n_windows)
        hipLaunchKernelGGL(sw_detect_windows_kernel, dim3((n_windows + SWMI_SPLIT_WAVES - 1) / SWMI_SPLIT_WAVES), dim3(WAVE * SWMI_SPLIT_WAVES),
                           det_words * sizeof(uint32_t), st, *a);
    const size_t per_wave = (size_t)a->lds_words + a->lds_read_words + SWMI_TB_REFWIN_WORDS + win;
    // enough wavefronts to fill the chip several times over, but no more workgroups than there can be items
    uint32_t groups = (a->q_cap + SWMI_SPLIT_WAVES - 1) / SWMI_SPLIT_WAVES;
    if (groups > 2048u) groups = 2048u;
    if (groups < 1u) groups = 1u;
    hipLaunchKernelGGL(sw_walk_items_kernel, dim3(groups), dim3(WAVE * SWMI_SPLIT_WAVES), SWMI_SPLIT_WAVES * per_wave * sizeof(uint32_t), st, *a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// resident pairs (mode 1): a pair whose WHOLE 2-bit direction field fits a wavefront's share of LDS -- the reference's
// own benchmark shapes, 80 bp reads against 400 bp references (EngineerData.java:51-224) -- is handled start to finish
// by one wavefront, with nothing but its result leaving the CU:
//   A  score sweep (the 3-VALU cells of sweep_fast), one maximum per 32-step window kept in LDS -> the pair's maximum;
//   B  second sweep with direction bits (the same cell stream the replay uses) into LDS, with the cell test switched on
//      in the windows whose maximum equals the pair's -> the tied maximum cells, listed in LDS;
//   C  ALL alignments walked at once, one LANE each: a lane chases its own path through the field in LDS (three LDS
//      reads and ~35 VALU per step for up to 64 alignments together), tracking the score like SmithWaterman.java:380-409,
//      packing its ops into its own scratch row; the wave then reserves arena space with one atomicAdd and the lanes
//      copy their records out.  Periodic references give every pair a handful of alignments: they cost one walk, not five.
// No checkpoints, no HBM workspace.  The host orders a pair's records by cell (SWMI_RANK_BY_CELL).
// LDS per wavefront (dwords): field [wblocks*R*64] | window maxima [n_ck] | cells [2*cell_cap] | ops [64*ops_words] |
//                             reference codes [(n+3)/4+1] | read codes [(m+3)/4+1] | string scratch [128]
// ------------------------------------------------------------------------------------------------
template <int R, bool STRICT>
__device__ __forceinline__ void resident_pair(const TraceArgs &A, const ResidentArgs &X, const PairDesc pd, const uint32_t lane, uint32_t *__restrict__ lds) {
    const SeqDesc rd = A.refs[pd.ref_id];
    const SeqDesc qd = A.reads[pd.read_id];
    const uint32_t n = rd.len, m = qd.len;
    const uint32_t *__restrict__ refw = A.seqw + rd.boff;
    const uint32_t *__restrict__ readw = A.seqw + qd.boff;
    const uint32_t lact = (m + R - 1) / R;                                  // one strip: m <= 64 * R
    const uint32_t lane_eff = lane < lact ? lane : 0x40000000u;
    const uint32_t T = n + lact - 1, nblk = (T + 15u) / 16u, n_ck = (nblk + SWMI_CK_BLOCKS - 1u) / SWMI_CK_BLOCKS;
    uint32_t *field = lds;                                                  // [nblk][R][64]
    uint32_t *wmaxs = field + nblk * R * WAVE;
    uint2 *cells = reinterpret_cast<uint2 *>(wmaxs + ((n_ck + 1u) & ~1u));
    uint32_t *opsb = reinterpret_cast<uint32_t *>(cells + X.res_cell_cap);
    uint32_t *refc = opsb + WAVE * X.res_ops_words;
    uint32_t *readc = refc + (n + 3u) / 4u + 1u;
    uint32_t *scratch = readc + (m + 3u) / 4u + 1u;                         // [SWMI_EMIT_SCRATCH_WORDS] 256 characters of both strings
    for (uint32_t w = lane; w < (n + 3u) / 4u; w += WAVE) refc[w] = refw[w];
    for (uint32_t w = lane; w < (m + 3u) / 4u; w += WAVE) readc[w] = readw[w];
    const uint4 *__restrict__ refq = reinterpret_cast<const uint4 *>(refw);

    // ---- A: scores only ---------------------------------------------------------------------------------------------
    int pair_max = 0;
    {
        const uint32_t gm = (uint32_t)(-(int64_t)A.gap);
        const int one = 1;
        SweepState<R> S;
        build_profiles<R>(S.q, readw, lane * R, m, A.match, A.mismatch);
#pragma unroll
        for (int k = 0; k < R; ++k) { S.h[k] = 0; S.g[k] = 0; S.hp[k] = 0; }
        S.lmax = -1;
        uint4 wnext = refq[0];
        S.rby = 0;
        S.rbx = wave_shr1((int)(1u << (wnext.x & 31u)), 0);
        for (uint32_t tb = 0; tb < nblk; ++tb) {
            const uint4 w = wnext;
            wnext = refq[tb + 1];
            if ((tb % SWMI_CK_BLOCKS) == 0u && tb > 0u) {
                const int wm = wave_max_i32(lane < lact ? S.lmax : -1);
                if (lane == 0) wmaxs[tb / SWMI_CK_BLOCKS - 1u] = (uint32_t)wm;
                pair_max = pair_max > wm ? pair_max : wm;
                S.lmax = -1;
            }
            const uint32_t t0 = 16u * tb;
#ifndef SWMI_NO_ASM
            if (t0 + 15u < n) {
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
        const int wm = wave_max_i32(lane < lact ? S.lmax : -1);
        if (lane == 0) wmaxs[(nblk - 1u) / SWMI_CK_BLOCKS] = (uint32_t)wm;
        pair_max = pair_max > wm ? pair_max : wm;
    }
    PairOut po;
    if (pair_max <= 0) {                                                   // every cell ties at 0: SmithWaterman.java:154,182-185
        po.score = 0; po.flags = SWMI_F_DEGENERATE | SWMI_F_DONE; po.n_cells = (uint64_t)m * n;
        if (lane == 0) { A.out[pd.out_id] = po; if (A.out_host) A.out_host[pd.out_id] = po; }
        return;
    }
    WAVE_SYNC();

    // ---- B: direction bits into LDS, the cells equal to the maximum listed on the way ----------------------------------
    uint32_t ncell;
    {
        FillState<R> S;
        S.thr = pair_max; S.cnt = 0; S.ev_prev = 0; S.events = 0; S.dbg_skip = false; S.lmax = -1;
        setup_rows<R, true>(S, readw, lane * R, m, A.match, A.mismatch);
        uint4 wnext = refq[0];
        for (uint32_t tb = 0; tb < nblk; ++tb) {
            const uint4 w = wnext;
            wnext = refq[tb + 1];
            const uint32_t t0 = 16u * tb;
            const bool steady = (t0 + 1u >= lact) && (t0 + 15u < n);
            const bool hot = (int)wmaxs[tb / SWMI_CK_BLOCKS] == pair_max;       // (wave-uniform: an LDS word)
            if (hot) {
                if (steady) fill_block16<R, true, STRICT, false, false, SWMI_MODE_DETECT>(S, w, t0, lane, lane_eff, n, m, lane * R, A.gap, A.match, A.mismatch,
                                                                                          0, false, false, nullptr, cells, X.res_cell_cap);
                else        fill_block16<R, true, STRICT, false, true, SWMI_MODE_DETECT>(S, w, t0, lane, lane_eff, n, m, lane * R, A.gap, A.match, A.mismatch,
                                                                                         0, false, false, nullptr, cells, X.res_cell_cap);
            } else {
                if (steady) fill_block16<R, true, STRICT, false, false, SWMI_MODE_REPLAY>(S, w, t0, lane, lane_eff, n, m, lane * R, A.gap, A.match, A.mismatch,
                                                                                          0, false, false, nullptr, nullptr, 0u);
                else        fill_block16<R, true, STRICT, false, true, SWMI_MODE_REPLAY>(S, w, t0, lane, lane_eff, n, m, lane * R, A.gap, A.match, A.mismatch,
                                                                                         0, false, false, nullptr, nullptr, 0u);
            }
            const int miss = (int)(t0 + 15u) - ((int)(lane + n) - 1);           // a lane past its last column still owes the missing shifts
#pragma unroll
            for (int k = 0; k < R; ++k) {
                uint32_t v = S.acc[k];
                if (miss > 0 && miss < 16) v <<= 2 * miss;
                field[(tb * R + k) * WAVE + lane] = v;
            }
        }
        ncell = S.cnt;
    }
    po.score = pair_max; po.flags = SWMI_F_DONE | (ncell > X.res_cell_cap ? SWMI_F_CELL_OVF : 0u); po.n_cells = ncell;
    if (lane == 0) { A.out[pd.out_id] = po; if (A.out_host) A.out_host[pd.out_id] = po; }
    if (ncell > X.res_cell_cap || ncell == 0u) return;            // (too many: the host re-runs the pair through the ordinary path)
    WAVE_SYNC();

    // ---- C: one lane per alignment ----------------------------------------------------------------------------------
    const uint8_t *ref_b = reinterpret_cast<const uint8_t *>(refc);
    const uint8_t *read_b = reinterpret_cast<const uint8_t *>(readc);
    const uint32_t umat = (uint32_t)A.match, umis = (uint32_t)A.mismatch, ugap = (uint32_t)A.gap;
    const uint32_t max_ops = 16u * X.res_ops_words;
    for (uint32_t base = 0; base < ncell; base += WAVE) {
        const bool mine = base + lane < ncell;
        const uint2 c0 = mine ? cells[base + lane] : make_uint2(0u, 0u);
        uint32_t i = c0.x, j = c0.y, score = (uint32_t)pair_max, nops = 0, cur = 0;
        int begin = 0;
        bool active = mine;
        uint32_t *my_ops = opsb + lane * X.res_ops_words;
        while (BALLOT(active)) {
            if (active) {
                const uint32_t rho = i - 1u, l = rho / R, k = rho - l * R;
                const uint32_t t = j - 1u + l;
                const uint32_t dw = field[((t >> 4) * R + k) * WAVE + l];
                const uint32_t rc = ref_b[j - 1u], qc = read_b[i - 1u];
                const uint32_t d = (dw >> (2u * (15u - (t & 15u)))) & 3u;
                const bool isA = (d & 1u) != 0u, isI = d == 2u;
                begin = (int)j;                                                  // SmithWaterman.java:383
                score -= isA ? (rc == qc ? umat : umis) : ugap;                  // :388-406, H(pred) = H - delta
                const uint32_t op = isA ? SWMI_DIR_A : (isI ? SWMI_DIR_I : SWMI_DIR_D);
                cur |= op << (2u * (nops & 15u));
                ++nops;
                if ((nops & 15u) == 0u) { if (nops <= max_ops) my_ops[(nops >> 4) - 1u] = cur; cur = 0; }
                i -= (isA || isI) ? 1u : 0u;
                j -= (isA || !isI) ? 1u : 0u;
                active = (int)score > 0 && i != 0u && j != 0u;                   // `while (score > 0)` :380
            }
        }
        if ((nops & 15u) != 0u && nops <= max_ops) my_ops[nops >> 4] = cur;
        WAVE_SYNC();
        // records: table entries + payloads (packed ops [+ strings]), contiguous for the whole wave
        const uint32_t opw = A.raw ? 0u : (nops + 15u) / 16u;                // (records with strings carry no ops)
        const uint32_t words = mine ? swmi_payload_words(nops, A.raw != nullptr) : 0u;
        const uint32_t incl = wave_scan_add_u32(words);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t nhere = ncell - base < WAVE ? ncell - base : WAVE;
        unsigned long long off;
        uint32_t rslot;
        const bool fits = swmi_reserve(A, lane, total, nhere, off, rslot);
        const bool too_long = BALLOT(mine && nops > max_ops) != 0ull;
        if (fits && !too_long) {
            if (mine) {
                uint32_t *dst = A.arena + off + (incl - words);
                swmi_write_rec(A, rslot + lane, pd.out_id, SWMI_RANK_BY_CELL, begin, c0.x, c0.y, nops, off + (incl - words));
                for (uint32_t w = 0; w < opw; ++w) dst[w] = my_ops[w];
            }
            if (A.raw) {
                // the strings (SmithWaterman.java:418-431): one alignment after the other, the whole wavefront on each
                const uint8_t *__restrict__ raw_ref = A.raw + A.raw_off[pd.ref_id];
                const uint8_t *__restrict__ raw_read = A.raw + A.raw_off[A.raw_reads_at + pd.read_id];
                for (uint32_t a = 0; a < nhere; ++a) {
                    const uint32_t na = (uint32_t)__builtin_amdgcn_readlane((int)nops, (int)a);
                    const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)(incl - words), (int)a);
                    const uint32_t ai = (uint32_t)__builtin_amdgcn_readlane((int)c0.x, (int)a);
                    const uint32_t aj = (uint32_t)__builtin_amdgcn_readlane((int)c0.y, (int)a);
                    swmi_emit_strings(A.arena + off + at, SwmiOpsPacked{opsb + a * X.res_ops_words},
                                      na, ai, aj, raw_ref, raw_read, lane, scratch);
                }
            }
        } else if (lane == 0) {
            atomicOr(&A.out[pd.out_id].flags, SWMI_F_ARENA_OVF);
            if (A.ovf_host) *A.ovf_host = 1u;
        }
        WAVE_SYNC();
    }
}

extern "C" __global__ void __launch_bounds__(WAVE * FILL_WAVES)
sw_resident_pairs_kernel(const TraceArgs A, const ResidentArgs X) {
    extern __shared__ uint32_t rp_lds[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t item = blockIdx.x * FILL_WAVES + wave;
    if (item >= X.n_res) return;
    // (the arena header was reset by sw_sweep_winmax_kernel, one launch earlier; the traceback kernels append after this one)
    const PairDesc pd = A.pairs[X.res_items[item]];
    uint32_t *lds = rp_lds + wave * X.res_lds_words;
    const uint32_t R = swmi_rows_per_lane(A.reads[pd.read_id].len);
    if (A.strict) {
        if (R == 1)      resident_pair<1, true>(A, X, pd, lane, lds);
        else if (R == 2) resident_pair<2, true>(A, X, pd, lane, lds);
        else if (R == 3) resident_pair<3, true>(A, X, pd, lane, lds);
        else             resident_pair<4, true>(A, X, pd, lane, lds);
    } else {
        if (R == 1)      resident_pair<1, false>(A, X, pd, lane, lds);
        else if (R == 2) resident_pair<2, false>(A, X, pd, lane, lds);
        else if (R == 3) resident_pair<3, false>(A, X, pd, lane, lds);
        else             resident_pair<4, false>(A, X, pd, lane, lds);
    }
}

extern "C" hipError_t swmi_launch_resident(const TraceArgs *a, const ResidentArgs *x, hipStream_t st) {
    if (x->n_res == 0) return hipSuccess;
    static const bool attr = [] { swmi_allow_big_lds(sw_resident_pairs_kernel); return true; }();
    (void)attr;
    hipLaunchKernelGGL(sw_resident_pairs_kernel, dim3((x->n_res + FILL_WAVES - 1) / FILL_WAVES), dim3(WAVE * FILL_WAVES),
                       (size_t)FILL_WAVES * x->res_lds_words * sizeof(uint32_t), st, *a, *x);
    return hipGetLastError();
}

extern "C" hipError_t swmi_launch_traceback(const TraceArgs *a, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (a->n_pairs == 0) return hipSuccess;
    const size_t tile = (size_t)(a->mode == 0 ? SWMI_TB_BLOCKS : SWMI_CK_BLOCKS) * SWMI_RMAX * WAVE;
    const size_t per_wave = (size_t)a->lds_words + a->lds_read_words + SWMI_TB_REFWIN_WORDS + tile;
    const dim3 block(WAVE * FILL_WAVES);
    if (a->mode == 1) {
        // 8 waves per pair (bigger teams, shorter critical path) while every workgroup of the launch can be resident
        // at once (4 waves per SIMD at this kernel's register count), else 4.  Big batches are throughput-bound: there a
        // helper wave that mostly waits only takes a slot another pair's walker could use, so every pair gets ONE wave
        // (it lists the cells, then walks the alignments one after the other).
        static int forced = getenv("SWMI_TB_WAVES") ? atoi(getenv("SWMI_TB_WAVES")) : 0;
        static int big = getenv("SWMI_TB_BIG") ? atoi(getenv("SWMI_TB_BIG")) : 10000;   // measured crossover: between 8 k and 16 k pairs
        const uint32_t n_waves = forced ? (uint32_t)forced : (a->n_pairs <= 512u ? SWMI_TB_WAVES : a->n_pairs <= (uint32_t)big ? 4u : 1u);
        const size_t n_walkers = n_waves < SWMI_TB_SLOTS ? n_waves : SWMI_TB_SLOTS;
        const size_t tiles = (size_t)n_waves * SWMI_CK_BLOCKS * SWMI_RMAX * WAVE;
        size_t words = 32 + tiles + n_walkers * ((size_t)a->lds_words + a->lds_read_words + SWMI_TB_REFWIN_WORDS);
        // speculative staging (traceback_pair): a second set of tiles, while teams have helpers and the block still fits.
        // Measured (profiles/r03/ab_spec_staging.txt): 250 pairs 0.0554 -> 0.0491 ms, 500 pairs 0.0600 -> 0.0593, 1000 pairs
        // 0.0735 -> 0.0768 -- from about 500 pairs on the SIMDs are shared by the waves of several pairs and the helpers'
        // extra re-sweeps (a span whose walk ends early is wasted) cost other pairs' walkers more than the waits they save.
        static const int spec_opt = getenv("SWMI_TB_SPEC") ? atoi(getenv("SWMI_TB_SPEC")) : 1;      // 0 never, 1 automatic, 2 always
        TraceArgs t = *a;
        t.pad2 = (spec_opt && (spec_opt == 2 || a->n_pairs <= 384u) && n_waves > 1u && (words + tiles) * sizeof(uint32_t) <= 160u * 1024u) ? 1u : 0u;
        if (t.pad2) words += tiles;
        if (ev_start && ev_stop)
            hipExtLaunchKernelGGL(sw_traceback_winmax_kernel, dim3(a->n_pairs), dim3(WAVE * n_waves), (uint32_t)(words * sizeof(uint32_t)), st, ev_start, ev_stop, 0u, t);
        else
            hipLaunchKernelGGL(sw_traceback_winmax_kernel, dim3(a->n_pairs), dim3(WAVE * n_waves), words * sizeof(uint32_t), st, t);
    } else {
        const dim3 grid((a->n_pairs + FILL_WAVES - 1) / FILL_WAVES, SWMI_TB_SLOTS);
        if (a->mode == 0) hipLaunchKernelGGL(sw_traceback_kernel, grid, block, per_wave * FILL_WAVES * sizeof(uint32_t), st, *a);
        else              hipLaunchKernelGGL(sw_traceback_replay_kernel, grid, block, per_wave * FILL_WAVES * sizeof(uint32_t), st, *a);
    }
    return hipGetLastError();
}
