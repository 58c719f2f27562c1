// swmi_subopt.hip -- gfx950 kernels of options "subopt"  and "hits" (8p): a local pair's second-best score, or its K best
// separated end cells, from its row of column maxima.
//
// The local sweeps of such a run (swmi_affine.hip, SUBOPT = 1) leave colmax(j), the maximum of H over column j, for every column
// the pair's sweep reached: one int32 per column behind the pair's direction fields (swmi_device.h: swmi_aff_pair_table_off is where
// the row starts, swmi_aff_colmax_cols where it ends).  With s the pair's score and w the mask half-width (swmi.h):
//   j* is a maximum column iff colmax(j*) == s;  column j is eligible iff |j - j*| > w for every maximum column;
//   score2 = the largest colmax over the eligible columns (0: none),  end2 = the smallest eligible column that holds it (0: none).
//
// sw_subopt_kernel: ONE WAVEFRONT PER PAIR, 64 columns per step, ONE ascending pass that only reads the row (so the kernel may run
//   again over the same workspace: the traceback's retry does).  A column's nearest maximum column on either side decides it:
//     left   a maximum column of this step at or below the lane (ballot, the highest such bit), else L, the last one of the steps
//            before -- a wave-uniform value carried along
//     right  a maximum column of this step at or above the lane (the lowest such bit), else `nxt`, the first one behind this step --
//            found by a LOOKAHEAD that searches the row from the step's end on, four loads in flight per lane, and is kept until the
//            pass has moved beyond it.  The search resumes where it stopped, so it reads the row once more in total, plus at most
//            three steps of 64 per maximum column found.
//   A lane keeps its first strictly larger eligible value (its columns ascend); the wave takes the maximum and then the smallest
//   column among the lanes that hold it, both through wave_max_i32, as the "band_adapt" pass does for p(s).  The main pass has four
//   loads in flight per lane as well.  All column arithmetic is in 64 bits: j + w may pass 2^31.
//   A degenerate pair (score 0) writes (0, 0) without touching the row; a pair with an empty side is not part of any launch.
//
// sw_hits_kernel (option "hits"): IN PLACE OF sw_subopt_kernel on a run with hits = K.  One wavefront per pair, read-only on
//   the pair's two rows -- colmax(j) and, swmi_aff_colmax_stride(n) dwords behind it, row(j), the smallest row that holds it.
//     entry 0    (s, row(j0), j0), j0 the first maximum column: one ascending search, four loads in flight per lane
//     entry k    one round of the pass above, in which a column must ALSO lie more than w from the end column of every entry 1 .. k - 1.
//                Lane q keeps entry q's column; a round tests them with one readlane each, in 64 bits.  The round ends with the
//                wave_max_i32 pair: the maximum, then the smallest column among its holders.  A round that finds 0 ends the list.
//   Entry 1 is (score2, end2): the kernel writes the pair's SuboptOut too, and runs that round even when K = 1.  row(j) is loaded for
//   the chosen column only.  Lanes 0 .. K - 1 store one 16-byte entry each behind the count, plain vector stores; entries past the
//   count are zero.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "swmi_device.h"
#include "swmi_launch.h"
#include "swmi_wave.h"

#define SUB_WAVES 4                    // wavefronts (= pairs) per workgroup

extern "C" __global__ void __launch_bounds__(WAVE * SUB_WAVES) sw_subopt_kernel(const SuboptArgs A) {
    const uint32_t pair = blockIdx.x * SUB_WAVES + (threadIdx.x >> 6);
    if (pair >= A.n_pairs) return;
    const uint32_t lane = threadIdx.x & 63u;
    const PairDesc pd = A.pairs[pair];
    const PairOut po = A.out[pd.out_id];
    const uint32_t n = uni(A.refs[pd.ref_id].len), m = uni(A.reads[pd.read_id].len);
    SuboptOut res;
    res.score2 = 0; res.end2 = 0u;
    const int s = (int)uni((uint32_t)po.score);
    if (!(uni(po.flags) & SWMI_F_DEGENERATE) && s > 0 && m && n) {
        const int64_t w = A.subopt < 0 ? (int64_t)(m / 2u > 15u ? m / 2u : 15u) : (int64_t)A.subopt;
        const uint32_t cols = swmi_aff_colmax_cols(m, n, A.band);
        const int *const row = reinterpret_cast<const int *>(A.dir + pd.dir_off + swmi_aff_pair_table_off(m, n, AffGeom{A.band, false, false, true}));
        const int64_t FAR = (int64_t)1 << 40;                    // no maximum column on that side: further than any w
        int64_t L = -FAR;                                        // the last maximum column before this step (0-based, as every column here)
        int64_t nxt = -1;                                        // the first maximum column at or behind the end of the step it was searched for
        uint32_t scan = 0u;                                      // where the lookahead goes on (a multiple of 64)
        int bv = 0;                                              // the lane's best eligible value (> 0 only) and its first column
        uint32_t bc = 0u;
        const auto step = [&](const uint32_t base, const int v) {
            const uint32_t j = base + lane, end = base + WAVE;
            const bool valid = j < cols;
            const uint64_t mk = BALLOT(valid && v == s);
            if (nxt < (int64_t)end) {
                if (scan < end) scan = end;
                nxt = FAR;
                while (scan < cols) {
                    const uint32_t i0 = scan + lane, i1 = i0 + WAVE, i2 = i1 + WAVE, i3 = i2 + WAVE;
                    const int u0 = i0 < cols ? row[i0] : -1, u1 = i1 < cols ? row[i1] : -1;
                    const int u2 = i2 < cols ? row[i2] : -1, u3 = i3 < cols ? row[i3] : -1;
                    const uint64_t b0 = BALLOT(u0 == s), b1 = BALLOT(u1 == s), b2 = BALLOT(u2 == s), b3 = BALLOT(u3 == s);
                    // (scan stays at the step of the column found: the next search starts behind the pass, which is then beyond it)
                    if (b0) { nxt = (int64_t)scan + __builtin_ctzll(b0); break; }
                    if (b1) { scan += WAVE; nxt = (int64_t)scan + __builtin_ctzll(b1); break; }
                    if (b2) { scan += 2u * WAVE; nxt = (int64_t)scan + __builtin_ctzll(b2); break; }
                    if (b3) { scan += 3u * WAVE; nxt = (int64_t)scan + __builtin_ctzll(b3); break; }
                    scan += 4u * WAVE;
                }
            }
            const uint64_t ml = mk & (~0ull >> (63u - lane)), mr = mk & (~0ull << lane);
            const int64_t lcol = ml ? (int64_t)base + 63 - __builtin_clzll(ml) : L;
            const int64_t rcol = mr ? (int64_t)base + __builtin_ctzll(mr) : nxt;
            if (valid && (int64_t)j - lcol > w && rcol - (int64_t)j > w && v > bv) { bv = v; bc = j; }
            if (mk) L = (int64_t)base + 63 - __builtin_clzll(mk);
        };
        uint32_t base = 0u;
        for (; base + 3u * WAVE < cols; base += 4u * WAVE) {
            // (the last of the four may run past the row's end: guarded)
            const uint32_t j3 = base + 3u * WAVE + lane;
            const int v0 = row[base + lane], v1 = row[base + WAVE + lane], v2 = row[base + 2u * WAVE + lane], v3 = j3 < cols ? row[j3] : -1;
            step(base, v0);
            step(base + WAVE, v1);
            step(base + 2u * WAVE, v2);
            step(base + 3u * WAVE, v3);
        }
        for (; base < cols; base += WAVE) {
            const uint32_t j = base + lane;
            step(base, j < cols ? row[j] : -1);
        }
        const int smax = wave_max_i32(bv);
        if (smax > 0) {
            // the smallest column among the lanes that hold the maximum (bc < 2^31: its negative orders them)
            const uint32_t p = (uint32_t)(-wave_max_i32(bv == smax ? -(int)bc : INT32_MIN));
            res.score2 = smax;
            res.end2 = p + 1u;
        }
    }
    if (lane == 0) {
        A.sub[pd.out_id] = res;
        if (A.sub_host) A.sub_host[pd.out_id] = res;             // results straight into pinned host memory
    }
}

// One round of sw_hits_kernel: sw_subopt_kernel's pass with the end columns of the entries 1 .. nprev - 1 (0-based, in lanes 1 ..
// nprev - 1 of pj) masked as well.  Returns the largest eligible column maximum (0: none) and the smallest column that holds it.
__device__ __forceinline__ void hits_round(const int *__restrict__ row, const uint32_t cols, const int s, const int64_t w, const uint32_t lane,
                                           const int pj, const uint32_t nprev, int &smax_out, uint32_t &col_out) {
    const int64_t FAR = (int64_t)1 << 40;
    int64_t L = -FAR, nxt = -1;
    uint32_t scan = 0u;
    int bv = 0;
    uint32_t bc = 0u;
    const auto step = [&](const uint32_t base, const int v) {
        const uint32_t j = base + lane, end = base + WAVE;
        const bool valid = j < cols;
        const uint64_t mk = BALLOT(valid && v == s);
        if (nxt < (int64_t)end) {
            if (scan < end) scan = end;
            nxt = FAR;
            while (scan < cols) {
                const uint32_t i0 = scan + lane, i1 = i0 + WAVE, i2 = i1 + WAVE, i3 = i2 + WAVE;
                const int u0 = i0 < cols ? row[i0] : -1, u1 = i1 < cols ? row[i1] : -1;
                const int u2 = i2 < cols ? row[i2] : -1, u3 = i3 < cols ? row[i3] : -1;
                const uint64_t b0 = BALLOT(u0 == s), b1 = BALLOT(u1 == s), b2 = BALLOT(u2 == s), b3 = BALLOT(u3 == s);
                if (b0) { nxt = (int64_t)scan + __builtin_ctzll(b0); break; }
                if (b1) { scan += WAVE; nxt = (int64_t)scan + __builtin_ctzll(b1); break; }
                if (b2) { scan += 2u * WAVE; nxt = (int64_t)scan + __builtin_ctzll(b2); break; }
                if (b3) { scan += 3u * WAVE; nxt = (int64_t)scan + __builtin_ctzll(b3); break; }
                scan += 4u * WAVE;
            }
        }
        const uint64_t ml = mk & (~0ull >> (63u - lane)), mr = mk & (~0ull << lane);
        const int64_t lcol = ml ? (int64_t)base + 63 - __builtin_clzll(ml) : L;
        const int64_t rcol = mr ? (int64_t)base + __builtin_ctzll(mr) : nxt;
        bool ok = valid && (int64_t)j - lcol > w && rcol - (int64_t)j > w && v > bv;
        // the earlier entries' end columns (wave-uniform values, one readlane each); only while some lane still has a candidate
        if (BALLOT(ok) != 0ull) {
            for (uint32_t q = 1u; q < nprev; ++q) {
                const int64_t d = (int64_t)j - (int64_t)__builtin_amdgcn_readlane(pj, (int)q);
                ok = ok && (d > w || -d > w);
            }
        }
        if (ok) { bv = v; bc = j; }
        if (mk) L = (int64_t)base + 63 - __builtin_clzll(mk);
    };
    uint32_t base = 0u;
    for (; base + 3u * WAVE < cols; base += 4u * WAVE) {
        const uint32_t j3 = base + 3u * WAVE + lane;
        const int v0 = row[base + lane], v1 = row[base + WAVE + lane], v2 = row[base + 2u * WAVE + lane], v3 = j3 < cols ? row[j3] : -1;
        step(base, v0);
        step(base + WAVE, v1);
        step(base + 2u * WAVE, v2);
        step(base + 3u * WAVE, v3);
    }
    for (; base < cols; base += WAVE) {
        const uint32_t j = base + lane;
        step(base, j < cols ? row[j] : -1);
    }
    const int smax = wave_max_i32(bv);
    smax_out = smax;
    // the smallest column among the lanes that hold the maximum (bc < 2^31: its negative orders them)
    col_out = smax > 0 ? (uint32_t)(-wave_max_i32(bv == smax ? -(int)bc : INT32_MIN)) : 0u;
}

extern "C" __global__ void __launch_bounds__(WAVE * SUB_WAVES) sw_hits_kernel(const HitsArgs H) {
    const SuboptArgs &A = H.s;
    const uint32_t pair = blockIdx.x * SUB_WAVES + (threadIdx.x >> 6);
    if (pair >= A.n_pairs) return;
    const uint32_t lane = threadIdx.x & 63u;
    const PairDesc pd = A.pairs[pair];
    const PairOut po = A.out[pd.out_id];
    const uint32_t n = uni(A.refs[pd.ref_id].len), m = uni(A.reads[pd.read_id].len);
    const uint32_t K = H.k;
    SuboptOut res;
    res.score2 = 0; res.end2 = 0u;
    uint32_t nh = 0u;                                            // the entries found
    HitEnt mine;                                                 // lane q: entry q
    mine.score = 0; mine.end_i = 0u; mine.end_j = 0u; mine.reserved = 0u;
    const int s = (int)uni((uint32_t)po.score);
    if (!(uni(po.flags) & SWMI_F_DEGENERATE) && s > 0 && m && n) {
        const int64_t w = A.subopt < 0 ? (int64_t)(m / 2u > 15u ? m / 2u : 15u) : (int64_t)A.subopt;
        const uint32_t cols = swmi_aff_colmax_cols(m, n, A.band);
        const int *const row = reinterpret_cast<const int *>(A.dir + pd.dir_off + swmi_aff_pair_table_off(m, n, AffGeom{A.band, false, false, true, true}));
        const int *const rrow = row + swmi_aff_colmax_stride(n);
        // entry 0: the first maximum column (there is one: s > 0 is some column's maximum)
        uint32_t j0 = 0xFFFFFFFFu;
        for (uint32_t base = 0u; base < cols && j0 == 0xFFFFFFFFu; base += 4u * WAVE) {
            const uint32_t i0 = base + lane, i1 = i0 + WAVE, i2 = i1 + WAVE, i3 = i2 + WAVE;
            const int u0 = i0 < cols ? row[i0] : -1, u1 = i1 < cols ? row[i1] : -1;
            const int u2 = i2 < cols ? row[i2] : -1, u3 = i3 < cols ? row[i3] : -1;
            const uint64_t b0 = BALLOT(u0 == s), b1 = BALLOT(u1 == s), b2 = BALLOT(u2 == s), b3 = BALLOT(u3 == s);
            if (b0) j0 = base + (uint32_t)__builtin_ctzll(b0);
            else if (b1) j0 = base + WAVE + (uint32_t)__builtin_ctzll(b1);
            else if (b2) j0 = base + 2u * WAVE + (uint32_t)__builtin_ctzll(b2);
            else if (b3) j0 = base + 3u * WAVE + (uint32_t)__builtin_ctzll(b3);
        }
        if (j0 != 0xFFFFFFFFu) {
            const uint32_t r0 = (uint32_t)rrow[j0];
            if (lane == 0u) { mine.score = s; mine.end_i = r0; mine.end_j = j0 + 1u; }
            nh = 1u;
            int pj = 0;                                          // lane q, q >= 1: the 0-based end column of entry q
            const uint32_t rounds = K > 2u ? K : 2u;             // (entry 1 is the pair's SuboptOut, whatever K is)
            for (uint32_t k = 1u; k < rounds; ++k) {
                int smax;
                uint32_t p;
                hits_round(row, cols, s, w, lane, pj, k, smax, p);
                if (smax <= 0) break;
                if (k == 1u) { res.score2 = smax; res.end2 = p + 1u; }
                if (k < K) {
                    const uint32_t rk = (uint32_t)rrow[p];
                    if (lane == k) { mine.score = smax; mine.end_i = rk; mine.end_j = p + 1u; pj = (int)p; }
                    nh = k + 1u;
                }
            }
        }
    }
    HitEnt *const dst = H.hits + (uint64_t)pd.out_id * (1u + K);
    HitEnt *const dsth = H.hits_host ? H.hits_host + (uint64_t)pd.out_id * (1u + K) : nullptr;
    if (lane == 0) {
        HitEnt hd;
        hd.score = (int32_t)nh; hd.end_i = 0u; hd.end_j = 0u; hd.reserved = 0u;
        A.sub[pd.out_id] = res;
        dst[0] = hd;
        if (A.sub_host) A.sub_host[pd.out_id] = res;             // results straight into pinned host memory
        if (dsth) dsth[0] = hd;
    }
    if (lane < K) {
        dst[1u + lane] = mine;
        if (dsth) dsth[1u + lane] = mine;
    }
}

// ------------------------------------------------------------------------------------------------
// host-callable launcher
// ------------------------------------------------------------------------------------------------
extern "C" hipError_t swmi_launch_subopt(const SuboptArgs *a, hipStream_t st) {
    if (a->n_pairs == 0) return hipSuccess;
    if (a->subopt == 0 || a->subopt < -1 || a->subopt > (1 << 30) || a->band > SWMI_AFF_BAND_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_subopt_kernel, dim3((a->n_pairs + SUB_WAVES - 1) / SUB_WAVES), dim3(WAVE * SUB_WAVES), 0, st, *a);
    return hipGetLastError();
}

extern "C" hipError_t swmi_launch_hits(const HitsArgs *a, hipStream_t st) {
    if (a->s.n_pairs == 0) return hipSuccess;
    if (a->s.subopt == 0 || a->s.subopt < -1 || a->s.subopt > (1 << 30) || a->s.band > SWMI_AFF_BAND_MAX || a->k < 1u || a->k > SWMI_HITS_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_hits_kernel, dim3((a->s.n_pairs + SUB_WAVES - 1) / SUB_WAVES), dim3(WAVE * SUB_WAVES), 0, st, *a);
    return hipGetLastError();
}
