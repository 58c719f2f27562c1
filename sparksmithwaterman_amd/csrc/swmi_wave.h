// swmi_wave.h -- wavefront-level helpers shared by the kernel units (swmi_sweep.hip, swmi_traceback.hip,
// swmi_affine.hip, swmi_tfused.hip): lane-to-lane moves and reductions through
// the DPP network, ballots, wave-uniform values, loads that bypass L1.  Device code only; everything is __forceinline__.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define WAVE 64
#define BALLOT(pred) __builtin_amdgcn_ballot_w64(pred)
// LDS hand-offs between lanes of ONE wavefront: DS operations of a wave execute in order, so a compiler-level
// fence is all that is needed (a workgroup barrier would deadlock the fused kernel's 4 independent waves)
#define WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------
// v_mov_b32_dpp wave_shr:1 : lane l receives lane l-1's value, lane 0 keeps `old`.
__device__ __forceinline__ int wave_shr1(int old, int src) {
    return __builtin_amdgcn_update_dpp(old, src, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
}
// same, lane 0 receives 0 (bound_ctrl)
__device__ __forceinline__ int wave_shr1_zero(int src) {
    return __builtin_amdgcn_update_dpp(0, src, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
}

// wave-wide signed max through the DPP network (no LDS): 4 row steps, 2 row broadcasts, result read from lane 63.
// The DPP modifier sits on the v_max itself (a lane without a source lane, or outside the row mask, is simply not written: it
// keeps its value, which is what max(v, v) gave before): 6 VALU + the wait states a DPP read of a just-written register
// needs, where `update_dpp` + max compiled to a copy, a v_mov_b32_dpp and a v_max per step -- 24 instructions per window
// close of the sweep, 0.4 per anti-diagonal step.
__device__ __forceinline__ int wave_max_i32(int v) {
#ifndef SWMI_NO_ASM
    asm volatile("s_nop 1\n\t"
                 "v_max_i32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
                 "v_max_i32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
                 "v_max_i32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
                 "v_max_i32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"      // lane 15 of every row holds the row's max
                 "v_max_i32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"   // into rows 1 and 3
                 "v_max_i32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"         // into rows 2 and 3: lane 63 holds the wave's max
                 : "+v"(v));
#else
#define SWMI_DPP_MAX(ctrl, rmask)                                                          \
    { int o_ = __builtin_amdgcn_update_dpp(v, v, ctrl, rmask, 0xf, false); v = v > o_ ? v : o_; }
    SWMI_DPP_MAX(0x111, 0xf)   // row_shr:1
    SWMI_DPP_MAX(0x112, 0xf)   // row_shr:2
    SWMI_DPP_MAX(0x114, 0xf)   // row_shr:4
    SWMI_DPP_MAX(0x118, 0xf)   // row_shr:8   -> lane 15 of every row holds the row's max
    SWMI_DPP_MAX(0x142, 0xa)   // row_bcast:15 into rows 1 and 3
    SWMI_DPP_MAX(0x143, 0xc)   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's max
#undef SWMI_DPP_MAX
#endif
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ uint32_t lanemask_lt_count(uint64_t mask) {
    // number of set bits of `mask` below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// load served by L2 (bypasses this CU's L1): for data another wave -- or this wave, earlier -- stored in the same launch
__device__ __forceinline__ uint32_t ld_l2(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A value every lane of the wave holds alike, moved to a scalar register: what hangs on it (loop bounds, branches,
// base addresses) then runs on the scalar unit instead of as exec-masked vector code.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v); }

__device__ __forceinline__ uint32_t seq_code(const uint32_t *__restrict__ w, uint32_t pos) {
    return (w[pos >> 2] >> (8u * (pos & 3u))) & 0xFFu;
}

__device__ __forceinline__ uint32_t wave_scan_add_u32(uint32_t v) {          // inclusive prefix sum over the 64 lanes (DPP)
#define SWMI_DPP_ADD(ctrl, rmask, bmask)                                                     \
    { const uint32_t o_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, bmask, true); v += o_; }
    SWMI_DPP_ADD(0x111, 0xf, 0xf)   // row_shr:1
    SWMI_DPP_ADD(0x112, 0xf, 0xf)   // row_shr:2
    SWMI_DPP_ADD(0x114, 0xf, 0xf)   // row_shr:4
    SWMI_DPP_ADD(0x118, 0xf, 0xf)   // row_shr:8  -> inclusive scan inside every row of 16
    SWMI_DPP_ADD(0x142, 0xa, 0xf)   // row_bcast:15 -> rows 1 and 3 add the total of the row before
    SWMI_DPP_ADD(0x143, 0xc, 0xf)   // row_bcast:31 -> rows 2 and 3 add the total of rows 0-1
#undef SWMI_DPP_ADD
    return v;
}
