// swmi_launch.h -- the host-callable launchers of the gfx950 kernels (internal).  Included by every .hip file that defines
// one and by the host units that call one, so that the compiler checks each definition against the prototype its callers
// see (an `extern "C"` mismatch would otherwise link and break at run time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "swmi_device.h"

// Allow `kernel` the whole 160 KB of a CU's LDS as dynamic shared memory (the default limit is 64 KB).  A launcher calls it
// once per process, behind a static guard of its own.
template <class K>
static inline void swmi_allow_big_lds(K kernel) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

extern "C" hipError_t swmi_launch_fill(const FillArgs *a, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);
extern "C" hipError_t swmi_launch_traceback(const TraceArgs *a, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop);
extern "C" hipError_t swmi_launch_traceback_split(const TraceArgs *a, uint32_t n_windows, hipStream_t st);
extern "C" hipError_t swmi_launch_resident(const TraceArgs *a, const ResidentArgs *x, hipStream_t st);
extern "C" hipError_t swmi_launch_tfused(const TraceArgs *a, const TFusedArgs *x, hipStream_t st);
extern "C" hipError_t swmi_launch_affine_sweep(const FillArgs *a, int32_t gap_open, uint32_t align_mode, const uint32_t *mat, uint32_t nn,
                                               uint32_t r_min, uint32_t r_max, uint32_t long_reads, uint32_t band, uint32_t xdrop,
                                               uint32_t band_adapt, int32_t gap_open2, int32_t gap2, hipStream_t st);
extern "C" hipError_t swmi_launch_affine_traceback(const TraceArgs *a, uint32_t align_mode, uint32_t long_reads, uint32_t band, uint32_t band_adapt,
                                                   uint32_t two, uint32_t tile_words, uint32_t ops_words, hipStream_t st);
extern "C" hipError_t swmi_launch_encode(const uint8_t *raw, const uint64_t *raw_off, SeqDesc *desc, uint32_t *seqw,
                                         const uint8_t *lut, uint32_t n_seq, hipStream_t st);
