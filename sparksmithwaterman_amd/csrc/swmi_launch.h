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
// What the two launchers of the affine kernels (swmi_affine.hip) need from a run's options.  The host runtime builds one per run
// (aff_run in swmi_run.cpp, the only place) and passes the same one to the launch of the short shape and of the long shape.
struct AffRun {
    int32_t gap_open;            // a gap of length k costs gap_open + k * gap
    int32_t gap_open2, gap2;     // option "gap_open2" (0: none) and "gap2": the two-piece kernels
    uint32_t mode;               // 0 local, 1 fit, 2 global (option "align_mode"), 3 extend (option "extend" on a global run)
    uint32_t band;               // option "band": the half-width (0: none) -- the banded strip kernels
    uint32_t xdrop;              // option "xdrop": the threshold (0: none) -- the strip sweep that may stop at a seam
    uint32_t adapt;              // option "band_adapt" (0 / 1) -- the banded strip kernels whose windows follow the alignment
    const uint32_t *mat;         // the device image of the score matrix (swmi_aff_mat_words dwords), or null: the plain sweeps
    uint32_t nn;                 // ... and its side n + 1 (2 .. SWMI_MAT_NN_MAX)
    uint32_t cigar;              // option "cigar" (0: off; 1: M/I/D, 2: =/X/I/D) -- the payload the walks write (swmi_emit.h); the sweeps do not read it
    int32_t subopt;              // option "subopt" (0: off; 1 .. 2^30: the mask half-width, -1: per pair) -- the local sweeps that leave the column maxima
    uint32_t hits;               // option "hits" (0: off; 1 .. 16 = K, with subopt only) -- the local sweeps that leave the maxima's rows as well
    uint32_t end_bonus;          // option "end_bonus" (0: off; 1 .. 2^30: the bonus) -- the extend sweeps that also choose the read's end
};
// What the launchers refuse (hipErrorInvalidValue): the combinations no kernel exists for.  band, xdrop and adapt are options of
// the long shape (long_reads: every pair of the launch has a read longer than SWMI_AFF_MAX_READ); the short shape ignores them.
// Every run check_run_params (swmi_run.cpp) admits passes.
static inline bool aff_run_ok(const AffRun &r, uint32_t long_reads) {
    if (r.mode > 3u || r.band > SWMI_AFF_BAND_MAX || r.xdrop > 0x7FFFFFFFu || r.adapt > 1u || r.cigar > 2u) return false;
    if (r.mat && (r.nn < 2u || r.nn > SWMI_MAT_NN_MAX)) return false;
    if (r.gap_open2 && (r.mode < 2u || r.mat || r.xdrop || r.adapt)) return false;      // two-piece: plain global and extend runs
    if (r.subopt < -1 || r.subopt > (1 << 30) || (r.subopt && r.mode != 0u)) return false;   // subopt: local runs
    if (r.hits > SWMI_HITS_MAX || (r.hits && !r.subopt)) return false;                   // hits: runs under subopt
    // end_bonus: one-piece extend runs without xdrop or band_adapt
    if (r.end_bonus > (1u << 30) || (r.end_bonus && (r.mode != 3u || r.xdrop || r.adapt || r.gap_open2 || r.subopt))) return false;
    if (long_reads && r.xdrop && r.mode != 3u) return false;                            // xdrop: extend runs
    if (long_reads && r.adapt && (!r.band || r.mode != 3u)) return false;               // band_adapt: banded extend runs
    return true;
}
// long_reads 0: the pairs with reads of at most SWMI_AFF_MAX_READ bases; r_min / r_max: the rows per lane of the launch's shortest
// and longest read (the narrow and the wide sweep: only the one that has pairs is launched).  long_reads 1: the strip kernels.
extern "C" hipError_t swmi_launch_affine_sweep(const FillArgs *a, const AffRun *r, uint32_t long_reads, uint32_t r_min, uint32_t r_max,
                                               hipStream_t st);
// tile_words, ops_words: the LDS dwords of a wavefront's direction tile and of its packed ops
extern "C" hipError_t swmi_launch_affine_traceback(const TraceArgs *a, const AffRun *r, uint32_t long_reads, uint32_t tile_words,
                                                   uint32_t ops_words, hipStream_t st);
// Option "subopt" (swmi_subopt.hip): sw_subopt_kernel, one wavefront per pair of the launch -- the short and the long shape alike --
// behind the sweeps on the same stream.  It reads the pair's score and its row of column maxima (behind the pair's fields in `dir`,
// swmi_device.h) and writes (score2, end2) as swmi.h defines them.
struct SuboptArgs {
    const SeqDesc *refs, *reads;
    const PairDesc *pairs;
    const uint32_t *dir;         // the launch's workspace
    const PairOut *out;          // the sweeps' pair outputs, by out_id
    SuboptOut *sub;              // per out_id, device memory
    SuboptOut *sub_host;         // zero-copy results: its host-mapped mirror, or null
    uint32_t n_pairs;
    uint32_t band;               // option "band" (0: none): it shapes the fields the row lies behind, and ends the row
    int32_t subopt;              // the mask half-width, or -1: max(m / 2, 15) per pair
};
extern "C" hipError_t swmi_launch_subopt(const SuboptArgs *a, hipStream_t st);
// Option "hits" (swmi_subopt.hip): sw_hits_kernel IN PLACE OF sw_subopt_kernel on such a run, one wavefront per pair.  It reads the
// pair's score and its two rows -- the column maxima and, swmi_aff_colmax_stride(n) dwords behind, their rows -- and writes the pair's
// SuboptOut as sw_subopt_kernel would and its 1 + K HitEnt (swmi_device.h).
struct HitsArgs {
    SuboptArgs s;                // as for sw_subopt_kernel
    HitEnt *hits;                // (1 + k) entries per out_id, device memory
    HitEnt *hits_host;           // zero-copy results: its host-mapped mirror, or null
    uint32_t k;                  // option "hits": 1 .. SWMI_HITS_MAX
};
extern "C" hipError_t swmi_launch_hits(const HitsArgs *a, hipStream_t st);
extern "C" hipError_t swmi_launch_encode(const uint8_t *raw, const uint64_t *raw_off, SeqDesc *desc, uint32_t *seqw,
                                         const uint8_t *lut, uint32_t n_seq, hipStream_t st);
// pair lists: the segments' images (and the raw bytes of reversed segments) from the resident sources (sw_gather_kernel)
extern "C" hipError_t swmi_launch_gather(uint8_t *raw, const uint64_t *src_off, const uint64_t *raw_off, SeqDesc *desc, uint32_t *seqw,
                                         const uint8_t *lut, uint32_t n_seg, hipStream_t st);
