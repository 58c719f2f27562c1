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
    uint32_t mode;               // 0 local, 1 fit, 2 global (option "align_mode"), 3 extend (option "extend" on a global run), 4 overlap (option "overlap" on a fit run)
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
// The flags word of an affine kernel: the 0/1 columns of the kernel lists of swmi_affine.hip (AFF_SWEEPS, AFF_TRACEBACKS), the
// template argument of the device functions there and, with the mode and the shape, the key a launcher finds a kernel by.
enum : uint32_t {
    AFF_F_MATRIX = 1u << 0, AFF_F_LONG = 1u << 1, AFF_F_BAND = 1u << 2, AFF_F_XDROP = 1u << 3, AFF_F_ADAPT = 1u << 4,
    AFF_F_TWO = 1u << 5, AFF_F_SUBOPT = 1u << 6, AFF_F_ENDB = 1u << 7, AFF_F_HITS = 1u << 8,
    // per-read score profiles (swmi_batch_set_read_profiles): a bit of the device templates' flags word alone.  It is
    // no argument of aff_flags and no part of a key -- aff_key has no free bit below the mode -- so the profile sweeps have a table
    // and a launcher of their own, keyed by shape and mode.
    AFF_F_PROFILE = 1u << 16
};
constexpr uint32_t aff_flags(bool matrix, bool lng, bool band, bool xdrop, bool adapt, bool two, bool subopt, bool endb, bool hits) {
    return (matrix ? AFF_F_MATRIX : 0u) | (lng ? AFF_F_LONG : 0u) | (band ? AFF_F_BAND : 0u) | (xdrop ? AFF_F_XDROP : 0u) |
           (adapt ? AFF_F_ADAPT : 0u) | (two ? AFF_F_TWO : 0u) | (subopt ? AFF_F_SUBOPT : 0u) | (endb ? AFF_F_ENDB : 0u) | (hits ? AFF_F_HITS : 0u);
}
// shape: 0 narrow (1 .. 4 rows per lane), 1 wide (5 .. 16), 2 long (the strip sweeps); the walks have one shape, 0
// (nine flag bits, three bits of mode -- 0 .. 4 -- then the shape)
constexpr uint32_t aff_key(uint32_t shape, uint32_t mode, uint32_t flags) { return flags | mode << 9 | shape << 12; }
// The combinations a kernel may exist for (mode: 0 local, 1 fit, 2 global, 3 extend, 4 overlap).  Every row of the kernel lists and
// every device entry static_asserts it; aff_run_ok refuses a run by it.
constexpr bool aff_flags_ok(uint32_t mode, uint32_t f) {
    const bool xdrop_or_adapt = f & (AFF_F_XDROP | AFF_F_ADAPT);
    if (mode > 4u) return false;
    if (f & AFF_F_PROFILE) return f == AFF_F_PROFILE;                                    // profiles: the five short one-piece sweeps, nothing else
    if (mode == 4u) return !(f & ~(AFF_F_MATRIX | AFF_F_LONG));                          // overlap: a score matrix and long reads, nothing else
    if ((f & AFF_F_BAND) && !(f & AFF_F_LONG)) return false;                             // band: the strip sweeps
    if ((f & AFF_F_XDROP) && !((f & AFF_F_LONG) && mode == 3u)) return false;            // xdrop: the strip sweeps of an extend run
    if ((f & AFF_F_ADAPT) && !((f & AFF_F_BAND) && mode == 3u)) return false;            // band_adapt: the banded ones
    if ((f & AFF_F_TWO) && (mode < 2u || (f & AFF_F_MATRIX) || xdrop_or_adapt)) return false;    // two-piece: plain global and extend runs
    if ((f & AFF_F_SUBOPT) && mode != 0u) return false;                                  // subopt: local runs
    if ((f & AFF_F_HITS) && !(f & AFF_F_SUBOPT)) return false;                           // hits: runs under subopt
    if ((f & AFF_F_ENDB) && (mode != 3u || xdrop_or_adapt || (f & AFF_F_TWO))) return false;     // end_bonus: one-piece extend runs
    return true;
}
// The flags of a run's kernels.  band, xdrop and adapt are options of the long shape (long_reads: every pair of the launch has a
// read longer than SWMI_AFF_MAX_READ); the short shape ignores them.  (band_adapt without a band: no kernel, aff_flags_ok.)
static inline uint32_t aff_run_flags(const AffRun &r, uint32_t long_reads) {
    return aff_flags(r.mat != nullptr, long_reads != 0u, long_reads && r.band, long_reads && r.xdrop, long_reads && r.adapt,
                     r.gap_open2 != 0, r.subopt != 0, r.end_bonus != 0u, r.hits != 0u);
}
// What the launchers refuse (hipErrorInvalidValue): values out of range and the combinations no kernel exists for.
// Every run check_run_params (swmi_run.cpp) admits passes.
static inline bool aff_run_ok(const AffRun &r, uint32_t long_reads) {
    if (r.band > SWMI_AFF_BAND_MAX || r.xdrop > 0x7FFFFFFFu || r.adapt > 1u || r.cigar > 2u) return false;
    if (r.mat && (r.nn < 2u || r.nn > SWMI_MAT_NN_MAX)) return false;
    if (r.subopt < -1 || r.subopt > (1 << 30) || r.hits > SWMI_HITS_MAX || r.end_bonus > (1u << 30)) return false;
    // two-piece and end_bonus runs take neither xdrop nor band_adapt, whatever the shape
    if ((r.gap_open2 || r.end_bonus) && (r.xdrop || r.adapt)) return false;
    // an overlap run takes none of the options of the long shape either, whatever the shape
    if (r.mode == 4u && (r.band || r.xdrop || r.adapt || r.gap_open2 || r.subopt || r.hits || r.end_bonus)) return false;
    return aff_flags_ok(r.mode, aff_run_flags(r, long_reads));
}
// The kernel the launchers below pick for a run, by name -- null where they refuse the run; shape: 0 narrow, 1 wide, 2 long (what
// a launch with long_reads set asks for).  They call no HIP function.  For the tests: not part of include/swmi.h.
extern "C" int swmi_affine_run_ok(const AffRun *r, uint32_t long_reads);
extern "C" const char *swmi_affine_sweep_name(const AffRun *r, uint32_t long_reads, uint32_t shape);
extern "C" const char *swmi_affine_traceback_name(const AffRun *r, uint32_t long_reads);
// Per-read score profiles (swmi_batch_set_read_profiles): the device image of a batch's profiles.
//   dwords 0 .. 255     key[code] = class(code) * 4, class n for a code outside the alphabet
//   dwords 256, 257     where the scores start, in dwords from the image's start (64 bits)
//   from dword 258      row_off[read], 64 bits each: the read's first row = its first byte in upload order
//   then                the scores as the caller gave them, n int32 per row
struct AffProfile {
    const uint32_t *image;
    uint32_t n;                  // symbols, 1 .. SWMI_MAT_MAX_SYMBOLS
};
#define SWMI_PROF_KEY_WORDS 256u
#define SWMI_PROF_HDR_WORDS 258u
// The LDS bound of a profile run (swmi.h): with m the longest read and M = 64 * ceil(m / 64), M * (n + 1) <= 32768 dwords -- one
// wavefront's table, 128 KiB, beside the 1 KiB of keys.
#define SWMI_PROF_LDS_WORDS 32768u
// The profile sweep a run takes, by name -- null where the launcher below refuses: a run with gap_open2, subopt, hits, end_bonus or
// a score matrix, and the long shape (shape: 0 narrow, 1 wide).  It calls no HIP function.  For the tests: not part of include/swmi.h.
extern "C" const char *swmi_affine_profile_sweep_name(const AffRun *r, uint32_t shape);
// The wavefronts of a workgroup (1 .. 4) the launcher below gives the sweep of that shape in a launch over n symbols whose longest
// read has r_max rows per lane: min(4, 159 KiB / table), table = 64 * r * (n + 1) int32 with r = r_max, for the narrow sweep
// min(r_max, 4).  0 where one table exceeds SWMI_PROF_LDS_WORDS or an argument is out of range: no launch.  The launcher calls it, so
// what a test reads is what a launch uses.  It calls no HIP function.  For the tests: not part of include/swmi.h.
extern "C" uint32_t swmi_affine_profile_waves(uint32_t n, uint32_t r_max, uint32_t shape);
// The short shape of a run whose batch has profiles, in place of swmi_launch_affine_sweep (.., 0, ..); r->mat is null.  Every
// wavefront stages its own read's table, so a workgroup has as many wavefronts (1 .. 4) as tables of the launch's longest read fit
// the LDS.  The walks are the run's ordinary ones.
extern "C" hipError_t swmi_launch_affine_profile_sweep(const FillArgs *a, const AffRun *r, const AffProfile *p, uint32_t r_min, uint32_t r_max,
                                                       hipStream_t st);
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
// pair lists: the segments' images (and the raw bytes of reversed or complemented segments) from the resident sources
// (sw_gather_kernel); `comp`: the 256-byte complement table (swmi_host.h: complement_table)
extern "C" hipError_t swmi_launch_gather(uint8_t *raw, const uint64_t *src_off, const uint64_t *raw_off, SeqDesc *desc, uint32_t *seqw,
                                         const uint8_t *lut, const uint8_t *comp, uint32_t n_seg, hipStream_t st);
