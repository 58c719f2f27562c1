// swmi_host.h -- what the units of the host runtime share (internal; the C ABI is include/swmi.h).
//
//   swmi_ctx.cpp      library / context / options / score matrix / upload; owns the thread's last error
//   swmi_run.cpp      run_chunk, batch_run, the async worker, and (swmi_plan.h) the chunk plan -- the whole per-step path, in ONE unit
//   swmi_results.cpp  the record stream and its lazy index, pair accessors, MapRef views
//   swmi_stream.cpp   swmi_stream_*
//   swmi_diag.cpp     SWMI_DEBUG_FILL / SWMI_DEBUG_WATCHDOG printers
//
// Owns device memory, the HIP stream, batching/chunking, the overflow re-runs and the host-side assembly of results (the
// part of the reference that builds Java Strings from the traceback stack, src/sw/SmithWaterman.java:418-431, and MapRef's
// aggregation, src/sw/Distribution.java:403-436).  All DP arithmetic and every traceback step run in the gfx950 kernels:
// there is no CPU implementation of the algorithm in this library, and every entry point fails if no GPU is usable.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/swmi.h"
#include "swmi_device.h"
#include "swmi_io_internal.h"

// Functions shared between the units: hidden, so that the library exports what include/swmi.h declares and nothing more.
// None of them is called on the per-step path of a repeated run (fail: errors; settle_raw: the exact-size re-run and
// streams; the diagnostics: behind their environment switches).
namespace swmi_host __attribute__((visibility("hidden"))) {
int fail(int code, const char *fmt, ...);      // sets swmi_last_error(); returns code
int check_offsets(const uint64_t *off, uint32_t n, const char *what);
int upload_device(swmi_ctx *ctx, swmi_batch *b, hipStream_t st, const uint8_t *ref_src, const uint8_t *read_src);
int settle_raw(swmi_batch *b);
int dump_traceback_diagnostics(swmi_batch *b, const TraceArgs &ta, size_t np, size_t n_tf);
int dump_fill_diagnostics(swmi_batch *b, const FillArgs &fa, size_t np);
void watchdog_wait(hipStream_t st, const swmi_batch *b, const char *limit_s);
const uint8_t *code_table();                   // byte -> canonical code (swmi_ctx.cpp); applied AFTER the complement

// The complement of a base, as a 256-entry byte table (SWMI_SPEC_READ_REVCOMP): the IUPAC pairs A<->T, C<->G,
// R<->Y, K<->M, B<->V, D<->H; S, W and N are their own complements; U -> A (and so not an involution on U); lower case likewise
// and stays lower case; every other byte maps to itself.  Stated here once: sw_gather_kernel reads a device copy of it
// (swmi_ctx.d_comp), materialise reads it for host-built strings.
inline const uint8_t *complement_table() {
    static const struct Table {
        uint8_t t[256];
        Table() {
            for (int i = 0; i < 256; i++) t[i] = (uint8_t)i;
            const char *from = "ATCGRYKMBVDHU", *to = "TAGCYRMKVBHDA";
            for (int k = 0; from[k]; k++) {
                t[(uint8_t)from[k]] = (uint8_t)to[k];
                t[(uint8_t)(from[k] | 0x20)] = (uint8_t)(to[k] | 0x20);
            }
        }
    } T;
    return T.t;
}
}  // namespace swmi_host
using namespace swmi_host;

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? SWMI_ERR_NOMEM : SWMI_ERR_HIP,            \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                       \
    } while (0)

// ------------------------------------------------------------------------------------------
// device buffer with capacity (grow-only)
// ------------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // Allocations leave headroom (x 1.5 for workspaces of 256 MiB and more, x 1.25 when growing): a stream's chunks differ by a
    // few per cent, and freeing and re-allocating a 20 GB workspace for every new largest chunk stalled every slot of a stream
    // for 1.5-3 s each time (hipFree / hipMalloc hold a device-wide lock; profiles/r03/config3_host_breakdown.txt).
    int reserve(size_t bytes) {
        if (bytes <= cap) return SWMI_OK;
        size_t want = bytes >= (256u << 20) ? bytes + bytes / 2 : bytes;      // (big workspaces: the first allocation already leaves room)
        if (p) { want = std::max(want, cap + cap / 4); (void)hipFree(p); p = nullptr; cap = 0; }
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess && want > bytes) { want = bytes; e = hipMalloc(&p, want); }
        if (e != hipSuccess) { p = nullptr; return fail(SWMI_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
        cap = want;
        return SWMI_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }                 // (a buffer added to a struct later cannot be forgotten by its free function)
};

struct PinnedBuf {
    void *p = nullptr;      // host address
    void *dp = nullptr;     // the same memory as the GPU addresses it (zero-copy results)
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return SWMI_OK;
        if (p) { bytes = std::max(bytes, cap + cap / 4); (void)hipHostFree(p); p = nullptr; dp = nullptr; cap = 0; }      // (headroom: see DevBuf)
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped);
        if (e != hipSuccess) { p = nullptr; return fail(SWMI_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
        e = hipHostGetDevicePointer(&dp, p, 0);
        if (e != hipSuccess) { (void)hipHostFree(p); p = nullptr; return fail(SWMI_ERR_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e)); }
        cap = bytes;
        return SWMI_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; dp = nullptr; cap = 0; }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
};

// A substitution score matrix (swmi_set_score_matrix), immutable once built: contexts, stream slots and the batches of the
// runs that use it share it, so a new matrix set while a run is in flight never touches that run's copy.
struct ScoreMatrix {
    uint64_t gen = 0;                       // unique per matrix set (the plan cache and the batch's device copy key on it)
    uint32_t n = 0;                         // symbols
    int32_t max_entry = 0;                  // the largest score (path_bound)
    std::vector<uint32_t> image;            // the device image: swmi_aff_mat_words(n + 1) dwords (swmi_device.h)
};

// The per-read score profiles of a batch (swmi_batch_set_read_profiles), immutable once built and held by shared_ptr
// as a ScoreMatrix is: the batch keeps the current ones, a run takes those set when it was asked for.
struct ReadProfiles {
    uint64_t gen = 0;                       // unique per set (the plan cache and the batch's device copy key on it)
    uint32_t n = 0;                         // symbols
    int32_t max_entry = 0;                  // the largest entry (path_bound)
    int32_t max_abs = 0;                    // the largest |entry| (S of the affine bounds)
    std::vector<uint32_t> image;            // the device image (AffProfile, swmi_launch.h): keys, the reads' first rows, the scores
};

// What a run takes as the context has it WHEN THE RUN IS ASKED FOR: swmi_batch_run_async records it at the call, a stream's
// slots copy it at swmi_stream_open.  The context holds the plain part, RunModes, the plan key embeds it and every hand-over
// copies it whole: a new option of this kind is a new member, its setter, its checks and its consumer.  (gap_open and affine
// are not of this kind: a run reads them from the context when it STARTS, under ctx->mu -- an asynchronous run too.)
struct __attribute__((visibility("hidden"))) RunModes {
    int align_mode = SWMI_ALIGN_LOCAL;      // SWMI_ALIGN_FIT / _GLOBAL: end-to-end alignment, on the affine kernels
    int long_reads = 0;                     // 1: the affine kernels take reads longer than 1024 bases, swept in strips (swmi.h)
    int band = 0;                           // > 0: the half-width of the band the strip sweeps of such reads keep to (swmi.h); the affine kernels
    int extend = 0;                         // 1: seed extension -- a global run whose maximum is taken over every cell (swmi.h); refused in the other modes
    int xdrop = 0;                          // > 0: the drop-off threshold X of an extend run -- the strip sweep of a long read ends at a seam (swmi.h); refused in other runs
    int band_adapt = 0;                     // 1: the band of an extend run follows the alignment, strip by strip (swmi.h); refused in other runs
    int gap_open2 = 0;                      // != 0: two-piece gaps on a global or extend run -- the second piece's open (swmi.h); refused in other runs
    int gap2 = 0;                           // ... and its per-base extension (not read while gap_open2 == 0)
    int cigar = 0;                          // 1 / 2: the records' payload is a CIGAR, M/I/D or =/X/I/D (swmi.h); the affine kernels
    int subopt = 0;                         // != 0: a local run also returns every pair's second-best score -- the mask half-width, -1 automatic (swmi.h); refused in the other modes
    int hits = 0;                           // 1 .. 16 = K: a run under subopt also returns every pair's K best separated end cells (swmi.h); refused without subopt
    int end_bonus = 0;                      // > 0: an extend run also returns every pair's best score in read row m and takes the pair to the read's end when that is less than this bonus below the best score (swmi.h); refused in other runs
    int overlap = 0;                        // 1: overlap (ends-free) alignment -- a fit run whose read ends are free as well (swmi.h); refused in other runs
    bool two_piece() const { return gap_open2 != 0; }
    // the MODE of the affine kernels and their launchers: the align_mode, 3 (extend) for a global run with option "extend" or
    // 4 (overlap) for a fit run with option "overlap"
    uint32_t kernel_mode() const {
        return extend && align_mode == SWMI_ALIGN_GLOBAL ? 3u : overlap && align_mode == SWMI_ALIGN_FIT ? 4u : (uint32_t)align_mode;
    }
    bool operator==(const RunModes &o) const { return memcmp(this, &o, sizeof(RunModes)) == 0; }
};
static_assert(std::has_unique_object_representations_v<RunModes>, "RunModes is compared bytewise: no padding, no floating point");
// Option "band_adapt": the lower bound of every real H of a pair (m > 1024, NS = ceil(m / 1024) strips; gap_open, gap <= 0),
// (2 NS + 1) gap_open + (1024 NS + n) gap, and the run's condition on it, >= -2^30 (swmi.h).  In the header, and
// of plain integers: tests/test_adapt_cpu.py compiles it into a program of its own.
static inline int64_t swmi_adapt_low(uint64_t m, uint64_t n, int64_t gap_open, int64_t gap) {
    const int64_t ns = (int64_t)((m + SWMI_AFF_MAX_READ - 1) / SWMI_AFF_MAX_READ);
    return (2 * ns + 1) * gap_open + (ns * (int64_t)SWMI_AFF_MAX_READ + (int64_t)n) * gap;
}
static inline bool swmi_adapt_bound_ok(uint64_t m, uint64_t n, int64_t gap_open, int64_t gap) {
    return swmi_adapt_low(m, n, gap_open, gap) >= -((int64_t)1 << 30);
}
// the options that decide the size of a mode-3 pair's workspace (swmi_device.h), as a run has them
static inline AffGeom aff_geom(const RunModes &md) {
    return AffGeom{md.band > 0 ? (uint32_t)md.band : 0u, md.band > 0 && md.band_adapt != 0, md.two_piece(), md.subopt != 0, md.subopt != 0 && md.hits != 0};
}
// Everything a batch's schedule (swmi_batch::work: the pairs in launch order with their workspace sizes) depends on besides the
// sequences.  A run whose key equals the key of the schedule the batch holds keeps it.  An input of the sizes that is missing
// here hands a re-run under other options a schedule with the old sizes -- but an option that changes a mode-3 pair's workspace
// is a member of AffGeom, which is part of the key as it is: add it there (and to aff_geom), not here.
struct __attribute__((visibility("hidden"))) SchedKey {
    int eff_mode = -1;                      // the pipeline the sizes were made for; -1: no schedule (a new upload, a schedule handed on)
    bool tfused = false;                    // the sizes leave room for sw_tfused_kernel's column checkpoints
    AffGeom geom{};                         // mode 3: the run's; all-zero under the other modes
    SchedKey() = default;
    SchedKey(uint32_t mode, bool tf, const RunModes &md) : eff_mode((int)mode), tfused(tf), geom(mode == 3 ? aff_geom(md) : AffGeom{}) {}
    bool operator==(const SchedKey &o) const { return eff_mode == o.eff_mode && tfused == o.tfused && geom == o.geom; }
};
struct __attribute__((visibility("hidden"))) RunOptions {
    RunModes modes;
    std::shared_ptr<const ScoreMatrix> mat; // swmi_set_score_matrix (null: none); keeps the matrix's host image alive
    std::shared_ptr<const ReadProfiles> prof;   // the BATCH's profiles (null: none), taken with the context's options (run_options)
};

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
struct swmi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // options
    uint32_t cell_cap = 64;
    uint64_t max_workspace_bytes = 32ull << 30;
    int profiling = 0;
    uint32_t mode = 1;                      // requested pipeline (see swmi.h); mode 1 falls back to 2 for scores it cannot handle
    int zero_copy = 1;                      // kernels write results straight into pinned host memory (no D2H copy)
    uint64_t arena_words_per_pair = 160;    // first guess of the record arena (header + ops + two strings of a ~180-step alignment), grows on demand
    uint64_t arena_copy_wpp = 160;          // arena words per pair fetched with the first D2H (tracks the last run)
    uint64_t recs_per_pair_x16 = 32;        // first guess of the record table: entries per pair x 16, grows on demand
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    PinnedBuf h_err;                        // one host-mapped word the kernels raise on an internal failure (strip pipeline timeout)
    DevBuf d_hdr_ring;                      // arena headers of launches that run sw_tfused_kernel / sw_resident_pairs_kernel ONLY: a fresh zeroed
    uint32_t hdr_next = 0;                  // slot per launch, so that no kernel has to run first just to reset the bump pointer
    DevBuf d_lut;                           // 256-byte canonical-code table of the encode kernel
    DevBuf d_comp;                          // 256-byte complement table of sw_gather_kernel (complement_table)
    int64_t spin_us = 2000;                 // how long a run polls its stream for completion before it blocks (a batch is sub-millisecond)
    uint32_t dbg_strip_spins = 0;           // test knob: spin budget of the strip pipeline (0 = default)
    uint32_t dbg_reverse_strips = 0;        // test knob: strip items dispatched consumer-first
    uint32_t dbg_async_delay_us = 0;        // test knob: the async worker waits this long before it starts a job
    uint32_t auto_ties_x100 = 300;          // automatic traceback grain: split when a sampled pair has this many tied maxima (x 1/100) on average
    uint32_t col_chunks = 0;                // test knob: force this many column chunks per pair (0 = automatic)
    int tb_split = -1;                      // mode-1 traceback grain: -1 automatic, 0 one workgroup per pair, 1 one wavefront per window / alignment
    bool ext_events = false;                // SWMI_EXT_EVENTS=1: the plain two-kernel run is timed by the dispatches' own start/stop times (pure kernel
                                            // durations, as rocprofv3 shows them) -- measured 8-12 us per run DEARER than three hipEventRecord, so off
    int tfused = -1;                        // transposed sweep + traceback by one wavefront per pair (swmi_tfused.hip): -1 automatic, 0 never, 1 whenever a pair qualifies
    int resident = -1;                      // small pairs handled by one wavefront with the direction field in LDS: -1 automatic, 0 never, 1 whenever it fits
    int scores_only = 0;                    // 1: the sweep only -- every pair's score (and MapRef's totals), no tied-maximum lists, no alignments
    int stream_keep_records = 1;            // streams: 0 = a chunk's alignment records are dropped once its scores and counts are taken (a driver
                                            // that only needs totals and re-aligns its few winners, Distribution.java:341-353)
    int device_strings = 1;                 // the traceback kernels write both aligned strings behind every record (swmi_emit.h); 0: 2-bit ops only, strings built by the host
    bool cell_cap_set = false;              // cell_cap given by the caller (otherwise small launches get longer lists)
    int32_t gap_open = 0;                   // affine gaps: a gap of length k costs gap_open + k * gap (0: linear)
    int affine = -1;                        // -1: the affine kernels (mode 3) when gap_open != 0; 1: always
    RunModes modes;                         // options "align_mode", "long_reads", "band", "extend", "xdrop", "band_adapt", "gap_open2", "gap2", "cigar", "subopt", "hits", "end_bonus" and "overlap"
    std::mutex mat_mu;                      // guards `matrix` (not ctx->mu: setting a matrix does not wait for a run)
    std::shared_ptr<const ScoreMatrix> matrix;   // swmi_set_score_matrix; a run with one takes the affine kernels
    // swmi_batch_run_async: one run in flight on the context's own host thread
    std::thread worker;
    std::mutex job_mu;
    std::condition_variable job_cv;
    std::atomic<int> job_state{0};          // 0 idle, 1 submitted, 2 finished, 3 quit
    swmi_batch *job_batch = nullptr;
    swmi_params job_params{};
    RunOptions job_opt;                              // run_options(ctx) when swmi_batch_run_async was called
    uint32_t job_delay_us = 0;                       // debug_async_delay_us when swmi_batch_run_async was called
    int job_rc = 0;
    std::string job_err;
};

// one alignment as parsed from the arena
struct HostAln {
    uint32_t rank;
    int32_t begin, end_i, end_j;
    uint32_t n_ops;
    const uint32_t *rec = nullptr;   // the alignment's payload in the arena: the two strings written by the kernels, the packed ops, or the CIGAR
    int64_t str_id = -1;    // records without strings: >= 0 once the strings are built, offset of the reference-side string in swmi_batch::str_buf
};

struct PairRes {
    int32_t score = 0;
    uint32_t flags = 0;
    uint64_t n_cells = 0;
    uint32_t strips = 0;    // option "xdrop": the strips swept of a pair that was stopped, else 0 (swmi_pair_rows_swept)
    uint64_t first = 0;     // index of the pair's first HostAln (ordered)
    uint64_t count = 0;     // alignment records present (0 when degenerate)
};

struct SiteRef { uint64_t pair; uint64_t k; int32_t begin; };

struct Work {            // one pair scheduled for a launch
    uint32_t pair;       // ref * n_reads + read (a pair list: the position in the list)
    uint64_t cells;      // m * n
    uint64_t dir_words;  // workspace dwords (direction field or checkpoints)
    uint64_t seam_words;
};

// Everything the plan of a chunk (swmi_plan.h: plan_chunk) depends on.  A run whose key equals the key of the plan the
// batch holds -- a repeated run of the same chunk with the same parameters: bench.py's steps, a Spark job re-running a
// partition -- skips the per-pair preparation and its uploads.  An input of the planner that is missing here gives a stale
// plan on such a re-run: add it to BOTH the struct and operator== -- unless it is one of the run's modes: a member added to
// RunModes is part of the key as it is.
struct __attribute__((visibility("hidden"))) PlanKey {
    bool valid = false;                     // false: no plan (a new upload, the sampled pre-pass: they reset the key)
    size_t lo = 0, hi = 0;                  // the chunk: work[lo, hi) ...
    const void *work = nullptr;             // ... of this schedule
    swmi_params params{};
    uint32_t eff_mode = 0;
    uint32_t col_chunks = 0;                // the context's options the planner reads
    bool reverse_strips = false;
    int resident = -1, tfused = -1;
    bool exact = false;                     // the exact-size re-run: no resident, no tfused pairs
    bool scores_only = false;
    uint64_t mat_gen = 0;                   // the score matrix's generation (0: none): it bounds the paths (not the matrix: a key keeps none alive)
    uint64_t prof_gen = 0;                  // the batch's profiles' generation (0: none), for the same reason
    RunModes modes;                         // the run's modes: the alignment mode bounds the paths too
    const void *d_pairs = nullptr;          // where the chunk's PairDesc image sits on the device, and its size
    size_t pairs_bytes = 0;
    bool operator==(const PlanKey &o) const {
        return valid == o.valid && lo == o.lo && hi == o.hi && work == o.work && memcmp(&params, &o.params, sizeof(swmi_params)) == 0 &&
               eff_mode == o.eff_mode && col_chunks == o.col_chunks && reverse_strips == o.reverse_strips && resident == o.resident &&
               tfused == o.tfused && exact == o.exact && scores_only == o.scores_only && mat_gen == o.mat_gen && prof_gen == o.prof_gen &&
               modes == o.modes && d_pairs == o.d_pairs && pairs_bytes == o.pairs_bytes;
    }
};

// What the planner derives for a chunk besides the arrays it uploads: the sizes everything downstream is dimensioned by.
struct __attribute__((visibility("hidden"))) ChunkPlan {
    uint64_t dir_words = 0, seam_words = 0; // workspace of the launch
    uint64_t seam_priv_words = 0;           // private seam rows of the strip pipeline's column chunks (behind the shared rows in d_seam)
    uint32_t max_path = 0, max_read = 0;    // longest possible traceback / longest read
    size_t n_strip_items = 0;               // mode 1: (pair, column chunk, strip) of every read longer than one strip, one wavefront each
    size_t n_strip_chunks = 0;              // ... and how many chunk sweeps (0: every multi-strip pair in one)
    size_t n_col_items = 0;                 // mode 1: column chunks of single-strip pairs when the launch has few pairs
    uint64_t n_windows = 0;                 // split traceback: checkpoint windows of all pairs
    size_t n_res = 0;                       // pairs handled whole by sw_resident_pairs_kernel
    uint32_t res_lds_words = 0, res_ops_words = 0;
    size_t n_tf = 0;                        // pairs handled whole by sw_tfused_kernel (transposed sweep + traceback)
    uint32_t tf_max_m = 0, tf_max_n = 0, tf_max_path = 0;
    uint32_t aff_r_min = 0xFFFFFFFFu, aff_r_max = 0;   // mode 3: rows per lane of the chunk's shortest and longest read of at most 1024 bases
    size_t aff_n_long = 0;                  // mode 3: pairs whose read is longer (the strip kernels); they are the LAST of the PairDesc array
};

struct swmi_batch {
    uint32_t n_refs = 0, n_reads = 0;
    // A PAIR LIST (swmi_batch_upload_pairs): the sequences of the batch -- n_refs, n_reads, ref_desc, read_desc, d_refs, d_reads,
    // the images in d_seqw -- are the SEGMENTS, n_pairs on either side, pair k = (reference segment k, read segment k); everything
    // from the schedule down sees Work, PairDesc and SeqDesc as for a cross product.  ref_bytes / read_bytes / ref_off / read_off
    // are the SOURCES (n_src_refs, n_src_reads of them), resident in d_raw; specs[k] is pair k with SWMI_SPEC_WHOLE resolved.
    bool paired = false;
    uint32_t n_src_refs = 0, n_src_reads = 0;
    std::vector<swmi_pair_spec> specs;
    bool sources_on_device = false;         // d_raw holds the sources (it is grown, and filled again, when a list needs a larger transformed area)
    DevBuf d_src_off;                       // per segment: where sw_gather_kernel reads it (bit 63: reversed, bit 62: complemented), indexed as d_raw_off
    // original bytes (for string building: characters keep their case) and offsets
    std::vector<uint8_t> ref_bytes, read_bytes;
    // a streamed chunk keeps no copy of its references: their bytes are read again from the mapped file when an
    // alignment string is asked for (swmi_stream_push_file)
    const uint8_t *src_map = nullptr;
    std::vector<swmi_io_recpos> src_recs;
    std::unordered_map<uint32_t, std::vector<uint8_t>> src_cache;
    std::vector<uint64_t> ref_off, read_off;
    std::vector<SeqDesc> ref_desc, read_desc;
    // device
    DevBuf d_raw, d_raw_off;                // the caller's bytes as uploaded (input of the encode kernel) and their offsets
    DevBuf d_seqw, d_refs, d_reads, d_pairs, d_dir, d_seam, d_result, d_cells, d_cells_off, d_cells_cap, d_dbg, d_dbg2;
    DevBuf d_strip_items, d_progress;       // mode 1: strip-per-wavefront sweep of long reads
    DevBuf d_col_items;                     // mode 1: column chunks of single-strip pairs
    DevBuf d_win_off, d_queue;              // split traceback: per-pair window offsets, walk-item queue
    DevBuf d_tf_items;                      // pairs of the launch taken by sw_tfused_kernel
    DevBuf d_res_items;                     // resident pairs of the launch
    bool views_built = false;               // some MapRef view of the last run was built (they are reset by the next run)
    bool tb_split_used = false;             // the last run used the split traceback
    bool acgt_known = false;                // ref_desc/read_desc[].acgt fetched back from the device (set there by the encode kernel)
    PinnedBuf h_result;
    // per run
    swmi_params params{};
    bool has_run = false;
    int auto_choice = -1;                   // sampled pre-pass of the automatic traceback grain: 0 tie-heavy, 1 not, -1 not decided yet
    swmi_params auto_params{};
    std::vector<Work> work;                 // schedule (pairs sorted by work), valid for work_key
    SchedKey work_key;                      // reset or moved together with `work`
    uint32_t eff_mode = 1;                  // pipeline of the current run (3: the affine kernels, swmi_affine.hip)
    int32_t gap_open = 0;                   // the context's gap_open when the run started (mode 3)
    RunOptions opt;                         // the context's run options when the run was asked for (mode 3)
    DevBuf d_mat;                           // the device image of opt.mat, copied on the run's stream
    uint64_t d_mat_gen = 0;                 // generation of the matrix in d_mat (0: none)
    std::shared_ptr<const ReadProfiles> profiles;   // swmi_batch_set_read_profiles (null: none); guarded by the context's mat_mu
    DevBuf d_prof;                          // the device image of opt.prof, copied on the run's stream
    uint64_t d_prof_gen = 0;                // generation of the profiles in d_prof (0: none)
    uint64_t work_cells = 0;
    std::vector<uint8_t> pairs_on_device;   // image of the PairDesc array currently in d_pairs
    const void *pairs_dev_ptr = nullptr;
    PlanKey plan_key;                       // the chunk the device-side item lists and `plan` were prepared for last
    ChunkPlan plan;
    std::vector<PairRes> pairs;             // by pair index
    bool has_sub = false;                   // the last run had option "subopt": `sub` holds every pair's (score2, end2), (0, 0) for a pair that was not swept
    std::vector<SuboptOut> sub;                // by pair index
    int hits_k = 0;                         // the last run had option "hits" = hits_k (0: none): `hitv` holds 1 + hits_k entries per pair (swmi_device.h: HitEnt), zeros for a pair that was not swept
    std::vector<HitEnt> hitv;               // by pair index
    bool has_endb = false;                  // the last run had option "end_bonus": `endv` holds every pair's (max_score, end_score, end_col), (0, 0, 0) for a pair that was not swept
    std::vector<EndOut> endv;               // by pair index
    // option "band_adapt": the window tables the sweeps of the last run left (the centre of every strip, swmi_device.h), fetched
    // after every launch; win_at[pair] = 1 + the index of the pair's first entry in win_tab, 0 for a pair without a table
    std::vector<uint32_t> win_tab;
    std::vector<uint64_t> win_at;
    // raw record streams of the last run (one per launch chunk), indexed lazily on the first alignment access
    // the record table entries (AlnRec, swmi_device.h) and the payload arenas of the launches, one RawChunk per launch
    struct RawChunk { size_t at, words; size_t tab_at, n_rec; size_t lo; std::vector<uint32_t> wpos; };   // wpos: re-run chunks only
    std::vector<uint32_t> raw;
    std::vector<AlnRec> rtab;
    // a run of ONE launch with results in pinned memory leaves its record stream where the kernels wrote it (the pinned block
    // is the batch's own and lives until the next run): copied into `raw` only when something needs it there
    const uint32_t *raw_ext = nullptr;
    const AlnRec *rtab_ext = nullptr;
    uint64_t raw_ext_records = 0, raw_ext_cap = 0;
    std::vector<RawChunk> raw_chunks;
    bool indexed = false;
    bool rec_strings = false;               // the records of the last run carry both aligned strings (option device_strings)
    int rec_cigar = 0;                      // != 0: they carry a CIGAR instead (option cigar, its value): {n_cigar, nm, entries} (swmi_emit.h)
    bool scores_only = false;               // the last run computed scores only (option scores_only): no counts, no alignments
    bool records_dropped = false;           // a streamed chunk whose records were not kept (option stream_keep_records = 0)
    std::vector<HostAln> alns;              // grouped by pair, ordered as OptAlignments returns them
    std::vector<char> str_buf;              // every alignment's two NUL-terminated strings, at fixed offsets (str_at)
    std::vector<uint64_t> str_at;           // per alignment: offset of its reference-side string; the read side follows it
    // MapRef view cache
    std::vector<int8_t> ref_view_ready;
    std::vector<std::vector<SiteRef>> ref_sites;
    std::vector<uint64_t> ref_degenerate;   // leading (0,"","") sites per ref
    swmi_timing timing{};
};

// the run options of a run of batch b: the context's as set now, and the batch's profiles as set now (b null: the context's alone)
// (in the header: every swmi_batch_run takes them, and no per-step call may cross a unit boundary)
static inline RunOptions run_options(swmi_ctx *ctx, const swmi_batch *b) {
    std::lock_guard<std::mutex> g(ctx->mat_mu);
    return RunOptions{ctx->modes, ctx->matrix, b ? b->profiles : nullptr};
}

// Which sequences a pair is made of: the cross product's division, or the identity of a pair list.  Every place that turns a
// pair index into its two sequences goes through these two.
static inline uint64_t batch_n_pairs(const swmi_batch *b) { return b->paired ? (uint64_t)b->n_refs : (uint64_t)b->n_refs * b->n_reads; }
static inline uint32_t pair_ref(const swmi_batch *b, uint64_t pair) { return b->paired ? (uint32_t)pair : (uint32_t)(pair / b->n_reads); }
static inline uint32_t pair_read(const swmi_batch *b, uint64_t pair) { return b->paired ? (uint32_t)pair : (uint32_t)(pair % b->n_reads); }

struct RunState {
    swmi_ctx *ctx;
    swmi_batch *b;
    FillArgs fa{};
    TraceArgs ta{};
    float fill_ms = 0, tb_ms = 0, d2h_ms = 0;
    uint32_t launches = 0;
    double enqueue_us = 0, wait_us = 0, copyout_us = 0, prep_us = 0, prep_upload_us = 0;
    bool one_wave_sweep = false;            // the strip pipeline gave up once in this run: long reads are swept by one wavefront
    bool tb_split = false;                  // mode 1: detect per window + walk per alignment instead of one workgroup per pair
    bool defer_copy = false;                // this launch is the whole run: its records may stay in the pinned block
    bool keep = true;                       // the launch's records belong to the batch's results (false: the sampled pre-pass)
};

// layout of the result block: [ArenaHdr | PairOut x np | sub: SuboptOut x np (option "subopt") or EndOut x np (option "end_bonus"), else nothing |
//                              record table, tab_cap entries | arena words ...]
// sub: the bytes per pair of that array -- the two options exclude each other, so they share the place.  Option "hits" (with "subopt"):
// a second array, (1 + K) HitEnt per pair, follows the SuboptOut array at result_hits_off and counts in `sub`
static inline size_t result_out_off() { return 64; }
static inline size_t result_sub_off(size_t np) { return 64 + np * sizeof(PairOut); }
static inline size_t result_hits_off(size_t np) { return result_sub_off(np) + np * sizeof(SuboptOut); }
static inline size_t result_tab_off(size_t np, size_t sub) { return (64 + np * (sizeof(PairOut) + sub) + 255) & ~(size_t)255; }
static inline size_t result_arena_off(size_t np, uint64_t tab_cap, size_t sub) { return (result_tab_off(np, sub) + tab_cap * sizeof(AlnRec) + 255) & ~(size_t)255; }
// dwords of one alignment's payload: the two strings, n_ops / 4 + 1 dwords each, or the ops packed 16 per dword (swmi_emit.h)
static inline uint64_t rec_words(uint32_t n_ops, bool strings) {
    return strings ? 2 * ((uint64_t)n_ops / 4 + 1) : ((uint64_t)n_ops + 15) / 16;
}
// ... of a record of the batch's last run, at dword `off` of an arena of `words` dwords.  A CIGAR record is sized from its own first
// dword, read only when it lies inside the arena; false: the payload does not fit the arena
static inline bool payload_end(const swmi_batch *b, const AlnRec &e, const uint32_t *arena, uint64_t words, uint64_t &end) {
    const uint64_t off = ((uint64_t)e.off_hi << 32) | e.off_lo;
    if (!b->rec_cigar) { end = off + rec_words(e.n_ops, b->rec_strings); return end <= words; }
    if (off + 2 > words || off + 2 < off) return false;
    end = off + 2 + arena[off];
    return end <= words;
}
