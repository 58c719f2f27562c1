// swmi_run.cpp -- a run of a batch: the schedule, the plan of each chunk, the launches, their wait and retries.
//
// Everything a repeated run executes once per step lives in this unit (batch_run -> run_chunk -> prepare_chunk of swmi_plan.h
// and their helpers, all static): a step of the headline is 0.12 ms and the host's share of it is measurable, so none of it calls
// across a unit boundary.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <numeric>

#include "swmi_host.h"
#include "swmi_launch.h"
#include "swmi_plan.h"

// ------------------------------------------------------------------------------------------
// one chunk: launch, wait, retry
// ------------------------------------------------------------------------------------------
// The records of a finished launch become part of the batch's results.  The only launch of a run leaves its table and
// payloads in the pinned block (the batch's own until the next run): indexed there when something asks for an alignment.
// With several launches in one run each one's records are copied out of the block, which the next launch writes again; the
// table is dense, so its sequential read also tells how much of the arena is in use.
static int keep_chunk_records(RunState &rs, const AlnRec *tab, uint64_t n_rec, const uint32_t *arena, uint64_t arena_cap, size_t lo) {
    swmi_batch *b = rs.b;
    if (rs.defer_copy && b->raw_chunks.empty()) {
        b->raw_ext = arena; b->rtab_ext = tab; b->raw_ext_records = n_rec; b->raw_ext_cap = arena_cap;
        b->raw_chunks.push_back(swmi_batch::RawChunk{0, 0, 0, (size_t)n_rec, lo, {}});
        return SWMI_OK;
    }
    uint64_t used = 0;
    for (uint64_t k = 0; k < n_rec; k++) {
        uint64_t end;
        if (!payload_end(b, tab[k], arena, arena_cap, end)) return fail(SWMI_ERR_HIP, "record payloads overrun the arena");
        used = std::max(used, end);
    }
    b->raw_chunks.push_back(swmi_batch::RawChunk{b->raw.size(), (size_t)used, b->rtab.size(), (size_t)n_rec, lo, {}});
    b->raw.insert(b->raw.end(), arena, arena + used);
    b->rtab.insert(b->rtab.end(), tab, tab + n_rec);
    return SWMI_OK;
}

namespace {
// A chunk's launch as its attempts see it: what is fixed before the first attempt, and what each attempt decides.
struct Launch {
    size_t np = 0, lo = 0;
    const std::vector<uint64_t> *cells_exact = nullptr;   // exact per-pair cell lists (the re-run of overflowed pairs), or null: cell_cap each
    std::vector<uint64_t> coff;             // ... their offsets and capacities, alive until the launch has read them
    std::vector<uint32_t> ccap;
    uint32_t cell_cap = 0;
    uint64_t cells_total = 0;
    bool split = false;                     // the split traceback takes the launch
    bool zc = false;                        // results land in pinned host memory while the kernels run
    bool sweep_only = false;                // option scores_only
    bool sub = false;                       // option "subopt": the result block holds a SuboptOut per pair behind the pair outputs
    bool endb = false;                      // option "end_bonus": ... an EndOut per pair, in the same place (the two options exclude each other)
    uint32_t hits = 0;                      // option "hits" (with sub): K -- behind the SuboptOut array, 1 + K HitEnt per pair
    size_t hit_bytes() const { return hits ? (1u + hits) * sizeof(HitEnt) : 0; }
    size_t sub_bytes() const { return sub ? sizeof(SuboptOut) + hit_bytes() : endb ? sizeof(EndOut) : 0; }      // per pair, behind the pair outputs
    bool time_all = false;                  // (profiling = 2: only the sweep is bracketed -- two marker packets per run instead of three; each costs ~3.5 us of the step)
    uint64_t arena_cap = 0, tab_cap = 0;    // grown by an attempt that overflowed
    // per attempt
    int attempt = 0;
    uint8_t *res = nullptr;                 // the device result block and the offsets of the record table and the arena in it
    size_t t_off = 0, a_off = 0;
    uint64_t q_cap = 0;
    bool whole_only = false;                // no sweep kernel: the arena header comes from the context's ring
    bool ext_timing = false;
    uint64_t copy_words = 0, copy_recs = 0; // without zero-copy: arena words and table entries fetched with the first D2H
};
}  // namespace

static inline bool dbg_fill_on() {
    static const bool on = getenv("SWMI_DEBUG_FILL") != nullptr;      // (getenv walks the whole environment: once per process, not per run)
    return on;
}

// cell-list geometry: uniform (cell_cap per pair), or exact per pair and uploaded
static int size_cell_lists(RunState &rs, Launch &L) {
    swmi_ctx *ctx = rs.ctx;
    swmi_batch *b = rs.b;
    const size_t np = L.np;
    int rc;
    L.cell_cap = ctx->cell_cap;
    if (L.cells_exact) {
        L.coff.resize(np); L.ccap.resize(np);
        for (size_t k = 0; k < np; k++) {
            L.coff[k] = L.cells_total;
            L.ccap[k] = (uint32_t)std::min<uint64_t>((*L.cells_exact)[L.lo + k], 0xFFFFFFFFu);
            L.cells_total += L.ccap[k];
        }
        if ((rc = b->d_cells_off.reserve(np * 8))) return rc;
        if ((rc = b->d_cells_cap.reserve(np * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(b->d_cells_off.p, L.coff.data(), np * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(b->d_cells_cap.p, L.ccap.data(), np * 4, hipMemcpyHostToDevice, ctx->stream));
    } else {
        // a launch of few pairs can afford long lists: a periodic reference against one read is ONE pair with a tied maximum
        // per period (EngineerData.java:118), and a list that overflows costs a second run of the pair
        if (!ctx->cell_cap_set) L.cell_cap = (uint32_t)std::min<uint64_t>(65536, std::max<uint64_t>(L.cell_cap, (4ull << 20) / np));
        L.cells_total = (uint64_t)np * L.cell_cap;
    }
    return b->d_cells.reserve(std::max<uint64_t>(L.cells_total, 1) * sizeof(uint2));
}

static int build_fill_args(RunState &rs, Launch &L) {
    swmi_ctx *ctx = rs.ctx;
    swmi_batch *b = rs.b;
    const ChunkPlan &plan = b->plan;
    int rc;
    FillArgs &fa = rs.fa;
    fa.seqw = b->d_seqw.as<uint32_t>();
    fa.refs = b->d_refs.as<SeqDesc>();
    fa.reads = b->d_reads.as<SeqDesc>();
    fa.pairs = b->d_pairs.as<PairDesc>();
    fa.dir = b->d_dir.as<uint32_t>();
    fa.seam = b->d_seam.as<int32_t>();
    fa.out = (PairOut *)(L.res + result_out_off());
    fa.cells = b->d_cells.as<uint2>();
    fa.cells_off = L.cells_exact ? b->d_cells_off.as<uint64_t>() : nullptr;
    fa.cells_cap = L.cells_exact ? b->d_cells_cap.as<uint32_t>() : nullptr;
    fa.hdr = (ArenaHdr *)L.res;
    fa.dbg = nullptr;
    fa.dbg_pad = 0;
    if (dbg_fill_on()) {                          // diagnostics: per-pair slow-path entries and wave cycles
        if ((rc = b->d_dbg.reserve(L.np * 16))) return rc;
        fa.dbg = b->d_dbg.as<unsigned long long>();
        fa.dbg_thr0 = getenv("SWMI_DEBUG_THR0") ? (uint32_t)atoi(getenv("SWMI_DEBUG_THR0")) : 1u;
        fa.dbg_pad = getenv("SWMI_DEBUG_SKIP") ? 1u : 0u;
    }
    fa.n_pairs = (uint32_t)L.np;
    fa.cell_cap = L.cell_cap;
    fa.match = b->params.match; fa.mismatch = b->params.mismatch; fa.gap = b->params.gap;
    fa.strict = b->params.tie_mode == SWMI_TIE_STRICT;
    fa.mode = b->eff_mode;
    const bool pipe = plan.n_strip_items && !rs.one_wave_sweep;
    fa.skip_multi = pipe ? 1u : 0u;
    fa.strip_items = pipe ? b->d_strip_items.as<StripItem>() : nullptr;
    fa.progress = pipe ? b->d_progress.as<uint32_t>() : nullptr;
    fa.n_strip_items = pipe ? (uint32_t)plan.n_strip_items : 0u;
    fa.err_host = (uint32_t *)ctx->h_err.dp;
    fa.n_out = (uint32_t)L.np;
    if (L.attempt == 0) b->timing.col_chunks += (uint32_t)plan.n_col_items + (pipe ? (uint32_t)plan.n_strip_chunks : 0u);
    fa.col_items = plan.n_col_items ? b->d_col_items.as<ColItem>() : nullptr;
    fa.n_col_items = (uint32_t)plan.n_col_items;
    fa.strip_spins = ctx->dbg_strip_spins;
    // split traceback: the walk-item queue; its counter is zeroed by the sweep kernel of the first attempt
    L.q_cap = std::min<uint64_t>(std::max<uint64_t>(L.cells_total, 1), 1ull << 24);
    if (L.split && (rc = b->d_queue.reserve(256 + L.q_cap * sizeof(uint4)))) return rc;
    fa.q_reset = L.split ? b->d_queue.as<uint32_t>() : nullptr;
    return SWMI_OK;
}

// (after build_fill_args: the two share the batch's buffers)
static int build_trace_args(RunState &rs, Launch &L) {
    swmi_ctx *ctx = rs.ctx;
    swmi_batch *b = rs.b;
    const ChunkPlan &plan = b->plan;
    const FillArgs &fa = rs.fa;
    int rc;
    TraceArgs &ta = rs.ta;
    ta.seqw = fa.seqw; ta.refs = fa.refs; ta.reads = fa.reads; ta.pairs = fa.pairs;
    ta.dir = fa.dir; ta.out = fa.out; ta.cells = fa.cells;
    ta.cells_off = fa.cells_off; ta.cells_cap = fa.cells_cap;
    ta.hdr = (ArenaHdr *)L.res;
    ta.arena = (uint32_t *)(L.res + L.a_off);
    ta.arena_cap_words = L.arena_cap;
    ta.rec_tab = (AlnRec *)(L.res + L.t_off);
    ta.rec_tab_cap = (uint32_t)std::min<uint64_t>(L.tab_cap, 0xFFFFFFFFu);
    ta.n_pairs = fa.n_pairs; ta.cell_cap = fa.cell_cap;
    ta.match = fa.match; ta.mismatch = fa.mismatch; ta.gap = fa.gap; ta.strict = fa.strict;
    ta.lds_words = (plan.max_path + 3) / 4 + 1;               // one staged op per byte
    ta.seam = fa.seam;
    ta.mode = b->eff_mode;
    ta.pad2 = 0;
    ta.lds_read_words = (plan.max_read + 3) / 4 + 1;
    ta.out_host = nullptr;
    // (without zero-copy results the kernels' give-up codes still need a host-visible word: the context's own)
    ta.ovf_host = (uint32_t *)ctx->h_err.dp + 4;
    ((volatile uint32_t *)ctx->h_err.p)[4] = 0u; ((volatile uint32_t *)ctx->h_err.p)[5] = 0u;
    ta.win_off = nullptr; ta.q_count = nullptr; ta.q_items = nullptr; ta.q_cap = 0; ta.pad4 = 0;
    // (option "cigar": the payload is the CIGAR -- device_strings is not read and the walks get no raw bytes)
    const int cigar = b->eff_mode == 3 ? b->opt.modes.cigar : 0;
    const bool strings = !cigar && ctx->device_strings != 0 && b->d_raw.p != nullptr;
    ta.raw = strings ? b->d_raw.as<uint8_t>() : nullptr;
    ta.raw_off = strings ? b->d_raw_off.as<uint64_t>() : nullptr;
    ta.raw_reads_at = b->n_refs + 1u;
    b->rec_strings = strings;
    b->rec_cigar = cigar;
    if (L.zc) {
        // results land in pinned host memory while the kernel runs: [overflow word .. | PairOut x np | arena]
        if ((rc = b->h_result.reserve(L.a_off + L.arena_cap * 4))) return rc;
        uint8_t *hd = (uint8_t *)b->h_result.dp;
        *(volatile uint32_t *)b->h_result.p = 0u;
        ((volatile uint32_t *)b->h_result.p)[1] = 0u;
        ta.ovf_host = (uint32_t *)hd;
        ta.out_host = (PairOut *)(hd + result_out_off());
        ta.arena = (uint32_t *)(hd + L.a_off);
        ta.rec_tab = (AlnRec *)(hd + L.t_off);
    }
    ta.dbg = nullptr;
    if (dbg_fill_on()) {
        if ((rc = b->d_dbg2.reserve(L.np * 32))) return rc;
        HIP_TRY(hipMemsetAsync(b->d_dbg2.p, 0, L.np * 32, ctx->stream));
        ta.dbg = b->d_dbg2.as<unsigned long long>();
    }
    // Every pair handled whole by sw_tfused_kernel / sw_resident_pairs_kernel: the sweep kernel would run only to zero the
    // arena header.  Such a launch takes its header from a ring of zeroed slots instead (results in pinned memory only: a
    // D2H copy fetches the header with the block it sits in).
    L.whole_only = L.zc && plan.n_tf + plan.n_res == L.np;
    if (L.whole_only) {
        const uint32_t slots = 1024;
        if (!ctx->d_hdr_ring.p || ctx->hdr_next >= slots) {
            if ((rc = ctx->d_hdr_ring.reserve((size_t)slots * 64))) return rc;
            HIP_TRY(hipMemsetAsync(ctx->d_hdr_ring.p, 0, (size_t)slots * 64, ctx->stream));
            ctx->hdr_next = 0;
        }
        ta.hdr = (ArenaHdr *)(ctx->d_hdr_ring.as<uint8_t>() + (size_t)ctx->hdr_next++ * 64);
    }
    return SWMI_OK;
}

static ResidentArgs resident_args(const swmi_batch *b) {
    const ChunkPlan &plan = b->plan;
    ResidentArgs xa;
    xa.res_items = plan.n_res ? b->d_res_items.as<uint32_t>() : nullptr;
    xa.n_res = (uint32_t)plan.n_res; xa.res_lds_words = plan.res_lds_words; xa.res_cell_cap = SWMI_RES_CELL_CAP; xa.res_ops_words = plan.res_ops_words;
    return xa;
}

static TFusedArgs tfused_args(const swmi_batch *b) {
    const ChunkPlan &plan = b->plan;
    TFusedArgs xt{};
    xt.items = plan.n_tf ? b->d_tf_items.as<uint32_t>() : nullptr;
    xt.n_items = (uint32_t)plan.n_tf;
    xt.cell_cap = 16;
    xt.tile_words = ((plan.tf_max_m + 63u + 15u) / 16u) * 64u * SWMI_TF_BR;
    xt.ref_words = (plan.tf_max_n + 3u) / 4u + 1u;
    xt.read_words = (plan.tf_max_m + 3u) / 4u + 1u;
    xt.stage_words = (plan.tf_max_path + 3u) / 4u + 1u + SWMI_EMIT_SCRATCH_WORDS;
    static const bool tf_marks = getenv("SWMI_DEBUG_MARKS") != nullptr;
    xt.debug_marks = tf_marks ? 1u : 0u;
    xt.lds_words = (xt.tile_words + 2u * xt.cell_cap + xt.stage_words + xt.ref_words + xt.read_words + 3u) & ~3u;
    // helper wavefronts while their LDS regions fit beside the four sweepers' (the workgroup's LDS less its queues)
    static const int tf_helpers = getenv("SWMI_TF_HELPERS") ? atoi(getenv("SWMI_TF_HELPERS")) : 2;      // (diagnostics: 0 .. SWMI_TF_HELPERS)
    const uint64_t region = 4ull * xt.lds_words, budget = SWMI_LDS_BYTES - 4ull * 1024;
    const uint64_t left = budget > 4 * region ? budget - 4 * region : 0;
    xt.n_helpers = (uint32_t)std::min<uint64_t>((uint64_t)std::max(0, std::min(tf_helpers, (int)SWMI_TF_HELPERS)), region ? left / region : 0);
    return xt;
}

// The affine launch descriptor of the batch's run (swmi_launch.h) -- built here and nowhere else.
static inline AffRun aff_run(const swmi_batch *b) {
    const RunModes &md = b->opt.modes;
    AffRun r{};
    r.gap_open = b->gap_open;
    r.gap_open2 = md.gap_open2; r.gap2 = md.gap_open2 ? md.gap2 : 0;      // (gap2 is not read without gap_open2)
    r.mode = md.kernel_mode();
    r.band = (uint32_t)md.band; r.xdrop = (uint32_t)md.xdrop; r.adapt = (uint32_t)md.band_adapt;
    r.mat = b->opt.mat ? b->d_mat.as<uint32_t>() : nullptr;
    r.nn = b->opt.mat ? b->opt.mat->n + 1u : 0u;
    r.cigar = (uint32_t)md.cigar;
    r.subopt = md.subopt;
    r.hits = (uint32_t)md.hits;
    r.end_bonus = (uint32_t)md.end_bonus;
    return r;
}

// every kernel of one attempt onto the stream, with the profiling events around them and, without zero-copy, the D2H copies
static int enqueue_launches(RunState &rs, Launch &L, const ResidentArgs &xa, const TFusedArgs &xt) {
    swmi_ctx *ctx = rs.ctx;
    swmi_batch *b = rs.b;
    const ChunkPlan &plan = b->plan;
    FillArgs &fa = rs.fa;
    TraceArgs &ta = rs.ta;
    const size_t np = L.np, n_res = plan.n_res, n_tf = plan.n_tf;
    const bool first = L.attempt == 0;
    const AffRun ar = aff_run(b);       // (read by the mode-3 launches only)
    int rc;
    // diagnostics (SWMI_EXT_EVENTS=1): the plain case -- one sweep kernel, one traceback kernel -- timed by the kernels' own
    // dispatches instead of by events around them (the three events cost 3.5 us per run, tests/manual/prof_events_ab.py;
    // hipExtLaunchKernelGGL's start/stop events cost more: profiles/r02/ab_ext_events.txt)
    L.ext_timing = ctx->profiling == 1 && first && !L.whole_only && !n_res && !n_tf && !L.split && b->eff_mode == 1 &&
                   !fa.n_strip_items && !fa.n_col_items && ctx->ext_events;
    const bool ext = L.ext_timing;
    if (ctx->profiling && !ext) HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    if (first && !L.whole_only) {       // the workspace survives an arena-overflow retry
        if (fa.n_strip_items) HIP_TRY(hipMemsetAsync(fa.progress, 0, (size_t)fa.n_strip_items * sizeof(uint32_t), ctx->stream));
        if (b->eff_mode == 3) {
            // the pairs of the strip kernels (reads longer than 1024 bases, option "long_reads") are the last aff_n_long
            FillArgs fs = fa, fl = fa;
            fs.n_pairs = (uint32_t)(np - plan.aff_n_long);
            fl.n_pairs = (uint32_t)plan.aff_n_long; fl.pairs = fa.pairs + fs.n_pairs;
            // (options "band", "xdrop" and "band_adapt" are the strip kernels': the other pairs take the kernels they take without them)
            if (b->opt.prof) {
                // the batch has profiles: the profile sweeps, through their own launcher; such a run has no long pairs
                const AffProfile ap{b->d_prof.as<uint32_t>(), b->opt.prof->n};
                HIP_TRY(swmi_launch_affine_profile_sweep(&fs, &ar, &ap, plan.aff_r_min, plan.aff_r_max, ctx->stream));
            } else
            HIP_TRY(swmi_launch_affine_sweep(&fs, &ar, 0u, plan.aff_r_min, plan.aff_r_max, ctx->stream));
            HIP_TRY(swmi_launch_affine_sweep(&fl, &ar, 1u, 0u, 0u, ctx->stream));
        }
        else HIP_TRY(swmi_launch_fill(&fa, ctx->stream, ext ? ctx->ev[0] : nullptr, ext ? ctx->ev[1] : nullptr));
        rs.launches++;
    }
    if (L.sub) {
        // option "subopt": the reduce over the rows of column maxima the sweeps left, behind them on the stream.  On EVERY attempt:
        // it only reads the workspace, which survives a retry, and the pair outputs, which the retry has put back -- and the pinned
        // block it mirrors into may have been re-allocated.  Timed with the sweep.
        SuboptArgs sa{};
        sa.refs = fa.refs; sa.reads = fa.reads; sa.pairs = fa.pairs; sa.dir = fa.dir; sa.out = fa.out;
        sa.sub = (SuboptOut *)(L.res + result_sub_off(np));
        sa.sub_host = L.zc && !L.sweep_only ? (SuboptOut *)((uint8_t *)b->h_result.dp + result_sub_off(np)) : nullptr;
        sa.n_pairs = (uint32_t)np; sa.band = b->opt.modes.band > 0 ? (uint32_t)b->opt.modes.band : 0u; sa.subopt = ar.subopt;
        if (L.hits) {
            // option "hits": sw_hits_kernel in its place -- it writes the SuboptOut array as well, and the HitEnt array behind it
            HitsArgs ha{};
            ha.s = sa;
            ha.hits = (HitEnt *)(L.res + result_hits_off(np));
            ha.hits_host = sa.sub_host ? (HitEnt *)((uint8_t *)b->h_result.dp + result_hits_off(np)) : nullptr;
            ha.k = L.hits;
            HIP_TRY(swmi_launch_hits(&ha, ctx->stream));
        } else
        HIP_TRY(swmi_launch_subopt(&sa, ctx->stream));
    }
    if (n_tf) HIP_TRY(swmi_launch_tfused(&ta, &xt, ctx->stream));             // (sweep AND traceback of its pairs: timed with the sweep)
    if (L.whole_only && n_tf) rs.launches++;
    if (ctx->profiling && !ext) HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));     // end of the sweep = start of the traceback
    if (n_res) HIP_TRY(swmi_launch_resident(&ta, &xa, ctx->stream));          // (timed with the traceback)
    if (first) b->timing.resident_pairs += (uint32_t)n_res;
    if (first) b->timing.tfused_pairs += (uint32_t)n_tf;
    if (L.sweep_only) {
        // option scores_only: the pair outputs as the sweep kernels left them (the traceback kernels, which otherwise mirror
        // them into the host block, do not run)
        if ((rc = b->h_result.reserve(L.a_off + L.arena_cap * 4))) return rc;
        // (options "subopt" and "end_bonus": and the array that follows them)
        HIP_TRY(hipMemcpyAsync((uint8_t *)b->h_result.p + result_out_off(), L.res + result_out_off(),
                               np * (sizeof(PairOut) + L.sub_bytes()), hipMemcpyDeviceToHost, ctx->stream));
    } else if (L.split) {
        ta.win_off = b->d_win_off.as<uint32_t>();
        ta.q_count = b->d_queue.as<uint32_t>();
        ta.q_items = (uint4 *)(b->d_queue.as<uint8_t>() + 256);
        ta.q_cap = (uint32_t)L.q_cap;
        if (!first || L.whole_only) HIP_TRY(hipMemsetAsync(ta.q_count, 0, 4, ctx->stream));      // (no sweep kernel ran to zero it)
        HIP_TRY(swmi_launch_traceback_split(&ta, (uint32_t)plan.n_windows, ctx->stream));
    } else if (b->eff_mode == 3) {
        TraceArgs ts = ta, tl = ta;
        ts.n_pairs = (uint32_t)(np - plan.aff_n_long);
        tl.n_pairs = (uint32_t)plan.aff_n_long; tl.pairs = ta.pairs + ts.n_pairs;
        const uint32_t ops_words = (uint32_t)(((uint64_t)plan.max_path + 15) / 16 + 1);
        // (option "gap_open2": a block of the field is 2 * R * 64 dwords, and SWMI_AFF_TILE_WORDS holds one -- swmi_device.h)
        HIP_TRY(swmi_launch_affine_traceback(&ts, &ar, 0u, SWMI_AFF_TILE_WORDS, ops_words, ctx->stream));
        HIP_TRY(swmi_launch_affine_traceback(&tl, &ar, 1u, SWMI_AFF_TILE_WORDS, ops_words, ctx->stream));
        if (L.endb && L.zc) {
            // option "end_bonus", zero-copy results: the walks mirror the pair outputs into the pinned block, and this copy puts the
            // sweeps' EndOut array behind them.  On every attempt: the retry has put the array back with the pair outputs
            // (saved_outs), and the pinned block may have been re-allocated.  (Without zero-copy it is part of the D2H copy below.)
            HIP_TRY(hipMemcpyAsync((uint8_t *)b->h_result.p + result_sub_off(np), L.res + result_sub_off(np), np * sizeof(EndOut),
                                   hipMemcpyDeviceToHost, ctx->stream));
        }
    } else if (n_res + n_tf < np) {
        HIP_TRY(swmi_launch_traceback(&ta, ctx->stream, ext ? ctx->ev[2] : nullptr, ext ? ctx->ev[3] : nullptr));
    }
    if (L.time_all && !ext) HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));

    // without zero-copy: one D2H of header + pair outputs + as many table entries and arena words as the previous run used
    // (plus slack); the rare remainder is fetched after the header has been read
    L.copy_words = std::min<uint64_t>(L.arena_cap, std::max<uint64_t>(256, np * ctx->arena_copy_wpp));
    L.copy_recs = std::min<uint64_t>(L.tab_cap, np * ctx->recs_per_pair_x16 / 16 + 64);
    if (!L.zc && !L.sweep_only) {
        if ((rc = b->h_result.reserve(L.a_off + L.arena_cap * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(b->h_result.p, L.res, L.t_off + L.copy_recs * sizeof(AlnRec), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync((uint8_t *)b->h_result.p + L.a_off, L.res + L.a_off, L.copy_words * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (L.time_all) HIP_TRY(hipEventRecord(ctx->ev[4], ctx->stream));
    }
    return SWMI_OK;
}

// a batch is sub-millisecond: poll the stream for spin_us (this context only, no process-wide spin flag), then block
static int wait_for_stream(swmi_ctx *ctx) {
    const auto t0 = Clock::now();
    hipError_t q = hipErrorNotReady;
    while (ctx->spin_us > 0 && (q = hipStreamQuery(ctx->stream)) == hipErrorNotReady && us_between(t0, Clock::now()) < (double)ctx->spin_us)
        __builtin_ia32_pause();
    if (q != hipSuccess && q != hipErrorNotReady) return fail(SWMI_ERR_HIP, "hipStreamQuery: %s", hipGetErrorString(q));
    if (q != hipSuccess) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SWMI_OK;
}

// scores only: a pair swept by several wavefronts (column chunks, strips) has only its maximum combined, and a
// maximum of 0 is the degenerate case (what finish_pair does in the traceback kernels)
static void collect_scores(const swmi_batch *b, const std::vector<Work> &work, const Launch &L, std::vector<PairOut> &outs) {
    const uint8_t *h = (const uint8_t *)b->h_result.p;
    outs.assign((const PairOut *)(h + result_out_off()), (const PairOut *)(h + result_out_off()) + L.np);
    for (size_t k = 0; k < L.np; k++) {
        PairOut &o = outs[k];
        // (the end-to-end modes have no degenerate case: a score of 0 or below is an ordinary score)
        if (o.score <= 0 && !(o.flags & SWMI_F_DEGENERATE) && b->opt.modes.align_mode == 0) {
            const uint32_t pair = work[L.lo + k].pair;
            o.score = 0; o.flags = SWMI_F_DEGENERATE;
            o.n_cells = (uint64_t)b->read_desc[pair_read(b, pair)].len * b->ref_desc[pair_ref(b, pair)].len;
        }
        o.flags &= SWMI_F_DEGENERATE | SWMI_F_TO_END | SWMI_F_STRIPS_MASK;      // (the strips swept under option "xdrop" stay, and the choice of option "end_bonus")
    }
}

// What a finished attempt left: `retry` when records were dropped (arena or table too small: both are grown to the size the
// kernels asked for, the pair outputs saved for the next attempt), else the pair outputs in `outs` and the records kept.
static int collect_launch(RunState &rs, Launch &L, Clock::time_point t_done, std::vector<uint8_t> &saved_outs, std::vector<PairOut> &outs,
                          bool &retry) {
    swmi_ctx *ctx = rs.ctx;
    swmi_batch *b = rs.b;
    const size_t np = L.np;
    const bool zc = L.zc;
    int rc;
    retry = false;
    const uint8_t *h = (const uint8_t *)b->h_result.p;
    ArenaHdr hdr_copy{};
    const ArenaHdr *hdr = (const ArenaHdr *)h;
    bool overflow = false;
    if (zc) {
        overflow = *(const volatile uint32_t *)h != 0u;
        if (overflow) {        // rare: how much was needed is in the device-side header
            HIP_TRY(hipMemcpy(&hdr_copy, rs.ta.hdr, sizeof hdr_copy, hipMemcpyDeviceToHost));
            hdr = &hdr_copy;
        }
    }
    const uint64_t hdr_words = zc && !overflow ? 0 : hdr->reserved & SWMI_HDR_WORD_MASK;     // (zero-copy: only read after an overflow)
    const uint64_t hdr_recs = zc && !overflow ? 0 : hdr->reserved >> SWMI_HDR_WORD_BITS;
    if (!zc) overflow = hdr_words > L.arena_cap || hdr_recs > L.tab_cap;
    if (overflow) {            // records were dropped: grow to the exact need and redo the traceback
        // (option "end_bonus": the sweeps' EndOut array behind the pair outputs is carried along -- no kernel of the retry writes it)
        // (option "hits": the SuboptOut and HitEnt arrays are carried too -- sw_hits_kernel writes them again on the retry, the same values)
        const size_t keep = np * (sizeof(PairOut) + (L.endb || L.hits ? L.sub_bytes() : 0));
        if (zc) {
            saved_outs.resize(keep);
            HIP_TRY(hipMemcpy(saved_outs.data(), L.res + result_out_off(), saved_outs.size(), hipMemcpyDeviceToHost));
        } else {
            saved_outs.assign(h + result_out_off(), h + result_out_off() + keep);
        }
        for (size_t k = 0; k < np; k++) {
            PairOut &so = ((PairOut *)saved_outs.data())[k];
            so.flags &= ~SWMI_F_ARENA_OVF;
            // the split traceback counts a pair's cells by atomics and flags list overflows itself: start both over
            if (L.split && !(so.flags & SWMI_F_DEGENERATE)) { so.n_cells = 0; so.flags &= ~SWMI_F_CELL_OVF; }
        }
        L.arena_cap = std::max<uint64_t>(L.arena_cap, hdr_words + 1024);
        L.tab_cap = std::max<uint64_t>(L.tab_cap, hdr_recs + 64);
        // (the kernels reserve payload and table entry with one 64-bit counter: 36 bits of dwords, 28 bits of records)
        if (L.arena_cap >= SWMI_HDR_WORD_MASK || L.tab_cap >= (1ull << (64u - SWMI_HDR_WORD_BITS)) - 1ull)
            return fail(SWMI_ERR_UNSUPPORTED, "one launch would hold %llu alignment records in %llu arena dwords: lower max_workspace_bytes so that the batch runs in smaller launches",
                        (unsigned long long)L.tab_cap, (unsigned long long)L.arena_cap);
        ctx->arena_words_per_pair = std::max<uint64_t>(ctx->arena_words_per_pair, L.arena_cap / np + 1);
        ctx->recs_per_pair_x16 = std::max<uint64_t>(ctx->recs_per_pair_x16, L.tab_cap * 16 / np + 1);
        retry = true;
        return SWMI_OK;
    }
    outs.assign((const PairOut *)(h + result_out_off()), (const PairOut *)(h + result_out_off()) + np);
    for (auto &o : outs) o.flags &= ~SWMI_F_ARENA_OVF;
    // how many records there are follows from the pair outputs (zero-copy: the header sits in device memory)
    uint64_t n_rec = 0;
    if (zc) {
        for (auto &o : outs)
            if (!(o.flags & (SWMI_F_DEGENERATE | SWMI_F_CELL_OVF))) n_rec += o.n_cells;
    } else {
        n_rec = hdr_recs;
    }
    if (n_rec > L.tab_cap) return fail(SWMI_ERR_HIP, "more records than the table holds");
    const AlnRec *tab = (const AlnRec *)(h + L.t_off);
    const uint32_t *aw = (const uint32_t *)(h + L.a_off);
    if (!zc) {
        if (n_rec > L.copy_recs)
            HIP_TRY(hipMemcpy((uint8_t *)b->h_result.p + L.t_off + L.copy_recs * sizeof(AlnRec), L.res + L.t_off + L.copy_recs * sizeof(AlnRec),
                              (n_rec - L.copy_recs) * sizeof(AlnRec), hipMemcpyDeviceToHost));
        if (hdr_words > L.copy_words)
            HIP_TRY(hipMemcpy((uint8_t *)b->h_result.p + L.a_off + L.copy_words * 4, L.res + L.a_off + L.copy_words * 4,
                              (hdr_words - L.copy_words) * 4, hipMemcpyDeviceToHost));
        ctx->arena_copy_wpp = hdr_words * 5 / (4 * np) + 2;
        ctx->recs_per_pair_x16 = std::max<uint64_t>(ctx->recs_per_pair_x16, n_rec * 20 / np + 1);
    }
    if (rs.keep) {
        if ((rc = keep_chunk_records(rs, tab, n_rec, aw, L.arena_cap, L.lo))) return rc;
        rs.copyout_us += us_between(t_done, Clock::now());
    }
    return SWMI_OK;
}

// Option "band_adapt": the window tables of the launch's long pairs, from the workspace (the next launch rewrites it) into the
// batch, for swmi_pair_band_window.  One small copy per long pair: the tables lie behind the pairs' fields.  The exact-size re-run
// of a pair leaves the same table (same kernel, same inputs) and overwrites the entry.
static int fetch_windows(swmi_batch *b, const std::vector<Work> &work, size_t lo) {
    const ChunkPlan &plan = b->plan;
    if (b->eff_mode != 3 || !b->opt.modes.band_adapt || !plan.aff_n_long) return SWMI_OK;
    const size_t np = b->pairs_on_device.size() / sizeof(PairDesc);
    const PairDesc *pd = (const PairDesc *)b->pairs_on_device.data();
    const AffGeom g = aff_geom(b->opt.modes);
    if (b->win_at.size() != b->pairs.size()) b->win_at.assign(b->pairs.size(), 0);
    for (size_t k = np - plan.aff_n_long; k < np; k++) {
        const uint32_t pair = work[lo + pd[k].out_id].pair;
        const uint32_t m = b->read_desc[pd[k].read_id].len, n = b->ref_desc[pd[k].ref_id].len, ns = swmi_aff_strips(m);
        if (!b->win_at[pair]) { b->win_at[pair] = b->win_tab.size() + 1; b->win_tab.resize(b->win_tab.size() + ns, 0u); }
        HIP_TRY(hipMemcpy(b->win_tab.data() + (b->win_at[pair] - 1), b->d_dir.as<uint32_t>() + pd[k].dir_off + swmi_aff_pair_table_off(m, n, g),
                          (size_t)ns * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return SWMI_OK;
}

// Runs the kernels for work[lo, hi) -- one launch of each kernel the chunk needs -- waits, and keeps the records; a record arena
// or table that proves too small is grown to the size the kernels asked for and the traceback repeated.
// Cell-list geometry: uniform (cell_cap per pair) when cells_exact is null, else exact per pair (the re-run of overflowed pairs).
static int run_chunk(RunState &rs, const std::vector<Work> &work, size_t lo, size_t hi,
                     const std::vector<uint64_t> *cells_exact, std::vector<PairOut> &outs) {
    swmi_ctx *ctx = rs.ctx;
    swmi_batch *b = rs.b;
    const size_t np = hi - lo;
    int rc;
    if ((rc = prepare_chunk(rs, work, lo, hi, cells_exact))) return rc;
    const ChunkPlan &plan = b->plan;
    if (plan.seam_words) HIP_TRY(hipMemsetAsync(b->d_seam.p, 0, plan.seam_words * 4, ctx->stream));

    Launch L;
    L.np = np; L.lo = lo; L.cells_exact = cells_exact;
    if ((rc = size_cell_lists(rs, L))) return rc;
    {
        // the traceback stages one alignment's ops and the read per walker (4 per workgroup) next to its direction tiles:
        // the LDS of a workgroup bounds the longest pair (m + n of about 16 k bases in mode 0, 24 k in modes 1/2)
        // (mode 3: the affine traceback's direction tile, the ops packed 16 per dword and the string scratch)
        const uint64_t need = b->eff_mode == 3 ? 4ull * (SWMI_AFF_TILE_WORDS + ((uint64_t)plan.max_path + 15) / 16 + 1 + SWMI_EMIT_SCRATCH_WORDS)
                                               : traceback_lds_bytes(b->eff_mode, plan.max_path, plan.max_read);
        if (need > SWMI_LDS_BYTES)
            return fail(SWMI_ERR_UNSUPPORTED, "a pair of %u bases in total needs %llu bytes of LDS for the traceback (limit %u)",
                        plan.max_path, (unsigned long long)need, SWMI_LDS_BYTES);
    }
    // (the exact-size re-run of pairs whose lists overflowed takes one workgroup per pair: its lists have no per-window cap)
    L.split = rs.tb_split && !cells_exact && b->eff_mode == 1 && plan.n_windows < 0xFFFFFFFFull;
    L.zc = ctx->zero_copy != 0;
    L.sweep_only = ctx->scores_only != 0 && !cells_exact;
    L.time_all = ctx->profiling == 1;
    L.sub = b->eff_mode == 3 && b->opt.modes.subopt != 0;
    L.hits = L.sub ? (uint32_t)b->opt.modes.hits : 0u;
    L.endb = b->eff_mode == 3 && b->opt.modes.end_bonus != 0;

    const auto c0 = Clock::now();
    L.arena_cap = std::max<uint64_t>(np * ctx->arena_words_per_pair, 1024);
    L.tab_cap = std::max<uint64_t>(np * ctx->recs_per_pair_x16 / 16 + 64, 256);
    std::vector<uint8_t> saved_outs;       // PairOut block carried across an arena re-allocation
    for (L.attempt = 0;; L.attempt++) {
        // (an overflow that growing cannot cure -- a path longer than the staging area -- must not retry for ever)
        if (L.attempt > 4) return fail(SWMI_ERR_HIP, "the record arena overflowed %d times in a row; results discarded", L.attempt);
        L.t_off = result_tab_off(np, L.sub_bytes()); L.a_off = result_arena_off(np, L.tab_cap, L.sub_bytes());
        if ((rc = b->d_result.reserve(L.a_off + L.arena_cap * 4))) return rc;
        L.res = b->d_result.as<uint8_t>();
        if (L.attempt > 0) {         // (on the first attempt the fill kernel zeroes the arena header itself)
            HIP_TRY(hipMemsetAsync(L.res, 0, 64, ctx->stream));
            HIP_TRY(hipMemcpyAsync(L.res + result_out_off(), saved_outs.data(), saved_outs.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        if ((rc = build_fill_args(rs, L))) return rc;
        if ((rc = build_trace_args(rs, L))) return rc;
        if ((rc = enqueue_launches(rs, L, resident_args(b), tfused_args(b)))) return rc;
        static const char *watchdog = getenv("SWMI_DEBUG_WATCHDOG");      // diagnostics: give up on a launch that does not end
        if (watchdog) watchdog_wait(ctx->stream, b, watchdog);
        const auto c1 = Clock::now();
        if ((rc = wait_for_stream(ctx))) return rc;
        const auto c2 = Clock::now();
        volatile uint32_t *giveup = L.zc ? (volatile uint32_t *)b->h_result.p + 1 : (volatile uint32_t *)ctx->h_err.p + 5;
        if (*giveup != 0u) {      // sw_tfused_kernel gave up a wait that cannot last (never seen)
            const uint32_t code = *giveup;
            *giveup = 0u;
            return fail(SWMI_ERR_HIP, "sw_tfused_kernel: internal wait abandoned (code %08x); results discarded", code);
        }
        if (*(volatile uint32_t *)ctx->h_err.p != 0u) {
            // a strip of the pipelined sweep gave up waiting for its producer wavefront (it was not dispatched, or did not
            // move for the whole spin budget): nothing of this launch is used.  The chunk is swept again with ONE wavefront
            // per pair, strip after strip -- no wavefront of that sweep waits for another workgroup.
            *(volatile uint32_t *)ctx->h_err.p = 0u;
            if (rs.one_wave_sweep)
                return fail(SWMI_ERR_HIP, "the sweep raised its error flag without the strip pipeline; results discarded");
            rs.one_wave_sweep = true;
            b->timing.strip_fallbacks++;
            return run_chunk(rs, work, lo, hi, cells_exact, outs);
        }
        rs.enqueue_us += us_between(c0, c1);
        rs.wait_us += us_between(c1, c2);
        if (ctx->profiling) {
            float ms = 0;
            if (L.attempt == 0 || L.whole_only) { HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1])); rs.fill_ms += ms; }
            if (L.time_all) { HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[L.ext_timing ? 2 : 1], ctx->ev[3])); rs.tb_ms += ms; }
            if (L.time_all && !L.zc) { HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4])); rs.d2h_ms += ms; }
        }
        if (rs.ta.dbg && (rc = dump_traceback_diagnostics(b, rs.ta, np, plan.n_tf))) return rc;
        if (rs.fa.dbg && L.attempt == 0 && (rc = dump_fill_diagnostics(b, rs.fa, np))) return rc;
        if (L.attempt == 0 && (rc = fetch_windows(b, work, lo))) return rc;      // (the workspace survives an arena-overflow retry)
        if (L.sub) {
            // option "subopt": the launch's (score2, end2), in the host block by now -- written there by the kernel (zero-copy) or
            // part of the D2H copy.  The exact-size re-run of a pair computes the same values and overwrites them.
            const SuboptOut *hs = (const SuboptOut *)((const uint8_t *)b->h_result.p + result_sub_off(np));
            for (size_t k = 0; k < np; k++) b->sub[work[lo + k].pair] = hs[k];
        }
        if (L.hits) {
            // option "hits": likewise the launch's 1 + K entries per pair
            const HitEnt *hh = (const HitEnt *)((const uint8_t *)b->h_result.p + result_hits_off(np));
            const size_t per = 1u + L.hits;
            for (size_t k = 0; k < np; k++) std::copy(hh + k * per, hh + (k + 1) * per, b->hitv.begin() + (size_t)work[lo + k].pair * per);
        }
        if (L.endb) {
            // option "end_bonus": the launch's (max_score, end_score, end_col), in the host block by now -- part of a D2H copy on every
            // path.  The exact-size re-run of a pair (one that was not taken to the end) computes the same values and overwrites them.
            const EndOut *he = (const EndOut *)((const uint8_t *)b->h_result.p + result_sub_off(np));
            for (size_t k = 0; k < np; k++) b->endv[work[lo + k].pair] = he[k];
        }
        if (L.sweep_only) { collect_scores(b, work, L, outs); return SWMI_OK; }
        bool retry;
        if ((rc = collect_launch(rs, L, c2, saved_outs, outs, retry)) || !retry) return rc;
    }
}

// ------------------------------------------------------------------------------------------
// a run of the whole batch
// ------------------------------------------------------------------------------------------
// Option "band" (half-width w) with at least one read longer than 1024 bases: what a banded run refuses (swmi.h),
// in 64-bit arithmetic.  rows = 1024 * strips of the longest read, S = the largest |score|, max_n = the longest reference.
// Every condition is monotone in m and n, so the extreme lengths decide for every long pair of the batch.
// go, ge: the gap open and extension the bounds are read with -- under option "gap_open2" the larger |.| of the two pieces
static int check_band(const swmi_ctx *ctx, const swmi_batch *b, const swmi_params *p, const RunModes &md, uint64_t rows, int64_t S,
                      uint64_t max_n, int64_t go, int64_t ge) {
    const int align_mode = md.align_mode, band = md.band;
    const int64_t w = band;
    uint64_t min_n = UINT64_MAX, min_long = UINT64_MAX, max_m = 0;
    for (uint32_t r = 0; r < b->n_refs; r++)
        if (b->ref_desc[r].len) min_n = std::min<uint64_t>(min_n, b->ref_desc[r].len);       // (a pair with an empty side is not swept)
    for (uint32_t q = 0; q < b->n_reads; q++) {
        const uint64_t m = b->read_desc[q].len;
        if (m > SWMI_AFF_MAX_READ) min_long = std::min(min_long, m);
        max_m = std::max(max_m, m);
    }
    // a strip whose window is empty: the last strip's window starts at column 1024 (NS - 1) + 1 - w
    // (option "band_adapt": no window is ever empty -- its centre is a column of the reference)
    const int64_t last_lo = (int64_t)rows - SWMI_AFF_MAX_READ + 1 - w;
    if (!md.band_adapt && (int64_t)min_n < last_lo)
        return fail(SWMI_ERR_UNSUPPORTED, "band %d: the last strip of the longest read (%llu bases) starts at column %lld, past the end of the "
                    "shortest reference (%llu)", band, (unsigned long long)max_m, (long long)last_lo, (unsigned long long)min_n);
    // global mode: the one cell (m, n) must lie in the band, n <= 1024 NS + w (option "extend": the end cell is free -- the
    // maximum is taken over the in-band cells, and the reference may run on past the band)
    const uint64_t min_rows = (uint64_t)SWMI_AFF_MAX_READ * swmi_aff_strips((uint32_t)min_long);
    if (align_mode == SWMI_ALIGN_GLOBAL && !md.extend && max_n > min_rows + (uint64_t)w)
        return fail(SWMI_ERR_UNSUPPORTED, "band %d, align_mode global: the end of the longest reference (%llu) lies outside the band of a read of "
                    "%llu bases (at most %llu)", band, (unsigned long long)max_n, (unsigned long long)min_long, (unsigned long long)(min_rows + w));
    // the arithmetic bounds of a banded run: half of an unbanded run's, which leaves room for the value of a cell outside the band
    if (align_mode != SWMI_ALIGN_LOCAL && (int64_t)rows * S > ((int64_t)1 << 29))
        return fail(SWMI_ERR_UNSUPPORTED, "band %d, align_mode fit / global: the longest read (%llu bases) is swept as %llu rows, and %llu * %lld (the "
                    "largest |score|) is above 2^29", band, (unsigned long long)max_m, (unsigned long long)rows, (unsigned long long)rows, (long long)S);
    if (md.band_adapt) {
        // moving windows: an existing cell is reached by a staircase of gap moves with two gap openings per strip and the
        // boundary's, where the static band has a diagonal and three openings
        const int64_t low = swmi_adapt_low(max_m, max_n, ctx->gap_open, p->gap);
        if (!swmi_adapt_bound_ok(max_m, max_n, ctx->gap_open, p->gap))
            return fail(SWMI_ERR_UNSUPPORTED, "band %d, band_adapt: (2 * ceil(m / 1024) + 1) * gap_open + (1024 * ceil(m / 1024) + n) * gap = %lld for the "
                        "longest read (%llu) and reference (%llu) is below -2^30", band, (long long)low, (unsigned long long)max_m, (unsigned long long)max_n);
    } else if (align_mode == SWMI_ALIGN_GLOBAL) {
        const int64_t low = 3 * go + (int64_t)(rows + max_n) * ge;
        if (low < -((int64_t)1 << 30))
            return fail(SWMI_ERR_UNSUPPORTED, "band %d, align_mode global: 3 * gap_open + (1024 * ceil(m / 1024) + n) * gap = %lld for the longest "
                        "read (%llu) and reference (%llu) is below -2^30", band, (long long)low, (unsigned long long)max_m, (unsigned long long)max_n);
    }
    // the field of the largest pair alone against the workspace cap (it grows with m and with n)
    const uint64_t bytes = swmi_aff_pair_dir_words((uint32_t)max_m, (uint32_t)max_n, aff_geom(md)) * 4;
    if (bytes > ctx->max_workspace_bytes && md.two_piece())
        return fail(SWMI_ERR_UNSUPPORTED, "band %d, gap_open2: the two-plane direction field of the longest read (%llu) against the longest reference (%llu) "
                    "takes %llu bytes (twice the one-piece field), more than max_workspace_bytes (%llu)", band, (unsigned long long)max_m,
                    (unsigned long long)max_n, (unsigned long long)bytes, (unsigned long long)ctx->max_workspace_bytes);
    if (bytes > ctx->max_workspace_bytes)
        return fail(SWMI_ERR_UNSUPPORTED, "band %d: the direction field of the longest read (%llu) against the longest reference (%llu) takes %llu "
                    "bytes, more than max_workspace_bytes (%llu)", band, (unsigned long long)max_m, (unsigned long long)max_n,
                    (unsigned long long)bytes, (unsigned long long)ctx->max_workspace_bytes);
    return SWMI_OK;
}

// what a run cannot compute, refused before anything is launched (under ctx->mu: the context's options are read)
// opt: the run's options (the context's when the run was asked for)
static int check_run_params(const swmi_ctx *ctx, const swmi_batch *b, const swmi_params *p, bool affine, const RunOptions &opt) {
    const RunModes &md = opt.modes;
    const ScoreMatrix *mat = opt.mat.get();
    // option "overlap" frees the read's ends of a fit run: defined, and built, for unbanded one-piece fit runs alone.
    // Refused first, whatever pipeline the run would take: an overlap run takes the affine kernels (align_mode fit does)
    if (md.overlap) {
        if (md.align_mode != SWMI_ALIGN_FIT)
            return fail(SWMI_ERR_UNSUPPORTED, "overlap = %d needs align_mode fit (1), got align_mode %d", md.overlap, md.align_mode);
        const struct { const char *name; int value; } no[] = {{"band", md.band}, {"extend", md.extend}, {"xdrop", md.xdrop}, {"band_adapt", md.band_adapt},
                                                               {"gap_open2", md.gap_open2}, {"subopt", md.subopt}, {"hits", md.hits}, {"end_bonus", md.end_bonus}};
        for (const auto &x : no)
            if (x.value != 0) return fail(SWMI_ERR_UNSUPPORTED, "overlap = %d with %s = %d is not supported", md.overlap, x.name, x.value);
    }
    // option "subopt": the second-best score is defined, and built, for local runs -- which also rules out extend, xdrop, band_adapt
    // and gap_open2, options of a global run
    if (md.subopt != 0 && md.align_mode != SWMI_ALIGN_LOCAL)
        return fail(SWMI_ERR_UNSUPPORTED, "subopt = %d needs align_mode local (0), got align_mode %d", md.subopt, md.align_mode);
    // option "hits": the K-round pick runs on the rows the sweeps of option "subopt" leave, which also gives the mask half-width
    if (md.hits != 0 && md.subopt == 0)
        return fail(SWMI_ERR_UNSUPPORTED, "hits = %d needs a run under subopt (the mask half-width, or -1), got subopt 0", md.hits);
    // option "end_bonus": the to-end score is defined, and built, for one-piece extend runs whose sweep reaches read row m with the
    // static windows -- the linear pipeline has no such run, and an extend run takes the affine kernels anyway
    if (md.end_bonus != 0) {
        if (!(md.extend && md.align_mode == SWMI_ALIGN_GLOBAL))
            return fail(SWMI_ERR_UNSUPPORTED, "end_bonus = %d needs an extend run (align_mode global (2) with extend = 1), got align_mode %d, extend %d",
                        md.end_bonus, md.align_mode, md.extend);
        if (md.xdrop > 0) return fail(SWMI_ERR_UNSUPPORTED, "end_bonus = %d: the to-end score under xdrop is not supported (a stopped pair has no row m)", md.end_bonus);
        if (md.band_adapt) return fail(SWMI_ERR_UNSUPPORTED, "end_bonus = %d: the to-end score under band_adapt is not supported", md.end_bonus);
        if (md.two_piece()) return fail(SWMI_ERR_UNSUPPORTED, "end_bonus = %d: the to-end score with two-piece gaps (gap_open2) is not supported", md.end_bonus);
    }
    // The batch's per-read profiles (swmi_batch_set_read_profiles): built for the one-piece sweeps of reads of at
    // most 1024 bases in the five modes, with one table per wavefront in LDS
    const ReadProfiles *prof = opt.prof.get();
    if (prof) {
        if (mat) return fail(SWMI_ERR_UNSUPPORTED, "read profiles (%u symbols) with a score matrix (%u symbols) set on the context are not supported: "
                             "clear one of them", prof->n, mat->n);
        const struct { const char *name; int value; } no[] = {{"gap_open2", md.gap_open2}, {"subopt", md.subopt}, {"hits", md.hits}, {"end_bonus", md.end_bonus}};
        for (const auto &x : no)
            if (x.value != 0) return fail(SWMI_ERR_UNSUPPORTED, "read profiles (%u symbols) with %s = %d are not supported", prof->n, x.name, x.value);
        uint64_t pm, pn;
        longest_sequences(b, pm, pn);
        if (pm > SWMI_AFF_MAX_READ)
            return fail(SWMI_ERR_UNSUPPORTED, "read profiles (%u symbols): the longest read has %llu bases (at most %u: a longer read needs one table per strip)",
                        prof->n, (unsigned long long)pm, SWMI_AFF_MAX_READ);
        const uint64_t M = 64 * ((pm + 63) / 64);
        if (M * (prof->n + 1u) > SWMI_PROF_LDS_WORDS)
            return fail(SWMI_ERR_UNSUPPORTED, "read profiles (%u symbols): the longest read (%llu bases) needs a table of %llu * %u = %llu entries in LDS "
                        "(at most %u)", prof->n, (unsigned long long)pm, (unsigned long long)M, prof->n + 1u, (unsigned long long)(M * (prof->n + 1u)),
                        SWMI_PROF_LDS_WORDS);
    }
    if (p->tie_mode != SWMI_TIE_SERIAL && p->tie_mode != SWMI_TIE_STRICT)
        return fail(SWMI_ERR_INVALID, "unknown tie_mode %d", p->tie_mode);
    // GetAlignment tests `align == alignTypes[0]`, then `== alignTypes[1]`, else deletion
    // (SmithWaterman.java:388-401): with duplicate a/i/d characters the reference itself walks wrong
    // cells; that behaviour is not reproduced.
    if (p->types[0] == p->types[1] || p->types[0] == p->types[2] || p->types[1] == p->types[2])
        return fail(SWMI_ERR_UNSUPPORTED, "alignTypes a/i/d must be pairwise distinct");
    // option "extend" is global mode's sweep with another choice of maximum cells: there is no such sweep for local and fit
    if (md.extend && md.align_mode != SWMI_ALIGN_GLOBAL)
        return fail(SWMI_ERR_UNSUPPORTED, "extend = 1 needs align_mode global (2), got align_mode %d", md.align_mode);
    // option "xdrop" is the drop-off rule of an extend run: no other run has a running maximum over every cell to fall below
    if (md.xdrop > 0 && !(md.extend && md.align_mode == SWMI_ALIGN_GLOBAL))
        return fail(SWMI_ERR_UNSUPPORTED, "xdrop = %d needs an extend run (align_mode global (2) with extend = 1), got align_mode %d, extend %d",
                    md.xdrop, md.align_mode, md.extend);
    // option "band_adapt" moves the band of a banded extend run: there is nothing to move in any other run
    if (md.band_adapt && !(md.band > 0 && md.extend && md.align_mode == SWMI_ALIGN_GLOBAL))
        return fail(SWMI_ERR_UNSUPPORTED, "band_adapt = 1 needs a banded extend run (band > 0, align_mode global (2) with extend = 1), got band %d, "
                    "align_mode %d, extend %d", md.band, md.align_mode, md.extend);
    // option "gap_open2": two-piece gaps are built for plain global and extend runs; gap2 is not read without it
    if (md.two_piece()) {
        if (md.align_mode != SWMI_ALIGN_GLOBAL)
            return fail(SWMI_ERR_UNSUPPORTED, "gap_open2 = %d needs align_mode global (2), with or without extend; got align_mode %d", md.gap_open2, md.align_mode);
        if (mat) return fail(SWMI_ERR_UNSUPPORTED, "gap_open2 = %d: two-piece gaps with a score matrix are not supported", md.gap_open2);
        if (md.xdrop > 0) return fail(SWMI_ERR_UNSUPPORTED, "gap_open2 = %d: two-piece gaps under xdrop are not supported", md.gap_open2);
        if (md.band_adapt) return fail(SWMI_ERR_UNSUPPORTED, "gap_open2 = %d: two-piece gaps under band_adapt are not supported", md.gap_open2);
    }
    // the gap open and extension the bounds are read with: the larger |.| of the two pieces (all four are <= 0)
    const int64_t o2 = md.two_piece() ? md.gap_open2 : 0, e2 = md.two_piece() ? md.gap2 : 0;
    const int64_t go = std::min<int64_t>(ctx->gap_open, o2), ge = std::min<int64_t>(p->gap, e2);
    uint64_t max_m, max_n;
    if (affine) {
        // the bounds within which every sum of the affine recurrence fits int32 (DESIGN.md "Affine gaps")
        const int64_t lim = 1 << 20;
        if (p->gap > 0)
            return fail(SWMI_ERR_UNSUPPORTED, "affine gaps need gap <= 0 (the per-base extension), got %d", p->gap);
        if (std::llabs((int64_t)p->match) > lim || std::llabs((int64_t)p->mismatch) > lim || std::llabs((int64_t)p->gap) > lim ||
            std::llabs((int64_t)ctx->gap_open) > lim)
            return fail(SWMI_ERR_UNSUPPORTED, "affine gaps need |match|, |mismatch|, |gap|, |gap_open| <= 2^20");
        if (std::llabs(o2) > lim || std::llabs(e2) > lim)
            return fail(SWMI_ERR_UNSUPPORTED, "two-piece gaps need |gap_open2|, |gap2| <= 2^20");
        for (uint32_t q = 0; q < b->n_reads && !md.long_reads; q++)
            if (b->read_desc[q].len > SWMI_AFF_MAX_READ)
                return fail(SWMI_ERR_UNSUPPORTED, "affine gaps: read %u has %u bases (at most %u; option long_reads lifts the limit)", q,
                            b->read_desc[q].len, SWMI_AFF_MAX_READ);
        longest_sequences(b, max_m, max_n);
        // the rows a sweep computes for the longest read: whole strips of 1024 above 1024 bases, else whole lanes' rows
        const uint64_t rows = max_m > SWMI_AFF_MAX_READ ? (uint64_t)SWMI_AFF_MAX_READ * swmi_aff_strips((uint32_t)max_m) : 64 * ((max_m + 63) / 64);
        if (md.long_reads) {
            // M * S <= 2^30 (swmi.h, DESIGN.md "Long reads"): H <= M * S, and no sum of the recurrence leaves int32
            int64_t S = std::max(std::max(std::llabs((int64_t)p->match), std::llabs((int64_t)p->mismatch)),
                                 std::max(std::llabs((int64_t)p->gap), std::llabs((int64_t)ctx->gap_open)));
            S = std::max<int64_t>(S, std::max<int64_t>(std::llabs(o2), std::llabs(e2)));
            if (mat)
                for (size_t x = 256; x < mat->image.size(); x++) S = std::max<int64_t>(S, std::llabs((int64_t)(int32_t)mat->image[x]));
            if (prof) S = std::max<int64_t>(S, prof->max_abs);
            if ((int64_t)rows * S > ((int64_t)1 << 30))
                return fail(SWMI_ERR_UNSUPPORTED, "long_reads: the longest read (%llu bases) is swept as %llu rows, and %llu * %lld (the largest "
                            "|score|) is above 2^30", (unsigned long long)max_m, (unsigned long long)rows, (unsigned long long)rows, (long long)S);
            if (md.band > 0 && max_m > SWMI_AFF_MAX_READ && max_n) {
                int rc = check_band(ctx, b, p, md, rows, S, max_n, go, ge);
                if (rc) return rc;
            }
            // a pair of several strips is one launch's work at the least: refused when its field alone is over the cap
            // (a banded run is checked with its own, smaller field in check_band)
            const uint64_t bytes = md.band <= 0 && max_m > SWMI_AFF_MAX_READ && max_n
                                       ? swmi_aff_pair_dir_words((uint32_t)max_m, (uint32_t)max_n, aff_geom(md)) * 4 : 0;
            if (bytes > ctx->max_workspace_bytes && md.two_piece())
                return fail(SWMI_ERR_UNSUPPORTED, "long_reads, gap_open2: the two-plane direction field of the longest read (%llu) against the longest "
                            "reference (%llu) takes %llu bytes (twice the one-piece field), more than max_workspace_bytes (%llu)", (unsigned long long)max_m,
                            (unsigned long long)max_n, (unsigned long long)bytes, (unsigned long long)ctx->max_workspace_bytes);
            if (bytes > ctx->max_workspace_bytes)
                return fail(SWMI_ERR_UNSUPPORTED, "long_reads: the direction field of the longest read (%llu) against the longest reference (%llu) "
                            "takes %llu bytes, more than max_workspace_bytes (%llu)", (unsigned long long)max_m, (unsigned long long)max_n,
                            (unsigned long long)bytes, (unsigned long long)ctx->max_workspace_bytes);
        }
        if (md.align_mode == SWMI_ALIGN_GLOBAL) {
            // global mode: the smallest sum a sweep forms is 3 * gap_open + (64 * ceil(m / 64) + n) * gap (swmi.h, DESIGN.md
            // "End-to-end modes"); it must not leave int32.  Checked per pair in 64-bit arithmetic: it falls with m and n, so
            // the longest read against the longest reference decides.
            const int64_t low = 3 * go + (int64_t)(rows + max_n) * ge;
            if (max_m && max_n && low < (int64_t)INT32_MIN)
                return fail(SWMI_ERR_UNSUPPORTED, "align_mode global: 3 * gap_open + (64 * ceil(m / 64) + n) * gap = %lld for the longest read "
                            "(%llu) and reference (%llu) is below -2^31", (long long)low, (unsigned long long)max_m, (unsigned long long)max_n);
        }
    }
    if (!affine && p->gap > 0) {
        // The cell streams form the gap candidate as max(up, left) + gap where the reference wraps W + gap and N + gap each on
        // its own (SmithWaterman.java:227,235).  The two agree while no H + gap passes 2^31 - 1, always so for gap <= 0.  An H
        // is the exact sum of the scores along its path (a wrapped sum is negative and loses to 0), a path of at most m + n
        // moves: the largest positive score s1 at most (2^31 - 1) / s1 times, every other move at most the next positive
        // score s2.  A positive gap under which that bound plus gap leaves int32 is refused (swmi.h).
        longest_sequences(b, max_m, max_n);
        const uint64_t B = 0x7FFFFFFFull, moves = max_m + max_n;
        uint64_t pos[3] = {(uint64_t)std::max(p->match, 0), (uint64_t)std::max(p->mismatch, 0), (uint64_t)p->gap};
        std::sort(pos, pos + 3, std::greater<uint64_t>());
        const uint64_t s1 = pos[0], s2 = pos[1] != s1 ? pos[1] : (pos[2] != s1 ? pos[2] : 0);
        uint64_t h_max = std::min(moves, B / s1) * s1 + (s2 ? std::min(moves, B / s2) * s2 : 0);
        h_max = std::min(h_max, B);
        if (max_m && max_n && h_max + (uint64_t)p->gap > B)
            return fail(SWMI_ERR_UNSUPPORTED, "a positive gap score of %d could make H + gap pass 2^31 - 1 on a pair of %llu + %llu bases "
                        "(H may reach %llu); such sums are not reproduced", p->gap, (unsigned long long)max_m, (unsigned long long)max_n,
                        (unsigned long long)h_max);
    }
    return SWMI_OK;
}

// Grain of the mode-1 traceback, chosen once per batch and parameter set: a sample of the pairs is aligned and the
// tied maxima per pair are counted.  Periodic references (the reference's own EngineerData sets: every period ends
// in a tied maximum, EngineerData.java:118) give every pair many alignments; one workgroup per pair then walks them
// four at a time while most of the chip idles, so such batches take the split traceback (one wavefront per
// window and per alignment, swmi_traceback.hip).
// (measured, profiles/r02/sweeps_*.md: with ~5 alignments per pair the split traceback wins up to ~200 pairs; from a
// few hundred pairs on one workgroup per pair keeps every SIMD busy anyway and its teams share the window re-sweeps)
static int choose_traceback_grain(swmi_ctx *ctx, swmi_batch *b, const swmi_params *p) {
    const uint64_t n_pairs = batch_n_pairs(b);
    if (!(ctx->tb_split < 0 && !ctx->scores_only && b->eff_mode == 1 && n_pairs >= 64 && n_pairs <= 256 &&
          (b->auto_choice < 0 || memcmp(&b->auto_params, p, sizeof(swmi_params)) != 0)))
        return SWMI_OK;
    std::vector<Work> sample;
    const uint64_t want = 48, stride = std::max<uint64_t>(1, n_pairs / want);
    for (uint64_t pi = stride / 2; pi < n_pairs && sample.size() < want; pi += stride) {
        const uint32_t m = b->read_desc[pair_read(b, pi)].len, n = b->ref_desc[pair_ref(b, pi)].len;
        if (m == 0 || n == 0) continue;
        Work w;
        w.pair = (uint32_t)pi; w.cells = (uint64_t)m * n;
        w.dir_words = swmi_dir_words(m, n, 1); w.seam_words = swmi_seam_words(m, n);
        sample.push_back(w);
    }
    int choice = 1;
    if (!sample.empty()) {
        RunState rs0;
        rs0.ctx = ctx; rs0.b = b;
        rs0.tb_split = true;                      // (48 pairs: a small launch)
        rs0.keep = false;                         // (its records are not results)
        std::vector<PairOut> o0;
        int rc = run_chunk(rs0, sample, 0, sample.size(), nullptr, o0);
        if (rc) return rc;
        uint64_t cells = 0, live = 0;
        for (auto &o : o0)
            if (!(o.flags & SWMI_F_DEGENERATE)) { cells += o.n_cells; live++; }
        if (live && cells * 100 >= (uint64_t)ctx->auto_ties_x100 * live) choice = 0;
        b->plan_key = PlanKey{};                  // (the cached plan was the sample's)
        b->timing = swmi_timing{};
    }
    b->auto_choice = choice;                      // 0: tie-heavy
    b->auto_params = *p;
    return SWMI_OK;
}

// The schedule: every pair with two non-empty sides (pairs with an empty side never enter ScoreMatrix's loops,
// SmithWaterman.java:157-159: (0, [])).  It depends on the sequence lengths and the run's SchedKey only: kept until one of them changes.
static void build_schedule(const swmi_ctx *ctx, swmi_batch *b) {
    const SchedKey key(b->eff_mode, ctx->tfused == 1, b->opt.modes);
    if (b->work_key == key) return;
    const uint32_t n_refs = b->n_refs, n_reads = b->n_reads;
    b->work.clear();
    b->work.reserve(batch_n_pairs(b));
    b->work_cells = 0;
    // Longest first: the tail of a launch is made of short pairs.  The schedule depends on the LENGTHS only, so the two
    // sides are ordered by length once (n_refs log n_refs + n_reads log n_reads) and the pairs generated in that order --
    // by cells, exactly, whenever one side has a single length (one read, or a FASTA file of equal reads), else by
    // reference length first -- instead of sorting 10^6..10^8 pair records.
    std::vector<uint32_t> ro(b->paired ? 0u : n_refs), qo(b->paired ? 0u : n_reads);     // (a pair list is sorted pair by pair, below)
    std::iota(ro.begin(), ro.end(), 0u);
    std::iota(qo.begin(), qo.end(), 0u);
    std::stable_sort(ro.begin(), ro.end(), [&](uint32_t a, uint32_t c) { return b->ref_desc[a].len > b->ref_desc[c].len; });
    std::stable_sort(qo.begin(), qo.end(), [&](uint32_t a, uint32_t c) { return b->read_desc[a].len > b->read_desc[c].len; });
    const bool refs_uniform = !ro.empty() && b->ref_desc[ro.front()].len == b->ref_desc[ro.back()].len;
    // (mode 3: what the run's options make of a pair's field and seam row -- swmi_aff_pair_*, swmi_device.h)
    const bool aff = b->eff_mode == 3, tf = key.tfused;
    const AffGeom g = key.geom;
    auto seam_words = [aff, g](uint32_t m, uint32_t n) { return aff ? swmi_aff_pair_seam_words(m, n, g) : swmi_seam_words(m, n); };
    auto dir_words = [&](uint32_t m, uint32_t n) { return aff ? swmi_aff_pair_dir_words(m, n, g) : swmi_dir_words(m, n, b->eff_mode, tf); };
    auto add = [&](uint32_t r, uint32_t q, uint32_t n, uint32_t m, uint64_t dw, uint64_t sw) {
        Work w;
        w.pair = b->paired ? r : r * n_reads + q;
        w.cells = (uint64_t)m * n;
        w.dir_words = dw; w.seam_words = sw;
        b->work_cells += w.cells;
        b->work.push_back(w);
    };
    if (b->paired) {
        // a pair list: the pairs by cells, descending, in list order among equals; a pair with an empty side is left out
        for (uint32_t k = 0; k < n_refs; k++) {
            const uint32_t m = b->read_desc[k].len, n = b->ref_desc[k].len;
            if (m && n) add(k, k, n, m, 0, 0);
        }
        std::stable_sort(b->work.begin(), b->work.end(), [](const Work &a, const Work &c) { return a.cells > c.cells; });
        uint32_t last_m = 0xFFFFFFFFu, last_n = 0xFFFFFFFFu;
        uint64_t dw = 0, sw = 0;
        for (Work &w : b->work) {
            const uint32_t m = b->read_desc[w.pair].len, n = b->ref_desc[w.pair].len;
            if (m != last_m || n != last_n) { dw = dir_words(m, n); sw = seam_words(m, n); last_m = m; last_n = n; }
            w.dir_words = dw; w.seam_words = sw;
        }
    } else if (refs_uniform) {                       // (reads outermost: descending m x the one n)
        for (uint32_t q : qo) {
            const uint32_t m = b->read_desc[q].len;
            if (m == 0) continue;
            const uint32_t n = n_refs ? b->ref_desc[ro[0]].len : 0;
            if (n == 0) break;
            const uint64_t dw = dir_words(m, n), sw = seam_words(m, n);
            for (uint32_t r : ro) add(r, q, n, m, dw, sw);
        }
    } else {
        uint32_t last_m = 0xFFFFFFFFu;
        uint64_t dw = 0, sw = 0;
        for (uint32_t r : ro) {
            const uint32_t n = b->ref_desc[r].len;
            if (n == 0) continue;
            last_m = 0xFFFFFFFFu;
            for (uint32_t q : qo) {
                const uint32_t m = b->read_desc[q].len;
                if (m == 0) continue;
                if (m != last_m) { dw = dir_words(m, n); sw = seam_words(m, n); last_m = m; }
                add(r, q, n, m, dw, sw);
            }
        }
    }
    b->work_key = key;
}

// the end of the launch that starts at work[lo]: as many pairs as fit the workspace cap (always at least one)
static size_t next_launch(const std::vector<Work> &work, size_t lo, uint64_t cap_bytes, uint64_t &words) {
    words = 0;
    size_t hi = lo;
    while (hi < work.size() && (hi == lo || (words + work[hi].dir_words) * 4 <= cap_bytes)) {
        words += work[hi].dir_words;
        hi++;
    }
    return hi;
}

// pairs with more tied cells than cell_cap (`ovf`: their positions in `work`): run them again on the GPU with exact-size lists
static int rerun_overflowed(RunState &rs, const std::vector<Work> &work, const std::vector<size_t> &ovf, std::vector<PairOut> &outs) {
    swmi_batch *b = rs.b;
    int rc;
    if ((rc = settle_raw(b))) return rc;             // (the re-run writes the pinned block again)
    std::vector<Work> w2;
    std::vector<uint64_t> exact;
    for (size_t pos : ovf) { w2.push_back(work[pos]); exact.push_back(b->pairs[work[pos].pair].n_cells); }
    for (size_t lo = 0, hi; lo < w2.size(); lo = hi) {
        uint64_t words;
        hi = next_launch(w2, lo, rs.ctx->max_workspace_bytes, words);
        if ((rc = run_chunk(rs, w2, lo, hi, &exact, outs))) return rc;
        swmi_batch::RawChunk &rc2 = b->raw_chunks.back();                              // (the launch's records, just appended)
        rc2.wpos.resize(hi - lo);
        for (size_t k = 0; k < hi - lo; k++) rc2.wpos[k] = (uint32_t)ovf[lo + k];      // chunk-local id -> position in `work`
        for (size_t k = 0; k < hi - lo; k++) b->pairs[w2[lo + k].pair].n_cells = outs[k].n_cells;
        // (option "xdrop": the same kernel on the same inputs stops at the same strip)
        for (size_t k = 0; k < hi - lo; k++)
            if (b->pairs[w2[lo + k].pair].strips != outs[k].flags >> SWMI_F_STRIPS_SHIFT)
                return fail(SWMI_ERR_HIP, "the exact-size re-run swept another number of strips");
        for (size_t k = 0; k < hi - lo; k++)
            if (outs[k].flags & SWMI_F_CELL_OVF)
                return fail(SWMI_ERR_HIP, "cell list overflowed again on the exact-size re-run");
    }
    b->timing.rerun_pairs = (uint32_t)ovf.size();
    return SWMI_OK;
}

// opt: the context's run options when the run was asked for (run_options)
static int batch_run(swmi_ctx *ctx, swmi_batch *b, const swmi_params *p, RunOptions opt) {
    if (!ctx || !b || !p) return fail(SWMI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    // (a score matrix and the end-to-end modes run on the affine kernels only)
    // (... and so do a band, a CIGAR payload and the second-best score)
    const bool affine = ctx->affine == 1 || ctx->gap_open != 0 || opt.mat != nullptr || opt.modes.align_mode != SWMI_ALIGN_LOCAL || opt.modes.band > 0 ||
                        opt.modes.cigar != 0 || opt.modes.subopt != 0 || opt.prof != nullptr;      // (... and the batch's profiles)
    int rc;
    if ((rc = check_run_params(ctx, b, p, affine, opt))) return rc;
    static const bool host_dbg = getenv("SWMI_DEBUG_HOST") != nullptr;
    const auto h0 = Clock::now();
    {   // (hipSetDevice costs microseconds even when nothing changes; a sub-millisecond batch notices)
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != ctx->device) HIP_TRY(hipSetDevice(ctx->device));
    }
    b->params = *p;
    b->has_run = false;
    b->scores_only = ctx->scores_only != 0;

    const uint32_t n_refs = b->paired ? 0u : b->n_refs;     // (the references MapRef views exist for: none of a pair list)
    b->pairs.assign(batch_n_pairs(b), PairRes{});
    b->win_tab.clear(); b->win_at.clear();
    b->has_sub = opt.modes.subopt != 0;
    b->sub.assign(b->has_sub ? batch_n_pairs(b) : 0, SuboptOut{0, 0u});     // (a pair with an empty side is never swept: (0, 0))
    b->hits_k = b->has_sub ? opt.modes.hits : 0;
    b->hitv.assign(b->hits_k ? batch_n_pairs(b) * (size_t)(1 + b->hits_k) : 0, HitEnt{0, 0u, 0u, 0u});      // (... 0 entries)
    b->has_endb = opt.modes.end_bonus != 0;
    b->endv.assign(b->has_endb ? batch_n_pairs(b) : 0, EndOut{0, 0, 0u});   // (... (0, 0, 0))
    b->alns.clear(); b->str_at.clear();
    b->raw.clear(); b->rtab.clear(); b->raw_chunks.clear(); b->indexed = false;
    b->raw_ext = nullptr; b->rtab_ext = nullptr;
    if (b->views_built || b->ref_view_ready.size() != n_refs) {     // (a run nobody read MapRef views of leaves them as they are)
        b->ref_view_ready.assign(n_refs, 0);
        b->ref_sites.assign(n_refs, {});
        b->ref_degenerate.assign(n_refs, 0);
        b->views_built = false;
    }
    b->timing = swmi_timing{};

    // mode 1 needs pad rows that cannot outgrow the real cells they derive from: mismatch <= 0 and gap <= 0
    b->eff_mode = (ctx->mode == 1 && (p->mismatch > 0 || p->gap > 0)) ? 2u : ctx->mode;
    b->gap_open = ctx->gap_open;
    if (affine) b->eff_mode = 3;                         // the affine kernels (swmi_affine.hip): no other pipeline option applies
    b->opt = std::move(opt);
    if (b->opt.mat && b->d_mat_gen != b->opt.mat->gen) {
        // the run's own device copy, on its stream, complete before the run goes on: whatever an earlier (failed) run left on
        // the stream is done with d_mat, and the pageable host image is read before anything can release it.  Only when the
        // matrix changes: a batch re-run under the same matrix copies nothing.
        if ((rc = b->d_mat.reserve((size_t)swmi_aff_mat_words(SWMI_MAT_NN_MAX) * 4))) return rc;
        b->d_mat_gen = 0;
        HIP_TRY(hipMemcpyAsync(b->d_mat.p, b->opt.mat->image.data(), b->opt.mat->image.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        b->d_mat_gen = b->opt.mat->gen;
    }
    if (b->opt.prof && b->d_prof_gen != b->opt.prof->gen) {
        // the batch's profiles, likewise: the run's own device copy, complete before the run goes on, only when they changed
        if ((rc = b->d_prof.reserve(b->opt.prof->image.size() * 4))) return rc;
        b->d_prof_gen = 0;
        HIP_TRY(hipMemcpyAsync(b->d_prof.p, b->opt.prof->image.data(), b->opt.prof->image.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        b->d_prof_gen = b->opt.prof->gen;
    }
    if ((rc = choose_traceback_grain(ctx, b, p))) return rc;
    if (b->eff_mode == 0) {
        // mode 0's 256-step direction tiles leave the least LDS for the staged alignment: batches with pairs too long for
        // it run as mode 1 (or 2) -- the results are the same
        uint64_t max_m, max_n;
        longest_sequences(b, max_m, max_n);
        if (traceback_lds_bytes(0, path_bound(max_n, max_m, *p, p->match), max_m) > SWMI_LDS_BYTES)
            b->eff_mode = (p->mismatch > 0 || p->gap > 0) ? 2u : 1u;
    }
    build_schedule(ctx, b);
    const std::vector<Work> &work = b->work;
    const auto h1 = Clock::now();
    RunState rs;
    rs.ctx = ctx; rs.b = b;
    rs.tb_split = b->eff_mode == 1 &&
                  (ctx->tb_split == 1 || (ctx->tb_split < 0 && (work.size() < 64 || (work.size() <= 256 && b->auto_choice == 0 &&
                                                                                      memcmp(&b->auto_params, p, sizeof(swmi_params)) == 0))));
    b->tb_split_used = rs.tb_split;

    std::vector<PairOut> outs;
    std::vector<size_t> ovf;                         // positions in `work` that overflowed their cell list
    uint64_t dir_bytes = 0;
    for (size_t lo = 0, hi; lo < work.size(); lo = hi) {
        uint64_t words;
        hi = next_launch(work, lo, ctx->max_workspace_bytes, words);
        dir_bytes += words * 4;
        rs.defer_copy = lo == 0 && hi == work.size();
        rc = run_chunk(rs, work, lo, hi, nullptr, outs);
        rs.defer_copy = false;
        if (rc) return rc;
        for (size_t k = 0; k < hi - lo; k++) {
            PairRes &pr = b->pairs[work[lo + k].pair];
            pr.score = outs[k].score;
            pr.flags = ((outs[k].flags & SWMI_F_DEGENERATE) ? SWMI_PAIR_DEGENERATE : 0u) | ((outs[k].flags & SWMI_F_TO_END) ? SWMI_PAIR_TO_END : 0u);
            pr.n_cells = outs[k].n_cells;
            pr.strips = outs[k].flags >> SWMI_F_STRIPS_SHIFT;
            if (outs[k].flags & SWMI_F_CELL_OVF) ovf.push_back(lo + k);
        }
    }
    const auto h2 = Clock::now();
    if (!ovf.empty() && (rc = rerun_overflowed(rs, work, ovf, outs))) return rc;

    b->timing.fill_ms = rs.fill_ms; b->timing.traceback_ms = rs.tb_ms; b->timing.d2h_ms = rs.d2h_ms;
    b->timing.total_ms = rs.fill_ms + rs.tb_ms + rs.d2h_ms;
    b->timing.fill_launches = rs.launches;
    b->timing.cells = b->work_cells;
    b->timing.dir_bytes = dir_bytes;
    b->has_run = true;
    if (host_dbg)
        fprintf(stderr, "[swmi host] setup %.1f us, chunks (launch+wait+parse) %.1f us [prepare %.1f, its uploads %.1f, enqueue %.1f, wait %.1f, copy-out %.1f], grouping %.1f us\n",
                us_between(h0, h1), us_between(h1, h2), rs.prep_us, rs.prep_upload_us, rs.enqueue_us, rs.wait_us, rs.copyout_us, us_between(h2, Clock::now()));
    return SWMI_OK;
}

extern "C" int swmi_batch_run(swmi_ctx *ctx, swmi_batch *b, const swmi_params *p) {
    if (!ctx || !b || !p) return fail(SWMI_ERR_INVALID, "null argument");
    return batch_run(ctx, b, p, run_options(ctx, b));
}

// ---- asynchronous run: the same swmi_batch_run on the context's own host thread -------------------------------
// The caller gets its thread back while the GPU works (a Spark task can prepare its next partition, bench.py's rank
// can do the previous step's reduce).  The helper thread spins briefly between jobs, so back-to-back runs start
// without a wake-up latency, and sleeps when the context stays idle.
static void swmi_worker_loop(swmi_ctx *ctx) {
    for (;;) {
        int st = 0;
        for (int spin = 0; spin < 4000 && (st = ctx->job_state.load(std::memory_order_acquire)) != 1 && st != 3; ++spin)
            __builtin_ia32_pause();                  // back-to-back runs start without a wake-up; an idle context blocks
        if (st != 1 && st != 3) {
            std::unique_lock<std::mutex> lk(ctx->job_mu);
            ctx->job_cv.wait(lk, [&] { const int v = ctx->job_state.load(); return v == 1 || v == 3; });
            st = ctx->job_state.load();
        }
        if (st == 3) return;
        if (ctx->job_delay_us) std::this_thread::sleep_for(std::chrono::microseconds(ctx->job_delay_us));
        const int rc = batch_run(ctx, ctx->job_batch, &ctx->job_params, std::move(ctx->job_opt));
        ctx->job_rc = rc;
        ctx->job_err = rc ? swmi_last_error() : "";
        { std::lock_guard<std::mutex> lk(ctx->job_mu); ctx->job_state.store(2, std::memory_order_release); }
        ctx->job_cv.notify_all();
    }
}

extern "C" int swmi_batch_run_async(swmi_ctx *ctx, swmi_batch *b, const swmi_params *p) {
    if (!ctx || !b || !p) return fail(SWMI_ERR_INVALID, "null argument");
    if (ctx->job_state.load(std::memory_order_acquire) != 0)
        return fail(SWMI_ERR_INVALID, "a run is already in flight on this context: call swmi_batch_wait first");
    if (!ctx->worker.joinable()) ctx->worker = std::thread(swmi_worker_loop, ctx);
    ctx->job_batch = b;
    ctx->job_params = *p;
    ctx->job_opt = run_options(ctx, b);                 // (what is set now, whatever is set while the run is in flight)
    ctx->job_delay_us = ctx->dbg_async_delay_us;
    { std::lock_guard<std::mutex> lk(ctx->job_mu); ctx->job_state.store(1, std::memory_order_release); }
    ctx->job_cv.notify_all();
    return SWMI_OK;
}

extern "C" int swmi_batch_wait(swmi_ctx *ctx) {
    if (!ctx) return fail(SWMI_ERR_INVALID, "null argument");
    int st = ctx->job_state.load(std::memory_order_acquire);
    if (st == 0) return fail(SWMI_ERR_INVALID, "no run in flight on this context");
    for (int spin = 0; spin < 20000 && st != 2; ++spin) {           // a short bounded spin, then block
        __builtin_ia32_pause();
        st = ctx->job_state.load(std::memory_order_acquire);
    }
    if (st != 2) {
        std::unique_lock<std::mutex> lk(ctx->job_mu);
        ctx->job_cv.wait(lk, [&] { return ctx->job_state.load() == 2; });
    }
    const int rc = ctx->job_rc;
    const std::string err = ctx->job_err;
    ctx->job_state.store(0, std::memory_order_release);
    if (rc) return fail(rc, "%s", err.c_str());
    return SWMI_OK;
}

extern "C" int swmi_batch_mode(const swmi_batch *b, int *mode) {
    if (!b || !mode) return fail(SWMI_ERR_INVALID, "null argument");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    *mode = (int)b->eff_mode;
    return SWMI_OK;
}

extern "C" int swmi_batch_timing(const swmi_batch *b, swmi_timing *t) {
    if (!b || !t) return fail(SWMI_ERR_INVALID, "null argument");
    *t = b->timing;
    return SWMI_OK;
}

extern "C" int swmi_align_batch(swmi_ctx *ctx, const swmi_params *p,
                                const uint8_t *ref_bytes, const uint64_t *ref_off, uint32_t n_refs,
                                const uint8_t *read_bytes, const uint64_t *read_off, uint32_t n_reads,
                                swmi_batch **out) {
    int rc = swmi_batch_upload(ctx, ref_bytes, ref_off, n_refs, read_bytes, read_off, n_reads, out);
    if (rc) return rc;
    rc = swmi_batch_run(ctx, *out, p);
    if (rc) { swmi_batch_free(ctx, *out); *out = nullptr; }
    return rc;
}
