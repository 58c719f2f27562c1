// swmi_plan.h -- the plan of a chunk: which kernel takes each pair, the item lists of those kernels, the workspace offsets
// and the sizes a launch is dimensioned by (internal).  Host arithmetic (plan_chunk) and its uploads (upload_plan), cached
// in the batch by PlanKey (prepare_chunk).  Included by swmi_run.cpp ONLY: the planner is on the per-step path of a
// repeated run, which stays in one translation unit.
#pragma once
#include <chrono>
#include <cstdlib>

#include "swmi_host.h"

using Clock = std::chrono::steady_clock;
static inline double us_between(Clock::time_point a, Clock::time_point c) { return std::chrono::duration<double, std::micro>(c - a).count(); }

// longest possible traceback of an n x m pair: A + I <= m rows, A + D <= n columns, and -- with match > 0 > gap -- the
// score match*A + gap*(I + D) must stay positive (`while (score > 0)`), which caps the gap moves.  smax: the largest score of
// one alignment move (match; with a score matrix the larger of match and its largest entry)
// align_mode != 0: the score may be anything, so only A + I <= m and A + D <= n hold: m + n moves
static uint64_t path_bound(uint64_t n_, uint64_t m_, const swmi_params &p, int32_t smax, int align_mode = 0) {
    uint64_t path = n_ + m_;
    if (align_mode != 0) return path;
    if (smax > 0 && p.gap < 0 && p.mismatch <= smax) {
        const uint64_t g = (uint64_t)(-(int64_t)p.gap), mt = (uint64_t)smax;
        path = std::min(path, std::min(m_ + std::min(n_, mt * m_ / g), n_ + std::min(m_, mt * n_ / g)));
    }
    return path;
}

// bytes of LDS a traceback workgroup needs for pairs whose longest path / read are given (swmi_walk.h: SWMI_TB_WAVES = 8)
static uint64_t traceback_lds_bytes(uint32_t mode, uint64_t max_path, uint64_t max_read) {
    const uint64_t lds_words = (max_path + 3) / 4 + 1, lds_read_words = (max_read + 3) / 4 + 1;
    const uint64_t win = (uint64_t)SWMI_RMAX * 64;
    const uint64_t tile_words = mode == 0 ? 4ull * SWMI_TB_BLOCKS * win : (mode == 1 ? 32 + 8ull * SWMI_CK_BLOCKS * win : 4ull * SWMI_CK_BLOCKS * win);
    return 4ull * (tile_words + 4ull * (lds_words + lds_read_words + SWMI_TB_REFWIN_WORDS));
}

static void longest_sequences(const swmi_batch *b, uint64_t &max_m, uint64_t &max_n) {
    max_m = max_n = 0;
    for (const auto &d : b->read_desc) max_m = std::max<uint64_t>(max_m, d.len);
    for (const auto &d : b->ref_desc) max_n = std::max<uint64_t>(max_n, d.len);
}

// ------------------------------------------------------------------------------------------
// the plan of a chunk
// ------------------------------------------------------------------------------------------
// What a launch of work[lo, hi) needs besides the sequences: pair descriptors with their workspace offsets, the item lists of
// the kernels that take only some of the pairs (strips of long reads, column chunks, resident pairs, transposed pairs), the
// window offsets of the split traceback, and the sizes everything downstream is dimensioned by (ChunkPlan).  plan_chunk
// derives them on the host, upload_plan puts the arrays on the device; prepare_chunk skips both when the batch still holds
// the plan of the same PlanKey.

namespace {

struct PlanItems {                           // the arrays of a plan
    std::vector<PairDesc> pd;
    std::vector<StripItem> strip_items;
    std::vector<ColItem> col_items;
    std::vector<uint32_t> win_off;           // split traceback: first window of every pair
    std::vector<uint32_t> res_items, tf_items;
};

static const uint32_t CK_STEP_W = 16u * SWMI_CK_BLOCKS;     // anti-diagonal steps (= columns of lane 0) per checkpoint window
static inline uint32_t ck_windows(uint32_t n) {             // checkpoint windows of a sweep over n columns
    const uint64_t wblocks = ((uint64_t)n + 63u + 15u) / 16u;
    return (uint32_t)((wblocks + SWMI_CK_BLOCKS - 1u) / SWMI_CK_BLOCKS);
}
// columns a positive-score path can span: A <= m alignment moves, and match*A + gap*D > 0 bounds the deletions D
static inline uint64_t path_span(uint32_t m, const swmi_params &P) {
    return (uint64_t)m + (uint64_t)(P.match > 0 ? P.match : 0) * m / (uint64_t)(P.gap < 0 ? -(int64_t)P.gap : 1) + 1;
}

// One column chunk of a pair's sweep: the checkpoint windows [g_lo, g_hi) it owns, and the column it starts at -- far enough
// to the left of g_lo for every cell from there on to be exact, on a window boundary so that the checkpoints stay aligned.
// A chunk that is not the last must end where lane 0 is still inside the reference: one that would not takes the rest.
struct ColChunk { uint32_t g_lo, g_hi, col0; };
static ColChunk col_chunk(uint32_t g_lo, uint32_t wpc, uint32_t n_ck, uint32_t n, uint64_t span) {
    ColChunk c;
    c.g_lo = g_lo;
    c.g_hi = std::min(g_lo + wpc, n_ck);
    if (c.g_hi < n_ck && (uint64_t)c.g_hi * CK_STEP_W > n) c.g_hi = n_ck;
    const int64_t c0 = (int64_t)g_lo * CK_STEP_W - 64 - (int64_t)span - 1;
    c.col0 = g_lo == 0 || c0 <= 0 ? 0u : (uint32_t)(c0 / CK_STEP_W * CK_STEP_W);
    return c;
}

struct Planner {
    const swmi_ctx *ctx;
    const swmi_batch *b;
    const swmi_params &P;
    size_t np;
    ChunkPlan &plan;
    PlanItems &it;
    // Column chunks (swmi_device.h: ColItem): a launch of few pairs leaves most of the 1024 SIMDs idle while every pair is
    // one dependent chain of n + 63 steps.  A positive-score path spans at most path_span() columns, so a wavefront that
    // starts that far to the left of a window computes the window exactly: the reference is cut into chunks of windows,
    // one wavefront each.
    bool cols_possible = false;
    uint64_t chunk_budget = 1;
    // Resident pairs (sw_resident_pairs_kernel): a pair whose whole direction field fits a wavefront's share of LDS -- and
    // whose reference is short next to its read, so that the alignments cover most of the matrix anyway -- skips checkpoints
    // and window re-sweeps altogether: one wavefront sweeps it twice inside LDS and walks ALL its alignments at once, one per
    // lane.  (The exact-size re-run of pairs with more tied maxima than an LDS list holds takes the ordinary path.)
    // (measured, profiles/r02/sweeps_*.md: below ~300 pairs the launch is latency-bound and the split traceback, which
    // spreads a pair's windows and alignments over many wavefronts, is faster)
    bool res_possible = false, res_maybe = false;
    // Transposed, fused pairs (swmi_tfused.hip): reference columns on the lanes, the read streaming through, sweep AND
    // traceback in one launch -- for the usual pair (fast symbols, int4 scores, gap < 0, read <= 256, reference <= 2560).
    // Its sweep needs 20 % fewer instructions, but its traceback (one wavefront per block of a pair) does not beat the
    // workgroup-per-pair kernel: measured 0.170 ms against 0.088 + 0.071 at the headline, and slower for big batches (LDS and
    // registers hold it to one or two wavefronts per SIMD).  Kept as an option, tested in every GPU parity test; not chosen.
    bool tf_possible = false;

    Planner(const swmi_ctx *ctx_, const swmi_batch *b_, size_t np_, bool exact, ChunkPlan &plan_, PlanItems &it_)
        : ctx(ctx_), b(b_), P(b_->params), np(np_), plan(plan_), it(it_) {
        const bool mode1 = b->eff_mode == 1, whole = mode1 && !exact && !ctx->scores_only;
        cols_possible = mode1 && P.match > 0 && P.gap < 0 && P.mismatch <= 0 && P.match <= 7 && P.mismatch >= -8 &&
                        (np <= 512 || ctx->col_chunks > 1) && ctx->col_chunks != 1;
        chunk_budget = ctx->col_chunks > 1 ? ctx->col_chunks : std::max<uint64_t>(1, 1024 / std::max<size_t>(np, 1));
        res_possible = whole && ctx->resident != 0 && (ctx->resident == 1 || np >= 256) &&
                       P.match <= 7 && P.match >= -8 && P.mismatch >= -8 && P.mismatch <= 0 && P.gap <= 0;
        tf_possible = whole && ctx->tfused == 1 &&      // (-1, automatic: not chosen -- DESIGN.md 4.4)
                      P.match > 0 && P.match <= 7 && P.mismatch >= -8 && P.mismatch <= P.match && P.gap < 0 && P.gap >= -64;
    }
    bool fast_symbols(const PairDesc &d) const { return b->read_desc[d.read_id].acgt && b->ref_desc[d.ref_id].acgt; }

    // LDS dwords of a resident pair's wavefront; opw: the dwords of packed ops a lane stages
    uint64_t res_need_words(uint32_t m, uint32_t n, uint32_t &opw) const {
        const uint32_t R_ = swmi_rows_per_lane(m), lact = (m + R_ - 1) / R_;
        const uint64_t nblk = ((uint64_t)n + lact - 1 + 15) / 16, n_ck = (nblk + SWMI_CK_BLOCKS - 1) / SWMI_CK_BLOCKS;
        opw = (uint32_t)((path_bound(n, m, P, P.match) + 15) / 16 + 1);
        return nblk * R_ * 64 + ((n_ck + 1) & ~1ull) + 2ull * SWMI_RES_CELL_CAP + 64ull * opw + (n + 3) / 4 + 1 + (m + 3) / 4 + 1 + 8 +
               SWMI_EMIT_SCRATCH_WORDS;
    }
    // a resident pair by its lengths alone (the symbols are checked by fast_symbols, once they are known)
    bool res_size_fits(uint32_t m, uint32_t n) const {
        uint32_t opw;
        return m <= 64u * SWMI_RMAX && (ctx->resident == 1 || (uint64_t)n <= 8ull * m) &&
               res_need_words(m, n, opw) * 4 <= (ctx->resident == 1 ? 40u : 20u) * 1024u;
    }
    bool tf_fits(const PairDesc &d, const Work &w, uint32_t m, uint32_t n) const {
        return tf_possible && m <= SWMI_TF_MAX_M && n <= 64u * SWMI_TF_BMAX && fast_symbols(d) && w.dir_words >= swmi_tf_ck_words(m);
    }
    bool cols_fit(const PairDesc &d, uint32_t m) const {
        return cols_possible && chunk_budget > 1 && m <= 64u * SWMI_RMAX && fast_symbols(d);
    }

    void take_tfused(size_t k, PairDesc &d, uint32_t m, uint32_t n) {
        d.pad = SWMI_PAD_RESIDENT;                  // (every other kernel skips the pair)
        it.tf_items.push_back((uint32_t)k);
        plan.tf_max_m = std::max(plan.tf_max_m, m); plan.tf_max_n = std::max(plan.tf_max_n, n);
        plan.tf_max_path = std::max<uint32_t>(plan.tf_max_path, (uint32_t)path_bound(n, m, P, P.match));
    }
    void take_resident(size_t k, PairDesc &d, uint32_t m, uint32_t n) {
        d.pad = SWMI_PAD_RESIDENT;
        it.res_items.push_back((uint32_t)k);
        uint32_t opw;
        (void)res_need_words(m, n, opw);
        plan.res_ops_words = std::max(plan.res_ops_words, opw);
    }
    // a read longer than one strip: one wavefront per strip, pipelined through the seam rows
    void take_strips(size_t k, PairDesc &d, uint32_t m, uint32_t n) {
        const uint32_t strips = (m + 64u * SWMI_RMAX - 1u) / (64u * SWMI_RMAX);
        d.pad = (uint32_t)it.strip_items.size();
        auto push_strips = [&](StripItem si) {
            si.pair = (uint32_t)k;
            si.prog = (uint32_t)it.strip_items.size();
            si.pad = 0;
            if (ctx->dbg_reverse_strips) for (uint32_t st = strips; st-- > 0;) { si.strip = st; it.strip_items.push_back(si); }
            else                         for (uint32_t st = 0; st < strips; st++) { si.strip = st; it.strip_items.push_back(si); }
        };
        // Column chunks of a multi-strip pair (swmi_device.h: StripItem): the halo argument holds for the whole read, so
        // a chunk is a strip pipeline of its own over [col0, end of its windows], all strips starting from zero.  The
        // halo is long (2.25 m columns at the default scores): a chunk's body may be as short as a quarter of it -- the
        // launch has SIMDs to spare, and what counts is the length of the longest chain.
        uint64_t chunks = 1;
        const uint32_t n_ck = ck_windows(n);
        const uint64_t span = path_span(m, P);
        if (cols_possible) {                                   // (any symbols: the strip kernel has both cell streams)
            const uint64_t budget = ctx->col_chunks > 1 ? ctx->col_chunks : chunk_budget / strips;
            chunks = std::min<uint64_t>(budget, n / std::max<uint64_t>((span + 64) / 4, 256));
            chunks = std::min<uint64_t>(chunks, n_ck);
            if (chunks < 2) chunks = 1;
        }
        if (chunks == 1) {
            StripItem si{};
            si.col0 = 0; si.g_lo = 0; si.g_hi = 0xFFFFFFFFu; si.priv_stride = 0; si.priv_off = 0;
            push_strips(si);
            return;
        }
        const uint32_t wpc = (uint32_t)((n_ck + chunks - 1) / chunks);   // windows per chunk
        for (uint32_t g_lo = 0; g_lo < n_ck; g_lo += wpc) {
            const ColChunk c = col_chunk(g_lo, wpc, n_ck, n, span);
            StripItem si{};
            si.g_lo = c.g_lo; si.g_hi = c.g_hi; si.col0 = c.col0;
            // strip 0 runs furthest: 64 steps per strip below it past the chunk's last window, or to the reference's end
            const uint64_t ext0 = (uint64_t)c.g_hi * CK_STEP_W - c.col0 + 64ull * (strips - 1u);
            const uint64_t n0 = c.g_hi < n_ck ? std::min<uint64_t>(n - c.col0, ext0) : n - c.col0;
            si.priv_stride = (uint32_t)((n0 + 1 + 15) & ~15ull);
            si.priv_off = plan.seam_priv_words;                             // (+ the shared rows of the launch: finish())
            plan.seam_priv_words += (uint64_t)(strips - 1u) * si.priv_stride;
            if (c.g_hi == n_ck) si.g_hi = 0xFFFFFFFFu;                      // (the pair's last chunk: every window from g_lo on)
            push_strips(si);
            plan.n_strip_chunks++;
            if (c.g_hi == n_ck) break;
        }
    }
    // column chunks of a single-strip pair
    void take_cols(size_t k, PairDesc &d, uint32_t m, uint32_t n) {
        const uint64_t span = path_span(m, P);
        const uint32_t n_ck = ck_windows(n);
        uint64_t chunks = std::min<uint64_t>(chunk_budget, n / std::max<uint64_t>(span + 64, 256));
        chunks = std::min<uint64_t>(chunks, n_ck);
        static const bool dbg_one = getenv("SWMI_DEBUG_ONE_CHUNK") != nullptr;      // diagnostics: every pair through the chunk kernel, one chunk
        if (dbg_one) chunks = 1;
        if (chunks < 2 && !dbg_one) return;
        const uint32_t wpc = (uint32_t)((n_ck + chunks - 1) / chunks);   // windows per chunk
        const size_t first = it.col_items.size();
        for (uint32_t g_lo = 0; g_lo < n_ck; g_lo += wpc) {
            const ColChunk c = col_chunk(g_lo, wpc, n_ck, n, span);
            ColItem ci;
            ci.pair = (uint32_t)k; ci.g_lo = c.g_lo; ci.g_hi = c.g_hi; ci.col0 = c.col0;
            it.col_items.push_back(ci);
            if (c.g_hi == n_ck) break;
        }
        d.pad = SWMI_PAD_COLS | (uint32_t)(it.col_items.size() - first);
    }

    // once every pair's kernel is known: the resident pairs' common LDS share, and the workspace offsets
    void finish(const std::vector<Work> &work, size_t lo) {
        // the kernel lays every wavefront's LDS out with the launch-wide ops_words: size the share for that
        for (uint32_t k : it.res_items) {
            uint32_t opw;
            const uint64_t own = res_need_words(b->read_desc[it.pd[k].read_id].len, b->ref_desc[it.pd[k].ref_id].len, opw);
            plan.res_lds_words = std::max<uint32_t>(plan.res_lds_words, (uint32_t)(own + 64ull * (plan.res_ops_words - opw)));
        }
        if (16ull * plan.res_lds_words > SWMI_LDS_BYTES) {    // four such shares do not fit a CU's LDS: the ordinary path for all of them
            for (uint32_t k : it.res_items) it.pd[k].pad = 0;
            it.res_items.clear();
            plan.res_lds_words = 0; plan.res_ops_words = 0;
        }
        plan.n_strip_items = it.strip_items.size();
        plan.n_col_items = it.col_items.size();
        plan.n_res = it.res_items.size();
        plan.n_tf = it.tf_items.size();
        // a resident pair keeps everything in LDS and gets no workspace
        // (40,000 pairs of 80 x 400 were charged 0.6 GB of checkpoints nobody writes)
        std::vector<uint8_t> is_res(np, 0);
        for (uint32_t k : it.res_items) is_res[k] = 1;
        for (size_t k = 0; k < np; k++) {
            it.pd[k].dir_off = plan.dir_words;
            it.pd[k].seam_off = plan.seam_words;
            if (!is_res[k]) { plan.dir_words += work[lo + k].dir_words; plan.seam_words += work[lo + k].seam_words; }
        }
        if (b->eff_mode == 1) it.win_off[np] = (uint32_t)std::min<uint64_t>(plan.n_windows, 0xFFFFFFFFu);
        for (StripItem &si : it.strip_items)
            if (si.priv_stride) si.priv_off += plan.seam_words;
    }
};

}  // namespace

// host arithmetic: fills `plan` in place and the arrays of `it`
static int plan_chunk(swmi_ctx *ctx, swmi_batch *b, const std::vector<Work> &work, size_t lo, size_t np, bool exact, ChunkPlan &plan,
                      PlanItems &it) {
    plan = ChunkPlan{};
    Planner pl(ctx, b, np, exact, plan, it);
    if (pl.res_possible)
        for (size_t k = 0; k < np && !pl.res_maybe; k++)
            pl.res_maybe = pl.res_size_fits(b->read_desc[pair_read(b, work[lo + k].pair)].len, b->ref_desc[pair_ref(b, work[lo + k].pair)].len);
    if ((pl.cols_possible || pl.res_maybe || pl.tf_possible) && !b->acgt_known) {
        // the fast-symbol flags are derived on the device by the encode kernel
        if (b->n_refs) HIP_TRY(hipMemcpy(b->ref_desc.data(), b->d_refs.p, b->n_refs * sizeof(SeqDesc), hipMemcpyDeviceToHost));
        if (b->n_reads) HIP_TRY(hipMemcpy(b->read_desc.data(), b->d_reads.p, b->n_reads * sizeof(SeqDesc), hipMemcpyDeviceToHost));
        b->acgt_known = true;
    }
    it.pd.resize(np);
    if (b->eff_mode == 1) it.win_off.resize(np + 1);
    uint32_t pb_m = 0xFFFFFFFFu, pb_n = 0xFFFFFFFFu, pb_val = 0;
    // (a score matrix entry above match lets a positive path run longer: the bound takes the largest score of one move)
    // (the batch's profiles likewise: their largest entry)
    const int32_t smax = b->opt.mat ? std::max(b->params.match, b->opt.mat->max_entry)
                       : b->opt.prof ? std::max(b->params.match, b->opt.prof->max_entry) : b->params.match;
    for (size_t k = 0; k < np; k++) {
        const Work &w = work[lo + k];
        PairDesc d{};
        d.ref_id = pair_ref(b, w.pair);
        d.read_id = pair_read(b, w.pair);
        d.out_id = (uint32_t)k;
        const uint32_t m_ = b->read_desc[d.read_id].len, n_ = b->ref_desc[d.ref_id].len;
        if (b->eff_mode == 1) {
            const uint64_t rps = 64ull * swmi_rows_per_lane(m_);
            it.win_off[k] = (uint32_t)std::min<uint64_t>(plan.n_windows, 0xFFFFFFFFu);
            plan.n_windows += ((m_ + rps - 1) / rps) * ck_windows(n_);
        }
        const bool res_fit = pl.res_maybe && pl.fast_symbols(d) && pl.res_size_fits(m_, n_);
        if (!res_fit && pl.tf_fits(d, w, m_, n_)) pl.take_tfused(k, d, m_, n_);
        else if (res_fit) pl.take_resident(k, d, m_, n_);
        else if (b->eff_mode == 1 && m_ > 64u * SWMI_RMAX && it.strip_items.size() < (1u << 30)) pl.take_strips(k, d, m_, n_);
        else if (pl.cols_fit(d, m_)) pl.take_cols(k, d, m_, n_);
        it.pd[k] = d;
        if (m_ != pb_m || n_ != pb_n) { pb_m = m_; pb_n = n_; pb_val = (uint32_t)path_bound(n_, m_, b->params, smax, b->opt.modes.align_mode); }   // (runs of equal lengths)
        plan.max_path = std::max<uint32_t>(plan.max_path, pb_val);
        plan.max_read = std::max(plan.max_read, m_);
        if (m_ > SWMI_AFF_MAX_READ) { plan.aff_n_long++; continue; }      // (mode 3 with long_reads: the strip kernels' pair)
        plan.aff_r_min = std::min(plan.aff_r_min, swmi_aff_rows_per_lane(m_));
        plan.aff_r_max = std::max(plan.aff_r_max, swmi_aff_rows_per_lane(m_));
    }
    pl.finish(work, lo);
    if (b->eff_mode == 3 && plan.aff_n_long) {
        // the strip kernels' pairs go last (each keeps its out_id and its offsets): the sweeps and the tracebacks of the two
        // kinds are launched over their own part of the array
        std::stable_partition(it.pd.begin(), it.pd.end(), [&](const PairDesc &d) { return b->read_desc[d.read_id].len <= SWMI_AFF_MAX_READ; });
    }
    return SWMI_OK;
}

// one array of a plan onto the device (synchronised: the source is a local of the caller)
template <class T>
static int upload_items(hipStream_t st, DevBuf &dst, const std::vector<T> &v) {
    int rc;
    if ((rc = dst.reserve(v.size() * sizeof(T)))) return rc;
    HIP_TRY(hipMemcpyAsync(dst.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SWMI_OK;
}

static int upload_plan(swmi_ctx *ctx, swmi_batch *b, size_t np, const ChunkPlan &plan, const PlanItems &it) {
    int rc;
    if (b->eff_mode == 1 && (rc = upload_items(ctx->stream, b->d_win_off, it.win_off))) return rc;
    if ((rc = b->d_pairs.reserve(np * sizeof(PairDesc)))) return rc;
    if (!it.strip_items.empty()) {
        if ((rc = b->d_progress.reserve(it.strip_items.size() * sizeof(uint32_t)))) return rc;
        if ((rc = upload_items(ctx->stream, b->d_strip_items, it.strip_items))) return rc;
    }
    if (!it.res_items.empty() && (rc = upload_items(ctx->stream, b->d_res_items, it.res_items))) return rc;
    if (!it.tf_items.empty() && (rc = upload_items(ctx->stream, b->d_tf_items, it.tf_items))) return rc;
    if (!it.col_items.empty() && (rc = upload_items(ctx->stream, b->d_col_items, it.col_items))) return rc;
    if ((rc = b->d_dir.reserve(std::max<uint64_t>(plan.dir_words, 1) * 4))) return rc;
    if ((rc = b->d_seam.reserve(std::max<uint64_t>(plan.seam_words + plan.seam_priv_words, 1) * 4))) return rc;
    // repeated runs of one batch schedule the same pairs: skip the H2D copy when nothing changed
    const size_t bytes = np * sizeof(PairDesc);
    if (b->pairs_dev_ptr != b->d_pairs.p || b->pairs_on_device.size() != bytes || memcmp(b->pairs_on_device.data(), it.pd.data(), bytes) != 0) {
        HIP_TRY(hipMemcpyAsync(b->d_pairs.p, it.pd.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));      // pd is the caller's local: the copy must be done before it dies
        b->pairs_on_device.assign((const uint8_t *)it.pd.data(), (const uint8_t *)it.pd.data() + bytes);
        b->pairs_dev_ptr = b->d_pairs.p;
    }
    return SWMI_OK;
}

// b->plan and the device-side arrays for work[lo, hi): from the cache when the key is the one they were made for
static int prepare_chunk(RunState &rs, const std::vector<Work> &work, size_t lo, size_t hi, const std::vector<uint64_t> *cells_exact) {
    swmi_ctx *ctx = rs.ctx;
    swmi_batch *b = rs.b;
    const size_t np = hi - lo;
    const auto p0 = Clock::now();
    PlanKey key;
    key.valid = true;
    key.lo = lo; key.hi = hi; key.work = (const void *)work.data();
    key.params = b->params; key.eff_mode = b->eff_mode;
    key.col_chunks = ctx->col_chunks; key.reverse_strips = ctx->dbg_reverse_strips != 0;
    key.resident = ctx->resident; key.tfused = ctx->tfused;
    key.exact = cells_exact != nullptr; key.scores_only = ctx->scores_only != 0;
    key.mat_gen = b->opt.mat ? b->opt.mat->gen : 0u; key.modes = b->opt.modes;
    key.prof_gen = b->opt.prof ? b->opt.prof->gen : 0u;
    key.d_pairs = b->d_pairs.p; key.pairs_bytes = np * sizeof(PairDesc);
    auto p1 = p0;
    if (key == b->plan_key) {
        p1 = Clock::now();
    } else {
        b->plan_key = PlanKey{};                 // (no plan while this one is being made: an error below leaves none)
        PlanItems items;
        int rc;
        if ((rc = plan_chunk(ctx, b, work, lo, np, key.exact, b->plan, items))) return rc;
        p1 = Clock::now();
        if ((rc = upload_plan(ctx, b, np, b->plan, items))) return rc;
        key.d_pairs = b->pairs_dev_ptr;          // (= d_pairs.p, which the upload may have re-allocated)
        b->plan_key = key;
    }
    rs.prep_us += us_between(p0, p1);
    rs.prep_upload_us += us_between(p1, Clock::now());
    return SWMI_OK;
}
