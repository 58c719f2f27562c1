// swmi_results.cpp -- results of a run: the record stream the kernels left and its lazy index, the pair accessors, the
// host-built alignment strings, MapRef's views (Distribution.java:403-436).
#include <cstdio>
#include <cstdlib>

#include "swmi_host.h"

// the records left in the pinned block move into the batch's own vectors (before the block is written again)
int swmi_host::settle_raw(swmi_batch *b) {
    if (!b->raw_ext) return SWMI_OK;
    const uint32_t *aw = b->raw_ext;
    const AlnRec *tab = b->rtab_ext;
    b->raw_ext = nullptr; b->rtab_ext = nullptr;
    uint64_t used = 0;
    for (uint64_t k = 0; k < b->raw_ext_records; k++) {
        uint64_t end;
        if (!payload_end(b, tab[k], aw, b->raw_ext_cap, end)) return fail(SWMI_ERR_HIP, "record payloads overrun the arena");
        used = std::max(used, end);
    }
    b->raw.assign(aw, aw + used);
    b->rtab.assign(tab, tab + b->raw_ext_records);
    if (b->raw_chunks.size() == 1) { b->raw_chunks[0].at = 0; b->raw_chunks[0].words = (size_t)used; b->raw_chunks[0].tab_at = 0; }
    return SWMI_OK;
}

// Turns the record tables of the last run into per-pair alignment lists (first use of an alignment accessor).
static int ensure_indexed(swmi_batch *b) {
    if (b->indexed) return SWMI_OK;
    if (b->scores_only)
        return fail(SWMI_ERR_INVALID, "the batch was run with scores_only = 1: scores and totals only, no alignments");
    if (b->records_dropped)
        return fail(SWMI_ERR_INVALID, "this chunk's alignment records were not kept (option stream_keep_records = 0): scores, counts and totals only");
    const std::vector<Work> &work = b->work;
    // every launch's table (dense, read sequentially) with the arena its payload offsets refer to; the only launch of a
    // run may still sit in the pinned block the kernels wrote: indexed where it is, nothing copied
    struct Src { const AlnRec *tab; uint64_t n_rec; const uint32_t *arena; uint64_t words; const swmi_batch::RawChunk *c; };
    std::vector<Src> srcs;
    for (auto &c : b->raw_chunks) {
        if (b->raw_ext) srcs.push_back(Src{b->rtab_ext, b->raw_ext_records, b->raw_ext, b->raw_ext_cap, &c});
        else            srcs.push_back(Src{b->rtab.data() + c.tab_at, c.n_rec, b->raw.data() + c.at, c.words, &c});
    }
    auto wpos_of = [](const Src &sr, uint32_t out_id) -> uint64_t {
        return sr.c->wpos.empty() ? sr.c->lo + out_id : (out_id < sr.c->wpos.size() ? sr.c->wpos[out_id] : ~0ull);
    };
    for (auto &w : work) b->pairs[w.pair].count = 0;
    uint64_t total = 0;
    for (auto &sr : srcs) {
        for (uint64_t k = 0; k < sr.n_rec; k++) {
            const uint64_t wp = wpos_of(sr, sr.tab[k].out_id);
            if (wp >= work.size()) return fail(SWMI_ERR_HIP, "record of an unknown pair");
            b->pairs[work[wp].pair].count++;
        }
        total += sr.n_rec;
    }
    uint64_t run = 0;
    for (auto &w : work) { PairRes &pr = b->pairs[w.pair]; pr.first = run; run += pr.count; }
    if (run != total) return fail(SWMI_ERR_HIP, "record count mismatch");
    b->alns.assign(run, HostAln{});
    std::vector<uint32_t> cursor;
    const bool strict = b->params.tie_mode == SWMI_TIE_STRICT;
    for (auto &sr : srcs) {
        for (uint64_t k = 0; k < sr.n_rec; k++) {
            const AlnRec &e = sr.tab[k];
            const uint64_t wp = wpos_of(sr, e.out_id);
            PairRes &pr = b->pairs[work[wp].pair];
            const uint64_t off = ((uint64_t)e.off_hi << 32) | e.off_lo;
            uint64_t end;
            if (!payload_end(b, e, sr.arena, sr.words, end)) return fail(SWMI_ERR_HIP, "record payload overruns the arena");
            HostAln a;
            a.rank = e.rank; a.begin = e.begin; a.end_i = e.end_i; a.end_j = e.end_j; a.n_ops = e.n_ops;
            a.rec = sr.arena + off;
            // records of the split traceback come in any order: placed as they come, ordered by their cell below
            if (e.rank == SWMI_RANK_BY_CELL) {
                if (cursor.empty()) cursor.assign(work.size(), 0u);
                uint32_t &c = cursor[wp];
                if (c >= pr.count) return fail(SWMI_ERR_HIP, "more records than counted for a pair");
                b->alns[pr.first + c++] = a;
            } else {
                if (e.rank >= pr.count) return fail(SWMI_ERR_HIP, "record rank %u out of range", e.rank);
                b->alns[pr.first + e.rank] = a;
            }
        }
    }
    // ordered as OptAlignments lists them: by the rank the traceback kernel computed, or by cell: row-major
    // (SmithWaterman.java:157-185), or per anti-diagonal with ascending j for the strict mode (DistributedSW.java:209-239)
    for (size_t wi = 0; wi < work.size(); wi++) {
        PairRes &pr = b->pairs[work[wi].pair];
        if (!(pr.flags & SWMI_PAIR_DEGENERATE) && pr.count != pr.n_cells)
            return fail(SWMI_ERR_HIP, "pair %u: %llu records for %llu max cells", work[wi].pair,
                        (unsigned long long)pr.count, (unsigned long long)pr.n_cells);
        if (!cursor.empty() && cursor[wi] > 1) {
            auto key = [strict](const HostAln &x) {
                return strict ? (((uint64_t)((uint32_t)x.end_i + (uint32_t)x.end_j)) << 32) | (uint32_t)x.end_j
                              : ((uint64_t)(uint32_t)x.end_i << 32) | (uint32_t)x.end_j;
            };
            std::sort(b->alns.begin() + pr.first, b->alns.begin() + pr.first + pr.count,
                      [&](const HostAln &x, const HostAln &y) { return key(x) < key(y); });
        }
        if (!cursor.empty() && cursor[wi] != 0)
            for (uint64_t k = 0; k < pr.count; k++) b->alns[pr.first + k].rank = (uint32_t)k;
        // DistributedSW.GetAlignments sorts the collected alignments by beginning (DistributedSW.java:480)
        if (strict && pr.count > 1)
            std::stable_sort(b->alns.begin() + pr.first, b->alns.begin() + pr.first + pr.count,
                             [](const HostAln &x, const HostAln &y) { return x.begin < y.begin; });
    }
    if (!b->rec_strings) {
        // records without strings (option device_strings = 0): one buffer for all strings the host builds (two mallocs per
        // alignment cost more than filling them)
        b->str_at.resize(run);
        uint64_t chars = 0;
        for (uint64_t k = 0; k < run; k++) { b->alns[k].str_id = -1; b->str_at[k] = chars; chars += 2ull * (b->alns[k].n_ops + 1); }
        b->str_buf.resize(chars);
    }
    b->indexed = true;
    return SWMI_OK;
}

// ------------------------------------------------------------------------------------------
// result accessors
// ------------------------------------------------------------------------------------------
extern "C" uint64_t swmi_batch_n_pairs(const swmi_batch *b) { return b ? batch_n_pairs(b) : 0; }

static int check_pair(const swmi_batch *b, uint64_t pair) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (pair >= batch_n_pairs(b)) return fail(SWMI_ERR_RANGE, "pair %llu out of range", (unsigned long long)pair);
    return SWMI_OK;
}

extern "C" int swmi_pair_score(const swmi_batch *b, uint64_t pair, int32_t *score) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    if (score) *score = b->pairs[pair].score;
    return SWMI_OK;
}

extern "C" int swmi_pair_n_alignments(const swmi_batch *b, uint64_t pair, uint64_t *n, uint32_t *flags) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    if (b->scores_only && !(b->pairs[pair].flags & SWMI_PAIR_DEGENERATE))
        return fail(SWMI_ERR_INVALID, "the batch was run with scores_only = 1: the number of alignments was not computed");
    if (n) *n = b->pairs[pair].n_cells;
    if (flags) *flags = b->pairs[pair].flags;
    return SWMI_OK;
}

// the read rows a pair's sweep covered: the read's length, or 1024 * (strips swept) for a pair that option "xdrop" stopped
extern "C" int swmi_pair_rows_swept(const swmi_batch *b, uint64_t pair, uint32_t *rows) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    const PairRes &pr = b->pairs[pair];
    if (rows) *rows = pr.strips ? pr.strips * SWMI_AFF_MAX_READ : b->read_desc[pair_read(b, pair)].len;
    return SWMI_OK;
}

// the window of reference columns the pair's sweep used for strip `strip` of the read (swmi.h)
extern "C" int swmi_pair_band_window(const swmi_batch *b, uint64_t pair, uint32_t strip, uint32_t *c_lo, uint32_t *c_hi) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    const PairRes &pr = b->pairs[pair];
    const uint32_t m = b->read_desc[pair_read(b, pair)].len, n = b->ref_desc[pair_ref(b, pair)].len;
    const uint32_t ns = swmi_aff_strips(m), swept = pr.strips ? pr.strips : ns;
    if (strip >= ns) return fail(SWMI_ERR_RANGE, "strip %u: the read of pair %llu has %u strip%s", strip, (unsigned long long)pair, ns, ns == 1 ? "" : "s");
    if (strip >= swept) return fail(SWMI_ERR_RANGE, "strip %u of pair %llu was not swept: xdrop ended the sweep behind strip %u", strip,
                                    (unsigned long long)pair, swept - 1u);
    const RunModes &md = b->opt.modes;
    uint32_t lo = 1u, hi = n;
    if (b->eff_mode == 3 && md.band > 0 && m > SWMI_AFF_MAX_READ && n) {
        if (md.band_adapt) {
            if (pair >= b->win_at.size() || !b->win_at[pair]) return fail(SWMI_ERR_INVALID, "pair %llu has no window table", (unsigned long long)pair);
            const uint32_t cen = std::min(b->win_tab[b->win_at[pair] - 1 + strip], n);
            lo = swmi_aff_adapt_lo(cen, (uint32_t)md.band); hi = swmi_aff_adapt_hi(cen, n, (uint32_t)md.band);
        } else {
            lo = swmi_aff_band_lo(strip, (uint32_t)md.band); hi = swmi_aff_band_hi(strip, n, (uint32_t)md.band);
        }
    }
    if (c_lo) *c_lo = lo;
    if (c_hi) *c_hi = hi;
    return SWMI_OK;
}

// every pair's score and alignment count at once (bulk form of the two accessors above)
extern "C" int swmi_batch_pair_results(const swmi_batch *b, int32_t *scores, uint64_t *n_alignments, uint64_t n) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (n != batch_n_pairs(b)) return fail(SWMI_ERR_RANGE, "the batch has %llu pairs, not %llu",
                                           (unsigned long long)batch_n_pairs(b), (unsigned long long)n);
    if (b->scores_only && n_alignments)
        return fail(SWMI_ERR_INVALID, "the batch was run with scores_only = 1: pass n_alignments = NULL");
    for (uint64_t k = 0; k < n; k++) {
        if (scores) scores[k] = b->pairs[k].score;
        if (n_alignments) n_alignments[k] = b->pairs[k].n_cells;
    }
    return SWMI_OK;
}

// option "subopt": the pair's second-best score and its end column (swmi.h)
extern "C" int swmi_pair_subopt(const swmi_batch *b, uint64_t pair, int32_t *score2, uint32_t *end2) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    if (!b->has_sub) return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with subopt = 0: there is no second-best score");
    if (score2) *score2 = b->sub[pair].score2;
    if (end2) *end2 = b->sub[pair].end2;
    return SWMI_OK;
}

extern "C" int swmi_batch_pair_subopt(const swmi_batch *b, int32_t *score2, uint32_t *end2, uint64_t n) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (!b->has_sub) return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with subopt = 0: there is no second-best score");
    if (n != batch_n_pairs(b)) return fail(SWMI_ERR_RANGE, "the batch has %llu pairs, not %llu",
                                           (unsigned long long)batch_n_pairs(b), (unsigned long long)n);
    for (uint64_t k = 0; k < n; k++) {
        if (score2) score2[k] = b->sub[k].score2;
        if (end2) end2[k] = b->sub[k].end2;
    }
    return SWMI_OK;
}

// option "hits": the pair's K best separated local end cells (swmi.h); `hitv` holds 1 + K entries per pair, the count first
extern "C" int swmi_pair_hits(const swmi_batch *b, uint64_t pair, swmi_hit *hits, uint32_t cap, uint32_t *n_hits) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    if (!b->hits_k) return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with hits = 0: there is no list of hits");
    const HitEnt *e = b->hitv.data() + pair * (size_t)(1 + b->hits_k);
    const uint32_t cnt = (uint32_t)e[0].score;
    if (n_hits) *n_hits = cnt;
    if (!hits) return SWMI_OK;
    if (cap < cnt) return fail(SWMI_ERR_RANGE, "pair %llu has %u hits, the array holds %u", (unsigned long long)pair, cnt, cap);
    for (uint32_t k = 0; k < cnt; k++) hits[k] = swmi_hit{e[1 + k].score, e[1 + k].end_i, e[1 + k].end_j, 0u};
    return SWMI_OK;
}

extern "C" int swmi_batch_pair_hits(const swmi_batch *b, swmi_hit *hits, uint32_t cap_per_pair, uint32_t *n_hits, uint64_t n) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (!b->hits_k) return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with hits = 0: there is no list of hits");
    if (n != batch_n_pairs(b)) return fail(SWMI_ERR_RANGE, "the batch has %llu pairs, not %llu",
                                           (unsigned long long)batch_n_pairs(b), (unsigned long long)n);
    if (hits && cap_per_pair < (uint32_t)b->hits_k)
        return fail(SWMI_ERR_RANGE, "the run had hits = %d, the array holds %u entries per pair", b->hits_k, cap_per_pair);
    const size_t per = 1 + (size_t)b->hits_k;
    for (uint64_t p = 0; p < n; p++) {
        const HitEnt *e = b->hitv.data() + p * per;
        const uint32_t cnt = (uint32_t)e[0].score;
        if (n_hits) n_hits[p] = cnt;
        if (!hits) continue;
        for (uint32_t k = 0; k < cap_per_pair; k++)
            hits[p * cap_per_pair + k] = k < cnt ? swmi_hit{e[1 + k].score, e[1 + k].end_i, e[1 + k].end_j, 0u} : swmi_hit{0, 0u, 0u, 0u};
    }
    return SWMI_OK;
}

// option "end_bonus": the pair's best score anywhere, its best score in read row m and that score's first column (swmi.h)
extern "C" int swmi_pair_end_score(const swmi_batch *b, uint64_t pair, int32_t *max_score, int32_t *end_score, uint32_t *end_col) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    if (!b->has_endb) return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with end_bonus = 0: there is no to-end score");
    if (max_score) *max_score = b->endv[pair].max_score;
    if (end_score) *end_score = b->endv[pair].end_score;
    if (end_col) *end_col = b->endv[pair].end_col;
    return SWMI_OK;
}

extern "C" int swmi_batch_pair_end_scores(const swmi_batch *b, int32_t *max_score, int32_t *end_score, uint32_t *end_col, uint64_t n) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (!b->has_endb) return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with end_bonus = 0: there is no to-end score");
    if (n != batch_n_pairs(b)) return fail(SWMI_ERR_RANGE, "the batch has %llu pairs, not %llu",
                                           (unsigned long long)batch_n_pairs(b), (unsigned long long)n);
    for (uint64_t k = 0; k < n; k++) {
        if (max_score) max_score[k] = b->endv[k].max_score;
        if (end_score) end_score[k] = b->endv[k].end_score;
        if (end_col) end_col[k] = b->endv[k].end_col;
    }
    return SWMI_OK;
}

// Pops the traceback "stack" into the two aligned strings (SmithWaterman.java:418-431): ops are stored
// from the max cell backwards, so the strings are built by walking them in reverse.
static void materialise(swmi_batch *b, uint64_t pair, HostAln &a, uint64_t slot) {
    const uint32_t r = pair_ref(b, pair), q = pair_read(b, pair);
    const uint8_t *ref, *read;
    std::vector<uint8_t> rev_ref, rev_read;      // a transformed segment of a pair list: as the kernels saw it
    if (b->paired) {
        // a pair list: the segments are cut -- and reversed, the read of a minus-strand pair complemented -- from
        // the batch's copy of the source bytes
        const swmi_pair_spec &sp = b->specs[pair];
        ref = b->ref_bytes.data() + b->ref_off[sp.ref] + sp.ref_start;
        read = b->read_bytes.data() + b->read_off[sp.read] + sp.read_start;
        const bool R = (sp.flags & SWMI_SPEC_REVERSE) != 0, Cc = (sp.flags & SWMI_SPEC_READ_REVCOMP) != 0;
        if (R) {
            rev_ref.assign(std::make_reverse_iterator(ref + sp.ref_len), std::make_reverse_iterator(ref));
            ref = rev_ref.data();
        }
        if (R || Cc) {
            if (R != Cc) rev_read.assign(std::make_reverse_iterator(read + sp.read_len), std::make_reverse_iterator(read));
            else rev_read.assign(read, read + sp.read_len);
            if (Cc) { const uint8_t *K = complement_table(); for (auto &x : rev_read) x = K[x]; }
            read = rev_read.data();
        }
    } else if (b->src_map) {
        auto it = b->src_cache.find(r);
        if (it == b->src_cache.end()) {
            it = b->src_cache.emplace(r, std::vector<uint8_t>()).first;
            swmi_io_read_record(b->src_map, b->src_recs[r], it->second);
        }
        ref = it->second.data();
    } else {
        ref = b->ref_bytes.data() + b->ref_off[r];
    }
    if (!b->paired) read = b->read_bytes.data() + b->read_off[q];
    char *sr = b->str_buf.data() + b->str_at[slot], *sq = sr + a.n_ops + 1;
    sr[a.n_ops] = 0; sq[a.n_ops] = 0;
    int64_t i = a.end_i, j = a.end_j;     // 1-based cell of the op being emitted (both >= 1 while ops remain)
    if (b->rec_cigar) {
        // option "cigar": the payload is {n_cigar, nm, entries from the alignment's start}; the strings are filled from their end,
        // entry by entry backwards -- the walk's order.  An entry that would leave the strings or a sequence ends the expansion
        // (a corrupted record: the strings stay NUL-terminated)
        const uint32_t nc = a.rec[0];
        int64_t pos = (int64_t)a.n_ops - 1;
        for (uint32_t e = nc; e-- > 0;) {
            const uint32_t op = a.rec[2 + e] & 15u;
            const int64_t len = a.rec[2 + e] >> 4;
            const bool use_ref = op != SWMI_CIGAR_I, use_read = op != SWMI_CIGAR_D;
            if (len > pos + 1 || (use_ref && len > j) || (use_read && len > i)) break;
            for (int64_t x = 0; x < len; x++, pos--) {
                sr[pos] = use_ref ? (char)ref[j - 1 - x] : '_';
                sq[pos] = use_read ? (char)read[i - 1 - x] : '_';
            }
            if (use_ref) j -= len;
            if (use_read) i -= len;
        }
        a.str_id = (int64_t)b->str_at[slot];
        return;
    }
    const uint32_t *ops = a.rec;
    // Four ops (one byte of the packed stream) at a time: a table gives, for each of the 256 byte values, how far behind the
    // current cell every op reads its reference / read base (or that it writes '_'), so the four characters of each string do
    // not wait for each other's i, j -- the per-op loop below is one dependent chain per character.
    struct Lut { uint8_t nref, nread, roff[4], qoff[4], rgap[4], qgap[4]; };
    static const Lut *lut = [] {
        static Lut t[256];
        for (int v = 0; v < 256; v++) {
            Lut &L = t[v];
            L.nref = L.nread = 0;
            for (int k = 0; k < 4; k++) {
                const uint32_t op = (v >> (2 * k)) & 3u;
                const bool use_ref = op != SWMI_DIR_I, use_read = op != SWMI_DIR_D;
                L.roff[k] = L.nref; L.qoff[k] = L.nread;
                L.rgap[k] = use_ref ? 0 : 0xFF; L.qgap[k] = use_read ? 0 : 0xFF;
                L.nref += use_ref; L.nread += use_read;
            }
        }
        return t;
    }();
    uint32_t t = 0;
    while (t + 4 <= a.n_ops && i >= 4 && j >= 4) {          // (t is a multiple of 4: the byte does not straddle a dword)
        const Lut &L = lut[(ops[t >> 4] >> (2 * (t & 15))) & 0xFFu];
        const uint32_t pos = a.n_ops - 1 - t;
        for (int k = 0; k < 4; k++) {
            const uint8_t rc = ref[j - 1 - L.roff[k]], qc = read[i - 1 - L.qoff[k]];       // (always inside: i, j >= 4)
            sr[pos - k] = (char)((rc & ~L.rgap[k]) | ('_' & L.rgap[k]));
            sq[pos - k] = (char)((qc & ~L.qgap[k]) | ('_' & L.qgap[k]));
        }
        j -= L.nref; i -= L.nread;
        t += 4;
    }
    for (; t < a.n_ops; t++) {
        const uint32_t op = (ops[t >> 4] >> (2 * (t & 15))) & 3u;
        const uint32_t pos = a.n_ops - 1 - t;
        // branch-free: gaps come at random places of a path (:388-406: alignment takes both, insertion the read's, deletion the reference's)
        const bool use_ref = op != SWMI_DIR_I, use_read = op != SWMI_DIR_D;
        sr[pos] = use_ref ? (char)ref[j - 1] : '_';
        sq[pos] = use_read ? (char)read[i - 1] : '_';
        j -= use_ref; i -= use_read;
    }
    a.str_id = (int64_t)b->str_at[slot];
}

static const char EMPTY_STR[1] = {0};

extern "C" int swmi_pair_alignment(swmi_batch *b, uint64_t pair, uint64_t k,
                                   int32_t *begin, int32_t *end_i, int32_t *end_j,
                                   const char **ref_aln, const char **read_aln, uint32_t *len) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    if ((rc = ensure_indexed(b))) return rc;
    PairRes &pr = b->pairs[pair];
    if (k >= pr.n_cells) return fail(SWMI_ERR_RANGE, "alignment %llu out of range", (unsigned long long)k);
    if (pr.flags & SWMI_PAIR_DEGENERATE) {
        // every cell, row-major, traces to (0, "", "")  (SmithWaterman.java:378-380)
        const uint32_t n = b->ref_desc[pair_ref(b, pair)].len;
        if (begin) *begin = 0;
        if (end_i) *end_i = (int32_t)(k / n) + 1;
        if (end_j) *end_j = (int32_t)(k % n) + 1;
        if (ref_aln) *ref_aln = EMPTY_STR;
        if (read_aln) *read_aln = EMPTY_STR;
        if (len) *len = 0;
        return SWMI_OK;
    }
    HostAln &a = b->alns[pr.first + k];
    if (begin) *begin = a.begin;
    if (end_i) *end_i = a.end_i;
    if (end_j) *end_j = a.end_j;
    if (len) *len = a.n_ops;
    if (b->rec_strings) {
        // both strings were written by the traceback kernel right behind the record (swmi_emit.h): pointers only
        const uint32_t *sr = a.rec;
        if (ref_aln) *ref_aln = (const char *)sr;
        if (read_aln) *read_aln = (const char *)(sr + a.n_ops / 4u + 1u);
        return SWMI_OK;
    }
    if (a.str_id < 0) materialise(b, pair, a, pr.first + k);
    if (ref_aln) *ref_aln = b->str_buf.data() + a.str_id;
    if (read_aln) *read_aln = b->str_buf.data() + a.str_id + a.n_ops + 1;
    return SWMI_OK;
}

// Option "cigar": the alignment as the traceback kernel wrote it -- a pointer into the record stream, nothing is built.
extern "C" int swmi_pair_cigar(swmi_batch *b, uint64_t pair, uint64_t k,
                               int32_t *begin, int32_t *end_i, int32_t *end_j,
                               const uint32_t **cigar, uint32_t *n_cigar, uint32_t *nm) {
    int rc = check_pair(b, pair);
    if (rc) return rc;
    if (b->scores_only)
        return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with scores_only = 1: scores and totals only, no CIGARs");
    if (!b->rec_cigar)
        return fail(SWMI_ERR_UNSUPPORTED, "the batch was run with cigar = 0: set option cigar to 1 or 2 before the run");
    if ((rc = ensure_indexed(b))) return rc;
    PairRes &pr = b->pairs[pair];
    if (k >= pr.n_cells) return fail(SWMI_ERR_RANGE, "alignment %llu out of range", (unsigned long long)k);
    if (pr.flags & SWMI_PAIR_DEGENERATE) {
        const uint32_t n = b->ref_desc[pair_ref(b, pair)].len;
        if (begin) *begin = 0;
        if (end_i) *end_i = (int32_t)(k / n) + 1;
        if (end_j) *end_j = (int32_t)(k % n) + 1;
        if (cigar) *cigar = nullptr;
        if (n_cigar) *n_cigar = 0;
        if (nm) *nm = 0;
        return SWMI_OK;
    }
    const HostAln &a = b->alns[pr.first + k];
    if (begin) *begin = a.begin;
    if (end_i) *end_i = a.end_i;
    if (end_j) *end_j = a.end_j;
    if (cigar) *cigar = a.rec + 2;
    if (n_cigar) *n_cigar = a.rec[0];
    if (nm) *nm = a.rec[1];
    return SWMI_OK;
}

// Everything OptAlignments returns for every pair of the batch, built in one call: record index + both strings of every
// alignment (SmithWaterman.java:418-431).  The accessors above then only hand out pointers.
extern "C" int swmi_batch_materialise_all(swmi_batch *b, uint64_t *n_alignments, uint64_t *n_chars) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    int rc = ensure_indexed(b);
    if (rc) return rc;
    uint64_t na = 0, nc = 0;
    const uint64_t np = batch_n_pairs(b);
    for (uint64_t pair = 0; pair < np; pair++) {
        const PairRes &pr = b->pairs[pair];
        if (pr.flags & SWMI_PAIR_DEGENERATE) { na += pr.n_cells; continue; }     // (0, "", "") each: nothing to build
        for (uint64_t k = 0; k < pr.count; k++) nc += 2ull * b->alns[pr.first + k].n_ops;
        na += pr.count;
    }
    if (b->rec_strings) {          // the kernels wrote every string: the index is all there was to do
        if (n_alignments) *n_alignments = na;
        if (n_chars) *n_chars = nc;
        return SWMI_OK;
    }
    // every string has its own place in str_buf: pairs are built independently, by a few threads when there is enough to do
    // (streamed chunks re-read reference bytes through a cache that is not thread-safe: one thread there)
    auto build = [b](uint64_t lo, uint64_t hi) {
        for (uint64_t pair = lo; pair < hi; pair++) {
            PairRes &pr = b->pairs[pair];
            if (pr.flags & SWMI_PAIR_DEGENERATE) continue;
            for (uint64_t k = 0; k < pr.count; k++) {
                HostAln &a = b->alns[pr.first + k];
                if (a.str_id < 0) materialise(b, pair, a, pr.first + k);
            }
        }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    static const unsigned max_threads = getenv("SWMI_MAT_THREADS") ? (unsigned)atoi(getenv("SWMI_MAT_THREADS")) : 4u;
    // (measured at 412 k characters: 0.27 ms on one thread, no faster on 4 or 8 -- starting them costs what they save)
    const unsigned nt = (b->src_map || nc < 1000000) ? 1u : std::min<unsigned>({std::max(1u, max_threads), hw, (unsigned)(nc / 500000)});
    if (nt <= 1) {
        build(0, np);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back(build, np * t / nt, np * (t + 1) / nt);
        build(0, np / nt);
        for (auto &x : th) x.join();
    }
    if (n_alignments) *n_alignments = na;
    if (n_chars) *n_chars = nc;
    return SWMI_OK;
}

// ------------------------------------------------------------------------------------------
// MapRef view (Distribution.java:403-436)
// ------------------------------------------------------------------------------------------
// (a pair list has no "all reads of one reference": the views are refused there, swmi.h)
static int unsupported_on_pair_list(const char *what) {
    return fail(SWMI_ERR_UNSUPPORTED, "%s needs the cross product refs x reads: the batch is a pair list (swmi_batch_upload_pairs)", what);
}

static int check_ref(const swmi_batch *b, uint32_t ref) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (b->paired) return unsupported_on_pair_list("a MapRef view");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (ref >= b->n_refs) return fail(SWMI_ERR_RANGE, "reference %u out of range", ref);
    return SWMI_OK;
}

extern "C" int swmi_ref_total(const swmi_batch *b, uint32_t ref, int32_t *total) {
    int rc = check_ref(b, ref);
    if (rc) return rc;
    uint32_t t = 0;                                  // Java int arithmetic wraps
    for (uint32_t q = 0; q < b->n_reads; q++) t += (uint32_t)b->pairs[(uint64_t)ref * b->n_reads + q].score;
    if (total) *total = (int32_t)t;
    return SWMI_OK;
}

extern "C" int swmi_ref_totals(const swmi_batch *b, int32_t *totals, uint32_t n) {
    if (!b || !totals) return fail(SWMI_ERR_INVALID, "null argument");
    if (b->paired) return unsupported_on_pair_list("swmi_ref_totals");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (n != b->n_refs) return fail(SWMI_ERR_RANGE, "totals has %u entries, the batch has %u references", n, b->n_refs);
    for (uint32_t r = 0; r < b->n_refs; r++) {
        uint32_t t = 0;
        const PairRes *pr = b->pairs.data() + (uint64_t)r * b->n_reads;
        for (uint32_t q = 0; q < b->n_reads; q++) t += (uint32_t)pr[q].score;
        totals[r] = (int32_t)t;
    }
    return SWMI_OK;
}

static void build_ref_view(swmi_batch *b, uint32_t ref) {
    if (b->ref_view_ready[ref]) return;
    b->views_built = true;
    std::vector<SiteRef> &v = b->ref_sites[ref];
    uint64_t deg = 0;
    for (uint32_t q = 0; q < b->n_reads; q++) {
        const uint64_t pair = (uint64_t)ref * b->n_reads + q;
        const PairRes &pr = b->pairs[pair];
        if (pr.flags & SWMI_PAIR_DEGENERATE) { deg += pr.n_cells; continue; }   // begin 0: sorts before every real site
        for (uint64_t k = 0; k < pr.count; k++) v.push_back(SiteRef{pair, k, b->alns[pr.first + k].begin});
    }
    std::stable_sort(v.begin(), v.end(), [](const SiteRef &a, const SiteRef &c) { return a.begin < c.begin; });
    b->ref_degenerate[ref] = deg;
    b->ref_view_ready[ref] = 1;
}

extern "C" int swmi_ref_n_match_sites(swmi_batch *b, uint32_t ref, uint64_t *n) {
    int rc = check_ref(b, ref);
    if (rc) return rc;
    if ((rc = ensure_indexed(b))) return rc;
    build_ref_view(b, ref);
    if (n) *n = b->ref_degenerate[ref] + b->ref_sites[ref].size();
    return SWMI_OK;
}

extern "C" int swmi_ref_match_site(swmi_batch *b, uint32_t ref, uint64_t k, int32_t *begin,
                                   const char **ref_aln, const char **read_aln, uint32_t *len) {
    int rc = check_ref(b, ref);
    if (rc) return rc;
    if ((rc = ensure_indexed(b))) return rc;
    build_ref_view(b, ref);
    const uint64_t deg = b->ref_degenerate[ref];
    if (k < deg) {
        if (begin) *begin = 0;
        if (ref_aln) *ref_aln = EMPTY_STR;
        if (read_aln) *read_aln = EMPTY_STR;
        if (len) *len = 0;
        return SWMI_OK;
    }
    if (k - deg >= b->ref_sites[ref].size()) return fail(SWMI_ERR_RANGE, "match site %llu out of range", (unsigned long long)k);
    const SiteRef &s = b->ref_sites[ref][k - deg];
    return swmi_pair_alignment(b, s.pair, s.k, begin, nullptr, nullptr, ref_aln, read_aln, len);
}

// MapRef's output for a range of references in ONE call: what a per-partition binding (JNI, one call per Spark partition)
// hands back instead of three calls and two array allocations per match site (Distribution.java:419-433).
extern "C" int swmi_ref_sites_packed(swmi_batch *b, uint32_t ref_lo, uint32_t ref_hi,
                                     int32_t *totals, uint64_t *degenerate, uint64_t *site_first,
                                     int32_t *begins, uint32_t *lens, uint64_t *str_off, uint64_t sites_cap,
                                     uint8_t *blob, uint64_t blob_cap, uint64_t *n_sites, uint64_t *blob_bytes) {
    if (!b) return fail(SWMI_ERR_INVALID, "batch is null");
    if (b->paired) return unsupported_on_pair_list("swmi_ref_sites_packed");
    if (!b->has_run) return fail(SWMI_ERR_INVALID, "batch has no results (run it first)");
    if (ref_lo > ref_hi || ref_hi > b->n_refs) return fail(SWMI_ERR_RANGE, "reference range [%u, %u) out of range", ref_lo, ref_hi);
    int rc = ensure_indexed(b);
    if (rc) return rc;
    // pass 1: counts (always), so that a caller may ask for the sizes first (begins == NULL or capacities too small)
    uint64_t ns = 0, nb = 0;
    for (uint32_t r = ref_lo; r < ref_hi; r++) {
        build_ref_view(b, r);
        for (const SiteRef &sr : b->ref_sites[r]) nb += 2ull * b->alns[b->pairs[sr.pair].first + sr.k].n_ops;
        ns += b->ref_sites[r].size();
    }
    if (n_sites) *n_sites = ns;
    if (blob_bytes) *blob_bytes = nb;
    const bool fill = begins && lens && str_off && (blob || nb == 0) && sites_cap >= ns && blob_cap >= nb;
    uint64_t s_at = 0, c_at = 0;
    for (uint32_t r = ref_lo; r < ref_hi; r++) {
        if (totals) { int32_t t = 0; (void)swmi_ref_total(b, r, &t); totals[r - ref_lo] = t; }
        if (degenerate) degenerate[r - ref_lo] = b->ref_degenerate[r];           // leading (0, "", "") sites, not listed one by one
        if (site_first) site_first[r - ref_lo] = s_at;
        if (fill)
            for (const SiteRef &sr : b->ref_sites[r]) {
                const PairRes &pr = b->pairs[sr.pair];
                HostAln &a = b->alns[pr.first + sr.k];
                const char *ra, *qa;
                if (b->rec_strings) {
                    const uint32_t *w = a.rec;
                    ra = (const char *)w; qa = (const char *)(w + a.n_ops / 4u + 1u);
                } else {
                    if (a.str_id < 0) materialise(b, sr.pair, a, pr.first + sr.k);
                    ra = b->str_buf.data() + a.str_id; qa = ra + a.n_ops + 1;
                }
                begins[s_at] = a.begin; lens[s_at] = a.n_ops; str_off[s_at] = c_at;
                memcpy(blob + c_at, ra, a.n_ops);
                memcpy(blob + c_at + a.n_ops, qa, a.n_ops);
                c_at += 2ull * a.n_ops;
                s_at++;
            }
        else s_at += b->ref_sites[r].size();
    }
    if (site_first) site_first[ref_hi - ref_lo] = s_at;
    if (!fill && begins) return fail(SWMI_ERR_RANGE, "%llu sites / %llu string bytes do not fit the buffers (%llu / %llu)",
                                     (unsigned long long)ns, (unsigned long long)nb, (unsigned long long)sites_cap, (unsigned long long)blob_cap);
    return SWMI_OK;
}
