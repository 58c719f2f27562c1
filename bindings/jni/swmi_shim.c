/* swmi_shim.c -- see swmi_shim.h.  C99, no JNI types. */
#include <stdio.h>
#include <string.h>
#include "swmi_shim.h"

static int shim_fail(int code, char *err, size_t err_len, const char *where, const char *msg) {
    if (err && err_len) snprintf(err, err_len, "%s: %s", where, msg);
    return code;
}

static int check_side(const char *what, const void *bytes, int64_t cap, const int64_t *off, int32_t n,
                      char *err, size_t err_len) {
    int32_t k;
    if (n < 0) return shim_fail(SWMI_ERR_INVALID, err, err_len, what, "negative sequence count");
    if (!off) return shim_fail(SWMI_ERR_INVALID, err, err_len, what, "offset array is null");
    if (off[0] != 0) return shim_fail(SWMI_ERR_INVALID, err, err_len, what, "offsets must start at 0");
    for (k = 0; k < n; k++)
        if (off[k + 1] < off[k]) return shim_fail(SWMI_ERR_INVALID, err, err_len, what, "offsets decrease");
    if (off[n] > 0 && !bytes)
        return shim_fail(SWMI_ERR_INVALID, err, err_len, what, "byte buffer is null or not a direct ByteBuffer");
    if (off[n] > cap) return shim_fail(SWMI_ERR_INVALID, err, err_len, what, "offsets run past the buffer's capacity");
    return SWMI_OK;
}

int swmi_shim_set_gap_open(swmi_ctx *ctx, int32_t gap_open, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetGapOpen", "context handle is 0");
    if (gap_open > 0) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetGapOpen", "gapOpen must be <= 0");
    if ((rc = swmi_set_option(ctx, "gap_open", gap_open)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetGapOpen", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_align_mode(swmi_ctx *ctx, int32_t align_mode, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetAlignMode", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "align_mode", align_mode)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetAlignMode", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_long_reads(swmi_ctx *ctx, int32_t long_reads, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetLongReads", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "long_reads", long_reads)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetLongReads", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_band(swmi_ctx *ctx, int32_t band, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetBand", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "band", band)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetBand", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_extend(swmi_ctx *ctx, int32_t extend, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetExtend", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "extend", extend)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetExtend", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_xdrop(swmi_ctx *ctx, int32_t xdrop, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetXdrop", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "xdrop", xdrop)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetXdrop", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_gap2(swmi_ctx *ctx, int32_t gap_open2, int32_t gap2, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetGap2", "context handle is 0");
    if (gap_open2 > 0 || gap2 > 0) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetGap2", "gap_open2 and gap2 must be <= 0");
    if ((rc = swmi_set_option(ctx, "gap2", gap2)) != SWMI_OK || (rc = swmi_set_option(ctx, "gap_open2", gap_open2)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetGap2", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_band_adapt(swmi_ctx *ctx, int32_t band_adapt, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetBandAdapt", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "band_adapt", band_adapt)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetBandAdapt", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_cigar(swmi_ctx *ctx, int32_t cigar, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetCigar", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "cigar", cigar)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetCigar", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_subopt(swmi_ctx *ctx, int32_t subopt, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetSubopt", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "subopt", subopt)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetSubopt", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_pair_subopt(const swmi_batch *b, int64_t pair, int32_t out[2], char *err, size_t err_len) {
    int32_t s2 = 0;
    uint32_t e2 = 0;
    int rc;
    if (pair < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairSubopt", "negative index");
    rc = swmi_pair_subopt(b, (uint64_t)pair, &s2, &e2);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_pair_subopt", swmi_last_error());
    if (out) { out[0] = s2; out[1] = (int32_t)e2; }      /* (a column is below 2^30) */
    return SWMI_OK;
}

int swmi_shim_set_end_bonus(swmi_ctx *ctx, int32_t end_bonus, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetEndBonus", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "end_bonus", end_bonus)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetEndBonus", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_overlap(swmi_ctx *ctx, int32_t overlap, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetOverlap", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "overlap", overlap)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetOverlap", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_pair_end_score(const swmi_batch *b, int64_t pair, int32_t out[4], char *err, size_t err_len) {
    int32_t ms = 0, es = 0;
    uint32_t ec = 0, flags = 0;
    uint64_t na = 0;
    int rc;
    if (pair < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairEndScore", "negative index");
    rc = swmi_pair_end_score(b, (uint64_t)pair, &ms, &es, &ec);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_pair_end_score", swmi_last_error());
    rc = swmi_pair_n_alignments(b, (uint64_t)pair, &na, &flags);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_pair_n_alignments", swmi_last_error());
    if (out) { out[0] = ms; out[1] = es; out[2] = (int32_t)ec; out[3] = (flags & SWMI_PAIR_TO_END) ? 1 : 0; }      /* (a column is below 2^30) */
    return SWMI_OK;
}

int swmi_shim_set_hits(swmi_ctx *ctx, int32_t hits, char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetHits", "context handle is 0");
    if ((rc = swmi_set_option(ctx, "hits", hits)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetHits", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_pair_hits(const swmi_batch *b, int64_t pair, int32_t *out, int32_t cap, int32_t *n, char *err, size_t err_len) {
    swmi_hit h[16];                                       /* (option "hits": at most 16 entries) */
    uint32_t cnt = 0, k;
    int rc;
    if (pair < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairHits", "negative index");
    if (out && cap < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairHits", "negative capacity");
    rc = swmi_pair_hits(b, (uint64_t)pair, h, 16u, &cnt);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_pair_hits", swmi_last_error());
    if (n) *n = (int32_t)cnt;
    if (!out) return SWMI_OK;
    if ((uint32_t)cap < cnt) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairHits", "the array holds fewer entries than the pair has");
    for (k = 0; k < cnt; k++) {                           /* (a row and a column are below 2^31) */
        out[3 * k] = h[k].score; out[3 * k + 1] = (int32_t)h[k].end_i; out[3 * k + 2] = (int32_t)h[k].end_j;
    }
    return SWMI_OK;
}

int swmi_shim_pair_cigar(swmi_batch *b, int64_t pair, int64_t k, int32_t *begin, int32_t cell[2], const uint32_t **cigar,
                         uint32_t *n_cigar, uint32_t *nm, char *err, size_t err_len) {
    int32_t ei = 0, ej = 0;
    int rc;
    if (pair < 0 || k < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairCigar", "negative index");
    rc = swmi_pair_cigar(b, (uint64_t)pair, (uint64_t)k, begin, &ei, &ej, cigar, n_cigar, nm);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_pair_cigar", swmi_last_error());
    if (cell) { cell[0] = ei; cell[1] = ej; }
    return SWMI_OK;
}

int swmi_shim_set_score_matrix(swmi_ctx *ctx, const signed char *alphabet, size_t n, const int32_t *scores, size_t n_scores,
                               char *err, size_t err_len) {
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetScoreMatrix", "context handle is 0");
    if (n > 64) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetScoreMatrix", "at most 64 symbols");
    if (n > 0 && (!alphabet || !scores))
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetScoreMatrix", "alphabet or scores is null");
    if (n_scores != n * n) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetScoreMatrix", "scores must hold n * n entries");
    if ((rc = swmi_set_score_matrix(ctx, n ? (const uint8_t *)alphabet : NULL, (uint32_t)n, n ? scores : NULL)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "nativeSetScoreMatrix", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_set_read_profiles(swmi_ctx *ctx, swmi_batch *b, int32_t match, int32_t mismatch, int32_t gap, int32_t tie_mode,
                                const signed char *types, size_t types_len, const signed char *alphabet, size_t n,
                                const int32_t *scores, size_t n_scores, int64_t n_rows, char *err, size_t err_len) {
    swmi_params p;
    int rc;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetReadProfiles", "context handle is 0");
    if (!b) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetReadProfiles", "batch handle is 0");
    if (!types || types_len != 4)
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetReadProfiles", "alignTypes must hold exactly 4 characters");
    if (n > 64) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetReadProfiles", "at most 64 symbols");
    if (n > 0 && (!alphabet || !scores))
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetReadProfiles", "alphabet or scores is null");
    if (n_rows < 0 || n_scores != n * (size_t)n_rows)
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeSetReadProfiles", "scores must hold n entries per read byte");
    if ((rc = swmi_batch_set_read_profiles(ctx, b, n ? (const uint8_t *)alphabet : NULL, (uint32_t)n, n ? scores : NULL)) != SWMI_OK)
        return shim_fail(rc, err, err_len, "swmi_batch_set_read_profiles", swmi_last_error());
    swmi_default_params(&p);
    p.match = match; p.mismatch = mismatch; p.gap = gap; p.tie_mode = tie_mode;
    memcpy(p.types, types, 4);
    if ((rc = swmi_batch_run(ctx, b, &p)) != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_batch_run", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_align_batch(swmi_ctx *ctx, int32_t match, int32_t mismatch, int32_t gap, int32_t tie_mode,
                          const signed char *types, size_t types_len,
                          const void *ref_bytes, int64_t ref_cap, const int64_t *ref_off, int32_t n_refs,
                          const void *read_bytes, int64_t read_cap, const int64_t *read_off, int32_t n_reads,
                          swmi_batch **out, char *err, size_t err_len) {
    swmi_params p;
    int rc;
    if (!out) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignBatch", "out is null");
    *out = NULL;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignBatch", "context handle is 0");
    if (!types || types_len != 4)
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignBatch", "alignTypes must hold exactly 4 characters");
    if ((rc = check_side("references", ref_bytes, ref_cap, ref_off, n_refs, err, err_len)) != SWMI_OK) return rc;
    if ((rc = check_side("reads", read_bytes, read_cap, read_off, n_reads, err, err_len)) != SWMI_OK) return rc;
    swmi_default_params(&p);
    p.match = match; p.mismatch = mismatch; p.gap = gap; p.tie_mode = tie_mode;
    memcpy(p.types, types, 4);
    /* jlong and uint64_t have the same size and the offsets were checked non-negative */
    rc = swmi_align_batch(ctx, &p, (const uint8_t *)ref_bytes, (const uint64_t *)(const void *)ref_off, (uint32_t)n_refs,
                          (const uint8_t *)read_bytes, (const uint64_t *)(const void *)read_off, (uint32_t)n_reads, out);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_align_batch", swmi_last_error());
    return SWMI_OK;
}

int swmi_shim_align_pairs(swmi_ctx *ctx, int32_t match, int32_t mismatch, int32_t gap, int32_t tie_mode,
                          const signed char *types, size_t types_len,
                          const void *ref_bytes, int64_t ref_cap, const int64_t *ref_off, int32_t n_refs,
                          const void *read_bytes, int64_t read_cap, const int64_t *read_off, int32_t n_reads,
                          const int32_t *specs, int64_t n_spec_ints, swmi_batch **out, char *err, size_t err_len) {
    swmi_params p;
    int rc;
    if (!out) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignPairs", "out is null");
    *out = NULL;
    if (!ctx) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignPairs", "context handle is 0");
    if (!types || types_len != 4)
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignPairs", "alignTypes must hold exactly 4 characters");
    if ((rc = check_side("references", ref_bytes, ref_cap, ref_off, n_refs, err, err_len)) != SWMI_OK) return rc;
    if ((rc = check_side("reads", read_bytes, read_cap, read_off, n_reads, err, err_len)) != SWMI_OK) return rc;
    if (n_spec_ints < 0 || n_spec_ints % 8 != 0)
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignPairs", "specs must hold 8 ints per pair");
    if (n_spec_ints > 0 && !specs) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeAlignPairs", "specs is null");
    swmi_default_params(&p);
    p.match = match; p.mismatch = mismatch; p.gap = gap; p.tie_mode = tie_mode;
    memcpy(p.types, types, 4);
    /* eight jints are one swmi_pair_spec: the same size, its members the unsigned type of the same width */
    rc = swmi_batch_upload_pairs(ctx, (const uint8_t *)ref_bytes, (const uint64_t *)(const void *)ref_off, (uint32_t)n_refs,
                                 (const uint8_t *)read_bytes, (const uint64_t *)(const void *)read_off, (uint32_t)n_reads,
                                 (const swmi_pair_spec *)(const void *)specs, (uint64_t)(n_spec_ints / 8), out);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_batch_upload_pairs", swmi_last_error());
    rc = swmi_batch_run(ctx, *out, &p);
    if (rc != SWMI_OK) {
        shim_fail(rc, err, err_len, "swmi_batch_run", swmi_last_error());
        swmi_batch_free(ctx, *out);
        *out = NULL;
    }
    return rc;
}

int swmi_shim_pair_results(const swmi_batch *b, int32_t *scores, int64_t *n_alignments, int64_t n, char *err, size_t err_len) {
    int rc;
    if (n < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairResults", "negative array length");
    /* (a count is below 2^63: jlong and uint64_t hold it alike) */
    rc = swmi_batch_pair_results(b, scores, (uint64_t *)(void *)n_alignments, (uint64_t)n);
    return rc == SWMI_OK ? rc : shim_fail(rc, err, err_len, "swmi_batch_pair_results", swmi_last_error());
}

int swmi_shim_pair_alignment(swmi_batch *b, int64_t pair, int64_t k, int32_t *begin, int32_t cell[2], const char **ref_aln,
                             const char **read_aln, uint32_t *len, char *err, size_t err_len) {
    int32_t ei = 0, ej = 0;
    int rc;
    if (pair < 0 || k < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativePairAlignment", "negative index");
    rc = swmi_pair_alignment(b, (uint64_t)pair, (uint64_t)k, begin, &ei, &ej, ref_aln, read_aln, len);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_pair_alignment", swmi_last_error());
    if (cell) { cell[0] = ei; cell[1] = ej; }
    return SWMI_OK;
}

int swmi_shim_ref_total(const swmi_batch *b, int32_t ref, int32_t *total, char *err, size_t err_len) {
    int rc;
    if (ref < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativeRefTotal", "negative reference index");
    rc = swmi_ref_total(b, (uint32_t)ref, total);
    return rc == SWMI_OK ? rc : shim_fail(rc, err, err_len, "swmi_ref_total", swmi_last_error());
}

int swmi_shim_ref_site_count(swmi_batch *b, int32_t ref, int64_t *n, char *err, size_t err_len) {
    uint64_t v = 0;
    int rc;
    if (ref < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativeRefSiteCount", "negative reference index");
    rc = swmi_ref_n_match_sites(b, (uint32_t)ref, &v);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_ref_n_match_sites", swmi_last_error());
    if (n) *n = (int64_t)v;
    return SWMI_OK;
}

int swmi_shim_ref_site(swmi_batch *b, int32_t ref, int64_t k, int32_t *begin, const char **ref_aln, const char **read_aln,
                       uint32_t *len, char *err, size_t err_len) {
    int rc;
    if (ref < 0 || k < 0) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativeRefSite", "negative index");
    rc = swmi_ref_match_site(b, (uint32_t)ref, (uint64_t)k, begin, ref_aln, read_aln, len);
    return rc == SWMI_OK ? rc : shim_fail(rc, err, err_len, "swmi_ref_match_site", swmi_last_error());
}

int swmi_shim_ref_sites_sizes(swmi_batch *b, int32_t ref_lo, int32_t ref_hi, int64_t sizes[2], char *err, size_t err_len) {
    uint64_t ns = 0, nb = 0;
    int rc;
    if (ref_lo < 0 || ref_hi < ref_lo) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativeRefSitesSizes", "bad reference range");
    if (!sizes) return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeRefSitesSizes", "sizes is null");
    rc = swmi_ref_sites_packed(b, (uint32_t)ref_lo, (uint32_t)ref_hi, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, &ns, &nb);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_ref_sites_packed", swmi_last_error());
    sizes[0] = (int64_t)ns; sizes[1] = (int64_t)nb;
    return SWMI_OK;
}

int swmi_shim_ref_sites_packed(swmi_batch *b, int32_t ref_lo, int32_t ref_hi,
                               int32_t *totals, int64_t n_totals, int64_t *degenerate, int64_t n_degenerate,
                               int64_t *site_first, int64_t n_site_first,
                               int32_t *begins, int32_t *lens, int64_t *str_off, int64_t n_sites_cap,
                               signed char *blob, int64_t blob_cap, char *err, size_t err_len) {
    uint64_t ns = 0, nb = 0;
    int64_t n;
    int rc;
    if (ref_lo < 0 || ref_hi < ref_lo) return shim_fail(SWMI_ERR_RANGE, err, err_len, "nativeRefSitesPacked", "bad reference range");
    n = (int64_t)ref_hi - ref_lo;
    if (!totals || !degenerate || !site_first || !begins || !lens || !str_off || (!blob && blob_cap > 0))
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeRefSitesPacked", "null array argument");
    if (n_totals < n || n_degenerate < n || n_site_first < n + 1 || n_sites_cap < 0 || blob_cap < 0)
        return shim_fail(SWMI_ERR_INVALID, err, err_len, "nativeRefSitesPacked", "an output array is shorter than the reference range needs");
    /* jint / jlong and the C-ABI's unsigned types have the same sizes; counts were checked non-negative */
    rc = swmi_ref_sites_packed(b, (uint32_t)ref_lo, (uint32_t)ref_hi, totals, (uint64_t *)(void *)degenerate,
                               (uint64_t *)(void *)site_first, begins, (uint32_t *)(void *)lens, (uint64_t *)(void *)str_off,
                               (uint64_t)n_sites_cap, (uint8_t *)(void *)blob, (uint64_t)blob_cap, &ns, &nb);
    if (rc != SWMI_OK) return shim_fail(rc, err, err_len, "swmi_ref_sites_packed", swmi_last_error());
    return SWMI_OK;
}
