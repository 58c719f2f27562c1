/* shim_hits.c -- swmi_shim_set_hits and swmi_shim_pair_hits (bindings/jni/swmi_shim.h) from plain C99, as nativeSetHits and
 * nativePairHits call them.  Built and run by tests/test_hits_shim_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).
 * The sequences are those of shim_subopt.c, from the same rule, which the Python test repeats: x <- (x * 1103515245 + 12345) mod 2^31,
 * base = "ACGT"[(x >> 16) & 3].  The long read is 1100 bases from x = 20260, the short read its bases 900 .. 939.  The reference is the
 * long read's bases 100 .. 259, 50 bases from x = 4242, the short read once more, 50 bases from x = 777, and the long read's bases
 * 700 .. 1099.  With match 2, mismatch -3, gap -4, gapOpen -6 and subopt = 45 it prints, for the short pair and then for the long pair
 * (with long_reads = 1),
 *   "<n> : <score> <end_i> <end_j> ; ... mode <pipeline mode>"      under hits = 3, then under hits = 1
 *   "unsupported"                                                      under hits = 0 (swmi_shim_pair_hits returns SWMI_ERR_UNSUPPORTED)
 * and last "refused" for a run with hits = 3 and subopt = 0. */
#include <stdio.h>
#include <string.h>
#include "swmi.h"
#include "swmi_shim.h"

#define LONG_LEN 1100
#define SHORT_LEN 40
#define REF_LEN (160 + 50 + SHORT_LEN + 50 + 400)

static void gen(char *dst, int n, uint32_t x) {
    int k;
    for (k = 0; k < n; k++) {
        x = (x * 1103515245u + 12345u) & 0x7FFFFFFFu;
        dst[k] = "ACGT"[(x >> 16) & 3u];
    }
}

static int run(swmi_ctx *ctx, const char *ref, const char *read, int read_len, int expect_refusal) {
    char err[640];
    const signed char types[4] = {'a', 'i', 'd', '-'};
    int64_t ro[2], qo[2];
    swmi_batch *b = NULL;
    int32_t out[3 * 16], n = -1, n2 = -1;
    int mode = -1, rc, k;
    ro[0] = 0; ro[1] = REF_LEN; qo[0] = 0; qo[1] = read_len;
    rc = swmi_shim_align_batch(ctx, 2, -3, -4, 0, types, 4, ref, ro[1], ro, 1, read, qo[1], qo, 1, &b, err, sizeof err);
    if (expect_refusal) {
        if (rc != SWMI_ERR_UNSUPPORTED) { printf("ERROR hits without subopt: status %d\n", rc); return 6; }
        printf("refused\n");
        return 0;
    }
    if (rc != SWMI_OK) { printf("ERROR %s\n", err); return 6; }
    rc = swmi_shim_pair_hits(b, 0, out, 16, &n, err, sizeof err);
    if (rc == SWMI_ERR_UNSUPPORTED) { printf("unsupported\n"); swmi_batch_free(ctx, b); return 0; }
    if (rc != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    if (swmi_shim_pair_hits(b, 1, out, 16, &n2, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR pair 1 accepted\n"); return 7; }
    if (swmi_shim_pair_hits(b, -1, out, 16, &n2, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR pair -1 accepted\n"); return 7; }
    if (swmi_shim_pair_hits(b, 0, NULL, 0, &n2, err, sizeof err) != SWMI_OK || n2 != n) { printf("ERROR count only\n"); return 7; }
    if (n > 0 && swmi_shim_pair_hits(b, 0, out, n - 1, &n2, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR small array accepted\n"); return 7; }
    if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
    printf("%d :", (int)n);
    for (k = 0; k < n; k++) printf(" %d %d %d ;", (int)out[3 * k], (int)out[3 * k + 1], (int)out[3 * k + 2]);
    printf(" mode %d\n", mode);
    swmi_batch_free(ctx, b);
    return 0;
}

int main(void) {
    static char ref[REF_LEN], lng[LONG_LEN], shrt[SHORT_LEN];
    const int32_t values[3] = {3, 1, 0};
    char err[640];
    swmi_ctx *ctx = NULL;
    int rc, v;
    gen(lng, LONG_LEN, 20260u);
    memcpy(shrt, lng + 900, SHORT_LEN);
    memcpy(ref, lng + 100, 160);
    gen(ref + 160, 50, 4242u);
    memcpy(ref + 210, shrt, SHORT_LEN);
    gen(ref + 250, 50, 777u);
    memcpy(ref + 300, lng + 700, 400);
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_hits(NULL, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR hits: null context accepted\n"); return 4; }
    if (swmi_shim_set_hits(ctx, 17, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR hits 17 accepted\n"); return 4; }
    if (swmi_shim_set_hits(ctx, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR hits -1 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -6, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_subopt(ctx, 45, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (v = 0; v < 3; v++) {
        if (swmi_shim_set_hits(ctx, values[v], err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_set_long_reads(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if ((rc = run(ctx, ref, shrt, SHORT_LEN, 0)) != 0) return rc;
        if (swmi_shim_set_long_reads(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if ((rc = run(ctx, ref, lng, LONG_LEN, 0)) != 0) return rc;
    }
    if (swmi_shim_set_hits(ctx, 3, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_subopt(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if ((rc = run(ctx, ref, shrt, SHORT_LEN, 1)) != 0) return rc;
    swmi_destroy(ctx);
    return 0;
}
