/* shim_end_bonus.c -- swmi_shim_set_end_bonus and swmi_shim_pair_end_score (bindings/jni/swmi_shim.h) from plain C99, as
 * nativeSetEndBonus and nativePairEndScore call them.  Built and run by tests/test_end_bonus_shim_gpu.py (gcc -std=c99 -Wall -Wextra
 * -Werror -pedantic).
 * The sequences come from one rule, which the Python test repeats: x <- (x * 1103515245 + 12345) mod 2^31, base = "ACGT"[(x >> 16)
 * & 3].  The long read is 1100 bases from x = 20261, the short read its first 60 bases.  The reference is the long read's first 1090
 * bases with base 59 (0-based) replaced by the next letter of "ACGT", then 30 bases from x = 4243: the short read reaches its end 3 below
 * its best score (its last base meets the substituted one), the long read's last 10 bases do not match.  With match 5, mismatch -4, gap -3, gapOpen -5,
 * align_mode global and extend = 1 it prints, for the short pair and then for the long pair (long_reads = 1),
 *   "<score> <max_score> <end_score> <end_col> <taken> mode <pipeline mode>"      under end_bonus = 3, 5 and 2^30
 *   "unsupported"                                       under end_bonus = 0 (swmi_shim_pair_end_score returns SWMI_ERR_UNSUPPORTED) */
#include <stdio.h>
#include <string.h>
#include "swmi.h"
#include "swmi_shim.h"

#define LONG_LEN 1100
#define SHORT_LEN 60
#define REF_LEN (1090 + 30)

static void gen(char *dst, int n, uint32_t x) {
    int k;
    for (k = 0; k < n; k++) {
        x = (x * 1103515245u + 12345u) & 0x7FFFFFFFu;
        dst[k] = "ACGT"[(x >> 16) & 3u];
    }
}

static int run(swmi_ctx *ctx, const char *ref, const char *read, int read_len) {
    char err[640];
    const signed char types[4] = {'a', 'i', 'd', '-'};
    int64_t ro[2], qo[2];
    swmi_batch *b = NULL;
    int32_t score = 0, out[4] = {-1, -1, -1, -1};
    int mode = -1, rc;
    ro[0] = 0; ro[1] = REF_LEN; qo[0] = 0; qo[1] = read_len;
    rc = swmi_shim_align_batch(ctx, 5, -4, -3, 0, types, 4, ref, ro[1], ro, 1, read, qo[1], qo, 1, &b, err, sizeof err);
    if (rc != SWMI_OK) { printf("ERROR %s\n", err); return 6; }
    rc = swmi_shim_pair_end_score(b, 0, out, err, sizeof err);
    if (rc == SWMI_ERR_UNSUPPORTED) { printf("unsupported\n"); swmi_batch_free(ctx, b); return 0; }
    if (rc != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    if (swmi_shim_pair_end_score(b, 1, out, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR pair 1 accepted\n"); return 7; }
    if (swmi_shim_pair_end_score(b, -1, out, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR pair -1 accepted\n"); return 7; }
    if (swmi_pair_score(b, 0, &score) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 8; }
    if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
    printf("%d %d %d %d %d mode %d\n", (int)score, (int)out[0], (int)out[1], (int)out[2], (int)out[3], mode);
    swmi_batch_free(ctx, b);
    return 0;
}

int main(void) {
    static char ref[REF_LEN], lng[LONG_LEN];
    const int32_t values[4] = {3, 5, 1 << 30, 0};
    char err[640];
    swmi_ctx *ctx = NULL;
    const char *p;
    int rc, v;
    gen(lng, LONG_LEN, 20261u);
    memcpy(ref, lng, 1090);
    p = strchr("ACGT", ref[59]);
    ref[59] = "ACGT"[((p - "ACGT") + 1) & 3];
    gen(ref + 1090, 30, 4243u);
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_end_bonus(NULL, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR end_bonus: null context accepted\n"); return 4; }
    if (swmi_shim_set_end_bonus(ctx, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR end_bonus -1 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -5, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_GLOBAL, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_extend(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (v = 0; v < 4; v++) {
        if (swmi_shim_set_end_bonus(ctx, values[v], err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_set_long_reads(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if ((rc = run(ctx, ref, lng, SHORT_LEN)) != 0) return rc;
        if (swmi_shim_set_long_reads(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if ((rc = run(ctx, ref, lng, LONG_LEN)) != 0) return rc;
    }
    swmi_destroy(ctx);
    return 0;
}
