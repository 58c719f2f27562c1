/* shim_long.c -- swmi_shim_set_long_reads and swmi_shim_set_band (bindings/jni/swmi_shim.h) from plain C99, as nativeSetLongReads
 * and nativeSetBand call them.  Built and run by tests/test_affine_grid_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).
 * The sequences come from one rule, which the Python test repeats: x <- (x * 1103515245 + 12345) mod 2^31, base = "ACGT"[(x >> 16)
 * & 3]; the read is 1025 bases from x = 20260, the reference 300 bases from x = 4242 followed by the read -- so the whole read lies
 * on the diagonal j = i + 300, which a band of 16 cuts off at row 740.  With match 5, mismatch -3, gap -2, gapOpen -6 it prints
 *   "refused <status>"                                       without long_reads
 *   "<total> <sites> <begin>:<refAligned>/<readAligned> ... mode <pipeline mode>"   with long_reads = 1
 *   the same line                                            with band = 16
 *   "refused <status>"                                       with band = 0 and long_reads = 0 again */
#include <stdio.h>
#include "swmi.h"
#include "swmi_shim.h"

#define READ_LEN 1025
#define HEAD_LEN 300

static void gen(char *dst, int n, uint32_t x) {
    int k;
    for (k = 0; k < n; k++) {
        x = (x * 1103515245u + 12345u) & 0x7FFFFFFFu;
        dst[k] = "ACGT"[(x >> 16) & 3u];
    }
}

static int run(swmi_ctx *ctx, const char *ref, const char *read) {
    char err[640];
    const signed char types[4] = {'a', 'i', 'd', '-'};
    int64_t ro[2], qo[2], n = 0, k;
    swmi_batch *b = NULL;
    int32_t total = 0;
    int mode = -1, rc;
    ro[0] = 0; ro[1] = HEAD_LEN + READ_LEN; qo[0] = 0; qo[1] = READ_LEN;
    rc = swmi_shim_align_batch(ctx, 5, -3, -2, 0, types, 4, ref, ro[1], ro, 1, read, qo[1], qo, 1, &b, err, sizeof err);
    if (rc != SWMI_OK) { printf("refused %d\n", rc); return b == NULL ? 0 : 6; }
    if (swmi_shim_ref_total(b, 0, &total, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    if (swmi_shim_ref_site_count(b, 0, &n, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    printf("%d %ld", (int)total, (long)n);
    for (k = 0; k < n; k++) {
        int32_t begin = 0; const char *ra = NULL, *qa = NULL; uint32_t len = 0;
        if (swmi_shim_ref_site(b, 0, k, &begin, &ra, &qa, &len, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 8; }
        printf(" %d:%s/%s", (int)begin, ra, qa);
    }
    if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
    printf(" mode %d\n", mode);
    swmi_batch_free(ctx, b);
    return 0;
}

int main(void) {
    static char ref[HEAD_LEN + READ_LEN], read[READ_LEN];
    char err[640];
    swmi_ctx *ctx = NULL;
    int rc;
    gen(read, READ_LEN, 20260u);
    gen(ref, HEAD_LEN, 4242u);
    gen(ref + HEAD_LEN, READ_LEN, 20260u);
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_long_reads(NULL, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR long_reads: null context accepted\n"); return 4; }
    if (swmi_shim_set_long_reads(ctx, 2, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR long_reads 2 accepted\n"); return 4; }
    if (swmi_shim_set_long_reads(ctx, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR long_reads -1 accepted\n"); return 4; }
    if (swmi_shim_set_band(NULL, 16, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR band: null context accepted\n"); return 4; }
    if (swmi_shim_set_band(ctx, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR band -1 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -6, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if ((rc = run(ctx, ref, read)) != 0) return rc;              /* (the refused values left long_reads at 0) */
    if (swmi_shim_set_long_reads(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if ((rc = run(ctx, ref, read)) != 0) return rc;
    if (swmi_shim_set_band(ctx, 16, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if ((rc = run(ctx, ref, read)) != 0) return rc;
    if (swmi_shim_set_band(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_long_reads(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if ((rc = run(ctx, ref, read)) != 0) return rc;
    swmi_destroy(ctx);
    return 0;
}
