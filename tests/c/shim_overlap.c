/* shim_overlap.c -- swmi_shim_set_overlap (bindings/jni/swmi_shim.h) from plain C99, as nativeSetOverlap calls it.
 * Built and run by tests/test_overlap_shim_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  For ref TTTTTACGCGGA x read
 * ACGCGGAAAAAAA with match 2, mismatch -3, gap -1, gapOpen -3 in fit mode it prints the total, the number of match sites, the sites
 * and the pipeline mode of the run with overlap 1 and with overlap 0, and then "refused <status>" for overlap 1 in global mode. */
#include <stdio.h>
#include "swmi.h"
#include "swmi_shim.h"

int main(void) {
    char err[640];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    const char *ref = "TTTTTACGCGGA", *read = "ACGCGGAAAAAAA";
    int64_t ro[2], qo[2], n, k;
    int x, rc;
    ro[0] = 0; ro[1] = 12; qo[0] = 0; qo[1] = 13;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_overlap(NULL, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_overlap(ctx, 2, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR overlap 2 accepted\n"); return 4; }
    if (swmi_shim_set_overlap(ctx, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR overlap -1 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -3, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_FIT, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (x = 1; x >= 0; x--) {
        int32_t total = 0;
        int mode = -1;
        if (swmi_shim_set_overlap(ctx, x, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_align_batch(ctx, 2, -3, -1, 0, types, 4, ref, 12, ro, 1, read, 13, qo, 1, &b, err, sizeof err) != SWMI_OK) {
            printf("ERROR %s\n", err); return 6;
        }
        n = 0;
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
        b = NULL;
    }
    if (swmi_shim_set_overlap(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_GLOBAL, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    rc = swmi_shim_align_batch(ctx, 2, -3, -1, 0, types, 4, ref, 12, ro, 1, read, 13, qo, 1, &b, err, sizeof err);
    if (rc == SWMI_OK) { printf("ERROR overlap in global mode accepted\n"); return 10; }
    printf("refused %d\n", rc);
    swmi_destroy(ctx);
    return 0;
}
