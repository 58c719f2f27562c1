/* shim_ends.c -- swmi_shim_set_align_mode (bindings/jni/swmi_shim.h) from plain C99, as nativeSetAlignMode calls it.
 * Built and run by tests/test_ends_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  For ref CGTCCAGACT x read AGGTCGAC
 * with match 2, mismatch -3, gap -1, gapOpen -3 (tests/golden/ends_kat.json EKAT-1 / EKAT-2) it prints, for the modes fit,
 * global and local in turn, the total, the number of match sites, the sites and the pipeline mode of the run. */
#include <stdio.h>
#include "swmi.h"
#include "swmi_shim.h"

int main(void) {
    char err[640];
    swmi_ctx *ctx = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    const char *ref = "CGTCCAGACT", *read = "AGGTCGAC";
    const int32_t modes[3] = {SWMI_ALIGN_FIT, SWMI_ALIGN_GLOBAL, SWMI_ALIGN_LOCAL};
    int64_t ro[2], qo[2], n, k;
    int x;
    ro[0] = 0; ro[1] = 10; qo[0] = 0; qo[1] = 8;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_align_mode(NULL, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_align_mode(ctx, 3, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR align_mode 3 accepted\n"); return 4; }
    if (swmi_shim_set_align_mode(ctx, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR align_mode -1 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -3, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (x = 0; x < 3; x++) {
        swmi_batch *b = NULL;
        int32_t total = 0;
        int mode = -1;
        if (swmi_shim_set_align_mode(ctx, modes[x], err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_align_batch(ctx, 2, -3, -1, 0, types, 4, ref, 10, ro, 1, read, 8, qo, 1, &b, err, sizeof err) != SWMI_OK) {
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
    }
    swmi_destroy(ctx);
    return 0;
}
