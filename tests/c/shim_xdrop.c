/* shim_xdrop.c -- swmi_shim_set_xdrop (bindings/jni/swmi_shim.h) from plain C99, as nativeSetXdrop calls it.
 * Built and run by tests/test_xdrop_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  The reference is ACGTTGCA x 80 and 500
 * C's, the read ACGTTGCA x 80 and 385 A's (1025 bases: two strips), match 2, mismatch -4, gap -2, gapOpen -4, seed extension with
 * long reads on: the one maximum cell is (640, 640), and row 1024 lies 4 + 2 * 384 = 772 below it.  For xdrop 771, 772 and 0 it
 * prints the total, the number of match sites, begin:length of every site, the rows swept (swmi_pair_rows_swept) and the
 * pipeline mode, and then "refused <status>" for xdrop 771 without extend. */
#include <stdio.h>
#include <string.h>
#include "swmi.h"
#include "swmi_shim.h"

int main(void) {
    static const int32_t xs[3] = {771, 772, 0};
    char err[640], ref[1141], read[1026];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    int64_t ro[2], qo[2], n, k;
    int x, rc;
    for (x = 0; x < 80; x++) { memcpy(ref + 8 * x, "ACGTTGCA", 8); memcpy(read + 8 * x, "ACGTTGCA", 8); }
    memset(ref + 640, 'C', 500); ref[1140] = 0;
    memset(read + 640, 'A', 385); read[1025] = 0;
    ro[0] = 0; ro[1] = 1140; qo[0] = 0; qo[1] = 1025;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_xdrop(NULL, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_xdrop(ctx, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR xdrop -1 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -4, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_GLOBAL, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_long_reads(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_extend(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (x = 0; x < 3; x++) {
        int32_t total = 0;
        uint32_t rows = 0;
        int mode = -1;
        if (swmi_shim_set_xdrop(ctx, xs[x], err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_align_batch(ctx, 2, -4, -2, 0, types, 4, ref, 1140, ro, 1, read, 1025, qo, 1, &b, err, sizeof err) != SWMI_OK) {
            printf("ERROR %s\n", err); return 6;
        }
        n = 0;
        if (swmi_shim_ref_total(b, 0, &total, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
        if (swmi_shim_ref_site_count(b, 0, &n, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
        printf("%d %ld", (int)total, (long)n);
        for (k = 0; k < n; k++) {
            int32_t begin = 0; const char *ra = NULL, *qa = NULL; uint32_t len = 0;
            if (swmi_shim_ref_site(b, 0, k, &begin, &ra, &qa, &len, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 8; }
            printf(" %d:%u", (int)begin, (unsigned)len);
        }
        if (swmi_pair_rows_swept(b, 0, &rows) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
        if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
        printf(" rows %u mode %d\n", (unsigned)rows, mode);
        swmi_batch_free(ctx, b);
        b = NULL;
    }
    if (swmi_shim_set_xdrop(ctx, 771, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_extend(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    rc = swmi_shim_align_batch(ctx, 2, -4, -2, 0, types, 4, ref, 1140, ro, 1, read, 1025, qo, 1, &b, err, sizeof err);
    if (rc == SWMI_OK) { printf("ERROR xdrop without extend accepted\n"); return 10; }
    printf("refused %d\n", rc);
    swmi_destroy(ctx);
    return 0;
}
