/* shim_adapt.c -- swmi_shim_set_band_adapt (bindings/jni/swmi_shim.h) from plain C99, as nativeSetBandAdapt calls it.
 * Built and run by tests/test_adapt_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  The reference is 1300 bases of a
 * linear congruential generator (seed 1); the read is its first 1220 bases with 40 further bases (seeds 2 and 3) inserted after
 * bases 300 and 700: 1300 bases, two strips, and on row 1024 the alignment stands 80 columns left of the diagonal.  Match 2,
 * mismatch -4, gap -2, gapOpen -4, seed extension with long reads on, band 48: the static band loses the alignment in strip 1,
 * the adaptive band keeps it.  For band_adapt 1 and 0 it prints the total, the number of match sites, begin:length of every
 * site, the windows of both strips (swmi_pair_band_window) and the pipeline mode, then "range <status>" for strip 2 and
 * "refused <status>" for band_adapt 1 without a band. */
#include <stdio.h>
#include <string.h>
#include "swmi.h"
#include "swmi_shim.h"

static void lcg(unsigned long x, char *dst, int n) {
    int k;
    for (k = 0; k < n; k++) {
        x = (x * 1103515245ul + 12345ul) & 0x7FFFFFFFul;
        dst[k] = "ACGT"[(x >> 16) & 3ul];
    }
}

int main(void) {
    static const int32_t on[2] = {1, 0};
    char err[640], ref[1301], read[1301];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    int64_t ro[2], qo[2], n, k;
    uint32_t lo = 0, hi = 0;
    int x, rc;
    lcg(1ul, ref, 1300); ref[1300] = 0;
    memcpy(read, ref, 300); lcg(2ul, read + 300, 40);
    memcpy(read + 340, ref + 300, 400); lcg(3ul, read + 740, 40);
    memcpy(read + 780, ref + 700, 520); read[1300] = 0;
    ro[0] = 0; ro[1] = 1300; qo[0] = 0; qo[1] = 1300;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_band_adapt(NULL, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_band_adapt(ctx, 2, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR band_adapt 2 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -4, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_GLOBAL, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_long_reads(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_extend(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_band(ctx, 48, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (x = 0; x < 2; x++) {
        int32_t total = 0;
        int mode = -1;
        uint32_t s;
        if (swmi_shim_set_band_adapt(ctx, on[x], err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_align_batch(ctx, 2, -4, -2, 0, types, 4, ref, 1300, ro, 1, read, 1300, qo, 1, &b, err, sizeof err) != SWMI_OK) {
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
        printf(" windows");
        for (s = 0; s < 2; s++) {
            if (swmi_pair_band_window(b, 0, s, &lo, &hi) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
            printf(" %u-%u", (unsigned)lo, (unsigned)hi);
        }
        if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
        printf(" mode %d\n", mode);
        if (x == 1) printf("range %d\n", swmi_pair_band_window(b, 0, 2, &lo, &hi));
        swmi_batch_free(ctx, b);
        b = NULL;
    }
    if (swmi_shim_set_band_adapt(ctx, 1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_band(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    rc = swmi_shim_align_batch(ctx, 2, -4, -2, 0, types, 4, ref, 1300, ro, 1, read, 1300, qo, 1, &b, err, sizeof err);
    if (rc == SWMI_OK) { printf("ERROR band_adapt without a band accepted\n"); return 10; }
    printf("refused %d\n", rc);
    swmi_destroy(ctx);
    return 0;
}
