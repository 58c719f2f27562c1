/* shim_profile.c -- swmi_shim_set_read_profiles (bindings/jni/swmi_shim.h) from plain C99, as nativeSetReadProfiles calls it.
 * Built and run by tests/test_profile_shim_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  For ref GGACGTTCGAtt x read
 * ACGATCGA with match 2, mismatch -3, gap -1, gapOpen -3 in local mode it prints the total, the number of match sites, the sites and
 * the pipeline mode of the run without profiles, under a profile over ACGT that forgives a mismatch at read position 4, and with
 * the profiles cleared again; then "refused <status>" for a duplicate symbol, for a scores array of the wrong length and for a
 * run under option subopt. */
#include <stdio.h>
#include "swmi.h"
#include "swmi_shim.h"

static int show(swmi_batch *b, char *err, size_t err_len) {
    int32_t total = 0;
    int64_t n = 0, k;
    int mode = -1;
    if (swmi_shim_ref_total(b, 0, &total, err, err_len) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    if (swmi_shim_ref_site_count(b, 0, &n, err, err_len) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    printf("%d %ld", (int)total, (long)n);
    for (k = 0; k < n; k++) {
        int32_t begin = 0; const char *ra = NULL, *qa = NULL; uint32_t len = 0;
        if (swmi_shim_ref_site(b, 0, k, &begin, &ra, &qa, &len, err, err_len) != SWMI_OK) { printf("ERROR %s\n", err); return 8; }
        printf(" %d:%s/%s", (int)begin, ra, qa);
    }
    if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
    printf(" mode %d\n", mode);
    return 0;
}

int main(void) {
    char err[640];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    const signed char alphabet[4] = {'A', 'C', 'G', 'T'}, twice[4] = {'A', 'C', 'a', 'T'};
    const char *ref = "GGACGTTCGAtt", *read = "ACGATCGA";
    int32_t scores[32];
    int64_t ro[2], qo[2];
    int i, c, rc;
    ro[0] = 0; ro[1] = 12; qo[0] = 0; qo[1] = 8;
    /* row i: 2 in the column of the read's base, -3 elsewhere; position 4 (the A against the reference's T) costs nothing anywhere */
    for (i = 0; i < 8; i++)
        for (c = 0; c < 4; c++) scores[4 * i + c] = i == 3 ? 0 : (read[i] == (char)alphabet[c] ? 2 : -3);
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_gap_open(ctx, -3, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_align_batch(ctx, 2, -3, -1, 0, types, 4, ref, 12, ro, 1, read, 8, qo, 1, &b, err, sizeof err) != SWMI_OK) {
        printf("ERROR %s\n", err); return 6;
    }
    if ((rc = show(b, err, sizeof err))) return rc;
    if (swmi_shim_set_read_profiles(NULL, b, 2, -3, -1, 0, types, 4, alphabet, 4, scores, 32, 8, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_read_profiles(ctx, NULL, 2, -3, -1, 0, types, 4, alphabet, 4, scores, 32, 8, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null batch accepted\n"); return 4; }
    if (swmi_shim_set_read_profiles(ctx, b, 2, -3, -1, 0, types, 4, alphabet, 4, scores, 32, 8, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 6; }
    if ((rc = show(b, err, sizeof err))) return rc;
    if (swmi_shim_set_read_profiles(ctx, b, 2, -3, -1, 0, types, 4, NULL, 0, NULL, 0, 8, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 6; }
    if ((rc = show(b, err, sizeof err))) return rc;
    rc = swmi_shim_set_read_profiles(ctx, b, 2, -3, -1, 0, types, 4, twice, 4, scores, 32, 8, err, sizeof err);
    printf("refused %d\n", rc);
    rc = swmi_shim_set_read_profiles(ctx, b, 2, -3, -1, 0, types, 4, alphabet, 4, scores, 28, 8, err, sizeof err);
    printf("refused %d\n", rc);
    if ((rc = show(b, err, sizeof err))) return rc;          /* a refused set leaves the batch as it was, results included */
    if (swmi_shim_set_subopt(ctx, 5, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    rc = swmi_shim_set_read_profiles(ctx, b, 2, -3, -1, 0, types, 4, alphabet, 4, scores, 32, 8, err, sizeof err);
    printf("refused %d\n", rc);
    swmi_batch_free(ctx, b);
    swmi_destroy(ctx);
    return 0;
}
