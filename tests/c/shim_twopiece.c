/* shim_twopiece.c -- swmi_shim_set_gap2 (bindings/jni/swmi_shim.h) from plain C99, as nativeSetGap2 calls it.
 * Built and run by tests/test_twopiece_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  One global pair, a reference of
 * 45 bases that holds the read's 24 and a stretch of 21 more, with match 2, mismatch -4, gap -2, gapOpen -4, gap2 -1, gapOpen2
 * -24: the deletion of 21 costs 24 + 21 = 45 under the second piece and 4 + 42 = 46 under the first, so the total is 48 - 45 = 3
 * with two-piece gaps and 2 without.  It prints the total, the number of match sites, the sites and the pipeline mode of the run
 * with and without the second piece, and then "refused <status>" for the second piece in fit mode. */
#include <stdio.h>
#include <string.h>
#include "swmi.h"
#include "swmi_shim.h"

#define REF "GGCCCAGTCCAGCCCAACTAACGAATAAGTAGAATCCTCGGAAGT"
#define READ "GGCCCAGTCCAGATCCTCGGAAGT"
#define READ_ALIGNED "GGCCCAGTCCAG_____________________ATCCTCGGAAGT"

int main(void) {
    char err[640];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    const char *ref = REF, *read = READ;
    int64_t ro[2], qo[2], n, k;
    int x, rc;
    ro[0] = 0; ro[1] = (int64_t)strlen(ref); qo[0] = 0; qo[1] = (int64_t)strlen(read);
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_gap2(NULL, -24, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_gap2(ctx, 1, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR gap_open2 1 accepted\n"); return 4; }
    if (swmi_shim_set_gap2(ctx, -24, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR gap2 1 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -4, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_GLOBAL, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (x = 1; x >= 0; x--) {
        int32_t total = 0;
        int mode = -1;
        if (swmi_shim_set_gap2(ctx, x ? -24 : 0, -1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_align_batch(ctx, 2, -4, -2, 0, types, 4, ref, ro[1], ro, 1, read, qo[1], qo, 1, &b, err, sizeof err) != SWMI_OK) {
            printf("ERROR %s\n", err); return 6;
        }
        n = 0;
        if (swmi_shim_ref_total(b, 0, &total, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
        if (swmi_shim_ref_site_count(b, 0, &n, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
        printf("%d %ld", (int)total, (long)n);
        for (k = 0; k < n; k++) {
            int32_t begin = 0; const char *ra = NULL, *qa = NULL; uint32_t len = 0;
            if (swmi_shim_ref_site(b, 0, k, &begin, &ra, &qa, &len, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 8; }
            if (strcmp(ra, REF) != 0 || strcmp(qa, READ_ALIGNED) != 0) { printf("ERROR %s/%s\n", ra, qa); return 8; }
            printf(" %d:%s/%s", (int)begin, ra, qa);
        }
        if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
        printf(" mode %d\n", mode);
        swmi_batch_free(ctx, b);
        b = NULL;
    }
    if (swmi_shim_set_gap2(ctx, -24, -1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_FIT, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    rc = swmi_shim_align_batch(ctx, 2, -4, -2, 0, types, 4, ref, ro[1], ro, 1, read, qo[1], qo, 1, &b, err, sizeof err);
    if (rc == SWMI_OK) { printf("ERROR two-piece gaps in fit mode accepted\n"); return 10; }
    printf("refused %d\n", rc);
    swmi_destroy(ctx);
    return 0;
}
