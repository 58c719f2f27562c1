/* shim_matrix.c -- swmi_shim_set_score_matrix (bindings/jni/swmi_shim.h) from plain C99, as nativeSetScoreMatrix calls it.
 * Built and run by tests/test_matrix_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  Prints the total and the match
 * sites of ref CAGCA x read ACAG under the asymmetric matrix {A, C} = {{2, 5}, {-3, 2}} (row = read) with match 1, mismatch -1,
 * gap -2, gapOpen -1, then "cleared" and the pipeline mode of a run after the matrix is cleared and gapOpen reset. */
#include <stdio.h>
#include "swmi.h"
#include "swmi_shim.h"

int main(void) {
    char err[640];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    const signed char alpha[2] = {'A', 'C'}, dup[2] = {'A', 'a'};
    const int32_t scores[4] = {2, 5, -3, 2}, big[4] = {0, 0, 0, (1 << 20) + 1};
    const char *ref = "CAGCA", *read = "ACAG";
    int64_t ro[2], qo[2], n = 0, k;
    int32_t total = 0;
    int mode = -1;
    ro[0] = 0; ro[1] = 5; qo[0] = 0; qo[1] = 4;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_score_matrix(NULL, alpha, 2, scores, 4, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context\n"); return 4; }
    if (swmi_shim_set_score_matrix(ctx, alpha, 2, scores, 3, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR short scores\n"); return 4; }
    if (swmi_shim_set_score_matrix(ctx, dup, 2, scores, 4, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR duplicate\n"); return 4; }
    if (swmi_shim_set_score_matrix(ctx, alpha, 2, big, 4, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR |entry|\n"); return 4; }
    if (swmi_shim_set_score_matrix(ctx, alpha, 2, scores, 4, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_gap_open(ctx, -1, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_align_batch(ctx, 1, -1, -2, 0, types, 4, ref, 5, ro, 1, read, 4, qo, 1, &b, err, sizeof err) != SWMI_OK) {
        printf("ERROR %s\n", err); return 6;
    }
    if (swmi_shim_ref_total(b, 0, &total, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    if (swmi_shim_ref_site_count(b, 0, &n, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
    printf("%d %ld", (int)total, (long)n);
    for (k = 0; k < n; k++) {
        int32_t begin = 0; const char *ra = NULL, *qa = NULL; uint32_t len = 0;
        if (swmi_shim_ref_site(b, 0, k, &begin, &ra, &qa, &len, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 8; }
        printf(" %d:%s/%s", (int)begin, ra, qa);
    }
    swmi_batch_free(ctx, b);
    b = NULL;
    if (swmi_shim_set_score_matrix(ctx, NULL, 0, NULL, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 9; }
    if (swmi_shim_set_gap_open(ctx, 0, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 9; }
    if (swmi_shim_align_batch(ctx, 1, -1, -2, 0, types, 4, ref, 5, ro, 1, read, 4, qo, 1, &b, err, sizeof err) != SWMI_OK) {
        printf("ERROR %s\n", err); return 10;
    }
    if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 11; }
    printf(" cleared %d\n", mode);
    swmi_batch_free(ctx, b);
    swmi_destroy(ctx);
    return 0;
}
