/* shim_pairs.c -- swmi_shim_align_pairs, swmi_shim_pair_results and swmi_shim_pair_alignment (bindings/jni/swmi_shim.h) from plain
 * C99, as nativeAlignPairs / nativePairResults / nativePairAlignment call them.  Built and run by tests/test_pairs_shim_gpu.py
 * (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  Two references of 400 and 150 bases and two reads of 120 and 60 bases from a
 * linear congruential generator (the reads: stretches of reference 0 in lower case, with a substitution every 17 bases); a dozen
 * pairs as int[8] each -- forward and reversed, one to the end of both sequences (-1 as a length), one with an empty read
 * segment.  Default scores, serial ties.  Prints one line per pair: the score, the number of alignments and
 * begin:row:column:refAligned/readAligned of every alignment; then "views <status>" of swmi_shim_ref_total on the pair list,
 * "ints <status>" for an array of 7 ints, and "bad <status> <1 if the message names pair 1>" for a list whose second pair runs
 * past its reference. */
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

#define N_PAIRS 12

int main(void) {
    static const int32_t specs[8 * N_PAIRS] = {
        0, 0,  30, 160,   0, 120, 0, 0,
        0, 0,  30, 160,   0, 120, 1, 0,
        0, 0,  57,  93,  11,  64, 0, 0,
        0, 0,  57,  93,  11,  64, 1, 0,
        0, 1, 200, 101,   3,  50, 0, 0,
        0, 1, 203,  -1,   1,  -1, 1, 0,
        0, 1, 190,  70,   0,   0, 0, 0,
        1, 0,   0, 150,  40,  33, 0, 0,
        0, 0,   1,   5,   1,   6, 0, 0,
        0, 1, 399,   1,  59,   1, 1, 0,
        0, 0,  30, 160,   0, 120, 0, 0,
        0, 0,  31, 160,   1, 119, 1, 0
    };
    char err[640], seqs[551], reads[181];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    int64_t ro[3], qo[3], counts[N_PAIRS], p, k;
    int32_t scores[N_PAIRS], bad[16], total = 0;
    int x, rc;
    lcg(1ul, seqs, 400); lcg(2ul, seqs + 400, 150); seqs[550] = 0;
    for (x = 0; x < 120; x++) reads[x] = (char)((x % 17 == 16 ? "TGCA"[x & 3] : seqs[40 + x]) | 0x20);
    for (x = 0; x < 60; x++) reads[120 + x] = (char)((x % 17 == 16 ? "TGCA"[x & 3] : seqs[210 + x]) | 0x20);
    reads[180] = 0;
    ro[0] = 0; ro[1] = 400; ro[2] = 550; qo[0] = 0; qo[1] = 120; qo[2] = 180;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_align_pairs(ctx, 5, -3, -4, 0, types, 4, seqs, 550, ro, 2, reads, 180, qo, 2, specs, 8 * N_PAIRS, &b, err, sizeof err) != SWMI_OK) {
        printf("ERROR %s\n", err); return 4;
    }
    if (swmi_shim_pair_results(b, scores, counts, N_PAIRS, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_pair_results(b, scores, counts, N_PAIRS - 1, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR 11 pairs accepted\n"); return 5; }
    for (p = 0; p < N_PAIRS; p++) {
        printf("%d %ld", (int)scores[p], (long)counts[p]);
        for (k = 0; k < counts[p]; k++) {
            int32_t begin = 0, cell[2] = {0, 0}; const char *ra = NULL, *qa = NULL; uint32_t len = 0;
            if (swmi_shim_pair_alignment(b, p, k, &begin, cell, &ra, &qa, &len, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 6; }
            if (strlen(ra) != len || strlen(qa) != len) { printf("ERROR string lengths\n"); return 6; }
            printf(" %d:%d:%d:%s/%s", (int)begin, (int)cell[0], (int)cell[1], ra, qa);
        }
        printf("\n");
    }
    if (swmi_shim_pair_alignment(b, N_PAIRS, 0, NULL, NULL, NULL, NULL, NULL, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR pair 12 accepted\n"); return 6; }
    rc = swmi_shim_ref_total(b, 0, &total, err, sizeof err);
    printf("views %d\n", rc);
    swmi_batch_free(ctx, b);
    b = NULL;
    rc = swmi_shim_align_pairs(ctx, 5, -3, -4, 0, types, 4, seqs, 550, ro, 2, reads, 180, qo, 2, specs, 7, &b, err, sizeof err);
    printf("ints %d\n", rc);
    memcpy(bad, specs, sizeof bad);
    bad[8 + 3] = 371;                                   /* pair 1: 30 + 371 > 400 */
    rc = swmi_shim_align_pairs(ctx, 5, -3, -4, 0, types, 4, seqs, 550, ro, 2, reads, 180, qo, 2, bad, 16, &b, err, sizeof err);
    printf("bad %d %d\n", rc, strstr(err, "pair 1") != NULL && b == NULL);
    swmi_destroy(ctx);
    return 0;
}
