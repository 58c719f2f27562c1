/* shim_strand.c -- the minus strand through the JNI shim (bindings/jni/swmi_shim.h) from plain C99: swmi_shim_align_pairs passes
 * swmi_pair_spec.flags through as given, SWMI_SPEC_READ_REVCOMP (4) included.  Built and run by tests/test_strand_shim_gpu.py
 * (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  The sequences and the twelve pairs of shim_pairs.c, except that read 1 is the
 * REVERSE COMPLEMENT of its stretch of reference 0 (lower case, a substitution every 17 bases) and that half of the pairs carry
 * flags 4 or 5.  Default scores, serial ties.  Prints one line per pair: the score, the number of alignments and
 * begin:row:column:refAligned/readAligned of every alignment; then "flag2 <status> <1 if the message names pair 1>" for a list
 * whose second pair has the undefined flag bit 2. */
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

static char complement(char c) {
    switch (c) {
        case 'A': return 'T';
        case 'C': return 'G';
        case 'G': return 'C';
        default:  return 'A';
    }
}

#define N_PAIRS 12

int main(void) {
    static const int32_t specs[8 * N_PAIRS] = {
        0, 0,  30, 160,   0, 120, 0, 0,
        0, 0,  30, 160,   0, 120, 1, 0,
        0, 0,  57,  93,  11,  64, 4, 0,
        0, 0,  57,  93,  11,  64, 5, 0,
        0, 1, 200, 101,   3,  50, 4, 0,
        0, 1, 203,  -1,   1,  -1, 5, 0,
        0, 1, 190,  70,   0,   0, 0, 0,
        1, 0,   0, 150,  40,  33, 0, 0,
        0, 0,   1,   5,   1,   6, 4, 0,
        0, 1, 399,   1,  59,   1, 5, 0,
        0, 1, 200, 101,   3,  50, 0, 0,
        0, 1, 201, 100,   0,  60, SWMI_SPEC_REVERSE | SWMI_SPEC_READ_REVCOMP, 0
    };
    char err[640], seqs[551], reads[181];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    int64_t ro[3], qo[3], counts[N_PAIRS], p, k;
    int32_t scores[N_PAIRS], bad[16];
    int x, rc;
    lcg(1ul, seqs, 400); lcg(2ul, seqs + 400, 150); seqs[550] = 0;
    for (x = 0; x < 120; x++) reads[x] = (char)((x % 17 == 16 ? "TGCA"[x & 3] : seqs[40 + x]) | 0x20);
    for (x = 0; x < 60; x++) reads[120 + x] = (char)((x % 17 == 16 ? "TGCA"[x & 3] : complement(seqs[210 + 59 - x])) | 0x20);
    reads[180] = 0;
    ro[0] = 0; ro[1] = 400; ro[2] = 550; qo[0] = 0; qo[1] = 120; qo[2] = 180;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_align_pairs(ctx, 5, -3, -4, 0, types, 4, seqs, 550, ro, 2, reads, 180, qo, 2, specs, 8 * N_PAIRS, &b, err, sizeof err) != SWMI_OK) {
        printf("ERROR %s\n", err); return 4;
    }
    if (swmi_shim_pair_results(b, scores, counts, N_PAIRS, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
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
    swmi_batch_free(ctx, b);
    b = NULL;
    memcpy(bad, specs, sizeof bad);
    bad[8 + 6] = 2;                                     /* pair 1: the undefined flag bit */
    rc = swmi_shim_align_pairs(ctx, 5, -3, -4, 0, types, 4, seqs, 550, ro, 2, reads, 180, qo, 2, bad, 16, &b, err, sizeof err);
    printf("flag2 %d %d\n", rc, strstr(err, "pair 1") != NULL && b == NULL);
    swmi_destroy(ctx);
    return 0;
}
