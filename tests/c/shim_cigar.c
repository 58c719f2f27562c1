/* shim_cigar.c -- swmi_shim_set_cigar and swmi_shim_pair_cigar (bindings/jni/swmi_shim.h) from plain C99, as nativeSetCigar and
 * nativePairCigar call them.  Built and run by tests/test_cigar_shim_gpu.py (gcc -std=c99 -Wall -Wextra -Werror -pedantic).  One
 * global pair with match 2, mismatch -4, gap -2, gapOpen -4: the reference holds the read's 24 bases, one of them substituted, and
 * a stretch of 21 more.  For cigar = 2 and then 1 it prints one line: the pipeline mode, begin, the end cell, nm and the entries
 * as len:op; then "refused <status>" for a batch run with cigar = 0. */
#include <stdio.h>
#include <string.h>
#include "swmi.h"
#include "swmi_shim.h"

#define REF "GGCCCAGTCCAGCCCAACTAACGAATAAGTAGAATCCTCGGAAGT"
#define READ "GGCCTAGTCCAGATCCTCGGAAGT"

int main(void) {
    char err[640];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    const char *ref = REF, *read = READ;
    int64_t ro[2], qo[2];
    int c, rc;
    ro[0] = 0; ro[1] = (int64_t)strlen(ref); qo[0] = 0; qo[1] = (int64_t)strlen(read);
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_cigar(NULL, 2, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_cigar(ctx, 3, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR cigar 3 accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, -4, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    if (swmi_shim_set_align_mode(ctx, SWMI_ALIGN_GLOBAL, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
    for (c = 2; c >= 0; c--) {
        int32_t begin = 0, cell[2] = {0, 0};
        const uint32_t *cg = NULL;
        uint32_t n = 0, nm = 0, k;
        int mode = -1;
        if (swmi_shim_set_cigar(ctx, c, err, sizeof err) != SWMI_OK) { printf("ERROR %s\n", err); return 5; }
        if (swmi_shim_align_batch(ctx, 2, -4, -2, 0, types, 4, ref, ro[1], ro, 1, read, qo[1], qo, 1, &b, err, sizeof err) != SWMI_OK) {
            printf("ERROR %s\n", err); return 6;
        }
        rc = swmi_shim_pair_cigar(b, 0, 0, &begin, cell, &cg, &n, &nm, err, sizeof err);
        if (c == 0) {
            if (rc == SWMI_OK) { printf("ERROR a CIGAR after a run with cigar = 0\n"); return 10; }
            printf("refused %d\n", rc);
        } else {
            if (rc != SWMI_OK) { printf("ERROR %s\n", err); return 7; }
            if (swmi_shim_pair_cigar(b, -1, 0, NULL, NULL, NULL, NULL, NULL, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR pair -1 accepted\n"); return 8; }
            if (swmi_shim_pair_cigar(b, 0, 1, NULL, NULL, NULL, NULL, NULL, err, sizeof err) != SWMI_ERR_RANGE) { printf("ERROR alignment 1 accepted\n"); return 8; }
            if (swmi_batch_mode(b, &mode) != SWMI_OK) { printf("ERROR %s\n", swmi_last_error()); return 9; }
            printf("mode %d begin %d cell %d %d nm %u", mode, (int)begin, (int)cell[0], (int)cell[1], (unsigned)nm);
            for (k = 0; k < n; k++) printf(" %u:%u", (unsigned)(cg[k] >> 4), (unsigned)(cg[k] & 15u));
            printf("\n");
        }
        swmi_batch_free(ctx, b);
        b = NULL;
    }
    swmi_destroy(ctx);
    return 0;
}
