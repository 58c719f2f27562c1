/*
 * swmi_jni.c -- thin JNI shim over include/swmi.h for the Java class sw.GpuSmithWaterman
 * (bindings/java/sw/GpuSmithWaterman.java).  It only unwraps JNI types and forwards to swmi_shim.c, which holds the
 * argument checks and the C-ABI call sequence in JNI-free C99 (that part IS compiled and run by this repository's
 * tests: tests/c/shim_kat.c).  This file is NOT compiled in this repository's build: the build image has no JDK (no
 * jni.h).  On a machine with a JDK:
 *     gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude -Ibindings/jni \
 *         bindings/jni/swmi_jni.c bindings/jni/swmi_shim.c -Lsparksmithwaterman_amd/lib -lswmi -o libswmi_jni.so
 *
 * Replaces the per-pair call  new SmithWaterman.OptAlignments().call(seqs, alignScores, alignTypes)
 * at src/sw/Distribution.java:421-422 by ONE native call per partition (per-pair JNI calls would
 * drown in call overhead).
 */
#include <jni.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "swmi.h"
#include "swmi_shim.h"

static void throw_msg(JNIEnv *env, const char *msg) {
    jclass cls = (*env)->FindClass(env, "java/lang/RuntimeException");
    if (cls) (*env)->ThrowNew(env, cls, msg);
}

static void throw_rt(JNIEnv *env, const char *where) {
    char buf[640];
    snprintf(buf, sizeof buf, "%s: %s", where, swmi_last_error());
    throw_msg(env, buf);
}

JNIEXPORT jlong JNICALL Java_sw_GpuSmithWaterman_nativeCreate(JNIEnv *env, jclass cls, jint device) {
    swmi_ctx *ctx = NULL;
    (void)cls;
    if (swmi_create(device, &ctx) != SWMI_OK) { throw_rt(env, "swmi_create"); return 0; }
    return (jlong)(intptr_t)ctx;
}

JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeDestroy(JNIEnv *env, jclass cls, jlong ctx) {
    (void)env; (void)cls;
    swmi_destroy((swmi_ctx *)(intptr_t)ctx);
}

/* affine gaps on this context from now on: a gap of length k costs gapOpen + k * gap (0: linear) */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetGapOpen(JNIEnv *env, jclass cls, jlong ctx, jint gapOpen) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_gap_open((swmi_ctx *)(intptr_t)ctx, gapOpen, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* end-to-end alignment on this context from now on: 0 local, 1 fit (the whole read), 2 global (the whole read and reference) */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetAlignMode(JNIEnv *env, jclass cls, jlong ctx, jint alignMode) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_align_mode((swmi_ctx *)(intptr_t)ctx, alignMode, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* reads longer than 1024 bases on the affine kernels from now on: 1 allowed, 0 refused */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetLongReads(JNIEnv *env, jclass cls, jlong ctx, jint longReads) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_long_reads((swmi_ctx *)(intptr_t)ctx, longReads, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* a band of this half-width around the diagonal for reads longer than 1024 bases from now on, 0: none */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetBand(JNIEnv *env, jclass cls, jlong ctx, jint band) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_band((swmi_ctx *)(intptr_t)ctx, band, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* seed extension on this context from now on (with align mode global): 1 on, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetExtend(JNIEnv *env, jclass cls, jlong ctx, jint extend) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_extend((swmi_ctx *)(intptr_t)ctx, extend, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* the drop-off threshold of seed extension on this context from now on, 0: off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetXdrop(JNIEnv *env, jclass cls, jlong ctx, jint xdrop) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_xdrop((swmi_ctx *)(intptr_t)ctx, xdrop, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* the band of a banded extend run follows the alignment on this context from now on: 1 on, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetBandAdapt(JNIEnv *env, jclass cls, jlong ctx, jint band_adapt) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_band_adapt((swmi_ctx *)(intptr_t)ctx, band_adapt, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* alignments as CIGARs on this context from now on: 1 M/I/D, 2 =/X/I/D, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetCigar(JNIEnv *env, jclass cls, jlong ctx, jint cigar) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_cigar((swmi_ctx *)(intptr_t)ctx, cigar, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* the second-best score on this context from now on: the mask half-width, -1 automatic, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetSubopt(JNIEnv *env, jclass cls, jlong ctx, jint subopt) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_subopt((swmi_ctx *)(intptr_t)ctx, subopt, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* { second-best score, the reference column it ends in } of a pair after a run under option "subopt" */
JNIEXPORT jintArray JNICALL Java_sw_GpuSmithWaterman_nativePairSubopt(JNIEnv *env, jclass cls, jlong batch, jlong pair) {
    char err[640];
    int32_t out[2] = {0, 0};
    jint jo[2];
    jintArray res;
    (void)cls;
    if (swmi_shim_pair_subopt((const swmi_batch *)(intptr_t)batch, pair, out, err, sizeof err) != SWMI_OK) {
        throw_msg(env, err);
        return NULL;
    }
    res = (*env)->NewIntArray(env, 2);
    if (!res) return NULL;
    jo[0] = out[0]; jo[1] = out[1];
    (*env)->SetIntArrayRegion(env, res, 0, 2, jo);
    return res;
}

/* the end bonus of extend runs on this context from now on: 1 .. 2^30 the bonus, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetEndBonus(JNIEnv *env, jclass cls, jlong ctx, jint end_bonus) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_end_bonus((swmi_ctx *)(intptr_t)ctx, end_bonus, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* overlap alignment on this context from now on (with align mode fit): 1 on, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetOverlap(JNIEnv *env, jclass cls, jlong ctx, jint overlap) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_overlap((swmi_ctx *)(intptr_t)ctx, overlap, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* { max_score, end_score, end_col, taken to the end ? 1 : 0 } of a pair after a run under option "end_bonus" */
JNIEXPORT jintArray JNICALL Java_sw_GpuSmithWaterman_nativePairEndScore(JNIEnv *env, jclass cls, jlong batch, jlong pair) {
    char err[640];
    int32_t out[4] = {0, 0, 0, 0};
    jint jo[4];
    jintArray res;
    (void)cls;
    if (swmi_shim_pair_end_score((const swmi_batch *)(intptr_t)batch, pair, out, err, sizeof err) != SWMI_OK) {
        throw_msg(env, err);
        return NULL;
    }
    res = (*env)->NewIntArray(env, 4);
    if (!res) return NULL;
    jo[0] = out[0]; jo[1] = out[1]; jo[2] = out[2]; jo[3] = out[3];
    (*env)->SetIntArrayRegion(env, res, 0, 4, jo);
    return res;
}

/* the best local hits on this context from now on: the most entries per pair, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetHits(JNIEnv *env, jclass cls, jlong ctx, jint hits) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_hits((swmi_ctx *)(intptr_t)ctx, hits, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* { score, read row, reference column } x the pair's hits after a run under option "hits" */
JNIEXPORT jintArray JNICALL Java_sw_GpuSmithWaterman_nativePairHits(JNIEnv *env, jclass cls, jlong batch, jlong pair) {
    char err[640];
    int32_t out[3 * 16];
    int32_t n = 0;
    jint jo[3 * 16];
    jintArray res;
    int k;
    (void)cls;
    if (swmi_shim_pair_hits((const swmi_batch *)(intptr_t)batch, pair, out, 16, &n, err, sizeof err) != SWMI_OK) {
        throw_msg(env, err);
        return NULL;
    }
    res = (*env)->NewIntArray(env, 3 * n);
    if (!res) return NULL;
    for (k = 0; k < 3 * n; k++) jo[k] = out[k];
    (*env)->SetIntArrayRegion(env, res, 0, 3 * n, jo);
    return res;
}

/* two-piece gaps on this context from now on: gapOpen2 != 0 on, 0 off */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetGap2(JNIEnv *env, jclass cls, jlong ctx, jint gap_open2, jint gap2) {
    char err[640];
    (void)cls;
    if (swmi_shim_set_gap2((swmi_ctx *)(intptr_t)ctx, gap_open2, gap2, err, sizeof err) != SWMI_OK) throw_msg(env, err);
}

/* a substitution score matrix on this context from now on: alphabet = n ISO-8859-1 symbols, scores = int[n * n], row = read base;
 * alphabet == null clears it */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetScoreMatrix(JNIEnv *env, jclass cls, jlong ctx, jbyteArray alphabet,
                                                                     jintArray scores) {
    char err[640];
    jbyte *a = NULL;
    jint *sc = NULL;
    jsize n = 0, ns = 0;
    int rc;
    (void)cls;
    if (alphabet) {
        if (!scores) { throw_msg(env, "nativeSetScoreMatrix: scores is null"); return; }
        n = (*env)->GetArrayLength(env, alphabet);
        ns = (*env)->GetArrayLength(env, scores);
        a = (*env)->GetByteArrayElements(env, alphabet, NULL);
        sc = (*env)->GetIntArrayElements(env, scores, NULL);
        if (!a || !sc) {
            if (a) (*env)->ReleaseByteArrayElements(env, alphabet, a, JNI_ABORT);
            if (sc) (*env)->ReleaseIntArrayElements(env, scores, sc, JNI_ABORT);
            return;                                                   /* (OutOfMemoryError pending) */
        }
    }
    rc = swmi_shim_set_score_matrix((swmi_ctx *)(intptr_t)ctx, (const signed char *)a, (size_t)n, (const int32_t *)sc, (size_t)ns,
                                    err, sizeof err);
    if (a) (*env)->ReleaseByteArrayElements(env, alphabet, a, JNI_ABORT);
    if (sc) (*env)->ReleaseIntArrayElements(env, scores, sc, JNI_ABORT);
    if (rc != SWMI_OK) throw_msg(env, err);
}

/* per-read score profiles on a batch of nativeAlignBatch, and the batch run again under them: alphabet = n ISO-8859-1 symbols,
 * scores = int[n * nRows], n entries per read byte in upload order; alphabet == null clears them */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeSetReadProfiles(JNIEnv *env, jclass cls, jlong ctx, jlong batch, jint match,
                                                                      jint mismatch, jint gap, jint tieMode, jbyteArray types,
                                                                      jbyteArray alphabet, jintArray scores, jlong nRows) {
    char err[640];
    jbyte ty[4] = {0, 0, 0, 0};
    jbyte *a = NULL;
    jint *sc = NULL;
    jsize ty_len, n = 0, ns = 0;
    int rc;
    (void)cls;
    if (!types) { throw_msg(env, "nativeSetReadProfiles: types is null"); return; }
    ty_len = (*env)->GetArrayLength(env, types);
    if (ty_len == 4) (*env)->GetByteArrayRegion(env, types, 0, 4, ty);
    if (alphabet) {
        if (!scores) { throw_msg(env, "nativeSetReadProfiles: scores is null"); return; }
        n = (*env)->GetArrayLength(env, alphabet);
        ns = (*env)->GetArrayLength(env, scores);
        a = (*env)->GetByteArrayElements(env, alphabet, NULL);
        sc = (*env)->GetIntArrayElements(env, scores, NULL);
        if (!a || !sc) {
            if (a) (*env)->ReleaseByteArrayElements(env, alphabet, a, JNI_ABORT);
            if (sc) (*env)->ReleaseIntArrayElements(env, scores, sc, JNI_ABORT);
            return;                                                   /* (OutOfMemoryError pending) */
        }
    }
    rc = swmi_shim_set_read_profiles((swmi_ctx *)(intptr_t)ctx, (swmi_batch *)(intptr_t)batch, match, mismatch, gap, tieMode,
                                     (const signed char *)ty, (size_t)ty_len, (const signed char *)a, (size_t)n, (const int32_t *)sc,
                                     (size_t)ns, (int64_t)nRows, err, sizeof err);
    if (a) (*env)->ReleaseByteArrayElements(env, alphabet, a, JNI_ABORT);
    if (sc) (*env)->ReleaseIntArrayElements(env, scores, sc, JNI_ABORT);
    if (rc != SWMI_OK) throw_msg(env, err);
}

/* refBytes/readBytes: direct ByteBuffers of ISO-8859-1 bytes; refOff/readOff: long[n+1] */
JNIEXPORT jlong JNICALL Java_sw_GpuSmithWaterman_nativeAlignBatch(
        JNIEnv *env, jclass cls, jlong ctx, jint match, jint mismatch, jint gap, jint tieMode, jbyteArray types,
        jobject refBytes, jlongArray refOff, jint nRefs, jobject readBytes, jlongArray readOff, jint nReads) {
    char err[640];
    jbyte ty[4] = {0, 0, 0, 0};
    jsize ty_len;
    jlong *ro, *qo;
    swmi_batch *b = NULL;
    int rc;
    (void)cls;
    if (!types || !refOff || !readOff) { throw_msg(env, "nativeAlignBatch: null array argument"); return 0; }
    ty_len = (*env)->GetArrayLength(env, types);
    if (ty_len == 4) (*env)->GetByteArrayRegion(env, types, 0, 4, ty);
    if ((*env)->GetArrayLength(env, refOff) != (jsize)nRefs + 1 || (*env)->GetArrayLength(env, readOff) != (jsize)nReads + 1) {
        throw_msg(env, "nativeAlignBatch: an offset array does not have n + 1 entries");
        return 0;
    }
    ro = (*env)->GetLongArrayElements(env, refOff, NULL);
    qo = (*env)->GetLongArrayElements(env, readOff, NULL);
    if (!ro || !qo) {
        if (ro) (*env)->ReleaseLongArrayElements(env, refOff, ro, JNI_ABORT);
        if (qo) (*env)->ReleaseLongArrayElements(env, readOff, qo, JNI_ABORT);
        throw_msg(env, "nativeAlignBatch: out of memory pinning the offset arrays");
        return 0;
    }
    rc = swmi_shim_align_batch((swmi_ctx *)(intptr_t)ctx, match, mismatch, gap, tieMode, (const signed char *)ty, (size_t)ty_len,
                               refBytes ? (*env)->GetDirectBufferAddress(env, refBytes) : NULL,
                               refBytes ? (int64_t)(*env)->GetDirectBufferCapacity(env, refBytes) : 0, (const int64_t *)ro, nRefs,
                               readBytes ? (*env)->GetDirectBufferAddress(env, readBytes) : NULL,
                               readBytes ? (int64_t)(*env)->GetDirectBufferCapacity(env, readBytes) : 0, (const int64_t *)qo, nReads,
                               &b, err, sizeof err);
    (*env)->ReleaseLongArrayElements(env, refOff, ro, JNI_ABORT);
    (*env)->ReleaseLongArrayElements(env, readOff, qo, JNI_ABORT);
    if (rc != SWMI_OK) { throw_msg(env, err); return 0; }
    return (jlong)(intptr_t)b;
}

/* a pair list over the sequences: specs = int[8 * nPairs], eight ints per pair as in swmi_pair_spec (swmi_shim.h) */
JNIEXPORT jlong JNICALL Java_sw_GpuSmithWaterman_nativeAlignPairs(
        JNIEnv *env, jclass cls, jlong ctx, jint match, jint mismatch, jint gap, jint tieMode, jbyteArray types,
        jobject refBytes, jlongArray refOff, jint nRefs, jobject readBytes, jlongArray readOff, jint nReads, jintArray specs) {
    char err[640];
    jbyte ty[4] = {0, 0, 0, 0};
    jsize ty_len;
    jlong *ro, *qo;
    jint *sp;
    swmi_batch *b = NULL;
    int rc;
    (void)cls;
    if (!types || !refOff || !readOff || !specs) { throw_msg(env, "nativeAlignPairs: null array argument"); return 0; }
    ty_len = (*env)->GetArrayLength(env, types);
    if (ty_len == 4) (*env)->GetByteArrayRegion(env, types, 0, 4, ty);
    if ((*env)->GetArrayLength(env, refOff) != (jsize)nRefs + 1 || (*env)->GetArrayLength(env, readOff) != (jsize)nReads + 1) {
        throw_msg(env, "nativeAlignPairs: an offset array does not have n + 1 entries");
        return 0;
    }
    ro = (*env)->GetLongArrayElements(env, refOff, NULL);
    qo = (*env)->GetLongArrayElements(env, readOff, NULL);
    sp = (*env)->GetIntArrayElements(env, specs, NULL);
    if (!ro || !qo || !sp) {
        if (ro) (*env)->ReleaseLongArrayElements(env, refOff, ro, JNI_ABORT);
        if (qo) (*env)->ReleaseLongArrayElements(env, readOff, qo, JNI_ABORT);
        if (sp) (*env)->ReleaseIntArrayElements(env, specs, sp, JNI_ABORT);
        throw_msg(env, "nativeAlignPairs: out of memory pinning the arrays");
        return 0;
    }
    rc = swmi_shim_align_pairs((swmi_ctx *)(intptr_t)ctx, match, mismatch, gap, tieMode, (const signed char *)ty, (size_t)ty_len,
                               refBytes ? (*env)->GetDirectBufferAddress(env, refBytes) : NULL,
                               refBytes ? (int64_t)(*env)->GetDirectBufferCapacity(env, refBytes) : 0, (const int64_t *)ro, nRefs,
                               readBytes ? (*env)->GetDirectBufferAddress(env, readBytes) : NULL,
                               readBytes ? (int64_t)(*env)->GetDirectBufferCapacity(env, readBytes) : 0, (const int64_t *)qo, nReads,
                               (const int32_t *)sp, (int64_t)(*env)->GetArrayLength(env, specs), &b, err, sizeof err);
    (*env)->ReleaseLongArrayElements(env, refOff, ro, JNI_ABORT);
    (*env)->ReleaseLongArrayElements(env, readOff, qo, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, specs, sp, JNI_ABORT);
    if (rc != SWMI_OK) { throw_msg(env, err); return 0; }
    return (jlong)(intptr_t)b;
}

/* every pair's score and number of alignments into the caller's arrays (both as long as the batch has pairs) */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativePairResults(JNIEnv *env, jclass cls, jlong batch, jintArray scores, jlongArray counts) {
    char err[640];
    jint *sc;
    jlong *ct;
    int rc = SWMI_ERR_NOMEM;
    (void)cls;
    if (!scores || !counts) { throw_msg(env, "nativePairResults: null array argument"); return; }
    if ((*env)->GetArrayLength(env, scores) != (*env)->GetArrayLength(env, counts)) { throw_msg(env, "nativePairResults: the arrays differ in length"); return; }
    sc = (*env)->GetIntArrayElements(env, scores, NULL);
    ct = (*env)->GetLongArrayElements(env, counts, NULL);
    if (sc && ct)
        rc = swmi_shim_pair_results((swmi_batch *)(intptr_t)batch, (int32_t *)sc, (int64_t *)ct, (int64_t)(*env)->GetArrayLength(env, scores), err, sizeof err);
    else
        snprintf(err, sizeof err, "nativePairResults: out of memory pinning the output arrays");
    if (sc) (*env)->ReleaseIntArrayElements(env, scores, sc, 0);
    if (ct) (*env)->ReleaseLongArrayElements(env, counts, ct, 0);
    if (rc != SWMI_OK) throw_msg(env, err);
}

/* alignment k of a pair: fills info[0..2] = {begin, last row, last column} and returns {refAligned, readAligned} as ISO-8859-1 bytes */
JNIEXPORT jobjectArray JNICALL Java_sw_GpuSmithWaterman_nativePairAlignment(JNIEnv *env, jclass cls, jlong batch, jlong pair, jlong k, jintArray info) {
    char err[640];
    int32_t b = 0, cell[2] = {0, 0}; const char *r = NULL, *q = NULL; uint32_t len = 0;
    jint ji[3];
    jobjectArray out;
    jbyteArray ra, qa;
    jclass bytes_cls;
    (void)cls;
    if (swmi_shim_pair_alignment((swmi_batch *)(intptr_t)batch, pair, k, &b, cell, &r, &q, &len, err, sizeof err) != SWMI_OK) {
        throw_msg(env, err);
        return NULL;
    }
    ji[0] = b; ji[1] = cell[0]; ji[2] = cell[1];
    if (info && (*env)->GetArrayLength(env, info) >= 3) (*env)->SetIntArrayRegion(env, info, 0, 3, ji);
    bytes_cls = (*env)->FindClass(env, "[B");
    if (!bytes_cls) return NULL;
    out = (*env)->NewObjectArray(env, 2, bytes_cls, NULL);
    ra = (*env)->NewByteArray(env, (jsize)len);
    qa = (*env)->NewByteArray(env, (jsize)len);
    if (!out || !ra || !qa) return NULL;                     /* OutOfMemoryError is already pending */
    (*env)->SetByteArrayRegion(env, ra, 0, (jsize)len, (const jbyte *)r);
    (*env)->SetByteArrayRegion(env, qa, 0, (jsize)len, (const jbyte *)q);
    (*env)->SetObjectArrayElement(env, out, 0, ra);
    (*env)->SetObjectArrayElement(env, out, 1, qa);
    return out;
}

/* alignment k of a pair after a run under option "cigar": fills info[0..2] = {begin, last row, last column} and returns the entries
 * len << 4 | op, first entry = start of the alignment */
JNIEXPORT jintArray JNICALL Java_sw_GpuSmithWaterman_nativePairCigar(JNIEnv *env, jclass cls, jlong batch, jlong pair, jlong k, jintArray info) {
    char err[640];
    int32_t b = 0, cell[2] = {0, 0}; const uint32_t *cg = NULL; uint32_t n = 0, nm = 0;
    jint ji[3];
    jintArray out;
    (void)cls;
    if (swmi_shim_pair_cigar((swmi_batch *)(intptr_t)batch, pair, k, &b, cell, &cg, &n, &nm, err, sizeof err) != SWMI_OK) {
        throw_msg(env, err);
        return NULL;
    }
    ji[0] = b; ji[1] = cell[0]; ji[2] = cell[1];
    if (info && (*env)->GetArrayLength(env, info) >= 3) (*env)->SetIntArrayRegion(env, info, 0, 3, ji);
    out = (*env)->NewIntArray(env, (jsize)n);
    if (!out) return NULL;                                   /* OutOfMemoryError is already pending */
    if (n) (*env)->SetIntArrayRegion(env, out, 0, (jsize)n, (const jint *)(const void *)cg);
    return out;
}

/* ... and its edit distance (SAM's NM) */
JNIEXPORT jint JNICALL Java_sw_GpuSmithWaterman_nativePairNm(JNIEnv *env, jclass cls, jlong batch, jlong pair, jlong k) {
    char err[640];
    uint32_t nm = 0;
    (void)cls;
    if (swmi_shim_pair_cigar((swmi_batch *)(intptr_t)batch, pair, k, NULL, NULL, NULL, NULL, &nm, err, sizeof err) != SWMI_OK) {
        throw_msg(env, err);
        return 0;
    }
    return (jint)nm;
}

JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeFreeBatch(JNIEnv *env, jclass cls, jlong ctx, jlong batch) {
    (void)env; (void)cls;
    swmi_batch_free((swmi_ctx *)(intptr_t)ctx, (swmi_batch *)(intptr_t)batch);
}

JNIEXPORT jint JNICALL Java_sw_GpuSmithWaterman_nativeRefTotal(JNIEnv *env, jclass cls, jlong batch, jint ref) {
    char err[640];
    int32_t t = 0;
    (void)cls;
    if (swmi_shim_ref_total((swmi_batch *)(intptr_t)batch, ref, &t, err, sizeof err) != SWMI_OK) throw_msg(env, err);
    return t;
}

JNIEXPORT jlong JNICALL Java_sw_GpuSmithWaterman_nativeRefSiteCount(JNIEnv *env, jclass cls, jlong batch, jint ref) {
    char err[640];
    int64_t n = 0;
    (void)cls;
    if (swmi_shim_ref_site_count((swmi_batch *)(intptr_t)batch, ref, &n, err, sizeof err) != SWMI_OK) throw_msg(env, err);
    return (jlong)n;
}

/* fills begin[0] and returns {refAligned, readAligned} as ISO-8859-1 byte arrays */
JNIEXPORT jobjectArray JNICALL Java_sw_GpuSmithWaterman_nativeRefSite(JNIEnv *env, jclass cls, jlong batch, jint ref, jlong k, jintArray begin) {
    char err[640];
    int32_t b = 0; const char *r = NULL, *q = NULL; uint32_t len = 0;
    jint jb;
    jobjectArray out;
    jbyteArray ra, qa;
    jclass bytes_cls;
    (void)cls;
    if (swmi_shim_ref_site((swmi_batch *)(intptr_t)batch, ref, k, &b, &r, &q, &len, err, sizeof err) != SWMI_OK) {
        throw_msg(env, err);
        return NULL;
    }
    jb = b;
    if (begin && (*env)->GetArrayLength(env, begin) >= 1) (*env)->SetIntArrayRegion(env, begin, 0, 1, &jb);
    bytes_cls = (*env)->FindClass(env, "[B");
    if (!bytes_cls) return NULL;
    out = (*env)->NewObjectArray(env, 2, bytes_cls, NULL);
    ra = (*env)->NewByteArray(env, (jsize)len);
    qa = (*env)->NewByteArray(env, (jsize)len);
    if (!out || !ra || !qa) return NULL;                     /* OutOfMemoryError is already pending */
    (*env)->SetByteArrayRegion(env, ra, 0, (jsize)len, (const jbyte *)r);
    (*env)->SetByteArrayRegion(env, qa, 0, (jsize)len, (const jbyte *)q);
    (*env)->SetObjectArrayElement(env, out, 0, ra);
    (*env)->SetObjectArrayElement(env, out, 1, qa);
    return out;
}

/* {number of match sites, bytes of all their strings} of the references refLo .. refHi-1 */
JNIEXPORT jlongArray JNICALL Java_sw_GpuSmithWaterman_nativeRefSitesSizes(JNIEnv *env, jclass cls, jlong batch, jint refLo, jint refHi) {
    char err[640];
    int64_t sz[2] = {0, 0};
    jlong jsz[2];
    jlongArray out;
    (void)cls;
    if (swmi_shim_ref_sites_sizes((swmi_batch *)(intptr_t)batch, refLo, refHi, sz, err, sizeof err) != SWMI_OK) { throw_msg(env, err); return NULL; }
    out = (*env)->NewLongArray(env, 2);
    if (!out) return NULL;
    jsz[0] = (jlong)sz[0]; jsz[1] = (jlong)sz[1];
    (*env)->SetLongArrayRegion(env, out, 0, 2, jsz);
    return out;
}

/* MapRef's output of a whole range of references into the caller's arrays: ONE call per partition (swmi_shim.h) */
JNIEXPORT void JNICALL Java_sw_GpuSmithWaterman_nativeRefSitesPacked(
        JNIEnv *env, jclass cls, jlong batch, jint refLo, jint refHi, jintArray totals, jlongArray degenerate, jlongArray siteFirst,
        jintArray begins, jintArray lens, jlongArray strOff, jbyteArray blob) {
    char err[640];
    jint *t, *bg, *ln;
    jlong *dg, *sf, *so;
    jbyte *bl;
    int rc = SWMI_ERR_NOMEM;
    (void)cls;
    if (!totals || !degenerate || !siteFirst || !begins || !lens || !strOff || !blob) { throw_msg(env, "nativeRefSitesPacked: null array argument"); return; }
    t = (*env)->GetIntArrayElements(env, totals, NULL);
    dg = (*env)->GetLongArrayElements(env, degenerate, NULL);
    sf = (*env)->GetLongArrayElements(env, siteFirst, NULL);
    bg = (*env)->GetIntArrayElements(env, begins, NULL);
    ln = (*env)->GetIntArrayElements(env, lens, NULL);
    so = (*env)->GetLongArrayElements(env, strOff, NULL);
    bl = (*env)->GetByteArrayElements(env, blob, NULL);
    if (t && dg && sf && bg && ln && so && bl) {
        jsize ns = (*env)->GetArrayLength(env, begins);
        if ((*env)->GetArrayLength(env, lens) < ns) ns = (*env)->GetArrayLength(env, lens);
        if ((*env)->GetArrayLength(env, strOff) < ns) ns = (*env)->GetArrayLength(env, strOff);
        rc = swmi_shim_ref_sites_packed((swmi_batch *)(intptr_t)batch, refLo, refHi,
                                        (int32_t *)t, (int64_t)(*env)->GetArrayLength(env, totals),
                                        (int64_t *)dg, (int64_t)(*env)->GetArrayLength(env, degenerate),
                                        (int64_t *)sf, (int64_t)(*env)->GetArrayLength(env, siteFirst),
                                        (int32_t *)bg, (int32_t *)ln, (int64_t *)so, (int64_t)ns,
                                        (signed char *)bl, (int64_t)(*env)->GetArrayLength(env, blob), err, sizeof err);
    } else {
        snprintf(err, sizeof err, "nativeRefSitesPacked: out of memory pinning the output arrays");
    }
    /* mode 0: copy back (if the VM handed out copies) and release */
    if (t) (*env)->ReleaseIntArrayElements(env, totals, t, 0);
    if (dg) (*env)->ReleaseLongArrayElements(env, degenerate, dg, 0);
    if (sf) (*env)->ReleaseLongArrayElements(env, siteFirst, sf, 0);
    if (bg) (*env)->ReleaseIntArrayElements(env, begins, bg, 0);
    if (ln) (*env)->ReleaseIntArrayElements(env, lens, ln, 0);
    if (so) (*env)->ReleaseLongArrayElements(env, strOff, so, 0);
    if (bl) (*env)->ReleaseByteArrayElements(env, blob, bl, 0);
    if (rc != SWMI_OK) throw_msg(env, err);
}
