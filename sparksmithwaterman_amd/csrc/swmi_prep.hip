// swmi_prep.hip -- gfx950 kernels that prepare a batch on the device (no DP arithmetic here).
//
// sw_encode_kernel: raw sequence bytes (as the caller / the FASTA reader hands them over) -> the canonical byte
// images the sweep reads (swmi_device.h: `seqw`), one wavefront per sequence.  This is the device half of what
// AlignmentScore's `Character.toUpperCase(x) == Character.toUpperCase(y)` (src/sw/SmithWaterman.java:309-318)
// needs: a 256-entry table maps a byte to its canonical code, so that code equality <=> that equality; the host only
// uploads the untouched bytes (H2D at PCIe rate) instead of encoding 10^9 bases on one core.
// It also derives SeqDesc.acgt (every base one of the eight fast symbols) with one ballot per 64 dwords.
//
// sw_gather_kernel: the same for a PAIR LIST (swmi_batch_upload_pairs): the sequences of such a batch are segments of source
// sequences that stay resident in `raw`; the kernel cuts them -- and for a left extension reverses them, for a read on the
// minus strand reverse-complements them -- on the way into their images, so that a mapper uploads its reads and its reference
// once, not every overlapping window and not every read twice.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "swmi_device.h"
#include "swmi_launch.h"

#define WAVE 64
#define ENC_WAVES 4

// One wavefront per sequence.  raw_off[s] .. raw_off[s+1] are the sequence's bytes in `raw`; its image starts at dword
// desc[s].boff of `seqw` and is followed by zero pad dwords (the whole of seqw is zeroed by the host runtime before).
extern "C" __global__ void __launch_bounds__(WAVE * ENC_WAVES)
sw_encode_kernel(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ raw_off, SeqDesc *__restrict__ desc,
                 uint32_t *__restrict__ seqw, const uint8_t *__restrict__ lut, uint32_t n_seq) {
    __shared__ uint8_t T[256];
    T[threadIdx.x] = lut[threadIdx.x];            // blockDim.x == 256
    __syncthreads();
    const uint32_t s = blockIdx.x * ENC_WAVES + (threadIdx.x >> 6);
    if (s >= n_seq) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t b0 = raw_off[s];
    const uint32_t len = (uint32_t)(raw_off[s + 1] - b0);
    uint32_t *__restrict__ img = seqw + desc[s].boff;
    const uint8_t *__restrict__ src = raw + b0;
    const uint32_t nw = (len + 3u) >> 2;
    uint32_t bad = 0;
    for (uint32_t w = lane; w < nw; w += WAVE) {
        const uint32_t k = 4u * w;
        uint32_t v = 0;
        // (the image offset is 16-byte aligned, the raw offset is not: byte loads, served by L1)
        const uint32_t c0 = T[src[k]];
        const uint32_t c1 = k + 1u < len ? T[src[k + 1u]] : 0u;
        const uint32_t c2 = k + 2u < len ? T[src[k + 2u]] : 0u;
        const uint32_t c3 = k + 3u < len ? T[src[k + 3u]] : 0u;
        v = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        bad |= v & 0xE3E3E3E3u;                    // a fast symbol's code is 0, 4, ..., 28
        img[w] = v;
    }
    const uint64_t anybad = __builtin_amdgcn_ballot_w64(bad != 0u);
    if (lane == 0) desc[s].acgt = anybad ? 0u : 1u;
}

extern "C" hipError_t swmi_launch_encode(const uint8_t *raw, const uint64_t *raw_off, SeqDesc *desc, uint32_t *seqw,
                                         const uint8_t *lut, uint32_t n_seq, hipStream_t st) {
    if (n_seq == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_encode_kernel, dim3((n_seq + ENC_WAVES - 1) / ENC_WAVES), dim3(WAVE * ENC_WAVES), 0, st,
                       raw, raw_off, desc, seqw, lut, n_seq);
    return hipGetLastError();
}

// One wavefront per SEGMENT of a pair list.  src_off[s]: the byte offset in `raw` of the segment's first source byte (bits
// 0-61, any alignment), in bit 63 whether the segment is taken in reverse byte order and in bit 62 whether every byte goes
// through the complement table `comp` first (a read on the minus strand); desc[s].len its length and
// desc[s].boff its image, as for sw_encode_kernel.  Forward, image dword w holds source bytes 4w .. 4w + 3 of the segment;
// reversed, bytes len - 1 - 4w downwards; bytes past the end are 0 and every dword is stored whole.  The code table is applied
// AFTER the complement: the image, acgt and everything that reads them see the complemented base.  The alignment strings
// (swmi_emit.h) read a segment that is neither reversed nor complemented where it lies in its source (raw_off[s] = the source
// offset: nothing is copied); a TRANSFORMED segment's bytes -- reversed, complemented or both, with their case -- are written
// as whole dwords to raw + raw_off[s], a 4-byte aligned place of its own behind the sources.  The host has checked every range
// against the sources (swmi_ctx.cpp: check_specs) and sized the buffers from the same numbers: no address here is outside
// them.  Both bits are per segment, so every branch on them is wave-uniform.  acgt is the SEGMENT's: a 'K' elsewhere in the
// source does not cost it the fast path.
// Loads are byte loads served by L1, as in sw_encode_kernel (a segment start has any alignment; a wavefront's 64 lanes read
// 256 consecutive bytes per iteration); profiles/r14/pairs.md measures it against sw_encode_kernel on the same bytes,
// profiles/r20/strand.md the complemented segments against the plain ones.
// The loop of sw_gather_kernel for one kind of segment: REV and CMP are the segment's two bits, chosen once per wavefront outside
// the loop, so the loop of a segment that is neither is the plain cut (profiles/r20/strand.md).  Returns the lane's `bad` bits.
template <bool REV, bool CMP>
static __device__ __forceinline__ uint32_t gather_loop(const uint8_t *src, uint32_t len, uint32_t lane, uint32_t *__restrict__ img,
                                                       uint32_t *rdst, const uint8_t *T, const uint8_t *K) {
    const uint32_t nw = (len + 3u) >> 2;
    uint32_t bad = 0;
    for (uint32_t w = lane; w < nw; w += WAVE) {
        const uint32_t k = 4u * w;
        const bool in1 = k + 1u < len, in2 = k + 2u < len, in3 = k + 3u < len;
        uint32_t r0, r1, r2, r3;                  // the segment's bytes k .. k + 3 as the kernels see them (0 past the end)
        if (!REV) {
            r0 = src[k];
            r1 = in1 ? src[k + 1u] : 0u;
            r2 = in2 ? src[k + 2u] : 0u;
            r3 = in3 ? src[k + 3u] : 0u;
        } else {
            const uint32_t e = len - 1u - k;      // (k < len: w < nw)
            r0 = src[e];
            r1 = in1 ? src[e - 1u] : 0u;
            r2 = in2 ? src[e - 2u] : 0u;
            r3 = in3 ? src[e - 3u] : 0u;
        }
        if (CMP) {
            r0 = K[r0];
            r1 = in1 ? K[r1] : 0u;
            r2 = in2 ? K[r2] : 0u;
            r3 = in3 ? K[r3] : 0u;
        }
        if (REV || CMP) rdst[w] = r0 | (r1 << 8) | (r2 << 16) | (r3 << 24);       // a transformed segment
        const uint32_t c0 = T[r0];
        const uint32_t c1 = in1 ? T[r1] : 0u;
        const uint32_t c2 = in2 ? T[r2] : 0u;
        const uint32_t c3 = in3 ? T[r3] : 0u;
        const uint32_t v = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        bad |= v & 0xE3E3E3E3u;                    // a fast symbol's code is 0, 4, ..., 28
        img[w] = v;
    }
    return bad;
}

extern "C" __global__ void __launch_bounds__(WAVE * ENC_WAVES)
sw_gather_kernel(uint8_t *raw, const uint64_t *__restrict__ src_off, const uint64_t *__restrict__ raw_off, SeqDesc *__restrict__ desc,
                 uint32_t *__restrict__ seqw, const uint8_t *__restrict__ lut, const uint8_t *__restrict__ comp, uint32_t n_seg) {
    __shared__ uint8_t T[256];
    __shared__ uint8_t K[256];
    T[threadIdx.x] = lut[threadIdx.x];            // blockDim.x == 256
    K[threadIdx.x] = comp[threadIdx.x];
    __syncthreads();
    const uint32_t s = blockIdx.x * ENC_WAVES + (threadIdx.x >> 6);
    if (s >= n_seg) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t so = src_off[s];
    const bool rev = (so >> 63) != 0, cmp = ((so >> 62) & 1u) != 0;
    const uint8_t *src = raw + (so & 0x3FFFFFFFFFFFFFFFull);
    const uint32_t len = desc[s].len;
    uint32_t *__restrict__ img = seqw + desc[s].boff;
    uint32_t *rdst = rev || cmp ? (uint32_t *)(raw + raw_off[s]) : nullptr;        // a transformed segment's own place
    uint32_t bad;
    if (!rev && !cmp) bad = gather_loop<false, false>(src, len, lane, img, rdst, T, K);
    else if (!cmp) bad = gather_loop<true, false>(src, len, lane, img, rdst, T, K);
    else if (!rev) bad = gather_loop<false, true>(src, len, lane, img, rdst, T, K);
    else bad = gather_loop<true, true>(src, len, lane, img, rdst, T, K);
    const uint64_t anybad = __builtin_amdgcn_ballot_w64(bad != 0u);
    if (lane == 0) desc[s].acgt = anybad ? 0u : 1u;
}

extern "C" hipError_t swmi_launch_gather(uint8_t *raw, const uint64_t *src_off, const uint64_t *raw_off, SeqDesc *desc, uint32_t *seqw,
                                         const uint8_t *lut, const uint8_t *comp, uint32_t n_seg, hipStream_t st) {
    if (n_seg == 0) return hipSuccess;
    hipLaunchKernelGGL(sw_gather_kernel, dim3((n_seg + ENC_WAVES - 1) / ENC_WAVES), dim3(WAVE * ENC_WAVES), 0, st,
                       raw, src_off, raw_off, desc, seqw, lut, comp, n_seg);
    return hipGetLastError();
}
