// swmi_ctx.cpp -- library and context: ABI version, the thread's last error, options, score matrices, sequence upload.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "swmi_host.h"
#include "swmi_launch.h"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int swmi_host::fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int swmi_io_fail(int code, const std::string &msg) { return fail(code, "%s", msg.c_str()); }

// ------------------------------------------------------------------------------------------
// library / context
// ------------------------------------------------------------------------------------------
extern "C" int swmi_abi_version(void) { return SWMI_ABI_VERSION; }

extern "C" const char *swmi_last_error(void) { return g_err.c_str(); }

extern "C" int swmi_device_count(int *count) {
    if (!count) return fail(SWMI_ERR_INVALID, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(SWMI_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return SWMI_OK;
}

extern "C" void swmi_default_params(swmi_params *p) {
    if (!p) return;
    p->match = 5; p->mismatch = -3; p->gap = -4;            // Distribution.java:36
    p->tie_mode = SWMI_TIE_SERIAL;
    p->types[0] = 'a'; p->types[1] = 'i'; p->types[2] = 'd'; p->types[3] = '-';   // Distribution.java:37
}

static void ctx_release(swmi_ctx *c) {
    for (auto &ev : c->ev) if (ev) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    c->h_err.release();
    c->d_lut.release();
    c->d_comp.release();
    c->d_hdr_ring.release();
    delete c;
}

extern "C" int swmi_create(int device, swmi_ctx **out) {
    if (!out) return fail(SWMI_ERR_INVALID, "out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(SWMI_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n) return fail(SWMI_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(SWMI_ERR_NO_DEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SWMI_ERR_NO_DEVICE, "device %d is %s; the kernels are built for gfx950 (MI355X) only",
                    device, prop.gcnArchName);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(SWMI_ERR_NO_DEVICE, "hipSetDevice: %s", hipGetErrorString(e));
    // (no process-wide hipSetDeviceFlags: a run polls its own stream for `spin_us` before it blocks, see wait_for_stream)
    swmi_ctx *c = new swmi_ctx;
    c->device = device;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { c->stream = nullptr; ctx_release(c); return fail(SWMI_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    for (auto &ev : c->ev) {
        e = hipEventCreate(&ev);
        if (e != hipSuccess) { ev = nullptr; ctx_release(c); return fail(SWMI_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e)); }
    }
    { int r = c->h_err.reserve(64); if (r) { ctx_release(c); return r; } }
    { static const char *ee = getenv("SWMI_EXT_EVENTS"); if (ee) c->ext_events = atoi(ee) != 0; }
    *(volatile uint32_t *)c->h_err.p = 0u;
    { int r = c->d_lut.reserve(256); if (r) { ctx_release(c); return r; } }
    e = hipMemcpy(c->d_lut.p, code_table(), 256, hipMemcpyHostToDevice);
    if (e != hipSuccess) { ctx_release(c); return fail(SWMI_ERR_HIP, "code table upload: %s", hipGetErrorString(e)); }
    { int r = c->d_comp.reserve(256); if (r) { ctx_release(c); return r; } }
    e = hipMemcpy(c->d_comp.p, complement_table(), 256, hipMemcpyHostToDevice);
    if (e != hipSuccess) { ctx_release(c); return fail(SWMI_ERR_HIP, "complement table upload: %s", hipGetErrorString(e)); }
    *out = c;
    return SWMI_OK;
}

extern "C" void swmi_destroy(swmi_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->worker.joinable()) {
        {
            std::unique_lock<std::mutex> lk(ctx->job_mu);
            ctx->job_cv.wait(lk, [&] { return ctx->job_state.load() != 1; });      // a run still in flight
            ctx->job_state.store(3);
        }
        ctx->job_cv.notify_all();
        ctx->worker.join();
    }
    ctx_release(ctx);
}

extern "C" int swmi_set_option(swmi_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return fail(SWMI_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!strcmp(name, "cell_cap")) {
        if (value < 1 || value > (1 << 20)) return fail(SWMI_ERR_INVALID, "cell_cap out of range");
        ctx->cell_cap = (uint32_t)value;
        ctx->cell_cap_set = true;
    } else if (!strcmp(name, "max_workspace_bytes")) {
        if (value < (1 << 20)) return fail(SWMI_ERR_INVALID, "max_workspace_bytes too small");
        ctx->max_workspace_bytes = (uint64_t)value;
    } else if (!strcmp(name, "mode")) {
        // -1 is the same as 1 (kept for callers that passed "automatic": mode 0 was measured and is never faster)
        if (value < -1 || value > 2) return fail(SWMI_ERR_INVALID, "mode must be -1 (automatic), 0, 1 or 2");
        ctx->mode = value < 0 ? 1u : (uint32_t)value;
    } else if (!strcmp(name, "auto_ties_x100")) {
        if (value < 100) return fail(SWMI_ERR_INVALID, "auto_ties_x100 out of range");
        ctx->auto_ties_x100 = (uint32_t)value;
    } else if (!strcmp(name, "spin_us")) {
        if (value < 0) return fail(SWMI_ERR_INVALID, "spin_us out of range");
        ctx->spin_us = value;
    } else if (!strcmp(name, "debug_strip_spins")) {
        ctx->dbg_strip_spins = (uint32_t)value;
    } else if (!strcmp(name, "debug_reverse_strips")) {
        ctx->dbg_reverse_strips = value != 0;
    } else if (!strcmp(name, "debug_async_delay_us")) {
        if (value < 0 || value > 10000000) return fail(SWMI_ERR_INVALID, "debug_async_delay_us out of range");
        ctx->dbg_async_delay_us = (uint32_t)value;
    } else if (!strcmp(name, "tfused")) {
        if (value < -1 || value > 1) return fail(SWMI_ERR_INVALID, "tfused must be -1 (automatic), 0 or 1");
        ctx->tfused = (int)value;
    } else if (!strcmp(name, "resident")) {
        if (value < -1 || value > 1) return fail(SWMI_ERR_INVALID, "resident must be -1 (automatic), 0 or 1");
        ctx->resident = (int)value;
    } else if (!strcmp(name, "scores_only")) {
        ctx->scores_only = value != 0;
    } else if (!strcmp(name, "stream_keep_records")) {
        ctx->stream_keep_records = value != 0;
    } else if (!strcmp(name, "device_strings")) {
        ctx->device_strings = value != 0;
    } else if (!strcmp(name, "tb_split")) {
        if (value < -1 || value > 1) return fail(SWMI_ERR_INVALID, "tb_split must be -1 (automatic), 0 or 1");
        ctx->tb_split = (int)value;
    } else if (!strcmp(name, "col_chunks")) {
        if (value < 0 || value > 4096) return fail(SWMI_ERR_INVALID, "col_chunks out of range");
        ctx->col_chunks = (uint32_t)value;
    } else if (!strcmp(name, "zero_copy")) {
        ctx->zero_copy = value != 0;
    } else if (!strcmp(name, "profiling")) {
        if (value < 0 || value > 2) return fail(SWMI_ERR_INVALID, "profiling must be 0, 1 (every stage) or 2 (the sweep only)");
        ctx->profiling = (int)value;
    } else if (!strcmp(name, "gap_open")) {
        if (value > 0) return fail(SWMI_ERR_INVALID, "gap_open must be <= 0 (a penalty), got %lld", (long long)value);
        if (value < INT32_MIN) return fail(SWMI_ERR_INVALID, "gap_open out of range");
        ctx->gap_open = (int32_t)value;
    } else if (!strcmp(name, "affine")) {
        if (value != -1 && value != 1) return fail(SWMI_ERR_INVALID, "affine must be -1 (when gap_open != 0) or 1 (always)");
        ctx->affine = (int)value;
    } else if (!strcmp(name, "align_mode")) {
        if (value != SWMI_ALIGN_LOCAL && value != SWMI_ALIGN_FIT && value != SWMI_ALIGN_GLOBAL)
            return fail(SWMI_ERR_INVALID, "align_mode must be 0 (local), 1 (fit) or 2 (global), got %lld", (long long)value);
        ctx->modes.align_mode = (int)value;
    } else if (!strcmp(name, "long_reads")) {
        if (value != 0 && value != 1) return fail(SWMI_ERR_INVALID, "long_reads must be 0 or 1, got %lld", (long long)value);
        ctx->modes.long_reads = (int)value;
    } else if (!strcmp(name, "band")) {
        if (value < 0 || value > (int64_t)SWMI_AFF_BAND_MAX)
            return fail(SWMI_ERR_INVALID, "band must be 0 (none) or a half-width of 1 .. %u columns, got %lld", SWMI_AFF_BAND_MAX, (long long)value);
        ctx->modes.band = (int)value;
    } else if (!strcmp(name, "extend")) {
        if (value != 0 && value != 1) return fail(SWMI_ERR_INVALID, "extend must be 0 or 1, got %lld", (long long)value);
        ctx->modes.extend = (int)value;
    } else if (!strcmp(name, "xdrop")) {
        if (value < 0 || value > 0x7FFFFFFFll)
            return fail(SWMI_ERR_INVALID, "xdrop must be 0 (off) or a threshold of 1 .. 2^31 - 1, got %lld", (long long)value);
        ctx->modes.xdrop = (int)value;
    } else if (!strcmp(name, "band_adapt")) {
        if (value != 0 && value != 1) return fail(SWMI_ERR_INVALID, "band_adapt must be 0 or 1, got %lld", (long long)value);
        ctx->modes.band_adapt = (int)value;
    } else if (!strcmp(name, "gap_open2")) {
        if (value > 0) return fail(SWMI_ERR_INVALID, "gap_open2 must be <= 0 (a penalty; 0: one-piece gaps), got %lld", (long long)value);
        if (value < INT32_MIN) return fail(SWMI_ERR_INVALID, "gap_open2 out of range");
        ctx->modes.gap_open2 = (int)value;
    } else if (!strcmp(name, "gap2")) {
        if (value > 0) return fail(SWMI_ERR_INVALID, "gap2 must be <= 0 (the second piece's per-base extension), got %lld", (long long)value);
        if (value < INT32_MIN) return fail(SWMI_ERR_INVALID, "gap2 out of range");
        ctx->modes.gap2 = (int)value;
    } else if (!strcmp(name, "cigar")) {
        if (value < 0 || value > 2) return fail(SWMI_ERR_INVALID, "cigar must be 0 (off), 1 (M/I/D) or 2 (=/X/I/D), got %lld", (long long)value);
        ctx->modes.cigar = (int)value;
    } else if (!strcmp(name, "subopt")) {
        if (value < SWMI_SUBOPT_AUTO || value > (1ll << 30))
            return fail(SWMI_ERR_INVALID, "subopt must be 0 (off), a mask half-width of 1 .. 2^30 columns or -1 (SWMI_SUBOPT_AUTO), got %lld", (long long)value);
        ctx->modes.subopt = (int)value;
    } else if (!strcmp(name, "hits")) {
        if (value < 0 || value > (int64_t)SWMI_HITS_MAX)
            return fail(SWMI_ERR_INVALID, "hits must be 0 (off) or 1 .. %u entries per pair, got %lld", SWMI_HITS_MAX, (long long)value);
        ctx->modes.hits = (int)value;
    } else if (!strcmp(name, "end_bonus")) {
        if (value < 0 || value > (1ll << 30))
            return fail(SWMI_ERR_INVALID, "end_bonus must be 0 (off) or a bonus of 1 .. 2^30, got %lld", (long long)value);
        ctx->modes.end_bonus = (int)value;
    } else if (!strcmp(name, "overlap")) {
        if (value != 0 && value != 1) return fail(SWMI_ERR_INVALID, "overlap must be 0 or 1, got %lld", (long long)value);
        ctx->modes.overlap = (int)value;
    } else if (!strcmp(name, "arena_words_per_pair")) {
        if (value < 1) return fail(SWMI_ERR_INVALID, "arena_words_per_pair out of range");
        ctx->arena_words_per_pair = (uint64_t)value;
    } else {
        return fail(SWMI_ERR_INVALID, "unknown option '%s'", name);
    }
    return SWMI_OK;
}

// The classes of an alphabet of n symbols by canonical code (a score matrix's, a batch's profiles'): cls[code] = the symbol's index,
// n for a code outside the alphabet.  Two symbols with one code are refused.
static int alphabet_classes(const uint8_t *alphabet, uint32_t n, const char *what, uint32_t cls[256]) {
    const uint8_t *T = code_table();
    for (uint32_t c = 0; c < 256; c++) cls[c] = n;         // class n: outside the alphabet
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t c = T[alphabet[i]];
        if (cls[c] != n)
            return fail(SWMI_ERR_INVALID, "%s symbols %u and %u are the same symbol (0x%02x, 0x%02x)", what, cls[c], i,
                        alphabet[cls[c]], alphabet[i]);
        cls[c] = i;
    }
    return SWMI_OK;
}

extern "C" int swmi_set_score_matrix(swmi_ctx *ctx, const uint8_t *alphabet, uint32_t n, const int32_t *scores) {
    if (!ctx) return fail(SWMI_ERR_INVALID, "null context");
    if (n == 0) {                                          // clears the matrix
        std::lock_guard<std::mutex> g(ctx->mat_mu);
        ctx->matrix.reset();
        return SWMI_OK;
    }
    if (n > SWMI_MAT_MAX_SYMBOLS) return fail(SWMI_ERR_INVALID, "a score matrix has at most %u symbols, got %u", SWMI_MAT_MAX_SYMBOLS, n);
    if (!alphabet || !scores) return fail(SWMI_ERR_INVALID, "alphabet or scores is null");
    uint32_t cls[256];
    if (int rc = alphabet_classes(alphabet, n, "score matrix", cls)) return rc;
    auto M = std::make_shared<ScoreMatrix>();
    M->n = n;
    M->max_entry = INT32_MIN;
    const uint32_t nn = n + 1;
    M->image.assign(swmi_aff_mat_words(nn), 0u);
    for (uint64_t x = 0; x < (uint64_t)n * n; x++) {
        if (std::llabs((int64_t)scores[x]) > (1 << 20))
            return fail(SWMI_ERR_INVALID, "score matrix entry [%u][%u] = %d: |entries| must be <= 2^20", (uint32_t)(x / n),
                        (uint32_t)(x % n), scores[x]);
        M->max_entry = std::max(M->max_entry, scores[x]);
        M->image[256 + (x / n) * nn + x % n] = (uint32_t)scores[x];
    }
    for (uint32_t c = 0; c < 256; c++) M->image[c] = cls[c] * 4u | ((cls[c] == n ? c : 0x1FFu) << 16);
    static std::atomic<uint64_t> gens{0};
    M->gen = ++gens;
    std::lock_guard<std::mutex> g(ctx->mat_mu);
    ctx->matrix = std::move(M);
    return SWMI_OK;
}

// ------------------------------------------------------------------------------------------
// sequence encoding
// ------------------------------------------------------------------------------------------
// Canonical base codes: Character.toUpperCase restricted to ISO-8859-1 input (SmithWaterman.java:311-312:
// a-z and 0xE0-0xFE except 0xF7 drop 0x20; 0xB5 and 0xFF map outside Latin-1 and only equal themselves) followed by a permutation of the byte values that puts the eight
// "fast" symbols A,C,G,T,N,U,R,Y on the codes 0,4,...,28 (their bit offsets in an 8 x int4 score profile), so that
// code(x) == code(y)  <=>  toUpperCase(x) == toUpperCase(y).  Sequences made of those symbols only (and scores within
// int4) run the v_dot8_i32_i4 cell stream -- a reference with N stretches stays on the fast path; any other byte alphabet
// runs the compare-and-select variant.
const uint8_t *swmi_host::code_table() {
    static uint8_t T[256];
    static std::once_flag once;              // MapRef.call runs on every executor thread (Distribution.java:32,403)
    std::call_once(once, [] {
        uint8_t perm[256];
        for (int i = 0; i < 256; i++) perm[i] = (uint8_t)i;
        const uint8_t fast[8] = {'A', 'C', 'G', 'T', 'N', 'U', 'R', 'Y'};
        for (int k = 0; k < 8; k++) std::swap(perm[fast[k]], perm[4 * k]);   // -> 0,4,...,28
        for (int i = 0; i < 256; i++) {
            int u = i;
            if ((i >= 'a' && i <= 'z') || (i >= 0xE0 && i <= 0xFE && i != 0xF7)) u = i - 32;
            T[i] = perm[u];
        }
    });
    return T;
}

// Geometry of the byte images (swmi_device.h): every image 16-byte aligned and followed by SWMI_SEQ_PAD_WORDS zero
// dwords.  The bytes themselves are canonicalised on the GPU (sw_encode_kernel, swmi_prep.hip).
static uint64_t layout_sequences(const uint64_t *off, uint32_t n, uint64_t word0, std::vector<SeqDesc> &desc) {
    desc.resize(n);
    uint64_t at = word0;
    for (uint32_t s = 0; s < n; s++) {
        const uint64_t len = off[s + 1] - off[s];
        at = (at + 3) & ~(uint64_t)3;
        SeqDesc d{};
        d.len = (uint32_t)len;
        d.boff = (uint32_t)at;                 // (checked against 2^32 by the caller)
        d.acgt = 0;                            // set by the encode kernel
        desc[s] = d;
        at += (len + 3) / 4 + SWMI_SEQ_PAD_WORDS;
    }
    return at;
}

int swmi_host::check_offsets(const uint64_t *off, uint32_t n, const char *what) {
    if (!off) return fail(SWMI_ERR_INVALID, "%s offsets are null", what);
    if (off[0] != 0) return fail(SWMI_ERR_INVALID, "%s offsets must start at 0", what);
    for (uint32_t k = 0; k < n; k++) {
        if (off[k + 1] < off[k]) return fail(SWMI_ERR_INVALID, "%s offsets decrease at %u", what, k);
        if (off[k + 1] - off[k] >= (1ull << 30))
            return fail(SWMI_ERR_UNSUPPORTED, "%s %u is longer than 2^30-1 bases", what, k);
    }
    return SWMI_OK;
}

// ------------------------------------------------------------------------------------------
// upload
// ------------------------------------------------------------------------------------------
extern "C" void swmi_batch_free(swmi_ctx *ctx, swmi_batch *b) {
    if (!b) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    b->d_raw.release(); b->d_raw_off.release(); b->d_src_off.release();
    b->d_seqw.release(); b->d_refs.release(); b->d_reads.release(); b->d_pairs.release();
    b->d_dir.release(); b->d_seam.release(); b->d_result.release(); b->d_cells.release();
    b->d_cells_off.release(); b->d_cells_cap.release(); b->d_dbg.release(); b->d_dbg2.release();
    b->d_strip_items.release(); b->d_progress.release(); b->d_col_items.release(); b->d_win_off.release(); b->d_queue.release(); b->d_res_items.release();
    b->d_tf_items.release(); b->d_mat.release(); b->d_prof.release();
    b->h_result.release();
    delete b;
}

// Device side of an upload: geometry from the offsets already stored in the batch, the raw bytes H2D, and the
// canonical images written by sw_encode_kernel.  `ref_src` / `read_src` may be pinned (the streaming path) or pageable.
// Enqueued on `st` and synchronised before returning.
int swmi_host::upload_device(swmi_ctx *ctx, swmi_batch *b, hipStream_t st, const uint8_t *ref_src, const uint8_t *read_src) {
    const uint32_t n_refs = b->n_refs, n_reads = b->n_reads;
    const uint64_t ref_total = b->ref_off[n_refs], read_total = b->read_off[n_reads];
    uint64_t words = layout_sequences(b->ref_off.data(), n_refs, 0, b->ref_desc);
    words = layout_sequences(b->read_off.data(), n_reads, words, b->read_desc);
    words = ((words + 3) & ~(uint64_t)3) + SWMI_SEQ_PAD_WORDS;
    if (words >= (1ull << 32)) return fail(SWMI_ERR_UNSUPPORTED, "sequence image exceeds 16 GiB");
    int rc;
    const uint64_t read_base = (ref_total + 15) & ~(uint64_t)15;
    if ((rc = b->d_seqw.reserve(words * 4))) return rc;
    if ((rc = b->d_raw.reserve(read_base + read_total + 16))) return rc;
    if ((rc = b->d_raw_off.reserve(((uint64_t)n_refs + n_reads + 2) * 8))) return rc;
    if ((rc = b->d_refs.reserve(std::max<size_t>(n_refs, 1) * sizeof(SeqDesc)))) return rc;
    if ((rc = b->d_reads.reserve(std::max<size_t>(n_reads, 1) * sizeof(SeqDesc)))) return rc;
    HIP_TRY(hipMemsetAsync(b->d_seqw.p, 0, words * 4, st));
    uint8_t *raw = b->d_raw.as<uint8_t>();
    uint64_t *roff = b->d_raw_off.as<uint64_t>();
    if (ref_total) HIP_TRY(hipMemcpyAsync(raw, ref_src, ref_total, hipMemcpyHostToDevice, st));
    if (read_total) HIP_TRY(hipMemcpyAsync(raw + read_base, read_src, read_total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(roff, b->ref_off.data(), ((size_t)n_refs + 1) * 8, hipMemcpyHostToDevice, st));
    // (the reads' offsets are stored absolute -- from the start of `raw` -- so that one base pointer serves both sides)
    std::vector<uint64_t> read_abs(b->read_off);
    for (auto &o : read_abs) o += read_base;
    HIP_TRY(hipMemcpyAsync(roff + n_refs + 1, read_abs.data(), ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, st));
    if (n_refs) HIP_TRY(hipMemcpyAsync(b->d_refs.p, b->ref_desc.data(), n_refs * sizeof(SeqDesc), hipMemcpyHostToDevice, st));
    if (n_reads) HIP_TRY(hipMemcpyAsync(b->d_reads.p, b->read_desc.data(), n_reads * sizeof(SeqDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(swmi_launch_encode(raw, roff, b->d_refs.as<SeqDesc>(), b->d_seqw.as<uint32_t>(), ctx->d_lut.as<uint8_t>(), n_refs, st));
    HIP_TRY(swmi_launch_encode(raw, roff + n_refs + 1, b->d_reads.as<SeqDesc>(), b->d_seqw.as<uint32_t>(),
                               ctx->d_lut.as<uint8_t>(), n_reads, st));
    HIP_TRY(hipStreamSynchronize(st));
    // a new set of sequences invalidates everything derived from the old one
    b->work_key = SchedKey{}; b->plan_key = PlanKey{}; b->pairs_dev_ptr = nullptr; b->pairs_on_device.clear();
    b->has_run = false; b->acgt_known = false; b->auto_choice = -1;
    return SWMI_OK;
}

extern "C" int swmi_batch_upload(swmi_ctx *ctx,
                                 const uint8_t *ref_bytes, const uint64_t *ref_off, uint32_t n_refs,
                                 const uint8_t *read_bytes, const uint64_t *read_off, uint32_t n_reads,
                                 swmi_batch **out) {
    if (!ctx || !out) return fail(SWMI_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = check_offsets(ref_off, n_refs, "reference"))) return rc;
    if ((rc = check_offsets(read_off, n_reads, "read"))) return rc;
    if ((n_refs && ref_off[n_refs] && !ref_bytes) || (n_reads && read_off[n_reads] && !read_bytes))
        return fail(SWMI_ERR_INVALID, "sequence bytes are null");
    if ((uint64_t)n_refs * n_reads >= (1ull << 32))
        return fail(SWMI_ERR_UNSUPPORTED, "more than 2^32-1 pairs in one batch");
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));

    std::unique_ptr<swmi_batch> b(new swmi_batch);
    b->n_refs = n_refs; b->n_reads = n_reads;
    b->ref_off.assign(ref_off, ref_off + n_refs + 1);
    b->read_off.assign(read_off, read_off + n_reads + 1);
    // the caller's buffers are only valid during this call: the original bytes are kept for the alignment strings
    // (characters keep their case, SmithWaterman.java:388-406)
    b->ref_bytes.assign(ref_bytes, ref_bytes + ref_off[n_refs]);
    b->read_bytes.assign(read_bytes, read_bytes + read_off[n_reads]);
    if ((rc = upload_device(ctx, b.get(), ctx->stream, ref_bytes, read_bytes))) { swmi_batch_free(ctx, b.release()); return rc; }
    *out = b.release();
    return SWMI_OK;
}

// ------------------------------------------------------------------------------------------
// pair lists (swmi.h: swmi_batch_upload_pairs)
// ------------------------------------------------------------------------------------------
// The refusals of a list, on the host and before anything is uploaded or launched: `out` receives the list with
// SWMI_SPEC_WHOLE resolved.  After it every segment lies inside its source, which is all sw_gather_kernel relies on.
static int check_specs(const uint64_t *ref_off, uint32_t n_refs, const uint64_t *read_off, uint32_t n_reads, const swmi_pair_spec *specs,
                       uint64_t n_pairs, std::vector<swmi_pair_spec> &out) {
    if (n_pairs >= (1ull << 32)) return fail(SWMI_ERR_UNSUPPORTED, "more than 2^32-1 pairs in one batch (%llu)", (unsigned long long)n_pairs);
    if (n_pairs && !specs) return fail(SWMI_ERR_INVALID, "specs is null with n_pairs = %llu (pair 0 is missing)", (unsigned long long)n_pairs);
    out.resize(n_pairs);
    for (uint64_t k = 0; k < n_pairs; k++) {
        swmi_pair_spec sp = specs[k];
        const unsigned long long kk = k;
        if (sp.flags & ~(SWMI_SPEC_REVERSE | SWMI_SPEC_READ_REVCOMP))
            return fail(SWMI_ERR_INVALID, "pair %llu: unknown flag bits 0x%x (SWMI_SPEC_REVERSE and SWMI_SPEC_READ_REVCOMP are defined)", kk, sp.flags);
        if (sp.reserved) return fail(SWMI_ERR_INVALID, "pair %llu: reserved must be 0, got %u", kk, sp.reserved);
        if (sp.ref >= n_refs) return fail(SWMI_ERR_INVALID, "pair %llu: reference %u out of range (%u uploaded)", kk, sp.ref, n_refs);
        if (sp.read >= n_reads) return fail(SWMI_ERR_INVALID, "pair %llu: read %u out of range (%u uploaded)", kk, sp.read, n_reads);
        const uint64_t ref_len = ref_off[sp.ref + 1] - ref_off[sp.ref], read_len = read_off[sp.read + 1] - read_off[sp.read];
        if (sp.ref_len == SWMI_SPEC_WHOLE && sp.ref_start <= ref_len) sp.ref_len = (uint32_t)(ref_len - sp.ref_start);
        if (sp.read_len == SWMI_SPEC_WHOLE && sp.read_start <= read_len) sp.read_len = (uint32_t)(read_len - sp.read_start);
        if ((uint64_t)sp.ref_start + sp.ref_len > ref_len)
            return fail(SWMI_ERR_INVALID, "pair %llu: reference segment [%u, %u + %u) runs past the end of reference %u (%llu bytes)", kk,
                        sp.ref_start, sp.ref_start, sp.ref_len, sp.ref, (unsigned long long)ref_len);
        if ((uint64_t)sp.read_start + sp.read_len > read_len)
            return fail(SWMI_ERR_INVALID, "pair %llu: read segment [%u, %u + %u) runs past the end of read %u (%llu bytes)", kk, sp.read_start,
                        sp.read_start, sp.read_len, sp.read, (unsigned long long)read_len);
        out[k] = sp;
    }
    return SWMI_OK;
}

// Device side of a pair list.  d_raw: the reference sources, the read sources from a 16-byte boundary (as upload_device lays
// them out), then from a 4-byte boundary the raw bytes of every TRANSFORMED segment -- reversed, complemented or both --, each a
// whole number of dwords (written by the kernel).  A reference segment is reversed under SWMI_SPEC_REVERSE; a read segment is
// reversed under REVERSE xor READ_REVCOMP and complemented under READ_REVCOMP.  d_raw_off / d_src_off:
// n_pairs + 1 entries for the reference segments, then n_pairs + 1 for the read segments (the emitters' indexing, TraceArgs.raw_reads_at = n_pairs + 1; the last entry of a side is not read).  The sources get no image.
// `specs` is checked (check_specs); the batch's host state changes only once nothing can be refused any more.
static int pairs_to_device(swmi_ctx *ctx, swmi_batch *b, hipStream_t st, std::vector<swmi_pair_spec> &specs) {
    const uint32_t np = (uint32_t)specs.size();
    const uint64_t ref_total = b->ref_off[b->n_src_refs], read_total = b->read_off[b->n_src_reads];
    const uint64_t read_base = (ref_total + 15) & ~(uint64_t)15;
    std::vector<uint64_t> roff((size_t)np + 1, 0), qoff((size_t)np + 1, 0);          // the segments' lengths as offsets, for layout_sequences
    for (uint32_t k = 0; k < np; k++) { roff[k + 1] = roff[k] + specs[k].ref_len; qoff[k + 1] = qoff[k] + specs[k].read_len; }
    std::vector<SeqDesc> ref_desc, read_desc;
    uint64_t words = layout_sequences(roff.data(), np, 0, ref_desc);
    words = layout_sequences(qoff.data(), np, words, read_desc);
    words = ((words + 3) & ~(uint64_t)3) + SWMI_SEQ_PAD_WORDS;
    if (words >= (1ull << 32)) return fail(SWMI_ERR_UNSUPPORTED, "sequence image exceeds 16 GiB (the images of the %u pairs' segments together)", np);
    const size_t side = (size_t)np + 1;
    std::vector<uint64_t> raw_off(2 * side, 0), src_off(2 * side, 0);
    uint64_t rev_at = (read_base + read_total + 3) & ~(uint64_t)3;
    for (uint32_t k = 0; k < np; k++) {
        const swmi_pair_spec &sp = specs[k];
        const uint64_t rs = b->ref_off[sp.ref] + sp.ref_start, qs = read_base + b->read_off[sp.read] + sp.read_start;
        const bool R = (sp.flags & SWMI_SPEC_REVERSE) != 0, Cc = (sp.flags & SWMI_SPEC_READ_REVCOMP) != 0;
        src_off[k] = raw_off[k] = rs;
        src_off[side + k] = raw_off[side + k] = qs;
        if (R) {
            src_off[k] |= 1ull << 63;
            raw_off[k] = rev_at; rev_at += 4 * (((uint64_t)sp.ref_len + 3) / 4);
        }
        if (R || Cc) {
            src_off[side + k] |= (uint64_t)(R != Cc) << 63 | (uint64_t)Cc << 62;
            raw_off[side + k] = rev_at; rev_at += 4 * (((uint64_t)sp.read_len + 3) / 4);
        }
    }
    int rc;
    const size_t raw_need = rev_at + 16;
    if (raw_need > b->d_raw.cap) b->sources_on_device = false;         // (growing the buffer drops what it held)
    if ((rc = b->d_raw.reserve(raw_need))) return rc;
    if ((rc = b->d_seqw.reserve(words * 4))) return rc;
    if ((rc = b->d_raw_off.reserve(2 * side * 8))) return rc;
    if ((rc = b->d_src_off.reserve(2 * side * 8))) return rc;
    if ((rc = b->d_refs.reserve(std::max<size_t>(np, 1) * sizeof(SeqDesc)))) return rc;
    if ((rc = b->d_reads.reserve(std::max<size_t>(np, 1) * sizeof(SeqDesc)))) return rc;
    // from here on the batch is the new list
    b->n_refs = b->n_reads = np;
    b->specs.swap(specs);
    b->ref_desc.swap(ref_desc); b->read_desc.swap(read_desc);
    b->work.clear(); b->work_key = SchedKey{}; b->plan_key = PlanKey{}; b->pairs_dev_ptr = nullptr; b->pairs_on_device.clear();
    b->has_run = false; b->acgt_known = false; b->auto_choice = -1;
    b->pairs.clear(); b->alns.clear(); b->str_at.clear(); b->str_buf.clear(); b->raw.clear(); b->rtab.clear(); b->raw_chunks.clear();
    b->raw_ext = nullptr; b->rtab_ext = nullptr; b->indexed = false; b->win_tab.clear(); b->win_at.clear();
    uint8_t *raw = b->d_raw.as<uint8_t>();
    if (!b->sources_on_device) {
        if (ref_total) HIP_TRY(hipMemcpyAsync(raw, b->ref_bytes.data(), ref_total, hipMemcpyHostToDevice, st));
        if (read_total) HIP_TRY(hipMemcpyAsync(raw + read_base, b->read_bytes.data(), read_total, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemsetAsync(b->d_seqw.p, 0, words * 4, st));
    uint64_t *d_raw_off = b->d_raw_off.as<uint64_t>(), *d_src_off = b->d_src_off.as<uint64_t>();
    HIP_TRY(hipMemcpyAsync(d_raw_off, raw_off.data(), 2 * side * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_src_off, src_off.data(), 2 * side * 8, hipMemcpyHostToDevice, st));
    if (np) {
        HIP_TRY(hipMemcpyAsync(b->d_refs.p, b->ref_desc.data(), np * sizeof(SeqDesc), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b->d_reads.p, b->read_desc.data(), np * sizeof(SeqDesc), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(swmi_launch_gather(raw, d_src_off, d_raw_off, b->d_refs.as<SeqDesc>(), b->d_seqw.as<uint32_t>(), ctx->d_lut.as<uint8_t>(),
                               ctx->d_comp.as<uint8_t>(), np, st));
    HIP_TRY(swmi_launch_gather(raw, d_src_off + side, d_raw_off + side, b->d_reads.as<SeqDesc>(), b->d_seqw.as<uint32_t>(),
                               ctx->d_lut.as<uint8_t>(), ctx->d_comp.as<uint8_t>(), np, st));
    HIP_TRY(hipStreamSynchronize(st));               // (the host vectors above are pageable locals)
    b->sources_on_device = true;
    return SWMI_OK;
}

extern "C" int swmi_batch_upload_pairs(swmi_ctx *ctx,
                                       const uint8_t *ref_bytes, const uint64_t *ref_off, uint32_t n_refs,
                                       const uint8_t *read_bytes, const uint64_t *read_off, uint32_t n_reads,
                                       const swmi_pair_spec *specs, uint64_t n_pairs, swmi_batch **out) {
    if (!ctx || !out) return fail(SWMI_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = check_offsets(ref_off, n_refs, "reference"))) return rc;
    if ((rc = check_offsets(read_off, n_reads, "read"))) return rc;
    if ((n_refs && ref_off[n_refs] && !ref_bytes) || (n_reads && read_off[n_reads] && !read_bytes))
        return fail(SWMI_ERR_INVALID, "sequence bytes are null");
    std::vector<swmi_pair_spec> resolved;
    if ((rc = check_specs(ref_off, n_refs, read_off, n_reads, specs, n_pairs, resolved))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<swmi_batch> b(new swmi_batch);
    b->paired = true;
    b->n_src_refs = n_refs; b->n_src_reads = n_reads;
    b->ref_off.assign(ref_off, ref_off + n_refs + 1);
    b->read_off.assign(read_off, read_off + n_reads + 1);
    // (kept: host-built strings are cut from them, and a list with a larger transformed area uploads them again)
    b->ref_bytes.assign(ref_bytes, ref_bytes + ref_off[n_refs]);
    b->read_bytes.assign(read_bytes, read_bytes + read_off[n_reads]);
    if ((rc = pairs_to_device(ctx, b.get(), ctx->stream, resolved))) { swmi_batch_free(ctx, b.release()); return rc; }
    *out = b.release();
    return SWMI_OK;
}

extern "C" int swmi_batch_set_pairs(swmi_ctx *ctx, swmi_batch *b, const swmi_pair_spec *specs, uint64_t n_pairs) {
    if (!ctx || !b) return fail(SWMI_ERR_INVALID, "null argument");
    if (!b->paired) return fail(SWMI_ERR_INVALID, "the batch is a cross product (swmi_batch_upload): only a batch of swmi_batch_upload_pairs takes a pair list");
    std::lock_guard<std::mutex> g(ctx->mu);
    int rc;
    std::vector<swmi_pair_spec> resolved;
    if ((rc = check_specs(b->ref_off.data(), b->n_src_refs, b->read_off.data(), b->n_src_reads, specs, n_pairs, resolved))) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return pairs_to_device(ctx, b, ctx->stream, resolved);
}

extern "C" int swmi_batch_pair_spec(const swmi_batch *b, uint64_t pair, swmi_pair_spec *spec) {
    if (!b || !spec) return fail(SWMI_ERR_INVALID, "null argument");
    if (!b->paired) return fail(SWMI_ERR_INVALID, "the batch is a cross product (swmi_batch_upload): its pairs have no spec");
    if (pair >= b->specs.size()) return fail(SWMI_ERR_RANGE, "pair %llu out of range", (unsigned long long)pair);
    *spec = b->specs[pair];
    return SWMI_OK;
}

// ------------------------------------------------------------------------------------------
// per-read score profiles (swmi.h: swmi_batch_set_read_profiles)
// ------------------------------------------------------------------------------------------
// Builds the immutable ReadProfiles with its device image (AffProfile, swmi_launch.h) and hands it to the batch; the run uploads it.
// Everything that can be refused is refused before the batch is touched.
extern "C" int swmi_batch_set_read_profiles(swmi_ctx *ctx, swmi_batch *b, const uint8_t *alphabet, uint32_t n, const int32_t *scores) {
    if (!ctx || !b) return fail(SWMI_ERR_INVALID, "null argument");
    if (b->paired)
        return fail(SWMI_ERR_UNSUPPORTED, "read profiles on a pair list (swmi_batch_upload_pairs) are not supported: a segment would need its rows cut, "
                    "and the minus strand complemented columns");
    std::shared_ptr<const ReadProfiles> next;
    if (n != 0) {
        if (n > SWMI_MAT_MAX_SYMBOLS) return fail(SWMI_ERR_INVALID, "read profiles have at most %u symbols, got %u", SWMI_MAT_MAX_SYMBOLS, n);
        if (!alphabet || !scores) return fail(SWMI_ERR_INVALID, "alphabet or scores is null");
        uint32_t cls[256];
        if (int rc = alphabet_classes(alphabet, n, "read profile", cls)) return rc;
        const uint64_t rows = b->read_off[b->n_reads], entries = rows * n;
        auto P = std::make_shared<ReadProfiles>();
        P->n = n;
        P->max_entry = INT32_MIN;
        for (uint64_t x = 0; x < entries; x++) {
            if (std::llabs((int64_t)scores[x]) > (1 << 20))
                return fail(SWMI_ERR_INVALID, "read profile entry [row %llu][%u] = %d: |entries| must be <= 2^20", (unsigned long long)(x / n),
                            (uint32_t)(x % n), scores[x]);
            P->max_entry = std::max(P->max_entry, scores[x]);
            P->max_abs = std::max(P->max_abs, (int32_t)std::llabs((int64_t)scores[x]));
        }
        if (entries == 0) P->max_entry = 0;
        const uint64_t soff = ((uint64_t)SWMI_PROF_HDR_WORDS + 2ull * b->n_reads + 1u) & ~1ull;
        P->image.assign(soff + entries, 0u);
        for (uint32_t c = 0; c < 256; c++) P->image[c] = cls[c] * 4u;
        memcpy(&P->image[SWMI_PROF_KEY_WORDS], &soff, 8);
        if (b->n_reads) memcpy(&P->image[SWMI_PROF_HDR_WORDS], b->read_off.data(), (size_t)b->n_reads * 8);
        if (entries) memcpy(&P->image[soff], scores, entries * 4);
        static std::atomic<uint64_t> gens{0};
        P->gen = ++gens;
        next = std::move(P);
    }
    std::lock_guard<std::mutex> g(ctx->mu);             // (serialised with the runs of the context, as swmi_batch_set_pairs is)
    { std::lock_guard<std::mutex> gm(ctx->mat_mu); b->profiles = std::move(next); }
    // the old results are dropped: the batch is to be run again
    b->has_run = false;
    b->pairs.clear(); b->alns.clear(); b->str_at.clear(); b->str_buf.clear(); b->raw.clear(); b->rtab.clear(); b->raw_chunks.clear();
    b->raw_ext = nullptr; b->rtab_ext = nullptr; b->indexed = false; b->win_tab.clear(); b->win_at.clear();
    return SWMI_OK;
}
