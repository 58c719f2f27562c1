// swmi_diag.cpp -- diagnostics behind environment switches; nothing here runs unless one is set.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <unistd.h>

#include "swmi_host.h"

// SWMI_DEBUG_FILL=1: where the time of the traceback (per-pair ticks, walk / staging shares, the slowest pairs) and of the
// sweep (ticks, wave placement by HW_ID) went.  Diagnostics only.  (The traceback's per-pair counters are compiled into the
// kernels only with `make KFLAGS=-DSWMI_TB_DIAG`: without it this prints zeros for them.)
int swmi_host::dump_traceback_diagnostics(swmi_batch *b, const TraceArgs &ta, size_t np, size_t n_tf) {
    if (!ta.dbg) return SWMI_OK;
    std::vector<unsigned long long> d(np * 4);
    HIP_TRY(hipMemcpy(d.data(), ta.dbg, np * 32, hipMemcpyDeviceToHost));
    if (n_tf) {          // sw_tfused_kernel's own fields: {ticks, sweep | prologue << 32, replay << 16 | steps, replays | walk << 32}
        double t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0; unsigned long long mx = 0;
        for (size_t k = 0; k < np; k++) {
            t0 += d[4*k]; t1 += d[4*k+1] & 0xFFFFFFFFull; t2 += d[4*k+1] >> 32; t3 += d[4*k+2] >> 16; t4 += d[4*k+3] >> 32; t5 += d[4*k+3] & 0xFFFFFFFFull;
            mx = std::max(mx, d[4*k]);
        }
        fprintf(stderr, "[swmi tfused dbg] ticks per sweeper wavefront: lifetime mean=%.0f max=%llu = prologue %.0f + sweep %.0f + first block task %.0f (%.2f block tasks per wavefront) + waiting for tasks %.0f + rest (more tasks, walk items) %.0f\n",
                t0 / np, mx, t2 / np, t1 / np, t3 / np, t5 / np, t4 / np, (t0 - t1 - t2 - t3 - t4) / np);
        {   // the distribution of the wavefront lifetimes and the slowest ones
            std::vector<size_t> idx(np);
            for (size_t k = 0; k < np; k++) idx[k] = k;
            std::sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return d[4 * x] < d[4 * y]; });
            auto at = [&](double q) { return d[4 * idx[std::min<size_t>(np - 1, (size_t)(q * np))]]; };
            fprintf(stderr, "[swmi tfused dbg]   lifetime p10=%llu p50=%llu p90=%llu p99=%llu max=%llu\n", at(0.10), at(0.50), at(0.90), at(0.99), d[4 * idx[np - 1]]);
            for (size_t t = 0; t < std::min<size_t>(np, 6); t++) {
                const size_t k = idx[np - 1 - t];
                fprintf(stderr, "[swmi tfused dbg]   slow wavefront (pair %zu): lifetime %llu, sweep %llu, first block task %llu, block tasks taken %llu, waiting %llu, alignments of its pair %llu\n",
                        k, d[4 * k], d[4 * k + 1] & 0xFFFFFFFFull, d[4 * k + 2] >> 16, d[4 * k + 3] & 0xFFFFFFFFull, d[4 * k + 3] >> 32,
                        (unsigned long long)((const PairOut *)((const uint8_t *)b->h_result.p + result_out_off()))[k].n_cells);
            }
        }
    }
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0; unsigned long long mx = 0;
    double a4 = 0;
    for (size_t k = 0; k < np; k++) { a0 += d[4*k]; a1 += d[4*k+1] & 0xFFFFFFFFull; a2 += d[4*k+2] & 0xFFFF; a4 += d[4*k+2] >> 16; a3 += d[4*k+3] & 0xFFFFFFFFull; mx = std::max(mx, d[4*k]); }
    fprintf(stderr, "[swmi tb dbg] wave ticks mean=%.0f max=%llu; walk ticks mean=%.0f; staging ticks mean=%.0f; steps mean=%.1f; iterations mean=%.2f\n",
            a0 / np, mx, a1 / np, a4 / np, a2 / np, a3 / np);
    const PairOut *po_dbg = (const PairOut *)((const uint8_t *)b->h_result.p + result_out_off());
    double cs[4] = {0, 0, 0, 0}, cw[4] = {0, 0, 0, 0}; unsigned long long cm[4] = {0, 0, 0, 0}; size_t cn[4] = {0, 0, 0, 0};
    for (size_t k = 0; k < np; k++) {
        const size_t c = std::min<uint64_t>(po_dbg[k].n_cells, 4) - (po_dbg[k].n_cells ? 1 : 0);
        cs[c] += d[4 * k]; cw[c] += d[4 * k + 1] & 0xFFFFFFFFull; cm[c] = std::max(cm[c], d[4 * k]); cn[c]++;
    }
    {   // the slowest pairs: what makes the launch's tail
        std::vector<size_t> idx(np);
        for (size_t k = 0; k < np; k++) idx[k] = k;
        const size_t top = std::min<size_t>(np, 6);
        std::partial_sort(idx.begin(), idx.begin() + top, idx.end(), [&](size_t x, size_t y) { return d[4 * x] > d[4 * y]; });
        for (size_t t = 0; t < top; t++)
            fprintf(stderr, "[swmi tb dbg]   slow pair %zu: ticks=%llu walk=%llu staging=%llu in %llu stagings, steps=%llu iterations=%llu alignments=%llu\n", idx[t],
                    d[4 * idx[t]], d[4 * idx[t] + 1] & 0xFFFFFFFFull, d[4 * idx[t] + 2] >> 16, d[4 * idx[t] + 3] >> 32, d[4 * idx[t] + 2] & 0xFFFF,
                    d[4 * idx[t] + 3] & 0xFFFFFFFFull, (unsigned long long)po_dbg[idx[t]].n_cells);
        for (size_t t = 0; t < top; t++)
            fprintf(stderr, "[swmi tb dbg]     ... of the staging time of pair %zu, %llu ticks waiting for helpers\n", idx[t], d[4 * idx[t] + 1] >> 32);
    }
    for (int c = 0; c < 4; c++)
        if (cn[c]) fprintf(stderr, "[swmi tb dbg]   %d%s alignment(s): %zu pairs, wave ticks mean=%.0f max=%llu, walk(slot 0) mean=%.0f\n",
                           c + 1, c == 3 ? "+" : "", cn[c], cs[c] / cn[c], cm[c], cw[c] / cn[c]);
    return SWMI_OK;
}

int swmi_host::dump_fill_diagnostics(swmi_batch *b, const FillArgs &fa, size_t np) {
    if (!fa.dbg) return SWMI_OK;
    std::vector<unsigned long long> d(np * 2);
    HIP_TRY(hipMemcpy(d.data(), fa.dbg, np * 16, hipMemcpyDeviceToHost));
#ifdef SWMI_STRIP_DIAG
    // strip pipeline (reads of two strips or more): see fill_pair
    for (size_t k = 0; k < np && k < 8; k++)
        fprintf(stderr, "[swmi strip dbg] pair %zu: strip 0 lifetime %llu ticks, %llu waiting before publications; strip 1 lifetime %llu, "
                "%llu polls, %llu ticks in polls, %llu waiting for seam groups\n", k, d[2 * k] >> 32, d[2 * k] & 0xFFFFFFFFull,
                d[2 * k + 1] >> 40, (d[2 * k + 1] >> 32) & 0xFF, (d[2 * k + 1] >> 16) & 0xFFFF, d[2 * k + 1] & 0xFFFF);
#endif
    unsigned long long ev = 0, cyc = 0, evmax = 0, cmax = 0, cmin = ~0ull;
    for (size_t k = 0; k < np; k++) {
        ev += d[2 * k]; cyc += d[2 * k + 1];
        evmax = std::max(evmax, d[2 * k]); cmax = std::max(cmax, d[2 * k + 1]); cmin = std::min(cmin, d[2 * k + 1]);
    }
    fprintf(stderr, "[swmi fill dbg] pairs=%zu slow-path entries mean=%.1f max=%llu; wave ticks mean=%.0f min=%llu max=%llu\n",
            np, (double)ev / np, evmax, (double)cyc / np, cmin, cmax);
    if (b->eff_mode == 1) {
        // the fast sweep stores HW_ID | XCC_ID << 32 instead of an event count: placement of the waves
        std::unordered_map<unsigned long long, int> per_simd, per_cu;
        for (size_t k = 0; k < np; k++) {
            const unsigned long long hw = d[2 * k] & 0xFFFFFFFFull, xcc = (d[2 * k] >> 32) & 0xF;
            const unsigned long long simd = (hw >> 4) & 3, cu = (hw >> 8) & 15, sh = (hw >> 12) & 1, se = (hw >> 13) & 7;
            const unsigned long long cukey = (xcc << 16) | (se << 8) | (sh << 4) | cu;
            per_cu[cukey]++; per_simd[(cukey << 4) | simd]++;
        }
        int h_simd[9] = {0}, h_cu[17] = {0};
        for (auto &kv : per_simd) h_simd[std::min(kv.second, 8)]++;
        for (auto &kv : per_cu) h_cu[std::min(kv.second, 16)]++;
        fprintf(stderr, "[swmi fill dbg] placement: %zu CUs, %zu SIMDs used; SIMDs by waves held: 1:%d 2:%d 3:%d 4+:%d; CUs by waves held: 1-4:%d 5-8:%d 9+:%d\n",
                per_cu.size(), per_simd.size(), h_simd[1], h_simd[2], h_simd[3], h_simd[4] + h_simd[5] + h_simd[6] + h_simd[7] + h_simd[8],
                h_cu[1] + h_cu[2] + h_cu[3] + h_cu[4], h_cu[5] + h_cu[6] + h_cu[7] + h_cu[8], h_cu[9] + h_cu[10] + h_cu[11] + h_cu[12] + h_cu[13] + h_cu[14] + h_cu[15] + h_cu[16]);
    }
    return SWMI_OK;
}

// SWMI_DEBUG_WATCHDOG=<seconds>: give up on a launch that does not end, show the kernel's marks
void swmi_host::watchdog_wait(hipStream_t st, const swmi_batch *b, const char *limit_s) {
    const auto w0 = std::chrono::steady_clock::now();
    while (hipStreamQuery(st) == hipErrorNotReady)
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() > atof(limit_s)) {
            const volatile uint32_t *hm = (const volatile uint32_t *)b->h_result.p;
            fprintf(stderr, "[swmi watchdog] launch still running after %s s; marks:", limit_s);
            for (int k = 0; k < 12; k++) fprintf(stderr, " %08x", hm ? hm[k] : 0u);
            fprintf(stderr, "\n");
            fflush(stderr);
            _exit(3);
        }
}
