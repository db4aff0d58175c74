// lmi_host_debug.h -- reading a call's phase timings (events or device stamps), scan / prefilter statistics and the test hooks.
#pragma once
#include "lmi_host_mutate.h"
#include "lmi_host_search.h"

static int read_event_set(const hipEvent_t* ev, const bool* ev_valid, float* ms) {
    for (int i = 0; i < LMI_T_COUNT; ++i) ms[i] = 0.0f;
    auto span = [&](int a, int b, float* out) -> int {
        if (ev_valid[a] && ev_valid[b]) HIPCHK(hipEventElapsedTime(out, ev[a], ev[b]));
        return 0;
    };
    CHK(span(0, 1, &ms[LMI_T_INFERENCE]));
    CHK(span(1, 2, &ms[LMI_T_ROUTE]));
    CHK(span(2, 3, &ms[LMI_T_SCAN]));
    CHK(span(3, 4, &ms[LMI_T_MERGE]));
    CHK(span(2, 5, &ms[LMI_T_PF_SAMPLE]));
    CHK(span(5, 6, &ms[LMI_T_PF_EMIT]));
    CHK(span(6, 7, &ms[LMI_T_RESCORE]));
    CHK(span(7, 3, &ms[LMI_T_FALLBACK]));
    int first = ev_valid[0] ? 0 : 1;
    int last = ev_valid[4] ? 4 : 1;
    CHK(span(first, last, &ms[LMI_T_TOTAL]));
    return 0;
}

// the same phases from one set of device stamps (timing level 2): `v` the set's ST_COUNT words, `mask` the stamps this call's
// kernels were given; ticks of the chip's constant clock -> ms
static void read_stamp_set(const lmi_index* h, const unsigned long long* v, unsigned mask, float* ms) {
    for (int i = 0; i < LMI_T_COUNT; ++i) ms[i] = 0.0f;
    auto have = [&](int a) { return (mask >> a) & 1u; };
    auto span = [&](int a, int b, float* out) {
        if (have(a) && have(b) && v[b] >= v[a]) *out = (float)((double)(v[b] - v[a]) / h->wall_khz);
    };
    span(ST_MLP0, have(ST_MLP1) ? ST_MLP1 : ST_FRONT, &ms[LMI_T_INFERENCE]);
    span(ST_FRONT, have(ST_P1) ? ST_P1 : ST_SCAN0, &ms[LMI_T_ROUTE]);
    if (have(ST_P1)) {
        span(ST_P1, ST_P2, &ms[LMI_T_PF_SAMPLE]);
        span(ST_P2, ST_P2END, &ms[LMI_T_PF_EMIT]);
        span(ST_P2END, ST_FB, &ms[LMI_T_RESCORE]);
        const int after = have(ST_MERGE) ? ST_MERGE : ST_END;   // (the fused tail merges in its own kernels: no merge launch)
        span(ST_FB, after, &ms[LMI_T_FALLBACK]);
        span(ST_P1, after, &ms[LMI_T_SCAN]);
    } else {
        span(ST_SCAN0, ST_SCAN1, &ms[LMI_T_SCAN]);
    }
    span(ST_MERGE, ST_END, &ms[LMI_T_MERGE]);
    const int first = have(ST_MLP0) ? ST_MLP0 : ST_FRONT, last = have(ST_END) ? ST_END : ST_MLP1;
    span(first, last, &ms[LMI_T_TOTAL]);
    // the clock the chip held under the dominant kernel: block 0's life in shader cycles (s_memtime) over the same in 100 MHz ticks
    if (have(ST_CLK_WALL) && have(ST_CLK_CYC) && v[ST_CLK_WALL] > 0) ms[LMI_T_CLOCK_MHZ] = (float)((double)v[ST_CLK_CYC] / (double)v[ST_CLK_WALL] * (h->wall_khz / 1000.0));
}

extern "C" LMI_API int lmi_timings(lmi_index* h, float* ms) {
    if (!h || !ms) return fail("lmi_timings: NULL argument");
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->timing_level == 2) {
        unsigned long long v[ST_COUNT] = {};
        if (h->ts_set) HIPCHK(hipMemcpy(v, h->ts_set, sizeof(v), hipMemcpyDeviceToHost));
        read_stamp_set(h, v, h->ts_set ? h->ts_mask[h->ev_cur] : 0u, ms);
        return 0;
    }
    return read_event_set(h->ev, h->ev_valid, ms);
}

extern "C" LMI_API int lmi_set_timing(lmi_index* h, int level) {
    if (!h) return fail("lmi_set_timing: NULL handle");
    if (level < 0 || level > 3) return fail("lmi_set_timing: level %d outside 0..3", level);
    h->timing_level = level;
    return 0;
}

extern "C" LMI_API int lmi_timings_reset(lmi_index* h) {
    if (!h) return fail("lmi_timings_reset: NULL handle");
    h->ev_calls = 0;
    return 0;
}

extern "C" LMI_API int lmi_timings_mean(lmi_index* h, float* ms, int* n_calls) {
    if (!h || !ms) return fail("lmi_timings_mean: NULL argument");
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int n = (int)std::min<long long>(h->ev_calls, lmi_index::EV_RING);
    double sum[LMI_T_COUNT] = {};
    std::vector<unsigned long long> ring;
    if (h->timing_level == 2 && h->ts_ring.p) {
        ring.resize((size_t)lmi_index::EV_RING * ST_COUNT);
        HIPCHK(hipMemcpy(ring.data(), h->ts_ring.p, ring.size() * 8, hipMemcpyDeviceToHost));
    }
    for (int j = 0; j < n; ++j) {
        const int r = ((h->ev_cur - j) % lmi_index::EV_RING + lmi_index::EV_RING) % lmi_index::EV_RING;
        float one[LMI_T_COUNT];
        if (h->timing_level == 2) {
            if (ring.empty()) break;
            read_stamp_set(h, ring.data() + (size_t)r * ST_COUNT, h->ts_mask[r], one);
        } else
        CHK(read_event_set(h->ev_ring[r], h->valid_ring[r], one));
        for (int i = 0; i < LMI_T_COUNT; ++i) sum[i] += one[i];
    }
    for (int i = 0; i < LMI_T_COUNT; ++i) ms[i] = n ? (float)(sum[i] / n) : 0.0f;
    if (n_calls) *n_calls = n;
    return 0;
}

extern "C" LMI_API int lmi_prefilter_stats(lmi_index* h, int* active, int64_t* survivors, int64_t* fallbacks) {
    if (!h) return fail("lmi_prefilter_stats: NULL handle");
    CHK(set_dev(h));
    unsigned long long acc[2] = {0, 0};
    if (h->last_fast && h->last_nslots > 0) {
        unsigned long long* d_acc = reinterpret_cast<unsigned long long*>(h->stats.as<long long>() + 2);
        HIPCHK(hipMemsetAsync(d_acc, 0, 16, h->stream));
        prefilter_stats_kernel<<<64, 256, 0, h->stream>>>(h->nkeep.as<int>(), h->fallback.as<int>(), h->last_nslots, d_acc);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(acc, d_acc, 16, hipMemcpyDeviceToHost));
    }
    if (active) *active = (h->prefilter && h->have16) ? 1 : 0;
    if (survivors) *survivors = (int64_t)acc[0];
    if (fallbacks) *fallbacks = (int64_t)acc[1];
    return 0;
}

// ---- test hooks (tests/test_gpu_bound.py): the fp16 scores the pass-2 kernel really produced --------------
extern "C" LMI_API int lmi_debug_emit_all(lmi_index* h, int on) {
    if (!h) return fail("lmi_debug_emit_all: NULL handle");
    h->debug_emit_all = on != 0;
    return 0;
}

extern "C" LMI_API int lmi_debug_layout(lmi_index* h, int32_t* rb_start, int32_t* cap_rb, int64_t* n_rb_total, int64_t* alloc,
                                        int64_t* counters) {
    if (!h) return fail("lmi_debug_layout: NULL handle");
    if (!h->built) return fail("lmi_debug_layout: the bucket index is not built (lmi_buckets_end has not run)");
    const int L = h->L;
    if (rb_start) std::copy(h->h_rb_start.begin(), h->h_rb_start.begin() + L + 1, rb_start);
    if (cap_rb) std::copy(h->h_cap_rb.begin(), h->h_cap_rb.end(), cap_rb);
    if (n_rb_total) *n_rb_total = h->n_rb_total;
    if (alloc) *alloc = alloc_rb(h);
    if (counters) std::copy(h->mut_paths, h->mut_paths + 4, counters);
    return 0;
}

// ---- test hooks (tests/test_gpu_seams.py): which kernel forms a scan takes ----
extern "C" LMI_API int lmi_debug_last_plan(lmi_index* h, int32_t* out, int n) {
    if (!h || !out) return fail("lmi_debug_last_plan: NULL argument");
    if (n < 1) return fail("lmi_debug_last_plan: n %d < 1", n);
    std::copy(h->last_plan, h->last_plan + std::min<int>(n, LMI_PLAN_COUNT), out);
    return 0;
}

extern "C" LMI_API int lmi_debug_plan(lmi_index* h, int nq, int nb, int k, int32_t* out, int n) {
    if (!h || !out) return fail("lmi_debug_plan: NULL argument");
    if (n < 1) return fail("lmi_debug_plan: n %d < 1", n);
    int kout = 0;
    CHK(check_scan_args(h, nq, nb, k, &kout, "lmi_debug_plan"));
    int32_t w[LMI_PLAN_COUNT];
    plan_report(h, scan_plan(h, nq, nb, kout), w);
    std::copy(w, w + std::min<int>(n, LMI_PLAN_COUNT), out);
    return 0;
}

// ---- test hooks (tests/test_gpu_mlp_seams.py): which form an MLP forward takes ----
extern "C" LMI_API int lmi_debug_last_mlp_plan(lmi_index* h, int32_t* out, int n) {
    if (!h || !out) return fail("lmi_debug_last_mlp_plan: NULL argument");
    if (n < 1) return fail("lmi_debug_last_mlp_plan: n %d < 1", n);
    std::copy(h->last_mlp_plan, h->last_mlp_plan + std::min<int>(n, LMI_MLP_PLAN_COUNT), out);
    return 0;
}

extern "C" LMI_API int lmi_debug_mlp_plan(lmi_index* h, int nq, int nb, int want_proba, int want_logits, int32_t* out, int n) {
    if (!h || !out) return fail("lmi_debug_mlp_plan: NULL argument");
    if (n < 1) return fail("lmi_debug_mlp_plan: n %d < 1", n);
    if (nq < 0) return fail("lmi_debug_mlp_plan: nq < 0");
    const bool proba = want_proba != 0;
    if (proba && h->root().n_layers > 0) nb = h->root().dims.back();   // lmi_mlp_proba ranks every class
    RankStop stop;
    CHK(mlp_call_check(h, nb, proba, "lmi_debug_mlp_plan", stop));
    const FusedLds F = fused_lds_plan(h->models);   // what build_descs would find, without touching the device
    int32_t w[LMI_MLP_PLAN_COUNT];
    mlp_plan_report(h, F, mlp_plan(h->num_cus, h->fused_mlp, F.ok, F.logits_lds, nq, proba, want_logits != 0 && !proba, stop), stop, proba, w);
    std::copy(w, w + std::min<int>(n, LMI_MLP_PLAN_COUNT), out);
    return 0;
}

extern "C" LMI_API int lmi_debug_read_candidates(lmi_index* h, int64_t slot, int cap, uint32_t* rows, float* shat,
                                         int* count, float* eps2, float* qscale, float* xscale) {
    if (!h) return fail("lmi_debug_read_candidates: NULL handle");
    if (!h->last_fast) return fail("lmi_debug_read_candidates: the last scan did not use the prefilter");
    if (slot < 0 || slot >= h->last_nslots) return fail("lmi_debug_read_candidates: slot outside the last scan's %d", h->last_nslots);
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    int col = -1;
    HIPCHK(hipMemcpy(&col, h->slot_col.as<int>() + slot, 4, hipMemcpyDeviceToHost));
    unsigned cnt = 0;
    float e2 = 0.0f, qs = 1.0f, xs[2] = {1.0f, 1.0f};
    if (col >= 0) {
        HIPCHK(hipMemcpy(&cnt, h->cand_cnt.as<unsigned>() + col, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&e2, h->eps2.as<float>() + col, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&qs, h->qscale.as<float>() + slot / h->last_nb, 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(xs, h->xscale.p, 8, hipMemcpyDeviceToHost));
        const unsigned n = std::min<unsigned>(std::min<unsigned>(cnt, (unsigned)PF_CAP), (unsigned)std::max(cap, 0));
        if (n && rows) HIPCHK(hipMemcpy(rows, h->cand_row.as<unsigned>() + (size_t)col * PF_CAP, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (n && shat) HIPCHK(hipMemcpy(shat, h->cand_s.as<float>() + (size_t)col * PF_CAP, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    if (count) *count = col >= 0 ? (int)cnt : -1;
    if (eps2) *eps2 = e2;
    if (qscale) *qscale = qs;
    if (xscale) *xscale = xs[0];
    return 0;
}

// developer aid: the first `bytes` of a named internal device buffer ("pf_bound": LMI_PF_STAMPS builds keep phase timings there)
extern "C" LMI_API int lmi_debug_peek(lmi_index* h, const char* name, void* dst, int64_t bytes) {
    if (!h || !name || !dst) return fail("lmi_debug_peek: NULL argument");
    CHK(set_dev(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    DevBuf* b = nullptr;
    size_t off = 0;
    if (!strcmp(name, "pf_bound")) b = &h->pf_bound;
    if (!strcmp(name, "fr_dbg")) b = &h->fr_dbg;
    if (!strcmp(name, "pf_stamps")) { b = &h->pf_bound; off = h->stamps_off; }
    if (!strcmp(name, "cand_total")) {   // 8 bytes: candidates pass 2 emitted in the last scan, summed over the columns (capped counts not: the counters run on)
        if (bytes != 8 || !h->last_fast) return fail("lmi_debug_peek: cand_total is 8 bytes after a prefilter scan");
        unsigned long long* d_acc = reinterpret_cast<unsigned long long*>(h->stats.as<long long>() + 2);
        HIPCHK(hipMemsetAsync(d_acc, 0, 8, h->stream));
        sum_u32_kernel<<<64, 256, 0, h->stream>>>(h->cand_cnt.as<unsigned>(), h->last_ncols, d_acc);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(dst, d_acc, 8, hipMemcpyDeviceToHost));
        return 0;
    }
    if (!strcmp(name, "pf_redo")) b = &h->redo;   // [0]: columns whose candidate buffer overflowed in the last scan (second run of pass 2)
    // 32 bytes: [0] slots fallback_kernel handled, [1] / [2] fail flags of the overflow log (pass 2 / its redo launch), [3] entries
    // appended to the log, [4] entries sorted by column, [5] slots that scanned their WHOLE bucket (the rest re-scored candidates)
    if (!strcmp(name, "pf_fallback")) b = &h->fb_list;
    if (!b) return fail("lmi_debug_peek: unknown buffer '%s'", name);
    if (bytes < 0 || off + (size_t)bytes > b->cap) return fail("lmi_debug_peek: %lld bytes asked of a %zu-byte buffer", (long long)bytes, b->cap);
    if (bytes) HIPCHK(hipMemcpy(dst, static_cast<char*>(b->p) + off, (size_t)bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" LMI_API int lmi_scan_stats(lmi_index* h, double* flops, int64_t* pairs, int64_t* items) {
    if (!h) return fail("lmi_scan_stats: NULL handle");
    CHK(set_dev(h));
    if (h->stats_pending) {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(h->h_stats, h->stats.p, 32, hipMemcpyDeviceToHost));
        h->stats_pending = false;
    }
    if (pairs) *pairs = h->h_stats[0];
    if (items) *items = h->h_stats[1];
    if (flops) *flops = 2.0 * h->d * (double)h->h_stats[0];
    return 0;
}
