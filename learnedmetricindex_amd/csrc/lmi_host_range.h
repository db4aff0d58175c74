// lmi_host_range.h -- the range search: every candidate of the union scan within a radius, in ordinal order (kernels: lmi_range.h;
// the offsets, lims and gathers: lmi_range_plan.h; include/lmi_hip.h states the contract).  The plan, the tables and the scores are the
// candidate stage's (lmi_host_candidates.h), opened with the smallest list since no lists are kept; the front of the three forms is
// the union scan's (UnionFront, lmi_host_union.h).  Per wave: the stage's scores, count; the wave's counts come back to the host (ONE
// synchronisation per wave); a chunk of exactly the wave's results is allocated, the slots' offsets go up, emit.  Behind the last
// group the final arrays are allocated once at lims[nq] and every wave's runs are gathered (one descriptor table for all of them, one
// synchronisation).
// lmi_scan_range, lmi_search_range, lmi_search_tree_range, lmi_range_result_*, lmi_debug_range_plan.  A result keeps the call's nb and
// the counts of every (query, rank): what the join of the ranks' parts (lmi_host_range_join.h) is planned from.
#pragma once
#include "lmi_host_union.h"
#include "lmi_range.h"
#include "lmi_range_plan.h"

// A call's results: the device arrays and the host lims.  It holds no pointer to the handle it was made on and may outlive it.
struct lmi_range_result {
    int device = 0;
    std::vector<int64_t> lims;   // [nq + 1]
    int nb = 0;                  // the ranks per query of the call that made it
    std::vector<int> pair_count; // [nq][nb]: the results of every (query, rank); row q sums to lims[q + 1] - lims[q]
    float* dists = nullptr;      // [lims[nq]], device
    uint32_t* ids = nullptr;
    bool sorted = false;         // lmi_range_result_sort has run: every segment is in distance order, no longer in (rank, row) order
    ~lmi_range_result() {
        if (dists) (void)hipFree(dists);
        if (ids) (void)hipFree(ids);
    }
};

namespace {

thread_local int64_t g_range_last[LMI_RANGE_PLAN_COUNT] = {};

// how every form begins: the plan words cleared, then the refusals that need no launch
int range_begin(lmi_index* h, const char* who, int nq, int nb, const float* radius, const lmi_filter* f, const int32_t* filter_of,
                int64_t max_total, lmi_range_result** out) {
    for (int64_t& w : g_range_last) w = 0;
    if (out) *out = nullptr;
    if (!h) return fail("%s: NULL handle", who);
    CHK(union_check(h, who, nq, nb, 1));
    if (!out) return fail("%s: the result pointer is NULL", who);
    if (!radius && nq > 0) return fail("%s: radius is NULL", who);
    if (max_total < 0) return fail("%s: max_total %lld is negative", who, (long long)max_total);
    if (f) CHK(filter_check(h, who, f, filter_of, nq));
    else if (filter_of) return fail("%s: filter_of without a filter", who);
    return 0;
}

int range_empty(lmi_index* h, int nq, int nb, lmi_range_result** out) {
    lmi_range_result* r = new lmi_range_result();
    r->device = h->device;
    r->nb = nb;
    r->lims.assign((size_t)nq + 1, 0);
    *out = r;
    return 0;
}

// d_qs [nq][d_user] and d_order [nq][nb] on the device, already enqueued on h->stream; radius [nq] on the host.
int range_core(lmi_index* h, const char* who, const float* d_qs, int nq, const int* d_order, int nb, const float* radius,
               const lmi_filter* f, const int32_t* filter_of, int64_t max_total, lmi_range_result** out) {
    namespace up = lmi_union_plan;
    namespace rp = lmi_range_plan;
    hipStream_t st = h->stream;
    CandidateStage S(h, who);
    CHK(S.open(d_qs, nq, d_order, nb, rp::PLAN_K, true, f, filter_of));
    const up::Plan& p = S.p;
    const std::vector<up::Tables>& groups = S.groups;
    const int64_t max_slots = S.ext.group_slots;
    CallScratch chunks(who);
    float* d_radius = nullptr;
    int *d_slot_q = nullptr, *d_counts = nullptr;
    long long *d_slot_pos0 = nullptr, *d_slot_off = nullptr;
    CHK(S.mem.alloc(&d_slot_q, (size_t)max_slots * 4, "slot queries"));
    CHK(S.mem.alloc(&d_slot_pos0, (size_t)max_slots * 8, "slot positions"));
    CHK(S.mem.alloc(&d_slot_off, (size_t)max_slots * 8, "slot offsets"));
    CHK(S.mem.alloc(&d_counts, (size_t)max_slots * 4, "slot counts"));
    CHK(S.mem.alloc(&d_radius, (size_t)nq * 4, "radius"));
    HIPCHK(hipMemcpyAsync(d_radius, radius, (size_t)nq * 4, hipMemcpyHostToDevice, st));

    // what a wave leaves behind for the gather: its chunk and, per slot, the count and the offset inside the chunk
    struct WaveOut {
        float* D = nullptr;
        unsigned* I = nullptr;
        int64_t total = 0;
        std::vector<int> counts;
        std::vector<long long> off;
    };
    std::vector<std::vector<WaveOut>> outs(groups.size());
    rp::Totals tot(nq, nb);
    int64_t counted = 0, chunk_bytes = 0;
    const unsigned* d_mask = f ? f->mask.as<unsigned>() : nullptr;
    for (size_t g = 0; g < groups.size(); ++g) {
        const up::Tables& G = groups[g];
        CHK(S.upload(G));
        CHK(S.up(d_slot_q, G.scan_q.data(), G.scan_q.size() * 4));
        CHK(S.up(d_slot_pos0, G.scan_pos0.data(), G.scan_pos0.size() * 8));
        outs[g].resize(G.waves.size());
        for (size_t w = 0; w < G.waves.size(); ++w) {
            const up::Wave& W = G.waves[w];
            WaveOut& O = outs[g][w];
            if (W.slots == 0) continue;
            CHK(S.score(W));
            const long long* smask = f ? S.d_slot_mask + W.slot0 : nullptr;
            range_count_kernel<<<(int)W.slots, 64, 0, st>>>(S.d_S, S.d_slots + W.slot0, d_slot_q + W.slot0, smask, d_mask, S.C.qn2, d_radius,
                                                           d_counts + W.slot0);
            HIPCHK(hipGetLastError());
            O.counts.assign((size_t)W.slots, 0);
            O.off.assign((size_t)W.slots, 0);
            HIPCHK(hipMemcpyAsync(O.counts.data(), d_counts + W.slot0, (size_t)W.slots * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));   // the wave's one synchronisation: its counts size its chunk
            O.total = rp::chunk_offsets(O.counts.data(), W.slots, O.off.data());
            counted += rp::add_wave(tot, p, G, W, O.counts.data());
            if (rp::over_total(counted, max_total))
                return fail("%s: more than max_total = %lld results: %lld had been counted when the call stopped (group %lld of %lld, wave %lld of "
                            "%lld); nothing further was launched",
                            who, (long long)max_total, (long long)counted, (long long)g + 1, (long long)groups.size(), (long long)w + 1,
                            (long long)G.waves.size());
            if (O.total == 0) continue;
            CHK(chunks.alloc(&O.D, (size_t)O.total * 4, "result chunk (dists)"));
            CHK(chunks.alloc(&O.I, (size_t)O.total * 4, "result chunk (ids)"));
            chunk_bytes += O.total * 8;
            CHK(S.up(d_slot_off + W.slot0, O.off.data(), (size_t)W.slots * 8));
            range_emit_kernel<<<(int)W.slots, 64, 0, st>>>(S.d_S, S.d_slots + W.slot0, d_slot_q + W.slot0, smask, d_mask, S.C.qn2, d_radius,
                                                          d_counts + W.slot0, d_slot_off + W.slot0, d_slot_pos0 + W.slot0,
                                                          h->ids_slab.as<unsigned>(), O.D, O.I);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(st));   // the next group rewrites the tables
    }

    const std::vector<int64_t> first = rp::run_starts(tot);
    lmi_range_result* r = new lmi_range_result();
    r->device = h->device;
    r->lims = rp::make_lims(tot, first);
    r->nb = nb;
    r->pair_count = tot.pair_count;
    const int64_t total = r->lims.back();
    // the gathers: every wave's descriptors back to back in one table, one upload, one launch per wave that produced results
    auto finish = [&]() -> int {
        if (total == 0) return 0;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&r->dists), (size_t)total * 4));
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&r->ids), (size_t)total * 4));
        rp::Gather all;
        std::vector<std::vector<size_t>> at(groups.size());
        for (size_t g = 0; g < groups.size(); ++g)
            for (size_t w = 0; w < groups[g].waves.size(); ++w) {
                at[g].push_back(all.n.size());
                const WaveOut& O = outs[g][w];
                if (O.total == 0) continue;
                const rp::Gather one = rp::gather_of(p, groups[g], groups[g].waves[w], O.counts.data(), O.off.data(), first);
                all.src.insert(all.src.end(), one.src.begin(), one.src.end());
                all.dst.insert(all.dst.end(), one.dst.begin(), one.dst.end());
                all.n.insert(all.n.end(), one.n.begin(), one.n.end());
            }
        long long *d_src = nullptr, *d_dst = nullptr;
        int* d_n = nullptr;
        CHK(S.mem.alloc(&d_src, all.src.size() * 8, "run sources"));
        CHK(S.mem.alloc(&d_dst, all.dst.size() * 8, "run targets"));
        CHK(S.mem.alloc(&d_n, all.n.size() * 4, "run lengths"));
        CHK(S.up(d_src, all.src.data(), all.src.size() * 8));
        CHK(S.up(d_dst, all.dst.data(), all.dst.size() * 8));
        CHK(S.up(d_n, all.n.data(), all.n.size() * 4));
        for (size_t g = 0; g < groups.size(); ++g)
            for (size_t w = 0; w < groups[g].waves.size(); ++w) {
                const WaveOut& O = outs[g][w];
                if (O.total == 0) continue;
                const size_t a = at[g][w];
                range_gather_kernel<<<(int)groups[g].waves[w].slots, 64, 0, st>>>(O.D, O.I, d_src + a, d_dst + a, d_n + a, r->dists, r->ids);
                HIPCHK(hipGetLastError());
            }
        HIPCHK(hipStreamSynchronize(st));   // the result is complete; the descriptors and the chunks may go
        return 0;
    };
    if (finish() != 0) {
        (void)hipStreamSynchronize(st);
        delete r;
        return -1;
    }
    g_range_last[LMI_RANGE_PLAN_GROUPS] = p.query_groups;
    g_range_last[LMI_RANGE_PLAN_QUERY_ROWS] = p.query_rows;
    g_range_last[LMI_RANGE_PLAN_WAVES] = (int64_t)groups.back().waves.size();
    g_range_last[LMI_RANGE_PLAN_SLAB_BYTES] = S.ext.slab_bytes;
    g_range_last[LMI_RANGE_PLAN_RESULTS] = total;
    g_range_last[LMI_RANGE_PLAN_CHUNK_BYTES] = chunk_bytes;
    g_range_last[LMI_RANGE_PLAN_WORKSPACE_BYTES] = S.mem.total;
    *out = r;
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_debug_range_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_range_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_RANGE_PLAN_COUNT); ++i) out[i] = g_range_last[i];
    return 0;
}

// every range entry point: a, b as UnionFront states them.  A copy back that fails takes the result with it.
static int range_call(UnionForm form, const char* who, lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb,
                      const float* radius, const lmi_filter* f, const int32_t* filter_of, int64_t max_total, lmi_range_result** result,
                      int32_t* a, int32_t* b, int on_device) {
    CHK(range_begin(h, who, nq, nb, radius, f, filter_of, max_total, result));
    UnionFront F{form, a, b};
    CHK(F.open(h, who, queries_nav, queries_search, nq, nb, on_device, true, nullptr));
    if (nq == 0) return range_empty(h, nq, nb, result);
    CHK(range_core(h, who, F.d_qs, nq, F.d_order, nb, radius, f, filter_of, max_total, result));
    if (F.close(h, on_device) != 0) {
        delete *result;
        *result = nullptr;
        return -1;
    }
    return 0;
}
extern "C" LMI_API int lmi_scan_range(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, const float* radius,
                                      const lmi_filter* f, const int32_t* filter_of, int64_t max_total, lmi_range_result** result,
                                      int on_device) {
    return range_call(ORDER_GIVEN, "lmi_scan_range", h, nullptr, queries_search, nq, nb, radius, f, filter_of, max_total, result,
                      const_cast<int32_t*>(bucket_order), nullptr, on_device);
}
extern "C" LMI_API int lmi_search_range(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, const float* radius,
                                        const lmi_filter* f, const int32_t* filter_of, int64_t max_total, lmi_range_result** result,
                                        int32_t* bucket_order, int on_device) {
    return range_call(ORDER_MLP, "lmi_search_range", h, queries_nav, queries_search, nq, nb, radius, f, filter_of, max_total, result, bucket_order,
                      nullptr, on_device);
}
extern "C" LMI_API int lmi_search_tree_range(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb,
                                             const float* radius, const lmi_filter* f, const int32_t* filter_of, int64_t max_total,
                                             lmi_range_result** result, int32_t* slab_ids, int32_t* entries, int on_device) {
    return range_call(ORDER_TREE, "lmi_search_tree_range", h, queries_nav, queries_search, nq, nb, radius, f, filter_of, max_total, result, slab_ids,
                      entries, on_device);
}

extern "C" LMI_API int lmi_range_result_total(const lmi_range_result* r, int64_t* total) {
    if (!r || !total) return fail("lmi_range_result_total: NULL argument");
    *total = r->lims.back();
    return 0;
}
extern "C" LMI_API int lmi_range_result_lims(const lmi_range_result* r, int64_t* lims) {
    if (!r || !lims) return fail("lmi_range_result_lims: NULL argument");
    std::copy(r->lims.begin(), r->lims.end(), lims);
    return 0;
}
extern "C" LMI_API int lmi_range_result_pair_counts(const lmi_range_result* r, int32_t* nb, int32_t* counts) {
    if (!r) return fail("lmi_range_result_pair_counts: NULL result");
    if (nb) *nb = r->nb;
    if (counts) std::copy(r->pair_count.begin(), r->pair_count.end(), counts);
    return 0;
}
extern "C" LMI_API int lmi_range_result_read(const lmi_range_result* r, float* dists, uint32_t* ids, int on_device) {
    if (!r) return fail("lmi_range_result_read: NULL result");
    const int64_t total = r->lims.back();
    if (total == 0) return 0;
    if (!dists || !ids) return fail("lmi_range_result_read: dists and ids must not be NULL (the result holds %lld)", (long long)total);
    HIPCHK(hipSetDevice(r->device));
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpy(dists, r->dists, (size_t)total * 4, kind));
    HIPCHK(hipMemcpy(ids, r->ids, (size_t)total * 4, kind));
    if (on_device) HIPCHK(hipDeviceSynchronize());
    return 0;
}
extern "C" LMI_API int lmi_range_result_destroy(lmi_range_result* r) {
    if (!r) return 0;
    (void)hipSetDevice(r->device);
    delete r;
    return 0;
}
