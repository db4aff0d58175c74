// lmi_host_range_sort.h -- a range result sorted by distance on the device: lmi_range_result_sort, lmi_range_result_sorted, the
// geometry hook and the plan words (kernels: lmi_range_sort.h; the arithmetic: lmi_range_sort_plan.h; include/lmi_hip.h states the
// contract).  The handle provides the device and the stream; the result is any lmi_range_result of that device -- a scan's or a join's.
// Per group of whole segments: the scratch is allocated, the group's entries are copied into the permuted copy (so that a skipped
// segment's entries are there too), the forms' kernels overwrite every sorted segment of the copy, the copy goes back over the group's
// entries, ONE synchronisation, the scratch is freed.
#pragma once
#include "lmi_host_range.h"
#include "lmi_range_sort.h"
#include "lmi_range_sort_plan.h"

namespace {

thread_local int64_t g_range_sort_tile_rows = 0;       // 0: lmi_range_sort_plan::DEFAULT_TILE_ROWS
thread_local int64_t g_range_sort_scratch_bytes = 0;   // 0: lmi_range_sort_plan::DEFAULT_SCRATCH_BYTES
thread_local int64_t g_range_sort_last[LMI_RANGE_SORT_PLAN_COUNT] = {};

// one group: everything is enqueued on h->stream; returns when the group's entries are sorted
int range_sort_group(lmi_index* h, const char* who, lmi_range_result* r, const lmi_range_sort_plan::Plan& P,
                     const lmi_range_sort_plan::Group& G) {
    hipStream_t st = h->stream;
    const int64_t g0 = G.e0, entries = G.e1 - G.e0;
    const size_t nw = G.wave_n.size(), nt = G.tile_n.size();
    CallScratch mem(who);
    float* cD = nullptr;
    unsigned* cI = nullptr;
    unsigned long long *kA = nullptr, *kB = nullptr;
    long long *d_wave_at = nullptr, *d_tile_at = nullptr;
    int *d_wave_n = nullptr, *d_tile_n = nullptr;
    CHK(mem.alloc(&cD, (size_t)entries * 4, "permuted copy (dists)"));
    CHK(mem.alloc(&cI, (size_t)entries * 4, "permuted copy (ids)"));
    if (G.longest > 0) {
        CHK(mem.alloc(&kA, (size_t)G.longest * 8, "key buffer"));
        CHK(mem.alloc(&kB, (size_t)G.longest * 8, "second key buffer"));
    }
    if (nw) {
        CHK(mem.alloc(&d_wave_at, nw * 8, "wave segments"));
        CHK(mem.alloc(&d_wave_n, nw * 4, "wave lengths"));
    }
    if (nt) {
        CHK(mem.alloc(&d_tile_at, nt * 8, "tile segments"));
        CHK(mem.alloc(&d_tile_n, nt * 4, "tile lengths"));
    }
    // from here on the result is only read until the copy goes back
    HIPCHK(hipMemcpyAsync(cD, r->dists + g0, (size_t)entries * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(cI, r->ids + g0, (size_t)entries * 4, hipMemcpyDeviceToDevice, st));
    if (nw) {
        HIPCHK(hipMemcpyAsync(d_wave_at, G.wave_at.data(), nw * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_wave_n, G.wave_n.data(), nw * 4, hipMemcpyHostToDevice, st));
        range_sort_wave_kernel<<<cdiv((long long)nw, RANGE_SORT_BLOCK / 64), RANGE_SORT_BLOCK, 0, st>>>(d_wave_at, d_wave_n, (int)nw, r->dists,
                                                                                                     r->ids, g0, cD, cI);
        HIPCHK(hipGetLastError());
    }
    if (nt) {
        const int64_t longest = *std::max_element(G.tile_n.begin(), G.tile_n.end());
        HIPCHK(hipMemcpyAsync(d_tile_at, G.tile_at.data(), nt * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_tile_n, G.tile_n.data(), nt * 4, hipMemcpyHostToDevice, st));
        range_sort_tile_kernel<<<(unsigned)nt, RANGE_SORT_BLOCK, (size_t)lmi_range_sort_plan::padded(longest) * 8, st>>>(
            d_tile_at, d_tile_n, r->dists, r->ids, g0, cD, cI);
        HIPCHK(hipGetLastError());
    }
    const int T = (int)P.tile_rows, M = (int)P.merge_rows;
    for (const lmi_range_sort_plan::LongSeg& S : G.longs) {
        range_sort_runs_kernel<<<(unsigned)S.tiles, RANGE_SORT_BLOCK, (size_t)T * 8, st>>>(r->dists, S.at, S.n, T, kA);
        HIPCHK(hipGetLastError());
        unsigned long long *src = kA, *dst = kB;
        for (int64_t run = T; run < S.n; run <<= 1) {
            range_sort_merge_kernel<<<(unsigned)S.pieces, RANGE_SORT_BLOCK, (size_t)M * 8, st>>>(src, S.n, run, M, dst);
            HIPCHK(hipGetLastError());
            std::swap(src, dst);
        }
        range_sort_apply_kernel<<<(unsigned)cdiv(S.n, RANGE_SORT_BLOCK), RANGE_SORT_BLOCK, 0, st>>>(src, S.at, S.n, r->dists, r->ids, g0, cD, cI);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(r->dists + g0, cD, (size_t)entries * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(r->ids + g0, cI, (size_t)entries * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st));   // the group's one synchronisation: its segments are sorted, the scratch may go
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_range_sort_set_geometry(int64_t tile_rows, int64_t scratch_bytes) {
    namespace sp = lmi_range_sort_plan;
    if (tile_rows < 0 || scratch_bytes < 0)
        return fail("lmi_range_sort_set_geometry: negative value (tile_rows %lld, scratch_bytes %lld)", (long long)tile_rows,
                    (long long)scratch_bytes);
    if (!sp::tile_rows_ok(tile_rows))
        return fail("lmi_range_sort_set_geometry: tile_rows %lld is not a power of two in [%lld, %lld]", (long long)tile_rows,
                    (long long)sp::MIN_TILE_ROWS, (long long)sp::MAX_TILE_ROWS);
    if (!sp::scratch_bytes_ok(scratch_bytes))
        return fail("lmi_range_sort_set_geometry: scratch_bytes %lld above 2^40", (long long)scratch_bytes);
    g_range_sort_tile_rows = tile_rows;
    g_range_sort_scratch_bytes = scratch_bytes;
    return 0;
}

extern "C" LMI_API int lmi_debug_range_sort_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_range_sort_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_RANGE_SORT_PLAN_COUNT); ++i) out[i] = g_range_sort_last[i];
    return 0;
}

extern "C" LMI_API int lmi_range_result_sorted(const lmi_range_result* r, int* sorted) {
    if (!r || !sorted) return fail("lmi_range_result_sorted: NULL argument");
    *sorted = r->sorted ? 1 : 0;
    return 0;
}

extern "C" LMI_API int lmi_range_result_sort(lmi_index* h, lmi_range_result* r) {
    namespace sp = lmi_range_sort_plan;
    const char* who = "lmi_range_result_sort";
    for (int64_t& w : g_range_sort_last) w = 0;
    if (!h) return fail("%s: NULL handle", who);
    if (!r) return fail("%s: NULL result", who);
    if (r->device != h->device) return fail("%s: the result is on device %d, the handle on device %d", who, r->device, h->device);
    const int64_t nq = (int64_t)r->lims.size() - 1;
    sp::Plan P;
    const sp::Verdict v = sp::make_plan(r->lims.data(), nq, g_range_sort_tile_rows, g_range_sort_scratch_bytes, P);
    switch (v.problem) {
    case sp::OK: break;
    case sp::BAD_LIMS: return fail("%s: the limits of query %lld descend (%lld)", who, (long long)v.q, (long long)v.value);
    case sp::SEGMENT_TOO_LONG:
        return fail("%s: query %lld has %lld results: a segment of 2^32 entries or more is not sorted (the position is a 32-bit word); "
                    "nothing was launched", who, (long long)v.q, (long long)v.value);
    }
    for (const sp::Group& G : P.groups)
        if ((long long)G.wave_n.size() >= (1ll << 31) || (long long)G.tile_n.size() >= (1ll << 31))
            return fail("%s: a group of %zu + %zu segments is more than one launch takes; lower scratch_bytes", who, G.wave_n.size(),
                        G.tile_n.size());
    if (!P.groups.empty()) {
        CHK(set_dev(h));
        // the tile forms' dynamic LDS reaches 64 KiB at the default T
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&range_sort_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sp::MAX_TILE_ROWS * 8)));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&range_sort_runs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sp::MAX_TILE_ROWS * 8)));
        for (const sp::Group& G : P.groups)
            if (range_sort_group(h, who, r, P, G) != 0) {
                (void)hipStreamSynchronize(h->stream);   // no kernel may still read the scratch that frees itself
                return -1;
            }
    }
    r->sorted = true;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_GROUPS] = (int64_t)P.groups.size();
    g_range_sort_last[LMI_RANGE_SORT_PLAN_WAVE_SEGMENTS] = P.waves;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_TILE_SEGMENTS] = P.tiles;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_LONG_SEGMENTS] = P.longs;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_SKIPPED_SEGMENTS] = P.skipped;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_TILE_ROWS] = P.tile_rows;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_WAVE_ROWS] = P.wave_rows;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_MERGE_ROWS] = P.merge_rows;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_MAX_PASSES] = P.max_passes;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_SCRATCH_BYTES] = P.scratch_bytes;
    g_range_sort_last[LMI_RANGE_SORT_PLAN_RESULTS] = P.total;
    return 0;
}
