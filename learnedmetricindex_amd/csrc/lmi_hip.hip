// lmi_hip.hip -- host side of liblmi_hip.so: the C ABI declared in include/lmi_hip.h, one translation unit.
// Owns the device-resident index (fragment-major slab, ids, CSR of buckets), the packed MLP weights and the per-call
// workspaces; enqueues the kernels of lmi_kernels.h .. lmi_train.h on one HIP stream.  This file: handle creation,
// destruction, clone views and the setters; everything else in the lmi_host*.h headers.
#include "lmi_host.h"         // the kernel headers, the handle (lmi_handle.h: error macros, DevBuf), per-call helpers
#include "lmi_host_call.h"    // open_device; the scratch and the uploads of the calls that take no handle
#include "lmi_host_model.h"   // model packing, MLP forward, tree navigation
#include "lmi_host_build.h"   // lmi_buckets_begin / add_rows / end, bucket read
#include "lmi_host_mutate.h"  // lmi_buckets_insert / lmi_buckets_delete
#include "lmi_host_subset.h"  // lmi_subset
#include "lmi_host_scan.h"    // scan_plan, the scan's stages, scan_enqueue, lmi_workspace_bytes
#include "lmi_host_search.h"  // lmi_scan_topk / lmi_search / lmi_search_tree / lmi_knn_ip, lmi_pipeline_submit
#include "lmi_host_comm.h"    // lmi_merge_gathered, RCCL; lmi_merge_union_parts, lmi_allgather_merge_union (lmi_union_merge.h)
#include "lmi_host_debug.h"   // timings, statistics, test hooks
#include "lmi_kmeans.h"       // the kernels of lmi_kmeans
#include "lmi_host_kmeans.h"  // lmi_kmeans
#include "lmi_train.h"        // the kernels of lmi_train
#include "lmi_host_train.h"   // lmi_train
#include "lmi_knn.h"          // the kernels of lmi_knn
#include "lmi_host_knn.h"     // lmi_knn, lmi_knn_set_geometry, lmi_debug_knn_plan
#include "lmi_union.h"        // the kernels of the union scan
#include "lmi_filter.h"       // the kernels of the filter sets and the masked select of the filtered union scan
#include "lmi_host_candidates.h"   // the candidate stage of the union scan and the range search: plan, tables, buffers, pack and score
#include "lmi_host_union.h"   // lmi_scan_union / lmi_scan_union_part / lmi_search_union / lmi_search_tree_union, geometry and plan hooks; the *_filtered forms (lmi_host_filter.h); the front of the three forms
#include "lmi_range.h"        // the kernels of the range search
#include "lmi_host_range.h"   // lmi_scan_range / lmi_search_range / lmi_search_tree_range, lmi_range_result_*, lmi_debug_range_plan
#include "lmi_knn_range.h"    // the kernels of lmi_knn_range
#include "lmi_host_knn_range.h"   // lmi_knn_range, lmi_debug_knn_range_plan
#include "lmi_range_join.h"   // the kernel of the join of range parts
#include "lmi_host_range_join.h"   // lmi_join_range_parts / lmi_allgather_join_range, lmi_range_join_set_geometry, lmi_debug_range_join_plan
#include "lmi_range_sort.h"   // the kernels of the sort of a range result by distance
#include "lmi_host_range_sort.h"   // lmi_range_result_sort / lmi_range_result_sorted, lmi_range_sort_set_geometry, lmi_debug_range_sort_plan
#include "lmi_regroup.h"        // the kernels of lmi_regroup (its sort merges with lmi_range_sort.h's kernel)
#include "lmi_host_regroup.h"   // lmi_regroup, lmi_regroup_set_geometry, lmi_debug_regroup_plan
#include "lmi_concat.h"         // the kernels of lmi_concat
#include "lmi_host_concat.h"    // lmi_concat, lmi_debug_concat_plan
#include "lmi_fetch.h"          // the kernels of lmi_rows_fetch
#include "lmi_host_fetch.h"     // lmi_rows_fetch / lmi_rows_fetch_f16, lmi_fetch_set_geometry, lmi_debug_fetch_plan
#include "lmi_cover.h"          // the kernels of the bucket cover and of the pruning pass
#include "lmi_host_cover.h"     // lmi_cover_create / _destroy / _read, lmi_cover_order, lmi_search_range_exact, lmi_cover_set_geometry, lmi_debug_cover_plan
#include <mutex>

extern "C" LMI_API int lmi_abi_version(void) { return LMI_ABI_VERSION; }
#ifndef LMI_SOURCE_SHA16
#define LMI_SOURCE_SHA16 "unknown"
#endif
#define LMI_STR2(x) #x
#define LMI_STR(x) LMI_STR2(x)
extern "C" LMI_API const char* lmi_build_info(void) {
    return "src=" LMI_SOURCE_SHA16 " p2_waves=" LMI_STR(LMI_P2_WAVES) " p2_bring=" LMI_STR(LMI_P2_BR) " pf_cap=" LMI_STR(LMI_PF_CAP);
}
extern "C" LMI_API const char* lmi_last_error(void) { return g_err.c_str(); }

extern "C" LMI_API int lmi_create(int device, lmi_index** out) {
    if (!out) return fail("lmi_create: out is NULL");
    hipDeviceProp_t prop;
    CHK(open_device("lmi_create", device, &prop));
    lmi_index* h = new lmi_index();
    h->device = device;
    h->num_cus = prop.multiProcessorCount;
    // route_group_kernel sorts the buckets in dynamic LDS (route_group_lds: fan-outs up to ROUTE_MAX_BUCKETS)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&route_group_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));  // its static LDS: 4 bytes
    int occ = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, scan_kernel, 256, SCAN_LDS));
    h->scan_blocks_per_cu = std::max(1, std::min(occ, RB == 1 ? 2 : 1));
    // the timing events are created on first use (record): a handle that lives for one lmi_knn_ip call
    // touches 4 of the ring's 1 280
    {   // fp16 subnormal self-test (lmi_prefilter.h): the error bound of the prefilter relies on it
        static std::mutex mu;    // per process; every MI355X behaves the same
        static int cached = -1;
        std::lock_guard<std::mutex> lock(mu);
        if (cached < 0) {
            int* d_ok = nullptr;
            int ok = 0;
            HIPCHK(hipMalloc(&d_ok, sizeof(int)));
            pf_selftest_kernel<<<1, 64>>>(d_ok);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy(&ok, d_ok, sizeof(int), hipMemcpyDeviceToHost));
            HIPCHK(hipFree(d_ok));
            cached = ok;
        }
        h->pf_hw_ok = cached == 1;
        if (!h->pf_hw_ok) h->prefilter = false;
    }
    if (const char* e = getenv("LMI_RESCORE_SIMPLE")) h->rescore_streamed = !(e[0] && e[0] != '0');
    if (const char* e = getenv("LMI_PF_NO_REDO")) h->pf_redo = !(e[0] && e[0] != '0');
    if (const char* e = getenv("LMI_PF_SMALL")) h->pf_small = !(e[0] == '0');
    if (const char* e = getenv("LMI_PF_QBOUND")) h->pf_qbound = e[0] && e[0] != '0';
    if (const char* e = getenv("LMI_PF_PRIMARY")) h->pf_primary = e[0] && e[0] != '0';
    if (const char* e = getenv("LMI_PS_WIDE")) h->ps_force_wide = e[0] == '1' ? 1 : e[0] == '0' ? 0 : -1;
    if (const char* e = getenv("LMI_FRONT")) h->use_front = !(e[0] == '0');
    if (const char* e = getenv("LMI_P2_GRADED")) h->graded_chunks = !(e[0] == '0');
    if (const char* e = getenv("LMI_P2_CHUNKS")) (void)sscanf(e, "%d,%d,%d", &h->chunk_lvl_rows[0], &h->chunk_lvl_rows[1], &h->chunk_lvl_rows[2]);
    if (const char* e = getenv("LMI_P2_CHUNK_FRAC")) (void)sscanf(e, "%f,%f", &h->chunk_frac[0], &h->chunk_frac[1]);
    if (const char* e = getenv("LMI_TAIL")) h->use_tail = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
    if (const char* e = getenv("LMI_FR_DEBUG")) { if (e[0] == '1') { CHK(h->fr_dbg.reserve(256)); HIPCHK(hipMemset(h->fr_dbg.p, 0, 256)); } }
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) h->wall_khz = (double)khz;
    }
    // per handle = per device (a process may hold handles on several devices; the attribute is per device)
#define LMI_PS_ATTR(K) \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pass2_small_kernel<K, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, ps_lds_bytes(K, false))); \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pass2_small_kernel<K, true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, ps_lds_bytes(K, false))); \
    if constexpr (ps_has_wide(K)) { \
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pass2_small_kernel<K, false, ps_has_wide(K)>), hipFuncAttributeMaxDynamicSharedMemorySize, ps_lds_bytes(K, true))); \
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&pass2_small_kernel<K, true, ps_has_wide(K)>), hipFuncAttributeMaxDynamicSharedMemorySize, ps_lds_bytes(K, true))); \
    }
    // every K: the dynamic part alone stays under 64 KiB up to K = 5, but the static arrays beside it (queue prefix, candidate
    // list, item) put the block's total above it from K = 5 on
    LMI_PS_ATTR(1) LMI_PS_ATTR(2) LMI_PS_ATTR(3) LMI_PS_ATTR(4) LMI_PS_ATTR(5) LMI_PS_ATTR(6) LMI_PS_ATTR(7) LMI_PS_ATTR(8)
#undef LMI_PS_ATTR
#define LMI_RC_ATTR(GV) \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rescore_kernel<GV, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rescore_kernel<GV, true>), hipFuncAttributeMaxDynamicSharedMemorySize, RC_SMALL_LDS_CAP));
    LMI_RC_ATTR(1) LMI_RC_ATTR(2) LMI_RC_ATTR(3) LMI_RC_ATTR(4)
#undef LMI_RC_ATTR
#define LMI_TL_ATTR(GV) \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tail_kernel<GV>), hipFuncAttributeMaxDynamicSharedMemorySize, RC_SMALL_LDS_CAP));
    LMI_TL_ATTR(1) LMI_TL_ATTR(2) LMI_TL_ATTR(3) LMI_TL_ATTR(4)
#undef LMI_TL_ATTR
    *out = h;
    return 0;
}

extern "C" LMI_API int lmi_destroy(lmi_index* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->parent) h->parent->live_clones--;
    if (h->side) {
        (void)hipStreamSynchronize(h->side);
        (void)hipStreamDestroy(h->side);
        (void)hipEventDestroy(h->side_fork);
        (void)hipEventDestroy(h->side_join);
    }
    if (h->h_oflag) (void)hipHostFree(h->h_oflag);
    for (int r = 0; r < lmi_index::EV_RING; ++r)
        for (int i = 0; i < 10; ++i)
            if (h->ev_ring[r][i]) (void)hipEventDestroy(h->ev_ring[r][i]);
    delete h;   // every DevBuf frees what it owns
    return 0;
}

// A second handle on the SAME index: its MLP weights, tree and bucket slabs are the parent's memory (borrowed), its
// per-call workspaces, stream, side stream and timing events are its own.  Two searches can then be in flight on one
// index (one per handle, each on its own stream): the pipeline alternates handles so that a batch's kernels start in
// the tails of the previous batch's.  The clone must be destroyed before the parent and the parent's index must not be
// rebuilt while it lives.
extern "C" LMI_API int lmi_clone_view(lmi_index* h, lmi_index** out) {
    if (!h || !out) return fail("lmi_clone_view: NULL argument");
    if (h->building) return fail("lmi_clone_view: the parent's index is being built");
    CHK(set_dev(h));
    CHK(build_descs(h));                       // the device copy of the model descriptors is shared as it stands
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = clone_handle(h);
    return 0;
}

extern "C" LMI_API int lmi_set_stream(lmi_index* h, void* s) {
    if (!h) return fail("lmi_set_stream: NULL handle");
    h->stream = reinterpret_cast<hipStream_t>(s);
    return 0;
}

extern "C" LMI_API int lmi_set_chunk_rows(lmi_index* h, int rows) {
    if (!h) return fail("lmi_set_chunk_rows: NULL handle");
    if (rows < P2_TILE_ROWS || rows % P2_TILE_ROWS) return fail("lmi_set_chunk_rows: rows must be a positive multiple of %d", P2_TILE_ROWS);
    if (h->building || h->built) return fail("lmi_set_chunk_rows: must be called before lmi_buckets_begin");
    h->chunk_rows = rows;
    h->chunk_rows_set = rows;
    h->chunk_rows_auto = false;
    return 0;
}

extern "C" LMI_API int lmi_set_metric(lmi_index* h, int metric) {
    if (!h) return fail("lmi_set_metric: NULL handle");
    if (metric != LMI_METRIC_IP && metric != LMI_METRIC_L2) return fail("lmi_set_metric: unknown metric %d", metric);
    if ((h->built || h->building) && metric != h->metric) return fail("lmi_set_metric: the metric is fixed once lmi_buckets_begin has run");
    h->metric = metric;
    return 0;
}

extern "C" LMI_API int lmi_set_storage(lmi_index* h, int storage) {
    if (!h) return fail("lmi_set_storage: NULL handle");
    if (storage != LMI_STORAGE_F32 && storage != LMI_STORAGE_F16)
        return fail("lmi_set_storage: unknown storage %d (LMI_STORAGE_F32 = 0, LMI_STORAGE_F16 = 1)", storage);
    if (h->building) return fail("lmi_set_storage: an index is being built; the storage is chosen before lmi_buckets_begin");
    if (h->parent) return fail("lmi_set_storage: a clone view builds no index");
    if (storage == LMI_STORAGE_F16)
        if (const char* why = storage16_conflict(h)) return fail("lmi_set_storage: LMI_STORAGE_F16: %s", why);
    h->storage_req = storage;
    return 0;
}

extern "C" LMI_API int lmi_index_bytes(lmi_index* h, int64_t* bytes) {
    if (!h || !bytes) return fail("lmi_index_bytes: NULL argument");
    if (!h->building && !h->built) return fail("lmi_index_bytes: no index (valid from lmi_buckets_begin on)");
    *bytes = h->index_bytes();
    return 0;
}

extern "C" LMI_API int lmi_set_prefilter(lmi_index* h, int on) {
    if (!h) return fail("lmi_set_prefilter: NULL handle");
    if ((h->built || h->building) && (on != 0) != h->prefilter)
        return fail("lmi_set_prefilter: the mode is fixed once lmi_buckets_begin has run (the index is stored differently)");
    if (on && !h->pf_hw_ok) return fail("lmi_set_prefilter: fp16 subnormal self-test failed on this device; the prefilter's error bound does not hold");
    if (on != 0 && on != 1) return fail("lmi_set_prefilter: mode %d unknown (0: all-f32 scan, 1: fp16 prefilter + exact re-rank)", on);
    h->prefilter = on != 0;
    return 0;
}
