// lmi_host_union.h -- the union scan: argument checks, the call's device buffers and the schedule on the handle's stream.  The geometry
// and every table the kernels are launched from come from lmi_union_plan.h (pure host code, checked on the CPU): nothing here loops
// over slots, chunks or tiles.  The bucket order comes back to the host once (that is the call's internal synchronisation); per query
// group the tables are built and uploaded; per wave pack, score, select; per group one finish.
// lmi_scan_union, lmi_scan_union_part, lmi_search_union, lmi_search_tree_union, lmi_union_set_geometry, lmi_debug_union_plan.
// The filtered forms (lmi_scan_union_filtered, lmi_search_union_filtered, lmi_search_tree_union_filtered; lmi_host_filter.h) are the
// same schedule with two differences: a slot whose (filter, bucket) pair allows no row is left out, and the select is the masked one.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_host_filter.h"
#include "lmi_host_model.h"
#include "lmi_host_scan.h"
#include "lmi_union.h"
#include "lmi_union_merge.h"
#include "lmi_union_plan.h"

static_assert(LMI_UNION_MAX_K == lmi_union_plan::MAX_K, "lmi_union_plan.h restates LMI_UNION_MAX_K");
static_assert(KNN_ROWS == lmi_union_plan::ITEM_ROWS, "lmi_union_plan.h restates the rows of a bucket that one item scores");
static_assert(LMI_UNION_PART_PLANES == UNION_PART_PLANES && LMI_UPART_SCORE == UPART_SCORE && LMI_UPART_DIST == UPART_DIST &&
                  LMI_UPART_ID == UPART_ID && LMI_UPART_RANK == UPART_RANK && LMI_UPART_ROW == UPART_ROW,
              "lmi_union_merge.h restates the planes of a part");

namespace {

thread_local lmi_union_plan::Forced g_union_forced;
thread_local int64_t g_union_last[LMI_UNION_PLAN_COUNT] = {};

template <bool VEC>
int union_score_launch(int ct, int n_items, hipStream_t st, const UnionItem* items, const float* rows, int dp, int d, const float4* Qf, int KG,
                       const long long* tile_off, const int* tile_cnt, float* S) {
    if (ct == 1) union_score_kernel<1, VEC><<<n_items, 256, 0, st>>>(items, rows, dp, d, Qf, KG, tile_off, tile_cnt, S);
    else if (ct == 2) union_score_kernel<2, VEC><<<n_items, 256, 0, st>>>(items, rows, dp, d, Qf, KG, tile_off, tile_cnt, S);
    else union_score_kernel<4, VEC><<<n_items, 256, 0, st>>>(items, rows, dp, d, Qf, KG, tile_off, tile_cnt, S);
    HIPCHK(hipGetLastError());
    return 0;
}

// what every form refuses before any launch
int union_check(lmi_index* h, const char* who, int nq, int nb, int k) {
    if (!h->built) return fail("%s: the bucket index is not built (lmi_buckets_begin/add_rows/end)", who);
    if (k < 1 || k > LMI_UNION_MAX_K) return fail("%s: k %d outside [1,%d]", who, k, LMI_UNION_MAX_K);
    if (nq < 0 || nb < 1) return fail("%s: bad nq/n_buckets", who);
    if (nb > 1024) return fail("%s: n_buckets %d exceeds 1024", who, nb);
    if ((long long)nq * nb >= (1ll << 31)) return fail("%s: nq*n_buckets too large", who);
    if (stored_form(h) != FORM_ROWMAJOR)
        return fail("%s: the index is not stored row-major (%s): the union scan reads its candidates from the row-major f32 image only", who,
                    h->storage == LMI_STORAGE_F16 ? "LMI_STORAGE_F16" : "lmi_set_prefilter(0)");
    int64_t largest = 0;
    for (int n : h->h_nb_rows) largest = std::max<int64_t>(largest, n);
    if ((int64_t)nb * largest >= (1ll << 32) - 1)
        return fail("%s: n_buckets %d x the largest bucket (%lld rows) does not fit a 32-bit ordinal", who, nb, (long long)largest);
    return 0;
}

// where a call's results go: dists / ids [nq][k], or -- as_part (lmi_scan_union_part) -- the [LMI_UNION_PART_PLANES][nq][k] block
// `part`; counts [nq] is nullable in both
struct UnionOut {
    float* dists = nullptr;
    uint32_t* ids = nullptr;
    int32_t* part = nullptr;
    int32_t* counts = nullptr;
    bool as_part = false;
};

// d_qs [nq][d_user] and d_order [nq][nb] on the device, already enqueued on h->stream; out as the caller gave it.
// f != nullptr (the filtered forms; filter_check has passed): query q's candidates are the rows filter filter_of[q] allows (host [nq];
// nullptr: filter 0; -1: all rows); a slot whose (filter, bucket) pair allows no row is left out of the tables (lmi_union_plan.h states
// the rule) and the select is the masked one.  Without f nothing differs from the unfiltered call.
int union_core(lmi_index* h, const char* who, const float* d_qs, int nq, const int* d_order, int nb, int k, const UnionOut& out, int on_device,
               const lmi_filter* f = nullptr, const int32_t* filter_of = nullptr) {
    namespace up = lmi_union_plan;
    hipStream_t st = h->stream;
    const int L = h->L;
    // L2: the queries at the stored width, [q, 1, 0..], and |q|^2
    ScanCall C;
    C.P.nq = nq;
    CHK(scan_augment_l2(h, C, d_qs));
    // the bucket order and the live bucket tables, on the host
    std::vector<int> order((size_t)nq * nb), nrows(L), rbs(L + 1);
    HIPCHK(hipMemcpyAsync(order.data(), d_order, order.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(nrows.data(), h->d_nb_rows.p, (size_t)L * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rbs.data(), h->d_rb_start.p, (size_t)(L + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));

    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const up::Plan p = up::make_plan(nq, nb, k, h->d, on_device != 0, (int64_t)free_b, g_union_forced);
    const int LR = p.list_rows, KG = p.kg;
    const bool vec = h->d % 4 == 0;   // rows of the image start 16-byte aligned (dp % 4 == 0); d % 4 == 0 keeps every 16-byte load inside d

    // every group's tables, on the host, and the largest of each for the buffers
    const up::Layout layout{L, nrows.data(), rbs.data()};
    const up::FilterView fview{f ? f->counts.data() : nullptr, filter_of, f ? f->n_rb_total : 0};
    std::vector<up::Tables> groups;
    groups.reserve((size_t)p.query_groups);
    int64_t max_slab = 0, max_tiles = 0, max_group_tiles = 0, max_items = 0, max_slots = 0, skipped = 0;
    for (int64_t g = 0; g < p.query_groups; ++g) {
        groups.push_back(up::build_tables(p, g, order.data(), layout, f ? &fview : nullptr));
        const up::Tables& G = groups.back();
        for (const up::Wave& W : G.waves) {
            max_slab = std::max(max_slab, W.slab_floats * 4);
            max_tiles = std::max(max_tiles, W.tiles);
        }
        max_group_tiles = std::max<int64_t>(max_group_tiles, (int64_t)G.tile_cnt.size());
        max_items = std::max<int64_t>(max_items, (int64_t)G.items.size());
        max_slots = std::max<int64_t>(max_slots, (int64_t)G.slots.size());
        skipped += G.skipped;
    }
    const int64_t Q = p.query_rows;
    CallScratch mem(who);
    float *d_S = nullptr, *d_D = nullptr;
    float4* d_qf = nullptr;
    knn_entry* d_lists = nullptr;
    UnionItem* d_items = nullptr;
    UnionSlot* d_slots = nullptr;
    int *d_rowq = nullptr, *d_tile_cnt = nullptr, *d_slot_n = nullptr, *d_C = nullptr;
    long long *d_tile_off = nullptr, *d_slot_pos0 = nullptr, *d_slot_mask = nullptr;
    unsigned *d_slot_base = nullptr, *d_I = nullptr;
    int* d_P = nullptr;   // a group's staged part: [LMI_UNION_PART_PLANES][Q * k]
    CHK(mem.alloc(&d_S, (size_t)max_slab, "score slab"));
    CHK(mem.alloc(&d_lists, (size_t)Q * nb * LR * sizeof(knn_entry), "lists"));
    CHK(mem.alloc(&d_qf, (size_t)max_tiles * KG * 1024, "query fragments"));
    CHK(mem.alloc(&d_items, (size_t)max_items * sizeof(UnionItem), "items"));
    CHK(mem.alloc(&d_slots, (size_t)max_slots * sizeof(UnionSlot), "slots"));
    CHK(mem.alloc(&d_rowq, (size_t)max_group_tiles * 32 * 4, "fragment rows"));
    CHK(mem.alloc(&d_tile_cnt, (size_t)max_group_tiles * 4, "tile counts"));
    CHK(mem.alloc(&d_tile_off, (size_t)max_group_tiles * 8, "tile offsets"));
    CHK(mem.alloc(&d_slot_n, (size_t)Q * nb * 4, "slot rows"));
    CHK(mem.alloc(&d_slot_base, (size_t)Q * nb * 4, "slot bases"));
    CHK(mem.alloc(&d_slot_pos0, (size_t)Q * nb * 8, "slot positions"));
    if (f) CHK(mem.alloc(&d_slot_mask, (size_t)max_slots * 8, "slot masks"));
    if (!on_device) {
        if (out.as_part) CHK(mem.alloc(&d_P, (size_t)LMI_UNION_PART_PLANES * Q * k * 4, "part"));
        else {
            CHK(mem.alloc(&d_D, (size_t)Q * k * 4, "dists"));
            CHK(mem.alloc(&d_I, (size_t)Q * k * 4, "ids"));
        }
        CHK(mem.alloc(&d_C, (size_t)Q * 4, "counts"));
    }
    g_union_last[LMI_UNION_PLAN_GROUPS] = p.query_groups;
    g_union_last[LMI_UNION_PLAN_QUERY_ROWS] = p.query_rows;
    g_union_last[LMI_UNION_PLAN_WAVES] = (int64_t)groups.back().waves.size();
    g_union_last[LMI_UNION_PLAN_SLAB_BYTES] = max_slab;
    g_union_last[LMI_UNION_PLAN_LIST_ROWS] = LR;
    g_union_last[LMI_UNION_PLAN_LISTS_PER_QUERY] = p.lists_per_query;
    g_union_last[LMI_UNION_PLAN_WORKSPACE_BYTES] = mem.total;
    g_union_last[LMI_UNION_PLAN_VEC_ROWS] = vec;
    if (f) {
        g_filter_last[LMI_FILTER_PLAN_FILTERS] = f->nf;
        g_filter_last[LMI_FILTER_PLAN_MASK_BYTES] = f->mask_bytes();
        g_filter_last[LMI_FILTER_PLAN_SLOTS] = (int64_t)groups.back().slots.size();
        g_filter_last[LMI_FILTER_PLAN_SKIPPED] = skipped;
    }

    const size_t lds = (size_t)2 * LR * sizeof(knn_entry);
    auto up_async = [&](void* dst, const void* src, size_t bytes) -> int {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        return 0;
    };
    auto down_async = [&](void* dst, const void* src, size_t bytes) -> int {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        return 0;
    };
    // A group's finish.  Device pointers: the kernel writes the group's rows of the caller's arrays.  Host pointers: it writes the staged
    // arrays, which are copied back (a part's planes lie Q * k words apart in the stage, nq * k in the caller's block).
    auto finish = [&](const up::Tables& G) -> int {
        const int64_t gq = G.q1 - G.q0;
        const size_t at = (size_t)G.q0 * k, bytes = (size_t)gq * k * 4;
        const float* qn2 = C.qn2 ? C.qn2 + G.q0 : nullptr;
        int* oC = on_device ? (out.counts ? out.counts + G.q0 : nullptr) : d_C;
        if (out.as_part) {
            const long long plane = on_device ? (long long)nq * k : (long long)Q * k;
            union_finish_part_kernel<<<(int)gq, 64, lds, st>>>(d_lists, d_slot_n, d_slot_base, d_slot_pos0, nb, LR, k, qn2, h->ids_slab.as<unsigned>(),
                                                              on_device ? out.part + at : d_P, plane, oC);
            HIPCHK(hipGetLastError());
            if (!on_device)
                for (int pl = 0; pl < LMI_UNION_PART_PLANES; ++pl) CHK(down_async(out.part + (size_t)pl * nq * k + at, d_P + (size_t)pl * plane, bytes));
        } else {
            union_finish_kernel<<<(int)gq, 64, lds, st>>>(d_lists, d_slot_n, d_slot_base, d_slot_pos0, nb, LR, k, qn2, h->ids_slab.as<unsigned>(),
                                                         on_device ? out.dists + at : d_D, on_device ? out.ids + at : d_I, oC);
            HIPCHK(hipGetLastError());
            if (!on_device) {
                CHK(down_async(out.dists + at, d_D, bytes));
                CHK(down_async(out.ids + at, d_I, bytes));
            }
        }
        if (!on_device && out.counts) CHK(down_async(out.counts + G.q0, d_C, (size_t)gq * 4));
        return 0;
    };
    for (const up::Tables& G : groups) {
        CHK(up_async(d_items, G.items.data(), G.items.size() * sizeof(UnionItem)));
        CHK(up_async(d_slots, G.slots.data(), G.slots.size() * sizeof(UnionSlot)));
        CHK(up_async(d_rowq, G.rowq.data(), G.rowq.size() * 4));
        CHK(up_async(d_tile_cnt, G.tile_cnt.data(), G.tile_cnt.size() * 4));
        CHK(up_async(d_tile_off, G.tile_off.data(), G.tile_off.size() * 8));
        CHK(up_async(d_slot_n, G.slot_n.data(), G.slot_n.size() * 4));
        CHK(up_async(d_slot_base, G.slot_base.data(), G.slot_base.size() * 4));
        CHK(up_async(d_slot_pos0, G.slot_pos0.data(), G.slot_pos0.size() * 8));
        if (f) CHK(up_async(d_slot_mask, G.slot_mask.data(), G.slot_mask.size() * 8));
        for (const up::Wave& W : G.waves) {
            if (W.slots == 0) continue;
            union_pack_kernel<<<cdiv(W.tiles * 32 * KG, 256), 256, 0, st>>>(C.q, d_rowq + W.tile0 * 32, h->d, (int)W.tiles, KG, d_qf);
            HIPCHK(hipGetLastError());
            if (vec) CHK(union_score_launch<true>(W.ct, (int)W.items, st, d_items + W.item0, h->rowmajor.as<float>(), h->dp, h->d, d_qf, KG,
                                                  d_tile_off + W.tile0, d_tile_cnt + W.tile0, d_S));
            else CHK(union_score_launch<false>(W.ct, (int)W.items, st, d_items + W.item0, h->rowmajor.as<float>(), h->dp, h->d, d_qf, KG,
                                               d_tile_off + W.tile0, d_tile_cnt + W.tile0, d_S));
            if (f) union_select_masked_kernel<<<(int)W.slots, 64, lds, st>>>(d_S, d_slots + W.slot0, d_slot_mask + W.slot0, f->mask.as<unsigned>(), k, LR, d_lists);
            else union_select_kernel<<<(int)W.slots, 64, lds, st>>>(d_S, d_slots + W.slot0, k, LR, d_lists);
            HIPCHK(hipGetLastError());
        }
        CHK(finish(G));
        // the next group rewrites the tables and the lists; the host tables above live until the call returns
        HIPCHK(hipStreamSynchronize(st));
    }
    return 0;
}

// the filter of a call: none (the unfiltered entry points) or the (f, filter_of) pair of a *_filtered one, which must then be valid
struct UnionFilter {
    bool asked = false;
    const lmi_filter* f = nullptr;
    const int32_t* filter_of = nullptr;
};
// how every form begins: the plan words cleared, then the refusals that need no pointer
int union_begin(lmi_index* h, const char* who, int nq, int nb, int k, const UnionFilter& uf) {
    for (int64_t& w : g_union_last) w = 0;
    for (int64_t& w : g_filter_last) w = 0;
    if (!h) return fail("%s: NULL handle", who);
    CHK(union_check(h, who, nq, nb, k));
    if (uf.asked) CHK(filter_check(h, who, uf.f, uf.filter_of, nq));
    return 0;
}

// queries_nav [nq][dims[0]] and queries_search [nq][d_user] of the two search forms, on the device: one array where the caller passed
// one and the widths agree
int union_queries(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int on_device, const float** d_qn,
                  const float** d_qs) {
    const void *qn = nullptr, *qs = nullptr;
    CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &qn));
    if (queries_search == queries_nav && h->root().dims[0] == h->d_user) qs = qn;
    else CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &qs));
    *d_qn = static_cast<const float*>(qn);
    *d_qs = static_cast<const float*>(qs);
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_union_set_geometry(int64_t query_rows, int64_t slab_bytes) {
    if (query_rows < 0 || query_rows > (1ll << 20)) return fail("lmi_union_set_geometry: query_rows %lld outside [0, 2^20]", (long long)query_rows);
    if (slab_bytes < 0) return fail("lmi_union_set_geometry: slab_bytes %lld is negative", (long long)slab_bytes);
    g_union_forced.query_rows = query_rows;
    g_union_forced.slab_bytes = slab_bytes;
    return 0;
}

extern "C" LMI_API int lmi_debug_union_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_union_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_UNION_PLAN_COUNT); ++i) out[i] = g_union_last[i];
    return 0;
}

static int scan_union_impl(const char* who, lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                           const UnionOut& out, int on_device, const UnionFilter& uf) {
    CHK(union_begin(h, who, nq, nb, k, uf));
    if (nq == 0) return 0;
    if (out.as_part) {
        if (!queries_search || !bucket_order || !out.part) return fail("%s: queries_search, bucket_order and part must not be NULL", who);
    } else if (!queries_search || !bucket_order || !out.dists || !out.ids)
        return fail("%s: queries_search, bucket_order, dists and ids must not be NULL", who);
    CHK(set_dev(h));
    const void* d_qs = nullptr;
    const void* d_order = nullptr;
    CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &d_qs));
    CHK(input_ptr(h, bucket_order, (size_t)nq * nb * 4, on_device, h->order, &d_order));
    begin_call(h);
    return union_core(h, who, static_cast<const float*>(d_qs), nq, static_cast<const int*>(d_order), nb, k, out, on_device, uf.f, uf.filter_of);
}
extern "C" LMI_API int lmi_scan_union(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                      float* dists, uint32_t* ids, int32_t* counts, int on_device) {
    return scan_union_impl("lmi_scan_union", h, queries_search, nq, bucket_order, nb, k, UnionOut{dists, ids, nullptr, counts}, on_device,
                           UnionFilter{});
}
extern "C" LMI_API int lmi_scan_union_filtered(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                               float* dists, uint32_t* ids, int32_t* counts, int on_device, const lmi_filter* f,
                                               const int32_t* filter_of) {
    return scan_union_impl("lmi_scan_union_filtered", h, queries_search, nq, bucket_order, nb, k, UnionOut{dists, ids, nullptr, counts}, on_device,
                           UnionFilter{true, f, filter_of});
}
extern "C" LMI_API int lmi_scan_union_part(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                           int32_t* part, int32_t* counts, int on_device) {
    return scan_union_impl("lmi_scan_union_part", h, queries_search, nq, bucket_order, nb, k, UnionOut{nullptr, nullptr, part, counts, true},
                           on_device, UnionFilter{});
}

static int search_union_impl(const char* who, lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                             float* dists, uint32_t* ids, int32_t* counts, int32_t* bucket_order, int on_device, const UnionFilter& uf) {
    CHK(union_begin(h, who, nq, nb, k, uf));
    if (h->root().n_layers == 0) return fail("%s: no MLP set (lmi_set_mlp)", who);
    if (h->root().dims.back() != h->L) return fail("%s: MLP has %d classes, index has %d buckets", who, h->root().dims.back(), h->L);
    if (nq == 0) return 0;
    if (!queries_nav || !queries_search || !dists || !ids) return fail("%s: queries_nav, queries_search, dists and ids must not be NULL", who);
    CHK(set_dev(h));
    const float *d_qn = nullptr, *d_qs = nullptr;
    CHK(union_queries(h, queries_nav, queries_search, nq, on_device, &d_qn, &d_qs));
    int* d_order = bucket_order;
    if (!on_device || !bucket_order) { CHK(h->order.reserve((size_t)nq * nb * 4)); d_order = h->order.as<int>(); }
    begin_call(h);
    CHK(mlp_enqueue(h, d_qn, nq, nb, d_order, nullptr));
    CHK(union_core(h, who, d_qs, nq, d_order, nb, k, UnionOut{dists, ids, nullptr, counts}, on_device, uf.f, uf.filter_of));
    if (!on_device) CHK(copy_back(h, {{bucket_order, d_order, (size_t)nq * nb * 4}}));
    return 0;
}
extern "C" LMI_API int lmi_search_union(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                        float* dists, uint32_t* ids, int32_t* counts, int32_t* bucket_order, int on_device) {
    return search_union_impl("lmi_search_union", h, queries_nav, queries_search, nq, nb, k, dists, ids, counts, bucket_order, on_device, UnionFilter{});
}
extern "C" LMI_API int lmi_search_union_filtered(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                                 float* dists, uint32_t* ids, int32_t* counts, int32_t* bucket_order, int on_device,
                                                 const lmi_filter* f, const int32_t* filter_of) {
    return search_union_impl("lmi_search_union_filtered", h, queries_nav, queries_search, nq, nb, k, dists, ids, counts, bucket_order, on_device,
                             UnionFilter{true, f, filter_of});
}

static int search_tree_union_impl(const char* who, lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                  float* dists, uint32_t* ids, int32_t* counts, int32_t* slab_ids, int32_t* entries, int on_device,
                                  const UnionFilter& uf) {
    CHK(union_begin(h, who, nq, nb, k, uf));
    if (nq == 0) return 0;
    if (!queries_nav || !queries_search || !dists || !ids) return fail("%s: queries_nav, queries_search, dists and ids must not be NULL", who);
    CHK(nav_check(h, nq, nb, who));
    const float *d_qn = nullptr, *d_qs = nullptr;
    CHK(union_queries(h, queries_nav, queries_search, nq, on_device, &d_qn, &d_qs));
    CHK(h->nav_slab.reserve((size_t)nq * nb * 4));
    CHK(h->nav_ent.reserve((size_t)nq * nb * 4));
    int* d_slab = (on_device && slab_ids) ? slab_ids : h->nav_slab.as<int>();
    int* d_ent = (on_device && entries) ? entries : h->nav_ent.as<int>();
    begin_call(h);
    CHK(nav_enqueue(h, d_qn, nq, nb, d_slab, d_ent));
    CHK(union_core(h, who, d_qs, nq, d_slab, nb, k, UnionOut{dists, ids, nullptr, counts}, on_device, uf.f, uf.filter_of));
    if (!on_device) CHK(copy_back(h, {{slab_ids, d_slab, (size_t)nq * nb * 4}, {entries, d_ent, (size_t)nq * nb * 4}}));
    return 0;
}
extern "C" LMI_API int lmi_search_tree_union(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                             float* dists, uint32_t* ids, int32_t* counts, int32_t* slab_ids, int32_t* entries, int on_device) {
    return search_tree_union_impl("lmi_search_tree_union", h, queries_nav, queries_search, nq, nb, k, dists, ids, counts, slab_ids, entries, on_device,
                                  UnionFilter{});
}
extern "C" LMI_API int lmi_search_tree_union_filtered(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                                      float* dists, uint32_t* ids, int32_t* counts, int32_t* slab_ids, int32_t* entries,
                                                      int on_device, const lmi_filter* f, const int32_t* filter_of) {
    return search_tree_union_impl("lmi_search_tree_union_filtered", h, queries_nav, queries_search, nq, nb, k, dists, ids, counts, slab_ids, entries,
                                  on_device, UnionFilter{true, f, filter_of});
}
