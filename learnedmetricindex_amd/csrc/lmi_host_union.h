// lmi_host_union.h -- the union scan: argument checks, the front of the three forms, the call's own device buffers and the schedule on
// the handle's stream.  The candidate stage (lmi_host_candidates.h) plans the call, builds and uploads the tables and scores every
// wave; what is the union scan's own is here: a sorted list per (query, rank), per wave the select behind the scores, per group one
// finish.  UnionFront is the front of every union and range call (lmi_host_range.h): the checks of the form -- bucket order given,
// ranked by the MLP, walked down the tree --, the device pointers, the MLP or the walk enqueued, the orders copied back afterwards.
// lmi_scan_union, lmi_scan_union_part, lmi_search_union, lmi_search_tree_union, lmi_union_set_geometry, lmi_debug_union_plan.
// The filtered forms (lmi_scan_union_filtered, lmi_search_union_filtered, lmi_search_tree_union_filtered; lmi_host_filter.h) are the
// same schedule with two differences: a slot whose (filter, bucket) pair allows no row is left out, and the select is the masked one.
#pragma once
#include "lmi_host_candidates.h"
#include "lmi_host_model.h"
#include "lmi_union_merge.h"

static_assert(LMI_UNION_MAX_K == lmi_union_plan::MAX_K, "lmi_union_plan.h restates LMI_UNION_MAX_K");
static_assert(LMI_UNION_PART_PLANES == UNION_PART_PLANES && LMI_UPART_SCORE == UPART_SCORE && LMI_UPART_DIST == UPART_DIST &&
                  LMI_UPART_ID == UPART_ID && LMI_UPART_RANK == UPART_RANK && LMI_UPART_ROW == UPART_ROW,
              "lmi_union_merge.h restates the planes of a part");

namespace {

thread_local int64_t g_union_last[LMI_UNION_PLAN_COUNT] = {};

// the stored form the union scan, the range search and the bucket cover read
int rowmajor_check(const lmi_index* h, const char* who) {
    if (stored_form(h) != FORM_ROWMAJOR)
        return fail("%s: the index is not stored row-major (%s): the union scan reads its candidates from the row-major f32 image only", who,
                    h->storage == LMI_STORAGE_F16 ? "LMI_STORAGE_F16" : "lmi_set_prefilter(0)");
    return 0;
}

// what every form refuses before any launch
int union_check(lmi_index* h, const char* who, int nq, int nb, int k) {
    if (!h->built) return fail("%s: the bucket index is not built (lmi_buckets_begin/add_rows/end)", who);
    if (k < 1 || k > LMI_UNION_MAX_K) return fail("%s: k %d outside [1,%d]", who, k, LMI_UNION_MAX_K);
    if (nq < 0 || nb < 1) return fail("%s: bad nq/n_buckets", who);
    if (nb > 1024) return fail("%s: n_buckets %d exceeds 1024", who, nb);
    if ((long long)nq * nb >= (1ll << 31)) return fail("%s: nq*n_buckets too large", who);
    CHK(rowmajor_check(h, who));
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
// f != nullptr (the filtered forms; filter_check has passed): the stage leaves the slots out that the filters empty and the select is
// the masked one.  Without f nothing differs from the unfiltered call.
int union_core(lmi_index* h, const char* who, const float* d_qs, int nq, const int* d_order, int nb, int k, const UnionOut& out, int on_device,
               const lmi_filter* f = nullptr, const int32_t* filter_of = nullptr) {
    namespace up = lmi_union_plan;
    hipStream_t st = h->stream;
    CandidateStage S(h, who);
    CHK(S.open(d_qs, nq, d_order, nb, k, on_device != 0, f, filter_of));
    const int LR = S.p.list_rows;
    const int64_t Q = S.p.query_rows;
    float* d_D = nullptr;
    knn_entry* d_lists = nullptr;
    int *d_slot_n = nullptr, *d_C = nullptr;
    long long* d_slot_pos0 = nullptr;
    unsigned *d_slot_base = nullptr, *d_I = nullptr;
    int* d_P = nullptr;   // a group's staged part: [LMI_UNION_PART_PLANES][Q * k]
    CHK(S.mem.alloc(&d_lists, (size_t)Q * nb * LR * sizeof(knn_entry), "lists"));
    CHK(S.mem.alloc(&d_slot_n, (size_t)Q * nb * 4, "slot rows"));
    CHK(S.mem.alloc(&d_slot_base, (size_t)Q * nb * 4, "slot bases"));
    CHK(S.mem.alloc(&d_slot_pos0, (size_t)Q * nb * 8, "slot positions"));
    if (!on_device) {
        if (out.as_part) CHK(S.mem.alloc(&d_P, (size_t)LMI_UNION_PART_PLANES * Q * k * 4, "part"));
        else {
            CHK(S.mem.alloc(&d_D, (size_t)Q * k * 4, "dists"));
            CHK(S.mem.alloc(&d_I, (size_t)Q * k * 4, "ids"));
        }
        CHK(S.mem.alloc(&d_C, (size_t)Q * 4, "counts"));
    }
    const up::Tables& last = S.groups.back();
    g_union_last[LMI_UNION_PLAN_GROUPS] = S.p.query_groups;
    g_union_last[LMI_UNION_PLAN_QUERY_ROWS] = S.p.query_rows;
    g_union_last[LMI_UNION_PLAN_WAVES] = (int64_t)last.waves.size();
    g_union_last[LMI_UNION_PLAN_SLAB_BYTES] = S.ext.slab_bytes;
    g_union_last[LMI_UNION_PLAN_LIST_ROWS] = LR;
    g_union_last[LMI_UNION_PLAN_LISTS_PER_QUERY] = S.p.lists_per_query;
    g_union_last[LMI_UNION_PLAN_WORKSPACE_BYTES] = S.mem.total;
    g_union_last[LMI_UNION_PLAN_VEC_ROWS] = S.vec;
    if (f) {
        g_filter_last[LMI_FILTER_PLAN_FILTERS] = f->nf;
        g_filter_last[LMI_FILTER_PLAN_MASK_BYTES] = f->mask_bytes();
        g_filter_last[LMI_FILTER_PLAN_SLOTS] = (int64_t)last.slots.size();
        g_filter_last[LMI_FILTER_PLAN_SKIPPED] = S.ext.skipped;
    }

    const size_t lds = (size_t)2 * LR * sizeof(knn_entry);
    auto down_async = [&](void* dst, const void* src, size_t bytes) -> int {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        return 0;
    };
    // A group's finish.  Device pointers: the kernel writes the group's rows of the caller's arrays.  Host pointers: it writes the staged
    // arrays, which are copied back (a part's planes lie Q * k words apart in the stage, nq * k in the caller's block).
    auto finish = [&](const up::Tables& G) -> int {
        const int64_t gq = G.q1 - G.q0;
        const size_t at = (size_t)G.q0 * k, bytes = (size_t)gq * k * 4;
        const float* qn2 = S.C.qn2 ? S.C.qn2 + G.q0 : nullptr;
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
    for (const up::Tables& G : S.groups) {
        CHK(S.upload(G));
        CHK(S.up(d_slot_n, G.slot_n.data(), G.slot_n.size() * 4));
        CHK(S.up(d_slot_base, G.slot_base.data(), G.slot_base.size() * 4));
        CHK(S.up(d_slot_pos0, G.slot_pos0.data(), G.slot_pos0.size() * 8));
        for (const up::Wave& W : G.waves) {
            if (W.slots == 0) continue;
            CHK(S.score(W));
            if (f) union_select_masked_kernel<<<(int)W.slots, 64, lds, st>>>(S.d_S, S.d_slots + W.slot0, S.d_slot_mask + W.slot0, f->mask.as<unsigned>(), k, LR, d_lists);
            else union_select_kernel<<<(int)W.slots, 64, lds, st>>>(S.d_S, S.d_slots + W.slot0, k, LR, d_lists);
            HIPCHK(hipGetLastError());
        }
        CHK(finish(G));
        HIPCHK(hipStreamSynchronize(st));   // the next group rewrites the tables and the lists
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

// The front of a union or range call, behind the consumer's own refusals (union_begin, range_begin).  The three forms and what a and b
// are in each: ORDER_GIVEN (lmi_scan_*): a = bucket_order [nq][nb], read only; ORDER_MLP (lmi_search_*): a = bucket_order, a nullable
// output; ORDER_TREE (lmi_search_tree_*): a = slab_ids, b = entries, nullable outputs.
// open: the form's refusals, then -- unless nq == 0, which the caller answers when open has returned 0 -- d_qs and d_order on the
// device, with the MLP or the walk that fills d_order enqueued on h->stream.  close: behind the core, the orders back to host pointers.
enum UnionForm { ORDER_GIVEN, ORDER_MLP, ORDER_TREE };
struct UnionFront {
    UnionForm form;
    int32_t *a, *b;
    const float* d_qs = nullptr;
    int *d_order = nullptr, *d_ent = nullptr;
    size_t bytes = 0;   // of one [nq][nb] order

    // outs_ok: no required output of the consumer is NULL; outs: how the refusal names them behind the two inputs (nullptr: there are none)
    int open(lmi_index* h, const char* who, const float* queries_nav, const float* queries_search, int nq, int nb, int on_device, bool outs_ok,
             const char* outs) {
        if (form == ORDER_MLP) {
            if (h->root().n_layers == 0) return fail("%s: no MLP set (lmi_set_mlp)", who);
            if (h->root().dims.back() != h->L) return fail("%s: MLP has %d classes, index has %d buckets", who, h->root().dims.back(), h->L);
        }
        if (nq == 0) return 0;
        const bool given = form == ORDER_GIVEN;
        if (!queries_search || !(given ? static_cast<const void*>(a) : queries_nav) || !outs_ok)
            return fail("%s: %s%s%s%s must not be NULL", who, given ? "queries_search" : "queries_nav", outs ? ", " : " and ",
                        given ? "bucket_order" : "queries_search", outs ? outs : "");
        if (form == ORDER_TREE) CHK(nav_check(h, nq, nb, who));
        else CHK(set_dev(h));
        bytes = (size_t)nq * nb * 4;
        const float* d_qn = nullptr;
        if (given) {
            const void *qs = nullptr, *order = nullptr;
            CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &qs));
            CHK(input_ptr(h, a, bytes, on_device, h->order, &order));
            d_qs = static_cast<const float*>(qs);
            d_order = static_cast<int*>(const_cast<void*>(order));   // (a given order is only read)
        } else CHK(union_queries(h, queries_nav, queries_search, nq, on_device, &d_qn, &d_qs));
        if (form == ORDER_MLP) {
            d_order = a;
            if (!on_device || !a) { CHK(h->order.reserve(bytes)); d_order = h->order.as<int>(); }
        } else if (form == ORDER_TREE) {
            CHK(h->nav_slab.reserve(bytes));
            CHK(h->nav_ent.reserve(bytes));
            d_order = (on_device && a) ? a : h->nav_slab.as<int>();
            d_ent = (on_device && b) ? b : h->nav_ent.as<int>();
        }
        begin_call(h);
        if (form == ORDER_MLP) CHK(mlp_enqueue(h, d_qn, nq, nb, d_order, nullptr));
        else if (form == ORDER_TREE) CHK(nav_enqueue(h, d_qn, nq, nb, d_order, d_ent));
        return 0;
    }
    int close(lmi_index* h, int on_device) {
        if (on_device || form == ORDER_GIVEN) return 0;
        return copy_back(h, {{a, d_order, bytes}, {b, d_ent, bytes}});
    }
};

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

// every union entry point: a, b as UnionFront states them
static int union_call(UnionForm form, const char* who, lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                      const UnionOut& out, int32_t* a, int32_t* b, int on_device, const UnionFilter& uf) {
    CHK(union_begin(h, who, nq, nb, k, uf));
    UnionFront F{form, a, b};
    CHK(F.open(h, who, queries_nav, queries_search, nq, nb, on_device, out.as_part ? out.part != nullptr : out.dists && out.ids,
               out.as_part ? " and part" : ", dists and ids"));
    if (nq == 0) return 0;
    CHK(union_core(h, who, F.d_qs, nq, F.d_order, nb, k, out, on_device, uf.f, uf.filter_of));
    return F.close(h, on_device);
}
extern "C" LMI_API int lmi_scan_union(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                      float* dists, uint32_t* ids, int32_t* counts, int on_device) {
    return union_call(ORDER_GIVEN, "lmi_scan_union", h, nullptr, queries_search, nq, nb, k, UnionOut{dists, ids, nullptr, counts},
                      const_cast<int32_t*>(bucket_order), nullptr, on_device, UnionFilter{});
}
extern "C" LMI_API int lmi_scan_union_filtered(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                               float* dists, uint32_t* ids, int32_t* counts, int on_device, const lmi_filter* f,
                                               const int32_t* filter_of) {
    return union_call(ORDER_GIVEN, "lmi_scan_union_filtered", h, nullptr, queries_search, nq, nb, k, UnionOut{dists, ids, nullptr, counts},
                      const_cast<int32_t*>(bucket_order), nullptr, on_device, UnionFilter{true, f, filter_of});
}
extern "C" LMI_API int lmi_scan_union_part(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                           int32_t* part, int32_t* counts, int on_device) {
    return union_call(ORDER_GIVEN, "lmi_scan_union_part", h, nullptr, queries_search, nq, nb, k, UnionOut{nullptr, nullptr, part, counts, true},
                      const_cast<int32_t*>(bucket_order), nullptr, on_device, UnionFilter{});
}
extern "C" LMI_API int lmi_search_union(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                        float* dists, uint32_t* ids, int32_t* counts, int32_t* bucket_order, int on_device) {
    return union_call(ORDER_MLP, "lmi_search_union", h, queries_nav, queries_search, nq, nb, k, UnionOut{dists, ids, nullptr, counts}, bucket_order,
                      nullptr, on_device, UnionFilter{});
}
extern "C" LMI_API int lmi_search_union_filtered(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                                 float* dists, uint32_t* ids, int32_t* counts, int32_t* bucket_order, int on_device,
                                                 const lmi_filter* f, const int32_t* filter_of) {
    return union_call(ORDER_MLP, "lmi_search_union_filtered", h, queries_nav, queries_search, nq, nb, k, UnionOut{dists, ids, nullptr, counts},
                      bucket_order, nullptr, on_device, UnionFilter{true, f, filter_of});
}
extern "C" LMI_API int lmi_search_tree_union(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                             float* dists, uint32_t* ids, int32_t* counts, int32_t* slab_ids, int32_t* entries, int on_device) {
    return union_call(ORDER_TREE, "lmi_search_tree_union", h, queries_nav, queries_search, nq, nb, k, UnionOut{dists, ids, nullptr, counts}, slab_ids,
                      entries, on_device, UnionFilter{});
}
extern "C" LMI_API int lmi_search_tree_union_filtered(lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                                                      float* dists, uint32_t* ids, int32_t* counts, int32_t* slab_ids, int32_t* entries,
                                                      int on_device, const lmi_filter* f, const int32_t* filter_of) {
    return union_call(ORDER_TREE, "lmi_search_tree_union_filtered", h, queries_nav, queries_search, nq, nb, k, UnionOut{dists, ids, nullptr, counts},
                      slab_ids, entries, on_device, UnionFilter{true, f, filter_of});
}
