// lmi_host_union.h -- the union scan: argument checks, the geometry (lmi_union_plan.h), the call's device buffers and the schedule on
// the handle's stream.  The bucket order comes back to the host once (that is the call's internal synchronisation): per query group the
// host sorts the slots by bucket, cuts them into waves and writes the item tables; per wave pack, score, select; per group one finish.
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

// d_qs [nq][d_user] and d_order [nq][nb] on the device, already enqueued on h->stream; dists / ids / counts as the caller gave them.
// part != nullptr (lmi_scan_union_part): the caller's [LMI_UNION_PART_PLANES][nq][k] block is written instead of dists / ids.
// f != nullptr (the filtered forms; filter_check has passed): query q's candidates are the rows filter filter_of[q] allows (host [nq];
// nullptr: filter 0; -1: all rows).  A slot whose (filter, bucket) pair allows no row gets slot_n = 0 and no slot -- it is not packed,
// scored or selected -- while slot_base still advances by the bucket's rows: ordinals stay the unfiltered concatenation's, the finish
// kernel skips the rank, and no entry carries an ordinal of the gap.  Without f nothing differs from the unfiltered call.
int union_core(lmi_index* h, const char* who, const float* d_qs, int nq, const int* d_order, int nb, int k, float* dists, uint32_t* ids,
               int32_t* counts, int on_device, int32_t* part = nullptr, const lmi_filter* f = nullptr, const int32_t* filter_of = nullptr) {
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

    // per group: the slots sorted by bucket, the waves and every table, on the host
    struct Wave { int64_t item0, items, slot0, slots, tile0, tiles, slab_floats; int ct; };
    struct Group {
        int64_t q0, q1;
        std::vector<Wave> waves;
        std::vector<UnionItem> items;
        std::vector<UnionSlot> slots;
        std::vector<int> rowq, tile_cnt, slot_n;
        std::vector<long long> tile_off, slot_pos0;
        std::vector<unsigned> slot_base;
        std::vector<long long> slot_mask;   // filtered: beside `slots`, the word offset of each slot's mask row (-1: unfiltered query)
    };
    std::vector<Group> groups((size_t)p.query_groups);
    int64_t max_slab = 0, max_tiles = 0, max_items = 0, max_slots = 0, skipped = 0;
    auto filter_of_query = [&](int64_t q) -> int { return f ? (filter_of ? filter_of[q] : 0) : -1; };
    std::vector<int64_t> rows64(nrows.begin(), nrows.end());
    for (int64_t g = 0; g < p.query_groups; ++g) {
        Group& G = groups[g];
        up::group_range(p, g, &G.q0, &G.q1);
        const int64_t gq = G.q1 - G.q0;
        G.slot_n.assign((size_t)gq * nb, 0);
        G.slot_base.assign((size_t)gq * nb, 0u);
        G.slot_pos0.assign((size_t)gq * nb, 0);
        std::vector<int64_t> cnt(L, 0);
        for (int64_t q = 0; q < gq; ++q) {
            int64_t base = 0;
            const int fj = filter_of_query(G.q0 + q);
            for (int t = 0; t < nb; ++t) {
                const int b = order[(size_t)(G.q0 + q) * nb + t];
                const int n = b >= 0 && b < L ? nrows[b] : 0;
                const bool dead = fj >= 0 && n > 0 && f->counts[(size_t)fj * L + b] == 0;   // the filter allows no row of the bucket
                G.slot_base[q * nb + t] = (unsigned)base;
                G.slot_n[q * nb + t] = dead ? 0 : n;
                if (n > 0) base += n;
                if (dead) ++skipped;
                else if (n > 0) { G.slot_pos0[q * nb + t] = (long long)rbs[b] * 32; cnt[b]++; }
            }
        }
        // a bucket's slots in (query, rank) order
        std::vector<int64_t> start(L + 1, 0);
        for (int b = 0; b < L; ++b) start[b + 1] = start[b] + cnt[b];
        std::vector<int64_t> by_bucket((size_t)start[L]), fill(start.begin(), start.end() - 1);
        for (int64_t s = 0; s < gq * nb; ++s)
            if (G.slot_n[s] > 0) by_bucket[fill[order[(size_t)G.q0 * nb + s]]++] = s;
        int n_waves = 0;
        const std::vector<up::Chunk> chunks = up::cut_waves(p, rows64, cnt, &n_waves);
        G.waves.assign((size_t)n_waves, Wave{0, 0, 0, 0, 0, 0, 0, 1});
        for (const up::Chunk& c : chunks) {
            Wave& W = G.waves[c.wave];
            const int64_t tiles = up::cdiv(c.slots, 32), pitch = up::slab_pitch(c.n);
            // the tables of a group are laid out wave after wave: a wave's start in the slot and tile tables (a chunk's tile0 and slab_off
            // count from its wave's)
            if (W.slots == 0) { W.slot0 = (int64_t)G.slots.size(); W.tile0 = (int64_t)G.tile_cnt.size(); }
            W.tiles += tiles;
            W.slots += c.slots;
            W.slab_floats = std::max(W.slab_floats, c.slab_off + c.slots * pitch);
            W.ct = std::max(W.ct, tiles >= 3 ? 4 : (int)tiles);
            for (int64_t i = 0; i < tiles * 32; ++i) {
                const bool real = i < c.slots;
                const int64_t s = real ? by_bucket[start[c.bucket] + c.slot0 + i] : -1;
                G.rowq.push_back(real ? (int)(G.q0 + s / nb) : -1);
                if (real) G.slots.push_back(UnionSlot{c.slab_off + i * pitch, s * LR, (int)c.n, G.slot_base[s]});
                if (real && f) {
                    const int fj = filter_of_query(G.q0 + s / nb);
                    G.slot_mask.push_back(fj < 0 ? -1ll : (long long)lmi_filter_plan::mask_word(fj, f->n_rb_total, rbs[c.bucket], 0));
                }
            }
            for (int64_t t = 0; t < tiles; ++t) {
                G.tile_off.push_back(c.slab_off + t * 32 * pitch);
                G.tile_cnt.push_back((int)std::min<int64_t>(32, c.slots - t * 32));
            }
        }
        // the items need the wave's tile group width, which is known only now
        for (int w = 0; w < n_waves; ++w) {
            Wave& W = G.waves[w];
            W.item0 = (int64_t)G.items.size();
            for (const up::Chunk& c : chunks) {
                if (c.wave != w) continue;
                const int64_t tiles = up::cdiv(c.slots, 32), blocks = up::cdiv(c.n, KNN_ROWS);
                for (int64_t t0 = 0; t0 < tiles; t0 += W.ct)
                    for (int64_t blk = 0; blk < blocks; ++blk)
                        G.items.push_back(UnionItem{(long long)rbs[c.bucket] * 32, (int)c.n, (int)blk, (int)(c.tile0 + t0),
                                                    (int)std::min<int64_t>(W.ct, tiles - t0)});
            }
            W.items = (int64_t)G.items.size() - W.item0;
            max_slab = std::max(max_slab, W.slab_floats * 4);
            max_tiles = std::max(max_tiles, W.tiles);
        }
        max_items = std::max<int64_t>(max_items, (int64_t)G.items.size());
        max_slots = std::max<int64_t>(max_slots, (int64_t)G.slots.size());
    }
    const int64_t Q = p.query_rows;
    CallScratch mem(who);
    float *d_S = nullptr, *d_D = nullptr;
    float4* d_qf = nullptr;
    knn_entry* d_lists = nullptr;
    UnionItem* d_items = nullptr;
    UnionSlot* d_slots = nullptr;
    int *d_rowq = nullptr, *d_tile_cnt = nullptr, *d_slot_n = nullptr, *d_C = nullptr;
    long long *d_tile_off = nullptr, *d_slot_pos0 = nullptr;
    unsigned *d_slot_base = nullptr, *d_I = nullptr;
    int* d_P = nullptr;   // a group's staged part: [LMI_UNION_PART_PLANES][Q * k]
    int64_t max_group_tiles = 0;
    for (const Group& G : groups) max_group_tiles = std::max<int64_t>(max_group_tiles, (int64_t)G.tile_cnt.size());
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
    long long* d_slot_mask = nullptr;
    if (f) CHK(mem.alloc(&d_slot_mask, (size_t)max_slots * 8, "slot masks"));
    if (!on_device) {
        if (part) CHK(mem.alloc(&d_P, (size_t)LMI_UNION_PART_PLANES * Q * k * 4, "part"));
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
    for (const Group& G : groups) {
        const int64_t gq = G.q1 - G.q0;
        CHK(up_async(d_items, G.items.data(), G.items.size() * sizeof(UnionItem)));
        CHK(up_async(d_slots, G.slots.data(), G.slots.size() * sizeof(UnionSlot)));
        CHK(up_async(d_rowq, G.rowq.data(), G.rowq.size() * 4));
        CHK(up_async(d_tile_cnt, G.tile_cnt.data(), G.tile_cnt.size() * 4));
        CHK(up_async(d_tile_off, G.tile_off.data(), G.tile_off.size() * 8));
        CHK(up_async(d_slot_n, G.slot_n.data(), G.slot_n.size() * 4));
        CHK(up_async(d_slot_base, G.slot_base.data(), G.slot_base.size() * 4));
        CHK(up_async(d_slot_pos0, G.slot_pos0.data(), G.slot_pos0.size() * 8));
        if (f) CHK(up_async(d_slot_mask, G.slot_mask.data(), G.slot_mask.size() * 8));
        for (const Wave& W : G.waves) {
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
        int* oC = on_device ? (counts ? counts + G.q0 : nullptr) : d_C;
        if (part) {
            // device pointers: the group's rows of every plane of the caller's block; host pointers: the staged planes, Q * k words apart
            int* oP = on_device ? part + (size_t)G.q0 * k : d_P;
            const long long plane = on_device ? (long long)nq * k : (long long)Q * k;
            union_finish_part_kernel<<<(int)gq, 64, lds, st>>>(d_lists, d_slot_n, d_slot_base, d_slot_pos0, nb, LR, k,
                                                              C.qn2 ? C.qn2 + G.q0 : nullptr, h->ids_slab.as<unsigned>(), oP, plane, oC);
            HIPCHK(hipGetLastError());
            if (!on_device)
                for (int pl = 0; pl < LMI_UNION_PART_PLANES; ++pl)
                    HIPCHK(hipMemcpyAsync(part + ((size_t)pl * nq + G.q0) * k, d_P + (size_t)pl * plane, (size_t)gq * k * 4,
                                          hipMemcpyDeviceToHost, st));
        } else {
            float* oD = on_device ? dists + (size_t)G.q0 * k : d_D;
            unsigned* oI = on_device ? ids + (size_t)G.q0 * k : d_I;
            union_finish_kernel<<<(int)gq, 64, lds, st>>>(d_lists, d_slot_n, d_slot_base, d_slot_pos0, nb, LR, k,
                                                         C.qn2 ? C.qn2 + G.q0 : nullptr, h->ids_slab.as<unsigned>(), oD, oI, oC);
            HIPCHK(hipGetLastError());
            if (!on_device) {
                HIPCHK(hipMemcpyAsync(dists + (size_t)G.q0 * k, d_D, (size_t)gq * k * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(ids + (size_t)G.q0 * k, d_I, (size_t)gq * k * 4, hipMemcpyDeviceToHost, st));
            }
        }
        if (!on_device && counts) HIPCHK(hipMemcpyAsync(counts + G.q0, d_C, (size_t)gq * 4, hipMemcpyDeviceToHost, st));
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
// how every form except the part begins: the plan words cleared, then the refusals that need no pointer
int union_begin(lmi_index* h, const char* who, int nq, int nb, int k, const UnionFilter& uf) {
    for (int64_t& w : g_union_last) w = 0;
    for (int64_t& w : g_filter_last) w = 0;
    if (!h) return fail("%s: NULL handle", who);
    CHK(union_check(h, who, nq, nb, k));
    if (uf.asked) CHK(filter_check(h, who, uf.f, uf.filter_of, nq));
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
                           float* dists, uint32_t* ids, int32_t* counts, int on_device, const UnionFilter& uf) {
    CHK(union_begin(h, who, nq, nb, k, uf));
    if (nq == 0) return 0;
    if (!queries_search || !bucket_order || !dists || !ids) return fail("%s: queries_search, bucket_order, dists and ids must not be NULL", who);
    CHK(set_dev(h));
    const void* d_qs = nullptr;
    const void* d_order = nullptr;
    CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &d_qs));
    CHK(input_ptr(h, bucket_order, (size_t)nq * nb * 4, on_device, h->order, &d_order));
    begin_call(h);
    return union_core(h, who, static_cast<const float*>(d_qs), nq, static_cast<const int*>(d_order), nb, k, dists, ids, counts, on_device,
                      nullptr, uf.f, uf.filter_of);
}
extern "C" LMI_API int lmi_scan_union(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                      float* dists, uint32_t* ids, int32_t* counts, int on_device) {
    return scan_union_impl("lmi_scan_union", h, queries_search, nq, bucket_order, nb, k, dists, ids, counts, on_device, UnionFilter{});
}
extern "C" LMI_API int lmi_scan_union_filtered(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                               float* dists, uint32_t* ids, int32_t* counts, int on_device, const lmi_filter* f,
                                               const int32_t* filter_of) {
    return scan_union_impl("lmi_scan_union_filtered", h, queries_search, nq, bucket_order, nb, k, dists, ids, counts, on_device,
                           UnionFilter{true, f, filter_of});
}

extern "C" LMI_API int lmi_scan_union_part(lmi_index* h, const float* queries_search, int nq, const int32_t* bucket_order, int nb, int k,
                                           int32_t* part, int32_t* counts, int on_device) {
    const char* who = "lmi_scan_union_part";
    for (int64_t& w : g_union_last) w = 0;
    for (int64_t& w : g_filter_last) w = 0;
    if (!h) return fail("%s: NULL handle", who);
    CHK(union_check(h, who, nq, nb, k));
    if (nq == 0) return 0;
    if (!queries_search || !bucket_order || !part) return fail("%s: queries_search, bucket_order and part must not be NULL", who);
    CHK(set_dev(h));
    const void* d_qs = nullptr;
    const void* d_order = nullptr;
    CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &d_qs));
    CHK(input_ptr(h, bucket_order, (size_t)nq * nb * 4, on_device, h->order, &d_order));
    begin_call(h);
    return union_core(h, who, static_cast<const float*>(d_qs), nq, static_cast<const int*>(d_order), nb, k, nullptr, nullptr, counts, on_device,
                      part);
}

static int search_union_impl(const char* who, lmi_index* h, const float* queries_nav, const float* queries_search, int nq, int nb, int k,
                             float* dists, uint32_t* ids, int32_t* counts, int32_t* bucket_order, int on_device, const UnionFilter& uf) {
    CHK(union_begin(h, who, nq, nb, k, uf));
    if (h->root().n_layers == 0) return fail("%s: no MLP set (lmi_set_mlp)", who);
    if (h->root().dims.back() != h->L) return fail("%s: MLP has %d classes, index has %d buckets", who, h->root().dims.back(), h->L);
    if (nq == 0) return 0;
    if (!queries_nav || !queries_search || !dists || !ids) return fail("%s: queries_nav, queries_search, dists and ids must not be NULL", who);
    CHK(set_dev(h));
    const void* d_qn = nullptr;
    const void* d_qs = nullptr;
    CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &d_qn));
    if (queries_search == queries_nav && h->root().dims[0] == h->d_user) d_qs = d_qn;
    else CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &d_qs));
    int* d_order = bucket_order;
    if (!on_device || !bucket_order) { CHK(h->order.reserve((size_t)nq * nb * 4)); d_order = h->order.as<int>(); }
    begin_call(h);
    CHK(mlp_enqueue(h, static_cast<const float*>(d_qn), nq, nb, d_order, nullptr));
    CHK(union_core(h, who, static_cast<const float*>(d_qs), nq, d_order, nb, k, dists, ids, counts, on_device, nullptr, uf.f, uf.filter_of));
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
    const void* d_qn = nullptr;
    const void* d_qs = nullptr;
    CHK(input_ptr(h, queries_nav, (size_t)nq * h->root().dims[0] * 4, on_device, h->q_nav, &d_qn));
    if (queries_search == queries_nav && h->root().dims[0] == h->d_user) d_qs = d_qn;
    else CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &d_qs));
    CHK(h->nav_slab.reserve((size_t)nq * nb * 4));
    CHK(h->nav_ent.reserve((size_t)nq * nb * 4));
    int* d_slab = (on_device && slab_ids) ? slab_ids : h->nav_slab.as<int>();
    int* d_ent = (on_device && entries) ? entries : h->nav_ent.as<int>();
    begin_call(h);
    CHK(nav_enqueue(h, static_cast<const float*>(d_qn), nq, nb, d_slab, d_ent));
    CHK(union_core(h, who, static_cast<const float*>(d_qs), nq, d_slab, nb, k, dists, ids, counts, on_device, nullptr, uf.f, uf.filter_of));
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
