// lmi_host_candidates.h -- the candidate stage: what the union scan (lmi_host_union.h) and the range search (lmi_host_range.h) share up
// to and including the scores of every visited bucket.  Opening a stage augments the queries, brings the bucket order and the live
// bucket tables to the host (the call's one internal synchronisation before any launch), makes the plan and every group's tables
// (lmi_union_plan.h: pure host code, checked on the CPU) and allocates the buffers the shared kernels use; upload(G) sends a group's
// tables, score(W) launches pack and score for one wave.  What becomes of a wave's scores is the consumer's: it adds its own buffers
// to the stage's scratch, uploads its own per-slot arrays beside upload(G) and launches its kernels behind score(W).
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_host_filter.h"
#include "lmi_host_scan.h"
#include "lmi_union.h"
#include "lmi_union_plan.h"

static_assert(KNN_ROWS == lmi_union_plan::ITEM_ROWS, "lmi_union_plan.h restates the rows of a bucket that one item scores");

namespace {

thread_local lmi_union_plan::Forced g_union_forced;

template <bool VEC>
int union_score_launch(int ct, int n_items, hipStream_t st, const UnionItem* items, const float* rows, int dp, int d, const float4* Qf, int KG,
                       const long long* tile_off, const int* tile_cnt, float* S) {
    if (ct == 1) union_score_kernel<1, VEC><<<n_items, 256, 0, st>>>(items, rows, dp, d, Qf, KG, tile_off, tile_cnt, S);
    else if (ct == 2) union_score_kernel<2, VEC><<<n_items, 256, 0, st>>>(items, rows, dp, d, Qf, KG, tile_off, tile_cnt, S);
    else union_score_kernel<4, VEC><<<n_items, 256, 0, st>>>(items, rows, dp, d, Qf, KG, tile_off, tile_cnt, S);
    HIPCHK(hipGetLastError());
    return 0;
}

// The members are declared in the order the lifetimes need: the host tables (groups) are destroyed AFTER mem has freed the device
// buffers, whose frees wait for the uploads that still read those tables.
struct CandidateStage {
    lmi_index* h;
    ScanCall C;                // C.q: the queries at the stored width; C.qn2: |q|^2 (L2), else null
    lmi_union_plan::Plan p;
    std::vector<lmi_union_plan::Tables> groups;   // every group's tables
    lmi_union_plan::Extents ext;                  // and what the buffers are sized by
    bool vec = false;          // rows of the image start 16-byte aligned (dp % 4 == 0); d % 4 == 0 keeps every 16-byte load inside d
    CallScratch mem;           // the stage's buffers; a consumer adds its own, so that mem.total is the call's workspace
    float* d_S = nullptr;      // the score slab of one wave
    float4* d_qf = nullptr;
    UnionItem* d_items = nullptr;
    UnionSlot* d_slots = nullptr;
    int *d_rowq = nullptr, *d_tile_cnt = nullptr;
    long long *d_tile_off = nullptr, *d_slot_mask = nullptr;   // d_slot_mask: only with a filter

    CandidateStage(lmi_index* h_, const char* who) : h(h_), mem(who) {}

    // d_qs [nq][d_user] and d_order [nq][nb] on the device, already enqueued on h->stream.  k and on_device: what the plan is made
    // for.  f != nullptr (filter_check has passed): query q's candidates are the rows filter filter_of[q] allows (host [nq]; nullptr:
    // filter 0; -1: all rows); a slot whose (filter, bucket) pair allows no row is left out of the tables (lmi_union_plan.h).
    int open(const float* d_qs, int nq, const int* d_order, int nb, int k, bool on_device, const lmi_filter* f, const int32_t* filter_of) {
        namespace up = lmi_union_plan;
        hipStream_t st = h->stream;
        const int L = h->L;
        // L2: the queries at the stored width, [q, 1, 0..], and |q|^2
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
        p = up::make_plan(nq, nb, k, h->d, on_device, (int64_t)free_b, g_union_forced);
        vec = h->d % 4 == 0;
        const up::Layout layout{L, nrows.data(), rbs.data()};
        const up::FilterView fview{f ? f->counts.data() : nullptr, filter_of, f ? f->n_rb_total : 0};
        up::Groups built = up::build_groups(p, order.data(), layout, f ? &fview : nullptr);
        groups = std::move(built.groups);
        ext = built.ext;
        const up::Extents& e = ext;
        CHK(mem.alloc(&d_S, (size_t)e.slab_bytes, "score slab"));
        CHK(mem.alloc(&d_qf, (size_t)e.wave_tiles * p.kg * 1024, "query fragments"));
        CHK(mem.alloc(&d_items, (size_t)e.group_items * sizeof(UnionItem), "items"));
        CHK(mem.alloc(&d_slots, (size_t)e.group_slots * sizeof(UnionSlot), "slots"));
        CHK(mem.alloc(&d_rowq, (size_t)e.group_tiles * 32 * 4, "fragment rows"));
        CHK(mem.alloc(&d_tile_cnt, (size_t)e.group_tiles * 4, "tile counts"));
        CHK(mem.alloc(&d_tile_off, (size_t)e.group_tiles * 8, "tile offsets"));
        if (f) CHK(mem.alloc(&d_slot_mask, (size_t)e.group_slots * 8, "slot masks"));
        return 0;
    }

    // host -> device on the stream (nothing for no bytes); the source must live until the stream has been synchronised
    int up(void* dst, const void* src, size_t bytes) {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
        return 0;
    }
    // the shared tables of a group; the group before it must have left the stream (the consumer synchronises per group)
    int upload(const lmi_union_plan::Tables& G) {
        CHK(up(d_items, G.items.data(), G.items.size() * sizeof(UnionItem)));
        CHK(up(d_slots, G.slots.data(), G.slots.size() * sizeof(UnionSlot)));
        CHK(up(d_rowq, G.rowq.data(), G.rowq.size() * 4));
        CHK(up(d_tile_cnt, G.tile_cnt.data(), G.tile_cnt.size() * 4));
        CHK(up(d_tile_off, G.tile_off.data(), G.tile_off.size() * 8));
        if (d_slot_mask) CHK(up(d_slot_mask, G.slot_mask.data(), G.slot_mask.size() * 8));
        return 0;
    }
    // pack, then score: the scores of wave W's slots are in d_S when what follows on the stream runs.  W has slots.
    int score(const lmi_union_plan::Wave& W) {
        hipStream_t st = h->stream;
        const int KG = p.kg;
        union_pack_kernel<<<cdiv(W.tiles * 32 * KG, 256), 256, 0, st>>>(C.q, d_rowq + W.tile0 * 32, h->d, (int)W.tiles, KG, d_qf);
        HIPCHK(hipGetLastError());
        if (vec) return union_score_launch<true>(W.ct, (int)W.items, st, d_items + W.item0, h->rowmajor.as<float>(), h->dp, h->d, d_qf, KG,
                                                 d_tile_off + W.tile0, d_tile_cnt + W.tile0, d_S);
        return union_score_launch<false>(W.ct, (int)W.items, st, d_items + W.item0, h->rowmajor.as<float>(), h->dp, h->d, d_qf, KG,
                                         d_tile_off + W.tile0, d_tile_cnt + W.tile0, d_S);
    }
};

}  // namespace
