// lmi_host_scan.h -- the bucket scan of one batch on the host side.  scan_plan() decides the call's shape and form from
// (handle, nq, n_buckets, k) alone; scan_enqueue() runs the stages in order on h->stream, each a function of its own:
//   scan_augment_l2 -> scan_reserve -> scan_route_arrays -> front_fused | front_separate
//   -> exact_scan | (record(2) -> prefilter_passes -> overflow_arm [-> overflow_redo] -> rerank -> scan_fallback) -> final_merge
// lmi_workspace_bytes sums the sizes scan_reserve asks for, from the same plan.
#pragma once
#include "lmi_host.h"

// the exact re-rank runs in its streamed form (select_kernel + rescore_kernel, lmi_rescore.h) for these shapes
static bool rescore_is_streamed(const lmi_index* h) {
    return h->rescore_streamed && rc_waves_for(h->dp, 4) > 0 && rc_wave_lds(h->dp, 4, true) <= RC_SMALL_LDS_CAP;
}
static int rescore_group_size(int nb) { return nb % 4 == 0 ? 4 : nb % 3 == 0 ? 3 : nb % 2 == 0 ? 2 : 1; }

// Everything about one scan call that is decided before its first launch.
struct ScanPlan {
    int nq, nb, kout, L;
    long long nslots;      // nq x nb (a scan call: < 2^31, check_scan_args)
    long long ncb_bound;   // col-blocks: every bucket's last one may be partly filled
    long long ncols;       // 32 x ncb_bound
    int max_nch;           // the largest bucket's chunk count
    long long part_lists;  // partial lists of the exact scan (the prefilter path writes rank lists, not chunk partials: 1)
    bool fast;             // fp16 prefilter + exact re-rank (lmi_prefilter.h, lmi_pass2.h); otherwise the all-f32 scan_kernel
    bool low_d;            // low_d_form() of the index: pass2_small_kernel instead of pass2_kernel
    bool ps_wide;          // the low-dimensional kernels' wide form (one 8-wave block per CU, 12-col-block tiles)
    int tile_cb;           // col-blocks per query tile
    int sample_max;        // pass 1's largest sampling stride
    bool qbound;           // one bound per query (query_bound_kernel) ...
    int primary_nb;        // ... and pass 1 samples the primary slots only (> 0: = nb)
    bool use_front;        // route_kernel + pack_kernel (lmi_front.h) instead of the eight preparation launches
    bool streamed;         // rescore_is_streamed()
    int G, groups, sub_cap;        // the re-rank's slots of one query per wave, its groups, the sub-lists' capacity (groups and sub_cap
                                   // mean something for a scan call only: lmi_workspace_bytes may plan nslots >= 2^31 and does not read them)
    bool use_tail, tail_merges;    // tail_kernel (lmi_tail.h) instead of the five launches; it also merges the ranks (G == nb)
};

static ScanPlan scan_plan(const lmi_index* h, int nq, int nb, int kout) {
    ScanPlan P;
    P.nq = nq; P.nb = nb; P.kout = kout; P.L = h->L;
    P.nslots = (long long)nq * nb;
    P.ncb_bound = P.nslots / 32 + P.L + 4;
    P.ncols = P.ncb_bound * 32;
    P.fast = h->prefilter && h->have16;
    // partial-list bound (exact mode only): a row of bucket_order is caller data and may repeat a bucket, so a query owns at most
    // nb x the largest chunk count
    P.max_nch = 0;
    for (int b = 0; b < P.L; ++b) P.max_nch = std::max(P.max_nch, h->h_nch[b]);
    P.part_lists = P.fast ? 1 : std::max<long long>(1, (long long)nb * P.max_nch * nq);
    P.low_d = low_d_form(h, h->KG16);
    // low-dimensional kernels: the wide form when the visited buckets receive more queries than the narrow form's tile holds --
    // decided from the call's shape alone (no device round trip)
    P.ps_wide = false;
    if (P.fast && P.low_d) {
        const double per_bucket = (double)nq * nb / std::max(1, std::min(h->n_nonempty, (int)std::min<long long>((long long)nq * nb, 1 << 30)));
        P.ps_wide = h->ps_force_wide >= 0 ? h->ps_force_wide != 0 : ps_use_wide(h->KG16, per_bucket);
    }
    P.tile_cb = !P.fast ? 4 : P.low_d ? ps_tile_cb(h->KG16, P.ps_wide) : P2_MAXCB;   // lmi_pass2.h: tiles of up to 12 col-blocks
    P.sample_max = (P.fast && h->pf_small && h->KG16 <= PF_SAMPLE_LOWD_KG) ? PF_SAMPLE_LOWD : PF_SAMPLE;
    // one bound per QUERY is enough when the caller keeps the k <= 10 best over all ranks (query_bound_kernel, lmi_pass2.h): pass 1
    // then samples only each query's primary slot(s) -- a quarter of the columns at n_buckets = 4
    P.qbound = P.fast && h->pf_qbound && nb > 1 && kout <= KPB;
    P.primary_nb = (P.qbound && h->pf_primary) ? nb : 0;
    // front (lmi_front.h): routing, query norms / packing / bounds and the fills in two launches -- for moderate fan-outs and batches
    P.use_front = P.fast && h->use_front && P.L <= FR_MAX_L && P.nslots <= FR_MAX_SLOTS && h->d <= FR_MAX_D;
    P.streamed = rescore_is_streamed(h);
    P.G = rescore_group_size(nb);
    P.groups = (int)std::min<long long>(P.nslots / P.G, INT32_MAX);
    P.sub_cap = cdiv(P.groups, RC_SUB);
    // the fused tail (lmi_tail.h): a wave per query selects, re-ranks and merges -- n_buckets <= 4 (a query's slots in ONE wave).
    // tail_kernel also runs group-wise (8 buckets: two waves of 4 + merge_ranks_kernel; LMI_TAIL=2), but there the five launches are
    // faster -- 4M x 768, 16 buckets: re-rank 0.39 against 0.25 ms; 4M x 45, 2 000 leaves, 8 buckets: 0.23 against 0.18: most of the
    // 160 000+ slots have nothing to re-rank, which select_kernel's compacted lists skip and a wave per group does not
    P.use_tail = P.fast && P.streamed && h->use_tail && (P.G == nb || h->use_tail == 2) &&
                 RC_WAVES * tail_wave_lds(h->dp, P.G, true) <= RC_SMALL_LDS_CAP;
    P.tail_merges = P.use_tail && P.G == nb;
    return P;
}

// ---- the instances the launch sites pick on top of the plan: each condition is ONE function, called by the launch and by the
// plan report (plan_report, lmi_debug_plan), so that the report cannot drift from the launch ----
// route_kernel<NB>: the rank counts it is specialised for; 0: the generic instance
static int route_nb_template(int nb) {
    switch (nb) {
        case 1: case 2: case 3: case 4: case 5: case 6: case 8: case 10: case 16: return nb;
        default: return 0;
    }
}
// pack_kernel<GS, CP, vec>: lanes per row and chunks per lane by the row's 8-float chunks; vec: whole chunks only
struct PackForm { int gs, cp; bool vec; };
static PackForm pack_form(int d) {
    const int nchunk = (d + 7) / 8;
    PackForm f;
    f.gs = nchunk <= 8 ? 8 : nchunk <= 16 ? 16 : nchunk <= 32 ? 32 : 64;
    f.cp = nchunk <= 64 ? 1 : nchunk <= 128 ? 2 : 4;
    f.vec = d % 8 == 0;
    return f;
}
// route_group_kernel: the bucket sort in LDS, or (huge fan-outs) the same sort in a global scratch buffer
static bool route_sort_global(int L) { return L > ROUTE_MAX_BUCKETS; }
// rescore_kernel's small form keeps four waves as long as a block stays under its LDS cap
static int rescore_small_waves(int dp, int G) { return RC_WAVES * rc_wave_lds(dp, G, true) <= RC_SMALL_LDS_CAP ? RC_WAVES : 1; }
// who writes the caller's rows: 0 the fused tail (tail_kernel / fallback_kernel), 1 merge_ranks_kernel (rank lists exist: a thread
// per query), 2 merge_kernel
static int merge_kind(const ScanPlan& P) { return P.tail_merges ? 0 : (P.fast && P.nb <= 16) ? 1 : 2; }

static_assert(LMI_PLAN_COUNT <= CallState::PLAN_WORDS, "lmi_handle.h holds the plan words");
// The LMI_PLAN_* words of a call (include/lmi_hip.h): the plan's fields, and the launch sites' choices as the functions above give
// them for the sites this plan reaches (-1: not launched).  lmi_debug_plan returns this; scan_enqueue starts the handle's record
// with the plan's fields only (plan_record) and every launch site writes its own word as it launches.
static void plan_record(const lmi_index* h, const ScanPlan& P, int32_t* w) {
    for (int i = 0; i < LMI_PLAN_COUNT; ++i) w[i] = -1;
    w[LMI_PLAN_FAST] = P.fast; w[LMI_PLAN_LOW_D] = P.low_d; w[LMI_PLAN_PS_WIDE] = P.ps_wide; w[LMI_PLAN_TILE_CB] = P.tile_cb;
    w[LMI_PLAN_SAMPLE_MAX] = P.sample_max; w[LMI_PLAN_QBOUND] = P.qbound; w[LMI_PLAN_PRIMARY_NB] = P.primary_nb;
    w[LMI_PLAN_USE_FRONT] = P.use_front; w[LMI_PLAN_STREAMED] = P.streamed; w[LMI_PLAN_G] = P.G; w[LMI_PLAN_USE_TAIL] = P.use_tail;
    w[LMI_PLAN_TAIL_MERGES] = P.tail_merges; w[LMI_PLAN_KG16] = h->KG16; w[LMI_PLAN_DP] = h->dp;
}
static void plan_report(const lmi_index* h, const ScanPlan& P, int32_t* w) {
    plan_record(h, P, w);
    if (P.use_front) {
        const PackForm pf = pack_form(h->d);
        w[LMI_PLAN_ROUTE_NB_TEMPLATE] = route_nb_template(P.nb);
        w[LMI_PLAN_PACK_GS] = pf.gs; w[LMI_PLAN_PACK_CP] = pf.cp; w[LMI_PLAN_PACK_VEC] = pf.vec;
    } else {
        w[LMI_PLAN_ROUTE_SORT_GLOBAL] = route_sort_global(P.L);
    }
    if (P.fast && P.streamed && !P.use_tail) w[LMI_PLAN_RESCORE_SMALL_WAVES] = rescore_small_waves(h->dp, P.G);
    w[LMI_PLAN_MERGE_KIND] = merge_kind(P);
}

// one call's arguments and what its stages hand on
struct ScanCall {
    ScanPlan P;
    const float* q;     // [nq][d]: the queries at the stored width
    const float* qn2;   // L2: |q|^2 (else null)
    const int* order;   // [nq][nb]
    int raw;
    float* out_d; uint32_t* out_id; uint32_t* out_key;   // the caller's rows [nq][kout]
    RouteArrays R;
    FillRanges Z;       // what the front stage's first launch initialises
};
// the end-of-launch cells of the device stamps (head [32, 36): pass 2, scan_kernel)
static unsigned long long* p2_end_cell(lmi_index* h) { return reinterpret_cast<unsigned long long*>(h->head.as<unsigned>() + 32); }
static unsigned long long* scan_end_cell(lmi_index* h) { return reinterpret_cast<unsigned long long*>(h->head.as<unsigned>() + 34); }

// pass 1 (SAMPLE) / pass 2 of the fp16 prefilter: the low-dimensional form for d <= 128 (lmi_pass2_small.h), else lmi_pass2.h
template <bool SAMPLE>
static int launch_pass2(lmi_index* h, const ScanPlan& P, const PrefilterParams& F) {
    if (P.low_d) {
        const bool wide = P.ps_wide;
        const int grid = h->num_cus * ps_blocks_per_cu(F.KG16, wide), lds = ps_lds_bytes(F.KG16, wide) - (SAMPLE ? ps_spill_bytes(F.KG16, wide) : 0);
#define LMI_PS_CASE(K) case K: \
            if (wide && ps_has_wide(K)) pass2_small_kernel<K, SAMPLE, ps_has_wide(K)><<<grid, 64 * ps_waves(K, true), lds, h->stream>>>(F); \
            else pass2_small_kernel<K, SAMPLE, false><<<grid, 64 * ps_waves(K, false), lds, h->stream>>>(F); \
            break;
        switch (F.KG16) {
            LMI_PS_CASE(1) LMI_PS_CASE(2) LMI_PS_CASE(3) LMI_PS_CASE(4) LMI_PS_CASE(5) LMI_PS_CASE(6) LMI_PS_CASE(7) LMI_PS_CASE(8)
            default: return fail("internal: KG16 = %d outside the low-dimensional form (%s:%d)", F.KG16, __FILE__, __LINE__);
        }
#undef LMI_PS_CASE
    } else {
        pass2_kernel<SAMPLE><<<h->num_cus * P2_BLOCKS_PER_CU, 64 * P2_WAVES, 0, h->stream>>>(F);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// stage 1 -- L2: queries [nq][d_user] -> [q, 1, 0..] of the stored width, |q|^2 aside
static int scan_augment_l2(lmi_index* h, ScanCall& C, const float* d_qs) {
    C.q = d_qs;
    C.qn2 = nullptr;
    if (h->metric != LMI_METRIC_L2) return 0;
    const int nq = C.P.nq;
    CHK(h->q_aug.reserve((size_t)nq * h->d * 4));
    CHK(h->qn2.reserve((size_t)nq * 4));
    augment_copy_kernel<<<cdiv((long long)nq * h->d, 256), 256, 0, h->stream>>>(d_qs, h->d_user, h->d, nq, h->q_aug.as<float>());
    HIPCHK(hipGetLastError());
    augment_norm_kernel<<<cdiv(nq, 256), 256, 0, h->stream>>>(d_qs, h->d_user, h->d, nq, h->q_aug.as<float>(), h->qn2.as<float>());
    HIPCHK(hipGetLastError());
    C.q = h->q_aug.as<float>();
    C.qn2 = h->qn2.as<float>();
    return 0;
}

// stage 2 -- the call's workspaces, and the ranges the front stage's first launch fills (C.Z)
static int scan_reserve(lmi_index* h, ScanCall& C) {
    const ScanPlan& P = C.P;
    const int L = P.L;
    const size_t nslots = (size_t)P.nslots, ncols = (size_t)P.ncols;
    CHK(h->m.reserve((size_t)L * 4 * 3));   // m [L] | m0 [L] | the non-primary slots' counter [L]
    CHK(h->cb_start.reserve((L + 1) * 4));
    CHK(h->item_base.reserve((L + 1) * 4));
    CHK(h->part_base.reserve((L + 1) * 8));
    CHK(h->stats.reserve(32));
    CHK(h->head.reserve(256));   // [0, 32): queue heads | [32, 36): the end-of-launch cells of the device stamps (pass 2, scan_kernel)
    const size_t grp_ints = (size_t)NGRP * L + 2 * (size_t)NGRP * (L + 1) + 3 * NGRP + (size_t)L;   // (+ the call's chunk length per bucket)
    CHK(h->grp.reserve(grp_ints * 4));
    CHK(h->slot_local.reserve(nslots * 4));
    CHK(h->slot_col.reserve(nslots * 4));
    CHK(h->colmap.reserve(ncols * 4));
    CHK(h->col_thr.reserve(ncols * 4));
    CHK(h->qfrag.reserve((size_t)P.ncb_bound * h->KGs * 1024));
    CHK(h->part_score.reserve((size_t)P.part_lists * KPB * 4));
    CHK(h->part_row.reserve((size_t)P.part_lists * KPB * 4));
    CHK(h->rank_d.reserve(nslots * KPB * 4));
    CHK(h->rank_id.reserve(nslots * KPB * 4));

    FillRanges& Z = C.Z;
    Z.count = 0;
    Z.ts = nullptr;
    bool fill_ok = true;
    auto fill = [&](void* ptr, long long words, unsigned value) { fill_ok = Z.add(ptr, words, value) && fill_ok; };
    // route_kernel's blocks compute m / m0 and set their own columns' pass-1 lists, so those fills are not queued with the front
    if (!P.use_front) fill(h->m.p, 3ll * L, 0u);
    fill(h->head.p, 64, 0u);   // [0..8] pass-2 queue heads + the pass-1 head, [16..24) the heads of pass 2's redo launch, [32..36) stamp cells
    if (!P.use_front) fill(h->colmap.p, P.ncols, 0xFFFFFFFFu);
    fill(h->col_thr.p, P.ncols, 0xFF800000u /* -inf */);
    if (P.fast) {
        CHK(h->qnorm.reserve((size_t)P.nq * 4));
        CHK(h->qdelta.reserve((size_t)P.nq * 4));
        CHK(h->qscale.reserve((size_t)P.nq * 4));
        CHK(h->qfrag16.reserve((size_t)P.ncb_bound * h->KG16 * 1024 + 8192));   // (+ 8 KiB: the same look-ahead on the query fragments)
        CHK(h->eps2.reserve(ncols * 4));
        CHK(h->cand_cnt.reserve(ncols * 4));
        CHK(h->cand_row.reserve(ncols * PF_CAP * 4));
        CHK(h->cand_s.reserve(ncols * PF_CAP * 4));
        CHK(h->fallback.reserve(nslots * 4));
        CHK(h->nkeep.reserve(nslots * 4));
        const size_t bound_words = ncols * P2_NSL * 16;   // pass 1: [P2_NSL lists][16 slots][columns]
        CHK(h->pf_bound.reserve(bound_words * 4 + 4096));  // + room for the developer builds' phase stamps
        if (!P.use_front) fill(h->pf_bound.p, (long long)bound_words, 0xFF800000u /* -inf */);
        fill(h->cand_cnt.p, P.ncols, 0u);
        fill(h->stats.as<long long>() + 2, 4, 0u);
        CHK(h->redo.reserve((size_t)(1 + L) * 4 + ncols));
        fill(h->redo.p, (long long)(1 + L) + (long long)((ncols + 3) / 4), 0u);
        CHK(h->fb_list.reserve((8 + nslots) * 4));
        fill(h->fb_list.p, 8, 0u);   // fallback count, fail flags of the two pass-2 launches, log head, sorted total
        if (h->x_cap == 0) {         // the overflow log (16 B an entry) and its sorted form (8 B): allocated with the first prefilter batch
            const size_t cap = (size_t)1 << LMI_PF_X_LOG2;
            CHK(h->x_log.reserve(cap * 16));
            CHK(h->x_ext.reserve(cap * 8));
            h->x_cap = (unsigned)cap;
        }
        CHK(h->x_off.reserve(ncols * 4));
        if (P.streamed) {   // the streamed re-rank's flags and list counters (lmi_rescore.h): zeroed here, not by a launch of their own
            CHK(h->rs_flag.reserve((size_t)P.groups * 4));
            CHK(h->rs_active.reserve((size_t)(RC_SUB + RC_SUB * P.sub_cap) * 4 + (size_t)(1 + P.groups) * 4));
            fill(h->rs_flag.p, P.groups, 0u);
            fill(h->rs_active.p, RC_SUB, 0u);
            fill(h->rs_active.as<int>() + RC_SUB + RC_SUB * P.sub_cap, 1, 0u);
        }
    }
    if (!fill_ok) return fail("internal: more than %d fill ranges queued (%s:%d)", FillRanges::MAXR, __FILE__, __LINE__);
    return 0;
}

// stage 3 -- the routing kernels' view of the workspaces, and the call's graded chunk levels
static void scan_route_arrays(lmi_index* h, const ScanPlan& P, RouteArrays& R) {
    const int L = P.L;
    R.nb_rows = h->d_nb_rows.as<int>();
    R.nch = h->d_nch.as<int>();
    R.m = h->m.as<int>();
    R.m0 = R.m + L;
    R.cb_start = h->cb_start.as<int>();
    R.item_base = h->item_base.as<int>();
    R.part_base = h->part_base.as<long long>();
    R.stats = h->stats.as<long long>();
    R.grp_bucket = h->grp.as<int>();
    R.grp_base = R.grp_bucket + (size_t)NGRP * L;
    R.grp_n = R.grp_base + (size_t)NGRP * (L + 1);
    R.grp_total = R.grp_n + NGRP;
    R.grp_base1 = R.grp_total + NGRP;
    R.grp_total1 = R.grp_base1 + (size_t)NGRP * (L + 1);
    R.dbg = nullptr;
    // graded pass-2 items (lmi_kernels.h RouteArrays): long chunks for the buckets a queue serves first, short ones for the last
    R.chunk_rb = h->chunk_rows / 32;
    R.chunk_rb_b = (P.fast && h->graded_chunks) ? R.grp_total1 + NGRP : nullptr;
    const int base = h->chunk_rows;
    int rows[3] = {base, base / 2, base / 4};   // (longer than the static chunk: no gain at C2, and a 4 096-row chunk of 768-d rows no longer fits an L2 beside a second query tile: hard leg +3.5 %)
    // d <= 128 (lmi_pass2_small.h): an item's start and end are a fifth of its time there and the rows are short -- twice the static chunk for the
    // buckets served first (10M x 45: pass 2 0.270 -> 0.256-0.262 ms; four times: 0.38, too few items for 512 workgroups)
    if (P.low_d) rows[0] = 2 * base;
    for (int i = 0; i < 3; ++i) {
        if (h->chunk_lvl_rows[i] > 0) rows[i] = h->chunk_lvl_rows[i];
        rows[i] = std::max(P2_TILE_ROWS, rows[i] / P2_TILE_ROWS * P2_TILE_ROWS);
        R.chunk_lvl[i] = rows[i] / 32;
    }
    R.chunk_frac[0] = h->chunk_frac[0];
    R.chunk_frac[1] = h->chunk_frac[1];
    R.tile_cb = P.tile_cb;
    R.sample_max = P.sample_max;
    R.sample_items = P.fast ? 1 : 0;
    R.primary_nb = P.primary_nb;
}

// stage 4, separate kernels: the fills, the routing (five launches; the work queues on the side stream) and, for the prefilter, the
// queries' norms, fp16 fragments and per-slot bounds.  The side stream is joined here on the prefilter path, by exact_scan otherwise.
static int front_separate(lmi_index* h, ScanCall& C) {
    const ScanPlan& P = C.P;
    const RouteArrays& R = C.R;
    const int L = P.L, nslots = (int)P.nslots;
    C.Z.ts = tsp(h, ST_FRONT);
    fill_ranges_kernel<<<h->num_cus * 4, 256, 0, h->stream>>>(C.Z);
    HIPCHK(hipGetLastError());
    route_count_kernel<<<cdiv(nslots, 256), 256, 0, h->stream>>>(C.order, nslots, L, R, h->slot_local.as<int>());
    HIPCHK(hipGetLastError());
    route_scan_kernel<<<1, 256, 0, h->stream>>>(L, R);
    HIPCHK(hipGetLastError());
    // the work queues (one 1 024-thread block, ~20 us) are only read by the scan kernels: built on the side stream while
    // this one packs the queries
    CHK(side_fork(h));
    const bool sort_global = route_sort_global(L);
    h->last_plan[LMI_PLAN_ROUTE_SORT_GLOBAL] = sort_global;
    if (!sort_global) {
        route_group_kernel<false><<<1, 1024, route_group_lds(L), h->side>>>(L, R, nullptr);
    } else {   // huge fan-outs: the same sort in a global scratch buffer
        CHK(h->grp_scratch.reserve(route_group_lds(L) + (size_t)L * 4));
        route_group_kernel<true><<<1, 1024, 0, h->side>>>(L, R, h->grp_scratch.as<char>());
    }
    HIPCHK(hipGetLastError());
    route_fill_kernel<<<cdiv(nslots, 256), 256, 0, h->stream>>>(C.order, h->slot_local.as<int>(), nslots, P.nb,
                                                               R.cb_start, R.m0, h->colmap.as<int>(), h->slot_col.as<int>());
    HIPCHK(hipGetLastError());
    if (!P.fast) return 0;   // (exact_scan packs the f32 fragments and joins the side stream)
    query_norm_kernel<<<cdiv(P.nq, 4), 256, 0, h->stream>>>(C.q, P.nq, h->d, h->qnorm.as<float>(), h->qdelta.as<float>(),
                                                            h->qscale.as<float>());
    HIPCHK(hipGetLastError());
    const long long total = P.ncols * h->KG16 * 2;
    pack_queries16_kernel<<<cdiv(total, 256), 256, 0, h->stream>>>(C.q, h->d, h->colmap.as<int>(), P.ncols,
                                                                  h->KG16, h->qscale.as<float>(), h->qfrag16.as<uint4>(), frag16x16(h));
    HIPCHK(hipGetLastError());
    slot_bound_kernel<<<cdiv(nslots, 256), 256, 0, h->stream>>>(C.order, h->slot_col.as<int>(), nslots, P.nb, h->KG16 * 16,
                                                               h->qnorm.as<float>(), h->qdelta.as<float>(),
                                                               h->bnorm.as<unsigned>(), h->bdelta.as<unsigned>(), h->eps2.as<float>());
    HIPCHK(hipGetLastError());
    CHK(side_join(h));   // the work queues
    return 0;
}

// the device word that tags route_kernel's granules (behind them in cb_alloc; bumped by bound_merge2_kernel)
static unsigned* front_epoch(lmi_index* h) { return reinterpret_cast<unsigned*>(h->cb_alloc.as<unsigned long long>() + FR_MAX_L + 1); }

// stage 4, lmi_front.h: route_kernel (routing + the fills) and pack_kernel (query norms, fp16 fragments, bounds)
static int front_fused(lmi_index* h, ScanCall& C) {
    const ScanPlan& P = C.P;
    const int L = P.L;
    FrontParams A;
    A.bucket_order = C.order;
    A.nq = P.nq; A.nb = P.nb; A.L = L;
    // granules [FR_MAX_L + 1] | the tag word (device-resident: a kernel argument would be frozen by a graph replay of this call)
    if (!h->cb_alloc.p) {
        CHK(h->cb_alloc.reserve((size_t)(FR_MAX_L + 2) * 8));
        HIPCHK(hipMemsetAsync(h->cb_alloc.p, 0, (size_t)(FR_MAX_L + 2) * 8, h->stream));
        front_epoch_bump_kernel<<<1, 1, 0, h->stream>>>(front_epoch(h));   // 0 -> 1
        HIPCHK(hipGetLastError());
    }
    CHK(h->cb_bucket.reserve((size_t)P.ncb_bound * 4));
    if (h->fr_bump_pending) {   // an earlier call left after route_kernel and before its bump: bump now
        front_epoch_bump_kernel<<<1, 1, 0, h->stream>>>(front_epoch(h));
        HIPCHK(hipGetLastError());
    }
    h->fr_bump_pending = true;   // (until prefilter_passes has launched bound_merge2_kernel)
    A.epoch_dev = front_epoch(h);
    A.gran = h->cb_alloc.as<unsigned long long>();
    A.cb_bucket = h->cb_bucket.as<int>();
    A.colmap = h->colmap.as<int>();
    A.R = C.R;
    A.R.dbg = h->fr_dbg.as<unsigned long long>();
    A.Z = C.Z;
    A.q = C.q;
    A.d = h->d; A.KG16 = h->KG16; A.f16x16 = frag16x16(h);
    A.qnorm = h->qnorm.as<float>(); A.qdelta = h->qdelta.as<float>(); A.qscale = h->qscale.as<float>();
    A.qfrag16 = h->qfrag16.as<uint4>();
    A.slot_col = h->slot_col.as<int>();
    A.eps2 = h->eps2.as<float>();
    A.bnorm = h->bnorm.as<unsigned>(); A.bdelta = h->bdelta.as<unsigned>();
    A.pf_bound = h->pf_bound.as<float>();
    A.ncols = P.ncols;
    A.bound_rows = P2_NSL * 16;
    A.ts = tsp(h, ST_FRONT);
    A.dbg = h->fr_dbg.as<unsigned long long>();
    const size_t rlds = fr_route_lds(L);
    const int nbt = route_nb_template(P.nb);
    switch (nbt) {   // the rank count as a compile-time constant: a wave's bucket ids of several steps are loaded at once (lmi_front.h, FrChunk)
#define LMI_FR_CASE(NBV) case NBV: route_kernel<NBV><<<L, FR_THREADS, rlds, h->stream>>>(A); break;
        LMI_FR_CASE(0) LMI_FR_CASE(1) LMI_FR_CASE(2) LMI_FR_CASE(3) LMI_FR_CASE(4) LMI_FR_CASE(5) LMI_FR_CASE(6) LMI_FR_CASE(8) LMI_FR_CASE(10) LMI_FR_CASE(16)
#undef LMI_FR_CASE
        default: return fail("internal: no route_kernel instance for the rank count %d (%s:%d)", nbt, __FILE__, __LINE__);
    }
    HIPCHK(hipGetLastError());
    h->last_plan[LMI_PLAN_ROUTE_NB_TEMPLATE] = nbt;
    A.ts = nullptr;
    const int pgrid = 1 + (int)P.ncb_bound;
    const size_t plds = fr_pack_lds(L, h->KG16);
    const PackForm pf = pack_form(h->d);
#define LMI_FP_LAUNCH(GSV, CPV) if (pf.gs == GSV && pf.cp == CPV) { \
                                    if (pf.vec) pack_kernel<GSV, CPV, true><<<pgrid, FP_THREADS, plds, h->stream>>>(A); \
                                    else pack_kernel<GSV, CPV, false><<<pgrid, FP_THREADS, plds, h->stream>>>(A); }
    LMI_FP_LAUNCH(8, 1)
    else LMI_FP_LAUNCH(16, 1)
    else LMI_FP_LAUNCH(32, 1)
    else LMI_FP_LAUNCH(64, 1)
    else LMI_FP_LAUNCH(64, 2)
    else LMI_FP_LAUNCH(64, 4)
    else return fail("internal: no pack_kernel instance <%d, %d> (%s:%d)", pf.gs, pf.cp, __FILE__, __LINE__);
#undef LMI_FP_LAUNCH
    HIPCHK(hipGetLastError());
    h->last_plan[LMI_PLAN_PACK_GS] = pf.gs; h->last_plan[LMI_PLAN_PACK_CP] = pf.cp; h->last_plan[LMI_PLAN_PACK_VEC] = pf.vec;
    return 0;
}

// stage 5 -- the all-f32 scan: f32 query fragments, then scan_kernel's chunk partials
static int exact_scan(lmi_index* h, ScanCall& C) {
    const ScanPlan& P = C.P;
    const RouteArrays& R = C.R;
    ScanParams S;
    S.slab = h->slab.as<float4>();
    S.qfrag = h->qfrag.as<float4>();
    S.KG = h->KGs;
    S.L = P.L;
    S.chunk_rb = h->chunk_rows / 32;
    S.rb_start = h->d_rb_start.as<int>();
    S.nb_rows = R.nb_rows;
    S.nch = R.nch;
    S.m = R.m;
    S.cb_start = R.cb_start;
    S.grp_bucket = R.grp_bucket;
    S.grp_base = R.grp_base;
    S.grp_n = R.grp_n;
    S.grp_total = R.grp_total;
    S.part_base = R.part_base;
    S.head = h->head.as<unsigned>();
    S.col_thr = h->col_thr.as<float>();
    S.part_score = h->part_score.as<float>();
    S.part_row = h->part_row.as<unsigned>();
    S.ts_end_cell = nullptr;
    const long long total = P.ncols * h->KGs;
    pack_gather_kernel<<<cdiv(total, 256), 256, 0, h->stream>>>(C.q, h->d, h->colmap.as<int>(), P.nq, P.ncols, h->KGs, h->qfrag.as<float4>());
    HIPCHK(hipGetLastError());
    CHK(side_join(h));   // the work queues
    CHK(record(h, 2));
    S.ts_start = tsp(h, ST_SCAN0);
    if (S.ts_start) { S.ts_end_cell = scan_end_cell(h); (void)tsp(h, ST_SCAN1); }
    scan_kernel<<<h->num_cus * h->scan_blocks_per_cu, 256, SCAN_LDS, h->stream>>>(S);
    HIPCHK(hipGetLastError());
    CHK(record(h, 3));
    return 0;
}

// what pass 1 and pass 2 of the fp16 prefilter read and write (lmi_prefilter.h); the stamps are set per launch
static void prefilter_params(lmi_index* h, const ScanCall& C, PrefilterParams& F) {
    const RouteArrays& R = C.R;
    F.slab16 = h->slab16.as<uint4>();
    F.qfrag16 = h->qfrag16.as<uint4>();
    F.KG16 = h->KG16;
    F.L = C.P.L;
    F.chunk_rb = R.chunk_rb;
    F.chunk_rb_b = R.chunk_rb_b;
    F.tile_cb = R.tile_cb;
    F.sample_max = R.sample_max;
    F.rb_start = h->d_rb_start.as<int>();
    F.nb_rows = R.nb_rows;
    F.nch = R.nch;
    F.m = R.m;
    F.m0 = R.m0;
    F.cb_start = R.cb_start;
    F.grp_bucket = R.grp_bucket;
    F.grp_base = R.grp_base;
    F.grp_n = R.grp_n;
    F.grp_total = R.grp_total;
    F.grp_base1 = R.grp_base1;
    F.grp_total1 = R.grp_total1;
    F.ncols = C.P.ncols;
    F.head = h->head.as<unsigned>();
    F.bound = h->pf_bound.as<float>();
    F.bound1 = h->col_thr.as<float>();
    F.eps2 = h->eps2.as<float>();
    F.cand_cnt = h->cand_cnt.as<unsigned>();
    F.cand_row = h->cand_row.as<unsigned>();
    F.cand_s = h->cand_s.as<float>();
    F.redo_count = nullptr; F.redo_bucket = nullptr; F.redo_col = nullptr;
    unsigned* fbw = h->fb_list.as<unsigned>();   // [0] fallback count, [1] / [2] fail flags, [3] log head, [4] sorted total
    F.x.log = h->x_log.as<uint4>();
    F.x.cap = h->x_cap;
    F.x.head = fbw + 3;
    F.x.fail = fbw + 1;
    F.x.launch = 0;
    h->stamps_off = ((size_t)C.P.ncols * P2_NSL * 16 * 4 + 255) / 256 * 256;
    F.stamps = reinterpret_cast<unsigned long long*>(static_cast<char*>(h->pf_bound.p) + h->stamps_off);
    F.ts_start = nullptr;
    F.ts_end_cell = nullptr;
}

// stage 6 -- pass 1 (slot maxima of the sampled tiles), the bounds' merge, pass 2 (candidates)
static int prefilter_passes(lmi_index* h, const ScanCall& C, PrefilterParams& F) {
    const ScanPlan& P = C.P;
    F.ts_start = tsp(h, ST_P1);
#if defined(LMI_P2_STAMPS)
    HIPCHK(hipMemsetAsync(F.stamps, 0, 2 * 8 * 12 * 8, h->stream));
#endif
    CHK(launch_pass2<true>(h, P, F));
    bound_merge2_kernel<<<cdiv(P.ncols, 64), 256, 0, h->stream>>>(F.bound, P.ncols, F.bound1, P.use_front ? front_epoch(h) : nullptr);
    HIPCHK(hipGetLastError());
    h->fr_bump_pending = false;
    if (P.qbound) {   // the caller keeps the k <= 10 best over all ranks: one bound per query
        query_bound_kernel<<<cdiv(P.nq, 256), 256, 0, h->stream>>>(h->slot_col.as<int>(), P.nq, P.nb, F.eps2, F.bound1);
        HIPCHK(hipGetLastError());
    }
    if (h->debug_emit_all) {  // test hook: bound = -inf, every row of the bucket is a candidate
        FillRanges D;
        D.count = 1; D.p[0] = reinterpret_cast<unsigned*>(F.bound1); D.n[0] = P.ncols; D.v[0] = 0xFF800000u; D.ts = nullptr;
        fill_ranges_kernel<<<h->num_cus * 4, 256, 0, h->stream>>>(D);
        HIPCHK(hipGetLastError());
    }
    CHK(record(h, 5));
    F.ts_start = tsp(h, ST_P2);
    F.ts_end_cell = F.ts_start ? p2_end_cell(h) : nullptr;
    if (F.ts_start) { (void)tsp(h, ST_CLK_WALL); (void)tsp(h, ST_CLK_CYC); }
    CHK(launch_pass2<false>(h, P, F));
    F.ts_start = nullptr;
    F.ts_end_cell = nullptr;
    CHK(record(h, 6));
    return 0;
}

// Stage 7a -- the one step of a scan that is NOT decided by the plan: it reads and writes handle state.
// The overflow machinery (overflow_rebound_kernel + pass 2's redo launch: two launches that return at once on ordinary batches,
// 11 us of a 0.2-0.5 ms search) stays OUT of the fused-tail sequence until a batch needs it: fallback_kernel then picks a flagged
// column's entries out of the unsorted log (or, log full, scans the bucket: always correct) and raises a flag in pinned host memory
// (h_oflag), read here; the next 1 000 calls (overflow_armed, counted down here) run with the machinery in.  The five-launch tail
// keeps it always.  Runs after pass 2 is enqueued and before the re-rank: *sorted says whether overflow_redo follows.
static int overflow_arm(lmi_index* h, const ScanPlan& P, bool* sorted) {
    if (P.use_tail && !h->h_oflag) {
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->h_oflag), 64, hipHostMallocMapped));
        *h->h_oflag = 0u;
    }
    if (P.use_tail && *reinterpret_cast<volatile unsigned*>(h->h_oflag) != 0u) { h->overflow_armed = 1000; *h->h_oflag = 0u; }
    *sorted = h->pf_redo && !h->debug_emit_all && (!P.use_tail || h->overflow_armed > 0);
    if (P.use_tail && h->overflow_armed > 0) --h->overflow_armed;
    return 0;
}

// stage 7b -- columns whose candidate buffer overflowed get the 10th best stored score as their bound and one more run of pass 2
// over their buckets (a launch that returns at once when there is none: ~15 us per batch; lmi_prefilter.h)
static int overflow_redo(lmi_index* h, const ScanCall& C, const PrefilterParams& F) {
    const int nslots = (int)C.P.nslots;
    unsigned* fbw = h->fb_list.as<unsigned>();
    unsigned* rc = h->redo.as<unsigned>();
    int* rb = reinterpret_cast<int*>(rc + 1);
    unsigned char* rcol = reinterpret_cast<unsigned char*>(rc + 1 + C.P.L);
    overflow_rebound_kernel<<<cdiv(nslots, 256), 256, 0, h->stream>>>(h->slot_col.as<int>(), C.order, nslots, F.cand_cnt, F.cand_s,
                                                                     F.bound1, rc, rb, rcol, F.x.fail, F.x.cap, h->x_off.as<unsigned>(), fbw + 4);
    HIPCHK(hipGetLastError());
    PrefilterParams F2 = F;
    F2.x.cap = 0;          // (only runs when the first launch filled the log: what overflows again takes the exact fallback)
    F2.x.fail = fbw + 2;
    F2.x.launch = 1;
    F2.head = F.head + 16;
    F2.redo_count = rc; F2.redo_bucket = rb; F2.redo_col = rcol;
    CHK(launch_pass2<false>(h, C.P, F2));
    return 0;
}

// what the re-rank and fallback_kernel read and write; overflow_sorted: overflow_rebound_kernel handed out the log's ranges
static void rescore_params(lmi_index* h, const ScanCall& C, const PrefilterParams& F, bool overflow_sorted, RescoreParams& Q) {
    const ScanPlan& P = C.P;
    unsigned* fbw = h->fb_list.as<unsigned>();
    Q.bucket_order = C.order;
    Q.slot_col = h->slot_col.as<int>();
    Q.nslots = (int)P.nslots;
    Q.nb = P.nb;
    Q.d = h->d;
    Q.raw = C.raw;
    Q.rb_start = h->d_rb_start.as<int>();
    Q.nb_rows = C.R.nb_rows;
    Q.cand_cnt = F.cand_cnt;
    Q.cand_row = F.cand_row;
    Q.cand_s = F.cand_s;
    Q.eps2 = F.eps2;
    Q.rows = h->rowmajor.as<float>();
    Q.dp = h->dp;
    Q.q = C.q;
    Q.qn2 = C.qn2;
    Q.ids_slab = h->ids_slab.as<unsigned>();
    Q.rank_d = h->rank_d.as<float>();
    Q.rank_id = h->rank_id.as<unsigned>();
    Q.fallback = h->fallback.as<int>();
    Q.nkeep = h->nkeep.as<int>();
    Q.fb_count = reinterpret_cast<int*>(fbw);
    Q.fb_list = reinterpret_cast<int*>(fbw + 8);
    Q.x_fail = fbw + 1;
    Q.x_off = overflow_sorted ? h->x_off.as<unsigned>() : nullptr;
    Q.x_ext = h->x_ext.as<uint2>();
    Q.x_log = F.x.log;
    Q.x_head = F.x.head;
    Q.x_cap = F.x.cap;
    Q.redo_col = overflow_sorted ? reinterpret_cast<const unsigned char*>(h->redo.as<unsigned>() + 1 + P.L) : nullptr;
    Q.ts = h->ts_set;
    Q.p2_end = p2_end_cell(h);
    if (Q.ts) { (void)tsp(h, ST_TAIL); (void)tsp(h, ST_P2END); (void)tsp(h, ST_FB); }
    Q.merge_pending = nullptr; Q.m_kout = 0; Q.m_out_d = nullptr; Q.m_out_id = nullptr; Q.m_out_key = nullptr;
#ifndef LMI_ABL_NOEMIT
    if (P.tail_merges) {   // tail_kernel / fallback_kernel write the caller's rows; rs_flag [groups] is used as [nq] (then groups == nq)
        Q.merge_pending = h->rs_flag.as<int>(); Q.m_kout = P.kout; Q.m_out_d = C.out_d; Q.m_out_id = C.out_id; Q.m_out_key = C.out_key;
        if (Q.ts) (void)tsp(h, ST_END);
    }
#endif
    Q.host_oflag = P.use_tail ? h->h_oflag : nullptr;
}
// LMI_STORAGE_F16: where the *16 kernels read the rows (RescoreParams::rows is null: no f32 image exists)
static Frag16 frag16_of(const lmi_index* h) {
    Frag16 F;
    F.frag = h->slab16.as<uint4>(); F.scale = h->xscale.as<float>(); F.KG16 = h->KG16; F.f16x16 = frag16x16(h);
    return F;
}

// stage 8 -- the exact re-rank of the candidates: tail_kernel | select_kernel + rescore_kernel x 2 | select_rescore_kernel
static int rerank(lmi_index* h, const ScanCall& C, const RescoreParams& Q) {
    const ScanPlan& P = C.P;
    const int nslots = (int)P.nslots, G = P.G, groups = P.groups;
    const bool f16 = h->storage == LMI_STORAGE_F16;
    if (!P.streamed) {
        if (f16) select_rescore_kernel<true><<<cdiv(nslots, RS_WAVES), 64 * RS_WAVES, 0, h->stream>>>(Q, frag16_of(h));
        else select_rescore_kernel<false><<<cdiv(nslots, RS_WAVES), 64 * RS_WAVES, 0, h->stream>>>(Q);
        HIPCHK(hipGetLastError());
        return 0;
    }
    CHK(h->surv_row.reserve((size_t)nslots * RC_KEEP * 4));
    SelectOut O;
    O.surv_row = h->surv_row.as<unsigned>();
    O.G = G;
    O.grp_flag = P.use_tail ? nullptr : h->rs_flag.as<int>();
    O.active = h->rs_active.as<int>();
    O.sub_cap = P.sub_cap;
    O.big = O.active + RC_SUB + RC_SUB * P.sub_cap;
    if (P.use_tail) {
        TailParams T;
        T.ngroups = groups; T.merge = P.tail_merges ? 1 : 0; T.kout = P.kout;
        T.out_d = C.out_d; T.out_id = C.out_id; T.out_key = C.out_key;
        T.pending = h->rs_flag.as<int>();   // [groups] (used as [nq] when the tail merges: then groups == nq)
        const int lds_s = RC_WAVES * tail_wave_lds(h->dp, G, true);
        const int blocks = cdiv(groups, RC_WAVES);
#define LMI_TL_LAUNCH(GV) { if (f16) tail_kernel<GV, true><<<blocks, 64 * RC_WAVES, lds_s, h->stream>>>(Q, O, T, frag16_of(h)); \
                           else tail_kernel<GV><<<blocks, 64 * RC_WAVES, lds_s, h->stream>>>(Q, O, T); }
        if (G == 4) LMI_TL_LAUNCH(4) else if (G == 3) LMI_TL_LAUNCH(3) else if (G == 2) LMI_TL_LAUNCH(2) else LMI_TL_LAUNCH(1)
#undef LMI_TL_LAUNCH
        HIPCHK(hipGetLastError());
        return 0;
    }
    // selection at full occupancy, then the survivors' rows streamed through LDS in coalesced pieces (lmi_rescore.h)
    select_kernel<<<cdiv(nslots, 4), 256, 0, h->stream>>>(Q, O);
    HIPCHK(hipGetLastError());
    // (wide rows: fewer waves per block in the big form, whose per-wave buffers hold the query and 256 survivors per slot; the small
    // form keeps four waves as long as a block stays under 64 KiB)
    const int wb = rc_waves_for(h->dp, G), ws = rescore_small_waves(h->dp, G);
    h->last_plan[LMI_PLAN_RESCORE_SMALL_WAVES] = ws;
    const int blocks = cdiv(groups, ws);
    const int lds = wb * rc_wave_lds(h->dp, G), lds_s = ws * rc_wave_lds(h->dp, G, true);
    // first every group in the small-LDS form (three blocks per CU), then the groups it passed on (more survivors than it holds)
#define LMI_RC_LAUNCH(GV) { if (f16) { rescore_kernel<GV, true, true><<<blocks, 64 * ws, lds_s, h->stream>>>(Q, O, frag16_of(h)); \
                                       rescore_kernel<GV, false, true><<<std::min(cdiv(groups, wb), h->num_cus), 64 * wb, lds, h->stream>>>(Q, O, frag16_of(h)); } \
                            else { rescore_kernel<GV, true><<<blocks, 64 * ws, lds_s, h->stream>>>(Q, O); \
                                   rescore_kernel<GV, false><<<std::min(cdiv(groups, wb), h->num_cus), 64 * wb, lds, h->stream>>>(Q, O); } }
    if (G == 4) LMI_RC_LAUNCH(4) else if (G == 3) LMI_RC_LAUNCH(3) else if (G == 2) LMI_RC_LAUNCH(2) else LMI_RC_LAUNCH(1)
#undef LMI_RC_LAUNCH
    HIPCHK(hipGetLastError());
    return 0;
}

// stage 9 -- the slots the re-rank flagged (overflowed candidate buffers, failed bounds): exact, from the log or the whole bucket
static int scan_fallback(lmi_index* h, const ScanCall& C, const RescoreParams& Q) {
    if (h->storage == LMI_STORAGE_F16) fallback_kernel<true><<<std::min(cdiv(C.P.nslots, 4), h->num_cus * 4), 256, 0, h->stream>>>(Q, frag16_of(h));
    else fallback_kernel<false><<<std::min(cdiv(C.P.nslots, 4), h->num_cus * 4), 256, 0, h->stream>>>(Q);
    HIPCHK(hipGetLastError());
    return 0;
}

// stage 10 -- the ranks' (or the exact scan's chunk partials') lists into the caller's rows, unless the fused tail already did
static int final_merge(lmi_index* h, const ScanCall& C) {
    const ScanPlan& P = C.P;
    const RouteArrays& R = C.R;
    MergeParams M;
    M.bucket_order = C.order;
    M.slot_col = h->slot_col.as<int>();
    M.nq = P.nq;
    M.nb = P.nb;
    M.L = P.L;
    M.kout = P.kout;
    M.raw = C.raw;
    M.skip_a = P.fast ? 1 : 0;
    M.rb_start = h->d_rb_start.as<int>();
    M.nb_rows = R.nb_rows;
    M.nch = R.nch;
    M.cb_start = R.cb_start;
    M.part_base = R.part_base;
    M.part_score = h->part_score.as<float>();
    M.part_row = h->part_row.as<unsigned>();
    M.ids_slab = h->ids_slab.as<unsigned>();
    M.qn2 = C.qn2;
    M.rank_d = h->rank_d.as<float>();
    M.rank_id = h->rank_id.as<unsigned>();
    M.ts = h->ts_set;
    M.scan_end = (!P.fast && h->ts_set) ? scan_end_cell(h) : nullptr;
    if (M.ts && !P.tail_merges) { (void)tsp(h, ST_MERGE); (void)tsp(h, ST_END); }
    M.out_d = C.out_d;
    M.out_id = C.out_id;
    M.out_key = C.out_key;
    const int kind = merge_kind(P);
    if (kind == 0) { /* merged by tail_kernel / fallback_kernel */ }
    else if (kind == 1) merge_ranks_kernel<<<cdiv(P.nq, 64), 64, 0, h->stream>>>(M);  // rank lists exist: a thread per query
    else merge_kernel<<<P.nq, 64, 0, h->stream>>>(M);
    HIPCHK(hipGetLastError());
    h->last_plan[LMI_PLAN_MERGE_KIND] = kind;
    return 0;
}

static int scan_enqueue(lmi_index* h, const float* d_qs, int nq, const int* d_order, int nb, int kout, int raw,
                        float* d_dists, uint32_t* d_ids, uint32_t* d_keys) {
    ScanCall C;
    C.P = scan_plan(h, nq, nb, kout);
    const ScanPlan& P = C.P;
    C.order = d_order; C.raw = raw;
    C.out_d = d_dists; C.out_id = d_ids; C.out_key = d_keys;
    plan_record(h, P, h->last_plan);   // (the launch sites add their words)
    CHK(scan_augment_l2(h, C, d_qs));
    CHK(scan_reserve(h, C));
    scan_route_arrays(h, P, C.R);
    CHK(P.use_front ? front_fused(h, C) : front_separate(h, C));
    if (!P.fast) {
        CHK(exact_scan(h, C));
    } else {   // fp16 prefilter + exact re-rank (lmi_prefilter.h)
        CHK(record(h, 2));
        PrefilterParams F;
        prefilter_params(h, C, F);
        CHK(prefilter_passes(h, C, F));
        bool overflow_sorted = false;
        CHK(overflow_arm(h, P, &overflow_sorted));
        if (overflow_sorted) CHK(overflow_redo(h, C, F));
        h->last_plan[LMI_PLAN_OVERFLOW_SORTED] = overflow_sorted;
        RescoreParams Q;
        rescore_params(h, C, F, overflow_sorted, Q);
#ifndef LMI_ABL_NOEMIT  // timing-only ablation builds emit nothing: no re-rank, no fallback
        CHK(rerank(h, C, Q));
#endif
        CHK(record(h, 7));
#ifndef LMI_ABL_NOEMIT
        CHK(scan_fallback(h, C, Q));
#endif
        CHK(record(h, 3));
    }
    CHK(final_merge(h, C));
    CHK(record(h, 4));
    h->stats_pending = true;
    h->last_nslots = (int)P.nslots;
    h->last_nb = nb;
    h->last_ncols = P.ncols;
    h->last_fast = P.fast;
    return 0;
}

// Device memory one lmi_search / lmi_scan_topk call of nq queries x nb buckets needs for its per-call workspaces (the
// sizes scan_reserve asks for, summed; host-pointer calls add the staged inputs and outputs).  A caller with a memory budget
// sizes its query chunks from this instead of a constant (li/LearnedIndex.py).
extern "C" LMI_API int lmi_workspace_bytes(lmi_index* h, int nq, int nb, int64_t* bytes) {
    if (!h || !bytes) return fail("lmi_workspace_bytes: NULL argument");
    if (nq < 0 || nb < 1) return fail("lmi_workspace_bytes: bad nq/n_buckets");
    if (!h->built) return fail("lmi_workspace_bytes: the bucket index is not built");
    const ScanPlan P = scan_plan(h, nq, nb, KPB);   // (k does not enter the sizes)
    const long long L = P.L, nslots = P.nslots, ncb = P.ncb_bound, ncols = P.ncols;
    long long t = 0;
    t += nslots * (4 + 4 + 2 * KPB * 4);                         // slot_local, slot_col, rank lists
    t += ncols * (4 + 4) + ncb * h->KGs * 1024;                  // colmap, col_thr, f32 query fragments
    t += (long long)nq * h->d * 4 * 2 + nslots * 4 + (long long)nq * std::max(nb, KPB) * 12;   // staged queries, bucket order, outputs
    if (P.fast) {
        t += (long long)nq * 12 + ncb * h->KG16 * 1024;           // query norms / scales, fp16 query fragments
        t += ncols * (4 + 4 + 2ll * PF_CAP * 4 + 1);             // eps2, candidate counts + buffers, redo flags
        t += ncols * P2_NSL * 16 * 4 + 4096;                     // pass-1 lists
        t += nslots * (4 + 4 + (long long)RC_KEEP * 4) + nslots; // fallback, nkeep, survivor rows, re-rank lists
        t += nslots * 4 + 32 + ncols * 4;                        // fallback list, overflow offsets
        t += ((long long)1 << LMI_PF_X_LOG2) * (16 + 8);         // the handle's overflow log + its sorted form (96 MiB, allocated with the first prefilter batch:
                                                                 // part of what a caller's memory budget must leave room for, whatever nq is)
    } else {
        t += P.part_lists * KPB * 8;                             // chunk partial lists of the exact scan
    }
    t += L * (3 * NGRP + 16) * 4;                                // per-bucket routing arrays, the work queues, the call's chunk lengths
    if (h->metric == LMI_METRIC_L2) t += (long long)nq * (h->d + 1) * 4;
    *bytes = t;
    return 0;
}
