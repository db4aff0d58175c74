// lmi_host_knn_exact.h -- the exact k-NN through the index (kernels: lmi_knn_exact.h; the words, the seed budget and the split:
// lmi_knn_exact_plan.h; include/lmi_hip.h states the contract): lmi_search_knn_exact, lmi_debug_knn_exact_plan.
// No reference counterpart (the reference answers a k-NN query from the buckets its model ranks first and has no exact form).
// One call, five steps on the handle's stream:
//   1  per query group: the bound of every (query, bucket) pair as a 64-bit word, then the seeds of every query;
//   2  the union scan's part form over the seeds (union_core, unchanged), the part on the device; tau from its k-th entry;
//   3  tau comes to the host (4 nq bytes, with the seed counts: ONE synchronisation) and goes into the pruning pass as it stands
//      (CoverPass, lmi_host_cover.h), whose counts decide nb of the second scan or refuse the call;
//   4  the split: the admitted order loses the seeds, the seed part's ranks move to the admitted order's numbering; the second part;
//   5  lmi_merge_union_parts's kernel over the two parts (world = 2) into the caller's arrays.
// Every bucket is scored at most once; nothing is written to the caller's arrays before step 5.
#pragma once
#include "lmi_host_cover.h"
#include "lmi_host_comm.h"
#include "lmi_knn_exact.h"
#include "lmi_knn_exact_plan.h"

static_assert(LMI_KNN_EXACT_MAX_SEEDS == lmi_knn_exact_plan::MAX_SEEDS, "lmi_knn_exact_plan.h restates LMI_KNN_EXACT_MAX_SEEDS");

namespace {

thread_local int64_t g_knn_exact_last[LMI_KNN_EXACT_PLAN_COUNT] = {};

int knn_exact_impl(lmi_index* h, const lmi_cover* c, const char* who, const float* queries_search, int nq, int k, float* dists, uint32_t* ids,
                   int32_t* counts, int32_t* visited, int on_device) {
    namespace kp = lmi_knn_exact_plan;
    namespace cp = lmi_cover_plan;
    hipStream_t st = h->stream;
    const int L = c->L, S = kp::MAX_SEEDS;
    const void* qs = nullptr;
    CHK(input_ptr(h, queries_search, (size_t)nq * h->d_user * 4, on_device, h->q_srch, &qs));
    const float* d_qs = static_cast<const float*>(qs);
    begin_call(h);

    CallScratch mem(who);
    const int64_t Q = kp::query_rows_for(g_cover_query_rows, nq, L), groups = cp::groups_for(nq, Q);
    const size_t part_words = (size_t)LMI_UNION_PART_PLANES * nq * k;
    unsigned long long* d_words = nullptr;
    double* d_qn = nullptr;
    float* d_tau = nullptr;
    int *d_seeds = nullptr, *d_nseeds = nullptr, *d_parts = nullptr, *d_rest = nullptr, *d_visited = nullptr;
    CHK(mem.alloc(&d_words, (size_t)kp::word_bytes(Q, L), "bound words"));
    CHK(mem.alloc(&d_qn, (size_t)nq * 8, "query norms"));
    CHK(mem.alloc(&d_seeds, (size_t)nq * S * 4, "seed order"));
    CHK(mem.alloc(&d_nseeds, (size_t)nq * 4, "seed counts"));
    CHK(mem.alloc(&d_tau, (size_t)nq * 4, "radii"));
    CHK(mem.alloc(&d_parts, 2 * part_words * 4, "parts"));

    // 1: bounds and seeds
    cover_qnorm_kernel<<<cdiv(nq, 256), 256, 0, st>>>(d_qs, nq, c->d, d_qn);
    HIPCHK(hipGetLastError());
    for (int64_t g = 0; g < groups; ++g) {
        const int64_t q0 = g * Q;
        const int gq = (int)std::min<int64_t>(Q, nq - q0);
        const dim3 grid((unsigned)cdiv(gq, COVER_Q_PER_BLOCK), (unsigned)cdiv(L, 64));
        knn_exact_bound_kernel<<<grid, 256, 0, st>>>(c->metric, d_qs + (size_t)q0 * c->d, d_qn + q0, gq, c->d, c->centres, c->radius, c->d_nb_rows, L,
                                                    d_words);
        HIPCHK(hipGetLastError());
        knn_exact_seed_kernel<<<gq, 64, 0, st>>>(d_words, c->d_nb_rows, L, k, d_seeds + (size_t)q0 * S, d_nseeds + q0);
        HIPCHK(hipGetLastError());
    }

    // 2: the seed part and tau
    CHK(union_core(h, who, d_qs, nq, d_seeds, S, k, UnionOut{nullptr, nullptr, d_parts, nullptr, true}, 1));
    knn_exact_tau_kernel<<<cdiv(nq, 256), 256, 0, st>>>(d_parts, nq, k, d_tau);
    HIPCHK(hipGetLastError());

    // 3: tau to the host, the pruning pass
    std::vector<float> tau((size_t)nq);
    std::vector<int32_t> nseeds((size_t)nq);
    HIPCHK(hipMemcpyAsync(tau.data(), d_tau, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(nseeds.data(), d_nseeds, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    CoverPass P(h, c, who);
    CHK(P.open(d_qs, nq, tau.data(), d_qn));   // |q| is step 1's
    CHK(P.count());
    if (P.max_count > cp::MAX_ORDER_BUCKETS) {
        int32_t unused = 0;
        const int64_t bad = cp::first_over(P.counts.data(), nq, cp::MAX_ORDER_BUCKETS, &unused);
        return fail("%s: query %lld needs %d buckets, more than the %d one union scan visits (splitting a query into several scans is not "
                    "offered); nothing was written",
                    who, (long long)bad, (int)P.counts[(size_t)bad], cp::MAX_ORDER_BUCKETS);
    }
    const int nb = std::max<int>(1, P.max_count);
    CHK(union_check(h, who, nq, nb, k));   // what the scan refuses of this nb

    // 4: the split and the second part
    CHK(mem.alloc(&d_rest, (size_t)nq * nb * 4, "rest order"));
    if (visited) CHK(mem.alloc(&d_visited, (size_t)nq * 4, "visited"));   // (staged for device pointers too: nothing of the caller's is written before step 5)
    CHK(P.write(d_rest, nb));
    int* d_missed = nullptr;
#ifdef LMI_DEBUG_CHECKS
    CHK(mem.alloc(&d_missed, 4, "missed seeds"));
    HIPCHK(hipMemsetAsync(d_missed, 0, 4, st));
#endif
    knn_exact_split_kernel<<<nq, 64, 0, st>>>(d_rest, P.d_counts, nb, d_seeds, d_parts, nq, k, d_visited, d_missed);
    HIPCHK(hipGetLastError());
#ifdef LMI_DEBUG_CHECKS
    {   // the rule admits every seed: each holds a row with dist <= tau, or tau is +inf
        int missed = 0;
        HIPCHK(hipMemcpyAsync(&missed, d_missed, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (missed != 0) return fail("%s: %d seed buckets were not admitted (the admission rule is broken)", who, missed);
    }
#endif
    CHK(union_core(h, who, d_qs, nq, d_rest, nb, k, UnionOut{nullptr, nullptr, d_parts + part_words, nullptr, true}, 1));

    // 5: the merge
    if (on_device) {
        CHK(union_merge_launch(h, d_parts, 2, nq, k, dists, ids, counts));
        if (visited) HIPCHK(hipMemcpyAsync(visited, d_visited, (size_t)nq * 4, hipMemcpyDeviceToDevice, st));
    } else {
        const size_t nout = (size_t)nq * k * 4;
        float* d_D = nullptr;
        unsigned* d_I = nullptr;
        int* d_C = nullptr;
        CHK(mem.alloc(&d_D, nout, "dists"));
        CHK(mem.alloc(&d_I, nout, "ids"));
        CHK(mem.alloc(&d_C, (size_t)nq * 4, "counts"));
        CHK(union_merge_launch(h, d_parts, 2, nq, k, d_D, d_I, d_C));
        HIPCHK(hipMemcpyAsync(dists, d_D, nout, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ids, d_I, nout, hipMemcpyDeviceToHost, st));
        if (counts) HIPCHK(hipMemcpyAsync(counts, d_C, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        if (visited) HIPCHK(hipMemcpyAsync(visited, d_visited, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));   // the outputs have landed; the call's buffers may go

    int64_t seed_buckets = 0, tau_inf = 0;
    for (int q = 0; q < nq; ++q) {
        seed_buckets += nseeds[(size_t)q];
        tau_inf += tau[(size_t)q] == INFINITY;
    }
    P.report(nb);
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_GROUPS] = groups;
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_QUERY_ROWS] = Q;
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_SEED_BUCKETS] = seed_buckets;
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_TAU_INF] = tau_inf;
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_ADMITTED] = P.admitted;
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_MAX_PER_QUERY] = P.max_count;
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_NB_REST] = nb;
    g_knn_exact_last[LMI_KNN_EXACT_PLAN_WORKSPACE_BYTES] = mem.total + P.mem.total;
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_search_knn_exact(lmi_index* h, const lmi_cover* c, const float* queries_search, int nq, int k, float* dists,
                                            uint32_t* ids, int32_t* counts, int32_t* visited, int on_device) {
    const char* who = "lmi_search_knn_exact";
    for (int64_t& w : g_knn_exact_last) w = 0;
    for (int64_t& w : g_cover_last) w = 0;
    // the seed scan's nb is LMI_KNN_EXACT_MAX_SEEDS whatever the index holds: what lmi_scan_union refuses of it, in its words
    CHK(union_begin(h, who, nq, lmi_knn_exact_plan::MAX_SEEDS, k, UnionFilter{}));
    CHK(cover_check(h, who, c));
    if ((long long)nq * k * 2 * LMI_UNION_PART_PLANES >= (1ll << 31)) return fail("%s: nq*k too large (the two parts hold 10 nq k words)", who);
    if (nq == 0) return 0;
    if (!queries_search || !dists || !ids) return fail("%s: queries_search, dists and ids must not be NULL", who);
    CHK(set_dev(h));
    if (knn_exact_impl(h, c, who, queries_search, nq, k, dists, ids, counts, visited, on_device) != 0) {
        (void)hipStreamSynchronize(h->stream);   // no kernel may still use the call's buffers, which have freed themselves
        for (int64_t& w : g_cover_last) w = 0;
        return -1;
    }
    return 0;
}

extern "C" LMI_API int lmi_debug_knn_exact_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_knn_exact_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_KNN_EXACT_PLAN_COUNT); ++i) out[i] = g_knn_exact_last[i];
    return 0;
}
