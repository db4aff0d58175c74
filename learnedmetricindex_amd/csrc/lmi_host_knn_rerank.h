// lmi_host_knn_rerank.h -- lmi_knn_rerank: argument checks, the candidate check and the schedule on the NULL stream of the device.
// knn_rerank_run mirrors knn_hamming_run (lmi_host_knn_hamming.h): the same call scratch, upload in pieces and loop over query groups
// and pieces, the plan of lmi_knn_plan.h for the groups and the pieces -- its score slab, query fragments and base norms are simply not
// allocated, there is one list per query (SPLITS = 1) of LR = rerank_list_rows(c) entries, and with device pointers the base is ONE
// piece unless lmi_knn_set_geometry forces piece_rows: nothing is uploaded, and every further piece would only send every wave over
// its 64 candidates once more.  The forced geometry and the last-plan words are lmi_knn's (g_knn_forced, g_knn_last).
// Device memory, Q = queries per group, P = rows per piece:  8 Q LR (lists) + 4 Q (qn); with device pointers 8 more (the candidate
// check's counter), with host pointers 4 Q d + 4 P d + 8 Q c + 12 Q k more (queries, piece, candidates, results).
#pragma once
#include "lmi_host_knn.h"
#include "lmi_knn_rerank.h"

namespace {

template <bool VEC>
void knn_rerank_score_launch(bool l2, int blocks, const float* px, long long r0, long long len, int d, const float* q, int gq,
                             const long long* cand, int c, int LR, knn_entry* lists) {
    if (l2) rerank_score_kernel<VEC, true><<<blocks, 64 * RR_WAVES>>>(px, r0, len, d, q, gq, cand, c, LR, lists);
    else rerank_score_kernel<VEC, false><<<blocks, 64 * RR_WAVES>>>(px, r0, len, d, q, gq, cand, c, LR, lists);
}

int knn_rerank_run(int device, const float* xq, int64_t nq, const float* xb, int64_t nb, int d, const int64_t* cand64, int c, int k,
                   int metric, float* D, int64_t* I, int on_device) {
    const char* who = "lmi_knn_rerank";
    for (int64_t& w : g_knn_last) w = 0;
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    if (c < 1 || c > LMI_KNN_MAX_K) return fail("%s: c %d outside [1,%d]", who, c, LMI_KNN_MAX_K);
    if (k < 1 || k > c) return fail("%s: k %d outside [1,c = %d]", who, k, c);
    if (nq < 0 || nq >= (1ll << 31)) return fail("%s: nq %lld outside [0, 2^31)", who, (long long)nq);
    if (nb < 0 || nb >= (1ll << 31)) return fail("%s: nb %lld outside [0, 2^31)", who, (long long)nb);
    if (metric != LMI_METRIC_IP && metric != LMI_METRIC_L2) return fail("%s: unknown metric %d", who, metric);
    if (nq > 0 && (!xq || !cand64 || !D || !I)) return fail("%s: xq, cand, D and I must not be NULL", who);
    if (nq > 0 && nb > 0 && !xb) return fail("%s: xb must not be NULL", who);
    if ((reinterpret_cast<uintptr_t>(xq) | reinterpret_cast<uintptr_t>(xb)) & 3) return fail("%s: xq and xb must be 4-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(cand64) & 7) return fail("%s: cand must be 8-byte aligned", who);
    if (nq == 0) return 0;
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));

    const long long* cand = reinterpret_cast<const long long*>(cand64);
    const long long ncand = (long long)nq * c;
    CallScratch mem(who);
    // one pass over cand before anything is scored: the entries outside [-1, nb)
    unsigned long long bad = 0;
    if (on_device) {
        unsigned long long* d_bad = nullptr;
        CHK(mem.alloc(&d_bad, sizeof(bad), "candidate check"));
        HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(bad), nullptr));
        rerank_check_kernel<<<(int)std::min<long long>(cdiv(ncand, 256), prop.multiProcessorCount * 8), 256>>>(cand, ncand, nb, d_bad);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
    } else {
        for (long long i = 0; i < ncand; ++i) bad += cand[i] < -1 || cand[i] >= nb;
    }
    if (bad) return fail("%s: %llu candidates outside [-1, nb = %lld)", who, bad, (long long)nb);

    const bool l2 = metric == LMI_METRIC_L2;
    // the groups and pieces are lmi_knn's for these sizes, its memory budget included: that budget counts the score slab, the query
    // fragments and the norms, which this call never allocates, and lists of k, not c, entries -- conservative (the slab outweighs
    // 8 Q LR by far), so groups or pieces may come out smaller than this call's own memory asks for; the result does not depend on it
    lmi_knn_plan::Plan p =lmi_knn_plan::make_plan(nq, nb, d, k, l2, on_device != 0, (int64_t)free_b, prop.multiProcessorCount, g_knn_forced);
    if (on_device && g_knn_forced.piece_rows <= 0) p.piece_rows = std::max<int64_t>(nb, 1);   // resident: one piece
    p.pieces = cdiv(nb, p.piece_rows);
    const int LR = rerank_list_rows(c);
    const int64_t Q = p.query_rows;
    float *d_qn = nullptr, *d_xq = nullptr, *d_xb = nullptr, *d_D = nullptr;
    knn_entry* d_lists = nullptr;
    long long *d_cand = nullptr, *d_I = nullptr;
    CHK(mem.alloc(&d_lists, (size_t)Q * LR * sizeof(knn_entry), "lists"));
    CHK(mem.alloc(&d_qn, (size_t)Q * 4, "query norms"));
    if (!on_device) {
        CHK(mem.alloc(&d_xq, (size_t)Q * d * 4, "queries"));
        CHK(mem.alloc(&d_xb, (size_t)p.piece_rows * d * 4, "base piece"));
        CHK(mem.alloc(&d_cand, (size_t)Q * c * 8, "candidates"));
        CHK(mem.alloc(&d_D, (size_t)Q * k * 4, "D"));
        CHK(mem.alloc(&d_I, (size_t)Q * k * 8, "I"));
    }
    // 16-byte loads of the rows: every row and every piece's first row stay aligned when the scanned base is
    const bool vec_xb = knn_vec_xb(on_device ? xb : d_xb, d);
    g_knn_last[LMI_KNN_PLAN_PIECES] = p.pieces;
    g_knn_last[LMI_KNN_PLAN_PIECE_ROWS] = p.piece_rows;
    g_knn_last[LMI_KNN_PLAN_SPLITS] = 1;
    g_knn_last[LMI_KNN_PLAN_QUERY_GROUPS] = p.query_groups;
    g_knn_last[LMI_KNN_PLAN_QUERY_ROWS] = p.query_rows;
    g_knn_last[LMI_KNN_PLAN_VEC_XQ] = 0;   // the query words are scalar loads
    g_knn_last[LMI_KNN_PLAN_VEC_XB] = vec_xb;
    g_knn_last[LMI_KNN_PLAN_WORKSPACE_BYTES] = mem.total;
    g_knn_last[LMI_KNN_PLAN_LIST_ROWS] = LR;

    const int wpq = cdiv(c, 64);
    for (int64_t g = 0; g < p.query_groups; ++g) {
        int64_t q0, q1;
        lmi_knn_plan::group_range(p, g, &q0, &q1);
        const int gq = (int)(q1 - q0);
        const float* gxq = xq + (size_t)q0 * d;
        const long long* gcand = cand + (size_t)q0 * c;
        if (!on_device) {
            CHK(upload_pieces(d_xq, gxq, (size_t)gq * d * 4));
            CHK(upload_pieces(d_cand, gcand, (size_t)gq * c * 8));
            gxq = d_xq;
            gcand = d_cand;
        }
        if (l2) {
            rerank_qnorm_kernel<<<cdiv(gq, 256), 256>>>(gxq, gq, d, d_qn);
            HIPCHK(hipGetLastError());
        }
        const long long nlist = (long long)gq * LR;
        knn_fill_kernel<<<(int)std::min<long long>(cdiv(nlist, 256), prop.multiProcessorCount * 8), 256>>>(d_lists, nlist);
        HIPCHK(hipGetLastError());
        for (int64_t i = 0; i < p.pieces; ++i) {
            int64_t r0, r1;
            lmi_knn_plan::piece_range(p, i, &r0, &r1);
            const long long len = r1 - r0;
            const float* px = xb + (size_t)r0 * d;
            if (!on_device) {
                CHK(upload_pieces(d_xb, px, (size_t)len * d * 4));
                px = d_xb;
            }
            const int blocks = (int)cdiv((long long)gq * wpq, RR_WAVES);
            if (vec_xb) knn_rerank_score_launch<true>(l2, blocks, px, r0, len, d, gxq, gq, gcand, c, LR, d_lists);
            else knn_rerank_score_launch<false>(l2, blocks, px, r0, len, d, gxq, gq, gcand, c, LR, d_lists);
            HIPCHK(hipGetLastError());
        }
        float* oD = on_device ? D + (size_t)q0 * k : d_D;
        long long* oI = on_device ? reinterpret_cast<long long*>(I) + (size_t)q0 * k : d_I;
        rerank_sort_kernel<<<gq, 64, (size_t)LR * sizeof(knn_entry)>>>(d_lists, LR, k, l2 ? d_qn : nullptr, oD, oI);
        HIPCHK(hipGetLastError());
        if (!on_device) {
            HIPCHK(hipMemcpy(D + (size_t)q0 * k, d_D, (size_t)gq * k * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(I + (size_t)q0 * k, d_I, (size_t)gq * k * 8, hipMemcpyDeviceToHost));
        }
    }
    HIPCHK(hipStreamSynchronize(nullptr));
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_knn_rerank(int device, const float* xq, int64_t nq, const float* xb, int64_t nb, int d, const int64_t* cand,
                                      int c, int k, int metric, float* D, int64_t* I, int on_device) {
    return knn_rerank_run(device, xq, nq, xb, nb, d, cand, c, k, metric, D, I, on_device);
}
