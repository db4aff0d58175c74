// lmi_host_knn_range.h -- lmi_knn_range: the exact range query over a whole base with no index (kernels: lmi_knn_range.h; the
// geometry, offsets, lims and gathers: lmi_knn_range_plan.h; include/lmi_hip.h states the contract).  The frame is lmi_knn's
// (open_device, CallScratch, upload_pieces, the NULL stream of the device) and the schedule lmi_host_range.h's: per query group pack
// the queries (L2: their norms), then per piece of the base (upload,) norms, scores, count; the piece's counts come back to the host
// (ONE synchronisation per piece); a chunk of exactly the piece's results is allocated, the offsets go up, emit.  Behind the last group
// the final arrays are allocated once at lims[nq] and every (query, piece) run is gathered (one descriptor table, one synchronisation).
// lmi_knn_range, lmi_debug_knn_range_plan.  The result is an lmi_range_result (lmi_host_range.h) with nb = 1.
// lmi_knn_range_f16 is the same implementation (knn_range_run) on halves, through lmi_host_knn.h's source-type overloads.
#pragma once
#include "lmi_host_knn.h"
#include "lmi_host_range.h"
#include "lmi_knn_range.h"
#include "lmi_knn_range_plan.h"

namespace {

thread_local int64_t g_knn_range_last[LMI_KNN_RANGE_PLAN_COUNT] = {};

// a result without results: lims all zero, every query's one pair count zero
lmi_range_result* knn_range_empty(int device, int64_t nq) {
    lmi_range_result* r = new lmi_range_result();
    r->device = device;
    r->nb = 1;
    r->lims.assign((size_t)nq + 1, 0);
    r->pair_count.assign((size_t)nq, 0);
    return r;
}

template <class T>
int knn_range_run(const char* who, int device, const T* xq, int64_t nq, const T* xb, int64_t nb, int d, int metric, const float* radius,
                  int64_t max_total, lmi_range_result** result, int on_device);

}  // namespace

extern "C" LMI_API int lmi_debug_knn_range_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_knn_range_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_KNN_RANGE_PLAN_COUNT); ++i) out[i] = g_knn_range_last[i];
    return 0;
}

extern "C" LMI_API int lmi_knn_range(int device, const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int metric,
                                     const float* radius, int64_t max_total, lmi_range_result** result, int on_device) {
    return knn_range_run<float>("lmi_knn_range", device, xq, nq, xb, nb, d, metric, radius, max_total, result, on_device);
}

extern "C" LMI_API int lmi_knn_range_f16(int device, const uint16_t* xq, int64_t nq, const uint16_t* xb, int64_t nb, int d, int metric,
                                         const float* radius, int64_t max_total, lmi_range_result** result, int on_device) {
    return knn_range_run<uint16_t>("lmi_knn_range_f16", device, xq, nq, xb, nb, d, metric, radius, max_total, result, on_device);
}

namespace {

template <class T>
int knn_range_run(const char* who, int device, const T* xq, int64_t nq, const T* xb, int64_t nb, int d, int metric, const float* radius,
                  int64_t max_total, lmi_range_result** result, int on_device) {
    namespace kp = lmi_knn_plan;
    namespace krp = lmi_knn_range_plan;
    for (int64_t& w : g_knn_range_last) w = 0;
    if (result) *result = nullptr;
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    if (nq < 0 || nq >= (1ll << 31)) return fail("%s: nq %lld outside [0, 2^31)", who, (long long)nq);
    if (nb < 0 || nb >= (1ll << 31)) return fail("%s: nb %lld outside [0, 2^31)", who, (long long)nb);
    if (metric != LMI_METRIC_IP && metric != LMI_METRIC_L2) return fail("%s: unknown metric %d", who, metric);
    if (!result) return fail("%s: the result pointer is NULL", who);
    if (nq > 0 && !radius) return fail("%s: radius is NULL", who);
    if (nq > 0 && !xq) return fail("%s: xq must not be NULL", who);
    if (nq > 0 && nb > 0 && !xb) return fail("%s: xb must not be NULL", who);
    if (max_total < 0) return fail("%s: max_total %lld is negative", who, (long long)max_total);
    if (nq == 0) {
        *result = knn_range_empty(device, 0);
        return 0;
    }
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));

    const bool l2 = metric == LMI_METRIC_L2;
    const krp::Plan P = krp::make_plan(nq, nb, d, l2, on_device != 0, (int64_t)free_b, prop.multiProcessorCount, g_knn_forced, (int)sizeof(T));
    const kp::Plan& p = P.g;
    const int KG = p.kg;
    CallScratch mem(who), chunks(who);
    float *d_S = nullptr, *d_qn = nullptr, *d_xnh = nullptr, *d_radius = nullptr;
    T *d_xq = nullptr, *d_xb = nullptr;
    float4* d_qf = nullptr;
    int* d_counts = nullptr;
    long long* d_off = nullptr;
    CHK(mem.alloc(&d_S, p.slab_bytes, "score slab"));
    CHK(mem.alloc(&d_qf, p.qfrag_bytes, "query fragments"));
    CHK(mem.alloc(&d_qn, p.qn_bytes, "query norms"));
    CHK(mem.alloc(&d_xnh, p.xnh_bytes, "base norms"));
    if (!on_device) {
        CHK(mem.alloc(&d_xq, p.xq_bytes, "queries"));
        CHK(mem.alloc(&d_xb, p.xb_bytes, "base piece"));
    }
    CHK(mem.alloc(&d_radius, P.radius_bytes, "radius"));
    CHK(mem.alloc(&d_counts, P.count_bytes, "stretch counts"));
    CHK(mem.alloc(&d_off, P.offset_bytes, "stretch offsets"));
    HIPCHK(hipMemcpy(d_radius, radius, (size_t)nq * 4, hipMemcpyHostToDevice));
    // 16-byte loads of the base: as in lmi_knn
    const bool vec_xb = knn_vec_xb(on_device ? xb : d_xb, d);

    // what a (group, piece) leaves behind for the gather: its chunk and its runs
    struct PieceOut {
        float* D = nullptr;
        unsigned* I = nullptr;
    };
    std::vector<PieceOut> outs;
    std::vector<krp::PieceRuns> runs;
    krp::Totals tot(nq);
    std::vector<int> counts((size_t)(p.query_rows * p.splits));
    std::vector<long long> off(counts.size());
    int64_t counted = 0, chunk_bytes = 0;
    for (int64_t g = 0; g < p.query_groups && p.pieces > 0; ++g) {
        int64_t q0, q1;
        kp::group_range(p, g, &q0, &q1);
        const int gq = (int)(q1 - q0), nct = cdiv(gq, 32), ct = nct >= 3 ? 4 : nct;
        const size_t slots = (size_t)gq * p.splits;
        const T* gxq = xq + (size_t)q0 * d;
        if (!on_device) {
            CHK(upload_pieces(d_xq, gxq, (size_t)gq * d * sizeof(T)));
            gxq = d_xq;
        }
        knn_pack_queries(gxq, l2 ? 1.0f : 0.0f, gq, d, nct, KG, d_qf);
        if (l2) knn_norms(gxq, gq, d, 0, d_qn);
        HIPCHK(hipGetLastError());
        const float* qn = l2 ? d_qn : nullptr;
        for (int64_t i = 0; i < p.pieces; ++i) {
            int64_t r0, r1;
            kp::piece_range(p, i, &r0, &r1);
            const long long len = r1 - r0;
            const T* px = xb + (size_t)r0 * d;
            if (!on_device) {
                CHK(upload_pieces(d_xb, px, (size_t)len * d * sizeof(T)));
                px = d_xb;
            }
            if (l2) knn_norms(px, len, d, 1, d_xnh);
            CHK(knn_score_piece(vec_xb, ct, px, len, d, l2 ? d_xnh : nullptr, d_qf, KG, nct, gq, d_S, p.pitch));
            knn_range_count_kernel<<<dim3(gq, p.splits), 64>>>(d_S, p.pitch, len, qn, d_radius + q0, d_counts);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy(counts.data(), d_counts, slots * 4, hipMemcpyDeviceToHost));   // the piece's one synchronisation
            runs.push_back(krp::chunk_offsets(counts.data(), q0, gq, p.splits, off.data()));
            outs.emplace_back();
            const krp::PieceRuns& R = runs.back();
            counted += krp::add_piece(tot, R);
            if (krp::over_total(counted, max_total))
                return fail("%s: more than max_total = %lld results: %lld had been counted when the call stopped (group %lld of "
                            "%lld, piece %lld of %lld); nothing further was launched",
                            who, (long long)max_total, (long long)counted, (long long)g + 1, (long long)p.query_groups, (long long)i + 1,
                            (long long)p.pieces);
            if (R.total == 0) continue;
            PieceOut& O = outs.back();
            CHK(chunks.alloc(&O.D, (size_t)R.total * 4, "result chunk (dists)"));
            CHK(chunks.alloc(&O.I, (size_t)R.total * 4, "result chunk (ids)"));
            chunk_bytes += R.total * 8;
            HIPCHK(hipMemcpy(d_off, off.data(), slots * 8, hipMemcpyHostToDevice));
            knn_range_emit_kernel<<<dim3(gq, p.splits), 64>>>(d_S, p.pitch, len, (unsigned)r0, qn, d_radius + q0, d_counts, d_off, O.D, O.I);
            HIPCHK(hipGetLastError());
        }
    }

    lmi_range_result* r = knn_range_empty(device, nq);
    r->lims = krp::make_lims(tot);
    r->pair_count = tot.per_query;
    const int64_t total = r->lims.back();
    // the gathers: every piece's descriptors back to back in one table, one upload, one launch per piece that produced results
    auto finish = [&]() -> int {
        if (total == 0) return 0;
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&r->dists), (size_t)total * 4));
        HIPCHK(hipMalloc(reinterpret_cast<void**>(&r->ids), (size_t)total * 4));
        const krp::Gather G = krp::gather_of(runs, r->lims);
        long long *d_src = nullptr, *d_dst = nullptr;
        int* d_n = nullptr;
        CHK(mem.alloc(&d_src, G.src.size() * 8, "run sources"));
        CHK(mem.alloc(&d_dst, G.dst.size() * 8, "run targets"));
        CHK(mem.alloc(&d_n, G.n.size() * 4, "run lengths"));
        HIPCHK(hipMemcpy(d_src, G.src.data(), G.src.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_dst, G.dst.data(), G.dst.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_n, G.n.data(), G.n.size() * 4, hipMemcpyHostToDevice));
        for (size_t j = 0; j < runs.size(); ++j) {
            const size_t a = G.first[j], n = G.first[j + 1] - a;
            if (n == 0) continue;
            range_gather_kernel<<<(unsigned)n, 64>>>(outs[j].D, outs[j].I, d_src + a, d_dst + a, d_n + a, r->dists, r->ids);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(nullptr));   // the result is complete; the descriptors and the chunks may go
        return 0;
    };
    if (finish() != 0) {
        (void)hipStreamSynchronize(nullptr);
        delete r;
        return -1;
    }
    g_knn_range_last[LMI_KNN_RANGE_PLAN_PIECES] = p.pieces;
    g_knn_range_last[LMI_KNN_RANGE_PLAN_PIECE_ROWS] = p.piece_rows;
    g_knn_range_last[LMI_KNN_RANGE_PLAN_SPLITS] = p.splits;
    g_knn_range_last[LMI_KNN_RANGE_PLAN_QUERY_GROUPS] = p.query_groups;
    g_knn_range_last[LMI_KNN_RANGE_PLAN_QUERY_ROWS] = p.query_rows;
    g_knn_range_last[LMI_KNN_RANGE_PLAN_RESULTS] = total;
    g_knn_range_last[LMI_KNN_RANGE_PLAN_CHUNK_BYTES] = chunk_bytes;
    g_knn_range_last[LMI_KNN_RANGE_PLAN_WORKSPACE_BYTES] = mem.total;
    *result = r;
    return 0;
}

}  // namespace
