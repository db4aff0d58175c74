// lmi_host_knn.h -- lmi_knn: argument checks, the geometry (lmi_knn_plan.h), the call's device buffers, and the schedule on the NULL
// stream of the device: per query group pack the queries, then per piece of the base (upload,) norms, scores, selection; one merge of
// the split lists per group writes the group's rows.  lmi_knn_set_geometry, lmi_debug_knn_plan.
// lmi_knn_f16 is the same implementation (knn_run) on halves: the source type picks the half forms of the pack, the norms and the score
// kernel, the element size of the uploads and the plan, and the 16-byte rule; the schedule is written once.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_knn.h"
#include "lmi_knn_plan.h"

static_assert(LMI_KNN_MAX_K == lmi_knn_plan::MAX_K, "lmi_knn_plan.h restates LMI_KNN_MAX_K");

namespace {

thread_local lmi_knn_plan::Forced g_knn_forced;
thread_local int64_t g_knn_last[LMI_KNN_PLAN_COUNT] = {};

template <bool VEC>
int knn_score_launch(int ct, dim3 grid, const float* x, long long n, int d, const float* xnh, const float4* Qf, int KG, int nct, int nq,
                     float* S, long long pitch) {
    if (ct == 1) knn_score_kernel<1, VEC><<<grid, 256>>>(x, n, d, xnh, Qf, KG, nct, nq, S, pitch);
    else if (ct == 2) knn_score_kernel<2, VEC><<<grid, 256>>>(x, n, d, xnh, Qf, KG, nct, nq, S, pitch);
    else knn_score_kernel<4, VEC><<<grid, 256>>>(x, n, d, xnh, Qf, KG, nct, nq, S, pitch);
    HIPCHK(hipGetLastError());
    return 0;
}
// the half form: knn_score16_kernel
template <bool VEC>
int knn_score_launch(int ct, dim3 grid, const uint16_t* x, long long n, int d, const float* xnh, const float4* Qf, int KG, int nct, int nq,
                     float* S, long long pitch) {
    if (ct == 1) knn_score16_kernel<1, VEC><<<grid, 256>>>(x, n, d, xnh, Qf, KG, nct, nq, S, pitch);
    else if (ct == 2) knn_score16_kernel<2, VEC><<<grid, 256>>>(x, n, d, xnh, Qf, KG, nct, nq, S, pitch);
    else knn_score16_kernel<4, VEC><<<grid, 256>>>(x, n, d, xnh, Qf, KG, nct, nq, S, pitch);
    HIPCHK(hipGetLastError());
    return 0;
}

// What differs between the source types beside the kernels' own overloads: the query pack, the norms, and whether a base at `x` is read
// with 16-byte loads -- binary32: d % 4 == 0 keeps every row and every piece's first row aligned when the array's base is; halves:
// half_src_vec (d % 8 == 0).  x: the caller's pointer with on_device, the piece buffer otherwise.
void knn_pack_queries(const float* xq, float tail, int gq, int d, int nct, int KG, float4* qf) {
    dense_pack_kernel<<<cdiv((long long)nct * 32 * KG, 256), 256>>>(xq, nullptr, tail, gq, d, nct, KG, qf);
}
void knn_pack_queries(const uint16_t* xq, float tail, int gq, int d, int nct, int KG, float4* qf) {
    dense_pack16_kernel<<<cdiv((long long)nct * 32 * KG, 256), 256>>>(xq, tail, gq, d, nct, KG, qf);
}
void knn_norms(const float* x, long long n, int d, int neg_half, float* out) { dense_norm_kernel<<<cdiv(n, 64), 64>>>(x, n, d, neg_half, out); }
void knn_norms(const uint16_t* x, long long n, int d, int neg_half, float* out) { dense_norm16_kernel<<<cdiv(n, 64), 64>>>(x, n, d, neg_half, out); }
bool knn_vec_xb(const float* x, int d) { return d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0; }
bool knn_vec_xb(const uint16_t* x, int d) { return half_src_vec(x, d); }

// the scores of one (group, piece) into the slab, by the form of the score kernel the call chose
template <class T>
int knn_score_piece(bool vec_xb, int ct, const T* px, long long len, int d, const float* xnh, const float4* qf, int KG, int nct, int gq,
                    float* S, long long pitch) {
    const dim3 grid(cdiv(len, KNN_ROWS), cdiv(nct, ct));
    if (vec_xb) return knn_score_launch<true>(ct, grid, px, len, d, xnh, qf, KG, nct, gq, S, pitch);
    return knn_score_launch<false>(ct, grid, px, len, d, xnh, qf, KG, nct, gq, S, pitch);
}

template <class T>
int knn_run(const char* who, int device, const T* xq, int64_t nq, const T* xb, int64_t nb, int d, int k, int metric, float* D, int64_t* I,
            int on_device);

}  // namespace

extern "C" LMI_API int lmi_knn_set_geometry(int64_t piece_rows, int splits, int64_t query_rows) {
    if (piece_rows < 0 || piece_rows >= (1ll << 31)) return fail("lmi_knn_set_geometry: piece_rows %lld outside [0, 2^31)", (long long)piece_rows);
    if (splits < 0 || splits > lmi_knn_plan::MAX_SPLITS) return fail("lmi_knn_set_geometry: splits %d outside [0, %d]", splits, lmi_knn_plan::MAX_SPLITS);
    if (query_rows < 0 || query_rows > (1ll << 20)) return fail("lmi_knn_set_geometry: query_rows %lld outside [0, 2^20]", (long long)query_rows);
    g_knn_forced.piece_rows = piece_rows;
    g_knn_forced.splits = splits;
    g_knn_forced.query_rows = query_rows;
    return 0;
}

extern "C" LMI_API int lmi_debug_knn_plan(int64_t* out, int n) {
    if (!out || n < 0) return fail("lmi_debug_knn_plan: NULL argument");
    for (int i = 0; i < std::min(n, (int)LMI_KNN_PLAN_COUNT); ++i) out[i] = g_knn_last[i];
    return 0;
}

extern "C" LMI_API int lmi_knn(int device, const float* xq, int64_t nq, const float* xb, int64_t nb, int d, int k, int metric, float* D,
                               int64_t* I, int on_device) {
    return knn_run<float>("lmi_knn", device, xq, nq, xb, nb, d, k, metric, D, I, on_device);
}

extern "C" LMI_API int lmi_knn_f16(int device, const uint16_t* xq, int64_t nq, const uint16_t* xb, int64_t nb, int d, int k, int metric,
                                   float* D, int64_t* I, int on_device) {
    return knn_run<uint16_t>("lmi_knn_f16", device, xq, nq, xb, nb, d, k, metric, D, I, on_device);
}

namespace {

template <class T>
int knn_run(const char* who, int device, const T* xq, int64_t nq, const T* xb, int64_t nb, int d, int k, int metric, float* D, int64_t* I,
            int on_device) {
    for (int64_t& w : g_knn_last) w = 0;
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    if (k < 1 || k > LMI_KNN_MAX_K) return fail("%s: k %d outside [1,%d]", who, k, LMI_KNN_MAX_K);
    if (nq < 0 || nq >= (1ll << 31)) return fail("%s: nq %lld outside [0, 2^31)", who, (long long)nq);
    if (nb < 0 || nb >= (1ll << 31)) return fail("%s: nb %lld outside [0, 2^31)", who, (long long)nb);
    if (metric != LMI_METRIC_IP && metric != LMI_METRIC_L2) return fail("%s: unknown metric %d", who, metric);
    if (nq > 0 && (!xq || !D || !I)) return fail("%s: xq, D and I must not be NULL", who);
    if (nq > 0 && nb > 0 && !xb) return fail("%s: xb must not be NULL", who);
    if (nq == 0) return 0;
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));

    const bool l2 = metric == LMI_METRIC_L2;
    const lmi_knn_plan::Plan p = lmi_knn_plan::make_plan(nq, nb, d, k, l2, on_device != 0, (int64_t)free_b, prop.multiProcessorCount, g_knn_forced,
                                                         (int)sizeof(T));
    const int LR = p.list_rows, KG = p.kg;
    CallScratch mem(who);
    float *d_S = nullptr, *d_qn = nullptr, *d_xnh = nullptr, *d_D = nullptr;
    T *d_xq = nullptr, *d_xb = nullptr;   // halves stay halves: the piece buffer of lmi_knn_f16 holds what was uploaded
    float4* d_qf = nullptr;
    knn_entry* d_lists = nullptr;
    long long* d_I = nullptr;
    CHK(mem.alloc(&d_S, p.slab_bytes, "score slab"));
    CHK(mem.alloc(&d_lists, p.list_bytes, "lists"));
    CHK(mem.alloc(&d_qf, p.qfrag_bytes, "query fragments"));
    CHK(mem.alloc(&d_qn, p.qn_bytes, "query norms"));
    CHK(mem.alloc(&d_xnh, p.xnh_bytes, "base norms"));
    if (!on_device) {
        CHK(mem.alloc(&d_xq, p.xq_bytes, "queries"));
        CHK(mem.alloc(&d_xb, p.xb_bytes, "base piece"));
        CHK(mem.alloc(&d_D, p.d_bytes, "D"));
        CHK(mem.alloc(&d_I, p.i_bytes, "I"));
    }
    // 16-byte loads of the base: knn_vec_xb
    const bool vec_xb = knn_vec_xb(on_device ? xb : d_xb, d);
    g_knn_last[LMI_KNN_PLAN_PIECES] = p.pieces;
    g_knn_last[LMI_KNN_PLAN_PIECE_ROWS] = p.piece_rows;
    g_knn_last[LMI_KNN_PLAN_SPLITS] = p.splits;
    g_knn_last[LMI_KNN_PLAN_QUERY_GROUPS] = p.query_groups;
    g_knn_last[LMI_KNN_PLAN_QUERY_ROWS] = p.query_rows;
    g_knn_last[LMI_KNN_PLAN_VEC_XQ] = 0;   // dense_pack_kernel loads the queries element by element
    g_knn_last[LMI_KNN_PLAN_VEC_XB] = vec_xb;
    g_knn_last[LMI_KNN_PLAN_WORKSPACE_BYTES] = mem.total;
    g_knn_last[LMI_KNN_PLAN_LIST_ROWS] = LR;

    const size_t lds = (size_t)2 * LR * sizeof(knn_entry);
    for (int64_t g = 0; g < p.query_groups; ++g) {
        int64_t q0, q1;
        lmi_knn_plan::group_range(p, g, &q0, &q1);
        const int gq = (int)(q1 - q0), nct = cdiv(gq, 32), ct = nct >= 3 ? 4 : nct;
        const T* gxq = xq + (size_t)q0 * d;
        if (!on_device) {
            CHK(upload_pieces(d_xq, gxq, (size_t)gq * d * sizeof(T)));
            gxq = d_xq;
        }
        knn_pack_queries(gxq, l2 ? 1.0f : 0.0f, gq, d, nct, KG, d_qf);
        if (l2) knn_norms(gxq, gq, d, 0, d_qn);
        const long long nlist = (long long)gq * p.splits * LR;
        knn_fill_kernel<<<(int)std::min<long long>(cdiv(nlist, 256), prop.multiProcessorCount * 8), 256>>>(d_lists, nlist);
        HIPCHK(hipGetLastError());
        for (int64_t i = 0; i < p.pieces; ++i) {
            int64_t r0, r1;
            lmi_knn_plan::piece_range(p, i, &r0, &r1);
            const long long len = r1 - r0;
            const T* px = xb + (size_t)r0 * d;
            if (!on_device) {
                CHK(upload_pieces(d_xb, px, (size_t)len * d * sizeof(T)));
                px = d_xb;
            }
            if (l2) knn_norms(px, len, d, 1, d_xnh);
            CHK(knn_score_piece(vec_xb, ct, px, len, d, l2 ? d_xnh : nullptr, d_qf, KG, nct, gq, d_S, p.pitch));
            knn_select_kernel<<<dim3(gq, p.splits), 64, lds>>>(d_S, p.pitch, len, (unsigned)r0, k, LR, d_lists);
            HIPCHK(hipGetLastError());
        }
        float* oD = on_device ? D + (size_t)q0 * k : d_D;
        long long* oI = on_device ? reinterpret_cast<long long*>(I) + (size_t)q0 * k : d_I;
        knn_merge_kernel<<<gq, 64, lds>>>(d_lists, p.splits, LR, k, l2 ? d_qn : nullptr, oD, oI);
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
