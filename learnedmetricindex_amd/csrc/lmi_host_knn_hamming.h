// lmi_host_knn_hamming.h -- lmi_knn_hamming: argument checks and the schedule on the NULL stream of the device.  knn_hamming_run
// mirrors knn_run (lmi_host_knn.h): the same plan (lmi_knn_plan.h, made for rows of W = code_bytes / 4 four-byte words), the same call
// scratch, upload in pieces and loop over groups and pieces; knn_fill_kernel and knn_select_kernel are launched as they are.  What is
// not there: the query pack, the norms and their buffers -- the score kernel reads the queries as they lie, uploaded once per group.
// The forced geometry and the last-plan words are lmi_knn's (g_knn_forced, g_knn_last).
#pragma once
#include "lmi_host_knn.h"
#include "lmi_knn_hamming.h"

namespace {

// the distances of one (group, piece) into the slab: every row tile against shares of the group's query tiles
int knn_hamming_score_piece(bool vec_xb, int cus, const unsigned* px, long long len, int W, const unsigned* q, int gq, float* S,
                            long long pitch) {
    // eight blocks per compute unit where the row tiles alone do not give them; a block keeps at least four query tiles (or all)
    // against its row tile, which amortises the tile's load
    const int nrt = cdiv(len, HAM_ROWS), nct = cdiv(gq, HAM_TQ);
    const int tps = std::max(std::min(nct, 4), cdiv(nct, std::max(1, cdiv((long long)cus * 8, nrt))));
    const dim3 grid(nrt, cdiv(nct, tps));
    const size_t lds = ham_lds_bytes(W);
    if (vec_xb) hamming_score_kernel<true><<<grid, 256, lds>>>(px, len, W, q, gq, nct, tps, S, pitch);
    else hamming_score_kernel<false><<<grid, 256, lds>>>(px, len, W, q, gq, nct, tps, S, pitch);
    HIPCHK(hipGetLastError());
    return 0;
}

int knn_hamming_run(int device, const uint8_t* xq8, int64_t nq, const uint8_t* xb8, int64_t nb, int code_bytes, int k, int32_t* D,
                    int64_t* I, int on_device) {
    const char* who = "lmi_knn_hamming";
    for (int64_t& w : g_knn_last) w = 0;
    if (code_bytes < 4 || code_bytes > 4 * HAM_MAX_WORDS || code_bytes % 4)
        return fail("%s: code_bytes %d is not a multiple of 4 in [4,%d]", who, code_bytes, 4 * HAM_MAX_WORDS);
    if (k < 1 || k > LMI_KNN_MAX_K) return fail("%s: k %d outside [1,%d]", who, k, LMI_KNN_MAX_K);
    if (nq < 0 || nq >= (1ll << 31)) return fail("%s: nq %lld outside [0, 2^31)", who, (long long)nq);
    if (nb < 0 || nb >= (1ll << 31)) return fail("%s: nb %lld outside [0, 2^31)", who, (long long)nb);
    if (nq > 0 && (!xq8 || !D || !I)) return fail("%s: xq, D and I must not be NULL", who);
    if (nq > 0 && nb > 0 && !xb8) return fail("%s: xb must not be NULL", who);
    if ((reinterpret_cast<uintptr_t>(xq8) | reinterpret_cast<uintptr_t>(xb8)) & 3) return fail("%s: xq and xb must be 4-byte aligned", who);
    if (nq == 0) return 0;
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));

    const int W = code_bytes / 4;
    const unsigned* xq = reinterpret_cast<const unsigned*>(xq8);
    const unsigned* xb = reinterpret_cast<const unsigned*>(xb8);
    // a row of W four-byte words; the plan's fragment and norm bytes are not allocated here
    const lmi_knn_plan::Plan p = lmi_knn_plan::make_plan(nq, nb, W, k, false, on_device != 0, (int64_t)free_b, prop.multiProcessorCount,
                                                         g_knn_forced);
    const int LR = p.list_rows;
    CallScratch mem(who);
    float* d_S = nullptr;
    unsigned *d_xq = nullptr, *d_xb = nullptr;
    knn_entry* d_lists = nullptr;
    int* d_D = nullptr;
    long long* d_I = nullptr;
    CHK(mem.alloc(&d_S, p.slab_bytes, "score slab"));
    CHK(mem.alloc(&d_lists, p.list_bytes, "lists"));
    if (!on_device) {
        CHK(mem.alloc(&d_xq, p.xq_bytes, "queries"));
        CHK(mem.alloc(&d_xb, p.xb_bytes, "base piece"));
        CHK(mem.alloc(&d_D, p.d_bytes, "D"));
        CHK(mem.alloc(&d_I, p.i_bytes, "I"));
    }
    // 16-byte loads of the row tiles: every row and every piece's first row stay aligned when the scanned base is
    const bool vec_xb = W % 4 == 0 && (reinterpret_cast<uintptr_t>(on_device ? xb : d_xb) & 15) == 0;
    g_knn_last[LMI_KNN_PLAN_PIECES] = p.pieces;
    g_knn_last[LMI_KNN_PLAN_PIECE_ROWS] = p.piece_rows;
    g_knn_last[LMI_KNN_PLAN_SPLITS] = p.splits;
    g_knn_last[LMI_KNN_PLAN_QUERY_GROUPS] = p.query_groups;
    g_knn_last[LMI_KNN_PLAN_QUERY_ROWS] = p.query_rows;
    g_knn_last[LMI_KNN_PLAN_VEC_XQ] = 0;   // the query words are scalar loads
    g_knn_last[LMI_KNN_PLAN_VEC_XB] = vec_xb;
    g_knn_last[LMI_KNN_PLAN_WORKSPACE_BYTES] = mem.total;
    g_knn_last[LMI_KNN_PLAN_LIST_ROWS] = LR;

    // the row tile of the widest codes is above the 64 KiB a kernel gets unasked
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&hamming_score_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)ham_lds_bytes(HAM_MAX_WORDS)));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&hamming_score_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)ham_lds_bytes(HAM_MAX_WORDS)));
    const size_t lds = (size_t)2 * LR * sizeof(knn_entry);
    for (int64_t g = 0; g < p.query_groups; ++g) {
        int64_t q0, q1;
        lmi_knn_plan::group_range(p, g, &q0, &q1);
        const int gq = (int)(q1 - q0);
        const unsigned* gxq = xq + (size_t)q0 * W;
        if (!on_device) {
            CHK(upload_pieces(d_xq, gxq, (size_t)gq * code_bytes));
            gxq = d_xq;
        }
        const long long nlist = (long long)gq * p.splits * LR;
        knn_fill_kernel<<<(int)std::min<long long>(cdiv(nlist, 256), prop.multiProcessorCount * 8), 256>>>(d_lists, nlist);
        HIPCHK(hipGetLastError());
        for (int64_t i = 0; i < p.pieces; ++i) {
            int64_t r0, r1;
            lmi_knn_plan::piece_range(p, i, &r0, &r1);
            const long long len = r1 - r0;
            const unsigned* px = xb + (size_t)r0 * W;
            if (!on_device) {
                CHK(upload_pieces(d_xb, px, (size_t)len * code_bytes));
                px = d_xb;
            }
            CHK(knn_hamming_score_piece(vec_xb, prop.multiProcessorCount, px, len, W, gxq, gq, d_S, p.pitch));
            knn_select_kernel<<<dim3(gq, p.splits), 64, lds>>>(d_S, p.pitch, len, (unsigned)r0, k, LR, d_lists);
            HIPCHK(hipGetLastError());
        }
        int* oD = on_device ? D + (size_t)q0 * k : d_D;
        long long* oI = on_device ? reinterpret_cast<long long*>(I) + (size_t)q0 * k : d_I;
        knn_merge_hamming_kernel<<<gq, 64, lds>>>(d_lists, p.splits, LR, k, oD, oI);
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

extern "C" LMI_API int lmi_knn_hamming(int device, const uint8_t* xq, int64_t nq, const uint8_t* xb, int64_t nb, int code_bytes, int k,
                                       int32_t* D, int64_t* I, int on_device) {
    return knn_hamming_run(device, xq, nq, xb, nb, code_bytes, k, D, I, on_device);
}
