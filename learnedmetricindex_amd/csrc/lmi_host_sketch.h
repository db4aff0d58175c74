// lmi_host_sketch.h -- lmi_sketch and lmi_sketch_f16 (one body over the type of x, in the shape of project_run): argument checks, the
// call's device buffers, and the schedule on the NULL stream of the device: pack the basis, the mean and the thresholds once, then per
// piece of x (upload,) sketch (, download).  With host pointers x is never resident as a whole and the codes come back piece by piece:
// the device memory of the call does not depend on n.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_host_knn.h"       // knn_vec_xb: the 16-byte rule of dense_load_b's two forms
#include "lmi_host_project.h"   // PJ_PIECE_BYTES
#include "lmi_sketch.h"

// LMI_SKETCH_WALK=1 (a variant build, for measurement): one block per row block walks the column groups itself instead of the
// column group being the fast part of the block index.  Never changes a bit.
#ifndef LMI_SKETCH_WALK
#define LMI_SKETCH_WALK 0
#endif

namespace {

constexpr int SK_MAX_BITS = 4096;   // lmi_knn_hamming's widest code

template <class T, bool VEC>
int sketch_launch(int ct, unsigned grid, size_t lds, const T* x, long long n, int d, const float* ml, const float* tl, const float4* Bf,
                  int KG, int nct, int G, unsigned* codes, int vec_out) {
    if (ct == 1) sketch_kernel<T, 1, VEC><<<grid, 256, lds>>>(x, n, d, ml, tl, Bf, KG, nct, G, codes, vec_out);
    else if (ct == 2) sketch_kernel<T, 2, VEC><<<grid, 256, lds>>>(x, n, d, ml, tl, Bf, KG, nct, G, codes, vec_out);
    else sketch_kernel<T, 4, VEC><<<grid, 256, lds>>>(x, n, d, ml, tl, Bf, KG, nct, G, codes, vec_out);
    HIPCHK(hipGetLastError());
    return 0;
}

template <class T>
int sketch_run(const char* who, int device, const T* x, int64_t n, int d, const float* mean, const float* basis, int m,
               const float* thresh, uint8_t* codes, int on_device) {
    if (!x || !basis || !codes) return fail("%s: x, basis and codes must not be NULL", who);
    if (n < 1 || n >= (1ll << 31)) return fail("%s: n %lld outside [1, 2^31)", who, (long long)n);
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    if (m < 32 || m > SK_MAX_BITS || m % 32) return fail("%s: m %d is not a multiple of 32 in [32,%d]", who, m, SK_MAX_BITS);
    if (on_device && (reinterpret_cast<uintptr_t>(codes) & 3)) return fail("%s: codes on the device must be 4-byte aligned", who);
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));

    const int nct = m / 32, ct = nct >= 3 ? 4 : nct, KG = (int)(rup(d, 32) / 8), cb = m / 8;
    const int G = LMI_SKETCH_WALK ? 1 : cdiv(nct, ct);
    const int64_t piece_rows = on_device ? n : std::min<int64_t>(n, std::max<int64_t>(PJ_ROWS, (int64_t)(PJ_PIECE_BYTES / ((size_t)d * sizeof(T))) / PJ_ROWS * PJ_ROWS));
    CallScratch mem(who);
    T* d_x = nullptr;
    float *d_basis = nullptr, *d_mean = nullptr, *d_thresh = nullptr, *d_ml = nullptr, *d_tl = nullptr;
    uint8_t* d_codes = nullptr;
    float4* d_bf = nullptr;
    CHK(mem.alloc(&d_bf, (size_t)nct * KG * 1024, "basis fragments"));
    CHK(mem.alloc(&d_ml, (size_t)KG * 32, "mean"));
    CHK(mem.alloc(&d_tl, (size_t)m * 4, "thresholds"));
    if (!on_device) {
        CHK(mem.alloc(&d_basis, (size_t)m * d * 4, "basis"));
        if (mean) CHK(mem.alloc(&d_mean, (size_t)d * 4, "mean"));
        if (thresh) CHK(mem.alloc(&d_thresh, (size_t)m * 4, "thresholds"));
        CHK(mem.alloc(&d_x, (size_t)piece_rows * d * sizeof(T), "x piece"));
        CHK(mem.alloc(&d_codes, (size_t)piece_rows * cb, "codes piece"));
        CHK(upload_pieces(d_basis, basis, (size_t)m * d * 4));
        if (mean) CHK(upload_pieces(d_mean, mean, (size_t)d * 4));
        if (thresh) CHK(upload_pieces(d_thresh, thresh, (size_t)m * 4));
    }
    dense_pack_kernel<<<cdiv((long long)nct * 32 * KG, 256), 256>>>(on_device ? basis : d_basis, nullptr, 0.0f, m, d, nct, KG, d_bf);
    project_mean_kernel<<<cdiv(KG * 8, 256), 256>>>(on_device ? mean : d_mean, d, KG * 8, d_ml);
    sketch_thresh_kernel<<<cdiv(m, 256), 256>>>(on_device ? thresh : d_thresh, m, d_tl);
    HIPCHK(hipGetLastError());
    const size_t lds = (size_t)KG * 32 + (size_t)nct * 128;   // at most 16 KiB + 16 KiB
    for (int64_t r0 = 0; r0 < n; r0 += piece_rows) {
        const long long len = std::min<int64_t>(piece_rows, n - r0);
        const T* px = x + (size_t)r0 * d;
        uint8_t* pc = codes + (size_t)r0 * cb;
        if (!on_device) {
            CHK(upload_pieces(d_x, px, (size_t)len * d * sizeof(T)));
            px = d_x;
            pc = d_codes;
        }
        // one 16-byte store of a group's four words: every row of the piece starts on a 16-byte boundary
        const int vec_out = ct == 4 && m % 128 == 0 && (reinterpret_cast<uintptr_t>(pc) & 15) == 0;
        const unsigned grid = (unsigned)(cdiv(len, PJ_ROWS) * G);   // < 2^23 row blocks x at most 32 groups
        unsigned* pw = reinterpret_cast<unsigned*>(pc);
        if (knn_vec_xb(px, d)) CHK((sketch_launch<T, true>(ct, grid, lds, px, len, d, d_ml, d_tl, d_bf, KG, nct, G, pw, vec_out)));
        else CHK((sketch_launch<T, false>(ct, grid, lds, px, len, d, d_ml, d_tl, d_bf, KG, nct, G, pw, vec_out)));
        if (!on_device) HIPCHK(hipMemcpy(codes + (size_t)r0 * cb, d_codes, (size_t)len * cb, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipStreamSynchronize(nullptr));
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_sketch(int device, const float* x, int64_t n, int d, const float* mean, const float* basis, int m,
                                  const float* thresh, uint8_t* codes, int on_device) {
    return sketch_run<float>("lmi_sketch", device, x, n, d, mean, basis, m, thresh, codes, on_device);
}

extern "C" LMI_API int lmi_sketch_f16(int device, const uint16_t* x, int64_t n, int d, const float* mean, const float* basis, int m,
                                      const float* thresh, uint8_t* codes, int on_device) {
    return sketch_run<uint16_t>("lmi_sketch_f16", device, x, n, d, mean, basis, m, thresh, codes, on_device);
}
