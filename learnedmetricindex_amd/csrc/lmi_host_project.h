// lmi_host_project.h -- lmi_project and lmi_project_f16 (one body over the type of x): argument checks, the call's device buffers, and
// the schedule on the NULL stream of the device: pack the basis and the mean once, then per piece of x (upload,) project (, download).
// With host pointers x is never resident as a whole, as lmi_knn treats its base: the device memory of the call does not depend on n.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_host_knn.h"   // knn_vec_xb: the 16-byte rule of dense_load_b's two forms
#include "lmi_project.h"

namespace {

constexpr size_t PJ_PIECE_BYTES = (size_t)64 << 20;   // of x per uploaded piece, at most (host pointers)

template <class T, bool VEC>
int project_launch(int ct, dim3 grid, size_t lds, const T* x, long long n, int d, const float* ml, const float4* Bf, int KG, int nct,
                   int m, float* y, int vec_out) {
    if (ct == 1) project_kernel<T, 1, VEC><<<grid, 256, lds>>>(x, n, d, ml, Bf, KG, nct, m, y, vec_out);
    else if (ct == 2) project_kernel<T, 2, VEC><<<grid, 256, lds>>>(x, n, d, ml, Bf, KG, nct, m, y, vec_out);
    else project_kernel<T, 4, VEC><<<grid, 256, lds>>>(x, n, d, ml, Bf, KG, nct, m, y, vec_out);
    HIPCHK(hipGetLastError());
    return 0;
}

template <class T>
int project_run(const char* who, int device, const T* x, int64_t n, int d, const float* mean, const float* basis, int m, float* y,
                int on_device) {
    if (!x || !basis || !y) return fail("%s: x, basis and y must not be NULL", who);
    if (n < 1 || n >= (1ll << 31)) return fail("%s: n %lld outside [1, 2^31)", who, (long long)n);
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    if (m < 1 || m > LMI_PROJECT_MAX_M) return fail("%s: m %d outside [1,%d]", who, m, LMI_PROJECT_MAX_M);
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));

    const int nct = cdiv(m, 32), ct = nct >= 3 ? 4 : nct, KG = (int)(rup(d, 32) / 8);
    const int64_t piece_rows = on_device ? n : std::min<int64_t>(n, std::max<int64_t>(PJ_ROWS, (int64_t)(PJ_PIECE_BYTES / ((size_t)d * sizeof(T))) / PJ_ROWS * PJ_ROWS));
    CallScratch mem(who);
    T* d_x = nullptr;
    float *d_basis = nullptr, *d_mean = nullptr, *d_ml = nullptr, *d_y = nullptr;
    float4* d_bf = nullptr;
    CHK(mem.alloc(&d_bf, (size_t)nct * KG * 1024, "basis fragments"));
    CHK(mem.alloc(&d_ml, (size_t)KG * 32, "mean"));
    if (!on_device) {
        CHK(mem.alloc(&d_basis, (size_t)m * d * 4, "basis"));
        if (mean) CHK(mem.alloc(&d_mean, (size_t)d * 4, "mean"));
        CHK(mem.alloc(&d_x, (size_t)piece_rows * d * sizeof(T), "x piece"));
        CHK(mem.alloc(&d_y, (size_t)piece_rows * m * 4, "y piece"));
        CHK(upload_pieces(d_basis, basis, (size_t)m * d * 4));
        if (mean) CHK(upload_pieces(d_mean, mean, (size_t)d * 4));
    }
    dense_pack_kernel<<<cdiv((long long)nct * 32 * KG, 256), 256>>>(on_device ? basis : d_basis, nullptr, 0.0f, m, d, nct, KG, d_bf);
    project_mean_kernel<<<cdiv(KG * 8, 256), 256>>>(on_device ? mean : d_mean, d, KG * 8, d_ml);
    HIPCHK(hipGetLastError());
    for (int64_t r0 = 0; r0 < n; r0 += piece_rows) {
        const long long len = std::min<int64_t>(piece_rows, n - r0);
        const T* px = x + (size_t)r0 * d;
        float* py = y + (size_t)r0 * m;
        if (!on_device) {
            CHK(upload_pieces(d_x, px, (size_t)len * d * sizeof(T)));
            px = d_x;
            py = d_y;
        }
        // 16-byte stores of y: every row of the piece starts on a 16-byte boundary
        const int vec_out = m % 4 == 0 && (reinterpret_cast<uintptr_t>(py) & 15) == 0;
        const dim3 grid(cdiv(len, PJ_ROWS), cdiv(nct, ct));
        if (knn_vec_xb(px, d)) CHK((project_launch<T, true>(ct, grid, (size_t)KG * 32, px, len, d, d_ml, d_bf, KG, nct, m, py, vec_out)));
        else CHK((project_launch<T, false>(ct, grid, (size_t)KG * 32, px, len, d, d_ml, d_bf, KG, nct, m, py, vec_out)));
        if (!on_device) HIPCHK(hipMemcpy(y + (size_t)r0 * m, d_y, (size_t)len * m * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipStreamSynchronize(nullptr));
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_project(int device, const float* x, int64_t n, int d, const float* mean, const float* basis, int m, float* y,
                                   int on_device) {
    return project_run<float>("lmi_project", device, x, n, d, mean, basis, m, y, on_device);
}

extern "C" LMI_API int lmi_project_f16(int device, const uint16_t* x, int64_t n, int d, const float* mean, const float* basis, int m,
                                       float* y, int on_device) {
    return project_run<uint16_t>("lmi_project_f16", device, x, n, d, mean, basis, m, y, on_device);
}
