// lmi_host_kmeans.h -- lmi_kmeans and lmi_kmeans_f16 (one body over the type of x): argument checks, the call's device buffers, the upload in pieces, the pass schedule
// (assign, count `changed`, sort rows by label, integer sums, divide) on the NULL stream of the device.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_kmeans.h"
#include <cmath>

namespace {

template <bool VEC>
int km_assign_launch(int ct, int grid, const float* x, long long n, int d, const float4* Cf, int KG, int nct, int k, int* labels,
                     unsigned long long* changed) {
    if (ct == 1) km_assign_kernel<1, VEC><<<grid, 256>>>(x, n, d, Cf, KG, nct, k, labels, changed);
    else if (ct == 2) km_assign_kernel<2, VEC><<<grid, 256>>>(x, n, d, Cf, KG, nct, k, labels, changed);
    else km_assign_kernel<4, VEC><<<grid, 256>>>(x, n, d, Cf, KG, nct, k, labels, changed);
    HIPCHK(hipGetLastError());
    return 0;
}

template <bool VEC>
int km_assign_launch(int ct, int grid, const uint16_t* x, long long n, int d, const float4* Cf, int KG, int nct, int k, int* labels,
                     unsigned long long* changed) {
    if (ct == 1) km_assign16_kernel<1, VEC><<<grid, 256>>>(x, n, d, Cf, KG, nct, k, labels, changed);
    else if (ct == 2) km_assign16_kernel<2, VEC><<<grid, 256>>>(x, n, d, Cf, KG, nct, k, labels, changed);
    else km_assign16_kernel<4, VEC><<<grid, 256>>>(x, n, d, Cf, KG, nct, k, labels, changed);
    HIPCHK(hipGetLastError());
    return 0;
}

// What differs between the source types beside the assign kernels: the pass that takes max|x| (out: the bit pattern of the maximal
// |value| in the source's own format), what that pattern says, the sums, and whether x is read with 16-byte loads -- binary32:
// d % 4 == 0 and an aligned base; halves: half_src_vec (d % 8 == 0).
void km_absmax(const float* x, long long total, int grid, unsigned* out) { dense_absmax_kernel<<<grid, 256>>>(x, total, out); }
void km_absmax(const uint16_t* x, long long total, int grid, unsigned* out) { dense_absmax16_kernel<<<grid, 256>>>(x, total, out); }
bool km_finite(const float*, unsigned bits) { return bits < 0x7f800000u; }
bool km_finite(const uint16_t*, unsigned bits) { return bits < 0x7c00u; }
float km_max_value(const float*, unsigned bits) {
    float m;
    memcpy(&m, &bits, 4);
    return m;
}
float km_max_value(const uint16_t*, unsigned bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }   // exact
bool km_vec(const float* x, int d) { return d % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0; }
bool km_vec(const uint16_t* x, int d) { return half_src_vec(x, d); }
void km_accum(dim3 grid, const float* x, int d, const int* perm, const int* slab, long long n, double scale, unsigned long long* S) {
    km_accum_kernel<<<grid, 256>>>(x, d, perm, slab, n, scale, S);
}
void km_accum(dim3 grid, const uint16_t* x, int d, const int* perm, const int* slab, long long n, double scale, unsigned long long* S) {
    km_accum16_kernel<<<grid, 256>>>(x, d, perm, slab, n, scale, S);
}

template <class T>
int kmeans_run(const char* who, int device, const T* x, int64_t n, int d, int k, int niter, float* centroids, int32_t* labels,
               int64_t* counts, int64_t* changed, int on_device);

}  // namespace

extern "C" LMI_API int lmi_kmeans(int device, const float* x, int64_t n, int d, int k, int niter, float* centroids, int32_t* labels,
                                  int64_t* counts, int64_t* changed, int on_device) {
    return kmeans_run<float>("lmi_kmeans", device, x, n, d, k, niter, centroids, labels, counts, changed, on_device);
}

extern "C" LMI_API int lmi_kmeans_f16(int device, const uint16_t* x, int64_t n, int d, int k, int niter, float* centroids,
                                      int32_t* labels, int64_t* counts, int64_t* changed, int on_device) {
    return kmeans_run<uint16_t>("lmi_kmeans_f16", device, x, n, d, k, niter, centroids, labels, counts, changed, on_device);
}

namespace {

template <class T>
int kmeans_run(const char* who, int device, const T* x, int64_t n, int d, int k, int niter, float* centroids, int32_t* labels,
               int64_t* counts, int64_t* changed, int on_device) {
    if (!x || !centroids || !labels) return fail("%s: x, centroids and labels must not be NULL", who);
    if (n < 1) return fail("%s: n %lld < 1", who, (long long)n);
    if (n > (1ll << 26)) return fail("%s: n %lld exceeds 2^26 (the bound of the int64 sums)", who, (long long)n);
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    if (k < 1 || k > 16384) return fail("%s: k %d outside [1,16384]", who, k);
    if (k > n) return fail("%s: k %d exceeds n %lld", who, k, (long long)n);
    if (niter < 0 || niter > 1000) return fail("%s: niter %d outside [0,1000]", who, niter);
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));

    const int nct = cdiv(k, 32), KG = (int)(rup(d + 1, 32) / 8);
    const size_t xbytes = (size_t)n * d * sizeof(T), cbytes = (size_t)k * d * 4;
    CallScratch mem(who);
    T* d_x = nullptr;
    float *d_c = nullptr, *d_cnh = nullptr;
    float4* d_cf = nullptr;
    int *d_lab = nullptr, *d_cnt = nullptr, *d_cursor = nullptr, *d_perm = nullptr, *d_slab = nullptr;
    unsigned long long *d_S = nullptr, *d_changed = nullptr;
    unsigned* d_max = nullptr;
    if (on_device) {
        d_x = const_cast<T*>(x);
        d_c = centroids;
        d_lab = labels;
    } else {
        CHK(mem.alloc(&d_x, xbytes, "x"));
        CHK(mem.alloc(&d_c, cbytes, "centroids"));
        CHK(mem.alloc(&d_lab, (size_t)n * 4, "labels"));
        CHK(upload_pieces(d_x, x, xbytes));   // the rows go up once, in the type they came in, and stay for every pass
        HIPCHK(hipMemcpyAsync(d_c, centroids, cbytes, hipMemcpyHostToDevice, nullptr));
    }
    CHK(mem.alloc(&d_cf, (size_t)nct * KG * 1024, "centroid fragments"));
    CHK(mem.alloc(&d_cnh, (size_t)k * 4, "centroid norms"));
    CHK(mem.alloc(&d_cnt, (size_t)k * 4, "counts"));
    CHK(mem.alloc(&d_cursor, (size_t)k * 4, "cursors"));
    CHK(mem.alloc(&d_changed, (size_t)(niter + 1) * 8, "changed"));
    CHK(mem.alloc(&d_max, 8, "max"));
    if (niter > 0) {
        CHK(mem.alloc(&d_perm, (size_t)n * 4, "sorted rows"));
        CHK(mem.alloc(&d_slab, (size_t)n * 4, "sorted labels"));
        CHK(mem.alloc(&d_S, (size_t)k * d * 8, "sums"));
    }

    // max|x| and the non-finite check of x and of the initial centroids, before anything of the caller's is written
    unsigned h_max[2] = {0, 0};
    HIPCHK(hipMemsetAsync(d_max, 0, 8, nullptr));
    const int gs = (int)std::min<long long>(prop.multiProcessorCount * 8, cdiv((long long)n * d, 256));
    km_absmax(d_x, (long long)n * d, gs, d_max);
    dense_absmax_kernel<<<std::min(gs, cdiv((long long)k * d, 256)), 256>>>(d_c, (long long)k * d, d_max + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h_max, d_max, 8, hipMemcpyDeviceToHost));
    if (!km_finite(d_x, h_max[0])) return fail("%s: x holds a value that is not finite (inf or NaN)", who);
    if (h_max[1] >= 0x7f800000u) return fail("%s: the initial centroids hold a value that is not finite (inf or NaN)", who);
    int e = 0;   // the smallest integer with max|x| < 2^e (0 for all-zero data)
    if (h_max[0]) (void)std::frexp(km_max_value(d_x, h_max[0]), &e);
    const double scale = std::ldexp(1.0, 36 - e), unscale = std::ldexp(1.0, e - 36);

    HIPCHK(hipMemsetAsync(d_lab, 0xff, (size_t)n * 4, nullptr));   // labels start at -1
    HIPCHK(hipMemsetAsync(d_changed, 0, (size_t)(niter + 1) * 8, nullptr));
    const bool vec = km_vec(d_x, d);
    const int ct = nct >= 3 ? 4 : nct, grid = cdiv(n, KM_ROWS);
    const int hist_grid = (int)std::min<long long>(prop.multiProcessorCount * 4, cdiv(n, 256));
    const int sc_per = 16, sc_grid = cdiv(n, 256 * sc_per);
    std::vector<unsigned long long> h_changed((size_t)niter + 1, 0);
    auto histogram = [&]() -> int {
        HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)k * 4, nullptr));
        km_hist_kernel<<<hist_grid, 256, (size_t)k * 4>>>(d_lab, n, k, d_cnt);
        HIPCHK(hipGetLastError());
        return 0;
    };
    for (int it = 0; it <= niter; ++it) {
        dense_norm_kernel<<<cdiv(k, 64), 64>>>(d_c, k, d, 1, d_cnh);
        dense_pack_kernel<<<cdiv((long long)nct * 32 * KG, 256), 256>>>(d_c, d_cnh, 0.0f, k, d, nct, KG, d_cf);
        HIPCHK(hipGetLastError());
        if (vec) CHK(km_assign_launch<true>(ct, grid, d_x, n, d, d_cf, KG, nct, k, d_lab, d_changed + it));
        else CHK(km_assign_launch<false>(ct, grid, d_x, n, d, d_cf, KG, nct, k, d_lab, d_changed + it));
        if (it == niter) break;
        HIPCHK(hipMemcpy(&h_changed[it], d_changed + it, 8, hipMemcpyDeviceToHost));
        if (it >= 1 && h_changed[it] == 0) break;   // a fixed point: every later pass would repeat this one
        CHK(histogram());
        km_scan_kernel<<<1, 1>>>(d_cnt, k, d_cursor);
        km_scatter_kernel<<<sc_grid, 256, (size_t)k * 4>>>(d_lab, n, k, sc_per, d_cursor, d_perm, d_slab);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(d_S, 0, (size_t)k * d * 8, nullptr));
        km_accum(dim3(cdiv(n, KM_ACC_ROWS), cdiv(d, 256)), d_x, d, d_perm, d_slab, n, scale, d_S);
        km_finish_kernel<<<cdiv((long long)k * d, 256), 256>>>(reinterpret_cast<const long long*>(d_S), d_cnt, k, d, unscale, d_c);
        HIPCHK(hipGetLastError());
    }
    CHK(histogram());
    std::vector<int> h_cnt((size_t)k);
    HIPCHK(hipMemcpy(h_changed.data(), d_changed, h_changed.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_cnt.data(), d_cnt, (size_t)k * 4, hipMemcpyDeviceToHost));
    if (!on_device) {
        HIPCHK(hipMemcpy(centroids, d_c, cbytes, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(labels, d_lab, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipStreamSynchronize(nullptr));
    if (counts) for (int j = 0; j < k; ++j) counts[j] = h_cnt[(size_t)j];
    if (changed) for (int it = 0; it <= niter; ++it) changed[it] = (int64_t)h_changed[(size_t)it];
    return 0;
}

}  // namespace
