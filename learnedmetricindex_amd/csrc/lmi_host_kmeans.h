// lmi_host_kmeans.h -- lmi_kmeans: argument checks, the call's device buffers, the upload in pieces, the pass schedule
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

}  // namespace

extern "C" LMI_API int lmi_kmeans(int device, const float* x, int64_t n, int d, int k, int niter, float* centroids, int32_t* labels,
                                  int64_t* counts, int64_t* changed, int on_device) {
    if (!x || !centroids || !labels) return fail("lmi_kmeans: x, centroids and labels must not be NULL");
    if (n < 1) return fail("lmi_kmeans: n %lld < 1", (long long)n);
    if (n > (1ll << 26)) return fail("lmi_kmeans: n %lld exceeds 2^26 (the bound of the int64 sums)", (long long)n);
    if (d < 1 || d > 4096) return fail("lmi_kmeans: d %d outside [1,4096]", d);
    if (k < 1 || k > 16384) return fail("lmi_kmeans: k %d outside [1,16384]", k);
    if (k > n) return fail("lmi_kmeans: k %d exceeds n %lld", k, (long long)n);
    if (niter < 0 || niter > 1000) return fail("lmi_kmeans: niter %d outside [0,1000]", niter);
    hipDeviceProp_t prop;
    CHK(open_device("lmi_kmeans", device, &prop));

    const int nct = cdiv(k, 32), KG = (int)(rup(d + 1, 32) / 8);
    const size_t xbytes = (size_t)n * d * 4, cbytes = (size_t)k * d * 4;
    CallScratch mem("lmi_kmeans");
    float *d_x = nullptr, *d_c = nullptr, *d_cnh = nullptr;
    float4* d_cf = nullptr;
    int *d_lab = nullptr, *d_cnt = nullptr, *d_cursor = nullptr, *d_perm = nullptr, *d_slab = nullptr;
    unsigned long long *d_S = nullptr, *d_changed = nullptr;
    unsigned* d_max = nullptr;
    if (on_device) {
        d_x = const_cast<float*>(x);
        d_c = centroids;
        d_lab = labels;
    } else {
        CHK(mem.alloc(&d_x, xbytes, "x"));
        CHK(mem.alloc(&d_c, cbytes, "centroids"));
        CHK(mem.alloc(&d_lab, (size_t)n * 4, "labels"));
        CHK(upload_pieces(d_x, x, xbytes));   // the rows go up once and stay for every pass
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
    dense_absmax_kernel<<<gs, 256>>>(d_x, (long long)n * d, d_max);
    dense_absmax_kernel<<<std::min(gs, cdiv((long long)k * d, 256)), 256>>>(d_c, (long long)k * d, d_max + 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h_max, d_max, 8, hipMemcpyDeviceToHost));
    if (h_max[0] >= 0x7f800000u) return fail("lmi_kmeans: x holds a value that is not finite (inf or NaN)");
    if (h_max[1] >= 0x7f800000u) return fail("lmi_kmeans: the initial centroids hold a value that is not finite (inf or NaN)");
    int e = 0;   // the smallest integer with max|x| < 2^e (0 for all-zero data)
    if (h_max[0]) {
        float m;
        memcpy(&m, &h_max[0], 4);
        (void)std::frexp(m, &e);
    }
    const double scale = std::ldexp(1.0, 36 - e), unscale = std::ldexp(1.0, e - 36);

    HIPCHK(hipMemsetAsync(d_lab, 0xff, (size_t)n * 4, nullptr));   // labels start at -1
    HIPCHK(hipMemsetAsync(d_changed, 0, (size_t)(niter + 1) * 8, nullptr));
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(d_x) & 15) == 0;
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
        km_accum_kernel<<<dim3(cdiv(n, KM_ACC_ROWS), cdiv(d, 256)), 256>>>(d_x, d, d_perm, d_slab, n, scale, d_S);
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
