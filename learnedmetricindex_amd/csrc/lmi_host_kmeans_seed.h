// lmi_host_kmeans_seed.h -- lmi_kmeans_seed and lmi_kmeans_seed_f16 (one body over the type of x): argument checks, the call's
// device buffers, the upload in pieces (lmi_kmeans's frame), the exponent E, and the round schedule (sample, gather, norm, pack,
// round, update, scan) on the NULL stream of the device.  Nothing comes back to the host between rounds.
#pragma once
#include "lmi_host.h"
#include "lmi_host_call.h"
#include "lmi_host_kmeans.h"   // km_absmax, km_finite, km_max_value, km_vec: what differs between the source types
#include "lmi_kmeans_seed.h"
#include <cmath>

namespace {

void kpp_norm(const float* x, long long n, int d, float* out) { dense_norm_kernel<<<cdiv(n, 64), 64>>>(x, n, d, 0, out); }
void kpp_norm(const uint16_t* x, long long n, int d, float* out) { dense_norm16_kernel<<<cdiv(n, 64), 64>>>(x, n, d, 0, out); }

template <class T>
int kmeans_seed_run(const char* who, int device, const T* x, int64_t n, int d, int k, int n_trials, uint64_t seed, float* centroids,
                    int64_t* rows, int64_t* potential, int on_device) {
    if (!x || !centroids) return fail("%s: x and centroids must not be NULL", who);
    if (n < 1) return fail("%s: n %lld < 1", who, (long long)n);
    if (n > (1ll << 26)) return fail("%s: n %lld exceeds 2^26 (the bound of the int64 sums)", who, (long long)n);
    if (d < 1 || d > 4096) return fail("%s: d %d outside [1,4096]", who, d);
    if (k < 1 || k > 16384) return fail("%s: k %d outside [1,16384]", who, k);
    if (k > n) return fail("%s: k %d exceeds n %lld", who, k, (long long)n);
    if (n_trials < 0 || n_trials > KPP_MAX_TRIALS) return fail("%s: n_trials %d outside [0,%d]", who, n_trials, KPP_MAX_TRIALS);
    const int L = n_trials ? n_trials : 2 + (int)std::floor(std::log((double)k));   // k <= 16384: at most 11
    hipDeviceProp_t prop;
    CHK(open_device(who, device, &prop));

    const int KG = (int)(rup(d + 1, 32) / 8), nb = (int)cdiv(n, KPP_BLOCK);
    const size_t xbytes = (size_t)n * d * sizeof(T), cbytes = (size_t)k * d * 4;
    CallScratch mem(who);
    T* d_x = nullptr;
    float *d_c = nullptr, *d_xn = nullptr, *d_slab = nullptr, *d_cand_rows = nullptr, *d_cnh = nullptr;
    float4* d_cf = nullptr;
    unsigned long long *d_W = nullptr, *d_bsum = nullptr, *d_prefix = nullptr, *d_pot = nullptr, *d_potential = nullptr;
    long long *d_cand = nullptr, *d_rows = nullptr;
    unsigned* d_max = nullptr;
    if (on_device) {
        d_x = const_cast<T*>(x);
        d_c = centroids;
    } else {
        CHK(mem.alloc(&d_x, xbytes, "x"));
        CHK(mem.alloc(&d_c, cbytes, "centroids"));
        CHK(upload_pieces(d_x, x, xbytes));   // the rows go up once, in the type they came in, and stay for every round
    }
    CHK(mem.alloc(&d_max, 4, "max"));
    CHK(mem.alloc(&d_xn, (size_t)n * 4, "row norms"));
    CHK(mem.alloc(&d_W, (size_t)n * 8, "weights"));
    CHK(mem.alloc(&d_slab, (size_t)n * L * 4, "distance slab"));
    CHK(mem.alloc(&d_bsum, (size_t)nb * 8, "block sums"));
    CHK(mem.alloc(&d_prefix, (size_t)(nb + 1) * 8, "block prefix"));
    CHK(mem.alloc(&d_pot, (size_t)k * KPP_MAX_TRIALS * 8, "trial potentials"));
    CHK(mem.alloc(&d_potential, (size_t)k * 8, "potentials"));
    CHK(mem.alloc(&d_rows, (size_t)k * 8, "rows"));
    CHK(mem.alloc(&d_cand, (size_t)KPP_MAX_TRIALS * 8, "candidates"));
    CHK(mem.alloc(&d_cand_rows, (size_t)KPP_MAX_TRIALS * d * 4, "candidate rows"));
    CHK(mem.alloc(&d_cnh, (size_t)KPP_MAX_TRIALS * 4, "candidate norms"));
    CHK(mem.alloc(&d_cf, (size_t)KG * 1024, "candidate fragments"));

    // max|x| and the non-finite check, before anything of the caller's is written
    unsigned h_max = 0;
    HIPCHK(hipMemsetAsync(d_max, 0, 4, nullptr));
    const int gs = (int)std::min<long long>(prop.multiProcessorCount * 8, cdiv((long long)n * d, 256));
    km_absmax(d_x, (long long)n * d, gs, d_max);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&h_max, d_max, 4, hipMemcpyDeviceToHost));
    if (!km_finite(d_x, h_max)) return fail("%s: x holds a value that is not finite (inf or NaN)", who);
    int e = 0, lg = 0;   // the smallest integer with max|x| < 2^e (0 for all-zero data); ceil(log2 d)
    if (h_max) (void)std::frexp(km_max_value(d_x, h_max), &e);
    while ((1 << lg) < d) ++lg;
    const int E = 2 * e + 3 + lg;
    if (E > 127)
        return fail("%s: E = 2e + 3 + ceil(log2 d) = %d exceeds 127 (max|x| < 2^%d, d %d): a distance could overflow binary32", who, E, e, d);
    const double scale = std::ldexp(1.0, 36 - E);

    kpp_norm(d_x, n, d, d_xn);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(d_W, 0xff, (size_t)n * 8, nullptr));           // round 0 takes every minimum against all ones
    HIPCHK(hipMemsetAsync(d_prefix, 0, (size_t)(nb + 1) * 8, nullptr));   // and draws its row with T = 0
    HIPCHK(hipMemsetAsync(d_pot, 0, (size_t)k * KPP_MAX_TRIALS * 8, nullptr));
    HIPCHK(hipMemsetAsync(d_cand, 0, (size_t)KPP_MAX_TRIALS * 8, nullptr));
    const bool vec = km_vec(d_x, d);
    // two blocks per CU (two waves per SIMD), each wave walking its row blocks grid-stride
    const int grid = (int)std::min<long long>((long long)prop.multiProcessorCount * 2, cdiv(n, 4 * KPP_XB * 32));
    for (int t = 0; t < k; ++t) {
        const int Lt = t ? L : 1;
        unsigned long long* pot = d_pot + (size_t)t * KPP_MAX_TRIALS;
        kpp_sample_kernel<<<Lt, 256>>>(d_W, n, d_prefix, nb, (unsigned long long)seed, t, d_cand);
        kpp_gather_kernel<T><<<cdiv((long long)Lt * d, 256), 256>>>(d_x, d_cand, Lt, d, d_cand_rows);
        dense_norm_kernel<<<1, 64>>>(d_cand_rows, Lt, d, 1, d_cnh);
        dense_pack_kernel<<<cdiv((long long)32 * KG, 256), 256>>>(d_cand_rows, d_cnh, 0.0f, Lt, d, 1, KG, d_cf);
        if (vec) kpp_round_kernel<true, T><<<grid, 256>>>(d_x, n, d, d_cf, KG, Lt, d_xn, d_W, scale, d_slab, pot);
        else kpp_round_kernel<false, T><<<grid, 256>>>(d_x, n, d, d_cf, KG, Lt, d_xn, d_W, scale, d_slab, pot);
        kpp_update_kernel<<<nb, 256>>>(d_slab, n, Lt, pot, d_cand, scale, d_W, d_bsum, d_rows + t, d_potential + t);
        kpp_scan_kernel<<<1, 1024>>>(d_bsum, nb, d_prefix);
        HIPCHK(hipGetLastError());
    }
    kpp_gather_kernel<T><<<cdiv((long long)k * d, 256), 256>>>(d_x, d_rows, k, d, d_c);
    HIPCHK(hipGetLastError());
    std::vector<long long> h_rows((size_t)k);
    std::vector<unsigned long long> h_pot((size_t)k);
    HIPCHK(hipMemcpy(h_rows.data(), d_rows, (size_t)k * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_pot.data(), d_potential, (size_t)k * 8, hipMemcpyDeviceToHost));
    if (!on_device) HIPCHK(hipMemcpy(centroids, d_c, cbytes, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(nullptr));
    if (rows) for (int t = 0; t < k; ++t) rows[t] = (int64_t)h_rows[(size_t)t];
    if (potential) for (int t = 0; t < k; ++t) potential[t] = (int64_t)h_pot[(size_t)t];
    return 0;
}

}  // namespace

extern "C" LMI_API int lmi_kmeans_seed(int device, const float* x, int64_t n, int d, int k, int n_trials, uint64_t seed,
                                       float* centroids, int64_t* rows, int64_t* potential, int on_device) {
    return kmeans_seed_run<float>("lmi_kmeans_seed", device, x, n, d, k, n_trials, seed, centroids, rows, potential, on_device);
}

extern "C" LMI_API int lmi_kmeans_seed_f16(int device, const uint16_t* x, int64_t n, int d, int k, int n_trials, uint64_t seed,
                                           float* centroids, int64_t* rows, int64_t* potential, int on_device) {
    return kmeans_seed_run<uint16_t>("lmi_kmeans_seed_f16", device, x, n, d, k, n_trials, seed, centroids, rows, potential, on_device);
}
