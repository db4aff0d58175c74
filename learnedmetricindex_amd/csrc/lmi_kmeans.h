// lmi_kmeans.h -- device code of lmi_kmeans: Lloyd's k-means whose centroids and labels do not depend on the launch geometry
// (include/lmi_hip.h states the arithmetic).
//
// Assignment (km_assign_kernel): S^T = C . X^T by v_mfma_f32_32x32x2_f32, A = centroids in fragment order (lmi_kernels.h) with the
// extra column -|c|^2/2 at k = d (dense_norm_kernel, dense_pack_kernel: lmi_dense.h), B = rows of x straight from the caller's
// row-major array with a 1 at k = d and zeros behind it (dense_load_b).
// In the 32x32 accumulator a lane owns ONE row of x (lane & 31) and 16 centroids, so the running (best key, label) of a row is a
// register pair; the k order inside every accumulator is 0, 1, 2, ..: the key is the canonical chain of oracle.knn_l2.
// Update: rows are counting-sorted by label (km_hist_kernel, km_scan_kernel, km_scatter_kernel), blocks over (256 sorted rows x 256
// dimensions) sum q(x) = rint(x * 2^(36-e)) in int64 registers and add a run's sum to S[cluster][dim] with one 64-bit atomicAdd
// (km_accum_kernel); integer addition is associative, so S is the same for any order.  km_finish_kernel divides.
// lmi_kmeans_f16 (x as binary16 bit patterns, resident as halves): km_assign16_kernel and km_accum16_kernel read the halves and widen
// them exactly where they are loaded; everything that touches only labels, sums and centroids is shared with the float form.
#pragma once
#include "lmi_dense.h"

namespace lmi {

constexpr int KM_XB = 2;          // 32-row blocks of x per wave
constexpr int KM_ROWS = 4 * KM_XB * 32;   // rows of x per workgroup (4 waves)
constexpr int KM_ACC_ROWS = 256;  // sorted rows per km_accum_kernel block

// grid cdiv(n, KM_ROWS), block 256: wave w -> rows [(blockIdx.x * 4 + w) * 64, +64) as KM_XB column blocks; the centroid tiles
// (32 centroids) are visited in ascending order, CT at a time; every tile set streams the rows again (k <= 32 * CT: once).
// Cf [nct][KG][64], KG a multiple of 4.  labels: read (the previous pass) and written; *changed += rows whose label moved.
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void km_assign_kernel(const float* __restrict__ x, long long n, int d, const float4* __restrict__ Cf,
                                                        int KG, int nct, int k, int* __restrict__ labels,
                                                        unsigned long long* __restrict__ changed) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const long long row0 = ((long long)blockIdx.x * 4 + w) * (KM_XB * 32);
    if (row0 >= n) return;
    const float* xr[KM_XB];
#pragma unroll
    for (int b = 0; b < KM_XB; ++b) {
        const long long r = row0 + b * 32 + c;
        xr[b] = x + (size_t)(r < n ? r : n - 1) * d;   // clamp: duplicates are computed and discarded
    }
    float best[KM_XB];
    int lab[KM_XB];
#pragma unroll
    for (int b = 0; b < KM_XB; ++b) { best[b] = -INFINITY; lab[b] = 0; }
    const int nch = KG >> 2;
    for (int ct0 = 0; ct0 < nct; ct0 += CT) {
        f32x16 acc[CT][KM_XB];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int b = 0; b < KM_XB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][b][r] = 0.0f;
        const float4* ap[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) ap[t] = Cf + (size_t)(ct0 + t < nct ? ct0 + t : nct - 1) * KG * 64 + lane;
        float bv[KM_XB][16];
#pragma unroll
        for (int b = 0; b < KM_XB; ++b) dense_load_b<VEC>(xr[b], d, 0, h, 1.0f, bv[b]);
        float4 a[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) a[t] = ap[t][0];
        for (int ch = 0; ch < nch; ++ch) {
            // the next chunk's rows are requested before this chunk's MFMAs (the last chunk reads itself again)
            float bn[KM_XB][16];
            const int chn = ch + 1 < nch ? ch + 1 : ch;
#pragma unroll
            for (int b = 0; b < KM_XB; ++b) dense_load_b<VEC>(xr[b], d, chn, h, 1.0f, bn[b]);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int gn = ch * 4 + g + 1 < KG ? ch * 4 + g + 1 : ch * 4 + g;
                float4 an[CT];
#pragma unroll
                for (int t = 0; t < CT; ++t) an[t] = ap[t][(size_t)gn * 64];
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int t = 0; t < CT; ++t) {
                        const float av = s == 0 ? a[t].x : s == 1 ? a[t].y : s == 2 ? a[t].z : a[t].w;
#pragma unroll
                        for (int b = 0; b < KM_XB; ++b)
                            acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b][4 * g + s], acc[t][b], 0, 0, 0);
                    }
#pragma unroll
                for (int t = 0; t < CT; ++t) a[t] = an[t];
            }
#pragma unroll
            for (int b = 0; b < KM_XB; ++b)
#pragma unroll
                for (int s = 0; s < 16; ++s) bv[b][s] = bn[b][s];
        }
        // this lane's 16 centroids of every tile, ascending: a key replaces the best only when it is greater
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            if (ct0 + t >= nct) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (ct0 + t) * 32 + acc_row(r, h);
                if (j >= k) continue;
#pragma unroll
                for (int b = 0; b < KM_XB; ++b) {
                    const float v = acc[t][b][r];
                    if (j == 0 && v != v) best[b] = v;   // best starts as key 0: a NaN there is never replaced
                    else if (v > best[b]) { best[b] = v; lab[b] = j; }
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < KM_XB; ++b) {
        // the other half of the row's centroids sits in lane ^ 32: equal keys go to the lower centroid
        const float ov = __shfl_xor(best[b], 32);
        const int ol = __shfl_xor(lab[b], 32);
        if (ov > best[b] || (ov == best[b] && ol < lab[b])) { best[b] = ov; lab[b] = ol; }
        const long long r = row0 + b * 32 + c;
        bool moved = false;
        if (h == 0 && r < n) {
            moved = labels[r] != lab[b];
            labels[r] = lab[b];
        }
        const unsigned long long m = __ballot(moved);
        if (lane == 0 && m) atomicAdd(changed, (unsigned long long)__popcll(m));
    }
}

// km_assign_kernel on rows of halves (lmi_kmeans_f16): the same loop, B from the half form of dense_load_b -- every half is widened
// where it is loaded, so every key is the key of the widened row.  VEC by half_src_vec's rule (d % 8 == 0, x 16-byte aligned).
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void km_assign16_kernel(const unsigned short* __restrict__ x, long long n, int d,
                                                          const float4* __restrict__ Cf, int KG, int nct, int k, int* __restrict__ labels,
                                                          unsigned long long* __restrict__ changed) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const long long row0 = ((long long)blockIdx.x * 4 + w) * (KM_XB * 32);
    if (row0 >= n) return;
    const unsigned short* xr[KM_XB];
#pragma unroll
    for (int b = 0; b < KM_XB; ++b) {
        const long long r = row0 + b * 32 + c;
        xr[b] = x + (size_t)(r < n ? r : n - 1) * d;   // clamp: duplicates are computed and discarded
    }
    float best[KM_XB];
    int lab[KM_XB];
#pragma unroll
    for (int b = 0; b < KM_XB; ++b) { best[b] = -INFINITY; lab[b] = 0; }
    const int nch = KG >> 2;
    for (int ct0 = 0; ct0 < nct; ct0 += CT) {
        f32x16 acc[CT][KM_XB];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int b = 0; b < KM_XB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][b][r] = 0.0f;
        const float4* ap[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) ap[t] = Cf + (size_t)(ct0 + t < nct ? ct0 + t : nct - 1) * KG * 64 + lane;
        float bv[KM_XB][16];
#pragma unroll
        for (int b = 0; b < KM_XB; ++b) dense_load_b<VEC>(xr[b], d, 0, h, 1.0f, bv[b]);
        float4 a[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) a[t] = ap[t][0];
        for (int ch = 0; ch < nch; ++ch) {
            // the next chunk's rows are requested before this chunk's MFMAs (the last chunk reads itself again)
            float bn[KM_XB][16];
            const int chn = ch + 1 < nch ? ch + 1 : ch;
#pragma unroll
            for (int b = 0; b < KM_XB; ++b) dense_load_b<VEC>(xr[b], d, chn, h, 1.0f, bn[b]);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int gn = ch * 4 + g + 1 < KG ? ch * 4 + g + 1 : ch * 4 + g;
                float4 an[CT];
#pragma unroll
                for (int t = 0; t < CT; ++t) an[t] = ap[t][(size_t)gn * 64];
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int t = 0; t < CT; ++t) {
                        const float av = s == 0 ? a[t].x : s == 1 ? a[t].y : s == 2 ? a[t].z : a[t].w;
#pragma unroll
                        for (int b = 0; b < KM_XB; ++b)
                            acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b][4 * g + s], acc[t][b], 0, 0, 0);
                    }
#pragma unroll
                for (int t = 0; t < CT; ++t) a[t] = an[t];
            }
#pragma unroll
            for (int b = 0; b < KM_XB; ++b)
#pragma unroll
                for (int s = 0; s < 16; ++s) bv[b][s] = bn[b][s];
        }
        // this lane's 16 centroids of every tile, ascending: a key replaces the best only when it is greater
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            if (ct0 + t >= nct) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (ct0 + t) * 32 + acc_row(r, h);
                if (j >= k) continue;
#pragma unroll
                for (int b = 0; b < KM_XB; ++b) {
                    const float v = acc[t][b][r];
                    if (j == 0 && v != v) best[b] = v;   // best starts as key 0: a NaN there is never replaced
                    else if (v > best[b]) { best[b] = v; lab[b] = j; }
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < KM_XB; ++b) {
        // the other half of the row's centroids sits in lane ^ 32: equal keys go to the lower centroid
        const float ov = __shfl_xor(best[b], 32);
        const int ol = __shfl_xor(lab[b], 32);
        if (ov > best[b] || (ov == best[b] && ol < lab[b])) { best[b] = ov; lab[b] = ol; }
        const long long r = row0 + b * 32 + c;
        bool moved = false;
        if (h == 0 && r < n) {
            moved = labels[r] != lab[b];
            labels[r] = lab[b];
        }
        const unsigned long long m = __ballot(moved);
        if (lane == 0 && m) atomicAdd(changed, (unsigned long long)__popcll(m));
    }
}

// cnt[j] += rows with label j.  Dynamic LDS: k ints (a block's own histogram, flushed once).
__global__ void km_hist_kernel(const int* __restrict__ labels, long long n, int k, int* __restrict__ cnt) {
    extern __shared__ int km_lds[];
    for (int j = threadIdx.x; j < k; j += blockDim.x) km_lds[j] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) atomicAdd(&km_lds[labels[i]], 1);
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x)
        if (km_lds[j]) atomicAdd(&cnt[j], km_lds[j]);
}

// cursor[j] = rows of the clusters before j (k <= 16384: one thread)
__global__ void km_scan_kernel(const int* __restrict__ cnt, int k, int* __restrict__ cursor) {
    int s = 0;
    for (int j = 0; j < k; ++j) { cursor[j] = s; s += cnt[j]; }
}

// perm: the row numbers sorted by label (any order inside a cluster), slab: their labels.  A block counts its rows per cluster in LDS,
// reserves one range per cluster from `cursor` and places its rows inside.  Dynamic LDS: k ints.  blockDim.x * per rows per block.
__global__ void km_scatter_kernel(const int* __restrict__ labels, long long n, int k, int per, int* __restrict__ cursor,
                                  int* __restrict__ perm, int* __restrict__ slab) {
    extern __shared__ int km_lds[];
    for (int j = threadIdx.x; j < k; j += blockDim.x) km_lds[j] = 0;
    __syncthreads();
    const long long i0 = (long long)blockIdx.x * blockDim.x * per;
    for (int u = 0; u < per; ++u) {
        const long long i = i0 + (long long)u * blockDim.x + threadIdx.x;
        if (i < n) atomicAdd(&km_lds[labels[i]], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const int m = km_lds[j];
        km_lds[j] = m ? atomicAdd(&cursor[j], m) : 0;
    }
    __syncthreads();
    for (int u = 0; u < per; ++u) {
        const long long i = i0 + (long long)u * blockDim.x + threadIdx.x;
        if (i < n) {
            const int l = labels[i];
            const int p = atomicAdd(&km_lds[l], 1);
            perm[p] = (int)i;
            slab[p] = l;
        }
    }
}

// The update rule's two pieces of arithmetic, shared with the bucket cover (lmi_cover.h), whose centres are this rule's means:
// q(v) = rint(v * 2^(36-e)) -- the product is exact in binary64, rint rounds to nearest even -- and the mean of a cluster of m rows
// from its int64 sum S, c = (float)((double)S / (double)m * 2^(e-36)).
__device__ __forceinline__ long long km_quant(float v, double scale) { return (long long)__builtin_rint((double)v * scale); }
__device__ __forceinline__ float km_mean(long long S, long long m, double unscale) { return (float)((double)S / (double)m * unscale); }

// grid (cdiv(n, KM_ACC_ROWS), cdiv(d, 256)), block 256: thread -> dimension blockIdx.y * 256 + threadIdx.x, sorted rows
// [blockIdx.x * KM_ACC_ROWS, +KM_ACC_ROWS).  scale = 2^(36-e): the product is exact in binary64, rint rounds to nearest even.
__global__ __launch_bounds__(256) void km_accum_kernel(const float* __restrict__ x, int d, const int* __restrict__ perm,
                                                       const int* __restrict__ slab, long long n, double scale,
                                                       unsigned long long* __restrict__ S) {
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= d) return;
    const long long p0 = (long long)blockIdx.x * KM_ACC_ROWS;
    const long long p1 = p0 + KM_ACC_ROWS < n ? p0 + KM_ACC_ROWS : n;
    int cur = -1;
    long long acc = 0;
    for (long long p = p0; p < p1; p += 4) {
        float v[4];
        int l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long q = p + u < p1 ? p + u : p1 - 1;
            l[u] = slab[q];
            v[u] = x[(size_t)perm[q] * d + t];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p + u >= p1) break;
            if (l[u] != cur) {
                if (cur >= 0 && acc) atomicAdd(&S[(size_t)cur * d + t], (unsigned long long)acc);
                cur = l[u];
                acc = 0;
            }
            acc += km_quant(v[u], scale);
        }
    }
    if (cur >= 0 && acc) atomicAdd(&S[(size_t)cur * d + t], (unsigned long long)acc);
}

// km_accum_kernel on rows of halves: q = rint((double)(float)h * scale), the q of the widened value; element loads (2-byte aligned x)
__global__ __launch_bounds__(256) void km_accum16_kernel(const unsigned short* __restrict__ x, int d, const int* __restrict__ perm,
                                                         const int* __restrict__ slab, long long n, double scale,
                                                         unsigned long long* __restrict__ S) {
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= d) return;
    const long long p0 = (long long)blockIdx.x * KM_ACC_ROWS;
    const long long p1 = p0 + KM_ACC_ROWS < n ? p0 + KM_ACC_ROWS : n;
    int cur = -1;
    long long acc = 0;
    for (long long p = p0; p < p1; p += 4) {
        float v[4];
        int l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long q = p + u < p1 ? p + u : p1 - 1;
            l[u] = slab[q];
            v[u] = (float)__builtin_bit_cast(_Float16, x[(size_t)perm[q] * d + t]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p + u >= p1) break;
            if (l[u] != cur) {
                if (cur >= 0 && acc) atomicAdd(&S[(size_t)cur * d + t], (unsigned long long)acc);
                cur = l[u];
                acc = 0;
            }
            acc += km_quant(v[u], scale);
        }
    }
    if (cur >= 0 && acc) atomicAdd(&S[(size_t)cur * d + t], (unsigned long long)acc);
}

// c[j][t] = (float)((double)S / (double)cnt * 2^(e-36)) for cnt[j] > 0 (unscale = 2^(e-36)); an empty cluster keeps its centroid
__global__ void km_finish_kernel(const long long* __restrict__ S, const int* __restrict__ cnt, int k, int d, double unscale,
                                 float* __restrict__ c) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)k * d) return;
    const int m = cnt[idx / d];
    if (m > 0) c[idx] = km_mean(S[idx], m, unscale);
}

}  // namespace lmi
