// lmi_knn.h -- device code of lmi_knn: exact brute-force k-NN for k up to 1024 whose result does not depend on the launch geometry
// (include/lmi_hip.h states the arithmetic and the order).
//
// Scores (knn_score_kernel): S = Q . X^T by v_mfma_f32_32x32x2_f32, km_assign_kernel's loop (the two are kept equal: lmi_dense.h) --
// A = a group's queries in fragment order (dense_pack_kernel; L2: a 1 at link d), B = rows of the base straight from the row-major
// piece (dense_load_b; L2: -|x|^2/2 at link d, from dense_norm_kernel), the link order inside every accumulator 0, 1, 2, ..: a score is
// the canonical chain of oracle.knn_ip / knn_l2.
// A block writes its 256 rows x 32 CT queries to the slab S[query][row of the piece].
// knn_score16_kernel is the same kernel for a piece of halves (lmi_knn_f16, lmi_knn_range_f16); everything behind
// the slab is shared by both.
// Selection (knn_select_kernel): one wave per (query, split) reads its stretch of the query's slab row, keeps what beats the k-th best
// so far -- compared as the pair (score, row) -- in an LDS buffer by ballot compaction, and when the buffer is full sorts it and merges
// it into the sorted list (bitonic, in LDS), which raises the threshold.  The list lives in global memory between launches: the next
// piece continues it.  knn_merge_kernel merges a query's split lists and writes the caller's rows.
#pragma once
#include "lmi_dense.h"
#include <cfloat>

namespace lmi {

constexpr int KNN_XB = 2;                      // 32-row blocks of the base per wave
constexpr int KNN_ROWS = 4 * KNN_XB * 32;      // rows of the base per workgroup (4 waves)

// A list entry: the score's bits in the high word, the row in the low one.  An empty slot is (-FLT_MAX, 0xffffffff): every admissible
// score is greater, so it sorts behind all of them.
typedef unsigned long long knn_entry;
constexpr knn_entry KNN_EMPTY = ((knn_entry)0xff7fffffu << 32) | 0xffffffffu;
__device__ __forceinline__ knn_entry knn_make(float s, unsigned row) { return ((knn_entry)__float_as_uint(s) << 32) | row; }
__device__ __forceinline__ float knn_score(knn_entry e) { return __uint_as_float((unsigned)(e >> 32)); }
__device__ __forceinline__ unsigned knn_row(knn_entry e) { return (unsigned)e; }
// the total order: score descending (as floats: -0 == +0), row ascending
__device__ __forceinline__ bool knn_better(knn_entry a, knn_entry b) {
    const float sa = knn_score(a), sb = knn_score(b);
    return sa > sb || (sa == sb && knn_row(a) < knn_row(b));
}

// grid (cdiv(n, KNN_ROWS), cdiv(nct, CT)), block 256: wave w -> rows [(blockIdx.x * 4 + w) * 64, +64) of the piece x [n][d] as KNN_XB
// column blocks, against the query tiles [blockIdx.y * CT, +CT).  Qf [nct][KG][64], KG a multiple of 4; xnh [n]: the rows' value at
// link d (nullptr: 0).  S[q * pitch + row] <- the score, q < nq, row < n.
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void knn_score_kernel(const float* __restrict__ x, long long n, int d, const float* __restrict__ xnh,
                                                        const float4* __restrict__ Qf, int KG, int nct, int nq, float* __restrict__ S,
                                                        long long pitch) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const long long row0 = ((long long)blockIdx.x * 4 + w) * (KNN_XB * 32);
    if (row0 >= n) return;
    const int ct0 = blockIdx.y * CT;
    const float* xr[KNN_XB];
    float tl[KNN_XB];
#pragma unroll
    for (int b = 0; b < KNN_XB; ++b) {
        const long long r = row0 + b * 32 + c;
        const long long rc = r < n ? r : n - 1;   // clamp: duplicates are computed and not written
        xr[b] = x + (size_t)rc * d;
        tl[b] = xnh ? xnh[rc] : 0.0f;
    }
    const int nch = KG >> 2;
    f32x16 acc[CT][KNN_XB];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][b][r] = 0.0f;
    const float4* ap[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) ap[t] = Qf + (size_t)(ct0 + t < nct ? ct0 + t : nct - 1) * KG * 64 + lane;
    float bv[KNN_XB][16];
#pragma unroll
    for (int b = 0; b < KNN_XB; ++b) dense_load_b<VEC>(xr[b], d, 0, h, tl[b], bv[b]);
    float4 a[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) a[t] = ap[t][0];
    for (int ch = 0; ch < nch; ++ch) {
        // the next chunk's rows are requested before this chunk's MFMAs (the last chunk reads itself again)
        float bn[KNN_XB][16];
        const int chn = ch + 1 < nch ? ch + 1 : ch;
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b) dense_load_b<VEC>(xr[b], d, chn, h, tl[b], bn[b]);
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
                    for (int b = 0; b < KNN_XB; ++b)
                        acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b][4 * g + s], acc[t][b], 0, 0, 0);
                }
#pragma unroll
            for (int t = 0; t < CT; ++t) a[t] = an[t];
        }
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b)
#pragma unroll
            for (int s = 0; s < 16; ++s) bv[b][s] = bn[b][s];
    }
    // a lane holds one row of the piece and 16 queries of every tile: 32 lanes write 128 consecutive bytes of a query's slab row
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        if (ct0 + t >= nct) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = (ct0 + t) * 32 + acc_row(r, h);
            if (q >= nq) continue;
#pragma unroll
            for (int b = 0; b < KNN_XB; ++b) {
                const long long row = row0 + b * 32 + c;
                if (row < n) S[(size_t)q * pitch + row] = acc[t][b][r];
            }
        }
    }
}

// knn_score_kernel for a piece of halves (lmi_knn_f16, lmi_knn_range_f16): x [n][d] binary16 bit patterns, widened where they are
// loaded (dense_load_b's half form; VEC: d % 8 == 0 and x 16-byte aligned).  Grid, block, Qf, xnh and S as there, and the product loop
// word for word: a score is the chain of the widened row, bit for bit.  A kernel of its own so that the float kernel keeps its
// instructions (the precedent: ingest16_half_kernel).
template <int CT, bool VEC>
__global__ __launch_bounds__(256) void knn_score16_kernel(const unsigned short* __restrict__ x, long long n, int d,
                                                          const float* __restrict__ xnh, const float4* __restrict__ Qf, int KG, int nct,
                                                          int nq, float* __restrict__ S, long long pitch) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const long long row0 = ((long long)blockIdx.x * 4 + w) * (KNN_XB * 32);
    if (row0 >= n) return;
    const int ct0 = blockIdx.y * CT;
    const unsigned short* xr[KNN_XB];
    float tl[KNN_XB];
#pragma unroll
    for (int b = 0; b < KNN_XB; ++b) {
        const long long r = row0 + b * 32 + c;
        const long long rc = r < n ? r : n - 1;   // clamp: duplicates are computed and not written
        xr[b] = x + (size_t)rc * d;
        tl[b] = xnh ? xnh[rc] : 0.0f;
    }
    const int nch = KG >> 2;
    f32x16 acc[CT][KNN_XB];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][b][r] = 0.0f;
    const float4* ap[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) ap[t] = Qf + (size_t)(ct0 + t < nct ? ct0 + t : nct - 1) * KG * 64 + lane;
    float bv[KNN_XB][16];
#pragma unroll
    for (int b = 0; b < KNN_XB; ++b) dense_load_b<VEC>(xr[b], d, 0, h, tl[b], bv[b]);
    float4 a[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) a[t] = ap[t][0];
    for (int ch = 0; ch < nch; ++ch) {
        // the next chunk's rows are requested before this chunk's MFMAs (the last chunk reads itself again)
        float bn[KNN_XB][16];
        const int chn = ch + 1 < nch ? ch + 1 : ch;
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b) dense_load_b<VEC>(xr[b], d, chn, h, tl[b], bn[b]);
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
                    for (int b = 0; b < KNN_XB; ++b)
                        acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b][4 * g + s], acc[t][b], 0, 0, 0);
                }
#pragma unroll
            for (int t = 0; t < CT; ++t) a[t] = an[t];
        }
#pragma unroll
        for (int b = 0; b < KNN_XB; ++b)
#pragma unroll
            for (int s = 0; s < 16; ++s) bv[b][s] = bn[b][s];
    }
    // a lane holds one row of the piece and 16 queries of every tile: 32 lanes write 128 consecutive bytes of a query's slab row
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        if (ct0 + t >= nct) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = (ct0 + t) * 32 + acc_row(r, h);
            if (q >= nq) continue;
#pragma unroll
            for (int b = 0; b < KNN_XB; ++b) {
                const long long row = row0 + b * 32 + c;
                if (row < n) S[(size_t)q * pitch + row] = acc[t][b][r];
            }
        }
    }
}

// lists [n] <- empty
__global__ void knn_fill_kernel(knn_entry* __restrict__ lists, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) lists[i] = KNN_EMPTY;
}

// One wave (a 64-thread block): compare-exchange passes over e[0, n), n a power of two >= 128.
// knn_bitonic_merge: e is best-first in its first half and worst-first in its second -> best-first throughout.
__device__ __forceinline__ void knn_bitonic_merge(knn_entry* e, int n, int lane) {
    for (int stride = n >> 1; stride > 0; stride >>= 1) {
        for (int i = lane; i < (n >> 1); i += 64) {
            const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
            const knn_entry a = e[lo], b = e[hi];
            if (knn_better(b, a)) { e[lo] = b; e[hi] = a; }
        }
        __syncthreads();
    }
}
// knn_bitonic_sort_up: any e -> worst-first
__device__ __forceinline__ void knn_bitonic_sort_up(knn_entry* e, int n, int lane) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = lane; i < (n >> 1); i += 64) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
                const bool up = (lo & size) == 0 || size == n;   // worst-first blocks; the last pass: all of it
                const knn_entry a = e[lo], b = e[hi];
                if (up ? knn_better(a, b) : knn_better(b, a)) { e[lo] = b; e[hi] = a; }
            }
            __syncthreads();
        }
}

// One wave (a 64-thread block, dynamic LDS 2 * LR entries): continues the sorted list `mine` (best-first, LR a power of two >=
// max(k, 128); fresh: starts from an empty list instead of reading it) with the scores row[a .. b); the score at position p enters as
// the pair (score, row_base + p).  Only scores > -FLT_MAX are taken (a NaN is not).  knn_select_kernel and union_select_kernel
// (lmi_union.h) are this with their own addressing.
__device__ __forceinline__ void knn_select_wave(const float* __restrict__ row, long long a, long long b, unsigned row_base, int k, int LR,
                                                knn_entry* __restrict__ mine, bool fresh) {
    extern __shared__ knn_entry knn_lds[];
    const int lane = threadIdx.x;
    for (int i = lane; i < LR; i += 64) knn_lds[i] = fresh ? KNN_EMPTY : mine[i];
    __syncthreads();
    knn_entry thr = knn_lds[k - 1];
    knn_entry* buf = knn_lds + LR;
    int cnt = 0;   // uniform
    auto flush = [&]() {
        for (int i = cnt + lane; i < LR; i += 64) buf[i] = KNN_EMPTY;
        __syncthreads();
        knn_bitonic_sort_up(buf, LR, lane);
        knn_bitonic_merge(knn_lds, 2 * LR, lane);
        thr = knn_lds[k - 1];
        cnt = 0;
        __syncthreads();
    };
    for (long long p0 = a; p0 < b; p0 += 256) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long p = p0 + u * 64 + lane;
            v[u] = p < b ? row[p] : -FLT_MAX;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const knn_entry e = knn_make(v[u], row_base + (unsigned)(p0 + u * 64 + lane));
            const bool pass = v[u] > -FLT_MAX && knn_better(e, thr);
            const unsigned long long m = __ballot(pass);
            if (!m) continue;
            const int np = __popcll(m);
            if (cnt + np > LR) flush();   // what passed the old threshold still goes in: the merge puts it where it belongs
            if (pass) buf[cnt + __popcll(m & ((1ull << lane) - 1))] = e;
            cnt += np;
        }
    }
    if (cnt) flush();
    else __syncthreads();
    for (int i = lane; i < LR; i += 64) mine[i] = knn_lds[i];
}

// grid (nq, splits), block 64, dynamic LDS 2 * LR entries.  The wave of (query q, split s) continues lists[(q * splits + s) * LR ..)
// with the scores S[q * pitch + a .. b), [a, b) = split s of the piece's len rows; a score's row number is row_base + its position.
__global__ __launch_bounds__(64) void knn_select_kernel(const float* __restrict__ S, long long pitch, long long len, unsigned row_base,
                                                        int k, int LR, knn_entry* __restrict__ lists) {
    const int q = blockIdx.x, s = blockIdx.y, splits = gridDim.y;
    const long long a = len * s / splits, b = len * (s + 1) / splits;
    if (a >= b) return;   // uniform
    knn_select_wave(S + (size_t)q * pitch, a, b, row_base, k, LR, lists + ((size_t)q * splits + s) * LR, false);
}

// grid nq, block 64, dynamic LDS 2 * LR entries: merges the `splits` lists of query q and writes D[q][k], I[q][k] -- the first k
// entries in the total order; an empty slot pads with I = -1 and D = -FLT_MAX (L2: FLT_MAX).  qn: L2 only, D = fmaf(-2, key, qn[q]).
__global__ __launch_bounds__(64) void knn_merge_kernel(const knn_entry* __restrict__ lists, int splits, int LR, int k,
                                                       const float* __restrict__ qn, float* __restrict__ D, long long* __restrict__ I) {
    extern __shared__ knn_entry knn_lds[];
    const int lane = threadIdx.x, q = blockIdx.x;
    const knn_entry* mine = lists + (size_t)q * splits * LR;
    for (int i = lane; i < LR; i += 64) knn_lds[i] = mine[i];
    __syncthreads();
    for (int s = 1; s < splits; ++s) {
        for (int i = lane; i < LR; i += 64) knn_lds[LR + i] = mine[(size_t)s * LR + (LR - 1 - i)];
        __syncthreads();
        knn_bitonic_merge(knn_lds, 2 * LR, lane);
    }
    for (int j = lane; j < k; j += 64) {
        const knn_entry e = knn_lds[j];
        const bool empty = knn_row(e) == 0xffffffffu;
        const float key = knn_score(e);
        D[(size_t)q * k + j] = empty ? (qn ? FLT_MAX : -FLT_MAX) : qn ? __builtin_fmaf(-2.0f, key, qn[q]) : key;
        I[(size_t)q * k + j] = empty ? -1ll : (long long)knn_row(e);
    }
}

}  // namespace lmi
