// lmi_gram.h -- device code of lmi_gram: the mean and the centred scatter matrix of x [n][d], bit for bit the same on any launch
// geometry (include/lmi_hip.h states the arithmetic).
//
// Mean (gram_sum_kernel, gram_mean_kernel): lmi_kmeans's update with one cluster -- int64 sums of km_quant, km_mean (lmi_kmeans.h).
// Scatter (gram_kernel): G = C^T . C by v_mfma_f32_32x32x2_f32 where BOTH operands are column strips of the same row-major x: at the
// step of rows (i, i+1) lane (h, c) supplies c[i+h][A0+c] as A and c[i+h][B0+c] as B, so the link order inside every accumulator is the
// row order i, i+1, ..: an element of a piece's g_p is the canonical chain acc = fmaf(c[i][a], c[i][b], acc).  A block owns one tile
// of the upper triangle and a run of consecutive pieces; it stages panels of GRAM_PANEL rows x (A strip + B strip) through LDS (two
// buffers: the next panel is in flight from global memory while this one feeds the MFMAs), subtracts the mean as a value leaves LDS --
// no centred copy of x exists --, and at every piece seam turns the accumulators into Q_p = rint(g_p * 2^(32-2e)) and adds them to
// int64 registers; one 64-bit atomicAdd per element and block then folds the run into T.  Integer addition is associative: T does
// not depend on the tiles, the runs or the order of the atomics.  gram_finish_kernel converts and mirrors.
// Rows past the run's end are staged as the mean itself (m - m = +0) and columns past d as 0 against a mean of 0: the padded links are
// fmaf(+0, +0, acc).
// The half form (lmi_gram_f16) widens every half exactly where it is loaded from global memory; LDS holds binary32 either way, so the
// product loop is the float form's and the result is that of the widened array.
#pragma once
#include "lmi_dense.h"
#include "lmi_kmeans.h"   // km_quant, km_mean

namespace lmi {

constexpr int GRAM_PANEL = 16;       // rows per LDS panel (lmi_gram_plan::PANEL_ROWS)
constexpr int GRAM_PIECE = 4096;     // LMI_GRAM_PIECE_ROWS: rows per piece chain
constexpr int GRAM_SUM_ROWS = 1024;  // rows per gram_sum_kernel block

__device__ __forceinline__ float gram_widen(float v) { return v; }
__device__ __forceinline__ float gram_widen(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }

// grid (cdiv(n, GRAM_SUM_ROWS), cdiv(d, 64)), block 256 = 4 row lanes x 64 columns: S[t] += the sum of km_quant(x[i][t]) over the
// block's rows, the four row lanes joined in LDS, one atomicAdd per column.
template <class T>
__global__ __launch_bounds__(256) void gram_sum_kernel(const T* __restrict__ x, long long n, int d, double scale,
                                                       unsigned long long* __restrict__ S) {
    __shared__ long long part[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, t = blockIdx.y * 64 + tx;
    const long long r0 = (long long)blockIdx.x * GRAM_SUM_ROWS, r1 = r0 + GRAM_SUM_ROWS < n ? r0 + GRAM_SUM_ROWS : n;
    long long acc = 0;
    if (t < d)
        for (long long i = r0 + ty; i < r1; i += 4) acc += km_quant(gram_widen(x[(size_t)i * d + t]), scale);
    part[ty][tx] = acc;
    __syncthreads();
    if (ty == 0 && t < d) {
        const long long s = part[0][tx] + part[1][tx] + part[2][tx] + part[3][tx];
        if (s) atomicAdd(&S[t], (unsigned long long)s);
    }
}

__global__ void gram_mean_kernel(const long long* __restrict__ S, long long n, int d, double unscale, float* __restrict__ mean) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < d) mean[t] = km_mean(S[t], n, unscale);
}

// One unit of a panel: V consecutive columns of one row, from column t (a multiple of V; VEC: d % V == 0, so a unit lies inside the
// row or past it).  Rows >= r_end hold the mean, columns >= d hold 0.
template <class T, bool VEC>
struct GramUnit;
template <>
struct GramUnit<float, true> {
    static constexpr int V = 4;
    static __device__ __forceinline__ void load(const float* __restrict__ x, const float* __restrict__ mean, long long i, long long r_end,
                                                int d, int t, float (&v)[4]) {
        if (t >= d) { v[0] = v[1] = v[2] = v[3] = 0.0f; return; }
        const float4 q = *reinterpret_cast<const float4*>(i < r_end ? x + (size_t)i * d + t : mean + t);   // mean: a hipMalloc'ed base, t % 4 == 0
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
};
template <>
struct GramUnit<float, false> {
    static constexpr int V = 1;
    static __device__ __forceinline__ void load(const float* __restrict__ x, const float* __restrict__ mean, long long i, long long r_end,
                                                int d, int t, float (&v)[1]) {
        v[0] = t >= d ? 0.0f : i < r_end ? x[(size_t)i * d + t] : mean[t];
    }
};
template <>
struct GramUnit<unsigned short, true> {
    static constexpr int V = 8;
    static __device__ __forceinline__ void load(const unsigned short* __restrict__ x, const float* __restrict__ mean, long long i,
                                                long long r_end, int d, int t, float (&v)[8]) {
        if (t >= d) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.0f;
        } else if (i < r_end) {
            const half8 hv = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(x + (size_t)i * d + t));
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)hv[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = mean[t + j];
        }
    }
};
template <>
struct GramUnit<unsigned short, false> {
    static constexpr int V = 1;
    static __device__ __forceinline__ void load(const unsigned short* __restrict__ x, const float* __restrict__ mean, long long i,
                                                long long r_end, int d, int t, float (&v)[1]) {
        v[0] = t >= d ? 0.0f : i < r_end ? gram_widen(x[(size_t)i * d + t]) : mean[t];
    }
};

// grid (tiles of the upper triangle, runs), block 256.  NT: 32-wide accumulator tiles per wave and side; the block's tile of G is
// TC x TC, TC = 64 * NT, wave w -> rows [64 * NT / 2 * (w >> 1), ..) x columns [.. (w & 1), ..) of it as NT x NT accumulators.
// tile_map[blockIdx.x] = ta << 16 | tb, ta <= tb.  Run blockIdx.y covers the rows [run * ppb * GRAM_PIECE, ..) clipped to n.
// Tq [d][d] int64, zeroed: receives the elements with a <= b < d.  scale = 2^(32-2e).
template <class T, bool VEC, int NT>
__global__ __launch_bounds__(256) void gram_kernel(const T* __restrict__ x, long long n, int d, const float* __restrict__ mean,
                                                   const int* __restrict__ tile_map, long long ppb, double scale,
                                                   unsigned long long* __restrict__ Tq) {
    constexpr int TC = 64 * NT, V = GramUnit<T, VEC>::V, UPR = TC / V;      // units per strip row
    constexpr int LDW = 2 * TC + 32;                                         // floats per LDS row: A strip, B strip, pad
    constexpr int UNITS = 2 * GRAM_PANEL * UPR, ITER = UNITS / 256;          // units of a panel (both strips), per thread
    static_assert(UNITS % 256 == 0, "a panel's units divide over the block");
    __shared__ float lds[2][GRAM_PANEL][LDW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const int ta = tile_map[blockIdx.x] >> 16, tb = tile_map[blockIdx.x] & 0xffff;
    const bool diag = ta == tb;                                              // uniform: the B strip is the A strip
    const int A0 = ta * TC, B0 = tb * TC;
    const long long r_begin = (long long)blockIdx.y * ppb * GRAM_PIECE;
    const long long r_last = r_begin + ppb * GRAM_PIECE;
    const long long r_end = r_last < n ? r_last : n;
    const int panels = (int)((r_end - r_begin + GRAM_PANEL - 1) / GRAM_PANEL);
    const int units = diag ? UNITS / 2 : UNITS;

    // this wave's columns of both strips and their means (columns >= d: 0)
    const int aoff = (w >> 1) * 32 * NT, boff = (diag ? 0 : TC) + (w & 1) * 32 * NT;
    float mA[NT], mB[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int a = A0 + aoff + 32 * j + c, b = B0 + (w & 1) * 32 * NT + 32 * j + c;
        mA[j] = a < d ? mean[a] : 0.0f;
        mB[j] = b < d ? mean[b] : 0.0f;
    }
    f32x16 acc[NT][NT];
    long long tq[NT][NT][16];
#pragma unroll
    for (int ja = 0; ja < NT; ++ja)
#pragma unroll
        for (int jb = 0; jb < NT; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[ja][jb][r] = 0.0f; tq[ja][jb][r] = 0; }

    float stash[ITER][V];
    auto fetch = [&](int panel) {
        const long long i0 = r_begin + (long long)panel * GRAM_PANEL;
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int u = it * 256 + threadIdx.x;
            if (u >= units) continue;
            const int s = u / (GRAM_PANEL * UPR), rem = u % (GRAM_PANEL * UPR);
            GramUnit<T, VEC>::load(x, mean, i0 + rem / UPR, r_end, d, (s ? B0 : A0) + (rem % UPR) * V, stash[it]);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int u = it * 256 + threadIdx.x;
            if (u >= units) continue;
            const int s = u / (GRAM_PANEL * UPR), rem = u % (GRAM_PANEL * UPR);
            float* dst = &lds[buf][rem / UPR][s * TC + (rem % UPR) * V];
#pragma unroll
            for (int j = 0; j < V; ++j) dst[j] = stash[it][j];
        }
    };

    fetch(0);
    stage(0);
    __syncthreads();
    for (int p = 0; p < panels; ++p) {
        const int buf = p & 1;
        if (p + 1 < panels) fetch(p + 1);   // in flight under this panel's MFMAs
#pragma unroll
        for (int k = 0; k < GRAM_PANEL; k += 2) {
            float av[NT], bv[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                av[j] = lds[buf][k + h][aoff + 32 * j + c] - mA[j];
                bv[j] = lds[buf][k + h][boff + 32 * j + c] - mB[j];
            }
#pragma unroll
            for (int ja = 0; ja < NT; ++ja)
#pragma unroll
                for (int jb = 0; jb < NT; ++jb) acc[ja][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ja], bv[jb], acc[ja][jb], 0, 0, 0);
        }
        // a piece seam (GRAM_PIECE / GRAM_PANEL panels from the run's start) or the run's end: g_p -> Q_p, into the int64 registers
        if ((p + 1) % (GRAM_PIECE / GRAM_PANEL) == 0 || p + 1 == panels) {
#pragma unroll
            for (int ja = 0; ja < NT; ++ja)
#pragma unroll
                for (int jb = 0; jb < NT; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tq[ja][jb][r] += (long long)__builtin_rint((double)acc[ja][jb][r] * scale);
                        acc[ja][jb][r] = 0.0f;
                    }
        }
        if (p + 1 < panels) stage(buf ^ 1);   // the buffer the previous iteration read: every wave has passed the barrier behind it
        __syncthreads();
    }
#pragma unroll
    for (int ja = 0; ja < NT; ++ja)
#pragma unroll
        for (int jb = 0; jb < NT; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int a = A0 + aoff + 32 * ja + acc_row(r, h), b = B0 + (w & 1) * 32 * NT + 32 * jb + c;
                if (a <= b && b < d && tq[ja][jb][r]) atomicAdd(&Tq[(size_t)a * d + b], (unsigned long long)tq[ja][jb][r]);
            }
}

// gram[a][b] = (double)T[min(a,b)][max(a,b)] * 2^(2e-32) (unscale): one int64 -> binary64 conversion, an exact scaling, the mirror
__global__ void gram_finish_kernel(const long long* __restrict__ Tq, int d, double unscale, double* __restrict__ gram) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)d * d) return;
    const int a = (int)(idx / d), b = (int)(idx % d);
    gram[idx] = (double)Tq[a <= b ? idx : (long long)b * d + a] * unscale;
}

}  // namespace lmi
