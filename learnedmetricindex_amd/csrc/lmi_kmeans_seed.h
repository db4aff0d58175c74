// lmi_kmeans_seed.h -- device code of lmi_kmeans_seed / lmi_kmeans_seed_f16: greedy k-means++ seeding whose rows, potentials and
// centroids do not depend on the launch geometry (include/lmi_hip.h states the arithmetic).
//
// State per row: one integer W_i = w(distance to the nearest chosen centre), w(dist) = rint(dist * 2^(36-E)) in binary64.  w is
// monotone, so the minimum of distances is the minimum of weights and no float minimum is kept; every sum is an integer sum.
// A round (round 0: one candidate, W = all ones, T = 0) is
//   kpp_sample_kernel   one block per trial: draw below T, find the row whose inclusive prefix sum of W crosses it (T == 0: below n);
//   kpp_gather_kernel   the candidates' rows, widened, into a small row-major buffer; dense_norm_kernel and dense_pack_kernel
//                       (lmi_dense.h) turn it into ONE 32-wide A tile with -|c|^2/2 at link d;
//   kpp_round_kernel    S^T = C . X^T by v_mfma_f32_32x32x2_f32 -- the loop of km_assign_kernel with one centroid tile, B straight
//                       from the row-major x with a 1 at link d.  A lane owns one row and 16 candidates: it turns its keys into
//                       dist, stores dist into the candidate-major slab [L][n] (32 lanes: 128 consecutive bytes) and adds
//                       min(W_i, w(dist)) into 16 int64 partial sums; a block issues one 64-bit atomicAdd per candidate;
//   kpp_update_kernel   every block finds the winner of pot[0..L) itself, W_i = min(W_i, w(slab[win][i])), one exact sum per block
//                       of KPP_BLOCK rows; block 0 records the round's row and potential;
//   kpp_scan_kernel     one block: the exclusive scan of the block sums, and T behind it.
// Nothing returns to the host between rounds.  Every store is a plain vector store.
#pragma once
#include "lmi_dense.h"

namespace lmi {

constexpr int KPP_XB = 2;         // 32-row blocks of x per wave step
constexpr int KPP_BLOCK = 1024;   // rows per block sum (kpp_update_kernel, kpp_sample_kernel: 256 threads x 4 rows)
constexpr int KPP_MAX_TRIALS = 32;

__device__ __forceinline__ unsigned long long kpp_weight(float dist, double scale) {
    return (unsigned long long)__builtin_rint((double)dist * scale);
}

// z(t, j): the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (1 + 32 t + j), all mod 2^64
__device__ __forceinline__ unsigned long long kpp_draw(unsigned long long seed, int t, int j) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(1 + 32ll * t + j);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// out[p][.] = row list[p] of x, widened: p < m
template <class T>
__global__ void kpp_gather_kernel(const T* __restrict__ x, const long long* __restrict__ list, int m, int d, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)m * d) return;
    const int p = (int)(idx / d), t = (int)(idx % d);
    const T v = x[(size_t)list[p] * d + t];
    if constexpr (sizeof(T) == 2) out[idx] = (float)__builtin_bit_cast(_Float16, v);
    else out[idx] = v;
}

// grid: any, block 256.  Wave g of the grid -> rows [g * 64, +64), [(g + waves) * 64, +64), ..  Cf [1][KG][64]: the candidates'
// tile, KG a multiple of 4.  xn [n]: |x_i|^2 by the chain.  W [n] is read only.  slab [L][n], pot [L] (+=).
template <bool VEC, class T>
__global__ __launch_bounds__(256, 2) void kpp_round_kernel(const T* __restrict__ x, long long n, int d, const float4* __restrict__ Cf,
                                                           int KG, int L, const float* __restrict__ xn,
                                                           const unsigned long long* __restrict__ W, double scale,
                                                           float* __restrict__ slab, unsigned long long* __restrict__ pot) {
    __shared__ unsigned long long part_lds[4][32];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    const long long step = (long long)gridDim.x * 4 * (KPP_XB * 32);
    unsigned long long part[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) part[r] = 0;
    const int nch = KG >> 2;
    const float4* ap = Cf + lane;
    for (long long row0 = ((long long)blockIdx.x * 4 + w) * (KPP_XB * 32); row0 < n; row0 += step) {
        const T* xr[KPP_XB];
#pragma unroll
        for (int b = 0; b < KPP_XB; ++b) {
            const long long r = row0 + b * 32 + c;
            xr[b] = x + (size_t)(r < n ? r : n - 1) * d;   // clamp: duplicates are computed and discarded
        }
        f32x16 acc[KPP_XB];
#pragma unroll
        for (int b = 0; b < KPP_XB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
        float bv[KPP_XB][16];
#pragma unroll
        for (int b = 0; b < KPP_XB; ++b) dense_load_b<VEC>(xr[b], d, 0, h, 1.0f, bv[b]);
        float4 a = ap[0];
        for (int ch = 0; ch < nch; ++ch) {
            // the next chunk's rows are requested before this chunk's MFMAs (the last chunk reads itself again)
            float bn[KPP_XB][16];
            const int chn = ch + 1 < nch ? ch + 1 : ch;
#pragma unroll
            for (int b = 0; b < KPP_XB; ++b) dense_load_b<VEC>(xr[b], d, chn, h, 1.0f, bn[b]);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int gn = ch * 4 + g + 1 < KG ? ch * 4 + g + 1 : ch * 4 + g;
                const float4 an = ap[(size_t)gn * 64];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float av = s == 0 ? a.x : s == 1 ? a.y : s == 2 ? a.z : a.w;
#pragma unroll
                    for (int b = 0; b < KPP_XB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b][4 * g + s], acc[b], 0, 0, 0);
                }
                a = an;
            }
#pragma unroll
            for (int b = 0; b < KPP_XB; ++b)
#pragma unroll
                for (int s = 0; s < 16; ++s) bv[b][s] = bn[b][s];
        }
        // this lane's 16 candidates of its row: key -> dist -> the slab, and min(W, w(dist)) into the candidate's partial sum
#pragma unroll
        for (int b = 0; b < KPP_XB; ++b) {
            const long long i = row0 + b * 32 + c;
            if (i >= n) continue;
            const float xni = xn[i];
            const unsigned long long wi = W[i];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = acc_row(r, h);
                if (j >= L) continue;
                const float dist = __builtin_fmaxf(__builtin_fmaf(-2.0f, acc[b][r], xni), 0.0f);
                slab[(size_t)j * n + i] = dist;
                const unsigned long long wd = kpp_weight(dist, scale);
                part[r] += wd < wi ? wd : wi;
            }
        }
    }
    // the 32 lanes of a half hold partial sums of the same 16 candidates: across the half, then across the block's waves
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) part[r] += __shfl_xor(part[r], o);
        if (c == 0) part_lds[w][acc_row(r, h)] = part[r];
    }
    __syncthreads();
    if (threadIdx.x < L) {
        const unsigned long long s = part_lds[0][threadIdx.x] + part_lds[1][threadIdx.x] + part_lds[2][threadIdx.x] + part_lds[3][threadIdx.x];
        if (s) atomicAdd(&pot[threadIdx.x], s);
    }
}

// grid cdiv(n, KPP_BLOCK), block 256: thread -> rows blockIdx.x * KPP_BLOCK + threadIdx.x + 256 u.  The winner of pot[0..L) is the
// lowest potential, ties to the lowest trial.  bsum[blockIdx.x] = the sum of the block's new W.  Block 0: rows_out = cand[win],
// pot_out = pot[win].
__global__ __launch_bounds__(256) void kpp_update_kernel(const float* __restrict__ slab, long long n, int L,
                                                         const unsigned long long* __restrict__ pot, const long long* __restrict__ cand,
                                                         double scale, unsigned long long* __restrict__ W,
                                                         unsigned long long* __restrict__ bsum, long long* __restrict__ rows_out,
                                                         unsigned long long* __restrict__ pot_out) {
    __shared__ unsigned long long red[4];
    int win = 0;
    unsigned long long best = pot[0];
    for (int j = 1; j < L; ++j) {
        const unsigned long long p = pot[j];
        if (p < best) { best = p; win = j; }
    }
    const float* srow = slab + (size_t)win * n;
    unsigned long long s = 0;
#pragma unroll
    for (int u = 0; u < KPP_BLOCK / 256; ++u) {
        const long long i = (long long)blockIdx.x * KPP_BLOCK + u * 256 + threadIdx.x;
        if (i < n) {
            const unsigned long long wd = kpp_weight(srow[i], scale), wi = W[i];
            const unsigned long long m = wd < wi ? wd : wi;
            W[i] = m;
            s += m;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        if (blockIdx.x == 0) {
            *rows_out = cand[win];
            *pot_out = best;
        }
    }
}

// one block of 1024: prefix[b] = bsum[0] + .. + bsum[b-1], prefix[nb] = T.  nb <= 65536: a thread owns cdiv(nb, 1024) consecutive sums.
__global__ __launch_bounds__(1024) void kpp_scan_kernel(const unsigned long long* __restrict__ bsum, int nb,
                                                        unsigned long long* __restrict__ prefix) {
    __shared__ unsigned long long tot[1024];
    const int per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
    unsigned long long s = 0;
    for (int b = b0; b < b1; ++b) s += bsum[b];
    tot[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const unsigned long long v = threadIdx.x >= o ? tot[threadIdx.x - o] : 0;
        __syncthreads();
        tot[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = tot[threadIdx.x] - s;   // exclusive
    for (int b = b0; b < b1; ++b) { prefix[b] = run; run += bsum[b]; }
    if (threadIdx.x == 1023) prefix[nb] = tot[1023];
}

// grid L, block 256: trial j = blockIdx.x of round t.  T = prefix[nb].  T > 0: r = mulhi64(z, T); the block is the last one whose
// exclusive prefix is <= r, the row the one of that block's KPP_BLOCK whose exclusive prefix inside it is <= the rest < its inclusive
// prefix (a row of weight 0 is never that row).  T == 0: cand = mulhi64(z, n).
__global__ __launch_bounds__(256) void kpp_sample_kernel(const unsigned long long* __restrict__ W, long long n,
                                                         const unsigned long long* __restrict__ prefix, int nb, unsigned long long seed,
                                                         int t, long long* __restrict__ cand) {
    __shared__ unsigned long long sc[256];
    const unsigned long long z = kpp_draw(seed, t, blockIdx.x), T = prefix[nb];
    if (T == 0) {
        if (threadIdx.x == 0) cand[blockIdx.x] = (long long)__umul64hi(z, (unsigned long long)n);
        return;
    }
    const unsigned long long r = __umul64hi(z, T);
    int lo = 0, hi = nb;   // prefix[lo] <= r < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= r) lo = mid; else hi = mid;
    }
    const unsigned long long rest = r - prefix[lo];
    constexpr int PER = KPP_BLOCK / 256;
    unsigned long long wv[PER], s = 0;
    const long long i0 = (long long)lo * KPP_BLOCK + threadIdx.x * PER;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        wv[u] = i0 + u < n ? W[i0 + u] : 0;
        s += wv[u];
    }
    sc[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned long long v = threadIdx.x >= o ? sc[threadIdx.x - o] : 0;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = sc[threadIdx.x] - s;   // exclusive
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (run <= rest && rest < run + wv[u]) cand[blockIdx.x] = i0 + u;
        run += wv[u];
    }
}

}  // namespace lmi
