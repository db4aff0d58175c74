// lmi_cover.h -- device code of the bucket cover and of the pruning pass of the exact range search (lmi_cover_create,
// lmi_cover_order, lmi_search_range_exact; include/lmi_hip.h states the contract).
//
// The cover: three passes over the live rows of the row-major image, each bucket found through the per-bucket tables (rb_start,
// nb_rows), so a bucket that a mutation moved is read where it lies; rows at or past nb_rows[b], spare row-blocks and holes are never
// visited.  Only the caller's d columns of a row are read (L2: not the stored -|x|^2/2 column behind them).
//   cover_absmax_kernel   max |x| over the finite values as the bit pattern of its absolute value (dense_absmax_kernel's word), one
//                         atomicMax per wave;
//   cover_accum_kernel    S[b][t] += q(x[t]) in int64 registers, one 64-bit atomicAdd per (thread, column) -- km_accum_kernel's
//                         arithmetic (km_quant, lmi_kmeans.h); integer addition is associative, so S is the same on any grid;
//   cover_centre_kernel   c_b = km_mean(S, n_b) (km_finish_kernel's arithmetic), zeros for an empty bucket; cn_b = |c_b| in binary64;
//   cover_radius_kernel   per live row ONE binary64 chain acc = fma(delta, delta, acc) over the columns in ascending order (a tile
//                         of rows goes through LDS 32 columns at a time, the chain stays in the row's thread), the bucket's maximum
//                         by an atomicMax on the bit pattern of the non-negative binary64 -- a maximum does not depend on the order
//                         it is taken in.  A chain that is not finite is entered as +inf;
//   cover_finish_kernel   R_b = lmi_cover_plan::radius_of(R2_b).
// VEC: d % 4 == 0, a thread moves 16 bytes (the pitch is a multiple of 4 floats and the image 16-byte aligned, so every row is);
// otherwise scalar loads.
// The pruning pass:
//   cover_qnorm_kernel    |q| per query, a binary64 chain;
//   cover_admit_kernel    one thread per (query, bucket): lmi_cover_plan::link over the columns in ascending order with the chain in a
//                         register (the centres of 64 buckets and the block's queries go through LDS 32 columns at a time), then
//                         lmi_cover_plan::tail; a wave's 64 verdicts by ballot into two words of the query's bitmap row.  Every
//                         verdict is one thread's unsplit chain: the bitmap does not depend on groups, waves or grids;
//   cover_compact_kernel  one wave per query: the popcount of its row, and -- where an order is asked for -- the admitted bucket
//                         ids in ascending order by a prefix popcount, then -1 up to nb.
// Every store is a plain vector store; no atomic touches a float.
#pragma once
#include "lmi_kmeans.h"
#include "lmi_cover_plan.h"

namespace lmi {

constexpr int COVER_TILE_ROWS = 1024;   // rows of a bucket per block of the absmax and accum passes
constexpr int COVER_RAD_ROWS = 256;     // rows per block step of the radius pass: one per thread
constexpr int COVER_COLS = 32;          // columns staged per step (radius pass, admission)
constexpr int COVER_Q_PER_WAVE = 4;     // queries a thread of cover_admit_kernel carries
constexpr int COVER_Q_PER_BLOCK = 4 * COVER_Q_PER_WAVE;

// grid (tiles, L), block 256.  E = elements of a row (VEC: float4s, else floats); element i of the tile is (row i / E, piece i % E):
// consecutive threads take consecutive pieces of one row.
template <bool VEC>
__global__ __launch_bounds__(256) void cover_absmax_kernel(const float* __restrict__ rowmajor, int dp, int d, const int* __restrict__ rb_start,
                                                           const int* __restrict__ nb_rows, unsigned* __restrict__ out) {
    const int b = blockIdx.y;
    const int n_b = nb_rows[b];
    const int E = VEC ? d >> 2 : d;
    const float* base = rowmajor + (size_t)rb_start[b] * 32 * dp;
    unsigned m = 0;
    // a value that is not finite does not enter: its bucket's radius becomes +inf (cover_radius_kernel), the exponent stays the others'
    auto take = [&](float v) {
        const unsigned bits = __float_as_uint(v) & 0x7fffffffu;
        if (bits < 0x7f800000u) m = max(m, bits);
    };
    for (long long row0 = (long long)blockIdx.x * COVER_TILE_ROWS; row0 < n_b; row0 += (long long)gridDim.x * COVER_TILE_ROWS) {
        const int rows = (int)(n_b - row0 < COVER_TILE_ROWS ? n_b - row0 : COVER_TILE_ROWS);
        const int total = rows * E;   // (at most 1024 x 4096)
        for (int i = threadIdx.x; i < total; i += 256) {
            const int r = i / E;
            const int c = i - r * E;
            const float* src = base + (size_t)(row0 + r) * dp;
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(src + 4 * c);
                take(v.x), take(v.y), take(v.z), take(v.w);
            } else {
                take(src[c]);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// grid (tiles, L, cdiv(E, 256)), block 256.  The block's pieces: [blockIdx.z * 256, + CW), CW <= 256; thread -> piece tid % CW of
// the rows tid / CW, + RL, .. of the tile (RL = 256 / CW row lanes; the threads behind RL * CW idle).  scale = 2^(36-e).
template <bool VEC>
__global__ __launch_bounds__(256) void cover_accum_kernel(const float* __restrict__ rowmajor, int dp, int d, const int* __restrict__ rb_start,
                                                          const int* __restrict__ nb_rows, double scale, unsigned long long* __restrict__ S) {
    const int b = blockIdx.y;
    const int n_b = nb_rows[b];
    const int E = VEC ? d >> 2 : d;
    const int c0 = blockIdx.z * 256;
    const int CW = E - c0 < 256 ? E - c0 : 256;
    const int RL = 256 / CW;
    const int rl = threadIdx.x / CW, c = c0 + threadIdx.x % CW;
    if (rl >= RL) return;
    const float* base = rowmajor + (size_t)rb_start[b] * 32 * dp;
    constexpr int NV = VEC ? 4 : 1;
    long long acc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = 0;
    for (long long row0 = (long long)blockIdx.x * COVER_TILE_ROWS; row0 < n_b; row0 += (long long)gridDim.x * COVER_TILE_ROWS) {
        const long long row1 = row0 + COVER_TILE_ROWS < n_b ? row0 + COVER_TILE_ROWS : n_b;
        for (long long r = row0 + rl; r < row1; r += RL) {
            const float* src = base + (size_t)r * dp;
            if constexpr (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(src + 4 * c);
                acc[0] += km_quant(v.x, scale);
                acc[1] += km_quant(v.y, scale);
                acc[2] += km_quant(v.z, scale);
                acc[3] += km_quant(v.w, scale);
            } else {
                acc[0] += km_quant(src[c], scale);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (acc[j]) atomicAdd(&S[(size_t)b * d + (size_t)c * NV + j], (unsigned long long)acc[j]);
}

// one thread per (bucket, column): the centre; unscale = 2^(e-36)
__global__ void cover_centre_kernel(const long long* __restrict__ S, const int* __restrict__ nb_rows, int L, int d, double unscale,
                                    float* __restrict__ centres) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)L * d) return;
    const int m = nb_rows[idx / d];
    centres[idx] = m > 0 ? km_mean(S[idx], m, unscale) : 0.0f;
}

// one thread per bucket: cn_b = |c_b|
__global__ void cover_cnorm_kernel(const float* __restrict__ centres, int L, int d, double* __restrict__ cn) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L) return;
    cn[b] = lmi_cover_plan::norm_of(centres + (size_t)b * d, d);
}

// grid (tiles, L), block COVER_RAD_ROWS: thread -> row row0 + tid of bucket blockIdx.y.  r2bits [L] (zeroed by the caller) <- the
// bit pattern of the bucket's largest chain.
template <bool VEC>
__global__ __launch_bounds__(COVER_RAD_ROWS) void cover_radius_kernel(const float* __restrict__ rowmajor, int dp, int d,
                                                                     const int* __restrict__ rb_start, const int* __restrict__ nb_rows,
                                                                     const float* __restrict__ centres,
                                                                     unsigned long long* __restrict__ r2bits) {
    __shared__ float tile[COVER_RAD_ROWS][COVER_COLS + 1];   // (+ 1: a thread walks its own row, the rows fall into different banks)
    __shared__ float cen[COVER_COLS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n_b = nb_rows[b];
    const float* base = rowmajor + (size_t)rb_start[b] * 32 * dp;
    const float* cb = centres + (size_t)b * d;
    // (n_b, row0 and t0 are uniform over the block: every thread reaches every barrier)
    for (long long row0 = (long long)blockIdx.x * COVER_RAD_ROWS; row0 < n_b; row0 += (long long)gridDim.x * COVER_RAD_ROWS) {
        const bool live = row0 + tid < n_b;
        double acc = 0.0;
        for (int t0 = 0; t0 < d; t0 += COVER_COLS) {
            __syncthreads();   // the previous step's tile has been read
            if constexpr (VEC) {
#pragma unroll
                for (int j = 0; j < COVER_COLS / 4; ++j) {
                    const int i = j * COVER_RAD_ROWS + tid;
                    const int r = i / (COVER_COLS / 4), c4 = i % (COVER_COLS / 4);
                    if (row0 + r < n_b && t0 + 4 * c4 < d) {   // (d % 4 == 0: the piece lies inside the row)
                        const float4 v = *reinterpret_cast<const float4*>(base + (size_t)(row0 + r) * dp + t0 + 4 * c4);
                        tile[r][4 * c4 + 0] = v.x, tile[r][4 * c4 + 1] = v.y, tile[r][4 * c4 + 2] = v.z, tile[r][4 * c4 + 3] = v.w;
                    }
                }
            } else {
#pragma unroll 8
                for (int j = 0; j < COVER_COLS; ++j) {
                    const int i = j * COVER_RAD_ROWS + tid;
                    const int r = i / COVER_COLS, c = i % COVER_COLS;
                    if (row0 + r < n_b && t0 + c < d) tile[r][c] = base[(size_t)(row0 + r) * dp + t0 + c];
                }
            }
            if (tid < COVER_COLS) cen[tid] = t0 + tid < d ? cb[t0 + tid] : 0.0f;
            __syncthreads();
            if (live) {
                const int tn = d - t0 < COVER_COLS ? d - t0 : COVER_COLS;
                for (int t = 0; t < tn; ++t) acc = lmi_cover_plan::radius_link(acc, tile[tid][t], cen[t]);
            }
        }
        if (!live) acc = 0.0;
        else if (!(acc < INFINITY)) acc = INFINITY;   // a row with inf or NaN: the bucket is always visited
        unsigned long long bits = (unsigned long long)__double_as_longlong(acc);   // acc >= 0: the order of the bits is the order of the values
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)bits, o);
            bits = other > bits ? other : bits;
        }
        if ((tid & 63) == 0 && bits) atomicMax(r2bits + b, bits);
    }
}

__global__ void cover_finish_kernel(const unsigned long long* __restrict__ r2bits, int L, float* __restrict__ radius) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L) return;
    radius[b] = lmi_cover_plan::radius_of(__longlong_as_double((long long)r2bits[b]));
}

// ---- the pruning pass ----
// one thread per query: qn[q] = |q|
__global__ void cover_qnorm_kernel(const float* __restrict__ queries, int nq, int d, double* __restrict__ qn) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    qn[q] = lmi_cover_plan::norm_of(queries + (size_t)q * d, d);
}

// grid (cdiv(gq, COVER_Q_PER_BLOCK), cdiv(L, 64)), block 256.  Lane l of every wave judges bucket blockIdx.y * 64 + l; wave w takes
// the block's queries w * COVER_Q_PER_WAVE + j.  queries / qn / radius: the group's first query onwards, gq of them.
// bitmap [gq][W] words: the block writes words 2 blockIdx.y and 2 blockIdx.y + 1 of its queries' rows (W is even: every word of a
// row is written by exactly one wave; buckets >= L judge as not admitted).
__global__ __launch_bounds__(256) void cover_admit_kernel(int metric, const float* __restrict__ queries, const double* __restrict__ qn,
                                                          const float* __restrict__ radius, int gq, int d,
                                                          const float* __restrict__ centres, const double* __restrict__ cn,
                                                          const float* __restrict__ R, const int* __restrict__ nb_rows, int L, int W,
                                                          unsigned* __restrict__ bitmap) {
    __shared__ float cen[64][COVER_COLS + 1];
    __shared__ float qs[COVER_Q_PER_BLOCK][COVER_COLS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y * 64 + lane;
    const int q0 = blockIdx.x * COVER_Q_PER_BLOCK;
    double chain[COVER_Q_PER_WAVE];
#pragma unroll
    for (int j = 0; j < COVER_Q_PER_WAVE; ++j) chain[j] = 0.0;
    for (int t0 = 0; t0 < d; t0 += COVER_COLS) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 64 * COVER_COLS / 256; ++j) {
            const int i = j * 256 + tid;
            const int r = i / COVER_COLS, c = i % COVER_COLS;
            const int bb = blockIdx.y * 64 + r;
            cen[r][c] = bb < L && t0 + c < d ? centres[(size_t)bb * d + t0 + c] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < COVER_Q_PER_BLOCK * COVER_COLS / 256; ++j) {
            const int i = j * 256 + tid;
            const int r = i / COVER_COLS, c = i % COVER_COLS;
            qs[r][c] = q0 + r < gq && t0 + c < d ? queries[(size_t)(q0 + r) * d + t0 + c] : 0.0f;
        }
        __syncthreads();
        const int tn = d - t0 < COVER_COLS ? d - t0 : COVER_COLS;
        for (int t = 0; t < tn; ++t) {
            const float c = cen[lane][t];
#pragma unroll
            for (int j = 0; j < COVER_Q_PER_WAVE; ++j) chain[j] = lmi_cover_plan::link(metric, chain[j], qs[w * COVER_Q_PER_WAVE + j][t], c);
        }
    }
    const bool in = b < L;
    const double cnb = in ? cn[b] : 0.0;
    const float Rb = in ? R[b] : 0.0f;
    const long long n_b = in ? nb_rows[b] : 0;
    const double u = lmi_cover_plan::margin_unit(d);
#pragma unroll
    for (int j = 0; j < COVER_Q_PER_WAVE; ++j) {
        const int q = q0 + w * COVER_Q_PER_WAVE + j;
        if (q >= gq) break;   // uniform over the wave
        const bool ok = lmi_cover_plan::tail(metric, chain[j], qn[q], cnb, Rb, n_b, radius[q], u);
        const unsigned long long m = __ballot(ok);
        unsigned* row = bitmap + (size_t)q * W + 2 * blockIdx.y;
        if (lane == 0) row[0] = (unsigned)m;
        if (lane == 32) row[1] = (unsigned)(m >> 32);
    }
}

// grid gq, block 64: query q of the group.  counts[q] <- the admitted buckets; order (nullable) [gq][nb] <- their ids ascending,
// then -1.  Nothing at or past column nb is written (the host refuses a call whose counts exceed nb before it hands the order on).
__global__ __launch_bounds__(64) void cover_compact_kernel(const unsigned* __restrict__ bitmap, int W, int nb, int* __restrict__ order,
                                                           int* __restrict__ counts) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const unsigned* row = bitmap + (size_t)q * W;
    int* out = order ? order + (size_t)q * nb : nullptr;
    int base = 0;   // uniform
    for (int w0 = 0; w0 < W; w0 += 64) {
        unsigned word = w0 + lane < W ? row[w0 + lane] : 0u;
        const int pc = __popc(word);
        int incl = pc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o);
            if (lane >= o) incl += v;
        }
        if (out) {
            int at = base + incl - pc;
            while (word) {
                const int bit = __ffs((int)word) - 1;
                word &= word - 1;
                if (at < nb) out[at] = (w0 + lane) * 32 + bit;
                ++at;
            }
        }
        base += __shfl(incl, 63);
    }
    if (lane == 0) counts[q] = base;
    if (out)
        for (int i = base + lane; i < nb; i += 64) out[i] = -1;
}

}  // namespace lmi
