// lmi_store16.h -- LMI_STORAGE_F16: an index that keeps its vectors as the prefilter's fp16 fragments only (gfx950).
//
// For vectors that are exactly representable in binary16 -- data distributed as 16-bit floats -- the fragments pass 1 and pass 2
// stream already hold every bit, and the row-major f32 image (two thirds of the index) is redundant.  Here are the kernels that
// build the fragments WITHOUT that image and read rows back out of them; the re-rank's readers are in lmi_prefilter.h
// (exact_score16), lmi_rescore.h (rc_run_batch<.., H>) and lmi_tail.h.
//
// Admissibility (decided here, on the device): every stored x is finite and binary16-exact, and so is x * s for the index scale s of
// scale_of_max (max|x| * s in [0.5, 1)).  Then (_Float16)(x * s) -- what convert16_one stores -- equals x * s, the fragments are the
// ones an LMI_STORAGE_F32 build makes, and (float)h * (1 / s) gives x back bit for bit: the canonical chain sees the same x[k].
// The absmax is only known at lmi_buckets_end, so a piece is stored UNSCALED as it arrives (ingest16_kernel: flags 1 / 2) and the
// whole slab is multiplied by s in place at the end (rescale16_kernel: flag 4; only a scale below 1 can lose bits).
//
// Binary16 sources (the *_f16 entry points of lmi_hip.h; halves travel as their uint16 bit patterns): rows and queries that the
// caller already holds as halves.  A half source pointer is only 2-byte aligned, so every kernel that reads one has two forms,
// chosen per launch on the host (half_src_vec): VEC -- one 16-byte load per 8 halves, only where d % 8 == 0 and the piece's base is
// 16-byte aligned, so that every row starts on a 16-byte boundary -- and element by element otherwise.
#pragma once
#include "lmi_prefilter.h"

namespace lmi {

constexpr unsigned S16_NONFINITE = 1u, S16_INEXACT = 2u, S16_SCALE_LOSS = 4u;   // state[1] of the kernels below

// One thread per (row i of the piece, 16-byte fragment piece k8): 8 consecutive k of the row -> halves -> the fragment of the row's
// slab position (scatter_rows_kernel's addressing of the input).  state[0] <- max |x| (bits), state[1] |= S16_* flags.
__global__ void ingest16_kernel(const float* __restrict__ src, int d, const int* __restrict__ pos, long long row0,
                                const long long* __restrict__ index, long long n_total, long long nrows, int KG16, int f16x16,
                                uint4* __restrict__ dst, unsigned* __restrict__ state) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n8 = 2 * KG16;
    float m = 0.0f;
    unsigned flags = 0u;
    if (idx < nrows * n8) {
        const long long i = idx / n8;
        const int k8 = (int)(idx - i * n8);
        const long long o = index ? index[i] : row0 + i;
        const long long p = (o < 0 || o >= n_total) ? -1 : pos[o];
        if (p >= 0) {
            half8 h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 8 * k8 + j;
                const float x = k < d ? src[i * d + k] : 0.0f;
                h[j] = (_Float16)x;
                if (!(fabsf(x) < INFINITY)) flags |= S16_NONFINITE;        // inf, NaN
                else if ((float)h[j] != x) flags |= S16_INEXACT;
                else m = fmaxf(m, fabsf(x));
            }
            dst[frag16_piece(p, k8, KG16, f16x16)] = *reinterpret_cast<uint4*>(&h);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o)); flags |= __shfl_xor(flags, o); }
    if ((threadIdx.x & 63) == 0) {
        if (m > 0.0f) atomicMax(state, __float_as_uint(m));
        if (flags) atomicOr(state + 1, flags);
    }
}

// ingest16_kernel for a piece that arrives as halves: the same thread shape and addressing, 8 halves gathered (VEC: one 16-byte load)
// and scattered as they are.  Every finite half is binary16-exact, so S16_INEXACT cannot arise; inf / NaN raise S16_NONFINITE as there
// and the absmax is taken over the finite values.  The float form above is left as it is.
template <bool VEC>
__global__ void ingest16_half_kernel(const unsigned short* __restrict__ src, int d, const int* __restrict__ pos, long long row0,
                                     const long long* __restrict__ index, long long n_total, long long nrows, int KG16, int f16x16,
                                     uint4* __restrict__ dst, unsigned* __restrict__ state) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n8 = 2 * KG16;
    float m = 0.0f;
    unsigned flags = 0u;
    if (idx < nrows * n8) {
        const long long i = idx / n8;
        const int k8 = (int)(idx - i * n8);
        const long long o = index ? index[i] : row0 + i;
        const long long p = (o < 0 || o >= n_total) ? -1 : pos[o];
        if (p >= 0) {
            uint4 w = make_uint4(0u, 0u, 0u, 0u);   // k >= d: zeros
            if constexpr (VEC) {
                if (8 * k8 < d) w = *reinterpret_cast<const uint4*>(src + i * d + 8 * k8);   // (d % 8 == 0: the whole piece is inside the row)
            } else {
                unsigned short e[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 8 * k8 + j;
                    e[j] = k < d ? src[i * d + k] : (unsigned short)0;
                }
                w = make_uint4(e[0] | (unsigned)e[1] << 16, e[2] | (unsigned)e[3] << 16, e[4] | (unsigned)e[5] << 16, e[6] | (unsigned)e[7] << 16);
            }
            const half8 h = __builtin_bit_cast(half8, w);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = (float)h[j];
                if (!(fabsf(x) < INFINITY)) flags |= S16_NONFINITE;        // inf, NaN
                else m = fmaxf(m, fabsf(x));
            }
            dst[frag16_piece(p, k8, KG16, f16x16)] = w;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o)); flags |= __shfl_xor(flags, o); }
    if ((threadIdx.x & 63) == 0) {
        if (m > 0.0f) atomicMax(state, __float_as_uint(m));
        if (flags) atomicOr(state + 1, flags);
    }
}

// n halves -> n floats (exact), dst 16-byte aligned (the library's own buffer): a staged piece of rows for an LMI_STORAGE_F32 build,
// which then takes scatter_rows_kernel / pack_scatter_kernel / augment_* unchanged, and the queries of the *_f16 search calls.
// VEC: n % 8 == 0, one thread per 8 halves.
template <bool VEC>
__global__ void widen16_kernel(const unsigned short* __restrict__ src, long long n, float* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (VEC) {
        if (idx >= (n >> 3)) return;
        const half8 h = __builtin_bit_cast(half8, reinterpret_cast<const uint4*>(src)[idx]);
        float4* o = reinterpret_cast<float4*>(dst) + 2 * idx;
        o[0] = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
        o[1] = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
    } else {
        if (idx >= n) return;
        dst[idx] = (float)__builtin_bit_cast(_Float16, src[idx]);
    }
}

// the whole slab x s in place (s = scale[0], a power of two; the product is exact in binary32): a half that changes when it is
// rounded back to binary16 raises S16_SCALE_LOSS
__global__ void rescale16_kernel(uint4* __restrict__ frag, long long n_pieces, const float* __restrict__ scale, unsigned* __restrict__ state) {
    const float s = scale[0];
    unsigned flags = 0u;
    if (s != 1.0f) {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pieces; i += (long long)gridDim.x * blockDim.x) {
            uint4 w = frag[i];
            if ((w.x | w.y | w.z | w.w) == 0u) continue;   // holes, padding
            half8 h = __builtin_bit_cast(half8, w);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)h[j] * s;
                h[j] = (_Float16)v;
                if ((float)h[j] != v) flags |= S16_SCALE_LOSS;
            }
            frag[i] = __builtin_bit_cast(uint4, h);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o);
    if ((threadIdx.x & 63) == 0 && flags) atomicOr(state + 1, flags);
}

// bucket_norm_kernel from the stored halves: x' = x * s IS the stored value, so ||x^ - x'|| = 0 (bdelta stays 0) and ||x'|| is summed
// in row_norms' order (k ascending, one multiply and one add per k): the same bits an LMI_STORAGE_F32 build of the rows gets
__global__ void bucket_norm16_kernel(const uint4* __restrict__ frag, int d, int KG16, int f16x16, const int* __restrict__ rb_start,
                                     const int* __restrict__ nb_rows, unsigned* __restrict__ bnorm_bits) {
    const int b = blockIdx.y;
    const int n_b = nb_rows[b];
    const float guard = norm_guard(d);
    const int n8 = (d + 7) >> 3;
    float best = 0.0f;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n_b; row += gridDim.x * blockDim.x) {
        const long long p = (long long)rb_start[b] * 32 + row;
        float acc = 0.0f;
        for (int k8 = 0; k8 < n8; ++k8) {
            const half8 h = __builtin_bit_cast(half8, frag[frag16_piece(p, k8, KG16, f16x16)]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (8 * k8 + j < d) {
                    const float xs = (float)h[j];
                    acc += xs * xs;
                }
            }
        }
        best = fmaxf(best, sqrtf(acc) * guard);
    }
    if (best > 0.0f) atomicMax(bnorm_bits + b, __float_as_uint(best));
}

// fragments of slab rows [p0, p0 + n) -> row-major f32 [n][d] (lmi_bucket_read; unpack_kernel's counterpart): x = (float)h * (1 / s)
__global__ void unpack16_kernel(const uint4* __restrict__ frag, int KG16, int f16x16, long long p0, long long n, int d,
                                const float* __restrict__ scale, float* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n8 = (d + 7) >> 3;
    if (idx >= n * n8) return;
    const int k8 = (int)(idx % n8);
    const long long i = idx / n8;
    const float inv = scale[1];
    const half8 h = __builtin_bit_cast(half8, frag[frag16_piece(p0 + i, k8, KG16, f16x16)]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (8 * k8 + j < d) dst[i * d + 8 * k8 + j] = (float)h[j] * inv;
}

// unpack16_kernel writing halves [n][d] (lmi_bucket_read_f16 on an LMI_STORAGE_F16 index): (float)h * (1 / s) is the original value,
// binary16-exact by the admissibility rule, so narrowing it returns the bits that were ingested.  dst: the library's staging buffer.
__global__ void unpack16_half_kernel(const uint4* __restrict__ frag, int KG16, int f16x16, long long p0, long long n, int d,
                                     const float* __restrict__ scale, unsigned short* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n8 = (d + 7) >> 3;
    if (idx >= n * n8) return;
    const int k8 = (int)(idx % n8);
    const long long i = idx / n8;
    const float inv = scale[1];
    const half8 h = __builtin_bit_cast(half8, frag[frag16_piece(p0 + i, k8, KG16, f16x16)]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (8 * k8 + j < d) dst[i * d + 8 * k8 + j] = __builtin_bit_cast(unsigned short, (_Float16)((float)h[j] * inv));
}

// lmi_bucket_read_f16 on an LMI_STORAGE_F32 index: slab rows [p0, p0 + n), columns [0, d) -> halves [n][d], one thread per value.
// FRAG = false: the row-major image (`a` = its pitch in floats); FRAG = true: the f32 fragments of the all-f32 scan (`a` = KGs; the
// layout of pack_scatter_kernel: k-group g of row p is float4s e, o = ((p >> 5) * KG + g) * 64 + (p & 31) + {0, 32}, k = 8 g + 2 c + {0, 1}
// their component c).  flag[0] |= 1 where a value is not finite or not binary16-exact: the call then fails and serves nothing.
template <bool FRAG>
__global__ void narrow16_kernel(const float* __restrict__ src, int a, long long p0, long long n, int d, unsigned short* __restrict__ dst,
                                unsigned* __restrict__ flag) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned bad = 0u;
    if (idx < n * d) {
        const long long i = idx / d, p = p0 + i;
        const int k = (int)(idx - i * d);
        float x;
        if constexpr (FRAG) x = src[((((size_t)(p >> 5) * a + (k >> 3)) * 64 + (p & 31) + (k & 1) * 32) << 2) + ((k & 7) >> 1)];
        else x = src[(size_t)p * a + k];
        const _Float16 hx = (_Float16)x;
        if (!(fabsf(x) < INFINITY) || (float)hx != x) bad = 1u;
        dst[idx] = __builtin_bit_cast(unsigned short, hx);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr(flag, bad);
}

}  // namespace lmi
