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

}  // namespace lmi
