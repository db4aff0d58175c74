// lmi_dense.h -- the device pieces lmi_kmeans, lmi_knn and lmi_train share: of the streamed f32 product S^T = F . X^T by
// v_mfma_f32_32x32x2_f32 the operand load (dense_load_b) and the packing of F (dense_pack_kernel); the row norms (dense_norm_kernel)
// and the finite check (dense_absmax_kernel).
//
// F = the smaller side's rows in fragment order (lmi_kernels.h), X = the larger side's rows straight from a row-major array.  Both
// carry one link more than d: at link d a row of X holds a value the caller gives and a row of F another, so that their product adds
// one term to the chain (L2: the 1 meets the -|.|^2/2); links past d are zeros.  The link order inside every accumulator is
// 0, 1, 2, ..: an element of S is the canonical fmaf chain of oracle.knn_ip / knn_l2.
// The loop that runs the product is written out in km_assign_kernel, again in km_assign16_kernel (lmi_kmeans.h: the rows as halves),
// again in knn_score_kernel, again in knn_score16_kernel (lmi_knn.h: the base as halves) and again in union_score_kernel (lmi_union.h):
// the five must stay equal (DESIGN.md 5.11 says why it is not a function here).
//
// Half forms (lmi_knn_f16 / lmi_knn_range_f16: X and the rows F is packed from arrive as binary16 bit patterns; lmi_kmeans_f16: X
// does): dense_load_b on an unsigned short row, dense_pack16_kernel, dense_norm16_kernel, dense_absmax16_kernel.  Every half is widened by an exact conversion where it is loaded and
// from there on the arithmetic is the float form's, so the results are those of the widened arrays bit for bit; no row is widened
// into a buffer.  The float forms are left as they are, instruction for instruction.
#pragma once
#include "lmi_kernels.h"
#include "lmi_prefilter.h"   // half8

namespace lmi {

// max |v| as the bit pattern of its absolute value (monotone for binary32; >= 0x7f800000: inf or NaN)
__global__ void dense_absmax_kernel(const float* __restrict__ v, long long total, unsigned* __restrict__ out) {
    unsigned m = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        m = max(m, __float_as_uint(v[i]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// dense_absmax_kernel over halves: max of bits & 0x7fff (monotone for binary16; >= 0x7c00: inf or NaN).  The widened maximum is the
// maximum of the widened values -- subnormal halves included: widening is monotone and exact.
__global__ void dense_absmax16_kernel(const unsigned short* __restrict__ v, long long total, unsigned* __restrict__ out) {
    unsigned m = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) m = max(m, (unsigned)v[i] & 0x7fffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// out[i] = the chain acc = fmaf(x[t], x[t], acc) from 0, t ascending (neg_half: times -0.5f).  One thread per row.
__global__ void dense_norm_kernel(const float* __restrict__ x, long long n, int d, int neg_half, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = x + (size_t)i * d;
    float acc = 0.0f;
    for (int t = 0; t < d; ++t) acc = __builtin_fmaf(r[t], r[t], acc);
    out[i] = neg_half ? -0.5f * acc : acc;
}

// dense_norm_kernel over rows of halves: the same chain over the widened values
__global__ void dense_norm16_kernel(const unsigned short* __restrict__ x, long long n, int d, int neg_half, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned short* r = x + (size_t)i * d;
    float acc = 0.0f;
    for (int t = 0; t < d; ++t) {
        const float v = (float)__builtin_bit_cast(_Float16, r[t]);
        acc = __builtin_fmaf(v, v, acc);
    }
    out[i] = neg_half ? -0.5f * acc : acc;
}

// rows [n][d] -> fragment order [nct][KG][64] float4 (rows >= n and links > d: zeros; link d: tailv[row], or `tail` for every row
// when tailv is null).  One thread per (row, group of 8 links); element loads: any 4-byte aligned src.
__global__ void dense_pack_kernel(const float* __restrict__ src, const float* __restrict__ tailv, float tail, int n, int d, int nct,
                                  int KG, float4* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)nct * 32 * KG) return;
    const int g = (int)(idx % KG);
    const int p = (int)(idx / KG);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int t = g * 8 + j;
        v[j] = p >= n ? 0.0f : t < d ? src[(size_t)p * d + t] : t == d ? (tailv ? tailv[p] : tail) : 0.0f;
    }
    float4* f = dst + ((size_t)(p >> 5) * KG + g) * 64 + (p & 31);
    f[0] = make_float4(v[0], v[2], v[4], v[6]);
    f[32] = make_float4(v[1], v[3], v[5], v[7]);
}

// dense_pack_kernel from rows of halves (no tailv: the callers give one tail for every row).  Element loads: any 2-byte aligned src.
__global__ void dense_pack16_kernel(const unsigned short* __restrict__ src, float tail, int n, int d, int nct, int KG,
                                    float4* __restrict__ dst) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)nct * 32 * KG) return;
    const int g = (int)(idx % KG);
    const int p = (int)(idx / KG);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int t = g * 8 + j;
        v[j] = p >= n ? 0.0f : t < d ? (float)__builtin_bit_cast(_Float16, src[(size_t)p * d + t]) : t == d ? tail : 0.0f;
    }
    float4* f = dst + ((size_t)(p >> 5) * KG + g) * 64 + (p & 31);
    f[0] = make_float4(v[0], v[2], v[4], v[6]);
    f[32] = make_float4(v[1], v[3], v[5], v[7]);
}

// The B operands of one 32-link chunk for the row `xr` points to: b[s] feeds MFMA step s of the chunk, i.e. this lane's
// link 32*ch + 2*s + h.  VEC (d % 4 == 0, x 16-byte aligned): the lane pair (c, 0), (c, 1) reads the row's 128 bytes of the chunk
// with four 16-byte loads each (h = 0: links 0..15, h = 1: links 16..31) and trades the halves it does not feed with
// v_permlane32_swap; otherwise sixteen 4-byte loads.  Link d is `tail`, links past d are zero.
template <bool VEC>
__device__ __forceinline__ void dense_load_b(const float* __restrict__ xr, int d, int ch, int h, float tail, float (&b)[16]) {
    if constexpr (VEC) {
        float r[16];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int k0 = 32 * ch + 16 * h + 4 * f;
            float4 v = *reinterpret_cast<const float4*>(xr + (k0 < d ? k0 : 0));
            if (k0 >= d) v = make_float4(k0 == d ? tail : 0.0f, 0.0f, 0.0f, 0.0f);
            r[4 * f] = v.x; r[4 * f + 1] = v.y; r[4 * f + 2] = v.z; r[4 * f + 3] = v.w;
        }
        // lanes 32..63 of r[2i] (k = 16+2i) <-> lanes 0..31 of r[2i+1] (k = 2i+1): then r[2i] = (k 2i | 2i+1), r[2i+1] = (k 16+2i | 16+2i+1)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r[2 * i]), __float_as_uint(r[2 * i + 1]), false, false);
            b[i] = __uint_as_float(sw[0]);
            b[8 + i] = __uint_as_float(sw[1]);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int t = 32 * ch + 2 * s + h;
            const float v = xr[t < d ? t : 0];
            b[s] = t < d ? v : t == d ? tail : 0.0f;
        }
    }
}

// dense_load_b for a row of halves.  VEC (d % 8 == 0, x 16-byte aligned: every row then starts on a 16-byte boundary and every group
// of 8 links that starts below d lies inside the row): the lane's 16 links 32*ch + 16*h .. + 15 are two 16-byte loads of 8 halves,
// each widened exactly and traded as in the float form; a group that starts at or past d is read at offset 0 and replaced (link d:
// `tail`), so nothing is read past the row's d halves.  Otherwise sixteen 2-byte loads.
template <bool VEC>
__device__ __forceinline__ void dense_load_b(const unsigned short* __restrict__ xr, int d, int ch, int h, float tail, float (&b)[16]) {
    if constexpr (VEC) {
        float r[16];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int k0 = 32 * ch + 16 * h + 8 * f;
            const half8 hv = __builtin_bit_cast(half8, *reinterpret_cast<const uint4*>(xr + (k0 < d ? k0 : 0)));
#pragma unroll
            for (int j = 0; j < 8; ++j) r[8 * f + j] = k0 < d ? (float)hv[j] : j == 0 && k0 == d ? tail : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r[2 * i]), __float_as_uint(r[2 * i + 1]), false, false);
            b[i] = __uint_as_float(sw[0]);
            b[8 + i] = __uint_as_float(sw[1]);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int t = 32 * ch + 2 * s + h;
            const float v = (float)__builtin_bit_cast(_Float16, xr[t < d ? t : 0]);
            b[s] = t < d ? v : t == d ? tail : 0.0f;
        }
    }
}

}  // namespace lmi
