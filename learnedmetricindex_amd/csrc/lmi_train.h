// lmi_train.h -- device code of lmi_train: Adam steps on a Linear/ReLU stack whose trained weights do not depend on the launch
// geometry (include/lmi_hip.h states the arithmetic).
//
// The three products of a layer -- forward z = b + a . W^T, back-propagation da = g . W, weight gradient dW = g^T . a -- are one
// kernel, tr_gemm_kernel: a wave owns ONE 32 x 32 tile of the output and runs v_mfma_f32_32x32x2_f32 over the whole chain index
// (the input dimension, o, r) in ascending order, so every output element is the k-ordered fmaf chain of the contract and has
// exactly one owner; nothing is split, nothing is added atomically.  Operands are read straight from the row-major arrays through
// two strides each; rows, columns and chain indices past the end are zeros in the operands, never a change of the chain order.
// The epilogue is what the product is for: store z; mask da by z_{l-1} > 0; Adam on W (and, in the tiles of column block 0, the bias
// gradient as a row-ordered chain of adds and Adam on b).  Activations are not stored: a_l = z_{l-1} > 0 ? z_{l-1} : +0 is applied
// where z_{l-1} is read as an operand.
#pragma once
#include "lmi_dense.h"   // dense_absmax_kernel: the finite check of the named rows and the weights

namespace lmi {

enum { TR_FWD = 0, TR_DA = 1, TR_DW = 2 };

struct TrGemm {
    const float* A; long long a_sm, a_sk;   // A(m, k) = A[m * a_sm + k * a_sk]
    const float* B; long long b_sk, b_sn;   // B(k, n) = B[k * b_sk + n * b_sn]
    int M, N, K;
    int relu_a, relu_b;                     // the operand is z of the layer before: read it as z > 0 ? z : +0
    const float* bias;                      // TR_FWD: the chain starts at bias[n]
    float* out;                             // TR_FWD: z [M][N]; TR_DA: g of the layer before [M][N]
    const float* zprev;                     // TR_DA: z of the layer before [M][N]
    float *W, *mW, *vW;                     // TR_DW: [M][N], updated in place
    float *b, *mb, *vb;                     // TR_DW: [M]
    const float* g;                         // TR_DW: g [K][M] (the A operand) for the bias chain
    float step, r2;                         // Adam: (float)(lr / (1 - 0.9^t)), (float)sqrt(1 - 0.999^t)
    const float* lrow;                      // TR_DW, nullable: -logf(p[r][y_r]) of the K rows -> *loss (tile (0, 0))
    float* loss;
};

// One Adam update, every operation rounded on its own (the build has -ffp-contract=off); sqrtf and / are hipcc's correctly rounded
// forms (its default: -fhip-fp32-correctly-rounded-divide-sqrt).
__device__ __forceinline__ void tr_adam(float grad, float& p, float& m, float& v, float step, float r2) {
    m = 0.9f * m + 0.1f * grad;
    v = 0.999f * v + (0.001f * grad) * grad;
    const float den = __builtin_sqrtf(v) / r2 + 1e-8f;
    p = p - step * (m / den);
}

// this lane's operands of the 16 MFMA steps of chunk ch: step s takes k = 32 * ch + 2 * s + h
__device__ __forceinline__ void tr_load(const float* __restrict__ p, long long s_row, long long s_k, int row, int rows, int K, int ch, int h,
                                        int relu, float (&v)[16]) {
    const float* pr = p + (long long)row * s_row;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int k = 32 * ch + 2 * s + h;
        float x = 0.0f;
        if (row < rows && k < K) x = pr[(long long)k * s_k];
        v[s] = relu ? (x > 0.0f ? x : 0.0f) : x;
    }
}

// grid (cdiv(N, 32), cdiv(M, 32)), block 64: the wave owns rows [32 * blockIdx.y, +32) x columns [32 * blockIdx.x, +32)
template <int MODE>
__global__ __launch_bounds__(64) void tr_gemm_kernel(TrGemm P) {
    const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const int n = n0 + c;
    f32x16 acc;
    const float init = (MODE == TR_FWD && n < P.N) ? P.bias[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = init;
    const int nch = (P.K + 31) >> 5;
    float a[16], b[16];
    tr_load(P.A, P.a_sm, P.a_sk, m0 + c, P.M, P.K, 0, h, P.relu_a, a);
    tr_load(P.B, P.b_sn, P.b_sk, n, P.N, P.K, 0, h, P.relu_b, b);
    for (int ch = 0; ch < nch; ++ch) {
        // the next chunk is requested before this chunk's MFMAs (past the end: zeros, no load)
        float an[16], bn[16];
        tr_load(P.A, P.a_sm, P.a_sk, m0 + c, P.M, P.K, ch + 1, h, P.relu_a, an);
        tr_load(P.B, P.b_sn, P.b_sk, n, P.N, P.K, ch + 1, h, P.relu_b, bn);
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 16; ++s) { a[s] = an[s]; b[s] = bn[s]; }
    }
    // outputs: row m0 + acc_row(r, h), column n
    if (n < P.N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + acc_row(r, h);
            if (m >= P.M) continue;
            const size_t at = (size_t)m * P.N + n;
            if (MODE == TR_FWD) P.out[at] = acc[r];
            else if (MODE == TR_DA) P.out[at] = P.zprev[at] > 0.0f ? acc[r] : 0.0f;
            else {
                float w = P.W[at], mm = P.mW[at], vv = P.vW[at];
                tr_adam(acc[r], w, mm, vv, P.step, P.r2);
                P.W[at] = w; P.mW[at] = mm; P.vW[at] = vv;
            }
        }
    }
    if (MODE == TR_DW && blockIdx.x == 0) {
        // db[o] = the chain acc = acc + g[r][o] from +0, r ascending: one lane per o of this tile's rows
        const int o = m0 + c;
        if (h == 0 && o < P.M) {
            float db = 0.0f;
            for (int r = 0; r < P.K; ++r) db = db + P.g[(size_t)r * P.M + o];
            float bb = P.b[o], mm = P.mb[o], vv = P.vb[o];
            tr_adam(db, bb, mm, vv, P.step, P.r2);
            P.b[o] = bb; P.mb[o] = mm; P.vb[o] = vv;
        }
        if (blockIdx.y == 0 && lane == 0 && P.loss) {
            double s = 0.0;
            for (int r = 0; r < P.K; ++r) s += (double)P.lrow[r];
            *P.loss = (float)(s / (double)P.K);
        }
    }
}

// p = lmi_mlp_proba's softmax of a row of logits (softmax_ranked_kernel: the maximum by `v > m ? v : m` from l[0], lmi_expf, the row
// sum as ONE chain of adds in class order, one division), g[r][c] = (p - [c == y_r]) * inv_b, lrow[r] = -logf(p[y_r]).
// One wave per row: grid B, block 64.
__global__ __launch_bounds__(64) void tr_softmax_grad_kernel(const float* __restrict__ logits, const int* __restrict__ y, int L, float inv_b,
                                                            float* __restrict__ g, float* __restrict__ lrow) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* l = logits + (size_t)r * L;
    float m = l[0];
    for (int j = lane; j < L; j += 64) {
        const float v = l[j];
        m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(m, o);
        m = ov > m ? ov : m;
    }
    float s = 0.0f;
    for (int j0 = 0; j0 < L; j0 += 64) {
        const int j = j0 + lane;
        const float e = j < L ? lmi_expf(l[j] - m) : 0.0f;   // past L: +0, which leaves the non-negative sum as it is
#pragma unroll
        for (int k = 0; k < 64; ++k) s += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), k));
    }
    const int yr = y[r];
    for (int j = lane; j < L; j += 64) {
        const float p = lmi_expf(l[j] - m) / s;
        g[(size_t)r * L + j] = (p - (j == yr ? 1.0f : 0.0f)) * inv_b;
        if (j == yr && lrow) lrow[r] = -logf(p);
    }
}

// xb[j][:] = x[rows[j]][:], yb[j] = labels[rows[j]] for the j-th named row; *bad becomes 1 when a label is outside [0, classes).
// Grid-stride over (row, dimension).
__global__ void tr_gather_kernel(const float* __restrict__ x, const int* __restrict__ labels, const long long* __restrict__ rows,
                                 long long n_rows, int d, int classes, float* __restrict__ xb, int* __restrict__ yb, int* __restrict__ bad) {
    const long long total = n_rows * d, stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long j = i / d;
        const int t = (int)(i - j * d);
        const long long src = rows[j];
        xb[i] = x[(size_t)src * d + t];
        if (t == 0) {
            const int lab = labels[src];
            yb[j] = lab;
            if (lab < 0 || lab >= classes) atomicOr(bad, 1);
        }
    }
}

// tr_gather_kernel on rows of halves (lmi_train_f16): xb[j][:] = the named row widened exactly; the label check is the same
__global__ void tr_gather16_kernel(const unsigned short* __restrict__ x, const int* __restrict__ labels, const long long* __restrict__ rows,
                                   long long n_rows, int d, int classes, float* __restrict__ xb, int* __restrict__ yb,
                                   int* __restrict__ bad) {
    const long long total = n_rows * d, stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long j = i / d;
        const int t = (int)(i - j * d);
        const long long src = rows[j];
        xb[i] = (float)__builtin_bit_cast(_Float16, x[(size_t)src * d + t]);
        if (t == 0) {
            const int lab = labels[src];
            yb[j] = lab;
            if (lab < 0 || lab >= classes) atomicOr(bad, 1);
        }
    }
}

}  // namespace lmi
