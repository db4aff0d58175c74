// lmi_project.h -- device code of lmi_project: y = (x - mean) . basis^T, every element one unsplit chain (include/lmi_hip.h states the
// arithmetic).
//
// project_kernel is the streamed product of lmi_dense.h: Y^T = B . C^T by v_mfma_f32_32x32x2_f32, A = the basis rows in fragment order
// (dense_pack_kernel, link d and the links behind it zero), B = rows of x straight from the row-major array (dense_load_b, either
// form), the loop knn_score_kernel's (the loops are kept equal: lmi_dense.h) with two additions:
//  - the mean, padded with zeros to the chain's length, lies in LDS in the order the lanes consume it (PJ_MEAN below) and is
//    subtracted from bv after dense_load_b's permlane trade: c = x - mean in binary32, one rounding, in the register that feeds the
//    MFMA.  No mean: the LDS holds +0 and x - (+0) = x, bit for bit.
//  - the output leaves through an LDS transpose.  In the accumulator a lane holds ONE row of x and 16 basis rows of a tile: sixteen
//    stores m floats apart.  Each wave instead writes a (32 rows x 32 basis rows) tile to its own LDS square and reads it back row by
//    row: eight lanes write a row's 128 contiguous bytes as 16-byte stores (m % 4 == 0 and y 16-byte aligned; 4-byte stores, still
//    contiguous along a row, otherwise).
// T = float or unsigned short (lmi_project_f16: halves widened where dense_load_b loads them).
#pragma once
#include "lmi_dense.h"

namespace lmi {

constexpr int PJ_XB = 2;                    // 32-row blocks of x per wave
constexpr int PJ_ROWS = 4 * PJ_XB * 32;     // rows of x per workgroup (4 waves)
constexpr int PJ_TW = 36;                   // floats per row of a wave's transpose square: 32 + 4 keeps the rows 16-byte aligned

// PJ_MEAN: out[(ch * 2 + h) * 16 + s] = mean[32 * ch + 2 * s + h] (0 at and past d, everywhere when mean is null) -- the 16 values
// lane half h subtracts in chunk ch, contiguous.  links = the chain's padded length, a multiple of 32; one thread per link.
__global__ void project_mean_kernel(const float* __restrict__ mean, int d, int links, float* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= links) return;
    const int ch = t >> 5, s = (t & 31) >> 1, h = t & 1;
    out[(ch * 2 + h) * 16 + s] = mean && t < d ? mean[t] : 0.0f;
}

// grid (cdiv(n, PJ_ROWS), cdiv(nct, CT)), block 256, dynamic LDS KG * 32 bytes (the mean in PJ_MEAN order): wave w -> rows
// [(blockIdx.x * 4 + w) * 64, +64) of x [n][d] as PJ_XB column blocks, against the basis tiles [blockIdx.y * CT, +CT).
// Bf [nct][KG][64], KG a multiple of 4; ml [KG * 8] in PJ_MEAN order.  y[row * m + j] <- the chain, row < n, j < m.
template <class T, int CT, bool VEC>
__global__ __launch_bounds__(256) void project_kernel(const T* __restrict__ x, long long n, int d, const float* __restrict__ ml,
                                                      const float4* __restrict__ Bf, int KG, int nct, int m, float* __restrict__ y,
                                                      int vec_out) {
    extern __shared__ float pj_mean[];
    __shared__ __attribute__((aligned(16))) float pj_sq[4][32][PJ_TW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    for (int t = threadIdx.x; t < KG * 8; t += 256) pj_mean[t] = ml[t];
    __syncthreads();
    const long long row0 = ((long long)blockIdx.x * 4 + w) * (PJ_XB * 32);
    if (row0 >= n) return;   // (behind the block's only barrier)
    const int ct0 = blockIdx.y * CT;
    const T* xr[PJ_XB];
#pragma unroll
    for (int b = 0; b < PJ_XB; ++b) {
        const long long r = row0 + b * 32 + c;
        xr[b] = x + (size_t)(r < n ? r : n - 1) * d;   // clamp: duplicates are computed and not written
    }
    const int nch = KG >> 2;
    f32x16 acc[CT][PJ_XB];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int b = 0; b < PJ_XB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][b][r] = 0.0f;
    const float4* ap[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) ap[t] = Bf + (size_t)(ct0 + t < nct ? ct0 + t : nct - 1) * KG * 64 + lane;
    float bv[PJ_XB][16];
#pragma unroll
    for (int b = 0; b < PJ_XB; ++b) dense_load_b<VEC>(xr[b], d, 0, h, 0.0f, bv[b]);
    float4 a[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) a[t] = ap[t][0];
    for (int ch = 0; ch < nch; ++ch) {
        // the next chunk's rows are requested before this chunk's MFMAs (the last chunk reads itself again)
        float bn[PJ_XB][16];
        const int chn = ch + 1 < nch ? ch + 1 : ch;
#pragma unroll
        for (int b = 0; b < PJ_XB; ++b) dense_load_b<VEC>(xr[b], d, chn, h, 0.0f, bn[b]);
        // this chunk's 16 means of this lane half, then c = x - mean
        const float4* mq = reinterpret_cast<const float4*>(pj_mean + (ch * 2 + h) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 mv = mq[q];
#pragma unroll
            for (int b = 0; b < PJ_XB; ++b) {
                bv[b][4 * q] -= mv.x; bv[b][4 * q + 1] -= mv.y; bv[b][4 * q + 2] -= mv.z; bv[b][4 * q + 3] -= mv.w;
            }
        }
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
                    for (int b = 0; b < PJ_XB; ++b)
                        acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[b][4 * g + s], acc[t][b], 0, 0, 0);
                }
#pragma unroll
            for (int t = 0; t < CT; ++t) a[t] = an[t];
        }
#pragma unroll
        for (int b = 0; b < PJ_XB; ++b)
#pragma unroll
            for (int s = 0; s < 16; ++s) bv[b][s] = bn[b][s];
    }
    // the transpose: sq[row of x][basis row of the tile], written as this lane's four runs of four accumulator rows, read back by rows
    float(*sq)[PJ_TW] = pj_sq[w];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        if (ct0 + t >= nct) continue;   // uniform
        const int j0 = (ct0 + t) * 32;
#pragma unroll
        for (int b = 0; b < PJ_XB; ++b) {
#pragma unroll
            for (int q = 0; q < 4; ++q)   // acc_row(4q .. 4q+3, h) = 8q + 4h .. + 3
                *reinterpret_cast<float4*>(&sq[c][8 * q + 4 * h]) =
                    make_float4(acc[t][b][4 * q], acc[t][b][4 * q + 1], acc[t][b][4 * q + 2], acc[t][b][4 * q + 3]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const long long rb = row0 + b * 32;
            if (vec_out) {
#pragma unroll
                for (int pass = 0; pass < 4; ++pass) {
                    const int r = pass * 8 + (lane >> 3), j = j0 + 4 * (lane & 7);
                    if (rb + r < n && j < m) *reinterpret_cast<float4*>(y + (size_t)(rb + r) * m + j) = *reinterpret_cast<const float4*>(&sq[r][4 * (lane & 7)]);
                }
            } else {
#pragma unroll
                for (int pass = 0; pass < 16; ++pass) {
                    const int r = pass * 2 + h, j = j0 + c;
                    if (rb + r < n && j < m) y[(size_t)(rb + r) * m + j] = sq[r][c];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

}  // namespace lmi
