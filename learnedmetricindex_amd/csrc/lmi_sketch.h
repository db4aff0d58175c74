// lmi_sketch.h -- device code of lmi_sketch: bit j of row i = [ y[i][j] > thresh[j] ], y = (x - mean) . basis^T as lmi_project writes
// it, packed 32 bits to a word (include/lmi_hip.h states the contract).
//
// sketch_kernel runs project_kernel's product -- the streamed v_mfma_f32_32x32x2_f32 product of lmi_dense.h, A = the basis rows in
// fragment order (dense_pack_kernel), B = rows of x by dense_load_b in either form, the mean in LDS in PJ_MEAN order and subtracted in
// the register that feeds the MFMA; the K loop is project_kernel's, statement for statement (lmi_dense.h: the loops are kept equal),
// so an accumulator holds the bits lmi_project would store -- and then no float leaves the lane:
//  - in the accumulator a lane (h, c) holds ONE row of x (c) and 16 of a tile's 32 basis rows: register r = 4q + i is basis row
//    8q + 4h + i.  The tile's thresholds lie in LDS behind the mean in that order (SK_THRESH below): four 16-byte reads give the lane
//    its 16, it compares (ordered greater-than: a NaN on either side is 0) and sets bit 8q + 4h + i of a word.
//  - a wave holds two 32-row blocks of x, so a lane holds two such half words, hw[0] and hw[1].  One v_permlane32_swap of the pair
//    gives lane half 0 both halves of block 0's word and lane half 1 both halves of block 1's: an OR completes the word for (row of x,
//    basis tile) in a register, and all 64 lanes hold a row to store.
//  - with CT tiles per wave the lane then holds CT consecutive words of its code row: one 16-byte store at CT = 4 (m % 128 == 0 and
//    codes 16-byte aligned), 4-byte stores otherwise.  No LDS transpose, no second pass.
// Work split: the block index is (row block, column group) with the column group the FAST part, so the groups of one row block are
// dispatched back to back and all but the first read of the block's rows of x hit L2; with G = 1 the block walks its column groups
// itself instead (the same kernel: the group loop below strides by G).  profiles/sketch.txt holds both measurements.
// T = float or unsigned short (lmi_sketch_f16: halves widened where dense_load_b loads them).
#pragma once
#include "lmi_project.h"   // PJ_XB, PJ_ROWS, the PJ_MEAN order and project_mean_kernel

namespace lmi {

// SK_THRESH: out[(tile * 2 + h) * 16 + 4 * q + i] = thresh[32 * tile + 8 * q + 4 * h + i] (+0 everywhere when thresh is null) -- the 16
// values lane half h compares its accumulator registers 0..15 of a tile with, contiguous.  m a multiple of 32; one thread per bit.
__global__ void sketch_thresh_kernel(const float* __restrict__ thresh, int m, float* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int tile = t >> 5, q = (t >> 3) & 3, h = (t >> 2) & 1, i = t & 3;
    out[(tile * 2 + h) * 16 + 4 * q + i] = thresh ? thresh[t] : 0.0f;
}

// grid cdiv(n, PJ_ROWS) * G, block 256, dynamic LDS KG * 32 + nct * 128 bytes (the mean in PJ_MEAN order, then the thresholds in
// SK_THRESH order): block -> row block blockIdx.x / G, column groups blockIdx.x % G, + G, .. below cdiv(nct, CT); wave w -> rows
// [(row block * 4 + w) * 64, +64) of x [n][d] as PJ_XB column blocks against the basis tiles [group * CT, +CT).
// Bf [nct][KG][64], KG a multiple of 4; ml [KG * 8]; tl [nct * 32].  codes [n][nct] words: word (row, tile) <- the 32 comparisons,
// row < n, tile < nct.
// Two blocks per compute unit (two waves per SIMD, as project_kernel runs): without the bound the CT = 4 forms take 178 VGPRs beside
// their 128 accumulator registers and run one wave per SIMD; with it they fit 256 unified registers, no scratch.
template <class T, int CT, bool VEC>
__global__ __launch_bounds__(256, 2) void sketch_kernel(const T* __restrict__ x, long long n, int d, const float* __restrict__ ml,
                                                     const float* __restrict__ tl, const float4* __restrict__ Bf, int KG, int nct,
                                                     int G, unsigned* __restrict__ codes, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) float sk_lds[];
    float* const pj_mean = sk_lds;
    float* const sk_th = sk_lds + KG * 8;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    for (int t = threadIdx.x; t < KG * 8; t += 256) pj_mean[t] = ml[t];
    for (int t = threadIdx.x; t < nct * 32; t += 256) sk_th[t] = tl[t];
    __syncthreads();
    const long long row0 = ((long long)(blockIdx.x / G) * 4 + w) * (PJ_XB * 32);
    if (row0 >= n) return;   // (behind the block's only barrier)
    const T* xr[PJ_XB];
#pragma unroll
    for (int b = 0; b < PJ_XB; ++b) {
        const long long r = row0 + b * 32 + c;
        xr[b] = x + (size_t)(r < n ? r : n - 1) * d;   // clamp: duplicates are computed and not written
    }
    const long long orow = row0 + lane;   // the row whose words this lane stores: block h, column c
    const int nch = KG >> 2;
    for (int ct0 = (int)(blockIdx.x % G) * CT; ct0 < nct; ct0 += G * CT) {
        // the row pointers are made opaque per group: the first chunk's loads of x do not depend on the group and would otherwise be
        // hoisted out of this loop and held across it (24 VGPRs more in the CT = 4 float form)
#pragma unroll
        for (int b = 0; b < PJ_XB; ++b) asm volatile("" : "+v"(xr[b]));
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
        // compare, place, trade: wd[t] = the word of (row orow, tile ct0 + t)
        unsigned wd[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const float4* tq = reinterpret_cast<const float4*>(sk_th + ((ct0 + t < nct ? ct0 + t : nct - 1) * 2 + h) * 16);
            unsigned hw[PJ_XB];
#pragma unroll
            for (int b = 0; b < PJ_XB; ++b) hw[b] = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {   // acc_row(4q .. 4q+3, h) = 8q + 4h .. + 3: bits 8q .. 8q+3 here, shifted by 4h below
                const float4 tv = tq[q];
#pragma unroll
                for (int b = 0; b < PJ_XB; ++b)
                    hw[b] |= (unsigned)(acc[t][b][4 * q] > tv.x) << (8 * q) | (unsigned)(acc[t][b][4 * q + 1] > tv.y) << (8 * q + 1) |
                             (unsigned)(acc[t][b][4 * q + 2] > tv.z) << (8 * q + 2) | (unsigned)(acc[t][b][4 * q + 3] > tv.w) << (8 * q + 3);
            }
            // lanes 32..63 of hw[0] (block 0, basis rows 8q+4..7) <-> lanes 0..31 of hw[1] (block 1, basis rows 8q..3): then lane half
            // 0 holds both halves of block 0's word of row c and lane half 1 both halves of block 1's
            const auto sw = __builtin_amdgcn_permlane32_swap(hw[0] << (4 * h), hw[1] << (4 * h), false, false);
            wd[t] = sw[0] | sw[1];
        }
        if (orow < n) {
            unsigned* out = codes + (size_t)orow * nct + ct0;
            if (CT == 4 && vec_out && ct0 + 4 <= nct) {
                // written once and not read again by this call: a non-temporal store (which also keeps the compiler from folding
                // this store into the 4-byte ones below, at their alignment)
                typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
                const u32x4v v = {wd[0], wd[CT > 1 ? 1 : 0], wd[CT > 2 ? 2 : 0], wd[CT > 3 ? 3 : 0]};
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4v*>(out));
            } else {
#pragma unroll
                for (int t = 0; t < CT; ++t)
                    if (ct0 + t < nct) out[t] = wd[t];
            }
        }
    }
}

}  // namespace lmi
