// lmi_knn_hamming.h -- device code of lmi_knn_hamming: exact Hamming k-NN on bit-packed codes (include/lmi_hip.h states the contract;
// DESIGN.md 5.13.3).  A code is W = code_bytes / 4 dwords; dist(q, x) = the bits set in q ^ x, an integer <= 32 W <= 4096.
//
// Scores (hamming_score_kernel): S[q * pitch + row] = -(float)dist into the slab knn_score_kernel writes -- the distances are exact in
// binary32 and the negation makes "score descending, row ascending" the required order, so everything behind the slab is lmi_knn's,
// unchanged: knn_fill_kernel, knn_select_kernel, the lists.  No MFMA and no float chain: v_xor_b32 and v_bcnt_u32_b32 on the vector
// ALU, two operations per pair of dwords, accumulated as integers.
//   row tile     a block of 256 threads owns 256 consecutive rows of the piece: one contiguous stretch of 256 W dwords, loaded
//                coalesced (16-byte loads in the VEC form) into LDS at a row pitch of W | 1 dwords -- odd, so the 64 lanes of a wave,
//                each reading the same word of its own row, fall into 64 different banks.  The whole tile is resident: the largest
//                code (W = 128) takes 256 * 129 * 4 = 132 096 bytes of the 160 KiB.
//   accumulators a lane owns one row and keeps HAM_TQ = 32 integer accumulators in VGPRs, one per query of the current query tile.
//                Per chunk of 8 words it reads its row's words from LDS once, then does 8 x (xor, bit count + add) for each of
//                the 32 queries: 8 ds_read_b32 per 512 vector-ALU operations.
//   query words  are uniform over the wave and are taken through SCALAR LOADS of the const __restrict__ query pointer at a uniform
//                index (s_load_dwordx8 per query and chunk): the XOR takes the SGPR as its operand, so the query side costs no
//                vector instruction, no LDS bandwidth and no VGPR; an LDS broadcast would put one ds_read beside every 2 to 8 vector
//                operations.  Nothing is written through the scalar unit: results leave in vector stores only.
//   query tiles  a block walks `tps` query tiles against its resident row tile (grid.y cuts the group's tiles into shares), which
//                amortises the tile load and keeps the piece's re-reads in L2.  Per query a wave writes 64 consecutive floats.
//   edges        rows past the piece's end compute on whatever the LDS holds and do not write; queries past the group's end are
//                read as the group's last query and skipped at the store; W % 8 words go through a 4-word and 1-word chunk.
// knn_merge_hamming_kernel: knn_merge_kernel with an integer epilogue; a kernel of its own so that knn_merge_kernel keeps its
// instructions (the precedent: knn_score16_kernel).
#pragma once
#include "lmi_knn.h"
#include <climits>

namespace lmi {

constexpr int HAM_ROWS = 256;      // rows of the base per workgroup: one per lane
constexpr int HAM_TQ = 32;         // queries per tile: accumulators per lane
constexpr int HAM_MAX_WORDS = 128; // 4096 bits

// dwords between two rows of the tile in LDS, and the tile's bytes
__host__ __device__ constexpr int ham_pitch(int W) { return W | 1; }
inline size_t ham_lds_bytes(int W) { return (size_t)HAM_ROWS * ham_pitch(W) * sizeof(unsigned); }

// acc += the bits set in v, in one instruction.  (Written as acc += __popc(v), the sums of a chunk are re-associated into
// v_bcnt_u32_b32 v, v, 0 and a tree of v_add3_u32: 20 vector operations per 8 words instead of 16.)
__device__ __forceinline__ void ham_bcnt_acc(int& acc, unsigned v) { asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(v)); }

// acc[j] += bits of (row[0 .. CW) ^ words [0 .. CW) of query min(j, jmax) of the tile at q), j < HAM_TQ; q and jmax are uniform
template <int CW>
__device__ __forceinline__ void ham_chunk(const unsigned* row, const unsigned* __restrict__ q, int W, int jmax, int (&acc)[HAM_TQ]) {
    unsigned r[CW];
#pragma unroll
    for (int u = 0; u < CW; ++u) r[u] = row[u];
#pragma unroll
    for (int j = 0; j < HAM_TQ; ++j) {
        const unsigned* qj = q + (size_t)(j < jmax ? j : jmax) * W;
#pragma unroll
        for (int u = 0; u < CW; ++u) ham_bcnt_acc(acc[j], r[u] ^ qj[u]);
    }
}

// grid (cdiv(n, HAM_ROWS), cdiv(nct, tps)), block 256, dynamic LDS ham_lds_bytes(W): rows [blockIdx.x * 256, +256) of the piece
// x [n][W] against the query tiles [blockIdx.y * tps, +tps) of q [nq][W], nct = cdiv(nq, 32).  S[qi * pitch + row] <- -(float)dist,
// qi < nq, row < n.  VEC: W % 4 == 0 and x 16-byte aligned; q needs 4-byte alignment only.
template <bool VEC>
__global__ __launch_bounds__(256) void hamming_score_kernel(const unsigned* __restrict__ x, long long n, int W,
                                                            const unsigned* __restrict__ q, int nq, int nct, int tps,
                                                            float* __restrict__ S, long long pitch) {
    extern __shared__ unsigned ham_lds[];
    const int t = threadIdx.x, P = ham_pitch(W);
    const long long row0 = (long long)blockIdx.x * HAM_ROWS;
    const int rows = (int)(n - row0 < HAM_ROWS ? n - row0 : HAM_ROWS);
    const unsigned* src = x + (size_t)row0 * W;
    const int total = rows * W;   // dwords of the tile: at most 256 * 128
    {   // dword i of the stretch -> (row i / W, word i % W), kept by increments: a thread's next element is STEP dwords on
        constexpr int STEP = VEC ? 1024 : 256;
        const int i0 = VEC ? t * 4 : t, dr = STEP / W, dc = STEP % W;
        int r = i0 / W, c = i0 % W;
        for (int i = i0; i < total; i += STEP) {
            unsigned* dst = ham_lds + r * P + c;
            if constexpr (VEC) {   // W % 4 == 0: the four dwords are of one row
                const uint4 v = *reinterpret_cast<const uint4*>(src + i);
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            } else {
                dst[0] = src[i];
            }
            r += dr;
            c += dc;
            if (c >= W) { c -= W; ++r; }
        }
    }
    __syncthreads();
    const unsigned* mine = ham_lds + t * P;
    const long long row = row0 + t;
    const int ct1 = (blockIdx.y + 1) * tps < nct ? (blockIdx.y + 1) * tps : nct;
#pragma unroll 1
    for (int ct = blockIdx.y * tps; ct < ct1; ++ct) {
        const int q0 = ct * HAM_TQ, jmax = nq - 1 - q0 < HAM_TQ - 1 ? nq - 1 - q0 : HAM_TQ - 1;
        const unsigned* qt = q + (size_t)q0 * W;
        int acc[HAM_TQ];
#pragma unroll
        for (int j = 0; j < HAM_TQ; ++j) acc[j] = 0;
        int w = 0;
#pragma unroll 1
        for (; w + 8 <= W; w += 8) ham_chunk<8>(mine + w, qt + w, W, jmax, acc);
        if (w + 4 <= W) {
            ham_chunk<4>(mine + w, qt + w, W, jmax, acc);
            w += 4;
        }
#pragma unroll 1
        for (; w < W; ++w) ham_chunk<1>(mine + w, qt + w, W, jmax, acc);
        if (row < n) {
            float* out = S + (size_t)q0 * pitch + row;
#pragma unroll
            for (int j = 0; j < HAM_TQ; ++j)
                if (j <= jmax) out[(size_t)j * pitch] = -(float)acc[j];
        }
    }
}

// grid nq, block 64, dynamic LDS 2 * LR entries: knn_merge_kernel's merge of the `splits` lists of query q, then D[q][k] =
// (int)(-score) -- the distance, exact -- and I[q][k]; an empty slot pads with I = -1 and D = INT32_MAX.
__global__ __launch_bounds__(64) void knn_merge_hamming_kernel(const knn_entry* __restrict__ lists, int splits, int LR, int k,
                                                               int* __restrict__ D, long long* __restrict__ I) {
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
        D[(size_t)q * k + j] = empty ? INT_MAX : (int)(-knn_score(e));
        I[(size_t)q * k + j] = empty ? -1ll : (long long)knn_row(e);
    }
}

}  // namespace lmi
