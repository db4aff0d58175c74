// lmi_knn_rerank.h -- device code of lmi_knn_rerank: the exact top k among per-query candidate rows (include/lmi_hip.h states the
// contract).  Per (query, candidate) one dot product over a row gathered from a random address: nothing is shared
// between queries, no MFMA fits, and the bound is the gather -- the kernel is built to keep bytes in flight.
//
// Scores (rerank_score_kernel): a wave owns 64 consecutive positions of one query's list; lane j owns candidate j and its accumulator
// (L2: two, s and xn).
//   gather       a row is contiguous, so the wave reads cooperatively, a chunk of RR_T = 32 floats per row at a time: in the VEC form
//                8 adjacent lanes fetch one row's 128 bytes with one 16-byte load each (8 instructions cover the 64 rows), in the dword
//                form 32 adjacent lanes fetch them word by word (32 instructions).  Every instruction covers whole 128-byte stretches.
//   tile         the chunk lands in the wave's own LDS tile of 64 rows at the odd pitch of RR_T + 1 floats (hamming_score_kernel's
//                trick): when lane j then reads word t of row j, the 64 lanes fall into 64 different banks.
//   look-ahead   the next chunk's global loads are issued into 32 registers before the current chunk's FMAs; the tile is written from
//                registers only and read by its own wave only, so there is no barrier: LDS operations of one wave stay in order.
//                A block of 4 waves holds 4 * 64 * 33 * 4 = 33 792 bytes of tiles (+ 2 KiB of row offsets): four blocks per compute
//                unit inside the 160 KiB, 16 waves with 8 KiB in registers and 8 KiB in LDS each.
//   query        is uniform over the wave (the wave's number goes through readfirstlane) and is read through SCALAR LOADS of the
//                const __restrict__ pointer: the FMA takes the SGPR as its operand, so the query costs no VGPR, no LDS read and no
//                vector instruction.  Results leave in vector stores only.
//   chain        per element exactly one v_fmac_f32 (L2: two) in ascending t: acc = fmaf(q[t], x[t], acc) from +0, never split.
//   edges        a lane without a candidate of its own (cand == -1, a position >= c, a row outside the piece) loads the row of the
//                wave's first valid lane and writes nothing; a wave with no valid lane leaves after one ballot; the words past d of
//                the last chunk are neither loaded nor multiplied.
// rerank_qnorm_kernel (L2 only): qn[q] by the same chain.  rerank_sort_kernel: one wave per query sorts the query's list in LDS
// (knn_bitonic_sort_up, read backwards) and writes D and I with knn_merge_kernel's epilogue.  rerank_check_kernel counts the candidates
// outside [-1, nb) before anything is scored.  lmi_knn.h is used as it is.
#pragma once
#include "lmi_knn.h"

namespace lmi {

constexpr int RR_T = 32;             // floats of a row per chunk
constexpr int RR_PITCH = RR_T + 1;   // floats between two rows of a wave's tile: odd
constexpr int RR_WAVES = 4;          // waves per block, each with a tile of its own

// entries of a query's list: max(128, c rounded up to a power of two) -- what knn_bitonic_sort_up takes
inline int rerank_list_rows(int c) {
    int p = 128;
    while (p < c) p <<= 1;
    return p;
}

// bad <- += the entries of cand [n] outside [-1, nb)
__global__ void rerank_check_kernel(const long long* __restrict__ cand, long long n, long long nb, unsigned long long* __restrict__ bad) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned cnt = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) cnt += cand[i] < -1 || cand[i] >= nb;
    if (cnt) atomicAdd(bad, (unsigned long long)cnt);
}

// qn[i] <- the chain fmaf(q[i][t], q[i][t], acc) from +0, i < nq
__global__ void rerank_qnorm_kernel(const float* __restrict__ q, int nq, int d, float* __restrict__ qn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const float* r = q + (size_t)i * d;
    float acc = 0.0f;
    for (int t = 0; t < d; ++t) acc = __builtin_fmaf(r[t], r[t], acc);
    qn[i] = acc;
}

// words [t0, t0 + RR_T) of the 64 rows at x + offs[r] into r[]: VEC: r[4 i ..] = four words at column (lane & 7) * 4 of row
// i * 8 + lane / 8; dword form: r[i] = the word at column lane & 31 of row i * 2 + lane / 32.  Columns >= d are not read.
template <bool VEC>
__device__ __forceinline__ void rerank_load_chunk(const float* __restrict__ x, const long long* offs, int lane, int t0, int d,
                                                  float (&r)[RR_T]) {
    if constexpr (VEC) {   // d % 4 == 0: a 16-byte word is inside the row or past it as a whole
        const int col = t0 + (lane & 7) * 4;
#pragma unroll
        for (int i = 0; i < RR_T / 4; ++i) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (col < d) v = *reinterpret_cast<const float4*>(x + offs[i * 8 + (lane >> 3)] + col);
            r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
        }
    } else {
        const int col = t0 + (lane & 31);
#pragma unroll
        for (int i = 0; i < RR_T; ++i) r[i] = col < d ? x[offs[i * 2 + (lane >> 5)] + col] : 0.0f;
    }
}
// r[] into the tile, each word at [row * RR_PITCH + column of the chunk]
template <bool VEC>
__device__ __forceinline__ void rerank_store_chunk(float* tile, int lane, const float (&r)[RR_T]) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < RR_T / 4; ++i) {
            float* dst = tile + (i * 8 + (lane >> 3)) * RR_PITCH + (lane & 7) * 4;
            dst[0] = r[4 * i]; dst[1] = r[4 * i + 1]; dst[2] = r[4 * i + 2]; dst[3] = r[4 * i + 3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < RR_T; ++i) tile[(i * 2 + (lane >> 5)) * RR_PITCH + (lane & 31)] = r[i];
    }
}

// grid cdiv(nq * cdiv(c, 64), RR_WAVES), block 64 * RR_WAVES.  Wave g = blockIdx.x * RR_WAVES + its number in the block owns the
// positions [64 * (g % wpq), +64) of query g / wpq, wpq = cdiv(c, 64).  x [len][d]: the rows [r0, r0 + len) of the base; a candidate
// outside them (or -1) is not scored here.  lists[q * LR + position] <- knn_make(score, row of the base) where score > -FLT_MAX; the
// slot is left as it is otherwise.  VEC: d % 4 == 0 and x 16-byte aligned; q and x need 4-byte alignment only otherwise.
template <bool VEC, bool L2>
__global__ __launch_bounds__(64 * RR_WAVES) void rerank_score_kernel(const float* __restrict__ x, long long r0, long long len, int d,
                                                                     const float* __restrict__ q, int nq,
                                                                     const long long* __restrict__ cand, int c, int LR,
                                                                     knn_entry* __restrict__ lists) {
    __shared__ float rr_tiles[RR_WAVES][64 * RR_PITCH];
    __shared__ long long rr_offs[RR_WAVES][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wpq = (c + 63) >> 6;
    const long long g = (long long)blockIdx.x * RR_WAVES + w;
    const int qi = (int)(g / wpq), pos = (int)(g % wpq) * 64 + lane;   // qi is uniform
    if (qi >= nq) return;
    const long long row = pos < c ? cand[(size_t)qi * c + pos] - r0 : -1;
    const bool valid = row >= 0 && row < len;
    const unsigned long long m = __ballot(valid);
    if (!m) return;   // uniform: none of the 64 candidates is a row of this piece
    float* tile = rr_tiles[w];
    long long* offs = rr_offs[w];
    offs[lane] = (valid ? row : __shfl(row, __ffsll(m) - 1)) * d;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const float* qr = q + (size_t)qi * d;
    const float* mine = tile + lane * RR_PITCH;
    float s = 0.0f, xn = 0.0f;
    float cur[RR_T];
    rerank_load_chunk<VEC>(x, offs, lane, 0, d, cur);
#pragma unroll 1
    for (int t0 = 0; t0 < d; t0 += RR_T) {
        // the words of this chunk go from the registers into the tile; the reads of the chunk before are done: one wave, in order
        rerank_store_chunk<VEC>(tile, lane, cur);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the next chunk is requested before this chunk's FMAs
        if (t0 + RR_T < d) rerank_load_chunk<VEC>(x, offs, lane, t0 + RR_T, d, cur);
        const float* qc = qr + t0;
        if (t0 + RR_T <= d) {
#pragma unroll
            for (int u = 0; u < RR_T; ++u) {
                const float xv = mine[u];
                s = __builtin_fmaf(qc[u], xv, s);
                if constexpr (L2) xn = __builtin_fmaf(xv, xv, xn);
            }
        } else {
#pragma unroll 1
            for (int u = 0; u < d - t0; ++u) {
                const float xv = mine[u];
                s = __builtin_fmaf(qc[u], xv, s);
                if constexpr (L2) xn = __builtin_fmaf(xv, xv, xn);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // L2: the link at d; then the link lmi_knn's padding to 32 adds where the chain's length is no multiple of 32: -0 becomes +0
    if constexpr (L2) s = __builtin_fmaf(1.0f, -0.5f * xn, s);
    if ((d + (L2 ? 1 : 0)) % 32) s = __builtin_fmaf(0.0f, 0.0f, s);
    if (valid && s > -FLT_MAX) lists[(size_t)qi * LR + pos] = knn_make(s, (unsigned)(row + r0));
}

// grid nq, block 64, dynamic LDS LR entries: sorts the LR entries of query q's list (LR a power of two >= 128) and writes D[q][k],
// I[q][k] -- the first k in the total order; an empty slot pads with I = -1 and D = -FLT_MAX (L2: FLT_MAX).  qn: L2 only,
// D = fmaf(-2, key, qn[q]): knn_merge_kernel's epilogue.
__global__ __launch_bounds__(64) void rerank_sort_kernel(const knn_entry* __restrict__ lists, int LR, int k, const float* __restrict__ qn,
                                                         float* __restrict__ D, long long* __restrict__ I) {
    extern __shared__ knn_entry knn_lds[];
    const int lane = threadIdx.x, q = blockIdx.x;
    for (int i = lane; i < LR; i += 64) knn_lds[i] = lists[(size_t)q * LR + i];
    __syncthreads();
    knn_bitonic_sort_up(knn_lds, LR, lane);   // worst-first: read from the end
    for (int j = lane; j < k; j += 64) {
        const knn_entry e = knn_lds[LR - 1 - j];
        const bool empty = knn_row(e) == 0xffffffffu;
        const float key = knn_score(e);
        D[(size_t)q * k + j] = empty ? (qn ? FLT_MAX : -FLT_MAX) : qn ? __builtin_fmaf(-2.0f, key, qn[q]) : key;
        I[(size_t)q * k + j] = empty ? -1ll : (long long)knn_row(e);
    }
}

}  // namespace lmi
