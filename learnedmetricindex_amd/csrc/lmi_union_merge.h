// lmi_union_merge.h -- device code of lmi_merge_union_parts / lmi_allgather_merge_union: the merge of the ranks' parts of a union scan
// (lmi_scan_union_part; include/lmi_hip.h states the order).
//
// A part is [LMI_UNION_PART_PLANES][nq][k] int32 words: score bits, dist bits, id, rank, row per result, best first, padding behind.
// The order is (score descending with -0 == +0, rank ascending, row ascending, part ascending): the single handle's (score, ordinal)
// order, since (rank, row) orders as the ordinal does.  The distance cannot stand in for the score -- 1.0f - s and fmaf(-2, key, |q|^2)
// round, two scores may share a distance -- and the ordinal cannot be computed by a rank that holds only its own buckets' counts.
//
// union_merge_kernel: one wave per query, knn_merge_kernel's scheme with a 16-byte entry -- a sorted list of LR entries in LDS, every
// part's k entries loaded worst-first behind it and bitonic-merged, `world` rounds.
// An entry is two 64-bit words, kept in two LDS planes of 2 * LR words each:
//   hi = (image of the score << 32) | rank      image: -0 -> +0, then the order-preserving unsigned image of the float, inverted,
//   lo = (row << 32) | source                   so that a SMALLER (hi, lo) is the better entry; source = part * k + j
// An empty slot and a part's padding are (~0, ~0): behind every real entry.
// Two planes of 8-byte words and not one array of 16-byte entries: per wave instruction ds_read_b64 takes 2 LDS cycles and
// ds_read_b128 4, ds_write_b64 about 6 and ds_write_b128 about 13, so both layouts cost the same cycles per exchange; from stride 32
// on a lane group's 32 consecutive 8-byte words are exactly one 256-byte bank row (no conflict), below it both layouts are 2-way.  The
// planes keep knn_bitonic_merge's 8-byte accesses and their natural alignment, and the read-out touches the lo plane alone.
#pragma once
#include <hip/hip_runtime.h>

namespace lmi {

constexpr int UNION_PART_PLANES = 5;   // LMI_UNION_PART_PLANES
enum { UPART_SCORE = 0, UPART_DIST, UPART_ID, UPART_RANK, UPART_ROW };
constexpr unsigned long long UMERGE_EMPTY = ~0ull;

// smaller = better: the inverted order-preserving image of the score (as floats: -0 == +0), then the rank
__device__ __forceinline__ unsigned long long umerge_hi(unsigned score_bits, unsigned rank) {
    const unsigned u = score_bits == 0x80000000u ? 0u : score_bits;
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)~asc << 32) | rank;
}

// knn_bitonic_merge on (hi, lo) pairs: e[0, n) best-first in its first half and worst-first in its second -> best-first throughout
__device__ __forceinline__ void umerge_bitonic_merge(unsigned long long* hi, unsigned long long* lo, int n, int lane) {
    for (int stride = n >> 1; stride > 0; stride >>= 1) {
        for (int i = lane; i < (n >> 1); i += 64) {
            const int a = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), b = a | stride;
            const unsigned long long ah = hi[a], bh = hi[b], al = lo[a], bl = lo[b];
            if (bh < ah || (bh == ah && bl < al)) { hi[a] = bh; hi[b] = ah; lo[a] = bl; lo[b] = al; }
        }
        __syncthreads();
    }
}

// grid nq, block 64, dynamic LDS 4 * LR 8-byte words (LR a power of two >= max(128, k)).  parts [world][5][nq][k], dense.
// Query q: D[q][k], I[q][k] <- DIST and ID of the first k of its world * k entries in the order above (behind the real ones +inf / 0),
// counts[q] (nullable) <- the number of real ones.  An entry whose ROW is 0xffffffff is padding and never selected.
__global__ __launch_bounds__(64) void union_merge_kernel(const int* __restrict__ parts, int world, int nq, int k, int LR,
                                                         float* __restrict__ D, unsigned* __restrict__ I, int* __restrict__ counts) {
    extern __shared__ unsigned long long umerge_lds[];
    unsigned long long* hi = umerge_lds;
    unsigned long long* lo = umerge_lds + 2 * LR;
    const int lane = threadIdx.x, q = blockIdx.x;
    const size_t plane = (size_t)nq * k;
    for (int i = lane; i < LR; i += 64) { hi[i] = UMERGE_EMPTY; lo[i] = UMERGE_EMPTY; }
    __syncthreads();
    for (int w = 0; w < world; ++w) {
        const int* p = parts + (size_t)w * UNION_PART_PLANES * plane + (size_t)q * k;
        for (int i = lane; i < LR; i += 64) {
            const int j = LR - 1 - i;   // worst-first
            unsigned long long eh = UMERGE_EMPTY, el = UMERGE_EMPTY;
            if (j < k) {
                const unsigned row = (unsigned)p[UPART_ROW * plane + j];
                if (row != 0xffffffffu) {
                    eh = umerge_hi((unsigned)p[UPART_SCORE * plane + j], (unsigned)p[UPART_RANK * plane + j]);
                    el = ((unsigned long long)row << 32) | (unsigned)(w * k + j);
                }
            }
            hi[LR + i] = eh;
            lo[LR + i] = el;
        }
        __syncthreads();
        umerge_bitonic_merge(hi, lo, 2 * LR, lane);
    }
    int real = 0;   // uniform
    for (int j0 = 0; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long el = j < k ? lo[j] : UMERGE_EMPTY;
        const bool have = (unsigned)(el >> 32) != 0xffffffffu;
        real += __popcll(__ballot(have));
        if (j >= k) continue;
        float dv = __builtin_inff();
        unsigned iv = 0u;
        if (have) {
            const unsigned src = (unsigned)el;
            const int* p = parts + (size_t)(src / (unsigned)k) * UNION_PART_PLANES * plane + (size_t)q * k + (src % (unsigned)k);
            dv = __uint_as_float((unsigned)p[UPART_DIST * plane]);
            iv = (unsigned)p[UPART_ID * plane];
        }
        D[(size_t)q * k + j] = dv;
        I[(size_t)q * k + j] = iv;
    }
    if (counts && lane == 0) counts[q] = real;
}

}  // namespace lmi
