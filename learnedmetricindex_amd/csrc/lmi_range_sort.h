// lmi_range_sort.h -- device code of lmi_range_result_sort: every segment of a range result stably sorted by distance (include/lmi_hip.h
// states the contract; the host arithmetic: lmi_range_sort_plan.h).
//
// An entry is ONE 64-bit word: (image of the distance << 32) | position in the segment.  The image is union_merge_kernel's, not
// inverted: -0 -> +0, then the order-preserving unsigned image of the float; every NaN becomes 0xffffffff, above +inf (0xff800000).
// The position makes the words of a segment unique, so ANY sorting network or merge yields the one ascending order of the words, which
// is the stable order of the keys: tile length, run boundaries, grid and the form cannot show in the result.  Padding is all ones: a
// segment has fewer than 2^32 entries, so no position and no real word is all ones, and the padding sorts behind every real entry.
//
// The kernels read the result's dists / ids and write a COPY (cD / cI, indexed from the group's first entry g0); the host copies the
// copy back.  No kernel writes the result's arrays, so a position may be gathered from anywhere in its segment at any time.
//   range_sort_wave_kernel   one WAVE per segment of 2 .. 256 entries, four waves per block: the words in 4 registers per lane
//                            (entry e = r * 64 + lane), a bitonic network of __shfl_xor exchanges below stride 64 and register
//                            exchanges at 64 and 128; no LDS, no barrier.  A segment padded to P <= 64 * r skips register r's shuffles.
//   range_sort_tile_kernel   one BLOCK per segment of up to T entries: the words in LDS (P * 8 bytes, P the padded length), the
//                            bitonic network in knn_bitonic_sort_up's form: thread i of a step owns the pair (lo, lo | stride).  From
//                            stride 32 on a wave's 64 pairs read two runs of 32 consecutive 8-byte words: conflict-free with
//                            ds_read_b64's 64 banks; below it 2-way at most.
//   range_sort_runs_kernel   the same sort for tile `blockIdx.x` of ONE long segment; the sorted words go to a key buffer.
//   range_sort_merge_kernel  one merge pass over the key buffer: runs of `run` words become runs of 2 * run.  Block b produces the output
//                            piece [b * M, b * M + M): it finds the piece's two ends on the merge path of its pair of runs (two binary
//                            searches, the same in every lane: lmi_range_sort_plan.h's merge_piece and merge_split, which the CPU
//                            self-test replays), loads the A part ascending and the B part descending into LDS -- together exactly
//                            the piece, a bitonic sequence -- and merges it with log2(M) exchange steps.
//   range_sort_apply_kernel  cD / cI <- dists / ids of the long segment gathered through the sorted words' positions.
// Every global access is guarded by the segment's length; LDS indices are < P <= T (tile, runs) or < M (merge).
#pragma once
#include <hip/hip_runtime.h>

#include "lmi_range_sort_plan.h"   // merge_piece, merge_split: the merge pass's arithmetic, shared with the CPU self-test

namespace lmi {

constexpr int RANGE_SORT_BLOCK = 256;
constexpr int RANGE_SORT_WAVE_REGS = 4;   // lmi_range_sort_plan::WAVE_ROWS / 64
constexpr unsigned long long RSORT_PAD = ~0ull;

__device__ __forceinline__ unsigned long long rsort_word(float dist, unsigned pos) {
    unsigned u = __float_as_uint(dist);
    if (u == 0x80000000u) u = 0u;
    unsigned key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if ((u & 0x7fffffffu) > 0x7f800000u) key = 0xffffffffu;   // NaN, either sign, any payload
    return ((unsigned long long)key << 32) | pos;
}

// lo < hi are the two entries of a pair; up: the pair's block ascends
__device__ __forceinline__ void rsort_cx(unsigned long long& lo, unsigned long long& hi, bool up) {
    const unsigned long long a = lo, b = hi;
    if ((a > b) == up) { lo = b; hi = a; }
}

// grid ceil(n_seg / 4), block 256.  seg_at [n_seg]: where the segment begins in D / I; seg_n [n_seg]: its length, 2 .. 256.
__global__ __launch_bounds__(RANGE_SORT_BLOCK) void range_sort_wave_kernel(const long long* __restrict__ seg_at, const int* __restrict__ seg_n,
                                                                          int n_seg, const float* __restrict__ D,
                                                                          const unsigned* __restrict__ I, long long g0,
                                                                          float* __restrict__ cD, unsigned* __restrict__ cI) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * (RANGE_SORT_BLOCK / 64) + (threadIdx.x >> 6);
    if (item >= n_seg) return;   // the whole wave; the kernel has no barrier
    const long long at = seg_at[item];
    const int n = seg_n[item];
    int P = 2;
    while (P < n) P <<= 1;
    unsigned long long v[RANGE_SORT_WAVE_REGS];
#pragma unroll
    for (int r = 0; r < RANGE_SORT_WAVE_REGS; ++r) {
        const int e = r * 64 + lane;
        v[r] = e < n ? rsort_word(D[at + e], (unsigned)e) : RSORT_PAD;
    }
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j == 128) {
                rsort_cx(v[0], v[2], (lane & k) == 0);          // entries lane and 128 + lane: k is 256, bit k of both is clear
                rsort_cx(v[1], v[3], ((64 + lane) & k) == 0);
            } else if (j == 64) {
                rsort_cx(v[0], v[1], (lane & k) == 0);          // k is 128 or 256
                rsort_cx(v[2], v[3], ((128 + lane) & k) == 0);
            } else {
#pragma unroll
                for (int r = 0; r < RANGE_SORT_WAVE_REGS; ++r) {
                    if (r * 64 < P) {   // the same in every lane
                        const unsigned long long mine = v[r], other = __shfl_xor(mine, j);
                        const bool up = ((r * 64 + lane) & k) == 0, lower = (lane & j) == 0;
                        v[r] = (lower == up) ? (mine < other ? mine : other) : (mine < other ? other : mine);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RANGE_SORT_WAVE_REGS; ++r) {
        const int e = r * 64 + lane;
        if (e < n) {
            const unsigned pos = (unsigned)v[r];
            cD[at - g0 + e] = D[at + pos];
            cI[at - g0 + e] = I[at + pos];
        }
    }
}

// any e[0, P) -> ascending; P a power of two >= 2; every thread of the block calls it
__device__ __forceinline__ void rsort_lds_sort(unsigned long long* e, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int stride = k >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += RANGE_SORT_BLOCK) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
                const unsigned long long a = e[lo], b = e[hi];
                if ((a > b) == ((lo & k) == 0)) { e[lo] = b; e[hi] = a; }
            }
            __syncthreads();
        }
    }
}

// e[0, P) ascending up to some index and descending from it on (a bitonic sequence) -> ascending throughout
__device__ __forceinline__ void rsort_lds_merge(unsigned long long* e, int P, int tid) {
    for (int stride = P >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < (P >> 1); i += RANGE_SORT_BLOCK) {
            const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
            const unsigned long long a = e[lo], b = e[hi];
            if (a > b) { e[lo] = b; e[hi] = a; }
        }
        __syncthreads();
    }
}

// grid n_seg, block 256, dynamic LDS 8 * (the largest padded length of the launch).  seg_n [n_seg]: 2 .. T.
__global__ __launch_bounds__(RANGE_SORT_BLOCK) void range_sort_tile_kernel(const long long* __restrict__ seg_at, const int* __restrict__ seg_n,
                                                                          const float* __restrict__ D, const unsigned* __restrict__ I,
                                                                          long long g0, float* __restrict__ cD, unsigned* __restrict__ cI) {
    extern __shared__ unsigned long long rsort_lds[];
    const int tid = threadIdx.x;
    const long long at = seg_at[blockIdx.x];
    const int n = seg_n[blockIdx.x];
    int P = 2;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += RANGE_SORT_BLOCK) rsort_lds[i] = i < n ? rsort_word(D[at + i], (unsigned)i) : RSORT_PAD;
    __syncthreads();
    rsort_lds_sort(rsort_lds, P, tid);
    for (int i = tid; i < n; i += RANGE_SORT_BLOCK) {
        const unsigned pos = (unsigned)rsort_lds[i];
        cD[at - g0 + i] = D[at + pos];
        cI[at - g0 + i] = I[at + pos];
    }
}

// grid ceil(n / T), block 256, dynamic LDS 8 * T.  One long segment: D + at, n entries; keys [n] <- tile b's words, ascending.
__global__ __launch_bounds__(RANGE_SORT_BLOCK) void range_sort_runs_kernel(const float* __restrict__ D, long long at, long long n, int T,
                                                                          unsigned long long* __restrict__ keys) {
    extern __shared__ unsigned long long rsort_lds[];
    const int tid = threadIdx.x;
    const long long s = (long long)blockIdx.x * T;
    const int cnt = (int)(n - s < T ? n - s : T);
    for (int i = tid; i < T; i += RANGE_SORT_BLOCK) rsort_lds[i] = i < cnt ? rsort_word(D[at + s + i], (unsigned)(s + i)) : RSORT_PAD;
    __syncthreads();
    rsort_lds_sort(rsort_lds, T, tid);
    for (int i = tid; i < cnt; i += RANGE_SORT_BLOCK) keys[s + i] = rsort_lds[i];
}

// grid ceil(n / M), block 256, dynamic LDS 8 * M; M a power of two <= run.  src [n]: ascending runs of `run` words (the last may be
// shorter) -> dst [n]: ascending runs of 2 * run.
__global__ __launch_bounds__(RANGE_SORT_BLOCK) void range_sort_merge_kernel(const unsigned long long* __restrict__ src, long long n,
                                                                           long long run, int M, unsigned long long* __restrict__ dst) {
    extern __shared__ unsigned long long rsort_lds[];
    const int tid = threadIdx.x;
    namespace sp = lmi_range_sort_plan;
    const sp::Piece X = sp::merge_piece(n, run, M, blockIdx.x);   // the piece, its pair of runs: the same in every lane
    const long long o0 = X.o0, o1 = X.o1;
    const unsigned long long* A = src + X.p0;
    const unsigned long long* B = A + X.la;
    const long long i0 = sp::merge_split(A, X.la, B, X.lb, o0 - X.p0), i1 = sp::merge_split(A, X.la, B, X.lb, o1 - X.p0);
    const long long j0 = o0 - X.p0 - i0;
    const int na = (int)(i1 - i0), nb = (int)(o1 - o0) - na;   // na + nb = o1 - o0 <= M
    for (int t = tid; t < M; t += RANGE_SORT_BLOCK) {
        unsigned long long w = RSORT_PAD;
        if (t < na) w = A[i0 + t];
        else if (t >= M - nb) w = B[j0 + (M - 1 - t)];
        rsort_lds[t] = w;
    }
    __syncthreads();
    rsort_lds_merge(rsort_lds, M, tid);
    for (int t = tid; t < (int)(o1 - o0); t += RANGE_SORT_BLOCK) dst[o0 + t] = rsort_lds[t];
}

// grid ceil(n / 256), block 256.  One long segment: entry i of the copy <- the entry at the position of the i-th sorted word.
__global__ __launch_bounds__(RANGE_SORT_BLOCK) void range_sort_apply_kernel(const unsigned long long* __restrict__ keys, long long at, long long n,
                                                                           const float* __restrict__ D, const unsigned* __restrict__ I,
                                                                           long long g0, float* __restrict__ cD, unsigned* __restrict__ cI) {
    const long long i = (long long)blockIdx.x * RANGE_SORT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned pos = (unsigned)keys[i];
    cD[at - g0 + i] = D[at + pos];
    cI[at - g0 + i] = I[at + pos];
}

}  // namespace lmi
