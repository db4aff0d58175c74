// lmi_knn_range.h -- device code of lmi_knn_range: the exact range query over a whole base with no index (include/lmi_hip.h states the
// contract).
//
// dense_pack_kernel, dense_norm_kernel and knn_score_kernel (lmi_dense.h, lmi_knn.h) run as they are: the scores of one (query group,
// piece of the base) are the slab S[q * pitch + row of the piece].  Behind them, one wave (64 lanes) per (query, split of the piece),
// walking its stretch [a, b) of the query's slab row 64 rows at a time in row order (256 contiguous bytes per step, from a on; the
// loads of four steps are issued together):
//   knn_range_count_kernel   a ballot of the admission predicate, its popcount summed uniformly, one store of the stretch's count;
//   knn_range_emit_kernel    the same walk: an admitted lane writes (dist, row_base + row) at the stretch's offset in the piece's
//                            chunk + the running count + the popcount of the ballot below the lane -- row order, no sort, no atomic.
// The final placement is range_gather_kernel (lmi_range.h) as it is.  knn_range_load / knn_range_step are the one walk step and
// range_admit (without a mask) the one predicate: count and emit cannot disagree about a row, and the emit never writes at or past the
// stretch's counted length in any case.  Every store is a plain vector store; offsets into the slab and the chunk are 64-bit.
#pragma once
#include "lmi_knn.h"
#include "lmi_range.h"

namespace lmi {

// what both walks read of a (query, split): the query's slab row, the stretch, the radius
struct KnnRangeView {
    const float* row;
    long long a, b;
    int q;
    float radius;
};
// grid (gq, splits): block (q, s) owns split s of the piece's len rows (lmi_knn_plan::split_range)
__device__ __forceinline__ KnnRangeView knn_range_view(const float* __restrict__ S, long long pitch, long long len,
                                                       const float* __restrict__ radius) {
    const int q = blockIdx.x, s = blockIdx.y, splits = gridDim.y;
    return KnnRangeView{S + (size_t)q * pitch, len * s / splits, len * (s + 1) / splits, q, radius[q]};
}
// A walk takes KNN_RANGE_STEPS steps of 64 rows at a time so that their loads are in flight together (one wave owns a stretch of
// thousands of rows: a load per step would leave it waiting on one 256-byte request after another); the ballots follow in row order.
constexpr int KNN_RANGE_STEPS = 4;
// lane l's score of the step at p0 (a + a multiple of 64): row p0 + l of the piece; past the stretch: -FLT_MAX, which is never admitted
__device__ __forceinline__ float knn_range_load(const KnnRangeView& v, long long p0, int lane) {
    const long long p = p0 + lane;
    return p < v.b ? v.row[p] : -FLT_MAX;
}
// the ballot of a step: lane l judges the score it loaded
__device__ __forceinline__ unsigned long long knn_range_step(const KnnRangeView& v, const float* __restrict__ qn, float s) {
    return __ballot(range_admit(s, qn, v.q, v.radius, 0xffffffffu, 0));
}

// grid (gq, splits), block 64.  S: the slab of the group's gq queries against the piece's len rows; qn [gq]: the queries' squared
// norms (L2) or nullptr (IP); radius [gq].  counts[q * splits + s] <- the admitted rows of the stretch.
__global__ __launch_bounds__(64) void knn_range_count_kernel(const float* __restrict__ S, long long pitch, long long len,
                                                             const float* __restrict__ qn, const float* __restrict__ radius,
                                                             int* __restrict__ counts) {
    const int lane = threadIdx.x;
    const KnnRangeView v = knn_range_view(S, pitch, len, radius);
    int cnt = 0;   // uniform
    for (long long p0 = v.a; p0 < v.b; p0 += 64 * KNN_RANGE_STEPS) {
        float s[KNN_RANGE_STEPS];
#pragma unroll
        for (int u = 0; u < KNN_RANGE_STEPS; ++u) s[u] = knn_range_load(v, p0 + u * 64, lane);
#pragma unroll
        for (int u = 0; u < KNN_RANGE_STEPS; ++u) cnt += __popcll(knn_range_step(v, qn, s[u]));
    }
    if (lane == 0) counts[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = cnt;
}

// grid (gq, splits), block 64.  The admitted rows of stretch (q, s), in row order, go to D / I [off[q * splits + s], + its count) of
// the piece's chunk: the distance (sim_to_dist) and the row's number in the base, row_base + its row in the piece.
__global__ __launch_bounds__(64) void knn_range_emit_kernel(const float* __restrict__ S, long long pitch, long long len, unsigned row_base,
                                                            const float* __restrict__ qn, const float* __restrict__ radius,
                                                            const int* __restrict__ counts, const long long* __restrict__ off,
                                                            float* __restrict__ D, unsigned* __restrict__ I) {
    const int lane = threadIdx.x;
    const size_t slot = (size_t)blockIdx.x * gridDim.y + blockIdx.y;
    const int total = counts[slot];
    if (total <= 0) return;   // uniform
    const KnnRangeView v = knn_range_view(S, pitch, len, radius);
    const long long o = off[slot];
    int cnt = 0;   // uniform
    for (long long p0 = v.a; p0 < v.b && cnt < total; p0 += 64 * KNN_RANGE_STEPS) {
        float s[KNN_RANGE_STEPS];
#pragma unroll
        for (int u = 0; u < KNN_RANGE_STEPS; ++u) s[u] = knn_range_load(v, p0 + u * 64, lane);
#pragma unroll
        for (int u = 0; u < KNN_RANGE_STEPS; ++u) {
            const unsigned long long m = knn_range_step(v, qn, s[u]);
            const int at = cnt + __popcll(m & ((1ull << lane) - 1));
            if (((m >> lane) & 1ull) && at < total) {
                D[o + at] = sim_to_dist(s[u], qn, v.q);
                I[o + at] = row_base + (unsigned)(p0 + u * 64 + lane);
            }
            cnt += __popcll(m);
        }
    }
}

}  // namespace lmi
