// lmi_range_join.h -- device code of the join of range parts (lmi_join_range_parts, lmi_allgather_join_range; include/lmi_hip.h
// states the contract): every run of the joined result is one part's run, copied unchanged.
//
// The host cuts the runs into pieces of at most piece_rows results (lmi_range_join_plan.h); grid = the pieces, one block per piece.
// A piece is n (dist, id) pairs of part `part` from `src` of that part's arrays to `dst` of the joined ones; the parts' base pointers
// come from two tables of `world` pointers.  Source and destination offsets are sums of unrelated counts and share no alignment, so
// every access is a 4-byte one: lane l of a step reads and writes element step * 256 + l -- 256 contiguous bytes per wave-instruction
// on both sides, at most one cache line more than the bytes moved, whatever the offsets are.  256 lanes: the default piece (4 096
// results, 32 KiB) is 16 steps of two independent load/store pairs per lane, four waves of loads in flight per block; a block of 64
// would need 64 dependent steps for the same piece.  No LDS, no atomic; nothing outside [dst, dst + n) is written.
#pragma once
#include <hip/hip_runtime.h>

namespace lmi {

constexpr int RANGE_JOIN_BLOCK = 256;

__global__ __launch_bounds__(RANGE_JOIN_BLOCK) void range_join_kernel(const float* const* __restrict__ part_dists,
                                                                      const unsigned* const* __restrict__ part_ids,
                                                                      const int* __restrict__ part, const long long* __restrict__ src,
                                                                      const long long* __restrict__ dst, const int* __restrict__ n,
                                                                      float* __restrict__ D, unsigned* __restrict__ I) {
    const int cnt = n[blockIdx.x];
    const int r = part[blockIdx.x];
    const float* sD = part_dists[r] + src[blockIdx.x];
    const unsigned* sI = part_ids[r] + src[blockIdx.x];
    float* tD = D + dst[blockIdx.x];
    unsigned* tI = I + dst[blockIdx.x];
    for (int i = threadIdx.x; i < cnt; i += RANGE_JOIN_BLOCK) {
        tD[i] = sD[i];
        tI[i] = sI[i];
    }
}

}  // namespace lmi
