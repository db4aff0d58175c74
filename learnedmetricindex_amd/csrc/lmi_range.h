// lmi_range.h -- device code of the range search (lmi_scan_range, lmi_search_range, lmi_search_tree_range; include/lmi_hip.h states
// the contract): every candidate of the union scan within a radius, in ordinal order.
//
// Per wave of a query group union_pack_kernel and union_score_kernel (lmi_union.h) run as they are: a slot's scores are one row of
// the wave's slab.  Behind them, one wave (64 lanes) per slot, walking the slot's slab row 64 rows at a time in row order (256
// contiguous bytes per step):
//   range_count_kernel   a ballot of the admission predicate, its popcount summed uniformly, one store of the slot's count;
//   range_emit_kernel    the same walk: an admitted lane writes (dist, id) at the slot's offset in the wave's chunk + the running
//                        count + the popcount of the ballot below the lane -- row order, no sort, no atomic;
//   range_gather_kernel  a slot's run from its wave's chunk to its final place (the host computes both: lmi_range_plan.h).
// range_admit is the one admission predicate: count and emit cannot disagree about a row, and the emit never writes at or past the
// slot's counted length in any case.  Every store is a plain vector store.
#pragma once
#include "lmi_union.h"

namespace lmi {

// Whether the candidate at row `row` of a slot is admitted: its filter (mword: the mask word of row-block row >> 5; all ones without
// a filter) allows it, its score is > -FLT_MAX (the union scan's rule: NaN never passes) and the distance the scan would write is
// <= radius in binary32.  A NaN or -inf radius admits nothing.
__device__ __forceinline__ bool range_admit(float s, const float* __restrict__ qn2, int q, float radius, unsigned mword, int row) {
    if (!((mword >> (row & 31)) & 1u)) return false;
    if (!(s > -FLT_MAX)) return false;
    return radius > -__builtin_inff() && sim_to_dist(s, qn2, q) <= radius;
}

// what both walks read of a slot: slot_q[i] the (global) query of slot i, slot_mask (nullable: no filter) the word offset of its mask
// row or -1
struct RangeSlotView {
    const float* row;
    const unsigned* mrow;
    int n, q;
    float radius;
};
__device__ __forceinline__ RangeSlotView range_slot_view(const float* __restrict__ S, const UnionSlot* __restrict__ slots,
                                                         const int* __restrict__ slot_q, const long long* __restrict__ slot_mask,
                                                         const unsigned* __restrict__ mask, const float* __restrict__ radius) {
    const UnionSlot sl = slots[blockIdx.x];
    const long long mo = slot_mask ? slot_mask[blockIdx.x] : -1;
    const int q = slot_q[blockIdx.x];
    return RangeSlotView{S + sl.s_off, mo >= 0 ? mask + mo : nullptr, sl.n, q, radius[q]};
}
// the ballot of step p0 (a multiple of 64): lane l judges row p0 + l
__device__ __forceinline__ unsigned long long range_step(const RangeSlotView& v, const float* __restrict__ qn2, int p0, int lane, float* s_out) {
    const int p = p0 + lane;
    const bool in = p < v.n;
    const float s = in ? v.row[p] : -FLT_MAX;
    // two distinct words per step: lanes 0..31 share one, lanes 32..63 the next
    const unsigned w = v.mrow && in ? v.mrow[p >> 5] : 0xffffffffu;
    *s_out = s;
    return __ballot(in && range_admit(s, qn2, v.q, v.radius, w, p));
}

// grid = the wave's slots, block 64: counts[slot] <- the admitted rows of the slot
__global__ __launch_bounds__(64) void range_count_kernel(const float* __restrict__ S, const UnionSlot* __restrict__ slots,
                                                         const int* __restrict__ slot_q, const long long* __restrict__ slot_mask,
                                                         const unsigned* __restrict__ mask, const float* __restrict__ qn2,
                                                         const float* __restrict__ radius, int* __restrict__ counts) {
    const int lane = threadIdx.x;
    const RangeSlotView v = range_slot_view(S, slots, slot_q, slot_mask, mask, radius);
    int cnt = 0;   // uniform
    for (int p0 = 0; p0 < v.n; p0 += 64) {
        float s;
        cnt += __popcll(range_step(v, qn2, p0, lane, &s));
    }
    if (lane == 0) counts[blockIdx.x] = cnt;
}

// grid = the wave's slots, block 64.  Slot i's admitted rows, in row order, go to D / I [slot_off[i], + counts[i]) of the wave's chunk:
// the distance the scan writes and ids_slab[slot_pos0[i] + row] (fetched for admitted lanes only).
__global__ __launch_bounds__(64) void range_emit_kernel(const float* __restrict__ S, const UnionSlot* __restrict__ slots,
                                                        const int* __restrict__ slot_q, const long long* __restrict__ slot_mask,
                                                        const unsigned* __restrict__ mask, const float* __restrict__ qn2,
                                                        const float* __restrict__ radius, const int* __restrict__ counts,
                                                        const long long* __restrict__ slot_off, const long long* __restrict__ slot_pos0,
                                                        const unsigned* __restrict__ ids_slab, float* __restrict__ D,
                                                        unsigned* __restrict__ I) {
    const int lane = threadIdx.x;
    const int total = counts[blockIdx.x];
    if (total <= 0) return;   // uniform
    const RangeSlotView v = range_slot_view(S, slots, slot_q, slot_mask, mask, radius);
    const long long off = slot_off[blockIdx.x], pos0 = slot_pos0[blockIdx.x];
    int cnt = 0;   // uniform
    for (int p0 = 0; p0 < v.n && cnt < total; p0 += 64) {
        float s;
        const unsigned long long m = range_step(v, qn2, p0, lane, &s);
        const int at = cnt + __popcll(m & ((1ull << lane) - 1));
        if (((m >> lane) & 1ull) && at < total) {
            D[off + at] = sim_to_dist(s, qn2, v.q);
            I[off + at] = ids_slab[pos0 + p0 + lane];
        }
        cnt += __popcll(m);
    }
}

// grid = the wave's slots, block 64: slot i's run of n[i] results from the wave's chunk at src[i] to the final arrays at dst[i]
__global__ __launch_bounds__(64) void range_gather_kernel(const float* __restrict__ cD, const unsigned* __restrict__ cI,
                                                          const long long* __restrict__ src, const long long* __restrict__ dst,
                                                          const int* __restrict__ n, float* __restrict__ D, unsigned* __restrict__ I) {
    const int cnt = n[blockIdx.x];
    const long long s = src[blockIdx.x], t = dst[blockIdx.x];
    for (int i = threadIdx.x; i < cnt; i += 64) {
        D[t + i] = cD[s + i];
        I[t + i] = cI[s + i];
    }
}

}  // namespace lmi
