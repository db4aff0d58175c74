// lmi_filter.h -- device code of the filtered union scan (lmi_filter_create, lmi_scan_union_filtered and its relatives;
// include/lmi_hip.h states the contract).
//
// A filter set's masks: one 32-bit word per row-block of 32 slab rows, [nf][n_rb_total]; row r of bucket b is bit r & 31 of word
// rb_start[b] + (r >> 5) of its filter's row (buckets start on row-block boundaries).  The bits of rows >= n_b, of a bucket's spare
// row-blocks and of holes are 0: the host zero-fills the masks and filter_mark_kernel writes the words of live row-blocks only.
//   filter_mark_kernel           every live row against every filter's sorted id list (mark_rows_kernel's search), a wave's 64 verdicts
//                                by ballot into two words, the allowed rows counted per (filter, bucket);
//   union_select_masked_kernel   union_select_kernel whose candidates enter only where the slot's mask row has their bit: the one place
//                                of the union scan where candidates are chosen.  Pack, score, finish and the merges are lmi_union.h's.
// Every store is a plain vector store; the only atomic is an integer atomicAdd.
#pragma once
#include "lmi_union.h"

namespace lmi {

// grid (cdiv(row-blocks of the largest bucket, 8), L, nf), block 256: wave w of block x takes rows [(4 x + w) * 64, +64) of bucket
// blockIdx.y against filter blockIdx.z, one row per lane.  list: the filters' sorted, de-duplicated id lists back to back, filter j's at
// [list_off[j], list_off[j + 1]); modes[j]: 0 keep the listed, 1 drop them.  mask [nf][n_rb_total] (zero-filled by the caller) <- the
// verdicts of live rows; counts [nf][L] (zeroed by the caller) += the allowed rows.
__global__ __launch_bounds__(256) void filter_mark_kernel(const uint32_t* __restrict__ ids_slab, const int* __restrict__ rb_start,
                                                          const int* __restrict__ nb_rows, const uint32_t* __restrict__ list,
                                                          const int* __restrict__ list_off, const int* __restrict__ modes,
                                                          long long n_rb_total, int L, unsigned* __restrict__ mask,
                                                          int* __restrict__ counts) {
    const int b = blockIdx.y, j = blockIdx.z;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n_b = nb_rows[b];
    const long long row0 = ((long long)blockIdx.x * 4 + w) * 64;
    if (row0 >= n_b) return;   // uniform over the wave: every lane below reaches the ballot
    const long long row = row0 + lane;
    const bool live = row < n_b;
    const long long rb0 = rb_start[b];
    const uint32_t id = live ? ids_slab[rb0 * 32 + row] : 0u;
    const int l0 = list_off[j], l1 = list_off[j + 1];
    int lo = l0, hi = l1;   // first entry >= id
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (list[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    const bool hit = lo < l1 && list[lo] == id;
    const bool allowed = live && (modes[j] ? !hit : hit);
    const unsigned long long m = __ballot(allowed);
    // the wave's two row-blocks: the second one is the bucket's only while it holds a live row (behind it the next bucket may start)
    unsigned* out = mask + (size_t)j * n_rb_total + rb0 + (row0 >> 5);
    if (lane == 0) out[0] = (unsigned)m;
    if (lane == 32 && row0 + 32 < n_b) out[1] = (unsigned)(m >> 32);
    const int cnt = __popcll(m);   // the wave's sum, an integer
    if (lane == 0 && cnt) atomicAdd(counts + (size_t)j * L + b, cnt);
}

// knn_select_wave (lmi_knn.h) on a fresh list over row[0 .. n), with a mask: the score at position p enters only if bit p & 31 of
// mrow[p >> 5] is set (mrow == nullptr: every position).  A masked-out score is replaced by -FLT_MAX, which the rule "only scores
// > -FLT_MAX are taken" never admits; position p keeps its pair (score, row_base + p), so the order among the allowed is untouched.
// The loop is written out here, so that knn_select_kernel and union_select_kernel compile to what they were; the sorting networks are
// shared.
__device__ __forceinline__ void union_select_masked_wave(const float* __restrict__ row, long long n, const unsigned* __restrict__ mrow,
                                                         unsigned row_base, int k, int LR, knn_entry* __restrict__ mine) {
    extern __shared__ knn_entry knn_lds[];
    const int lane = threadIdx.x;
    for (int i = lane; i < LR; i += 64) knn_lds[i] = KNN_EMPTY;
    __syncthreads();
    knn_entry thr = knn_lds[k - 1];
    knn_entry* buf = knn_lds + LR;
    int cnt = 0;   // uniform
    auto flush = [&]() {
        for (int i = cnt + lane; i < LR; i += 64) buf[i] = KNN_EMPTY;
        __syncthreads();
        knn_bitonic_sort_up(buf, LR, lane);
        knn_bitonic_merge(knn_lds, 2 * LR, lane);
        thr = knn_lds[k - 1];
        cnt = 0;
        __syncthreads();
    };
    for (long long p0 = 0; p0 < n; p0 += 256) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long p = p0 + u * 64 + lane;
            v[u] = p < n ? row[p] : -FLT_MAX;
            // two distinct words per wave step: lanes 0..31 share one, lanes 32..63 the next (p0 is a multiple of 64)
            if (mrow && p < n && !((mrow[p >> 5] >> (p & 31)) & 1u)) v[u] = -FLT_MAX;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const knn_entry e = knn_make(v[u], row_base + (unsigned)(p0 + u * 64 + lane));
            const bool pass = v[u] > -FLT_MAX && knn_better(e, thr);
            const unsigned long long m = __ballot(pass);
            if (!m) continue;
            const int np = __popcll(m);
            if (cnt + np > LR) flush();   // what passed the old threshold still goes in: the merge puts it where it belongs
            if (pass) buf[cnt + __popcll(m & ((1ull << lane) - 1))] = e;
            cnt += np;
        }
    }
    if (cnt) flush();
    else __syncthreads();
    for (int i = lane; i < LR; i += 64) mine[i] = knn_lds[i];
}

// grid = the wave's slots, block 64, dynamic LDS 2 * LR entries.  slot_mask[slot]: the word offset of the slot's mask row inside mask
// (its filter's row + its bucket's first row-block), or -1: the slot's query is unfiltered.
__global__ __launch_bounds__(64) void union_select_masked_kernel(const float* __restrict__ S, const UnionSlot* __restrict__ slots,
                                                                 const long long* __restrict__ slot_mask, const unsigned* __restrict__ mask,
                                                                 int k, int LR, knn_entry* __restrict__ lists) {
    const UnionSlot sl = slots[blockIdx.x];
    const long long mo = slot_mask[blockIdx.x];
    union_select_masked_wave(S + sl.s_off, sl.n, mo >= 0 ? mask + mo : nullptr, sl.base, k, LR, lists + sl.list);
}

}  // namespace lmi
