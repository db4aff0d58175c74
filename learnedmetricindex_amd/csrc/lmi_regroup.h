// lmi_regroup.h -- device side of lmi_regroup (lmi_host_regroup.h; include/lmi_hip.h states the contract): a second, independent index
// that holds a built index's objects under new bucket labels.
//
// Nothing here sums a float and no position is decided by the order in which atomics arrive: the counters below are integer sums, and
// where an object lands follows from the ascending order of unique 64-bit words.
//   regroup_label_kernel    every live row of the source: its new label (the sorted list's, found by mark_rows_kernel's binary search,
//                           else bucket_map[its bucket]), its word (label << 32) | ordinal and its slab row, both stored AT its ordinal
//                           (ordinal = ord_base[bucket] + row in the bucket: the source's order, whatever the slab looks like); the
//                           objects per new label, the unnamed rows of buckets mapped to -1 per old bucket, the named objects.
//   regroup_runs_kernel     tile `blockIdx.x` of the words sorted in LDS, in place (lmi_range_sort.h's network)
//   (lmi_range_sort.h's range_sort_merge_kernel doubles the runs until one run holds every word)
//   regroup_srcpos_kernel   the i-th sorted word is the (i - first[label])-th object of new bucket `label`: srcpos[its new slab row] <-
//                           the source's slab row of its ordinal.  The caller has filled srcpos with -1 (subset_srcpos_kernel's form),
//                           which lmi_subset.h's three gather kernels then read unchanged.
// Every store is a plain vector store; nothing in this file is read by the query path.  The label kernel writes at ordinals < n (the
// host's sum of the live bucket sizes); the runs kernel guards by n; srcpos indices are below the new slab's rows because first[] and
// new_rb_start[] are made from the very counts the label kernel returned.
#pragma once
#include "lmi_range_sort.h"

namespace lmi {

// grid (x, L), bucket = blockIdx.y, block 256.  list / list_label [n_list]: sorted by id, unique.  map [L]: -1 = "must be emptied by
// the list".  words / ord_row [n]; counts [L_new], left [L], named [1]: zeroed by the caller.
__global__ __launch_bounds__(256) void regroup_label_kernel(const uint32_t* __restrict__ ids_slab, const int* __restrict__ rb_start,
                                                           const int* __restrict__ nb_rows, const int* __restrict__ ord_base,
                                                           const uint32_t* __restrict__ list, const int* __restrict__ list_label, int n_list,
                                                           const int* __restrict__ map, unsigned long long* __restrict__ words,
                                                           int* __restrict__ ord_row, int* __restrict__ counts, int* __restrict__ left,
                                                           unsigned long long* __restrict__ named) {
    const int b = blockIdx.y;
    const int n_b = nb_rows[b];
    const size_t base = (size_t)rb_start[b] * 32;
    const int ob = ord_base[b], mapped = map[b];
    const int lane = threadIdx.x & 63;
    int n_named = 0, n_left = 0;
    for (int r0 = blockIdx.x * blockDim.x; r0 < n_b; r0 += gridDim.x * blockDim.x) {   // (r0: the same in every lane of the block)
        const int row = r0 + threadIdx.x;
        int lab = -1;
        if (row < n_b) {
            const uint32_t id = ids_slab[base + row];
            int lo = 0, hi = n_list;   // first entry >= id
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (list[mid] < id) lo = mid + 1;
                else hi = mid;
            }
            const bool hit = lo < n_list && list[lo] == id;
            lab = hit ? list_label[lo] : mapped;
            n_named += hit;
            n_left += lab < 0;
            // (an unmapped object: the call is refused once the counts are back; its word only has to be a valid one)
            words[ob + row] = ((unsigned long long)(unsigned)(lab < 0 ? 0 : lab) << 32) | (unsigned)(ob + row);
            ord_row[ob + row] = (int)(base + row);
        }
        // one atomic per distinct label of the wave: the unnamed rows of a bucket share theirs
        unsigned long long todo = __ballot(lab >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int ll = __shfl(lab, leader);
            const unsigned long long same = __ballot(lab == ll);
            if (lane == leader) atomicAdd(counts + ll, __popcll(same));
            todo &= ~same;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_named += __shfl_xor(n_named, o);
        n_left += __shfl_xor(n_left, o);
    }
    if (lane == 0 && n_named) atomicAdd(named, (unsigned long long)n_named);
    if (lane == 0 && n_left) atomicAdd(left + b, n_left);
}

// grid ceil(n / T), block 256, dynamic LDS 8 * T; T a power of two.  words [n]: tile b's words <- the same words, ascending.
__global__ __launch_bounds__(RANGE_SORT_BLOCK) void regroup_runs_kernel(unsigned long long* __restrict__ words, long long n, int T) {
    extern __shared__ unsigned long long rsort_lds[];
    const int tid = threadIdx.x;
    const long long s = (long long)blockIdx.x * T;
    const int cnt = (int)(n - s < T ? n - s : T);
    int P = 2;   // (the last tile: the power of two its words need, not all of T)
    while (P < cnt) P <<= 1;
    for (int i = tid; i < P; i += RANGE_SORT_BLOCK) rsort_lds[i] = i < cnt ? words[s + i] : RSORT_PAD;
    __syncthreads();
    rsort_lds_sort(rsort_lds, P, tid);
    for (int i = tid; i < cnt; i += RANGE_SORT_BLOCK) words[s + i] = rsort_lds[i];
}

// grid-stride over the n sorted words.  first [L_new]: exclusive prefix of the new counts; new_rb_start [L_new]: the new layout.
__global__ void regroup_srcpos_kernel(const unsigned long long* __restrict__ sorted, long long n, const int* __restrict__ ord_row,
                                      const int* __restrict__ first, const int* __restrict__ new_rb_start, int* __restrict__ srcpos) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long w = sorted[i];
        const int lab = (int)(w >> 32);
        srcpos[(size_t)new_rb_start[lab] * 32 + (size_t)(i - first[lab])] = ord_row[(unsigned)w];
    }
}

}  // namespace lmi
