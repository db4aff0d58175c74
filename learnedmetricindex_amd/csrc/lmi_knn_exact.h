// lmi_knn_exact.h -- device code of the exact k-NN through the index (lmi_search_knn_exact; include/lmi_hip.h states the contract;
// the words, the seed budget and the split: lmi_knn_exact_plan.h).
//
// The call scans a few promising buckets first (the seeds), takes the k-th distance they give as the query's radius, prunes the
// other buckets with the cover's admission rule (lmi_cover.h) and scans what is left.  Its own kernels:
//   knn_exact_bound_kernel  cover_admit_kernel's layout -- a block serves 16 queries against a strip of 64 buckets, centres and
//                           queries go through LDS 32 columns at a time, each thread owns the unsplit binary64 chains of its
//                           (query, bucket) pairs in ascending column order -- but where the admission kernel decides, this one
//                           keeps the rule's optimistic bound: one 64-bit word per pair (lmi_knn_exact_plan::word_of), a lane's
//                           consecutive buckets as consecutive 8-byte stores;
//   knn_exact_seed_kernel   one wave per query: every lane holds the smallest word of its strided share of the row; the wave's
//                           minimum is taken by six cross-lane exchanges of the 64-bit word, the lane that held it refills from its
//                           share, until the taken buckets' live rows reach k (or 32 are taken, or none is left).  Lane i keeps the
//                           i-th bucket taken; their ascending order is a rank by 32 broadcasts.  Words are unique, so what is taken
//                           does not depend on which lane held what;
//   knn_exact_tau_kernel    the radius of a query from the seed part: the k-th distance if the part is full, else +inf;
//   knn_exact_split_kernel  one wave per query: each seed is looked up in the admitted order (both ascending: a binary search), its
//                           entry is set to -1 -- what remains is the order of the second scan -- and the seed part's rank plane is
//                           rewritten from "position among the seeds" to "position in the admitted order", the numbering the second
//                           part's ranks have by construction.
// Every store is a plain vector store; nothing here touches a score.
#pragma once
#include "lmi_cover.h"
#include "lmi_knn_exact_plan.h"
#include "lmi_union_merge.h"

namespace lmi {

constexpr int KNN_EXACT_SEEDS = lmi_knn_exact_plan::MAX_SEEDS;

// grid (cdiv(gq, COVER_Q_PER_BLOCK), cdiv(L, 64)), block 256: cover_admit_kernel's roles.  Lane l of every wave holds bucket
// blockIdx.y * 64 + l; wave w takes the block's queries w * COVER_Q_PER_WAVE + j.  queries / qn: the group's first query onwards.
// words [gq][L]: every entry is written by exactly one thread (NO_WORD for a bucket without rows).
__global__ __launch_bounds__(256) void knn_exact_bound_kernel(int metric, const float* __restrict__ queries, const double* __restrict__ qn,
                                                              int gq, int d, const float* __restrict__ centres,
                                                              const float* __restrict__ R, const int* __restrict__ nb_rows, int L,
                                                              unsigned long long* __restrict__ words) {
    __shared__ float cen[64][COVER_COLS + 1];
    __shared__ float qs[COVER_Q_PER_BLOCK][COVER_COLS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y * 64 + lane;
    const int q0 = blockIdx.x * COVER_Q_PER_BLOCK;
    double chain[COVER_Q_PER_WAVE];
#pragma unroll
    for (int j = 0; j < COVER_Q_PER_WAVE; ++j) chain[j] = 0.0;
    for (int t0 = 0; t0 < d; t0 += COVER_COLS) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 64 * COVER_COLS / 256; ++j) {
            const int i = j * 256 + tid;
            const int r = i / COVER_COLS, c = i % COVER_COLS;
            const int bb = blockIdx.y * 64 + r;
            cen[r][c] = bb < L && t0 + c < d ? centres[(size_t)bb * d + t0 + c] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < COVER_Q_PER_BLOCK * COVER_COLS / 256; ++j) {
            const int i = j * 256 + tid;
            const int r = i / COVER_COLS, c = i % COVER_COLS;
            qs[r][c] = q0 + r < gq && t0 + c < d ? queries[(size_t)(q0 + r) * d + t0 + c] : 0.0f;
        }
        __syncthreads();
        const int tn = d - t0 < COVER_COLS ? d - t0 : COVER_COLS;
        for (int t = 0; t < tn; ++t) {
            const float c = cen[lane][t];
#pragma unroll
            for (int j = 0; j < COVER_Q_PER_WAVE; ++j) chain[j] = lmi_cover_plan::link(metric, chain[j], qs[w * COVER_Q_PER_WAVE + j][t], c);
        }
    }
    if (b >= L) return;   // (behind the last barrier)
    const double Rb = (double)R[b];
    const bool has = nb_rows[b] > 0;
#pragma unroll
    for (int j = 0; j < COVER_Q_PER_WAVE; ++j) {
        const int q = q0 + w * COVER_Q_PER_WAVE + j;
        if (q >= gq) break;
        unsigned long long word = lmi_knn_exact_plan::NO_WORD;
        if (has) {
            const double bound = metric == lmi_cover_plan::METRIC_IP ? lmi_cover_plan::bound_ip(chain[j], qn[q], Rb)
                                                                     : lmi_cover_plan::bound_l2(chain[j], Rb);
            word = lmi_knn_exact_plan::word_of(metric, bound, (unsigned)b);
        }
        words[(size_t)q * L + b] = word;
    }
}

// grid gq, block 64: query q of the group.  words [gq][L]; nb_rows [L] the live rows.  seeds [gq][KNN_EXACT_SEEDS] <- the taken
// buckets in ascending id, then -1; n_seeds [gq] <- their number.
__global__ __launch_bounds__(64) void knn_exact_seed_kernel(const unsigned long long* __restrict__ words, const int* __restrict__ nb_rows, int L,
                                                            int k, int* __restrict__ seeds, int* __restrict__ n_seeds) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* w = words + (size_t)q * L;
    unsigned long long mine = lmi_knn_exact_plan::NO_WORD;
    for (int b = lane; b < L; b += 64) {
        const unsigned long long v = w[b];
        mine = v < mine ? v : mine;
    }
    int taken = 0, my_seed = -1;   // taken, rows: uniform over the wave
    long long rows = 0;
    for (;;) {
        unsigned long long m = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)m, o);
            m = other < m ? other : m;
        }
        if (m == lmi_knn_exact_plan::NO_WORD) break;
        const int b = (int)lmi_knn_exact_plan::bucket_of(m);   // (< L: the bound pass wrote it)
        if (lane == taken) my_seed = b;
        rows += nb_rows[b];
        ++taken;
        if (lmi_knn_exact_plan::seeds_done(rows, k, taken)) break;
        if (mine == m) {   // one lane: the smallest word of its share behind the one it gave
            unsigned long long next = lmi_knn_exact_plan::NO_WORD;
            for (int bb = lane; bb < L; bb += 64) {
                const unsigned long long v = w[bb];
                if (v > m && v < next) next = v;
            }
            mine = next;
        }
    }
    int rank = 0;
#pragma unroll
    for (int i = 0; i < KNN_EXACT_SEEDS; ++i) {
        const int s = __shfl(my_seed, i);
        rank += i < taken && s < my_seed;
    }
    int* out = seeds + (size_t)q * KNN_EXACT_SEEDS;
    if (lane < taken) out[rank] = my_seed;
    else if (lane < KNN_EXACT_SEEDS) out[lane] = -1;
    if (lane == 0) n_seeds[q] = taken;
}

// one thread per query.  part: a [UNION_PART_PLANES][nq][k] part.  tau [nq] <- the dist at [q][k-1] where that entry is real, else +inf
// (a distance that is no number gives +inf as well: the pruning pass would admit nothing under a NaN radius).
__global__ void knn_exact_tau_kernel(const int* __restrict__ part, int nq, int k, float* __restrict__ tau) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const size_t plane = (size_t)nq * k, at = (size_t)q * k + (k - 1);
    const float dv = __int_as_float(part[UPART_DIST * plane + at]);
    tau[q] = (unsigned)part[UPART_ROW * plane + at] != 0xffffffffu && dv == dv ? dv : __builtin_inff();
}

// grid nq, block 64.  order [nq][nb]: row q holds counts[q] <= nb admitted bucket ids ascending, then -1 -- in place: a seed's entry
// becomes -1.  seeds [nq][KNN_EXACT_SEEDS].  part: the seed part, [UNION_PART_PLANES][nq][k]; its rank plane is rewritten for the real
// entries.  visited [nq] (nullable) <- the seeds plus the admitted buckets that are no seeds.  missed (nullable; debug builds) += the
// seeds the admitted order does not hold.
__global__ __launch_bounds__(64) void knn_exact_split_kernel(int* __restrict__ order, const int* __restrict__ counts, int nb,
                                                             const int* __restrict__ seeds, int* __restrict__ part, int nq, int k,
                                                             int* __restrict__ visited, int* __restrict__ missed) {
    __shared__ int rank_of[KNN_EXACT_SEEDS];
    const int q = blockIdx.x, lane = threadIdx.x;
    int* ord = order + (size_t)q * nb;
    const int n = counts[q] < nb ? counts[q] : nb;
    const int s = lane < KNN_EXACT_SEEDS ? seeds[(size_t)q * KNN_EXACT_SEEDS + lane] : -1;
    int pos = 0;
    bool found = false;
    if (s >= 0) {
        pos = lmi_knn_exact_plan::lower_bound(ord, n, s);
        found = pos < n && ord[pos] == s;
    }
    if (lane < KNN_EXACT_SEEDS) rank_of[lane] = pos;
    const int nseed = __popcll(__ballot(s >= 0)), nfound = __popcll(__ballot(found));
    __syncthreads();   // every search has read the order
    if (found) ord[pos] = -1;
    const size_t plane = (size_t)nq * k;
    int* rk = part + UPART_RANK * plane + (size_t)q * k;
    const int* rw = part + UPART_ROW * plane + (size_t)q * k;
    for (int j = lane; j < k; j += 64) {
        const unsigned r = (unsigned)rk[j];
        if ((unsigned)rw[j] != 0xffffffffu && r < (unsigned)KNN_EXACT_SEEDS) rk[j] = rank_of[r];
    }
    if (lane == 0) {
        if (visited) visited[q] = nseed + n - nfound;
        if (missed && nfound != nseed) atomicAdd(missed, nseed - nfound);
    }
}

}  // namespace lmi
