// lmi_knn_exact_plan.h -- the arithmetic of the exact k-NN through the index (lmi_search_knn_exact; include/lmi_hip.h states the
// contract; host: lmi_host_knn_exact.h; kernels: lmi_knn_exact.h; DESIGN.md 5.14.7 holds the proof).
//   word          the 64-bit word of one (query, bucket) pair of the bound pass: the order-preserving image of the rule's optimistic
//                 bound (lmi_cover_plan::bound_ip / bound_l2) above the bucket id.  A SMALLER word is the more promising bucket;
//   seed budget   how many of a query's most promising buckets are scanned first, to get it a finite radius;
//   split         where a bucket id lies in the admitted order: the rank a seed's results carry in the merge, and the slot of the
//                 rest order that the seed leaves empty;
//   groups        the cut of the queries into groups of the bound pass.
// The kernels run image_of / word_of / seeds_done / lower_bound as they stand here; seeds_of and split_of restate the two wave kernels
// over whole rows for tests/host/knn_exact_selftest.cpp.  Pure: no HIP call, no handle.
#pragma once
#include "lmi_cover_plan.h"

namespace lmi_knn_exact_plan {

constexpr int MAX_SEEDS = 32;                       // LMI_KNN_EXACT_MAX_SEEDS
constexpr unsigned long long NO_WORD = ~0ull;       // a bucket without rows: behind every real word, never taken
constexpr int64_t WORD_BYTES = 256ll << 20;         // a group's words stay below this where one query's row allows it

// ---- the word ----
// ascending image of a binary32: a < b (as numbers) => image(a) < image(b); -0 and +0 share one image; a NaN maps to 0, the best
// value there is, so that it cannot hide a bucket
LMI_COVER_HD inline uint32_t image_of(float v) {
    if (v != v) return 0u;
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the float an image stands for (the NaN's image reads back as a NaN of the negative half; only the self-test looks)
LMI_COVER_HD inline float value_of(uint32_t image) {
    const uint32_t u = (image & 0x80000000u) ? (image & 0x7fffffffu) : ~image;
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}
// bound: bound_ip (the largest similarity a row of the ball could have: negated, so that smaller is better) or bound_l2 (the smallest
// distance), rounded to binary32.  Words of one query are unique: the bucket id is part of them.
LMI_COVER_HD inline unsigned long long word_of(int metric, double bound, uint32_t bucket) {
    const float f = metric == lmi_cover_plan::METRIC_IP ? -(float)bound : (float)bound;
    return ((unsigned long long)image_of(f) << 32) | bucket;
}
LMI_COVER_HD inline uint32_t bucket_of(unsigned long long word) { return (uint32_t)word; }
LMI_COVER_HD inline float bound_of(int metric, unsigned long long word) {
    const float f = value_of((uint32_t)(word >> 32));
    return metric == lmi_cover_plan::METRIC_IP ? -f : f;
}

// ---- the seed budget ----
// buckets are taken in ascending word order until their live rows reach k, or MAX_SEEDS of them are taken, or none is left
LMI_COVER_HD inline bool seeds_done(long long rows, int k, int taken) { return rows >= k || taken >= MAX_SEEDS; }

// knn_exact_seed_kernel over one query's row: words [L], n_b [L] -> seeds [MAX_SEEDS] ascending bucket ids, then -1; returns the number
inline int seeds_of(const unsigned long long* words, const int* n_b, int L, int k, int* seeds) {
    int taken = 0;
    long long rows = 0;
    unsigned long long last = 0;
    for (int i = 0; i < MAX_SEEDS; ++i) seeds[i] = -1;
    for (;;) {
        unsigned long long best = NO_WORD;
        for (int b = 0; b < L; ++b)
            if (words[b] < best && (taken == 0 || words[b] > last)) best = words[b];
        if (best == NO_WORD) break;
        last = best;
        const int b = (int)bucket_of(best);
        int at = taken++;   // insertion keeps the ids ascending
        while (at > 0 && seeds[at - 1] > b) { seeds[at] = seeds[at - 1]; --at; }
        seeds[at] = b;
        rows += n_b[b];
        if (seeds_done(rows, k, taken)) break;
    }
    return taken;
}

// ---- the split ----
// the first position of order [0, n) (ascending) whose entry is >= b; n if there is none
LMI_COVER_HD inline int lower_bound(const int* order, int n, int b) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (order[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// knn_exact_split_kernel over one query's rows: order [0, n) the admitted buckets, ascending (in place: a seed's entry becomes -1);
// seeds as seeds_of wrote them; rank_of [MAX_SEEDS] <- position of seed i in the admitted order.  Returns the buckets the two scans
// score between them: the seeds and the admitted ones that are no seeds; *missed <- the seeds the order does not hold (the rule
// admits every seed: 0).
inline int split_of(int* order, int n, const int* seeds, int* rank_of, int* missed) {
    int nseed = 0, found = 0;
    int pos[MAX_SEEDS];
    for (int i = 0; i < MAX_SEEDS; ++i) {
        rank_of[i] = pos[i] = -1;
        if (seeds[i] < 0) continue;
        ++nseed;
        rank_of[i] = lower_bound(order, n, seeds[i]);
        if (rank_of[i] < n && order[rank_of[i]] == seeds[i]) { pos[i] = rank_of[i]; ++found; }
    }
    for (int i = 0; i < MAX_SEEDS; ++i)
        if (pos[i] >= 0) order[pos[i]] = -1;
    if (missed) *missed = nseed - found;
    return nseed + n - found;
}

// ---- groups ----
// queries per group of the bound pass: the pruning pass's (the same hook, lmi_cover_set_geometry), fewer where the group's words
// would pass WORD_BYTES (at least 1); a forced value stands
inline int64_t query_rows_for(int64_t forced, int64_t nq, int64_t L) {
    int64_t rows = lmi_cover_plan::query_rows_for(forced, nq, L);
    if (forced <= 0) {
        const int64_t fit = WORD_BYTES / (8 * (L > 0 ? L : 1));
        if (rows > fit) rows = fit;
    }
    return rows < 1 ? 1 : rows;
}
inline int64_t word_bytes(int64_t query_rows, int64_t L) { return 8 * query_rows * L; }

}  // namespace lmi_knn_exact_plan
