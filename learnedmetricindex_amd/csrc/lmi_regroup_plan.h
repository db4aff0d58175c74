// lmi_regroup_plan.h -- the host arithmetic of lmi_regroup (include/lmi_hip.h states the contract; host: lmi_host_regroup.h; kernels:
// lmi_regroup.h): the checks of the caller's list and map, the list in the form the labelling kernel searches, the ordinal bases of
// the old buckets, the first row of every new label in the sorted words, and the shape of the sort.
//   ordinal    an object's dense position in the source's order: exclusive prefix of the LIVE bucket sizes + row in the bucket.  Not
//              the slab row: an insert may have moved a bucket behind later ones, and spare row-blocks and holes lie between buckets.
//   word       (new label << 32) | ordinal: unique, so ascending words ARE "new label, then the source's order"
//   sort       one tile (n <= T: sorted in LDS, no pass) or cdiv(n, T) tiles and ceil(log2(tiles)) merge passes of lmi_range_sort.h
// Host only and pure: the standard library, no HIP call, no handle; tests/host/regroup_plan_selftest.cpp checks all of it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace lmi_regroup_plan {

constexpr int64_t MAX_LABELS = 1ll << 20;     // the routing kernels' bucket ids (ROUTE_ID_BITS)
constexpr int64_t MIN_TILE_ROWS = 64;
constexpr int64_t MAX_TILE_ROWS = 8192;       // lmi_range_sort_plan's: 64 KiB of 8-byte words
constexpr int64_t DEFAULT_TILE_ROWS = MAX_TILE_ROWS;
constexpr int64_t MAX_MERGE_ROWS = 2048;
// per OBJECT of the source: two buffers of 8-byte words (the sort's ping and pong) and the 4-byte slab row of its ordinal;
// per slab row of the NEW index: the 4-byte source position the gathers read; per list entry: its id and its label, 4 bytes each
constexpr int64_t BYTES_PER_OBJECT = 20, BYTES_PER_NEW_SLAB_ROW = 4, BYTES_PER_LIST_ENTRY = 8;

inline bool power_of_two(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
inline bool tile_rows_ok(int64_t t) { return t == 0 || (power_of_two(t) && t >= MIN_TILE_ROWS && t <= MAX_TILE_ROWS); }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

enum Problem {
    OK = 0,
    BAD_L_NEW,        // value = L_new
    BAD_N,            // value = n
    NULL_LIST,        // n > 0 and ids or labels is NULL
    BAD_LABEL,        // at = the list entry, value = the label
    BAD_MAP,          // at = the old bucket, value = the entry
    NULL_MAP_SHRINKS, // value = L_new (below L)
    DUPLICATE_ID      // value = the id
};
struct Verdict {
    Problem problem = OK;
    int64_t at = 0, value = 0;
};

// The list sorted by id with its labels alongside (what the labelling kernel binary-searches).
struct List {
    std::vector<uint32_t> ids;
    std::vector<int> labels;
};

// Every check that needs no device.  bucket_map nullable ([L] otherwise).  On OK `out` is the sorted list.
inline Verdict check(int L, int64_t L_new, const uint32_t* ids, const int64_t* labels, int64_t n, const int32_t* bucket_map, List& out) {
    out = List();
    if (L_new < 1 || L_new >= MAX_LABELS) return Verdict{BAD_L_NEW, 0, L_new};
    if (n < 0) return Verdict{BAD_N, 0, n};
    if (n > 0 && (!ids || !labels)) return Verdict{NULL_LIST, 0, n};
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] < 0 || labels[i] >= L_new) return Verdict{BAD_LABEL, i, labels[i]};
    if (bucket_map) {
        for (int b = 0; b < L; ++b)
            if (bucket_map[b] < -1 || bucket_map[b] >= L_new) return Verdict{BAD_MAP, b, bucket_map[b]};
    } else if (L_new < L) {
        return Verdict{NULL_MAP_SHRINKS, 0, L_new};
    }
    std::vector<int64_t> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), (int64_t)0);
    const bool sorted = std::is_sorted(ids, ids + n);
    if (!sorted) std::sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return ids[a] < ids[b]; });
    out.ids.resize((size_t)n);
    out.labels.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        out.ids[(size_t)i] = ids[perm[(size_t)i]];
        out.labels[(size_t)i] = (int)labels[perm[(size_t)i]];
    }
    for (int64_t i = 1; i < n; ++i)
        if (out.ids[(size_t)i] == out.ids[(size_t)i - 1]) return Verdict{DUPLICATE_ID, i, (int64_t)out.ids[(size_t)i]};
    return Verdict();
}

// The map the kernel reads: the caller's, or the identity.
inline std::vector<int> map_of(int L, const int32_t* bucket_map) {
    std::vector<int> m((size_t)L);
    for (int b = 0; b < L; ++b) m[(size_t)b] = bucket_map ? (int)bucket_map[b] : b;
    return m;
}

// base[b]: the ordinal of bucket b's first object; base[L]: the objects the source stores.
inline std::vector<int64_t> ordinal_bases(const std::vector<int>& nb_rows) {
    std::vector<int64_t> base(nb_rows.size() + 1, 0);
    for (size_t b = 0; b < nb_rows.size(); ++b) base[b + 1] = base[b] + nb_rows[b];
    return base;
}

// The first bucket that keeps unnamed objects although its map entry is -1 (left[b]: how many), or -1.
inline int first_unmapped(const std::vector<int>& left) {
    for (size_t b = 0; b < left.size(); ++b)
        if (left[b] > 0) return (int)b;
    return -1;
}

struct SortPlan {
    int64_t n = 0, tile_rows = DEFAULT_TILE_ROWS, tiles = 0, merge_rows = MAX_MERGE_ROWS, merge_pieces = 0;
    int passes = 0;
    // what the call's maps take, the small per-bucket tables aside (one buffer of words less when one tile holds them all)
    int64_t map_bytes(int64_t new_slab_rows, int64_t n_list) const {
        return (BYTES_PER_OBJECT - (passes ? 0 : 8)) * n + BYTES_PER_NEW_SLAB_ROW * new_slab_rows + BYTES_PER_LIST_ENTRY * n_list;
    }
};
inline SortPlan sort_plan(int64_t n, int64_t forced_tile_rows) {
    SortPlan P;
    P.n = n;
    P.tile_rows = forced_tile_rows > 0 ? forced_tile_rows : DEFAULT_TILE_ROWS;
    P.merge_rows = std::min(MAX_MERGE_ROWS, P.tile_rows);
    P.tiles = cdiv(n, P.tile_rows);
    for (int64_t run = P.tile_rows; run < n; run <<= 1) ++P.passes;
    P.merge_pieces = P.passes ? cdiv(n, P.merge_rows) : 0;
    return P;
}

// The order rule on the host (the self-test's reference): src[j] = the ordinal of the j-th object of the new order.
inline std::vector<int64_t> new_order(const std::vector<int>& new_label_of_ordinal) {
    std::vector<int64_t> src(new_label_of_ordinal.size());
    std::iota(src.begin(), src.end(), (int64_t)0);
    std::stable_sort(src.begin(), src.end(), [&](int64_t a, int64_t b) { return new_label_of_ordinal[(size_t)a] < new_label_of_ordinal[(size_t)b]; });
    return src;
}

}  // namespace lmi_regroup_plan
