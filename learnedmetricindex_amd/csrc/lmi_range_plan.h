// lmi_range_plan.h -- the host arithmetic of a range search (lmi_scan_range and the two search forms; include/lmi_hip.h): which
// (query, rank) a slot of the union scan's tables belongs to, where a slot's results lie inside its wave's chunk, how the counts of
// every (query, rank) become lims, where every slot's run goes in the final arrays, and the max_total test.
// Host only and pure: the standard library and lmi_union_plan.h (whose plan and tables it reads and never changes), no HIP call, no
// handle -- lmi_host_range.h passes the counts in and launches from what comes back; tests/host/range_plan_selftest.cpp checks all of
// it on the CPU.
#pragma once
#include <cstdint>
#include <vector>

#include "lmi_union_plan.h"

namespace lmi_range_plan {

namespace up = lmi_union_plan;

// the k the union plan is made with: a range search keeps no lists, so the smallest list decides the query groups
constexpr int PLAN_K = 1;

// Slot i of a group's slot table is (query, rank) pair s = q * nb + t of the group (build_tables numbers a slot's list by it).
inline int64_t slot_pair(const up::Plan& p, const up::Tables& T, int64_t i) { return T.slots[(size_t)i].list / p.list_rows; }

// (The arrays parallel to a group's slot table that the range kernels read -- the global query of slot i and the slab position of its
// bucket's row 0 -- are the tables' own scan_q and scan_pos0.)

// A wave's chunk: slot i of the wave (counts[i] results) owns [off[i], off[i] + counts[i]) of it; returns the chunk's length.
inline int64_t chunk_offsets(const int* counts, int64_t slots, long long* off) {
    int64_t at = 0;
    for (int64_t i = 0; i < slots; ++i) {
        off[i] = at;
        at += counts[i] > 0 ? counts[i] : 0;
    }
    return at;
}

// whether `counted` results are more than the call may produce (max_total == 0: only memory limits it)
inline bool over_total(int64_t counted, int64_t max_total) { return max_total > 0 && counted > max_total; }

// The results of a whole call.  pair_count [nq][nb]: the results of every (query, rank) -- 0 for a rank that is no slot (a hole, an
// empty bucket, one its filter emptied).
struct Totals {
    int64_t nq = 0;
    int nb = 0;
    std::vector<int> pair_count;
    explicit Totals(int64_t nq_ = 0, int nb_ = 0) : nq(nq_), nb(nb_), pair_count((size_t)(nq_ * nb_), 0) {}
};
// the counts of one wave of group T (counts[i]: slot W.slot0 + i) enter the totals; returns the wave's sum
inline int64_t add_wave(Totals& tot, const up::Plan& p, const up::Tables& T, const up::Wave& W, const int* counts) {
    int64_t sum = 0;
    for (int64_t i = 0; i < W.slots; ++i) {
        const int64_t s = slot_pair(p, T, W.slot0 + i);
        tot.pair_count[(size_t)(T.q0 * p.nb + s)] = counts[i];
        sum += counts[i];
    }
    return sum;
}

// first [nq * nb + 1]: the exclusive sums of pair_count -- where the run of (query, rank) begins in the final arrays: behind every
// earlier query's results and the query's own earlier ranks'.  lims[q] = first[q * nb].
inline std::vector<int64_t> run_starts(const Totals& tot) {
    std::vector<int64_t> first(tot.pair_count.size() + 1, 0);
    for (size_t i = 0; i < tot.pair_count.size(); ++i) first[i + 1] = first[i] + tot.pair_count[i];
    return first;
}
inline std::vector<int64_t> make_lims(const Totals& tot, const std::vector<int64_t>& first) {
    std::vector<int64_t> lims((size_t)tot.nq + 1, 0);
    for (int64_t q = 0; q <= tot.nq; ++q) lims[(size_t)q] = first[(size_t)(q * tot.nb)];
    return lims;
}

// The gather of one wave: slot i's run of n[i] results lies at src[i] of the wave's chunk and goes to dst[i] of the final arrays.
struct Gather {
    std::vector<long long> src, dst;
    std::vector<int> n;
};
// counts, off: the wave's (as chunk_offsets made them); first: run_starts of the finished totals
inline Gather gather_of(const up::Plan& p, const up::Tables& T, const up::Wave& W, const int* counts, const long long* off,
                        const std::vector<int64_t>& first) {
    Gather G;
    G.src.assign(off, off + W.slots);
    G.n.assign(counts, counts + W.slots);
    G.dst.resize((size_t)W.slots);
    for (int64_t i = 0; i < W.slots; ++i) G.dst[(size_t)i] = first[(size_t)(T.q0 * p.nb + slot_pair(p, T, W.slot0 + i))];
    return G;
}

}  // namespace lmi_range_plan
