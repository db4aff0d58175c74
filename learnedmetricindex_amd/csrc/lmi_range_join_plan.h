// lmi_range_join_plan.h -- the host arithmetic of the join of range parts (lmi_join_range_parts, lmi_allgather_join_range;
// include/lmi_hip.h): from the ranks' per-(query, rank t) counts to the joined result's run starts and lims, the owner of every
// non-empty run, where that run lies inside its owner's arrays, and the table of copy pieces the kernel (lmi_range_join.h) works off.
// A part is a range result in (query, t, row) order, so the run of (q, t) of part r lies behind every earlier (q', t') run of part r:
// its offset is the exclusive sum of counts[r] in (q, t) order.  In the joined result it lies behind every earlier run of ANY part:
// first[q * nb + t].  Every (q, t) names one bucket and one part owns it, so a run comes whole from one part and the join is a gather.
// Host only and pure: the standard library, no HIP call, no handle; tests/host/range_join_selftest.cpp checks all of it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lmi_range_join_plan {

constexpr int64_t DEFAULT_PIECE_ROWS = 4096;   // results one block copies: a longer run is cut, so that no run is one block's work
constexpr int64_t MAX_PIECE_ROWS = 1ll << 30;

inline int64_t piece_rows_for(int64_t forced) { return forced > 0 ? std::min(forced, MAX_PIECE_ROWS) : DEFAULT_PIECE_ROWS; }

// why a set of counts is not planned
enum Problem { OK = 0, NEGATIVE_COUNT, TWO_OWNERS, OVER_TOTAL };
struct Verdict {
    Problem problem = OK;
    int64_t q = 0;       // NEGATIVE_COUNT, TWO_OWNERS: the query
    int t = 0;           //                             the rank of the bucket in the query's order
    int part_a = 0;      // NEGATIVE_COUNT: the part; TWO_OWNERS: the lower claimant
    int part_b = 0;      // TWO_OWNERS: the other claimant
    int64_t value = 0;   // NEGATIVE_COUNT: the count; OVER_TOTAL: the grand total
};

struct Plan {
    int world = 0, nb = 0;
    int64_t nq = 0, piece_rows = DEFAULT_PIECE_ROWS;
    int64_t total = 0, runs = 0, largest_part = 0;
    std::vector<int64_t> part_total;   // [world]
    std::vector<int> pair_count;       // [nq * nb]: the sum over the parts = the owner's count
    std::vector<int> owner;            // [nq * nb]: the part whose count is > 0, -1 for an empty (q, t)
    std::vector<int64_t> run_src;      // [nq * nb]: where the run begins in its owner's arrays (0 for an empty one)
    std::vector<int64_t> first;        // [nq * nb + 1]: where it begins in the joined arrays
    std::vector<int64_t> lims;         // [nq + 1]: lims[q] = first[q * nb]
    // the pieces, parallel arrays: n[i] results of part[i] from src[i] of that part's arrays to dst[i] of the joined ones
    std::vector<int> piece_part, piece_n;
    std::vector<long long> piece_src, piece_dst;
};

// counts [world][nq][nb]; max_total 0: no limit.  On a problem `out` is left in an unspecified state and must not be used.
inline Verdict make_plan(int world, int64_t nq, int nb, const int32_t* counts, int64_t forced_piece_rows, int64_t max_total, Plan& out) {
    Verdict v;
    const int64_t pairs = nq * nb;
    out = Plan();
    out.world = world;
    out.nb = nb;
    out.nq = nq;
    out.piece_rows = piece_rows_for(forced_piece_rows);
    out.part_total.assign((size_t)world, 0);
    out.pair_count.assign((size_t)pairs, 0);
    out.owner.assign((size_t)pairs, -1);
    out.run_src.assign((size_t)pairs, 0);
    out.first.assign((size_t)pairs + 1, 0);
    out.lims.assign((size_t)nq + 1, 0);
    for (int64_t s = 0; s < pairs; ++s) {
        for (int r = 0; r < world; ++r) {
            const int32_t c = counts[(size_t)r * pairs + s];
            if (c < 0) return Verdict{NEGATIVE_COUNT, s / nb, (int)(s % nb), r, 0, c};
            if (c == 0) continue;
            if (out.owner[(size_t)s] >= 0) return Verdict{TWO_OWNERS, s / nb, (int)(s % nb), out.owner[(size_t)s], r, 0};
            out.owner[(size_t)s] = r;
            out.pair_count[(size_t)s] = c;
            out.run_src[(size_t)s] = out.part_total[(size_t)r];   // the exclusive sum of part r's counts in (q, t) order
            out.part_total[(size_t)r] += c;
        }
        out.first[(size_t)s + 1] = out.first[(size_t)s] + out.pair_count[(size_t)s];
        out.runs += out.pair_count[(size_t)s] > 0;
    }
    out.total = out.first[(size_t)pairs];
    for (int64_t q = 0; q <= nq; ++q) out.lims[(size_t)q] = out.first[(size_t)(q * nb)];
    for (int64_t t : out.part_total) out.largest_part = std::max(out.largest_part, t);
    if (max_total > 0 && out.total > max_total) {
        v.problem = OVER_TOTAL;
        v.value = out.total;
        return v;
    }
    for (int64_t s = 0; s < pairs; ++s) {
        const int64_t n = out.pair_count[(size_t)s];
        for (int64_t at = 0; at < n; at += out.piece_rows) {
            out.piece_part.push_back(out.owner[(size_t)s]);
            out.piece_src.push_back(out.run_src[(size_t)s] + at);
            out.piece_dst.push_back(out.first[(size_t)s] + at);
            out.piece_n.push_back((int)std::min(out.piece_rows, n - at));
        }
    }
    return v;
}

}  // namespace lmi_range_join_plan
