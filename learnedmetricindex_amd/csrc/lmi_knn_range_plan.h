// lmi_knn_range_plan.h -- the host arithmetic of lmi_knn_range (include/lmi_hip.h): the geometry of the call (lmi_knn_plan.h's pieces,
// splits and query groups, as they are), the device bytes it allocates, where the results of every (query, split) of one (group, piece)
// lie inside that piece's chunk, how the counts of all pieces become lims and the per-query totals, where every (query, piece) run goes
// in the final arrays, and the max_total test.
// Host only and pure: the standard library and lmi_knn_plan.h (whose signatures it uses and never changes), no HIP call --
// lmi_host_knn_range.h passes the counts in and launches from what comes back; tests/host/knn_range_plan_selftest.cpp checks all of it
// on the CPU.
//
// Nothing here can change a result: a query's results are its admitted rows in ascending row order, whichever pieces, splits and
// groups they were counted in.
#pragma once
#include <cstdint>
#include <vector>

#include "lmi_knn_plan.h"

namespace lmi_knn_range_plan {

namespace kp = lmi_knn_plan;

// the k the geometry is made with: the call keeps no lists, so the smallest list decides nothing but the splits' upper bound
constexpr int PLAN_K = 1;

struct Plan {
    kp::Plan g;   // pieces, splits, query groups, pitch, kg; its list_bytes, d_bytes and i_bytes are zero: nothing of them is allocated
    // device bytes beside g's slab, fragments, norms and (host pointers) queries and piece
    int64_t radius_bytes = 0;   // the radii of the whole call
    int64_t count_bytes = 0;    // int [query_rows][splits]: the counts of one (group, piece)
    int64_t offset_bytes = 0;   // long long [query_rows][splits]: where each (query, split) writes inside the piece's chunk
    int64_t workspace_bytes = 0;
};

// (nq, nb, d) as lmi_knn_range accepts them (nq >= 1; nb may be 0); free_bytes, cus, f: as lmi_knn_plan::make_plan takes them.  The
// geometry is lmi_knn's at k = 1 -- memory that is short shrinks pieces and groups exactly as there, judged with that call's lists
// counted in, which errs on the safe side -- and the bytes are this call's own.
// elem: the bytes of an input element, as there (2: lmi_knn_range_f16).
inline Plan make_plan(int64_t nq, int64_t nb, int d, bool l2, bool on_device, int64_t free_bytes, int cus, const kp::Forced& f,
                      int elem = 4) {
    Plan p;
    p.g = kp::make_plan(nq, nb, d, PLAN_K, l2, on_device, free_bytes, cus, f, elem);
    p.g.list_bytes = p.g.d_bytes = p.g.i_bytes = 0;
    p.radius_bytes = nq * 4;
    p.count_bytes = p.g.query_rows * p.g.splits * 4;
    p.offset_bytes = p.g.query_rows * p.g.splits * 8;
    p.g.workspace_bytes = p.g.slab_bytes + p.g.qfrag_bytes + p.g.qn_bytes + p.g.xnh_bytes + p.g.xq_bytes + p.g.xb_bytes;
    p.workspace_bytes = p.g.workspace_bytes + p.radius_bytes + p.count_bytes + p.offset_bytes;
    return p;
}

// whether `counted` results are more than the call may produce (max_total == 0: only memory limits it)
inline bool over_total(int64_t counted, int64_t max_total) { return max_total > 0 && counted > max_total; }

// A non-empty run: the n results query q (of the whole call) has in one piece, contiguous at src of that piece's chunk.
struct Run {
    int64_t q = 0;
    int n = 0;
    long long src = 0;
};
// What one (group, piece) leaves behind for the gather.
struct PieceRuns {
    std::vector<Run> runs;   // ascending q
    int64_t total = 0;       // the chunk's length
};

// The chunk of one (group, piece), query-major: counts [gq][splits] -> off [gq][splits], (query, split) owns
// [off, off + count) of the chunk, so that the splits of a query -- ascending stretches of the piece -- lie back to back in row
// order.  q0: the group's first query.  A negative count is taken as 0.
inline PieceRuns chunk_offsets(const int* counts, int64_t q0, int64_t gq, int splits, long long* off) {
    PieceRuns P;
    int64_t at = 0;
    for (int64_t q = 0; q < gq; ++q) {
        const int64_t first = at;
        for (int s = 0; s < splits; ++s) {
            const size_t i = (size_t)(q * splits + s);
            off[i] = at;
            at += counts[i] > 0 ? counts[i] : 0;
        }
        if (at > first) P.runs.push_back(Run{q0 + q, (int)(at - first), (long long)first});
    }
    P.total = at;
    return P;
}

// The results of a whole call: per_query [nq], what every query has been counted so far.
struct Totals {
    std::vector<int> per_query;
    explicit Totals(int64_t nq = 0) : per_query((size_t)nq, 0) {}
};
// the runs of one (group, piece) enter the totals; returns their sum
inline int64_t add_piece(Totals& tot, const PieceRuns& P) {
    for (const Run& r : P.runs) tot.per_query[(size_t)r.q] += r.n;
    return P.total;
}
// lims [nq + 1]: the exclusive sums of the totals
inline std::vector<int64_t> make_lims(const Totals& tot) {
    std::vector<int64_t> lims(tot.per_query.size() + 1, 0);
    for (size_t q = 0; q < tot.per_query.size(); ++q) lims[q + 1] = lims[q] + tot.per_query[q];
    return lims;
}

// The gather of the call: run i lies at src[i] of ITS piece's chunk and goes to dst[i] of the final arrays; the runs of piece j (in
// the order the pieces were passed) are [first[j], first[j + 1]).  One descriptor per non-empty (query, piece) run.
struct Gather {
    std::vector<long long> src, dst;
    std::vector<int> n;
    std::vector<size_t> first;
};
// pieces: every (group, piece) of the call in the order it ran -- a query's pieces in ascending row order, which is all that is
// needed: a run goes behind the query's earlier runs.
inline Gather gather_of(const std::vector<PieceRuns>& pieces, const std::vector<int64_t>& lims) {
    Gather G;
    std::vector<int64_t> next(lims.begin(), lims.end() - 1);
    G.first.push_back(0);
    for (const PieceRuns& P : pieces) {
        for (const Run& r : P.runs) {
            G.src.push_back(r.src);
            G.dst.push_back((long long)next[(size_t)r.q]);
            G.n.push_back(r.n);
            next[(size_t)r.q] += r.n;
        }
        G.first.push_back(G.n.size());
    }
    return G;
}

}  // namespace lmi_knn_range_plan
