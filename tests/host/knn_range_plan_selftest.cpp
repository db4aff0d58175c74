// knn_range_plan_selftest.cpp -- stand-alone check of lmi_knn_range's host arithmetic (csrc/lmi_knn_range_plan.h: pure host code) on the
// CPU, meant for -fsanitize=address,undefined (tests/test_knn_range_host.py builds and runs it).  A simulated call: a seeded base of
// "admitted" (query, row) pairs is counted stretch by stretch exactly as the kernels address it -- pieces, splits and query groups
// with ragged ends -- and emitted into per-piece chunks at the planned offsets, then gathered; the final arrays must hold every
// query's admitted rows in ascending row order, whatever the geometry.  Beside it: empty runs produce no descriptor, the byte counts
// add up and hold no lists, offsets beyond 2^31 results stay exact, and the max_total edge.
#include "lmi_knn_range_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace lmi_knn_range_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

// whether row r is admitted for query q: a hash; `dense` queries admit everything, `none` queries nothing
static bool admitted(int64_t q, int64_t r, int mode) {
    if (q % 5 == 3) return false;            // queries with empty results
    if (mode == 1 || q % 7 == 2) return true;   // everything
    uint64_t h = (uint64_t)q * 0x9e3779b97f4a7c15ull ^ (uint64_t)r * 0xc2b2ae3d27d4eb4full;
    h ^= h >> 29;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 32;
    return h % 11 == 0;
}

static void simulate(int64_t nq, int64_t nb, int d, bool l2, bool dev, const kp::Forced& f, int mode) {
    const Plan P = make_plan(nq, nb, d, l2, dev, 0, 256, f);
    const kp::Plan& p = P.g;
    // the bytes: lmi_knn's buffers without lists and without D / I, plus the radii, the counts and the offsets
    EXPECT(p.list_bytes == 0 && p.d_bytes == 0 && p.i_bytes == 0);
    EXPECT(P.radius_bytes == 4 * nq && P.count_bytes == 4 * p.query_rows * p.splits && P.offset_bytes == 8 * p.query_rows * p.splits);
    EXPECT(P.workspace_bytes == p.slab_bytes + p.qfrag_bytes + p.qn_bytes + p.xnh_bytes + p.xq_bytes + p.xb_bytes + P.radius_bytes + P.count_bytes + P.offset_bytes);
    const kp::Plan k1 = kp::make_plan(nq, nb, d, PLAN_K, l2, dev, 0, 256, f);
    EXPECT(p.piece_rows == k1.piece_rows && p.splits == k1.splits && p.query_rows == k1.query_rows && p.pieces == k1.pieces && p.pitch == k1.pitch);
    if (dev) EXPECT(p.xq_bytes == 0 && p.xb_bytes == 0);

    struct Chunk { std::vector<float> D; std::vector<uint32_t> I; };
    std::vector<Chunk> chunks;
    std::vector<PieceRuns> runs;
    Totals tot(nq);
    std::vector<int> counts((size_t)(p.query_rows * p.splits));
    std::vector<long long> off(counts.size());
    int64_t counted = 0;
    for (int64_t g = 0; g < p.query_groups && p.pieces > 0; ++g) {
        int64_t q0, q1;
        kp::group_range(p, g, &q0, &q1);
        const int64_t gq = q1 - q0;
        for (int64_t i = 0; i < p.pieces; ++i) {
            int64_t r0, r1;
            kp::piece_range(p, i, &r0, &r1);
            // the count kernel: block (q, s) counts its stretch
            for (int64_t q = 0; q < gq; ++q)
                for (int s = 0; s < p.splits; ++s) {
                    int64_t a, b;
                    kp::split_range(r1 - r0, p.splits, s, &a, &b);
                    int c = 0;
                    for (int64_t r = a; r < b; ++r) c += admitted(q0 + q, r0 + r, mode);
                    counts[(size_t)(q * p.splits + s)] = c;
                }
            const PieceRuns R = chunk_offsets(counts.data(), q0, gq, p.splits, off.data());
            // offsets are the exclusive sums in (query, split) order; one run per query with results, none for the others
            int64_t at = 0;
            size_t nr = 0;
            for (int64_t q = 0; q < gq; ++q) {
                int64_t mine = 0;
                for (int s = 0; s < p.splits; ++s) {
                    EXPECT(off[(size_t)(q * p.splits + s)] == at + mine);
                    mine += counts[(size_t)(q * p.splits + s)];
                }
                if (mine > 0) {
                    EXPECT(nr < R.runs.size() && R.runs[nr].q == q0 + q && R.runs[nr].n == mine && R.runs[nr].src == at);
                    ++nr;
                }
                at += mine;
            }
            EXPECT(nr == R.runs.size() && R.total == at);
            counted += add_piece(tot, R);
            runs.push_back(R);
            chunks.emplace_back();
            // the emit kernel: block (q, s) writes its admitted rows from its offset on, in row order
            Chunk& C = chunks.back();
            C.D.assign((size_t)R.total, -1.0f);
            C.I.assign((size_t)R.total, 0xffffffffu);
            for (int64_t q = 0; q < gq; ++q)
                for (int s = 0; s < p.splits; ++s) {
                    int64_t a, b;
                    kp::split_range(r1 - r0, p.splits, s, &a, &b);
                    long long o = off[(size_t)(q * p.splits + s)];
                    for (int64_t r = a; r < b; ++r)
                        if (admitted(q0 + q, r0 + r, mode)) {
                            EXPECT(o < R.total && C.I[(size_t)o] == 0xffffffffu);
                            C.D[(size_t)o] = (float)(q0 + q);
                            C.I[(size_t)o++] = (uint32_t)(r0 + r);
                        }
                }
        }
    }
    EXPECT(runs.size() == (size_t)(p.pieces > 0 ? p.query_groups * p.pieces : 0));
    const std::vector<int64_t> lims = make_lims(tot);
    EXPECT(lims.size() == (size_t)nq + 1 && lims[0] == 0 && lims.back() == counted);
    const Gather G = gather_of(runs, lims);
    EXPECT(G.first.size() == runs.size() + 1 && G.first[0] == 0 && G.first.back() == G.n.size() && G.src.size() == G.n.size() && G.dst.size() == G.n.size());
    std::vector<float> D((size_t)counted, -2.0f);
    std::vector<uint32_t> I((size_t)counted, 0xfffffffeu);
    for (size_t j = 0; j < runs.size(); ++j) {
        EXPECT(G.first[j + 1] - G.first[j] == runs[j].runs.size());
        for (size_t i = G.first[j]; i < G.first[j + 1]; ++i) {
            EXPECT(G.n[i] > 0);   // one descriptor per NON-EMPTY (query, piece) run
            for (int t = 0; t < G.n[i]; ++t) {
                const size_t to = (size_t)(G.dst[i] + t), from = (size_t)(G.src[i] + t);
                EXPECT(to < D.size() && from < chunks[j].D.size() && I[to] == 0xfffffffeu);   // inside, and written once
                D[to] = chunks[j].D[from];
                I[to] = chunks[j].I[from];
            }
        }
    }
    // the final arrays: every query's admitted rows, ascending
    for (int64_t q = 0; q < nq; ++q) {
        int64_t at = lims[(size_t)q];
        for (int64_t r = 0; r < nb; ++r)
            if (admitted(q, r, mode)) {
                EXPECT(at < lims[(size_t)q + 1] && I[(size_t)at] == (uint32_t)r && D[(size_t)at] == (float)q);
                ++at;
            }
        EXPECT(at == lims[(size_t)q + 1] && tot.per_query[(size_t)q] == lims[(size_t)q + 1] - lims[(size_t)q]);
        if (q % 5 == 3) EXPECT(lims[(size_t)q + 1] == lims[(size_t)q]);
    }
    // the max_total edge at this call's total
    EXPECT(!over_total(counted, 0) && !over_total(counted, counted) && !over_total(counted, counted + 1));
    if (counted > 1) EXPECT(over_total(counted, counted - 1));
}

int main() {
    const kp::Forced forced[] = {{0, 0, 0}, {64, 1, 0}, {100, 3, 32}, {257, 8, 0}, {1000, 2, 40}, {1, 1, 1}, {7, 5, 3}, {333, 16, 33}};
    const int64_t nqs[] = {1, 33, 67};
    const int64_t nbs[] = {0, 1, 63, 64, 65, 777, 2011};
    for (int64_t nq : nqs)
        for (int64_t nb : nbs)
            for (const kp::Forced& f : forced)
                for (int dev = 0; dev < 2; ++dev)
                    for (int mode = 0; mode < 2; ++mode) {
                        if (mode == 1 && nq * nb > 70000) continue;   // everything admitted: the small shapes say it all
                        simulate(nq, nb, 45, dev == 1, dev == 1, f, mode);
                    }
    // empty counts: no run, offsets all zero
    {
        const int z[6] = {0, 0, 0, 0, 0, 0};
        long long off[6] = {9, 9, 9, 9, 9, 9};
        const PieceRuns R = chunk_offsets(z, 10, 3, 2, off);
        EXPECT(R.total == 0 && R.runs.empty());
        for (long long o : off) EXPECT(o == 0);
        Totals tot(13);
        EXPECT(add_piece(tot, R) == 0);
        const std::vector<int64_t> lims = make_lims(tot);
        EXPECT(lims.size() == 14 && lims.back() == 0);
        const Gather G = gather_of({R}, lims);
        EXPECT(G.n.empty() && G.first.size() == 2 && G.first[1] == 0);
        EXPECT(make_lims(Totals(0)).size() == 1 && gather_of({}, make_lims(Totals(0))).first.size() == 1);
    }
    // beyond 2^31 results: 5 queries (one empty) x 2 pieces, every run 2^30 - 1 long -- a query's total stays below 2^31 as nb < 2^31
    // keeps it, the call's passes 2^33: lims, the targets and a chunk's offsets stay exact in 64 bits
    {
        const int big = (1 << 30) - 1;
        Totals tot(5);
        std::vector<PieceRuns> runs;
        int64_t counted = 0;
        for (int i = 0; i < 2; ++i) {
            const int counts[10] = {big - 1, 1, 0, 0, big, 0, 0, big, 1, big - 1};   // query 1 is empty; two splits
            long long off[10];
            runs.push_back(chunk_offsets(counts, 0, 5, 2, off));
            EXPECT(off[0] == 0 && off[1] == big - 1 && off[2] == big && off[3] == big && off[4] == big && off[5] == 2ll * big);
            EXPECT(off[6] == 2ll * big && off[7] == 2ll * big && off[8] == 3ll * big && off[9] == 3ll * big + 1);
            EXPECT(runs.back().total == 4ll * big && runs.back().runs.size() == 4 && runs.back().runs[1].q == 2 && runs.back().runs[1].src == big);
            EXPECT(runs.back().runs[3].q == 4 && runs.back().runs[3].src == 3ll * big && runs.back().runs[3].n == big);
            counted += add_piece(tot, runs.back());
            EXPECT(over_total(counted, counted - 1) && !over_total(counted, counted));
        }
        EXPECT(counted == 8ll * big && counted > (1ll << 32));
        const std::vector<int64_t> lims = make_lims(tot);
        EXPECT(lims[1] == 2ll * big && lims[2] == 2ll * big && lims[3] == 4ll * big && lims[4] == 6ll * big && lims[5] == 8ll * big);
        const Gather G = gather_of(runs, lims);
        EXPECT(G.n.size() == 8 && G.first[1] == 4);
        for (int i = 0; i < 2; ++i) {
            const long long dst[4] = {0, 2ll * big, 4ll * big, 6ll * big}, src[4] = {0, big, 2ll * big, 3ll * big};
            for (int j = 0; j < 4; ++j)
                EXPECT(G.dst[(size_t)(4 * i + j)] == dst[j] + (long long)i * big && G.src[(size_t)(4 * i + j)] == src[j] && G.n[(size_t)(4 * i + j)] == big);
        }
    }
    // the automatic geometry of a full-size call is lmi_knn's, and its bytes hold no lists
    {
        const Plan P = make_plan(10000, 10000000, 45, false, true, (int64_t)200 << 30, 256, kp::Forced{});
        const kp::Plan k = kp::make_plan(10000, 10000000, 45, PLAN_K, false, true, (int64_t)200 << 30, 256, kp::Forced{});
        EXPECT(P.g.pieces == k.pieces && P.g.splits == k.splits && P.g.query_groups == k.query_groups && P.g.query_groups == 2);
        EXPECT(P.workspace_bytes == k.workspace_bytes - k.list_bytes + 4 * 10000 + 12 * P.g.query_rows * P.g.splits);
    }
    std::printf("knn range plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
