// range_join_selftest.cpp -- stand-alone check of the host arithmetic of the join of range parts (csrc/lmi_range_join_plan.h: pure
// host code) on the CPU, meant for -fsanitize=address,undefined (tests/test_range_sharded_host.py builds and runs it).  For random
// counts with one owner per (query, t) -- worlds of 1 to 64, parts that are empty, runs of 0, 1 and thousands of results -- and for
// piece_rows of 1, 64, 100 and 4096:
//   - the pieces tile [0, total) of the result exactly once;
//   - the pieces tile every part's [0, part total) exactly once;
//   - a run's pieces are consecutive, begin at the run's start on both sides, and none exceeds piece_rows;
//   - runs are in (q, t) order and back to back; lims is monotone and equals the row sums;
//   - the pair counts are the sum over the parts, the owner is the part that holds the run;
//   - a (q, t) with two claimants, a negative count and a total above max_total are reported, not planned;
//   - worlds of 1 and 64, a part that is empty, nq = 0.
#include "lmi_range_join_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace lmi_range_join_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

// counts [world][nq][nb] with one owner per pair; `empty_part` (or -1) owns nothing
static std::vector<int32_t> random_counts(std::mt19937& rng, int world, int64_t nq, int nb, int empty_part, int big) {
    auto rnd = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    std::vector<int32_t> c((size_t)(world * nq * nb), 0);
    for (int64_t s = 0; s < nq * nb; ++s) {
        int r = rnd(0, world - 1);
        if (r == empty_part) r = (r + 1) % world;
        if (r == empty_part) continue;   // a world of one whose only part is the empty one
        const int kind = rnd(0, 9);
        const int n = kind < 3 ? 0 : kind < 5 ? 1 : kind < 8 ? rnd(2, 130) : kind == 8 ? 64 * rnd(1, 3) : rnd(1, big);
        c[(size_t)r * (size_t)(nq * nb) + (size_t)s] = n;
    }
    return c;
}

static void check_plan(int world, int64_t nq, int nb, const std::vector<int32_t>& c, int64_t piece_rows) {
    Plan P;
    const Verdict v = make_plan(world, nq, nb, c.data(), piece_rows, 0, P);
    EXPECT(v.problem == OK);
    const int64_t pairs = nq * nb, pr = piece_rows_for(piece_rows);
    EXPECT(P.piece_rows == pr && P.world == world && P.nq == nq && P.nb == nb);
    EXPECT((int64_t)P.lims.size() == nq + 1 && (int64_t)P.first.size() == pairs + 1 && (int64_t)P.part_total.size() == world);
    // totals, owners, pair counts, run starts: against sums formed here
    std::vector<int64_t> ptot((size_t)world, 0);
    int64_t total = 0, runs = 0, largest = 0;
    EXPECT(P.lims[0] == 0 && P.first[0] == 0);
    for (int64_t s = 0; s < pairs; ++s) {
        int64_t sum = 0;
        int own = -1;
        for (int r = 0; r < world; ++r) {
            const int32_t n = c[(size_t)r * (size_t)pairs + (size_t)s];
            sum += n;
            if (n > 0) own = r;
        }
        EXPECT(P.pair_count[(size_t)s] == sum && P.owner[(size_t)s] == own);
        EXPECT(P.first[(size_t)s] == total);   // runs in (q, t) order, back to back
        if (own >= 0) {
            EXPECT(P.run_src[(size_t)s] == ptot[(size_t)own]);   // the exclusive sum of the owner's counts
            ptot[(size_t)own] += sum;
            ++runs;
        }
        total += sum;
    }
    EXPECT(P.first[(size_t)pairs] == total && P.total == total && P.runs == runs);
    for (int r = 0; r < world; ++r) {
        EXPECT(P.part_total[(size_t)r] == ptot[(size_t)r]);
        largest = std::max(largest, ptot[(size_t)r]);
    }
    EXPECT(P.largest_part == largest);
    for (int64_t q = 0; q < nq; ++q) {
        int64_t row = 0;
        for (int t = 0; t < nb; ++t) row += P.pair_count[(size_t)(q * nb + t)];
        EXPECT(P.lims[(size_t)q + 1] - P.lims[(size_t)q] == row && row >= 0);   // monotone, equal to the row sums
    }
    EXPECT(P.lims[(size_t)nq] == total);
    // the pieces
    const size_t np = P.piece_n.size();
    EXPECT(P.piece_part.size() == np && P.piece_src.size() == np && P.piece_dst.size() == np);
    std::vector<char> hit((size_t)total, 0);
    std::vector<std::vector<char>> phit((size_t)world);
    for (int r = 0; r < world; ++r) phit[(size_t)r].assign((size_t)ptot[(size_t)r], 0);
    size_t i = 0;
    for (int64_t s = 0; s < pairs; ++s) {   // a run's pieces are consecutive in the table, in order, and cover the run from its start
        int64_t left = P.pair_count[(size_t)s], at = 0;
        while (left > 0) {
            EXPECT(i < np);
            const int64_t n = P.piece_n[i];
            EXPECT(n >= 1 && n <= pr && n == std::min(pr, left));
            EXPECT(P.piece_part[i] == P.owner[(size_t)s]);
            EXPECT(P.piece_dst[i] == P.first[(size_t)s] + at && P.piece_src[i] == P.run_src[(size_t)s] + at);
            const int r = P.piece_part[i];
            EXPECT(P.piece_dst[i] >= 0 && P.piece_dst[i] + n <= total && P.piece_src[i] >= 0 && P.piece_src[i] + n <= ptot[(size_t)r]);
            for (int64_t j = 0; j < n; ++j) {
                EXPECT(!hit[(size_t)(P.piece_dst[i] + j)] && !phit[(size_t)r][(size_t)(P.piece_src[i] + j)]);
                hit[(size_t)(P.piece_dst[i] + j)] = 1;
                phit[(size_t)r][(size_t)(P.piece_src[i] + j)] = 1;
            }
            left -= n, at += n, ++i;
        }
    }
    EXPECT(i == np);
    for (char h : hit) EXPECT(h == 1);   // [0, total) exactly once
    for (const auto& ph : phit)
        for (char h : ph) EXPECT(h == 1);   // every part's [0, part total) exactly once
    // max_total: passes at the exact total, reported one below it
    if (total > 0) {
        Plan Q;
        EXPECT(make_plan(world, nq, nb, c.data(), piece_rows, total, Q).problem == OK && Q.piece_n.size() == np);
        if (total > 1) {
            const Verdict over = make_plan(world, nq, nb, c.data(), piece_rows, total - 1, Q);
            EXPECT(over.problem == OVER_TOTAL && over.value == total && Q.piece_n.empty());
        }
    }
}

int main() {
    std::mt19937 rng(20240);
    const int64_t rows[] = {1, 64, 100, 4096, 0};
    const int worlds[] = {1, 2, 3, 8, 64};
    for (int world : worlds)
        for (int64_t pr : rows)
            for (int rep = 0; rep < 3; ++rep) {
                const int64_t nq = rep == 0 ? 1 : rep == 1 ? 7 : 40;
                const int nb = rep == 0 ? 1 : rep == 1 ? 3 : 8;
                const int empty = rep == 2 && world >= 3 ? 1 : -1;   // a part that is empty
                const std::vector<int32_t> c = random_counts(rng, world, nq, nb, empty, pr == 1 ? 300 : 9000);
                check_plan(world, nq, nb, c, pr);
            }
    {   // a world of one whose part is empty; nq = 0
        std::vector<int32_t> zero(24, 0);
        check_plan(1, 3, 8, zero, 0);
        Plan P;
        EXPECT(make_plan(4, 0, 5, zero.data(), 0, 0, P).problem == OK);
        EXPECT(P.total == 0 && P.lims.size() == 1 && P.lims[0] == 0 && P.piece_n.empty() && P.runs == 0 && P.largest_part == 0);
    }
    {   // runs of exactly piece_rows and piece_rows + 1
        for (int64_t pr : {64ll, 100ll, 4096ll}) {
            std::vector<int32_t> c = {(int32_t)pr, 0, 0, (int32_t)pr + 1};   // world 2, nq 1, nb 2
            Plan P;
            EXPECT(make_plan(2, 1, 2, c.data(), pr, 0, P).problem == OK);
            EXPECT(P.piece_n.size() == 3 && P.piece_n[0] == pr && P.piece_n[1] == pr && P.piece_n[2] == 1);
            EXPECT(P.piece_part[0] == 0 && P.piece_part[1] == 1 && P.piece_part[2] == 1 && P.piece_src[1] == 0 && P.piece_src[2] == pr);
            EXPECT(P.piece_dst[1] == pr && P.piece_dst[2] == 2 * pr);
            check_plan(2, 1, 2, c, pr);
        }
    }
    {   // reported, not planned
        Plan P;
        std::vector<int32_t> c = {3, 0, 5, 0, /* part 1 */ 0, 2, 4, 0, /* part 2 */ 0, 0, 0, 1};   // world 3, nq 2, nb 2
        Verdict v = make_plan(3, 2, 2, c.data(), 0, 0, P);
        EXPECT(v.problem == TWO_OWNERS && v.q == 1 && v.t == 0 && v.part_a == 0 && v.part_b == 1);
        c[6] = 0;
        EXPECT(make_plan(3, 2, 2, c.data(), 0, 0, P).problem == OK && P.total == 11);
        c[9] = -7;
        v = make_plan(3, 2, 2, c.data(), 0, 0, P);
        EXPECT(v.problem == NEGATIVE_COUNT && v.q == 0 && v.t == 1 && v.part_a == 2 && v.value == -7);
        c[9] = 0;
        v = make_plan(3, 2, 2, c.data(), 0, 10, P);
        EXPECT(v.problem == OVER_TOTAL && v.value == 11);
        EXPECT(make_plan(3, 2, 2, c.data(), 0, 11, P).problem == OK);
    }
    {   // counts near the top of int32 sum in 64 bits
        std::vector<int32_t> c = {2147483647, 2147483647, 2147483647};
        Plan P;
        const Verdict v = make_plan(1, 3, 1, c.data(), 1 << 30, 0, P);
        EXPECT(v.problem == OK && P.total == 3ll * 2147483647 && P.piece_n.size() == 6 && P.lims[3] == P.total);
    }
    std::printf("range join plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
