// fetch_plan_selftest.cpp -- stand-alone check of the host arithmetic of lmi_rows_fetch (csrc/lmi_fetch_plan.h: pure host code) on the
// CPU, meant for -fsanitize=address,undefined (tests/test_fetch_host.py builds and runs it).
//   - n = 0, n = 1, all requests equal, all distinct, the ids 0 and 2^32 - 1;
//   - the unique list ascends strictly and holds exactly the requested ids; unique[map[i]] == ids[i] for 200 random lists;
//   - the pieces tile [0, n) in order, each of piece_rows requests but the last: piece_rows = 1, piece_rows > n, the default;
//   - what the hook and the request count accept and refuse; the default piece fits the stage;
//   - the location word: (bucket, row) order is the order of the words, all ones is absent;
//   - the locate pass replayed on the host on an index with repeated ids: the minimum over the rows is the first (bucket, row) in
//     whatever order the rows are visited.
#include "lmi_fetch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <set>

using namespace lmi_fetch_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void check_plan(const std::vector<uint32_t>& ids, int64_t piece_rows) {
    const int64_t n = (int64_t)ids.size();
    const Plan P = make_plan(ids.data(), n, piece_rows);
    EXPECT(P.n == n && P.piece_rows == piece_rows && (int64_t)P.map.size() == n);
    const std::set<uint32_t> want(ids.begin(), ids.end());
    EXPECT(P.unique.size() == want.size());
    EXPECT(std::equal(P.unique.begin(), P.unique.end(), want.begin()));   // (a set iterates ascending: strictly ascending and complete)
    for (int64_t i = 0; i < n; ++i) {
        EXPECT(P.map[(size_t)i] >= 0 && (size_t)P.map[(size_t)i] < P.unique.size());
        EXPECT(P.unique[(size_t)P.map[(size_t)i]] == ids[(size_t)i]);
    }
    EXPECT(P.pieces() == (n == 0 ? 0 : cdiv(n, piece_rows)));
    int64_t at = 0;
    for (int64_t p = 0; p < P.pieces(); ++p) {
        EXPECT(P.piece_begin(p) == at && P.piece_end(p) > at && P.piece_end(p) <= n);
        EXPECT(P.piece_end(p) - at == piece_rows || (p == P.pieces() - 1 && P.piece_end(p) - at <= piece_rows));
        at = P.piece_end(p);
    }
    EXPECT(at == n);
    EXPECT(P.table_bytes() <= TABLE_BYTES_PER_REQUEST * n && P.table_bytes() == (int64_t)P.unique.size() * 12 + 4 * n);
}

// fetch_locate_kernel on the host: rows visited in the given order, each lowering its id's word
static std::vector<uint64_t> locate(const Plan& P, const std::vector<std::vector<uint32_t>>& buckets, const std::vector<std::pair<int, int>>& order) {
    std::vector<uint64_t> loc(P.unique.size(), ABSENT);
    for (const auto& br : order) {
        const uint32_t id = buckets[(size_t)br.first][(size_t)br.second];
        const auto it = std::lower_bound(P.unique.begin(), P.unique.end(), id);
        if (it != P.unique.end() && *it == id) {
            uint64_t& w = loc[(size_t)(it - P.unique.begin())];
            w = std::min(w, loc_word(br.first, br.second));
        }
    }
    return loc;
}

int main() {
    std::mt19937 rng(20261021);
    EXPECT(n_ok(0) && n_ok(1) && n_ok(MAX_REQUESTS) && !n_ok(MAX_REQUESTS + 1) && !n_ok(-1) && MAX_REQUESTS + 1 == (1ll << 31));
    EXPECT(piece_rows_ok(0) && piece_rows_ok(1) && piece_rows_ok(MAX_PIECE_ROWS) && !piece_rows_ok(MAX_PIECE_ROWS + 1) && !piece_rows_ok(-1));
    EXPECT(request_bytes(768, 4, true) == 768 * 4 + 8 && request_bytes(768, 2, true) == 768 * 2 + 8 && request_bytes(768, 4, false) == 8);
    EXPECT(piece_rows_for(7, 3080) == 7 && piece_rows_for(MAX_PIECE_ROWS, 8) == MAX_PIECE_ROWS);
    EXPECT(piece_rows_for(0, 3080) == STAGE_BYTES / 3080 && piece_rows_for(0, 3080) * 3080 <= STAGE_BYTES);
    EXPECT(piece_rows_for(0, 3080, false) == MAX_PIECE_ROWS && piece_rows_for(7, 3080, false) == 7);   // device outputs: no stage to fit
    EXPECT(piece_rows_for(0, 8) == STAGE_BYTES / 8 && piece_rows_for(0, 1) == MAX_PIECE_ROWS && piece_rows_for(0, 2 * STAGE_BYTES) == 1);

    for (int64_t pr : {(int64_t)1, (int64_t)7, (int64_t)1000}) {
        check_plan({}, pr);                                        // n = 0
        check_plan({42u}, pr);                                     // n = 1
        check_plan(std::vector<uint32_t>(37, 5u), pr);             // all equal
        std::vector<uint32_t> distinct(129);
        std::iota(distinct.begin(), distinct.end(), 1000u);
        std::shuffle(distinct.begin(), distinct.end(), rng);
        check_plan(distinct, pr);                                  // all distinct
        check_plan({0xffffffffu, 0u, 7u, 0u, 0xffffffffu}, pr);    // the ends of the id range
    }
    {
        const Plan P = make_plan(nullptr, 0, 5);
        EXPECT(P.unique.empty() && P.map.empty() && P.pieces() == 0 && P.table_bytes() == 0);
        const uint32_t ends[] = {0xffffffffu, 0u};
        const Plan E = make_plan(ends, 2, 1);
        EXPECT(E.unique.size() == 2 && E.unique[0] == 0u && E.unique[1] == 0xffffffffu && E.map[0] == 1 && E.map[1] == 0 && E.pieces() == 2);
        const uint32_t same[] = {9u, 9u, 9u};
        const Plan S = make_plan(same, 3, 10);   // piece_rows > n
        EXPECT(S.unique.size() == 1 && S.map[0] == 0 && S.map[2] == 0 && S.pieces() == 1 && S.piece_end(0) == 3);
    }
    for (int rep = 0; rep < 200; ++rep) {   // random lists: few values (heavy repeats), many values, the whole range
        const int64_t n = 1 + (int64_t)(rng() % 400);
        const uint32_t span = rep % 3 == 0 ? 8u : rep % 3 == 1 ? 100000u : 0xffffffffu;
        std::vector<uint32_t> ids((size_t)n);
        for (uint32_t& v : ids) v = span == 0xffffffffu ? (uint32_t)rng() : (uint32_t)(rng() % span);
        const int64_t prs[] = {1, n - 1 > 0 ? n - 1 : 1, n, n + 1, 1 + (int64_t)(rng() % 50)};
        check_plan(ids, prs[rep % 5]);
    }

    // the location word orders like (bucket, row); absent is above every location
    EXPECT(loc_word(0, 5) < loc_word(1, 0) && loc_word(2, 3) < loc_word(2, 4) && loc_word(0x7fffffff, 0x7fffffff) < ABSENT);
    EXPECT(loc_bucket(loc_word(5, 9)) == 5 && loc_row(loc_word(5, 9)) == 9 && loc_bucket(ABSENT) == -1 && loc_row(ABSENT) == -1);
    {   // id 77 in bucket 5 (row 0) and twice in bucket 2 (rows 4 and 1); id 3 nowhere
        std::vector<std::vector<uint32_t>> buckets(6);
        buckets[2] = {10u, 77u, 11u, 12u, 77u};
        buckets[5] = {77u, 13u};
        buckets[0] = {14u};
        const uint32_t req[] = {77u, 3u, 13u, 77u};
        const Plan P = make_plan(req, 4, 2);
        std::vector<std::pair<int, int>> order;
        for (int b = 0; b < 6; ++b)
            for (int r = 0; r < (int)buckets[(size_t)b].size(); ++r) order.push_back({b, r});
        for (int rep = 0; rep < 50; ++rep) {
            std::shuffle(order.begin(), order.end(), rng);
            const std::vector<uint64_t> loc = locate(P, buckets, order);
            const uint64_t w77 = loc[(size_t)P.map[0]];
            EXPECT(loc_bucket(w77) == 2 && loc_row(w77) == 1 && loc[(size_t)P.map[3]] == w77);
            EXPECT(loc[(size_t)P.map[1]] == ABSENT);
            EXPECT(loc_bucket(loc[(size_t)P.map[2]]) == 5 && loc_row(loc[(size_t)P.map[2]]) == 1);
        }
    }
    std::printf("fetch plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
