// Stand-alone self-test of csrc/lmi_regroup_plan.h (pure host code): the argument checks, the sorted list, the ordinal bases, the sort's
// shape, and a replay of the whole partition on the CPU -- words made as regroup_label_kernel makes them, tiles sorted, runs merged with
// lmi_range_sort_plan.h's merge_piece / merge_split (what range_sort_merge_kernel runs) -- against the order rule's plain statement,
// for every tile length.  Built with -fsanitize=address,undefined by tests/test_regroup_host.py; prints "regroup plan selftest: clean".
#include <cstdio>
#include <cstdlib>
#include <random>

#include "lmi_range_sort_plan.h"
#include "lmi_regroup_plan.h"

namespace rp = lmi_regroup_plan;
namespace sp = lmi_range_sort_plan;

static int failures = 0;
#define EXPECT(c)                                                    \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void checks() {
    rp::List out;
    const uint32_t ids[5] = {9, 4, 4000000000u, 1, 7};
    const int64_t lab[5] = {0, 3, 2, 1, 3};
    const int32_t map[3] = {2, -1, 0};
    EXPECT(rp::check(3, 4, ids, lab, 5, map, out).problem == rp::OK);
    EXPECT(out.ids.size() == 5 && out.ids[0] == 1 && out.ids[1] == 4 && out.ids[2] == 7 && out.ids[3] == 9 && out.ids[4] == 4000000000u);
    EXPECT(out.labels[0] == 1 && out.labels[1] == 3 && out.labels[2] == 3 && out.labels[3] == 0 && out.labels[4] == 2);
    EXPECT(rp::check(3, 4, nullptr, nullptr, 0, nullptr, out).problem == rp::OK && out.ids.empty());
    EXPECT(rp::check(3, 0, ids, lab, 5, map, out).problem == rp::BAD_L_NEW);
    EXPECT(rp::check(3, rp::MAX_LABELS, ids, lab, 5, map, out).problem == rp::BAD_L_NEW);
    EXPECT(rp::check(3, rp::MAX_LABELS - 1, nullptr, nullptr, 0, nullptr, out).problem == rp::OK);
    EXPECT(rp::check(3, 4, ids, lab, -1, map, out).problem == rp::BAD_N);
    EXPECT(rp::check(3, 4, nullptr, lab, 5, map, out).problem == rp::NULL_LIST);
    EXPECT(rp::check(3, 4, ids, nullptr, 5, map, out).problem == rp::NULL_LIST);
    rp::Verdict v = rp::check(3, 3, ids, lab, 5, map, out);
    EXPECT(v.problem == rp::BAD_LABEL && v.at == 1 && v.value == 3);
    const int64_t neg[5] = {0, 1, -1, 1, 1};
    v = rp::check(3, 4, ids, neg, 5, map, out);
    EXPECT(v.problem == rp::BAD_LABEL && v.at == 2 && v.value == -1);
    const int32_t bad_map[3] = {2, -2, 0}, big_map[3] = {2, 1, 4};
    v = rp::check(3, 4, ids, lab, 5, bad_map, out);
    EXPECT(v.problem == rp::BAD_MAP && v.at == 1 && v.value == -2);
    v = rp::check(3, 4, ids, lab, 5, big_map, out);
    EXPECT(v.problem == rp::BAD_MAP && v.at == 2 && v.value == 4);
    EXPECT(rp::check(5, 4, ids, lab, 5, nullptr, out).problem == rp::NULL_MAP_SHRINKS);
    const uint32_t dup[4] = {8, 3, 8, 1};
    v = rp::check(3, 4, dup, lab, 4, map, out);
    EXPECT(v.problem == rp::DUPLICATE_ID && v.value == 8);
    const std::vector<int> id_map = rp::map_of(3, nullptr), given = rp::map_of(3, map);
    EXPECT(id_map[0] == 0 && id_map[2] == 2 && given[0] == 2 && given[1] == -1 && given[2] == 0);
    const std::vector<int64_t> base = rp::ordinal_bases({0, 5, 0, 33, 1});
    EXPECT(base.size() == 6 && base[0] == 0 && base[1] == 0 && base[2] == 5 && base[3] == 5 && base[4] == 38 && base[5] == 39);
    EXPECT(rp::first_unmapped({0, 0, 4, 1}) == 2 && rp::first_unmapped({0, 0}) == -1 && rp::first_unmapped({}) == -1);
    EXPECT(rp::tile_rows_ok(0) && rp::tile_rows_ok(64) && rp::tile_rows_ok(8192) && !rp::tile_rows_ok(32) && !rp::tile_rows_ok(16384) &&
           !rp::tile_rows_ok(96) && !rp::tile_rows_ok(-64));
    rp::SortPlan P = rp::sort_plan(0, 0);
    EXPECT(P.tiles == 0 && P.passes == 0 && P.merge_pieces == 0);
    P = rp::sort_plan(8192, 0);
    EXPECT(P.tile_rows == 8192 && P.tiles == 1 && P.passes == 0 && P.merge_rows == 2048);
    P = rp::sort_plan(8193, 0);
    EXPECT(P.tiles == 2 && P.passes == 1 && P.merge_pieces == 5);
    P = rp::sort_plan(20000, 64);
    EXPECT(P.tile_rows == 64 && P.merge_rows == 64 && P.tiles == 313 && P.passes == 9 && P.merge_pieces == 313);
    EXPECT(P.map_bytes(1000, 50) == 20 * 20000 + 4000 + 400);
    EXPECT(rp::sort_plan(6000, 0).map_bytes(6400, 0) == 12 * 6000 + 4 * 6400);
}

// the device's sort on the CPU: tiles sorted, then merge passes piece by piece
static std::vector<uint64_t> replay_sort(std::vector<uint64_t> w, int64_t forced_T) {
    const int64_t n = (int64_t)w.size();
    const rp::SortPlan P = rp::sort_plan(n, forced_T);
    for (int64_t t = 0; t < P.tiles; ++t)
        std::sort(w.begin() + t * P.tile_rows, w.begin() + std::min(n, (t + 1) * P.tile_rows));
    std::vector<uint64_t> other(w.size());
    int passes = 0;
    for (int64_t run = P.tile_rows; run < n; run <<= 1, ++passes) {
        for (int64_t b = 0; b < P.merge_pieces; ++b) {
            const sp::Piece X = sp::merge_piece(n, run, P.merge_rows, b);
            const uint64_t* A = w.data() + X.p0;
            const uint64_t* B = A + X.la;
            const int64_t i0 = sp::merge_split(A, X.la, B, X.lb, X.o0 - X.p0), i1 = sp::merge_split(A, X.la, B, X.lb, X.o1 - X.p0);
            const int64_t j0 = X.o0 - X.p0 - i0, j1 = X.o1 - X.p0 - i1;
            EXPECT(i1 - i0 + j1 - j0 == X.o1 - X.o0 && X.o1 - X.o0 <= P.merge_rows);
            std::merge(A + i0, A + i1, B + j0, B + j1, other.begin() + X.o0);
        }
        w.swap(other);
    }
    EXPECT(passes == P.passes);
    return w;
}

static void partition(std::mt19937& rng, int L, int L_new, int max_rows) {
    std::vector<int> nb((size_t)L);
    for (int& v : nb) v = (int)(rng() % (unsigned)(max_rows + 1)) * (int)(rng() % 3 != 0);
    const std::vector<int64_t> base = rp::ordinal_bases(nb);
    const int64_t n = base[(size_t)L];
    std::vector<int> lab((size_t)n);
    for (int& v : lab) v = (int)(rng() % (unsigned)L_new);
    std::vector<uint64_t> words((size_t)n);
    for (int64_t o = 0; o < n; ++o) words[(size_t)o] = ((uint64_t)(unsigned)lab[(size_t)o] << 32) | (uint64_t)o;
    const std::vector<int64_t> want = rp::new_order(lab);
    for (int64_t T : {(int64_t)0, (int64_t)64, (int64_t)256, (int64_t)4096}) {
        const std::vector<uint64_t> got = replay_sort(words, T);
        bool same = got.size() == want.size();
        for (size_t i = 0; same && i < got.size(); ++i) same = (int64_t)(uint32_t)got[i] == want[i] && (int)(got[i] >> 32) == lab[(size_t)want[i]];
        EXPECT(same);
    }
}

int main() {
    checks();
    std::mt19937 rng(2024);
    partition(rng, 1, 1, 0);
    partition(rng, 1, 3, 1);
    partition(rng, 12, 17, 700);
    partition(rng, 12, 5, 3000);
    partition(rng, 40, 1000, 600);
    partition(rng, 3, 2, 9000);
    if (failures) {
        std::printf("regroup plan selftest: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("regroup plan selftest: clean\n");
    return 0;
}
