// Stand-alone self-test of csrc/lmi_concat_plan.h (pure host code): the compatibility verdicts, the result's counts and the first row
// of every (part, bucket) against a naive restatement of the order rule on random and forced counts, a replay of the source map the
// way concat_srcmap_kernel fills it (parts with slack and relocated buckets), and the limit refusals no GPU test can reach cheaply.
// Built with -fsanitize=address,undefined by tests/test_concat_host.py; prints "concat plan selftest: clean".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>

#include "lmi_concat_plan.h"

namespace cp = lmi_concat_plan;

static int failures = 0;
#define EXPECT(c)                                                    \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                              \
        }                                                            \
    } while (0)

static cp::Shape shape(int device, int d, int L, int metric, int storage, bool prefilter, std::vector<unsigned char> owned = {}) {
    cp::Shape s;
    s.device = device; s.d = d; s.L = L; s.metric = metric; s.storage = storage; s.prefilter = prefilter; s.owned = std::move(owned);
    return s;
}

static void verdicts() {
    const cp::Shape a = shape(0, 45, 4, 0, 0, true);
    EXPECT(cp::compatible({a}).problem == cp::OK);
    EXPECT(cp::compatible({a, a, a}).problem == cp::OK);
    EXPECT(cp::compatible({}).problem == cp::BAD_N_PARTS);
    EXPECT(cp::compatible(std::vector<cp::Shape>(cp::MAX_PARTS, a)).problem == cp::OK);
    cp::Verdict v = cp::compatible(std::vector<cp::Shape>(cp::MAX_PARTS + 1, a));
    EXPECT(v.problem == cp::BAD_N_PARTS && v.value == cp::MAX_PARTS + 1);
    EXPECT(cp::n_parts_ok(1) && cp::n_parts_ok(64) && !cp::n_parts_ok(0) && !cp::n_parts_ok(65) && !cp::n_parts_ok(-1));
    v = cp::compatible({a, a, shape(1, 45, 4, 0, 0, true)});
    EXPECT(v.problem == cp::DEVICE && v.part == 2 && v.value == 1 && v.want == 0);
    v = cp::compatible({a, shape(0, 46, 4, 0, 0, true)});
    EXPECT(v.problem == cp::DIMS && v.part == 1 && v.value == 46 && v.want == 45);
    v = cp::compatible({a, shape(0, 45, 5, 0, 0, true)});
    EXPECT(v.problem == cp::BUCKETS && v.part == 1 && v.value == 5 && v.want == 4);
    v = cp::compatible({a, shape(0, 45, 4, 1, 0, true)});
    EXPECT(v.problem == cp::METRIC && v.value == 1 && v.want == 0);
    v = cp::compatible({a, shape(0, 45, 4, 0, 1, true)});
    EXPECT(v.problem == cp::STORAGE && v.value == 1 && v.want == 0);
    v = cp::compatible({a, shape(0, 45, 4, 0, 0, false)});
    EXPECT(v.problem == cp::PREFILTER && v.value == 0 && v.want == 1);
    v = cp::compatible({a, shape(0, 45, 4, 0, 0, true, {1, 0, 1, 0})});
    EXPECT(v.problem == cp::OWNED && v.part == 1 && v.value == 1 && v.want == 0);
    const cp::Shape o = shape(0, 45, 4, 0, 0, true, {1, 0, 1, 0});
    EXPECT(cp::compatible({o, shape(0, 45, 4, 0, 0, true, {1, 0, 7, 0})}).problem == cp::OK);   // (a mask is zero / non-zero)
    v = cp::compatible({o, a});
    EXPECT(v.problem == cp::OWNED && v.value == 0 && v.want == 1);
    v = cp::compatible({o, o, shape(0, 45, 4, 0, 0, true, {1, 0, 1, 1})});
    EXPECT(v.problem == cp::OWNED && v.part == 2 && v.at == 3 && v.value == 1 && v.want == 1);
    // the first difference in part order, and within a part in the order of the enum
    v = cp::compatible({a, shape(0, 45, 4, 1, 1, true), shape(0, 46, 4, 0, 0, true)});
    EXPECT(v.problem == cp::METRIC && v.part == 1);
}

// the order rule, stated plainly: the object list "part 0's objects (bucket ascending, then row), then part 1's, ...", built stably
// by bucket; per bucket the (part, row) of its j-th object
static std::vector<std::vector<std::pair<int, int>>> naive(const std::vector<std::vector<int>>& rows, int L) {
    std::vector<std::tuple<int, int, int>> list;   // (bucket, part, row)
    for (size_t t = 0; t < rows.size(); ++t)
        for (int b = 0; b < L; ++b)
            for (int j = 0; j < rows[t][(size_t)b]; ++j) list.emplace_back(b, (int)t, j);
    std::stable_sort(list.begin(), list.end(), [](const auto& x, const auto& y) { return std::get<0>(x) < std::get<0>(y); });
    std::vector<std::vector<std::pair<int, int>>> out((size_t)L);
    for (const auto& e : list) out[(size_t)std::get<0>(e)].emplace_back(std::get<1>(e), std::get<2>(e));
    return out;
}

static void against_naive(std::mt19937& rng, const std::vector<std::vector<int>>& rows, int L) {
    const int n_parts = (int)rows.size();
    std::vector<std::vector<unsigned char>> any((size_t)n_parts, std::vector<unsigned char>((size_t)L, 0));
    std::vector<int64_t> N((size_t)n_parts, 0);
    std::vector<unsigned char> any_want((size_t)L, 0);
    int64_t total = 0, N_want = 0;
    for (int t = 0; t < n_parts; ++t) {
        for (int b = 0; b < L; ++b) {
            any[(size_t)t][(size_t)b] = rows[(size_t)t][(size_t)b] > 0 || rng() % 5 == 0;   // (a bucket with rows on another rank only)
            any_want[(size_t)b] |= any[(size_t)t][(size_t)b];
            N[(size_t)t] += rows[(size_t)t][(size_t)b];
        }
        N[(size_t)t] += (int64_t)(rng() % 100);   // (objects of other ranks)
        N_want += N[(size_t)t];
    }
    const cp::Plan P = cp::plan(rows, any, N);
    EXPECT(P.verdict.problem == cp::OK && P.n_parts == n_parts && P.L == L && P.N == N_want && P.any == any_want);
    const auto want = naive(rows, L);
    // the layout is lmi_layout::fresh_layout of the counts
    std::vector<int> rb_start, cap_rb;
    int64_t rb = 0;
    for (int b = 0; b < L; ++b) {
        EXPECT(P.counts[(size_t)b] == (int)want[(size_t)b].size());
        EXPECT(P.rb_start[(size_t)b] == rb && P.cap_rb[(size_t)b] == (P.counts[(size_t)b] + 31) / 32);
        rb += P.cap_rb[(size_t)b];
        total += P.counts[(size_t)b];
    }
    EXPECT(P.rb_start[(size_t)L] == rb && P.n_rb_total == rb && P.rows == total && P.map_bytes() == 8 * 32 * rb);
    // the parts as a mutated index may hold them: buckets in any order of the slab, spare row-blocks between them
    std::vector<std::vector<int>> first((size_t)n_parts, std::vector<int>((size_t)L, 0));
    for (int t = 0; t < n_parts; ++t) {
        std::vector<int> order((size_t)L);
        for (int b = 0; b < L; ++b) order[(size_t)b] = b;
        std::shuffle(order.begin(), order.end(), rng);
        int at = 0;
        for (int b : order) {
            at += (int)(rng() % 3);
            first[(size_t)t][(size_t)b] = at * 32;
            at += (rows[(size_t)t][(size_t)b] + 31) / 32;
        }
    }
    // the source map as concat_srcmap_kernel fills it: written once everywhere, the naive list's (part, row) at every object's place
    std::vector<std::pair<int, int>> map((size_t)(P.n_rb_total * 32), {-7, -7});
    for (int b = 0; b < L; ++b) {
        const int64_t nb = (int64_t)P.rb_start[(size_t)b] * 32;
        const int cap = (P.rb_start[(size_t)b + 1] - P.rb_start[(size_t)b]) * 32;
        for (int t = 0; t < n_parts; ++t)
            for (int j = 0; j < rows[(size_t)t][(size_t)b]; ++j) {
                std::pair<int, int>& e = map[(size_t)(nb + P.offset(t, b) + j)];
                EXPECT(e.first == -7);
                e = {t, first[(size_t)t][(size_t)b] + j};
            }
        for (int j = P.counts[(size_t)b]; j < cap; ++j) {
            EXPECT(map[(size_t)(nb + j)].first == -7);
            map[(size_t)(nb + j)] = {-1, -1};
        }
        bool same = true;
        for (int j = 0; same && j < P.counts[(size_t)b]; ++j) {
            const auto& w = want[(size_t)b][(size_t)j];
            same = map[(size_t)(nb + j)] == std::make_pair(w.first, first[(size_t)w.first][(size_t)b] + w.second);
        }
        EXPECT(same);
    }
    for (const auto& e : map) EXPECT(e.first != -7);
}

static void random_counts(std::mt19937& rng, int n_parts, int L, int max_rows) {
    std::vector<std::vector<int>> rows((size_t)n_parts, std::vector<int>((size_t)L));
    for (auto& r : rows)
        for (int& v : r) v = (int)(rng() % (unsigned)(max_rows + 1)) * (int)(rng() % 3 != 0);
    against_naive(rng, rows, L);
}

static void limits() {
    const int L = 4;
    const int64_t max_rb = lmi_layout::max_slab_rb(L);
    const std::vector<std::vector<unsigned char>> any2(2, std::vector<unsigned char>((size_t)L, 1));
    // a bucket that passes the last row-block only as the sum of two parts (N counted small: a rank's N is the caller's word)
    const int half = (int)(max_rb * 32 / 2);
    cp::Plan P = cp::plan({{0, half, 0, 0}, {0, half, 0, 0}}, any2, {10, 10});
    EXPECT(P.verdict.problem == cp::OK && P.counts[1] == 2 * half && P.offset(1, 1) == half);
    P = cp::plan({{0, half, 0, 0}, {0, half + 33, 0, 0}}, any2, {10, 10});
    EXPECT(P.verdict.problem == cp::BUCKET_PAST_LIMIT && P.verdict.at == 1 && P.verdict.value == 2ll * half + 33);
    // every bucket fits, the layout does not
    const int third = (int)(max_rb * 32 / 3);
    P = cp::plan({{third, third, 0, 0}, {0, 0, third, 64}}, any2, {10, 10});
    EXPECT(P.verdict.problem == cp::TOTAL_PAST_LIMIT && P.verdict.value > max_rb);
    P = cp::plan({{third, third, 0, 0}, {0, 0, third - 64, 0}}, any2, {10, 10});
    EXPECT(P.verdict.problem == cp::OK && P.n_rb_total <= max_rb);
    // sums past 2^31 do not wrap: 64 parts of 2^30 rows in one bucket
    P = cp::plan(std::vector<std::vector<int>>(64, {1 << 30, 0, 0, 0}), std::vector<std::vector<unsigned char>>(64, {1, 0, 0, 0}),
                 std::vector<int64_t>(64, 10));
    EXPECT(P.verdict.problem == cp::BUCKET_PAST_LIMIT && P.verdict.at == 0 && P.verdict.value == 64ll << 30);
    // N is lmi_buckets_begin's limit on the sum
    P = cp::plan({{1, 0, 0, 0}, {1, 0, 0, 0}}, any2, {1ll << 30, (1ll << 30) - 64 * L});
    EXPECT(P.verdict.problem == cp::N_PAST_LIMIT && P.verdict.value == (1ll << 31) - 64 * L);
    P = cp::plan({{1, 0, 0, 0}, {1, 0, 0, 0}}, any2, {1ll << 30, (1ll << 30) - 64 * L - 1});
    EXPECT(P.verdict.problem == cp::OK && P.N == (1ll << 31) - 64 * L - 1);
}

int main() {
    verdicts();
    std::mt19937 rng(2025);
    // the seams: empty in one or both parts; a second part starting at the last row of a row-block, at a boundary, one past it
    against_naive(rng, {{0, 0, 1, 31, 32, 33, 1, 2500}, {0, 1, 0, 1, 1, 32, 2500, 33}}, 8);
    against_naive(rng, {{5}}, 1);
    against_naive(rng, {{0}}, 1);
    against_naive(rng, {{0, 0}, {0, 0}, {0, 0}}, 2);
    against_naive(rng, {{7, 40}, {7, 40}}, 2);   // (a part listed twice has the same counts twice)
    random_counts(rng, 1, 12, 700);
    random_counts(rng, 2, 12, 3000);
    random_counts(rng, 5, 12, 300);
    random_counts(rng, 64, 3, 70);
    random_counts(rng, 7, 40, 100);
    limits();
    if (failures) {
        std::printf("concat plan selftest: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("concat plan selftest: clean\n");
    return 0;
}
