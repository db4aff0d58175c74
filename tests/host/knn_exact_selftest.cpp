// knn_exact_selftest.cpp -- stand-alone check of the pure code of the exact k-NN through the index (csrc/lmi_knn_exact_plan.h: the
// text the kernels run) on the CPU, meant for -fsanitize=address,undefined (tests/test_knn_exact_host.py builds and runs it).
//   - the word: the image is order preserving over negative, zero, subnormal, normal and infinite values, a NaN takes the best image,
//     IP words order by DESCENDING bound, the bucket id survives, value_of inverts image_of;
//   - the seed rule and the split on a small brute force: clustered rows in 9 buckets (an empty one, a one-row one), both metrics;
//     the whole schedule of lmi_search_knn_exact is replayed -- words from the header's bounds, seeds_of, the k-th distance of the
//     seeds' rows as tau, the admission rule (lmi_cover_plan::admit) with radius tau, split_of -- and the k best of (seeds + rest) in
//     the order (distance, bucket, row) must be the k best of all rows; every seed must be admitted; the rank map must name each
//     seed's position in the admitted order; on these separated clusters a small k must prune;
//   - group sizing.
#include "lmi_knn_exact_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <tuple>
#include <vector>

using namespace lmi_knn_exact_plan;
namespace cp = lmi_cover_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

// the scan's distance of row x to query q (cover_selftest.cpp's)
static float scan_dist(int metric, const float* q, const float* x, int d) {
    float s = 0.0f;
    for (int t = 0; t < d; ++t) s = fmaf(q[t], x[t], s);
    if (metric == cp::METRIC_IP) return 1.0f - s;
    float nx = 0.0f, qn2 = 0.0f;
    for (int t = 0; t < d; ++t) nx = fmaf(x[t], x[t], nx);
    for (int t = 0; t < d; ++t) qn2 = fmaf(q[t], q[t], qn2);
    return fmaf(-2.0f, fmaf(1.0f, -0.5f * nx, s), qn2);
}

static long g_visited = 0, g_pairs = 0;

static void run_case(int metric, int d, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<double> gauss(0.0, 1.0);
    const int L = 9;
    const int sizes[L] = {120, 0, 1, 30, 257, 64, 33, 7, 90};
    std::vector<double> cen((size_t)L * d);
    for (double& v : cen) v = 3.0 * gauss(rng);
    std::vector<float> X;
    std::vector<int> lab, row_in;
    for (int b = 0; b < L; ++b)
        for (int i = 0; i < sizes[b]; ++i) {
            std::vector<double> row(d);
            double nn = 0.0;
            for (int t = 0; t < d; ++t) { row[t] = cen[(size_t)b * d + t] + 0.05 * gauss(rng); nn += row[t] * row[t]; }
            const double s = metric == cp::METRIC_IP ? 1.0 / std::sqrt(nn) : 1.0;
            for (int t = 0; t < d; ++t) X.push_back((float)(row[t] * s));
            lab.push_back(b);
            row_in.push_back(i);
        }
    const size_t N = lab.size();
    // the cover: double means, the header's radius chain and round-up
    std::vector<float> c((size_t)L * d, 0.0f), R(L, 0.0f);
    std::vector<double> cn(L, 0.0), sum((size_t)L * d, 0.0), r2(L, 0.0);
    for (size_t i = 0; i < N; ++i)
        for (int t = 0; t < d; ++t) sum[(size_t)lab[i] * d + t] += X[i * d + t];
    for (int b = 0; b < L; ++b)
        for (int t = 0; t < d; ++t) c[(size_t)b * d + t] = sizes[b] ? (float)(sum[(size_t)b * d + t] / sizes[b]) : 0.0f;
    for (size_t i = 0; i < N; ++i) {
        double acc = 0.0;
        for (int t = 0; t < d; ++t) acc = cp::radius_link(acc, X[i * d + t], c[(size_t)lab[i] * d + t]);
        r2[lab[i]] = std::max(r2[lab[i]], acc);
    }
    for (int b = 0; b < L; ++b) { R[b] = cp::radius_of(r2[b]); cn[b] = cp::norm_of(&c[(size_t)b * d], d); }

    for (int qi = 0; qi < 24; ++qi) {
        std::vector<float> q(d);
        const size_t src = rng() % N;
        double nn = 0.0;
        std::vector<double> qd(d);
        for (int t = 0; t < d; ++t) { qd[t] = X[src * d + t] + (qi % 6 == 5 ? 2.0 : 0.01) * gauss(rng); nn += qd[t] * qd[t]; }
        for (int t = 0; t < d; ++t) q[t] = (float)(metric == cp::METRIC_IP ? qd[t] / std::sqrt(nn) : qd[t]);
        const double qn = cp::norm_of(q.data(), d);
        // (distance, bucket, row) of every row: the order of the result
        typedef std::tuple<float, int, int> Entry;
        std::vector<Entry> all;
        for (size_t i = 0; i < N; ++i) all.push_back(Entry(scan_dist(metric, q.data(), &X[i * d], d), lab[i], row_in[i]));
        std::vector<Entry> sorted = all;
        std::sort(sorted.begin(), sorted.end());
        // the bound pass
        std::vector<unsigned long long> words(L, NO_WORD);
        for (int b = 0; b < L; ++b) {
            if (!sizes[b]) continue;
            double chain = 0.0;
            for (int t = 0; t < d; ++t) chain = cp::link(metric, chain, q[t], c[(size_t)b * d + t]);
            const double bound = metric == cp::METRIC_IP ? cp::bound_ip(chain, qn, R[b]) : cp::bound_l2(chain, R[b]);
            words[b] = word_of(metric, bound, (uint32_t)b);
            EXPECT(bucket_of(words[b]) == (uint32_t)b);
        }
        for (int k : {1, 10, 100, 400, 700}) {
            int seeds[MAX_SEEDS];
            const int ns = seeds_of(words.data(), sizes, L, k, seeds);
            EXPECT(ns >= 1 && ns <= 8);
            long long seed_rows = 0;
            for (int i = 0; i < MAX_SEEDS; ++i) {
                EXPECT((i < ns) == (seeds[i] >= 0));
                if (i + 1 < ns) EXPECT(seeds[i] < seeds[i + 1]);
                if (i < ns) seed_rows += sizes[seeds[i]];
            }
            EXPECT(seed_rows >= k || ns == 8);   // the budget: enough rows, or every bucket with rows
            // the rule took the ns smallest words
            std::vector<unsigned long long> w = words;
            std::sort(w.begin(), w.end());
            for (int i = 0; i < ns; ++i) EXPECT(std::find(seeds, seeds + ns, (int)bucket_of(w[i])) != seeds + ns);
            // tau: the k-th distance over the seeds' rows
            std::vector<float> sd;
            for (const Entry& e : all)
                if (std::find(seeds, seeds + ns, std::get<1>(e)) != seeds + ns) sd.push_back(std::get<0>(e));
            std::sort(sd.begin(), sd.end());
            const float tau = (int)sd.size() >= k ? sd[k - 1] : INFINITY;
            // the pruning pass and the split
            std::vector<int> order, admitted;
            for (int b = 0; b < L; ++b)
                if (cp::admit(metric, q.data(), qn, &c[(size_t)b * d], cn[b], R[b], sizes[b], tau, d)) order.push_back(b);
            admitted = order;
            int rank_of[MAX_SEEDS], missed = -1;
            const int visited = split_of(order.data(), (int)order.size(), seeds, rank_of, &missed);
            EXPECT(missed == 0);   // the rule admits every seed
            EXPECT(visited == (int)admitted.size());
            for (int i = 0; i < ns; ++i) EXPECT(admitted[rank_of[i]] == seeds[i] && order[rank_of[i]] == -1);
            EXPECT((int)std::count(order.begin(), order.end(), -1) == ns);
            g_visited += visited;
            g_pairs += 8;
            // the k best of the buckets scored == the k best of all rows
            std::vector<Entry> got;
            for (const Entry& e : all)
                if (std::find(admitted.begin(), admitted.end(), std::get<1>(e)) != admitted.end()) got.push_back(e);
            std::sort(got.begin(), got.end());
            const size_t kk = std::min<size_t>(k, N);
            EXPECT(got.size() >= kk);
            for (size_t j = 0; j < kk; ++j) EXPECT(got[j] == sorted[j]);
        }
    }
}

int main() {
    // the image
    const float inf = INFINITY, tiny = std::numeric_limits<float>::denorm_min();
    const float vals[] = {-inf, -3.0e38f, -1.0f, -tiny, 0.0f, tiny, 1.0e-20f, 1.0f, 3.0e38f, inf};
    for (size_t i = 0; i + 1 < sizeof vals / sizeof *vals; ++i) {
        EXPECT(image_of(vals[i]) < image_of(vals[i + 1]));
        EXPECT(value_of(image_of(vals[i])) == vals[i]);
    }
    EXPECT(image_of(-0.0f) == image_of(0.0f));
    EXPECT(image_of(std::numeric_limits<float>::quiet_NaN()) == 0u && image_of(-std::numeric_limits<float>::quiet_NaN()) == 0u);
    EXPECT(image_of(-inf) > 0u);   // the NaN's image lies before every number's
    EXPECT(word_of(cp::METRIC_L2, 0.5, 7) < word_of(cp::METRIC_L2, 0.75, 3) && word_of(cp::METRIC_IP, 0.75, 7) < word_of(cp::METRIC_IP, 0.5, 3));
    EXPECT(word_of(cp::METRIC_L2, 0.5, 3) < word_of(cp::METRIC_L2, 0.5, 7) && word_of(cp::METRIC_L2, 1.0e300, 65534) < NO_WORD);
    EXPECT(bucket_of(word_of(cp::METRIC_IP, -2.0, 65534)) == 65534u && bound_of(cp::METRIC_IP, word_of(cp::METRIC_IP, 0.25, 1)) == 0.25f);
    EXPECT(bound_of(cp::METRIC_L2, word_of(cp::METRIC_L2, 1.5, 1)) == 1.5f);
    EXPECT(word_of(cp::METRIC_IP, std::numeric_limits<double>::quiet_NaN(), 9) == 9ull);
    // the budget
    EXPECT(!seeds_done(9, 10, 1) && seeds_done(10, 10, 1) && seeds_done(0, 10, MAX_SEEDS) && !seeds_done(0, 10, MAX_SEEDS - 1));
    {   // 40 one-row buckets and k = 1024: the cap; no words at all: no seed
        std::vector<unsigned long long> w;
        std::vector<int> n(40, 1);
        for (int b = 0; b < 40; ++b) w.push_back(word_of(cp::METRIC_L2, 40.0 - b, (uint32_t)b));
        int seeds[MAX_SEEDS];
        EXPECT(seeds_of(w.data(), n.data(), 40, 1024, seeds) == MAX_SEEDS && seeds[0] == 8 && seeds[MAX_SEEDS - 1] == 39);
        EXPECT(seeds_of(w.data(), n.data(), 40, 3, seeds) == 3 && seeds[0] == 37 && seeds[2] == 39 && seeds[3] == -1);
        std::fill(w.begin(), w.end(), NO_WORD);
        EXPECT(seeds_of(w.data(), n.data(), 40, 3, seeds) == 0 && seeds[0] == -1);
    }
    {   // the search, and a seed the order does not hold
        const int order[] = {2, 5, 9, 30};
        EXPECT(lower_bound(order, 4, 0) == 0 && lower_bound(order, 4, 5) == 1 && lower_bound(order, 4, 6) == 2 && lower_bound(order, 4, 31) == 4);
        EXPECT(lower_bound(order, 0, 3) == 0);
        int ord[] = {2, 5, 9, 30}, seeds[MAX_SEEDS], rank_of[MAX_SEEDS], missed = 0;
        std::fill(seeds, seeds + MAX_SEEDS, -1);
        seeds[0] = 5, seeds[1] = 7, seeds[2] = 30;
        EXPECT(split_of(ord, 4, seeds, rank_of, &missed) == 5 && missed == 1);
        EXPECT(ord[0] == 2 && ord[1] == -1 && ord[2] == 9 && ord[3] == -1 && rank_of[0] == 1 && rank_of[1] == 2 && rank_of[2] == 3);
    }
    // groups
    EXPECT(query_rows_for(0, 100, 12) == 100 && query_rows_for(7, 100, 12) == 7 && query_rows_for(7, 3, 12) == 3);
    EXPECT(word_bytes(query_rows_for(0, 1 << 20, 65535), 65535) <= WORD_BYTES && query_rows_for(0, 1 << 20, 65535) >= 1);
    EXPECT(query_rows_for(0, 1 << 20, 12) == cp::DEFAULT_QUERY_ROWS && word_bytes(3, 5) == 120);
    unsigned seed = 11;
    for (int metric : {cp::METRIC_IP, cp::METRIC_L2})
        for (int d : {1, 24, 33}) run_case(metric, d, seed++);
    EXPECT(g_visited * 4 < g_pairs * 3);   // it prunes: it does not pass by visiting everything
    std::printf("knn exact plan selftest: clean (%ld checks, %ld buckets visited of %ld)\n", g_checks, g_visited, g_pairs);
    return 0;
}
