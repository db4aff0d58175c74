// cover_selftest.cpp -- stand-alone check of the admission rule of the exact range search (csrc/lmi_cover_plan.h: pure code, the text
// the kernel runs) on the CPU, meant for -fsanitize=address,undefined (tests/test_cover_host.py builds and runs it).
//   - clustered rows in 7 buckets (an empty one, a one-row one, one of equal rows), both metrics, d = 1, 24, 33 and 70; a cover made
//     with the header's own radius chain and round-up about the mean of each bucket;
//   - every row is scored as the scan scores it: binary32 fmaf chains in ascending order, IP dist = 1.0f - s, L2 the stored
//     -|x|^2/2 inside the chain and dist = fmaf(-2, key, |q|^2);
//   - radii sit EXACTLY on computed distances (the nearest, the 5th, the 40th and the farthest row of a query, and one step below
//     the nearest): whenever a row of a bucket is admitted by the scan's comparison, the rule must admit the bucket -- no needed
//     pair may be missed; on these well-separated clusters the rule must also prune (it is not allowed to admit everything);
//   - NaN, +inf and -inf radii, a NaN query, an empty bucket, R = +inf, the round-up of radius_of, the geometry helpers.
#include "lmi_cover_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

using namespace lmi_cover_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

struct Cover {
    int L = 0, d = 0;
    std::vector<int64_t> n;
    std::vector<float> c, R;
    std::vector<double> cn;
};

// the scan's distance of row x to query q
static float scan_dist(int metric, const float* q, const float* x, int d) {
    float s = 0.0f;
    for (int t = 0; t < d; ++t) s = fmaf(q[t], x[t], s);
    if (metric == METRIC_IP) return 1.0f - s;
    float nx = 0.0f, qn2 = 0.0f;
    for (int t = 0; t < d; ++t) nx = fmaf(x[t], x[t], nx);
    for (int t = 0; t < d; ++t) qn2 = fmaf(q[t], q[t], qn2);
    const float key = fmaf(1.0f, -0.5f * nx, s);   // link d of the chain: the query's 1 meets the stored -|x|^2/2
    return fmaf(-2.0f, key, qn2);
}

static Cover make_cover(const std::vector<float>& X, const std::vector<int>& lab, int L, int d) {
    Cover C;
    C.L = L, C.d = d;
    C.n.assign(L, 0);
    C.c.assign((size_t)L * d, 0.0f);
    C.R.assign(L, 0.0f);
    C.cn.assign(L, 0.0);
    std::vector<double> sum((size_t)L * d, 0.0), r2(L, 0.0);
    const size_t N = lab.size();
    for (size_t i = 0; i < N; ++i) {
        ++C.n[lab[i]];
        for (int t = 0; t < d; ++t) sum[(size_t)lab[i] * d + t] += X[i * d + t];
    }
    for (int b = 0; b < L; ++b)
        for (int t = 0; t < d; ++t) C.c[(size_t)b * d + t] = C.n[b] ? (float)(sum[(size_t)b * d + t] / (double)C.n[b]) : 0.0f;
    for (size_t i = 0; i < N; ++i) {
        double acc = 0.0;
        for (int t = 0; t < d; ++t) acc = radius_link(acc, X[i * d + t], C.c[(size_t)lab[i] * d + t]);
        if (acc > r2[lab[i]]) r2[lab[i]] = acc;
    }
    for (int b = 0; b < L; ++b) {
        C.R[b] = radius_of(r2[b]);
        C.cn[b] = norm_of(&C.c[(size_t)b * d], d);
        EXPECT((double)C.R[b] * (double)C.R[b] >= r2[b]);   // rounded UP: the ball holds every row
    }
    return C;
}

static long g_needed = 0, g_pairs = 0, g_admitted = 0;

static void run_case(int metric, int d, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<double> gauss(0.0, 1.0);
    const int L = 7;
    const int sizes[L] = {120, 0, 1, 30, 257, 64, 33};
    std::vector<double> cen((size_t)L * d);
    for (double& v : cen) v = 3.0 * gauss(rng);
    std::vector<float> X;
    std::vector<int> lab;
    for (int b = 0; b < L; ++b)
        for (int i = 0; i < sizes[b]; ++i) {
            std::vector<double> row(d);
            double nn = 0.0;
            for (int t = 0; t < d; ++t) {
                row[t] = cen[(size_t)b * d + t] + (b == 3 ? 0.0 : 0.05 * gauss(rng));   // bucket 3: equal rows
                nn += row[t] * row[t];
            }
            const double s = metric == METRIC_IP ? 1.0 / std::sqrt(nn) : 1.0;
            for (int t = 0; t < d; ++t) X.push_back((float)(row[t] * s));
            lab.push_back(b);
        }
    const size_t N = lab.size();
    const Cover C = make_cover(X, lab, L, d);
    EXPECT(C.n[1] == 0 && C.R[2] == 0.0f);
    const int nq = 48;
    for (int qi = 0; qi < nq; ++qi) {
        // a query near a stored row, now and then a far one
        std::vector<float> q(d);
        const size_t src = rng() % N;
        const double spread = qi % 6 == 5 ? 2.0 : 0.01;
        double nn = 0.0;
        std::vector<double> qd(d);
        for (int t = 0; t < d; ++t) { qd[t] = X[src * d + t] + spread * gauss(rng); nn += qd[t] * qd[t]; }
        for (int t = 0; t < d; ++t) q[t] = (float)(metric == METRIC_IP ? qd[t] / std::sqrt(nn) : qd[t]);
        const double qn = norm_of(q.data(), d);
        std::vector<float> dist(N), sorted;
        for (size_t i = 0; i < N; ++i) dist[i] = scan_dist(metric, q.data(), &X[i * d], d);
        sorted = dist;
        std::sort(sorted.begin(), sorted.end());
        const float radii[] = {sorted[0], sorted[4], sorted[39], sorted[N - 1], std::nextafterf(sorted[0], -INFINITY)};
        for (float radius : radii) {
            std::vector<char> needed(L, 0);
            for (size_t i = 0; i < N; ++i)
                if (dist[i] <= radius) needed[lab[i]] = 1;   // the scan's comparison, in binary32
            for (int b = 0; b < L; ++b) {
                const bool adm = admit(metric, q.data(), qn, &C.c[(size_t)b * d], C.cn[b], C.R[b], C.n[b], radius, d);
                ++g_pairs;
                g_admitted += adm;
                if (needed[b]) {
                    ++g_needed;
                    EXPECT(adm);   // no needed pair may be missed
                }
                if (C.n[b] == 0) EXPECT(!adm);
                // a smaller margin may only prune more, a larger one only admit more
                const bool half = admit(metric, q.data(), qn, &C.c[(size_t)b * d], C.cn[b], C.R[b], C.n[b], radius, d, 0.5);
                const bool twice = admit(metric, q.data(), qn, &C.c[(size_t)b * d], C.cn[b], C.R[b], C.n[b], radius, d, 2.0);
                EXPECT((!half || adm) && (!adm || twice));
            }
        }
        // the radii that are no numbers, a bucket that is always visited, a query that is no number
        for (int b = 0; b < L; ++b) {
            const float* cb = &C.c[(size_t)b * d];
            const bool has = C.n[b] > 0;
            EXPECT(!admit(metric, q.data(), qn, cb, C.cn[b], C.R[b], C.n[b], std::numeric_limits<float>::quiet_NaN(), d));
            EXPECT(!admit(metric, q.data(), qn, cb, C.cn[b], C.R[b], C.n[b], -INFINITY, d));
            EXPECT(admit(metric, q.data(), qn, cb, C.cn[b], C.R[b], C.n[b], INFINITY, d) == has);
            EXPECT(admit(metric, q.data(), qn, cb, C.cn[b], INFINITY, C.n[b], sorted[0], d) == has);
            EXPECT(admit(metric, q.data(), qn, cb, C.cn[b], INFINITY, C.n[b], -1.0e30f, d) == has);
            std::vector<float> bad = q;
            bad[d / 2] = std::numeric_limits<float>::quiet_NaN();
            EXPECT(admit(metric, bad.data(), norm_of(bad.data(), d), cb, C.cn[b], C.R[b], C.n[b], sorted[0], d) == has);
        }
    }
}

int main() {
    // the round-up of the covering radius
    EXPECT(radius_of(0.0) == 0.0f);
    EXPECT(radius_of(INFINITY) == INFINITY && radius_of(std::numeric_limits<double>::quiet_NaN()) == INFINITY);
    EXPECT(radius_of(4.0) == std::nextafterf(2.0f, INFINITY));
    for (double r2 : {1.0e-30, 0.1, 1.0 / 3.0, 2.0, 12345.678, 3.0e30}) {
        const float R = radius_of(r2);
        EXPECT((double)R > std::sqrt(r2) && (double)R <= std::sqrt(r2) * (1.0 + 0x1p-22));
    }
    EXPECT(margin_unit(24) == 32.0 * 0x1p-23 && margin_unit(24, 2.0) == 64.0 * 0x1p-23);
    // geometry
    EXPECT(words_per_query(1) == 2 && words_per_query(64) == 2 && words_per_query(65) == 4 && words_per_query(70) == 4);
    EXPECT(query_rows_ok(0) && query_rows_ok(MAX_QUERY_ROWS) && !query_rows_ok(-1) && !query_rows_ok(MAX_QUERY_ROWS + 1));
    EXPECT(query_rows_for(0, 100, 12) == 100 && query_rows_for(32, 100, 12) == 32 && query_rows_for(32, 7, 12) == 7);
    EXPECT(query_rows_for(0, 1 << 20, 12) == DEFAULT_QUERY_ROWS);
    EXPECT(query_rows_for(0, 1 << 20, 65535) * words_per_query(65535) * 4 <= BITMAP_BYTES && query_rows_for(0, 1 << 20, 65535) >= 1);
    EXPECT(groups_for(0, 1) == 0 && groups_for(1, 1) == 1 && groups_for(100, 32) == 4 && groups_for(64, 32) == 2);
    {
        const int32_t counts[] = {1, 0, 5, 2, 7};
        int32_t m = -1;
        EXPECT(first_over(counts, 5, 4, &m) == 2 && m == 7);
        EXPECT(first_over(counts, 5, 7, &m) == -1 && m == 7);
        EXPECT(first_over(counts, 0, 0, &m) == -1 && m == 0);
    }
    unsigned seed = 1;
    for (int metric : {METRIC_IP, METRIC_L2})
        for (int d : {1, 24, 33, 70}) run_case(metric, d, seed++);
    EXPECT(g_needed > 2000);
    // well-separated clusters from d = 24 on: the rule prunes; it does not pass by admitting everything
    EXPECT(g_admitted * 2 < g_pairs);
    std::printf("cover plan selftest: clean (%ld checks, %ld needed pairs of %ld, %ld admitted)\n", g_checks, g_needed, g_pairs, g_admitted);
    return 0;
}
