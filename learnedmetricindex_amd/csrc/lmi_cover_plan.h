// lmi_cover_plan.h -- the arithmetic of the bucket cover and of its admission rule (include/lmi_hip.h states the contract; host:
// lmi_host_cover.h; kernels: lmi_cover.h; DESIGN.md 5.14.6 holds the proof).
//   radius_of      a bucket's covering radius from the maximum of its rows' binary64 chains: rounded to binary32 and then UP by one
//   link / tail    the admission rule of one (query, bucket) pair: the chain over the columns, one link at a time in ascending
//                  order, and what is decided from the finished chain.  cover_admit_kernel runs the links with the chain in a
//                  register and then the tail; admit() below runs the same two over whole rows.
//   words, groups  the geometry of the admission bitmap and the cut of the queries into groups
// Everything that decides is binary64 with explicit fma() calls and no product that feeds a sum otherwise, so that no compiler
// contracts anything and the host and the device decide alike.  Pure: <cmath> only, no HIP call, no handle;
// tests/host/cover_selftest.cpp checks the rule against a brute force on the CPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LMI_COVER_HD __host__ __device__
#else
#define LMI_COVER_HD
#endif

namespace lmi_cover_plan {

constexpr int METRIC_IP = 0, METRIC_L2 = 1;          // LMI_METRIC_IP, LMI_METRIC_L2
constexpr int64_t MAX_BUCKET_ROWS = 1ll << 26;       // the bound of the int64 sums: 2^26 rows of |q(x)| < 2^36 (lmi_kmeans's)
constexpr int SUM_BITS = 36;                         // q(v) = rint(v * 2^(SUM_BITS - e))
constexpr int MAX_ORDER_BUCKETS = 1024;              // the range scan's limit on n_buckets
constexpr int64_t DEFAULT_QUERY_ROWS = 1 << 14;      // queries per group unless the hook says otherwise
constexpr int64_t MAX_QUERY_ROWS = 1ll << 20;        // what lmi_cover_set_geometry takes at most
constexpr int64_t BITMAP_BYTES = 64ll << 20;         // a group's bitmap stays below this where one query's row allows it

// ---- the cover ----
// R_b from R2_b, the maximum over the bucket's live rows of the chain acc = fma(delta, delta, acc): 0 stays 0 (one row, equal rows);
// anything else is rounded to binary32 and moved one step up, which is never below the binary64 root; a maximum that is not finite
// (a row held inf or NaN) gives +inf, and such a bucket is always visited.
LMI_COVER_HD inline float radius_of(double R2) {
    if (R2 == 0.0) return 0.0f;
    if (!(R2 < INFINITY)) return INFINITY;
    return nextafterf((float)sqrt(R2), INFINITY);
}
// one link of a row's chain about its centre
LMI_COVER_HD inline double radius_link(double acc, float x, float c) {
    const double delta = (double)x - (double)c;
    return fma(delta, delta, acc);
}
// sqrt(sum v[t]^2): |q| of a query, |c_b| of a centre; one chain, t ascending
LMI_COVER_HD inline double norm_of(const float* v, int d) {
    double acc = 0.0;
    for (int t = 0; t < d; ++t) acc = fma((double)v[t], (double)v[t], acc);
    return sqrt(acc);
}

// ---- the admission rule ----
// u = (d + 8) * 2^-23: twice the classical constant of the scan's binary32 chains; `factor` scales it (1 in the
// library; the tests halve and double it to bracket the admitted set)
LMI_COVER_HD inline double margin_unit(int d, double factor = 1.0) { return factor * (double)(d + 8) * 0x1p-23; }

// one link of the (query, bucket) chain: IP sum q[t] c[t]; L2 sum (q[t] - c[t])^2
LMI_COVER_HD inline double link(int metric, double acc, float q, float c) {
    if (metric == METRIC_IP) return fma((double)q, (double)c, acc);
    const double delta = (double)q - (double)c;
    return fma(delta, delta, acc);
}

// The verdict from the finished chain.  qn = |q|, cn = |c_b| (norm_of), R = R_b, n_b the bucket's live rows, u = margin_unit(d).
// IP: pruned iff  chain + qn R  <  1 - r - u (1 + |r| + qn (cn + R)).
// L2: pruned iff  max(0, sqrt(chain) - R)^2  >  r + u (qn + cn + R)^2.
// Admitted iff the bucket has rows, the radius is neither NaN nor -inf, and it is not pruned; the comparisons are written so that a
// NaN anywhere admits.
LMI_COVER_HD inline bool tail(int metric, double chain, double qn, double cn, float R, int64_t n_b, float radius, double u) {
    if (n_b <= 0) return false;
    if (radius != radius || radius == -INFINITY) return false;
    const double r = (double)radius, Rb = (double)R;
    if (metric == METRIC_IP) {
        const double ub = fma(qn, Rb, chain);
        const double scale = fma(qn, cn + Rb, 1.0 + fabs(r));
        const double thr = fma(-u, scale, 1.0 - r);
        return !(ub < thr);
    }
    const double dc = sqrt(chain);
    const double lo = fmax(0.0, dc - Rb);   // (fmax drops a NaN: lo = 0 admits)
    const double s = qn + cn + Rb;
    const double s2 = s * s;
    const double thr = fma(u, s2, r);
    const double lo2 = lo * lo;
    return !(lo2 > thr);
}

// the rule over whole rows: what one thread of cover_admit_kernel computes for its (query, bucket)
LMI_COVER_HD inline bool admit(int metric, const float* q, double qn, const float* c, double cn, float R, int64_t n_b, float radius, int d,
                               double factor = 1.0) {
    double chain = 0.0;
    for (int t = 0; t < d; ++t) chain = link(metric, chain, q[t], c[t]);
    return tail(metric, chain, qn, cn, R, n_b, radius, margin_unit(d, factor));
}

// ---- geometry ----
// 32-bit words of one query's row of the bitmap: bucket b is bit b & 31 of word b >> 5; a wave judges 64 buckets and writes two
// words, so a row holds an even number of them
LMI_COVER_HD inline int64_t words_per_query(int64_t L) { return 2 * ((L + 63) / 64); }
inline bool query_rows_ok(int64_t query_rows) { return query_rows >= 0 && query_rows <= MAX_QUERY_ROWS; }
// queries per group: the hook's value; else DEFAULT_QUERY_ROWS, fewer where the bitmap would pass BITMAP_BYTES (at least 1)
inline int64_t query_rows_for(int64_t forced, int64_t nq, int64_t L) {
    int64_t rows = forced > 0 ? forced : DEFAULT_QUERY_ROWS;
    if (forced <= 0) {
        const int64_t fit = BITMAP_BYTES / (words_per_query(L) * 4);
        if (rows > fit) rows = fit;
        if (rows < 1) rows = 1;
    }
    if (rows > nq) rows = nq;
    return rows < 1 ? 1 : rows;
}
inline int64_t groups_for(int64_t nq, int64_t query_rows) { return nq <= 0 ? 0 : (nq + query_rows - 1) / query_rows; }

// the first query whose count exceeds nb (-1: none); *max_count <- the largest count (0 for nq == 0)
inline int64_t first_over(const int32_t* counts, int64_t nq, int64_t nb, int32_t* max_count) {
    int64_t first = -1;
    int32_t m = 0;
    for (int64_t q = 0; q < nq; ++q) {
        if (counts[q] > m) m = counts[q];
        if (first < 0 && counts[q] > nb) first = q;
    }
    if (max_count) *max_count = m;
    return first;
}

}  // namespace lmi_cover_plan
