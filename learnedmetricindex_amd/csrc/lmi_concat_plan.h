// lmi_concat_plan.h -- the host arithmetic of lmi_concat (include/lmi_hip.h states the contract; host: lmi_host_concat.h; kernels:
// lmi_concat.h): whether the parts go together, the result's per-bucket counts, the first in-bucket row every (part, bucket) takes,
// the limits of the 32-bit slab positions and the fresh layout that follows from the counts (lmi_layout::fresh_layout).
//   order rule   bucket b of the result is parts[0]'s bucket b, then parts[1]'s, ...: part t's objects of bucket b take the in-bucket
//                rows [offset(t, b), offset(t, b) + rows(t, b)), offset(t, b) = the rows of bucket b in the parts before t
//   source map   per row of the new slab 8 bytes: the part and the part's slab row it is gathered from
// Host only and pure: the standard library, no HIP call, no handle; tests/host/concat_plan_selftest.cpp checks all of it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lmi_layout.h"

namespace lmi_concat_plan {

constexpr int MAX_PARTS = 64;                     // LMI_CONCAT_MAX_PARTS
constexpr int64_t BYTES_PER_NEW_SLAB_ROW = 8;     // the source map: (part, slab row of the part)

// what has to agree between parts[0] and every other part
struct Shape {
    int device = 0, d = 0, L = 0, metric = 0, storage = 0;
    bool prefilter = true;
    std::vector<unsigned char> owned;   // lmi_buckets_begin's mask (empty: every bucket)
};

enum Problem {
    OK = 0,
    BAD_N_PARTS,        // value = n_parts
    DEVICE,             // part, value = its device, want = parts[0]'s   (and so on: the property the message names)
    DIMS,
    BUCKETS,
    METRIC,
    STORAGE,
    PREFILTER,
    OWNED,              // value / want: 1 = carries a mask, 0 = none; both 1: the masks differ, at = the first bucket where
    N_PAST_LIMIT,       // value = the sum of the parts' N
    BUCKET_PAST_LIMIT,  // at = the bucket, value = its rows
    TOTAL_PAST_LIMIT    // value = the row-blocks of the layout
};
struct Verdict {
    Problem problem = OK;
    int part = 0;
    int64_t at = 0, value = 0, want = 0;
};

inline bool n_parts_ok(int64_t n_parts) { return n_parts >= 1 && n_parts <= MAX_PARTS; }

// parts[t] against parts[0], in part order; within a part in the order of the enum
inline Verdict compatible(const std::vector<Shape>& parts) {
    if (!n_parts_ok((int64_t)parts.size())) return Verdict{BAD_N_PARTS, 0, 0, (int64_t)parts.size(), 0};
    const Shape& a = parts[0];
    for (size_t t = 1; t < parts.size(); ++t) {
        const Shape& p = parts[t];
        const int ti = (int)t;
        if (p.device != a.device) return Verdict{DEVICE, ti, 0, p.device, a.device};
        if (p.d != a.d) return Verdict{DIMS, ti, 0, p.d, a.d};
        if (p.L != a.L) return Verdict{BUCKETS, ti, 0, p.L, a.L};
        if (p.metric != a.metric) return Verdict{METRIC, ti, 0, p.metric, a.metric};
        if (p.storage != a.storage) return Verdict{STORAGE, ti, 0, p.storage, a.storage};
        if (p.prefilter != a.prefilter) return Verdict{PREFILTER, ti, 0, p.prefilter, a.prefilter};
        if (p.owned.empty() != a.owned.empty()) return Verdict{OWNED, ti, 0, !p.owned.empty(), !a.owned.empty()};
        for (size_t b = 0; b < a.owned.size(); ++b)
            if ((p.owned[b] != 0) != (a.owned[b] != 0)) return Verdict{OWNED, ti, (int64_t)b, 1, 1};
    }
    return Verdict();
}

struct Plan {
    Verdict verdict;
    int n_parts = 0, L = 0;
    std::vector<int> counts;           // [L]: rows per bucket of the result
    std::vector<int> offsets;          // [n_parts][L]: the first in-bucket row of part t's objects of bucket b
    std::vector<unsigned char> any;    // [L]: the bucket holds rows on some rank, in any part
    int64_t rows = 0;                  // objects the result stores
    int64_t N = 0;                     // the sum of the parts' N (a sharded rank: objects on every rank)
    std::vector<int> rb_start, cap_rb; // the fresh layout of `counts`
    int64_t n_rb_total = 0;
    int offset(int t, int b) const { return offsets[(size_t)t * L + b]; }
    int64_t map_bytes() const { return BYTES_PER_NEW_SLAB_ROW * n_rb_total * 32; }
};

// rows[t][b]: the rows part t stores in bucket b; any[t][b]: part t's word that the bucket holds rows on some rank; N[t]: part t's N.
// On a refusal only `verdict` is meaningful.
inline Plan plan(const std::vector<std::vector<int>>& rows, const std::vector<std::vector<unsigned char>>& any, const std::vector<int64_t>& N) {
    Plan P;
    P.n_parts = (int)rows.size();
    P.L = rows.empty() ? 0 : (int)rows[0].size();
    const int L = P.L;
    const int64_t max_rb = lmi_layout::max_slab_rb(L);
    std::vector<int64_t> sum((size_t)L, 0);
    P.offsets.assign((size_t)P.n_parts * L, 0);
    P.any.assign((size_t)L, 0);
    for (int t = 0; t < P.n_parts; ++t) {
        P.N += N[(size_t)t];
        for (int b = 0; b < L; ++b) {
            // (past the limit the offset is never used: the call is refused below)
            P.offsets[(size_t)t * L + b] = (int)std::min<int64_t>(sum[(size_t)b], INT32_MAX);
            sum[(size_t)b] += rows[(size_t)t][(size_t)b];
            P.any[(size_t)b] |= any[(size_t)t][(size_t)b] != 0;
        }
    }
    if (P.N >= (1ll << 31) - 64ll * L) { P.verdict = Verdict{N_PAST_LIMIT, 0, 0, P.N, 0}; return P; }
    int64_t total_rb = 0;
    for (int b = 0; b < L; ++b) {
        const int64_t rb = lmi_layout::cdiv(sum[(size_t)b], 32);
        if (rb > max_rb) { P.verdict = Verdict{BUCKET_PAST_LIMIT, 0, b, sum[(size_t)b], 0}; return P; }
        total_rb += rb;
        P.rows += sum[(size_t)b];
    }
    if (total_rb > max_rb) { P.verdict = Verdict{TOTAL_PAST_LIMIT, 0, 0, total_rb, 0}; return P; }
    P.counts.resize((size_t)L);
    for (int b = 0; b < L; ++b) P.counts[(size_t)b] = (int)sum[(size_t)b];
    P.n_rb_total = lmi_layout::fresh_layout(P.counts, P.rb_start, P.cap_rb);
    return P;
}

}  // namespace lmi_concat_plan
