// lmi_fetch_plan.h -- the host arithmetic of lmi_rows_fetch (include/lmi_hip.h states the contract; host: lmi_host_fetch.h; kernels:
// lmi_fetch.h): from the caller's request list
//   unique       the requested ids sorted ascending, each once: what every live row of the index is searched in
//   map          per request the index of its id in `unique` (requests may repeat and come in any order; every occurrence of an id
//                reads the same word of the location table, so every occurrence gets the same answer)
//   pieces       the cut of [0, n) into runs of piece_rows requests: one gather launch and -- for host outputs -- one round through
//                the stage each
// Host only and pure: the standard library, no HIP call, no handle; tests/host/fetch_plan_selftest.cpp checks all of it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lmi_fetch_plan {

constexpr int64_t MAX_REQUESTS = (1ll << 31) - 1;    // n < 2^31: `map` and the tables are indexed by 32-bit words
constexpr int64_t MAX_PIECE_ROWS = 1ll << 24;        // what lmi_fetch_set_geometry takes at most
constexpr int64_t STAGE_BYTES = 64ll << 20;          // the default piece: what fits a stage of 64 MiB
constexpr int64_t TABLE_BYTES_PER_REQUEST = 16;      // at most: unique 4 + map 4 + location 8

inline bool n_ok(int64_t n) { return n >= 0 && n <= MAX_REQUESTS; }
inline bool piece_rows_ok(int64_t piece_rows) { return piece_rows >= 0 && piece_rows <= MAX_PIECE_ROWS; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// bytes of one request in a piece's stage: its row (d values of elt bytes; 0 for a pure locate) + bucket + row
inline int64_t request_bytes(int64_t d, int64_t elt, bool want_rows) { return (want_rows ? d * elt : 0) + 8; }
// requests per piece: the hook's value; else, for host outputs (staged), what a 64-MiB stage holds (at least 1, at most
// MAX_PIECE_ROWS); device outputs pass through no stage and take MAX_PIECE_ROWS requests per launch
inline int64_t piece_rows_for(int64_t forced, int64_t req_bytes, bool staged = true) {
    if (forced > 0) return forced;
    if (!staged) return MAX_PIECE_ROWS;
    return std::max<int64_t>(1, std::min<int64_t>(MAX_PIECE_ROWS, STAGE_BYTES / std::max<int64_t>(req_bytes, 1)));
}

struct Plan {
    int64_t n = 0, piece_rows = 0;
    std::vector<uint32_t> unique;   // ascending, no repeats
    std::vector<int32_t> map;       // [n]: unique[map[i]] == ids[i]
    int64_t pieces() const { return n == 0 ? 0 : cdiv(n, piece_rows); }
    int64_t piece_begin(int64_t p) const { return std::min(n, p * piece_rows); }
    int64_t piece_end(int64_t p) const { return std::min(n, (p + 1) * piece_rows); }
    int64_t table_bytes() const { return (int64_t)unique.size() * 12 + n * 4; }
};

// n requests (n_ok(n); ids may be null when n == 0), piece_rows > 0
inline Plan make_plan(const uint32_t* ids, int64_t n, int64_t piece_rows) {
    Plan P;
    P.n = n;
    P.piece_rows = piece_rows;
    if (n == 0) return P;
    P.unique.assign(ids, ids + n);
    std::sort(P.unique.begin(), P.unique.end());
    P.unique.erase(std::unique(P.unique.begin(), P.unique.end()), P.unique.end());
    P.map.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        P.map[(size_t)i] = (int32_t)(std::lower_bound(P.unique.begin(), P.unique.end(), ids[i]) - P.unique.begin());
    return P;
}

// ---- what the kernels compute, restated for the host (the selftest and the counting of FOUND) ----
constexpr uint64_t ABSENT = ~0ull;   // a word of the location table no live row has lowered
inline uint64_t loc_word(int32_t bucket, int32_t row) { return ((uint64_t)(uint32_t)bucket << 32) | (uint32_t)row; }
inline int32_t loc_bucket(uint64_t w) { return w == ABSENT ? -1 : (int32_t)(w >> 32); }
inline int32_t loc_row(uint64_t w) { return w == ABSENT ? -1 : (int32_t)(w & 0xffffffffu); }

}  // namespace lmi_fetch_plan
