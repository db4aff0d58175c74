// lmi_range_sort_plan.h -- the host arithmetic of the sort of a range result by distance (lmi_range_result_sort; include/lmi_hip.h
// states the contract; kernels: lmi_range_sort.h): from lims alone to the form every segment is sorted in, the
// groups of whole segments whose scratch stays within a budget, and for the long form the tiles, the merge passes and the merge
// pieces.  A segment is a query's [lims[q], lims[q + 1]).
//   skipped   0 or 1 entries: nothing to do
//   wave      2 .. wave_rows entries: one wave per segment, the entries in registers (WAVE_ROWS = 4 per lane)
//   tile      up to tile_rows (T) entries: one block per segment, sorted in LDS
//   long      above T: tiles of T entries sorted in LDS into a key buffer, then ceil(log2(tiles)) merge passes that double the run
//             length, every pass cut into output pieces of merge_rows entries
// Host only and pure: the standard library, no HIP call, no handle; tests/host/range_sort_selftest.cpp checks all of it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lmi_range_sort_plan {

constexpr int64_t WAVE_ROWS = 256;            // the wave form's registers: 4 entries per lane of a wave of 64
constexpr int64_t MIN_TILE_ROWS = 64;
constexpr int64_t MAX_TILE_ROWS = 8192;       // the LDS form's limit: 64 KiB of 8-byte entries, two blocks per CU of 160 KiB
constexpr int64_t DEFAULT_TILE_ROWS = MAX_TILE_ROWS;
constexpr int64_t MAX_MERGE_ROWS = 2048;      // entries of one merge piece (16 KiB of LDS); never above T
constexpr int64_t DEFAULT_SCRATCH_BYTES = 1ll << 30;
constexpr int64_t MAX_SCRATCH_BYTES = 1ll << 40;
constexpr int64_t ENTRY_BYTES = 24;           // what a group is cut by: two 8-byte key words and the 8 bytes of the permuted copy
constexpr int64_t MAX_SEGMENT = (1ll << 32) - 1;   // the position inside a segment is a 32-bit word and all ones is the padding

inline bool power_of_two(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// what lmi_range_sort_set_geometry accepts: 0 = the default
inline bool tile_rows_ok(int64_t t) { return t == 0 || (power_of_two(t) && t >= MIN_TILE_ROWS && t <= MAX_TILE_ROWS); }
inline bool scratch_bytes_ok(int64_t b) { return b >= 0 && b <= MAX_SCRATCH_BYTES; }

inline int64_t tile_rows_for(int64_t forced) { return forced > 0 ? forced : DEFAULT_TILE_ROWS; }
inline int64_t scratch_for(int64_t forced) { return forced > 0 ? forced : DEFAULT_SCRATCH_BYTES; }
// A forced T below 2 * WAVE_ROWS lowers the wave form's limit to T / 2, so that every T leaves the tile form segments of its own.
inline int64_t wave_rows_for(int64_t T) { return std::min(WAVE_ROWS, T / 2); }
inline int64_t merge_rows_for(int64_t T) { return std::min(MAX_MERGE_ROWS, T); }

enum Form { SKIPPED = 0, WAVE, TILE, LONG };
inline Form form_of(int64_t len, int64_t T) {
    if (len <= 1) return SKIPPED;
    if (len <= wave_rows_for(T)) return WAVE;
    return len <= T ? TILE : LONG;
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// the power of two a tile or a wave's segment is padded to (>= 2)
inline int64_t padded(int64_t n) {
    int64_t p = 2;
    while (p < n) p <<= 1;
    return p;
}
inline int64_t tiles_of(int64_t len, int64_t T) { return cdiv(len, T); }
// merge passes of a long segment: runs of T, 2T, 4T .. until one run holds the segment
inline int passes_of(int64_t len, int64_t T) {
    int p = 0;
    for (int64_t run = T; run < len; run <<= 1) ++p;
    return p;
}
inline int64_t merge_pieces_of(int64_t len, int64_t T) { return cdiv(len, merge_rows_for(T)); }

// The two functions range_sort_merge_kernel runs (lmi_range_sort.h), written without the standard library so that device code can
// call them; the self-test replays a pass with them on the CPU.
#if defined(__HIPCC__)
#define LMI_RANGE_SORT_HD __host__ __device__
#else
#define LMI_RANGE_SORT_HD
#endif
// One output piece of a merge pass over n keys in runs of `run` (the last run may be shorter): piece b produces out [o0, o1); it lies
// in ONE pair of runs because 2 * run is a multiple of merge_rows.  The pair is A = [p0, p0 + la), B = [p0 + la, p0 + la + lb); lb may be
// 0 (an odd run at the end: copied).
struct Piece {
    int64_t o0, o1, p0, la, lb;
};
LMI_RANGE_SORT_HD inline Piece merge_piece(int64_t n, int64_t run, int64_t merge_rows, int64_t b) {
    Piece P;
    P.o0 = b * merge_rows;
    P.o1 = P.o0 + merge_rows < n ? P.o0 + merge_rows : n;
    P.p0 = P.o0 / (2 * run) * (2 * run);
    P.la = run < n - P.p0 ? run : n - P.p0;
    P.lb = run < n - P.p0 - P.la ? run : n - P.p0 - P.la;
    return P;
}
// The merge path: how many of the first d outputs of merge(A, B) come from A.  Keys are unique, so the split is unique.
template <class K>
LMI_RANGE_SORT_HD inline int64_t merge_split(const K* A, int64_t la, const K* B, int64_t lb, int64_t d) {
    int64_t lo = d - lb > 0 ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] < B[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

enum Problem { OK = 0, BAD_LIMS, SEGMENT_TOO_LONG };
struct Verdict {
    Problem problem = OK;
    int64_t q = 0;       // the query
    int64_t value = 0;   // BAD_LIMS: lims[q + 1] - lims[q]; SEGMENT_TOO_LONG: the length
};

struct LongSeg {
    int64_t at, n;   // where the segment begins in the result's arrays, its length
    int64_t tiles, pieces;
    int passes;
};
// A group: the whole segments [q0, q1), entries [e0, e1) of the result; only groups with something to sort are kept.
struct Group {
    int64_t q0 = 0, q1 = 0, e0 = 0, e1 = 0;
    std::vector<long long> wave_at, tile_at;   // where each segment of the form begins in the result's arrays
    std::vector<int> wave_n, tile_n;           // its length
    std::vector<LongSeg> longs;
    int64_t longest = 0;                       // the longest long segment: what the two key buffers hold
    int64_t scratch_bytes() const { return 8 * (e1 - e0) + 16 * longest; }   // the copy + the key buffers: <= ENTRY_BYTES * (e1 - e0)
};

struct Plan {
    int64_t tile_rows = DEFAULT_TILE_ROWS, wave_rows = WAVE_ROWS, merge_rows = MAX_MERGE_ROWS, budget = DEFAULT_SCRATCH_BYTES;
    int64_t total = 0, skipped = 0, waves = 0, tiles = 0, longs = 0, scratch_bytes = 0;
    int max_passes = 0;
    std::vector<Group> groups;
};

// lims [nq + 1].  On a problem `out` is left in an unspecified state and must not be used.
inline Verdict make_plan(const int64_t* lims, int64_t nq, int64_t forced_tile_rows, int64_t forced_scratch, Plan& out) {
    out = Plan();
    out.tile_rows = tile_rows_for(forced_tile_rows);
    out.wave_rows = wave_rows_for(out.tile_rows);
    out.merge_rows = merge_rows_for(out.tile_rows);
    out.budget = scratch_for(forced_scratch);
    const int64_t T = out.tile_rows;
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t len = lims[q + 1] - lims[q];
        if (len < 0) return Verdict{BAD_LIMS, q, len};
        if (len > MAX_SEGMENT) return Verdict{SEGMENT_TOO_LONG, q, len};
    }
    out.total = nq > 0 ? lims[nq] - lims[0] : 0;
    Group G;
    bool open = false, work = false;
    auto close = [&]() {
        if (open && work) {
            out.scratch_bytes = std::max(out.scratch_bytes, G.scratch_bytes());
            out.groups.push_back(std::move(G));
        }
        G = Group();
        open = work = false;
    };
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t at = lims[q], len = lims[q + 1] - at;
        // a segment is never split: one that does not fit beside the group's others begins the next group, one above the budget is alone
        if (open && ENTRY_BYTES * (G.e1 - G.e0 + len) > out.budget) close();
        if (!open) {
            G.q0 = q;
            G.e0 = at;
            open = true;
        }
        G.q1 = q + 1;
        G.e1 = at + len;
        switch (form_of(len, T)) {
        case SKIPPED: ++out.skipped; break;
        case WAVE:
            G.wave_at.push_back(at);
            G.wave_n.push_back((int)len);
            ++out.waves;
            work = true;
            break;
        case TILE:
            G.tile_at.push_back(at);
            G.tile_n.push_back((int)len);
            ++out.tiles;
            work = true;
            break;
        case LONG: {
            const LongSeg S{at, len, tiles_of(len, T), merge_pieces_of(len, T), passes_of(len, T)};
            G.longs.push_back(S);
            G.longest = std::max(G.longest, len);
            out.max_passes = std::max(out.max_passes, S.passes);
            ++out.longs;
            work = true;
            break;
        }
        }
    }
    close();
    return Verdict();
}

}  // namespace lmi_range_sort_plan
