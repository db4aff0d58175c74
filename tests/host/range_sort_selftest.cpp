// range_sort_selftest.cpp -- stand-alone check of the host arithmetic of the sort of a range result (csrc/lmi_range_sort_plan.h: pure
// host code) on the CPU, meant for -fsanitize=address,undefined (tests/test_range_sort_host.py builds and runs it).
//   - the form of a segment on both sides of every seam (1 | 2, wave_rows | + 1, T | + 1) for every T the hook accepts;
//   - what the hook accepts and refuses;
//   - for random lims: every segment is in exactly one form of exactly one group or skipped; groups are runs of whole consecutive
//     segments in order; a group's 24 bytes per entry stay within the budget unless it is one segment taken alone; the scratch word is
//     the largest group's copy + key buffers; passes, tiles and pieces of the long segments;
//   - the merge pass as range_sort_merge_kernel runs it, replayed here on unique words: the pieces tile [0, n) exactly once, each
//     lies in one pair of runs, its A and B parts together are exactly the piece (so they fit the M words of LDS), and after
//     passes_of passes the words ascend -- for run boundaries that fall anywhere (n no multiple of T, an odd run at the end);
//   - descending lims and a segment of 2^32 entries are reported, not planned; nq = 0.
#include "lmi_range_sort_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace lmi_range_sort_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void check_forms() {
    for (int64_t T = MIN_TILE_ROWS; T <= MAX_TILE_ROWS; T <<= 1) {
        const int64_t W = wave_rows_for(T);
        EXPECT(W >= 2 && W <= WAVE_ROWS && W < T && W <= T / 2);
        EXPECT(form_of(0, T) == SKIPPED && form_of(1, T) == SKIPPED && form_of(2, T) == WAVE);
        EXPECT(form_of(W, T) == WAVE && form_of(W + 1, T) == TILE);
        EXPECT(form_of(T, T) == TILE && form_of(T + 1, T) == LONG && form_of(MAX_SEGMENT, T) == LONG);
        EXPECT(merge_rows_for(T) <= T && power_of_two(merge_rows_for(T)) && merge_rows_for(T) <= MAX_MERGE_ROWS);
        EXPECT(passes_of(T + 1, T) == 1 && passes_of(2 * T, T) == 1 && passes_of(2 * T + 1, T) == 2 && passes_of(4 * T, T) == 2);
        EXPECT(tiles_of(T + 1, T) == 2 && tiles_of(2 * T, T) == 2);
    }
    EXPECT(wave_rows_for(DEFAULT_TILE_ROWS) == WAVE_ROWS && wave_rows_for(512) == 256 && wave_rows_for(256) == 128 && wave_rows_for(128) == 64);
    EXPECT(padded(2) == 2 && padded(3) == 4 && padded(64) == 64 && padded(65) == 128 && padded(8192) == 8192);
    EXPECT(tile_rows_ok(0) && tile_rows_ok(64) && tile_rows_ok(128) && tile_rows_ok(8192));
    EXPECT(!tile_rows_ok(-1) && !tile_rows_ok(32) && !tile_rows_ok(100) && !tile_rows_ok(16384) && !tile_rows_ok(65));
    EXPECT(scratch_bytes_ok(0) && scratch_bytes_ok(1) && scratch_bytes_ok(MAX_SCRATCH_BYTES) && !scratch_bytes_ok(MAX_SCRATCH_BYTES + 1) &&
           !scratch_bytes_ok(-1));
    EXPECT(MAX_TILE_ROWS * 8 * 2 <= 160 * 1024 && MAX_TILE_ROWS * 2 * 8 * 2 > 160 * 1024);   // the largest T two blocks per CU leave room for
}

static std::vector<int64_t> random_lims(std::mt19937& rng, int64_t nq, int64_t T, int big) {
    auto rnd = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    const int seams[] = {0, 1, 2, 3, (int)wave_rows_for(T) - 1, (int)wave_rows_for(T), (int)wave_rows_for(T) + 1, (int)T - 1, (int)T, (int)T + 1,
                         2 * (int)T, 2 * (int)T + 1};
    std::vector<int64_t> lims((size_t)nq + 1, 0);
    for (int64_t q = 0; q < nq; ++q) {
        const int kind = rnd(0, 9);
        const int n = kind < 2 ? rnd(0, 1) : kind < 6 ? rnd(2, 150) : kind < 8 ? seams[rnd(0, 11)] : rnd(1, big);
        lims[(size_t)q + 1] = lims[(size_t)q] + n;
    }
    return lims;
}

static void check_plan(const std::vector<int64_t>& lims, int64_t forced_T, int64_t forced_scratch) {
    const int64_t nq = (int64_t)lims.size() - 1;
    Plan P;
    const Verdict v = make_plan(lims.data(), nq, forced_T, forced_scratch, P);
    EXPECT(v.problem == OK);
    const int64_t T = tile_rows_for(forced_T), budget = scratch_for(forced_scratch);
    EXPECT(P.tile_rows == T && P.wave_rows == wave_rows_for(T) && P.merge_rows == merge_rows_for(T) && P.budget == budget);
    EXPECT(P.total == lims.back());
    std::vector<int> seen((size_t)nq, 0);
    int64_t waves = 0, tiles = 0, longs = 0, scratch = 0, prev_q1 = 0;
    int passes = 0;
    for (const Group& G : P.groups) {
        EXPECT(G.q0 >= prev_q1 && G.q1 > G.q0 && G.q1 <= nq);   // in order, disjoint, whole segments
        prev_q1 = G.q1;
        EXPECT(G.e0 == lims[(size_t)G.q0] && G.e1 == lims[(size_t)G.q1]);
        EXPECT(G.wave_at.size() == G.wave_n.size() && G.tile_at.size() == G.tile_n.size());
        EXPECT(!G.wave_n.empty() || !G.tile_n.empty() || !G.longs.empty());   // only groups with work are kept
        if (ENTRY_BYTES * (G.e1 - G.e0) > budget) {   // over the budget: one segment with entries, taken alone
            int64_t with_entries = 0;
            for (int64_t q = G.q0; q < G.q1; ++q) with_entries += lims[(size_t)q + 1] > lims[(size_t)q];
            EXPECT(with_entries == 1);
        }
        EXPECT(G.scratch_bytes() <= ENTRY_BYTES * (G.e1 - G.e0));
        scratch = std::max(scratch, G.scratch_bytes());
        // the group's tables name its segments, in order, each once
        size_t iw = 0, it = 0, il = 0;
        int64_t longest = 0;
        for (int64_t q = G.q0; q < G.q1; ++q) {
            const int64_t at = lims[(size_t)q], n = lims[(size_t)q + 1] - at;
            ++seen[(size_t)q];
            switch (form_of(n, T)) {
            case SKIPPED: break;
            case WAVE:
                EXPECT(iw < G.wave_n.size() && G.wave_at[iw] == at && G.wave_n[iw] == n && n >= 2 && n <= WAVE_ROWS);
                ++iw;
                break;
            case TILE:
                EXPECT(it < G.tile_n.size() && G.tile_at[it] == at && G.tile_n[it] == n && n <= T && padded(n) <= T);
                ++it;
                break;
            case LONG:
                EXPECT(il < G.longs.size() && G.longs[il].at == at && G.longs[il].n == n);
                EXPECT(G.longs[il].tiles == cdiv(n, T) && G.longs[il].pieces == cdiv(n, P.merge_rows) && G.longs[il].passes == passes_of(n, T));
                EXPECT((T << G.longs[il].passes) >= n && (G.longs[il].passes == 0 || (T << (G.longs[il].passes - 1)) < n));
                passes = std::max(passes, G.longs[il].passes);
                longest = std::max(longest, n);
                ++il;
                break;
            }
        }
        EXPECT(iw == G.wave_n.size() && it == G.tile_n.size() && il == G.longs.size() && longest == G.longest);
        waves += (int64_t)iw;
        tiles += (int64_t)it;
        longs += (int64_t)il;
    }
    int64_t skipped = 0;
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t n = lims[(size_t)q + 1] - lims[(size_t)q];
        skipped += n <= 1;
        EXPECT(seen[(size_t)q] <= 1 && (n <= 1 || seen[(size_t)q] == 1));   // a sortable segment is in exactly one group
    }
    EXPECT(P.waves == waves && P.tiles == tiles && P.longs == longs && P.skipped == skipped && waves + tiles + longs + skipped == nq);
    EXPECT(P.max_passes == passes && P.scratch_bytes == scratch);
}

// one long segment of n unique words, as the kernels sort it: tiles of T, then passes of pieces of M words
static void check_merge(std::mt19937& rng, int64_t n, int64_t T) {
    const int64_t M = merge_rows_for(T);
    std::vector<uint64_t> a((size_t)n), b((size_t)n), lds((size_t)M);
    for (int64_t i = 0; i < n; ++i) a[(size_t)i] = ((uint64_t)(rng() % 7) << 32) | (uint64_t)i;   // heavy ties in the key, unique words
    std::vector<uint64_t> want = a;
    std::sort(want.begin(), want.end());
    for (int64_t s = 0; s < n; s += T) std::sort(a.begin() + s, a.begin() + std::min(n, s + T));
    int passes = 0;
    for (int64_t run = T; run < n; run <<= 1, ++passes) {
        std::vector<char> written((size_t)n, 0);
        for (int64_t p = 0; p < cdiv(n, M); ++p) {
            const Piece X = merge_piece(n, run, M, p);
            EXPECT(X.o0 < X.o1 && X.o1 <= n && X.o1 - X.o0 <= M && X.p0 <= X.o0 && X.p0 % (2 * run) == 0);
            EXPECT(X.la >= 1 && X.la <= run && X.lb >= 0 && X.lb <= run && X.o1 <= X.p0 + X.la + X.lb);   // in ONE pair of runs
            const uint64_t* A = a.data() + X.p0;
            const uint64_t* B = A + X.la;
            const int64_t i0 = merge_split(A, X.la, B, X.lb, X.o0 - X.p0), i1 = merge_split(A, X.la, B, X.lb, X.o1 - X.p0);
            const int64_t j0 = X.o0 - X.p0 - i0, na = i1 - i0, nb = (X.o1 - X.o0) - na;
            EXPECT(i0 >= 0 && i1 >= i0 && i1 <= X.la && j0 >= 0 && nb >= 0 && j0 + nb <= X.lb && na + nb <= M);
            // the LDS image: the A part ascending, padding, the B part descending
            for (int64_t t = 0; t < M; ++t)
                lds[(size_t)t] = t < na ? A[i0 + t] : t >= M - nb ? B[j0 + (M - 1 - t)] : ~0ull;
            for (int64_t stride = M >> 1; stride > 0; stride >>= 1)
                for (int64_t i = 0; i < (M >> 1); ++i) {
                    const int64_t lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
                    if (lds[(size_t)lo] > lds[(size_t)hi]) std::swap(lds[(size_t)lo], lds[(size_t)hi]);
                }
            for (int64_t t = 0; t < X.o1 - X.o0; ++t) {
                EXPECT(!written[(size_t)(X.o0 + t)]);
                written[(size_t)(X.o0 + t)] = 1;
                b[(size_t)(X.o0 + t)] = lds[(size_t)t];
            }
        }
        for (int64_t i = 0; i < n; ++i) EXPECT(written[(size_t)i]);
        for (int64_t s = 0; s < n; s += 2 * run)
            EXPECT(std::is_sorted(b.begin() + s, b.begin() + std::min(n, s + 2 * run)));
        a.swap(b);
    }
    EXPECT(passes == passes_of(n, T));
    EXPECT(a == want);
}

int main() {
    std::mt19937 rng(20261020);
    check_forms();
    for (int rep = 0; rep < 40; ++rep)
        for (int64_t T : {(int64_t)0, (int64_t)64, (int64_t)128, (int64_t)256, (int64_t)1024})
            for (int64_t scratch : {(int64_t)0, (int64_t)24 * 100, (int64_t)24 * 5000, (int64_t)1}) {
                const std::vector<int64_t> lims = random_lims(rng, rep == 0 ? 0 : 1 + (int64_t)(rng() % 60), tile_rows_for(T), 20000);
                check_plan(lims, T, scratch);
            }
    {   // the seam lengths of the GPU test, T = 128: all three forms, more than one pass, and a small budget cuts several groups
        const int64_t lens[] = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2047, 2048, 2049, 5000, 70001};
        std::vector<int64_t> lims(1, 0);
        for (int64_t n : lens) lims.push_back(lims.back() + n);
        Plan P;
        EXPECT(make_plan(lims.data(), 19, 128, 0, P).problem == OK);
        EXPECT(P.skipped == 2 && P.waves == 4 && P.tiles == 3 && P.longs == 10 && P.max_passes == 10 && P.groups.size() == 1);
        EXPECT(make_plan(lims.data(), 19, 128, 24 * 6000, P).problem == OK);
        EXPECT(P.groups.size() > 3 && P.groups.back().q1 - P.groups.back().q0 == 1 && P.groups.back().longest == 70001);
        EXPECT(make_plan(lims.data(), 19, 0, 0, P).problem == OK);
        EXPECT(P.waves == 10 && P.tiles == 6 && P.longs == 1 && P.max_passes == 4 && P.scratch_bytes == 8 * lims.back() + 16 * 70001);
    }
    for (int64_t T : {(int64_t)64, (int64_t)128, (int64_t)4096})
        for (int64_t n : {T + 1, 2 * T, 2 * T + 1, 3 * T - 1, 5 * T + 17, 8 * T, 13 * T + T / 2, 37 * T + 3}) check_merge(rng, n, T);
    {
        Plan P;
        const int64_t down[] = {0, 5, 3};
        Verdict v = make_plan(down, 2, 0, 0, P);
        EXPECT(v.problem == BAD_LIMS && v.q == 1 && v.value == -2);
        const int64_t huge[] = {0, 7, 7 + (1ll << 32)}, most[] = {0, (1ll << 32) - 1};
        v = make_plan(huge, 2, 0, 0, P);
        EXPECT(v.problem == SEGMENT_TOO_LONG && v.q == 1 && v.value == (1ll << 32));
        EXPECT(make_plan(most, 1, 0, 0, P).problem == OK && P.longs == 1 && P.groups.size() == 1);   // alone, above the budget
        const int64_t none[] = {0};
        EXPECT(make_plan(none, 0, 0, 0, P).problem == OK && P.groups.empty() && P.total == 0 && P.skipped == 0);
        const int64_t ones[] = {0, 1, 1, 2, 3};
        EXPECT(make_plan(ones, 4, 0, 0, P).problem == OK && P.groups.empty() && P.skipped == 4 && P.total == 3);
    }
    std::printf("range sort plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
