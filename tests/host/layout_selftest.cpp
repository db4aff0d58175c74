// layout_selftest.cpp -- the bucket layout's arithmetic (csrc/lmi_layout.h), checked on the CPU: the chunk length, a fresh build's
// layout, the derived tables, the four paths of an insert (slack, relocation, growth re-pack, hole re-pack) and its refusals, the
// staging groups of a delete.  Stand-alone: it includes lmi_layout.h and nothing else of the library.  Built with
// -fsanitize=address,undefined by tests/test_layout_host.py.
#include "lmi_layout.h"

#include <cstdio>
#include <cstdlib>

using namespace lmi_layout;
using IVec = std::vector<int>;
using AVec = std::vector<int64_t>;

#define REQUIRE(cond)                                                                          \
    do {                                                                                       \
        if (!(cond)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// ---- chunk_rows ----
static int picked(int64_t rows, int L, const AutoChunk& pick) {   // rows spread evenly over L buckets, the automatic pick
    IVec nb(L, (int)(rows / L)), nch;
    nb[0] += (int)(rows - rows / L * L);
    std::vector<unsigned char> any(L, 1);
    const Tables t = derive_tables(nb, any, 2048, &pick, nch);
    REQUIRE(t.owned_total == rows && t.n_nonempty == L);
    return t.chunk_rows;
}
static void chunk_rows_rule() {
    const AutoChunk wide = {768, false, true}, low = {48, true, true}, exact = {768, false, false};
    REQUIRE(picked(100000, 120, wide) == 256);
    REQUIRE(picked(10000000, 120, wide) == 2048);
    REQUIRE(picked(10000000, 256, low) == 4096);
    REQUIRE(picked(10000000, 120, exact) == 1024);
    REQUIRE(picked(3000000, 1, wide) == 3072);   // one bucket: 1024 chunks of the pick (768 rows) would not cover it
    // the pieces of the rule
    REQUIRE(auto_chunk_rows(0, 768, false, true) == TILE_ROWS && auto_chunk_rows(0, 48, true, true) == TILE_ROWS);
    REQUIRE(auto_chunk_rows(100000, 48, true, true) == 256 && auto_chunk_rows(2000000, 48, true, true) == 2048);
    REQUIRE(auto_chunk_rows(100000, 768, false, false) == 256);             // (the 3 MiB cap only lowers)
    REQUIRE(auto_chunk_rows(10000000, 100000, false, false) == TILE_ROWS);  // (and never below a tile)
    REQUIRE(floor_chunk_rows(256, 1024 * 256) == 256 && floor_chunk_rows(256, 1024 * 256 + 1) == 512);
    // a caller-set value is kept unless the floor exceeds it
    IVec nch;
    const std::vector<unsigned char> any2(2, 1);
    REQUIRE(derive_tables({100000, 5}, any2, 512, nullptr, nch).chunk_rows == 512);
    REQUIRE(derive_tables({3000000, 5}, any2, 512, nullptr, nch).chunk_rows == 3072);
    REQUIRE(nch[0] == (int)cdiv(cdiv(3000000, 32), 3072 / 32) && nch[0] <= MAX_CHUNKS && nch[1] == 1);
}

// ---- a fresh layout and the derived tables ----
static void fresh_and_derived() {
    const IVec nb = {0, 1, 31, 32, 33, 0, 1000};
    const std::vector<unsigned char> any = {0, 1, 1, 1, 1, 1, 1};   // bucket 5: another rank's (rows there, none stored here)
    IVec start, cap, nch;
    const Tables t = derive_tables(nb, any, 256, nullptr, nch);
    REQUIRE(t.owned_total == 1097 && t.n_nonempty == 6 && t.chunk_rows == 256);
    const int64_t total = fresh_layout(nb, start, cap);
    REQUIRE((start == IVec{0, 0, 1, 2, 3, 5, 5, 37}) && (cap == IVec{0, 1, 1, 1, 2, 0, 32}) && total == 37);
    REQUIRE((nch == IVec{0, 1, 1, 1, 1, 0, 4}));
    for (size_t b = 0; b < nb.size(); ++b) {
        REQUIRE(cap[b] == (int)cdiv(nb[b], 32) && start[b + 1] - start[b] == cap[b]);
        REQUIRE(nch[b] == (int)cdiv(cap[b], t.chunk_rows / 32));
    }
    // no rows anywhere: one bucket still counts (a scan's arithmetic divides by it); a stored row counts without `any`
    REQUIRE(derive_tables({0, 0}, {0, 0}, 256, nullptr, nch).n_nonempty == 1);
    REQUIRE(derive_tables({0, 7, 9}, {0, 0, 0}, 256, nullptr, nch).n_nonempty == 2);
    REQUIRE(fresh_layout({}, start, cap) == 0 && start == IVec{0} && cap.empty());
}

// ---- insert ----
struct Index { IVec nb, start, cap; int64_t total; };
static void check_accepted(const Index& x, const AVec& add, const InsertPlan& p, int64_t alloc, int64_t max_rb, const int64_t (&paths)[4]) {
    const int L = (int)x.nb.size();
    REQUIRE(p.refusal == InsertPlan::OK && p.bucket == -1);
    REQUIRE((int)p.start.size() == L && (int)p.cap.size() == L && (int)p.moved.size() == L);
    REQUIRE(p.total <= max_rb && p.total <= p.alloc_new && p.alloc_new <= std::max(alloc, max_rb));
    for (int b = 0; b < L; ++b) {
        REQUIRE((int64_t)p.cap[b] * 32 >= x.nb[b] + add[b] && p.cap[b] >= x.cap[b]);      // cap >= need, and a bucket never shrinks
        REQUIRE(p.start[b] >= 0 && (int64_t)p.start[b] + p.cap[b] <= p.total);             // inside the layout
        REQUIRE(p.moved[b] == (cdiv(x.nb[b] + add[b], 32) > x.cap[b]));
        if (!p.pack && !p.moved[b]) REQUIRE(p.start[b] == x.start[b] && p.cap[b] == x.cap[b]);
        if (!p.pack && p.moved[b]) REQUIRE(p.start[b] >= x.total);                        // behind the old tail: the old place is a hole
        for (int c = 0; c < b; ++c)                                                       // disjoint
            REQUIRE(p.start[c] + p.cap[c] <= p.start[b] || p.start[b] + p.cap[b] <= p.start[c] || !p.cap[b] || !p.cap[c]);
    }
    if (!p.pack) REQUIRE(p.alloc_new == alloc);
    for (int i = 0; i < 4; ++i) REQUIRE(p.paths[i] == paths[i]);
}
static InsertPlan plan(const Index& x, const AVec& add, int chunk_rb, int64_t alloc, int64_t max_rb) {
    IVec start = x.start;
    start.push_back((int)x.total);   // (the handle's table has L + 1 entries)
    return plan_insert(x.nb, start, x.cap, x.total, add, chunk_rb, alloc, max_rb);
}
static void insert_paths() {
    const int64_t lim = max_slab_rb(3);
    REQUIRE(max_slab_rb(1) == ((1ll << 31) - 64) / 32 - 1 && lim == ((1ll << 31) - 192) / 32 - 1);
    {   // slack: both buckets take their rows where they are, nothing moves
        const Index x = {{40, 10, 0}, {0, 4, 6}, {4, 2, 3}, 9};
        const AVec add = {20, 5, 0};
        const InsertPlan p = plan(x, add, 8, 20, lim);
        check_accepted(x, add, p, 20, lim, {2, 0, 0, 0});
        REQUIRE(!p.pack && p.start == x.start && p.cap == x.cap && p.total == 9 && p.alloc_new == 20 && (p.moved == std::vector<unsigned char>{0, 0, 0}));
    }
    {   // relocation: bucket 1 needs 3 row-blocks and has 1 -- cap = need + max(need / 4, chunk_rb) at the old tail; bucket 0 has slack
        const Index x = {{60, 32}, {0, 2}, {2, 1}, 3};
        const AVec add = {2, 40};
        const InsertPlan p = plan(x, add, 8, 100, lim);
        check_accepted(x, add, p, 100, lim, {1, 1, 0, 0});
        REQUIRE(!p.pack && (p.start == IVec{0, 3}) && (p.cap == IVec{2, 3 + 8}) && p.total == 14 && p.alloc_new == 100);
    }
    {   // relocation of a long bucket: the quarter is the larger slack (need 100 -> 125)
        const Index x = {{0}, {0}, {0}, 0};
        const AVec add = {3200};
        const InsertPlan p = plan(x, add, 8, 1000, lim);
        check_accepted(x, add, p, 1000, lim, {0, 1, 0, 0});
        REQUIRE(!p.pack && p.start[0] == 0 && p.cap[0] == 125 && p.total == 125);
    }
    {   // growth re-pack: the same relocation, but the tail (14) passes the allocations (10): packed starts, 1/8 headroom
        const Index x = {{60, 32}, {0, 2}, {2, 1}, 3};
        const AVec add = {2, 40};
        const InsertPlan p = plan(x, add, 8, 10, lim);
        check_accepted(x, add, p, 10, lim, {0, 0, 1, 0});
        REQUIRE(p.pack && (p.start == IVec{0, 2}) && (p.cap == IVec{2, 11}) && p.total == 13 && p.alloc_new == 13 + 13 / 8);
        const InsertPlan q = plan(x, add, 8, 10, 13);   // the headroom is capped at the position limit
        check_accepted(x, add, q, 10, 13, {0, 0, 1, 0});
        REQUIRE(q.pack && q.total == 13 && q.alloc_new == 13);
    }
    {   // hole re-pack: bucket 0 moves and leaves 10 of 30 row-blocks empty (more than a quarter) while everything fits the allocations
        const Index x = {{320, 32}, {0, 10}, {10, 1}, 11};
        const AVec add = {32, 0};
        const InsertPlan p = plan(x, add, 8, 100, lim);
        check_accepted(x, add, p, 100, lim, {0, 0, 0, 1});
        REQUIRE(p.pack && (p.start == IVec{0, 19}) && (p.cap == IVec{19, 1}) && p.total == 20 && p.alloc_new == 22);
        // one hole of exactly a quarter stays: 3 of 12 -> no re-pack
        const Index y = {{96, 32}, {0, 3}, {3, 1}, 4};
        const AVec addy = {1, 0};
        const InsertPlan q = plan(y, addy, 4, 100, lim);   // need 4 -> cap 8 at row-block 4: tail 12, holes 3
        check_accepted(y, addy, q, 100, lim, {0, 1, 0, 0});
        REQUIRE(!q.pack && (q.start == IVec{4, 3}) && (q.cap == IVec{8, 1}) && q.total == 12);
    }
    {   // refusals: one bucket past the 32-bit positions; every bucket inside them, the layout not
        const Index x = {{2000000000}, {0}, {62500000}, 62500000};
        const InsertPlan p = plan(x, {200000000}, 64, 70000000, max_slab_rb(1));
        REQUIRE(p.refusal == InsertPlan::BUCKET_PAST_LIMIT && p.bucket == 0);
        const Index y = {{0, 0}, {0, 0}, {0, 0}, 0};
        const InsertPlan q = plan(y, {512, 512}, 8, 0, 30);   // 24 row-blocks each
        REQUIRE(q.refusal == InsertPlan::TOTAL_PAST_LIMIT && q.total == 48 && q.bucket == -1);
        const InsertPlan r = plan(y, {512, 100000}, 8, 0, 30);
        REQUIRE(r.refusal == InsertPlan::BUCKET_PAST_LIMIT && r.bucket == 1);
    }
}

// ---- delete ----
static void check_groups(const IVec& span, int64_t budget, const DeleteGroups& g) {
    REQUIRE(g.goff.size() == span.size() && g.gfirst.front() == 0 && g.gfirst.back() == (int)span.size());
    int64_t longest = 0;
    for (int k = 0; k < g.n(); ++k) {
        REQUIRE(g.gfirst[k] < g.gfirst[k + 1]);   // in order, none empty
        int64_t acc = 0;
        for (int i = g.gfirst[k]; i < g.gfirst[k + 1]; ++i) { REQUIRE(g.goff[i] == acc); acc += span[i]; }   // the running sums
        REQUIRE(acc <= budget || g.gfirst[k + 1] - g.gfirst[k] == 1);
        if (k + 1 < g.n()) REQUIRE(acc + span[g.gfirst[k + 1]] > budget);   // a group ends only where the next bucket does not fit
        longest = std::max(longest, acc);
    }
    REQUIRE(g.stage_rows == longest);
}
static void delete_staging() {
    const IVec a = {64, 32, 96, 32, 32};
    const DeleteGroups g = delete_groups(a, 100);
    check_groups(a, 100, g);
    REQUIRE((g.gfirst == IVec{0, 2, 3, 5}) && (g.goff == std::vector<long long>{0, 64, 0, 0, 32}) && g.stage_rows == 96);
    const IVec b = {200, 32, 32};   // a bucket longer than the budget is a group of its own
    const DeleteGroups h = delete_groups(b, 100);
    check_groups(b, 100, h);
    REQUIRE((h.gfirst == IVec{0, 1, 3}) && h.stage_rows == 200);
    const DeleteGroups one = delete_groups(a, 1 << 20);   // everything fits: one group
    check_groups(a, 1 << 20, one);
    REQUIRE(one.n() == 1 && one.stage_rows == 256);
    REQUIRE(delete_groups({}, 100).n() == 0 && delete_groups({}, 100).stage_rows == 0);
}

int main() {
    chunk_rows_rule();
    fresh_and_derived();
    insert_paths();
    delete_staging();
    printf("layout selftest: clean\n");
    return 0;
}
