// union_plan_selftest.cpp -- stand-alone check of the union scan's geometry (csrc/lmi_union_plan.h: pure host code) on the CPU, meant
// for -fsanitize=address,undefined (tests/test_union_host.py builds and runs it).  For a grid of (nq, nb, k, d, pointers, forced values,
// free memory) and several bucket / slot-count profiles: budgets are respected (a wave goes past its slab budget only as one lone tile
// of 32 slots), forced values are honoured, the query groups tile [0, nq), and the waves' chunks cover every slot of every bucket
// exactly once, with slab rows and query tiles that do not overlap inside a wave.  check_tables: for small explicit layouts, bucket
// orders and filter tables, what build_tables hands the kernels -- every live (query, rank) owns exactly one slot with the right list,
// rows and ordinal base, a wave's slab rows are disjoint and inside its slab, fragment rows, tile tables and slots agree, the items
// cover every (tile, 256-row block) exactly once, and the mask offsets are the filter's -- derived here from the inputs alone.
// check_groups: on the same grid, build_groups is build_tables group by group, and its extents are the brute-force maxima.
#include "lmi_union_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>

using namespace lmi_union_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static void check_plan(int64_t nq, int nb, int k, int d, bool dev, int64_t free_bytes, const Forced& f, Plan* out) {
    const Plan p = make_plan(nq, nb, k, d, dev, free_bytes, f);
    EXPECT(p.list_rows >= k && p.list_rows >= MIN_LIST && (p.list_rows & (p.list_rows - 1)) == 0 && p.list_rows <= 1024);
    EXPECT(p.lists_per_query == nb);
    EXPECT(p.kg % 4 == 0 && p.kg * 8 >= d && p.kg * 8 < d + 32);
    EXPECT(p.query_rows >= 1 && p.query_rows <= nq && p.slab_bytes >= MIN_SLAB_BYTES && p.max_tiles >= 1);
    if (f.query_rows > 0) EXPECT(p.query_rows == std::min(f.query_rows, nq));
    else EXPECT(p.query_rows == nq || (p.query_rows % 32 == 0 && p.list_bytes <= std::max<int64_t>(AUTO_LIST_BYTES, 32 * (int64_t)nb * p.list_rows * 8)));
    if (f.slab_bytes > 0) EXPECT(p.slab_bytes == std::max(f.slab_bytes, MIN_SLAB_BYTES));
    else EXPECT(p.slab_bytes <= AUTO_SLAB_BYTES);
    EXPECT(p.list_bytes == p.query_rows * nb * (int64_t)p.list_rows * 8);
    EXPECT(p.frag_bytes == p.max_tiles * p.kg * 1024 && p.frag_bytes <= std::max<int64_t>(AUTO_FRAG_BYTES, (int64_t)p.kg * 1024));
    EXPECT(p.out_bytes == (dev ? 0 : p.query_rows * (8 * (int64_t)k + 4)));
    EXPECT(p.workspace_bytes == p.slab_bytes + p.list_bytes + p.frag_bytes + p.table_bytes + p.out_bytes && p.workspace_bytes > 0);
    if (free_bytes > 0 && f.query_rows == 0 && f.slab_bytes == 0 && p.workspace_bytes > free_bytes / 10 * 8)
        EXPECT(p.slab_bytes <= (64ll << 20) && p.query_rows <= 32);   // it gave way as far as it goes
    // query groups tile [0, nq)
    EXPECT(p.query_groups >= 1);
    int64_t qat = 0;
    const int64_t qstep = p.query_groups > 64 ? p.query_groups / 7 : 1;
    for (int64_t g = 0; g < p.query_groups; g += (g + qstep < p.query_groups || g == p.query_groups - 1 ? qstep : p.query_groups - 1 - g)) {
        int64_t q0, q1;
        group_range(p, g, &q0, &q1);
        EXPECT(q0 == g * p.query_rows && q0 < q1 && q1 <= nq);
        if (qstep == 1) EXPECT(q0 == qat);
        if (g == p.query_groups - 1) EXPECT(q1 == nq);
        else EXPECT(q1 - q0 == p.query_rows);
        qat = q1;
    }
    EXPECT(qat == nq);
    *out = p;
}

static void check_waves(const Plan& p, const std::vector<int64_t>& rows, const std::vector<int64_t>& slots) {
    int n_waves = -1;
    const std::vector<Chunk> ch = cut_waves(p, rows, slots, &n_waves);
    std::vector<int64_t> next(rows.size(), 0);   // per bucket: the next slot a chunk must start at
    int wave = 0;
    int64_t slab_at = 0, tile_at = 0, chunks_in_wave = 0;
    for (const Chunk& c : ch) {
        EXPECT(c.bucket >= 0 && (size_t)c.bucket < rows.size());
        EXPECT(c.n == rows[c.bucket] && c.n > 0 && c.slots > 0);   // no chunk for an empty bucket or for no slots
        EXPECT(c.slot0 == next[c.bucket]);                        // a bucket's slots in order, each exactly once
        next[c.bucket] += c.slots;
        EXPECT(c.wave == wave || c.wave == wave + 1);
        if (c.wave != wave) { wave = c.wave; slab_at = 0; tile_at = 0; chunks_in_wave = 0; }
        // slab rows and tiles of a wave follow each other without overlap
        EXPECT(c.slab_off == slab_at && c.tile0 == tile_at && c.slab_off % 64 == 0);
        slab_at += c.slots * slab_pitch(c.n);
        tile_at += cdiv(c.slots, 32);
        ++chunks_in_wave;
        // the budgets: only a wave's first chunk, cut down to one tile, may go past the slab budget
        const bool lone_tile = chunks_in_wave == 1 && c.slots <= 32;
        EXPECT(slab_at * 4 <= p.slab_bytes || lone_tile);
        EXPECT(tile_at <= p.max_tiles);
        // whole tiles except at a bucket's end
        EXPECT(c.slots % 32 == 0 || c.slot0 + c.slots == slots[c.bucket]);
    }
    for (size_t b = 0; b < rows.size(); ++b) EXPECT(next[b] == (rows[b] > 0 && slots[b] > 0 ? slots[b] : 0));
    EXPECT(n_waves == (ch.empty() ? 0 : wave + 1));
}

// build_tables for every group of p, against properties worked out from (order, layout, filter) alone
static void check_tables(const Plan& p, const std::vector<int>& order, const Layout& lay, const FilterView* fv) {
    const int nb = p.nb, L = lay.L, LR = p.list_rows;
    for (int64_t g = 0; g < p.query_groups; ++g) {
        const Tables T = build_tables(p, g, order.data(), lay, fv);
        int64_t q0, q1;
        group_range(p, g, &q0, &q1);
        EXPECT(T.q0 == q0 && T.q1 == q1);
        const int64_t gq = q1 - q0, ns = gq * nb;
        EXPECT((int64_t)T.slot_n.size() == ns && (int64_t)T.slot_base.size() == ns && (int64_t)T.slot_pos0.size() == ns);
        // per (query, rank): what it must be
        std::vector<int> want_n((size_t)ns, 0), bucket_of((size_t)ns, -1), filter_of_slot((size_t)ns, -1);
        int64_t want_slots = 0, want_skipped = 0;
        for (int64_t q = 0; q < gq; ++q) {
            const int fj = fv ? (fv->filter_of ? fv->filter_of[q0 + q] : 0) : -1;
            int64_t base = 0;
            for (int t = 0; t < nb; ++t) {
                const int64_t s = q * nb + t;
                const int b = order[(size_t)((q0 + q) * nb + t)];
                const bool live = b >= 0 && b < L && lay.nb_rows[b] > 0;
                const bool dead = live && fj >= 0 && fv->counts[(size_t)fj * L + b] == 0;
                EXPECT(T.slot_base[s] == (unsigned)base);   // earlier ranks' rows: dead ones included, absent and empty ones not
                if (live) base += lay.nb_rows[b];
                if (dead) ++want_skipped;
                if (live && !dead) {
                    want_n[s] = lay.nb_rows[b];
                    bucket_of[s] = b;
                    filter_of_slot[s] = fj;
                    ++want_slots;
                    EXPECT(T.slot_pos0[s] == (long long)lay.rb_start[b] * 32);
                }
                EXPECT(T.slot_n[s] == want_n[s]);
            }
        }
        EXPECT(T.skipped == want_skipped);
        // every live (q, t) owns exactly one UnionSlot, nothing else owns one
        EXPECT((int64_t)T.slots.size() == want_slots);
        EXPECT(T.slot_mask.size() == (fv ? T.slots.size() : 0));
        EXPECT(T.scan_q.size() == T.slots.size() && T.scan_pos0.size() == T.slots.size());
        std::vector<int> owned((size_t)ns, 0);
        for (size_t i = 0; i < T.slots.size(); ++i) {
            const UnionSlot& sl = T.slots[i];
            EXPECT(sl.list >= 0 && sl.list % LR == 0 && sl.list / LR < ns);
            const int64_t s = sl.list / LR;
            EXPECT(owned[s]++ == 0 && want_n[s] > 0 && sl.n == want_n[s] && sl.base == T.slot_base[s] && sl.s_off >= 0);
            EXPECT(T.scan_q[i] == (int)(q0 + s / nb) && T.scan_pos0[i] == (long long)lay.rb_start[bucket_of[s]] * 32);
            if (fv) {
                const int fj = filter_of_slot[s];
                EXPECT(T.slot_mask[i] == (fj < 0 ? -1 : (long long)lmi_filter_plan::mask_word(fj, fv->n_rb_total, lay.rb_start[bucket_of[s]], 0)));
            }
        }
        // the waves tile the group's arrays
        EXPECT(T.rowq.size() == T.tile_cnt.size() * 32 && T.tile_off.size() == T.tile_cnt.size());
        int64_t item_at = 0, slot_at = 0, tile_at = 0;
        for (const Wave& W : T.waves) {
            EXPECT(W.item0 == item_at && W.slot0 == slot_at && W.tile0 == tile_at);
            EXPECT(W.items > 0 && W.slots > 0 && W.tiles > 0 && W.slab_floats > 0 && (W.ct == 1 || W.ct == 2 || W.ct == 4));
            item_at += W.items; slot_at += W.slots; tile_at += W.tiles;
            EXPECT(item_at <= (int64_t)T.items.size() && slot_at <= (int64_t)T.slots.size() && tile_at <= (int64_t)T.tile_cnt.size());
            // tile by tile: the wave's slots in order fill the tiles' real rows; slab row, fragment row and bucket agree
            std::vector<int> tile_bucket((size_t)W.tiles, -1);
            std::vector<std::pair<int64_t, int64_t>> ranges;
            std::map<int, int64_t> tiles_of_bucket;
            int64_t cur = W.slot0;
            for (int64_t t = 0; t < W.tiles; ++t) {
                const int64_t gt = W.tile0 + t;
                const int cnt = T.tile_cnt[gt];
                EXPECT(cnt >= 1 && cnt <= 32 && cur + cnt <= W.slot0 + W.slots);
                for (int j = 0; j < 32; ++j) {
                    if (j >= cnt) { EXPECT(T.rowq[gt * 32 + j] == -1); continue; }
                    const UnionSlot& sl = T.slots[cur++];
                    const int64_t s = sl.list / LR;
                    if (j == 0) tile_bucket[t] = bucket_of[s];
                    EXPECT(bucket_of[s] == tile_bucket[t]);
                    EXPECT(sl.s_off == T.tile_off[gt] + j * slab_pitch(sl.n));
                    EXPECT(T.rowq[gt * 32 + j] == (int)(q0 + s / nb));
                    EXPECT(sl.s_off + sl.n <= W.slab_floats);
                    ranges.push_back({sl.s_off, sl.s_off + sl.n});
                }
                ++tiles_of_bucket[tile_bucket[t]];
            }
            EXPECT(cur == W.slot0 + W.slots);
            std::sort(ranges.begin(), ranges.end());
            for (size_t i = 1; i < ranges.size(); ++i) EXPECT(ranges[i - 1].second <= ranges[i].first);
            int64_t widest = 0;
            for (const auto& kv : tiles_of_bucket) widest = std::max(widest, kv.second);
            EXPECT(W.ct == (widest >= 3 ? 4 : (int)widest));
            // the items: every (tile, 256-row block of the tile's bucket) exactly once
            std::map<std::pair<int64_t, int>, int> covered;
            for (int64_t i = W.item0; i < W.item0 + W.items; ++i) {
                const UnionItem& it = T.items[i];
                EXPECT(it.ntiles >= 1 && it.ntiles <= W.ct && it.tile0 >= 0 && it.tile0 + it.ntiles <= W.tiles);
                const int b = tile_bucket[it.tile0];
                EXPECT(it.pos0 == (long long)lay.rb_start[b] * 32 && it.n == lay.nb_rows[b] && it.blk >= 0 && (int64_t)it.blk * 256 < it.n);
                for (int t = it.tile0; t < it.tile0 + it.ntiles; ++t) {
                    EXPECT(tile_bucket[t] == b);   // one bucket per wave is one chunk: no item spans two
                    ++covered[{t, it.blk}];
                }
            }
            int64_t want_cover = 0;
            for (int64_t t = 0; t < W.tiles; ++t) want_cover += cdiv(lay.nb_rows[tile_bucket[t]], 256);
            EXPECT((int64_t)covered.size() == want_cover);
            for (const auto& kv : covered) EXPECT(kv.second == 1);
        }
        EXPECT(item_at == (int64_t)T.items.size() && slot_at == (int64_t)T.slots.size() && tile_at == (int64_t)T.tile_cnt.size());
    }
}

template <class V>
static bool same_bytes(const std::vector<V>& a, const std::vector<V>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}

// build_groups: the group list is build_tables called group by group, the extents are the maxima (skipped: the sum) over those tables
static void check_groups(const Plan& p, const std::vector<int>& order, const Layout& lay, const FilterView* fv) {
    const Groups R = build_groups(p, order.data(), lay, fv);
    EXPECT((int64_t)R.groups.size() == p.query_groups);
    Extents want;
    for (int64_t g = 0; g < p.query_groups; ++g) {
        const Tables T = build_tables(p, g, order.data(), lay, fv);
        const Tables& G = R.groups[(size_t)g];
        EXPECT(G.q0 == T.q0 && G.q1 == T.q1 && G.skipped == T.skipped);
        EXPECT(same_bytes(G.items, T.items) && same_bytes(G.slots, T.slots) && G.waves.size() == T.waves.size());   // (records without padding)
        for (size_t w = 0; w < T.waves.size(); ++w) {
            const Wave &a = G.waves[w], &b = T.waves[w];
            EXPECT(a.item0 == b.item0 && a.items == b.items && a.slot0 == b.slot0 && a.slots == b.slots && a.tile0 == b.tile0 &&
                   a.tiles == b.tiles && a.slab_floats == b.slab_floats && a.ct == b.ct);
        }
        EXPECT(G.rowq == T.rowq && G.tile_cnt == T.tile_cnt && G.tile_off == T.tile_off);
        EXPECT(G.slot_n == T.slot_n && G.slot_base == T.slot_base && G.slot_pos0 == T.slot_pos0 && G.slot_mask == T.slot_mask);
        EXPECT(G.scan_q == T.scan_q && G.scan_pos0 == T.scan_pos0);
        for (const Wave& W : T.waves) {
            want.slab_bytes = std::max(want.slab_bytes, W.slab_floats * 4);
            want.wave_tiles = std::max(want.wave_tiles, W.tiles);
        }
        want.group_tiles = std::max<int64_t>(want.group_tiles, (int64_t)T.tile_cnt.size());
        want.group_items = std::max<int64_t>(want.group_items, (int64_t)T.items.size());
        want.group_slots = std::max<int64_t>(want.group_slots, (int64_t)T.slots.size());
        want.skipped += T.skipped;
    }
    const Extents& e = R.ext;
    EXPECT(e.slab_bytes == want.slab_bytes && e.wave_tiles == want.wave_tiles && e.group_tiles == want.group_tiles);
    EXPECT(e.group_items == want.group_items && e.group_slots == want.group_slots && e.skipped == want.skipped);
    // every buffer sized by the extents holds every wave and group that is uploaded into it or written by it
    for (const Tables& G : R.groups) {
        EXPECT((int64_t)G.items.size() <= e.group_items && (int64_t)G.slots.size() <= e.group_slots && (int64_t)G.tile_cnt.size() <= e.group_tiles);
        EXPECT(G.slot_mask.size() <= (size_t)e.group_slots && G.rowq.size() <= (size_t)e.group_tiles * 32);
        for (const Wave& W : G.waves) EXPECT(W.slab_floats * 4 <= e.slab_bytes && W.tiles <= e.wave_tiles);
    }
}

// the grid of check_tables: two layouts x (nq, nb, k) x forced geometry x bucket orders x filters
static void check_tables_grid() {
    struct Lay { std::vector<int> rows, rbs; };
    Lay lays[2] = {{{0, 1, 33, 257, 2000, 640, 0, 5, 64, 65, 900, 1203}, {}}, {{40, 0, 700}, {}}};
    for (Lay& l : lays) {   // buckets start on 32-row blocks, with a gap in front of each
        int at = 3;
        for (int n : l.rows) { l.rbs.push_back(at); at += (int)cdiv(n, 32) + 2; }
        l.rbs.push_back(at);
    }
    const Forced forced[] = {{0, 0}, {32, 64 << 10}, {7, 4096}};
    uint32_t rng = 12345u;
    auto next = [&rng]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (const Lay& l : lays) {
        const int L = (int)l.rows.size();
        const Layout lay{L, l.rows.data(), l.rbs.data()};
        const int64_t n_rb_total = l.rbs.back();
        // three filters: 0 empties the buckets b % 3 == 1, 1 the even ones, 2 all of them
        std::vector<int32_t> counts((size_t)3 * L);
        for (int b = 0; b < L; ++b) {
            counts[0 * L + b] = b % 3 == 1 ? 0 : std::max(1, l.rows[b] / 2);
            counts[1 * L + b] = b % 2 == 0 ? 0 : l.rows[b];
            counts[2 * L + b] = 0;
        }
        for (int64_t nq : {1, 33, 150})
            for (int nb : {1, 3, 8})
                for (int k : {10, 129, 1024})
                    for (const Forced& f : forced) {
                        const Plan p = make_plan(nq, nb, k, 64, false, 0, f);
                        std::vector<int> mixed((size_t)nq * nb), twice((size_t)nq * nb), one((size_t)nq * nb, L - 1);
                        for (size_t i = 0; i < mixed.size(); ++i) {
                            const uint32_t r = next() % (uint32_t)(L + 3);   // -1, 0 .. L-1, L, L+1
                            mixed[i] = (int)r - 1;
                            twice[i] = i % (size_t)nb < 2 ? 2 % L : (int)(next() % (uint32_t)L);   // ranks 0 and 1 list the same bucket
                        }
                        std::vector<int32_t> mix((size_t)nq), all_dead((size_t)nq, 2);
                        for (int64_t q = 0; q < nq; ++q) mix[q] = (int32_t)(next() % 4u) - 1;
                        const FilterView views[] = {{counts.data(), nullptr, n_rb_total}, {counts.data(), mix.data(), n_rb_total},
                                                    {counts.data(), all_dead.data(), n_rb_total}};
                        for (const std::vector<int>* o : {&mixed, &twice, &one}) {
                            check_tables(p, *o, lay, nullptr);
                            check_groups(p, *o, lay, nullptr);
                            for (const FilterView& v : views) {
                                check_tables(p, *o, lay, &v);
                                check_groups(p, *o, lay, &v);
                            }
                        }
                    }
    }
}

int main() {
    const int64_t nqs[] = {1, 33, 150, 10000, ((int64_t)1 << 31) / 1024 - 1};
    const int nbs[] = {1, 3, 8, 120, 1024};
    const int ks[] = {1, 10, 100, 129, 1024};
    const int ds[] = {1, 45, 48, 136, 768, 4096};
    const Forced forced[] = {{0, 0}, {32, 0}, {0, 1}, {32, 64 << 10}, {7, 1 << 20}, {1 << 20, (int64_t)1 << 40}};
    const int64_t frees[] = {0, (int64_t)1 << 28, (int64_t)200 << 30};
    const std::vector<int64_t> rows_a = {0, 1, 33, 257, 2000, 640, 0, 5, 64, 65, 900, 1203};
    const std::vector<int64_t> rows_b(120, 83333);
    for (int64_t nq : nqs)
        for (int nb : nbs)
            for (int k : ks)
                for (int d : ds)
                    for (const Forced& f : forced)
                        for (int64_t fr : frees)
                            for (int dev = 0; dev < 2; ++dev) {
                                Plan p;
                                check_plan(nq, nb, k, d, dev, fr, f, &p);
                                if (nq > 10000 || d == 4096 || dev) continue;   // (the pointers' kind changes out_bytes only)
                                // slot profiles of one group: spread evenly, all on one bucket, none, one per bucket
                                const int64_t total = p.query_rows * nb;
                                for (const std::vector<int64_t>* rows : {&rows_a, &rows_b}) {
                                    const int64_t L = (int64_t)rows->size();
                                    std::vector<int64_t> even(L), one(L, 0), none(L, 0), each(L, 1);
                                    for (int64_t b = 0; b < L; ++b) even[b] = total / L + (b < total % L);
                                    one[4] = total;
                                    check_waves(p, *rows, even);
                                    check_waves(p, *rows, one);
                                    check_waves(p, *rows, none);
                                    check_waves(p, *rows, each);
                                }
                            }
    // the case the header's formula names: the benchmark's shape takes one group and a handful of waves
    {
        const Plan p = make_plan(10000, 4, 1000, 768, true, (int64_t)200 << 30, Forced{});
        EXPECT(p.query_groups == 1 && p.query_rows == 10000 && p.list_rows == 1024 && p.slab_bytes == AUTO_SLAB_BYTES);
        std::vector<int64_t> slots(120, 40000 / 120 + 1);
        int n_waves = 0;
        const std::vector<Chunk> ch = cut_waves(p, rows_b, slots, &n_waves);
        EXPECT(n_waves >= 6 && n_waves <= 8 && !ch.empty());
        // forced values give several groups and waves on the tests' small shape
        const Plan s = make_plan(150, 8, 100, 64, false, 0, Forced{32, 64 << 10});
        EXPECT(s.query_groups == 5 && s.query_rows == 32 && s.slab_bytes == (64 << 10));
    }
    check_tables_grid();
    std::printf("union plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
