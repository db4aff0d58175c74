// lmi_union_plan.h -- the geometry of one union scan (lmi_scan_union and the two search forms): how the batch is cut into query
// groups, a group's (bucket, slots) work into waves that share one score slab, the device bytes the call allocates for that, and
// (build_tables) every table a group's kernels are launched from, and (build_groups) the tables of all groups with the extents the
// call's buffers are sized by.
// Host only and pure: the standard library, no HIP call, no kernel header -- lmi_host_candidates.h passes the sizes, the free memory,
// the forced values, the bucket order and the layout in, uploads what comes back and launches from it, for the union scan and the range
// search alike; tests/host/union_plan_selftest.cpp checks all of it on the CPU.
//
// A slot is one (query, rank) whose bucket has rows.  A slot is scored against its whole bucket in one piece and owns one sorted list,
// so nothing here can change a result (include/lmi_hip.h, lmi_scan_union); the geometry decides memory and speed only -- but the
// tables are addresses the kernels trust.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lmi_filter_plan.h"

// ---- the launch records.  They stay in namespace lmi, beside the kernels that take them (lmi_union.h): a kernel's symbol carries the
// namespace of its parameter types. ----
namespace lmi {

// one block of union_score_kernel
struct UnionItem {
    long long pos0;   // slab position (row of the row-major image) of the bucket's row 0
    int n;            // rows of the bucket (> 0: no item is emitted for an empty bucket -- the kernel's row clamp needs n - 1 >= 0)
    int blk;          // which 256 rows of it
    int tile0;        // first query tile (of the wave's packed queries)
    int ntiles;       // 1 .. CT
};
// one block of union_select_kernel
struct UnionSlot {
    long long s_off;  // the slot's row of the slab (floats)
    long long list;   // its list (entries)
    int n;            // scores in the row = rows of the bucket
    unsigned base;    // ordinal of the bucket's row 0 for this query
};
static_assert(sizeof(UnionItem) == 24 && sizeof(UnionSlot) == 24, "the kernels read these records as the host lays them out");

}  // namespace lmi

namespace lmi_union_plan {

using lmi::UnionItem;
using lmi::UnionSlot;

constexpr int MAX_K = 1024;          // LMI_UNION_MAX_K (lmi_host_union.h asserts that they agree)
constexpr int MIN_LIST = 128;        // a slot's sorted list holds max(MIN_LIST, k rounded up to a power of two) entries
constexpr int64_t AUTO_SLAB_BYTES = 2048ll << 20;   // the score slab of one wave, at most
constexpr int64_t AUTO_LIST_BYTES = 1024ll << 20;   // the lists of one query group, at most
constexpr int64_t AUTO_FRAG_BYTES = 256ll << 20;    // the packed queries of one wave, at most
constexpr int64_t MIN_SLAB_BYTES = 4096;

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t rup(int64_t a, int64_t b) { return cdiv(a, b) * b; }

struct Forced { int64_t query_rows = 0; int64_t slab_bytes = 0; };   // 0: chosen here

struct Plan {
    int64_t nq = 0;
    int nb = 0, k = 0, d = 0;
    int list_rows = 0;         // entries of a slot's sorted list (a power of two >= max(k, MIN_LIST))
    int lists_per_query = 0;   // = nb: one list per (query, rank)
    int kg = 0;                // groups of 8 links of a chain: the stored width, padded to a multiple of 32
    int64_t query_rows = 0, query_groups = 0;
    int64_t slab_bytes = 0;    // the budget of a wave's score slab (one chunk of 32 slots is taken even where it alone is larger)
    int64_t max_tiles = 0;     // 32-query tiles of packed queries per wave, at most
    int64_t list_bytes = 0, frag_bytes = 0, table_bytes = 0, out_bytes = 0;
    int64_t workspace_bytes = 0;   // an upper bound: what the call allocates when every wave fills its budget
};

inline int list_rows_for(int k) {
    int p = MIN_LIST;
    while (p < k) p <<= 1;
    return p;
}

inline void size_buffers(Plan& p, bool on_device) {
    p.list_bytes = p.query_rows * p.nb * (int64_t)p.list_rows * 8;
    p.max_tiles = std::max<int64_t>(1, AUTO_FRAG_BYTES / ((int64_t)p.kg * 1024));
    // no wave packs more tiles than the group has slots and buckets to fill them with
    p.max_tiles = std::min(p.max_tiles, p.query_rows * p.nb);
    p.frag_bytes = p.max_tiles * p.kg * 1024;
    p.table_bytes = p.query_rows * p.nb * 48;   // per slot: the query of its fragment row, its slab row, its ordinal base, its list ..
    p.out_bytes = on_device ? 0 : p.query_rows * (8 * (int64_t)p.k + 4);
    p.workspace_bytes = p.slab_bytes + p.list_bytes + p.frag_bytes + p.table_bytes + p.out_bytes;
}

// (nq >= 1, nb, k) as the call accepts them; d: the stored width.  free_bytes: the device's free memory, 0 = unknown.
inline Plan make_plan(int64_t nq, int nb, int k, int d, bool on_device, int64_t free_bytes, const Forced& f) {
    Plan p;
    p.nq = nq; p.nb = nb; p.k = k; p.d = d;
    p.list_rows = list_rows_for(k);
    p.lists_per_query = nb;
    p.kg = (int)(rup(d, 32) / 8);
    const int64_t per_query = (int64_t)nb * p.list_rows * 8;
    if (f.query_rows > 0) p.query_rows = std::min(f.query_rows, nq);
    else p.query_rows = std::min(nq, std::max<int64_t>(32, AUTO_LIST_BYTES / per_query / 32 * 32));
    p.slab_bytes = f.slab_bytes > 0 ? std::max(f.slab_bytes, MIN_SLAB_BYTES) : AUTO_SLAB_BYTES;
    size_buffers(p, on_device);
    // automatic values give way to the memory there is: a smaller slab first, then smaller groups
    const int64_t budget = free_bytes > 0 ? free_bytes / 10 * 8 : INT64_MAX;
    while (p.workspace_bytes > budget) {
        if (f.slab_bytes <= 0 && p.slab_bytes > (64ll << 20)) p.slab_bytes /= 2;
        else if (f.query_rows <= 0 && p.query_rows > 32) p.query_rows = std::max<int64_t>(32, p.query_rows / 2 / 32 * 32);
        else break;   // the allocation will say what it wanted
        size_buffers(p, on_device);
    }
    p.query_groups = cdiv(nq, p.query_rows);
    return p;
}

inline void group_range(const Plan& p, int64_t g, int64_t* q0, int64_t* q1) {
    *q0 = g * p.query_rows;
    *q1 = std::min(p.nq, *q0 + p.query_rows);
}

// the floats between two slots' rows of the slab, for a bucket of n rows
inline int64_t slab_pitch(int64_t n) { return rup(n, 64); }

// A chunk: slots [slot0, slot0 + slots) of one bucket's slot list, scored in one wave.  Its queries take cdiv(slots, 32) tiles from
// tile0 on (of the wave's packed queries); slot i's scores lie at slab_off + i * slab_pitch(n) (floats, of the wave's slab).
struct Chunk { int bucket; int64_t n; int64_t slot0, slots; int64_t tile0; int64_t slab_off; int wave; };

// Cuts a group's work into waves.  rows[b]: the bucket's rows, slots[b]: how many of the group's slots visit it.  A bucket without rows
// or without slots gives no chunk.  Buckets are taken in ascending order, a bucket's slots in order, whole tiles of 32 slots at a
// time; a wave closes when the next tile would take its slab past p.slab_bytes or its tiles past p.max_tiles -- but never empty.
inline std::vector<Chunk> cut_waves(const Plan& p, const std::vector<int64_t>& rows, const std::vector<int64_t>& slots, int* n_waves) {
    std::vector<Chunk> out;
    int wave = 0;
    int64_t used = 0, tiles = 0;   // of the open wave: slab bytes, tiles
    for (size_t b = 0; b < rows.size(); ++b) {
        if (rows[b] <= 0 || slots[b] <= 0) continue;
        const int64_t row_bytes = slab_pitch(rows[b]) * 4;
        int64_t s = 0;
        while (s < slots[b]) {
            // whole tiles that still fit (the last tile of a bucket may hold fewer than 32 slots)
            int64_t fit_tiles = std::min((p.slab_bytes - used) / (32 * row_bytes), p.max_tiles - tiles);
            if (fit_tiles <= 0) {
                if (tiles > 0) { ++wave; used = 0; tiles = 0; continue; }
                fit_tiles = 1;   // an empty wave takes one tile whatever it costs
            }
            const int64_t take = std::min(slots[b] - s, fit_tiles * 32);
            out.push_back({(int)b, rows[b], s, take, tiles, used / 4, wave});
            used += take * row_bytes;
            tiles += cdiv(take, 32);
            s += take;
        }
    }
    *n_waves = out.empty() ? 0 : wave + 1;
    return out;
}

constexpr int ITEM_ROWS = 256;   // rows of a bucket per item: KNN_ROWS (lmi_host_union.h asserts that they agree)

// A wave of a group: its ranges of the group's item, slot and tile tables, the floats of the slab it writes, and the query tiles an
// item spans (the CT of union_score_kernel).
struct Wave { int64_t item0 = 0, items = 0, slot0 = 0, slots = 0, tile0 = 0, tiles = 0, slab_floats = 0; int ct = 1; };

// Everything the kernels of query group [q0, q1) are launched from.  With gq = q1 - q0:
//   slot_n, slot_base, slot_pos0 [gq][nb]   per (query, rank), for the finish: rows to merge (0: none), ordinal of the bucket's row 0,
//                                           slab position of the bucket's row 0;
//   slots, slot_mask, scan_q, scan_pos0     one per scanned slot, wave after wave, inside a wave by (bucket, query, rank);
//                                           slot_mask[i]: the word offset of slot i's mask row, -1 for an unfiltered query (empty
//                                           without a filter); scan_q[i]: the GLOBAL query of slot i; scan_pos0[i]: the slab position
//                                           of its bucket's row 0 (the range kernels read these two);
//   rowq, tile_off, tile_cnt                per 32-query tile of a wave's packed queries: rowq [tiles][32] the global query of each
//                                           fragment row (-1: padding), the tile's first slab row (floats), its real slots;
//   items                                   wave after wave; inside a wave by chunk, tile group, 256-row block (blocks of one bucket
//                                           and tile group run back to back: that order is speed);
//   skipped                                 the slots a filter left out.
struct Tables {
    int64_t q0 = 0, q1 = 0;
    std::vector<Wave> waves;
    std::vector<UnionItem> items;
    std::vector<UnionSlot> slots;
    std::vector<int> rowq, tile_cnt, slot_n, scan_q;
    std::vector<long long> tile_off, slot_pos0, slot_mask, scan_pos0;
    std::vector<unsigned> slot_base;
    int64_t skipped = 0;
};

// the live layout: rows and first 32-row block of each of the L buckets
struct Layout { int L; const int* nb_rows; const int* rb_start; };
// a filter set as the tables need it: counts [nf][L] allowed rows; filter_of [nq] (nullptr: every query uses filter 0; -1: unfiltered);
// n_rb_total: the words of one filter's mask row
struct FilterView { const int32_t* counts; const int32_t* filter_of; int64_t n_rb_total; };

// The tables of query group `group` of plan p.  order [p.nq][p.nb]: the buckets each query visits, by rank; fv: nullptr without a filter.
// The rules:
//   - a bucket id outside [0, L) or an empty bucket is no slot and advances no ordinal;
//   - a slot whose (filter, bucket) pair allows no row gets slot_n = 0 and no UnionSlot -- it is not packed, scored or selected -- but
//     still advances slot_base by the bucket's rows: ordinals stay the unfiltered concatenation's, the finish skips the rank, and no
//     entry carries an ordinal of the gap;
//   - a query that lists a bucket twice gets two slots;
//   - a wave's ct is 1, 2 or 4, from the widest chunk of the wave (a chunk of 3 or more tiles takes 4).
inline Tables build_tables(const Plan& p, int64_t group, const int* order, const Layout& lay, const FilterView* fv) {
    Tables T;
    group_range(p, group, &T.q0, &T.q1);
    const int nb = p.nb, L = lay.L;
    const int64_t gq = T.q1 - T.q0;
    const int* ord = order + T.q0 * nb;   // the group's rows of order: slot s = q * nb + t visits ord[s]
    auto filter_of_slot = [&](int64_t s) -> int { return fv ? (fv->filter_of ? fv->filter_of[T.q0 + s / nb] : 0) : -1; };
    T.slot_n.assign((size_t)(gq * nb), 0);
    T.slot_base.assign((size_t)(gq * nb), 0u);
    T.slot_pos0.assign((size_t)(gq * nb), 0);
    std::vector<int64_t> rows(lay.nb_rows, lay.nb_rows + L), cnt((size_t)L, 0);
    for (int64_t q = 0; q < gq; ++q) {
        int64_t base = 0;
        const int fj = filter_of_slot(q * nb);
        for (int t = 0; t < nb; ++t) {
            const int64_t s = q * nb + t;
            const int b = ord[s];
            const int n = b >= 0 && b < L ? lay.nb_rows[b] : 0;
            const bool dead = fj >= 0 && n > 0 && fv->counts[(size_t)fj * L + b] == 0;   // the filter allows no row of the bucket
            T.slot_base[s] = (unsigned)base;
            T.slot_n[s] = dead ? 0 : n;
            if (n > 0) base += n;
            if (dead) ++T.skipped;
            else if (n > 0) { T.slot_pos0[s] = (long long)lay.rb_start[b] * 32; cnt[b]++; }
        }
    }
    // a bucket's slots in (query, rank) order
    std::vector<int64_t> start((size_t)L + 1, 0);
    for (int b = 0; b < L; ++b) start[b + 1] = start[b] + cnt[b];
    std::vector<int64_t> by_bucket((size_t)start[L]), fill(start.begin(), start.end() - 1);
    for (int64_t s = 0; s < gq * nb; ++s)
        if (T.slot_n[s] > 0) by_bucket[fill[ord[s]]++] = s;
    int n_waves = 0;
    const std::vector<Chunk> chunks = cut_waves(p, rows, cnt, &n_waves);
    T.waves.assign((size_t)n_waves, Wave{});
    // cut_waves gives a wave's chunks back to back; a chunk's tile0 and slab_off count from its wave's start
    for (size_t c0 = 0, c1 = 0; c0 < chunks.size(); c0 = c1) {
        Wave& W = T.waves[chunks[c0].wave];
        for (c1 = c0; c1 < chunks.size() && chunks[c1].wave == chunks[c0].wave; ++c1) {
            const int64_t tiles = cdiv(chunks[c1].slots, 32);
            W.ct = std::max(W.ct, tiles >= 3 ? 4 : (int)tiles);
        }
        W.item0 = (int64_t)T.items.size();
        W.slot0 = (int64_t)T.slots.size();
        W.tile0 = (int64_t)T.tile_cnt.size();
        for (size_t ci = c0; ci < c1; ++ci) {
            const Chunk& c = chunks[ci];
            const int64_t tiles = cdiv(c.slots, 32), pitch = slab_pitch(c.n), blocks = cdiv(c.n, ITEM_ROWS);
            const long long pos0 = (long long)lay.rb_start[c.bucket] * 32;
            W.tiles += tiles;
            W.slots += c.slots;
            W.slab_floats = std::max(W.slab_floats, c.slab_off + c.slots * pitch);
            for (int64_t i = 0; i < tiles * 32; ++i) {
                if (i >= c.slots) { T.rowq.push_back(-1); continue; }
                const int64_t s = by_bucket[start[c.bucket] + c.slot0 + i];
                T.rowq.push_back((int)(T.q0 + s / nb));
                T.slots.push_back(UnionSlot{c.slab_off + i * pitch, s * p.list_rows, (int)c.n, T.slot_base[s]});
                T.scan_q.push_back(T.rowq.back());
                T.scan_pos0.push_back(pos0);
                if (fv) {
                    const int fj = filter_of_slot(s);
                    T.slot_mask.push_back(fj < 0 ? -1ll : (long long)lmi_filter_plan::mask_word(fj, fv->n_rb_total, lay.rb_start[c.bucket], 0));
                }
            }
            for (int64_t t = 0; t < tiles; ++t) {
                T.tile_off.push_back(c.slab_off + t * 32 * pitch);
                T.tile_cnt.push_back((int)std::min<int64_t>(32, c.slots - t * 32));
            }
            for (int64_t t0 = 0; t0 < tiles; t0 += W.ct)
                for (int64_t blk = 0; blk < blocks; ++blk)
                    T.items.push_back(UnionItem{pos0, (int)c.n, (int)blk, (int)(c.tile0 + t0), (int)std::min<int64_t>(W.ct, tiles - t0)});
        }
        W.items = (int64_t)T.items.size() - W.item0;
    }
    return T;
}

// What a call's device buffers are sized by: the largest wave (its slab in bytes, its tiles), the largest group (its tiles, items and
// scanned slots) and, over all groups, the slots the filters left out.
struct Extents { int64_t slab_bytes = 0, wave_tiles = 0, group_tiles = 0, group_items = 0, group_slots = 0, skipped = 0; };
struct Groups { std::vector<Tables> groups; Extents ext; };

// The tables of every query group of plan p, in order, and their extents.
inline Groups build_groups(const Plan& p, const int* order, const Layout& lay, const FilterView* fv) {
    Groups R;
    R.groups.reserve((size_t)p.query_groups);
    Extents& e = R.ext;
    for (int64_t g = 0; g < p.query_groups; ++g) {
        R.groups.push_back(build_tables(p, g, order, lay, fv));
        const Tables& T = R.groups.back();
        for (const Wave& W : T.waves) {
            e.slab_bytes = std::max(e.slab_bytes, W.slab_floats * 4);
            e.wave_tiles = std::max(e.wave_tiles, W.tiles);
        }
        e.group_tiles = std::max(e.group_tiles, (int64_t)T.tile_cnt.size());
        e.group_items = std::max(e.group_items, (int64_t)T.items.size());
        e.group_slots = std::max(e.group_slots, (int64_t)T.slots.size());
        e.skipped += T.skipped;
    }
    return R;
}

}  // namespace lmi_union_plan
