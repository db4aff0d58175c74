// lmi_union_plan.h -- the geometry of one union scan (lmi_scan_union and the two search forms): how the batch is cut into query
// groups, a group's (bucket, slots) work into waves that share one score slab, and the device bytes the call allocates for that.
// Host only and pure: the standard library, no HIP call, no kernel header -- lmi_host_union.h passes the sizes, the free memory and
// the forced values in and acts on what comes back; tests/host/union_plan_selftest.cpp checks it on the CPU.
//
// A slot is one (query, rank) whose bucket has rows.  A slot is scored against its whole bucket in one piece and owns one sorted list,
// so nothing here can change a result (include/lmi_hip.h, lmi_scan_union); the geometry decides memory and speed only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace lmi_union_plan {

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

}  // namespace lmi_union_plan
