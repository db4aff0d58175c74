// union_plan_selftest.cpp -- stand-alone check of the union scan's geometry (csrc/lmi_union_plan.h: pure host code) on the CPU, meant
// for -fsanitize=address,undefined (tests/test_union_host.py builds and runs it).  For a grid of (nq, nb, k, d, pointers, forced values,
// free memory) and several bucket / slot-count profiles: budgets are respected (a wave goes past its slab budget only as one lone tile
// of 32 slots), forced values are honoured, the query groups tile [0, nq), and the waves' chunks cover every slot of every bucket
// exactly once, with slab rows and query tiles that do not overlap inside a wave.
#include "lmi_union_plan.h"

#include <cstdio>
#include <cstdlib>

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
    std::printf("union plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
