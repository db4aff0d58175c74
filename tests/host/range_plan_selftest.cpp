// range_plan_selftest.cpp -- stand-alone check of the range search's host arithmetic (csrc/lmi_range_plan.h: pure host code) on the
// CPU, meant for -fsanitize=address,undefined (tests/test_range_host.py builds and runs it).  For random layouts, bucket orders (holes,
// buckets listed twice, ids outside the index, empty buckets), filter tables with emptied (filter, bucket) pairs and forced geometries
// that give several groups and waves, with random per-slot counts:
//   - a slot's parallel arrays (the tables' scan_q and scan_pos0) name its query and its bucket's slab position;
//   - a wave's offsets tile its chunk exactly once, in slot order;
//   - lims starts at 0, is monotone and ends at the sum of all counts;
//   - the gathered runs tile [0, total) exactly once, every run inside its query's [lims[q], lims[q + 1]), a query's runs in rank order;
//   - a rank that is no slot (a hole, an empty bucket, one its filter emptied) and a slot that counted nothing own nothing;
//   - the max_total test passes at the exact total and fails one below it.
#include "lmi_range_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace lmi_range_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static void check_case(std::mt19937& rng, int64_t nq, int nb, int L, int nf, int64_t force_rows, int64_t force_slab, int fill) {
    auto rnd = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    std::vector<int> nrows((size_t)L), rbs((size_t)L + 1, 0);
    for (int b = 0; b < L; ++b) {
        const int kind = rnd(0, 5);
        nrows[(size_t)b] = kind == 0 ? 0 : kind == 1 ? rnd(1, 3) : kind == 2 ? 64 * rnd(1, 3) : rnd(1, 700);
        rbs[(size_t)b + 1] = rbs[(size_t)b] + (nrows[(size_t)b] + 31) / 32 + rnd(0, 2);   // spare row-blocks behind a bucket
    }
    std::vector<int> order((size_t)(nq * nb));
    for (int& o : order) o = rnd(0, 9) == 0 ? -1 : rnd(0, 19) == 0 ? L + rnd(0, 3) : rnd(0, L - 1);
    std::vector<int32_t> fcounts((size_t)(nf > 0 ? nf * L : 0)), filter_of((size_t)nq);
    for (int j = 0; j < nf; ++j)
        for (int b = 0; b < L; ++b) fcounts[(size_t)j * L + b] = rnd(0, 2) == 0 ? 0 : rnd(0, nrows[(size_t)b]);
    for (int32_t& v : filter_of) v = nf > 0 ? rnd(-1, nf - 1) : -1;
    const up::Layout lay{L, nrows.data(), rbs.data()};
    const up::FilterView fv{fcounts.data(), filter_of.data(), rbs[(size_t)L]};
    up::Forced forced;
    forced.query_rows = force_rows;
    forced.slab_bytes = force_slab;
    const up::Plan p = up::make_plan(nq, nb, PLAN_K, 40, true, 0, forced);

    Totals tot(nq, nb);
    struct WaveOut { std::vector<int> counts; std::vector<long long> off; int64_t total; };
    const up::Groups all = up::build_groups(p, order.data(), lay, nf > 0 ? &fv : nullptr);
    const std::vector<up::Tables>& groups = all.groups;
    std::vector<std::vector<WaveOut>> outs;
    int64_t counted = 0;
    std::vector<char> is_slot((size_t)(nq * nb), 0);
    EXPECT((int64_t)groups.size() == p.query_groups);
    for (const up::Tables& T : groups) {
        EXPECT(T.scan_q.size() == T.slots.size() && T.scan_pos0.size() == T.slots.size());
        for (size_t i = 0; i < T.slots.size(); ++i) {
            const int64_t s = slot_pair(p, T, (int64_t)i);
            EXPECT(s >= 0 && s < (T.q1 - T.q0) * nb);
            const int64_t q = T.q0 + s / nb, t = s % nb;
            const int b = order[(size_t)(q * nb + t)];
            EXPECT(T.scan_q[i] == q && b >= 0 && b < L && T.slots[i].n == nrows[(size_t)b] && T.slots[i].n > 0);
            EXPECT(T.scan_pos0[i] == (long long)rbs[(size_t)b] * 32);
            EXPECT(!is_slot[(size_t)(q * nb + t)]);   // every (query, rank) owns at most one slot
            is_slot[(size_t)(q * nb + t)] = 1;
            if (nf > 0 && filter_of[(size_t)q] >= 0) EXPECT(fcounts[(size_t)filter_of[(size_t)q] * L + b] > 0);
        }
        outs.emplace_back();
        int64_t slots_seen = 0;
        for (const up::Wave& W : T.waves) {
            WaveOut O;
            O.counts.resize((size_t)W.slots);
            O.off.resize((size_t)W.slots);
            for (int64_t i = 0; i < W.slots; ++i) {
                const int n = T.slots[(size_t)(W.slot0 + i)].n;
                O.counts[(size_t)i] = fill == 0 ? 0 : fill == 2 ? n : rnd(0, 3) == 0 ? 0 : rnd(0, n);
            }
            O.total = chunk_offsets(O.counts.data(), W.slots, O.off.data());
            int64_t at = 0;   // the offsets tile the chunk in slot order
            for (int64_t i = 0; i < W.slots; ++i) {
                EXPECT(O.off[(size_t)i] == at);
                at += O.counts[(size_t)i];
            }
            EXPECT(at == O.total);
            const int64_t sum = add_wave(tot, p, T, W, O.counts.data());
            EXPECT(sum == O.total);
            counted += sum;
            slots_seen += W.slots;
            outs.back().push_back(std::move(O));
        }
        EXPECT(slots_seen == (int64_t)T.slots.size());
    }
    EXPECT(!over_total(counted, 0) && !over_total(counted, counted));
    if (counted > 1) EXPECT(over_total(counted, counted - 1));   // (max_total 0 means no limit: one below a total of 1 cannot be asked for)

    const std::vector<int64_t> first = run_starts(tot);
    const std::vector<int64_t> lims = make_lims(tot, first);
    EXPECT((int64_t)lims.size() == nq + 1 && lims[0] == 0 && lims[(size_t)nq] == counted);
    for (int64_t q = 0; q < nq; ++q) EXPECT(lims[(size_t)q] <= lims[(size_t)q + 1]);
    for (int64_t s = 0; s < nq * nb; ++s)
        if (!is_slot[(size_t)s]) EXPECT(tot.pair_count[(size_t)s] == 0);   // no slot: nothing

    // the runs tile [0, total) exactly once
    std::vector<char> owned((size_t)counted, 0);
    std::vector<int64_t> run_of_pair((size_t)(nq * nb), -1);
    for (size_t g = 0; g < groups.size(); ++g)
        for (size_t w = 0; w < groups[g].waves.size(); ++w) {
            const up::Wave& W = groups[g].waves[w];
            const WaveOut& O = outs[g][w];
            const Gather G = gather_of(p, groups[g], W, O.counts.data(), O.off.data(), first);
            EXPECT((int64_t)G.src.size() == W.slots && (int64_t)G.dst.size() == W.slots && (int64_t)G.n.size() == W.slots);
            for (int64_t i = 0; i < W.slots; ++i) {
                const int64_t s = groups[g].q0 * nb + slot_pair(p, groups[g], W.slot0 + i);
                const int64_t q = s / nb;
                EXPECT(G.n[(size_t)i] == O.counts[(size_t)i] && G.src[(size_t)i] == O.off[(size_t)i]);
                EXPECT(G.src[(size_t)i] >= 0 && G.src[(size_t)i] + G.n[(size_t)i] <= O.total);
                EXPECT(G.dst[(size_t)i] >= lims[(size_t)q] && G.dst[(size_t)i] + G.n[(size_t)i] <= lims[(size_t)q + 1]);
                for (int64_t j = 0; j < G.n[(size_t)i]; ++j) {
                    EXPECT(!owned[(size_t)(G.dst[(size_t)i] + j)]);
                    owned[(size_t)(G.dst[(size_t)i] + j)] = 1;
                }
                run_of_pair[(size_t)s] = G.dst[(size_t)i];
            }
        }
    for (char c : owned) EXPECT(c == 1);
    // a query's runs in rank order, back to back
    for (int64_t q = 0; q < nq; ++q) {
        int64_t at = lims[(size_t)q];
        for (int t = 0; t < nb; ++t) {
            const int64_t s = q * nb + t;
            if (run_of_pair[(size_t)s] < 0) continue;
            EXPECT(run_of_pair[(size_t)s] == at);
            at += tot.pair_count[(size_t)s];
        }
        EXPECT(at == lims[(size_t)q + 1]);
    }
}

int main() {
    std::mt19937 rng(20240611u);
    int c[2] = {5, 0};
    long long o[2] = {-1, -1};
    EXPECT(chunk_offsets(c, 2, o) == 5 && o[0] == 0 && o[1] == 5);
    EXPECT(chunk_offsets(nullptr, 0, nullptr) == 0);
    EXPECT(!over_total(1ll << 40, 0) && over_total(11, 10) && !over_total(10, 10));
    for (int fill = 0; fill < 3; ++fill)
        for (int nf : {0, 1, 4})
            for (int nb : {1, 3, 8})
                for (int64_t nq : {1, 31, 150})
                    for (int64_t rows : {0, 32, 7})
                        for (int64_t slab : {0, 4096, 300 << 10}) check_case(rng, nq, nb, 12, nf, rows, slab, fill);
    check_case(rng, 40, 1024, 3, 2, 16, 64 << 10, 1);
    std::printf("range plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
