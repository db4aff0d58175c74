// filter_plan_selftest.cpp -- stand-alone check of a filter set's host arithmetic (csrc/lmi_filter_plan.h: pure host code) on the CPU,
// meant for -fsanitize=address,undefined (tests/test_union_filter_host.py builds and runs it).  The argument checks refuse what the
// header says and nothing else; the normal form is sorted, unique, keeps every distinct id and no other, for empty lists, lists that
// arrive sorted, reversed, with duplicates and with the extreme ids; `allows` agrees with a linear search of the raw list; the check of
// filter_of names the first bad query; and the mask addressing stays inside [nf][n_rb_total] for every row of a layout with slack.
#include "lmi_filter_plan.h"

#include <cstdio>
#include <cstdlib>
#include <set>

using namespace lmi_filter_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static uint32_t g_state = 12345u;
static uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

static void check_refusals() {
    const uint32_t ids[4] = {3, 1, 2, 1};
    const int32_t keep_drop[2] = {KEEP, DROP};
    int bad = 7;
    {
        const int64_t off[3] = {0, 2, 4};
        EXPECT(check_lists(ids, off, 2, keep_drop, &bad) == nullptr && bad == -1);
        EXPECT(check_lists(ids, off, 2, keep_drop, nullptr) == nullptr);
        EXPECT(check_lists(ids, off, 0, keep_drop, &bad) != nullptr && bad == -1);
        EXPECT(check_lists(ids, off, -1, keep_drop, &bad) != nullptr);
        EXPECT(check_lists(ids, off, MAX_FILTERS + 1, keep_drop, &bad) != nullptr);   // (refused before offsets is read)
        EXPECT(check_lists(ids, nullptr, 2, keep_drop, &bad) != nullptr);
        EXPECT(check_lists(ids, off, 2, nullptr, &bad) != nullptr);
        EXPECT(check_lists(nullptr, off, 2, keep_drop, &bad) != nullptr && bad == -1);
    }
    {
        const int64_t off[3] = {1, 2, 4};
        EXPECT(check_lists(ids, off, 2, keep_drop, &bad) != nullptr && bad == -1);
    }
    {
        const int64_t off[3] = {0, 3, 2};
        EXPECT(check_lists(ids, off, 2, keep_drop, &bad) != nullptr && bad == 1);
    }
    {
        const int64_t off[3] = {0, 0, MAX_IDS};
        EXPECT(check_lists(ids, off, 2, keep_drop, &bad) != nullptr && bad == 1);   // (ids is never read)
        const int64_t ok[3] = {0, 0, 0};
        EXPECT(check_lists(nullptr, ok, 2, keep_drop, &bad) == nullptr);            // no ids at all: ids may be NULL
    }
    for (int32_t m : {-1, 2, 1 << 30}) {
        const int64_t off[3] = {0, 2, 4};
        const int32_t modes[2] = {DROP, m};
        EXPECT(check_lists(ids, off, 2, modes, &bad) != nullptr && bad == 1);
    }
    // MAX_FILTERS filters are accepted
    std::vector<int64_t> off((size_t)MAX_FILTERS + 1, 0);
    std::vector<int32_t> modes((size_t)MAX_FILTERS, KEEP);
    EXPECT(check_lists(nullptr, off.data(), MAX_FILTERS, modes.data(), &bad) == nullptr);
}

static void check_normal_form() {
    for (int round = 0; round < 200; ++round) {
        const int nf = 1 + (int)(rnd() % 6);
        std::vector<uint32_t> ids;
        std::vector<int64_t> off(1, 0);
        std::vector<int32_t> modes;
        for (int j = 0; j < nf; ++j) {
            const int shape = (int)(rnd() % 5);
            const int n = shape == 0 ? 0 : 1 + (int)(rnd() % 300);
            std::vector<uint32_t> one;
            for (int i = 0; i < n; ++i) one.push_back(shape == 1 ? (rnd() % 40) : shape == 2 ? (0xffffffffu - rnd() % 3) : rnd());
            if (shape == 3) std::sort(one.begin(), one.end());
            if (shape == 4) std::sort(one.rbegin(), one.rend());
            if (n && rnd() % 2) one.push_back(0u);
            ids.insert(ids.end(), one.begin(), one.end());
            off.push_back((int64_t)ids.size());
            modes.push_back((int32_t)(rnd() % 2));
        }
        EXPECT(check_lists(ids.data(), off.data(), nf, modes.data(), nullptr) == nullptr);
        const Lists l = normalise(ids.data(), off.data(), nf);
        EXPECT((int)l.off.size() == nf + 1 && l.off[0] == 0 && (size_t)l.off[(size_t)nf] == l.ids.size());
        for (int j = 0; j < nf; ++j) {
            const std::set<uint32_t> want(ids.begin() + off[(size_t)j], ids.begin() + off[(size_t)j + 1]);
            EXPECT(l.off[(size_t)j + 1] - l.off[(size_t)j] == (int32_t)want.size());
            EXPECT(std::equal(want.begin(), want.end(), l.ids.begin() + l.off[(size_t)j]));   // a set iterates ascending, unique
            for (int t = 0; t < 50; ++t) {
                const uint32_t probe = t < 25 && !want.empty() ? ids[(size_t)off[(size_t)j] + rnd() % (size_t)(off[(size_t)j + 1] - off[(size_t)j])]
                                                               : (t % 3 == 0 ? rnd() % 40 : rnd());
                const bool hit = want.count(probe) != 0;
                EXPECT(allows(l, j, KEEP, probe) == hit && allows(l, j, DROP, probe) == !hit);
            }
        }
    }
    // an empty keep list allows nothing, an empty drop list everything
    const int64_t off[2] = {0, 0};
    const Lists none = normalise(nullptr, off, 1);
    EXPECT(none.ids.empty() && !allows(none, 0, KEEP, 5u) && allows(none, 0, DROP, 5u));
}

static void check_filter_of() {
    const int32_t fo[6] = {-1, 0, 4, 2, 5, -2};
    EXPECT(first_bad_filter_of(nullptr, 6, 1) == -1);
    EXPECT(first_bad_filter_of(fo, 0, 5) == -1);
    EXPECT(first_bad_filter_of(fo, 4, 5) == -1);
    EXPECT(first_bad_filter_of(fo, 6, 5) == 4);
    EXPECT(first_bad_filter_of(fo, 6, 6) == 5);
    EXPECT(first_bad_filter_of(fo, 6, 4) == 2);
}

static void check_mask_addressing() {
    // a layout with spare row-blocks and a hole, as a mutated index has: every live row's word lies inside its bucket's row-blocks
    const int64_t rows[5] = {0, 1, 33, 64, 257}, start[5] = {0, 0, 3, 9, 11}, cap[5] = {0, 2, 2, 2, 10};
    const int64_t n_rb_total = 21;
    const int nf = 3;
    std::vector<int> seen((size_t)mask_words(nf, n_rb_total) * 32, 0);
    for (int j = 0; j < nf; ++j)
        for (int b = 0; b < 5; ++b)
            for (int64_t r = 0; r < rows[b]; ++r) {
                const int64_t w = mask_word(j, n_rb_total, start[b], r);
                EXPECT(w >= (int64_t)j * n_rb_total + start[b] && w < (int64_t)j * n_rb_total + start[b] + cap[b] && w < mask_words(nf, n_rb_total));
                EXPECT(mask_bit(r) >= 0 && mask_bit(r) < 32);
                EXPECT(seen[(size_t)w * 32 + (size_t)mask_bit(r)]++ == 0);   // no two rows share a bit
            }
}

int main() {
    check_refusals();
    check_normal_form();
    check_filter_of();
    check_mask_addressing();
    std::printf("filter plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
