// eigh_plan_selftest.cpp -- stand-alone check of lmi_eigh's schedule and geometry (csrc/lmi_eigh_plan.h: pure host code) on the CPU,
// meant for -fsanitize=address,undefined (tests/test_eigh_host.py builds and runs it).  For every d in 1..130 and for 4096: the rounds
// of a sweep partition all d (d - 1) / 2 pairs, the pairs of a round are disjoint, partner_of and slot_of invert pair_of; the resident
// form's LDS holds what the kernel lays out in it and stays under the limit up to its bound; the streamed tiles cover every
// (row pair, column pair) once.
#include "lmi_eigh_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lmi_eigh_plan;

static long g_checks = 0;
static void expect(bool ok, const char* what, int line) {
    ++g_checks;
    if (!ok) { std::printf("FAILED %s:%d: %s\n", __FILE__, line, what); std::exit(1); }
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

static void check_schedule(int d) {
    const int D = even_d(d);
    EXPECT(D % 2 == 0 && D >= d && D - d <= 1 && rounds(d) == D - 1);
    std::vector<char> met((size_t)d * d, 0);
    long pairs = 0;
    for (int r = 0; r < D - 1; ++r) {
        std::vector<char> used((size_t)D, 0);
        for (int k = 0; k < D / 2; ++k) {
            int p = -1, q = -1;
            pair_of(D, r, k, &p, &q);
            EXPECT(0 <= p && p < q && q < D && p < d);
            EXPECT(!used[(size_t)p] && !used[(size_t)q]);   // the pairs of a round are disjoint
            used[(size_t)p] = used[(size_t)q] = 1;
            EXPECT(partner_of(D, r, p) == q && partner_of(D, r, q) == p && slot_of(D, r, p) == k && slot_of(D, r, q) == k);
            if (q >= d) continue;   // the bye
            EXPECT(!met[(size_t)p * d + q]);
            met[(size_t)p * d + q] = 1;
            ++pairs;
        }
    }
    EXPECT(pairs == (long)d * (d - 1) / 2);   // with "none twice" above: a partition
}

static void check_geometry(int d, int tile) {
    const Plan a = make_plan(d, Forced{}), res = make_plan(d, Forced{FORM_RESIDENT, 0}), p = make_plan(d, Forced{FORM_STREAMED, tile});
    EXPECT(a.form == (d <= RESIDENT_MAX_D ? FORM_RESIDENT : FORM_STREAMED) && res.form == (d <= RESIDENT_MAX_D ? FORM_RESIDENT : 0));
    if (res.form)   // A, V, a round's rotations by pair (three doubles, three ints), the rotated word
        EXPECT(res.grid == 1 && res.lds_bytes <= LDS_MAX && res.lds_bytes >= 16ll * d * d + res.D / 2 * 36 + 4);
    EXPECT(p.form == FORM_STREAMED && p.tile == (tile ? tile : TILE_LARGE) && p.lds_bytes <= 64 * 1024);
    EXPECT(p.tiles_side * p.tile >= p.D / 2 && (p.tiles_side - 1) * p.tile < p.D / 2);
    EXPECT(p.v_row_tiles * 2 * p.tile >= d && (p.v_row_tiles - 1) * 2 * p.tile < d);
    EXPECT(p.grid == p.a_tiles + p.v_row_tiles * p.tiles_side && p.grid > 0 && p.launches_per_sweep == p.D - 1);
    std::vector<char> seen((size_t)p.tiles_side * p.tiles_side, 0);
    for (int b = 0; b < p.a_tiles; ++b) {
        int ti = -1, tj = -1;
        tile_pair(p.tiles_side, b, &ti, &tj);
        EXPECT(0 <= ti && ti <= tj && tj < p.tiles_side && !seen[(size_t)ti * p.tiles_side + tj]);
        seen[(size_t)ti * p.tiles_side + tj] = 1;
    }
    EXPECT(p.a_tiles == p.tiles_side * (p.tiles_side + 1) / 2);   // with "none twice, ti <= tj" above: every tile of the triangle
}

int main() {
    for (int d = 1; d <= 4096; d = d < 130 ? d + 1 : d < 4095 ? 4095 : d + 1) {   // 1..130, 4095, 4096
        check_schedule(d);
        for (int tile : {0, TILE_SMALL, TILE_LARGE}) check_geometry(d, tile);
    }
    EXPECT(RESIDENT_MAX_D == 100);   // 16 d^2 + 18 D + 16 <= 160 KiB: the header and the tests name the figure
    EXPECT(resident_lds_bytes(RESIDENT_MAX_D) <= LDS_MAX && resident_lds_bytes(RESIDENT_MAX_D + 1) > LDS_MAX);
    std::printf("eigh plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
