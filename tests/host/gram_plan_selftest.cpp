// gram_plan_selftest.cpp -- stand-alone check of lmi_gram's geometry (csrc/lmi_gram_plan.h: pure host code) on the CPU, meant for
// -fsanitize=address,undefined (tests/test_pca_host.py builds and runs it).  For a grid of (n, d, compute units, forced values): the
// runs tile [0, n) exactly once in whole pieces, no panel straddles a piece seam, the tile map lists every (ta, tb) with ta <= tb
// exactly once and in bounds, the tiles cover the upper triangle of d x d, and the grid stays inside what a launch takes.
#include "lmi_gram_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lmi_gram_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static void check(int64_t n, int d, int cus, const Forced& f) {
    const Plan p = make_plan(n, d, cus, f);
    EXPECT(p.tile_cols == TILE_SMALL || p.tile_cols == TILE_LARGE);
    if (f.tile_cols) EXPECT(p.tile_cols == f.tile_cols);
    EXPECT(p.tiles_side >= 1 && (int64_t)p.tiles_side * p.tile_cols >= d && (int64_t)(p.tiles_side - 1) * p.tile_cols < d);
    EXPECT(p.tiles == (int64_t)p.tiles_side * (p.tiles_side + 1) / 2 && p.tiles <= 2080);
    EXPECT(p.pieces == cdiv(n, PIECE_ROWS) && p.pieces >= 1 && p.pieces <= (1 << 14));
    EXPECT(p.pieces_per_block >= 1 && p.pieces_per_block <= p.pieces);
    if (f.pieces_per_block) EXPECT(p.pieces_per_block == std::min(f.pieces_per_block, p.pieces));
    EXPECT(p.runs >= 1 && p.runs <= 65535 && p.runs == cdiv(p.pieces, p.pieces_per_block));
    // the runs tile [0, n) in whole pieces; none is empty; every run starts on a piece seam, so its panels never straddle one
    int64_t at = 0;
    for (int64_t r = 0; r < p.runs; ++r) {
        int64_t r0, r1;
        run_rows(p, r, &r0, &r1);
        EXPECT(r0 == at && r0 < r1 && r1 <= n && r0 % PIECE_ROWS == 0 && r1 - r0 <= p.pieces_per_block * PIECE_ROWS);
        if (r + 1 < p.runs) EXPECT(r1 - r0 == p.pieces_per_block * PIECE_ROWS);
        at = r1;
    }
    EXPECT(at == n);
    // the tile map: every pair of the upper triangle once, in bounds, in row order
    std::vector<char> seen((size_t)p.tiles_side * p.tiles_side, 0);
    int pa = 0, pb = -1;
    for (int64_t i = 0; i < p.tiles; ++i) {
        int ta = -1, tb = -1;
        tile_pair(p.tiles_side, i, &ta, &tb);
        EXPECT(0 <= ta && ta <= tb && tb < p.tiles_side && tb < 65536);
        EXPECT(!seen[(size_t)ta * p.tiles_side + tb]);
        EXPECT(ta > pa || (ta == pa && tb > pb));
        seen[(size_t)ta * p.tiles_side + tb] = 1;
        pa = ta;
        pb = tb;
    }
    for (int a = 0; a < p.tiles_side; ++a)
        for (int b = a; b < p.tiles_side; ++b) EXPECT(seen[(size_t)a * p.tiles_side + b]);
}

int main() {
    const int64_t ns[] = {1, 15, 16, 17, 4095, 4096, 4097, 8197, 1000000, ((int64_t)1 << 26) - 1, (int64_t)1 << 26};
    const int ds[] = {1, 31, 33, 45, 63, 64, 65, 96, 127, 128, 129, 130, 768, 4095, 4096};
    const int cus[] = {0, 1, 64, 256};
    const Forced forced[] = {{0, 0}, {64, 0}, {128, 0}, {0, 1}, {64, 1}, {128, 3}, {0, 1 << 14}, {64, 7}};
    for (int64_t n : ns)
        for (int d : ds)
            for (int cu : cus)
                for (const Forced& f : forced) check(n, d, cu, f);
    // the automatic choices the header names
    EXPECT(auto_tile_cols(96) == TILE_SMALL && auto_tile_cols(130) == TILE_SMALL && auto_tile_cols(768) == TILE_LARGE && auto_tile_cols(64) == TILE_SMALL);
    {
        const Plan p = make_plan(1000000, 768, 256, Forced{});   // 21 tiles x 49 runs of 5 pieces
        EXPECT(p.tiles == 21 && p.pieces == 245 && p.pieces_per_block == 5 && p.runs == 49);
        const Plan q = make_plan(10000000, 96, 256, Forced{});    // 3 tiles: the pieces fill the chip
        EXPECT(q.tiles == 3 && q.pieces == 2442 && q.pieces_per_block == 8 && q.runs == 306);
    }
    std::printf("gram plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
