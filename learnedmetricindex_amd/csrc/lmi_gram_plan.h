// lmi_gram_plan.h -- the geometry of one lmi_gram call: how the rows are cut into pieces (the contract's: PIECE_ROWS rows each, the last
// may be shorter), the pieces into runs of consecutive pieces (one block folds a run in int64 registers), the d x d scatter matrix
// into square tiles of which only the upper triangle is computed, and the map from a block's linear tile number to its (ta, tb).
// Host only and pure: the standard library, no HIP call, no kernel header -- lmi_host_gram.h passes the sizes and the forced values in
// and acts on what comes back; tests/host/gram_plan_selftest.cpp checks it on the CPU.
//
// Nothing here can change a result (include/lmi_hip.h, lmi_gram: a piece's chain is never split and the fold is integer addition);
// PIECE_ROWS is the one constant that would, and it is not a choice.
#pragma once
#include <algorithm>
#include <cstdint>

namespace lmi_gram_plan {

constexpr int64_t PIECE_ROWS = 4096;   // LMI_GRAM_PIECE_ROWS (lmi_host_gram.h asserts that they agree)
constexpr int PANEL_ROWS = 16;         // rows a block stages per LDS panel; divides PIECE_ROWS: no panel straddles a piece seam
constexpr int TILE_SMALL = 64, TILE_LARGE = 128;   // tile widths the kernel is built for (four waves of 1 x 1 or 2 x 2 accumulators)
constexpr int BLOCKS_PER_CU = 4;       // blocks the automatic run length aims at, per compute unit

static_assert(PIECE_ROWS % PANEL_ROWS == 0, "a panel must not straddle a piece seam");

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Forced { int tile_cols = 0; int64_t pieces_per_block = 0; };   // 0: chosen here

struct Plan {
    int64_t n = 0;
    int d = 0;
    int tile_cols = 0;          // TILE_SMALL or TILE_LARGE
    int tiles_side = 0;         // cdiv(d, tile_cols)
    int64_t tiles = 0;          // tiles of the upper triangle, the diagonal included: grid.x
    int64_t pieces = 0;         // cdiv(n, PIECE_ROWS)
    int64_t pieces_per_block = 0;
    int64_t runs = 0;           // cdiv(pieces, pieces_per_block): grid.y
};

// columns a tiling computes, the padding and the diagonal tiles' lower halves included
inline int64_t tiled_work(int d, int tile_cols) {
    const int64_t t = cdiv(d, tile_cols);
    return t * (t + 1) / 2 * tile_cols * tile_cols;
}

// The wide tile feeds four MFMAs from four LDS reads, the narrow one one from two: the wide tile stays unless the narrow one saves a
// fifth of the work (d = 96: three 64-tiles against one 128-tile).
inline int auto_tile_cols(int d) { return tiled_work(d, TILE_SMALL) * 5 <= tiled_work(d, TILE_LARGE) * 4 ? TILE_SMALL : TILE_LARGE; }

inline Plan make_plan(int64_t n, int d, int cus, const Forced& f) {
    Plan p;
    p.n = n;
    p.d = d;
    p.tile_cols = f.tile_cols ? f.tile_cols : auto_tile_cols(d);
    p.tiles_side = (int)cdiv(d, p.tile_cols);
    p.tiles = (int64_t)p.tiles_side * (p.tiles_side + 1) / 2;
    p.pieces = cdiv(n, PIECE_ROWS);
    if (f.pieces_per_block > 0) {
        p.pieces_per_block = std::min(f.pieces_per_block, p.pieces);
    } else {
        const int64_t want_runs = std::max<int64_t>(1, cdiv((int64_t)std::max(cus, 1) * BLOCKS_PER_CU, p.tiles));
        p.pieces_per_block = cdiv(p.pieces, std::min(want_runs, p.pieces));
    }
    p.runs = cdiv(p.pieces, p.pieces_per_block);
    return p;
}

// rows [r0, r1) of run `run`: whole pieces, the last run ends at n
inline void run_rows(const Plan& p, int64_t run, int64_t* r0, int64_t* r1) {
    *r0 = run * p.pieces_per_block * PIECE_ROWS;
    *r1 = std::min(p.n, (run + 1) * p.pieces_per_block * PIECE_ROWS);
}

// tile number idx in [0, tiles) -> (ta, tb) with ta <= tb, row by row of the upper triangle: (0,0), (0,1), .., (0,T-1), (1,1), ..
inline void tile_pair(int tiles_side, int64_t idx, int* ta, int* tb) {
    int a = 0;
    int64_t row = tiles_side;   // tiles in row a
    while (idx >= row) { idx -= row; ++a; --row; }
    *ta = a;
    *tb = a + (int)idx;
}

}  // namespace lmi_gram_plan
