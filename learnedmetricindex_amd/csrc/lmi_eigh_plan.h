// lmi_eigh_plan.h -- the schedule and the geometry of one lmi_eigh call.  The schedule is the contract's (include/lmi_hip.h): a sweep
// of the cyclic Jacobi method is D - 1 rounds of D / 2 disjoint pairs (the round-robin tournament on D = d rounded up to even players),
// a function of d alone; pair_of and slot_of are its two directions, both O(1).  The geometry is the library's choice and never shows
// in a bit: the form (the whole solve resident in one block's LDS, or streamed through device memory with one launch per round), the
// streamed form's tile of pairs x pairs, the LDS bytes and the grid.
// Pure: no HIP call, no kernel header; the functions the kernels share are __host__ __device__ when a HIP compiler reads this,
// plain inline functions otherwise -- tests/host/eigh_plan_selftest.cpp checks them on the CPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LMI_EIGH_HD __host__ __device__ inline
#else
#define LMI_EIGH_HD inline
#endif

namespace lmi_eigh_plan {

constexpr int MAX_D = 4096;
constexpr int SWEEP_CAP = 64;                 // LMI_EIGH_SWEEP_CAP (lmi_host_eigh.h asserts that they agree)
constexpr int FORM_RESIDENT = 1, FORM_STREAMED = 2;
constexpr int TILE_SMALL = 8, TILE_LARGE = 16;   // pairs per side of a streamed block's tile: TILE x TILE threads, one 2 x 2 block of A each
constexpr int LDS_MAX = 160 * 1024;           // bytes of LDS a gfx950 block may opt in to
constexpr int RESIDENT_THREADS = 1024;

LMI_EIGH_HD int even_d(int d) { return d + (d & 1); }
LMI_EIGH_HD int rounds(int d) { return even_d(d) - 1; }

// pair k in [0, D / 2) of round r in [0, D - 1): p < q.  k = 0 is {D - 1, r}, k = i is {(r + i) mod (D - 1), (r - i) mod (D - 1)}.
// A pair with q >= d sits out (odd d: the pair that holds D - 1).
LMI_EIGH_HD void pair_of(int D, int r, int k, int* p, int* q) {
    const int M = D - 1;
    const int a = k == 0 ? M : (r + k) % M, b = k == 0 ? r : (r - k + M) % M;
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// the other index of x's pair in round r (x in [0, D))
LMI_EIGH_HD int partner_of(int D, int r, int x) {
    const int M = D - 1;
    return x == M ? r : x == r ? M : (2 * r - x + M) % M;
}

// the k with x in pair_of(D, r, k)
LMI_EIGH_HD int slot_of(int D, int r, int x) {
    const int M = D - 1;
    if (x == M || x == r) return 0;
    const int k = (x - r + M) % M;   // x = r + k, or x = r - k' with k = M - k'
    return k < D / 2 ? k : M - k;
}

// Resident form: A [d][d] and V [d][d]; per pair of the round c, s, t (doubles) and state, p, q (ints); the rotated word.
constexpr int64_t resident_lds_bytes(int d) { return 16ll * d * d + 18ll * (d + (d & 1)) + 16; }
constexpr int resident_max_d_search() {
    int d = 1;
    while (d < MAX_D && resident_lds_bytes(d + 1) <= LDS_MAX) ++d;
    return d;
}
constexpr int RESIDENT_MAX_D = resident_max_d_search();   // 100

struct Forced { int form = 0, tile = 0; };   // 0: chosen here

struct Plan {
    int d = 0, D = 0;
    int form = 0;              // FORM_RESIDENT or FORM_STREAMED; 0: the forced form does not admit d
    int tile = 0;              // streamed: pairs per side of a tile
    int64_t lds_bytes = 0;     // resident: dynamic LDS of the one block; streamed: the rotations of a tile's row and column pairs
    int tiles_side = 0;        // streamed: cdiv(D / 2, tile)
    int a_tiles = 0;           // streamed: tiles (ti <= tj) of pairs x pairs: both triangles of A leave the same block
    int v_row_tiles = 0;       // streamed: cdiv(d, 2 * tile) row strips of V, each against tiles_side column-pair tiles
    int grid = 0;              // streamed: a_tiles + v_row_tiles * tiles_side blocks of tile * tile threads
    int launches_per_sweep = 0;
};

inline Plan make_plan(int d, const Forced& f) {
    Plan p;
    p.d = d;
    p.D = even_d(d);
    const int form = f.form ? f.form : d <= RESIDENT_MAX_D ? FORM_RESIDENT : FORM_STREAMED;
    if (form == FORM_RESIDENT) {
        if (d > RESIDENT_MAX_D) return p;
        p.form = FORM_RESIDENT;
        p.lds_bytes = resident_lds_bytes(d);
        p.grid = 1;
        p.launches_per_sweep = 0;   // one launch for the whole solve
        return p;
    }
    p.form = FORM_STREAMED;
    p.tile = f.tile ? f.tile : TILE_LARGE;
    p.lds_bytes = 2ll * p.tile * 32;
    p.tiles_side = (p.D / 2 + p.tile - 1) / p.tile;
    p.a_tiles = p.tiles_side * (p.tiles_side + 1) / 2;
    p.v_row_tiles = (d + 2 * p.tile - 1) / (2 * p.tile);
    p.grid = p.a_tiles + p.v_row_tiles * p.tiles_side;
    p.launches_per_sweep = p.D - 1;
    return p;
}

// streamed: block b in [0, a_tiles) -> (ti, tj), ti <= tj, row by row of the upper triangle of tiles
LMI_EIGH_HD void tile_pair(int tiles_side, int b, int* ti, int* tj) {
    int a = 0, row = tiles_side;
    while (b >= row) { b -= row; ++a; --row; }
    *ti = a;
    *tj = a + b;
}

}  // namespace lmi_eigh_plan
