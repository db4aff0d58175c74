// lmi_knn_plan.h -- the geometry of one lmi_knn call: how the base is cut into pieces (uploaded or scanned one at a time), a piece into
// splits (scanned by different waves of one query, their lists merged afterwards), the queries into groups, and the device bytes the
// call allocates for that (elem: the bytes of an input element -- 2 for the _f16 forms, whose uploaded queries and piece are halves).
// Host only and pure: the standard library, no HIP call, no kernel header -- lmi_host_knn.h passes the
// sizes, the free memory and the forced values in and acts on what comes back; tests/host/knn_plan_selftest.cpp checks it on the CPU.
//
// Nothing here can change a result (include/lmi_hip.h, lmi_knn: every score is one unsplit chain and the order is total); the
// geometry decides memory and speed only.
#pragma once
#include <algorithm>
#include <cstdint>

namespace lmi_knn_plan {

constexpr int MAX_K = 1024;          // LMI_KNN_MAX_K (lmi_host_knn.h asserts that they agree)
constexpr int MIN_LIST = 256;        // a query's sorted list holds max(MIN_LIST, k rounded up to a power of two) entries
constexpr int MAX_SPLITS = 1024;
constexpr int64_t AUTO_QUERY_ROWS = 8192;     // queries per group, at most, where the caller forces nothing
constexpr int64_t AUTO_PIECE_ROWS = 65536;    // rows per piece, at most
constexpr int64_t AUTO_SLAB_BYTES = 512ll << 20;   // the score slab of one (group, piece), at most

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t rup(int64_t a, int64_t b) { return cdiv(a, b) * b; }

struct Forced { int64_t piece_rows = 0; int splits = 0; int64_t query_rows = 0; };   // 0: chosen here

struct Plan {
    int64_t nq = 0, nb = 0;
    int d = 0, k = 0, l2 = 0, on_device = 0;
    int elem = 4;             // bytes of an input element: 4 = binary32 (lmi_knn), 2 = binary16 (lmi_knn_f16); sizes xq_bytes and xb_bytes only
    int list_rows = 0;        // entries of a query's sorted list (a power of two >= max(k, MIN_LIST))
    int kg = 0;               // groups of 8 links of a chain: the d links (d + 1 for L2), padded to a multiple of 32
    int64_t piece_rows = 0, pieces = 0;
    int splits = 0;
    int64_t query_rows = 0, query_groups = 0;
    int64_t pitch = 0;        // floats between two queries' rows of the score slab
    // device bytes, by buffer; the last four with host pointers only
    int64_t slab_bytes = 0, list_bytes = 0, qfrag_bytes = 0, qn_bytes = 0, xnh_bytes = 0;
    int64_t xq_bytes = 0, xb_bytes = 0, d_bytes = 0, i_bytes = 0;
    int64_t workspace_bytes = 0;
};

inline int list_rows_for(int k) {
    int p = MIN_LIST;
    while (p < k) p <<= 1;
    return p;
}

// the byte counts that follow from (piece_rows, splits, query_rows)
inline void size_buffers(Plan& p) {
    const int64_t qp = rup(p.query_rows, 32);
    p.pitch = rup(p.piece_rows, 64);
    p.slab_bytes = qp * p.pitch * 4;
    p.list_bytes = p.query_rows * p.splits * (int64_t)p.list_rows * 8;
    p.qfrag_bytes = qp / 32 * p.kg * 1024;
    p.qn_bytes = p.query_rows * 4;
    p.xnh_bytes = p.piece_rows * 4;
    p.xq_bytes = p.on_device ? 0 : p.query_rows * p.d * p.elem;
    p.xb_bytes = p.on_device ? 0 : p.piece_rows * p.d * p.elem;
    p.d_bytes = p.on_device ? 0 : p.query_rows * p.k * 4;
    p.i_bytes = p.on_device ? 0 : p.query_rows * p.k * 8;
    p.workspace_bytes = p.slab_bytes + p.list_bytes + p.qfrag_bytes + p.qn_bytes + p.xnh_bytes + p.xq_bytes + p.xb_bytes + p.d_bytes + p.i_bytes;
}

// (nq, nb, d, k) as lmi_knn accepts them (nq >= 1; nb may be 0).  free_bytes: the device's free memory, 0 = unknown; cus: its compute
// units.  With host pointers nothing that is allocated depends on nb: a piece is sized by the queries, d and the memory alone.
// elem (4 or 2): the geometry -- piece rows, pieces, splits, groups, pitch, lists -- is made for binary32 inputs whatever elem is, short
// memory included, so that a call on halves is cut exactly as the call on the widened arrays; only xq_bytes, xb_bytes and with them
// workspace_bytes follow elem.
inline Plan make_plan(int64_t nq, int64_t nb, int d, int k, bool l2, bool on_device, int64_t free_bytes, int cus, const Forced& f,
                      int elem = 4) {
    Plan p;
    p.nq = nq; p.nb = nb; p.d = d; p.k = k; p.l2 = l2; p.on_device = on_device;
    p.list_rows = list_rows_for(k);
    p.kg = (int)(rup(d + (l2 ? 1 : 0), 32) / 8);
    // query groups: as few as AUTO_QUERY_ROWS allows, of equal size up to the 32-query tile
    if (f.query_rows > 0) p.query_rows = std::min(f.query_rows, nq);
    else p.query_rows = std::min(nq, rup(cdiv(nq, cdiv(nq, AUTO_QUERY_ROWS)), 32));
    // pieces: the slab of one (group, piece) within AUTO_SLAB_BYTES
    if (f.piece_rows > 0) p.piece_rows = f.piece_rows;
    else {
        const int64_t by_slab = AUTO_SLAB_BYTES / (rup(p.query_rows, 32) * 4) / 256 * 256;
        p.piece_rows = std::max<int64_t>(256, std::min(AUTO_PIECE_ROWS, by_slab));
    }
    if (on_device) p.piece_rows = std::min(p.piece_rows, std::max<int64_t>(nb, 1));   // nothing is uploaded: no piece longer than the base
    auto pick_splits = [&]() {
        if (f.splits > 0) return std::min(f.splits, MAX_SPLITS);
        // one wave per (query, split): eight waves per compute unit when the queries alone do not give them, 2048 rows per split or more
        const int64_t want = cdiv((int64_t)std::max(cus, 1) * 8, p.query_rows);
        return (int)std::max<int64_t>(1, std::min<int64_t>({want, 32, p.piece_rows / 2048}));
    };
    p.splits = pick_splits();
    size_buffers(p);
    // automatic values give way to the memory there is: shorter pieces first, then smaller groups
    const int64_t budget = free_bytes > 0 ? free_bytes / 10 * 8 : INT64_MAX;
    while (p.workspace_bytes > budget) {
        if (f.piece_rows <= 0 && p.piece_rows > 256) p.piece_rows = std::max<int64_t>(256, p.piece_rows / 2 / 256 * 256);
        else if (f.query_rows <= 0 && p.query_rows > 32) p.query_rows = std::max<int64_t>(32, p.query_rows / 2 / 32 * 32);
        else break;   // the allocation will say what it wanted
        p.splits = pick_splits();
        size_buffers(p);
    }
    p.pieces = cdiv(nb, p.piece_rows);
    p.query_groups = cdiv(nq, p.query_rows);
    if (elem != p.elem) {
        p.elem = elem;
        size_buffers(p);
    }
    return p;
}

// piece i = rows [r0, r1) of the base, group g = queries [q0, q1), split s of a piece of len rows = its rows [a, b) (may be empty)
inline void piece_range(const Plan& p, int64_t i, int64_t* r0, int64_t* r1) {
    *r0 = i * p.piece_rows;
    *r1 = std::min(p.nb, *r0 + p.piece_rows);
}
inline void group_range(const Plan& p, int64_t g, int64_t* q0, int64_t* q1) {
    *q0 = g * p.query_rows;
    *q1 = std::min(p.nq, *q0 + p.query_rows);
}
inline void split_range(int64_t len, int splits, int s, int64_t* a, int64_t* b) {
    *a = len * s / splits;
    *b = len * (s + 1) / splits;
}

}  // namespace lmi_knn_plan
