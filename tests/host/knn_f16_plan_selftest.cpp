// knn_f16_plan_selftest.cpp -- stand-alone check of the input element size in lmi_knn's and lmi_knn_range's geometry
// (csrc/lmi_knn_plan.h, csrc/lmi_knn_range_plan.h: pure host code) on the CPU, meant for -fsanitize=address,undefined
// (tests/test_knn_f16_host.py builds and runs it).  For a grid of (nq, nb, d, k, metric, pointers, forced values, free memory) --
// the shapes and forced geometries of tests/knn_cases.py and tests/knn_f16_cases.py among them: the default element size is 4 and gives
// the plan the call without it gives; element size 2 halves xq_bytes and xb_bytes, takes exactly that off workspace_bytes and changes
// nothing else -- piece rows, pieces, splits, groups, pitch and lists are those of binary32, also where memory is short.
#include "lmi_knn_range_plan.h"

#include <cstdio>
#include <cstdlib>

namespace kp = lmi_knn_plan;
namespace krp = lmi_knn_range_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

// everything of a plan but elem, xq_bytes, xb_bytes and workspace_bytes
static bool same_geometry(const kp::Plan& a, const kp::Plan& b) {
    return a.nq == b.nq && a.nb == b.nb && a.d == b.d && a.k == b.k && a.l2 == b.l2 && a.on_device == b.on_device && a.list_rows == b.list_rows &&
           a.kg == b.kg && a.piece_rows == b.piece_rows && a.pieces == b.pieces && a.splits == b.splits && a.query_rows == b.query_rows &&
           a.query_groups == b.query_groups && a.pitch == b.pitch && a.slab_bytes == b.slab_bytes && a.list_bytes == b.list_bytes &&
           a.qfrag_bytes == b.qfrag_bytes && a.qn_bytes == b.qn_bytes && a.xnh_bytes == b.xnh_bytes && a.d_bytes == b.d_bytes && a.i_bytes == b.i_bytes;
}

static void check(int64_t nq, int64_t nb, int d, int k, bool l2, bool dev, int64_t free_bytes, int cus, const kp::Forced& f) {
    const kp::Plan p4 = kp::make_plan(nq, nb, d, k, l2, dev, free_bytes, cus, f);
    const kp::Plan q4 = kp::make_plan(nq, nb, d, k, l2, dev, free_bytes, cus, f, 4);
    const kp::Plan p2 = kp::make_plan(nq, nb, d, k, l2, dev, free_bytes, cus, f, 2);
    EXPECT(p4.elem == 4 && q4.elem == 4 && p2.elem == 2);
    EXPECT(same_geometry(p4, q4) && q4.xq_bytes == p4.xq_bytes && q4.xb_bytes == p4.xb_bytes && q4.workspace_bytes == p4.workspace_bytes);
    EXPECT(same_geometry(p4, p2));
    EXPECT(2 * p2.xq_bytes == p4.xq_bytes && 2 * p2.xb_bytes == p4.xb_bytes);
    EXPECT(p2.xq_bytes == (dev ? 0 : 2 * p2.query_rows * d) && p2.xb_bytes == (dev ? 0 : 2 * p2.piece_rows * d));
    EXPECT(p4.workspace_bytes - p2.workspace_bytes == p2.xq_bytes + p2.xb_bytes);
    EXPECT(p2.workspace_bytes == p2.slab_bytes + p2.list_bytes + p2.qfrag_bytes + p2.qn_bytes + p2.xnh_bytes + p2.xq_bytes + p2.xb_bytes + p2.d_bytes + p2.i_bytes);
    // the range call's plan: the same, with its own buffers unchanged
    const krp::Plan r4 = krp::make_plan(nq, nb, d, l2, dev, free_bytes, cus, f);
    const krp::Plan r2 = krp::make_plan(nq, nb, d, l2, dev, free_bytes, cus, f, 2);
    EXPECT(r4.g.elem == 4 && r2.g.elem == 2 && same_geometry(r4.g, r2.g));
    EXPECT(r4.g.list_bytes == 0 && r2.g.list_bytes == 0 && r2.g.d_bytes == 0 && r2.g.i_bytes == 0);
    EXPECT(2 * r2.g.xq_bytes == r4.g.xq_bytes && 2 * r2.g.xb_bytes == r4.g.xb_bytes);
    EXPECT(r2.radius_bytes == r4.radius_bytes && r2.count_bytes == r4.count_bytes && r2.offset_bytes == r4.offset_bytes);
    EXPECT(r4.workspace_bytes - r2.workspace_bytes == r2.g.xq_bytes + r2.g.xb_bytes);
    EXPECT(r2.workspace_bytes == r2.g.slab_bytes + r2.g.qfrag_bytes + r2.g.qn_bytes + r2.g.xnh_bytes + r2.g.xq_bytes + r2.g.xb_bytes + r2.radius_bytes +
                                     r2.count_bytes + r2.offset_bytes);
}

int main() {
    const int64_t edge = ((int64_t)1 << 31) - 1;
    // (nq, nb, d): tests/knn_cases.py, tests/knn_f16_cases.py, the full-size problem, the ends of the contract
    const int64_t shapes[][3] = {{67, 20011, 45},  {33, 4099, 768}, {129, 9000, 1000}, {300, 70001, 129},   {5, 300, 8},        {33, 1027, 40},
                                 {33, 1027, 44},   {67, 2011, 45},  {40, 3001, 136},   {129, 1500, 264},    {10000, 1000000, 768}, {1, 0, 1},
                                 {1, 1, 4096},     {edge, edge, 1}, {100000, 100000000, 768}};
    const int ks[] = {1, 10, 65, 1024};
    const kp::Forced forced[] = {{0, 0, 0},    {4096, 1, 0}, {4096, 3, 32}, {20011, 8, 0}, {1000, 2, 40},          {256, 1, 0},
                                 {1000, 3, 32}, {3001, 8, 0}, {2011, 8, 0},  {1, 1, 1},     {edge, 1024, 1 << 20}};
    const int64_t frees[] = {0, (int64_t)1 << 20, (int64_t)1 << 28, (int64_t)200 << 30};   // (1 MiB: memory so short that everything gives way)
    for (const auto& s : shapes)
        for (int k : ks)
            for (const kp::Forced& f : forced)
                for (int64_t fr : frees)
                    for (int l2 = 0; l2 < 2; ++l2)
                        for (int dev = 0; dev < 2; ++dev) check(s[0], s[1], (int)s[2], k, l2, dev, fr, 256, f);
    // the figures DESIGN.md 5.13.2 quotes: 10000 queries over 1M x 768 from host arrays
    {
        const kp::Plan p4 = kp::make_plan(10000, 1000000, 768, 10, false, false, (int64_t)200 << 30, 256, kp::Forced{});
        const kp::Plan p2 = kp::make_plan(10000, 1000000, 768, 10, false, false, (int64_t)200 << 30, 256, kp::Forced{}, 2);
        EXPECT(p2.piece_rows == 26624 && p2.pieces == 38 && p2.query_rows == 5024 && p2.query_groups == 2);
        EXPECT(p4.xb_bytes == 26624ll * 768 * 4 && p2.xb_bytes == 26624ll * 768 * 2 && p2.xq_bytes == 5024ll * 768 * 2);
    }
    std::printf("knn f16 plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
