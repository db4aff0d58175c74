// knn_plan_selftest.cpp -- stand-alone check of lmi_knn's geometry (csrc/lmi_knn_plan.h: pure host code) on the CPU, meant for
// -fsanitize=address,undefined (tests/test_knn_host.py builds and runs it).  For a grid of (nq, nb, d, k, metric, pointers, forced
// values, free memory): the pieces tile [0, nb) exactly once, the splits tile every piece, the query groups tile [0, nq), no count is
// zero where there is work, the byte counts add up, and with host pointers nothing allocated depends on nb.
#include "lmi_knn_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace lmi_knn_plan;

static long g_checks = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);              \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)

static void check(int64_t nq, int64_t nb, int d, int k, bool l2, bool dev, int64_t free_bytes, int cus, const Forced& f) {
    const Plan p = make_plan(nq, nb, d, k, l2, dev, free_bytes, cus, f);
    EXPECT(p.list_rows >= k && p.list_rows >= MIN_LIST && (p.list_rows & (p.list_rows - 1)) == 0 && p.list_rows <= 1024);
    EXPECT(p.kg % 4 == 0 && p.kg * 8 >= d + (l2 ? 1 : 0) && p.kg * 8 < d + 1 + 32);
    EXPECT(p.piece_rows >= 1 && p.query_rows >= 1 && p.query_rows <= nq && p.splits >= 1 && p.splits <= MAX_SPLITS);
    if (f.piece_rows > 0) EXPECT(p.piece_rows == (dev ? std::min(f.piece_rows, std::max<int64_t>(nb, 1)) : f.piece_rows));
    if (f.splits > 0) EXPECT(p.splits == f.splits);
    if (f.query_rows > 0) EXPECT(p.query_rows == std::min(f.query_rows, nq));
    EXPECT(p.pitch >= p.piece_rows && p.pitch % 64 == 0);
    // pieces tile [0, nb) exactly once, in order; none is empty
    EXPECT((p.pieces == 0) == (nb == 0));
    int64_t at = 0;
    const int64_t step = p.pieces > 64 ? p.pieces / 7 : 1;   // huge counts: every piece's bounds by formula, a sample walked
    for (int64_t i = 0; i < p.pieces; i += (i + step < p.pieces || i == p.pieces - 1 ? step : p.pieces - 1 - i)) {
        int64_t r0, r1;
        piece_range(p, i, &r0, &r1);
        EXPECT(r0 == i * p.piece_rows && r0 < r1 && r1 <= nb && r1 - r0 <= p.piece_rows);
        if (step == 1) EXPECT(r0 == at);
        if (i == p.pieces - 1) EXPECT(r1 == nb);
        else EXPECT(r1 - r0 == p.piece_rows);
        at = r1;
        // the splits tile the piece
        int64_t sat = 0, nonempty = 0;
        for (int s = 0; s < p.splits; ++s) {
            int64_t a, b;
            split_range(r1 - r0, p.splits, s, &a, &b);
            EXPECT(a == sat && a <= b && b <= r1 - r0);
            nonempty += b > a;
            sat = b;
        }
        EXPECT(sat == r1 - r0 && nonempty >= 1);
    }
    if (p.pieces) EXPECT(at == nb);
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
    // the bytes
    const int64_t qp = rup(p.query_rows, 32);
    EXPECT(p.slab_bytes == qp * p.pitch * 4 && p.list_bytes == p.query_rows * p.splits * (int64_t)p.list_rows * 8);
    EXPECT(p.qfrag_bytes == qp * p.kg * 32 && p.qn_bytes == 4 * p.query_rows && p.xnh_bytes == 4 * p.piece_rows);
    if (dev) EXPECT(p.xq_bytes == 0 && p.xb_bytes == 0 && p.d_bytes == 0 && p.i_bytes == 0);
    else EXPECT(p.xq_bytes == 4 * p.query_rows * d && p.xb_bytes == 4 * p.piece_rows * d && p.d_bytes == 4 * p.query_rows * k && p.i_bytes == 8 * p.query_rows * k);
    EXPECT(p.workspace_bytes == p.slab_bytes + p.list_bytes + p.qfrag_bytes + p.qn_bytes + p.xnh_bytes + p.xq_bytes + p.xb_bytes + p.d_bytes + p.i_bytes);
    EXPECT(p.workspace_bytes > 0);
    if (free_bytes > 0 && f.piece_rows == 0 && f.query_rows == 0 && p.workspace_bytes > free_bytes / 10 * 8)
        EXPECT(p.piece_rows <= 256 && p.query_rows <= 32);   // it gave way as far as it goes
    // host pointers: nothing allocated depends on nb
    if (!dev) {
        for (int64_t nb2 : {(int64_t)0, (int64_t)1, (int64_t)4096, (int64_t)1 << 20, ((int64_t)1 << 31) - 1}) {
            const Plan o = make_plan(nq, nb2, d, k, l2, dev, free_bytes, cus, f);
            EXPECT(o.workspace_bytes == p.workspace_bytes && o.piece_rows == p.piece_rows && o.splits == p.splits && o.query_rows == p.query_rows);
        }
    }
}

int main() {
    const int64_t edge = ((int64_t)1 << 31) - 1;
    const int64_t nqs[] = {1, 33, 300, 8193, 100000, edge};
    const int64_t nbs[] = {0, 1, 4, 31, 33, 255, 256, 257, 4099, 20011, 70001, 1000000, 100000000, edge};
    const int ds[] = {1, 45, 768, 4096};
    const int ks[] = {1, 10, 65, 257, 1024};
    const Forced forced[] = {{0, 0, 0}, {4096, 1, 0}, {4096, 3, 32}, {20011, 8, 0}, {1000, 2, 40}, {1, 1, 1}, {edge, 1024, 1 << 20}, {0, 5, 0}, {100, 0, 7}};
    const int64_t frees[] = {0, (int64_t)1 << 28, (int64_t)200 << 30};
    for (int64_t nq : nqs)
        for (int64_t nb : nbs)
            for (int d : ds)
                for (int k : ks)
                    for (const Forced& f : forced)
                        for (int64_t fr : frees)
                            for (int l2 = 0; l2 < 2; ++l2)
                                for (int dev = 0; dev < 2; ++dev) check(nq, nb, d, k, l2, dev, fr, 256, f);
    // the cases the header's formula names: automatic values on a full-size problem
    {
        const Plan p = make_plan(10000, 1000000, 768, 10, false, false, (int64_t)200 << 30, 256, Forced{});
        EXPECT(p.query_groups == 2 && p.query_rows == 5024 && p.piece_rows == 26624 && p.pieces == 38 && p.splits == 1);
        const Plan q = make_plan(10000, 100000000, 768, 10, false, false, (int64_t)200 << 30, 256, Forced{});
        EXPECT(q.workspace_bytes == p.workspace_bytes && q.pieces == 3757);
        const Plan s = make_plan(8, 1000000, 768, 1024, true, true, (int64_t)200 << 30, 256, Forced{});
        EXPECT(s.splits == 32 && s.piece_rows == 65536 && s.list_rows == 1024);
    }
    std::printf("knn plan selftest: clean (%ld checks)\n", g_checks);
    return 0;
}
