"""GPU (`-m gpu`): the bucket cover, the pruning pass and the exact range search (lmi_cover_create, lmi_cover_order,
lmi_search_range_exact; include/lmi_hip.h).

The cover against tests/cover_ref.py: centres bit for bit, radii within the round-up.  The admitted sets between the reference sets
of half and twice the margin.  The exact call against the ground truth `_capi.range_knn` over everything the handle stores (ids as
sets per query, distance bits per id) and, bit for bit, against `scan_range` on `cover_order`'s order.  The shapes are the union
tests' (tests/union_ref.py) and the clustered case of tests/cover_ref.py; tests/test_cover_host.py checks on the oracle alone that
both have the properties relied on here."""
import numpy as np
import pandas as pd
import pytest
import torch

import cover_ref as cr
import union_ref as ur
from path_mass_ref import synthetic_tree

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
FIXED = {"ip": 0.8, "l2": 1.6}   # test_gpu_range.py's fixed radii on unit vectors: cos >= 0.2


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def build(capi, X, lab, ids, n_buckets, **kw):
    idx = capi.Index(0, **kw)
    idx.set_buckets(np.ascontiguousarray(X), np.asarray(lab, dtype=np.int64), n_buckets, ids=np.ascontiguousarray(ids, dtype=np.uint32))
    return idx


_built = {}


@pytest.fixture(scope="module")
def built(capi, oracle):
    """(index, cover, X, Q, labels, ids, L, radius, home) per (case, d, metric), made once; the cover is read-only."""
    def get(case, d, metric):
        key = (case, d, metric)
        if key not in _built:
            if case == "union":
                X, Q, lab, ids = ur.case(d)
                L, radius, home = ur.L, cr.union_radii(oracle, d, metric), None
            else:
                X, Q, lab, ids, radius, home = cr.clustered_case(oracle, d, metric)
                L = cr.CL
            idx = build(capi, X, lab, ids, L, metric=metric)
            _built[key] = (idx, capi.Cover(idx), X, Q, lab, ids, L, radius, home)
        return _built[key]
    yield get
    for t in _built.values():
        t[1].close()
        t[0].close()
    _built.clear()


def per_query(lims, dists, ids):
    """[{id: dist bits}] per query; ids in these cases are unique."""
    lims, dists, ids = np.asarray(lims), np.ascontiguousarray(dists, dtype=np.float32), np.asarray(ids)
    out = []
    for q in range(len(lims) - 1):
        a, b = int(lims[q]), int(lims[q + 1])
        m = dict(zip(ids[a:b].tolist(), dists[a:b].view(np.uint32).tolist()))
        assert len(m) == b - a, f"query {q}: an id came back twice"
        out.append(m)
    return out


def truth(capi, Q, X, ids, radius, metric):
    """The ground truth: `range_knn` over all objects, rows mapped to ids."""
    with capi.range_knn(np.ascontiguousarray(Q), np.ascontiguousarray(X), radius, metric=metric) as res:
        dd, rows = res.read()
        return per_query(res.lims, dd, np.asarray(ids)[rows.astype(np.int64)])


def check_cover(cover, idx, X, lab, L, what):
    c, R, n = cover.read()
    ref = cr.cover_of(X, lab, L)
    np.testing.assert_array_equal(n, idx.bucket_sizes(), err_msg=f"counts {what}")
    np.testing.assert_array_equal(n, ref["n"], err_msg=f"counts {what}")
    assert c.dtype == np.float32 and R.dtype == np.float32 and n.dtype == np.int64
    np.testing.assert_array_equal(c.view(np.uint32), ref["c"].view(np.uint32), err_msg=f"centre bits {what}")
    R64 = R.astype(np.float64)
    # binary64 chain noise is about d * 2^-53 and the binary32 round-up 2^-23: 2^-20 leaves room for both and no more
    assert np.all(ref["R"] <= R64) and np.all(R64 <= ref["R"] * (1.0 + 2.0 ** -20)), (what, ref["R"], R64)
    assert np.all((R == 0) == (ref["R"] == 0))
    return c, R, n


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_cover_read(built, d, metric):
    """d = 45: scalar loads, 64 and 136: 16-byte loads; L2: the stored norm column is not part of the cover."""
    idx, cover, X, Q, lab, ids, L, _, _ = built("union", d, metric)
    c, R, n = check_cover(cover, idx, X, lab, L, f"d={d} {metric}")
    assert n[0] == 0 and n[6] == 0 and R[0] == 0 and not c[0].any()   # the empty buckets
    assert n[1] == 1   # (one row: R is 0 where the integer mean is the row itself -- check_cover compares with the reference's verdict)


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", (33, 64))
def test_cover_of_the_clustered_case(built, d, metric):
    idx, cover, X, Q, lab, ids, L, _, _ = built("clustered", d, metric)
    c, R, n = check_cover(cover, idx, X, lab, L, f"clustered d={d} {metric}")
    assert n[cr.C_EMPTY] == 0 and n[cr.C_ONE] == 1 and n[cr.C_SAME] == cr.CSIZES[cr.C_SAME]
    assert R[cr.C_ONE] == 0 and R[cr.C_SAME] == 0 and R[cr.C_EMPTY] == 0
    assert np.all(R[[0, 4, 5, 6, 7]] > 0)


def check_order(order, counts, lo, hi, what):
    nq, nb = order.shape
    assert order.dtype == np.int32 and counts.dtype == np.int32
    for q in range(nq):
        got = order[q, :counts[q]]
        assert np.all(np.diff(got) > 0) and np.all(got >= 0), f"{what}: query {q} is not ascending"
        assert np.all(order[q, counts[q]:] == -1), f"{what}: query {q} is not padded with -1"
        s = set(got.tolist())
        assert set(np.flatnonzero(lo[q]).tolist()) <= s <= set(np.flatnonzero(hi[q]).tolist()), f"{what}: query {q}"


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
@pytest.mark.parametrize("case", ("union", "clustered"))
def test_cover_order_lies_between_the_reference_sets(capi, built, case, d, metric):
    idx, cover, X, Q, lab, ids, L, radius, home = built(case, d, metric)
    ref = cr.cover_of(X, lab, L)
    for r in (radius, FIXED[metric]):
        lo, hi = cr.admitted_ref(ref, Q, r, metric, 0.5), cr.admitted_ref(ref, Q, r, metric, 2.0)
        order, counts = idx.cover_order(Q, r, cover)
        assert order.shape == (Q.shape[0], max(1, counts.max()))
        check_order(order, counts, lo, hi, f"{case} d={d} {metric}")
        plan = capi.cover_last_plan()
        assert plan["GROUPS"] == 1 and plan["BUCKETS"] == L and plan["ADMITTED"] == counts.sum() and plan["MAX_PER_QUERY"] == counts.max()
        assert plan["NB_USED"] == order.shape[1]
    if case == "clustered":   # (the last pass above used the fixed radius: ask again with the case's own)
        order, counts = idx.cover_order(Q, radius, cover)
        assert counts.tolist() == [1] * cr.CNQ and np.array_equal(order[:, 0], home), "one bucket per query, each its own"


def many_clusters(oracle, L, d=24, nq=40, seed=9):
    """L well-separated clusters (L2), queries near stored rows with the 5th smallest distance as radius: every query admits its own
    bucket alone, and the buckets are spread over the words of the bitmap."""
    per = 64 if L == 1 else 12
    rs = np.random.RandomState(seed + L)
    lab = np.repeat(np.arange(L, dtype=np.int64), per)
    X = (3.0 * rs.randn(L, d)[lab] + 0.05 * rs.randn(L * per, d)).astype(np.float32)
    perm = rs.permutation(L * per)
    X, lab = np.ascontiguousarray(X[perm]), lab[perm]
    src = rs.choice(L * per, size=nq, replace=False)
    Q = np.ascontiguousarray((X[src] + 0.01 * rs.randn(nq, d)).astype(np.float32))
    D, _ = oracle.knn_l2(Q, X, 5)
    return X, Q, lab, np.arange(L * per, dtype=np.uint32) + 7, np.ascontiguousarray(D[:, 4], dtype=np.float32), lab[src]


@pytest.mark.parametrize("L", (1, 12, 70))
def test_cover_order_seams(capi, oracle, L):
    """L = 1: one word, one bit; L = 12; L = 70: the bitmap crosses a 32- and a 64-bit word.  nq = 1; host against device pointers; a
    group of 32 queries against the default; an nb that is too small."""
    X, Q, lab, ids, radius, home = many_clusters(oracle, L)
    idx = build(capi, X, lab, ids, L, metric="l2")
    try:
        with capi.Cover(idx) as cover:
            ref = cr.cover_of(X, lab, L)
            order, counts = idx.cover_order(Q, radius, cover)
            check_order(order, counts, cr.admitted_ref(ref, Q, radius, "l2", 0.5), cr.admitted_ref(ref, Q, radius, "l2", 2.0), f"L={L}")
            assert counts.tolist() == [1] * Q.shape[0] and np.array_equal(order[:, 0], home)
            if L == 70:
                assert (home < 32).any() and ((home >= 32) & (home < 64)).any() and (home >= 64).any()
            # +inf: every bucket, across every word
            o_all, c_all = idx.cover_order(Q, INF, cover)
            assert np.all(c_all == L) and np.array_equal(o_all, np.tile(np.arange(L, dtype=np.int32), (Q.shape[0], 1)))
            # nq = 1
            o1, c1 = idx.cover_order(Q[7:8], radius[7:8], cover)
            assert np.array_equal(o1, order[7:8]) and np.array_equal(c1, counts[7:8])
            # a wider order: padded with -1
            o5, c5 = idx.cover_order(Q, radius, cover, nb=5)
            assert o5.shape == (Q.shape[0], 5) and np.array_equal(o5[:, :1], order) and np.all(o5[:, 1:] == -1) and np.array_equal(c5, counts)
            # groups of 32 queries against the default: identical bits
            capi.cover_set_geometry(32)
            try:
                o32, c32 = idx.cover_order(Q, radius, cover)
                plan = capi.cover_last_plan()
                oa32, _ = idx.cover_order(Q, INF, cover)
            finally:
                capi.cover_set_geometry(0)
            assert plan["GROUPS"] == 2 and plan["QUERY_ROWS"] == 32
            assert np.array_equal(o32, order) and np.array_equal(c32, counts) and np.array_equal(oa32, o_all)
            # device pointers
            q_t = torch.from_numpy(np.array(Q)).cuda()
            o_t = torch.full((Q.shape[0], 3), 7, dtype=torch.int32, device="cuda")
            c_t = torch.full((Q.shape[0],), 7, dtype=torch.int32, device="cuda")
            idx.cover_order_device(q_t, radius, cover, 3, o_t, c_t)
            assert np.array_equal(o_t.cpu().numpy()[:, :1], order) and np.all(o_t.cpu().numpy()[:, 1:] == -1)
            assert np.array_equal(c_t.cpu().numpy(), counts)
            c_only = torch.full((Q.shape[0],), 7, dtype=torch.int32, device="cuda")
            idx.cover_order_device(q_t, INF, cover, 1, None, c_only)   # counting alone: nb is not looked at
            assert np.all(c_only.cpu().numpy() == L)
            # nb too small: refused by name, the outputs untouched
            if L > 1:
                o_t.fill_(7)
                c_t.fill_(7)
                with pytest.raises(capi.LmiError, match=rf"query 0 admits {L} buckets, more than nb = 3"):
                    idx.cover_order_device(q_t, INF, cover, 3, o_t, c_t)
                assert np.all(o_t.cpu().numpy() == 7) and np.all(c_t.cpu().numpy() == 7)
                with pytest.raises(capi.LmiError, match="more than nb = 1"):
                    idx.cover_order(Q, INF, cover, nb=1)
                assert all(v == 0 for v in capi.cover_last_plan().values())
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_search_range_exact_is_the_ground_truth(capi, built, d, metric):
    """Radii on computed distances (dist == radius on every query), ids unique: per query the id set of the brute force over all
    objects and per id its distance bits; and bit for bit `scan_range` on `cover_order`'s order."""
    idx, cover, X, Q, lab, ids, L, radius, _ = built("union", d, metric)
    lims, dd, ii = idx.search_range_exact(Q, radius, cover)
    want = truth(capi, Q, X, ids, radius, metric)
    assert per_query(lims, dd, ii) == want
    assert min(len(m) for m in want) >= 1 and lims[-1] > 5000
    plan, rplan = capi.cover_last_plan(), capi.range_last_plan()
    order, counts = idx.cover_order(Q, radius, cover)
    assert plan["NB_USED"] == order.shape[1] and plan["ADMITTED"] == counts.sum() and rplan["RESULTS"] == lims[-1]
    l2, d2, i2 = idx.scan_range(Q, order, radius)
    assert np.array_equal(lims, l2) and np.array_equal(ii, i2) and np.array_equal(dd.view(np.uint32), d2.view(np.uint32))


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("case", ("union", "clustered"))
def test_search_range_exact_fixed_and_special_radii(capi, built, case, metric):
    d = 64
    idx, cover, X, Q, lab, ids, L, radius, _ = built(case, d, metric)
    nq = Q.shape[0]
    for r in (FIXED[metric], radius):
        got = per_query(*idx.search_range_exact(Q, r, cover))
        assert got == truth(capi, Q, X, ids, r, metric), f"{case} {metric}"
        assert sum(len(m) for m in got) > nq
    special = np.array(radius)
    special[0::4], special[1::4], special[2::4] = INF, np.nan, -np.inf
    lims, dd, ii = idx.search_range_exact(Q, special, cover)
    got = per_query(lims, dd, ii)
    assert got == truth(capi, Q, X, ids, special, metric)
    n = np.diff(lims)
    assert np.all(n[0::4] == X.shape[0]) and np.all(n[1::4] == 0) and np.all(n[2::4] == 0) and np.all(n[3::4] >= 1)
    if case == "clustered":   # the pruning is real here: one bucket per query
        idx.search_range_exact(Q, radius, cover)
        plan = capi.cover_last_plan()
        assert plan["ADMITTED"] == nq and plan["NB_USED"] == 1 and plan["MAX_PER_QUERY"] == 1
    empty = idx.search_range_exact(Q[:0], 0.5, cover)
    assert empty[0].tolist() == [0] and empty[1].size == 0 and empty[2].size == 0


@pytest.mark.parametrize("metric", ur.METRICS)
def test_sort_filter_max_total_and_device_forms(capi, built, metric):
    d = 45
    idx, cover, X, Q, lab, ids, L, radius, _ = built("union", d, metric)
    lims, dd, ii = idx.search_range_exact(Q, radius, cover)
    order, counts = idx.cover_order(Q, radius, cover)
    # sort=True: scan_range's
    ls, ds, is_ = idx.search_range_exact(Q, radius, cover, sort=True)
    l2, d2, i2 = idx.scan_range(Q, order, radius, sort=True)
    assert np.array_equal(ls, l2) and np.array_equal(is_, i2) and np.array_equal(ds.view(np.uint32), d2.view(np.uint32))
    assert all(np.all(np.diff(ds[ls[q]: ls[q + 1]]) >= 0) for q in range(Q.shape[0]))
    # a keep filter: scan_range's with the same filter, and the truth restricted to the kept ids
    keep = np.asarray(ids)[::3]
    f = capi.Filter(idx, [keep])
    try:
        lf, df, jf = idx.search_range_exact(Q, radius, cover, filter=f)
        l3, d3, i3 = idx.scan_range(Q, order, radius, filter=f)
        assert np.array_equal(lf, l3) and np.array_equal(jf, i3) and np.array_equal(df.view(np.uint32), d3.view(np.uint32))
        kept = set(keep.tolist())
        assert per_query(lf, df, jf) == [{i: b for i, b in m.items() if i in kept} for m in per_query(lims, dd, ii)]
    finally:
        f.close()
    # max_total: at the exact total it passes, one below it fails and leaves no result
    total = int(lims[-1])
    assert idx.search_range_exact(Q, radius, cover, max_total=total)[0][-1] == total
    with pytest.raises(capi.LmiError, match="max_total"):
        idx.search_range_exact(Q, radius, cover, max_total=total - 1)
    # device tensors
    q_t = torch.from_numpy(np.array(Q)).cuda()
    c_t = torch.zeros(Q.shape[0], dtype=torch.int32, device="cuda")
    with idx.search_range_exact_device(q_t, radius, cover, counts_t=c_t) as res:
        assert res.nb_used == order.shape[1] and np.array_equal(c_t.cpu().numpy(), counts)
        rd, ri = res.read()
        assert np.array_equal(res.lims, lims) and np.array_equal(ri, ii) and np.array_equal(rd.view(np.uint32), dd.view(np.uint32))
        assert np.array_equal(res.pair_counts().sum(axis=1), np.diff(lims))
    # groups of 32 queries in the pruning pass: identical bits
    capi.cover_set_geometry(32)
    try:
        lg, dg, ig = idx.search_range_exact(Q, radius, cover)
        assert capi.cover_last_plan()["GROUPS"] == 5
    finally:
        capi.cover_set_geometry(0)
    assert np.array_equal(lg, lims) and np.array_equal(ig, ii) and np.array_equal(dg.view(np.uint32), dd.view(np.uint32))


@pytest.mark.parametrize("metric", ur.METRICS)
def test_validity_and_mutation(capi, oracle, metric):
    """After insert + delete (a relocated bucket) the old cover is stale; a new one on the mutated handle equals the cover of a fresh
    build of the same objects, bit for bit, and the exact call still equals the ground truth.  A clone view accepts its parent's
    cover, a subset refuses it."""
    d = 45
    X, Q, lab, ids = ur.case(d)
    radius = cr.union_radii(oracle, d, metric)
    first = np.arange(ur.N) < 5000
    gone = ids[np.flatnonzero(first)[::7]]
    idx = build(capi, X[first], lab[first], ids[first], ur.L, metric=metric)
    fresh = None
    try:
        old = capi.Cover(idx)
        view = idx.clone_view()
        assert per_query(*view.search_range_exact(Q, radius, old)) == truth(capi, Q, X[first], ids[first], radius, metric)
        with capi.Cover(view) as made_on_view:   # allowed on a clone view, and while one lives
            assert np.array_equal(made_on_view.read()[0], old.read()[0])
            idx.cover_order(Q, radius, made_on_view)
        view.close()
        sub = idx.subset(ids[np.flatnonzero(first)[::2]])
        try:
            with pytest.raises(capi.LmiError, match="stale"):
                sub.search_range_exact(Q, radius, old)
        finally:
            sub.close()
        assert idx.insert(np.ascontiguousarray(X[~first]), lab[~first], ids[~first]) == 1000
        assert idx.delete(gone) == gone.size
        assert idx.debug_layout()["counters"][1:].sum() > 0   # a bucket was relocated (or the slab re-packed)
        for call in (lambda: idx.search_range_exact(Q, radius, old), lambda: idx.cover_order(Q, radius, old)):
            with pytest.raises(capi.LmiError, match="stale"):
                call()
        old.close()
        alive = ~np.isin(ids, gone)
        order_of_objects = np.concatenate([np.flatnonzero(first & alive), np.flatnonzero(~first)])   # survivors of the build, then the inserted
        Xa, la, ia = X[order_of_objects], lab[order_of_objects], ids[order_of_objects]
        fresh = build(capi, Xa, la, ia, ur.L, metric=metric)
        with capi.Cover(idx) as new, capi.Cover(fresh) as ref:
            (c1, R1, n1), (c2, R2, n2) = new.read(), ref.read()
            assert np.array_equal(n1, n2) and np.array_equal(c1.view(np.uint32), c2.view(np.uint32))
            assert np.array_equal(R1.view(np.uint32), R2.view(np.uint32))
            check_cover(new, idx, Xa, la, ur.L, f"mutated {metric}")
            assert per_query(*idx.search_range_exact(Q, radius, new)) == truth(capi, Q, Xa, ia, radius, metric)
            with pytest.raises(capi.LmiError, match="stale"):
                fresh.search_range_exact(Q, radius, new)   # another index
    finally:
        if fresh is not None:
            fresh.close()
        idx.close()


def test_refusals(capi, built):
    X, Q, lab, ids = ur.case(45)
    for kw in (dict(prefilter=False), dict(storage="f16")):
        Xs = (np.rint(X * 256.0) / 256.0).astype(np.float32) if "storage" in kw else X   # binary16-exact rows for the f16 build
        idx = build(capi, Xs, lab, ids, ur.L, **kw)
        try:
            with pytest.raises(capi.LmiError, match="row-major"):
                capi.Cover(idx)
        finally:
            idx.close()
    empty = capi.Index(0)
    try:
        with pytest.raises(capi.LmiError, match="not built"):
            capi.Cover(empty)
    finally:
        empty.close()
    idx, cover, *_ = built("union", 45, "ip")
    other, other_cover, *_ = built("union", 64, "ip")
    with pytest.raises(capi.LmiError, match="stale"):
        idx.search_range_exact(Q, 0.5, other_cover)
    with pytest.raises(capi.LmiError, match="stale"):
        idx.cover_order(Q, 0.5, other_cover)


def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


def unit(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def gap_radii(lims, dists, fallback):
    """Per query a radius in the middle of the widest gap around the median of its sorted distances: no distance lies within rounding
    of it, so two correct implementations return the same SET."""
    r = np.full(len(lims) - 1, fallback, dtype=np.float32)
    for q in range(len(lims) - 1):
        v = np.sort(dists[lims[q]: lims[q + 1]])
        if v.size >= 4:
            j = v.size // 2
            r[q] = np.float32((float(v[j - 1]) + float(v[j])) / 2)
    return r


@pytest.mark.parametrize("levels", ([4], [4, 3]), ids=("one-level", "two-levels"))
def test_li_range_search_exact_equals_the_baseline(capi, levels):
    """`li.LearnedIndex.range_search_exact` on a 1-level and on a [4, 3] index == `Baseline.range_search` as sets; the cover is made on
    first use, kept, and made again after a mutation."""
    from learnedmetricindex_amd.li.Baseline import Baseline
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    Xs, Qs = unit(Xs), unit(Qs)
    if len(levels) == 1:
        dp = np.random.RandomState(2).randint(0, 4, size=(Xn.shape[0], 1)).astype(np.int64)
        li = LearnedIndex(net_from(root), {}, [(b,) for b in range(4)])
    else:
        li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    try:
        l0, d0, _, _ = Baseline().range_search(Qs, Xs, 0.6)
        radius = gap_radii(l0, d0, 0.6)
        lw, dw, iw, _ = Baseline().range_search(Qs, Xs, radius)
        want = [set(iw[lw[q]: lw[q + 1]].tolist()) for q in range(Qs.shape[0])]
        assert sum(len(s) for s in want) > 10 * Qs.shape[0]
        lims, dists, nns, clock = li.range_search_exact(frame(Xn), Qn, frame(Xs), Qs, dp, levels, radius)
        assert dists.dtype == np.float64 and nns.dtype == np.uint32 and clock["search"] > 0 and clock["buckets_visited"] >= 1
        assert [set(nns[lims[q]: lims[q + 1]].tolist()) for q in range(Qs.shape[0])] == want
        cover = li._engine._li_cover
        ls, ds, ns, _ = li.range_search_exact_resident(Qn, Qs, levels, radius, sort=True)
        assert li._engine._li_cover is cover   # kept
        assert np.array_equal(ls, lims) and all(np.all(np.diff(ds[ls[q]: ls[q + 1]]) >= 0) for q in range(Qs.shape[0]))
        assert [set(ns[ls[q]: ls[q + 1]].tolist()) for q in range(Qs.shape[0])] == want
        with pytest.raises(Exception, match="max_total"):
            li.range_search_exact_resident(Qn, Qs, levels, radius, max_total=int(lims[-1]) - 1)
        if len(levels) == 1:   # a mutation makes the kept cover stale: it is made again, and the deleted objects are gone
            gone = np.arange(1, 400)
            assert li.delete(gone) == gone.size
            lm, _, nm, _ = li.range_search_exact_resident(Qn, Qs, levels, radius)
            assert li._engine._li_cover is not cover
            dead = set(gone.tolist())
            assert [set(nm[lm[q]: lm[q + 1]].tolist()) for q in range(Qs.shape[0])] == [s - dead for s in want]
    finally:
        li.close()
