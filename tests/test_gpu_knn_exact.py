"""GPU (`-m gpu`): the exact k-NN through the index (lmi_search_knn_exact; include/lmi_hip.h).

Against `scan_union` with every bucket listed and tests/union_ref.py on the oracle, bit for bit; the pruning against tests/cover_ref.py.
Shapes: the union tests' 6 000 objects in 12 buckets with a NaN row and 40 copies of one vector in three buckets (ties across buckets
at the k-th place), their first 700 objects (k = 1024 exceeds the index), and the clustered case."""
import numpy as np
import pandas as pd
import pytest
import torch

import cover_ref as cr
import union_ref as ur
from path_mass_ref import synthetic_tree

pytestmark = pytest.mark.gpu

SMALL = 700   # objects of the small handle: fewer than LMI_UNION_MAX_K


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def build(capi, X, lab, ids, n_buckets, **kw):
    idx = capi.Index(0, **kw)
    idx.set_buckets(np.ascontiguousarray(X), np.asarray(lab, dtype=np.int64), n_buckets, ids=np.ascontiguousarray(ids, dtype=np.uint32))
    return idx


last_error = lambda capi: capi.lib().lmi_last_error().decode("utf-8", "replace")


def case(d):
    """`ur.tie_case(d)` (queries 0..3 equal a vector stored 40 times in buckets 5, 3 and 11) with a NaN in one row of bucket 11."""
    X, Q, lab, ids, _ = ur.tie_case(d)
    X[int(np.flatnonzero(lab == 11)[100]), d // 2] = np.nan
    return X, Q, lab, ids


_built = {}


@pytest.fixture(scope="module")
def built(capi, oracle):
    """(index, cover, X, Q, labels, ids, L) per (case, d, metric), made once: `case(d)`, its first 700 objects, `cr.clustered_case`."""
    def get(name, d, metric):
        key = (name, d, metric)
        if key not in _built:
            if name == "clustered":
                X, Q, lab, ids = cr.clustered_case(oracle, d, metric)[:4]
                L = cr.CL
            else:
                X, Q, lab, ids = case(d)
                L = ur.L
                if name == "small":
                    X, lab, ids = X[:SMALL], lab[:SMALL], ids[:SMALL]
            idx = build(capi, X, lab, ids, L, metric=metric)
            _built[key] = (idx, capi.Cover(idx), X, Q, lab, ids, L)
        return _built[key]
    yield get
    for t in _built.values():
        t[1].close()
        t[0].close()
    _built.clear()


def same_bits(got, want, what):
    for name, g, w in zip(("dists", "ids", "counts", "visited"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if name == "dists":
            g, w = g.view(np.uint32), w.view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


@pytest.mark.parametrize("k", (1, 10, 129, 1024))
@pytest.mark.parametrize("d", ur.DIMS)
@pytest.mark.parametrize("metric", ur.METRICS)
def test_equals_the_scan_of_every_bucket(capi, oracle, built, metric, d, k):
    """dists, ids and counts == `scan_union` with the order arange(L) on the same handle == `union_ref` on the oracle.  The full
    handle: a NaN row (R_b = +inf: for IP the lone seed, above the other tied buckets), ties across buckets at the k-th place of queries 0..3 for k = 1 and 10.  The small handle at
    k = 1024: the seeds cannot hold k rows (tau = +inf) and k exceeds the index (padding, counts)."""
    for name in ("full", "small"):
        idx, cover, X, Q, lab, ids, L = built(name, d, metric)
        order = np.tile(np.arange(L, dtype=np.int32), (ur.NQ, 1))
        dd, ii, cc, visited = idx.search_knn_exact(Q, k, cover)
        plan = capi.knn_exact_last_plan()
        want = idx.scan_union(Q, order, k)
        same_bits((dd, ii, cc), want, f"{name} against scan_union")
        rows, labs = ur.buckets_of(X, lab, ids)
        same_bits((dd, ii, cc), ur.union_ref(oracle, rows, labs, order, Q, k, metric), f"{name} against the oracle")
        n_live = int(np.sum(idx.bucket_sizes() > 0))
        assert visited.dtype == np.int32 and np.all(visited >= 1) and np.all(visited <= n_live)
        assert plan["GROUPS"] == 1 and plan["ADMITTED"] >= ur.NQ and plan["NB_REST"] == plan["MAX_PER_QUERY"] <= n_live
        if name == "small" and k == 1024:
            assert np.all(cc < k) and np.all(visited == n_live) and plan["TAU_INF"] == ur.NQ and plan["SEED_BUCKETS"] == ur.NQ * n_live
        else:
            assert np.all(cc == k) and plan["TAU_INF"] == 0
    if k <= 10:   # the ties: queries 0..3 are the vector itself, and its copies in bucket 3 come before those in 5 and 11
        idx, cover, X, Q, lab, ids, L = built("full", d, metric)
        dd, ii, _, _ = idx.search_knn_exact(Q[:4], k, cover)
        tied = np.flatnonzero((X == Q[0]).all(axis=1))
        assert len(set(lab[tied].tolist())) == 3 and set(ii[0].tolist()) <= set(ids[tied[lab[tied] == 3]].tolist())
        if metric == "ip":   # the inputs make the split's rank rewrite show: bucket 11's ball alone is unbounded and it holds k rows, so it
            # is the lone seed, ABOVE the tied buckets 3 and 5 of the rest scan; with its rank left at 0 its copies would come first
            R, n = (cr.cover_of(X, lab, L)[key] for key in ("R", "n"))
            assert not np.isfinite(R[11]) and np.isfinite(np.delete(R, 11)).all() and n[11] >= k
            assert capi.knn_exact_last_plan()["SEED_BUCKETS"] == 4


@pytest.mark.parametrize("metric", ur.METRICS)
def test_it_prunes_as_the_reference_says(capi, oracle, built, metric):
    d, k = 64, 10
    idx, cover, X, Q, lab, ids, L = built("clustered", d, metric)
    D, _ = (oracle.knn_ip if metric == "ip" else oracle.knn_l2)(np.ascontiguousarray(Q), np.ascontiguousarray(X), k)
    ref = cr.cover_of(X, lab, L)
    # a condition on the inputs, from the reference and the oracle alone: one bucket per query at the true 10th distance
    assert cr.admitted_ref(ref, Q, cr.dists_of(D, metric)[:, k - 1], metric).sum(axis=1).tolist() == [1] * cr.CNQ
    dd, ii, cc, visited = idx.search_knn_exact(Q, k, cover)
    plan = capi.knn_exact_last_plan()
    assert visited.tolist() == [1] * cr.CNQ and plan["ADMITTED"] == cr.CNQ and plan["SEED_BUCKETS"] == cr.CNQ and plan["NB_REST"] == 1
    np.testing.assert_array_equal(dd.view(np.uint32), cr.dists_of(D, metric).view(np.uint32))
    # k = 200, d = 45 (a replay of the schedule on cover_ref): several seeds, for some queries a rest of 1 to 3 buckets, every query prunes
    idx, cover, X, Q, lab, ids, L = built("clustered", 45, metric)
    order = np.tile(np.arange(L, dtype=np.int32), (cr.CNQ, 1))
    got = idx.search_knn_exact(Q, 200, cover)
    plan = capi.knn_exact_last_plan()
    same_bits(got, idx.scan_union(Q, order, 200), "clustered against scan_union")
    same_bits(got, ur.union_ref(oracle, *ur.buckets_of(X, lab, ids, L), order, Q, 200, metric), "clustered against the oracle")
    assert plan["ADMITTED"] > plan["SEED_BUCKETS"] > cr.CNQ and np.all(got[3] < np.sum(idx.bucket_sizes() > 0))
    # on any fixture the rule admits at tau what it admits at the final k-th distance, or more
    idx, cover, X, Q, lab, ids, L = built("full", d, metric)
    dd, _, _, visited = idx.search_knn_exact(Q, k, cover)
    assert np.all(visited >= cr.admitted_ref(cr.cover_of(X, lab, L), Q, dd[:, k - 1], metric).sum(axis=1))


@pytest.mark.parametrize("metric", ur.METRICS)
def test_geometry_pointers_and_views_cannot_show(capi, built, metric):
    d, k = 45, 129
    idx, cover, X, Q, lab, ids, L = built("full", d, metric)
    want = idx.search_knn_exact(Q, k, cover)
    capi.cover_set_geometry(query_rows=7)
    capi.union_set_geometry(query_rows=32, slab_bytes=1 << 20)
    try:
        got = idx.search_knn_exact(Q, k, cover)
        plan, uplan = capi.knn_exact_last_plan(), capi.union_last_plan()
    finally:
        capi.cover_set_geometry(0)
        capi.union_set_geometry(0, 0)
    assert plan["GROUPS"] == -(-ur.NQ // 7) and plan["QUERY_ROWS"] == 7 and uplan["QUERY_ROWS"] == 32 and uplan["GROUPS"] == 5
    same_bits(got, want, "forced geometry")
    t = idx.search_knn_exact(torch.from_numpy(np.array(Q)).cuda(), k, cover)
    same_bits([x.cpu().numpy().view(np.uint32) for x in t], [np.ascontiguousarray(x).view(np.uint32) for x in want], "device tensors")
    view = idx.clone_view()
    try:
        same_bits(view.search_knn_exact(Q, k, cover), want, "clone view")
    finally:
        view.close()
    dd, ii, cc, vv = idx.search_knn_exact(Q[:0], k, cover)
    assert dd.shape == (0, k) and vv.shape == (0,) and all(v == 0 for v in capi.knn_exact_last_plan().values())


def test_stale_and_refused(capi, built):
    X, Q, lab, ids = ur.case(45)
    first = np.arange(ur.N) < 5000
    idx = build(capi, X[first], lab[first], ids[first], ur.L)
    q_t = torch.from_numpy(np.array(Q)).cuda()
    d_t = torch.full((ur.NQ, 10), 7.0, dtype=torch.float32, device="cuda")
    i_t, c_t, v_t = (torch.full(s, 7, dtype=torch.int32, device="cuda") for s in ((ur.NQ, 10), (ur.NQ,), (ur.NQ,)))

    def raw(index, cover, k):
        return capi.lib().lmi_search_knn_exact(index._h, cover._c, capi._ptr(q_t), ur.NQ, k, capi._ptr(d_t), capi._ptr(i_t), capi._ptr(c_t),
                                               capi._ptr(v_t), 1)

    untouched = lambda: bool((d_t == 7).all() and (i_t == 7).all() and (c_t == 7).all() and (v_t == 7).all())
    try:
        with capi.Cover(idx) as cover:
            assert raw(idx, cover, 10) == 0 and not untouched()
            for t in (d_t, i_t, c_t, v_t):
                t.fill_(7)
            for k in (0, 1025):
                assert raw(idx, cover, k) != 0 and "outside [1,1024]" in last_error(capi) and untouched()
                with pytest.raises(ValueError):
                    idx.search_knn_exact(Q, k, cover)
            assert idx.insert(np.ascontiguousarray(X[~first]), lab[~first], ids[~first]) == 1000
            assert raw(idx, cover, 10) != 0 and "stale" in last_error(capi) and untouched()
            with pytest.raises(capi.LmiError, match="stale"):
                idx.search_knn_exact(Q, 10, cover)
        other, other_cover, *_ = built("full", 64, "ip")
        for kw in (dict(prefilter=False), dict(storage="f16")):
            Xs = (np.rint(X * 256.0) / 256.0).astype(np.float32) if "storage" in kw else X
            bad = build(capi, Xs, lab, ids, ur.L, **kw)
            try:
                assert raw(bad, other_cover, 10) != 0 and "row-major" in last_error(capi) and untouched()
            finally:
                bad.close()
    finally:
        idx.close()


def test_a_query_that_admits_more_than_1024_buckets_is_refused(capi):
    """L = 1100 tight buckets of one or two rows, k = 1024: the 32 seeds hold fewer than k rows, tau stays +inf, all are admitted."""
    L, d, nq = 1100, 3, 3
    rs = np.random.RandomState(3)
    lab = np.concatenate([np.arange(L), np.arange(0, L, 2)]).astype(np.int64)
    X = (rs.randn(L, d)[lab] + 0.01 * rs.randn(lab.shape[0], d)).astype(np.float32)
    Q = rs.randn(nq, d).astype(np.float32)
    idx = build(capi, X, lab, np.arange(lab.shape[0], dtype=np.uint32) + 9, L, metric="l2")
    try:
        with capi.Cover(idx) as cover:
            q_t = torch.from_numpy(Q).cuda()
            outs = [torch.full(s, 7, dtype=t, device="cuda") for s, t in (((nq, 1024), torch.float32), ((nq, 1024), torch.int32),
                                                                          ((nq,), torch.int32), ((nq,), torch.int32))]
            rc = capi.lib().lmi_search_knn_exact(idx._h, cover._c, capi._ptr(q_t), nq, 1024, *(capi._ptr(t) for t in outs), 1)
            assert rc != 0 and "query 0 needs 1100 buckets" in last_error(capi)
            assert all(bool((t == 7).all()) for t in outs)
    finally:
        idx.close()


@pytest.mark.parametrize("levels", ([4], [4, 3]), ids=("one-level", "two-levels"))
def test_li_search_exact_equals_the_baseline(capi, levels):
    """`li.search_exact` == `Baseline.search` as sets with equal distance bits per id; a following `li.search` returns what it did."""
    from learnedmetricindex_amd.li.Baseline import Baseline, _unit
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    frame = lambda X: pd.DataFrame(X, index=np.arange(1, X.shape[0] + 1))   # object ids are 1-based

    def fixed(a):
        # unit rows on which the Baseline's own normalisation is the identity, so that both sides score the same bits
        for _ in range(5):
            a = _unit(a)
        return a, (_unit(a) == a).all(axis=1)

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    (Xs, keep), (Qs, qkeep) = fixed(Xs), fixed(Qs)
    Xn, Xs, dp, Qn, Qs = Xn[keep], np.ascontiguousarray(Xs[keep]), dp[keep], Qn[qkeep], np.ascontiguousarray(Qs[qkeep])
    assert Xs.shape[0] > 3900 and Qs.shape[0] > 290
    if len(levels) == 1:
        dp = np.random.RandomState(2).randint(0, 4, size=(Xn.shape[0], 1)).astype(np.int64)
        li = LearnedIndex(net_from(root), {}, [(b,) for b in range(4)])
    else:
        li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    k = 25
    try:
        before = li.search(frame(Xn), Qn, frame(Xs), Qs, dp, levels, n_buckets=2, k=10)[:2]
        dists, nns, clock = li.search_exact(frame(Xs), Qs, dp, levels, k)
        wd, wi, _ = Baseline().search(Qs, Xs, k)
        assert dists.dtype == np.float64 and nns.dtype == np.uint32 and dists.shape == nns.shape == (Qs.shape[0], k)
        assert clock["search"] > 0 and 1 <= clock["buckets_visited"] <= len(bucket_paths if len(levels) > 1 else range(4))
        for q in range(Qs.shape[0]):
            got = dict(zip(nns[q].tolist(), dists[q].astype(np.float32).view(np.uint32).tolist()))
            assert got == dict(zip(wi[q].tolist(), np.ascontiguousarray(wd[q], dtype=np.float32).view(np.uint32).tolist())), q
        cover = li._engine._li_cover
        d2, n2, _ = li.search_exact_resident(Qs, k)
        assert li._engine._li_cover is cover and np.array_equal(n2, nns) and np.array_equal(d2, dists)
        after = li.search(frame(Xn), Qn, frame(Xs), Qs, dp, levels, n_buckets=2, k=10)[:2]
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        li.close()
