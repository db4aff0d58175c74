"""GPU (`-m gpu`): the union scan (lmi_scan_union, lmi_search_union, lmi_search_tree_union; include/lmi_hip.h) -- per query the k best
objects of the union of its visited buckets, k up to 1024 -- against the unchanged CPU oracle.

Every comparison is exact: dists as uint32 bit patterns, ids and counts with array_equal, against tests/union_ref.py (the contract in
numpy on oracle.knn_ip / oracle.knn_l2).  The inputs come from union_ref too; tests/test_union_host.py checks on the oracle alone that
they have the properties relied on here (most queries fill k = 100, the tie cases tie, the short cases come up short)."""
import numpy as np
import pandas as pd
import pytest
import torch

import union_ref as ur
from path_mass_ref import synthetic_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def same(got, want, what=""):
    d, i, c = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got[:3])
    assert d.dtype == np.float32 and d.shape == want[0].shape and i.shape == want[1].shape and c.shape == want[2].shape, what
    np.testing.assert_array_equal(c.astype(np.int32), want[2], err_msg=f"counts {what}")
    np.testing.assert_array_equal(i.view(np.uint32) if i.dtype != np.uint32 else i, want[1], err_msg=f"ids {what}")
    np.testing.assert_array_equal(d.view(np.uint32), want[0].view(np.uint32), err_msg=f"dist bits {what}")


def build(capi, X, lab, ids, n_buckets=ur.L, layers=None, **kw):
    idx = capi.Index(0, **kw)
    if layers is not None:
        idx.set_mlp(layers)
    idx.set_buckets(np.ascontiguousarray(X), lab, n_buckets, ids=np.ascontiguousarray(ids, dtype=np.uint32))
    return idx


_idx, _ref = {}, {}


@pytest.fixture(scope="module")
def index_of(capi):
    """One built index per (d, metric) of union_ref.case, with a random root model so that lmi_search_union can run on it."""
    def get(d, metric):
        if (d, metric) not in _idx:
            X, Q, lab, ids = ur.case(d)
            _idx[(d, metric)] = build(capi, X, lab, ids, layers=ur.layers_for(d, ur.L, 3), metric=metric)
            assert np.array_equal(_idx[(d, metric)].bucket_sizes(), ur.SIZES)
        return _idx[(d, metric)]
    yield get
    for h in _idx.values():
        h.close()
    _idx.clear()


def reference(oracle, d, order, k, metric, key=None):
    """union_ref on union_ref.case(d); computed once per key and shared."""
    if key is None or key not in _ref:
        X, Q, lab, ids = ur.case(d)
        rows, labs = ur.buckets_of(X, lab, ids)
        out = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
        for a in out:
            a.setflags(write=False)
        if key is None:
            return out
        _ref[key] = out
    return _ref[key]


@pytest.mark.parametrize("k", ur.KS)
@pytest.mark.parametrize("nb", ur.NBS)
@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_scan_union_parity(capi, index_of, oracle, d, metric, nb, k):
    """The main grid: d = 45 element loads, 64 vector loads, 136 a pitch that is no multiple of 32; a random order with -1 slots."""
    order = ur.random_order(nb)
    assert (order < 0).any()
    want = reference(oracle, d, order, k, metric, key=("main", d, metric, nb, k))
    got = index_of(d, metric).scan_union(ur.case(d)[1], order, k)
    same(got, want, f"d={d} {metric} nb={nb} k={k}")
    plan = capi.union_last_plan()
    assert plan["VEC_ROWS"] == (0 if (d == 45 and metric == "ip") else 1) and plan["LISTS_PER_QUERY"] == nb and plan["LIST_ROWS"] >= k


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("k", [10, 25, 100])
def test_ties_are_ordered_by_rank_then_row(capi, oracle, metric, k):
    """40 copies of one vector over three buckets and queries equal to it: k = 10 cuts the first bucket's copies, 25 the second's,
    100 contains them all -- the copies come first, by (rank, row)."""
    d = 64
    X, Q, lab, ids, order = ur.tie_case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    want = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])   # the copies' ids by (rank, row)
    assert tied.size == 40
    m = min(k, 40)
    np.testing.assert_array_equal(want[1][:4, :m], np.broadcast_to(tied[:m], (4, m)))   # the case still has its ties
    idx = build(capi, X, lab, ids, metric=metric)
    got = idx.scan_union(Q, order, k)
    idx.close()
    same(got, want, f"ties {metric} k={k}")
    np.testing.assert_array_equal(got[1][:4, :m], np.broadcast_to(tied[:m], (4, m)))
    assert np.all(got[0][:4, :m].view(np.uint32) == got[0][0, 0].view(np.uint32))   # one score, bit for bit


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("bucket", [1, 2, 0])
def test_short_unions_pad_and_count(index_of, oracle, metric, bucket):
    """nb = 1 on the 1-row, the 33-row and an empty bucket with k = 100: counts = the bucket's size, +inf / 0 behind."""
    d = 64
    order = np.full((ur.NQ, 1), bucket, dtype=np.int32)
    want = reference(oracle, d, order, 100, metric)
    n = ur.SIZES[bucket]
    assert np.all(want[2] == n) and np.all(np.isposinf(want[0][:, n:])) and np.all(want[1][:, n:] == 0)
    got = index_of(d, metric).scan_union(ur.case(d)[1], order, 100)
    same(got, want, f"short {metric} bucket {bucket}")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_a_nan_row_is_never_returned(capi, oracle, metric):
    d = 45
    X, Q, lab, ids, row = ur.nan_case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    order = np.tile(np.asarray([3, 4], dtype=np.int32), (ur.NQ, 1))
    want = ur.union_ref(oracle, rows, labs, order, Q, 1024, metric)
    assert not np.any(want[1] == ids[row]) and not np.any(np.isnan(want[0]))
    idx = build(capi, X, lab, ids, metric=metric)
    got = idx.scan_union(Q, order, 1024)
    idx.close()
    same(got, want, f"nan {metric}")
    assert not np.any(got[1] == ids[row])


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_k10_one_bucket_equals_lmi_scan_topk(index_of, d, metric):
    """For a query whose bucket holds at least 10 rows, the union of one bucket at k = 10 is what the bucket scan returns."""
    order = ur.random_order(1, seed=3, holes=False)
    idx = index_of(d, metric)
    Q = ur.case(d)[1]
    ds, is_ = idx.scan_topk(Q, order, 10)
    du, iu, cu = idx.scan_union(Q, order, 10)
    full = np.asarray(ur.SIZES)[order[:, 0]] >= 10
    assert full.sum() >= 100 and np.all(cu[full] == 10)
    np.testing.assert_array_equal(iu[full], is_[full])
    np.testing.assert_array_equal(du[full].view(np.uint32), ds[full].view(np.uint32))


@pytest.mark.parametrize("metric", ur.METRICS)
def test_forced_geometry_changes_nothing(capi, index_of, oracle, metric):
    """32 queries per group and a 64-KiB slab: several groups, several waves, the same bits as the automatic geometry."""
    d, nb, k = 64, 8, 129
    order = ur.random_order(nb)
    want = reference(oracle, d, order, k, metric, key=("main", d, metric, nb, k))
    idx, Q = index_of(d, metric), ur.case(d)[1]
    try:
        capi.union_set_geometry(0, 0)
        auto = idx.scan_union(Q, order, k)
        auto_plan = capi.union_last_plan()
        capi.union_set_geometry(32, 64 << 10)
        forced = idx.scan_union(Q, order, k)
        plan = capi.union_last_plan()
    finally:
        capi.union_set_geometry(0, 0)
    same(auto, want, "automatic")
    same(forced, want, "forced")
    assert auto_plan["GROUPS"] == 1 and auto_plan["WAVES"] == 1 and auto_plan["QUERY_ROWS"] == ur.NQ
    assert plan["GROUPS"] == 5 and plan["QUERY_ROWS"] == 32 and plan["WAVES"] > 1 and plan["LIST_ROWS"] == 256
    assert plan["WORKSPACE_BYTES"] < auto_plan["WORKSPACE_BYTES"]


@pytest.mark.parametrize("metric", ur.METRICS)
def test_search_union_with_the_stops(index_of, oracle, metric):
    """lmi_search_union equals the reference applied to the bucket order it returns -- with a row budget, and with a probability mass
    as well; either way some slots are -1, and the order is lmi_mlp_topk's under the same settings."""
    d, nb, k = 64, 8, 100
    idx = index_of(d, metric)
    Q = ur.case(d)[1]
    for rows, mass in ((1500, 0.0), (3000, 0.6)):
        idx.set_stop_rows(rows)
        idx.set_stop_mass(mass)
        try:
            dd, ii, cc, bo = idx.search_union(Q, Q, nb, k)
            np.testing.assert_array_equal(bo, idx.mlp_topk(Q, nb))
        finally:
            idx.set_stop_rows(0)
            idx.set_stop_mass(0.0)
        assert (bo < 0).any() and (bo[:, 0] >= 0).all(), (rows, mass)
        same((dd, ii, cc), reference(oracle, d, bo, k, metric), f"search_union {metric} rows={rows} mass={mass}")
    dd, ii, cc, bo = idx.search_union(Q, Q, nb, k)   # and with no stop: nothing is cut
    assert (bo >= 0).all()
    same((dd, ii, cc), reference(oracle, d, bo, k, metric), f"search_union {metric}")


def tree_index(capi, metric="ip"):
    """A 2-level [4, 3] tree with random models over synthetic_tree's objects, by the C ABI alone: model 0 the root, model 1 + i the
    node of root class i, slab bucket 3 * i + j the leaf (i, j)."""
    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    idx = capi.Index(0, metric=metric)
    idx.set_mlp(root)
    for i, (_, layers) in enumerate(internal):
        idx.nav_set_model(i + 1, layers)
    idx.nav_set_tree([0, 4, 7, 10, 13, 16], [1, 2, 3, 4] + [-1] * 12, [-2] * 4 + list(range(12)))
    lab = dp[:, 0] * 3 + dp[:, 1]
    ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    idx.set_buckets(Xs, lab, 12, ids=ids)
    return idx, Xs, lab, ids, Qn, Qs


@pytest.mark.parametrize("metric", ur.METRICS)
def test_search_tree_union(capi, oracle, metric):
    idx, Xs, lab, ids, Qn, Qs = tree_index(capi, metric)
    rows, labs = ur.buckets_of(Xs, lab, ids, 12)
    try:
        for nb, k, path_mass in ((5, 100, 0.0), (7, 1024, 0.0), (7, 100, 0.9)):
            idx.set_path_mass(path_mass)
            dd, ii, cc, slab, ent = idx.search_tree_union(Qn, Qs, nb, k)
            want_slab, want_ent = idx.nav_order(Qn, nb)
            np.testing.assert_array_equal(slab, want_slab)
            np.testing.assert_array_equal(ent, want_ent)
            assert path_mass == 0 or (slab < 0).any()
            same((dd, ii, cc), ur.union_ref(oracle, rows, labs, slab, Qs, k, metric), f"tree {metric} nb={nb} k={k} mass={path_mass}")
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_device_pointers_equal_host_pointers(index_of, metric):
    d, nb, k = 136, 3, 129
    idx, Q = index_of(d, metric), ur.case(d)[1]
    order = ur.random_order(nb)
    host = idx.scan_union(Q, order, k)
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(order).cuda()
    d_t = torch.empty((ur.NQ, k), dtype=torch.float32, device="cuda")
    i_t = torch.empty((ur.NQ, k), dtype=torch.int32, device="cuda")
    c_t = torch.empty((ur.NQ,), dtype=torch.int32, device="cuda")
    idx.scan_union_device(q_t, bo_t, nb, k, d_t, i_t, c_t)
    same((d_t, i_t, c_t), host, "scan_union_device")
    hs = idx.search_union(Q, Q, nb, k)
    d_t.fill_(0), i_t.fill_(0), c_t.fill_(0)
    bo_o = torch.empty((ur.NQ, nb), dtype=torch.int32, device="cuda")
    idx.search_union_device(q_t, q_t, nb, k, d_t, i_t, c_t, bo_o)
    same((d_t, i_t, c_t), hs, "search_union_device")
    np.testing.assert_array_equal(bo_o.cpu().numpy(), hs[3])
    d_t.fill_(0), i_t.fill_(0)
    idx.search_union_device(q_t, q_t, nb, k, d_t, i_t)   # counts and the order declined
    same((d_t, i_t, torch.from_numpy(hs[2])), hs, "search_union_device without counts")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_clone_view_and_subset_answer_like_a_fresh_build(capi, index_of, oracle, metric):
    d, nb, k = 64, 3, 100
    X, Q, lab, ids = ur.case(d)
    order = ur.random_order(nb)
    idx = index_of(d, metric)
    view = idx.clone_view()
    same(view.scan_union(Q, order, k), reference(oracle, d, order, k, metric, key=("main", d, metric, nb, k)), "clone view")
    view.close()
    keep = np.flatnonzero(np.arange(ur.N) % 3 != 0)
    sub = idx.subset(ids[keep])
    fresh = build(capi, X[keep], lab[keep], ids[keep], metric=metric)
    try:
        rows, labs = ur.buckets_of(X[keep], lab[keep], ids[keep])
        want = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
        same(sub.scan_union(Q, order, k), want, "subset")
        same(sub.clone_view().scan_union(Q, order, k), want, "a clone view of the subset")
        same(fresh.scan_union(Q, order, k), want, "fresh build")
    finally:
        sub.close()
        fresh.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_after_insert_and_delete(capi, oracle, metric):
    """After insert + delete the union scan answers like a fresh build of the surviving + inserted objects (bucket order: survivors
    in their order, then the inserted ones)."""
    d, nb, k = 45, 3, 100
    X, Q, lab, ids = ur.case(d)
    first = np.arange(ur.N) < 5000
    gone = ids[np.flatnonzero(first)[::7]]
    idx = build(capi, X[first], lab[first], ids[first], metric=metric)
    try:
        assert idx.insert(np.ascontiguousarray(X[~first]), lab[~first], ids[~first]) == 1000
        assert idx.delete(gone) == gone.size
        alive = ~np.isin(ids, gone)
        rows, labs = ur.buckets_of(X[alive], lab[alive], ids[alive])   # object order = survivors of the build, then the inserted
        for b in range(ur.L):
            r, i = idx.read_bucket(b)
            np.testing.assert_array_equal(i, labs[b])
        order = ur.random_order(nb)
        same(idx.scan_union(Q, order, k), ur.union_ref(oracle, rows, labs, order, Q, k, metric), f"mutated {metric}")
    finally:
        idx.close()


def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


def test_li_api_one_level(oracle):
    """li.LearnedIndex.search(merge="union") at k = 100 on a 1-level index: the reference on the engine's bucket order."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    root, _, _, dp2, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    rs = np.random.RandomState(2)
    dp = rs.randint(0, 4, size=(Xn.shape[0], 1)).astype(np.int64)
    li = LearnedIndex(net_from(root), {}, [(b,) for b in range(4)])
    for metric in ur.METRICS:
        dists, nns, _ = li.search(frame(Xn), Qn, frame(Xs), Qs, dp, [4], n_buckets=3, k=100, metric=metric, merge="union", stop_rows=1800)
        eng = li._engine
        eng.set_stop_rows(1800)
        bo = eng.mlp_topk(Qn, 3)
        eng.set_stop_rows(0)
        assert (bo < 0).any()
        rows, labs = ur.buckets_of(Xs, dp[:, 0], np.arange(1, Xs.shape[0] + 1), 4)
        want = ur.union_ref(oracle, rows, labs, bo, Qs, 100, metric)
        assert dists.dtype == np.float64 and dists.shape == nns.shape == (Qn.shape[0], 100)
        np.testing.assert_array_equal(nns, want[1])
        np.testing.assert_array_equal(dists.astype(np.float32).view(np.uint32), want[0].view(np.uint32))
        d2, n2, _ = li.search_resident(Qn, Qs, [4], n_buckets=3, k=100, merge="union", stop_rows=1800)
        np.testing.assert_array_equal(n2, nns)
        # the default is untouched: k <= 20 and ten per bucket
        d10, n10, _ = li.search_resident(Qn, Qs, [4], n_buckets=3, k=10)
        assert n10.shape == (Qn.shape[0], 10)
        with pytest.raises(AssertionError):
            li.search_resident(Qn, Qs, [4], n_buckets=3, k=100)
    with pytest.raises(ValueError, match="merge"):
        li.search_resident(Qn, Qs, [4], n_buckets=3, k=10, merge="best")


def test_li_api_two_levels(oracle):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    dists, nns, _ = li.search(frame(Xn), Qn, frame(Xs), Qs, dp, [4, 3], n_buckets=5, k=100, merge="union")
    slab, _ = li._engine.nav_order(Qn, 5)
    n_slab = len(li._path_ids)
    lab = np.asarray([li._path_ids[tuple(int(v) for v in p)] for p in dp])
    rows, labs = ur.buckets_of(Xs, lab, np.arange(1, Xs.shape[0] + 1), n_slab)
    want = ur.union_ref(oracle, rows, labs, slab, Qs, 100, "ip")
    assert dists.shape == nns.shape == (Qn.shape[0], 100)
    np.testing.assert_array_equal(nns, want[1])
    np.testing.assert_array_equal(dists.astype(np.float32).view(np.uint32), want[0].view(np.uint32))


def test_refusals(capi):
    X, Q, lab, ids = ur.case(64)
    order = ur.random_order(3)
    for kw, word in ((dict(prefilter=False), "row-major"), (dict(storage="f16"), "row-major")):
        Xh = X.astype(np.float16).astype(np.float32) if "storage" in kw else X
        idx = build(capi, Xh, lab, ids, layers=ur.layers_for(64, ur.L, 3), **kw)
        try:
            with pytest.raises(capi.LmiError, match=word):
                idx.scan_union(Q, order, 10)
            with pytest.raises(capi.LmiError, match=word):
                idx.search_union(Q, Q, 3, 10)
            d, i = idx.scan_topk(Q, np.abs(order), 10)   # and the ordinary scan still answers
            assert d.shape == (ur.NQ, 10)
        finally:
            idx.close()
    idx = capi.Index(0)
    try:
        with pytest.raises(capi.LmiError, match="not built"):
            idx.scan_union(Q, order, 10)
        d = np.empty((ur.NQ, 1025), np.float32)
        i = np.empty((ur.NQ, 1025), np.uint32)
        for k in (0, 1025):   # past the Python check, at the C ABI
            idx2 = build(capi, X, lab, ids)
            rc = capi.lib().lmi_scan_union(idx2._h, Q.ctypes.data, ur.NQ, order.ctypes.data, 3, k, d.ctypes.data, i.ctypes.data, None, 0)
            assert rc != 0 and b"outside [1,1024]" in capi.lib().lmi_last_error()
            assert capi.lib().lmi_scan_union(idx2._h, Q.ctypes.data, ur.NQ, order.ctypes.data, 3, 10, None, i.ctypes.data, None, 0) != 0
            assert b"NULL" in capi.lib().lmi_last_error()
            assert capi.lib().lmi_scan_union(idx2._h, Q.ctypes.data, 0, order.ctypes.data, 3, 10, None, None, None, 0) == 0   # nq == 0
            idx2.close()
            with pytest.raises(ValueError):
                idx.scan_union(Q, order, k)
        assert capi.union_last_plan()["GROUPS"] == 0
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_an_ordinary_search_is_unchanged_by_a_union_call(index_of, metric):
    d, nb = 64, 4
    idx, Q = index_of(d, metric), ur.case(d)[1]
    before = idx.search(Q, Q, nb, 10, want_keys=True)
    idx.search_union(Q, Q, nb, 1024)
    idx.scan_union(Q, ur.random_order(8), 129)
    after = idx.search(Q, Q, nb, 10, want_keys=True)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
