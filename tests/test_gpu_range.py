"""GPU (`-m gpu`): the range search (lmi_scan_range, lmi_search_range, lmi_search_tree_range; include/lmi_hip.h) -- per query every
object of its visited buckets within a radius, in ordinal order -- against the unchanged CPU oracle.

Every comparison is exact: lims and ids with array_equal, dists as uint32 bit patterns, against tests/range_ref.py (the contract in
numpy on oracle.knn_ip / oracle.knn_l2).  The shapes are the union tests' (tests/union_ref.py: N = 6000 in 12 buckets of 0 to 2003
rows, 150 queries); tests/test_range_host.py checks on the oracle alone that the radius recipe has the properties relied on here."""
import numpy as np
import pandas as pd
import pytest
import torch

import range_ref as rr
import union_filter_ref as fr
import union_parts_ref as upr
import union_ref as ur
from path_mass_ref import synthetic_tree

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
# a fixed radius on union_ref.case's unit vectors: cos >= 0.2 (IP 1 - cos, L2 2 - 2 cos) -- about one candidate in twenty at d = 64
FIXED = {"ip": 0.8, "l2": 1.6}


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def same(got, want, what=""):
    lims, d, i = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got[:3])
    np.testing.assert_array_equal(lims, want[0], err_msg=f"lims {what}")
    assert lims.dtype == np.int64 and d.dtype == np.float32 and d.shape == i.shape == (int(want[0][-1]),), what
    np.testing.assert_array_equal(i.view(np.uint32), want[2], err_msg=f"ids {what}")
    np.testing.assert_array_equal(d.view(np.uint32), want[1].view(np.uint32), err_msg=f"dist bits {what}")


def build(capi, X, lab, ids, n_buckets=ur.L, layers=None, **kw):
    idx = capi.Index(0, **kw)
    if layers is not None:
        idx.set_mlp(layers)
    idx.set_buckets(np.ascontiguousarray(X), lab, n_buckets, ids=np.ascontiguousarray(ids, dtype=np.uint32))
    return idx


_idx = {}


@pytest.fixture(scope="module")
def index_of(capi):
    """One built index per (d, metric) of union_ref.case, with a random root model so that lmi_search_range can run on it."""
    def get(d, metric):
        if (d, metric) not in _idx:
            X, Q, lab, ids = ur.case(d)
            _idx[(d, metric)] = build(capi, X, lab, ids, layers=ur.layers_for(d, ur.L, 3), metric=metric)
        return _idx[(d, metric)]
    yield get
    for h in _idx.values():
        h.close()
    _idx.clear()


def reference(oracle, d, order, radius, metric, allowed=None, filter_of=None):
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    return rr.range_ref(oracle, rows, labs, order, Q, radius, metric, allowed, filter_of)


@pytest.mark.parametrize("nb", ur.NBS)
@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_scan_range_parity(capi, index_of, oracle, d, metric, nb):
    """The main grid with the recipe's radii: every finite radius is some candidate's distance, so dist == radius is exercised on
    every such query; the others get +inf (everything) or visit nothing."""
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    want = rr.recipe_ref(oracle, d, nb, metric)
    got = index_of(d, metric).scan_range(ur.case(d)[1], order, radius)
    same(got, want, f"d={d} {metric} nb={nb}")
    plan = capi.range_last_plan()
    assert plan["GROUPS"] == 1 and plan["QUERY_ROWS"] == ur.NQ and plan["RESULTS"] == want[0][-1] and plan["CHUNK_BYTES"] == 8 * want[0][-1]
    assert np.all(np.diff(got[0])[:4] == 0)   # queries that visit nothing: flat lims


@pytest.mark.parametrize("metric", ur.METRICS)
def test_a_fixed_radius_returns_long_uneven_runs(index_of, oracle, metric):
    d, nb = 64, 3   # (three ranks: some queries see the large buckets, some only small ones)
    order = ur.random_order(nb)
    radius = FIXED[metric]
    want = reference(oracle, d, order, radius, metric)
    n = np.diff(want[0])   # on the oracle: the longest run holds 301 results, the shortest non-empty one 29, 30 531 in all
    assert n.max() > 200 and n[n > 0].min() < n.max() // 4 and want[0][-1] > 10000
    same(index_of(d, metric).scan_range(ur.case(d)[1], order, radius), want, f"fixed {metric}")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_infinity_returns_the_buckets_themselves(index_of, metric):
    """+inf on query 4: more than 1024 results -- which no other call returns -- equal to the concatenated bucket ids."""
    d, nb = 64, 3
    idx, Q = index_of(d, metric), ur.case(d)[1]
    order = ur.random_order(nb)
    lims, dd, ii = idx.scan_range(Q[4:5], order[4:5], INF)
    want = np.concatenate([idx.read_bucket(int(b))[1] for b in order[4] if b >= 0])
    assert lims[1] > 1024 and np.array_equal(ii, want) and np.all(np.isfinite(dd))


@pytest.mark.parametrize("metric", ur.METRICS)
def test_nan_and_minus_infinity_admit_nothing(index_of, oracle, metric):
    d, nb = 45, 3
    idx, Q = index_of(d, metric), ur.case(d)[1]
    order = ur.random_order(nb)
    radius = np.full(ur.NQ, INF, dtype=np.float32)
    radius[5::3] = np.nan
    radius[6::3] = -np.inf
    want = reference(oracle, d, order, radius, metric)
    n = np.diff(want[0])
    assert np.all(n[5::3] == 0) and np.all(n[6::3] == 0) and np.all(n[:4] == 0) and n[4] > 1024 and n[4::3].sum() > n[4]
    same(idx.scan_range(Q, order, radius), want, f"nan / -inf {metric}")
    empty = idx.scan_range(Q, order, np.nan)
    assert np.all(empty[0] == 0) and empty[1].size == 0 and empty[2].size == 0


@pytest.mark.parametrize("metric", ur.METRICS)
def test_ties_come_back_in_rank_then_row_order(capi, oracle, metric):
    """Radius = the tie vector's own distance: all 40 copies, by (rank, row), and nothing else."""
    d = 64
    X, Q, lab, ids, order = ur.tie_case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    r0 = ur.union_ref(oracle, rows, labs, order[:1], Q[:1], 1, metric)[0][0, 0]
    radius = np.full(ur.NQ, r0, dtype=np.float32)
    want = rr.range_ref(oracle, rows, labs, order, Q, radius, metric)
    assert np.all(np.diff(want[0])[:4] == 40)
    idx = build(capi, X, lab, ids, metric=metric)
    got = idx.scan_range(Q, order, radius)
    idx.close()
    same(got, want, f"ties {metric}")
    for q in range(4):
        np.testing.assert_array_equal(got[2][got[0][q]: got[0][q + 1]], tied)


def test_two_scores_of_one_distance_are_both_admitted(capi, oracle):
    """Scores 2^-30 and 2^-31 both give the distance 1.0f: radius 1.0f admits both, in ordinal order."""
    rows, ids, order, q, _ = upr.collapse_case()
    X, lab, idv = np.concatenate(rows), np.repeat(np.arange(2), [r.shape[0] for r in rows]), np.concatenate(ids)
    want = rr.range_ref(oracle, rows, ids, order, q, 1.0, "ip")
    assert list(want[2]) == [102, 203] and np.all(want[1].view(np.uint32) == np.float32(1.0).view(np.uint32))
    idx = build(capi, X, lab, idv, n_buckets=2)
    try:
        same(idx.scan_range(q, order, np.float32(1.0)), want, "collapse")
        assert idx.scan_range(q, order, np.nextafter(np.float32(1.0), np.float32(0.0)))[0][-1] == 0
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_a_nan_row_is_never_returned(capi, oracle, metric):
    d = 45
    X, Q, lab, ids, row = ur.nan_case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    order = np.tile(np.asarray([3, 4], dtype=np.int32), (ur.NQ, 1))[:20]
    want = rr.range_ref(oracle, rows, labs, order, Q[:20], INF, metric)
    assert np.all(np.diff(want[0]) == 257 + 2003 - 1) and not np.any(want[2] == ids[row])
    idx = build(capi, X, lab, ids, metric=metric)
    got = idx.scan_range(Q[:20], order, INF)
    idx.close()
    same(got, want, f"nan row {metric}")
    assert not np.any(got[2] == ids[row]) and not np.any(np.isnan(got[1]))


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_against_the_union_scan(index_of, d, metric):
    """Radius = scan_union's 10th distance: the stably distance-sorted run begins with the union's ten ids (the recipe shows on the
    oracle that no two candidates share a distance there)."""
    nb = 3
    idx, Q = index_of(d, metric), ur.case(d)[1]
    order = ur.random_order(nb)
    du, iu, cu = idx.scan_union(Q, order, 10)
    full = cu == 10
    assert full.sum() >= 140
    radius = np.where(full, du[:, 9], -INF).astype(np.float32)
    lims, dd, ii = idx.scan_range(Q, order, radius)
    ds, is_ = rr.stable_by_distance(lims, dd, ii)
    for q in np.flatnonzero(full):
        assert lims[q + 1] - lims[q] == 10, q
        np.testing.assert_array_equal(is_[lims[q]: lims[q] + 10], iu[q])
        np.testing.assert_array_equal(ds[lims[q]: lims[q] + 10].view(np.uint32), du[q].view(np.uint32))
    assert np.all(np.diff(lims)[~full] == 0)


@pytest.mark.parametrize("metric", ur.METRICS)
def test_forced_geometry_changes_nothing(capi, index_of, oracle, metric):
    """32 queries per group and a 256-KiB slab: several groups, several waves, the same bits as the automatic geometry."""
    d, nb = 64, 8
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    want = rr.recipe_ref(oracle, d, nb, metric)
    idx, Q = index_of(d, metric), ur.case(d)[1]
    try:
        capi.union_set_geometry(0, 0)
        auto = idx.scan_range(Q, order, radius)
        auto_plan = capi.range_last_plan()
        capi.union_set_geometry(32, 256 << 10)
        forced = idx.scan_range(Q, order, radius)
        plan = capi.range_last_plan()
        capi.union_set_geometry(7, 4096)
        tiny = idx.scan_range(Q, order, radius)
        tiny_plan = capi.range_last_plan()
    finally:
        capi.union_set_geometry(0, 0)
    same(auto, want, "automatic")
    same(forced, want, "forced")
    same(tiny, want, "7 queries per group, one tile per wave")
    assert auto_plan["GROUPS"] == 1 and auto_plan["WAVES"] == 1 and auto_plan["QUERY_ROWS"] == ur.NQ
    assert plan["GROUPS"] == 5 and plan["QUERY_ROWS"] == 32 and plan["WAVES"] > 1 and plan["SLAB_BYTES"] < auto_plan["SLAB_BYTES"]
    assert tiny_plan["GROUPS"] == 22 and tiny_plan["QUERY_ROWS"] == 7
    for p in (auto_plan, plan, tiny_plan):
        assert p["RESULTS"] == want[0][-1] and p["CHUNK_BYTES"] == 8 * want[0][-1] and p["WORKSPACE_BYTES"] > 0


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_shared_filters(capi, index_of, oracle, metric):
    """The five filters of union_filter_ref with filter_of cycling -1, 0..4: the reference is the buckets with their disallowed rows
    out of the candidates; filter 3 keeps nothing, so every sixth query is emptied by its filter."""
    d, nb = 64, 8
    idx, Q = index_of(d, metric), ur.case(d)[1]
    order = ur.random_order(nb)
    allowed, fo = fr.case_allowed(d), fr.filter_of()
    filt = capi.Filter(idx, fr.filter_lists(d), fr.MODES)
    try:
        for radius in (INF, FIXED[metric]):
            want = reference(oracle, d, order, radius, metric, allowed, fo)
            n = np.diff(want[0])
            assert np.all(n[fo == 3] == 0) and n[fo == 4].max() > 0
            same(idx.scan_range(Q, order, radius, filter=filt, filter_of=fo), want, f"filters {metric} r={radius}")
        one = reference(oracle, d, order, INF, metric, allowed[:1], None)   # filter_of = None: every query uses filter 0
        same(idx.scan_range(Q, order, INF, filter=filt), one, "filter 0 for all")
        try:
            capi.union_set_geometry(32, 256 << 10)
            want = reference(oracle, d, order, INF, metric, allowed, fo)
            same(idx.scan_range(Q, order, INF, filter=filt, filter_of=fo), want, "filters, forced geometry")
        finally:
            capi.union_set_geometry(0, 0)
    finally:
        filt.close()


def test_union_and_range_sit_on_one_candidate_stage(capi, index_of):
    """A filtered union scan (k = 10) and a filtered range search have lists of 128 rows both, so the one stage they share cuts the
    same batch into the same groups and waves with the same slab: several of each under the forced geometry, on device pointers."""
    d, nb, metric = 64, 8, "l2"
    idx, Q = index_of(d, metric), ur.case(d)[1]
    fo = fr.filter_of()
    filt = capi.Filter(idx, fr.filter_lists(d), fr.MODES)
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(ur.random_order(nb))).cuda()
    d_t = torch.empty((ur.NQ, 10), dtype=torch.float32, device="cuda")
    i_t = torch.empty((ur.NQ, 10), dtype=torch.int32, device="cuda")
    try:
        capi.union_set_geometry(32, 256 << 10)
        idx.scan_union_device(q_t, bo_t, nb, 10, d_t, i_t, filter=filt, filter_of=fo)
        union_plan = capi.union_last_plan()
        with idx.scan_range_device(q_t, bo_t, nb, FIXED[metric], filter=filt, filter_of=fo):
            range_plan = capi.range_last_plan()
    finally:
        capi.union_set_geometry(0, 0)
        filt.close()
    assert union_plan["LIST_ROWS"] == 128
    for word in ("GROUPS", "QUERY_ROWS", "WAVES", "SLAB_BYTES"):
        assert union_plan[word] == range_plan[word], (word, union_plan, range_plan)
    assert union_plan["GROUPS"] == 5 and union_plan["QUERY_ROWS"] == 32 and union_plan["WAVES"] > 1 and union_plan["SLAB_BYTES"] > 0


@pytest.mark.parametrize("metric", ur.METRICS)
def test_search_range_with_the_stops(index_of, oracle, metric):
    """lmi_search_range equals the reference applied to the bucket order it returns, and that order is lmi_search_union's."""
    d, nb = 64, 8
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius = FIXED[metric]
    for rows, mass in ((1500, 0.0), (3000, 0.6), (0, 0.0)):
        idx.set_stop_rows(rows)
        idx.set_stop_mass(mass)
        try:
            lims, dd, ii, bo = idx.search_range(Q, Q, nb, radius)
            np.testing.assert_array_equal(bo, idx.search_union(Q, Q, nb, 10)[3])
        finally:
            idx.set_stop_rows(0)
            idx.set_stop_mass(0.0)
        assert (rows == 0) != bool((bo < 0).any()), (rows, mass)
        same((lims, dd, ii), reference(oracle, d, bo, radius, metric), f"search_range {metric} rows={rows} mass={mass}")


def tree_index(capi, metric="ip"):
    """test_gpu_union.tree_index: a 2-level [4, 3] tree with random models over synthetic_tree's objects, by the C ABI alone."""
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


def tree_radius(oracle, rows, labs, slab, Qs, metric):
    """One radius per query: its 30th distance in the union of its buckets (+inf where it has fewer)."""
    dd, _, cc = ur.union_ref(oracle, rows, labs, slab, Qs, 30, metric)
    return np.where(cc == 30, dd[:, 29], INF).astype(np.float32)


@pytest.mark.parametrize("metric", ur.METRICS)
def test_search_tree_range(capi, oracle, metric):
    idx, Xs, lab, ids, Qn, Qs = tree_index(capi, metric)
    rows, labs = ur.buckets_of(Xs, lab, ids, 12)
    try:
        for nb, path_mass in ((5, 0.0), (7, 0.9)):
            idx.set_path_mass(path_mass)
            want_slab, want_ent = idx.search_tree_union(Qn, Qs, nb, 10)[3:]
            radius = tree_radius(oracle, rows, labs, want_slab, Qs, metric)
            lims, dd, ii, slab, ent = idx.search_tree_range(Qn, Qs, nb, radius)
            np.testing.assert_array_equal(slab, want_slab)
            np.testing.assert_array_equal(ent, want_ent)
            assert path_mass == 0 or (slab < 0).any()
            same((lims, dd, ii), rr.range_ref(oracle, rows, labs, slab, Qs, radius, metric), f"tree {metric} nb={nb} mass={path_mass}")
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_device_pointers_equal_host_pointers(capi, index_of, oracle, metric):
    d, nb = 136, 3
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    host = idx.scan_range(Q, order, radius)
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(order)).cuda()
    with idx.scan_range_device(q_t, bo_t, nb, radius) as res:
        assert res.total == host[0][-1]
        d_t = torch.zeros(res.total, dtype=torch.float32, device="cuda")
        i_t = torch.zeros(res.total, dtype=torch.int32, device="cuda")
        res.read_into(d_t, i_t)
        same((res.lims, d_t, i_t), host, "scan_range_device, read_into")
        same((res.lims,) + res.read(), host, "scan_range_device, read")
    with pytest.raises(ValueError, match="closed"):
        res.read()
    hs = idx.search_range(Q, Q, nb, radius)
    bo_o = torch.empty((ur.NQ, nb), dtype=torch.int32, device="cuda")
    with idx.search_range_device(q_t, q_t, nb, radius, bo_o) as res:
        same((res.lims,) + res.read(), hs, "search_range_device")
    np.testing.assert_array_equal(bo_o.cpu().numpy(), hs[3])
    with idx.search_range_device(q_t, q_t, nb, radius) as res:   # the order declined
        same((res.lims,) + res.read(), hs, "search_range_device without the order")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_clone_view_and_subset(capi, index_of, oracle, metric):
    d, nb = 64, 3
    X, Q, lab, ids = ur.case(d)
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    idx = index_of(d, metric)
    view = idx.clone_view()
    same(view.scan_range(Q, order, radius), rr.recipe_ref(oracle, d, nb, metric), "clone view")
    view.close()
    keep = np.flatnonzero(np.arange(ur.N) % 3 != 0)
    sub = idx.subset(ids[keep])
    try:
        rows, labs = ur.buckets_of(X[keep], lab[keep], ids[keep])
        same(sub.scan_range(Q, order, radius), rr.range_ref(oracle, rows, labs, order, Q, radius, metric), "subset")
    finally:
        sub.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_after_insert_and_delete(capi, oracle, metric):
    d, nb = 45, 3
    X, Q, lab, ids = ur.case(d)
    first = np.arange(ur.N) < 5000
    gone = ids[np.flatnonzero(first)[::7]]
    idx = build(capi, X[first], lab[first], ids[first], metric=metric)
    try:
        assert idx.insert(np.ascontiguousarray(X[~first]), lab[~first], ids[~first]) == 1000
        assert idx.delete(gone) == gone.size
        alive = ~np.isin(ids, gone)
        rows, labs = ur.buckets_of(X[alive], lab[alive], ids[alive])   # object order = survivors of the build, then the inserted
        radius, order = rr.recipe_radii(oracle, d, nb, metric)          # (radii of the whole case: a spread of run lengths here too)
        same(idx.scan_range(Q, order, radius), rr.range_ref(oracle, rows, labs, order, Q, radius, metric), f"mutated {metric}")
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_max_total(capi, index_of, oracle, metric):
    """At the exact total the call succeeds; one below it fails, naming the count, and leaves no result -- and the handle answers
    lmi_search and lmi_scan_union as before."""
    d, nb = 64, 3
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    want = rr.recipe_ref(oracle, d, nb, metric)
    total = int(want[0][-1])
    before = idx.search(Q, Q, nb, 10, want_keys=True) + idx.scan_union(Q, order, 100)
    same(idx.scan_range(Q, order, radius, max_total=total), want, "at the exact total")
    with pytest.raises(capi.LmiError, match=rf"max_total = {total - 1} results: {total} had been counted"):
        idx.scan_range(Q, order, radius, max_total=total - 1)
    assert capi.range_last_plan()["GROUPS"] == 0
    try:
        capi.union_set_geometry(32, 256 << 10)   # several groups and waves: it stops at the first wave that passes the limit
        with pytest.raises(capi.LmiError, match=r"max_total = 500 results: \d+ had been counted") as e:
            idx.scan_range(Q, order, radius, max_total=500)
        counted = int(str(e.value).split("results: ")[1].split(" ")[0])
        assert 500 < counted < total
        same(idx.scan_range(Q, order, radius, max_total=total), want, "forced geometry, at the exact total")
    finally:
        capi.union_set_geometry(0, 0)
    with pytest.raises(capi.LmiError, match="max_total"):
        idx.search_range(Q, Q, nb, INF, max_total=1)
    res = capi._vp(1)   # a failed call leaves *result NULL, at the C ABI
    r32 = np.ascontiguousarray(radius)
    rc = capi.lib().lmi_scan_range(idx._h, Q.ctypes.data, ur.NQ, order.ctypes.data, nb, r32.ctypes.data, None, None, 1, res, 0)
    assert rc != 0 and not res.value
    after = idx.search(Q, Q, nb, 10, want_keys=True) + idx.scan_union(Q, order, 100)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals(capi):
    X, Q, lab, ids = ur.case(64)
    order = ur.random_order(3)
    lib = capi.lib()
    err = lambda: lib.lmi_last_error().decode()
    for kw in (dict(prefilter=False), dict(storage="f16")):
        Xh = X.astype(np.float16).astype(np.float32) if "storage" in kw else X
        idx = build(capi, Xh, lab, ids, layers=ur.layers_for(64, ur.L, 3), **kw)
        try:
            with pytest.raises(capi.LmiError, match="row-major"):
                idx.scan_range(Q, order, 0.5)
            with pytest.raises(capi.LmiError, match="row-major"):
                idx.search_range(Q, Q, 3, 0.5)
            d, i = idx.scan_topk(Q, np.abs(order), 10)   # and the ordinary scan still answers
            assert d.shape == (ur.NQ, 10)
        finally:
            idx.close()
    idx = capi.Index(0)
    try:
        with pytest.raises(capi.LmiError, match="not built"):
            idx.scan_range(Q, order, 0.5)
    finally:
        idx.close()
    idx = build(capi, X, lab, ids, layers=ur.layers_for(64, ur.L, 3))
    other = build(capi, X, lab, ids)
    filt = capi.Filter(other, fr.filter_lists(64), fr.MODES)
    mine = capi.Filter(idx, fr.filter_lists(64), fr.MODES)
    radius = np.full(ur.NQ, 0.5, np.float32)
    wide = np.zeros((ur.NQ, 1025), np.int32)

    def scan(nq=ur.NQ, bo=order, nb=3, r=radius, f=None, fo=None, max_total=0, res=True):
        out = capi._vp()
        rc = lib.lmi_scan_range(idx._h, Q.ctypes.data, nq, bo.ctypes.data, nb, None if r is None else r.ctypes.data, f, fo, max_total,
                                out if res else None, 0)
        assert rc == 0 or not out.value
        return rc, out

    try:
        for nb in (0, 1025):   # past the Python check, at the C ABI
            assert scan(bo=wide, nb=nb)[0] != 0 and "n_buckets" in err()
        assert scan(r=None)[0] != 0 and "radius is NULL" in err()
        assert scan(res=False)[0] != 0 and "result pointer is NULL" in err()
        assert scan(max_total=-1)[0] != 0 and "negative" in err()
        assert scan(f=filt._f)[0] != 0 and "stale" in err()                       # a foreign filter
        bad_fo = np.full(ur.NQ, fr.NF, np.int32)
        assert scan(f=mine._f, fo=bad_fo.ctypes.data)[0] != 0 and "filter_of" in err()
        assert scan(fo=bad_fo.ctypes.data)[0] != 0 and "without a filter" in err()
        assert capi.range_last_plan()["GROUPS"] == 0
        rc, out = scan(nq=0)                                                       # nq == 0: an empty result
        assert rc == 0 and out.value
        with capi.RangeResult(out, 0) as res:
            assert res.total == 0 and list(res.lims) == [0] and res.read()[0].size == 0
        assert idx.insert(np.ascontiguousarray(X[:5]), lab[:5], np.arange(5, dtype=np.uint32)) == 5
        with pytest.raises(capi.LmiError, match="stale"):                         # a layout change makes the filter stale
            idx.scan_range(Q, order, 0.5, filter=mine)
        with pytest.raises(capi.LmiError, match="stale"):
            idx.search_range(Q, Q, 3, 0.5, filter=mine)
    finally:
        filt.close()
        mine.close()
        other.close()
        idx.close()


def test_a_result_outlives_its_handle(capi, oracle):
    d, nb, metric = 64, 3, "ip"
    X, Q, lab, ids = ur.case(d)
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    idx = build(capi, X, lab, ids)
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(order)).cuda()
    res = idx.scan_range_device(q_t, bo_t, nb, radius)
    idx.close()
    try:
        same((res.lims,) + res.read(), rr.recipe_ref(oracle, d, nb, metric), "after the handle's close()")
    finally:
        res.close()
    res.close()   # twice: nothing


def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


def test_li_api_one_level(oracle):
    """li.LearnedIndex.range_search on a 1-level index: the reference on the engine's bucket order; sort=True; a filter list."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    root, _, _, dp2, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    rs = np.random.RandomState(2)
    dp = rs.randint(0, 4, size=(Xn.shape[0], 1)).astype(np.int64)
    all_ids = np.arange(1, Xs.shape[0] + 1)
    rows, labs = ur.buckets_of(Xs, dp[:, 0], all_ids, 4)
    li = LearnedIndex(net_from(root), {}, [(b,) for b in range(4)])
    try:
        with pytest.raises(ValueError, match="storage"):
            li.range_search(frame(Xn), Qn, frame(Xs), Qs, dp, [4], 0.5, storage="f16")
        assert li._engine is None   # refused before any work
        for metric in ur.METRICS:
            li.prepare(frame(Xn), frame(Xs), dp, [4], metric=metric)
            eng = li._engine
            eng.set_stop_rows(1800)
            bo = eng.mlp_topk(Qn, 3)
            eng.set_stop_rows(0)
            assert (bo < 0).any()
            radius = tree_radius(oracle, rows, labs, bo, Qs, metric)
            want = rr.range_ref(oracle, rows, labs, bo, Qs, radius, metric)
            lims, dists, nns, clock = li.range_search(frame(Xn), Qn, frame(Xs), Qs, dp, [4], radius, n_buckets=3, metric=metric, stop_rows=1800)
            assert dists.dtype == np.float64 and nns.dtype == np.uint32 and clock["search"] > 0 and eng.stop_rows == 0
            same((lims, dists.astype(np.float32), nns), want, f"li {metric}")
            ls, ds, ns, _ = li.range_search_resident(Qn, Qs, [4], radius, n_buckets=3, sort=True, stop_rows=1800)
            wd, wi = rr.stable_by_distance(*want)
            same((ls, ds.astype(np.float32), ns), (want[0], wd, wi), f"li sorted {metric}")
            assert all(np.all(np.diff(ds[ls[q]: ls[q + 1]]) >= 0) for q in range(Qn.shape[0]))
            keep = all_ids[::3]
            allowed = fr.allowed_rows([keep], [fr.KEEP], labs)
            lf, df_, nf, _ = li.range_search_resident(Qn, Qs, [4], radius, n_buckets=3, stop_rows=1800, filter=keep)
            same((lf, df_.astype(np.float32), nf), rr.range_ref(oracle, rows, labs, bo, Qs, radius, metric, allowed, None), f"li filter {metric}")
            total = int(want[0][-1])
            with pytest.raises(Exception, match="max_total"):
                li.range_search_resident(Qn, Qs, [4], radius, n_buckets=3, stop_rows=1800, max_total=total - 1)
    finally:
        li.close()


def test_li_api_two_levels(oracle, monkeypatch):
    """A [4, 3] index, walked in pieces of 64 queries whose lims are joined."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    try:
        li.prepare(frame(Xn), frame(Xs), dp, [4, 3])
        slab, _ = li._engine.nav_order(Qn, 5)
        lab = np.asarray([li._path_ids[tuple(int(v) for v in p)] for p in dp])
        rows, labs = ur.buckets_of(Xs, lab, np.arange(1, Xs.shape[0] + 1), len(li._path_ids))
        radius = tree_radius(oracle, rows, labs, slab, Qs, "ip")
        want = rr.range_ref(oracle, rows, labs, slab, Qs, radius, "ip")
        same_li = lambda got, w, what: same((got[0], got[1].astype(np.float32), got[2]), w, what)
        same_li(li.range_search(frame(Xn), Qn, frame(Xs), Qs, dp, [4, 3], radius, n_buckets=5), want, "two levels")
        assert Qn.shape[0] > 64
        monkeypatch.setattr(LearnedIndex, "_nav_chunk", lambda self: 64)
        same_li(li.range_search_resident(Qn, Qs, [4, 3], radius, n_buckets=5), want, "two levels, in pieces")
        wd, wi = rr.stable_by_distance(*want)
        same_li(li.range_search_resident(Qn, Qs, [4, 3], radius, n_buckets=5, sort=True), (want[0], wd, wi), "two levels, sorted")
        same_li(li.range_search_resident(Qn, Qs, [4, 3], radius, n_buckets=5, max_total=int(want[0][-1])), want, "at the exact total")
        with pytest.raises(Exception, match="max_total"):
            li.range_search_resident(Qn, Qs, [4, 3], radius, n_buckets=5, max_total=int(want[0][-1]) - 1)
    finally:
        li.close()
