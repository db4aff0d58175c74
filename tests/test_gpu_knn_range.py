"""GPU (`-m gpu`): lmi_knn_range, the exact brute-force range query over a whole base (include/lmi_hip.h), against the unchanged CPU
oracle.

Every comparison is exact: lims and ids with array_equal, dists as uint32 bit patterns.  The references are tests/knn_range_ref.py
(the prefix of the oracle's k = 1024 truth, for the shapes of tests/knn_cases.py) and tests/range_ref.py with the whole base as one
bucket (k = nb, small bases); tests/test_knn_range_host.py checks on the oracle alone that the recipe has the properties relied on
here."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import knn_cases as kc
import knn_range_ref as kr
import range_ref as rr
import union_ref as ur
from learnedmetricindex_amd import _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)
SHAPE_IDS = dict(ids=lambda s: "x".join(map(str, s)))


def read(res):
    """(lims, dists, ids) of a RangeResult, which is closed."""
    with res:
        return (res.lims,) + res.read()


def same(got, want, what=""):
    lims, d, i = (np.ascontiguousarray(a) for a in got[:3])
    np.testing.assert_array_equal(lims, want[0], err_msg=f"lims {what}")
    assert lims.dtype == np.int64 and d.dtype == np.float32 and i.dtype == np.uint32 and d.shape == i.shape == (int(want[0][-1]),), what
    np.testing.assert_array_equal(i, want[2], err_msg=f"ids {what}")
    np.testing.assert_array_equal(d.view(np.uint32), want[1].view(np.uint32), err_msg=f"dist bits {what}")


def on_device(*arrays):
    return tuple(torch.from_numpy(np.array(a, order="C")).cuda() for a in arrays)


def plan_is_zero():
    return all(v == 0 for v in _capi.knn_range_last_plan().values())


@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("shape", kc.SHAPES, **SHAPE_IDS)
def test_parity_with_the_reference(oracle, shape, metric):
    """The recipe's radii -- every one some row's distance, so dist == radius is met on every query -- and two more queries whose
    radii are NaN and -inf."""
    xq, xb = kc.case(*shape)
    radius, ref = kr.recipe(oracle, shape, metric)
    xq2, r2, want = kr.with_empty_queries(xq, radius, ref)
    res = _capi.range_knn(xq2, xb, r2, metric)
    counts = res.pair_counts()
    got = read(res)
    same(got, want, f"{shape} {metric}")
    lims, dd, ii = got
    assert lims[-1] == lims[-2] == lims[-3]   # the NaN and the -inf radius: empty runs
    np.testing.assert_array_equal(counts, np.diff(lims).astype(np.int32)[:, None])   # nb = 1: the per-query totals
    g = kc.tie_group(shape[1]).astype(np.uint32)
    for q in (0, 1, 4, 5):   # j = 0 and j = 9: the tie group, ascending, one distance bit pattern
        a, b = lims[q], lims[q + 1]
        np.testing.assert_array_equal(ii[a:b], g)
        assert np.all(dd[a:b].view(np.uint32) == dd[a].view(np.uint32))
    plan = _capi.knn_range_last_plan()
    assert plan["RESULTS"] == lims[-1] and plan["CHUNK_BYTES"] == 8 * lims[-1] and plan["QUERY_GROUPS"] == 1 and plan["WORKSPACE_BYTES"] > 0
    assert plan["PIECES"] == -(-shape[1] // plan["PIECE_ROWS"]) and plan["QUERY_ROWS"] == shape[0] + 2


@pytest.mark.parametrize("geometry", kc.GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
@pytest.mark.parametrize("shape", [kc.SHAPES[0], kc.SHAPES[1]], **SHAPE_IDS)
def test_forced_geometry_changes_nothing(oracle, shape, geometry):
    """Pieces, splits and query groups with ragged ends, from host arrays and from device tensors: the automatic result, the forced
    result and the reference are one."""
    xq, xb = kc.case(*shape)
    nq, nb, d = shape
    piece, splits, qrows = geometry
    dq, db = on_device(xq, xb)
    try:
        for metric in kc.METRICS:
            radius, want = kr.recipe(oracle, shape, metric)
            _capi.knn_set_geometry(0, 0, 0)
            auto_host = read(_capi.range_knn(xq, xb, radius, metric))
            auto_dev = read(_capi.range_knn(dq, db, radius, metric))
            _capi.knn_set_geometry(*geometry)
            for kind, q, x, auto in (("host", xq, xb, auto_host), ("device", dq, db, auto_dev)):
                got = read(_capi.range_knn(q, x, radius, metric))
                plan = _capi.knn_range_last_plan()
                what = f"{shape} {metric} {geometry} {kind}"
                same(got, want, what)
                same(got, auto, what + " vs automatic")
                rows = piece if kind == "host" else min(piece, nb)
                assert plan["PIECE_ROWS"] == rows and plan["PIECES"] == -(-nb // rows), (what, plan)
                assert plan["SPLITS"] == splits, (what, plan)
                if qrows:
                    assert plan["QUERY_ROWS"] == min(qrows, nq) and plan["QUERY_GROUPS"] == -(-nq // min(qrows, nq)), (what, plan)
                else:
                    assert plan["QUERY_GROUPS"] == 1, (what, plan)
                assert plan["RESULTS"] == want[0][-1] and plan["CHUNK_BYTES"] == 8 * want[0][-1], (what, plan)
    finally:
        _capi.knn_set_geometry(0, 0, 0)


@pytest.mark.parametrize("metric", kc.METRICS)
def test_infinity_returns_every_admissible_row(oracle, metric):
    """+inf on a small base: every row, in row order, with the distances the oracle gives at k = nb -- also under splits and pieces
    whose stretches start at no multiple of 64."""
    xq, xb = kc.case(40, 777, 45, seed=5)
    want = kr.whole_base_ref(oracle, xq, xb, INF, metric)
    assert np.array_equal(np.diff(want[0]), np.full(40, 777)) and np.array_equal(want[2], np.tile(np.arange(777, dtype=np.uint32), 40))
    same(read(_capi.range_knn(xq, xb, INF, metric)), want, f"+inf {metric}")
    same(read(_capi.range_knn(*on_device(xq, xb), INF, metric)), want, f"+inf {metric} device")
    try:
        _capi.knn_set_geometry(300, 7, 33)
        same(read(_capi.range_knn(xq, xb, INF, metric)), want, f"+inf {metric} forced")
        assert _capi.knn_range_last_plan()["PIECES"] == 3 and _capi.knn_range_last_plan()["QUERY_GROUPS"] == 2
    finally:
        _capi.knn_set_geometry(0, 0, 0)


@pytest.mark.parametrize("metric", kc.METRICS)
def test_special_values_do_what_the_oracle_does(oracle, metric):
    """A NaN row, a row with +inf, a row whose squared norm is subnormal, an all-zero query: under +inf the result is whatever the
    oracle's chain admits; the NaN row never is."""
    xq, xb = kc.special()
    with np.errstate(all="ignore"):
        want = kr.whole_base_ref(oracle, xq, xb, INF, metric)
    got = read(_capi.range_knn(xq, xb, INF, metric))
    same(got, want, f"special {metric}")
    lims, dd, ii = got
    assert not np.any(ii == 3) and not np.any(np.isnan(dd))
    for q in range(xq.shape[0]):   # the +inf row and the subnormal-norm row are there exactly where the oracle has them
        for row in (5, 7):
            assert (row in ii[lims[q]:lims[q + 1]]) == (row in want[2][want[0][q]:want[0][q + 1]]), (q, row)
    assert np.all(np.diff(lims) >= 1997)
    same(read(_capi.range_knn(*on_device(xq, xb), INF, metric)), want, f"special {metric} device")
    # a finite radius on the same base
    with np.errstate(all="ignore"):
        D, _ = kc.truth(oracle, "special", xq, xb, 64, metric)
        radius = kr.dists_of(D, metric)[:, 20].copy()
        want = kr.whole_base_ref(oracle, xq, xb, radius, metric)
    same(read(_capi.range_knn(xq, xb, radius, metric)), want, f"special {metric} finite")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_agrees_with_the_range_search_of_an_index(metric):
    """A built index scanned with an order that lists every bucket sees the whole base: per query the set of (id, distance bits) is
    lmi_knn_range's, rows mapped to ids.  Both are held to the same oracle chains, so the bits agree."""
    d = 45
    X, Q, lab, ids = ur.case(d)
    radius = {"ip": 0.8, "l2": 1.6}[metric]
    idx = _capi.Index(0, metric=metric)
    try:
        idx.set_buckets(np.ascontiguousarray(X), lab, ur.L, ids=np.ascontiguousarray(ids, dtype=np.uint32))
        order = np.ascontiguousarray(np.tile(np.arange(ur.L, dtype=np.int32), (ur.NQ, 1)))
        il, idd, iid = idx.scan_range(Q, order, radius)[:3]
    finally:
        idx.close()
    kl, kdd, krow = read(_capi.range_knn(np.ascontiguousarray(Q), np.ascontiguousarray(X), radius, metric))
    np.testing.assert_array_equal(il, kl)
    assert kl[-1] > 1000
    kid = np.asarray(ids, dtype=np.uint32)[krow]
    for q in range(ur.NQ):
        a, b = kl[q], kl[q + 1]
        assert set(zip(iid[a:b].tolist(), idd[a:b].view(np.uint32).tolist())) == set(zip(kid[a:b].tolist(), kdd[a:b].view(np.uint32).tolist())), q


@pytest.mark.parametrize("metric", kc.METRICS)
def test_sort_by_distance(oracle, metric):
    shape = kc.SHAPES[0]
    xq, xb = kc.case(*shape)
    radius, ref = kr.recipe(oracle, shape, metric)
    want_d, want_i = rr.stable_by_distance(*ref)
    idx = _capi.Index(0)
    try:
        with _capi.range_knn(xq, xb, radius, metric) as res:
            assert not res.sorted
            res.sort(idx)
            assert res.sorted
            same((res.lims,) + res.read(), (ref[0], want_d, want_i), f"sorted {metric}")
    finally:
        idx.close()


@pytest.mark.parametrize("metric", kc.METRICS)
def test_max_total(oracle, metric):
    shape = kc.SHAPES[0]
    xq, xb = kc.case(*shape)
    radius, want = kr.recipe(oracle, shape, metric)
    total = int(want[0][-1])
    try:
        _capi.knn_set_geometry(4096, 2, 32)   # several pieces and groups: the count is tested after each
        with pytest.raises(_capi.LmiError, match=r"lmi_knn_range: more than max_total = %d results: (\d+) had been counted" % (total - 1)) as e:
            _capi.range_knn(xq, xb, radius, metric, max_total=total - 1)
        assert int(str(e.value).split("results: ")[1].split()[0]) == total   # the excess shows at the last piece of the last group
        assert plan_is_zero()
        with pytest.raises(_capi.LmiError, match="had been counted"):
            _capi.range_knn(xq, xb, radius, metric, max_total=1)
        same(read(_capi.range_knn(xq, xb, radius, metric, max_total=total)), want, f"max_total = total {metric}")   # the next call works
        assert _capi.knn_range_last_plan()["RESULTS"] == total
        same(read(_capi.range_knn(*on_device(xq, xb), radius, metric, max_total=total + 1)), want, f"max_total = total + 1 {metric}")
    finally:
        _capi.knn_set_geometry(0, 0, 0)
    # the library itself: the result pointer comes back NULL
    import ctypes

    res = ctypes.c_void_p(7)
    r = np.ascontiguousarray(radius)
    rc = _capi.lib().lmi_knn_range(0, xq.ctypes.data, xq.shape[0], xb.ctypes.data, xb.shape[0], xb.shape[1], _capi.KNN_METRICS[metric],
                                   r.ctypes.data, total - 1, ctypes.byref(res), 0)
    assert rc != 0 and res.value is None


def test_refusals_and_empty_cases():
    import ctypes

    xq, xb = kc.case(*kc.SHAPES[0])
    nq, nb, d = xq.shape[0], xb.shape[0], xq.shape[1]
    dq, db = on_device(xq, xb)
    for a, b in ((xq, db), (dq, xb)):   # mixed kinds
        with pytest.raises(ValueError):
            _capi.range_knn(a, b, 0.5)
    L = _capi.lib()
    q, x = xq.ctypes.data, xb.ctypes.data
    radius = np.full(nq, 0.5, np.float32)
    r = radius.ctypes.data
    read(_capi.range_knn(xq[:3], xb[:100], INF))
    assert not plan_is_zero()
    # (xq, nq, xb, nb, d, metric, radius, max_total), the message
    for args, msg in (((q, nq, x, nb, 0, 0, r, 0), b"lmi_knn_range: d 0 outside [1,4096]"),
                      ((q, 1, x, 1, 4097, 0, r, 0), b"lmi_knn_range: d 4097 outside [1,4096]"),
                      ((q, -1, x, nb, d, 0, r, 0), b"lmi_knn_range: nq -1 outside [0, 2^31)"),
                      ((q, 1 << 31, x, nb, d, 0, r, 0), b"lmi_knn_range: nq 2147483648 outside [0, 2^31)"),
                      ((q, nq, x, -1, d, 0, r, 0), b"lmi_knn_range: nb -1 outside [0, 2^31)"),
                      ((q, nq, x, 1 << 31, d, 0, r, 0), b"lmi_knn_range: nb 2147483648 outside [0, 2^31)"),
                      ((q, nq, x, nb, d, 7, r, 0), b"lmi_knn_range: unknown metric 7"),
                      ((q, nq, x, nb, d, 0, None, 0), b"lmi_knn_range: radius is NULL"),
                      ((None, nq, x, nb, d, 0, r, 0), b"lmi_knn_range: xq must not be NULL"),
                      ((q, nq, None, nb, d, 0, r, 0), b"lmi_knn_range: xb must not be NULL"),
                      ((q, nq, x, nb, d, 0, r, -1), b"lmi_knn_range: max_total -1 is negative")):
        res = ctypes.c_void_p(7)
        assert L.lmi_knn_range(0, *args, ctypes.byref(res), 0) != 0, args
        assert L.lmi_last_error() == msg, (args, L.lmi_last_error())
        assert res.value is None and plan_is_zero(), args
        read(_capi.range_knn(xq[:3], xb[:100], INF))   # the next call works and reports its plan
        assert not plan_is_zero()
    assert L.lmi_knn_range(0, q, nq, x, nb, d, 0, r, 0, None, 0) != 0
    assert L.lmi_last_error() == b"lmi_knn_range: the result pointer is NULL" and plan_is_zero()
    # nq == 0: an empty result, whatever else is NULL; the plan words stay zero
    for xq0, xb0 in ((xq[:0], xb), (dq[:0], db)):
        res = _capi.range_knn(xq0, xb0, 0.5)
        assert res.nq == 0 and res.total == 0 and np.array_equal(res.lims, [0]) and res.pair_counts().shape == (0, 1)
        dd, ii = res.read()
        assert dd.size == 0 and ii.size == 0 and plan_is_zero()
        res.close()
    res = ctypes.c_void_p(7)
    assert L.lmi_knn_range(0, None, 0, None, nb, d, 0, None, 0, ctypes.byref(res), 0) == 0 and res.value is not None
    L.lmi_range_result_destroy(res)
    # nb == 0: lims all zero
    for xq0, xb0 in ((xq, xb[:0]), (dq, db[:0])):
        for metric in kc.METRICS:
            res = _capi.range_knn(xq0, xb0, INF, metric)
            assert res.total == 0 and np.array_equal(res.lims, np.zeros(nq + 1, np.int64)) and not np.any(res.pair_counts())
            plan = _capi.knn_range_last_plan()
            assert plan["PIECES"] == 0 and plan["RESULTS"] == 0 and plan["QUERY_GROUPS"] >= 1
            res.close()
    res = ctypes.c_void_p(7)
    assert L.lmi_knn_range(0, q, nq, None, 0, d, 0, r, 0, ctypes.byref(res), 0) == 0 and res.value is not None   # a NULL xb with nb == 0
    L.lmi_range_result_destroy(res)
    assert L.lmi_debug_knn_range_plan(None, 8) != 0


def test_baseline_range_search():
    """li.Baseline.range_search on the data of test_gpu_knn.test_baseline_beyond_k_10: the cosine distances within a radius, ids
    1-based, against float64 -- away from the radius by more than the binary32 error of a unit-row product (2e-6, as there)."""
    from learnedmetricindex_amd.li.Baseline import Baseline

    rs = np.random.RandomState(3)
    X = rs.randn(3000, 48).astype(np.float32) * rs.uniform(0.1, 10, size=(3000, 1)).astype(np.float32)
    Q = rs.randn(64, 48).astype(np.float32)
    xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    qn = Q / np.linalg.norm(Q, axis=1, keepdims=True)
    ref = 1 - qn.astype(np.float64) @ xn.astype(np.float64).T
    radius = 0.7
    lims, d, ids, secs = Baseline().range_search(Q, X, radius)
    assert lims.shape == (65,) and d.shape == ids.shape == (int(lims[-1]),) and secs > 0 and lims[-1] > 64
    for q in range(64):
        got = ids[lims[q]:lims[q + 1]]
        assert np.all(np.diff(got) > 0) and got.min(initial=1) >= 1
        sure_in, sure_out = np.flatnonzero(ref[q] < radius - 2e-6) + 1, np.flatnonzero(ref[q] > radius + 2e-6) + 1
        assert np.all(np.isin(sure_in, got)) and not np.any(np.isin(sure_out, got))
        np.testing.assert_allclose(d[lims[q]:lims[q + 1]], ref[q, got - 1], atol=2e-6)
    lims2, d2, ids2, _ = Baseline().range_search(Q, X, radius, sort=True)
    want_d, want_i = rr.stable_by_distance(lims, d, ids)
    np.testing.assert_array_equal(lims2, lims)
    np.testing.assert_array_equal(ids2, want_i)
    np.testing.assert_array_equal(d2.view(np.uint32), want_d.view(np.uint32))
    with pytest.raises(_capi.LmiError, match="max_total"):
        Baseline().range_search(Q, X, radius, max_total=int(lims[-1]) - 1)


def test_driver_reports_range_recall(monkeypatch, tmp_path):
    """search.py --range-radius --eval on the synthetic source, cut down to 4000 objects and 64 queries: with a budget that covers every
    bucket and no stop the range search sees the whole base, so its recall against lmi_knn_range is 1.0."""
    spec = importlib.util.spec_from_file_location("lmi_search_driver_knn_range_gpu", os.path.join(ROOT, "learnedmetricindex_amd", "search.py"))
    drv = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "lmi_search_driver_knn_range_gpu", drv)
    spec.loader.exec_module(drv)
    monkeypatch.setitem(drv.CARDINALITY, "100K", 4000)
    monkeypatch.setattr(drv, "QUERY_COUNT", 64)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(2023)
    args = ["--dataset", "clip768v2", "--emb", "emb", "--size", "100K", "--synthetic", "--n-categories", "8", "--epochs", "20",
            "--clustering-algorithm", "hip_kmeans", "--trainer", "hip", "-bp", "25", "100", "--save", "", "--range-radius", "0.6"]
    out = drv.run(drv.Experiment.from_argv(args + ["--eval"]))
    assert out["range_recall_8"] == 1.0 and 0.0 < out["range_recall_2"] <= 1.0
    assert out["range_8"][0] > 1.0   # the radius admits something: a recall of 1.0 is not the empty truth's
    assert out["range_2"][0] <= out["range_8"][0]
    plain = drv.run(drv.Experiment.from_argv(args))
    assert not any(str(k).startswith("range_recall") for k in plain) and "range_8" in plain   # without --eval nothing changes
