"""CPU (`-m "not gpu"`): the host side of lmi_knn_range.  The two entry points are exported and bound and the plan words follow the
header; `_capi.range_knn` refuses bad arguments before the library is loaded; the call's host arithmetic (csrc/lmi_knn_range_plan.h,
pure host code) passes its stand-alone self-test under AddressSanitizer + UBSan; the prefix reference of tests/knn_range_ref.py
equals the range search's own reference where k = nb is affordable; the radius recipe has, on the oracle, the properties
tests/test_gpu_knn_range.py relies on; and the driver's `range_recall` does its set arithmetic."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import knn_cases as kc
import knn_range_ref as kr
from learnedmetricindex_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_range_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in (("lmi_knn_range", 11), ("lmi_debug_knn_range_plan", 2)):
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    words = re.findall(r"\bLMI_KNN_RANGE_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", header)
    assert words[-1] == "COUNT" and list(_capi.KNN_RANGE_PLAN_FIELDS) == words[:-1] and len(words) == 9


def test_range_knn_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    q, x = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    for args, kw in (((q, x, 0.5), dict(metric="cosine")), ((q.astype(np.float64), x, 0.5), {}), ((q, x.astype(np.float16), 0.5), {}),
                     ((q, x[:, :7], 0.5), {}), ((q[0], x, 0.5), {}), ((q.tolist(), x, 0.5), {}), ((q, None, 0.5), {}), ((q, x, None), {}),
                     ((q, x, np.zeros(4, np.float32)), {}), ((q, x, np.zeros((3, 1), np.float32)), {}), ((q, x, "far"), {}),
                     ((q, x, 0.5), dict(max_total=-1)), ((q, x, 0.5), dict(max_total=1.5)), ((q, x, 0.5), dict(max_total=True)),
                     ((np.zeros((1, 4097), np.float32), np.zeros((1, 4097), np.float32), 0.5), {}),
                     ((np.zeros((1, 0), np.float32), np.zeros((1, 0), np.float32), 0.5), {})):
        with pytest.raises(ValueError):
            _capi.range_knn(*args, **kw)

    class FakeTensor:   # a torch tensor beside a numpy array: both must be of one kind
        dtype, ndim, shape, is_cuda = "torch.float32", 2, (5, 8), True

        def data_ptr(self):
            return 0

    with pytest.raises(ValueError, match="both"):
        _capi.range_knn(q, FakeTensor(), 0.5)
    with pytest.raises(ValueError, match="both"):
        _capi.range_knn(FakeTensor(), x, 0.5)


def test_knn_range_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "knn_range_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "knn_range_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "knn range plan selftest: clean" in r.stdout


@pytest.mark.parametrize("metric", kc.METRICS)
def test_the_prefix_reference_equals_the_whole_base_reference(oracle, metric):
    """A base of 1500 rows: more than the 1024 entries of the truth, few enough for the oracle at k = nb."""
    xq, xb = kc.case(*kc.SHAPES[0])
    xq, xb = np.ascontiguousarray(xq[:24]), np.ascontiguousarray(xb[:1500])
    with np.errstate(all="ignore"):
        D, I = (oracle.knn_ip if metric == "ip" else oracle.knn_l2)(xq, xb, kr.K)
    j = np.asarray(kr.RECIPE_J)[np.arange(24) % 4]
    radius = kr.dists_of(D, metric)[np.arange(24), j]
    got = kr.prefix_ref(D, I, radius, metric)
    want = kr.whole_base_ref(oracle, xq, xb, radius, metric)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.all(np.diff(got[0]) >= j + 1) and got[0][-1] > 24
    # a radius that admits the last entry is refused by the helper, not answered short
    with pytest.raises(AssertionError, match="cut short"):
        kr.prefix_ref(D, I, np.full(24, np.inf, np.float32), metric)
    # NaN and -inf admit nothing
    lims, dd, ii = kr.prefix_ref(D, I, np.where(np.arange(24) % 2 == 0, np.nan, -np.inf).astype(np.float32), metric)
    assert np.all(lims == 0) and dd.size == 0 and ii.size == 0


@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("shape", kc.SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_the_radius_recipe(oracle, shape, metric):
    """At most 708 admitted per query (j = 700 and what ties with it), entry 1023 never admitted (asserted by the helper, and seen here
    again), every radius is some row's distance -- so dist == radius is exercised on every query -- and the tie queries admit exactly
    the 52-row tie group at j = 0."""
    nq, nb, d = shape
    radius, (lims, dd, ii) = kr.recipe(oracle, shape, metric)
    xq, xb = kc.case(*shape)
    D, _ = kc.truth(oracle, shape, xq, xb, kr.K, metric)
    n = np.diff(lims)
    j = np.asarray(kr.RECIPE_J)[np.arange(nq) % 4]
    assert radius.shape == (nq,) and np.all(np.isfinite(radius)) and not radius.flags.writeable
    assert np.all(n >= j + 1) and n.max() <= 708 and n.max() > 700
    assert np.all(kr.dists_of(D, metric)[:, kr.K - 1] > radius)
    g = kc.tie_group(nb)
    for q in range(nq):
        a, b = lims[q], lims[q + 1]
        assert np.all(np.diff(ii[a:b].astype(np.int64)) > 0)                  # ascending rows
        assert np.any(dd[a:b].view(np.uint32) == radius[q:q + 1].view(np.uint32))   # the radius is met exactly
    for q in range(0, kc.TIE_QUERIES, 4):   # j = 0
        a, b = lims[q], lims[q + 1]
        np.testing.assert_array_equal(ii[a:b], g.astype(np.uint32))
        assert np.all(dd[a:b].view(np.uint32) == dd[a].view(np.uint32))
    for q in range(1, kc.TIE_QUERIES, 4):   # j = 9 lies inside the tie group: the same 52
        assert lims[q + 1] - lims[q] == 52


def _driver(monkeypatch):
    spec = importlib.util.spec_from_file_location("lmi_search_driver_knn_range", os.path.join(ROOT, "learnedmetricindex_amd", "search.py"))
    drv = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "lmi_search_driver_knn_range", drv)   # dataclasses resolves the module of Experiment
    spec.loader.exec_module(drv)
    return drv


def test_range_recall_on_hand_made_arrays(monkeypatch):
    rec = _driver(monkeypatch).range_recall
    lims_t, ids_t = np.array([0, 3, 3, 5]), np.array([1, 2, 3, 7, 8])
    assert rec(lims_t, ids_t, lims_t, ids_t) == 1.0
    assert rec([0, 0, 0, 0], [], lims_t, ids_t) == 0.0                                 # nothing found
    assert rec([0, 2, 4, 5], [4, 5, 1, 2, 9], lims_t, ids_t) == 0.0                    # disjoint, query by query: 1, 2 belong to query 0
    assert rec([0, 2, 2, 3], [1, 9, 8], lims_t, ids_t) == pytest.approx(2 / 5)         # partial
    assert rec([0, 4, 4, 6], [3, 3, 3, 1, 7, 7], lims_t, ids_t) == pytest.approx(3 / 5)   # duplicates in found count once
    assert rec([0, 1, 1], [5], [0, 0, 0], []) == 1.0                                   # empty truth
    assert rec([0, 0], np.zeros(0, np.uint32), [0], np.zeros(0, np.uint32)) == 1.0     # no queries
    # found covers more queries than the truth (the driver's truth is the first 1000): the first ones are compared
    assert rec([0, 3, 3, 5, 9], [1, 2, 3, 7, 8, 1, 1, 1, 1], lims_t, ids_t) == 1.0
    # the id types of the two sides differ (uint32 from the library, int64 from a frame's index)
    assert rec(lims_t, ids_t.astype(np.uint32), lims_t, ids_t.astype(np.int64)) == 1.0


def test_driver_reports_range_recall_only_with_eval(monkeypatch):
    """`range_truth` asks `range_knn` for the first 1000 queries over the scan vectors as they are and maps rows to ids through the
    frame's index (against a stand-in for the binding: no GPU call is made)."""
    import pandas as pd

    drv = _driver(monkeypatch)
    asked = []

    class FakeResult:
        lims = np.array([0, 2, 2, 3], dtype=np.int64)

        def read(self):
            return np.zeros(3, np.float32), np.array([0, 4, 2], dtype=np.uint32)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            asked.append("closed")

    def fake_range_knn(xq, xb, radius, metric="ip", max_total=0, device=0):
        asked.append((xq.shape, xb.shape, radius, metric, xq.dtype, xb.dtype))
        return FakeResult()

    monkeypatch.setattr(drv._capi, "range_knn", fake_range_knn)
    objects = pd.DataFrame(np.full((5, 4), 2.0, np.float32))   # not unit rows: they go to the call as they are
    objects.index = [11, 12, 13, 14, 15]
    queries = np.zeros((3, 4), np.float32)
    lims, ids = drv.range_truth(queries, objects, 0.25)
    assert asked == [((3, 4), (5, 4), 0.25, "ip", np.float32, np.float32), "closed"]
    np.testing.assert_array_equal(lims, [0, 2, 2, 3])
    np.testing.assert_array_equal(ids, [11, 15, 13])
    assert drv.range_recall([0, 1, 1, 2], [15, 13], lims, ids) == pytest.approx(2 / 3)
    drv.range_truth(np.zeros((1500, 4), np.float32), objects, 0.5)
    assert asked[2][0] == (1000, 4)


def test_baseline_range_search_routes(monkeypatch):
    """`Baseline.range_search`: unit rows, the inner product, ids 1-based; `sort=True` sorts through a temporary Index on the device."""
    from learnedmetricindex_amd.li import Baseline as mod

    seen = []

    class FakeResult:
        lims = np.array([0, 1, 3], dtype=np.int64)

        def sort(self, index):
            seen.append(("sort", index))

        def read(self):
            return np.array([0.5, 0.25, 0.125], np.float32), np.array([4, 0, 2], dtype=np.uint32)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            seen.append("closed")

    class FakeIndex:
        def __init__(self, device):
            seen.append(("index", device))

        def close(self):
            seen.append("index closed")

    def fake_range_knn(xq, xb, radius, metric="ip", max_total=0, device=0):
        seen.append((np.linalg.norm(xq, axis=1), np.linalg.norm(xb, axis=1), radius, metric, max_total, device))
        return FakeResult()

    monkeypatch.setattr(mod._capi, "range_knn", fake_range_knn)
    monkeypatch.setattr(mod._capi, "Index", FakeIndex)
    rs = np.random.RandomState(0)
    X, Q = rs.randn(5, 8).astype(np.float32) * 3, rs.randn(2, 8).astype(np.float32) * 7
    lims, d, ids, secs = mod.Baseline().range_search(Q, X, 0.3, max_total=9)
    qn, xn, radius, metric, max_total, device = seen[0]
    np.testing.assert_allclose(qn, 1, atol=1e-6)
    np.testing.assert_allclose(xn, 1, atol=1e-6)
    assert (radius, metric, max_total, device) == (0.3, "ip", 9, 0) and seen[1:] == ["closed"] and secs >= 0
    np.testing.assert_array_equal(lims, [0, 1, 3])
    np.testing.assert_array_equal(ids, [5, 1, 3])
    assert ids.dtype == np.int64 and d.dtype == np.float32
    del seen[:]
    mod.Baseline().range_search(Q, X, 0.3, sort=True, device=0)
    assert [s if isinstance(s, str) else s[0] for s in seen[1:]] == ["index", "sort", "index closed", "closed"]
