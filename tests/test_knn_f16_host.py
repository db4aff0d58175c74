"""CPU (`-m "not gpu"`): the host side of lmi_knn_f16 / lmi_knn_range_f16.  The two entry points are declared, exported and bound;
`_capi.knn` / `_capi.range_knn` route by the arrays' precision (against a recording stand-in for the library: no GPU call is made)
and refuse mixed pairs before the library is loaded; the element size of csrc/lmi_knn_plan.h halves the uploaded bytes and changes
nothing else (a stand-alone self-test under AddressSanitizer + UBSan); the driver's `range_truth` hands halves through; and the
inputs of tests/knn_f16_cases.py have, on the oracle alone, the properties tests/test_gpu_knn_f16.py relies on."""
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
import knn_f16_cases as hc
import knn_range_ref as kr
from learnedmetricindex_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f16_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = fh.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, namesake in (("lmi_knn_f16", "lmi_knn"), ("lmi_knn_range_f16", "lmi_knn_range")):
        decl = re.search(r"LMI_API int %s\((.*?)\);" % name, code, flags=re.S)
        assert decl, f"{name} is not declared in include/lmi_hip.h"
        assert re.search(r"const uint16_t \*xq\b.*const uint16_t \*xb\b", decl.group(1), flags=re.S), decl.group(1)
        assert hasattr(L, name), f"{name} is not exported by the built library"
        assert name in _capi.SIGNATURES, f"{name} is not bound"
        assert _capi.SIGNATURES[name] == _capi.SIGNATURES[namesake]   # pointers travel as void*: the same argument list
    # the contract paragraph lists them
    contract = header.split("One contract for every *_f16 entry point")[1].split("*/")[0]
    assert "lmi_knn_f16" in contract and "lmi_knn_range_f16" in contract
    # no new plan word
    assert len(_capi.KNN_PLAN_FIELDS) == 9 and len(_capi.KNN_RANGE_PLAN_FIELDS) == 8


class Recorder:
    """Stands in for the loaded library: every entry point returns 0 and is recorded as (name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call

    def knn_calls(self):
        """the calls of the four ground-truth entry points (a range call also asks its result for the lims)"""
        return [(n, a) for n, a in self.calls if n.startswith("lmi_knn")]


class FakeTensor:
    """What `_capi` asks of a device tensor."""

    ndim, is_cuda, device = 2, True, "cuda:0"

    def __init__(self, dtype, shape, ptr):
        self.dtype, self.shape, self.ptr = dtype, shape, ptr

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return True


def test_knn_routes_by_precision(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    rs = np.random.RandomState(0)
    q32, x32 = rs.randn(4, 8).astype(np.float32), rs.randn(50, 8).astype(np.float32)
    q16, x16 = q32.astype(np.float16), x32.astype(np.float16)
    D, I = _capi.knn(q16, x16, 11, "l2")
    name, args = rec.knn_calls()[-1]
    assert name == "lmi_knn_f16" and D.shape == I.shape == (4, 11) and D.dtype == np.float32 and I.dtype == np.int64
    # (device, xq, nq, xb, nb, d, k, metric, D, I, on_device): the halves' own addresses -- nothing was widened or copied
    assert args[:8] == (0, q16.ctypes.data, 4, x16.ctypes.data, 50, 8, 11, 1) and args[8:] == (D.ctypes.data, I.ctypes.data, 0)
    D, I = _capi.knn(q32, x32, 11, "l2")
    name, args = rec.knn_calls()[-1]
    assert name == "lmi_knn" and args[:8] == (0, q32.ctypes.data, 4, x32.ctypes.data, 50, 8, 11, 1) and args[8:] == (D.ctypes.data, I.ctypes.data, 0)
    res = _capi.range_knn(q16, x16, 0.5, "ip", max_total=9)
    name, args = rec.knn_calls()[-1]
    assert name == "lmi_knn_range_f16" and args[:7] == (0, q16.ctypes.data, 4, x16.ctypes.data, 50, 8, 0) and args[8] == 9 and args[10] == 0
    res._r = None   # (the stand-in made no result: nothing to destroy)
    res = _capi.range_knn(q32, x32, 0.5, "ip", max_total=9)
    name, args = rec.knn_calls()[-1]
    assert name == "lmi_knn_range" and args[:7] == (0, q32.ctypes.data, 4, x32.ctypes.data, 50, 8, 0) and args[8] == 9 and args[10] == 0
    res._r = None
    assert [n for n, _ in rec.knn_calls()] == ["lmi_knn_f16", "lmi_knn", "lmi_knn_range_f16", "lmi_knn_range"]


def test_device_tensors_route_by_precision(monkeypatch):
    torch = pytest.importorskip("torch")
    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    monkeypatch.setattr(_capi, "_sync_device", lambda t: 0)
    made = []

    def fake_empty(shape, dtype=None, device=None):
        made.append((tuple(shape), dtype))
        return FakeTensor(str(dtype), tuple(shape), 4096 * len(made))

    monkeypatch.setattr(torch, "empty", fake_empty)
    for dtype, want in (("torch.float16", "lmi_knn_f16"), ("torch.float32", "lmi_knn")):
        q, x = FakeTensor(dtype, (4, 8), 1026), FakeTensor(dtype, (50, 8), 2050)
        _capi.knn(q, x, 3)
        name, args = rec.knn_calls()[-1]
        assert name == want and args[1] == 1026 and args[3] == 2050 and args[10] == 1
        assert made[-2:] == [((4, 3), torch.float32), ((4, 3), torch.int64)]


def test_mixed_pairs_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    q, x = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    h, g = q.astype(np.float16), x.astype(np.float16)
    t16, t32 = FakeTensor("torch.float16", (5, 8), 0), FakeTensor("torch.float32", (5, 8), 0)
    for a, b in ((q, g), (h, x), (h, x.astype(np.float64)), (q.astype(np.float64), g), (h.astype(np.float64), g.astype(np.float64)),
                 (h, t16), (t16, g), (h, t32), (t32, t16), (t16, t32), (h, g[:, :7]), (h[0], g), (h, None)):
        with pytest.raises(ValueError):
            _capi.knn(a, b)
        with pytest.raises(ValueError):
            _capi.range_knn(a, b, 0.5)
    for a, b in ((h, t16), (t16, g)):   # a half tensor beside a half array: both must be of one kind
        with pytest.raises(ValueError, match="both"):
            _capi.knn(a, b)
        with pytest.raises(ValueError, match="both"):
            _capi.range_knn(a, b, 0.5)
    for kw in (dict(k=0), dict(k=1025), dict(metric="cosine")):   # the namesake's refusals hold for halves
        with pytest.raises(ValueError):
            _capi.knn(h, g, **kw)


def test_knn_f16_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "knn_f16_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "knn_f16_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "knn f16 plan selftest: clean" in r.stdout


def test_driver_range_truth_hands_halves_through(monkeypatch):
    """`range_truth` passes float16 on when the scan frame and the scan queries are both float16, and widens otherwise (against a
    stand-in for the binding: no GPU call is made)."""
    import pandas as pd

    spec = importlib.util.spec_from_file_location("lmi_search_driver_knn_f16", os.path.join(ROOT, "learnedmetricindex_amd", "search.py"))
    drv = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "lmi_search_driver_knn_f16", drv)   # dataclasses resolves the module of Experiment
    spec.loader.exec_module(drv)
    asked = []

    class FakeResult:
        lims = np.array([0, 2, 2, 3], dtype=np.int64)

        def read(self):
            return np.zeros(3, np.float32), np.array([0, 4, 2], dtype=np.uint32)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

    def fake_range_knn(xq, xb, radius, metric="ip", max_total=0, device=0):
        asked.append((xq.dtype, xb.dtype, xq.copy(), xb.copy()))
        return FakeResult()

    monkeypatch.setattr(drv._capi, "range_knn", fake_range_knn)
    x16 = (np.arange(20, dtype=np.float32).reshape(5, 4) / 8).astype(np.float16)
    q16 = (np.arange(12, dtype=np.float32).reshape(3, 4) / 4).astype(np.float16)
    frame16, frame32 = pd.DataFrame(x16), pd.DataFrame(x16.astype(np.float32))
    for f in (frame16, frame32):
        f.index = [11, 12, 13, 14, 15]
    assert (frame16.dtypes == np.float16).all()
    want = [(np.float16, np.float16), (np.float32, np.float32), (np.float32, np.float32), (np.float32, np.float32)]
    for (q, f), (dq, dx) in zip(((q16, frame16), (q16, frame32), (q16.astype(np.float32), frame16), (q16.astype(np.float32), frame32)), want):
        lims, ids = drv.range_truth(q, f, 0.25)
        got = asked[-1]
        assert (got[0], got[1]) == (dq, dx)
        assert np.array_equal(got[2].astype(np.float32), q16.astype(np.float32)) and np.array_equal(got[3].astype(np.float32), x16.astype(np.float32))
        np.testing.assert_array_equal(ids, [11, 15, 13])


@pytest.mark.parametrize("shape", hc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cases_are_halves_and_keep_their_tie_group_on_top(oracle, shape):
    nq, nb, d = shape
    c = hc.case(*shape)
    g, t = kc.tie_group(nb), hc.tie_queries(nq)
    assert c.q16.shape == (nq, d) and c.x16.shape == (nb, d) and c.q16.dtype == c.x16.dtype == np.float16
    assert c.q32.dtype == c.x32.dtype == np.float32 and not any(a.flags.writeable for a in c)
    # narrowed once: the binary32 copies hold the same values, and every value is a finite half
    assert np.array_equal(c.q32.astype(np.float16).view(np.uint16), c.q16.view(np.uint16)) and np.array_equal(c.x32.astype(np.float16).view(np.uint16), c.x16.view(np.uint16))
    assert np.all(np.isfinite(c.x32)) and np.all(np.isfinite(c.q32))
    assert g.size == 52 and g[-1] == nb - 1 and g[0] == 17 and t >= 4
    assert np.all(c.x16[g] == c.x16[17]) and np.all(c.q16[:t] == c.x16[17])
    for metric in hc.METRICS:
        D, I = hc.truth(oracle, shape, c, 65, metric)
        np.testing.assert_array_equal(I[:t, :52], np.broadcast_to(g, (t, 52)))   # the tie group is the top of its queries, ascending
        assert np.all(D[:t, :52].view(np.uint32) == D[0, 0].view(np.uint32))
        assert np.all(D[:t, 52] < D[0, 0]) if metric == "ip" else np.all(D[:t, 52] > D[0, 0])   # and nothing else ties with it


@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("shape", hc.RANGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_radius_recipe(oracle, shape, metric):
    """At least half of the queries have a non-empty result, at least one has an empty one, every non-empty query's radius is some
    row's distance exactly -- the `<=` edge -- and the reference is the whole-base reference (k = nb on the oracle)."""
    nq, nb, d = shape
    c = hc.case(*shape)
    radius, (lims, dd, ii) = hc.recipe(oracle, shape, metric)
    n = np.diff(lims)
    assert radius.shape == (nq,) and radius.dtype == np.float32 and not np.any(np.isnan(radius))
    assert 2 * np.count_nonzero(n) >= nq and np.count_nonzero(n == 0) >= 1
    assert np.all((n == 0) == (np.arange(nq) % 4 == 3))
    met = 0
    for q in np.flatnonzero(n):
        a, b = lims[q], lims[q + 1]
        assert np.all(np.diff(ii[a:b].astype(np.int64)) > 0)                       # ascending rows
        met += bool(np.any(dd[a:b].view(np.uint32) == radius[q:q + 1].view(np.uint32)))
        assert b - a >= hc.RECIPE_J[q % 4] + 1
    assert met == np.count_nonzero(n) >= 1                                         # dist == radius on every non-empty query
    for q in range(0, hc.tie_queries(nq), 4):   # j = 0 on a tie query: exactly the tie group
        np.testing.assert_array_equal(ii[lims[q]:lims[q + 1]], kc.tie_group(nb).astype(np.uint32))
    with np.errstate(all="ignore"):
        want = kr.whole_base_ref(oracle, c.q32, c.x32, radius, metric)
    np.testing.assert_array_equal(lims, want[0])
    np.testing.assert_array_equal(ii, want[2])
    np.testing.assert_array_equal(dd.view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("d", [40, 45])
def test_special_case_holds_what_it_says(oracle, d):
    c = hc.special(d)
    sub = np.float32(2.0 ** -14)   # the smallest normal half
    assert np.all(np.isnan(c.x32[3])) and np.isinf(c.x32[5, 0]) and np.all(c.x32[7] > 0) and np.all(c.x32[7] < sub)
    assert np.all(c.x16[9].view(np.uint16) == 0x8000) and np.all(c.x32[11] == 65504) and np.all(c.x32[13] == -65504)
    assert not np.any(c.q32[2]) and np.all(c.q16[3].view(np.uint16) == 0x8000) and c.x32[699, d - 1] == 65504
    for metric in hc.METRICS:
        D, I = hc.truth(oracle, ("special", d), c, 64, metric)
        assert not np.any(I == 3) and not np.any(np.isnan(D))
