"""CPU (`-m "not gpu"`): the host side of lmi_knn.  The three entry points are exported and bound; `_capi.knn` refuses bad arguments
before the library is loaded; `li.Baseline` and the driver's recall route by k (against a recording stand-in for the library: no GPU
call is made); the inputs of tests/knn_cases.py have, on the oracle, the properties tests/test_gpu_knn.py relies on; and the call's
geometry (csrc/lmi_knn_plan.h, pure host code) passes its stand-alone self-test under AddressSanitizer + UBSan."""
import ctypes
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import knn_cases as kc
from learnedmetricindex_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in (("lmi_knn", 11), ("lmi_knn_set_geometry", 3), ("lmi_debug_knn_plan", 2)):
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    assert _capi.KNN_MAX_K == 1024 and _capi.K_PER_BUCKET == 10
    assert len(_capi.KNN_PLAN_FIELDS) == 9 and _capi.KNN_METRICS == {"ip": 0, "l2": 1}
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = fh.read()
    assert "#define LMI_KNN_MAX_K 1024" in header
    words = header.split("LMI_KNN_PLAN_PIECES = 0")[1].split("LMI_KNN_PLAN_COUNT")[0]
    assert [w for w in _capi.KNN_PLAN_FIELDS[1:]] == [ln.split(",")[0].strip()[len("LMI_KNN_PLAN_"):] for ln in words.splitlines()[1:] if "LMI_KNN_PLAN_" in ln]


def test_knn_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    q, x = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32)
    for args, kw in (((q, x), dict(k=0)), ((q, x), dict(k=1025)), ((q, x), dict(metric="cosine")), ((q.astype(np.float64), x), {}),
                     ((q, x.astype(np.float16)), {}), ((q, x[:, :7]), {}), ((q[0], x), {}), ((q.tolist(), x), {}), ((q, None), {}),
                     ((np.zeros((1, 4097), np.float32), np.zeros((1, 4097), np.float32)), {}), ((np.zeros((1, 0), np.float32), np.zeros((1, 0), np.float32)), {})):
        with pytest.raises(ValueError):
            _capi.knn(*args, **kw)

    class FakeTensor:   # a torch tensor beside a numpy array: both must be of one kind
        dtype, ndim, shape, is_cuda = "torch.float32", 2, (5, 8), True

        def data_ptr(self):
            return 0

    with pytest.raises(ValueError, match="both"):
        _capi.knn(q, FakeTensor())
    with pytest.raises(ValueError, match="both"):
        _capi.knn(FakeTensor(), x)


class Recorder:
    """Stands in for the loaded library: every entry point returns 0 and is recorded as (name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_baseline_routes_by_k(monkeypatch):
    from learnedmetricindex_amd.li.Baseline import Baseline

    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    rs = np.random.RandomState(0)
    X, Q = rs.randn(50, 8).astype(np.float32), rs.randn(4, 8).astype(np.float32)
    assert Baseline.MAX_K == _capi.KNN_MAX_K
    with np.errstate(all="ignore"):   # the stand-in fills nothing in
        d, ids, _ = Baseline().search(Q, X, k=10)
    assert [n for n, _ in rec.calls] == ["lmi_knn_ip"] and d.shape == ids.shape == (4, 10)
    with np.errstate(all="ignore"):
        d, ids, _ = Baseline().search(Q, X, k=11)
    name, args = rec.calls[-1]
    assert [n for n, _ in rec.calls] == ["lmi_knn_ip", "lmi_knn"] and d.shape == ids.shape == (4, 11)
    assert args[2] == 4 and args[4] == 50 and args[5] == 8 and args[6] == 11 and args[7] == 0 and args[10] == 0   # nq, nb, d, k, IP, host pointers
    for k in (0, 1025):
        with pytest.raises(ValueError):
            Baseline().search(Q, X, k=k)
    assert len(rec.calls) == 2


def test_driver_recall_asks_for_k_true_neighbours(monkeypatch):
    spec = importlib.util.spec_from_file_location("lmi_search_driver_knn", os.path.join(ROOT, "learnedmetricindex_amd", "search.py"))
    drv = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "lmi_search_driver_knn", drv)   # dataclasses resolves the module of Experiment
    spec.loader.exec_module(drv)
    import pandas as pd

    asked = []

    class FakeBaseline:
        MAX_K = drv.Baseline.MAX_K

        def search(self, queries, data, k=10, device=0):
            asked.append(k)
            return None, np.tile(np.arange(1, k + 1), (queries.shape[0], 1)), 0.0

    monkeypatch.setattr(drv, "Baseline", FakeBaseline)
    objects = pd.DataFrame(np.zeros((100, 4), np.float32))
    objects.index += 1
    queries = np.zeros((6, 4), np.float32)
    found30 = np.tile(np.arange(1, 31), (6, 1))
    found30[:, 15:] += 50                    # 15 of the true 30; all of the true 10
    assert drv.recall_against_bruteforce(queries, objects, found30, 30) == pytest.approx(0.5)
    assert drv.recall_against_bruteforce(queries, objects, found30[:, :10], 10) == pytest.approx(1.0)
    assert drv.recall_against_bruteforce(queries, objects, found30[:, :7], 7) == pytest.approx(1.0)
    assert asked == [30, 10, 7]


@pytest.mark.parametrize("shape", kc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cases_keep_their_tie_group_on_top(oracle, shape):
    xq, xb = kc.case(*shape)
    nq, nb, d = shape
    g = kc.tie_group(nb)
    assert xq.shape == (nq, d) and xb.shape == (nb, d) and g.size == 52 and np.all(np.diff(g) > 0) and g[-1] == nb - 1
    assert np.all(xb[g] == xb[17]) and not xq.flags.writeable and not xb.flags.writeable
    for metric in kc.METRICS:
        D, I = kc.truth(oracle, shape, xq, xb, 64, metric)
        np.testing.assert_array_equal(I[:kc.TIE_QUERIES, :52], np.broadcast_to(g, (kc.TIE_QUERIES, 52)))
        assert np.all(D[:kc.TIE_QUERIES, :52] == D[0, 0])
        assert np.all(D[:kc.TIE_QUERIES, 52] < D[0, 0]) if metric == "ip" else np.all(D[:kc.TIE_QUERIES, 52] > D[0, 0])   # and nothing else ties with it
        # the oracle does not depend on its thread count (the tests take it with several)
        D1, I1 = (oracle.knn_ip if metric == "ip" else oracle.knn_l2)(xq[:9], xb, 64, nthreads=1)
        np.testing.assert_array_equal(I1, I[:9])
        np.testing.assert_array_equal(D1.view(np.uint32), D[:9].view(np.uint32))


def test_adversarial_case_is_strictly_monotone(oracle):
    xq, xb = kc.adversarial()
    assert xb.shape == (5000, 8) and xq.shape == (2, 8)
    D, I = kc.truth(oracle, "adversarial", xq, xb, 1024, "ip")
    np.testing.assert_array_equal(I[0], 4999 - np.arange(1024))
    np.testing.assert_array_equal(I[1], np.arange(1024))
    assert np.all(np.diff(D, axis=1) < 0)
    full, _ = oracle.knn_ip(xq[:1], xb, 5000)
    assert np.all(np.diff(full[0]) < 0)   # all 5000 scores differ: fed in row order, every row is a new best
    # L2: the keys near +u are flat to rounding (s - |x|^2/2 peaks there), so the order is whatever the chain says: oracle only
    D2, I2 = kc.truth(oracle, "adversarial", xq, xb, 1024, "l2")
    assert np.all(np.diff(D2, axis=1) >= 0) and np.all(I2 >= 0)


def test_special_case_holds_what_it_says(oracle):
    xq, xb = kc.special()
    assert np.all(np.isnan(xb[3])) and np.isinf(xb[5, 0]) and not np.any(xq[2])
    sub = np.float32(np.finfo(np.float32).tiny)
    assert 0 < oracle.sqnorms(xb[7:8])[0] < sub   # the row's squared norm is subnormal
    for metric in kc.METRICS:
        D, I = kc.truth(oracle, "special", xq, xb, 64, metric)
        assert not np.any(I == 3) and not np.any(np.isnan(D))


def test_knn_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "knn_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "knn_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "knn plan selftest: clean" in r.stdout
