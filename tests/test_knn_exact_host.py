"""CPU (`-m "not gpu"`): the host side of the exact k-NN through the index (lmi_search_knn_exact): symbols and plan
enum, argument errors before the library loads, `li` routing, and the pure code the kernels run (csrc/lmi_knn_exact_plan.h) in its
stand-alone self-test under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from learnedmetricindex_amd import _capi
from test_cover_host import _stand_ins
from test_union_host import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_exact_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, nargs in (("lmi_search_knn_exact", 10), ("lmi_debug_knn_exact_plan", 2)):
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in lmi_hip.h"
    words = re.findall(r"\bLMI_KNN_EXACT_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", header)
    assert words[-1] == "COUNT" and list(_capi.KNN_EXACT_PLAN_FIELDS) == words[:-1]
    assert re.search(r"#define LMI_KNN_EXACT_MAX_SEEDS %d\b" % _capi.KNN_EXACT_MAX_SEEDS, header)


def test_knn_exact_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    closed, live, cover, shut = _stand_ins()
    q = np.zeros((3, 8), np.float32)
    for bad in (0, -1, 1025, 1.5, True, None, "4"):
        with pytest.raises(ValueError):
            live.search_knn_exact(q, bad, cover)
    for bad in (None, object(), live, shut, "cover"):
        with pytest.raises(ValueError):
            live.search_knn_exact(q, 10, bad)
    for bad in (None, np.zeros(8, np.float32), np.zeros((3, 9), np.float32), np.zeros((2, 3, 8), np.float32), [[0.0] * 8]):
        with pytest.raises(ValueError):
            live.search_knn_exact(bad, 10, cover)
    with pytest.raises(ValueError):
        closed.search_knn_exact(q, 10, cover)
    for k in (1, 10, 1024, np.int64(7)):
        with pytest.raises(AssertionError, match="library was loaded"):
            live.search_knn_exact(q, k, cover)


def test_li_routes_to_the_one_call(monkeypatch):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    eng = _capi.Index(0)
    eng._h, eng.d, eng.L = ctypes.c_void_p(1), 8, 12   # (closed below, while the stand-in still answers)
    li = LearnedIndex(None, {}, [])
    with pytest.raises(AssertionError, match="no resident index"):
        li.search_exact_resident(np.zeros((7, 8), np.float32), 5)
    li._engine = eng
    rec.calls.clear()
    d, n, clock = li.search_exact_resident(np.zeros((7, 8), np.float32), k=100)
    assert [c[0] for c in rec.calls] == ["lmi_cover_create", "lmi_search_knn_exact"]
    args = rec.calls[1][1]
    assert args[3:5] == (7, 100) and args[-1] == 0 and d.shape == n.shape == (7, 100) and d.dtype == np.float64 and n.dtype == np.uint32
    rec.calls.clear()
    li.search_exact_resident(np.zeros((2, 8), np.float32), k=3)   # the cover is kept
    assert [c[0] for c in rec.calls] == ["lmi_search_knn_exact"]
    d0, n0, _ = li.search_exact_resident(np.zeros((0, 8), np.float32), k=3)
    assert d0.shape == n0.shape == (0, 3)
    li.close()
    assert li._engine is None and rec.calls[-1][0] == "lmi_destroy"


def test_knn_exact_plan_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "knn_exact_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "knn_exact_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "knn exact plan selftest: clean" in r.stdout
