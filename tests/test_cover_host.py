"""CPU (`-m "not gpu"`): the host side of the bucket cover and the exact range search (lmi_cover_create, lmi_cover_order,
lmi_search_range_exact).  The entry points are exported, declared and bound and the plan enum matches
`_capi.COVER_PLAN_FIELDS`; the bindings refuse bad arguments before the library is loaded; the admission rule
(csrc/lmi_cover_plan.h: the text the kernel runs) passes its stand-alone self-test under AddressSanitizer + UBSan; and on the oracle
alone the contract restated in tests/cover_ref.py is complete -- a range scan over the cover's order returns what the scan of the
whole base returns -- and the clustered case has the property tests/test_gpu_cover.py relies on."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cover_ref as cr
import knn_range_ref as kr
import range_ref as rr
import union_ref as ur
from learnedmetricindex_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = (("lmi_cover_create", 2), ("lmi_cover_destroy", 1), ("lmi_cover_read", 4), ("lmi_cover_order", 9),
           ("lmi_search_range_exact", 12), ("lmi_cover_set_geometry", 1), ("lmi_debug_cover_plan", 2))
WORDS = ["GROUPS", "QUERY_ROWS", "BUCKETS", "ADMITTED", "MAX_PER_QUERY", "NB_USED", "WORKSPACE_BYTES"]


def test_cover_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, _ in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in lmi_hip.h"
    assert "typedef struct lmi_cover lmi_cover;" in header
    words = re.findall(r"\bLMI_COVER_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", header)
    assert words[-1] == "COUNT" and list(_capi.COVER_PLAN_FIELDS) == words[:-1] == WORDS
    assert re.search(r"#define LMI_ABI_VERSION 1\b", text)
    for name in ("cover_order", "cover_order_device", "search_range_exact", "search_range_exact_device"):
        assert callable(getattr(_capi.Index, name))
    for name in ("read", "close", "__enter__", "__exit__"):
        assert callable(getattr(_capi.Cover, name))
    assert callable(_capi.cover_set_geometry) and callable(_capi.cover_last_plan)
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    assert callable(LearnedIndex.range_search_exact) and callable(LearnedIndex.range_search_exact_resident)


def _stand_ins():
    closed = object.__new__(_capi.Index)
    closed._h = None
    live = object.__new__(_capi.Index)
    live._h, live.d, live.L = ctypes.c_void_p(1), 8, 12
    cover = object.__new__(_capi.Cover)
    cover._c, cover.L, cover.d = ctypes.c_void_p(2), 12, 8
    shut = object.__new__(_capi.Cover)
    shut._c = None
    return closed, live, cover, shut


def test_cover_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    closed, live, cover, shut = _stand_ins()
    q = np.zeros((3, 8), np.float32)
    for bad in (None, "far", np.zeros(2, np.float32), np.zeros((3, 1), np.float32), [0.1, 0.2]):
        with pytest.raises(ValueError):
            live.cover_order(q, bad, cover)
        with pytest.raises(ValueError):
            live.search_range_exact(q, bad, cover)
    for bad in (None, object(), live, shut, "cover"):
        with pytest.raises(ValueError):
            live.cover_order(q, 0.5, bad)
        with pytest.raises(ValueError):
            live.search_range_exact(q, 0.5, bad)
    for bad in (None, np.zeros(8, np.float32), np.zeros((3, 9), np.float32), np.zeros((2, 3, 8), np.float32), [[0.0] * 8]):
        with pytest.raises(ValueError):
            live.cover_order(bad, 0.5, cover)
        with pytest.raises(ValueError):
            live.search_range_exact(bad, 0.5, cover)
    for bad in (0, -1, 1.5, True, "4"):
        with pytest.raises(ValueError):
            live.cover_order(q, 0.5, cover, nb=bad)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            live.search_range_exact(q, 0.5, cover, max_total=bad)
    with pytest.raises(ValueError):
        live.search_range_exact(q, 0.5, cover, filter_of=np.zeros(3, np.int32))   # filter_of without a filter
    with pytest.raises(ValueError):
        live.search_range_exact(q, 0.5, cover, filter=[1, 2, 3])                   # not a _capi.Filter
    with pytest.raises(ValueError):
        closed.cover_order(q, 0.5, cover)
    with pytest.raises(ValueError):
        closed.search_range_exact(q, 0.5, cover)
    with pytest.raises(ValueError):
        live.cover_order_device(q, 0.5, cover, 4)          # numpy where a device tensor is due
    with pytest.raises(ValueError):
        live.search_range_exact_device(q, 0.5, cover)
    with pytest.raises(ValueError):
        _capi.Cover(closed)
    with pytest.raises(ValueError):
        _capi.Cover("index")
    with pytest.raises(ValueError):
        shut.read()
    for bad in (-1, (1 << 20) + 1, 1.0, None, True, "8"):
        with pytest.raises(ValueError):
            _capi.cover_set_geometry(query_rows=bad)
    # the accepted forms reach the library (and only then fail, on the stand-in that forbids it)
    for radius in (0.5, 1, np.float32(0.25), np.zeros(3, np.float32), np.zeros(3, np.float64), [0.1, 0.2, 0.3]):
        with pytest.raises(AssertionError, match="library was loaded"):
            live.cover_order(q, radius, cover)
        with pytest.raises(AssertionError, match="library was loaded"):
            live.search_range_exact(q, radius, cover, max_total=5)


def test_cover_rule_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cover_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "cover_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cover plan selftest: clean" in r.stdout


def _inputs(oracle, case, d, metric):
    """(X, Q, labels, ids, L, radius) of the union case or the clustered case."""
    if case == "union":
        X, Q, lab, ids = ur.case(d)
        return X, Q, lab, ids, ur.L, cr.union_radii(oracle, d, metric)
    X, Q, lab, ids, radius, _ = cr.clustered_case(oracle, d, metric)
    return X, Q, lab, ids, cr.CL, radius


def _per_query(lims, dists, ids):
    """[{id: dist bits}] per query; ids in these cases are unique."""
    out = []
    for q in range(len(lims) - 1):
        a, b = int(lims[q]), int(lims[q + 1])
        m = dict(zip(ids[a:b].tolist(), dists[a:b].view(np.uint32).tolist()))
        assert len(m) == b - a
        out.append(m)
    return out


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
@pytest.mark.parametrize("case", ("union", "clustered"))
def test_the_scan_of_the_cover_order_is_the_scan_of_the_whole_base(oracle, case, d, metric):
    """On the oracle alone: `range_ref` over `cover_ref`'s order == the range scan of all rows as one bucket -- ids as sets per query,
    dist bits per id.  The rule of tests/cover_ref.py (float64, margin factor 1) misses no needed bucket."""
    X, Q, lab, ids, L, radius = _inputs(oracle, case, d, metric)
    cover = cr.cover_of(X, lab, L)
    order, counts = cr.order_ref(cr.admitted_ref(cover, Q, radius, metric))
    assert order.shape[1] == max(1, counts.max())
    rows, labs = ur.buckets_of(X, lab, ids, L)
    got = _per_query(*rr.range_ref(oracle, rows, labs, order, Q, radius, metric))
    lims, dd, ii = kr.whole_base_ref(oracle, np.ascontiguousarray(Q), np.ascontiguousarray(X), radius, metric)
    want = _per_query(lims, dd, np.asarray(ids)[ii.astype(np.int64)])
    assert sum(len(m) for m in want) >= len(want)   # every radius sits on a computed distance: no query comes back empty
    assert got == want


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", (24, 33) + ur.DIMS)
def test_the_clustered_case_admits_one_bucket_per_query_with_the_margin_doubled(oracle, d, metric):
    """A condition on the INPUTS that tests/test_gpu_cover.py relies on: the admitted set lies between the sets of margin / 2 and
    margin x 2, and in the clustered case both are the query's own bucket alone; the special buckets are what they are called."""
    X, Q, lab, ids, radius, home = cr.clustered_case(oracle, d, metric)
    cover = cr.cover_of(X, lab, cr.CL)
    assert cover["n"].tolist() == list(cr.CSIZES) and cover["n"][cr.C_EMPTY] == 0
    assert cover["R"][cr.C_ONE] == 0.0 and cover["R"][cr.C_SAME] == 0.0 and not cover["c"][cr.C_EMPTY].any()
    assert np.all(cover["R"][[b for b in range(cr.CL) if cr.CSIZES[b] > 1 and b != cr.C_SAME]] > 0)
    for factor in (0.5, 1.0, 2.0):
        adm = cr.admitted_ref(cover, Q, radius, metric, factor)
        assert adm.sum(axis=1).tolist() == [1] * cr.CNQ
        assert np.array_equal(np.argmax(adm, axis=1), home)
    assert len(set(home.tolist())) >= 4 and len(np.unique(ids)) == len(ids)


def test_the_reference_rule_at_the_edges(oracle):
    X, Q, lab, ids, radius, home = cr.clustered_case(oracle, 24, "l2")
    cover = cr.cover_of(X, lab, cr.CL)
    has = cover["n"] > 0
    r = np.array(radius)
    r[0], r[1], r[2] = np.nan, -np.inf, np.inf
    adm = cr.admitted_ref(cover, Q, r, "l2")
    assert not adm[0].any() and not adm[1].any() and np.array_equal(adm[2], has)
    Qn = np.array(Q)
    Qn[3, 5] = np.nan
    for metric in ur.METRICS:
        assert np.array_equal(cr.admitted_ref(cover, Qn, r, metric)[3], has)   # a NaN query admits every non-empty bucket
    order, counts = cr.order_ref(adm)
    assert counts[2] == has.sum() and order[2, :counts[2]].tolist() == np.flatnonzero(has).tolist() and (order[0] == -1).all()


def _driver(monkeypatch):
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("lmi_search_driver_cover", os.path.join(ROOT, "learnedmetricindex_amd", "search.py"))
    drv = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "lmi_search_driver_cover", drv)   # dataclasses resolves the module of Experiment
    spec.loader.exec_module(drv)
    return drv


def test_driver_flags(monkeypatch):
    drv = _driver(monkeypatch)
    exp = drv.Experiment.from_argv(["--range-radius", "0.7", "--range-exact"])
    assert exp.range_exact and exp.range_radius == 0.7
    assert not drv.Experiment.from_argv(["--range-radius", "0.7"]).range_exact
    for argv in (["--range-exact"], ["--range-radius", "0.7", "--range-exact", "--storage", "f16"]):
        with pytest.raises(SystemExit):
            drv.Experiment.from_argv(argv)
