"""CPU (`-m "not gpu"`): the host side of the range search.  The entry points are exported and bound and the plan enum matches
`_capi.RANGE_PLAN_FIELDS`; the bindings refuse bad arguments before the library is loaded; `li.LearnedIndex.range_search` routes
(against a recording stand-in for the library: no GPU call is made) -- one call on a 1-level index, pieces on a multi-level one, the
stops set and put back; the offsets, lims and gathers (csrc/lmi_range_plan.h, pure host code) pass their stand-alone self-test under
AddressSanitizer + UBSan; and the radius recipe of tests/range_ref.py has, on the oracle alone, the properties tests/test_gpu_range.py
relies on."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import range_ref as rr
import union_ref as ur
from learnedmetricindex_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = (("lmi_scan_range", 11), ("lmi_search_range", 12), ("lmi_search_tree_range", 13), ("lmi_range_result_total", 2),
           ("lmi_range_result_lims", 2), ("lmi_range_result_read", 4), ("lmi_range_result_destroy", 1), ("lmi_debug_range_plan", 2))


def test_range_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, _ in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in lmi_hip.h"
    assert "typedef struct lmi_range_result lmi_range_result;" in header
    words = re.findall(r"\bLMI_RANGE_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", header)
    assert words[-1] == "COUNT" and list(_capi.RANGE_PLAN_FIELDS) == words[:-1]
    assert words[:-1] == ["GROUPS", "QUERY_ROWS", "WAVES", "SLAB_BYTES", "RESULTS", "CHUNK_BYTES", "WORKSPACE_BYTES"]
    # the words of the other plan enums are found by prefix (tests/test_capi_exports.py): these must not be
    assert not re.search(r"\bLMI_(MLP_)?PLAN_(RESULTS|CHUNK_BYTES)\b", header)
    for name in ("scan_range", "search_range", "search_tree_range", "scan_range_device", "search_range_device", "search_tree_range_device"):
        assert callable(getattr(_capi.Index, name))
    for name in ("read", "read_into", "close"):
        assert callable(getattr(_capi.RangeResult, name))
    assert callable(_capi.range_last_plan)


def test_range_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    idx = object.__new__(_capi.Index)   # no handle: nothing below may reach the library
    q, bo = np.zeros((3, 8), np.float32), np.zeros((3, 2), np.int32)
    for bad in (None, "far", np.zeros(2, np.float32), np.zeros((3, 1), np.float32), np.zeros(4, np.float32), [0.1, 0.2]):
        with pytest.raises(ValueError):
            idx.scan_range(q, bo, bad)
        with pytest.raises(ValueError):
            idx.search_range(q, q, 2, bad)
        with pytest.raises(ValueError):
            idx.search_tree_range(q, q, 2, bad)
    for max_total in (-1, 2.5, None, True):
        with pytest.raises(ValueError):
            idx.scan_range(q, bo, 0.5, max_total=max_total)
    for bad_q, bad_bo in ((q[0], bo), (q, bo[0]), (None, bo), (q, None), (q, bo[:2]), (q, np.zeros((3, 0), np.int32)),
                          (q, np.zeros((3, 1025), np.int32))):
        with pytest.raises(ValueError):
            idx.scan_range(bad_q, bad_bo, 0.5)
    for nb in (0, 1025):
        with pytest.raises(ValueError):
            idx.search_range(q, q, nb, 0.5)
        with pytest.raises(ValueError):
            idx.search_tree_range(q, q, nb, 0.5)
    with pytest.raises(ValueError):
        idx.search_range(q, q[:2], 2, 0.5)
    with pytest.raises(ValueError):
        idx.scan_range(q, bo, 0.5, filter_of=np.zeros(3, np.int32))   # filter_of without a filter
    with pytest.raises(ValueError):
        idx.scan_range(q, bo, 0.5, filter=[1, 2, 3])                  # not a _capi.Filter
    with pytest.raises(ValueError):
        idx.scan_range_device(q, bo, 2, None)


class Recorder:
    """Stands in for the loaded library: every entry point returns 0 and is recorded as (name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_li_range_search_routes(monkeypatch):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    eng = _capi.Index(0)
    eng.n_classes = 12
    rs = np.random.RandomState(0)
    Q = rs.randn(7, 8).astype(np.float32)
    names = lambda: [n for n, _ in rec.calls]
    searches = lambda: [c for c in rec.calls if c[0] in ("lmi_search_range", "lmi_search_tree_range")]

    li = LearnedIndex(None, {}, [])
    # refused before any work: nothing is prepared, nothing is called
    rec.calls.clear()
    for kw in (dict(radius=None), dict(radius=0.5, storage="f16"), dict(radius=0.5, max_total=-1), dict(radius=0.5, filter_of=[0] * 7),
               dict(radius=0.5, stop_mass=0.5, n_categories=[4, 3]), dict(radius=0.5, path_mass=0.5)):
        kw.setdefault("n_categories", [12])
        with pytest.raises(ValueError):
            li.range_search(None, Q, None, Q, None, **kw)
    assert rec.calls == []
    li._engine = eng

    # 1 level: one lmi_search_range with the whole batch; a scalar radius serves every query
    lims, d, n, clock = li.range_search_resident(Q, Q, [12], 0.25, n_buckets=3)
    assert names() == ["lmi_search_range", "lmi_range_result_lims", "lmi_range_result_read", "lmi_range_result_destroy"]
    assert lims.dtype == np.int64 and lims.shape == (8,) and d.dtype == np.float64 and n.dtype == np.uint32 and d.shape == n.shape == (0,)
    args = searches()[0][1]
    assert args[3:5] == (7, 3) and args[-1] == 0 and args[1] == args[2] and args[6] is None and args[7] is None and args[8] == 0
    assert args[5] is not None   # the radius array
    rec.calls.clear()
    li.range_search_resident(Q, Q, [12], np.linspace(0, 1, 7), n_buckets=1, max_total=99, sort=True)
    assert searches()[0][1][8] == 99
    with pytest.raises(ValueError):
        li.range_search_resident(Q, Q, [12], np.zeros(6), n_buckets=3)

    # the stops compose: set before the call, put back after it
    rec.calls.clear()
    li.range_search_resident(Q, Q, [12], 0.25, n_buckets=3, stop_mass=0.9, stop_rows=500)
    assert [x for x in names() if "result" not in x] == ["lmi_set_stop_mass", "lmi_set_stop_rows", "lmi_search_range", "lmi_set_stop_mass",
                                                         "lmi_set_path_mass", "lmi_set_stop_rows"]
    sets = [c for c in rec.calls if c[0] == "lmi_set_stop_rows"]
    assert [int(getattr(c[1][1], "value", c[1][1])) for c in sets] == [500, 0]

    # several levels: lmi_search_tree_range in pieces of the walk's queue limit; the pieces' lims are joined
    li._entry_paths, li._nav_cap = np.zeros((16, 2), np.int32), 16
    monkeypatch.setattr(LearnedIndex, "_nav_chunk", lambda self: 3)
    rec.calls.clear()
    lims, d, n, _ = li.range_search_resident(Q, Q, [4, 3], 0.25, n_buckets=5, path_mass=0.9)
    assert [c[1][3] for c in searches()] == [3, 3, 1] and all(c[0] == "lmi_search_tree_range" for c in searches())
    assert lims.shape == (8,) and lims[0] == 0 and np.all(lims == 0)
    assert names().count("lmi_set_path_mass") == 2

    # joined lims: pieces with results of their own
    def fake(qn, qs, nb, r, filter=None, filter_of=None, max_total=0):
        m = qn.shape[0]
        lims = np.arange(m + 1, dtype=np.int64) * 2
        return lims, np.arange(2 * m, dtype=np.float32)[::-1].copy(), np.arange(2 * m, dtype=np.uint32), None, None

    monkeypatch.setattr(eng, "search_tree_range", fake, raising=False)
    lims, d, n, _ = li.range_search_resident(Q, Q, [4, 3], 0.25, n_buckets=5, sort=True)
    assert np.array_equal(lims, np.arange(8) * 2) and d.shape == (14,)
    assert np.all(d[0::2] <= d[1::2]) and np.array_equal(n[:6], [1, 0, 3, 2, 5, 4])   # every run sorted by distance
    with pytest.raises(_capi.LmiError, match="max_total"):
        li.range_search_resident(Q, Q, [4, 3], 0.25, n_buckets=5, max_total=13)
    assert li.range_search_resident(Q, Q, [4, 3], 0.25, n_buckets=5, max_total=14)[0][-1] == 14


def test_driver_flag():
    from learnedmetricindex_amd.search import Experiment

    assert Experiment.from_argv(["--n-categories", "12"]).range_radius is None
    assert Experiment.from_argv(["--n-categories", "12", "--range-radius", "0.3"]).range_radius == 0.3
    with pytest.raises(SystemExit):
        Experiment.from_argv(["--n-categories", "12", "--range-radius", "0.3", "--storage", "f16"])


def test_range_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "range_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "range_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "range plan selftest: clean" in r.stdout


# ---- the GPU cases' inputs, on the oracle alone ----
def test_the_admission_rule():
    d = np.asarray([0.5, 1.0, np.nan, -np.inf, np.inf], dtype=np.float32)
    assert rr.admitted(d, 1.0).tolist() == [True, True, False, True, False]
    assert rr.admitted(d, np.inf).tolist() == [True, True, False, True, True]
    assert not rr.admitted(d, np.nan).any() and not rr.admitted(d, -np.inf).any()
    assert rr.admitted(np.float32(1.0), np.float64(1.0) + 1e-12).all()   # the radius is compared in binary32


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("nb", ur.NBS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_the_radius_recipe(oracle, d, nb, metric):
    """Every query with a finite radius gets exactly j + 1 results (dist == radius is exercised on each, no two candidates collapse
    onto one distance); the finite-radius totals; queries 0..3 visit nothing; query 4 returns more than 1024 at +inf."""
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    lims, dd, ii = rr.recipe_ref(oracle, d, nb, metric)
    n = np.diff(lims)
    j = np.asarray(rr.RECIPE_J)[np.arange(ur.NQ) % 3]
    finite = np.isfinite(radius)
    assert finite.sum() >= 120 and (~finite).any()
    assert np.array_equal(n[finite], j[finite] + 1)
    assert int(n[finite].sum()) == (5138 if nb == 1 else 5438)
    assert np.all(n[:4] == 0) and np.all(order[:4] < 0) and lims[0] == 0 and np.all(np.diff(lims) >= 0)
    for q in np.flatnonzero(finite)[:20]:
        run = dd[lims[q]: lims[q + 1]]
        assert run.max().view(np.uint32) == radius[q].view(np.uint32)   # the farthest admitted lies ON the radius
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    assert order[4, 0] == 4
    l4, d4, i4 = rr.range_ref(oracle, rows, labs, order[4:5], Q[4:5], np.inf, metric)
    want = np.concatenate([labs[b] for b in order[4] if b >= 0])
    assert l4[1] > 1024 and np.array_equal(i4, want)   # ordinal order = the concatenated buckets


def test_the_reference_orders_by_ordinal_and_filters_by_mask(oracle):
    import union_filter_ref as fr

    d = 64
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    order = ur.random_order(3)
    allowed, fo = fr.case_allowed(d), fr.filter_of()
    lims, dd, ii = rr.range_ref(oracle, rows, labs, order, Q, np.inf, "ip", allowed, fo)
    for q in range(ur.NQ):
        want = [labs[b][allowed[fo[q]][b]] if fo[q] >= 0 else labs[b] for b in order[q] if b >= 0]
        want = np.concatenate(want + [np.zeros(0, np.uint32)])
        assert np.array_equal(ii[lims[q]: lims[q + 1]], want), q
    assert any(lims[q + 1] == lims[q] and (order[q] >= 0).any() for q in range(ur.NQ))   # a query emptied by its filter
