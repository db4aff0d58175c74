"""CPU (`-m "not gpu"`): the host side of the union scan.  The five entry points are exported and bound; the plan enum matches
`_capi.UNION_PLAN_FIELDS`; the bindings refuse bad arguments before the library is loaded; `li.LearnedIndex` routes by `merge` (against
a recording stand-in for the library: no GPU call is made); the call's geometry (csrc/lmi_union_plan.h, pure host code) passes its
stand-alone self-test under AddressSanitizer + UBSan; and the inputs of tests/union_ref.py have, on the oracle, the properties
tests/test_gpu_union.py relies on."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import union_ref as ur
from learnedmetricindex_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_union_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in (("lmi_scan_union", 10), ("lmi_search_union", 11), ("lmi_search_tree_union", 12), ("lmi_union_set_geometry", 2),
                        ("lmi_debug_union_plan", 2)):
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    assert _capi.SIGNATURES["lmi_union_set_geometry"][1] == [ctypes.c_int64, ctypes.c_int64]
    assert _capi.UNION_MAX_K == 1024 and _capi.K_PER_BUCKET == 10
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = fh.read()
    assert "#define LMI_UNION_MAX_K 1024" in header
    words = header.split("LMI_UNION_PLAN_GROUPS = 0")[1].split("LMI_UNION_PLAN_COUNT")[0]
    assert _capi.UNION_PLAN_FIELDS[0] == "GROUPS" and len(_capi.UNION_PLAN_FIELDS) == 8
    assert list(_capi.UNION_PLAN_FIELDS[1:]) == [ln.split(",")[0].strip()[len("LMI_UNION_PLAN_"):] for ln in words.splitlines()[1:]
                                                 if "LMI_UNION_PLAN_" in ln]
    for want in ("groups", "query_rows", "waves", "slab_bytes", "list_rows", "lists_per_query", "workspace_bytes", "vec_rows"):
        assert want.upper() in _capi.UNION_PLAN_FIELDS   # the words the plan has to report, at least
    for name in ("scan_union", "search_union", "search_tree_union", "scan_union_device", "search_union_device", "search_tree_union_device"):
        assert callable(getattr(_capi.Index, name))
    assert callable(_capi.union_set_geometry) and callable(_capi.union_last_plan)


def test_union_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    idx = object.__new__(_capi.Index)   # no handle: nothing below may reach the library
    q, bo = np.zeros((3, 8), np.float32), np.zeros((3, 2), np.int32)
    for k in (0, 1025, -1, 2.5):
        with pytest.raises(ValueError):
            idx.scan_union(q, bo, k)
        with pytest.raises(ValueError):
            idx.search_union(q, q, 2, k)
        with pytest.raises(ValueError):
            idx.search_tree_union(q, q, 2, k)
    for bad_q, bad_bo in ((q[0], bo), (q, bo[0]), (None, bo), (q, None), (q, bo[:2]), (q, np.zeros((3, 0), np.int32)),
                          (q, np.zeros((3, 1025), np.int32))):
        with pytest.raises(ValueError):
            idx.scan_union(bad_q, bad_bo, 10)
    for nb in (0, 1025):
        with pytest.raises(ValueError):
            idx.search_union(q, q, nb, 10)
        with pytest.raises(ValueError):
            idx.search_tree_union(q, q, nb, 10)
    with pytest.raises(ValueError):
        idx.search_union(q, q[:2], 2, 10)
    with pytest.raises(ValueError):
        idx.scan_union_device(q, bo, 2, 0, None, None)


class Recorder:
    """Stands in for the loaded library: every entry point returns 0 and is recorded as (name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_li_routes_by_merge(monkeypatch):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    for fn in (LearnedIndex.search, LearnedIndex.search_resident):
        assert inspect.signature(fn).parameters["merge"].default == "ranks", fn
    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    eng = _capi.Index(0)
    eng.n_classes = 12
    rs = np.random.RandomState(0)
    Q = rs.randn(7, 8).astype(np.float32)
    names = lambda: [n for n, _ in rec.calls]

    li = LearnedIndex(None, {}, [])
    with pytest.raises(ValueError, match="merge"):   # refused before anything else is looked at
        li.search(None, None, None, None, None, [12], 2, 10, merge="best")
    with pytest.raises(ValueError, match="merge"):
        li.search_resident(None, None, [12], 2, 10, merge=None)
    li._engine = eng

    # 1 level, union: one lmi_search_union with the whole batch; k and the shapes are the caller's, also for one bucket
    rec.calls.clear()
    with np.errstate(all="ignore"):   # the stand-in fills nothing in
        d, n, clock = li.search_resident(Q, Q, [12], n_buckets=3, k=100, merge="union")
    assert names() == ["lmi_search_union"] and d.shape == n.shape == (7, 100) and d.dtype == np.float64 and n.dtype == np.uint32
    args = rec.calls[0][1]
    assert args[3:6] == (7, 3, 100) and args[-1] == 0 and args[1] == args[2]   # nq, nb, k; host pointers; one query array
    rec.calls.clear()
    with np.errstate(all="ignore"):
        d, n, _ = li.search_resident(Q, Q, [12], n_buckets=1, k=1024, merge="union")
    assert names() == ["lmi_search_union"] and d.shape == (7, 1024)
    for k in (0, 1025):
        with pytest.raises(ValueError):
            li.search_resident(Q, Q, [12], n_buckets=3, k=k, merge="union")

    # the stops compose: set before the call, put back after it
    rec.calls.clear()
    with np.errstate(all="ignore"):
        li.search_resident(Q, Q, [12], n_buckets=3, k=100, merge="union", stop_mass=0.9, stop_rows=500)
    assert names() == ["lmi_set_stop_mass", "lmi_set_stop_rows", "lmi_search_union", "lmi_set_stop_mass", "lmi_set_path_mass", "lmi_set_stop_rows"]
    assert int(getattr(rec.calls[1][1][1], "value", rec.calls[1][1][1])) == 500 and int(getattr(rec.calls[5][1][1], "value", rec.calls[5][1][1])) == 0

    # several levels, union: lmi_search_tree_union
    li._entry_paths, li._nav_cap = np.zeros((16, 2), np.int32), 16
    rec.calls.clear()
    with np.errstate(all="ignore"):
        d, n, _ = li.search_resident(Q, Q, [4, 3], n_buckets=5, k=100, merge="union", path_mass=0.9)
    assert [x for x in names() if "set_" not in x] == ["lmi_search_tree_union"] and d.shape == (7, 100)

    # the default is today's call, and its k <= 20 rule stands
    rec.calls.clear()
    with np.errstate(all="ignore"):
        d, n, _ = li.search_resident(Q, Q, [12], n_buckets=3, k=10)
        d2, n2, _ = li.search_resident(Q, Q, [12], n_buckets=3, k=10, merge="ranks")
    assert "lmi_search" in names() and not any("union" in x for x in names()) and d.shape == d2.shape == (7, 10)
    with pytest.raises(AssertionError):
        li.search_resident(Q, Q, [12], n_buckets=3, k=100)


def test_driver_flag():
    from learnedmetricindex_amd.search import Experiment

    assert Experiment.from_argv(["--n-categories", "12"]).merge == "ranks"
    e = Experiment.from_argv(["--n-categories", "12", "--merge", "union", "--k", "1000"])
    assert e.merge == "union" and e.k == 1000
    for bad in (["--n-categories", "12", "--merge", "union", "--k", "1025"], ["--n-categories", "12", "--merge", "best"],
                ["--n-categories", "12", "--merge", "union", "--storage", "f16"]):
        with pytest.raises(SystemExit):
            Experiment.from_argv(bad)


def test_union_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "union_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "union_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "union plan selftest: clean" in r.stdout


# ---- the GPU cases' inputs, on the oracle alone ----
def test_the_shapes_are_the_ones_asked_for():
    assert ur.N == 6000 and ur.L == 12 and ur.NQ == 150
    assert {0, 1, 33, 257}.issubset(ur.SIZES) and 1900 <= max(ur.SIZES) <= 2100
    assert ur.DIMS == (45, 64, 136) and ur.NBS == (1, 3, 8) and ur.KS == (1, 10, 100, 129, 1024) and ur.METRICS == ("ip", "l2")
    for d in ur.DIMS:
        X, Q, lab, ids = ur.case(d)
        assert X.shape == (ur.N, d) and Q.shape == (ur.NQ, d) and not X.flags.writeable
        assert np.array_equal(np.bincount(lab, minlength=ur.L), ur.SIZES) and np.unique(ids).size == ur.N and not np.array_equal(ids, np.arange(1, ur.N + 1))


@pytest.mark.parametrize("nb", ur.NBS)
def test_most_queries_of_the_main_grid_fill_k_100(nb):
    """counts depend on the order and the sizes alone: at k = 100 at least 90 % of the queries get 100 real results, some do not,
    and the order has -1 slots."""
    order = ur.random_order(nb)
    sizes = np.asarray(ur.SIZES)
    cand = np.where(order >= 0, sizes[np.maximum(order, 0)], 0).sum(axis=1)
    assert (order < 0).any() and (cand >= 100).mean() >= 0.9 and (cand < 100).any() and (cand == 0).any()
    assert order[4, 0] == 4


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_reference_counts_pads_and_skips(oracle, metric):
    d = 64
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    order = ur.random_order(3)
    dd, ii, cc = ur.union_ref(oracle, rows, labs, order, Q, 100, metric)
    sizes = np.asarray(ur.SIZES)
    cand = np.where(order >= 0, sizes[np.maximum(order, 0)], 0).sum(axis=1)
    assert np.array_equal(cc, np.minimum(cand, 100)) and (cc == 100).mean() >= 0.9
    for q in (0, 4, 77):
        assert np.all(np.isposinf(dd[q, cc[q]:])) and np.all(ii[q, cc[q]:] == 0) and np.all(np.isfinite(dd[q, :cc[q]]))
        assert np.all(np.diff(dd[q, :cc[q]]) >= 0)   # ascending distances
        mine = np.concatenate([labs[b] for b in order[q] if b >= 0] + [np.zeros(0, np.uint32)])
        assert np.isin(ii[q, :cc[q]], mine).all()
    # a bucket listed twice contributes twice: every object of it appears twice among all candidates
    twice = np.tile(np.asarray([[2, 2]], np.int32), (ur.NQ, 1))
    d2, i2, c2 = ur.union_ref(oracle, rows, labs, twice, Q, 100, metric)
    assert np.all(c2 == 66) and np.all(np.sort(i2[:, :66], axis=1)[:, ::2] == np.sort(i2[:, :66], axis=1)[:, 1::2])


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_tie_case_ties(oracle, metric):
    X, Q, lab, ids, order = ur.tie_case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    copies = [int(np.all(rows[b] == Q[0], axis=1).sum()) for b in ur.TIE_BUCKETS]
    assert tuple(copies) == ur.TIE_COPIES and np.all(Q[:4] == Q[0])
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    dd, ii, cc = ur.union_ref(oracle, rows, labs, order, Q, 100, metric)
    np.testing.assert_array_equal(ii[:4, :40], np.broadcast_to(tied, (4, 40)))          # by (rank, row)
    assert np.all(dd[:4, :40].view(np.uint32) == dd[0, 0].view(np.uint32)) and np.all(dd[:4, 40] > dd[0, 0])   # and nothing else ties with them


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_short_cases_come_up_short(oracle, metric):
    X, Q, lab, ids = ur.case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    for bucket in (1, 2, 0):
        order = np.full((ur.NQ, 1), bucket, dtype=np.int32)
        dd, ii, cc = ur.union_ref(oracle, rows, labs, order, Q, 100, metric)
        n = ur.SIZES[bucket]
        assert n < 100 and np.all(cc == n) and np.all(np.isposinf(dd[:, n:])) and np.all(ii[:, n:] == 0)
        assert np.all(np.sort(ii[:, :n], axis=1) == np.sort(labs[bucket]))


def test_the_nan_case_holds_a_nan(oracle):
    X, Q, lab, ids, row = ur.nan_case(45)
    assert np.isnan(X[row]).sum() == 1 and lab[row] == 3
    rows, labs = ur.buckets_of(X, lab, ids)
    order = np.tile(np.asarray([3, 4], dtype=np.int32), (ur.NQ, 1))
    for metric in ur.METRICS:
        dd, ii, cc = ur.union_ref(oracle, rows, labs, order, Q, 1024, metric)
        assert np.all(cc == 1024) and not np.any(ii == ids[row]) and not np.any(np.isnan(dd))
        # with k = everything the row is still absent: it is refused, not merely ranked last
        few = np.full((2, 1), 3, dtype=np.int32)
        d3, i3, c3 = ur.union_ref(oracle, rows, labs, few, Q[:2], 257, metric)
        assert np.all(c3 == 256) and not np.any(i3 == ids[row])
