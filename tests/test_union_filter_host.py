"""CPU (`-m "not gpu"`): the host side of the filtered union scan.  The new entry points are exported and bound and the header's
constants match `_capi`; the bindings refuse bad arguments before the library is loaded; `li.LearnedIndex` routes a filter (against a
recording stand-in for the library: no GPU call is made) and refuses one without merge="union"; the sharded searchers refuse one; the
lists' arithmetic (csrc/lmi_filter_plan.h, pure host code) passes its stand-alone self-test under AddressSanitizer + UBSan; and the
filter set of tests/union_filter_ref.py has, on the oracle alone, the properties tests/test_gpu_union_filter.py relies on."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import union_filter_ref as fr
import union_ref as ur
from learnedmetricindex_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = (("lmi_filter_create", 6), ("lmi_filter_destroy", 1), ("lmi_filter_counts", 2), ("lmi_filter_bucket_mask", 4),
           ("lmi_scan_union_filtered", 12), ("lmi_search_union_filtered", 13), ("lmi_search_tree_union_filtered", 14),
           ("lmi_debug_filter_plan", 2))


def test_filter_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = fh.read()
    for name, nargs in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert f"LMI_API int {name}(" in header, name
    # a filtered call is its parent's arguments plus (filter, filter_of)
    for parent in ("lmi_scan_union", "lmi_search_union", "lmi_search_tree_union"):
        assert _capi.SIGNATURES[parent + "_filtered"][1] == _capi.SIGNATURES[parent][1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert "#define LMI_FILTER_KEEP 0" in header and "#define LMI_FILTER_DROP 1" in header and "#define LMI_FILTER_MAX 1024" in header
    assert (_capi.FILTER_KEEP, _capi.FILTER_DROP, _capi.FILTER_MAX) == (0, 1, 1024) == (fr.KEEP, fr.DROP, 1024)
    words = header.split("LMI_FILTER_PLAN_FILTERS = 0")[1].split("LMI_FILTER_PLAN_COUNT")[0]
    assert _capi.FILTER_PLAN_FIELDS[0] == "FILTERS" and len(_capi.FILTER_PLAN_FIELDS) == 4
    assert list(_capi.FILTER_PLAN_FIELDS[1:]) == [ln.split(",")[0].strip()[len("LMI_FILTER_PLAN_"):] for ln in words.splitlines()[1:]
                                                  if "LMI_FILTER_PLAN_" in ln]
    # the union plan's enum is pinned: the filter words live in an enum of their own
    assert len(_capi.UNION_PLAN_FIELDS) == 8 and "FILTER" not in header.split("LMI_UNION_PLAN_GROUPS = 0")[1].split("LMI_UNION_PLAN_COUNT")[0]
    assert "stale" in header and "not on the routing" in header   # the header says when a filter stops fitting, and what the stops count
    for name in ("scan_union", "search_union", "search_tree_union", "scan_union_device", "search_union_device", "search_tree_union_device"):
        pars = inspect.signature(getattr(_capi.Index, name)).parameters
        assert pars["filter"].default is None and pars["filter_of"].default is None, name
    assert callable(_capi.filter_last_plan) and all(callable(getattr(_capi.Filter, m)) for m in ("counts", "bucket_mask", "close"))


def test_filter_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    idx = object.__new__(_capi.Index)   # no handle: nothing below may reach the library
    good = [np.asarray([1, 2, 3])]
    for lists, modes in (([], None), ([[1]] * 1025, None), (good, ["keep", "drop"]), (good, ["both"]), (good, [2]), (good, [True]),
                         ([np.asarray([1.5])], None), ([np.asarray([-1])], None), ([np.asarray([2 ** 32])], None), (np.asarray([1, 2, 3]), None)):
        with pytest.raises(ValueError):
            _capi.Filter(idx, lists, modes)
    ids, off, modes = _capi.Filter.pack([[5, 5, 1], [], [7]], ["keep", "drop", _capi.FILTER_DROP])
    assert ids.dtype == np.uint32 and ids.tolist() == [5, 5, 1, 7] and off.dtype == np.int64 and off.tolist() == [0, 3, 3, 4]
    assert modes.dtype == np.int32 and modes.tolist() == [0, 1, 1]
    assert _capi.Filter.pack([[], []])[0].size == 0

    f = object.__new__(_capi.Filter)   # a filter of five, never created in the library
    f._f, f.nf, f.L, f._sizes = ctypes.c_void_p(1), 5, 12, np.zeros(12, np.int64)
    q, bo = np.zeros((3, 8), np.float32), np.zeros((3, 2), np.int32)
    for filt, fo in ((None, np.zeros(3, np.int32)), ("even", None), ([1, 2], None), (f, np.zeros(2, np.int32)), (f, np.zeros((3, 1), np.int32)),
                     (f, np.zeros(3, np.float32)), (f, np.asarray([0, 5, 0])), (f, np.asarray([0, -2, 0]))):
        with pytest.raises(ValueError):
            idx.scan_union(q, bo, 10, filter=filt, filter_of=fo)
        with pytest.raises(ValueError):
            idx.search_union(q, q, 2, 10, filter=filt, filter_of=fo)
        with pytest.raises(ValueError):
            idx.search_tree_union(q, q, 2, 10, filter=filt, filter_of=fo)
        with pytest.raises(ValueError):
            idx.scan_union_device(q, bo, 2, 10, None, None, filter=filt, filter_of=fo)
    closed = object.__new__(_capi.Filter)
    closed._f, closed.nf = None, 5
    with pytest.raises(ValueError, match="closed"):
        idx.scan_union(q, bo, 10, filter=closed)
    for j, b in ((5, 0), (-1, 0), (0, 12)):
        with pytest.raises(ValueError):
            f.bucket_mask(j, b)
    f._f = None   # (nothing to destroy)


class Recorder:
    """Stands in for the loaded library: every entry point returns 0 and is recorded as (name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_li_routes_a_filter(monkeypatch):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    for fn in (LearnedIndex.search, LearnedIndex.search_resident):
        pars = inspect.signature(fn).parameters
        assert pars["filter"].default is None and pars["filter_of"].default is None, fn
    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    eng = _capi.Index(0)
    eng.n_classes = eng.L = 12
    rs = np.random.RandomState(0)
    Q = rs.randn(7, 8).astype(np.float32)
    names = lambda: [n for n, _ in rec.calls]

    li = LearnedIndex(None, {}, [])
    li._engine = eng
    # refused before any work: a filter with the rank merge, filter_of without a filter
    rec.calls.clear()
    for kw in (dict(filter=[1, 2, 3]), dict(filter=[1, 2, 3], merge="ranks"), dict(filter_of=np.zeros(7, np.int32), merge="union")):
        with pytest.raises(ValueError, match="filter"):
            li.search_resident(Q, Q, [12], n_buckets=3, k=10, **kw)
        with pytest.raises(ValueError, match="filter"):
            li.search(None, None, None, None, None, [12], 3, 10, **kw)
    assert names() == []

    # an id list: a keep filter of one list is made for the call, used by one lmi_search_union_filtered and destroyed
    with np.errstate(all="ignore"):   # the stand-in fills nothing in
        d, n, _ = li.search_resident(Q, Q, [12], n_buckets=3, k=100, merge="union", filter=[9, 4, 4])
    assert names() == ["lmi_filter_create", "lmi_bucket_sizes", "lmi_search_union_filtered", "lmi_filter_destroy"] and d.shape == n.shape == (7, 100)
    create, call = rec.calls[0][1], rec.calls[2][1]
    assert create[3] == 1 and call[3:6] == (7, 3, 100) and call[10] == 0 and call[12] is None   # nf; nq, nb, k; host pointers; filter 0 for all

    # a Filter of the caller's is passed on, with filter_of, and is not destroyed; the stops compose
    filt = _capi.Filter(eng, [[1, 2], [3]], ["keep", "drop"])
    fo = np.asarray([-1, 0, 1, 0, 1, -1, 0])
    rec.calls.clear()
    with np.errstate(all="ignore"):
        li.search_resident(Q, Q, [12], n_buckets=3, k=100, merge="union", filter=filt, filter_of=fo, stop_rows=500)
    assert [x for x in names() if "set_" not in x] == ["lmi_search_union_filtered"] and "lmi_set_stop_rows" in names()
    call = [a for n_, a in rec.calls if n_ == "lmi_search_union_filtered"][0]
    assert call[11] == filt._f and call[12] is not None
    with pytest.raises(ValueError):
        li.search_resident(Q, Q, [12], n_buckets=3, k=100, merge="union", filter=filt, filter_of=fo[:3])

    # several levels: lmi_search_tree_union_filtered
    li._entry_paths, li._nav_cap = np.zeros((16, 2), np.int32), 16
    rec.calls.clear()
    with np.errstate(all="ignore"):
        d, n, _ = li.search_resident(Q, Q, [4, 3], n_buckets=5, k=100, merge="union", filter=filt, filter_of=fo)
    assert [x for x in names() if "set_" not in x] == ["lmi_search_tree_union_filtered"] and d.shape == (7, 100)

    # without a filter the calls are the parent's
    rec.calls.clear()
    with np.errstate(all="ignore"):
        li.search_resident(Q, Q, [12], n_buckets=3, k=100, merge="union")
    assert names() == ["lmi_search_union"]
    filt.close()
    assert names()[-1] == "lmi_filter_destroy"


def test_the_sharded_searchers_refuse_a_filter():
    from learnedmetricindex_amd import sharded

    for cls in (sharded.ShardedSearcher, sharded.ReplicaSearcher):
        s = object.__new__(cls)   # refused before anything of the searcher is looked at
        with pytest.raises(ValueError, match="filter"):
            s.search(None, None, 3, 10, merge="union", filter=[1, 2])
    with pytest.raises(ValueError, match="filter"):
        object.__new__(sharded.ShardedSearcher).search_routed(None, None, 3, 10, merge="union", filter=[1, 2])


def test_filter_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "filter_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "filter_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "filter plan selftest: clean" in r.stdout


# ---- the GPU cases' filters, on the oracle alone ----
def test_the_filter_set_is_the_one_asked_for():
    lists, lab, ids = fr.filter_lists(), ur.labels(), ur.case(64)[3]
    assert len(lists) == fr.NF == 5 and fr.MODES == (fr.KEEP, fr.KEEP, fr.DROP, fr.KEEP, fr.KEEP)
    assert set(lists[0].tolist()) == set(ids[ids % 2 == 0].tolist()) and np.unique(lists[0]).size < lists[0].size   # even ids, some twice
    assert np.unique(lists[1]).size == 60 and np.isin(lists[1], ids).all()
    assert lists[2].size == 3 and np.isin(lists[2], ids).sum() == 2 and fr.ABSENT_ID in lists[2]
    assert lists[3].size == 0
    assert np.array_equal(np.sort(lists[4]), np.sort(ids[lab == 4])) and not np.array_equal(lists[4], np.sort(lists[4]))
    assert np.array_equal(fr.filter_of()[:7], [-1, 0, 1, 2, 3, 4, -1]) and fr.filter_of().shape == (ur.NQ,)
    allowed = fr.case_allowed()
    sizes = np.asarray(ur.SIZES)
    cnt = np.asarray([[a.sum() for a in per] for per in allowed])
    assert cnt.shape == (5, ur.L) and np.all(cnt[3] == 0) and np.array_equal(cnt[4], np.where(np.arange(ur.L) == 4, sizes, 0))
    assert cnt[1].sum() == 60 and cnt[2].sum() == ur.N - 2 and 0 < cnt[0].sum() < ur.N
    for b, n in enumerate(ur.SIZES):   # the row-block edges are among the bucket sizes the masks are checked on
        assert all(a[b].shape == (n,) for a in allowed)
    assert {0, 1, 33, 64, 65, 257}.issubset(ur.SIZES)


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_filters_produce_what_the_gpu_tests_rely_on(oracle, metric):
    """Some query comes up short of k, some query gets nothing, some visited (filter, bucket) pair allows no row -- and the removal
    form of the reference equals the forced form, in which the disallowed rows keep their ordinals and are never selected."""
    d, nb, k = 64, 8, 100   # (F1 keeps 60 ids: its queries cannot fill 100)
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    order, fo, allowed = ur.random_order(nb), fr.filter_of(), fr.case_allowed()
    want = fr.union_filter_ref(oracle, rows, labs, order, Q, k, metric, allowed, fo)
    forced = fr.union_filter_forced(oracle, rows, labs, order, Q, k, metric, allowed, fo)
    for a, b in zip(want, forced):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    plain = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
    cc = want[2]
    visits = order[4:] >= 0   # (queries 0..3 visit nothing at all)
    assert ((cc[4:] > 0) & (cc[4:] < k) & (plain[2][4:] == k)).any(), "no query comes up short because of its filter"
    assert ((cc[4:] == 0) & visits.any(axis=1)).any() and cc[4] == 0 and order[4, 0] == 4, "no visiting query is emptied by its filter"
    cnt = np.asarray([[a.sum() for a in per] for per in allowed])
    dead = [(q, t) for q in range(ur.NQ) for t in range(nb) if fo[q] >= 0 and order[q, t] >= 0 and ur.SIZES[order[q, t]] > 0 and cnt[fo[q], order[q, t]] == 0]
    live = [(q, t) for q in range(ur.NQ) for t in range(nb) if fo[q] >= 0 and order[q, t] >= 0 and cnt[fo[q], order[q, t]] > 0]
    assert len(dead) > 50 and len(live) > 50
    # the unfiltered queries are untouched, the filtered ones return allowed ids only
    unf = fo < 0
    np.testing.assert_array_equal(want[1][unf], plain[1][unf])
    for j in range(fr.NF):
        got = want[1][fo == j]
        real = np.arange(k)[None, :] < want[2][fo == j][:, None]
        ok = np.concatenate([l[a] for l, a in zip(labs, allowed[j])])
        assert np.isin(got[real], ok).all()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_a_filter_splits_the_tie_group(oracle, metric):
    X, Q, lab, ids, order = ur.tie_case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    gone, left = fr.tie_filter(tied)
    assert tied.size == 40 and gone.size == 13 and left.size == 27
    mid = labs[ur.TIE_BUCKETS[1]]
    assert np.isin(gone, mid).sum() >= 5 and np.isin(left, mid).sum() >= 5   # the middle bucket's copies are split
    allowed = fr.allowed_rows([gone], [fr.DROP], labs)
    dd, ii, cc = fr.union_filter_ref(oracle, rows, labs, order, Q, 100, metric, allowed, None)
    np.testing.assert_array_equal(ii[:4, :27], np.broadcast_to(left, (4, 27)))   # the survivors, by (rank, row)
    assert np.all(dd[:4, :27].view(np.uint32) == dd[0, 0].view(np.uint32)) and np.all(dd[:4, 27] > dd[0, 0]) and not np.isin(ii, gone).any()
    forced = fr.union_filter_forced(oracle, rows, labs, order, Q, 100, metric, allowed, None)
    np.testing.assert_array_equal(forced[1], ii)
    np.testing.assert_array_equal(forced[0].view(np.uint32), dd.view(np.uint32))
