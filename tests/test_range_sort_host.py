"""CPU (`-m "not gpu"`): the host side of the sort of a range result by distance (lmi_range_result_sort).  The entry
points are exported and bound and the plan enum matches `_capi.RANGE_SORT_PLAN_FIELDS`; the bindings refuse bad arguments before the
library is loaded; the plan's arithmetic (csrc/lmi_range_sort_plan.h, pure host code) passes its stand-alone self-test under
AddressSanitizer + UBSan; tests/range_sort_ref.py's two statements of the order (stable argsort; the kernels' 64-bit words) agree with
np.lexsort((position, key)) on inputs with +-0, +-inf, NaNs and heavy ties; and `li` routes `sort=True` to an engine that sorts on the
device and orders the results itself for one that does not."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import range_sort_ref as rsr
from learnedmetricindex_amd import _capi, sharded

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = (("lmi_range_result_sort", 2), ("lmi_range_result_sorted", 2), ("lmi_range_sort_set_geometry", 2), ("lmi_debug_range_sort_plan", 2))
WORDS = ["GROUPS", "WAVE_SEGMENTS", "TILE_SEGMENTS", "LONG_SEGMENTS", "SKIPPED_SEGMENTS", "TILE_ROWS", "WAVE_ROWS", "MERGE_ROWS", "MAX_PASSES",
         "SCRATCH_BYTES", "RESULTS"]


def test_range_sort_symbols_exported_and_bound():
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
    words = re.findall(r"\bLMI_RANGE_SORT_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", header)
    assert words[-1] == "COUNT" and list(_capi.RANGE_SORT_PLAN_FIELDS) == words[:-1] == WORDS
    assert re.search(r"#define LMI_ABI_VERSION 1\b", text)
    assert "a device-side sort by distance" not in text   # no longer under "Not offered"
    assert callable(_capi.RangeResult.sort) and isinstance(_capi.RangeResult.sorted, property)
    assert callable(_capi.range_sort_set_geometry) and callable(_capi.range_sort_last_plan)
    assert _capi.Index.range_sort is True
    import inspect

    for name in ("scan_range", "search_range", "search_tree_range", "scan_range_device", "search_range_device", "search_tree_range_device"):
        assert inspect.signature(getattr(_capi.Index, name)).parameters["sort"].default is False, name
    for fn in (sharded.ShardedSearcher.range_search, sharded.ShardedSearcher.range_search_routed, sharded.ReplicaSearcher.range_search):
        assert inspect.signature(fn).parameters["sort"].default is False


def test_range_sort_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    for bad in (-1, 32, 63, 100, 16384, 1 << 20, 2.0, None, True, "128"):
        with pytest.raises(ValueError):
            _capi.range_sort_set_geometry(tile_rows=bad)
    for bad in (-1, (1 << 40) + 1, 1.5, None, True):
        with pytest.raises(ValueError):
            _capi.range_sort_set_geometry(scratch_bytes=bad)
    res = object.__new__(_capi.RangeResult)
    res._r = ctypes.c_void_p(1)
    closed = object.__new__(_capi.Index)
    closed._h = None
    for bad in (None, object(), 0, closed):
        with pytest.raises(ValueError):
            res.sort(bad)
    res._r = None   # a closed result
    live = object.__new__(_capi.Index)
    live._h = ctypes.c_void_p(1)
    with pytest.raises(ValueError):
        res.sort(live)
    with pytest.raises(ValueError):
        res.sorted


def test_range_sort_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "range_sort_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "range_sort_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "range sort plan selftest: clean" in r.stdout


def special_dists(rs, n):
    """n distances from 8 ordinary values with +-0, negatives, +-inf and NaNs of both signs and several payloads sprinkled in."""
    d = rs.choice(np.asarray([0.125, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0], np.float32), size=n).astype(np.float32)
    bits = np.asarray([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC12345,
                       0xBF000000, 0xC0400000, 0x00000001, 0x80000001], np.uint32).view(np.float32)
    where = rs.rand(n) < 0.3
    d[where] = rs.choice(bits, size=int(where.sum()))
    return d


def test_the_reference_is_a_lexsort_by_key_then_position():
    rs = np.random.RandomState(11)
    lens = [0, 1, 2, 3, 17, 64, 65, 1000, 4099]
    lims = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d = special_dists(rs, int(lims[-1]))
    ids = rs.randint(0, 2 ** 32, d.size, dtype=np.uint64).astype(np.uint32)
    keep_d, keep_i = d.copy(), ids.copy()
    got_d, got_i = rsr.range_sort_ref(lims, d, ids)
    assert d.tobytes() == keep_d.tobytes() and ids.tobytes() == keep_i.tobytes()   # the inputs stay
    for q, n in enumerate(lens):
        a, b = int(lims[q]), int(lims[q + 1])
        seg = d[a:b]
        key = rsr.key_image(seg)
        o = np.lexsort((np.arange(n), key))
        np.testing.assert_array_equal(rsr.order_by_words(seg), o, err_msg=f"the words' order, segment {q}")
        np.testing.assert_array_equal(got_d[a:b].view(np.uint32), seg[o].view(np.uint32), err_msg=f"dist bits, segment {q}")
        np.testing.assert_array_equal(got_i[a:b], ids[a:b][o], err_msg=f"ids, segment {q}")
        # the order itself: non-NaN values ascend numerically (-0 == +0), every NaN is behind them, bits are moved
        s = got_d[a:b]
        nan = np.isnan(s)
        assert not nan[: n - int(nan.sum())].any() and nan[n - int(nan.sum()):].all()
        assert np.all(s[~nan][:-1] <= s[~nan][1:])
        assert sorted(s.view(np.uint32).tolist()) == sorted(seg.view(np.uint32).tolist())
    k = rsr.key_image(np.asarray([0x80000000, 0, 0x7F800000, 0x7FC00000, 0xFFC00000, 0xFF800000, 0x7F800001], np.uint32).view(np.float32))
    assert k[0] == k[1] == 0x80000000 and k[2] == 0xFF800000 and k[3] == k[4] == k[6] == 0xFFFFFFFF and k[5] == 0x007FFFFF


class _Engine:
    """Stands in for the engine under `li`: records how the range calls were made and returns runs in descending distance."""

    n_classes = 12
    stop_mass = path_mass = 0.0
    stop_rows = 0

    def __init__(self):
        self.calls = []

    def _answer(self, name, qn, kw):
        self.calls.append((name, dict(kw)))
        m = qn.shape[0]
        lims = np.arange(m + 1, dtype=np.int64) * 3
        d = np.tile(np.asarray([3.0, 1.0, 2.0], np.float32), m)
        if kw.get("sort"):
            d = np.tile(np.asarray([1.0, 2.0, 3.0], np.float32), m)
            return lims, d, np.tile(np.asarray([1, 2, 0], np.uint32), m), None, None
        return lims, d, np.tile(np.asarray([0, 1, 2], np.uint32), m), None, None

    def search_range(self, qn, qs, nb, r, filter=None, filter_of=None, max_total=0, **kw):
        return self._answer("search_range", qn, kw)

    def search_tree_range(self, qn, qs, nb, r, filter=None, filter_of=None, max_total=0, **kw):
        return self._answer("search_tree_range", qn, kw)


class _SortingEngine(_Engine):
    range_sort = True

    def search_range(self, qn, qs, nb, r, filter=None, filter_of=None, max_total=0, sort=False):
        return self._answer("search_range", qn, {"sort": sort} if sort else {})

    def search_tree_range(self, qn, qs, nb, r, filter=None, filter_of=None, max_total=0, sort=False):
        return self._answer("search_tree_range", qn, {"sort": sort} if sort else {})


@pytest.mark.parametrize("levels", ([12], [4, 3]))
def test_li_routes_the_sort_to_an_engine_that_has_it(monkeypatch, levels):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    monkeypatch.setattr(LearnedIndex, "_nav_chunk", lambda self: 3)
    monkeypatch.setattr(np, "argsort", lambda *a, **k: (_ for _ in ()).throw(AssertionError("li ordered the results again")))
    Q = np.random.RandomState(0).randn(7, 8).astype(np.float32)
    li = LearnedIndex(None, {}, [])
    li._entry_paths, li._nav_cap = np.zeros((16, 2), np.int32), 16
    eng = li._engine = _SortingEngine()
    name = "search_range" if len(levels) == 1 else "search_tree_range"
    lims, d, n, _ = li.range_search_resident(Q, Q, levels, 0.25, n_buckets=2, sort=True)
    assert eng.calls and all(c == (name, {"sort": True}) for c in eng.calls)
    assert len(eng.calls) == (1 if len(levels) == 1 else 3)   # each piece sorted by its own call
    np.testing.assert_array_equal(lims, np.arange(8) * 3)
    np.testing.assert_array_equal(d, np.tile([1.0, 2.0, 3.0], 7))
    np.testing.assert_array_equal(n, np.tile([1, 2, 0], 7))   # what the engine returned, untouched
    eng.calls.clear()
    li.range_search_resident(Q, Q, levels, 0.25, n_buckets=2)
    assert all(c == (name, {}) for c in eng.calls)   # without sort=True the engine is called as ever


@pytest.mark.parametrize("levels", ([12], [4, 3]))
def test_li_orders_the_results_itself_for_an_engine_without_it(monkeypatch, levels):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    monkeypatch.setattr(LearnedIndex, "_nav_chunk", lambda self: 3)
    Q = np.random.RandomState(0).randn(7, 8).astype(np.float32)
    li = LearnedIndex(None, {}, [])
    li._entry_paths, li._nav_cap = np.zeros((16, 2), np.int32), 16
    eng = li._engine = _Engine()
    lims, d, n, _ = li.range_search_resident(Q, Q, levels, 0.25, n_buckets=2, sort=True)
    assert eng.calls and all(kw == {} for _, kw in eng.calls)   # exactly today's calls: no `sort` keyword reaches it
    np.testing.assert_array_equal(d, np.tile([1.0, 2.0, 3.0], 7))
    np.testing.assert_array_equal(n, np.tile([1, 2, 0], 7))
    # an engine that claims the sort but whose call takes no `sort` is called as ever, too
    eng.range_sort = True
    eng.calls.clear()
    monkeypatch.setattr(eng, "search_range", lambda qn, qs, nb, r, filter=None, filter_of=None, max_total=0: eng._answer("search_range", qn, {}),
                        raising=False)
    monkeypatch.setattr(eng, "search_tree_range",
                        lambda qn, qs, nb, r, filter=None, filter_of=None, max_total=0: eng._answer("search_tree_range", qn, {}), raising=False)
    lims, d, n, _ = li.range_search_resident(Q, Q, levels, 0.25, n_buckets=2, sort=True)
    assert all(kw == {} for _, kw in eng.calls)
    np.testing.assert_array_equal(n, np.tile([1, 2, 0], 7))


def test_driver_flag():
    from learnedmetricindex_amd.search import Experiment

    assert Experiment.from_argv(["--n-categories", "12", "--range-radius", "0.3"]).range_sort is False
    assert Experiment.from_argv(["--n-categories", "12", "--range-radius", "0.3", "--range-sort"]).range_sort is True
    with pytest.raises(SystemExit):
        Experiment.from_argv(["--n-categories", "12", "--range-sort"])
