"""CPU (`-m "not gpu"`): the host side of the fetch of stored objects by id (lmi_rows_fetch).  The entry points are
exported, declared and bound and the plan enum matches `_capi.FETCH_PLAN_FIELDS`; the bindings refuse bad arguments before the library
is loaded; the plan's arithmetic (csrc/lmi_fetch_plan.h, pure host code) passes its stand-alone self-test under AddressSanitizer +
UBSan; `li` routes `reconstruct` and `search_like` to an engine as documented; the sharded join picks the owning rank's row."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from learnedmetricindex_amd import _capi, sharded

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = (("lmi_rows_fetch", 7), ("lmi_rows_fetch_f16", 7), ("lmi_fetch_set_geometry", 1), ("lmi_debug_fetch_plan", 2))
WORDS = ["REQUESTS", "UNIQUE", "PIECES", "PIECE_ROWS", "FOUND", "FORM", "WORKSPACE_BYTES"]


def test_fetch_symbols_exported_and_bound():
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
    words = re.findall(r"\bLMI_FETCH_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", header)
    assert words[-1] == "COUNT" and list(_capi.FETCH_PLAN_FIELDS) == words[:-1] == WORDS
    assert re.search(r"#define LMI_ABI_VERSION 1\b", text)
    for name in ("fetch", "locate", "fetch_device"):
        assert callable(getattr(_capi.Index, name))
    assert callable(_capi.fetch_set_geometry) and callable(_capi.fetch_last_plan)
    import inspect

    p = inspect.signature(_capi.Index.fetch).parameters
    assert p["dtype"].default is np.float32 and p["rows_out"].default is None and p["where"].default is False


def _handles():
    closed = object.__new__(_capi.Index)
    closed._h = None
    live = object.__new__(_capi.Index)
    live._h, live.d = ctypes.c_void_p(1), 8
    return closed, live


def test_fetch_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    closed, live = _handles()
    for bad in ([-1], [2 ** 32], [1, 2 ** 40], np.asarray([1.0, 2.0]), ["a"], [1.5]):
        with pytest.raises(ValueError):
            live.fetch(bad)
        with pytest.raises(ValueError):
            live.locate(bad)
    for bad in (np.float64, np.int32, "bfloat16", None, object()):
        with pytest.raises(ValueError):
            live.fetch([1, 2], dtype=bad)
    for bad in (np.empty((2, 8), np.float16), np.empty((3, 8), np.float32), np.empty((2, 9), np.float32), np.empty((8, 2), np.float32).T,
                [[0.0] * 8] * 2):
        with pytest.raises(ValueError):
            live.fetch([1, 2], rows_out=bad)
    with pytest.raises(ValueError):
        closed.fetch([1])
    with pytest.raises(ValueError):
        closed.locate([1])
    with pytest.raises(ValueError):
        closed.fetch_device(torch.zeros(3, dtype=torch.int32))
    for bad in (-1, (1 << 24) + 1, 1.0, None, True, "8"):
        with pytest.raises(ValueError):
            _capi.fetch_set_geometry(piece_rows=bad)
    # device tensors: wrong place, wrong dtype, wrong shape, nothing asked for
    ids = torch.zeros(3, dtype=torch.int32)
    for args in ((ids,), (ids, torch.zeros((3, 8))), (np.zeros(3, np.uint32), None, ids), (torch.zeros((3, 1), dtype=torch.int32),)):
        with pytest.raises(ValueError):
            live.fetch_device(*args)
    # the accepted forms reach the library (and only then fail, on the stand-in that forbids it)
    for good in ([0, 2 ** 32 - 1], np.asarray([3, 3, 1], np.int64), np.asarray([], np.int64), [], (5,)):
        with pytest.raises(AssertionError, match="library was loaded"):
            live.fetch(good)


def test_fetch_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fetch_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "fetch_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "fetch plan selftest: clean" in r.stdout


class _Engine:
    """Stands in for the engine under `li`: holds objects 10, 20, 30 (vector = id in every column) and records its calls."""

    device = 0
    n_classes = 12
    stop_mass = path_mass = 0.0
    stop_rows = 0
    T = np.zeros(_capi.T_COUNT, np.float32)

    def __init__(self, d=4, d_nav=4):
        self.d, self.d_nav, self.calls = d, d_nav, []
        self._h = ctypes.c_void_p(1)

    def _rows(self, ids, dtype):
        ids = np.asarray(ids).reshape(-1)
        found = np.isin(ids, [10, 20, 30])
        rows = np.where(found[:, None], ids[:, None].astype(np.float64), 0.0) * np.ones((1, self.d))
        return rows.astype(dtype), np.where(found, ids // 10, -1).astype(np.int32), np.where(found, 0, -1).astype(np.int32)

    def fetch(self, ids, dtype=np.float32, rows_out=None, where=False):
        self.calls.append(("fetch", np.dtype(dtype), where))
        out = self._rows(ids, dtype)
        return out if where else out[0]

    def fetch_device(self, ids_t, rows_t=None, bucket_t=None, row_t=None):
        self.calls.append(("fetch_device", rows_t, bucket_t))
        rows, bucket, _ = self._rows(ids_t.numpy().view(np.uint32), np.float32)
        rows_t.copy_(torch.from_numpy(rows))
        bucket_t.copy_(torch.from_numpy(bucket))

    def workspace_bytes(self, nq, nb):
        return 1024 * (1 + nq)

    def timings(self):
        return self.T

    def _answer(self, name, qn_t, qs_t, d_t, i_t, kw):
        self.calls.append((name, qn_t, qs_t, kw))
        d_t.copy_(qs_t[:, :1].expand_as(d_t))
        i_t.fill_(7)

    def search_device(self, qn_t, qs_t, nb, k, d_t, i_t, keys_t=None, bo_t=None):
        self._answer("search_device", qn_t, qs_t, d_t, i_t, {})

    def search_tree_device(self, qn_t, qs_t, nb, k, d_t, i_t, keys_t=None, slab_t=None, ent_t=None):
        self._answer("search_tree_device", qn_t, qs_t, d_t, i_t, {})

    def search_union_device(self, qn_t, qs_t, nb, k, d_t, i_t, counts_t=None, bo_t=None, filter=None, filter_of=None):
        self._answer("search_union_device", qn_t, qs_t, d_t, i_t, {"filter": filter})

    def search_tree_union_device(self, qn_t, qs_t, nb, k, d_t, i_t, counts_t=None, slab_t=None, ent_t=None, filter=None, filter_of=None):
        self._answer("search_tree_union_device", qn_t, qs_t, d_t, i_t, {"filter": filter})


def _li(monkeypatch, eng):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    monkeypatch.setattr(LearnedIndex, "_nav_chunk", lambda self: 2)
    monkeypatch.setattr(LearnedIndex, "_torch_device", staticmethod(lambda e: torch.device("cpu")))
    li = LearnedIndex(None, {}, [])
    li._entry_paths, li._nav_cap = np.zeros((16, 2), np.int32), 16
    li._engine = eng
    return li


def test_li_reconstruct_honours_both_missing_modes(monkeypatch):
    eng = _Engine()
    li = _li(monkeypatch, eng)
    rows = li.reconstruct([30, 10, 30])
    np.testing.assert_array_equal(rows, np.asarray([[30.0] * 4, [10.0] * 4, [30.0] * 4], np.float32))
    assert rows.dtype == np.float32 and eng.calls[-1] == ("fetch", np.dtype(np.float32), True)
    assert li.reconstruct([20], dtype=np.float16).dtype == np.float16
    with pytest.raises(KeyError, match=r"\[11, 12\]"):
        li.reconstruct([10, 12, 11, 12])
    many = list(range(100, 125))
    with pytest.raises(KeyError, match="and 15 more"):
        li.reconstruct(many)
    rows, found = li.reconstruct([10, 11, 30], missing="zero")
    np.testing.assert_array_equal(found, [True, False, True])
    np.testing.assert_array_equal(rows[1], np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        li.reconstruct([10], missing="skip")
    li._engine = None
    with pytest.raises(AssertionError, match="no resident index"):
        li.reconstruct([10])


@pytest.mark.parametrize("levels", ([12], [4, 3]))
@pytest.mark.parametrize("merge", ("ranks", "union"))
def test_li_search_like_hands_the_fetched_tensor_on(monkeypatch, levels, merge):
    eng = _Engine()
    li = _li(monkeypatch, eng)
    dists, nns, mt = li.search_like([30, 10, 20], levels, n_buckets=2, k=5, merge=merge)
    fetched = [c for c in eng.calls if c[0] == "fetch_device"]
    assert len(fetched) == 1
    rows_t = fetched[0][1]
    name = {("ranks", 1): "search_device", ("ranks", 2): "search_tree_device", ("union", 1): "search_union_device",
            ("union", 2): "search_tree_union_device"}[(merge, len(levels))]
    searches = [c for c in eng.calls if c[0] != "fetch_device"]
    assert searches and all(c[0] == name for c in searches)
    assert len(searches) == (1 if len(levels) == 1 else 2)   # a multi-level index is walked in pieces of _nav_chunk() queries
    base = rows_t.untyped_storage().data_ptr()
    for c in searches:   # the very memory the fetch wrote, for navigation and for the scan
        assert c[1].untyped_storage().data_ptr() == base and c[2].untyped_storage().data_ptr() == base
    assert searches[0][1].data_ptr() == rows_t.data_ptr()
    np.testing.assert_array_equal(dists[:, 0], [30.0, 10.0, 20.0])
    assert dists.dtype == np.float64 and nns.dtype == np.uint32 and (nns == 7).all() and "search" in mt


def test_li_search_like_needs_navigation_queries_when_the_widths_differ(monkeypatch):
    eng = _Engine(d=4, d_nav=6)
    li = _li(monkeypatch, eng)
    with pytest.raises(ValueError, match="queries_navigation"):
        li.search_like([10, 20], [12])
    assert not eng.calls   # refused before anything was fetched
    with pytest.raises(ValueError):
        li.search_like([10, 20], [12], queries_navigation=np.zeros((3, 6), np.float32))
    QN = np.arange(12, dtype=np.float32).reshape(2, 6)
    dists, _, _ = li.search_like([10, 20], [12], queries_navigation=QN)
    call = [c for c in eng.calls if c[0] == "search_device"][0]
    np.testing.assert_array_equal(call[1].numpy(), QN)
    rows_t = [c for c in eng.calls if c[0] == "fetch_device"][0][1]
    assert call[2].data_ptr() == rows_t.data_ptr()
    np.testing.assert_array_equal(dists[:, 0], [10.0, 20.0])
    with pytest.raises(KeyError, match=r"\[11\]"):
        li.search_like([10, 11], [12], queries_navigation=QN)
    with pytest.raises(ValueError):
        li.search_like([10], [12], queries_navigation=QN[:1], merge="best")
    with pytest.raises(TypeError):
        li.search_like([10], [12], queries_navigation=QN[:1], sort=True)


class _Rank:
    def __init__(self, rank, world, owns):
        self.rank, self.world, self.owns = rank, world, owns

    fetch_part = sharded.ShardedSearcher.fetch_part
    reconstruct = sharded.ShardedSearcher.reconstruct
    join_fetch_parts = staticmethod(sharded.ShardedSearcher.join_fetch_parts)

    @property
    def index(self):
        return self

    def fetch(self, ids, dtype=np.float32, where=False):
        ids = np.asarray(ids).reshape(-1)
        mine = np.isin(ids, list(self.owns))
        rows = np.where(mine[:, None], ids[:, None], 0).astype(dtype) * np.ones((1, 3), dtype)
        bucket = np.asarray([self.owns.get(int(v), (-1, -1))[0] for v in ids], np.int32)
        row = np.asarray([self.owns.get(int(v), (-1, -1))[1] for v in ids], np.int32)
        return rows, bucket, row


def test_sharded_join_takes_each_row_from_the_rank_that_holds_it():
    # id 5 is carried on rank 0 (bucket 4) and on rank 2 (bucket 1, rows 3): one handle would answer (1, 3), rank 2's
    ranks = [_Rank(0, 3, {1: (0, 0), 5: (4, 0)}), _Rank(1, 3, {2: (2, 7)}), _Rank(2, 3, {3: (1, 0), 5: (1, 3)})]
    ids = [3, 1, 2, 2, 5]
    for me in range(3):
        rows = ranks[me].reconstruct(ids, peers=[r for r in ranks if r is not ranks[me]])
        np.testing.assert_array_equal(rows[:, 0], [3, 1, 2, 2, 5])
    parts = [r.fetch_part(ids) for r in ranks]
    parts[0][0][4] = 50.0   # rank 0's copy of id 5 must lose to rank 2's
    np.testing.assert_array_equal(sharded.ShardedSearcher.join_fetch_parts(ids, parts)[:, 0], [3, 1, 2, 2, 5])
    with pytest.raises(KeyError, match=r"\[9\]"):
        ranks[0].reconstruct([1, 9], peers=ranks[1:])
    with pytest.raises(ValueError, match="peers"):
        ranks[0].reconstruct([1])
    assert ranks[1].reconstruct([], peers=[ranks[0], ranks[2]]).shape == (0, 3)
