"""CPU (`-m "not gpu"`): the host side of `lmi_concat`.  The two entry points are exported and bound and the plan enum matches
`_capi.CONCAT_PLAN_FIELDS`; `Index.concat` refuses bad arguments before the library is loaded; `LearnedIndex.concat` and `extended`
route as documented against a recording stand-in for the library (the bucket-path refusal, the placement shared with `insert`, the
small index closed also when the concatenation fails); and the pure planning header (csrc/lmi_concat_plan.h) passes its stand-alone
self-test under AddressSanitizer + UBSan."""
import ctypes
import gc
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from learnedmetricindex_amd import _capi
from test_f16_inputs_host import Recorder
from test_regroup_host import net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_concat_symbols_exported_and_bound():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in (("lmi_concat", 4), ("lmi_debug_concat_plan", 2)):
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = fh.read()
    words = header.split("LMI_CONCAT_PLAN_PARTS = 0")[1].split("LMI_CONCAT_PLAN_COUNT")[0]
    assert _capi.CONCAT_PLAN_FIELDS[0] == "PARTS"
    assert list(_capi.CONCAT_PLAN_FIELDS[1:]) == [ln.split(",")[0].strip()[len("LMI_CONCAT_PLAN_"):] for ln in words.splitlines()[1:]
                                                  if "LMI_CONCAT_PLAN_" in ln]
    assert f"#define LMI_CONCAT_MAX_PARTS {_capi.CONCAT_MAX_PARTS}\n" in header
    with open(os.path.join(ROOT, "learnedmetricindex_amd", "csrc", "lmi_concat_plan.h")) as fh:
        assert f"constexpr int MAX_PARTS = {_capi.CONCAT_MAX_PARTS};" in fh.read()
    assert callable(_capi.Index.concat) and callable(_capi.concat_last_plan)
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    assert callable(LearnedIndex.concat)
    assert list(inspect.signature(LearnedIndex.extended).parameters) == ["self", "data_navigation_new", "data_search_new", "ids"]


def bare(handle=1):
    idx = object.__new__(_capi.Index)
    idx._h, idx._views = ctypes.c_void_p(handle), []
    return idx


def test_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    idx, other = bare(1), bare(2)
    try:
        for bad in (None, 7, "index", np.zeros(3), object()):
            with pytest.raises(ValueError, match="part 2 must be an Index"):
                idx.concat(other, bad)
        closed = bare(3)
        closed._h = None
        with pytest.raises(ValueError, match="part 1 is closed"):
            idx.concat(closed)
        with pytest.raises(ValueError, match="part 3 is closed"):
            idx.concat(other, other, bare(0))          # a NULL handle
        with pytest.raises(ValueError, match=r"65 parts \(this index and 64 others\), at most 64"):
            idx.concat(*[other] * 64)
        assert _capi.concat_args(idx, [other] * 63)[0] is idx and len(_capi.concat_args(idx, [other] * 63)) == 64
        assert _capi.concat_args(idx, []) == [idx]
    finally:
        idx._h = other._h = None                       # (no handle to destroy)


class Concatter(Recorder):
    """The stand-in with an `lmi_create` that hands out handles and an `lmi_concat` that reads the handles it is given."""

    def __init__(self):
        super().__init__()
        self.seen, self.made, self.fail_concat = [], 0x1000, False

    def lmi_create(self, device, out):
        self.calls.append(("lmi_create", (device, out)))
        self.made += 1
        out._obj.value = self.made
        return 0

    def lmi_buckets_begin(self, h, N, d, L, labels, ids, owned):
        self.calls.append(("lmi_buckets_begin", (h, N, d, L, labels, ids, owned)))
        self.begun = (np.ctypeslib.as_array(ctypes.cast(labels, ctypes.POINTER(ctypes.c_int64)), shape=(N,)).copy(),
                      np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_uint32)), shape=(N,)).copy())
        return 0

    def lmi_concat(self, handles, n, out, total):
        self.calls.append(("lmi_concat", (handles, n, out, total)))
        self.seen.append([handles[t] for t in range(n)])
        if self.fail_concat:
            return -1
        out._obj.value = 0xBEEF0 + len(self.seen)
        total._obj.value = 100 * n
        return 0

    def lmi_last_error(self):
        return b"lmi_concat: LMI_STORAGE_F16 refused: stand-in"


@pytest.fixture
def engine(monkeypatch):
    made = []

    def make(rec, handle, L=3, storage="f32", metric="ip"):
        monkeypatch.setattr(_capi, "_lib", rec)
        idx = _capi.Index.__new__(_capi.Index)
        idx._h, idx._views = ctypes.c_void_p(handle), []
        idx.device, idx.n_classes, idx.d_nav, idx.d, idx.L, idx.N, idx.bytes_in = 0, L, 16, 8, L, 20, 0
        idx.metric, idx.storage, idx.stop_mass, idx.path_mass, idx.stop_rows = metric, storage, 0.0, 0.0, 0
        made.append(idx)
        return idx

    yield make
    for idx in made:
        idx._h = None
    gc.collect()


def test_index_concat_marshals(engine):
    rec = Concatter()
    a, b, c = engine(rec, 1, storage="f16"), engine(rec, 2), engine(rec, 3)
    out = a.concat(b, c, b)
    assert rec.seen[-1] == [1, 2, 3, 2] and rec.calls[-1][1][1] == 4               # the receiver is parts[0]
    assert isinstance(out, _capi.Index) and out is not a and out._h.value == 0xBEEF1 and out.N == 400 and out.bytes_in == 0
    assert out.storage == "f16" and out.L == a.L and out.d == a.d and out.metric == a.metric   # it describes the receiver
    assert out not in a._views and not hasattr(out, "_parent")                     # an owning Index, not a view
    alone = a.concat()
    assert rec.seen[-1] == [1] and alone.N == 100
    for x in (out, alone):
        x.close()


def li_over(eng, paths, path_ids=None, root=None, internal=None):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    li = LearnedIndex(root if root is not None else net(16, 3), internal or {}, list(paths))
    li._engine, li._engine_key, li._path_ids = eng, ("k",), path_ids
    return li


def test_li_concat_routes_and_refuses_other_bucket_paths(engine):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Concatter()
    one = [(0,), (1,), (2,)]
    li, a, b = li_over(engine(rec, 1), one), li_over(engine(rec, 2), one), li_over(engine(rec, 3), [[0], [1], [2]])   # (lists or tuples: the same paths)
    out = li.concat(a, b)
    assert rec.seen[-1] == [1, 2, 3]
    assert out.root_model is li.root_model and out.internal_models is li.internal_models and out.bucket_paths is li.bucket_paths
    assert out._engine is not li._engine and out._engine_key[0] == "mutated" and li._engine_key == ("k",) and out._path_ids is None
    n_before = len(rec.seen)
    with pytest.raises(ValueError, match="argument 1 has other bucket_paths"):
        li.concat(a, li_over(engine(rec, 4), one + [(3,)]))
    with pytest.raises(ValueError, match="argument 0 has other bucket_paths"):
        li.concat(li_over(engine(rec, 5), [(0,), (2,), (1,)]))                     # the same set in another order
    ids = {(0, 0): 0, (0, 1): 1, (1, -1): 2}
    two = li_over(engine(rec, 6), list(ids), dict(ids))
    with pytest.raises(ValueError, match="argument 0 has other bucket_paths"):     # the same listed paths, other bucket ids
        two.concat(li_over(engine(rec, 7), list(ids), {(0, 0): 0, (1, -1): 1, (0, 1): 2}))
    with pytest.raises(ValueError, match="argument 0 has no resident index"):
        li.concat(LearnedIndex(li.root_model, {}, one))
    with pytest.raises(ValueError, match="argument 1 must be a LearnedIndex"):
        li.concat(a, a._engine)
    assert len(rec.seen) == n_before, "a refused call reached the library"
    ok = two.concat(li_over(engine(rec, 8), list(ids), dict(ids)))
    assert rec.seen[-1] == [6, 8] and ok._path_ids == ids
    for x in (out, ok):
        x.close()
    for x in (li, a, b, two):
        x._engine = None


def test_li_extended_places_like_insert_and_closes_the_small_index(engine, monkeypatch):
    import pandas as pd

    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Concatter()
    root, child = net(16, 2), net(16, 2, 1)
    ids = {(0, 0): 0, (0, 1): 1, (1, -1): 2}
    li = li_over(engine(rec, 1, storage="f16"), list(ids), dict(ids), root=root, internal={(0, -1): child})
    li._entry_paths, li._nav_cap = np.zeros((4, 2), np.int32), 4
    monkeypatch.setattr(root, "predict", lambda x: (np.arange(x.shape[0]) % 2 == 1).astype(np.int64))   # objects 0, 2 -> node 0; 1 -> leaf (1,)
    monkeypatch.setattr(child, "predict", lambda x: np.ones(x.shape[0], dtype=np.int64))                # node 0's objects -> (0, 1)
    frame = pd.DataFrame(np.arange(24, dtype=np.float16).reshape(3, 8), index=[101, 102, 103])
    placed = []
    real = LearnedIndex._place
    monkeypatch.setattr(LearnedIndex, "_place", lambda self, *a, **k: placed.append(a) or real(self, *a, **k))
    new, dp = li.extended(frame)
    assert len(placed) == 1                                                        # insert's placement, not a copy of it
    assert dp.tolist() == [[0, 1], [1, -1], [0, 1]]
    names = [n for n, _ in rec.calls]
    order = [names.index(n) for n in ("lmi_create", "lmi_set_storage", "lmi_buckets_begin", "lmi_buckets_add_rows_f16", "lmi_buckets_end",
                                      "lmi_concat", "lmi_destroy")]
    assert order == sorted(order), names                                           # a float16 frame goes up as halves
    small = rec.made
    begin = rec.calls[names.index("lmi_buckets_begin")][1]
    assert begin[0].value == small and begin[1:4] == (3, 8, 3)                     # N, d, L of the resident engine
    lab, got_ids = rec.begun
    assert list(lab) == [1, 2, 1] and list(got_ids) == [101, 102, 103] and begin[6] is None
    assert rec.calls[names.index("lmi_set_storage")][1][1] == _capi.Index.STORAGES["f16"]
    assert rec.seen[-1] == [1, small]                                              # the resident engine first, then the small index
    assert rec.calls[names.index("lmi_destroy")][1][0].value == small and names.count("lmi_destroy") == 1
    assert new is not li and new._engine._h.value == 0xBEEF1 and new._engine.storage == "f16" and new._path_ids == ids
    assert new.bucket_paths is li.bucket_paths and new._engine_key[0] == "mutated"
    assert li._engine._h.value == 1 and li._engine_key == ("k",)                   # this object is unchanged
    # insert goes through the same placement
    li._engine.storage = "f32"
    li.insert(frame)
    assert len(placed) == 2 and rec.calls[-1][0] == "lmi_buckets_insert_f16"
    li._engine.storage = "f16"
    # a leaf path that holds no bucket: refused before anything is made, as in insert without create_buckets
    monkeypatch.setattr(child, "predict", lambda x: np.full(x.shape[0], 0, dtype=np.int64))
    del li._path_ids[(0, 0)]
    n_calls = len(rec.calls)
    with pytest.raises(ValueError, match=r"2 of 3 object\(s\) fall on a leaf path that holds no bucket"):
        li.extended(frame)
    assert len(rec.calls) == n_calls
    li._path_ids[(0, 0)] = 0
    # the concatenation is refused: the small index is closed all the same, this object keeps its engine
    rec.fail_concat = True
    with pytest.raises(_capi.LmiError, match="LMI_STORAGE_F16 refused"):
        li.extended(frame)
    tail = [n for n, _ in rec.calls[n_calls:]]
    assert tail[0] == "lmi_create" and tail[-2:] == ["lmi_concat", "lmi_destroy"]
    assert rec.calls[-1][1][0].value == rec.made and li._engine._h.value == 1
    new.close()
    li._engine = None


def test_concat_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "concat_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "concat_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "concat plan selftest: clean" in r.stdout
