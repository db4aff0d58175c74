"""CPU (`-m "not gpu"`): the host side of `lmi_regroup`.  The three entry points are exported and bound and the plan enum matches
`_capi.REGROUP_PLAN_FIELDS`; `Index.regroup` refuses bad arguments before the library is loaded; `LearnedIndex.regroup` and
`insert(create_buckets=True)` route (path set, sorted ids, bucket_map, padding) as documented, against a recording stand-in for the
library; the order rule in numpy (tests/regroup_ref.py, the GPU test's reference) says what its plain statement says; and the pure
planning header (csrc/lmi_regroup_plan.h) passes its stand-alone self-test under AddressSanitizer + UBSan."""
import ctypes
import gc
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import regroup_ref as rr
from learnedmetricindex_amd import _capi
from test_f16_inputs_host import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_regroup_symbols_exported_and_bound():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in (("lmi_regroup", 8), ("lmi_regroup_set_geometry", 1), ("lmi_debug_regroup_plan", 2)):
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = fh.read()
    words = header.split("LMI_REGROUP_PLAN_ROWS = 0")[1].split("LMI_REGROUP_PLAN_COUNT")[0]
    assert _capi.REGROUP_PLAN_FIELDS[0] == "ROWS"
    assert list(_capi.REGROUP_PLAN_FIELDS[1:]) == [ln.split(",")[0].strip()[len("LMI_REGROUP_PLAN_"):] for ln in words.splitlines()[1:]
                                                   if "LMI_REGROUP_PLAN_" in ln]
    assert callable(_capi.Index.regroup) and callable(_capi.regroup_set_geometry) and callable(_capi.regroup_last_plan)
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    assert callable(LearnedIndex.regroup)
    assert inspect.signature(LearnedIndex.insert).parameters["create_buckets"].default is False


def test_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    idx = object.__new__(_capi.Index)   # no handle: nothing below may reach the library
    idx.L = 4
    ok_ids, ok_lab = [5, 6, 7], [0, 1, 5]
    for L_new in (0, -3, 1 << 20, 2.0, None, True):
        with pytest.raises(ValueError, match="L_new"):
            idx.regroup(ok_ids, ok_lab, L_new)
    with pytest.raises(ValueError, match="3 ids but 2 labels"):
        idx.regroup(ok_ids, [0, 1], 6)
    with pytest.raises(ValueError, match="integers"):
        idx.regroup([1.5, 2.0, 3.0], ok_lab, 6)
    with pytest.raises(ValueError, match="integers"):
        idx.regroup(ok_ids, [0.0, 1.0, 2.0], 6)
    for bad in ([1, 2, 2 ** 32], [-1, 2, 3]):
        with pytest.raises(ValueError, match="uint32"):
            idx.regroup(bad, ok_lab, 6)
    with pytest.raises(ValueError, match=r"labels\[2\] = 5 outside \[0, 5\)"):
        idx.regroup(ok_ids, ok_lab, 5)
    with pytest.raises(ValueError, match=r"labels\[0\] = -1"):
        idx.regroup(ok_ids, [-1, 0, 0], 6)
    with pytest.raises(ValueError, match="id 6 is listed twice"):
        idx.regroup([5, 6, 7, 6], [0, 1, 2, 3], 6)
    with pytest.raises(ValueError, match="needs L_new >= L"):
        idx.regroup(ok_ids, [0, 1, 2], 3)
    for bad_map in ([0, 1, 2], [0, 1, 2, 3, 4], [0.0, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="bucket_map must be 4 integers"):
            idx.regroup(ok_ids, ok_lab, 6, bucket_map=bad_map)
    with pytest.raises(ValueError, match=r"bucket_map\[1\] = -2"):
        idx.regroup(ok_ids, ok_lab, 6, bucket_map=[0, -2, 1, 1])
    with pytest.raises(ValueError, match=r"bucket_map\[3\] = 6"):
        idx.regroup(ok_ids, ok_lab, 6, bucket_map=[0, -1, 1, 6])
    for bad_t in (-64, 32, 96, 16384, 64.0, True):
        with pytest.raises(ValueError):
            _capi.regroup_set_geometry(bad_t)
    # what passes: the arrays as the library takes them
    ids_a, lab_a, map_a, L_new = _capi.regroup_args(np.asarray([[9, 4], [2 ** 32 - 1, 1]])[:, ::-1], [[1, 0], [2, 2]], 3, [2, -1, 0, 1], 4)
    assert ids_a.dtype == np.uint32 and ids_a.flags.c_contiguous and list(ids_a) == [4, 9, 1, 2 ** 32 - 1]
    assert lab_a.dtype == np.int64 and list(lab_a) == [1, 0, 2, 2] and map_a.dtype == np.int32 and list(map_a) == [2, -1, 0, 1] and L_new == 3
    assert _capi.regroup_args([], [], 4, None, 4)[2] is None


class Regrouper(Recorder):
    """The stand-in with an `lmi_regroup` that reads what it is handed and writes a handle and a count."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def lmi_regroup(self, h, ids, labels, n, bucket_map, L_new, out, n_named):
        self.calls.append(("lmi_regroup", (h, ids, labels, n, bucket_map, L_new, out, n_named)))
        got_ids = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).copy() if n else np.empty(0, np.uint32)
        got_lab = np.ctypeslib.as_array(ctypes.cast(labels, ctypes.POINTER(ctypes.c_int64)), shape=(n,)).copy() if n else np.empty(0, np.int64)
        L = self.L_of[h.value]
        got_map = None if not bucket_map else np.ctypeslib.as_array(ctypes.cast(bucket_map, ctypes.POINTER(ctypes.c_int32)), shape=(L,)).copy()
        self.seen.append((got_ids, got_lab, got_map, L_new))
        out._obj.value = 0xBEEF0 + len(self.seen)
        self.L_of[out._obj.value] = L_new
        n_named._obj.value = n
        return 0


@pytest.fixture
def engine(monkeypatch):
    made = []

    def make(rec, L):
        monkeypatch.setattr(_capi, "_lib", rec)
        idx = _capi.Index.__new__(_capi.Index)
        idx._h, idx._views = ctypes.c_void_p(1), []
        idx.device, idx.n_classes, idx.d_nav, idx.d, idx.L, idx.N, idx.bytes_in = 0, 3, 16, 8, L, 20, 0
        idx.metric, idx.storage, idx.stop_mass, idx.path_mass, idx.stop_rows = "ip", "f32", 0.0, 0.0, 0
        rec.L_of = {1: L}
        made.append(idx)
        return idx

    yield make
    for idx in made:
        idx._h = None
    gc.collect()


def net(d, classes, seed=0):
    from learnedmetricindex_amd.li.model import NeuralNetwork

    import torch

    torch.manual_seed(seed)
    return NeuralNetwork(input_dim=d, output_dim=classes, model_type="MLP")


def test_index_regroup_marshals(engine):
    rec = Regrouper()
    idx = engine(rec, 4)
    out = idx.regroup([9, 4, 7], [5, 0, 5], 6, bucket_map=[0, -1, 2, 3])
    ids, lab, bmap, L_new = rec.seen[-1]
    assert list(ids) == [9, 4, 7] and list(lab) == [5, 0, 5] and list(bmap) == [0, -1, 2, 3] and L_new == 6
    assert isinstance(out, _capi.Index) and out is not idx and out.L == 6 and idx.L == 4 and out.n_named == 3 and out.N == 20
    assert out not in idx._views and not hasattr(out, "_parent")   # an owning Index, not a view
    same = idx.regroup([], [], 4)
    assert rec.seen[-1][2] is None and rec.calls[-1][1][3] == 0 and same.n_named == 0
    same.close()
    out.close()


def test_li_regroup_one_level(engine):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Regrouper()
    eng = engine(rec, 5)
    root5, root7, root3 = net(16, 5), net(16, 7, 1), net(16, 3, 2)
    li = LearnedIndex(root5, {}, [(i,) for i in range(5)])
    li._engine, li._engine_key = eng, ("some", "key")
    with pytest.raises(ValueError, match="one path per id"):
        li.regroup([1, 2], [0])
    new = li.regroup([11, 12], [6, 0], root_model=root7)
    ids, lab, bmap, L_new = rec.seen[-1]
    assert list(ids) == [11, 12] and list(lab) == [6, 0] and bmap is None and L_new == 7   # the new root's classes; identity for the rest
    names = [n for n, _ in rec.calls]
    assert names[names.index("lmi_regroup") + 1] == "lmi_set_mlp"                          # the new model goes onto the new engine
    assert new.root_model is root7 and new.internal_models is li.internal_models and new.bucket_paths is li.bucket_paths
    assert new._engine is not eng and new._engine.L == 7 and new._engine.n_classes == 7 and new._path_ids is None
    assert new._engine_key[0] == "mutated" and li._engine_key == ("some", "key") and li._engine is eng and li.root_model is root5
    fewer = li.regroup([11], np.asarray([[2]]), root_model=root3)                           # fewer classes: buckets 3, 4 must be emptied
    assert list(rec.seen[-1][2]) == [0, 1, 2, -1, -1] and rec.seen[-1][3] == 3
    for x in (new, fewer):
        x.close()
    li._engine = None


def test_li_regroup_multi_level_paths_ids_map_and_padding(engine):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Regrouper()
    paths = [(0, 0), (0, 2), (1, 1), (2, 0)]                      # the resident buckets, ids 0..3 in sorted order
    eng = engine(rec, 4)
    root, child, deeper = net(16, 3), net(16, 3, 1), net(16, 2, 2)
    internal = {(0, -1): child}
    li = LearnedIndex(root, internal, paths + [(1, 0)])           # a listed path that holds no bucket yet
    li._engine, li._engine_key = eng, ("k",)
    li._path_ids = {p: i for i, p in enumerate(paths)}
    li._entry_paths, li._nav_cap = np.zeros((6, 2), np.int32), 6
    # same depth: one object to an existing path, one to a new one
    same = li.regroup([70, 71], [[2, 0], [1, 0]])
    ids, lab, bmap, L_new = rec.seen[-1]
    want = [(0, 0), (0, 2), (1, 0), (1, 1), (2, 0)]               # np.unique(axis=0) of old paths U named paths
    assert L_new == 5 and same._path_ids == {p: i for i, p in enumerate(want)}
    assert list(bmap) == [0, 1, 3, 4] and list(lab) == [4, 2] and list(ids) == [70, 71]
    names = [n for n, _ in rec.calls]
    after = names[names.index("lmi_regroup") + 1:]
    assert after[0] == "lmi_set_mlp" and "lmi_nav_set_model" in after and after[-1] == "lmi_nav_set_tree"
    assert same._entry_paths.shape == (6, 2) and same._nav_cap == 6 and li._path_ids == {p: i for i, p in enumerate(paths)}
    # a level deeper: bucket (0, 2) is split by a child model; the old paths are padded with EMPTY_VALUE and (0, 2, -1) stays, empty
    internal3 = {(0, -1, -1): child, (0, 2, -1): deeper}
    paths3 = [(0, 0, -1), (0, 2, 0), (0, 2, 1), (1, 1, -1), (2, 0, -1), (1, 0, -1)]
    deep = li.regroup([5, 6, 7], [[0, 2, 1], [0, 2, 0], [0, 2, 1]], internal_models=internal3, bucket_paths=paths3)
    ids, lab, bmap, L_new = rec.seen[-1]
    want3 = [(0, 0, -1), (0, 2, -1), (0, 2, 0), (0, 2, 1), (1, 1, -1), (2, 0, -1)]
    assert L_new == 6 and deep._path_ids == {p: i for i, p in enumerate(want3)}
    assert list(bmap) == [0, 1, 4, 5] and list(lab) == [3, 2, 3]
    assert deep._entry_paths.shape[1] == 3 and deep.internal_models is internal3 and deep.bucket_paths is paths3
    with pytest.raises(ValueError, match="1 level"):
        li.regroup([5], [[1]])
    for x in (same, deep):
        x.close()
    li._engine = None


def test_li_insert_create_buckets_routes_through_regroup(engine, monkeypatch):
    import pandas as pd

    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Regrouper()
    paths = [(0, 0), (0, 1), (1, -1)]
    eng = engine(rec, 3)
    root, child = net(16, 2), net(16, 2, 1)
    li = LearnedIndex(root, {(0, -1): child}, list(paths))
    li._engine, li._engine_key = eng, ("k",)
    li._path_ids = {(0, 0): 0, (1, -1): 1}                        # (0, 1) is listed but holds no bucket
    li._entry_paths, li._nav_cap = np.zeros((4, 2), np.int32), 4
    monkeypatch.setattr(root, "predict", lambda x: np.zeros(x.shape[0], dtype=np.int64))
    monkeypatch.setattr(child, "predict", lambda x: np.ones(x.shape[0], dtype=np.int64))
    rec.L_of[1] = 2
    eng.L = 2
    frame = pd.DataFrame(np.zeros((3, 8), np.float32), index=[101, 102, 103])
    with pytest.raises(ValueError, match=r"3 of 3 object\(s\) fall on a leaf path that holds no bucket; creating buckets is not "
                                         r"supported \(rebuild the index\): nothing was inserted"):
        li.insert(frame)
    assert not any(n == "lmi_regroup" for n, _ in rec.calls) and li._engine is eng
    dp = li.insert(frame, create_buckets=True)
    assert dp.tolist() == [[0, 1]] * 3
    ids, lab, bmap, L_new = rec.seen[-1]
    assert ids.size == 0 and L_new == 3 and list(bmap) == [0, 2]  # (0, 1) opens between the two: no object is named
    assert li._path_ids == {(0, 0): 0, (0, 1): 1, (1, -1): 2} and li._engine is not eng and li._engine.L == 3
    names = [n for n, _ in rec.calls]
    r = names.index("lmi_regroup")
    assert "lmi_nav_set_tree" in names[r:] and "lmi_destroy" in names[r:]               # the old engine was closed
    ins = names.index("lmi_buckets_insert")
    assert ins > names.index("lmi_destroy")
    lab_ptr = rec.calls[ins][1][2]
    got = np.ctypeslib.as_array(ctypes.cast(lab_ptr, ctypes.POINTER(ctypes.c_int64)), shape=(3,))
    assert list(got) == [1, 1, 1]                                                      # the objects go to the new bucket's id
    assert li._engine_key[0] == "mutated" and (0, 1) in li.bucket_paths
    li._engine._h = None
    li._engine = None


# ---- the order rule in numpy ----
def test_order_rule_statement():
    rs = np.random.RandomState(0)
    N, L, L_new = 500, 6, 9
    old = rs.randint(0, L, N)
    old[old == 4] = 1                                             # an empty old bucket
    ids = (rs.permutation(10 * N)[:N] + 1).astype(np.uint32)
    pick = rs.rand(N) < 0.4
    pick[old == 3] = True                                         # bucket 3 is emptied by the list
    order = rs.permutation(int(pick.sum()))
    list_ids, list_lab = ids[pick][order], rs.randint(0, L_new, int(pick.sum()))
    bmap = np.asarray([8, 2, 2, -1, 5, 0])
    new, named = rr.new_labels(old, ids, list_ids, list_lab, bmap)
    assert named == pick.sum() and (new >= 0).all()
    assert np.array_equal(new[pick][order], list_lab) and np.array_equal(new[~pick], bmap[old[~pick]])
    absent = np.asarray([10 * N + 5, 10 * N + 6], dtype=np.uint32)                     # ids no object carries change nothing
    again, named2 = rr.new_labels(old, ids, np.concatenate([absent, list_ids]), np.concatenate([[0, 0], list_lab]), bmap)
    assert named2 == named and np.array_equal(again, new)
    X = rs.randn(N, 3).astype(np.float32)
    Xr, lr, ir = rr.regrouped(X, old, ids, new)
    want = rr.bucket_contents(old, ids, new, L_new)
    for b in range(L_new):                                        # a stable build of the list = the plain statement
        assert np.array_equal(ir[lr == b], want[b]), b
    row_of = {int(i): j for j, i in enumerate(ids)}
    assert np.array_equal(Xr, X[[row_of[int(i)] for i in ir]])   # the rows travel with their ids
    # the list's order does not matter, and an unnamed object on a -1 entry is visible as -1
    shuffled = rs.permutation(list_ids.size)
    assert np.array_equal(rr.new_labels(old, ids, list_ids[shuffled], list_lab[shuffled], bmap)[0], new)
    one = np.flatnonzero(np.isin(list_ids, ids[old == 3]))[0]    # a listed object of bucket 3, no longer listed
    left, _ = rr.new_labels(old, ids, np.delete(list_ids, one), np.delete(list_lab, one), bmap)
    assert (left < 0).sum() == 1 and old[left < 0][0] == 3
    # two objects that share an id both take its label
    ids2 = ids.copy()
    ids2[1] = ids2[0]
    both, n2 = rr.new_labels(old, ids2, [ids2[0]], [7], None)
    assert both[0] == both[1] == 7 and n2 == 2 and np.array_equal(both[2:], old[2:])
    # the identity is the resident order itself
    same, n0 = rr.new_labels(old, ids, [], [], None)
    assert n0 == 0 and np.array_equal(same, old)


def test_regroup_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "regroup_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "regroup_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "regroup plan selftest: clean" in r.stdout
