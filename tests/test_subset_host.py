"""CPU (`-m "not gpu"`): `Index.subset` / `LearnedIndex.subset` marshal `lmi_subset` (include/lmi_hip.h) as the header declares it.
No GPU call is made: the dispatch runs against the recording stand-in for the library that test_f16_inputs_host.py uses."""
import ctypes
import gc

import numpy as np
import pytest

from learnedmetricindex_amd import _capi
from test_f16_inputs_host import Recorder


class Subsetter(Recorder):
    """The stand-in with an `lmi_subset` that behaves: it reads the id array it is handed, writes a handle and a kept count (or
    fails with a message, `fail` set)."""

    def __init__(self, fail=None):
        super().__init__()
        self.fail = fail
        self.seen_ids = None

    def lmi_subset(self, h, ids, n, mode, out, n_kept):
        self.calls.append(("lmi_subset", (h, ids, n, mode, out, n_kept)))
        self.seen_ids = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).copy() if n else np.empty(0, np.uint32)
        if self.fail:
            return -1
        out._obj.value = 0xBEEF0
        n_kept._obj.value = 7
        return 0

    def lmi_last_error(self):
        return (self.fail or "").encode()


@pytest.fixture
def parent_index(monkeypatch):
    """parent_index(stand-in) -> a built-looking Index over it.  Every handle made during the test is dropped while the stand-in is
    still in place: none of them may reach the real library's lmi_destroy."""
    made = []

    def make(rec):
        monkeypatch.setattr(_capi, "_lib", rec)
        idx = _capi.Index.__new__(_capi.Index)
        idx._h, idx._views = ctypes.c_void_p(1), []
        idx.device, idx.n_classes, idx.d_nav, idx.d, idx.L, idx.N, idx.bytes_in = 0, 3, 16, 8, 3, 20, 0
        idx.metric, idx.storage, idx.stop_mass, idx.path_mass = "l2", "f32", 0.5, 0.25
        made.append(idx)
        return idx

    yield make
    for idx in made:
        idx._h = None
    gc.collect()


@pytest.mark.parametrize("drop", [False, True])
def test_subset_marshals_ids_and_mode(parent_index, drop):
    rec = Subsetter()
    idx = parent_index(rec)
    ids = np.asarray([[9, 4], [4, 2 ** 32 - 1]], dtype=np.int64)[:, ::-1]   # neither uint32 nor contiguous
    sub = idx.subset(ids, drop=drop)
    name, (h, ptr, n, mode, _, _) = rec.calls[-1]
    assert name == "lmi_subset" and h is idx._h and n == 4 and mode == (1 if drop else 0)
    np.testing.assert_array_equal(rec.seen_ids, np.asarray([4, 9, 2 ** 32 - 1, 4], dtype=np.uint32))   # a contiguous uint32 array
    assert isinstance(sub, _capi.Index) and sub is not idx and sub._h.value == 0xBEEF0
    assert sub not in idx._views and sub._views == [] and not hasattr(sub, "_parent")   # an owning Index, not a view
    for a in ("device", "n_classes", "d_nav", "d", "L", "metric", "storage", "stop_mass", "path_mass"):
        assert getattr(sub, a) == getattr(idx, a), a
    assert sub.N == 7 and idx.N == 20
    empty = idx.subset([], drop=drop)                                        # no ids: n == 0 goes through
    assert rec.calls[-1][0] == "lmi_subset" and rec.calls[-1][1][2] == 0 and rec.calls[-1][1][3] == (1 if drop else 0)
    empty.close()
    sub.close()
    assert rec.calls[-1][0] == "lmi_destroy" and rec.calls[-1][1][0].value == 0xBEEF0    # closing it destroys ITS handle only


@pytest.mark.parametrize("bad", [[1, 2 ** 32], [-1, 5], np.asarray([3, 2 ** 40], dtype=np.int64)])
def test_ids_outside_uint32_raise_before_the_call(parent_index, bad):
    rec = Subsetter()
    idx = parent_index(rec)
    with pytest.raises(ValueError, match="uint32"):
        idx.subset(bad)
    assert rec.calls == []


@pytest.mark.parametrize("bad", [[1.5], np.asarray([1.0, 2.0]), ["7"], [True, False]])
def test_ids_that_are_not_integers_raise_before_the_call(parent_index, bad):
    rec = Subsetter()
    idx = parent_index(rec)
    with pytest.raises(ValueError, match="integers"):
        idx.subset(bad)
    assert rec.calls == []


def test_library_failure_raises_and_leaves_no_handle(parent_index):
    rec = Subsetter(fail="lmi_subset: unknown mode 7")
    idx = parent_index(rec)
    with pytest.raises(_capi.LmiError, match="lmi_subset: unknown mode"):
        idx.subset([1, 2, 3])
    assert [n for n, _ in rec.calls] == ["lmi_subset"]            # nothing to destroy: *out stayed NULL
    assert not rec.calls[0][1][4]._obj.value
    assert idx._views == [] and idx.N == 20


def test_li_subset_needs_a_resident_index():
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    li = LearnedIndex(object(), {}, [(0,), (1,)])
    with pytest.raises(AssertionError, match="no resident index"):
        li.subset([1, 2])


def test_li_subset_wraps_the_derived_engine(parent_index):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    rec = Subsetter()
    eng = parent_index(rec)
    root, internal, paths = object(), {(0, -1): object()}, [(0, 1), (1, 0)]
    li = LearnedIndex(root, internal, paths)
    li._engine, li._engine_key = eng, ("some", "key")
    li._path_ids, li._entry_paths, li._nav_cap = {(0, 1): 0}, np.zeros((2, 2), np.int32), 5
    sub = li.subset(np.asarray([5, 6], dtype=np.int64), drop=True)
    assert rec.calls[-1][0] == "lmi_subset" and rec.calls[-1][1][2:4] == (2, 1)
    assert isinstance(sub, LearnedIndex) and sub is not li
    assert sub.root_model is root and sub.internal_models is internal and sub.bucket_paths is paths
    assert sub._engine is not eng and sub._engine._h.value == 0xBEEF0
    assert sub._engine_key[0] == "mutated" and sub._engine_key != li._engine_key and li._engine_key == ("some", "key")
    assert sub._path_ids is li._path_ids and sub._nav_cap == 5
    sub.close()
    li._engine = None
