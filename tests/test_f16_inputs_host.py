"""CPU (`-m "not gpu"`): the binary16 entry points (`*_f16`, include/lmi_hip.h) are exported and bound, `_capi.Index` sends float16
arrays to them without copying or widening them on the host, and `index_io` picks the vectors file a meta.json names.  No GPU call is
made: the dispatch runs against a recording stand-in for the library."""
import ctypes

import numpy as np
import pytest

from learnedmetricindex_amd import _capi, index_io

#: name -> (namesake, positions of the half pointers among the arguments)
F16_CALLS = {
    "lmi_buckets_add_rows_f16": ("lmi_buckets_add_rows", (1,)),
    "lmi_buckets_add_owned_rows_f16": ("lmi_buckets_add_owned_rows", (1,)),
    "lmi_buckets_insert_f16": ("lmi_buckets_insert", (1,)),
    "lmi_bucket_read_f16": ("lmi_bucket_read", (2,)),
    "lmi_scan_topk_f16": ("lmi_scan_topk", (1,)),
    "lmi_search_f16": ("lmi_search", (1, 2)),
    "lmi_search_tree_f16": ("lmi_search_tree", (1, 2)),
}


def test_f16_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, (namesake, half_args) in F16_CALLS.items():
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        res0, args0 = _capi.SIGNATURES[namesake]
        assert res is ctypes.c_int and res0 is ctypes.c_int
        assert len(args) == len(args0), name                      # the namesake's argument list ...
        for pos, (a, a0) in enumerate(zip(args, args0)):
            if pos in half_args:                                  # ... with the half pointers as untyped or uint16 pointers
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint16)), (name, pos, a)
            else:
                assert a is a0, (name, pos, a, a0)
    assert L.lmi_abi_version() == 1


class Recorder:
    """Stands in for the loaded library: every entry point returns 0 and is recorded as (name, arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call

    def names(self):
        return [n for n, _ in self.calls if n != "lmi_bucket_sizes"]


@pytest.fixture
def fake(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    idx = _capi.Index.__new__(_capi.Index)
    idx._h, idx._views = ctypes.c_void_p(1), []
    idx.d, idx.L, idx.N, idx.n_classes, idx.bytes_in = 8, 3, 0, 3, 0
    yield rec, idx
    idx._h = None


def test_ingest_dispatch_by_dtype(fake):
    rec, idx = fake
    a16 = np.arange(40, dtype=np.float16).reshape(5, 8)
    a32 = a16.astype(np.float32)
    idx.add_rows(a16, 10)
    name, args = rec.calls[-1]
    assert name == "lmi_buckets_add_rows_f16"
    assert args[1] == a16.ctypes.data, "the halves were copied on the way in"     # its own buffer: no copy, no widening
    assert args[2:] == (10, 5, 0)
    idx.add_rows(a32, 0)
    assert rec.calls[-1][0] == "lmi_buckets_add_rows" and rec.calls[-1][1][1] == a32.ctypes.data
    idx.add_rows(a16.astype(np.float64), 0)                                     # anything else goes where it went: float32
    assert rec.calls[-1][0] == "lmi_buckets_add_rows"
    assert idx.bytes_in == a16.nbytes + 2 * a32.nbytes
    index = np.arange(5, dtype=np.int64)
    idx.add_owned_rows(a16, index)
    assert rec.calls[-1][0] == "lmi_buckets_add_owned_rows_f16" and rec.calls[-1][1][1] == a16.ctypes.data
    idx.add_owned_rows(a32, index)
    assert rec.calls[-1][0] == "lmi_buckets_add_owned_rows"
    ids = np.arange(5, dtype=np.uint32)
    idx.insert(a16, np.zeros(5, dtype=np.int64), ids)
    assert rec.calls[-1][0] == "lmi_buckets_insert_f16" and rec.calls[-1][1][1] == a16.ctypes.data
    idx.insert(a32, np.zeros(5, dtype=np.int64), ids)
    assert rec.calls[-1][0] == "lmi_buckets_insert"


def test_set_buckets_keeps_halves_and_counts_bytes(fake):
    rec, idx = fake
    data = np.arange(80, dtype=np.float16).reshape(10, 8)
    idx.bytes_in = 123
    idx.set_buckets(data, np.zeros(10, dtype=np.int64), 3, piece=4)
    assert rec.names() == ["lmi_buckets_begin"] + ["lmi_buckets_add_rows_f16"] * 3 + ["lmi_buckets_end"]
    adds = [a for n, a in rec.calls if n == "lmi_buckets_add_rows_f16"]
    assert [a[1] for a in adds] == [data.ctypes.data + r0 * 16 for r0 in (0, 4, 8)]   # slices of the caller's array
    assert idx.bytes_in == data.nbytes                                              # counted since buckets_begin
    rec.calls.clear()
    idx.set_buckets(data.astype(np.float32), np.zeros(10, dtype=np.int64), 3, piece=4)
    assert rec.names() == ["lmi_buckets_begin"] + ["lmi_buckets_add_rows"] * 3 + ["lmi_buckets_end"]
    assert idx.bytes_in == data.nbytes * 2


def test_sharded_owned_ingest_passes_halves_through(fake):
    from learnedmetricindex_amd import sharded

    rec, idx = fake
    data = np.arange(96, dtype=np.float16).reshape(12, 8)
    labels = np.arange(12) % 3
    n = sharded.ingest_owned(idx, data, labels, 3, owner=[0, 1, 0], rank=0, piece=5)
    assert n == 8
    assert rec.names() == ["lmi_buckets_begin"] + ["lmi_buckets_add_owned_rows_f16"] * 2 + ["lmi_buckets_end"]
    assert idx.bytes_in == 8 * 8 * 2
    rec.calls.clear()
    sharded.ingest_owned(idx, data.astype(np.float32), labels, 3, owner=[0, 1, 0], rank=1, piece=5)
    assert rec.names() == ["lmi_buckets_begin", "lmi_buckets_add_owned_rows", "lmi_buckets_end"]
    assert idx.bytes_in == 4 * 8 * 4


def test_query_and_read_dispatch_by_dtype(fake):
    rec, idx = fake
    q16 = np.ones((4, 8), dtype=np.float16)
    p16 = np.ones((4, 8), dtype=np.float16)
    q32 = q16.astype(np.float32)
    order = np.zeros((4, 2), dtype=np.int32)
    idx.scan_topk(q16, order)
    assert rec.calls[-1][0] == "lmi_scan_topk_f16" and rec.calls[-1][1][1] == q16.ctypes.data
    idx.scan_topk(q32, order)
    assert rec.calls[-1][0] == "lmi_scan_topk"
    for method, stem in ((idx.search, "lmi_search"), (idx.search_tree, "lmi_search_tree")):
        method(q16, q16, 2)
        name, args = rec.calls[-1]
        assert name == stem + "_f16" and args[1] == args[2] == q16.ctypes.data       # one array stays one array
        method(q16, p16, 2)
        name, args = rec.calls[-1]
        assert name == stem + "_f16" and (args[1], args[2]) == (q16.ctypes.data, p16.ctypes.data)
        method(q32, q32, 2)
        assert rec.calls[-1][0] == stem
        method(q16, q32, 2)                                                         # mixed: the half one is widened on the host
        name, args = rec.calls[-1]
        assert name == stem and args[1] != q16.ctypes.data and args[2] == q32.ctypes.data
        method(q32, q16, 2)
        name, args = rec.calls[-1]
        assert name == stem and args[1] == q32.ctypes.data and args[2] != q16.ctypes.data
    rows, _ = idx.read_bucket(1, dtype=np.float16)
    assert rec.calls[-1][0] == "lmi_bucket_read_f16" and rows.dtype == np.float16 and rows.shape == (0, 8)
    rows, _ = idx.read_bucket(1)
    assert rec.calls[-1][0] == "lmi_bucket_read" and rows.dtype == np.float32
    with pytest.raises(AssertionError):
        idx.read_bucket(1, dtype=np.float64)


def test_index_io_vectors_file_from_meta():
    assert index_io.vectors_file({}) == ("vectors.f32.npy", np.dtype(np.float32))               # a directory without the key
    assert index_io.vectors_file({"storage": "f16"}) == ("vectors.f32.npy", np.dtype(np.float32))   # written before the key existed
    assert index_io.vectors_file({"vectors": "f32"}) == ("vectors.f32.npy", np.dtype(np.float32))
    assert index_io.vectors_file({"vectors": "f16", "storage": "f16"}) == ("vectors.f16.npy", np.dtype(np.float16))
    with pytest.raises(AssertionError):
        index_io.vectors_file({"vectors": "bf16"})
    assert index_io.VERSION == 2
