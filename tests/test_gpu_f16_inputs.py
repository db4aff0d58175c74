"""GPU (`-m gpu`): binary16 rows and queries as they are distributed -- the `*_f16` entry points of include/lmi_hip.h through
`_capi.Index`, `li` and `index_io`.  One contract: a call that takes halves returns bit for bit what the binary32 call returns for the
same values widened, so every comparison is `assert_array_equal` on bit patterns; there is no tolerance anywhere in this file.

Shapes: N = 3 000 rows, L = 4 buckets with bucket 2 empty, 64 queries; d = 45 (low-dimensional fragments, d % 8 != 0: 90-byte rows, the
element-by-element kernels), 136 (the other fragment shape, d % 8 == 0: the 16-byte kernels), 768 (the workload's).  Data: unit-length
rows rounded to binary16, as tests/test_gpu_f16_storage.py builds it."""
import json
import os

import numpy as np
import pytest

from test_f16_storage_host import CASES
from test_gpu_f16_storage import assert_same, q16, scan
from test_gpu_front import make

pytestmark = pytest.mark.gpu

N, L, NQ, EMPTY = 3000, 4, 64, 2
#: mode -> (storage, prefilter, metric)
MODES = {"f16": ("f16", True, "ip"), "f32": ("f32", True, "ip"), "f32-exact": ("f32", False, "ip"), "f32-l2": ("f32", True, "l2")}


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


_data = {}


def data(d):
    """(X f32 binary16-exact, X16 = the same values as float16, lab, Q, Q16, order [64, 3] with unvisited slots), read-only."""
    if d not in _data:
        X, lab, Q, order = make(300 + d, N, d, L, NQ, 3, empty=(EMPTY,))
        X16, Q16 = X.astype(np.float16), Q.astype(np.float16)
        X, Q = X16.astype(np.float32), Q16.astype(np.float32)
        order = np.ascontiguousarray(order)
        order[::5, 2] = -1
        assert (lab != EMPTY).all() and (order == EMPTY).any()
        for a in (X, X16, lab, Q, Q16, order):
            a.setflags(write=False)
        _data[d] = (X, X16, lab, Q, Q16, order)
    return _data[d]


def new_index(capi, mode):
    storage, prefilter, metric = MODES[mode]
    return capi.Index(0, chunk_rows=256, prefilter=prefilter, metric=metric, storage=storage)


def build(capi, mode, lab, d, pieces, **kw):
    """An index of `mode` filled by add_rows(block, r0) for (r0, block) in `pieces`."""
    idx = new_index(capi, mode)
    idx.buckets_begin(lab, d, L, **kw)
    for r0, block in pieces:
        idx.add_rows(block, r0)
    idx.buckets_end()
    return idx


def u(a):
    """Bit patterns of a float32 / float16 array."""
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def assert_same_buckets(a, b, dtype=np.float32):
    for bkt in range(a.L):
        ra, ia = a.read_bucket(bkt, dtype=dtype) if dtype != np.float32 else a.read_bucket(bkt)
        rb, ib = b.read_bucket(bkt, dtype=dtype) if dtype != np.float32 else b.read_bucket(bkt)
        np.testing.assert_array_equal(u(ra), u(rb))
        np.testing.assert_array_equal(ia, ib)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("d", [45, 136, 768])
def test_ingest_equality(capi, d, mode):
    """1. Pieces of 777 rows in reversed order, the second one float32 (mixed types), the others float16, against the same pieces all
    widened: scan results, statistics, every bucket's rows and ids, index_bytes; bytes_in counts each piece's own bytes."""
    X, X16, lab, Q, _, order = data(d)
    starts = list(range(0, N, 777))[::-1]
    halves = [(r0, X[r0:r0 + 777] if j == 1 else X16[r0:r0 + 777]) for j, r0 in enumerate(starts)]
    floats = [(r0, X[r0:r0 + 777]) for r0 in starts]
    assert [b.dtype for _, b in halves] == [np.float16, np.float32, np.float16, np.float16]
    a, b = build(capi, mode, lab, d, halves), build(capi, mode, lab, d, floats)
    assert a.bytes_in == sum(blk.shape[0] * d * (2 if blk.dtype == np.float16 else 4) for _, blk in halves)
    assert b.bytes_in == N * d * 4
    assert_same(scan(a, Q, order, 10), scan(b, Q, order, 10))
    assert (scan(a, Q, order, 10)[1] != 0).any()
    assert_same_buckets(a, b)
    for bkt in range(L):
        rows, _ = a.read_bucket(bkt)
        np.testing.assert_array_equal(u(rows), u(X[lab == bkt]))
    assert a.index_bytes() == b.index_bytes()
    a.close()
    b.close()


@pytest.mark.parametrize("mode", ["f16", "f32"])
@pytest.mark.parametrize("d", [45, 136])
def test_owned_ingest(capi, d, mode):
    """2. add_owned_rows with halves == with floats: half the buckets owned, two calls, both storages."""
    X, X16, lab, Q, _, order = data(d)
    owned = np.array([1, 1, 0, 0], dtype=np.uint8)
    rows = np.flatnonzero(owned[lab] == 1).astype(np.int64)
    half = rows.shape[0] // 2
    out = []
    for src in (X16, X):
        idx = new_index(capi, mode)
        idx.buckets_begin(lab, d, L, owned=owned)
        idx.add_owned_rows(src[rows[half:]], rows[half:])
        idx.add_owned_rows(src[rows[:half]], rows[:half])
        idx.buckets_end()
        out.append(idx)
    assert out[0].bytes_in * 2 == out[1].bytes_in == rows.shape[0] * d * 4
    assert_same(scan(out[0], Q, order, 10), scan(out[1], Q, order, 10))
    assert (scan(out[0], Q, order, 10)[1] != 0).any()
    assert_same_buckets(out[0], out[1])
    np.testing.assert_array_equal(out[0].bucket_sizes(), np.bincount(lab, minlength=L) * owned)
    for idx in out:
        idx.close()


@pytest.mark.parametrize("mode", ["f16", "f32"])
@pytest.mark.parametrize("d", [136, 45])
def test_device_pointers_and_alignment(capi, d, mode):
    """3. torch.float16 device tensors: one whose data pointer is 2 bytes past a 16-byte boundary (a flat buffer with one leading
    element, viewed as [n, d]) and one on the boundary; both give the host-fed index."""
    import torch

    X, X16, lab, Q, _, order = data(d)
    host = build(capi, mode, lab, d, [(0, X16)])
    want = scan(host, Q, order, 10)
    for lead in (1, 0):
        flat = torch.empty(N * d + 8, dtype=torch.float16, device="cuda:0")
        assert flat.data_ptr() % 16 == 0
        t = flat[lead:lead + N * d].view(N, d)
        t.copy_(torch.from_numpy(np.array(X16)))
        torch.cuda.synchronize()
        assert t.is_contiguous() and t.data_ptr() % 16 == 2 * lead
        dev = build(capi, mode, lab, d, [(1500, t[1500:]), (0, t[:1500])])
        assert dev.bytes_in == N * d * 2
        assert_same(want, scan(dev, Q, order, 10))
        assert_same_buckets(host, dev)
        dev.close()
        del t, flat
    host.close()


HALF_VERDICTS = {
    "inf": CASES["inf"][0][-1],
    "-inf": -CASES["inf"][0][-1],
    "nan": np.where(np.isinf(CASES["inf"][0][-1]), np.float32(np.nan), CASES["inf"][0][-1]).astype(np.float32),
    "2.0 and 2**-24": CASES["2.0 and 2**-24"][0][-1],
}


@pytest.mark.parametrize("name", list(HALF_VERDICTS))
def test_verdicts(capi, name):
    """4. The inadmissible cases of test_f16_storage_host.CASES that halves can express, each as one row of a half-fed F16 build:
    buckets_end fails with the float-fed build's message class; the handle then takes a fresh build and searches correctly."""
    row = HALF_VERDICTS[name]
    assert not capi.f16_admissible(row)[0] and (np.isnan(row).any() or np.array_equal(q16(row), row, equal_nan=True))
    X, lab, Q, order = make(5, N, row.shape[0], L, NQ, 2)
    good, Q = q16(X), q16(Q)
    bad = good.copy()
    bad[1234] = row
    msgs = []
    idx = capi.Index(0, storage="f16")
    for src in (bad.astype(np.float16), bad):
        with pytest.raises(capi.LmiError) as e:
            idx.set_buckets(src, lab, L)
        msgs.append(str(e.value))
        with pytest.raises(capi.LmiError):
            idx.scan_topk(Q, order, 10)          # no index was built
    for word in ("LMI_STORAGE_F16", "finite", "scale"):
        assert (word in msgs[0]) == (word in msgs[1]), msgs
    assert "LMI_STORAGE_F16" in msgs[0] and (("finite" in msgs[0]) != ("scale" in msgs[0])), msgs[0]
    idx.set_buckets(good.astype(np.float16), lab, L)    # the same handle, a fresh half-fed build
    ref = capi.Index(0, storage="f32")
    ref.set_buckets(good, lab, L)
    assert_same(scan(ref, Q, order, 10), scan(idx, Q, order, 10))
    ref.close()
    idx.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("d", [45, 768])
def test_read_back_halves(capi, d, mode):
    """5a. read_bucket(dtype=float16) returns the input halves bit for bit: from the stored halves of an F16 index, narrowed on the
    device from both F32 layouts (and without the L2 norm column)."""
    _, X16, lab, _, _, _ = data(d)
    ids = (np.arange(N, dtype=np.uint32) * 7 + 3).astype(np.uint32)
    idx = build(capi, mode, lab, d, [(0, X16)], ids=ids)
    for bkt in range(L):
        rows, bid = idx.read_bucket(bkt, dtype=np.float16)
        assert rows.dtype == np.float16 and rows.shape == (int((lab == bkt).sum()), d)
        np.testing.assert_array_equal(u(rows), u(X16[lab == bkt]))
        np.testing.assert_array_equal(bid, ids[lab == bkt])
    idx.close()


@pytest.mark.parametrize("d", [40, 200])
def test_read_back_scale_below_one(capi, d):
    """5b. An F16 index with scale 1/8 (built as test_gpu_f16_storage.py::test_scale_below_one builds it), fed and read as halves."""
    rs = np.random.RandomState(d)
    X16 = (rs.randint(-256, 257, size=(N, d)) / 64.0).astype(np.float16)
    X16[17, 3] = 4.0
    lab = rs.randint(0, 6, N).astype(np.int64)
    assert capi.f16_admissible(X16.astype(np.float32))[0] and np.abs(X16).max() == 4.0
    idx = capi.Index(0, chunk_rows=256, storage="f16")
    idx.set_buckets(X16, lab, 6)
    for bkt in range(6):
        rows, _ = idx.read_bucket(bkt, dtype=np.float16)
        np.testing.assert_array_equal(u(rows), u(X16[lab == bkt]))
        rows32, _ = idx.read_bucket(bkt)
        np.testing.assert_array_equal(u(rows32), u(X16[lab == bkt].astype(np.float32)))
    idx.close()


@pytest.mark.parametrize("mode", ["f32", "f32-exact"])
def test_read_back_refuses_inexact(capi, mode):
    """5c. An F32 index with one row that binary16 cannot hold: reading its bucket as halves raises and names binary16, the other
    buckets read fine, and a search afterwards equals the search before."""
    X, _, lab, Q, _, order = data(45)
    X = X.copy()
    X[100, 5] = np.float32(0.1)
    assert np.float32(np.float16(X[100, 5])) != X[100, 5]
    idx = build(capi, mode, lab, 45, [(0, X)])
    before = scan(idx, Q, order, 10)
    with pytest.raises(capi.LmiError, match="binary16"):
        idx.read_bucket(int(lab[100]), dtype=np.float16)
    assert_same(before, scan(idx, Q, order, 10))
    for bkt in range(L):
        if bkt != lab[100]:
            rows, _ = idx.read_bucket(bkt, dtype=np.float16)
            np.testing.assert_array_equal(u(rows), u(X[lab == bkt].astype(np.float16)))
    rows, _ = idx.read_bucket(int(lab[100]))
    np.testing.assert_array_equal(u(rows), u(X[lab == lab[100]]))
    idx.close()


@pytest.mark.parametrize("mode", ["f32", "f32-exact"])
@pytest.mark.parametrize("d", [45, 136])
def test_insert(capi, d, mode):
    """6. insert of 500 half rows into an F32-storage index (both layouts) == insert of the widened rows: search results, every
    bucket, the layout tables."""
    X, X16, lab, Q, _, order = data(d)
    ids = np.arange(50_000, 50_500, dtype=np.uint32)
    out = []
    for src in (X16, X):
        idx = build(capi, mode, lab[:2500], d, [(0, X[:2500])])
        assert idx.insert(src[2500:], lab[2500:], ids) == 500
        out.append(idx)
    assert_same(scan(out[0], Q, order, 10), scan(out[1], Q, order, 10))
    assert (scan(out[0], Q, order, 10)[1] >= 50_000).any(), "no inserted object among the results"
    assert_same_buckets(out[0], out[1])
    la, lb = out[0].debug_layout(), out[1].debug_layout()
    assert sorted(la) == sorted(lb)
    for key in la:
        np.testing.assert_array_equal(la[key], lb[key])
    for idx in out:
        idx.close()


def test_insert_refused_on_f16_storage(capi):
    X, X16, lab, Q, _, order = data(45)
    idx = build(capi, "f16", lab, 45, [(0, X16)])
    before = scan(idx, Q, order, 10)
    with pytest.raises(capi.LmiError, match="LMI_STORAGE_F16"):
        idx.insert(X16[:3], lab[:3], np.array([90001, 90002, 90003], dtype=np.uint32))
    assert_same(before, scan(idx, Q, order, 10))
    idx.close()


@pytest.mark.parametrize("d", [45, 768])
def test_queries_one_level(capi, d):
    """7a. scan_topk and search (stop mass off and 0.9; one array passed twice and two arrays) with float16 queries == the calls with
    the widened arrays."""
    X, X16, lab, Q, Q16, order = data(d)
    rs = np.random.RandomState(d)
    layers = [((rs.randn(32, d) * 0.5).astype(np.float32), (rs.randn(32) * 0.1).astype(np.float32)),
              ((rs.randn(L, 32) * 2.0).astype(np.float32), (rs.randn(L) * 0.1).astype(np.float32))]   # (sharp: 0.9 is reached early)
    P16 = (Q[::-1] * 0.5).astype(np.float16)    # a second query set for the two-array form
    P = P16.astype(np.float32)
    idx = build(capi, "f32", lab, d, [(0, X16)])
    idx.set_mlp(layers)
    assert_same(scan(idx, Q16, order, 10), scan(idx, Q, order, 10))
    for mass in (0.0, 0.9):
        idx.set_stop_mass(mass)
        for h_args, f_args in (((Q16, Q16), (Q, Q)), ((Q16, P16), (Q, P))):
            dh, ih, boh, kh = idx.search(*h_args, 3, 10, want_keys=True)
            df, i_f, bof, kf = idx.search(*f_args, 3, 10, want_keys=True)
            np.testing.assert_array_equal(u(dh), u(df))
            np.testing.assert_array_equal(ih, i_f)
            np.testing.assert_array_equal(boh, bof)
            np.testing.assert_array_equal(kh, kf)
            assert (ih != 0).any()
        if mass:
            assert (boh < 0).any(), "the stop mass cut no query short"
    idx.close()


@pytest.mark.parametrize("same", [False, True], ids=["two arrays", "one array"])
def test_queries_search_tree(capi, same):
    """7b. search_tree on the [4, 3] synthetic tree, path mass off and 0.9, float16 queries == the widened ones; `one array`: the
    navigation vectors are the scan vectors too (queries_search is queries_nav)."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from path_mass_ref import synthetic_tree
    from test_gpu_path_mass import frame, net_from

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree([4, 3], nq=NQ)
    Xs = Xn if same else Xs
    Xs = q16(Xs / np.linalg.norm(Xs, axis=1, keepdims=True))
    Qn16, Qs16 = Qn.astype(np.float16), Qs.astype(np.float16)
    li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    eng = li.prepare(frame(Xn), frame(Xs), dp, [4, 3])
    for mass in (0.0, 0.9):
        eng.set_path_mass(mass)
        if same:
            h = eng.search_tree(Qn16, Qn16, 5, 10, want_keys=True, want_order=True)
            qf = Qn16.astype(np.float32)
            f = eng.search_tree(qf, qf, 5, 10, want_keys=True, want_order=True)
        else:
            h = eng.search_tree(Qn16, Qs16, 5, 10, want_keys=True, want_order=True)
            f = eng.search_tree(Qn16.astype(np.float32), Qs16.astype(np.float32), 5, 10, want_keys=True, want_order=True)
        np.testing.assert_array_equal(u(h[0]), u(f[0]))
        for a, b in zip(h[1:], f[1:]):
            np.testing.assert_array_equal(a, b)
        assert (h[1] != 0).any()
        if mass:
            assert (h[4] < 0).any(), "the path mass cut no walk short"
    li.close()


def dev16(a16, lead):
    """`a16` (float16 [n, d]) as a device tensor whose data pointer is 2 * lead bytes past a 16-byte boundary; (tensor, its buffer)."""
    import torch

    n, d = a16.shape
    flat = torch.empty(n * d + 8, dtype=torch.float16, device="cuda:0")
    t = flat[lead:lead + n * d].view(n, d)
    t.copy_(torch.from_numpy(np.array(a16)))
    assert t.is_contiguous() and t.data_ptr() % 16 == 2 * lead
    return t, flat


def dev_out(nq, kout, nb):
    import torch

    return [torch.zeros((nq, w), dtype=torch.int32 if j else torch.float32, device="cuda:0") for j, w in enumerate((kout, kout, kout, nb))]


def host_bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("lead", [1, 0], ids=["2 bytes past a 16-byte boundary", "16-byte aligned"])
@pytest.mark.parametrize("d", [45, 136])
def test_queries_device_tensors(capi, d, lead):
    """7c. scan_topk_device / search_device with torch.float16 query tensors (on_device: widened into the handle's buffers from the
    caller's memory, which is left as it was) == the host calls with the widened arrays; one tensor passed twice and two tensors."""
    import torch

    X, X16, lab, Q, Q16, order = data(d)
    rs = np.random.RandomState(d)
    layers = [((rs.randn(32, d) * 0.5).astype(np.float32), (rs.randn(32) * 0.1).astype(np.float32)),
              ((rs.randn(L, 32) * 2.0).astype(np.float32), (rs.randn(L) * 0.1).astype(np.float32))]
    P16 = (Q[::-1] * 0.5).astype(np.float16)
    P = P16.astype(np.float32)
    idx = build(capi, "f32", lab, d, [(0, X16)])
    idx.set_mlp(layers)
    q_t, q_buf = dev16(Q16, lead)
    p_t, p_buf = dev16(P16, lead)
    order_t = torch.from_numpy(np.array(order)).to("cuda:0")
    torch.cuda.synchronize()
    dw, iw, kw = idx.scan_topk(Q, order, 10, want_keys=True)
    d_t, i_t, k_t, _ = dev_out(NQ, 10, 3)
    idx.scan_topk_device(q_t, order_t, 3, 10, d_t, i_t, k_t)
    torch.cuda.synchronize()
    for got, want in ((d_t, dw), (i_t, iw), (k_t, kw)):
        np.testing.assert_array_equal(host_bits(got), want.view(np.uint32))
    for (a_t, b_t), (a, b) in (((q_t, q_t), (Q, Q)), ((q_t, p_t), (Q, P))):
        dw, iw, bw, kw = idx.search(a, b, 3, 10, want_keys=True)
        d_t, i_t, k_t, b_o = dev_out(NQ, 10, 3)
        idx.search_device(a_t, b_t, 3, 10, d_t, i_t, k_t, b_o)
        torch.cuda.synchronize()
        for got, want in ((d_t, dw), (i_t, iw), (k_t, kw), (b_o, bw)):
            np.testing.assert_array_equal(host_bits(got), want.view(np.uint32))
        assert (iw != 0).any()
    np.testing.assert_array_equal(q_t.cpu().numpy().view(np.uint16), u(Q16))   # the caller's halves were only read
    with pytest.raises(AssertionError):
        idx.search_device(q_t, p_t.float(), 3, 10, d_t, i_t, k_t, b_o)        # mixed device types are refused, not converted
    idx.close()
    del q_t, p_t, q_buf, p_buf


@pytest.mark.parametrize("lead", [1, 0], ids=["2 bytes past a 16-byte boundary", "16-byte aligned"])
def test_device_tree_queries_then_host_call(capi, lead):
    """7d. search_tree_device with torch.float16 tensors == the host call; and a host-pointer float32 search_tree with OTHER queries
    issued right behind it, without a synchronisation in between -- its scan vectors are uploaded on the library's side stream into
    the buffer the device call's scan reads -- leaves the device call's results what they are and returns its own."""
    import torch

    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from path_mass_ref import synthetic_tree
    from test_gpu_path_mass import frame, net_from

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree([4, 3], nq=256)
    Xs = q16(Xs / np.linalg.norm(Xs, axis=1, keepdims=True))
    Qn16, Qs16 = Qn.astype(np.float16), Qs.astype(np.float16)
    On, Os = np.ascontiguousarray(Qn[::-1] * 0.5), np.ascontiguousarray(Qs[::-1] * 0.25)   # the host call's queries
    li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    eng = li.prepare(frame(Xn), frame(Xs), dp, [4, 3])
    want_dev = eng.search_tree(Qn16.astype(np.float32), Qs16.astype(np.float32), 5, 10, want_keys=True, want_order=True)
    want_host = eng.search_tree(On, Os, 5, 10, want_keys=True, want_order=True)
    assert not np.array_equal(want_dev[1], want_host[1])
    qn_t, b0 = dev16(Qn16, lead)
    qs_t, b1 = dev16(Qs16, lead)
    outs = dev_out(256, 10, 5) + dev_out(256, 10, 5)[3:]
    torch.cuda.synchronize()
    eng.search_tree_device(qn_t, qs_t, 5, 10, *outs)
    got_host = eng.search_tree(On, Os, 5, 10, want_keys=True, want_order=True)   # no synchronisation in between
    torch.cuda.synchronize()
    for got, want in zip(outs, want_dev):
        np.testing.assert_array_equal(host_bits(got), want.view(np.uint32))
    for got, want in zip(got_host, want_host):
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    li.close()
    del qn_t, qs_t, b0, b1


def test_li_and_disk(capi, tmp_path):
    """8. A 5 000 x 64 float16 frame and float16 queries through li.search(storage="f16") == the float32 frame and queries; the
    frame went in as halves; save_index writes vectors.f16.npy only; load_index answers identically in either storage; a directory
    saved from an f32-resident engine is in the layout it always had."""
    from learnedmetricindex_amd import index_io
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import frame, net_from

    rs = np.random.RandomState(11)
    X16 = rs.randn(5000, 64).astype(np.float32)
    X16 = (X16 / np.linalg.norm(X16, axis=1, keepdims=True)).astype(np.float16)   # the data as it is distributed
    X = X16.astype(np.float32)
    Q16 = (X[rs.randint(0, 5000, 200)] + 0.05 * rs.randn(200, 64).astype(np.float32)).astype(np.float16)
    Q = Q16.astype(np.float32)
    layers = [((rs.randn(128, 64) * 0.3).astype(np.float32), (rs.randn(128) * 0.1).astype(np.float32)),
              ((rs.randn(12, 128) * 0.3).astype(np.float32), (rs.randn(12) * 0.1).astype(np.float32))]
    dp = rs.randint(0, 12, 5000).astype(np.int64)
    df, df16 = frame(X), frame(X16)
    assert (df16.dtypes == np.float16).all()
    li = LearnedIndex(net_from(layers), {}, [(i,) for i in range(12)])
    d32, n32, _ = li.search(df, Q, df, Q, dp, [12], n_buckets=3, k=10)
    assert li._engine.storage == "f32" and li._engine.bytes_in == 5000 * 64 * 4
    path32 = str(tmp_path / "idx32")
    index_io.save_index(path32, li, [12])
    assert sorted(os.listdir(path32)) == ["ids.npy", "meta.json", "sizes.npy", "vectors.f32.npy", "weights.npz"]
    meta32 = json.load(open(os.path.join(path32, "meta.json")))
    assert sorted(meta32) == sorted(["format", "version", "N", "d", "metric", "n_categories", "bucket_paths", "root_layers", "internal"])
    assert meta32["version"] == 2
    order = np.argsort(dp, kind="stable")
    v32 = np.load(os.path.join(path32, "vectors.f32.npy"))
    assert v32.dtype == np.float32
    np.testing.assert_array_equal(u(v32), u(X[order]))

    d16, n16, _ = li.search(df16, Q16, df16, Q16, dp, [12], n_buckets=3, k=10, storage="f16")
    assert li._engine.storage == "f16"
    assert li._engine.bytes_in == 5000 * 64 * 2, "the float16 frame was widened on the host"
    np.testing.assert_array_equal(n16, n32)
    np.testing.assert_array_equal(d16, d32)
    path = str(tmp_path / "idx16")
    index_io.save_index(path, li, [12])
    assert sorted(os.listdir(path)) == ["ids.npy", "meta.json", "sizes.npy", "vectors.f16.npy", "weights.npz"]
    v16 = np.load(os.path.join(path, "vectors.f16.npy"), mmap_mode="r")
    assert v16.dtype == np.float16 and v16.shape == (5000, 64) and v16.nbytes == 5000 * 64 * 2
    np.testing.assert_array_equal(u(np.asarray(v16)), u(X16[order]))
    meta = json.load(open(os.path.join(path, "meta.json")))
    assert meta["vectors"] == "f16" and meta["storage"] == "f16" and meta["version"] == 2
    li.close()
    for storage in (None, "f32"):
        li2, ncat = index_io.load_index(path, storage=storage)
        assert li2._engine.storage == (storage or "f16")
        assert li2._engine.bytes_in == 5000 * 64 * 2          # streamed in as halves, into either storage
        for qa in (Q16, Q):
            d2, n2, _ = li2.search_resident(qa, qa, ncat, n_buckets=3, k=10)
            np.testing.assert_array_equal(n2, n32)
            np.testing.assert_array_equal(d2, d32)
        li2.close()
