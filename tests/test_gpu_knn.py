"""GPU (`-m gpu`): lmi_knn, the exact brute-force k-NN for k up to 1024 (include/lmi_hip.h), against the unchanged CPU oracle.

Every comparison is exact: D as uint32 bit patterns, I with array_equal, against oracle.knn_ip / oracle.knn_l2 at the same k.  The
inputs come from tests/knn_cases.py; tests/test_knn_host.py checks on the oracle alone that they have the properties relied on here."""
import numpy as np
import pytest
import torch

import knn_cases as kc
from learnedmetricindex_amd import _capi

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(np.finfo(np.float32).max)


def same(got, want, what=""):
    D, I = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == want[0].shape and I.shape == want[1].shape, what
    np.testing.assert_array_equal(I, want[1], err_msg=f"I {what}")
    np.testing.assert_array_equal(D.view(np.uint32), want[0].view(np.uint32), err_msg=f"D bits {what}")


def on_device(*arrays):
    return tuple(torch.from_numpy(np.array(a, order="C")).cuda() for a in arrays)


@pytest.mark.parametrize("k", kc.KS)
@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("shape", kc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_oracle(oracle, shape, metric, k):
    xq, xb = kc.case(*shape)
    same(_capi.knn(xq, xb, k, metric), kc.truth(oracle, shape, xq, xb, k, metric), f"{shape} {metric} k={k}")


@pytest.mark.parametrize("shape", kc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_agrees_with_lmi_knn_ip_at_k_10(shape):
    xq, xb = kc.case(*shape)
    same(_capi.knn(xq, xb, 10, "ip"), _capi.knn_ip(xq, xb, 10), f"{shape}")


@pytest.mark.parametrize("k", [10, 11, 64])
@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("shape", kc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ties_at_the_boundary_go_to_the_lower_row(oracle, shape, metric, k):
    """k = 10 and 11 cut the 52-row tie group, k = 64 contains it: either way its rows come first, ascending."""
    xq, xb = kc.case(*shape)
    g = kc.tie_group(shape[1])
    m = min(k, g.size)
    want = np.broadcast_to(g[:m], (kc.TIE_QUERIES, m))
    np.testing.assert_array_equal(kc.truth(oracle, shape, xq, xb, k, metric)[1][:kc.TIE_QUERIES, :m], want)   # the case still has its ties
    D, I = _capi.knn(xq, xb, k, metric)
    np.testing.assert_array_equal(I[:kc.TIE_QUERIES, :m], want)
    assert np.all(D[:kc.TIE_QUERIES, :m].view(np.uint32) == D[0, 0].view(np.uint32))   # one score, bit for bit


@pytest.mark.parametrize("geometry", kc.GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
@pytest.mark.parametrize("shape", [kc.SHAPES[0], kc.SHAPES[1]], ids=lambda s: "x".join(map(str, s)))
def test_forced_geometry_changes_nothing(oracle, shape, geometry):
    """Pieces, splits and query groups with ragged ends, from host arrays and from device tensors: the automatic result, the forced
    result and the oracle are one."""
    xq, xb = kc.case(*shape)
    nq, nb, d = shape
    piece, splits, qrows = geometry
    dq, db = on_device(xq, xb)
    try:
        for metric in kc.METRICS:
            for k in (65, 1024):
                want = kc.truth(oracle, shape, xq, xb, k, metric)
                _capi.knn_set_geometry(0, 0, 0)
                auto_host = _capi.knn(xq, xb, k, metric)
                auto_dev = _capi.knn(dq, db, k, metric)
                _capi.knn_set_geometry(*geometry)
                for kind, q, x, auto in (("host", xq, xb, auto_host), ("device", dq, db, auto_dev)):
                    got = _capi.knn(q, x, k, metric)
                    plan = _capi.knn_last_plan()
                    what = f"{shape} {metric} k={k} {geometry} {kind}"
                    same(got, want, what)
                    same(got, tuple(np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in auto), what + " vs automatic")
                    rows = piece if kind == "host" else min(piece, nb)
                    assert plan["PIECE_ROWS"] == rows and plan["PIECES"] == -(-nb // rows), (what, plan)
                    assert plan["SPLITS"] == splits, (what, plan)
                    if qrows:
                        assert plan["QUERY_ROWS"] == min(qrows, nq) and plan["QUERY_GROUPS"] == -(-nq // min(qrows, nq)), (what, plan)
                    else:
                        assert plan["QUERY_GROUPS"] == 1, (what, plan)
                    assert plan["LIST_ROWS"] == max(256, k) and plan["VEC_XQ"] == 0 and plan["VEC_XB"] == (d % 4 == 0), (what, plan)
        if shape == kc.SHAPES[0] and piece == 4096:
            _capi.knn(xq, xb, 65, "ip")
            full = _capi.knn_last_plan()
            assert full["PIECES"] == 5
            _capi.knn(xq, xb[:8000], 65, "ip")
            part = _capi.knn_last_plan()
            assert part["PIECES"] == 2 and part["WORKSPACE_BYTES"] == full["WORKSPACE_BYTES"] > 0   # device memory does not follow nb
    finally:
        _capi.knn_set_geometry(0, 0, 0)


@pytest.mark.parametrize("k", [64, 1024])
@pytest.mark.parametrize("metric", kc.METRICS)
def test_adversarial_order_every_row_a_new_best(oracle, metric, k):
    xq, xb = kc.adversarial()
    D, I = _capi.knn(xq, xb, k, metric)
    same((D, I), kc.truth(oracle, "adversarial", xq, xb, k, metric), f"{metric} k={k}")
    if metric == "ip":
        np.testing.assert_array_equal(I[0], 4999 - np.arange(k))   # +u: the stream ascends, every row beats the threshold
        np.testing.assert_array_equal(I[1], np.arange(k))          # -u
    dq, db = on_device(xq, xb)
    same(_capi.knn(dq, db, k, metric), (D, I), f"{metric} k={k} device")


@pytest.mark.parametrize("metric", kc.METRICS)
@pytest.mark.parametrize("nb", [0, 1, 4, 31, 33])
def test_padding_when_the_base_is_shorter_than_k(oracle, nb, metric):
    xq, xb = kc.case(*kc.SHAPES[0])
    xq, xb = xq[:37], xb[:nb]
    D, I = _capi.knn(xq, xb, 64, metric)
    same((D, I), kc.truth(oracle, ("pad", nb), xq, xb, 64, metric), f"nb={nb} {metric}")
    assert np.all(I[:, nb:] == -1) and np.all(D[:, nb:] == (-FLT_MAX if metric == "ip" else FLT_MAX)) and np.all(I[:, :nb] >= 0)
    dq, db = on_device(xq, xb)
    same(_capi.knn(dq, db, 64, metric), (D, I), f"nb={nb} {metric} device")


@pytest.mark.parametrize("metric", kc.METRICS)
def test_no_queries_writes_nothing(metric):
    xq, xb = kc.case(*kc.SHAPES[0])
    D, I = _capi.knn(xq[:0], xb, 64, metric)
    assert D.shape == (0, 64) and I.shape == (0, 64)
    guard_d, guard_i = np.full((2, 64), 7, np.float32), np.full((2, 64), 7, np.int64)
    rc = _capi.lib().lmi_knn(0, xq.ctypes.data, 0, xb.ctypes.data, xb.shape[0], xb.shape[1], 64, _capi.KNN_METRICS[metric],
                             guard_d.ctypes.data, guard_i.ctypes.data, 0)
    assert rc == 0 and np.all(guard_d == 7) and np.all(guard_i == 7)


@pytest.mark.parametrize("metric", kc.METRICS)
def test_device_tensors(oracle, metric):
    shape = kc.SHAPES[1]   # d = 768: 16-byte loads where the base allows them
    xq, xb = kc.case(*shape)
    k = 65
    want = kc.truth(oracle, shape, xq, xb, k, metric)
    dq, db = on_device(xq, xb)
    D, I = _capi.knn(dq, db, k, metric)
    assert D.is_cuda and I.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64 and D.device == dq.device
    assert _capi.knn_last_plan()["VEC_XB"] == 1
    same((D, I), want, "device")
    same((D, I), _capi.knn(xq, xb, k, metric), "device vs host")
    assert np.array_equal(dq.cpu().numpy(), xq) and np.array_equal(db.cpu().numpy(), xb)   # only read
    D2, I2 = _capi.knn(dq, db, k, metric)
    assert torch.equal(D.view(torch.int32), D2.view(torch.int32)) and torch.equal(I, I2)
    # a base that is 4-byte but not 16-byte aligned is read element by element
    flat = torch.empty(xb.size + 1, dtype=torch.float32, device=db.device)
    off = flat[1:].view(xb.shape)
    off.copy_(db)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    same(_capi.knn(dq, off, k, metric), want, "offset base")
    assert _capi.knn_last_plan()["VEC_XB"] == 0
    qflat = torch.empty(xq.size + 1, dtype=torch.float32, device=db.device)
    qoff = qflat[1:].view(xq.shape)
    qoff.copy_(dq)
    same(_capi.knn(qoff, off, k, metric), want, "offset queries and base")


@pytest.mark.parametrize("metric", kc.METRICS)
def test_special_values_do_what_the_oracle_does(oracle, metric):
    xq, xb = kc.special()
    want = kc.truth(oracle, "special", xq, xb, 64, metric)
    got = _capi.knn(xq, xb, 64, metric)
    same(got, want, metric)
    assert not np.any(got[1] == 3)   # the NaN row is never returned
    dq, db = on_device(xq, xb)
    same(_capi.knn(dq, db, 64, metric), want, metric + " device")


def test_refusals_leave_the_outputs_untouched():
    xq, xb = kc.case(*kc.SHAPES[0])
    dq, db = on_device(xq, xb)
    for bad in (dict(k=0), dict(k=1025), dict(metric="cosine")):
        with pytest.raises(ValueError):
            _capi.knn(xq, xb, **{"k": 10, "metric": "ip", **bad})
    for a, b in ((xq, db), (dq, xb)):   # mixed kinds
        with pytest.raises(ValueError):
            _capi.knn(a, b, 10)
    with pytest.raises(ValueError):
        _capi.knn(np.zeros((2, 4097), np.float32), np.zeros((3, 4097), np.float32), 1)
    # the library itself
    L = _capi.lib()
    D, I = np.full((xq.shape[0], 1025), 7, np.float32), np.full((xq.shape[0], 1025), 7, np.int64)
    nq, nb, d = xq.shape[0], xb.shape[0], xq.shape[1]
    q, x = xq.ctypes.data, xb.ctypes.data
    for args in ((q, nq, x, nb, d, 0, 0), (q, nq, x, nb, d, 1025, 0), (q, 1, x, 1, 4097, 1, 0), (q, nq, x, nb, d, 10, 7), (q, nq, x, nb, 0, 10, 0),
                 (q, -1, x, nb, d, 10, 0), (q, nq, x, 1 << 31, d, 10, 0), (None, nq, x, nb, d, 10, 0), (q, nq, None, nb, d, 10, 0)):
        assert L.lmi_knn(0, *args, D.ctypes.data, I.ctypes.data, 0) != 0, args
        assert L.lmi_last_error().startswith(b"lmi_knn:"), args
        assert np.all(D == 7) and np.all(I == 7), args
    assert L.lmi_knn(0, q, nq, x, nb, d, 10, 0, None, I.ctypes.data, 0) != 0 and np.all(I == 7)
    with pytest.raises(_capi.LmiError):
        _capi.knn_set_geometry(-1, 0, 0)
    with pytest.raises(_capi.LmiError):
        _capi.knn_set_geometry(0, 1025, 0)
    _capi.knn_set_geometry(0, 0, 0)


def test_baseline_beyond_k_10():
    """li.Baseline at k = 30 (through lmi_knn), on the data and with the tolerances of test_gpu_build_io.test_baseline_is_gpu_bruteforce."""
    from learnedmetricindex_amd.li.Baseline import Baseline

    rs = np.random.RandomState(3)
    X = rs.randn(3000, 48).astype(np.float32) * rs.uniform(0.1, 10, size=(3000, 1)).astype(np.float32)
    Q = rs.randn(64, 48).astype(np.float32)
    assert Baseline.MAX_K == _capi.KNN_MAX_K == 1024
    d, ids, secs = Baseline().search(Q, X, k=30)
    xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    qn = Q / np.linalg.norm(Q, axis=1, keepdims=True)
    ref = 1 - qn.astype(np.float64) @ xn.astype(np.float64).T
    order = np.argsort(ref, axis=1, kind="stable")[:, :30]
    assert d.shape == ids.shape == (64, 30)
    assert (ids == order + 1).mean() > 0.99 and secs > 0
    np.testing.assert_allclose(d, np.take_along_axis(ref, order, 1), atol=2e-6)
    for k in (5, 12):   # fewer objects than k, on both paths
        d3, ids3, _ = Baseline().search(Q[:4], X[:3], k=k)
        assert np.all(ids3[:, 3:] == 0) and np.all(np.isinf(d3[:, 3:])) and np.all(ids3[:, :3] >= 1)
    with pytest.raises(ValueError):
        Baseline().search(Q, X, k=1025)
