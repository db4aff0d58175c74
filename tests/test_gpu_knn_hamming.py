"""GPU (`-m gpu`): lmi_knn_hamming, the exact Hamming k-NN on bit-packed codes (include/lmi_hip.h), against exact
integer numpy: the bits of the XOR counted, a stable argsort, the first k, padded.  Every comparison is array_equal."""
import functools

import numpy as np
import pytest
import torch

from learnedmetricindex_amd import _capi

pytestmark = pytest.mark.gpu

INT32_MAX = np.iinfo(np.int32).max
# dword and 16-byte tile loads, a row pitch that is no multiple of 16 bytes, one chunk of 8 words, a partial last chunk, the widest code
CODE_BYTES = [4, 12, 16, 36, 128, 132, 512]


@functools.lru_cache(maxsize=None)
def case(nq, nb, cb):
    """(xq, xb, all distances int64[nq, nb]), read-only.  At 4 bytes there are 33 distinct distances: every list is full of ties."""
    rs = np.random.RandomState(1000 * cb + nb + nq)
    xq, xb = rs.randint(0, 256, (nq, cb), dtype=np.uint8), rs.randint(0, 256, (nb, cb), dtype=np.uint8)
    dist = np.unpackbits(xq[:, None, :] ^ xb[None, :, :], axis=-1).sum(-1).astype(np.int64)
    for a in (xq, xb, dist):
        a.setflags(write=False)
    return xq, xb, dist


def truth(dist, k):
    nq, nb = dist.shape
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    D, I = np.full((nq, k), INT32_MAX, np.int32), np.full((nq, k), -1, np.int64)
    D[:, :order.shape[1]] = np.take_along_axis(dist, order, axis=1)
    I[:, :order.shape[1]] = order
    return D, I


def same(got, want, what):
    D, I = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in got)
    assert D.dtype == np.int32 and I.dtype == np.int64, what
    np.testing.assert_array_equal(I, want[1], err_msg=f"I {what}")
    np.testing.assert_array_equal(D, want[0], err_msg=f"D {what}")


def on_device(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)


@pytest.mark.parametrize("k", [1, 10, 300])
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("nb", [1, 255, 256, 257])
@pytest.mark.parametrize("cb", CODE_BYTES)
def test_parity_with_numpy_from_host_arrays_and_device_tensors(cb, nb, nq, k):
    xq, xb, dist = case(nq, nb, cb)
    want = truth(dist, k)
    same(_capi.knn_hamming(xq, xb, k), want, "host")
    assert _capi.knn_last_plan()["VEC_XB"] == (cb % 16 == 0)
    same(_capi.knn_hamming(*on_device(xq, xb), k), want, "device")


@pytest.mark.parametrize("cb", [4, 36, 128])
def test_forced_geometry_changes_nothing(cb):
    """10 pieces of 100 rows, 3 splits each, query groups of 33 (two tiles, the second of one query) with a ragged last group."""
    xq, xb, dist = case(70, 1000, cb)
    want = truth(dist, 300)
    auto = _capi.knn_hamming(xq, xb, 300)
    try:
        _capi.knn_set_geometry(piece_rows=100, splits=3, query_rows=33)
        forced = _capi.knn_hamming(xq, xb, 300), _capi.knn_hamming(*on_device(xq, xb), 300)
        plan = _capi.knn_last_plan()
    finally:
        _capi.knn_set_geometry(0, 0, 0)
    assert tuple(plan[w] for w in ("PIECES", "PIECE_ROWS", "SPLITS", "QUERY_GROUPS", "QUERY_ROWS")) == (10, 100, 3, 3, 33)
    for got, what in ((auto, "auto"), (forced[0], "forced host"), (forced[1], "forced device")):
        same(got, want, what)


@pytest.mark.parametrize("cb", CODE_BYTES)
def test_planted_answers(cb):
    """A query equal to a stored row returns it first at distance 0; an all-ones query against an all-zeros row gives 8 * code_bytes."""
    xq, xb = (np.array(a) for a in case(33, 257, cb)[:2])
    xq[0], xb[5], xq[1] = xb[200], 0, 255
    D, I = _capi.knn_hamming(xq, xb, 257)
    assert (D[0, 0], I[0, 0]) == (0, 200)
    assert (D[1, -1], I[1, -1]) == (8 * cb, 5)
    D, I = _capi.knn_hamming(xq, np.empty((0, cb), np.uint8), 3)   # nb == 0 is all padding
    assert np.all(D == INT32_MAX) and np.all(I == -1)


def test_refusals_by_name_leave_the_outputs_untouched():
    L = _capi.lib()
    xq, xb = np.zeros((2, 520), np.uint8), np.zeros((5, 520), np.uint8)
    D, I = np.full((2, 1025), 7, np.int32), np.full((2, 1025), 7, np.int64)
    q, x = xq.ctypes.data, xb.ctypes.data
    # (xq, nq, xb, nb, code_bytes, k)
    for args in ((q, 2, x, 5, 6, 3), (q, 2, x, 5, 0, 3), (q, 2, x, 5, 516, 3), (q, 2, x, 5, 16, 0), (q, 2, x, 5, 16, 1025),
                 (q, -1, x, 5, 16, 3), (q, 2, x, 1 << 31, 16, 3), (None, 2, x, 5, 16, 3), (q, 2, None, 5, 16, 3), (q + 1, 2, x, 5, 16, 3)):
        assert L.lmi_knn_hamming(0, *args, D.ctypes.data, I.ctypes.data, 0) != 0, args
        assert L.lmi_last_error().startswith(b"lmi_knn_hamming:"), args
        assert np.all(D == 7) and np.all(I == 7), args
        assert not any(_capi.knn_last_plan().values())
    assert L.lmi_knn_hamming(0, q, 0, x, 5, 16, 3, None, None, 0) == 0   # nq == 0 writes nothing and succeeds
