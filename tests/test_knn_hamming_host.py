"""CPU (`-m "not gpu"`): the host side of lmi_knn_hamming.  `_capi.knn_hamming` and `Baseline.search_hamming` refuse bad arguments
before the library is loaded, and `search_hamming` hands uint64 word arrays on as bytes without a copy (against a stand-in for the
binding: no GPU call is made)."""
import numpy as np
import pytest

from learnedmetricindex_amd import _capi
from learnedmetricindex_amd.li import Baseline as baseline_module


class FakeTensor:
    """What `_capi` asks of a device tensor."""

    ndim, is_cuda, device, dtype, shape = 2, True, "cuda:0", "torch.uint8", (5, 16)

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return True


@pytest.fixture
def no_lib(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", refuse)


def test_knn_hamming_raises_before_the_library_loads(no_lib):
    q, x = np.zeros((3, 16), np.uint8), np.zeros((5, 16), np.uint8)
    for a, b in ((q.astype(np.float32), x), (q, x.astype(np.int8)), (q.view(np.uint64), x.view(np.uint64)),   # dtype
                 (q[0], x), (q, x[None]), (q, None),                                                            # rank, kind
                 (q, x[:, :12]), (q[:, :6], x[:, :6]), (np.zeros((3, 516), np.uint8), np.zeros((5, 516), np.uint8)),   # widths
                 (q[:, :0], x[:, :0])):
        with pytest.raises(ValueError, match="knn_hamming"):
            _capi.knn_hamming(a, b)
    for a, b in ((q, FakeTensor()), (FakeTensor(), x)):   # an array beside a tensor
        with pytest.raises(ValueError, match="both"):
            _capi.knn_hamming(a, b)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k "):
            _capi.knn_hamming(q, x, k)


def test_search_hamming_raises_before_the_library_loads(no_lib):
    b = baseline_module.Baseline()
    q, x = np.zeros((3, 16), np.uint8), np.zeros((5, 16), np.uint8)
    for a, c, k in ((q.astype(np.float32), x, 10), (q, x.view(np.uint32), 10), (q[0], x, 10), (q, x, 0), (q, x, 1025),
                    (q.view(np.uint64), x[:, :8], 10)):
        with pytest.raises(ValueError, match="hamming"):
            b.search_hamming(a, c, k)


def test_search_hamming_views_words_as_bytes_without_a_copy(monkeypatch):
    seen = []

    def fake(xq, xb, k=10, device=0):
        seen.append((xq, xb))
        return np.array([[3, 9, 2 ** 31 - 1]], np.int32), np.array([[4, 0, -1]], np.int64)

    monkeypatch.setattr(baseline_module._capi, "knn_hamming", fake)
    q, x = np.arange(16, dtype=np.uint64).reshape(1, 16), np.arange(80, dtype=np.uint64).reshape(5, 16)   # 1024-bit sketches
    dists, ids, seconds = baseline_module.Baseline().search_hamming(q, x, 3)
    (bq, bx), = seen
    assert bq.dtype == bx.dtype == np.uint8 and bq.shape == (1, 128) and bx.shape == (5, 128)
    assert np.shares_memory(bq, q) and np.shares_memory(bx, x) and bx.tobytes() == x.tobytes()
    np.testing.assert_array_equal(ids, [[5, 1, 0]])   # 1-based; padding becomes 0
    np.testing.assert_array_equal(dists, [[3, 9, np.iinfo(np.int32).max]])
    assert dists.dtype == np.int32 and seconds >= 0
