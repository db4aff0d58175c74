"""CPU (`-m "not gpu"`): the host side of lmi_knn_rerank.  The symbol is exported, declared and bound with one signature;
`_capi.knn_rerank`, `Baseline.rerank` and `Baseline.search_sketch` refuse bad arguments before the library is loaded."""
import ctypes
import os
import re

import numpy as np
import pytest

from learnedmetricindex_amd import _capi
from learnedmetricindex_amd.li.Baseline import Baseline


class FakeTensor:   # what `_capi` asks of a device tensor before it loads the library
    ndim, is_cuda, device, dtype, shape, data_ptr = 2, True, "cuda:0", "torch.float32", (5, 8), None


@pytest.fixture
def no_lib(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", refuse)


def test_the_symbol_is_exported_declared_and_bound():
    header = open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "lmi_hip.h")).read()
    decl = re.search(r"LMI_API int lmi_knn_rerank\((.*?)\);", header, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", decl).split(",")]
    assert params == ["int device", "const float *xq", "int64_t nq", "const float *xb", "int64_t nb", "int d", "const int64_t *cand",
                      "int c", "int k", "int metric", "float *D", "int64_t *I", "int on_device"]
    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _capi.SIGNATURES["lmi_knn_rerank"] == (i, [i, p, l, p, l, i, p, i, i, i, p, p, i])
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "lmi_knn_rerank")


def test_knn_rerank_raises_before_the_library_loads(no_lib):
    q, x, c = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32), np.zeros((3, 4), np.int64)
    for a, b, cd, k in ((q.astype(np.float64), x, c, 2), (q, x.astype(np.float16), c, 2), (q, x, c.astype(np.int32), 2),   # dtype
                        (q[0], x, c, 2), (q, x, c[0], 2), (q, x, None, 2),                                                  # rank, kind
                        (q, x[:, :6], c, 2), (q[:2], x, c, 2), (q[:, :0], x[:, :0], c, 2),                                  # shapes
                        (q, x, c, 5), (q, x, c, 0), (q, x, c[:, :0], 1), (q, x, np.zeros((3, 1025), np.int64), 3)):         # k, c
        with pytest.raises(ValueError, match="knn_rerank"):
            _capi.knn_rerank(a, b, cd, k)
    with pytest.raises(ValueError, match="metric"):
        _capi.knn_rerank(q, x, c, 2, metric="cosine")
    for a, b in ((q, FakeTensor()), (FakeTensor(), x)):   # an array beside a tensor
        with pytest.raises(ValueError, match="all"):
            _capi.knn_rerank(a, b, c, 2)


def test_baseline_rerank_and_search_sketch_raise_before_the_library_loads(no_lib):
    b = Baseline()
    q, x, ids = np.zeros((3, 8), np.float32), np.zeros((5, 8), np.float32), np.ones((3, 4), np.int64)
    cq, cx = np.zeros((3, 16), np.uint8), np.zeros((5, 16), np.uint8)
    for a, c, cd, k in ((q, x, ids.astype(np.float32), 2), (q, x, ids[0], 2), (q, x, ids, 5), (q, x, ids, 0),
                        (q, x, np.ones((3, 1025), np.int64), 2), (q[:2], x, ids, 2), (q, x[:, :6], ids, 2)):
        with pytest.raises(ValueError, match="rerank"):
            b.rerank(a, c, cd, k)
    for args, kw in (((q, x, cq, cx), dict(k=11, n_candidates=10)), ((q, x, cq, cx), dict(n_candidates=1025)),
                     ((q, x[:, :6], cq, cx), {}), ((q, x, cq[:2], cx), {}), ((q, x, cq, cx.astype(np.float32)), {})):
        with pytest.raises(ValueError, match="sketch|hamming"):
            b.search_sketch(*args, **kw)
