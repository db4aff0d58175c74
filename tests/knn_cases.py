"""Seeded inputs of the lmi_knn tests (tests/test_gpu_knn.py on the device, tests/test_knn_host.py on the oracle alone).

The shapes are the smallest that still cross every seam of the call: d odd and no multiple of 4 (45), d one past a 32-link chunk
(129), d above 768 and no multiple of 32 (1000), a d % 4 == 0 (768, 1000); nq below, one past and several times a 32-query tile; nb
ragged against 32 and against any piece, with ragged ends under the forced pieces and splits of the geometry test.

Every array is made once, shared and read-only."""
import functools

import numpy as np

SHAPES = [(67, 20011, 45), (33, 4099, 768), (129, 9000, 1000), (300, 70001, 129)]
KS = [1, 10, 11, 64, 65, 1024]
METRICS = ["ip", "l2"]
GEOMETRIES = [(4096, 1, 0), (4096, 3, 32), (20011, 8, 0), (1000, 2, 40)]   # (piece_rows, splits, query_rows); 0 = automatic
TIE_QUERIES = 8


def tie_group(nb: int) -> np.ndarray:
    """52 rows that all hold row 17's vector, spread over distant tiles, splits and pieces; ascending."""
    return np.array([17] + list(range(nb // 4, nb // 4 + 40)) + list(range(nb - 11, nb)), dtype=np.int64)


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def case(nq: int, nb: int, d: int, seed: int = 2023):
    """(xq, xb): standard-normal rows; the rows of tie_group(nb) all equal row 17; the first TIE_QUERIES queries are 0.5 * row 17,
    so for them the group is the top of both metrics, in ascending row order."""
    rs = np.random.RandomState(seed)
    xb = rs.randn(nb, d).astype(np.float32)
    xq = rs.randn(nq, d).astype(np.float32)
    xb[tie_group(nb)] = xb[17]
    xq[:TIE_QUERIES] = np.float32(0.5) * xb[17]
    return _frozen(xq), _frozen(xb)


@functools.lru_cache(maxsize=None)
def adversarial():
    """(xq, xb): xb[i] = ((i + 1) / 5000) * u, queries +u and -u.  For the inner product +u meets every row as a new best (the result
    is rows 4999, 4998, ..) and -u ranks rows 0, 1, ..: a stream that the threshold never thins out."""
    nb, d = 5000, 8
    u = np.random.RandomState(7).randn(d).astype(np.float32)
    scale = ((np.arange(nb, dtype=np.float64) + 1) / nb).astype(np.float32)
    xb = scale[:, None] * u[None, :]
    xq = np.stack([u, -u]).astype(np.float32)
    return _frozen(xq), _frozen(np.ascontiguousarray(xb, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def special():
    """(xq, xb): a base row of NaN, a row holding +inf, a row scaled by 2^-70 (its squared norm is subnormal), an all-zero query."""
    rs = np.random.RandomState(11)
    xb = rs.randn(2000, 45).astype(np.float32)
    xq = rs.randn(5, 45).astype(np.float32)
    xb[3] = np.nan
    xb[5, 0] = np.inf
    xb[7] *= np.float32(2.0 ** -70)
    xq[2] = 0
    return _frozen(xq), _frozen(xb)


_ORACLE = {}


def truth(oracle, name: str, xq, xb, k: int, metric: str):
    """oracle.knn_ip / knn_l2 of a named input at this k, computed once (the oracle's result does not depend on its thread count)."""
    key = (name, k, metric)
    if key not in _ORACLE:
        with np.errstate(all="ignore"):
            D, I = (oracle.knn_ip if metric == "ip" else oracle.knn_l2)(xq, xb, k, nthreads=8)
        _ORACLE[key] = (_frozen(D), _frozen(I))
    return _ORACLE[key]
