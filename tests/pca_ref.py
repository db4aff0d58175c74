"""`lmi_gram` and `lmi_project` restated in numpy on top of the unchanged oracle's `dot` (the k-ordered fmaf chain) and of
kmeans_ref's update (the int64 mean) -- shared by test_pca_host.py and test_gpu_pca.py.  include/lmi_hip.h states the contract."""
import functools

import numpy as np

import kmeans_ref

PIECE = 4096   # LMI_GRAM_PIECE_ROWS


def mean_ref(x):
    """(mean f32[d], e): lmi_kmeans's update with one cluster."""
    e = kmeans_ref.exponent(x)
    return kmeans_ref.update(x, np.zeros(x.shape[0], dtype=np.int64), np.zeros((1, x.shape[1]), dtype=np.float32), e)[0], e


def gram_ref(oracle, x):
    """(mean f32[d], gram f64[d,d], e)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    mean, e = mean_ref(x)
    c = x - mean   # binary32, one rounding
    T = np.zeros((d, d), dtype=np.int64)
    for p0 in range(0, n, PIECE):
        ct = np.ascontiguousarray(c[p0:p0 + PIECE].T)
        for a in range(d):
            for b in range(a, d):
                T[a, b] += int(np.rint(np.float64(oracle.dot(ct[a], ct[b])) * 2.0 ** (32 - 2 * e)))
    T = np.triu(T) + np.triu(T, 1).T
    return mean, T.astype(np.float64) * 2.0 ** (2 * e - 32), e


def project_ref(oracle, x, basis, mean=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = x if mean is None else x - mean
    return np.array([[oracle.dot(r, b) for b in basis] for r in c], dtype=np.float32).reshape(x.shape[0], basis.shape[0])


def rows(n, d, seed, scale=1.0):
    """f32 [n,d] exactly representable in binary16: columns with their own offset and spread, so that the mean matters."""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, d) * rs.uniform(0.2, 2.0, d) + rs.uniform(-1.5, 1.5, d)
    return (x * scale).astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gram_case(n, d):
    """(x, mean, gram, e) of a case, computed once per process and read-only."""
    from oracle import lmi_oracle

    lmi_oracle.build()
    x = rows(n, d, 100 * d + n % 97)
    out = (x,) + gram_ref(lmi_oracle, x)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def project_case(n, d, m, centred):
    """(x, basis, mean or None, y)"""
    from oracle import lmi_oracle

    lmi_oracle.build()
    x = rows(n, d, 7 * d + n + m)
    basis = np.random.RandomState(m).randn(m, d).astype(np.float32)
    mean = x.mean(axis=0).astype(np.float32) if centred else None
    return x, basis, mean, project_ref(lmi_oracle, x, basis, mean)
