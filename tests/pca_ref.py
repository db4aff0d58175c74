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


def _poke(x, i, j, v):
    x[i, j] = v
    return x


def _const_and_equal(x):
    x[:, 3], x[:, 8] = 2.5, x[:, 5]
    return x


def _halves_only(x):
    """Rows that only binary16 data brings: the largest halves of either sign, half subnormals, -0.0."""
    d = x.shape[1]
    x[0], x[1] = 65504.0, -65504.0
    x[1, ::2] = 65504.0
    x[2] = (1 + np.arange(d) * 37 % 1023) * 2.0 ** -24 * np.where(np.arange(d) % 3, 1.0, -1.0)
    x[3] = -0.0
    return x


#: name -> (x = f(rows(n, d, seed), rs), the exponent e the contract gives it); `plain` is the untransformed base of the others
VALUES = {
    "plain": (lambda x, rs: x, 3),
    "down70": (lambda x, rs: x * np.float32(2.0 ** -70), -67),                 # products of two centred values: binary32 subnormals
    "up40": (lambda x, rs: x * np.float32(2.0 ** 40), 43),
    "last_exponent": (lambda x, rs: _poke(x * np.float32(2.0 ** 40), x.shape[0] // 2, x.shape[1] // 3, 2.0 ** 56 - 2.0 ** 32), 56),
    "full_mantissa": (lambda x, rs: (rs.randn(*x.shape) * 3).astype(np.float32), 4),
    "zero": (lambda x, rs: np.zeros_like(x), 0),
    "const_and_equal": (lambda x, rs: _const_and_equal(x), 3),
    "halves_only": (lambda x, rs: _halves_only(x), 16),
}
GRAM_VALUE_NAMES = sorted(set(VALUES) - {"plain"})
GRAM_VALUE_SHAPES = [(4097, 33), (4100, 44)]


def values(name, n, d):
    """f32 [n,d] of a VALUES case; `plain`, `up40` and `down70` of one (n, d) are the same rows at three scales.  The base is
    rows() at half scale: max|x| of 10^5 such values lies in [4, 8), e = 3, which the exponents of the table count from."""
    seed = 100 * d + n % 97
    x = VALUES[name][0](rows(n, d, seed, scale=0.5), np.random.RandomState(seed + 1))
    assert x.dtype == np.float32 and x.shape == (n, d)
    return x


@functools.lru_cache(maxsize=None)
def gram_values_case(name, n, d):
    """(x, mean, gram, e) of a VALUES case, computed once per process and read-only."""
    from oracle import lmi_oracle

    lmi_oracle.build()
    x = values(name, n, d)
    out = (x,) + gram_ref(lmi_oracle, x)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _nonfinite(x):
    x[7, 3], x[9, 4] = np.nan, np.inf
    return x


#: name -> (x = f(rows), basis = g(basis)) at PROJECT_VALUE_SHAPE; `clean` is what `nonfinite` pokes
PROJECT_VALUES = {
    "clean": (lambda x, rs: x, lambda b: b),
    "full_mantissa": (VALUES["full_mantissa"][0], lambda b: b),
    "down70": (VALUES["down70"][0], lambda b: b),
    "neg_zero_row": (lambda x, rs: _poke(x, 5, slice(None), -0.0), lambda b: b),
    "zero_basis_row": (lambda x, rs: x, lambda b: _poke(b, 2, slice(None), 0.0)),
    "nonfinite": (lambda x, rs: _nonfinite(x), lambda b: b),
}
PROJECT_VALUE_SHAPE = (70, 44, 33)   # 16-byte loads, a padded chain, two basis tiles (the second holds one row), 4-byte stores
NONFINITE_ROWS = (7, 9)


@functools.lru_cache(maxsize=None)
def project_values_case(name, centred):
    """(x, basis, mean or None, y) of a PROJECT_VALUES case, read-only.  The mean is that of the `clean` rows in every case."""
    from oracle import lmi_oracle

    lmi_oracle.build()
    n, d, m = PROJECT_VALUE_SHAPE
    base = rows(n, d, 7 * d + n + m)
    x = PROJECT_VALUES[name][0](base.copy(), np.random.RandomState(d))
    basis = PROJECT_VALUES[name][1](np.random.RandomState(m).randn(m, d).astype(np.float32))
    mean = None
    if centred:
        mean = base.mean(axis=0).astype(np.float32) * (np.float32(2.0 ** -70) if name == "down70" else np.float32(1))
    with np.errstate(invalid="ignore"):
        y = project_ref(lmi_oracle, x, basis, mean)
    for a in (x, basis, y):
        a.setflags(write=False)
    return x, basis, mean, y


def lattice_rows(n, d, seed):
    """f32 [n,d] exactly representable in binary16, cheap to draw at 10^7 elements: multiples of 2^-8 in [-8, 8)."""
    return np.random.RandomState(seed).randint(-2048, 2048, size=(n, d)).astype(np.float32) / np.float32(256)


@functools.lru_cache(maxsize=None)
def project_pieces_case(n, d, m, piece):
    """(x, basis, mean, rows, y[rows]) of a host call of two pieces: the restatement on the first 64 rows, the 128 around the seam at
    row `piece`, and the last 64."""
    from oracle import lmi_oracle

    lmi_oracle.build()
    x = lattice_rows(n, d, n + m)
    basis = np.random.RandomState(m).randn(m, d).astype(np.float32)
    mean = np.random.RandomState(d).uniform(-1, 1, d).astype(np.float32)
    at = np.concatenate([np.arange(64), np.arange(piece - 64, piece + 64), np.arange(n - 64, n)])
    y = project_ref(lmi_oracle, x[at], basis, mean)
    for a in (x, basis, mean, at, y):
        a.setflags(write=False)
    return x, basis, mean, at, y


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
