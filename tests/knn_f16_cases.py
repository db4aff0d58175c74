"""Seeded binary16 inputs of the lmi_knn_f16 / lmi_knn_range_f16 tests (tests/test_gpu_knn_f16.py on the device,
tests/test_knn_f16_host.py on the oracle alone).

Every array is drawn as binary32, narrowed ONCE to binary16 and widened again: `Case.q16 / x16` go to the `_f16` calls, `Case.q32 / x32`
-- the same values -- to the oracle and to the binary32 calls.  The shapes are the smallest that cross the seams of the half load
path (16-byte groups of 8 halves against d, the 32-link chunk and the row's end):

  (5, 300, 8)       one 16-byte group; the L2 tail (link d = 8) opens the second
  (33, 1027, 40)    16-byte form; the second group of the last chunk's lanes starts at d; the last row ends the allocation
  (33, 1027, 44)    d % 4 == 0 and d % 8 != 0: the float path would vectorise, the half path must not
  (67, 2011, 45)    odd d, 90-byte rows
  (40, 3001, 136)   16-byte form, d % 32 != 0
  (129, 1500, 264)  more than one 32-query tile (and a CT = 4 launch), nine chunks

The tie group is knn_cases.tie_group's 52 rows; they hold twice the base's longest row, so that by Cauchy-Schwarz no other row can
reach them for a query that equals them -- under either metric, at any d -- and the first TIE_QUERIES queries are that vector.

Every array is made once, shared and read-only."""
import collections
import functools

import numpy as np

import knn_cases as kc
import knn_range_ref as kr

SHAPES = [(5, 300, 8), (33, 1027, 40), (33, 1027, 44), (67, 2011, 45), (40, 3001, 136), (129, 1500, 264)]
KS = [1, 10, 65, 1024]
METRICS = kc.METRICS
RANGE_SHAPES = [SHAPES[1], SHAPES[3], SHAPES[4]]
RANGE_K = 128                    # the truth the range reference is a prefix of
RECIPE_J = (0, 9, 40, None)      # radius[q] = the j-th distance of the truth, j = RECIPE_J[q mod 4]; None: just below the nearest
VEC_SHAPE, ODD_SHAPE = SHAPES[4], SHAPES[3]   # the forced-geometry shapes: a 16-byte one and d = 45

Case = collections.namedtuple("Case", "q16 x16 q32 x32")


def geometries(nb: int):
    """(piece_rows, splits, query_rows); 0 = automatic"""
    return [(256, 1, 0), (1000, 3, 32), (nb, 8, 0), (1000, 2, 40)]


def tie_queries(nq: int) -> int:
    return min(kc.TIE_QUERIES, nq)


def _frozen(a):
    a.flags.writeable = False
    return a


def widen(a16):
    return np.ascontiguousarray(a16, dtype=np.float32)


def _case_of(q16, x16):
    return Case(_frozen(np.ascontiguousarray(q16)), _frozen(np.ascontiguousarray(x16)), _frozen(widen(q16)), _frozen(widen(x16)))


@functools.lru_cache(maxsize=None)
def case(nq: int, nb: int, d: int, seed: int = 2025) -> Case:
    rs = np.random.RandomState(seed)
    x16 = rs.randn(nb, d).astype(np.float32).astype(np.float16)
    q16 = rs.randn(nq, d).astype(np.float32).astype(np.float16)
    longest = int(np.argmax((x16.astype(np.float64) ** 2).sum(axis=1)))
    x16[kc.tie_group(nb)] = np.float16(2) * x16[longest]   # exact in binary16
    q16[:tie_queries(nq)] = x16[17]
    return _case_of(q16, x16)


@functools.lru_cache(maxsize=None)
def special(d: int) -> Case:
    """A base row of NaN, a row holding +inf, a row of binary16 subnormals, a row of -0.0, rows of +65504 and -65504 (the largest
    halves), an all-zero query and a query of -0.0."""
    rs = np.random.RandomState(11)
    x16 = rs.randn(700, d).astype(np.float32).astype(np.float16)
    q16 = rs.randn(6, d).astype(np.float32).astype(np.float16)
    x16[3] = np.nan
    x16[5, 0] = np.inf
    x16[7] = (np.arange(d) % 1023 + 1).astype(np.uint16).view(np.float16)   # bit patterns 1 ..: subnormals
    x16[9] = np.float16(-0.0)
    x16[11] = np.float16(65504)
    x16[13] = np.float16(-65504)
    x16[699, d - 1] = np.float16(65504)     # the allocation's last half
    q16[2] = 0
    q16[3] = np.float16(-0.0)
    return _case_of(q16, x16)


def truth(oracle, name, c: Case, k: int, metric: str):
    """oracle.knn_ip / knn_l2 of the WIDENED arrays, computed once (knn_cases' cache, under a name of this module's own)."""
    return kc.truth(oracle, ("f16", name), c.q32, c.x32, k, metric)


_recipe = {}


def recipe(oracle, shape, metric):
    """(radius f32[nq], (lims, dists, rows)): per query the RECIPE_J-th distance of the truth at RANGE_K -- some row's distance, so
    dist == radius is met -- or, every fourth query, the float just below the nearest distance: an empty run.  The reference is
    knn_range_ref.prefix_ref of them."""
    key = (shape, metric)
    if key not in _recipe:
        c = case(*shape)
        D, I = truth(oracle, shape, c, RANGE_K, metric)
        dd = kr.dists_of(D, metric)
        nq = shape[0]
        radius = np.empty(nq, dtype=np.float32)
        for q in range(nq):
            j = RECIPE_J[q % len(RECIPE_J)]
            radius[q] = np.nextafter(dd[q, 0], np.float32(-np.inf)) if j is None else dd[q, j]
        ref = kr.prefix_ref(D, I, radius, metric)
        for a in (radius,) + ref:
            a.setflags(write=False)
        _recipe[key] = (radius, ref)
    return _recipe[key]
