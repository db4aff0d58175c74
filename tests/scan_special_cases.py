"""Seeded inputs of the scan's special-value tests (tests/test_gpu_scan_specials.py on the device, tests/test_scan_specials_host.py on
the oracle alone): NaN, +-inf, subnormal and overflowing values in stored rows and in queries, through lmi_scan_topk.

One shape: N = 4000 clustered, un-normalised rows in L = 4 buckets, 64 queries that visit nb = 3 buckets each, k = 10; every case
at d = 48 (the low-dimensional pass-2 kernels) and d = 160 (the general ones), under both metrics.  The contract the cases pin is the
paragraph at lmi_scan_topk in include/lmi_hip.h; the one pair it leaves unspecified (an infinite query component under L2: the
oracle's distances are NaN) is the one pair missing from CASES.

Stored side (`special_rows` = the rows that carry the special values):
  nan_rows        200 rows with one NaN each
  nan_bucket      every row of bucket 1 carries a NaN: its slots are padded like an empty bucket's
  nan_crowd       for queries 0..8, copies of the query's 1..9 nearest rows of its first bucket with one component NaN, written over
                  far rows of that bucket: NaN candidates right where the selection looks for its tenth-best score
  inf_rows        +-inf in 200 rows; every 4th query has 30 % exact zeros, so some pairs score 0 * inf
  inf_and_large   one row with +inf (the index scale becomes 1) beside components of 1e5 .. 1e6 in every 13th row: finite values
                  that overflow binary16 at that scale
  huge_rows       every 7th row x 1e30: squared norms overflow, inner products reach 1e30
Query side (`special_queries` = the queries that carry them; `plain_Q` = the batch before they were put in):
  nan_q, inf_q    a NaN / +-inf in every 5th query
  tiny_q          every 3rd query x 1e-40: all its components are binary32 subnormals
  subnormal_q     every 3rd query x 2^-130 exactly
  huge_q          every 3rd query x 1e30
  zero_q          every 3rd query all zeros: every score ties

Every array is made once, shared and read-only."""
import collections
import functools

import numpy as np

N, L, NQ, NB, K = 4000, 4, 64, 3, 10
DIMS = (48, 160)
METRICS = ("ip", "l2")
STORED = ("nan_rows", "nan_bucket", "nan_crowd", "inf_rows", "inf_and_large", "huge_rows")
QUERY = ("nan_q", "inf_q", "tiny_q", "subnormal_q", "huge_q", "zero_q")
CASES = [(name, d, metric) for name in STORED + QUERY for d in DIMS for metric in METRICS if (name, metric) != ("inf_q", "l2")]

Case = collections.namedtuple("Case", "X Q labels order special_rows special_queries plain_Q")


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def base(d: int):
    """(X, Q, labels, order): ordinary data.  Rows and queries around four centres, row norms spread over 0.5 .. 2; a query visits
    the three buckets whose centres are nearest."""
    rs = np.random.RandomState(7000 + d)
    cen = rs.randn(L, d).astype(np.float32)
    labels = rs.randint(0, L, size=N).astype(np.int64)
    X = (cen[labels] + np.float32(0.8) * rs.randn(N, d).astype(np.float32)) * rs.uniform(0.5, 2.0, size=(N, 1)).astype(np.float32)
    Q = cen[rs.randint(0, L, size=NQ)] + np.float32(0.8) * rs.randn(NQ, d).astype(np.float32)
    order = np.argsort(((Q[:, None, :] - cen[None, :, :]) ** 2).sum(-1), axis=1, kind="stable")[:, :NB].astype(np.int32)
    return _frozen(X.astype(np.float32)), _frozen(Q.astype(np.float32)), _frozen(labels), _frozen(np.ascontiguousarray(order))


def _nearest(X, q, rows, metric):
    """`rows` ordered from the query's nearest on, in float64."""
    x = X[rows].astype(np.float64)
    key = x @ q.astype(np.float64) - (0.5 * (x * x).sum(1) if metric == "l2" else 0.0)
    return rows[np.argsort(-key, kind="stable")]


@functools.lru_cache(maxsize=None)
def case(name: str, d: int, metric: str = "ip") -> Case:
    X0, Q0, labels, order = base(d)
    X, Q = X0.copy(), Q0.copy()
    rs = np.random.RandomState(sum(map(ord, name)) * 1000 + d)
    rows = np.zeros(0, np.int64)
    queries = np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        if name == "nan_rows":
            rows = np.sort(rs.choice(N, 200, replace=False))
            X[rows, rs.randint(0, d, size=200)] = np.nan
        elif name == "nan_bucket":
            rows = np.flatnonzero(labels == 1)
            X[rows, rs.randint(0, d, size=rows.size)] = np.nan
        elif name == "nan_crowd":
            ranked = [_nearest(X0, Q0[q], np.flatnonzero(labels == order[q, 0]), metric) for q in range(9)]
            near = set(int(r) for lst in ranked for r in lst[:50])
            taken, picked = set(), []
            for q, lst in enumerate(ranked):
                far = [int(r) for r in lst[::-1] if int(r) not in near and int(r) not in taken][:q + 1]
                taken.update(far)
                for victim, src in zip(far, lst[:q + 1]):
                    X[victim] = X0[src]
                    X[victim, rs.randint(0, d)] = np.nan
                    picked.append(victim)
            rows = np.sort(np.array(picked, np.int64))
        elif name == "inf_rows":
            rows = np.sort(rs.choice(N, 200, replace=False))
            X[rows, rs.randint(0, d, size=200)] = np.where(np.arange(200) % 2 == 0, np.inf, -np.inf).astype(np.float32)
            for q in range(0, NQ, 4):
                Q[q, rs.rand(d) < 0.3] = 0.0
            Q0 = Q.copy()   # (the zeros belong to the ordinary batch of this case)
        elif name == "inf_and_large":
            rows = np.arange(0, N, 13, dtype=np.int64)
            for r in rows[1:]:
                cols = rs.choice(d, 3, replace=False)
                X[r, cols] = (rs.choice([-1.0, 1.0], size=3) * rs.uniform(1e5, 1e6, size=3)).astype(np.float32)
            X[rows[0], rs.randint(0, d)] = np.inf
        elif name == "huge_rows":
            rows = np.arange(0, N, 7, dtype=np.int64)
            X[rows] *= np.float32(1e30)
        elif name == "nan_q":
            queries = np.arange(0, NQ, 5, dtype=np.int64)
            Q[queries, rs.randint(0, d, size=queries.size)] = np.nan
        elif name == "inf_q":
            queries = np.arange(0, NQ, 5, dtype=np.int64)
            Q[queries, rs.randint(0, d, size=queries.size)] = np.where(np.arange(queries.size) % 2 == 0, np.inf, -np.inf).astype(np.float32)
        elif name == "tiny_q":
            queries = np.arange(0, NQ, 3, dtype=np.int64)
            Q[queries] *= np.float32(1e-40)
        elif name == "subnormal_q":
            queries = np.arange(0, NQ, 3, dtype=np.int64)
            Q[queries] *= np.float32(2.0 ** -130)
        elif name == "huge_q":
            queries = np.arange(0, NQ, 3, dtype=np.int64)
            Q[queries] *= np.float32(1e30)
        elif name == "zero_q":
            queries = np.arange(0, NQ, 3, dtype=np.int64)
            Q[queries] = 0.0
        else:
            raise ValueError(name)
    return Case(_frozen(X), _frozen(Q), labels, order, _frozen(rows), _frozen(queries), _frozen(np.ascontiguousarray(Q0)))


def search(oracle, X, Q, labels, order, metric, ids=None, nthreads=4):
    """oracle.search over the given visiting order: (dists f64 [nq, K], ids u32 [nq, K])."""
    with np.errstate(all="ignore"):
        do, io, _ = oracle.search(None, None, X, Q, np.asarray(labels)[:, None], NB, K, ids=ids, nthreads=nthreads,
                                  bucket_order=np.asarray(order)[:, :, None], metric=metric)
    return do, io


_ORACLE = {}


def truth(oracle, name: str, d: int, metric: str):
    """The oracle's answer of a case, computed once (it does not depend on the thread count: test_scan_specials_host.py)."""
    key = (name, d, metric)
    if key not in _ORACLE:
        c = case(name, d, metric)
        do, io = search(oracle, c.X, c.Q, c.labels, c.order, metric)
        _ORACLE[key] = (_frozen(do), _frozen(io))
    return _ORACLE[key]


def split(c: Case):
    """(kept, inserted): each (rows, labels, ids) -- the case's objects without the special rows, and the special rows, ids as in a
    plain build (row + 1).  Building `kept` and inserting `inserted` stores every bucket in the order of a build from kept + inserted."""
    keep = np.ones(N, bool)
    keep[c.special_rows] = False
    ids = np.arange(1, N + 1, dtype=np.uint32)
    return tuple((np.ascontiguousarray(c.X[m]), np.ascontiguousarray(c.labels[m]), np.ascontiguousarray(ids[m])) for m in (keep, ~keep))
