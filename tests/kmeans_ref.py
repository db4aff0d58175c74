"""`lmi_kmeans` restated in numpy on top of the unchanged oracle -- shared by test_kmeans_host.py and test_gpu_kmeans.py.

Definition (include/lmi_hip.h): pass it = 0..niter assigns every row to the centroid with the greatest LMI_METRIC_L2 key
(`oracle.knn_l2(x, c, k=1)`: k-ordered fmaf chains, ties to the lower centroid); changed[it] counts the labels that moved
(labels start at -1); after every pass but the last a cluster with rows gets c = float32(S / cnt * 2^(e-36)), S the int64 sum of
q(x) = rint(x * 2^(36-e)) over its rows, e the smallest integer with max|x| < 2^e (0 for all-zero data); an empty cluster keeps
its centroid.  A pass it >= 1 that moves no label is a fixed point: the rest of `changed` is 0."""
import functools

import numpy as np

NITER = 8
#: (n, d, k, seed) -> (empty clusters at the end, pass of the fixed point or None) for niter = 8
CASES = {(3001, 45, 7, 1): (0, None), (2500, 770, 130, 2): (13, 3), (4099, 33, 33, 3): (0, None), (600, 768, 257, 4): (1, 3),
         (1500, 64, 20, 5): (1, None), (1500, 64, 40, 6): (0, 7)}   # the last two: 16-byte row loads against one and two tiles


def exponent(x):
    m = float(np.abs(x).max()) if x.size else 0.0
    return 0 if m == 0.0 else int(np.frexp(m)[1])   # m = f * 2^e with f in [0.5, 1): the smallest e with m < 2^e


def assign(oracle, x, c):
    return oracle.knn_l2(x, c, k=1, nthreads=4)[1][:, 0].astype(np.int32)


def update(x, labels, c, e):
    k, d = c.shape
    q = np.rint(x.astype(np.float64) * 2.0 ** (36 - e)).astype(np.int64)
    S = np.zeros((k, d), dtype=np.int64)
    np.add.at(S, labels, q)
    cnt = np.bincount(labels, minlength=k).astype(np.int64)
    out = c.copy()
    has = cnt > 0
    out[has] = (S[has].astype(np.float64) / cnt[has, None].astype(np.float64) * 2.0 ** (e - 36)).astype(np.float32)
    return out


def kmeans_ref(oracle, x, c0, niter):
    """(centroids f32[k,d], labels i32[n], counts i64[k], changed i64[niter+1])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = np.array(c0, dtype=np.float32, order="C")
    e = exponent(x)
    labels = np.full(x.shape[0], -1, dtype=np.int32)
    changed = np.zeros(niter + 1, dtype=np.int64)
    for it in range(niter + 1):
        new = assign(oracle, x, c)
        changed[it] = int((new != labels).sum())
        labels = new
        if it == niter or (it >= 1 and changed[it] == 0):
            break
        c = update(x, labels, c, e)
    return c, labels, np.bincount(labels, minlength=c.shape[0]).astype(np.int64), changed


def make_case(n, d, k, seed):
    """(x f32[n,d] with normalised rows, c0 f32[k,d]): a mixture with two equal initial centroids and duplicate rows."""
    rs = np.random.RandomState(seed)
    cen = rs.randn(max(k // 2, 2), d)
    x = (cen[rs.randint(0, len(cen), n)] + 0.7 * rs.randn(n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    init = rs.choice(n, k, replace=False)
    x[init[1]] = x[init[0]]
    x[5:9] = x[4]
    return x, x[init].copy()


@functools.lru_cache(maxsize=None)
def _case(n, d, k, seed, niter):
    from oracle import lmi_oracle

    lmi_oracle.build()
    x, c0 = make_case(n, d, k, seed)
    out = (x, c0) + kmeans_ref(lmi_oracle, x, c0, niter)
    for a in out:
        a.setflags(write=False)
    return out


def case(n, d, k, seed, niter=NITER):
    """(x, c0, centroids, labels, counts, changed) of a case, computed once per process and read-only."""
    return _case(n, d, k, seed, niter)
