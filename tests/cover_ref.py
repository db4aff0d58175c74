"""The bucket cover and the pruning pass of the exact range search (include/lmi_hip.h, lmi_cover_create / lmi_cover_order) restated in
numpy, and the inputs their tests share (tests/test_cover_host.py on the oracle alone, tests/test_gpu_cover.py on the device).

Centres: the integer rule of lmi_kmeans (`kmeans_ref.update`): q = rint(x * 2^(36-e)) summed in int64 per (bucket, column), one
division, one cast to float32 -- the library's centres are these bits.  Radii: float64, sqrt of the largest sum of squares about
the float32 centre (0 stays 0); the library rounds to float32 and one step up.  The admission rule in float64 with a factor on
the margin: the library's set lies between the sets of factor 1/2 and factor 2.  The order: admitted bucket ids ascending, then -1."""
import numpy as np

import kmeans_ref
import union_ref as ur

ONE = np.float32(1.0)


def cover_of(X, lab, L):
    """dict(n i64[L], c f32[L, d], R f64[L], cn f64[L]) of the objects X f32[N, d] with buckets lab[N]."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    lab = np.asarray(lab, dtype=np.int64)
    d = X.shape[1]
    e = kmeans_ref.exponent(X)
    q = np.rint(X.astype(np.float64) * 2.0 ** (36 - e)).astype(np.int64)
    S = np.zeros((L, d), dtype=np.int64)
    np.add.at(S, lab, q)
    n = np.bincount(lab, minlength=L).astype(np.int64)
    c = np.zeros((L, d), dtype=np.float32)
    has = n > 0
    c[has] = (S[has].astype(np.float64) / n[has, None].astype(np.float64) * 2.0 ** (e - 36)).astype(np.float32)
    R = np.zeros(L, dtype=np.float64)
    for b in np.flatnonzero(has):
        delta = X[lab == b].astype(np.float64) - c[b].astype(np.float64)
        R[b] = np.sqrt((delta * delta).sum(axis=1).max())
    cn = np.sqrt((c.astype(np.float64) ** 2).sum(axis=1))
    return dict(n=n, c=c, R=R, cn=cn)


def admitted_ref(cover, Q, radius, metric, factor=1.0):
    """bool[nq, L]: the rule of lmi_hip.h with the margin scaled by `factor`; anything that is NaN admits (a non-empty bucket)."""
    Q64 = np.asarray(Q, dtype=np.float64)
    nq, d = Q64.shape
    r = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)).astype(np.float64)[:, None]
    c, R, cn, n = cover["c"].astype(np.float64), cover["R"][None, :], cover["cn"][None, :], cover["n"]
    qn = np.sqrt((Q64 * Q64).sum(axis=1))[:, None]
    u = factor * (d + 8) * 2.0 ** -23
    with np.errstate(all="ignore"):
        if metric == "ip":
            ub = Q64 @ c.T + qn * R
            m = u * (1.0 + np.abs(r) + qn * (cn + R))
            pruned = ub < 1.0 - r - m
        else:
            dc = np.sqrt(((Q64[:, None, :] - c[None, :, :]) ** 2).sum(axis=2))
            lo = np.maximum(0.0, dc - R)
            lo = np.where(np.isnan(lo), 0.0, lo)
            m = u * (qn + cn + R) ** 2
            pruned = lo * lo > r + m
    ok = ~np.isnan(r) & (r != -np.inf)
    return (n > 0)[None, :] & ok & ~pruned


def order_ref(adm, nb=None):
    """(order i32[nq, nb], counts i32[nq]): the admitted bucket ids ascending, then -1; nb = max(1, the largest count) unless given."""
    counts = adm.sum(axis=1).astype(np.int32)
    nb = max(1, int(counts.max()) if counts.size else 1) if nb is None else nb
    order = np.full((adm.shape[0], nb), -1, dtype=np.int32)
    for q in range(adm.shape[0]):
        ids = np.flatnonzero(adm[q])
        order[q, :len(ids)] = ids
    return order, counts


def dists_of(D, metric):
    return (ONE - D).astype(np.float32) if metric == "ip" else np.asarray(D, dtype=np.float32)


# ---- radii on union_ref.case(d): radius[q] = the j-th smallest distance over ALL objects, j = (0, 9, 99)[q mod 3] ----
RECIPE_J = (0, 9, 99)
_radii = {}


def union_radii(oracle, d, metric):
    """f32[NQ]: every radius sits on some object's computed distance, so dist == radius is exercised (computed once, read-only)."""
    key = (d, metric)
    if key not in _radii:
        X, Q, _, _ = ur.case(d)
        D, _ = (oracle.knn_ip if metric == "ip" else oracle.knn_l2)(Q, X, 100)
        j = np.asarray(RECIPE_J)[np.arange(ur.NQ) % 3]
        r = dists_of(D, metric)[np.arange(ur.NQ), j].copy()
        r.setflags(write=False)
        _radii[key] = r
    return _radii[key]


# ---- the clustered case: 8 well-separated buckets, among them an empty one, a one-row one and one of identical rows ----
CL = 8
CSIZES = (300, 0, 1, 40, 517, 64, 33, 129)
C_EMPTY, C_ONE, C_SAME = 1, 2, 3
CNQ = 64
_clustered = {}


def clustered_case(oracle, d, metric):
    """(X f32[N, d], Q f32[64, d], labels i64[N], ids u32[N], radius f32[64], home i64[64]) -- read-only.  Centres 3 N(0,1), rows =
    centre + 0.05 N(0,1), normalised for IP; the rows of the one-row bucket and of the bucket of identical rows lie on a 2^-16 grid, so
    that the integer mean is the row itself.  Query q lies near a stored row of bucket home[q] (a bucket of 5 rows or more) and
    radius[q] is the exact 5th smallest computed distance: its five nearest objects are in its own bucket."""
    key = (d, metric)
    if key not in _clustered:
        rs = np.random.RandomState(4000 + d)
        lab = np.repeat(np.arange(CL, dtype=np.int64), CSIZES)
        N = lab.shape[0]
        cen = 3.0 * rs.randn(CL, d)
        X = (cen[lab] + 0.05 * rs.randn(N, d)).astype(np.float32)
        X[lab == C_SAME] = X[np.flatnonzero(lab == C_SAME)[0]]
        if metric == "ip":
            X /= np.linalg.norm(X, axis=1, keepdims=True)
        grid = (lab == C_ONE) | (lab == C_SAME)
        X[grid] = (np.rint(X[grid].astype(np.float64) * 65536.0) / 65536.0).astype(np.float32)
        perm = rs.permutation(N)
        X, lab = np.ascontiguousarray(X[perm]), lab[perm]
        ids = (rs.permutation(N) + 500).astype(np.uint32)
        src = rs.choice(np.flatnonzero(np.isin(lab, [b for b in range(CL) if CSIZES[b] >= 5])), size=CNQ, replace=False)
        Q = (X[src] + (0.002 if metric == "ip" else 0.01) * rs.randn(CNQ, d)).astype(np.float32)
        if metric == "ip":
            Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        Q = np.ascontiguousarray(Q)
        D, _ = (oracle.knn_ip if metric == "ip" else oracle.knn_l2)(Q, X, 5)
        radius = dists_of(D, metric)[:, 4].copy()
        out = (X, Q, lab, ids, radius, lab[src].copy())
        for a in out:
            a.setflags(write=False)
        _clustered[key] = out
    return _clustered[key]
