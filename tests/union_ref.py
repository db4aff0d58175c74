"""The union scan's contract (include/lmi_hip.h, lmi_scan_union) restated in numpy on the unchanged oracle, and the inputs the union
tests share.

Per query: oracle.knn_ip / oracle.knn_l2 against the concatenation of the rows of its buckets in rank order (a rank of -1 or of no
bucket id contributes nothing, a bucket listed twice contributes twice); IP maps D -> 1 - D; I (the ordinal) maps to the id stored at
that ordinal; -1 becomes padding (dist = +inf, id = 0) and counts the real results."""
import numpy as np

ONE = np.float32(1.0)


def union_ref(oracle, bucket_rows, bucket_ids, order, queries, k, metric):
    """bucket_rows[b] f32[n_b, d], bucket_ids[b] u32[n_b]; order i32[nq, nb]; queries f32[nq, d] -> (dists f32[nq, k], ids u32[nq, k],
    counts i32[nq])."""
    order = np.asarray(order)
    nq, nb = order.shape
    d = queries.shape[1]
    dists = np.full((nq, k), np.inf, dtype=np.float32)
    ids = np.zeros((nq, k), dtype=np.uint32)
    counts = np.zeros(nq, dtype=np.int32)
    knn = oracle.knn_ip if metric == "ip" else oracle.knn_l2
    groups = {}
    for q in range(nq):
        groups.setdefault(tuple(int(b) for b in order[q]), []).append(q)
    for key, qs in groups.items():   # queries with one order share one oracle call
        ranks = [b for b in key if 0 <= b < len(bucket_rows) and bucket_rows[b].shape[0] > 0]
        if not ranks:
            continue
        rows = np.ascontiguousarray(np.concatenate([bucket_rows[b] for b in ranks]).reshape(-1, d), dtype=np.float32)
        lab = np.concatenate([np.asarray(bucket_ids[b], dtype=np.uint32) for b in ranks])
        D, I = knn(np.ascontiguousarray(queries[qs]), rows, k)
        real = I >= 0
        dd = (ONE - D).astype(np.float32) if metric == "ip" else D.astype(np.float32)
        dists[qs] = np.where(real, dd, np.float32(np.inf))
        ids[qs] = np.where(real, lab[np.where(real, I, 0)], 0).astype(np.uint32)
        counts[qs] = real.sum(axis=1)
    return dists, ids, counts


# ---- the shared inputs: N = 6000 objects in L = 12 buckets whose sizes include 0, 1, 33, 257 and one of about 2000; nq = 150 ----
L = 12
SIZES = (0, 1, 33, 257, 2003, 640, 0, 5, 64, 65, 1729, 1203)
N = sum(SIZES)
NQ = 150
DIMS = (45, 64, 136)
NBS = (1, 3, 8)
KS = (1, 10, 100, 129, 1024)
METRICS = ("ip", "l2")
TIE_BUCKETS = (5, 3, 11)     # the ties case visits these, in this order
TIE_COPIES = (13, 20, 7)     # copies of the tie vector in each: 40 in all
assert N == 6000 and len(SIZES) == L and sum(TIE_COPIES) == 40

_cache = {}


def labels():
    """i64[N]: the bucket of every object, shuffled with a fixed seed."""
    lab = np.repeat(np.arange(L, dtype=np.int64), SIZES)
    np.random.RandomState(7).shuffle(lab)
    return lab


def case(d):
    """(X f32[N, d], Q f32[NQ, d], labels, ids u32[N]) -- read-only.  Unit-norm rows; ids are a permutation, not the row numbers."""
    if d not in _cache:
        rs = np.random.RandomState(100 + d)
        X = rs.randn(N, d).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        Q = rs.randn(NQ, d).astype(np.float32)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        ids = (rs.permutation(N) + 1000).astype(np.uint32)
        out = (X, Q, labels(), ids)
        for a in out:
            a.setflags(write=False)
        _cache[d] = out
    return _cache[d]


def buckets_of(X, lab, ids, n_buckets=L):
    """(rows per bucket, ids per bucket) in the order lmi_bucket_read returns them: ascending object number inside a bucket."""
    rows, labs = [], []
    for b in range(n_buckets):
        sel = np.flatnonzero(lab == b)
        rows.append(np.ascontiguousarray(X[sel]))
        labs.append(np.asarray(ids)[sel].astype(np.uint32))
    return rows, labs


def random_order(nb, seed=0, holes=True):
    """i32[NQ, nb]: distinct buckets per query, drawn with probability ~ size + 10 (as a model sends queries: mostly to the large
    buckets, now and then to the small and the empty ones); behind rank 0 about one slot in six is -1, queries 0..3 visit nothing
    and query 4 surely sees the large bucket first."""
    rs = np.random.RandomState(1000 + 17 * nb + seed)
    w = np.asarray(SIZES, dtype=np.float64) + 10.0
    order = np.stack([rs.choice(L, size=nb, replace=False, p=w / w.sum()) for _ in range(NQ)]).astype(np.int32)
    if holes:
        order[:, 1:][rs.rand(NQ, nb - 1) < 1.0 / 6.0] = -1
        order[:4, :] = -1
        order[4, 0] = 4
    return order


def tie_case(d):
    """(X, Q, labels, ids, order): `case(d)` with 40 copies of one vector spread over TIE_BUCKETS and queries 0..3 equal to it."""
    X, Q, lab, ids = (np.array(a) for a in case(d))
    rs = np.random.RandomState(5)
    src = np.flatnonzero(lab == TIE_BUCKETS[0])[0]
    v = X[src].copy()
    for b, n in zip(TIE_BUCKETS, TIE_COPIES):
        sel = np.flatnonzero(lab == b)
        sel = sel[sel != src]   # the vector's own row is one of the first bucket's copies
        X[rs.choice(sel, size=n - (b == TIE_BUCKETS[0]), replace=False)] = v
    Q[:4] = v
    order = np.tile(np.asarray(TIE_BUCKETS, dtype=np.int32), (NQ, 1))
    return X, Q, lab, ids, order


def nan_case(d):
    """(X, Q, labels, ids, row): `case(d)` with a NaN in one row of the 257-row bucket."""
    X, Q, lab, ids = (np.array(a) for a in case(d))
    row = int(np.flatnonzero(lab == 3)[100])
    X[row, d // 2] = np.nan
    return X, Q, lab, ids, row


def layers_for(d_in, n_classes, seed):
    """A random two-layer model as (W [out, in], b [out]) pairs."""
    rs = np.random.RandomState(seed)
    return [(rs.randn(16, d_in).astype(np.float32) * 0.5, rs.randn(16).astype(np.float32) * 0.1),
            (rs.randn(n_classes, 16).astype(np.float32), rs.randn(n_classes).astype(np.float32) * 0.1)]
