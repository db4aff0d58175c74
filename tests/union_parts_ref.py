"""The union scan across ranks (include/lmi_hip.h, lmi_scan_union_part / lmi_merge_union_parts) restated in numpy on the unchanged
oracle, for tests/test_union_sharded_host.py and tests/test_gpu_union_sharded.py.

The part of a rank is union_ref's computation on the buckets the rank owns, extended to return the score, (rank, row) and the padding.
It is computed without one oracle call per (rank, query): `Candidates` scores every (query, bucket) once -- oracle.knn_ip with k = the
bucket's size returns every admissible row with its score (L2: the key of the augmented vectors, knn_l2's own recipe, and knn_l2 for
the distance) -- and sorts a query's candidates once in the total order (score descending with -0 == +0, rank, row).  The order
restricted to the owned buckets is the same order, so a part is the first k owned entries of that list.  `union_ref` on an order with
the other ranks' buckets struck out is the direct statement; test_union_sharded_host.py checks that the two agree.  The merge is
sharded.merge_union_parts_numpy: a lexsort on (part, row, rank, -score)."""
import numpy as np

import union_ref as ur

PLANES = 5
SCORE, DIST, ID, RANK, ROW = range(5)
PAD_SCORE = np.float32(-np.finfo(np.float32).max).view(np.int32)
PAD = np.asarray([PAD_SCORE, np.float32(np.inf).view(np.int32), 0, -1, -1], dtype=np.int32)   # per plane; -1 = 0xffffffff


def bucket_scores(oracle, rows, queries, metric):
    """(score f32[nq, n], dist f32[nq, n], ok bool[nq, n]) of every query against every row of one bucket, on the oracle."""
    nq, n = queries.shape[0], rows.shape[0]
    score = np.zeros((nq, n), np.float32)
    dist = np.zeros((nq, n), np.float32)
    ok = np.zeros((nq, n), bool)
    if n == 0:
        return score, dist, ok
    if metric == "ip":
        S, I = oracle.knn_ip(queries, rows, n)
        D = (ur.ONE - S).astype(np.float32)
    else:   # oracle.knn_l2's recipe for the key; knn_l2 itself for the distance
        xa = np.concatenate([rows, (np.float32(-0.5) * oracle.sqnorms(rows))[:, None]], axis=1)
        qa = np.concatenate([queries, np.ones((nq, 1), np.float32)], axis=1)
        S, I = oracle.knn_ip(qa, xa, n)
        D, I2 = oracle.knn_l2(queries, rows, n)
        assert np.array_equal(I, I2)
    q, j = np.nonzero(I >= 0)
    score[q, I[q, j]] = S[q, j]
    dist[q, I[q, j]] = D[q, j]
    ok[q, I[q, j]] = True
    return score, dist, ok


class Candidates:
    """Every query's candidates over `order`, sorted once in the total order; parts and the whole-index answer are cuts of it."""

    def __init__(self, oracle, bucket_rows, bucket_ids, order, queries, metric, per_bucket=None):
        """per_bucket: a dict the caller keeps for these (buckets, queries, metric), so that several orders share the scores."""
        order = np.asarray(order)
        self.nq, self.nb = order.shape
        self.order = order
        per_bucket = {} if per_bucket is None else per_bucket
        self.lists = []
        for q in range(self.nq):
            sc, di, idd, rk, rw, bk = [], [], [], [], [], []
            for t in range(self.nb):
                b = int(order[q, t])
                if not (0 <= b < len(bucket_rows)) or bucket_rows[b].shape[0] == 0:
                    continue
                if b not in per_bucket:
                    per_bucket[b] = bucket_scores(oracle, np.ascontiguousarray(bucket_rows[b], dtype=np.float32), queries, metric)
                s, d, ok = per_bucket[b]
                keep = np.flatnonzero(ok[q])
                sc.append(s[q, keep]), di.append(d[q, keep]), idd.append(np.asarray(bucket_ids[b], np.uint32)[keep])
                rk.append(np.full(keep.size, t, np.int64)), rw.append(keep.astype(np.int64)), bk.append(np.full(keep.size, b, np.int64))
            if not sc:
                self.lists.append(None)
                continue
            sc, di, idd, rk, rw, bk = (np.concatenate(a) for a in (sc, di, idd, rk, rw, bk))
            o = np.lexsort((rw, rk, -sc.astype(np.float64)))   # -0.0 and +0.0 compare equal
            self.lists.append((sc[o], di[o], idd[o], rk[o], rw[o], bk[o]))

    def part(self, owned, k):
        """(part i32[5, nq, k], counts i32[nq]) of a rank that owns the buckets with owned[b] != 0 (None: every bucket)."""
        part = np.empty((PLANES, self.nq, k), np.int32)
        part[:] = PAD[:, None, None]
        counts = np.zeros(self.nq, np.int32)
        for q, l in enumerate(self.lists):
            if l is None:
                continue
            sc, di, idd, rk, rw, bk = l
            sel = np.arange(min(k, sc.size)) if owned is None else np.flatnonzero(np.asarray(owned)[bk] != 0)[:k]
            n = sel.size
            counts[q] = n
            part[SCORE, q, :n] = sc[sel].view(np.int32)
            part[DIST, q, :n] = di[sel].view(np.int32)
            part[ID, q, :n] = idd[sel].view(np.int32)
            part[RANK, q, :n] = rk[sel]
            part[ROW, q, :n] = rw[sel]
        return part, counts

    def whole(self, k):
        """(dists, ids, counts) as union_ref returns them for the whole index."""
        part, counts = self.part(None, k)
        return part[DIST].view(np.float32), part[ID].view(np.uint32), counts


def struck_order(order, owned):
    """`order` with the buckets of other ranks replaced by -1: what a rank's scan sees of it (an unowned bucket has no rows)."""
    order = np.asarray(order)
    mine = (order >= 0) & (np.asarray(owned)[np.clip(order, 0, len(owned) - 1)] != 0)
    return np.where(mine, order, -1).astype(np.int32)


def owners(world, kind="assign"):
    """owner i32[L] of union_ref's buckets: `assign_buckets` on their sizes, or ("gap") the same over world - 1 ranks with rank 1
    skipped, so that rank 1 owns nothing."""
    from learnedmetricindex_amd.sharded import assign_buckets

    if kind == "assign":
        return assign_buckets(ur.SIZES, world)
    assert kind == "gap" and world >= 3
    o = assign_buckets(ur.SIZES, world - 1)
    return np.where(o >= 1, o + 1, o).astype(np.int32)


def collapse_case(d=64):
    """The distance-collapse case (IP): (bucket rows, bucket ids, order i32[1, 2], query f32[1, d], owner i32[2]).  The query is e0.
    Bucket 0, first in the order, holds a row with x0 = 2^-31; bucket 1, second, one with x0 = 2^-30; every other row has x0 = -1.
    Both scores give the distance 1.0f: 1 - 2^-30 and 1 - 2^-31 round to 1.  By score the row of bucket 1 comes first; by
    (distance, rank, row) the row of bucket 0 would.  The buckets are on different ranks."""
    rs = np.random.RandomState(11)
    rows = []
    for b, x0 in ((0, 2.0 ** -31), (1, 2.0 ** -30)):
        x = (rs.randn(5, d) * 0.1).astype(np.float32)
        x[:, 0] = -1.0
        x[2 + b, 0] = x0
        rows.append(x)
    ids = [np.arange(100, 105, dtype=np.uint32), np.arange(200, 205, dtype=np.uint32)]
    q = np.zeros((1, d), np.float32)
    q[0, 0] = 1.0
    return rows, ids, np.asarray([[0, 1]], np.int32), q, np.asarray([0, 1], np.int32)
