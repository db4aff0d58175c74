"""The range search's contract (include/lmi_hip.h, lmi_scan_range) restated in numpy on the unchanged oracle, and the radius recipe
the range tests share.

Per query: oracle.knn_ip / oracle.knn_l2 with k = every candidate, against the concatenation of the rows of its buckets in rank order
(`union_ref`'s candidates: a rank of -1 or of no bucket id contributes nothing, a bucket listed twice contributes twice).  The oracle
never returns a score that is not > -FLT_MAX (I = -1), IP maps D -> 1 - D, and a result is ADMITTED iff dist <= radius[q] in
binary32 (a NaN or -inf radius admits nothing).  The admitted come back in ascending ORDINAL order, with the id stored at the ordinal.
With a filter the disallowed rows become rows of NaN -- never admitted -- so the ordinals stay the unfiltered ones
(`union_filter_ref.union_filter_forced`'s statement)."""
import numpy as np

import union_ref as ur

ONE = np.float32(1.0)


def admitted(dist, radius):
    """bool: dist <= radius in binary32; a NaN or -inf radius admits nothing."""
    r = np.float32(radius)
    if np.isnan(r) or r == -np.inf:
        return np.zeros(np.shape(dist), dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(dist, dtype=np.float32) <= r


def range_ref(oracle, bucket_rows, bucket_ids, order, queries, radius, metric, allowed=None, filter_of=None):
    """bucket_rows[b] f32[n_b, d], bucket_ids[b] u32[n_b]; order i32[nq, nb]; queries f32[nq, d]; radius a scalar or f32[nq];
    allowed[j][b] bool[n_b] and filter_of i32[nq] (-1: unfiltered; None with `allowed`: every query uses filter 0)
    -> (lims i64[nq + 1], dists f32[total], ids u32[total])."""
    order = np.asarray(order)
    nq, nb = order.shape
    d = queries.shape[1]
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,))
    if allowed is None:
        fo = np.full(nq, -1, dtype=np.int32)
    else:
        fo = np.zeros(nq, dtype=np.int32) if filter_of is None else np.asarray(filter_of, dtype=np.int32)
    knn = oracle.knn_ip if metric == "ip" else oracle.knn_l2
    runs_d = [np.zeros(0, np.float32)] * nq
    runs_i = [np.zeros(0, np.uint32)] * nq
    groups = {}
    for q in range(nq):
        groups.setdefault((tuple(int(b) for b in order[q]), int(fo[q])), []).append(q)
    for (key, j), qs in groups.items():   # queries with one order and one filter share one oracle call
        ranks = [b for b in key if 0 <= b < len(bucket_rows) and bucket_rows[b].shape[0] > 0]
        if not ranks:
            continue
        parts = []
        for b in ranks:
            r = np.array(bucket_rows[b], dtype=np.float32)
            if j >= 0:
                r[~allowed[j][b]] = np.nan
            parts.append(r)
        rows = np.ascontiguousarray(np.concatenate(parts).reshape(-1, d))
        lab = np.concatenate([np.asarray(bucket_ids[b], dtype=np.uint32) for b in ranks])
        D, I = knn(np.ascontiguousarray(queries[qs]), rows, rows.shape[0])
        dd = (ONE - D).astype(np.float32) if metric == "ip" else D.astype(np.float32)
        for i, q in enumerate(qs):
            ok = (I[i] >= 0) & admitted(dd[i], radius[q])
            o = I[i][ok]
            by_ordinal = np.argsort(o, kind="stable")
            runs_d[q] = dd[i][ok][by_ordinal]
            runs_i[q] = lab[o[by_ordinal]]
    lims = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum([len(r) for r in runs_d], out=lims[1:])
    return lims, np.concatenate(runs_d).astype(np.float32), np.concatenate(runs_i).astype(np.uint32)


# ---- the radius recipe: radius[q] = the j-th distance of union_ref(k = 100), j = (0, 9, 99)[q mod 3]; +inf where the query has fewer ----
RECIPE_J = (0, 9, 99)
_recipe = {}


def recipe_radii(oracle, d, nb, metric):
    """(radius f32[NQ], order i32[NQ, nb]) on union_ref.case(d) with union_ref.random_order(nb) (computed once per case)."""
    key = (d, nb, metric)
    if key not in _recipe:
        X, Q, lab, ids = ur.case(d)
        rows, labs = ur.buckets_of(X, lab, ids)
        order = ur.random_order(nb)
        dd, _, cc = ur.union_ref(oracle, rows, labs, order, Q, 100, metric)
        j = np.asarray(RECIPE_J)[np.arange(ur.NQ) % 3]
        radius = np.where(cc > j, dd[np.arange(ur.NQ), j], np.float32(np.inf)).astype(np.float32)
        radius.setflags(write=False)
        order.setflags(write=False)
        _recipe[key] = (radius, order)
    return _recipe[key]


_ref_cache = {}


def recipe_ref(oracle, d, nb, metric):
    """`range_ref` of the recipe's case (computed once per case and shared; read-only)."""
    key = (d, nb, metric)
    if key not in _ref_cache:
        X, Q, lab, ids = ur.case(d)
        rows, labs = ur.buckets_of(X, lab, ids)
        radius, order = recipe_radii(oracle, d, nb, metric)
        out = range_ref(oracle, rows, labs, order, Q, radius, metric)
        for a in out:
            a.setflags(write=False)
        _ref_cache[key] = out
    return _ref_cache[key]


def stable_by_distance(lims, dists, ids):
    """Every query's run stably sorted by distance (what `li.range_search(sort=True)` returns)."""
    d2, i2 = np.array(dists), np.array(ids)
    for q in range(len(lims) - 1):
        a, b = int(lims[q]), int(lims[q + 1])
        o = np.argsort(d2[a:b], kind="stable")
        d2[a:b], i2[a:b] = d2[a:b][o], i2[a:b][o]
    return d2, i2
