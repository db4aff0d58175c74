"""The filtered union scan's contract (include/lmi_hip.h, lmi_scan_union_filtered) restated in numpy on the unchanged oracle, and the
filter set the filter tests share.

Per query: `union_ref` (tests/union_ref.py) against its buckets with the rows its filter disallows REMOVED.  `union_filter_forced` is
the second statement -- the disallowed rows stay where they are, so ordinals are the unfiltered concatenation's, and their scores are
forced to never-selected (a NaN row: the selection takes scores > -FLT_MAX only) -- which is how the device does it;
tests/test_union_filter_host.py checks on the oracle alone that the two agree."""
import numpy as np

import union_ref as ur

KEEP, DROP = 0, 1


def allowed_rows(lists, modes, bucket_ids):
    """allowed[j][b]: bool[n_b], whether filter j allows each row of bucket b (an id listed twice or absent from the index changes
    nothing; rows that share an id all follow it)."""
    out = []
    for ids, mode in zip(lists, modes):
        ids = np.asarray(ids, dtype=np.uint32).reshape(-1)
        out.append([np.isin(np.asarray(b, dtype=np.uint32), ids) != (mode == DROP) for b in bucket_ids])
    return out


def union_filter_ref(oracle, bucket_rows, bucket_ids, order, queries, k, metric, allowed, filter_of):
    """`union_ref` per group of (order row, filter) on the buckets with their disallowed rows removed.  allowed[j][b] bool[n_b];
    filter_of i32[nq] in [-1, len(allowed)), -1 = unfiltered, None = every query uses filter 0."""
    order = np.asarray(order)
    nq = order.shape[0]
    fo = np.zeros(nq, dtype=np.int32) if filter_of is None else np.asarray(filter_of, dtype=np.int32)
    assert fo.shape == (nq,) and fo.min(initial=0) >= -1 and fo.max(initial=-1) < len(allowed)
    dists = np.full((nq, k), np.inf, dtype=np.float32)
    ids = np.zeros((nq, k), dtype=np.uint32)
    counts = np.zeros(nq, dtype=np.int32)
    for j in np.unique(fo):
        qs = np.flatnonzero(fo == j)
        if j < 0:
            rows, labs = bucket_rows, bucket_ids
        else:
            rows = [np.ascontiguousarray(r[a]) for r, a in zip(bucket_rows, allowed[j])]
            labs = [np.asarray(i)[a] for i, a in zip(bucket_ids, allowed[j])]
        dists[qs], ids[qs], counts[qs] = ur.union_ref(oracle, rows, labs, order[qs], np.ascontiguousarray(queries[qs]), k, metric)
    return dists, ids, counts


def union_filter_forced(oracle, bucket_rows, bucket_ids, order, queries, k, metric, allowed, filter_of):
    """The same result by the other statement: every disallowed row becomes a row of NaN, whose score the selection never takes; the
    candidates keep their unfiltered ordinals."""
    order = np.asarray(order)
    nq = order.shape[0]
    fo = np.zeros(nq, dtype=np.int32) if filter_of is None else np.asarray(filter_of, dtype=np.int32)
    dists = np.full((nq, k), np.inf, dtype=np.float32)
    ids = np.zeros((nq, k), dtype=np.uint32)
    counts = np.zeros(nq, dtype=np.int32)
    for j in np.unique(fo):
        qs = np.flatnonzero(fo == j)
        rows = bucket_rows
        if j >= 0:
            rows = []
            for r, a in zip(bucket_rows, allowed[j]):
                r = np.array(r, dtype=np.float32)
                r[~a] = np.nan
                rows.append(r)
        dists[qs], ids[qs], counts[qs] = ur.union_ref(oracle, rows, bucket_ids, order[qs], np.ascontiguousarray(queries[qs]), k, metric)
    return dists, ids, counts


# ---- the shared filter set over union_ref.case(d) (the ids are a permutation drawn per d: so are the lists) ----
NF = 5
MODES = (KEEP, KEEP, DROP, KEEP, KEEP)
ABSENT_ID = 7   # case()'s ids start at 1000


def filter_lists(d=64):
    """The five lists for union_ref.case(d).  F0 keep the even ids; F1 keep 60 random ids; F2 drop three ids, one of them absent from
    the index; F3 keep nothing; F4 keep exactly the ids of bucket 4.  Unsorted and with a duplicate here and there: the library
    normalises."""
    ids, lab = ur.case(d)[3], ur.labels()
    rs = np.random.RandomState(11)
    f0 = ids[ids % 2 == 0]
    f0 = np.concatenate([f0[::-1], f0[:5]])                   # descending, five ids twice
    f1 = rs.choice(ids, size=60, replace=False)
    f2 = np.asarray([ids[lab == 4][17], ABSENT_ID, ids[lab == 10][0]], dtype=np.uint32)
    f3 = np.zeros(0, dtype=np.uint32)
    f4 = rs.permutation(ids[lab == 4])
    return [np.asarray(f, dtype=np.uint32) for f in (f0, f1, f2, f3, f4)]


def filter_of():
    """i32[NQ]: cycles through -1, 0, 1, 2, 3, 4."""
    return (np.arange(ur.NQ) % (NF + 1) - 1).astype(np.int32)


_allowed = {}


def case_allowed(d=64):
    """allowed[j][b] of the shared filter set on union_ref.case(d)'s buckets (computed once per d)."""
    if d not in _allowed:
        X, Q, lab, ids = ur.case(d)
        _allowed[d] = allowed_rows(filter_lists(d), MODES, ur.buckets_of(X, lab, ids)[1])
    return _allowed[d]


def tie_filter(ids_by_rank_row):
    """A keep list for union_ref.tie_case that removes every third of the 40 copies (given by (rank, row)) and keeps everything else:
    returned as (drop list, survivors in (rank, row) order)."""
    tied = np.asarray(ids_by_rank_row, dtype=np.uint32)
    gone = tied[1::3]
    return gone, tied[~np.isin(tied, gone)]
