"""The range search across ranks (include/lmi_hip.h, lmi_join_range_parts) restated on the unchanged oracle, for
tests/test_range_sharded_host.py and tests/test_gpu_range_sharded.py.

A rank of a bucket-sharded index holds no rows of the buckets it does not own, so its scan sees `order` with those buckets struck out
(`union_parts_ref.struck_order`).  Its PART is `range_ref` on that order; its per-(query, t) counts are the lengths `range_ref` returns
on the struck order's single columns -- one bucket per query, so a query's length is the run's.  The join is
`sharded.join_range_parts_numpy`."""
import numpy as np

import range_ref as rr
import union_parts_ref as upr


def pair_counts(oracle, bucket_rows, bucket_ids, order, queries, radius, metric, owned=None, allowed=None, filter_of=None):
    """i32[nq, nb]: the results of every (query, t) of a rank that owns the buckets with owned[b] != 0 (None: every bucket)."""
    order = np.asarray(order)
    seen = order if owned is None else upr.struck_order(order, owned)
    counts = np.zeros(order.shape, np.int32)
    for t in range(order.shape[1]):
        lims = rr.range_ref(oracle, bucket_rows, bucket_ids, seen[:, t:t + 1], queries, radius, metric, allowed, filter_of)[0]
        counts[:, t] = np.diff(lims)
    return counts


def part(oracle, bucket_rows, bucket_ids, order, queries, radius, metric, owned, allowed=None, filter_of=None):
    """(counts i32[nq, nb], lims, dists, ids) of the rank that owns the buckets with owned[b] != 0."""
    seen = upr.struck_order(order, owned)
    lims, d, i = rr.range_ref(oracle, bucket_rows, bucket_ids, seen, queries, radius, metric, allowed, filter_of)
    counts = pair_counts(oracle, bucket_rows, bucket_ids, order, queries, radius, metric, owned, allowed, filter_of)
    assert np.array_equal(counts.sum(axis=1), np.diff(lims))
    return counts, lims, d, i


def parts(oracle, bucket_rows, bucket_ids, order, queries, radius, metric, owner, world):
    """(counts i32[world, nq, nb], [dists per rank], [ids per rank]) for owner i32[L]."""
    got = [part(oracle, bucket_rows, bucket_ids, order, queries, radius, metric, owner == r) for r in range(world)]
    return np.stack([g[0] for g in got]), [g[2] for g in got], [g[3] for g in got]


def feeders(counts):
    """i[nq]: how many ranks feed each query (have a result for it)."""
    return (np.asarray(counts).sum(axis=2) > 0).sum(axis=0)
