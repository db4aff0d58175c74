"""The row-budget stop (`lmi_set_stop_rows`) restated in numpy on top of the unchanged oracle -- shared by
test_stop_rows_host.py and test_gpu_stop_rows.py.

Definition (include/lmi_hip.h): n(b) = the objects the index holds in bucket b.  In a query's bucket order r_0 = n(b_0),
r_t = r_{t-1} + n(b_t) in int64; a rank without a class (-1) and a listed bucket without objects add 0.  Rank 0 is always
visited, rank t >= 1 iff r_{t-1} < rows; a rank that is not visited is -1 in the order.  The same rule cuts the 1-level order
(`oracle.precompute_bucket_order`) and the multi-level walk's (`oracle.precompute_bucket_order_multilevel`, which is
`path_mass_ref.walk(tree, nb, 0)`).  With a probability mass as well (`stop_mass_ref` / `path_mass_ref`) a query goes on only
while both stops allow it: both are prefix cuts of one order, so it visits the smaller of the two counts."""
import numpy as np

from stop_mass_ref import assert_not_vacuous, count_histogram  # noqa: F401  (re-exported for the tests)

EMPTY_VALUE = -1


def visited_mask(slot_sizes, rows):
    """bool[nq, nb]: which ranks a query visits, from the sizes int[nq, nb] of the buckets at its ranks (0 where a rank adds
    nothing)."""
    n = np.asarray(slot_sizes, dtype=np.int64)
    assert (n >= 0).all()
    r = np.cumsum(n, axis=1, dtype=np.int64)
    keep = np.ones(n.shape, dtype=bool)
    keep[:, 1:] = r[:, :-1] < np.int64(rows)
    return keep


def sizes_of_classes(classes, sizes):
    """int64[nq, nb]: n(class) per rank of a 1-level order int[nq, nb]; a class of -1 adds 0."""
    classes = np.asarray(classes)
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.where(classes >= 0, sizes[np.clip(classes, 0, None)], 0)


def sizes_of_paths(order, data_prediction):
    """int64[nq, nb]: the objects placed on each path of a multi-level order int[nq, nb, n_levels]; a listed bucket without
    objects and an empty slot (EMPTY_VALUE in the first level) add 0."""
    paths, cnt = np.unique(np.asarray(data_prediction, dtype=np.int64), axis=0, return_counts=True)
    held = {tuple(int(v) for v in p): int(c) for p, c in zip(paths, cnt)}
    out = np.zeros(order.shape[:2], dtype=np.int64)
    for q in range(order.shape[0]):
        for j in range(order.shape[1]):
            out[q, j] = held.get(tuple(int(v) for v in order[q, j]), 0)
    return out


def cut(order, counts):
    """A copy of order int[nq, nb, n_levels] with every slot from a query's visited count on set to EMPTY_VALUE."""
    out = np.array(order, copy=True)
    behind = np.arange(order.shape[1])[None, :] >= np.asarray(counts)[:, None]
    out[behind] = EMPTY_VALUE
    return out


def expected_order(oracle, layers, Q, nb, sizes, rows, mass=0.0, nthreads=4):
    """1-level: (bucket_order int32[nq, nb, 1] with the cut ranks at -1, visited counts int[nq]); mass > 0: both stops."""
    full = oracle.precompute_bucket_order(layers, Q, nb, nthreads)
    counts = visited_mask(sizes_of_classes(full[:, :, 0], sizes), rows).sum(axis=1)
    if mass:
        import stop_mass_ref

        counts = np.minimum(counts, stop_mass_ref.expected_order(oracle, layers, Q, nb, mass, nthreads)[1])
    return cut(full, counts), counts


def expected_walk(full, data_prediction, rows, mass_counts=None):
    """Multi-level: the uncut walk's order int32[nq, nb, n_levels] (the oracle's, or path_mass_ref.walk at mass 0) cut by the row
    budget -> (order, visited counts).  `mass_counts`: the visited counts of path_mass_ref.walk at a mass, for both stops.
    The counts count recorded buckets (those without objects included)."""
    recorded = full[:, :, 0] != EMPTY_VALUE
    assert (np.diff(recorded.astype(int), axis=1) <= 0).all()   # an exhausted queue leaves a suffix empty
    keep = visited_mask(sizes_of_paths(full, data_prediction), rows) & recorded
    counts = keep.sum(axis=1)
    if mass_counts is not None:
        counts = np.minimum(counts, mass_counts)
    return cut(full, counts), counts
