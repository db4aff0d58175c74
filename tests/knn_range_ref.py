"""The contract of lmi_knn_range (include/lmi_hip.h) restated on the unchanged oracle for bases too large for k = nb, and the radius
recipe its tests share (tests/test_gpu_knn_range.py on the device, tests/test_knn_range_host.py on the oracle alone).

Truth without k = nb: take oracle.knn_ip / knn_l2 at k = 1024 (`knn_cases.truth`, shared with the lmi_knn tests) and map IP
D -> 1 - D.  The distance is monotone along the oracle's (score descending, row ascending) order, so the rows within a radius are a
PREFIX of those 1024 entries whenever entry 1023 is itself not admitted; `prefix_ref` asserts that for every query and sorts the
prefix by row.  The oracle never returns a score that is not > -FLT_MAX (I = -1): such an entry is never admitted."""
import numpy as np

import knn_cases as kc
import range_ref as rr

K = 1024
RECIPE_J = (0, 9, 99, 700)   # radius[q] = the j-th distance of the truth, j = RECIPE_J[q mod 4]


def dists_of(D, metric):
    """The distances of oracle.knn_* results: IP 1 - D in binary32, L2 as they are."""
    return (rr.ONE - D).astype(np.float32) if metric == "ip" else np.asarray(D, dtype=np.float32)


def prefix_ref(D, I, radius, metric):
    """D, I [nq, k] of oracle.knn_ip / knn_l2 at some k; radius f32[nq] -> (lims i64[nq + 1], dists f32[total], rows u32[total]): every
    query's admitted rows in ascending row order.  Asserts that the admitted entries are a prefix of the k and that the last entry
    is not admitted -- the rows behind it then are not either."""
    nq, k = I.shape
    dd = dists_of(D, metric)
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,))
    runs_d, runs_i = [], []
    for q in range(nq):
        ok = (I[q] >= 0) & rr.admitted(dd[q], radius[q])
        n = int(ok.sum())
        assert not ok[k - 1], f"query {q}: entry {k - 1} is admitted, the truth at k = {k} may be cut short"
        assert np.all(ok[:n]), f"query {q}: the admitted entries are no prefix"
        by_row = np.argsort(I[q, :n], kind="stable")
        runs_d.append(dd[q, :n][by_row])
        runs_i.append(I[q, :n][by_row].astype(np.uint32))
    lims = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum([len(r) for r in runs_d], out=lims[1:])
    return lims, np.concatenate(runs_d).astype(np.float32), np.concatenate(runs_i).astype(np.uint32)


_recipe = {}


def recipe(oracle, shape, metric):
    """(radius f32[nq], (lims, dists, rows)) of knn_cases.case(*shape): the recipe's radii and `prefix_ref` of them, computed once per
    case and read-only."""
    key = (shape, metric)
    if key not in _recipe:
        xq, xb = kc.case(*shape)
        D, I = kc.truth(oracle, shape, xq, xb, K, metric)
        nq = xq.shape[0]
        j = np.asarray(RECIPE_J)[np.arange(nq) % len(RECIPE_J)]
        radius = dists_of(D, metric)[np.arange(nq), j].copy()
        ref = prefix_ref(D, I, radius, metric)
        for a in (radius,) + ref:
            a.setflags(write=False)
        _recipe[key] = (radius, ref)
    return _recipe[key]


def whole_base_ref(oracle, xq, xb, radius, metric):
    """`range_ref.range_ref` with the whole base as one bucket (ids = row numbers) and an order of zeros: k = nb on the oracle, for bases
    small enough for its insertion sort."""
    nb = xb.shape[0]
    return rr.range_ref(oracle, [np.ascontiguousarray(xb)], [np.arange(nb, dtype=np.uint32)], np.zeros((xq.shape[0], 1), dtype=np.int32),
                        np.ascontiguousarray(xq), radius, metric)


def with_empty_queries(xq, radius, ref):
    """Two more queries (copies of the first two) whose radii are NaN and -inf: their runs are empty."""
    lims, dd, ii = ref
    xq2 = np.ascontiguousarray(np.concatenate([xq, xq[:2]]))
    r2 = np.concatenate([radius, np.array([np.nan, -np.inf], dtype=np.float32)]).astype(np.float32)
    return xq2, r2, (np.concatenate([lims, lims[-1:], lims[-1:]]), dd, ii)
