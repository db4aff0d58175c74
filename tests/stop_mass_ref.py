"""The probability-mass stop (`lmi_set_stop_mass`) restated in numpy on top of the unchanged oracle -- shared by
test_stop_mass_host.py and test_gpu_stop_mass.py.

Definition (include/lmi_hip.h): p_t = predict_proba's probability at rank t; c_0 = p_0, c_t = c_{t-1} + p_t in binary32, one
rounding per add, in rank order; rank 0 is always visited, rank t >= 1 iff c_{t-1} < mass (a binary32 compare: false on NaN);
a rank that is not visited is -1 in the bucket order."""
import numpy as np


def visited_mask(probs, nb, mass):
    """bool[nq, nb]: which ranks a query visits, from predict_proba's descending probabilities."""
    p = np.ascontiguousarray(probs[:, :nb], dtype=np.float32)
    m = np.float32(mass)
    keep = np.ones(p.shape, dtype=bool)
    c = p[:, 0].copy()
    for t in range(1, nb):
        keep[:, t] = c < m
        c = c + p[:, t]          # float32 + float32: one rounding
        assert c.dtype == np.float32
    return keep


def expected_order(oracle, layers, Q, nb, mass, nthreads=4):
    """(bucket_order int32[nq, nb, 1] with the cut ranks at -1, visited counts int[nq])."""
    probs, _ = oracle.predict_proba(layers, Q, nthreads)
    bo = oracle.precompute_bucket_order(layers, Q, nb, nthreads)
    keep = visited_mask(probs, nb, mass)
    bo[~keep] = -1
    return bo, keep.sum(axis=1)


def count_histogram(counts, nb):
    """[queries that visit exactly 1, 2, .., nb ranks]"""
    return np.bincount(counts, minlength=nb + 1)[1:].tolist()


def assert_not_vacuous(counts, nb):
    """The non-vacuity condition of a parity case: at least three distinct visited counts, at least 10 % of the queries cut
    (they visit fewer than nb ranks) and at least 10 % not cut."""
    counts = np.asarray(counts)
    full = counts == nb
    assert np.unique(counts).size >= 3, np.unique(counts)
    assert (~full).mean() >= 0.10 and full.mean() >= 0.10, full.mean()
