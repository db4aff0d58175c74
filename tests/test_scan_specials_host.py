"""CPU: the case table of the scan's special-value tests (scan_special_cases.py) against the oracle alone.  What makes the GPU
comparison decidable is checked here: the oracle's answer does not depend on its thread count, its distances hold no NaN (no order of
NaNs is defined), every case contains what its name says, and a special value in one query changes no other query's answer."""
import numpy as np
import pytest

import scan_special_cases as sc

FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.finfo(np.float32).tiny)   # the smallest normal binary32


@pytest.mark.parametrize("name,d,metric", sc.CASES, ids=[f"{n}-d{d}-{m}" for n, d, m in sc.CASES])
def test_case_is_decidable_and_holds_what_it_names(oracle, name, d, metric):
    c = sc.case(name, d, metric)
    do, io = sc.truth(oracle, name, d, metric)
    d1, i1 = sc.search(oracle, c.X, c.Q, c.labels, c.order, metric, nthreads=1)
    np.testing.assert_array_equal(io, i1)
    np.testing.assert_array_equal(do, d1)
    assert do.shape == io.shape == (sc.NQ, sc.K)
    assert not np.isnan(do).any()
    # the ordinary queries of the batch answer as they do without the special ones
    assert (name in sc.QUERY) == (c.special_queries.size > 0) and (name in sc.STORED) == (c.special_rows.size > 0)
    plain = np.setdiff1d(np.arange(sc.NQ), c.special_queries)
    np.testing.assert_array_equal(c.Q[plain], c.plain_Q[plain])
    dp, ip = sc.search(oracle, c.X, c.plain_Q, c.labels, c.order, metric)
    np.testing.assert_array_equal(io[plain], ip[plain])
    np.testing.assert_array_equal(do[plain], dp[plain])
    assert np.isfinite(dp).all() or name in sc.STORED
    # what the name says
    hit = np.isin(io.astype(np.int64) - 1, c.special_rows)
    padded = do == FLT_MAX
    sq, X, Q = c.special_queries, c.X, c.Q
    if name in ("nan_rows", "nan_bucket", "nan_crowd"):
        assert (np.isnan(X).sum(1)[c.special_rows] == 1).all() and np.isnan(X).sum() == c.special_rows.size
        assert not hit.any() and not padded.any()
    if name == "nan_rows":
        assert c.special_rows.size == 200
    if name == "nan_bucket":
        assert (c.order == 1).any() and np.array_equal(c.special_rows, np.flatnonzero(c.labels == 1))
    if name == "nan_crowd":
        assert c.special_rows.size == sum(range(1, 10))
        X0 = sc.base(d)[0]
        for q in range(9):   # the query's q + 1 nearest rows have NaN twins in its first bucket, and are themselves returned
            twins = [r for r in c.special_rows if c.labels[r] == c.order[q, 0]
                     and any(np.array_equal(X[r][~np.isnan(X[r])], X0[s][~np.isnan(X[r])]) for s in io[q, :q + 1].astype(np.int64) - 1)]
            assert len(twins) >= q + 1
    if name == "inf_rows":
        assert np.isinf(X).sum() == 200 and (np.isinf(X).sum(1)[c.special_rows] == 1).all()
        zeros = (Q[:, None, :] == 0) & np.isinf(X[c.special_rows])[None, :, :]
        assert zeros.any(), "no pair scores 0 * inf"
        assert ((do == -np.inf).sum() > 0 and hit.any()) if metric == "ip" else not hit.any()
    if name == "inf_and_large":
        assert np.isposinf(X).sum() == 1 and np.isinf(X).sum() == 1
        big = np.abs(np.where(np.isfinite(X), X, 0))
        assert big.max() < 1e6 and ((big >= 1e5).sum(1) == 3).sum() == c.special_rows.size - 1   # beyond binary16's 65504
        assert ((do == -np.inf).sum() > 0 and hit.any()) if metric == "ip" else not hit.any()
    if name == "huge_rows":
        assert np.isfinite(X).all() and np.abs(X[c.special_rows]).max() > 1e30
        assert hit.all() if metric == "ip" else not hit.any()   # inner products of 1e30; squared norms that overflow
    if name == "nan_q":
        assert (np.isnan(Q).sum(1)[sq] == 1).all() and np.isnan(Q).sum() == sq.size
        assert padded[sq].all() and not padded[plain].any()
    if name == "inf_q":
        assert (np.isinf(Q).sum(1)[sq] == 1).all() and np.isinf(Q).sum() == sq.size
        assert (do[sq] == -np.inf).all() and np.isfinite(do[plain]).all()
    if name in ("tiny_q", "subnormal_q"):
        a = np.abs(Q[sq])
        assert (a < TINY).all() and (a > 0).mean() > 0.9 and np.abs(Q[plain]).max() > 1
        assert np.isfinite(do).all()
        if metric == "ip":   # scores far below 1's ulp: ten real neighbours at distance exactly 1, ordered by subnormal scores
            assert (do[sq] == 1.0).all() and (np.sort(io[sq], axis=1)[:, 1:] != np.sort(io[sq], axis=1)[:, :-1]).all()
    if name == "huge_q":
        assert np.isfinite(Q).all() and np.abs(Q[sq]).max() > 1e30
        assert (do[sq] == np.inf).all() if metric == "l2" else (np.isfinite(do[sq]).all() and np.abs(do[sq]).min() > 1e28)
    if name == "zero_q":
        assert not Q[sq].any() and sq.size > 0
        if metric == "ip":
            assert (do[sq] == 1.0).all()
