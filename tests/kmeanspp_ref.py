"""`lmi_kmeans_seed` restated in numpy on top of the unchanged oracle -- shared by the tests of test_gpu_kmeanspp.py.

Definition (include/lmi_hip.h): the distance of a row to a centre (always a row of x) is `oracle.knn_l2`'s, clamped at 0; its weight
w = rint(dist * 2^(36-E)) in binary64, E = 2e + 3 + ceil(log2 d), e as in kmeans_ref; W_i is the least weight of row i so far.  Round
0 takes the row mulhi64(z(0,0), n); round t draws L candidates, candidate j the first row whose inclusive prefix sum of W exceeds
mulhi64(z(t,j), T) (T == 0: the row mulhi64(z(t,j), n)), and keeps the lowest potential sum_i min(W_i, w_ij), ties to the lowest j.
Integers are Python ints or uint64 (every sum is below 2^62)."""
import functools
import math

import numpy as np

import kmeans_ref

M64 = (1 << 64) - 1


def draw(seed, t, j):
    z = (seed + 0x9E3779B97F4A7C15 * (1 + 32 * t + j)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mulhi(z, bound):
    return (z * int(bound)) >> 64


def seed_ref(oracle, x, k, n_trials=0, seed=2023):
    """(centroids f32[k,d], rows i64[k], potential i64[k])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    E = 2 * kmeans_ref.exponent(x) + 3 + (d - 1).bit_length()
    L = n_trials or 2 + int(math.floor(math.log(k)))

    def weights(cands):   # u64 [n, len(cands)]
        D, I = oracle.knn_l2(x, x[cands], k=len(cands), nthreads=4)   # ascending per row: put back by candidate
        dist = np.empty_like(D)
        np.put_along_axis(dist, I, np.maximum(D, np.float32(0)), axis=1)
        return np.rint(dist.astype(np.float64) * 2.0 ** (36 - E)).astype(np.uint64)

    rows, pot = np.zeros(k, np.int64), np.zeros(k, np.int64)
    rows[0] = mulhi(draw(seed, 0, 0), n)
    W = weights(rows[:1])[:, 0]
    pot[0] = int(W.sum())
    for t in range(1, k):
        T, cum = int(W.sum()), np.cumsum(W)
        cands = [mulhi(draw(seed, t, j), n) if T == 0 else int(np.searchsorted(cum, np.uint64(mulhi(draw(seed, t, j), T)), side="right"))
                 for j in range(L)]
        M = np.minimum(W[:, None], weights(np.array(cands)))
        p = M.sum(axis=0)
        win = int(np.argmin(p))   # the first of the least
        rows[t], pot[t], W = cands[win], int(p[win]), M[:, win].copy()
    return x[rows].copy(), rows, pot


def data(n, d):
    """kmeans_ref's mixture (normalised rows, duplicates included)"""
    return kmeans_ref.make_case(n, d, 8, 1)[0]


@functools.lru_cache(maxsize=None)
def case(n, d, k, n_trials, seed=2023):
    """(x, centroids, rows, potential) of a case, computed once per process and read-only."""
    from oracle import lmi_oracle

    lmi_oracle.build()
    x = data(n, d)
    out = (x,) + seed_ref(lmi_oracle, x, k, n_trials, seed)
    for a in out:
        a.setflags(write=False)
    return out
