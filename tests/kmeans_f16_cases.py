"""The `lmi_kmeans_f16` cases -- shared by test_build_f16_host.py and test_gpu_kmeans_f16.py, computed once per process, read-only.

A case is `kmeans_ref.make_case` narrowed once to float16: `x16` are the halves the call takes, `x` = `x16` widened again is what
the restatement (tests/kmeans_ref.py, unchanged) and `_capi.kmeans` run on, `c0` = the widened initial rows, niter = 8.  Widening is
exact, so the result on `x16` has to be the result on `x` bit for bit."""
import functools

import numpy as np

import kmeans_ref

NITER = kmeans_ref.NITER
#: (n, d, k, seed) -> (empty clusters at the end, pass of the fixed point or None, halves of x16 that are binary16 subnormals)
CASES = {
    (3001, 45, 7, 1): (0, None, 49),
    (2500, 770, 130, 2): (13, 3, 2585),
    (4099, 33, 33, 3): (0, None, 39),
    (600, 768, 257, 4): (1, 3, 640),
    (1500, 64, 20, 5): (1, None, 21),
    (1500, 64, 40, 6): (0, 7, 34),
    # d % 4 == 0 and d % 8 != 0: the float path reads 16 bytes at a time, the half path must not
    (1500, 44, 20, 7): (0, None, 22),
    # one 16-byte group of halves; the tail at link d opens the second group
    (700, 8, 5, 8): (0, None, 1),
}


def subnormals(x16):
    """nonzero halves with a zero exponent field"""
    b = x16.view(np.uint16)
    return int((((b & 0x7C00) == 0) & ((b & 0x03FF) != 0)).sum())


@functools.lru_cache(maxsize=None)
def _case(n, d, k, seed, niter):
    from oracle import lmi_oracle

    lmi_oracle.build()
    x32, c32 = kmeans_ref.make_case(n, d, k, seed)
    x16 = np.ascontiguousarray(x32.astype(np.float16))
    x = x16.astype(np.float32)
    c0 = c32.astype(np.float16).astype(np.float32)
    out = (x16, x, c0) + kmeans_ref.kmeans_ref(lmi_oracle, x, c0, niter)
    for a in out:
        a.setflags(write=False)
    return out


def case(n, d, k, seed, niter=NITER):
    """(x16, x, c0, centroids, labels, counts, changed) of a case"""
    return _case(n, d, k, seed, niter)
