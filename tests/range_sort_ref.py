"""The contract of lmi_range_result_sort (include/lmi_hip.h) restated in numpy.

For every query q with segment [a, b) = [lims[q], lims[q + 1]): dists[a:b] and ids[a:b] are permuted together so that the pairs
(key(dist), position in the segment before the call) ascend.  key orders binary32 values numerically with -0 == +0; every NaN, of
either sign and any payload, sorts behind +inf; equal keys keep their earlier order.  Bits are moved, never recomputed.  That is
`np.argsort(dists[a:b], kind="stable")` applied to both arrays -- which `range_ref.stable_by_distance` spells per query; `key_image` and
`order_by_words` spell the same order the way the kernels build it, as one unsigned 64-bit word per entry, so that the two statements
can be held against each other (tests/test_range_sort_host.py)."""
import numpy as np


def range_sort_ref(lims, dists, ids):
    """(dists f32[total], ids u32[total]) of a result sorted by `lmi_range_result_sort`; the inputs are left unchanged."""
    d2 = np.array(dists, dtype=np.float32)
    i2 = np.array(ids, dtype=np.uint32)
    for q in range(len(lims) - 1):
        a, b = int(lims[q]), int(lims[q + 1])
        if b - a > 1:
            o = np.argsort(d2[a:b], kind="stable")
            d2[a:b], i2[a:b] = d2[a:b][o], i2[a:b][o]
    return d2, i2


def key_image(dists):
    """u32: the order-preserving unsigned image of the key -- -0 -> +0, negative values inverted, the others with the sign bit set,
    every NaN all ones (above +inf = 0xff800000)."""
    u = np.ascontiguousarray(dists, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[(u & 0x7FFFFFFF) > 0x7F800000] = 0xFFFFFFFF
    return key


def order_by_words(dists):
    """The permutation of ONE segment as the kernels define it: ascending (key image << 32) | position."""
    words = (key_image(dists).astype(np.uint64) << np.uint64(32)) | np.arange(len(dists), dtype=np.uint64)
    return (np.sort(words) & np.uint64(0xFFFFFFFF)).astype(np.int64)
