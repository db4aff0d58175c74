"""GPU (`-m gpu`): the fp16 prefilter's error bound under the L2 metric, MEASURED as test_gpu_bound.py measures it under the inner
product: `lmi_debug_emit_all` + `lmi_debug_read_candidates` give the kernel's shat for every (query, row) of four small buckets.

Under LMI_METRIC_L2 the stored row is [x, -|x|^2/2, 0..] (rup(d + 1, 4) columns) and the query [q, 1, 0..]; the ranking key is their
inner product.  So the index's power-of-two scale is set by the norm column, which grows with the SQUARE of the row norm -- the
components sit binades below it in fp16 -- and a query's scale can never exceed 1/2 (the constant 1): a short query is stored as
subnormals beside it.  The reference is the oracle's canonical key: s_c = the k-ordered fmaf chain over the augmented vectors (its
last real link is fmaf(1, -xn/2, s): lmi_oracle.c), s' = s_c * qscale * xscale exactly.  Asserted for every pair:
|shat - s'| / eps' < 1 (the inequality lmi_prefilter.h derives, not a tolerance); every row emitted; eps' finite and positive; ids
and distance bits equal the all-f32 handle's for the batch and the oracle's for the first 16 queries.

Kinds (all un-normalised: on unit vectors the column is the constant -1/2):
  gauss, positive       standard normal / its absolute value
  binade_mix, scales    test_gpu_bound.py's: per-element exponents over 12 binades; rows and queries over four orders of magnitude
  offset                x = c + 0.05 noise, |c_k| ~ 8, queries alike: every key of a bucket is ~ 32 d (<q,x> ~ 64 d against
                        |x|^2/2 ~ 32 d) and two rows' keys differ in the last bits of that number
  norm_dominates        x * 2^10: column ~ d 2^19, components ~ 2^10 -- at d = 768 their fp16 images are subnormal or zero
  short_query           q * 2^-18: beside the augmented 1 every real query component is an fp16 subnormal
  edge_col              one row (8, 0, ..) whose column is exactly -32, the index's largest magnitude: max |x'| = 0.5
  edge_col_below        one row (8 - 2^-21, 2^-9, 0, ..): |x|^2 = nextafter(64, 0), the column the largest binary32 below 32 -- its
                        fp16 image rounds UP to 1.0
Widths: 15 / 16, 31 / 32, 47 / 48 (the column is the last link of a k16 group or the first of the next), 127 / 128 (stored 128 / 132:
the low-dimensional kernels against the general ones), 768, 2047 / 2048 (stored 2048 / 2052).  Every kind runs at 48 and 768, gauss
and offset at every width.  The max ratio and the fallback-slot count per case are printed (pytest -s); a slot that the window
sends to the exact kernel is correct behaviour and not asserted on.

Measured on an MI355X, max |shat - s'| / eps' per case over 256 320 (query, row) pairs each (fallback slots of 384 in brackets):
  kind             d = 48        d = 768
  gauss            0.1471 (0)    0.0181 (0)
  positive         0.1355 (0)    0.0188 (1)
  binade_mix       0.7014 (0)    0.0758 (0)
  scales           0.8996 (288)  0.5742 (288)
  offset           0.0196 (288)  0.0024 (288)
  norm_dominates   0.1218 (0)    0.0164 (0)
  short_query      0.9562 (0)    0.6065 (0)
  edge_col         0.2276 (0)    0.1387 (0)
  edge_col_below   0.2276 (0)    0.1387 (0)
  d        15      16      31      32      47      127     128     2047          2048
  gauss    0.3379  0.3243  0.2063  0.1947  0.1515  0.0819  0.0757  0.0094 (282)  0.0094 (283)
  offset   0.0541  0.0452  0.0311  0.0274  0.0208  0.0098  0.0103  0.0012 (288)  0.0012 (288)
(offset sends 288 slots to the exact kernel at every width, the other gauss cases none.)  The largest, short_query at d = 48, is where
Cauchy-Schwarz is nearly an equality: q' is almost one-hot on the augmented column (1/2 there, 2^-19 elsewhere), so the error is
almost exactly q'_col * (x^_col - x'_col), and for the row whose column rounds worst that is almost qn * dx, the bound's main term.
"""
import numpy as np
import pytest

from test_gpu_bound import L, NB, NQ, SIZES, make

pytestmark = pytest.mark.gpu

WIDTHS = (15, 16, 31, 32, 47, 48, 127, 128, 768, 2047, 2048)
KINDS = ("gauss", "positive", "binade_mix", "scales", "offset", "norm_dominates", "short_query", "edge_col", "edge_col_below")
CASES = [(k, d) for d in (48, 768) for k in KINDS]
CASES += [(k, d) for d in WIDTHS if d not in (48, 768) for k in ("gauss", "offset")]


def make_l2(kind, d, seed):
    if kind in ("binade_mix", "scales"):
        return make(kind, d, seed)
    rs = np.random.RandomState(seed)
    n = sum(SIZES)
    X = rs.randn(n, d).astype(np.float32)
    Q = rs.randn(NQ, d).astype(np.float32)
    if kind == "gauss":
        pass
    elif kind == "positive":
        X, Q = np.abs(X), np.abs(Q)
    elif kind == "offset":
        c = (rs.choice([-8.0, 8.0], size=d) * rs.uniform(0.95, 1.05, size=d)).astype(np.float32)
        X = c + np.float32(0.05) * X
        Q = c + np.float32(0.05) * Q
    elif kind == "norm_dominates":
        X = X * np.float32(2.0 ** 10)
    elif kind == "short_query":
        Q = Q * np.float32(2.0 ** -18)
    elif kind in ("edge_col", "edge_col_below"):   # |x|^2 ~ 16 for the crowd: columns ~ -8, components below 8
        X = X * np.float32(4.0 / np.sqrt(d))
        Q = Q * np.float32(4.0 / np.sqrt(d))
        X[0] = 0.0
        if kind == "edge_col":
            X[0, 0] = 8.0
        else:
            X[0, 0] = np.nextafter(np.float32(8.0), np.float32(0.0))
            X[0, 1] = 2.0 ** -9
    else:
        raise ValueError(kind)
    labels = np.repeat(np.arange(L), SIZES).astype(np.int64)
    perm = rs.permutation(n)
    return np.ascontiguousarray(X[perm]), np.ascontiguousarray(Q), labels[perm]


def augment(oracle, X, Q):
    """The oracle's augmented vectors (knn_l2), zero-padded to the stored width rup(d + 1, 4)."""
    d = X.shape[1]
    dp = (d + 1 + 3) // 4 * 4
    Xa = np.zeros((X.shape[0], dp), np.float32)
    Qa = np.zeros((Q.shape[0], dp), np.float32)
    Xa[:, :d] = X
    Xa[:, d] = np.float32(-0.5) * oracle.sqnorms(X)
    Qa[:, :d] = Q
    Qa[:, d] = 1.0
    return Xa, Qa


@pytest.mark.parametrize("kind,d", CASES)
def test_prefilter_bound_holds_l2(oracle, kind, d):
    from learnedmetricindex_amd import _capi

    X, Q, labels = make_l2(kind, d, seed=1000 + d)
    Xa, Qa = augment(oracle, X, Q)
    col = Xa[:, d]
    if kind == "edge_col":
        assert np.abs(Xa).max() == 32.0 and (col == -32.0).sum() == 1
    if kind == "edge_col_below":
        assert np.abs(Xa).max() == np.nextafter(np.float32(32.0), np.float32(0.0)) and (np.abs(col) == np.abs(Xa).max()).sum() == 1
    order = np.tile(np.arange(L, dtype=np.int32), (NQ, 1))
    idx = _capi.Index(0, prefilter=True, metric="l2")
    idx.set_buckets(X, labels, L)
    idx.debug_emit_all(True)
    dd, ii = idx.scan_topk(Q, order, 10)
    active, _, fallbacks = idx.prefilter_stats()
    assert active
    worst, worst_at, checked = 0.0, None, 0
    for b in range(L):
        rows_b = np.flatnonzero(labels == b)                      # bucket order = ascending original row
        s_c = oracle.forward_logits([(Xa[rows_b], np.zeros(rows_b.size, np.float32))], Qa, nthreads=8)  # chain from 0
        for q in range(NQ):
            r, shat, cnt, eps2, qs, xs = idx.debug_read_candidates(q * NB + b)
            assert cnt == rows_b.size, f"bucket {b} query {q}: {cnt} of {rows_b.size} rows emitted"
            assert eps2 > 0 and np.isfinite(eps2)
            sp = s_c[q, r].astype(np.float64) * float(qs) * float(xs)   # exact: powers of two
            ratio = np.abs(shat.astype(np.float64) - sp) / (0.5 * eps2)
            checked += r.size
            j = int(np.argmax(ratio))
            if ratio[j] > worst:
                worst, worst_at = float(ratio[j]), (b, q, int(r[j]), float(shat[j]), float(sp[j]), 0.5 * eps2)
    print(f"[bound l2] {kind:14s} d={d:4d}: max |shat - s'|/eps' = {worst:.4f} over {checked} (query,row) pairs "
          f"(fallback slots {fallbacks})")
    assert worst < 1.0, f"bound violated: ratio {worst} at (bucket, query, row, shat, s', eps') = {worst_at}"
    # and the answers are the exact mode's / the oracle's, whatever path (fallback) produced them
    idx.close()
    ex = _capi.Index(0, prefilter=False, metric="l2")
    ex.set_buckets(X, labels, L)
    d0, i0 = ex.scan_topk(Q, order, 10)
    ex.close()
    np.testing.assert_array_equal(ii, i0)
    np.testing.assert_array_equal(dd.view(np.uint32), d0.view(np.uint32))
    do, io, _ = oracle.search(None, None, X, Q[:16], labels[:, None], NB, 10, nthreads=8, bucket_order=order[:16][:, :, None],
                              metric="l2")
    np.testing.assert_array_equal(ii[:16], io)
    np.testing.assert_array_equal(dd[:16].astype(np.float64), do)
