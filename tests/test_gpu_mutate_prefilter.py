"""GPU (`-m gpu`): the prefilter's own state after inserts and deletes, slot by slot against a fresh build.

A mutation redoes the fp16 row-blocks, the per-bucket norm maxima (bnorm / bdelta) and, when new rows break max|x'| < 1, the
power-of-two scale, piecemeal.  A stale fp16 row-block, a maximum over the wrong rows or a scale that is not re-derived can
leave the answers unchanged on friendly data while eps' shrinks below the real error.  So the test hooks of test_gpu_bound.py
(`debug_emit_all`: pass 2 emits every row of a visited bucket of <= 1024 rows; `debug_read_candidates`: its shat, count,
2 eps' and the two scales per slot) read the mutated index's state out:

  * after inserts (slack, relocation and re-packs, with and without a new scale): every slot's rows, shat, count, eps2, qscale
    and xscale equal the fresh build's bit for bit -- the scale, the maxima and the fp16 images are order-independent
    functions of the stored rows;
  * after deletes (the rows that hold a bucket's largest norm and the global absmax among them): with the fresh build's
    xscale, bit for bit as above; with a smaller one (the absmax left: a delete keeps the scale), |shat - s'| < eps' against
    the oracle's canonical chain, as test_gpu_bound.py asserts;
  * always: the answers equal the all-f32 mode's and the oracle's.
The data is test_gpu_bound.py's `make` (positive, binade_mix, scales, edge_one), not only friendly Gaussians."""
import numpy as np
import pytest

from test_gpu_bound import make
from test_gpu_mutate import Mirror

pytestmark = pytest.mark.gpu

L, NB, NQ = 4, 4, 96


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def emit_all(capi, m, prefilter=True, chunk_rows=256):
    idx = capi.Index(0, prefilter=prefilter, chunk_rows=chunk_rows)
    idx.set_buckets(m.X, m.lab, L, ids=m.ids)
    return idx


def slots(idx, Q):
    """scan_topk of every query over the buckets in order 0..3, every row emitted; per slot the hooks' state, rows sorted."""
    idx.debug_emit_all(True)
    order = np.tile(np.arange(L, dtype=np.int32), (Q.shape[0], 1))
    dd, ii = idx.scan_topk(Q, order, 10)
    active, _, _ = idx.prefilter_stats()
    assert active
    out = []
    for s in range(Q.shape[0] * NB):
        r, shat, cnt, eps2, qs, xs = idx.debug_read_candidates(s)
        o = np.argsort(r, kind="stable")
        out.append((r[o], shat[o], cnt, eps2, qs, xs))
    return out, dd, ii


def assert_bit_equal(a, b, what):
    for s, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]), f"{what}: slot {s} rows"
        assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), f"{what}: slot {s} shat"
        assert x[2] == y[2], f"{what}: slot {s} count {x[2]} != {y[2]}"
        for j, name in ((3, "eps2"), (4, "qscale"), (5, "xscale")):
            assert np.float32(x[j]).view(np.uint32) == np.float32(y[j]).view(np.uint32), f"{what}: slot {s} {name} {x[j]} != {y[j]}"


def assert_answers(capi, oracle, m, Q, dd, ii):
    order = np.tile(np.arange(L, dtype=np.int32), (Q.shape[0], 1))
    ex = capi.Index(0, prefilter=False)
    ex.set_buckets(m.X, m.lab, L, ids=m.ids)
    d0, i0 = ex.scan_topk(Q, order, 10)
    ex.close()
    np.testing.assert_array_equal(ii, i0)
    np.testing.assert_array_equal(dd, d0)
    do, io, _ = oracle.search(None, None, m.X, Q[:16], m.lab, NB, 10, ids=m.ids, nthreads=8, bucket_order=order[:16][:, :, None])
    np.testing.assert_array_equal(ii[:16].view(np.uint32), io)
    np.testing.assert_array_equal(dd[:16].astype(np.float64), do)


INSERT_CASES = [(k, d, r) for k, d in (("positive", 768), ("binade_mix", 768), ("edge_one", 768), ("binade_mix", 45),
                                       ("scales", 100), ("positive", 100)) for r in (False, True)]


@pytest.mark.parametrize("kind,d,rescale", INSERT_CASES)
def test_prefilter_state_after_inserts_equals_fresh(capi, oracle, kind, d, rescale):
    X, Q, lab = make(kind, d, seed=2000 + d)
    rs = np.random.RandomState(d + rescale)
    rows = [np.flatnonzero(lab == b) for b in range(L)]      # bucket sizes 1000, 640, 997, 33
    # built: 700 / 448 / 997 / 1 rows (69 row-blocks); then, 256-row chunks (8 row-blocks of slack per relocation):
    #   +4 rows into bucket 0's last row-block (slack), +552 into bucket 1 (40 row-blocks: past the allocation, a re-pack),
    #   +32 into bucket 3 (2 -> 10 row-blocks behind the last one: a relocation into the re-pack's 1/8 headroom)
    init = np.sort(np.concatenate([rows[0][:700], rows[1][:448], rows[2], rows[3][:1]]))
    m = Mirror(X[init], lab[init], init.astype(np.uint32) + 1)
    idx = emit_all(capi, m)
    pool = np.setdiff1d(np.arange(X.shape[0]), init)
    next_id = 10_000
    steps = [(0, 4), (1, 552), (3, 32)]
    big_at = 1 + int(rs.randint(2)) if rescale else -1       # the step whose rows carry a new absmax (4x the index's)
    seen = np.zeros(4, dtype=np.int64)
    for i, (b, n) in enumerate(steps):
        src = pool[rs.randint(0, pool.size, n)]             # other buckets' rows as well: not only the bucket's own distribution
        xb = X[src].copy()
        if i == big_at:
            xb[0] = 0
            xb[0, rs.randint(d)] = np.float32(4.0) * np.abs(m.X).max()
        ids = np.arange(next_id, next_id + n, dtype=np.uint32)
        next_id += n
        assert idx.insert(xb, np.full(n, b), ids) == n
        m.insert(xb, np.full(n, b), ids)
        seen = idx.debug_layout()["counters"]
        ref = emit_all(capi, m)
        a, dd, ii = slots(idx, Q)
        f, _, _ = slots(ref, Q)
        ref.close()
        assert_bit_equal(a, f, f"{kind} d={d} after insert {i} (layout paths {seen.tolist()})")
        assert_answers(capi, oracle, m, Q, dd, ii)
    assert seen[0] >= 1 and seen[1] >= 1 and seen[2] + seen[3] >= 1, f"layout paths {seen.tolist()}"
    idx.close()


DELETE_CASES = [(k, d, s) for k, d in (("positive", 768), ("binade_mix", 768), ("edge_one", 768), ("binade_mix", 45),
                                       ("scales", 100)) for s in (True, False)]


@pytest.mark.parametrize("kind,d,sentinel", DELETE_CASES)
def test_prefilter_state_after_deletes(capi, oracle, kind, d, sentinel):
    """A planted row holds the index's absmax (4x the rest) in bucket 3.  sentinel: it is never deleted, the scale stays the
    fresh build's and everything must be bit-equal; otherwise the second delete takes it, the fresh build's scale is larger and
    the mutated index must keep the bound with its own (smaller) scale."""
    X, Q, lab = make(kind, d, seed=3000 + d)
    rs = np.random.RandomState(d + 7 * sentinel)
    plant = np.zeros((1, d), np.float32)
    plant[0, rs.randint(d)] = np.float32(4.0) * np.abs(X).max()
    X = np.concatenate([X, plant])
    lab = np.concatenate([lab, [3]])
    m = Mirror(X, lab, np.arange(1, X.shape[0] + 1, dtype=np.uint32))
    idx = emit_all(capi, m)
    norms = np.linalg.norm(X.astype(np.float64), axis=1)
    rest = np.arange(X.shape[0] - 1)
    absmax_row = int(rest[np.argmax(np.abs(X[rest]).max(axis=1))])
    top_norm = [int(np.flatnonzero(lab == b)[np.argmax(norms[lab == b])]) for b in (0, 1, 2)]
    steps = [np.concatenate([top_norm, rs.choice(np.flatnonzero(lab == 2), 100, replace=False)]),
             np.asarray([absmax_row] + ([] if sentinel else [X.shape[0] - 1])
                        + list(rs.choice(np.flatnonzero(lab == 0), 300, replace=False)))]
    for i, gone in enumerate(steps):
        ids = np.unique(gone).astype(np.uint32) + 1
        assert idx.delete(ids) == m.delete(ids)
        ref = emit_all(capi, m)
        a, dd, ii = slots(idx, Q)
        f, _, _ = slots(ref, Q)
        ref.close()
        xs_m, xs_f = a[0][5], f[0][5]
        if sentinel or i == 0:
            assert xs_m == xs_f, (xs_m, xs_f)
        else:
            assert xs_m < xs_f, (xs_m, xs_f)                  # the absmax row is gone: the fresh scale is at least 2x
        if xs_m == xs_f:
            assert_bit_equal(a, f, f"{kind} d={d} after delete {i}")
        else:
            worst = 0.0
            for b in range(L):
                sel = m.lab == b
                s_c = oracle.forward_logits([(m.X[sel], np.zeros(int(sel.sum()), np.float32))], Q, nthreads=8)
                for q in range(NQ):
                    r, shat, cnt, eps2, qs, xs = a[q * NB + b]
                    assert cnt == sel.sum(), f"bucket {b} query {q}: {cnt} of {sel.sum()} rows emitted"
                    assert xs == xs_m and eps2 > 0 and np.isfinite(eps2)
                    sp = s_c[q, r].astype(np.float64) * float(qs) * float(xs)
                    if r.size:
                        worst = max(worst, float((np.abs(shat.astype(np.float64) - sp) / (0.5 * eps2)).max()))
            print(f"[mutate bound] {kind:10s} d={d:4d} after delete {i}: max |shat - s'|/eps' = {worst:.4f}")
            assert worst < 1.0, f"bound violated after a delete: ratio {worst}"
        assert_answers(capi, oracle, m, Q, dd, ii)
    idx.close()
