"""GPU (`-m gpu`): insert into / delete from a built index (lmi_buckets_insert / lmi_buckets_delete, LearnedIndex.insert /
.delete).

Contract: after any sequence of mutations, searches return byte-identical dists / ids (/ keys) to a fresh build of the
EQUIVALENT OBJECT LIST -- the survivors in the order the index held them, then the inserted objects in call order -- with
the same labels and ids; the oracle (`oracle.search` on that list) agrees as well.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from helpers import inputs_for, layers_from, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def mlp(rs, d, L, hidden=32):
    return [((rs.randn(hidden, d) / np.sqrt(d)).astype(np.float32), (0.1 * rs.randn(hidden)).astype(np.float32)),
            ((rs.randn(L, hidden) / np.sqrt(hidden)).astype(np.float32), (0.1 * rs.randn(L)).astype(np.float32))]


def dataset(rs, n, d, n_centres=16):
    C = rs.randn(n_centres, d).astype(np.float32)
    X = C[rs.randint(0, n_centres, n)] + 0.5 * rs.randn(n, d).astype(np.float32)
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


class Mirror:
    """The equivalent object list of a mutated index."""

    def __init__(self, X, lab, ids):
        self.X, self.lab, self.ids = X.copy(), lab.astype(np.int64).copy(), ids.astype(np.uint32).copy()

    def insert(self, X, lab, ids):
        self.X = np.concatenate([self.X, X])
        self.lab = np.concatenate([self.lab, lab.astype(np.int64)])
        self.ids = np.concatenate([self.ids, ids.astype(np.uint32)])

    def delete(self, ids):
        keep = ~np.isin(self.ids, np.asarray(ids, dtype=np.uint32))
        self.X, self.lab, self.ids = self.X[keep], self.lab[keep], self.ids[keep]
        return int((~keep).sum())


def fresh(capi, layers, m, L, **kw):
    idx = capi.Index(0, **kw)
    idx.set_mlp(layers)
    idx.set_buckets(m.X, m.lab, L, ids=m.ids)
    return idx


def assert_same(capi, oracle, idx, layers, m, L, Q, nbk, metric="ip", prefilter=None):
    ref = fresh(capi, layers, m, L, metric=metric, prefilter=prefilter)
    for nb, k in nbk:
        d1, i1, _, k1 = idx.search(Q, Q, nb, k, want_keys=True)
        d2, i2, _, k2 = ref.search(Q, Q, nb, k, want_keys=True)
        assert np.array_equal(i1, i2), (nb, k)
        assert np.array_equal(d1, d2), (nb, k)
        assert np.array_equal(k1, k2), (nb, k)
        if k <= 2 * capi.K_PER_BUCKET:
            do, no, _ = oracle.search(layers, Q, m.X, Q, m.lab, nb, k, ids=m.ids, nthreads=8, metric=metric)
            assert np.array_equal(i1, no), (nb, k)
            assert np.array_equal(d1.astype(np.float64), do), (nb, k)
    np.testing.assert_array_equal(idx.bucket_sizes(), ref.bucket_sizes())
    ref.close()


@pytest.mark.parametrize("d", [768, 45])
def test_insert_equals_fresh_build(capi, oracle, d):
    rs = np.random.RandomState(d)
    L, N = 12, 6000
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = rs.permutation(10 * N)[:N].astype(np.uint32) + 1
    layers = mlp(rs, d, L)
    Q = dataset(rs, 128, d)
    n0 = int(0.8 * N)
    idx = fresh(capi, layers, Mirror(X[:n0], lab[:n0], ids[:n0]), L)
    m = Mirror(X[:n0], lab[:n0], ids[:n0])
    size0 = int(idx.bucket_sizes()[3])
    # three calls of uneven size; the second sends > 3x bucket 3's size into it (relocation across chunk boundaries)
    extra = dataset(rs, 3 * size0 + 77, d)
    extra_ids = (np.arange(extra.shape[0]) + 20 * N).astype(np.uint32)
    batches = [(X[n0:n0 + 100], lab[n0:n0 + 100], ids[n0:n0 + 100]),
               (extra, np.full(extra.shape[0], 3), extra_ids),
               (X[n0 + 100:], lab[n0 + 100:], ids[n0 + 100:])]
    for xb, lb, ib in batches:
        assert idx.insert(xb, lb, ib) == xb.shape[0]
        m.insert(xb, lb, ib)
    assert idx.bucket_sizes()[3] >= 4 * size0
    assert_same(capi, oracle, idx, layers, m, L, Q, [(nb, k) for nb in (1, 3, 8) for k in (10, 32) if nb == 1 or k <= 10 * nb])
    idx.close()


def test_delete_equals_fresh_build(capi, oracle):
    rs = np.random.RandomState(5)
    L, N, d = 10, 5000, 96
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 128, d)
    m = Mirror(X, lab, ids)
    idx = fresh(capi, layers, m, L)
    gone = list(rs.choice(ids, N // 10, replace=False))
    for b in (0, 4, 7):   # first and last row of some buckets
        sel = ids[lab == b]
        gone += [sel[0], sel[-1]]
    gone += list(ids[lab == 2])   # a whole bucket: it becomes empty
    gone = np.asarray(gone, dtype=np.uint32)
    absent = np.asarray([N + 5, N + 1000, 4_000_000_000], dtype=np.uint32)
    expect = m.delete(gone)
    assert idx.delete(np.concatenate([gone, absent, gone[:7]])) == expect
    assert idx.bucket_sizes()[2] == 0
    assert idx.delete(absent) == 0
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10), (8, 10), (8, 32)])
    idx.close()


@pytest.mark.parametrize("prefilter", [True, False])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_interleaved(capi, oracle, prefilter, metric):
    rs = np.random.RandomState(17 + prefilter + 2 * (metric == "l2"))
    L, N, d = 8, 3000, 64
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 128, d)
    m = Mirror(X[:2000], lab[:2000], ids[:2000])
    idx = fresh(capi, layers, m, L, metric=metric, prefilter=prefilter)
    idx.insert(X[2000:2600], lab[2000:2600], ids[2000:2600])
    m.insert(X[2000:2600], lab[2000:2600], ids[2000:2600])
    gone = np.concatenate([ids[2000:2600:3], m.ids[m.lab == 5], ids[10:400:7]])
    assert idx.delete(gone) == m.delete(gone)
    assert idx.bucket_sizes()[5] == 0
    into5 = np.arange(2600, 3000)
    idx.insert(X[into5], np.full(into5.size, 5), ids[into5])   # the emptied bucket
    m.insert(X[into5], np.full(into5.size, 5), ids[into5])
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10), (8, 16)], metric=metric, prefilter=prefilter)
    idx.close()


def test_insert_rescales(capi, oracle):
    rs = np.random.RandomState(23)
    L, N, d = 6, 2000, 128
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 128, d)
    m = Mirror(X[:1500], lab[:1500], ids[:1500])
    idx = fresh(capi, layers, m, L)
    big = X[1500:] * 4.0 * np.abs(X).max() / np.abs(X[1500:]).max()
    idx.insert(big, lab[1500:], ids[1500:])
    m.insert(big, lab[1500:], ids[1500:])
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10), (6, 20)])
    idx.close()


def test_refusals_leave_the_index_unchanged(capi):
    from learnedmetricindex_amd._capi import LmiError

    rs = np.random.RandomState(29)
    L, N, d = 5, 1000, 32
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 64, d)
    idx = fresh(capi, layers, Mirror(X, lab, ids), L)
    before = idx.search(Q, Q, 3, 10)
    view = idx.clone_view()
    with pytest.raises(LmiError, match="clone"):
        idx.insert(X[:10], lab[:10], ids[:10] + N)
    with pytest.raises(LmiError, match="clone"):
        idx.delete(ids[:10])
    with pytest.raises(LmiError, match="clone"):
        view.delete(ids[:10])
    view.close()
    idx._views.remove(view)
    with pytest.raises(LmiError, match="outside"):
        idx.insert(X[:10], np.r_[lab[:9], L], ids[:10] + N)
    after = idx.search(Q, Q, 3, 10)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    np.testing.assert_array_equal(idx.bucket_sizes(), np.bincount(lab, minlength=L))
    unbuilt = capi.Index(0)
    with pytest.raises(LmiError, match="not built"):
        unbuilt.delete(ids[:3])
    unbuilt.close()
    idx.close()


def test_search_enqueued_before_an_insert_reads_the_old_index(capi):
    rs = np.random.RandomState(31)
    L, N, d = 6, 4000, 256
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 256, d)
    idx = fresh(capi, layers, Mirror(X[:2000], lab[:2000], ids[:2000]), L)
    d0, i0, _ = idx.search(Q, Q, 3, 10)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    q_t = torch.from_numpy(Q).to(dev)
    d_t = torch.empty((Q.shape[0], 10), dtype=torch.float32, device=dev)
    i_t = torch.empty((Q.shape[0], 10), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    idx.set_stream(s.cuda_stream)
    idx.search_device(q_t, q_t, 3, 10, d_t, i_t)
    idx.insert(Q[:50] * 1.5, np.arange(50) % L, np.arange(50, dtype=np.uint32) + 10 * N)   # the queries' near-duplicates
    s.synchronize()
    idx.set_stream(0)
    assert np.array_equal(i_t.cpu().numpy().view(np.uint32), i0)
    assert np.array_equal(d_t.cpu().numpy(), d0)
    d1, i1, _ = idx.search(Q, Q, 3, 10)
    assert not np.array_equal(i1, i0)
    idx.close()


def test_owned_ranks_merge_to_the_fresh_build(capi, oracle):
    rs = np.random.RandomState(37)
    L, N, d, world = 9, 4000, 80, 2
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 128, d)
    m = Mirror(X[:3000], lab[:3000], ids[:3000])
    owned = [(np.arange(L) % world == r).astype(np.uint8) for r in range(world)]
    ranks = []
    for r in range(world):
        h = capi.Index(0)
        h.set_mlp(layers)
        h.set_buckets(m.X, m.lab, L, ids=m.ids, owned=owned[r])
        ranks.append(h)
    stored = [h.insert(X[3000:], lab[3000:], ids[3000:]) for h in ranks]
    assert stored == [int(owned[r][lab[3000:]].sum()) for r in range(world)]
    m.insert(X[3000:], lab[3000:], ids[3000:])
    gone = ids[::9]
    assert sum(h.delete(gone) for h in ranks) == m.delete(gone)
    ref = fresh(capi, layers, m, L)
    for nb, k in ((1, 10), (4, 10), (9, 20)):
        outs = [h.search(Q, Q, nb, k, want_keys=True) for h in ranks]
        kout = outs[0][0].shape[1]
        gd = np.ascontiguousarray(np.stack([o[0] for o in outs]))
        gi = np.ascontiguousarray(np.stack([o[1] for o in outs]))
        gk = np.ascontiguousarray(np.stack([o[3] for o in outs]))
        hd = np.empty((Q.shape[0], kout), np.float32)
        hi = np.empty((Q.shape[0], kout), np.uint32)
        ranks[0].merge_gathered(gd, gi, gk, world, Q.shape[0], kout, hd, hi)
        d2, i2, _ = ref.search(Q, Q, nb, k)
        assert np.array_equal(hi, i2) and np.array_equal(hd, d2), (nb, k)
    for h in ranks + [ref]:
        h.close()


# ---- the `li` API ----------------------------------------------------------------------------------------------------------
def net_from(layers):
    from learnedmetricindex_amd.li.model import NeuralNetwork

    net = NeuralNetwork(input_dim=layers[0][0].shape[1], output_dim=layers[-1][0].shape[0], model_type="MLP")
    lin = [mod for mod in net.model.layers if isinstance(mod, torch.nn.Linear)]
    with torch.no_grad():
        for mod, (W, b) in zip(lin, layers):
            mod.weight.copy_(torch.from_numpy(W))
            mod.bias.copy_(torch.from_numpy(b))
    return net


def frame(X, first_id=1):
    df = pd.DataFrame(X)
    df.index += first_id
    return df


def test_li_insert_delete_one_level(oracle, tmp_path):
    from learnedmetricindex_amd import index_io
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    g = load_golden("G1")
    Xn, Qn, Xs, Qs = inputs_for("G1", g)
    layers = layers_from(g)
    L = layers[-1][0].shape[0]
    dp = g["data_prediction"].astype(np.int64).reshape(-1, 1)
    li = LearnedIndex(net_from(layers), {}, [(i,) for i in range(L)])
    nav = frame(Xn)
    d_orig, n_orig, _ = li.search(nav, Qn, nav, Qs, dp, [L], 3, 10)
    rs = np.random.RandomState(41)
    new = (Xn[rs.choice(Xn.shape[0], 700)] + 0.05 * rs.randn(700, Xn.shape[1])).astype(np.float32)
    new_df = frame(new, first_id=Xn.shape[0] + 1)
    dp_new = li.insert(new_df)
    np.testing.assert_array_equal(dp_new[:, 0], oracle.predict(layers, new))
    gone = np.concatenate([nav.index.to_numpy()[::11], new_df.index.to_numpy()[::5]])
    assert li.delete(gone) == gone.size
    d_res, n_res, _ = li.search_resident(Qn, Qs, [L], 3, 10)
    # the equivalent frames: survivors in order, then the new objects
    all_df = pd.concat([nav, new_df])
    all_dp = np.concatenate([dp, dp_new])
    keep = ~np.isin(all_df.index.to_numpy(), gone)
    eq_df, eq_dp = all_df[keep], all_dp[keep]
    do, no, _ = oracle.search(layers, Qn, eq_df.to_numpy(), Qs, eq_dp, 3, 10, ids=eq_df.index.to_numpy(), nthreads=8)
    assert np.array_equal(n_res, no) and np.array_equal(d_res, do)
    sizes = li._engine.bucket_sizes()
    np.testing.assert_array_equal(sizes, np.bincount(eq_dp[:, 0], minlength=sizes.shape[0]))
    for b in range(sizes.shape[0]):
        rows, bid = li._engine.read_bucket(b)
        sel = eq_dp[:, 0] == b
        np.testing.assert_array_equal(rows, eq_df.to_numpy(dtype=np.float32)[sel])
        np.testing.assert_array_equal(bid, eq_df.index.to_numpy()[sel])
    # save -> load of the mutated index searches identically
    index_io.save_index(str(tmp_path / "mut"), li, [L])
    li2, ncat = index_io.load_index(str(tmp_path / "mut"))
    d_l, n_l, _ = li2.search_resident(Qn, Qs, ncat, 3, 10)
    assert np.array_equal(n_l, n_res) and np.array_equal(d_l, d_res)
    li2.close()
    # `search` answers from the frames it is given: the original ones, then the equivalent ones
    d_o2, n_o2, _ = li.search(nav, Qn, nav, Qs, dp, [L], 3, 10)
    assert np.array_equal(n_o2, n_orig) and np.array_equal(d_o2, d_orig)
    d_f, n_f, _ = li.search(eq_df, Qn, eq_df, Qs, eq_dp, [L], 3, 10)
    assert np.array_equal(n_f, n_res) and np.array_equal(d_f, d_res)
    li.close()


def test_li_insert_two_levels(oracle):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_oracle_multilevel import internal_of

    g = load_golden("G7")
    Xn, Qn, Xs, Qs = inputs_for("G7", g)
    ncat = [int(v) for v in g["n_categories"]]
    nb, k = int(g["n_buckets"]), int(g["k"])
    internal = internal_of(g)
    bucket_paths = [tuple(int(v) for v in p) for p in g["bucket_paths"]]
    dp = g["data_prediction"].astype(np.int64)
    li = LearnedIndex(net_from(layers_from(g)), {p: net_from(lay) for p, lay in internal}, bucket_paths)
    nav, srch = frame(Xn), frame(Xs)
    li.prepare(nav, srch, dp, ncat)
    rs = np.random.RandomState(43)
    pick = rs.choice(Xn.shape[0], 500, replace=False)
    new_nav = frame(Xn[pick] + 0.01 * rs.randn(500, Xn.shape[1]).astype(np.float32), first_id=Xn.shape[0] + 1)
    new_srch = frame(Xs[pick], first_id=Xn.shape[0] + 1)
    sizes0 = li._engine.bucket_sizes().copy()
    dp_new = li.insert(new_nav, new_srch)
    # the per-level argmax: the root, then the model of the node the object went to
    x = new_nav.to_numpy(dtype=np.float32)
    lay_of = dict(internal)
    expect = np.empty_like(dp_new)
    expect[:, 0] = oracle.predict(layers_from(g), x)
    for c in np.unique(expect[:, 0]):
        sel = expect[:, 0] == c
        expect[sel, 1] = oracle.predict(lay_of[(int(c), -1)], x[sel])
    np.testing.assert_array_equal(dp_new, expect)
    assert li._engine.bucket_sizes().sum() == sizes0.sum() + 500
    d_res, n_res, _ = li.search_resident(Qn, Qs, ncat, nb, k)
    li2 = LearnedIndex(li.root_model, li.internal_models, bucket_paths)
    d_f, n_f, _ = li2.search(pd.concat([nav, new_nav]), Qn, pd.concat([srch, new_srch]), Qs, np.concatenate([dp, dp_new]), ncat, nb, k)
    assert np.array_equal(n_res, n_f) and np.array_equal(d_res, d_f)
    li2.close()
    li.close()
    # an index whose data holds no object on one leaf path: an insert that lands there is refused whole, nothing changes
    path = tuple(int(v) for v in dp[0])
    on_path = (dp == np.asarray(path)).all(axis=1)
    li3 = LearnedIndex(net_from(layers_from(g)), {p: net_from(lay) for p, lay in internal}, bucket_paths)
    li3.prepare(nav[~on_path], srch[~on_path], dp[~on_path], ncat)
    sizes3 = li3._engine.bucket_sizes().copy()
    before = li3.search_resident(Qn, Qs, ncat, nb, k)
    with pytest.raises(ValueError, match="no bucket"):
        li3.insert(frame(Xn[on_path][:3], first_id=10 ** 6))
    np.testing.assert_array_equal(li3._engine.bucket_sizes(), sizes3)
    after = li3.search_resident(Qn, Qs, ncat, nb, k)
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[0], after[0])
    li3.close()


# ---- directed edges the random sequences of test_gpu_mutate_fuzz.py cannot afford or might not reach ------------------------
@pytest.mark.parametrize("prefilter", [True, False])
def test_delete_in_several_staging_groups(capi, oracle, prefilter):
    """d = 9000: a delete stages the hit buckets' rows in groups of ~1 GiB (29 826 rows of 36 kB); three buckets of ~11 500
    rows need two groups in both modes."""
    rng = np.random.default_rng(47)
    L, d, per = 3, 9000, 11_500
    X = rng.standard_normal((L * per, d), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    lab = rng.permutation(np.repeat(np.arange(L), per))
    ids = np.arange(1, X.shape[0] + 1, dtype=np.uint32)
    layers = mlp(np.random.RandomState(47), d, L)
    Q = X[rng.choice(X.shape[0], 16, replace=False)] + 0.1 * rng.standard_normal((16, d), dtype=np.float32)
    m = Mirror(X, lab, ids)
    idx = fresh(capi, layers, m, L, prefilter=prefilter)
    gone = np.concatenate([ids[rng.random(ids.size) < 0.05], ids[lab == 1][-40:]])
    assert idx.delete(gone) == m.delete(gone)
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10)], prefilter=prefilter)
    idx.close()


def test_chunk_rows_grow_past_1024_chunks(capi, oracle):
    """chunk_rows = 256 and 270 000 rows inserted into one bucket: it passes 1 024 chunks, so the chunk length grows."""
    rs = np.random.RandomState(53)
    L, N, d = 4, 4000, 8
    X = dataset(rs, N + 270_000, d)
    lab = np.r_[rs.randint(0, L, N), np.full(270_000, 2)]
    ids = np.arange(1, X.shape[0] + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 64, d)
    m = Mirror(X[:N], lab[:N], ids[:N])
    idx = capi.Index(0, chunk_rows=256)
    idx.set_mlp(layers)
    idx.set_buckets(m.X, m.lab, L, ids=m.ids)
    assert idx.insert(X[N:], lab[N:], ids[N:]) == 270_000
    m.insert(X[N:], lab[N:], ids[N:])
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (2, 10), (4, 20)])
    idx.close()


@pytest.mark.parametrize("prefilter", [True, False])
def test_more_than_65535_buckets(capi, oracle, prefilter):
    """L = 70 000: the build's per-bucket maxima, the delete's marking and the range lists of an insert and of a delete that
    touch every bucket each cover more buckets than a grid's y dimension of 65 535."""
    rs = np.random.RandomState(59)
    L, N, d = 70_000, 160_000, 32
    X = dataset(rs, N + L, d)
    lab = np.r_[rs.randint(0, L, N), rs.permutation(L)]
    ids = np.arange(1, X.shape[0] + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 32, d)
    m = Mirror(X[:N], lab[:N], ids[:N])
    idx = fresh(capi, layers, m, L, prefilter=prefilter)
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10)], prefilter=prefilter)
    assert idx.insert(X[N:], lab[N:], ids[N:]) == L      # one row into every bucket
    m.insert(X[N:], lab[N:], ids[N:])
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10)], prefilter=prefilter)
    gone = ids[N:]                                        # ... and out of every bucket again, with some of the build's rows
    gone = np.r_[gone, ids[:N:7]]
    assert idx.delete(gone) == m.delete(gone)
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10)], prefilter=prefilter)
    idx.close()


@pytest.mark.parametrize("prefilter", [True, False])
def test_device_insert_l2(capi, oracle, prefilter):
    """Rows inserted from a CUDA tensor under L2 (the norm column is added on the device)."""
    rs = np.random.RandomState(61)
    L, N, d = 6, 3000, 100
    X = dataset(rs, N, d) * rs.uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 64, d)
    m = Mirror(X[:2000], lab[:2000], ids[:2000])
    idx = fresh(capi, layers, m, L, metric="l2", prefilter=prefilter)
    dev = torch.device("cuda", 0)
    for s in (slice(2000, 2050), slice(2050, 3000)):   # the second one relocates or re-packs
        lb = np.where(np.arange(s.stop - s.start) % 2 == 0, 4, lab[s])
        assert idx.insert(torch.from_numpy(X[s]).to(dev), lb, ids[s]) == s.stop - s.start
        m.insert(X[s], lb, ids[s])
    for b in range(L):
        rows, bid = idx.read_bucket(b)
        np.testing.assert_array_equal(rows, m.X[m.lab == b])
        np.testing.assert_array_equal(bid, m.ids[m.lab == b])
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10), (6, 20)], metric="l2", prefilter=prefilter)
    idx.close()


def test_delete_everything_then_insert(capi, oracle):
    rs = np.random.RandomState(67)
    L, N, d = 5, 2000, 64
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 32, d)
    m = Mirror(X[:1200], lab[:1200], ids[:1200])
    idx = fresh(capi, layers, m, L)
    assert idx.delete(ids) == 1200 == m.delete(ids)
    assert idx.bucket_sizes().sum() == 0
    assert idx.delete(ids) == 0
    for nb, k in ((1, 10), (3, 10)):   # an index of no objects: the oracle's empty answer (inf, id 0)
        d1, i1, _ = idx.search(Q, Q, nb, k)
        do, no, _ = oracle.search(layers, Q, m.X, Q, m.lab, nb, k, ids=m.ids, nthreads=8)
        assert np.array_equal(i1, no) and np.array_equal(d1.astype(np.float64), do), (nb, k)
    small = X[1200:] * np.float32(0.25)   # rows below the old scale's range: the scale stays, the answers must not care
    assert idx.insert(small, lab[1200:], ids[1200:]) == N - 1200
    m.insert(small, lab[1200:], ids[1200:])
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10), (5, 20)])
    idx.close()


def test_rank_that_stores_no_row(capi, oracle):
    """Two ranks; an insert that lands only in rank 0's buckets stores nothing on rank 1 (its early return)."""
    rs = np.random.RandomState(71)
    L, N, d, world = 6, 3000, 48, 2
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 64, d)
    m = Mirror(X[:2000], lab[:2000], ids[:2000])
    owned = [(np.arange(L) % world == r).astype(np.uint8) for r in range(world)]
    ranks = []
    for r in range(world):
        h = capi.Index(0)
        h.set_mlp(layers)
        h.set_buckets(m.X, m.lab, L, ids=m.ids, owned=owned[r])
        ranks.append(h)
    lb = np.where(lab[2000:] % 2 == 0, lab[2000:], 0)   # rank 0's buckets only
    assert [h.insert(X[2000:], lb, ids[2000:]) for h in ranks] == [N - 2000, 0]
    m.insert(X[2000:], lb, ids[2000:])
    gone = ids[::5]
    assert sum(h.delete(gone) for h in ranks) == m.delete(gone)
    ref = fresh(capi, layers, m, L)
    for nb, k in ((1, 10), (3, 10), (6, 20)):
        outs = [h.search(Q, Q, nb, k, want_keys=True) for h in ranks]
        kout = outs[0][0].shape[1]
        gd = np.ascontiguousarray(np.stack([o[0] for o in outs]))
        gi = np.ascontiguousarray(np.stack([o[1] for o in outs]))
        gk = np.ascontiguousarray(np.stack([o[3] for o in outs]))
        hd = np.empty((Q.shape[0], kout), np.float32)
        hi = np.empty((Q.shape[0], kout), np.uint32)
        ranks[0].merge_gathered(gd, gi, gk, world, Q.shape[0], kout, hd, hi)
        d2, i2, _ = ref.search(Q, Q, nb, k)
        assert np.array_equal(hi, i2) and np.array_equal(hd, d2), (nb, k)
    for h in ranks + [ref]:
        h.close()


def test_clone_view_after_mutations(capi, oracle):
    rs = np.random.RandomState(73)
    L, N, d = 7, 3000, 128
    X = dataset(rs, N, d)
    lab = rs.randint(0, L, N)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    layers = mlp(rs, d, L)
    Q = dataset(rs, 64, d)
    m = Mirror(X[:2000], lab[:2000], ids[:2000])
    idx = fresh(capi, layers, m, L)
    idx.insert(X[2000:], np.full(N - 2000, 3), ids[2000:])   # a relocation or re-pack: the view must see the new tables
    m.insert(X[2000:], np.full(N - 2000, 3), ids[2000:])
    gone = ids[::3]
    assert idx.delete(gone) == m.delete(gone)
    view = idx.clone_view()
    ref = fresh(capi, layers, m, L)
    for nb, k in ((1, 10), (3, 10), (7, 20)):
        d1, i1, _, k1 = view.search(Q, Q, nb, k, want_keys=True)
        d2, i2, _, k2 = ref.search(Q, Q, nb, k, want_keys=True)
        assert np.array_equal(i1, i2) and np.array_equal(d1, d2) and np.array_equal(k1, k2), (nb, k)
    ref.close()
    view.close()
    idx._views.remove(view)
    idx.insert(X[:10] * 0.5, np.arange(10) % L, ids[:10] + 10 * N)   # mutable again once the view is gone
    m.insert(X[:10] * 0.5, np.arange(10) % L, ids[:10] + 10 * N)
    assert_same(capi, oracle, idx, layers, m, L, Q, [(1, 10), (3, 10)])
    idx.close()


def test_save_load_mutated_exact_l2(oracle, tmp_path, monkeypatch):
    """A mutated all-f32 L2 index: read_bucket (the f32 fragments unpacked, no norm column) and save -> load."""
    from learnedmetricindex_amd import index_io
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    monkeypatch.setenv("LMI_PREFILTER", "0")
    rs = np.random.RandomState(79)
    L, N, d = 6, 3000, 40
    X = dataset(rs, N, d) * rs.uniform(0.2, 3.0, (N, 1)).astype(np.float32)
    layers = mlp(rs, d, L, hidden=128)   # NeuralNetwork's "MLP": in -> 128 -> out
    Q = dataset(rs, 64, d)
    li = LearnedIndex(net_from(layers), {}, [(i,) for i in range(L)])
    nav = frame(X[:2000])
    dp = oracle.predict(layers, X[:2000]).astype(np.int64).reshape(-1, 1)
    li.prepare(nav, nav, dp, [L], metric="l2")
    assert not li._engine.prefilter_stats()[0]
    new_df = frame(X[2000:], first_id=2001)
    dp_new = li.insert(new_df)
    gone = np.r_[np.arange(1, 2001, 4), np.arange(2001, N + 1, 9)]
    assert li.delete(gone) == gone.size
    all_df = pd.concat([nav, new_df])
    all_dp = np.concatenate([dp, dp_new])
    keep = ~np.isin(all_df.index.to_numpy(), gone)
    eq_X, eq_dp, eq_ids = all_df.to_numpy(dtype=np.float32)[keep], all_dp[keep], all_df.index.to_numpy()[keep]
    for b in range(L):
        rows, bid = li._engine.read_bucket(b)
        sel = eq_dp[:, 0] == b
        np.testing.assert_array_equal(rows, eq_X[sel])
        np.testing.assert_array_equal(bid, eq_ids[sel])
    d_res, n_res, _ = li.search_resident(Q, Q, [L], 3, 10)
    do, no, _ = oracle.search(layers, Q, eq_X, Q, eq_dp, 3, 10, ids=eq_ids, nthreads=8, metric="l2")
    assert np.array_equal(n_res, no) and np.array_equal(d_res, do)
    index_io.save_index(str(tmp_path / "mut"), li, [L])
    li2, ncat = index_io.load_index(str(tmp_path / "mut"))
    assert li2._engine.metric == "l2" and not li2._engine.prefilter_stats()[0]
    d_l, n_l, _ = li2.search_resident(Q, Q, ncat, 3, 10)
    assert np.array_equal(n_l, n_res) and np.array_equal(d_l, d_res)
    li2.close()
    li.close()
