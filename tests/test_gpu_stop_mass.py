"""GPU (`-m gpu`): the probability-mass stop (lmi_set_stop_mass) -- a query's bucket order ends once the probabilities of
the ranks it has visited sum to `mass` or more; the ranks cut are -1 and the scan skips them.

Every comparison is exact.  The expected order comes from the unchanged oracle (`predict_proba`, `precompute_bucket_order`)
plus the binary32 running sum of tests/stop_mass_ref.py; expected results from `oracle.search(..., bucket_order=...)`.
Every parity case first asserts that its inputs exercise the cut (stop_mass_ref.assert_not_vacuous).

Inputs: G1 at 0.999 and G5 at 0.99 as they are (n_buckets 4: the histograms test_stop_mass_host.py pins).  G1 at n_buckets 8
leaves only 5 of its 200 queries uncut, so that case runs G1's queries AND a copy of them scaled by 0.7 (flatter
probabilities): 110 of 400 uncut.  G3's model is so sure at 0.999 (233 of 256 queries stop after one bucket, 8 uncut) that
its case takes mass 0.9999 (51 uncut).  The wide path (L = 1 024 > 512 classes) has no fixture: a seeded random MLP."""
import numpy as np
import pandas as pd
import pytest
import torch

from helpers import inputs_for, layers_from, load_golden
from stop_mass_ref import assert_not_vacuous, expected_order

pytestmark = pytest.mark.gpu

MODEL_OF = {"G1": "MLP", "G5": "MLP-4"}


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def wide_model():
    """48 -> 64 -> 1 024 classes, output weights scaled so that the top probabilities spread over several ranks."""
    rs = np.random.RandomState(7)
    d, hidden, L = 48, 64, 1024
    layers = [((rs.randn(hidden, d) / np.sqrt(d)).astype(np.float32), (0.1 * rs.randn(hidden)).astype(np.float32)),
              ((12.0 * rs.randn(L, hidden) / np.sqrt(hidden)).astype(np.float32), (0.1 * rs.randn(L)).astype(np.float32))]
    return layers, rs.randn(300, d).astype(np.float32)


def nav_case(name):
    """(layers, navigation queries) of an order-parity case."""
    if name == "wide1024":
        return wide_model()
    g = load_golden(name.split("+")[0])
    _, Qn, _, _ = inputs_for(name.split("+")[0], g)
    if name.endswith("+flat"):
        Qn = np.concatenate([Qn, (Qn * np.float32(0.7)).astype(np.float32)])
    return layers_from(g), Qn


def search_case(name):
    g = load_golden(name)
    Xn, Qn, Xs, Qs = inputs_for(name, g)
    return g, layers_from(g), Qn, Xs, Qs, g["data_prediction"]


def built(capi, layers, Xs, dp, **kw):
    idx = capi.Index(0, **kw)
    idx.set_mlp(layers)
    idx.set_buckets(Xs, dp[:, 0], layers[-1][0].shape[0])
    return idx


ORDER_CASES = [("G1", 0.999, 4), ("G1+flat", 0.999, 8), ("G5", 0.99, 4), ("G5", 0.99, 8), ("G3", 0.9999, 4), ("wide1024", 0.9, 4)]


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("name,mass,nb", ORDER_CASES)
def test_order_parity(capi, oracle, name, mass, nb, fused):
    """1. lmi_mlp_topk with the stop on equals the oracle's order with the cut ranks at -1, on each of the three ranking
    paths: per-layer kernels + ranking kernel (fused 0, and 1 at these batch sizes), the fused kernel's epilogue (2), and
    the ranking kernel behind a fused launch whose 1 024 logits went through global memory (wide1024 under 2)."""
    layers, Qn = nav_case(name)
    bo, counts = expected_order(oracle, layers, Qn, nb, mass)
    assert_not_vacuous(counts, nb)
    idx = capi.Index(0)
    idx.set_mlp(layers)
    idx.set_fused_mlp(fused)
    idx.set_stop_mass(mass)
    got = idx.mlp_topk(Qn, nb)
    idx.close()
    print(f"{name} mass {mass} nb {nb} fused {fused}: rows differing {(got != bo[:, :, 0]).any(axis=1).sum()} of {Qn.shape[0]}")
    assert np.array_equal(got, bo[:, :, 0])


def test_order_parity_split_batch(capi, oracle):
    """A batch of 313 32-query blocks under the default mode: the fused kernel takes one full round of blocks and the
    per-layer kernels the rest on a side stream -- both halves must cut alike."""
    layers, Qn = nav_case("G1")
    rs = np.random.RandomState(11)
    scale = rs.uniform(0.5, 1.0, size=(10000, 1)).astype(np.float32)
    Q = np.ascontiguousarray(Qn[rs.randint(Qn.shape[0], size=10000)] * scale)
    bo, counts = expected_order(oracle, layers, Q, 4, 0.999)
    assert_not_vacuous(counts, 4)
    idx = capi.Index(0)
    idx.set_mlp(layers)
    idx.set_stop_mass(0.999)
    got = idx.mlp_topk(Q, 4)
    idx.close()
    assert np.array_equal(got, bo[:, :, 0])


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("prefilter", [True, False])
@pytest.mark.parametrize("name,mass,nb", [("G1", 0.999, 4), ("G5", 0.99, 4)])
def test_search_parity(capi, oracle, name, mass, nb, prefilter, metric):
    """2. lmi_search: dists, ids and the returned bucket order equal the oracle's search over the cut order."""
    g, layers, Qn, Xs, Qs, dp = search_case(name)
    bo, counts = expected_order(oracle, layers, Qn, nb, mass)
    assert_not_vacuous(counts, nb)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo, metric=metric)
    idx = built(capi, layers, Xs, dp, prefilter=prefilter, metric=metric)
    idx.set_stop_mass(mass)
    d, i, got_bo = idx.search(Qn, Qs, nb, 10)
    idx.close()
    assert np.array_equal(got_bo, bo[:, :, 0])
    assert np.array_equal(i, no)
    assert np.array_equal(d.astype(np.float64), do)


@pytest.mark.parametrize("name,mass,nb", [("G1", 0.999, 4), ("G5", 0.99, 4)])
def test_work_is_skipped(capi, oracle, name, mass, nb):
    """3. lmi_scan_stats' pairs is the sum of the bucket sizes over the slots that were kept -- an exact integer, strictly
    below the full search's."""
    g, layers, Qn, Xs, Qs, dp = search_case(name)
    bo, counts = expected_order(oracle, layers, Qn, nb, mass)
    assert_not_vacuous(counts, nb)
    sizes = np.bincount(dp[:, 0], minlength=layers[-1][0].shape[0]).astype(np.int64)
    full = oracle.precompute_bucket_order(layers, Qn, nb)[:, :, 0]
    kept = bo[:, :, 0]
    idx = built(capi, layers, Xs, dp)
    idx.search(Qn, Qs, nb, 10)
    pairs_off = idx.scan_stats()[1]
    idx.set_stop_mass(mass)
    idx.search(Qn, Qs, nb, 10)
    pairs_on = idx.scan_stats()[1]
    idx.close()
    print(f"{name}: pairs {pairs_on} with the stop, {pairs_off} without")
    assert pairs_off == int(sizes[full].sum())
    assert pairs_on == int(sizes[kept[kept >= 0]].sum())
    assert pairs_on < pairs_off


def test_off_means_off(capi, oracle):
    """4. mass 0 after a mass is today's behaviour; n_buckets 1 is unaffected; invalid values are refused with a message
    and leave the setting in force."""
    g, layers, Qn, Xs, Qs, dp = search_case("G1")
    nb, mass = 4, 0.999
    bo, _ = expected_order(oracle, layers, Qn, nb, mass)
    never = built(capi, layers, Xs, dp)
    idx = built(capi, layers, Xs, dp)
    ref = never.search(Qn, Qs, nb, 10)
    ref1 = never.search(Qn, Qs, 1, 10)
    idx.set_stop_mass(mass)
    assert idx.stop_mass == float(np.float32(mass))
    on1 = idx.search(Qn, Qs, 1, 10)
    for a, b in zip(on1, ref1):
        assert np.array_equal(a, b)
    assert np.array_equal(idx.mlp_topk(Qn, 1), never.mlp_topk(Qn, 1))
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(capi.LmiError, match="lmi_set_stop_mass"):
            idx.set_stop_mass(bad)
        assert idx.stop_mass == float(np.float32(mass))
    assert np.array_equal(idx.search(Qn, Qs, nb, 10)[2], bo[:, :, 0])   # the refused values changed nothing
    idx.set_stop_mass(1.0)   # the largest valid value
    assert np.array_equal(idx.mlp_topk(Qn, nb), expected_order(oracle, layers, Qn, nb, 1.0)[0][:, :, 0])
    idx.set_stop_mass(0.0)
    off = idx.search(Qn, Qs, nb, 10)
    for a, b in zip(off, ref):
        assert np.array_equal(a, b)
    assert np.array_equal(idx.mlp_topk(Qn, nb), never.mlp_topk(Qn, nb))
    probs, classes = idx.mlp_proba(Qn)   # predict_proba is never cut
    idx.set_stop_mass(mass)
    probs2, classes2 = idx.mlp_proba(Qn)
    assert np.array_equal(classes, classes2) and np.array_equal(probs, probs2) and (classes2 >= 0).all()
    idx.close()
    never.close()


def test_clone_view_inherits(capi, oracle):
    """5. A clone view starts with the value its parent has when the clone is made; afterwards the two are independent."""
    g, layers, Qn, Xs, Qs, dp = search_case("G1")
    nb, mass = 4, 0.999
    bo, _ = expected_order(oracle, layers, Qn, nb, mass)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo)
    full = oracle.precompute_bucket_order(layers, Qn, nb)[:, :, 0]
    idx = built(capi, layers, Xs, dp)
    plain = idx.clone_view()
    idx.set_stop_mass(mass)
    view = idx.clone_view()
    assert view.stop_mass == idx.stop_mass and plain.stop_mass == 0.0
    idx.set_stop_mass(0.0)
    d, i, got = view.search(Qn, Qs, nb, 10)
    assert np.array_equal(got, bo[:, :, 0]) and np.array_equal(i, no) and np.array_equal(d.astype(np.float64), do)
    assert np.array_equal(plain.search(Qn, Qs, nb, 10)[2], full)
    assert np.array_equal(idx.search(Qn, Qs, nb, 10)[2], full)
    idx.close()


def test_mutated_index(capi, oracle):
    """6. After insert and delete the stop's results equal the oracle's on the equivalent object list (the survivors in the
    order the index held them, then the inserted objects)."""
    g, layers, Qn, Xs, Qs, dp = search_case("G1")
    nb, mass = 4, 0.999
    lab = dp[:, 0].astype(np.int64)
    ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    n0 = int(0.8 * Xs.shape[0])
    idx = capi.Index(0)
    idx.set_mlp(layers)
    idx.set_buckets(Xs[:n0], lab[:n0], 12, ids=ids[:n0])
    assert idx.insert(Xs[n0:], lab[n0:], ids[n0:]) == Xs.shape[0] - n0
    gone = np.random.RandomState(3).choice(ids, 700, replace=False)
    assert idx.delete(gone) == 700
    keep = ~np.isin(ids, gone)
    bo, counts = expected_order(oracle, layers, Qn, nb, mass)
    assert_not_vacuous(counts, nb)
    do, no, _ = oracle.search(layers, Qn, Xs[keep], Qs, lab[keep], nb, 10, ids=ids[keep], nthreads=4, bucket_order=bo)
    idx.set_stop_mass(mass)
    d, i, got = idx.search(Qn, Qs, nb, 10)
    idx.close()
    assert np.array_equal(got, bo[:, :, 0]) and np.array_equal(i, no) and np.array_equal(d.astype(np.float64), do)


def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


def net_from(layers, model_type="MLP"):
    from learnedmetricindex_amd.li.model import NeuralNetwork

    net = NeuralNetwork(input_dim=layers[0][0].shape[1], output_dim=layers[-1][0].shape[0], model_type=model_type)
    lin = [m for m in net.model.layers if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for m, (W, b) in zip(lin, layers):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
    return net


@pytest.mark.parametrize("name,mass,nb", [("G1", 0.999, 4), ("G5", 0.99, 4)])
def test_li_api(oracle, name, mass, nb):
    """7. LearnedIndex.search / search_resident with stop_mass equal the oracle; the next call without it is the full search."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    g, layers, Qn, Xs, Qs, dp = search_case(name)
    L = layers[-1][0].shape[0]
    dp = dp.astype(np.int64)
    bo, counts = expected_order(oracle, layers, Qn, nb, mass)
    assert_not_vacuous(counts, nb)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo)
    df, nf, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4)
    if name == "G5":   # (G1's neighbour ids at 0.999 are the full search's for all 200 queries; G5's differ for 5 %)
        assert not np.array_equal(no, nf)
    li = LearnedIndex(net_from(layers, MODEL_OF[name]), {}, [(i,) for i in range(L)])
    nav, srch = frame(inputs_for(name, g)[0]), frame(Xs)
    d, n, mt = li.search(nav, Qn, srch, Qs, dp, [L], nb, 10, stop_mass=mass)
    assert np.array_equal(n, no) and np.array_equal(d, do) and mt["inference"] > 0
    assert li._engine.stop_mass == 0.0   # applied for the call, restored afterwards
    d, n, _ = li.search(nav, Qn, srch, Qs, dp, [L], nb, 10)
    assert np.array_equal(n, nf) and np.array_equal(d, df)
    d, n, _ = li.search_resident(Qn, Qs, [L], nb, 10, stop_mass=mass)
    assert np.array_equal(n, no) and np.array_equal(d, do)
    d, n, _ = li.search_resident(Qn, Qs, [L], nb, 10)
    assert np.array_equal(n, nf) and np.array_equal(d, df)
    with pytest.raises(_lmi_error()):   # an invalid value is the engine's error; the setting is as before afterwards
        li.search_resident(Qn, Qs, [L], nb, 10, stop_mass=1.5)
    d, n, _ = li.search_resident(Qn, Qs, [L], nb, 10)
    assert np.array_equal(n, nf) and np.array_equal(d, df)
    li.close()


def _lmi_error():
    from learnedmetricindex_amd import _capi

    return _capi.LmiError


def test_li_api_refuses_multi_level(oracle):
    """7. A 2-level index (G2, [4, 3]) refuses stop_mass with ValueError before any work; its searches are unchanged."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_oracle_multilevel import internal_of

    g = load_golden("G2")
    Xn, Qn, Xs, Qs = inputs_for("G2", g)
    ncat = [int(v) for v in g["n_categories"]]
    nb, k = int(g["n_buckets"]), int(g["k"])
    internal = internal_of(g)
    bucket_paths = [tuple(int(v) for v in p) for p in g["bucket_paths"]]
    li = LearnedIndex(net_from(layers_from(g)), {p: net_from(l) for p, l in internal}, bucket_paths)
    dp = g["data_prediction"].astype(np.int64)
    nav, srch = frame(Xn), frame(Xs)
    with pytest.raises(ValueError, match="multi-level"):
        li.search(nav, Qn, srch, Qs, dp, ncat, nb, k, stop_mass=0.9)
    assert li._engine is None   # refused before the index was even uploaded
    d0, n0, _ = li.search(nav, Qn, srch, Qs, dp, ncat, nb, k)
    with pytest.raises(ValueError, match="multi-level"):
        li.search_resident(Qn, Qs, ncat, nb, k, stop_mass=0.9)
    d1, n1, _ = li.search_resident(Qn, Qs, ncat, nb, k)
    assert np.array_equal(n0, n1) and np.array_equal(d0, d1)
    bo_o = oracle.precompute_bucket_order_multilevel(layers_from(g), internal, bucket_paths, Qn, nb, ncat)
    do, no, _ = oracle.search(layers_from(g), Qn, Xs, Qs, dp, nb, k, bucket_order=bo_o)
    assert np.array_equal(n0, no) and np.array_equal(d0, do)
    # the C calls of the walk ignore a mass set on the handle
    li._engine.set_stop_mass(0.5)
    d2, n2, _ = li.search_resident(Qn, Qs, ncat, nb, k)
    assert np.array_equal(n2, no) and np.array_equal(d2, do)
    li.close()


@pytest.mark.parametrize("mode", ["nav", "plain", "twin", "plain-python"])
def test_pipeline(capi, oracle, mode):
    """8. HostPipeline(stop_mass=...) returns, batch by batch, what the direct call with the stop returns (and the oracle)."""
    from learnedmetricindex_amd.pipeline import HostPipeline

    g, layers, Qn, Xs, Qs, dp = search_case("G1")
    nb, mass, nq = 4, 0.999, 96
    idx = built(capi, layers, Xs, dp)
    pipe = HostPipeline(idx, nq, Qn.shape[1], Qs.shape[1], nb, 10, depth=2, same_queries=True, want_bucket_order=True,
                        overlap_inference=mode == "nav", two_handles=mode == "twin", native_submit=mode != "plain-python",
                        stop_mass=mass)
    assert len(pipe.handles) == (2 if mode == "twin" else 1) and all(h.stop_mass == float(np.float32(mass)) for h, _ in pipe.handles)
    rs = np.random.RandomState(0)
    batches = [np.sort(rs.choice(Qn.shape[0], nq, replace=False)) for _ in range(5)]
    got = []
    for sel in batches:
        t = pipe.submit(np.ascontiguousarray(Qn[sel]))
        d, i = pipe.result(t)
        got.append((d.copy(), i.copy(), pipe.bucket_order(t).copy()))
    pipe.close()
    assert idx.stop_mass == 0.0   # the pipeline's setting ends with it
    idx.set_stream(0)
    idx.set_stop_mass(mass)       # the direct calls below
    cut = 0
    for sel, (d, i, bo_p) in zip(batches, got):
        q = np.ascontiguousarray(Qn[sel])
        d0, i0, bo0 = idx.search(q, q, nb, 10)
        bo, counts = expected_order(oracle, layers, q, nb, mass)
        cut += int((counts < nb).sum())
        assert np.array_equal(bo_p, bo0) and np.array_equal(bo_p, bo[:, :, 0])
        assert np.array_equal(i, i0) and np.array_equal(d, d0)
    assert cut > 0
    q = np.ascontiguousarray(Qn[batches[0]])
    do, no, _ = oracle.search(layers, q, Xs, q, dp, nb, 10, nthreads=4, bucket_order=expected_order(oracle, layers, q, nb, mass)[0])
    assert np.array_equal(got[0][1], no) and np.array_equal(got[0][0].astype(np.float64), do)
    idx.close()


@pytest.mark.parametrize("searcher", ["sharded", "replica"])
def test_sharded_world_of_one(capi, oracle, searcher):
    """9. A world-of-one ShardedSearcher / ReplicaSearcher with stop_mass equals the direct call and the oracle."""
    from learnedmetricindex_amd.sharded import ReplicaSearcher, ShardedSearcher

    g, layers, Qn, Xs, Qs, dp = search_case("G5")
    nb, mass = 4, 0.99
    bo, counts = expected_order(oracle, layers, Qn, nb, mass)
    assert_not_vacuous(counts, nb)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo)
    dev = torch.device("cuda", 0)
    qn, qs = torch.from_numpy(Qn).to(dev), torch.from_numpy(Qs).to(dev)
    idx = built(capi, layers, Xs, dp, chunk_rows=256)
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    s = ShardedSearcher(idx, 0, 1, stop_mass=mass) if searcher == "sharded" else ReplicaSearcher(idx, 0, 1, stop_mass=mass)
    sd, si, sbo = s.search(qn, qs, nb, 10)
    torch.cuda.synchronize()
    sd, si, sbo = sd.cpu().numpy(), si.cpu().numpy().view(np.uint32), sbo.cpu().numpy()
    idx.set_stream(0)
    d0, i0, bo0 = idx.search(Qn, Qs, nb, 10)
    s.close()
    assert idx.stop_mass == 0.0   # the searcher's setting ends with it
    assert np.array_equal(idx.search(Qn, Qs, nb, 10)[2], oracle.precompute_bucket_order(layers, Qn, nb)[:, :, 0])
    idx.close()
    assert np.array_equal(sbo, bo0) and np.array_equal(si, i0) and np.array_equal(sd, d0)
    assert np.array_equal(sbo, bo[:, :, 0]) and np.array_equal(si, no) and np.array_equal(sd.astype(np.float64), do)


def test_pipeline_refuses_invalid_mass_cleanly(capi):
    """An invalid stop_mass fails in HostPipeline's constructor before its clone view is made: nothing is left on the index."""
    from learnedmetricindex_amd.pipeline import HostPipeline

    g, layers, Qn, Xs, Qs, dp = search_case("G1")
    idx = built(capi, layers, Xs, dp)
    with pytest.raises(capi.LmiError, match="lmi_set_stop_mass"):
        HostPipeline(idx, 32, Qn.shape[1], Qs.shape[1], 4, 10, same_queries=True, two_handles=True, stop_mass=1.5)
    assert idx.stop_mass == 0.0 and not getattr(idx, "_views", [])
    assert idx.insert(Xs[:1], dp[:1, 0], np.asarray([4_000_000], dtype=np.uint32)) == 1   # no clone view alive: a mutation is accepted
    idx.set_stream(0)
    idx.close()
