"""GPU (`-m gpu`): the index build on binary16 rows, end to end.  `lmi_mlp_topk_f16` (the placement check's forward) on float16
queries, host and device, equals `lmi_mlp_topk` on the widened queries; `LearnedIndexBuilder` with `hip_kmeans` and `trainer="hip"`
on a float16 frame hands float16 to `_capi.kmeans` / `_capi.train` / the placement check and builds, bit for bit, the index it
builds from the widened frame: the same weights, the same placement, the same bucket paths."""
import numpy as np
import pandas as pd
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- lmi_mlp_topk_f16 ---------------------------------------------------------------------------------------------------------------
def random_layers(rs, dims):
    return [((rs.randn(dims[i + 1], dims[i]) / np.sqrt(dims[i])).astype(np.float32), (0.1 * rs.randn(dims[i + 1])).astype(np.float32))
            for i in range(len(dims) - 1)]


# odd d: element loads everywhere; d % 8 == 0: the widening kernel's 16-byte form, the fused forward's 16-byte input loads
@pytest.mark.parametrize("dims", [(45, 32, 7), (64, 128, 12), (768, 512, 130)], ids=lambda v: "x".join(map(str, v)))
def test_mlp_topk_on_halves_equals_the_call_on_the_widened_queries(capi, oracle, dims):
    rs = np.random.RandomState(dims[0])
    layers = random_layers(rs, dims)
    nq, nb, L = 333, min(5, dims[-1]), dims[-1]
    q16 = rs.randn(nq, dims[0]).astype(np.float16)
    q32 = q16.astype(np.float32)
    idx = capi.Index(0)
    try:
        idx.set_mlp(layers)
        order32, logits32 = idx.mlp_topk(q32, nb, want_logits=True)
        order16, logits16 = idx.mlp_topk(q16, nb, want_logits=True)
        assert order16.dtype == np.int32 and np.array_equal(order16, order32)
        assert np.array_equal(bits(logits16), bits(logits32))
        assert np.array_equal(order16[:, 0], oracle.predict(layers, q32))
        assert np.array_equal(idx.mlp_topk(q16, nb), order32)   # without the logits output: the fused form ranks in LDS
        for shift in (0, 1):   # device halves: 16-byte aligned, and one half past the boundary
            room = torch.zeros(nq * dims[0] + shift, dtype=torch.float16, device="cuda")
            room[shift:] = torch.from_numpy(q16).cuda().reshape(-1)
            qt = room[shift:].reshape(nq, dims[0])
            assert qt.data_ptr() % 16 == 2 * shift and qt.is_contiguous()
            keep = qt.clone()
            bo = torch.full((nq, nb), -7, dtype=torch.int32, device="cuda")
            lg = torch.zeros((nq, L), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            idx.mlp_topk_device(qt, nb, bo, lg)
            torch.cuda.synchronize()
            assert np.array_equal(bo.cpu().numpy(), order32) and np.array_equal(bits(lg.cpu().numpy()), bits(logits32))
            assert torch.equal(qt, keep)
        with pytest.raises(capi.LmiError, match="lmi_mlp_topk_f16: nq < 0"):
            capi._check(capi.lib().lmi_mlp_topk_f16(idx._h, q16.ctypes.data, -1, nb, order16.ctypes.data, None, 0))
    finally:
        idx.close()


def test_predict_keeps_halves(capi, monkeypatch):
    """NeuralNetwork.predict on float16 arrays and tensors: the chunks reach the library as float16, the classes are those of the
    widened rows."""
    from learnedmetricindex_amd.li.model import NeuralNetwork

    torch.manual_seed(7)
    net = NeuralNetwork(input_dim=40, output_dim=9, model_type="MLP")
    x16 = np.random.RandomState(8).randn(700, 40).astype(np.float16)
    want = net.predict(x16.astype(np.float32))
    seen = []
    host, device = capi.Index.mlp_topk, capi.Index.mlp_topk_device
    monkeypatch.setattr(capi.Index, "mlp_topk", lambda self, q, *a, **k: (seen.append(str(q.dtype)), host(self, q, *a, **k))[1])
    monkeypatch.setattr(capi.Index, "mlp_topk_device", lambda self, q, *a, **k: (seen.append(str(q.dtype)), device(self, q, *a, **k))[1])
    monkeypatch.setattr(NeuralNetwork, "_CHUNK", 256)   # three chunks, the last one ragged
    assert np.array_equal(net.predict(x16), want)
    assert np.array_equal(net.predict(torch.from_numpy(x16)), want)
    assert np.array_equal(net.predict(torch.from_numpy(x16).cuda()), want)
    assert seen == ["float16"] * 6 + ["torch.float16"] * 3


# ---- the builder --------------------------------------------------------------------------------------------------------------------
def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


@pytest.fixture(scope="module")
def mixture16():
    X, _ = synth.mixture(2023, 5000, 64, 12, 200)   # test_gpu_train.py's builder shape
    X16 = X.astype(np.float16)
    X16.setflags(write=False)
    return X16


def build(df, ncat):
    from learnedmetricindex_amd.li.BuildConfiguration import BuildConfiguration
    from learnedmetricindex_amd.li.clustering import algorithms
    from learnedmetricindex_amd.li.LearnedIndexBuilder import LearnedIndexBuilder

    torch.manual_seed(2023)   # the initial weights are torch's
    cfg = BuildConfiguration([algorithms["hip_kmeans"]] * len(ncat), [20] * len(ncat), ["MLP"] * len(ncat), [0.01] * len(ncat), ncat)
    return LearnedIndexBuilder(df, cfg, trainer="hip").build()


@pytest.mark.parametrize("ncat", [[12], [4, 3]])
def test_builder_on_a_float16_frame_equals_the_widened_frame(capi, monkeypatch, mixture16, ncat):
    from learnedmetricindex_amd.li.model import NeuralNetwork, linear_layers

    seen = {"kmeans": [], "train": [], "predict": []}
    kmeans, train, predict = capi.kmeans, capi.train, NeuralNetwork.predict

    def dtype_of(x):
        return str(x.dtype).replace("torch.", "")

    monkeypatch.setattr(capi, "kmeans", lambda x, *a, **k: (seen["kmeans"].append(dtype_of(x)), kmeans(x, *a, **k))[1])
    monkeypatch.setattr(capi, "train", lambda x, *a, **k: (seen["train"].append(dtype_of(x)), train(x, *a, **k))[1])
    monkeypatch.setattr(NeuralNetwork, "predict", lambda self, x: (seen["predict"].append(dtype_of(x)), predict(self, x))[1])

    df16 = frame(np.array(mixture16))
    assert (df16.dtypes == np.float16).all()
    li16, dp16, nb16, _, _ = build(df16, ncat)
    n_models = 1 if len(ncat) == 1 else 1 + ncat[0]
    for what, calls in seen.items():   # float16 arrived, at every node
        assert len(calls) >= n_models and set(calls) == {"float16"}, (what, calls)
    calls16 = {what: len(calls) for what, calls in seen.items()}
    for calls in seen.values():
        calls.clear()
    li32, dp32, nb32, _, _ = build(frame(mixture16.astype(np.float32)), ncat)
    for what, calls in seen.items():   # the widened frame takes the float path, call for call
        assert len(calls) == calls16[what] and set(calls) == {"float32"}, (what, calls)

    assert dp16.shape == (5000, len(ncat)) and dp16.dtype == np.int64
    assert np.array_equal(dp16, dp32) and nb16 == nb32 and li16.bucket_paths == li32.bucket_paths
    assert list(li16.internal_models) == list(li32.internal_models) and len(li16.internal_models) == n_models - 1
    for m16, m32 in zip([li16.root_model] + list(li16.internal_models.values()), [li32.root_model] + list(li32.internal_models.values())):
        for (W1, b1), (W2, b2) in zip(linear_layers(m16.model), linear_layers(m32.model)):
            assert np.array_equal(bits(W1), bits(W2)) and np.array_equal(bits(b1), bits(b2))
        assert m16._hip_state[1] == m32._hip_state[1] >= 20
    assert len(np.unique(dp16[:, 0])) == ncat[0]
    li16.close()
    li32.close()


def test_another_clusterer_gets_float32_per_node(capi, mixture16):
    """A clusterer other than hip_kmeans gets what it gets from a float32 frame: the node's rows widened."""
    from learnedmetricindex_amd.li.BuildConfiguration import BuildConfiguration
    from learnedmetricindex_amd.li.clustering import algorithms
    from learnedmetricindex_amd.li.LearnedIndexBuilder import LearnedIndexBuilder

    seen = []

    def mine(data, n_clusters, parameters):
        seen.append((data.dtype, data.shape))
        return algorithms["hip_kmeans"](data, n_clusters, parameters)

    torch.manual_seed(2023)
    cfg = BuildConfiguration([mine], [20], ["MLP"], [0.01], [12])
    li, dp, n_buckets, _, _ = LearnedIndexBuilder(frame(np.array(mixture16)), cfg, trainer="hip").build()
    assert seen == [(np.dtype(np.float32), (5000, 64))] and n_buckets == 12
    li.close()
