"""GPU (`-m gpu`): `lmi_kmeans` -- Lloyd's k-means on the device -- against its numpy restatement (tests/kmeans_ref.py, on top of
the unchanged oracle's `knn_l2`).  Every comparison is exact: centroids as uint32 bit patterns, labels, counts and `changed` with
array_equal.  The six parity cases cover odd d, d > 768 that is no multiple of 32, k below a tile, one past a tile and over several
tiles -- and with d a multiple of 4 (16-byte row loads) one tile, two and several -- ragged n, exact ties, duplicate rows, empty
clusters and the early stop (test_kmeans_host.py pins that they do)."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import kmeans_ref
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want):
    c, labels, counts, changed = got
    wc, wl, wn, wch = want
    assert c.dtype == np.float32 and labels.dtype == np.int32 and counts.dtype == np.int64 and changed.dtype == np.int64
    assert np.array_equal(changed, wch), (changed, wch)
    assert np.array_equal(labels, wl), int((labels != wl).sum())
    assert np.array_equal(counts, wn)
    assert np.array_equal(bits(c), bits(wc)), int((bits(c) != bits(wc)).sum())


@pytest.mark.parametrize("key", sorted(kmeans_ref.CASES))
def test_parity_with_the_reference(capi, key):
    x, c0, *want = kmeans_ref.case(*key)
    assert_same(capi.kmeans(x, key[2], niter=kmeans_ref.NITER, init=c0), want)


def test_niter_0_assigns_to_the_initial_centroids(capi, oracle):
    x, c0 = kmeans_ref.case(3001, 45, 7, 1)[:2]
    c, labels, counts, changed = capi.kmeans(x, 7, niter=0, init=c0)
    assert np.array_equal(bits(c), bits(c0))
    assert np.array_equal(labels, oracle.knn_l2(x, c0, k=1, nthreads=4)[1][:, 0])
    assert changed.tolist() == [3001] and np.array_equal(counts, np.bincount(labels, minlength=7))


@pytest.mark.parametrize("key", [(4099, 33, 33, 3), (600, 768, 257, 4)])
def test_device_tensors_equal_the_host_call(capi, key):
    x, c0, *want = kmeans_ref.case(*key)
    xt = torch.from_numpy(np.array(x)).cuda()
    keep = xt.clone()
    runs = [capi.kmeans(xt, key[2], niter=kmeans_ref.NITER, init=c0) for _ in range(2)]
    for c, labels, counts, changed in runs:
        assert c.is_cuda and labels.is_cuda and c.dtype == torch.float32 and labels.dtype == torch.int32
        assert_same((c.cpu().numpy(), labels.cpu().numpy(), counts, changed), want)
    assert torch.equal(xt, keep)


def test_default_init_is_the_seeded_choice_of_rows(capi, oracle):
    x = kmeans_ref.case(4099, 33, 33, 3)[0]
    c0 = x[np.random.RandomState(2023).choice(4099, 33, replace=False)]
    assert_same(capi.kmeans(x, 33, niter=2), kmeans_ref.kmeans_ref(oracle, x, c0, 2))


MAGNITUDES = ["down20", "up10", "column", "max1", "zero"]


def magnitude_case(name):
    if name == "zero":
        return np.zeros((64, 8), np.float32), np.zeros((2, 8), np.float32), 2
    if name == "max1":   # max|x| is exactly 1.0: e = 1
        rs = np.random.RandomState(11)
        x = rs.uniform(-1, 1, (300, 16)).astype(np.float32)
        x[7, 3] = 1.0
        assert np.abs(x).max() == 1.0 and kmeans_ref.exponent(x) == 1
        return x, x[:5].copy(), 2
    x, c0 = (np.array(a) for a in kmeans_ref.case(4099, 33, 33, 3)[:2])
    if name == "column":   # one column so small that it quantises to 0
        x[:, 5] *= np.float32(2.0 ** -40)
        c0[:, 5] *= np.float32(2.0 ** -40)
        assert not np.rint(x[:, 5].astype(np.float64) * 2.0 ** (36 - kmeans_ref.exponent(x))).any()
    else:
        s = np.float32(2.0 ** (-20 if name == "down20" else 10))
        x, c0 = x * s, c0 * s
    return x, c0, 2


@pytest.mark.parametrize("name", MAGNITUDES)
def test_magnitudes(capi, oracle, name):
    x, c0, niter = magnitude_case(name)
    got = capi.kmeans(x, c0.shape[0], niter=niter, init=c0)
    assert_same(got, kmeans_ref.kmeans_ref(oracle, x, c0, niter))
    if name == "zero":
        assert not got[1].any() and got[2].tolist() == [64, 0]


def raw_call(capi, x, k, niter, c, labels, counts, changed, d=None, n=None):
    n = x.shape[0] if n is None else n
    d = x.shape[1] if d is None else d
    rc = capi.lib().lmi_kmeans(0, x.ctypes.data, n, d, k, niter, c.ctypes.data, labels.ctypes.data, counts.ctypes.data,
                               changed.ctypes.data, 0)
    capi._check(rc)


REFUSALS = {
    "nan_x": (dict(poke_x=np.nan), "x holds a value that is not finite"),
    "inf_x": (dict(poke_x=np.inf), "x holds a value that is not finite"),
    "nan_init": (dict(poke_c=np.nan), "initial centroids hold a value that is not finite"),
    "k_gt_n": (dict(k=41), "k 41 exceeds n 40"),
    "k_0": (dict(k=0), "k 0 outside"),
    "d_4097": (dict(d=4097), "d 4097 outside"),
    "niter_1001": (dict(niter=1001), "niter 1001 outside"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_condition_and_write_nothing(capi, name):
    spec, message = REFUSALS[name]
    n, d, k, niter = 40, spec.get("d", 12), spec.get("k", 3), spec.get("niter", 2)
    rs = np.random.RandomState(5)
    x = rs.randn(n, d).astype(np.float32)
    kk = max(k, 1)
    c = x[:min(kk, n)].copy() if kk <= n else np.zeros((kk, d), np.float32)
    if "poke_x" in spec:
        x[17, 5] = spec["poke_x"]
    if "poke_c" in spec:
        c[1, 2] = spec["poke_c"]
    labels = np.full(n, 77, np.int32)
    counts = np.full(kk, 78, np.int64)
    changed = np.full(1002, 79, np.int64)
    c_before = c.copy()
    with pytest.raises(capi.LmiError, match=message):
        raw_call(capi, x, k, niter, c, labels, counts, changed)
    assert np.array_equal(bits(c), bits(c_before))
    assert (labels == 77).all() and (counts == 78).all() and (changed == 79).all()


def test_builder_with_hip_kmeans(capi):
    from learnedmetricindex_amd.li.BuildConfiguration import BuildConfiguration
    from learnedmetricindex_amd.li.clustering import algorithms
    from learnedmetricindex_amd.li.LearnedIndexBuilder import LearnedIndexBuilder

    torch.manual_seed(2023)
    X, _ = synth.mixture(2023, 3000, 32, 8, 10)
    df = pd.DataFrame(X)
    df.index += 1
    obj, labels = algorithms["hip_kmeans"](X, 8, None)
    assert labels.dtype == np.int32 and labels.shape == (3000,) and obj.centroids.shape == (8, 32)
    assert obj.counts.sum() == 3000 and obj.changed.shape == (21,) and obj.changed[0] == 3000
    cfg = BuildConfiguration([algorithms["hip_kmeans"]], [20], ["MLP"], [0.01], [8])
    li, dp, n_buckets, _, _ = LearnedIndexBuilder(df, cfg).build()
    assert n_buckets == 8 and dp.shape == (3000, 1)
    assert ((dp >= 0) & (dp < 8)).all()
    li.close()
