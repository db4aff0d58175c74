"""Host side of the index build on binary16 rows (no GPU): the narrowed k-means cases of tests/kmeans_f16_cases.py keep what they
were chosen for, on the oracle; `_capi.kmeans` / `_capi.train` take float16 and refuse bad arguments before they load the library;
the three new entry points are bound (test_capi_exports.py then checks that the library exports them)."""
import numpy as np
import pytest

import kmeans_f16_cases as cases
import kmeans_ref


@pytest.mark.parametrize("key", sorted(cases.CASES))
def test_narrowed_cases_cover_what_they_claim(oracle, key):
    empty, fixed, subnormal = cases.CASES[key]
    n, d, k, _ = key
    x16, x, c0, c, labels, counts, changed = cases.case(*key)
    assert x16.dtype == np.float16 and x16.shape == (n, d) and x.dtype == np.float32 and c0.dtype == np.float32
    assert np.array_equal(x16.astype(np.float32), x) and np.isfinite(x).all()            # x is x16 widened, nothing else
    assert np.array_equal(c0.astype(np.float16).astype(np.float32), c0)                  # c0 = widened rows
    assert np.array_equal(c0[0], c0[1])                                                  # two equal initial centroids
    assert (x[5:9] == x[4]).all()                                                        # duplicate rows
    assert cases.subnormals(x16) == subnormal
    assert counts.sum() == n and changed[0] == n
    assert int((counts == 0).sum()) == empty
    if fixed is None:
        assert (changed > 0).all()
    else:
        assert changed[fixed] == 0 and (changed[1:fixed] > 0).all() and not changed[fixed:].any()
    assert np.array_equal(labels, kmeans_ref.assign(oracle, x, c))


def test_the_cases_are_the_float_form_s_six_and_two_of_the_half_form_s_own():
    assert set(kmeans_ref.CASES) < set(cases.CASES) and len(cases.CASES) == len(kmeans_ref.CASES) + 2
    for key, (empty, fixed) in kmeans_ref.CASES.items():   # narrowing moved neither the empty clusters nor the fixed point
        assert cases.CASES[key][:2] == (empty, fixed)
        assert cases.CASES[key][2] >= 21                   # and every one of them holds binary16 subnormals
    ds = sorted(key[1] for key in set(cases.CASES) - set(kmeans_ref.CASES))
    assert ds == [8, 44] and 44 % 4 == 0 and 44 % 8 != 0


def test_the_three_calls_are_bound():
    from learnedmetricindex_amd import _capi

    for name in ("lmi_kmeans", "lmi_train", "lmi_mlp_topk"):
        assert _capi.SIGNATURES[name + "_f16"] == _capi.SIGNATURES[name]   # the pointers are void*: the same prototype


@pytest.fixture
def no_lib(monkeypatch):
    from learnedmetricindex_amd import _capi

    def refuse():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", refuse)
    return _capi


def test_kmeans_refuses_bad_arguments_without_loading_the_library(no_lib):
    x16 = np.zeros((10, 4), dtype=np.float16)
    with pytest.raises(ValueError, match="k 11"):
        no_lib.kmeans(x16, 11)
    with pytest.raises(ValueError, match="k 0"):
        no_lib.kmeans(x16, 0)
    with pytest.raises(ValueError, match="niter -1"):
        no_lib.kmeans(x16, 2, niter=-1)
    with pytest.raises(ValueError, match="init must be float32"):   # a given init stays float32, also beside float16 rows
        no_lib.kmeans(x16, 2, init=np.zeros((2, 4), dtype=np.float16))
    with pytest.raises(ValueError, match="init"):
        no_lib.kmeans(x16, 2, init=np.zeros((2, 5), dtype=np.float32))
    with pytest.raises(ValueError, match=r"\[n,d\]"):
        no_lib.kmeans(np.zeros(10, dtype=np.float16), 2)
    with pytest.raises(ValueError, match="float32"):   # what is neither float16 nor float32 is told the default
        no_lib.kmeans(np.zeros((10, 4), dtype=np.float64), 2)


def test_train_refuses_bad_arguments_without_loading_the_library(no_lib):
    import torch

    x16 = np.zeros((10, 4), dtype=np.float16)
    labels = np.zeros(10, dtype=np.int32)
    layers = [(np.zeros((3, 4), np.float32), np.zeros(3, np.float32))]
    rows = np.zeros((2, 2), dtype=np.int64)
    with pytest.raises(ValueError, match="both be numpy arrays or both be tensors"):   # labels of the other pointer kind
        no_lib.train(x16, torch.zeros(10, dtype=torch.int32), layers, rows, 0.01)
    with pytest.raises(ValueError, match="both be numpy arrays or both be tensors"):
        no_lib.train(torch.zeros((10, 4), dtype=torch.float16), labels, layers, rows, 0.01)
    with pytest.raises(ValueError, match="labels must be int32"):
        no_lib.train(x16, labels.astype(np.int64), layers, rows, 0.01)
    with pytest.raises(ValueError, match=r"labels must be \[10\]"):
        no_lib.train(x16, labels[:9], layers, rows, 0.01)
    with pytest.raises(ValueError, match="layer 0 must be"):
        no_lib.train(x16, labels, [(np.zeros((3, 5), np.float32), np.zeros(3, np.float32))], rows, 0.01)
    with pytest.raises(ValueError, match="batch_rows"):
        no_lib.train(x16, labels, layers, np.zeros(4, dtype=np.int64), 0.01)
    with pytest.raises(ValueError, match="lr"):
        no_lib.train(x16, labels, layers, rows, float("nan"))
    with pytest.raises(ValueError, match="contiguous tensors on the device"):   # a float16 tensor that is not on the device
        no_lib.train(torch.zeros((10, 4), dtype=torch.float16), torch.zeros(10, dtype=torch.int32), layers, rows, 0.01)
    with pytest.raises(ValueError, match="x must be float32"):
        no_lib.train(x16.astype(np.float64), labels, layers, rows, 0.01)


def test_hip_kmeans_passes_a_float16_array_on_as_it_is(monkeypatch):
    from learnedmetricindex_amd import _capi
    from learnedmetricindex_amd.li.clustering import algorithms

    seen = []

    def fake(x, k, niter=20, seed=2023):
        seen.append((x.dtype, x.flags["C_CONTIGUOUS"]))
        return np.zeros((k, x.shape[1]), np.float32), np.zeros(x.shape[0], np.int32), np.zeros(k, np.int64), np.zeros(niter + 1, np.int64)

    monkeypatch.setattr(_capi, "kmeans", fake)
    x16 = np.zeros((12, 6), dtype=np.float16)
    algorithms["hip_kmeans"](x16, 3, None)
    algorithms["hip_kmeans"](x16.T, 3, None)
    algorithms["hip_kmeans"](x16.astype(np.float64), 3, None)
    assert seen == [(np.dtype(np.float16), True), (np.dtype(np.float16), True), (np.dtype(np.float32), True)]
