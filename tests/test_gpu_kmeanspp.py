"""GPU (`-m gpu`): `lmi_kmeans_seed` -- greedy k-means++ seeding on the device -- against its numpy restatement
(tests/kmeanspp_ref.py, on top of the unchanged oracle's `knn_l2`).  Every comparison is exact: centroids as uint32 bit patterns,
rows and potential with array_equal.  d: element loads (45), 16-byte loads over two chunks (64), a partial last chunk (136); n: one
row past a wave's 64, one past a scan block, several blocks with a ragged end; (k, n_trials): round 0 alone, plain k-means++, L = 5,
a full candidate tile."""
import numpy as np
import pytest
import torch

import kmeanspp_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want):
    c, rows, pot = got
    wc, wr, wp = want
    assert np.array_equal(rows, wr), (rows, wr)
    assert np.array_equal(pot, wp), (pot, wp)
    assert np.array_equal(bits(c), bits(wc))


@pytest.mark.parametrize("k,n_trials", [(1, 0), (2, 1), (33, 0), (8, 32)])
@pytest.mark.parametrize("n", [65, 1025, 2500])
@pytest.mark.parametrize("d", [45, 64, 136])
def test_parity_with_the_restatement(capi, d, n, k, n_trials):
    x, *want = kmeanspp_ref.case(n, d, k, n_trials)
    assert_same(capi.kmeans_seed(x, k, n_trials=n_trials), want)


def test_more_rows_than_one_sweep_of_the_grid(capi):   # 2 blocks per CU x 256 rows x 256 CUs: a wave walks 3 row blocks, the last ragged
    x, *want = kmeanspp_ref.case(2 * 131072 + 77, 16, 3, 2)
    assert_same(capi.kmeans_seed(x, 3, n_trials=2), want)


def test_k_equal_n_chooses_every_row_once(capi):
    rs = np.random.RandomState(3)
    x = rs.randn(65, 45).astype(np.float32)   # distinct rows: a chosen row has weight 0 and is not drawn again
    c, rows, pot = capi.kmeans_seed(x, 65, n_trials=2)
    assert sorted(rows.tolist()) == list(range(65)) and pot[-1] == 0
    assert np.array_equal(bits(c), bits(x[rows]))


def test_all_rows_equal_takes_the_t0_rule(capi, oracle):
    x = np.tile(np.random.RandomState(4).randn(1, 45).astype(np.float32), (65, 1))
    got = capi.kmeans_seed(x, 3, n_trials=4)
    assert_same(got, kmeanspp_ref.seed_ref(oracle, x, 3, 4))
    assert not got[2].any() and got[1].tolist() == [kmeanspp_ref.mulhi(kmeanspp_ref.draw(2023, t, 0), 65) for t in range(3)]


@pytest.mark.parametrize("d", [45, 64])
def test_float16_equals_the_widened_array(capi, d):
    x16 = kmeanspp_ref.data(1025, d).astype(np.float16)
    got, want = capi.kmeans_seed(x16, 8), capi.kmeans_seed(x16.astype(np.float32), 8)
    assert_same(got, want)
    got_t = capi.kmeans_seed(torch.from_numpy(x16).cuda(), 8)
    assert_same((got_t[0].cpu().numpy(),) + got_t[1:], want)


def test_device_tensors_equal_host_arrays_run_after_run(capi):
    x, *want = kmeanspp_ref.case(2500, 64, 33, 0)
    xt = torch.from_numpy(np.array(x)).cuda()
    keep = xt.clone()
    for _ in range(2):
        c, rows, pot = capi.kmeans_seed(xt, 33)
        assert c.is_cuda and c.dtype == torch.float32
        assert_same((c.cpu().numpy(), rows, pot), want)
    assert torch.equal(xt, keep)


def test_kmeans_with_init_kmeanspp_is_the_two_calls_chained(capi):
    x = kmeanspp_ref.case(2500, 64, 33, 0)[0]
    for arg in (x, torch.from_numpy(np.array(x)).cuda()):
        seeded = capi.kmeans_seed(arg, 33, n_trials=3, seed=7)[0]
        want = capi.kmeans(arg, 33, niter=4, init=seeded)
        got = capi.kmeans(arg, 33, niter=4, init="k-means++", n_trials=3, seed=7)
        for g, w in zip(got, want):
            g, w = (a.cpu().numpy() if hasattr(a, "cpu") else a for a in (g, w))
            assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


REFUSALS = {
    "k_gt_n": (dict(k=41), "k 41 exceeds n 40"),
    "n_trials_33": (dict(n_trials=33), "n_trials 33 outside"),
    "nan_x": (dict(poke=np.nan), "x holds a value that is not finite"),
    "null_x": (dict(null="x"), "x and centroids must not be NULL"),
    "null_centroids": (dict(null="centroids"), "x and centroids must not be NULL"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_condition_and_write_nothing(capi, name):
    spec, message = REFUSALS[name]
    k = spec.get("k", 3)
    x = np.random.RandomState(5).randn(40, 12).astype(np.float32)
    if "poke" in spec:
        x[17, 5] = spec["poke"]
    c, rows, pot = np.full((k, 12), 7.0, np.float32), np.full(k, 78, np.int64), np.full(k, 79, np.int64)
    ptr = {"x": x.ctypes.data, "centroids": c.ctypes.data}
    ptr[spec.get("null", "")] = None
    with pytest.raises(capi.LmiError, match=message):
        capi._check(capi.lib().lmi_kmeans_seed(0, ptr["x"], 40, 12, k, spec.get("n_trials", 0), 2023, ptr["centroids"],
                                               rows.ctypes.data, pot.ctypes.data, 0))
    assert (c == 7.0).all() and (rows == 78).all() and (pot == 79).all()
