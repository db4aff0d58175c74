"""GPU (`-m gpu`): `lmi_gram` / `lmi_project` -- the PCA pair on the device -- against their numpy restatement (tests/pca_ref.py, on top
of the unchanged oracle's `dot`).  Parity is exact: mean and y as uint32 bit patterns, gram as uint64.  n covers the piece seams
(4096 rows), d the tile seams (64, 128), the 16-byte and the element loads; m the basis tiles (32) and both store forms."""
import numpy as np
import pytest
import torch

import kmeans_ref
import pca_ref

pytestmark = pytest.mark.gpu

GRAM_CASES = [(1, 33), (4095, 1), (4096, 45), (4097, 31), (4097, 96), (8197, 130)]
PROJECT_CASES = [(1, 45, 1), (63, 64, 32), (65, 136, 33), (300, 45, 96), (300, 64, 33), (65, 136, 96)]


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    yield _capi
    _capi.gram_set_geometry(0, 0)


def b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_gram(got, mean, g):
    assert got[0].dtype == np.float32 and got[1].dtype == np.float64
    assert np.array_equal(b32(got[0]), b32(mean)), int((b32(got[0]) != b32(mean)).sum())
    assert np.array_equal(b64(got[1]), b64(g)), int((b64(got[1]) != b64(g)).sum())


@pytest.mark.parametrize("n,d", GRAM_CASES)
def test_gram_parity_on_every_geometry(capi, n, d):
    x, mean, g, e = pca_ref.gram_case(n, d)
    for tile_cols, ppb in [(0, 0), (64, 1), (128, 1), (64, 1 << 14), (128, 2)]:
        capi.gram_set_geometry(tile_cols, ppb)
        assert_gram(capi.gram(x), mean, g)
        plan = capi.gram_last_plan()
        assert plan["PIECES"] == -(-n // 4096) and plan["EXPONENT"] == e and plan["VEC"] == (d % 4 == 0)
        assert tile_cols in (0, plan["TILE_COLS"]) and plan["RUNS"] == -(-plan["PIECES"] // plan["PIECES_PER_BLOCK"])
    capi.gram_set_geometry(0, 0)


@pytest.mark.parametrize("n,d", [(4097, 96), (4097, 31), (8197, 130)])
def test_gram_halves_and_device_pointers(capi, n, d):
    x, mean, g, _ = pca_ref.gram_case(n, d)   # exactly representable in binary16
    x16 = x.astype(np.float16)
    assert np.array_equal(x16.astype(np.float32), x)
    assert_gram(capi.gram(x16), mean, g)
    for xt in (torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(x16).cuda()):
        keep = xt.clone()
        mt, gt = capi.gram(xt)
        assert mt.is_cuda and gt.is_cuda and torch.equal(xt, keep)
        assert_gram((mt.cpu().numpy(), gt.cpu().numpy()), mean, g)


def test_gram_mean_is_the_kmeans_centroid_of_one_cluster(capi):
    x, mean = pca_ref.gram_case(4097, 96)[:2]
    c = capi.kmeans(x, 1, niter=1)[0]
    assert np.array_equal(b32(c[0]), b32(mean))


def test_gram_against_float64_and_the_fit_against_weyl(capi):
    """|gram - G64| <= (4096 + 2) 2^-24 sum_i |c_a||c_b| + P 2^(2e-33) entrywise: the chain bound of a piece and the fold's quantum;
    by Weyl the fitted eigenvalues lie within the Frobenius norm of that bound of eigh(G64 / (n - 1))."""
    from learnedmetricindex_amd.projection import PcaProjection

    n, d = 8197, 130
    x, _, _, e = pca_ref.gram_case(n, d)
    mean, g = capi.gram(x)
    c = (x - mean).astype(np.float64)
    G64 = c.T @ c
    bound = (4096 + 2) * 2.0 ** -24 * (np.abs(c).T @ np.abs(c)) + -(-n // 4096) * 2.0 ** (2 * e - 33)
    err = np.abs(g - G64)
    print("max err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    p = PcaProjection.fit(x, 16)
    w = np.linalg.eigh(G64 / (n - 1))[0][::-1][:16]
    print("max eigenvalue gap", float(np.abs(p.explained_variance - w).max()), "allowed", float(np.linalg.norm(bound) / (n - 1)))
    assert np.abs(p.explained_variance - w).max() <= np.linalg.norm(bound) / (n - 1)
    assert p.basis.shape == (16, d) and p.basis.dtype == np.float32 and np.all(np.diff(p.explained_variance) <= 0)
    assert (p.basis[np.arange(16), np.abs(p.basis).argmax(axis=1)] > 0).all()
    y = p.transform(x[:300])
    assert np.array_equal(b32(y), b32(capi.project(x[:300], p.basis, mean=p.mean)))
    assert np.allclose(y, (x[:300].astype(np.float64) - p.mean) @ p.basis.astype(np.float64).T, atol=1e-3)


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("n,d,m", PROJECT_CASES)
def test_project_parity(capi, n, d, m, centred):
    x, basis, mean, y = pca_ref.project_case(n, d, m, centred)
    got = capi.project(x, basis, mean=mean)
    assert got.dtype == np.float32 and got.shape == (n, m)
    assert np.array_equal(b32(got), b32(y)), int((b32(got) != b32(y)).sum())
    x16 = x.astype(np.float16)
    assert np.array_equal(b32(capi.project(x16, basis, mean=mean)), b32(y))
    for xt in (torch.from_numpy(x).cuda(), torch.from_numpy(x16).cuda()):
        yt = capi.project(xt, torch.from_numpy(basis).cuda(), mean=mean)
        assert yt.is_cuda and np.array_equal(b32(yt.cpu().numpy()), b32(y))


REFUSALS = {
    "gram_n_0": ("gram", dict(n=0), "n 0 < 1"),
    "gram_d_4097": ("gram", dict(d=4097), "d 4097 outside"),
    "gram_nan": ("gram", dict(poke=np.nan), "not finite"),
    "gram_2_56": ("gram", dict(poke=2.0 ** 56), r"2\^56"),
    "project_n_0": ("project", dict(n=0), "n 0 outside"),
    "project_d_4097": ("project", dict(d=4097), "d 4097 outside"),
    "project_m_1025": ("project", dict(m=1025), "m 1025 outside"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_condition_and_write_nothing(capi, name):
    call, spec, message = REFUSALS[name]
    x = pca_ref.rows(40, 12, 5)
    if "poke" in spec:
        x[17, 5] = spec["poke"]
    n, d, m = spec.get("n", 40), spec.get("d", 12), spec.get("m", 3)
    basis = np.ones((max(m, 3), 12), np.float32)
    mean, g, y = np.full(12, 77, np.float32), np.full((12, 12), 78, np.float64), np.full((40, 3), 79, np.float32)
    with pytest.raises(capi.LmiError, match=message):
        if call == "gram":
            capi._check(capi.lib().lmi_gram(0, x.ctypes.data, n, d, mean.ctypes.data, g.ctypes.data, 0))
        else:
            capi._check(capi.lib().lmi_project(0, x.ctypes.data, n, d, None, basis.ctypes.data, m, y.ctypes.data, 0))
    assert (mean == 77).all() and (g == 78).all() and (y == 79).all()
    assert not any(capi.gram_last_plan().values()) or call == "project"
