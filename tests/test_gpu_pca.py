"""GPU (`-m gpu`): `lmi_gram` / `lmi_project` -- the PCA pair on the device -- against their numpy restatement (tests/pca_ref.py, on top
of the unchanged oracle's `dot`).  Parity is exact: mean and y as uint32 bit patterns, gram as uint64.  n covers the piece seams
(4096 rows), d the tile seams (64, 128), the 16-byte and the element loads; m the basis tiles (32) and both store forms.
The values run from exponent -67 to 56 (pca_ref.VALUES), the bases are aligned and not, a host x comes in one and in two pieces."""
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


GEOMETRIES = [(0, 0), (64, 1), (128, 1), (64, 1 << 14), (128, 2)]


@pytest.mark.parametrize("n,d", pca_ref.GRAM_VALUE_SHAPES)
@pytest.mark.parametrize("name", pca_ref.GRAM_VALUE_NAMES)
def test_gram_values(capi, name, n, d):
    """Exponents from -67 to 56, subnormal products, full binary32 mantissas, degenerate columns (tests/pca_ref.py's VALUES)."""
    x, mean, g, e = pca_ref.gram_values_case(name, n, d)
    assert e == pca_ref.VALUES[name][1]
    for tile_cols, ppb in [(0, 0), (64, 1), (128, 2)]:
        capi.gram_set_geometry(tile_cols, ppb)
        assert_gram(capi.gram(x), mean, g)
        plan = capi.gram_last_plan()
        assert plan["EXPONENT"] == e and plan["PIECES"] == 2 and tile_cols in (0, plan["TILE_COLS"]) and plan["VEC"] == (d % 4 == 0)
    capi.gram_set_geometry(0, 0)
    mt, gt = capi.gram(torch.from_numpy(np.array(x)).cuda())
    assert capi.gram_last_plan()["EXPONENT"] == e
    assert_gram((mt.cpu().numpy(), gt.cpu().numpy()), mean, g)
    if name == "down70":
        assert np.asarray(capi.gram(x)[1]).all()   # no product was flushed
    if name == "halves_only":   # lmi_gram_f16 on the halves themselves: the result of the widened array
        x16 = x.astype(np.float16)
        assert np.array_equal(b32(x16.astype(np.float32)), b32(x))
        for xs in (x16, torch.from_numpy(x16).cuda()):
            got = capi.gram(xs)
            assert capi.gram_last_plan()["EXPONENT"] == e and capi.gram_last_plan()["VEC"] == 0
            assert_gram(got if xs is x16 else (got[0].cpu().numpy(), got[1].cpu().numpy()), mean, g)


def test_gram_five_tiles_a_side(capi):
    """d = 257: 15 tiles at tile 64; at tile 128 three a side, the last holding one real column."""
    n, d = 4100, 257
    x, mean, g, e = pca_ref.gram_case(n, d)
    for tile_cols, ppb in GEOMETRIES:
        capi.gram_set_geometry(tile_cols, ppb)
        assert_gram(capi.gram(x), mean, g)
        plan = capi.gram_last_plan()
        assert plan["PIECES"] == 2 and plan["EXPONENT"] == e and plan["VEC"] == 0
        assert tile_cols in (0, plan["TILE_COLS"]) and plan["RUNS"] == -(-plan["PIECES"] // plan["PIECES_PER_BLOCK"])
        assert plan["TILES"] == {64: 15, 128: 6}[plan["TILE_COLS"]]
    capi.gram_set_geometry(0, 0)


def off_by_one(a):
    """A device copy of `a` that starts one element past an aligned base."""
    flat = torch.empty(a.size + 8, dtype={2: torch.float16, 4: torch.float32}[a.itemsize], device="cuda")
    view = flat[1:1 + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(np.array(a)))
    assert view.is_contiguous() and flat.data_ptr() % 16 == 0 and view.data_ptr() - flat.data_ptr() == a.itemsize
    return view


@pytest.mark.parametrize("d,halves", [(44, False), (48, True)])
def test_gram_from_a_misaligned_base(capi, d, halves):
    """d admits 16-byte loads, the base does not: element loads, the same bits."""
    x, mean, g, _ = pca_ref.gram_case(4100, d)
    xs = x.astype(np.float16) if halves else x
    mt, gt = capi.gram(torch.from_numpy(np.array(xs)).cuda())
    assert capi.gram_last_plan()["VEC"] == 1
    assert_gram((mt.cpu().numpy(), gt.cpu().numpy()), mean, g)
    for tile_cols in (64, 128):
        capi.gram_set_geometry(tile_cols, 1)
        mt, gt = capi.gram(off_by_one(xs))
        assert capi.gram_last_plan()["VEC"] == 0
        assert_gram((mt.cpu().numpy(), gt.cpu().numpy()), mean, g)
    capi.gram_set_geometry(0, 0)


def test_gram_halves_where_only_binary32_is_vectorised(capi):
    """d = 44: d % 4 == 0 and d % 8 == 4."""
    x, mean, g, _ = pca_ref.gram_case(4100, 44)
    x16 = x.astype(np.float16)
    for xs, vec in [(x, 1), (x16, 0), (torch.from_numpy(np.array(x)).cuda(), 1), (torch.from_numpy(x16).cuda(), 0)]:
        got = capi.gram(xs)
        assert capi.gram_last_plan()["VEC"] == vec
        assert_gram(got if isinstance(xs, np.ndarray) else (got[0].cpu().numpy(), got[1].cpu().numpy()), mean, g)


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


#: two rows of basis-tile groups (the last with three clamped tiles, then whole); m at and below its bound; the longest chain with
#: 16-byte and with element loads (32 KB of mean in LDS); the 256-row workgroup seam from both sides; the 64-row wave seam
PROJECT_SEAMS = [(70, 40, 129), (70, 40, 160), (40, 8, 1024), (40, 8, 1023), (70, 4096, 33), (70, 4095, 32), (255, 12, 4), (256, 12, 4),
                 (257, 12, 4), (64, 12, 5)]


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("n,d,m", PROJECT_CASES + PROJECT_SEAMS)
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


@pytest.mark.parametrize("n,m,halves", [(4096 + 257, 4, False), (8192 + 257, 3, True)])
def test_project_host_rows_in_two_pieces(capi, n, m, halves):
    """d = 4096: a 64 MiB piece is 4096 rows of binary32, 8192 of halves.  The host call (two uploads, two launches, two copies back)
    against the device call on the same data (one launch), all of y; the restatement at both ends and around the seam."""
    d, piece = 4096, 8192 if halves else 4096
    x, basis, mean, at, y = pca_ref.project_pieces_case(n, d, m, piece)
    xs = x.astype(np.float16) if halves else x
    got = capi.project(xs, basis, mean=mean)
    assert got.shape == (n, m) and np.array_equal(b32(got[at]), b32(y)), int((b32(got[at]) != b32(y)).sum())
    whole = capi.project(torch.from_numpy(np.array(xs)).cuda(), np.array(basis), mean=np.array(mean)).cpu().numpy()
    assert np.array_equal(b32(got), b32(whole)), int((b32(got) != b32(whole)).sum())


def device_project(capi, x, basis, mean, y):
    """lmi_project through the C ABI on device tensors as they lie (x float32)."""
    n, d = x.shape
    capi._check(capi.lib().lmi_project(0, x.data_ptr(), n, d, None if mean is None else mean.data_ptr(), basis.data_ptr(), basis.shape[0],
                                       y.data_ptr(), 1))
    torch.cuda.synchronize()


@pytest.mark.parametrize("centred", [False, True])
def test_project_misaligned_y_and_x(capi, centred):
    """m = 8 into a y four bytes past an aligned base: 4-byte stores, nothing written before or behind it.  d = 44 from an x one
    element past an aligned base: element loads.  The same bits either way."""
    n, d, m = 300, 44, 8
    x, basis, mean, y = pca_ref.project_case(n, d, m, centred)
    xt, bt = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(basis).cuda()
    mt = None if mean is None else torch.from_numpy(mean).cuda()
    flat = torch.full((n * m + 8,), 79.0, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    device_project(capi, xt, bt, mt, flat[1:])
    got = flat.cpu().numpy()
    assert np.array_equal(b32(got[1:1 + n * m].reshape(n, m)), b32(y)) and got[0] == 79 and (got[1 + n * m:] == 79).all()
    yt = torch.empty((n, m), dtype=torch.float32, device="cuda")
    device_project(capi, off_by_one(x), bt, mt, yt)
    assert np.array_equal(b32(yt.cpu().numpy()), b32(y))


def assert_bits_but_nan(got, want):
    """Exact, but for the payload and sign of a NaN: the CPU's fmaf and the MFMA may differ there."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), int((np.isnan(got) != nan).sum())
    assert np.array_equal(b32(got)[~nan], b32(want)[~nan]), int((b32(got)[~nan] != b32(want)[~nan]).sum())


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("name", sorted(set(pca_ref.PROJECT_VALUES) - {"clean"}))
def test_project_values(capi, name, centred):
    """Full mantissas, tiny rows, -0.0, a zero basis row; NaN and +inf do what the chain does with them, in their own rows only."""
    x, basis, mean, y = pca_ref.project_values_case(name, centred)
    forms = [x, torch.from_numpy(np.array(x)).cuda()]
    x16 = x.astype(np.float16)
    if np.array_equal(b32(x16.astype(np.float32)), b32(x)):
        forms += [x16, torch.from_numpy(x16).cuda()]
    assert len(forms) == (2 if name in ("full_mantissa", "down70") else 4)
    for xs in forms:
        got = capi.project(xs, np.array(basis), mean=mean)
        got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
        assert_bits_but_nan(got, y)
        if name == "nonfinite":
            clean = pca_ref.project_values_case("clean", centred)[3]
            others = np.setdiff1d(np.arange(x.shape[0]), pca_ref.NONFINITE_ROWS)
            assert np.array_equal(b32(got[others]), b32(clean[others]))


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
