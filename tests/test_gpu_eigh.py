"""GPU (`-m gpu`): `lmi_eigh` against its numpy restatement (tests/eigh_ref.py).  Parity is exact -- w and v as uint64 bit patterns,
sweeps as an integer -- on every form the size admits and both streamed tiles.  d covers 1, 2, the bye of an odd d, one and several
tiles, both sides of the resident bound; the matrices full rank, rank-deficient, with zero and repeated eigenvalues, indefinite, zero;
scaled by 2^+-900, subnormal, with an entry the scaling rounds; every branch of the rotation (eigh_ref.BRANCHES)."""
import numpy as np
import pytest
import torch

import eigh_ref
import pca_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    yield _capi
    _capi.eigh_set_geometry(0, 0)


def b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_eigh(got, w, v, sweeps):
    assert np.array_equal(b64(got[0]), b64(w)), int((b64(got[0]) != b64(w)).sum())
    assert np.array_equal(b64(got[1]), b64(v)), int((b64(got[1]) != b64(v)).sum())
    assert got[2] == sweeps


@pytest.mark.parametrize("name", sorted(eigh_ref.INPUTS))
def test_parity_on_every_form_and_tile(capi, name):
    a, w, v, sweeps = eigh_ref.case(name)
    d, RES, STR = a.shape[0], capi.EIGH_FORM_RESIDENT, capi.EIGH_FORM_STREAMED
    resident = d <= eigh_ref.RESIDENT_MAX_D
    assert sweeps == 1 or name != "zero"
    for form, tile in [(0, 0), (STR, 8), (STR, 16)] + [(RES, 0)] * resident:
        capi.eigh_set_geometry(form, tile)
        assert_eigh(capi.eigh(a), w, v, sweeps)
        plan = capi.eigh_plan()
        assert plan["RESIDENT_MAX_D"] == eigh_ref.RESIDENT_MAX_D and plan["SWEEPS"] == sweeps
        assert plan["FORM"] == (form or (RES if resident else STR)) and plan["TILE"] == (tile or (0 if plan["FORM"] == RES else 16))
        assert plan["LAUNCHES"] == (1 if plan["FORM"] == RES else (d + d % 2 - 1) * sweeps)
        assert plan["EXPONENT"] == eigh_ref.exponent(a)
        assert (plan["LDS_BYTES"], plan["GRID"]) == lds_and_grid(d, plan["TILE"])
    capi.eigh_set_geometry(0, 0)


def lds_and_grid(d, tile):
    """lmi_eigh_plan.h restated.  Resident (tile 0): A, V and the rotations of D / 2 pairs in one block.  Streamed: a tile's row and
    column rotations; one block per tile (ti <= tj) of pairs x pairs for A, one per (strip of 2 * tile rows, tile of pairs) for V."""
    D = d + d % 2
    if tile == 0:
        return 16 * d * d + 18 * D + 16, 1
    side = -(-(D // 2) // tile)
    return 64 * tile, side * (side + 1) // 2 + -(-d // (2 * tile)) * side


def test_a_tie_cut_by_index_inside_the_leading_rows(capi):
    """diag(3, -1, 3, 0, 7, -1, 3), m = 3: the rows of 7, of the 3 at index 0 and of the 3 at index 2 -- not the one at index 6."""
    a, w, v, sweeps = eigh_ref.case("diag_unsorted")
    assert w[:3].tolist() == [7.0, 3.0, 3.0] and v[:3].argmax(axis=1).tolist() == [4, 0, 2] and sweeps == 1
    for form, tile in [(0, 0), (capi.EIGH_FORM_STREAMED, 8), (capi.EIGH_FORM_STREAMED, 16), (capi.EIGH_FORM_RESIDENT, 0)]:
        capi.eigh_set_geometry(form, tile)
        assert_eigh(capi.eigh(a, 3), w[:3], v[:3], sweeps)
        wt, vt, st = capi.eigh(torch.from_numpy(np.array(a)).cuda(), 3)
        assert_eigh((wt.cpu().numpy(), vt.cpu().numpy(), st), w[:3], v[:3], sweeps)
    capi.eigh_set_geometry(0, 0)


@pytest.mark.parametrize("name", ["full_mantissa", "up40"])
def test_fit_and_transform_end_to_end_by_bits(capi, name):
    """PcaProjection.fit(solver="hip") and transform against gram_ref -> eigh_ref -> project_ref: mean, basis, explained variance
    and y, on rows with full binary32 mantissas and on rows of order 2^40."""
    from learnedmetricindex_amd.projection import PcaProjection

    n, d, m = 500, 44, 8
    x, mean, g, e = pca_ref.gram_values_case(name, n, d)
    w, v, _ = eigh_ref.eigh_ref(g, m)
    basis = v.astype(np.float32)
    from oracle import lmi_oracle

    y = pca_ref.project_ref(lmi_oracle, x, basis, mean)
    for xs in (x, torch.from_numpy(np.array(x)).cuda()):
        p = PcaProjection.fit(xs, m, solver="hip")
        assert capi.gram_last_plan()["EXPONENT"] == e and capi.eigh_plan()["EXPONENT"] == eigh_ref.exponent(g)
        assert np.array_equal(p.mean.view(np.uint32), mean.view(np.uint32)) and np.array_equal(p.basis.view(np.uint32), basis.view(np.uint32))
        assert np.array_equal(b64(p.explained_variance), b64(w / float(n - 1)))
        got = p.transform(xs)
        got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), y.view(np.uint32)), int((got.view(np.uint32) != y.view(np.uint32)).sum())


@pytest.mark.parametrize("name", ["d33", "d101"])
def test_leading_rows_device_pointers_and_an_unread_lower_triangle(capi, name):
    a, w, v, sweeps = eigh_ref.case(name)
    assert_eigh(capi.eigh(a, 5), w[:5], v[:5], sweeps)
    poked = np.array(a)
    poked[np.tril_indices(a.shape[0], -1)] = np.nan
    assert_eigh(capi.eigh(poked), w, v, sweeps)
    at = torch.from_numpy(poked).cuda()
    keep = at.clone()
    wt, vt, st = capi.eigh(at, 7)
    assert wt.is_cuda and vt.is_cuda and torch.equal(at.view(torch.int64), keep.view(torch.int64))
    assert_eigh((wt.cpu().numpy(), vt.cpu().numpy(), st), w[:7], v[:7], sweeps)


def test_fit_with_the_device_solver_and_with_lapack_as_before(capi):
    from learnedmetricindex_amd.projection import PcaProjection

    n, d, m = 500, 33, 8
    x = pca_ref.rows(n, d, 11)
    mean, g = capi.gram(x)
    w, v, _ = eigh_ref.eigh_ref(g, m)
    for xs in (x, torch.from_numpy(x).cuda()):
        p = PcaProjection.fit(xs, m, solver="hip")
        assert np.array_equal(p.basis.view(np.uint32), v.astype(np.float32).view(np.uint32)) and np.array_equal(p.mean, mean)
        assert np.array_equal(b64(p.explained_variance), b64(w / float(n - 1)))
    wl, vl = np.linalg.eigh(g / float(n - 1))   # the fit as it was before there was a solver to choose
    order = np.argsort(wl, kind="stable")[::-1][:m]
    basis = vl[:, order].T
    basis = basis * np.where(basis[np.arange(m), np.abs(basis).argmax(axis=1)] < 0, -1.0, 1.0)[:, None]
    for p in (PcaProjection.fit(x, m), PcaProjection.fit(x, m, solver="lapack")):
        assert np.array_equal(p.basis.view(np.uint32), basis.astype(np.float32).view(np.uint32))
        assert np.array_equal(b64(p.explained_variance), b64(wl[order]))


REFUSALS = {
    "d_0": (dict(d=0), "d 0 outside"),
    "d_4097": (dict(d=4097), "d 4097 outside"),
    "m_0": (dict(m=0), "m 0 outside"),
    "m_d_plus_1": (dict(m=13), "m 13 outside"),
    "nan_at_0_1": (dict(poke=np.nan), "not finite"),
    "resident_past_its_bound": (dict(name="d101", form=1), "resident form holds d <= 100"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_condition_and_write_nothing(capi, name):
    spec, message = REFUSALS[name]
    a = np.array(eigh_ref.case(spec.get("name", "degenerate"))[0])   # degenerate: d = 12
    a[0, 1] = spec.get("poke", a[0, 1])
    d = a.shape[0]
    w, v = np.full(d, 77.0), np.full((d, d), 78.0)
    capi.eigh_set_geometry(spec.get("form", 0), 0)
    with pytest.raises(capi.LmiError, match=message):
        capi._check(capi.lib().lmi_eigh(0, a.ctypes.data, spec.get("d", d), spec.get("m", d), w.ctypes.data, v.ctypes.data, None, 0))
    capi.eigh_set_geometry(0, 0)
    assert (w == 77).all() and (v == 78).all() and not any(capi.eigh_plan().values())
