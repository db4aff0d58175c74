"""GPU (`-m gpu`): `lmi_kmeans_f16` -- `lmi_kmeans` on rows given as binary16 -- against the numpy restatement (tests/kmeans_ref.py,
unchanged) and against `_capi.kmeans`, both on the widened array.  Widening a half is exact, so every comparison is exact: centroids
as uint32 bit patterns, labels, counts and `changed` with array_equal.  The cases are those of tests/kmeans_f16_cases.py: the six of
the float form narrowed once (they hold binary16 subnormals), d % 4 == 0 with d % 8 != 0 (the float path reads 16 bytes at a time,
the half path must not) and d = 8 (one 16-byte group, the tail at link d opens the second); test_build_f16_host.py pins that they
keep what they were chosen for."""
import numpy as np
import pytest
import torch

import kmeans_f16_cases as cases
import kmeans_ref

pytestmark = pytest.mark.gpu
NITER = cases.NITER


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


def host(got):
    c, labels, counts, changed = got
    assert c.is_cuda and labels.is_cuda and c.dtype == torch.float32 and labels.dtype == torch.int32
    return c.cpu().numpy(), labels.cpu().numpy(), counts, changed


@pytest.mark.parametrize("key", sorted(cases.CASES))
def test_parity_with_the_reference_and_with_the_float_call(capi, key):
    x16, x, c0, *want = cases.case(*key)
    got = capi.kmeans(x16, key[2], niter=NITER, init=c0)
    assert_same(got, want)
    assert_same(got, capi.kmeans(x, key[2], niter=NITER, init=c0))


def test_niter_0_assigns_to_the_initial_centroids(capi, oracle):
    x16, x, c0 = cases.case(3001, 45, 7, 1)[:3]
    c, labels, counts, changed = capi.kmeans(x16, 7, niter=0, init=c0)
    assert np.array_equal(bits(c), bits(c0))
    assert np.array_equal(labels, oracle.knn_l2(x, c0, k=1, nthreads=4)[1][:, 0])
    assert changed.tolist() == [3001] and np.array_equal(counts, np.bincount(labels, minlength=7))


# (1500, 64, ..) and (600, 768, ..): d % 8 == 0, so the layout alone decides between 16-byte and 2-byte loads
@pytest.mark.parametrize("layout", ["aligned", "shifted", "end"])
@pytest.mark.parametrize("key", [(1500, 64, 40, 6), (600, 768, 257, 4), (4099, 33, 33, 3)])
def test_device_tensors_equal_the_host_call(capi, key, layout):
    x16, _, c0, *want = cases.case(*key)
    n, d = x16.shape
    flat = torch.from_numpy(np.array(x16)).cuda().reshape(-1)
    if layout == "aligned":
        xt = flat.reshape(n, d)
        assert xt.data_ptr() % 16 == 0
    elif layout == "shifted":   # one half past a 16-byte boundary: the element form, also where d % 8 == 0
        room = torch.zeros(n * d + 1, dtype=torch.float16, device="cuda")
        room[1:] = flat
        xt = room[1:].reshape(n, d)
        assert xt.data_ptr() % 16 == 2 and xt.is_contiguous()
    else:   # the last row ends the tensor's storage: the 16-byte form where d % 8 == 0, and nothing is read behind the last half
        room = torch.zeros(8 + n * d, dtype=torch.float16, device="cuda")
        room[8:] = flat
        xt = room[8:].reshape(n, d)
        assert xt.data_ptr() % 16 == 0 and xt.data_ptr() + n * d * 2 == room.data_ptr() + room.untyped_storage().nbytes()
    keep = xt.clone()
    for _ in range(2):
        assert_same(host(capi.kmeans(xt, key[2], niter=NITER, init=c0)), want)
    assert torch.equal(xt, keep)


def test_default_init_is_the_seeded_choice_of_rows(capi, oracle):
    x16, x = cases.case(4099, 33, 33, 3)[:2]
    c0 = x[np.random.RandomState(2023).choice(4099, 33, replace=False)]
    want = kmeans_ref.kmeans_ref(oracle, x, c0, 2)
    assert_same(capi.kmeans(x16, 33, niter=2), want)
    assert_same(host(capi.kmeans(torch.from_numpy(np.array(x16)).cuda(), 33, niter=2)), want)


MAGNITUDES = ["subnormal", "max65504", "zero", "negzero", "column"]


def magnitude_case(name):
    """(x16, c0 f32, niter, e)"""
    rs = np.random.RandomState(21)
    if name == "zero":
        return np.zeros((64, 8), np.float16), np.zeros((2, 8), np.float32), 2, 0
    if name == "negzero":   # -0.0 is zero: it is no maximum, it adds nothing to a sum
        x16 = np.zeros((64, 8), np.float16)
        x16[::3] = np.float16(-0.0)
        assert (x16.view(np.uint16) == 0x8000).any()
        return x16, np.zeros((2, 8), np.float32), 2, 0
    if name == "subnormal":   # every value a binary16 subnormal (or zero): the widened maximum is below 2^-14
        x16 = rs.randint(-1023, 1024, (300, 24)).astype(np.int16)
        x16 = (np.abs(x16).astype(np.uint16) | np.where(x16 < 0, 0x8000, 0).astype(np.uint16)).view(np.float16)
        x16[7, 3] = np.uint16(0x03FF).view(np.float16)   # the largest subnormal: e = -14
        assert cases.subnormals(x16) == int((x16 != 0).sum()) and float(np.abs(x16.astype(np.float32)).max()) == 1023 * 2.0 ** -24
        return x16, x16[:5].astype(np.float32), 2, -14
    if name == "max65504":   # a row of +-65504, the largest half: e = 16
        x16 = rs.uniform(-3, 3, (300, 16)).astype(np.float16)
        x16[11] = np.float16(65504.0) * np.where(np.arange(16) % 2, -1, 1).astype(np.float16)
        return x16, x16[9:14].astype(np.float32), 2, 16
    x16 = np.array(cases.case(4099, 33, 33, 3)[0])   # "column": one dominant column, the others quantise coarsely beside it
    x16[:, 5] = (x16[:, 5].astype(np.float32) * 4096).astype(np.float16)
    c0 = x16[np.random.RandomState(3).choice(4099, 33, replace=False)].astype(np.float32)
    return x16, c0, 2, kmeans_ref.exponent(x16.astype(np.float32))


@pytest.mark.parametrize("name", MAGNITUDES)
def test_magnitudes(capi, oracle, name):
    x16, c0, niter, e = magnitude_case(name)
    x = x16.astype(np.float32)
    assert np.isfinite(x).all() and kmeans_ref.exponent(x) == e
    got = capi.kmeans(x16, c0.shape[0], niter=niter, init=c0)
    assert_same(got, kmeans_ref.kmeans_ref(oracle, x, c0, niter))
    assert_same(got, capi.kmeans(x, c0.shape[0], niter=niter, init=c0))
    if name in ("zero", "negzero"):
        assert not got[1].any() and got[2].tolist() == [64, 0] and not bits(got[0]).any()


def raw_call(capi, x16, k, niter, c, labels, counts, changed, d=None, n=None, null_x=False):
    n = x16.shape[0] if n is None else n
    d = x16.shape[1] if d is None else d
    rc = capi.lib().lmi_kmeans_f16(0, None if null_x else x16.ctypes.data, n, d, k, niter, c.ctypes.data, labels.ctypes.data,
                                   counts.ctypes.data, changed.ctypes.data, 0)
    capi._check(rc)


REFUSALS = {
    "nan_x": (dict(poke_x=np.nan), "x holds a value that is not finite"),
    "inf_x": (dict(poke_x=np.inf), "x holds a value that is not finite"),
    "neg_inf_x": (dict(poke_x=-np.inf), "x holds a value that is not finite"),
    "nan_init": (dict(poke_c=np.nan), "initial centroids hold a value that is not finite"),
    "k_gt_n": (dict(k=41), "k 41 exceeds n 40"),
    "k_0": (dict(k=0), "k 0 outside"),
    "k_16385": (dict(k=16385), "k 16385 outside"),
    "d_0": (dict(d=0), "d 0 outside"),
    "d_4097": (dict(d=4097), "d 4097 outside"),
    "n_0": (dict(n=0), "n 0 < 1"),
    "n_2_26": (dict(n=(1 << 26) + 1), "exceeds 2\\^26"),
    "niter_neg": (dict(niter=-1), "niter -1 outside"),
    "niter_1001": (dict(niter=1001), "niter 1001 outside"),
    "null_x": (dict(null_x=True), "must not be NULL"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_call_and_the_condition_and_write_nothing(capi, name):
    spec, message = REFUSALS[name]
    n, d, k, niter = 40, 12, spec.get("k", 3), spec.get("niter", 2)
    rs = np.random.RandomState(5)
    x16 = rs.randn(n, d).astype(np.float16)
    kk = min(max(k, 1), 64)
    c = x16[:min(kk, n)].astype(np.float32) if kk <= n else np.zeros((kk, d), np.float32)
    if "poke_x" in spec:
        x16[17, 5] = spec["poke_x"]
    if "poke_c" in spec:
        c[1, 2] = spec["poke_c"]
    labels = np.full(n, 77, np.int32)
    counts = np.full(kk, 78, np.int64)
    changed = np.full(1002, 79, np.int64)
    c_before = c.copy()
    with pytest.raises(capi.LmiError, match="lmi_kmeans_f16: .*" + message):
        raw_call(capi, x16, k, niter, c, labels, counts, changed, d=spec.get("d"), n=spec.get("n"), null_x=spec.get("null_x", False))
    assert np.array_equal(bits(c), bits(c_before))
    assert (labels == 77).all() and (counts == 78).all() and (changed == 79).all()


def test_a_refused_device_call_writes_nothing(capi):
    """The device form: a NaN half found by the pass that takes max|x| leaves the caller's centroids and labels as they were."""
    rs = np.random.RandomState(6)
    x16 = rs.randn(200, 16).astype(np.float16)
    x16[150, 9] = np.nan
    xt = torch.from_numpy(x16).cuda()
    c = torch.from_numpy(x16[:4].astype(np.float32)).cuda()
    labels = torch.full((200,), 77, dtype=torch.int32, device="cuda")
    c_before = c.clone()
    torch.cuda.synchronize()
    rc = capi.lib().lmi_kmeans_f16(0, xt.data_ptr(), 200, 16, 4, 2, c.data_ptr(), labels.data_ptr(), None, None, 1)
    with pytest.raises(capi.LmiError, match="lmi_kmeans_f16: x holds a value that is not finite"):
        capi._check(rc)
    assert torch.equal(c, c_before) and bool((labels == 77).all())
