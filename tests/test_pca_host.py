"""CPU (`-m "not gpu"`): the host side of the PCA pair -- lmi_gram's geometry under the sanitizers, the binding's argument errors
before any library is loaded, and the restatement (tests/pca_ref.py) against plain float64."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pca_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gram_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gram_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "gram_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "gram plan selftest: clean" in r.stdout


X = np.zeros((8, 6), np.float32)
BAD_ARGUMENTS = {
    "gram_list": (lambda c: c.gram([[1.0, 2.0]]), "numpy array or a torch tensor"),
    "gram_float64": (lambda c: c.gram(X.astype(np.float64)), "must be float32"),
    "gram_1d": (lambda c: c.gram(X[0]), "n, d >= 1"),
    "gram_empty": (lambda c: c.gram(X[:0]), "n, d >= 1"),
    "gram_wide": (lambda c: c.gram(np.zeros((1, 4097), np.float16)), "d 4097 outside"),
    "project_basis_shape": (lambda c: c.project(X, np.zeros((3, 5), np.float32)), r"basis must be float32 \[m,6\]"),
    "project_basis_dtype": (lambda c: c.project(X, np.zeros((3, 6), np.float64)), "basis must be float32"),
    "project_m_1025": (lambda c: c.project(X, np.zeros((1025, 6), np.float32)), "m 1025 outside"),
    "project_mean_shape": (lambda c: c.project(X, np.zeros((3, 6), np.float32), mean=np.zeros(5, np.float32)), r"mean must be float32 \[6\]"),
    "fit_m": (lambda c: __import__("learnedmetricindex_amd.projection", fromlist=["x"]).PcaProjection.fit(X, 7), "m 7 outside"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGUMENTS))
def test_argument_errors_raise_before_the_library_loads(monkeypatch, name):
    from learnedmetricindex_amd import _capi

    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/liblmi_hip.so")
    call, message = BAD_ARGUMENTS[name]
    with pytest.raises(ValueError, match=message):
        call(_capi)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,d", pca_ref.GRAM_VALUE_SHAPES)
def test_the_value_cases_are_what_their_names_say(n, d):
    """The exponent of every case, and what the restatement makes of the degenerate ones (tests/test_gpu_pca.py holds the device to
    the restatement bit for bit, so these are statements about the device too)."""
    for name in pca_ref.GRAM_VALUE_NAMES:
        x, mean, g, e = pca_ref.gram_values_case(name, n, d)
        assert e == pca_ref.VALUES[name][1], (name, e)
        assert np.isfinite(g).all() and np.array_equal(g, g.T)
    x, mean, g, _ = pca_ref.gram_values_case("down70", n, d)
    c = x - mean
    assert float(np.abs(c[:, 0] * c[:, 1]).max()) < 2.0 ** -126 and g.all()   # subnormal products, and none of them lost
    x, mean, g, _ = pca_ref.gram_values_case("last_exponent", n, d)
    assert float(np.abs(x).max()) == 2.0 ** 56 - 2.0 ** 32 == float(np.nextafter(np.float32(2.0 ** 56), np.float32(0)))
    x, mean, g, _ = pca_ref.gram_values_case("full_mantissa", n, d)
    assert not np.array_equal(x.astype(np.float16).astype(np.float32), x) and (u32(x) & 0xfff).any()
    x, mean, g, _ = pca_ref.gram_values_case("zero", n, d)
    assert not u32(mean).any() and not u64(g).any()   # +0 everywhere
    x, mean, g, _ = pca_ref.gram_values_case("const_and_equal", n, d)
    assert mean[3] == 2.5 and not u64(g[3]).any() and not u64(g[:, 3]).any()
    assert np.array_equal(u64(g[5]), u64(g[8])) and g[5, 5] == g[8, 8] == g[5, 8] > 0
    x, mean, g, _ = pca_ref.gram_values_case("halves_only", n, d)
    x16 = x.astype(np.float16)
    assert np.array_equal(u32(x16.astype(np.float32)), u32(x)) and np.signbit(x[3]).all() and not x[3].any()
    assert (np.abs(x[:2]) == 65504).all() and ((x16[2].view(np.uint16) & 0x7c00) == 0).all() and x[2].all()


@pytest.mark.parametrize("n,d", pca_ref.GRAM_VALUE_SHAPES)
def test_the_gram_restatement_under_a_change_of_scale(n, d):
    """x 2^40 is exact all the way: mean 2^40 and gram 2^80 of the plain case, bit for bit.  x 2^-70 is not -- the products of a chain
    are binary32 subnormals -- and is held against the float64 product instead: test_gram_against_float64's entrywise bound
    (tests/test_gpu_pca.py) and one quantum of the smallest subnormal, 2^-149, for every link of every piece's chain."""
    x, mean, g, e = pca_ref.gram_values_case("plain", n, d)
    xu, meanu, gu, eu = pca_ref.gram_values_case("up40", n, d)
    assert np.array_equal(u32(xu), u32(np.ldexp(x, 40))) and eu == e + 40
    assert np.array_equal(u32(meanu), u32(np.ldexp(mean, 40))) and np.array_equal(u64(gu), u64(np.ldexp(g, 80)))
    xd, meand, gd, ed = pca_ref.gram_values_case("down70", n, d)
    assert np.array_equal(u32(xd), u32(np.ldexp(x, -70))) and ed == e - 70 and np.array_equal(u32(meand), u32(np.ldexp(mean, -70)))
    c = (xd - meand).astype(np.float64)
    bound = (4096 + 2) * 2.0 ** -24 * (np.abs(c).T @ np.abs(c)) + -(-n // 4096) * 2.0 ** (2 * ed - 33) + n * 2.0 ** -149
    err = np.abs(gd - c.T @ c)
    print("down70", (n, d), "max err / bound", float((err / bound).max()), "gram changed by the subnormal products:",
          int((u64(gd) != u64(np.ldexp(g, -140))).sum()), "of", d * d)
    assert (err <= bound).all()


def test_the_project_value_cases(oracle):
    """What the restatement makes of the special rows: the non-finite rows alone differ from the clean case; a row of -0.0 and an
    all-zero basis row give +0 (the chain starts from +0) where nothing is centred."""
    for centred in (False, True):
        clean = pca_ref.project_values_case("clean", centred)[3]
        x, basis, mean, y = pca_ref.project_values_case("nonfinite", centred)
        others = np.setdiff1d(np.arange(x.shape[0]), pca_ref.NONFINITE_ROWS)
        assert np.array_equal(u32(y[others]), u32(clean[others])) and np.isfinite(y[others]).all()
        assert np.isnan(y[7]).all() and not np.isfinite(y[9]).any() and np.isinf(y[9]).any()
        assert not u32(pca_ref.project_values_case("zero_basis_row", centred)[3][:, 2]).any()
        y = pca_ref.project_values_case("down70", centred)[3]
        assert y.all() and float(np.abs(y).max()) < 2.0 ** -60
    assert not u32(pca_ref.project_values_case("neg_zero_row", False)[3][5]).any()


def test_the_restatement_is_a_scatter_matrix_and_a_projection(oracle, tmp_path):
    from learnedmetricindex_amd.projection import PcaProjection

    x = pca_ref.rows(4100, 5, 3)   # two pieces
    mean, g, e = pca_ref.gram_ref(oracle, x)
    assert e == pca_ref.kmeans_ref.exponent(x) and np.allclose(mean, x.mean(axis=0, dtype=np.float64), rtol=0, atol=2.0 ** (e - 24))
    c = (x - mean).astype(np.float64)
    assert np.allclose(g, c.T @ c, rtol=1e-4) and np.array_equal(g, g.T)
    basis = np.random.RandomState(1).randn(3, 5).astype(np.float32)
    y = pca_ref.project_ref(oracle, x[:9], basis, mean)
    assert y.dtype == np.float32 and np.allclose(y, c[:9] @ basis.astype(np.float64).T, atol=1e-4)
    p = PcaProjection(mean, basis, [3.0, 2.0, 1.0])
    p.save(tmp_path / "p.npz")
    q = PcaProjection.load(tmp_path / "p.npz")
    assert np.array_equal(q.mean, mean) and np.array_equal(q.basis, basis) and q.explained_variance.tolist() == [3.0, 2.0, 1.0] and (q.m, q.d) == (3, 5)
