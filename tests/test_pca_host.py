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
