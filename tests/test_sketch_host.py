"""CPU (`-m "not gpu"`): the host side of lmi_sketch -- one signature in the header, the binding and the library; argument errors
raised before the library is loaded; a SketchProjection is a function of its arguments and survives save / load bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from learnedmetricindex_amd import _capi
from learnedmetricindex_amd.li.Baseline import Baseline
from learnedmetricindex_amd.projection import PcaProjection, SketchProjection

X, B = np.zeros((8, 6), np.float32), np.zeros((64, 6), np.float32)


@pytest.fixture
def no_lib(monkeypatch):
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/liblmi_hip.so")


def test_the_symbols_are_exported_declared_and_bound():
    header = open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "lmi_hip.h")).read()
    decl = re.search(r"LMI_API int lmi_sketch\((.*?)\);", header, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", decl).split(",")]
    assert params == ["int device", "const float *x", "int64_t n", "int d", "const float *mean", "const float *basis", "int m",
                      "const float *thresh", "uint8_t *codes", "int on_device"]
    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _capi.SIGNATURES["lmi_sketch"] == (i, [i, p, l, i, p, p, i, p, p, i]) == _capi.SIGNATURES["lmi_sketch_f16"]
    L = ctypes.CDLL(_capi.LIB_PATH)
    assert hasattr(L, "lmi_sketch") and hasattr(L, "lmi_sketch_f16") and _capi.SKETCH_MAX_BITS == 8 * _capi.HAMMING_MAX_BYTES


BAD_ARGUMENTS = {
    "basis_shape": (lambda: _capi.sketch(X, B[:, :5]), r"sketch: basis must be float32 \[m,6\]"),
    "m_40": (lambda: _capi.sketch(X, B[:40]), "sketch: m 40 is not a multiple of 32"),
    "m_4128": (lambda: _capi.sketch(X, np.zeros((4128, 6), np.float32)), "sketch: m 4128 is not a multiple of 32"),
    "mean_shape": (lambda: _capi.sketch(X, B, mean=np.zeros(5, np.float32)), r"sketch: mean must be float32 \[6\]"),
    "projection_bits": (lambda: SketchProjection(B[:48]), "SketchProjection: bits 48"),
    "projection_mean": (lambda: SketchProjection(B, mean=np.zeros(5)), "SketchProjection: mean"),
    "from_pca_bits": (lambda: SketchProjection.from_pca(PcaProjection(np.zeros(6), B, np.zeros(64)), 96), "from_pca: bits 96 outside"),
    "searched_sketcher": (lambda: Baseline().search_sketched(X, X, B), "search_sketched: sketcher"),
    "searched_k": (lambda: Baseline().search_sketched(X, X, SketchProjection(B), k=11, n_candidates=10), "search_sketched: n_candidates"),
    "searched_d": (lambda: Baseline().search_sketched(X, X[:, :5], SketchProjection(B)), "search_sketched: queries"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGUMENTS))
def test_argument_errors_raise_before_the_library_loads(no_lib, name):
    call, message = BAD_ARGUMENTS[name]
    with pytest.raises(ValueError, match=message):
        call()


def test_a_sketch_projection_is_a_function_of_its_arguments_and_keeps_its_bits(tmp_path):
    a, b = SketchProjection.random(44, 96, 7), SketchProjection.random(44, 96, 7)
    assert (a.bits, a.d) == (96, 44) and a.basis.dtype == np.float32 and a.mean is None and a.thresh is None
    assert np.array_equal(a.basis.view(np.uint32), b.basis.view(np.uint32))
    assert np.array_equal(a.basis, np.random.RandomState(7).randn(96, 44).astype(np.float32))
    assert not np.array_equal(a.basis, SketchProjection.random(44, 96, 8).basis)
    pca = PcaProjection(np.arange(44), np.random.RandomState(1).randn(70, 44), np.arange(70)[::-1])
    s = SketchProjection.from_pca(pca, 64)
    assert np.array_equal(s.basis, pca.basis[:64]) and np.array_equal(s.mean, pca.mean) and s.bits == 64
    full = SketchProjection(a.basis, mean=np.full(44, -0.0), thresh=np.random.RandomState(2).randn(96))
    for p, name in ((a, "bare.npz"), (full, "full.npz")):
        p.save(tmp_path / name)
        q = SketchProjection.load(tmp_path / name)
        for u, v in ((p.basis, q.basis), (p.mean, q.mean), (p.thresh, q.thresh)):
            assert (u is None and v is None) or (v.dtype == np.float32 and np.array_equal(u.view(np.uint32), v.view(np.uint32)))
