"""CPU: `_capi.f16_admissible`, the numpy statement of the rule by which the library accepts scan vectors for
`storage="f16"` (LMI_STORAGE_F16, include/lmi_hip.h): every value finite and exactly representable in binary16, and still
so once multiplied by the index scale -- the power of two s with max|x| * s in [0.5, 1).  The GPU suite
(test_gpu_f16_storage.py) checks that the library's own verdict, taken on the device, is the same on these cases."""
import numpy as np

from learnedmetricindex_amd import _capi


def gaussian(seed=0, n=200, d=32):
    """Gaussian rows of unit length, like the embeddings this storage is for (max|x| < 1: the index scale is >= 1 and only
    grows values; N(0, 1) rows with max|x| >= 1 get a scale <= 1/2, under which a quantised value below 2**-13 usually
    loses its last bits -- such data is rightly refused, see test_f16_admissible_edges)."""
    x = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def quantised(x):
    return x.astype(np.float16).astype(np.float32)


#: name -> (rows, admissible); shared with the GPU test, which places each row inside otherwise admissible data
CASES = {
    "quantised gaussian": (quantised(gaussian()), True),
    "raw f32 gaussian": (gaussian(), False),
    "2.0 and 2**-24": (np.array([[2.0, 2.0 ** -24, 0.5, 0.0]], dtype=np.float32), False),   # s <= 1/4 pushes 2**-26 out of binary16
    "0.75 and 2**-24": (np.array([[0.75, 2.0 ** -24, 0.5, 0.0]], dtype=np.float32), True),  # s = 1: nothing moves
    "all zeros": (np.zeros((3, 8), dtype=np.float32), True),
    "inf": (np.array([[0.5, np.inf, 0.25, 0.0]], dtype=np.float32), False),
}


def test_f16_admissible_cases():
    for name, (x, want) in CASES.items():
        ok, reason = _capi.f16_admissible(x)
        assert ok is want, (name, reason)
        assert isinstance(reason, str) and reason


def test_f16_admissible_names_the_condition():
    assert "finite" in _capi.f16_admissible(CASES["inf"][0])[1]
    assert "binary16" in _capi.f16_admissible(CASES["raw f32 gaussian"][0])[1]
    assert "scale" in _capi.f16_admissible(CASES["2.0 and 2**-24"][0])[1]
    assert "scale" not in _capi.f16_admissible(CASES["raw f32 gaussian"][0])[1]


def test_f16_admissible_edges():
    f = _capi.f16_admissible
    assert f(np.array([65504.0, -65504.0, 2.0 ** -8], dtype=np.float32))[0]        # the largest half; s = 2**-16 keeps 2**-24
    assert not f(np.array([65504.0, 2.0 ** -9], dtype=np.float32))[0]              # ... and loses 2**-25
    assert not f(np.array([65520.0], dtype=np.float32))[0]                         # rounds to inf in binary16
    assert not f(np.array([np.nan], dtype=np.float32))[0]
    assert f(np.array([2.0 ** -24, -2.0 ** -24], dtype=np.float32))[0]             # subnormals alone: the scale only grows them
    assert f(np.array([1.0, 2.0 ** -23], dtype=np.float32))[0]                     # max|x| = 1: s = 1/2, 2**-24 survives
    assert not f(np.array([1.0, 2.0 ** -24], dtype=np.float32))[0]
    assert f(np.empty((0, 4), dtype=np.float32))[0]
    # a quantised normal half below 2**-14 / s keeps 11 significant bits that the subnormal range under a scale s < 1 cannot hold
    x = np.array([3.0, (1.0 + 2.0 ** -10) * 2.0 ** -13], dtype=np.float32)   # s = 1/4
    assert f(x[1:])[0] and not f(x)[0]
