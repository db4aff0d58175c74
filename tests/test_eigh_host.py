"""CPU (`-m "not gpu"`): the host side of lmi_eigh -- the schedule and the plan under the sanitizers, the binding's argument errors
before any library is loaded, and the accuracy of the restatement (tests/eigh_ref.py) against LAPACK.  The device equals the
restatement bit for bit (tests/test_gpu_eigh.py), so the last is the accuracy statement for the device too."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import eigh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eigh_plan_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "eigh_plan_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "eigh_plan_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "eigh plan selftest: clean" in r.stdout, (r.stdout + r.stderr)[-3000:]


A = np.zeros((6, 6))
BAD_ARGUMENTS = {
    "list": (lambda c: c.eigh([[1.0]]), "numpy array or a torch tensor"),
    "float32": (lambda c: c.eigh(A.astype(np.float32)), "must be float64"),
    "empty": (lambda c: c.eigh(A[:0]), "n, d >= 1"),
    "not_square": (lambda c: c.eigh(A[:4]), "must be square"),
    "d_4097": (lambda c: c.eigh(np.zeros((4097, 4097))), "d 4097 outside"),
    "m_0": (lambda c: c.eigh(A, 0), "m 0 outside"),
    "m_7": (lambda c: c.eigh(A, 7), "m 7 outside"),
    "solver": (lambda c: __import__("learnedmetricindex_amd.projection", fromlist=["x"]).PcaProjection.fit(A.astype(np.float32), 2, solver="qr"),
               "neither 'lapack' nor 'hip'"),
}


@pytest.mark.parametrize("name", sorted(BAD_ARGUMENTS))
def test_argument_errors_raise_before_the_library_loads(monkeypatch, name):
    from learnedmetricindex_amd import _capi

    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/liblmi_hip.so")
    call, message = BAD_ARGUMENTS[name]
    with pytest.raises(ValueError, match=message):
        call(_capi)


def test_the_branch_inputs_reach_their_branches(monkeypatch):
    """big_theta_*: rotated pairs with a finite |theta| >= 2^512 (d5: two of them); inf_theta: an infinite theta; neg_zero_theta:
    theta == -0.  Counted on the restatement, which the device equals bit for bit (tests/test_gpu_eigh.py)."""
    seen = {}
    plain = eigh_ref.rotations

    def spy(A, p, q):
        out = plain(A, p, q)
        with np.errstate(all="ignore"):
            theta = ((A[q, q] - A[p, p]) / (2.0 * A[p, q]))[out[3]]
        seen["big"] += int((np.isfinite(theta) & (np.abs(theta) >= 2.0 ** 512)).sum())
        seen["inf"] += int(np.isinf(theta).sum())
        seen["neg_zero"] += int(((theta == 0) & np.signbit(theta)).sum())
        return out

    monkeypatch.setattr(eigh_ref, "rotations", spy)
    for name, branch, at_least in [("big_theta_d2", "big", 1), ("big_theta_d5", "big", 2), ("inf_theta", "inf", 1),
                                   ("neg_zero_theta", "neg_zero", 1), ("mixed_sub_seen", "big", 1), ("d33", "big", 0)]:
        seen.update(big=0, inf=0, neg_zero=0)
        eigh_ref.eigh_ref(eigh_ref.INPUTS[name]())
        print(name, seen)
        assert seen[branch] >= at_least and (name != "d33" or not any(seen.values()))


@pytest.mark.parametrize("k", [900, -900])
def test_the_restatement_is_scale_invariant(k):
    """eigh_ref(a 2^k) = (w 2^k, v, sweeps) bit for bit: the first step normalises, ldexp is exact on both ends.  This, not LAPACK,
    is the statement for scaled_up and scaled_down."""
    a, w, v, sweeps = eigh_ref.case("degenerate")
    scaled = eigh_ref.case("scaled_up" if k > 0 else "scaled_down")
    assert np.array_equal(scaled[0], np.ldexp(a, k)) and eigh_ref.exponent(scaled[0]) == eigh_ref.exponent(a) + k
    assert np.array_equal(scaled[1].view(np.uint64), np.ldexp(w, k).view(np.uint64))
    assert np.array_equal(scaled[2].view(np.uint64), v.view(np.uint64)) and scaled[3] == sweeps


def test_the_rounded_entry_of_mixed_sub_seen_shows_in_v():
    """The entry lies past the midpoint of two subnormals after scaling: ldexp rounds it up.  An entry cut off instead (or flushed to
    zero) is a different matrix with a different v, so a device that scaled otherwise could not pass the parity test.  mixed_sub's own
    entry vanishes: it underflows to zero against a pair that is skipped."""
    a, w, v, sweeps = eigh_ref.case("mixed_sub_seen")
    e = eigh_ref.exponent(a)
    kept = np.ldexp(a[3, 11], -e)
    assert 0 < kept < 2.0 ** -1022 and kept == 2.0 ** -1024 + 2.0 ** -1074 and np.ldexp(kept, e) != a[3, 11]
    for entry in (2.0 ** -418, 0.0):   # the entry rounded toward zero, flushed
        other = eigh_ref.eigh_ref(eigh_ref.mixed_sub_seen(entry))
        assert not np.array_equal(other[1].view(np.uint64), v.view(np.uint64))
    assert np.ldexp(eigh_ref.INPUTS["mixed_sub"]()[0, 11], -eigh_ref.exponent(eigh_ref.INPUTS["mixed_sub"]())) == 0.0


@pytest.mark.parametrize("name", eigh_ref.ORDINARY_SCALE)
def test_the_restatement_against_lapack(name):
    """Residual ||GV - V L||_F / ||G||_F and orthogonality ||V^T V - I||_F within K = 3 * sweeps times LAPACK's own on the same
    matrix (DESIGN.md 5.16 derives K: an entry of V takes sweeps * (D - 1) plane rotations of three roundings each where LAPACK's
    takes of the order of d updates), floored at d * 2^-53 where LAPACK is exact; the eigenvalues within the sum of both residuals."""
    g, w, v, sweeps = eigh_ref.case(name)
    d = g.shape[0]
    assert sweeps < eigh_ref.SWEEP_CAP
    wl, vl = np.linalg.eigh(g)
    wl, vl = wl[::-1], vl[:, ::-1].T
    gnorm = np.linalg.norm(g)
    res, res_l = np.linalg.norm(v @ g - w[:, None] * v), np.linalg.norm(vl @ g - wl[:, None] * vl)
    orth, orth_l = np.linalg.norm(v @ v.T - np.eye(d)), np.linalg.norm(vl @ vl.T - np.eye(d))
    gap, floor, K = np.abs(w - wl).max(), d * 2.0 ** -53, 3 * sweeps
    print(f"{name}: sweeps {sweeps}, residual {res / max(gnorm, 1e-300):.3g} (LAPACK {res_l / max(gnorm, 1e-300):.3g}), "
          f"orthogonality {orth:.3g} (LAPACK {orth_l:.3g}), eigenvalue gap / max|w| {gap / max(np.abs(w).max(), 1e-300):.3g}, K {K}")
    assert res <= K * max(res_l, floor * gnorm) and orth <= K * max(orth_l, floor) and gap <= (K + 1) * max(res_l, floor * gnorm)
    assert np.all(np.diff(w) <= 0) and (v[np.arange(d), np.abs(v).argmax(axis=1)] > 0).all()
