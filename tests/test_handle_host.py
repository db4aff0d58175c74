"""CPU (`-m "not gpu"`): the ownership rules of the handle (csrc/lmi_handle.h) under AddressSanitizer + UBSan with leak detection.

tests/host/handle_selftest.cpp is a stand-alone program: it includes lmi_handle.h, defines the four HIP calls DevBuf makes over
malloc / free with a record of the live allocations, and links no HIP library.  What it asserts: a DevBuf's copy borrows and cannot
grow, its move hands the memory on, a growing vector<DevBuf> keeps its allocations, an early error return frees temporaries; a clone
(clone_handle) shares every model and index image as a borrowed view, starts with a fresh call state, and frees only what it
reserved itself; after the parent has gone nothing is left."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handle_ownership_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "handle_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "handle_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "handle selftest: clean" in r.stdout
