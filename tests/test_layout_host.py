"""CPU (`-m "not gpu"`): the bucket layout's arithmetic (csrc/lmi_layout.h) under AddressSanitizer + UBSan.

tests/host/layout_selftest.cpp is a stand-alone program: it includes lmi_layout.h, which is pure host code (the standard library, no
HIP call, no kernel header), and nothing else of the library.  What it asserts: the chunk length a build picks (by index size, the
low-dimensional form's 4096, the all-f32 scan's 3 MiB, the 1024-chunk floor, a caller-set value); a fresh build's layout and the
tables derived from the per-bucket counts; for an insert one hand-built case per layout path (slack, relocation, growth re-pack, hole
re-pack) with the exact numbers, both refusals, and on every accepted plan disjoint bucket ranges inside the layout, cap >= need and
exactly the path counters lmi_debug_layout documents; the staging groups of a delete."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "layout_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "layout_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "layout selftest: clean" in r.stdout
