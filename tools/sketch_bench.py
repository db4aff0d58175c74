#!/usr/bin/env python3
"""Times `_capi.sketch` on device tensors at 1M x 768 -> 1024 bits, float32 and float16 rows, beside the two ways to the same codes
without it: `_capi.project` followed by a torch compare-and-pack on the device (checked equal to `sketch` byte for byte before anything
is timed), and torch's own `(x - mean) @ B.T` followed by the same pack (float32 rows; its sums are ordered differently, so some bits
differ: the count is reported).  Writes what was measured to profiles/sketch.txt; nothing is asserted about speed.

Every time is a host clock around a call that ends in a device synchronise, the median of `--reps` calls after `--warmup` calls; the
contenders of one shape alternate inside every repetition.  The operation count is the algorithm's, 2 n d m; the bytes are x once and
the codes once.  `--walk-lib PATH` adds the same call through a second build of the library (csrc/build.sh with
LMI_EXTRA_FLAGS=-DLMI_SKETCH_WALK=1: a block walks its column groups instead of the group being the fast part of the block index),
checked equal and alternated with the others: the work-split measurement.  `--only sketch` times nothing else (for a kernel trace).

  python3 tools/sketch_bench.py [--out profiles/sketch.txt] [--reps 5] [--warmup 2] [--small] [--walk-lib PATH] [--only sketch]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, D, BITS = 1_000_000, 768, 1024


def timed(fns, reps, warmup, sync):
    """{name: (median, min, max)} of the calls in `fns`, alternated inside every repetition."""
    out = {name: [] for name in fns}
    for r in range(warmup + reps):
        for name, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if r >= warmup:
                out[name].append(time.perf_counter() - t0)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a rehearsal at 1/100 of the rows")
    ap.add_argument("--walk-lib", default=None, help="a build with -DLMI_SKETCH_WALK=1, timed beside the default work split")
    ap.add_argument("--only", default=None, choices=["sketch"], help="time this contender alone")
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("sketch_bench needs the MI355X: there is no CPU path to time")
    from learnedmetricindex_amd import _capi

    sync = torch.cuda.synchronize
    n, d, m = (N // 100 if a.small else N), D, BITS
    weights = (1 << torch.arange(8, device="cuda")).to(torch.uint8)

    def pack(y, thresh):   # np.packbits(y > thresh, axis=1, bitorder="little") on the device
        return ((y > thresh).view(n, m // 8, 8) * weights).sum(dim=2, dtype=torch.uint8)

    walk = None
    if a.walk_lib:
        walk = ctypes.CDLL(os.path.abspath(a.walk_lib))
        for name in ("lmi_sketch", "lmi_sketch_f16"):
            getattr(walk, name).restype, getattr(walk, name).argtypes = _capi.SIGNATURES[name]
        walk.lmi_last_error.restype = ctypes.c_char_p
    lines = [f"# tools/sketch_bench.py: median (min .. max) of {a.reps} calls after {a.warmup} warm-up calls, device tensors, "
             f"n={n} d={d} bits={m}; the contenders of a shape alternate inside every repetition",
             f"# device: {torch.cuda.get_device_name(0)}; library: {_capi.lib().lmi_build_info().decode()}"]
    g = torch.Generator(device="cuda").manual_seed(2023)
    x32 = torch.randn((n, d), device="cuda", generator=g) + torch.linspace(-1, 1, d, device="cuda")
    basis = torch.randn((m, d), device="cuda", generator=g)
    thresh = torch.randn(m, device="cuda", generator=g)
    flop, nbytes = 2.0 * n * d * m, lambda esz: float(n) * d * esz + n * m / 8
    for dtype in (torch.float32, torch.float16):
        x = x32.to(dtype)
        mean = x.float().mean(dim=0)
        codes = _capi.sketch(x, basis, mean, thresh)
        same = torch.equal(codes, pack(_capi.project(x, basis, mean=mean), thresh))
        lines.append(f"{str(dtype):14s} sketch == pack(project > thresh): {same}")
        if not same:
            raise SystemExit("\n".join(lines + ["the codes differ: nothing is timed"]))
        fns = {"sketch": lambda: _capi.sketch(x, basis, mean, thresh)}
        if walk is not None:
            out = torch.empty_like(codes)
            entry = walk.lmi_sketch_f16 if dtype == torch.float16 else walk.lmi_sketch

            def walking():
                rc = entry(0, x.data_ptr(), n, d, mean.data_ptr(), basis.data_ptr(), m, thresh.data_ptr(), out.data_ptr(), 1)
                assert rc == 0, walk.lmi_last_error()

            walking()
            lines.append(f"{str(dtype):14s} walking build == default build: {torch.equal(out, codes)}")
            fns["sketch, walking build"] = walking
        if a.only is None:
            fns["project + torch pack"] = lambda: pack(_capi.project(x, basis, mean=mean), thresh)
            fns["project alone"] = lambda: _capi.project(x, basis, mean=mean)
            if dtype == torch.float32:
                bt = basis.t().contiguous()
                diff = torch.bitwise_xor(codes, pack((x - mean) @ bt, thresh))
                flipped = int(((diff.unsqueeze(2) >> torch.arange(8, device="cuda", dtype=torch.uint8)) & 1).sum())
                lines.append(f"{str(dtype):14s} torch matmul + pack: {flipped} of {n * m} bits differ from sketch ({flipped / (n * m):.2e})")
                del diff
                fns["torch (x - mean) @ B.T + pack"] = lambda: pack((x - mean) @ bt, thresh)
        for name, (med, lo, hi) in timed(fns, a.reps, a.warmup, sync).items():
            lines.append(f"{str(dtype):14s} {name:30s}: {med * 1e3:9.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})  {flop / med / 1e12:7.2f} TFLOP/s, "
                         f"{nbytes(x.element_size()) / med / 1e9:7.1f} GB/s of the algorithm's counts")
        del x, codes
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
