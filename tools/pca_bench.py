#!/usr/bin/env python3
"""Times `_capi.gram` and `_capi.project` on device tensors at the two shapes a user of the index meets -- 1M x 768 -> 96 (fit and
apply a navigation PCA on clip768-like data) and 10M x 96 -> 32 -- and, beside them, torch on the same device doing the same work in
float32: `xc.T @ xc` and `xc @ B.T` on the centred copy `xc`.  Writes what was measured to profiles/pca.txt; nothing is asserted.

Every time is a host clock around a call that ends in a device synchronise (the library's calls return when their outputs have landed;
the torch lines synchronise explicitly), the median of `--reps` calls after `--warmup` calls of the same shape.  The operation counts
are the algorithm's: n d^2 multiply-adds for the full scatter matrix (the library computes the upper triangle's tiles only, so its
rate over this count can exceed what its MFMAs do), n d m for the projection.  torch's lines do not include making `xc`.

  python3 tools/pca_bench.py [--out profiles/pca.txt] [--reps 5] [--warmup 2] [--small]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1_000_000, 768, 96), (10_000_000, 96, 32)]


def timed(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a rehearsal at 1/100 of the rows")
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("pca_bench needs the MI355X: there is no CPU path to time")
    from learnedmetricindex_amd import _capi

    sync = torch.cuda.synchronize
    lines = [f"# tools/pca_bench.py: median (min .. max) of {a.reps} calls after {a.warmup} warm-up calls, device tensors, float32",
             f"# device: {torch.cuda.get_device_name(0)}; library: {_capi.lib().lmi_build_info().decode()}"]
    for n, d, m in SHAPES:
        n = n // 100 if a.small else n
        g = torch.Generator(device="cuda").manual_seed(2023)
        x = torch.randn((n, d), device="cuda", generator=g) + torch.linspace(-1, 1, d, device="cuda")
        basis = torch.randn((m, d), device="cuda", generator=g)
        mean = x.mean(dim=0)
        rows = [("gram", lambda: _capi.gram(x), 2.0 * n * d * d),
                ("project", lambda: _capi.project(x, basis, mean=mean), 2.0 * n * d * m)]
        plan = None
        for name, fn, flop in rows:
            med, lo, hi = timed(fn, a.reps, a.warmup, sync)
            if name == "gram":
                plan = _capi.gram_last_plan()
            lines.append(f"{name:8s} n={n} d={d} m={m}: {med * 1e3:9.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})  {flop / med / 1e12:7.2f} TFLOP/s of the algorithm's count")
        lines.append(f"         gram plan: {plan}")
        xc = x - mean
        bt = basis.t().contiguous()
        for name, fn, flop in [("torch xc.T @ xc", lambda: xc.t() @ xc, 2.0 * n * d * d), ("torch xc @ B.T", lambda: xc @ bt, 2.0 * n * d * m)]:
            med, lo, hi = timed(fn, a.reps, a.warmup, sync)
            lines.append(f"{name:16s} n={n} d={d} m={m}: {med * 1e3:9.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})  {flop / med / 1e12:7.2f} TFLOP/s")
        del x, xc, basis, bt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
