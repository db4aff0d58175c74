#!/usr/bin/env python3
"""Times `_capi.eigh` on a device tensor at d = 96 (the resident form), 768 and 4096 (the streamed form) and, beside it,
`np.linalg.eigh` of the same matrix on the host the benchmark runs on.  The matrix is a scatter matrix X^T X of Gaussian X with decaying
column scales, as a PCA fit meets it.  Writes what was measured to profiles/eigh.txt; nothing is asserted and nothing about speed is
promised: the streamed form issues (D - 1) * sweeps launches and is bound by their rate at moderate d.

Every time is a host clock around a call that has returned its outputs (the library's call ends in a device synchronise), the median
of `--reps` calls after `--warmup` calls of the same shape.  Each line is printed as soon as it is measured.

  python3 tools/eigh_bench.py [--out profiles/eigh.txt] [--reps 5] [--warmup 1] [--dims 96 768 4096]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigh.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dims", type=int, nargs="+", default=[96, 768, 4096])
    a = ap.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("eigh_bench needs the MI355X: there is no CPU path to time")
    from learnedmetricindex_amd import _capi

    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"# tools/eigh_bench.py: median (min .. max) of {a.reps} calls after {a.warmup} warm-up call(s); float64, all d eigenpairs")
    say(f"# device: {torch.cuda.get_device_name(0)}; library: {_capi.lib().lmi_build_info().decode()}; host BLAS threads: {os.cpu_count()} CPUs visible")
    for d in a.dims:
        x = np.random.RandomState(d).randn(2 * d, d) * (0.999 ** np.arange(d))
        g = x.T @ x
        gt = torch.from_numpy(g).cuda()
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: _capi.eigh(gt), a.reps, a.warmup)
        plan = _capi.eigh_plan()
        say(f"lmi_eigh        d={d}: {med * 1e3:11.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})  sweeps {plan['SWEEPS']}, launches {plan['LAUNCHES']}, "
            f"form {plan['FORM']}, tile {plan['TILE']}, LDS {plan['LDS_BYTES']} B, workspace {plan['WORKSPACE_BYTES']} B")
        med, lo, hi = timed(lambda: np.linalg.eigh(g), a.reps, a.warmup)
        say(f"np.linalg.eigh  d={d}: {med * 1e3:11.3f} ms ({lo * 1e3:.3f} .. {hi * 1e3:.3f})")
        del gt
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
