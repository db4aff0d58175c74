#!/usr/bin/env python3
"""Cost of the exact brute-force k-NN on the device (`_capi.knn`, lmi_knn) against the two calls that did the same work before it,
on the same card, the same data and in the same process.

Data: standard-normal rows, --nb x --d base (default 1M x 768), --nq queries (10 000); k in --ks (10 100 1024); both metrics; with
device tensors (nothing uploaded inside the window) and with host arrays (the base goes up in pieces inside the window).
Yardsticks, both older than lmi_knn:
  (a) `_capi.knn_ip` (lmi_knn_ip), k = 10, host arrays: builds a one-bucket index per call and scans it -- against knn's host leg
  (b) the all-f32 scan: `Index(prefilter=False)`, one bucket, n_buckets = 1, data resident, device queries, LMI_T_SCAN of
      `lmi_scan_topk` -- the same 2 * nq * nb * d FLOP by the same instruction -- against knn's device leg at k = 10 (inner product)
One warm-up of every leg, then --reps (5) timed runs with the legs alternated; the times are a host clock around the synchronising
call; median (min .. max) in ms, FLOP/s = 2 * nq * nb * d / median, and its share of the 157.3 TFLOP/s f32 MFMA peak.
The split between the score, selection and merge kernels comes from a kernel trace of `--trace-run` (this program started with
that flag runs only the device legs, once each after a warm-up, for a profiler to watch).

--f16: the binary16 form (lmi_knn_f16) beside the binary32 one.  The rows are narrowed once (`astype(float16)` of the same draw); the
"knn16" legs take the halves, the "knn" legs the same values widened, so both forms do the same arithmetic and return the same bits
(checked on the warm-up); the legs of the two forms alternate, and the yardsticks (a) and (b) are left out.  Per pair of legs the
table adds f16 / f32, and per form the host leg minus the device leg: the upload and the staging the host arrays cost.

  python tools/knn_bench.py [--nb 1000000] [--d 768] [--nq 10000] [--ks 10 100 1024] [--reps 5] [--f16] [--out profiles/knn.txt]

Prints a table and one JSON line; --out also writes both to a file.  No gate: the feature is the capability.  Not a yardstick:
bench.py is.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from learnedmetricindex_amd import _capi  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--no-host", action="store_true", help="skip the legs that upload from host arrays")
    ap.add_argument("--f16", action="store_true", help="lmi_knn_f16 on the rows narrowed once beside lmi_knn on the same values widened")
    ap.add_argument("--trace-run", action="store_true", help="only the device legs, once each (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    db = torch.randn((a.nb, a.d), generator=gen, device="cuda", dtype=torch.float32)
    dq = torch.randn((a.nq, a.d), generator=gen, device="cuda", dtype=torch.float32)
    flop = 2.0 * a.nq * a.nb * a.d
    if a.f16:
        db16, dq16 = db.half(), dq.half()
        db, dq = db16.float(), dq16.float()

    legs = {}
    for metric in ("ip", "l2"):
        for k in a.ks:
            legs[f"knn device {metric} k={k}"] = (lambda metric=metric, k=k: _capi.knn(dq, db, k, metric))
            if a.f16:
                legs[f"knn16 device {metric} k={k}"] = (lambda metric=metric, k=k: _capi.knn(dq16, db16, k, metric))
    if a.trace_run:
        for name, fn in legs.items():
            fn()
            _, ms = wall(fn)
            print(f"{name}: {ms:.1f} ms   plan {_capi.knn_last_plan()}", flush=True)
        return

    xb, xq = db.cpu().numpy(), dq.cpu().numpy()
    if a.f16:
        xb16, xq16 = xb.astype(np.float16), xq.astype(np.float16)
    if not a.no_host:
        for metric in ("ip", "l2"):
            for k in a.ks:
                legs[f"knn host {metric} k={k}"] = (lambda metric=metric, k=k: _capi.knn(xq, xb, k, metric))
                if a.f16:
                    legs[f"knn16 host {metric} k={k}"] = (lambda metric=metric, k=k: _capi.knn(xq16, xb16, k, metric))
        if not a.f16:
            legs["(a) knn_ip host k=10"] = lambda: _capi.knn_ip(xq, xb, 10)
    if a.f16:
        return report_f16(a, legs, flop)
    # (b): the all-f32 scan of a resident one-bucket index
    idx = _capi.Index(0, prefilter=False)
    idx.set_buckets(xb, np.zeros(a.nb, dtype=np.int64), 1)
    bo = torch.zeros((a.nq, 1), dtype=torch.int32, device="cuda")
    sd = torch.empty((a.nq, 10), dtype=torch.float32, device="cuda")
    si = torch.empty((a.nq, 10), dtype=torch.int32, device="cuda")
    scan_ms = []

    def scan():
        idx.scan_topk_device(dq, bo, 1, 10, sd, si)
        torch.cuda.synchronize()
        scan_ms.append(float(idx.timings()[_capi.T_SCAN]))

    legs["(b) all-f32 scan k=10 (wall)"] = scan

    plans = {}
    for name, fn in legs.items():   # warm-up
        fn()
        if name.startswith("knn"):
            plans[name] = _capi.knn_last_plan()
    scan_ms.clear()
    times = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            _, ms = wall(fn)
            times[name].append(ms)
    times["(b) all-f32 scan k=10 (LMI_T_SCAN)"] = list(scan_ms)

    med = {n: statistics.median(v) for n, v in times.items()}
    lines = [f"# tools/knn_bench.py: base {a.nb} x {a.d}, {a.nq} queries, {a.reps} timed runs per leg after one warm-up, legs alternated",
             f"# library: {_capi.lib().lmi_build_info().decode()}",
             f"# device: {torch.cuda.get_device_name(0)}; 2 * nq * nb * d = {flop:.3e} FLOP; f32 MFMA peak {PEAK_F32_MFMA / 1e12:.1f} TFLOP/s",
             "# leg | ms median (min .. max) | TFLOP/s | share of peak"]
    for n, v in times.items():
        lines.append(f"{n:38s} | {med[n]:9.2f} ({min(v):.2f} .. {max(v):.2f}) | {flop / med[n] / 1e9:7.2f} | {flop / med[n] * 1e3 / PEAK_F32_MFMA:6.1%}")
    result = {"nb": a.nb, "d": a.d, "nq": a.nq, "median_ms": med}
    kb = f"knn device ip k={a.ks[0]}"
    b = "(b) all-f32 scan k=10 (LMI_T_SCAN)"
    vb = times[b]
    lines.append(f"# {kb} / (b) LMI_T_SCAN: {med[kb] / med[b]:.3f}   ((b)'s own spread: {(max(vb) - min(vb)) / med[b]:.1%})")
    result["ratio_device_to_scan"] = med[kb] / med[b]
    if not a.no_host:
        kh, ka = f"knn host ip k={a.ks[0]}", "(a) knn_ip host k=10"
        lines.append(f"# {kh} / {ka}: {med[kh] / med[ka]:.3f}")
        result["ratio_host_to_knn_ip"] = med[kh] / med[ka]
    for kind in ("device",) + (() if a.no_host else ("host",)):
        for metric in ("ip", "l2"):
            lo, hi = f"knn {kind} {metric} k={a.ks[0]}", f"knn {kind} {metric} k={a.ks[-1]}"
            lines.append(f"# {kind} {metric}: k={a.ks[0]} -> k={a.ks[-1]}: {med[lo]:.2f} -> {med[hi]:.2f} ms (x{med[hi] / med[lo]:.2f})")
    for n, p in plans.items():
        lines.append(f"# plan of {n}: {p}")
    lines.append(json.dumps(result))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    idx.close()


def report_f16(a, legs, flop):
    """The --f16 run: warm-up (the two forms must agree bit for bit), timed runs with the legs alternated, the table."""
    import torch

    plans, first = {}, {}
    for name, fn in legs.items():
        D, I = fn()
        plans[name] = _capi.knn_last_plan()
        first[name] = (np.asarray(D.cpu() if hasattr(D, "cpu") else D).view(np.uint32), np.asarray(I.cpu() if hasattr(I, "cpu") else I))
    for name in legs:
        if name.startswith("knn16 "):
            ref = first["knn " + name[len("knn16 "):]]
            assert np.array_equal(first[name][0], ref[0]) and np.array_equal(first[name][1], ref[1]), f"{name} differs from the binary32 leg"
    del first
    times = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            _, ms = wall(fn)
            times[name].append(ms)
    med = {n: statistics.median(v) for n, v in times.items()}
    lines = [f"# tools/knn_bench.py --f16: base {a.nb} x {a.d}, {a.nq} queries, {a.reps} timed runs per leg after one warm-up, legs alternated",
             "# knn16: lmi_knn_f16 on the rows narrowed once; knn: lmi_knn on the same values widened; the warm-up results agree bit for bit",
             f"# library: {_capi.lib().lmi_build_info().decode()}",
             f"# device: {torch.cuda.get_device_name(0)}; 2 * nq * nb * d = {flop:.3e} FLOP; f32 MFMA peak {PEAK_F32_MFMA / 1e12:.1f} TFLOP/s",
             "# leg | ms median (min .. max) | TFLOP/s | share of peak"]
    for n, v in times.items():
        lines.append(f"{n:38s} | {med[n]:9.2f} ({min(v):.2f} .. {max(v):.2f}) | {flop / med[n] / 1e9:7.2f} | {flop / med[n] * 1e3 / PEAK_F32_MFMA:6.1%}")
    result = {"nb": a.nb, "d": a.d, "nq": a.nq, "median_ms": med, "f16_over_f32": {}}
    for n in legs:
        if n.startswith("knn16 "):
            n32 = "knn " + n[len("knn16 "):]
            result["f16_over_f32"][n32] = med[n] / med[n32]
            lines.append(f"# {n} / {n32}: {med[n] / med[n32]:.3f}   ({med[n]:.2f} ms against {med[n32]:.2f} ms, whose own max is {max(times[n32]):.2f})")
    if not a.no_host:
        for form in ("knn", "knn16"):
            for metric in ("ip", "l2"):
                for k in a.ks:
                    h, dv = f"{form} host {metric} k={k}", f"{form} device {metric} k={k}"
                    lines.append(f"# {form} {metric} k={k}: host - device = {med[h] - med[dv]:.2f} ms")
    for n, p in plans.items():
        lines.append(f"# plan of {n}: {p}")
    lines.append(json.dumps(result))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
