#!/usr/bin/env python3
"""Cost of the exact brute-force range query on the device (`_capi.range_knn`, lmi_knn_range) against `_capi.knn` (lmi_knn) at
k = 10 on the same card, the same arrays and in the same process.

Both calls compute the same scores with the same kernels (lmi_knn is not touched by lmi_knn_range: its time here is its time
before), so the difference is the last stage -- count, emit and gather instead of selection and merge -- and the one synchronisation
per piece that sizes a piece's chunk.

Data: standard-normal rows, --nb x --d base (default 1M x 768), --nq queries (10 000), inner product.  Radii: per query the
distance of its --targets-th (10 1000) nearest row in a `knn(k = 1024)` run, so that a leg admits that many results per query (ties
aside).  Legs: with device tensors (nothing uploaded inside the window) and with host arrays (the base goes up in pieces inside the
window).  One warm-up of every leg, then --reps (5) timed runs with the legs alternated; the times are a host clock around the
synchronising call, result read-back not included (the result stays on the device and is freed outside the window); median
(min .. max) in ms.  The split between the score, count, emit and gather kernels comes from a kernel trace of `--trace-run` (this
program started with that flag runs only the device legs, once each after a warm-up, for a profiler to watch).

--f16: the binary16 forms (lmi_knn_range_f16, lmi_knn_f16) beside the binary32 ones.  The rows are narrowed once; the "range16" /
"knn16" legs take the halves, the others the same values widened (the radii are made on those), so both forms admit the same results;
the legs of the two forms alternate.

  python tools/knn_range_bench.py [--nb 1000000] [--d 768] [--nq 10000] [--targets 10 1000] [--reps 5] [--f16] [--out FILE]

Prints a table and one JSON line; --out also writes both to a file.  No gate.  Not a yardstick: bench.py is.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from learnedmetricindex_amd import _capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--targets", type=int, nargs="+", default=[10, 1000], help="results per query a leg's radii admit (1..1024)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--no-host", action="store_true", help="skip the legs that upload from host arrays")
    ap.add_argument("--f16", action="store_true", help="the _f16 forms on the rows narrowed once beside the binary32 forms on the same values widened")
    ap.add_argument("--trace-run", action="store_true", help="only the device legs, once each after a warm-up (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert all(1 <= t <= _capi.KNN_MAX_K for t in a.targets)

    import torch

    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    db = torch.randn((a.nb, a.d), generator=gen, device="cuda", dtype=torch.float32)
    dq = torch.randn((a.nq, a.d), generator=gen, device="cuda", dtype=torch.float32)
    if a.f16:
        db16, dq16 = db.half(), dq.half()
        db, dq = db16.float(), dq16.float()
    D, _ = _capi.knn(dq, db, max(a.targets), "ip")
    radii = {t: (1.0 - D[:, t - 1]).cpu().numpy() for t in a.targets}
    del D
    if a.trace_run:
        a.no_host = True
    xb, xq = (None, None) if a.no_host else (db.cpu().numpy(), dq.cpu().numpy())
    xb16, xq16 = (xb.astype("float16"), xq.astype("float16")) if a.f16 and not a.no_host else (None, None)

    plans, results = {}, {}

    def knn_leg(q, x):
        return lambda: _capi.knn(q, x, 10, "ip")

    def range_leg(name, q, x, t):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = _capi.range_knn(q, x, radii[t], "ip")
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            plans[name] = _capi.knn_range_last_plan()
            results[name] = res.total
            res.close()
            return ms
        return run

    def timed(fn):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        return run

    legs = {}
    for kind, q, x, q16, x16 in (("device", dq, db, dq16 if a.f16 else None, db16 if a.f16 else None),) + (() if a.no_host else (("host", xq, xb, xq16, xb16),)):
        legs[f"knn {kind} k=10"] = timed(knn_leg(q, x))
        if a.f16:
            legs[f"knn16 {kind} k=10"] = timed(knn_leg(q16, x16))
        for t in a.targets:
            name = f"range {kind} ~{t}/query"
            legs[name] = range_leg(name, q, x, t)
            if a.f16:
                name = f"range16 {kind} ~{t}/query"
                legs[name] = range_leg(name, q16, x16, t)
    if a.trace_run:
        for name, fn in legs.items():
            fn()
            print(f"{name}: {fn():.1f} ms   plan {plans.get(name) or _capi.knn_last_plan()}", flush=True)
        return
    for name, fn in legs.items():   # warm-up
        fn()
        if name.startswith("knn"):
            plans[name] = _capi.knn_last_plan()
    times = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            times[name].append(fn())

    med = {n: statistics.median(v) for n, v in times.items()}
    lines = [f"# tools/knn_range_bench.py{' --f16' if a.f16 else ''}: base {a.nb} x {a.d}, {a.nq} queries, inner product, {a.reps} timed runs per leg after one warm-up, legs alternated",
             f"# library: {_capi.lib().lmi_build_info().decode()}",
             f"# device: {torch.cuda.get_device_name(0)}",
             "# leg | ms median (min .. max) | results | ratio to knn k=10 of the same pointer kind"]
    result = {"nb": a.nb, "d": a.d, "nq": a.nq, "median_ms": med, "ratio": {}, "results": results}
    for n, v in times.items():
        base = med[f"knn{'16' if n.split()[0].endswith('16') else ''} {n.split()[1]} k=10"]   # the knn leg of the same form
        result["ratio"][n] = med[n] / base
        lines.append(f"{n:28s} | {med[n]:9.2f} ({min(v):.2f} .. {max(v):.2f}) | {results.get(n, a.nq * 10):11d} | {med[n] / base:6.3f}")
    if a.f16:
        result["f16_over_f32"] = {}
        for n in legs:
            if n.split()[0] in ("knn16", "range16"):
                n32 = n.replace("16 ", " ", 1)
                assert results.get(n) == results.get(n32), f"{n} admits {results.get(n)} results, {n32} {results.get(n32)}"
                result["f16_over_f32"][n32] = med[n] / med[n32]
                lines.append(f"# {n} / {n32}: {med[n] / med[n32]:.3f}   ({med[n]:.2f} ms against {med[n32]:.2f} ms, whose own max is {max(times[n32]):.2f})")
        for form in ("", "16"):
            for n in legs:
                if n.split()[0] == "knn" + form or n.split()[0] == "range" + form:
                    if " host " in n:
                        lines.append(f"# {n}: host - device = {med[n] - med[n.replace(' host ', ' device ')]:.2f} ms")
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
