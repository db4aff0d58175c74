#!/usr/bin/env python3
"""Cost of clustering on the device with `hip_kmeans` (lmi_kmeans) against the torch stand-in that `faiss_kmeans` falls back to
where faiss is absent (`faiss_kmeans.TorchKmeans`), on the same card and the same data.

Data: the `synth` mixture (tests/golden/synth.py), --n rows x --d (default 1M x 768), --k clusters (120), --niter passes (20).
Both sides are timed from the host array in to the host labels out -- the boundary `LearnedIndexBuilder` sees:
  hip       li.clustering.hip_kmeans.cluster(x, k, {"niter": niter})
  stand-in  km = TorchKmeans(d, k, niter); km.train(x); km.assign()
One warm-up of each, then --reps (5) timed runs, alternating the two; the medians and the spread (min .. max) are reported.
Gate: the median of `hip` is not above the median of the stand-in by more than the run-to-run spread of the two (the larger of
their max - min); exit status 1 otherwise.
Beside the gate, with x resident on the device (no upload in the window): the whole call at niter = 0 (set-up and one assignment)
and at --niter, whose difference over niter is one full pass (assignment + update).  The per-kernel split of a pass comes from a
kernel trace of `--trace-run` (this program started with that flag runs only the device-resident call, a few passes, for a profiler
to watch); --kernel-ms "assign=..,update=.." carries the traced per-pass kernel times into the report, which turns the assignment's
into a fraction of the 157.3 TFLOP/s f32 MFMA peak (flops = 2 * n * roundup(k, 32) * roundup(d + 1, 32) as executed, and
2 * n * k * d as the algorithm needs).
The two sides do not compute the same labels (different seeding draws, different arithmetic); hip's result is checked for being a
clustering at all: every label in range, the counts its histogram.

  python tools/kmeans_bench.py [--n 1000000] [--d 768] [--k 120] [--niter 20] [--reps 5] [--out profiles/kmeans.txt]
  python tools/kmeans_bench.py --f16 [--n ..] [--d ..] [--k ..] [--niter ..] [--out profiles/kmeans_f16.txt]

--f16: instead of the above, `lmi_kmeans_f16` beside `lmi_kmeans` on the same values in one process: the mixture narrowed to float16
(the half form's input) and widened again (the float form's).  Per form: the host-pointer call at niter = 0 less the device-tensor
call at niter = 0 (the upload, the allocations of x and the labels' way back), one pass from the device-tensor calls as above, and
the peak device memory of the host-pointer call -- polled from a second thread while the call runs, beside the figure of the
header's formula.  Five repeats each, alternating the forms; the spread (max - min) of the float form's five pass times is what a
difference between the forms is held against.  The results of the two forms must be equal bit for bit, or the run stops.

Prints a table and one JSON line; --out also writes both to a file.  Not a yardstick: bench.py is.
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from learnedmetricindex_amd import _capi  # noqa: E402
from learnedmetricindex_amd.li.clustering.faiss_kmeans import TorchKmeans  # noqa: E402
from learnedmetricindex_amd.li.clustering.hip_kmeans import cluster as hip_cluster  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run_hip(x, k, niter):
    return hip_cluster(x, k, {"niter": niter})


def run_standin(x, k, niter):
    km = TorchKmeans(d=x.shape[1], k=k, niter=niter)
    km.train(x)
    return km, km.assign()


class PeakPoll:
    """Peak device memory in use while the block runs, less what was in use before: free memory polled from a second thread (the
    library call releases the interpreter lock)."""

    def __enter__(self):
        import threading

        import torch

        torch.cuda.synchronize()
        self.base = torch.cuda.mem_get_info()[0]
        self.low, self.stop = self.base, False

        def poll():
            while not self.stop:
                self.low = min(self.low, torch.cuda.mem_get_info()[0])

        self.thread = threading.Thread(target=poll)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()
        self.peak = self.base - self.low


def f16_ab(a):
    """lmi_kmeans_f16 beside lmi_kmeans on the same values"""
    import torch
    import synth

    reps = 5
    x32, _ = synth.mixture(a.seed, a.n, a.d, a.k, 1)
    x16 = x32.astype(np.float16)
    x32 = x16.astype(np.float32)
    forms = {"f32": (x32, torch.from_numpy(x32).cuda()), "f16": (x16, torch.from_numpy(x16).cuda())}
    rup = lambda v, m: (v + m - 1) // m * m  # noqa: E731
    kk = rup(a.k, 32)
    shared = 8 * a.n + kk * (8 * a.d + 4 * rup(a.d + 1, 32) + 12) + 8 * (a.niter + 2) + 4 * a.k * a.d + 4 * a.n
    lines = [f"kmeans_bench --f16: {a.n} x {a.d}, k = {a.k}, niter = {a.niter}, {reps} repeats, the forms alternating; "
             f"{torch.cuda.get_device_name(0)}; {_capi.lib().lmi_build_info().decode()}"]
    out, t = {}, {f: dict(host0=[], dev0=[], devn=[]) for f in forms}
    for f, (xh, xd) in forms.items():   # warm-up, and the results
        out[f] = _capi.kmeans(xh, a.k, niter=a.niter, seed=a.seed)
        got = _capi.kmeans(xd, a.k, niter=a.niter, seed=a.seed)
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), out[f][0].view(np.uint32)) and np.array_equal(got[1].cpu().numpy(), out[f][1])
    same = all(np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, v.view(np.uint32) if v.dtype == np.float32 else v)
               for u, v in zip(out["f32"], out["f16"]))
    assert same, "lmi_kmeans_f16 and lmi_kmeans differ on the same values"
    for _ in range(reps):
        for f, (xh, xd) in forms.items():
            t[f]["host0"].append(wall(lambda: _capi.kmeans(xh, a.k, niter=0, seed=a.seed))[1])
            t[f]["dev0"].append(wall(lambda: _capi.kmeans(xd, a.k, niter=0, seed=a.seed))[1])
            t[f]["devn"].append(wall(lambda: _capi.kmeans(xd, a.k, niter=a.niter, seed=a.seed))[1])
    res = dict(n=a.n, d=a.d, k=a.k, niter=a.niter, bitwise_equal=True, build=_capi.lib().lmi_build_info().decode())
    lines.append("form   upload ms (host - device call, niter 0)   one pass ms: median  min  max   peak device MiB: polled  formula")
    for f, (xh, xd) in forms.items():
        passes = [(n_ - z) / max(a.niter, 1) for n_, z in zip(t[f]["devn"], t[f]["dev0"])]
        upload = statistics.median(t[f]["host0"]) - statistics.median(t[f]["dev0"])
        with PeakPoll() as peak:
            _capi.kmeans(xh, a.k, niter=min(a.niter, 2), seed=a.seed)
        formula = shared - 8 * (a.niter - min(a.niter, 2)) + xh.dtype.itemsize * a.n * a.d
        lines.append(f"  {f}  {upload:12.2f}                                {statistics.median(passes):10.3f} {min(passes):8.3f} {max(passes):8.3f}"
                     f"          {peak.peak / 2 ** 20:10.1f} {formula / 2 ** 20:9.1f}")
        res[f] = dict(upload_ms=upload, pass_ms=passes, pass_median_ms=statistics.median(passes), peak_polled_bytes=int(peak.peak),
                      peak_formula_bytes=int(formula), host0_ms=t[f]["host0"], dev0_ms=t[f]["dev0"], devn_ms=t[f]["devn"])
    spread = max(res["f32"]["pass_ms"]) - min(res["f32"]["pass_ms"])
    diff = res["f16"]["pass_median_ms"] - res["f32"]["pass_median_ms"]
    lines += [f"  spread of the float form's {reps} pass times: {spread:.3f} ms; f16 - f32 (medians): {diff:+.3f} ms: "
              + ("within the spread" if diff <= spread else "the half form is SLOWER by more than the spread"),
              "  centroids, labels, counts and changed of the two forms: equal bit for bit"]
    res.update(f32_pass_spread_ms=spread, f16_minus_f32_pass_ms=diff, f16_slower_than_spread=bool(diff > spread))
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=120)
    ap.add_argument("--niter", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--kernel-ms", default="", help='traced kernel times per pass, e.g. "assign=3.1,update=1.2"')
    ap.add_argument("--trace-run", action="store_true", help="only the device-resident call (for a kernel trace)")
    ap.add_argument("--f16", action="store_true", help="lmi_kmeans_f16 beside lmi_kmeans on the same values")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import synth

    assert torch.cuda.is_available(), "kmeans_bench needs the MI355X"
    _capi.lib()
    if a.f16:
        return f16_ab(a)
    x, _ = synth.mixture(a.seed, a.n, a.d, a.k, 1)
    xt = torch.from_numpy(x).cuda()
    if a.trace_run:
        _capi.kmeans(xt, a.k, niter=a.niter)
        torch.cuda.synchronize()
        return 0

    lines = [f"kmeans_bench: {a.n} x {a.d}, k = {a.k}, niter = {a.niter}, {a.reps} timed runs after one warm-up each; "
             f"{torch.cuda.get_device_name(0)}; {_capi.lib().lmi_build_info().decode()}"]
    (obj, labels), _ = wall(lambda: run_hip(x, a.k, a.niter))           # warm-up
    assert labels.shape == (a.n,) and labels.min() >= 0 and labels.max() < a.k
    assert np.array_equal(obj.counts, np.bincount(labels, minlength=a.k))
    wall(lambda: run_standin(x, a.k, a.niter))                           # warm-up
    hip_ms, std_ms = [], []
    for _ in range(a.reps):
        hip_ms.append(wall(lambda: run_hip(x, a.k, a.niter))[1])
        std_ms.append(wall(lambda: run_standin(x, a.k, a.niter))[1])
    med_h, med_s = statistics.median(hip_ms), statistics.median(std_ms)
    spread = max(max(hip_ms) - min(hip_ms), max(std_ms) - min(std_ms))
    ok = med_h <= med_s + spread
    lines += ["host array in -> host labels out (ms)        median       min       max",
              f"  hip_kmeans.cluster                      {med_h:10.1f} {min(hip_ms):9.1f} {max(hip_ms):9.1f}",
              f"  TorchKmeans.train + .assign (stand-in)  {med_s:10.1f} {min(std_ms):9.1f} {max(std_ms):9.1f}",
              f"  gate (hip <= stand-in + spread {spread:.1f} ms): {'met' if ok else 'MISSED'}; stand-in / hip = {med_s / med_h:.2f}",
              f"  passes that moved labels: {int((obj.changed > 0).sum())} of {a.niter + 1}"]

    # x resident on the device: the call without the upload
    dev0, devn = [], []
    _capi.kmeans(xt, a.k, niter=a.niter)
    for _ in range(a.reps):
        dev0.append(wall(lambda: _capi.kmeans(xt, a.k, niter=0))[1])
        devn.append(wall(lambda: _capi.kmeans(xt, a.k, niter=a.niter))[1])
    m0, mn = statistics.median(dev0), statistics.median(devn)
    per_pass = (mn - m0) / max(a.niter, 1)
    lines += ["device tensor in -> device labels out (ms)",
              f"  niter = 0 (set-up + one assignment)     {m0:10.2f}",
              f"  niter = {a.niter:<4d}                            {mn:10.2f}",
              f"  one pass (assignment + update)          {per_pass:10.3f}"]
    res = dict(n=a.n, d=a.d, k=a.k, niter=a.niter, hip_ms=hip_ms, standin_ms=std_ms, hip_median_ms=med_h, standin_median_ms=med_s,
               spread_ms=spread, gate_met=bool(ok), device_niter0_ms=m0, device_ms=mn, pass_ms=per_pass,
               build=_capi.lib().lmi_build_info().decode())
    if a.kernel_ms:
        km = {p.split("=")[0]: float(p.split("=")[1]) for p in a.kernel_ms.split(",")}
        rup = lambda v, m: (v + m - 1) // m * m  # noqa: E731
        done = 2.0 * a.n * rup(a.k, 32) * rup(a.d + 1, 32)
        need = 2.0 * a.n * a.k * a.d
        lines += ["traced kernel time per pass (ms)"] + [f"  {name:<10s} {ms:8.3f}" for name, ms in km.items()]
        if "assign" in km:
            frac_done, frac_need = done / (km["assign"] * 1e-3) / PEAK_F32_MFMA, need / (km["assign"] * 1e-3) / PEAK_F32_MFMA
            lines.append(f"  assignment: {done / km['assign'] * 1e-9:.1f} TFLOP/s executed = {frac_done:.2f} of the f32 MFMA peak "
                         f"({frac_need:.2f} counting only 2 n k d)")
            res.update(assign_fraction_of_peak=frac_done, assign_fraction_of_peak_useful=frac_need)
        res["kernel_ms"] = km
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
