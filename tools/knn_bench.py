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

--hamming [--bits 1024]: the Hamming form (lmi_knn_hamming) on random codes generated on the device, --nb x --bits against --nq
queries at k = --ks[0], device tensors, against the ways a user had before it, alternated in the same run:
  (a) a torch expression on the device, chunked over the base to fit memory: the codes unpacked to +-1 halves and one half matmul per
      chunk (dot = bits - 2 dist, exact: integers up to 4096 in a binary32 accumulator), or XOR and a SWAR bit count on int32 words
      (a byte popcount table wants an int64 index per byte); both run on the warm-up and the faster is the leg; topk per chunk, merged
  (b) `_capi.knn` with "l2" on the codes unpacked to float32 0/1, whose squared distance is the Hamming distance
All legs' distances are compared exactly before a time is printed, and the row numbers of lmi_knn_hamming and (b), which share
the tie rule (torch.topk has none).  Reported: median (min .. max), pairs/s, the call's device bytes (its plan) and, as a lower
bound taken from the whole call, the rate against the vector ALU: the score kernel issues 2 operations per pair of 32-bit words, so
2 * W * pairs / (CUs * 64 lanes * clock).  `--hamming --trace-run` runs only the HIP leg for `rocprofv3 --kernel-trace --stats`;
`--hamming --kernel-stats FILE` reads that run's kernel_stats.csv and prints the score / select split and the same fraction from the
score kernel's own time.

--rerank [--cands 1024] [--bits 1024]: the re-ranking call (lmi_knn_rerank) as the second stage of a sketch filter; main_rerank states
the legs and the checks.  `--rerank --trace-run` and `--rerank --kernel-stats FILE` work as for --hamming and print the kernels' split
and the score kernel's gather rate, nq * c * d * 4 bytes over its own time.

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
    ap.add_argument("--hamming", action="store_true", help="lmi_knn_hamming on random codes against a torch expression and the unpacked lmi_knn")
    ap.add_argument("--bits", type=int, default=1024, help="--hamming: bits per code (a multiple of 32)")
    ap.add_argument("--torch-form", choices=["both", "matmul", "SWAR"], default="both",
                    help="--hamming: the forms of leg (a) to run (the SWAR form takes seconds at 1M rows)")
    ap.add_argument("--kernel-stats", default=None, help="--hamming: the kernel_stats.csv of a traced --trace-run, to print the split")
    ap.add_argument("--rerank", action="store_true", help="lmi_knn_rerank behind a sketch filter against a torch gather + bmm and the whole-base lmi_knn")
    ap.add_argument("--cands", type=int, default=1024, help="--rerank: candidates per query")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.hamming:
        return main_hamming(a)
    if a.rerank:
        return main_rerank(a)

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


TRACE_CALLS = 2   # what `--trace-run` runs of a leg: one warm-up and one timed call


def valu_lanes_per_second():
    """(lane operations per second of the vector ALUs, CUs, MHz): 4 SIMDs of 16 lanes per compute unit, at the peak engine clock the
    runtime reports for the device (hipDeviceAttributeClockRate)."""
    import ctypes

    import torch

    khz = ctypes.c_int(0)
    err = ctypes.CDLL("libamdhip64.so").hipDeviceGetAttribute(ctypes.byref(khz), 5, 0)   # 5: hipDeviceAttributeClockRate, kHz
    assert err == 0 and khz.value > 0, "hipDeviceGetAttribute(hipDeviceAttributeClockRate) failed"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * 64 * khz.value * 1e3, cus, khz.value / 1e3


def hamming_torch_forms(dq, db, k, bits, chunk):
    """Leg (a): {name: closure -> (D int32 [nq,k], I int64 [nq,k])}.  What a closure keeps resident beside the codes (the +-1 halves of
    the base) is made here, outside every timed window."""
    import torch

    nq, nb, W = dq.shape[0], db.shape[0], bits // 32
    shifts = torch.arange(8, device="cuda", dtype=torch.uint8)

    def merged(parts, largest):
        v, i = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
        tv, ti = torch.topk(v, min(k, v.shape[1]), dim=1, largest=largest)
        return tv, torch.gather(i, 1, ti)

    pm_b = torch.empty((nb, bits), device="cuda", dtype=torch.float16)
    for c0 in range(0, nb, chunk):
        pm_b[c0:c0 + chunk] = 1 - 2 * ((db[c0:c0 + chunk, :, None] >> shifts) & 1).reshape(-1, bits).to(torch.float16)

    def matmul():
        pm_q = 1 - 2 * ((dq[:, :, None] >> shifts) & 1).reshape(nq, bits).to(torch.float16)
        parts = []
        for c0 in range(0, nb, chunk):
            v, i = torch.topk(pm_q @ pm_b[c0:c0 + chunk].T, min(k, nb - c0, chunk), dim=1, largest=True)
            parts.append((v, i + c0))
        v, i = merged(parts, True)
        return ((bits - v.float()) / 2).to(torch.int32), i

    q32, b32 = dq.view(torch.int32), db.view(torch.int32)

    def swar():
        rows = []
        for q0 in range(0, nq, 256):
            parts = []
            for c0 in range(0, nb, chunk // 8):
                v = q32[q0:q0 + 256, None, :] ^ b32[None, c0:c0 + chunk // 8, :]
                v = v - ((v >> 1) & 0x55555555)
                v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
                v = (((v + (v >> 4)) & 0x0F0F0F0F) * 0x01010101) >> 24
                tv, ti = torch.topk(v.sum(-1, dtype=torch.int32), min(k, nb - c0, chunk // 8), dim=1, largest=False)
                parts.append((tv, ti + c0))
            rows.append(merged(parts, False))
        return torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows])

    return {"(a) torch: +-1 halves, matmul, topk": matmul, "(a) torch: xor, SWAR bit count, topk": swar}


def hamming_split(a):
    """--kernel-stats: the score / select split of a traced `--hamming --trace-run`, and the score kernel's rate against the vector ALU."""
    import csv

    W, pairs = a.bits // 32, float(a.nq) * a.nb
    with open(a.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh)]
    ns = {}
    for key in ("hamming_score_kernel", "knn_select_kernel", "knn_merge_hamming_kernel", "knn_fill_kernel"):
        ns[key] = sum(float(r["TotalDurationNs"]) for r in rows if key in r["Name"]) / TRACE_CALLS
    total = sum(ns.values())
    lanes, cus, mhz = valu_lanes_per_second()
    lines = [f"# tools/knn_bench.py --hamming --kernel-stats: base {a.nb} x {a.bits} bits, {a.nq} queries, k = {a.ks[0]}; kernel time per call, from {TRACE_CALLS} traced calls"]
    for key, v in ns.items():
        lines.append(f"{key:28s} | {v / 1e6:9.2f} ms | {v / total:6.1%}")
    score_s = ns["hamming_score_kernel"] / 1e9
    lines.append(f"# score kernel: {pairs / score_s:.3e} pairs/s; 2 * W * pairs = {2 * W * pairs:.3e} lane operations over {score_s * 1e3:.2f} ms = "
                 f"{2 * W * pairs / score_s / lanes:.1%} of {cus} CUs x 64 lanes x {mhz:.0f} MHz (derived, not measured: 2 operations per word pair)")
    lines.append(f"# slab traffic: {8 * pairs:.3e} bytes written by the score and read by the selection")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def main_hamming(a):
    import torch

    if a.kernel_stats:
        return hamming_split(a)
    assert a.bits % 32 == 0 and 32 <= a.bits <= 4096
    cb, W, k, pairs = a.bits // 8, a.bits // 32, a.ks[0], float(a.nq) * a.nb
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    db = torch.randint(0, 256, (a.nb, cb), generator=gen, device="cuda", dtype=torch.uint8)
    dq = torch.randint(0, 256, (a.nq, cb), generator=gen, device="cuda", dtype=torch.uint8)
    hip = "knn_hamming device"
    legs = {hip: lambda: _capi.knn_hamming(dq, db, k)}
    if a.trace_run:
        legs[hip]()
        _, ms = wall(legs[hip])
        print(f"{hip}: {ms:.1f} ms   plan {_capi.knn_last_plan()}", flush=True)
        return
    chunk = 131072
    forms = hamming_torch_forms(dq, db, k, a.bits, chunk)
    if a.torch_form != "both":
        forms = {n: f for n, f in forms.items() if a.torch_form in n}
    shifts = torch.arange(8, device="cuda", dtype=torch.uint8)
    fb = torch.empty((a.nb, a.bits), device="cuda", dtype=torch.float32)
    for c0 in range(0, a.nb, chunk):
        fb[c0:c0 + chunk] = ((db[c0:c0 + chunk, :, None] >> shifts) & 1).reshape(-1, a.bits).to(torch.float32)
    fq = ((dq[:, :, None] >> shifts) & 1).reshape(a.nq, a.bits).to(torch.float32)
    b = "(b) knn l2 on the codes unpacked to float32"

    def knn_l2():
        D, I = _capi.knn(fq, fb, k, "l2")
        return D.to(torch.int32), I

    # warm-up: every leg once; the results must agree before any time is printed; the faster form of (a) is its leg
    first, warm = {}, {}
    for name, fn in {**legs, **forms, b: knn_l2}.items():
        first[name], warm[name] = wall(fn)
        if name in forms:   # (the first call of a form also loads its kernels; the second one is what picks the leg)
            warm[name] = wall(fn)[1]
    legs[hip]()   # (the last knn call was (b)'s)
    plan = _capi.knn_last_plan()
    D0, I0 = first[hip]
    for name, (D, I) in first.items():
        assert torch.equal(D, D0), f"{name}: distances differ from {hip}"
    assert torch.equal(first[b][1], I0), f"{b}: row numbers differ from {hip}"
    ta = min(forms, key=lambda n: warm[n])
    legs[ta], legs[b] = forms[ta], knn_l2
    del first
    times = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            _, ms = wall(fn)
            times[name].append(ms)
    med = {n: statistics.median(v) for n, v in times.items()}
    lanes, cus, mhz = valu_lanes_per_second()
    lines = [f"# tools/knn_bench.py --hamming: base {a.nb} x {a.bits} bits, {a.nq} queries, k = {k}, device tensors; {a.reps} timed runs per leg after one warm-up, legs alternated",
             f"# library: {_capi.lib().lmi_build_info().decode()}",
             f"# device: {torch.cuda.get_device_name(0)}; pairs = nq * nb = {pairs:.3e}",
             "# the distances of all legs are equal, and the row numbers of knn_hamming and (b) (torch.topk has no tie order)",
             "# second warm-up call of (a)'s forms: " + ", ".join(f"{n}: {warm[n]:.1f} ms" for n in forms) + "; what (a) and (b) keep unpacked is made outside the windows",
             "# leg | ms median (min .. max) | pairs/s"]
    for n, v in times.items():
        lines.append(f"{n:44s} | {med[n]:9.2f} ({min(v):.2f} .. {max(v):.2f}) | {pairs / med[n] * 1e3:.3e}")
    lines.append(f"# {hip} / {ta}: {med[hip] / med[ta]:.3f};  / {b}: {med[hip] / med[b]:.3f}")
    lines.append(f"# vector ALU, whole call (a lower bound of the score kernel's share): 2 * W * pairs = {2 * W * pairs:.3e} lane operations / "
                 f"{med[hip]:.2f} ms = {2 * W * pairs / med[hip] * 1e3 / lanes:.1%} of {cus} CUs x 64 lanes x {mhz:.0f} MHz")
    lines.append(f"# device bytes of the call beside the codes ({(a.nb + a.nq) * cb} bytes): {plan['WORKSPACE_BYTES']}; plan {plan}")
    result = {"hamming": True, "nb": a.nb, "bits": a.bits, "nq": a.nq, "k": k, "median_ms": med, "hip_over_torch": med[hip] / med[ta],
              "hip_over_knn_l2": med[hip] / med[b], "workspace_bytes": plan["WORKSPACE_BYTES"]}
    lines.append(json.dumps(result))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


RERANK_KERNELS = ("rerank_score_kernel", "rerank_sort_kernel", "rerank_qnorm_kernel", "rerank_check_kernel", "knn_fill_kernel")


def rerank_split(a):
    """--rerank --kernel-stats: the kernels' split of a traced `--rerank --trace-run`, and the score kernel's gather rate."""
    import csv

    with open(a.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh)]
    ns = {key: sum(float(r["TotalDurationNs"]) for r in rows if key in r["Name"]) / TRACE_CALLS for key in RERANK_KERNELS}
    total, gathered = sum(ns.values()), 4.0 * a.nq * a.cands * a.d
    lines = [f"# tools/knn_bench.py --rerank --kernel-stats: base {a.nb} x {a.d}, {a.nq} queries, c = {a.cands}, k = {a.ks[0]}; kernel time per call, from {TRACE_CALLS} traced calls"]
    lines += [f"{key:28s} | {v / 1e6:9.2f} ms | {v / total:6.1%}" for key, v in ns.items()]
    lines.append("# knn_fill_kernel also holds the fills of the one knn_hamming call that makes the candidates in the traced process")
    lines.append(f"# score kernel: nq * c * d * 4 = {gathered:.3e} bytes gathered in {ns['rerank_score_kernel'] / 1e6:.2f} ms = "
                 f"{gathered / ns['rerank_score_kernel']:.1f} GB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


def main_rerank(a):
    """--rerank: lmi_knn_rerank behind a sketch filter.  Codes: the sign bits of a random projection to --bits, packed; stage 1 is
    knn_hamming's top c = --cands; stage 2 the legs (a) knn_rerank, (b) a torch gather + bmm + topk in chunks of queries, (c) knn over
    the whole base.  Before any time is printed: (a) on knn's own shuffled top c equals knn bit for bit; (b) sums in another order, so
    bit equality with (a) cannot be asked of it: its scores must agree to 1e-4 and at least 99.9 % of its row numbers must be equal
    (a rounding difference of about d * 2^-24 * |s| swaps two neighbours only where their scores are that close: far rarer)."""
    import torch

    if a.kernel_stats:
        return rerank_split(a)
    k, c, metric = a.ks[0], a.cands, "ip"
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    db = torch.randn((a.nb, a.d), generator=gen, device="cuda", dtype=torch.float32)
    dq = torch.randn((a.nq, a.d), generator=gen, device="cuda", dtype=torch.float32)
    proj = torch.randn((a.d, a.bits), generator=gen, device="cuda", dtype=torch.float32)
    weights = (1 << torch.arange(8, device="cuda")).to(torch.uint8)

    def codes(x):
        out = torch.empty((x.shape[0], a.bits // 8), device="cuda", dtype=torch.uint8)
        for r0 in range(0, x.shape[0], 131072):
            bits = (x[r0:r0 + 131072] @ proj > 0).reshape(-1, a.bits // 8, 8).to(torch.uint8)
            out[r0:r0 + 131072] = (bits * weights).sum(2, dtype=torch.uint8)
        return out

    cb, cq = codes(db), codes(dq)
    stage1 = "stage 1: knn_hamming top c"
    hip, tb, full = "(a) knn_rerank device", "(b) torch gather + bmm + topk", "(c) knn over the whole base"
    cand = _capi.knn_hamming(cq, cb, c)[1]
    chunk = max(1, (1 << 30) // (4 * c * a.d))   # 1 GiB of gathered rows at a time

    def torch_leg():
        D, I = torch.empty((a.nq, k), device="cuda"), torch.empty((a.nq, k), device="cuda", dtype=torch.int64)
        for q0 in range(0, a.nq, chunk):
            cd = cand[q0:q0 + chunk].clamp_min(0)
            s = torch.bmm(db[cd], dq[q0:q0 + chunk, :, None]).squeeze(2)
            D[q0:q0 + chunk], pos = s.topk(k, dim=1)
            I[q0:q0 + chunk] = cd.gather(1, pos)
        return D, I

    legs = {stage1: lambda: _capi.knn_hamming(cq, cb, c), hip: lambda: _capi.knn_rerank(dq, db, cand, k, metric)}
    if a.trace_run:
        legs[hip]()
        _, ms = wall(legs[hip])
        print(f"{hip}: {ms:.1f} ms   plan {_capi.knn_last_plan()}", flush=True)
        return
    legs.update({tb: torch_leg, full: lambda: _capi.knn(dq, db, k, metric)})
    first = {name: wall(fn)[0] for name, fn in legs.items()}
    top = _capi.knn(dq, db, c, metric)[1]
    top = top.gather(1, torch.rand(top.shape, generator=gen, device="cuda").argsort(1))
    D, I = _capi.knn_rerank(dq, db, top, k, metric)
    assert torch.equal(D.view(torch.int32), first[full][0].view(torch.int32)) and torch.equal(I, first[full][1]), \
        "knn_rerank on knn's shuffled top c differs from knn"
    assert torch.allclose(first[tb][0], first[hip][0], rtol=1e-4, atol=1e-4), f"{tb}: scores differ from {hip}"
    same_ids = (first[tb][1] == first[hip][1]).float().mean().item()
    assert same_ids >= 0.999, f"{tb}: only {same_ids:.4%} of the row numbers equal {hip}'s"
    recall = (first[hip][1][:, :, None] == first[full][1][:, None, :]).any(2).float().mean().item()
    legs[hip]()
    plan = _capi.knn_last_plan()
    del first, top
    times = {name: [] for name in legs}
    for _ in range(a.reps):
        for name, fn in legs.items():
            times[name].append(wall(fn)[1])
    med = {n: statistics.median(v) for n, v in times.items()}
    gathered = 4.0 * a.nq * c * a.d
    lines = [f"# tools/knn_bench.py --rerank: base {a.nb} x {a.d}, {a.nq} queries, sketches of {a.bits} bits (sign bits of a random projection), "
             f"c = {c}, k = {k}, {metric}, device tensors; {a.reps} timed runs per leg after one warm-up, legs alternated",
             f"# library: {_capi.lib().lmi_build_info().decode()}",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"# checked first: knn_rerank on knn's shuffled top {c} == knn bit for bit; (b)'s scores within 1e-4 of (a)'s, {same_ids:.4%} of its row numbers equal",
             "# leg | ms median (min .. max)"]
    lines += [f"{n:36s} | {med[n]:9.2f} ({min(v):.2f} .. {max(v):.2f})" for n, v in times.items()]
    lines.append(f"# (a) / (b): {med[hip] / med[tb]:.3f};  two stages / (c): {(med[stage1] + med[hip]) / med[full]:.3f};  "
                 f"stage 1 : stage 2 = {med[stage1]:.2f} : {med[hip]:.2f} ms;  recall@{k} of the two stages against (c): {recall:.4f}")
    lines.append(f"# gather, whole call (a lower bound of the score kernel's rate): nq * c * d * 4 = {gathered:.3e} bytes / {med[hip]:.2f} ms = "
                 f"{gathered / med[hip] / 1e6:.1f} GB/s;  device bytes of the call: {plan['WORKSPACE_BYTES']}; plan {plan}")
    result = {"rerank": True, "nb": a.nb, "d": a.d, "nq": a.nq, "c": c, "k": k, "bits": a.bits, "median_ms": med, "recall": recall,
              "hip_over_torch": med[hip] / med[tb], "gather_GBps_whole_call": gathered / med[hip] / 1e6}
    lines.append(json.dumps(result))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
