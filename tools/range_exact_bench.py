#!/usr/bin/env python3
"""What the exact range search through the index costs and how much the covering balls prune (`Index.search_range_exact`,
lmi_search_range_exact), on clustered synthetic data generated on the device.

Data: --L unit centres in --d dimensions, --nb unit rows = normalise(centre + --sigma * N(0, 1) / sqrt(d)), a row's bucket = its
centre (what a converged k-means would give); --nq queries = stored rows moved by the same noise.  Inner product.  The router of the
`search_range` leg is the best a one-layer model can be on this data: logits = <centre, q>.  Radii: per query the distance of its
--targets-th nearest row in a `knn` run, so a leg returns about that many results per query.

Measured, each after one warm-up, --reps runs, a host clock around the synchronising call, median (min .. max) in ms:
  cover        `Cover(index)`: three passes over the stored rows; beside it the bytes of one pass over the row-major image and the rate
               that time would mean for ONE pass (the call makes three, so a third of the HBM rate is the ceiling of that figure);
  prune        `cover_order_device` counting alone: the pruning pass without the scan;
  visited      admitted buckets per query / L;
  exact        `search_range_exact_device`;
  brute force  `range_knn` over the same base on device tensors: the time to beat;
  search_range `search_range_device` at the smallest n_buckets (doubling from 1, then L) whose result is complete on this batch -- found
               by comparing totals with the exact call: a search_range result is a subset of it.

  python tools/range_exact_bench.py [--nb 1000000] [--d 768] [--L 120] [--nq 1000] [--sigma 1.0] [--targets 1 10 100 1000] [--reps 5]
                                    [--out profiles/range_exact.txt]

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
    ap.add_argument("--L", type=int, default=120)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--sigma", type=float, default=1.0, help="noise norm relative to the centre's (1.0: a row is 45 degrees off its centre)")
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 10, 100, 1000], help="results per query a leg's radii admit (1..1024)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--no-brute", action="store_true", help="skip the brute-force leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert all(1 <= t <= _capi.KNN_MAX_K for t in a.targets) and a.nq <= a.nb

    import numpy as np
    import torch

    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    unit = lambda x: x / x.norm(dim=1, keepdim=True)
    centres = unit(torch.randn((a.L, a.d), generator=gen, device="cuda"))
    lab = torch.randint(0, a.L, (a.nb,), generator=gen, device="cuda")
    piece = 1 << 18
    db = torch.empty((a.nb, a.d), device="cuda", dtype=torch.float32)
    for lo in range(0, a.nb, piece):
        hi = min(a.nb, lo + piece)
        db[lo:hi] = unit(centres[lab[lo:hi]] + a.sigma / a.d ** 0.5 * torch.randn((hi - lo, a.d), generator=gen, device="cuda"))
    src = torch.randperm(a.nb, generator=gen, device="cuda")[: a.nq]
    dq = unit(db[src] + a.sigma / a.d ** 0.5 * torch.randn((a.nq, a.d), generator=gen, device="cuda")).contiguous()

    idx = _capi.Index(0)
    idx.set_mlp([(centres.cpu().numpy(), np.zeros(a.L, np.float32))])
    idx.buckets_begin(lab.cpu().numpy().astype(np.int64), a.d, a.L)
    for lo in range(0, a.nb, piece):
        idx.add_rows(db[lo: min(a.nb, lo + piece)], lo)
    idx.buckets_end()
    torch.cuda.synchronize()

    D, _ = _capi.knn(dq, db, max(a.targets), "ip")
    radii = {t: np.ascontiguousarray((1.0 - D[:, t - 1]).cpu().numpy(), dtype=np.float32) for t in a.targets}
    del D

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def timed(fn, close=True):
        ms = []
        for rep in range(a.reps + 1):   # the first run warms up
            t, out = clock(fn)
            if close and hasattr(out, "close"):
                out.close()
            if rep:
                ms.append(t)
        return ms

    fmt = lambda v: f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"
    image_bytes = a.nb * a.d * 4
    result = {"nb": a.nb, "d": a.d, "L": a.L, "nq": a.nq, "sigma": a.sigma, "legs": {}}
    lines = [f"# tools/range_exact_bench.py: base {a.nb} x {a.d} in {a.L} buckets (sigma {a.sigma}), {a.nq} queries, inner product, {a.reps} timed "
             f"runs per leg after one warm-up",
             f"# library: {_capi.lib().lmi_build_info().decode()}",
             f"# device: {torch.cuda.get_device_name(0)}"]

    ms = timed(lambda: _capi.Cover(idx))
    med = statistics.median(ms)
    result["legs"]["cover"] = {"ms": med, "image_bytes": image_bytes, "gb_per_s_as_one_pass": image_bytes / med / 1e6}
    lines.append(f"cover build                  | {fmt(ms)} ms | row-major image {image_bytes / 1e9:.2f} GB: {image_bytes / med / 1e6:.0f} GB/s if it were "
                 f"one pass (it is three: x3 = {3 * image_bytes / med / 1e6:.0f} GB/s of reads)")
    cover = _capi.Cover(idx)
    c_t = torch.zeros(a.nq, dtype=torch.int32, device="cuda")
    lines.append("# target/query | visited (mean buckets / L) | max buckets | prune ms | exact ms | results | brute force ms | search_range: "
                 "n_buckets, ms")
    for t in a.targets:
        r = radii[t]
        p_ms = timed(lambda: idx.cover_order_device(dq, r, cover, 1, None, c_t))
        plan = _capi.cover_last_plan()
        visited = plan["ADMITTED"] / a.nq / a.L
        x_ms = timed(lambda: idx.search_range_exact_device(dq, r, cover))
        with idx.search_range_exact_device(dq, r, cover) as res:
            total, nb_used = res.total, res.nb_used
        leg = {"visited": visited, "max_buckets": plan["MAX_PER_QUERY"], "prune_ms": statistics.median(p_ms), "exact_ms": statistics.median(x_ms),
               "results": total, "nb_used": nb_used}
        b_txt = "not measured"
        if not a.no_brute:
            b_ms = timed(lambda: _capi.range_knn(dq, db, r, "ip"))
            with _capi.range_knn(dq, db, r, "ip") as res:
                assert res.total == total, f"the exact call returned {total} results, the brute force {res.total}"
            leg["brute_ms"] = statistics.median(b_ms)
            b_txt = fmt(b_ms)
        s_txt, nb = "not complete at any n_buckets", 1
        while True:
            with idx.search_range_device(dq, dq, nb, r) as res:
                complete = res.total == total
            if complete:
                s_ms = timed(lambda: idx.search_range_device(dq, dq, nb, r))
                leg["search_range_nb"], leg["search_range_ms"] = nb, statistics.median(s_ms)
                s_txt = f"{nb}, {fmt(s_ms)}"
                break
            if nb == a.L:
                break
            nb = min(a.L, nb * 2)
        result["legs"][f"target {t}"] = leg
        lines.append(f"{t:14d} | {visited:10.4f} | {plan['MAX_PER_QUERY']:5d} | {fmt(p_ms)} | {fmt(x_ms)} | {total:9d} | {b_txt} | {s_txt}")
    cover.close()
    idx.close()
    lines.append(json.dumps(result))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
