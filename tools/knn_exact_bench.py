#!/usr/bin/env python3
"""What the exact k-NN through the index costs and how much the covering balls prune (`Index.search_knn_exact`,
lmi_search_knn_exact), on tools/range_exact_bench.py's clustered synthetic data, generated on the device.

Data, per --sigmas value: --L unit centres in --d dimensions, --nb unit rows = normalise(centre + sigma * N(0, 1) / sqrt(d)), a row's
bucket = its centre; --nq queries = stored rows moved by the same noise.  Inner product.  The router of the `search_union` leg is the
best a one-layer model can be on this data: logits = <centre, q>.

Measured per (sigma, k), each after one warm-up, --reps runs, a host clock around the synchronising call, median (min .. max) in ms:
  exact        `search_knn_exact` on device tensors; beside it the mean buckets scored per query / L, the seed buckets per query, the
               queries whose radius stayed +inf and nb of the second scan (`knn_exact_last_plan`);
  prune        `cover_order_device` counting alone at the radii the exact call ends with (its k-th distances): the pruning pass
               without the scans -- the radii the call prunes with are these or larger;
  knn          `knn` (lmi_knn) over the same base on device tensors: the brute force, the time to beat;
  union        `search_union_device` at --union-nb buckets: NOT exact; its recall against the exact result is printed.
The exact result is compared with `knn`'s: the same ids per query as sets.

  python tools/knn_exact_bench.py [--nb 1000000] [--d 768] [--L 120] [--nq 1000] [--sigmas 0.3 0.5 0.7 1.0] [--ks 1 10 100 1000]
                                  [--reps 5] [--union-nb 4] [--out profiles/knn_exact.txt]

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
    ap.add_argument("--sigmas", type=float, nargs="+", default=[0.3, 0.5, 0.7, 1.0])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 10, 100, 1000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--union-nb", type=int, default=4)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert all(1 <= k <= _capi.UNION_MAX_K for k in a.ks) and a.nq <= a.nb and a.union_nb <= a.L

    import numpy as np
    import torch

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def timed(fn):
        return [clock(fn)[0] for rep in range(a.reps + 1)][1:]   # the first run warms up

    fmt = lambda v: f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"
    result = {"nb": a.nb, "d": a.d, "L": a.L, "nq": a.nq, "union_nb": a.union_nb, "legs": {}}
    lines = [f"# tools/knn_exact_bench.py: base {a.nb} x {a.d} in {a.L} buckets, {a.nq} queries, inner product, {a.reps} timed runs per leg "
             f"after one warm-up",
             f"# library: {_capi.lib().lmi_build_info().decode()}",
             f"# device: {torch.cuda.get_device_name(0)}",
             f"# sigma | k | visited (mean buckets / L) | seeds/query | tau = inf | nb rest | exact ms | prune ms | knn ms | "
             f"search_union({a.union_nb}) ms, recall"]
    unit = lambda x: x / x.norm(dim=1, keepdim=True)
    piece = 1 << 18
    for sigma in a.sigmas:
        gen = torch.Generator(device="cuda").manual_seed(a.seed)
        centres = unit(torch.randn((a.L, a.d), generator=gen, device="cuda"))
        lab = torch.randint(0, a.L, (a.nb,), generator=gen, device="cuda")
        db = torch.empty((a.nb, a.d), device="cuda", dtype=torch.float32)
        for lo in range(0, a.nb, piece):
            hi = min(a.nb, lo + piece)
            db[lo:hi] = unit(centres[lab[lo:hi]] + sigma / a.d ** 0.5 * torch.randn((hi - lo, a.d), generator=gen, device="cuda"))
        src = torch.randperm(a.nb, generator=gen, device="cuda")[: a.nq]
        dq = unit(db[src] + sigma / a.d ** 0.5 * torch.randn((a.nq, a.d), generator=gen, device="cuda")).contiguous()
        idx = _capi.Index(0)
        idx.set_mlp([(centres.cpu().numpy(), np.zeros(a.L, np.float32))])
        idx.buckets_begin(lab.cpu().numpy().astype(np.int64), a.d, a.L)   # ids: 1 .. nb, `knn`'s row numbers + 1
        for lo in range(0, a.nb, piece):
            idx.add_rows(db[lo: min(a.nb, lo + piece)], lo)
        idx.buckets_end()
        torch.cuda.synchronize()
        cover = _capi.Cover(idx)
        c_t = torch.zeros(a.nq, dtype=torch.int32, device="cuda")
        for k in a.ks:
            x_ms = timed(lambda: idx.search_knn_exact(dq, k, cover))
            dd, ii, cc, vv = idx.search_knn_exact(dq, k, cover)
            plan = _capi.knn_exact_last_plan()
            visited = float(vv.float().mean()) / a.L
            k_ms = timed(lambda: _capi.knn(dq, db, k, "ip"))
            _, rows = _capi.knn(dq, db, k, "ip")
            same = bool((torch.sort(ii.long(), dim=1).values == torch.sort(rows.long() + 1, dim=1).values).all())
            r = np.ascontiguousarray(dd[:, k - 1].cpu().numpy(), dtype=np.float32)
            p_ms = timed(lambda: idx.cover_order_device(dq, r, cover, 1, None, c_t))
            ud = torch.empty((a.nq, k), dtype=torch.float32, device="cuda")
            ui = torch.empty((a.nq, k), dtype=torch.int32, device="cuda")
            u_ms = timed(lambda: idx.search_union_device(dq, dq, a.union_nb, k, ud, ui))
            hit = (ui.long().unsqueeze(2) == ii.long().unsqueeze(1)).any(dim=2).float().mean().item() if k <= 100 else float(
                np.mean([len(set(x) & set(y)) / k for x, y in zip(ui.cpu().tolist(), ii.cpu().tolist())]))
            leg = {"visited": visited, "seeds_per_query": plan["SEED_BUCKETS"] / a.nq, "tau_inf": plan["TAU_INF"], "nb_rest": plan["NB_REST"],
                   "exact_ms": statistics.median(x_ms), "prune_ms": statistics.median(p_ms), "knn_ms": statistics.median(k_ms),
                   "union_ms": statistics.median(u_ms), "union_recall": hit, "equals_knn": same}
            result["legs"][f"sigma {sigma} k {k}"] = leg
            lines.append(f"{sigma:5.2f} | {k:4d} | {visited:7.4f} | {leg['seeds_per_query']:6.2f} | {plan['TAU_INF']:4d} | {plan['NB_REST']:4d} | "
                         f"{fmt(x_ms)} | {fmt(p_ms)} | {fmt(k_ms)} | {fmt(u_ms)}, {hit:.4f} | {'== knn' if same else 'DIFFERS from knn'}")
        cover.close()
        idx.close()
        del db, dq
        torch.cuda.empty_cache()
    lines.append(json.dumps(result))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
