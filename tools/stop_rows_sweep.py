#!/usr/bin/env python3
"""What the row-budget stop (lmi_set_stop_rows) buys: recall against work on a hard synthetic mixture (developer aid).

The mixture and the trained 1-level model of tools/stop_mass_sweep.py, and the [10, 10] tree of tools/path_mass_sweep.py.  Per
budget in {off and a few fractions of N}: recall@10 against brute force (lmi_knn), the mean number of buckets a query visits,
the mean and the maximum number of rows scanned per query, lmi_scan_stats' pairs and the per-batch phase times of
lmi_timings_mean (device-side stamps).  A record of the trade-off on the machine it runs on, not a pass/fail gate.

  python tools/stop_rows_sweep.py                        # 1 level: 4M x 64, 256 buckets, budget 8; tree: 2M x 64, [10, 10], budget 10
  python tools/stop_rows_sweep.py --n 200000 --nq 2000   # a quick look
  python tools/stop_rows_sweep.py --only tree
  python tools/stop_rows_sweep.py --inference-cost       # what the cut adds to LMI_T_INFERENCE, per ranking path and walk form"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.dirname(os.path.abspath(__file__))]

from path_mass_sweep import build_index, upload_tree  # noqa: E402
from stop_mass_sweep import train_model  # noqa: E402


def inference_cost(steps, seed):
    """LMI_T_INFERENCE with the stop off / on.  lmi_mlp_topk: bench.py's C2 (10 000 queries) and C1 (1 000) navigation shapes
    (768 -> 512 -> 120, n_buckets 4) and a 1 024-class model (the wide path), under each lmi_set_fused_mlp mode, over an index of
    64 objects per bucket on average (uniform random labels) -- budgets of 1.5 and 3 mean buckets.  lmi_nav_order: [10, 10] (queues in
    LDS) and [12, 12] (queues in global memory), n_buckets 10, budgets of 3 and 6 mean buckets.  Random weights."""
    import torch

    from learnedmetricindex_amd import _capi

    rs = np.random.RandomState(seed)
    dev = torch.device("cuda", 0)
    per = 64
    print("# shape | fused mode | LMI_T_INFERENCE us: off, rows 1.5 buckets, rows 3 buckets, rows 3 buckets + mass 0.999 | mean visited ranks at each")
    for name, nq, d, hidden, L in (("C2", 10_000, 768, 512, 120), ("C1", 1_000, 768, 512, 120), ("wide", 10_000, 768, 512, 1024)):
        layers = [((rs.randn(hidden, d) / np.sqrt(d)).astype(np.float32), (0.1 * rs.randn(hidden)).astype(np.float32)),
                  ((6.0 * rs.randn(L, hidden) / np.sqrt(hidden)).astype(np.float32), (0.1 * rs.randn(L)).astype(np.float32))]
        q = torch.from_numpy(rs.randn(nq, d).astype(np.float32)).to(dev)
        bo = torch.empty((nq, 4), dtype=torch.int32, device=dev)
        eng = _capi.Index(0)
        eng.set_mlp(layers)
        eng.set_buckets(rs.randn(L * per, 8).astype(np.float32), rs.randint(0, L, L * per), L)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        for mode in (0, 1, 2):
            eng.set_fused_mlp(mode)
            us, visited = [], []
            for rows, mass in ((0, 0.0), (per * 3 // 2, 0.0), (per * 3, 0.0), (per * 3, 0.999)):
                eng.set_stop_rows(rows)
                eng.set_stop_mass(mass)
                for _ in range(5):
                    eng.mlp_topk_device(q, 4, bo)
                eng.timings_reset()
                for _ in range(steps):
                    eng.mlp_topk_device(q, 4, bo)
                ms, _ = eng.timings_mean()
                us.append(1e3 * float(ms[_capi.T_INFERENCE]))
                visited.append(float((bo >= 0).sum(dim=1).float().mean().item()))
            print(f"{name:>5} nq {nq:>6} L {L:>5} | {mode} | " + ", ".join(f"{v:.1f}" for v in us) + " | " + ", ".join(f"{v:.2f}" for v in visited), flush=True)
        eng.set_stream(0)
        eng.close()
    d, hidden, nq, nb = 96, 128, 10_000, 10
    print("# tree | LMI_T_INFERENCE us of lmi_nav_order: off, rows 3 buckets, rows 6 buckets, rows 6 buckets + path mass 0.99 | mean recorded buckets at each")

    def model(n_out):
        return [((rs.randn(hidden, d) / np.sqrt(d)).astype(np.float32), (0.1 * rs.randn(hidden)).astype(np.float32)),
                ((3.0 * rs.randn(n_out, hidden) / np.sqrt(hidden)).astype(np.float32), (0.1 * rs.randn(n_out)).astype(np.float32))]

    for n0, n1 in ((10, 10), (12, 12)):
        eng = _capi.Index(0)
        upload_tree(eng, model(n0), [model(n1) for _ in range(n0)], [(c, j) for c in range(n0) for j in range(n1)])
        L = n0 * n1
        eng.set_buckets(rs.randn(L * per, 8).astype(np.float32), rs.randint(0, L, L * per), L)
        Q = rs.randn(nq, d).astype(np.float32)
        us, visited = [], []
        for rows, mass in ((0, 0.0), (per * 3, 0.0), (per * 6, 0.0), (per * 6, 0.99)):
            eng.set_stop_rows(rows)
            eng.set_path_mass(mass)
            for _ in range(3):
                eng.nav_order(Q, nb)
            eng.timings_reset()
            for _ in range(steps):
                slab, ent = eng.nav_order(Q, nb)
            ms, _ = eng.timings_mean()
            us.append(1e3 * float(ms[_capi.T_INFERENCE]))
            visited.append(float((ent >= 0).sum(axis=1).mean()))
        print(f"[{n0}, {n1}] | " + ", ".join(f"{v:.1f}" for v in us) + " | " + ", ".join(f"{v:.2f}" for v in visited), flush=True)
        eng.close()


def sweep(eng, search, Q, truth, rq, rk, nb, n_objects, fractions, steps):
    """One table: `search()` -> (ids, slab bucket ids [nq, nb] with -1 behind the stop)."""
    from learnedmetricindex_amd import _capi

    sizes = eng.bucket_sizes().astype(np.int64)
    print(f"# rows (fraction of N) | recall@{rk} | visited buckets per query | rows scanned per query: mean, max | scan pairs | "
          "ms per batch: total, inference, pass 2, rescore | held MHz")
    for frac in fractions:
        rows = 0 if frac == 0 else max(1, int(round(frac * n_objects)))
        eng.set_stop_rows(rows)
        for _ in range(3):
            search()
        eng.timings_reset()
        for _ in range(steps):
            ids, slab = search()
        ms, calls = eng.timings_mean()
        pairs = eng.scan_stats()[1]
        scanned = np.where(slab >= 0, sizes[np.clip(slab, 0, None)], 0).sum(axis=1)
        if int(scanned.sum()) != pairs:
            sys.exit(f"rows {rows}: lmi_scan_stats reports {pairs} pairs, the visited buckets hold {int(scanned.sum())}")
        recall = float(np.mean([len(set(t) & set(f)) / float(rk) for t, f in zip(truth.tolist(), ids[:rq].tolist())]))
        label = "off" if rows == 0 else f"{rows} ({frac:g})"
        print(f"{label:>18} | {recall:.4f} | {(slab >= 0).sum(axis=1).mean():.3f} | {scanned.mean():.0f}, {scanned.max()} | {pairs} | "
              f"{ms[_capi.T_TOTAL]:.3f}, {ms[_capi.T_INFERENCE]:.3f}, {ms[_capi.T_PF_EMIT]:.3f}, {ms[_capi.T_RESCORE]:.3f} | "
              f"{ms[_capi.T_CLOCK_MHZ]:.0f}   ({calls} calls)", flush=True)
    eng.set_stop_rows(0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=4_000_000, help="objects of the 1-level index (the tree takes half)")
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--leaves", type=int, default=256)
    ap.add_argument("--cats", type=int, nargs=2, default=[10, 10], help="the tree: classes of the root and of every node model")
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nb", type=int, default=8, help="bucket budget per query (n_buckets) of the 1-level index")
    ap.add_argument("--nb-tree", type=int, default=10, help="bucket budget per query of the tree")
    ap.add_argument("--spread", type=float, default=1.3, help="cluster noise of synth.mixture (1.0: well separated)")
    ap.add_argument("--model", default="MLP")
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.0, 0.005, 0.01, 0.02, 0.03], help="budgets as fractions of N; 0 = off")
    ap.add_argument("--only", choices=("both", "flat", "tree"), default="both")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--inference-cost", action="store_true", help="only: LMI_T_INFERENCE with the stop on / off (see inference_cost)")
    a = ap.parse_args()
    if a.inference_cost:
        inference_cost(max(a.steps, 50), a.seed)
        return
    import synth

    from learnedmetricindex_amd import _capi

    rk = 10
    rq = min(a.recall_queries, a.nq)
    if a.only in ("both", "flat"):
        t0 = time.time()
        X, Q = synth.mixture(a.seed, a.n, a.d, a.leaves, a.nq, spread=a.spread)
        layers = train_model(X, a.leaves, a.model, min(a.train_rows, a.n), a.epochs, a.seed)
        eng = _capi.Index(0)
        eng.set_mlp(layers)
        labels = np.concatenate([eng.mlp_topk(X[r0: r0 + (1 << 18)], 1)[:, 0] for r0 in range(0, a.n, 1 << 18)]).astype(np.int64)
        eng.set_buckets(X, labels, a.leaves)
        sizes = eng.bucket_sizes()
        _, truth = _capi.knn(Q[:rq], X, rk, "ip")
        print(f"# 1 level: {a.n} x {a.d}, {a.leaves} buckets (sizes min/median/max {sizes.min()}/{int(np.median(sizes))}/{sizes.max()}), spread {a.spread}, "
              f"{a.nq} queries, n_buckets {a.nb}, k {rk}; recall@{rk} over {rq} queries; {a.steps} timed batches per row; setup {time.time() - t0:.0f} s")

        def flat():
            _, ids, bo = eng.search(Q, Q, a.nb, rk)
            return ids, bo

        sweep(eng, flat, Q, truth + 1, rq, rk, a.nb, a.n, a.fractions, a.steps)   # ids are 1-based row numbers
        eng.close()
    if a.only in ("both", "tree"):
        t0 = time.time()
        b = SimpleNamespace(**vars(a))
        b.n = max(a.n // 2, 1000)
        eng, X, Q, root, nodes, child_bucket = build_index(b)
        sizes = eng.bucket_sizes()
        _, truth = _capi.knn(Q[:rq], X, rk, "ip")
        print(f"# tree {a.cats}: {b.n} x {a.d}, {sizes.size} buckets with objects (sizes min/median/max {sizes.min()}/{int(np.median(sizes))}/{sizes.max()}), "
              f"spread {a.spread}, {a.nq} queries, n_buckets {a.nb_tree}, k {rk}; recall@{rk} over {rq} queries; {a.steps} timed batches per row; "
              f"setup {time.time() - t0:.0f} s")

        def tree():
            _, ids, slab, _ = eng.search_tree(Q, Q, a.nb_tree, rk, want_order=True)
            return ids, slab

        sweep(eng, tree, Q, truth + 1, rq, rk, a.nb_tree, b.n, a.fractions, a.steps)
        eng.close()


if __name__ == "__main__":
    main()
