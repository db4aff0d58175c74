#!/usr/bin/env python3
"""What the probability-mass stop (lmi_set_stop_mass) buys: recall against work on a hard synthetic mixture (developer aid).

A mixture of overlapping Gaussian clusters from tests/golden/synth.py (`--spread` > 1: the clusters run into each other, so
the navigation model is often unsure), a model trained on k-means labels the way bench.py trains its own, the index built
from the model's placement.  Per mass in {off, 0.9, 0.99, 0.999}: recall@10 against brute force (lmi_knn_ip), the mean
number of buckets a query visits, lmi_scan_stats' pairs and the per-batch times of lmi_timings_mean (device-side stamps).
A record of the trade-off on the machine it runs on, not a pass/fail gate.

  python tools/stop_mass_sweep.py                      # 4M x 64, 256 buckets, 10 000 queries, budget 8
  python tools/stop_mass_sweep.py --n 200000 --nq 2000 # a quick look
  python tools/stop_mass_sweep.py --n 8000000 --leaves 128   # larger buckets: pass 2 is most of a batch
  python tools/stop_mass_sweep.py --inference-cost     # what the cut adds to LMI_T_INFERENCE at the C2 / C1 shapes, per ranking path"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]


def train_model(X, L, model_type, train_rows, epochs, seed):
    """k-means labels on a sample (10 Lloyd iterations on unit vectors) -> full-batch Adam / cross entropy, as bench.py does."""
    import torch

    from learnedmetricindex_amd.li.model import NeuralNetwork, linear_layers

    net = NeuralNetwork(input_dim=X.shape[1], output_dim=L, lr=0.01, model_type=model_type)
    torch.manual_seed(seed)
    xtr = torch.from_numpy(X[:train_rows]).to(net.device)
    cent = xtr[torch.randperm(xtr.shape[0], device=net.device)[:L]].clone()
    for _ in range(10):
        lab = (xtr @ cent.T).argmax(1)
        cent = torch.nn.functional.normalize(torch.zeros_like(cent).index_put_((lab,), xtr, accumulate=True), dim=1)
    net.train(xtr, (xtr @ cent.T).argmax(1), epochs=epochs)
    return linear_layers(net.model)


def inference_cost(steps, seed):
    """LMI_T_INFERENCE of lmi_mlp_topk with the stop off / on: bench.py's C2 (10 000 queries) and C1 (1 000) navigation shapes
    (768 -> 512 -> 120, n_buckets 4) and a 1 024-class model (the wide path), under each lmi_set_fused_mlp mode.  Random weights,
    the output layer scaled so that the queries stop after 1 .. 4 ranks."""
    import torch

    from learnedmetricindex_amd import _capi

    rs = np.random.RandomState(seed)
    dev = torch.device("cuda", 0)
    print("# shape | fused mode | LMI_T_INFERENCE us: off, mass 0.9, mass 0.999 | mean visited ranks at 0.9, 0.999")
    for name, nq, d, hidden, L in (("C2", 10_000, 768, 512, 120), ("C1", 1_000, 768, 512, 120), ("wide", 10_000, 768, 512, 1024)):
        layers = [((rs.randn(hidden, d) / np.sqrt(d)).astype(np.float32), (0.1 * rs.randn(hidden)).astype(np.float32)),
                  ((6.0 * rs.randn(L, hidden) / np.sqrt(hidden)).astype(np.float32), (0.1 * rs.randn(L)).astype(np.float32))]
        q = torch.from_numpy(rs.randn(nq, d).astype(np.float32)).to(dev)
        bo = torch.empty((nq, 4), dtype=torch.int32, device=dev)
        eng = _capi.Index(0)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.set_mlp(layers)
        for mode in (0, 1, 2):
            eng.set_fused_mlp(mode)
            us, visited = [], []
            for mass in (0.0, 0.9, 0.999):
                eng.set_stop_mass(mass)
                for _ in range(5):
                    eng.mlp_topk_device(q, 4, bo)
                eng.timings_reset()
                for _ in range(steps):
                    eng.mlp_topk_device(q, 4, bo)
                ms, _ = eng.timings_mean()
                us.append(1e3 * float(ms[_capi.T_INFERENCE]))
                visited.append(float((bo >= 0).sum(dim=1).float().mean().item()))
            print(f"{name:>5} nq {nq:>6} L {L:>5} | {mode} | {us[0]:.1f}, {us[1]:.1f}, {us[2]:.1f} | {visited[1]:.2f}, {visited[2]:.2f}", flush=True)
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--leaves", type=int, default=256)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nb", type=int, default=8, help="bucket budget per query (n_buckets)")
    ap.add_argument("--spread", type=float, default=1.3, help="cluster noise of synth.mixture (1.0: well separated; 1.3: a full budget of 8 finds ~96 %% of the neighbours)")
    ap.add_argument("--model", default="MLP")
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--recall-k", type=int, default=10, help="k of the searches and of recall@k, 1..64; other than 10: the truth comes from lmi_knn")
    ap.add_argument("--masses", type=float, nargs="+", default=[0.0, 0.9, 0.99, 0.999], help="0 = off")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--inference-cost", action="store_true", help="only: LMI_T_INFERENCE with the stop on / off (see inference_cost)")
    a = ap.parse_args()
    if a.inference_cost:
        inference_cost(max(a.steps, 50), a.seed)
        return
    import synth

    from learnedmetricindex_amd import _capi

    t0 = time.time()
    X, Q = synth.mixture(a.seed, a.n, a.d, a.leaves, a.nq, spread=a.spread)
    layers = train_model(X, a.leaves, a.model, min(a.train_rows, a.n), a.epochs, a.seed)
    eng = _capi.Index(0)
    eng.set_mlp(layers)
    labels = np.concatenate([eng.mlp_topk(X[r0: r0 + (1 << 18)], 1)[:, 0] for r0 in range(0, a.n, 1 << 18)]).astype(np.int64)
    eng.set_buckets(X, labels, a.leaves)
    sizes = eng.bucket_sizes()
    rq = min(a.recall_queries, a.nq)
    rk = a.recall_k
    if not 1 <= rk <= 64:
        sys.exit("--recall-k must be in 1..64 (LMI_MAX_K)")
    _, truth = _capi.knn_ip(Q[:rq], X, 10) if rk == 10 else _capi.knn(Q[:rq], X, rk, "ip")
    truth = truth + 1   # ids are 1-based row numbers
    print(f"# {a.n} x {a.d}, {a.leaves} buckets (sizes min/median/max {sizes.min()}/{int(np.median(sizes))}/{sizes.max()}), spread {a.spread}, "
          f"{a.nq} queries, n_buckets {a.nb}, k {rk}; recall@{rk} over {rq} queries; {a.steps} timed batches per row; setup {time.time() - t0:.0f} s")
    print(f"# mass | recall@{rk} | visited buckets per query | scan pairs | ms per batch: total, inference, pass 2, rescore | held MHz")
    for mass in a.masses:
        eng.set_stop_mass(mass)
        for _ in range(3):
            eng.search(Q, Q, a.nb, rk)
        eng.timings_reset()
        for _ in range(a.steps):
            _, ids, bo = eng.search(Q, Q, a.nb, rk)
        ms, calls = eng.timings_mean()
        pairs = eng.scan_stats()[1]
        recall = float(np.mean([len(set(t) & set(f)) / float(rk) for t, f in zip(truth.tolist(), ids[:rq].tolist())]))
        print(f"{'off' if mass == 0 else mass:>6} | {recall:.4f} | {(bo >= 0).sum(axis=1).mean():.3f} | {pairs} | "
              f"{ms[_capi.T_TOTAL]:.3f}, {ms[_capi.T_INFERENCE]:.3f}, {ms[_capi.T_PF_EMIT]:.3f}, {ms[_capi.T_RESCORE]:.3f} | "
              f"{ms[_capi.T_CLOCK_MHZ]:.0f}   ({calls} calls)", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
