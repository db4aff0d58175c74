#!/usr/bin/env python3
"""What the path-mass stop of the multi-level walk (lmi_set_path_mass) buys: recall against work on a synthetic 2-level index
(developer aid).

A mixture of overlapping Gaussian clusters from tests/golden/synth.py, a root model trained on k-means labels and one model
per root class trained on k-means labels of the objects the root places there (the way tools/stop_mass_sweep.py trains its
1-level model), the index built from the models' placement.  Per mass in {off, 0.8, 0.9, 0.99, 0.999}: recall@10 against
brute force (lmi_knn_ip), the mean number of buckets a query visits, lmi_scan_stats' pairs, the number of walk steps that
still had queries waiting for a model (and the mean number of node models a query is evaluated by) and the per-batch times
of lmi_timings_mean (device-side stamps).  The step counts come from a vectorised numpy restatement of the walk over the
device's own probabilities (lmi_mlp_proba per model); the device's order must equal the restatement's, or the run stops.
A record of the trade-off on the machine it runs on, not a pass/fail gate.

  python tools/path_mass_sweep.py                        # 2M x 64, [10, 10], 10 000 queries, budget 10
  python tools/path_mass_sweep.py --n 200000 --nq 2000   # a quick look
  python tools/path_mass_sweep.py --walk-cost            # LMI_T_INFERENCE of lmi_nav_order, mass forms against the plain ones"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tools")]

from stop_mass_sweep import train_model  # noqa: E402


def upload_tree(eng, root, nodes, paths_with_rows):
    """Root + one model per root class; child (0, c) -> model c + 1, child (c + 1, j) -> bucket (c, j) or, when the placement
    left it without objects, a listed bucket without objects (-1).  Returns the slab bucket id of every (c, j)."""
    eng.set_mlp(root)
    n0, n1 = len(nodes), nodes[0][-1][0].shape[0]
    for c, layers in enumerate(nodes):
        eng.nav_set_model(c + 1, layers)
    bucket_id = {p: i for i, p in enumerate(paths_with_rows)}
    offset = [0, n0]
    child_model = [c + 1 for c in range(n0)]
    child_bucket = [-2] * n0
    for c in range(n0):
        child_model += [-1] * n1
        child_bucket += [bucket_id.get((c, j), -1) for j in range(n1)]
        offset.append(len(child_model))
    eng.nav_set_tree(offset, child_model, child_bucket)
    return np.asarray(child_bucket, dtype=np.int64)


def probabilities(root, nodes, Q):
    """lmi_mlp_proba of every model over all queries: [(probs descending, classes)], the root first."""
    from learnedmetricindex_amd import _capi

    out = []
    for layers in [root] + list(nodes):
        m = _capi.Index(0)
        m.set_mlp(layers)
        out.append(m.mlp_proba(Q))
        m.close()
    return out


def walk_numpy(P, child_bucket, nb, mass):
    """The walk of a 2-level tree for all queries at once (include/lmi_hip.h: lmi_set_path_mass).  Returns (entries [nq, nb] with
    -1 behind the stop, model evaluations per query [nq])."""
    (rp, rc), nodes = P[0], P[1:]
    nq, n0, n1 = rp.shape[0], rp.shape[1], nodes[0][0].shape[1]
    cap = n0 + n0 * n1
    prio = np.zeros((nq, cap), dtype=np.float32)
    pm = np.zeros((nq, cap), dtype=np.float32)
    ent = np.full((nq, cap), -1, dtype=np.int64)
    prio[:, :n0] = rp[:, ::-1]                    # least probable first
    pm[:, :n0] = rp[:, ::-1]
    ent[:, :n0] = rc[:, ::-1]
    length = np.full(nq, n0)
    have = np.zeros(nq, dtype=np.int64)
    cum = np.zeros(nq, dtype=np.float32)
    evals = np.zeros(nq, dtype=np.int64)
    out = np.full((nq, nb), -1, dtype=np.int64)
    live = np.ones(nq, dtype=bool)
    limit = np.float32(mass)
    rows = np.arange(nq)
    while live.any():
        q = rows[live]
        key = np.where(ent[q] >= 0, prio[q], np.float32(-1))
        best = cap - 1 - np.argmax(key[:, ::-1], axis=1)      # the later entry wins a tie
        e, m = ent[q, best], pm[q, best]
        ent[q, best] = -1
        node = e < n0
        qn, cn, mn = q[node], e[node], m[node]                 # expand: children most probable first
        for c in np.unique(cn):
            s = cn == c
            pr, cl = nodes[c]
            cols = length[qn[s]][:, None] + np.arange(n1)[None, :]
            prio[qn[s][:, None], cols] = pr[qn[s]]
            pm[qn[s][:, None], cols] = mn[s][:, None] * pr[qn[s]]
            ent[qn[s][:, None], cols] = n0 + c * n1 + cl[qn[s]]
        length[qn] += n1
        evals[qn] += 1
        qb, eb, mb = q[~node], e[~node], m[~node]              # record a bucket
        out[qb, have[qb]] = eb
        cum[qb] = np.where(have[qb] == 0, mb, cum[qb] + mb)
        have[qb] += 1
        done = have[qb] >= nb
        if mass > 0:
            done |= ~(cum[qb] < limit)
        live[qb[done]] = False
    return out, evals


def build_index(a):
    import synth

    from learnedmetricindex_amd import _capi

    n0, n1 = a.cats
    X, Q = synth.mixture(a.seed, a.n, a.d, n0 * n1, a.nq, spread=a.spread)
    root = train_model(X, n0, a.model, min(a.train_rows, a.n), a.epochs, a.seed)
    m = _capi.Index(0)
    m.set_mlp(root)
    top = np.concatenate([m.mlp_topk(X[r0: r0 + (1 << 18)], 1)[:, 0] for r0 in range(0, a.n, 1 << 18)]).astype(np.int64)
    m.close()
    nodes, low = [], np.zeros(a.n, dtype=np.int64)
    for c in range(n0):
        sel = np.flatnonzero(top == c)
        assert sel.size >= n1, f"root class {c} received {sel.size} objects"
        layers = train_model(X[sel], n1, a.model, min(a.train_rows, sel.size), a.epochs, a.seed + 1 + c)
        m = _capi.Index(0)
        m.set_mlp(layers)
        low[sel] = np.concatenate([m.mlp_topk(X[sel[r0: r0 + (1 << 18)]], 1)[:, 0] for r0 in range(0, sel.size, 1 << 18)])
        m.close()
        nodes.append(layers)
    flat = top * n1 + low
    used, bucket_of = np.unique(flat, return_inverse=True)
    eng = _capi.Index(0)
    child_bucket = upload_tree(eng, root, nodes, [(int(f) // n1, int(f) % n1) for f in used])
    eng.set_buckets(X, np.asarray(bucket_of).reshape(-1), used.size)
    return eng, X, Q, root, nodes, child_bucket


def walk_cost(a):
    """LMI_T_INFERENCE of lmi_nav_order with the mass forms (mass 0.9999: almost nobody is cut, so the walk is the same) against
    the plain ones, 10 000 queries, at [10, 10] (queues in LDS) and [12, 12] (queues in global memory).  Random models; the
    two settings alternate, `--steps` timed calls per turn, three turns each."""
    from learnedmetricindex_amd import _capi

    rs = np.random.RandomState(a.seed)
    d, hidden, nq, nb = 96, 128, 10_000, 10
    print("# tree | LMI_T_INFERENCE us per call, three alternating turns: off / mass 0.9999 | queries cut at 0.9999   (held clock: not stamped, "
          "lmi_nav_order runs no scan and only the scan carries the clock stamp)")

    def model(n_out):
        return [((rs.randn(hidden, d) / np.sqrt(d)).astype(np.float32), (0.1 * rs.randn(hidden)).astype(np.float32)),
                ((3.0 * rs.randn(n_out, hidden) / np.sqrt(hidden)).astype(np.float32), (0.1 * rs.randn(n_out)).astype(np.float32))]

    for n0, n1 in ((10, 10), (12, 12)):
        eng = _capi.Index(0)
        upload_tree(eng, model(n0), [model(n1) for _ in range(n0)], [(c, j) for c in range(n0) for j in range(n1)])
        Q = rs.randn(nq, d).astype(np.float32)
        turns = {0.0: [], 0.9999: []}
        cut = 0
        for _ in range(3):
            for mass in (0.0, 0.9999):
                eng.set_path_mass(mass)
                for _ in range(3):
                    eng.nav_order(Q, nb)
                eng.timings_reset()
                for _ in range(a.steps):
                    slab, ent = eng.nav_order(Q, nb)
                ms, _ = eng.timings_mean()
                turns[mass].append(1e3 * float(ms[_capi.T_INFERENCE]))
                if mass:
                    cut = int((ent[:, -1] < 0).sum())
        fmt = lambda v: ", ".join(f"{x:.1f}" for x in v)  # noqa: E731
        print(f"[{n0}, {n1}] | {fmt(turns[0.0])} / {fmt(turns[0.9999])} | {cut} of {nq}", flush=True)
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--cats", type=int, nargs=2, default=[10, 10], help="classes of the root and of every node model")
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nb", type=int, default=10, help="bucket budget per query (n_buckets)")
    ap.add_argument("--spread", type=float, default=1.3, help="cluster noise of synth.mixture (1.0: well separated)")
    ap.add_argument("--model", default="MLP")
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--recall-k", type=int, default=10, help="k of the searches and of recall@k, 1..64; other than 10: the truth comes from lmi_knn")
    ap.add_argument("--masses", type=float, nargs="+", default=[0.0, 0.8, 0.9, 0.99, 0.999], help="0 = off")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--walk-cost", action="store_true", help="only: LMI_T_INFERENCE of the walk, mass forms against the plain ones (see walk_cost)")
    a = ap.parse_args()
    if a.walk_cost:
        a.steps = max(a.steps, 50)
        walk_cost(a)
        return
    from learnedmetricindex_amd import _capi

    t0 = time.time()
    eng, X, Q, root, nodes, child_bucket = build_index(a)
    sizes = eng.bucket_sizes()
    rq = min(a.recall_queries, a.nq)
    rk = a.recall_k
    if not 1 <= rk <= 64:
        sys.exit("--recall-k must be in 1..64 (LMI_MAX_K)")
    _, truth = _capi.knn_ip(Q[:rq], X, 10) if rk == 10 else _capi.knn(Q[:rq], X, rk, "ip")
    truth = truth + 1   # ids are 1-based row numbers
    P = probabilities(root, nodes, Q)
    print(f"# {a.n} x {a.d}, tree {a.cats}: {sizes.size} buckets with objects (sizes min/median/max {sizes.min()}/{int(np.median(sizes))}/{sizes.max()}), "
          f"spread {a.spread}, {a.nq} queries, n_buckets {a.nb}, k {rk}; recall@{rk} over {rq} queries; {a.steps} timed batches per row; setup {time.time() - t0:.0f} s")
    print(f"# mass | recall@{rk} | visited buckets per query | scan pairs | walk steps with waiting queries (node models per query) | "
          "ms per batch: total, inference, pass 2, rescore | held MHz")
    for mass in a.masses:
        eng.set_path_mass(mass)
        for _ in range(3):
            eng.search_tree(Q, Q, a.nb, rk)
        eng.timings_reset()
        for _ in range(a.steps):
            _, ids, slab, ent = eng.search_tree(Q, Q, a.nb, rk, want_order=True)
        ms, calls = eng.timings_mean()
        pairs = eng.scan_stats()[1]
        want, evals = walk_numpy(P, child_bucket, a.nb, mass)
        if not np.array_equal(want, ent):
            sys.exit(f"mass {mass}: the device's order differs from the restatement in {(want != ent).any(axis=1).sum()} of {a.nq} queries")
        recall = float(np.mean([len(set(t) & set(f)) / float(rk) for t, f in zip(truth.tolist(), ids[:rq].tolist())]))
        print(f"{'off' if mass == 0 else mass:>6} | {recall:.4f} | {(ent >= 0).sum(axis=1).mean():.3f} | {pairs} | {int(evals.max())} ({evals.mean():.2f}) | "
              f"{ms[_capi.T_TOTAL]:.3f}, {ms[_capi.T_INFERENCE]:.3f}, {ms[_capi.T_PF_EMIT]:.3f}, {ms[_capi.T_RESCORE]:.3f} | "
              f"{ms[_capi.T_CLOCK_MHZ]:.0f}   ({calls} calls)", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
