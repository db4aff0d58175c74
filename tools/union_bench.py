#!/usr/bin/env python3
"""What the union scan (merge="union": lmi_search_union) costs beside the calls it sits between (developer aid).

On the benchmark's shape -- 10M x 768 unit-norm rows in 120 Gaussian clusters, 10 000 queries, the 4 most probable buckets each
(bench.py's c2 generator; the routing model here is not trained: its logits are the inner products with the cluster centres, which
sends an object to its cluster and a query to the 4 nearest) -- ms per batch, device tensors in and out, of

  lmi_search_union at k = 10, 100, 1000      f32 work on the visited 4 / 120 of the base, exact top-k of their union
  lmi_knn at k = 10                          exact brute force over the whole base (the ground truth of recall@k)
  lmi_search at k = 10, prefilter mode       fp16 prefilter + exact re-rank, at most 10 per bucket (the default scan)
  lmi_search at k = 10, all-f32 mode         lmi_set_prefilter(0)

and recall@k of the union results against lmi_knn over the first --recall-queries queries.  lmi_knn, lmi_search and both of its
modes are the code the union scan was added beside; nothing here is a pass/fail gate.  A record of the machine it runs on.

The sharded leg (profiles/union_sharded.txt) follows the union rows on the same index and bucket order, batches timed one by one:
lmi_scan_union and lmi_scan_union_part (a rank's part: the same launches, five planes written instead of two), and
lmi_merge_union_parts alone on the parts of emulated worlds of 2 and 8 ranks (rank r owns the buckets b with b % world == r).

  python tools/union_bench.py                          # the full shape: about 80 GB of device memory
  python tools/union_bench.py --n 400000 --nq 2000     # a quick look"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

CHUNK = 1 << 18


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--leaves", type=int, default=120)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nb", type=int, default=4)
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--steps", type=int, default=3, help="timed batches per row (after one warm-up batch)")
    ap.add_argument("--recall-queries", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2023)
    a = ap.parse_args()
    import torch

    from learnedmetricindex_amd import _capi

    dev = torch.device("cuda", 0)
    N, d, L, nq, nb = a.n, a.d, a.leaves, a.nq, a.nb
    t0 = time.time()
    centres = torch.randn(L, d, generator=torch.Generator().manual_seed(a.seed)).to(dev)

    def gen_rows(tag, piece, n):
        g = torch.Generator(device=dev).manual_seed(a.seed * 1_000_003 + tag * 100_003 + piece)
        c = torch.randint(0, L, (n,), generator=g, device=dev)
        return torch.nn.functional.normalize(centres[c] + torch.randn(n, d, generator=g, device=dev), dim=1).contiguous()

    X = torch.empty((N, d), dtype=torch.float32, device=dev)
    for p in range(0, N, CHUNK):
        X[p: p + CHUNK] = gen_rows(1, p // CHUNK, min(CHUNK, N - p))
    Q = gen_rows(7, 0, nq)
    # logits = <x, centre> + max |centre| + 1 through a ReLU that never clips (|<x, centre>| <= |centre|) and an identity layer
    cn = centres.cpu().numpy()
    layers = [(cn, np.full(L, float(np.linalg.norm(cn, axis=1).max()) + 1.0, np.float32)),
              (np.eye(L, dtype=np.float32), np.zeros(L, np.float32))]

    def build(prefilter):
        eng = _capi.Index(0, prefilter=prefilter)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.set_mlp(layers)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        for p in range(0, N, CHUNK):
            eng.mlp_topk_device(X[p: p + CHUNK], 1, labels[p: p + CHUNK])
        torch.cuda.synchronize()
        eng.buckets_begin(labels.cpu().numpy().astype(np.int64), d, L)
        for p in range(0, N, CHUNK):
            eng.add_rows(X[p: p + CHUNK], p)
            torch.cuda.synchronize()
        eng.buckets_end()
        return eng

    def timed(fn, steps):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / steps

    eng = build(True)
    sizes = eng.bucket_sizes()
    print(f"# {N} x {d}, {L} buckets (sizes min/median/max {sizes.min()}/{int(np.median(sizes))}/{sizes.max()}), {nq} queries, n_buckets {nb}; "
          f"device tensors; {a.steps} timed batches per row after one warm-up; setup {time.time() - t0:.0f} s", flush=True)
    rq = min(a.recall_queries, nq)
    kmax = max(a.ks)
    t = time.perf_counter()
    _, truth = _capi.knn(Q[:rq], X, kmax, "ip")
    truth = truth.cpu().numpy() + 1   # ids are 1-based row numbers
    print(f"# ground truth: lmi_knn, {rq} queries, k {kmax}: {1e3 * (time.perf_counter() - t):.1f} ms", flush=True)

    print("# call | k | ms per batch | recall@k | plan")
    bo = torch.empty((nq, nb), dtype=torch.int32, device=dev)
    for k in a.ks:
        d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        i_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
        c_t = torch.empty((nq,), dtype=torch.int32, device=dev)
        ms = timed(lambda: eng.search_union_device(Q, Q, nb, k, d_t, i_t, c_t, bo), a.steps)
        plan = _capi.union_last_plan()
        got = i_t[:rq].cpu().numpy().view(np.uint32)
        recall = float(np.mean([len(set(t_) & set(f)) / float(k) for t_, f in zip(truth[:, :k].tolist(), got.tolist())]))
        print(f"lmi_search_union | {k} | {ms:.2f} | {recall:.4f} | groups {plan['GROUPS']} waves {plan['WAVES']} slab {plan['SLAB_BYTES'] >> 20} MiB "
              f"workspace {plan['WORKSPACE_BYTES'] >> 20} MiB; mean results {float(c_t.float().mean().item()):.1f}", flush=True)

    # ---- the sharded leg: a rank's part beside lmi_scan_union, and the merge kernel alone for emulated worlds ----
    def timed_each(fn, steps):
        """(min, mean, max) ms over `steps` batches timed one by one, after one warm-up batch."""
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        return min(ms), sum(ms) / len(ms), max(ms)

    print("# sharded leg: call | k | ms per batch min / mean / max | note")
    steps = max(a.steps, 5)
    for k in a.ks:
        d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        i_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
        c_t = torch.empty((nq,), dtype=torch.int32, device=dev)
        part = torch.empty((5, nq, k), dtype=torch.int32, device=dev)
        c_p = torch.empty((nq,), dtype=torch.int32, device=dev)
        lo, mean, hi = timed_each(lambda: eng.scan_union_device(Q, bo, nb, k, d_t, i_t, c_t), steps)
        print(f"lmi_scan_union | {k} | {lo:.2f} / {mean:.2f} / {hi:.2f} |", flush=True)
        lo, mean, hi = timed_each(lambda: eng.scan_union_part_device(Q, bo, nb, k, part, c_p), steps)
        ok = torch.equal(part[1], d_t.view(torch.int32)) and torch.equal(part[2], i_t) and torch.equal(c_p, c_t)
        print(f"lmi_scan_union_part | {k} | {lo:.2f} / {mean:.2f} / {hi:.2f} | dist, id, counts {'equal' if ok else 'DIFFER from'} lmi_scan_union's",
              flush=True)
        for world in (2, 8):
            # rank r of the emulated world owns the buckets b with b % world == r: the others are struck out of its order, which is what
            # an `owned` mask does to them (no rows), and leaves every rank t where it is
            parts = torch.empty((world, 5, nq, k), dtype=torch.int32, device=dev)
            for r in range(world):
                eng.scan_union_part_device(Q, torch.where(bo % world == r, bo, torch.full_like(bo, -1)), nb, k, parts[r])
            m_d, m_i, m_c = torch.empty_like(d_t), torch.empty_like(i_t), torch.empty_like(c_t)
            lo, mean, hi = timed_each(lambda: eng.merge_union_parts(parts, world, nq, k, m_d, m_i, m_c), steps)
            ok = torch.equal(m_d.view(torch.int32), d_t.view(torch.int32)) and torch.equal(m_i, i_t) and torch.equal(m_c, c_t)
            print(f"lmi_merge_union_parts, world {world} | {k} | {lo:.3f} / {mean:.3f} / {hi:.3f} | {world * 20 * nq * k >> 20} MiB of parts; "
                  f"{'equal to' if ok else 'DIFFERS from'} lmi_scan_union", flush=True)
            del parts

    d_t = torch.empty((nq, 10), dtype=torch.float32, device=dev)
    i_t = torch.empty((nq, 10), dtype=torch.int32, device=dev)

    def search_row(e, what):
        ms = timed(lambda: e.search_device(Q, Q, nb, 10, d_t, i_t, None, bo), max(a.steps, 10))
        got = i_t[:rq].cpu().numpy().view(np.uint32)
        recall = float(np.mean([len(set(t_) & set(f)) / 10.0 for t_, f in zip(truth[:, :10].tolist(), got.tolist())]))
        print(f"lmi_search, {what} | 10 | {ms:.2f} | {recall:.4f} |", flush=True)

    search_row(eng, "prefilter")
    eng.set_stream(0)
    eng.close()
    eng = build(False)
    search_row(eng, "all-f32")
    eng.set_stream(0)
    eng.close()
    torch.cuda.empty_cache()
    t = time.perf_counter()
    _capi.knn(Q, X, 10, "ip")
    print(f"lmi_knn, whole base | 10 | {1e3 * (time.perf_counter() - t):.2f} | 1.0000 | {_capi.knn_last_plan()}", flush=True)


if __name__ == "__main__":
    main()
