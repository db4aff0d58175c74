#!/usr/bin/env python3
"""What a filter costs the union scan (lmi_search_union_filtered beside lmi_search_union on the same handle; developer aid).

On the benchmark's shape -- 10M x 768 unit-norm rows in 120 Gaussian clusters, 10 000 queries, the 4 most probable buckets each
(tools/union_bench.py's set-up: bench.py's c2 generator and an untrained routing model whose logits are the inner products with the
cluster centres) -- ms per batch, device tensors in and out, at k = 10 and 100, of

  lmi_search_union                                   the unfiltered call
  lmi_search_union_filtered, 100 % allowed           an empty drop list: every row passes the mask
  lmi_search_union_filtered, 50 % allowed            keep the even ids
  lmi_search_union_filtered, 1 % allowed             keep the ids that are multiples of 100
  lmi_search_union_filtered, 3 of 4 buckets emptied  one keep filter per bucket (its own ids); a query uses the filter of the first
                                                     bucket it visits, so its other three (filter, bucket) pairs allow no row and
                                                     their slots are skipped

and the time and the device bytes of making each filter set.  Nothing here is a pass/fail gate: a record of the machine it runs on.

  python tools/union_filter_bench.py                          # the full shape: about 80 GB of device memory
  python tools/union_filter_bench.py --n 400000 --nq 2000     # a quick look"""
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
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--steps", type=int, default=3, help="timed batches per row (after one warm-up batch)")
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
    cn = centres.cpu().numpy()
    layers = [(cn, np.full(L, float(np.linalg.norm(cn, axis=1).max()) + 1.0, np.float32)),
              (np.eye(L, dtype=np.float32), np.zeros(L, np.float32))]
    eng = _capi.Index(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.set_mlp(layers)
    labels_t = torch.empty(N, dtype=torch.int32, device=dev)
    for p in range(0, N, CHUNK):
        eng.mlp_topk_device(X[p: p + CHUNK], 1, labels_t[p: p + CHUNK])
    torch.cuda.synchronize()
    labels = labels_t.cpu().numpy().astype(np.int64)
    eng.buckets_begin(labels, d, L)
    for p in range(0, N, CHUNK):
        eng.add_rows(X[p: p + CHUNK], p)
        torch.cuda.synchronize()
    eng.buckets_end()
    del X
    torch.cuda.empty_cache()
    sizes = eng.bucket_sizes()
    print(f"# {N} x {d}, {L} buckets (sizes min/median/max {sizes.min()}/{int(np.median(sizes))}/{sizes.max()}), {nq} queries, n_buckets {nb}; "
          f"device tensors; {a.steps} timed batches per row after one warm-up; setup {time.time() - t0:.0f} s", flush=True)

    def timed(fn, steps):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / steps

    ids = np.arange(1, N + 1, dtype=np.uint32)   # the ids of a build without ids: 1-based row numbers
    bo = torch.empty((nq, nb), dtype=torch.int32, device=dev)
    eng.search_union_device(Q, Q, nb, 10, torch.empty((nq, 10), dtype=torch.float32, device=dev), torch.empty((nq, 10), dtype=torch.int32, device=dev),
                            None, bo)
    first = bo[:, 0].cpu().numpy().astype(np.int32)
    by_bucket = np.argsort(labels, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=L))])
    sets = (("100 % allowed", [ids[:0]], ["drop"], None),
            ("50 % allowed", [ids[ids % 2 == 0]], ["keep"], None),
            ("1 % allowed", [ids[ids % 100 == 0]], ["keep"], None),
            ("3 of 4 buckets emptied", [ids[by_bucket[cuts[b]: cuts[b + 1]]] for b in range(L)], ["keep"] * L, first))

    print("# call | k | ms per batch | vs unfiltered | mean results | slots scanned / skipped | filter set: filters, mask MiB, ms to make")
    base = {}
    for k in a.ks:
        d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        i_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
        c_t = torch.empty((nq,), dtype=torch.int32, device=dev)
        base[k] = timed(lambda: eng.search_union_device(Q, Q, nb, k, d_t, i_t, c_t, bo), a.steps)
        print(f"lmi_search_union | {k} | {base[k]:.2f} | 1.00 | {float(c_t.float().mean().item()):.1f} | |", flush=True)
    for name, lists, modes, fo in sets:
        t = time.perf_counter()
        filt = _capi.Filter(eng, lists, modes)
        make_ms = 1e3 * (time.perf_counter() - t)
        for k in a.ks:
            d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
            i_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
            c_t = torch.empty((nq,), dtype=torch.int32, device=dev)
            ms = timed(lambda: eng.search_union_device(Q, Q, nb, k, d_t, i_t, c_t, bo, filter=filt, filter_of=fo), a.steps)
            plan = _capi.filter_last_plan()
            print(f"lmi_search_union_filtered, {name} | {k} | {ms:.2f} | {ms / base[k]:.2f} | {float(c_t.float().mean().item()):.1f} | "
                  f"{plan['SLOTS']} / {plan['SKIPPED']} | {plan['FILTERS']}, {plan['MASK_BYTES'] / 2 ** 20:.1f}, {make_ms:.0f}", flush=True)
        filt.close()
    eng.set_stream(0)
    eng.close()


if __name__ == "__main__":
    main()
