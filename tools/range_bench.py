#!/usr/bin/env python3
"""What the range search (lmi_search_range) costs beside the union scan it shares its score stage with (developer aid).

On tools/union_bench.py's shape -- 10M x 768 unit-norm rows in 120 Gaussian clusters, 10 000 queries, the 4 most probable buckets each;
the routing model's logits are the inner products with the cluster centres -- ms per batch, device tensors in, batches timed one by
one after one warm-up, in ONE run on one index:

  lmi_search_union at k = 10 and k = 1000        the call beside it: pack, score, select, merge
  lmi_search_range, per-query radii              radius[q] = the query's k-th distance of the union call: k results per query
  lmi_search_range, one radius                   the median of those radii for every query: about k per query, uneven runs

A range row also says how many results came back (mean and max per query), the plan, and whether every query's run, stably sorted
by distance, begins with the union's ids.  Nothing here is a pass/fail gate.  A record of the machine it runs on.

The sharded leg (profiles/range_sharded.txt) follows on the same index and bucket order, batches timed one by one: lmi_scan_range on
the whole handle, the same call on the buckets of one rank of emulated worlds of 2 and 8 ranks (rank r owns the buckets b with
b % world == r; the slowest rank's row is printed), and lmi_join_range_parts alone on those ranks' parts, with what a padded all-gather
of them would move.  One card plays every rank; nothing is said about several GPUs.

The sort leg (--sort; profiles/range_sort.txt) runs INSTEAD of the rows above, on the same index: per-query radii that yield about
--sort-k results per query, then per repeat lmi_scan_range, lmi_range_result_sort on its result, and the host route to the same
order (read() and one stable argsort per query), each timed on its own; and one skewed result -- a single query that owns a segment
of --skew entries among the others' hundred -- so that the long form is timed.  Medians of the repeats; both sorts are compared with
numpy bit for bit.

  python tools/range_bench.py                          # the full shape: about 80 GB of device memory
  python tools/range_bench.py --n 400000 --nq 2000     # a quick look
  python tools/range_bench.py --sort                   # the sort leg alone"""
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
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 1000])
    ap.add_argument("--steps", type=int, default=5, help="timed batches per row (after one warm-up batch)")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--sort", action="store_true", help="run the sort leg (lmi_range_result_sort) instead of the other rows")
    ap.add_argument("--sort-k", type=int, default=100, help="sort leg: results per query (the radius is the query's k-th distance)")
    ap.add_argument("--skew", type=int, default=1_000_000, help="sort leg: entries of the one long segment of the skewed result")
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
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    for p in range(0, N, CHUNK):
        eng.mlp_topk_device(X[p: p + CHUNK], 1, labels[p: p + CHUNK])
    torch.cuda.synchronize()
    eng.buckets_begin(labels.cpu().numpy().astype(np.int64), d, L)
    for p in range(0, N, CHUNK):
        eng.add_rows(X[p: p + CHUNK], p)
        torch.cuda.synchronize()
    eng.buckets_end()
    del X

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

    sizes = eng.bucket_sizes()
    print(f"# {N} x {d}, {L} buckets (sizes min/median/max {sizes.min()}/{int(np.median(sizes))}/{sizes.max()}), {nq} queries, n_buckets {nb}; "
          f"device tensors; {a.steps} batches per row timed one by one after one warm-up; setup {time.time() - t0:.0f} s", flush=True)
    bo = torch.empty((nq, nb), dtype=torch.int32, device=dev)
    if a.sort:
        sort_leg(a, _capi, eng, Q, bo, dev)
        eng.set_stream(0)
        eng.close()
        return
    print("# call | k or radius | ms per batch min / mean / max | results per query mean / max | note", flush=True)
    for k in a.ks:
        d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        i_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
        c_t = torch.empty((nq,), dtype=torch.int32, device=dev)
        lo, mean, hi = timed_each(lambda: eng.search_union_device(Q, Q, nb, k, d_t, i_t, c_t, bo), a.steps)
        plan = _capi.union_last_plan()
        print(f"lmi_search_union | k {k} | {lo:.2f} / {mean:.2f} / {hi:.2f} | {float(c_t.float().mean().item()):.1f} / {int(c_t.max().item())} | "
              f"groups {plan['GROUPS']} waves {plan['WAVES']} slab {plan['SLAB_BYTES'] >> 20} MiB workspace {plan['WORKSPACE_BYTES'] >> 20} MiB",
              flush=True)
        du, iu = d_t.cpu().numpy(), i_t.cpu().numpy().view(np.uint32)
        per_query = np.ascontiguousarray(du[:, k - 1])
        for what, radius in ((f"radius[q] = the k = {k} distance", per_query),
                             (f"radius {float(np.median(per_query)):.6f}", np.full(nq, np.median(per_query), np.float32))):
            keep = []

            def call():
                for r in keep:
                    r.close()
                keep[:] = [eng.search_range_device(Q, Q, nb, radius, bo)]

            lo, mean, hi = timed_each(call, a.steps)
            res = keep[0]
            plan = _capi.range_last_plan()
            n = np.diff(res.lims)
            dd, ii = res.read()
            res.close()
            agree = 0   # queries whose run, stably sorted by distance, begins with the union's ids (as far as both go)
            for q in range(nq):
                lo_q, hi_q = int(res.lims[q]), int(res.lims[q + 1])
                o = np.argsort(dd[lo_q:hi_q], kind="stable")[:k]
                m = min(k, hi_q - lo_q)
                agree += bool(np.array_equal(ii[lo_q:hi_q][o][:m], iu[q, :m]))
            print(f"lmi_search_range | {what} | {lo:.2f} / {mean:.2f} / {hi:.2f} | {n.mean():.1f} / {n.max()} | groups {plan['GROUPS']} waves "
                  f"{plan['WAVES']} slab {plan['SLAB_BYTES'] >> 20} MiB workspace {plan['WORKSPACE_BYTES'] >> 20} MiB chunks "
                  f"{plan['CHUNK_BYTES'] >> 10} KiB; sorted runs begin with the union's ids for {agree} of {nq} queries", flush=True)
    # ---- the sharded leg (profiles/range_sharded.txt): a rank's part call beside lmi_scan_range, and the join alone, for emulated worlds ----
    # Rank r of an emulated world owns the buckets b with b % world == r: the others are struck out of its order, which is what an
    # `owned` mask does to them (no rows), and leaves every rank t where it is.  One card plays every rank: no multi-GPU claim is made.
    print("# sharded leg: call | radius | ms per batch min / mean / max | note", flush=True)
    steps = max(a.steps, 5)
    stalls = []   # (row, batch times) of the rows in which one batch took more than three times the fastest

    def timed_row(row, fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        if max(ms) > 3 * min(ms):
            stalls.append((row, ms))
        return min(ms), sum(ms) / len(ms), max(ms)

    for k in a.ks:
        d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        i_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
        eng.search_union_device(Q, Q, nb, k, d_t, i_t, None, bo)
        torch.cuda.synchronize()
        radius = np.ascontiguousarray(d_t[:, k - 1].cpu().numpy())
        what = f"radius[q] = the k = {k} distance"
        keep = []

        def call(order):
            for r in keep:
                r.close()
            keep[:] = [eng.scan_range_device(Q, order, nb, radius)]

        lo, mean, hi = timed_row(f"lmi_scan_range, k {k}", lambda: call(bo))
        whole = keep.pop()
        wd = torch.empty(whole.total, dtype=torch.float32, device=dev)
        wi = torch.empty(whole.total, dtype=torch.int32, device=dev)
        whole.read_into(wd, wi)
        print(f"lmi_scan_range | {what} | {lo:.2f} / {mean:.2f} / {hi:.2f} | {whole.total} results", flush=True)
        for world in (2, 8):
            counts, ds, is_, rows = [], [], [], []
            for r in range(world):
                order = torch.where(bo % world == r, bo, torch.full_like(bo, -1))
                rows.append(timed_row(f"rank {r} of {world}, k {k}", lambda: call(order)))
                part = keep.pop()
                counts.append(part.pair_counts())
                ds.append(torch.empty(part.total, dtype=torch.float32, device=dev))
                is_.append(torch.empty(part.total, dtype=torch.int32, device=dev))
                if part.total:
                    part.read_into(ds[-1], is_[-1])
                part.close()
            counts = np.stack(counts)
            totals = counts.reshape(world, -1).sum(axis=1)
            slow = max(rows, key=lambda t: t[1])
            print(f"lmi_scan_range on a rank's buckets, world {world} | {what} | {slow[0]:.2f} / {slow[1]:.2f} / {slow[2]:.2f} | the slowest of "
                  f"the {world} ranks (the fastest: mean {min(t[1] for t in rows):.2f}); part totals min / max {totals.min()} / {totals.max()}",
                  flush=True)

            def join():
                for r in keep:
                    r.close()
                keep[:] = [eng.join_range_parts(counts, ds, is_)]

            lo, mean, hi = timed_row(f"join, world {world}, k {k}", join)
            res = keep.pop()
            jd, ji = torch.empty_like(wd), torch.empty_like(wi)
            ok = res.total == whole.total and np.array_equal(res.lims, whole.lims)
            if ok and res.total:
                res.read_into(jd, ji)
                ok = torch.equal(jd.view(torch.int32), wd.view(torch.int32)) and torch.equal(ji, wi)
            res.close()
            plan = _capi.range_join_last_plan()
            print(f"lmi_join_range_parts, world {world} | {what} | {lo:.3f} / {mean:.3f} / {hi:.3f} | {plan['RUNS']} runs in {plan['PIECES']} "
                  f"pieces, {8 * plan['RESULTS'] >> 10} KiB of results; a padded all-gather would receive {8 * world * plan['LARGEST_PART'] >> 10} "
                  f"KiB; {'equal to' if ok else 'DIFFERS from'} lmi_scan_range", flush=True)
        whole.close()
    for row, ms in stalls:
        print(f"# a stalled batch in: {row}: " + " ".join(f"{t:.2f}" for t in ms), flush=True)
    eng.set_stream(0)
    eng.close()


def host_sort(lims, dd, ii):
    """The parent commit's route to the ordered result: one stable argsort per query (li.range_search(sort=True) before the device sort)."""
    for q in range(len(lims) - 1):
        lo, hi = int(lims[q]), int(lims[q + 1])
        if hi - lo > 1:
            o = np.argsort(dd[lo:hi], kind="stable")
            dd[lo:hi], ii[lo:hi] = dd[lo:hi][o], ii[lo:hi][o]
    return dd, ii


def sort_leg(a, _capi, eng, Q, bo, dev):
    import torch

    nq, nb, k, steps = a.nq, a.nb, a.sort_k, max(a.steps, 5)
    d_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    i_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
    eng.search_union_device(Q, Q, nb, k, d_t, i_t, None, bo)
    torch.cuda.synchronize()
    radius = np.ascontiguousarray(d_t[:, k - 1].cpu().numpy())

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), out

    def row(name, ms, note):
        print(f"{name} | {np.median(ms):.3f} | {min(ms):.3f} / {max(ms):.3f} | {note}", flush=True)

    print(f"# sort leg: radius[q] = the k = {k} distance; {steps} repeats after one warm-up, each call timed on its own", flush=True)
    print("# call | ms median | min / max | note", flush=True)
    scan_ms, sort_ms, read_ms, loop_ms, ok = [], [], [], [], True
    for step in range(steps + 1):
        t_scan, res = clock(lambda: eng.scan_range_device(Q, bo, nb, radius))
        t_read, (dd, ii) = clock(res.read)
        t0 = time.perf_counter()
        hd, hi_ = host_sort(res.lims, dd, ii)
        t_loop = 1e3 * (time.perf_counter() - t0)
        t_sort, _ = clock(lambda: res.sort(eng))
        plan = _capi.range_sort_last_plan()
        gd, gi = res.read()
        ok = ok and gd.view(np.uint32).tobytes() == hd.view(np.uint32).tobytes() and gi.tobytes() == hi_.tobytes()
        n = np.diff(res.lims)
        res.close()
        if step:   # the first is the warm-up
            scan_ms.append(t_scan), sort_ms.append(t_sort), read_ms.append(t_read), loop_ms.append(t_loop)
    what = (f"{int(n.sum())} results, per query mean {n.mean():.1f} max {n.max()}; groups {plan['groups']} wave {plan['wave_segments']} tile "
            f"{plan['tile_segments']} long {plan['long_segments']} skipped {plan['skipped_segments']} scratch {plan['scratch_bytes'] >> 10} KiB")
    row("(a) lmi_range_result_sort", sort_ms, what + f"; {'equal to' if ok else 'DIFFERS from'} the host order")
    row("(b) lmi_scan_range before it", scan_ms, "device pointers")
    row("(c) read() + one stable argsort per query", [x + y for x, y in zip(read_ms, loop_ms)],
        f"read() median {np.median(read_ms):.3f}, the loop median {np.median(loop_ms):.3f}")
    # the skewed result: no index needed, lmi_join_range_parts makes a result of any host arrays
    rs = np.random.RandomState(a.seed)
    lens = np.full(nq, k, np.int32)
    lens[nq // 2] = a.skew
    total = int(lens.sum())
    sd = rs.rand(total).astype(np.float32)
    si = np.arange(total, dtype=np.uint32)
    lims = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    skew_ms, ok = [], True
    for step in range(steps + 1):
        res = eng.join_range_parts(lens.reshape(1, nq, 1), [sd], [si])
        t_sort, _ = clock(lambda: res.sort(eng))
        plan = _capi.range_sort_last_plan()
        if step == 0:
            gd, gi = res.read()
            hd, hi_ = host_sort(lims, sd.copy(), si.copy())
            ok = gd.view(np.uint32).tobytes() == hd.view(np.uint32).tobytes() and gi.tobytes() == hi_.tobytes()
        else:
            skew_ms.append(t_sort)
        res.close()
    row(f"(d) lmi_range_result_sort, one segment of {a.skew}", skew_ms,
        f"{total} results; wave {plan['wave_segments']} long {plan['long_segments']} passes {plan['max_passes']} scratch "
        f"{plan['scratch_bytes'] >> 20} MiB; {'equal to' if ok else 'DIFFERS from'} the host order")


if __name__ == "__main__":
    main()
