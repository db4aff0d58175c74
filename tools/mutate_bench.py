#!/usr/bin/env python3
"""Cost of mutating a resident index (lmi_buckets_insert / lmi_buckets_delete) and the search rate after it.

The index is bench.py's synthetic one (default C2: 10M x 768, 120 leaves, the MLP trained as bench.py trains it), built once.
Measured, each with hipEvents on the handle's stream around the call and the host wall time of the call:
  - an insert of --insert rows (fresh draws of the same generator, placed by argmax MLP like the build) from HOST memory: every
    bucket of a fresh build is full to the row-block, so this one relocates them (a re-pack into new allocations);
  - a second insert of as many rows, which lands in the slack the first one left;
  - a delete of --delete ids drawn at random from the index;
  - the search rate with the query batch resident in HBM (one lmi_search per batch on one stream, as bench.py's `value` loop),
    on the fresh index and on the mutated one.

  python tools/mutate_bench.py [--config c2] [--insert 100000] [--delete 100000] [--steps 20] [--warmup 3]

Prints a human-readable report and one JSON line.  Not a yardstick: bench.py is.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def resident_rate(eng, q, nb, k, steps, warmup):
    import torch

    nq = q.shape[0]
    kout = eng.kout(nb, k)
    dev = q.device
    d_t = torch.empty((nq, kout), dtype=torch.float32, device=dev)
    i_t = torch.empty((nq, kout), dtype=torch.int32, device=dev)
    bo_t = torch.empty((nq, nb), dtype=torch.int32, device=dev)
    for _ in range(max(1, warmup)):
        eng.search_device(q, q, nb, k, d_t, i_t, None, bo_t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.search_device(q, q, nb, k, d_t, i_t, None, bo_t)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return nq * steps / dt, dt / steps * 1e3, i_t.cpu().numpy()


def timed(fn):
    import torch

    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    e1.record(s)
    e1.synchronize()
    return out, e0.elapsed_time(e1), wall


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--insert", type=int, default=100_000)
    ap.add_argument("--delete", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--train-rows", type=int, default=200_000)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--exact", action="store_true", help="the all-f32 scan (lmi_set_prefilter(0)) instead of the fp16 prefilter")
    args = ap.parse_args()
    bargs = argparse.Namespace(seed=args.seed, train_rows=args.train_rows, epochs=args.epochs, exact=args.exact, chunk_rows=None,
                               timing_level=2, shard_mode="bucket", emulate_shard=None)
    import torch

    cfg = dict(bench.CONFIGS[args.config])
    N, d, L, nb, nq, k = cfg["n"], cfg["d"], cfg["leaves"], cfg["nb"], cfg["nq"], args.k
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    wl = bench.Workload(bargs, cfg, dev, 0, 1, 0)
    eng, q = wl.eng, wl.queries
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    rate0, ms0, _ = resident_rate(eng, q, nb, k, args.steps, args.warmup)
    bench.log(f"[mutate] fresh index: {rate0 / 1e6:.3f} M q/s ({ms0:.3f} ms per {nq}-query batch)")

    # insert: fresh draws of the generator, placed by argmax MLP (as the build), handed over from host memory
    new_t = wl.gen_rows(11, 0, args.insert)
    lab_t = torch.empty(args.insert, dtype=torch.int32, device=dev)
    eng.mlp_topk_device(new_t, 1, lab_t)
    torch.cuda.synchronize()
    new_h = new_t.cpu().numpy()
    lab_h = lab_t.cpu().numpy().astype(np.int64)
    ids_h = (np.arange(args.insert) + N + 1).astype(np.uint32)
    del new_t, lab_t
    stored, ins_ev, ins_wall = timed(lambda: eng.insert(new_h, lab_h, ids_h))
    assert stored == args.insert
    bench.log(f"[mutate] insert of {args.insert} rows ({new_h.nbytes / 1e6:.0f} MB from host): {ins_ev:.2f} ms (events), {ins_wall:.2f} ms (wall)")

    # a second insert of the same size: the buckets relocated by the first one have slack, nothing moves
    new2_t = wl.gen_rows(12, 0, args.insert)
    lab2_t = torch.empty(args.insert, dtype=torch.int32, device=dev)
    eng.mlp_topk_device(new2_t, 1, lab2_t)
    torch.cuda.synchronize()
    new2_h, lab2_h = new2_t.cpu().numpy(), lab2_t.cpu().numpy().astype(np.int64)
    del new2_t, lab2_t
    stored2, ins2_ev, ins2_wall = timed(lambda: eng.insert(new2_h, lab2_h, ids_h + args.insert))
    assert stored2 == args.insert
    bench.log(f"[mutate] second insert of {args.insert} rows (into the slack): {ins2_ev:.2f} ms (events), {ins2_wall:.2f} ms (wall)")

    rs = np.random.RandomState(args.seed)
    gone = (rs.choice(N, args.delete, replace=False) + 1).astype(np.uint32)
    removed, del_ev, del_wall = timed(lambda: eng.delete(gone))
    assert removed == args.delete
    bench.log(f"[mutate] delete of {args.delete} ids: {del_ev:.2f} ms (events), {del_wall:.2f} ms (wall)")

    rate1, ms1, _ = resident_rate(eng, q, nb, k, args.steps, args.warmup)
    bench.log(f"[mutate] mutated index: {rate1 / 1e6:.3f} M q/s ({ms1:.3f} ms per batch), {100 * (rate1 / rate0 - 1):+.2f} % vs fresh")
    sizes = eng.bucket_sizes()
    line = {"config": args.config, "N": N, "d": d, "leaves": L, "nb": nb, "nq": nq, "k": k, "exact": bool(args.exact),
            "insert_rows": args.insert, "insert_ms_events": round(ins_ev, 3), "insert_ms_wall": round(ins_wall, 3),
            "insert2_ms_events": round(ins2_ev, 3), "insert2_ms_wall": round(ins2_wall, 3),
            "delete_ids": args.delete, "delete_ms_events": round(del_ev, 3), "delete_ms_wall": round(del_wall, 3),
            "rate_fresh_qps": round(rate0, 1), "rate_mutated_qps": round(rate1, 1), "ms_per_batch_fresh": round(ms0, 4),
            "ms_per_batch_mutated": round(ms1, 4), "rate_change_pct": round(100 * (rate1 / rate0 - 1), 3),
            "n_after": int(sizes.sum()), "steps": args.steps, "warmup": args.warmup,
            "lib": bench.lib_provenance()}
    print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
