#!/usr/bin/env python3
"""Cost of fetching stored objects by id (lmi_rows_fetch) against the only route an index without it offers, taken in the same run.

The index is synthetic and needs no model: --n rows x --d (default 1M x 768; standard normal values times 0.015, rounded to binary16
so that every stored form holds the same data), --leaves buckets by uniform random labels, ids = a random permutation of 1..N;
generated on the device piece by piece.  For each stored form (f32: row-major with the prefilter; exact: f32 fragments,
lmi_set_prefilter(0); f16: LMI_STORAGE_F16) and each request size (--requests, default 10, 10 000 and 1 000 000 random present ids,
drawn with replacement):
  fetch host     Index.fetch(ids): ids and rows in host memory (pageable numpy), wall time;
  fetch device   Index.fetch_device: ids and rows in device memory, wall time up to the call's return (it synchronises);
  read + gather  what a caller did before: a host dictionary id -> (bucket, row) (built once from read_bucket's ids, NOT timed), then
                 per call read_bucket of every bucket that holds a requested id and a numpy gather of the rows on the host.
One warm-up, then --reps alternating repeats (fetch host, fetch device, read + gather, and again); median / min / max in ms.
The three results are compared byte for byte before any time is reported.

  python tools/fetch_bench.py [--n 1000000] [--d 768] [--leaves 120] [--out profiles/fetch.txt]

Prints a table and one JSON line; --out also writes both to a file.  Not a yardstick: bench.py is.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from learnedmetricindex_amd import _capi  # noqa: E402

MODES = {"f32": dict(), "exact": dict(prefilter=False), "f16": dict(storage="f16")}


def build_on_device(mode, N, d, L, labels, ids, seed, piece):
    import torch

    eng = _capi.Index(0, **MODES[mode])
    eng.buckets_begin(labels, d, L, ids=ids)
    g = torch.Generator(device="cuda")
    for r0 in range(0, N, piece):
        n = min(piece, N - r0)
        g.manual_seed(seed + r0)
        x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).mul_(0.015).to(torch.float16)
        eng.add_rows(x if mode == "f16" else x.to(torch.float32), r0)
    eng.buckets_end()
    return eng


def wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def stats(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--leaves", type=int, default=120)
    ap.add_argument("--requests", type=int, nargs="+", default=[10, 10_000, 1_000_000])
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    N, d, L = args.n, args.d, args.leaves
    rs = np.random.RandomState(args.seed)
    labels = rs.randint(0, L, N).astype(np.int64)
    ids = (rs.permutation(N) + 1).astype(np.uint32)
    piece = min(1 << 18, max(1, N // 4))
    lines = [f"# lmi_rows_fetch on {N} x {d}, {L} buckets; lib {_capi.lib().lmi_build_info().decode()}",
             "# ms: median (min .. max) of %d alternating repeats after one warm-up" % args.reps,
             "# form | requests | unique | fetch host ms | fetch device ms | read_bucket + host gather ms | buckets read | old / fetch host"]
    records = []
    for mode in args.modes:
        eng = build_on_device(mode, N, d, L, labels, ids, args.seed, piece)
        sizes = eng.bucket_sizes()
        # the caller's own dictionary (not timed): id -> (bucket, row), from the ids read_bucket returns
        where_b, where_r = np.empty(N + 1, np.int32), np.empty(N + 1, np.int32)
        for b in range(L):
            _, bid = eng.read_bucket(b, rows_out=np.empty((int(sizes[b]), d), np.float32))
            where_b[bid], where_r[bid] = b, np.arange(bid.size, dtype=np.int32)
        for n in args.requests:
            req = ids[rs.randint(0, N, n)]
            req_t = torch.from_numpy(req.view(np.int32)).cuda()
            rows_t = torch.empty((n, d), dtype=torch.float32, device="cuda")
            out = np.empty((n, d), np.float32)

            def old():
                res = np.empty((n, d), np.float32)
                rb, rr = where_b[req], where_r[req]
                for b in np.unique(rb):
                    rows, _ = eng.read_bucket(int(b))
                    sel = rb == b
                    res[sel] = rows[rr[sel]]
                return res

            runs = {"host": lambda: eng.fetch(req, rows_out=out), "device": lambda: eng.fetch_device(req_t, rows_t), "old": old}
            got = {k: wall(f)[0] for k, f in runs.items()}   # the warm-up, and the comparison
            plan = _capi.fetch_last_plan()
            assert np.array_equal(got["host"].view(np.uint8), got["old"].view(np.uint8))
            assert np.array_equal(rows_t.cpu().numpy().view(np.uint8), got["old"].view(np.uint8))
            ms = {k: [] for k in runs}
            for _ in range(args.reps):
                for k, f in runs.items():
                    ms[k].append(wall(f)[1])
            st = {k: stats(v) for k, v in ms.items()}
            rec = dict(form=mode, requests=n, unique=int(np.unique(req).size), fetch_host_ms=st["host"], fetch_device_ms=st["device"],
                       read_gather_ms=st["old"], buckets_read=int(np.unique(where_b[req]).size), pieces=plan["PIECES"],
                       workspace_bytes=plan["WORKSPACE_BYTES"])
            records.append(rec)

            def cell(s):
                return f"{s['median']:.2f} ({s['min']:.2f} .. {s['max']:.2f})"

            lines.append(f"{mode} | {n} | {rec['unique']} | {cell(st['host'])} | {cell(st['device'])} | {cell(st['old'])} | {rec['buckets_read']} | "
                         f"{st['old']['median'] / st['host']['median']:.1f}")
            print(lines[-1], flush=True)
            del rows_t, out
        eng.close()
        torch.cuda.empty_cache()
    line = json.dumps({"n": N, "d": d, "leaves": L, "points": records, "lib": _capi.lib().lmi_build_info().decode()})
    text = "\n".join(lines) + "\n" + line + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
