#!/usr/bin/env python3
"""What LMI_STORAGE_F16 saves and what it costs: the same synthetic fp16-exact vectors in both storages (developer aid).

The vectors are generated on the GPU piece by piece -- unit-length rows around --buckets random centres, rounded to binary16 and
widened again, the way 16-bit datasets reach the library -- and handed to lmi_buckets_add_rows as device tensors, so neither
storage ever needs N x d floats of host memory.  Every object's bucket is the centre it was drawn around; a query visits the
--nb centres nearest to it (lmi_scan_topk on device tensors: no MLP, so that the timing slots are the scan's).  Per storage:
  - lmi_index_bytes (between the last add_rows and lmi_buckets_end, and of the built index) and the build's wall time;
  - the timing slots of a search, averaged over --steps calls (lmi_timings_mean): LMI_T_PF_SAMPLE / LMI_T_PF_EMIT (pass 1 / pass 2:
    they read the same fragments in both storages), LMI_T_RESCORE (the exact re-rank: contiguous f32 rows against rows gathered
    from 16-byte fragment pieces) and LMI_T_TOTAL.
The results of the two storages are compared bit for bit.

  python tools/f16_storage_ab.py [--n 10000000] [--d 768] [--buckets 120] [--nb 4] [--nq 10000] [--steps 20] [--warmup 3]

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


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def piece_rows(cent, lab_t, seed, r0, n):
    """Rows r0 .. r0+n of the dataset: fp16-exact unit vectors around their bucket's centre (deterministic per piece)."""
    import torch

    g = torch.Generator(device=cent.device)
    g.manual_seed(seed * 1_000_003 + r0)
    x = cent[lab_t[r0:r0 + n]] + 0.7 * torch.randn((n, cent.shape[1]), generator=g, device=cent.device, dtype=torch.float32)
    x = x / x.norm(dim=1, keepdim=True)
    return x.half().float().contiguous()


def run(storage, args, cent, lab, lab_t, q_t, order_t):
    import torch

    from learnedmetricindex_amd import _capi

    dev = cent.device
    eng = _capi.Index(dev.index or 0, storage=storage)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.buckets_begin(lab, args.d, args.buckets)
    for r0 in range(0, args.n, args.piece):
        n = min(args.piece, args.n - r0)
        eng.add_rows(piece_rows(cent, lab_t, args.seed, r0, n), r0)
    torch.cuda.synchronize()
    mid = eng.index_bytes()
    eng.buckets_end()
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    built = eng.index_bytes()
    nq, kout = q_t.shape[0], eng.kout(args.nb, args.k)
    d_t = torch.empty((nq, kout), dtype=torch.float32, device=dev)
    i_t = torch.empty((nq, kout), dtype=torch.int32, device=dev)
    for _ in range(max(1, args.warmup)):
        eng.scan_topk_device(q_t, order_t, args.nb, args.k, d_t, i_t)
    torch.cuda.synchronize()
    eng.timings_reset()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.scan_topk_device(q_t, order_t, args.nb, args.k, d_t, i_t)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) / args.steps * 1e3
    ms, calls = eng.timings_mean()
    _, survivors, fallbacks = eng.prefilter_stats()
    out = dict(storage=storage, index_bytes_mid_build=mid, index_bytes=built, build_s=round(build_s, 3), wall_ms_per_batch=round(wall_ms, 4),
               t_pf_sample_ms=round(float(ms[_capi.T_PF_SAMPLE]), 4), t_pf_emit_ms=round(float(ms[_capi.T_PF_EMIT]), 4),
               t_rescore_ms=round(float(ms[_capi.T_RESCORE]), 4), t_fallback_ms=round(float(ms[_capi.T_FALLBACK]), 4),
               t_total_ms=round(float(ms[_capi.T_TOTAL]), 4), calls=calls, survivors=survivors, fallbacks=fallbacks)
    res = (d_t.cpu().numpy().view(np.uint32), i_t.cpu().numpy())
    eng.close()
    del d_t, i_t
    torch.cuda.empty_cache()
    return out, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--buckets", type=int, default=120)
    ap.add_argument("--nb", type=int, default=4)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--piece", type=int, default=250_000, help="rows generated and handed over per lmi_buckets_add_rows call")
    ap.add_argument("--storages", default="f32,f16")
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    cent = torch.randn((args.buckets, args.d), generator=g, device=dev, dtype=torch.float32)
    lab = np.random.RandomState(args.seed).randint(0, args.buckets, args.n).astype(np.int64)
    lab_t = torch.from_numpy(lab).to(dev)
    q = cent[torch.randint(0, args.buckets, (args.nq,), generator=g, device=dev)] + 0.7 * torch.randn((args.nq, args.d), generator=g, device=dev)
    q_t = (q / q.norm(dim=1, keepdim=True)).half().float().contiguous()
    order_t = torch.topk(q_t @ cent.T, args.nb, dim=1).indices.to(torch.int32).contiguous()
    rows, results = [], []
    for storage in args.storages.split(","):
        out, res = run(storage, args, cent, lab, lab_t, q_t, order_t)
        rows.append(out)
        results.append(res)
        log(f"[f16_ab] {storage}: index_bytes {out['index_bytes'] / 1e9:.3f} GB (mid-build {out['index_bytes_mid_build'] / 1e9:.3f} GB), build {out['build_s']:.2f} s; "
            f"pass 1 {out['t_pf_sample_ms']:.4f} ms, pass 2 {out['t_pf_emit_ms']:.4f} ms, re-rank {out['t_rescore_ms']:.4f} ms, "
            f"total {out['t_total_ms']:.4f} ms ({out['wall_ms_per_batch']:.4f} ms wall), survivors {out['survivors']}, fallbacks {out['fallbacks']}")
    same = None
    if len(results) == 2:
        same = bool(np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1]))
        log(f"[f16_ab] results identical bit for bit: {same}; index_bytes ratio {rows[1]['index_bytes'] / rows[0]['index_bytes']:.3f}, "
            f"re-rank x{rows[1]['t_rescore_ms'] / max(rows[0]['t_rescore_ms'], 1e-9):.2f}, total x{rows[1]['t_total_ms'] / max(rows[0]['t_total_ms'], 1e-9):.3f}")
    from learnedmetricindex_amd import _capi

    print(json.dumps({"n": args.n, "d": args.d, "buckets": args.buckets, "nb": args.nb, "nq": args.nq, "k": args.k, "steps": args.steps,
                      "identical": same, "runs": rows, "lib": _capi.lib().lmi_build_info().decode()}), flush=True)
    if same is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
