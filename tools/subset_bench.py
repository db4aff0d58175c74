#!/usr/bin/env python3
"""Cost of deriving a filtered copy of a resident index on the device (lmi_subset) against the only route without it: read every
bucket back to the host (read_bucket), filter there, and build a fresh index from the host.

The index is synthetic and needs no model: --n rows x --d (default 10M x 768; standard normal values, rounded to binary16 so that
both storages hold the same data), --leaves buckets by uniform random labels, ids 1..N; it is generated on the device piece by
piece.  For each mode (F32 with the prefilter, LMI_STORAGE_F16) and each kept fraction (--fractions, default 0.1 0.5 1.0), all in
the same run:
  subset    wall time of Index.subset with a SORTED id list of the kept objects (fraction 1.0: drop=True with no ids); the call
            returns when the new index is complete.  With --unsorted also the same list shuffled (the library sorts it on the host);
  rebuild   read_bucket of every bucket into one host slab (once per mode: it does not depend on the fraction; float16 rows for the
            F16 index, half the bytes), the host filter, and set_buckets of the kept rows from the host -- the times are summed;
  copy      a device-to-device copy (torch) of as many bytes as the subset's images hold (index_bytes), the yardstick of what
            moving that much memory costs at all.
The derived index is checked against the rebuilt one (bucket sizes, layout, the ids of every bucket) before its time is reported.
The rebuild route is charged what it really costs a caller: the host slab the buckets are read into (N x d values of pageable
memory), numpy's `isin` over the ids, and the upload of the kept rows from pageable host memory.  The subset's time is the whole
call -- the new handle, the copies of the models, the maps, the zero-filled images, the gather AND what a build derives from the
rows (an F32 index: absmax, the fp16 fragments, the norms: three more passes over the new rows) -- so "subset / copy" compares a
whole derivation with ONE plain copy of the images' bytes, not the gather kernel with a copy.
When an allocation fails (device or host) the run starts over with half the rows: "the largest that fits".
Exit status 1 if the derived copy is not faster than the rebuild route at some measured point.

  python tools/subset_bench.py [--n 10000000] [--d 768] [--leaves 120] [--out profiles/subset.txt]

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


def build_on_device(storage, N, d, L, labels, seed, piece=1 << 18):
    import torch

    eng = _capi.Index(0, storage=storage)
    eng.buckets_begin(labels, d, L)
    g = torch.Generator(device="cuda")
    for r0 in range(0, N, piece):
        n = min(piece, N - r0)
        g.manual_seed(seed + r0)
        x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).mul_(0.05)
        eng.add_rows(x.to(torch.float16) if storage == "f16" else x.to(torch.float16).to(torch.float32), r0)
    eng.buckets_end()
    return eng


def wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def copy_ms(nbytes, reps=3):
    import torch

    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    best = float("inf")
    for _ in range(reps):
        _, ms = wall(lambda: dst.copy_(src))
        best = min(best, ms)
    del src, dst
    torch.cuda.empty_cache()
    return best


def run(N, args):
    """(report lines, records) of one whole measurement at N rows."""
    import torch

    d, L = args.d, args.leaves
    rs = np.random.RandomState(args.seed)
    labels = rs.randint(0, L, N).astype(np.int64)
    lines = [f"# lmi_subset against read-back + rebuild: {N} x {d}, {L} buckets; lib {_capi.lib().lmi_build_info().decode()}",
             "# mode | kept fraction | kept objects | image MB | subset ms | rebuild ms = read-back + filter + build | copy ms | "
             "rebuild / subset | subset / copy"]
    records = []
    for mode in args.modes:
        eng, build_ms = wall(lambda: build_on_device(mode, N, d, L, labels, args.seed))
        dtype = np.float16 if mode == "f16" else np.float32
        sizes = eng.bucket_sizes()
        start = np.concatenate([[0], np.cumsum(sizes)])
        host_rows = np.empty((N, d), dtype=dtype)
        host_ids = np.empty(N, dtype=np.uint32)

        def read_back():
            for b in range(L):
                eng.read_bucket(b, host_rows[start[b]: start[b + 1]], host_ids[start[b]: start[b + 1]], dtype=dtype)

        _, read_ms = wall(read_back)
        host_lab = np.repeat(np.arange(L, dtype=np.int64), sizes)
        for frac in args.fractions:
            full = frac >= 1.0
            keep = np.ones(N, dtype=bool) if full else rs.rand(N) < frac
            ids = np.flatnonzero(keep).astype(np.uint32) + 1   # ids are 1..N in original order: sorted
            sub, sub_ms = wall(lambda: eng.subset([], drop=True) if full else eng.subset(ids))
            unsorted_ms = None
            if args.unsorted and not full:
                shuffled = ids[rs.permutation(ids.size)]
                tmp, unsorted_ms = wall(lambda: eng.subset(shuffled))
                tmp.close()

            def rebuild():
                sel = np.isin(host_ids, ids) if not full else slice(None)
                ref = _capi.Index(0, storage=mode)
                ref.set_buckets(host_rows[sel], host_lab[sel], L, ids=host_ids[sel])
                return ref

            ref, rebuild_ms = wall(rebuild)
            np.testing.assert_array_equal(sub.bucket_sizes(), ref.bucket_sizes())
            np.testing.assert_array_equal(sub.debug_layout()["rb_start"], ref.debug_layout()["rb_start"])
            assert sub.index_bytes() == ref.index_bytes()
            for b in range(0, L, max(1, L // 8)):
                r1, i1 = sub.read_bucket(b, dtype=dtype)
                r2, i2 = ref.read_bucket(b, dtype=dtype)
                assert np.array_equal(i1, i2) and np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), b
            nbytes = sub.index_bytes()
            kept = sub.N
            ref.close()
            sub.close()
            cp_ms = copy_ms(nbytes)
            total = read_ms + rebuild_ms
            rec = dict(mode=mode, fraction=frac, kept=int(kept), image_bytes=int(nbytes), subset_ms=round(sub_ms, 3),
                       readback_ms=round(read_ms, 3), filter_build_ms=round(rebuild_ms, 3), rebuild_ms=round(total, 3),
                       copy_ms=round(cp_ms, 3), rebuild_over_subset=round(total / sub_ms, 2), subset_over_copy=round(sub_ms / cp_ms, 2))
            if unsorted_ms is not None:
                rec["subset_unsorted_ms"] = round(unsorted_ms, 3)
            records.append(rec)
            lines.append(f"{mode} | {frac:g} | {kept} | {nbytes / 1e6:.0f} | {sub_ms:.1f}" + (f" (unsorted list: {unsorted_ms:.1f})" if unsorted_ms is not None else "")
                         + f" | {total:.1f} = {read_ms:.1f} + {rebuild_ms:.1f} | {cp_ms:.2f} | {total / sub_ms:.1f} | {sub_ms / cp_ms:.1f}")
            print(lines[-1], flush=True)
        del host_rows, host_ids
        eng.close()
        torch.cuda.empty_cache()
    return lines, records


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--leaves", type=int, default=120)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.1, 0.5, 1.0])
    ap.add_argument("--modes", nargs="+", default=["f32", "f16"], choices=["f32", "f16"])
    ap.add_argument("--unsorted", action="store_true", help="also time the subset with the id list shuffled")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    N, d, L = args.n, args.d, args.leaves
    while True:
        try:
            lines, records = run(N, args)
            break
        except (_capi.LmiError, MemoryError, torch.cuda.OutOfMemoryError) as e:
            if N <= 1000 or not any(w in str(e).lower() for w in ("alloc", "memory")):
                raise
            print(f"# {N} rows do not fit ({str(e)[:120]}): starting over with {N // 2}", flush=True)
            torch.cuda.empty_cache()
            N //= 2
    line = json.dumps({"n": N, "d": d, "leaves": L, "points": records, "lib": _capi.lib().lmi_build_info().decode()})
    text = "\n".join(lines) + "\n" + line + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    slow = [(r["mode"], r["fraction"]) for r in records if not r["subset_ms"] < r["rebuild_ms"]]
    if slow:
        print(f"FAILED: the derived copy is not faster than read-back + rebuild at {slow}", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
