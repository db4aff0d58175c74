#!/usr/bin/env python3
"""Cost of re-bucketing a resident index on the device (lmi_regroup) against the only route without it: a fresh build of the same
object list, under the new labels, from host arrays.

The index is synthetic and needs no model: --n rows x --d (default 1M x 768; standard normal values times 0.05, rounded to binary16 so
that both storages hold the same data), --leaves buckets, ids 1..N.  The rows are generated on the device piece by piece and kept in
ONE host array, which both builds read.  The old labels are random and SORTED, so that the order in which the host array holds the
objects is the order the parent index holds them: the fresh build of (host rows, new labels, ids) is then exactly what the regroup has
to equal, and it is checked to (bucket sizes, layout, index bytes, rows and ids of sampled buckets) before a time is reported.
The new labels are random over the same number of buckets and EVERY object is named: a complete re-placement, the most the call can be
asked to do (the whole list is sorted on the host, every row is looked up, every word is sorted).  For each mode (F32 with the
prefilter, LMI_STORAGE_F16), in the same run:
  regroup   wall time of Index.regroup with the ids in sorted order (best of --reps calls; all of them are in the JSON line); with
            --unsorted also the same list shuffled, once; the call returns when the new index is complete (maps, gathers and what a
            build derives from the rows included)
  build     wall time of Index.set_buckets of the host rows under the new labels (best of --reps): the existing path, pageable host
            memory
  copy      a device-to-device copy (torch) of as many bytes as the new index's images hold: what moving that much memory costs
  peak      device bytes at the call's high-water mark as the library accounts for them: the parent's images + the new index's + the
            call's maps (lmi_debug_regroup_plan's MAP_BYTES), and the drop of free device memory the call left behind
When an allocation fails (device or host) the run starts over with half the rows: "the largest that fits".  Nothing is promised about
speed: there is no exit status for it.

  python tools/regroup_bench.py [--n 1000000] [--d 768] [--leaves 120] [--out profiles/regroup.txt]

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


def host_rows(N, d, seed, piece=1 << 18):
    import torch

    out = np.empty((N, d), dtype=np.float32)
    g = torch.Generator(device="cuda")
    for r0 in range(0, N, piece):
        n = min(piece, N - r0)
        g.manual_seed(seed + r0)
        x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).mul_(0.05)
        out[r0: r0 + n] = x.to(torch.float16).to(torch.float32).cpu().numpy()
    return out


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


def free_bytes():
    import torch

    return int(torch.cuda.mem_get_info()[0])


def run(N, args):
    """(report lines, records) of one whole measurement at N rows."""
    import torch

    d, L = args.d, args.leaves
    rs = np.random.RandomState(args.seed)
    old = np.sort(rs.randint(0, L, N)).astype(np.int64)   # sorted: the host order IS the parent's order
    new = rs.randint(0, L, N).astype(np.int64)
    ids = np.arange(1, N + 1, dtype=np.uint32)
    X = host_rows(N, d, args.seed)
    lines = [f"# lmi_regroup (complete re-placement) against a fresh build from host arrays: {N} x {d}, {L} buckets; "
             f"lib {_capi.lib().lmi_build_info().decode()}",
             "# mode | image MB | regroup ms | build ms | copy ms | build / regroup | regroup / copy | peak MB = parent + new + maps | "
             "free-memory drop MB"]
    records = []
    for mode in args.modes:
        rows = X.astype(np.float16) if mode == "f16" else X

        def build(labels):
            eng = _capi.Index(0, storage=mode)
            eng.set_buckets(rows, labels, L, ids=ids)
            return eng

        parent = build(old)
        torch.cuda.empty_cache()
        warm = parent.regroup(ids[:1], new[:1], L)   # (the first call of a process loads the kernels)
        warm.close()
        before = free_bytes()
        out, regroup_ms = wall(lambda: parent.regroup(ids, new, L))
        drop = before - free_bytes()
        plan = _capi.regroup_last_plan()
        assert out.n_named == N
        regroup_all = [regroup_ms]
        for _ in range(args.reps - 1):   # the same call again: the spread, and the best of them is what is reported
            tmp, ms = wall(lambda: parent.regroup(ids, new, L))
            tmp.close()
            regroup_all.append(ms)
        regroup_ms = min(regroup_all)
        unsorted_ms = None
        if args.unsorted:
            order = rs.permutation(N)
            tmp, unsorted_ms = wall(lambda: parent.regroup(ids[order], new[order], L))
            tmp.close()
        ref, build_ms = wall(lambda: build(new))
        build_all = [build_ms]
        for _ in range(args.reps - 1):
            tmp, ms = wall(lambda: build(new))
            tmp.close()
            build_all.append(ms)
        build_ms = min(build_all)
        np.testing.assert_array_equal(out.bucket_sizes(), ref.bucket_sizes())
        np.testing.assert_array_equal(out.debug_layout()["rb_start"], ref.debug_layout()["rb_start"])
        assert out.index_bytes() == ref.index_bytes()
        dtype = np.float16 if mode == "f16" else np.float32
        for b in range(0, L, max(1, L // 8)):
            r1, i1 = out.read_bucket(b, dtype=dtype)
            r2, i2 = ref.read_bucket(b, dtype=dtype)
            assert np.array_equal(i1, i2) and np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), b
        nbytes, parent_bytes = out.index_bytes(), parent.index_bytes()
        ref.close()
        out.close()
        parent.close()
        torch.cuda.empty_cache()
        cp_ms = copy_ms(nbytes)
        peak = parent_bytes + nbytes + plan["map_bytes"]
        rec = dict(mode=mode, image_bytes=int(nbytes), parent_bytes=int(parent_bytes), map_bytes=int(plan["map_bytes"]), peak_bytes=int(peak),
                   free_drop_bytes=int(drop), regroup_ms=round(regroup_ms, 3), build_ms=round(build_ms, 3), copy_ms=round(cp_ms, 3),
                   build_over_regroup=round(build_ms / regroup_ms, 2), regroup_over_copy=round(regroup_ms / cp_ms, 2),
                   tiles=plan["tiles"], passes=plan["passes"], regroup_all_ms=[round(v, 3) for v in regroup_all],
                   build_all_ms=[round(v, 3) for v in build_all])
        if unsorted_ms is not None:
            rec["regroup_unsorted_ms"] = round(unsorted_ms, 3)
        records.append(rec)
        lines.append(f"{mode} | {nbytes / 1e6:.0f} | {regroup_ms:.1f}" + (f" (unsorted list: {unsorted_ms:.1f})" if unsorted_ms is not None else "")
                     + f" | {build_ms:.1f} | {cp_ms:.2f} | {build_ms / regroup_ms:.1f} | {regroup_ms / cp_ms:.1f} | "
                     f"{peak / 1e6:.0f} = {parent_bytes / 1e6:.0f} + {nbytes / 1e6:.0f} + {plan['map_bytes'] / 1e6:.0f} | {drop / 1e6:.0f}")
        print(lines[-1], flush=True)
        del rows
    return lines, records


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--leaves", type=int, default=120)
    ap.add_argument("--modes", nargs="+", default=["f32", "f16"], choices=["f32", "f16"])
    ap.add_argument("--unsorted", action="store_true", help="also time the regroup with the list shuffled")
    ap.add_argument("--reps", type=int, default=3, help="times each timed call is made; the best is reported, all are in the JSON line")
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


if __name__ == "__main__":
    main()
