#!/usr/bin/env python3
"""Cost of concatenating two resident indexes on the device (lmi_concat) against two yardsticks taken in the same run.

The indexes are synthetic and need no model: --n rows x --d (default 2M x 768; standard normal values times 0.015, rounded to binary16
so that every stored form holds the same data; the first value of every generated piece is 0.125, above all others, so that the parts
and `whole` have the same maximum and an f16 part is multiplied on the way only where --rescale asks for it), --leaves buckets by
uniform random labels, ids 1..N; generated on the device piece by
piece.  Part A holds the first --split of the rows, part B the rest, `whole` all of them -- so A.concat(B) must equal `whole`.  For
each stored form (f32: row-major with the prefilter; exact: f32 fragments, lmi_set_prefilter(0); f16: LMI_STORAGE_F16):
  concat    wall time of A.concat(B), best of --reps; the call returns when the new index is complete: the new handle, the copies of
            the models, the source map, the zero-filled images, the gather AND what a build derives from the rows (f32: absmax, the
            fp16 fragments, the norms: three more passes over the new rows);
  copy      wall time of whole.subset([], drop=True), best of --reps: lmi_subset's full copy of an index of the same total size --
            the same bytes moved by the kernels lmi_concat's are modelled on, the same derivation afterwards;
  build     wall time of a fresh build of the same rows from host memory (set_buckets from a pageable host slab, read back from
            `whole` beforehand and not timed): what a caller without lmi_concat does after concatenating on the host;
  GB/s      the result's image bytes (index_bytes) over the concat's time: bytes WRITTEN per second by the whole call.
With --rescale the f16 form is also timed with part B's values times 4 (maximum 0.5: the result's scale is 1, part A's is 4), so that
every half of part A is multiplied by 1/4 on the way.
The result is checked against `whole` (bucket sizes, layout, bytes, rows and ids of sampled buckets) before its time is reported.
When an allocation fails (device or host) the run starts over with half the rows: "the largest that fits".

  python tools/concat_bench.py [--n 2000000] [--d 768] [--leaves 120] [--out profiles/concat.txt]

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


def build_on_device(mode, rows, d, L, labels, seed, piece, factor=1.0):
    """An index of the objects `rows` (original row numbers, ascending) of the synthetic set; ids = row + 1."""
    import torch

    eng = _capi.Index(0, **MODES[mode])
    eng.buckets_begin(labels[rows], d, L, ids=(rows + 1).astype(np.uint32))
    g = torch.Generator(device="cuda")
    first = int(rows[0]) if rows.size else 0
    for r0 in range(0, rows.size, piece):
        n = min(piece, rows.size - r0)
        g.manual_seed(seed + first + r0)   # (a part is a range of the rows that starts on a piece boundary: the same pieces as in `whole`)
        x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).mul_(0.015)
        x[0, 0] = 0.125   # (the maximum of every piece, hence of every part: 8 sigma)
        x = x.mul_(factor).to(torch.float16)
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


def best_of(reps, fn):
    """(the last result, the best time); earlier results are closed."""
    best, out = float("inf"), None
    for _ in range(reps):
        if out is not None:
            out.close()
        out, ms = wall(fn)
        best = min(best, ms)
    return out, best


def same_index(a, b, L, dtype):
    np.testing.assert_array_equal(a.bucket_sizes(), b.bucket_sizes())
    np.testing.assert_array_equal(a.debug_layout()["rb_start"], b.debug_layout()["rb_start"])
    assert a.index_bytes() == b.index_bytes()
    for bkt in range(0, L, max(1, L // 8)):
        r1, i1 = a.read_bucket(bkt, dtype=dtype)
        r2, i2 = b.read_bucket(bkt, dtype=dtype)
        assert np.array_equal(i1, i2) and np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), bkt


def run(N, args):
    """(report lines, records) of one whole measurement at N rows."""
    import torch

    d, L = args.d, args.leaves
    piece = min(1 << 18, max(1, N // 8))
    cut = min(max(1, round(N * args.split / piece)), (N - 1) // piece) * piece   # on a piece boundary: A ++ B generates what `whole` does
    rs = np.random.RandomState(args.seed)
    labels = rs.randint(0, L, N).astype(np.int64)
    all_rows = np.arange(N, dtype=np.int64)
    lines = [f"# lmi_concat of two parts ({cut} + {N - cut} rows) x {d}, {L} buckets; lib {_capi.lib().lmi_build_info().decode()}",
             "# form | objects | image MB | concat ms | GB/s written | full copy (lmi_subset) ms | build from host ms | concat / copy | build / concat"]
    records = []
    cases = [(m, 1.0) for m in args.modes] + ([("f16", 4.0)] if args.rescale and "f16" in args.modes else [])
    for mode, factor in cases:
        dtype = np.float16 if mode == "f16" else np.float32
        a = build_on_device(mode, all_rows[:cut], d, L, labels, args.seed, piece)
        b = build_on_device(mode, all_rows[cut:], d, L, labels, args.seed, piece, factor)
        cat, cat_ms = best_of(args.reps, lambda: a.concat(b))
        plan = _capi.concat_last_plan()
        assert plan["rescaled_parts"] == (1 if factor != 1.0 else 0), plan
        nbytes = cat.index_bytes()
        rec = dict(form=mode, rescaled=factor != 1.0, objects=int(cat.N), image_bytes=int(nbytes), concat_ms=round(cat_ms, 3),
                   gb_per_s=round(nbytes / cat_ms / 1e6, 1), map_bytes=plan["map_bytes"])
        if factor == 1.0:
            whole = build_on_device(mode, all_rows, d, L, labels, args.seed, piece)
            same_index(cat, whole, L, dtype)
            cat.close()
            full, copy_ms = best_of(args.reps, lambda: whole.subset([], drop=True))
            full.close()
            sizes = whole.bucket_sizes()
            start = np.concatenate([[0], np.cumsum(sizes)])
            host_rows, host_ids = np.empty((N, d), dtype=dtype), np.empty(N, dtype=np.uint32)
            for bkt in range(L):
                whole.read_bucket(bkt, host_rows[start[bkt]: start[bkt + 1]], host_ids[start[bkt]: start[bkt + 1]], dtype=dtype)
            whole.close()
            host_lab = np.repeat(np.arange(L, dtype=np.int64), sizes)

            def rebuild():
                ref = _capi.Index(0, **MODES[mode])
                ref.set_buckets(host_rows, host_lab, L, ids=host_ids)
                return ref

            ref, build_ms = wall(rebuild)
            ref.close()
            del host_rows, host_ids
            rec.update(copy_ms=round(copy_ms, 3), build_ms=round(build_ms, 3), concat_over_copy=round(cat_ms / copy_ms, 2),
                       build_over_concat=round(build_ms / cat_ms, 1))
            lines.append(f"{mode} | {rec['objects']} | {nbytes / 1e6:.0f} | {cat_ms:.1f} | {rec['gb_per_s']:.0f} | {copy_ms:.1f} | {build_ms:.1f} | "
                         f"{cat_ms / copy_ms:.2f} | {build_ms / cat_ms:.1f}")
        else:
            cat.close()
            lines.append(f"{mode}, part A's halves rescaled on the way | {rec['objects']} | {nbytes / 1e6:.0f} | {cat_ms:.1f} | {rec['gb_per_s']:.0f} | - | - | - | -")
        records.append(rec)
        print(lines[-1], flush=True)
        a.close()
        b.close()
        torch.cuda.empty_cache()
    return lines, records


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--leaves", type=int, default=120)
    ap.add_argument("--split", type=float, default=0.5, help="fraction of the rows in part A")
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--rescale", action="store_true", help="also time the f16 form with part B's values times 4 (part A is rescaled)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    torch.cuda.set_device(0)
    N = args.n
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
    line = json.dumps({"n": N, "d": args.d, "leaves": args.leaves, "points": records, "lib": _capi.lib().lmi_build_info().decode()})
    text = "\n".join(lines) + "\n" + line + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
