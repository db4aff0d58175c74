#!/usr/bin/env python3
"""What taking binary16 data as it is distributed saves: the same values as float32 and as float16 host arrays, in one process
(developer aid).  The float32 paths are the code that was there before the *_f16 entry points, so they are the baseline of the run.

  build   an LMI_STORAGE_F16 index of --n x --d unit-length, binary16-exact rows (host memory -> lmi_buckets_add_rows /
          lmi_buckets_add_rows_f16 in pieces of --piece rows): bytes handed over (Index.bytes_in) and wall time per source type;
  load    index_io.load_index of that index from vectors.f32.npy and from vectors.f16.npy (the same directory otherwise; both files
          were just written, so they come from the page cache: the time is the library's side, not the disk's), into f16 storage;
  search  the search step of the notebook configuration's shape -- 100 000 x 768 scan vectors, 32-d navigation vectors, a [10, 10]
          index, 10 buckets, 10 000 queries, k = 10 -- through lmi_search_tree with float32 and with float16 host queries (pageable
          memory).  The models are random and the placement is their own argmax path: what is measured is the step's uploads and
          kernels, not recall.
Every measurement is repeated --repeats times; the report gives the median and the range.  The results of the two source types are
compared bit for bit.

  python tools/f16_ingest_ab.py [--n 2000000] [--d 768] [--buckets 120] [--repeats 3] [--dir DIR]

Prints a human-readable report and one JSON line.  Not a yardstick: bench.py is.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def fmt(s, unit):
    return f"{s['median']:.3f} {unit} ({s['min']:.3f} .. {s['max']:.3f})"


def host_rows(n, d, buckets, seed, dev):
    """(X16 [n, d] float16 in host memory, labels): unit-length rows around `buckets` centres, generated on the GPU piece by piece."""
    import torch

    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cent = torch.randn((buckets, d), generator=g, device=dev)
    lab = np.random.RandomState(seed).randint(0, buckets, n).astype(np.int64)
    lab_t = torch.from_numpy(lab).to(dev)
    out = np.empty((n, d), dtype=np.float16)
    for r0 in range(0, n, 250_000):
        m = min(250_000, n - r0)
        x = cent[lab_t[r0:r0 + m]] + 0.7 * torch.randn((m, d), generator=g, device=dev)
        out[r0:r0 + m] = torch.nn.functional.normalize(x, dim=1).half().cpu().numpy()
    return out, lab, cent


def timed_build(_capi, rows, lab, buckets, piece):
    import torch

    eng = _capi.Index(0, storage="f16")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.set_buckets(rows, lab, buckets, piece=piece)
    torch.cuda.synchronize()
    return eng, time.perf_counter() - t0


def leg_build(_capi, args, X16, X32, lab, cent):
    import torch

    q = torch.nn.functional.normalize(cent[:64] + 0.5, dim=1).half().float().cpu().numpy()[: min(64, args.buckets)]
    order = np.argsort(-(q @ cent.cpu().numpy().T), axis=1)[:, :4].astype(np.int32)
    out, results = {}, {}
    for name, rows in (("float32", X32), ("float16", X16)):
        secs = []
        for _ in range(args.repeats):
            eng, s = timed_build(_capi, rows, lab, args.buckets, args.piece)
            secs.append(s)
            moved, held = eng.bytes_in, eng.index_bytes()
            d, i = eng.scan_topk(q, order, 10)
            results[name] = (d.view(np.uint32), i)
            eng.close()
        out[name] = dict(bytes_in=moved, index_bytes=held, build_s=stats(secs))
        log(f"[f16_ingest] build from {name} rows: {moved / 1e9:.3f} GB handed over, {fmt(out[name]['build_s'], 's')}; index {held / 1e9:.3f} GB")
    same = all(np.array_equal(a, b) for a, b in zip(results["float32"], results["float16"]))
    return out, same


def leg_load(_capi, args, X16, lab, wd):
    """save_index of an f16-resident index (vectors.f16.npy), a copy of the directory with the vectors as float32, load_index of both."""
    from learnedmetricindex_amd import index_io
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from learnedmetricindex_amd.li.model import NeuralNetwork, linear_layers

    net = NeuralNetwork(input_dim=args.d, output_dim=args.buckets, model_type="MLP")
    li = LearnedIndex(net, {}, [(i,) for i in range(args.buckets)])
    eng = _capi.Index(0, storage="f16")
    eng.set_mlp(linear_layers(net.model))
    eng.set_buckets(X16, lab, args.buckets, piece=args.piece)
    li._engine = eng
    d16, d32 = os.path.join(wd, "idx16"), os.path.join(wd, "idx32")
    t0 = time.perf_counter()
    index_io.save_index(d16, li, [args.buckets])
    save_s = time.perf_counter() - t0
    li.close()
    os.makedirs(d32)
    for f in ("weights.npz", "sizes.npy", "ids.npy"):
        shutil.copy(os.path.join(d16, f), os.path.join(d32, f))
    meta = json.load(open(os.path.join(d16, "meta.json")))
    del meta["vectors"]                                   # the directory as it was written before the key existed
    json.dump(meta, open(os.path.join(d32, "meta.json"), "w"))
    v16 = np.load(os.path.join(d16, "vectors.f16.npy"), mmap_mode="r")
    v32 = np.lib.format.open_memmap(os.path.join(d32, "vectors.f32.npy"), mode="w+", dtype=np.float32, shape=v16.shape)
    for r0 in range(0, v16.shape[0], 250_000):
        v32[r0:r0 + 250_000] = v16[r0:r0 + 250_000]
    v32.flush()
    del v32, v16
    q = X16[:: max(1, X16.shape[0] // 256)][:256]
    out, results = {"save_f16_s": round(save_s, 3)}, {}
    for name, path in (("vectors.f32.npy", d32), ("vectors.f16.npy", d16)):
        secs = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            li2, ncat = index_io.load_index(path)
            secs.append(time.perf_counter() - t0)
            moved = li2._engine.bytes_in
            dd, nn, _ = li2.search_resident(q, q, ncat, n_buckets=3, k=10)
            results[name] = (dd, nn)
            li2.close()
        size = os.path.getsize(os.path.join(path, name))
        out[name] = dict(file_bytes=size, bytes_in=moved, load_s=stats(secs))
        log(f"[f16_ingest] load_index from {name}: {size / 1e9:.3f} GB on disk, {moved / 1e9:.3f} GB handed over, {fmt(out[name]['load_s'], 's')}")
    same = all(np.array_equal(a, b) for a, b in zip(*results.values()))
    return out, same


def leg_search(_capi, args, dev):
    import pandas as pd
    import torch

    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from learnedmetricindex_amd.li.model import NeuralNetwork
    from learnedmetricindex_amd.li.PriorityQueue import EMPTY_VALUE

    N, d, d_nav, nb, nq, k = 100_000, 768, 32, 10, 10_000, 10
    torch.manual_seed(args.seed)
    X16, _, _ = host_rows(N + nq, d, 100, args.seed + 1, dev)
    X, Q16 = X16[:N].astype(np.float32), X16[N:]
    proj = (np.random.RandomState(args.seed).randn(d, d_nav) / np.sqrt(d_nav)).astype(np.float32)
    Xn, Qn16 = (X @ proj).astype(np.float32), (Q16.astype(np.float32) @ proj).astype(np.float16)
    root = NeuralNetwork(input_dim=d_nav, output_dim=10, model_type="MLP")
    internal = {(i, EMPTY_VALUE): NeuralNetwork(input_dim=d_nav, output_dim=10, model_type="MLP") for i in range(10)}
    dp = np.empty((N, 2), dtype=np.int64)
    dp[:, 0] = root.predict(Xn)
    for i in range(10):
        sel = np.flatnonzero(dp[:, 0] == i)
        if sel.size:
            dp[sel, 1] = internal[(i, EMPTY_VALUE)].predict(Xn[sel])
    li = LearnedIndex(root, internal, [(i, j) for i in range(10) for j in range(10)])
    nav, srch = pd.DataFrame(Xn), pd.DataFrame(X)
    nav.index += 1
    srch.index += 1
    eng = li.prepare(nav, srch, dp, [10, 10])
    out, results = {}, {}
    for name, qn, qs in (("float32", Qn16.astype(np.float32), Q16.astype(np.float32)), ("float16", Qn16, Q16)):
        for _ in range(3):
            eng.search_tree(qn, qs, nb, k)
        ms = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                res = eng.search_tree(qn, qs, nb, k)
            ms.append((time.perf_counter() - t0) / args.steps * 1e3)
        results[name] = (res[0].view(np.uint32), res[1])
        out[name] = dict(query_bytes=int(qn.nbytes + qs.nbytes), step_ms=stats(ms))
        log(f"[f16_ingest] notebook-shape search_tree, {name} host queries: {(qn.nbytes + qs.nbytes) / 1e6:.1f} MB uploaded, {fmt(out[name]['step_ms'], 'ms')} per call")
    li.close()
    same = all(np.array_equal(a, b) for a, b in zip(results["float32"], results["float16"]))
    return out, same


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--buckets", type=int, default=120)
    ap.add_argument("--piece", type=int, default=1 << 18, help="rows per add_rows call of the build leg")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="search calls per repeat of the search leg")
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--dir", default=None, help="where the two index directories are written (default: a temporary directory)")
    ap.add_argument("--legs", default="build,load,search")
    args = ap.parse_args()
    import torch

    from learnedmetricindex_amd import _capi

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    legs = args.legs.split(",")
    report, identical = {}, {}
    if "build" in legs or "load" in legs:
        X16, lab, cent = host_rows(args.n, args.d, args.buckets, args.seed, dev)
    if "build" in legs:
        X32 = X16.astype(np.float32)
        report["build"], identical["build"] = leg_build(_capi, args, X16, X32, lab, cent)
        del X32
    if "load" in legs:
        wd = args.dir or tempfile.mkdtemp(prefix="f16_ingest_")
        try:
            report["load"], identical["load"] = leg_load(_capi, args, X16, lab, wd)
        finally:
            if args.dir is None:
                shutil.rmtree(wd, ignore_errors=True)
    if "search" in legs:
        report["search"], identical["search"] = leg_search(_capi, args, dev)
    log(f"[f16_ingest] results identical bit for bit: {identical}")
    print(json.dumps({"n": args.n, "d": args.d, "buckets": args.buckets, "piece": args.piece, "repeats": args.repeats, "identical": identical,
                      **report, "lib": _capi.lib().lmi_build_info().decode()}), flush=True)
    if not all(identical.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
