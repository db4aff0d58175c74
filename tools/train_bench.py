#!/usr/bin/env python3
"""Cost of one training round of the index build (`LearnedIndexBuilder._fit` without the clustering: --epochs epochs of training,
then the placement check `predict` over all rows) with the torch trainer (`NeuralNetwork.train_batch` over the builder's shuffling
DataLoader) against `trainer="hip"` (`NeuralNetwork.train_batch_hip`, lmi_train), on the same card and the same data.

Data: a unit-norm Gaussian mixture of --classes components, generated ON THE DEVICE in pieces (10M x 768 is 30.7 GB: it fits the
card, not a host array); the component of a row is its label (what k-means would hand over).  Model: --model (MLP-4), lr 0.01.
  torch  x and the labels on the host, as the builder has them; DataLoader(batch 256, shuffle) -> train_batch -> predict(host x).
         --torch-epochs E (default: --epochs) times fewer epochs and reports the per-epoch cost times --epochs beside it, for sizes
         where a whole round takes minutes; 0 skips the torch side (and the host copy of x).
  hip    x uploaded once as the builder does (the upload is in the window when the torch side ran, i.e. a host x exists; with
         --torch-epochs 0 x is already resident and there is no upload to time) -> train_batch_hip -> predict(device x).
Beside the rounds: lmi_train alone on the resident x at --epochs and 2 x --epochs steps; the difference over --epochs is the device
time of one step (the launches of a step run back to back on the NULL stream; the call's set-up cancels out).

  python tools/train_bench.py [--n 100000] [--d 768] [--classes 120] [--epochs 20] [--torch-epochs E] [--reps 3] [--out FILE]
  python tools/train_bench.py --quality [--seeds 3] [--epochs 20] [--out FILE]
  python tools/train_bench.py --f16 [--n ..] [--d ..] [--classes ..] [--epochs ..] [--out profiles/kmeans_f16.txt]

--quality: instead of the timings, what the two trainers' models are worth.  On the C1 mixture of bench.py (`synth.mixture`, 100 000 x
768, 120 leaves, 1 000 queries, top-4 buckets) the index is built (hip_kmeans labels, MLP-4, --epochs epochs per round, lr 0.01) with
--seeds torch seeds and as many hip seeds; per build: the training rounds the stopping rule needed, the build seconds and recall@10
against exact brute force.  The hip schedule draws other rows than torch's shuffle, so the models differ; accepted when every hip build
met the stopping rule and its recall lies within the torch builds' range widened by that range's own width on either side.

--f16: instead of the timings above, `lmi_train_f16` beside `lmi_train` on the same values in one process (the mixture narrowed to
float16 and widened again): --epochs steps from host arrays (the gather and the upload of the named rows are in the window) and from
device tensors, five repeats each with the forms alternating, the spread of the float form's five beside the medians, and the peak
device memory of the host-array call (polled from a second thread).  The results must be equal bit for bit, losses included.

Prints a table and one JSON line; --out appends both to a file.  Not a yardstick: bench.py is.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learnedmetricindex_amd import _capi  # noqa: E402
from learnedmetricindex_amd.li.LearnedIndexBuilder import MINI_BATCH, _PositionBatches  # noqa: E402
from learnedmetricindex_amd.li.model import NeuralNetwork, linear_layers  # noqa: E402


def wall(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def device_mixture(seed, n, d, classes, piece=1 << 18):
    """(x f32[n,d] unit-norm rows, labels int32[n]) on the device"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn(classes, d, device="cuda", generator=g)
    x = torch.empty((n, d), dtype=torch.float32, device="cuda")
    labels = torch.randint(0, classes, (n,), device="cuda", generator=g, dtype=torch.int32)
    for r0 in range(0, n, piece):
        part = centres[labels[r0: r0 + piece].long()] + torch.randn(min(piece, n - r0), d, device="cuda", generator=g)
        x[r0: r0 + piece] = part / part.norm(dim=1, keepdim=True)
    return x, labels


def quality(a):
    import pandas as pd
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import synth
    from learnedmetricindex_amd.li.BuildConfiguration import BuildConfiguration
    from learnedmetricindex_amd.li.clustering import algorithms
    from learnedmetricindex_amd.li.LearnedIndexBuilder import LearnedIndexBuilder

    n, d, leaves, nq, nb, k = 100_000, 768, 120, 1000, 4, 10
    X, Q = synth.mixture(2023, n, d, leaves, nq)
    df = pd.DataFrame(X)
    df.index += 1
    gt = (torch.from_numpy(Q).cuda().double() @ torch.from_numpy(X).cuda().double().T).topk(k, dim=1)[1].cpu().numpy() + 1
    cfg = BuildConfiguration([algorithms["hip_kmeans"]], [a.epochs], [a.model], [0.01], [leaves])
    lines = [f"train_bench --quality: {n} x {d}, {leaves} leaves, {a.model}, {a.epochs} epochs per round, top-{nb} of {nq} queries; "
             f"{_capi.lib().lmi_build_info().decode()}", "  trainer  seed  rounds  build s  recall@10"]
    rows = []
    print("\n".join(lines), flush=True)
    for trainer in ("hip", "torch"):
        for seed in range(2023, 2023 + a.seeds):
            torch.manual_seed(seed)
            li, dp, _, build_s, _ = LearnedIndexBuilder(df, cfg, trainer=trainer, trainer_seed=seed).build()
            net = li.root_model
            steps = net._hip_state[1] if trainer == "hip" else int(next(iter(net.optimizer.state.values()))["step"])
            classes = int(linear_layers(net.model)[-1][0].shape[0])   # the clusters that received rows
            _, nns, _ = li.search(df, Q, df, Q, dp, [classes], nb, k)
            rec = float(np.mean([len(set(g.tolist()) & set(r.tolist())) / k for g, r in zip(gt, np.asarray(nns, dtype=np.int64))]))
            rows.append(dict(trainer=trainer, seed=seed, rounds=steps // a.epochs, build_s=build_s, recall_at_10=rec,
                             classes=classes, categories=int(len(np.unique(dp[:, 0])))))
            lines.append(f"  {trainer:<7s}  {seed}  {steps // a.epochs:6d}  {build_s:7.1f}  {rec:.4f}")
            print(lines[-1], flush=True)
            li.close()
    tr = [r["recall_at_10"] for r in rows if r["trainer"] == "torch"]
    lo, hi = min(tr) - (max(tr) - min(tr)), max(tr) + (max(tr) - min(tr))
    ok = all(r["categories"] == r["classes"] and lo <= r["recall_at_10"] <= hi for r in rows if r["trainer"] == "hip")
    lines.append(f"  torch range {min(tr):.4f} .. {max(tr):.4f}, widened by its width: {lo:.4f} .. {hi:.4f}; every hip build inside and "
                 f"with all {rows[0]['classes']} categories predicted: {'yes' if ok else 'NO'}")
    text = "\n".join(lines)
    print(lines[-1])
    print(json.dumps(dict(quality=rows, accepted=bool(ok))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n" + json.dumps(dict(quality=rows, accepted=bool(ok))) + "\n")
    return 0 if ok else 1


def f16_ab(a):
    """lmi_train_f16 beside lmi_train on the same values"""
    import torch

    from kmeans_bench import PeakPoll

    reps = 5
    xt, yt = device_mixture(a.seed, a.n, a.d, a.classes)
    x16t = xt.half()
    del xt
    x32t = x16t.float()
    y = yt.cpu().numpy()
    forms = {"f32": (x32t.cpu().numpy(), x32t), "f16": (x16t.cpu().numpy(), x16t)}
    torch.manual_seed(a.seed)
    layers = linear_layers(NeuralNetwork(input_dim=a.d, output_dim=a.classes, lr=0.01, model_type=a.model).model)
    rows = NeuralNetwork.hip_batch_rows(np.random.default_rng(a.seed), a.n, a.epochs)
    lines = [f"train_bench --f16: {a.n} x {a.d}, {a.model}, {a.classes} classes, {a.epochs} steps on {rows.shape[1]} rows each, {reps} repeats, "
             f"the forms alternating; {torch.cuda.get_device_name(0)}; {_capi.lib().lmi_build_info().decode()}"]
    out, t = {}, {f: dict(host=[], dev=[]) for f in forms}
    for f, (xh, xd) in forms.items():   # warm-up, and the results
        out[f] = _capi.train(xh, y, layers, rows, 0.01)
        _capi.train(xd, yt, layers, rows, 0.01)
    flat = lambda o: [v for W, b in o[0] for v in (W, b)] + list(o[1][0]) + [o[2]]  # noqa: E731
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(flat(out["f32"]), flat(out["f16"]))), \
        "lmi_train_f16 and lmi_train differ on the same values"
    for _ in range(reps):
        for f, (xh, xd) in forms.items():
            t[f]["host"].append(wall(lambda: _capi.train(xh, y, layers, rows, 0.01))[1] * 1e3)
            t[f]["dev"].append(wall(lambda: _capi.train(xd, yt, layers, rows, 0.01))[1] * 1e3)
    res = dict(n=a.n, d=a.d, classes=a.classes, model=a.model, steps=a.epochs, rows_per_step=int(rows.shape[1]), bitwise_equal=True,
               build=_capi.lib().lmi_build_info().decode())
    lines.append("form   host arrays ms: median  min  max     device tensors ms: median  min  max     peak device MiB (polled, host arrays)")
    for f, (xh, xd) in forms.items():
        with PeakPoll() as peak:
            _capi.train(xh, y, layers, rows, 0.01)
        h, d = t[f]["host"], t[f]["dev"]
        lines.append(f"  {f}  {statistics.median(h):20.3f} {min(h):8.3f} {max(h):8.3f}   {statistics.median(d):22.3f} {min(d):8.3f} {max(d):8.3f}"
                     f"   {peak.peak / 2 ** 20:12.1f}")
        res[f] = dict(host_ms=h, device_ms=d, host_median_ms=statistics.median(h), device_median_ms=statistics.median(d),
                      peak_polled_bytes=int(peak.peak))
    for kind in ("host", "device"):
        spread = max(res["f32"][kind + "_ms"]) - min(res["f32"][kind + "_ms"])
        diff = res["f16"][kind + "_median_ms"] - res["f32"][kind + "_median_ms"]
        lines.append(f"  {kind}: spread of the float form's {reps}: {spread:.3f} ms; f16 - f32 (medians): {diff:+.3f} ms: "
                     + ("within the spread" if diff <= spread else "the half form is SLOWER by more than the spread"))
        res.update({kind + "_f32_spread_ms": spread, kind + "_f16_minus_f32_ms": diff})
    lines.append("  parameters, moments, t and losses of the two forms: equal bit for bit")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--classes", type=int, default=120)
    ap.add_argument("--model", default="MLP-4")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--torch-epochs", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quality", action="store_true", help="model quality of the two trainers instead of the timings")
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--f16", action="store_true", help="lmi_train_f16 beside lmi_train on the same values")
    a = ap.parse_args()
    if a.f16:
        _capi.lib()
        return f16_ab(a)
    if a.quality:
        _capi.lib()
        return quality(a)
    te = a.epochs if a.torch_epochs is None else a.torch_epochs

    import torch
    import torch.utils.data

    assert torch.cuda.is_available(), "train_bench needs the MI355X"
    _capi.lib()
    xt, yt = device_mixture(a.seed, a.n, a.d, a.classes)
    r = NeuralNetwork.hip_batch_size(a.n)
    lines = [f"train_bench: {a.n} x {a.d}, {a.model}, {a.classes} classes, {a.epochs} epochs (one step on {r} rows each), lr 0.01; "
             f"{torch.cuda.get_device_name(0)}; {_capi.lib().lmi_build_info().decode()}"]
    res = dict(n=a.n, d=a.d, classes=a.classes, model=a.model, epochs=a.epochs, rows_per_step=r, build=_capi.lib().lmi_build_info().decode())

    def fresh():
        torch.manual_seed(a.seed)
        return NeuralNetwork(input_dim=a.d, output_dim=a.classes, lr=0.01, model_type=a.model)

    x = y = None
    if te > 0:
        x, y = xt.cpu().numpy(), yt.cpu().numpy().astype(np.int64)
        batches = torch.utils.data.DataLoader(_PositionBatches(x, y), batch_size=MINI_BATCH, shuffle=True)
        fresh().train_batch(batches, epochs=1)   # warm-up
        net = fresh()
        _, train_s = wall(lambda: net.train_batch(batches, epochs=te))
        chosen, predict_s = wall(lambda: net.predict(x))
        per_epoch = train_s / te
        lines += ["torch trainer (s)",
                  f"  train_batch, {te} epochs                 {train_s:10.2f}   ({per_epoch:.3f} per epoch: {a.n} item fetches, "
                  f"{-(-a.n // MINI_BATCH)} forward passes, 1 step)",
                  f"  predict (host x, uploaded per call)     {predict_s:10.3f}",
                  f"  one round of {a.epochs} epochs + predict       {per_epoch * a.epochs + predict_s:10.2f}" + ("" if te == a.epochs else "   (scaled from the epochs timed)")]
        res.update(torch_epochs_timed=te, torch_train_s=train_s, torch_predict_s=predict_s, torch_round_s=per_epoch * a.epochs + predict_s,
                   torch_categories=int(len(np.unique(chosen))))

    def hip_round():
        net = fresh()
        t0 = time.perf_counter()
        tx, ty = (torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()) if x is not None else (xt, yt)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        net.train_batch_hip(tx, ty, epochs=a.epochs)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        chosen = net.predict(tx)
        t3 = time.perf_counter()
        return (t1 - t0, t2 - t1, t3 - t2, t3 - t0), chosen, net

    hip_round()   # warm-up
    runs = [hip_round() for _ in range(a.reps)]
    med = [statistics.median(run[0][i] for run in runs) for i in range(4)]
    lines += [f"hip trainer (s, median of {a.reps})",
              f"  upload of x, once                       {med[0]:10.3f}" + ("" if x is not None else "   (x was resident: nothing to upload)"),
              f"  train_batch_hip, {a.epochs} epochs             {med[1]:10.4f}",
              f"  predict (device x)                      {med[2]:10.4f}",
              f"  one round                               {med[3]:10.3f}"]
    res.update(hip_upload_s=med[0], hip_train_s=med[1], hip_predict_s=med[2], hip_round_s=med[3],
               hip_categories=int(len(np.unique(runs[-1][1]))))
    if te > 0:
        lines.append(f"  torch round / hip round = {res['torch_round_s'] / med[3]:.1f}; most of it is the {-(-a.n // MINI_BATCH) - 1} forward passes per "
                     "epoch whose result train_batch discards, and the item fetches behind them, which are no longer run")
    # the steps alone: lmi_train on the resident x, the difference between 2E and E steps
    layers = linear_layers(fresh().model)
    rng = np.random.default_rng(a.seed)
    rows = NeuralNetwork.hip_batch_rows(rng, a.n, 2 * a.epochs)
    t1, t2 = [], []
    _capi.train(xt, yt, layers, rows, 0.01)
    for _ in range(max(a.reps, 3)):
        t1.append(wall(lambda: _capi.train(xt, yt, layers, rows[: a.epochs], 0.01))[1])
        t2.append(wall(lambda: _capi.train(xt, yt, layers, rows, 0.01))[1])
    step_ms = (statistics.median(t2) - statistics.median(t1)) / a.epochs * 1e3
    dims = [a.d] + [W.shape[0] for W, _ in layers]
    flop = sum(6.0 * r * dims[i] * dims[i + 1] for i in range(len(layers))) - 2.0 * r * dims[0] * dims[1]
    lines += ["lmi_train alone, x resident (ms)",
              f"  {a.epochs} steps                                {statistics.median(t1) * 1e3:10.3f}",
              f"  {2 * a.epochs} steps                                {statistics.median(t2) * 1e3:10.3f}",
              f"  one step on the device                  {step_ms:10.4f}   ({3 * len(layers)} launches, {flop / 1e9:.3f} GFLOP: "
              f"{flop / (step_ms * 1e-3) / 1e12:.2f} TFLOP/s)"]
    res.update(train_call_ms=statistics.median(t1) * 1e3, train_call_2x_ms=statistics.median(t2) * 1e3, step_ms=step_ms, step_gflop=flop / 1e9)
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
