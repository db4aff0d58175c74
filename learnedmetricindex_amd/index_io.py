"""On-disk index: everything `LearnedIndex.search` needs, without the
DataFrames -- replaces the reference's whole-object pickle (search.py:234-241, utils.py:14-29),
which stores the models only and drops `data_prediction` and the vectors.

    <dir>/meta.json      format/version, N, d, metric ("ip" | "l2"), storage ("f32" | "f16"; optional, absent = "f32"),
                         vectors ("f16"; optional, absent = "f32": which vectors file the directory holds),
                         n_categories, bucket paths, model descriptions
    <dir>/weights.npz    Linear weights/biases of the root and internal models (float32)
    <dir>/sizes.npy      int64 [B]    objects per bucket, in bucket-id order
    <dir>/ids.npy        uint32 [N]   object labels, bucket-contiguous
    <dir>/vectors.f32.npy   float32 [N, d] scan vectors, bucket-contiguous row-major (memory-mappable) -- or, written from an
    <dir>/vectors.f16.npy   f16-resident index, the same as float16 [N, d]: the halves the index holds, half the bytes

`save_index` reads the vectors back from HBM bucket by bucket (lmi_bucket_read); `load_index` streams
them into a fresh device slab in pieces, so neither needs N x d floats of host memory at once."""
import json
import os
from typing import List, Tuple

import numpy as np

from . import _capi
from .li.LearnedIndex import LearnedIndex
from .li.model import linear_layers, network_from_layers

FORMAT, VERSION = "lmi-mi355x-index", 2   # 2: + "metric" (a version-1 directory has none: inner product)


def _put(store, prefix, net):
    layers = linear_layers(net.model)
    for i, (W, b) in enumerate(layers):
        store[f"{prefix}W{i}"], store[f"{prefix}b{i}"] = W, b
    return len(layers)


def _get(store, prefix, n):
    return [(store[f"{prefix}W{i}"], store[f"{prefix}b{i}"]) for i in range(n)]


def vectors_file(meta: dict):
    """(file name, dtype) of the scan vectors of a directory with this meta.json: the optional key "vectors" names the
    element type ("f16": vectors.f16.npy); a directory without it holds vectors.f32.npy."""
    kind = meta.get("vectors", "f32")
    assert kind in ("f32", "f16"), f"unknown vectors type {kind!r} in meta.json"
    return f"vectors.{kind}.npy", np.dtype(np.float16 if kind == "f16" else np.float32)


def save_index(path: str, li: LearnedIndex, n_categories: List[int]) -> None:
    """Writes the resident index of `li` (after prepare()/search()) to directory `path`."""
    eng = li._engine
    assert eng is not None, "nothing resident: call li.prepare(...) or li.search(...) first"
    os.makedirs(path, exist_ok=True)
    sizes = eng.bucket_sizes()
    N, d = int(sizes.sum()), eng.d
    weights = {}
    meta = {"format": FORMAT, "version": VERSION, "N": N, "d": d, "metric": eng.metric, "n_categories": [int(v) for v in n_categories],
            "bucket_paths": [[int(v) for v in p] for p in li.bucket_paths],
            "root_layers": _put(weights, "root_", li.root_model), "internal": []}
    if getattr(eng, "storage", "f32") != "f32":   # how the index was resident; a reader that does not know the key loads an
        meta["storage"] = eng.storage             # f32-resident index: same results
    if getattr(eng, "storage", "f32") == "f16":   # ... and its vectors go to disk as the halves it holds (every other engine:
        meta["vectors"] = "f16"                   # vectors.f32.npy and no key, as ever)
    vname, vdtype = vectors_file(meta)
    for i, (p, net) in enumerate(li.internal_models.items()):
        meta["internal"].append({"path": [int(v) for v in p], "layers": _put(weights, f"int{i}_", net)})
    if li._path_ids is not None:  # multi-level: bucket id -> path
        meta["paths"] = [list(p) for p, _ in sorted(li._path_ids.items(), key=lambda kv: kv[1])]
    np.savez(os.path.join(path, "weights.npz"), **weights)
    np.save(os.path.join(path, "sizes.npy"), sizes)
    ids = np.empty(N, dtype=np.uint32)
    vec = np.lib.format.open_memmap(os.path.join(path, vname), mode="w+", dtype=vdtype, shape=(N, d))
    o = 0
    for b, n in enumerate(sizes):
        if n:
            rows, bid = eng.read_bucket(b) if vdtype == np.float32 else eng.read_bucket(b, dtype=vdtype)
            vec[o:o + n], ids[o:o + n] = rows, bid
            o += int(n)
    vec.flush()
    del vec
    np.save(os.path.join(path, "ids.npy"), ids)
    with open(os.path.join(path, "meta.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


def load_index(path: str, device: int = 0, storage=None) -> Tuple[LearnedIndex, List[int]]:
    """(LearnedIndex with the index resident on `device`, n_categories); use `li.search_resident`.  `storage`: None = as the
    directory says (its "storage" key; absent: "f32"), or "f32" / "f16" to override it."""
    meta = json.load(open(os.path.join(path, "meta.json")))
    assert meta["format"] == FORMAT and meta["version"] in (1, VERSION), f"unknown index format {meta.get('format')} v{meta.get('version')}"
    metric = meta.get("metric", "ip")
    assert metric in _capi.Index.METRICS, f"unknown metric {metric!r} in {path}/meta.json"
    store = np.load(os.path.join(path, "weights.npz"))
    root = network_from_layers(_get(store, "root_", meta["root_layers"]))
    internal = {tuple(e["path"]): network_from_layers(_get(store, f"int{i}_", e["layers"]))
                for i, e in enumerate(meta["internal"])}
    li = LearnedIndex(root, internal, [tuple(p) for p in meta["bucket_paths"]])
    sizes = np.load(os.path.join(path, "sizes.npy"))
    ids = np.load(os.path.join(path, "ids.npy"))
    vec = np.load(os.path.join(path, vectors_file(meta)[0]), mmap_mode="r")   # halves are streamed in as halves, into either storage
    if storage is None:
        storage = meta.get("storage", "f32")
    assert storage in _capi.Index.STORAGES, f"unknown storage {storage!r}"
    eng = _capi.Index(device, metric=metric, storage=storage)
    if len(meta["n_categories"]) == 1:
        eng.set_mlp(linear_layers(root.model))
    else:
        li._path_ids = {tuple(p): i for i, p in enumerate(meta["paths"])}
        li._upload_tree(eng, len(meta["n_categories"]))  # the nodes' models + the tree for the device-side walk
    labels = np.repeat(np.arange(sizes.shape[0], dtype=np.int64), sizes)
    eng.buckets_begin(labels, int(meta["d"]), int(sizes.shape[0]), ids=ids)
    piece = max(1, (256 << 20) // (4 * int(meta["d"])))
    for r0 in range(0, vec.shape[0], piece):
        eng.add_rows(np.ascontiguousarray(vec[r0:r0 + piece]), r0)
    eng.buckets_end()
    li._engine, li._engine_key = eng, ("disk", os.path.abspath(path))
    return li, [int(v) for v in meta["n_categories"]]
