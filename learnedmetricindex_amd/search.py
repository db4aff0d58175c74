#!/usr/bin/env python3
"""Experiment driver for the MI355X build: build an index, answer the query set at several bucket budgets,
write one result file per budget.

It accepts the reference driver's command line (SURVEY.md section 5 "Config / flags"; reference
search/search.py:306-327) so that existing job scripts keep working:

    python learnedmetricindex_amd/search.py --dataset pca96v2 --emb pca96 --size 100K \\
        --n-categories 10 10 --epochs 100 --model-type MLP --lr 0.01 -bp 10 --clustering-algorithm scikit_kmeans

and produces the reference's result schema (datasets `knns` uint32 / `dists` float64, attributes `algo, data,
buildtime, querytime, size, params`; search/search.py:51-63) so the SISAP `eval` tooling reads it.  Everything
else is this build's own structure:

    Experiment   the parsed command line (per-level lists expanded)
    VectorSource where the vectors come from: local `data/<kind>/<size>/{dataset,query}.(h5|npy)` or, only
                 when `--synthetic` is given, a generated stand-in whose results are stamped `synthetic-<kind>`
    ResultSink   `.h5` when h5py is importable, `.npz` with the same keys otherwise
    run()        build (LearnedIndexBuilder) -> one resident index in HBM -> `search_resident` per budget ->
                 optional recall@k against the GPU brute-force `Baseline`

Flags the reference parses but ignores are accepted and ignored the same way (`-b/--n-buckets`); its
`type=bool` flags (`--preprocess`, `--save`) keep "any non-empty string is true".  Downloading from the SISAP
S3 bucket is not supported (no network on the target machines): place the files locally or use `--synthetic`.
"""
from __future__ import annotations

import argparse
import dataclasses
import logging
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:  # `li` importable next to this file, as in the reference layout
    sys.path.insert(0, _HERE)

import _capi  # noqa: E402  (the module `li` binds when it is imported as a top-level package)
from li.Baseline import Baseline  # noqa: E402
from li.BuildConfiguration import BuildConfiguration  # noqa: E402
from li.clustering import algorithms  # noqa: E402
from li.LearnedIndexBuilder import LearnedIndexBuilder  # noqa: E402
from li.utils import save_as_pickle, serialize  # noqa: E402

LOG = logging.getLogger("lmi.driver")

SCAN_KIND, SCAN_KEY = "clip768v2", "emb"   # the scan always runs on the 768-d embeddings
PER_LEVEL = ("clustering_algorithm", "model_type", "epochs", "lr")
CARDINALITY = {"100K": 100_000, "300K": 300_000, "10M": 10_000_000, "30M": 30_000_000, "100M": 100_000_000}
WIDTH = {"clip768v2": 768, "pca96v2": 96, "pca32v2": 32}
QUERY_COUNT = 10_000


# ------------------------------------------------------------------------------------------- command line
@dataclasses.dataclass
class Experiment:
    dataset: str
    emb: str
    size: str
    k: int
    n_categories: List[int]
    epochs: List[int]
    model_type: List[str]
    lr: List[float]
    buckets_perc: List[int]
    preprocess: bool
    save: bool
    clustering_algorithm: List[str]
    synthetic: bool = False
    evaluate: bool = False
    job: str = "unknown"
    stop_mass: Optional[float] = None
    path_mass: Optional[float] = None
    stop_rows: Optional[int] = None
    storage: str = "f32"
    trainer: str = "torch"
    merge: str = "ranks"
    range_radius: Optional[float] = None
    range_sort: bool = False
    range_exact: bool = False

    @classmethod
    def from_argv(cls, argv: Optional[Sequence[str]] = None) -> "Experiment":
        p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
        p.add_argument("--dataset", default="pca96v2")
        p.add_argument("--emb", default="pca96")
        p.add_argument("--size", default="100K", choices=sorted(CARDINALITY, key=CARDINALITY.get))
        p.add_argument("--k", default=10, type=int)
        p.add_argument("--n-categories", nargs="+", default=[10, 10], type=int)
        p.add_argument("--epochs", nargs="+", default=[100], type=int)
        p.add_argument("--model-type", nargs="+", default=["MLP"])
        p.add_argument("--lr", nargs="+", default=[0.01], type=float)
        p.add_argument("-b", "--n-buckets", nargs="+", default=[2, 3, 4], type=int, help="accepted, unused (as upstream)")
        p.add_argument("-bp", "--buckets-perc", nargs="+", default=[10], type=int)
        p.add_argument("--preprocess", default=True, type=bool)
        p.add_argument("--save", default=True, type=bool)
        p.add_argument("--clustering-algorithm", nargs="+", default=["faiss_kmeans"], choices=sorted(algorithms))
        p.add_argument("--synthetic", action="store_true",
                       help="generate stand-in vectors when the dataset files are missing (results are stamped synthetic)")
        p.add_argument("--eval", dest="evaluate", action="store_true", help="report recall@k against GPU brute force")
        p.add_argument("--stop-mass", type=float, default=None,
                       help="1-level indexes: a query stops visiting buckets once the visited ranks' probabilities sum to this "
                            "(0 < mass <= 1); default: every query visits its whole budget")
        p.add_argument("--path-mass", type=float, default=None,
                       help="multi-level indexes: a query's walk stops once the path probabilities of the buckets it has recorded "
                            "sum to this (0 < mass <= 1); default: every query visits its whole budget")
        p.add_argument("--stop-rows", type=int, default=None,
                       help="any index: a query stops visiting buckets once the buckets it has visited hold this many objects "
                            "(an integer >= 1; the bucket that crosses the budget is scanned whole); default: every query visits its "
                            "whole budget")
        p.add_argument("--storage", choices=("f32", "f16"), default="f32",
                       help="how the resident index keeps the scan vectors: f16 = the fp16 fragments only, a third of the device memory, "
                            "for vectors that are binary16-exact (refused otherwise); same results")
        p.add_argument("--trainer", choices=("torch", "hip"), default="torch",
                       help="how the nodes' models are trained: torch = the reference's loop (autograd, a DataLoader pass per epoch); "
                            "hip = its effective schedule on the device (lmi_train), repeatable bit for bit")
        p.add_argument("--merge", choices=("ranks", "union"), default="ranks",
                       help="ranks = at most 10 results per visited bucket, merged by rank (the reference; k <= 20); union = the k best "
                            "objects of all visited buckets, k up to 1024 -- with --eval, recall@k then measures what the index returned "
                            "for that k")
        p.add_argument("--range-radius", type=float, default=None,
                       help="also run a range search per budget: every object of the visited buckets within this distance of the "
                            "query; the results per query (mean, max) are reported -- with --eval also the recall against the "
                            "exhaustive range query over all objects (GPU brute force)")
        p.add_argument("--range-sort", action="store_true",
                       help="with --range-radius: every query's range results nearest first, sorted on the device")
        p.add_argument("--range-exact", action="store_true",
                       help="with --range-radius: also answer the range query EXACTLY through the index -- every object within the "
                            "radius, visiting only the buckets whose covering ball the query's ball may meet; the visited fraction of "
                            "the buckets and the time are reported -- with --eval also range_recall_exact, which must print 1.0")
        a = vars(p.parse_args(argv))
        a.pop("n_buckets")
        levels = len(a["n_categories"])
        if a["stop_mass"] is not None and levels > 1:
            p.error("--stop-mass needs a 1-level index (one value for --n-categories)")
        if a["stop_mass"] is not None and not 0.0 < a["stop_mass"] <= 1.0:
            p.error("--stop-mass must lie in (0, 1]")
        if a["path_mass"] is not None and levels == 1:
            p.error("--path-mass needs a multi-level index (on a 1-level index use --stop-mass)")
        if a["path_mass"] is not None and not 0.0 < a["path_mass"] <= 1.0:
            p.error("--path-mass must lie in (0, 1]")
        if a["stop_rows"] is not None and a["stop_rows"] < 1:
            p.error("--stop-rows must be an integer >= 1")
        if a["merge"] == "union" and not 1 <= a["k"] <= 1024:
            p.error("--merge union takes --k from 1 to 1024")
        if a["merge"] == "union" and a["storage"] != "f32":
            p.error("--merge union needs --storage f32 (the union scan reads the row-major f32 image)")
        if a["range_radius"] is not None and a["storage"] != "f32":
            p.error("--range-radius needs --storage f32 (the range search reads the row-major f32 image)")
        if a["range_radius"] is not None and a["range_radius"] != a["range_radius"]:
            p.error("--range-radius must be a number")
        if a["range_sort"] and a["range_radius"] is None:
            p.error("--range-sort needs --range-radius")
        if a["range_exact"] and a["range_radius"] is None:
            p.error("--range-exact needs --range-radius")
        if a["range_exact"] and a["storage"] != "f32":
            p.error("--range-exact needs --storage f32 (the bucket cover reads the row-major f32 image)")
        for name in PER_LEVEL:  # one value for all levels, or one per level
            if len(a[name]) == 1:
                a[name] = a[name] * levels
            elif len(a[name]) != levels:
                p.error(f"--{name.replace('_', '-')} needs 1 or {levels} values, got {len(a[name])}")
        return cls(job=os.environ.get("PBS_JOBID", "unknown"), **a)

    def build_configuration(self) -> BuildConfiguration:
        return BuildConfiguration([algorithms[c] for c in self.clustering_algorithm], self.epochs, self.model_type,
                                  self.lr, self.n_categories)

    def tag(self, prefix: str, **extra) -> str:
        """File-name stem in the upstream format: <prefix>-ep=..-lr=..-cat=..-model=..[-k=v..]-<job>."""
        parts = [prefix, f"ep={serialize(self.epochs)}", f"lr={serialize(self.lr)}", f"cat={serialize(self.n_categories)}",
                 f"model={serialize(self.model_type)}"]
        parts += [f"{k}={v}" for k, v in extra.items()]
        parts += [f"clustering_algorithm={serialize(self.clustering_algorithm)}", self.job]
        return "-".join(parts)


# ------------------------------------------------------------------------------------------- vectors
class VectorSource:
    """`data/<kind>/<size>/{dataset,query}.h5|.npy`; synthetic stand-ins only on request."""

    def __init__(self, size: str, synthetic: bool, root: str = "data"):
        self.size, self.synthetic, self.root = size, synthetic, root
        self.generated = set()

    def _path(self, kind: str, what: str, ext: str) -> str:
        return os.path.join(self.root, kind, self.size, f"{what}.{ext}")

    def load(self, kind: str, key: str, keep_f16: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """(objects f32[N,d], queries f32[nq,d]) of embedding `kind`.  `keep_f16`: arrays the files hold as float16 are returned as
        float16 -- for `--storage f16`, which takes halves as they are (no host copy of twice the size)."""
        out = []
        for what in ("dataset", "query"):
            if os.path.exists(self._path(kind, what, "h5")):
                import h5py

                with h5py.File(self._path(kind, what, "h5"), "r") as fh:
                    out.append(np.asarray(fh[key], dtype=np.float16 if keep_f16 and fh[key].dtype == np.float16 else np.float32))
            elif os.path.exists(self._path(kind, what, "npy")):
                a = np.load(self._path(kind, what, "npy"))
                out.append(a if keep_f16 and a.dtype == np.float16 else a.astype(np.float32, copy=False))
            elif self.synthetic:
                self.generated.add(kind)
                out.append(self._generate(kind, what))
            else:
                raise FileNotFoundError(
                    f"{self._path(kind, what, 'h5')} (or .npy) not found; there is no network access to fetch the SISAP "
                    f"files -- copy them there or pass --synthetic for a generated stand-in")
        return out[0], out[1]

    def _generate(self, kind: str, what: str) -> np.ndarray:
        """Unit-norm mixture of 256 Gaussians in 768-d; the narrower kinds are one fixed random projection of the
        same objects (so that `pca32v2` navigation and `clip768v2` scan describe the same set)."""
        n = CARDINALITY[self.size] if what == "dataset" else QUERY_COUNT
        d = WIDTH[kind]
        centres = np.random.RandomState(2023).randn(256, 768).astype(np.float32)
        proj = None if d == 768 else (np.random.RandomState(d).randn(768, d) / np.sqrt(768.0)).astype(np.float32)
        rs = np.random.RandomState(11 if what == "dataset" else 12)
        out = np.empty((n, d), dtype=np.float32)
        step = 1 << 17
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            x = centres[rs.randint(256, size=hi - lo)] + rs.randn(hi - lo, 768).astype(np.float32)
            x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
            out[lo:hi] = x if proj is None else x @ proj
        return out

    def stamp(self, kind: str) -> str:
        return f"synthetic-{kind}" if kind in self.generated else kind


def unit_rows(x: np.ndarray) -> np.ndarray:
    """sklearn.preprocessing.normalize(x) (l2, zero rows untouched) without the dependency."""
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return (x / np.where(n == 0, 1, n)).astype(np.float32)


# ------------------------------------------------------------------------------------------- results
class ResultSink:
    """One file per bucket budget under result/<kind>/<size>/ with the upstream schema."""

    def __init__(self, root: str = "result"):
        self.root = root
        try:
            import h5py  # noqa: F401

            self.h5 = True
        except ImportError:
            self.h5 = False

    def write(self, folder_kind: str, folder_size: str, stem: str, dists: np.ndarray, knns: np.ndarray, **attrs) -> str:
        folder = os.path.join(self.root, folder_kind, folder_size)
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, stem + (".h5" if self.h5 else ".npz"))
        if self.h5:
            import h5py

            with h5py.File(path, "w") as fh:
                fh.attrs.update(attrs)
                fh.create_dataset("knns", data=knns)
                fh.create_dataset("dists", data=dists)
        else:
            np.savez(path, knns=knns, dists=dists, **attrs)
        LOG.info("results -> %s", path)
        return path


# ------------------------------------------------------------------------------------------- the run
def bucket_budgets(percentages: Sequence[int], n_buckets_in_index: int) -> List[int]:
    """`-bp`: per cent of the index's buckets -> bucket counts, int(p/100 * n) like upstream; zeros dropped."""
    return sorted({b for b in (int(p / 100 * n_buckets_in_index) for p in percentages) if b > 0})


def recall_against_bruteforce(queries: np.ndarray, objects: pd.DataFrame, knns: np.ndarray, k: int, sample: int = 1000):
    """recall@k of the first `sample` queries (notebook cell 31: |found & true| / (k * nq)); ground truth from the
    GPU brute-force Baseline over the scan vectors."""
    # k <= 10: as before; 10 < k <= Baseline.MAX_K (LMI_KNN_MAX_K): the truth has k neighbours too (Baseline goes through lmi_knn), so this is recall@k
    m, kk = min(sample, knns.shape[0]), (k if k <= Baseline.MAX_K else 10)
    _, truth, _ = Baseline().search(queries[:m].astype(np.float32, copy=False), objects.to_numpy(dtype=np.float32), k=kk)
    labels = objects.index.to_numpy()
    truth = labels[truth - 1]  # Baseline ids are 1-based positions
    return float(np.mean([len(set(t) & set(f)) / kk for t, f in zip(truth.tolist(), knns[:m, :k].tolist())]))


def range_recall(lims_found, ids_found, lims_true, ids_true) -> float:
    """Recall of a range search against the exhaustive one: sum |found & true| / sum |true| over the queries of `lims_true`, found
    and true being the SETS of object ids of a query (query q owns [lims[q], lims[q + 1]) of its ids; an id found twice counts once);
    1.0 where the truth is empty.  `lims_found` may cover more queries than `lims_true`: the first ones are compared."""
    lf, lt = np.asarray(lims_found, dtype=np.int64), np.asarray(lims_true, dtype=np.int64)
    found, true = np.asarray(ids_found), np.asarray(ids_true)
    assert lf.shape[0] >= lt.shape[0] >= 1
    hit = total = 0
    for q in range(lt.shape[0] - 1):
        t = set(true[lt[q]:lt[q + 1]].tolist())
        hit += len(t & set(found[lf[q]:lf[q + 1]].tolist()))
        total += len(t)
    return hit / total if total else 1.0


def range_truth(queries: np.ndarray, objects: pd.DataFrame, radius: float, sample: int = 1000):
    """(lims, object ids) of the exhaustive range query (`lmi_knn_range`) of the first `sample` queries over the scan vectors AS THE
    INDEX HOLDS THEM -- not re-normalised: a radius is an absolute distance.  Rows map to ids through `objects.index`.
    Where the frame and the queries are both held as float16 (`--storage f16` on files of 16-bit floats) they go to the call as
    halves (`lmi_knn_range_f16`: the same result bit for bit, and no float32 copy of the data on the host); otherwise as float32.
    (The top-k truth of `recall_against_bruteforce` cannot do the same: `li.Baseline` re-normalises its rows in float32.)"""
    m = min(sample, queries.shape[0])
    f16 = queries.dtype == np.float16 and bool((objects.dtypes == np.float16).all())
    dtype = np.float16 if f16 else np.float32
    with _capi.range_knn(np.ascontiguousarray(queries[:m], dtype=dtype), objects.to_numpy(dtype=dtype), radius, metric="ip") as res:
        _, rows = res.read()
        return res.lims, objects.index.to_numpy()[rows.astype(np.int64)]


def run(exp: Experiment) -> Dict:
    LOG.info("experiment: %s", dataclasses.asdict(exp))
    src = VectorSource(exp.size, exp.synthetic)
    nav_x, nav_q = src.load(exp.dataset, exp.emb)
    if exp.preprocess:
        nav_x, nav_q = unit_rows(nav_x), unit_rows(nav_q)
    LOG.info("navigation vectors %s, queries %s", nav_x.shape, nav_q.shape)
    nav = pd.DataFrame(nav_x)
    nav.index += 1  # object ids are 1-based
    # --storage f16: scan vectors that the files hold as float16 go to the library as halves, unwidened.  Only where the scan
    # vectors are a dataset of their own: when one dataset serves navigation and scan, the builder needs it as float32 anyway and a
    # second, float16 copy would cost host memory instead of saving it.  The scan queries stay halves too, but beside float32
    # navigation queries they are widened on the host (`_capi._queries`): the driver saves on the ingest, not on the query upload.
    keep_f16 = exp.storage == "f16"
    if exp.dataset == SCAN_KIND:
        scan, scan_q = nav, nav_q
    else:  # navigate in the narrow embedding, scan in clip768v2 (not normalised by the driver, as upstream)
        sx, scan_q = src.load(SCAN_KIND, SCAN_KEY, keep_f16=keep_f16)
        scan = pd.DataFrame(sx)
        scan.index += 1
        LOG.info("scan vectors %s, queries %s", scan.shape, scan_q.shape)

    t0 = time.time()
    index, placement, n_buckets_in_index, build_s, cluster_s = LearnedIndexBuilder(nav, exp.build_configuration(), trainer=exp.trainer).build()
    LOG.info("index with %d buckets: clustering %.2fs, build %.2fs, total %.2fs", n_buckets_in_index, cluster_s, build_s,
             time.time() - t0)
    if exp.save:
        os.makedirs("models", exist_ok=True)
        save_as_pickle(os.path.join("models", exp.tag(f"{exp.dataset}-{exp.size}", prep=exp.preprocess) + ".pkl"), index)

    index.prepare(nav, scan, placement, exp.n_categories, storage=exp.storage)  # one upload; every budget below reuses the resident slab
    sink, out, truth = ResultSink(), {}, None
    for budget in bucket_budgets(exp.buckets_perc, n_buckets_in_index):
        dists, knns, clock = index.search_resident(nav_q, scan_q, exp.n_categories, n_buckets=budget, k=exp.k, stop_mass=exp.stop_mass,
                                                     path_mass=exp.path_mass, stop_rows=exp.stop_rows, merge=exp.merge)
        LOG.info("%d buckets: search %.4fs (inference %.4fs, within buckets %.4fs, scan %.4fs, merge %.4fs)", budget,
                 clock["search"], clock["inference"], clock["search_within_buckets"], clock["seq_search"], clock["sort"])
        if exp.evaluate:
            out[f"recall_{budget}"] = recall_against_bruteforce(scan_q, scan, knns, exp.k)
            LOG.info("%d buckets: recall@%d = %.5f", budget, exp.k, out[f"recall_{budget}"])
        stem = exp.tag(f"learned-index-{exp.dataset}-{exp.size}", buck=budget, **({} if exp.stop_mass is None else {"stop": exp.stop_mass}),
                       **({} if exp.path_mass is None else {"pathmass": exp.path_mass}),
                       **({} if exp.stop_rows is None else {"stoprows": exp.stop_rows}),
                       **({} if exp.merge == "ranks" else {"merge": exp.merge}))
        sink.write(exp.dataset, exp.size, stem, dists, knns, algo="Learned-index", data=src.stamp(exp.dataset),
                   buildtime=build_s, querytime=clock["search"], size=exp.size, params=stem)
        out[budget] = (dists, knns, clock)
        if exp.range_radius is not None:
            lims, _, found, rclock = index.range_search_resident(nav_q, scan_q, exp.n_categories, exp.range_radius, n_buckets=budget,
                                                             sort=exp.range_sort, stop_mass=exp.stop_mass, path_mass=exp.path_mass,
                                                             stop_rows=exp.stop_rows)
            per_query = np.diff(lims)
            out[f"range_{budget}"] = (float(per_query.mean()) if per_query.size else 0.0, int(per_query.max(initial=0)))
            LOG.info("%d buckets: range search within %g: %.4fs, results per query mean %.2f, max %d", budget, exp.range_radius,
                     rclock["search"], *out[f"range_{budget}"])
            if exp.evaluate:
                if truth is None:   # one exhaustive scan serves every budget
                    truth = range_truth(scan_q, scan, exp.range_radius)
                out[f"range_recall_{budget}"] = range_recall(lims, found, *truth)
                LOG.info("%d buckets: range recall within %g = %.5f (%d true results over %d queries)", budget, exp.range_radius,
                         out[f"range_recall_{budget}"], int(truth[0][-1]), len(truth[0]) - 1)
    if exp.range_exact:   # once, not per budget: the exact call has no budget
        lims, _, found, xclock = index.range_search_exact_resident(nav_q, scan_q, exp.n_categories, exp.range_radius, sort=exp.range_sort)
        out["range_exact_visited"] = xclock["buckets_visited"] / n_buckets_in_index
        out["range_exact_seconds"] = xclock["search"]
        per_query = np.diff(lims)
        LOG.info("exact range search within %g: %.4fs (cover %.4fs), %.4f of the %d buckets visited per query, results per query mean %.2f, "
                 "max %d", exp.range_radius, xclock["search"], xclock["cover"], out["range_exact_visited"], n_buckets_in_index,
                 float(per_query.mean()) if per_query.size else 0.0, int(per_query.max(initial=0)))
        if exp.evaluate:
            if truth is None:
                truth = range_truth(scan_q, scan, exp.range_radius)
            out["range_recall_exact"] = range_recall(lims, found, *truth)
            LOG.info("exact range search: range_recall_exact = %s (%d true results over %d queries)", out["range_recall_exact"],
                     int(truth[0][-1]), len(truth[0]) - 1)
    index.close()
    return out


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s][%(levelname)-5.5s][%(name)-.20s] %(message)s")
    np.random.seed(2023)
    return run(Experiment.from_argv(argv))


if __name__ == "__main__":
    main()
