"""Exact k-NN baseline on the MI355X (the role of reference li/Baseline.py:7-21: ground truth for recall).

Cosine distance by brute force: rows are L2-normalised on the host, then ONE `lmi_knn_ip` call (the C ABI's
`faiss.knn(..., METRIC_INNER_PRODUCT)` replacement: fp16-MFMA prefilter + exact binary32 re-rank over a
single-bucket index in HBM) yields the k largest inner products per query; distance = 1 - similarity.
`k` above 10, up to `MAX_K`, goes through `lmi_knn` instead (exact binary32 brute force, no index).
`range_search` (an extension) is the range query's ground truth the same way: `lmi_knn_range` on the unit rows.
Same call surface as the reference class: `search(queries, data, k) -> (dists, ids 1-based, seconds)`,
`build(data) -> seconds`.  There is no CPU path here; `li.utils.pairwise_cosine` remains for callers that
want the sklearn form."""
import time

import numpy as np

from .Logger import Logger

try:
    from .. import _capi
except ImportError:  # pragma: no cover  (`li` used as a top-level package next to _capi.py)
    import _capi  # type: ignore


def _unit(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = np.linalg.norm(x, axis=1, keepdims=True)
    return x / np.where(n == 0, 1, n)


class Baseline(Logger):
    MAX_K = _capi.KNN_MAX_K  # k <= 10: lmi_knn_ip (LearnedIndex.py:334), as before; above it the exact k-NN call lmi_knn

    def build(self, data) -> float:
        """Nothing to build: the scan is exhaustive."""
        self.logger.info("Baseline: exhaustive GPU scan, no index to build.")
        return 0.0

    def search(self, queries, data, k: int = 10, device: int = 0):
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"Baseline.search: k must be in [1, {self.MAX_K}]")
        t0 = time.time()
        if k <= _capi.K_PER_BUCKET:
            sims, rows = _capi.knn_ip(_unit(queries), _unit(data), k=k, device=device)
        else:
            sims, rows = _capi.knn(_unit(queries), _unit(data), k=k, metric="ip", device=device)
        found = rows >= 0  # fewer than k objects: faiss-style padding (-1)
        dists = np.where(found, np.float32(1) - sims, np.float32(np.inf))
        return dists, np.where(found, rows + 1, 0), time.time() - t0

    def search_hamming(self, queries, data, k: int = 10, device: int = 0):
        """`search` on bit-packed codes under the Hamming distance (`lmi_knn_hamming`): (dists int32[nq,k], ids 1-based, seconds).
        `queries`, `data`: uint8 arrays [n, code_bytes], or uint64 word arrays [n, words] as the challenge's `hammingv2` files hold
        them -- viewed as bytes without a copy.  Fewer than k objects pad with ids = 0 and dists = the largest int32."""
        if not 1 <= k <= self.MAX_K:
            raise ValueError(f"Baseline.search_hamming: k must be in [1, {self.MAX_K}]")
        codes = []
        for name, a in (("queries", queries), ("data", data)):
            a = np.asarray(a)
            if a.dtype not in (np.uint8, np.uint64) or a.ndim != 2:
                raise ValueError(f"Baseline.search_hamming: {name} must be a two-dimensional uint8 or uint64 array, not {a.dtype}{tuple(a.shape)}")
            codes.append(np.ascontiguousarray(a).view(np.uint8))
        t0 = time.time()
        dists, rows = _capi.knn_hamming(codes[0], codes[1], k=k, device=device)
        return dists, np.where(rows >= 0, rows + 1, 0), time.time() - t0

    def rerank(self, queries, data, candidates, k: int = 10, device: int = 0):
        """`search` restricted to per-query candidate lists (`lmi_knn_rerank` on the unit rows): (dists, ids 1-based, seconds).
        `candidates`: integer ids [nq, c], 1-based with 0 for "none", as `search` and `search_hamming` return them; c <= MAX_K,
        k <= c.  Where a list holds the true k nearest objects the result is `search`'s."""
        cand = np.asarray(candidates)
        if cand.ndim != 2 or cand.dtype.kind not in "iu":
            raise ValueError(f"Baseline.rerank: candidates must be a two-dimensional integer array, not {cand.dtype}{tuple(cand.shape)}")
        if not 1 <= cand.shape[1] <= self.MAX_K or not 1 <= k <= cand.shape[1]:
            raise ValueError(f"Baseline.rerank: c = {cand.shape[1]} must be in [1, {self.MAX_K}] and k = {k} in [1, c]")
        if np.ndim(queries) != 2 or np.ndim(data) != 2 or np.shape(queries)[0] != cand.shape[0] or np.shape(queries)[1] != np.shape(data)[1]:
            raise ValueError(f"Baseline.rerank: queries {np.shape(queries)}, data {np.shape(data)} and candidates {cand.shape} do not fit")
        t0 = time.time()
        sims, rows = _capi.knn_rerank(_unit(queries), _unit(data), cand.astype(np.int64) - 1, k, metric="ip", device=device)
        found = rows >= 0
        dists = np.where(found, np.float32(1) - sims, np.float32(np.inf))
        return dists, np.where(found, rows + 1, 0), time.time() - t0

    def search_sketch(self, queries, data, query_codes, data_codes, k: int = 10, n_candidates: int = 1024, device: int = 0):
        """The sketch-filter baseline, two stages on the device: `search_hamming(query_codes, data_codes, k=n_candidates)`, then
        `rerank` of those candidates on the vectors: (dists, ids 1-based, seconds) in `search`'s shape.  There is no CPU path."""
        if not 1 <= n_candidates <= self.MAX_K or not 1 <= k <= n_candidates:
            raise ValueError(f"Baseline.search_sketch: n_candidates = {n_candidates} must be in [1, {self.MAX_K}] and k = {k} in [1, n_candidates]")
        if np.ndim(queries) != 2 or np.ndim(data) != 2 or np.shape(queries)[1] != np.shape(data)[1]:
            raise ValueError(f"Baseline.search_sketch: queries {np.shape(queries)} and data {np.shape(data)} do not fit")
        if len(query_codes) != len(queries) or len(data_codes) != len(data):
            raise ValueError("Baseline.search_sketch: one code per query and one per object")
        t0 = time.time()
        _, cand, _ = self.search_hamming(query_codes, data_codes, k=n_candidates, device=device)
        dists, ids, _ = self.rerank(queries, data, cand, k=k, device=device)
        return dists, ids, time.time() - t0

    def search_sketched(self, queries, data, sketcher, k: int = 10, n_candidates: int = 1024, device: int = 0):
        """`search_sketch` from the vectors alone: `sketcher` (a `projection.SketchProjection`) encodes the unit rows of `queries`
        and `data` on the device (`lmi_sketch`), then the Hamming filter and the exact re-rank run as in `search_sketch`."""
        if not (hasattr(sketcher, "encode") and hasattr(sketcher, "d")):
            raise ValueError("Baseline.search_sketched: sketcher must be a projection.SketchProjection")
        if not 1 <= n_candidates <= self.MAX_K or not 1 <= k <= n_candidates:
            raise ValueError(f"Baseline.search_sketched: n_candidates = {n_candidates} must be in [1, {self.MAX_K}] and k = {k} in [1, n_candidates]")
        if np.ndim(queries) != 2 or np.ndim(data) != 2 or not np.shape(queries)[1] == np.shape(data)[1] == sketcher.d:
            raise ValueError(f"Baseline.search_sketched: queries {np.shape(queries)}, data {np.shape(data)} and the sketcher's d = "
                             f"{sketcher.d} do not fit")
        t0 = time.time()
        codes = [sketcher.encode(_unit(a), device=device) for a in (queries, data)]   # (the re-rank normalises the rows itself)
        dists, ids, _ = self.search_sketch(queries, data, codes[0], codes[1], k=k, n_candidates=n_candidates, device=device)
        return dists, ids, time.time() - t0

    def range_search(self, queries, data, radius, sort: bool = False, max_total: int = 0, device: int = 0):
        """Every object within cosine distance `radius` (a number, or one per query) of each query, by brute force (`lmi_knn_range`
        on unit rows, like `search`): (lims i64[nq + 1], dists f32[total], ids 1-based [total], seconds); query q owns
        [lims[q], lims[q + 1]), in ascending id order, or nearest first with `sort=True` (sorted on the device)."""
        t0 = time.time()
        with _capi.range_knn(_unit(queries), _unit(data), radius, metric="ip", max_total=max_total, device=device) as res:
            if sort:
                index = _capi.Index(device)   # provides the stream of the sort only
                try:
                    res.sort(index)
                finally:
                    index.close()
            dists, rows = res.read()
            return res.lims, dists, rows.astype(np.int64) + 1, time.time() - t0
