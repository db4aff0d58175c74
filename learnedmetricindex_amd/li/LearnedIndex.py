"""LearnedIndex.search on the MI355X (reference: li/LearnedIndex.py:22-373).

Drop-in for the reference class: same constructor, same `search(...)` signature and return
values `(dists f64[nq,k], nns u32[nq,k], measured_time)`.  What changes underneath:

* the index lives in HBM: on the first `search` (or an explicit `prepare`) the scan vectors are
  uploaded once into a bucket-contiguous, fragment-major slab together with the 1-based labels
  (the reference instead re-groups the DataFrame and copies every visited bucket on every rank
  of every call, LearnedIndex.py:350-357);
* one `lmi_search` call does MLP forward -> top-n_buckets -> routing -> bucket scan -> merge on the
  GPU (LearnedIndex.py:87-146 + 163-214 + 328-373);
* multi-level indexes (`len(n_categories) > 1`): the batched priority-queue walk of the reference
  (LearnedIndex.py:216-325, PriorityQueue.py) runs on the device (`lmi_nav_order`): per step every
  unfinished query pops its most probable node (priority = the child's local softmax probability), the
  queries that popped the same internal node are evaluated by that node's model in one grouped launch of
  the fused MLP kernel and its children are pushed; then ONE lmi_scan_topk call scans the buckets of
  all ranks;
* `data_navigation` is never mutated (the reference adds/drops `category_L*` columns,
  :101-104/:153-157), so passing the same frame for navigation and scan works.

Reference quirks kept on purpose: ids are the DataFrame's index labels as uint32, unvisited slots
are (inf, 0) (Q2); the per-bucket k is always 10 and a single-bucket search returns 10 columns
whatever `k` is (Q3); buckets with < 10 objects are padded like faiss does (Q4); dist = 1 - ip in
float32 stored as float64 (Q5/Q6).
"""
import functools
import inspect
import time
from collections import defaultdict
from logging import INFO
from typing import Dict, List, Optional, Tuple

import numpy as np
import numpy.typing as npt
import pandas as pd

from .Logger import Logger
from .model import NeuralNetwork, data_X_to_torch, linear_layers
from .PriorityQueue import EMPTY_VALUE
from .utils import log_runtime

try:
    from .. import _capi
except ImportError:  # pragma: no cover
    import _capi  # type: ignore

np.random.seed(2023)


def _feature_columns(df: pd.DataFrame) -> list:
    return [c for c in df.columns if not (isinstance(c, str) and c.startswith("category_L"))]


class _Hasher:
    """Streamed 64-bit content hash: xxh3 when the wheel is there (~10 GB/s), zlib.crc32 + adler32 otherwise."""

    def __init__(self):
        try:
            import xxhash   # optional (requirements.txt): ~10 GB/s; without it the zlib pair below, ~10x slower
            self._h, self._z = xxhash.xxh3_64(), None
        except ImportError:
            self._h, self._z = None, [0, 1]

    def update(self, a) -> None:
        a = np.ascontiguousarray(a)   # logical (row-major) element order, whatever the array's memory layout
        buf = memoryview(a.reshape(-1).view(np.uint8)) if a.size else b""
        if self._h is not None:
            self._h.update(buf)
        else:
            import zlib
            self._z = [zlib.crc32(buf, self._z[0]), zlib.adler32(buf, self._z[1])]

    def digest(self) -> int:
        return self._h.intdigest() if self._h is not None else (self._z[0] << 32) | self._z[1]


def _array_fingerprint(a) -> int:
    h = _Hasher()
    h.update(a)
    return h.digest()


def _scan_dtype(df: pd.DataFrame, cols: list):
    """np.float16 when every feature column of the scan frame is float16 -- data distributed as halves, which the library
    takes as it is (`lmi_buckets_add_rows_f16`: no host widening, half the upload) -- else np.float32."""
    return np.float16 if len(cols) and all(df[c].dtype == np.float16 for c in cols) else np.float32


def _query_array(a):
    """C-contiguous float16 (kept: uploaded as halves) or float32 (everything else) view of a query array."""
    return np.ascontiguousarray(a, dtype=np.float16 if getattr(a, "dtype", None) == np.float16 else np.float32)


def _frame_bytes(df: pd.DataFrame) -> int:
    return int(df.shape[0]) * int(df.shape[1]) * 4


def _frame_fingerprint(df: pd.DataFrame, full: bool) -> int:
    """Hash of the frame's values: every byte (`full`: blocks of the frame as they lie in memory, no copy for a single-dtype
    frame) or 4 096 evenly spaced whole rows."""
    h = _Hasher()
    if not full:
        rows = np.unique(np.linspace(0, max(0, df.shape[0] - 1), num=min(4096, max(1, df.shape[0])), dtype=np.int64))
        h.update(df.iloc[rows].to_numpy() if df.shape[0] else np.empty(0))
        return h.digest()
    # rows in order, every row's columns in order -- independent of how pandas lays the frame out.  A single-dtype frame made
    # from a row-major array (the usual case) is one block whose transposed values ARE that array: hashed in place, no copy;
    # any other layout is hashed through row-chunk copies.
    vals = None
    try:
        blocks = list(df._mgr.blocks)
        if len(blocks) == 1 and blocks[0].values.ndim == 2 and blocks[0].values.T.flags.c_contiguous \
                and np.array_equal(np.asarray(blocks[0].mgr_locs.as_array), np.arange(df.shape[1])):
            vals = blocks[0].values.T
    except Exception:  # noqa: BLE001  (pandas internals: best effort)
        vals = None
    if vals is not None:
        h.update(vals)
    else:
        step = max(1, (64 << 20) // max(1, 8 * df.shape[1]))
        for r0 in range(0, df.shape[0], step):
            h.update(df.iloc[r0: r0 + step].to_numpy())
    h.update(np.asarray([str(c) for c in df.columns]).astype("U"))
    return h.digest()


class LearnedIndex(Logger):
    _WORKSPACE_BYTES = 6 << 30  # per-call device workspace budget of one search chunk
    _NAV_QUEUE_BYTES = 4 << 30  # multi-level walk: per-query priority queues hold one 8-byte entry per child of every node
                                # (12 bytes with the path-mass stop on; lmi_nav_order refuses 2^31 entries); larger batches
                                # are walked in query chunks

    def __init__(self, root_model: NeuralNetwork, internal_models: Dict[Tuple, NeuralNetwork],
                 bucket_paths: List[Tuple]):
        self.root_model = root_model
        """The root model of the index."""
        self.internal_models = internal_models
        """path (padded with EMPTY_VALUE) -> internal model."""
        self.bucket_paths = bucket_paths
        """List of paths to the buckets."""
        self._engine = None
        self._engine_key = None
        self._path_ids = None
        self._entry_paths = None
        self._nav_cap = 0

    def __getstate__(self):  # picklable like the reference object (search.py:234-241)
        state = dict(self.__dict__)
        state["_engine"] = None
        state["_engine_key"] = None
        state["_path_ids"] = None
        state["_entry_paths"] = None
        state.pop("_fp_memo", None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("_engine", None)
        self.__dict__.setdefault("_engine_key", None)
        self.__dict__.setdefault("_path_ids", None)
        self.__dict__.setdefault("_entry_paths", None)
        self.__dict__.setdefault("_nav_cap", 0)

    # ------------------------------------------------------------------------------------------
    def invalidate(self) -> None:
        """Drops the HBM-resident copy: the next `search`/`prepare` uploads the frames again (call after editing
        the vectors in place beyond what the sampled fingerprint can see)."""
        self.close()

    def close(self) -> None:
        """Frees the HBM-resident index."""
        if self._engine is not None:
            cover = getattr(self._engine, "_li_cover", None)   # the cover range_search_exact keeps with the engine
            if cover is not None:
                cover.close()
            self._engine.close()
        self._engine = None
        self._engine_key = None

    #: "auto": full-content fingerprint of the scan frame for frames up to _STRICT_BYTES, a row sample above; True: always full;
    #: False: always the sample (an in-place edit of unsampled rows is then only caught by `invalidate()`);
    #: "memo": the full fingerprint once per (frame object, shape, address of its values), later calls with the same triple re-check a
    #: 4 096-row sample only -- for callers that search the same frames again and again (the full hash costs ~0.1 s per GB and call,
    #: 10-100x the GPU search itself); an in-place edit of unsampled rows of the SAME buffer is then only caught by `invalidate()`
    strict_cache = "auto"
    _STRICT_BYTES = 1 << 30

    def prepare(self, data_navigation: pd.DataFrame, data_search: pd.DataFrame,
                data_prediction: npt.NDArray[np.int64], n_categories: List[int], device: int = 0, metric: str = "ip",
                assume_unchanged: bool = False, storage: str = "f32"):
        """Uploads the scan vectors bucket-contiguously (the one-time replacement of the
        reference's per-call groupby + `.loc` gather).  Called by `search` when needed.
        `storage` (an extension; `lmi_set_storage`): "f32" (default) or "f16" -- the resident copy keeps the fp16 fragments
        only, a third of the device memory, for scan vectors that are binary16-exact (`_capi.f16_admissible`); the library
        checks that on the device and its refusal surfaces as `_capi.LmiError`.  Same results bit for bit."""
        assert self.root_model is not None, "Model is not trained, call `build` first."
        dp = np.asarray(data_prediction)
        if dp.ndim == 1:
            dp = dp[:, None]
        assert dp.shape[0] == data_navigation.shape[0] == data_search.shape[0]
        # What the resident copy was built from.  The reference re-reads both frames on every call (LearnedIndex.py:350-357), so a
        # drop-in must never answer from a slab the caller has since edited: the key is a CONTENT fingerprint -- a streamed 64-bit
        # hash of every byte of the scan vectors, of the labels, of the placement and of every model's weights -- and not the
        # frames' identity: an equal-content frame built afresh (`df[cols]`, `.copy()`) hits the cache, an in-place edit of any row
        # misses it.  Hashing costs ~0.1 s per GB and call; frames above `_STRICT_BYTES` (1 GiB) are fingerprinted by a row sample
        # instead unless `strict_cache` is True, and `assume_unchanged=True` skips the vectors' fingerprint altogether (the caller
        # then vouches that the frames are the ones the resident index was built from; `invalidate()` drops it).
        full = self.strict_cache is True or (self.strict_cache == "auto" and _frame_bytes(data_search) <= self._STRICT_BYTES)
        if assume_unchanged and self._engine is not None:
            content = self._engine_key[0] if self._engine_key else None
        elif self.strict_cache == "memo":
            try:
                addr = int(data_search._mgr.blocks[0].values.__array_interface__["data"][0])
            except Exception:  # noqa: BLE001  (pandas internals: best effort)
                addr = None
            who = (id(data_search), tuple(data_search.shape), addr)
            sample = _frame_fingerprint(data_search, False)
            memo = getattr(self, "_fp_memo", None)
            if addr is not None and memo is not None and memo[0] == who and memo[1] == sample:
                content = memo[2]
            else:
                content = _frame_fingerprint(data_search, True)
                self._fp_memo = (who, sample, content)
        else:
            content = _frame_fingerprint(data_search, full)
        w_h = _Hasher()
        for net in [self.root_model] + list(self.internal_models.values()):
            for W, b in linear_layers(net.model):
                w_h.update(W)
                w_h.update(b)
        key = (content, tuple(data_search.shape), _array_fingerprint(data_navigation.index.to_numpy()), dp.shape, _array_fingerprint(dp),
               w_h.digest(), tuple(tuple(int(v) for v in p) for p in self.internal_models), tuple(n_categories), device, metric, storage)
        if self._engine is not None and key == self._engine_key:
            return self._engine
        self.close()
        n_levels = len(n_categories)
        assert dp.shape[1] == n_levels
        eng = _capi.Index(device, metric=metric, storage=storage)
        try:
            self._build_engine(eng, dp, n_levels, n_categories, data_navigation, data_search)
        except BaseException:
            eng.close()   # (a refused build -- storage="f16" on data that is not binary16-exact -- leaves nothing resident)
            raise
        self._engine, self._engine_key = eng, key
        return eng

    def _build_engine(self, eng, dp, n_levels, n_categories, data_navigation, data_search) -> None:
        if n_levels == 1:
            # bucket id == class id: lmi_search can run MLP -> scan without leaving the device
            eng.set_mlp(linear_layers(self.root_model.model))
            assert eng.n_classes >= int(dp[:, 0].max(initial=0)) + 1, "data_prediction outside the model's classes"
            bucket_of = dp[:, 0]
            n_bucket_ids = max(int(n_categories[0]), eng.n_classes)
            self._path_ids = None
        else:
            # a bucket is a distinct path; ids follow the sorted order pandas groupby yields (:343-350)
            paths, bucket_of = np.unique(dp, axis=0, return_inverse=True)
            bucket_of = np.asarray(bucket_of).reshape(-1)
            n_bucket_ids = paths.shape[0]
            self._path_ids = {tuple(int(v) for v in p): i for i, p in enumerate(paths)}
            self._upload_tree(eng, n_levels)
        labels = data_navigation.index.to_numpy()
        assert labels.min(initial=0) >= 0 and labels.max(initial=0) < 2 ** 32, "ids must fit uint32"
        cols = _feature_columns(data_search)
        if data_search.index.equals(data_navigation.index):
            frame = data_search
        else:  # the reference fetches scan rows by label: data_search.loc[g.index] (:357)
            frame = data_search.loc[data_navigation.index]
        eng.buckets_begin(bucket_of, len(cols), n_bucket_ids, ids=labels.astype(np.uint32))
        piece = max(1, (256 << 20) // (4 * max(1, len(cols))))
        dtype = _scan_dtype(frame, cols)   # a float16 frame is passed on as halves, block by block
        for r0 in range(0, frame.shape[0], piece):
            block = frame.iloc[r0: r0 + piece]
            eng.add_rows(np.ascontiguousarray(block[cols].to_numpy(dtype=dtype)), r0)
        eng.buckets_end()

    def search_resident(self, queries_navigation, queries_search, n_categories: List[int], n_buckets: int = 1,
                        k: int = 10, stop_mass: Optional[float] = None, path_mass: Optional[float] = None,
                        stop_rows: Optional[int] = None, merge: str = "ranks", filter=None, filter_of=None):
        """`search` against the index already resident in HBM (after `prepare`, a previous `search`
        or `index_io.load_index`): no DataFrames needed.  Same return values as `search`; `stop_mass`, `path_mass`, `stop_rows`,
        `merge`, `filter` and `filter_of` as there."""
        self._check_merge(merge)
        self._check_filter(filter, filter_of, merge)
        self._check_stop_mass(stop_mass, n_categories)
        self._check_path_mass(path_mass, n_categories)
        assert self._engine is not None, "no resident index: call prepare()/search() or index_io.load_index()"
        return self._search_with(self._engine, queries_navigation, queries_search, n_categories, n_buckets, k,
                                 time.time(), stop_mass, path_mass, stop_rows, merge, filter, filter_of)

    # ---- stored objects by id (an extension; the resident counterpart of the reference's `data_search.loc[ids]`, :357) ----
    @staticmethod
    def _missing(who: str, ids, found) -> KeyError:
        """What `DataFrame.loc` would raise for labels it does not hold: the absent ids, ten at most."""
        gone = np.unique(np.asarray(ids).reshape(-1)[~found])
        more = f" and {gone.size - 10} more" if gone.size > 10 else ""
        return KeyError(f"{who}: {[int(v) for v in gone[:10]]}{more} not in the index")

    def reconstruct(self, ids, dtype=np.float32, missing: str = "raise"):
        """The scan vectors of the objects with these ids (DataFrame index labels), [n, d], read back from the index resident in HBM
        (after `prepare`, a `search` or `index_io.load_index`; `Index.fetch`): no DataFrame needed, and exactly the stored values
        also for `storage="f16"`.  `ids` in any order, repeats allowed.  `dtype`: np.float32 or np.float16 (an f32 index whose
        values are not binary16-exact raises `_capi.LmiError`).  `missing`: "raise" (default) raises KeyError naming up to ten ids
        no object carries, as `DataFrame.loc` would; "zero" returns (rows, found bool [n]) with zero rows for them."""
        if missing not in ("raise", "zero"):
            raise ValueError(f"missing {missing!r} unknown: 'raise' or 'zero'")
        eng = self._resident("reconstruct")
        rows, bucket, _ = eng.fetch(ids, dtype=dtype, where=True)
        found = bucket >= 0
        if missing == "zero":
            return rows, found
        if not found.all():
            raise self._missing("reconstruct", ids, found)
        return rows

    @staticmethod
    def _torch_device(eng):
        import torch

        return torch.device("cuda", eng.device)

    def search_like(self, ids, n_categories: List[int], n_buckets: int = 1, k: int = 10, queries_navigation=None, **kw):
        """Query by stored object: `search_resident` with the scan vectors of the objects `ids` as queries -- "more like this".  The
        vectors are fetched into a device tensor (`Index.fetch_device`) and handed to the engine's device calls as they lie: no
        host copy of them exists.  Returns what `search_resident(V, V, ..)` with V = `reconstruct(ids)` returns, bit for bit; `**kw`
        (`stop_mass`, `path_mass`, `stop_rows`, `merge`, `filter`, `filter_of`) as there.  The index holds scan vectors only: where
        the root model's input width differs from the scan width `queries_navigation` [n, d_nav] is required (ValueError
        otherwise); where it is the same the fetched vectors navigate too unless `queries_navigation` is given.  KeyError for an
        id no object carries."""
        import torch

        eng = self._resident("search_like")
        ids_a, _ = _capi.fetch_args("search_like", eng, ids, np.float32)
        n = int(ids_a.shape[0])
        if queries_navigation is None and eng.d_nav != eng.d:
            raise ValueError(f"search_like: the root model takes {eng.d_nav} inputs, the index stores vectors of {eng.d}: it holds no "
                             "navigation vectors, pass queries_navigation")
        unknown = sorted(set(kw) - {"stop_mass", "path_mass", "stop_rows", "merge", "filter", "filter_of"})
        if unknown:
            raise TypeError(f"search_like: unexpected keyword {unknown[0]!r}")
        merge = kw.get("merge", "ranks")
        self._check_merge(merge)
        self._check_filter(kw.get("filter"), kw.get("filter_of"), merge)
        self._check_stop_mass(kw.get("stop_mass"), n_categories)
        self._check_path_mass(kw.get("path_mass"), n_categories)
        qn = None
        if queries_navigation is not None:
            qn = np.ascontiguousarray(_query_array(queries_navigation), dtype=np.float32)
            if qn.ndim != 2 or qn.shape[0] != n:
                raise ValueError(f"search_like: queries_navigation must be [{n}, d_nav], not {tuple(qn.shape)}")
        dev = self._torch_device(eng)
        ids_t = torch.from_numpy(ids_a.view(np.int32)).to(dev)
        rows_t = torch.empty((n, eng.d), dtype=torch.float32, device=dev)
        bucket_t = torch.empty((n,), dtype=torch.int32, device=dev)
        eng.fetch_device(ids_t, rows_t, bucket_t)
        found = bucket_t.cpu().numpy() >= 0 if n else np.ones(0, dtype=bool)
        if not found.all():
            raise self._missing("search_like", ids_a, found)
        qn_t = rows_t if qn is None else torch.from_numpy(qn).to(dev)
        return self._search_with(eng, qn_t, rows_t, n_categories, n_buckets, k, time.time(), kw.get("stop_mass"), kw.get("path_mass"),
                                 kw.get("stop_rows"), merge, kw.get("filter"), kw.get("filter_of"), on_device=True)

    MERGES = ("ranks", "union")

    @classmethod
    def _check_merge(cls, merge) -> None:
        if merge not in cls.MERGES:
            raise ValueError(f"merge {merge!r} unknown: 'ranks' (at most 10 results per visited bucket, merged by rank; the reference) "
                             "or 'union' (the k best objects of all visited buckets)")

    @staticmethod
    def _check_filter(filter, filter_of, merge) -> None:
        """A filter restricts the candidates of the union scan: the rank merge has no filtered form.  Refused before any work is
        done."""
        if filter is None and filter_of is not None:
            raise ValueError("filter_of without a filter")
        if filter is not None and merge != "union":
            raise ValueError("a filter needs merge='union' (the rank merge has no filtered form)")

    @staticmethod
    def _check_stop_mass(stop_mass, n_categories) -> None:
        """`stop_mass` is defined on the root model's probabilities of a 1-level index; the multi-level walk ranks by local
        probabilities, so it is refused there before any work is done."""
        if stop_mass is not None and len(n_categories) > 1:
            raise ValueError("stop_mass is not supported on a multi-level index (the walk ranks buckets by local probabilities)")

    @staticmethod
    def _check_path_mass(path_mass, n_categories) -> None:
        """`path_mass` is the stop of the multi-level walk; a 1-level index has `stop_mass` for the same purpose.  Refused
        before any work is done."""
        if path_mass is not None and len(n_categories) == 1:
            raise ValueError("path_mass is the stop of the multi-level walk; on a 1-level index use stop_mass")

    # ------------------------------------------------------------------------------------------
    def insert(self, data_navigation_new: pd.DataFrame, data_search_new: Optional[pd.DataFrame] = None,
               ids=None, create_buckets: bool = False) -> npt.NDArray[np.int64]:
        """Adds objects to the HBM-resident index (an extension: the reference rebuilds).  Each object is placed the way
        `LearnedIndexBuilder.build` places it -- argmax of the root model, then argmax of each internal node's model down the
        tree, through the HIP MLP -- and goes after the last object of its bucket (`lmi_buckets_insert`; refused by the library,
        `_capi.LmiError`, on a `storage="f16"` index, which cannot be changed in place yet: `extended` returns a new index
        instead).  `data_search_new`
        (default: `data_navigation_new`) holds the scan vectors, `ids` (default: `data_navigation_new.index`) the labels.
        Returns the objects' `data_prediction` rows (int64 [n, n_levels]) for the caller to append to their own frames.
        A multi-level placement onto a leaf path that holds no bucket would need a new bucket: the whole call is refused
        with ValueError before anything changes -- unless `create_buckets=True`: then the missing leaf paths are opened first
        as empty buckets (a `regroup` that names no object: the resident engine is replaced by the re-bucketed one and closed,
        the paths join `bucket_paths`) and the insert goes on as usual.  Afterwards `search_resident` answers from the mutated
        index; `search` keeps answering from the frames it is given (they no longer match the resident copy, which it rebuilds)."""
        eng = self._resident("insert")
        dp, bucket_of, rows, labels = self._place(data_navigation_new, data_search_new, ids, create_buckets)
        eng = self._engine   # (create_buckets may have replaced it)
        eng.insert(rows, bucket_of, labels)
        self._engine_key = self._mutated_key()
        return dp

    def _place(self, data_navigation_new, data_search_new, ids, create_buckets: bool = False):
        """What `insert` and `extended` share: the new objects' `data_prediction` rows (int64 [n, n_levels]; argmax of the root
        model, then of each internal node's model down the tree), their bucket ids in the resident engine, their scan vectors
        (float16 frames stay halves) and their ids (uint32).  A placement onto a leaf path that holds no bucket raises ValueError
        before anything changes -- unless `create_buckets`, which opens the missing paths first (`_open_buckets`)."""
        nav = data_navigation_new
        srch = nav if data_search_new is None else data_search_new
        labels = nav.index.to_numpy() if ids is None else np.asarray(ids).reshape(-1)
        assert labels.shape[0] == nav.shape[0], "one id per object"
        assert labels.min(initial=0) >= 0 and labels.max(initial=0) < 2 ** 32, "ids must fit uint32"
        x_nav = np.ascontiguousarray(nav[_feature_columns(nav)].to_numpy(dtype=np.float32))
        n_levels = 1 if self._path_ids is None else len(next(iter(self._path_ids)))
        dp = np.full((nav.shape[0], n_levels), EMPTY_VALUE, dtype=np.int64)
        if nav.shape[0]:
            dp[:, 0] = self.root_model.predict(x_nav)
        for level in range(1, n_levels):   # every node's objects by its own model (LearnedIndexBuilder.build)
            prefixes, which = np.unique(dp[:, :level], axis=0, return_inverse=True)
            which = np.asarray(which).reshape(-1)
            for j, prefix in enumerate(prefixes):
                net = self.internal_models.get(tuple(int(v) for v in prefix) + (EMPTY_VALUE,) * (n_levels - level))
                if net is not None and (prefix != EMPTY_VALUE).all():
                    sel = np.flatnonzero(which == j)
                    dp[sel, level] = net.predict(x_nav[sel])
        if n_levels == 1:
            bucket_of = dp[:, 0]
        else:
            bucket_of = np.asarray([self._path_ids.get(tuple(int(v) for v in p), -1) for p in dp], dtype=np.int64)
            missing = int((bucket_of < 0).sum())
            if missing and create_buckets:
                self._open_buckets(np.unique(dp[bucket_of < 0], axis=0))
                bucket_of = np.asarray([self._path_ids[tuple(int(v) for v in p)] for p in dp], dtype=np.int64)
            elif missing:
                raise ValueError(f"{missing} of {dp.shape[0]} object(s) fall on a leaf path that holds no bucket; creating buckets "
                                 "is not supported (rebuild the index): nothing was inserted")
        cols = _feature_columns(srch)
        frame = srch if srch.index.equals(nav.index) else srch.loc[nav.index]
        rows = np.ascontiguousarray(frame[cols].to_numpy(dtype=_scan_dtype(frame, cols)))
        return dp, bucket_of, rows, labels.astype(np.uint32)

    def _derived_like(self, engine) -> "LearnedIndex":
        """A new `LearnedIndex` over this object's models and bucket paths that answers from `engine` (an index derived from the
        resident one without a change of partition: `subset`, `concat`)."""
        other = LearnedIndex(self.root_model, self.internal_models, self.bucket_paths)
        other._engine, other._engine_key = engine, self._mutated_key()
        other._path_ids, other._entry_paths, other._nav_cap = self._path_ids, self._entry_paths, self._nav_cap
        return other

    def concat(self, *others: "LearnedIndex") -> "LearnedIndex":
        """A new `LearnedIndex` over this object's models and bucket paths whose HBM-resident index holds this one's resident
        objects followed by every one of `others`' (an extension; `lmi_concat`): bucket by bucket this index's objects, then
        `others[0]`'s, and so on -- laid out like a fresh build of that list.  Every other must be resident and have this object's
        `bucket_paths` (a bucket id must mean the same path in every part): anything else is refused with ValueError before any
        device work.  The copy is derived on the device, is independent of every part, is answered by `search_resident` /
        `range_search_resident` and saves and loads through `index_io` like any derived index.  Works on `storage="f16"`.  The
        parts are unchanged."""
        eng = self._resident("concat")
        mine = [tuple(int(v) for v in p) for p in self.bucket_paths]
        engines = []
        for t, o in enumerate(others):
            if not isinstance(o, LearnedIndex):
                raise ValueError(f"concat: argument {t} must be a LearnedIndex, not {type(o).__name__}")
            if o._engine is None:
                raise ValueError(f"concat: argument {t} has no resident index: call prepare()/search() or index_io.load_index()")
            if [tuple(int(v) for v in p) for p in o.bucket_paths] != mine or o._path_ids != self._path_ids:
                raise ValueError(f"concat: argument {t} has other bucket_paths than this index: its bucket ids do not mean the same "
                                 "paths (parts with different partitions are not concatenated; regroup one of them first)")
            engines.append(o._engine)
        return self._derived_like(eng.concat(*engines))

    def extended(self, data_navigation_new: pd.DataFrame, data_search_new: Optional[pd.DataFrame] = None, ids=None):
        """`insert`'s counterpart that returns a NEW index and works on `storage="f16"` (an extension; `lmi_concat`): the objects
        are placed exactly as `insert` places them, built into a small index in the resident engine's storage and metric (a
        `float16` frame goes up as halves), and the result is the resident index followed, bucket by bucket, by the new objects --
        what `insert` leaves behind where `insert` works.  Returns `(new LearnedIndex, data_prediction)`; this object is
        unchanged and the small index is closed, also when the concatenation is refused (`_capi.LmiError`: on `storage="f16"`, new
        values so large that the result's scale pushes a stored half below the binary16 subnormals -- as a fresh build of all the
        rows would be refused).  A placement onto a leaf path that holds no bucket is refused with ValueError, as in `insert`
        without `create_buckets`."""
        eng = self._resident("extended")
        dp, bucket_of, rows, labels = self._place(data_navigation_new, data_search_new, ids)
        small = _capi.Index(eng.device, metric=eng.metric, storage=eng.storage)
        try:
            small.set_buckets(rows, bucket_of, eng.L, ids=labels)
            new = eng.concat(small)
        finally:
            small.close()
        return self._derived_like(new), dp

    def delete(self, ids) -> int:
        """Removes every object whose id (DataFrame index label) is in `ids` from the HBM-resident index (an extension;
        `lmi_buckets_delete`; refused by the library on a `storage="f16"` index); the others keep their order.  Returns how many
        were removed.  Afterwards `search_resident`
        answers from the mutated index; `search` keeps answering from the frames it is given."""
        eng = self._resident("delete")
        n = eng.delete(np.asarray(ids).reshape(-1).astype(np.uint32))
        self._engine_key = self._mutated_key()
        return n

    def subset(self, ids, drop: bool = False) -> "LearnedIndex":
        """A new `LearnedIndex` over the same models and bucket paths whose HBM-resident index holds only the objects whose id
        (DataFrame index label) is in `ids` -- or, with `drop=True`, all but those (an extension; `lmi_subset`).  The copy is
        derived on the device, is independent of this object's resident index (either may be closed or mutated), and is laid
        out like a fresh build of the kept objects; it is answered by `search_resident`.  Unlike `delete` it works on a
        `storage="f16"` index.  Ids not present are ignored; this object is unchanged."""
        eng = self._resident("subset")
        return self._derived_like(eng.subset(np.asarray(ids).reshape(-1), drop=drop))

    def regroup(self, ids, data_prediction, root_model: Optional[NeuralNetwork] = None,
                internal_models: Optional[Dict[Tuple, NeuralNetwork]] = None,
                bucket_paths: Optional[List[Tuple]] = None) -> "LearnedIndex":
        """A new `LearnedIndex` over the SAME resident objects under a new partition (an extension; `lmi_regroup`): the object
        whose id (DataFrame index label) is `ids[i]` takes the path `data_prediction[i]` (int64 [n, n_levels_new], n_levels_new >=
        the current depth); every other object keeps its path, padded with EMPTY_VALUE where the tree got deeper.  `root_model`,
        `internal_models` and `bucket_paths` default to this object's; pass what the new partition changes (a split's child model,
        a retrained root).  The copy is derived on the device -- no DataFrame is needed, nothing is uploaded again -- is independent
        of this object's resident index, is laid out like a fresh build of the same objects in the order held here, and is answered
        by `search_resident` / `range_search_resident`; it saves and loads through `index_io` like any mutated index.  This object
        is unchanged.
        Bucket ids: on a 1-level index bucket id == class id and the new index has as many buckets as the (new) root model has
        classes.  Otherwise the buckets are the distinct paths among this index's bucket paths and the rows of `data_prediction`,
        numbered in sorted order as a build numbers them; a path left without objects stays, as an empty bucket.
        When to split or merge, with which clustering and how many epochs is the caller's policy: INTEGRATION.md has the recipe."""
        other = LearnedIndex(self.root_model if root_model is None else root_model,
                             self.internal_models if internal_models is None else internal_models,
                             self.bucket_paths if bucket_paths is None else bucket_paths)
        self._regroup_into(other, ids, data_prediction)
        return other

    def _current_paths(self, eng) -> npt.NDArray[np.int64]:
        """[L, depth]: the path of every bucket id of the resident engine."""
        if self._path_ids is None:
            return np.arange(eng.L, dtype=np.int64)[:, None]
        return np.asarray([p for p, _ in sorted(self._path_ids.items(), key=lambda kv: kv[1])], dtype=np.int64).reshape(eng.L, -1)

    def _regroup_into(self, other: "LearnedIndex", ids, data_prediction, extra_paths=None) -> None:
        """`regroup` into `other` (which holds the new models and bucket paths): the new path set, its sorted ids, the old id -> new
        id shift as the engine's `bucket_map`, the named objects' labels; then the new engine's models and tree.  `extra_paths`
        [m, n_levels]: paths that become buckets although no object is placed there (`insert(create_buckets=True)`)."""
        eng = self._resident("regroup")
        ids = np.asarray(ids).reshape(-1)
        old = self._current_paths(eng)
        dp = np.asarray(data_prediction, dtype=np.int64)
        if dp.ndim == 1:
            dp = dp[:, None] if dp.size else dp.reshape(0, old.shape[1])
        if dp.ndim != 2 or dp.shape[0] != ids.shape[0]:
            raise ValueError(f"regroup: data_prediction {tuple(dp.shape)} must hold one path per id ({ids.shape[0]})")
        n_levels = dp.shape[1]
        if n_levels < old.shape[1]:
            raise ValueError(f"regroup: data_prediction has {n_levels} level(s), the index has {old.shape[1]}")
        if n_levels == 1 and self._path_ids is None:
            # bucket id == class id; a bucket past the new model's classes has to be emptied by the list
            L_new = int(linear_layers(other.root_model.model)[-1][0].shape[0])
            bucket_map = None if L_new >= eng.L else np.where(np.arange(eng.L) < L_new, np.arange(eng.L), -1).astype(np.int32)
            new = eng.regroup(ids, dp[:, 0], L_new, bucket_map)
            try:
                new.set_mlp(linear_layers(other.root_model.model))
            except BaseException:
                new.close()
                raise
            other._path_ids = None
        else:
            padded = np.full((old.shape[0], n_levels), EMPTY_VALUE, dtype=np.int64)
            padded[:, : old.shape[1]] = old
            stack = [padded, dp] + ([] if extra_paths is None else [np.asarray(extra_paths, dtype=np.int64).reshape(-1, n_levels)])
            paths, inv = np.unique(np.concatenate(stack), axis=0, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            L = old.shape[0]
            new = eng.regroup(ids, inv[L: L + dp.shape[0]], int(paths.shape[0]), inv[:L].astype(np.int32))
            other._path_ids = {tuple(int(v) for v in p): i for i, p in enumerate(paths)}
            try:
                other._upload_tree(new, n_levels)
            except BaseException:
                new.close()
                raise
        other._engine, other._engine_key = new, self._mutated_key()

    def _open_buckets(self, missing_paths):
        """`insert(create_buckets=True)`: the resident engine re-bucketed with `missing_paths` as empty buckets; this object now
        answers from the new engine, the old one is closed.  Returns the new engine."""
        known = {tuple(int(v) for v in p) for p in self.bucket_paths}
        more = [tuple(int(v) for v in p) for p in missing_paths]
        other = LearnedIndex(self.root_model, self.internal_models, list(self.bucket_paths) + [p for p in more if p not in known])
        self._regroup_into(other, [], np.empty((0, missing_paths.shape[1]), dtype=np.int64), extra_paths=missing_paths)
        old = self._engine
        self.bucket_paths = other.bucket_paths
        self._engine, self._engine_key = other._engine, other._engine_key
        self._path_ids, self._entry_paths, self._nav_cap = other._path_ids, other._entry_paths, other._nav_cap
        other._engine = None
        old.close()
        return self._engine

    def _resident(self, what: str):
        assert self._engine is not None, f"{what}: no resident index: call prepare()/search() or index_io.load_index()"
        return self._engine

    @staticmethod
    def _mutated_key():
        """An `_engine_key` no `prepare` key equals: the resident index no longer holds what any frames it was built from
        hold, so a later `search(frames)` must not be answered from it."""
        return ("mutated", object())

    def search(
        self,
        data_navigation: pd.DataFrame,
        queries_navigation: npt.NDArray[np.float32],
        data_search: pd.DataFrame,
        queries_search: npt.NDArray[np.float32],
        data_prediction: npt.NDArray[np.int64],
        n_categories: List[int],
        n_buckets: int = 1,
        k: int = 10,
        metric: str = "ip",
        assume_unchanged: bool = False,
        stop_mass: Optional[float] = None,
        path_mass: Optional[float] = None,
        storage: str = "f32",
        stop_rows: Optional[int] = None,
        merge: str = "ranks",
        filter=None,
        filter_of=None,
    ) -> Tuple[npt.NDArray, npt.NDArray[np.uint32], Dict[str, float]]:
        """Searches for `k` nearest neighbors of every query in its `n_buckets` most probable buckets.
        Parameters and return values as the reference (LearnedIndex.py:41-83).  `metric` (an extension; the
        reference scans with `1 - inner product` only): "ip" (default) or "l2" -- squared Euclidean distances.
        `assume_unchanged` (an extension): the caller vouches that `data_search` still holds what the HBM-resident copy was
        built from, so its bytes are not fingerprinted again (see `prepare`); the default re-checks them on every call.
        `stop_mass` (an extension, 1-level indexes only; `lmi_set_stop_mass`): None = off; 0 < stop_mass <= 1: a query stops
        visiting buckets once the probabilities of the ranks it has visited sum to `stop_mass` or more -- the ranks it skips
        stay unvisited, the result shapes do not change.  It holds for this call only.  ValueError on a multi-level index.
        `path_mass` (an extension, multi-level indexes only; `lmi_set_path_mass`): None = off; 0 < path_mass <= 1: the walk keeps
        its order, and a query stops once the path probabilities (the product of the local probabilities along a bucket's path)
        of the buckets it has recorded sum to `path_mass` or more -- the slots behind the stop stay unvisited, the result shapes
        do not change.  It holds for this call only.  ValueError on a 1-level index (use `stop_mass` there).
        `stop_rows` (an extension, 1-level and multi-level indexes alike; `lmi_set_stop_rows`): None = off; an integer >= 1: a
        query stops visiting buckets once the buckets it has visited hold `stop_rows` objects or more (the bucket that crosses
        the budget is scanned whole) -- the slots behind the stop stay unvisited, the result shapes do not change.  With
        `stop_mass` / `path_mass` as well a query goes on only while both allow it.  It holds for this call only.
        `storage` (an extension): "f32" (default) or "f16", how the HBM-resident copy keeps the scan vectors (see `prepare`).
        `merge` (an extension): "ranks" (default) is the reference: at most 10 results per visited bucket, merged rank by rank,
        k <= 20 for n_buckets >= 2.  "union" returns the `k` best objects of the union of the visited buckets (`lmi_search_union` /
        `lmi_search_tree_union`): k up to 1024, results [nq, k] for any n_buckets; a query whose buckets hold fewer than k objects
        is padded with dist = +inf, id = 0.  The stops compose with it.  It needs the default storage ("f32", prefilter on).
        ValueError for anything else.
        `filter` (an extension, with merge="union" only; `lmi_search_union_filtered` / `lmi_search_tree_union_filtered`): None = off;
        a list of ids (DataFrame index labels): only those objects may be returned; or a `_capi.Filter` made on the resident engine
        (several filters, keep or drop), with `filter_of` [nq] naming each query's filter (-1 = unfiltered; None = all use filter 0).
        The filter acts on the scan, not on the routing: the stops count whole buckets as before.  ValueError with merge="ranks"."""
        self._check_merge(merge)
        self._check_filter(filter, filter_of, merge)
        self._check_stop_mass(stop_mass, n_categories)
        self._check_path_mass(path_mass, n_categories)
        s = time.time()
        eng = self.prepare(data_navigation, data_search, data_prediction, n_categories, metric=metric, assume_unchanged=assume_unchanged,
                           storage=storage)
        return self._search_with(eng, queries_navigation, queries_search, n_categories, n_buckets, k, s, stop_mass, path_mass, stop_rows, merge,
                                 filter, filter_of)

    def _search_with(self, eng, queries_navigation, queries_search, n_categories, n_buckets, k, s, stop_mass=None, path_mass=None,
                     stop_rows=None, merge="ranks", filter=None, filter_of=None, on_device=False):
        """`on_device` (`search_like`): the queries are device tensors and go to the `_device` forms of the same engine calls."""
        if filter is not None and not isinstance(filter, _capi.Filter):   # an id list: one keep filter, made for this call
            made = _capi.Filter(eng, [np.asarray(filter).reshape(-1)])
            try:
                return self._search_with(eng, queries_navigation, queries_search, n_categories, n_buckets, k, s, stop_mass, path_mass,
                                         stop_rows, merge, made, filter_of, on_device)
            finally:
                made.close()
        union, chunks = self._search_union, self._search_chunks
        if on_device:
            union, chunks = functools.partial(union, on_device=True), functools.partial(chunks, on_device=True)
        run = union if merge == "union" else chunks
        if filter is not None:
            run = functools.partial(union, filter=filter, filter_of=filter_of)
        if stop_mass is None and path_mass is None and stop_rows is None:
            return run(eng, queries_navigation, queries_search, n_categories, n_buckets, k, s)
        # the engine's own settings come back afterwards: a later call without the arguments is as before
        before = eng.stop_mass, eng.path_mass, eng.stop_rows
        try:
            if stop_mass is not None:
                eng.set_stop_mass(stop_mass)
            if path_mass is not None:
                eng.set_path_mass(path_mass)
            if stop_rows is not None:
                eng.set_stop_rows(stop_rows)
            return run(eng, queries_navigation, queries_search, n_categories, n_buckets, k, s)
        finally:
            eng.set_stop_mass(before[0])
            eng.set_path_mass(before[1])
            eng.set_stop_rows(before[2])

    def _search_union(self, eng, queries_navigation, queries_search, n_categories, n_buckets, k, s, filter=None, filter_of=None,
                      on_device=False):
        """merge="union": the batch goes to the library whole (it groups the queries itself); a multi-level index is walked in
        pieces of `_nav_chunk()` queries, the walk's queue limit.  `filter` (a `_capi.Filter`) and `filter_of` go with the calls.
        `on_device` (`search_like`): the queries are float32 device tensors and go to the `_device` forms, in the same pieces."""
        fo = None if filter_of is None else np.asarray(filter_of).reshape(-1)
        measured_time = defaultdict(float)
        if on_device:
            qn, qs = queries_navigation, queries_search
            search_union, search_tree_union = self._device_form(eng.search_union_device, k), self._device_form(eng.search_tree_union_device, k)
        else:
            qn = np.ascontiguousarray(_query_array(queries_navigation), dtype=np.float32)   # the union calls take binary32 queries
            qs = qn if queries_search is queries_navigation else np.ascontiguousarray(_query_array(queries_search), dtype=np.float32)
            search_union, search_tree_union = eng.search_union, eng.search_tree_union
        assert qn.shape[0] == qs.shape[0]
        nq = qs.shape[0]
        if len(n_categories) == 1:
            assert n_buckets <= eng.n_classes, "n_buckets exceeds the number of classes"
        if nq == 0:
            return np.empty((0, k)), np.empty((0, k), dtype=np.uint32), measured_time
        t0 = time.time()
        if len(n_categories) == 1:
            d32, nns = search_union(qn, qs, n_buckets, k, filter=filter, filter_of=fo)[:2]
        else:
            step = self._nav_chunk()
            parts = [search_tree_union(qn[lo: lo + step], qn[lo: lo + step] if qs is qn else qs[lo: lo + step], n_buckets, k,
                                           filter=filter, filter_of=None if fo is None else fo[lo: lo + step])[:2]
                     for lo in range(0, nq, step)]
            d32 = parts[0][0] if len(parts) == 1 else np.concatenate([p[0] for p in parts])
            nns = parts[0][1] if len(parts) == 1 else np.concatenate([p[1] for p in parts])
        measured_time["search_within_buckets"] = time.time() - t0   # wall time of the calls: the library times no phase of them
        measured_time["search"] = time.time() - s
        return d32.astype(np.float64), nns, measured_time

    # ---- range search (an extension; no reference counterpart): every object of the visited buckets within a radius ----
    @staticmethod
    def _check_range(radius, max_total, storage) -> None:
        """Refused before any work is done."""
        if radius is None:
            raise ValueError("range_search: radius is None")
        if isinstance(max_total, bool) or not isinstance(max_total, (int, np.integer)) or max_total < 0:
            raise ValueError(f"range_search: max_total {max_total!r} must be an integer >= 0 (0: no limit)")
        if storage != "f32":
            raise ValueError(f"range_search needs the default storage ('f32', prefilter on): the candidates are read from the row-major "
                             f"image, which storage={storage!r} does not keep")

    def range_search(
        self,
        data_navigation: pd.DataFrame,
        queries_navigation: npt.NDArray[np.float32],
        data_search: pd.DataFrame,
        queries_search: npt.NDArray[np.float32],
        data_prediction: npt.NDArray[np.int64],
        n_categories: List[int],
        radius,
        n_buckets: int = 1,
        metric: str = "ip",
        sort: bool = False,
        max_total: int = 0,
        assume_unchanged: bool = False,
        stop_mass: Optional[float] = None,
        path_mass: Optional[float] = None,
        stop_rows: Optional[int] = None,
        filter=None,
        filter_of=None,
        storage: str = "f32",
    ):
        """Every object of each query's `n_buckets` most probable buckets whose distance to the query is <= `radius` (a number, or one
        per query): `lmi_search_range` / `lmi_search_tree_range`.  Returns (lims i64[nq + 1], dists f64[total], nns u32[total],
        measured_time): query q owns [lims[q], lims[q + 1]), its results in (rank, row) order -- or, with `sort=True`, stably sorted
        by distance (on the device when the engine has `range_sort`: `lmi_range_result_sort`).  `metric`, `assume_unchanged`, the
        stops, `filter` and `filter_of` as in `search` (the filter needs no `merge`); `max_total` > 0 makes the call fail (`_capi.LmiError`) once more results than that have been counted -- on a
        multi-level index per piece of `_nav_chunk()` queries, less what the earlier pieces returned.  It needs the default storage:
        ValueError otherwise, before any work."""
        self._check_range(radius, max_total, storage)
        self._check_filter(filter, filter_of, "union")
        self._check_stop_mass(stop_mass, n_categories)
        self._check_path_mass(path_mass, n_categories)
        s = time.time()
        eng = self.prepare(data_navigation, data_search, data_prediction, n_categories, metric=metric, assume_unchanged=assume_unchanged,
                           storage=storage)
        return self._range_with(eng, queries_navigation, queries_search, n_categories, n_buckets, radius, sort, max_total, s, stop_mass,
                                path_mass, stop_rows, filter, filter_of)

    def range_search_resident(self, queries_navigation, queries_search, n_categories: List[int], radius, n_buckets: int = 1,
                              sort: bool = False, max_total: int = 0, stop_mass: Optional[float] = None,
                              path_mass: Optional[float] = None, stop_rows: Optional[int] = None, filter=None, filter_of=None):
        """`range_search` against the index already resident in HBM: no DataFrames needed.  Same return values."""
        assert self._engine is not None, "no resident index: call prepare()/search() or index_io.load_index()"
        self._check_range(radius, max_total, getattr(self._engine, "storage", "f32"))
        self._check_filter(filter, filter_of, "union")
        self._check_stop_mass(stop_mass, n_categories)
        self._check_path_mass(path_mass, n_categories)
        return self._range_with(self._engine, queries_navigation, queries_search, n_categories, n_buckets, radius, sort, max_total,
                                time.time(), stop_mass, path_mass, stop_rows, filter, filter_of)

    # ---- exact range search (an extension; no reference counterpart): every stored object within a radius, buckets pruned by balls ----
    def range_search_exact(
        self,
        data_navigation: pd.DataFrame,
        queries_navigation: npt.NDArray[np.float32],
        data_search: pd.DataFrame,
        queries_search: npt.NDArray[np.float32],
        data_prediction: npt.NDArray[np.int64],
        n_categories: List[int],
        radius,
        metric: str = "ip",
        sort: bool = False,
        max_total: int = 0,
        assume_unchanged: bool = False,
        filter=None,
        filter_of=None,
    ):
        """EVERY object of the index whose distance to the query is <= `radius` (a number, or one per query): `lmi_search_range_exact`.
        No model is consulted and there is no `n_buckets`: the buckets a query visits are those whose covering ball (centre, radius:
        `_capi.Cover`, over the leaf buckets of 1-level and multi-level indexes alike) its own ball may meet, and the answer is the one a
        brute force over all stored objects gives.  `queries_navigation` is accepted for symmetry with `range_search` and not read.
        Return values, `sort`, `max_total`, `filter` and `filter_of` as in `range_search`; the results of a query come in (bucket, row)
        order unless sorted.  The cover is made on first use, kept with the resident index and made again when the library calls it
        stale (after `insert` / `delete`).  It needs the default storage."""
        self._check_range(radius, max_total, "f32")
        self._check_filter(filter, filter_of, "union")
        s = time.time()
        eng = self.prepare(data_navigation, data_search, data_prediction, n_categories, metric=metric, assume_unchanged=assume_unchanged)
        return self._range_exact_with(eng, queries_search, radius, sort, max_total, s, filter, filter_of)

    def range_search_exact_resident(self, queries_navigation, queries_search, n_categories: List[int], radius, sort: bool = False,
                                    max_total: int = 0, filter=None, filter_of=None):
        """`range_search_exact` against the index already resident in HBM: no DataFrames needed.  Same return values."""
        eng = self._resident("range_search_exact_resident")
        self._check_range(radius, max_total, getattr(eng, "storage", "f32"))
        self._check_filter(filter, filter_of, "union")
        return self._range_exact_with(eng, queries_search, radius, sort, max_total, time.time(), filter, filter_of)

    @staticmethod
    def _cover_of(eng, remake: bool = False):
        """The engine's cover: made on first use and kept with the engine."""
        cover = getattr(eng, "_li_cover", None)
        if remake and cover is not None:
            cover.close()
            cover = None
        if cover is None or getattr(cover, "_c", None) is None:
            cover = _capi.Cover(eng)
            eng._li_cover = cover
        return cover

    def _range_exact_with(self, eng, queries_search, radius, sort, max_total, s, filter, filter_of):
        if filter is not None and not isinstance(filter, _capi.Filter):   # an id list: one keep filter, made for this call
            made = _capi.Filter(eng, [np.asarray(filter).reshape(-1)])
            try:
                return self._range_exact_with(eng, queries_search, radius, sort, max_total, s, made, filter_of)
            finally:
                made.close()
        fo = None if filter_of is None else np.asarray(filter_of).reshape(-1)
        measured_time = defaultdict(float)
        qs = np.ascontiguousarray(_query_array(queries_search), dtype=np.float32)
        nq = qs.shape[0]
        r = np.asarray(radius, dtype=np.float32)
        if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != nq):
            raise ValueError(f"range_search_exact: radius must be a number or one number per query ([{nq}]), not {tuple(r.shape)}")
        r = np.ascontiguousarray(np.broadcast_to(r, (nq,)))
        if nq == 0:
            return np.zeros(1, dtype=np.int64), np.empty(0), np.empty(0, dtype=np.uint32), measured_time
        t0 = time.time()
        cover = self._cover_of(eng)
        measured_time["cover"] = time.time() - t0
        t0 = time.time()
        try:
            lims, d32, nns = eng.search_range_exact(qs, r, cover, filter=filter, filter_of=fo, max_total=max_total, sort=bool(sort))
        except _capi.LmiError as e:
            if "stale" not in str(e) or "cover" not in str(e):
                raise
            cover = self._cover_of(eng, remake=True)   # the index was mutated since the cover was made
            lims, d32, nns = eng.search_range_exact(qs, r, cover, filter=filter, filter_of=fo, max_total=max_total, sort=bool(sort))
        measured_time["search_within_buckets"] = time.time() - t0   # wall time of the call: the library times no phase of it
        measured_time["search"] = time.time() - s
        measured_time["buckets_visited"] = float(_capi.cover_last_plan()["ADMITTED"]) / nq
        return lims, d32.astype(np.float64), nns, measured_time

    def _range_with(self, eng, queries_navigation, queries_search, n_categories, n_buckets, radius, sort, max_total, s, stop_mass,
                    path_mass, stop_rows, filter, filter_of):
        if filter is not None and not isinstance(filter, _capi.Filter):   # an id list: one keep filter, made for this call
            made = _capi.Filter(eng, [np.asarray(filter).reshape(-1)])
            try:
                return self._range_with(eng, queries_navigation, queries_search, n_categories, n_buckets, radius, sort, max_total, s,
                                        stop_mass, path_mass, stop_rows, made, filter_of)
            finally:
                made.close()
        run = functools.partial(self._range_run, eng, queries_navigation, queries_search, n_categories, n_buckets, radius, sort, max_total,
                                s, filter, filter_of)
        if stop_mass is None and path_mass is None and stop_rows is None:
            return run()
        before = eng.stop_mass, eng.path_mass, eng.stop_rows   # the engine's own settings come back afterwards
        try:
            if stop_mass is not None:
                eng.set_stop_mass(stop_mass)
            if path_mass is not None:
                eng.set_path_mass(path_mass)
            if stop_rows is not None:
                eng.set_stop_rows(stop_rows)
            return run()
        finally:
            eng.set_stop_mass(before[0])
            eng.set_path_mass(before[1])
            eng.set_stop_rows(before[2])

    def _range_run(self, eng, queries_navigation, queries_search, n_categories, n_buckets, radius, sort, max_total, s, filter, filter_of):
        """The batch goes to the library whole on a 1-level index; a multi-level index is walked in pieces of `_nav_chunk()` queries and
        the pieces' lims are joined."""
        fo = None if filter_of is None else np.asarray(filter_of).reshape(-1)
        measured_time = defaultdict(float)
        qn = np.ascontiguousarray(_query_array(queries_navigation), dtype=np.float32)
        qs = qn if queries_search is queries_navigation else np.ascontiguousarray(_query_array(queries_search), dtype=np.float32)
        assert qn.shape[0] == qs.shape[0]
        nq = qs.shape[0]
        r = np.asarray(radius, dtype=np.float32)
        if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != nq):
            raise ValueError(f"range_search: radius must be a number or one number per query ([{nq}]), not {tuple(r.shape)}")
        r = np.ascontiguousarray(np.broadcast_to(r, (nq,)))
        if len(n_categories) == 1:
            assert n_buckets <= eng.n_classes, "n_buckets exceeds the number of classes"
        if nq == 0:
            return np.zeros(1, dtype=np.int64), np.empty(0), np.empty(0, dtype=np.uint32), measured_time
        t0 = time.time()
        call = eng.search_range if len(n_categories) == 1 else eng.search_tree_range
        # an engine that sorts on the device (`range_sort`) is asked to; any other, and a call that takes no `sort`, is called as ever
        # and its results are ordered below
        engine_sorts = bool(sort) and bool(getattr(eng, "range_sort", False)) and "sort" in inspect.signature(call).parameters
        how = {"sort": True} if engine_sorts else {}
        if len(n_categories) == 1:
            lims, d32, nns = eng.search_range(qn, qs, n_buckets, r, filter=filter, filter_of=fo, max_total=max_total, **how)[:3]
        else:
            step = self._nav_chunk()
            parts, got = [], 0
            for lo in range(0, nq, step):
                # what is left of the budget (a 0 would mean "no limit" to the library: 1 then, and the sum is checked below)
                left = max(1, max_total - got) if max_total > 0 else 0
                part = eng.search_tree_range(qn[lo: lo + step], qn[lo: lo + step] if qs is qn else qs[lo: lo + step], n_buckets,
                                             r[lo: lo + step], filter=filter, filter_of=None if fo is None else fo[lo: lo + step],
                                             max_total=left, **how)[:3]   # segments never span pieces: each is sorted by its call
                if max_total > 0 and got + int(part[0][-1]) > max_total:
                    raise _capi.LmiError(f"range_search: more than max_total = {max_total} results: {got + int(part[0][-1])} had been "
                                         f"counted when the call stopped")
                got += int(part[0][-1])
                parts.append(part)
            lims = np.concatenate([parts[0][0][:1]] + [p[0][1:] + off for p, off in
                                                       zip(parts, np.cumsum([0] + [int(p[0][-1]) for p in parts[:-1]]))]).astype(np.int64)
            d32 = np.concatenate([p[1] for p in parts])
            nns = np.concatenate([p[2] for p in parts])
        if sort and not engine_sorts:
            for q in range(nq):
                a, b = int(lims[q]), int(lims[q + 1])
                if b - a > 1:
                    o = np.argsort(d32[a:b], kind="stable")
                    d32[a:b], nns[a:b] = d32[a:b][o], nns[a:b][o]
        measured_time["search_within_buckets"] = time.time() - t0   # wall time of the calls: the library times no phase of them
        measured_time["search"] = time.time() - s
        return lims, d32.astype(np.float64), nns, measured_time

    def _search_chunks(self, eng, queries_navigation, queries_search, n_categories, n_buckets, k, s, on_device=False):
        """`on_device` (`search_like`): the queries are float32 device tensors and go to the `_device` forms, in the same chunks."""
        measured_time = defaultdict(float)
        if on_device:
            qn, qs = queries_navigation, queries_search
            kout = _capi.Index.kout(n_buckets, k)
            search, search_tree = self._device_form(eng.search_device, kout), self._device_form(eng.search_tree_device, kout)
        else:
            qn = _query_array(queries_navigation)   # float16 arrays stay halves: the engine uploads them as they are
            qs = qn if queries_search is queries_navigation else _query_array(queries_search)
            search, search_tree = eng.search, eng.search_tree
        assert qn.shape[0] == qs.shape[0]
        nq = qs.shape[0]
        if n_buckets >= 2:
            # LearnedIndex.py:142-146: after the first merge the arrays must be (nq, k)
            assert k <= 2 * _capi.K_PER_BUCKET, "k > 20 cannot be merged from two 10-result ranks"
        if len(n_categories) == 1:
            assert n_buckets <= eng.n_classes, "n_buckets exceeds the number of classes"  # :213 would fail to broadcast
        if nq == 0:
            kout = _capi.Index.kout(n_buckets, k)
            return np.empty((0, kout)), np.empty((0, kout), dtype=np.uint32), measured_time
        # The prefilter's per-call workspace is ~10 KiB per (query, bucket) slot (candidate buffers): large batches x many
        # buckets are answered in query chunks that keep it under _WORKSPACE_BYTES.  The library says what a call needs.
        fixed = eng.workspace_bytes(0, n_buckets)
        per_query = max(1, (eng.workspace_bytes(1024, n_buckets) - fixed) // 1024)
        step = max(1, min(nq, (self._WORKSPACE_BYTES - fixed) // per_query if self._WORKSPACE_BYTES > fixed else 1))
        if len(n_categories) > 1:
            step = min(step, self._nav_chunk())
        parts_d, parts_n = [], []
        for lo in range(0, nq, step):
            hi = min(nq, lo + step)
            whole = lo == 0 and hi == nq
            qn_c = qn if whole else qn[lo:hi]
            qs_c = qs if whole else (qn_c if qs is qn else qs[lo:hi])
            if len(n_categories) == 1:
                d32, nn = search(qn_c, qs_c, n_buckets, k)[:2]
                t = eng.timings() * 1e-3
                measured_time["inference"] += float(t[_capi.T_INFERENCE])
            else:
                # the priority-queue walk on the device, then the scan of its buckets: one call (lmi_search_tree), the scan vectors
                # uploaded while the walk runs
                d32, nn = search_tree(qn_c, qs_c, n_buckets, k)
                t = eng.timings() * 1e-3
                measured_time["inference"] += float(t[_capi.T_INFERENCE])
            measured_time["search_within_buckets"] += float(t[_capi.T_ROUTE] + t[_capi.T_SCAN] + t[_capi.T_MERGE])
            measured_time["seq_search"] += float(t[_capi.T_SCAN])
            measured_time["sort"] += float(t[_capi.T_MERGE])
            parts_d.append(d32)
            parts_n.append(nn)
        d32 = parts_d[0] if len(parts_d) == 1 else np.concatenate(parts_d)
        nns = parts_n[0] if len(parts_n) == 1 else np.concatenate(parts_n)
        dists = d32.astype(np.float64)  # float32 values in a float64 array, like the reference (Q6)
        assert dists.shape == nns.shape
        measured_time["search"] = time.time() - s
        return dists, nns, measured_time

    @staticmethod
    def _device_form(call, kout: int):
        """The `_device` form of an engine's search call (`search_like`: the queries are float32 device tensors) as the host form is
        called: (qn_t, qs_t, n_buckets, k, **kw) -> (dists f32 [n, kout], ids u32 [n, kout]) as numpy, the outputs made beside the
        queries and read back once the call has run."""
        def run(qn_t, qs_t, n_buckets, k, **kw):
            import torch

            d_t = torch.empty((int(qs_t.shape[0]), kout), dtype=torch.float32, device=qs_t.device)
            i_t = torch.empty((int(qs_t.shape[0]), kout), dtype=torch.int32, device=qs_t.device)
            call(qn_t, qs_t, n_buckets, k, d_t, i_t, **kw)
            if d_t.is_cuda:
                torch.cuda.synchronize(d_t.device)
            return d_t.cpu().numpy(), i_t.cpu().numpy().view(np.uint32)
        return run

    # ------------------------------------------------------------------------------------------
    def _upload_tree(self, eng, n_levels: int) -> None:
        """Models of the internal nodes + the tree tables of lmi_nav_set_tree (include/lmi_hip.h).  Model 0 is the
        root, model i+1 the i-th entry of `internal_models`; child (m, c) is the path of model m extended by class
        c: an internal node, a listed bucket (slab id, or -1 when no object was placed there) or neither (-2)."""
        eng.set_mlp(linear_layers(self.root_model.model))
        prefixes = [()]
        model_of = {}
        for i, (path, net) in enumerate(self.internal_models.items()):
            prefix = tuple(int(v) for v in path if v != EMPTY_VALUE)
            eng.nav_set_model(i + 1, linear_layers(net.model))
            model_of[prefix] = i + 1
            prefixes.append(prefix)
        buckets = {tuple(int(v) for v in p if v != EMPTY_VALUE) for p in self.bucket_paths}
        classes = [linear_layers(self.root_model.model)[-1][0].shape[0]] + [
            linear_layers(net.model)[-1][0].shape[0] for net in self.internal_models.values()]
        offset, child_model, child_bucket, entry_path = [0], [], [], []
        for prefix, n_cls in zip(prefixes, classes):
            for c in range(n_cls):
                child = prefix + (c,)
                child_model.append(model_of.get(child, -1))
                padded = child + (EMPTY_VALUE,) * (n_levels - len(child))
                child_bucket.append(self._path_ids.get(padded, -1) if child in buckets else -2)
                entry_path.append(padded[:n_levels])
            offset.append(len(child_model))
        eng.nav_set_tree(offset, child_model, child_bucket)
        self._entry_paths = np.asarray(entry_path, dtype=np.int32).reshape(-1, n_levels)
        self._nav_cap = len(child_model)

    def _nav_chunk(self) -> int:
        """Queries per lmi_nav_order call: queue memory under _NAV_QUEUE_BYTES and under the call's 2^31-entry limit."""
        cap = max(1, getattr(self, "_nav_cap", 0) or len(self._entry_paths))
        entry_bytes = 12 if self._engine is not None and self._engine.path_mass > 0 else 8   # priority + child index (+ path mass)
        return max(1, min(self._NAV_QUEUE_BYTES // (entry_bytes * cap), ((1 << 31) - 1) // cap))

    @log_runtime(INFO, "Precomputed bucket order time: {}")
    def _precompute_bucket_order(self, queries_navigation: npt.NDArray[np.float32], n_buckets: int,
                                 n_categories: List[int]) -> Tuple[npt.NDArray[np.int32], float]:
        """(bucket_order int32[nq, n_buckets, n_levels], inference seconds) -- LearnedIndex.py:163-252.

        1 level: lmi_mlp_topk on the root model.  More levels: lmi_nav_order on the resident index (`prepare`
        uploaded the tree); the visited buckets' flat child indices are mapped back to their paths.  With the path-mass stop or the
        row-budget stop on (`Index.set_path_mass` / `Index.set_stop_rows` on the resident engine) the slots behind a query's stop are
        EMPTY_VALUE paths."""
        assert self.root_model is not None, "Model is not trained, call `build` first."
        qn = np.ascontiguousarray(queries_navigation, dtype=np.float32)
        n_queries, n_levels = qn.shape[0], len(n_categories)
        bucket_order = np.full((n_queries, n_buckets, n_levels), EMPTY_VALUE, dtype=np.int32)
        if n_levels == 1:
            eng = self.root_model.engine()
            bucket_order[:, :, 0] = eng.mlp_topk(qn, n_buckets)
            return bucket_order, float(eng.timings()[_capi.T_INFERENCE]) * 1e-3
        assert self._engine is not None, "multi-level navigation needs the resident index: call prepare() first"
        seconds, step = 0.0, self._nav_chunk()
        for lo in range(0, n_queries, step):
            _, entries = self._engine.nav_order(qn[lo: lo + step], n_buckets)
            seconds += float(self._engine.timings()[_capi.T_INFERENCE]) * 1e-3
            found = entries >= 0
            bucket_order[lo: lo + step][found] = self._entry_paths[entries[found]]
        return bucket_order, seconds
