"""Bucket-sharded multi-GPU search (no counterpart in the reference).

One process per GPU.  Bucket b lives on rank owner[b]; the MLP weights and the query batch are
replicated; every rank scans only the (query, rank) pairs whose bucket it owns, then an all-gather
(RCCL over xGMI; `gloo` in the CPU tests) moves every rank's `[dists | ids | keys]` block of nq*k*12
bytes and a merge kernel orders the union by (distance, bucket rank, position) -- the same total
order the single-GPU merge uses, so results are byte-identical for every world size.
Two layouts of the routing step (`ShardedSearcher(shard_inference=...)`):
  * False: every rank runs the MLP on the whole batch -- ONE collective per search (the all-gather above);
  * True (default for world > 1): every rank routes its 1/world slice of the batch and the bucket order
    (nq*nb*4 bytes) is all-gathered first -- TWO small collectives, 1/world of the MLP work per rank.
`merge="union"` (both searchers) answers with the union scan instead: the k <= 1024 best objects of all visited
buckets.  A rank's scan writes a PART (`Index.scan_union_part_device`: score bits | dist bits | ids | ranks | rows, int32 [5, nq, k]); the
one result collective moves 20*nq*k bytes per rank and the merge orders by (score, bucket rank, row) -- by score, not by distance, whose
rounding can make two scores one; by (rank, row), which orders as the single handle's ordinal does and needs no other rank's bucket sizes.
`range_search` (both searchers) answers the range query -- every object of the visited buckets within a radius.
A rank's `Index.scan_range_device` answers for the buckets it owns; its per-(query, bucket rank) counts and its [dists | ids] block (padded
to the largest rank's total) are all-gathered, and the join is a gather (`Index.join_range_parts`): a result is in (query, bucket rank, row)
order, every (query, bucket rank) names one bucket and one rank owns it, so every run comes whole from its owner -- no ordering by score.  `sort=True` sorts the JOINED result
by distance on the device (`RangeResult.sort`); the parts stay in (rank, row) order, which the join needs.
`ReplicaSearcher` is the other mode SURVEY section 8e names: QUERY-sharded replicas -- every rank holds the whole
index and answers its 1/world slice of the batch; one all-gather of [dists | ids | bucket order] rows.  A query's
answer does not depend on the rest of its batch, so the result is again byte-identical for every world size.  It
pays off when a rank's slice still fills the query tiles (>= ~350 queries per bucket and rank: batches of >= 80 k
at 8 ranks on the 10M benchmark); at 10 k queries bucket-sharding is 2-3 x faster.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np


def assign_buckets(sizes, world: int, weights=None) -> np.ndarray:
    """owner[L]: greedy longest-processing-time assignment of buckets to ranks.

    `weights` (default: sizes) is the expected scan work of a bucket; ties and zero-weight buckets
    are spread round-robin so that every rank's result is deterministic and identical on all ranks."""
    sizes = np.asarray(sizes, dtype=np.int64)
    w = sizes.astype(np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    owner = np.zeros(sizes.shape[0], dtype=np.int32)
    load = np.zeros(world, dtype=np.float64)
    count = np.zeros(world, dtype=np.int64)
    for b in np.argsort(-w, kind="stable"):
        r = int(np.lexsort((np.arange(world), count, load))[0])  # least load, then fewest buckets, then rank
        owner[b] = r
        load[r] += w[b]
        count[r] += 1
    return owner


def estimate_bucket_work(index, sample_nav_t, nb: int, sizes) -> np.ndarray:
    """Expected scan work of every bucket = its rows x the queries it will receive, the second factor
    estimated at build time by routing a sample of the DATA through the MLP like a query batch (top-nb).
    `index` needs its MLP set (`set_mlp`), not its buckets.  Deterministic: every rank computes the same
    weights for `assign_buckets` without any knowledge of the queries.  (Weights sizes**2 left one of eight
    ranks with 1.7x the mean work on the 10M x 768 benchmark; these are within 2 %.)"""
    import torch

    sizes = np.asarray(sizes, dtype=np.float64)
    probe = torch.empty((sample_nav_t.shape[0], nb), dtype=torch.int32, device=sample_nav_t.device)
    index.mlp_topk_device(sample_nav_t.contiguous(), nb, probe)
    torch.cuda.synchronize(sample_nav_t.device)
    visited = probe.cpu().numpy().ravel()
    routed = np.bincount(visited[visited >= 0], minlength=sizes.shape[0]).astype(np.float64)   # (-1: cut by the index's stop mass)
    return sizes * (routed[: sizes.shape[0]] + 1.0)


def ingest_owned(index, data, labels, L: int, owner, rank: int, ids=None, piece: int = 1 << 18) -> int:
    """Builds rank `rank`'s shard of a bucket-sharded index (`Index.add_owned_rows`): of the rows of `data` (a host array or
    memory map [N, d]) only those of the buckets with owner[b] == rank are read, `piece` rows at a time, and handed over with their
    original row numbers.  `data` is passed on in the type it has: float16 rows go in as halves (`lmi_buckets_add_owned_rows_f16`),
    anything else as float32.  Returns the number of rows this rank holds."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    owned = (np.asarray(owner).reshape(-1)[:L] == rank).astype(np.uint8)
    mine = np.flatnonzero(owned[labels] == 1).astype(np.int64)
    dtype = np.float16 if data.dtype == np.float16 else np.float32
    index.buckets_begin(labels, data.shape[1], L, ids, owned)
    for lo in range(0, mine.shape[0], piece):
        sel = mine[lo:lo + piece]
        index.add_owned_rows(np.ascontiguousarray(data[sel], dtype=dtype), sel)
    index.buckets_end()
    return int(mine.shape[0])


def pack_block(xp, dists, ids, keys):
    """[3, nq, kout] int32 block: float32 distance bits | uint32 ids | uint32 keys (xp: numpy or torch)."""
    if xp is np:
        return np.stack([dists.view(np.int32), ids.view(np.int32), keys.view(np.int32)])
    import torch

    return torch.stack([dists.view(torch.int32), ids.view(torch.int32), keys.view(torch.int32)])


def _all_gather_cat(t, world: int, group=None):
    """all_gather_into_tensor along dim 0.  RCCL ("nccl") takes device tensors as they are; under `gloo`
    (CPU rehearsals of the multi-rank path, also with tensors living on a GPU) the payload is staged on the host."""
    import torch
    import torch.distributed as dist

    t = t.contiguous()
    if t.is_cuda and dist.get_backend(group) == "gloo":
        out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype)
        dist.all_gather_into_tensor(out, t.cpu(), group=group)
        return out.to(t.device)
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t, group=group)
    return out


def all_gather_blocks(block, world: int, group=None):
    """The one collective of the path: [world, 3, nq, kout] <- all_gather(block)."""
    import torch
    import torch.distributed as dist

    shape = tuple(block.shape)
    out = _all_gather_cat(block, world, group)  # rank-major concatenation
    return out.view((world,) + shape)


def row_slice(nq: int, rank: int, world: int):
    """(per, lo, hi): rank's contiguous share [lo, hi) of nq rows in equal slices of `per` rows (the last ones short or empty)."""
    per = -(-nq // world)
    lo = min(rank * per, nq)
    return per, lo, min(lo + per, nq)


def all_gather_rows(local, nq: int, world: int, group=None):
    """[nq, ...] <- the ranks' [per, ...] slices concatenated in rank order (rows past a rank's share are padding)."""
    import torch
    import torch.distributed as dist

    per = local.shape[0]
    assert per * world >= nq
    return _all_gather_cat(local, world, group)[:nq]


def merge_blocks_numpy(gathered: np.ndarray, kout: int):
    """Host restatement of merge_gathered_kernel, used by the CPU (gloo) tests only."""
    world, three, nq, kk = gathered.shape
    assert three == 3 and kk == kout
    d = gathered[:, 0].view(np.float32).transpose(1, 0, 2).reshape(nq, world * kout).astype(np.float64)
    i = gathered[:, 1].view(np.uint32).transpose(1, 0, 2).reshape(nq, world * kout)
    k = gathered[:, 2].view(np.uint32).transpose(1, 0, 2).reshape(nq, world * kout).astype(np.int64)
    src = np.broadcast_to(np.repeat(np.arange(world), kout)[None, :], k.shape)
    order = np.lexsort((src, k, d), axis=1)[:, :kout]
    return np.take_along_axis(d, order, 1).astype(np.float32), np.take_along_axis(i, order, 1)


def merge_union_parts_numpy(gathered: np.ndarray):
    """Host restatement of union_merge_kernel (lmi_merge_union_parts), used by the CPU tests only: gathered int32 [world, 5, nq, k] ->
    (dists f32[nq, k], ids u32[nq, k], counts i32[nq])."""
    world, five, nq, k = gathered.shape
    assert five == 5
    flat = lambda p: np.ascontiguousarray(gathered[:, p].transpose(1, 0, 2)).reshape(nq, world * k)
    score = flat(0).view(np.float32).astype(np.float64)
    dist, ids = flat(1).view(np.float32), flat(2).view(np.uint32)
    rank, row = flat(3).view(np.uint32).astype(np.int64), flat(4).view(np.uint32).astype(np.int64)
    real = row != 0xFFFFFFFF
    src = np.broadcast_to(np.repeat(np.arange(world), k)[None, :], row.shape)
    # padding behind everything real; -score: -0.0 and +0.0 compare equal
    order = np.lexsort((src, row, rank, np.where(real, -score, np.inf)), axis=1)[:, :k]
    sel = np.take_along_axis(real, order, 1)
    d = np.where(sel, np.take_along_axis(dist, order, 1), np.float32(np.inf)).astype(np.float32)
    i = np.where(sel, np.take_along_axis(ids, order, 1), 0).astype(np.uint32)
    return d, i, sel.sum(axis=1).astype(np.int32)


def join_range_parts_numpy(counts, dists, ids):
    """Host restatement of `lmi_join_range_parts`, used by the CPU tests and their stand-in index: counts int [world, nq, nb], `dists` /
    `ids` lists of the parts' arrays in (query, t, row) order (None for a part without results) -> (lims i64[nq + 1], dists f32[total],
    ids u32[total]).  The run of (q, t) is the run of the one part whose count is > 0, copied unchanged; a (q, t) two parts both claim
    means overlapping ownership: ValueError, as the library refuses it."""
    counts = np.asarray(counts)
    if counts.ndim != 3:
        raise ValueError("join_range_parts_numpy: counts must be [world, nq, nb]")
    world, nq, nb = counts.shape
    c = counts.astype(np.int64).reshape(world, nq * nb)
    if (c < 0).any():
        r, s = (int(x[0]) for x in np.nonzero(c < 0))
        raise ValueError(f"join_range_parts_numpy: the count of part {r} at query {s // nb}, t {s % nb} is negative")
    claimed = (c > 0).sum(axis=0)
    if (claimed > 1).any():
        s = int(np.flatnonzero(claimed > 1)[0])
        a, b = (int(x) for x in np.flatnonzero(c[:, s] > 0)[:2])
        raise ValueError(f"join_range_parts_numpy: query {s // nb}, t {s % nb} has results in part {a} and in part {b}: the parts' "
                         "buckets overlap")
    src = np.cumsum(c, axis=1) - c                      # a part's exclusive run offsets
    n = c.sum(axis=0)
    first = np.concatenate([[0], np.cumsum(n)])         # the joined result's
    total = int(first[-1])
    owner = np.argmax(c > 0, axis=0)
    out_d, out_i = np.empty(total, np.float32), np.empty(total, np.uint32)
    for r in range(world):
        if c[r].sum() == 0:
            continue
        pd = np.asarray(dists[r]).view(np.float32).reshape(-1)
        pi = np.asarray(ids[r]).view(np.uint32).reshape(-1)
        for s in np.flatnonzero((owner == r) & (n > 0)):
            out_d[first[s]: first[s] + n[s]] = pd[src[r, s]: src[r, s] + n[s]]
            out_i[first[s]: first[s] + n[s]] = pi[src[r, s]: src[r, s] + n[s]]
    return first[::nb].astype(np.int64), out_d, out_i   # lims[q] = first[q * nb]


def _radius_rows(radius, nq: int) -> np.ndarray:
    """radius f32[nq] of a sharded range search: a scalar serves every query (the same on every rank)."""
    r = np.asarray(radius.cpu().numpy() if hasattr(radius, "cpu") else radius)
    if r.dtype.kind not in "fiu" or r.ndim > 1 or (r.ndim == 1 and r.shape[0] != nq):
        raise ValueError(f"range_search: radius must be a number or one number per query ([{nq}])")
    return np.ascontiguousarray(np.broadcast_to(r.astype(np.float32), (nq,)))


def _read_range(res, dev):
    """(lims, dists tensor, ids tensor) of a range result on `dev`; the result is closed."""
    import torch

    d = torch.empty(res.total, dtype=torch.float32, device=dev)
    i = torch.empty(res.total, dtype=torch.int32, device=dev)
    if res.total > 0:
        res.read_into(d, i)
    lims = np.array(res.lims, dtype=np.int64)
    res.close()
    return lims, d, i


def _read_empty(dev):
    import torch

    return torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)


def _over_total(who: str, max_total: int, total: int):
    from ._capi import LmiError

    return LmiError(f"{who}: more than max_total = {max_total} results: the ranks hold {total}")


def _check_merge(merge, filter=None) -> None:
    if merge not in ("ranks", "union"):
        raise ValueError(f"merge must be 'ranks' or 'union', not {merge!r}")
    if filter is not None:   # (the part form of the union scan has no filtered counterpart yet: DESIGN.md section 5.14.2)
        raise ValueError("a filter is not supported by the sharded searchers (use Index.search_union(filter=...) on one handle)")


class ShardedSearcher:
    """Device-side driver of the sharded search for one rank (torch tensors in, torch tensors out).

    `shard_inference` (default on for world > 1): every rank runs the MLP on its 1/world slice of the query
    batch and the bucket order is all-gathered (nq*nb*4 bytes), instead of every rank routing the whole batch
    (at 8 ranks the replicated MLP was a sixth of a rank's step).  `calls_per_search` tells a caller that
    averages `Index.timings_mean()` how many C-ABI calls one search makes."""

    def __init__(self, index, rank: int, world: int, group=None, shard_inference: bool = True, lib_comm=None,
                 stop_mass: Optional[float] = None, stop_rows: Optional[int] = None):
        """`lib_comm`: an ncclComm_t from `Index.comm_init` -- the result exchange then runs inside the library
        (`lmi_allgather_merge`: ncclAllGather + merge kernel on the handle's stream) instead of torch.distributed.
        `stop_mass`: the probability-mass stop (`Index.set_stop_mass`), set on the rank's handle until `close()` gives
        the handle its earlier value back; None leaves the handle's own setting.  Every rank cuts the order of the queries
        it routes (its slice, or the whole batch), so the gathered order carries the -1s and every rank skips the same slots.
        `stop_rows`: the row-budget stop (`Index.set_stop_rows`), kept and given back like `stop_mass`.  World of one only: a
        rank of a bucket-sharded index holds its own buckets' counts, not the other ranks', so ValueError for world > 1 (before
        anything is set)."""
        if stop_rows is not None and world > 1:
            raise ValueError("stop_rows is not supported on a bucket-sharded index of more than one rank (a rank does not know the "
                             "other ranks' bucket sizes); ReplicaSearcher holds the whole index on every rank")
        self._mass_before = None
        self._rows_before = None
        if stop_mass is not None:
            self._mass_before = index.stop_mass
            index.set_stop_mass(stop_mass)
        if stop_rows is not None:
            self._rows_before = index.stop_rows
            index.set_stop_rows(stop_rows)
        self.index, self.rank, self.world, self.group = index, rank, world, group
        self.lib_comm = lib_comm
        self.shard_inference = bool(shard_inference) and world > 1
        self.calls_per_search = 2 if self.shard_inference else 1
        self._buf = None
        self._ubuf = None
        self._bo_loc = None
        # time_collectives: every collective of a search is bracketed by two events on the current stream (device tensors) -- what a
        # rank really WAITS for each exchange, the other ranks' lateness included; read with collective_ms() after a synchronize
        self.time_collectives = False
        self._coll = {"bucket_order_allgather": [], "result_allgather_merge": []}

    def close(self) -> None:
        """Ends the constructor's `stop_mass` / `stop_rows`: the handle gets the values it had before (the index itself stays open)."""
        if self._mass_before is not None:
            self.index.set_stop_mass(self._mass_before)
            self._mass_before = None
        if self._rows_before is not None:
            self.index.set_stop_rows(self._rows_before)
            self._rows_before = None

    # ---- stored objects by id across the ranks: every rank fetches what it owns, the join is a host-side pick.  `reconstruct` is the
    #      call; `fetch_part` and `join_fetch_parts` are its two halves, public as helpers for ranks that live in separate processes
    #      (the library makes no collective here: INTEGRATION.md section 3 has the recipe) ----
    def fetch_part(self, ids, dtype=np.float32):
        """This rank's part of a fetch: (rows [n, d], bucket i32 [n], row i32 [n]) of `Index.fetch(ids, where=True)` on the rank's
        handle.  An id whose bucket another rank owns is absent here (zero row, bucket -1): the bucket holds no rows on this rank."""
        return self.index.fetch(ids, dtype=dtype, where=True)

    @staticmethod
    def join_fetch_parts(ids, parts):
        """The ranks' `fetch_part` results for the same `ids`, in rank order -> rows [n, d]: per request the row of the rank that
        holds it (`bucket >= 0`); where objects on several ranks carry the id, the first by (bucket, row), as on one handle.  Host
        arrays, no collective.  KeyError naming up to ten ids no rank holds."""
        absent = np.iinfo(np.int64).max
        where = np.stack([np.where(b >= 0, (b.astype(np.int64) << 32) | r.astype(np.int64), absent) for _, b, r in parts])   # [world, n]
        best = where.argmin(axis=0)
        found = where.min(axis=0) != absent
        rows = np.zeros_like(parts[0][0])
        for rank, (part_rows, _, _) in enumerate(parts):
            take = found & (best == rank)
            rows[take] = part_rows[take]
        if not found.all():
            gone = np.unique(np.asarray(ids).reshape(-1)[~found])
            more = f" and {gone.size - 10} more" if gone.size > 10 else ""
            raise KeyError(f"reconstruct: {[int(v) for v in gone[:10]]}{more} not in the index")
        return rows

    def reconstruct(self, ids, dtype=np.float32, peers=()):
        """The scan vectors of the objects with these ids, [n, d], from a bucket-sharded index: what `Index.fetch` returns on one
        handle that holds everything.  `peers`: the other ranks' searchers where one process drives several ranks (one per
        card); their parts are joined on the host.  No collective is made: ranks that live in other processes exchange their
        `fetch_part` results by whatever carries host arrays and call `join_fetch_parts`.  KeyError for an id no rank holds."""
        if self.world > 1 and len(peers) != self.world - 1:
            raise ValueError(f"reconstruct: a world of {self.world} ranks needs the {self.world - 1} other ranks' searchers as peers "
                             f"(got {len(peers)}); across processes exchange fetch_part() results and call join_fetch_parts()")
        parts = [s.fetch_part(ids, dtype) for s in sorted([self, *peers], key=lambda s: s.rank)]
        return self.join_fetch_parts(ids, parts)

    def _timed(self, name, fn, on_cuda: bool):
        if not self.time_collectives or self.world == 1:
            return fn()
        import time

        import torch

        if on_cuda:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            self._coll[name].append((a, b))
        else:
            t0 = time.perf_counter()
            out = fn()
            self._coll[name].append((time.perf_counter() - t0) * 1e3)
        return out

    def collective_ms(self, reset: bool = True):
        """{collective: mean exposed ms per search} since the last reset (call after torch.cuda.synchronize())."""
        out = {}
        for name, items in self._coll.items():
            vals = [it if isinstance(it, float) else it[0].elapsed_time(it[1]) for it in items]
            out[name] = round(float(np.mean(vals)), 4) if vals else None
            if reset:
                items.clear()
        return out

    def _buffers(self, nq: int, nb: int, kout: int, dev):
        import torch

        if self._buf is None or self._buf[0].shape != (3, nq, kout):
            self._buf = (torch.empty((3, nq, kout), dtype=torch.int32, device=dev),
                         torch.empty((nq, kout), dtype=torch.float32, device=dev),
                         torch.empty((nq, kout), dtype=torch.int32, device=dev),
                         torch.empty((nq, nb), dtype=torch.int32, device=dev))
        return self._buf

    def new_route_buffer(self, nq: int, nb: int, dev):
        """[ceil(nq / world), nb] int32 buffer for `route_local` (a pipeline keeps one per batch in flight)."""
        import torch

        per, _, _ = row_slice(nq, self.rank, self.world)
        return torch.full((per, nb), -1, dtype=torch.int32, device=dev)

    def route_local(self, qn_t, nb: int, bo_loc) -> None:
        """This rank's share of the routing: the MLP on its 1/world slice of the batch -> bo_loc[: hi - lo].  No
        collective, so a pipeline may run it for batch i+1 on a stream of its own beside the scan of batch i."""
        assert self.shard_inference
        _, lo, hi = row_slice(qn_t.shape[0], self.rank, self.world)
        if hi > lo:
            self.index.mlp_topk_device(qn_t[lo:hi], nb, bo_loc[: hi - lo])

    def _union_buffers(self, nq: int, nb: int, k: int, dev):
        import torch

        if self._ubuf is None or self._ubuf[0].shape != (5, nq, k) or self._ubuf[4].shape != (nq, nb):
            self._ubuf = (torch.empty((5, nq, k), dtype=torch.int32, device=dev),
                          torch.empty((nq, k), dtype=torch.float32, device=dev),
                          torch.empty((nq, k), dtype=torch.int32, device=dev),
                          torch.empty((nq,), dtype=torch.int32, device=dev),
                          torch.empty((nq, nb), dtype=torch.int32, device=dev))
        return self._ubuf

    def _scan_exchange_union(self, qs_t, bo, nb: int, k: int):
        """merge="union" behind the routing: this rank's part of the union scan over `bo`, then the exchange -- none for a world of one
        without a communicator, `lmi_allgather_merge_union` with a `lib_comm`, else one all-gather of the [5, nq, k] block and
        `lmi_merge_union_parts`.  -> (dists [nq, k], ids, bucket order, counts)."""
        import torch

        nq = qs_t.shape[0]
        part, out_d, out_i, cnt, _ = self._union_buffers(nq, nb, k, qs_t.device)
        self.index.scan_union_part_device(qs_t, bo, nb, k, part, cnt)
        if self.world == 1 and self.lib_comm is None:
            return part[1].view(torch.float32), part[2], bo, cnt
        if self.lib_comm is not None:
            self._timed("result_allgather_merge",
                        lambda: self.index.allgather_merge_union(self.lib_comm, self.rank, self.world, part, out_d, out_i, cnt), part.is_cuda)
            return out_d, out_i, bo, cnt

        def exchange():
            g = all_gather_blocks(part, self.world, self.group)  # [world, 5, nq, k]
            self.index.merge_union_parts(g, self.world, nq, k, out_d, out_i, cnt)

        self._timed("result_allgather_merge", exchange, part.is_cuda)
        return out_d, out_i, bo, cnt

    def search_routed(self, qs_t, bo_loc, nb: int, k: int, merge: str = "ranks", filter=None):
        """The rest of a sharded search: all-gather of the bucket order, scan of the owned buckets, all-gather + merge.
        merge="union": the union scan, k <= 1024 -> (dists [nq, k], ids, bucket order, counts)."""
        _check_merge(merge, filter)
        nq = qs_t.shape[0]
        if merge == "union":
            bo = self._timed("bucket_order_allgather", lambda: all_gather_rows(bo_loc, nq, self.world, self.group), bo_loc.is_cuda)
            return self._scan_exchange_union(qs_t, bo, nb, k)
        kout = self.index.kout(nb, k)
        blk, out_d, out_i, _ = self._buffers(nq, nb, kout, qs_t.device)
        bo = self._timed("bucket_order_allgather", lambda: all_gather_rows(bo_loc, nq, self.world, self.group), bo_loc.is_cuda)
        self.index.scan_topk_device(qs_t, bo, nb, k, blk[0], blk[1], blk[2])
        return self._exchange(blk, out_d, out_i, bo, nq, kout)

    def _exchange(self, blk, out_d, out_i, bo, nq: int, kout: int):
        import torch

        if self.world == 1 and self.lib_comm is None:
            return blk[0].view(torch.float32), blk[1], bo
        if self.lib_comm is not None:
            self._timed("result_allgather_merge",
                        lambda: self.index.allgather_merge(self.lib_comm, self.rank, self.world, blk[0], blk[1], blk[2], out_d, out_i), blk.is_cuda)
            return out_d, out_i, bo

        def exchange():
            g = all_gather_blocks(blk, self.world, self.group)  # [world, 3, nq, kout]
            plane = nq * kout
            self.index.merge_gathered(g[0, 0], g[0, 1], g[0, 2], self.world, nq, kout, out_d, out_i, world_stride=3 * plane)

        self._timed("result_allgather_merge", exchange, blk.is_cuda)
        return out_d, out_i, bo

    def search(self, qn_t, qs_t, nb: int, k: int, merge: str = "ranks", filter=None):
        """(dists, ids, bucket order); merge="union": the union scan, k <= 1024 -> (dists [nq, k], ids, bucket order, counts)."""
        _check_merge(merge, filter)
        nq = qn_t.shape[0]
        if self.shard_inference:
            if self._bo_loc is None or self._bo_loc.shape[1] != nb or self._bo_loc.shape[0] != row_slice(nq, self.rank, self.world)[0]:
                self._bo_loc = self.new_route_buffer(nq, nb, qn_t.device)
            self.route_local(qn_t, nb, self._bo_loc)
            return self.search_routed(qs_t, self._bo_loc, nb, k, merge)
        if merge == "union":
            bo = self._union_buffers(nq, nb, k, qn_t.device)[4]
            self.index.mlp_topk_device(qn_t, nb, bo)
            return self._scan_exchange_union(qs_t, bo, nb, k)
        kout = self.index.kout(nb, k)
        blk, out_d, out_i, bo = self._buffers(nq, nb, kout, qn_t.device)
        # the three planes of `blk` are written in place by lmi_search / lmi_scan_topk
        self.index.search_device(qn_t, qs_t, nb, k, blk[0], blk[1], blk[2], bo)
        return self._exchange(blk, out_d, out_i, bo, nq, kout)

    # ---- the range search: every object of the visited buckets within a radius, joined across the ranks ----
    def _scan_exchange_range(self, qs_t, bo, nb: int, radius, max_total: int, sort: bool = False):
        """Behind the routing: this rank's `scan_range_device` over `bo` (its owned buckets answer), then the exchange -- none for a
        world of one without a communicator; `lmi_allgather_join_range` with a `lib_comm`; else one all-gather of the nq*nb counts,
        one of the [2, Tmax] block (dists | ids, padded to the largest part) and `lmi_join_range_parts` on pointers into the gathered
        buffer.  `max_total` limits the joined result on every path, checked on the gathered counts, which every rank sees alike; a
        rank whose own part already exceeds it says so to the others through the counts, so that no rank waits in a collective.
        `sort`: the JOINED result is sorted by distance (`RangeResult.sort`) -- the parts must stay in (rank, row) order for the join."""
        import torch

        from ._capi import LmiError

        nq, dev = qs_t.shape[0], qs_t.device
        radius = _radius_rows(radius, nq)
        if self.world == 1 and self.lib_comm is None:
            how = {"sort": True} if sort else {}
            return _read_range(self.index.scan_range_device(qs_t, bo, nb, radius, max_total=max_total, **how), dev) + (bo,)
        if self.lib_comm is not None:
            part = self.index.scan_range_device(qs_t, bo, nb, radius)
            try:
                joined = self._timed("result_allgather_merge",
                                     lambda: self.index.allgather_join_range(self.lib_comm, self.rank, self.world, part, max_total), qs_t.is_cuda)
            finally:
                part.close()
            return _read_range(joined.sort(self.index) if sort else joined, dev) + (bo,)
        try:
            part = self.index.scan_range_device(qs_t, bo, nb, radius, max_total=max_total)
            counts = torch.from_numpy(part.pair_counts()).to(dev)
        except LmiError:
            if max_total == 0:
                raise
            part, counts = None, torch.full((nq, nb), -1, dtype=torch.int32, device=dev)   # this rank alone is over max_total

        def exchange():
            g_counts = _all_gather_cat(counts, self.world, self.group).cpu().numpy().reshape(self.world, nq, nb)
            if (g_counts < 0).any():
                raise LmiError(f"range_search: more than max_total = {max_total} results on rank {int(np.nonzero(g_counts < 0)[0][0])} alone")
            totals = g_counts.astype(np.int64).reshape(self.world, -1).sum(axis=1)
            if max_total > 0 and totals.sum() > max_total:
                raise _over_total("range_search", max_total, int(totals.sum()))
            tmax = int(totals.max())
            if tmax == 0:
                return self.index.join_range_parts(g_counts, [None] * self.world, [None] * self.world, max_total)
            blk = torch.zeros((2, tmax), dtype=torch.int32, device=dev)
            if part.total > 0:
                part.read_into(blk[0], blk[1])
            g = all_gather_blocks(blk, self.world, self.group)   # [world, 2, tmax]
            return self.index.join_range_parts(g_counts, [g[r, 0] for r in range(self.world)], [g[r, 1] for r in range(self.world)], max_total)

        try:
            joined = self._timed("result_allgather_merge", exchange, qs_t.is_cuda)
        finally:
            if part is not None:
                part.close()
        return _read_range(joined.sort(self.index) if sort else joined, dev) + (bo,)

    def range_search_routed(self, qs_t, bo_loc, nb: int, radius, max_total: int = 0, sort: bool = False):
        """The rest of a sharded range search behind `route_local`: all-gather of the bucket order (as `search_routed`), scan of the
        owned buckets, exchange and join -> (lims i64 numpy [nq + 1], dists tensor [total], ids tensor [total], bucket order)."""
        nq = qs_t.shape[0]
        radius = _radius_rows(radius, nq)
        bo = self._timed("bucket_order_allgather", lambda: all_gather_rows(bo_loc, nq, self.world, self.group), bo_loc.is_cuda)
        return self._scan_exchange_range(qs_t, bo.contiguous(), nb, radius, max_total, sort)

    def range_search(self, qn_t, qs_t, nb: int, radius, max_total: int = 0, sort: bool = False):
        """Per query every object of its nb visited buckets within `radius` (a number, or one per query; the same on every rank), in
        (bucket rank, row) order: what `Index.search_range` returns on one handle that holds the whole index, bit for bit, on every
        rank.  Routing as `search(merge="union")`.  `sort=True`: nearest first -- the joined result is sorted on the device after the
        join, alike on every rank.  -> (lims i64 numpy [nq + 1], dists tensor, ids tensor, bucket order)."""
        import torch

        nq = qn_t.shape[0]
        radius = _radius_rows(radius, nq)   # (argument errors before any work)
        if self.shard_inference:
            if self._bo_loc is None or self._bo_loc.shape[1] != nb or self._bo_loc.shape[0] != row_slice(nq, self.rank, self.world)[0]:
                self._bo_loc = self.new_route_buffer(nq, nb, qn_t.device)
            self.route_local(qn_t, nb, self._bo_loc)
            return self.range_search_routed(qs_t, self._bo_loc, nb, radius, max_total, sort)
        bo = torch.empty((nq, nb), dtype=torch.int32, device=qn_t.device)
        self.index.mlp_topk_device(qn_t, nb, bo)
        return self._scan_exchange_range(qs_t, bo, nb, radius, max_total, sort)


class ReplicaSearcher:
    """Query-sharded replicas: the index is whole on every rank (`set_buckets` / `add_rows` without an `owned`
    mask), rank r answers rows [lo, hi) of the batch (`row_slice`) and ONE all-gather assembles the batch's
    answer: per query [kout distances | kout ids | nb buckets] as int32 words.  No merge step: the slices are
    disjoint.  Same call signature and return value as `ShardedSearcher.search`."""

    calls_per_search = 1
    shard_inference = False   # (HostPipeline: nothing to route ahead of the search call)
    lib_comm = None

    def __init__(self, index, rank: int, world: int, group=None, stop_mass: Optional[float] = None, stop_rows: Optional[int] = None):
        """`stop_mass`: as `ShardedSearcher` (a rank's slice of the batch is cut by its own search call; `close()` ends it).
        `stop_rows`: the row-budget stop, for any world: every rank holds the whole index and with it every bucket's count."""
        self.index, self.rank, self.world, self.group = index, rank, world, group
        self._buf = None
        self._mass_before = None
        self._rows_before = None
        if stop_rows is not None:
            self._rows_before = index.stop_rows
            index.set_stop_rows(stop_rows)
        if stop_mass is not None:
            self._mass_before = index.stop_mass
            index.set_stop_mass(stop_mass)

    close = ShardedSearcher.close

    def _buffers(self, per: int, nb: int, kout: int, dev):
        import torch

        if self._buf is None or self._buf[0].shape != (per, 2 * kout + nb):
            self._buf = (torch.empty((per, 2 * kout + nb), dtype=torch.int32, device=dev),
                         torch.empty((per, kout), dtype=torch.float32, device=dev),
                         torch.empty((per, kout), dtype=torch.int32, device=dev),
                         torch.empty((per, kout), dtype=torch.int32, device=dev),
                         torch.empty((per, nb), dtype=torch.int32, device=dev))
        return self._buf

    def _search_union(self, qn_t, qs_t, nb: int, k: int):
        """merge="union": `search_union_device` on the rank's slice, then one all-gather of [k dists | k ids | count | nb buckets] rows."""
        import torch

        nq, dev = qn_t.shape[0], qn_t.device
        per, lo, hi = row_slice(nq, self.rank, self.world)
        d = torch.full((per, k), float("inf"), dtype=torch.float32, device=dev)
        i = torch.zeros((per, k), dtype=torch.int32, device=dev)
        c = torch.zeros((per,), dtype=torch.int32, device=dev)
        bo = torch.full((per, nb), -1, dtype=torch.int32, device=dev)
        if hi > lo:
            n = hi - lo
            self.index.search_union_device(qn_t[lo:hi], qs_t[lo:hi], nb, k, d[:n], i[:n], c[:n], bo[:n])
        if self.world == 1:
            return d[:nq], i[:nq], bo[:nq], c[:nq]
        row = torch.cat([d.view(torch.int32), i, c[:, None], bo], dim=1)
        g = all_gather_rows(row, nq, self.world, self.group)   # the one collective
        return (g[:, :k].contiguous().view(torch.float32), g[:, k:2 * k].contiguous(), g[:, 2 * k + 1:].contiguous(),
                g[:, 2 * k].contiguous())

    def range_search(self, qn_t, qs_t, nb: int, radius, max_total: int = 0, sort: bool = False):
        """Same signature and return value as `ShardedSearcher.range_search` (`sort=True`: a rank sorts its slice's result before the
        exchange -- a query's results all lie in one slice).  `search_range_device` on the rank's slice with that slice
        of `radius`; one all-gather of [count | nb buckets] rows and one of the [2, Tmax] payload (dists | ids, padded to the largest
        slice's total).  The slices are contiguous runs of queries, so the batch's result is their concatenation in rank order: no
        kernel.  `max_total` limits the batch's total, checked on the gathered counts (alike on every rank)."""
        import torch

        from ._capi import LmiError

        nq, dev = qn_t.shape[0], qn_t.device
        radius = _radius_rows(radius, nq)
        per, lo, hi = row_slice(nq, self.rank, self.world)
        n = hi - lo
        bo = torch.full((per, nb), -1, dtype=torch.int32, device=dev)
        cnt = torch.zeros((per,), dtype=torch.int64, device=dev)
        part = None
        if n > 0:
            try:
                part = self.index.search_range_device(qn_t[lo:hi], qs_t[lo:hi], nb, radius[lo:hi], bo_t=bo[:n], max_total=max_total,
                                                      **({"sort": True} if sort else {}))
                cnt[:n] = torch.from_numpy(np.diff(part.lims)).to(dev)
            except LmiError:
                if max_total == 0 or self.world == 1:
                    raise
                cnt[:n] = -1   # this rank's slice alone is over max_total: the others learn it from the counts
        if self.world == 1:
            if part is None:   # an empty batch
                return (np.zeros(1, np.int64),) + _read_empty(dev) + (bo[:nq],)
            return _read_range(part, dev) + (bo[:nq],)
        try:
            row = torch.cat([cnt.view(torch.int32).view(per, 2), bo], dim=1)
            g = _all_gather_cat(row, self.world, self.group)           # [world * per, 2 + nb]
            counts = g[:, :2].contiguous().view(torch.int64).view(-1).cpu().numpy()
            if (counts < 0).any():
                raise LmiError(f"range_search: more than max_total = {max_total} results on rank {int(np.flatnonzero(counts < 0)[0]) // per} alone")
            totals = counts.reshape(self.world, per).sum(axis=1)
            if max_total > 0 and totals.sum() > max_total:
                raise _over_total("range_search", max_total, int(totals.sum()))
            lims = np.concatenate([[0], np.cumsum(counts[:nq])]).astype(np.int64)
            tmax = int(totals.max())
            if tmax == 0:
                return (lims,) + _read_empty(dev) + (g[:nq, 2:].contiguous(),)
            blk = torch.zeros((2, tmax), dtype=torch.int32, device=dev)
            if part is not None and part.total > 0:
                part.read_into(blk[0], blk[1])
            p = all_gather_blocks(blk, self.world, self.group)          # [world, 2, tmax]
            d = torch.cat([p[r, 0, : int(totals[r])] for r in range(self.world)]).view(torch.float32)
            i = torch.cat([p[r, 1, : int(totals[r])] for r in range(self.world)])
            return lims, d, i, g[:nq, 2:].contiguous()
        finally:
            if part is not None:
                part.close()

    def search(self, qn_t, qs_t, nb: int, k: int, merge: str = "ranks", filter=None):
        import torch

        _check_merge(merge, filter)
        if merge == "union":
            return self._search_union(qn_t, qs_t, nb, k)
        nq = qn_t.shape[0]
        kout = self.index.kout(nb, k)
        per, lo, hi = row_slice(nq, self.rank, self.world)
        row, d, i, keys, bo = self._buffers(per, nb, kout, qn_t.device)
        if hi > lo:
            n = hi - lo
            self.index.search_device(qn_t[lo:hi], qs_t[lo:hi], nb, k, d[:n], i[:n], keys[:n], bo[:n])
        if self.world == 1:
            return d[:nq], i[:nq], bo[:nq]
        row[:, :kout] = d.view(torch.int32)
        row[:, kout:2 * kout] = i
        row[:, 2 * kout:] = bo
        g = all_gather_rows(row, nq, self.world, self.group)   # the one collective
        return g[:, :kout].contiguous().view(torch.float32), g[:, kout:2 * kout].contiguous(), g[:, 2 * kout:].contiguous()
