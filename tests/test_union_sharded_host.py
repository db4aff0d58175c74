"""CPU (`-m "not gpu"`): the host side of the union scan across ranks (lmi_scan_union_part, lmi_merge_union_parts,
lmi_allgather_merge_union).  The three entry points are exported and bound; the bindings refuse bad arguments before
the library is loaded; and on the oracle alone: the numpy merge (sharded.merge_union_parts_numpy) of the reference parts
(tests/union_parts_ref.py) equals union_ref on the whole index for worlds of 1, 2, 3 and 8 ranks, for a rank without buckets, for the
tie case spread over three ranks and for the case in which two scores collapse into one distance -- where a merge by distance fails.
A two-rank gloo world runs ShardedSearcher's union exchange on reference parts.  Every comparison is on bit patterns."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import union_parts_ref as upr
import union_ref as ur
from learnedmetricindex_amd import _capi, sharded

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORLDS = ((1, "assign"), (2, "assign"), (3, "assign"), (8, "assign"), (3, "gap"))
KS = (1, 10, 129, 1024)


def same(got, want, what=""):
    np.testing.assert_array_equal(np.asarray(got[2], np.int32), want[2], err_msg=f"counts {what}")
    np.testing.assert_array_equal(np.asarray(got[1]).view(np.uint32), want[1], err_msg=f"ids {what}")
    np.testing.assert_array_equal(np.asarray(got[0]).view(np.uint32), want[0].view(np.uint32), err_msg=f"dist bits {what}")


def test_union_part_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in (("lmi_scan_union_part", 9), ("lmi_merge_union_parts", 9), ("lmi_allgather_merge_union", 10)):
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    assert _capi.UNION_PART_PLANES == 5 == upr.PLANES
    assert (_capi.UPART_SCORE, _capi.UPART_DIST, _capi.UPART_ID, _capi.UPART_RANK, _capi.UPART_ROW) == (0, 1, 2, 3, 4)
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = fh.read()
    assert "#define LMI_UNION_PART_PLANES 5" in header
    assert "enum { LMI_UPART_SCORE = 0, LMI_UPART_DIST, LMI_UPART_ID, LMI_UPART_RANK, LMI_UPART_ROW };" in header
    for name in ("scan_union_part", "scan_union_part_device", "merge_union_parts", "allgather_merge_union"):
        assert callable(getattr(_capi.Index, name))
    assert callable(sharded.merge_union_parts_numpy)


def test_union_part_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    idx = object.__new__(_capi.Index)   # no handle: nothing below may reach the library
    q, bo = np.zeros((3, 8), np.float32), np.zeros((3, 2), np.int32)
    for k in (0, 1025, -1, 2.5):
        with pytest.raises(ValueError):
            idx.scan_union_part(q, bo, k)
        with pytest.raises(ValueError):
            idx.merge_union_parts(np.zeros((2, 5, 3, 4), np.int32), 2, 3, k, q, q)
    for bad_q, bad_bo in ((q[0], bo), (q, bo[0]), (None, bo), (q, None), (q, bo[:2]), (q, np.zeros((3, 0), np.int32))):
        with pytest.raises(ValueError):
            idx.scan_union_part(bad_q, bad_bo, 10)
    with pytest.raises(ValueError):
        idx.scan_union_part_device(q, bo, 2, 0, np.zeros((5, 3, 1), np.int32))
    with pytest.raises(ValueError):
        idx.scan_union_part_device(q, bo, 2, 4, np.zeros((3, 3, 4), np.int32))   # not five planes
    parts, d, i = np.zeros((2, 5, 3, 4), np.int32), np.zeros((3, 4), np.float32), np.zeros((3, 4), np.uint32)
    for world in (0, 65, -1, 1.5):
        with pytest.raises(ValueError):
            idx.merge_union_parts(parts, world, 3, 4, d, i)
        with pytest.raises(ValueError):
            idx.allgather_merge_union(object(), 0, world, parts[0], d, i)
    with pytest.raises(ValueError):
        idx.merge_union_parts(parts, 2, -1, 4, d, i)
    with pytest.raises(ValueError):
        idx.merge_union_parts(parts, 3, 3, 4, d, i)   # not world * 5 * nq * k words
    for a, b, c in ((None, d, i), (parts, None, i), (parts, d, None)):
        with pytest.raises(ValueError):
            idx.merge_union_parts(a, 2, 3, 4, b, c)
    for rank in (-1, 2):
        with pytest.raises(ValueError):
            idx.allgather_merge_union(object(), rank, 2, parts[0], d, i)
    with pytest.raises(ValueError):
        idx.allgather_merge_union(None, 0, 2, parts[0], d, i)
    with pytest.raises(ValueError):
        idx.allgather_merge_union(object(), 0, 2, parts, d, i)   # a stack of parts, not one part
    for searcher in (sharded.ShardedSearcher(idx, 0, 1), sharded.ReplicaSearcher(idx, 0, 1)):
        with pytest.raises(ValueError, match="merge"):
            searcher.search(None, None, 2, 10, merge="best")


def gather(cand, owner, world, k):
    """[world, 5, nq, k]: the ranks' reference parts as the all-gather stacks them."""
    return np.stack([cand.part(owner == r, k)[0] for r in range(world)])


_scores = {}


def candidates(oracle, metric, nb):
    X, Q, lab, ids = ur.case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    return upr.Candidates(oracle, rows, labs, ur.random_order(nb), Q, metric, _scores.setdefault(metric, {})), rows, labs, Q


@pytest.mark.parametrize("nb", (1, 3, 8))
@pytest.mark.parametrize("metric", ur.METRICS)
def test_numpy_merge_of_reference_parts_equals_the_whole_index(oracle, metric, nb):
    cand, rows, labs, Q = candidates(oracle, metric, nb)
    order = cand.order
    for k in KS:
        want = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
        same(cand.whole(k), want, f"the reference's own whole-index cut {metric} nb={nb} k={k}")
        for world, kind in WORLDS:
            owner = upr.owners(world, kind)
            assert kind != "gap" or not (owner == 1).any()
            assert kind == "gap" or set(np.unique(owner)) == set(range(world))
            g = gather(cand, owner, world, k)
            same(sharded.merge_union_parts_numpy(g), want, f"{metric} nb={nb} k={k} world={world} {kind}")
            if kind == "gap":   # the rank without buckets hands on padding alone
                assert np.all(g[1] == upr.PAD[:, None, None])
    # a world of one reproduces the part
    part, counts = cand.part(None, 129)
    same(sharded.merge_union_parts_numpy(part[None]), (part[upr.DIST].view(np.float32), part[upr.ID].view(np.uint32), counts), "world 1")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_a_reference_part_is_union_ref_on_the_owned_buckets(oracle, metric):
    """The direct statement of a part's DIST, ID and counts: union_ref on the order with the other ranks' buckets struck out."""
    nb, k = 8, 129
    cand, rows, labs, Q = candidates(oracle, metric, nb)
    owner = upr.owners(3)
    for r in range(3):
        part, counts = cand.part(owner == r, k)
        want = ur.union_ref(oracle, rows, labs, upr.struck_order(cand.order, owner == r), Q, k, metric)
        same((part[upr.DIST].view(np.float32), part[upr.ID], counts), want, f"rank {r}")
        pad = np.arange(k)[None, :] >= counts[:, None]
        for plane in range(upr.PLANES):
            assert np.all(part[plane][pad] == upr.PAD[plane])
        real = ~pad
        assert np.all(part[upr.RANK][real] >= 0) and np.all(part[upr.RANK][real] < nb) and np.all(part[upr.ROW][real] >= 0)
        # (rank, row) names the object: the id stored at that row of the bucket at that rank
        for q in (4, 77, 149):
            for j in range(0, int(counts[q]), 17):
                b = cand.order[q, part[upr.RANK, q, j]]
                assert owner[b] == r and labs[b][part[upr.ROW, q, j]] == part[upr.ID, q, j].view(np.uint32)


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_tie_case_across_three_ranks(oracle, metric):
    X, Q, lab, ids, order = ur.tie_case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    owner = np.zeros(ur.L, np.int32)
    owner[list(ur.TIE_BUCKETS)] = (2, 0, 1)   # its three buckets on three different ranks, not in rank order
    cand = upr.Candidates(oracle, rows, labs, order, Q, metric)
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    for k in (10, 25, 100):
        want = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
        got = sharded.merge_union_parts_numpy(gather(cand, owner, 3, k))
        same(got, want, f"ties {metric} k={k}")
        m = min(k, 40)
        np.testing.assert_array_equal(got[1][:4, :m], np.broadcast_to(tied[:m], (4, m)))   # by (rank, row), whoever owns the bucket


def merge_by_distance(gathered):
    """What a merge by (distance, rank, row) would select: lmi_merge_gathered's kind of order on a part's planes."""
    world, _, nq, k = gathered.shape
    flat = lambda p: np.ascontiguousarray(gathered[:, p].transpose(1, 0, 2)).reshape(nq, world * k)
    d = flat(upr.DIST).view(np.float32).astype(np.float64)
    order = np.lexsort((flat(upr.ROW).view(np.uint32), flat(upr.RANK).view(np.uint32), d), axis=1)[:, :k]
    return np.take_along_axis(flat(upr.ID).view(np.uint32), order, 1)


def test_two_scores_that_collapse_into_one_distance(oracle):
    rows, ids, order, q, owner = upr.collapse_case()
    k = 2
    for b, x0 in ((0, 2.0 ** -31), (1, 2.0 ** -30)):   # on the oracle: the scores differ, both distances are the bits of 1.0f
        S, I = oracle.knn_ip(q, rows[b], 1)
        assert S[0, 0] == np.float32(x0) and I[0, 0] == 2 + b
        assert (ur.ONE - S).astype(np.float32).view(np.uint32)[0, 0] == np.float32(1.0).view(np.uint32)
    want = ur.union_ref(oracle, rows, ids, order, q, k, "ip")
    assert np.all(want[0].view(np.uint32) == np.float32(1.0).view(np.uint32)) and list(want[1][0]) == [203, 102] and want[2][0] == 2
    cand = upr.Candidates(oracle, rows, ids, order, q, "ip")
    g = gather(cand, owner, 2, k)
    assert g[0, upr.ID, 0, 0] == 102 and g[1, upr.ID, 0, 0] == 203            # each rank's best is its near row
    same(sharded.merge_union_parts_numpy(g), want, "collapse")               # bucket 1's row first: the greater score
    assert list(merge_by_distance(g)[0]) == [102, 203]                        # by distance: bucket 0's row first -- the wrong order


# ---- a two-rank gloo world: ShardedSearcher's union exchange on reference parts, merged by the numpy restatement ----
class _RefIndex:
    """Stands in for `_capi.Index` under ShardedSearcher on the CPU: the part from the reference, the merge in numpy."""

    def __init__(self, cand, owned):
        self.cand, self.owned = cand, owned

    def scan_union_part_device(self, qs_t, bo_t, nb, k, part_t, counts_t=None):
        assert np.array_equal(bo_t.numpy(), self.cand.order) and tuple(part_t.shape) == (5, self.cand.nq, k)
        part, counts = self.cand.part(self.owned, k)
        part_t.copy_(torch.from_numpy(part))
        if counts_t is not None:
            counts_t.copy_(torch.from_numpy(counts))

    def merge_union_parts(self, parts, world, nq, k, out_d, out_i, counts=None):
        assert tuple(parts.shape) == (world, 5, nq, k)
        d, i, c = sharded.merge_union_parts_numpy(parts.numpy())
        out_d.copy_(torch.from_numpy(d))
        out_i.copy_(torch.from_numpy(i.view(np.int32)))
        counts.copy_(torch.from_numpy(c))


def _worker(rank, world, port, metric, nb, k, out_dir):
    sys.path[:0] = [ROOT, HERE]
    from oracle import lmi_oracle as oracle

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        X, Q, lab, ids = ur.case(64)
        rows, labs = ur.buckets_of(X, lab, ids)
        order = ur.random_order(nb)
        owner = upr.owners(world)
        cand = upr.Candidates(oracle, rows, labs, order, Q, metric)
        s = sharded.ShardedSearcher(_RefIndex(cand, owner == rank), rank, world)
        per, lo, hi = sharded.row_slice(ur.NQ, rank, world)
        bo_loc = torch.full((per, nb), -1, dtype=torch.int32)
        bo_loc[: hi - lo] = torch.from_numpy(order[lo:hi])     # this rank routed its slice of the batch
        d, i, bo, c = s.search_routed(torch.from_numpy(np.array(Q)), bo_loc, nb, k, merge="union")
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), d=d.numpy(), i=i.numpy().view(np.uint32), bo=bo.numpy(), c=c.numpy())
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_world_runs_the_union_exchange(oracle, tmp_path):
    from test_sharded_gloo import _free_port

    metric, nb, k, world = "l2", 3, 129, 2
    mp.spawn(_worker, args=(world, _free_port(), metric, nb, k, str(tmp_path)), nprocs=world, join=True)
    X, Q, lab, ids = ur.case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    order = ur.random_order(nb)
    want = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        np.testing.assert_array_equal(got["bo"], order)
        same((got["d"], got["i"], got["c"]), want, f"rank {r}")
