"""CPU (`-m "not gpu"`): the host side of the range search across ranks (lmi_range_result_pair_counts, lmi_join_range_parts,
lmi_allgather_join_range).  The entry points are exported and bound and the plan enum matches
`_capi.RANGE_JOIN_FIELDS`; the bindings refuse bad arguments before the library is loaded; the join's arithmetic
(csrc/lmi_range_join_plan.h, pure host code) passes its stand-alone self-test under AddressSanitizer + UBSan; and on the oracle alone:
the numpy join (sharded.join_range_parts_numpy) of the reference parts (tests/range_parts_ref.py) equals range_ref on the whole index
for worlds of 2, 3 and 8 ranks and for a rank without buckets, for the tie case spread over three ranks and for the two rows of one
distance on two ranks.  Two-rank gloo worlds run ShardedSearcher's and ReplicaSearcher's range exchange on reference parts.  Every
comparison is on bit patterns."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import range_parts_ref as rpr
import range_ref as rr
import union_parts_ref as upr
import union_ref as ur
from learnedmetricindex_amd import _capi, sharded

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORLDS = ((2, "assign"), (3, "assign"), (3, "gap"), (8, "assign"))
SYMBOLS = (("lmi_range_result_pair_counts", 3), ("lmi_join_range_parts", 10), ("lmi_allgather_join_range", 7),
           ("lmi_range_join_set_geometry", 1), ("lmi_debug_range_join_plan", 2))


def same(got, want, what=""):
    np.testing.assert_array_equal(np.asarray(got[0]), want[0], err_msg=f"lims {what}")
    assert np.asarray(got[0]).dtype == np.int64, what
    np.testing.assert_array_equal(np.asarray(got[2]).view(np.uint32), want[2], err_msg=f"ids {what}")
    np.testing.assert_array_equal(np.asarray(got[1]).view(np.uint32), want[1].view(np.uint32), err_msg=f"dist bits {what}")


def test_range_join_symbols_exported_and_bound():
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in SYMBOLS:
        assert hasattr(L, name), f"{name} is not exported by the built library"
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    with open(os.path.join(ROOT, "include", "lmi_hip.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name, _ in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in lmi_hip.h"
    words = re.findall(r"\bLMI_RANGE_JOIN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", header)
    assert words[-1] == "COUNT" and list(_capi.RANGE_JOIN_FIELDS) == words[:-1]
    assert words[:-1] == ["PARTS", "RUNS", "PIECES", "RESULTS", "LARGEST_PART"]
    for name in ("join_range_parts", "allgather_join_range", "set_range_join_geometry"):
        assert callable(getattr(_capi.Index, name))
    assert callable(_capi.RangeResult.pair_counts) and callable(_capi.range_join_last_plan)
    assert callable(sharded.join_range_parts_numpy)
    for cls in (sharded.ShardedSearcher, sharded.ReplicaSearcher):
        assert callable(cls.range_search)
    assert callable(sharded.ShardedSearcher.range_search_routed)


def test_range_join_argument_errors_raise_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    idx = object.__new__(_capi.Index)   # no handle: nothing below may reach the library
    c = np.zeros((2, 3, 4), np.int32)
    c[0, 0, 0], c[1, 1, 2] = 2, 3
    d = [np.zeros(2, np.float32), np.zeros(3, np.float32)]
    i = [np.zeros(2, np.uint32), np.zeros(3, np.uint32)]
    for bad in (None, c[0], c.astype(np.float32), np.zeros((0, 3, 4), np.int32), np.zeros((65, 1, 1), np.int32),
                np.zeros((2, 3, 0), np.int32), np.zeros((2, 3, 1025), np.int32), c.tolist()):
        with pytest.raises(ValueError):
            idx.join_range_parts(bad, d, i)
    for bad_d, bad_i in ((d[:1], i), (d, i[:1]), (None, i), (d, None), ([d[0], None], i), (d, [None, i[1]]),
                         ([d[0], d[1][:2]], i), (d, [i[0], i[1][:2]]), ([d[0], d[1][None, :]], i),
                         ([d[0], torch.zeros(3)], i), ([d[0], [0.0, 0.0, 0.0]], i)):
        with pytest.raises(ValueError):
            idx.join_range_parts(c, bad_d, bad_i)
    for max_total in (-1, 2.5, None, True):
        with pytest.raises(ValueError):
            idx.join_range_parts(c, d, i, max_total=max_total)
    part = object.__new__(_capi.RangeResult)
    for world in (0, 65, -1, 1.5):
        with pytest.raises(ValueError):
            idx.allgather_join_range(object(), 0, world, part)
    for rank in (-1, 2, 0.5):
        with pytest.raises(ValueError):
            idx.allgather_join_range(object(), rank, 2, part)
    with pytest.raises(ValueError):
        idx.allgather_join_range(None, 0, 2, part)
    with pytest.raises(ValueError):
        idx.allgather_join_range(object(), 0, 2, (c, d, i))   # not a RangeResult
    with pytest.raises(ValueError):
        idx.allgather_join_range(object(), 0, 2, part, max_total=-1)
    for rows in (-1, (1 << 30) + 1, 2.5, None, True):
        with pytest.raises(ValueError):
            idx.set_range_join_geometry(rows)
    q = torch.zeros((3, 8))
    for searcher in (sharded.ShardedSearcher(idx, 0, 1), sharded.ReplicaSearcher(idx, 0, 1)):
        for bad in (None, "far", np.zeros(2, np.float32), np.zeros((3, 1), np.float32)):
            with pytest.raises(ValueError):
                searcher.range_search(q, q, 2, bad)
        with pytest.raises(TypeError):
            searcher.range_search(q, q, 2, 0.5, filter=object())   # there is no filter argument


def test_range_join_plan_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "range_join_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall",
           "-I" + os.path.join(ROOT, "learnedmetricindex_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "range_join_selftest.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "cannot find -lasan" in b.stderr + b.stdout:
        pytest.skip("libasan not installed")
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "range join plan selftest: clean" in r.stdout


def inputs(d=64):
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    return rows, labs, Q


@pytest.mark.parametrize("nb", (1, 3, 8))
@pytest.mark.parametrize("metric", ur.METRICS)
def test_numpy_join_of_reference_parts_equals_the_whole_index(oracle, metric, nb):
    rows, labs, Q = inputs()
    radius, order = rr.recipe_radii(oracle, 64, nb, metric)
    want = rr.recipe_ref(oracle, 64, nb, metric)
    whole = rpr.pair_counts(oracle, rows, labs, order, Q, radius, metric)
    np.testing.assert_array_equal(whole.sum(axis=1), np.diff(want[0]))
    for world, kind in WORLDS:
        owner = upr.owners(world, kind)
        counts, pd, pi = rpr.parts(oracle, rows, labs, order, Q, radius, metric, owner, world)
        what = f"{metric} nb={nb} world={world} {kind}"
        np.testing.assert_array_equal(counts.sum(axis=0), whole, err_msg=f"pair counts {what}")
        same(sharded.join_range_parts_numpy(counts, pd, pi), want, what)
        # not vacuous: the ranks really share queries
        fed = rpr.feeders(counts)
        if nb >= 3:
            assert (fed >= 2).sum() >= 75, (what, int((fed >= 2).sum()))
        if kind == "gap":
            assert counts[1].sum() == 0 and pd[1].size == 0
            same(sharded.join_range_parts_numpy(counts, [pd[0], None, pd[2]], [pi[0], None, pi[2]]), want, what + " (None)")
        if world == 8 and nb >= 3:
            assert fed.max() >= 3, what
    # a world of one reproduces the part
    same(sharded.join_range_parts_numpy(whole[None], [want[1]], [want[2]]), want, "world 1")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_tie_case_across_three_ranks(oracle, metric):
    X, Q, lab, ids, order = ur.tie_case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    owner = np.zeros(ur.L, np.int32)
    owner[list(ur.TIE_BUCKETS)] = (2, 0, 1)   # its three buckets on three different ranks, not in rank order
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    r0 = ur.union_ref(oracle, rows, labs, order[:1], Q[:1], 1, metric)[0][0, 0]
    radius = np.full(ur.NQ, r0, dtype=np.float32)
    want = rr.range_ref(oracle, rows, labs, order, Q, radius, metric)
    assert np.all(np.diff(want[0])[:4] == 40)
    counts, pd, pi = rpr.parts(oracle, rows, labs, order, Q, radius, metric, owner, 3)
    assert np.all(rpr.feeders(counts)[:4] == 3)
    got = sharded.join_range_parts_numpy(counts, pd, pi)
    same(got, want, f"ties {metric}")
    for q in range(4):   # all 40 copies by (rank, row), whoever owns the bucket
        np.testing.assert_array_equal(got[2][got[0][q]: got[0][q + 1]], tied)


def test_two_rows_of_one_distance_on_two_ranks(oracle):
    rows, ids, order, q, owner = upr.collapse_case()
    want = rr.range_ref(oracle, rows, ids, order, q, np.float32(1.0), "ip")
    assert list(want[2]) == [102, 203] and np.all(want[1].view(np.uint32) == np.float32(1.0).view(np.uint32))
    counts, pd, pi = rpr.parts(oracle, rows, ids, order, q, np.float32(1.0), "ip", owner, 2)
    assert counts.tolist() == [[[1, 0]], [[0, 1]]] and list(pi[0]) == [102] and list(pi[1]) == [203]
    got = sharded.join_range_parts_numpy(counts, pd, pi)
    same(got, want, "collapse")   # in (rank, row) order: bucket 0's row first
    swapped = sharded.join_range_parts_numpy(counts[::-1], pd[::-1], pi[::-1])   # the order of the parts does not matter
    same(swapped, want, "collapse, parts swapped")


def test_two_owners_and_negative_counts_raise():
    c = np.zeros((3, 2, 2), np.int32)
    c[0, 1, 0], c[2, 1, 0] = 1, 2
    d, i = [np.zeros(2, np.float32)] * 3, [np.zeros(2, np.uint32)] * 3
    with pytest.raises(ValueError, match=r"query 1, t 0 has results in part 0 and in part 2"):
        sharded.join_range_parts_numpy(c, d, i)
    c[2, 1, 0] = -1
    with pytest.raises(ValueError, match=r"part 2 at query 1, t 0 is negative"):
        sharded.join_range_parts_numpy(c, d, i)
    lims, dd, ii = sharded.join_range_parts_numpy(np.zeros((2, 0, 3), np.int32), [None, None], [None, None])
    assert lims.tolist() == [0] and dd.size == 0 and ii.size == 0


# ---- two-rank gloo worlds: the searchers' range exchange on reference parts, joined by the numpy restatement ----
class _RefResult:
    """Stands in for `_capi.RangeResult` on the CPU."""

    def __init__(self, lims, d, i, counts=None):
        self.lims, self._d, self._i, self._c = np.asarray(lims, np.int64), d, i, counts
        self.total, self.nq = int(self.lims[-1]), len(lims) - 1

    def pair_counts(self):
        return self._c

    def read_into(self, d_t, i_t):
        d_t[: self.total].copy_(torch.from_numpy(np.array(self._d)).view(d_t.dtype))
        i_t[: self.total].copy_(torch.from_numpy(np.array(self._i).view(np.int32)))

    def close(self):
        pass


class _RefIndex:
    """Stands in for `_capi.Index` under the searchers on the CPU: the part from the reference, the join in numpy."""

    def __init__(self, oracle, rows, labs, metric, owned=None, order=None):
        self.oracle, self.rows, self.labs, self.metric, self.owned, self.order = oracle, rows, labs, metric, owned, order

    def scan_range_device(self, qs_t, bo_t, nb, radius, filter=None, filter_of=None, max_total=0):
        assert filter is None and tuple(bo_t.shape) == (qs_t.shape[0], nb) and radius.shape == (qs_t.shape[0],)
        c, lims, d, i = rpr.part(self.oracle, self.rows, self.labs, bo_t.numpy(), qs_t.numpy(), radius, self.metric, self.owned)
        return _RefResult(lims, d, i, c)

    def search_range_device(self, qn_t, qs_t, nb, radius, bo_t=None, filter=None, filter_of=None, max_total=0):
        lo = int(qn_t.storage_offset() // qn_t.shape[1])   # the slice's place in the batch: the stand-in routes by the given order
        order = self.order[lo: lo + qn_t.shape[0]]
        bo_t.copy_(torch.from_numpy(np.array(order)))
        assert radius.shape == (qn_t.shape[0],)
        return _RefResult(*rr.range_ref(self.oracle, self.rows, self.labs, order, qs_t.numpy(), radius, self.metric))

    def join_range_parts(self, counts, dists, ids, max_total=0):
        world, nq, nb = counts.shape
        tot = counts.reshape(world, -1).sum(axis=1)
        lims, d, i = sharded.join_range_parts_numpy(counts, [t.numpy()[: tot[r]] for r, t in enumerate(dists)],
                                                    [t.numpy()[: tot[r]] for r, t in enumerate(ids)])
        return _RefResult(lims, d, i, counts.sum(axis=0))


def _worker(rank, world, port, metric, nb, kind, out_dir):
    sys.path[:0] = [ROOT, HERE]
    from oracle import lmi_oracle as oracle

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        rows, labs, Q = inputs()
        radius, order = rr.recipe_radii(oracle, 64, nb, metric)
        q_t = torch.from_numpy(np.array(Q))
        if kind == "sharded":
            owner = upr.owners(world)
            s = sharded.ShardedSearcher(_RefIndex(oracle, rows, labs, metric, owner == rank), rank, world)
            per, lo, hi = sharded.row_slice(ur.NQ, rank, world)
            bo_loc = torch.full((per, nb), -1, dtype=torch.int32)
            bo_loc[: hi - lo] = torch.from_numpy(order[lo:hi])     # this rank routed its slice of the batch
            lims, d, i, bo = s.range_search_routed(q_t, bo_loc, nb, radius)
        else:
            s = sharded.ReplicaSearcher(_RefIndex(oracle, rows, labs, metric, order=order), rank, world)
            lims, d, i, bo = s.range_search(q_t, q_t, nb, radius)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), lims=lims, d=d.numpy(), i=i.numpy().view(np.uint32), bo=bo.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ("sharded", "replica"))
def test_two_rank_gloo_world_runs_the_range_exchange(oracle, tmp_path, kind):
    from test_sharded_gloo import _free_port

    metric, nb, world = "l2", 3, 2
    mp.spawn(_worker, args=(world, _free_port(), metric, nb, kind, str(tmp_path)), nprocs=world, join=True)
    want = rr.recipe_ref(oracle, 64, nb, metric)
    order = rr.recipe_radii(oracle, 64, nb, metric)[1]
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        np.testing.assert_array_equal(got["bo"], order)
        same((got["lims"], got["d"], got["i"]), want, f"{kind} rank {r}")
