"""GPU (`-m gpu`): the union scan across the ranks of a bucket-sharded index (lmi_scan_union_part, lmi_merge_union_parts,
lmi_allgather_merge_union; include/lmi_hip.h).  One card plays every rank in turn, as in test_gpu_sharded.py: one
handle per rank with its `owned` mask, the all-gather is a stack of the ranks' parts, and the merge must reproduce the single handle's
lmi_scan_union and tests/union_ref.py bit for bit.  The parts themselves are held to tests/union_parts_ref.py, all five planes.
Inputs: union_ref's (N = 6 000, 12 buckets of 0..2 003 rows, 150 queries).  Every comparison is on bit patterns."""
import numpy as np
import pytest
import torch

import union_parts_ref as upr
import union_ref as ur

pytestmark = pytest.mark.gpu

KS = (1, 10, 129, 1024)
WORLDS = (2, 3, 8)


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def same(got, want, what=""):
    d, i, c = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got[:3])
    assert d.shape == want[0].shape and i.shape == want[1].shape and c.shape == want[2].shape, what
    np.testing.assert_array_equal(c.astype(np.int32), want[2], err_msg=f"counts {what}")
    np.testing.assert_array_equal(i.view(np.uint32), np.asarray(want[1]).view(np.uint32), err_msg=f"ids {what}")
    np.testing.assert_array_equal(d.view(np.uint32), np.asarray(want[0]).view(np.uint32), err_msg=f"dist bits {what}")


def same_part(got, want, what=""):
    (gp, gc), (wp, wc) = got, want
    gp = gp.cpu().numpy() if hasattr(gp, "cpu") else gp
    gc = gc.cpu().numpy() if hasattr(gc, "cpu") else gc
    assert gp.dtype == np.int32 and gp.shape == wp.shape, what
    np.testing.assert_array_equal(gc, wc, err_msg=f"counts {what}")
    for plane, name in enumerate(("score", "dist", "id", "rank", "row")):
        np.testing.assert_array_equal(gp[plane], wp[plane], err_msg=f"{name} plane {what}")


def build(capi, X, lab, ids, n_buckets=ur.L, layers=None, owned=None, **kw):
    idx = capi.Index(0, **kw)
    if layers is not None:
        idx.set_mlp(layers)
    idx.set_buckets(np.ascontiguousarray(X), lab, n_buckets, ids=np.ascontiguousarray(ids, dtype=np.uint32),
                    owned=None if owned is None else np.ascontiguousarray(owned, dtype=np.uint8))
    return idx


_idx, _ref, _scores = {}, {}, {}


@pytest.fixture(scope="module")
def index_of(capi):
    """One built index per (d, metric, world, rank) of union_ref.case; world 0: the single handle that holds everything (with a
    random root model, so that lmi_search_union can run on it)."""
    def get(d, metric, world=0, rank=0):
        key = (d, metric, world, rank)
        if key not in _idx:
            X, Q, lab, ids = ur.case(d)
            if world == 0:
                _idx[key] = build(capi, X, lab, ids, layers=ur.layers_for(d, ur.L, 3), metric=metric)
            else:
                owner = upr.owners(world)
                _idx[key] = build(capi, X, lab, ids, owned=owner == rank, metric=metric)
                assert np.array_equal(_idx[key].bucket_sizes(), np.where(owner == rank, ur.SIZES, 0))
        return _idx[key]
    yield get
    for h in _idx.values():
        h.close()
    _idx.clear()


def reference(oracle, d, nb, k, metric):
    """union_ref on union_ref.case(d) and random_order(nb); computed once and shared."""
    key = (d, metric, nb, k)
    if key not in _ref:
        X, Q, lab, ids = ur.case(d)
        rows, labs = ur.buckets_of(X, lab, ids)
        _ref[key] = ur.union_ref(oracle, rows, labs, ur.random_order(nb), Q, k, metric)
        for a in _ref[key]:
            a.setflags(write=False)
    return _ref[key]


def candidates(oracle, d, nb, metric):
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    return upr.Candidates(oracle, rows, labs, ur.random_order(nb), Q, metric, _scores.setdefault((d, metric), {}))


def merged_on_device(idx, parts, k):
    """lmi_merge_union_parts with device pointers on the stacked parts [world, 5, nq, k] (numpy) -> (dists, ids, counts) tensors."""
    world, _, nq, _ = parts.shape
    g = torch.from_numpy(np.ascontiguousarray(parts)).cuda()
    d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    i = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    c = torch.empty((nq,), dtype=torch.int32, device="cuda")
    idx.merge_union_parts(g, world, nq, k, d, i, c)
    torch.cuda.synchronize()
    return d, i, c


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_part_of_an_unsharded_handle(capi, index_of, oracle, d, metric):
    """On a handle that owns every bucket the DIST and ID planes and counts are lmi_scan_union's outputs, and all five planes are the
    reference part: d = 45 element loads, 64 vector loads, 136 a pitch that is no multiple of 32; a random order with -1 slots."""
    nb = 8
    order = ur.random_order(nb)
    assert (order < 0).any()
    idx, Q = index_of(d, metric), ur.case(d)[1]
    cand = candidates(oracle, d, nb, metric)
    for k in (10, 129, 1024):
        part, counts = idx.scan_union_part(Q, order, k)
        plan = capi.union_last_plan()
        same((part[upr.DIST], part[upr.ID], counts), idx.scan_union(Q, order, k), f"against lmi_scan_union d={d} {metric} k={k}")
        # the same geometry, word for word; with host pointers the staged part is 20 Q k bytes where dists + ids are 8 Q k
        assert plan == dict(capi.union_last_plan(), WORKSPACE_BYTES=plan["WORKSPACE_BYTES"])
        assert plan["WORKSPACE_BYTES"] - capi.union_last_plan()["WORKSPACE_BYTES"] == 12 * ur.NQ * k
        same_part((part, counts), cand.part(None, k), f"d={d} {metric} k={k}")
        same((part[upr.DIST], part[upr.ID], counts), reference(oracle, d, nb, k, metric), f"against union_ref d={d} {metric} k={k}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nb", ur.NBS)
@pytest.mark.parametrize("metric", ur.METRICS)
def test_emulated_worlds_merge_to_the_single_handle(index_of, oracle, metric, nb, k):
    """2, 3 and 8 ranks with `owned` masks: every rank's part is the reference part, and the stacked parts merge (device pointers) to
    the single handle's lmi_scan_union and to union_ref.  With nb = 1 most ranks own nothing of what a query visits."""
    d = 64
    order, Q = ur.random_order(nb), ur.case(d)[1]
    want = reference(oracle, d, nb, k, metric)
    single = index_of(d, metric)
    same(single.scan_union(Q, order, k), want, "the single handle")
    cand = candidates(oracle, d, nb, metric)
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(order).cuda()
    for world in WORLDS:
        owner = upr.owners(world)
        parts = torch.empty((world, 5, ur.NQ, k), dtype=torch.int32, device="cuda")
        cnt = torch.empty((world, ur.NQ), dtype=torch.int32, device="cuda")
        for r in range(world):
            index_of(d, metric, world, r).scan_union_part_device(q_t, bo_t, nb, k, parts[r], cnt[r])
            same_part((parts[r], cnt[r]), cand.part(owner == r, k), f"{metric} nb={nb} k={k} world={world} rank={r}")
        got = merged_on_device(index_of(d, metric, world, 0), parts.cpu().numpy(), k)
        same(got, want, f"{metric} nb={nb} k={k} world={world}")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_merge_with_host_pointers(capi, index_of, oracle, metric):
    d, nb, k, world = 64, 8, 129, 3
    order, Q = ur.random_order(nb), ur.case(d)[1]
    parts = np.stack([index_of(d, metric, world, r).scan_union_part(Q, order, k)[0] for r in range(world)])
    md, mi, mc = np.empty((ur.NQ, k), np.float32), np.empty((ur.NQ, k), np.uint32), np.empty((ur.NQ,), np.int32)
    merger = capi.Index(0)   # the merge needs no built index
    try:
        merger.merge_union_parts(parts, world, ur.NQ, k, md, mi, mc)
        same((md, mi, mc), reference(oracle, d, nb, k, metric), f"host pointers {metric}")
        md2, mi2 = np.empty_like(md), np.empty_like(mi)
        merger.merge_union_parts(parts, world, ur.NQ, k, md2, mi2)   # counts declined
        same((md2, mi2, mc), (md, mi, mc), "without counts")
        # a world of one reproduces the part
        merger.merge_union_parts(parts[1:2], 1, ur.NQ, k, md, mi, mc)
        whole, wc = index_of(d, metric, world, 1).scan_union_part(Q, order, k)
        same((md, mi, mc), (whole[upr.DIST], whole[upr.ID], wc), "world 1")
    finally:
        merger.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_tie_case_across_ranks(capi, oracle, metric):
    """40 copies of one vector over three buckets on three different ranks: the copies come first, by (rank, row), whoever owns them."""
    d = 64
    X, Q, lab, ids, order = ur.tie_case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    owner = np.zeros(ur.L, np.int32)
    owner[list(ur.TIE_BUCKETS)] = (2, 0, 1)
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    handles = [build(capi, X, lab, ids, owned=owner == r, metric=metric) for r in range(3)]
    try:
        for k in (10, 25, 100):
            want = ur.union_ref(oracle, rows, labs, order, Q, k, metric)
            parts = np.stack([h.scan_union_part(Q, order, k)[0] for h in handles])
            got = merged_on_device(handles[0], parts, k)
            same(got, want, f"ties {metric} k={k}")
            m = min(k, 40)
            np.testing.assert_array_equal(got[1].cpu().numpy().view(np.uint32)[:4, :m], np.broadcast_to(tied[:m], (4, m)))
    finally:
        for h in handles:
            h.close()


def test_the_collapse_case_across_ranks(capi, oracle):
    """Two scores, 2^-30 and 2^-31, whose distances are both the bits of 1.0f, on different ranks: the greater score comes first, as
    on one handle -- not the lower rank, as a merge by distance would have it."""
    rows, ids, order, q, owner = upr.collapse_case()
    X, lab, idv = np.concatenate(rows), np.repeat(np.arange(2), [r.shape[0] for r in rows]), np.concatenate(ids)
    want = ur.union_ref(oracle, rows, ids, order, q, 2, "ip")
    assert list(want[1][0]) == [203, 102] and np.all(want[0].view(np.uint32) == np.float32(1.0).view(np.uint32))
    single = build(capi, X, lab, idv, n_buckets=2)
    handles = [build(capi, X, lab, idv, n_buckets=2, owned=owner == r) for r in range(2)]
    try:
        same(single.scan_union(q, order, 2), want, "the single handle")
        parts = np.stack([h.scan_union_part(q, order, 2)[0] for h in handles])
        assert parts[0, upr.ID, 0, 0] == 102 and parts[1, upr.ID, 0, 0] == 203
        assert parts[0, upr.DIST, 0, 0] == parts[1, upr.DIST, 0, 0] and parts[0, upr.SCORE, 0, 0] != parts[1, upr.SCORE, 0, 0]
        same(merged_on_device(single, parts, 2), want, "collapse")
    finally:
        for h in handles + [single]:
            h.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_a_rank_that_owns_nothing_a_query_visits(capi, oracle, metric):
    """Rank 1 owns the large bucket alone and no query visits it: its part is padding throughout, and the merged count is
    min(k, total)."""
    d, k = 64, 1024
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    owner = (np.arange(ur.L) == 4).astype(np.int32)
    order = np.tile(np.asarray([2, 8, 0, 9], np.int32), (ur.NQ, 1))   # 33 + 64 + 0 + 65 rows
    handles = [build(capi, X, lab, ids, owned=owner == r, metric=metric) for r in range(2)]
    try:
        parts, counts = zip(*[h.scan_union_part(Q, order, k) for h in handles])
        assert np.all(counts[1] == 0) and np.all(parts[1] == upr.PAD[:, None, None])
        got = merged_on_device(handles[1], np.stack(parts), k)
        assert np.all(got[2].cpu().numpy() == min(k, 33 + 64 + 65))
        same(got, ur.union_ref(oracle, rows, labs, order, Q, k, metric), f"{metric}")
    finally:
        for h in handles:
            h.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_forced_geometry_changes_no_bit_of_a_part(capi, index_of, metric):
    d, nb, k, world = 64, 8, 129, 2
    order, Q = ur.random_order(nb), ur.case(d)[1]
    idx = index_of(d, metric, world, 1)
    try:
        capi.union_set_geometry(0, 0)
        auto = idx.scan_union_part(Q, order, k)
        auto_plan = capi.union_last_plan()
        capi.union_set_geometry(32, 64 << 10)
        forced = idx.scan_union_part(Q, order, k)
        plan = capi.union_last_plan()
    finally:
        capi.union_set_geometry(0, 0)
    same_part(forced, auto, "forced geometry")
    assert auto_plan["GROUPS"] == 1 and plan["GROUPS"] == 5 and plan["QUERY_ROWS"] == 32 and plan["LIST_ROWS"] == 256


@pytest.mark.parametrize("with_comm", (False, True))
def test_sharded_searcher_world1_equals_search_union(capi, index_of, with_comm):
    """ShardedSearcher(world = 1).search(merge="union") is Index.search_union -- without a communicator (no exchange) and with a
    single-rank RCCL communicator (a real ncclAllGather of the part on the handle's stream, then the merge kernel)."""
    from learnedmetricindex_amd.sharded import ShardedSearcher

    d, nb, k, metric = 64, 3, 129, "l2"
    idx, Q = index_of(d, metric), ur.case(d)[1]
    want = idx.search_union(Q, Q, nb, k)
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    comm = idx.comm_init(0, 1, capi.Index.comm_unique_id()) if with_comm else None
    try:
        q_t = torch.from_numpy(np.array(Q)).cuda()
        dd, ii, bo, cc = ShardedSearcher(idx, 0, 1, lib_comm=comm).search(q_t, q_t, nb, k, merge="union")
        torch.cuda.synchronize()
        same((dd, ii, cc), want[:3], f"comm={with_comm}")
        np.testing.assert_array_equal(bo.cpu().numpy(), want[3])
        out = ShardedSearcher(idx, 0, 1, lib_comm=comm).search(q_t, q_t, nb, 10)   # the default path and its three-tuple stand
        assert len(out) == 3 and tuple(out[0].shape) == (ur.NQ, 10)
    finally:
        torch.cuda.synchronize()
        if comm is not None:
            capi.Index.comm_destroy(comm)
        idx.set_stream(0)


@pytest.mark.parametrize("world", (2, 7))
def test_replica_slices_concatenate_to_the_whole_batch(index_of, world):
    from learnedmetricindex_amd.sharded import ReplicaSearcher, row_slice

    d, nb, k, metric = 64, 3, 129, "ip"
    idx, Q = index_of(d, metric), ur.case(d)[1]
    want = idx.search_union(Q, Q, nb, k)
    q_t = torch.from_numpy(np.array(Q)).cuda()
    whole = [t.clone() for t in ReplicaSearcher(idx, 0, 1).search(q_t, q_t, nb, k, merge="union")]
    same((whole[0], whole[1], whole[3]), want[:3], "the whole batch")
    np.testing.assert_array_equal(whole[2].cpu().numpy(), want[3])
    parts = []
    for r in range(world):
        per, lo, hi = row_slice(ur.NQ, r, world)
        if hi > lo:
            parts.append([t.clone() for t in ReplicaSearcher(idx, 0, 1).search(q_t[lo:hi].contiguous(), q_t[lo:hi].contiguous(), nb, k,
                                                                                merge="union")])
    for j in range(4):
        assert torch.equal(torch.cat([p[j] for p in parts]), whole[j])


def test_refusals(capi):
    X, Q, lab, ids = ur.case(64)
    order = ur.random_order(3)
    L = capi.lib()
    idx = build(capi, X, lab, ids)
    part = np.zeros((5, ur.NQ, 1025), np.int32)
    d, i = np.zeros((ur.NQ, 1025), np.float32), np.zeros((ur.NQ, 1025), np.uint32)
    try:
        for k in (0, 1025):   # past the Python checks, at the C ABI
            assert L.lmi_scan_union_part(idx._h, Q.ctypes.data, ur.NQ, order.ctypes.data, 3, k, part.ctypes.data, None, 0) != 0
            assert b"outside [1,1024]" in L.lmi_last_error()
            assert L.lmi_merge_union_parts(idx._h, part.ctypes.data, 1, ur.NQ, k, d.ctypes.data, i.ctypes.data, None, 0) != 0
            assert b"outside [1,1024]" in L.lmi_last_error()
        for world in (0, 65):
            assert L.lmi_merge_union_parts(idx._h, part.ctypes.data, world, ur.NQ, 10, d.ctypes.data, i.ctypes.data, None, 0) != 0
            assert b"outside [1,64]" in L.lmi_last_error()
            assert L.lmi_allgather_merge_union(idx._h, part.ctypes.data, 0, world, part.ctypes.data, ur.NQ, 10, d.ctypes.data, i.ctypes.data,
                                               None) != 0
            assert b"outside [1,64]" in L.lmi_last_error()
        assert L.lmi_scan_union_part(idx._h, Q.ctypes.data, ur.NQ, order.ctypes.data, 3, 10, None, None, 0) != 0
        assert b"NULL" in L.lmi_last_error()
        assert L.lmi_scan_union_part(None, Q.ctypes.data, ur.NQ, order.ctypes.data, 3, 10, part.ctypes.data, None, 0) != 0
        for args in ((None, d.ctypes.data, i.ctypes.data), (part.ctypes.data, None, i.ctypes.data), (part.ctypes.data, d.ctypes.data, None)):
            assert L.lmi_merge_union_parts(idx._h, args[0], 2, ur.NQ, 10, args[1], args[2], None, 0) != 0
            assert b"NULL" in L.lmi_last_error()
        assert L.lmi_merge_union_parts(None, part.ctypes.data, 2, ur.NQ, 10, d.ctypes.data, i.ctypes.data, None, 0) != 0
        assert L.lmi_merge_union_parts(idx._h, part.ctypes.data, 2, -1, 10, d.ctypes.data, i.ctypes.data, None, 0) != 0
        assert L.lmi_allgather_merge_union(idx._h, None, 0, 1, part.ctypes.data, ur.NQ, 10, d.ctypes.data, i.ctypes.data, None) != 0
        assert L.lmi_allgather_merge_union(idx._h, part.ctypes.data, 1, 1, part.ctypes.data, ur.NQ, 10, d.ctypes.data, i.ctypes.data, None) != 0
        # nq == 0 writes nothing and succeeds
        assert L.lmi_scan_union_part(idx._h, Q.ctypes.data, 0, order.ctypes.data, 3, 10, None, None, 0) == 0
        assert L.lmi_merge_union_parts(idx._h, None, 2, 0, 10, None, None, None, 0) == 0
        assert capi.union_last_plan()["GROUPS"] == 0
    finally:
        idx.close()
    idx = capi.Index(0)
    try:
        with pytest.raises(capi.LmiError, match="not built"):
            idx.scan_union_part(Q, order, 10)
    finally:
        idx.close()
    idx = build(capi, X.astype(np.float16).astype(np.float32), lab, ids, storage="f16")
    try:
        with pytest.raises(capi.LmiError, match="row-major"):
            idx.scan_union_part(Q, order, 10)
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_existing_calls_are_unchanged_by_a_part_call(index_of, oracle, metric):
    """lmi_scan_union on the main grid's inputs and an ordinary lmi_search answer the same bits after part calls as before them."""
    d, nb = 64, 8
    idx, Q = index_of(d, metric), ur.case(d)[1]
    order = ur.random_order(nb)
    before_union = {k: idx.scan_union(Q, order, k) for k in KS}
    before = idx.search(Q, Q, 4, 10, want_keys=True)
    for k in KS:
        idx.scan_union_part(Q, order, k)
    for k in KS:
        got = idx.scan_union(Q, order, k)
        same(got, before_union[k], f"scan_union k={k}")
        same(got, reference(oracle, d, nb, k, metric), f"scan_union against union_ref k={k}")
    after = idx.search(Q, Q, 4, 10, want_keys=True)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
