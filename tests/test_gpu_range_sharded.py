"""GPU (`-m gpu`): the range search across the ranks of a bucket-sharded index (lmi_range_result_pair_counts, lmi_join_range_parts,
lmi_allgather_join_range; include/lmi_hip.h).  One card plays every rank in turn, as in test_gpu_union_sharded.py:
one handle per rank with its `owned` mask, every rank runs lmi_scan_range on the same queries, order and radius, and the join of the
parts must reproduce the single handle's lmi_scan_range and tests/range_ref.py bit for bit -- lims, the distances' bit patterns, the
ids.  Inputs: union_ref's (N = 6 000, 12 buckets of 0..2 003 rows, 150 queries) with range_ref's radius recipe."""
import ctypes

import numpy as np
import pytest
import torch

import range_parts_ref as rpr
import range_ref as rr
import union_filter_ref as fr
import union_parts_ref as upr
import union_ref as ur

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
WORLDS = ((2, "assign"), (3, "assign"), (3, "gap"), (8, "assign"))


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def same(got, want, what=""):
    lims, d, i = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got[:3])
    np.testing.assert_array_equal(lims, want[0], err_msg=f"lims {what}")
    assert lims.dtype == np.int64 and d.shape == i.shape == (int(want[0][-1]),), what
    np.testing.assert_array_equal(i.view(np.uint32), np.asarray(want[2]).view(np.uint32), err_msg=f"ids {what}")
    np.testing.assert_array_equal(d.view(np.uint32), np.asarray(want[1]).view(np.uint32), err_msg=f"dist bits {what}")


def build(capi, X, lab, ids, n_buckets=ur.L, layers=None, owned=None, **kw):
    idx = capi.Index(0, **kw)
    if layers is not None:
        idx.set_mlp(layers)
    idx.set_buckets(np.ascontiguousarray(X), lab, n_buckets, ids=np.ascontiguousarray(ids, dtype=np.uint32),
                    owned=None if owned is None else np.ascontiguousarray(owned, dtype=np.uint8))
    return idx


_idx = {}


@pytest.fixture(scope="module")
def index_of(capi):
    """One built index per (d, metric, world, kind, rank) of union_ref.case; world 0: the single handle that holds everything (with a
    random root model, so that lmi_search_range can run on it)."""
    def get(d, metric, world=0, kind="assign", rank=0):
        key = (d, metric, world, kind, rank)
        if key not in _idx:
            X, Q, lab, ids = ur.case(d)
            if world == 0:
                _idx[key] = build(capi, X, lab, ids, layers=ur.layers_for(d, ur.L, 3), metric=metric)
            else:
                owner = upr.owners(world, kind)
                _idx[key] = build(capi, X, lab, ids, owned=owner == rank, metric=metric)
                assert np.array_equal(_idx[key].bucket_sizes(), np.where(owner == rank, ur.SIZES, 0))
        return _idx[key]
    yield get
    for h in _idx.values():
        h.close()
    _idx.clear()


def rank_parts(handles, Q, order, radius, **kw):
    """Every rank's lmi_scan_range (device pointers) -> (counts i32[world, nq, nb], [dists tensor per rank], [ids tensor per rank])."""
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(order)).cuda()
    counts, ds, is_ = [], [], []
    for h in handles:
        with h.scan_range_device(q_t, bo_t, order.shape[1], radius, **kw) as res:
            c = res.pair_counts()
            assert c.dtype == np.int32 and c.shape == order.shape and np.array_equal(c.sum(axis=1), np.diff(res.lims))
            d = torch.empty(res.total, dtype=torch.float32, device="cuda")
            i = torch.empty(res.total, dtype=torch.int32, device="cuda")
            if res.total:
                res.read_into(d, i)
            counts.append(c), ds.append(d), is_.append(i)
    return np.stack(counts), ds, is_


def joined(idx, counts, ds, is_, max_total=0):
    """lmi_join_range_parts -> ((lims, dists, ids), pair counts)."""
    with idx.join_range_parts(counts, ds, is_, max_total) as res:
        return (res.lims,) + res.read(), res.pair_counts()


def inputs(d=64):
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    return rows, labs, Q


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", ur.DIMS)
def test_pair_counts_of_an_unsharded_handle(index_of, oracle, d, metric):
    """The counts a result keeps are the reference's per-(query, t) counts, and their rows sum to lims' steps."""
    nb = 3
    rows, labs, Q = inputs(d)
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    want = rpr.pair_counts(oracle, rows, labs, order, Q, radius, metric)
    counts, ds, is_ = rank_parts([index_of(d, metric)], Q, order, radius)
    np.testing.assert_array_equal(counts[0], want)
    lims = rr.recipe_ref(oracle, d, nb, metric)[0]
    np.testing.assert_array_equal(counts[0].sum(axis=1), np.diff(lims))
    assert (counts[0][order < 0] == 0).all() and (counts[0] > 0).sum() >= 100


@pytest.mark.parametrize("nb", ur.NBS)
@pytest.mark.parametrize("metric", ur.METRICS)
def test_emulated_worlds_join_to_the_single_handle(capi, index_of, oracle, metric, nb):
    """2, 3 and 8 ranks with `owned` masks, and 3 ranks of which rank 1 owns nothing: the ranks' parts, joined with device pointers,
    are the single handle's lmi_scan_range and range_ref; the joined pair counts are the single handle's."""
    d = 64
    Q = ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    want = rr.recipe_ref(oracle, d, nb, metric)
    single = index_of(d, metric)
    same(single.scan_range(Q, order, radius), want, "the single handle")
    whole = rank_parts([single], Q, order, radius)[0][0]
    for world, kind in WORLDS:
        what = f"{metric} nb={nb} world={world} {kind}"
        handles = [index_of(d, metric, world, kind, r) for r in range(world)]
        counts, ds, is_ = rank_parts(handles, Q, order, radius)
        got, pc = joined(handles[0], counts, ds, is_)
        same(got, want, what)
        np.testing.assert_array_equal(pc, whole, err_msg=f"pair counts {what}")
        plan = capi.range_join_last_plan()
        assert plan["PARTS"] == world and plan["RESULTS"] == want[0][-1] and plan["RUNS"] == (whole > 0).sum()
        assert plan["LARGEST_PART"] == counts.reshape(world, -1).sum(axis=1).max()
        assert plan["PIECES"] == (-(-whole.astype(np.int64) // 4096)).sum()
        fed = rpr.feeders(counts)
        if nb >= 3:
            assert (fed >= 2).sum() >= 75, what
        if kind == "gap":
            assert counts[1].sum() == 0


@pytest.mark.parametrize("d,metric", ((45, "ip"), (136, "l2")))
def test_other_dimensions(index_of, oracle, d, metric):
    nb, world = 3, 3
    Q = ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    handles = [index_of(d, metric, world, "assign", r) for r in range(world)]
    counts, ds, is_ = rank_parts(handles, Q, order, radius)
    got, _ = joined(handles[1], counts, ds, is_)
    same(got, rr.recipe_ref(oracle, d, nb, metric), f"d={d} {metric}")
    same(got, index_of(d, metric).scan_range(Q, order, radius), f"against the single handle d={d} {metric}")


@pytest.mark.parametrize("metric", ur.METRICS)
def test_join_with_host_pointers_and_an_empty_part_as_null(capi, index_of, oracle, metric):
    d, nb, world = 64, 8, 3
    Q = ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    want = rr.recipe_ref(oracle, d, nb, metric)
    handles = [index_of(d, metric, world, "gap", r) for r in range(world)]
    counts, ds, is_ = rank_parts(handles, Q, order, radius)
    assert counts[1].sum() == 0 and ds[1].numel() == 0
    joiner = capi.Index(0)   # the join needs no built index
    try:
        hd, hi = [t.cpu().numpy() for t in ds], [t.cpu().numpy().view(np.uint32) for t in is_]
        same(joined(joiner, counts, hd, hi)[0], want, f"host pointers {metric}")
        hd[1] = hi[1] = None
        same(joined(joiner, counts, hd, hi)[0], want, f"host pointers, NULL part {metric}")
        ds[1] = is_[1] = None
        same(joined(joiner, counts, ds, is_)[0], want, f"device pointers, NULL part {metric}")
        # a world of one reproduces the part
        w = rank_parts([index_of(d, metric)], Q, order, radius)
        same(joined(joiner, w[0], w[1], w[2])[0], want, "world 1")
    finally:
        joiner.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_forced_piece_rows_change_no_bit(capi, index_of, oracle, metric):
    """Query 4 at +inf has a run above 1 024 results: pieces of 1, 64 and 100 cut it (and every run of 10 or 100) at seams that are
    no multiple of anything; the bits stay those of the default, and the plan words report the pieces."""
    d, nb, world = 64, 3, 3
    rows_, labs, Q = inputs(d)
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    radius = np.array(radius)
    radius[4] = INF
    want = rr.range_ref(oracle, rows_, labs, order, Q, radius, metric)
    handles = [index_of(d, metric, world, "assign", r) for r in range(world)]
    counts, ds, is_ = rank_parts(handles, Q, order, radius)
    n = counts.sum(axis=0).astype(np.int64)
    assert n[4].max() > 1024 and (n[4] > 0).sum() >= 2   # bucket 4's 2 003 rows, and another bucket behind it
    try:
        for rows in (1, 64, 100, 0):
            capi.Index.set_range_join_geometry(rows)
            same(joined(handles[0], counts, ds, is_)[0], want, f"piece_rows={rows} {metric}")
            plan = capi.range_join_last_plan()
            assert plan["PIECES"] == (-(-n // (rows or 4096))).sum() and plan["RUNS"] == (n > 0).sum() and plan["RESULTS"] == n.sum()
            if rows == 1:
                assert plan["PIECES"] == plan["RESULTS"]
    finally:
        capi.Index.set_range_join_geometry(0)


@pytest.mark.parametrize("rows", (64, 0))
def test_runs_of_exactly_piece_rows_and_one_more(capi, rows):
    """Synthetic parts (the join needs no index): runs of piece_rows - 1, piece_rows, piece_rows + 1 and 2 * piece_rows + 1 results,
    alternating between two parts, against the numpy join: a piece that wrote one result past its end would overwrite the first
    result of the next run, which belongs to the other part and holds other bits."""
    from learnedmetricindex_amd.sharded import join_range_parts_numpy

    pr = rows or 4096
    lens = np.asarray([pr - 1, pr, pr + 1, 0, 2 * pr + 1, 1, pr, pr + 1], np.int32).reshape(2, 4)
    counts = np.zeros((2, 2, 4), np.int32)
    owner = (np.arange(8).reshape(2, 4) % 2)
    for r in range(2):
        counts[r] = np.where(owner == r, lens, 0)
    rs = np.random.RandomState(3)
    ds = [rs.randn(int(counts[r].sum())).astype(np.float32) for r in range(2)]
    is_ = [rs.randint(0, 2 ** 32, int(counts[r].sum()), dtype=np.uint64).astype(np.uint32) for r in range(2)]
    want = join_range_parts_numpy(counts, ds, is_)
    idx = capi.Index(0)
    try:
        capi.Index.set_range_join_geometry(rows)
        got, pc = joined(idx, counts, ds, is_)
        same(got, want, f"host, piece_rows={pr}")
        np.testing.assert_array_equal(pc, lens)
        assert capi.range_join_last_plan()["PIECES"] == (-(-lens.astype(np.int64) // pr)).sum() == 1 + 1 + 2 + 0 + 3 + 1 + 1 + 2
        dt = [torch.from_numpy(a).cuda() for a in ds]
        it = [torch.from_numpy(a.view(np.int32)).cuda() for a in is_]
        same(joined(idx, counts, dt, it)[0], want, f"device, piece_rows={pr}")
    finally:
        capi.Index.set_range_join_geometry(0)
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_the_tie_case_across_ranks(capi, oracle, metric):
    """40 copies of one vector over three buckets on three different ranks, radius = their distance: all 40, by (rank, row)."""
    d = 64
    X, Q, lab, ids, order = ur.tie_case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    owner = np.zeros(ur.L, np.int32)
    owner[list(ur.TIE_BUCKETS)] = (2, 0, 1)
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    r0 = ur.union_ref(oracle, rows, labs, order[:1], Q[:1], 1, metric)[0][0, 0]
    radius = np.full(ur.NQ, r0, dtype=np.float32)
    want = rr.range_ref(oracle, rows, labs, order, Q, radius, metric)
    assert np.all(np.diff(want[0])[:4] == 40)
    handles = [build(capi, X, lab, ids, owned=owner == r, metric=metric) for r in range(3)]
    try:
        counts, ds, is_ = rank_parts(handles, Q, order, radius)
        assert np.all(rpr.feeders(counts)[:4] == 3)
        got, _ = joined(handles[0], counts, ds, is_)
        same(got, want, f"ties {metric}")
        for q in range(4):
            np.testing.assert_array_equal(got[2][got[0][q]: got[0][q + 1]], tied)
    finally:
        for h in handles:
            h.close()


def test_the_collapse_case_across_ranks(capi, oracle):
    """Two rows whose distances are both the bits of 1.0f, on different ranks, radius 1.0f: both, in (rank, row) order -- bucket 0's
    first, whichever part comes first."""
    rows, ids, order, q, owner = upr.collapse_case()
    X, lab, idv = np.concatenate(rows), np.repeat(np.arange(2), [r.shape[0] for r in rows]), np.concatenate(ids)
    want = rr.range_ref(oracle, rows, ids, order, q, np.float32(1.0), "ip")
    assert list(want[2]) == [102, 203] and np.all(want[1].view(np.uint32) == np.float32(1.0).view(np.uint32))
    handles = [build(capi, X, lab, idv, n_buckets=2, owned=owner == r) for r in range(2)]
    try:
        counts, ds, is_ = rank_parts(handles, q, order, np.float32(1.0))
        assert counts.tolist() == [[[1, 0]], [[0, 1]]]
        same(joined(handles[0], counts, ds, is_)[0], want, "collapse")
        same(joined(handles[0], counts[::-1], ds[::-1], is_[::-1])[0], want, "collapse, parts swapped")
    finally:
        for h in handles:
            h.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_forced_union_geometry_on_the_rank_calls_changes_nothing(capi, index_of, oracle, metric):
    d, nb, world = 64, 8, 2
    Q = ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    handles = [index_of(d, metric, world, "assign", r) for r in range(world)]
    try:
        capi.union_set_geometry(0, 0)
        auto = rank_parts(handles, Q, order, radius)
        assert capi.range_last_plan()["GROUPS"] == 1
        capi.union_set_geometry(32, 256 << 10)
        forced = rank_parts(handles, Q, order, radius)
        assert capi.range_last_plan()["GROUPS"] == 5
    finally:
        capi.union_set_geometry(0, 0)
    np.testing.assert_array_equal(forced[0], auto[0])
    for r in range(world):
        assert torch.equal(forced[1][r].view(torch.int32), auto[1][r].view(torch.int32)) and torch.equal(forced[2][r], auto[2][r])
    same(joined(handles[0], *forced)[0], rr.recipe_ref(oracle, d, nb, metric), f"forced geometry {metric}")


def test_filtered_parts_join_to_the_filtered_whole(capi, index_of, oracle):
    """The same keep list (the even ids) as a filter on every rank's handle and on the whole handle."""
    d, nb, world, metric = 64, 3, 3, "l2"
    rows, labs, Q = inputs(d)
    order = ur.random_order(nb)
    keep = [fr.filter_lists(d)[0]]
    allowed = fr.allowed_rows(keep, [fr.KEEP], labs)
    want = rr.range_ref(oracle, rows, labs, order, Q, INF, metric, allowed)
    total = rr.range_ref(oracle, rows, labs, order, Q, INF, metric)[0][-1]
    assert 0 < want[0][-1] < total
    single = index_of(d, metric)
    handles = [index_of(d, metric, world, "assign", r) for r in range(world)]
    filters = [capi.Filter(h, keep, [fr.KEEP]) for h in handles + [single]]
    try:
        same(single.scan_range(Q, order, INF, filter=filters[-1]), want, "the single handle, filtered")
        q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(order).cuda()
        counts, ds, is_ = [], [], []
        for h, f in zip(handles, filters):
            with h.scan_range_device(q_t, bo_t, nb, INF, filter=f) as res:
                counts.append(res.pair_counts())
                a, b = res.read()
                ds.append(a), is_.append(b)
        same(joined(handles[0], np.stack(counts), ds, is_)[0], want, "filtered parts")
    finally:
        for f in filters:
            f.close()


def test_max_total_and_the_handle_afterwards(capi, index_of, oracle):
    d, nb, world, metric = 64, 3, 2, "ip"
    Q = ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    want = rr.recipe_ref(oracle, d, nb, metric)
    total = int(want[0][-1])
    handles = [index_of(d, metric, world, "assign", r) for r in range(world)]
    single = index_of(d, metric)
    counts, ds, is_ = rank_parts(handles, Q, order, radius)
    before = (single.search(Q, Q, 4, 10), single.scan_union(Q, order, 10), single.scan_range(Q, order, radius))
    same(joined(single, counts, ds, is_, max_total=total)[0], want, "max_total at the total")
    with pytest.raises(capi.LmiError, match=rf"lmi_join_range_parts: more than max_total = {total - 1} results: the parts hold {total}"):
        single.join_range_parts(counts, ds, is_, max_total=total - 1)
    assert capi.range_join_last_plan() == dict.fromkeys(capi.RANGE_JOIN_FIELDS, 0)
    after = (single.search(Q, Q, 4, 10), single.scan_union(Q, order, 10), single.scan_range(Q, order, radius))
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    same(joined(single, counts, ds, is_)[0], want, "after the refusal")


@pytest.mark.parametrize("with_comm", (False, True))
def test_sharded_searcher_world1_equals_search_range(capi, index_of, oracle, with_comm):
    """ShardedSearcher(world = 1).range_search is Index.search_range -- without a communicator (no exchange) and with a single-rank
    RCCL communicator (two real ncclAllGather calls on the handle's stream, then the join kernel)."""
    from learnedmetricindex_amd.sharded import ShardedSearcher

    d, nb, metric = 64, 3, "l2"
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius = rr.recipe_radii(oracle, d, nb, metric)[0]
    want = idx.search_range(Q, Q, nb, radius)
    assert want[0][-1] > 1000
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    comm = idx.comm_init(0, 1, capi.Index.comm_unique_id()) if with_comm else None
    try:
        q_t = torch.from_numpy(np.array(Q)).cuda()
        lims, dd, ii, bo = ShardedSearcher(idx, 0, 1, lib_comm=comm).range_search(q_t, q_t, nb, radius)
        torch.cuda.synchronize()
        same((lims, dd, ii), want[:3], f"comm={with_comm}")
        np.testing.assert_array_equal(bo.cpu().numpy(), want[3])
        if with_comm:
            plan = capi.range_join_last_plan()
            assert plan["PARTS"] == 1 and plan["RESULTS"] == plan["LARGEST_PART"] == want[0][-1]
            with pytest.raises(capi.LmiError, match="max_total"):
                ShardedSearcher(idx, 0, 1, lib_comm=comm).range_search(q_t, q_t, nb, radius, max_total=int(want[0][-1]) - 1)
        one = ShardedSearcher(idx, 0, 1, lib_comm=comm).range_search(q_t, q_t, nb, 0.5)   # a scalar radius serves every query
        same(one[:3], idx.search_range(Q, Q, nb, 0.5)[:3], "scalar radius")
    finally:
        torch.cuda.synchronize()
        if comm is not None:
            capi.Index.comm_destroy(comm)
        idx.set_stream(0)


@pytest.mark.parametrize("world", (1, 2, 3))
def test_replica_slices_concatenate_to_the_whole_batch(index_of, oracle, world):
    from learnedmetricindex_amd.sharded import ReplicaSearcher, row_slice

    d, nb, metric = 64, 3, "ip"
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius = rr.recipe_radii(oracle, d, nb, metric)[0]
    want = idx.search_range(Q, Q, nb, radius)
    q_t = torch.from_numpy(np.array(Q)).cuda()
    whole = ReplicaSearcher(idx, 0, 1).range_search(q_t, q_t, nb, radius)
    same(whole[:3], want[:3], "the whole batch")
    np.testing.assert_array_equal(whole[3].cpu().numpy(), want[3])
    lims, ds, is_, bos = [0], [], [], []
    for r in range(world):
        per, lo, hi = row_slice(ur.NQ, r, world)
        if hi > lo:
            l, dd, ii, bo = ReplicaSearcher(idx, 0, 1).range_search(q_t[lo:hi].contiguous(), q_t[lo:hi].contiguous(), nb, radius[lo:hi])
            lims += list(lims[-1] + l[1:])
            ds.append(dd), is_.append(ii), bos.append(bo)
    same((np.asarray(lims, np.int64), torch.cat(ds), torch.cat(is_)), want[:3], f"world={world}")
    assert torch.equal(torch.cat(bos), whole[3])


def test_refusals(capi, index_of, oracle):
    d, nb, world, metric = 64, 3, 2, "ip"
    Q = ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    handles = [index_of(d, metric, world, "assign", r) for r in range(world)]
    counts, ds, is_ = rank_parts(handles, Q, order, radius)
    L, h = capi.lib(), handles[0]._h
    vp = ctypes.c_void_p
    pd = (vp * world)(*[t.data_ptr() for t in ds])
    pi = (vp * world)(*[t.data_ptr() for t in is_])
    res = vp()
    cp = counts.ctypes.data

    def refused(needle, *args):
        res.value = 1
        assert L.lmi_join_range_parts(*args) != 0
        assert needle in L.lmi_last_error(), L.lmi_last_error()
        assert args[8] is None or res.value is None   # *result = NULL after a refusal

    ok = (h, world, ur.NQ, nb, cp, pd, pi, 0, ctypes.byref(res), 1)
    change = lambda **kw: tuple(kw.get(n, v) for n, v in zip(("h", "world", "nq", "nb", "counts", "dists", "ids", "max_total", "result",
                                                               "on_device"), ok))
    refused(b"NULL handle", *change(h=None))
    for w in (0, 65):
        refused(b"outside [1,64]", *change(world=w))
    refused(b"negative", *change(nq=-1))
    for bad_nb in (0, 1025):
        refused(b"outside [1,1024]", *change(nb=bad_nb))
    refused(b"too large", *change(nq=1 << 21, nb=1024))
    for name in ("counts", "dists", "ids"):
        refused(b"must not be NULL", *change(**{name: None}))
    refused(b"result pointer is NULL", *change(result=None))
    refused(b"max_total -1 is negative", *change(max_total=-1))
    neg = counts.copy()
    q, t = (int(x[0]) for x in np.nonzero(counts[1] > 0))
    neg[1, q, t] = -5
    refused(f"part 1 at query {q}, t {t} is negative (-5)".encode(), *change(counts=neg.ctypes.data))
    two = counts.copy()
    two[0, q, t] = 1
    refused(f"query {q}, t {t} has results in part 0 and in part 1".encode(), *change(counts=two.ctypes.data))
    pd_null = (vp * world)(ds[0].data_ptr(), None)
    refused(b"part 1 holds", *change(dists=pd_null))
    total = int(counts.sum())
    refused(f"the parts hold {total}".encode(), *change(max_total=total - 1))
    # nq == 0 succeeds with an empty result that reports the call's nb
    assert L.lmi_join_range_parts(h, world, 0, nb, None, None, None, 0, ctypes.byref(res), 1) == 0
    empty = capi.RangeResult(res, 0)
    assert empty.total == 0 and empty.lims.tolist() == [0] and empty.pair_counts().shape == (0, nb)
    empty.close()
    assert capi.range_join_last_plan() == dict.fromkeys(capi.RANGE_JOIN_FIELDS, 0)
    with handles[0].scan_range_device(torch.zeros((0, d), device="cuda"), torch.zeros((0, nb), dtype=torch.int32, device="cuda"), nb,
                                      0.5) as e0:
        assert e0.pair_counts().shape == (0, nb)
    assert L.lmi_range_result_pair_counts(None, None, None) != 0 and b"NULL result" in L.lmi_last_error()
    for bad in (-1, (1 << 30) + 1):
        assert L.lmi_range_join_set_geometry(bad) != 0 and b"outside [0, 2^30]" in L.lmi_last_error()
    # lmi_allgather_join_range: its own refusals, then the join's
    part = handles[0].scan_range_device(torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(order)).cuda(), nb, radius)
    handles[0].set_stream(torch.cuda.current_stream().cuda_stream)
    comm = handles[0].comm_init(0, 1, capi.Index.comm_unique_id())
    try:
        def refused_ag(needle, *args):
            assert L.lmi_allgather_join_range(*args) != 0
            assert needle in L.lmi_last_error(), L.lmi_last_error()

        refused_ag(b"NULL handle", None, comm, 0, 1, part._r, 0, ctypes.byref(res))
        refused_ag(b"NULL communicator", h, None, 0, 1, part._r, 0, ctypes.byref(res))
        refused_ag(b"NULL part", h, comm, 0, 1, None, 0, ctypes.byref(res))
        for w in (0, 65):
            refused_ag(b"outside [1,64]", h, comm, 0, w, part._r, 0, ctypes.byref(res))
        for rank in (-1, 1):
            refused_ag(b"rank", h, comm, rank, 1, part._r, 0, ctypes.byref(res))
        refused_ag(b"result pointer is NULL", h, comm, 0, 1, part._r, 0, None)
        refused_ag(b"is negative", h, comm, 0, 1, part._r, -1, ctypes.byref(res))
        refused_ag(f"the parts hold {part.total}".encode(), h, comm, 0, 1, part._r, part.total - 1, ctypes.byref(res))
        with handles[0].allgather_join_range(comm, 0, 1, part, max_total=part.total) as whole:   # and at the total it passes
            same((whole.lims,) + whole.read(), (part.lims,) + part.read(), "a world of one reproduces the part")
            np.testing.assert_array_equal(whole.pair_counts(), part.pair_counts())
    finally:
        torch.cuda.synchronize()
        part.close()
        capi.Index.comm_destroy(comm)
        handles[0].set_stream(0)


def test_a_joined_result_outlives_its_handle(capi, index_of, oracle):
    d, nb, world, metric = 64, 3, 2, "l2"
    Q = ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    counts, ds, is_ = rank_parts([index_of(d, metric, world, "assign", r) for r in range(world)], Q, order, radius)
    joiner = capi.Index(0)
    res = joiner.join_range_parts(counts, ds, is_)
    joiner.close()
    del ds, is_
    torch.cuda.empty_cache()
    with res:
        same((res.lims,) + res.read(), rr.recipe_ref(oracle, d, nb, metric), "after the handle is gone")
        assert res.pair_counts().sum() == res.total


@pytest.mark.parametrize("metric", ur.METRICS)
def test_existing_calls_are_unchanged_by_part_and_join_calls(index_of, oracle, metric):
    d, nb = 64, 8
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    before = (idx.search(Q, Q, 4, 10, want_keys=True), idx.scan_union(Q, order, 129), idx.scan_range(Q, order, radius))
    handles = [index_of(d, metric, 2, "assign", r) for r in range(2)]
    counts, ds, is_ = rank_parts(handles + [idx], Q, order, radius)
    joined(idx, counts[:2], ds[:2], is_[:2])
    after = (idx.search(Q, Q, 4, 10, want_keys=True), idx.scan_union(Q, order, 129), idx.scan_range(Q, order, radius))
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    same(after[2], rr.recipe_ref(oracle, d, nb, metric), f"scan_range against range_ref {metric}")
