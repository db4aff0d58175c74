"""GPU (`-m gpu`): a range result sorted by distance on the device (lmi_range_result_sort; include/lmi_hip.h) against
tests/range_sort_ref.py -- numpy's stable argsort per segment applied to both arrays.  Every comparison is on bit patterns: the
distances as uint32, the ids, lims.  Arbitrary results need no index: `join_range_parts` with a world of one turns any host counts /
dists / ids into a `RangeResult`; the results of real scans come from union_ref.case (6 000 rows in 12 buckets, 150 queries) with
range_ref's radius recipe."""
import ctypes

import numpy as np
import pytest
import torch

import range_ref as rr
import range_sort_ref as rsr
import union_filter_ref as fr
import union_parts_ref as upr
import union_ref as ur
from path_mass_ref import synthetic_tree

pytestmark = pytest.mark.gpu

SEAMS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2047, 2048, 2049, 5000, 70001)
ZERO = dict.fromkeys(("groups", "wave_segments", "tile_segments", "long_segments"), 0)


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


@pytest.fixture(scope="module")
def plain(capi):
    """A handle without an index: the sort and the join need the device and the stream only."""
    idx = capi.Index(0)
    yield idx
    idx.close()


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return a.view(np.uint32)


def same(got, want, what=""):
    """got, want: (dists, ids)"""
    assert bits(got[0]).shape == bits(want[0]).shape and bits(got[1]).shape == bits(want[1]).shape, what
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=f"ids {what}")
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]), err_msg=f"dist bits {what}")


def result_of(idx, lens, d, ids):
    """Any host segments as a RangeResult on the device (lmi_join_range_parts, one part)."""
    counts = np.asarray(lens, np.int32).reshape(1, -1, 1)
    return idx.join_range_parts(counts, [np.ascontiguousarray(d, np.float32)], [np.ascontiguousarray(ids, np.uint32)])


_seams = {}


def seam_case():
    """(lims, dists, ids, reference): the seam lengths in a shuffled order; 8 distinct distances so that most entries tie, with -0, +0,
    negatives, +inf and NaNs of both signs sprinkled in; ids = arange.  Computed once."""
    if not _seams:
        rs = np.random.RandomState(5)
        lens = np.asarray(SEAMS)[rs.permutation(len(SEAMS))]
        lims = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        total = int(lims[-1])
        d = rs.choice(np.asarray([0.125, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0], np.float32), size=total).astype(np.float32)
        special = np.asarray([0x80000000, 0x00000000, 0xBF000000, 0xC0400000, 0x7F800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF],
                             np.uint32).view(np.float32)
        where = rs.rand(total) < 0.05
        d[where] = rs.choice(special, size=int(where.sum()))
        ids = np.arange(total, dtype=np.uint32)
        want = rsr.range_sort_ref(lims, d, ids)
        for a in (lens, lims, d, ids) + want:
            a.setflags(write=False)
        _seams["case"] = (lens, lims, d, ids, want)
    return _seams["case"]


def sorted_under(capi, plain, tile_rows, scratch_bytes):
    lens, lims, d, ids, _ = seam_case()
    try:
        capi.range_sort_set_geometry(tile_rows, scratch_bytes)
        with result_of(plain, lens, d, ids) as res:
            assert res.sorted is False
            assert res.sort(plain) is res and res.sorted is True
            np.testing.assert_array_equal(res.lims, lims)
            np.testing.assert_array_equal(res.pair_counts()[:, 0], lens)
            return res.read(), capi.range_sort_last_plan()
    finally:
        capi.range_sort_set_geometry(0, 0)


def test_seams_under_the_default_geometry(capi, plain):
    lens, lims, d, ids, want = seam_case()
    got, plan = sorted_under(capi, plain, 0, 0)
    same(got, want, "default geometry")
    assert plan == dict(groups=1, wave_segments=10, tile_segments=6, long_segments=1, skipped_segments=2, tile_rows=8192, wave_rows=256,
                        merge_rows=2048, max_passes=4, scratch_bytes=8 * int(lims[-1]) + 16 * 70001, results=int(lims[-1]))
    # not vacuous: ties everywhere, the special values present, and the order differs from the input's
    assert np.unique(bits(d)).size <= 17 and np.isnan(d).sum() > 100 and (bits(d) == 0x80000000).sum() > 10
    assert (bits(got[1]) != ids).sum() > 50000


@pytest.mark.parametrize("tile_rows,forms,passes", ((128, (4, 3, 10), 10), (256, (7, 3, 7), 9)))
def test_seams_with_forced_tile_rows(capi, plain, tile_rows, forms, passes):
    """All three forms in use and more than one merge pass: the tile seams (T, T + 1, 2T, 2T + 1 are among the lengths), run boundaries
    that fall anywhere, an odd run at the end of a pass."""
    got, plan = sorted_under(capi, plain, tile_rows, 0)
    same(got, seam_case()[4], f"tile_rows={tile_rows}")
    assert (plan["wave_segments"], plan["tile_segments"], plan["long_segments"]) == forms and min(forms) > 0
    assert plan["max_passes"] == passes > 1 and plan["tile_rows"] == tile_rows and plan["wave_rows"] == tile_rows // 2
    assert plan["merge_rows"] == tile_rows and plan["skipped_segments"] == 2
    same(got, sorted_under(capi, plain, 0, 0)[0], f"tile_rows={tile_rows} against the default geometry")


def test_seams_with_a_small_scratch_budget(capi, plain):
    """24 bytes per entry and a budget of 6 000 entries: several groups, the segment of 70 001 entries taken alone (above the budget)."""
    lens, lims, d, ids, want = seam_case()
    got, plan = sorted_under(capi, plain, 0, 24 * 6000)
    same(got, want, "scratch_bytes = 144 000")
    assert plan["groups"] >= 4 and plan["scratch_bytes"] == 24 * 70001 > 24 * 6000
    got2, plan2 = sorted_under(capi, plain, 128, 24 * 300)
    same(got2, want, "tile_rows = 128, scratch_bytes = 7 200")
    assert plan2["groups"] > plan["groups"]
    same(got, got2, "the two budgets")


@pytest.fixture(scope="module")
def index_of(capi):
    """One built index per (d, metric) of union_ref.case, with a random root model."""
    made = {}

    def get(d, metric):
        if (d, metric) not in made:
            X, Q, lab, ids = ur.case(d)
            idx = capi.Index(0, metric=metric)
            idx.set_mlp(ur.layers_for(d, ur.L, 3))
            idx.set_buckets(np.ascontiguousarray(X), lab, ur.L, ids=np.ascontiguousarray(ids, dtype=np.uint32))
            made[(d, metric)] = idx
        return made[(d, metric)]
    yield get
    for h in made.values():
        h.close()


def sorted_ref(want):
    """range_ref's (lims, dists, ids) -> (lims, dists, ids) sorted; range_ref.stable_by_distance is the same statement."""
    d2, i2 = rsr.range_sort_ref(*want)
    e2, j2 = rr.stable_by_distance(*want)
    assert bits(d2).tobytes() == bits(e2).tobytes() and bits(i2).tobytes() == bits(j2).tobytes()
    return want[0], d2, i2


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", (45, 64))
def test_sorted_scan_on_a_real_index(capi, index_of, oracle, d, metric):
    """scan_range(sort=True) is range_ref, sorted; host pointers equal device pointers; search_range sorts the same."""
    nb = 8
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    lims, wd, wi = sorted_ref(rr.recipe_ref(oracle, d, nb, metric))
    got = idx.scan_range(Q, order, radius, sort=True)
    np.testing.assert_array_equal(got[0], lims)
    same(got[1:], (wd, wi), f"host pointers d={d} {metric}")
    plan = capi.range_sort_last_plan()
    assert plan["results"] == lims[-1] > 1000 and plan["wave_segments"] + plan["tile_segments"] >= 50
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(order)).cuda()
    with idx.scan_range_device(q_t, bo_t, nb, radius, sort=True) as res:
        assert res.sorted is True
        d_t = torch.zeros(res.total, dtype=torch.float32, device="cuda")
        i_t = torch.zeros(res.total, dtype=torch.int32, device="cuda")
        res.read_into(d_t, i_t)
        np.testing.assert_array_equal(res.lims, lims)
        same((d_t, i_t), (wd, wi), f"device pointers d={d} {metric}")
    unsorted = idx.search_range(Q, Q, 3, radius)
    hs = idx.search_range(Q, Q, 3, radius, sort=True)
    np.testing.assert_array_equal(hs[0], unsorted[0])
    np.testing.assert_array_equal(hs[3], unsorted[3])
    same(hs[1:3], rsr.range_sort_ref(*unsorted[:3]), f"search_range d={d} {metric}")
    with idx.search_range_device(q_t, q_t, 3, radius, sort=True) as res:
        same(res.read(), hs[1:3], "search_range_device")


def test_sorted_scan_with_a_filter(capi, index_of, oracle):
    d, nb, metric = 64, 3, "l2"
    idx = index_of(d, metric)
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    order = ur.random_order(nb)
    keep = [fr.filter_lists(d)[0]]
    allowed = fr.allowed_rows(keep, [fr.KEEP], labs)
    lims, wd, wi = sorted_ref(rr.range_ref(oracle, rows, labs, order, Q, np.float32(np.inf), metric, allowed))
    f = capi.Filter(idx, keep, [fr.KEEP])
    try:
        got = idx.scan_range(Q, order, np.float32(np.inf), filter=f, sort=True)
    finally:
        f.close()
    np.testing.assert_array_equal(got[0], lims)
    assert np.diff(lims).max() > 256   # a tile-form segment
    same(got[1:], (wd, wi), "filtered, sorted")


def test_search_tree_range_sorted(capi, oracle):
    from test_gpu_range import tree_index, tree_radius

    idx, Xs, lab, ids, Qn, Qs = tree_index(capi, "ip")
    rows, labs = ur.buckets_of(Xs, lab, ids, 12)
    try:
        slab = idx.search_tree_union(Qn, Qs, 5, 10)[3]
        radius = tree_radius(oracle, rows, labs, slab, Qs, "ip")
        lims, wd, wi = sorted_ref(rr.range_ref(oracle, rows, labs, slab, Qs, radius, "ip"))
        got = idx.search_tree_range(Qn, Qs, 5, radius, sort=True)
        np.testing.assert_array_equal(got[0], lims)
        same(got[1:3], (wd, wi), "search_tree_range")
        q_n, q_s = torch.from_numpy(Qn).cuda(), torch.from_numpy(Qs).cuda()
        with idx.search_tree_range_device(q_n, q_s, 5, radius, sort=True) as res:
            same(res.read(), (wd, wi), "search_tree_range_device")
    finally:
        idx.close()


def test_idempotence_and_the_flag(capi, plain, index_of, oracle):
    """Sorting twice changes no bit; the flag; lmi_allgather_join_range (one rank) refuses a sorted part by name."""
    d, nb, metric = 64, 3, "ip"
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(np.array(order)).cuda()
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    comm = idx.comm_init(0, 1, capi.Index.comm_unique_id())
    try:
        with idx.scan_range_device(q_t, bo_t, nb, radius) as part:
            assert part.sorted is False
            before = part.read()
            counts = part.pair_counts()
            with idx.allgather_join_range(comm, 0, 1, part) as joined:   # an unsorted part joins
                same(joined.read(), before, "a world of one reproduces the part")
                assert joined.sorted is False
                joined.sort(idx)                                          # and the JOINED result may be sorted
                assert joined.sorted is True
                once_joined = joined.read()
            part.sort(plain)   # any handle of the device serves
            assert part.sorted is True
            once = part.read()
            same(once, rsr.range_sort_ref(part.lims, *before), "sorted once")
            same(once_joined, once, "the joined result, sorted")
            part.sort(idx)
            assert part.sorted is True
            same(part.read(), once, "sorted twice")
            np.testing.assert_array_equal(part.pair_counts(), counts)
            with pytest.raises(capi.LmiError, match="sorted"):
                idx.allgather_join_range(comm, 0, 1, part)
    finally:
        torch.cuda.synchronize()
        capi.Index.comm_destroy(comm)
        idx.set_stream(0)


def frame(X):
    import pandas as pd

    df = pd.DataFrame(X)
    df.index += 1
    return df


@pytest.mark.parametrize("levels", ((4,), (4, 3)))
def test_li_sorts_on_the_device(capi, oracle, monkeypatch, levels):
    """range_search_resident(sort=True) returns what it returned before -- range_ref, stably sorted -- and the sort ran in the library."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from
    from test_gpu_range import tree_radius

    root, internal, bucket_paths, dp2, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    if len(levels) == 1:
        dp = np.random.RandomState(2).randint(0, 4, size=(Xn.shape[0], 1)).astype(np.int64)
        li = LearnedIndex(net_from(root), {}, [(b,) for b in range(4)])
    else:
        dp = dp2
        li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    try:
        li.prepare(frame(Xn), frame(Xs), dp, list(levels))
        all_ids = np.arange(1, Xs.shape[0] + 1)
        if len(levels) == 1:
            nb = 3
            bo = li._engine.mlp_topk(Qn, nb)
            rows, labs = ur.buckets_of(Xs, dp[:, 0], all_ids, 4)
        else:
            nb = 5
            bo, _ = li._engine.nav_order(Qn, nb)
            lab = np.asarray([li._path_ids[tuple(int(v) for v in p)] for p in dp])
            rows, labs = ur.buckets_of(Xs, lab, all_ids, len(li._path_ids))
            monkeypatch.setattr(LearnedIndex, "_nav_chunk", lambda self: 64)   # several pieces, each sorted by its own call
            assert Qn.shape[0] > 64
        radius = tree_radius(oracle, rows, labs, bo, Qs, "ip")
        lims, wd, wi = sorted_ref(rr.range_ref(oracle, rows, labs, bo, Qs, radius, "ip"))
        capi.range_sort_set_geometry(0, 0)
        assert capi.lib().lmi_range_result_sort(None, None) != 0           # clears the plan words
        assert capi.range_sort_last_plan()["results"] == 0
        ls, ds, ns, _ = li.range_search_resident(Qn, Qs, list(levels), radius, n_buckets=nb, sort=True)
        np.testing.assert_array_equal(ls, lims)
        assert ds.dtype == np.float64 and ns.dtype == np.uint32
        same((ds.astype(np.float32), ns), (wd, wi), f"li sorted, levels {levels}")
        plan = capi.range_sort_last_plan()
        assert plan["results"] > 0 and plan["wave_segments"] > 0
        if len(levels) == 1:
            assert plan["results"] == lims[-1]
    finally:
        li.close()


@pytest.mark.parametrize("world", (1, 3))
def test_sharded_range_search_sorted(capi, oracle, monkeypatch, world):
    """One card plays every rank: rank r's ShardedSearcher.range_search(sort=True) with the collectives replayed from the other
    ranks' parts equals the single handle's sorted result, on every rank."""
    from learnedmetricindex_amd import sharded

    d, nb, metric = 64, 3, "l2"
    X, Q, lab, ids = ur.case(d)
    layers = ur.layers_for(d, ur.L, 3)
    radius = rr.recipe_radii(oracle, d, nb, metric)[0]
    owner = upr.owners(world) if world > 1 else np.zeros(ur.L, np.int32)
    handles = []
    try:
        for r in range(world):
            h = capi.Index(0, metric=metric)
            h.set_mlp(layers)
            h.set_buckets(np.ascontiguousarray(X), lab, ur.L, ids=np.ascontiguousarray(ids, dtype=np.uint32),
                          owned=None if world == 1 else np.ascontiguousarray(owner == r, dtype=np.uint8))
            handles.append(h)
        single = capi.Index(0, metric=metric)
        handles.append(single)
        single.set_mlp(layers)
        single.set_buckets(np.ascontiguousarray(X), lab, ur.L, ids=np.ascontiguousarray(ids, dtype=np.uint32))
        want = single.search_range(Q, Q, nb, radius, sort=True)
        assert want[0][-1] > 1000
        q_t = torch.from_numpy(np.array(Q)).cuda()
        bo_t = torch.from_numpy(want[3]).cuda()
        # what every rank contributes to the two collectives
        counts, blocks = [], []
        for r in range(world):
            with handles[r].scan_range_device(q_t, bo_t, nb, radius) as part:
                counts.append(torch.from_numpy(part.pair_counts()).cuda())
                blocks.append(part.read())
        tmax = max(b[0].size for b in blocks)
        padded = []
        for dd, ii in blocks:
            blk = torch.zeros((2, tmax), dtype=torch.int32, device="cuda")
            blk[0, : dd.size] = torch.from_numpy(dd.view(np.int32)).cuda()
            blk[1, : ii.size] = torch.from_numpy(ii.view(np.int32)).cuda()
            padded.append(blk)
        for r in range(world):
            def gather(t, w, group=None, r=r):
                mine, every = (counts[r], counts) if tuple(t.shape) == (ur.NQ, nb) else (padded[r], padded)
                assert w == world and torch.equal(t, mine)   # the rank sent what it owns
                return torch.cat(every)

            monkeypatch.setattr(sharded, "_all_gather_cat", gather)
            s = sharded.ShardedSearcher(handles[r], r, world, shard_inference=False)
            lims, dd, ii, bo = s.range_search(q_t, q_t, nb, radius, sort=True)
            np.testing.assert_array_equal(lims, want[0])
            np.testing.assert_array_equal(bo.cpu().numpy(), want[3])
            same((dd, ii), want[1:3], f"world {world}, rank {r}")
            un = s.range_search(q_t, q_t, nb, radius)   # and without sort: (rank, row) order as ever
            same(un[1:3], single.search_range(Q, Q, nb, radius)[1:3], f"unsorted, world {world}, rank {r}")
        rep = sharded.ReplicaSearcher(single, 0, 1).range_search(q_t, q_t, nb, radius, sort=True)
        np.testing.assert_array_equal(rep[0], want[0])
        same(rep[1:3], want[1:3], "ReplicaSearcher")
    finally:
        for h in handles:
            h.close()


def test_empty_and_singleton_results_launch_nothing(capi, plain):
    with result_of(plain, [], np.zeros(0, np.float32), np.zeros(0, np.uint32)) as res:   # nq == 0
        assert res.sorted is False and res.sort(plain).sorted is True
        plan = capi.range_sort_last_plan()
        assert {k: plan[k] for k in ZERO} == ZERO and plan["results"] == 0 and plan["skipped_segments"] == 0
    with result_of(plain, [0, 0, 0], np.zeros(0, np.float32), np.zeros(0, np.uint32)) as res:   # a total of 0
        assert res.sort(plain).sorted is True
        plan = capi.range_sort_last_plan()
        assert {k: plan[k] for k in ZERO} == ZERO and plan["skipped_segments"] == 3 and plan["scratch_bytes"] == 0
    d = np.asarray([3.0, np.nan, -1.0, 2.0], np.float32)
    with result_of(plain, [1, 0, 1, 1, 0, 1], d, np.arange(4, dtype=np.uint32)) as res:   # all singletons
        assert res.sort(plain).sorted is True
        plan = capi.range_sort_last_plan()
        assert {k: plan[k] for k in ZERO} == ZERO and plan["skipped_segments"] == 6 and plan["results"] == 4
        same(res.read(), (d, np.arange(4, dtype=np.uint32)), "singletons stay")
    with result_of(plain, [1, 2, 1], np.asarray([5.0, 2.0, 1.0, 0.0], np.float32), np.arange(4, dtype=np.uint32)) as res:
        res.sort(plain)   # one pair between two singletons: nothing outside its segment moves
        same(res.read(), (np.asarray([5.0, 1.0, 2.0, 0.0], np.float32), np.asarray([0, 2, 1, 3], np.uint32)), "a pair between singletons")
        assert capi.range_sort_last_plan()["wave_segments"] == 1


def test_refusals_and_the_handle_afterwards(capi, plain, index_of, oracle):
    d, nb, metric = 64, 3, "ip"
    idx, Q = index_of(d, metric), ur.case(d)[1]
    radius, order = rr.recipe_radii(oracle, d, nb, metric)
    L = capi.lib()
    before = (idx.search(Q, Q, 4, 10), idx.scan_union(Q, order, 10), idx.scan_range(Q, order, radius))
    with result_of(plain, [3], np.asarray([3.0, 1.0, 2.0], np.float32), np.arange(3, dtype=np.uint32)) as res:
        assert L.lmi_range_result_sort(None, res._r) != 0 and b"NULL handle" in L.lmi_last_error()
        assert L.lmi_range_result_sort(plain._h, None) != 0 and b"NULL result" in L.lmi_last_error()
        assert capi.range_sort_last_plan() == dict.fromkeys((n.lower() for n in capi.RANGE_SORT_PLAN_FIELDS), 0)
        flag = ctypes.c_int(7)
        assert L.lmi_range_result_sorted(None, ctypes.byref(flag)) != 0 and L.lmi_range_result_sorted(res._r, None) != 0
        assert res.sorted is False   # no refusal set it
        for tile_rows, scratch, needle in ((-1, 0, b"negative"), (0, -1, b"negative"), (32, 0, b"power of two"), (100, 0, b"power of two"),
                                           (16384, 0, b"power of two"), (0, (1 << 40) + 1, b"above 2^40")):
            assert L.lmi_range_sort_set_geometry(tile_rows, scratch) != 0 and needle in L.lmi_last_error(), (tile_rows, scratch)
        res.sort(idx)
        assert capi.range_sort_last_plan()["tile_rows"] == 8192   # a refused value set nothing
        for tile_rows in (64, 8192):
            assert L.lmi_range_sort_set_geometry(tile_rows, 1 << 40) == 0
        assert L.lmi_range_sort_set_geometry(0, 0) == 0
        same(res.read(), (np.asarray([1.0, 2.0, 3.0], np.float32), np.asarray([1, 2, 0], np.uint32)), "a triple")
    after = (idx.search(Q, Q, 4, 10), idx.scan_union(Q, order, 10), idx.scan_range(Q, order, radius))
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
