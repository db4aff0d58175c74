"""GPU (`-m gpu`): the filtered union scan (lmi_filter_create, lmi_scan_union_filtered, lmi_search_union_filtered,
lmi_search_tree_union_filtered; include/lmi_hip.h) -- the union scan with every query's candidates restricted to the rows its filter
allows -- against the unchanged CPU oracle.

Every comparison is exact: dists as uint32 bit patterns, ids and counts with array_equal, against tests/union_filter_ref.py (union_ref on
the buckets with their disallowed rows removed).  The inputs are union_ref's, the filter set is union_filter_ref's;
tests/test_union_filter_host.py checks on the oracle alone that they have the properties relied on here."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import union_filter_ref as fr
import union_ref as ur
from path_mass_ref import synthetic_tree

pytestmark = pytest.mark.gpu

DIMS, NBS, KS = (45, 64, 136), (1, 8), (1, 10, 129, 1024)


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def same(got, want, what=""):
    d, i, c = (np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a) for a in got[:3])
    assert d.dtype == np.float32 and d.shape == want[0].shape and i.shape == want[1].shape and c.shape == want[2].shape, what
    np.testing.assert_array_equal(c.astype(np.int32), want[2], err_msg=f"counts {what}")
    np.testing.assert_array_equal(i.view(np.uint32) if i.dtype != np.uint32 else i, want[1], err_msg=f"ids {what}")
    np.testing.assert_array_equal(d.view(np.uint32), want[0].view(np.uint32), err_msg=f"dist bits {what}")


def build(capi, X, lab, ids, n_buckets=ur.L, layers=None, **kw):
    idx = capi.Index(0, **kw)
    if layers is not None:
        idx.set_mlp(layers)
    idx.set_buckets(np.ascontiguousarray(X), lab, n_buckets, ids=np.ascontiguousarray(ids, dtype=np.uint32))
    return idx


_idx = {}


@pytest.fixture(scope="module")
def index_of(capi):
    """One built index per (d, metric) of union_ref.case with a random root model, and the shared filter set made on it."""
    def get(d, metric):
        if (d, metric) not in _idx:
            X, Q, lab, ids = ur.case(d)
            idx = build(capi, X, lab, ids, layers=ur.layers_for(d, ur.L, 3), metric=metric)
            _idx[(d, metric)] = (idx, capi.Filter(idx, fr.filter_lists(d), fr.MODES))
        return _idx[(d, metric)]
    yield get
    for h, f in _idx.values():
        f.close()
        h.close()
    _idx.clear()


def reference(oracle, d, order, k, metric, filter_of, allowed=None):
    X, Q, lab, ids = ur.case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    return fr.union_filter_ref(oracle, rows, labs, order, Q, k, metric, fr.case_allowed(d) if allowed is None else allowed, filter_of)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_filtered_scan_parity(capi, index_of, oracle, d, metric, nb, k):
    """The grid: d = 45 element loads, 64 and 136 16-byte loads; k = 129 and 1024 cross the list sizes; filter_of cycles through
    unfiltered and the five filters."""
    order, fo = ur.random_order(nb), fr.filter_of()
    idx, filt = index_of(d, metric)
    got = idx.scan_union(ur.case(d)[1], order, k, filter=filt, filter_of=fo)
    same(got, reference(oracle, d, order, k, metric, fo), f"d={d} {metric} nb={nb} k={k}")
    plan, fplan = capi.union_last_plan(), capi.filter_last_plan()
    assert plan["VEC_ROWS"] == (0 if (d == 45 and metric == "ip") else 1) and plan["LIST_ROWS"] >= k and fplan["FILTERS"] == fr.NF


def test_masks_and_counts(index_of):
    """bucket_mask of every (filter, bucket) against numpy -- the bucket sizes 0, 1, 33, 64, 65 and 257 are the row-block edges -- and
    counts() against the masks' sums."""
    idx, filt = index_of(64, "ip")
    allowed = fr.case_allowed(64)
    cnt = filt.counts()
    assert cnt.shape == (fr.NF, ur.L) and cnt.dtype == np.int64
    for j in range(fr.NF):
        for b in range(ur.L):
            m = filt.bucket_mask(j, b)
            assert m.dtype == np.uint8 and m.shape == (ur.SIZES[b],)
            np.testing.assert_array_equal(m, allowed[j][b].astype(np.uint8), err_msg=f"filter {j} bucket {b}")
            assert cnt[j, b] == int(m.sum())
    assert np.all(cnt[3] == 0) and cnt[4, 4] == ur.SIZES[4] and cnt[2].sum() == ur.N - 2


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("j", [0, 2])
def test_one_filter_equals_subset_then_scan(capi, index_of, metric, j):
    """A batch that uses one filter answers like lmi_subset(list, mode) followed by lmi_scan_union, bit for bit: KEEP (F0) and DROP (F2)."""
    d, nb, k = 64, 8, 129
    idx, filt = index_of(d, metric)
    Q, order = ur.case(d)[1], ur.random_order(nb)
    sub = idx.subset(fr.filter_lists(d)[j], drop=fr.MODES[j] == fr.DROP)
    try:
        want = sub.scan_union(Q, order, k)
    finally:
        sub.close()
    same(idx.scan_union(Q, order, k, filter=filt, filter_of=np.full(ur.NQ, j, np.int32)), want, f"filter {j} of the set")
    one = capi.Filter(idx, [fr.filter_lists(d)[j]], [fr.MODES[j]])
    try:
        same(idx.scan_union(Q, order, k, filter=one), want, f"a set of one, filter_of = None")
    finally:
        one.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_filters_that_remove_nothing_equal_scan_union(capi, index_of, metric):
    d, nb, k = 45, 8, 129
    idx, filt = index_of(d, metric)
    Q, order = ur.case(d)[1], ur.random_order(nb)
    want = idx.scan_union(Q, order, k)
    same(idx.scan_union(Q, order, k, filter=filt, filter_of=np.full(ur.NQ, -1, np.int32)), want, "filter_of all -1")
    assert capi.filter_last_plan()["SKIPPED"] == 0
    none = capi.Filter(idx, [[]], ["drop"])
    try:
        assert np.array_equal(none.counts()[0], ur.SIZES)
        same(idx.scan_union(Q, order, k, filter=none), want, "an empty drop list")
    finally:
        none.close()


@pytest.mark.parametrize("metric", ur.METRICS)
@pytest.mark.parametrize("k", [10, 25, 100])
def test_a_split_tie_group_keeps_rank_then_row(capi, oracle, metric, k):
    """40 copies of one vector over three buckets, a filter that drops every third: the survivors come first, by (rank, row)."""
    X, Q, lab, ids, order = ur.tie_case(64)
    rows, labs = ur.buckets_of(X, lab, ids)
    tied = np.concatenate([labs[b][np.all(rows[b] == Q[0], axis=1)] for b in ur.TIE_BUCKETS])
    gone, left = fr.tie_filter(tied)
    allowed = fr.allowed_rows([gone], [fr.DROP], labs)
    want = fr.union_filter_ref(oracle, rows, labs, order, Q, k, metric, allowed, None)
    idx = build(capi, X, lab, ids, metric=metric)
    filt = capi.Filter(idx, [gone], ["drop"])
    try:
        got = idx.scan_union(Q, order, k, filter=filt)
    finally:
        filt.close()
        idx.close()
    same(got, want, f"ties {metric} k={k}")
    m = min(k, left.size)
    np.testing.assert_array_equal(got[1][:4, :m], np.broadcast_to(left[:m], (4, m)))
    assert np.all(got[0][:4, :m].view(np.uint32) == got[0][0, 0].view(np.uint32)) and not np.isin(got[1], gone).any()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_an_allowed_nan_row_is_never_returned(capi, oracle, metric):
    d = 45
    X, Q, lab, ids, row = ur.nan_case(d)
    rows, labs = ur.buckets_of(X, lab, ids)
    order = np.tile(np.asarray([3, 4], dtype=np.int32), (ur.NQ, 1))
    keep = np.concatenate([labs[3][::2], [ids[row]], labs[4][1::3]]).astype(np.uint32)   # the NaN row is allowed
    allowed = fr.allowed_rows([keep], [fr.KEEP], labs)
    assert allowed[0][3][np.flatnonzero(labs[3] == ids[row])[0]]
    want = fr.union_filter_ref(oracle, rows, labs, order, Q, 1024, metric, allowed, None)
    assert not np.any(want[1] == ids[row]) and np.all(want[2] == allowed[0][3].sum() + allowed[0][4].sum() - 1)
    idx = build(capi, X, lab, ids, metric=metric)
    filt = capi.Filter(idx, [keep])
    try:
        got = idx.scan_union(Q, order, 1024, filter=filt)
    finally:
        filt.close()
        idx.close()
    same(got, want, f"nan {metric}")
    assert not np.any(got[1] == ids[row])


def host_slots(filt, order, fo):
    """(scanned, skipped) slots as the host can count them from counts() and the order."""
    cnt, sizes = filt.counts(), np.asarray(ur.SIZES)
    scanned = skipped = 0
    for q in range(order.shape[0]):
        for b in order[q]:
            if b < 0 or sizes[b] == 0:
                continue
            if fo[q] >= 0 and cnt[fo[q], b] == 0:
                skipped += 1
            else:
                scanned += 1
    return scanned, skipped


def test_skipped_slots_are_accounted_for(capi, index_of):
    d, nb, k = 64, 8, 10
    idx, filt = index_of(d, "ip")
    order, fo = ur.random_order(nb), fr.filter_of()
    idx.scan_union(ur.case(d)[1], order, k, filter=filt, filter_of=fo)
    plan = capi.filter_last_plan()
    scanned, skipped = host_slots(filt, order, fo)
    assert skipped > 50 and plan["SKIPPED"] == skipped and plan["SLOTS"] == scanned and plan["FILTERS"] == fr.NF
    assert plan["MASK_BYTES"] == fr.NF * 4 * sum((n + 31) // 32 for n in ur.SIZES)
    idx.scan_union(ur.case(d)[1], order, k)   # an unfiltered call clears the words
    assert capi.filter_last_plan() == dict.fromkeys(capi.FILTER_PLAN_FIELDS, 0)


@pytest.mark.parametrize("metric", ur.METRICS)
def test_forced_geometry_changes_nothing(capi, index_of, oracle, metric):
    """32 queries per group and a 64-KiB slab: several groups, several waves, the same bits."""
    d, nb, k = 64, 8, 129
    order, fo = ur.random_order(nb), fr.filter_of()
    want = reference(oracle, d, order, k, metric, fo)
    (idx, filt), Q = index_of(d, metric), ur.case(d)[1]
    try:
        capi.union_set_geometry(32, 64 << 10)
        forced = idx.scan_union(Q, order, k, filter=filt, filter_of=fo)
        plan, fplan = capi.union_last_plan(), capi.filter_last_plan()
    finally:
        capi.union_set_geometry(0, 0)
    same(forced, want, "forced")
    assert plan["GROUPS"] == 5 and plan["QUERY_ROWS"] == 32 and plan["WAVES"] > 1
    assert fplan["SKIPPED"] == host_slots(filt, order, fo)[1] and fplan["SLOTS"] == host_slots(filt, order[128:], fo[128:])[0]


@pytest.mark.parametrize("metric", ur.METRICS)
def test_search_union_filtered_with_a_row_budget(index_of, oracle, metric):
    """The routed form equals the reference applied to the order it returns; the order is lmi_mlp_topk's under the same budget -- the
    stop counts whole buckets, whatever the filter allows."""
    d, nb, k = 64, 8, 100
    idx, filt = index_of(d, metric)
    Q, fo = ur.case(d)[1], fr.filter_of()
    idx.set_stop_rows(1500)
    try:
        dd, ii, cc, bo = idx.search_union(Q, Q, nb, k, filter=filt, filter_of=fo)
        np.testing.assert_array_equal(bo, idx.mlp_topk(Q, nb))
    finally:
        idx.set_stop_rows(0)
    assert (bo < 0).any() and (bo[:, 0] >= 0).all()
    same((dd, ii, cc), reference(oracle, d, bo, k, metric, fo), f"search_union_filtered {metric}")


def tree_index(capi, metric="ip"):
    """test_gpu_union.py's 2-level [4, 3] tree over synthetic_tree's objects."""
    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    idx = capi.Index(0, metric=metric)
    idx.set_mlp(root)
    for i, (_, layers) in enumerate(internal):
        idx.nav_set_model(i + 1, layers)
    idx.nav_set_tree([0, 4, 7, 10, 13, 16], [1, 2, 3, 4] + [-1] * 12, [-2] * 4 + list(range(12)))
    lab = dp[:, 0] * 3 + dp[:, 1]
    ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    idx.set_buckets(Xs, lab, 12, ids=ids)
    return idx, Xs, lab, ids, Qn, Qs


@pytest.mark.parametrize("metric", ur.METRICS)
def test_search_tree_union_filtered_with_path_mass(capi, oracle, metric):
    idx, Xs, lab, ids, Qn, Qs = tree_index(capi, metric)
    rows, labs = ur.buckets_of(Xs, lab, ids, 12)
    lists, modes = [ids[ids % 3 == 0], ids[:40], labs[5]], (fr.KEEP, fr.DROP, fr.KEEP)
    allowed = fr.allowed_rows(lists, modes, labs)
    fo = (np.arange(Qn.shape[0]) % 4 - 1).astype(np.int32)
    filt = capi.Filter(idx, lists, modes)
    try:
        for nb, k, path_mass in ((5, 100, 0.0), (7, 100, 0.9)):
            idx.set_path_mass(path_mass)
            dd, ii, cc, slab, ent = idx.search_tree_union(Qn, Qs, nb, k, filter=filt, filter_of=fo)
            want_slab, want_ent = idx.nav_order(Qn, nb)
            np.testing.assert_array_equal(slab, want_slab)
            np.testing.assert_array_equal(ent, want_ent)
            assert path_mass == 0 or (slab < 0).any()
            same((dd, ii, cc), fr.union_filter_ref(oracle, rows, labs, slab, Qs, k, metric, allowed, fo), f"tree {metric} nb={nb} mass={path_mass}")
    finally:
        filt.close()
        idx.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_device_pointers_equal_host_pointers(index_of, metric):
    d, nb, k = 136, 8, 129
    (idx, filt), Q = index_of(d, metric), ur.case(d)[1]
    order, fo = ur.random_order(nb), fr.filter_of()
    host = idx.scan_union(Q, order, k, filter=filt, filter_of=fo)
    q_t, bo_t = torch.from_numpy(np.array(Q)).cuda(), torch.from_numpy(order).cuda()
    d_t = torch.empty((ur.NQ, k), dtype=torch.float32, device="cuda")
    i_t = torch.empty((ur.NQ, k), dtype=torch.int32, device="cuda")
    c_t = torch.empty((ur.NQ,), dtype=torch.int32, device="cuda")
    idx.scan_union_device(q_t, bo_t, nb, k, d_t, i_t, c_t, filter=filt, filter_of=fo)   # filter_of stays on the host
    same((d_t, i_t, c_t), host, "scan_union_device")
    hs = idx.search_union(Q, Q, nb, k, filter=filt, filter_of=fo)
    d_t.fill_(0), i_t.fill_(0), c_t.fill_(0)
    bo_o = torch.empty((ur.NQ, nb), dtype=torch.int32, device="cuda")
    idx.search_union_device(q_t, q_t, nb, k, d_t, i_t, c_t, bo_o, filter=filt, filter_of=fo)
    same((d_t, i_t, c_t), hs, "search_union_device")
    np.testing.assert_array_equal(bo_o.cpu().numpy(), hs[3])


def test_a_clone_view_takes_its_parents_filter(capi, index_of, oracle):
    d, nb, k, metric = 64, 8, 10, "ip"
    (idx, filt), Q = index_of(d, metric), ur.case(d)[1]
    order, fo = ur.random_order(nb), fr.filter_of()
    want = reference(oracle, d, order, k, metric, fo)
    view = idx.clone_view()
    try:
        same(view.scan_union(Q, order, k, filter=filt, filter_of=fo), want, "the parent's filter on the view")
        mine = capi.Filter(view, fr.filter_lists(d), fr.MODES)   # and one made on the view fits the parent
        try:
            same(idx.scan_union(Q, order, k, filter=mine, filter_of=fo), want, "the view's filter on the parent")
        finally:
            mine.close()
    finally:
        view.close()


@pytest.mark.parametrize("metric", ur.METRICS)
def test_a_layout_change_makes_a_filter_stale(capi, oracle, metric):
    """After lmi_buckets_insert, and on lmi_subset's output, the old filter is refused by name; one made afterwards answers like the
    reference on the index as it is now."""
    d, nb, k = 45, 8, 100
    X, Q, lab, ids = ur.case(d)
    first = np.arange(ur.N) < 5000
    order = ur.random_order(nb)
    fo = (np.arange(ur.NQ) % 3 - 1).astype(np.int32)
    lists, modes = [ids[ids % 2 == 0], ids[::5]], (fr.KEEP, fr.DROP)
    idx = build(capi, X[first], lab[first], ids[first], metric=metric)
    old = capi.Filter(idx, lists, modes)
    sub = None
    try:
        rows, labs = ur.buckets_of(X[first], lab[first], ids[first])
        same(idx.scan_union(Q, order, k, filter=old, filter_of=fo),
             fr.union_filter_ref(oracle, rows, labs, order, Q, k, metric, fr.allowed_rows(lists, modes, labs), fo), "before the insert")
        sub = idx.subset(ids[::2])
        with pytest.raises(capi.LmiError, match="stale"):
            sub.scan_union(Q, order, k, filter=old, filter_of=fo)
        assert idx.insert(np.ascontiguousarray(X[~first]), lab[~first], ids[~first]) == 1000
        with pytest.raises(capi.LmiError, match="stale"):
            idx.scan_union(Q, order, k, filter=old, filter_of=fo)
        assert capi.filter_last_plan()["FILTERS"] == 0
        new = capi.Filter(idx, lists, modes)
        try:
            rows, labs = ur.buckets_of(X, lab, ids)   # object order: the build's, then the inserted
            same(idx.scan_union(Q, order, k, filter=new, filter_of=fo),
                 fr.union_filter_ref(oracle, rows, labs, order, Q, k, metric, fr.allowed_rows(lists, modes, labs), fo), "after the insert")
            assert idx.delete(ids[:10]) == 10
            with pytest.raises(capi.LmiError, match="stale"):
                idx.scan_union(Q, order, k, filter=new, filter_of=fo)
        finally:
            new.close()
    finally:
        old.close()
        if sub is not None:
            sub.close()
        idx.close()


def test_refusals(capi, index_of):
    lib = capi.lib()
    X, Q, lab, ids = ur.case(64)
    order = ur.random_order(3)
    idx, filt = index_of(64, "ip")
    err = lambda: lib.lmi_last_error().decode()
    d = np.empty((ur.NQ, 10), np.float32)
    i = np.empty((ur.NQ, 10), np.uint32)
    scan = lambda h, k, f, fo, nq=ur.NQ: lib.lmi_scan_union_filtered(h, Q.ctypes.data, nq, order.ctypes.data, 3, k, d.ctypes.data, i.ctypes.data, None, 0,
                                                                      f, None if fo is None else fo.ctypes.data)
    # the filtered calls: a NULL filter (also with no queries), a filter_of entry outside [-1, nf), what union_check refuses
    assert scan(idx._h, 10, None, None) != 0 and "NULL filter" in err()
    assert scan(idx._h, 10, None, None, nq=0) != 0 and "NULL filter" in err()
    for bad in (fr.NF, -2):
        fo = np.zeros(ur.NQ, np.int32)
        fo[77] = bad
        assert scan(idx._h, 10, filt._f, fo) != 0 and "filter_of[77]" in err()
        assert capi.filter_last_plan()["FILTERS"] == 0
    for k in (0, 1025):
        assert scan(idx._h, k, filt._f, None) != 0 and "outside [1,1024]" in err()
    assert scan(idx._h, 10, filt._f, None, nq=0) == 0
    bo = np.empty((ur.NQ, 3), np.int32)
    assert lib.lmi_search_union_filtered(idx._h, Q.ctypes.data, Q.ctypes.data, ur.NQ, 3, 10, d.ctypes.data, i.ctypes.data, None, bo.ctypes.data, 0,
                                         None, None) != 0 and "NULL filter" in err()
    assert lib.lmi_search_tree_union_filtered(idx._h, Q.ctypes.data, Q.ctypes.data, ur.NQ, 3, 10, d.ctypes.data, i.ctypes.data, None, None, None, 0,
                                              None, None) != 0 and "NULL filter" in err()
    # a foreign filter: made on another index of the very same contents
    other = build(capi, X, lab, ids)
    try:
        with pytest.raises(capi.LmiError, match="stale"):
            other.scan_union(Q, order, 10, filter=filt)
    finally:
        other.close()
    # the stored forms the union scan does not read: a filter can be made, the scan is refused as its parent is
    for kw in (dict(prefilter=False), dict(storage="f16")):
        Xh = X.astype(np.float16).astype(np.float32) if "storage" in kw else X
        h = build(capi, Xh, lab, ids, layers=ur.layers_for(64, ur.L, 3), **kw)
        f = capi.Filter(h, fr.filter_lists(64), fr.MODES)
        try:
            np.testing.assert_array_equal(f.counts(), filt.counts())
            with pytest.raises(capi.LmiError, match="row-major"):
                h.scan_union(Q, order, 10, filter=f)
            with pytest.raises(capi.LmiError, match="row-major"):
                h.search_union(Q, Q, 3, 10, filter=f)
        finally:
            f.close()
            h.close()
    # lmi_filter_create
    out = ctypes.c_void_p()
    some = np.asarray([5, 3, 3], np.uint32)

    def create(h, off, nf, modes):
        off_a, modes_a = np.asarray(off, np.int64), np.asarray(modes, np.int32)   # (alive across the call)
        return lib.lmi_filter_create(h, some.ctypes.data, off_a.ctypes.data, nf, modes_a.ctypes.data, ctypes.byref(out))

    empty = capi.Index(0)
    try:
        assert create(empty._h, [0, 3], 1, [0]) != 0 and "not built" in err() and not out
    finally:
        empty.close()
    assert create(None, [0, 3], 1, [0]) != 0 and "NULL handle" in err()
    for nf in (0, 1025, -1):
        assert create(idx._h, [0] * 1026, nf, [0] * 1025) != 0 and "nf outside [1,1024]" in err() and not out
    assert create(idx._h, [0, 3, 2], 2, [0, 0]) != 0 and "non-decreasing" in err()
    assert create(idx._h, [1, 3], 1, [0]) != 0 and "offsets[0]" in err()
    assert create(idx._h, [0, 2 ** 31], 1, [0]) != 0 and "2^31" in err()
    assert create(idx._h, [0, 2, 3], 2, [0, 2]) != 0 and "mode" in err() and not out
    assert lib.lmi_filter_destroy(None) == 0


@pytest.mark.parametrize("metric", ur.METRICS)
def test_ordinary_calls_are_unchanged_by_a_filtered_call(index_of, metric):
    d, nb = 64, 4
    (idx, filt), Q = index_of(d, metric), ur.case(d)[1]
    order = ur.random_order(8)
    before = idx.search(Q, Q, nb, 10, want_keys=True), idx.scan_union(Q, order, 129)
    idx.search_union(Q, Q, nb, 1024, filter=filt, filter_of=fr.filter_of())
    idx.scan_union(Q, order, 129, filter=filt)
    after = idx.search(Q, Q, nb, 10, want_keys=True), idx.scan_union(Q, order, 129)
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


def test_li_api_one_level(capi, oracle):
    """li.LearnedIndex.search(merge="union", filter=id list) on a 1-level index: the reference on the engine's bucket order; then a
    Filter of the caller's with filter_of."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    root, _, _, dp2, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    rs = np.random.RandomState(2)
    dp = rs.randint(0, 4, size=(Xn.shape[0], 1)).astype(np.int64)
    li = LearnedIndex(net_from(root), {}, [(b,) for b in range(4)])
    all_ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    keep = all_ids[all_ids % 4 == 1]
    rows, labs = ur.buckets_of(Xs, dp[:, 0], all_ids, 4)
    for metric in ur.METRICS:
        dists, nns, _ = li.search(frame(Xn), Qn, frame(Xs), Qs, dp, [4], n_buckets=3, k=100, metric=metric, merge="union", filter=keep,
                                  stop_rows=1800)
        eng = li._engine
        eng.set_stop_rows(1800)
        bo = eng.mlp_topk(Qn, 3)
        eng.set_stop_rows(0)
        assert (bo < 0).any()
        want = fr.union_filter_ref(oracle, rows, labs, bo, Qs, 100, metric, fr.allowed_rows([keep], [fr.KEEP], labs), None)
        assert dists.dtype == np.float64 and dists.shape == nns.shape == (Qn.shape[0], 100)
        np.testing.assert_array_equal(nns, want[1])
        np.testing.assert_array_equal(dists.astype(np.float32).view(np.uint32), want[0].view(np.uint32))
        filt = capi.Filter(eng, [keep, all_ids[:100]], ["keep", "drop"])
        fo = (np.arange(Qn.shape[0]) % 3 - 1).astype(np.int32)
        try:
            d2, n2, _ = li.search_resident(Qn, Qs, [4], n_buckets=3, k=100, merge="union", filter=filt, filter_of=fo, stop_rows=1800)
        finally:
            filt.close()
        want2 = fr.union_filter_ref(oracle, rows, labs, bo, Qs, 100, metric, fr.allowed_rows([keep, all_ids[:100]], [fr.KEEP, fr.DROP], labs), fo)
        np.testing.assert_array_equal(n2, want2[1])
        with pytest.raises(ValueError, match="filter"):
            li.search_resident(Qn, Qs, [4], n_buckets=3, k=10, filter=keep)


def test_li_api_two_levels(oracle):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
    all_ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    keep = all_ids[all_ids % 3 != 0]
    dists, nns, _ = li.search(frame(Xn), Qn, frame(Xs), Qs, dp, [4, 3], n_buckets=5, k=100, merge="union", filter=keep)
    slab, _ = li._engine.nav_order(Qn, 5)
    n_slab = len(li._path_ids)
    lab = np.asarray([li._path_ids[tuple(int(v) for v in p)] for p in dp])
    rows, labs = ur.buckets_of(Xs, lab, all_ids, n_slab)
    want = fr.union_filter_ref(oracle, rows, labs, slab, Qs, 100, "ip", fr.allowed_rows([keep], [fr.KEEP], labs), None)
    assert dists.shape == nns.shape == (Qn.shape[0], 100)
    np.testing.assert_array_equal(nns, want[1])
    np.testing.assert_array_equal(dists.astype(np.float32).view(np.uint32), want[0].view(np.uint32))
