"""GPU (`-m gpu`): a built index re-bucketed on the device (lmi_regroup, Index.regroup, LearnedIndex.regroup,
LearnedIndex.insert(create_buckets=True)).

Contract (include/lmi_hip.h, "the order rule"): the new handle holds exactly what a fresh build of "the parent's objects in the order
the parent holds them, each with its new label" holds.  "Equals fresh" is test_gpu_subset.py's: equality -- no tolerance anywhere -- of
dists (bit patterns), ids and keys for (n_buckets, k) in (1, 10), (3, 10), (4, 30), of bucket_sizes, of read_bucket's rows and ids for
every bucket, of debug_layout (all four counters zero) and of index_bytes.  The reference object list is tests/regroup_ref.py's:
`perm = np.argsort(old_labels, kind="stable")` applied to (X, new labels, ids); `Mirror` keeps the objects in arrival order, for which
that permutation IS the resident order."""
import ctypes

import numpy as np
import pytest

import regroup_ref as rr
from test_gpu_mutate import Mirror, dataset, fresh, mlp
from test_gpu_subset import FORCED, MODES, NBK, L, N, answers, data, half_exact, new_ids, same_answers

pytestmark = pytest.mark.gpu

L_NEW = 17


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def same_buckets(a, b, n_buckets, dtype=np.float32):
    np.testing.assert_array_equal(a.bucket_sizes(), b.bucket_sizes())
    for bkt in range(n_buckets):
        r1, i1 = a.read_bucket(bkt, dtype=dtype)
        r2, i2 = b.read_bucket(bkt, dtype=dtype)
        assert np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), bkt
        assert np.array_equal(i1, i2), bkt


def expected(m, new_lab):
    """The object list a fresh build of which the regrouped index equals."""
    return Mirror(*rr.regrouped(m.X, m.lab, m.ids, new_lab))


def equals_fresh(capi, out, layers, want, Q, n_buckets, f16=False, **kw):
    """`out` (with `layers` set on it) against a fresh build of the object list `want` under the same settings."""
    assert out.L == n_buckets and out.N == want.ids.size
    ref = fresh(capi, layers, want, n_buckets, **kw)
    try:
        same_answers(answers(out, Q), answers(ref, Q))
        same_buckets(out, ref, n_buckets)
        for bkt in range(n_buckets):   # ... which are the objects themselves, in (old bucket, old row) order
            rows, bid = out.read_bucket(bkt)
            np.testing.assert_array_equal(rows, want.X[want.lab == bkt])
            np.testing.assert_array_equal(bid, want.ids[want.lab == bkt])
        la, lb = out.debug_layout(), ref.debug_layout()
        np.testing.assert_array_equal(la["rb_start"], lb["rb_start"])
        np.testing.assert_array_equal(la["cap_rb"], lb["cap_rb"])
        assert la["n_rb_total"] == lb["n_rb_total"]
        assert not la["counters"].any() and not lb["counters"].any()
        assert out.index_bytes() == ref.index_bytes()
        if f16:
            same_buckets(out, ref, n_buckets, dtype=np.float16)
            wide = fresh(capi, layers, want, n_buckets)   # the same rows in an LMI_STORAGE_F32 index
            try:
                same_answers(answers(out, Q), answers(wide, Q))
                same_buckets(out, wide, n_buckets)
            finally:
                wide.close()
    finally:
        ref.close()


def split_and_move(m, rs):
    """Test 1's re-labelling: the 2 500-row bucket split over new buckets 12..15, a random 30 % of the rest moved to random buckets
    of 0..15, bucket 16 left empty.  (new labels [N], the named objects' positions in shuffled order)"""
    big = next(b for b, n in FORCED.items() if n == 2500)
    new_lab = m.lab.copy()
    inside = np.flatnonzero(m.lab == big)
    new_lab[inside] = 12 + rs.randint(0, 4, inside.size)
    rest = np.flatnonzero(m.lab != big)
    moved = rest[rs.rand(rest.size) < 0.3]
    new_lab[moved] = rs.randint(0, 16, moved.size)
    named = np.concatenate([inside, moved])
    return new_lab, named[rs.permutation(named.size)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [45, 768])
@pytest.mark.parametrize("mode", list(MODES))
def test_equals_fresh_across_modes_and_dimensions(capi, mode, d):
    f16 = mode == "f16"
    m, layers, Q = data(d, f16)
    rs = np.random.RandomState(100 + d + len(mode))
    new_lab, named = split_and_move(m, rs)
    parent = fresh(capi, layers, m, L, **MODES[mode])
    before = answers(parent, Q)
    out = parent.regroup(m.ids[named], new_lab[named], L_NEW)
    assert out.storage == parent.storage and out.metric == "ip" and out.L == L_NEW and out.d == d and out.n_named == named.size
    plan = capi.regroup_last_plan()
    assert plan["rows"] == N and plan["tiles"] == 1 and plan["passes"] == 0 and plan["named"] == named.size   # one tile holds 6 000 words
    sizes = out.bucket_sizes()
    assert sizes[16] == 0 and sizes[12:16].sum() >= 2500 and sizes.sum() == N
    layers17 = mlp(rs, d, L_NEW)
    with pytest.raises(capi.LmiError, match="classes"):   # the parent's 12-class root model came along and no longer fits
        out.search(Q, Q, 3, 10)
    out.set_mlp(layers17)
    equals_fresh(capi, out, layers17, expected(m, new_lab), Q, L_NEW, f16=f16, **MODES[mode])
    same_answers(answers(parent, Q), before)   # the call only read the parent
    out.close()
    parent.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["merge", "reverse", "fewer"])
def test_map_only(capi, case):
    d = 64
    m, layers, Q = data(d)
    rs = np.random.RandomState(2)
    bmap, n_new = {"merge": (np.where(np.isin(np.arange(L), (7, 9)), 2, np.arange(L)), L),
                   "reverse": (L - 1 - np.arange(L), L),
                   "fewer": (np.arange(L) % 5, 5)}[case]
    parent = fresh(capi, layers, m, L)
    old = [parent.read_bucket(b)[1] for b in range(L)]
    out = parent.regroup([], [], n_new, bucket_map=bmap)
    assert out.n_named == 0
    for nb in range(n_new):   # a new bucket holds its old buckets one after the other, in ascending old id
        np.testing.assert_array_equal(out.read_bucket(nb)[1], np.concatenate([old[b] for b in range(L) if bmap[b] == nb] + [np.empty(0, np.uint32)]))
    if case == "merge":
        np.testing.assert_array_equal(out.read_bucket(2)[1], np.concatenate([old[2], old[7], old[9]]))
        assert out.bucket_sizes()[7] == out.bucket_sizes()[9] == 0
    new_layers = mlp(rs, d, n_new)
    out.set_mlp(new_layers)
    equals_fresh(capi, out, new_layers, expected(m, bmap[m.lab]), Q, n_new)
    out.close()
    parent.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_mutated_parent(capi):
    """Inserts relocate a bucket behind later ones and deletes leave holes: the slab row no longer follows the parent's order, which
    a regroup that took the slab row for the ordinal would show here."""
    d = 128
    m0, layers, Q = data(d)
    rs = np.random.RandomState(3)
    m = Mirror(m0.X, m0.lab, m0.ids)
    parent = fresh(capi, layers, m, L)
    size7 = int(parent.bucket_sizes()[7])
    for j, (b, n) in enumerate(((7, 3 * size7 + 77), (1, 40))):   # a growth re-pack with headroom, then a relocation into it
        xb = dataset(rs, n, d)
        ib = new_ids(10_000 * j, n)
        parent.insert(xb, np.full(n, b), ib)
        m.insert(xb, np.full(n, b), ib)
    gone = np.concatenate([m.ids[::4], m.ids[m.lab == 8]])
    assert parent.delete(gone) == m.delete(gone)
    lay = parent.debug_layout()
    assert lay["counters"][1] > 0, "no bucket was relocated"
    assert lay["n_rb_total"] > int(np.sum((parent.bucket_sizes() + 31) // 32)), "the parent holds no slack or hole"
    assert lay["rb_start"][1] > lay["rb_start"][2:L].max(), "bucket 1 does not lie behind the later buckets: slab order is bucket order"
    same = parent.regroup([], [], L)             # the identity: the parent's compaction
    full = parent.subset([], drop=True)
    same_answers(answers(same, Q), answers(full, Q))
    same_buckets(same, full, L)
    np.testing.assert_array_equal(same.debug_layout()["rb_start"], full.debug_layout()["rb_start"])
    equals_fresh(capi, same, layers, expected(m, m.lab), Q, L)
    full.close()
    same.close()
    named = np.flatnonzero(rs.rand(m.ids.size) < 0.5)
    new_lab = m.lab.copy()
    new_lab[named] = rs.randint(0, L_NEW, named.size)
    out = parent.regroup(m.ids[named][::-1], new_lab[named][::-1], L_NEW)
    layers17 = mlp(rs, d, L_NEW)
    out.set_mlp(layers17)
    equals_fresh(capi, out, layers17, expected(m, new_lab), Q, L_NEW)
    out.close()
    parent.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_l2(capi):
    d = 45
    m0, layers, Q = data(d)
    rs = np.random.RandomState(4)
    m = Mirror(m0.X * rs.uniform(0.2, 3.0, (N, 1)).astype(np.float32), m0.lab, m0.ids)   # norms that matter
    new_lab, named = split_and_move(m, rs)
    parent = fresh(capi, layers, m, L, metric="l2")
    out = parent.regroup(m.ids[named], new_lab[named], L_NEW)
    assert out.metric == "l2"
    layers17 = mlp(rs, d, L_NEW)
    out.set_mlp(layers17)
    equals_fresh(capi, out, layers17, expected(m, new_lab), Q, L_NEW, metric="l2")
    out.close()
    parent.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_shared_ids_absent_ids_and_the_named_count(capi):
    d = 45
    m0, layers, Q = data(d)
    rs = np.random.RandomState(5)
    ids = m0.ids.copy()
    a, b = np.flatnonzero(m0.lab == 5)[3], np.flatnonzero(m0.lab == 9)[0]
    ids[b] = ids[a]                              # two objects of different buckets carry one id
    m = Mirror(m0.X, m0.lab, ids)
    absent = np.asarray([1, 2, 3, 2 ** 32 - 1], dtype=np.uint32)
    assert not np.isin(absent, ids).any()
    pick = np.flatnonzero(rs.rand(N) < 0.1)
    pick = np.unique(np.concatenate([pick[pick != b], [a]]))      # the shared id is listed once
    list_ids = np.concatenate([absent[:2], ids[pick], absent[2:]])
    list_lab = np.concatenate([[0, 1], rs.randint(0, L_NEW, pick.size), [2, 3]])
    new_lab, named = rr.new_labels(m.lab, ids, list_ids, list_lab)
    assert named == pick.size + 1 and new_lab[a] == new_lab[b]
    parent = fresh(capi, layers, m, L)
    out = parent.regroup(list_ids, list_lab, L_NEW)
    assert out.n_named == named and capi.regroup_last_plan()["named"] == named
    layers17 = mlp(rs, d, L_NEW)
    out.set_mlp(layers17)
    equals_fresh(capi, out, layers17, expected(m, new_lab), Q, L_NEW)
    out.close()
    parent.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_sort_seams_and_forced_geometries(capi):
    """20 000 objects are more than one tile of 8 192 words: tiles and merge passes.  Every forced tile length gives the same index."""
    d, n, n_old, n_new = 45, 20_000, 9, 23
    rs = np.random.RandomState(6)
    X = dataset(rs, n, d)
    lab = rs.randint(0, n_old, n)
    ids = (rs.permutation(2 ** 20)[:n].astype(np.uint64) * 4093 + 7).astype(np.uint32)
    m = Mirror(X, lab, ids)
    layers, layers_new = mlp(rs, d, n_old), mlp(rs, d, n_new)
    Q = dataset(rs, 64, d)
    new_lab = rs.randint(0, n_new, n)            # a complete re-placement
    order = rs.permutation(n)
    parent = fresh(capi, layers, m, n_old)
    want = expected(m, new_lab)
    seen = []
    try:
        for tile_rows, tiles, passes in ((0, 3, 2), (8192, 3, 2), (1024, 20, 5), (64, 313, 9)):
            capi.regroup_set_geometry(tile_rows)
            out = parent.regroup(ids[order], new_lab[order], n_new)
            plan = capi.regroup_last_plan()
            assert plan["rows"] == n and plan["tile_rows"] == (tile_rows or 8192) and plan["tiles"] == tiles and plan["passes"] == passes, plan
            assert plan["merge_rows"] == min(2048, tile_rows or 8192) and plan["map_bytes"] >= 20 * n and out.n_named == n
            out.set_mlp(layers_new)
            seen.append([out.read_bucket(b) for b in range(n_new)] + [out.debug_layout()["rb_start"]])
            if tile_rows in (0, 64):
                equals_fresh(capi, out, layers_new, want, Q, n_new)
            out.close()
    finally:
        capi.regroup_set_geometry(0)
    for other in seen[1:]:
        for x, y in zip(seen[0][:-1], other[:-1]):
            assert np.array_equal(x[0].view(np.uint32), y[0].view(np.uint32)) and np.array_equal(x[1], y[1])
        np.testing.assert_array_equal(seen[0][-1], other[-1])
    parent.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_union_and_range_scans(capi):
    d = 64
    m, layers, Q = data(d)
    rs = np.random.RandomState(7)
    new_lab, named = split_and_move(m, rs)
    parent = fresh(capi, layers, m, L)
    out = parent.regroup(m.ids[named], new_lab[named], L_NEW)   # no model is set: the explicit-order calls work at once
    ref = fresh(capi, mlp(rs, d, L_NEW), expected(m, new_lab), L_NEW)
    order = np.stack([rs.permutation(L_NEW)[:4] for _ in range(Q.shape[0])]).astype(np.int32)
    order[::5, 3] = -1
    d1, i1, c1 = out.scan_union(Q, order, 100)[:3]
    d2, i2, c2 = ref.scan_union(Q, order, 100)[:3]
    assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32)) and np.array_equal(i1, i2) and np.array_equal(c1, c2)
    radius = float(np.median(d1[:, 40]))
    l1, rd1, ri1 = out.scan_range(Q, order, radius)[:3]
    l2, rd2, ri2 = ref.scan_range(Q, order, radius)[:3]
    assert l1[-1] > 0 and np.array_equal(l1, l2) and np.array_equal(rd1.view(np.uint32), rd2.view(np.uint32)) and np.array_equal(ri1, ri2)
    for x in (out, ref, parent):
        x.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_independence(capi):
    d = 96
    m, layers, Q = data(d)
    rs = np.random.RandomState(8)
    new_lab, named = split_and_move(m, rs)
    layers17 = mlp(rs, d, L_NEW)
    want = expected(m, new_lab)
    parent = fresh(capi, layers, m, L)
    before = answers(parent, Q)
    flt = capi.Filter(parent, [m.ids[::2]])
    view = parent.clone_view()
    out = parent.regroup(m.ids[named], new_lab[named], L_NEW)        # while a clone view lives
    via = view.regroup(m.ids[named], new_lab[named], L_NEW)          # on the clone view itself
    assert len(parent._views) == 1 and out not in parent._views and via not in view._views
    for x in (out, via):
        x.set_mlp(layers17)
    same_answers(answers(out, Q), answers(via, Q))
    same_buckets(out, via, L_NEW)
    via.close()
    same_answers(answers(parent, Q), before)
    order = np.tile(np.arange(3, dtype=np.int32), (Q.shape[0], 1))
    parent.scan_union(Q, order, 10, filter=flt)                      # the parent's filter still fits the parent ...
    with pytest.raises(capi.LmiError, match="stale or belongs to another index"):
        out.scan_union(Q, order, 10, filter=flt)                     # ... and is foreign to the result
    flt.close()
    view.close()
    parent._views.remove(view)
    mine = answers(out, Q)
    # the parent is mutated: the result does not notice
    extra = dataset(rs, 700, d)
    parent.insert(extra, np.full(700, 2), new_ids(0, 700))
    parent.delete(m.ids[::3])
    same_answers(answers(out, Q), mine)
    # the result is mutated: the parent does not notice, and the result equals fresh
    theirs = answers(parent, Q)
    more, more_lab, more_ids = dataset(rs, 300, d), rs.randint(0, L_NEW, 300), new_ids(5000, 300)
    assert out.insert(more, more_lab, more_ids) == 300
    want.insert(more, more_lab, more_ids)
    gone = np.concatenate([want.ids[::7], more_ids[::2]])
    assert out.delete(gone) == want.delete(gone)
    same_answers(answers(parent, Q), theirs)
    ref = fresh(capi, layers17, want, L_NEW)
    same_answers(answers(out, Q), answers(ref, Q))
    same_buckets(out, ref, L_NEW)
    ref.close()
    mine = answers(out, Q)
    parent.close()                                                   # the parent goes first: the result owns its models and images
    same_answers(answers(out, Q), mine)
    out.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(capi):
    d = 45
    m, layers, Q = data(d)
    lib = capi.lib()
    LmiError = capi.LmiError
    ids = np.ascontiguousarray(m.ids[:10])
    lab = np.arange(10, dtype=np.int64)
    ident = np.arange(L, dtype=np.int32)

    def call(h, ids_a, lab_a, n, bmap, n_new, with_out=True):
        out, named = ctypes.c_void_p(), ctypes.c_int64(-1)
        rc = lib.lmi_regroup(h, None if ids_a is None else ids_a.ctypes.data, None if lab_a is None else lab_a.ctypes.data, n,
                             None if bmap is None else bmap.ctypes.data, n_new, ctypes.byref(out) if with_out else None, ctypes.byref(named))
        assert rc != 0 and not out.value and (named.value == 0 or not with_out)
        capi._check(rc)

    unbuilt = capi.Index(0)
    unbuilt.set_mlp(layers)
    with pytest.raises(LmiError, match="lmi_regroup.*not built"):
        call(unbuilt._h, ids, lab, 10, None, L)
    unbuilt.buckets_begin(m.lab, d, L, ids=m.ids)
    with pytest.raises(LmiError, match="lmi_regroup.*being built"):
        call(unbuilt._h, ids, lab, 10, None, L)
    unbuilt.close()
    owned = capi.Index(0)
    owned.set_mlp(layers)
    mask = (np.arange(L) % 2 == 0).astype(np.uint8)
    owned.buckets_begin(m.lab, d, L, ids=m.ids, owned=mask)
    mine = np.flatnonzero(mask[m.lab] == 1)
    owned.add_owned_rows(m.X[mine], mine)
    owned.buckets_end()
    with pytest.raises(LmiError, match="lmi_regroup.*`owned` mask"):
        call(owned._h, ids, lab, 10, None, L)
    owned.close()

    parent = fresh(capi, layers, m, L)
    before = answers(parent, Q)
    sizes = parent.bucket_sizes().copy()

    def refused(match, *args, **kw):
        with pytest.raises(LmiError, match=match):
            call(*args, **kw)
        assert capi.regroup_last_plan()["rows"] == 0
        same_answers(answers(parent, Q), before)
        np.testing.assert_array_equal(parent.bucket_sizes(), sizes)

    with pytest.raises(LmiError, match="lmi_regroup: NULL handle"):
        call(None, ids, lab, 10, None, L)
    refused("lmi_regroup: out is NULL", parent._h, ids, lab, 10, None, L, with_out=False)
    refused(r"lmi_regroup: L_new = 0 outside \[1, 1048576\)", parent._h, ids, lab, 10, None, 0)
    refused(r"lmi_regroup: L_new = 1048576 outside", parent._h, ids, lab, 10, None, 1 << 20)
    refused("lmi_regroup: bad arguments.*negative", parent._h, ids, lab, -1, None, L)
    refused("lmi_regroup: bad arguments.*required when n > 0", parent._h, None, lab, 10, None, L)
    refused("lmi_regroup: bad arguments.*required when n > 0", parent._h, ids, None, 10, None, L)
    refused(r"lmi_regroup: labels\[9\] = 9 outside \[0,9\)", parent._h, ids, lab, 10, ident % 9, 9)
    refused(r"lmi_regroup: labels\[0\] = -1 outside", parent._h, ids, lab - 1, 10, None, L)
    bad = ident.copy()
    bad[3] = -2
    refused(r"lmi_regroup: bucket_map\[3\] = -2 outside \[-1,12\)", parent._h, ids, lab, 10, bad, L)
    bad[3] = L
    refused(r"lmi_regroup: bucket_map\[3\] = 12 outside \[-1,12\)", parent._h, ids, lab, 10, bad, L)
    refused("lmi_regroup: a NULL bucket_map is the identity and needs L_new >= L", parent._h, ids, lab, 10, None, L - 1)
    twice = np.ascontiguousarray(np.concatenate([ids, ids[4:5]]))
    refused(f"lmi_regroup: id {int(ids[4])} is listed twice", parent._h, twice, np.arange(11, dtype=np.int64), 11, None, L)
    # after the labelling pass: a bucket mapped to -1 that the list does not empty
    emptied = ident.copy()
    emptied[4] = emptied[3] = -1
    in4 = np.ascontiguousarray(np.concatenate([m.ids[m.lab == 4][:-2], m.ids[m.lab == 3][1:]]))
    refused("lmi_regroup: bucket 3 maps to -1.*but 1 of its 33 objects are not in the list.*no index was made", parent._h, in4,
            np.zeros(in4.size, dtype=np.int64), in4.size, emptied, L)
    # the binding raises the same argument errors as ValueError, before the call
    with pytest.raises(ValueError, match="listed twice"):
        parent.regroup(twice, np.arange(11), L)
    # ... and once the list does empty them the call goes through
    in4 = np.concatenate([m.ids[m.lab == 4], m.ids[m.lab == 3]])
    out = parent.regroup(in4, np.zeros(in4.size, dtype=np.int64), L, bucket_map=emptied)
    assert out.n_named == 2533 and out.bucket_sizes()[0] == 2533 and out.bucket_sizes()[3] == out.bucket_sizes()[4] == 0
    out.close()
    same_answers(answers(parent, Q), before)
    parent.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def li_frames(X, ids):
    import pandas as pd

    return pd.DataFrame(X, index=ids.astype(np.int64))


def same_li_answers(a, b, Qn, Qs, ncat, cases=((1, 10), (3, 10), (5, 10))):
    for nb, k in cases:
        d1, n1, _ = a.search_resident(Qn, Qs, ncat, nb, k)
        d2, n2, _ = b.search_resident(Qn, Qs, ncat, nb, k)
        assert np.array_equal(n1, n2) and np.array_equal(d1, d2), (nb, k)
    d1, n1, _ = a.search_resident(Qn, Qs, ncat, 4, 50, merge="union")
    d2, n2, _ = b.search_resident(Qn, Qs, ncat, 4, 50, merge="union")
    assert np.array_equal(n1, n2) and np.array_equal(d1, d2), "union"


def test_li_one_level_replacement_under_a_new_root_model():
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import net_from

    d = 64
    m, layers, Q = data(d)
    rs = np.random.RandomState(10)
    root = net_from(mlp(rs, d, L, hidden=128))
    frame = li_frames(m.X, m.ids)
    li = LearnedIndex(root, {}, [(i,) for i in range(L)])
    li.prepare(frame, frame, m.lab, [L])
    new_root = net_from(mlp(rs, d, 15, hidden=128))
    new_lab = new_root.predict(m.X)                                  # the complete re-placement: every object by the new model
    order = rs.permutation(N)
    out = li.regroup(m.ids[order], new_lab[order][:, None], root_model=new_root)
    assert out is not li and out._engine is not li._engine and out._engine.L == 15 and out._engine.n_named == N
    assert out.root_model is new_root and li.root_model is root and li._engine.L == L
    perm = rr.resident_order(m.lab)
    ref = LearnedIndex(new_root, {}, [(i,) for i in range(15)])
    ref.prepare(li_frames(m.X[perm], m.ids[perm]), li_frames(m.X[perm], m.ids[perm]), new_lab[perm], [15])
    same_li_answers(out, ref, Q, Q, [15])
    radius = float(np.median(ref.search_resident(Q, Q, [15], 3, 50, merge="union")[0][:, 20]))
    l1, d1, n1, _ = out.range_search_resident(Q, Q, [15], radius, n_buckets=3)
    l2, d2, n2, _ = ref.range_search_resident(Q, Q, [15], radius, n_buckets=3)
    assert l1[-1] > 0 and np.array_equal(l1, l2) and np.array_equal(d1, d2) and np.array_equal(n1, n2)
    li.close()                                                       # the source may go first
    same_li_answers(out, ref, Q, Q, [15], cases=((3, 10),))
    out.close()
    ref.close()


# ---- 11 -----------------------------------------------------------------------------------------------------------------------
def two_level():
    from path_mass_ref import synthetic_tree
    from test_gpu_path_mass import frame, net_from

    ncat = [4, 3]
    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree(ncat)
    models = net_from(root), {tuple(p): net_from(lay) for p, lay in internal}
    return ncat, models, bucket_paths, dp, frame(Xn), frame(Xs), Qn, Qs


def test_li_two_level_split_a_leaf_a_level_deeper(tmp_path):
    from learnedmetricindex_amd import index_io
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from learnedmetricindex_amd.li.PriorityQueue import EMPTY_VALUE as E
    from test_gpu_path_mass import net_from

    ncat, (root, internal), bucket_paths, dp, nav, srch, Qn, Qs = two_level()
    rs = np.random.RandomState(11)
    li = LearnedIndex(root, internal, bucket_paths)
    li.prepare(nav, srch, dp, ncat)
    leaf = (2, 1)
    inside = np.flatnonzero((dp == leaf).all(axis=1))
    assert inside.size > 50
    child = net_from(mlp(rs, nav.shape[1], 2, hidden=128))           # the hand-made child model of the split leaf
    c = child.predict(nav.to_numpy(dtype=np.float32)[inside])
    assert 0 < c.sum() < inside.size, "the child model sends everything one way"
    dp3 = np.concatenate([dp, np.full((dp.shape[0], 1), E, dtype=np.int64)], axis=1)
    dp3[inside, 2] = c
    internal3 = {tuple(p) + (E,): net for p, net in internal.items()}
    internal3[leaf + (E,)] = child
    paths3 = [tuple(p) + (E,) for p in bucket_paths if tuple(p) != leaf] + [leaf + (0,), leaf + (1,)]
    ncat3 = ncat + [2]
    ids = nav.index.to_numpy()
    out = li.regroup(ids[inside][::-1], dp3[inside][::-1], internal_models=internal3, bucket_paths=paths3)
    assert out._engine.n_named == inside.size and out._engine.L == li._engine.L + 2
    assert out._engine.bucket_sizes()[out._path_ids[leaf + (E,)]] == 0       # the old leaf stays, as an empty bucket
    # the frames-built equivalent: the same objects in the order the source holds them
    _, old_bucket = np.unique(dp, axis=0, return_inverse=True)
    perm = rr.resident_order(np.asarray(old_bucket).reshape(-1))
    ref = LearnedIndex(root, internal3, paths3)
    ref.prepare(nav.iloc[perm], srch.iloc[perm], dp3[perm], ncat3)
    same_li_answers(out, ref, Qn, Qs, ncat3)
    d0, n0, _ = li.search_resident(Qn, Qs, ncat, 5, 10)              # the source still answers as a [4, 3] tree
    assert d0.shape[0] == Qn.shape[0]
    # ... and it round-trips through index_io like any mutated index
    index_io.save_index(str(tmp_path / "regrouped"), out, ncat3)
    back, ncat_back = index_io.load_index(str(tmp_path / "regrouped"))
    assert ncat_back == ncat3
    same_li_answers(back, ref, Qn, Qs, ncat3, cases=((1, 10), (5, 10)))
    for x in (back, out, ref, li):
        x.close()


def test_li_insert_create_buckets():
    import pandas as pd

    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    ncat, (root, internal), bucket_paths, dp, nav, srch, Qn, Qs = two_level()
    rs = np.random.RandomState(12)
    li = LearnedIndex(root, internal, bucket_paths)
    li.prepare(nav, srch, dp, ncat)
    # objects that the models place under node 1 on a listed child that holds no bucket (only (1, 0) does)
    Xn = rs.randn(600, nav.shape[1]).astype(np.float32)
    r = root.predict(Xn)
    c = internal[(1, -1)].predict(Xn)
    pick = np.flatnonzero((r == 1) & (c != 0))[:40]
    assert pick.size >= 5 and len({(1, int(v)) for v in c[pick]} - set(li._path_ids)) >= 1
    new_ids_ = np.arange(pick.size, dtype=np.int64) + 10 ** 6
    new_nav = pd.DataFrame(Xn[pick], index=new_ids_)
    new_srch = pd.DataFrame(rs.randn(pick.size, srch.shape[1]).astype(np.float32), index=new_ids_)
    L0, before = li._engine.L, li.search_resident(Qn, Qs, ncat, 5, 10)
    with pytest.raises(ValueError, match=r"fall on a leaf path that holds no bucket; creating buckets is not supported \(rebuild the "
                                         r"index\): nothing was inserted"):
        li.insert(new_nav, new_srch)
    after = li.search_resident(Qn, Qs, ncat, 5, 10)
    assert li._engine.L == L0 and np.array_equal(before[1], after[1]) and np.array_equal(before[0], after[0])
    placed = li.insert(new_nav, new_srch, create_buckets=True)
    assert np.array_equal(placed, np.stack([r[pick], c[pick]], axis=1)) and li._engine.L > L0
    ref = LearnedIndex(root, internal, bucket_paths)
    ref.prepare(pd.concat([nav, new_nav]), pd.concat([srch, new_srch]), np.concatenate([dp, placed]), ncat)
    same_li_answers(li, ref, Qn, Qs, ncat)
    ours, theirs = li._engine.bucket_sizes(), ref._engine.bucket_sizes()
    np.testing.assert_array_equal(ours[ours > 0], theirs[theirs > 0])
    li.close()
    ref.close()


def test_the_split_recipe_of_the_integration_guide():
    """INTEGRATION.md, "Splitting an overfull bucket": read the bucket, cluster it, train a child model, place by the model, regroup."""
    from learnedmetricindex_amd.li.clustering import algorithms
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from learnedmetricindex_amd.li.model import NeuralNetwork
    from learnedmetricindex_amd.li.PriorityQueue import EMPTY_VALUE as E
    from test_gpu_path_mass import net_from

    d, n, n_buckets = 64, 5000, 8
    rs = np.random.RandomState(13)
    X = dataset(rs, n, d)
    ids = (rs.permutation(10 * n)[:n] + 1).astype(np.uint32)
    root = net_from(mlp(rs, d, n_buckets, hidden=128))
    lab = root.predict(X)
    Q = dataset(rs, 100, d)
    li = LearnedIndex(root, {}, [(i,) for i in range(n_buckets)])
    li.prepare(li_frames(X, ids), li_frames(X, ids), lab, [n_buckets])
    # 1: the overfull bucket's ids and rows, from the resident index
    b = int(np.argmax(li._engine.bucket_sizes()))
    rows, bucket_ids = li._engine.read_bucket(b)
    # 2: cluster them; 3: train a child model on the clusters; 4: place by the MODEL (what a later insert will do)
    _, clusters = algorithms["hip_kmeans"](rows, 2, {"seed": 2023, "niter": 10})
    child = NeuralNetwork(input_dim=d, output_dim=2, model_type="MLP")
    child.train_batch_hip(rows, clusters, epochs=20)
    placed = child.predict(rows)
    # 5: regroup: only the split bucket's objects are named
    paths = [(i, E) for i in range(n_buckets) if i != b] + [(b, 0), (b, 1)]
    out = li.regroup(bucket_ids, np.stack([np.full(placed.size, b), placed], axis=1), internal_models={(b, E): child}, bucket_paths=paths)
    sizes = out._engine.bucket_sizes()
    assert sizes.sum() == n and sizes[out._path_ids[(b, E)]] == 0
    assert sizes[out._path_ids[(b, 0)]] == (placed == 0).sum() and sizes[out._path_ids[(b, 1)]] == (placed == 1).sum()
    # the frames-built equivalent
    dp2 = np.stack([lab, np.full(n, E)], axis=1)
    row_of = {int(i): j for j, i in enumerate(ids)}
    dp2[[row_of[int(i)] for i in bucket_ids], 1] = placed
    perm = rr.resident_order(lab)
    ref = LearnedIndex(root, {(b, E): child}, paths)
    ref.prepare(li_frames(X[perm], ids[perm]), li_frames(X[perm], ids[perm]), dp2[perm], [n_buckets, 2])
    same_li_answers(out, ref, Q, Q, [n_buckets, 2])
    for x in (out, ref, li):
        x.close()
