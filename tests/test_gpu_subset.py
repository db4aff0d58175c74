"""GPU (`-m gpu`): a filtered, independent copy of a built index derived on the device (lmi_subset, Index.subset,
LearnedIndex.subset).

Contract: the new handle holds exactly what a fresh build of "every bucket's kept objects, in the order the parent holds them"
holds.  "Equals fresh" below is equality -- no tolerance anywhere -- of dists (bit patterns), ids and keys for (n_buckets, k) in
(1, 10), (3, 10), (4, 30), of bucket_sizes, of read_bucket's rows and ids for every bucket, of debug_layout (rb_start, cap_rb,
n_rb_total, all four counters zero), of index_bytes and of the kept count.  `Mirror` keeps the objects in their original order, so
filtering it IS that object list (a bucket's objects are held in ascending original row)."""
import numpy as np
import pytest

from test_gpu_mutate import Mirror, dataset, fresh, mlp

pytestmark = pytest.mark.gpu

L, N, NQ = 12, 6000, 128
NBK = ((1, 10), (3, 10), (4, 30))
MODES = {"f32": dict(), "exact": dict(prefilter=False), "f16": dict(storage="f16")}
# bucket sizes that are forced: empty, one row, exactly one row-block, one row past it, many row-blocks (several scan chunks)
FORCED = {0: 0, 1: 1, 2: 32, 3: 33, 4: 2500}


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def half_exact(X):
    return X.astype(np.float16).astype(np.float32)


_data = {}


def data(d, f16=False):
    """(Mirror of N objects with the forced bucket sizes in shuffled order, model, queries), made once per (d, f16) and never changed."""
    if (d, f16) not in _data:
        rs = np.random.RandomState(1000 + d)
        X = dataset(rs, N, d)
        rest = N - sum(FORCED.values())
        free = [b for b in range(L) if b not in FORCED]
        lab = np.concatenate([np.full(n, b) for b, n in FORCED.items()] + [np.asarray(free)[rs.randint(0, len(free), rest)]])
        lab = lab[rs.permutation(N)]
        ids = (rs.permutation(2 ** 20)[:N].astype(np.uint64) * 4093 + 7).astype(np.uint32)   # unique, up to 2^32: above 2^31 too
        assert np.unique(ids).size == N and ids.max() > 2 ** 31
        Q = dataset(rs, NQ, d)
        if f16:   # data as it is distributed in binary16 (max |x| < 1: the index scale only moves exponents up)
            X, Q = half_exact(X), half_exact(Q)
        for a in (X, lab, ids, Q):
            a.setflags(write=False)
        _data[(d, f16)] = (Mirror(X, lab, ids), mlp(rs, d, L), Q)
    return _data[(d, f16)]


def new_ids(start, n):
    """n ids that no object of data() carries (those are 7 mod 4093)."""
    return ((start + np.arange(n, dtype=np.uint64)) * 4093 + 8).astype(np.uint32)


def kept_of(m, ids, drop=False):
    hit = np.isin(m.ids, np.asarray(ids, dtype=np.uint32))
    keep = ~hit if drop else hit
    return Mirror(m.X[keep], m.lab[keep], m.ids[keep])


def answers(idx, Q):
    return [idx.search(Q, Q, nb, k, want_keys=True) for nb, k in NBK]


def same_answers(a, b):
    for (d1, i1, _, k1), (d2, i2, _, k2), nbk in zip(a, b, NBK):
        assert np.array_equal(i1, i2), nbk
        assert np.array_equal(d1.view(np.uint32), d2.view(np.uint32)), nbk
        assert np.array_equal(k1, k2), nbk


def same_buckets(a, b, dtype=np.float32):
    np.testing.assert_array_equal(a.bucket_sizes(), b.bucket_sizes())
    for bkt in range(L):
        r1, i1 = a.read_bucket(bkt, dtype=dtype)
        r2, i2 = b.read_bucket(bkt, dtype=dtype)
        assert np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), bkt
        assert np.array_equal(i1, i2), bkt


def equals_fresh(capi, sub, layers, kept, Q, f16=False, **kw):
    """`sub` against a fresh build of the object list `kept` with the same settings (and, for f16, against an F32 build too)."""
    assert sub.N == kept.ids.size
    ref = fresh(capi, layers, kept, L, **kw)
    try:
        same_answers(answers(sub, Q), answers(ref, Q))
        same_buckets(sub, ref)
        for bkt in range(L):   # ... which are the kept objects themselves
            rows, bid = sub.read_bucket(bkt)
            np.testing.assert_array_equal(rows, kept.X[kept.lab == bkt])
            np.testing.assert_array_equal(bid, kept.ids[kept.lab == bkt])
        la, lb = sub.debug_layout(), ref.debug_layout()
        np.testing.assert_array_equal(la["rb_start"], lb["rb_start"])
        np.testing.assert_array_equal(la["cap_rb"], lb["cap_rb"])
        assert la["n_rb_total"] == lb["n_rb_total"]
        assert not la["counters"].any() and not lb["counters"].any()
        assert sub.index_bytes() == ref.index_bytes()
        if f16:
            same_buckets(sub, ref, dtype=np.float16)
            wide = fresh(capi, layers, kept, L)   # the same rows in an LMI_STORAGE_F32 index
            try:
                same_answers(answers(sub, Q), answers(wide, Q))
                same_buckets(sub, wide)
            finally:
                wide.close()
    finally:
        ref.close()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [45, 768])
@pytest.mark.parametrize("mode", list(MODES))
def test_equals_fresh_across_modes_and_dimensions(capi, mode, d):
    """d = 45: the low-dimensional fragment shape, d % 8 != 0; d = 768: the 16 x 32 shape.  KEEP a random 40 %, plus all of one bucket,
    none of another and only the last row of a third."""
    f16 = mode == "f16"
    m, layers, Q = data(d, f16)
    rs = np.random.RandomState(d + len(mode))
    keep = rs.rand(N) < 0.4
    keep[m.lab == 5] = True
    keep[m.lab == 6] = False
    keep[m.lab == 3] = False
    keep[np.flatnonzero(m.lab == 3)[-1]] = True
    ids = m.ids[keep][rs.permutation(int(keep.sum()))]   # the list's order does not matter
    parent = fresh(capi, layers, m, L, **MODES[mode])
    sub = parent.subset(ids)
    assert sub.storage == parent.storage and sub.metric == "ip" and sub.L == L and sub.d == d
    sizes = sub.bucket_sizes()
    assert sizes[3] == 1 and sizes[6] == 0 and sizes[5] == (m.lab == 5).sum() and sizes[0] == 0
    equals_fresh(capi, sub, layers, kept_of(m, ids), Q, f16=f16, **MODES[mode])
    sub.close()
    parent.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [45, 768])
def test_f16_subset_with_a_larger_scale(capi, d):
    """Three rows of the parent are multiplied by 4 (still binary16-exact) and set its scale; DROP exactly those: the subset's scale
    is larger, so every stored piece has to be rescaled."""
    m0, layers, Q = data(d, True)
    X = half_exact(m0.X * np.float32(0.125))   # (room for the three rows; rounded AFTER the scaling: binary16-exact)
    big = np.argsort(np.abs(X).max(axis=1))[-3:]   # (the rows with the largest values: times 4 they are 4x above every other row)
    X[big] *= np.float32(4.0)
    m = Mirror(X, m0.lab, m0.ids)
    ok, why = capi.f16_admissible(X)
    assert ok, why
    rest = np.ones(N, dtype=bool)
    rest[big] = False
    assert np.frexp(np.abs(X).max())[1] > np.frexp(np.abs(X[rest]).max())[1], "the three rows do not set the scale"
    parent = fresh(capi, layers, m, L, storage="f16")
    sub = parent.subset(m.ids[big], drop=True)
    assert sub.N == N - 3
    equals_fresh(capi, sub, layers, kept_of(m, m.ids[big], drop=True), Q, f16=True, storage="f16")
    sub.close()
    parent.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_modes_and_edge_cases(capi, mode):
    """(f16: a subset that keeps nothing skips the F16 finishing, as the build of zero objects does.)"""
    d, f16, kw = 64, mode == "f16", MODES[mode]
    m, layers, Q = data(d, f16)
    rs = np.random.RandomState(3)
    parent = fresh(capi, layers, m, L, **kw)
    before = answers(parent, Q)
    gone = m.ids[rs.rand(N) < 0.3]
    stay = m.ids[~np.isin(m.ids, gone)]
    kept = kept_of(m, gone, drop=True)
    # DROP equals KEEP of the complement
    a, b = parent.subset(gone, drop=True), parent.subset(stay)
    assert a.N == b.N == stay.size
    same_answers(answers(a, Q), answers(b, Q))
    same_buckets(a, b)
    equals_fresh(capi, a, layers, kept, Q, f16=f16, **kw)
    a.close()
    b.close()
    # DROP with n = 0: the full copy answers like the parent
    full = parent.subset([], drop=True)
    assert full.N == N
    same_answers(answers(full, Q), before)
    same_buckets(full, parent)
    equals_fresh(capi, full, layers, m, Q, f16=f16, **kw)
    full.close()
    # unknown and duplicate ids are ignored
    absent = np.asarray([1, 2, 3, 2 ** 32 - 1], dtype=np.uint32)
    assert not np.isin(absent, m.ids).any()
    noisy = parent.subset(np.concatenate([stay, absent, stay[:50], stay[-1:]]))
    equals_fresh(capi, noisy, layers, kept, Q, f16=f16, **kw)
    noisy.close()
    none = parent.subset(absent)   # ... and a list of unknown ids only keeps nothing
    assert none.N == 0 and none.bucket_sizes().sum() == 0
    equals_fresh(capi, none, layers, Mirror(m.X[:0], m.lab[:0], m.ids[:0]), Q, f16=f16, **kw)
    none.close()
    # KEEP with n = 0: the index of zero objects
    empty = parent.subset([])
    assert empty.N == 0
    equals_fresh(capi, empty, layers, Mirror(m.X[:0], m.lab[:0], m.ids[:0]), Q, f16=f16, **kw)
    empty.close()
    same_answers(answers(parent, Q), before)
    parent.close()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_independence(capi):
    d = 96
    m, layers, Q = data(d)
    rs = np.random.RandomState(4)
    ids = m.ids[rs.rand(N) < 0.5]
    kept = kept_of(m, ids)
    parent = fresh(capi, layers, m, L)
    before = answers(parent, Q)
    sub = parent.subset(ids)
    same_answers(answers(parent, Q), before)   # the call only read the parent
    assert getattr(parent, "_views", []) == [] and parent.debug_layout()["counters"].sum() == 0
    sub_before = answers(sub, Q)
    # the parent is mutated afterwards (an insert that relocates a bucket, a delete): the subset does not notice
    extra = dataset(rs, 700, d)
    parent.insert(extra, np.full(700, 2), new_ids(0, 700))
    parent.delete(m.ids[::3])
    same_answers(answers(sub, Q), sub_before)
    equals_fresh(capi, sub, layers, kept, Q)
    # the subset takes an insert and a delete of its own, then equals fresh
    more = dataset(rs, 300, d)
    more_lab, more_ids = rs.randint(0, L, 300), new_ids(5000, 300)
    assert sub.insert(more, more_lab, more_ids) == 300
    kept.insert(more, more_lab, more_ids)
    gone = np.concatenate([kept.ids[::7], more_ids[::2]])
    assert sub.delete(gone) == kept.delete(gone)
    ref = fresh(capi, layers, kept, L)
    same_answers(answers(sub, Q), answers(ref, Q))
    same_buckets(sub, ref)
    ref.close()
    # the parent is closed first: the subset still answers (it owns its models)
    mine = answers(sub, Q)
    parent.close()
    same_answers(answers(sub, Q), mine)
    sub.close()


def test_allowed_beside_and_on_a_clone_view(capi):
    d = 45
    m, layers, Q = data(d)
    ids = m.ids[::2]
    parent = fresh(capi, layers, m, L)
    view = parent.clone_view()
    a = parent.subset(ids)        # while a clone view of the parent lives
    b = view.subset(ids)          # on the clone view itself
    assert len(parent._views) == 1 and b not in view._views
    kept = kept_of(m, ids)
    equals_fresh(capi, a, layers, kept, Q)
    equals_fresh(capi, b, layers, kept, Q)
    view.close()
    parent._views.remove(view)
    parent.insert(m.X[:5], m.lab[:5], new_ids(0, 5))   # neither subset counts as a view: the parent is mutable again
    parent.close()
    same_answers(answers(a, Q), answers(b, Q))
    a.close()
    b.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_full_copy_compacts_a_mutated_index(capi):
    d = 128
    m0, layers, Q = data(d)
    rs = np.random.RandomState(5)
    m = Mirror(m0.X, m0.lab, m0.ids)
    parent = fresh(capi, layers, m, L)
    size7 = int(parent.bucket_sizes()[7])
    for j, (b, n) in enumerate(((7, 3 * size7 + 77), (2, 900), (9, 40))):   # relocations behind the last row-block, a fill in the slack
        xb = dataset(rs, n, d)
        ib = new_ids(10_000 * j, n)
        parent.insert(xb, np.full(n, b), ib)
        m.insert(xb, np.full(n, b), ib)
    gone = np.concatenate([m.ids[::4], m.ids[m.lab == 8]])   # holes inside the buckets' row-blocks; bucket 8 emptied
    assert parent.delete(gone) == m.delete(gone)
    lay = parent.debug_layout()
    assert lay["counters"][1] + lay["counters"][2] + lay["counters"][3] > 0, "no bucket moved: the parent is still packed"
    assert lay["n_rb_total"] > int(np.sum((parent.bucket_sizes() + 31) // 32)), "the parent holds no slack or hole"
    full = parent.subset([], drop=True)
    assert full.debug_layout()["n_rb_total"] == int(np.sum((full.bucket_sizes() + 31) // 32))
    equals_fresh(capi, full, layers, m, Q)
    full.close()
    parent.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_l2(capi):
    d = 45
    m0, layers, Q = data(d)
    rs = np.random.RandomState(6)
    m = Mirror(m0.X * rs.uniform(0.2, 3.0, (N, 1)).astype(np.float32), m0.lab, m0.ids)   # norms that matter
    ids = m.ids[rs.rand(N) < 0.4]
    parent = fresh(capi, layers, m, L, metric="l2")
    sub = parent.subset(ids)
    assert sub.metric == "l2"
    equals_fresh(capi, sub, layers, kept_of(m, ids), Q, metric="l2")
    sub.close()
    parent.close()


def test_owned_mask(capi):
    """A sharded rank that owns half the buckets, built with add_owned_rows: the subset keeps the mask."""
    d = 45
    m, layers, Q = data(d)
    rs = np.random.RandomState(7)
    owned = (np.arange(L) % 2 == 0).astype(np.uint8)

    def rank(mm):
        h = capi.Index(0)
        h.set_mlp(layers)
        h.buckets_begin(mm.lab, d, L, ids=mm.ids, owned=owned)
        mine = np.flatnonzero(owned[mm.lab] == 1)
        h.add_owned_rows(mm.X[mine], mine)
        h.buckets_end()
        return h

    keep = rs.rand(N) < 0.4
    keep[m.lab == 8] = False                     # an owned bucket left empty
    for b in np.flatnonzero(owned == 0):         # every other rank's bucket keeps an object (this rank cannot see them go)
        if (m.lab == b).any():
            keep[np.flatnonzero(m.lab == b)[0]] = True
    ids = m.ids[keep]
    kept = kept_of(m, ids)
    parent = rank(m)
    sub = parent.subset(ids)
    ref = rank(kept)
    assert sub.N == int(owned[kept.lab].sum()) == ref.bucket_sizes().sum()
    same_answers(answers(sub, Q), answers(ref, Q))
    same_buckets(sub, ref)
    assert (sub.bucket_sizes()[owned == 0] == 0).all() and sub.bucket_sizes()[8] == 0
    la, lb = sub.debug_layout(), ref.debug_layout()
    np.testing.assert_array_equal(la["rb_start"], lb["rb_start"])
    np.testing.assert_array_equal(la["cap_rb"], lb["cap_rb"])
    assert sub.index_bytes() == ref.index_bytes()
    more = dataset(rs, 40, d)                    # the mask is the parent's: objects of other ranks' buckets are skipped
    assert sub.insert(more, np.arange(40) % L, new_ids(0, 40)) == int(owned[np.arange(40) % L].sum())
    for h in (sub, ref, parent):
        h.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_li_subset_multi_level(storage):
    """A [4, 3] tree: li.subset(ids) answers like li.delete(complement) on an F32 copy -- with storage="f16" too, where li.delete is
    refused."""
    from learnedmetricindex_amd._capi import LmiError
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from path_mass_ref import synthetic_tree
    from test_gpu_path_mass import frame, net_from

    ncat = [4, 3]
    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree(ncat)
    Xs, Qs = half_exact(Xs * np.float32(0.125)), half_exact(Qs)   # binary16-exact with max |x| < 1: admissible as storage="f16"
    models = net_from(root), {tuple(p): net_from(lay) for p, lay in internal}
    nav, srch = frame(Xn), frame(Xs)
    all_ids = nav.index.to_numpy()
    rs = np.random.RandomState(8)
    ids = all_ids[rs.rand(all_ids.size) < 0.4]
    li = LearnedIndex(models[0], models[1], bucket_paths)
    li.prepare(nav, srch, dp, ncat, storage=storage)
    assert li._engine.storage == storage
    sub = li.subset(ids)
    assert sub is not li and sub._engine is not li._engine and sub._engine.storage == storage and sub._engine.N == ids.size
    assert sub.root_model is li.root_model and sub.internal_models is li.internal_models and sub.bucket_paths is li.bucket_paths
    other = LearnedIndex(models[0], models[1], bucket_paths)   # the same frames in an F32 index that deletes the complement
    other.prepare(nav, srch, dp, ncat)
    assert other.delete(all_ids[~np.isin(all_ids, ids)]) == all_ids.size - ids.size
    for nb, k in ((1, 10), (5, 10)):
        d1, n1, _ = sub.search_resident(Qn, Qs, ncat, nb, k)
        d2, n2, _ = other.search_resident(Qn, Qs, ncat, nb, k)
        assert np.array_equal(n1, n2) and np.array_equal(d1, d2), (nb, k)
    if storage == "f16":
        with pytest.raises(LmiError, match="LMI_STORAGE_F16"):
            li.delete(ids[:3])
    d0, n0, _ = li.search_resident(Qn, Qs, ncat, 5, 10)   # the source still answers, from all of its objects
    assert not np.array_equal(n0, n1)
    dropped = li.subset(all_ids[~np.isin(all_ids, ids)], drop=True)
    d3, n3, _ = dropped.search_resident(Qn, Qs, ncat, 5, 10)
    assert np.array_equal(n3, n2) and np.array_equal(d3, d2)
    li.close()                                            # ... and may go first
    d4, n4, _ = sub.search_resident(Qn, Qs, ncat, 5, 10)
    assert np.array_equal(n4, n2) and np.array_equal(d4, d2)
    for x in (sub, dropped, other):
        x.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(capi):
    import ctypes

    from learnedmetricindex_amd._capi import LmiError

    d = 45
    m, layers, Q = data(d)
    unbuilt = capi.Index(0)
    unbuilt.set_mlp(layers)
    with pytest.raises(LmiError, match="lmi_subset.*not built"):
        unbuilt.subset([1, 2, 3])
    unbuilt.buckets_begin(m.lab, d, L, ids=m.ids)
    with pytest.raises(LmiError, match="lmi_subset.*being built"):
        unbuilt.subset([1, 2, 3])
    unbuilt.close()
    parent = fresh(capi, layers, m, L)
    before = answers(parent, Q)
    ids = np.ascontiguousarray(m.ids[:10])
    out, kept = ctypes.c_void_p(), ctypes.c_int64(-1)
    lib = capi.lib()
    with pytest.raises(LmiError, match="lmi_subset.*unknown mode 2"):
        capi._check(lib.lmi_subset(parent._h, ids.ctypes.data, 10, 2, ctypes.byref(out), ctypes.byref(kept)))
    assert not out.value and kept.value == 0
    assert lib.lmi_subset(parent._h, ids.ctypes.data, -1, 0, ctypes.byref(out), None) != 0 and not out.value
    assert lib.lmi_subset(parent._h, None, 10, 0, ctypes.byref(out), None) != 0 and not out.value
    assert lib.lmi_subset(parent._h, ids.ctypes.data, 10, 0, None, None) != 0
    assert b"lmi_subset" in lib.lmi_last_error()
    same_answers(answers(parent, Q), before)
    np.testing.assert_array_equal(parent.bucket_sizes(), np.bincount(m.lab, minlength=L))
    parent.close()
