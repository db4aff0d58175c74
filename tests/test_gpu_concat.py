"""GPU (`-m gpu`): several built indexes over the same partition as one new, independent index, derived on the device (lmi_concat,
Index.concat, LearnedIndex.concat / .extended).

Contract: the new handle holds exactly what a fresh build of "part 0's objects in the order it holds them, then part 1's, ..." holds.
"Equals fresh" is test_gpu_subset's notion -- equality, no tolerance anywhere, of dists (bit patterns), ids and keys, of bucket_sizes,
of read_bucket's rows and ids for every bucket, of debug_layout (all four counters zero), of index_bytes and of the object count.
`Mirror` keeps the objects in their original order and a build is stable within a bucket, so the concatenation of the parts' Mirrors
IS that object list."""
import numpy as np
import pytest

from test_gpu_mutate import Mirror, dataset, fresh, mlp
from test_gpu_subset import MODES, answers, equals_fresh, half_exact, same_answers, same_buckets

pytestmark = pytest.mark.gpu

L, NQ = 12, 128
# per-bucket counts of (part 0, part 1) that are forced: a bucket empty in one or both parts; a second part that starts at the last
# row of a row-block, at a row-block boundary and one row past it; several scan chunks on either side.  The other buckets: random.
SEAMS = {0: (0, 0), 1: (0, 1), 2: (1, 0), 3: (31, 1), 4: (32, 1), 5: (33, 32), 6: (1, 2500), 7: (2500, 33)}
FREE = 400   # objects per part in the buckets that are not forced


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def unique_ids(rs, n):
    ids = (rs.permutation(2 ** 20)[:n].astype(np.uint64) * 4093 + 7).astype(np.uint32)   # unique, up to 2^32: above 2^31 too
    assert np.unique(ids).size == n
    return ids


def whole(parts):
    """The object list of the concatenation: part 0's objects, then part 1's, ..."""
    return Mirror(np.concatenate([p.X for p in parts]), np.concatenate([p.lab for p in parts]), np.concatenate([p.ids for p in parts]))


_seams = {}


def seam_parts(d, f16=False):
    """(two Mirrors with the forced per-bucket counts in shuffled order, model, queries), made once per (d, f16) and never changed."""
    if (d, f16) not in _seams:
        rs = np.random.RandomState(2000 + d)
        free = [b for b in range(L) if b not in SEAMS]
        parts = []
        for t in (0, 1):
            lab = np.concatenate([np.full(n[t], b) for b, n in SEAMS.items()] + [np.asarray(free)[rs.randint(0, len(free), FREE)]])
            lab = lab[rs.permutation(lab.size)]
            X = dataset(rs, lab.size, d)
            parts.append([half_exact(X) if f16 else X, lab])
        ids = unique_ids(rs, sum(p[1].size for p in parts))
        n0 = parts[0][1].size
        Q = dataset(rs, NQ, d)
        Q = half_exact(Q) if f16 else Q
        _seams[(d, f16)] = ([Mirror(parts[0][0], parts[0][1], ids[:n0]), Mirror(parts[1][0], parts[1][1], ids[n0:])], mlp(rs, d, L), Q)
    return _seams[(d, f16)]


def unequal_parts(d, sizes, f16=False, seed=0):
    rs = np.random.RandomState(3000 + d + seed)
    n = sum(sizes)
    X = dataset(rs, n, d)
    X = half_exact(X) if f16 else X
    lab, ids = rs.randint(0, L, n), unique_ids(rs, n)
    Q = dataset(rs, NQ, d)
    cuts = np.cumsum([0] + list(sizes))
    return [Mirror(X[a:b], lab[a:b], ids[a:b]) for a, b in zip(cuts[:-1], cuts[1:])], mlp(rs, d, L), half_exact(Q) if f16 else Q


def close_all(*handles):
    for h in handles:
        h.close()


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [45, 768])
@pytest.mark.parametrize("mode", list(MODES))
def test_seams_across_modes_and_dimensions(capi, mode, d):
    """d = 45: the low-dimensional fragment shape, d % 8 != 0; d = 768: the 16 x 32 shape.  In the fragment forms part 1's rows land
    mid-row-block wherever part 0 leaves n % 32 != 0 rows."""
    f16 = mode == "f16"
    (m0, m1), layers, Q = seam_parts(d, f16)
    for b, (n0, n1) in SEAMS.items():
        assert (m0.lab == b).sum() == n0 and (m1.lab == b).sum() == n1
    a, b = fresh(capi, layers, m0, L, **MODES[mode]), fresh(capi, layers, m1, L, **MODES[mode])
    before = answers(a, Q), answers(b, Q)
    cat = a.concat(b)
    assert cat.storage == a.storage and cat.metric == "ip" and cat.L == L and cat.d == d and cat.N == m0.ids.size + m1.ids.size
    plan = capi.concat_last_plan()
    assert plan["parts"] == 2 and plan["rows"] == cat.N and plan["rescaled_parts"] == 0
    assert plan["slab_rows"] == 32 * int(np.sum((cat.bucket_sizes() + 31) // 32))
    assert 8 * plan["slab_rows"] <= plan["map_bytes"] <= 8 * plan["slab_rows"] + 2 * (64 + 12 * L)   # 8 bytes per row + the small tables
    np.testing.assert_array_equal(cat.bucket_sizes()[:len(SEAMS)], [sum(SEAMS[bk]) for bk in range(len(SEAMS))])
    equals_fresh(capi, cat, layers, whole([m0, m1]), Q, f16=f16, **MODES[mode])
    same_answers(answers(a, Q), before[0])   # the call only read the parts
    same_answers(answers(b, Q), before[1])
    close_all(cat, a, b)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_five_parts_one_of_them_empty(capi, mode):
    f16 = mode == "f16"
    d = 768 if f16 else 45
    ms, layers, Q = unequal_parts(d, (1500, 37, 700, 1, 900), f16)
    hs = [fresh(capi, layers, m, L, **MODES[mode]) for m in ms]
    empty = hs[2].subset([], drop=False)   # an index of zero objects
    assert empty.N == 0
    none = Mirror(ms[0].X[:0], ms[0].lab[:0], ms[0].ids[:0])
    cat = hs[0].concat(hs[1], empty, hs[2], hs[3], hs[4])
    assert capi.concat_last_plan()["parts"] == 6
    equals_fresh(capi, cat, layers, whole([ms[0], ms[1], none, ms[2], ms[3], ms[4]]), Q, f16=f16, **MODES[mode])
    first = empty.concat(hs[1])            # ... also as the receiver, and alone
    equals_fresh(capi, first, layers, ms[1], Q, f16=f16, **MODES[mode])
    alone = empty.concat()
    assert alone.N == 0
    equals_fresh(capi, alone, layers, none, Q, f16=f16, **MODES[mode])
    close_all(cat, first, alone, empty, *hs)


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_the_same_part_twice(capi, mode):
    f16 = mode == "f16"
    (m0, m1), layers, Q = seam_parts(45, f16)
    a, b = fresh(capi, layers, m0, L, **MODES[mode]), fresh(capi, layers, m1, L, **MODES[mode])
    cat = a.concat(b, a)
    assert cat.N == 2 * m0.ids.size + m1.ids.size
    equals_fresh(capi, cat, layers, whole([m0, m1, m0]), Q, f16=f16, **MODES[mode])
    close_all(cat, a, b)


def test_a_single_mutated_part_is_its_compaction(capi):
    """f32, after inserts that relocate buckets and deletes that leave holes: concat of one part equals subset DROP of nothing."""
    d = 128
    (m0, _), layers, Q = seam_parts(d)
    rs = np.random.RandomState(5)
    m = Mirror(m0.X, m0.lab, m0.ids)
    h = fresh(capi, layers, m, L)
    size9 = int(h.bucket_sizes()[9])
    for j, (b, n) in enumerate(((9, 3 * size9 + 77), (2, 900), (10, 40))):
        xb, ib = dataset(rs, n, d), ((10_000 * j + np.arange(n, dtype=np.uint64)) * 4093 + 8).astype(np.uint32)
        h.insert(xb, np.full(n, b), ib)
        m.insert(xb, np.full(n, b), ib)
    gone = np.concatenate([m.ids[::4], m.ids[m.lab == 8]])
    assert h.delete(gone) == m.delete(gone)
    lay = h.debug_layout()
    assert lay["counters"][1] + lay["counters"][2] + lay["counters"][3] > 0, "no bucket moved: the part is still packed"
    assert lay["n_rb_total"] > int(np.sum((h.bucket_sizes() + 31) // 32)), "the part holds no slack or hole"
    cat, full = h.concat(), h.subset([], drop=True)
    assert not cat.debug_layout()["counters"].any()
    same_answers(answers(cat, Q), answers(full, Q))
    same_buckets(cat, full)
    np.testing.assert_array_equal(cat.debug_layout()["rb_start"], full.debug_layout()["rb_start"])
    assert cat.index_bytes() == full.index_bytes()
    equals_fresh(capi, cat, layers, m, Q)
    close_all(cat, full, h)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [45, 768])
def test_f16_parts_under_different_scales(capi, d):
    """Part 1 holds three rows 4 x above everything else, so the result's scale is below part 0's: every half of part 0 is multiplied
    by a power of two < 1 on the way and is still exact (max |x| < 1: the index scale stays >= 1 and only moves exponents up)."""
    (s0, s1), layers, Q = seam_parts(d, True)
    # (rounded AFTER the scaling: binary16-exact.  + 0: a value that underflows to -0.0 becomes +0.0 -- read_bucket(dtype=float16) of
    # a storage="f16" index, a fresh build's too, returns +0.0 for a stored -0.0 while its float32 read returns -0.0, and the last
    # check below is on the bits that went in)
    X0, X1 = half_exact(s0.X * np.float32(0.125)) + np.float32(0), half_exact(s1.X * np.float32(0.125)) + np.float32(0)
    assert not (X0.view(np.uint32) == 0x80000000).any() and not (X1.view(np.uint32) == 0x80000000).any()
    big = np.argsort(np.abs(X1).max(axis=1))[-3:]   # (the rows with the largest values: times 4 they are far above every other row)
    X1[big] *= np.float32(4.0)
    m0, m1 = Mirror(X0, s0.lab, s0.ids), Mirror(X1, s1.lab, s1.ids)
    both = whole([m0, m1])
    ok, why = capi.f16_admissible(both.X)
    assert ok, why
    rest = np.ones(m1.ids.size, dtype=bool)
    rest[big] = False
    assert np.frexp(np.abs(X1).max())[1] > np.frexp(max(np.abs(X0).max(), np.abs(X1[rest]).max()))[1], "the three rows do not set the scale"
    assert np.abs(both.X).max() < 1
    a, b = fresh(capi, layers, m0, L, storage="f16"), fresh(capi, layers, m1, L, storage="f16")
    cat = a.concat(b)
    assert capi.concat_last_plan()["rescaled_parts"] == 1
    equals_fresh(capi, cat, layers, both, Q, f16=True, storage="f16")   # the fresh F16 build and the fresh F32 build
    for bkt in range(L):   # read_bucket(dtype=float16) returns the ingested bits
        rows, _ = cat.read_bucket(bkt, dtype=np.float16)
        assert np.array_equal(rows.view(np.uint16), both.X[both.lab == bkt].astype(np.float16).view(np.uint16)), bkt
    back = b.concat(a)     # the other way round part 1 keeps its scale and part 0, now second, is the one rescaled
    assert capi.concat_last_plan()["rescaled_parts"] == 1
    equals_fresh(capi, back, layers, whole([m1, m0]), Q, f16=True, storage="f16")
    close_all(cat, back, a, b)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_f16_refusal_is_a_fresh_builds(capi):
    """Part 0 contains 2^-24, the smallest subnormal half; part 1's maximum is 4.0, whose scale is 1/8: 2^-27 is no half."""
    d = 45
    (s0, s1), layers, Q = seam_parts(d, True)
    X0 = s0.X.copy()
    X0[5, 7] = np.float32(2.0 ** -24)
    X1 = (np.round(s1.X * 256) / 256).astype(np.float32)   # multiples of 2^-8: times 1/8 they are halves
    X1[3, 2] = np.float32(4.0)
    m0, m1 = Mirror(X0, s0.lab, s0.ids), Mirror(X1, s1.lab, s1.ids)
    for X in (X0, X1):
        ok, why = capi.f16_admissible(X)
        assert ok, why
    both = whole([m0, m1])
    ok, why = capi.f16_admissible(both.X)   # the verdict a fresh F16 build of the concatenated rows reaches, restated on the host
    assert not ok and "index scale 0.125" in why
    with pytest.raises(capi.LmiError, match=r"lmi_buckets_end: LMI_STORAGE_F16 refused.*index scale 0\.125"):   # ... and on the device
        fresh(capi, layers, both, L, storage="f16")
    a, b = fresh(capi, layers, m0, L, storage="f16"), fresh(capi, layers, m1, L, storage="f16")
    before = answers(a, Q), answers(b, Q)
    with pytest.raises(capi.LmiError, match=r"lmi_concat: LMI_STORAGE_F16 refused.*index scale 0\.125.*no index was made") as e:
        a.concat(b)
    assert "max|x| = 4" in str(e.value)
    assert not any(capi.concat_last_plan().values())
    with pytest.raises(capi.LmiError, match="LMI_STORAGE_F16 refused"):
        b.concat(a)
    same_answers(answers(a, Q), before[0])
    same_answers(answers(b, Q), before[1])
    for bkt in range(L):   # ... and still hold the bits they ingested
        rows, _ = a.read_bucket(bkt, dtype=np.float16)
        assert np.array_equal(rows.view(np.uint16), X0[m0.lab == bkt].astype(np.float16).view(np.uint16)), bkt
    close_all(a, b)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "exact"])
def test_l2_the_norm_column_travels(capi, mode):
    d = 45
    (s0, s1), layers, Q = seam_parts(d)
    rs = np.random.RandomState(6)
    m0 = Mirror(s0.X * rs.uniform(0.2, 3.0, (s0.ids.size, 1)).astype(np.float32), s0.lab, s0.ids)   # norms that matter
    m1 = Mirror(s1.X * rs.uniform(0.2, 3.0, (s1.ids.size, 1)).astype(np.float32), s1.lab, s1.ids)
    kw = dict(MODES[mode], metric="l2")
    a, b = fresh(capi, layers, m0, L, **kw), fresh(capi, layers, m1, L, **kw)
    cat = a.concat(b)
    assert cat.metric == "l2"
    equals_fresh(capi, cat, layers, whole([m0, m1]), Q, **kw)
    close_all(cat, a, b)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_union_and_range_scans_equal_fresh(capi):
    d = 45
    (m0, m1), layers, Q = seam_parts(d)
    a, b = fresh(capi, layers, m0, L), fresh(capi, layers, m1, L)
    cat, ref = a.concat(b), fresh(capi, layers, whole([m0, m1]), L)
    order = np.stack([np.random.RandomState(q).permutation(L)[:5] for q in range(NQ)]).astype(np.int32)
    for x, y in zip(cat.scan_union(Q, order, 100), ref.scan_union(Q, order, 100)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    got, want = cat.scan_range(Q, order, 0.6), ref.scan_range(Q, order, 0.6)
    assert want[0][-1] > NQ, "the radius catches next to nothing"
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    close_all(cat, ref, a, b)


def test_tree_walk_with_the_tables_of_part_0(capi):
    """A [4, 3] tree: part 0 carries the node models and the tree tables, part 1 only a root model of its own, which is ignored."""
    from path_mass_ref import synthetic_tree

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree((4, 3))
    lab = dp[:, 0] * 3 + dp[:, 1]
    ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    first = np.random.RandomState(7).rand(ids.size) < 0.6

    def treed(sel):
        h = capi.Index(0)
        h.set_mlp(root)
        for i, (_, layers) in enumerate(internal):
            h.nav_set_model(i + 1, layers)
        h.nav_set_tree([0, 4, 7, 10, 13, 16], [1, 2, 3, 4] + [-1] * 12, [-2] * 4 + list(range(12)))
        h.set_buckets(Xs[sel], lab[sel], 12, ids=ids[sel])
        return h

    a = treed(first)
    b = capi.Index(0)
    b.set_mlp([(0 * W, 0 * c) for W, c in root])
    b.set_buckets(Xs[~first], lab[~first], 12, ids=ids[~first])
    cat = a.concat(b)
    ref = treed(np.concatenate([np.flatnonzero(first), np.flatnonzero(~first)]))
    for nb, k in ((1, 10), (5, 10), (7, 30)):
        got, want = cat.search_tree(Qn, Qs, nb, k, want_keys=True, want_order=True), ref.search_tree(Qn, Qs, nb, k, want_keys=True, want_order=True)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (nb, k)
    close_all(cat, ref, a, b)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_independence(capi):
    d = 45
    (m0, m1), layers, Q = seam_parts(d)
    a, b = fresh(capi, layers, m0, L), fresh(capi, layers, m1, L)
    filt = capi.Filter(a, [m0.ids[::2]])
    view = b.clone_view()
    cat = a.concat(view)              # a clone view is accepted as a part, and b has a live clone view
    assert len(b._views) == 1 and getattr(a, "_views", []) == [] and cat not in b._views and not hasattr(cat, "_parent")
    order = np.tile(np.arange(3, dtype=np.int32), (NQ, 1))
    a.scan_union(Q, order, 10, filter=filt)
    with pytest.raises(capi.LmiError, match="the filter is stale or belongs to another index"):   # the result has a layout stamp of its own
        cat.scan_union(Q, order, 10, filter=filt)
    mine = answers(cat, Q)
    # the parts are mutated, then closed: the result does not notice
    a.insert(m1.X[:300], np.full(300, 2), ((np.arange(300, dtype=np.uint64)) * 4093 + 8).astype(np.uint32))
    a.delete(m0.ids[::3])
    same_answers(answers(cat, Q), mine)
    filt.close()
    close_all(view)
    b._views.remove(view)
    close_all(a, b)
    same_answers(answers(cat, Q), mine)
    equals_fresh(capi, cat, layers, whole([m0, m1]), Q)
    # the result takes an insert of its own
    assert cat.insert(m0.X[:5], m0.lab[:5], np.arange(1, 6, dtype=np.uint32)) == 5
    cat.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(capi):
    import ctypes

    d = 45
    (m0, m1), layers, Q = seam_parts(d)
    h0 = fresh(capi, layers, m0, L)
    h16 = fresh(capi, layers, Mirror(half_exact(m1.X), m1.lab, m1.ids), L, storage="f16")
    before = answers(h0, Q), answers(h16, Q)

    def refused(other, pattern):
        with pytest.raises(capi.LmiError, match=pattern):
            h0.concat(other)
        other.close()

    rs = np.random.RandomState(8)
    refused(fresh(capi, mlp(rs, d + 3, L), Mirror(dataset(rs, 200, d + 3), m1.lab[:200], m1.ids[:200]), L), r"lmi_concat: parts\[1\] differs from parts\[0\] in d: 48, not 45")
    refused(fresh(capi, mlp(rs, d, L + 1), Mirror(m1.X[:200], m1.lab[:200], m1.ids[:200]), L + 1), r"parts\[1\] differs from parts\[0\] in L: 13 buckets, not 12")
    refused(fresh(capi, layers, m1, L, metric="l2"), r"parts\[1\] differs from parts\[0\] in the metric: LMI_METRIC_L2, not LMI_METRIC_IP")
    refused(fresh(capi, layers, m1, L, prefilter=False), r"parts\[1\] differs from parts\[0\] in the prefilter: off, not on")
    with pytest.raises(capi.LmiError, match=r"parts\[1\] differs from parts\[0\] in the storage: LMI_STORAGE_F16, not LMI_STORAGE_F32"):
        h0.concat(h16)
    with pytest.raises(capi.LmiError, match=r"parts\[2\] differs from parts\[0\] in the storage"):
        h0.concat(h0, h16)
    with pytest.raises(capi.LmiError, match=r"parts\[1\] differs from parts\[0\] in the storage: LMI_STORAGE_F32, not LMI_STORAGE_F16"):
        h16.concat(h0)
    owned = (np.arange(L) % 2 == 0).astype(np.uint8)

    def rank(mask):
        h = capi.Index(0)
        h.set_mlp(layers)
        h.buckets_begin(m1.lab, d, L, ids=m1.ids, owned=mask)
        mine = np.flatnonzero(mask[m1.lab] == 1)
        h.add_owned_rows(m1.X[mine], mine)
        h.buckets_end()
        return h

    r0, r1 = rank(owned), rank(1 - owned)
    with pytest.raises(capi.LmiError, match=r"parts\[1\] differs from parts\[0\] in the owned mask: it has one, parts\[0\] has none"):
        h0.concat(r0)
    with pytest.raises(capi.LmiError, match=r"parts\[1\] differs from parts\[0\] in the owned mask: it has none"):
        r0.concat(h0)
    with pytest.raises(capi.LmiError, match=r"parts\[1\] differs from parts\[0\] in the owned mask at bucket 0"):
        r0.concat(r1)
    close_all(r0, r1)
    unbuilt = capi.Index(0)
    unbuilt.set_mlp(layers)
    unbuilt.L = L
    with pytest.raises(capi.LmiError, match=r"lmi_concat: parts\[1\] is not built"):
        h0.concat(unbuilt)
    with pytest.raises(capi.LmiError, match=r"lmi_concat: parts\[0\] is not built"):
        unbuilt.concat(h0)
    unbuilt.buckets_begin(m1.lab, d, L, ids=m1.ids)
    with pytest.raises(capi.LmiError, match=r"lmi_concat: parts\[1\] is being built"):
        h0.concat(unbuilt)
    unbuilt.close()
    # 0 parts, 65 parts and the NULLs, at the C ABI
    lib = capi.lib()
    out, total = ctypes.c_void_p(), ctypes.c_int64(-1)
    handles = (ctypes.c_void_p * 65)(*[h0._h.value] * 65)
    with pytest.raises(capi.LmiError, match=r"lmi_concat: n_parts = 0 outside \[1, 64\]"):
        capi._check(lib.lmi_concat(handles, 0, ctypes.byref(out), ctypes.byref(total)))
    assert not out.value and total.value == 0
    with pytest.raises(capi.LmiError, match=r"lmi_concat: n_parts = 65 outside \[1, 64\]"):
        capi._check(lib.lmi_concat(handles, 65, ctypes.byref(out), ctypes.byref(total)))
    assert not out.value
    handles[1] = None
    with pytest.raises(capi.LmiError, match=r"lmi_concat: parts\[1\] is NULL"):
        capi._check(lib.lmi_concat(handles, 3, ctypes.byref(out), None))
    assert lib.lmi_concat(None, 1, ctypes.byref(out), None) != 0 and b"parts is NULL" in lib.lmi_last_error()
    assert lib.lmi_concat(handles, 1, None, None) != 0 and b"out is NULL" in lib.lmi_last_error()
    assert not any(capi.concat_last_plan().values())
    with pytest.raises(ValueError, match="65 parts"):
        h0.concat(*[h0] * 64)
    same_answers(answers(h0, Q), before[0])   # after every refusal the parts answer unchanged
    same_answers(answers(h16, Q), before[1])
    np.testing.assert_array_equal(h0.bucket_sizes(), np.bincount(m0.lab, minlength=L))
    close_all(h0, h16)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_owned_parts(capi):
    """Two parts of a sharded rank that owns half the buckets, built with add_owned_rows: the result keeps the mask and equals the
    rank's fresh build of both object lists."""
    d = 45
    (m0, m1), layers, Q = seam_parts(d)
    owned = (np.arange(L) % 2 == 0).astype(np.uint8)

    def rank(mm):
        h = capi.Index(0)
        h.set_mlp(layers)
        h.buckets_begin(mm.lab, d, L, ids=mm.ids, owned=owned)
        mine = np.flatnonzero(owned[mm.lab] == 1)
        h.add_owned_rows(mm.X[mine], mine)
        h.buckets_end()
        return h

    both = whole([m0, m1])
    a, b, ref = rank(m0), rank(m1), rank(both)
    cat = a.concat(b)
    assert cat.N == int(owned[both.lab].sum()) == ref.bucket_sizes().sum()
    same_answers(answers(cat, Q), answers(ref, Q))
    same_buckets(cat, ref)
    assert (cat.bucket_sizes()[owned == 0] == 0).all()
    la, lb = cat.debug_layout(), ref.debug_layout()
    np.testing.assert_array_equal(la["rb_start"], lb["rb_start"])
    np.testing.assert_array_equal(la["cap_rb"], lb["cap_rb"])
    assert not la["counters"].any() and cat.index_bytes() == ref.index_bytes()
    more = dataset(np.random.RandomState(9), 40, d)   # the mask is the parts': objects of other ranks' buckets are skipped
    assert cat.insert(more, np.arange(40) % L, np.arange(1, 41, dtype=np.uint32)) == int(owned[np.arange(40) % L].sum())
    close_all(cat, ref, a, b)


# ---- 10 -----------------------------------------------------------------------------------------------------------------------
def li_case():
    from test_gpu_mutate import frame, net_from

    rs = np.random.RandomState(11)
    X = rs.randn(5600, 64).astype(np.float32)
    X16 = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float16)   # the data as it is distributed
    Q = (X16[rs.randint(0, 5600, 200)].astype(np.float32) + 0.05 * rs.randn(200, 64).astype(np.float32)).astype(np.float16).astype(np.float32)
    layers = [((rs.randn(128, 64) * 0.3).astype(np.float32), (rs.randn(128) * 0.1).astype(np.float32)),
              ((rs.randn(12, 128) * 0.3).astype(np.float32), (rs.randn(12) * 0.1).astype(np.float32))]
    dp = rs.randint(0, 12, 5000).astype(np.int64)
    return frame(X16[:5000]), frame(X16[5000:], first_id=70001), dp, Q, net_from(layers)


def test_li_extended_on_f16_equals_a_search_over_all_frames(capi, tmp_path):
    """A 5 000 x 64 float16 frame, resident as storage="f16", grows by 600 objects: `extended`, then `search_resident`, equals
    `li.search` over the concatenated frames with storage="f16" -- where `insert` is refused."""
    import pandas as pd

    from learnedmetricindex_amd import index_io
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    df, new_df, dp, Q, net = li_case()
    assert df.dtypes.iloc[0] == np.float16
    li = LearnedIndex(net, {}, [(i,) for i in range(12)])
    li.prepare(df, df, dp, [12], storage="f16")
    with pytest.raises(capi.LmiError, match="LMI_STORAGE_F16"):
        li.insert(new_df)
    grown, dp_new = li.extended(new_df)
    assert grown is not li and grown._engine is not li._engine and grown._engine.storage == "f16" and grown._engine.N == 5600
    assert dp_new.shape == (600, 1) and li._engine.N == 5000
    ref = LearnedIndex(net, {}, [(i,) for i in range(12)])
    all_df, all_dp = pd.concat([df, new_df]), np.concatenate([dp, dp_new[:, 0]])
    for nb, k in ((1, 10), (3, 10), (5, 10)):
        d1, n1, _ = grown.search_resident(Q, Q, [12], nb, k)
        d2, n2, _ = ref.search(all_df, Q, all_df, Q, all_dp, [12], n_buckets=nb, k=k, storage="f16")
        assert np.array_equal(n1, n2) and np.array_equal(d1, d2), (nb, k)
    assert ref._engine.storage == "f16"
    same_buckets(grown._engine, ref._engine, dtype=np.float16)
    # li.concat of two resident indexes is the same thing
    delta = LearnedIndex(net, {}, [(i,) for i in range(12)])
    delta.prepare(new_df, new_df, dp_new, [12], storage="f16")
    cat = li.concat(delta)
    same_buckets(cat._engine, ref._engine, dtype=np.float16)
    with pytest.raises(ValueError, match="bucket_paths"):
        li.concat(_with_engine(delta, [(i,) for i in range(11)]))
    # save -> load -> the same answers
    index_io.save_index(str(tmp_path / "grown"), grown, [12])
    back, ncat = index_io.load_index(str(tmp_path / "grown"))
    assert back._engine.storage == "f16"
    d3, n3, _ = back.search_resident(Q, Q, ncat, 3, 10)
    d1, n1, _ = grown.search_resident(Q, Q, [12], 3, 10)
    assert np.array_equal(n3, n1) and np.array_equal(d3, d1)
    for x in (back, cat, delta, ref, grown, li):
        x.close()


def _with_engine(src, bucket_paths):
    """A LearnedIndex that shares `src`'s resident engine under other bucket paths (never closed by itself)."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    class Borrowed(LearnedIndex):
        def close(self):
            self._engine = None

    other = Borrowed(src.root_model, src.internal_models, bucket_paths)
    other._engine = src._engine
    return other


def test_li_extended_on_f32_equals_insert_on_a_copy(capi):
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    df, new_df, dp, Q, net = li_case()
    li = LearnedIndex(net, {}, [(i,) for i in range(12)])
    li.prepare(df, df, dp, [12])
    copy = LearnedIndex(net, {}, [(i,) for i in range(12)])
    copy.prepare(df, df, dp, [12])
    grown, dp_new = li.extended(new_df)
    np.testing.assert_array_equal(copy.insert(new_df), dp_new)
    assert grown._engine.storage == "f32" and grown._engine.N == copy._engine.N == 5600
    for nb, k in ((1, 10), (3, 10), (5, 10)):
        d1, n1, _ = grown.search_resident(Q, Q, [12], nb, k)
        d2, n2, _ = copy.search_resident(Q, Q, [12], nb, k)
        assert np.array_equal(n1, n2) and np.array_equal(d1, d2), (nb, k)
    same_buckets(grown._engine, copy._engine)
    for x in (grown, copy, li):
        x.close()
