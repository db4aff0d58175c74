"""GPU (`-m gpu`): stored objects by id (lmi_rows_fetch / lmi_rows_fetch_f16; Index.fetch / locate / fetch_device,
LearnedIndex.reconstruct / search_like, ShardedSearcher.reconstruct).

Every comparison is equality of bytes; there is no tolerance anywhere.  The truth never comes from the code under test: rows are the
original array's (`X[original row of the id]`), locations come from a dictionary built with `read_bucket` over all buckets (the first
(bucket, row) that carries an id).  N = 600 objects in L = 7 buckets whose sizes are forced to 0, 1, 32, 33 and 70 rows (two more
share the rest); ids are unique unless a case says otherwise and some lie above 2^31.  d = 8: one piece per row; d = 45: a partial
last piece and a row length that is no multiple of 16 bytes; d = 136: K above 128, the other fp16 fragment shape."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

from helpers import inputs_for, layers_from, load_golden
from test_gpu_mutate import Mirror, dataset, fresh, mlp

pytestmark = pytest.mark.gpu

N, L = 600, 7
FORCED = {0: 0, 1: 1, 2: 32, 3: 33, 4: 70}
DIMS = (8, 45, 136)
FORMS = {"f32-ip": dict(), "f32-l2": dict(metric="l2"), "exact-ip": dict(prefilter=False), "exact-l2": dict(prefilter=False, metric="l2"),
         "f16-ip": dict(storage="f16")}
FORM_WORD = {"f32-ip": 1, "f32-l2": 1, "exact-ip": 0, "exact-l2": 0, "f16-ip": 2}   # LMI_FETCH_PLAN_FORM: the StoredForm
ABSENT = np.asarray([8, 4093 * 3 + 9, 2 ** 32 - 1, 0], dtype=np.uint32)   # (the objects' ids are 7 mod 4093)


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def half_exact(X):
    return X.astype(np.float16).astype(np.float32)


_data, _idx = {}, {}


def data(d, exact16=False):
    """(Mirror of N objects with the forced bucket sizes in shuffled order, model), made once per (d, exact16) and never changed."""
    if (d, exact16) not in _data:
        rs = np.random.RandomState(2000 + d)
        X = dataset(rs, N, d)
        free = [b for b in range(L) if b not in FORCED]
        rest = N - sum(FORCED.values())
        lab = np.concatenate([np.full(n, b) for b, n in FORCED.items()] + [np.asarray(free)[rs.randint(0, len(free), rest)]])
        lab = lab[rs.permutation(N)]
        ids = (rs.permutation(2 ** 20)[:N].astype(np.uint64) * 4093 + 7).astype(np.uint32)
        assert np.unique(ids).size == N and ids.max() > 2 ** 31 and not np.isin(ABSENT, ids).any()
        if exact16:
            X = half_exact(X)
        for a in (X, lab, ids):
            a.setflags(write=False)
        _data[(d, exact16)] = (Mirror(X, lab, ids), mlp(rs, d, L))
        for a in (_data[(d, exact16)][0].X, _data[(d, exact16)][0].lab, _data[(d, exact16)][0].ids):
            a.setflags(write=False)
    return _data[(d, exact16)]


@pytest.fixture(scope="module")
def built(capi):
    """One built index per (d, form, exact16), shared by the cases that only read it."""
    def get(d, form, exact16=False):
        key = (d, form, exact16 or form == "f16-ip")
        if key not in _idx:
            m, layers = data(d, key[2])
            _idx[key] = fresh(capi, layers, m, L, **FORMS[form])
            np.testing.assert_array_equal(_idx[key].bucket_sizes()[:5], [0, 1, 32, 33, 70])
        return _idx[key], data(d, key[2])[0]
    yield get
    for h in _idx.values():
        h.close()
    _idx.clear()


def table(idx, dtype=np.float32, n_buckets=L):
    """id -> (bucket, row, the row's values) of the FIRST stored row that carries the id, from read_bucket over all buckets."""
    out = {}
    for b in range(n_buckets):
        rows, ids = idx.read_bucket(b, dtype=dtype)
        for r, i in enumerate(ids.tolist()):
            out.setdefault(i, (b, r, rows[r]))
    return out


def expected(tab, ids, d, dtype=np.float32):
    ids = np.asarray(ids).reshape(-1)
    rows = np.zeros((ids.size, d), dtype=dtype)
    bucket, row = np.full(ids.size, -1, np.int32), np.full(ids.size, -1, np.int32)
    for j, i in enumerate(ids.tolist()):
        if i in tab:
            bucket[j], row[j], rows[j] = tab[i]
    return rows, bucket, row


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("rows", "bucket", "row")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (name, what)


def check(idx, ids, tab, dtype=np.float32, what=""):
    got = idx.fetch(ids, dtype=dtype, where=True)
    same(got, expected(tab, ids, idx.d, dtype), what)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("d", DIMS)
def test_every_id_in_shuffled_order(capi, built, d, form, dtype):
    idx, m = built(d, form, exact16=dtype == np.float16)
    order = np.random.RandomState(d).permutation(N)
    ids = m.ids[order]
    rows, bucket, row = check(idx, ids, table(idx, dtype), dtype, (d, form))
    assert np.array_equal(rows.view(np.uint8), m.X[order].astype(dtype).view(np.uint8))   # the original array's rows
    np.testing.assert_array_equal(bucket, m.lab[order])
    rank_in_bucket = np.asarray([np.count_nonzero(m.lab[:o] == m.lab[o]) for o in order], np.int32)   # a bucket holds its objects in ascending original row
    np.testing.assert_array_equal(row, rank_in_bucket)
    plan = capi.fetch_last_plan()
    assert plan["REQUESTS"] == plan["UNIQUE"] == plan["FOUND"] == N and plan["PIECES"] == 1 and plan["FORM"] == FORM_WORD[form]
    assert 0 < plan["WORKSPACE_BYTES"] <= 16 * N + N * (d * 4 + 8) + 64
    np.testing.assert_array_equal(idx.fetch(ids, dtype=dtype), rows)   # where=False: the rows alone


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32-ip", "exact-l2", "f16-ip"])
def test_present_absent_and_repeated_requests(capi, built, form):
    idx, m = built(45, form)
    tab = table(idx)
    rs = np.random.RandomState(7)
    ids = np.concatenate([m.ids[rs.randint(0, N, 150)], ABSENT, m.ids[:40], ABSENT[:2], m.ids[:40]])[rs.permutation(150 + 4 + 40 + 2 + 40)]
    rows, bucket, row = check(idx, ids, tab, what=form)
    gone = np.isin(ids, ABSENT)
    assert gone.sum() == 6 and (bucket[gone] == -1).all() and (row[gone] == -1).all() and not rows[gone].any() and (bucket[~gone] >= 0).all()
    plan = capi.fetch_last_plan()
    assert plan["REQUESTS"] == ids.size and plan["UNIQUE"] == np.unique(ids).size and plan["FOUND"] == int(np.isin(ids, m.ids).sum())
    for one in (m.ids[5:6], ABSENT[2:3]):   # n = 1: present, absent
        check(idx, one, tab, what="n = 1")
        assert capi.fetch_last_plan()["FOUND"] == int(one[0] in tab)
    rows, bucket, row = idx.fetch([], where=True)   # n = 0
    assert rows.shape == (0, 45) and bucket.shape == row.shape == (0,)
    plan = capi.fetch_last_plan()
    assert plan["REQUESTS"] == plan["PIECES"] == plan["FOUND"] == 0 and plan["FORM"] == FORM_WORD[form]


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("form", ["f32-ip", "exact-ip", "f16-ip"])
def test_the_piece_seam(capi, built, form, dtype):
    idx, m = built(45, form, exact16=True)
    ids = np.concatenate([m.ids[::3], ABSENT[:1], m.ids[:9]])
    n = ids.size
    want = idx.fetch(ids, dtype=dtype, where=True)
    same(want, expected(table(idx, dtype), ids, 45, dtype))
    assert capi.fetch_last_plan()["PIECES"] == 1 and capi.fetch_last_plan()["PIECE_ROWS"] >= n
    try:
        for p in (1, 7, n - 1, n, n + 1):
            capi.fetch_set_geometry(piece_rows=p)
            same(idx.fetch(ids, dtype=dtype, where=True), want, f"piece_rows {p}")
            plan = capi.fetch_last_plan()
            assert plan["PIECES"] == -(-n // p) and plan["PIECE_ROWS"] == p, p
            b, r = idx.locate(ids)
            same((b, r), want[1:], f"locate, piece_rows {p}")
            assert capi.fetch_last_plan()["PIECES"] == -(-n // p)
    finally:
        capi.fetch_set_geometry(piece_rows=0)
    same(idx.fetch(ids, dtype=dtype, where=True), want)
    assert capi.fetch_last_plan()["PIECES"] == 1


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_pure_locate_equals_the_where_outputs(capi, built, form):
    idx, m = built(136, form)
    ids = np.concatenate([m.ids[::-1], ABSENT])
    _, bucket, row = idx.fetch(ids, where=True)
    b, r = idx.locate(ids)
    same((b, r), (bucket, row))
    assert capi.fetch_last_plan()["WORKSPACE_BYTES"] <= 16 * ids.size + 8 * ids.size + 64   # the tables and a stage of (bucket, row): no rows


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_repeated_stored_ids_answer_with_the_first_bucket_and_row(capi):
    m0, layers = data(45)
    ids = m0.ids.copy()
    in2, in5 = np.flatnonzero(m0.lab == 2), np.flatnonzero(m0.lab == 5)
    twin = np.uint32(4093 * 77 + 11)
    ids[[in5[0], in2[20], in2[9]]] = twin   # one row of bucket 5 and rows 9 and 20 of bucket 2 carry the same id
    m = Mirror(m0.X, m0.lab, ids)
    idx = fresh(capi, layers, m, L, chunk_rows=256)   # (a relocated bucket reserves its rows + a chunk: 8 row-blocks here)
    try:
        rows, bucket, row = idx.fetch([twin, m.ids[0], twin], where=True)
        assert bucket.tolist()[::2] == [2, 2] and row.tolist()[::2] == [9, 9]
        assert np.array_equal(rows[0], m.X[in2[9]]) and np.array_equal(rows[2], m.X[in2[9]])
        same((rows, bucket, row), expected(table(idx), [twin, m.ids[0], twin], 45))
        # A first, large insert re-packs the slab into allocations with an eighth of headroom (some 140 row-blocks); then bucket 2
        # (exactly one full row-block) takes one more row, outgrows its row-block and moves behind the last bucket -- 10 row-blocks at the
        # tail, which now fit: the answer is by (bucket, row), not by slab position
        rs = np.random.RandomState(5)
        n_big = 3000
        extra = dataset(rs, n_big + 1, 45)
        extra_ids = ((np.arange(n_big + 1, dtype=np.uint64) + 5000) * 4093 + 8).astype(np.uint32)
        assert idx.insert(extra[:n_big], np.full(n_big, 6), extra_ids[:n_big]) == n_big
        before = idx.debug_layout()
        assert idx.insert(extra[n_big:], np.full(1, 2), extra_ids[n_big:]) == 1
        after = idx.debug_layout()
        assert after["counters"][1] == before["counters"][1] + 1, "the setup did not relocate bucket 2"
        assert before["rb_start"][2] < before["rb_start"][5] and after["rb_start"][2] > after["rb_start"][5]
        rows2, bucket2, row2 = idx.fetch([twin, extra_ids[n_big], twin], where=True)
        assert bucket2.tolist() == [2, 2, 2] and row2.tolist() == [9, 32, 9]
        assert np.array_equal(rows2[0], m.X[in2[9]]) and np.array_equal(rows2[1], extra[n_big])
        same((rows2, bucket2, row2), expected(table(idx), [twin, extra_ids[n_big], twin], 45))
        assert idx.delete([twin]) == 3   # every carrier of the id goes: it is absent
        assert idx.locate([twin])[0].tolist() == [-1]
    finally:
        idx.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32-ip", "f32-l2", "exact-ip", "exact-l2"])
def test_after_delete_and_insert(capi, form):
    m0, layers = data(45)
    rs = np.random.RandomState(len(form))
    idx = fresh(capi, layers, m0, L, **FORMS[form])
    try:
        gone = m0.ids[rs.choice(N, 100, replace=False)]
        assert idx.delete(gone) == 100
        new = dataset(rs, 150, 45)
        new_lab = rs.randint(0, L, 150)
        new_ids = ((np.arange(150, dtype=np.uint64) + 9000) * 4093 + 8).astype(np.uint32)
        assert idx.insert(new, new_lab, new_ids) == 150
        everything = np.concatenate([m0.ids, new_ids, ABSENT])[rs.permutation(N + 150 + ABSENT.size)]
        tab = table(idx)
        assert len(tab) == N - 100 + 150
        rows, bucket, row = check(idx, everything, tab, what=form)
        assert (bucket[np.isin(everything, gone)] == -1).all() and (bucket[np.isin(everything, new_ids)] >= 0).all()
        at = {int(i): j for j, i in enumerate(new_ids)}
        for j, i in enumerate(everything.tolist()):   # the inserted rows are the arrays that were inserted
            if i in at:
                assert np.array_equal(rows[j], new[at[i]]) and bucket[j] == new_lab[at[i]]
        assert capi.fetch_last_plan()["FOUND"] == N - 100 + 150
    finally:
        idx.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32-ip", "exact-l2", "f16-ip"])
def test_derived_handles_answer_as_their_own_buckets_say(capi, built, form):
    idx, m = built(45, form, exact16=True)
    layers = data(45, True)[1]
    rs = np.random.RandomState(3)
    other_ids = ((np.arange(90, dtype=np.uint64) + 20000) * 4093 + 8).astype(np.uint32)
    other = fresh(capi, layers, Mirror(half_exact(dataset(rs, 90, 45)), rs.randint(0, L, 90), other_ids), L, **FORMS[form])
    ask = np.concatenate([m.ids, other_ids, ABSENT])[rs.permutation(N + 90 + ABSENT.size)]
    derived = []
    try:
        if form != "f16-ip":
            derived.append(("clone_view", idx.clone_view()))
        derived.append(("subset", idx.subset(m.ids[::2])))
        derived.append(("regroup", idx.regroup(m.ids[:50], (m.lab[:50] + 1) % L, L)))
        derived.append(("concat", idx.concat(other)))
        for name, h in derived:
            for dtype in (np.float32, np.float16):
                tab = table(h, dtype)
                _, bucket, _ = check(h, ask, tab, dtype, (name, form))
                assert int((bucket >= 0).sum()) == {"clone_view": N, "subset": N // 2, "regroup": N, "concat": N + 90}[name]
        check(idx, ask, table(idx), what="the parent, while views and copies live")
    finally:
        for name, h in derived:
            if name != "clone_view":   # (a view is closed with its parent's fixture)
                h.close()
        other.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32-ip", "exact-ip"])
def test_f16_of_a_value_that_is_no_half_is_refused_whole(capi, form):
    from learnedmetricindex_amd._capi import LmiError

    m0, layers = data(45, True)
    X = m0.X.copy()
    X[N - 1, 44] = np.float32(1.0) / np.float32(3.0)   # the last column of the last object: not binary16-exact
    idx = fresh(capi, layers, Mirror(X, m0.lab, m0.ids), L, **FORMS[form])
    try:
        for p in (0, 7):   # one piece; many pieces, the offending row in the last
            capi.fetch_set_geometry(piece_rows=p)
            out = np.full((N, 45), np.float16(-7.5))
            with pytest.raises(LmiError, match=r"lmi_rows_fetch_f16.*binary16"):
                idx.fetch(m0.ids, dtype=np.float16, rows_out=out)
            assert (out == np.float16(-7.5)).all()   # nothing was written
            assert not any(capi.fetch_last_plan().values())
            rows = idx.fetch(m0.ids[:-1], dtype=np.float16, rows_out=out[:-1])
            assert np.array_equal(rows.view(np.uint16), X[:-1].astype(np.float16).view(np.uint16)) and (out[-1] == np.float16(-7.5)).all()
            rows = idx.fetch(np.r_[m0.ids[:3], ABSENT], dtype=np.float16)   # the zero rows of absent ids do not count
            assert not rows[3:].any()
            assert np.array_equal(idx.fetch(m0.ids[-1:]), X[-1:])   # as floats the object is served
    finally:
        capi.fetch_set_geometry(piece_rows=0)
        idx.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32-ip", "exact-ip", "f16-ip"])
@pytest.mark.parametrize("d", [45, 136])
def test_device_in_device_out(capi, built, d, form):
    idx, m = built(d, form, exact16=True)
    ids = np.concatenate([m.ids[::-1], ABSENT, m.ids[:5]])
    n = ids.size
    ids_t = torch.from_numpy(ids.view(np.int32)).cuda()
    try:
        for p in (0, 7):
            capi.fetch_set_geometry(piece_rows=p)
            for dtype, tdtype in ((np.float32, torch.float32), (np.float16, torch.float16)):
                want = idx.fetch(ids, dtype=dtype, where=True)
                rows_t = torch.full((n, d), -3.0, dtype=tdtype, device="cuda")
                bucket_t = torch.full((n,), 99, dtype=torch.int32, device="cuda")
                row_t = torch.full((n,), 99, dtype=torch.int32, device="cuda")
                idx.fetch_device(ids_t, rows_t, bucket_t, row_t)
                assert capi.fetch_last_plan()["PIECES"] == (1 if p == 0 else -(-n // p))
                same((rows_t.cpu().numpy(), bucket_t.cpu().numpy(), row_t.cpu().numpy()), want, (d, form, p))
                rows_t.fill_(-3.0)
                idx.fetch_device(ids_t, rows_t)   # the rows alone
                assert np.array_equal(rows_t.cpu().numpy().view(np.uint8), want[0].view(np.uint8))
                bucket_t.fill_(99)
                idx.fetch_device(ids_t, bucket_t=bucket_t)   # a pure locate
                np.testing.assert_array_equal(bucket_t.cpu().numpy(), want[1])
    finally:
        capi.fetch_set_geometry(piece_rows=0)


# ---- 10, 11 -------------------------------------------------------------------------------------------------------------------
def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


def net_from(layers, model_type="MLP"):
    from learnedmetricindex_amd.li.model import NeuralNetwork

    net = NeuralNetwork(input_dim=layers[0][0].shape[1], output_dim=layers[-1][0].shape[0], model_type=model_type)
    lin = [mod for mod in net.model.layers if isinstance(mod, torch.nn.Linear)]
    with torch.no_grad():
        for mod, (W, b) in zip(lin, layers):
            mod.weight.copy_(torch.from_numpy(W))
            mod.bias.copy_(torch.from_numpy(b))
    return net


_li = {}


@pytest.fixture(scope="module")
def resident():
    """A LearnedIndex with its index resident, per golden fixture: G1 one level (d = 64), G2 two levels [4, 3], G6 one level whose
    navigation vectors (32-d) differ from the scan vectors (96-d).  The scan vectors are rounded to binary16 so that both dtypes read."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_oracle_multilevel import internal_of

    def get(name):
        if name not in _li:
            g = load_golden(name)
            Xn, _, Xs, _ = inputs_for(name, g)
            Xs = half_exact(Xs)
            ncat = [int(v) for v in g["n_categories"]]
            if len(ncat) == 1:
                n_cls = layers_from(g)[-1][0].shape[0]
                li = LearnedIndex(net_from(layers_from(g), "MLP-5" if name == "G6" else "MLP"), {}, [(i,) for i in range(n_cls)])
            else:
                li = LearnedIndex(net_from(layers_from(g)), {p: net_from(l) for p, l in internal_of(g)},
                                  [tuple(int(v) for v in p) for p in g["bucket_paths"]])
            li.prepare(frame(Xn if name == "G6" else Xs), frame(Xs), g["data_prediction"].astype(np.int64), ncat)
            _li[name] = (li, Xn, Xs, ncat)
        return _li[name]
    yield get
    for li, *_ in _li.values():
        li.close()
    _li.clear()


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_li_reconstruct(resident, name):
    li, _, Xs, _ = resident(name)
    n = Xs.shape[0]
    rs = np.random.RandomState(1)
    ids = np.concatenate([rs.randint(1, n + 1, 300), [1, n, n, 1]])   # the frame's labels are 1 .. n
    for dtype in (np.float32, np.float16):
        rows = li.reconstruct(ids, dtype=dtype)
        assert rows.dtype == dtype and np.array_equal(rows.view(np.uint8), Xs[ids - 1].astype(dtype).view(np.uint8))
        mixed = np.concatenate([ids[:20], [0, n + 1, n + 5]])
        rows, found = li.reconstruct(mixed, dtype=dtype, missing="zero")
        np.testing.assert_array_equal(found, np.r_[np.ones(20, bool), np.zeros(3, bool)])
        assert np.array_equal(rows[:20], Xs[mixed[:20] - 1].astype(dtype)) and not rows[20:].any()
        with pytest.raises(KeyError, match=rf"\[0, {n + 1}, {n + 5}\]"):
            li.reconstruct(mixed, dtype=dtype)
    assert li.reconstruct([]).shape == (0, Xs.shape[1])


@pytest.mark.parametrize("merge", ["ranks", "union"])
@pytest.mark.parametrize("name", ["G1", "G2"])
def test_search_like_equals_search_resident_on_the_reconstructed_vectors(resident, name, merge):
    li, _, Xs, ncat = resident(name)
    ids = np.random.RandomState(2).randint(1, Xs.shape[0] + 1, 200)
    V = li.reconstruct(ids)
    for nb, k in ((1, 10), (3, 10)) if merge == "ranks" else ((3, 10), (2, 40)):
        d1, n1, mt = li.search_like(ids, ncat, n_buckets=nb, k=k, merge=merge)
        d2, n2, _ = li.search_resident(V, V, ncat, n_buckets=nb, k=k, merge=merge)
        assert d1.dtype == d2.dtype and d1.shape == d2.shape and np.array_equal(d1.view(np.uint64), d2.view(np.uint64)), (nb, k)
        assert n1.dtype == n2.dtype and np.array_equal(n1, n2), (nb, k)
        assert (n1[:, 0] != 0).all() and "search" in mt
    if merge == "union":   # **kw go where search_resident's go: a filter that excludes the objects themselves
        d1, n1, _ = li.search_like(ids, ncat, n_buckets=3, k=10, merge="union", filter=np.setdiff1d(np.arange(1, Xs.shape[0] + 1), ids))
        d2, n2, _ = li.search_resident(V, V, ncat, n_buckets=3, k=10, merge="union", filter=np.setdiff1d(np.arange(1, Xs.shape[0] + 1), ids))
        assert np.array_equal(d1.view(np.uint64), d2.view(np.uint64)) and np.array_equal(n1, n2) and not np.isin(n1[np.isfinite(d1)], ids).any()
    with pytest.raises(KeyError, match=rf"\[{Xs.shape[0] + 3}\]"):
        li.search_like([1, Xs.shape[0] + 3], ncat)
    d0, n0, _ = li.search_like([], ncat, n_buckets=3, k=10, merge=merge)
    assert d0.shape == n0.shape == (0, 10)


def test_search_like_on_an_index_without_navigation_vectors(resident):
    li, Xn, Xs, ncat = resident("G6")
    assert li._engine.d_nav == 32 and li._engine.d == 96
    ids = np.random.RandomState(4).randint(1, Xs.shape[0] + 1, 100)
    with pytest.raises(ValueError, match="queries_navigation"):
        li.search_like(ids, ncat, n_buckets=3)
    V = li.reconstruct(ids)
    assert np.array_equal(V, Xs[ids - 1])
    for merge in ("ranks", "union"):
        d1, n1, _ = li.search_like(ids, ncat, n_buckets=3, k=10, queries_navigation=Xn[ids - 1], merge=merge)
        d2, n2, _ = li.search_resident(Xn[ids - 1], V, ncat, n_buckets=3, k=10, merge=merge)
        assert np.array_equal(d1.view(np.uint64), d2.view(np.uint64)) and np.array_equal(n1, n2), merge


# ---- 12 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32-ip", "f16-ip"])
def test_sharded_reconstruct_joins_what_the_ranks_own(capi, built, form):
    from learnedmetricindex_amd.sharded import ShardedSearcher

    whole, m = built(45, form, exact16=True)
    world = 3
    owner = np.arange(L) % world
    ranks = []
    try:
        for r in range(world):
            h = capi.Index(0, **FORMS[form])
            h.set_buckets(np.ascontiguousarray(m.X), m.lab, L, ids=np.ascontiguousarray(m.ids), owned=np.ascontiguousarray(owner == r, dtype=np.uint8))
            ranks.append(ShardedSearcher(h, r, world))
        ids = np.concatenate([m.ids[::-1], m.ids[:7]])
        for dtype in (np.float32, np.float16):
            want = whole.fetch(ids, dtype=dtype)
            for r in range(world):
                rows, bucket, _ = ranks[r].fetch_part(ids, dtype)
                np.testing.assert_array_equal(bucket >= 0, owner[m.lab[np.r_[np.arange(N)[::-1], np.arange(7)]]] == r)   # what it owns, nothing else
                assert not rows[bucket < 0].any()
                got = ranks[r].reconstruct(ids, dtype=dtype, peers=[s for s in ranks if s is not ranks[r]])
                assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (r, dtype)
        with pytest.raises(KeyError, match=rf"\[{int(ABSENT[0])}\]"):
            ranks[0].reconstruct(np.r_[m.ids[:3], ABSENT[:1]], peers=ranks[1:])
        with pytest.raises(ValueError, match="peers"):
            ranks[0].reconstruct(m.ids[:3])
    finally:
        for s in ranks:
            s.index.close()


# ---- 13 -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_call(capi, built):
    idx, m = built(8, "f32-ip")
    lib = capi.lib()
    ids = np.ascontiguousarray(m.ids[:4])
    rows = np.full((4, 8), -1.0, np.float32)
    bucket = np.full(4, 99, np.int32)

    def refused(h, ids_p, n, rows_p, bucket_p, row_p, fn=lib.lmi_rows_fetch):
        assert fn(h, ids_p, n, rows_p, bucket_p, row_p, 0) != 0
        return lib.lmi_last_error().decode()

    unbuilt = capi.Index(0)
    try:
        msg = refused(unbuilt._h, ids.ctypes.data, 4, rows.ctypes.data, None, None)
        assert "lmi_rows_fetch" in msg and "not built" in msg
        msg = refused(unbuilt._h, ids.ctypes.data, 4, rows.ctypes.data, None, None, lib.lmi_rows_fetch_f16)
        assert "lmi_rows_fetch_f16" in msg and "not built" in msg
    finally:
        unbuilt.close()
    msg = refused(idx._h, ids.ctypes.data, 4, None, None, None)
    assert "lmi_rows_fetch" in msg and "all NULL" in msg
    for n in (-1, 2 ** 31):
        msg = refused(idx._h, ids.ctypes.data, n, rows.ctypes.data, bucket.ctypes.data, None)
        assert "lmi_rows_fetch" in msg and "outside [0, 2^31)" in msg
    msg = refused(idx._h, None, 4, rows.ctypes.data, None, None)
    assert "lmi_rows_fetch" in msg and "ids is NULL" in msg
    msg = refused(None, ids.ctypes.data, 4, rows.ctypes.data, None, None)
    assert "lmi_rows_fetch" in msg and "NULL handle" in msg
    assert (rows == -1.0).all() and (bucket == 99).all()   # a refused call writes nothing
    assert not any(capi.fetch_last_plan().values())
    assert lib.lmi_rows_fetch(idx._h, None, 0, rows.ctypes.data, None, None, 0) == 0 and (rows == -1.0).all()   # n == 0: nothing to do
    assert lib.lmi_fetch_set_geometry(ctypes.c_int64(-1)) != 0 and "lmi_fetch_set_geometry" in lib.lmi_last_error().decode()
    assert lib.lmi_fetch_set_geometry(ctypes.c_int64((1 << 24) + 1)) != 0
    check(idx, ids, table(idx))   # and the handle serves on
