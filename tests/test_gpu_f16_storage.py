"""GPU (`-m gpu`): LMI_STORAGE_F16 -- an index that keeps the prefilter's fp16 fragments only (lmi_store16.h) -- against the default
LMI_STORAGE_F32 index of the same rows, bit for bit: ids, distances (compared as uint32), keys and prefilter statistics, through every
kernel that reads a stored row (tail_kernel, select_kernel + rescore_kernel, select_rescore_kernel, fallback_kernel, unpack16_kernel);
the memory it saves, the library's admissibility verdict, its refusals, clone views, owned builds, the multi-level walk, the li API
and the on-disk format.

fp16-exact data is `X.astype(np.float16).astype(np.float32)` of unit-length rows (max|x| < 1: the index scale only grows values); the
queries are quantised the same way where a case says so -- the storages must agree for any f32 query."""
import json
import os

import numpy as np
import pytest

from test_f16_storage_host import CASES
from test_gpu_front import make
from test_gpu_tail import dup_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def q16(a):
    return a.astype(np.float16).astype(np.float32)


def index(capi, X, lab, L, storage, env=None, chunk_rows=256, **kw):
    """An index of (X, lab) in `storage`; `env` is set around the handle's creation only (the library reads it there)."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        idx = capi.Index(0, chunk_rows=chunk_rows, storage=storage)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    idx.set_buckets(X, lab, L, **kw)
    return idx


def scan(idx, Q, order, k):
    d, i, keys = idx.scan_topk(Q, order, k, want_keys=True)
    return d.view(np.uint32), i, keys, idx.prefilter_stats()


def assert_same(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    assert a[3] == b[3], (a[3], b[3])   # (active, survivors, fallbacks)


_data = {}


def data(d):
    """N = 20 000, L = 16, 256 queries, quantised; orders for 8 buckets with unvisited (-1 / out of range) and repeated slots."""
    if d not in _data:
        X, lab, Q, order = make(100 + d, 20_000, d, 16, 256, 8, invalid_frac=0.04, repeat_frac=0.1)
        X, Q = q16(X), q16(Q)
        for a in (X, lab, Q, order):
            a.setflags(write=False)
        _data[d] = (X, lab, Q, order)
    return _data[d]


_pair = {}


def pair(capi, d):
    """The two indexes of data(d), built once per d (one d at a time) and shared by the (n_buckets, k) cases."""
    if d not in _pair:
        test_close_shared_indexes()
        X, lab, _, _ = data(d)
        _pair[d] = (index(capi, X, lab, 16, "f32"), index(capi, X, lab, 16, "f16"))
    return _pair[d]


@pytest.mark.parametrize("nb,k", [(1, 10), (4, 10), (4, 15), (8, 10)])
@pytest.mark.parametrize("d", [45, 64, 128, 136, 200, 768])
def test_equals_f32_storage_bit_for_bit(capi, oracle, d, nb, k):
    """1. Both fragment layouts (d <= 128 / > 128), d not a multiple of 8 / 32, a padded last chunk; n_buckets = 8 takes select_kernel +
    rescore_kernel + merge_ranks_kernel.  The first 64 queries are checked against the oracle as well."""
    X, lab, Q, order = data(d)
    order = np.ascontiguousarray(order[:, :nb])
    f32, f16 = pair(capi, d)
    assert f16.storage == "f16" and f32.storage == "f32"
    a, b = scan(f32, Q, order, k), scan(f16, Q, order, k)
    assert_same(a, b)
    assert b[3][0], "the prefilter path did not run"
    do, io, _ = oracle.search(None, None, X, Q[:64], lab, nb, k, nthreads=4, bucket_order=order[:64, :, None])
    np.testing.assert_array_equal(b[1][:64], io)
    np.testing.assert_array_equal(b[0][:64].view(np.float32), do.astype(np.float32))


ROW_READERS = [   # env -> the plan words (debug_last_plan) of the re-rank form the case is about
    ({}, dict(streamed=1, use_tail=1, tail_merges=1, rescore_small_waves=-1)),                        # tail_kernel
    ({"LMI_TAIL": "0"}, dict(streamed=1, use_tail=0, tail_merges=0, rescore_small_waves=4)),          # select_kernel + rescore_kernel x 2
    ({"LMI_RESCORE_SIMPLE": "1"}, dict(streamed=0, use_tail=0, tail_merges=0, rescore_small_waves=-1)),   # select_rescore_kernel
]


@pytest.mark.parametrize("env,form", ROW_READERS, ids=["default", "LMI_TAIL=0", "LMI_RESCORE_SIMPLE=1"])
def test_every_row_reading_path(capi, env, form):
    """2. tail_kernel | select_kernel + rescore_kernel (small and big form) | select_rescore_kernel, at d = 96."""
    X, lab, Q, order = make(7, 20_000, 96, 16, 256, 4, invalid_frac=0.04, repeat_frac=0.1)
    X, Q = q16(X), q16(Q)
    out = []
    for storage in ("f32", "f16"):
        idx = index(capi, X, lab, 16, storage, env=env)
        out.append(scan(idx, Q, order, 10))
        plan = idx.debug_last_plan()
        assert plan["fast"] == 1 and {f: plan[f] for f in form} == form, (storage, plan)
        idx.close()
    assert_same(*out)
    assert out[1][3][1] > 0, "no survivor was re-scored"


@pytest.mark.parametrize("n_dup,tail", [(40, "1"), (300, "1"), (1500, "1"), (40, "0"), (300, "0")])
def test_hand_overs(capi, n_dup, tail):
    """3. Queries with more survivors than the small ring holds (40 near-copies) and slots flagged for fallback_kernel (300: survivors,
    1 500: candidate overflow), whose fragment loader must really have run.  With the fused tail such a query is re-scored in batches
    through the small ring; with LMI_TAIL=0 it is passed on to rescore_kernel<G, false, true>, the big ring and its 4- and 9-piece chunks."""
    X, lab, L, Q, order = dup_data(7, 64, n_dup, 6 if n_dup < 1000 else 3, 0.0 if n_dup >= 1000 else 1e-6)
    X = q16(X)
    out = []
    for storage in ("f32", "f16"):
        idx = index(capi, X, lab, L, storage, env={"LMI_TAIL": tail}, chunk_rows=2048)
        out.append(scan(idx, Q, order, 10))
        idx.close()
    assert_same(*out)
    if n_dup >= 300:
        assert out[0][3][2] > 0 and out[1][3][2] > 0, "the data was meant to flag slots for fallback_kernel"


@pytest.mark.parametrize("d", [40, 200])
def test_scale_below_one(capi, oracle, d):
    """An admissible index with max|x| >= 1: multiples of 2**-6 in [-4, 4] (s = 1/8: every value times s is a multiple of 2**-9 below 1,
    exact in binary16), so rescale16_kernel scales DOWN without a loss and the readers multiply by 1 / s = 8.  Both fragment shapes."""
    rs = np.random.RandomState(d)
    N, L = 6000, 6
    X = (rs.randint(-256, 257, size=(N, d)) / 64.0).astype(np.float32)
    X[17, 3] = 4.0
    lab = rs.randint(0, L, N).astype(np.int64)
    Q = q16(rs.randn(128, d).astype(np.float32))
    order = np.stack([rs.permutation(L)[:3] for _ in range(128)]).astype(np.int32)
    assert capi.f16_admissible(X)[0] and np.abs(X).max() == 4.0
    f32, f16 = index(capi, X, lab, L, "f32"), index(capi, X, lab, L, "f16")
    a, b = scan(f32, Q, order, 10), scan(f16, Q, order, 10)
    assert_same(a, b)
    do, io, _ = oracle.search(None, None, X, Q[:32], lab, 3, 10, nthreads=4, bucket_order=order[:32, :, None])
    np.testing.assert_array_equal(b[1][:32], io)
    np.testing.assert_array_equal(b[0][:32].view(np.float32), do.astype(np.float32))
    for bkt in range(L):
        rows, _ = f16.read_bucket(bkt)
        np.testing.assert_array_equal(rows.view(np.uint32), X[lab == bkt].view(np.uint32))
    f32.close()
    f16.close()


@pytest.mark.parametrize("d", [64, 768])
def test_memory(capi, d):
    """4. index_bytes of the F16 index <= 0.40 x the F32 index's (derived: (2 Kpad + 4) / (4 dp + 2 Kpad + 4) ~ 0.33-0.34), after the
    build and between the last add_rows and buckets_end: no f32 image exists during the build either."""
    X, lab, _, _ = data(d)
    mid, end = {}, {}
    for storage in ("f32", "f16"):
        idx = capi.Index(0, storage=storage)
        idx.buckets_begin(lab, d, 16)
        for r0 in range(0, X.shape[0], 6000):
            idx.add_rows(X[r0:r0 + 6000], r0)
        mid[storage] = idx.index_bytes()
        idx.buckets_end()
        end[storage] = idx.index_bytes()
        idx.close()
    print(f"d = {d}: index_bytes mid-build f32 {mid['f32']} f16 {mid['f16']} ({mid['f16'] / mid['f32']:.3f}); "
          f"built f32 {end['f32']} f16 {end['f16']} ({end['f16'] / end['f32']:.3f})")
    assert end["f16"] <= 0.40 * end["f32"]
    assert mid["f16"] <= 0.40 * mid["f32"]
    assert end["f16"] >= X.shape[0] * (2 * d + 4)   # it does hold the halves and the ids


@pytest.mark.parametrize("d", [45, 768])
def test_read_back(capi, d):
    """5. read_bucket returns the input rows and ids byte for byte."""
    X, lab, _, _ = data(d)
    ids = (np.arange(X.shape[0], dtype=np.uint32) * 7 + 3).astype(np.uint32)
    idx = index(capi, X, lab, 16, "f16", ids=ids)
    sizes = idx.bucket_sizes()
    np.testing.assert_array_equal(sizes, np.bincount(lab, minlength=16))
    for b in range(16):
        rows, bid = idx.read_bucket(b)
        sel = np.flatnonzero(lab == b)
        np.testing.assert_array_equal(rows.view(np.uint32), X[sel].view(np.uint32))
        np.testing.assert_array_equal(bid, ids[sel])
    idx.close()


@pytest.mark.parametrize("name", [n for n in CASES if n != "quantised gaussian"])
def test_admissibility_verdict(capi, name):
    """6. The library's verdict (a flag read after a synchronise: no fault, and the handle goes on working) equals f16_admissible, with
    each CPU case placed as one row inside otherwise admissible data; a refused handle then takes an F32 build and searches correctly."""
    rows, _ = CASES[name]
    X, lab, Q, order = make(5, 3000, rows.shape[1], 4, 64, 2)
    X, Q = q16(X), q16(Q)
    X[1234] = rows[-1]
    want, reason = capi.f16_admissible(X)
    idx = capi.Index(0, storage="f16")
    if want:
        idx.set_buckets(X, lab, 4)
        got = scan(idx, Q, order, 10)
    else:
        with pytest.raises(capi.LmiError) as e:
            idx.set_buckets(X, lab, 4)
        msg = str(e.value)
        assert "LMI_STORAGE_F16" in msg and (("finite" in msg) == ("finite" in reason)) and (("scale" in msg) == ("scale" in reason)), (msg, reason)
        with pytest.raises(capi.LmiError):
            idx.scan_topk(Q, order, 10)          # no index was built
        idx.set_storage("f32")                   # ... and the handle takes a fresh F32 build
        idx.set_buckets(X, lab, 4)
        got = scan(idx, Q, order, 10)
    ref = index(capi, X, lab, 4, "f32")
    if np.isfinite(X).all():
        assert_same(scan(ref, Q, order, 10), got)
    ref.close()
    idx.close()


def test_refusals(capi):
    """7. F16 with L2, without the prefilter, insert / delete on an F16 index (a search afterwards equals the search before), an
    unknown storage value."""
    X, lab, Q, order = make(9, 4000, 32, 4, 64, 2)
    X = q16(X)
    with pytest.raises(capi.LmiError, match="L2"):
        capi.Index(0, metric="l2", storage="f16")
    with pytest.raises(capi.LmiError, match="prefilter"):
        capi.Index(0, prefilter=False, storage="f16")
    idx = capi.Index(0, storage="f16")
    idx.set_prefilter(False)                     # the other order: refused where the build starts, the handle as it was
    with pytest.raises(capi.LmiError, match="prefilter"):
        idx.buckets_begin(lab, 32, 4)
    idx.set_prefilter(True)
    idx.set_buckets(X, lab, 4)
    before = scan(idx, Q, order, 10)
    with pytest.raises(capi.LmiError, match="LMI_STORAGE_F16"):
        idx.insert(X[:3], lab[:3], np.array([90001, 90002, 90003], dtype=np.uint32))
    with pytest.raises(capi.LmiError, match="LMI_STORAGE_F16"):
        idx.delete(np.array([1, 2, 3], dtype=np.uint32))
    assert_same(before, scan(idx, Q, order, 10))
    with pytest.raises(capi.LmiError, match="unknown storage 7"):
        capi._check(capi.lib().lmi_set_storage(idx._h, 7))
    assert_same(before, scan(idx, Q, order, 10))
    idx.close()


def test_clone_view_and_owned_build(capi):
    """8. A clone view of an F16 index answers like its parent; an owned-mask build through add_owned_rows (half the buckets)
    in F16 equals the same build in F32."""
    X, lab, Q, order = data(64)
    order = np.ascontiguousarray(order[:, :4])
    _, f16 = pair(capi, 64)
    view = f16.clone_view()
    assert view.storage == "f16"
    assert_same(scan(f16, Q, order, 10), scan(view, Q, order, 10))
    view.close()
    owned = (np.arange(16) % 2 == 0).astype(np.uint8)
    rows = np.flatnonzero(owned[lab] == 1).astype(np.int64)
    out = []
    for storage in ("f32", "f16"):
        idx = capi.Index(0, chunk_rows=256, storage=storage)
        idx.buckets_begin(lab, 64, 16, owned=owned)
        half = rows.shape[0] // 2
        idx.add_owned_rows(X[rows[half:]], rows[half:])
        idx.add_owned_rows(X[rows[:half]], rows[:half])
        idx.buckets_end()
        out.append(scan(idx, Q, order, 10))
        idx.close()
    assert_same(*out)
    assert (out[1][1] != 0).any()


def test_multi_level(capi):
    """9. One [4, 3] tree built the way test_gpu_path_mass.py builds its trees: search_tree with path_mass off and at 0.9."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from path_mass_ref import synthetic_tree
    from test_gpu_path_mass import frame, net_from

    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree([4, 3])
    Xs = q16(Xs / np.linalg.norm(Xs, axis=1, keepdims=True))
    out = {}
    for storage in ("f32", "f16"):
        li = LearnedIndex(net_from(root), {tuple(p): net_from(l) for p, l in internal}, bucket_paths)
        eng = li.prepare(frame(Xn), frame(Xs), dp, [4, 3], storage=storage)
        assert eng.storage == storage
        for mass in (0.0, 0.9):
            eng.set_path_mass(mass)
            d, i, keys, slab, ent = eng.search_tree(Qn, Qs, 5, 10, want_keys=True, want_order=True)
            out[storage, mass] = (d.view(np.uint32), i, keys, slab, ent)
        li.close()
    for mass in (0.0, 0.9):
        for a, b in zip(out["f32", mass], out["f16", mass]):
            np.testing.assert_array_equal(a, b)
    assert (out["f16", 0.9][4] < 0).sum() > (out["f16", 0.0][4] < 0).sum()   # the stop did cut walks short


def test_li_api_and_disk(capi, tmp_path):
    """10. li.search(storage="f16") == storage="f32" on a 5 000 x 64 frame of float16-origin data; insert / delete on the f16-resident
    index raise the library's refusal; save_index -> load_index keeps the storage; a directory without the key loads as f32."""
    from learnedmetricindex_amd import index_io
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from test_gpu_path_mass import frame, net_from

    rs = np.random.RandomState(11)
    X16 = rs.randn(5000, 64).astype(np.float32)
    X16 = (X16 / np.linalg.norm(X16, axis=1, keepdims=True)).astype(np.float16)   # the data as it is distributed
    X = X16.astype(np.float32)
    Q = q16(X[rs.randint(0, 5000, 200)] + 0.05 * rs.randn(200, 64).astype(np.float32))
    layers = [((rs.randn(128, 64) * 0.3).astype(np.float32), (rs.randn(128) * 0.1).astype(np.float32)),
              ((rs.randn(12, 128) * 0.3).astype(np.float32), (rs.randn(12) * 0.1).astype(np.float32))]
    dp = rs.randint(0, 12, 5000).astype(np.int64)
    df = frame(X)
    li = LearnedIndex(net_from(layers), {}, [(i,) for i in range(12)])
    d32, n32, _ = li.search(df, Q, df, Q, dp, [12], n_buckets=3, k=10)
    assert li._engine.storage == "f32"
    d16, n16, _ = li.search(df, Q, df, Q, dp, [12], n_buckets=3, k=10, storage="f16")
    assert li._engine.storage == "f16"              # the storage is part of the resident copy's key: it was rebuilt
    np.testing.assert_array_equal(n16, n32)
    np.testing.assert_array_equal(d16, d32)
    with pytest.raises(capi.LmiError, match="LMI_STORAGE_F16"):
        li.insert(frame(X[:2]), ids=[70001, 70002])
    with pytest.raises(capi.LmiError, match="LMI_STORAGE_F16"):
        li.delete([1, 2])
    path = str(tmp_path / "idx16")
    index_io.save_index(path, li, [12])
    assert json.load(open(os.path.join(path, "meta.json")))["storage"] == "f16"
    li2, ncat = index_io.load_index(path)
    assert li2._engine.storage == "f16"
    d2, n2, _ = li2.search_resident(Q, Q, ncat, n_buckets=3, k=10)
    np.testing.assert_array_equal(n2, n32)
    np.testing.assert_array_equal(d2, d32)
    li2.close()
    li3, _ = index_io.load_index(path, storage="f32")           # the caller's choice overrides the directory's
    assert li3._engine.storage == "f32"
    li3.close()
    meta = json.load(open(os.path.join(path, "meta.json")))
    del meta["storage"]                                         # a directory written before the key existed
    json.dump(meta, open(os.path.join(path, "meta.json"), "w"))
    li4, _ = index_io.load_index(path)
    assert li4._engine.storage == "f32"
    d4, n4, _ = li4.search_resident(Q, Q, ncat, n_buckets=3, k=10)
    np.testing.assert_array_equal(n4, n32)
    np.testing.assert_array_equal(d4, d32)
    li4.close()
    # a refused build surfaces as the library's error and leaves nothing resident
    raw = frame(rs.randn(5000, 64).astype(np.float32))
    with pytest.raises(capi.LmiError, match="binary16"):
        li.search(raw, Q, raw, Q, dp, [12], n_buckets=3, k=10, storage="f16")
    assert li._engine is None
    li.close()


def test_close_shared_indexes():
    """(the indexes shared by the cases above)"""
    for pr in _pair.values():
        for idx in pr:
            idx.close()
    _pair.clear()
