"""GPU (`-m gpu`): lmi_knn_f16 and lmi_knn_range_f16, the exact ground truths on binary16 inputs (include/lmi_hip.h), against the
unchanged CPU oracle and against the binary32 calls on the same values widened.

The contract is that of every `_f16` entry point -- bit for bit the namesake's result for the widened values -- so every comparison
is exact: D and dists as uint32 bit patterns, I, lims and ids with array_equal; there is no tolerance anywhere.  The inputs come from
tests/knn_f16_cases.py (drawn as binary32, narrowed once); tests/test_knn_f16_host.py checks on the oracle alone that they have the
properties relied on here."""
import ctypes

import numpy as np
import pytest
import torch

import knn_cases as kc
import knn_f16_cases as hc
import knn_range_ref as kr
import range_ref as rr
from learnedmetricindex_amd import _capi

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(np.finfo(np.float32).max)
SHAPE_IDS = dict(ids=lambda s: "x".join(map(str, s)))


def host(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def same(got, want, what=""):
    D, I = (host(a) for a in got)
    wD, wI = (host(a) for a in want)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == wD.shape and I.shape == wI.shape, what
    np.testing.assert_array_equal(I, wI, err_msg=f"I {what}")
    np.testing.assert_array_equal(D.view(np.uint32), wD.view(np.uint32), err_msg=f"D bits {what}")


def read(res):
    """(lims, dists, ids) of a RangeResult, which is closed."""
    with res:
        return (res.lims,) + res.read()


def same_range(got, want, what=""):
    lims, d, i = (np.ascontiguousarray(a) for a in got[:3])
    np.testing.assert_array_equal(lims, want[0], err_msg=f"lims {what}")
    assert lims.dtype == np.int64 and d.dtype == np.float32 and i.dtype == np.uint32 and d.shape == i.shape == (int(want[0][-1]),), what
    np.testing.assert_array_equal(i, want[2], err_msg=f"ids {what}")
    np.testing.assert_array_equal(d.view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32), err_msg=f"dist bits {what}")


def on_device(*arrays):
    return tuple(torch.from_numpy(np.array(a, order="C")).cuda() for a in arrays)


def shifted(t, halves):
    """A contiguous copy of the 2-d tensor `t` that starts `halves` elements into its storage."""
    flat = torch.empty(t.numel() + halves, dtype=t.dtype, device=t.device)
    out = flat[halves:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() == flat.data_ptr() + halves * t.element_size()
    return out


def vec_form(d):
    return int(d % 8 == 0)


@pytest.mark.parametrize("k", hc.KS)
@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("shape", hc.SHAPES, **SHAPE_IDS)
def test_parity_with_the_oracle_and_with_the_widened_call(oracle, shape, metric, k):
    c = hc.case(*shape)
    got = _capi.knn(c.q16, c.x16, k, metric)
    plan = _capi.knn_last_plan()
    what = f"{shape} {metric} k={k}"
    same(got, hc.truth(oracle, shape, c, k, metric), what + " vs the oracle")
    assert plan["VEC_XB"] == vec_form(shape[2]) and plan["VEC_XQ"] == 0 and plan["PIECES"] == 1, (what, plan)   # (a piece buffer is a whole allocation)
    same(got, _capi.knn(c.q32, c.x32, k, metric), what + " vs lmi_knn on the widened arrays")


@pytest.mark.parametrize("k", [10, 65])
@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("shape", hc.SHAPES, **SHAPE_IDS)
def test_ties_at_the_boundary_go_to_the_lower_row(oracle, shape, metric, k):
    """k = 10 cuts the 52-row tie group, k = 65 contains it: either way its rows come first, ascending, with one score."""
    c = hc.case(*shape)
    g, t = kc.tie_group(shape[1]), hc.tie_queries(shape[0])
    m = min(k, g.size)
    want = np.broadcast_to(g[:m], (t, m))
    np.testing.assert_array_equal(hc.truth(oracle, shape, c, k, metric)[1][:t, :m], want)   # the case still has its ties
    D, I = _capi.knn(c.q16, c.x16, k, metric)
    np.testing.assert_array_equal(I[:t, :m], want)
    assert np.all(D[:t, :m].view(np.uint32) == D[0, 0].view(np.uint32))


@pytest.mark.parametrize("gi", range(4))
@pytest.mark.parametrize("shape", [hc.VEC_SHAPE, hc.ODD_SHAPE], **SHAPE_IDS)
def test_forced_geometry_changes_no_bit(oracle, shape, gi):
    """Pieces, splits and query groups with ragged ends, from host arrays and from device tensors: the automatic result, the forced
    result and the oracle are one, and the geometry is the one lmi_knn makes for the same sizes."""
    nq, nb, d = shape
    geometry = hc.geometries(nb)[gi]
    piece, splits, qrows = geometry
    c = hc.case(*shape)
    dq, db = on_device(c.q16, c.x16)
    try:
        for metric in hc.METRICS:
            for k in (65, 1024):
                want = hc.truth(oracle, shape, c, k, metric)
                _capi.knn_set_geometry(0, 0, 0)
                auto = _capi.knn(c.q16, c.x16, k, metric)
                _capi.knn_set_geometry(*geometry)
                _capi.knn(c.q32, c.x32, k, metric)
                plan32 = _capi.knn_last_plan()
                for kind, q, x in (("host", c.q16, c.x16), ("device", dq, db)):
                    got = _capi.knn(q, x, k, metric)
                    plan = _capi.knn_last_plan()
                    what = f"{shape} {metric} k={k} {geometry} {kind}"
                    same(got, want, what)
                    same(got, auto, what + " vs automatic")
                    rows = piece if kind == "host" else min(piece, nb)
                    assert plan["PIECE_ROWS"] == rows and plan["PIECES"] == -(-nb // rows) and plan["SPLITS"] == splits, (what, plan)
                    if qrows:
                        assert plan["QUERY_ROWS"] == min(qrows, nq) and plan["QUERY_GROUPS"] == -(-nq // min(qrows, nq)), (what, plan)
                    else:
                        assert plan["QUERY_GROUPS"] == 1, (what, plan)
                    assert plan["LIST_ROWS"] == max(256, k) and plan["VEC_XQ"] == 0 and plan["VEC_XB"] == vec_form(d), (what, plan)
                    if kind == "host":   # cut as the binary32 call is; the uploaded queries and piece are halves
                        for w in ("PIECES", "PIECE_ROWS", "SPLITS", "QUERY_GROUPS", "QUERY_ROWS", "LIST_ROWS"):
                            assert plan[w] == plan32[w], (what, w, plan, plan32)
                        assert plan32["WORKSPACE_BYTES"] - plan["WORKSPACE_BYTES"] == 2 * d * (plan["QUERY_ROWS"] + plan["PIECE_ROWS"]), (what, plan, plan32)
    finally:
        _capi.knn_set_geometry(0, 0, 0)


@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("nb", [0, 1, 33])
def test_padding_when_the_base_is_shorter_than_k(oracle, nb, metric):
    c = hc.case(*hc.SHAPES[1])
    q16, x16 = np.ascontiguousarray(c.q16[:9]), np.ascontiguousarray(c.x16[:nb])
    D, I = _capi.knn(q16, x16, 64, metric)
    same((D, I), kc.truth(oracle, ("f16", "pad", nb), hc.widen(q16), hc.widen(x16), 64, metric), f"nb={nb} {metric}")
    assert np.all(I[:, nb:] == -1) and np.all(D[:, nb:] == (-FLT_MAX if metric == "ip" else FLT_MAX)) and np.all(I[:, :nb] >= 0)
    same(_capi.knn(*on_device(q16, x16), 64, metric), (D, I), f"nb={nb} {metric} device")


@pytest.mark.parametrize("metric", hc.METRICS)
def test_no_queries_writes_nothing(metric):
    c = hc.case(*hc.SHAPES[1])
    D, I = _capi.knn(c.q16[:0], c.x16, 64, metric)
    assert D.shape == (0, 64) and I.shape == (0, 64) and D.dtype == np.float32 and I.dtype == np.int64
    guard_d, guard_i = np.full((2, 64), 7, np.float32), np.full((2, 64), 7, np.int64)
    rc = _capi.lib().lmi_knn_f16(0, c.q16.ctypes.data, 0, c.x16.ctypes.data, c.x16.shape[0], c.x16.shape[1], 64, _capi.KNN_METRICS[metric],
                                 guard_d.ctypes.data, guard_i.ctypes.data, 0)
    assert rc == 0 and np.all(guard_d == 7) and np.all(guard_i == 7)
    assert all(v == 0 for v in _capi.knn_last_plan().values())


@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("shape", [hc.SHAPES[1], hc.SHAPES[2], hc.SHAPES[3]], **SHAPE_IDS)
def test_device_tensors(oracle, shape, metric):
    """torch.float16 tensors equal the host call; a base one half into its storage is 2-byte aligned and read element by element, one
    8 halves in is 16-byte aligned again and, where d % 8 == 0, read 16 bytes at a time; the inputs are only read."""
    nq, nb, d = shape
    c = hc.case(*shape)
    k = 65
    want = _capi.knn(c.q16, c.x16, k, metric)
    same(want, hc.truth(oracle, shape, c, k, metric), "host")
    dq, db = on_device(c.q16, c.x16)
    assert dq.dtype == torch.float16 and db.dtype == torch.float16
    D, I = _capi.knn(dq, db, k, metric)
    assert D.is_cuda and I.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64 and D.device == dq.device
    assert _capi.knn_last_plan()["VEC_XB"] == vec_form(d)
    same((D, I), want, "device")
    off1 = shifted(db, 1)
    assert off1.data_ptr() % 16 == 2
    same(_capi.knn(dq, off1, k, metric), want, "base one half in")
    assert _capi.knn_last_plan()["VEC_XB"] == 0
    off8 = shifted(db, 8)
    assert off8.data_ptr() % 16 == 0
    same(_capi.knn(dq, off8, k, metric), want, "base 8 halves in")
    assert _capi.knn_last_plan()["VEC_XB"] == vec_form(d)
    same(_capi.knn(shifted(dq, 1), off1, k, metric), want, "queries and base one half in")
    for t, a in ((dq, c.q16), (db, c.x16), (off1, c.x16), (off8, c.x16)):   # only read
        assert np.array_equal(t.cpu().numpy().view(np.uint16), a.view(np.uint16))
    for a, b in ((c.q16, db), (dq, c.x16), (dq, db.float()), (dq.float(), db)):   # mixed kinds, mixed precisions
        with pytest.raises(ValueError):
            _capi.knn(a, b, k, metric)


@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("d", [40, 45])
def test_special_values_do_what_the_oracle_does(oracle, d, metric):
    """A NaN row, a +inf element, a row of half subnormals, a row of -0.0, rows of +-65504, an all-zero and a -0.0 query."""
    c = hc.special(d)
    want = hc.truth(oracle, ("special", d), c, 64, metric)
    got = _capi.knn(c.q16, c.x16, 64, metric)
    same(got, want, f"{d} {metric}")
    assert not np.any(got[1] == 3)   # the NaN row is never returned
    same(got, _capi.knn(c.q32, c.x32, 64, metric), f"{d} {metric} vs lmi_knn on the widened arrays")
    same(_capi.knn(*on_device(c.q16, c.x16), 64, metric), want, f"{d} {metric} device")
    # the subnormal row against itself: a half subnormal is a normal binary32 value, and widening must not flush it
    sub = np.ascontiguousarray(c.x16[7:8])
    D, _ = _capi.knn(sub, sub, 1, "ip")
    with np.errstate(all="ignore"):
        wD, _ = oracle.knn_ip(hc.widen(sub), hc.widen(sub), 1)
    assert D.view(np.uint32)[0, 0] == wD.view(np.uint32)[0, 0] and D[0, 0] > 0


@pytest.mark.parametrize("metric", hc.METRICS)
@pytest.mark.parametrize("shape", hc.RANGE_SHAPES, **SHAPE_IDS)
def test_range_parity(oracle, shape, metric):
    """Per-query radii -- three in four some row's distance, so dist == radius is met, one in four just below the nearest: an empty
    run -- from host arrays, device tensors and under a forced geometry: knn_range_ref's prefix of the oracle's truth, and
    lmi_knn_range on the widened arrays."""
    nq, nb, d = shape
    c = hc.case(*shape)
    radius, want = hc.recipe(oracle, shape, metric)
    res = _capi.range_knn(c.q16, c.x16, radius, metric)
    counts = res.pair_counts()
    got = read(res)
    plan = _capi.knn_range_last_plan()
    same_range(got, want, f"{shape} {metric} vs the reference")
    np.testing.assert_array_equal(counts, np.diff(got[0]).astype(np.int32)[:, None])
    assert plan["RESULTS"] == got[0][-1] and plan["CHUNK_BYTES"] == 8 * got[0][-1] and plan["PIECES"] == 1
    same_range(got, read(_capi.range_knn(c.q32, c.x32, radius, metric)), f"{shape} {metric} vs lmi_knn_range on the widened arrays")
    plan32 = _capi.knn_range_last_plan()
    assert plan32["WORKSPACE_BYTES"] - plan["WORKSPACE_BYTES"] == 2 * d * (plan["QUERY_ROWS"] + plan["PIECE_ROWS"]), (plan, plan32)
    dq, db = on_device(c.q16, c.x16)
    same_range(read(_capi.range_knn(dq, db, radius, metric)), want, f"{shape} {metric} device")
    same_range(read(_capi.range_knn(dq, shifted(db, 1), radius, metric)), want, f"{shape} {metric} device, base one half in")
    try:
        _capi.knn_set_geometry(1000, 3, 32)
        for kind, q, x in (("host", c.q16, c.x16), ("device", dq, db)):
            same_range(read(_capi.range_knn(q, x, radius, metric)), want, f"{shape} {metric} forced {kind}")
            plan = _capi.knn_range_last_plan()
            assert plan["PIECE_ROWS"] == 1000 and plan["PIECES"] == -(-nb // 1000) and plan["SPLITS"] == 3 and plan["QUERY_ROWS"] == 32, plan
    finally:
        _capi.knn_set_geometry(0, 0, 0)


@pytest.mark.parametrize("metric", hc.METRICS)
def test_range_max_total_and_sort(oracle, metric):
    shape = hc.RANGE_SHAPES[1]
    c = hc.case(*shape)
    radius, want = hc.recipe(oracle, shape, metric)
    total = int(want[0][-1])
    for name, q, x in (("lmi_knn_range_f16", c.q16, c.x16), ("lmi_knn_range", c.q32, c.x32)):   # refused as the namesake refuses it
        with pytest.raises(_capi.LmiError, match=r"%s: more than max_total = %d results: (\d+) had been counted" % (name, total - 1)) as e:
            _capi.range_knn(q, x, radius, metric, max_total=total - 1)
        assert int(str(e.value).split("results: ")[1].split()[0]) == total
        assert all(v == 0 for v in _capi.knn_range_last_plan().values())
    same_range(read(_capi.range_knn(c.q16, c.x16, radius, metric, max_total=total)), want, f"max_total = total {metric}")   # the next call works
    res = ctypes.c_void_p(7)
    r = np.ascontiguousarray(radius)
    rc = _capi.lib().lmi_knn_range_f16(0, c.q16.ctypes.data, shape[0], c.x16.ctypes.data, shape[1], shape[2], _capi.KNN_METRICS[metric],
                                       r.ctypes.data, total - 1, ctypes.byref(res), 0)
    assert rc != 0 and res.value is None
    want_d, want_i = rr.stable_by_distance(*want)
    idx = _capi.Index(0)
    try:
        with _capi.range_knn(c.q16, c.x16, radius, metric) as res:
            assert not res.sorted
            res.sort(idx)
            assert res.sorted
            same_range((res.lims,) + res.read(), (want[0], want_d, want_i), f"sorted {metric}")
    finally:
        idx.close()


def test_refusals_name_the_f16_symbols_and_leave_the_outputs_untouched():
    c = hc.case(*hc.SHAPES[1])
    nq, nb, d = hc.SHAPES[1]
    L = _capi.lib()
    q, x = c.q16.ctypes.data, c.x16.ctypes.data
    D, I = np.full((nq, 1025), 7, np.float32), np.full((nq, 1025), 7, np.int64)
    _capi.knn(c.q16, c.x16, 10)
    # (xq, nq, xb, nb, d, k, metric), the message
    for args, msg in (((q, nq, x, nb, d, 0, 0), b"lmi_knn_f16: k 0 outside [1,1024]"),
                      ((q, nq, x, nb, d, 1025, 0), b"lmi_knn_f16: k 1025 outside [1,1024]"),
                      ((q, 1, x, 1, 4097, 1, 0), b"lmi_knn_f16: d 4097 outside [1,4096]"),
                      ((q, nq, x, nb, 0, 10, 0), b"lmi_knn_f16: d 0 outside [1,4096]"),
                      ((q, nq, x, nb, d, 10, 7), b"lmi_knn_f16: unknown metric 7"),
                      ((q, -1, x, nb, d, 10, 0), b"lmi_knn_f16: nq -1 outside [0, 2^31)"),
                      ((q, nq, x, 1 << 31, d, 10, 0), b"lmi_knn_f16: nb 2147483648 outside [0, 2^31)"),
                      ((None, nq, x, nb, d, 10, 0), b"lmi_knn_f16: xq, D and I must not be NULL"),
                      ((q, nq, None, nb, d, 10, 0), b"lmi_knn_f16: xb must not be NULL")):
        assert L.lmi_knn_f16(0, *args, D.ctypes.data, I.ctypes.data, 0) != 0, args
        assert L.lmi_last_error() == msg, (args, L.lmi_last_error())
        assert np.all(D == 7) and np.all(I == 7), args
        assert all(v == 0 for v in _capi.knn_last_plan().values()), args
    assert L.lmi_knn_f16(0, q, nq, x, nb, d, 10, 0, None, I.ctypes.data, 0) != 0 and np.all(I == 7)
    radius = np.full(nq, 0.5, np.float32)
    r = radius.ctypes.data
    # (xq, nq, xb, nb, d, metric, radius, max_total), the message
    for args, msg in (((q, nq, x, nb, 0, 0, r, 0), b"lmi_knn_range_f16: d 0 outside [1,4096]"),
                      ((q, 1, x, 1, 4097, 0, r, 0), b"lmi_knn_range_f16: d 4097 outside [1,4096]"),
                      ((q, -1, x, nb, d, 0, r, 0), b"lmi_knn_range_f16: nq -1 outside [0, 2^31)"),
                      ((q, nq, x, 1 << 31, d, 0, r, 0), b"lmi_knn_range_f16: nb 2147483648 outside [0, 2^31)"),
                      ((q, nq, x, nb, d, 7, r, 0), b"lmi_knn_range_f16: unknown metric 7"),
                      ((q, nq, x, nb, d, 0, None, 0), b"lmi_knn_range_f16: radius is NULL"),
                      ((None, nq, x, nb, d, 0, r, 0), b"lmi_knn_range_f16: xq must not be NULL"),
                      ((q, nq, None, nb, d, 0, r, 0), b"lmi_knn_range_f16: xb must not be NULL"),
                      ((q, nq, x, nb, d, 0, r, -1), b"lmi_knn_range_f16: max_total -1 is negative")):
        res = ctypes.c_void_p(7)
        assert L.lmi_knn_range_f16(0, *args, ctypes.byref(res), 0) != 0, args
        assert L.lmi_last_error() == msg, (args, L.lmi_last_error())
        assert res.value is None and all(v == 0 for v in _capi.knn_range_last_plan().values()), args
    assert L.lmi_knn_range_f16(0, q, nq, x, nb, d, 0, r, 0, None, 0) != 0
    assert L.lmi_last_error() == b"lmi_knn_range_f16: the result pointer is NULL"
    # nq == 0 and nb == 0 as the namesake has them
    res = _capi.range_knn(c.q16[:0], c.x16, 0.5)
    assert res.nq == 0 and res.total == 0 and np.array_equal(res.lims, [0])
    res.close()
    res = _capi.range_knn(c.q16, c.x16[:0], np.inf)
    assert res.total == 0 and np.array_equal(res.lims, np.zeros(nq + 1, np.int64)) and _capi.knn_range_last_plan()["PIECES"] == 0
    res.close()


@pytest.mark.parametrize("metric", hc.METRICS)
def test_a_binary32_call_after_an_f16_call_returns_what_it_returned_before(metric):
    shape = kc.SHAPES[1]   # lmi_knn's own case: values that are no halves
    xq, xb = kc.case(*shape)
    xb = xb[:1500]
    c = hc.case(*hc.SHAPES[5])
    before = _capi.knn(xq, xb, 65, metric)
    plan_before = _capi.knn_last_plan()
    radius = kr.dists_of(before[0], metric)[:, 20].copy()
    range_before = read(_capi.range_knn(xq, xb, radius, metric))
    _capi.knn(c.q16, c.x16, 65, metric)
    read(_capi.range_knn(c.q16, c.x16, np.inf, metric))
    same(_capi.knn(xq, xb, 65, metric), before, metric)
    assert _capi.knn_last_plan() == plan_before
    same_range(read(_capi.range_knn(xq, xb, radius, metric)), range_before, metric)
