"""GPU (`-m gpu`): `lmi_train_f16` -- `lmi_train` on rows given as binary16 -- against the numpy restatement (tests/train_ref.py,
unchanged) and against `_capi.train`, both on the widened array.  The cases are train_ref's A to E with x narrowed once to float16.
Widening is exact and the named rows land in the same binary32 batch buffer, so weights, biases, both Adam moments and `t` equal
the restatement bit for bit (the losses within test_gpu_train.py's LOSS_RTOL: the device's logf is not the host's) and EVERYTHING,
losses included, equals the float call bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_ref

pytestmark = pytest.mark.gpu
LOSS_RTOL = 2e-6   # test_gpu_train.py's


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


@functools.lru_cache(maxsize=None)
def case(name):
    """train_ref.case(name) with x narrowed: x16 the halves, x the halves widened, out the restatement on x; read-only."""
    from oracle import lmi_oracle

    lmi_oracle.build()
    c = train_ref.case(name)
    x16 = np.ascontiguousarray(c["x"].astype(np.float16))
    x = x16.astype(np.float32)
    out = train_ref.train_ref(lmi_oracle, x, c["labels"], c["layers"], c["rows"], train_ref.LR)
    return train_ref._freeze(dict(x16=x16, x=x, labels=c["labels"], layers=c["layers"], rows=c["rows"], out=out))


@functools.lru_cache(maxsize=None)
def float_call(name):
    """`_capi.train` on the widened array, once per case"""
    from learnedmetricindex_amd import _capi

    c = case(name)
    return train_ref._freeze(_capi.train(c["x"], c["labels"], c["layers"], c["rows"], train_ref.LR))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what="", exact_losses=False):
    (layers, (adam, t), losses), (wl, (wa, wt), wlosses) = got, want
    assert t == wt
    g, w = train_ref.flat(layers, adam), train_ref.flat(wl, wa)
    assert len(g) == len(w)
    for i, (a, b) in enumerate(zip(g, w)):
        assert a.dtype == np.float32 and a.shape == b.shape
        diff = int((bits(a) != bits(b)).sum())
        print(f"{what} array {i} {a.shape}: {diff} of {a.size} words differ")
        assert diff == 0, (what, i, diff, a.size)
    print(f"{what} losses {losses} want {wlosses}")
    if exact_losses:
        assert np.array_equal(bits(losses), bits(wlosses))
    else:
        np.testing.assert_allclose(losses, wlosses, rtol=LOSS_RTOL, atol=0)


@pytest.mark.parametrize("name", sorted(train_ref.CASES))
def test_parity_with_the_restatement_and_with_the_float_call(capi, name):
    c = case(name)
    got = capi.train(c["x16"], c["labels"], c["layers"], c["rows"], train_ref.LR)
    assert_same(got, c["out"], name + " vs the restatement")
    assert_same(got, float_call(name), name + " vs lmi_train on the widened array", exact_losses=True)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("name", ["A", "D"])   # d = 45 and d = 96 (d % 8 == 0: the shift alone takes the 16-byte alignment away)
def test_device_tensors_equal_the_host_call(capi, name, shift):
    c = case(name)
    n, d = c["x16"].shape
    room = torch.zeros(n * d + shift, dtype=torch.float16, device="cuda")
    room[shift:] = torch.from_numpy(np.array(c["x16"])).cuda().reshape(-1)
    xt = room[shift:].reshape(n, d)
    assert xt.data_ptr() % 16 == 2 * shift and xt.is_contiguous()
    yt = torch.from_numpy(np.array(c["labels"])).cuda()
    keep = xt.clone()
    for _ in range(2):
        got = capi.train(xt, yt, c["layers"], c["rows"], train_ref.LR)
        assert_same(got, c["out"], name)
        assert_same(got, float_call(name), name, exact_losses=True)
    assert torch.equal(xt, keep)


@pytest.mark.parametrize("name", ["A", "D"])
def test_two_calls_that_hand_the_state_on_equal_one(capi, name):
    c = case(name)
    cut = 2
    layers, state, l1 = capi.train(c["x16"], c["labels"], c["layers"], c["rows"][:cut], train_ref.LR)
    assert state[1] == cut
    layers, state, l2 = capi.train(c["x16"], c["labels"], layers, c["rows"][cut:], train_ref.LR, state=state)
    assert_same((layers, state, np.concatenate([l1, l2])), float_call(name), name, exact_losses=True)


def test_no_steps_change_nothing(capi):
    c = case("E")
    layers0, state0, _ = c["out"]    # a trained state: moments that are not zero
    layers, (adam, t), losses = capi.train(c["x16"], c["labels"], layers0, c["rows"][:0], train_ref.LR, state=state0)
    assert t == state0[1] and losses.shape == (0,)
    for a, b in zip(train_ref.flat(layers, adam), train_ref.flat(layers0, state0[0])):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_an_unnamed_row_may_hold_anything_and_a_named_one_is_refused(capi, device):
    c = case("C")
    x16 = np.array(c["x16"])
    free = np.setdiff1d(np.arange(x16.shape[0]), c["rows"].ravel())
    x16[free[0], 3] = np.nan
    x16[free[1], 0] = np.inf

    def call(x):
        if device:
            return capi.train(torch.from_numpy(x).cuda(), torch.from_numpy(np.array(c["labels"])).cuda(), c["layers"], c["rows"],
                              train_ref.LR)
        return capi.train(x, c["labels"], c["layers"], c["rows"], train_ref.LR)

    assert_same(call(x16), float_call("C"), "C", exact_losses=True)
    for bad in (np.nan, -np.inf):
        x16[c["rows"][2, 0], 7] = bad
        with pytest.raises(capi.LmiError, match="lmi_train_f16: a named row of x holds a value that is not finite"):
            call(x16)


def test_refusals_carry_the_new_name_and_write_nothing(capi):
    """The argument checks are lmi_train's own (test_gpu_train.py walks all of them): one of each kind under the new name."""
    rs = np.random.RandomState(5)
    n, d, h, cl, bsz, steps = 40, 12, 5, 3, 4, 2
    x16 = rs.randn(n, d).astype(np.float16)
    labels = rs.randint(0, cl, n).astype(np.int32)
    Ws = [rs.randn(h, d).astype(np.float32), rs.randn(cl, h).astype(np.float32)]
    bs = [rs.randn(h).astype(np.float32), rs.randn(cl).astype(np.float32)]
    rows = rs.randint(0, n, (steps, bsz)).astype(np.int64)
    rows[1, 1] = 17
    vp = ctypes.c_void_p
    Wp, bp = (vp * 2)(*[W.ctypes.data for W in Ws]), (vp * 2)(*[b.ctypes.data for b in bs])
    before = [a.copy() for a in Ws + bs]

    def call(x=x16, n_=n, bsz_=bsz, rows_=rows, labels_=labels):
        losses = np.full(steps, 77.0, np.float32)
        t = ctypes.c_int64(3)
        rc = capi.lib().lmi_train_f16(0, None if x is None else x.ctypes.data, n_, labels_.ctypes.data, 2, (ctypes.c_int32 * 3)(d, h, cl),
                                      Wp, bp, None, ctypes.byref(t), rows_.ctypes.data, steps, bsz_, 0.01, losses.ctypes.data, 0)
        try:
            capi._check(rc)
        finally:
            assert t.value == 3 and (losses == 77.0).all()
            for a, b in zip(Ws + bs, before):
                assert a.tobytes() == b.tobytes()

    with pytest.raises(capi.LmiError, match="lmi_train_f16: n 0 < 1"):
        call(n_=0)
    with pytest.raises(capi.LmiError, match="lmi_train_f16: bsz 257 outside"):
        call(bsz_=257)
    with pytest.raises(capi.LmiError, match="lmi_train_f16: x, labels, dims, W and b must not be NULL"):
        call(x=None)
    bad_rows = rows.copy()
    bad_rows[1, 1] = n
    with pytest.raises(capi.LmiError, match=r"lmi_train_f16: batch_rows\[5\] = 40 outside"):
        call(rows_=bad_rows)
    bad_labels = labels.copy()
    bad_labels[17] = cl
    with pytest.raises(capi.LmiError, match="lmi_train_f16: the label 3 of row 17 is outside"):
        call(labels_=bad_labels)
