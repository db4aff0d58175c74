"""GPU (`-m gpu`): `lmi_train` -- Adam steps on a Linear/ReLU stack on the device -- against its numpy restatement
(tests/train_ref.py, on top of the unchanged oracle's `forward_logits` and `softmax`).  Weights, biases and both Adam moments are
compared as uint32 bit patterns and `t` exactly; the losses to rtol 2e-6 (logf is <= 2 ulp on either side, plus one final rounding:
about 5e-7).  The five cases cover odd and wide d, ragged and full batches, B = 1, a single Linear and three layers, a repeated row,
dead hidden units and absent classes (test_train_host.py pins that they do)."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import synth
import train_ref

pytestmark = pytest.mark.gpu
LOSS_RTOL = 2e-6


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what=""):
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
    np.testing.assert_allclose(losses, wlosses, rtol=LOSS_RTOL, atol=0)


@pytest.mark.parametrize("name", sorted(train_ref.CASES))
def test_parity_with_the_restatement(capi, name):
    c = train_ref.case(name)
    assert_same(capi.train(c["x"], c["labels"], c["layers"], c["rows"], train_ref.LR), c["out"], name)


@pytest.mark.parametrize("name", ["A", "D"])
def test_device_tensors_equal_the_host_call(capi, name):
    c = train_ref.case(name)
    xt, yt = torch.from_numpy(np.array(c["x"])).cuda(), torch.from_numpy(np.array(c["labels"])).cuda()
    keep = xt.clone()
    for _ in range(2):
        assert_same(capi.train(xt, yt, c["layers"], c["rows"], train_ref.LR), c["out"], name)
    assert torch.equal(xt, keep)


@pytest.mark.parametrize("name", ["A", "D"])
def test_two_calls_that_hand_the_state_on_equal_one(capi, name):
    c = train_ref.case(name)
    cut = 2
    layers, state, l1 = capi.train(c["x"], c["labels"], c["layers"], c["rows"][:cut], train_ref.LR)
    assert state[1] == cut
    layers, state, l2 = capi.train(c["x"], c["labels"], layers, c["rows"][cut:], train_ref.LR, state=state)
    assert_same((layers, state, np.concatenate([l1, l2])), c["out"], name)


def test_no_steps_change_nothing(capi):
    c = train_ref.case("E")
    layers0, state0, _ = c["out"]    # a trained state: moments that are not zero
    layers, (adam, t), losses = capi.train(c["x"], c["labels"], layers0, c["rows"][:0], train_ref.LR, state=state0)
    assert t == state0[1] and losses.shape == (0,)
    for a, b in zip(train_ref.flat(layers, adam), train_ref.flat(layers0, state0[0])):
        assert np.array_equal(bits(a), bits(b))


def test_an_unnamed_row_may_hold_anything(capi):
    c = train_ref.case("C")
    x = np.array(c["x"])
    free = np.setdiff1d(np.arange(x.shape[0]), c["rows"].ravel())
    x[free[0], 3] = np.nan
    assert_same(capi.train(x, c["labels"], c["layers"], c["rows"], train_ref.LR), c["out"], "C")


# ---- refusals: argument and data checks, none of them launches a training step ----------------------------------------------------
N, D, H, C, BSZ, STEPS = 40, 12, 5, 3, 4, 2
REFUSALS = {
    "n_0": (dict(n=0), "n 0 < 1"),
    "layers_0": (dict(n_layers=0), "n_layers 0 outside"),
    "layers_9": (dict(n_layers=9), "n_layers 9 outside"),
    "d_4097": (dict(dims=[4097, H, C]), r"dims\[0\] = 4097 outside"),
    "hidden_0": (dict(dims=[D, 0, C]), r"dims\[1\] = 0 outside"),
    "hidden_4097": (dict(dims=[D, 4097, C]), r"dims\[1\] = 4097 outside"),
    "classes_0": (dict(dims=[D, H, 0]), "0 classes outside"),
    "classes_16385": (dict(dims=[D, H, 16385]), "16385 classes outside"),
    "bsz_0": (dict(bsz=0), "bsz 0 outside"),
    "bsz_257": (dict(bsz=257), "bsz 257 outside"),
    "steps_neg": (dict(n_steps=-1), "n_steps -1 outside"),
    "steps_100001": (dict(n_steps=100001), "n_steps 100001 outside"),
    "lr_nan": (dict(lr=float("nan")), "lr .* not a finite positive"),
    "lr_inf": (dict(lr=float("inf")), "lr .* not a finite positive"),
    "lr_0": (dict(lr=0.0), "lr .* not a finite positive"),
    "lr_neg": (dict(lr=-0.01), "lr .* not a finite positive"),
    "t_neg": (dict(t=-1), r"\*t = -1 < 0"),
    "null_x": (dict(null="x"), "must not be NULL"),
    "null_labels": (dict(null="labels"), "must not be NULL"),
    "null_W1": (dict(null="W1"), "NULL weight/bias for layer 1"),
    "null_b0": (dict(null="b0"), "NULL weight/bias for layer 0"),
    "null_adam5": (dict(null="adam5"), r"adam\[5\] is NULL"),
    "null_rows": (dict(null="rows"), "batch_rows must not be NULL"),
    "row_n": (dict(poke_row=N), r"batch_rows\[5\] = 40 outside"),
    "row_neg": (dict(poke_row=-1), r"batch_rows\[5\] = -1 outside"),
    "label_3": (dict(poke_label=C), "label 3 of row 17 is outside"),
    "label_neg": (dict(poke_label=-1), "label -1 of row 17 is outside"),
    "label_3_device": (dict(poke_label=C, device=True), "label of a named row is outside"),
    "nan_x": (dict(poke_x=np.nan), "named row of x holds a value that is not finite"),
    "inf_x_device": (dict(poke_x=np.inf, device=True), "named row of x holds a value that is not finite"),
    "inf_W": (dict(poke_W=np.inf), "initial weights hold a value that is not finite"),
    "nan_b": (dict(poke_b=np.nan), "initial weights hold a value that is not finite"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_name_the_condition_and_write_nothing(capi, name):
    spec, message = REFUSALS[name]
    rs = np.random.RandomState(5)
    x = rs.randn(N, D).astype(np.float32)
    labels = rs.randint(0, C, N).astype(np.int32)
    Ws = [rs.randn(H, D).astype(np.float32), rs.randn(C, H).astype(np.float32)]
    bs = [rs.randn(H).astype(np.float32), rs.randn(C).astype(np.float32)]
    adam = [rs.rand(*a.shape).astype(np.float32) for W, b in zip(Ws, bs) for a in (W, W, b, b)]
    rows = rs.randint(0, N, (STEPS, BSZ)).astype(np.int64)
    rows[1, 1] = 17    # batch_rows[5]
    if "poke_row" in spec:
        rows[1, 1] = spec["poke_row"]
    if "poke_label" in spec:
        labels[17] = spec["poke_label"]
    if "poke_x" in spec:
        x[17, 5] = spec["poke_x"]
    if "poke_W" in spec:
        Ws[1][2, 3] = spec["poke_W"]
    if "poke_b" in spec:
        bs[0][1] = spec["poke_b"]
    losses = np.full(STEPS, 77.0, np.float32)
    t = ctypes.c_int64(spec.get("t", 3))
    before = [a.copy() for a in Ws + bs + adam]
    null = spec.get("null", "")
    dims = spec.get("dims", [D, H, C])
    vp = ctypes.c_void_p
    Wp = (vp * 2)(*[None if null == f"W{i}" else W.ctypes.data for i, W in enumerate(Ws)])
    bp = (vp * 2)(*[None if null == f"b{i}" else b.ctypes.data for i, b in enumerate(bs)])
    ap = (vp * 8)(*[None if null == f"adam{i}" else a.ctypes.data for i, a in enumerate(adam)])
    on_device = 1 if spec.get("device") else 0
    xa, la = (torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()) if on_device else (x, labels)
    xp = None if null == "x" else (xa.data_ptr() if on_device else xa.ctypes.data)
    lp = None if null == "labels" else (la.data_ptr() if on_device else la.ctypes.data)
    with pytest.raises(capi.LmiError, match=message):
        capi._check(capi.lib().lmi_train(0, xp, spec.get("n", N), lp, spec.get("n_layers", 2), (ctypes.c_int32 * 3)(*dims), Wp, bp, ap,
                                         ctypes.byref(t), None if null == "rows" else rows.ctypes.data, spec.get("n_steps", STEPS),
                                         spec.get("bsz", BSZ), spec.get("lr", 0.01), losses.ctypes.data, on_device))
    for a, b in zip(Ws + bs + adam, before):
        assert a.tobytes() == b.tobytes()
    assert t.value == spec.get("t", 3) and (losses == 77.0).all()


# ---- the builder ------------------------------------------------------------------------------------------------------------------
def frame(X):
    df = pd.DataFrame(X)
    df.index += 1
    return df


@pytest.fixture(scope="module")
def mixture():
    return synth.mixture(2023, 5000, 64, 12, 200)


def build(X, ncat):
    from learnedmetricindex_amd.li.BuildConfiguration import BuildConfiguration
    from learnedmetricindex_amd.li.clustering import algorithms
    from learnedmetricindex_amd.li.LearnedIndexBuilder import LearnedIndexBuilder

    torch.manual_seed(2023)   # the initial weights are torch's
    cfg = BuildConfiguration([algorithms["hip_kmeans"]], [20], ["MLP"], [0.01], ncat)
    return LearnedIndexBuilder(frame(X), cfg, trainer="hip").build()


@pytest.mark.parametrize("ncat", [[12], [4, 3]])
def test_builder_is_repeatable_and_meets_the_stopping_rule(capi, mixture, ncat):
    from learnedmetricindex_amd.li.model import linear_layers

    X, _ = mixture
    runs = [build(X, ncat) for _ in range(2)]
    (li1, dp1, nb1, _, _), (li2, dp2, nb2, _, _) = runs
    assert dp1.shape == (5000, len(ncat)) and dp1.dtype == np.int64
    assert np.array_equal(dp1, dp2) and nb1 == nb2 and li1.bucket_paths == li2.bucket_paths
    models1 = [li1.root_model] + list(li1.internal_models.values())
    models2 = [li2.root_model] + list(li2.internal_models.values())
    assert list(li1.internal_models) == list(li2.internal_models) and len(models1) == (1 if len(ncat) == 1 else 1 + ncat[0])
    for m1, m2 in zip(models1, models2):
        for (W1, b1), (W2, b2) in zip(linear_layers(m1.model), linear_layers(m2.model)):
            assert np.array_equal(bits(W1), bits(W2)) and np.array_equal(bits(b1), bits(b2))
        assert m1._hip_state[1] == m2._hip_state[1] and m1._hip_state[1] % 20 == 0 and m1._hip_state[1] >= 20
    # every category is predicted for at least one object: the reference's stopping rule
    assert len(np.unique(dp1[:, 0])) == ncat[0]
    for path, m in li1.internal_models.items():
        under = dp1[dp1[:, 0] == path[0]]
        assert len(np.unique(under[:, 1])) == linear_layers(m.model)[-1][0].shape[0]
    li1.close()
    li2.close()


def test_builder_search_equals_the_oracle_with_those_weights(capi, oracle, mixture):
    from learnedmetricindex_amd.li.model import linear_layers

    X, Q = mixture
    li, dp, n_buckets, _, _ = build(X, [12])
    root = linear_layers(li.root_model.model)
    np.testing.assert_array_equal(dp[:, 0], oracle.predict(root, X))   # the device-tensor placement is the model's argmax
    df = frame(X)
    dists, nns, _ = li.search(df, Q, df, Q, dp, [12], 3, 10)
    do, no, _ = oracle.search(root, Q, X, Q, dp, 3, 10)
    np.testing.assert_array_equal(nns, no)
    assert np.array_equal(np.asarray(dists, dtype=np.float64).view(np.uint64), np.asarray(do, dtype=np.float64).view(np.uint64))
    li.close()
