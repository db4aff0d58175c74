"""Host side of `lmi_train` (no GPU): the numpy restatement of tests/train_ref.py reproduces what the five parity cases were chosen
for and agrees with `torch.optim.Adam` on float64 tensors; `_capi.train` marshals its arguments as include/lmi_hip.h declares them
(against a recording stand-in for the library); `NeuralNetwork.train_batch_hip` draws the reference's effective row schedule; the
builder and the driver know the trainer."""
import ctypes

import numpy as np
import pytest
import torch

import train_ref

from learnedmetricindex_amd import _capi

#: largest |parameter - float64 torch| / lr and largest relative loss deviation of the restatement over a case's steps, as measured
#: with this file's train_ref.py.  B (and, less, D) has gradients within a few 1e-9 of zero, where the 1e-8 of Adam's denominator
#: makes m / (sqrt(v) + eps) follow the float32 rounding of the gradient; the other cases sit at float32 rounding of the parameters.
MEASURED = {"A": (3.1e-6, 2.7e-8), "B": (0.126, 5.9e-8), "C": (3.2e-6, 4.6e-8), "D": (1.3e-3, 5.4e-8), "E": (5.2e-6, 2.9e-8)}
#: asserted: 4x the measured maximum (five cases sample rounding noise thinly) -- per case for the parameters, which is never wider
#: than 4x the maximum over the cases (0.126 lr -> 0.5 lr)
SLACK = 4.0
LOSS_BOUND = SLACK * max(v[1] for v in MEASURED.values())


@pytest.mark.parametrize("name", sorted(train_ref.CASES))
def test_cases_cover_what_they_claim(name):
    c = train_ref.case(name)
    n, d, hidden, classes, bsz, steps, _ = train_ref.CASES[name]
    assert c["x"].shape == (n, d) and c["rows"].shape == (steps, bsz) and c["out"][1][1] == steps
    assert len(c["layers"]) == len(hidden) + 1 and c["layers"][-1][0].shape[0] == classes
    np.testing.assert_allclose(np.linalg.norm(c["x"], axis=1), 1.0, rtol=1e-6)
    for W, b in c["layers"]:
        k = 1.0 / np.sqrt(W.shape[1])
        assert np.abs(W).max() <= k and np.abs(b).max() <= k
    if name in "ADE":
        assert c["dead"] > 0       # hidden units that are dead over a whole batch: whole rows of dW are exact zeros
    if name in "BC":
        assert c["absent"] > 0     # classes without a row in a batch
    repeated = [len(np.unique(r)) < len(r) for r in c["rows"]]
    assert all(repeated) if name == "A" else not any(repeated)
    assert all(np.isfinite(a).all() for a in train_ref.flat(c["out"][0], c["out"][1][0])) and np.isfinite(c["out"][2]).all()


def torch_float64(c):
    params = [torch.tensor(np.array(a), dtype=torch.float64, requires_grad=True) for W, b in c["layers"] for a in (W, b)]
    opt = torch.optim.Adam(params, lr=train_ref.LR)
    x = torch.tensor(np.array(c["x"]), dtype=torch.float64)
    y = torch.tensor(np.array(c["labels"]), dtype=torch.long)
    losses = []
    for rows in c["rows"]:
        a = x[rows]
        for i in range(0, len(params), 2):
            a = a @ params[i].T + params[i + 1]
            if i + 2 < len(params):
                a = torch.relu(a)
        loss = torch.nn.functional.cross_entropy(a, y[rows])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return [p.detach().numpy() for p in params], np.array(losses)


@pytest.mark.parametrize("name", sorted(train_ref.CASES))
def test_restatement_agrees_with_torch_adam_in_float64(name):
    c = train_ref.case(name)
    want, want_losses = torch_float64(c)
    got = [a for wb in c["out"][0] for a in wb]
    dev = max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want)) / train_ref.LR
    loss_dev = float(np.max(np.abs(c["out"][2].astype(np.float64) - want_losses) / np.abs(want_losses)))
    print(f"{name}: parameters {dev:.3g} lr (measured {MEASURED[name][0]:.3g}), loss {loss_dev:.3g} (measured {MEASURED[name][1]:.3g})")
    assert dev <= SLACK * MEASURED[name][0]
    assert loss_dev <= LOSS_BOUND


# ---- _capi.train against a recording stand-in for the library -----------------------------------------------------------------------
class Recorder:
    """Stands in for the loaded library: lmi_train returns 0, is recorded, and writes what a call of one step per row would."""

    def __init__(self):
        self.calls = []

    def lmi_train(self, *args):
        self.calls.append(args)
        self.rows = np.ctypeslib.as_array(ctypes.cast(args[10], ctypes.POINTER(ctypes.c_int64)), shape=(args[11], args[12])).copy()
        t = args[9]._obj
        t.value += args[11]
        return 0


def test_wrapper_marshals_what_the_header_declares(monkeypatch):
    res, args = _capi.SIGNATURES["lmi_train"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[2] is ctypes.c_int64 and args[13] is ctypes.c_double and args[9] == ctypes.POINTER(ctypes.c_int64)
    rec = Recorder()
    monkeypatch.setattr(_capi, "_lib", rec)
    rs = np.random.RandomState(0)
    x = rs.randn(20, 6).astype(np.float32)
    labels = rs.randint(0, 3, 20).astype(np.int32)
    layers = [(rs.randn(4, 6).astype(np.float32), rs.randn(4).astype(np.float32)),
              (rs.randn(3, 4).astype(np.float32), rs.randn(3).astype(np.float32))]
    keep = [(W.copy(), b.copy()) for W, b in layers]
    rows = rs.randint(0, 20, (5, 7)).astype(np.int32)
    out_layers, (adam, t), losses = _capi.train(x, labels, layers, rows, 0.01)
    (device, xp, n, lp, nl, dims, Wp, bp, ap, tp, rp, n_steps, bsz, lr, lossp, on_device), = rec.calls
    assert (device, n, nl, n_steps, bsz, lr, on_device) == (0, 20, 2, 5, 7, 0.01, 0)
    assert xp == x.ctypes.data and lp == labels.ctypes.data            # the caller's arrays, not copies
    assert list(dims) == [6, 4, 3]
    assert [Wp[i] for i in range(2)] == [W.ctypes.data for W, _ in out_layers]
    assert [bp[i] for i in range(2)] == [b.ctypes.data for _, b in out_layers]
    assert [ap[i] for i in range(8)] == [a.ctypes.data for a in adam]
    assert [a.shape for a in adam] == [(4, 6), (4, 6), (4,), (4,), (3, 4), (3, 4), (3,), (3,)] and not any(a.any() for a in adam)
    assert lossp == losses.ctypes.data and losses.shape == (5,) and losses.dtype == np.float32
    assert t == 5                                                      # read back from the int64 the call was handed
    for (W, b), (W0, b0), (Wo, bo) in zip(layers, keep, out_layers):
        assert np.array_equal(W, W0) and np.array_equal(b, b0)         # the initial layers are copied, not trained in place
        assert Wo is not W and bo is not b and Wo.flags.c_contiguous
    # a second call hands the state on: t in, the moments' own buffers
    state = ([a + 1 for a in adam], 5)
    _, (adam2, t2), _ = _capi.train(x, labels, out_layers, rows[:2], 0.5, state=state, device=3)
    args2 = rec.calls[-1]
    assert args2[0] == 3 and args2[11] == 2 and args2[13] == 0.5 and t2 == 7
    assert all(np.array_equal(a, b) for a, b in zip(adam2, state[0])) and all(a is not b for a, b in zip(adam2, state[0]))
    # batch_rows of another integer type arrive as contiguous int64
    assert np.array_equal(rec.rows, rows[:2])


def test_wrapper_refuses_bad_arguments_without_loading_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_capi, "lib", no_lib)
    x = np.zeros((10, 4), dtype=np.float32)
    y = np.zeros(10, dtype=np.int32)
    layers = [(np.zeros((3, 4), np.float32), np.zeros(3, np.float32))]
    rows = np.zeros((2, 5), dtype=np.int64)
    with pytest.raises(ValueError, match="x must be float32"):
        _capi.train(x.astype(np.float64), y, layers, rows, 0.01)
    with pytest.raises(ValueError, match="labels must be int32"):
        _capi.train(x, y.astype(np.int64), layers, rows, 0.01)
    with pytest.raises(ValueError, match=r"labels must be \[10\]"):
        _capi.train(x, y[:9], layers, rows, 0.01)
    with pytest.raises(ValueError, match="layer 0"):
        _capi.train(x, y, [(np.zeros((3, 5), np.float32), np.zeros(3, np.float32))], rows, 0.01)
    with pytest.raises(ValueError, match="batch_rows"):
        _capi.train(x, y, layers, rows[0], 0.01)
    with pytest.raises(ValueError, match="lr"):
        _capi.train(x, y, layers, rows, 0.0)
    with pytest.raises(ValueError, match=r"state\[0\]"):
        _capi.train(x, y, layers, rows, 0.01, state=([np.zeros(3, np.float32)] * 4, 0))
    with pytest.raises(ValueError, match="state t -1"):
        _capi.train(x, y, layers, rows, 0.01, state=([np.zeros((3, 4)), np.zeros((3, 4)), np.zeros(3), np.zeros(3)], -1))
    with pytest.raises(ValueError, match="both"):
        _capi.train(x, torch.zeros(10, dtype=torch.int32), layers, rows, 0.01)


# ---- the row schedule of train_batch_hip ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r", [(1, 1), (256, 256), (257, 1), (100_000, 160), (10_000_000, 128)])
def test_row_schedule(n, r):
    from learnedmetricindex_amd.li.model import NeuralNetwork

    assert NeuralNetwork.hip_batch_size(n) == r
    # what is left for the last mini-batch of a pass in batches of 256
    assert r == len(range(n)[256 * ((n - 1) // 256):])
    rows = NeuralNetwork.hip_batch_rows(np.random.default_rng(2023), n, 3)
    assert rows.shape == (3, r) and rows.dtype == np.int64
    assert ((rows >= 0) & (rows < n)).all()
    assert all(len(np.unique(e)) == r for e in rows)
    assert np.array_equal(rows, NeuralNetwork.hip_batch_rows(np.random.default_rng(2023), n, 3))
    if n > 256:
        assert not np.array_equal(rows[0], rows[1])
        assert not np.array_equal(rows, NeuralNetwork.hip_batch_rows(np.random.default_rng(7), n, 3))
    assert NeuralNetwork.hip_batch_rows(np.random.default_rng(1), n, 0).shape == (0, r)


def test_train_batch_hip_keeps_its_generator_and_state_and_writes_the_weights_back(monkeypatch):
    from learnedmetricindex_amd.li import model

    calls = []

    def fake_train(x, labels, layers, batch_rows, lr, state=None, device=0):
        calls.append((x, labels, [(W.copy(), b.copy()) for W, b in layers], batch_rows, lr, state))
        t = 0 if state is None else state[1]
        return [(W + 1, b + 2) for W, b in layers], ("adam", t + len(batch_rows)), np.arange(len(batch_rows), dtype=np.float32)

    monkeypatch.setattr(model._capi, "train", fake_train)
    net = model.NeuralNetwork(input_dim=6, output_dim=3, lr=0.02, model_type="MLP-8")
    net._engine = "stale"
    before = [(W.copy(), b.copy()) for W, b in model.linear_layers(net.model)]
    x = np.zeros((300, 6), dtype=np.float32)
    y = np.zeros(300, dtype=np.int64)
    losses = net.train_batch_hip(x, y, epochs=4, seed=9)
    assert losses == [0.0, 1.0, 2.0, 3.0] and net._engine is None
    rng = np.random.default_rng(9)
    want = model.NeuralNetwork.hip_batch_rows(rng, 300, 4)
    assert np.array_equal(calls[0][3], want) and want.shape == (4, 300 - 256)
    assert calls[0][1].dtype == np.int32 and calls[0][4] == 0.02 and calls[0][5] is None
    for (W, b), (W0, b0) in zip(model.linear_layers(net.model), before):
        assert np.array_equal(W, W0 + 1) and np.array_equal(b, b0 + 2)      # pickling, index_io and engine() read the modules
    net.train_batch_hip(x, y, epochs=2, seed=12345)                           # the seed of a later round is not used
    assert calls[1][5] == ("adam", 4) and net._hip_state == ("adam", 6)
    assert np.array_equal(calls[1][3], model.NeuralNetwork.hip_batch_rows(rng, 300, 2))
    for (W, b), (W0, b0) in zip(calls[1][2], before):
        assert np.array_equal(W, W0 + 1) and np.array_equal(b, b0 + 2)      # the second round starts from the first's weights


def test_builder_and_driver_know_the_trainer():
    import pandas as pd

    from learnedmetricindex_amd import search
    from learnedmetricindex_amd.li.LearnedIndexBuilder import LearnedIndexBuilder

    assert search.Experiment.from_argv([]).trainer == "torch"
    assert search.Experiment.from_argv(["--trainer", "hip"]).trainer == "hip"
    with pytest.raises(SystemExit):
        search.Experiment.from_argv(["--trainer", "triton"])
    df = pd.DataFrame(np.zeros((4, 2), dtype=np.float32))
    assert LearnedIndexBuilder(df, None).trainer == "torch" and LearnedIndexBuilder(df, None, trainer="hip").trainer == "hip"
    with pytest.raises(ValueError, match="trainer"):
        LearnedIndexBuilder(df, None, trainer="eager")
