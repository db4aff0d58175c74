"""`lmi_train` restated in numpy on top of the unchanged oracle -- shared by test_train_host.py and test_gpu_train.py.

Definition (include/lmi_hip.h): every step runs the Linear/ReLU stack forward on the batch's rows, takes the gradient of the mean
cross-entropy loss and makes one Adam update.  Each of the three products of a layer is `oracle.forward_logits` on ONE layer with a
zero bias -- a k-ordered chain of fmaf from +0 -- with the operands transposed so that the chain index is the contract's: the input
dimension for z, the batch row r for dW, the output o for da.  p is `oracle.softmax`; db is a row-by-row float32 add; Adam is plain
float32 numpy (every operation rounded on its own) with the bias corrections taken on the host in binary64 as running products."""
import functools
import math

import numpy as np

LR = 0.01
F = np.float32
#: name -> (n, d, hidden widths, classes, bsz, steps, seed)
CASES = {
    "A": (500, 45, (32,), 7, 37, 6, 11),        # odd d, ragged B, one row repeated inside each batch
    "B": (3000, 770, (512,), 130, 256, 4, 12),  # d > 768 and no multiple of 32, classes over several tiles, full batch
    "C": (64, 33, (), 33, 1, 5, 13),            # a single Linear, B = 1, one past a tile
    "D": (1000, 96, (256, 128), 10, 232, 5, 14),  # three layers
    "E": (400, 32, (8, 16), 2, 144, 8, 15),     # the reference's narrowest widths, two classes
}


def product(oracle, a, w):
    """out[i][j] = the chain acc = fmaf(a[i][k], w[j][k], acc) from +0, k ascending"""
    w = np.ascontiguousarray(w, dtype=F)
    return oracle.forward_logits([(w, np.zeros(w.shape[0], dtype=F))], np.ascontiguousarray(a, dtype=F), nthreads=4)


def relu(z):
    return np.where(z > 0, z, F(0)).astype(F)


def adam_update(p, m, v, grad, step, r2):
    m = F(0.9) * m + F(0.1) * grad
    v = F(0.999) * v + (F(0.001) * grad) * grad
    den = np.sqrt(v) / r2 + F(1e-8)
    return p - step * (m / den), m, v


def powers(t):
    """(0.9^t, 0.999^t) as t-fold products of the double literals from 1.0"""
    p1 = p2 = 1.0
    for _ in range(t):
        p1 *= 0.9
        p2 *= 0.999
    return p1, p2


def train_ref(oracle, x, labels, layers, batch_rows, lr, state=None, trace=None):
    """(layers, (adam, t), losses) -- what `_capi.train` returns.  trace: a list that receives (z of every layer, labels) per step."""
    x = np.ascontiguousarray(x, dtype=F)
    W = [np.array(w, dtype=F, order="C") for w, _ in layers]
    b = [np.array(v, dtype=F, order="C") for _, v in layers]
    nl = len(W)
    if state is None:
        adam, t = [np.zeros_like(a) for w, v in zip(W, b) for a in (w, w, v, v)], 0
    else:
        adam, t = [np.array(a, dtype=F) for a in state[0]], int(state[1])
    rows = np.asarray(batch_rows, dtype=np.int64)
    losses = np.zeros(rows.shape[0], dtype=F)
    p1, p2 = powers(t)
    for s in range(rows.shape[0]):
        t += 1
        p1 *= 0.9
        p2 *= 0.999
        step, r2 = F(lr / (1.0 - p1)), F(math.sqrt(1.0 - p2))
        B = rows.shape[1]
        a = [x[rows[s]]]
        z = []
        for l in range(nl):
            z.append(oracle.forward_logits([(W[l], b[l])], a[l], nthreads=4))   # one layer: no ReLU inside
            if l + 1 < nl:
                a.append(relu(z[l]))
        y = labels[rows[s]]
        if trace is not None:
            trace.append(([v.copy() for v in z], y.copy()))
        p = oracle.softmax(z[-1])
        onehot = np.zeros_like(p)
        onehot[np.arange(B), y] = F(1)
        g = (p - onehot) * (F(1) / F(B))
        losses[s] = F(np.sum(-np.log(p[np.arange(B), y]).astype(np.float64)) / B)
        for l in range(nl - 1, -1, -1):
            g_prev = None
            if l > 0:   # before W_l is touched
                da = product(oracle, g, W[l].T)
                g_prev = np.where(z[l - 1] > 0, da, F(0)).astype(F)
            dW = product(oracle, g.T, a[l].T)
            db = np.zeros(W[l].shape[0], dtype=F)
            for r in range(B):
                db = db + g[r]
            W[l], adam[4 * l], adam[4 * l + 1] = adam_update(W[l], adam[4 * l], adam[4 * l + 1], dW, step, r2)
            b[l], adam[4 * l + 2], adam[4 * l + 3] = adam_update(b[l], adam[4 * l + 2], adam[4 * l + 3], db, step, r2)
            g = g_prev
    return list(zip(W, b)), (adam, t), losses


def make_case(name):
    """(x f32[n,d] unit-norm mixture rows, labels i32[n], layers uniform(+-1/sqrt(fan_in)), batch_rows i64[steps,bsz])"""
    n, d, hidden, classes, bsz, steps, seed = CASES[name]
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, classes, n)
    cen = rs.randn(classes, d)
    x = (cen[comp] + 0.5 * rs.randn(n, d)).astype(F)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    labels = comp.astype(np.int32)
    dims = (d,) + tuple(hidden) + (classes,)
    layers = []
    for i in range(len(dims) - 1):
        k = 1.0 / math.sqrt(dims[i])
        layers.append((rs.uniform(-k, k, (dims[i + 1], dims[i])).astype(F), rs.uniform(-k, k, dims[i + 1]).astype(F)))
    rows = np.stack([rs.choice(n, bsz, replace=False) for _ in range(steps)]).astype(np.int64)
    if name == "A":
        rows[:, 5] = rows[:, 2]   # the same row twice in every batch
    return x, labels, layers, rows


def _freeze(a):
    if isinstance(a, np.ndarray):
        a.setflags(write=False)
    elif isinstance(a, (list, tuple)):
        for v in a:
            _freeze(v)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of a case, computed once per process and read-only: x, labels, layers (initial), rows, and the restatement's `out` =
    (layers, (adam, t), losses) with `dead` = hidden units that are <= 0 for every row of a step's batch (summed over the steps and
    layers) and `absent` = classes without a row in a step's batch (summed over the steps)."""
    from oracle import lmi_oracle

    lmi_oracle.build()
    x, labels, layers, rows = make_case(name)
    trace = []
    out = train_ref(lmi_oracle, x, labels, layers, rows, LR, trace=trace)
    classes = CASES[name][3]
    dead = sum(int((z <= 0).all(axis=0).sum()) for zs, _ in trace for z in zs[:-1])
    absent = sum(classes - len(np.unique(y)) for _, y in trace)
    return _freeze(dict(x=x, labels=labels, layers=layers, rows=rows, out=out, dead=dead, absent=absent))


def flat(layers, adam):
    """every parameter and moment of a result as one list of arrays, in a fixed order"""
    return [a for w, b in layers for a in (w, b)] + list(adam)
