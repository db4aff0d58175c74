"""numpy restatement of `lmi_eigh` (include/lmi_hip.h states the arithmetic): a cyclic Jacobi eigen-solver in binary64 whose every
operation is written down.  Elementwise only -- no `@`, no BLAS: numpy's float64 `*`, `+`, `-`, `/` and `sqrt` are the correctly
rounded operations the contract names.  `eigh_ref(a, m)` -> (w [m], v [m, d], sweeps); the inputs the tests share are below it."""
import functools

import numpy as np

SWEEP_CAP = 64
RESIDENT_MAX_D = 100   # lmi_eigh_plan.h's bound (the GPU test checks that the library reports the same)


def round_pairs(d: int, r: int):
    """(p, q) index arrays of round r, p < q, the pairs with q >= d (the bye of an odd d) left out."""
    D = d + (d & 1)
    i = np.arange(1, D // 2)
    a = np.concatenate([[D - 1], (r + i) % (D - 1)])
    b = np.concatenate([[r], (r - i) % (D - 1)])
    p, q = np.minimum(a, b), np.maximum(a, b)
    return p[q < d], q[q < d]


def rotations(A, p, q):
    """(c, s, t, rotated) of the pairs, from A as it stands."""
    app, aqq, apq = A[p, p], A[q, q], A[p, q]
    skip = (np.abs(app) + np.abs(apq) == np.abs(app)) & (np.abs(aqq) + np.abs(apq) == np.abs(aqq))
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        t = np.where(np.abs(theta) >= 2.0 ** 512, 1.0 / (2.0 * theta), t)
    t = np.where(skip, 0.0, t)
    c = 1.0 / np.sqrt(t * t + 1.0)
    return np.where(skip, 1.0, c), np.where(skip, 0.0, t * c), t, ~skip


def eigh_ref(a, m=None):
    a = np.asarray(a, dtype=np.float64)
    d = a.shape[0]
    m = d if m is None else m
    up = np.triu(a)
    amax = np.abs(up).max()
    assert np.isfinite(amax)
    e = int(np.frexp(amax)[1]) if amax else 0   # amax = f * 2^e, f in [0.5, 1)
    A = np.ldexp(up, -e)
    A = A + np.triu(A, 1).T
    V = np.eye(d)
    for sweep in range(1, SWEEP_CAP + 1):
        any_rotated = False
        for r in range(d + (d & 1) - 1):
            p, q = round_pairs(d, r)
            c, s, t, rot = rotations(A, p, q)
            any_rotated |= bool(rot.any())
            U, W = A.copy(), V.copy()          # the column step, of A and of V
            U[:, p], U[:, q] = A[:, p] * c - A[:, q] * s, A[:, p] * s + A[:, q] * c
            W[:, p], W[:, q] = V[:, p] * c - V[:, q] * s, V[:, p] * s + V[:, q] * c
            B = U.copy()                       # the row step
            B[p, :], B[q, :] = U[p, :] * c[:, None] - U[q, :] * s[:, None], U[p, :] * s[:, None] + U[q, :] * c[:, None]
            pr, qr, tr = p[rot], q[rot], t[rot]
            B[pr, qr] = 0.0
            B[pr, pr], B[qr, qr] = A[pr, pr] - tr * A[pr, qr], A[qr, qr] + tr * A[pr, qr]
            A, V = np.triu(B) + np.triu(B, 1).T, W   # only i <= j counts; the rest is its mirror
        if not any_rotated:
            break
    else:
        raise RuntimeError(f"eigh_ref: no convergence within {SWEEP_CAP} sweeps")
    diag = np.diagonal(A)
    order = np.argsort(-diag, kind="stable")[:m]
    v = V[:, order].T
    v = v * np.where(v[np.arange(m), np.abs(v).argmax(axis=1)] < 0, -1.0, 1.0)[:, None]
    return np.ldexp(diag[order], e), np.ascontiguousarray(v), sweep


def scatter(n: int, d: int, seed: int, fix=lambda x: x):
    """G = X^T X of seeded Gaussian X [n, d] with decaying column scales (elementwise: no BLAS in this file)."""
    x = fix(np.random.RandomState(seed).randn(n, d) * (0.97 ** np.arange(d)))
    return (x[:, :, None] * x[:, None, :]).sum(axis=0)


def degenerate(x):
    """One column constant (zero after centring: a zero eigenvalue) and two columns equal (a repeated direction)."""
    x[:, 3], x[:, 8] = 2.5, x[:, 5]
    return x - x.mean(axis=0)


#: name -> the symmetric matrix; indefinite: [[0, 1], [1, 0]] embedded at d = 5
INPUTS = {f"d{d}": functools.partial(scatter, 3 * d + 5, d, d) for d in (1, 2, 3, 33, 64, RESIDENT_MAX_D, RESIDENT_MAX_D + 1, 130)}
INPUTS.update(rank20_d70=functools.partial(scatter, 20, 70, 1), degenerate=functools.partial(scatter, 40, 12, 7, degenerate),
              indefinite=lambda: np.pad(np.array([[0.0, 1.0], [1.0, 0.0]]), ((1, 2), (1, 2))), zero=functools.partial(np.zeros, (6, 6)))


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(a, w, v, sweeps) of a named input: computed once, shared, read-only."""
    a = INPUTS[name]()
    out = (a,) + eigh_ref(a)
    for x in out[:3]:
        x.setflags(write=False)
    return out
