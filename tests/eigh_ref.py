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


ORDINARY_SCALE = sorted(INPUTS)   # what test_eigh_host.py holds against LAPACK; the inputs of ordinary scale below join it


def exponent(a):
    """e of the contract's scale step: the smallest integer with max|a_ij| < 2^e over i <= j, 0 for the zero matrix."""
    amax = np.abs(np.triu(a)).max()
    return int(np.frexp(amax)[1]) if amax else 0


def base():
    return INPUTS["degenerate"]()


def symmetric(d, entries):
    """The d x d matrix with a[i, j] = a[j, i] = v for (i, j, v) in entries, zero elsewhere."""
    a = np.zeros((d, d))
    for i, j, v in entries:
        a[i, j] = a[j, i] = v
    return a


def mixed_sub():
    """base * 2^600 with one entry that lands below 2^-1022 when the matrix is scaled by 2^-e: the one rounding ldexp may make."""
    a = np.ldexp(base(), 600)
    a[0, 11] = a[11, 0] = (1.0 + 2.0 ** -52) * 2.0 ** -470
    return a


MIXED_SUB_SEEN = (1.0 + 2.0 ** -51 + 2.0 ** -52) * 2.0 ** -418


def mixed_sub_seen(entry=MIXED_SUB_SEEN):
    """mixed_sub's rounding where it shows in v: the entry (2^-1024 (1 + 3 * 2^-52) after scaling, between two subnormals and past
    their midpoint) couples the zero row 3 -- a_33 == 0, so the pair is rotated, with t = 1 / (2 theta) -- to row 11."""
    a = np.ldexp(base(), 600)
    assert not a[3].any()
    a[3, 11] = a[11, 3] = entry
    return a


# Extreme scales: the scaling step far from e = 0, subnormal inputs, an entry that ldexp rounds.
INPUTS.update(scaled_up=lambda: np.ldexp(base(), 900), scaled_down=lambda: np.ldexp(base(), -900),
              subnormal=lambda: np.ldexp(base(), -1040), mixed_sub=mixed_sub, mixed_sub_seen=mixed_sub_seen)
# The branches of the rotation (test_eigh_host.py counts that each is reached): |theta| >= 2^512 once and twice, an infinite theta,
# theta == -0 (a_pp == a_qq against a negative a_pq).
BRANCHES = dict(
    big_theta_d2=lambda: symmetric(2, [(0, 1, 2.0 ** -600), (1, 1, 0.75)]),
    big_theta_d5=lambda: symmetric(5, [(4, 4, 0.75), (0, 4, 2.0 ** -600), (3, 3, 2.0 ** -700), (3, 4, -2.0 ** -620),
                                       (1, 1, 2.0), (2, 2, 1.0), (1, 2, 0.5)]),
    inf_theta=lambda: symmetric(2, [(0, 1, 2.0 ** -1060), (1, 1, 0.75)]),
    neg_zero_theta=lambda: np.array([[1.0, -0.5, 0.25], [-0.5, 1.0, 0.125], [0.25, 0.125, 1.0]]))
INPUTS.update(BRANCHES)
# Spectra: all negative; repeated and unsorted on a diagonal (ties by index, nothing to rotate); the odd sizes with a bye at the
# resident bound (99) and where the pair count does not (127: 64 pairs) and does (129: 65 pairs) run past the streamed tile.
SPECTRA = dict(negative_definite=lambda: -base(), diag_unsorted=lambda: np.diag([3.0, -1.0, 3.0, 0.0, 7.0, -1.0, 3.0]),
               identity9=functools.partial(np.eye, 9), **{f"d{d}": functools.partial(scatter, 3 * d + 5, d, d) for d in (99, 127, 129)})
INPUTS.update(SPECTRA)
ORDINARY_SCALE = sorted(ORDINARY_SCALE + list(BRANCHES) + list(SPECTRA))


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(a, w, v, sweeps) of a named input: computed once, shared, read-only."""
    a = INPUTS[name]()
    out = (a,) + eigh_ref(a)
    for x in out[:3]:
        x.setflags(write=False)
    return out
