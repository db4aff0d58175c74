"""A PCA projection fitted and applied on the device: navigation vectors for data that comes without a `pca32` / `pca96` kind.

`PcaProjection.fit(x, m)` takes the mean and the centred scatter matrix from `_capi.gram` (bit for bit reproducible: include/lmi_hip.h)
and solves the d x d eigenproblem on the host -- or, with `solver="hip"`, on the device by `_capi.eigh`; `.transform(x)` is
`_capi.project`.  There is no CPU fallback for any of these calls."""
from __future__ import annotations

import numpy as np

try:
    from . import _capi   # the package
except ImportError:
    import _capi          # next to _capi.py on sys.path (search.py's layout)


class PcaProjection:
    """`mean` f32 [d], `basis` f32 [m, d] (rows: principal directions, by descending eigenvalue, each with its largest-magnitude
    entry positive), `explained_variance` f64 [m] (the eigenvalues of gram / (n - 1)).

    The eigen-solve is LAPACK's (`np.linalg.eigh` in float64) and NOT part of the bit-for-bit contract: `mean` and the scatter
    matrix are reproducible to the bit, the basis only as far as LAPACK is on the machine at hand.  `transform` is reproducible
    to the bit for a given (mean, basis): keep a fitted projection with `save` rather than fitting it again elsewhere.
    With `solver="hip"` the eigen-solve is `lmi_eigh` and the basis is part of the bit-for-bit contract too."""

    def __init__(self, mean, basis, explained_variance):
        self.mean = np.ascontiguousarray(mean, dtype=np.float32)
        self.basis = np.ascontiguousarray(basis, dtype=np.float32)
        self.explained_variance = np.ascontiguousarray(explained_variance, dtype=np.float64)
        if self.basis.ndim != 2 or self.mean.shape != (self.basis.shape[1],) or self.explained_variance.shape != (self.basis.shape[0],):
            raise ValueError(f"PcaProjection: mean {self.mean.shape}, basis {self.basis.shape} and explained_variance "
                             f"{self.explained_variance.shape} do not fit [d], [m,d], [m]")

    @property
    def m(self) -> int:
        return int(self.basis.shape[0])

    @property
    def d(self) -> int:
        return int(self.basis.shape[1])

    @classmethod
    def fit(cls, x, m: int, device: int = 0, solver: str = "lapack") -> "PcaProjection":
        """`x`: what `_capi.gram` takes (float32 or float16 [n,d], numpy or a device tensor), n >= 2; 1 <= m <= min(d, 1024).
        `solver`: "lapack" (`np.linalg.eigh` of gram / (n - 1) on the host) or "hip" (`_capi.eigh` of gram itself, where it lies;
        the eigenvalues are divided by n - 1 afterwards, so the matrix solved is the integer-exact scatter matrix)."""
        if getattr(x, "ndim", 0) != 2:
            raise ValueError("PcaProjection.fit: x must be [n,d]")
        n, d, m = int(x.shape[0]), int(x.shape[1]), int(m)
        if n < 2:
            raise ValueError(f"PcaProjection.fit: n {n} < 2")
        if m < 1 or m > min(d, _capi.PROJECT_MAX_M):
            raise ValueError(f"PcaProjection.fit: m {m} outside [1, min(d = {d}, {_capi.PROJECT_MAX_M})]")
        if solver not in ("lapack", "hip"):
            raise ValueError(f"PcaProjection.fit: solver {solver!r} is neither 'lapack' nor 'hip'")
        mean, g = _capi.gram(x, device=device)
        if solver == "hip":
            w, v, _ = _capi.eigh(g, m, device=device)
            if not isinstance(mean, np.ndarray):
                mean, w, v = mean.cpu().numpy(), w.cpu().numpy(), v.cpu().numpy()
            return cls(mean, v.astype(np.float32), w / float(n - 1))
        if not isinstance(mean, np.ndarray):
            mean, g = mean.cpu().numpy(), g.cpu().numpy()
        w, v = np.linalg.eigh(g / float(n - 1))   # ascending
        order = np.argsort(w, kind="stable")[::-1][:m]
        basis = v[:, order].T
        lead = basis[np.arange(m), np.abs(basis).argmax(axis=1)]
        basis = basis * np.where(lead < 0, -1.0, 1.0)[:, None]
        return cls(mean, basis.astype(np.float32), w[order])

    def transform(self, x, device: int = 0):
        """f32 [n, m]: numpy for a numpy `x`, a tensor on x's device for a device tensor (`_capi.project`)."""
        return _capi.project(x, self.basis, mean=self.mean, device=device)

    def save(self, path) -> None:
        np.savez(path, mean=self.mean, basis=self.basis, explained_variance=self.explained_variance)

    @classmethod
    def load(cls, path) -> "PcaProjection":
        with np.load(path) as z:
            return cls(z["mean"], z["basis"], z["explained_variance"])


class SketchProjection:
    """Hyperplanes that turn vectors into bit-packed Hamming codes on the device (`_capi.sketch`): `basis` f32 [bits, d], `mean`
    f32 [d] or None, `thresh` f32 [bits] or None (+0).  Bit j of a row is `((x - mean) . basis[j]) > thresh[j]`, with the arithmetic
    of `_capi.project`; the codes are reproducible to the bit for a given (basis, mean, thresh).  `bits` is a multiple of 32 in
    [32, SKETCH_MAX_BITS], the range of `_capi.knn_hamming`."""

    def __init__(self, basis, mean=None, thresh=None):
        self.basis = np.ascontiguousarray(basis, dtype=np.float32)
        self.mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float32)
        self.thresh = None if thresh is None else np.ascontiguousarray(thresh, dtype=np.float32)
        if self.basis.ndim != 2 or self.basis.shape[1] < 1:
            raise ValueError(f"SketchProjection: basis {self.basis.shape} is not [bits, d]")
        if self.bits < 32 or self.bits > _capi.SKETCH_MAX_BITS or self.bits % 32:
            raise ValueError(f"SketchProjection: bits {self.bits} is not a multiple of 32 in [32, {_capi.SKETCH_MAX_BITS}]")
        if (self.mean is not None and self.mean.shape != (self.d,)) or (self.thresh is not None and self.thresh.shape != (self.bits,)):
            raise ValueError(f"SketchProjection: mean {getattr(self.mean, 'shape', None)} and thresh "
                             f"{getattr(self.thresh, 'shape', None)} do not fit basis {self.basis.shape}: [d], [bits]")

    @property
    def bits(self) -> int:
        return int(self.basis.shape[0])

    @property
    def d(self) -> int:
        return int(self.basis.shape[1])

    @classmethod
    def random(cls, d: int, bits: int, seed: int, mean=None) -> "SketchProjection":
        """Gaussian hyperplanes: `np.random.RandomState(seed).randn(bits, d)` as float32, a function of (d, bits, seed)."""
        d, bits = int(d), int(bits)
        if d < 1 or bits < 1:
            raise ValueError(f"SketchProjection.random: d {d} and bits {bits} must be positive")
        return cls(np.random.RandomState(seed).randn(bits, d).astype(np.float32), mean=mean)

    @classmethod
    def from_pca(cls, pca: PcaProjection, bits=None) -> "SketchProjection":
        """The `bits` leading components of a fitted `PcaProjection` (default: all of them) and its mean."""
        bits = pca.m if bits is None else int(bits)
        if bits < 1 or bits > pca.m:
            raise ValueError(f"SketchProjection.from_pca: bits {bits} outside [1, pca.m = {pca.m}]")
        return cls(pca.basis[:bits], mean=pca.mean)

    def encode(self, x, device: int = 0):
        """uint8 [n, bits // 8]: numpy for a numpy `x`, a tensor on x's device for a device tensor (`_capi.sketch`)."""
        return _capi.sketch(x, self.basis, mean=self.mean, thresh=self.thresh, device=device)

    def save(self, path) -> None:
        given = {k: v for k, v in (("mean", self.mean), ("thresh", self.thresh)) if v is not None}
        np.savez(path, basis=self.basis, **given)

    @classmethod
    def load(cls, path) -> "SketchProjection":
        with np.load(path) as z:
            return cls(z["basis"], z["mean"] if "mean" in z else None, z["thresh"] if "thresh" in z else None)
