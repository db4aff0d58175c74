"""k-means on the MI355X (`lmi_kmeans`): Lloyd's algorithm in HIP, deterministic -- the same data, seed and iteration count give
the same centroids and labels bit for bit (include/lmi_hip.h states the arithmetic).  faiss's defaults: 20 iterations, random initial
centroids from the data, seed 2023 (reference: li/clustering/faiss_kmeans.py:8-24).  A float16 array stays float16
(`lmi_kmeans_f16`): half the upload, the result that of the widened array.  There is no fallback: without the library or the device
the call raises."""
from typing import Any, Dict, Optional

import numpy as np


class HipKmeans:
    """What `cluster` returns beside the labels: `centroids` f32[k,d], `counts` i64[k] (objects per cluster), `changed`
    i64[niter+1] (labels that moved per pass; zeros behind a fixed point)."""

    def __init__(self, centroids, counts, changed):
        self.centroids, self.counts, self.changed = centroids, counts, changed


def cluster(data, n_clusters: int, parameters: Optional[Dict[str, Any]]):
    params = {} if parameters is None else dict(parameters)
    seed, niter = int(params.pop("seed", 2023)), int(params.pop("niter", 20))
    params.pop("verbose", None)
    if params:
        raise ValueError(f"hip_kmeans: unknown parameters {sorted(params)} (seed, niter)")
    try:
        from ... import _capi   # the package
    except ImportError:
        import _capi            # `li` on sys.path next to _capi.py (search.py's layout)
    if not isinstance(data, np.ndarray):
        data = np.asarray(data)
    # a float16 array is passed on as it is (lmi_kmeans_f16: resident as halves, the result that of the widened array)
    data = np.ascontiguousarray(data, dtype=np.float16 if data.dtype == np.float16 else np.float32)
    centroids, labels, counts, changed = _capi.kmeans(data, n_clusters, niter=niter, seed=seed)
    return HipKmeans(centroids, counts, changed), labels
