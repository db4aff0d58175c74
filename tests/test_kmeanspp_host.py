"""CPU (`-m "not gpu"`): `hip_kmeans.cluster` routes `init` and `n_trials` to `_capi.kmeans` and rejects what it does not know --
against a recording stand-in; no library is loaded."""
import numpy as np
import pytest


@pytest.fixture
def seen(monkeypatch):
    from learnedmetricindex_amd import _capi

    calls = []

    def fake(x, k, niter=20, seed=2023, **seeding):
        calls.append(dict(niter=niter, seed=seed, **seeding))
        return np.zeros((k, x.shape[1]), np.float32), np.zeros(x.shape[0], np.int32), np.zeros(k, np.int64), np.zeros(niter + 1, np.int64)

    monkeypatch.setattr(_capi, "kmeans", fake)
    return calls


@pytest.mark.parametrize("params,want", [
    (None, dict(niter=20, seed=2023)),
    ({"init": "random", "n_trials": 5}, dict(niter=20, seed=2023)),
    ({"init": "k-means++", "seed": 7}, dict(niter=20, seed=7, init="k-means++", n_trials=0)),
    ({"init": "k-means++", "n_trials": 4, "niter": 3}, dict(niter=3, seed=2023, init="k-means++", n_trials=4)),
    ({"n_init": 3}, r"unknown parameters \['n_init'\] \(seed, niter, init, n_trials\)"),
    ({"init": "kmeans||"}, r"init 'kmeans\|\|' must be"),
])
def test_cluster_routes_the_seeding_and_rejects_the_rest(seen, params, want):
    from learnedmetricindex_amd.li.clustering import algorithms

    if isinstance(want, str):
        with pytest.raises(ValueError, match=want):
            algorithms["hip_kmeans"](np.zeros((12, 6), np.float32), 3, params)
        assert seen == []
    else:
        algorithms["hip_kmeans"](np.zeros((12, 6), np.float32), 3, params)
        assert seen == [want]
