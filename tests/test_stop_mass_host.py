"""CPU (`-m "not gpu"`): the probability-mass stop's interface and its definition.

The header declares `lmi_set_stop_mass`, the library exports it and the binding exposes it; and the numpy restatement of the
rule (tests/stop_mass_ref.py, on top of the unchanged oracle) reproduces the visited-rank histograms recorded when the
feature was specified -- which pins the definition the GPU tests compare against: the probabilities are predict_proba's,
the running sum is binary32 in rank order, rank t >= 1 is visited iff the sum of the ranks before it is below the mass."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from helpers import inputs_for, layers_from, load_golden
from stop_mass_ref import assert_not_vacuous, count_histogram, expected_order, visited_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_exposes():
    from learnedmetricindex_amd import _capi

    text = open(os.path.join(ROOT, "include", "lmi_hip.h")).read()
    assert re.search(r"LMI_API\s+int\s+lmi_set_stop_mass\s*\(\s*lmi_index\s*\*\s*h\s*,\s*float\s+mass\s*\)\s*;", text)
    assert re.search(r"#define\s+LMI_ABI_VERSION\s+1\b", text)
    assert _capi.SIGNATURES["lmi_set_stop_mass"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_float])
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "lmi_set_stop_mass")
    assert callable(_capi.Index.set_stop_mass)


def test_python_layers_take_stop_mass():
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from learnedmetricindex_amd.pipeline import HostPipeline
    from learnedmetricindex_amd.sharded import ReplicaSearcher, ShardedSearcher

    for fn in (LearnedIndex.search, LearnedIndex.search_resident, HostPipeline.__init__, ShardedSearcher.__init__, ReplicaSearcher.__init__):
        assert inspect.signature(fn).parameters["stop_mass"].default is None, fn
    li = LearnedIndex(None, {}, [])
    with pytest.raises(ValueError, match="multi-level"):   # refused before anything else is looked at
        li.search(None, None, None, None, None, [4, 3], 2, 10, stop_mass=0.9)
    with pytest.raises(ValueError, match="multi-level"):
        li.search_resident(None, None, [4, 3], 2, 10, stop_mass=0.9)


def test_driver_flag():
    from learnedmetricindex_amd.search import Experiment

    assert Experiment.from_argv(["--n-categories", "12"]).stop_mass is None
    assert Experiment.from_argv(["--n-categories", "12", "--stop-mass", "0.99"]).stop_mass == 0.99
    for bad in (["--n-categories", "4", "3", "--stop-mass", "0.9"], ["--n-categories", "12", "--stop-mass", "1.5"],
                ["--n-categories", "12", "--stop-mass", "0"]):
        with pytest.raises(SystemExit):
            Experiment.from_argv(bad)


def test_rule_on_hand_made_probabilities():
    p = np.array([[0.5, 0.25, 0.125, 0.125],        # c = .5 .75 .875: mass .75 stops after two ranks (c_1 < .75 is false)
                  [0.9, 0.05, 0.03, 0.02],
                  [np.nan, np.nan, np.nan, np.nan],   # NaN: the compare is false, rank 0 alone
                  [0.25, 0.25, 0.25, 0.25]], dtype=np.float32)
    assert visited_mask(p, 4, 0.75).tolist() == [[True, True, False, False], [True, False, False, False],
                                                 [True, False, False, False], [True, True, True, False]]
    assert visited_mask(p, 4, 1.0).tolist()[3] == [True, True, True, True]
    assert visited_mask(p, 1, 0.5).all()
    # the running sum is binary32: 2^-25 is lost against 1 - 2^-24 + .. only in float32
    q = np.array([[1.0 - 2.0 ** -24, 2.0 ** -26, 2.0 ** -26, 0.0]], dtype=np.float32)
    assert visited_mask(q, 4, 1.0).tolist() == [[True, True, True, True]]   # a float64 sum would reach 1 - 2^-25 too: still below 1
    r = np.array([[0.5, 2.0 ** -26, 2.0 ** -26, 0.0]], dtype=np.float32)
    m = np.float32(0.5) + np.float32(2.0 ** -24)                            # the float32 after 0.5
    assert visited_mask(r, 4, 0.5).tolist() == [[True, False, False, False]]
    assert visited_mask(r, 4, m).tolist() == [[True, True, True, True]]     # each 2^-26 is rounded away: the sum stays 0.5


@pytest.mark.parametrize("name,mass,hist", [("G1", 0.999, [65, 46, 33, 56]), ("G5", 0.99, [121, 21, 12, 46])])
def test_recorded_histograms(oracle, name, mass, hist):
    g = load_golden(name)
    _, Qn, _, _ = inputs_for(name, g)
    layers = layers_from(g)
    bo, counts = expected_order(oracle, layers, Qn, 4, mass)
    assert count_histogram(counts, 4) == hist
    assert_not_vacuous(counts, 4)
    full = oracle.precompute_bucket_order(layers, Qn, 4)
    kept = bo >= 0
    assert np.array_equal(bo[kept], full[kept]) and kept[:, 0].all()
    assert np.array_equal(kept[:, :, 0].sum(axis=1), counts)
    assert (np.diff(kept[:, :, 0].astype(int), axis=1) <= 0).all()   # once cut, cut for good
