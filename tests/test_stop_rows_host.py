"""CPU (`-m "not gpu"`): the row-budget stop's interface and its definition.

The header declares `lmi_set_stop_rows`, the library exports it, the binding and the Python layers expose it; and the numpy
restatement of the rule (tests/stop_rows_ref.py, on top of the unchanged oracle) reproduces the visited-count histograms recorded
when the feature was specified -- which pins the definition and the non-vacuity of every parity case of test_gpu_stop_rows.py.
Sizes are the fixtures' own (`data_prediction`)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import path_mass_ref
import stop_mass_ref
from helpers import inputs_for, layers_from, load_golden
from stop_rows_ref import (assert_not_vacuous, count_histogram, cut, expected_order, expected_walk, sizes_of_classes, sizes_of_paths,
                           visited_mask)
from test_oracle_multilevel import internal_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: 1-level parity cases: (fixture, n_buckets, rows) -> histogram of visited counts
ONE_LEVEL = {("G1", 4, 1079): [0, 65, 53, 82], ("G1", 8, 2526): [0, 0, 0, 0, 1, 85, 77, 37], ("G5", 4, 238): [0, 14, 106, 80],
             ("G5", 8, 498): [0, 0, 0, 4, 26, 63, 69, 38], ("G3", 4, 400): [3, 55, 101, 97]}
#: the wide model (1 024 classes; test_gpu_stop_mass.wide_model) over WIDE_N objects with seeded uniform labels
WIDE_N, WIDE_SEED, WIDE_NB, WIDE_ROWS, WIDE_HIST = 6000, 23, 4, 16, [0, 24, 181, 95]
#: walk parity cases on the fixtures
WALK_FIXTURES = {("G2", 4, 1554): [0, 94, 54, 52], ("G7", 6, 478): [0, 10, 31, 54, 42, 63], ("G8", 6, 1352): [0, 0, 23, 35, 91, 51]}
#: walk parity cases on path_mass_ref.synthetic_tree, n_buckets 7.  (20, 3): at 366 only 8 % of the queries are uncut; 400: 40 %
SYNTH_NB = 7
WALK_SYNTH = {((20, 3), 400): [0, 0, 0, 2, 3, 175, 120], ((12, 12), 152): [0, 0, 0, 0, 46, 215, 39], ((5, 4), 1035): [0, 0, 3, 24, 41, 133, 99]}
#: both stops: (G1, n_buckets 4, mass 0.999, rows 1079) and the synthetic (5, 4) tree at mass 0.999, rows 1035
COMBINED_G1 = ("G1", 4, 0.999, 1079, [65, 64, 33, 38])
COMBINED_SYNTH = ((5, 4), 0.999, 1035, [17, 52, 48, 60, 44, 55, 24])


def wide_labels():
    return np.random.RandomState(WIDE_SEED).randint(0, 1024, WIDE_N).astype(np.int64)


def test_header_declares_and_binding_exposes():
    from learnedmetricindex_amd import _capi

    text = open(os.path.join(ROOT, "include", "lmi_hip.h")).read()
    assert re.search(r"LMI_API\s+int\s+lmi_set_stop_rows\s*\(\s*lmi_index\s*\*\s*h\s*,\s*int64_t\s+rows\s*\)\s*;", text)
    assert _capi.SIGNATURES["lmi_set_stop_rows"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64])
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "lmi_set_stop_rows")
    assert callable(_capi.Index.set_stop_rows)
    src = inspect.getsource(_capi.Index._configure)
    assert re.search(r"self\.stop_rows\s*=\s*0\b", src)
    assert '"stop_rows"' in inspect.getsource(_capi.Index._derived)


def test_python_layers_take_stop_rows():
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex
    from learnedmetricindex_amd.pipeline import HostPipeline
    from learnedmetricindex_amd.sharded import ReplicaSearcher, ShardedSearcher

    for fn in (LearnedIndex.search, LearnedIndex.search_resident, HostPipeline.__init__, ShardedSearcher.__init__, ReplicaSearcher.__init__):
        assert inspect.signature(fn).parameters["stop_rows"].default is None, fn

    class Untouched:   # stands in for an Index: the refusal comes before anything is read or set
        def __getattr__(self, name):
            raise AssertionError(f"ShardedSearcher touched index.{name} before refusing")

    for world in (2, 8):
        with pytest.raises(ValueError, match="stop_rows"):
            ShardedSearcher(Untouched(), 0, world, stop_rows=100)
    li = LearnedIndex(None, {}, [])
    with pytest.raises(ValueError, match="multi-level"):   # stop_mass on a tree and path_mass on a 1-level index stay refused
        li.search_resident(None, None, [4, 3], 2, 10, stop_mass=0.9, stop_rows=100)
    with pytest.raises(ValueError, match="stop_mass"):
        li.search_resident(None, None, [12], 2, 10, path_mass=0.9, stop_rows=100)


def test_driver_flag():
    from learnedmetricindex_amd.search import Experiment

    assert Experiment.from_argv(["--n-categories", "12"]).stop_rows is None
    assert Experiment.from_argv(["--n-categories", "12", "--stop-rows", "5000"]).stop_rows == 5000
    e = Experiment.from_argv(["--n-categories", "4", "3", "--stop-rows", "1"])     # any number of levels
    assert e.stop_rows == 1 and e.n_categories == [4, 3]
    e = Experiment.from_argv(["--n-categories", "12", "--stop-rows", "7", "--stop-mass", "0.9"])
    assert (e.stop_rows, e.stop_mass) == (7, 0.9)
    for bad in (["--n-categories", "12", "--stop-rows", "0"], ["--n-categories", "12", "--stop-rows", "-3"],
                ["--n-categories", "12", "--stop-rows", "1.5"], ["--n-categories", "12", "--stop-rows", "many"],
                ["--n-categories", "4", "3", "--stop-rows", "10", "--stop-mass", "0.9"],
                ["--n-categories", "12", "--stop-rows", "10", "--path-mass", "0.9"]):
        with pytest.raises(SystemExit):
            Experiment.from_argv(bad)


def test_rule_on_hand_made_sizes():
    sizes = np.array([10, 0, 5, 7, 100], dtype=np.int64)
    order = np.array([[0, 1, 2, 3],      # r = 10 10 15 22
                      [4, 0, 1, 2],      # r = 100 ..: the first bucket alone passes every budget below
                      [1, 1, 1, 1],      # zero-size buckets: r stays 0, never cut
                      [2, -1, 3, 0],     # a rank without a class adds 0: r = 5 5 12 22
                      [3, 2, -1, -1]])   # r = 7 12 12 12
    n = sizes_of_classes(order, sizes)
    assert n.tolist() == [[10, 0, 5, 7], [100, 10, 0, 5], [0, 0, 0, 0], [5, 0, 7, 10], [7, 5, 0, 0]]
    T, F = True, False
    assert visited_mask(n, 11).tolist() == [[T, T, T, F], [T, F, F, F], [T, T, T, T], [T, T, T, F], [T, T, F, F]]
    # a budget equal to a prefix sum: `r < rows` is false, the query stops there
    assert visited_mask(n, 10).tolist()[0] == [T, F, F, F]
    assert visited_mask(n, 15).tolist()[0] == [T, T, T, F]
    assert visited_mask(n, 16).tolist()[0] == [T, T, T, T]
    assert visited_mask(n, 12).tolist()[3:] == [[T, T, T, F], [T, T, F, F]]
    assert visited_mask(n, 13).tolist()[3:] == [[T, T, T, T], [T, T, T, T]]
    assert visited_mask(n, 1).tolist() == [[T, F, F, F], [T, F, F, F], [T, T, T, T], [T, F, F, F], [T, F, F, F]]
    assert visited_mask(n, np.iinfo(np.int64).max).all()           # the largest budget cuts nothing
    assert visited_mask(n[:, :1], 1).all()                          # n_buckets 1 is never cut
    big = np.full((1, 4), 2 ** 31 - 1, dtype=np.int64)              # the sum is int64: four buckets of 2^31 - 1 do not wrap
    assert visited_mask(big, 2 ** 33).tolist() == [[T, T, T, T]] and visited_mask(big, 2 ** 32).tolist() == [[T, T, T, F]]
    o3 = np.arange(24, dtype=np.int32).reshape(2, 4, 3)
    c = cut(o3, [1, 4])
    assert (c[0, 1:] == -1).all() and np.array_equal(c[0, 0], o3[0, 0]) and np.array_equal(c[1], o3[1])


def one_level(name):
    if name == "wide1024":
        from test_gpu_stop_mass import wide_model

        layers, Qn = wide_model()
        return layers, Qn, np.bincount(wide_labels(), minlength=1024)
    g = load_golden(name)
    _, Qn, _, _ = inputs_for(name, g)
    layers = layers_from(g)
    return layers, Qn, np.bincount(g["data_prediction"][:, 0], minlength=layers[-1][0].shape[0])


@pytest.mark.parametrize("name,nb,rows,hist", [k + (v,) for k, v in ONE_LEVEL.items()] + [("wide1024", WIDE_NB, WIDE_ROWS, WIDE_HIST)])
def test_recorded_histograms(oracle, name, nb, rows, hist):
    layers, Qn, sizes = one_level(name)
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes, rows)
    print(f"{name} nb {nb} rows {rows}: {count_histogram(counts, nb)}, empty buckets {(sizes == 0).sum()}")
    assert count_histogram(counts, nb) == hist
    assert_not_vacuous(counts, nb)
    full = oracle.precompute_bucket_order(layers, Qn, nb)
    kept = bo >= 0
    assert np.array_equal(bo[kept], full[kept]) and kept[:, 0].all()
    assert np.array_equal(kept[:, :, 0].sum(axis=1), counts)
    assert (np.diff(kept[:, :, 0].astype(int), axis=1) <= 0).all()   # once cut, cut for good
    n = sizes_of_classes(full[:, :, 0], sizes)
    for q in range(n.shape[0]):                                       # all visited ranks but the last stay under the budget
        assert n[q, :counts[q] - 1].sum() < rows and (counts[q] == nb or n[q, :counts[q]].sum() >= rows)
    if name == "G3":   # zero-size buckets inside a visited prefix
        assert (sizes == 0).sum() == 10
        assert ((n == 0) & kept[:, :, 0]).any()


_trees = {}


def walk_case(oracle, key):
    """(the uncut walk's order, data_prediction, path_mass_ref.Tree) of a fixture name or a synthetic tree's n_categories."""
    if key not in _trees:
        if isinstance(key[0], str):
            name, nb = key
            g = load_golden(name)
            _, Qn, _, _ = inputs_for(name, g)
            ncat = [int(v) for v in g["n_categories"]]
            bucket_paths = [tuple(int(v) for v in p) for p in g["bucket_paths"]]
            full = oracle.precompute_bucket_order_multilevel(layers_from(g), internal_of(g), bucket_paths, Qn, nb, ncat)
            tree = path_mass_ref.Tree(oracle, layers_from(g), internal_of(g), bucket_paths, Qn, ncat)
            dp = g["data_prediction"]
        else:
            ncat, nb = key
            root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = path_mass_ref.synthetic_tree(list(ncat))
            full = oracle.precompute_bucket_order_multilevel(root, internal, bucket_paths, Qn, nb, list(ncat))
            tree = path_mass_ref.Tree(oracle, root, internal, bucket_paths, Qn, list(ncat))
        assert np.array_equal(path_mass_ref.walk(tree, nb, 0.0)[0], full)   # the two statements of the uncut walk agree
        _trees[key] = (full, dp, tree)
    return _trees[key]


@pytest.mark.parametrize("name,nb,rows,hist", [k + (v,) for k, v in WALK_FIXTURES.items()])
def test_recorded_histograms_walk_fixtures(oracle, name, nb, rows, hist):
    full, dp, _ = walk_case(oracle, (name, nb))
    bo, counts = expected_walk(full, dp, rows)
    print(f"{name} nb {nb} rows {rows}: {count_histogram(counts, nb)}")
    assert count_histogram(counts, nb) == hist
    assert_not_vacuous(counts, nb)
    for q in range(bo.shape[0]):
        assert (bo[q, counts[q]:] == -1).all() and np.array_equal(bo[q, :counts[q]], full[q, :counts[q]])


@pytest.mark.parametrize("ncat,rows,hist", [k + (v,) for k, v in WALK_SYNTH.items()])
def test_recorded_histograms_walk_synthetic(oracle, ncat, rows, hist):
    full, dp, _ = walk_case(oracle, (ncat, SYNTH_NB))
    bo, counts = expected_walk(full, dp, rows)
    n = sizes_of_paths(full, dp)
    inside = ((n == 0) & (np.arange(SYNTH_NB)[None, :] < counts[:, None])).any(axis=1).sum()
    print(f"{list(ncat)} rows {rows}: {count_histogram(counts, SYNTH_NB)}, queries with a listed-empty bucket in their visited prefix {inside}")
    assert count_histogram(counts, SYNTH_NB) == hist
    assert_not_vacuous(counts, SYNTH_NB)
    assert inside > 0
    if ncat == (5, 4):
        assert inside == 164
    if ncat == (20, 3):   # why this case does not run at 366
        c366 = expected_walk(full, dp, 366)[1]
        assert abs((c366 == SYNTH_NB).mean() - 0.08) < 1e-9


def test_recorded_histograms_combined(oracle):
    """Both stops: the visited count is the smaller of the two, and each stop binds alone for at least 10 % of the queries."""
    name, nb, mass, rows, hist = COMBINED_G1
    layers, Qn, sizes = one_level(name)
    cr = expected_order(oracle, layers, Qn, nb, sizes, rows)[1]
    cm = stop_mass_ref.expected_order(oracle, layers, Qn, nb, mass)[1]
    bo, cb = expected_order(oracle, layers, Qn, nb, sizes, rows, mass=mass)
    assert np.array_equal(cb, np.minimum(cr, cm)) and count_histogram(cb, nb) == hist
    assert ((cm < cr).sum(), (cr < cm).sum(), ((cm == nb) & (cr == nb)).sum()) == (109, 30, 38)
    assert min((cm < cr).mean(), (cr < cm).mean()) >= 0.10
    assert np.array_equal((bo[:, :, 0] >= 0).sum(axis=1), cb)
    ncat, mass, rows, hist = COMBINED_SYNTH
    full, dp, tree = walk_case(oracle, (ncat, SYNTH_NB))
    bo_m, cm = path_mass_ref.walk(tree, SYNTH_NB, mass)
    cr = expected_walk(full, dp, rows)[1]
    bo, cb = expected_walk(full, dp, rows, mass_counts=cm)
    assert np.array_equal(cb, np.minimum(cr, cm)) and count_histogram(cb, SYNTH_NB) == hist
    assert ((cm < cr).sum(), (cr < cm).sum()) == (201, 55)
    assert min((cm < cr).mean(), (cr < cm).mean()) >= 0.10
    only_mass = cm <= cr
    assert np.array_equal(bo[only_mass], bo_m[only_mass])   # where the mass binds, the order is the mass walk's
