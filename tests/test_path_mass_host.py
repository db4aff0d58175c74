"""CPU: the numpy restatement of the path-mass stop (tests/path_mass_ref.py) against the unchanged oracle, and the non-vacuity
of every parity case test_gpu_path_mass.py uses."""
import numpy as np
import pytest

from helpers import inputs_for, layers_from, load_golden
from path_mass_ref import Tree, assert_not_vacuous, count_histogram, synthetic_tree, walk
from test_oracle_multilevel import internal_of

#: the parity cases of the GPU tests: (fixture, mass); n_buckets is the fixture's own
FIXTURE_CASES = [("G2", 0.99), ("G7", 0.8), ("G7", 0.9), ("G8", 0.9)]
#: (tree, mass) at 300 queries, n_buckets 7
SYNTH_CASES = [((20, 3), 0.99), ((12, 12), 0.99), ((5, 4), 0.999)]
SYNTH_NB = 7

#: visited-count histograms over the fixtures' 200 queries ([queries visiting 1, 2, ..] buckets)
PINNED_HISTOGRAMS = {("G2", 0.99): [52, 43, 105], ("G7", 0.8): [32, 33, 20, 15, 14, 9, 6, 7, 8, 56], ("G8", 0.9): [79, 37, 29, 20, 35]}

_trees = {}


def fixture_tree(oracle, name):
    if name not in _trees:
        g = load_golden(name)
        _, Qn, _, _ = inputs_for(name, g)
        ncat = [int(v) for v in g["n_categories"]]
        bucket_paths = [tuple(int(v) for v in p) for p in g["bucket_paths"]]
        _trees[name] = (g, Tree(oracle, layers_from(g), internal_of(g), bucket_paths, Qn, ncat), int(g["n_buckets"]), ncat, bucket_paths)
    return _trees[name]


def synth_tree(oracle, ncat):
    key = tuple(ncat)
    if key not in _trees:
        root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree(list(ncat))
        _trees[key] = Tree(oracle, root, internal, bucket_paths, Qn, list(ncat))
    return _trees[key]


@pytest.mark.parametrize("name", ["G2", "G7", "G8"])
def test_mass_zero_is_the_oracles_walk(oracle, name):
    g, tree, nb, ncat, bucket_paths = fixture_tree(oracle, name)
    bo, counts = walk(tree, nb, 0.0)
    ref = oracle.precompute_bucket_order_multilevel(layers_from(g), internal_of(g), bucket_paths, tree.Q, nb, ncat)
    assert np.array_equal(bo, ref)
    assert (counts == nb).all()


@pytest.mark.parametrize("ncat", [(20, 3), (12, 12), (5, 4)])
def test_mass_zero_is_the_oracles_walk_synthetic(oracle, ncat):
    root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs = synthetic_tree(list(ncat))
    bo, counts = walk(synth_tree(oracle, ncat), SYNTH_NB, 0.0)
    ref = oracle.precompute_bucket_order_multilevel(root, internal, bucket_paths, Qn, SYNTH_NB, list(ncat))
    assert np.array_equal(bo, ref)
    assert (counts == SYNTH_NB).all()


@pytest.mark.parametrize("name", ["G2", "G7", "G8"])
def test_counts_grow_with_the_mass(oracle, name):
    g, tree, nb, ncat, _ = fixture_tree(oracle, name)
    prev, prev_bo = None, None
    for mass in (1e-30, 0.5, 0.8, 0.9, 0.99, 0.999, 1.0):
        bo, counts = walk(tree, nb, mass)
        assert counts.min() >= 1 and counts.max() <= nb
        if mass == 1e-30:
            assert (counts == 1).all()
        for q in range(bo.shape[0]):                     # slots behind the stop are EMPTY_VALUE
            assert (bo[q, counts[q]:] == -1).all()
        if prev is not None:
            assert (counts >= prev).all()
            for q in range(bo.shape[0]):                 # a larger mass extends the same order
                assert np.array_equal(bo[q, :prev[q]], prev_bo[q, :prev[q]])
        prev, prev_bo = counts, bo


@pytest.mark.parametrize("name,mass", FIXTURE_CASES)
def test_fixture_cases_are_not_vacuous(oracle, name, mass):
    g, tree, nb, ncat, _ = fixture_tree(oracle, name)
    _, counts = walk(tree, nb, mass)
    hist = count_histogram(counts, nb)
    print(f"{name} {ncat} nb {nb} mass {mass}: {hist}, cut {(counts < nb).mean():.0%}")
    assert_not_vacuous(counts, nb)
    if (name, mass) in PINNED_HISTOGRAMS:
        assert hist == PINNED_HISTOGRAMS[(name, mass)]


@pytest.mark.parametrize("ncat,mass", SYNTH_CASES)
def test_synthetic_cases_are_not_vacuous(oracle, ncat, mass):
    _, counts = walk(synth_tree(oracle, ncat), SYNTH_NB, mass)
    print(f"{list(ncat)} nb {SYNTH_NB} mass {mass}: {count_histogram(counts, SYNTH_NB)}, cut {(counts < SYNTH_NB).mean():.0%}")
    assert_not_vacuous(counts, SYNTH_NB)


def test_the_vacuous_cases_stay_out(oracle):
    """G7 at 0.99 cuts nobody; G2 and G8 at 0.5 cut everybody: none of them is a parity case."""
    g, tree, nb, _, _ = fixture_tree(oracle, "G7")
    assert (walk(tree, nb, 0.99)[1] == nb).all()
    for name in ("G2", "G8"):
        g, tree, nb, _, _ = fixture_tree(oracle, name)
        assert (walk(tree, nb, 0.5)[1] < nb).all()
