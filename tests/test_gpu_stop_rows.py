"""GPU (`-m gpu`): the row-budget stop (lmi_set_stop_rows) -- a query visits buckets in the model's order until the buckets it has
visited hold `rows` objects or more; the ranks behind the stop are -1 and the scan skips them.  One setting for the 1-level bucket
order and for the multi-level walk, alone and together with lmi_set_stop_mass / lmi_set_path_mass.

Every comparison is exact.  The expected order is the unchanged oracle's, cut by tests/stop_rows_ref.py; expected results come from
`oracle.search(..., bucket_order=cut order)`.  Every parity case first asserts that its inputs exercise the cut (assert_not_vacuous);
the cases, their budgets and their histograms are pinned on the CPU by test_stop_rows_host.py.

Ranking paths of the 1-level order (lmi_set_fused_mlp 0 / 1 / 2): per-layer kernels + rank_classes_rows_kernel, the fused kernel's
FM_TOPK_ROWS epilogue, and the ranking kernel behind a fused launch whose 1 024 logits went through global memory (wide1024 under 2).
Launch forms of the walk: (20, 3) steps in batches with the count read back; (12, 12) the global-memory pop kernel; (5, 4) and the
fixtures everything up front, queues in LDS."""
import numpy as np
import pytest
import torch

import stop_mass_ref
from helpers import inputs_for, layers_from, load_golden
from stop_rows_ref import assert_not_vacuous, expected_order, expected_walk, sizes_of_classes
from test_gpu_path_mass import Case, frame, net_from
from test_stop_rows_host import (COMBINED_G1, COMBINED_SYNTH, ONE_LEVEL, SYNTH_NB, WALK_FIXTURES, WALK_SYNTH, WIDE_NB, WIDE_ROWS, one_level,
                                 wide_labels)

pytestmark = pytest.mark.gpu

MODEL_OF = {"G1": "MLP", "G5": "MLP-4"}
INT64_MAX = int(np.iinfo(np.int64).max)


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def built(capi, layers, Xs, labels, **kw):
    idx = capi.Index(0, **kw)
    idx.set_mlp(layers)
    idx.set_buckets(Xs, labels, layers[-1][0].shape[0])
    return idx


_one = {}


def search_case(name):
    """(layers, Qn, Xs, Qs, data_prediction, sizes) of a 1-level fixture -- or of the wide model over seeded objects."""
    if name not in _one:
        layers, Qn, sizes = one_level(name)
        if name == "wide1024":
            rs = np.random.RandomState(5)
            lab = wide_labels()
            Xs, Qs = rs.randn(lab.shape[0], 8).astype(np.float32), rs.randn(Qn.shape[0], 8).astype(np.float32)
            _one[name] = (layers, Qn, Xs, Qs, lab[:, None], sizes)
        else:
            g = load_golden(name)
            _, _, Xs, Qs = inputs_for(name, g)
            _one[name] = (layers, Qn, Xs, Qs, g["data_prediction"], sizes)
    return _one[name]


_idx = {}


@pytest.fixture(scope="module")
def index_of(capi):
    """One built index per 1-level case for the order tests (they only change settings and put them back)."""
    def get(name):
        if name not in _idx:
            layers, Qn, Xs, Qs, dp, sizes = search_case(name)
            _idx[name] = built(capi, layers, Xs, dp[:, 0])
            assert np.array_equal(_idx[name].bucket_sizes(), sizes)
        return _idx[name]
    yield get
    for h in _idx.values():
        h.close()
    _idx.clear()


ORDER_CASES = list(ONE_LEVEL) + [("wide1024", WIDE_NB, WIDE_ROWS)]


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("name,nb,rows", ORDER_CASES)
def test_order_parity(index_of, oracle, name, nb, rows, fused):
    """1. lmi_mlp_topk on a built index equals the oracle's order cut by the cumulative sizes, on each of the three ranking paths;
    G3 has zero-size buckets inside visited prefixes."""
    layers, Qn, Xs, Qs, dp, sizes = search_case(name)
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes, rows)
    assert_not_vacuous(counts, nb)
    idx = index_of(name)
    idx.set_fused_mlp(fused)
    idx.set_stop_rows(rows)
    try:
        got = idx.mlp_topk(Qn, nb)
    finally:
        idx.set_stop_rows(0)
        idx.set_fused_mlp(1)
    print(f"{name} rows {rows} nb {nb} fused {fused}: rows differing {(got != bo[:, :, 0]).any(axis=1).sum()} of {Qn.shape[0]}")
    assert np.array_equal(got, bo[:, :, 0])


def test_order_parity_split_batch(index_of, oracle):
    """2. A batch of 313 32-query blocks under the default mode: the fused kernel takes one full round of blocks and the per-layer
    kernels the rest on a side stream -- both halves must cut alike."""
    layers, Qn, Xs, Qs, dp, sizes = search_case("G1")
    rs = np.random.RandomState(11)
    scale = rs.uniform(0.5, 1.0, size=(10000, 1)).astype(np.float32)
    Q = np.ascontiguousarray(Qn[rs.randint(Qn.shape[0], size=10000)] * scale)
    bo, counts = expected_order(oracle, layers, Q, 4, sizes, 1079)
    assert_not_vacuous(counts, 4)
    idx = index_of("G1")
    idx.set_stop_rows(1079)
    try:
        got = idx.mlp_topk(Q, 4)
    finally:
        idx.set_stop_rows(0)
    assert np.array_equal(got, bo[:, :, 0])


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("prefilter", [True, False])
@pytest.mark.parametrize("name,nb,rows", [("G1", 4, 1079), ("G5", 4, 238)])
def test_search_parity(capi, oracle, name, nb, rows, prefilter, metric):
    """3. lmi_search: dists, ids and the returned bucket order equal the oracle's search over the cut order."""
    layers, Qn, Xs, Qs, dp, sizes = search_case(name)
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes, rows)
    assert_not_vacuous(counts, nb)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo, metric=metric)
    idx = built(capi, layers, Xs, dp[:, 0], prefilter=prefilter, metric=metric)
    idx.set_stop_rows(rows)
    d, i, got_bo = idx.search(Qn, Qs, nb, 10)
    idx.close()
    assert np.array_equal(got_bo, bo[:, :, 0])
    assert np.array_equal(i, no)
    assert np.array_equal(d.astype(np.float64), do)


@pytest.mark.parametrize("name,nb,rows", [("G1", 4, 1079), ("G5", 4, 238)])
def test_work_is_skipped(capi, oracle, name, nb, rows):
    """4. lmi_scan_stats' pairs is the sum of the bucket sizes over the kept slots, strictly below the uncut run's; and for every
    query the sizes of its visited ranks but the last sum to less than the budget."""
    layers, Qn, Xs, Qs, dp, sizes = search_case(name)
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes, rows)
    assert_not_vacuous(counts, nb)
    full = oracle.precompute_bucket_order(layers, Qn, nb)[:, :, 0]
    kept = bo[:, :, 0]
    idx = built(capi, layers, Xs, dp[:, 0])
    idx.search(Qn, Qs, nb, 10)
    pairs_off = idx.scan_stats()[1]
    idx.set_stop_rows(rows)
    got = idx.search(Qn, Qs, nb, 10)[2]
    pairs_on = idx.scan_stats()[1]
    live = idx.bucket_sizes()
    idx.close()
    print(f"{name}: pairs {pairs_on} with the stop, {pairs_off} without")
    assert pairs_off == int(sizes[full].sum())
    assert pairs_on == int(sizes[kept[kept >= 0]].sum())
    assert pairs_on < pairs_off
    n = sizes_of_classes(got, live)
    for q in range(got.shape[0]):
        v = int((got[q] >= 0).sum())
        assert v >= 1 and (got[q, v:] == -1).all()
        assert n[q, :v - 1].sum() < rows
        assert v == nb or n[q, :v].sum() >= rows


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_combined_with_stop_mass(index_of, capi, oracle, fused):
    """5. Both stops on a 1-level call: a query goes on only while both conditions hold (each binds alone for >= 10 % of the queries)."""
    name, nb, mass, rows, _ = COMBINED_G1
    layers, Qn, Xs, Qs, dp, sizes = search_case(name)
    cr = expected_order(oracle, layers, Qn, nb, sizes, rows)[1]
    cm = stop_mass_ref.expected_order(oracle, layers, Qn, nb, mass)[1]
    assert min((cm < cr).mean(), (cr < cm).mean()) >= 0.10
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes, rows, mass=mass)
    assert np.array_equal(counts, np.minimum(cm, cr))
    idx = index_of(name)
    idx.set_fused_mlp(fused)
    idx.set_stop_rows(rows)
    idx.set_stop_mass(mass)
    try:
        got = idx.mlp_topk(Qn, nb)
        d, i, got_bo = idx.search(Qn, Qs, nb, 10)
    finally:
        idx.set_stop_rows(0)
        idx.set_stop_mass(0.0)
        idx.set_fused_mlp(1)
    assert np.array_equal(got, bo[:, :, 0]) and np.array_equal(got_bo, bo[:, :, 0])
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo)
    assert np.array_equal(i, no) and np.array_equal(d.astype(np.float64), do)


# ---- the walk ----
_cases = {}


@pytest.fixture
def case(oracle):
    def get(key):
        key = key if isinstance(key, str) else tuple(key)
        if key not in _cases:
            _cases[key] = Case(oracle, key)
        return _cases[key]
    return get


def walk_expected(c, nb, rows, mass=0.0):
    """(order, counts) of the restatement: path_mass_ref.walk at mass 0 (the oracle's walk: test_stop_rows_host.py) cut by the rows."""
    full, _ = c.expected(0.0, nb)
    return expected_walk(full, c.dp, rows, mass_counts=c.expected(mass, nb)[1] if mass else None)


def check_walk(c, li, nb, rows, mass=0.0):
    bo, counts = walk_expected(c, nb, rows, mass)
    slab_e, ent_e = c.device_order(li, bo)
    eng = li._engine
    eng.set_stop_rows(rows)
    eng.set_path_mass(mass)
    try:
        slab, ent = eng.nav_order(c.Qn, nb)
    finally:
        eng.set_stop_rows(0)
        eng.set_path_mass(0.0)
    print(f"{c.ncat} rows {rows} mass {mass} nb {nb}: rows differing {(ent != ent_e).any(axis=1).sum()} of {c.Qn.shape[0]}, "
          f"cut {(counts < nb).mean():.0%}")
    assert np.array_equal(ent, ent_e)
    assert np.array_equal(slab, slab_e)
    return slab_e, ent_e, bo, counts


@pytest.mark.parametrize("name,nb,rows", list(WALK_FIXTURES))
def test_walk_parity_fixtures(case, name, nb, rows):
    """6. lmi_nav_order on the reference-built fixtures (slab_ids and entries, the -1s included), and result parity: lmi_search_tree
    with host buffers and twice in a row with device buffers, lmi_nav_order + lmi_scan_topk, all against the oracle's search over
    the cut order."""
    c = case(name)
    bo, counts = walk_expected(c, nb, rows)
    assert_not_vacuous(counts, nb)
    li = c.index()
    eng = li._engine
    slab_e, ent_e, _, _ = check_walk(c, li, nb, rows)
    do, no, _ = c.oracle.search(c.root, c.Qn, c.Xs, c.Qs, c.dp, nb, c.k, nthreads=4, bucket_order=bo)
    eng.set_stop_rows(rows)
    d_a, i_a, slab_a, ent_a = eng.search_tree(c.Qn, c.Qs, nb, c.k, want_order=True)
    slab_b, ent_b = eng.nav_order(c.Qn, nb)
    d_b, i_b = eng.scan_topk(c.Qs, slab_b, c.k)
    for a, b in ((d_a, d_b), (i_a, i_b), (slab_a, slab_b), (ent_a, ent_b)):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(slab_a, slab_e) and np.array_equal(ent_a, ent_e)
    assert np.array_equal(i_a, no)
    assert np.array_equal(d_a.astype(np.float64), do)
    dev = torch.device("cuda", 0)
    qn_t, qs_t = torch.from_numpy(np.ascontiguousarray(c.Qn)).to(dev), torch.from_numpy(np.ascontiguousarray(c.Qs)).to(dev)
    ko = eng.kout(nb, c.k)
    nq = c.Qn.shape[0]
    d_t = torch.empty((nq, ko), dtype=torch.float32, device=dev)
    i_t = torch.empty((nq, ko), dtype=torch.int32, device=dev)
    slab_t = torch.empty((nq, nb), dtype=torch.int32, device=dev)
    ent_t = torch.empty((nq, nb), dtype=torch.int32, device=dev)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):   # the per-query sums are set up by the call itself
        eng.search_tree_device(qn_t, qs_t, nb, c.k, d_t, i_t, None, slab_t, ent_t)
    torch.cuda.synchronize()
    eng.set_stream(0)
    assert i_t.cpu().numpy().view(np.uint32).tobytes() == i_a.tobytes()
    assert d_t.cpu().numpy().tobytes() == d_a.tobytes()
    assert np.array_equal(slab_t.cpu().numpy(), slab_e) and np.array_equal(ent_t.cpu().numpy(), ent_e)
    # work is skipped on the walk too
    pairs_on = eng.scan_stats()[1]
    sizes = eng.bucket_sizes().astype(np.int64)
    assert pairs_on == int(sizes[slab_e[slab_e >= 0]].sum())
    eng.set_stop_rows(0)
    eng.search_tree(c.Qn, c.Qs, nb, c.k)
    assert pairs_on < eng.scan_stats()[1]
    li.close()


@pytest.mark.parametrize("ncat,rows", list(WALK_SYNTH))
def test_walk_parity_forms(case, ncat, rows):
    """6. The three launch forms of the walk; listed buckets without objects are recorded and add 0."""
    c = case(ncat)
    bo, counts = walk_expected(c, SYNTH_NB, rows)
    assert_not_vacuous(counts, SYNTH_NB)
    li = c.index()
    slab_e, ent_e, _, _ = check_walk(c, li, SYNTH_NB, rows)
    assert ((ent_e >= 0) & (slab_e < 0)).any()   # recorded buckets without objects inside visited prefixes
    li.close()


@pytest.mark.parametrize("ncat,mass,rows", [COMBINED_SYNTH[:3], ((12, 12), 0.99, 152)])
def test_combined_with_path_mass(case, ncat, mass, rows):
    """5. Both stops on the walk: (5, 4) with its queues in LDS, (12, 12) through the global-memory pop kernel.  The condition of a
    combined case: each stop binds alone for >= 10 % of the queries ((5, 4): the mass for 201 of 300, the rows for 55; (12, 12): 165
    and 86)."""
    c = case(ncat)
    cm = c.expected(mass, SYNTH_NB)[1]
    cr = walk_expected(c, SYNTH_NB, rows)[1]
    assert min((cm < cr).mean(), (cr < cm).mean()) >= 0.10
    bo, counts = walk_expected(c, SYNTH_NB, rows, mass)
    assert np.array_equal(counts, np.minimum(cm, cr)) and np.unique(counts).size >= 3
    li = c.index()
    check_walk(c, li, SYNTH_NB, rows, mass)
    li.close()


# ---- live counts ----
def test_mutated_index(capi, oracle):
    """7. After an insert of the last 20 % and a delete of 700 ids the cut follows the new sizes and the results equal the oracle's on
    the equivalent object list."""
    layers, Qn, Xs, Qs, dp, _ = search_case("G1")
    nb, rows = 4, 1079
    lab = dp[:, 0].astype(np.int64)
    ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    n0 = int(0.8 * Xs.shape[0])
    gone = np.random.RandomState(3).choice(ids, 700, replace=False)
    keep = ~np.isin(ids, gone)
    sizes_first = np.bincount(lab[:n0], minlength=12)
    sizes_new = np.bincount(lab[keep], minlength=12)
    bo_first, _ = expected_order(oracle, layers, Qn, nb, sizes_first, rows)
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes_new, rows)
    assert_not_vacuous(counts, nb)
    assert (bo != bo_first).any(axis=(1, 2)).sum() >= 10     # the sizes at the build would cut differently
    idx = capi.Index(0)
    idx.set_mlp(layers)
    idx.set_buckets(Xs[:n0], lab[:n0], 12, ids=ids[:n0])
    idx.set_stop_rows(rows)                                  # before the mutations: the counts are read by the call, not by the setter
    assert np.array_equal(idx.mlp_topk(Qn, nb), bo_first[:, :, 0])
    assert idx.insert(Xs[n0:], lab[n0:], ids[n0:]) == Xs.shape[0] - n0
    assert idx.delete(gone) == 700
    assert np.array_equal(idx.bucket_sizes(), sizes_new)
    do, no, _ = oracle.search(layers, Qn, Xs[keep], Qs, lab[keep], nb, 10, ids=ids[keep], nthreads=4, bucket_order=bo)
    d, i, got = idx.search(Qn, Qs, nb, 10)
    idx.close()
    assert np.array_equal(got, bo[:, :, 0]) and np.array_equal(i, no) and np.array_equal(d.astype(np.float64), do)


def test_subset_carries_and_cuts_by_its_own_counts(capi, oracle):
    """7. A subset that drops every second object carries the setting and cuts by its OWN counts: its order differs from its
    parent's, and its results equal the oracle's on the kept objects."""
    layers, Qn, Xs, Qs, dp, sizes = search_case("G1")
    nb, rows = 4, 540
    lab = dp[:, 0].astype(np.int64)
    ids = np.arange(1, Xs.shape[0] + 1, dtype=np.uint32)
    sizes_sub = np.bincount(lab[::2], minlength=12)
    bo_par, _ = expected_order(oracle, layers, Qn, nb, sizes, rows)
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes_sub, rows)
    assert_not_vacuous(counts, nb)
    assert (bo != bo_par).any()
    idx = capi.Index(0)
    idx.set_mlp(layers)
    idx.set_buckets(Xs, lab, 12, ids=ids)
    idx.set_stop_rows(rows)
    sub = idx.subset(ids[::2])
    assert sub.stop_rows == rows
    assert np.array_equal(sub.bucket_sizes(), sizes_sub)
    got_par = idx.mlp_topk(Qn, nb)
    idx.set_stop_rows(0)                       # independent handles: the subset keeps its value
    d, i, got = sub.search(Qn, Qs, nb, 10)
    sub.close()
    idx.close()
    assert np.array_equal(got_par, bo_par[:, :, 0])
    assert np.array_equal(got, bo[:, :, 0]) and (got != got_par).any()
    do, no, _ = oracle.search(layers, Qn, Xs[::2], Qs, lab[::2], nb, 10, ids=ids[::2], nthreads=4, bucket_order=bo)
    assert np.array_equal(i, no) and np.array_equal(d.astype(np.float64), do)


def test_clone_view_inherits(capi, oracle):
    """7. A clone view made after the setter inherits the value, one made before does not; the two are independent afterwards."""
    layers, Qn, Xs, Qs, dp, sizes = search_case("G1")
    nb, rows = 4, 1079
    bo, _ = expected_order(oracle, layers, Qn, nb, sizes, rows)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo)
    full = oracle.precompute_bucket_order(layers, Qn, nb)[:, :, 0]
    idx = built(capi, layers, Xs, dp[:, 0])
    plain = idx.clone_view()
    idx.set_stop_rows(rows)
    view = idx.clone_view()
    assert view.stop_rows == rows and plain.stop_rows == 0
    idx.set_stop_rows(0)
    d, i, got = view.search(Qn, Qs, nb, 10)
    assert np.array_equal(got, bo[:, :, 0]) and np.array_equal(i, no) and np.array_equal(d.astype(np.float64), do)
    assert np.array_equal(plain.search(Qn, Qs, nb, 10)[2], full)
    assert np.array_equal(idx.search(Qn, Qs, nb, 10)[2], full)
    idx.close()


# ---- off means off, and refusals ----
def test_off_means_off_and_refusals(capi, oracle):
    """8. 0 after a value is byte-identical to a handle that never called the setter; n_buckets 1 and lmi_mlp_proba are unaffected; a
    negative value is refused and leaves the value in force; the largest int64 cuts nothing; a handle without an index and an index
    with a partial `owned` mask refuse a call that would be cut."""
    layers, Qn, Xs, Qs, dp, sizes = search_case("G1")
    nb, rows = 4, 1079
    bo, _ = expected_order(oracle, layers, Qn, nb, sizes, rows)
    never = built(capi, layers, Xs, dp[:, 0])
    idx = built(capi, layers, Xs, dp[:, 0])
    assert idx.stop_rows == 0
    ref, ref1 = never.search(Qn, Qs, nb, 10), never.search(Qn, Qs, 1, 10)
    probs, classes = never.mlp_proba(Qn)
    idx.set_stop_rows(rows)
    assert idx.stop_rows == rows
    for a, b in zip(idx.search(Qn, Qs, 1, 10), ref1):
        assert a.tobytes() == b.tobytes()
    assert idx.mlp_topk(Qn, 1).tobytes() == never.mlp_topk(Qn, 1).tobytes()
    probs2, classes2 = idx.mlp_proba(Qn)
    assert classes2.tobytes() == classes.tobytes() and probs2.tobytes() == probs.tobytes() and (classes2 >= 0).all()
    for bad in (-1, -(2 ** 40), -INT64_MAX - 1):
        with pytest.raises(capi.LmiError, match="lmi_set_stop_rows"):
            idx.set_stop_rows(bad)
        assert idx.stop_rows == rows
    assert np.array_equal(idx.search(Qn, Qs, nb, 10)[2], bo[:, :, 0])   # the refused values changed nothing
    assert np.array_equal(idx.mlp_topk(Qn, nb), bo[:, :, 0])
    # a caller's own bucket order is scanned as it is
    for a, b in zip(idx.scan_topk(Qs, ref[2], 10), never.scan_topk(Qs, ref[2], 10)):
        assert a.tobytes() == b.tobytes()
    idx.set_stop_rows(INT64_MAX)
    for a, b in zip(idx.search(Qn, Qs, nb, 10), ref):
        assert a.tobytes() == b.tobytes()
    idx.set_stop_rows(1)                                                # the smallest budget: G1 has no empty bucket, one rank each
    got = idx.mlp_topk(Qn, nb)
    assert np.array_equal(got[:, 0], ref[2][:, 0]) and (got[:, 1:] == -1).all()
    idx.set_stop_rows(0)
    for a, b in zip(idx.search(Qn, Qs, nb, 10), ref):
        assert a.tobytes() == b.tobytes()
    assert idx.mlp_topk(Qn, nb).tobytes() == never.mlp_topk(Qn, nb).tobytes()
    idx.close()
    never.close()
    # a handle with an MLP and no index
    bare = capi.Index(0)
    bare.set_mlp(layers)
    full = oracle.precompute_bucket_order(layers, Qn, nb)[:, :, 0]
    assert np.array_equal(bare.mlp_topk(Qn, nb), full)                  # works with the stop off, as before
    bare.set_stop_rows(rows)
    with pytest.raises(capi.LmiError, match="lmi_set_stop_rows.*no built index"):
        bare.mlp_topk(Qn, nb)
    assert np.array_equal(bare.mlp_topk(Qn, 1), full[:, :1])            # a single rank is never cut: answered
    bare.set_stop_rows(0)
    assert np.array_equal(bare.mlp_topk(Qn, nb), full)
    bare.close()
    # an index built with an `owned` mask that leaves buckets out
    owned = (np.arange(12) % 2 == 0).astype(np.uint8)
    part = capi.Index(0)
    part.set_mlp(layers)
    part.set_buckets(Xs, dp[:, 0], 12, owned=owned)
    before = part.search(Qn, Qs, nb, 10)
    part.set_stop_rows(rows)
    for call in (lambda: part.mlp_topk(Qn, nb), lambda: part.search(Qn, Qs, nb, 10)):
        with pytest.raises(capi.LmiError, match="lmi_set_stop_rows.*owned"):
            call()
    for a, b in zip(part.search(Qn, Qs, 1, 10), never_search1(capi, layers, Xs, dp, owned, Qn, Qs)):
        assert a.tobytes() == b.tobytes()
    part.set_stop_rows(0)
    for a, b in zip(part.search(Qn, Qs, nb, 10), before):
        assert a.tobytes() == b.tobytes()
    part.close()


def never_search1(capi, layers, Xs, dp, owned, Qn, Qs):
    h = capi.Index(0)
    h.set_mlp(layers)
    h.set_buckets(Xs, dp[:, 0], 12, owned=owned)
    out = h.search(Qn, Qs, 1, 10)
    h.close()
    return out


def test_off_means_off_walk(case):
    """8. The walk: 0 after a value is byte-identical to a handle that never called the setter; n_buckets 1 is never cut; lmi_set_stop_mass
    still does nothing to the walk."""
    c = case("G7")
    nb, rows = 6, 478
    never, li = c.index(), c.index()
    ref = never._engine.search_tree(c.Qn, c.Qs, nb, c.k, want_order=True)
    first = never._engine.nav_order(c.Qn, 1)
    eng = li._engine
    eng.set_stop_rows(rows)
    cut = eng.search_tree(c.Qn, c.Qs, nb, c.k, want_order=True)
    assert not np.array_equal(cut[2], ref[2])
    for a, b in zip(eng.nav_order(c.Qn, 1), first):
        assert a.tobytes() == b.tobytes()
    eng.set_stop_rows(INT64_MAX)
    for a, b in zip(eng.search_tree(c.Qn, c.Qs, nb, c.k, want_order=True), ref):
        assert a.tobytes() == b.tobytes()
    eng.set_stop_rows(0)
    eng.set_stop_mass(0.5)
    for a, b in zip(eng.search_tree(c.Qn, c.Qs, nb, c.k, want_order=True), ref):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(eng.nav_order(c.Qn, nb), ref[2:]):
        assert a.tobytes() == b.tobytes()
    view_on = None
    eng.set_stop_mass(0.0)
    eng.set_stop_rows(rows)
    view_on = eng.clone_view()
    eng.set_stop_rows(0)
    assert view_on.stop_rows == rows
    for a, b in zip(view_on.search_tree(c.Qn, c.Qs, nb, c.k, want_order=True), cut):
        assert a.tobytes() == b.tobytes()
    li.close()
    never.close()


# ---- interfaces ----
def test_li_api_one_level(oracle):
    """9. LearnedIndex.search / search_resident(stop_rows=) on a 1-level index equal case 3; the engine's own value is restored and the
    next call without the argument is the full search."""
    from learnedmetricindex_amd import _capi
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    name, nb, rows = "G5", 4, 238
    layers, Qn, Xs, Qs, dp, sizes = search_case(name)
    L = layers[-1][0].shape[0]
    dp = dp.astype(np.int64)
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes, rows)
    assert_not_vacuous(counts, nb)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo)
    df, nf, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4)
    assert not np.array_equal(no, nf)
    li = LearnedIndex(net_from_type(layers, MODEL_OF[name]), {}, [(i,) for i in range(L)])
    nav, srch = frame(inputs_for(name, load_golden(name))[0]), frame(Xs)
    d, n, mt = li.search(nav, Qn, srch, Qs, dp, [L], nb, 10, stop_rows=rows)
    assert np.array_equal(n, no) and np.array_equal(d, do) and mt["inference"] > 0
    assert li._engine.stop_rows == 0   # applied for the call, restored afterwards
    d, n, _ = li.search(nav, Qn, srch, Qs, dp, [L], nb, 10)
    assert np.array_equal(n, nf) and np.array_equal(d, df)
    d, n, _ = li.search_resident(Qn, Qs, [L], nb, 10, stop_rows=rows)
    assert np.array_equal(n, no) and np.array_equal(d, do)
    d, n, _ = li.search_resident(Qn, Qs, [L], nb, 10)
    assert np.array_equal(n, nf) and np.array_equal(d, df)
    li._engine.set_stop_rows(7)        # the engine's own value survives a call that overrides it
    li.search_resident(Qn, Qs, [L], nb, 10, stop_rows=rows)
    assert li._engine.stop_rows == 7
    li._engine.set_stop_rows(0)
    with pytest.raises(_capi.LmiError, match="lmi_set_stop_rows"):
        li.search_resident(Qn, Qs, [L], nb, 10, stop_rows=-5)
    assert li._engine.stop_rows == 0
    with pytest.raises(ValueError, match="stop_mass"):   # path_mass on a 1-level index stays refused
        li.search_resident(Qn, Qs, [L], nb, 10, path_mass=0.9, stop_rows=rows)
    li.close()


def net_from_type(layers, model_type):
    from learnedmetricindex_amd.li.model import NeuralNetwork

    net = NeuralNetwork(input_dim=layers[0][0].shape[1], output_dim=layers[-1][0].shape[0], model_type=model_type)
    lin = [m for m in net.model.layers if isinstance(m, torch.nn.Linear)]
    assert len(lin) == len(layers)
    with torch.no_grad():
        for m, (W, b) in zip(lin, layers):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
    return net


def test_li_api_multi_level(case):
    """9. The same on a multi-level index (G7) equals case 6; _precompute_bucket_order returns EMPTY_VALUE paths behind the stop."""
    from learnedmetricindex_amd.li.LearnedIndex import LearnedIndex

    c, nb, rows = case("G7"), 6, 478
    bo, counts = walk_expected(c, nb, rows)
    assert_not_vacuous(counts, nb)
    full = c.expected(0.0, nb)[0]
    do, no, _ = c.oracle.search(c.root, c.Qn, c.Xs, c.Qs, c.dp, nb, c.k, nthreads=4, bucket_order=bo)
    df, nf, _ = c.oracle.search(c.root, c.Qn, c.Xs, c.Qs, c.dp, nb, c.k, nthreads=4, bucket_order=full)
    assert not np.array_equal(no, nf)
    li = LearnedIndex(net_from(c.root), {tuple(p): net_from(l) for p, l in c.internal}, c.bucket_paths)
    nav, srch = frame(c.Xn), frame(c.Xs)
    d, n, mt = li.search(nav, c.Qn, srch, c.Qs, c.dp, c.ncat, nb, c.k, stop_rows=rows)
    assert np.array_equal(n, no) and np.array_equal(d, do) and mt["inference"] > 0
    assert li._engine.stop_rows == 0
    d, n, _ = li.search(nav, c.Qn, srch, c.Qs, c.dp, c.ncat, nb, c.k)
    assert np.array_equal(n, nf) and np.array_equal(d, df)
    d, n, _ = li.search_resident(c.Qn, c.Qs, c.ncat, nb, c.k, stop_rows=rows)
    assert np.array_equal(n, no) and np.array_equal(d, do)
    d, n, _ = li.search_resident(c.Qn, c.Qs, c.ncat, nb, c.k)
    assert np.array_equal(n, nf) and np.array_equal(d, df)
    with pytest.raises(ValueError, match="multi-level"):   # stop_mass on a tree stays refused
        li.search_resident(c.Qn, c.Qs, c.ncat, nb, c.k, stop_mass=0.9, stop_rows=rows)
    li._NAV_QUEUE_BYTES = 8 * 110 * 37                      # the walk in chunks of 37 queries
    d, n, _ = li.search_resident(c.Qn, c.Qs, c.ncat, nb, c.k, stop_rows=rows)
    assert np.array_equal(n, no) and np.array_equal(d, do)
    li._engine.set_stop_rows(rows)
    got, _ = li._precompute_bucket_order(c.Qn, nb, c.ncat)
    assert np.array_equal(got, bo)
    li._engine.set_stop_rows(0)
    got, _ = li._precompute_bucket_order(c.Qn, nb, c.ncat)
    assert np.array_equal(got, full)
    li.close()


@pytest.mark.parametrize("mode", ["nav", "plain", "twin", "plain-python"])
def test_pipeline(capi, oracle, mode):
    """9. HostPipeline(stop_rows=...) returns, batch by batch, what the direct call with the stop returns (and the oracle)."""
    from learnedmetricindex_amd.pipeline import HostPipeline

    layers, Qn, Xs, Qs, dp, sizes = search_case("G1")
    nb, rows, nq = 4, 1079, 96
    idx = built(capi, layers, Xs, dp[:, 0])
    pipe = HostPipeline(idx, nq, Qn.shape[1], Qs.shape[1], nb, 10, depth=2, same_queries=True, want_bucket_order=True,
                        overlap_inference=mode == "nav", two_handles=mode == "twin", native_submit=mode != "plain-python",
                        stop_rows=rows)
    assert len(pipe.handles) == (2 if mode == "twin" else 1) and all(h.stop_rows == rows for h, _ in pipe.handles)
    rs = np.random.RandomState(0)
    batches = [np.sort(rs.choice(Qn.shape[0], nq, replace=False)) for _ in range(5)]
    got = []
    for sel in batches:
        t = pipe.submit(np.ascontiguousarray(Qn[sel]))
        d, i = pipe.result(t)
        got.append((d.copy(), i.copy(), pipe.bucket_order(t).copy()))
    pipe.close()
    assert idx.stop_rows == 0     # the pipeline's setting ends with it
    idx.set_stream(0)
    idx.set_stop_rows(rows)       # the direct calls below
    cut = 0
    for sel, (d, i, bo_p) in zip(batches, got):
        q = np.ascontiguousarray(Qn[sel])
        d0, i0, bo0 = idx.search(q, q, nb, 10)
        bo, counts = expected_order(oracle, layers, q, nb, sizes, rows)
        cut += int((counts < nb).sum())
        assert np.array_equal(bo_p, bo0) and np.array_equal(bo_p, bo[:, :, 0])
        assert np.array_equal(i, i0) and np.array_equal(d, d0)
    assert cut > 0
    q = np.ascontiguousarray(Qn[batches[0]])
    do, no, _ = oracle.search(layers, q, Xs, q, dp, nb, 10, nthreads=4, bucket_order=expected_order(oracle, layers, q, nb, sizes, rows)[0])
    assert np.array_equal(got[0][1], no) and np.array_equal(got[0][0].astype(np.float64), do)
    idx.close()


@pytest.mark.parametrize("searcher", ["sharded", "replica"])
def test_sharded_world_of_one(capi, oracle, searcher):
    """9. A world-of-one ShardedSearcher / ReplicaSearcher with stop_rows equals the direct call and the oracle; more than one
    bucket-sharded rank is refused before anything is set."""
    from learnedmetricindex_amd.sharded import ReplicaSearcher, ShardedSearcher

    layers, Qn, Xs, Qs, dp, sizes = search_case("G5")
    nb, rows = 4, 238
    bo, counts = expected_order(oracle, layers, Qn, nb, sizes, rows)
    assert_not_vacuous(counts, nb)
    do, no, _ = oracle.search(layers, Qn, Xs, Qs, dp, nb, 10, nthreads=4, bucket_order=bo)
    dev = torch.device("cuda", 0)
    qn, qs = torch.from_numpy(Qn).to(dev), torch.from_numpy(Qs).to(dev)
    idx = built(capi, layers, Xs, dp[:, 0], chunk_rows=256)
    with pytest.raises(ValueError, match="stop_rows"):
        ShardedSearcher(idx, 0, 2, stop_rows=rows)
    assert idx.stop_rows == 0
    idx.set_stream(torch.cuda.current_stream().cuda_stream)
    s = ShardedSearcher(idx, 0, 1, stop_rows=rows) if searcher == "sharded" else ReplicaSearcher(idx, 0, 1, stop_rows=rows)
    assert idx.stop_rows == rows
    sd, si, sbo = s.search(qn, qs, nb, 10)
    torch.cuda.synchronize()
    sd, si, sbo = sd.cpu().numpy(), si.cpu().numpy().view(np.uint32), sbo.cpu().numpy()
    idx.set_stream(0)
    d0, i0, bo0 = idx.search(Qn, Qs, nb, 10)
    s.close()
    assert idx.stop_rows == 0   # the searcher's setting ends with it
    assert np.array_equal(idx.search(Qn, Qs, nb, 10)[2], oracle.precompute_bucket_order(layers, Qn, nb)[:, :, 0])
    idx.close()
    assert np.array_equal(sbo, bo0) and np.array_equal(si, i0) and np.array_equal(sd, d0)
    assert np.array_equal(sbo, bo[:, :, 0]) and np.array_equal(si, no) and np.array_equal(sd.astype(np.float64), do)
