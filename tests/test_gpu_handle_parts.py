"""GPU (`-m gpu`): what a clone view and a subset take from their handle, by the parts the handle is made of (csrc/lmi_handle.h).

A clone view borrows the models and every index image and answers bit for bit like its parent, before and after another clone has
come and gone; its call state -- statistics, timings, the last scan's candidates -- is its own and starts empty.  A subset carries
the parent's settings over as a whole.  Equality below is equality of bit patterns, no tolerance.

Shapes: N = 4096 objects in L = 16 buckets, 64 queries, n_buckets = 4, k = 10 -- the smallest at which every form still runs its own
kernels: d = 64 is the prefilter's low-dimensional form, d = 256 the other one (its own fragment shape and images)."""
import numpy as np
import pytest

from test_gpu_mutate import Mirror, dataset, fresh, mlp

pytestmark = pytest.mark.gpu

N, L, NQ, NB, K = 4096, 16, 64, 4, 10
# (name, d, Index settings): the prefilter's low-d form, the all-f32 scan, the fp16 fragments only, the prefilter's other form
FORMS = [("f32", 64, dict()), ("exact", 64, dict(prefilter=False)), ("f16", 64, dict(storage="f16")), ("f32", 256, dict())]
FORM_IDS = [f"{name}-d{d}" for name, d, _ in FORMS]


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


_data = {}


def data(d):
    """(Mirror of N binary16-exact objects, root model, queries) per d: made once, never changed."""
    if d not in _data:
        rs = np.random.RandomState(7000 + d)
        X = dataset(rs, N, d).astype(np.float16).astype(np.float32)   # (max |x| < 1: admissible for storage="f16")
        lab = rs.randint(0, L, N)
        ids = (rs.permutation(2 ** 20)[:N].astype(np.uint64) * 4093 + 7).astype(np.uint32)
        Q = dataset(rs, NQ, d).astype(np.float16).astype(np.float32)
        for a in (X, lab, ids, Q):
            a.setflags(write=False)
        _data[d] = (Mirror(X, lab, ids), mlp(rs, d, L), Q)
    return _data[d]


def bits(out):
    return [np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a for a in out]


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(bits(a), bits(b)):
        assert x.dtype == y.dtype and np.array_equal(x, y)


@pytest.mark.parametrize("name,d,kw", FORMS, ids=FORM_IDS)
def test_clone_answers_like_its_parent_and_leaves_it_whole(capi, name, d, kw):
    m, layers, Q = data(d)
    parent = fresh(capi, layers, m, L, **kw)
    try:
        ref = parent.search(Q, Q, NB, K, want_keys=True)
        assert (ref[1] != 0).any()
        view = parent.clone_view()
        assert view.index_bytes() == parent.index_bytes()
        same_bits(view.search(Q, Q, NB, K, want_keys=True), ref)
        same_bits(view.search(Q, Q, NB, K, want_keys=True), ref)     # (its workspaces in use for the second time)
        same_bits(parent.search(Q, Q, NB, K, want_keys=True), ref)   # both alive
        view.close()                                                  # the clone first: it frees its own, nothing of the parent's
        same_bits(parent.search(Q, Q, NB, K, want_keys=True), ref)
        view = parent.clone_view()                                    # ... and once more
        same_bits(view.search(Q, Q, NB, K, want_keys=True), ref)
        view.close()
        same_bits(parent.search(Q, Q, NB, K, want_keys=True), ref)
    finally:
        parent.close()


@pytest.mark.parametrize("name,d,kw", FORMS, ids=FORM_IDS)
def test_clone_starts_with_a_call_state_of_its_own(capi, name, d, kw):
    m, layers, Q = data(d)
    parent = fresh(capi, layers, m, L, **kw)
    try:
        parent.timings_reset()
        parent.search(Q, Q, NB, K)
        stats = parent.scan_stats()            # (read: the parent now holds its last scan's figures on the host)
        pf = parent.prefilter_stats()
        calls = parent.timings_mean()[1]
        assert calls == 1 and stats[1] > 0
        view = parent.clone_view()
        assert view.scan_stats() == (0.0, 0, 0)
        assert view.prefilter_stats()[1:] == (0, 0)
        assert view.prefilter_stats()[0] == pf[0]          # (whether the index HAS the prefilter's images is the index's, not the call's)
        assert view.timings_mean()[1] == 0
        with pytest.raises(capi.LmiError):
            view.debug_read_candidates(0)
        view.search(Q[:33], Q[:33], 2, K)                  # another batch, another fan-out: other figures
        assert view.scan_stats() != stats and view.scan_stats()[1] > 0 and view.timings_mean()[1] == 1
        assert parent.scan_stats() == stats                # the parent's own are what they were
        assert parent.prefilter_stats() == pf
        assert parent.timings_mean()[1] == calls
        view.close()
    finally:
        parent.close()


def test_tree_clone_and_subset_walk_like_the_parent(capi):
    """Root + two node models (2 x 8 leaves = the 16 buckets): the clone borrows all three models and the tree tables, the subset has
    copies of its own made by one loop over the models."""
    d = 64
    m, _, Q = data(d)
    rs = np.random.RandomState(11)
    parent = capi.Index(0)
    view = sub = None
    try:
        parent.set_mlp(mlp(rs, d, 2))
        parent.nav_set_model(1, mlp(rs, d, 8))
        parent.nav_set_model(2, mlp(rs, d, 8, hidden=40))
        parent.nav_set_tree([0, 2, 10, 18], [1, 2] + [-1] * 16, [-2, -2] + list(range(16)))
        parent.set_buckets(m.X, m.lab, L, ids=m.ids)
        ref = parent.search_tree(Q, Q, NB, K, want_keys=True, want_order=True)
        assert (ref[3] >= 0).all() and (ref[3] < 8).any() and (ref[3] >= 8).any()   # leaves of both node models: all three took part
        view = parent.clone_view()
        sub = parent.subset([], drop=True)   # the same objects
        same_bits(view.search_tree(Q, Q, NB, K, want_keys=True, want_order=True), ref)
        same_bits(sub.search_tree(Q, Q, NB, K, want_keys=True, want_order=True), ref)
        view.close()
        view = None
        same_bits(parent.search_tree(Q, Q, NB, K, want_keys=True, want_order=True), ref)
        parent.close()                       # the subset owns its models, tree and images
        same_bits(sub.search_tree(Q, Q, NB, K, want_keys=True, want_order=True), ref)
    finally:
        for idx in (view, sub, parent):
            if idx is not None:
                idx.close()


def test_subset_carries_every_setting_over(capi):
    """chunk_rows, stop_mass, fused_mlp and the metric, none at its default: the full copy answers like a fresh Index given the same
    settings and rows, the ranks the stop cut (-1) included."""
    m, layers, Q = data(64)
    # the last layer times 8: the top class alone covers half the mass for some queries, the top three do for most, so the stop cuts
    # ranks for most queries and not the same number for all
    layers = [layers[0], (layers[1][0] * 8, layers[1][1] * 8)]

    def configured():
        idx = capi.Index(0, chunk_rows=256, metric="l2")
        idx.set_stop_mass(0.5)
        idx.set_fused_mlp(0)
        idx.set_mlp(layers)
        idx.set_buckets(m.X, m.lab, L, ids=m.ids)
        return idx

    parent, ref = configured(), configured()
    sub = None
    try:
        want = ref.search(Q, Q, NB, K, want_keys=True)
        order = want[2]
        assert (order[:, 0] >= 0).all() and (order == -1).any() and (order[:, 1:] >= 0).any()   # the stop cuts some ranks, not all
        sub = parent.subset([], drop=True)
        assert sub.N == N and sub.metric == "l2" and sub.stop_mass == 0.5
        same_bits(sub.search(Q, Q, NB, K, want_keys=True), want)
        same_bits(parent.search(Q, Q, NB, K, want_keys=True), want)
        parent.close()
        same_bits(sub.search(Q, Q, NB, K, want_keys=True), want)
        assert sub.debug_layout()["n_rb_total"] == ref.debug_layout()["n_rb_total"] and sub.index_bytes() == ref.index_bytes()
    finally:
        for idx in (sub, parent, ref):
            if idx is not None:
                idx.close()
