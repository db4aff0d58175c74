"""The path-mass stop of the multi-level walk (`lmi_set_path_mass`) restated in numpy on top of the unchanged oracle -- shared
by test_path_mass_host.py and test_gpu_path_mass.py.

Definition (include/lmi_hip.h): every queue entry carries a path mass beside its priority.  A root child's mass is the
probability predict_proba gives it; a child pushed when an internal entry of mass M is expanded has M * p_local (one binary32
multiply).  Priorities, pop order and the tie rule are the walk's own: the local probability, the later-pushed entry wins a tie,
the root's children are pushed least probable first and a node's children most probable first.  When the walk records a
bucket of mass m (a listed bucket without objects included; a path that is neither a node nor a bucket is dropped and adds
nothing) c_0 = m_0, c_j = c_{j-1} + m_j (one binary32 add each); the first bucket is always recorded and the query goes on
after j recorded buckets only while c_{j-1} < mass (a binary32 compare: false on NaN).  mass 0: off."""
import numpy as np

from stop_mass_ref import assert_not_vacuous, count_histogram  # noqa: F401  (re-exported for the tests)

EMPTY_VALUE = -1


class Tree:
    """The per-model probabilities of a batch of queries (one oracle.predict_proba per model) and the tree's paths."""

    def __init__(self, oracle, root_layers, internal, bucket_paths, Q, n_categories, nthreads=4):
        self.n_levels = len(n_categories)
        self.Q = np.ascontiguousarray(Q, dtype=np.float32)
        self.root = oracle.predict_proba(root_layers, self.Q, nthreads)          # (probs descending, classes)
        self.node = {}
        for path, layers in internal:
            prefix = tuple(int(v) for v in path if int(v) != EMPTY_VALUE)
            self.node[prefix] = oracle.predict_proba(layers, self.Q, nthreads)
        self.buckets = {tuple(int(v) for v in p if int(v) != EMPTY_VALUE) for p in bucket_paths}


def walk(tree, n_buckets, mass):
    """(bucket_order int32[nq, n_buckets, n_levels] with EMPTY_VALUE behind the stop, visited counts int[nq]).

    `visited` counts the recorded buckets (those without objects included): n_buckets for a query that is not cut."""
    nq, n_levels = tree.Q.shape[0], tree.n_levels
    limit = np.float32(mass)
    on = float(mass) != 0.0
    order = np.full((nq, n_buckets, n_levels), EMPTY_VALUE, dtype=np.int32)
    counts = np.zeros(nq, dtype=np.int64)
    rp, rc = tree.root
    for q in range(nq):
        prio, pmass, path, alive = [], [], [], []
        for j in reversed(range(rp.shape[1])):           # least probable first
            prio.append(rp[q, j]); pmass.append(np.float32(rp[q, j])); path.append((int(rc[q, j]),)); alive.append(True)
        have, cum = 0, np.float32(0)
        while have < n_buckets:
            best = -1
            for i in range(len(prio)):
                if alive[i] and (best < 0 or prio[i] >= prio[best]):   # >=: the later entry wins a tie
                    best = i
            if best < 0:
                break                                     # queue exhausted: the remaining slots stay EMPTY_VALUE
            alive[best] = False
            p, m = path[best], pmass[best]
            if p in tree.node:
                probs, cats = tree.node[p]
                for j in range(probs.shape[1]):           # most probable first
                    child = np.float32(m) * np.float32(probs[q, j])
                    assert child.dtype == np.float32
                    prio.append(probs[q, j]); pmass.append(child); path.append(p + (int(cats[q, j]),)); alive.append(True)
            elif p in tree.buckets:
                order[q, have, :len(p)] = p
                cum = np.float32(m) if have == 0 else cum + np.float32(m)
                assert cum.dtype == np.float32
                have += 1
                if on and not (cum < limit):
                    break
        counts[q] = have
    return order, counts


def expected_order(oracle, root_layers, internal, bucket_paths, Q, n_buckets, n_categories, mass, nthreads=4):
    return walk(Tree(oracle, root_layers, internal, bucket_paths, Q, n_categories, nthreads), n_buckets, mass)


def synthetic_tree(ncat, nq=300):
    """The generator of test_gpu_li_api.py::test_walk_forms_against_the_oracle (same seeds, same draws in the same order) without
    torch: (root layers, internal [(path, layers)], bucket_paths, data_prediction, Xn, Xs, Qn, Qs).  The li `MLP` model is
    Linear(d, 128) -> ReLU -> Linear(128, classes); node 1 keeps one bucket with rows, its other children are listed and empty."""
    rs = np.random.RandomState(sum(ncat))
    d_nav, d_s, N, hidden = 16, 24, 4000, 128

    def model(n_out):
        out = []
        for shape in ((hidden, d_nav), (n_out, hidden)):
            W = (rs.randn(*shape) * 0.5).astype(np.float32)
            b = (rs.randn(shape[0]) * 0.1).astype(np.float32)
            out.append((W, b))
        return out

    root = model(ncat[0])
    internal = [((i, EMPTY_VALUE), model(ncat[1])) for i in range(ncat[0])]
    bucket_paths = [(i, j) for i in range(ncat[0]) for j in range(ncat[1])]
    dp = np.stack([rs.randint(0, ncat[0], N), rs.randint(0, ncat[1], N)], axis=1).astype(np.int64)
    dp[dp[:, 0] == 1] = (1, 0)
    Xn, Xs = rs.randn(N, d_nav).astype(np.float32), rs.randn(N, d_s).astype(np.float32)
    Qn, Qs = rs.randn(nq, d_nav).astype(np.float32), rs.randn(nq, d_s).astype(np.float32)
    return root, internal, bucket_paths, dp, Xn, Xs, Qn, Qs
