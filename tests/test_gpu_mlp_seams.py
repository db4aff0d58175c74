"""GPU (`-m gpu`): the MLP forward's dispatch seams and model shapes.  mlp_plan() (csrc/lmi_host_model.h) and the launch sites pick
between mlp_fused_kernel<MODE>, the mlp_layer_kernel<LAST, CBW> chain and a split of a batch over both, and between the ranking in
the fused epilogue and one of three ranking kernels; here every threshold has one case on each side, and every case

  1. compares bucket order, logits, predict_proba's probabilities and classes with the CPU oracle (forward_logits, rank_classes,
     predict_proba) -- floats as their bits (`same_bits`), never by float equality: -0 is not +0 here;
  2. runs the call without the logits output and a second time: both equal the first;
  3. asserts, from `debug_last_mlp_plan()` after the call, the plan words the case is about, and that `debug_mlp_plan()`, which
     launches nothing, said the same word for word.

Then model shapes the fixtures do not hold (one to eight Linears, input widths around the kernel's chunking, class counts 1..65),
directed ranking and softmax inputs (ties, equal logits, -inf, the exponential's cut, -0 through ReLU, NaN), trees whose nodes
differ in depth, width and class count, and sequences of calls on ONE handle against fresh handles.

Where the thresholds come from (C = num_cus, a plan word; ncb = ceil(nq / 32); n_rb = ceil(width / 32)):
  fused at all         lmi_set_fused_mlp != 0 and every hidden width <= 512             (fused_lds_plan: FM_MAXH, lmi_mlp_fused.h)
  fill, mode 1         2 ncb >= C; mode 2 and lmi_mlp_proba: always                      (mlp_plan: `fill`)
  thin last round      mode 1, no logits output, not proba, classes <= 512, ncb > C, 0 < ncb % C, 10 (ncb % C) < 3 C: the last
                       ncb % C blocks go through the per-layer chain on a side stream   (mlp_plan: `rem`)
  CBW of a layer       ceil(n_rb / 4) ceil(ncb / 4) >= 2 C: 4; ... ceil(ncb / 2) ...: 2; else 1   (mlp_layer_cbw)
  logits in LDS        classes <= 512; beyond: through global memory and rank_classes_kernel / _stop_ / _rows_kernel (+
                       softmax_ranked_kernel for lmi_mlp_proba)                           (fused_lds_plan, rank_kernel_of)
  row-block passes     16 row-blocks (512 outputs) per pass of the fused kernel           (mlp_fused_kernel: `pass`)
  layer 0 of the fused kernel   chunks of 96 features; float4 fetches where d % 4 == 0 and the chunk is whole; the weight
                       rotation is three deep with clamps at KG - 1 (KG = ceil(d / 8))   (mlp_fused_kernel: fetch, FM_RANGE)
  LDS plan             (2 * 32 * 97 + 32 (w0 + 1) + 32 (w1 + 1)) * 4 bytes, w0 / w1 the widest padded layer of even / odd index
"""
import numpy as np
import pytest

import path_mass_ref
import stop_mass_ref
import stop_rows_ref

pytestmark = pytest.mark.gpu

FM_TOPK, FM_PROBA, FM_TOPK_STOP, FM_TOPK_ROWS = 0, 1, 3, 5


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def cdiv(a, b):
    return -(-a // b)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b, what=""):
    """Equal shape, type and bit patterns (floats are compared as uint32: -0 differs from +0, NaNs compare by payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


def mlp(seed, dims, scale=1.0, bias=0.1):
    """Linear stack dims[0] -> .. -> dims[-1] in torch layout, weights ~ N(0, scale^2 / fan_in)."""
    rs = np.random.RandomState(seed)
    return [((rs.randn(o, i) * (scale / np.sqrt(i))).astype(np.float32), (rs.randn(o) * bias).astype(np.float32))
            for i, o in zip(dims[:-1], dims[1:])]


def queries(seed, nq, d):
    return np.random.RandomState(seed).randn(nq, d).astype(np.float32)


def dims_of(layers):
    return [layers[0][0].shape[1]] + [W.shape[0] for W, _ in layers]


def lds_bytes(dims_list):
    """The fused kernel's LDS plan for a set of models (lmi_host_model.h fused_lds_plan), for widths that stay in LDS."""
    w = [0, 0]
    for dims in dims_list:
        for i, o in enumerate(dims[1:]):
            if cdiv(o, 32) * 32 <= 512:
                w[i & 1] = max(w[i & 1], cdiv(o, 32) * 32)
    return (2 * 32 * 97 + 32 * (w[0] + 1) + 32 * (w[1] + 1)) * 4


class Ref:
    """The oracle's answer for (layers, Q): computed once, read-only, sliced by the cases (rows are independent)."""

    def __init__(self, oracle, layers, Q):
        self.layers, self.Q = layers, Q
        self.logits = oracle.forward_logits(layers, Q, nthreads=4)
        self.L = self.logits.shape[1]
        self.order = oracle.rank_classes(self.logits, self.L)
        self.probs = np.take_along_axis(oracle.softmax(self.logits), self.order.astype(np.int64), axis=1)
        for a in (self.logits, self.order, self.probs):
            a.setflags(write=False)


def handle(capi, layers, mode):
    idx = capi.Index(0)
    idx.set_fused_mlp(mode)
    idx.set_mlp(layers)
    return idx


def has(plan, want):
    assert {f: plan[f] for f in want} == want, (want, plan)


def forward(idx, ref, nq, nb, order=None, proba=True):
    """Every check a case makes on one handle for the first nq queries; `order`: the expected bucket order where a stop cuts it.
    Returns the recorded plans of (mlp_topk with logits, mlp_topk, mlp_proba)."""
    q = np.ascontiguousarray(ref.Q[:nq])
    want = ref.order[:nq, :nb] if order is None else np.asarray(order[:nq], dtype=np.int32)   # (the restatements return int64)
    said = idx.debug_mlp_plan(nq, nb, want_logits=True)
    o, l = idx.mlp_topk(q, nb, want_logits=True)
    plan_l = idx.debug_last_mlp_plan()
    assert said == plan_l, (said, plan_l)
    same_bits(l, ref.logits[:nq], "logits")
    same_bits(o, want, "bucket order (with logits)")
    said = idx.debug_mlp_plan(nq, nb)
    o2 = idx.mlp_topk(q, nb)
    plan = idx.debug_last_mlp_plan()
    assert said == plan, (said, plan)
    same_bits(o2, want, "bucket order")
    same_bits(idx.mlp_topk(q, nb), want, "bucket order, second call")
    assert idx.debug_last_mlp_plan() == plan
    plan_p = None
    if proba:
        said = idx.debug_mlp_plan(nq, want_proba=True)
        p, c = idx.mlp_proba(q)
        plan_p = idx.debug_last_mlp_plan()
        assert said == plan_p, (said, plan_p)
        same_bits(p, ref.probs[:nq], "probabilities")
        same_bits(c, ref.order[:nq], "classes")
        p2, c2 = idx.mlp_proba(q)
        same_bits(p2, p, "probabilities, second call")
        same_bits(c2, c, "classes, second call")
    print(f"nq {nq} nb {nb}: logits {plan_l}\n   topk {plan}\n   proba {plan_p}")
    return plan_l, plan, plan_p


def num_cus(capi):
    idx = handle(capi, mlp(1, [4, 3]), 1)
    try:
        assert set(idx.debug_last_mlp_plan().values()) == {0}   # no forward yet
        return idx.debug_mlp_plan(1)["num_cus"]
    finally:
        idx.close()


# ---- (a) seams ---------------------------------------------------------------------------------------------------------------
SEAM_DIMS = [16, 64, 12]
_refs = {}


def seam_ref(oracle, dims, nq, seed=5, **kw):
    """One reference per model, grown to the largest batch asked for (the same seed: a prefix of the larger draw)."""
    key = (tuple(dims), seed, tuple(sorted(kw.items())))
    if key not in _refs or _refs[key].Q.shape[0] < nq:
        _refs[key] = Ref(oracle, mlp(seed, dims, **kw), queries(seed + 1, nq, dims[0]))
    return _refs[key]


def test_fill_rule(capi, oracle):
    """Mode 1 takes the fused kernel from the first batch whose 32-query blocks number half the CUs; mode 2 at one query; mode 0
    never, not even for predict_proba."""
    C = num_cus(capi)
    below = 32 * ((C - 1) // 2)              # the largest nq with 2 ceil(nq / 32) < C
    assert cdiv(below, 32) * 2 < C <= cdiv(below + 1, 32) * 2
    ref = seam_ref(oracle, SEAM_DIMS, below + 1)
    for mode, nq, fused in ((1, below, 0), (1, below + 1, 1), (2, 1, 1), (0, below + 1, 0)):
        idx = handle(capi, ref.layers, mode)
        try:
            plan_l, plan, plan_p = forward(idx, ref, nq, 4)
        finally:
            idx.close()
        for p in (plan_l, plan):
            has(p, dict(num_cus=C, fm_ok=1, logits_lds=1, lds_bytes=lds_bytes([SEAM_DIMS]), fused=fused, softmax_kernel=0))
            if fused:
                has(p, dict(mode=FM_TOPK, fused_blocks=cdiv(nq, 32), nq_head=nq, layers_queries=0, cbw0=-1, cbw1=-1, rank_kernel=-1, vec_in=1,
                            in_chunks=1))
            else:
                has(p, dict(mode=-1, fused_blocks=0, nq_head=0, layers_queries=nq, cbw0=1, cbw1=1, cbw2=-1, cbw7=-1, rank_kernel=0, vec_in=-1,
                            in_chunks=-1))
        # predict_proba: fused whatever the batch size unless the fused kernel is switched off
        if mode == 0:
            has(plan_p, dict(fused=0, mode=-1, layers_queries=nq, rank_kernel=0, softmax_kernel=1))
        else:
            has(plan_p, dict(fused=1, mode=FM_PROBA, nq_head=nq, layers_queries=0, rank_kernel=-1, softmax_kernel=0))


def split_grids(C):
    """(grid, split) on each side of the thin-last-round rule, and two rounds + 1."""
    last = (3 * C - 1) // 10                 # the last rem with 10 rem < 3 C
    assert 10 * last < 3 * C <= 10 * (last + 1)
    return [(C, False), (C + 1, True), (C + last, True), (C + last + 1, False), (2 * C + 1, True)]


@pytest.mark.parametrize("which", range(5), ids=["one_round", "plus_1", "last_thin", "first_thick", "two_rounds_plus_1"])
def test_split_rule(capi, oracle, which):
    """Mode 1: the blocks of a thin last round leave the fused launch for the per-layer chain; a ragged last block on every side.
    The logits output, predict_proba and a model whose classes do not fit LDS switch the split off."""
    C = num_cus(capi)
    grid, split = split_grids(C)[which]
    rem = grid % C
    nq = 32 * (grid - 1) + (1, 31)[which & 1]
    ref = seam_ref(oracle, SEAM_DIMS, nq)
    idx = handle(capi, ref.layers, 1)
    try:
        plan_l, plan, plan_p = forward(idx, ref, nq, 4)
    finally:
        idx.close()
    if split:
        head = 32 * (grid - rem)
        has(plan, dict(fused=1, mode=FM_TOPK, fused_blocks=grid - rem, nq_head=head, layers_queries=nq - head, cbw1=1, rank_kernel=0))
        assert plan["cbw0"] >= 1 and 0 < nq - head < nq
    else:
        has(plan, dict(fused=1, mode=FM_TOPK, fused_blocks=grid, nq_head=nq, layers_queries=0, cbw0=-1, rank_kernel=-1))
    has(plan_l, dict(fused=1, fused_blocks=grid, nq_head=nq, layers_queries=0, cbw0=-1, rank_kernel=-1))
    has(plan_p, dict(fused=1, mode=FM_PROBA, fused_blocks=grid, nq_head=nq, layers_queries=0, cbw0=-1, rank_kernel=-1))


def test_split_is_off_for_classes_beyond_lds(capi, oracle):
    C = num_cus(capi)
    nq = 32 * C + 1                          # grid C + 1: split for a model whose logits stay in LDS (test_split_rule[plus_1])
    dims = [16, 32, 544]
    ref = seam_ref(oracle, dims, nq)
    idx = handle(capi, ref.layers, 1)
    try:
        _, plan, _ = forward(idx, ref, nq, 4, proba=False)
    finally:
        idx.close()
    has(plan, dict(fm_ok=1, logits_lds=0, fused=1, fused_blocks=C + 1, nq_head=nq, layers_queries=0, cbw0=-1, rank_kernel=0, softmax_kernel=0))


def first_nq(idx, word, value, hi):
    """The first nq at which a plan word reaches `value` (the word is monotone in nq), by bisection over debug_mlp_plan."""
    lo = 1
    assert idx.debug_mlp_plan(lo)[word] < value <= idx.debug_mlp_plan(hi)[word]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if idx.debug_mlp_plan(mid)[word] >= value else (mid, hi)
    return hi


CBW_DIMS = [16, 512, 40]


@pytest.mark.parametrize("cbw,side", [(2, 0), (2, 1), (4, 0), (4, 1)], ids=["cbw1_last", "cbw2_first", "cbw2_last", "cbw4_first"])
def test_layer_cbw(capi, oracle, cbw, side):
    """Mode 0, 16 -> 512 -> 40: the hidden layer's col-blocks per wave go 1 -> 2 -> 4 with the batch, the 40-class layer stays at 1;
    on the upper side of each seam the last block column is ragged (ncb is no multiple of CBW)."""
    C = num_cus(capi)
    probe = handle(capi, mlp(5, CBW_DIMS), 0)
    try:
        at = first_nq(probe, "cbw0", cbw, 64 * 32 * C)
    finally:
        probe.close()
    nq = at - 1 + side
    ref = seam_ref(oracle, CBW_DIMS, nq)
    idx = handle(capi, ref.layers, 0)
    try:
        plan_l, plan, plan_p = forward(idx, ref, nq, 4)
    finally:
        idx.close()
    want = cbw if side else cbw // 2
    for p in (plan_l, plan, plan_p):
        has(p, dict(fused=0, mode=-1, layers_queries=nq, cbw0=want, cbw1=1, cbw2=-1, lds_bytes=lds_bytes([CBW_DIMS])))
    if side:
        assert cdiv(nq, 32) % cbw != 0


def test_last_layer_cbw2(capi, oracle):
    """Mode 0, 16 -> 32 -> 512: the LAST layer's instance with two col-blocks per wave, ragged."""
    C = num_cus(capi)
    dims = [16, 32, 512]
    probe = handle(capi, mlp(5, dims), 0)
    try:
        nq = first_nq(probe, "cbw1", 2, 64 * 32 * C)
    finally:
        probe.close()
    assert cdiv(nq, 32) % 2 == 1
    ref = seam_ref(oracle, dims, nq)
    idx = handle(capi, ref.layers, 0)
    try:
        _, plan, plan_p = forward(idx, ref, nq, 4)
    finally:
        idx.close()
    has(plan, dict(fused=0, cbw0=1, cbw1=2, rank_kernel=0, softmax_kernel=0))
    has(plan_p, dict(fused=0, cbw0=1, cbw1=2, rank_kernel=0, softmax_kernel=1))


@pytest.mark.parametrize("hidden", [512, 513])
def test_hidden_width_seam(capi, oracle, hidden):
    """A hidden layer of 513 (17 row-blocks) does not fit the fused kernel: mode 2 and predict_proba take the per-layer chain, and
    say so in the plan; the results are the oracle's either way."""
    dims = [16, hidden, 12]
    ref = seam_ref(oracle, dims, 77)
    ok = int(hidden <= 512)
    for mode in (2, 1):
        idx = handle(capi, ref.layers, mode)
        try:
            plan_l, plan, plan_p = forward(idx, ref, 77, 4)
        finally:
            idx.close()
        fused = ok if mode == 2 else 0       # (77 queries do not fill the chip)
        for p in (plan_l, plan):
            has(p, dict(fm_ok=ok, logits_lds=1, fused=fused, mode=FM_TOPK if fused else -1, layers_queries=0 if fused else 77))
        has(plan_p, dict(fm_ok=ok, fused=ok, mode=FM_PROBA if ok else -1, softmax_kernel=1 - ok, rank_kernel=-1 if ok else 0))
        if ok:
            has(plan, dict(lds_bytes=lds_bytes([dims])))


@pytest.mark.parametrize("L", [512, 513, 1024, 1056])
def test_class_count_seam(capi, oracle, L):
    """Up to 512 classes are ranked from LDS in the fused epilogue; beyond, the logits go through global memory to
    rank_classes_kernel (and softmax_ranked_kernel).  1 056 classes: three passes of 16 row-blocks."""
    dims = [16, 32, L]
    ref = seam_ref(oracle, dims, 77)
    lds = int(L <= 512)
    idx = handle(capi, ref.layers, 2)
    try:
        plan_l, plan, plan_p = forward(idx, ref, 77, 5)
    finally:
        idx.close()
    for p in (plan_l, plan):
        has(p, dict(fm_ok=1, logits_lds=lds, fused=1, mode=FM_TOPK, nq_head=77, rank_kernel=-1 if lds else 0, softmax_kernel=0,
                    lds_bytes=lds_bytes([dims])))
    has(plan_p, dict(logits_lds=lds, fused=1, mode=FM_PROBA, rank_kernel=-1 if lds else 0, softmax_kernel=1 - lds))


def peaked(seed, dims):
    """A model whose probabilities are peaked enough for a 0.9 mass to cut a six-rank order at different ranks."""
    return mlp(seed, dims, scale=3.5, bias=1.0)


@pytest.mark.parametrize("L", [512, 513])
def test_stop_mass_forms(capi, oracle, L):
    """lmi_set_stop_mass(0.9), six ranks: FM_TOPK_STOP ranks and cuts in the epilogue (512 classes), rank_classes_stop_kernel behind
    the fused launch (513) and behind the per-layer chain (mode 0); one rank is never cut."""
    dims, nb, mass, nq = [16, 32, L], 6, 0.9, 200
    layers, Q = peaked(7, dims), queries(8, nq, 16)
    ref = Ref(oracle, layers, Q)
    bo, counts = stop_mass_ref.expected_order(oracle, layers, Q, nb, mass)
    stop_mass_ref.assert_not_vacuous(counts, nb)
    for mode in (2, 0):
        idx = handle(capi, layers, mode)
        idx.set_stop_mass(mass)
        try:
            plan_l, plan, plan_p = forward(idx, ref, nq, nb, order=bo[:, :, 0])
            _, one, _ = forward(idx, ref, nq, 1, proba=False)
        finally:
            idx.close()
        if mode == 2:
            for p in (plan_l, plan):
                has(p, dict(fused=1, mode=FM_TOPK_STOP, rank_kernel=-1 if L <= 512 else 1))
            has(one, dict(fused=1, mode=FM_TOPK, rank_kernel=-1 if L <= 512 else 0))
            has(plan_p, dict(fused=1, mode=FM_PROBA))
        else:
            for p in (plan_l, plan):
                has(p, dict(fused=0, mode=-1, rank_kernel=1))
            has(one, dict(fused=0, rank_kernel=0))
            has(plan_p, dict(fused=0, rank_kernel=0, softmax_kernel=1))


def test_stop_rows_forms(capi, oracle):
    """lmi_set_stop_rows on a small built index: FM_TOPK_ROWS in the epilogue against rank_classes_rows_kernel behind the per-layer
    chain; one rank is never cut."""
    L, nb, rows, nq = 12, 6, 500, 200
    layers, Q = mlp(9, [16, 32, L], scale=3.0), queries(10, nq, 16)
    rs = np.random.RandomState(11)
    X = rs.randn(3000, 8).astype(np.float32)
    skew = 0.6 ** np.arange(L)                # bucket sizes from 1 244 down to 3: the budget ends a query anywhere from rank 1 to 6
    lab = rs.choice(L, 3000, p=skew / skew.sum()).astype(np.int32)
    sizes = np.bincount(lab, minlength=L)
    ref = Ref(oracle, layers, Q)
    bo, counts = stop_rows_ref.expected_order(oracle, layers, Q, nb, sizes, rows)
    stop_rows_ref.assert_not_vacuous(counts, nb)
    for mode in (2, 0):
        idx = handle(capi, layers, mode)
        try:
            idx.set_buckets(X, lab, L)
            idx.set_stop_rows(rows)
            plan_l, plan, plan_p = forward(idx, ref, nq, nb, order=bo[:, :, 0])
            _, one, _ = forward(idx, ref, nq, 1, proba=False)
        finally:
            idx.close()
        for p in (plan_l, plan):
            has(p, dict(fused=int(mode == 2), mode=FM_TOPK_ROWS if mode == 2 else -1, rank_kernel=-1 if mode == 2 else 2))
        has(one, dict(mode=FM_TOPK if mode == 2 else -1, rank_kernel=-1 if mode == 2 else 0))
        has(plan_p, dict(mode=FM_PROBA if mode == 2 else -1, rank_kernel=-1 if mode == 2 else 0))


def test_debug_mlp_plan_checks_like_the_calls_and_launches_nothing(capi):
    """debug_mlp_plan() refuses what mlp_topk refuses, with the same words behind its own name, and leaves the handle's record alone."""
    idx = capi.Index(0)
    try:
        with pytest.raises(capi.LmiError, match="no MLP set"):
            idx.debug_mlp_plan(8, 1)
        idx.set_mlp(mlp(1, [8, 16, 5]))
        assert set(idx.debug_last_mlp_plan().values()) == {0}
        for nb in (0, 6):
            with pytest.raises(capi.LmiError, match="outside") as mine:
                idx.debug_mlp_plan(8, nb)
            with pytest.raises(capi.LmiError, match="outside") as theirs:
                idx.mlp_topk(np.zeros((8, 8), np.float32), nb)
            assert str(mine.value).replace("lmi_debug_mlp_plan", "lmi_mlp_topk") == str(theirs.value)
        idx.set_stop_rows(10)                # the row budget needs a built index: refused before any launch, by both
        with pytest.raises(capi.LmiError, match="no built index") as mine:
            idx.debug_mlp_plan(8, 2)
        with pytest.raises(capi.LmiError, match="no built index") as theirs:
            idx.mlp_topk(np.zeros((8, 8), np.float32), 2)
        assert str(mine.value).replace("lmi_debug_mlp_plan", "lmi_mlp_topk") == str(theirs.value)
        assert set(idx.debug_last_mlp_plan().values()) == {0}   # a refused call records nothing
        idx.set_stop_rows(0)
        idx.mlp_topk(np.zeros((8, 8), np.float32), 2)
        plan = idx.debug_last_mlp_plan()
        assert plan["layers_queries"] == 8 and idx.debug_mlp_plan(1 << 20, 3)["fused"] == 1
        assert idx.debug_last_mlp_plan() == plan
    finally:
        idx.close()


# ---- (b) model shapes ----------------------------------------------------------------------------------------------------------
def shape_case(capi, oracle, dims, nbs, seed=21, expect=None, proba_expect=None):
    """Modes 2 and 0, nq in {1, 33, 77}, every nb of `nbs`; `expect`: plan words of the fused form's mlp_topk."""
    ref = seam_ref(oracle, dims, 77, seed=seed)
    for mode in (2, 0):
        idx = handle(capi, ref.layers, mode)
        try:
            for nq in (1, 33, 77):
                for nb in nbs:
                    plan_l, plan, plan_p = forward(idx, ref, nq, nb)
                    for p in (plan_l, plan):
                        has(p, dict(fused=int(mode == 2), layers_queries=0 if mode == 2 else nq))
                        if mode == 2 and expect:
                            has(p, expect)
                        if mode == 0:
                            n = len(dims) - 1
                            assert [p[f"cbw{i}"] for i in range(8)] == [1] * n + [-1] * (8 - n)
                    if mode == 2 and proba_expect:
                        has(plan_p, proba_expect)
        finally:
            idx.close()
    return ref


# d -> (vec_in, in_chunks): KG = ceil(d / 8) of 1, 2 and 3, every remainder of the three-deep rotation, scalar and float4 fetches, a
# partial last chunk with d % 4 == 0 (100, 196), exact multiples of 96, an odd wide input
IN_WIDTHS = {1: (0, 1), 7: (0, 1), 8: (1, 1), 9: (0, 1), 16: (1, 1), 17: (0, 1), 24: (1, 1), 92: (1, 1), 96: (1, 1), 97: (0, 2),
             100: (1, 2), 192: (1, 2), 196: (1, 3), 2049: (0, 22)}


@pytest.mark.parametrize("d", sorted(IN_WIDTHS))
def test_input_width(capi, oracle, d):
    vec, chunks = IN_WIDTHS[d]
    shape_case(capi, oracle, [d, 40, 12], (4,), expect=dict(vec_in=vec, in_chunks=chunks, mode=FM_TOPK, rank_kernel=-1))


@pytest.mark.parametrize("hidden", [1, 31, 32, 33, 100, 480, 512])
def test_hidden_width(capi, oracle, hidden):
    dims = [24, hidden, 12]
    shape_case(capi, oracle, dims, (4,), expect=dict(fm_ok=1, lds_bytes=lds_bytes([dims])))


@pytest.mark.parametrize("L", [3, 512, 513, 1056])
def test_one_linear(capi, oracle, L):
    """One Linear: layer 0 is also the last layer, the logits are in act0; beyond 512 classes the input chunks are streamed once per
    pass of 16 row-blocks."""
    lds = int(L <= 512)
    shape_case(capi, oracle, [40, L], (min(L, 5),), expect=dict(logits_lds=lds, rank_kernel=-1 if lds else 0, in_chunks=1),
               proba_expect=dict(softmax_kernel=1 - lds))


DEEP8 = [45, 33, 512, 31, 96, 8, 257, 64, 19]


@pytest.mark.parametrize("dims", [[24, 40, 64, 33, 12], DEEP8], ids=["four", "eight"])
def test_depth(capi, oracle, dims):
    """Four and eight Linears: the activations ping-pong by layer parity and the logits come from buffer (n_layers - 1) & 1."""
    ref = shape_case(capi, oracle, dims, (5,), expect=dict(fm_ok=1, logits_lds=1, lds_bytes=lds_bytes([dims])))
    assert len({tuple(r) for r in ref.order[:, :5]}) >= 10   # the deep model's logits are not degenerate


def test_nine_linears_are_refused(capi):
    idx = capi.Index(0)
    try:
        with pytest.raises(capi.LmiError, match="n_layers 9 out of range"):
            idx.set_mlp(mlp(1, [8] * 10))
        with pytest.raises(capi.LmiError, match="no MLP set"):
            idx.mlp_topk(np.zeros((1, 8), np.float32), 1)
        idx.set_mlp(mlp(1, [8] * 9))         # eight are taken
        assert idx.mlp_topk(np.zeros((1, 8), np.float32), 1).shape == (1, 1)
    finally:
        idx.close()


@pytest.mark.parametrize("L", [1, 2, 7, 8, 9, 63, 64, 65])
def test_class_count(capi, oracle, L):
    """Class counts around the 8-lane sub-groups of the fused ranking and the 64-lane stripes of rank_classes_kernel; one rank and
    all of them."""
    shape_case(capi, oracle, [24, 40, L], sorted({1, L}))


# ---- (c) ranking and softmax, directed -------------------------------------------------------------------------------------------
def directed(capi, oracle, layers, Q, nb, wide=False):
    """Modes 2 and 0 against the oracle; returns the reference.  `wide`: the model has more than 512 classes (the 1 024-class route:
    logits through global memory, rank_classes_kernel behind the fused launch)."""
    ref = Ref(oracle, layers, Q)
    for mode in (2, 0):
        idx = handle(capi, layers, mode)
        try:
            plan_l, plan, plan_p = forward(idx, ref, Q.shape[0], nb)
        finally:
            idx.close()
        has(plan, dict(fused=int(mode == 2), logits_lds=int(not wide), rank_kernel=0 if (wide or mode == 0) else -1))
    return ref


def tied_last_layer(seed, hidden, L):
    """A last layer whose rows are drawn from 3 distinct rows, zero bias: at most 3 distinct logits per query."""
    rs = np.random.RandomState(seed)
    rows = (rs.randn(3, hidden) / np.sqrt(hidden)).astype(np.float32)
    return rows[rs.randint(0, 3, L)], np.zeros(L, np.float32)


@pytest.mark.parametrize("L", [70, 1024])
def test_ties_go_to_the_lower_class(capi, oracle, L):
    layers = mlp(31, [24, 40]) + [tied_last_layer(32, 40, L)]
    ref = directed(capi, oracle, layers, queries(33, 77, 24), L, wide=L > 512)
    distinct = [np.unique(bits(r)).size for r in ref.logits]
    assert max(distinct) <= 3 and min(distinct) >= 2, (min(distinct), max(distinct))
    # inside a run of equal logits the classes ascend
    lg = np.take_along_axis(bits(ref.logits), ref.order.astype(np.int64), axis=1)
    assert ((lg[:, 1:] != lg[:, :-1]) | (ref.order[:, 1:] > ref.order[:, :-1])).all()


@pytest.mark.parametrize("L", [70, 1024])
def test_all_equal_logits(capi, oracle, L):
    layers = mlp(34, [24, 40]) + [(np.zeros((L, 40), np.float32), np.zeros(L, np.float32))]
    ref = directed(capi, oracle, layers, queries(35, 77, 24), L, wide=L > 512)
    same_bits(ref.order, np.tile(np.arange(L, dtype=np.int32), (77, 1)))
    assert np.unique(bits(ref.probs)).size == 1 and np.unique(bits(ref.logits)).tolist() == [0]


def test_probabilities_below_the_exponential_cut_are_zero(capi, oracle):
    """Last-layer biases 0, -10, .., -200: a class more than 87 below the row maximum has probability exactly +0."""
    L = 21
    W = (np.random.RandomState(36).randn(L, 40) * 0.01).astype(np.float32)
    layers = mlp(37, [24, 40]) + [(W, (-10.0 * np.arange(L)).astype(np.float32))]
    ref = directed(capi, oracle, layers, queries(38, 77, 24), L)
    zero = bits(ref.probs) == 0
    assert zero[:, 10:].all() and not zero[:, :8].any()
    same_bits(ref.order, np.tile(np.arange(L, dtype=np.int32), (77, 1)))


def test_minus_infinity_logits_rank_last(capi, oracle):
    L = 12
    layers = mlp(39, [24, 40, L])
    layers[-1][1][[3, 7]] = -np.inf
    ref = directed(capi, oracle, layers, queries(40, 77, 24), L)
    same_bits(ref.order[:, -2:], np.tile(np.array([3, 7], np.int32), (77, 1)))
    assert (bits(ref.probs[:, -2:]) == 0).all() and (bits(ref.probs[:, :-2]) != 0).all()


def test_relu_of_minus_zero_is_plus_zero(capi, oracle):
    """Hidden weights and bias all -0, inputs all 1: the hidden chain ends at -0.  The oracle's ReLU (`acc > 0 ? acc : 0`) makes it +0,
    and the next layer (weights 1, bias -0) then gives +0 = 0x00000000; a ReLU that kept -0 would give 0x80000000."""
    d, H, L = 8, 40, 5
    mz = np.float32(-0.0)
    layers = [(np.full((H, d), mz, np.float32), np.full(H, mz, np.float32)), (np.ones((L, H), np.float32), np.full(L, mz, np.float32))]
    assert np.signbit(layers[0][0]).all() and np.signbit(layers[1][1]).all()
    Q = np.ones((33, d), np.float32)
    ref = directed(capi, oracle, layers, Q, L)
    assert np.unique(bits(ref.logits)).tolist() == [0]


def test_nan_feature(capi):
    """The oracle defines no order for NaN logits.  What lmi_hip.h promises: classes -1 and probabilities NaN for that query, the same
    bits from both forms, and the other queries of the batch untouched."""
    layers = mlp(41, [24, 9])
    Q = queries(42, 5, 24)
    clean = {}
    Q[2, 11] = np.nan
    out = {}
    for mode in (2, 0):
        idx = handle(capi, layers, mode)
        try:
            o, l = idx.mlp_topk(Q, 4, want_logits=True)
            p, c = idx.mlp_proba(Q)
            Qc = Q.copy()
            Qc[2, 11] = 0.0
            clean[mode] = (idx.mlp_topk(Qc, 4), *idx.mlp_proba(Qc))
        finally:
            idx.close()
        out[mode] = (o, p, c)
        assert np.isnan(l[2]).all() and not np.isnan(np.delete(l, 2, axis=0)).any()
        assert (o[2] == -1).all() and (c[2] == -1).all() and np.isnan(p[2]).all()
        for got, want in zip((o, p, c), clean[mode]):
            same_bits(np.delete(got, 2, axis=0), np.delete(want, 2, axis=0))
    for a, b in zip(out[2], out[0]):
        same_bits(a, b)


# ---- (d) trees -----------------------------------------------------------------------------------------------------------------
ROOT_DIMS = [20, 96, 5]
NODE_DIMS = [[20, 3], [20, 512, 33, 40], [20, 8, 1], [20, 40, 200, 64, 9]]   # the root's fifth child is a bucket itself


def hetero_tree(scale=2.0):
    """(root, nodes, child_offset, child_model, child_bucket, bucket_paths, entry_paths) of the two-level tree."""
    root = mlp(51, ROOT_DIMS, scale=scale)
    nodes = [mlp(52 + i, dims, scale=scale) for i, dims in enumerate(NODE_DIMS)]
    classes = [ROOT_DIMS[-1]] + [dims[-1] for dims in NODE_DIMS]
    off = np.concatenate([[0], np.cumsum(classes)]).astype(np.int32)
    cm = np.full(off[-1], -1, np.int32)
    cb = np.full(off[-1], -2, np.int32)
    cm[:4] = [1, 2, 3, 4]
    entry_paths = [(j, -1) for j in range(5)]
    bucket_paths, nxt = [(4, -1)], 0
    cb[4] = nxt
    for i, dims in enumerate(NODE_DIMS):
        for j in range(dims[-1]):
            nxt += 1
            cb[off[i + 1] + j] = nxt
            entry_paths.append((i, j))
            bucket_paths.append((i, j))
    return root, nodes, off, cm, cb, bucket_paths, np.array(entry_paths, np.int32)


def tree_handle(capi, root, nodes, off, cm, cb):
    idx = capi.Index(0)
    idx.set_mlp(root)
    for i, layers in enumerate(nodes):
        idx.nav_set_model(i + 1, layers)
    idx.nav_set_tree(off, cm, cb)
    return idx


@pytest.mark.parametrize("mass", [0.0, 0.9])
def test_heterogeneous_tree(capi, oracle, mass):
    """Nodes of one, three and four Linears, 1 to 40 classes and widths 8 to 512 in one launch: the LDS strides are maxima over the
    models and every block reads its logits from its own model's parity."""
    root, nodes, off, cm, cb, bucket_paths, entry_paths = hetero_tree()
    nb, Q = 7, queries(60, 200, 20)
    internal = [((i, -1), layers) for i, layers in enumerate(nodes)]
    tree = path_mass_ref.Tree(oracle, root, internal, bucket_paths, Q, (5, 40))
    full, counts_full = path_mass_ref.walk(tree, nb, 0.0)
    assert (counts_full == nb).all()         # the uncut walk fills every slot of every query
    bo, counts = path_mass_ref.walk(tree, nb, mass)
    if mass:
        path_mass_ref.assert_not_vacuous(counts, nb)
    assert len({int(p[0]) for p in full.reshape(-1, 2)}) == 5   # every root child, so every node model, takes part
    idx = tree_handle(capi, root, nodes, off, cm, cb)
    try:
        idx.set_path_mass(mass)
        slab, ent = idx.nav_order(Q, nb)
        slab2, ent2 = idx.nav_order(Q, nb)
    finally:
        idx.close()
    same_bits(slab2, slab)
    same_bits(ent2, ent)
    # the path rebuilt from the flat child index (child_offset[parent] + class) is the reference's; the slab id is child_bucket's
    got = np.where(ent[:, :, None] >= 0, entry_paths[np.clip(ent, 0, None)], -1)
    same_bits(got.astype(np.int32), bo)
    same_bits(slab, np.where(ent >= 0, cb[np.clip(ent, 0, None)], -1).astype(np.int32))
    assert ((ent >= 0).sum(axis=1) == counts).all()


def test_tree_model_of_another_input_width_is_refused(capi, oracle):
    """Every model of a tree reads the same query rows at the root's width: a node packed for another width would be evaluated on the
    wrong features without a fault.  lmi_nav_set_tree refuses it, naming the model and both widths; replacing the root under a tree
    that was set is refused at the next walk; the handle stays usable."""
    root, nodes, off, cm, cb, _, _ = hetero_tree()
    Q = queries(60, 40, 20)
    good = tree_handle(capi, root, nodes, off, cm, cb)
    idx = tree_handle(capi, root, nodes, off, cm, cb)
    try:
        want = good.nav_order(Q, 7)
        for width in (24, 16):
            idx.nav_set_model(2, mlp(70, [width, 512, 33, 40]))
            with pytest.raises(capi.LmiError, match=rf"lmi_nav_set_tree: model 2 takes {width} input features, the root model 20"):
                idx.nav_set_tree(off, cm, cb)
            with pytest.raises(capi.LmiError, match="no tree"):
                idx.nav_order(Q, 7)
        idx.nav_set_model(2, nodes[1])
        idx.nav_set_tree(off, cm, cb)
        for a, b in zip(idx.nav_order(Q, 7), want):
            same_bits(a, b)
        idx.set_mlp(mlp(71, [24, 96, 5]))    # the root replaced under the tree
        with pytest.raises(capi.LmiError, match=r"lmi_nav_order: model 1 takes 20 input features, the root model 24"):
            idx.nav_order(queries(61, 40, 24), 7)
        idx.set_mlp(root)
        for a, b in zip(idx.nav_order(Q, 7), want):
            same_bits(a, b)
    finally:
        idx.close()
        good.close()


def test_tree_node_with_a_hidden_layer_of_513_is_refused(capi):
    root, nodes, off, cm, cb, _, _ = hetero_tree()
    idx = tree_handle(capi, root, nodes[:1] + [mlp(72, [20, 513, 33, 40])] + nodes[2:], off, cm, cb)
    try:
        with pytest.raises(capi.LmiError, match="does not fit the fused kernel"):
            idx.nav_order(queries(60, 40, 20), 7)
        idx.nav_set_model(2, nodes[1])
        idx.nav_set_tree(off, cm, cb)
        assert (idx.nav_order(queries(60, 40, 20), 7)[1] >= 0).all()
    finally:
        idx.close()


# ---- (e) sequences on one handle ---------------------------------------------------------------------------------------------------
def test_sequences_on_one_handle(capi, oracle):
    """A wide model (1 024 classes), a narrow one, a one-layer one and the wide one again (the descriptors are rebuilt, the LDS strides
    and the logits buffer shrink and grow); modes 2 -> 0 -> 1; a split batch, a small one, a split-sized one with the logits output;
    predict_proba between bucket orders; the mass stop on and off.  Every step equals the oracle and a fresh handle that ran only
    that step, plan included."""
    C = num_cus(capi)
    split = 32 * C + 1
    models = {"wide": [16, 32, 1024], "narrow": [24, 40, 12], "one": [16, 7], "seam": SEAM_DIMS, "peak": [16, 32, 512]}
    layers = {k: (peaked(7, v) if k == "peak" else mlp(80 + i, v)) for i, (k, v) in enumerate(models.items())}
    refs = {k: Ref(oracle, layers[k], queries(90 + i, split if k == "seam" else 200, v[0])) for i, (k, v) in enumerate(models.items())}
    mass_order = stop_mass_ref.expected_order(oracle, layers["peak"], refs["peak"].Q, 6, 0.9)[0][:, :, 0]
    # (model, mode, mass, call, nq, nb, expected plan words)
    steps = [
        ("wide", 2, 0.0, "topk", 77, 5, dict(logits_lds=0, fused=1, rank_kernel=0)),
        ("narrow", 2, 0.0, "topk", 77, 5, dict(logits_lds=1, fused=1, rank_kernel=-1, lds_bytes=lds_bytes([models["narrow"]]))),
        ("one", 2, 0.0, "topk", 33, 7, dict(fused=1, lds_bytes=lds_bytes([models["one"]]))),
        ("wide", 2, 0.0, "proba", 77, 0, dict(logits_lds=0, mode=FM_PROBA, softmax_kernel=1)),
        ("narrow", 0, 0.0, "topk", 77, 5, dict(fused=0, cbw0=1, cbw1=1, rank_kernel=0)),
        ("narrow", 1, 0.0, "topk", 77, 5, dict(fused=0)),
        ("narrow", 2, 0.0, "logits", 200, 12, dict(fused=1, nq_head=200)),
        ("seam", 1, 0.0, "topk", split, 4, dict(fused=1, nq_head=32 * C, layers_queries=1, rank_kernel=0)),
        ("seam", 1, 0.0, "topk", 33, 4, dict(fused=0, layers_queries=33)),
        ("seam", 1, 0.0, "logits", split, 4, dict(fused=1, nq_head=split, layers_queries=0, rank_kernel=-1)),
        ("seam", 1, 0.0, "proba", 77, 0, dict(fused=1, mode=FM_PROBA)),
        ("seam", 1, 0.0, "topk", split, 4, dict(fused=1, nq_head=32 * C, layers_queries=1)),
        ("peak", 2, 0.9, "topk", 200, 6, dict(mode=FM_TOPK_STOP)),
        ("peak", 2, 0.0, "topk", 200, 6, dict(mode=FM_TOPK)),
        ("peak", 0, 0.9, "topk", 200, 6, dict(fused=0, rank_kernel=1)),
        ("wide", 1, 0.0, "logits", 200, 1024, dict(fused=0, logits_lds=0, rank_kernel=0)),
    ]

    def run(idx, step):
        model, _, mass, call, nq, nb, _ = step
        q = np.ascontiguousarray(refs[model].Q[:nq])
        if call == "proba":
            out = idx.mlp_proba(q)
        elif call == "logits":
            out = idx.mlp_topk(q, nb, want_logits=True)
        else:
            out = (idx.mlp_topk(q, nb),)
        return out, idx.debug_last_mlp_plan()

    idx = capi.Index(0)
    state = dict(model=None, mode=1, mass=0.0)
    try:
        for n, step in enumerate(steps):
            model, mode, mass, call, nq, nb, want = step
            if state["model"] != model:
                idx.set_mlp(layers[model])
            if state["mode"] != mode:
                idx.set_fused_mlp(mode)
            if state["mass"] != mass:
                idx.set_stop_mass(mass)
            state = dict(model=model, mode=mode, mass=mass)
            out, plan = run(idx, step)
            print(f"step {n}: {step[:6]}: {plan}")
            has(plan, want)
            fresh = handle(capi, layers[model], mode)
            try:
                fresh.set_stop_mass(mass)
                theirs, their_plan = run(fresh, step)
            finally:
                fresh.close()
            assert their_plan == plan
            for a, b in zip(out, theirs):
                same_bits(a, b, f"step {n}")
            ref = refs[model]
            if call == "proba":
                same_bits(out[0], ref.probs[:nq])
                same_bits(out[1], ref.order[:nq])
            else:
                same_bits(out[0], mass_order[:nq] if mass else ref.order[:nq, :nb])
                if call == "logits":
                    same_bits(out[1], ref.logits[:nq])
    finally:
        idx.close()
