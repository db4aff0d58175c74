"""GPU (`-m gpu`): the scan's dispatch seams.  scan_plan() (lmi_host_scan.h) and the launch sites pick one of about a dozen kernel
forms from a call's shape; here every threshold between two forms has one case on each side, and every case

  1. asserts, from `debug_last_plan()` after the scan, the plan words the case is about -- the expected values stand in the case
     table next to the shape (and `debug_plan()`, which launches nothing, must have said the same);
  2. compares the whole batch on the prefilter handle with an all-f32 handle (`prefilter=False`) of the same rows: ids, distance
     bits and keys, and a second call on each handle with the first;
  3. checks the first 32 and the last 32 queries of the batch (the highest slot numbers) against the CPU oracle, ids and distances.

Then sequences of calls on ONE handle that cross the seams in both directions: the two fronts initialise different things, the
workspaces only grow and are not re-zeroed, the overflow machinery stays armed for 1 000 calls -- every step must equal the all-f32
twin and a fresh handle that ran only that call.

Where the thresholds come from (the headers; `dp` = d rounded up to 4, f16 storage: to 8):
  fused front          L <= 512, nq x nb <= 2^17, d <= 2048                                    (lmi_front.h FR_MAX_*)
  route sort           in LDS for L <= 8000                                                    (lmi_kernels.h ROUTE_MAX_BUCKETS)
  streamed re-rank     8192 + 4 dp + 256 <= 65536: dp <= 14272                                 (rc_wave_lds, small form, ONE wave)
  small form, 4 waves  4 (8192 + 4 dp + 256) <= 65536: dp <= 1984; beyond, one wave per block  (rescore_small_waves)
  fused tail           rup16(8448 + 4 dp) + 160 G <= 16384: dp <= 1824 / 1864 / 1904 / 1944 for G = 4 / 3 / 2 / 1
  route_kernel<NB>     NB in {1, 2, 3, 4, 5, 6, 8, 10, 16}, else the generic instance <0>
  pack_kernel<GS, CP>  ceil(d / 8) <= 8 / 16 / 32 / 64 / 128 / more: <8,1> <16,1> <32,1> <64,1> <64,2> <64,4>; vec: d % 8 == 0
  final merge          n_buckets <= 4: the fused tail; <= 16: merge_ranks_kernel; more: merge_kernel
  qbound               n_buckets > 1 and k <= 10;  sample_max 8 for KG16 <= 4 (d <= 64), else 16;  low_d for KG16 <= 8 (d <= 128)
"""
import os

import numpy as np
import pytest

from test_gpu_front import make
from test_gpu_tail import dup_data, ordinary_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def q16(a):
    return a.astype(np.float16).astype(np.float32)


def handle(capi, env=None, **kw):
    """A handle created with `env` in the environment (the library reads its switches there, at creation only)."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.Index(0, chunk_rows=256, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def scan(idx, Q, order, k):
    d, i, keys = idx.scan_topk(Q, order, k, want_keys=True)
    return d.view(np.uint32), i, keys


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


_data, _ref = {}, {}


def data(spec, nb, f16=False):
    """make() of test_gpu_front.py, once per shape and read-only.  spec = (seed, N, d, L, nq, options)."""
    key = (spec, nb, f16)
    if key not in _data:
        _data.clear()   # (one shape at a time: the wide ones are tens of MB)
        seed, N, d, L, nq, kw = spec
        X, lab, Q, order = make(seed, N, d, L, nq, nb, **dict(kw))
        if f16:
            X, Q = q16(X), q16(Q)
        for a in (X, lab, Q, order):
            a.setflags(write=False)
        _data[key] = (X, lab, Q, order)
    return _data[key]


def ends(a):
    return np.concatenate([a[:32], a[-32:]])


def oracle_search(oracle, X, Q, lab, order, k, metric):
    """oracle.search(..., bucket_order=order).  It restates the reference's rank merge, shape assertion included, which cannot hold
    before the ranks merged so far hold k results: for k > 20 the same per-rank oracle search and the same stable merge run here,
    over all ranks at once (a stable sort of the ranks' lists in rank order is what the rank-by-rank merge arrives at: truncating to
    k after each rank drops nothing that a later, larger list would have kept)."""
    nb = order.shape[1]
    if k <= 20 or nb == 1:
        do, io, _ = oracle.search(None, None, X, Q, lab, nb, k, nthreads=4, bucket_order=order[:, :, None], metric=metric)
        return do, io
    groups = oracle.group_buckets(np.asarray(lab)[:, None])
    ids = np.arange(1, X.shape[0] + 1, dtype=np.int64)
    per_rank = [oracle.search_single_bucket(X, ids, groups, Q, order[:, r, None], 4, metric) for r in range(nb)]
    dists, anns = np.hstack([p[0] for p in per_rank]), np.hstack([p[1] for p in per_rank])
    pick = dists.argsort(kind="stable", axis=1)[:, :k]
    return np.take_along_axis(dists, pick, axis=1), np.take_along_axis(anns, pick, axis=1)


def reference(capi, oracle, spec, nb, k, metric="ip", f16=False):
    """The all-f32 handle's answer for the whole batch (scanned twice) and the oracle's for its first and last 32 queries: computed
    once per (shape, n_buckets, k) and shared by the cases that differ in the prefilter handle's switches only."""
    key = (spec, nb, k, metric, f16)
    if key not in _ref:
        X, lab, Q, order = data(spec, nb, f16)
        L = spec[3]
        twin = handle(capi, prefilter=False, metric=metric)
        twin.set_buckets(X, lab, L)
        out = scan(twin, Q, order, k)
        same(out, scan(twin, Q, order, k))
        assert twin.debug_last_plan()["fast"] == 0
        twin.close()
        do, io = oracle_search(oracle, X, ends(Q), lab, ends(order), k, metric)
        for a in out:
            a.setflags(write=False)
        _ref[key] = (out, do.astype(np.float32), io)
    return _ref[key]


def check(capi, oracle, spec, nb, k, expect, env=None, metric="ip", storage="f32"):
    f16 = storage == "f16"
    X, lab, Q, order = data(spec, nb, f16)
    L, nq = spec[3], spec[4]
    assert nq >= 64
    idx = handle(capi, env, metric=metric, storage=storage)
    try:
        idx.set_buckets(X, lab, L)
        said = idx.debug_plan(nq, nb, k)
        out = scan(idx, Q, order, k)
        plan = idx.debug_last_plan()
        print(f"plan: nq {nq} nb {nb} k {k} d {spec[2]} L {L} {metric} {storage} {env or ''}: {plan}")
        same(out, scan(idx, Q, order, k))
        assert idx.debug_last_plan() == plan
    finally:
        idx.close()
    # 1. the form the case is about ran, and the dry report agrees with the record word for word
    assert plan["fast"] == 1, plan
    assert {f: plan[f] for f in expect} == expect, plan
    assert {f: v for f, v in said.items() if f != "overflow_sorted"} == {f: v for f, v in plan.items() if f != "overflow_sorted"}
    # 2. the all-f32 handle, the whole batch
    ref, do, io = reference(capi, oracle, spec, nb, k, metric, f16)
    same(out, ref)
    # 3. the oracle, the first and the last 32 queries
    np.testing.assert_array_equal(ends(out[1]), io)
    np.testing.assert_array_equal(ends(out[0]).view(np.float32), do)


MESSY = (("empty", (1,)), ("invalid_frac", 0.03), ("repeat_frac", 0.1))   # make()'s options: about half the cases switch them on
CLEAN = ()

# ---- one case on each side of every seam: (id, (seed, N, d, L, nq, options), nb, k, expected plan words[, handle settings]) ----
SLOTS = (51, 20_000, 32, 8)
WIDE = (52, 3_000)
SEAMS = [
    # slots: nq x nb = 2^17 is the last fused front
    ("slots_nb4_32768", SLOTS + (32_768, CLEAN), 4, 10, dict(use_front=1, route_sort_global=-1)),
    ("slots_nb4_32769", SLOTS + (32_769, CLEAN), 4, 10, dict(use_front=0, route_nb_template=-1, pack_gs=-1)),
    ("slots_nb2_65536", SLOTS + (65_536, MESSY), 2, 10, dict(use_front=1)),
    ("slots_nb2_65537", SLOTS + (65_537, MESSY), 2, 10, dict(use_front=0)),
    # buckets: 512 / 513 the fused front, 8000 / 8001 the route sort in LDS / in global memory
    ("L512", (53, 20_000, 24, 512, 600, MESSY), 3, 10, dict(use_front=1, route_sort_global=-1)),
    ("L513", (53, 20_000, 24, 513, 600, MESSY), 3, 10, dict(use_front=0, route_sort_global=0)),
    ("L8000", (54, 20_000, 24, 8000, 600, CLEAN), 3, 10, dict(use_front=0, route_sort_global=0)),
    ("L8001", (54, 20_000, 24, 8001, 600, CLEAN), 3, 10, dict(use_front=0, route_sort_global=1)),
    # width, front
    ("d2048", WIDE + (2048, 4, 96, CLEAN), 2, 10, dict(use_front=1, pack_gs=64, pack_cp=4, pack_vec=1)),
    ("d2049", WIDE + (2049, 4, 96, CLEAN), 2, 10, dict(use_front=0, pack_gs=-1)),
    # width, the streamed re-rank's small form: four waves per block up to dp = 1984, one beyond (both streamed, neither fused)
    ("d1984", WIDE + (1984, 4, 96, MESSY), 4, 10, dict(streamed=1, use_tail=0, rescore_small_waves=4)),
    ("d1988", WIDE + (1988, 4, 96, MESSY), 4, 10, dict(streamed=1, use_tail=0, rescore_small_waves=1)),
    # width, streamed re-rank | select_rescore_kernel
    ("d14272", (55, 1_200, 14_272, 4, 64, CLEAN), 2, 10, dict(streamed=1, use_tail=0, rescore_small_waves=1)),
    ("d14276", (55, 1_200, 14_276, 4, 64, CLEAN), 2, 10, dict(streamed=0, use_tail=0, rescore_small_waves=-1)),
    # width, the fused tail, f32 storage: the last fused dp per group size and the next one
    ("tail_d1824_nb4", WIDE + (1824, 4, 96, CLEAN), 4, 10, dict(use_tail=1, tail_merges=1, G=4, dp=1824, merge_kind=0)),
    ("tail_d1828_nb4", WIDE + (1828, 4, 96, CLEAN), 4, 10, dict(use_tail=0, tail_merges=0, G=4, dp=1828, merge_kind=1)),
    ("tail_d1864_nb3", WIDE + (1864, 4, 96, MESSY), 3, 10, dict(use_tail=1, G=3, dp=1864, merge_kind=0)),
    ("tail_d1868_nb3", WIDE + (1868, 4, 96, MESSY), 3, 10, dict(use_tail=0, G=3, dp=1868, merge_kind=1)),
    ("tail_d1904_nb2", WIDE + (1904, 4, 96, CLEAN), 2, 10, dict(use_tail=1, G=2, dp=1904, merge_kind=0)),
    ("tail_d1908_nb2", WIDE + (1908, 4, 96, CLEAN), 2, 10, dict(use_tail=0, G=2, dp=1908, merge_kind=1)),
    ("tail_d1944_nb1", WIDE + (1944, 4, 96, MESSY), 1, 10, dict(use_tail=1, G=1, dp=1944, merge_kind=0)),
    ("tail_d1948_nb1", WIDE + (1948, 4, 96, MESSY), 1, 10, dict(use_tail=0, G=1, dp=1948, merge_kind=1)),
    # ... f16 storage: dp is d rounded up to 8
    ("tail16_d1824_nb4", WIDE + (1824, 4, 96, MESSY), 4, 10, dict(use_tail=1, G=4, dp=1824), dict(storage="f16")),
    ("tail16_d1832_nb4", WIDE + (1832, 4, 96, MESSY), 4, 10, dict(use_tail=0, G=4, dp=1832), dict(storage="f16")),
    ("tail16_d1944_nb1", WIDE + (1944, 4, 96, CLEAN), 1, 10, dict(use_tail=1, G=1, dp=1944), dict(storage="f16")),
    ("tail16_d1952_nb1", WIDE + (1952, 4, 96, CLEAN), 1, 10, dict(use_tail=0, G=1, dp=1952), dict(storage="f16")),
    # plan switches.  qbound: k = 10 / 11 at four buckets, one / two buckets at k = 10
    ("qbound_k10_nb4", (56, 20_000, 48, 16, 300, MESSY), 4, 10, dict(qbound=1, primary_nb=4)),
    ("qbound_k11_nb4", (56, 20_000, 48, 16, 300, MESSY), 4, 11, dict(qbound=0, primary_nb=0)),
    ("qbound_k10_nb1", (56, 20_000, 48, 16, 300, MESSY), 1, 10, dict(qbound=0, primary_nb=0)),
    ("qbound_k10_nb2", (56, 20_000, 48, 16, 300, MESSY), 2, 10, dict(qbound=1, primary_nb=2)),
    # k at the cap, eight buckets (the five launches + merge_ranks_kernel)
    ("k10_nb8", (57, 20_000, 48, 16, 300, CLEAN), 8, 10, dict(qbound=1, use_tail=0, merge_kind=1)),
    ("k11_nb8", (57, 20_000, 48, 16, 300, CLEAN), 8, 11, dict(qbound=0, use_tail=0, merge_kind=1)),
    ("k64_nb8", (57, 20_000, 48, 16, 300, CLEAN), 8, 64, dict(qbound=0, use_tail=0, merge_kind=1)),
    # sample_max: KG16 4 / 5
    ("sample_d64", (58, 20_000, 64, 16, 300, CLEAN), 4, 10, dict(sample_max=8, KG16=4, low_d=1)),
    ("sample_d65", (58, 20_000, 65, 16, 300, CLEAN), 4, 10, dict(sample_max=16, KG16=5, low_d=1)),
    # low_d: KG16 8 / the general kernels (their K is padded to 32: KG16 10); the L2 metric stores one more column
    ("lowd_ip_d128", (59, 20_000, 128, 16, 300, MESSY), 4, 10, dict(low_d=1, KG16=8, tile_cb=6)),
    ("lowd_ip_d129", (59, 20_000, 129, 16, 300, MESSY), 4, 10, dict(low_d=0, KG16=10, tile_cb=12)),
    ("lowd_l2_d127", (60, 20_000, 127, 16, 300, CLEAN), 4, 10, dict(low_d=1, KG16=8, dp=128), dict(metric="l2")),
    ("lowd_l2_d128", (60, 20_000, 128, 16, 300, CLEAN), 4, 10, dict(low_d=0, KG16=10, dp=132), dict(metric="l2")),
    # ... and every width seam above: the plan decides on the STORED width rup(d + 1, 4), so under L2 each threshold falls one user
    # column earlier (the expectations are the rules of this file's docstring applied to that width)
    ("front_l2_d2047", WIDE + (2047, 4, 96, CLEAN), 2, 10, dict(use_front=1, dp=2048), dict(metric="l2")),
    ("front_l2_d2048", WIDE + (2048, 4, 96, CLEAN), 2, 10, dict(use_front=0, dp=2052), dict(metric="l2")),
    ("tail_l2_d1823_nb4", WIDE + (1823, 4, 96, MESSY), 4, 10, dict(use_tail=1, G=4, dp=1824), dict(metric="l2")),
    ("tail_l2_d1824_nb4", WIDE + (1824, 4, 96, MESSY), 4, 10, dict(use_tail=0, G=4, dp=1828), dict(metric="l2")),
    ("tail_l2_d1943_nb1", WIDE + (1943, 4, 96, CLEAN), 1, 10, dict(use_tail=1, G=1, dp=1944), dict(metric="l2")),
    ("tail_l2_d1944_nb1", WIDE + (1944, 4, 96, CLEAN), 1, 10, dict(use_tail=0, G=1, dp=1948), dict(metric="l2")),
    ("waves_l2_d1983", WIDE + (1983, 4, 96, MESSY), 4, 10, dict(streamed=1, use_tail=0, rescore_small_waves=4, dp=1984), dict(metric="l2")),
    ("waves_l2_d1984", WIDE + (1984, 4, 96, MESSY), 4, 10, dict(streamed=1, use_tail=0, rescore_small_waves=1, dp=1988), dict(metric="l2")),
]


@pytest.mark.parametrize("case", SEAMS, ids=[c[0] for c in SEAMS])
def test_seam(capi, oracle, case):
    _, spec, nb, k, expect = case[:5]
    opt = case[5] if len(case) > 5 else {}
    check(capi, oracle, spec, nb, k, expect, **opt)
    if k == 64:
        assert reference(capi, oracle, spec, nb, k)[0][1].shape == (spec[4], 64)


# pack_kernel's forms, the fused front against LMI_FRONT=0: both sides of each of its five switches, both `vec` values at three of them
PACK = [(64, 8, 1, 1), (65, 16, 1, 0), (128, 16, 1, 1), (129, 32, 1, 0), (256, 32, 1, 1), (257, 64, 1, 0), (384, 64, 1, 1), (512, 64, 1, 1),
        (513, 64, 2, 0), (1024, 64, 2, 1), (1025, 64, 4, 0)]


@pytest.mark.parametrize("d,gs,cp,vec", PACK, ids=[f"d{p[0]}" for p in PACK])
def test_pack_forms(capi, oracle, d, gs, cp, vec):
    spec = (61, 6_000, d, 7, 200, MESSY if d % 2 else CLEAN)
    check(capi, oracle, spec, 3, 10, dict(use_front=1, route_nb_template=3, pack_gs=gs, pack_cp=cp, pack_vec=vec))
    check(capi, oracle, spec, 3, 10, dict(use_front=0, route_nb_template=-1, pack_gs=-1, pack_cp=-1, pack_vec=-1, route_sort_global=0),
          env={"LMI_FRONT": "0"})


# route_kernel's rank-count template, the re-rank's group size and the final merge: (nb, NB template, G, merge kind)
RANKS = [(7, 0, 1, 1), (9, 0, 3, 1), (12, 0, 4, 1), (16, 16, 4, 1), (17, 0, 1, 2)]


RANK_CASES = [r + (front, tail) for r in RANKS for front in ("1", "0") for tail in ("0", "2") if r[0] <= 16 or tail == "0"]


@pytest.mark.parametrize("nb,nbt,G,kind,front,tail", RANK_CASES, ids=[f"nb{r[0]}_front{r[4]}_tail{r[5]}" for r in RANK_CASES])
def test_rank_counts(capi, oracle, nb, nbt, G, kind, front, tail):
    """One index (d = 96, L = 20); LMI_TAIL=2 runs tail_kernel group-wise (a wave per G slots) in front of the same merge.  Seventeen
    buckets, past merge_ranks_kernel, run with the five launches only."""
    spec = (62, 30_000, 96, 20, 400, MESSY)
    expect = dict(use_front=int(front), route_nb_template=nbt if front == "1" else -1, G=G, merge_kind=kind,
                  use_tail=int(tail == "2"), tail_merges=0)
    check(capi, oracle, spec, nb, 10, expect, env={"LMI_FRONT": front, "LMI_TAIL": tail})


@pytest.mark.parametrize("side", [0, 1], ids=["narrow", "wide"])
def test_ps_wide(capi, oracle, side):
    """The low-dimensional kernels' wide form is taken from the batch's queries per non-empty bucket: the two batch sizes on either side of
    ps_use_wide are found with debug_plan() on the built handle (K = 128: KG16 = 8 has a wide form)."""
    base = (63, 20_000, 128, 16)
    X, lab, _, _ = data(base + (64, CLEAN), 4)
    idx = handle(capi)
    idx.set_buckets(X, lab, 16)
    lo, hi = 64, 1 << 14
    assert idx.debug_plan(lo, 4)["ps_wide"] == 0 and idx.debug_plan(hi, 4)["ps_wide"] == 1
    while hi - lo > 1:   # ps_wide is monotone in nq
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if idx.debug_plan(mid, 4)["ps_wide"] else (mid, hi)
    idx.close()
    print(f"ps_wide: narrow up to nq = {lo}, wide from {hi}")
    nq = (lo, hi)[side]
    check(capi, oracle, base + (nq, CLEAN), 4, 10, dict(ps_wide=side, low_d=1, KG16=8, tile_cb=12 if side else 6))


def test_debug_plan_checks_like_a_scan_and_launches_nothing(capi):
    """debug_plan() refuses what scan_topk refuses, with the same words behind its own name, and leaves the handle's record alone."""
    X, lab, Q, order = data((64, 4_000, 40, 6, 64, CLEAN), 2)
    idx = handle(capi)
    try:
        with pytest.raises(capi.LmiError, match="not built"):
            idx.debug_plan(10, 2, 10)
        idx.set_buckets(X, lab, 6)
        assert set(idx.debug_last_plan().values()) == {0}   # no scan yet
        for nq, nb, k, why in ((10, 0, 10, "bad nq/n_buckets"), (-1, 2, 10, "bad nq/n_buckets"), (1 << 30, 2, 10, "too large")):
            with pytest.raises(capi.LmiError, match=why):
                idx.debug_plan(nq, nb, k)
        for nb, k, why in ((1025, 10, "exceeds 1024"), (2, 65, "outside"), (2, 0, "outside"), (2, 21, "exceeds n_buckets")):
            with pytest.raises(capi.LmiError, match=why) as mine:
                idx.debug_plan(8, nb, k)
            with pytest.raises(capi.LmiError, match=why) as scans:
                idx.scan_topk(np.zeros((8, 40), np.float32), np.zeros((8, nb), np.int32), k)
            assert str(mine.value).replace("lmi_debug_plan", "lmi_scan_topk") == str(scans.value)
        assert set(idx.debug_last_plan().values()) == {0}   # a refused scan records nothing
        scan(idx, Q, order, 10)
        plan = idx.debug_last_plan()
        assert idx.debug_plan(1 << 20, 3, 11)["use_front"] == 0 and idx.debug_plan(0, 2, 10)["fast"] == 1
        assert idx.debug_last_plan() == plan
    finally:
        idx.close()


# ---- sequences on one handle ----
def plan_has(plan, want):
    assert {f: plan[f] for f in want} == want, (want, plan)


def run_sequence(capi, X, lab, L, steps, batches):
    """steps: (batch name, nq, nb, k, emit_all, expected plan words).  Each step runs on the long-lived prefilter handle, on the all-f32
    twin and on a fresh prefilter handle that runs nothing else."""
    idx, twin = handle(capi), handle(capi, prefilter=False)
    idx.set_buckets(X, lab, L)
    twin.set_buckets(X, lab, L)
    emit = False
    try:
        for n, (name, nq, nb, k, emit_all, want) in enumerate(steps):
            Q, order = batches[name]
            Q, order = np.ascontiguousarray(Q[:nq]), np.ascontiguousarray(order[:nq, :nb])
            if emit_all != emit:
                idx.debug_emit_all(emit_all)
                emit = emit_all
            out = scan(idx, Q, order, k)
            plan = idx.debug_last_plan()
            print(f"step {n}: {name} nq {nq} nb {nb} k {k} emit_all {int(emit_all)}: {plan}")
            plan_has(plan, want)
            same(out, scan(twin, Q, order, k))
            fresh = handle(capi)
            try:
                fresh.set_buckets(X, lab, L)
                fresh.debug_emit_all(emit_all)
                same(out, scan(fresh, Q, order, k))
                theirs = fresh.debug_last_plan()
            finally:
                fresh.close()
            # the same plan; only the overflow machinery depends on what the handle has seen
            assert {f: v for f, v in theirs.items() if f != "overflow_sorted"} == {f: v for f, v in plan.items() if f != "overflow_sorted"}
    finally:
        idx.close()
        twin.close()


def test_sequence_crosses_the_seams_on_one_handle(capi):
    """use_front 1 -> 0 -> 1; a large batch and then a much smaller one (stale columns beyond ncols); the tail merging, five launches,
    merging; qbound on, off, on; a single unmerged rank between merged calls; debug_emit_all on and off."""
    X, lab, Q, order = make(71, 20_000, 64, 16, 32_769, 8, invalid_frac=0.03, repeat_frac=0.1)
    front = dict(use_front=1, use_tail=1, tail_merges=1, qbound=1, merge_kind=0)
    steps = [
        ("a", 300, 4, 10, False, front),
        ("a", 32_769, 4, 10, False, dict(use_front=0, use_tail=1, tail_merges=1, qbound=1)),
        ("a", 300, 4, 10, False, front),
        ("a", 40, 4, 10, False, front),
        ("a", 300, 8, 10, False, dict(use_front=1, use_tail=0, tail_merges=0, qbound=1, merge_kind=1, G=4)),
        ("a", 300, 4, 10, False, front),
        ("a", 300, 4, 11, False, dict(use_front=1, use_tail=1, tail_merges=1, qbound=0, primary_nb=0)),
        ("a", 300, 4, 10, False, front),
        ("a", 300, 1, 10, False, dict(use_front=1, use_tail=1, tail_merges=1, qbound=0, G=1, merge_kind=0)),
        ("a", 300, 4, 10, False, front),
        ("a", 32_769, 4, 10, False, dict(use_front=0)),
        ("a", 300, 8, 11, False, dict(use_front=1, use_tail=0, qbound=0, merge_kind=1)),
        ("a", 300, 4, 10, True, front),
        ("a", 300, 4, 10, False, front),
    ]
    run_sequence(capi, X, lab, 16, steps, {"a": (Q, order)})


def test_sequence_arms_the_overflow_machinery(capi):
    """Ordinary batch, overflow batch, ordinary, overflow: the fused tail's sequence takes overflow_rebound_kernel + pass 2's redo launch
    in from the call AFTER the first batch that logged candidates, and every call equals the all-f32 twin."""
    X, lab, L, Qo, oo = dup_data(9, 64, 1500, 3, 0.0)
    Qn, on = ordinary_batch(42, X, lab, L, 1500, 3, 300)
    idx, twin = capi.Index(0, chunk_rows=2048), capi.Index(0, chunk_rows=2048, prefilter=False)
    idx.set_buckets(X, lab, L)
    twin.set_buckets(X, lab, L)
    seen, logged = [], []
    try:
        for Q, order in ((Qn, on), (Qo, oo), (Qn, on), (Qo, oo)):
            out = scan(idx, Q, order, 10)
            plan = idx.debug_last_plan()
            plan_has(plan, dict(use_tail=1, tail_merges=1))
            seen.append(plan["overflow_sorted"])
            logged.append(int(idx.debug_peek("pf_fallback", 32).view(np.uint32)[3]))
            same(out, scan(twin, Q, order, 10))
    finally:
        idx.close()
        twin.close()
    assert seen == [0, 0, 1, 1], seen
    assert logged[0] == 0 and logged[1] > 0 and logged[2] == 0 and logged[3] > 0, logged
