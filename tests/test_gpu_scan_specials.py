"""GPU (`-m gpu`): NaN, +-inf, subnormal and overflowing values through lmi_scan_topk -- the contract paragraph at lmi_scan_topk in
include/lmi_hip.h.  For every case of scan_special_cases.py (d = 48 and 160: both pass-2 kernel families; both metrics) a prefilter
handle and an all-f32 handle each scan the batch twice: the four results are equal in ids, distance bits and keys, and equal the CPU
oracle for all 64 queries.  Each case runs with the fused front and with LMI_FRONT=0 (the two fronts compute a query's scale in
different kernels).  The stored-side cases also run through a mutation: built without the special rows, which are then inserted
(lmi_mutate.h folds their norms into the bucket's with its own atomicMax form) -- the search equals a fresh build's and the oracle's."""
import numpy as np
import pytest

import scan_special_cases as sc
from test_gpu_seams import handle, same, scan

pytestmark = pytest.mark.gpu

IDS = [f"{n}-d{d}-{m}" for n, d, m in sc.CASES]


@pytest.fixture(scope="module")
def capi():
    from learnedmetricindex_amd import _capi

    _capi.lib()
    return _capi


def check_oracle(out, do, io):
    np.testing.assert_array_equal(out[1], io)
    np.testing.assert_array_equal(out[0].view(np.float32).astype(np.float64), do)


@pytest.mark.parametrize("front", ["1", "0"], ids=["fused_front", "front0"])
@pytest.mark.parametrize("name,d,metric", sc.CASES, ids=IDS)
def test_special_values_through_the_scan(capi, oracle, name, d, metric, front):
    c = sc.case(name, d, metric)
    do, io = sc.truth(oracle, name, d, metric)
    outs = []
    for pf in (True, False):
        idx = handle(capi, {"LMI_FRONT": front}, prefilter=pf, metric=metric)
        try:
            idx.set_buckets(c.X, c.labels, sc.L)
            outs.append(scan(idx, c.Q, c.order, sc.K))
            outs.append(scan(idx, c.Q, c.order, sc.K))
            plan = idx.debug_last_plan()
            assert plan["fast"] == int(pf) and (not pf or plan["use_front"] == int(front)), plan
            if pf:
                print(f"[specials] {name} d={d} {metric} front={front}: fallback slots {idx.prefilter_stats()[2]}")
        finally:
            idx.close()
    check_oracle(outs[2], do, io)     # the all-f32 scan is the oracle's
    for o in outs[:2] + outs[3:]:
        same(o, outs[2])
    check_oracle(outs[0], do, io)


STORED_CASES = [c for c in sc.CASES if c[0] in sc.STORED]


@pytest.mark.parametrize("name,d,metric", STORED_CASES, ids=[f"{n}-d{d}-{m}" for n, d, m in STORED_CASES])
def test_special_rows_inserted_equal_a_fresh_build(capi, oracle, name, d, metric):
    c = sc.case(name, d, metric)
    (Xk, lk, ik), (Xs, ls, is_) = sc.split(c)
    X, lab, ids = np.concatenate([Xk, Xs]), np.concatenate([lk, ls]), np.concatenate([ik, is_])
    do, io = sc.search(oracle, X, c.Q, lab, c.order, metric, ids=ids)
    outs = []
    for mutate in (True, False):
        idx = handle(capi, prefilter=True, metric=metric)
        try:
            if mutate:
                idx.set_buckets(Xk, lk, sc.L, ids=ik)
                assert idx.insert(Xs, ls, is_) == Xs.shape[0]
            else:
                idx.set_buckets(X, lab, sc.L, ids=ids)
            outs.append(scan(idx, c.Q, c.order, sc.K))
            outs.append(scan(idx, c.Q, c.order, sc.K))
        finally:
            idx.close()
    for o in outs[1:]:
        same(o, outs[0])
    check_oracle(outs[0], do, io)
