#!/usr/bin/env python3
"""Developer aid (GPU box): random sequences of inserts and deletes on a built index, each step against a fresh build.

  python tools/fuzz_mutate.py [--cases 300 --seed 1]

Every case draws d from the kernels' boundaries (1 .. 2048, 1100: the streamed re-rank), 1 .. 1500 buckets, the prefilter on or off,
the ip or l2 metric, the chunk rows (automatic or 256) and, for a third of the cases, 2 or 3 ranks that own the buckets in turn.
It then runs 4-8 operations: inserts from host arrays or CUDA tensors (empty, spread, one bucket past its capacity, into a bucket
that is or became empty, duplicates of stored ids, rows whose absmax forces a new scale, a trickle of small overflows into many
buckets) and deletes (a random subset with absent and repeated ids, a whole bucket, most of one bucket, everything).  After every
operation the index must equal a fresh build of the equivalent object list (tests/test_gpu_mutate.py's Mirror): the whole
batch's dists, ids and keys byte for byte (ranks: after merge_gathered), bucket_sizes, read_bucket of every bucket, five
queries against the CPU oracle, and the layout invariants of lmi_debug_layout.  one_case returns the handles' layout-path
counters (slack fills, relocations, growth re-packs, hole re-packs) so that the caller can check that every path ran.
tests/test_gpu_mutate_fuzz.py runs the cases (LMI_MUTFUZZ_CASES / LMI_MUTFUZZ_SEED)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

D_CHOICES = [1, 3, 17, 45, 64, 65, 96, 128, 129, 200, 768, 1100, 2048]
L_CHOICES = [1, 2, 7, 40, 300, 1500]
PATHS = ("slack", "relocation", "growth re-pack", "hole re-pack")


class Mismatch(AssertionError):
    pass


def check(cond, what, desc):
    if not cond:
        raise Mismatch(f"{what}: {desc}")


def layout_ok(h, sizes, desc):
    """lmi_debug_layout's tables: buckets inside the layout, disjoint, each with room for its rows; the layout inside the allocations."""
    lay = h.debug_layout()
    st, cap = lay["rb_start"].astype(np.int64), lay["cap_rb"].astype(np.int64)
    L = cap.size
    check(st[L] == lay["n_rb_total"], "rb_start[L] != n_rb_total", desc)
    check(lay["n_rb_total"] <= lay["alloc_rb"], f"n_rb_total {lay['n_rb_total']} > alloc_rb {lay['alloc_rb']}", desc)
    check((cap >= (sizes + 31) // 32).all(), "a bucket's capacity is below its rows", desc)
    check((st >= 0).all() and (st[:L] + cap <= lay["n_rb_total"]).all(), "a bucket outside the layout", desc)
    live = np.flatnonzero(cap > 0)
    o = live[np.argsort(st[live], kind="stable")]
    check((st[o][1:] >= st[o][:-1] + cap[o][:-1]).all(), "buckets overlap", desc)
    return lay["counters"]


def rows_like(rs, n, d, centres, metric, scale=1.0):
    """Rows near random centres: unit norm for ip, norms 0.2 .. 3 for l2 (times `scale`)."""
    X = centres[rs.randint(0, centres.shape[0], n)] * 0.6 + rs.randn(n, d).astype(np.float32)
    X /= np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-20)
    if metric == "l2":
        X *= rs.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    return (X * np.float32(scale)).astype(np.float32)


def one_case(capi, rs, case, oracle=None, verbose=False):
    """Returns (counters i64[4] summed over the case's handles, description)."""
    import torch
    from test_gpu_mutate import Mirror, mlp

    d = int(rs.choice(D_CHOICES))
    L = int(rs.choice(L_CHOICES))
    prefilter = bool(rs.rand() < 0.7)
    metric = "l2" if rs.rand() < 0.3 else "ip"
    chunk = None if rs.rand() < 0.5 else 256
    world = int(rs.choice([2, 3])) if L >= 3 and rs.rand() < 0.3 else 1
    budget = int(3e6 // max(d, 16))                           # rows: keep a case under ~12 MB of f32
    N0 = int(min(budget, rs.choice([0, 40, 600, 3000, 12000]) if L < 300 else rs.choice([600, 3000, 12000])))
    n_ops = int(rs.randint(4, 9))
    desc = dict(case=case, d=d, L=L, prefilter=prefilter, metric=metric, chunk=chunk, world=world, N0=N0, ops=[])
    kw = dict(chunk_rows=chunk, prefilter=prefilter, metric=metric)
    centres = rs.randn(max(1, min(L, 16)), d).astype(np.float32)
    X0 = rows_like(rs, N0, d, centres, metric)
    lab0 = rs.randint(0, L, N0) if rs.rand() < 0.6 else np.minimum(rs.geometric(min(0.9, 3.0 / L), N0) - 1, L - 1)
    next_id = [1]

    def new_ids(n):
        out = np.arange(next_id[0], next_id[0] + n, dtype=np.uint32)
        next_id[0] += n
        return out

    m = Mirror(X0, lab0, new_ids(N0))
    layers = mlp(rs, d, L)
    nq = int(rs.choice([1, 37, 200]))
    Q = rows_like(rs, nq, d, centres, metric)
    nb = int(min(L, rs.choice([1, 2, 3, 5])))
    k = int(rs.choice([1, 5, 10, 20])) if nb > 1 else int(rs.choice([1, 5, 10]))
    k = min(k, 10 * nb)
    owned = [(np.arange(L) % world == r).astype(np.uint8) for r in range(world)]
    hs = []
    for r in range(world):
        h = capi.Index(0, **kw)
        h.set_mlp(layers)
        h.set_buckets(m.X, m.lab, L, ids=m.ids, owned=owned[r] if world > 1 else None)
        hs.append(h)
    dev = torch.device("cuda", 0)

    def insert(X, lab, ids):
        on_dev = X.shape[0] > 0 and rs.rand() < 0.4
        src = torch.from_numpy(X).to(dev) if on_dev else X
        stored = [h.insert(src, lab, ids) for h in hs]
        expect = [int(owned[r][lab].sum()) if world > 1 else lab.size for r in range(world)]
        check(stored == expect, f"stored {stored} != {expect}", desc)
        m.insert(X, lab, ids)
        return "dev" if on_dev else "host"

    def delete(ids):
        n = sum(h.delete(ids) for h in hs)
        check(n == m.delete(ids), "deleted count", desc)

    def scaled_max():
        return float(np.abs(m.X).max()) if m.X.size else 1.0

    for op in range(n_ops):
        sizes = np.bincount(m.lab, minlength=L)
        kind = rs.choice(["spread", "spread", "overflow", "empty_bucket", "dup_ids", "rescale", "trickle",
                          "del_subset", "del_subset", "del_bucket", "del_hard", "del_all"],
                         p=[.12, .08, .14, .08, .06, .06, .12, .12, .06, .06, .07, .03])
        note = str(kind)
        if kind in ("spread", "dup_ids", "rescale"):
            n = int(rs.choice([0, 1, 33, 300, 2000])) if kind == "spread" else int(rs.choice([5, 120, 900]))
            n = min(n, budget // 2)
            X = rows_like(rs, n, d, centres, metric)
            lab = rs.randint(0, L, n)
            ids = new_ids(n)
            if kind == "dup_ids" and m.ids.size:
                ids = m.ids[rs.randint(0, m.ids.size, n)]             # stored twice (or more): a delete takes every copy
            if kind == "rescale":
                X *= np.float32(rs.choice([2.0, 4.5, 64.0]) * scaled_max() / max(float(np.abs(X).max()), 1e-30))
            note += ":" + insert(X, lab, ids)
        elif kind == "overflow":                                     # one bucket, past its capacity (relocation or re-pack)
            b = int(rs.randint(L))
            n = min(int(sizes[b] + rs.randint(1, 3 * sizes[b] + 40)), budget // 2)
            note += f":b{b}+{n}:" + insert(rows_like(rs, n, d, centres, metric), np.full(n, b), new_ids(n))
        elif kind == "empty_bucket":                                 # a bucket that was empty at build time or has been emptied
            empty = np.flatnonzero(sizes == 0)
            b = int(rs.choice(empty)) if empty.size else int(rs.randint(L))
            n = int(rs.choice([1, 31, 32, 33, 400]))
            note += f":b{b}+{n}:" + insert(rows_like(rs, n, d, centres, metric), np.full(n, b), new_ids(n))
        elif kind == "trickle":                                      # small overflows of many buckets, one call each
            for b in rs.permutation(L)[:int(rs.randint(2, 12))]:
                n = int((-sizes[b]) % 32 + 1 + rs.randint(0, 40))   # one row-block more than the bucket holds
                insert(rows_like(rs, n, d, centres, metric), np.full(n, b), new_ids(n))
                sizes = np.bincount(m.lab, minlength=L)
        elif kind == "del_subset":
            sel = m.ids[rs.rand(m.ids.size) < rs.choice([0.02, 0.2, 0.6])]
            absent = np.asarray([next_id[0] + 7, 4_000_000_000], dtype=np.uint32)
            delete(np.concatenate([sel, absent, sel[:5]]))
        elif kind == "del_bucket":
            b = int(rs.choice(np.flatnonzero(sizes))) if sizes.any() else 0
            note += f":b{b}"
            delete(m.ids[m.lab == b])
        elif kind == "del_hard":                                     # most of the largest bucket: holes behind its rows
            b = int(np.argmax(sizes))
            sel = m.ids[m.lab == b]
            note += f":b{b}"
            delete(sel[rs.rand(sel.size) < 0.9])
        else:
            delete(m.ids.copy())
        desc["ops"].append(note)
        if verbose:
            print(" ", note, flush=True)
        compare(capi, hs, m, layers, Q, L, nb, k, kw, world, desc, oracle)
    counters = np.zeros(4, dtype=np.int64)
    for h in hs:
        counters += layout_ok(h, h.bucket_sizes(), desc)
        h.close()
    return counters, desc


def compare(capi, hs, m, layers, Q, L, nb, k, kw, world, desc, oracle):
    sizes = np.bincount(m.lab, minlength=L)
    got_sizes = sum(h.bucket_sizes() for h in hs)
    check(np.array_equal(got_sizes, sizes), "bucket_sizes", desc)
    for h in hs:
        layout_ok(h, h.bucket_sizes(), desc)
    for b in range(L):                                               # every bucket's rows and ids, in the equivalent order
        sel = m.lab == b
        h = hs[b % world]
        rows, ids = h.read_bucket(b)
        check(np.array_equal(rows, m.X[sel]) and np.array_equal(ids, m.ids[sel]), f"read_bucket({b})", desc)
    if world == 1:
        d1, i1, _, k1 = hs[0].search(Q, Q, nb, k, want_keys=True)
    else:
        outs = [h.search(Q, Q, nb, k, want_keys=True) for h in hs]
        kout = outs[0][0].shape[1]
        gd = np.ascontiguousarray(np.stack([o[0] for o in outs]))
        gi = np.ascontiguousarray(np.stack([o[1] for o in outs]))
        gk = np.ascontiguousarray(np.stack([o[3] for o in outs]))
        d1 = np.empty((Q.shape[0], kout), np.float32)
        i1 = np.empty((Q.shape[0], kout), np.uint32)
        hs[0].merge_gathered(gd, gi, gk, world, Q.shape[0], kout, d1, i1)
        k1 = None
    if m.lab.size:                                                   # (a fresh build of no objects is not this test's business)
        ref = capi.Index(0, **kw)
        ref.set_mlp(layers)
        ref.set_buckets(m.X, m.lab, L, ids=m.ids)
        d2, i2, _, k2 = ref.search(Q, Q, nb, k, want_keys=True)
        ref.close()
        check(np.array_equal(i1, i2), "ids vs the fresh build", desc)
        check(np.array_equal(d1.view(np.uint32), d2.view(np.uint32)), "dists vs the fresh build", desc)
        check(k1 is None or np.array_equal(k1, k2), "keys vs the fresh build", desc)
    if oracle is not None and k <= 2 * capi.K_PER_BUCKET:
        sub = np.arange(min(5, Q.shape[0]))
        do, no, _ = oracle.search(layers, Q[sub], m.X, Q[sub], m.lab, nb, k, ids=m.ids, nthreads=8, metric=kw["metric"])
        check(np.array_equal(i1[sub], no) and np.array_equal(d1[sub].astype(np.float64), do), "the oracle", desc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--oracle", action="store_true", help="five queries per step against the CPU oracle as well")
    a = ap.parse_args()
    from learnedmetricindex_amd import _capi

    oracle = None
    if a.oracle:
        from oracle import lmi_oracle as oracle

        oracle.build()
    t0 = time.time()
    total = np.zeros(4, dtype=np.int64)
    for case in range(a.cases):
        try:
            c, desc = one_case(_capi, np.random.RandomState(a.seed * 100003 + case), case, oracle)
        except Mismatch as e:
            print("MISMATCH", e, flush=True)
            sys.exit(1)
        total += c
        if case % 10 == 0:
            print(f"case {case}: ok {desc} ({time.time() - t0:.0f} s)", flush=True)
    print(f"{a.cases} cases equal to fresh builds ({time.time() - t0:.0f} s); layout paths:",
          ", ".join(f"{p} {n}" for p, n in zip(PATHS, total)))


if __name__ == "__main__":
    main()
