"""GPU (`-m gpu`): random insert / delete sequences, every step against a fresh build of the equivalent object list
(tools/fuzz_mutate.py draws the cases: d 1 .. 2048 at the kernels' boundaries, 1 .. 1500 buckets, prefilter on / off, ip / l2,
automatic or 256-row chunks, 1 .. 3 owned ranks merged with merge_gathered; 4-8 operations of inserts from host or device rows,
empty, into one bucket past its capacity, into empty buckets, with stored ids, with a new absmax, and deletes of subsets, whole
buckets, most of a bucket or everything).  Compared after every operation: the batch's dists / ids / keys byte for byte,
bucket_sizes, read_bucket of every bucket, five queries against the CPU oracle and the layout invariants of lmi_debug_layout.
The layout paths the inserts took (slack, relocation, growth re-pack, hole re-pack) are summed over the run: each must have run
a few times, or the generator has a blind spot.  300 cases here, about a minute (LMI_MUTFUZZ_CASES / LMI_MUTFUZZ_SEED for more)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_random_insert_delete_sequences_equal_fresh_builds(oracle):
    from fuzz_mutate import PATHS, one_case
    from learnedmetricindex_amd import _capi

    seed = int(os.environ.get("LMI_MUTFUZZ_SEED", "2026"))
    cases = int(os.environ.get("LMI_MUTFUZZ_CASES", "300"))
    total = np.zeros(4, dtype=np.int64)
    for case in range(cases):
        counters, _ = one_case(_capi, np.random.RandomState(seed * 100003 + case), case, oracle)
        total += counters
    print(f"[mutate fuzz] {cases} cases, seed {seed}; layout paths: " + ", ".join(f"{p} {n}" for p, n in zip(PATHS, total)))
    for p, n in zip(PATHS, total):
        assert n >= 3, f"the {p} path ran {n} times in {cases} cases: {dict(zip(PATHS, total.tolist()))}"
