"""The order rule of `lmi_regroup` in numpy (include/lmi_hip.h states it): the reference of tests/test_gpu_regroup.py, checked on
its own by tests/test_regroup_host.py.

An index holds its objects bucket by bucket, every bucket's in the order they arrived.  For objects given in arrival order with
labels `old_lab` that is `np.argsort(old_lab, kind="stable")`.  The regrouped index holds what a fresh build of THAT list -- each
object with its new label -- holds, so a new bucket's objects are ordered by (old bucket, old row) whatever the order of the list
or of the map."""
import numpy as np


def new_labels(old_lab, ids, list_ids, list_labels, bucket_map=None):
    """The new label of every object: `list_labels[i]` where its id is `list_ids[i]` (every object that carries the id), else
    `bucket_map[old label]` (None: the old label).  An object left on a map entry of -1 keeps -1: the call must refuse it.
    Returns (labels int64 [N], n_named)."""
    old_lab, ids = np.asarray(old_lab, dtype=np.int64), np.asarray(ids, dtype=np.uint32)
    list_ids, list_labels = np.asarray(list_ids, dtype=np.uint32).reshape(-1), np.asarray(list_labels, dtype=np.int64).reshape(-1)
    assert np.unique(list_ids).size == list_ids.size, "an id is listed twice"
    out = old_lab.copy() if bucket_map is None else np.asarray(bucket_map, dtype=np.int64)[old_lab]
    order = np.argsort(list_ids, kind="stable")
    at = np.searchsorted(list_ids[order], ids)
    at[at == list_ids.size] = 0
    named =(list_ids[order][at] == ids) if list_ids.size else np.zeros(ids.shape, dtype=bool)
    out[named] = list_labels[order][at[named]]
    return out, int(named.sum())


def resident_order(old_lab):
    """Where an index built from labels `old_lab` holds its objects: position j of the resident order is object `perm[j]`."""
    return np.argsort(np.asarray(old_lab), kind="stable")


def regrouped(X, old_lab, ids, new_lab):
    """The object list a fresh build of which the regrouped index equals: (X, new labels, ids) in the resident order."""
    perm = resident_order(old_lab)
    return np.asarray(X)[perm], np.asarray(new_lab)[perm], np.asarray(ids)[perm]


def bucket_contents(old_lab, ids, new_lab, L_new):
    """Per new bucket the ids it holds, in order: the plain statement -- walk the old buckets in ascending order, each in its own
    order, and append every object to its new bucket."""
    old_lab, ids, new_lab = np.asarray(old_lab), np.asarray(ids), np.asarray(new_lab)
    out = [[] for _ in range(L_new)]
    for b in np.unique(old_lab):
        for i in np.flatnonzero(old_lab == b):
            out[int(new_lab[i])].append(int(ids[i]))
    return [np.asarray(o, dtype=np.uint32) for o in out]
