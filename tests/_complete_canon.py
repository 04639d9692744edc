"""NumPy restatement of se_complete_rankings' contract (include/sehip.h), `status` and the "bad row gets `order`" rule included.
tests/test_ranked_host.py holds it against the reference's own line on Python lists (class_hierarchy.py:262-264)."""
import numpy as np

BAD_RANGE, BAD_DUP = 1, 2


def complete_rankings(lists, gallery, lengths=None, order=None):
    """lists [Q, L] ints, lengths [Q] | None, order [gallery] | None -> (rank [Q, gallery] int32, status [Q] int32)."""
    lists = np.asarray(lists).reshape(len(lists), -1)
    q, L = lists.shape
    order = np.arange(gallery, dtype=np.int32) if order is None else np.asarray(order, dtype=np.int32)
    rank = np.empty((q, gallery), dtype=np.int32)
    status = np.zeros(q, dtype=np.int32)
    for i in range(q):
        n = L if lengths is None else min(max(int(lengths[i]), 0), L)
        row = lists[i, :n].astype(np.int64)
        ok = (row >= 0) & (row < gallery)
        if not ok.all():
            status[i] |= BAD_RANGE
        if len(np.unique(row[ok])) != int(ok.sum()):
            status[i] |= BAD_DUP
        if status[i]:
            rank[i] = order
            continue
        present = np.zeros(gallery, dtype=bool)
        present[row] = True
        rank[i, :n] = row
        rank[i, n:] = order[~present[order]]
    return rank, status


def complete_list_reference(ret, all_ids):
    """The reference's own lines on Python lists (class_hierarchy.py:262-264)."""
    sret = set(ret)
    return ret + [id for id in all_ids if id not in sret]
