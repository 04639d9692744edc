"""NumPy restatement of the se_knn_vote contract (include/sehip.h), written from the contract and not from the kernel, and the
constructed neighbour lists the host and the GPU tests share."""
import numpy as np

PAD = 2 ** 31 - 1       # what sharded_topk writes behind the lists of a tiny shard


def knn_vote_host(idx, cls, C, ks, top, qidx=None):
    """(out_cls, out_votes), int32 [q, len(ks), top]: per query and cut-off k, the ``top`` classes under (votes descending, class
    index ascending) among the first k NEIGHBOURS of the list -- entries inside [0, len(cls)) other than qidx[i] -- and their votes;
    a neighbour whose class lies outside [0, C) counts towards k but casts no vote."""
    idx, cls = np.asarray(idx, dtype=np.int64), np.asarray(cls, dtype=np.int64)
    q = idx.shape[0]
    out_cls = np.zeros((q, len(ks), top), dtype=np.int32)
    out_votes = np.zeros((q, len(ks), top), dtype=np.int32)
    for i in range(q):
        row = idx[i]
        keep = (row >= 0) & (row < len(cls))
        if qidx is not None:
            keep &= row != int(qidx[i])
        neighbours = cls[row[keep]]
        for j, k in enumerate(ks):
            head = neighbours[:int(k)]
            votes = np.bincount(head[(head >= 0) & (head < C)], minlength=C)
            order = np.lexsort((np.arange(C), -votes))[:top]
            out_cls[i, j], out_votes[i, j] = order, votes[order]
    return out_cls, out_votes


def canonical_ranking(queries, gallery, cosine):
    """The oracle's canonical ranking [q, n] of float32 queries against a gallery: cosine on normalised rows, or squared Euclidean."""
    from oracle import retrieval_oracle as ro
    if cosine:
        queries, gallery = ro.canon_normalize_rows(queries), ro.canon_normalize_rows(gallery)
    return ro.canon_rank_rows(ro.canon_pdist(queries, gallery, ro.METRIC_COSINE if cosine else ro.METRIC_EUCLID))


def constructed_cases():
    """name -> (idx [q, L], cls [n], C, ks, top, qidx | None, expected out_cls [q, nk, top], expected out_votes): one property of
    the contract each, with the expected arrays written out by hand."""
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    cases = {}
    # gallery item g has class cls10[g]
    cls10 = i32([3, 1, 1, 3, 2, 0, 2, 4, 4, 0])
    # classes 3 and 1 get two votes each: the smaller index first
    cases["two-way tie"] = (i32([[0, 1, 2, 3, 4]]), cls10, 5, [4], 2, None, i32([[[1, 3]]]), i32([[[2, 2]]]))
    # classes 3, 1, 2 with two votes each, class 0 with one
    cases["three-way tie"] = (i32([[0, 4, 1, 3, 6, 2, 5]]), cls10, 5, [6, 7], 4, None,
                              i32([[[1, 2, 3, 0], [1, 2, 3, 0]]]), i32([[[2, 2, 2, 0], [2, 2, 2, 1]]]))
    # two voted classes, top = 5 = C: the tail 0, 2, 4 in ascending index with 0 votes
    cases["zero-vote tail"] = (i32([[0, 1, 3]]), cls10, 5, [3], 5, None, i32([[[3, 1, 0, 2, 4]]]), i32([[[2, 1, 0, 0, 0]]]))
    # the query's own index at the head, in the middle and absent: k = 2 takes the first two OTHER entries
    cases["qidx head / middle / absent"] = (i32([[7, 0, 1, 2], [0, 7, 1, 2], [0, 1, 2, 4]]), cls10, 5, [1, 2, 3], 2, i32([7, 7, 7]),
                                           i32([[[3, 0], [1, 3], [1, 3]], [[3, 0], [1, 3], [1, 3]], [[3, 0], [1, 3], [1, 3]]]),
                                           i32([[[1, 0], [1, 1], [2, 1]], [[1, 0], [1, 1], [2, 1]], [[1, 0], [1, 1], [2, 1]]]))
    # pads are no neighbours: k = 2 reaches past them; k = 4 finds only three neighbours and all of them vote
    cases["pad entries"] = (i32([[PAD, 4, -1, 6, PAD, 0]]), cls10, 5, [2, 4], 2, None, i32([[[2, 0], [2, 3]]]), i32([[[2, 0], [2, 1]]]))
    # class values outside [0, C) (gallery items 1 and 2 here) are neighbours without a vote: k = 3 counts 0, 1, 2 and sees one vote
    cases["classes outside [0, C)"] = (i32([[0, 1, 2, 4]]), i32([3, 5, -2, 3, 2]), 5, [3, 4], 2, None,
                                      i32([[[3, 0], [2, 3]]]), i32([[[1, 0], [1, 1]]]))
    # leave-one-out with list_len == k + 1: the query is in the list (row 0) -> k others; not in it (row 1) -> the first k
    cases["leave-one-out, list_len == k + 1"] = (i32([[5, 0, 3, 1], [0, 3, 1, 2]]), cls10, 5, [3], 2, i32([5, 9]),
                                                i32([[[3, 1]], [[3, 1]]]), i32([[[2, 1]], [[2, 1]]]))
    return cases
