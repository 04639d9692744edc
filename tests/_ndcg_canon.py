"""NumPy float64 restatement of se_ndcg's contract (include/sehip.h), written from the contract and not from the kernel: a Python
loop per query -- drop the own entry if it is among the entries read, gather the gains, sequential sums -- and the ideal DCG by
brute force (``np.sort`` of the expanded gain list, the own item removed for members).  ``HAND`` holds constructed cases whose
expected values are written out by hand."""
import numpy as np
import torch


def discounts(n):
    return 1 / np.log2(np.arange(2, n + 2))


def ideal_brute(gain, counts, disc, ks, full=True):
    """[C, 2, nk + 1]: per class and member, the DCG of the gallery's gains to that class in descending order at every cut-off
    (slot nk: the whole list, 0 unless ``full``)."""
    gain, counts = np.asarray(gain, dtype=np.float64), np.asarray(counts, dtype=np.int64)
    C = len(counts)
    out = np.zeros((C, 2, len(ks) + 1))
    for c in range(C):
        for member in (0, 1):
            cnt = counts.copy()
            if member and cnt[c] > 0:
                cnt[c] -= 1
            best = np.sort(np.repeat(gain[c], cnt))[::-1]
            cum = np.concatenate(([0.0], np.cumsum(best * np.asarray(disc)[:len(best)])))
            for t, k in enumerate(ks):
                out[c, member, t] = cum[min(k, len(best))]
            if full:
                out[c, member, len(ks)] = cum[len(best)]
    return out


def ndcg_rows(rank, list_len, cls, qcls, qidx, gain_a, gain_b, disc, ideal, ks, want_full):
    """[Q, 2 nk + 2] float64; the whole-list columns are NaN unless ``want_full`` (the kernel leaves them alone).
    ideal: [C, 2, 2, nk + 1], [class][member][table][slot]."""
    rank, cls, ks = np.asarray(rank), np.asarray(cls), [int(k) for k in ks]
    nk = len(ks)
    read = list_len if want_full else min(list_len, max(ks) + 1)
    out = np.full((len(rank), 2 * nk + 2), np.nan)
    for i in range(len(rank)):
        row = rank[i, :read].astype(np.int64)
        member = int(qidx is not None and qidx[i] >= 0)
        if member:
            hit = np.flatnonzero(row == qidx[i])
            if len(hit):
                row = np.delete(row, hit[0])
        n = len(row)
        for t, gain in enumerate((gain_a, gain_b)):
            g = np.asarray(gain, dtype=np.float64)[qcls[i], cls[row]]
            cum = np.concatenate(([0.0], np.cumsum(g * np.asarray(disc)[:n])))
            for s, k in enumerate(ks):
                z = ideal[qcls[i], member, t, s]
                out[i, t * nk + s] = cum[min(k, n)] / z if z > 0 else 0.0
            if want_full:
                z = ideal[qcls[i], member, t, nk]
                out[i, 2 * nk + t] = cum[n] / z if z > 0 else 0.0
    return out


def standin(rank, cls, qcls, qidx, gain_a, gain_b, disc, ideal, ks, want_full=False, list_len=None):
    """``sehip.ndcg`` on CPU tensors (the ``kernels={'ndcg': ...}`` hook); the unwritten whole-list columns are 0 as there."""
    L = rank.shape[1] if list_len is None else int(list_len)
    rows = ndcg_rows(rank.numpy(), L, cls.numpy(), qcls.numpy(), None if qidx is None else qidx.numpy(), gain_a.numpy(), gain_b.numpy(),
                     disc.numpy(), ideal.numpy(), ks.numpy().tolist(), want_full)
    return torch.from_numpy(np.nan_to_num(rows, nan=0.0))


# ---- constructed cases.  Five gallery items of classes 0 1 2 1 0; the gains of query class 0 are 1 / 0.5 / 0 (table a) and, for
# table b, 1 / 0.25 / 0.5 -- row 0 of non-symmetric tables whose other rows differ.  1 / log2(3) = 0.6309297535714575,
# 1 / log2(4) = 0.5, 1 / log2(5) = 0.43067655807339306
HAND_CLS = [0, 1, 2, 1, 0]
HAND_GAIN_A = [[1.0, 0.5, 0.0], [0.25, 1.0, 0.125], [0.0, 0.75, 1.0]]
HAND_GAIN_B = [[1.0, 0.25, 0.5], [0.5, 1.0, 0.0], [0.125, 0.0, 1.0]]
HAND = [
    # not a gallery item: ranking 3 0 2 4 1 -> gains a 0.5 1 0 1 0.5; ideal list 1 1 0.5 0.5 0
    dict(rank=[3, 0, 2, 4, 1], qcls=0, qidx=-1, k=3,
         dcg_a=0.5 + 1.0 * 0.6309297535714575 + 0.0 * 0.5,
         idcg_a=1.0 + 1.0 * 0.6309297535714575 + 0.5 * 0.5,
         # gains b 0.25 1 0.5 1 0.25; ideal list 1 1 0.5 0.25 0.25
         dcg_b=0.25 + 1.0 * 0.6309297535714575 + 0.5 * 0.5,
         idcg_b=1.0 + 1.0 * 0.6309297535714575 + 0.5 * 0.5),
    # gallery item 0, found at position 1 and dropped: 3 2 4 1 -> gains a 0.5 0 1 0.5; ideal list without item 0: 1 0.5 0.5 0
    dict(rank=[3, 0, 2, 4, 1], qcls=0, qidx=0, k=3,
         dcg_a=0.5 + 0.0 * 0.6309297535714575 + 1.0 * 0.5,
         idcg_a=1.0 + 0.5 * 0.6309297535714575 + 0.5 * 0.5,
         # gains b 0.25 0.5 1 0.25; ideal list 1 0.5 0.25 0.25
         dcg_b=0.25 + 0.5 * 0.6309297535714575 + 1.0 * 0.5,
         idcg_b=1.0 + 0.5 * 0.6309297535714575 + 0.25 * 0.5),
    # the whole list (k = 0 here): four entries after the drop
    dict(rank=[3, 0, 2, 4, 1], qcls=0, qidx=0, k=0,
         dcg_a=0.5 + 0.0 * 0.6309297535714575 + 1.0 * 0.5 + 0.5 * 0.43067655807339306,
         idcg_a=1.0 + 0.5 * 0.6309297535714575 + 0.5 * 0.5 + 0.0 * 0.43067655807339306,
         dcg_b=0.25 + 0.5 * 0.6309297535714575 + 1.0 * 0.5 + 0.25 * 0.43067655807339306,
         idcg_b=1.0 + 0.5 * 0.6309297535714575 + 0.25 * 0.5 + 0.25 * 0.43067655807339306),
    # a member whose entry is not in the list: nothing is dropped (3 2 4 1 2), the ideal still misses item 0
    dict(rank=[3, 2, 4, 1, 2], qcls=0, qidx=0, k=2,
         dcg_a=0.5 + 0.0 * 0.6309297535714575, idcg_a=1.0 + 0.5 * 0.6309297535714575,
         dcg_b=0.25 + 0.5 * 0.6309297535714575, idcg_b=1.0 + 0.5 * 0.6309297535714575),
]


def hand_values(case):
    """(NDCG a, NDCG b) of a HAND case through ``ndcg_rows`` with the brute-force ideal."""
    n = len(HAND_CLS)
    disc, counts = discounts(n), np.bincount(HAND_CLS, minlength=3)
    ks = [case["k"]] if case["k"] else [1]
    ideal = np.stack([ideal_brute(g, counts, disc, ks, full=True) for g in (HAND_GAIN_A, HAND_GAIN_B)], axis=2)
    rows = ndcg_rows(np.array([case["rank"]], dtype=np.int32), n, np.array(HAND_CLS), np.array([case["qcls"]]), np.array([case["qidx"]]),
                     HAND_GAIN_A, HAND_GAIN_B, disc, ideal, ks, True)
    return (rows[0, 0], rows[0, 1]) if case["k"] else (rows[0, 2], rows[0, 3])
