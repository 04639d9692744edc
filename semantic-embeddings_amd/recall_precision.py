"""Recall-precision curve and mAP of all-pairs nearest-neighbour retrieval (the loop of the reference's
plot_recall_precision.py:52-79), computed from the device rankings by the MI355X kernels of libsehip.so.

For every image ``qid`` taken as a query against all images, the reference takes the relevance of its ranking with the query
itself removed (``labels[r] == labels[qid]``).  Write ``R`` for the number of relevant items and ``p_j`` for the 1-based position
of the j-th one.  Then

* AP is ``(1 / R) sum_j j / p_j`` (sklearn's ``average_precision_score`` of a tie-free score), and mAP its mean over all queries;
* the query's curve points are ``(j / R, j / p_j)`` for j = 1 .. R, plus ``(0.0, 0.0)`` when the first retrieved item is not
  relevant (``p_1 > 1``); with ``bins = B`` the key of a point is ``int(recall * B) / B + 1 / (2 B)`` and a bin holds the max
  precision of its points;
* the curve is ``levels = sorted(keys)`` with the mean over the queries that have each key.

Edge cases:

* a query whose class has no other member (``R = 0``) contributes AP = 0 to the mAP (sklearn's value) and no curve points; one
  ``RuntimeWarning`` per call gives their number.  (The reference adds a separate NaN level per position in that case, and raises
  with ``--bins``.)
* levels are float64 values; ``j / R`` and ``j' / R'`` of different class sizes are one level exactly when the fractions are equal,
  as in the reference's dict.
* bin indices are computed as Python does: ``int((j / R) * B)`` in IEEE float64.
* ties: the device ranking is the canonical (stable) one; nothing here handles ties on its own.
"""
import warnings

import numpy as np


def _class_indices(lab):
    class_list = sorted(set(lab), key=lambda c: (str(type(c)), c))
    pos = {c: i for i, c in enumerate(class_list)}
    return np.array([pos[c] for c in lab], dtype=np.int32), len(class_list)


def _bin_keys(b, bins):
    return np.asarray(b, dtype=np.int64) / bins + 1 / (2 * bins)


def _warn_singletons(n_single):
    if n_single:
        warnings.warn('recall-precision: {} quer{} without any other item of their class: AP 0, no curve points'
                      .format(n_single, 'y' if n_single == 1 else 'ies'), RuntimeWarning, stacklevel=3)


def recall_precision_host(ranking, labels, bins=None):
    """NumPy statement of plot_recall_precision.py:52-79 on a full ranking (CPU use, and the tests' bridge to the golden values).

    ``ranking`` [N, N] ints: row i is query i's ranking of the item indices 0 .. N - 1 (itself included); ``labels[i]`` is the
    class of item i.  Returns ``(levels, mean_precision, mAP, per_query_ap)`` (float64 arrays, float)."""
    ranking = np.asarray(ranking)
    cls, _ = _class_indices(list(labels))
    n = ranking.shape[0]
    bins = int(bins) if bins else 0
    recprec = {}
    aps = np.zeros(n, dtype=np.float64)
    n_single = 0
    for q in range(n):
        row = ranking[q]
        row = row[row != q]
        pos = np.flatnonzero(cls[row] == cls[q]) + 1
        R = len(pos)
        if R == 0:
            n_single += 1
            continue
        j = np.arange(1, R + 1)
        prec = j / pos
        aps[q] = prec.sum() / R
        if bins:
            b = ((j / R) * bins).astype(np.int64)
            best = {}
            if pos[0] > 1:
                best[0] = 0.0
            for bi, p in zip(b.tolist(), prec.tolist()):
                best[bi] = max(best[bi], p) if bi in best else p
            pts = zip(_bin_keys(list(best), bins).tolist(), best.values())
        else:
            pts = list(zip((j / R).tolist(), prec.tolist()))
            if pos[0] > 1:
                pts.append((0.0, 0.0))
        for key, p in pts:
            recprec.setdefault(key, []).append(p)
    _warn_singletons(n_single)
    levels = np.array(sorted(recprec), dtype=np.float64)
    means = np.array([np.mean(recprec[k]) for k in levels.tolist()], dtype=np.float64)
    return levels, means, float(np.mean(aps)) if n else float('nan'), aps


def recall_precision_device(features, labels, normalize=False, bins=None, ids=None, kblocks=None, tile_rows=None, kernels=None):
    """``plot_recall_precision.py``'s per-feature-file computation (lines 52-79) without leaving the GPU: the rankings stay device
    tensors (``evaluate_retrieval.ranking_tiles``; every image is query and gallery item), ``se_relevant_positions`` finds the
    positions of each query's relevant items, ``se_recall_precision_reduce`` turns them into per-query AP and per-class sums
    (fixed summation order: the same bits on every call, whatever the tiling), and the levels are merged here in float64.

    ``features``: float32 ``[N, D]`` array / device tensor, or a dict / pickle path as ``pairwise_retrieval`` takes it;
    ``labels``: class label of image ``ids[i]`` (``ids`` defaults to the dict's keys, else ``range(N)``), a sequence or a mapping.
    ``bins``: None, or the number of recall bins of the reference's ``--bins``.  ``kblocks``: as ``ranking_tiles``.
    ``kernels`` (tests): CPU stand-ins ``{'ranking_tiles', 'relevant_positions', 'recall_precision_reduce', 'device'}``.
    Returns ``(levels, mean_precision, mAP, per_query_ap)``; see the module docstring for the edge cases."""
    import torch
    from evaluate_retrieval import _as_feature_matrix

    kernels = dict(kernels or {})
    if any(k not in kernels for k in ('ranking_tiles', 'relevant_positions', 'recall_precision_reduce')):
        import sehip
        from evaluate_retrieval import ranking_tiles
        kernels.setdefault('ranking_tiles', ranking_tiles)
        kernels.setdefault('relevant_positions', sehip.relevant_positions)
        kernels.setdefault('recall_precision_reduce', sehip.recall_precision_reduce)
    bins = int(bins) if bins else 0
    if bins < 0:
        raise ValueError('bins must be a positive number of recall levels')

    features, ind2id, _ = _as_feature_matrix(features)
    if ids is None and ind2id is not None:
        ids = ind2id.tolist()
    n = int(features.shape[0])
    ids = list(range(n)) if ids is None else list(ids)
    if len(ids) != n:
        raise ValueError('{} ids for {} feature rows'.format(len(ids), n))
    cls_h, C = _class_indices([labels[i] for i in ids])
    counts = np.bincount(cls_h, minlength=C)
    r_cls = counts - 1                                    # relevant items of a query of class c: the rest of its class
    class_off = np.concatenate([[0], np.cumsum(r_cls)]).astype(np.int64)
    dev = kernels.get('device') or torch.device('cuda', torch.cuda.current_device())
    if torch.is_tensor(features):
        feats = features.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
    else:
        feats = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(dev)

    cls_d = torch.from_numpy(cls_h).to(dev)
    qidx_d = torch.arange(n, dtype=torch.int32, device=dev)
    class_off_d = torch.from_numpy(class_off).to(dev)
    ap = torch.zeros(n, dtype=torch.float64, device=dev)
    prec_sum = torch.zeros(max(int(class_off[-1]), 1), dtype=torch.float64, device=dev)[:int(class_off[-1])]
    first_miss = torch.zeros(C, dtype=torch.int64, device=dev)
    bin_sum = torch.zeros((C, bins + 1), dtype=torch.float64, device=dev) if bins else None
    bin_count = torch.zeros((C, bins + 1), dtype=torch.int64, device=dev) if bins else None
    # each tile is consumed before the next one is drawn (ranking_tiles reuses its buffers)
    for r0, tile in kernels['ranking_tiles'](feats, normalize, tile_rows=tile_rows, kblocks=kblocks):
        rows = int(tile.shape[0])
        qc = cls_h[r0:r0 + rows]
        hit_off = np.concatenate([[0], np.cumsum(r_cls[qc])]).astype(np.int64)
        order = np.argsort(qc, kind='stable').astype(np.int32)
        class_start = np.concatenate([[0], np.cumsum(np.bincount(qc, minlength=C))]).astype(np.int32)
        hit_off_d = torch.from_numpy(hit_off).to(dev)
        hit_pos = kernels['relevant_positions'](tile, cls_d, cls_d[r0:r0 + rows], qidx_d[r0:r0 + rows], hit_off_d,
                                                num_classes=C, total=int(hit_off[-1]))
        kernels['recall_precision_reduce'](hit_pos, hit_off_d, torch.from_numpy(order).to(dev), torch.from_numpy(class_start).to(dev),
                                           class_off_d, bins, ap[r0:r0 + rows], prec_sum, first_miss, bin_sum, bin_count)

    ap_h = ap.cpu().numpy()
    _warn_singletons(int(counts[r_cls == 0].sum()))
    if bins:
        bs, bc = bin_sum.cpu().numpy(), bin_count.cpu().numpy()
        tot_s, tot_c = bs.sum(axis=0), bc.sum(axis=0)
        have = np.flatnonzero(tot_c > 0)
        levels, means = _bin_keys(have, bins), tot_s[have] / tot_c[have]
    else:
        S, miss = prec_sum.cpu().numpy(), first_miss.cpu().numpy()
        keys, sums, cnts = [], [], []
        for c in np.flatnonzero(r_cls > 0):
            R = int(r_cls[c])
            keys.append(np.arange(1, R + 1) / R)
            sums.append(S[class_off[c]:class_off[c + 1]])
            cnts.append(np.full(R, counts[c], dtype=np.int64))
            if miss[c] > 0:
                keys.append(np.zeros(1))
                sums.append(np.zeros(1))
                cnts.append(np.array([miss[c]], dtype=np.int64))
        if keys:
            levels, inv = np.unique(np.concatenate(keys), return_inverse=True)
            means = np.bincount(inv, weights=np.concatenate(sums)) / np.bincount(inv, weights=np.concatenate(cnts))
        else:
            levels, means = np.zeros(0), np.zeros(0)
    return (np.asarray(levels, dtype=np.float64), np.asarray(means, dtype=np.float64),
            float(ap_h.mean()) if n else float('nan'), ap_h)
