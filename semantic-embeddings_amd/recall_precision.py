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

Queries against a separate gallery (``recall_precision_device(..., gallery=...)``): the same statement with ``p_j`` the position in
the query's ranking of the GALLERY, the query's own gallery item (same id) removed where there is one.  The positions are counted
(``se_count_preceding`` / ``se_count_to_positions``: gallery columns in front of each relevant item), never read off a ranking.
"""
import collections
import warnings

import numpy as np

from evaluate_retrieval import RANKING_KERNELS, _as_feature_matrix, _cached_rows, _resolve_kblocks, is_float64, resolve_kernels, to_device_f64


def class_indices(*label_lists):
    """``(class list, [int32 class index of every label] per list)``: the classes of all lists together, sorted (by type name
    first, so that labels of several types still sort)."""
    class_list = sorted(set().union(*label_lists), key=lambda c: (str(type(c)), c))
    pos = {c: i for i, c in enumerate(class_list)}
    return class_list, [np.array([pos[c] for c in lab], dtype=np.int32) for lab in label_lists]


def to_device_f32(x, dev):
    """A float32 copy of the feature matrix ``x`` (array or tensor) on ``dev`` that the kernels may normalise in place."""
    import torch
    if torch.is_tensor(x):      # features straight from the network (learn_image_embeddings feature extraction): stay on the device
        return x.detach().to(device=dev, dtype=torch.float32).contiguous().clone()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _bin_keys(b, bins):
    return np.asarray(b, dtype=np.int64) / bins + 1 / (2 * bins)


def _number_of_bins(bins):
    bins = int(bins) if bins else 0
    if bins < 0:
        raise ValueError('bins must be a positive number of recall levels')
    return bins


def _warn_singletons(n_single, stacklevel=3):
    if n_single:
        warnings.warn('recall-precision: {} quer{} without any other item of their class: AP 0, no curve points'
                      .format(n_single, 'y' if n_single == 1 else 'ies'), RuntimeWarning, stacklevel=stacklevel)


def recall_precision_host(ranking, labels, bins=None):
    """NumPy statement of plot_recall_precision.py:52-79 on a full ranking (CPU use, and the tests' bridge to the golden values).

    ``ranking`` [N, N] ints: row i is query i's ranking of the item indices 0 .. N - 1 (itself included); ``labels[i]`` is the
    class of item i.  Returns ``(levels, mean_precision, mAP, per_query_ap)`` (float64 arrays, float)."""
    return recall_precision_host_gallery(ranking, labels, labels, np.arange(len(ranking)), bins, stacklevel=4)


def recall_precision_host_gallery(ranking, query_labels, gallery_labels, qidx=None, bins=None, stacklevel=3):
    """``recall_precision_host`` for queries that are not the gallery: ``ranking`` [Q, N] ints, row i is query i's ranking of the
    gallery items 0 .. N - 1; ``query_labels[i]`` / ``gallery_labels[j]`` their classes; ``qidx[i]`` the gallery item that IS
    query i (removed from its ranking, the reference's ``ignore_qids``), -1 / None when it is not in the gallery.  A query whose
    class has no (other) gallery item gets AP 0 and no curve points.  Returns ``(levels, mean_precision, mAP, per_query_ap)``.
    (``stacklevel``: of the warning about such queries -- it names the caller of whichever host function was called.)"""
    ranking = np.asarray(ranking)
    _, (qcls, gcls) = class_indices(list(query_labels), list(gallery_labels))
    nq = ranking.shape[0]
    bins = int(bins) if bins else 0
    recprec = {}
    aps = np.zeros(nq, dtype=np.float64)
    n_single = 0
    for q in range(nq):
        row = ranking[q]
        if qidx is not None and qidx[q] >= 0:
            row = row[row != qidx[q]]
        pos = np.flatnonzero(gcls[row] == qcls[q]) + 1
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
    _warn_singletons(n_single, stacklevel)
    levels = np.array(sorted(recprec), dtype=np.float64)
    means = np.array([np.mean(recprec[k]) for k in levels.tolist()], dtype=np.float64)
    return levels, means, float(np.mean(aps)) if nq else float('nan'), aps


def _accumulators(nq, groups, total, bins, dev):
    """What ``se_recall_precision_reduce`` adds into, zeroed: ``(ap [nq], prec_sum [total], first_miss [groups], bin_sum, bin_count
    [groups, bins + 1] -- None without bins)``."""
    import torch
    return (torch.zeros(nq, dtype=torch.float64, device=dev), torch.zeros(max(total, 1), dtype=torch.float64, device=dev)[:total],
            torch.zeros(groups, dtype=torch.int64, device=dev),
            torch.zeros((groups, bins + 1), dtype=torch.float64, device=dev) if bins else None,
            torch.zeros((groups, bins + 1), dtype=torch.int64, device=dev) if bins else None)


def recall_precision_device(features, labels, normalize=False, bins=None, ids=None, kblocks=None, tile_rows=None, kernels=None,
                            gallery=None, gallery_labels=None, gallery_ids=None, tile_cols=None, distributed=False, group=None,
                            precision=None):
    """``plot_recall_precision.py``'s per-feature-file computation (lines 52-79) without leaving the GPU: the rankings stay device
    tensors (``evaluate_retrieval.ranking_tiles``; every image is query and gallery item), ``se_relevant_positions`` finds the
    positions of each query's relevant items, ``se_recall_precision_reduce`` turns them into per-query AP and per-class sums
    (fixed summation order: the same bits on every call, whatever the tiling), and the levels are merged here in float64.

    ``features``: float32 ``[N, D]`` array / device tensor, or a dict / pickle path as ``pairwise_retrieval`` takes it;
    ``labels``: class label of image ``ids[i]`` (``ids`` defaults to the dict's keys, else ``range(N)``), a sequence or a mapping.
    ``bins``: None, or the number of recall bins of the reference's ``--bins``.  ``kblocks``: as ``ranking_tiles``.
    ``kernels`` (tests): CPU stand-ins ``{'ranking_tiles', 'relevant_positions', 'recall_precision_reduce', 'device'}``.
    Returns ``(levels, mean_precision, mAP, per_query_ap)``; see the module docstring for the edge cases.

    ``gallery`` (features in any of the forms above): the rows of ``features`` are QUERIES against this gallery instead of against
    each other; ``gallery_labels`` (default ``labels``) and ``gallery_ids`` name its items like ``labels`` / ``ids`` do the queries.
    A query whose id is also a gallery id is removed from its own ranking (the reference's ``ignore_qids``); a gallery given as a plain
    matrix without ``gallery_ids`` shares no id with the queries.  No ranking of the gallery is made: the positions of the relevant
    items are counted (``query_gallery_positions``), so the gallery may be far longer than a row ``se_rank_rows`` sorts in registers.
    ``tile_cols`` (tests): gallery columns per distance slab.  ``distributed``: every rank counts over its shard of the gallery
    (``sharded_retrieval.shard_bounds``) and ONE integer all-reduce per query tile adds the counts; all ranks return the same values.

    ``precision='float64'`` (opt-in): float64 ``features`` are ranked in float64 (``ranking_tiles(..., precision='float64')``); all-pairs
    only -- with a ``gallery`` or with ``kblocks`` it raises ``ValueError``."""
    f64 = is_float64(precision)
    if f64 and (gallery is not None or kblocks is not None):
        raise ValueError("precision='float64' ranks all pairs of one float64 feature matrix with ONE FMA chain per distance: a separate "
                         "gallery stays float32, kblocks does not apply")
    if gallery is not None:
        return _recall_precision_gallery(features, labels, normalize, bins, ids, kblocks, tile_rows, tile_cols, kernels, gallery,
                                         gallery_labels, gallery_ids, distributed, group)
    import torch

    kernels = resolve_kernels(kernels, ('ranking_tiles', 'relevant_positions', 'recall_precision_reduce', 'device'))
    bins = _number_of_bins(bins)
    p = gallery_problem(features, labels, ids)
    n, cls_h, C, dev = len(p.q_ids), p.qcls, len(p.class_list), kernels['device']
    counts = np.bincount(cls_h, minlength=C)
    r_cls = counts - 1                                    # relevant items of a query of class c: the rest of its class
    class_off = np.concatenate([[0], np.cumsum(r_cls)]).astype(np.int64)
    feats = to_device_f64(p.qf, dev) if f64 else to_device_f32(p.qf, dev)
    tiles_kw = {'precision': 'float64'} if f64 else {}

    cls_d = torch.from_numpy(cls_h).to(dev)
    qidx_d = torch.arange(n, dtype=torch.int32, device=dev)
    class_off_d = torch.from_numpy(class_off).to(dev)
    ap, prec_sum, first_miss, bin_sum, bin_count = _accumulators(n, C, int(class_off[-1]), bins, dev)
    # each tile is consumed before the next one is drawn (ranking_tiles reuses its buffers)
    for r0, tile in kernels['ranking_tiles'](feats, normalize, tile_rows=tile_rows, kblocks=kblocks, **tiles_kw):
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

    _warn_singletons(int(counts[r_cls == 0].sum()))
    return _merge_levels(ap.cpu().numpy(), r_cls, counts, class_off, bins, prec_sum, first_miss, bin_sum, bin_count)


def _merge_levels(ap_h, r_cls, nq_cls, class_off, bins, prec_sum, first_miss, bin_sum, bin_count):
    """Per-class device sums -> ``(levels, mean_precision, mAP, per_query_ap)`` in float64: ``r_cls[c]`` relevant items of every query
    of class c, ``nq_cls[c]`` its queries."""
    n = len(ap_h)
    if bins:
        bs, bc = bin_sum.cpu().numpy(), bin_count.cpu().numpy()
        tot_s, tot_c = bs.sum(axis=0), bc.sum(axis=0)
        have = np.flatnonzero(tot_c > 0)
        levels, means = _bin_keys(have, bins), tot_s[have] / tot_c[have]
    else:
        S, miss = prec_sum.cpu().numpy(), first_miss.cpu().numpy()
        keys, sums, cnts = [], [], []
        for c in np.flatnonzero((r_cls > 0) & (nq_cls > 0)):
            R = int(r_cls[c])
            keys.append(np.arange(1, R + 1) / R)
            sums.append(S[class_off[c]:class_off[c + 1]])
            cnts.append(np.full(R, nq_cls[c], dtype=np.int64))
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


# ---------------------------------------------------------------------------------------------- queries against a separate gallery

def _ids_of(ind2id, ids, n):
    if ids is None and ind2id is not None:
        ids = ind2id.tolist()
    if ids is not None and len(ids) != n:
        raise ValueError('{} ids for {} feature rows'.format(len(ids), n))
    return None if ids is None else list(ids)


EvalProblem = collections.namedtuple('EvalProblem', 'qf gf q_ids qcls gcls class_list qidx')


def gallery_problem(features, labels, ids=None, gallery=None, gallery_labels=None, gallery_ids=None):
    """Host bookkeeping of a query-vs-gallery evaluation: ``(query features, gallery features, query ids, qcls, gcls, class list,
    qidx)`` -- class indices int32 over the sorted union of the classes on either side, ``qidx[i]`` the (first) gallery row whose
    id equals query i's id, else -1.  Without a ``gallery`` the all-pairs problem: the gallery IS the queries (``gf is qf``,
    ``gcls is qcls``) and ``qidx[i] = i``."""
    qf, q_ind2id, _ = _as_feature_matrix(features)
    if gallery is not None:
        gf, g_ind2id, _ = _as_feature_matrix(gallery)
        if int(qf.shape[1]) != int(gf.shape[1]):
            raise ValueError('queries have {} feature dimensions, the gallery {}'.format(qf.shape[1], gf.shape[1]))
    nq = int(qf.shape[0])
    q_ids = _ids_of(q_ind2id, ids, nq)
    q_ids = list(range(nq)) if q_ids is None else q_ids
    q_lab = [labels[i] for i in q_ids]
    if gallery is None:
        class_list, (cls,) = class_indices(q_lab)
        return EvalProblem(qf, qf, q_ids, cls, cls, class_list, np.arange(nq, dtype=np.int32))
    ng = int(gf.shape[0])
    g_ids = _ids_of(g_ind2id, gallery_ids, ng)
    gallery_labels = labels if gallery_labels is None else gallery_labels
    g_lab = [gallery_labels[i] for i in (range(ng) if g_ids is None else g_ids)]
    class_list, (qcls, gcls) = class_indices(q_lab, g_lab)
    qidx = np.full(nq, -1, dtype=np.int32)
    if g_ids is not None:
        row_of = {}
        for j, g in enumerate(g_ids):
            row_of.setdefault(g, j)
        qidx = np.array([row_of.get(i, -1) for i in q_ids], dtype=np.int32)
    return EvalProblem(qf, gf, q_ids, qcls, gcls, class_list, qidx)


RankedProblem = collections.namedtuple('RankedProblem', 'q_ids g_ids qcls gcls class_list qidx list_len lengths index_tile')


def _integer_ids(ids):
    """``ids`` as a 1-d int64 array when they are integers that fit one, else None."""
    try:
        a = np.asarray(ids) if len(ids) else np.zeros(0, dtype=np.int64)
    except (ValueError, TypeError):     # ids of several shapes
        return None
    if a.ndim != 1 or a.dtype.kind not in 'iu' or (a.dtype == np.uint64 and len(a) and int(a.max()) >= 2 ** 63):
        return None
    return a.astype(np.int64)


class _GalleryIndex(object):
    """ids -> gallery indices (-1: not a gallery id).  Integer ids are looked up vectorised -- a search in the sorted gallery ids plus
    an equality check, on whichever device the ids are -- other hashables through a dict."""

    def __init__(self, g_ids):
        self.ids = g_ids
        arr = _integer_ids(g_ids)
        self.sorted = self.sorter = self.row_of = None
        self.on = {}
        if arr is not None:
            self.sorter = np.argsort(arr, kind='stable')
            self.sorted = arr[self.sorter]
            unique = not (self.sorted[1:] == self.sorted[:-1]).any()
        else:
            self.row_of = {g: j for j, g in enumerate(g_ids)}
            unique = len(self.row_of) == len(g_ids)
        if not unique:
            raise ValueError('the gallery ids are not distinct: a ranking cannot be a permutation of them')

    def _dict(self):
        if self.row_of is None:
            self.row_of = {g: j for j, g in enumerate(self.ids)}
        return self.row_of

    def of_tensor(self, ids):
        """int64 tensor of the gallery indices of an integer tensor of ids, on its device."""
        import torch
        if self.sorted is None or not len(self.ids):
            return torch.full(ids.shape, -1, dtype=torch.int64, device=ids.device)
        if ids.device not in self.on:
            self.on[ids.device] = (torch.from_numpy(self.sorted).to(ids.device), torch.from_numpy(self.sorter).to(ids.device))
        srt, sorter = self.on[ids.device]
        ids = ids.to(torch.int64)
        pos = torch.searchsorted(srt, ids.contiguous()).clamp_(max=len(self.ids) - 1)
        return torch.where(srt[pos] == ids, sorter[pos], torch.full_like(pos, -1))

    def of_sequence(self, ids):
        """int64 array of the gallery indices of a sequence of ids."""
        import torch
        arr = _integer_ids(ids) if self.sorted is not None else None
        if arr is not None:
            return self.of_tensor(torch.from_numpy(arr)).numpy()
        get = self._dict().get
        out = np.empty(len(ids), dtype=np.int64)
        for j, i in enumerate(ids):
            try:
                out[j] = get(i, -1)
            except TypeError:       # unhashable: no id
                out[j] = -1
        return out


def ranked_problem(retrieved, labels, ignore_qids=True, all_ids=None):
    """Host bookkeeping of an evaluation of GIVEN rankings (ClassHierarchy.hierarchical_precision_ranked, recall_precision_ranked):
    ``RankedProblem(q_ids, g_ids, qcls, gcls, class_list, qidx, list_len, lengths, index_tile)``.

    ``retrieved``: the reference's forms -- a dict ``query id -> ranked id list`` or a generator of such pairs -- or the array form
    ``(query_ids [Q], ranking [Q, L])`` / ``(query_ids, ranking, lengths [Q])`` with ``ranking`` a 2-d integer array or (device) tensor
    of ids, row i holding ``lengths[i]`` (default L) ids.  The gallery is ``all_ids`` when that is given (gallery index = position in
    it, so ids missing from a list are appended in ``all_ids`` order by completing in index order); otherwise it is the id set of the
    first list, and every list must be a permutation of it -- partial lists without ``all_ids`` raise ``ValueError``.
    ``qidx[i]``: gallery index of query i's id, -1 when it is no gallery id; None with ``ignore_qids=False`` (the kernels' NULL:
    keep everything).  Classes: ``class_indices`` over queries and gallery.  ``lengths``: int32 [Q] on the host.
    ``index_tile(r0, r1, dev)`` -> ``(lists, lengths)``: the lists of queries r0 .. r1 as int32 gallery indices ``[r1 - r0, list_len]``
    on ``dev`` (entries behind a row's length are -1) and their lengths (None when every row is full); an id that is not in the
    gallery raises ``ValueError`` naming the id and the query."""
    import torch
    rows = ranking = None
    if isinstance(retrieved, tuple) and len(retrieved) in (2, 3):
        q_ids, ranking = retrieved[0], retrieved[1]
        q_ids = q_ids.tolist() if hasattr(q_ids, 'tolist') else list(q_ids)
        if not torch.is_tensor(ranking):
            ranking = np.asarray(ranking)
        if ranking.ndim != 2 or (ranking.dtype.kind not in 'iu' if isinstance(ranking, np.ndarray) else
                                 (ranking.dtype.is_floating_point or ranking.dtype == torch.bool)):
            raise ValueError('the array form takes a 2-d integer ranking [queries, list length]')
        if int(ranking.shape[0]) != len(q_ids):
            raise ValueError('{} query ids for {} ranking rows'.format(len(q_ids), int(ranking.shape[0])))
        L = int(ranking.shape[1])
        if len(retrieved) == 3 and retrieved[2] is not None:
            lengths = retrieved[2]
            lengths = (lengths.cpu().numpy() if torch.is_tensor(lengths) else np.asarray(lengths)).astype(np.int64).reshape(-1)
            if len(lengths) != len(q_ids) or (len(lengths) and (lengths.min() < 0 or lengths.max() > L)):
                raise ValueError('lengths must hold one value in [0, {}] per query'.format(L))
        else:
            lengths = np.full(len(q_ids), L, dtype=np.int64)
        if isinstance(ranking, np.ndarray):
            ranking = torch.from_numpy(np.ascontiguousarray(ranking if ranking.dtype != np.uint64 else ranking.astype(np.int64)))
    else:
        items = list(retrieved.items() if hasattr(retrieved, 'items') else retrieved)
        q_ids = [qid for qid, _ in items]
        rows = [ret if isinstance(ret, (list, tuple, np.ndarray)) else list(ret) for _, ret in items]
        lengths = np.array([len(r) for r in rows], dtype=np.int64)
        L = int(lengths.max()) if len(rows) else 0
    nq = len(q_ids)

    def first_list():
        if rows is not None:
            return list(rows[0].tolist() if isinstance(rows[0], np.ndarray) else rows[0])
        return ranking[0, :int(lengths[0])].cpu().tolist()

    if all_ids is not None and len(all_ids):        # (an empty all_ids is none, as in the reference)
        g_ids = all_ids.tolist() if hasattr(all_ids, 'tolist') else list(all_ids)
    else:
        g_ids = first_list() if nq else []
        if nq and (lengths != len(g_ids)).any():
            i = int(np.flatnonzero(lengths != len(g_ids))[0])
            raise ValueError('the list of query {!r} holds {} ids, the first list {}: without all_ids every list must rank the whole '
                             'gallery.  Pass all_ids (missing ids are then appended in its order), or use the host '
                             'hierarchical_precision, which keeps the reference\'s rule for partial lists without all_ids'
                             .format(q_ids[i], int(lengths[i]), len(g_ids)))
    index = _GalleryIndex(g_ids)
    ng = len(g_ids)
    class_list, (qcls, gcls) = class_indices([labels[i] for i in q_ids], [labels[i] for i in g_ids])
    qidx = index.of_sequence(q_ids).astype(np.int32) if ignore_qids else None
    full = bool((lengths == L).all())

    def index_tile(r0, r1, dev):
        n = r1 - r0
        len_t = torch.from_numpy(lengths[r0:r1])
        if ranking is not None:
            idx = index.of_tensor(ranking[r0:r1].to(dev) if dev.type == 'cuda' else ranking[r0:r1])
        else:
            flat = [i for r in rows[r0:r1] for i in (r.tolist() if isinstance(r, np.ndarray) else r)]
            flat_idx = torch.from_numpy(index.of_sequence(flat))
            if full:
                idx = flat_idx.view(n, L)
            else:
                idx = torch.full((n, L), -1, dtype=torch.int64)
                idx[torch.arange(L)[None, :] < len_t[:, None]] = flat_idx
        idx = idx.to(dev)
        len_d = None if full else len_t.to(dev)
        bad = idx < 0 if full else (idx < 0) & (torch.arange(L, device=dev)[None, :] < len_d[:, None])
        if bool(bad.any()):
            r, c = (int(v) for v in bad.nonzero()[0])
            unknown = ranking[r0 + r, c].item() if ranking is not None else rows[r0 + r][c]
            raise ValueError('id {!r} at position {} of the ranking of query {!r} is not in the gallery of {} ids'
                             .format(unknown, c, q_ids[r0 + r], ng))
        if not full:
            idx = idx.masked_fill(torch.arange(L, device=dev)[None, :] >= len_d[:, None], -1)
        return idx.to(torch.int32), (None if full else len_d.to(torch.int32))

    return RankedProblem(q_ids, g_ids, qcls, gcls, class_list, qidx, L, lengths.astype(np.int32), index_tile)


def ranked_tile_rows(dev, nq, ng, list_len, fixed, row_extra, tile_rows, what):
    """Query rows per tile of an evaluation of given rankings, from what it holds on the device, known before anything is launched:
    ``fixed`` bytes whatever the tile, and per tile row the completed ranking (int32, rows of 16-byte pitch), the index list with
    the temporaries of its id look-up (28 bytes per entry) and ``row_extra`` bytes of results.  Sized from the free device memory the
    way ``class_hierarchy._ranked_gallery_tile_rows`` sizes its tiles; ``tile_rows`` overrides the size, not the check: a problem that
    cannot fit raises ``ValueError`` with the estimate."""
    from class_hierarchy import _free_device_bytes
    row_bytes = 4 * ((ng + 3) // 4 * 4) + 28 * list_len + row_extra
    free = _free_device_bytes(dev)
    budget = None if free is None else free - free // 10
    rows = max(1, nq)
    if tile_rows is not None:
        rows = max(1, min(rows, int(tile_rows)))
    elif budget is not None:
        rows = max(1, min(rows, (budget - fixed) // row_bytes))
        if 128 < rows < nq:
            rows = rows // 128 * 128
    estimate = fixed + rows * row_bytes
    if budget is not None and estimate > budget:
        raise ValueError('{} of {} given rankings over a gallery of {} items needs an estimated {:,} bytes of device memory ({:,} whatever '
                         'the tile, {:,} for a tile of {} query row{}), {:,} are free: fewer classes, shorter lists or a smaller gallery'
                         .format(what, nq, ng, estimate, fixed, estimate - fixed, rows, '' if rows == 1 else 's', free))
    return rows


def _raise_on_bad_rows(status, p, r0):
    """``status`` of ``complete_rankings`` for the tile that starts at query r0: a flagged row raises, naming its query."""
    bad = status.nonzero()
    if int(bad.numel()):
        r = int(bad[0])
        raise ValueError('the ranking of query {!r} names a gallery id more than once{}: it cannot be scored'
                         .format(p.q_ids[r0 + r], '' if not int(status[r]) & 1 else ' or an id outside the gallery'))


def recall_precision_ranked(retrieved, labels, bins=None, ignore_qids=True, all_ids=None, tile_rows=None, kernels=None):
    """The recall-precision curve and mAP of plot_recall_precision.py:52-79 for GIVEN rankings -- from another system, an approximate
    index, re-ranked or truncated lists -- instead of features: ``retrieved``, ``labels``, ``ignore_qids`` and ``all_ids`` as
    ``ranked_problem`` takes them (the reference's dict / generator, or the array form).  Every list is completed to a ranking of the
    whole gallery on the device (``se_complete_rankings``: ids missing from a list follow in ``all_ids`` order; every relevant position
    is needed, so there is no head-only shortcut), tile by tile, then ``se_relevant_positions`` and ``se_recall_precision_reduce`` run
    as in ``recall_precision_device(..., gallery=...)``, with its (class, is-a-gallery-item) reduce groups.  One process, one GPU.
    ``kernels`` (tests): CPU stand-ins ``{'complete_rankings', 'relevant_positions', 'recall_precision_reduce', 'device'}``.
    Returns ``(levels, mean_precision, mAP, per_query_ap)``.  Raises ``ValueError`` for an empty gallery, an id that is not in the
    gallery, a list that names an id twice and partial lists without ``all_ids``."""
    import torch
    kernels = resolve_kernels(kernels, ('complete_rankings', 'relevant_positions', 'recall_precision_reduce', 'device'))
    bins = _number_of_bins(bins)
    p = ranked_problem(retrieved, labels, ignore_qids, all_ids)
    nq, ng, C, dev = len(p.q_ids), len(p.g_ids), len(p.class_list), kernels['device']
    if nq and ng == 0:
        raise ValueError('the gallery is empty')
    # reduce groups as in _recall_precision_gallery: class 2 c + (the query is a gallery item of its class that leaves its ranking)
    gcounts = np.bincount(p.gcls, minlength=C)
    present = (p.qidx >= 0) & (p.gcls[np.maximum(p.qidx, 0)] == p.qcls) if (p.qidx is not None and ng) else np.zeros(nq, dtype=bool)
    rc = 2 * p.qcls.astype(np.int64) + present
    r_rc = np.repeat(gcounts, 2).astype(np.int64)
    r_rc[1::2] -= 1
    r_rc = np.maximum(r_rc, 0)
    nq_rc = np.bincount(rc, minlength=2 * C)
    class_off = np.concatenate([[0], np.cumsum(r_rc)]).astype(np.int64)
    max_r = int(r_rc.max()) if C else 0
    tile_rows = ranked_tile_rows(dev, nq, ng, p.list_len, 8 * int(class_off[-1]), 4 * max_r + 64, tile_rows, 'the recall-precision curve')

    gcls_d, qcls_d = torch.from_numpy(p.gcls).to(dev), torch.from_numpy(p.qcls).to(dev)
    qidx_d = None if p.qidx is None else torch.from_numpy(p.qidx).to(dev)
    class_off_d = torch.from_numpy(class_off).to(dev)
    ap, prec_sum, first_miss, bin_sum, bin_count = _accumulators(nq, max(2 * C, 1), int(class_off[-1]), bins, dev)
    for r0 in range(0, nq, tile_rows):      # each tile is consumed before the next one is made
        r1 = min(nq, r0 + tile_rows)
        lists_d, len_d = p.index_tile(r0, r1, dev)
        rank, status = kernels['complete_rankings'](lists_d, ng, lengths=len_d)
        _raise_on_bad_rows(status, p, r0)
        rc_t = rc[r0:r1]
        hit_off = np.concatenate([[0], np.cumsum(r_rc[rc_t])]).astype(np.int64)
        order = np.argsort(rc_t, kind='stable').astype(np.int32)
        class_start = np.concatenate([[0], np.cumsum(np.bincount(rc_t, minlength=2 * C))]).astype(np.int32)
        hit_off_d = torch.from_numpy(hit_off).to(dev)
        hit_pos = kernels['relevant_positions'](rank, gcls_d, qcls_d[r0:r1].contiguous(), None if qidx_d is None else qidx_d[r0:r1].contiguous(),
                                                hit_off_d, num_classes=C, total=int(hit_off[-1]))
        kernels['recall_precision_reduce'](hit_pos, hit_off_d, torch.from_numpy(order).to(dev), torch.from_numpy(class_start).to(dev),
                                           class_off_d, bins, ap[r0:r1], prec_sum, first_miss, bin_sum, bin_count)
    _warn_singletons(int(nq_rc[r_rc == 0].sum()))
    return _merge_levels(ap.cpu().numpy(), r_rc, nq_rc, class_off, bins, prec_sum, first_miss, bin_sum, bin_count)


def _recall_precision_gallery(features, labels, normalize, bins, ids, kblocks, tile_rows, tile_cols, kernels, gallery, gallery_labels,
                              gallery_ids, distributed, group):
    """``recall_precision_device`` with a separate gallery.  Per query tile (queries sorted by class):

    1. relevant keys: per class of the tile, the distances of its queries to the gathered gallery rows of that class
       (``se_pairwise_dist``: an element's fp32 chain depends on its two rows only, so these are the bits the slabs will hold),
       each row ordered by ``se_rank_rows``; the query's own gallery row is taken out;
    2. counting: (tile x gallery tile) distance slabs -> ``se_count_preceding``, over this rank's shard of the gallery, then ONE
       integer all-reduce of the counts;
    3. ``se_count_to_positions`` -> the input of ``se_recall_precision_reduce``; scan and reduce run on every rank (they cost a
       thousandth of the counting), so all ranks hold the same bits without a float64 collective."""
    import torch
    import torch.distributed as dist
    from sharded_retrieval import shard_bounds

    kernels = resolve_kernels(kernels, RANKING_KERNELS + ('count_preceding', 'count_to_positions', 'recall_precision_reduce', 'device'))
    bins = _number_of_bins(bins)
    qf, gf, _, qcls, gcls, class_list, qidx = gallery_problem(features, labels, ids, gallery, gallery_labels, gallery_ids)
    nq, ng, C, dev = int(qf.shape[0]), int(gf.shape[0]), len(class_list), kernels['device']
    kb = _resolve_kblocks(kblocks, int(qf.shape[1]))
    fq, fg = to_device_f32(qf, dev), to_device_f32(gf, dev)
    if normalize:
        kernels['normalize_rows_'](fq)
        kernels['normalize_rows_'](fg)
        sq_q = sq_g = None
    else:
        sq_q, sq_g = kernels['row_sqnorm'](fq), kernels['row_sqnorm'](fg)
    world = dist.get_world_size(group) if (distributed and dist.is_initialized()) else 1
    g_lo, g_hi = shard_bounds(ng, world)[dist.get_rank(group)] if world > 1 else (0, ng)

    # reduce classes: queries of one class share R only if they agree on being in the gallery -- class 2 c + present
    gcounts = np.bincount(gcls, minlength=C)
    present = (qidx >= 0) & (gcls[np.maximum(qidx, 0)] == qcls) if ng else np.zeros(nq, dtype=bool)
    rc = 2 * qcls.astype(np.int64) + present
    r_rc = np.repeat(gcounts, 2).astype(np.int64)
    r_rc[1::2] -= 1
    r_rc = np.maximum(r_rc, 0)
    nq_rc = np.bincount(rc, minlength=2 * C)
    class_off = np.concatenate([[0], np.cumsum(r_rc)]).astype(np.int64)
    by_class = torch.from_numpy(np.argsort(gcls, kind='stable')).to(dev)                     # gallery rows class by class, ascending inside
    class_at = np.concatenate([[0], np.cumsum(gcounts)])
    members = [by_class[class_at[c]:class_at[c + 1]] for c in range(C)]

    class_off_d = torch.from_numpy(class_off).to(dev)
    ap_sorted, prec_sum, first_miss, bin_sum, bin_count = _accumulators(nq, 2 * C, int(class_off[-1]), bins, dev)

    order_q = np.argsort(rc, kind='stable')
    tile_cols = min(max(ng, 1), int(tile_cols or 65536))
    tile_rows = min(max(nq, 1), int(tile_rows or max(128, (1 << 30) // (4 * tile_cols))))
    slab = None
    if dev.type == 'cuda':       # the grow-only distance buffer ranking_tiles uses: the CLI's next --feat pays no allocation
        slab = _cached_rows('pd', tile_rows, tile_cols, torch.float32, dev)
    for t0 in range(0, nq, tile_rows):
        sel = order_q[t0:t0 + tile_rows]
        rows = len(sel)
        sel_d = torch.from_numpy(sel).to(dev)
        q_rows = fq[sel_d]
        sq_rows = None if sq_q is None else sq_q[sel_d]
        rc_t = rc[sel]
        hit_off = np.concatenate([[0], np.cumsum(r_rc[rc_t])]).astype(np.int64)
        total = int(hit_off[-1])
        qidx_d = torch.from_numpy(qidx[sel]).to(dev)
        class_start = np.concatenate([[0], np.cumsum(np.bincount(rc_t, minlength=2 * C))]).astype(np.int32)
        # ---- 1. the relevant items' keys, class run by class run (the rows of a run are consecutive: the tile is sorted) ----
        rel_d, rel_i = [], []
        for k in np.flatnonzero(np.diff(class_start) > 0):
            if r_rc[k] == 0:
                continue
            a, b = int(class_start[k]), int(class_start[k + 1])
            mem = members[k // 2]
            pd_c = kernels['pairwise_dist'](q_rows[a:b], fg[mem], normalize, None if sq_rows is None else sq_rows[a:b],
                                            None if sq_g is None else sq_g[mem], kb)
            rk = kernels['rank_rows'](pd_c).long()
            d_sorted, i_sorted = torch.gather(pd_c, 1, rk), mem[rk].to(torch.int32)
            if k % 2:        # these queries are gallery items of their own class: that one entry leaves every row
                keep = i_sorted != qidx_d[a:b, None]
                d_sorted, i_sorted = d_sorted[keep], i_sorted[keep]
            rel_d.append(d_sorted.reshape(-1))
            rel_i.append(i_sorted.reshape(-1))
        rel_d = torch.cat(rel_d) if rel_d else torch.zeros(0, dtype=torch.float32, device=dev)
        rel_i = torch.cat(rel_i) if rel_i else torch.zeros(0, dtype=torch.int32, device=dev)
        if int(rel_d.numel()) != total:
            raise RuntimeError('relevant keys: {} found, {} expected (duplicate gallery ids?)'.format(int(rel_d.numel()), total))
        pad = max(total, 1)      # the kernels take no NULL: a tile without any relevant item still passes one element
        rel_d = torch.cat([rel_d, torch.zeros(pad - total, dtype=torch.float32, device=dev)]).contiguous()
        rel_i = torch.cat([rel_i, torch.zeros(pad - total, dtype=torch.int32, device=dev)]).contiguous()
        cnt = torch.zeros(pad, dtype=torch.int32, device=dev)
        hit_off_d = torch.from_numpy(hit_off).to(dev)
        # ---- 2. counting over this rank's gallery rows ----
        max_rel = int(r_rc[rc_t].max()) if rows else 0
        for g0 in range(g_lo, g_hi, tile_cols):
            g1 = min(g_hi, g0 + tile_cols)
            pd = kernels['pairwise_dist'](q_rows, fg[g0:g1], normalize, sq_rows, None if sq_g is None else sq_g[g0:g1], kb,
                                          None if slab is None else slab[:rows, :g1 - g0])
            kernels['count_preceding'](pd, g0, hit_off_d, rel_d, rel_i, qidx_d, cnt, max_rel)
        if world > 1:
            if cnt.is_cuda and dist.get_backend(group) == 'gloo':
                host = cnt.cpu()
                dist.all_reduce(host, group=group)
                cnt.copy_(host)
            else:
                dist.all_reduce(cnt, group=group)
        # ---- 3. positions, AP and the per-class sums ----
        hit_pos = kernels['count_to_positions'](cnt, hit_off_d)
        kernels['recall_precision_reduce'](hit_pos, hit_off_d, torch.arange(rows, dtype=torch.int32, device=dev),
                                           torch.from_numpy(class_start).to(dev), class_off_d, bins, ap_sorted[t0:t0 + rows], prec_sum,
                                           first_miss, bin_sum, bin_count)
    ap_h = np.zeros(nq, dtype=np.float64)
    ap_h[order_q] = ap_sorted.cpu().numpy()
    _warn_singletons(int(nq_rc[r_rc == 0].sum()))
    return _merge_levels(ap_h, r_rc, nq_rc, class_off, bins, prec_sum, first_miss, bin_sum, bin_count)
