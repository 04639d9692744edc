"""How bad are a classifier's mistakes: mistake severity, the hierarchical distance of the top-k predictions, and conditional risk
minimisation (CRM) decoding on the class hierarchy -- extensions of this build, the reference has none of them.  They are the
yardsticks of the hierarchy-aware losses of learn_classifier.py (``--loss hxe`` / ``soft_labels``): Bertinetto et al., "Making
Better Mistakes" (CVPR 2020) report the first two, Karthik et al., "No Cost Likelihood Manipulation at Test Time for Making Better
Mistakes in Deep Networks" (ICLR 2021) the CRM baseline every such loss has to be read against.

All values are in LEVELS: ``height(lcs(a, b))`` as an integer, not divided by the height of the hierarchy (which is what
``ClassHierarchy.lcs_height`` and the "Hierarchical Accuracy" column of evaluate_classification_accuracy.py do).
"""
from collections import OrderedDict

import numpy as np

DENSE_TILE_ROWS = 8192      # rows of one distance slab of the dense CRM path


def crm_classification(probs, hierarchy, classes, top=5, kernels=None):
    """CRM decoding: for every row of class probabilities ``probs`` [N, C] (float32 array or device tensor) the ``top`` classes
    of smallest expected LCS height ``sum_j p_j * height(lcs(k, j))``, best first, ties in ascending class index: NumPy int32
    ``[N, top]`` -- ``evaluate`` and ``mistake_metrics`` take it as it is.

    Where ``classes`` span a tree of at most ``sehip.TREE_RISK_MAX_CLASSES`` classes this is ONE ``se_tree_risk_topk`` launch on
    ``hierarchy.tree_risk_encoding``: float64 risks, O(C * levels) per row.  A DAG or a forest (``ValueError`` from the encoding) and
    larger C take the dense path on the existing kernels: ``sehip.pairwise_dist(P, -H, METRIC_COSINE)`` -- its ``-(p . (-h_k))`` is
    the float32 FMA chain of the risk -- in slabs of ``DENSE_TILE_ROWS`` rows, then ``sehip.topk_rows``.  The two paths agree
    wherever two risks of a row differ by more than the float32 chain's round-off.
    ``kernels`` (tests): CPU stand-ins ``{'tree_risk_topk', 'pairwise_dist', 'topk_rows', 'height_table', 'device'}``;
    ``pairwise_dist`` with the adapter signature of ``evaluate_retrieval.resolve_kernels``."""
    import torch
    import sehip
    from evaluate_retrieval import resolve_kernels
    classes = list(classes)
    C, top = len(classes), int(top)
    if top < 1 or top > min(C, sehip.TREE_RISK_TOP_MAX):
        raise ValueError('top must lie in [1, min(C = {}, {})], got {}'.format(C, sehip.TREE_RISK_TOP_MAX, top))
    if int(probs.shape[1]) != C:
        raise ValueError('the probabilities have {} columns, there are {} classes'.format(probs.shape[1], C))
    kernels = resolve_kernels(kernels, ('tree_risk_topk', 'pairwise_dist', 'topk_rows', 'device'))
    dev = kernels['device']
    P = (probs.detach().to(device=dev, dtype=torch.float32) if torch.is_tensor(probs)
         else torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).to(dev))
    if P.dim() != 2 or P.stride(1) != 1:
        P = P.reshape(P.shape[0], -1).contiguous()
    encoding = None
    if C <= sehip.TREE_RISK_MAX_CLASSES:
        try:
            encoding = hierarchy.tree_risk_encoding(classes)
        except ValueError:
            encoding = None
    if encoding is not None:
        return kernels['tree_risk_topk'](P, encoding, top)[0].cpu().numpy()
    height_table = kernels.get('height_table') or hierarchy.height_table
    negH = -height_table(classes, device=dev).to(torch.float32)
    out = np.empty((P.shape[0], top), dtype=np.int32)
    for r0 in range(0, int(P.shape[0]), DENSE_TILE_ROWS):
        slab = kernels['pairwise_dist'](P[r0:r0 + DENSE_TILE_ROWS], negH, True, None, None, None, None)
        out[r0:r0 + DENSE_TILE_ROWS] = kernels['topk_rows'](slab, top)[1].cpu().numpy()
    return out


def mistake_metrics(pred_lists, y_true, height_table, ks=(1, 5, 20)):
    """``OrderedDict`` of the mistake metrics of class lists ``pred_lists`` [N, >= max(ks)] (or [N] top-1 predictions with
    ``ks == [1]``) against the labels ``y_true`` [N], with ``h = height_table`` the integer [C, C] table of
    ``ClassHierarchy.height_table`` (device tensor or array):

    * ``'Mistake Severity'``: mean of ``h(y, pred_0)`` over the samples with ``pred_0 != y``; absent when there is no mistake.
    * ``'Hier. Dist@K'`` per K: mean over the samples of the mean of ``h(y, pred_i)``, ``i < K``.

    In levels.  Integer sums and one division each, so the values are exactly reproducible."""
    import torch
    ks = [int(k) for k in ks]
    pred = np.asarray(pred_lists)
    if pred.ndim == 1:
        pred = pred[:, None]
    y = np.asarray(y_true).astype(np.int64)
    kmax = max(ks) if ks else 1
    if pred.shape[0] != y.shape[0] or min(ks + [1]) < 1 or kmax > pred.shape[1]:
        raise ValueError('ks {} need lists of at least {} classes for {} samples, got {}'.format(ks, kmax, y.shape[0], pred.shape))
    pred = pred[:, :kmax].astype(np.int64)
    if torch.is_tensor(height_table):
        dev = height_table.device
        h = height_table[torch.from_numpy(y).to(dev)[:, None], torch.from_numpy(pred).to(dev)].cpu().numpy()
    else:
        h = np.asarray(height_table)[y[:, None], pred]
    h = h.astype(np.int64)
    out = OrderedDict()
    wrong = pred[:, 0] != y
    if wrong.any():
        out['Mistake Severity'] = int(h[wrong, 0].sum()) / int(wrong.sum())
    for k in ks:
        out['Hier. Dist@{}'.format(k)] = int(h[:, :k].sum()) / (k * len(y))
    return out


def metric_names(ks):
    """The table columns of ``mistake_metrics(..., ks)``."""
    return ['Mistake Severity'] + ['Hier. Dist@{}'.format(int(k)) for k in ks]
