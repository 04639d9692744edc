"""Float64 NumPy reference of se_tree_risk_topk and of the mistake metrics that does NOT use the range encoding of
ClassHierarchy.tree_risk_encoding: H[k, j] = heights[lcs(k, j)] comes from explicit ancestor sets (the deepest common ancestor; on a
DAG the pick among equally deep ones is ClassHierarchy.lcs's), the risks are P64 @ H.T, the lists np.lexsort((class, risk)) with NaN
last.  Also the restated range formula on an encoding (what the kernel evaluates, in NumPy's summation order), grid probabilities on
which every sum is exact, and the fixtures by the helpers the HXE tests use."""
import numpy as np

import _hxe_canon as hc
from test_class_embedding_host import load_hierarchy

_TREES = {}


def tree(name):
    """(hierarchy, classes) of a named tree, built once: cifar / cub / ilsvrc / inat400 (a 400-class sample of iNaturalist 2018) /
    wordnet_dag / rand<C> (``_hxe_canon.random_tree(C, 3)``) / c1 / c2 / cat33 and cat33x1000 (``_hxe_canon.caterpillar_tree(33)`` and
    ``(33, 1000)``: paths of every level count up to the 32 a path may hold)."""
    if name not in _TREES:
        if name == "c1":
            h, classes = _hierarchy([(10, 0)]), [0]
        elif name == "c2":
            h, classes = _hierarchy([(10, 0), (10, 1)]), [0, 1]
        elif name.startswith("cat33"):
            h, classes = hc.caterpillar_tree(33, 1000 if name == "cat33x1000" else 0)
        elif name.startswith("rand"):
            h, classes = hc.random_tree(int(name[4:]), 3)
        elif name == "inat400":
            h, classes = load_hierarchy("inat2018")
            classes = [classes[i] for i in np.sort(np.random.default_rng(400).choice(len(classes), 400, replace=False))]
        else:
            h, classes = load_hierarchy(name)
        _TREES[name] = (h, classes)
    return _TREES[name]


def _hierarchy(edges):
    from class_hierarchy import ClassHierarchy
    parents, children = {}, {}
    for p, c in edges:
        parents.setdefault(c, []).append(p)
        children.setdefault(p, []).append(c)
    return ClassHierarchy(parents, children)


def height_table(hierarchy, classes):
    """Integer [C, C]: heights[lcs(a, b)] from explicit descendant sets.  Every node of the ancestor closure writes its height over
    the block (classes below it) x (classes below it), shallow nodes first, so the deepest common ancestor of a pair writes last --
    among equally deep ones (a DAG only) the one of smallest height, which is ``ClassHierarchy.lcs``'s pick.  Built once per tree."""
    key = ("H", id(hierarchy), tuple(classes))
    if key not in _TREES:
        below = {}
        for i, c in enumerate(classes):
            for n in hierarchy.all_hypernym_depths(c):
                below.setdefault(n, []).append(i)
        C = len(classes)
        H = np.full((C, C), -1, dtype=np.int16 if C > 2000 else np.int64)
        for n in sorted(below, key=lambda n: (hierarchy.depth(n), -hierarchy.heights[n])):
            idx = np.asarray(below[n])
            H[idx[:, None], idx[None, :]] = hierarchy.heights[n]
        assert H.min() >= 0, "two classes without a common ancestor"
        _TREES[key] = H
    return _TREES[key]


def risks(P, H, own_h=None):
    """float64 [N, C]: risk[i, k] = sum_j P[i, j] * H[k, j] (``own_h``: in place of H's diagonal); a row with a NaN or an infinity is
    all NaN (the kernel's explicit rule)."""
    P = np.asarray(P, dtype=np.float64)
    R = np.empty(P.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, H.shape[0], 1024):
            R[:, k0:k0 + 1024] = P @ np.asarray(H[k0:k0 + 1024], dtype=np.float64).T
        if own_h is not None:
            R += (np.asarray(own_h, dtype=np.float64) - np.diagonal(H)) * P
    R[~np.isfinite(P).all(axis=1)] = np.nan
    return R


def lists(R, top):
    """(cls int32 [N, top], risk [N, top]): ascending (risk, class index), -0 == +0, NaN last."""
    R = np.asarray(R, dtype=np.float64)
    order = np.stack([np.lexsort((np.arange(R.shape[1]), np.where(np.isnan(r), 0.0, r + 0.0), np.isnan(r))) for r in R])[:, :top]
    return order.astype(np.int32), np.take_along_axis(R, order, axis=1)


def range_formula(P, enc):
    """The formula of include/sehip.h on an encoding, float64 [N, C]: one prefix sum (np.cumsum) of the row in depth-first order,
    every mass a difference of two of its entries."""
    P = np.asarray(P, dtype=np.float64)
    N, C = P.shape
    q = np.zeros((N, C))
    q[:, enc["pos"]] = P
    S = np.concatenate([np.zeros((N, 1)), np.cumsum(q, axis=1)], axis=1)
    R = np.empty((N, C))
    for k in range(C):
        r, below = enc["own_h"][k] * P[:, k], P[:, k]
        for e in range(enc["path_off"][k], enc["path_off"][k + 1]):
            m = S[:, enc["lvl_hi"][e]] - S[:, enc["lvl_lo"][e]]
            r = r + enc["lvl_h"][e] * (m - below)
            below = m
        R[:, k] = r
    return R


def grid_probs(N, C, seed):
    """float32 [N, C]: integers in [0, 64) / 1024 -- every product with a height and every sum of a row is exact in float64 (and in
    float32 up to C * 64 * H_max < 2^24), whatever the order, so that equal risks are equal bits: ties are reachable."""
    return (np.random.default_rng(seed).integers(0, 64, size=(N, C)) / 1024.0).astype(np.float32)


def softmax_probs(N, C, seed):
    """float32 [N, C]: the float32 softmax of 3 * randn logits."""
    z = (3.0 * np.random.default_rng(seed).standard_normal((N, C))).astype(np.float32).astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def risk_bound(P, C, L, H_max):
    """Per row: 8 (C + 2)(L + 1) H_max 2^-53 sum_j |p_j| (tests/test_gpu_tree_risk.py derives it)."""
    return 8.0 * (C + 2) * (L + 1) * H_max * 2.0 ** -53 * np.abs(np.asarray(P, dtype=np.float64)).sum(axis=1)


def metrics(pred, y, H, ks):
    """Plain-loop statement of mistakes.mistake_metrics."""
    out = {}
    wrong = [int(H[t, p[0]]) for p, t in zip(pred, y) if p[0] != t]
    if wrong:
        out["Mistake Severity"] = sum(wrong) / len(wrong)
    for k in ks:
        out["Hier. Dist@%d" % k] = sum(int(H[t, c]) for p, t in zip(pred, y) for c in p[:k]) / (k * len(y))
    return out
