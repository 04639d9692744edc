"""CPU stand-ins of the kernels behind query-vs-gallery evaluation (tests/test_query_gallery_host.py, the gloo test): the contracts of
se_count_preceding / se_count_to_positions in NumPy, next to the stand-ins the existing host tests use for ranking and metrics."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def canon_keys(d, idx):
    """uint64 image of the canonical order: distance ascending (NaN last, -0 == +0), then index."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    u = d.view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    k = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    k = np.where(np.isnan(d), 0xFFFFFFFF, k).astype(np.uint64)
    return (k << np.uint64(32)) | (np.asarray(idx).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)


def count_preceding(pd, col_offset, hit_off, rel_d, rel_i, qidx, cnt, max_rel=0):
    pd_h, off = pd.numpy(), hit_off.numpy()
    rd, ri, c = rel_d.numpy(), rel_i.numpy(), cnt.numpy()          # c shares cnt's memory
    cols = col_offset + np.arange(pd_h.shape[1], dtype=np.int64)
    for i in range(pd_h.shape[0]):
        a, b = int(off[i]), int(off[i + 1])
        if b == a:
            continue
        p = np.searchsorted(canon_keys(rd[a:b], ri[a:b]), canon_keys(pd_h[i], cols), side="left")
        keep = p < b - a
        if qidx is not None:
            keep &= cols != int(qidx[i])
        np.add.at(c, a + p[keep], 1)
    return cnt


def count_to_positions(cnt, hit_off, out=None):
    c, off = cnt.numpy(), hit_off.numpy()
    for i in range(len(off) - 1):
        c[off[i]:off[i + 1]] = np.cumsum(c[off[i]:off[i + 1]])
    return cnt


def ranked_positions(pd, qcls, gcls, qidx):
    """The positions read off a stable full ranking: per query the 1-based places (query removed) of the items of its class."""
    from oracle import retrieval_oracle as ro
    rank = ro.canon_rank_rows(np.ascontiguousarray(pd, dtype=np.float32))
    out = []
    for i in range(len(rank)):
        row = rank[i][rank[i] != qidx[i]]
        out.append((np.flatnonzero(gcls[row] == qcls[i]) + 1).astype(np.int32))
    return out


def cpu_kernels(cosine):
    """Every stand-in the gallery paths of recall_precision_device / hierarchical_precision_device look up."""
    from oracle import retrieval_oracle as ro
    from test_dp_gloo import _hprec_standin
    from test_recprec_host import _cpu_kernels as recprec_kernels
    metric = ro.METRIC_COSINE if cosine else ro.METRIC_EUCLID

    def normalize_rows_(x):
        x.copy_(torch.from_numpy(ro.canon_normalize_rows(x.numpy())))
        return x

    def pairwise_dist(a, b, cos, sqa, sqb, kblocks, out=None):
        assert bool(cos) == bool(cosine)
        return torch.from_numpy(ro.canon_pdist(a.numpy(), b.numpy(), metric, kblocks=kblocks))

    def local_topk(q, g, k, off, kblocks=None):
        qn, gn = (ro.canon_normalize_rows(q.numpy()), ro.canon_normalize_rows(g.numpy())) if cosine else (q.numpy(), g.numpy())
        d, i = ro.canon_topk_rows(ro.canon_pdist(qn, gn, metric, kblocks=kblocks), k, col_offset=off)
        return torch.from_numpy(d), torch.from_numpy(i)

    def merge(d, i):
        md, mi = ro.canon_topk_merge(d.numpy(), i.numpy())
        return torch.from_numpy(md), torch.from_numpy(mi)

    return {"normalize_rows_": normalize_rows_, "row_sqnorm": lambda x: torch.from_numpy(ro.canon_row_sqsum(x.numpy())),
            "pairwise_dist": pairwise_dist, "rank_rows": lambda pd: torch.from_numpy(ro.canon_rank_rows(pd.numpy())),
            "count_preceding": count_preceding, "count_to_positions": count_to_positions,
            "recall_precision_reduce": recprec_kernels()["recall_precision_reduce"], "hierarchical_precision": _hprec_standin,
            "local_topk": local_topk, "merge": merge, "device": torch.device("cpu")}


def load_fixture():
    return np.load(os.path.join(GOLDEN, "qg_retrieval.npz"))


def fixture_arguments(g):
    """(queries, labels mapping, keyword arguments naming the gallery) of the fixture, as the two device functions take them."""
    labels = {int(i): int(c) for i, c in zip(g["gallery_ids"], g["gallery_labels"])}
    labels.update({int(i): int(c) for i, c in zip(g["query_ids"], g["query_labels"])})
    return g["queries"].copy(), labels, {"ids": g["query_ids"].tolist(), "gallery": g["gallery"].copy(), "gallery_ids": g["gallery_ids"].tolist()}


def cifar_hierarchy():
    from class_hierarchy import ClassHierarchy
    parents, children = {}, {}
    for p, c in np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))["edges"].tolist():
        parents.setdefault(c, []).append(p)
        children.setdefault(p, []).append(c)
    return ClassHierarchy(parents, children)
