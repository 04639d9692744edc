"""Recall-precision curve and mAP on the MI355X (se_relevant_positions, se_recall_precision_reduce, recall_precision_device and
the plot_recall_precision.py CLI) against the canonical ranking of the oracle and the golden values of the reference's own
script (tests/golden/recprec_*.npz, written by tools/make_recprec_golden.py)."""
import functools
import glob
import os
import pickle
import tempfile
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p)[len("recprec_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "recprec_*.npz")))


@functools.lru_cache(maxsize=8)
def _canon(n, d, normalize, seed):
    from oracle import retrieval_oracle as ro
    f = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return ro.canon_retrieval(f, normalize)[1]


def _positions(rank, cls, qcls, qidx):
    """(hit_off, hit_pos) of the rows of `rank`, in NumPy."""
    offs, out = [0], []
    for i in range(len(rank)):
        row = rank[i] if qidx is None else rank[i][rank[i] != qidx[i]]
        p = np.flatnonzero(cls[row] == qcls[i]) + 1
        out.append(p)
        offs.append(offs[-1] + len(p))
    return np.array(offs, dtype=np.int64), (np.concatenate(out) if out else np.zeros(0)).astype(np.int32)


def _run_positions(rank, cls, with_qidx, r16=False, C=None):
    import sehip
    n = rank.shape[1]
    qidx = np.arange(len(rank), dtype=np.int32) if with_qidx else None
    hit_off, want = _positions(rank, cls, cls[:len(rank)], qidx)
    rk = torch.from_numpy(rank.astype(np.uint16).view(np.int16) if r16 else rank.astype(np.int32)).cuda()
    got = sehip.relevant_positions(rk, torch.from_numpy(cls).cuda(), torch.from_numpy(cls[:len(rank)].copy()).cuda(),
                                   None if qidx is None else torch.from_numpy(qidx).cuda(), torch.from_numpy(hit_off).cuda(),
                                   num_classes=C)
    torch.cuda.synchronize()
    return hit_off, want, got.cpu().numpy()


# (N, classes): single items, one / two partial chunks, 2048-rank chunk edges, C > 256 (16-bit LDS table), a final partial chunk
GRID = [(1, 1), (2, 1), (2, 2), (255, 3), (256, 7), (257, 300), (2048, 4), (2049, 9), (4097, 2), (4097, 256), (10000, 1000), (10000, 5)]


@pytest.mark.parametrize("n,c", GRID)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("with_qidx", [True, False])
def test_relevant_positions_bit_exact(n, c, normalize, with_qidx):
    rank = _canon(n, 8, normalize, n)
    cls = np.random.default_rng(n + c).integers(0, c, size=n).astype(np.int32)
    hit_off, want, got = _run_positions(rank, cls, with_qidx, C=c)
    assert np.array_equal(got, want), (n, c)
    if n == 4097 and c == 2:
        last = want[hit_off[1:][hit_off[1:] > hit_off[:-1]] - 1]
        assert (last > 4096 - (1 if with_qidx else 0)).any()          # some rows end in the final, one-rank chunk


@pytest.mark.parametrize("n,c", [(257, 3), (4097, 300), (10000, 2)])
def test_relevant_positions_r16_and_row_subset(n, c):
    """uint16 rankings give the same positions; a tile of rows (queries r0 ..) with a row pitch larger than the list."""
    rank = _canon(n, 8, True, n)
    cls = np.random.default_rng(c).integers(0, c, size=n).astype(np.int32)
    for r16 in (False, True):
        _, want, got = _run_positions(rank, cls, True, r16=r16, C=c)
        assert np.array_equal(got, want)
    import sehip
    r0, rows = n // 3, min(100, n - n // 3)
    padded = np.zeros((rows, n + 5), dtype=np.int32)
    padded[:, :n] = rank[r0:r0 + rows]
    qidx = np.arange(r0, r0 + rows, dtype=np.int32)
    hit_off, want = _positions(rank[r0:r0 + rows], cls, cls[r0:r0 + rows], qidx)
    rk = torch.from_numpy(padded).cuda()[:, :n]
    got = sehip.relevant_positions(rk, torch.from_numpy(cls).cuda(), torch.from_numpy(cls[r0:r0 + rows].copy()).cuda(),
                                   torch.from_numpy(qidx).cuda(), torch.from_numpy(hit_off).cuda())
    assert np.array_equal(got.cpu().numpy(), want)


def _misaligned(a):
    """`a` on the device as a view that starts one element into its buffer: contiguous, 4 bytes off the allocator's alignment."""
    buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda")
    buf[1:].copy_(torch.from_numpy(a))
    return buf[1:]


# class source of relpos_kernel (csrc/rank_stream.h): (classes, query rows) -- byte table, 16-bit table, global gather (5 rows:
# list_len * rows < 8 * gallery, no table is filled)
CLASS_SOURCES = {"byte_table": (3, None), "short_table": (300, None), "gather": (3, 5)}


@pytest.mark.parametrize("n", [2047, 2048, 2049])
@pytest.mark.parametrize("source", sorted(CLASS_SOURCES))
def test_relevant_positions_every_class_source(n, source):
    """Every relpos_kernel<CLSW, RT>: one 2048-rank chunk and one rank either side of it (2047 / 2049: a gallery that is no multiple
    of 4, rows that take the element loads; 2048: the vector loads), int32 and uint16 rankings, `cls` 16-byte aligned (the table
    fill's 16-byte loads) and as a view one element into its buffer (its scalar loads): the oracle's positions, bit for bit."""
    import sehip
    c, rows = CLASS_SOURCES[source]
    r0 = 0 if rows is None else n // 3
    rows = n if rows is None else rows
    rank = _canon(n, 8, True, n)[r0:r0 + rows]
    cls = np.random.default_rng(n + c).integers(0, c, size=n).astype(np.int32)
    qcls, qidx = cls[r0:r0 + rows].copy(), np.arange(r0, r0 + rows, dtype=np.int32)
    hit_off, want = _positions(rank, cls, qcls, qidx)
    assert (rank.shape[1] * min(rows, 4096) < 8 * n) == (source == "gather")          # the kernel's rule for leaving the table out
    for cls_dev in (torch.from_numpy(cls).cuda(), _misaligned(cls)):
        assert (cls_dev.data_ptr() % 16 == 0) == (cls_dev.storage_offset() == 0) and cls_dev.is_contiguous()
        for r16 in (False, True):
            rk = torch.from_numpy(rank.astype(np.uint16).view(np.int16) if r16 else rank.astype(np.int32)).cuda()
            got = sehip.relevant_positions(rk, cls_dev, torch.from_numpy(qcls).cuda(), torch.from_numpy(qidx).cuda(),
                                           torch.from_numpy(hit_off).cuda(), num_classes=c)
            assert np.array_equal(got.cpu().numpy(), want), (n, source, cls_dev.storage_offset(), r16)


def _hierarchy():
    from class_hierarchy import ClassHierarchy
    g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for p, c in g["edges"]:
            f.write("%d %d\n" % (p, c))
    h = ClassHierarchy.from_file(f.name, id_type=int)
    os.unlink(f.name)
    return h, g


@pytest.mark.parametrize("normalize", [True, False])
def test_ap_matches_the_hierarchical_precision_kernel(normalize):
    """Per-query AP of se_recall_precision_reduce == the AP column of se_hierarchical_precision (two independent kernels)."""
    from recall_precision import recall_precision_device
    h, g = _hierarchy()
    labels = g["labels"].tolist()
    _, per_q = h.hierarchical_precision_device(g["features"].copy(), labels, [1], compute_ap=True, normalize=normalize)
    _, _, mAP, aps = recall_precision_device(g["features"].copy(), labels, normalize=normalize)
    want = np.array([per_q["AP"][i] for i in range(len(labels))])
    assert np.abs(aps - want).max() <= 1e-12
    assert abs(mAP - want.mean()) <= 1e-12


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_curves(name):
    """recall_precision_device == the reference's plot_recall_precision.py: levels equal as float64, means and mAP to 1e-12; the
    same bits on a second call and with class-splitting tiles."""
    from recall_precision import recall_precision_device
    g = np.load(os.path.join(GOLDEN, "recprec_%s.npz" % name))
    norm = bool(g["normalize"])
    for b in g["bins"].tolist():
        res = [recall_precision_device(g["features"].copy(), g["labels"].tolist(), normalize=norm, bins=b or None, tile_rows=t)
               for t in (None, None, 100)]
        levels, means, mAP, aps = res[0]
        assert np.array_equal(levels, g["levels_%d" % b]), (name, b)
        assert np.abs(means - g["means_%d" % b]).max() <= 1e-12, (name, b)
        assert abs(mAP - g["aps_%d" % b].mean()) <= 1e-12
        assert np.abs(aps - g["aps_%d" % b]).max() <= 1e-12
        for other in res[1:]:                           # deterministic, and independent of the tiling
            assert np.array_equal(other[0], levels) and np.array_equal(other[1], means) and np.array_equal(other[3], aps)
            assert other[2] == mAP


def test_cli_end_to_end(tmp_path):
    """plot_recall_precision.py on synthetic:100x8x64x300 with a dict feature dump: --csv (and --save when matplotlib imports)
    against recall_precision_host on the oracle's ranking."""
    import plot_recall_precision as prp
    from datasets import get_data_generator
    from oracle import retrieval_oracle as ro
    from recall_precision import recall_precision_host
    labels_test = get_data_generator("synthetic:100x8x64x300", "unused").labels_test
    rng = np.random.default_rng(11)
    ids = rng.permutation(300).tolist()
    centers = rng.standard_normal((100, 16)).astype(np.float32)
    feats = {i: (centers[labels_test[i]] + 0.8 * rng.standard_normal(16)).astype(np.float32) for i in ids}
    path = str(tmp_path / "emb.pickle")
    with open(path, "wb") as f:
        pickle.dump({"feat": feats}, f)
    argv = ["--dataset", "synthetic:100x8x64x300", "--data_root", "unused", "--feat", path, "--norm", "yes", "--bins", "10",
            "--csv", str(tmp_path / "out.csv")]
    try:
        import matplotlib  # noqa: F401
        argv += ["--save", str(tmp_path / "curve.png")]
    except ImportError:
        pass
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # singleton classes among 300 images of 100 classes
        got = prp.main(argv)["emb"]
        rank = ro.canon_retrieval(np.stack([feats[i] for i in ids]), True)[1]
        want = recall_precision_host(rank, [labels_test[i] for i in ids], bins=10)
    assert np.array_equal(got[0], want[0]) and np.abs(got[1] - want[1]).max() <= 1e-12 and abs(got[2] - want[2]) <= 1e-12
    rows = (tmp_path / "out.csv").read_text().splitlines()
    assert rows[0] == "feature,level,mean_precision" and len(rows) == 1 + len(want[0])
    assert np.array_equal(np.array([float(r.split(",")[1]) for r in rows[1:]]), want[0])
    if "--save" in argv:
        assert (tmp_path / "curve.png").stat().st_size > 0


def test_50k():
    """50,000 x 50,000, D = 100, ~90 classes: positions of 64 sampled queries == canon.c's rankings of those rows; mAP == the mean
    of the hierarchical-precision path's AP column."""
    import sehip
    from evaluate_retrieval import ranking_tiles
    from oracle import retrieval_oracle as ro
    from recall_precision import recall_precision_device
    h, g = _hierarchy()
    classes = np.unique(g["labels"])
    rng = np.random.default_rng(50)
    n, d = 50000, 100
    lab_idx = rng.integers(0, len(classes), size=n)
    feats = (rng.standard_normal((len(classes), d)) * 0.5)[lab_idx] + rng.standard_normal((n, d))
    feats = feats.astype(np.float32)
    labels = classes[lab_idx].tolist()
    cls = lab_idx.astype(np.int32)
    counts = np.bincount(cls, minlength=len(classes))
    hit_off = np.concatenate([[0], np.cumsum(counts[cls] - 1)]).astype(np.int64)
    sample = np.sort(rng.choice(n, size=64, replace=False))
    f_dev = torch.from_numpy(feats).cuda()
    for r0, tile in ranking_tiles(f_dev, True):
        assert r0 == 0 and tile.shape[0] == n
        hp = sehip.relevant_positions(tile, torch.from_numpy(cls).cuda(), torch.from_numpy(cls).cuda(),
                                      torch.arange(n, dtype=torch.int32, device="cuda"), torch.from_numpy(hit_off).cuda(),
                                      num_classes=len(classes), total=int(hit_off[-1])).cpu().numpy()
    fn = ro.canon_normalize_rows(feats)
    rank_s = ro.canon_rank_rows(ro.canon_pdist(fn[sample], fn, ro.METRIC_COSINE))
    for k, q in enumerate(sample):
        row = rank_s[k][rank_s[k] != q]
        want = np.flatnonzero(cls[row] == cls[q]) + 1
        assert np.array_equal(hp[hit_off[q]:hit_off[q + 1]], want), q
    _, _, mAP, _ = recall_precision_device(feats, labels, normalize=True)
    means, _ = h.hierarchical_precision_device(feats.copy(), labels, [1], compute_ap=True, normalize=True, per_query=False)
    assert abs(mAP - means["AP"]) <= 1e-12
