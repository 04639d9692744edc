"""Query-vs-gallery retrieval evaluation on the MI355X: se_count_preceding + se_count_to_positions against se_rank_rows +
se_relevant_positions on the same rectangular distance matrix, the two device functions against the values of the imported
reference (tests/golden/qg_retrieval.npz, tools/make_qg_golden.py), the all-pairs path on a square problem, and the CLIs."""
import functools
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import _qg_standins as qg

pytestmark = pytest.mark.gpu

SENTINEL = 12345


@functools.lru_cache(maxsize=None)
def _problem(q, n, big_class):
    """Distances [q, n] with NaN of both signs, +0 / -0, +inf and 40 identical gallery columns (as 40 identical gallery rows give);
    gallery classes (``big_class``: all but 100 items in class 0), query classes (one of them absent from the gallery)."""
    rng = np.random.default_rng(1000 * q + n)
    pd = rng.standard_normal((q, n)).astype(np.float32)
    if n >= 64:
        same = rng.choice(n, size=40, replace=False)
        pd[:, same] = pd[:, same[:1]]
    special = np.array([0.0, -0.0, np.nan, -np.nan, np.inf], dtype=np.float32)
    at = rng.random((q, n)) < 0.1
    pd[at] = rng.choice(special, size=int(at.sum()))
    classes = 4
    gcls = rng.integers(0, classes, size=n).astype(np.int32)
    if big_class:
        gcls[:] = 0
        gcls[rng.choice(n, size=100, replace=False)] = rng.integers(1, classes, size=100)
    qcls = rng.integers(0, classes + 1, size=q).astype(np.int32)
    qcls[0] = 0
    if q > 2:
        qcls[1] = classes                       # nothing relevant: R = 0
    mixed = np.where(rng.random(q) < 0.5, rng.integers(0, n, size=q), -1).astype(np.int32)
    return pd, qcls, gcls, mixed


def _ranked(pd_d, qcls, gcls, qidx):
    """se_rank_rows + se_relevant_positions through _lib.call -> (rank on the host, hit_off, positions)."""
    import sehip
    from sehip._lib import call
    q, n = pd_d.shape
    sehip.rank_rows_init()
    rank = torch.empty((q, n), dtype=torch.int32, device="cuda")
    ws = torch.empty((max(int(call("se_rank_rows_workspace_bytes", q, n)), 16),), dtype=torch.uint8, device="cuda")
    call("se_rank_rows", pd_d, pd_d.stride(0), q, n, rank, 0, n, ws, ws.numel())
    own = np.full(q, -1, dtype=np.int32) if qidx is None else qidx
    R = np.array([int((gcls == qcls[i]).sum()) - int(own[i] >= 0 and gcls[own[i]] == qcls[i]) for i in range(q)])
    hit_off = torch.from_numpy(np.concatenate([[0], np.cumsum(R)]).astype(np.int64)).cuda()
    total = int(R.sum())
    pos = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    call("se_relevant_positions", rank, n, q, n, torch.from_numpy(gcls).cuda(), n, torch.from_numpy(qcls).cuda(),
         None if qidx is None else torch.from_numpy(qidx).cuda(), int(max(gcls.max(), qcls.max())) + 1, hit_off, pos)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), hit_off, pos.cpu().numpy()[:total]


SHAPES = [(37, 301, False), (3, 9100, True), (1, 1, False), (5, 1, False), (5, 63, False), (5, 64, False), (5, 65, False), (5, 257, False)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("tiles", [1, 2, 5])
@pytest.mark.parametrize("qidx_mode", ["null", "absent", "mixed"])
@pytest.mark.parametrize("q,n,big_class", SHAPES)
def test_counted_positions_equal_ranked_positions(q, n, big_class, qidx_mode, tiles, pad):
    from sehip._lib import call
    pd, qcls, gcls, mixed = _problem(q, n, big_class)
    qidx = {"null": None, "absent": np.full(q, -1, dtype=np.int32), "mixed": mixed}[qidx_mode]
    buf = torch.full((q, n + pad), float("nan"), dtype=torch.float32, device="cuda")      # ldp > n_cols when pad
    buf[:, :n] = torch.from_numpy(pd).cuda()
    pd_d = buf[:, :n]
    rank, hit_off, want = _ranked(pd_d, qcls, gcls, qidx)
    # the relevant items' keys in canonical order: read off the ranking, as the driver reads them off se_rank_rows on the class block
    off_h = hit_off.cpu().numpy()
    rel_i = []
    for i in range(q):
        row = rank[i] if qidx is None else rank[i][rank[i] != qidx[i]]
        rel_i.append(row[gcls[row] == qcls[i]])
        assert len(rel_i[-1]) == off_h[i + 1] - off_h[i]
    total = int(off_h[-1])
    rel_i_h = np.concatenate(rel_i).astype(np.int32) if total else np.zeros(0, dtype=np.int32)
    rel_d_h = np.concatenate([pd[i, r] for i, r in enumerate(rel_i)]).astype(np.float32) if total else np.zeros(0, dtype=np.float32)
    rel_i_d = torch.from_numpy(np.concatenate([rel_i_h, np.zeros(1, np.int32)])).cuda()
    rel_d_d = torch.from_numpy(np.concatenate([rel_d_h, np.zeros(1, np.float32)])).cuda()
    qidx_d = None if qidx is None else torch.from_numpy(qidx).cuda()
    bounds = np.linspace(0, n, min(tiles, n) + 1).astype(int)
    runs = []
    for _ in range(2):
        cnt = torch.full((total + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        cnt[:total] = 0
        for c0, c1 in zip(bounds[:-1], bounds[1:]):
            slab = pd_d[:, c0:c1]               # a column tile: non-zero col_offset, unaligned base for odd c0
            call("se_count_preceding", slab, slab.stride(0), q, int(c1 - c0), int(c0), hit_off, rel_d_d, rel_i_d, qidx_d, 0, cnt)
        call("se_count_to_positions", cnt, hit_off, q, cnt)
        torch.cuda.synchronize()
        runs.append(cnt.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])                           # a second run: identical bytes
    assert np.array_equal(runs[0][:total], want), (q, n, qidx_mode, tiles)
    assert (runs[0][total:] == SENTINEL).all()                        # nothing outside the queries' bins is written


def test_announced_list_length_only_changes_the_path():
    """max_rel below the real list length: those rows take the global-memory search -- the same counts."""
    from sehip._lib import call
    pd, qcls, gcls, _ = _problem(37, 301, False)
    pd_d = torch.from_numpy(pd).cuda()
    rank, hit_off, want = _ranked(pd_d, qcls, gcls, None)
    rel_i = np.concatenate([rank[i][gcls[rank[i]] == qcls[i]] for i in range(37)]).astype(np.int32)
    rel_d = np.concatenate([pd[i, rank[i][gcls[rank[i]] == qcls[i]]] for i in range(37)]).astype(np.float32)
    for max_rel in (0, 2, 10 ** 6):
        cnt = torch.zeros(len(want), dtype=torch.int32, device="cuda")
        call("se_count_preceding", pd_d, 301, 37, 301, 0, hit_off, torch.from_numpy(rel_d).cuda(), torch.from_numpy(rel_i).cuda(), None, max_rel, cnt)
        call("se_count_to_positions", cnt, hit_off, 37, cnt)
        assert np.array_equal(cnt.cpu().numpy(), want), max_rel


@pytest.mark.parametrize("name,normalize", [("cosine", True), ("euclid", False)])
def test_fixture_parity(name, normalize):
    """Both device functions against the imported reference: P@k / AHP@250 (WUP and LCS_HEIGHT) to 1e-10 (the bound of
    tests/test_gpu_dropin.py against its tie-free hierarchy fixture); levels equal, means / mAP / per-query AP to 1e-12 (the bounds
    of tests/test_gpu_recprec.py)."""
    from recall_precision import recall_precision_device
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    names = g[name + "_metric_names"].tolist()
    want = dict(zip(names, g[name + "_per_query"]))
    for tile_rows, tile_cols in ((None, None), (16, 100)):
        means, per_query = qg.cifar_hierarchy().hierarchical_precision_device(
            queries.copy(), labels, g["ks"].tolist(), compute_ahp=int(g["ahp_clip"]), compute_ap=True, normalize=normalize,
            tile_rows=tile_rows, tile_cols=tile_cols, **kw)
        assert set(means) == set(names)
        for m in names:
            got = np.array([per_query[m][i] for i in g["query_ids"].tolist()])
            assert np.abs(got - want[m]).max() <= (1e-12 if m == "AP" else 1e-10), (m, np.abs(got - want[m]).max())
            assert abs(means[m] - want[m].mean()) <= (1e-12 if m == "AP" else 1e-10), m
        for b in g["bins"].tolist():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                levels, pm, mAP, aps = recall_precision_device(queries.copy(), labels, normalize=normalize, bins=b or None,
                                                               tile_rows=tile_rows, tile_cols=tile_cols, **kw)
            assert np.array_equal(levels, g["%s_levels_%d" % (name, b)]), (name, b)
            assert np.abs(pm - g["%s_means_%d" % (name, b)]).max() <= 1e-12, (name, b)
            assert abs(mAP - want["AP"].mean()) <= 1e-12
            assert np.abs(aps - want["AP"]).max() <= 1e-12


@pytest.mark.parametrize("normalize", [True, False])
def test_blocked_chain_positions_equal_the_ranking_path(normalize):
    """D = 555 with the K-block list [278, 277]: the positions the driver counts == those read off se_rank_rows on the whole
    [q, n] matrix of the same blocked distances."""
    import sehip
    from recall_precision import gallery_problem, recall_precision_device
    rng = np.random.default_rng(555)
    q, n, d, kb = 37, 301, 555, [278, 277]
    gallery = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((q, d)).astype(np.float32)
    g_ids, q_ids = list(range(n)), [1000 + i for i in range(q)]
    for i, j in ((0, 7), (5, 100), (36, 300)):                        # three queries are gallery items
        queries[i], q_ids[i] = gallery[j], j
    labels = {j: int(c) for j, c in zip(g_ids, rng.integers(0, 5, size=n))}
    labels.update({i: int(c) for i, c in zip(q_ids, rng.integers(0, 6, size=q)) if i >= 1000})
    seen = []

    def spy(cnt, hit_off, out=None):
        pos = sehip.count_to_positions(cnt, hit_off, out)
        seen.append((hit_off.cpu().numpy(), pos.cpu().numpy()))
        return pos

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        recall_precision_device(queries.copy(), labels, normalize=normalize, ids=q_ids, kblocks=kb, gallery=gallery.copy(), gallery_ids=g_ids,
                                tile_cols=128, kernels={"count_to_positions": spy})
    assert len(seen) == 1
    _, _, _, qcls, gcls, _, qidx = gallery_problem(queries, labels, q_ids, gallery, None, g_ids)
    fq, fg = torch.from_numpy(queries).cuda(), torch.from_numpy(gallery).cuda()
    if normalize:
        sehip.normalize_rows_(fq), sehip.normalize_rows_(fg)
    pd = sehip.pairwise_dist(fq, fg, metric=sehip.METRIC_COSINE if normalize else sehip.METRIC_EUCLID, kblocks=kb)
    want = qg.ranked_positions(pd.cpu().numpy(), qcls, gcls, qidx)
    present = (qidx >= 0) & (gcls[np.maximum(qidx, 0)] == qcls)
    order = np.argsort(2 * qcls.astype(np.int64) + present, kind="stable")     # the driver's query order: class, then "is a gallery item"
    off, pos = seen[0]
    for s, i in enumerate(order):
        assert np.array_equal(pos[off[s]:off[s + 1]], want[i]), i


def test_square_problem_equals_the_all_pairs_path():
    """gallery = queries with the same ids: per-query AP bit-equal to recall_precision_device(features, labels) -- both hand the
    same positions to the same reduce kernel."""
    from recall_precision import recall_precision_device
    g = np.load(os.path.join(qg.GOLDEN, "recprec_d24_cos.npz"))
    labels, ids = g["labels"].tolist(), list(range(len(g["labels"])))
    for bins in (None, 10):
        a = recall_precision_device(g["features"].copy(), labels, normalize=True, bins=bins)
        b = recall_precision_device(g["features"].copy(), labels, normalize=True, bins=bins, ids=ids, gallery=g["features"].copy(),
                                    gallery_ids=ids, tile_rows=100, tile_cols=128)
        assert np.array_equal(a[3], b[3]) and a[2] == b[2]
        assert np.array_equal(a[0], b[0]) and np.abs(a[1] - b[1]).max() <= 1e-12


def test_clis_with_a_gallery(tmp_path, capsys):
    """evaluate_retrieval.main and plot_recall_precision.main with --gallery_feat on a synthetic dataset: the metric names of a run
    without it, the values of direct calls of the two functions."""
    import evaluate_retrieval as er
    import plot_recall_precision as prp
    from class_hierarchy import ClassHierarchy
    from datasets import get_data_generator
    from recall_precision import recall_precision_device
    hpath = tmp_path / "cifar.parent-child.txt"
    with open(hpath, "w") as f:
        for p, c in np.load(os.path.join(qg.GOLDEN, "hierarchy_cifar.npz"))["edges"]:
            f.write("%d %d\n" % (p, c))
    ds = "synthetic:100x8x400x120"
    gen = get_data_generator(ds, None)
    rng = np.random.default_rng(8)
    centers = rng.standard_normal((100, 24)).astype(np.float32)
    dumps = {}
    for split, lab in (("test", list(gen.labels_test)), ("train", list(gen.labels_train))):
        feats = (centers[lab] + 0.8 * rng.standard_normal((len(lab), 24))).astype(np.float32)
        dumps[split] = (tmp_path / (split + ".pickle"), feats, lab)
        with open(dumps[split][0], "wb") as f:
            pickle.dump({"feat": {i: feats[i] for i in range(len(lab))}}, f)
    common = ["--dataset", ds, "--data_root", str(tmp_path), "--feat", str(dumps["test"][0]), "--label", "run", "--norm", "yes"]
    ev = common + ["--hierarchy", str(hpath), "--plot_max", "0", "--clip_ahp", "50"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain = er.main(ev)
        header_plain = [ln for ln in capsys.readouterr().out.splitlines() if "P@1 (WUP)" in ln]
        perf = er.main(ev + ["--gallery_feat", str(dumps["train"][0])])
        header = [ln for ln in capsys.readouterr().out.splitlines() if "P@1 (WUP)" in ln]
        assert header == header_plain and set(perf["run"]) == set(plain["run"])
        # direct calls: train items are other images whatever their number -- ids that cannot coincide with the queries'
        q_feats, q_lab = dumps["test"][1], dumps["test"][2]
        g_feats, g_lab = dumps["train"][1], dumps["train"][2]
        g_ids = [("train", j) for j in range(len(g_lab))]
        kw = dict(ids=list(range(len(q_lab))), gallery=g_feats.copy(), gallery_labels=dict(zip(g_ids, g_lab)), gallery_ids=g_ids)
        want, _ = ClassHierarchy.from_file(str(hpath), id_type=int).hierarchical_precision_device(
            q_feats.copy(), q_lab, [1, 10, 50, 100], compute_ahp=50, compute_ap=True, normalize=True, per_query=False, **kw)
        assert perf["run"] == want
        common += ["--csv", str(tmp_path / "c.csv")] + (["--save", str(tmp_path / "c.png")] if _has_matplotlib() else [])
        curve = prp.main(common + ["--gallery_feat", str(dumps["train"][0])])["run"]
        direct = recall_precision_device(q_feats.copy(), q_lab, normalize=True, **kw)
        assert np.array_equal(curve[0], direct[0]) and np.array_equal(curve[1], direct[1]) and curve[2] == direct[2]
        # --gallery_split test with the query file itself as gallery: every query is a gallery item -> the all-pairs values
        same = prp.main(common + ["--gallery_feat", str(dumps["test"][0]), "--gallery_split", "test"])["run"]
        square = prp.main(common)["run"]
        assert np.array_equal(same[0], square[0]) and np.abs(same[1] - square[1]).max() <= 1e-12 and same[2] == square[2]
    assert "mAP" in capsys.readouterr().out


def _has_matplotlib():
    try:
        import matplotlib  # noqa: F401
        return True
    except ImportError:
        return False


def test_refused_arguments():
    import sehip
    from sehip._lib import call
    pd = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    off = torch.tensor([0, 1, 2], dtype=torch.int64, device="cuda")
    f1, i1 = torch.zeros(2, dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    for bad in ((None, 8, 2, 8, 0, off, f1, i1, None, 0, i1), (pd, 8, 2, 8, 0, None, f1, i1, None, 0, i1), (pd, 8, 2, 8, 0, off, None, i1, None, 0, i1),
                (pd, 8, 2, 8, 0, off, f1, None, None, 0, i1), (pd, 8, 2, 8, 0, off, f1, i1, None, 0, None), (pd, 8, -1, 8, 0, off, f1, i1, None, 0, i1)):
        with pytest.raises(sehip.SehipError):
            call("se_count_preceding", *bad)
    for bad in ((None, off, 2, i1), (i1, None, 2, i1), (i1, off, 2, None), (i1, off, -1, i1)):
        with pytest.raises(sehip.SehipError):
            call("se_count_to_positions", *bad)
    assert call("se_count_preceding", None, 8, 0, 8, 0, None, None, None, None, 0, None) == 0       # q = 0: no launch, nothing read
    assert call("se_count_preceding", None, 8, 2, 0, 0, None, None, None, None, 0, None) == 0
    assert call("se_count_to_positions", None, None, 0, None) == 0
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    with pytest.raises(ValueError, match="--clip_ahp"):
        qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, [1, 10], compute_ahp=True, **kw)
