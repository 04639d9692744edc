"""Whole-list metrics of a query-vs-gallery evaluation without a GPU: the host logic of hierarchical_precision_device(...,
gallery=..., rank_gallery=True) and of ranking_tiles(..., gallery=...) through the NumPy stand-ins of tests/_qg_standins.py, against
the values the imported reference produced on whole rankings (tests/golden/qg_full_ahp.npz, tools/make_qg_full_golden.py) and
against the top-k + counting path (tests/golden/qg_retrieval.npz); tiling, the memory refusal, the CLI flag.

Bound: 1e-10 absolute on every float64 metric, the bound of the project's hierarchy fixtures."""
import os

import numpy as np
import pytest
import torch

import _qg_standins as qg

CONFIGS = [("cosine", True), ("euclid", False)]
TOL = 1e-10


def load_full_fixture():
    return np.load(os.path.join(qg.GOLDEN, "qg_full_ahp.npz"))


def _ranked(normalize, compute_ahp=True, **more):
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    kw.update(more)
    return qg.cifar_hierarchy().hierarchical_precision_device(
        queries, labels, g["ks"].tolist(), compute_ahp=compute_ahp, compute_ap=True, normalize=normalize,
        kernels=qg.cpu_kernels(normalize), rank_gallery=True, **kw)


def _rows(per_query, names, ids):
    return np.array([[per_query[m][i] for i in ids] for m in names])


@pytest.mark.parametrize("name,normalize", CONFIGS)
def test_whole_list_metrics_reproduce_the_fixture(name, normalize):
    """AHP (WUP) / AHP (LCS_HEIGHT) over the whole list, P@k and AP: per query and as means."""
    full = load_full_fixture()
    names = full[name + "_metric_names"].tolist()
    assert {"AHP (WUP)", "AHP (LCS_HEIGHT)", "AP", "P@1 (WUP)", "P@100 (LCS_HEIGHT)"} <= set(names)
    means, per_query = _ranked(normalize, tile_rows=16)
    assert set(means) == set(names) == set(per_query)
    got = _rows(per_query, names, full["query_ids"].tolist())
    err = np.abs(got - full[name + "_per_query"]).max(axis=1)
    print(dict(zip(names, err.tolist())))
    assert err.max() <= TOL, dict(zip(names, err.tolist()))
    for m, want in zip(names, full[name + "_means"].tolist()):
        assert abs(means[m] - want) <= TOL, m


@pytest.mark.parametrize("name,normalize", CONFIGS)
def test_clipped_ahp_from_the_ranking_equals_the_topk_and_counting_results(name, normalize):
    """compute_ahp=250 with rank_gallery=True: P@k, AHP@250 and AP of tests/golden/qg_retrieval.npz from one ranking."""
    g = qg.load_fixture()
    names = g[name + "_metric_names"].tolist()
    means, per_query = _ranked(normalize, compute_ahp=int(g["ahp_clip"]), tile_rows=16)
    assert set(means) == set(names)
    got = _rows(per_query, names, g["query_ids"].tolist())
    assert np.abs(got - g[name + "_per_query"]).max() <= TOL
    assert np.abs(np.array([means[m] for m in names]) - g[name + "_means"]).max() <= TOL
    # and the path without the option, on the same stand-ins
    queries, labels, kw = qg.fixture_arguments(g)
    _, other = qg.cifar_hierarchy().hierarchical_precision_device(
        queries, labels, g["ks"].tolist(), compute_ahp=int(g["ahp_clip"]), compute_ap=True, normalize=normalize,
        kernels=qg.cpu_kernels(normalize), tile_rows=16, tile_cols=100, **kw)
    assert np.abs(got - _rows(other, names, g["query_ids"].tolist())).max() <= TOL


def test_rows_do_not_depend_on_the_tiling():
    full = load_full_fixture()
    names, ids = full["cosine_metric_names"].tolist(), full["query_ids"].tolist()
    rows = [_rows(_ranked(True, tile_rows=t)[1], names, ids) for t in (1, 5, 64)]
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[0], rows[2])


def test_means_only():
    full = load_full_fixture()
    means, per_query = _ranked(False, per_query=False)
    assert per_query is None
    for m, want in zip(full["euclid_metric_names"].tolist(), full["euclid_means"].tolist()):
        assert abs(means[m] - want) <= TOL, m


def test_own_item_is_dropped_and_the_others_keep_every_item():
    """What the metric kernel is handed: rows of all 301 gallery items, the gallery classes, per query its own gallery row or -1."""
    g = qg.load_fixture()
    seen = []
    kernels = qg.cpu_kernels(True)
    inner = kernels["hierarchical_precision"]

    def spy(tile, cls, qcls, qidx, *a, **k):
        seen.append((tuple(tile.shape), len(cls), qidx.numpy().copy(), k["ahp_len"], k["want_ap"]))
        return inner(tile, cls, qcls, qidx, *a, **k)

    kernels["hierarchical_precision"] = spy
    queries, labels, kw = qg.fixture_arguments(g)
    qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, [1, 10], compute_ahp=True, compute_ap=True, normalize=True,
                                                      kernels=kernels, rank_gallery=True, tile_rows=20, **kw)
    assert [s[0] for s in seen] == [(20, 301), (17, 301)] and all(s[1] == 301 and s[3] == 0 and s[4] is True for s in seen)
    qidx = np.concatenate([s[2] for s in seen])
    ids = g["query_ids"]
    assert np.array_equal(qidx, np.where(ids < 1000, ids, -1)) and int((qidx >= 0).sum()) == 5


def test_rectangular_ranking_tiles():
    """ranking_tiles(..., gallery=...): the canonical ranking of the canonical distances, for a sub-range of the queries, with a K-block
    list, and tiles a caller kept after the iteration are not views of the process-wide tile cache."""
    import evaluate_retrieval as er
    from oracle import retrieval_oracle as ro
    rng = np.random.default_rng(3)
    q, g = rng.standard_normal((11, 9)).astype(np.float32), rng.standard_normal((23, 9)).astype(np.float32)
    g[5] = g[17]                                                     # identical gallery rows: the tie goes to the lower index
    # (empty unless GPU tests ran earlier in this process: their all-pairs evaluations keep their buffers)
    held = {k: {kk: int(b.numel()) for kk, b in v.items()} for k, v in er._tile_cache.items()}
    for normalize in (True, False):
        for kb in (None, [5, 4]):
            qn, gn = (ro.canon_normalize_rows(q), ro.canon_normalize_rows(g)) if normalize else (q, g)
            want = ro.canon_rank_rows(ro.canon_pdist(qn, gn, ro.METRIC_COSINE if normalize else ro.METRIC_EUCLID, kblocks=kb))
            kernels = {k: v for k, v in qg.cpu_kernels(normalize).items() if k in ("normalize_rows_", "row_sqnorm", "pairwise_dist", "rank_rows")}
            tiles = list(er.ranking_tiles(torch.from_numpy(q.copy()), normalize, tile_rows=4, queries=(2, 11), kblocks=kb,
                                          gallery=torch.from_numpy(g.copy()), kernels=kernels))
            assert [r0 for r0, _ in tiles] == [2, 6, 10] and [t.shape[0] for _, t in tiles] == [4, 4, 1]
            assert np.array_equal(np.concatenate([t.numpy() for _, t in tiles]), want[2:])
    assert {k: {kk: int(b.numel()) for kk, b in v.items()} for k, v in er._tile_cache.items()} == held
    with pytest.raises(ValueError, match="feature dimensions"):
        list(er.ranking_tiles(torch.zeros((2, 3)), gallery=torch.zeros((2, 4)), kernels=kernels))
    with pytest.raises(ValueError, match="int32"):
        list(er.ranking_tiles(torch.zeros((2, 3)), gallery=torch.zeros((2, 3)), idx16=True, kernels=kernels))


def test_unclipped_ahp_without_the_option_is_still_refused():
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    for more in ({}, {"rank_gallery": False}):
        with pytest.raises(ValueError, match="--clip_ahp"):
            qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, [1], compute_ahp=True, kernels=qg.cpu_kernels(True), **kw, **more)
    with pytest.raises(ValueError, match="needs a gallery"):
        qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, [1], compute_ahp=True, kernels=qg.cpu_kernels(True),
                                                          rank_gallery=True)


def test_memory_refusal_names_its_estimate(monkeypatch):
    """Free memory patched to 64 KiB: the fixture's curves alone are 2 x 6 x 301 x 8 = 28,896 bytes, its features 9,464, and one
    tile row 8 x 304 + 8 x 11 -- with 16 rows the estimate is 78,680 bytes and is refused before anything runs; with the default
    sizing the tile shrinks until it fits."""
    import class_hierarchy
    monkeypatch.setattr(class_hierarchy, "_free_device_bytes", lambda dev: 64 << 10)
    kernels = qg.cpu_kernels(True)

    def boom(*a, **k):
        raise AssertionError("a kernel ran although the estimate does not fit")

    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    refused = dict(kernels, pairwise_dist=boom, rank_rows=boom, hierarchical_precision=boom, normalize_rows_=boom)
    with pytest.raises(ValueError, match=r"78,680 bytes") as e:
        qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, g["ks"].tolist(), compute_ahp=True, compute_ap=True, normalize=True,
                                                          kernels=refused, rank_gallery=True, tile_rows=16, **kw)
    assert "65,536 are free" in str(e.value)
    seen = []
    inner = kernels["rank_rows"]
    kernels["rank_rows"] = lambda pd: seen.append(pd.shape[0]) or inner(pd)
    _, per_query = qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, g["ks"].tolist(), compute_ahp=True, compute_ap=True,
                                                                     normalize=True, kernels=kernels, rank_gallery=True, **kw)
    # 9/10 of 65,536 less the fixed 38,360 bytes leave room for 8 rows of 2,520 bytes
    assert seen == [8, 8, 8, 8, 5]
    full = load_full_fixture()
    names = full["cosine_metric_names"].tolist()
    assert np.abs(_rows(per_query, names, full["query_ids"].tolist()) - full["cosine_per_query"]).max() <= TOL
    monkeypatch.setattr(class_hierarchy, "_free_device_bytes", lambda dev: 30000)
    with pytest.raises(ValueError, match=r"estimated [0-9,]+ bytes"):
        qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, g["ks"].tolist(), compute_ahp=True, normalize=True,
                                                          kernels=refused, rank_gallery=True, **kw)


def test_no_queries_and_a_gallery_of_one():
    hier = qg.cifar_hierarchy()
    kernels = qg.cpu_kernels(False)
    gallery = np.ones((1, 4), dtype=np.float32)
    labels = {0: 3, 1000: 3, 1001: 43}                 # 43 is a taxonomy sibling of 3: no similarity of the test is 0, no metric 0 / 0
    means, per_query = hier.hierarchical_precision_device(np.zeros((0, 4), dtype=np.float32), labels, [1], compute_ahp=True, compute_ap=True,
                                                          ids=[], gallery=gallery, gallery_ids=[0], kernels=kernels, rank_gallery=True)
    assert set(means) == {"P@1 (WUP)", "P@1 (LCS_HEIGHT)", "AHP (WUP)", "AHP (LCS_HEIGHT)", "AP"}
    assert all(np.isnan(v) for v in means.values()) and all(v == {} for v in per_query.values())
    queries = np.array([[1, 1, 1, 2], [0, 1, 0, 1]], dtype=np.float32)
    means, per_query = hier.hierarchical_precision_device(queries, labels, [1], compute_ahp=True, compute_ap=True, ids=[1000, 1001],
                                                          gallery=gallery, gallery_ids=[0], kernels=kernels, rank_gallery=True)
    want, _ = hier.hierarchical_precision({1000: [0], 1001: [0]}, labels, [1], compute_ahp=True, compute_ap=True)
    assert per_query["P@1 (WUP)"][1000] == 1.0 and per_query["AP"] == {1000: 1.0, 1001: 0.0}
    assert per_query["AHP (WUP)"] == {1000: 0.0, 1001: 0.0}                 # np.trapz of a single point
    for m in want:
        assert abs(means[m] - want[m]) <= TOL, m
    with pytest.raises(ValueError, match="gallery is empty"):
        hier.hierarchical_precision_device(queries, labels, [1], ids=[1000, 1001], gallery=np.zeros((0, 4), dtype=np.float32), gallery_ids=[],
                                           kernels=kernels, rank_gallery=True)


def test_cli_flag():
    """--rank_gallery parses next to --gallery_feat (in its group) and is a parser error without it; a command line without it parses
    to the namespace it always did."""
    import evaluate_retrieval as er
    base = "--dataset x --data_root y --hierarchy h --feat a.pkl"
    plain = er.parse_args(base.split())
    assert "rank_gallery" not in vars(plain)
    args = er.parse_args((base + " --gallery_feat g.pkl --rank_gallery").split())
    assert args.rank_gallery is True and args.clip_ahp is None and args.gallery_feat == ["g.pkl"]
    both = er.parse_args((base + " --gallery_feat g.pkl --rank_gallery --clip_ahp 250").split())
    assert both.rank_gallery is True and both.clip_ahp == 250
    with pytest.raises(SystemExit) as e:
        er.parse_args((base + " --rank_gallery").split())
    assert e.value.code == 2
    titles = [grp.title for grp in er.build_parser()._action_groups if any(a.dest == "rank_gallery" for a in grp._group_actions)]
    same = [grp.title for grp in er.build_parser()._action_groups if any(a.dest == "gallery_feat" for a in grp._group_actions)]
    assert len(titles) == 1 and titles == same


def test_cli_passes_the_option_on(monkeypatch, tmp_path):
    """main(): rank_gallery=True reaches hierarchical_precision_device with the gallery, compute_ahp stays True without --clip_ahp."""
    import pickle
    import evaluate_retrieval as er
    from class_hierarchy import ClassHierarchy
    calls = []

    def fake(self, features, labels, ks, **kw):
        calls.append(kw)
        return {m: 0.5 for m in er.METRICS + ["AHP@7 (WUP)", "AHP@7 (LCS_HEIGHT)"]}, None

    monkeypatch.setattr(ClassHierarchy, "hierarchical_precision_device", fake)
    hpath = tmp_path / "h.txt"
    hpath.write_text("0 1\n0 2\n")
    feats = {}
    for name, n in (("q", 4), ("g", 6)):
        feats[name] = str(tmp_path / (name + ".pickle"))
        with open(feats[name], "wb") as f:
            pickle.dump({"feat": {i: np.full(3, i, dtype=np.float32) for i in range(n)}}, f)
    argv = ["--dataset", "synthetic:2x3x6x4", "--data_root", str(tmp_path), "--hierarchy", str(hpath), "--plot_max", "0", "--feat", feats["q"],
            "--gallery_feat", feats["g"]]
    er.main(argv + ["--rank_gallery"])
    er.main(argv + ["--rank_gallery", "--clip_ahp", "7"])
    er.main(argv + ["--clip_ahp", "7"])
    assert calls[0]["rank_gallery"] is True and calls[0]["compute_ahp"] is True and calls[0]["gallery"].shape == (6, 3)
    assert calls[1]["rank_gallery"] is True and calls[1]["compute_ahp"] == 7
    assert "rank_gallery" not in calls[2] and calls[2]["compute_ahp"] == 7
