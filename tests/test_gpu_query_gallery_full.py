"""Whole-list metrics of a query-vs-gallery evaluation on the MI355X: hierarchical_precision_device(..., gallery=...,
rank_gallery=True) -- se_pairwise_dist + se_rank_rows on rectangular tiles, se_hierarchical_precision with the gallery's classes --
against the values of the imported reference (tests/golden/qg_full_ahp.npz, tests/golden/qg_retrieval.npz), against the host
ClassHierarchy.hierarchical_precision on oracle rankings for rows just past the 53,248-column limit of the register-resident ranking
kernel, the degenerate sizes, the rectangular ranking_tiles and the CLI.

Bound: 1e-10 absolute on every float64 metric, the bound of the project's hierarchy fixtures."""
import functools
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import _qg_standins as qg

pytestmark = pytest.mark.gpu

TOL = 1e-10
CLASSES = (3, 17, 42, 58, 43, 90)
KS = [1, 10, 50, 100]


def _rows(per_query, names, ids):
    return np.array([[per_query[m][i] for i in ids] for m in names])


@pytest.mark.parametrize("name,normalize", [("cosine", True), ("euclid", False)])
def test_fixture_parity(name, normalize):
    """P@k, whole-list AHP (WUP and LCS_HEIGHT) and AP of the reference, per query and as means, from one tile and from three; with
    compute_ahp=250 the values of the clipped fixture from the same ranking."""
    g = qg.load_fixture()
    full = np.load(os.path.join(qg.GOLDEN, "qg_full_ahp.npz"))
    queries, labels, kw = qg.fixture_arguments(g)
    ids = g["query_ids"].tolist()
    for want, ahp in ((full, True), (g, int(g["ahp_clip"]))):
        names = want[name + "_metric_names"].tolist()
        for tile_rows in (None, 16):
            means, per_query = qg.cifar_hierarchy().hierarchical_precision_device(
                queries.copy(), labels, KS, compute_ahp=ahp, compute_ap=True, normalize=normalize, tile_rows=tile_rows, rank_gallery=True, **kw)
            assert set(means) == set(names)
            err = np.abs(_rows(per_query, names, ids) - want[name + "_per_query"]).max(axis=1)
            print(name, ahp, tile_rows, dict(zip(names, err.tolist())))
            assert err.max() <= TOL, dict(zip(names, err.tolist()))
            assert np.abs(np.array([means[m] for m in names]) - want[name + "_means"]).max() <= TOL
        means_only, none = qg.cifar_hierarchy().hierarchical_precision_device(
            queries.copy(), labels, KS, compute_ahp=ahp, compute_ap=True, normalize=normalize, per_query=False, rank_gallery=True, **kw)
        assert none is None and all(abs(means_only[m] - means[m]) <= 1e-13 for m in names)


@functools.lru_cache(maxsize=None)
def _long_row_problem():
    """6 queries x 53,300 gallery items, D = 8, six CIFAR-100 classes.  Query 1 is gallery item 40,000; query 4 is gallery item 53,299,
    whose feature row gallery item 7 repeats: in its own ranking it comes second (the tie goes to the lower index), so its position
    has to be looked for.  Query 5's class is not in the gallery."""
    rng = np.random.default_rng(53300)
    n, q, d = 53300, 6, 8
    g_lab = rng.choice(CLASSES[:5], size=n, p=[0.4, 0.3, 0.2, 0.0999, 0.0001]).astype(np.int64)
    q_lab = np.array([3, 17, 42, 58, 3, 90])
    centers = {c: rng.standard_normal(d) for c in CLASSES}
    gallery = (np.stack([centers[c] for c in g_lab]) + rng.standard_normal((n, d))).astype(np.float32)
    queries = (np.stack([centers[c] for c in q_lab]) + rng.standard_normal((q, d))).astype(np.float32)
    g_ids, q_ids = list(range(n)), [100000 + i for i in range(q)]
    g_lab[40000], g_lab[53299], g_lab[7] = 17, 3, 3
    gallery[7] = gallery[53299]
    queries[1], q_ids[1] = gallery[40000], 40000
    queries[4], q_ids[4] = gallery[53299], 53299
    labels = {j: int(c) for j, c in zip(g_ids, g_lab)}
    labels.update({i: int(c) for i, c in zip(q_ids, q_lab)})
    return queries, gallery, q_ids, g_ids, labels


@functools.lru_cache(maxsize=None)
def _long_row_reference(normalize):
    """The repository's host ClassHierarchy.hierarchical_precision on the oracle's canonical rankings of the oracle's distances."""
    from oracle import retrieval_oracle as ro
    queries, gallery, q_ids, g_ids, labels = _long_row_problem()
    qn, gn = (ro.canon_normalize_rows(queries), ro.canon_normalize_rows(gallery)) if normalize else (queries, gallery)
    rank = ro.canon_rank_rows(ro.canon_pdist(qn, gn, ro.METRIC_COSINE if normalize else ro.METRIC_EUCLID))
    assert rank[4, 0] == 7 and rank[4, 1] == 53299 and rank[1, 0] == 40000
    retrieved = {q_ids[i]: rank[i].tolist() for i in range(len(q_ids))}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return qg.cifar_hierarchy().hierarchical_precision(retrieved, labels, KS, compute_ahp=True, compute_ap=True, ignore_qids=True)


@pytest.mark.parametrize("normalize", [True, False])
def test_rows_past_the_register_resident_ranking(normalize):
    """53,300 columns: the segment + merge ranking under a rectangular q, in two tiles of query rows (4 + 2)."""
    queries, gallery, q_ids, g_ids, labels = _long_row_problem()
    want_means, want = _long_row_reference(normalize)
    means, per_query = qg.cifar_hierarchy().hierarchical_precision_device(
        queries.copy(), labels, KS, compute_ahp=True, compute_ap=True, normalize=normalize, ids=q_ids, gallery=gallery.copy(),
        gallery_ids=g_ids, tile_rows=4, rank_gallery=True)
    assert set(per_query) == set(want)
    for m in want:
        err = max(abs(per_query[m][i] - want[m][i]) for i in q_ids)
        print(normalize, m, err)
        assert err <= TOL, (m, err)
        assert abs(means[m] - want_means[m]) <= TOL, m
    assert per_query["AP"][q_ids[5]] == 0.0


def test_a_gallery_of_one_item_and_no_queries():
    hier = qg.cifar_hierarchy()
    gallery = np.ones((1, 8), dtype=np.float32)
    labels = {0: 3, 1000: 3, 1001: 43, 1002: 42}     # taxonomy siblings of 3: no similarity is 0, no metric 0 / 0
    rng = np.random.default_rng(1)
    queries = rng.standard_normal((3, 8)).astype(np.float32)
    ids = [1000, 1001, 1002]
    for normalize in (True, False):
        means, per_query = hier.hierarchical_precision_device(queries.copy(), labels, [1], compute_ahp=True, compute_ap=True, normalize=normalize,
                                                              ids=ids, gallery=gallery.copy(), gallery_ids=[0], rank_gallery=True)
        want_means, want = hier.hierarchical_precision({i: [0] for i in ids}, labels, [1], compute_ahp=True, compute_ap=True)
        for m in want:
            assert max(abs(per_query[m][i] - want[m][i]) for i in ids) <= TOL, m
            assert abs(means[m] - want_means[m]) <= TOL, m
        assert per_query["AP"] == {1000: 1.0, 1001: 0.0, 1002: 0.0} and per_query["AHP (WUP)"][1000] == 0.0
        means, per_query = hier.hierarchical_precision_device(np.zeros((0, 8), dtype=np.float32), labels, [1], compute_ahp=True, compute_ap=True,
                                                              normalize=normalize, ids=[], gallery=gallery.copy(), gallery_ids=[0],
                                                              rank_gallery=True)
        assert set(means) == set(want) and all(np.isnan(v) for v in means.values()) and all(v == {} for v in per_query.values())


def test_rectangular_ranking_tiles():
    """ranking_tiles(..., gallery=...) against the oracle, K-block list included; a tile kept after its iteration has ended is not
    written again by the next one, and the process-wide tile cache is neither used nor grown."""
    import evaluate_retrieval as er
    from oracle import retrieval_oracle as ro
    rng = np.random.default_rng(4)
    q, g = rng.standard_normal((37, 555)).astype(np.float32), rng.standard_normal((301, 555)).astype(np.float32)
    g[100] = g[200]
    held = {k: {kk: int(b.numel()) for kk, b in v.items()} for k, v in er._tile_cache.items()}
    kept = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)             # D > 448 without a K-block list
        for normalize in (True, False):
            for kb in (None, [278, 277]):
                qn, gn = (ro.canon_normalize_rows(q), ro.canon_normalize_rows(g)) if normalize else (q, g)
                want = ro.canon_rank_rows(ro.canon_pdist(qn, gn, ro.METRIC_COSINE if normalize else ro.METRIC_EUCLID, kblocks=kb))
                got = []
                for r0, tile in er.ranking_tiles(torch.from_numpy(q).cuda(), normalize, tile_rows=16, queries=(3, 37), kblocks=kb,
                                                 gallery=torch.from_numpy(g).cuda()):
                    assert tile.dtype == torch.int32 and tuple(tile.shape) == (min(16, 37 - r0), 301)
                    got.append(tile.cpu().numpy())
                if kept is not None:
                    assert np.array_equal(kept[0].cpu().numpy(), kept[1])
                kept = (tile, got[-1].copy())
                assert np.array_equal(np.concatenate(got), want[3:]), (normalize, kb)
    assert {k: {kk: int(b.numel()) for kk, b in v.items()} for k, v in er._tile_cache.items()} == held


def test_cli_with_a_ranked_gallery(tmp_path, capsys):
    """evaluate_retrieval.main with --gallery_feat --rank_gallery: the reference's default columns, the values of a direct call; with
    --clip_ahp as well, the values of the run without --rank_gallery."""
    import evaluate_retrieval as er
    from class_hierarchy import ClassHierarchy
    from datasets import get_data_generator
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
    ev = ["--dataset", ds, "--data_root", str(tmp_path), "--feat", str(dumps["test"][0]), "--label", "run", "--norm", "yes",
          "--hierarchy", str(hpath), "--plot_max", "0", "--gallery_feat", str(dumps["train"][0])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        perf = er.main(ev + ["--rank_gallery"])
        header = [ln for ln in capsys.readouterr().out.splitlines() if "P@1 (WUP)" in ln]
        assert len(header) == 1 and all(m in header[0] for m in er.METRICS)
        q_feats, q_lab = dumps["test"][1], dumps["test"][2]
        g_feats, g_lab = dumps["train"][1], dumps["train"][2]
        g_ids = [("train", j) for j in range(len(g_lab))]
        kw = dict(ids=list(range(len(q_lab))), gallery=g_feats.copy(), gallery_labels=dict(zip(g_ids, g_lab)), gallery_ids=g_ids)
        want, _ = ClassHierarchy.from_file(str(hpath), id_type=int).hierarchical_precision_device(
            q_feats.copy(), q_lab, KS, compute_ahp=True, compute_ap=True, normalize=True, per_query=False, rank_gallery=True, **kw)
        assert perf["run"] == want and set(want) == set(er.METRICS)
        ranked = er.main(ev + ["--rank_gallery", "--clip_ahp", "50"])["run"]
        counted = er.main(ev + ["--clip_ahp", "50"])["run"]
        assert set(ranked) == set(counted)
        for m in counted:
            assert abs(ranked[m] - counted[m]) <= TOL, m
        with pytest.raises(ValueError, match="--clip_ahp"):
            er.main(ev)
