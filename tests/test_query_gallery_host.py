"""Query-vs-gallery retrieval evaluation without a GPU: the host logic of recall_precision_device(..., gallery=...) and
hierarchical_precision_device(..., gallery=...) through NumPy stand-ins of the kernels against the values the imported reference
produced (tests/golden/qg_retrieval.npz, tools/make_qg_golden.py); counted positions against a stable full ranking; the CLI flags;
the argument checks of the two C entry points."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import _qg_standins as qg

CONFIGS = [("cosine", True), ("euclid", False)]
TILES = [1, 7, 64, None]


@pytest.mark.parametrize("name,normalize", CONFIGS)
def test_recall_precision_reproduces_the_fixture(name, normalize):
    """Levels equal as float64; means, mAP and every per-query AP to 1e-12 (the bounds of tests/test_recprec_host.py)."""
    from recall_precision import recall_precision_device
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    names = g[name + "_metric_names"].tolist()
    want_ap = g[name + "_per_query"][names.index("AP")]
    for b in g["bins"].tolist():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # the queries without a relevant gallery item
            levels, means, mAP, aps = recall_precision_device(queries.copy(), labels, normalize=normalize, bins=b or None,
                                                              kernels=qg.cpu_kernels(normalize), tile_rows=16, tile_cols=100, **kw)
        assert np.array_equal(levels, g["%s_levels_%d" % (name, b)]), (name, b)
        assert np.abs(means - g["%s_means_%d" % (name, b)]).max() <= 1e-12, (name, b)
        assert abs(mAP - want_ap.mean()) <= 1e-12
        assert np.abs(aps - want_ap).max() <= 1e-12


@pytest.mark.parametrize("name,normalize", CONFIGS)
def test_hierarchical_precision_reproduces_the_fixture(name, normalize):
    """P@k, AHP@250 (WUP and LCS_HEIGHT) and AP, per query and as means, to rel / abs 1e-12 (the bound of tests/test_host.py)."""
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    means, per_query = qg.cifar_hierarchy().hierarchical_precision_device(
        queries, labels, g["ks"].tolist(), compute_ahp=int(g["ahp_clip"]), compute_ap=True, normalize=normalize,
        kernels=qg.cpu_kernels(normalize), tile_rows=16, tile_cols=100, **kw)
    names = g[name + "_metric_names"].tolist()
    assert set(means) == set(names)
    for m in names:
        want = g[name + "_per_query"][names.index(m)]
        got = np.array([per_query[m][i] for i in g["query_ids"].tolist()])
        assert got == pytest.approx(want, rel=1e-12, abs=1e-12), m
        assert means[m] == pytest.approx(float(g[name + "_means"][names.index(m)]), rel=1e-12, abs=1e-12), m


def test_recall_precision_does_not_depend_on_the_tiling():
    from recall_precision import recall_precision_device
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    res = []
    for tr in TILES:
        for tc in TILES:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                res.append(recall_precision_device(queries.copy(), labels, normalize=True, kernels=qg.cpu_kernels(True), tile_rows=tr,
                                                   tile_cols=tc, **kw))
    for other in res[1:]:
        assert np.array_equal(other[0], res[0][0]) and np.array_equal(other[1], res[0][1]) and np.array_equal(other[3], res[0][3])


def _random_problem(seed, q, n, classes):
    """Distances with every hard case of the canonical order: duplicated gallery columns (ties broken by the global index), NaN of
    both signs, +0 / -0, +inf; some queries are gallery items."""
    rng = np.random.default_rng(seed)
    pd = rng.standard_normal((q, n)).astype(np.float32)
    if n >= 8:
        dup = rng.choice(n, size=n // 2, replace=False)
        pd[:, dup[: len(dup) // 2]] = pd[:, dup[len(dup) // 2: 2 * (len(dup) // 2)]]      # identical gallery rows: identical columns
        special = np.array([0.0, -0.0, np.nan, -np.nan, np.inf], dtype=np.float32)
        at = rng.random((q, n)) < 0.15
        pd[at] = rng.choice(special, size=int(at.sum()))
    gcls = rng.integers(0, classes, size=n).astype(np.int32)
    qcls = rng.integers(0, classes + 1, size=q).astype(np.int32)                            # class `classes`: not in the gallery
    qidx = np.where(rng.random(q) < 0.4, rng.integers(0, n, size=q), -1).astype(np.int32)
    return pd, qcls, gcls, qidx


def _keys_and_offsets(pd, qcls, gcls, qidx):
    """What the driver hands to se_count_preceding: per query its relevant items' (distance, global index), canonically sorted."""
    from oracle import retrieval_oracle as ro
    rel_d, rel_i, off = [], [], [0]
    for i in range(len(pd)):
        mem = np.flatnonzero((gcls == qcls[i]) & (np.arange(len(gcls)) != qidx[i]))
        order = ro.canon_rank_rows(pd[i:i + 1, mem])[0] if len(mem) else np.zeros(0, dtype=np.int64)
        rel_d.append(pd[i, mem][order])
        rel_i.append(mem[order].astype(np.int32))
        off.append(off[-1] + len(mem))
    return (torch.from_numpy(np.concatenate(rel_d).astype(np.float32)), torch.from_numpy(np.concatenate(rel_i).astype(np.int32)),
            torch.from_numpy(np.array(off, dtype=np.int64)))


@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("tile_cols", TILES)
@pytest.mark.parametrize("tile_rows", TILES)
def test_counted_positions_equal_ranked_positions(tile_rows, tile_cols, shards):
    """Integer equality with the positions read off a stable full ranking, for every tiling and with the gallery split into shards
    whose counts are summed."""
    from sharded_retrieval import shard_bounds
    for seed, (q, n, classes) in enumerate([(9, 70, 3), (5, 131, 2), (3, 1, 1)]):
        pd, qcls, gcls, qidx = _random_problem(seed, q, n, classes)
        rel_d, rel_i, hit_off = _keys_and_offsets(pd, qcls, gcls, qidx)
        total = int(hit_off[-1])
        tr, tc = tile_rows or q, tile_cols or n
        parts = []
        for s0, s1 in shard_bounds(n, shards):
            cnt = torch.zeros(max(total, 1), dtype=torch.int32)
            for r0 in range(0, q, tr):
                r1 = min(q, r0 + tr)
                sub_off = hit_off[r0:r1 + 1] - hit_off[r0]
                a, b = int(hit_off[r0]), int(hit_off[r1])
                for c0 in range(s0, s1, tc):
                    c1 = min(s1, c0 + tc)
                    qg.count_preceding(torch.from_numpy(pd[r0:r1, c0:c1].copy()), c0, sub_off, rel_d[a:b], rel_i[a:b],
                                       torch.from_numpy(qidx[r0:r1]), cnt[a:max(b, a + 1)])
            parts.append(cnt)
        pos = qg.count_to_positions(torch.stack(parts).sum(dim=0).to(torch.int32), hit_off).numpy()
        want = qg.ranked_positions(pd, qcls, gcls, qidx)
        for i in range(q):
            assert np.array_equal(pos[hit_off[i]:hit_off[i + 1]], want[i]), (seed, i)


def test_cli_parsers_accept_the_gallery_flags():
    """--gallery_feat (repeatable) and --gallery_split {train, test}; without them nothing else of the namespace changes."""
    import evaluate_retrieval as er
    import plot_recall_precision as prp
    base = {er: "--dataset x --data_root y --hierarchy h --feat a.pkl --feat b.pkl", prp: "--dataset x --data_root y --feat a.pkl --feat b.pkl"}
    old = {er: {"dataset", "data_root", "hierarchy", "is_a", "str_ids", "classes_from", "feat", "label", "norm", "plot_max", "prec_type",
                "clip_ahp", "csv", "skip_ap", "kblocks"},
           prp: {"dataset", "data_root", "classes_from", "feat", "label", "norm", "bins", "save", "csv", "kblocks"}}
    for mod, argv in base.items():
        plain = vars(mod.build_parser().parse_args(argv.split()))
        assert set(plain) == old[mod] | {"gallery_feat", "gallery_split"}
        assert plain["gallery_feat"] is None and plain["gallery_split"] == "train"
        with_g = vars(mod.build_parser().parse_args((argv + " --gallery_feat g1.pkl --gallery_feat g2.pkl --gallery_split test").split()))
        assert with_g["gallery_feat"] == ["g1.pkl", "g2.pkl"] and with_g["gallery_split"] == "test"
        assert {k: v for k, v in with_g.items() if k in old[mod]} == {k: v for k, v in plain.items() if k in old[mod]}
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args((argv + " --gallery_split validation").split())
        titles = [grp.title for grp in mod.build_parser()._action_groups
                  if any(a.dest == "gallery_feat" for a in grp._group_actions)]
        assert len(titles) == 1 and titles[0].startswith("Extensions of this build")


def test_gallery_arguments_of_the_clis():
    """No --gallery_feat: no keyword reaches the metric functions.  'train' gallery ids never coincide with query ids."""
    import argparse
    import pickle
    import tempfile
    import evaluate_retrieval as er
    gen = argparse.Namespace(labels_train=[5, 6, 7], labels_test=[1, 2])
    assert er.gallery_arguments(argparse.Namespace(gallery_feat=None, gallery_split="train"), 0, gen, None) == {}
    with tempfile.NamedTemporaryFile(suffix=".pickle") as f:
        pickle.dump({"feat": {2: np.zeros(3, np.float32), 0: np.ones(3, np.float32)}}, f)
        f.flush()
        args = argparse.Namespace(gallery_feat=[f.name], gallery_split="train")
        assert er.gallery_arguments(args, 1, gen, None) == {}
        kw = er.gallery_arguments(args, 0, gen, None)
        assert kw["gallery_ids"] == [("train", 2), ("train", 0)] and [kw["gallery_labels"][i] for i in kw["gallery_ids"]] == [7, 5]
        args.gallery_split = "test"
        gen.labels_test = [1, 2, 3]
        kw = er.gallery_arguments(args, 0, gen, None)
        assert kw["gallery_ids"] == [2, 0] and kw["gallery_labels"] == [1, 2, 3] and kw["gallery"].shape == (2, 3)


def test_without_a_gallery_nothing_new_is_reached(monkeypatch):
    """gallery=None: the three stand-ins of the all-pairs path are all that is looked up -- the counting entry points and the
    gallery driver raise if touched -- and the result is the host mirror's."""
    import recall_precision as rp
    import sehip
    from test_recprec_host import _canon_rank, _cpu_kernels

    def boom(*a, **k):
        raise AssertionError("the query-vs-gallery path was reached without a gallery")

    for mod, name in ((rp, "_recall_precision_gallery"), (sehip, "count_preceding"), (sehip, "count_to_positions"),
                      (sehip.ops, "count_preceding"), (sehip.ops, "count_to_positions")):
        monkeypatch.setattr(mod, name, boom)
    resolve = rp.resolve_kernels

    def resolve_no_counting(kernels, names):
        if {"count_preceding", "count_to_positions"} & set(names):
            boom()
        return resolve(kernels, names)

    monkeypatch.setattr(rp, "resolve_kernels", resolve_no_counting)
    g = np.load(qg.GOLDEN + "/recprec_d24_euc.npz")
    kernels = _cpu_kernels()
    assert set(kernels) == {"ranking_tiles", "relevant_positions", "recall_precision_reduce", "device"}
    got = rp.recall_precision_device(g["features"].copy(), g["labels"].tolist(), kernels=kernels, tile_rows=64)
    want = rp.recall_precision_host(_canon_rank(g["features"], False), g["labels"])
    assert np.array_equal(got[0], want[0]) and np.abs(got[1] - want[1]).max() <= 1e-12 and np.abs(got[3] - want[3]).max() <= 1e-12


def test_unclipped_ahp_with_a_gallery_is_refused():
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    with pytest.raises(ValueError, match="--clip_ahp"):
        qg.cifar_hierarchy().hierarchical_precision_device(queries, labels, [1], compute_ahp=True, kernels=qg.cpu_kernels(True), **kw)


def test_host_variant_equals_the_square_statement():
    """recall_precision_host_gallery with gallery == queries and qidx = own index is recall_precision_host."""
    from recall_precision import recall_precision_host, recall_precision_host_gallery
    from test_recprec_host import _canon_rank
    g = np.load(qg.GOLDEN + "/recprec_d24_cos.npz")
    rank = _canon_rank(g["features"], True)
    for bins in (None, 10):
        a = recall_precision_host(rank, g["labels"], bins=bins)
        b = recall_precision_host_gallery(rank, g["labels"], g["labels"], np.arange(len(rank)), bins=bins)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_argument_validation_without_gpu():
    """The checks of se_count_preceding / se_count_to_positions run before any launch."""
    import sehip
    lib = sehip.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert lib.se_count_preceding(z, 8, 2, 8, 0, z, z, z, z, 0, z, z) == -1
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_count_preceding(one, 8, 2, 8, 0, one, one, one, z, 0, z, z) == -1                   # no histogram
    assert lib.se_count_preceding(one, 8, -1, 8, 0, one, one, one, z, 0, one, z) == -1
    assert b"bad shape" in lib.se_last_error()
    assert lib.se_count_preceding(one, 4, 2, 8, 0, one, one, one, z, 0, one, z) == -1                  # ldp < n_cols
    assert b"leading dimension" in lib.se_last_error()
    assert lib.se_count_preceding(one, 8, 2, 8, 2 ** 31 - 4, one, one, one, z, 0, one, z) == -1        # global indices are int32
    assert lib.se_count_preceding(z, 8, 0, 8, 0, z, z, z, z, 0, z, z) == 0                             # no query: nothing to do
    assert lib.se_count_preceding(z, 8, 2, 0, 0, z, z, z, z, 0, z, z) == 0                             # no column
    assert lib.se_count_to_positions(z, z, 3, z, z) == -1
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_count_to_positions(one, one, -1, one, z) == -1
    assert lib.se_count_to_positions(z, z, 0, z, z) == 0


def test_ops_refuse_without_gpu():
    import sehip
    i32, i64 = torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(sehip.SehipError):
        sehip.count_preceding(torch.zeros((2, 4)), 0, i64, torch.zeros(4), i32, None, i32)
    with pytest.raises(sehip.SehipError):
        sehip.count_to_positions(i32, i64)
