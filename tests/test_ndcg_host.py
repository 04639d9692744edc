"""NDCG without a GPU: the run-based ideal against brute force, the discounts bit for bit, the argument checks of se_ndcg through
raw ctypes, the two evaluation drivers on CPU stand-ins against the host ``ClassHierarchy.ndcg``, the command-line flags, and the
identity that ties NDCG with unit discounts to the hierarchical precision the reference defines."""
import ctypes

import numpy as np
import pytest
import torch

import _ndcg_canon as canon
import _qg_standins as qg


# ---------------------------------------------------------------------------------------------- canon, ideal, discounts

@pytest.mark.parametrize("case", range(len(canon.HAND)))
def test_canon_reproduces_the_hand_computed_cases(case):
    c = canon.HAND[case]
    a, b = canon.hand_values(c)
    assert abs(a - c["dcg_a"] / c["idcg_a"]) <= 1e-15 and abs(b - c["dcg_b"] / c["idcg_b"]) <= 1e-15


def test_discounts_are_numpys_bits():
    import sehip
    for n in (1, 7, 2049, 50000):
        d = sehip.ndcg_discounts(n, "cpu")
        assert d.dtype == torch.float64 and d.shape == (n,)
        assert np.array_equal(d.numpy().view(np.int64), (1 / np.log2(np.arange(2, n + 2))).view(np.int64))


def _ideal_cases():
    rng = np.random.RandomState(11)
    cases = []
    for C, hi in ((1, 5), (3, 4), (7, 9), (20, 30)):
        counts = rng.randint(0, hi, size=C)
        counts[rng.randint(C)] = 0                                   # a class without a gallery item
        if C > 2:
            counts[1] = 1                                            # a class whose only member is the query
        gain = rng.rand(C, C)                                        # not symmetric
        gain[rng.rand(C, C) < 0.3] = 0.5                             # ties between runs
        np.fill_diagonal(gain, 1.0)
        cases.append((gain, counts))
    cases.append((np.zeros((2, 2)), np.array([3, 2])))               # an ideal of 0
    cases.append((np.array(canon.HAND_GAIN_A), np.bincount(canon.HAND_CLS)))
    return cases


@pytest.mark.parametrize("full", [True, False])
def test_run_based_ideal_equals_brute_force(full):
    """Both sum the same non-negative products, the run form through differences of the prefix sums D of the discounts: each of the
    C runs carries an error of a few ulp of D[end] <= G (discounts are <= 1), so C * G * 2^-52 bounds the difference with room."""
    import sehip
    for gain, counts in _ideal_cases():
        G, C = int(counts.sum()), len(counts)
        ks = [1, 2, 3, max(G // 2, 1), max(G - 1, 1), max(G, 1), G + 5, 2]
        disc = sehip.ndcg_discounts(max(G, 1), "cpu")
        got = sehip.ndcg_ideal(torch.from_numpy(gain), counts, disc, ks, full=full)
        want = canon.ideal_brute(gain, counts, disc.numpy(), ks, full=full)
        assert got.dtype == torch.float64 and tuple(got.shape) == (C, 2, len(ks) + 1)
        assert np.abs(got.numpy() - want).max() <= max(C * G, 1) * 2.0 ** -52
        if not full:
            assert (got.numpy()[:, :, -1] == 0).all()
    with pytest.raises(sehip.SehipError):
        sehip.ndcg_ideal(np.eye(2), np.array([3, 3]), sehip.ndcg_discounts(5, "cpu"), [1], full=True)       # disc does not reach the gallery
    with pytest.raises(sehip.SehipError):
        sehip.ndcg_ideal(np.eye(2), np.array([3, 3]), sehip.ndcg_discounts(6, "cpu"), [0])


# ---------------------------------------------------------------------------------------------- the C entry point

def test_symbol_is_declared_from_the_header():
    import sehip
    from sehip import _lib
    assert "se_ndcg" in sehip.EXPORTS
    p = _lib.PROTOTYPES["se_ndcg"]
    assert p.stream and len(p.params) == 19 and [q.name for q in p.params][:4] == ["rank", "ldr", "q", "list_len"]
    assert sehip.NDCG_CHUNK == _lib.DEFINES["SE_NDCG_CHUNK"]


def test_raw_binding_refuses_invalid_arguments():
    """Every SE_ERR_INVALID case of the contract on dummy addresses: each returns before a launch, with its text."""
    import sehip
    from sehip import _lib
    L = sehip.lib()
    INVALID = _lib.DEFINES["SE_ERR_INVALID"]
    dummy = ctypes.create_string_buffer(4096)       # never touched
    a = ctypes.addressof(dummy)
    base = dict(rank=a, ldr=8, q=4, list_len=8, cls=a, gallery=16, qcls=a, qidx=None, gain_a=a, gain_b=a, num_classes=3, disc=a, disc_len=8,
                ideal=a, ks=a, nk=2, want_full=0, out=a, ldo=6)

    def call(**kw):
        v = dict(base, **kw)
        return L.se_ndcg(v["rank"], v["ldr"], v["q"], v["list_len"], v["cls"], v["gallery"], v["qcls"], v["qidx"], v["gain_a"], v["gain_b"],
                         v["num_classes"], v["disc"], v["disc_len"], v["ideal"], v["ks"], v["nk"], v["want_full"], v["out"], v["ldo"], None)

    def refused(text, **kw):
        assert call(**kw) == INVALID, kw
        msg = L.se_last_error().decode()
        assert msg.startswith("se_ndcg:") and text in msg, (kw, msg)

    for name in ("rank", "cls", "qcls", "gain_a", "gain_b", "disc", "ideal", "out", "ks"):
        refused("null pointer", **{name: None})
    refused("ldr", ldr=7)
    refused("disc covers", disc_len=7)
    refused("ldo", ldo=5)
    refused("nk=-1", nk=-1)
    refused("nk=513", nk=513, ldo=2000)
    for name in ("q", "list_len", "gallery", "disc_len", "ldr", "ldo"):
        refused("negative size", **{name: -1})
    refused("32-bit", list_len=2 ** 31 - 8192, ldr=2 ** 31, disc_len=2 ** 31)
    refused("num_classes=0", num_classes=0)
    refused("nothing to compute", nk=0, ks=None, want_full=0)
    # with every pointer NULL the shape checks still answer first
    nulls = {k: None for k in ("rank", "cls", "qcls", "gain_a", "gain_b", "disc", "ideal", "out", "ks")}
    refused("ldr", ldr=7, **nulls)
    refused("nk=513", nk=513, **nulls)
    # the empty problem: nothing is launched, nothing is looked at
    assert call(q=0, **nulls) == _lib.SE_OK
    assert call(list_len=0, **nulls) == _lib.SE_OK
    assert call(nk=0, ks=None, want_full=1, q=0) == _lib.SE_OK


# ---------------------------------------------------------------------------------------------- the drivers on CPU stand-ins

TOL = 1e-12      # stand-in and host reference sum the same products sequentially; the ideals differ as in the test above


def _per_query_equal(per_query, want_q, ids):
    for m, vals in want_q.items():
        got = np.array([per_query[m][i] for i in ids])
        assert np.abs(got - np.array([vals[i] for i in ids])).max() <= TOL, m


# names in the order of the result dictionaries (per cut-off WUP then LCS_HEIGHT, as the P@k names); the COLUMNS are grouped by table
NDCG_NAMES = ["NDCG@1 (WUP)", "NDCG@1 (LCS_HEIGHT)", "NDCG@5 (WUP)", "NDCG@5 (LCS_HEIGHT)", "NDCG (WUP)", "NDCG (LCS_HEIGHT)"]


def _host_rankings(g, normalize):
    """query id -> ranked gallery ids of the fixture, from the stable full ranking of the stand-ins."""
    from oracle import retrieval_oracle as ro
    q, ga = (ro.canon_normalize_rows(g["queries"]), ro.canon_normalize_rows(g["gallery"])) if normalize else (g["queries"], g["gallery"])
    rank = ro.canon_rank_rows(ro.canon_pdist(q, ga, ro.METRIC_COSINE if normalize else ro.METRIC_EUCLID))
    gids = g["gallery_ids"]
    return {int(i): gids[rank[r]].tolist() for r, i in enumerate(g["query_ids"])}


def test_device_driver_with_a_gallery_on_standins():
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    h, ks = qg.cifar_hierarchy(), [1, 10]
    ids = kw["ids"]
    kernels = dict(qg.cpu_kernels(True), ndcg=canon.standin)
    retrieved = _host_rankings(g, True)
    # ---- rank_gallery: whole rankings, every column
    base_m, base_q = h.hierarchical_precision_device(queries, labels, ks, compute_ahp=True, compute_ap=True, normalize=True, rank_gallery=True,
                                                     kernels=qg.cpu_kernels(True), tile_rows=16, **kw)
    means, per_query = h.hierarchical_precision_device(queries, labels, ks, compute_ahp=True, compute_ap=True, normalize=True, rank_gallery=True,
                                                       kernels=kernels, tile_rows=16, ndcg=[1, 5, 0], **kw)
    assert list(means) == list(base_m) + NDCG_NAMES and list(per_query) == list(means)
    assert all(means[m] == base_m[m] and per_query[m] == base_q[m] for m in base_m)          # the existing columns: unchanged, exactly
    want_m, want_q = h.ndcg(retrieved, labels, [1, 5, 0], gallery_ids=kw["gallery_ids"])
    assert list(want_q) == NDCG_NAMES
    _per_query_equal(per_query, want_q, ids)
    assert all(abs(means[m] - want_m[m]) <= TOL for m in NDCG_NAMES)
    # ---- top-L lists: K > 0 only; the MetricTable carries the new columns
    base_m, base_t = h.hierarchical_precision_device(queries, labels, ks, compute_ahp=10, normalize=True, kernels=qg.cpu_kernels(True),
                                                     per_query="table", **kw)
    means, table = h.hierarchical_precision_device(queries, labels, ks, compute_ahp=10, normalize=True, kernels=kernels, per_query="table",
                                                   ndcg=[1, 5, 20], **kw)
    names = list(base_t.columns)
    assert list(table.columns)[:len(names)] == names and [table.columns[m] for m in names] == [base_t.columns[m] for m in names]
    new = ["NDCG@1 (WUP)", "NDCG@5 (WUP)", "NDCG@20 (WUP)", "NDCG@1 (LCS_HEIGHT)", "NDCG@5 (LCS_HEIGHT)", "NDCG@20 (LCS_HEIGHT)"]
    assert sorted(list(table.columns)[len(names):]) == sorted(new)
    assert [table.columns[m] for m in new] == list(range(base_t.values.shape[1], base_t.values.shape[1] + 6))      # appended behind, grouped by table
    assert table.values.shape[1] == base_t.values.shape[1] + 8                                                 # (+ the two unused whole-list slots)
    assert all(torch.equal(table.values[:, table.columns[m]], base_t.values[:, base_t.columns[m]]) for m in names)
    want_m, want_q = h.ndcg(retrieved, labels, [1, 5, 20], gallery_ids=kw["gallery_ids"])
    for m in want_q:
        got = table.values[:, table.columns[m]].numpy()
        assert np.abs(got - np.array([want_q[m][i] for i in table.ids])).max() <= TOL and abs(means[m] - want_m[m]) <= TOL
    # ---- ndcg=None is today's call
    again_m, again_t = h.hierarchical_precision_device(queries, labels, ks, compute_ahp=10, normalize=True, kernels=qg.cpu_kernels(True),
                                                       per_query="table", ndcg=None, **kw)
    assert again_m == base_m and dict(again_t.columns) == dict(base_t.columns) and torch.equal(again_t.values, base_t.values)
    # ---- the whole list needs whole rankings
    with pytest.raises(ValueError, match="--rank_gallery"):
        h.hierarchical_precision_device(queries, labels, ks, compute_ahp=10, normalize=True, kernels=kernels, ndcg=[5, 0], **kw)
    with pytest.raises(ValueError, match="integers >= 0"):
        h.hierarchical_precision_device(queries, labels, ks, compute_ahp=10, normalize=True, kernels=kernels, ndcg=[-1], **kw)


def test_device_driver_all_pairs_on_standins():
    """Every image is query and gallery item: whole-list NDCG forces the full-ranking path, cut-offs alone stay on the top-L lists."""
    from evaluate_retrieval import pairwise_retrieval  # noqa: F401  (the host path of the reference, named in the docs)
    from oracle import retrieval_oracle as ro
    from test_dp_gloo import _cpu_kernels
    g = np.load(qg.GOLDEN + "/retrieval_cluster_cos.npz")
    feats = np.ascontiguousarray(g["features"][:90], dtype=np.float32)
    leaves = sorted(set(qg.load_fixture()["gallery_labels"].tolist()))
    labels = [leaves[(7 * i) % len(leaves)] for i in range(len(feats))]
    h = qg.cifar_hierarchy()

    class Counting(object):
        def __init__(self, fn):
            self.fn, self.calls = fn, 0

        def __call__(self, *a, **kw):
            self.calls += 1
            return self.fn(*a, **kw)

    rank = ro.canon_rank_rows(ro.canon_pdist(ro.canon_normalize_rows(feats), ro.canon_normalize_rows(feats), ro.METRIC_COSINE))
    retrieved = {i: rank[i].tolist() for i in range(len(feats))}
    for nd, full_path in (([1, 5, 0], True), ([1, 5], False)):
        kernels = dict(_cpu_kernels(), ndcg=canon.standin)
        kernels["ranking_tiles"], kernels["local_topk"] = Counting(kernels["ranking_tiles"]), Counting(kernels["local_topk"])
        means, per_query = h.hierarchical_precision_device(feats.copy(), labels, [1, 10], compute_ahp=10, normalize=True, kernels=kernels, ndcg=nd)
        assert (kernels["ranking_tiles"].calls > 0) == full_path and (kernels["local_topk"].calls > 0) == (not full_path)
        want_m, want_q = h.ndcg(retrieved, labels, nd)
        assert list(per_query)[-len(want_q):] == list(want_q)
        _per_query_equal(per_query, want_q, range(len(feats)))


def test_ranked_driver_on_standins():
    import test_ranked_host as R
    g, labels, as_dict, as_arrays, all_ids = R.partial_fixture()
    h, ks = R.hierarchy(), [1, 5]
    kw = dict(compute_ahp=True, compute_ap=True, all_ids=all_ids)
    base_m, base_q = h.hierarchical_precision_ranked(as_dict, labels, ks, kernels=R.cpu_kernels(), **kw)
    for ignore in (True, False):
        kernels = dict(R.cpu_kernels(), ndcg=canon.standin)
        means, per_query = h.hierarchical_precision_ranked(as_arrays, labels, ks, kernels=kernels, tile_rows=5, ndcg=[1, 5, 0], ignore_qids=ignore, **kw)
        assert list(means)[-6:] == NDCG_NAMES
        if ignore:
            assert all(means[m] == base_m[m] and per_query[m] == base_q[m] for m in base_m)
        want_m, want_q = h.ndcg(as_dict, labels, [1, 5, 0], ignore_qids=ignore, all_ids=all_ids)
        _per_query_equal(per_query, want_q, list(as_dict))
    # heads stay heads for K > 0; the whole list completes them
    shortest = int(g["lengths"].min())
    k = min(shortest - 1, 5)
    for nd, completes in (([k], False), ([k, 0], True)):
        kernels = dict(R.cpu_kernels(), ndcg=canon.standin)
        means, per_query = h.hierarchical_precision_ranked(as_dict, labels, [1], compute_ahp=k, kernels=kernels, all_ids=all_ids, ndcg=nd)
        assert (kernels["complete_rankings"].calls > 0) == completes
        _per_query_equal(per_query, h.ndcg(as_dict, labels, nd, all_ids=all_ids)[1], list(as_dict))
    with pytest.raises(ValueError, match="cut-offs"):
        h.hierarchical_precision_ranked(as_dict, labels, [1], kernels=R.cpu_kernels(), all_ids=all_ids, ndcg=[len(all_ids) + 1])


# ---------------------------------------------------------------------------------------------- command lines

def test_command_lines_take_the_flag():
    import evaluate_rankings
    import evaluate_retrieval
    common = ["--dataset", "d", "--data_root", "r", "--hierarchy", "h"]
    ret = common + ["--feat", "f.pickle"]
    assert evaluate_retrieval.parse_args(ret + ["--ndcg", "10", "0", "1"]).ndcg == [10, 0, 1]
    assert not hasattr(evaluate_retrieval.parse_args(ret), "ndcg")           # absent unless given
    assert evaluate_retrieval.parse_args(ret + ["--gallery_feat", "g.pickle", "--clip_ahp", "5", "--ndcg", "10"]).ndcg == [10]
    assert evaluate_retrieval.parse_args(ret + ["--gallery_feat", "g.pickle", "--rank_gallery", "--ndcg", "0"]).ndcg == [0]
    rk = common + ["--ranking", "r.npz"]
    assert evaluate_rankings.parse_args(rk + ["--ndcg", "0", "5"]).ndcg == [0, 5]
    assert not hasattr(evaluate_rankings.parse_args(rk), "ndcg")
    assert evaluate_retrieval.ndcg_metric_names([10, 0, 1]) == ["NDCG@10 (WUP)", "NDCG@10 (LCS_HEIGHT)", "NDCG@1 (WUP)", "NDCG@1 (LCS_HEIGHT)",
                                                                "NDCG (WUP)", "NDCG (LCS_HEIGHT)"]
    assert evaluate_retrieval.ndcg_metric_names(None) == []


def test_command_lines_refuse_bad_values(capsys):
    import evaluate_rankings
    import evaluate_retrieval
    common = ["--dataset", "d", "--data_root", "r", "--hierarchy", "h"]
    for parse, argv in ((evaluate_retrieval.parse_args, common + ["--feat", "f.pickle", "--ndcg", "-1"]),
                        (evaluate_rankings.parse_args, common + ["--ranking", "r.npz", "--ndcg", "5", "-2"])):
        with pytest.raises(SystemExit):
            parse(argv)
        assert "--ndcg" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        evaluate_retrieval.parse_args(common + ["--feat", "f.pickle", "--gallery_feat", "g.pickle", "--clip_ahp", "5", "--ndcg", "5", "0"])
    assert "--rank_gallery" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------- the tie to hierarchical precision

def test_unit_discounts_reproduce_hierarchical_precision():
    """With disc = 1 the DCG is the cumulative similarity and the ideal the best cumulative similarity: NDCG@k is the reference's
    P@k -- for queries that are first in their own ranking (the reference shifts the best curve and subtracts the self-similarity 1,
    which is the ideal without the own item because the diagonal of both tables is 1 and the row maximum) and for non-members."""
    g = qg.load_fixture()
    _, labels, kw = qg.fixture_arguments(g)
    h, ks = qg.cifar_hierarchy(), [1, 3, 10, 50]
    classes = sorted(set(labels.values()))
    for t in h.similarity_tables(classes):
        assert (np.diag(t) == 1).all() and (t.max(axis=1) == 1).all()
    gids = kw["gallery_ids"]
    rng = np.random.RandomState(5)
    retrieved = {}
    for q in kw["ids"][:12]:                 # non-members keep a permutation; members stand first in their own ranking
        perm = rng.permutation(len(gids)).tolist()
        ret = [gids[j] for j in perm]
        if q in gids:
            ret.remove(q)
            ret.insert(0, q)
        retrieved[q] = ret
    for q in gids[:6]:
        ret = [gids[j] for j in rng.permutation(len(gids)).tolist()]
        ret.remove(q)
        retrieved[q] = [q] + ret
    ones = np.ones(len(gids))
    _, want = h.hierarchical_precision(retrieved, labels, ks)
    _, got = h.ndcg(retrieved, labels, ks, disc=ones, gallery_ids=gids)
    for k in ks:
        for t in ("WUP", "LCS_HEIGHT"):
            a, b = got["NDCG@%d (%s)" % (k, t)], want["P@%d (%s)" % (k, t)]
            assert max(abs(a[q] - b[q]) for q in retrieved) <= 1e-12, (k, t)
