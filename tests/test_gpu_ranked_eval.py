"""GPU: evaluation of GIVEN rankings -- ClassHierarchy.hierarchical_precision_ranked and recall_precision.recall_precision_ranked on
se_complete_rankings + the metric kernels -- against the stored values of the reference (hierarchy_cifar.npz, qg_retrieval.npz /
qg_full_ahp.npz, ranked_partial.npz), and against the host functions on truncated lists with a shuffled all_ids.  Rankings come
from the CPU oracle, computed once per configuration.

Bounds: 1e-10 absolute on every float64 hierarchical metric (the bound of the project's hierarchy and query-gallery fixtures);
recall-precision levels equal as float64, means, mAP and per-query AP to 1e-12 (the bounds of tests/test_gpu_recprec.py)."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import _complete_canon as cc
import _qg_standins as qg

pytestmark = pytest.mark.gpu

TOL = 1e-10
GOLDEN = qg.GOLDEN


@functools.lru_cache(maxsize=None)
def cifar(normalize):
    """(fixture, labels, oracle rankings [200, 200]) of hierarchy_cifar.npz."""
    from oracle import retrieval_oracle as ro
    g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
    return g, g["labels"].tolist(), ro.canon_retrieval(g["features"], normalize)[1]


class Counting(object):
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def worst(per_query, want, ids):
    assert set(per_query) == set(want)
    return {m: max(abs(per_query[m][i] - want[m][i]) for i in ids) for m in want}


@pytest.mark.parametrize("normalize", [True, False])
def test_cifar_reference_values(normalize):
    """200 x 200 oracle rankings as a dict, as host arrays and as a device tensor, in one tile and in three: the reference's means."""
    g, labels, rk = cifar(normalize)
    n, ks, h = len(labels), g["ks"].tolist(), qg.cifar_hierarchy()
    want = dict(zip(g["metric_names"].tolist(), g["metric_values"].tolist()))
    forms = [({i: rk[i].tolist() for i in range(n)}, None), ((np.arange(n), rk), 80), ((list(range(n)), torch.from_numpy(rk).cuda()), None)]
    for ahp in (True, 50):
        results = []
        for retrieved, tile_rows in forms:
            for all_ids in (None, list(range(n))):
                avg, per_q = h.hierarchical_precision_ranked(retrieved, labels, ks, compute_ahp=ahp, compute_ap=True, all_ids=all_ids, tile_rows=tile_rows)
                for m, v in avg.items():
                    err = abs(v - want["%s|norm=%d|ahp=%s" % (m, normalize, ahp)])
                    assert err <= TOL, (m, normalize, ahp, err)
                results.append(per_q)
        for r in results[1:]:       # every input form and tiling scores the same class sequences: sums of at most 200 terms in [0, 1]
            assert max(worst(r, results[0], range(n)).values()) <= 1e-13


@pytest.mark.parametrize("ignore", [True, False])
def test_truncated_lists_with_a_shuffled_all_ids(ignore):
    """The rankings cut to 60 entries, the rest appended in a shuffled all_ids order: the host function on the same input -- whole
    AHP, AHP@50 and AP, per query and as means."""
    g, labels, rk = cifar(True)
    n, ks, h = len(labels), [1, 10, 50, 100], qg.cifar_hierarchy()
    all_ids = np.random.default_rng(60).permutation(n).tolist()
    cut = {i: rk[i, :60].tolist() for i in range(n)}
    for ahp in (True, 50):
        want_means, want = h.hierarchical_precision(cut, labels, ks, compute_ahp=ahp, compute_ap=True, ignore_qids=ignore, all_ids=all_ids)
        for retrieved, tile_rows in ((cut, None), ((np.arange(n), rk[:, :60].copy()), 64)):
            means, per_q = h.hierarchical_precision_ranked(retrieved, labels, ks, compute_ahp=ahp, compute_ap=True, ignore_qids=ignore,
                                                           all_ids=all_ids, tile_rows=tile_rows)
            err = worst(per_q, want, range(n))
            print(ignore, ahp, tile_rows, err)
            assert max(err.values()) <= TOL, err
            assert max(abs(means[m] - want_means[m]) for m in want_means) <= TOL


def test_head_only_path_completes_nothing():
    """Lists of 120 entries, ks <= 100, AHP@100, no AP: scored as they are -- complete_rankings is not called."""
    import sehip
    g, labels, rk = cifar(False)
    n, ks, h = len(labels), [1, 10, 50, 100], qg.cifar_hierarchy()
    heads = {i: rk[i, :120].tolist() for i in range(n)}
    counting = Counting(sehip.complete_rankings)
    kw = dict(compute_ahp=100, compute_ap=False, all_ids=list(range(n)))
    means, per_q = h.hierarchical_precision_ranked(heads, labels, ks, kernels={"complete_rankings": counting}, **kw)
    assert counting.calls == 0
    want_means, want = h.hierarchical_precision(heads, labels, ks, **kw)
    err = worst(per_q, want, range(n))
    assert max(err.values()) <= TOL, err
    assert max(abs(means[m] - want_means[m]) for m in want_means) <= TOL
    h.hierarchical_precision_ranked(heads, labels, ks, kernels={"complete_rankings": counting}, **dict(kw, compute_ap=True))
    assert counting.calls == 1


@pytest.mark.parametrize("name,normalize", [("cosine", True), ("euclid", False)])
def test_held_out_queries(name, normalize):
    """37 queries over 301 gallery items (qg_retrieval.npz / qg_full_ahp.npz): oracle rankings as gallery ids, the stored per-query
    values of the reference, whole-list AHP and AHP@clip."""
    from oracle import retrieval_oracle as ro
    g = qg.load_fixture()
    full = np.load(os.path.join(GOLDEN, "qg_full_ahp.npz"))
    queries, labels, kw = qg.fixture_arguments(g)
    qn, gn = (ro.canon_normalize_rows(queries), ro.canon_normalize_rows(kw["gallery"])) if normalize else (queries, kw["gallery"])
    rank = ro.canon_rank_rows(ro.canon_pdist(qn, gn, ro.METRIC_COSINE if normalize else ro.METRIC_EUCLID))
    ids, g_ids = g["query_ids"].tolist(), np.asarray(kw["gallery_ids"])
    retrieved = {q: g_ids[rank[i]].tolist() for i, q in enumerate(ids)}
    for want, ahp in ((full, True), (g, int(g["ahp_clip"]))):
        names = want[name + "_metric_names"].tolist()
        for form, tile_rows in ((retrieved, None), ((np.array(ids), g_ids[rank]), 16)):
            means, per_query = qg.cifar_hierarchy().hierarchical_precision_ranked(form, labels, [1, 10, 50, 100], compute_ahp=ahp, compute_ap=True,
                                                                                  all_ids=kw["gallery_ids"], tile_rows=tile_rows)
            assert set(means) == set(names)
            err = np.abs(np.array([[per_query[m][i] for i in ids] for m in names]) - want[name + "_per_query"]).max(axis=1)
            print(name, ahp, tile_rows, dict(zip(names, err.tolist())))
            assert err.max() <= TOL, dict(zip(names, err.tolist()))
            assert np.abs(np.array([means[m] for m in names]) - want[name + "_means"]).max() <= TOL


@pytest.mark.parametrize("ahp", [True, 20])
@pytest.mark.parametrize("ignore", [True, False])
def test_partial_lists_reference_values(ahp, ignore):
    """tests/golden/ranked_partial.npz: partial lists, a shuffled all_ids, queries inside and outside the gallery -- the per-query
    values of the reference's own hierarchical_precision."""
    from test_ranked_host import check_against_fixture, partial_fixture
    g, labels, as_dict, as_arrays, all_ids = partial_fixture()
    for retrieved, tile_rows in ((as_dict, None), (as_arrays, 5), ((as_arrays[0], torch.from_numpy(as_arrays[1]).cuda(), as_arrays[2]), 11)):
        means, per_query = qg.cifar_hierarchy().hierarchical_precision_ranked(retrieved, labels, g["ks"].tolist(), compute_ahp=ahp, compute_ap=True,
                                                                              ignore_qids=ignore, all_ids=all_ids, tile_rows=tile_rows)
        check_against_fixture(g, "ahp%s_ignore%d" % (ahp, int(ignore)), means, per_query)


def test_bad_rankings_raise():
    from test_ranked_host import partial_fixture
    g, labels, as_dict, as_arrays, all_ids = partial_fixture()
    q0 = int(g["query_ids"][3])
    dup = dict(as_dict)
    dup[q0] = dup[q0] + dup[q0][:1]
    with pytest.raises(ValueError, match=r"query %d\b.*more than once" % q0):
        qg.cifar_hierarchy().hierarchical_precision_ranked(dup, labels, [1, 5], compute_ap=True, all_ids=all_ids)
    arr = torch.from_numpy(as_arrays[1]).cuda()
    arr[3, 1] = 4711
    with pytest.raises(ValueError, match=r"4711.*query %d\b" % q0):
        qg.cifar_hierarchy().hierarchical_precision_ranked((as_arrays[0], arr, as_arrays[2]), labels, [1, 5], compute_ap=True, all_ids=all_ids)


@pytest.mark.parametrize("bins", [None, 10])
def test_recall_precision_ranked(bins):
    """recprec_d24_cos.npz: complete oracle rankings, and rankings cut to 50 entries with a shuffled all_ids, against
    recall_precision_host on the NumPy-completed rankings."""
    from oracle import retrieval_oracle as ro
    from recall_precision import recall_precision_host, recall_precision_host_gallery, recall_precision_ranked
    g = np.load(os.path.join(GOLDEN, "recprec_d24_cos.npz"))
    labels = g["labels"].tolist()
    n = len(labels)
    rk = ro.canon_retrieval(g["features"], bool(g["normalize"]))[1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = recall_precision_host(rk, labels, bins)
        for retrieved, all_ids, tile_rows in (({i: rk[i].tolist() for i in range(n)}, None, None), ((np.arange(n), rk), list(range(n)), 70)):
            got = recall_precision_ranked(retrieved, labels, bins=bins, all_ids=all_ids, tile_rows=tile_rows)
            assert np.array_equal(got[0], want[0])
            assert np.abs(got[1] - want[1]).max() <= 1e-12 and abs(got[2] - want[2]) <= 1e-12 and np.abs(got[3] - want[3]).max() <= 1e-12
        # cut to 50 entries; gallery index = position in the shuffled all_ids
        all_ids = np.random.default_rng(50).permutation(n)
        pos = np.empty(n, dtype=np.int64)
        pos[all_ids] = np.arange(n)
        completed, status = cc.complete_rankings(pos[rk[:, :50]], n)
        assert not status.any()
        for ignore in (True, False):
            want = recall_precision_host_gallery(completed, labels, [labels[i] for i in all_ids], pos if ignore else None, bins)
            for retrieved, tile_rows in (({i: rk[i, :50].tolist() for i in range(n)}, None), ((np.arange(n), torch.from_numpy(rk[:, :50].copy()).cuda()), 70)):
                got = recall_precision_ranked(retrieved, labels, bins=bins, ignore_qids=ignore, all_ids=all_ids.tolist(), tile_rows=tile_rows)
                assert np.array_equal(got[0], want[0])
                assert np.abs(got[1] - want[1]).max() <= 1e-12 and abs(got[2] - want[2]) <= 1e-12 and np.abs(got[3] - want[3]).max() <= 1e-12


def test_cli_prints_the_table_of_evaluate_retrieval(tmp_path, capsys):
    """evaluate_rankings.main on the pickle that pairwise_retrieval(..., return_generator=False) wrote for a 200-image feature file:
    the table evaluate_retrieval.main prints for the features themselves, and its values."""
    import pickle
    import evaluate_rankings as evr
    import evaluate_retrieval as er
    from datasets import get_data_generator
    hpath = tmp_path / "cifar.parent-child.txt"
    with open(hpath, "w") as f:
        for p, c in np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))["edges"]:
            f.write("%d %d\n" % (p, c))
    ds = "synthetic:100x8x300x200"
    lab = list(get_data_generator(ds, None).labels_test)
    rng = np.random.default_rng(200)
    feats = (rng.standard_normal((100, 24))[lab] + 0.8 * rng.standard_normal((len(lab), 24))).astype(np.float32)
    with open(tmp_path / "feat.pickle", "wb") as f:
        pickle.dump({"feat": {i: feats[i] for i in range(len(lab))}}, f)
    with open(tmp_path / "rankings.pickle", "wb") as f:
        pickle.dump(er.pairwise_retrieval(str(tmp_path / "feat.pickle"), True, return_generator=False), f)
    common = ["--dataset", ds, "--data_root", str(tmp_path), "--hierarchy", str(hpath), "--plot_max", "0", "--label", "run"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for extra in ([], ["--clip_ahp", "50", "--skip_ap"]):
            want = er.main(common + ["--feat", str(tmp_path / "feat.pickle"), "--norm", "yes"] + extra)
            table = capsys.readouterr().out
            got = evr.main(common + ["--ranking", str(tmp_path / "rankings.pickle")] + extra)
            assert capsys.readouterr().out == table and "P@1 (WUP)" in table
            assert set(got["run"]) == set(want["run"])
            assert max(abs(got["run"][m] - want["run"][m]) for m in want["run"]) <= TOL
