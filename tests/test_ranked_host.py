"""Host side of the evaluation of given rankings: the NumPy restatement of se_complete_rankings against the reference's own line,
the raw entry point's argument checks (no GPU needed: they return before any launch), the two drivers on CPU stand-ins against the
host functions, every ValueError they raise, the empty-query result, and the evaluate_rankings.py command line."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import _complete_canon as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------- the restatement and the raw binding

def test_restatement_equals_the_reference_line():
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 64, 65, 300):
        all_ids = rng.permutation(n).tolist()
        for L in sorted({0, 1, n // 2, n - 1, n}):
            ret = rng.permutation(n)[:L].tolist()
            want = cc.complete_list_reference(ret, all_ids)
            rank, status = cc.complete_rankings(np.array([ret], dtype=np.int32).reshape(1, L), n, None, np.array(all_ids, dtype=np.int32))
            assert status[0] == 0 and rank[0].tolist() == want
            # identity order == all_ids = range(n); a padded row with a length
            padded = np.array([ret + [-5] * 3], dtype=np.int32)
            rank, status = cc.complete_rankings(padded, n, [L], None)
            assert status[0] == 0 and rank[0].tolist() == cc.complete_list_reference(ret, list(range(n)))


def test_restatement_flags_bad_rows():
    order = np.array([3, 1, 0, 2], dtype=np.int32)
    lists = np.array([[0, 1, 2], [1, 1, 2], [0, 4, 2], [-1, 2, 2], [2, 3, 9]], dtype=np.int32)
    rank, status = cc.complete_rankings(lists, 4, [3, 3, 3, 3, 2], order)
    assert status.tolist() == [0, cc.BAD_DUP, cc.BAD_RANGE, cc.BAD_RANGE | cc.BAD_DUP, 0]
    assert rank.tolist() == [[0, 1, 2, 3], [3, 1, 0, 2], [3, 1, 0, 2], [3, 1, 0, 2], [2, 3, 1, 0]]


def invalid_calls(lists, rank, status):
    """Every SE_ERR_INVALID case of se_complete_rankings on the given (device or dummy) addresses: each returns before a launch."""
    import sehip
    from sehip import _lib
    L = sehip.lib()
    INVALID = _lib.DEFINES["SE_ERR_INVALID"]

    def call(lists_=lists, ldl=8, q=4, list_len=8, gallery=16, rank_=rank, ldr=16, status_=status, ws_bytes=0):
        return L.se_complete_rankings(lists_, ldl, None, q, list_len, None, gallery, rank_, ldr, status_, None, ws_bytes, None)

    assert call(lists_=None) == INVALID
    assert call(rank_=None) == INVALID
    assert call(status_=None) == INVALID
    assert call(ldl=7) == INVALID
    assert call(ldr=15) == INVALID
    assert call(q=-1) == INVALID
    assert call(list_len=-1) == INVALID
    assert call(gallery=-1) == INVALID
    assert call(ws_bytes=-1) == INVALID
    big = _lib.DEFINES["SE_COMPLETE_LDS_ITEMS"] + 1
    assert L.se_complete_rankings_workspace_bytes(4, big) > 0 and L.se_complete_rankings_workspace_bytes(4, big - 1) == 0
    assert call(gallery=big, ldr=big) == INVALID                     # a gallery above the LDS bound without its workspace
    assert b"se_complete_rankings" in L.se_last_error()
    assert call(q=0, lists_=None, rank_=None, status_=None) == _lib.SE_OK          # nothing to do: no launch, nothing looked at
    assert call(gallery=0, ldr=0, rank_=None) == _lib.SE_OK


def test_raw_binding_refuses_invalid_arguments():
    dummy = ctypes.create_string_buffer(4 * 16 * 4)       # never touched: every call returns before a launch
    addr = ctypes.addressof(dummy)
    invalid_calls(addr, addr, addr)


# ---------------------------------------------------------------------------------------------- the drivers on CPU stand-ins

TOL = 1e-10


class Counting(object):
    """A stand-in that counts its calls."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


def cpu_kernels():
    """CPU stand-ins of every kernel the two drivers look up: the restatement of se_complete_rankings and the NumPy stand-ins the
    existing host tests use for the metric kernels (a NULL qidx -- ignore_qids=False -- becomes -1 everywhere for them)."""
    from test_dp_gloo import _hprec_standin
    from test_recprec_host import _cpu_kernels as recprec_kernels

    def complete_rankings(lists, gallery, lengths=None, order=None, out=None):
        rank, status = cc.complete_rankings(lists.numpy(), gallery, None if lengths is None else lengths.numpy(),
                                            None if order is None else order.numpy())
        return torch.from_numpy(rank), torch.from_numpy(status)

    def hierarchical_precision(rank, cls, qcls, qidx, *a, **kw):
        qidx = torch.full((rank.shape[0],), -1, dtype=torch.int32) if qidx is None else qidx
        return _hprec_standin(rank, cls, qcls, qidx, *a, **kw)

    rp = recprec_kernels()
    return {"complete_rankings": Counting(complete_rankings), "hierarchical_precision": hierarchical_precision,
            "relevant_positions": rp["relevant_positions"], "recall_precision_reduce": rp["recall_precision_reduce"],
            "device": torch.device("cpu")}


def hierarchy():
    import _qg_standins as qg
    return qg.cifar_hierarchy()


def partial_fixture():
    """tests/golden/ranked_partial.npz (tools/make_ranked_golden.py): (fixture, labels, dict form, array form, all_ids)."""
    g = np.load(os.path.join(GOLDEN, "ranked_partial.npz"))
    labels = {int(i): int(c) for i, c in zip(g["gallery_ids"], g["gallery_labels"])}
    labels.update({int(i): int(c) for i, c in zip(g["query_ids"], g["query_labels"])})
    as_dict = {int(q): g["lists"][i, :g["lengths"][i]].tolist() for i, q in enumerate(g["query_ids"])}
    return g, labels, as_dict, (g["query_ids"], g["lists"], g["lengths"]), g["all_ids"].tolist()


def check_against_fixture(g, key, means, per_query):
    names, ids = g[key + "_metric_names"].tolist(), g["query_ids"].tolist()
    assert set(per_query) == set(names)
    got = np.array([[per_query[m][i] for i in ids] for m in names])
    err = np.abs(got - g[key + "_per_query"]).max(axis=1)
    print(key, dict(zip(names, err.tolist())))
    assert err.max() <= TOL, dict(zip(names, err.tolist()))
    assert np.abs(np.array([means[m] for m in names]) - g[key + "_per_query"].mean(axis=1)).max() <= TOL


@pytest.mark.parametrize("ahp", [True, 20])
@pytest.mark.parametrize("ignore", [True, False])
def test_ranked_driver_equals_the_reference_on_partial_lists(ahp, ignore):
    """Partial lists, a shuffled all_ids, queries inside and outside the gallery: the reference's own per-query values, from the
    dict form, a generator, the array form (host array and tensor) and several tiles; the host mirror agrees too."""
    g, labels, as_dict, as_arrays, all_ids = partial_fixture()
    h, ks, key = hierarchy(), g["ks"].tolist(), "ahp%s_ignore%d" % (ahp, int(ignore))
    kw = dict(compute_ahp=ahp, compute_ap=True, ignore_qids=ignore, all_ids=all_ids)
    forms = [(as_dict, None), ((pair for pair in as_dict.items()), 7), (as_arrays, 5),
             ((as_arrays[0].tolist(), torch.from_numpy(as_arrays[1]).to(torch.int32), torch.from_numpy(as_arrays[2])), None)]
    for retrieved, tile_rows in forms:
        kernels = cpu_kernels()
        means, per_query = h.hierarchical_precision_ranked(retrieved, labels, ks, tile_rows=tile_rows, kernels=kernels, **kw)
        assert kernels["complete_rankings"].calls == (1 if tile_rows is None else -(-len(as_dict) // tile_rows))
        check_against_fixture(g, key, means, per_query)
    host_means, host_q = h.hierarchical_precision(as_dict, labels, ks, **kw)
    check_against_fixture(g, key, host_means, host_q)
    means_only, none = h.hierarchical_precision_ranked(as_dict, labels, ks, per_query=False, kernels=cpu_kernels(), **kw)
    assert none is None and all(abs(means_only[m] - means[m]) <= 1e-13 for m in means)


def test_ranked_driver_with_ids_that_are_no_integers():
    """Tuple and string ids go through the dict look-up: the same values as the integer ids they stand for."""
    g, labels, as_dict, _, all_ids = partial_fixture()
    def name(i):
        return ("train", i) if i < 1000 else "query-%d" % i
    h, ks = hierarchy(), g["ks"].tolist()
    want, want_q = h.hierarchical_precision_ranked(as_dict, labels, ks, compute_ahp=True, compute_ap=True, all_ids=all_ids, kernels=cpu_kernels())
    got, got_q = h.hierarchical_precision_ranked({name(q): [name(i) for i in r] for q, r in as_dict.items()}, {name(i): c for i, c in labels.items()},
                                                 ks, compute_ahp=True, compute_ap=True, all_ids=[name(i) for i in all_ids], kernels=cpu_kernels())
    assert got == want and all(got_q[m][name(q)] == v for m in want_q for q, v in want_q[m].items())


def full_rankings():
    """Every list of the fixture completed: 26 rankings of the whole gallery."""
    g, labels, as_dict, _, all_ids = partial_fixture()
    return g, labels, {q: cc.complete_list_reference(r, all_ids) for q, r in as_dict.items()}, all_ids


@pytest.mark.parametrize("ignore", [True, False])
def test_head_only_shortcut_completes_nothing(ignore):
    g, labels, full, all_ids = full_rankings()
    heads = {q: r[:30] for q, r in full.items()}
    h, kernels = hierarchy(), cpu_kernels()
    kw = dict(compute_ahp=20, compute_ap=False, ignore_qids=ignore, all_ids=all_ids)
    means, per_query = h.hierarchical_precision_ranked(heads, labels, [1, 5, 20], kernels=kernels, **kw)
    assert kernels["complete_rankings"].calls == 0
    want_means, want = h.hierarchical_precision(heads, labels, [1, 5, 20], **kw)
    assert set(per_query) == set(want)
    for m in want:
        assert max(abs(per_query[m][q] - want[m][q]) for q in heads) <= TOL, m
        assert abs(means[m] - want_means[m]) <= TOL
    # one list too short for the head (21 entries are needed), or a metric that reads on: the lists are completed
    heads[next(iter(heads))] = heads[next(iter(heads))][:20]
    h.hierarchical_precision_ranked(heads, labels, [1, 5, 20], kernels=kernels, **kw)
    assert kernels["complete_rankings"].calls == 1
    h.hierarchical_precision_ranked({q: r[:30] for q, r in full.items()}, labels, [1, 5, 20], kernels=kernels, **dict(kw, compute_ap=True))
    assert kernels["complete_rankings"].calls == 2


def test_full_lists_without_all_ids():
    """No all_ids: the gallery is the first list's id set, every list a permutation of it -- the host function's values."""
    g, labels, full, _ = full_rankings()
    h = hierarchy()
    means, per_query = h.hierarchical_precision_ranked(full, labels, [1, 10, 50], compute_ahp=True, compute_ap=True, kernels=cpu_kernels())
    want_means, want = h.hierarchical_precision(full, labels, [1, 10, 50], compute_ahp=True, compute_ap=True)
    for m in want:
        assert max(abs(per_query[m][q] - want[m][q]) for q in full) <= TOL, m


@pytest.mark.parametrize("ignore", [True, False])
@pytest.mark.parametrize("bins", [None, 10])
def test_recall_precision_ranked_equals_the_host_statement(bins, ignore):
    import warnings
    from recall_precision import recall_precision_host_gallery, recall_precision_ranked
    g, labels, as_dict, as_arrays, all_ids = partial_fixture()
    pos = {i: j for j, i in enumerate(all_ids)}
    ranking = np.array([[pos[i] for i in cc.complete_list_reference(as_dict[int(q)], all_ids)] for q in g["query_ids"]])
    qidx = np.array([pos.get(int(q), -1) for q in g["query_ids"]]) if ignore else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = recall_precision_host_gallery(ranking, g["query_labels"].tolist(), [labels[i] for i in all_ids], qidx, bins)
        for retrieved, tile_rows in ((as_dict, None), (as_arrays, 4)):
            got = recall_precision_ranked(retrieved, labels, bins=bins, ignore_qids=ignore, all_ids=all_ids, tile_rows=tile_rows, kernels=cpu_kernels())
            assert np.array_equal(got[0], want[0])
            assert np.abs(got[1] - want[1]).max() <= 1e-12 and abs(got[2] - want[2]) <= 1e-12 and np.abs(got[3] - want[3]).max() <= 1e-12


def test_value_errors():
    from recall_precision import recall_precision_ranked
    g, labels, as_dict, as_arrays, all_ids = partial_fixture()
    h, kernels = hierarchy(), cpu_kernels()
    q0 = int(g["query_ids"][3])
    # an id that is not in the gallery: named, with its query
    bad = dict(as_dict)
    bad[q0] = bad[q0][:2] + [4711] + bad[q0][2:]
    for call in (lambda r: h.hierarchical_precision_ranked(r, dict(labels, **{}), [1, 5], compute_ap=True, all_ids=all_ids, kernels=kernels),
                 lambda r: recall_precision_ranked(r, labels, all_ids=all_ids, kernels=kernels)):
        with pytest.raises(ValueError, match=r"4711.*query %d\b" % q0):
            call(bad)
    arr = as_arrays[1].copy()
    arr[3, 1] = 4711
    with pytest.raises(ValueError, match=r"4711.*query %d\b" % q0):
        h.hierarchical_precision_ranked((as_arrays[0], arr, as_arrays[2]), labels, [1, 5], compute_ap=True, all_ids=all_ids, kernels=kernels)
    arr[3, 1] = as_arrays[1][3, 1]
    arr[3, 59] = 4711               # behind the row's length: not an entry
    assert g["lengths"][3] < 60
    h.hierarchical_precision_ranked((as_arrays[0], arr, as_arrays[2]), labels, [1, 5], compute_ap=True, all_ids=all_ids, kernels=kernels)
    # a duplicate: its query named
    dup = dict(as_dict)
    dup[q0] = dup[q0] + dup[q0][:1]
    for call in (lambda r: h.hierarchical_precision_ranked(r, labels, [1, 5], compute_ap=True, all_ids=all_ids, kernels=kernels),
                 lambda r: recall_precision_ranked(r, labels, all_ids=all_ids, kernels=kernels)):
        with pytest.raises(ValueError, match=r"query %d\b.*more than once" % q0):
            call(dup)
    with pytest.raises(ValueError, match="not distinct"):
        h.hierarchical_precision_ranked(as_dict, labels, [1], all_ids=all_ids + all_ids[:1], kernels=kernels)
    # partial lists without all_ids: the host function and all_ids are named
    with pytest.raises(ValueError, match=r"(?s)all_ids.*host hierarchical_precision"):
        h.hierarchical_precision_ranked(as_dict, labels, [1, 5], kernels=kernels)
    with pytest.raises(ValueError, match="all_ids"):
        recall_precision_ranked(as_arrays, labels, kernels=kernels)
    # cut-offs beyond the list: 90 gallery items, 89 once a query's own item is dropped
    for kw in (dict(ks=[1, 90]), dict(ks=[1], compute_ahp=90), dict(ks=[0, 1]), dict(ks=[91], ignore_qids=False)):
        with pytest.raises(ValueError, match="cut-offs"):
            h.hierarchical_precision_ranked(as_dict, labels, all_ids=all_ids, kernels=kernels, **kw)
    h.hierarchical_precision_ranked(as_dict, labels, [90], ignore_qids=False, all_ids=all_ids, kernels=kernels)
    # an empty gallery
    with pytest.raises(ValueError, match="gallery is empty"):
        h.hierarchical_precision_ranked({q0: []}, labels, [1], kernels=kernels)
    with pytest.raises(ValueError, match="gallery is empty"):
        recall_precision_ranked({q0: []}, labels, all_ids=[], kernels=kernels)
    with pytest.raises(ValueError, match="2-d integer"):
        h.hierarchical_precision_ranked((as_arrays[0], as_arrays[1].astype(np.float32)), labels, [1], all_ids=all_ids, kernels=kernels)


def test_tiles_are_sized_from_the_free_memory(monkeypatch):
    """A budget that holds three query rows: tiles of three; one that holds none: a ValueError with the estimate; tile_rows overrides
    the size, not the check."""
    import class_hierarchy
    from recall_precision import ranked_tile_rows
    g, labels, as_dict, _, all_ids = partial_fixture()
    h, ks = hierarchy(), g["ks"].tolist()
    C, ng, L, ncol = len(set(labels.values())), 90, 60, 2 * len(ks) + 3
    fixed, row = 2 * 8 * C * ng, 4 * 92 + 28 * L + 8 * ncol
    assert ranked_tile_rows(torch.device("cpu"), 26, ng, L, fixed, 8 * ncol, None, "x") == 26          # nothing to size against
    monkeypatch.setattr(class_hierarchy, "_free_device_bytes", lambda dev: (fixed + 3 * row + row // 2) * 10 // 9 + 1)
    assert ranked_tile_rows(torch.device("cpu"), 26, ng, L, fixed, 8 * ncol, None, "x") == 3
    kernels = cpu_kernels()
    means, per_query = h.hierarchical_precision_ranked(as_dict, labels, ks, compute_ahp=True, compute_ap=True, all_ids=all_ids, kernels=kernels)
    assert kernels["complete_rankings"].calls == 9
    check_against_fixture(g, "ahpTrue_ignore1", means, per_query)
    with pytest.raises(ValueError, match=r"estimated [\d,]+ bytes.*tile of 5 query rows"):
        h.hierarchical_precision_ranked(as_dict, labels, ks, compute_ahp=True, all_ids=all_ids, tile_rows=5, kernels=kernels)
    monkeypatch.setattr(class_hierarchy, "_free_device_bytes", lambda dev: fixed)
    with pytest.raises(ValueError, match=r"estimated [\d,]+ bytes.*tile of 1 query row\)"):
        h.hierarchical_precision_ranked(as_dict, labels, ks, compute_ahp=True, all_ids=all_ids, kernels=kernels)


def test_no_queries():
    from recall_precision import recall_precision_ranked
    _, labels, _, _, all_ids = partial_fixture()
    means, per_query = hierarchy().hierarchical_precision_ranked({}, labels, [1, 10], compute_ahp=True, compute_ap=True, all_ids=all_ids,
                                                                 kernels=cpu_kernels())
    assert list(means) == ["P@1 (WUP)", "P@1 (LCS_HEIGHT)", "P@10 (WUP)", "P@10 (LCS_HEIGHT)", "AHP (WUP)", "AHP (LCS_HEIGHT)", "AP"]
    assert all(np.isnan(v) for v in means.values()) and all(v == {} for v in per_query.values())
    means, none = hierarchy().hierarchical_precision_ranked((np.zeros(0, dtype=np.int64), np.zeros((0, 5), dtype=np.int64)), labels, [1],
                                                            all_ids=all_ids, per_query=False, kernels=cpu_kernels())
    assert none is None and np.isnan(means["P@1 (WUP)"])
    levels, mean_precision, mAP, aps = recall_precision_ranked({}, labels, all_ids=all_ids, kernels=cpu_kernels())
    assert len(levels) == 0 and len(mean_precision) == 0 and np.isnan(mAP) and len(aps) == 0


# ---------------------------------------------------------------------------------------------- the command line

def test_cli_parsing():
    import evaluate_rankings as evr
    base = ["--dataset", "d", "--data_root", "r", "--hierarchy", "h"]
    args = evr.parse_args(base + ["--ranking", "a.pickle", "--ranking", "b.npz", "--label", "A"])
    assert args.ranking == ["a.pickle", "b.npz"] and args.gallery_split == "test" and not args.no_all_ids and not args.keep_queries
    assert args.plot_max == 250 and args.prec_type == "LCS_HEIGHT" and args.clip_ahp is None and not args.skip_ap and args.recprec_csv is None
    assert evr.ranking_entry(args, 0) == "A" and evr.ranking_entry(args, 1) == "b"
    args = evr.parse_args(base + ["--ranking", "a", "--gallery_split", "train", "--no_all_ids", "--keep_queries", "--clip_ahp", "50", "--skip_ap",
                                  "--recprec_csv", "c.csv", "--bins", "10", "--str_ids", "--is_a", "--classes_from", "x"])
    assert args.gallery_split == "train" and args.no_all_ids and args.keep_queries and args.clip_ahp == 50 and args.skip_ap
    assert args.recprec_csv == "c.csv" and args.bins == 10 and args.str_ids and args.is_a and args.classes_from == "x"
    with pytest.raises(SystemExit):
        evr.parse_args(base)
    with pytest.raises(SystemExit):
        evr.parse_args(base + ["--ranking", "a", "--gallery_split", "val"])


def test_cli_file_formats_and_train_tags(tmp_path):
    import evaluate_rankings as evr
    ret = {5: [1, 2, 3], 6: [3, 1]}
    with open(tmp_path / "r.pickle", "wb") as f:
        pickle.dump(ret, f)
    assert evr.load_ranking(str(tmp_path / "r.pickle")) == ret
    np.savez(tmp_path / "r.npz", query_ids=np.array([5, 6]), ranking=np.array([[1, 2, 3], [3, 1, -1]]), lengths=np.array([3, 2]))
    q, r, n = evr.load_ranking(str(tmp_path / "r.npz"))
    assert q.tolist() == [5, 6] and r.tolist() == [[1, 2, 3], [3, 1, -1]] and n.tolist() == [3, 2]
    np.savez(tmp_path / "full.npz", query_ids=np.array([5]), ranking=np.array([[1, 2, 3]]))
    assert evr.load_ranking(str(tmp_path / "full.npz"))[2] is None
    np.savez(tmp_path / "bad.npz", ranking=np.array([[1]]))
    with pytest.raises(ValueError, match="query_ids"):
        evr.load_ranking(str(tmp_path / "bad.npz"))
    with open(tmp_path / "list.pickle", "wb") as f:
        pickle.dump([1, 2], f)
    with pytest.raises(ValueError, match="dict"):
        evr.load_ranking(str(tmp_path / "list.pickle"))
    tagged = {5: [("train", 1), ("train", 2), ("train", 3)], 6: [("train", 3), ("train", 1)]}
    assert dict(evr.tag_train_ids(ret)) == tagged
    assert dict(evr.tag_train_ids((q, r, n))) == tagged
    assert dict(evr.tag_train_ids(tagged)) == tagged


def test_cli_end_to_end_on_stand_ins(tmp_path, monkeypatch, capsys):
    """main() with the drivers running on the CPU stand-ins: both file formats print the table of the host function's values; the
    train split's ids are tagged; --keep_queries, --no_all_ids, --clip_ahp and --skip_ap reach the drivers."""
    import class_hierarchy
    import evaluate_rankings as evr
    import recall_precision
    from datasets import get_data_generator
    hpath = tmp_path / "cifar.parent-child.txt"
    with open(hpath, "w") as f:
        for p, c in np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))["edges"]:
            f.write("%d %d\n" % (p, c))
    ds = "synthetic:100x8x150x120"
    gen = get_data_generator(ds, None)
    labels_test, labels_train = list(gen.labels_test), list(gen.labels_train)
    n_test, n_train = len(labels_test), len(labels_train)
    rng = np.random.default_rng(2)
    # every query first in its own list of 25 test ids
    lists = np.stack([np.concatenate([[i], rng.permutation(np.setdiff1d(np.arange(n_test), [i]))[:24]]) for i in range(n_test)])
    as_dict = {i: lists[i].tolist() for i in range(n_test)}
    with open(tmp_path / "test.pickle", "wb") as f:
        pickle.dump(as_dict, f)
    np.savez(tmp_path / "test.npz", query_ids=np.arange(n_test), ranking=lists)
    train_lists = np.stack([rng.permutation(n_train)[:30] for _ in range(n_test)])
    np.savez(tmp_path / "train.npz", query_ids=np.arange(n_test), ranking=train_lists, lengths=np.full(n_test, 28))

    seen = []
    real_h, real_rp = class_hierarchy.ClassHierarchy.hierarchical_precision_ranked, recall_precision.recall_precision_ranked

    def hprec(self, retrieved, labels, ks, **kw):
        seen.append(("hprec", retrieved, labels, kw))
        return real_h(self, retrieved, labels, ks, kernels=cpu_kernels(), **kw)

    def recprec(retrieved, labels, **kw):
        seen.append(("recprec", retrieved, labels, kw))
        return real_rp(retrieved, labels, kernels=cpu_kernels(), **kw)

    monkeypatch.setattr(class_hierarchy.ClassHierarchy, "hierarchical_precision_ranked", hprec)
    monkeypatch.setattr(recall_precision, "recall_precision_ranked", recprec)
    common = ["--dataset", ds, "--data_root", str(tmp_path), "--hierarchy", str(hpath), "--plot_max", "0"]
    perf = evr.main(common + ["--ranking", str(tmp_path / "test.pickle"), "--ranking", str(tmp_path / "test.npz"), "--label", "p", "--label", "z",
                              "--csv", str(tmp_path / "out.csv"), "--recprec_csv", str(tmp_path / "rp.csv"), "--bins", "5"])
    out = capsys.readouterr().out
    assert "P@1 (WUP)" in out and "AHP (LCS_HEIGHT)" in out and "mAP" in out
    assert perf["p"] == perf["z"]
    assert [s[0] for s in seen] == ["hprec", "recprec"] * 2
    assert all(s[3]["ignore_qids"] and s[3]["all_ids"] == list(range(n_test)) for s in seen)
    h = class_hierarchy.ClassHierarchy.from_file(str(hpath), id_type=int)
    want, _ = h.hierarchical_precision(as_dict, labels_test, [1, 10, 50, 100], compute_ahp=True, compute_ap=True, all_ids=list(range(n_test)))
    assert set(want) | {"mAP"} == set(perf["p"])
    for m, v in want.items():
        assert abs(perf["p"][m] - v) <= TOL, m
    assert abs(perf["p"]["mAP"] - want["AP"]) <= 1e-12
    assert (tmp_path / "out.csv").read_text().splitlines()[0] == "k;p;z"
    rows = (tmp_path / "rp.csv").read_text().splitlines()
    assert rows[0] == "ranking,level,mean_precision" and {r.split(",")[0] for r in rows[1:]} == {"p", "z"}

    # the train split as gallery: integer ids of the file become ('train', j), lengths are honoured, nothing is a query's own item
    del seen[:]
    perf = evr.main(common + ["--ranking", str(tmp_path / "train.npz"), "--gallery_split", "train", "--keep_queries", "--clip_ahp", "20", "--skip_ap"])
    (_, retrieved, labels, kw), = seen
    assert not kw["ignore_qids"] and kw["all_ids"] == [("train", j) for j in range(n_train)] and kw["compute_ahp"] == 20 and not kw["compute_ap"]
    assert list(retrieved) == list(range(n_test)) and retrieved[3] == [("train", int(j)) for j in train_lists[3, :28]]
    assert labels[("train", 7)] == labels_train[7] and labels[7] == labels_test[7]
    tagged = {i: [("train", int(j)) for j in train_lists[i, :28]] for i in range(n_test)}
    all_labels = dict(enumerate(labels_test))
    all_labels.update({("train", j): c for j, c in enumerate(labels_train)})
    want, _ = h.hierarchical_precision(tagged, all_labels, [1, 10, 50, 100], compute_ahp=20, ignore_qids=False,
                                       all_ids=[("train", j) for j in range(n_train)])
    assert set(perf["train"]) == set(want) and "AHP@20 (WUP)" in want and "AP" not in want
    for m, v in want.items():
        assert abs(perf["train"][m] - v) <= TOL, m
    header = [ln for ln in capsys.readouterr().out.splitlines() if "P@1 (WUP)" in ln]
    assert len(header) == 1 and "AHP@20 (WUP)" in header[0] and " AP" not in header[0]

    # --no_all_ids: partial lists are refused, naming the way out
    del seen[:]
    with open(tmp_path / "ragged.pickle", "wb") as f:
        pickle.dump({q: (r[:10] if q == 5 else r) for q, r in as_dict.items()}, f)
    with pytest.raises(ValueError, match="all_ids"):
        evr.main(common + ["--ranking", str(tmp_path / "ragged.pickle"), "--no_all_ids"])
    assert seen[0][3]["all_ids"] is None
