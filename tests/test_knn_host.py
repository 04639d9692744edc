"""CPU: the k-NN vote contract (tests/_knn_canon.py) against scikit-learn and hand-made lists, knn_classification and the --knn flag of
evaluate_classification_accuracy.py with CPU stand-ins, and the argument checks of se_knn_vote through raw ctypes."""
import ctypes

import numpy as np
import pytest
import torch

from _knn_canon import PAD, canonical_ranking, constructed_cases, knn_vote_host
from oracle import retrieval_oracle as ro


# ---- the restatement against scikit-learn ----

SKLEARN_SEED = 0


@pytest.fixture(scope="module")
def sklearn_problem():
    rng = np.random.default_rng(SKLEARN_SEED)
    train, test = rng.standard_normal((200, 16)).astype(np.float32), rng.standard_normal((60, 16)).astype(np.float32)
    y = rng.integers(0, 7, size=200)
    assert len(np.unique(y)) == 7
    return y, ro.canon_pdist(test, train, ro.METRIC_EUCLID), ro.canon_pdist(train, train, ro.METRIC_EUCLID)


def test_host_vote_equals_scikit_learn(sklearn_problem):
    from sklearn.neighbors import KNeighborsClassifier
    y, pd, pd_train = sklearn_problem
    ks = [1, 5, 20]
    srt = np.sort(pd, axis=1)
    for k in ks:        # the neighbour SET is defined: no tie between the k-th and the (k + 1)-th distance
        assert np.all(srt[:, k - 1] < srt[:, k]), k
    _, lists = ro.canon_topk_rows(pd, max(ks))
    out_cls, out_votes = knn_vote_host(lists, y, 7, ks, 7)
    assert np.array_equal(np.sort(out_cls, axis=-1), np.broadcast_to(np.arange(7), out_cls.shape))
    for j, k in enumerate(ks):
        clf = KNeighborsClassifier(n_neighbors=k, metric="precomputed", algorithm="brute").fit(np.maximum(pd_train.astype(np.float64), 0.0), y)
        assert np.array_equal(clf.classes_, np.arange(7))
        counts = np.rint(clf.predict_proba(pd.astype(np.float64)) * k).astype(np.int32)
        votes_by_class = np.zeros((60, 7), dtype=np.int32)
        np.put_along_axis(votes_by_class, out_cls[:, j].astype(np.int64), out_votes[:, j], axis=1)
        assert np.array_equal(votes_by_class, counts), k
        assert votes_by_class.sum(axis=1).tolist() == [k] * 60
        assert np.array_equal(clf.predict(pd.astype(np.float64)), out_cls[:, j, 0]), k


# ---- constructed lists ----

@pytest.mark.parametrize("name", sorted(constructed_cases()))
def test_host_vote_on_constructed_lists(name):
    idx, cls, C, ks, top, qidx, want_cls, want_votes = constructed_cases()[name]
    got_cls, got_votes = knn_vote_host(idx, cls, C, ks, top, qidx)
    assert got_cls.dtype == np.int32 and got_votes.dtype == np.int32
    assert np.array_equal(got_cls, want_cls), (name, got_cls)
    assert np.array_equal(got_votes, want_votes), (name, got_votes)


def test_constructed_lists_cover_the_contract():
    cases = constructed_cases()
    assert len(cases) == 7
    assert any((c[0] == PAD).any() and (c[0] == -1).any() for c in cases.values())
    assert any(c[5] is not None and c[0].shape[1] == max(c[3]) + 1 for c in cases.values())      # leave-one-out with list_len == k + 1


# ---- knn_classification with CPU stand-ins ----

def cpu_kernels(calls=None):
    def normalize_rows_(x):
        x.copy_(torch.from_numpy(ro.canon_normalize_rows(x.numpy())))
        return x

    def retrieve_topk(q, g, k, metric=ro.METRIC_COSINE, kblocks=None):
        if calls is not None:
            calls.append(("retrieve_topk", tuple(q.shape), tuple(g.shape), k, metric, kblocks))
        d, i = ro.canon_topk_rows(ro.canon_pdist(q.numpy(), g.numpy(), metric, kblocks=kblocks), k)
        return torch.from_numpy(d), torch.from_numpy(i)

    def knn_vote(idx, cls, C, ks, top=5, qidx=None):
        if calls is not None:
            calls.append(("knn_vote", tuple(idx.shape), C, list(ks), top, qidx is not None))
        oc, ov = knn_vote_host(idx.numpy(), cls.numpy(), C, ks, top, None if qidx is None else qidx.numpy())
        return torch.from_numpy(oc), torch.from_numpy(ov)

    return {"normalize_rows_": normalize_rows_, "retrieve_topk": retrieve_topk, "knn_vote": knn_vote, "device": torch.device("cpu")}


@pytest.fixture(scope="module")
def features():
    rng = np.random.default_rng(3)
    return rng.standard_normal((120, 12)).astype(np.float32), rng.integers(0, 6, size=120), rng.standard_normal((40, 12)).astype(np.float32)


@pytest.mark.parametrize("cosine", [False, True])
def test_knn_classification_equals_the_host_vote_on_the_canonical_ranking(features, cosine):
    import evaluate_classification_accuracy as eca
    train, y, test = features
    calls = []
    ks = (5, 1, 20)
    ranks, votes = eca.knn_classification(train.copy(), y, test.copy(), ks=ks, normalize=cosine, top=4, kernels=cpu_kernels(calls), return_votes=True)
    assert [c[0] for c in calls] == ["retrieve_topk", "knn_vote"]        # ONE list call with k = max(ks), one vote over ascending cut-offs
    assert calls[0][1:] == ((40, 12), (120, 12), 20, ro.METRIC_COSINE if cosine else ro.METRIC_EUCLID, None)
    assert calls[1][1:] == ((40, 20), 6, [1, 5, 20], 4, False)
    head = canonical_ranking(test, train, cosine)[:, :20]
    want_cls, want_votes = knn_vote_host(head, y, 6, [1, 5, 20], 4)
    assert list(ranks) == list(ks) and list(votes) == list(ks)
    for k, j in ((1, 0), (5, 1), (20, 2)):
        assert ranks[k].shape == (40, 4) and ranks[k].dtype == np.int32
        assert np.array_equal(ranks[k], want_cls[:, j]) and np.array_equal(votes[k], want_votes[:, j])


@pytest.mark.parametrize("cosine", [False, True])
def test_leave_one_out_drops_every_rows_own_index(features, cosine):
    import evaluate_classification_accuracy as eca
    train, y, _ = features
    calls = []
    ranks = eca.knn_classification(train.copy(), y, ks=[3, 7], normalize=cosine, num_classes=8, kernels=cpu_kernels(calls))
    assert calls[0][1:4] == ((120, 12), (120, 12), 8) and calls[1][1:] == ((120, 8), 8, [3, 7], 5, True)
    full = canonical_ranking(train, train, cosine)
    others = np.stack([row[row != i][:7] for i, row in enumerate(full)])          # the all-pairs ranking without the row itself
    want_cls, _ = knn_vote_host(others, y, 8, [3, 7], 5)
    assert np.array_equal(ranks[3], want_cls[:, 0]) and np.array_equal(ranks[7], want_cls[:, 1])


def test_knn_classification_refuses_lists_it_cannot_have(features):
    import evaluate_classification_accuracy as eca
    import sehip
    train, y, test = features

    def no_launch(*a, **k):
        raise AssertionError("launched")
    kernels = {"normalize_rows_": no_launch, "retrieve_topk": no_launch, "knn_vote": no_launch, "device": torch.device("cpu")}
    with pytest.raises(ValueError, match="training rows"):
        eca.knn_classification(train, y, test, ks=[1, 121], kernels=kernels)
    with pytest.raises(ValueError, match="leave-one-out"):
        eca.knn_classification(train, y, ks=[120], kernels=kernels)                 # 120 others need 121 rows
    big = np.zeros((sehip.TOPK_MAX + 10, 2), dtype=np.float32)
    yb = np.zeros(len(big), dtype=np.int64)
    with pytest.raises(ValueError, match=str(sehip.TOPK_MAX)):
        eca.knn_classification(big, yb, test[:, :2], ks=[sehip.TOPK_MAX + 1], kernels=kernels)
    with pytest.raises(ValueError, match=str(sehip.TOPK_MAX)):
        eca.knn_classification(big, yb, ks=[sehip.TOPK_MAX], kernels=kernels)       # + 1 for leave-one-out
    with pytest.raises(ValueError):
        eca.knn_classification(train, y, test, ks=[0], kernels=kernels)


def test_top_is_capped_at_the_number_of_classes(features):
    import evaluate_classification_accuracy as eca
    train, y, test = features
    ranks = eca.knn_classification(train.copy(), y % 2, test.copy(), ks=[3], kernels=cpu_kernels())
    assert ranks[3].shape == (40, 2)


# ---- command line ----

def _cli_fixture(tmp_path):
    from datasets import get_data_generator
    ds = "synthetic:10x8x40x30"
    data = get_data_generator(ds, "-")
    hier = tmp_path / "hierarchy.txt"
    hier.write_text("".join("%d %d\n" % (100 + c // 5, c) for c in range(10)) + "200 100\n200 101\n")
    return ds, data, str(hier)


def test_cli_knn_rows(tmp_path, capsys):
    import evaluate_classification_accuracy as eca
    ds, data, hier = _cli_fixture(tmp_path)
    rng = np.random.default_rng(1)
    calls, rankings = [], {}

    def knn(data_, model, layer, normalize, ks, custom, batch_size):
        calls.append(("knn", model, layer, normalize, list(ks), batch_size))
        rankings[model] = {k: np.stack([rng.permutation(10)[:5] for _ in range(data.num_test)]) for k in ks}
        return rankings[model]

    def prob(data_, model, layer, custom, batch_size):
        calls.append(("prob", model))
        return np.stack([rng.permutation(10) for _ in range(data.num_test)])

    def svm(*a):
        raise AssertionError("the SVM mode was called with --knn")

    perf = eca.main(["--dataset", ds, "--data_root", "-", "--hierarchy", hier, "--batch_size", "5", "--knn", "1", "5",
                     "--model", "m1", "--layer", "-1", "--norm", "1", "--model", "m2", "--layer", "fc", "--label", "one", "--label", "two",
                     "--model", "m3", "--layer", "2", "--prob_features", "0", "--prob_features", "0", "--prob_features", "1"],
                    modes={"knn": knn, "svm": svm, "prob": prob})
    assert calls == [("knn", "m1", -1, True, [1, 5], 5), ("knn", "m2", "fc", False, [1, 5], 5), ("prob", "m3")]
    assert list(perf) == ["one [k-NN, k=1]", "one [k-NN, k=5]", "two [k-NN, k=1]", "two [k-NN, k=5]", "m3"]
    from class_hierarchy import ClassHierarchy
    hierarchy = ClassHierarchy.from_file(hier, id_type=int)
    for lbl, model in (("one", "m1"), ("two", "m2")):
        for k in (1, 5):
            row = perf["%s [k-NN, k=%d]" % (lbl, k)]
            assert sorted(row) == sorted(eca.METRICS)
            assert row == eca.evaluate(rankings[model][k], data, hierarchy)
    assert "two [k-NN, k=5]" in capsys.readouterr().out


def test_cli_without_knn_is_unchanged():
    import evaluate_classification_accuracy as eca
    from datasets import get_data_generator
    ds = "synthetic:10x8x40x30"
    data = get_data_generator(ds, "-")
    calls = []

    def svm(data_, model, layer, normalize, epochs, C, custom, batch_size):
        calls.append("svm")
        return np.tile(np.arange(10), (data.num_test, 1))

    def knn(*a):
        calls.append("knn")
        raise AssertionError("the k-NN mode was called without --knn")

    args = eca.build_parser().parse_args(["--dataset", ds, "--data_root", "-", "--model", "m", "--layer", "-1"])
    assert args.knn is None
    perf = eca.main(["--dataset", ds, "--data_root", "-", "--model", "m", "--layer", "-1"], modes={"svm": svm, "knn": knn})
    assert calls == ["svm"] and list(perf) == ["m"]


# ---- the C ABI without a GPU ----

def test_knn_vote_argument_validation_without_gpu():
    import sehip
    lib = sehip.lib()
    INVALID = sehip._lib.DEFINES["SE_ERR_INVALID"]
    assert sehip._lib.DEFINES["SE_KNN_TOP_MAX"] == 16
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(16)       # device pointers are not read before the launch
    ks = (ctypes.c_int32 * 3)(1, 5, 20)

    def call(idx=p, ldi=32, q=4, list_len=32, cls=p, gallery=100, C=7, qidx=z, ks=ks, nk=3, top=5, out_cls=p, out_votes=p):
        return lib.se_knn_vote(idx, ldi, q, list_len, cls, gallery, C, qidx, ks, nk, top, out_cls, out_votes, None)

    def invalid(**kw):
        rc = call(**kw)
        msg = lib.se_last_error()
        assert rc == INVALID and msg and b"se_knn_vote" in msg, (kw, rc, msg)

    for name in ("idx", "cls", "ks", "out_cls", "out_votes"):
        invalid(**{name: z})
    invalid(ldi=31)
    for top in (0, -1, 17, 8):       # 8 > num_classes = 7
        invalid(top=top)
    invalid(ks=(ctypes.c_int32 * 3)(5, 1, 20))
    invalid(ks=(ctypes.c_int32 * 3)(1, 5, 5))
    invalid(ks=(ctypes.c_int32 * 3)(0, 5, 20))
    invalid(ks=(ctypes.c_int32 * 3)(1, 5, 33))
    invalid(C=0)
    invalid(list_len=sehip.TOPK_MAX + 1, ldi=4096)
    assert call(q=0) == 0
    assert call(nk=0, ks=z) == 0
    assert call(q=0, idx=z, cls=z, out_cls=z, out_votes=z) == 0
