"""GPU: se_knn_vote (sehip.knn_vote) equals the NumPy restatement of its contract (tests/_knn_canon.py) bit for bit, over the
smallest shapes that reach each part of the kernel -- lists below, at, across and far beyond one wave's width (one to 32 steps of
the walk; 64 to 4,096 table slots; four or two queries per workgroup), cut-offs that complete inside and at the end of a step, a
ranking with and without a zero-vote tail, a grid that strides -- and knn_classification end to end against the oracle's ranking."""
import numpy as np
import pytest
import torch

from _knn_canon import PAD, canonical_ranking, constructed_cases, knn_vote_host

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_lists(q, L, n, C, kind, with_qidx, seed):
    """Random neighbour lists over a gallery of n items; kind: 'random', 'ties' (cls = index % 2: most classes tie) or 'pads'
    (30 % of the entries are 2^31 - 1 or -1).  ``with_qidx``: every second row holds its query's own index somewhere."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, size=(q, L)).astype(np.int32)
    cls = (np.arange(n) % min(2, C) if kind == "ties" else rng.integers(0, C, size=n)).astype(np.int32)
    if kind == "pads":
        holes = rng.random((q, L)) < 0.3
        idx[holes] = rng.choice(np.array([PAD, -1], dtype=np.int32), size=int(holes.sum()))
    qidx = None
    if with_qidx:
        qidx = rng.integers(0, n, size=q).astype(np.int32)
        rows = np.arange(0, q, 2)
        idx[rows, rng.integers(0, L, size=len(rows))] = qidx[rows]
    return idx, cls, qidx


def check(idx, cls, C, ks, top, qidx, pitch=0):
    import sehip
    idx_d = dev(idx)
    if pitch:       # rows further apart than they are long
        wide = torch.full((idx.shape[0], idx.shape[1] + pitch), -7, dtype=torch.int32, device="cuda")
        wide[:, :idx.shape[1]] = idx_d
        idx_d = wide[:, :idx.shape[1]]
    got_cls, got_votes = sehip.knn_vote(idx_d, dev(cls), C, ks, top=top, qidx=None if qidx is None else dev(qidx))
    want_cls, want_votes = knn_vote_host(idx, cls, C, ks, top, qidx)
    assert got_cls.dtype == torch.int32 and tuple(got_cls.shape) == (idx.shape[0], len(ks), top)
    assert np.array_equal(got_votes.cpu().numpy(), want_votes)
    assert np.array_equal(got_cls.cpu().numpy(), want_cls)


# (q, list_len, gallery, C, top, ks, kind, qidx, extra pitch)
SHAPES = [
    (1, 1, 10, 1, 1, [1], "random", False, 0),
    (3, 7, 40, 2, 2, [1, 5], "random", True, 0),                               # top == C
    (70, 7, 40, 100, 16, [7], "random", False, 0),                             # at most 7 voted classes: a zero-vote tail
    (70, 1, 300, 257, 5, [1], "random", True, 0),                              # a list that is the query alone: nobody votes
    (70, 64, 500, 100, 5, [1, 5, 20], "random", True, 0),
    (70, 65, 500, 257, 16, [65], "random", True, 3),
    (3, 65, 500, 1, 1, [1, 5, 20], "random", False, 0),
    (1, 64, 5000, 16384, 1, [64], "random", False, 5),
    (3, 300, 5000, 8142, 5, [1, 2, 5, 64, 65, 128, 299, 300], "random", True, 0),   # 8 cut-offs: inside, at the end of and across steps
    (70, 300, 2000, 100, 5, [1, 5, 20], "ties", False, 0),                     # two voted classes of 100
    (70, 300, 2000, 8142, 5, [1, 5, 20, 300], "pads", True, 0),                # fewer neighbours than the last cut-off
    (70, 2048, 5000, 16384, 16, [1, 5, 20], "random", True, 0),                # 4,096 slots: two queries per workgroup
    (70, 2048, 5000, 2, 2, [2048], "ties", True, 0),
    (3, 2048, 9000, 100, 5, [1, 63, 64, 65, 1000, 2046, 2047, 2048], "pads", True, 4),
    (3, 64, 5000, 1000000, 5, [1, 64], "random", False, 0),                    # the class count does not size anything
    (17000, 7, 300, 5, 5, [1, 7], "random", True, 0),                          # more queries than the grid holds: it strides
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "q%d-L%d-C%d-top%d-nk%d-%s" % (s[0], s[1], s[3], s[4], len(s[5]), s[6]))
def test_knn_vote_equals_the_host_vote(shape):
    q, L, n, C, top, ks, kind, with_qidx, pitch = shape
    idx, cls, qidx = make_lists(q, L, n, C, kind, with_qidx, seed=q + L)
    check(idx, cls, C, ks, top, qidx, pitch)


@pytest.mark.parametrize("name", sorted(constructed_cases()))
def test_knn_vote_on_constructed_lists(name):
    import sehip
    idx, cls, C, ks, top, qidx, want_cls, want_votes = constructed_cases()[name]
    got_cls, got_votes = sehip.knn_vote(dev(idx), dev(cls), C, ks, top=top, qidx=None if qidx is None else dev(qidx))
    assert np.array_equal(got_cls.cpu().numpy(), want_cls), (name, got_cls)
    assert np.array_equal(got_votes.cpu().numpy(), want_votes), (name, got_votes)


def test_knn_vote_on_a_side_stream():
    side = torch.cuda.Stream()
    idx, cls, qidx = make_lists(70, 64, 500, 100, "random", True, seed=9)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        check(idx, cls, 100, [1, 5, 20], 5, qidx)
    torch.cuda.synchronize()


def test_knn_vote_refuses_what_the_contract_excludes():
    import sehip
    idx, cls, _ = make_lists(3, 40, 100, 7, "random", False, seed=1)
    idx_d, cls_d = dev(idx), dev(cls)
    for ks, top in (([5, 1], 5), ([41], 5), ([0], 5), ([1], 8), ([1], 0), ([1], sehip.KNN_TOP_MAX + 1)):
        with pytest.raises(sehip.SehipError, match="code -1"):
            sehip.knn_vote(idx_d, cls_d, 7 if top <= 8 else 100, ks, top=top)
    with pytest.raises(sehip.SehipError, match="code -3"):          # more cut-offs than one launch takes
        sehip.knn_vote(idx_d, cls_d, 7, list(range(1, 35)), top=5)
    with pytest.raises(sehip.SehipError):
        sehip.knn_vote(idx_d.long(), cls_d, 7, [1])
    out_cls, out_votes = sehip.knn_vote(idx_d[:0], cls_d, 7, [1, 5])
    assert tuple(out_cls.shape) == (0, 2, 5) and tuple(out_votes.shape) == (0, 2, 5)


@pytest.fixture(scope="module")
def features():
    rng = np.random.default_rng(11)
    return rng.standard_normal((300, 24)).astype(np.float32), rng.integers(0, 7, size=300), rng.standard_normal((90, 24)).astype(np.float32)


@pytest.mark.parametrize("cosine", [False, True])
def test_knn_classification_end_to_end(features, cosine):
    """Device lists + device vote == the host vote over the head of the oracle's canonical ranking, bit for bit."""
    import evaluate_classification_accuracy as eca
    train, y, test = features
    ks = [1, 5, 20]
    ranks, votes = eca.knn_classification(train, y, test, ks=ks, normalize=cosine, return_votes=True)
    want_cls, want_votes = knn_vote_host(canonical_ranking(test, train, cosine)[:, :20], y, 7, ks, 5)
    for j, k in enumerate(ks):
        assert np.array_equal(ranks[k], want_cls[:, j]) and np.array_equal(votes[k], want_votes[:, j])
    # leave-one-out == the all-pairs ranking without each row itself; device tensors in
    loo = eca.knn_classification(torch.from_numpy(train).cuda(), y, ks=ks, normalize=cosine)
    full = canonical_ranking(train, train, cosine)
    others = np.stack([row[row != i][:20] for i, row in enumerate(full)])
    want_cls, _ = knn_vote_host(others, y, 7, ks, 5)
    for j, k in enumerate(ks):
        assert np.array_equal(loo[k], want_cls[:, j])
