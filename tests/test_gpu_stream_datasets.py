"""GPU: the streamed tier of the file-based datasets (datasets/files.py) against the resident tier on the same images -- the same
kernel, the same draws, so the batches are equal bit for bit -- through compose_batch, through sequences across an epoch boundary,
with the tier chosen per split by 'auto', and through the training command line."""
import pickle

import numpy as np
import pytest
import torch

import _stream_trees as trees

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return trees.write_ilsvrc(tmp_path_factory.mktemp("ilsvrc"))


def _tiers(root, **kw):
    from datasets import ILSVRCGenerator
    return ILSVRCGenerator(root, store="stream", prefetch_batches=2, **kw), ILSVRCGenerator(root, store="resident", **kw)


@pytest.mark.parametrize("dtype,color_mode,train", [(torch.float32, "rgb", True), (torch.bfloat16, "bgr", True), (torch.float32, "rgb", False)])
def test_streamed_batches_equal_resident_batches(dtype, color_mode, train, root):
    stream, resident = _tiers(root, seed=7, dtype=dtype, color_mode=color_mode)
    n = stream.num_train if train else stream.num_test
    assert (stream.num_train, stream.num_test) == (10, 3)
    ring = 2 + 2
    batches = [[(3 * k + j) % n for j in range(3)] for k in range(2 * ring + 1)]          # consecutive, byte sizes vary
    for k, idx in enumerate(batches):
        for nxt in batches[k + 1:k + 3]:
            stream.prefetch(nxt, train)
        got = stream.compose_batch(idx, train=train, augment=train)
        want = resident.compose_batch(idx, train=train, augment=train)
        assert got.shape == (3, 3, 224, 224) and got.dtype == dtype and got.is_cuda and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, want), (k, idx)
    st = stream._stores[train]
    assert st.tier == "stream" and len(st.ring) == ring and st.turn == 2 * ring + 1 and len(st.pending) == 0      # every slot used twice
    assert all(s.dev is not None and s.host.is_pinned() and s.dev.numel() == s.host.numel() for s in st.ring)
    assert resident._stores[train].tier == "resident" and set(stream._stores) == {train}
    if train:                       # augmentation drew something: two composes of the same indices differ
        assert not torch.equal(stream.compose_batch(batches[0], train=True, augment=True), got)


def test_a_whole_epoch_and_into_the_next(root):
    stream, resident = _tiers(root, seed=3)
    seqs = [g.train_sequence(4, shuffle=True, rank=1, world_size=2, seed=11) for g in (stream, resident)]
    assert len(seqs[0]) == 3
    for epoch in range(2):
        for b in range((3, 2)[epoch]):                   # a whole epoch, then two batches of the next permutation
            (X, y), (Xr, yr) = seqs[0][b], seqs[1][b]
            assert X.shape[1:] == (3, 224, 224) and X.shape[0] == len(y) and torch.equal(y, yr) and torch.equal(X, Xr)
        st = stream._stores[True]
        assert len(st.pending) == (0, 1)[epoch]           # an epoch leaves nothing announced behind; two batches in, the third is pending
        assert np.array_equal(seqs[0].perms[0], seqs[1].perms[0])
        for s in seqs:
            s.on_epoch_end()
    assert st.turn == 5


def test_auto_streams_only_the_split_that_does_not_fit(root):
    from datasets import ILSVRCGenerator
    resident = ILSVRCGenerator(root, seed=5)
    sizes = {t: resident._store(t).sizes.astype(np.int64) for t in (True, False)}
    nbytes = {t: int((s[:, 0] * s[:, 1]).sum()) * 3 for t, s in sizes.items()}
    assert nbytes[False] < nbytes[True]
    auto = ILSVRCGenerator(root, seed=5, store="auto", store_budget_bytes=(nbytes[False] + nbytes[True]) // 2)
    for train, idx in ((False, [0, 1, 2]), (True, [0, 4, 7, 9]), (True, [9, 9, 1]), (False, [2])):
        assert torch.equal(auto.compose_batch(idx, train=train, augment=train), resident.compose_batch(idx, train=train, augment=train))
    assert auto._stores[False].tier == "resident" and auto._stores[False].device_arena is not None
    assert auto._stores[True].tier == "stream" and auto._stores[True].turn == 2


def test_learn_image_embeddings_on_a_streamed_dataset(root, tmp_path, monkeypatch):
    import learn_image_embeddings as lie
    made = []

    def streaming_generator(*a, **k):
        g = lie_get(*a, **k)
        g.store_budget_bytes = 1           # 'auto' would keep thirteen tiny images resident: no split fits one byte
        made.append(g)
        return g

    lie_get = lie.get_data_generator
    monkeypatch.setattr(lie, "get_data_generator", streaming_generator)
    monkeypatch.setenv("SE_TRAIN_GRAPHS", "0")                                   # the step is not what this test is about
    feat = str(tmp_path / "feat.pickle")
    final = lie.main(["--dataset", "ILSVRC-stream", "--data_root", root, "--architecture", "simple", "--embedding", "onehot",
                      "--lr_schedule", "SGD", "--sgd_lr", "0.01", "--epochs", "1", "--batch_size", "4", "--read_workers", "2",
                      "--queue_size", "2", "--feature_dump", feat, "--no_progress"])
    assert np.isfinite(final["loss"])
    with open(feat, "rb") as f:
        dump = pickle.load(f)["feat"]
    assert sorted(dump) == [0, 1, 2] and all(np.asarray(v).shape == (3,) and np.isfinite(v).all() for v in dump.values())
    (g,) = made
    assert type(g).__name__ == "ILSVRCGenerator" and g.store == "auto" and g.decode_threads == 2 and g.prefetch_batches == 2
    assert g._decode_pool._max_workers == 2
    assert {t: st.tier for t, st in g._stores.items()} == {True: "stream", False: "stream"}
    assert all(len(st.ring) == 4 and st.turn >= 3 for st in g._stores.values())
