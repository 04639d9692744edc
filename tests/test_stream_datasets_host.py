"""CPU: ILSVRC and iNaturalist metadata against what the reference's classes made of the same trees
(tests/golden/stream_datasets_meta.json, tools/make_stream_datasets_golden.py), the '-stream' dataset names, the host half of the
streamed store against slices of the resident arena, its errors and statistics, and the prefetch hook of DeviceBatchSequence."""
import os
import shutil

import numpy as np
import PIL.Image
import pytest
import torch

import _file_pipeline as fp
import _stream_trees as trees

IMAGENET_MEAN, IMAGENET_STD = [122.65435242, 116.6545058, 103.99789959], [71.40583196, 69.56888997, 73.0440314]
CAFFE_MEAN = [123.68, 116.779, 103.939]
TRAIN = "ILSVRC2012_img_train/"
VAL = "ILSVRC2012_img_val/"


@pytest.fixture(scope="module")
def golden():
    return trees.load_golden()


@pytest.fixture(scope="module")
def ilsvrc_root(tmp_path_factory):
    return trees.write_ilsvrc(tmp_path_factory.mktemp("ilsvrc"))


@pytest.fixture(scope="module")
def inat_root(tmp_path_factory):
    return trees.write_inat(tmp_path_factory.mktemp("inat"))


def _rel(files, root):
    return [os.path.relpath(f, root) for f in files]


def _check_meta(g, want, root):
    assert list(g.classes) == want["classes"] and g.num_classes == want["num_classes"] == len(want["classes"])
    assert {str(k): v for k, v in g.class_indices.items()} == want["class_indices"]
    assert _rel(g.train_img_files, root) == want["train_files"] and _rel(g.test_img_files, root) == want["test_files"]
    assert list(g.labels_train) == want["train_labels"] and list(g.labels_test) == want["test_labels"]
    assert g.num_train == len(want["train_labels"]) and g.num_test == len(want["test_labels"])


def _check_presets(g, want):
    assert tuple(g.cropsize) == tuple(want["cropsize"]) and g.default_target_size == want["default_target_size"]
    assert (g.randzoom_range is None) == (want["randzoom_range"] is None)
    assert g.randzoom_range is None or tuple(g.randzoom_range) == tuple(want["randzoom_range"])
    assert g.randerase_prob == want["randerase_prob"] == 0.0 and g.color_mode == want["color_mode"]
    for got, ref in ((g._mean, want["mean"]), (g._std, want["std"])):
        assert got.dtype == np.float32 and np.array_equal(got, np.asarray(ref, dtype=np.float32))


# ---- ILSVRC

def test_ilsvrc_metadata(ilsvrc_root, golden):
    from datasets import ILSVRCGenerator, get_data_generator
    g = get_data_generator("ilsvrc-stream", ilsvrc_root)
    assert type(g) is ILSVRCGenerator and g.store == "auto"
    c0, c1, c2 = trees.SYNSETS
    assert g.classes == [c0, c1, c2] and g.class_indices == {c0: 0, c1: 1, c2: 2}
    # sorted by path: "_10" before "_2", the nested directory before the synset's own files; the .txt files are no images
    assert _rel(g.train_img_files, ilsvrc_root) == [
        TRAIN + c0 + "/n01440764_10.JPEG", TRAIN + c0 + "/n01440764_2.JPEG", TRAIN + c0 + "/n01440764_31.JPEG", TRAIN + c0 + "/n01440764_7.JPEG",
        TRAIN + c1 + "/extra/n01443537_9.JPEG", TRAIN + c1 + "/n01443537_1.JPEG", TRAIN + c1 + "/n01443537_5.JPEG",
        TRAIN + c2 + "/n01484850_12.JPEG", TRAIN + c2 + "/n01484850_3.JPEG", TRAIN + c2 + "/n01484850_4.JPEG"]
    assert list(g.labels_train) == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert _rel(g.test_img_files, ilsvrc_root) == [VAL + c0 + "/ILSVRC2012_val_00000017.JPEG", VAL + c0 + "/ILSVRC2012_val_00000293.JPEG",
                                                   VAL + c1 + "/ILSVRC2012_val_00000236.JPEG"]
    assert list(g.labels_test) == [0, 0, 1] and g.num_channels == 3
    _check_meta(g, golden["ilsvrc"]["ilsvrc"], ilsvrc_root)
    r = get_data_generator("ilsvrc-stream", ilsvrc_root, classes=[c2, c0])
    assert r.classes == [c2, c0] and list(r.labels_train) == [0, 0, 0, 1, 1, 1, 1] and list(r.labels_test) == [1, 1]
    assert _rel(r.train_img_files, ilsvrc_root)[:3] == [TRAIN + c2 + "/n01484850_12.JPEG", TRAIN + c2 + "/n01484850_3.JPEG", TRAIN + c2 + "/n01484850_4.JPEG"]
    _check_meta(r, golden["ilsvrc"]["restricted"], ilsvrc_root)


@pytest.mark.parametrize("name,mean,std,color_mode", [("ilsvrc-stream", IMAGENET_MEAN, IMAGENET_STD, "rgb"),
                                                      ("ilsvrc-caffe-stream", CAFFE_MEAN, [1., 1., 1.], "bgr"),
                                                      ("ILSVRC-ilsvrcmean-stream", IMAGENET_MEAN, IMAGENET_STD, "rgb")])
def test_ilsvrc_presets(name, mean, std, color_mode, ilsvrc_root, golden):
    from datasets import get_data_generator
    g = get_data_generator(name, ilsvrc_root)
    assert g.cropsize == (224, 224) and g.default_target_size == 256 and g.randzoom_range == (256, 480) and g.randerase_prob == 0.0
    assert g.color_mode == color_mode and g.store == "auto" and g.prefetch_batches == 2 and g.decode_threads == 16
    assert np.array_equal(g._mean, np.asarray(mean, dtype=np.float32)) and np.array_equal(g._std, np.asarray(std, dtype=np.float32))
    _check_presets(g, golden["ilsvrc"][name[:-len("-stream")]])
    _check_meta(g, golden["ilsvrc"][name[:-len("-stream")]], ilsvrc_root)


def test_ilsvrc_takes_no_sizes(ilsvrc_root):
    from datasets import ILSVRCGenerator, get_data_generator
    with pytest.raises((TypeError, ValueError)):
        get_data_generator("ilsvrc-large-stream", ilsvrc_root)
    with pytest.raises((TypeError, ValueError)):
        ILSVRCGenerator(ilsvrc_root, default_target_size=512)
    with pytest.raises(ValueError):
        ILSVRCGenerator(ilsvrc_root, store="sometimes")


# ---- iNaturalist

def test_inat_metadata(inat_root, golden):
    from datasets import INatGenerator, get_data_generator
    path = lambda rel: os.path.abspath(os.path.join(inat_root, rel))
    g = get_data_generator("inat-stream", inat_root, classes=["ignored"])           # like the reference's factory: not forwarded
    assert type(g) is INatGenerator and g.store == "auto"
    # ids 3, 7, 12 -> 0, 1, 2; annotations in the order of the file
    assert g.train_tuples == [(2, path(fn)) if c == 12 else (1, path(fn)) if c == 7 else (0, path(fn)) for _, c, fn in trees.INAT_TRAIN]
    assert g.test_tuples == [(0, path(trees.INAT_VAL[0][2])), (2, path(trees.INAT_VAL[1][2])), (1, path(trees.INAT_VAL[2][2]))]
    assert g.classes == ["Quercus robur", "Turdus merula", "Parus major"] and g.num_classes == 3
    assert g.class_indices == {"Quercus robur": 0, "Turdus merula": 1, "Parus major": 2}
    assert list(g.labels_train) == [2, 1, 0, 0, 1, 2] and list(g.train_img_files) == [t[1] for t in g.train_tuples]
    assert g.cropsize == (224, 224) and g.default_target_size == 256 and g.randzoom_range == (256, 480) and g.randerase_prob == 0.0
    assert np.array_equal(g._mean, np.asarray([119.99310088, 122.86333725, 102.38318464], dtype=np.float32))

    a = get_data_generator("iNat_Aves-stream", inat_root)
    assert a.classes == ["Turdus merula", "Parus major"] and a.class_indices == {"Turdus merula": 0, "Parus major": 1} and a.num_classes == 2
    assert list(a.labels_train) == [1, 0, 0, 1] and list(a.labels_test) == [1, 0] and a.randzoom_range == (256, 480)
    assert a.train_tuples == [(1, path(trees.INAT_TRAIN[0][2])), (0, path(trees.INAT_TRAIN[1][2])), (0, path(trees.INAT_TRAIN[4][2])),
                              (1, path(trees.INAT_TRAIN[5][2]))]
    assert np.array_equal(a._mean, np.asarray([125.68554284, 131.58931007, 123.51576605], dtype=np.float32))
    assert np.array_equal(a._std, np.asarray([56.91926625, 57.04151665, 67.97284604], dtype=np.float32))

    big = get_data_generator("inat2018_aves-large-stream", inat_root)
    assert big.cropsize == (448, 448) and big.default_target_size == 512 and big.randzoom_range is None and big.store == "auto"
    assert big.train_tuples == a.train_tuples and big.classes == a.classes and np.array_equal(big._mean, a._mean)

    n19 = get_data_generator("inat2019-stream", inat_root)
    assert n19.classes == ["2", "40"] and n19.class_indices == {"2": 0, "40": 1} and n19.num_classes == 2
    assert n19.train_tuples == [(1, path(trees.INAT19_TRAIN[0][2])), (0, path(trees.INAT19_TRAIN[1][2])), (1, path(trees.INAT19_TRAIN[2][2]))]
    assert list(n19.labels_test) == [0, 1] and n19.randzoom_range == (256, 480)
    assert np.array_equal(n19._mean, np.asarray([115.77492586, 120.84414891, 93.51744386], dtype=np.float32))
    assert np.array_equal(n19._std, np.asarray([60.46127213, 58.63136496, 63.5872299], dtype=np.float32))

    for name, gen in (("inat", g), ("iNat_Aves", a), ("inat2018_aves-large", big), ("inat2019", n19)):
        want = golden["inat"][name]
        _check_meta(gen, want, inat_root)
        _check_presets(gen, want)
        assert [[l, os.path.relpath(f, inat_root)] for l, f in gen.train_tuples] == want["train_tuples"]
        assert [[l, os.path.relpath(f, inat_root)] for l, f in gen.test_tuples] == want["test_tuples"]
    with pytest.raises(ValueError):
        get_data_generator("inat2020-stream", inat_root)


# ---- names, laziness

def test_stream_suffix_on_existing_names(tmp_path):
    from datasets import NABGenerator, get_data_generator
    root = fp.write_tree(fp.load_fixture(), tmp_path)
    g = get_data_generator("cub-stream", root)
    assert type(g) is NABGenerator and g.store == "auto" and g.cropsize == (448, 448) and g.num_train == 7
    big = get_data_generator("nab-large-stream", root)
    assert big.store == "auto" and big.default_target_size == 512 and big.randzoom_range is None
    assert get_data_generator("cub", root).store == "resident"
    with pytest.raises(ValueError):
        get_data_generator("cifar-100-stream", root)


def test_constructing_and_listing_opens_no_image(ilsvrc_root, inat_root, monkeypatch):
    from datasets import get_data_generator
    opened = []
    real_open = PIL.Image.open
    monkeypatch.setattr(PIL.Image, "open", lambda *a, **k: (opened.append(a[0]), real_open(*a, **k))[1])
    for g in (get_data_generator("ilsvrc-stream", ilsvrc_root), get_data_generator("inat-stream", inat_root)):
        assert len(g.labels_test) == 3 and len(g.labels_train) in (10, 6)
        assert len(g.test_sequence(2)) == 2 and len(g.train_sequence(4)) in (3, 2)
        assert g._stores == {} and g._decode_pool is None
    assert opened == []


# ---- the host half of the streamed store

@pytest.fixture(scope="module")
def resident(ilsvrc_root):
    """The resident arena of the ten training images: decoded once, read by every test below."""
    from datasets import ILSVRCGenerator
    g = ILSVRCGenerator(ilsvrc_root)
    st = g._decode(g.train_img_files)
    assert st.tier == "resident" and len(st.offsets) == 10
    modes = [PIL.Image.open(f).mode for f in g.train_img_files]
    assert modes.count("L") == 1 and modes.count("CMYK") == 1                      # .convert('RGB') has work to do
    return st


def _stream_store(root, **kw):
    from datasets import ILSVRCGenerator
    g = ILSVRCGenerator(root, store="stream", **kw)
    st = g._store(True, upload=False)
    assert st.tier == "stream" and not hasattr(st, "arena")
    return g, st


def _staged_equals_resident(st, resident, idx):
    slot, nbytes, offsets, sizes = st.stage(idx)
    host = slot.view(nbytes)
    assert offsets.dtype == np.int64 and sizes.dtype == np.int32 and sizes.shape == (len(idx), 2)
    assert np.array_equal(sizes, resident.sizes[idx])
    for b, i in enumerate(idx):
        n = int(sizes[b, 0]) * int(sizes[b, 1]) * 3
        assert 0 <= offsets[b] and offsets[b] + n <= nbytes
        assert np.array_equal(host[offsets[b]:offsets[b] + n], resident.arena[resident.offsets[i]:resident.offsets[i] + n]), (idx, b)
    distinct = sorted(set(idx))
    assert nbytes == sum(int(resident.sizes[i, 0]) * int(resident.sizes[i, 1]) * 3 for i in distinct)     # packed, every image once
    return slot


BATCHES = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9], [4, 4, 2], [7], [5, 0, 9]]      # batches of 3 from 10, a repeated index, batches of 1


@pytest.mark.parametrize("ahead", [0, 2])
@pytest.mark.parametrize("pattern", ["in_order", "out_of_order", "never", "all_at_once"])
def test_staged_batches_equal_slices_of_the_resident_arena(pattern, ahead, ilsvrc_root, resident):
    g, st = _stream_store(ilsvrc_root, prefetch_batches=ahead, decode_threads=3)
    assert len(st.ring) == ahead + 2 and g.prefetch_batches == ahead
    slots = []
    if pattern == "in_order":                                       # what a sequence does: the next `ahead` batches before each one
        for k, idx in enumerate(BATCHES):
            for nxt in BATCHES[k + 1:k + 1 + ahead]:
                g.prefetch(nxt, True)
            slots.append(_staged_equals_resident(st, resident, idx))
            assert len(st.pending) <= ahead
    elif pattern == "out_of_order":                                 # announced one way, collected another
        order = [2, 0, 1, 3, 6, 4, 5]
        for k in order[:ahead + 2]:
            g.prefetch(BATCHES[k], True)
        for k in reversed(order):
            slots.append(_staged_equals_resident(st, resident, BATCHES[k]))
    elif pattern == "never":
        for idx in BATCHES:
            slots.append(_staged_equals_resident(st, resident, idx))
        assert len(st.pending) == 0
    else:                                                           # more announcements than the ring holds: the oldest are dropped
        for idx in BATCHES:
            g.prefetch(idx, True)
        assert len(st.pending) == len(st.ring) and list(st.pending) == [tuple(b) for b in BATCHES[-len(st.ring):]]
        for idx in BATCHES:
            slots.append(_staged_equals_resident(st, resident, idx))
    assert len(st.pending) == 0
    assert [st.ring.index(s) for s in slots] == [k % len(st.ring) for k in range(7)]          # every slot in turn, each reused
    assert g._decode_pool._max_workers == 3


def test_prefetch_of_a_resident_or_unopened_split_does_nothing(ilsvrc_root):
    from datasets import ILSVRCGenerator
    g = ILSVRCGenerator(ilsvrc_root, store="stream")
    g.prefetch([0, 1], True)
    assert g._stores == {} and g._decode_pool is None
    r = ILSVRCGenerator(ilsvrc_root)
    assert r.store == "resident"
    r._store(True, upload=False)
    r.prefetch([0, 1], True)
    assert r._decode_pool is None


def test_a_decode_error_names_the_file_and_leaves_the_store_usable(ilsvrc_root, resident, tmp_path):
    import sehip
    root = str(tmp_path / "broken")
    shutil.copytree(ilsvrc_root, root)
    g, st = _stream_store(root, prefetch_batches=1)
    bad = g.train_img_files[4]
    with open(bad, "rb") as f:
        data = f.read()
    with open(bad, "wb") as f:
        f.write(data[:len(data) // 2])
    for announced in (False, True):
        if announced:
            g.prefetch([3, 4, 5], True)
        with pytest.raises(sehip.SehipError, match="n01443537_9.JPEG"):
            st.stage([3, 4, 5])
        assert st.turn == 0 and len(st.pending) == 0 and all(s.host is None for s in st.ring)       # no slot was touched
    with pytest.raises(sehip.SehipError, match="n01443537_9.JPEG"):
        st.stage([4, 4])
    _staged_equals_resident(st, resident, [3, 5, 6])
    with pytest.raises(sehip.SehipError, match="n01443537_9.JPEG"):          # the statistics pass meets the same file
        type(g)(root, mean=None, std=None, store="stream").mean


def test_streamed_statistics_equal_the_resident_ones(ilsvrc_root):
    from datasets import ILSVRCGenerator
    want = ILSVRCGenerator(ilsvrc_root, mean=None, std=None, store="resident")
    got = ILSVRCGenerator(ilsvrc_root, mean=None, std=None, store="stream", decode_threads=4)
    assert got.mean.dtype == got.std.dtype == np.float32
    assert np.array_equal(got.mean, want.mean) and np.array_equal(got.std, want.std)
    assert got._stores[True].tier == "stream" and want._stores[True].tier == "resident"
    only_std = ILSVRCGenerator(ilsvrc_root, std=None, store="stream")
    assert np.array_equal(only_std.mean, np.asarray(IMAGENET_MEAN, dtype=np.float32)) and only_std.std.shape == (3,)
    # a window shorter than the split: still every image, in file order
    small = ILSVRCGenerator(ilsvrc_root, mean=None, std=None, store="stream")
    small._stream = lambda files: _windowed(small, files, 3)
    assert np.array_equal(small.mean, want.mean) and np.array_equal(small.std, want.std)


def _windowed(gen, files, window):
    from datasets.files import _StreamStore
    st = _StreamStore(files, gen._pool, gen.prefetch_batches)
    st.STATS_WINDOW = window
    return st


def test_auto_decides_per_split_from_the_header_pass(ilsvrc_root, resident):
    from datasets import ILSVRCGenerator
    train_bytes = int(resident.sizes.astype(np.int64).prod(axis=1).sum()) * 3
    g = ILSVRCGenerator(ilsvrc_root, store="auto", store_budget_bytes=train_bytes - 1)
    assert g._store(True, upload=False).tier == "stream" and g._store(False, upload=False).tier == "resident"
    fits = ILSVRCGenerator(ilsvrc_root, store="auto", store_budget_bytes=train_bytes)
    assert fits._store(True, upload=False).tier == "resident"
    import sehip
    with pytest.raises(sehip.SehipError):                                          # 'resident' keeps refusing
        ILSVRCGenerator(ilsvrc_root, store_budget_bytes=train_bytes - 1)._store(True, upload=False)


# ---- the prefetch hook of DeviceBatchSequence

class _Recorder(object):
    prefetch_batches = 2

    def __init__(self):
        self.events = []

    def prefetch(self, indices, train):
        self.events.append(("announce", [int(i) for i in indices], train))

    def compose_batch(self, indices, train=True, augment=False, **kw):
        self.events.append(("compose", [int(i) for i in indices], train))
        return torch.from_numpy(np.asarray(indices, dtype=np.int64))


class _Plain(object):
    def compose_batch(self, indices, train=True, augment=False, **kw):
        return torch.from_numpy(np.asarray(indices, dtype=np.int64))


@pytest.mark.parametrize("rows,shuffle", [(10, False), (10, True), (9, True)])
def test_sequence_announces_the_next_batches_of_the_pass(rows, shuffle):
    """Batch size 4, rank 1 of 2.  9 rows: the last global batch has one row, which rank 1 re-uses (the short-last-batch rule)."""
    from datasets import DeviceBatchSequence
    labels = np.arange(rows) % 3
    ids = np.arange(rows) + 100
    rec = _Recorder()
    seq = DeviceBatchSequence(rec, ids, labels, batch_size=4, shuffle=shuffle, train=True, rank=1, world_size=2, seed=5)
    plain = DeviceBatchSequence(_Plain(), ids, labels, batch_size=4, shuffle=shuffle, train=True, rank=1, world_size=2, seed=5)
    assert len(seq) == 3
    for epoch in range(2):
        del rec.events[:]
        perm = seq.perms[0].copy()
        sel = [perm[b * 4:(b + 1) * 4][1::2] for b in range(3)]
        if rows == 9:
            assert len(sel[2]) == 0
            sel[2] = perm[8:9]
        want = [ids[s].tolist() for s in sel]
        got = [(X.tolist(), y.tolist()) for X, y in seq]
        assert [x for x, _ in got] == want and [y for _, y in got] == [labels[s].tolist() for s in sel]
        assert rec.events == [("announce", want[1], True), ("announce", want[2], True), ("compose", want[0], True),
                              ("announce", want[2], True), ("compose", want[1], True),
                              ("compose", want[2], True)]                    # nothing beyond the pass, nothing after the last batch
        assert [(X.tolist(), y.tolist()) for X, y in plain] == got           # a generator without the method: the same batches
        assert np.array_equal(plain.perms[0], seq.perms[0])
    if not shuffle:
        assert want == [[101, 103], [105, 107], [109]]
    rec.prefetch_batches = 0
    del rec.events[:]
    seq[0]
    assert [e[0] for e in rec.events] == ["compose"]


def test_sequence_with_sub_epochs_announces_within_one_permutation():
    from datasets import DeviceBatchSequence
    rec = _Recorder()
    seq = DeviceBatchSequence(rec, np.arange(6), np.zeros(6, dtype=int), batch_size=4, shuffle=True, train=False, seed=1, repeats=2)
    assert len(seq) == 4
    seq[1]                                                                    # the last batch of the first permutation
    assert [e[0] for e in rec.events] == ["compose"]
    del rec.events[:]
    seq[2]
    assert rec.events == [("announce", seq.perms[1][4:].tolist(), False), ("compose", seq.perms[1][:4].tolist(), False)]


def test_read_workers_and_queue_size_configure_a_streaming_generator(ilsvrc_root, tmp_path):
    import argparse
    import train_cli
    from datasets import get_data_generator
    args = argparse.Namespace(read_workers=40, queue_size=100)
    g = train_cli.configure_loader(args, get_data_generator("ilsvrc-stream", ilsvrc_root))
    assert g.decode_threads == 16 and g.prefetch_batches == 4
    g = train_cli.configure_loader(argparse.Namespace(read_workers=2, queue_size=1), g)
    assert g.decode_threads == 2 and g.prefetch_batches == 1
    assert len(g._stream(g.train_img_files).ring) == 3 and g._pool()._max_workers == 2
    cub = get_data_generator("cub", fp.write_tree(fp.load_fixture(), tmp_path))
    assert train_cli.configure_loader(args, cub).decode_threads == 16 and cub.prefetch_batches == 2      # resident: nothing to configure
    synthetic = get_data_generator("synthetic:10x8x64x32", ".")
    assert train_cli.configure_loader(args, synthetic) is synthetic and not hasattr(synthetic, "decode_threads")
