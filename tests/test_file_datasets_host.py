"""CPU: file-based datasets -- file lists, labels and statistics against what the reference's generators made of the same tree
(tests/golden/file_pipeline.npz, tools/make_file_pipeline_golden.py), the presets of get_data_generator, the resampling tables
against live Pillow, the host restatement of the reference's batch composition against its recorded batches, the distributions of
draw_params, and sub-epochs of DeviceBatchSequence."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

import _file_pipeline as fp


@pytest.fixture(scope="module")
def golden():
    return fp.load_fixture()


@pytest.fixture(scope="module")
def tree(golden, tmp_path_factory):
    return fp.write_tree(golden, tmp_path_factory.mktemp("file_pipeline"))


def _makers(root):
    from datasets import CarsGenerator, FlowersGenerator, NABGenerator, SubDirectoryGenerator
    return {
        "nab": lambda: NABGenerator(root, mean=None, std=None),
        "nab_restricted": lambda: NABGenerator(root, classes=[9, 3], mean=None, std=None),
        "subdir": lambda: SubDirectoryGenerator(root, img_dir="images"),
        "subdir_restricted": lambda: SubDirectoryGenerator(root, classes=["c08", "c05"], img_dir="images"),
        "cars": lambda: CarsGenerator(root, mean=None, std=None),
        "cars_restricted": lambda: CarsGenerator(root, classes=[5, 9], mean=None, std=None),
        "flowers": lambda: FlowersGenerator(root, mean=None, std=None),
    }


@pytest.mark.parametrize("name", ["nab", "nab_restricted", "subdir", "subdir_restricted", "cars", "cars_restricted", "flowers"])
def test_file_lists_labels_and_statistics_equal_the_reference(name, golden, tree):
    g = _makers(tree)[name]()
    rel = lambda files: [os.path.relpath(f, tree) for f in files]
    assert rel(g.train_img_files) == golden[name + "_train_files"].tolist()
    assert rel(g.test_img_files) == golden[name + "_test_files"].tolist()
    assert list(g.labels_train) == golden[name + "_train_labels"].tolist()
    assert list(g.labels_test) == golden[name + "_test_labels"].tolist()
    assert list(g.classes) == golden[name + "_classes"].tolist()
    assert [g.num_classes, g.num_train, g.num_test] == golden[name + "_counts"].tolist()
    assert g.num_channels == 3
    assert g.mean.dtype == np.float32 and np.array_equal(g.mean, golden[name + "_mean"])       # float64 sums in file order: bit-equal
    assert g.std.dtype == np.float32 and np.array_equal(g.std, golden[name + "_std"])


def test_constructing_a_generator_decodes_nothing(tree, monkeypatch):
    from datasets import NABGenerator, get_data_generator
    opened = []
    real_open = PIL.Image.open
    monkeypatch.setattr(PIL.Image, "open", lambda *a, **k: (opened.append(a[0]), real_open(*a, **k))[1])
    g = NABGenerator(tree, mean=None, std=None)
    g2 = get_data_generator("cub", tree)
    assert len(g.labels_test) == 3 and len(g2.labels_train) == 7 and g.num_classes == 4
    g2.test_sequence(2)
    assert opened == [] and g._stores == {} and g2._stores == {}
    g.mean                                           # the statistics need the training images: now they are decoded
    assert len(opened) == 2 * 7 and set(g._stores) == {True}


def test_store_budget_is_enforced(tree):
    import sehip
    from datasets import NABGenerator
    g = NABGenerator(tree, mean=None, std=None, store_budget_bytes=1000)
    total = sum(w * h * 3 for (w, h), t in zip([(37, 53), (64, 48), (90, 20), (23, 71), (50, 50), (11, 17), (24, 9), (80, 33), (29, 90), (45, 31)],
                                              [0, 0, 0, 0, 1, 0, 0, 1, 1, 0]) if not t)
    with pytest.raises(sehip.SehipError, match=r"%d bytes.*1000 bytes" % total):
        g.mean


def test_unsupported_augmentations_raise(tree):
    from datasets import NABGenerator, FileDatasetGenerator
    with pytest.raises(NotImplementedError):
        NABGenerator(tree, distort_colors=True)
    with pytest.raises(NotImplementedError):
        FileDatasetGenerator(tree, randrot_max=10)


PRESETS = {     # name: (class, {attribute: value}) -- datasets/__init__.py:60-162 of the reference and the constructors' defaults
    "nab": ("NABGenerator", dict(cropsize=(224, 224), default_target_size=256, randzoom_range=(256, 480), color_mode="rgb", train_repeats=1,
                                 _mean=[125.30513277, 129.66606421, 118.45121113], _std=[57.0045467, 56.70059436, 68.44430446])),
    "nab-large": ("NABGenerator", dict(cropsize=(448, 448), default_target_size=512, randzoom_range=None)),
    "NAB-ilsvrcmean": ("NABGenerator", dict(randzoom_range=(256, 480), _mean=[122.65435242, 116.6545058, 103.99789959],
                                            _std=[71.40583196, 69.56888997, 73.0440314])),
    "nab-large-caffe": ("NABGenerator", dict(cropsize=(448, 448), default_target_size=512, randzoom_range=None, color_mode="bgr",
                                             _mean=[123.68, 116.779, 103.939], _std=[1., 1., 1.])),
    "cub": ("NABGenerator", dict(cropsize=(448, 448), default_target_size=512, randzoom_range=None, randerase_prob=0.5, train_repeats=1,
                                 _mean=[123.82988033, 127.35116805, 110.25606303], _std=[59.2230949, 58.0736071, 67.80251684])),
    "cub-caffe": ("NABGenerator", dict(cropsize=(448, 448), color_mode="bgr", _mean=[123.68, 116.779, 103.939], _std=[1., 1., 1.])),
    "cub-sub5": ("NABGenerator", dict(cropsize=(448, 448), default_target_size=512, train_repeats=6,
                                      _mean=[123.82988033, 127.35116805, 110.25606303])),
    "cars": ("CarsGenerator", dict(cropsize=(448, 448), default_target_size=512, randzoom_range=None,
                                   _mean=[120.03730636, 117.33780928, 116.0130335], _std=[75.40415763, 75.15394251, 77.28286728])),
    "cars-ilsvrcmean": ("CarsGenerator", dict(_mean=[122.65435242, 116.6545058, 103.99789959])),
    "flowers": ("FlowersGenerator", dict(cropsize=(448, 448), default_target_size=512,
                                         _mean=[110.7799141, 97.65648664, 75.32889973], _std=[74.90387818, 62.70218863, 69.7656359])),
    "mit67scenes": ("SubDirectoryGenerator", dict(cropsize=(224, 224), default_target_size=256, randzoom_range=None,
                                                  _mean=[124.62788179, 110.01028625, 94.95780545], _std=[68.56923599, 66.86607736, 67.35944349])),
    "UCMLU": ("SubDirectoryGenerator", dict(_mean=[122.65409223, 124.40230701, 114.25659171], _std=[55.74499679, 51.65585669, 50.16527551])),
    "resisc45": ("SubDirectoryGenerator", dict(_mean=[94.17769482, 97.40967803, 87.80359702], _std=[51.92246172, 47.22081475, 47.07685676])),
    "resisc45-caffe": ("SubDirectoryGenerator", dict(color_mode="bgr", _mean=[123.68, 116.779, 103.939], _std=[1., 1., 1.])),
}


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_get_data_generator_presets(name, golden, tree, tmp_path):
    import shutil
    import datasets
    root = tree
    if name.lower().startswith("cub-sub5"):
        root = str(tmp_path / "cub")
        shutil.copytree(tree, root)
        shutil.copy(os.path.join(root, "train_test_split.txt"), os.path.join(root, "train_test_split_5.txt"))
    elif name == "mit67scenes":
        root = str(tmp_path / "mit")
        shutil.copytree(tree, root)
        os.rename(os.path.join(root, "images"), os.path.join(root, "Images"))
        shutil.copy(os.path.join(root, "train.txt"), os.path.join(root, "TrainImages.txt"))
        shutil.copy(os.path.join(root, "test.txt"), os.path.join(root, "TestImages.txt"))
    elif PRESETS[name][0] == "SubDirectoryGenerator":        # img_dir '.': the class directories lie in the root
        root = os.path.join(tree, "images")
        for f in ("train.txt", "test.txt"):
            shutil.copy(os.path.join(tree, f), os.path.join(root, f))
    g = datasets.get_data_generator(name, root)
    cls, want = PRESETS[name]
    assert type(g).__name__ == cls and isinstance(g, datasets.FileDatasetGenerator)
    for attr, value in want.items():
        got = getattr(g, attr)
        if attr in ("_mean", "_std"):
            assert got.dtype == np.float32 and np.array_equal(got, np.asarray(value, dtype=np.float32)), attr
        else:
            assert got == value, attr
    assert g.num_train == 7 and g.num_test == 3
    assert g.randerase_params == {"sl": 0.02, "sh": 0.3, "r1": 0.3, "r2": 1. / 0.3}
    if name == "cub-sub5":
        assert len(g.train_sequence(2)) == 6 * 4 and len(g.test_sequence(2)) == 2


def test_get_data_generator_restricts_classes_and_rejects_what_is_out_of_scope(tree):
    from datasets import get_data_generator
    g = get_data_generator("cub", tree, classes=[9, 3])
    assert g.classes == [9, 3] and sorted(set(g.labels_train)) == [0, 1]
    for name in ("ilsvrc", "ilsvrc-caffe", "inat", "inat2018_aves", "inat2019-large"):
        with pytest.raises(NotImplementedError, match="resident"):
            get_data_generator(name, tree)
    with pytest.raises(ValueError):
        get_data_generator("no-such-dataset", tree)


# ---- resampling tables against live Pillow ----

@pytest.mark.parametrize("src,dst", [((37, 53), (24, 34)), ((10, 14), (32, 45)), ((150, 200), (24, 32)), ((1, 1), (7, 5)), ((33, 33), (20, 33))])
def test_resample_tables_equal_pillow_bilinear(src, dst):
    """Shapes are (h, w): down-scaling, up-scaling, 6x down-scaling, a 1 x 1 source, one axis unchanged."""
    import sehip
    rng = np.random.default_rng(src[0] * 1000 + dst[0])
    img = rng.integers(0, 256, size=src + (3,), dtype=np.uint8)
    img[:2, :3] = 255
    img[-2:, -3:] = 0
    want = np.asarray(PIL.Image.fromarray(img).resize((dst[1], dst[0]), PIL.Image.BILINEAR))
    xmap, xk, ymap, yk = sehip.resample_tables([src], [dst], dst)
    assert xmap.dtype == xk.dtype == ymap.dtype == yk.dtype == np.int32
    assert xmap.shape == (1, dst[1], 3) and ymap.shape == (1, dst[0], 3) and xk.shape[:2] == (1, dst[1]) and yk.shape[:2] == (1, dst[0])
    got = fp.apply_tables(img, xmap[0], xk[0], ymap[0], yk[0])
    assert np.array_equal(got, want)
    assert np.array_equal(xmap[0, :, 0], np.arange(dst[1])) and np.array_equal(ymap[0, :, 0], np.arange(dst[0]))
    if src[1] == dst[1]:
        assert xk.shape[2] == 1 and np.all(xk == 1 << 22) and np.array_equal(xmap[0, :, 1], np.arange(dst[1]))


def test_resample_tables_fold_crop_reflect_padding_and_flip():
    """A batch of three: crop window + flip, reflect padding on both axes wider than the image (several periods), a size-1 axis."""
    import sehip
    rng = np.random.default_rng(5)
    src = [(40, 30), (9, 7), (1, 6)]
    dst = [(25, 19), (5, 4), (1, 9)]
    crop = (12, 16)
    params = {"size": np.asarray(dst), "flip": np.asarray([True, True, False]), "erase": np.zeros((3, 4), dtype=int),
              "offset": np.asarray([(7, 2), (0, 0), (0, 0)]), "pad": np.asarray([(0, 0), (4, 9), (6, 3)])}
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in src]
    xmap, xk, ymap, yk = sehip.resample_tables(src, dst, crop, params["offset"], params["pad"], params["flip"])
    want, _ = fp.host_batch(images, params, crop, [0, 0, 0], [1, 1, 1], False)
    for b in range(3):
        got = fp.apply_tables(images[b], xmap[b], xk[b], ymap[b], yk[b])
        assert np.array_equal(got.astype(np.float32), want[b]), b
        assert xmap[b, :, 0].min() >= 0 and xmap[b, :, 0].max() < dst[b][1] and ymap[b, :, 0].max() < dst[b][0]


# ---- the host restatement against the reference's recorded batches ----

@pytest.mark.parametrize("name", sorted(fp.CONFIGS))
def test_host_restatement_equals_the_reference_batches(name, golden, tree):
    kw, train, augment = fp.CONFIGS[name]
    files = [os.path.join(tree, f) for f in golden["cfg_%s_files" % name].tolist()]
    params = fp.config_params(golden, name)
    ref = golden["cfg_%s_batch" % name]
    cw, ch = kw["cropsize"]
    got, mask = fp.host_batch([fp.decode(f) for f in files], params, (ch, cw), golden["cfg_%s_mean" % name], golden["cfg_%s_std" % name],
                              kw.get("color_mode") == "bgr")
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    keep = ~mask
    assert np.array_equal(got[keep], ref[keep])
    if augment:
        assert mask.any() and not np.array_equal(got[mask], ref[mask])          # the erased pixels hold the reference's noise
        assert params["flip"].any()
    else:
        assert not mask.any() and not params["flip"].any() and not params["erase"].any()
    if name == "d":
        assert params["pad"].any() and (params["pad"][:, 0] > 0).any() and (params["pad"][:, 1] > 0).any()
    if name in ("b", "c"):
        assert len(set(map(tuple, params["size"].tolist()))) > 3


# ---- draw_params ----

def _draws(tree, n, seed, **kw):
    from datasets import NABGenerator
    g = NABGenerator(tree, **kw)
    rng = np.random.default_rng(seed)
    sizes = np.stack((rng.integers(20, 90, size=n), rng.integers(20, 90, size=n)), axis=1)
    return g, sizes, g.draw_params(sizes, True, True, np.random.default_rng(seed + 1))


def _within_4_sigma(hits, n, p):
    return abs(hits - n * p) <= 4 * np.sqrt(n * p * (1 - p))


@pytest.mark.parametrize("zoom", [(28, 44), (0.6, 1.4), None])
def test_draw_params_ranges_and_probabilities(tree, zoom):
    n = 2000
    g, sizes, p = _draws(tree, n, 11, cropsize=(24, 20), default_target_size=32, randzoom_range=zoom, randerase_prob=0.3)
    H, W = p["size"][:, 0], p["size"][:, 1]
    short = np.minimum(H, W)
    tall = sizes[:, 1] < sizes[:, 0]
    if zoom is None:
        assert np.all(short == 32)
    elif isinstance(zoom[0], int):
        assert short.min() >= 28 and short.max() <= 43 and len(np.unique(short)) == 16        # randint's upper end is exclusive
    else:
        assert short.min() >= round(32 * 0.6) and short.max() <= round(32 * 1.4) and len(np.unique(short)) > 20
    assert np.all(np.where(tall, W, H) == short)                                               # the shorter side stays the shorter side
    want_other = [round(int(h) * (int(s) / int(w))) if w < h else round(int(w) * (int(s) / int(h))) for (h, w), s in zip(sizes, short)]
    assert np.where(tall, H, W).tolist() == want_other                                         # Python's round(), like the reference
    assert _within_4_sigma(int(p["flip"].sum()), n, 0.5)
    ye, xe, he, we = p["erase"].T
    erased = he > 0
    assert np.all(ye >= 0) and np.all(xe >= 0) and np.all(ye + he <= H) and np.all(xe + we <= W) and np.all(he < H) and np.all(we < W)
    area = (he * we)[erased] / (H * W)[erased]
    assert area.max() <= 0.3 and area.min() >= 0.0
    for axis, c in ((0, 20), (1, 24)):
        D = p["size"][:, axis]
        assert np.all(p["offset"][:, axis] >= 0) and np.all(p["offset"][:, axis] <= np.maximum(D - c, 0))
        assert np.all(p["pad"][:, axis] >= 0) and np.all(p["pad"][:, axis] <= np.maximum(c - D, 0))
    assert p["seed"].dtype == np.uint32 and len(np.unique(p["seed"])) > n - 5


def test_draw_params_erase_probability(tree):
    """Its own draw so that the count is exact: a rectangle was drawn for a sample iff its (h, w) is not (0, 0) -- an area of 2 % of
    at least 20 x 20 pixels at aspect 0.3 .. 3.3 never truncates to zero."""
    n = 2000
    for prob in (0.5, 0.25):
        _, _, p = _draws(tree, n, 23, cropsize=(24, 24), default_target_size=-1, randerase_prob=prob)
        assert _within_4_sigma(int((p["erase"][:, 2] > 0).sum()), n, prob)
    _, _, p = _draws(tree, n, 23, cropsize=(24, 24), default_target_size=-1, randerase_prob=0.0)
    assert not p["erase"].any()


def test_draw_params_test_mode_is_deterministic(tree):
    from datasets import NABGenerator
    g = NABGenerator(tree, cropsize=(24, 20), default_target_size=32, randzoom_range=(28, 44), randerase_prob=0.5)
    sizes = np.asarray([(53, 37), (20, 90), (90, 29), (50, 50)])
    p = g.draw_params(sizes, False, False, np.random.default_rng(0))
    assert p["size"].tolist() == [[round(53 * (32 / 37)), 32], [32, round(90 * (32 / 20))], [round(90 * (32 / 29)), 32], [32, 32]]
    assert not p["flip"].any() and not p["erase"].any() and not p["pad"].any()
    assert np.array_equal(p["offset"], np.stack(((p["size"][:, 0] - 20) // 2, (p["size"][:, 1] - 24) // 2), axis=1))
    q = NABGenerator(tree, cropsize=(40, 36), default_target_size=-1).draw_params(sizes[:2], False, False, np.random.default_rng(0))
    assert q["size"].tolist() == sizes[:2].tolist() and q["pad"].tolist() == [[0, 1], [8, 0]] and q["offset"].tolist() == [[8, 0], [0, 25]]


# ---- sub-epochs ----

class _Echo(object):
    def compose_batch(self, indices, train=True, augment=False, **kw):
        return torch.from_numpy(np.asarray(indices, dtype=np.int64))


def test_sequence_repeats():
    from datasets import DeviceBatchSequence
    labels = np.arange(10) % 3
    one = DeviceBatchSequence(_Echo(), np.arange(10), labels, batch_size=4, shuffle=True, seed=3)
    three = DeviceBatchSequence(_Echo(), np.arange(10), labels, batch_size=4, shuffle=True, seed=3, repeats=3)
    assert len(one) == 3 and len(three) == 9
    epochs = [torch.cat([three[i][0] for i in range(s * 3, s * 3 + 3)]).tolist() for s in range(3)]
    assert all(sorted(e) == list(range(10)) for e in epochs)
    assert len({tuple(e) for e in epochs}) == 3                                 # three distinct permutations
    for X, y in three:
        assert torch.equal(y, torch.from_numpy(labels[X.numpy()]))
    # repeats = 1 is today's sequence: the same permutations from the same seed, epoch after epoch
    got = [torch.cat([X for X, _ in one]).tolist() for _ in range(2)]
    want_rng, perm = np.random.default_rng(3), np.arange(10)
    want = []
    for _ in range(2):
        want_rng.shuffle(perm)
        want.append(perm.tolist())
    assert got == want
    plain = DeviceBatchSequence(_Echo(), np.arange(10), labels, batch_size=4)
    assert torch.cat([plain[i][0] for i in range(len(plain))]).tolist() == list(range(10)) and plain[2][0].tolist() == [8, 9]


def test_image_batch_validates_its_arguments_without_a_gpu():
    """The host-side checks of se_image_batch run before any launch."""
    import ctypes
    import sehip
    lib = sehip.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    ptrs = lambda p: [p, 64] + [p] * 10
    assert lib.se_image_batch(*ptrs(z), 0, z, 0, 2, 8, 8, 3, 3, z) == -1 and b"null pointer" in lib.se_last_error()
    assert lib.se_image_batch(*ptrs(z), 0, z, 0, 0, 8, 8, 3, 3, z) == 0                          # an empty batch is accepted
    assert lib.se_image_batch(*ptrs(one), 0, one, 7, 2, 8, 8, 3, 3, z) == -1 and b"dtype" in lib.se_last_error()
    assert lib.se_image_batch(*ptrs(one), 0, one, 0, 2, 8, 0, 3, 3, z) == -1 and b"bad shape" in lib.se_last_error()
    assert lib.se_image_batch(*ptrs(one), 0, one, 0, 2, 8, 448, 64, 3, z) == -3 and b"LDS" in lib.se_last_error()   # 448 x 64 weights: 112 KB
    assert lib.se_image_batch(*ptrs(one), 0, one, 0, 70000, 8, 8, 3, 3, z) == -3
    with pytest.raises(sehip.SehipError):
        sehip.image_batch(*[torch.zeros(4, dtype=torch.uint8)] * 11)                             # host tensors: no CPU fallback
