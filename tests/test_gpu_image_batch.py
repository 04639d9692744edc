"""GPU: se_image_batch (csrc/image_batch.hip) against the batches the reference's generators composed (tests/golden/file_pipeline.npz)
and against the host restatement of the reference's pipeline (tests/_file_pipeline.py, itself held against those batches by
tests/test_file_datasets_host.py), and the file-based generators end to end.

Bit-identity outside the erased rectangles is derivable, not measured: the resampling is integer arithmetic on both sides and the
normalisation one correctly rounded float32 subtraction and one division of the same operands."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

import _file_pipeline as fp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return fp.load_fixture()


@pytest.fixture(scope="module")
def tree(golden, tmp_path_factory):
    return fp.write_tree(golden, tmp_path_factory.mktemp("file_pipeline"))


def _compose(images, params, crop, mean, std, bgr, seeds, dtype=torch.float32):
    """One se_image_batch launch through the binding: images -> arena, parameters -> tables."""
    from datasets.files import compose_on_device
    sizes = np.asarray([im.shape[:2] for im in images], dtype=np.int32)
    nbytes = np.asarray([im.size for im in images], dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(nbytes)[:-1]))
    arena = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).cuda()
    stats = tuple(torch.tensor(np.asarray(v, dtype=np.float32)).cuda() for v in (mean, std))
    X = compose_on_device(arena, offsets, sizes, dict(params, seed=np.asarray(seeds, dtype=np.uint32)), crop, stats, bgr, dtype)
    torch.cuda.synchronize()
    assert X.shape == (len(images), 3) + tuple(crop) and X.dtype == dtype and X.is_contiguous(memory_format=torch.channels_last)
    return X.permute(0, 2, 3, 1)          # [B, ch, cw, 3], the physical layout


def _check_noise(got, mask, mean, std, bgr):
    """Inside the erase rectangles: every value in [(0 - mean) / std, (255 - mean) / std) of its channel POSITION (RGB-ordered
    statistics even in BGR mode), more than 8 distinct values in a rectangle of 16 or more pixels."""
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    for b in range(len(got)):
        if not mask[b].any():
            continue
        v = got[b][mask[b]].astype(np.float64)              # [pixels, 3]
        assert np.all(v >= (0 - mean) / std - 1e-6) and np.all(v < (255 - mean) / std), b
        if mask[b].sum() >= 16:
            assert len(np.unique(v)) > 8, b


@pytest.mark.parametrize("name", sorted(fp.CONFIGS))
def test_image_batch_equals_the_reference_batches(name, golden, tree):
    kw, train, augment = fp.CONFIGS[name]
    images = [fp.decode(os.path.join(tree, f)) for f in golden["cfg_%s_files" % name].tolist()]
    params = fp.config_params(golden, name)
    ref = golden["cfg_%s_batch" % name]
    mean, std, bgr = golden["cfg_%s_mean" % name], golden["cfg_%s_std" % name], kw.get("color_mode") == "bgr"
    crop = (kw["cropsize"][1], kw["cropsize"][0])
    _, mask = fp.host_batch(images, params, crop, mean, std, bgr)
    seeds = np.arange(len(images)) * 7919 + 17
    got_t = _compose(images, params, crop, mean, std, bgr, seeds)
    got = got_t.cpu().numpy()
    keep = ~mask
    diff = got[keep].view(np.uint32) != ref[keep].view(np.uint32)
    print("config %s: %d of %d values outside the erased rectangles differ in their bits" % (name, int(diff.sum()), diff.size))
    assert not diff.any()
    _check_noise(got, mask, mean, std, bgr)
    # the same seeds give the same noise, other seeds other noise
    again = _compose(images, params, crop, mean, std, bgr, seeds).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    if mask.any():
        other = _compose(images, params, crop, mean, std, bgr, seeds + 1).cpu().numpy()
        assert np.array_equal(other[keep].view(np.uint32), got[keep].view(np.uint32))
        for b in np.nonzero(mask.reshape(len(mask), -1).sum(axis=1) >= 4)[0]:
            assert not np.array_equal(other[b][mask[b]], got[b][mask[b]]), b
    # bf16: the float32 value rounded to nearest even
    half = _compose(images, params, crop, mean, std, bgr, seeds, torch.bfloat16)
    expected = torch.from_numpy(np.where(mask[..., None], got, ref)).cuda()
    assert torch.equal(half.contiguous().view(torch.int16), expected.to(torch.bfloat16).view(torch.int16))


def test_image_batch_mixed_batch_in_one_launch():
    """B = 5 in one launch: 6x down-scaling with a crop window and a flip, up-scaling, reflect padding on both axes (several periods
    on one), an erase rectangle cut by the crop edge, a 1-pixel-high source; crop 24 x 28 is more than one band of rows and no
    multiple of the band."""
    rng = np.random.default_rng(77)
    src = [(150, 204), (10, 14), (9, 7), (60, 70), (1, 33)]                      # (h, w)
    dst = [(25, 34), (32, 45), (9, 7), (40, 47), (1, 33)]
    images = []
    for h, w in src:
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = 128 + 90 * np.sin(xx / 5.0 + h)[..., None] * np.cos(yy[..., None] / 7.0 + np.arange(3))
        images.append(np.clip(smooth + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8))
    crop = (24, 28)
    params = {"size": np.asarray(dst), "flip": np.asarray([True, False, True, True, False]),
              "erase": np.asarray([(0, 0, 0, 0), (10, 20, 11, 13), (2, 1, 4, 3), (30, 35, 9, 11), (0, 0, 0, 0)]),
              "offset": np.asarray([(1, 5), (6, 15), (0, 0), (13, 17), (0, 3)]),
              "pad": np.asarray([(0, 0), (0, 0), (8, 14), (0, 0), (11, 0)])}
    mean, std = [125.3, 129.7, 118.5], [57.0, 56.7, 68.4]
    want, mask = fp.host_batch(images, params, crop, mean, std, False)
    assert mask[3].any() and not mask[3].all() and mask[3][-1, -1] and mask[1].sum() == 11 * 13       # rectangle 3 is cut by the crop edge
    got = _compose(images, params, crop, mean, std, False, [1, 2, 3, 4, 5]).cpu().numpy()
    keep = ~mask
    diff = got[keep].view(np.uint32) != want[keep].view(np.uint32)
    print("mixed batch: %d of %d values differ in their bits" % (int(diff.sum()), diff.size))
    assert not diff.any()
    _check_noise(got, mask, mean, std, False)
    # the reflected copies of an erase rectangle carry the reflected noise: sample 2's padding mirrors its image, noise included
    img2 = got[2][8:17, 14:21]
    assert np.array_equal(got[2][7], got[2][9]) and np.array_equal(got[2][:, 13], got[2][:, 15]) and img2.shape == (9, 7, 3)


def test_image_batch_wide_crop_and_many_taps():
    """Crop 448 wide from sources of 1000 and more columns (taps reach 15 and more) and a batch whose samples need different tap
    counts: the column table and a band's source rows share the workgroup's LDS, and the band is split where they do not fit."""
    rng = np.random.default_rng(3)
    src = [(140, 1100), (130, 460), (700, 460)]
    dst = [(20, 150), (130, 460), (100, 460)]
    images = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in src]
    crop = (20, 448)
    params = {"size": np.asarray(dst), "flip": np.asarray([False, True, False]), "erase": np.zeros((3, 4), dtype=int),
              "offset": np.asarray([(0, 0), (57, 9), (40, 3)]), "pad": np.asarray([(0, 149), (0, 0), (0, 0)])}
    want, mask = fp.host_batch(images, params, crop, [0, 0, 0], [1, 1, 1], True)
    got = _compose(images, params, crop, [0, 0, 0], [1, 1, 1], True, [0, 0, 0]).cpu().numpy()
    assert not mask.any() and np.array_equal(got, want)


def _write_nab_tree(root, n=12, classes=3):
    rng = np.random.default_rng(12)
    os.makedirs(os.path.join(root, "images", "all"))
    with open(os.path.join(root, "images.txt"), "w") as fi, open(os.path.join(root, "image_class_labels.txt"), "w") as fl, \
            open(os.path.join(root, "train_test_split.txt"), "w") as fs:
        for i in range(n):
            h, w = int(rng.integers(30, 80)), int(rng.integers(30, 80))
            PIL.Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, "images", "all", "%d.png" % i))
            fi.write("%d all/%d.png\n" % (i, i))
            fl.write("%d %d\n" % (i, 1 + i % classes))
            fs.write("%d %d\n" % (i, int(i % 3 != 2)))
    return root


def test_nab_generator_feeds_the_trainer(tmp_path):
    from datasets import NABGenerator
    from engine import Trainer
    root = _write_nab_tree(str(tmp_path))
    gen = NABGenerator(root, cropsize=(32, 32), default_target_size=36, randzoom_range=(34, 48))
    assert gen.num_train == 8 and gen.num_test == 4 and gen.num_classes == 3 and gen._stores == {}
    seq = gen.train_sequence(4)
    assert len(seq) == 2
    X, y = seq[0]
    assert X.shape == (4, 3, 32, 32) and X.dtype == torch.float32 and X.is_cuda and X.stride() == (3 * 32 * 32, 1, 3 * 32, 3)
    assert y.shape == (4,) and y.dtype == torch.int64 and y.is_cuda and torch.isfinite(X).all()
    assert set(gen._stores) == {True}                                  # only the training split was decoded
    X2, _ = seq[0]
    assert not torch.equal(X, X2)                                      # fresh augmentation draws for every batch
    Xt, yt = gen.test_sequence(4)[0]
    assert Xt.shape == (4, 3, 32, 32) and torch.equal(Xt, gen.test_sequence(4)[0][0])          # test mode is deterministic
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 3, 3, padding=1),
                                torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten()).cuda().to(memory_format=torch.channels_last)
    tr = Trainer(model, {"out": (lambda yt, yp: torch.nn.functional.cross_entropy(yp.float(), yt, reduction="none"), 1.0)}, {}, lr=0.01)
    history = tr.fit(seq, epochs=1, verbose=False)                     # two steps
    assert tr.iterations == 2 and np.isfinite(history[0]["loss"])


def test_get_data_generator_cub_returns_batches(tmp_path):
    from datasets import get_data_generator
    gen = get_data_generator("cub", _write_nab_tree(str(tmp_path)))
    X, y = gen.train_sequence(3, shuffle=False)[0]
    assert X.shape == (3, 3, 448, 448) and X.is_cuda and X.is_contiguous(memory_format=torch.channels_last) and torch.isfinite(X).all()
    assert y.tolist() == [1 - 1, 2 - 1, 1 - 1]                         # images 0, 1, 3 of classes 1, 2, 1 -> indices 0, 1, 0
    Xt, _ = gen.test_sequence(2)[0]
    # test mode against the host restatement: shorter side 512 (up-scaling), centre crop of 448 x 448, CUB statistics
    st = gen._stores[False]
    imgs = [fp.decode(f) for f in gen.test_img_files[:2]]
    params = gen.draw_params(st.sizes[:2], False, False)
    want, _ = fp.host_batch(imgs, params, (448, 448), gen.mean, gen.std, False)
    assert np.array_equal(Xt.permute(0, 2, 3, 1).cpu().numpy(), want)
