"""CPU: the host side of the in-memory datasets' affine augmentation (datasets/common.py) -- the NumPy restatement of se_tiny_batch
against tests/golden/tiny_affine.npz (scipy.ndimage.affine_transform's batches) and against live scipy, Keras 2.2's matrices and
parameter distributions, the 'cifar-10' preset and the routing between the torch path and the kernel path."""
import numpy as np
import pytest
import torch

import _tiny_affine as ta


def _generator(kwargs, n=8, h=6, w=5, c=3):
    from datasets.common import InMemoryDatasetGenerator
    X = np.random.default_rng(0).integers(0, 256, (n, h, w, c)).astype(np.float32)
    return InMemoryDatasetGenerator(X, X[:2], [0] * n, [0, 0], train_generator_kwargs=kwargs)


# ---------------------------------------------------------------- the restatement is scipy's arithmetic

@pytest.mark.parametrize("mode", ta.MODES)
def test_host_restatement_equals_every_fixture_batch(mode):
    from datasets.common import affine_batch_host
    stores, cval = ta.load_fixture()
    assert sorted(stores) == ["s0", "s1", "s2", "s3", "s4"]
    for name, s in stores.items():
        got = affine_batch_host(s.images, s.index, s.matrices, s.flags, s.mean, s.stdp, mode, cval)
        diff = ta.bits(got) != ta.bits(s.expected[mode])
        print("%s %s: %d of %d values differ in their bits" % (name, mode, int(diff.sum()), diff.size))
        assert got.dtype == np.float32 and not diff.any(), (name, mode)


def test_fixture_covers_what_it_says():
    stores, cval = ta.load_fixture()
    assert cval == 7.5 and [stores[n].images.shape[1:] for n in sorted(stores)] == [(32, 32, 3), (5, 7, 1), (1, 9, 3), (9, 1, 4), (33, 17, 3)]
    for s in stores.values():
        h, w = s.images.shape[1:3]
        p = s.params
        assert len(s.index) == 24 and len(np.unique(s.index)) < 24 and (np.diff(s.index) < 0).sum() >= 3      # repeats, descending runs
        assert not any(np.any(p[k][0] != v) for k, v in zip(ta.PARAM_KEYS, (0, 0, 0, 0, 1, 1, 0, 0)))           # identity
        assert (p["theta"] == 90).any() and (np.abs(p["tx"]) > h).any() and (np.abs(p["ty"]) > w).any()
        assert (p["zx"] == 0.75).any() and (p["zx"] == 1.25).any() and (p["shear"] != 0).any()
        assert {(bool(a), bool(b)) for a, b in zip(p["hflip"], p["vflip"])} == {(False, False), (True, False), (False, True), (True, True)}
        for mode in ta.MODES[1:]:                                     # the fill modes are told apart
            assert (ta.bits(s.expected[mode]) != ta.bits(s.expected["nearest"])).any()
    assert (stores["s4"].images != np.round(stores["s4"].images)).any() and (stores["s0"].images == np.round(stores["s0"].images)).all()


def test_host_restatement_equals_live_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    from datasets.common import affine_batch_host, affine_matrices
    rng = np.random.default_rng(99)
    cval = -3.25
    for h, w in ((32, 32), (5, 7), (1, 9), (9, 1), (33, 17)):
        n = 12
        images = (rng.random((4, h, w, 2)) * 255).astype(np.float32)
        big = np.where(np.arange(n) % 4 == 0, 3.0, 0.3)                                     # every fourth: shifts of several image sizes
        params = {"theta": rng.uniform(-30, 30, n), "tx": rng.uniform(-1, 1, n) * big * h, "ty": rng.uniform(-1, 1, n) * big * w,
                  "shear": rng.uniform(-20, 20, n), "zx": rng.uniform(0.75, 1.25, n), "zy": rng.uniform(0.75, 1.25, n)}
        params["theta"][1] = 90.0
        M = affine_matrices(params, h, w)
        index = rng.integers(0, 4, n)
        mean, stdp = np.array([120.5, 131.25], np.float32), np.array([60.0, 71.5], np.float32)
        for mode in ta.MODES:
            want = np.empty((n, h, w, 2), np.float32)
            for b in range(n):
                for k in range(2):
                    t = ndimage.affine_transform(images[index[b], :, :, k], M[b].reshape(2, 3)[:, :2], M[b].reshape(2, 3)[:, 2], order=1,
                                                 mode=mode, cval=cval)
                    want[b, :, :, k] = (t - mean[k]) / stdp[k]
            got = affine_batch_host(images, index, M, np.zeros(n, np.int32), mean, stdp, mode, cval)
            assert np.array_equal(ta.bits(got), ta.bits(want)), (h, w, mode)


def test_host_restatement_flips_after_the_transform_and_marks_bad_indices():
    from datasets.common import affine_batch_host
    stores, cval = ta.load_fixture()
    s = stores["s1"]
    b = 15                                                              # everything combined
    args = (s.mean, s.stdp, "reflect", cval)
    plain = affine_batch_host(s.images, s.index[[b]], s.matrices[[b]], [0], *args)
    for flag, view in ((1, plain[:, :, ::-1]), (2, plain[:, ::-1]), (3, plain[:, ::-1, ::-1])):
        assert np.array_equal(ta.bits(affine_batch_host(s.images, s.index[[b]], s.matrices[[b]], [flag], *args)), ta.bits(view))
    out = affine_batch_host(s.images, [2, -1, len(s.images), 3], s.matrices[:4], [0] * 4, *args)
    assert np.isnan(out[1]).all() and np.isnan(out[2]).all() and np.isfinite(out[[0, 3]]).all()


# ---------------------------------------------------------------- matrices

def test_affine_matrices_equal_the_fixture_and_identity_is_exact():
    from datasets.common import affine_matrices
    stores, _ = ta.load_fixture()
    for s in stores.values():
        h, w = s.images.shape[1:3]
        M = affine_matrices(s.params, h, w)
        assert M.shape == (24, 6) and M.dtype == np.float64 and M.flags.c_contiguous
        assert np.abs(M - s.matrices).max() <= 1e-12
    ident = {"theta": np.zeros(3), "tx": np.zeros(3), "ty": np.zeros(3), "shear": np.zeros(3), "zx": np.ones(3), "zy": np.ones(3)}
    for h, w in ((32, 32), (5, 7), (33, 17)):
        assert np.array_equal(affine_matrices(ident, h, w), np.tile([1.0, 0, 0, 0, 1, 0], (3, 1)))
    # a pure shift is a pure offset, a pure zoom scales about (h / 2 + 0.5, w / 2 + 0.5): Keras 2.2's centre
    shift = dict(ident, tx=np.array([2.5, 0, 0]), ty=np.array([0, -1.25, 0]))
    assert np.array_equal(affine_matrices(shift, 8, 6), [[1, 0, 2.5, 0, 1, 0], [1, 0, 0, 0, 1, -1.25], [1, 0, 0, 0, 1, 0]])
    zoom = dict(ident, zx=np.array([0.5, 1, 1]), zy=np.array([1, 2.0, 1]))
    assert np.array_equal(affine_matrices(zoom, 8, 6), [[0.5, 0, 2.25, 0, 1, 0], [1, 0, 0, 0, 2, -3.5], [1, 0, 0, 0, 1, 0]])


# ---------------------------------------------------------------- distributions

def _uniform_ok(v, lo, hi):
    """n draws of U(lo, hi): inside the bounds, mean and variance within 4 standard errors."""
    n, a = len(v), hi - lo
    return (v.min() >= lo and v.max() <= hi and abs(v.mean() - (lo + hi) / 2) <= 4 * a / np.sqrt(12 * n)
            and abs(v.var() - a * a / 12) <= 4 * a * a * np.sqrt(1 / 180.0 / n))


def test_draw_affine_ranges_and_probabilities():
    n, h, w = 4000, 32, 24
    gen = _generator({"horizontal_flip": True, "vertical_flip": True, "width_shift_range": 0.15, "height_shift_range": 0.25,
                      "rotation_range": 30.0, "shear_range": 20.0, "zoom_range": 0.25})
    p = gen.draw_affine(n, h, w, np.random.default_rng([1, 0, 7]))
    assert sorted(p) == sorted(ta.PARAM_KEYS) and all(len(v) == n for v in p.values())
    assert _uniform_ok(p["theta"], -30, 30) and _uniform_ok(p["shear"], -20, 20)
    assert _uniform_ok(p["tx"], -0.25 * h, 0.25 * h) and _uniform_ok(p["ty"], -0.15 * w, 0.15 * w)      # rows by h, columns by w
    assert _uniform_ok(p["zx"], 0.75, 1.25) and _uniform_ok(p["zy"], 0.75, 1.25)
    assert abs(np.corrcoef(p["zx"], p["zy"])[0, 1]) <= 4 / np.sqrt(n)                                    # independent per axis
    for k in ("hflip", "vflip"):
        assert p[k].dtype == bool and abs(int(p[k].sum()) - n / 2) <= 4 * np.sqrt(n / 4)
    assert abs(int((p["hflip"] & p["vflip"]).sum()) - n / 4) <= 4 * np.sqrt(n * 3 / 16)
    # deterministic per key, different between keys
    again = gen.draw_affine(n, h, w, np.random.default_rng([1, 0, 7]))
    other = gen.draw_affine(n, h, w, np.random.default_rng([1, 1, 7]))
    assert all(np.array_equal(p[k], again[k]) for k in p) and not np.array_equal(p["theta"], other["theta"])


def test_draw_affine_draws_only_what_is_switched_on():
    gen = _generator({"zoom_range": (1.0, 1.0), "height_shift_range": 3.0, "fill_mode": "reflect"})
    p = gen.draw_affine(500, 32, 24, np.random.default_rng(3))
    assert not p["theta"].any() and not p["ty"].any() and not p["shear"].any() and not p["hflip"].any() and not p["vflip"].any()
    assert (p["zx"] == 1).all() and (p["zy"] == 1).all()
    assert _uniform_ok(p["tx"], -3.0, 3.0)                              # a range of 1 or more is in pixels
    gen = _generator({"zoom_range": (0.5, 0.75), "vertical_flip": True})
    p = gen.draw_affine(500, 32, 24, np.random.default_rng(3))
    assert _uniform_ok(p["zx"], 0.5, 0.75) and _uniform_ok(p["zy"], 0.5, 0.75) and p["vflip"].any() and not p["hflip"].any()


def test_sequences_key_their_draws_on_split_rank_and_seed():
    gen = _generator({"rotation_range": 10.0})
    draw = lambda seq: seq.compose_kwargs["rng"].uniform(size=4)
    a, b = draw(gen.train_sequence(4, seed=5, rank=1, world_size=2)), draw(gen.train_sequence(4, seed=5, rank=1, world_size=2))
    assert np.array_equal(a, b)
    for other in (gen.train_sequence(4, seed=5, rank=0, world_size=2), gen.train_sequence(4, seed=6, rank=1, world_size=2),
                  gen.test_sequence(4, seed=5, rank=1, world_size=2)):
        assert not np.array_equal(a, draw(other))
    plain = _generator({"horizontal_flip": True})
    assert plain.train_sequence(4).compose_kwargs == {}                 # the torch path takes no generator


# ---------------------------------------------------------------- preset, routing, refusals

def test_cifar10_preset_is_the_references_and_takes_the_affine_path(tmp_path):
    from datasets import get_data_generator
    import sehip
    ta.write_cifar10(tmp_path)
    gen = get_data_generator("cifar-10", str(tmp_path))
    assert gen.num_train == 200 and gen.num_test == 24 and gen.num_channels == 3
    assert gen.affine is not None
    given = {k: gen.affine[k] for k in ("horizontal_flip", "width_shift_range", "height_shift_range", "zoom_range")}
    assert given == {"horizontal_flip": True, "width_shift_range": 0.15, "height_shift_range": 0.15, "zoom_range": (0.75, 1.25)}
    assert (gen.affine["vertical_flip"], gen.affine["rotation_range"], gen.affine["shear_range"], gen.affine["fill_mode"]) == (False, 0, 0, "nearest")
    p = gen.draw_affine(2000, 32, 32, np.random.default_rng(0))
    assert p["zx"].min() < 0.8 and p["zx"].max() > 1.2 and np.abs(p["tx"]).max() <= 4.8 and p["hflip"].any() and not p["vflip"].any()
    seq = gen.train_sequence(batch_size=16)
    assert "rng" in seq.compose_kwargs
    if not torch.cuda.is_available():                                   # the affine path is the kernel: no CPU fallback
        gen.device = torch.device("cpu")
        with pytest.raises(sehip.SehipError):
            gen.compose_batch(np.arange(4), train=True, augment=True)
    assert gen._dev_data is None                                        # the torch path's standardised copy is never built


def test_cifar100_and_the_plain_configuration_keep_the_torch_path(tmp_path):
    import pickle
    from datasets import get_data_generator
    from datasets.common import InMemoryDatasetGenerator
    rng = np.random.default_rng(2)
    for name, n in (("train", 40), ("test", 8)):
        with open(str(tmp_path / name), "wb") as f:
            pickle.dump({b"data": rng.integers(0, 256, (n, 3072)).astype(np.uint8), b"fine_labels": rng.integers(0, 100, n).tolist()}, f)
    gen = get_data_generator("cifar-100", str(tmp_path))
    assert gen.affine is None and gen.shift_range == 0.15 and gen.horizontal_flip is True
    gen.device = torch.device("cpu")
    x, (row, col, flip) = gen.compose_batch(np.arange(40), train=True, augment=True, return_params=True)
    assert x.shape == (40, 3, 32, 32) and float(row.abs().max()) <= 4.8 + 1e-4 and not gen._raw
    X = rng.integers(0, 256, (8, 6, 5, 3)).astype(np.float32)
    for kwargs, shift, flip in (({"horizontal_flip": True, "width_shift_range": 0.15, "height_shift_range": 0.15}, 0.15, True),
                                ({"width_shift_range": 0.1, "height_shift_range": 0.1, "fill_mode": "nearest", "zoom_range": 0.0}, 0.1, False),
                                ({}, 0.0, False)):
        g = InMemoryDatasetGenerator(X, X[:2], [0] * 8, [0, 0], train_generator_kwargs=kwargs)
        assert g.affine is None and g.shift_range == shift and g.horizontal_flip is flip
        g.device = torch.device("cpu")
        assert g.compose_batch(np.arange(8), train=True, augment=True).shape == (8, 3, 6, 5)
    for kwargs in ({"width_shift_range": 0.15, "height_shift_range": 0.1}, {"width_shift_range": 2.0, "height_shift_range": 2.0},
                   {"vertical_flip": True}, {"rotation_range": 5.0}, {"shear_range": 5.0}, {"zoom_range": 0.1}, {"zoom_range": (0.9, 1.0)},
                   {"fill_mode": "constant"}, {"fill_mode": "reflect"}):
        assert InMemoryDatasetGenerator(X, X[:2], [0] * 8, [0, 0], train_generator_kwargs=kwargs).affine is not None, kwargs


@pytest.mark.parametrize("key, value", [("channel_shift_range", 0.1), ("brightness_range", (0.5, 1.5)), ("zca_whitening", True),
                                        ("preprocessing_function", None), ("featurewise_center", True), ("fill_mode", "wrap"),
                                        ("rotation_range", [0.0, 10.0]), ("rotation_range", 10), ("width_shift_range", 2),
                                        ("height_shift_range", [1.0, 2.0]), ("shear_range", -1.0), ("zoom_range", [0.9, 1.0, 1.1])])
def test_unknown_keys_and_unbuilt_values_are_refused_by_name(key, value):
    with pytest.raises(NotImplementedError, match=key):
        _generator({"horizontal_flip": True, key: value})
