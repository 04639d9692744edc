"""GPU: se_tiny_batch (csrc/tiny_batch.hip) through the C ABI and its binding, bit for bit against the batches scipy.ndimage.
affine_transform composed (tests/golden/tiny_affine.npz) and against the host restatement datasets.common.affine_batch_host (itself
held against that fixture and live scipy by tests/test_tiny_affine_host.py), and the 'cifar-10' preset end to end.

Bit-identity is derivable, not measured: both sides run the same separately rounded float64 operations in the same order, round once to
float32, and standardise with one correctly rounded float32 subtraction and one division."""
import numpy as np
import pytest
import torch

import _tiny_affine as ta

pytestmark = pytest.mark.gpu

GUARD = 64                     # sentinel elements on either side of an output
SENTINEL = -768.0              # exact in bf16


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _launch(images, index, affine, flags, mean, stdp, mode, cval, dtype=torch.float32):
    """One se_tiny_batch launch into a sentinel-guarded buffer: -> the batch [B, H, W, C] on the host (bf16 as its uint16 patterns
    widened to float32); the guards must come back untouched."""
    import sehip
    images = np.asarray(images, dtype=np.float32)
    B, shape = len(index), (len(index),) + images.shape[1:]
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    out = buf[GUARD:GUARD + n].view(shape)
    got = sehip.tiny_batch(_dev(images), _dev(np.asarray(index, dtype=np.int64)), _dev(np.asarray(affine, dtype=np.float64).reshape(B, 6)),
                           _dev(np.asarray(flags, dtype=np.int32)), _dev(np.asarray(mean, dtype=np.float32)),
                           _dev(np.asarray(stdp, dtype=np.float32)), mode, cval, dtype=dtype, out=out)
    torch.cuda.synchronize()
    assert got is out
    guards = torch.cat((buf[:GUARD], buf[GUARD + n:])).float().cpu().numpy()
    assert (guards == SENTINEL).all()
    return out.float().cpu().numpy()


def _bf16(a):
    """float32 -> bf16 (round to nearest even) -> float32, by torch on the host."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


@pytest.mark.parametrize("mode", ta.MODES)
@pytest.mark.parametrize("name", ["s0", "s1", "s2", "s3", "s4"])
def test_tiny_batch_equals_the_scipy_batches(name, mode):
    stores, cval = ta.load_fixture()
    s = stores[name]
    got = _launch(s.images, s.index, s.matrices, s.flags, s.mean, s.stdp, mode, cval)
    diff = ta.bits(got) != ta.bits(s.expected[mode])
    print("%s %s: %d of %d values differ in their bits" % (name, mode, int(diff.sum()), diff.size))
    assert not diff.any()
    half = _launch(s.images, s.index, s.matrices, s.flags, s.mean, s.stdp, mode, cval, torch.bfloat16)
    assert np.array_equal(ta.bits(half), ta.bits(_bf16(s.expected[mode])))


@pytest.mark.parametrize("mode", ta.MODES)
@pytest.mark.parametrize("shape", [(4, 4, 1), (2, 2, 3)], ids=["4x4x1", "2x2x3"])
def test_more_than_one_trip_of_the_grid_stride_loop(shape, mode):
    """B * H * W above what the capped grid covers in one pass (SE_TINY_BATCH_MAX_BLOCKS workgroups of 256 threads, one element
    each), and no multiple of it: the result does not depend on which trip composed an element."""
    import sehip
    from datasets.common import affine_batch_host, affine_matrices
    h, w, c = shape
    B = sehip.TINY_BATCH_MAX_BLOCKS * 256 // (h * w) + 37
    assert B * h * w > sehip.TINY_BATCH_MAX_BLOCKS * 256
    rng = np.random.default_rng(h * 10 + c)
    images = (rng.random((13, h, w, c)) * 255).astype(np.float32)
    params = {"theta": rng.uniform(-30, 30, B), "tx": rng.uniform(-0.4, 0.4, B) * h, "ty": rng.uniform(-0.4, 0.4, B) * w,
              "shear": rng.uniform(-20, 20, B), "zx": rng.uniform(0.75, 1.25, B), "zy": rng.uniform(0.75, 1.25, B)}
    M = affine_matrices(params, h, w)
    index, flags = rng.integers(0, 13, B), rng.integers(0, 4, B)
    mean, stdp = images.mean(axis=(0, 1, 2)), images.std(axis=(0, 1, 2)) + np.float32(1e-6)
    want = affine_batch_host(images, index, M, flags, mean, stdp, mode, 7.5)
    got = _launch(images, index, M, flags, mean, stdp, mode, 7.5)
    assert np.array_equal(ta.bits(got), ta.bits(want))


def test_bad_indices_give_nan_samples_and_leave_their_neighbours():
    from datasets.common import affine_batch_host
    stores, cval = ta.load_fixture()
    for name in ("s1", "s3"):                                           # C = 1 and C = 4
        s = stores[name]
        n = len(s.images)
        index = s.index.copy()
        index[[0, 5, 6, 23]] = (-1, n, 2 ** 40, -2 ** 40)
        for dtype in (torch.float32, torch.bfloat16):
            got = _launch(s.images, index, s.matrices, s.flags, s.mean, s.stdp, "reflect", cval, dtype)
            want = affine_batch_host(s.images, index, s.matrices, s.flags, s.mean, s.stdp, "reflect", cval)
            bad = np.isin(np.arange(24), [0, 5, 6, 23])
            assert np.isnan(got[bad]).all() and np.isnan(want[bad]).all()
            assert np.array_equal(ta.bits(got[~bad]), ta.bits(want[~bad] if dtype == torch.float32 else _bf16(want[~bad])))


def test_wild_matrices_read_inside_the_store():
    """Huge, infinite and NaN maps: every tap stays inside its image (the neighbouring images of the store are NaN-free, the output of
    a finite map is finite), and the host restatement agrees wherever it is finite."""
    from datasets.common import affine_batch_host
    stores, cval = ta.load_fixture()
    s = stores["s1"]
    M = np.tile([1.0, 0, 0, 0, 1, 0], (6, 1))
    M[0, 2], M[1, 5], M[2, 0], M[3, 2], M[4, 4], M[5, 1] = 1e300, -1e300, 1e18, np.inf, np.nan, -3e9
    for mode in ta.MODES:
        got = _launch(s.images, [3] * 6, M, [0, 1, 2, 3, 0, 1], s.mean, s.stdp, mode, cval)
        with np.errstate(all="ignore"):
            want = affine_batch_host(s.images, [3] * 6, M, [0, 1, 2, 3, 0, 1], s.mean, s.stdp, mode, cval)
        ok = np.isfinite(want)
        assert ok[[0, 1, 2, 5]].all() and np.array_equal(np.isfinite(got), ok) and np.array_equal(ta.bits(got[ok]), ta.bits(want[ok])), mode


def test_empty_batch_and_refused_arguments():
    import ctypes
    import sehip
    stores, _ = ta.load_fixture()
    s = stores["s2"]
    images, mean, stdp = _dev(s.images), _dev(s.mean), _dev(s.stdp)
    empty = sehip.tiny_batch(images, torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros((0, 6), dtype=torch.float64, device="cuda"),
                             torch.zeros(0, dtype=torch.int32, device="cuda"), mean, stdp)
    assert tuple(empty.shape) == (0, 1, 9, 3) and empty.dtype == torch.float32
    idx, M, fl = _dev(np.zeros(2, np.int64)), _dev(np.tile([1.0, 0, 0, 0, 1, 0], (2, 1))), _dev(np.zeros(2, np.int32))
    nchw = sehip.tiny_batch(images, idx, M, fl, mean, stdp).permute(0, 3, 1, 2)
    assert nchw.shape == (2, 3, 1, 9) and nchw.is_contiguous(memory_format=torch.channels_last)
    for bad in (lambda: sehip.tiny_batch(images.double(), idx, M, fl, mean, stdp),
                lambda: sehip.tiny_batch(images.permute(0, 3, 1, 2), idx, M, fl, mean, stdp),
                lambda: sehip.tiny_batch(images, idx.int(), M, fl, mean, stdp),
                lambda: sehip.tiny_batch(images, idx, M.float(), fl, mean, stdp),
                lambda: sehip.tiny_batch(images, idx, M[:1], fl, mean, stdp),
                lambda: sehip.tiny_batch(images, idx, M, fl.long(), mean, stdp),
                lambda: sehip.tiny_batch(images, idx, M, fl[:1], mean, stdp),
                lambda: sehip.tiny_batch(images, idx, M, fl, mean[:2], stdp),
                lambda: sehip.tiny_batch(images, idx, M, fl, mean, stdp, fill_mode="wrap"),
                lambda: sehip.tiny_batch(images, idx, M, fl, mean, stdp, dtype=torch.float16),
                lambda: sehip.tiny_batch(images, idx, M, fl, mean, stdp, out=torch.empty((2, 3, 1, 9), device="cuda")),
                lambda: sehip.tiny_batch(torch.zeros((2, 3, 3, 5), device="cuda"), idx, M, fl, torch.zeros(5, device="cuda"), torch.ones(5, device="cuda")),
                lambda: sehip.tiny_batch(images.cpu(), idx, M, fl, mean, stdp)):
        with pytest.raises(sehip.SehipError):
            bad()
    # the C ABI itself, without a launch
    lib, z, one = sehip.lib(), ctypes.c_void_p(0), ctypes.c_void_p(256)
    f32, inval = sehip.DTYPE_F32, -1
    assert lib.se_tiny_batch(z, 0, z, z, z, z, z, 0, 0.0, z, f32, 0, 4, 4, 3, z) == 0                 # B = 0: every pointer may be NULL
    assert lib.se_tiny_batch(z, 4, one, one, one, one, one, 0, 0.0, one, f32, 2, 4, 4, 3, z) == inval and b"null pointer" in lib.se_last_error()
    for args in ((one, 4, one, one, one, one, one, 3, 0.0, one, f32, 2, 4, 4, 3, z),                    # fill mode
                 (one, 4, one, one, one, one, one, 0, 0.0, one, 7, 2, 4, 4, 3, z),                      # dtype
                 (one, 4, one, one, one, one, one, 0, 0.0, one, f32, -1, 4, 4, 3, z),                   # B
                 (one, -1, one, one, one, one, one, 0, 0.0, one, f32, 2, 4, 4, 3, z),                   # N
                 (one, 4, one, one, one, one, one, 0, 0.0, one, f32, 2, 0, 4, 3, z),                    # H
                 (one, 4, one, one, one, one, one, 0, 0.0, one, f32, 2, 4, 0, 3, z),                    # W
                 (one, 4, one, one, one, one, one, 0, 0.0, one, f32, 2, 4, 4, 0, z),                    # C
                 (one, 4, one, one, one, one, one, 0, 0.0, one, f32, 2, 4, 4, 5, z)):
        assert lib.se_tiny_batch(*args) == inval and b"se_tiny_batch" in lib.se_last_error(), args
    torch.cuda.synchronize()


# ---------------------------------------------------------------- end to end: the 'cifar-10' preset

def test_cifar10_preset_end_to_end(tmp_path):
    from datasets import get_data_generator
    from datasets.cifar import CifarGenerator
    from datasets.common import affine_batch_host, affine_matrices
    train = ta.write_cifar10(tmp_path).astype(np.float32)
    gen = get_data_generator("cifar-10", str(tmp_path))
    idx = np.array([5, 199, 0, 0, 73, 12, 11, 10, 150, 5], dtype=np.int64)
    x, p = gen.compose_batch(idx, train=True, augment=True, return_params=True, rng=np.random.default_rng(4))
    assert x.is_cuda and x.shape == (10, 3, 32, 32) and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    flags = p["hflip"].astype(np.int32) | (p["vflip"].astype(np.int32) << 1)
    want = affine_batch_host(train, idx, affine_matrices(p, 32, 32), flags, gen.mean.reshape(-1), gen.std.reshape(-1), "nearest", 0.0)
    assert np.array_equal(ta.bits(x.permute(0, 2, 3, 1).cpu().numpy()), ta.bits(want))
    assert (p["zx"] != 1).all() and (p["zx"] != p["zy"]).all() and p["hflip"].any() and not p["hflip"].all() and gen._dev_data is None
    # the same key draws the same batch; sequences bring their own generator
    again = gen.compose_batch(idx, train=True, augment=True, rng=np.random.default_rng(4))
    assert torch.equal(again, x)
    seq = gen.train_sequence(batch_size=16, shuffle=False, seed=3)
    X0, y0 = seq[0]
    assert X0.shape == (16, 3, 32, 32) and y0.tolist() == gen.labels_train[:16]
    assert torch.equal(gen.train_sequence(batch_size=16, shuffle=False, seed=3)[0][0], X0)
    # without augmentation: the existing path's batch (the same float32 subtraction and division on the host) within its 2e-6
    plain = CifarGenerator(str(tmp_path), None, reenumerate=True, cifar10=True)
    assert plain.affine is None
    for tr, n in ((True, 200), (False, 24)):
        a = gen.compose_batch(np.arange(n), train=tr, augment=False)
        b = plain.compose_batch(np.arange(n), train=tr, augment=False)
        assert a.shape == b.shape and float((a - b).abs().max()) < 2e-6
    Xt, yt = gen.test_sequence(batch_size=24)[0]
    assert float((Xt - plain.compose_batch(np.arange(24), train=False)).abs().max()) < 2e-6 and yt.tolist() == gen.labels_test


def test_cifar10_preset_zoom_is_measurable_on_ramps(tmp_path):
    """On linear-ramp images (R = row, G = column) bilinear interpolation is exact, so the slope of the augmented channel along its
    axis IS the zoom factor of that axis: it varies over 0.75 .. 1.25, per axis, and equals the drawn zx / zy."""
    from datasets import get_data_generator
    ta.write_cifar10(tmp_path, ramp=True)
    gen = get_data_generator("cifar-10", str(tmp_path))
    gen.mean, gen.std = np.zeros((1, 1, 1, 3), np.float32), np.ones((1, 1, 1, 3), np.float32)
    x, p = gen.compose_batch(np.arange(200), train=True, augment=True, return_params=True, rng=np.random.default_rng(8))
    x = x.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)
    inner = slice(12, 20)                                               # |shift| <= 4.8 and zoom <= 1.25 keep these rows / columns inside
    sy = np.diff(x[:, inner, 16, 0], axis=1).mean(axis=1)              # rows of R along the row axis
    sx = np.diff(x[:, 16, inner, 1], axis=1).mean(axis=1) * np.where(p["hflip"], -1, 1)
    assert np.abs(sy - p["zx"]).max() < 1e-4 and np.abs(sx - p["zy"]).max() < 1e-4
    for s in (sy, sx):
        assert 0.75 - 1e-4 <= s.min() < 0.8 and 1.2 < s.max() <= 1.25 + 1e-4
    assert abs(np.corrcoef(sy, sx)[0, 1]) < 0.3
    assert x.min() >= 0 and x[..., 0].max() <= 31                        # fill 'nearest': nothing extrapolated
