"""Shared by test_tiny_affine_host.py and test_gpu_tiny_batch.py: tests/golden/tiny_affine.npz (tools/make_tiny_affine_golden.py: what
scipy.ndimage.affine_transform, Keras' flips and the float32 standardisation give for given parameters) and synthetic CIFAR pickles."""
import collections
import os
import pickle

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("nearest", "constant", "reflect")
PARAM_KEYS = ("theta", "tx", "ty", "shear", "zx", "zy", "hflip", "vflip")

Store = collections.namedtuple("Store", "name images params matrices index flags mean stdp expected")

_fixture = None


def load_fixture():
    """-> (stores: {name: Store}, cval).  ``images`` float32 [N, H, W, C], ``params`` a dict of [B] arrays as draw_affine returns them,
    ``flags`` [B] int32 (bit 0 horizontal, bit 1 vertical flip), ``expected`` {fill mode: float32 [B, H, W, C]}.  Loaded once; read only."""
    global _fixture
    if _fixture is None:
        g = np.load(os.path.join(ROOT, "tests", "golden", "tiny_affine.npz"))
        stores = {}
        for name in g["stores"].tolist():
            p = g[name + "_params"]
            params = {k: (p[:, i] != 0) if k.endswith("flip") else p[:, i].copy() for i, k in enumerate(PARAM_KEYS)}
            flags = (params["hflip"].astype(np.int32) | (params["vflip"].astype(np.int32) << 1))
            near = g[name + "_nearest"]
            expected = {"nearest": near}
            for mode in MODES[1:]:
                expected[mode] = (near.view(np.uint32) ^ g["%s_%s_xor" % (name, mode)]).view(np.float32)
            stores[name] = Store(name, g[name + "_images"].astype(np.float32), params, g[name + "_matrices"], g[name + "_index"], flags,
                                 g[name + "_mean"], g[name + "_stdp"], expected)
            for a in (stores[name].images, near, *expected.values()):
                a.setflags(write=False)
        _fixture = (stores, float(g["cval"]))
    return _fixture


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def write_cifar10(root, n_per_batch=40, n_test=24, seed=5, ramp=False):
    """Synthetic CIFAR-10 pickles (data_batch_1 .. 5, test_batch) under ``root``; ``ramp``: every image is the linear ramp
    R = row, G = column, B = row + 2 column (bilinear interpolation of it is exact).  Returns the training images [N, 32, 32, 3] uint8."""
    rng = np.random.default_rng(seed)
    rr, cc = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    ramp_img = np.stack([rr, cc, rr + 2 * cc]).astype(np.uint8).reshape(-1)          # CIFAR's layout: [3, 32, 32] flattened
    train = []
    for i, n in [(i, n_per_batch) for i in range(1, 6)] + [(0, n_test)]:
        data = np.tile(ramp_img, (n, 1)) if ramp else rng.integers(0, 256, (n, 3072)).astype(np.uint8)
        with open(os.path.join(str(root), "data_batch_%d" % i if i else "test_batch"), "wb") as f:
            pickle.dump({b"data": data, b"labels": rng.integers(0, 10, n).tolist()}, f)
        if i:
            train.append(data)
    return np.concatenate(train).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
