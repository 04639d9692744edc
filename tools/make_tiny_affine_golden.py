"""Golden fixture of the in-memory datasets' affine augmentation: tests/golden/tiny_affine.npz.

CPU only: NumPy and SciPy.  It imports neither the reference nor the product: the expected batches are what Keras 2.2's
``ImageDataGenerator.random_transform`` + ``standardize`` [third party: keras_preprocessing 1.0.x] compute for GIVEN parameters,
restated from their documented steps --

    transform_matrix = R (.) S (.) Sh (.) Z         (apply_affine_transform: a non-identity factor joins the product, np.dot)
    M = transform_matrix_offset_center(transform_matrix, h, w)          o_x = h / 2 + 0.5, o_y = w / 2 + 0.5 (Keras 2.2)
    x[:, :, k] = scipy.ndimage.affine_transform(x[:, :, k], M[:2, :2], M[:2, 2], order=1, mode=fill_mode, cval=cval)   per channel
    flip_axis(x, columns) if horizontal flip; flip_axis(x, rows) if vertical flip
    x = (x - mean) / (std + 1e-6)                   float32

-- with SciPy itself doing the interpolation, so the fixture pins ``datasets.common.affine_batch_host`` and ``se_tiny_batch`` to
scipy.ndimage bit for bit.

Stores (raw float32 pixels, 11 images each): s0 32 x 32 x 3, s1 5 x 7 x 1, s2 1 x 9 x 3, s3 9 x 1 x 4 with integer values 0 .. 255
(kept as uint8) and s4 33 x 17 x 3 with non-integer values.  Per store 24 parameter sets (theta, tx, ty, shear, zx, zy, hflip, vflip):
identity; each factor alone (rotations including exactly 90 degrees, shifts including one larger than the image, shears, zooms 0.75
and 1.25 and an anisotropic one); each flip alone and both; everything combined; 7 random draws (rotation +-30 degrees, shifts +-30 %,
shear +-20 degrees, zoom 0.75 .. 1.25).  Stored per store: images, params [24, 8], matrices [24, 6] float64, index [24] (repeats and
descending runs), mean and stdp [C] float32, the expected float32 batch [24, H, W, C] for 'nearest', and for 'constant' / 'reflect' the
XOR of their bit patterns with the 'nearest' batch (zero wherever no tap leaves the image, which keeps the file small; tests/
_tiny_affine.py puts them back together).  ``cval`` = 7.5.

    python tools/make_tiny_affine_golden.py
"""
import os

import numpy as np
import scipy.ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tiny_affine.npz")

CVAL = 7.5
MODES = ("nearest", "constant", "reflect")
STORES = (("s0", 32, 32, 3), ("s1", 5, 7, 1), ("s2", 1, 9, 3), ("s3", 9, 1, 4), ("s4", 33, 17, 3))
N_IMAGES = 11
INDEX = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 9, 8, 3, 3, 3, 0, 7, 2, 10, 5, 1, 0], dtype=np.int64)


def parameter_sets(h, w, rng):
    """[24, 8] float64: theta, tx, ty, shear (degrees / rows / columns), zx, zy, hflip, vflip."""
    ident = [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    rows = [list(ident) for _ in range(17)]
    rows[1][0], rows[2][0], rows[3][0] = 17.3, -30.0, 90.0
    rows[4][1] = 0.115 * h
    rows[5][2] = -0.13 * w
    rows[6][1], rows[6][2] = 1.3 * h, -1.6 * w                 # larger than the image
    rows[7][3], rows[8][3] = 20.0, -12.5
    rows[9][4] = rows[9][5] = 0.75
    rows[10][4] = rows[10][5] = 1.25
    rows[11][4], rows[11][5] = 0.8, 1.2
    rows[12][6] = 1.0
    rows[13][7] = 1.0
    rows[14][6] = rows[14][7] = 1.0
    rows[15] = [11.0, 0.08 * h, -0.11 * w, 7.0, 0.9, 1.15, 1.0, 0.0]
    rows[16] = [-23.0, -0.2 * h, 0.05 * w, -15.0, 1.2, 0.8, 0.0, 1.0]
    for _ in range(7):
        rows.append([rng.uniform(-30, 30), rng.uniform(-0.3, 0.3) * h, rng.uniform(-0.3, 0.3) * w, rng.uniform(-20, 20),
                     rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), float(rng.random() < 0.5), float(rng.random() < 0.5)])
    return np.asarray(rows, dtype=np.float64)


def keras_matrix(theta, tx, ty, shear, zx, zy, h, w):
    """apply_affine_transform's matrix (Keras 2.2 / keras_preprocessing 1.0.x), 3 x 3 float64."""
    transform_matrix = None
    if theta != 0:
        t = np.deg2rad(theta)
        transform_matrix = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    if tx != 0 or ty != 0:
        shift_matrix = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]])
        transform_matrix = shift_matrix if transform_matrix is None else np.dot(transform_matrix, shift_matrix)
    if shear != 0:
        s = np.deg2rad(shear)
        shear_matrix = np.array([[1, -np.sin(s), 0], [0, np.cos(s), 0], [0, 0, 1]])
        transform_matrix = shear_matrix if transform_matrix is None else np.dot(transform_matrix, shear_matrix)
    if zx != 1 or zy != 1:
        zoom_matrix = np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])
        transform_matrix = zoom_matrix if transform_matrix is None else np.dot(transform_matrix, zoom_matrix)
    if transform_matrix is None:
        return np.eye(3)
    o_x, o_y = float(h) / 2 + 0.5, float(w) / 2 + 0.5
    offset_matrix = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
    reset_matrix = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
    return np.dot(np.dot(offset_matrix, transform_matrix), reset_matrix)


def expected_batch(images, index, params, matrices, mean, stdp, mode):
    out = np.empty((len(index),) + images.shape[1:], dtype=np.float32)
    for b, (src, p, m) in enumerate(zip(index, params, matrices)):
        m = np.vstack([m.reshape(2, 3), [0, 0, 1]])
        x = np.stack([scipy.ndimage.affine_transform(images[src, :, :, k], m[:2, :2], m[:2, 2], order=1, mode=mode, cval=CVAL)
                      for k in range(images.shape[3])], axis=-1)
        assert x.dtype == np.float32
        if p[6]:
            x = x[:, ::-1]
        if p[7]:
            x = x[::-1]
        out[b] = (x - mean) / stdp
    return out


def main():
    rng = np.random.default_rng(20181)
    data = {"cval": np.float64(CVAL), "stores": np.array([s[0] for s in STORES])}
    for name, h, w, c in STORES:
        if name == "s4":
            images = (rng.random((N_IMAGES, h, w, c)) * 255).astype(np.float32)
            data[name + "_images"] = images
        else:
            data[name + "_images"] = rng.integers(0, 256, (N_IMAGES, h, w, c)).astype(np.uint8)
            images = data[name + "_images"].astype(np.float32)
        params = parameter_sets(h, w, rng)
        matrices = np.stack([keras_matrix(*p[:6], h, w)[:2].reshape(6) for p in params])
        mean = images.mean(axis=(0, 1, 2)).astype(np.float32)
        stdp = (images - mean).std(axis=(0, 1, 2)).astype(np.float32) + np.float32(1e-6)
        data.update({name + "_params": params, name + "_matrices": matrices, name + "_index": INDEX, name + "_mean": mean,
                     name + "_stdp": stdp})
        batches = {mode: expected_batch(images, INDEX, params, matrices, mean, stdp, mode) for mode in MODES}
        data[name + "_nearest"] = batches["nearest"]
        for mode in MODES[1:]:
            data["%s_%s_xor" % (name, mode)] = batches[mode].view(np.uint32) ^ batches["nearest"].view(np.uint32)
        print("%s %dx%dx%d: %d of %d values differ between nearest and constant, %d between nearest and reflect"
              % (name, h, w, c, np.count_nonzero(data[name + "_constant_xor"]), batches["nearest"].size,
                 np.count_nonzero(data[name + "_reflect_xor"])))
    np.savez_compressed(OUT, **data)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
