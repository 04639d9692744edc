"""Helpers of the file-dataset tests (no test in here): the fixture's dataset tree, a host restatement of the reference's batch
composition with GIVEN parameters (Pillow resize + NumPy normalise, flip, crop and pad -- the oracle of the GPU tests), and a NumPy
statement of what se_image_batch computes from its tables."""
import os

import numpy as np
import PIL.Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "file_pipeline.npz")
CONFIGS = {     # name: (constructor arguments, train split, augment) -- tools/make_file_pipeline_golden.py
    "a": (dict(cropsize=(24, 24), default_target_size=32, randerase_prob=0.5), False, False),
    "b": (dict(cropsize=(24, 24), default_target_size=32, randzoom_range=(28, 44), randerase_prob=0.5), True, True),
    "c": (dict(cropsize=(24, 24), default_target_size=32, randzoom_range=(0.6, 1.4), randerase_prob=0.5), True, True),
    "d": (dict(cropsize=(20, 12), default_target_size=-1, randerase_prob=0.5), True, True),
    "e": (dict(cropsize=(24, 24), default_target_size=32, randerase_prob=0.5, mean=[123.68, 116.779, 103.939], std=[1., 1., 1.],
               color_mode="bgr"), True, True),
}


def load_fixture():
    return np.load(GOLDEN)


def write_tree(g, root):
    """Write the fixture's dataset tree under ``root``."""
    offs, blob = g["tree_offsets"], g["tree_blob"]
    for i, name in enumerate(g["tree_names"].tolist()):
        path = os.path.join(str(root), name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(blob[offs[i]:offs[i + 1]].tobytes())
    return str(root)


def decode(path):
    with PIL.Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def config_params(g, name):
    return {k: g["cfg_%s_%s" % (name, k)] for k in ("size", "flip", "erase", "offset", "pad")}


def host_batch(images, params, crop, mean, std, bgr):
    """The reference's pipeline (datasets/common.py:380-581) for given parameters.  ``images``: uint8 [h, w, 3] arrays; ``crop`` =
    (ch, cw).  Returns the float32 batch [B, ch, cw, 3] (the erased rectangles keep the image's values) and a bool mask [B, ch, cw]
    of the pixels inside an erase rectangle."""
    ch, cw = crop
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    X, M = [], []
    for b, img in enumerate(images):
        H, W = (int(v) for v in params["size"][b])
        pil = PIL.Image.fromarray(img)
        if (W, H) != pil.size:
            pil = pil.resize((W, H), PIL.Image.BILINEAR)
        x = np.asarray(pil, dtype=np.float32).copy()
        x -= mean[None, None, :]
        x /= std[None, None, :]
        if bgr:
            x = x[:, :, ::-1]
        if params["flip"][b]:
            x = x[:, ::-1, :]
        m = np.zeros((H, W), dtype=bool)
        ye, xe, he, we = (int(v) for v in params["erase"][b])
        m[ye:ye + he, xe:xe + we] = he > 0
        (yo, xo), (yp, xp) = params["offset"][b], params["pad"][b]
        x, m = x[yo:yo + ch, xo:xo + cw], m[yo:yo + ch, xo:xo + cw]
        pads = ((yp, ch - x.shape[0] - yp), (xp, cw - x.shape[1] - xp))
        X.append(np.pad(x, pads + ((0, 0),), "reflect"))
        M.append(np.pad(m, pads, "reflect"))
    return np.stack(X), np.stack(M)


def apply_tables(img, xmap, xk, ymap, yk):
    """What se_image_batch computes before normalisation, for one image: uint8 [ch, cw, 3]."""
    ch, cw = len(ymap), len(xmap)
    src = img.astype(np.int64)
    t = np.zeros((img.shape[0], cw, 3), dtype=np.int64)
    for cx in range(cw):
        _, x0, n = xmap[cx]
        acc = (1 << 21) + (xk[cx, :n, None].astype(np.int64)[None] * src[:, x0:x0 + n, :]).sum(axis=1)
        t[:, cx] = np.clip(acc >> 22, 0, 255)
    out = np.zeros((ch, cw, 3), dtype=np.uint8)
    for cy in range(ch):
        _, y0, n = ymap[cy]
        acc = (1 << 21) + (yk[cy, :n, None, None].astype(np.int64) * t[y0:y0 + n]).sum(axis=0)
        out[cy] = np.clip(acc >> 22, 0, 255)
    return out
