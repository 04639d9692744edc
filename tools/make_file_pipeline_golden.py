#!/usr/bin/env python
"""Writes tests/golden/file_pipeline.npz: what the REFERENCE's file-based generators (datasets/common.py, nab.py, subdirectory.py,
cars.py, flowers.py -- imported unmodified through oracle/ref_import.py) make of a tiny synthetic dataset tree.

Run once where the reference checkout is present (SE_REFERENCE_ROOT); the tests only read the npz.  The file holds data only:

* ``tree_names / tree_offsets / tree_blob``: every file of the dataset tree (10 PNG images, smooth content plus noise; the NAB /
  sub-directory / Cars / Flowers metadata files), so that a test can write the tree again;
* per generator class: file lists (relative to the root), labels, classes and -- with ``mean = std = None`` -- the statistics the
  reference computed, with and without a ``classes=[...]`` restriction;
* configurations (a)-(e): the batch the reference composed, and the parameters it drew for it.  The draws are recorded by wrapping
  ``np.random.randint / uniform / random`` during the run and read back in the order datasets/common.py:414-431,456-470,522-540
  makes them (zoom, flip, erase test, erase geometry, noise per image; then the crop offsets or pads of all images).

The reference's modules need three Keras names: ``load_img`` (PIL open + convert('RGB'), what Keras does for color_mode 'rgb'),
``img_to_array`` (float32 array, channels_last) and ``K.image_data_format`` -- set on the imported modules here.
"""
import io
import os
import sys
import tempfile

import numpy as np
import PIL.Image
import scipy.io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

SIZES = [(37, 53), (64, 48), (90, 20), (23, 71), (50, 50), (11, 17), (24, 9), (80, 33), (29, 90), (45, 31)]     # (w, h)
LABELS = [3, 5, 8, 9, 3, 5, 8, 9, 3, 5]               # NAB labels: integers with gaps
IS_TEST = [0, 0, 0, 0, 1, 0, 0, 1, 1, 0]
CAFFE_MEAN, CAFFE_STD = [123.68, 116.779, 103.939], [1., 1., 1.]
NAB_MEAN, NAB_STD = [125.30513277, 129.66606421, 118.45121113], [57.0045467, 56.70059436, 68.44430446]

CONFIGS = {     # constructor arguments of the reference's NABGenerator, sequence mode
    'a': (dict(cropsize=(24, 24), default_target_size=32, randerase_prob=0.5), False),
    'b': (dict(cropsize=(24, 24), default_target_size=32, randzoom_range=(28, 44), randerase_prob=0.5), True),
    'c': (dict(cropsize=(24, 24), default_target_size=32, randzoom_range=(0.6, 1.4), randerase_prob=0.5), True),
    'd': (dict(cropsize=(20, 12), default_target_size=-1, randerase_prob=0.5), True),
    'e': (dict(cropsize=(24, 24), default_target_size=32, randerase_prob=0.5, mean=CAFFE_MEAN, std=CAFFE_STD, color_mode='bgr'), True),
}


def png_bytes(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(xx / (3 + 2 * c) + rng.uniform(0, 6)) * np.cos(yy / (4 + c) + rng.uniform(0, 6)) for c in range(3)], axis=-1)
    img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    PIL.Image.fromarray(img).save(buf, format='PNG')
    return buf.getvalue()


def make_tree(root):
    rng = np.random.default_rng(2024)
    files = {}
    rel = ['c%02d/img%d.png' % (l, i) for i, l in enumerate(LABELS)]
    for i, (w, h) in enumerate(SIZES):
        data = png_bytes(rng, w, h)
        files['images/' + rel[i]] = data
        files['jpg/image_%05d.jpg' % (i + 1)] = data          # Flowers' fixed file names; Pillow goes by content
    files['images.txt'] = ''.join('%d %s\n' % (i + 1, r) for i, r in enumerate(rel)).encode()
    files['image_class_labels.txt'] = ''.join('%d %d\n' % (i + 1, l) for i, l in enumerate(LABELS)).encode()
    files['train_test_split.txt'] = ''.join('%d %d\n' % (i + 1, 1 - t) for i, t in enumerate(IS_TEST)).encode()
    files['train.txt'] = ''.join(r + '\n' for r, t in zip(rel, IS_TEST) if not t).encode()
    files['test.txt'] = ''.join(r + '\n' for r, t in zip(rel, IS_TEST) if t).encode()
    for name, data in files.items():
        path = os.path.join(root, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'wb') as f:
            f.write(data)
    ann = np.zeros(len(rel), dtype=[('relative_im_path', 'O'), ('class', 'i4'), ('test', 'i4')])
    for i, r in enumerate(rel):
        ann[i] = ('images/' + r, LABELS[i], IS_TEST[i])
    scipy.io.savemat(os.path.join(root, 'cars_annos.mat'), {'annotations': ann})
    scipy.io.savemat(os.path.join(root, 'imagelabels.mat'), {'labels': np.asarray(LABELS)})
    ids = np.arange(1, len(rel) + 1)
    scipy.io.savemat(os.path.join(root, 'setid.mat'), {'trnid': ids[:4], 'valid': ids[4:7], 'tstid': ids[7:]})
    for name in ('cars_annos.mat', 'imagelabels.mat', 'setid.mat'):
        with open(os.path.join(root, name), 'rb') as f:
            files[name] = f.read()
    return files


class Recorder(object):
    """Wraps np.random.randint / uniform / random and logs (name, result) of every call."""

    def __init__(self):
        self.log, self.saved = [], {}

    def __enter__(self):
        for name in ('randint', 'uniform', 'random'):
            fn = self.saved[name] = getattr(np.random, name)
            setattr(np.random, name, (lambda name, fn: lambda *a, **k: self._call(name, fn, a, k))(name, fn))
        return self

    def _call(self, name, fn, a, k):
        r = fn(*a, **k)
        self.log.append((name, r))
        return r

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(np.random, name, fn)


def read_params(log, sizes, kw, augment):
    """The parameters behind a recorded batch, from the draws in the order the reference makes them."""
    log = list(log)

    def pop(name):
        got, value = log.pop(0)
        assert got == name, (got, name)
        return value

    cw, ch = kw['cropsize']
    ts0, zr, prob = kw['default_target_size'], kw.get('randzoom_range'), kw['randerase_prob']
    sl, sh, r1, r2 = 0.02, 0.3, 0.3, 1. / 0.3
    out = {k: [] for k in ('size', 'flip', 'erase', 'offset', 'pad')}
    for w, h in sizes:
        ts, zoom = ts0, augment and zr is not None
        W, H = w, h
        if ts > 0 or zoom:
            if ts <= 0:
                ts = (w, h)
            if zoom:
                ts = np.round(np.array(ts) * pop('uniform')).astype(int).tolist() if isinstance(zr[0], float) else pop('randint')
            if isinstance(ts, int):
                ts = (ts, round(h * (ts / w))) if w < h else (round(w * (ts / h)), ts)
            W, H = ts
        out['size'].append((H, W))
        out['flip'].append(bool(augment and pop('random') < 0.5))
        rect = (0, 0, 0, 0)
        if augment and prob > 0 and pop('random') < prob:
            while True:
                se, re = pop('uniform') * (H * W), pop('uniform')
                he, we = int(np.sqrt(se * re)), int(np.sqrt(se / re))
                if he < H and we < W:
                    break
            xe, ye = pop('randint'), pop('randint')
            assert pop('uniform').shape == (he, we, 3)
            rect = (ye, xe, he, we)
        out['erase'].append(rect)
    for H, W in out['size']:
        offs, pad = [0, 0], [0, 0]
        for axis, (D, c) in enumerate(((H, ch), (W, cw))):
            if D > c:
                offs[axis] = pop('randint') if augment else (D - c) // 2
            elif D < c:
                pad[axis] = pop('randint') if augment else (c - D) // 2
        out['offset'].append(offs)
        out['pad'].append(pad)
    assert not log, log
    return {k: np.asarray(v) for k, v in out.items()}


def main():
    ds = ref_import.import_reference_datasets()
    common = ds._submodules['datasets.common']
    common.load_img = lambda fn: PIL.Image.open(fn).convert('RGB')
    common.img_to_array = lambda img, data_format=None: np.asarray(img, dtype=np.float32)
    common.K.image_data_format = lambda: 'channels_last'
    nab, sub = ds._submodules['datasets.nab'], ds._submodules['datasets.subdirectory']
    cars, flowers = ds._submodules['datasets.cars'], ds._submodules['datasets.flowers']
    out = {}
    with tempfile.TemporaryDirectory() as root:
        files = make_tree(root)
        names = sorted(files)
        out['tree_names'] = np.asarray(names)
        out['tree_offsets'] = np.cumsum([0] + [len(files[n]) for n in names]).astype(np.int64)
        out['tree_blob'] = np.frombuffer(b''.join(files[n] for n in names), dtype=np.uint8)
        rel = lambda fs: np.asarray([os.path.relpath(f, root) for f in fs])
        makers = {
            'nab': lambda **k: nab.NABGenerator(root, mean=None, std=None, **k),
            'nab_restricted': lambda **k: nab.NABGenerator(root, classes=[9, 3], mean=None, std=None, **k),
            'subdir': lambda **k: sub.SubDirectoryGenerator(root, img_dir='images', **k),
            'subdir_restricted': lambda **k: sub.SubDirectoryGenerator(root, classes=['c08', 'c05'], img_dir='images', **k),
            'cars': lambda **k: cars.CarsGenerator(root, mean=None, std=None, **k),
            'cars_restricted': lambda **k: cars.CarsGenerator(root, classes=[5, 9], mean=None, std=None, **k),
            'flowers': lambda **k: flowers.FlowersGenerator(root, mean=None, std=None, **k),
        }
        for name, make in makers.items():
            g = make()
            out[name + '_train_files'], out[name + '_test_files'] = rel(g.train_img_files), rel(g.test_img_files)
            out[name + '_train_labels'], out[name + '_test_labels'] = np.asarray(g.labels_train), np.asarray(g.labels_test)
            out[name + '_classes'] = np.asarray(g.classes)
            out[name + '_counts'] = np.asarray([g.num_classes, g.num_train, g.num_test])
            out[name + '_mean'], out[name + '_std'] = g.mean, g.std
        for name, (kw, augment) in CONFIGS.items():
            np.random.seed(100 + ord(name))
            g = nab.NABGenerator(root, **kw)
            train = name != 'a'
            seq = (g.train_sequence if train else g.test_sequence)(batch_size=16, shuffle=False, augment=augment)
            fl = g.train_img_files if train else g.test_img_files
            sizes = [PIL.Image.open(f).size for f in fl]
            with Recorder() as rec:
                X, y = seq[0]
            assert X.shape == (len(fl), kw['cropsize'][1], kw['cropsize'][0], 3) and X.dtype == np.float32
            out['cfg_%s_batch' % name] = X
            out['cfg_%s_files' % name] = rel(fl)
            out['cfg_%s_mean' % name], out['cfg_%s_std' % name] = g.mean, g.std
            for k, v in read_params(rec.log, sizes, kw, augment).items():
                out['cfg_%s_%s' % (name, k)] = v
    path = os.path.join(ROOT, 'tests', 'golden', 'file_pipeline.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
