#!/usr/bin/env python
"""Writes tests/golden/stream_datasets_meta.json: what the REFERENCE's ILSVRCGenerator and INatGenerator (datasets/ilsvrc.py,
datasets/inat.py, imported unmodified through oracle/ref_import.py) and its get_data_generator make of the trees of
tests/_stream_trees.py -- classes, file lists (relative to the root), labels, and the preset attributes of the dataset names.

Run once where the reference checkout is present (SE_REFERENCE_ROOT); the tests only read the JSON, which holds data only.  The
constructors open no image (the statistics are given), so the image files are written empty.

The Keras stand-in (oracle/keras_stub.py) has no ``list_pictures``.  Where the name is missing, this script sets the rule the
project implements on the reference's module -- every file below the directory, at any depth, whose lower-cased name ends in the
extension -- and records that in the file's ``list_pictures`` entry: the ILSVRC file ORDER is then the reference's own sorting of
that rule's result, not Keras' listing.  ``get_tuples_for_supercategory`` is plain Python and runs as it is."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from oracle import ref_import  # noqa: E402
import _stream_trees as trees  # noqa: E402

PRESET_ATTRIBUTES = ('cropsize', 'default_target_size', 'randzoom_range', 'randerase_prob', 'color_mode')
ILSVRC_NAMES = ('ilsvrc', 'ilsvrc-caffe', 'ILSVRC-ilsvrcmean')
INAT_NAMES = ('inat', 'iNat_Aves', 'inat2018_aves-large', 'inat2019')


def meta(g, root):
    rel = lambda files: [os.path.relpath(f, root) for f in files]
    out = {'classes': list(g.classes), 'class_indices': {str(k): int(v) for k, v in g.class_indices.items()},
           'num_classes': int(g.num_classes), 'train_files': rel(g.train_img_files), 'test_files': rel(g.test_img_files),
           'train_labels': [int(l) for l in g.labels_train], 'test_labels': [int(l) for l in g.labels_test]}
    for a in PRESET_ATTRIBUTES:
        v = getattr(g, a)
        out[a] = list(v) if isinstance(v, tuple) else v
    out['mean'], out['std'] = [float(v) for v in g.mean.astype('float64')], [float(v) for v in g.std.astype('float64')]
    return out


def main():
    ds = ref_import.import_reference_datasets()
    ilsvrc = ds._submodules['datasets.ilsvrc']
    out = {'list_pictures': 'keras'}
    if getattr(ilsvrc, 'list_pictures', None) is None:
        ilsvrc.list_pictures = lambda directory, ext: [os.path.join(r, f) for r, _, fs in os.walk(directory) for f in fs
                                                       if f.lower().endswith('.' + ext)]
        out['list_pictures'] = ('the Keras stand-in has none: every file below the directory, at any depth, whose lower-cased name '
                                'ends in the extension; sorted by the reference')
    with tempfile.TemporaryDirectory() as root:
        trees.write_ilsvrc(root, images=False)
        out['ilsvrc'] = {name: meta(ds.get_data_generator(name, root), root) for name in ILSVRC_NAMES}
        out['ilsvrc']['restricted'] = meta(ds.get_data_generator('ilsvrc', root, classes=[trees.SYNSETS[2], trees.SYNSETS[0]]), root)
        trees.write_inat(root)
        out['inat'] = {}
        for name in INAT_NAMES:
            g = ds.get_data_generator(name, root)
            out['inat'][name] = dict(meta(g, root), train_tuples=[[int(l), os.path.relpath(f, root)] for l, f in g.train_tuples],
                                     test_tuples=[[int(l), os.path.relpath(f, root)] for l, f in g.test_tuples])
    path = os.path.join(ROOT, 'tests', 'golden', 'stream_datasets_meta.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
