"""ILSVRC 2012 (reference: datasets/ilsvrc.py): one directory of images per synset under ``ILSVRC2012_img_train`` and
``ILSVRC2012_img_val``.  Construction lists directories and opens no image.

About 1.28 million training images of roughly 0.5 MB decoded are several hundred GB, so the training split cannot be resident: build
the generator with ``store='auto'`` (what the dataset name ``ilsvrc-stream`` does) or ``store='stream'`` (datasets/files.py)."""
import os

from . import IMAGENET_MEAN, IMAGENET_STD
from .files import FileDatasetGenerator


def list_jpeg_files(directory):
    """Every file below ``directory``, at any depth, whose lower-cased name ends in '.jpeg' -- Keras' ``list_pictures(directory,
    'jpeg')`` as keras_preprocessing states it.  (Keras 2.0's older form matches names against the regular expression
    ``([\\w]+\\.(?:jpeg))`` and so also rejects names that do not start with word characters; ILSVRC has no such names, and that
    form is not reproduced.)  A directory that does not exist has no files."""
    return [os.path.join(root, f) for root, _, files in os.walk(directory) for f in files if f.lower().endswith('.jpeg')]


class ILSVRCGenerator(FileDatasetGenerator):
    """``classes``: the synsets to use, numbered in the given order; ``None`` takes the sub-directories of the training directory in
    lexicographical order.  The files of a class are sorted by path.  Like the reference's class, this one fixes the geometry
    (crops of 224 x 224 from a shorter side of 256, random zoom 256 .. 480, no random erasing) and takes no crop or target-size
    argument; ``store_kwargs`` are the store's (``store``, ``prefetch_batches``, ``decode_threads``, ``store_budget_bytes``,
    ``dtype``, ``seed``)."""

    def __init__(self, root_dir, classes=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, color_mode='rgb', **store_kwargs):
        super(ILSVRCGenerator, self).__init__(root_dir, cropsize=(224, 224), default_target_size=256, randzoom_range=(256, 480),
                                              randerase_prob=0.0, color_mode=color_mode, **store_kwargs)
        self.train_dir = os.path.join(root_dir, 'ILSVRC2012_img_train')
        self.test_dir = os.path.join(root_dir, 'ILSVRC2012_img_val')
        if classes is None:
            classes = [d for d in sorted(os.listdir(self.train_dir)) if os.path.isdir(os.path.join(self.train_dir, d))]
        self.classes = classes
        self.class_indices = dict(zip(self.classes, range(len(self.classes))))
        for lbl, synset in enumerate(self.classes):
            for top, files, labels in ((self.train_dir, self.train_img_files, self._train_labels),
                                       (self.test_dir, self.test_img_files, self._test_labels)):
                found = sorted(list_jpeg_files(os.path.join(top, synset)))
                files += found
                labels += [lbl] * len(found)
        self._compute_stats(mean, std)
