"""Helpers of the streamed-dataset tests (no test in here): the layout of a three-synset ILSVRC tree and of iNaturalist JSON files,
and the functions that write them.  tools/make_stream_datasets_golden.py writes the same layouts for the reference's classes."""
import json
import os

import numpy as np
import PIL.Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_datasets_meta.json")
SYNSETS = ["n01440764", "n01443537", "n01484850"]
SIZES = [(37, 53), (64, 48), (90, 20), (23, 71), (50, 50), (11, 17), (24, 9), (80, 33), (29, 90), (45, 31)]     # (w, h), tests/_file_pipeline's
# training images in no particular order: (path below ILSVRC2012_img_train, Pillow mode); "_10" sorts before "_2", the nested
# directory "extra" before the synset's own files
ILSVRC_TRAIN = [("n01440764/n01440764_2.JPEG", "RGB"), ("n01440764/n01440764_10.JPEG", "L"), ("n01440764/n01440764_7.JPEG", "RGB"),
                ("n01440764/n01440764_31.JPEG", "RGB"), ("n01443537/n01443537_5.JPEG", "RGB"), ("n01443537/n01443537_1.JPEG", "RGB"),
                ("n01443537/extra/n01443537_9.JPEG", "RGB"), ("n01484850/n01484850_4.JPEG", "CMYK"),
                ("n01484850/n01484850_12.JPEG", "RGB"), ("n01484850/n01484850_3.JPEG", "RGB")]
ILSVRC_VAL = [("n01440764/ILSVRC2012_val_00000293.JPEG", "RGB"), ("n01440764/ILSVRC2012_val_00000017.JPEG", "RGB"),
              ("n01443537/ILSVRC2012_val_00000236.JPEG", "RGB")]                                 # n01484850: a directory without files
ILSVRC_OTHER = ["ILSVRC2012_img_train/n01440764/notes.txt", "ILSVRC2012_img_train/LOC_synset_mapping.txt"]     # no images, no synsets

# iNaturalist: category ids with gaps and out of order, two super-categories, annotations out of id order
INAT_CATEGORIES = [{"id": 7, "name": "Turdus merula", "supercategory": "Aves"}, {"id": 3, "name": "Quercus robur", "supercategory": "Plantae"},
                   {"id": 12, "name": "Parus major", "supercategory": "Aves"}]
INAT_TRAIN = [(105, 12, "train_val2018/Aves/12/e.jpg"), (101, 7, "train_val2018/Aves/7/a.jpg"), (104, 3, "train_val2018/Plantae/3/d.jpg"),
              (102, 3, "train_val2018/Plantae/3/b.jpg"), (106, 7, "train_val2018/Aves/7/f.jpg"), (103, 12, "train_val2018/Aves/12/c.jpg")]
INAT_VAL = [(203, 3, "train_val2018/Plantae/3/z.jpg"), (201, 12, "train_val2018/Aves/12/x.jpg"), (202, 7, "train_val2018/Aves/7/y.jpg")]
# 2019: numeric names, no 'supercategory' key
INAT19_CATEGORIES = [{"id": 40, "name": "40"}, {"id": 2, "name": "2"}]
INAT19_TRAIN = [(11, 40, "train_val2019/Birds/40/a.jpg"), (12, 2, "train_val2019/Plants/2/b.jpg"), (10, 40, "train_val2019/Birds/40/c.jpg")]
INAT19_VAL = [(21, 2, "train_val2019/Plants/2/v.jpg"), (20, 40, "train_val2019/Birds/40/w.jpg")]


def _jpeg(path, rng, size, mode):
    w, h = size
    channels = {"L": (), "RGB": (3,), "CMYK": (4,)}[mode]
    noise = rng.integers(0, 256, size=(h, w) + channels, dtype=np.uint8)
    PIL.Image.fromarray(noise, mode=mode).save(path, format="JPEG", quality=90)


def write_ilsvrc(root, images=True, seed=2012):
    """The ILSVRC tree under ``root``; ``images=False`` writes empty files of the same names (enough for the metadata)."""
    rng = np.random.default_rng(seed)
    sizes = SIZES + SIZES
    entries = [("ILSVRC2012_img_train", e) for e in ILSVRC_TRAIN] + [("ILSVRC2012_img_val", e) for e in ILSVRC_VAL]
    for k, (top, (rel, mode)) in enumerate(entries):
        path = os.path.join(str(root), top, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if images:
            _jpeg(path, rng, sizes[k], mode)
        else:
            open(path, "wb").close()
    os.makedirs(os.path.join(str(root), "ILSVRC2012_img_val", SYNSETS[2]), exist_ok=True)
    for rel in ILSVRC_OTHER:
        with open(os.path.join(str(root), rel), "w") as f:
            f.write("not an image\n")
    return str(root)


def write_inat(root):
    """The four JSON files under ``root`` (no images: nothing here opens one)."""
    def dump(name, categories, rows):
        data = {"images": [{"id": i, "file_name": fn} for i, _, fn in sorted(rows)], "categories": categories,
                "annotations": [{"id": 1000 + k, "image_id": i, "category_id": c} for k, (i, c, _) in enumerate(rows)]}
        with open(os.path.join(str(root), name), "w") as f:
            json.dump(data, f)
    os.makedirs(str(root), exist_ok=True)
    dump("train2018.json", INAT_CATEGORIES, INAT_TRAIN)
    dump("val2018.json", INAT_CATEGORIES, INAT_VAL)
    dump("train2019.json", INAT19_CATEGORIES, INAT19_TRAIN)
    dump("val2019.json", INAT19_CATEGORIES, INAT19_VAL)
    return str(root)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
