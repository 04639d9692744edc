"""iNaturalist 2018 / 2019 (reference: datasets/inat.py): the competition's JSON files list images, categories and annotations.
Construction reads the two JSON files and opens no image.  Like ILSVRC, the training split is far larger than a resident store:
``store='auto'`` (the dataset names ``inat-stream``, ``inat_<supercategory>-stream``, ``inat2019-stream``) or ``store='stream'``."""
import json
import os

from .files import FileDatasetGenerator

# channel statistics of the training images of iNaturalist 2018, all of them (None) and per super-category, as the reference
# publishes them (datasets/inat.py:8-24): (mean, standard deviation), RGB
SUPERCATEGORY_STATS = {
    None: ([119.99310088, 122.86333725, 102.38318464], [60.83471124, 59.33123704, 65.92057842]),
    'actinopterygii': ([95.60659929, 109.21340134, 99.53273934], [62.64981594, 56.77583425, 57.79043402]),
    'amphibia': ([120.38820316, 112.09448704, 93.57291079], [64.38971069, 60.88945117, 60.689195]),
    'animalia': ([117.86148813, 112.27558493, 100.76823038], [65.10786879, 60.9941875, 61.3212783]),
    'arachnida': ([123.05328454, 123.11786486, 99.49669769], [62.10607939, 59.69295922, 64.12102046]),
    'aves': ([125.68554284, 131.58931007, 123.51576605], [56.91926625, 57.04151665, 67.97284604]),
    'bacteria': ([130.44253929, 118.58949652, 100.64353881], [63.52655078, 61.3866035, 62.52496727]),
    'chromista': ([126.63609004, 120.30744082, 103.69842308], [61.3142875, 60.35121831, 64.33445667]),
    'fungi': ([105.4904181, 98.20844854, 81.95195412], [66.43803547, 63.26916273, 61.75505097]),
    'insecta': ([126.79141945, 126.55725101, 94.4626541], [62.46710552, 59.70656548, 64.38703598]),
    'mammalia': ([119.32537707, 119.28610021, 105.22655576], [60.25561291, 58.86410094, 60.85549787]),
    'mollusca': ([119.15865454, 107.82338741, 93.65438902], [65.54171188, 62.00986655, 62.64830566]),
    'plantae': ([109.4558912, 115.78290918, 84.83970548], [60.36177593, 59.17162815, 60.81183456]),
    'protozoa': ([99.4855571, 90.12976005, 71.67906874], [69.23439903, 63.83415135, 59.1059619]),
    'reptilia': ([126.42469824, 119.44987437, 103.84680809], [63.4749642, 60.19704406, 60.20556052]),
}
INAT2019_MEAN = [115.77492586, 120.84414891, 93.51744386]
INAT2019_STD = [60.46127213, 58.63136496, 63.5872299]


def read_annotations(json_file, image_folder, supercategory=None):
    """``(tuples, class_indices)`` of one JSON file: the categories whose lower-cased ``supercategory`` is ``supercategory`` (all of
    them for ``None``) are renumbered from 0 in ascending order of their ids; ``class_indices`` maps their names to the new numbers;
    ``tuples`` holds ``(new number, absolute path)`` of every annotation of such a category, in the order of the file."""
    with open(json_file) as f:
        data = json.load(f)
    wanted = None if supercategory is None else supercategory.lower()
    categories = {c['id']: c for c in data['categories'] if wanted is None or c['supercategory'].lower() == wanted}
    renumbered = {old: new for new, old in enumerate(sorted(categories))}
    file_names = {im['id']: im['file_name'] for im in data['images']}
    tuples = [(renumbered[a['category_id']], os.path.abspath(os.path.join(image_folder, file_names[a['image_id']])))
              for a in data['annotations'] if a['category_id'] in categories]
    return tuples, {categories[old]['name']: new for old, new in renumbered.items()}


class INatGenerator(FileDatasetGenerator):
    """``train_file`` / ``val_file``: JSON files, relative to ``root_dir`` unless absolute; ``supercategory``: restrict the 2018
    dataset to one of the keys of SUPERCATEGORY_STATS.  ``classes`` are the category names in the order of their new numbers, taken
    from the training file.  With ``mean`` and ``std`` both ``None``, the published statistics of the super-category are used where
    there are any; otherwise missing statistics are computed from the training images.  No random erasing.  Every other argument is
    the base class's."""

    def __init__(self, root_dir, train_file='train2018.json', val_file='val2018.json', supercategory=None, cropsize=(224, 224),
                 default_target_size=256, mean=None, std=None, **kwargs):
        super(INatGenerator, self).__init__(root_dir, cropsize=cropsize, default_target_size=default_target_size, **kwargs)
        train_file, val_file = (f if os.path.isabs(f) else os.path.join(root_dir, f) for f in (train_file, val_file))
        self.train_tuples, self.class_indices = self.get_tuples_for_supercategory(train_file, root_dir, supercategory)[::2]
        self.test_tuples = self.get_tuples_for_supercategory(val_file, root_dir, supercategory)[0]
        self._train_labels, self.train_img_files = ([t[k] for t in self.train_tuples] for k in (0, 1))
        self._test_labels, self.test_img_files = ([t[k] for t in self.test_tuples] for k in (0, 1))
        self.classes = sorted(self.class_indices, key=self.class_indices.get)
        key = supercategory.lower() if isinstance(supercategory, str) else supercategory
        if mean is None and std is None and key in SUPERCATEGORY_STATS:
            mean, std = SUPERCATEGORY_STATS[key]
        self._compute_stats(mean, std)

    @staticmethod
    def get_tuples_for_supercategory(fname, image_folder, supercategory=None):
        """The reference's method: ``(tuples, number of classes, class_indices)`` (see ``read_annotations``)."""
        tuples, class_indices = read_annotations(fname, image_folder, supercategory)
        return tuples, len(class_indices), class_indices
