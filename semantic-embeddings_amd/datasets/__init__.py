"""Data generators with the attribute/method interface of the reference's ``datasets`` package
(reference: datasets/__init__.py:21-166, datasets/common.py:210-331,673-844):
``num_classes, num_train, num_test, num_channels, labels_train, labels_test, classes`` and
``train_sequence / test_sequence / flow_train / flow_test``.

Batches are produced ON THE DEVICE (channels_last float tensors), so images/s is not bound by a
Python loader: the synthetic generators draw N(0,1) images with fixed seeds (BASELINE.json's
configs are all measured on synthetic batches), the CIFAR generator keeps the whole pickle-decoded
dataset in HBM and augments there -- shift + flip as tensor ops; any other configuration of the reference's train_generator_kwargs
(the 'cifar-10' preset's zoom, rotation, shear, vertical flip, fill modes) as Keras' affine random_transform in one launch of
se_tiny_batch (csrc/tiny_batch.hip), bit for bit what scipy.ndimage.affine_transform gives -- and the file-based generators (NAB / CUB, Cars, Flowers, sub-directory datasets:
datasets/files.py) keep the DECODED uint8 images of a split in HBM and compose every batch -- Pillow's bilinear resize, normalisation,
flip, random erasing, crop, reflect padding -- in one launch of se_image_batch (csrc/image_batch.hip).  The decoded training images
of ILSVRC and iNaturalist (datasets/ilsvrc.py, datasets/inat.py) do not fit a resident store: a split that does not fit is STREAMED
-- decoded on the host ahead of use by a thread pool, staged through a ring of pinned buffers and composed by the same kernel
(datasets/files.py has the rules).  A streamed split is bound by the host's JPEG decoding, so it is opt-in: the keyword ``store`` of
the classes, or the last suffix '-stream' of a dataset name.
"""
# pre-processing statistics of the reference's presets (datasets/__init__.py:4-8), RGB order; ahead of the imports that read them
CAFFE_MEAN = [123.68, 116.779, 103.939]
CAFFE_STD = [1., 1., 1.]
IMAGENET_MEAN = [122.65435242, 116.6545058, 103.99789959]
IMAGENET_STD = [71.40583196, 69.56888997, 73.0440314]

from .common import (DeviceBatchSequence, InMemoryDatasetGenerator, SyntheticGenerator,  # noqa: E402,F401
                     affine_batch_host, affine_matrices)
from .cifar import CifarGenerator  # noqa: E402,F401
from .files import (CarsGenerator, FileDatasetGenerator, FlowersGenerator, NABGenerator,  # noqa: E402,F401
                    SubDirectoryGenerator)
from .ilsvrc import ILSVRCGenerator  # noqa: E402,F401
from .inat import INAT2019_MEAN, INAT2019_STD, INatGenerator  # noqa: E402,F401

# the reference's 'cifar-10' preset (datasets/__init__.py:80-83)
CIFAR10_AUGMENTATION = {'horizontal_flip': True, 'width_shift_range': 0.15, 'height_shift_range': 0.15, 'zoom_range': 0.25}

SYNTHETIC_PRESETS = {
    # name: (num_classes, height/width, channels, num_train, num_test)
    'synthetic-cifar100': (100, 32, 3, 50000, 10000),
    'synthetic-cub': (200, 224, 3, 5994, 5794),
    'synthetic-ilsvrc': (1000, 224, 3, 1281167, 50000),
}


def get_data_generator(dataset, data_root, classes=None):
    """Shortcut for creating a data generator with default settings (datasets/__init__.py:21).

    Supported names: 'cifar-10', 'cifar-100', 'cifar-100-a', 'cifar-100-b' (python pickles under
    ``data_root``) and 'synthetic-cifar100' / 'synthetic-cub' / 'synthetic-ilsvrc' or the generic
    'synthetic:<classes>x<size>x<train>x<test>' (``data_root`` ignored); the file-based 'nab', 'cub', 'cub-sub<N>', 'cars',
    'flowers', 'mit67scenes', 'ucmlu' and 'resisc45' with the reference's presets (datasets/__init__.py:60-162), each optionally
    followed by '-large' (NAB: target size 512, crops of 448 x 448), then '-ilsvrcmean' (ImageNet statistics) or '-caffe' (BGR,
    ImageNet mean, no standard deviation).

    Every file-based name takes '-stream' as its LAST suffix: the generator is built with ``store='auto'``, so a split whose
    decoded images do not fit the resident store is streamed instead of refused ('nab-large-stream': stream what does not fit).
    Only with it, 'ilsvrc', 'inat' / 'inat2018' (optionally '_<supercategory>') and 'inat2019' resolve to ILSVRCGenerator and
    INatGenerator with the reference's presets ('-large' applies to iNaturalist; ILSVRCGenerator takes no sizes, so
    'ilsvrc-large-stream' is a TypeError).  Like the reference's factory, ``classes`` is not handed to INatGenerator: its classes
    are the categories of the (super-category of the) JSON file.  Without '-stream', 'ilsvrc' and 'inat*' raise
    NotImplementedError: their training splits do not fit a resident store."""
    name = dataset.lower()
    stream = name.endswith('-stream')
    if stream:
        if name.startswith(('synthetic', 'cifar')):
            raise ValueError('Unknown dataset: {} (only file-based datasets stream)'.format(dataset))
        name = name[:-7]
    if name in SYNTHETIC_PRESETS:
        c, hw, ch, ntr, nte = SYNTHETIC_PRESETS[name]
        return SyntheticGenerator(c if classes is None else len(classes), hw, ch, ntr, nte, classes=classes)
    if name.startswith('synthetic:'):
        c, hw, ntr, nte = (int(v) for v in name.split(':', 1)[1].split('x'))
        return SyntheticGenerator(c if classes is None else len(classes), hw, 3, ntr, nte, classes=classes)
    if name == 'cifar-10':
        return CifarGenerator(data_root, classes, reenumerate=True, cifar10=True, train_generator_kwargs=dict(CIFAR10_AUGMENTATION))
    if name == 'cifar-100':
        return CifarGenerator(data_root, classes, reenumerate=True)
    if name.startswith('cifar-100-a'):
        return CifarGenerator(data_root, list(range(50)), reenumerate=name.endswith('-consec'))
    if name.startswith('cifar-100-b'):
        return CifarGenerator(data_root, list(range(50, 100)), reenumerate=name.endswith('-consec'))

    kwargs = {'store': 'auto'} if stream else {}
    if name.startswith('inat2018'):
        name = 'inat' + name[8:]
    if name.endswith('-ilsvrcmean'):
        kwargs.update(mean=IMAGENET_MEAN, std=IMAGENET_STD)
        name = name[:-11]
    elif name.endswith('-caffe'):
        kwargs.update(mean=CAFFE_MEAN, std=CAFFE_STD, color_mode='bgr')
        name = name[:-6]
    if name.endswith('-large'):
        kwargs.update(cropsize=(448, 448), default_target_size=512)
        name = name[:-6]
    if (name == 'ilsvrc' or name.startswith('inat')) and not stream:
        raise NotImplementedError('dataset "{0}": the decoded training images of ILSVRC and iNaturalist do not fit the device-resident '
                                  'image store; append -stream ("{0}-stream") to decode them on the host as they are used'.format(dataset))
    if name == 'ilsvrc':
        return ILSVRCGenerator(data_root, classes, **kwargs)
    if name == 'inat' or name.startswith('inat_'):
        if 'default_target_size' not in kwargs:
            kwargs['randzoom_range'] = (256, 480)
        return INatGenerator(data_root, supercategory=name[5:] if name.startswith('inat_') else None, **kwargs)
    if name == 'inat2019':
        if 'mean' not in kwargs and 'std' not in kwargs:
            kwargs.update(mean=INAT2019_MEAN, std=INAT2019_STD)
        if 'default_target_size' not in kwargs:
            kwargs['randzoom_range'] = (256, 480)
        return INatGenerator(data_root, 'train2019.json', 'val2019.json', **kwargs)
    if name == 'nab':
        if 'default_target_size' not in kwargs:
            kwargs['randzoom_range'] = (256, 480)
        return NABGenerator(data_root, classes, 'images', **kwargs)
    if name == 'cub' or name.startswith('cub-sub'):
        kwargs.setdefault('mean', [123.82988033, 127.35116805, 110.25606303])
        kwargs.setdefault('std', [59.2230949, 58.0736071, 67.80251684])
        if name.startswith('cub-sub'):
            samples_per_class = int(name[7:])
            kwargs['split_file'] = 'train_test_split_{}.txt'.format(samples_per_class)
            kwargs['train_repeats'] = 30 // samples_per_class
        kwargs.update(cropsize=(448, 448), default_target_size=512, randzoom_range=None)
        return NABGenerator(data_root, classes, 'images', **kwargs)
    if name == 'cars':
        return CarsGenerator(data_root, classes, **kwargs)
    if name == 'flowers':
        return FlowersGenerator(data_root, classes, **kwargs)
    presets = {'mit67scenes': ([124.62788179, 110.01028625, 94.95780545], [68.56923599, 66.86607736, 67.35944349]),
               'ucmlu': ([122.65409223, 124.40230701, 114.25659171], [55.74499679, 51.65585669, 50.16527551]),
               'resisc45': ([94.17769482, 97.40967803, 87.80359702], [51.92246172, 47.22081475, 47.07685676])}
    if name in presets:
        if 'mean' not in kwargs and 'std' not in kwargs:
            kwargs['mean'], kwargs['std'] = presets[name]
        if name == 'mit67scenes':
            kwargs.update(img_dir='Images', train_list='TrainImages.txt', test_list='TestImages.txt')
        return SubDirectoryGenerator(data_root, classes, **kwargs)
    raise ValueError('Unknown dataset: {}'.format(dataset))
