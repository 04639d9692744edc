"""Device-resident batch sequences (the role of datasets/common.py's DataSequence and
TinyDatasetGenerator in the reference, re-designed for one-process-per-GPU training).

The in-memory generator has two batch paths.  The configuration it always had -- equal fractional width / height shifts, an optional
horizontal flip, edges replicated -- is composed from torch tensor ops on a standardised copy of the split.  Every other
``train_generator_kwargs`` configuration of the reference (rotation, shear, zoom, vertical flip, unequal or pixel shifts, fill modes
'constant' and 'reflect') is Keras' affine ``random_transform``: ``draw_affine`` draws the parameters, ``affine_matrices`` builds
Keras 2.2's matrices and ONE launch of ``se_tiny_batch`` (csrc/tiny_batch.hip) gathers, transforms, flips and standardises a raw
float32 copy of the split, bit for bit what ``scipy.ndimage.affine_transform`` -- Keras' back end -- gives (``affine_batch_host`` is
the NumPy restatement of that arithmetic the tests compare the kernel with)."""
import numpy as np
import torch

FILL_MODES = ('nearest', 'constant', 'reflect')
# keys of the reference's train_generator_kwargs (keras ImageDataGenerator arguments) the affine path implements, with Keras' defaults
AFFINE_DEFAULTS = {'horizontal_flip': False, 'vertical_flip': False, 'width_shift_range': 0.0, 'height_shift_range': 0.0,
                   'rotation_range': 0.0, 'shear_range': 0.0, 'zoom_range': 0.0, 'fill_mode': 'nearest', 'cval': 0.0}


def _scalar_range(key, value):
    """A Keras range argument as a float >= 0: scalar floats only (a list means a choice of values and an integer a discrete pixel
    range in Keras; neither is built).  An integer 0 is Keras' own 'off'."""
    if isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_)) and value == 0:
        return 0.0
    if not isinstance(value, (float, np.floating)) or not value >= 0:
        raise NotImplementedError('train_generator_kwargs[%r] = %r: only scalar float ranges >= 0 are built' % (key, value))
    return float(value)


def affine_config(train_generator_kwargs):
    """The reference's ``train_generator_kwargs`` checked and normalised: every key of AFFINE_DEFAULTS present, ``zoom_range`` as
    (lo, hi).  A key outside that set, or a value this build does not implement, raises NotImplementedError naming the key."""
    cfg = dict(AFFINE_DEFAULTS)
    for key, value in dict(train_generator_kwargs).items():
        if key not in AFFINE_DEFAULTS:
            raise NotImplementedError('train_generator_kwargs[%r]: not built for the in-memory datasets (supported: %s)'
                                      % (key, ', '.join(sorted(AFFINE_DEFAULTS))))
        cfg[key] = value
    for key in ('width_shift_range', 'height_shift_range', 'rotation_range', 'shear_range'):
        cfg[key] = _scalar_range(key, cfg[key])
    zoom = cfg['zoom_range']
    if isinstance(zoom, (tuple, list)) and len(zoom) == 2 and all(isinstance(v, (int, float, np.integer, np.floating)) for v in zoom):
        cfg['zoom_range'] = (float(zoom[0]), float(zoom[1]))
    else:
        z = _scalar_range('zoom_range', zoom)
        cfg['zoom_range'] = (1.0 - z, 1.0 + z)
    if not 0 < cfg['zoom_range'][0] <= cfg['zoom_range'][1]:
        raise NotImplementedError('train_generator_kwargs[%r] = %r: 0 < lower <= upper' % ('zoom_range', zoom))
    if cfg['fill_mode'] not in FILL_MODES:
        raise NotImplementedError("train_generator_kwargs['fill_mode'] = %r: only %s are built" % (cfg['fill_mode'], ', '.join(FILL_MODES)))
    for key in ('horizontal_flip', 'vertical_flip'):
        cfg[key] = bool(cfg[key])
    cfg['cval'] = float(cfg['cval'])
    return cfg


def affine_matrices(params, h, w):
    """[B, 6] float64 ``(M00, M01, M02, M10, M11, M12)``: the output (row, col) -> source (row, col) maps of Keras 2.2's
    ``apply_affine_transform`` for the drawn ``params`` (``draw_affine``: theta and shear in degrees, tx / ty in rows / columns, zx / zy).
    ``T = R S Sh Z`` with R = [[cos t, -sin t, 0], [sin t, cos t, 0], [0, 0, 1]], S = [[1, 0, tx], [0, 1, ty], [0, 0, 1]],
    Sh = [[1, -sin s, 0], [0, cos s, 0], [0, 0, 1]], Z = diag(zx, zy, 1), centred with ``o_x = h / 2 + 0.5``, ``o_y = w / 2 + 0.5``:
    ``M = [[1, 0, o_x], [0, 1, o_y], [0, 0, 1]] T [[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]]``.  The ``+ 0.5`` is Keras 2.2's
    (keras_preprocessing 1.0.x ``transform_matrix_offset_center``), which the reference ran; later releases centre on
    ``h / 2 - 0.5``.  (Keras leaves an identity factor out of the product; multiplying by one changes no entry.)"""
    theta, shear = np.deg2rad(np.asarray(params['theta'], dtype=np.float64)), np.deg2rad(np.asarray(params['shear'], dtype=np.float64))
    b = theta.shape[0]
    eye = np.broadcast_to(np.eye(3), (b, 3, 3))
    R, S, Sh, Z = (eye.copy() for _ in range(4))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1] = np.cos(theta), -np.sin(theta), np.sin(theta), np.cos(theta)
    S[:, 0, 2], S[:, 1, 2] = params['tx'], params['ty']
    Sh[:, 0, 1], Sh[:, 1, 1] = -np.sin(shear), np.cos(shear)
    Z[:, 0, 0], Z[:, 1, 1] = params['zx'], params['zy']
    o_x, o_y = float(h) / 2 + 0.5, float(w) / 2 + 0.5
    offset = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]], dtype=np.float64)
    reset = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]], dtype=np.float64)
    M = np.matmul(np.matmul(offset, np.matmul(np.matmul(np.matmul(R, S), Sh), Z)), reset)
    return np.ascontiguousarray(M[:, :2, :].reshape(b, 6))


def _axis_host(v, n, fill_mode):
    """One axis of ``affine_batch_host``: (tap i0, tap i1, fraction f, outside) for float64 coordinates ``v`` on an axis of length n."""
    last = float(n - 1)
    if fill_mode == 'reflect':
        if n == 1:
            v = np.zeros_like(v)
        else:
            length, p = float(n), 2.0 * n
            lo, hi = v < 0, v > last
            with np.errstate(invalid='ignore', over='ignore'):
                far = v < -p
                a = np.where(far, p * np.trunc(-v / p) + v, v)
                a = np.where(a < -length, a + p, -a - 1.0)
                c = v - p * np.trunc(v / p)
                c = np.where(c >= length, p - c - 1.0, c)
            v = np.where(lo, a, np.where(hi, c, v))
        fl = np.floor(v)
        i = np.clip(np.nan_to_num(fl, nan=-1.0), -1, n - 1).astype(np.int64)
        fold = lambda j: np.where(np.mod(j, 2 * n) < n, np.mod(j, 2 * n), 2 * n - 1 - np.mod(j, 2 * n))
        return fold(i), fold(i + 1), v - fl, np.zeros(v.shape, dtype=bool)
    outside = (v < 0) | (v > last) if fill_mode == 'constant' else np.zeros(v.shape, dtype=bool)
    fl = np.floor(v)                                      # 'nearest' keeps the coordinate and clamps the taps
    i = np.clip(np.nan_to_num(fl, nan=-1.0), -1, n - 1).astype(np.int64)
    with np.errstate(invalid='ignore'):
        return np.maximum(i, 0), np.minimum(i + 1, n - 1), v - fl, outside


def affine_batch_host(images, index, affine, flags, mean, stdp, fill_mode='nearest', cval=0.0):
    """NumPy restatement of ``se_tiny_batch`` (include/sehip.h), operation for operation in the order of scipy's
    NI_GeometricTransform: float64 coordinates ``y = (r M00 + c M01) + M02`` evaluated at the flipped output position, the fill mode's
    per-axis coordinate rule, weights ``w0 = 1 - f``, ``w1 = 1 - w0``, the bilinear value ``(((0 + (a00 wy0) wx0) + (a01 wy0) wx1) +
    (a10 wy1) wx0) + (a11 wy1) wx1`` rounded to float32, then ``(v - mean) / stdp`` in float32.
    ``images`` [N, H, W, C] float32, ``index`` [B], ``affine`` [B, 6] float64, ``flags`` [B] (bit 0 horizontal, bit 1 vertical flip).
    Returns [B, H, W, C] float32; a sample whose index is outside the store is NaN."""
    if fill_mode not in FILL_MODES:
        raise ValueError('fill_mode %r' % (fill_mode,))
    images = np.asarray(images, dtype=np.float32)
    n_img, h, w, ch = images.shape
    index, flags = np.asarray(index, dtype=np.int64), np.asarray(flags, dtype=np.int64)
    m = np.asarray(affine, dtype=np.float64).reshape(-1, 6)[:, :, None, None]             # [B, 6, 1, 1]
    mean, stdp = np.asarray(mean, dtype=np.float32).reshape(-1), np.asarray(stdp, dtype=np.float32).reshape(-1)
    valid = (index >= 0) & (index < n_img)
    src = np.where(valid, index, 0)
    r = np.arange(h, dtype=np.float64)[None, :, None]
    c = np.arange(w, dtype=np.float64)[None, None, :]
    r = np.where((flags & 2)[:, None, None] != 0, (h - 1) - r, r)
    c = np.where((flags & 1)[:, None, None] != 0, (w - 1) - c, c)
    y = (r * m[:, 0] + c * m[:, 1]) + m[:, 2]
    x = (r * m[:, 3] + c * m[:, 4]) + m[:, 5]
    iy0, iy1, fy, oy = _axis_host(y, h, fill_mode)
    ix0, ix1, fx, ox = _axis_host(x, w, fill_mode)
    bi = src[:, None, None]
    tap = lambda iy, ix: images[bi, iy, ix].astype(np.float64)                               # [B, H, W, C]
    with np.errstate(over='ignore', invalid='ignore'):
        wy0, wx0 = 1.0 - fy[..., None], 1.0 - fx[..., None]
        wy1, wx1 = 1.0 - wy0, 1.0 - wx0
        t = (((0.0 + (tap(iy0, ix0) * wy0) * wx0) + (tap(iy0, ix1) * wy0) * wx1) + (tap(iy1, ix0) * wy1) * wx0) + (tap(iy1, ix1) * wy1) * wx1
        v32 = np.where((oy | ox)[..., None], np.float32(cval), t.astype(np.float32))
        out = ((v32 - mean) / stdp).astype(np.float32)
    out[~valid] = np.nan
    return out


class DeviceBatchSequence(object):
    """Indexable sequence of batches, ``len()`` = batches per epoch, ``seq[i] -> (X, y)`` like a
    ``keras.utils.Sequence`` (datasets/common.py:26-122), but X/y are device tensors.

    ``rank``/``world_size`` shard every global batch across data-parallel processes: rank r takes
    rows ``r::world_size`` of the global batch, so the union over ranks is the reference's batch.
    ``batch_transform(X, y, **kwargs)`` is applied last (e.g. learn_image_embeddings.transform_inputs).
    ``repeats`` sub-epochs make one epoch, each with a permutation of its own (datasets/common.py:87-122: ``len()`` is
    ``repeats`` x batches per sub-epoch); ``compose_kwargs`` are handed on to ``generator.compose_batch``.

    A generator with a ``prefetch(indices, train)`` method (the streamed store of datasets/files.py) is told, before batch ``i`` is
    composed, the rows of the next ``generator.prefetch_batches`` batches of the same pass -- this rank's rows, exactly what the
    later ``compose_batch`` calls will bring.  Never past the end of the current permutation: the next one does not exist yet."""

    def __init__(self, generator, indices, labels, batch_size=32, shuffle=False, train=False, augment=False,
                 batch_transform=None, batch_transform_kwargs={}, rank=0, world_size=1, seed=0, repeats=1, compose_kwargs=None):
        self.generator = generator
        self.indices = np.asarray(indices)
        self.labels = np.asarray(labels)
        self.batch_size, self.shuffle, self.train, self.augment = batch_size, shuffle, train, augment
        self.batch_transform, self.batch_transform_kwargs = batch_transform, batch_transform_kwargs
        self.rank, self.world_size = rank, world_size
        self.rng = np.random.default_rng(seed)      # same seed on every rank -> same permutation
        self.repeats, self.compose_kwargs = int(repeats), dict(compose_kwargs or {})
        self.epoch_len = int(np.ceil(len(self.indices) / self.batch_size))
        self.perms = [np.arange(len(self.indices)) for _ in range(self.repeats)]
        self.perm = self.perms[0]
        self.on_epoch_end()

    def __len__(self):
        return self.repeats * self.epoch_len

    def on_epoch_end(self):
        if self.shuffle:
            for perm in self.perms:
                self.rng.shuffle(perm)

    def _rows(self, sub, idx):
        glob = self.perms[sub][idx * self.batch_size:(idx + 1) * self.batch_size]
        sel = glob[self.rank::self.world_size]
        if len(sel) == 0 and len(glob):     # a short last batch with fewer rows than ranks: no rank may see an empty batch (its mean
            sel = glob[[self.rank % len(glob)]]   # would be NaN and the all-reduce would spread it): re-use one of the rows
        return sel

    def __getitem__(self, idx):
        sub = min(idx // max(self.epoch_len, 1), self.repeats - 1)
        idx -= sub * self.epoch_len
        sel = self._rows(sub, idx)
        announce = getattr(self.generator, 'prefetch', None)
        if announce is not None:
            ahead = int(getattr(self.generator, 'prefetch_batches', 0))
            for nxt in range(idx + 1, min(idx + 1 + ahead, self.epoch_len)):
                announce(self.indices[self._rows(sub, nxt)], self.train)
        X = self.generator.compose_batch(self.indices[sel], train=self.train, augment=self.augment, **self.compose_kwargs)
        y = torch.from_numpy(self.labels[sel].astype(np.int64)).to(X.device, non_blocking=True)
        if self.batch_transform is not None:
            return self.batch_transform(X, y, **self.batch_transform_kwargs)
        return X, y

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]
        self.on_epoch_end()


class _GeneratorBase(object):
    """Attribute interface shared by all generators (datasets/common.py:584-631,799-844)."""

    device = None

    def _dev(self):
        if self.device is None:
            self.device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        return self.device

    @property
    def labels_train(self):
        return self.y_train

    @property
    def labels_test(self):
        return self.y_test

    @property
    def num_classes(self):
        return len(self.classes)

    @property
    def num_train(self):
        return len(self.y_train)

    @property
    def num_test(self):
        return len(self.y_test)

    def train_sequence(self, batch_size=32, shuffle=True, augment=True, batch_transform=None, batch_transform_kwargs={}, **dp):
        return DeviceBatchSequence(self, np.arange(self.num_train), self.y_train, batch_size, shuffle, True, augment,
                                   batch_transform, batch_transform_kwargs, **dp)

    def test_sequence(self, batch_size=32, shuffle=False, augment=False, batch_transform=None, batch_transform_kwargs={}, **dp):
        return DeviceBatchSequence(self, np.arange(self.num_test), self.y_test, batch_size, shuffle, False, augment,
                                   batch_transform, batch_transform_kwargs, **dp)

    def flow_train(self, batch_size=32, include_labels=True, shuffle=True, augment=True):
        for X, y in self.train_sequence(batch_size, shuffle, augment):
            yield (X, y) if include_labels else X

    def flow_test(self, batch_size=32, include_labels=True, shuffle=False, augment=False):
        for X, y in self.test_sequence(batch_size, shuffle, augment):
            yield (X, y) if include_labels else X


class SyntheticGenerator(_GeneratorBase):
    """N(0,1) images drawn on the device from per-batch seeds (reproducible, no host traffic);
    labels uniform over the classes with a fixed seed."""

    def __init__(self, num_classes, size, channels, num_train, num_test, classes=None, dtype=torch.float32):
        self.classes = list(range(num_classes)) if classes is None else list(classes)
        self.size, self.num_channels, self.dtype = size, channels, dtype
        rng = np.random.default_rng(1)
        self.y_train = rng.integers(0, num_classes, size=num_train).tolist()
        self.y_test = rng.integers(0, num_classes, size=num_test).tolist()

    def compose_batch(self, indices, train=True, augment=False):
        dev = self._dev()
        g = torch.Generator(device=dev)
        g.manual_seed(int(indices[0]) * 2 + int(train) if len(indices) else 0)
        x = torch.randn((len(indices), self.num_channels, self.size, self.size), generator=g, device=dev, dtype=self.dtype)
        return x.contiguous(memory_format=torch.channels_last)


class InMemoryDatasetGenerator(_GeneratorBase):
    """Small-image datasets held entirely in HBM (the reference's TinyDatasetGenerator, datasets/common.py:635-844).

    Pre-processing follows Keras' ``ImageDataGenerator(featurewise_center, featurewise_std_normalization).fit(X_train)`` +
    ``standardize`` [third party: keras_preprocessing 1.0.x]: PER-CHANNEL mean and standard deviation of the training set
    (reduced over samples, rows and columns), float32, ``x = (x - mean) / (std + 1e-6)``.  Training batches get a random
    horizontal flip and random width / height shifts drawn uniformly from +-15 % of the image size -- continuous offsets,
    bilinear interpolation (Keras ``order = 1``) with edge replication (``fill_mode = 'nearest'``) -- as tensor ops on the
    device.  (The random numbers come from torch's device generator, not NumPy's: same distribution, different draws.)

    ``train_generator_kwargs`` takes the reference's dictionary of ``ImageDataGenerator`` arguments instead (it then replaces
    ``shift_range`` / ``horizontal_flip``; absent keys have Keras' defaults): ``horizontal_flip, vertical_flip, width_shift_range,
    height_shift_range, rotation_range, shear_range, zoom_range, fill_mode`` ('nearest', 'constant', 'reflect'), ``cval``; any other
    key raises NotImplementedError.  A configuration that is only the one above keeps the torch path (``self.affine`` is None); any
    other is composed by ``se_tiny_batch`` from a raw float32 NHWC copy of the split (``self.affine`` holds the checked
    configuration), with parameters from a NumPy generator.  That path needs the GPU."""

    def __init__(self, X_train, X_test, y_train, y_test, shift_range=0.15, horizontal_flip=True, train_generator_kwargs=None):
        self.X_train_h, self.X_test_h = X_train, X_test      # NHWC float32 host arrays
        self.y_train, self.y_test = list(y_train), list(y_test)
        self.affine = None
        if train_generator_kwargs is not None:
            cfg = affine_config(train_generator_kwargs)
            shift = cfg['width_shift_range']
            plain = (cfg['height_shift_range'] == shift and shift < 1 and not cfg['vertical_flip'] and not cfg['rotation_range']
                     and not cfg['shear_range'] and cfg['zoom_range'] == (1.0, 1.0) and cfg['fill_mode'] == 'nearest')
            shift_range, horizontal_flip = (shift if plain else None), cfg['horizontal_flip']
            if not plain:
                self.affine = cfg
        self.rng = np.random.default_rng(0)                  # affine draws of compose_batch calls that bring no generator of their own
        self._raw, self._stats = {}, None
        self.shift_range, self.horizontal_flip = shift_range, horizontal_flip
        X32 = np.asarray(X_train, dtype=np.float32)
        self.mean = np.mean(X32, axis=(0, 1, 2), keepdims=True)                       # [1, 1, 1, C]
        self.std = np.std(X32 - self.mean, axis=(0, 1, 2), keepdims=True) + np.float32(1e-6)
        self.num_channels = X_train.shape[-1]
        self._dev_data = None

    def _data(self):
        if self._dev_data is None:
            dev = self._dev()
            prep = lambda a: torch.from_numpy(((np.asarray(a, dtype=np.float32) - self.mean) / self.std).transpose(0, 3, 1, 2).copy()).to(dev)
            self._dev_data = (prep(self.X_train_h), prep(self.X_test_h))
        return self._dev_data

    @staticmethod
    def apply_transform(x, row_shift, col_shift, flip):
        """The reference's per-image augmentation with GIVEN parameters, batched on the device: Keras' ``random_transform`` shifts
        first -- ``out[r, c] = in[r + row_shift, c + col_shift]``, bilinear (``order = 1``), edges replicated (``fill_mode =
        'nearest'``) -- and flips horizontally afterwards (datasets/common.py:786-787 -> ImageDataGenerator.random_transform).
        x [B, C, H, W]; row_shift / col_shift [B] float pixels; flip [B] bool."""
        b, _, h, w = x.shape
        rr = torch.arange(h, device=x.device, dtype=torch.float32)[None, :] + row_shift.to(torch.float32)[:, None]   # source row of every output row
        cc = torch.arange(w, device=x.device, dtype=torch.float32)[None, :] + col_shift.to(torch.float32)[:, None]
        gy = (rr / max(h - 1, 1) * 2 - 1)[:, :, None].expand(b, h, w)
        gx = (cc / max(w - 1, 1) * 2 - 1)[:, None, :].expand(b, h, w)
        x = torch.nn.functional.grid_sample(x, torch.stack((gx, gy), dim=-1), mode='bilinear', padding_mode='border', align_corners=True)
        return torch.where(flip[:, None, None, None], x.flip(3), x)

    def draw_transform(self, b, h, w, device):
        """(row_shift, col_shift, flip) like ImageDataGenerator.get_random_transform: shifts uniform in +-shift_range x size, flip
        with probability 1/2 -- from torch's device generator (same distribution as the reference's np.random draws, other numbers)."""
        zero = torch.zeros(b, device=device)
        row = (torch.rand(b, device=device) * 2 - 1) * (self.shift_range * h) if self.shift_range else zero
        col = (torch.rand(b, device=device) * 2 - 1) * (self.shift_range * w) if self.shift_range else zero
        flip = (torch.rand(b, device=device) < 0.5) if self.horizontal_flip else torch.zeros(b, dtype=torch.bool, device=device)
        return row, col, flip

    def draw_affine(self, b, h, w, rng):
        """Per-sample parameters of the affine path with the distributions of Keras 2.2's ``get_random_transform``, from the NumPy
        generator ``rng``: theta ~ U(+-rotation_range) degrees; tx ~ U(+-height_shift_range) rows and ty ~ U(+-width_shift_range)
        columns, a range below 1 being a fraction of h / w; shear ~ U(+-shear_range) degrees; zx, zy ~ U(lo, hi) independently
        ((1, 1) draws nothing); each flip with probability 1/2.  A dict of [b] arrays: theta, tx, ty, shear, zx, zy (float64), hflip,
        vflip (bool)."""
        cfg = self.affine
        sym = lambda r: rng.uniform(-r, r, b) if r else np.zeros(b)
        p = {'theta': sym(cfg['rotation_range'])}
        p['tx'] = sym(cfg['height_shift_range']) * (h if cfg['height_shift_range'] < 1 else 1)
        p['ty'] = sym(cfg['width_shift_range']) * (w if cfg['width_shift_range'] < 1 else 1)
        p['shear'] = sym(cfg['shear_range'])
        lo, hi = cfg['zoom_range']
        if (lo, hi) == (1.0, 1.0):
            p['zx'], p['zy'] = np.ones(b), np.ones(b)
        else:
            zoom = rng.uniform(lo, hi, (b, 2))
            p['zx'], p['zy'] = zoom[:, 0].copy(), zoom[:, 1].copy()
        p['hflip'] = rng.random(b) < 0.5 if cfg['horizontal_flip'] else np.zeros(b, dtype=bool)
        p['vflip'] = rng.random(b) < 0.5 if cfg['vertical_flip'] else np.zeros(b, dtype=bool)
        return p

    def _raw_store(self, train):
        """The affine path's resident copy of a split: raw float32 NHWC on the device, built at first use."""
        if train not in self._raw:
            host = np.ascontiguousarray(np.asarray(self.X_train_h if train else self.X_test_h, dtype=np.float32))
            self._raw[train] = torch.from_numpy(host).to(self._dev())
        if self._stats is None:
            self._stats = tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1))).to(self._dev())
                                for v in (self.mean, self.std))
        return self._raw[train]

    def _compose_affine(self, indices, train, augment, return_params, rng):
        """draw_affine, affine_matrices, one upload (matrices, indices and flags in one int64 buffer), one se_tiny_batch launch."""
        import sehip
        store = self._raw_store(bool(train))
        _, h, w, _ = store.shape
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        b = len(idx)
        params = None
        buf = np.zeros(7 * b + (b + 1) // 2, dtype=np.int64)
        mats, flags = buf[:6 * b].view(np.float64).reshape(b, 6), buf[7 * b:].view(np.int32)[:b]
        if augment:
            params = self.draw_affine(b, h, w, self.rng if rng is None else rng)
            mats[:] = affine_matrices(params, h, w)
            flags[:] = params['hflip'].astype(np.int32) | (params['vflip'].astype(np.int32) << 1)
        else:
            mats[:] = (1, 0, 0, 0, 1, 0)
        buf[6 * b:7 * b] = idx
        if b == 0:
            x = torch.empty((0,) + tuple(store.shape[1:]), dtype=torch.float32, device=store.device).permute(0, 3, 1, 2)
            return (x, params) if return_params else x
        dev = torch.from_numpy(buf).to(store.device)
        out = sehip.tiny_batch(store, dev[6 * b:7 * b], dev[:6 * b].view(torch.float64).view(b, 6), dev[7 * b:].view(torch.int32)[:b],
                               self._stats[0], self._stats[1], self.affine['fill_mode'], self.affine['cval'])
        x = out.permute(0, 3, 1, 2)
        return (x, params) if return_params else x

    def _sequence(self, train, batch_size, shuffle, augment, batch_transform, batch_transform_kwargs, dp):
        labels = self.y_train if train else self.y_test
        kwargs = None
        if self.affine is not None:          # every (split, rank, seed) its own reproducible draws
            kwargs = {'rng': np.random.default_rng([int(train), dp.get('rank', 0), dp.get('seed', 0)])}
        return DeviceBatchSequence(self, np.arange(len(labels)), labels, batch_size, shuffle, train, augment, batch_transform,
                                   batch_transform_kwargs, compose_kwargs=kwargs, **dp)

    def train_sequence(self, batch_size=32, shuffle=True, augment=True, batch_transform=None, batch_transform_kwargs={}, **dp):
        return self._sequence(True, batch_size, shuffle, augment, batch_transform, batch_transform_kwargs, dp)

    def test_sequence(self, batch_size=32, shuffle=False, augment=False, batch_transform=None, batch_transform_kwargs={}, **dp):
        return self._sequence(False, batch_size, shuffle, augment, batch_transform, batch_transform_kwargs, dp)

    def compose_batch(self, indices, train=True, augment=False, return_params=False, rng=None):
        """The batch of ``indices``, [B, C, H, W] channels_last on the device.  Torch path: ``return_params`` adds the drawn (row shift,
        column shift, flip) tensors.  Affine path: it adds the dict ``draw_affine`` drew (None without augmentation), and ``rng`` is the
        NumPy generator the draws come from."""
        if self.affine is not None:
            return self._compose_affine(indices, train, augment, return_params, rng)
        data = self._data()[0 if train else 1]
        idx = torch.from_numpy(np.asarray(indices, dtype=np.int64)).to(data.device)
        x = data.index_select(0, idx)
        params = None
        if augment:
            b, _, h, w = x.shape
            params = self.draw_transform(b, h, w, x.device)
            x = self.apply_transform(x, *params)
        x = x.contiguous(memory_format=torch.channels_last)
        return (x, params) if return_params else x
