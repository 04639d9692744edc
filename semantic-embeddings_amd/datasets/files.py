"""File-based datasets (reference: datasets/common.py:126-631, nab.py, subdirectory.py, cars.py, flowers.py) on a device-resident
image store.

The reference decodes, resizes and augments every sample with Pillow / NumPy in 8 worker processes.  Here the DECODED uint8 images
of a split stay in HBM (CUB: about 6.6 GB) and a batch is composed in one launch of ``se_image_batch`` (csrc/image_batch.hip):
the host only draws the augmentation parameters (``draw_params``) and builds the resampling tables (``sehip.resample_tables``).

* File lists, labels and ``classes`` are built like the reference's, at construction, which reads the metadata files only.
* The store of a split is built lazily, on the first ``compose_batch`` of that split: Pillow decode
  (``Image.open(fn).convert('RGB')``, what Keras' ``load_img`` does) in a thread pool, packed into one uint8 device tensor.
* ``mean`` / ``std`` given as ``None`` are computed from the training images during their decode pass (``_compute_stats``,
  datasets/common.py:186-207), on first use.
* The random numbers come from a ``np.random.Generator``, not NumPy's global stream: the reference's distributions, other draws.

Store tiers (``store=``).  ``'resident'`` is the store above; a split larger than ``store_budget_bytes`` is an error.  ``'stream'``
holds no arena for a split (the ILSVRC training split would take several hundred GB): ``compose_batch`` obtains the decoded images
of exactly its indices, packs them into a staging arena, uploads it once and launches the same ``se_image_batch`` with offsets
relative to that arena and the sizes of the decoded images.  ``draw_params`` runs at compose time, in call order, on either tier, so
the random stream of a (split, rank, seed) does not depend on the tier and the batches of both are bit-identical.  ``'auto'`` decides
per split at first use, from the header-only size pass: what fits the budget is resident, what does not is streamed.  A streamed
split is bound by JPEG decoding on the host, not by the device; that is why it is opt-in.

Rules of the streamed store (``_StreamStore``):

* Threads.  Worker threads only decode (Pillow releases the GIL while it does) and hand NumPy arrays back; they are threads, not
  the reference's worker processes, because a process that has initialised the GPU must not be forked.  Every HIP call -- the upload,
  the launch -- is issued by the thread that called ``compose_batch``, on its current stream.  A generator has one pool of at most
  ``decode_threads`` workers for both splits.
* Look-ahead.  ``prefetch(indices, train)`` announces a batch; its decoding starts at once.  A later ``compose_batch`` finds it by
  its index tuple; a batch nobody announced is decoded on demand.  At most ``prefetch_batches + 2`` announced batches are kept: when
  one more arrives, the oldest that was never collected is dropped and its pending decodes are cancelled.
* Ring.  ``prefetch_batches + 2`` slots, each a pinned host buffer and a device uint8 buffer, taken in turn.  The caller packs the
  decoded images of a batch into the slot's host buffer only after all of them have arrived, copies it to the slot's device buffer
  ``non_blocking`` and records the slot's ``uploaded`` event behind that copy; after the launch it records ``consumed``.
  - A slot's host buffer is not written again until ``uploaded`` has completed (the caller waits on it; with more slots than
    batches in flight it has long completed).
  - A slot's device buffer is written again only in stream order behind the launch that read it: same stream, later in the queue;
    if the caller's current stream has changed since, that stream first waits for ``consumed``.
  - A slot grows geometrically when a batch needs more bytes.  Before its buffers are replaced, ``uploaded`` and ``consumed`` are
    synchronised, so that no copy from or to them and no kernel reading them is in flight when they are released.
* Errors.  Whatever a worker raises for a file surfaces in the caller as ``SehipError`` naming the file.  The futures of a batch are
  all waited for or cancelled before anything is written, so an error leaves no half-filled slot, and nothing waits on a worker
  that is not running.
* Statistics.  With ``mean`` or ``std`` missing, the training split is decoded in file order, a bounded window of images at a time,
  and fed to the sums of ``_stats_from``: the same float64 operations on the same arrays as the resident tier's, so the results are
  equal bit for bit.  The variance is taken around the finished float32 mean, so a generator that lacks both makes two passes (one
  per statistic); no arena is held.
"""
import os
import threading
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from glob import glob

import numpy as np
import torch

import sehip
from sehip import SehipError

from .common import DeviceBatchSequence, _GeneratorBase

DECODE_THREADS = 16
DEFAULT_ERASE_PARAMS = {'sl': 0.02, 'sh': 0.3, 'r1': 0.3, 'r2': 1. / 0.3}


class _Store(object):
    """Decoded images of one split: ``arena`` uint8 (host array until uploaded, then a device tensor), ``offsets`` int64 [N],
    ``sizes`` int32 [N, 2] = (h, w)."""

    tier = 'resident'

    def __init__(self, arena, offsets, sizes):
        self.arena, self.offsets, self.sizes = arena, offsets, sizes
        self.device_arena = None

    def images(self):
        """The decoded images in file order (views of the host arena)."""
        return (self.arena[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(self.offsets, self.sizes))


def _decode_rgb(fn):
    """One file as uint8 [h, w, 3], decoded like the resident store decodes it; any failure names the file."""
    from PIL import Image
    try:
        with Image.open(fn) as im:
            return np.asarray(im.convert('RGB'), dtype=np.uint8)
    except Exception as e:
        raise SehipError('%s: cannot decode: %s: %s' % (fn, type(e).__name__, e))


class _Slot(object):
    """One ring slot: pinned host buffer, device buffer, the event behind the last upload and the one behind the last launch."""

    def __init__(self):
        self.host = self.dev = self.uploaded = self.consumed = self.stream = None

    def view(self, nbytes):
        return self.host.numpy()[:nbytes]


class _StreamStore(object):
    """A split that is decoded batch by batch (the module docstring has the rules).  ``pool`` is a callable returning the
    generator's thread pool."""

    tier = 'stream'
    STATS_WINDOW = 64          # images decoded ahead of the statistics sums

    def __init__(self, files, pool, prefetch_batches):
        self.files, self._pool = files, pool
        self.ring = [_Slot() for _ in range(max(int(prefetch_batches), 0) + 2)]
        self.turn = 0
        self.pending = OrderedDict()       # index tuple -> {index: future}
        self.lock = threading.Lock()

    # -- host half

    def _submit(self, key):
        pool = self._pool()
        return {i: pool.submit(_decode_rgb, self.files[i]) for i in dict.fromkeys(key)}

    @staticmethod
    def _drop(job):
        for f in job.values():
            f.cancel()

    def announce(self, indices):
        key = tuple(int(i) for i in indices)
        with self.lock:
            if not key or key in self.pending:
                return
            while len(self.pending) >= len(self.ring):
                self._drop(self.pending.popitem(last=False)[1])
            self.pending[key] = self._submit(key)

    def collect(self, indices):
        """The decoded images of ``indices``, {index: array}; announced or not."""
        key = tuple(int(i) for i in indices)
        with self.lock:
            job = self.pending.pop(key, None)
        if job is None:
            job = self._submit(key)
        try:
            return key, {i: f.result() for i, f in job.items()}
        except BaseException:
            self._drop(job)
            raise

    def stage(self, indices):
        """Host half of a batch: ``(slot, nbytes, offsets [B] int64, sizes [B, 2] int32)``, the images packed into the host buffer
        of the next slot of the ring, every distinct index once."""
        key, images = self.collect(indices)
        at, total = {}, 0
        for i, a in images.items():
            at[i] = total
            total += a.size
        slot = self.ring[self.turn % len(self.ring)]
        self.turn += 1
        self._reserve(slot, total)
        host = slot.view(total)
        for i, a in images.items():
            host[at[i]:at[i] + a.size] = a.reshape(-1)
        offsets = np.asarray([at[i] for i in key], dtype=np.int64)
        sizes = np.asarray([images[i].shape[:2] for i in key], dtype=np.int32).reshape(len(key), 2)
        return slot, total, offsets, sizes

    def _reserve(self, slot, nbytes):
        """The slot's host buffer may be written: its last upload has completed, and it holds ``nbytes``."""
        if slot.uploaded is not None:
            slot.uploaded.synchronize()
        if slot.host is None or slot.host.numel() < nbytes:
            if slot.consumed is not None:
                slot.consumed.synchronize()
            cap = max(int(nbytes), 2 * (slot.host.numel() if slot.host is not None else 0), 1 << 16)
            slot.dev = None
            slot.host = torch.empty(cap, dtype=torch.uint8, pin_memory=torch.cuda.is_available())

    # -- device half: only ever called by the thread that composes the batch

    def upload(self, slot, nbytes, device):
        """The staged bytes on the device, ordered on the current stream behind the launch that last read this slot."""
        stream = torch.cuda.current_stream(device)
        if slot.consumed is not None and slot.stream != stream:
            stream.wait_event(slot.consumed)
        if slot.dev is None:
            slot.dev = torch.empty(slot.host.numel(), dtype=torch.uint8, device=device)
        if slot.uploaded is None:
            slot.uploaded, slot.consumed = torch.cuda.Event(), torch.cuda.Event()
        arena = slot.dev[:max(nbytes, 1)]
        arena.copy_(slot.host[:max(nbytes, 1)], non_blocking=True)
        slot.uploaded.record(stream)
        slot.stream = stream
        return arena

    def launched(self, slot):
        slot.consumed.record(slot.stream)

    # -- statistics

    def images(self):
        """The decoded images in file order, at most STATS_WINDOW of them in flight."""
        pool, futures = self._pool(), []
        try:
            for i in range(len(self.files) + self.STATS_WINDOW):
                if i < len(self.files):
                    futures.append(pool.submit(_decode_rgb, self.files[i]))
                if i >= self.STATS_WINDOW:
                    yield futures[i - self.STATS_WINDOW].result()
                    futures[i - self.STATS_WINDOW] = None
        finally:
            for f in futures:
                if f is not None:
                    f.cancel()


class FileDatasetGenerator(_GeneratorBase):
    """Base class of the file-based generators, with the reference's constructor arguments (datasets/common.py:129-162).

    ``cropsize`` is (width, height).  ``store_budget_bytes``: the largest decoded split the resident store accepts (default: 60 % of
    the device memory free when the split is decoded); ``dtype``: float32 or bfloat16 batches.  ``store``: 'resident' (a split over
    the budget is an error), 'stream' (no split is held; batches are decoded as they are composed) or 'auto' (per split: resident if
    it fits the budget, streamed if not).  ``prefetch_batches``: how many batches ahead a sequence announces to a streamed split;
    ``decode_threads``: the size of the decode pool (the module docstring has the streamed store's rules)."""

    def __init__(self, root_dir, cropsize=(224, 224), default_target_size=-1, randzoom_range=None, randrot_max=0,
                 distort_colors=False, colordistort_params={}, randerase_prob=0.0,
                 randerase_params={'sl': 0.02, 'sh': 0.4, 'r1': 0.3, 'r2': 1. / 0.3}, color_mode='rgb',
                 store_budget_bytes=None, dtype=torch.float32, seed=0, store='resident', prefetch_batches=2,
                 decode_threads=DECODE_THREADS):
        if distort_colors:
            raise NotImplementedError('distort_colors: colour distortion is not part of the device input pipeline '
                                      '(no preset of the reference turns it on)')
        if randrot_max > 0:
            raise NotImplementedError('randrot_max > 0: random rotation is not part of the device input pipeline '
                                      '(no preset of the reference turns it on)')
        if store not in ('resident', 'stream', 'auto'):
            raise ValueError("store=%r: 'resident', 'stream' or 'auto'" % (store,))
        self.store, self.prefetch_batches, self.decode_threads = store, int(prefetch_batches), int(decode_threads)
        self._decode_pool = None
        self.root_dir = root_dir
        self.cropsize = cropsize
        self.default_target_size = default_target_size
        self.randzoom_range = randzoom_range
        self.randrot_max, self.distort_colors, self.colordistort_params = randrot_max, distort_colors, colordistort_params
        self.randerase_prob = randerase_prob
        self.randerase_params = randerase_params
        self.color_mode = color_mode.lower()
        self.store_budget_bytes, self.dtype = store_budget_bytes, dtype
        self.rng = np.random.default_rng(seed)       # draws of compose_batch calls that bring no generator of their own
        self.classes = []
        self.train_img_files, self.test_img_files = [], []
        self._train_labels, self._test_labels = [], []
        self.train_repeats = 1
        self._mean = self._std = None
        self._stores = {}
        self._dev_stats = None

    # ---- the attribute interface of the reference ----

    y_train = property(lambda self: self._train_labels)
    y_test = property(lambda self: self._test_labels)
    num_channels = 3

    @property
    def mean(self):
        if self._mean is None:
            self._store(True, upload=False)
        return self._mean

    @property
    def std(self):
        if self._std is None:
            self._store(True, upload=False)
        return self._std

    def _compute_stats(self, mean=None, std=None):
        """Given statistics are stored; missing ones are computed with the training store (on first use, not here)."""
        self._mean = None if mean is None else np.asarray(mean, dtype=np.float32)
        self._std = None if std is None else np.asarray(std, dtype=np.float32)

    def _stats_from(self, images):
        """Channel mean / standard deviation of the training images, float64 on the host (datasets/common.py:186-207): the mean of
        the per-image means; the variance around the FLOAT32 mean, divided by N - 1.  Both sums run in file order."""
        if self._mean is None:
            mean = 0
            for img in images():
                mean += np.mean(np.asarray(img, dtype=np.float64), axis=(0, 1))
            self._mean = np.asarray(mean / len(self.train_img_files), dtype=np.float32)
        if self._std is None:
            var = 0
            for img in images():
                var += np.mean((np.asarray(img, dtype=np.float64) - self._mean) ** 2, axis=(0, 1))
            self._std = np.asarray(np.sqrt(var / (len(self.train_img_files) - 1)), dtype=np.float32)

    # ---- the store ----

    def _store(self, train, upload=True):
        key = bool(train)
        st = self._stores.get(key)
        if st is None:
            files = self.train_img_files if train else self.test_img_files
            st = self._stores[key] = self._stream(files) if self.store == 'stream' else self._decode(files)
            if train and (self._mean is None or self._std is None):
                self._stats_from(st.images)
        if (self._mean is None or self._std is None) and not train:
            self._store(True, upload=False)
        if upload and st.tier == 'resident' and st.device_arena is None:
            st.device_arena = torch.from_numpy(st.arena).to(self._dev())
            st.arena = None                      # the host copy has served its purpose
        return st

    def _pool(self):
        """The decode pool of the streamed splits, made at first use: at most 16 workers, whatever ``decode_threads`` asks for."""
        if self._decode_pool is None:
            self._decode_pool = ThreadPoolExecutor(max_workers=max(1, min(self.decode_threads, DECODE_THREADS)),
                                                   thread_name_prefix='sehip-decode')
        return self._decode_pool

    def _stream(self, files):
        return _StreamStore(files, self._pool, self.prefetch_batches)

    def prefetch(self, indices, train=True):
        """Announce a batch that a later ``compose_batch(indices, train)`` will ask for.  Only a streamed split that is already
        open starts decoding; every other split has its images at hand, and the call does nothing."""
        st = self._stores.get(bool(train))
        if st is not None and st.tier == 'stream':
            st.announce(indices)

    def _decode(self, files):
        from PIL import Image
        n = len(files)
        with ThreadPoolExecutor(max_workers=DECODE_THREADS) as pool:
            def size_of(fn):
                with Image.open(fn) as im:
                    return im.size
            wh = np.asarray(list(pool.map(size_of, files)), dtype=np.int64).reshape(n, 2)
            nbytes = wh[:, 0] * wh[:, 1] * 3
            offsets = np.concatenate(([0], np.cumsum(nbytes)[:-1])).astype(np.int64) if n else np.zeros(0, np.int64)
            total = int(nbytes.sum())
            budget = self.store_budget_bytes
            if budget is None and torch.cuda.is_available():
                budget = int(0.6 * torch.cuda.mem_get_info(self._dev())[0])
            if budget is not None and total > budget:
                if self.store == 'auto':         # the header pass has decided: this split streams
                    return self._stream(files)
                raise SehipError('the decoded images of this split take %d bytes, more than the store budget of %d bytes '
                                 '(store_budget_bytes; default: 60 %% of the free device memory)' % (total, budget))
            arena = np.empty(max(total, 1), dtype=np.uint8)

            def decode(i):
                with Image.open(files[i]) as im:
                    a = np.asarray(im.convert('RGB'), dtype=np.uint8)
                if a.shape != (wh[i, 1], wh[i, 0], 3):
                    raise SehipError('%s: decoded to %s, its header said %d x %d' % (files[i], a.shape, wh[i, 0], wh[i, 1]))
                arena[offsets[i]:offsets[i] + nbytes[i]] = a.reshape(-1)
            list(pool.map(decode, range(n)))
        return _Store(arena, offsets, np.ascontiguousarray(wh[:, ::-1]).astype(np.int32))

    # ---- augmentation parameters ----

    def draw_params(self, sizes, train=True, augment=False, rng=None, target_size=None):
        """Augmentation parameters of one batch, pure host code.  ``sizes`` [B, 2] = (h, w) of the stored images.  Returns a dict of
        arrays with one row per sample: ``size`` (H', W') of the zoomed image, ``flip``, ``erase`` (y, x, h, w) in the zoomed, flipped
        image (h == 0: none), ``seed`` uint32, ``offset`` (y, x) of the crop window and ``pad`` (y, x) of the reflect padding.

        Distributions of the reference (datasets/common.py:414-431, 456-470, 522-540): the target size is ``target_size`` or
        ``default_target_size`` -- an int is the shorter side, the other one ``round()``ed, -1 keeps the size; with ``augment`` an integer
        ``randzoom_range`` draws ``randint(lo, hi)`` for the shorter side and a float range multiplies the target size; flips with
        probability 1/2; erasing with probability ``randerase_prob``, area and aspect drawn until the rectangle fits; crop offset
        (or pad, where the image is smaller than the crop) ``randint(H' - ch + 1)``.  Without ``augment``: no zoom, flip or erase,
        centre crop.  ``train`` only names the split (the reference's sequences key every augmentation on ``augment``)."""
        rng = self.rng if rng is None else rng
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
        B = len(sizes)
        h, w = sizes[:, 0], sizes[:, 1]
        cw, ch = (int(v) for v in self.cropsize)
        ts = self.default_target_size if target_size is None else target_size
        zoom = augment and self.randzoom_range is not None
        # -- zoomed size
        if isinstance(ts, (tuple, list)):
            W, H = np.full(B, int(ts[0])), np.full(B, int(ts[1]))
            if zoom:
                raise NotImplementedError('random zoom with a (width, height) target size')
        elif ts > 0 or zoom:
            if zoom and isinstance(self.randzoom_range[0], float):
                f = rng.uniform(self.randzoom_range[0], self.randzoom_range[1], size=B)
                if ts > 0:
                    short = np.round(ts * f).astype(np.int64)
                else:
                    short = None
                    W, H = np.round(w * f).astype(np.int64), np.round(h * f).astype(np.int64)
            elif zoom:
                short = rng.integers(self.randzoom_range[0], self.randzoom_range[1], size=B)
            else:
                short = np.full(B, int(ts), dtype=np.int64)
            if short is not None:       # the shorter side is `short`, the other one round()ed (half to even, like Python's)
                tall = w < h
                W = np.where(tall, short, np.rint(w * (short / h)).astype(np.int64))
                H = np.where(tall, np.rint(h * (short / w)).astype(np.int64), short)
        else:
            W, H = w.copy(), h.copy()
        W, H = np.maximum(W, 1), np.maximum(H, 1)
        # -- flip, erase
        flip = rng.random(B) < 0.5 if augment else np.zeros(B, dtype=bool)
        erase = np.zeros((B, 4), dtype=np.int64)
        if augment and self.randerase_prob > 0:
            p = self.randerase_params
            for b in np.nonzero(rng.random(B) < self.randerase_prob)[0]:
                while True:
                    se = rng.uniform(p['sl'], p['sh']) * (H[b] * W[b])
                    re = rng.uniform(p['r1'], p['r2'])
                    he, we = int(np.sqrt(se * re)), int(np.sqrt(se / re))
                    if he < H[b] and we < W[b]:
                        break
                xe, ye = rng.integers(0, W[b] - we), rng.integers(0, H[b] - he)
                erase[b] = (ye, xe, he, we)
        seed = rng.integers(0, 2 ** 32, size=B, dtype=np.uint32)
        # -- crop window or reflect padding
        offset, pad = np.zeros((B, 2), dtype=np.int64), np.zeros((B, 2), dtype=np.int64)
        for axis, (D, c) in enumerate(((H, ch), (W, cw))):
            over, under = np.maximum(D - c, 0), np.maximum(c - D, 0)
            if augment:
                offset[:, axis] = rng.integers(0, over + 1)
                pad[:, axis] = rng.integers(0, under + 1)
            else:
                offset[:, axis], pad[:, axis] = over // 2, under // 2
        return {'size': np.stack((H, W), axis=1), 'flip': flip, 'erase': erase, 'seed': seed, 'offset': offset, 'pad': pad}

    # ---- batches ----

    def compose_batch(self, indices, train=True, augment=False, rng=None, target_size=None, params=None, return_params=False):
        """Batch of the images ``indices`` of the training / test split: [B, 3, ch, cw] channels_last on the device, composed in one
        kernel launch.  ``params``: parameters to use instead of drawing them (the dict of ``draw_params``)."""
        st = self._store(train)
        indices = np.asarray(indices, dtype=np.int64)
        crop = (int(self.cropsize[1]), int(self.cropsize[0]))
        if st.tier == 'stream':
            slot, nbytes, offsets, sizes = st.stage(indices)
            if params is None:
                params = self.draw_params(sizes, train, augment, rng, target_size)
            arena = st.upload(slot, nbytes, self._dev())
            X = compose_on_device(arena, offsets, sizes, params, crop, self._device_stats(), self.color_mode == 'bgr', self.dtype)
            st.launched(slot)
            return (X, params) if return_params else X
        sizes = st.sizes[indices]
        if params is None:
            params = self.draw_params(sizes, train, augment, rng, target_size)
        X = compose_on_device(st.device_arena, st.offsets[indices], sizes, params, crop, self._device_stats(),
                              self.color_mode == 'bgr', self.dtype)
        return (X, params) if return_params else X

    def _device_stats(self):
        if self._dev_stats is None:
            dev = self._dev()
            self._dev_stats = (torch.from_numpy(np.ascontiguousarray(self.mean, dtype=np.float32)).to(dev),
                               torch.from_numpy(np.ascontiguousarray(self.std, dtype=np.float32)).to(dev))
        return self._dev_stats

    def _sequence(self, train, batch_size, shuffle, augment, batch_transform, batch_transform_kwargs, target_size, repeats, dp):
        seed, rank = dp.get('seed', 0), dp.get('rank', 0)
        kwargs = {'rng': np.random.default_rng([int(train), rank, seed]), 'target_size': target_size}     # every rank its own draws
        labels = self._train_labels if train else self._test_labels
        return DeviceBatchSequence(self, np.arange(len(labels)), labels, batch_size, shuffle, train, augment, batch_transform,
                                   batch_transform_kwargs, repeats=repeats, compose_kwargs=kwargs, **dp)

    def train_sequence(self, batch_size=32, shuffle=True, target_size=None, augment=True, batch_transform=None, batch_transform_kwargs={}, **dp):
        return self._sequence(True, batch_size, shuffle, augment, batch_transform, batch_transform_kwargs, target_size, self.train_repeats, dp)

    def test_sequence(self, batch_size=32, shuffle=False, target_size=None, augment=False, batch_transform=None, batch_transform_kwargs={}, **dp):
        return self._sequence(False, batch_size, shuffle, augment, batch_transform, batch_transform_kwargs, target_size, 1, dp)

    def flow_train(self, batch_size=32, include_labels=True, shuffle=True, target_size=None, augment=True):
        for X, y in self._sequence(True, batch_size, shuffle, augment, None, {}, target_size, 1, {}):
            yield (X, y) if include_labels else X

    def flow_test(self, batch_size=32, include_labels=True, shuffle=False, target_size=None, augment=False):
        for X, y in self._sequence(False, batch_size, shuffle, augment, None, {}, target_size, 1, {}):
            yield (X, y) if include_labels else X


def pack_batch_tables(offsets, sizes, params, crop):
    """Everything ``se_image_batch`` reads for one batch, in ONE int32 host buffer (one upload): returns ``(buffer, views)`` with
    ``views`` = {name: (start, stop, shape)} in int32 elements; ``src_off`` comes first, so its int64 view is aligned."""
    B = len(offsets)
    xmap, xk, ymap, yk = sehip.resample_tables(sizes, params['size'], crop, params['offset'], params['pad'], params['flip'])
    parts = [('src_off', np.asarray(offsets, dtype=np.int64).view(np.int32), (B,)),
             ('src_hw', np.asarray(sizes, dtype=np.int32), (B, 2)),
             ('erase', np.asarray(params['erase'], dtype=np.int32), (B, 4)),
             ('seed', np.asarray(params['seed'], dtype=np.uint32).view(np.int32), (B,)),
             ('xmap', xmap, xmap.shape), ('xk', xk, xk.shape), ('ymap', ymap, ymap.shape), ('yk', yk, yk.shape)]
    buf = np.concatenate([a.reshape(-1) for _, a, _ in parts]) if B else np.zeros(0, np.int32)
    views, at = {}, 0
    for name, a, shape in parts:
        views[name] = (at, at + a.size, shape)
        at += a.size
    return buf, views


def compose_on_device(arena, offsets, sizes, params, crop, stats, bgr, dtype=torch.float32):
    """Tables of one batch -> one upload -> ``sehip.image_batch``.  ``crop`` = (ch, cw); ``stats`` = (mean, std) device tensors.
    Returns the batch as [B, 3, ch, cw] with channels_last strides."""
    buf, views = pack_batch_tables(offsets, sizes, params, crop)
    dbuf = torch.from_numpy(buf).to(arena.device)
    t = {}
    for name, (a, b, shape) in views.items():
        t[name] = dbuf[a:b].view(torch.int64) if name == 'src_off' else dbuf[a:b].view(shape)
    out = sehip.image_batch(arena, t['src_off'], t['src_hw'], t['xmap'], t['xk'], t['ymap'], t['yk'], t['erase'], t['seed'],
                            stats[0], stats[1], bgr=bgr, dtype=dtype)
    return out.permute(0, 3, 1, 2)


def _lines(path):
    with open(path) as f:
        return [l.strip() for l in f if l.strip() != '']


class NABGenerator(FileDatasetGenerator):
    """NABirds and CUB-200-2011 (reference: datasets/nab.py): ``images.txt`` (id, file name), ``image_class_labels.txt`` (id, label)
    and ``train_test_split.txt`` (id, 0 = test) under ``root_dir``; images in ``img_dir``; in the order of the image list."""

    def __init__(self, root_dir, classes=None, img_dir='images', img_list_file='images.txt', split_file='train_test_split.txt',
                 label_file='image_class_labels.txt', cropsize=(224, 224), default_target_size=256, randzoom_range=None,
                 distort_colors=False, randerase_prob=0.5, randerase_params=DEFAULT_ERASE_PARAMS,
                 mean=[125.30513277, 129.66606421, 118.45121113], std=[57.0045467, 56.70059436, 68.44430446], color_mode='rgb',
                 train_repeats=1, **store_kwargs):
        super(NABGenerator, self).__init__(root_dir, cropsize=cropsize, default_target_size=default_target_size,
                                           randzoom_range=randzoom_range, distort_colors=distort_colors,
                                           colordistort_params={'hue_delta': 0.0, 'saturation_range': (0.8, 1.2)},
                                           randerase_prob=randerase_prob, randerase_params=randerase_params, color_mode=color_mode,
                                           **store_kwargs)
        self.imgs_dir = os.path.join(root_dir, img_dir)
        self.img_list_file, self.label_file, self.split_file = (os.path.join(root_dir, f) for f in (img_list_file, label_file, split_file))
        self.train_repeats = train_repeats
        is_train = {i: flag != '0' for i, flag in (l.split() for l in _lines(self.split_file))}
        img_labels = {i: int(lbl) for i, lbl in (l.split() for l in _lines(self.label_file))}
        self.classes = classes if classes is not None else sorted(set(img_labels.values()))
        self.class_indices = dict(zip(self.classes, range(len(self.classes))))
        for img_id, fn in (l.split() for l in _lines(self.img_list_file)):
            if img_id in is_train and img_labels[img_id] in self.class_indices:
                files, labels = (self.train_img_files, self._train_labels) if is_train[img_id] else (self.test_img_files, self._test_labels)
                files.append(os.path.join(self.imgs_dir, fn))
                labels.append(self.class_indices[img_labels[img_id]])
        self._compute_stats(mean, std)


class SubDirectoryGenerator(FileDatasetGenerator):
    """Images in one sub-directory per class, two text files listing the training and the test images relative to ``img_dir``
    (reference: datasets/subdirectory.py; the presets mit67scenes, ucmlu and resisc45 use it)."""

    def __init__(self, root_dir, classes=None, img_dir='.', train_list='train.txt', test_list='test.txt', cropsize=(224, 224),
                 default_target_size=256, randzoom_range=None, randerase_prob=0.5, randerase_params=DEFAULT_ERASE_PARAMS,
                 mean=None, std=None, color_mode='rgb', **store_kwargs):
        super(SubDirectoryGenerator, self).__init__(root_dir, cropsize=cropsize, default_target_size=default_target_size,
                                                    randzoom_range=randzoom_range, randerase_prob=randerase_prob,
                                                    randerase_params=randerase_params, color_mode=color_mode, **store_kwargs)
        self.img_dir = img_dir if os.path.isabs(img_dir) else os.path.join(root_dir, img_dir)
        if classes is not None:
            self.classes = classes
        else:
            self.classes = sorted(os.path.basename(d) for d in glob(os.path.join(self.img_dir, '*'))
                                  if not os.path.basename(d).startswith('.') and os.path.isdir(d))
        self.class_indices = dict(zip(self.classes, range(len(self.classes))))
        for lst, files, labels in ((train_list, self.train_img_files, self._train_labels), (test_list, self.test_img_files, self._test_labels)):
            for rel in _lines(lst if os.path.isabs(lst) else os.path.join(root_dir, lst)):
                classname = os.path.dirname(rel)
                if classname in self.class_indices:
                    files.append(os.path.join(self.img_dir, rel))
                    labels.append(self.class_indices[classname])
        self._compute_stats(mean, std)


class CarsGenerator(FileDatasetGenerator):
    """Stanford Cars, merged training + test version (reference: datasets/cars.py): ``cars_annos.mat`` holds the structured array
    ``annotations`` with ``relative_im_path``, ``class`` (from 1) and ``test``."""

    def __init__(self, root_dir, classes=None, annotation_file='cars_annos.mat', cropsize=(448, 448), default_target_size=512,
                 randzoom_range=None, distort_colors=False, randerase_prob=0.5, randerase_params=DEFAULT_ERASE_PARAMS,
                 mean=[120.03730636, 117.33780928, 116.0130335], std=[75.40415763, 75.15394251, 77.28286728], color_mode='rgb',
                 **store_kwargs):
        import scipy.io
        super(CarsGenerator, self).__init__(root_dir, cropsize=cropsize, default_target_size=default_target_size,
                                            randzoom_range=randzoom_range, distort_colors=distort_colors, randerase_prob=randerase_prob,
                                            randerase_params=randerase_params, color_mode=color_mode, **store_kwargs)
        self.annotation_file = annotation_file if os.path.isabs(annotation_file) else os.path.join(root_dir, annotation_file)
        self._annotations = scipy.io.loadmat(self.annotation_file, squeeze_me=True)['annotations']
        self.classes = classes if classes is not None else sorted(set(self._annotations['class']))
        self.class_indices = dict(zip(self.classes, range(len(self.classes))))
        for sample in self._annotations:
            if sample['class'] in self.class_indices:
                fn = sample['relative_im_path']
                fn = fn if os.path.isabs(fn) else os.path.join(root_dir, fn)
                files, labels = (self.test_img_files, self._test_labels) if sample['test'] else (self.train_img_files, self._train_labels)
                files.append(fn)
                labels.append(self.class_indices[sample['class']])
        self._compute_stats(mean, std)


class FlowersGenerator(FileDatasetGenerator):
    """Oxford Flowers-102 (reference: datasets/flowers.py): ``imagelabels.mat`` (``labels``, from 1), ``setid.mat`` (arrays of image
    ids, from 1), images ``jpg/image_#####.jpg``.  Like the reference, every listed image's class must be among ``classes``."""

    def __init__(self, root_dir, classes=None, img_dir='jpg', label_file='imagelabels.mat', split_file='setid.mat',
                 train_splits=['trnid', 'valid'], test_splits=['tstid'], cropsize=(448, 448), default_target_size=512,
                 randzoom_range=None, distort_colors=False, randerase_prob=0.5, randerase_params=DEFAULT_ERASE_PARAMS,
                 mean=[110.7799141, 97.65648664, 75.32889973], std=[74.90387818, 62.70218863, 69.7656359], color_mode='rgb',
                 **store_kwargs):
        import scipy.io
        super(FlowersGenerator, self).__init__(root_dir, cropsize=cropsize, default_target_size=default_target_size,
                                               randzoom_range=randzoom_range, distort_colors=distort_colors,
                                               colordistort_params={'hue_delta': 0.0, 'saturation_range': (0.8, 1.2)},
                                               randerase_prob=randerase_prob, randerase_params=randerase_params, color_mode=color_mode,
                                               **store_kwargs)
        self.img_dir, self.label_file, self.split_file = (f if os.path.isabs(f) else os.path.join(root_dir, f)
                                                          for f in (img_dir, label_file, split_file))
        img_labels = scipy.io.loadmat(self.label_file, squeeze_me=True)['labels']
        splits = scipy.io.loadmat(self.split_file, squeeze_me=True)
        self.classes = classes if classes is not None else sorted(set(img_labels))
        self.class_indices = dict(zip(self.classes, range(len(self.classes))))
        for names, files, labels in ((train_splits, self.train_img_files, self._train_labels), (test_splits, self.test_img_files, self._test_labels)):
            for name in names:
                for i in np.atleast_1d(splits[name]):
                    files.append(os.path.join(self.img_dir, 'image_{:05d}.jpg'.format(i)))
                    labels.append(self.class_indices[img_labels[i - 1]])
        self._compute_stats(mean, std)
