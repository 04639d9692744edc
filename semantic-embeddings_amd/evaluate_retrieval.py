"""Drop-in for the reference's ``evaluate_retrieval.py`` (same CLI flags, same
``pairwise_retrieval`` signature and return convention), with the all-pairs distance + ranking
executed by the MI355X kernels of libsehip.so instead of NumPy/OpenBLAS/numexpr on the host.

reference: evaluate_retrieval.py:22-73 (pairwise_retrieval), :76-151 (reporting helpers),
:155-208 (CLI).  Differences a user can observe:

* ties in the ranking come back in canonical (distance, index) order -- the reference's
  ``np.argsort`` is unstable and returns them in arbitrary order;
* the ranking is produced query tile by query tile (the generator is genuinely lazy), so the
  N x N distance matrix never has to exist at once;
* there is no CPU fallback: without a ROCm device the call raises ``sehip.SehipError``;
* launched with one process per GPU (``python -m torch.distributed.run --nproc-per-node G evaluate_retrieval.py ...``)
  the queries are sharded across the ranks (gallery replicated, rows of a ranking are independent) and the per-query
  metrics are combined with one small all-reduce; rank 0 prints / writes / plots;
* ``--skip_ap`` (extension) drops the average-precision column; together with ``--clip_ahp`` no metric needs more than the
  head of each ranking, and under several ranks the SHARDED-GALLERY path is taken: per-shard fused distance + top-k,
  RCCL all-gather of the per-shard lists, k-way merge;
* ``--gallery_feat FILE`` (extension, with ``--gallery_split``): the --feat file at the same position holds QUERIES against this
  gallery -- held-out images against a database.  The gallery is never ranked in full: P@k / AHP@K read fused top-k lists
  (``--clip_ahp`` is required), AP counts the gallery items in front of every relevant one (``se_count_preceding``);
* ``--rank_gallery`` (extension, with ``--gallery_feat``): every query's row IS ranked against the whole gallery, tile of queries
  by tile, and every metric is read from that one ranking -- the whole-list ``AHP (WUP)`` / ``AHP (LCS_HEIGHT)`` columns the
  reference prints by default included, so ``--clip_ahp`` is no longer required (8 bytes per query and gallery item pass through
  device memory: meant for galleries of CIFAR / CUB / NABirds / Cars size);
* ``--float64`` (extension; ``pairwise_retrieval(..., precision='float64')``): float64 feature files are evaluated in float64 like the
  reference does -- float64 distances from one sequential FMA chain (``se_pairwise_dist_f64``), ranked exactly (``se_rank_rows`` on
  their float32 image, then ``se_rank_refine_f64``) -- instead of being cast to float32 behind a warning.  All-pairs, one process
  only: ``--gallery_feat`` / ``--rank_gallery`` and the sharded multi-GPU evaluation stay float32 and refuse the flag;
* ``--bootstrap R`` (extension; ``bootstrap.py``): below the table of means, ``mean [lo, hi]`` percentile intervals of the printed
  columns from R resamples of the queries (``se_bootstrap_means``; ``--bootstrap_seed``, ``--confidence``), with ``--compare_to LABEL``
  the paired difference ``delta [lo, hi] p=...`` of every other entry to that one, and ``--bootstrap_csv FILE``.  One process only.
* ``--ndcg K [K ...]`` (extension; ``se_ndcg``): ``NDCG@K (WUP)`` / ``NDCG@K (LCS_HEIGHT)`` columns behind the others -- discounted
  cumulative gain with the class similarities as gains and ``1 / log2(position + 1)`` as weights over that of the ideal ranking of
  the gallery -- and, for ``K = 0``, the whole-list ``NDCG (...)`` columns (whole rankings: with ``--gallery_feat`` pass
  ``--rank_gallery``).  Read from the same rank tiles; part of the ``--bootstrap`` output; ``--csv`` and the plots are unchanged.
"""
import argparse
import os.path
import pickle
import warnings
from collections import OrderedDict

import numpy as np

import bootstrap

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    def tqdm(it, **kwargs):
        return it


METRICS = ['P@1 (WUP)', 'P@10 (WUP)', 'P@50 (WUP)', 'P@100 (WUP)', 'AHP (WUP)',
           'P@1 (LCS_HEIGHT)', 'P@10 (LCS_HEIGHT)', 'P@50 (LCS_HEIGHT)', 'P@100 (LCS_HEIGHT)', 'AHP (LCS_HEIGHT)', 'AP']

# rows of the distance matrix ranked per launch group; bounds device memory to ~8 B x TILE x N
DEFAULT_TILE_BYTES = 4 << 30


def _as_feature_matrix(features):
    """Input normalisation of evaluate_retrieval.py:43-54: path | dict | {'feat': dict} | ndarray."""
    if isinstance(features, str):
        with open(features, 'rb') as feat_dump:
            features = pickle.load(feat_dump)
    if isinstance(features, dict):
        if 'feat' in features:
            features = features['feat']
        ind2id = np.array(list(features.keys()))
        features = np.stack(list(features.values()))
        if features.ndim > 2:
            raise ValueError('Feature matrix must be 2-dimensional. Actual shape: {}'.format(features.shape))
        owned = True
    else:
        ind2id = None
        owned = False
    return features, ind2id, owned


def host_blas_kblocks(d, q=448):
    """K-block list of OpenBLAS's level-3 drivers for a depth-``d`` product (GEMM_Q = ``q``; 448 for the Haswell / SkylakeX /
    Zen sgemm kernels): blocks of ``q`` while at least ``2 q`` remain, then the remainder split in two (first half rounded up)
    if it exceeds ``q``.  The reference's ``np.dot`` (evaluate_retrieval.py:59,62) restarts its fp32 FMA chain at every block,
    so for D > 448 bit-identical rankings need this list: ``pairwise_retrieval(..., kblocks=host_blas_kblocks(D))``.
    Verified against this image's NumPy/OpenBLAS for D up to 2048 (oracle/make_golden.py probes it for the fixtures)."""
    out, ls = [], 0
    while ls < d:
        m = d - ls
        if m >= 2 * q:
            m = q
        elif m > q:
            m = (m + 1) // 2
        out.append(m)
        ls += m
    return out


def _resolve_kblocks(kblocks, d, warn=True):
    if kblocks is not None and not isinstance(kblocks, str) and len(kblocks) == 0:
        return None            # "already resolved to a single chain" (pairwise_retrieval -> ranking_tiles): no second warning
    if kblocks is None:
        if warn and d > 448:
            warnings.warn("D = {} > 448: the reference's np.dot (evaluate_retrieval.py:59,62) restarts its float32 FMA chain per BLAS "
                          "K block; with kblocks=None distances come from ONE chain and near-tie orders can differ from the "
                          "reference's.  Pass kblocks='openblas' (CLI: --kblocks openblas) for bit-identical rankings."
                          .format(d), stacklevel=3)
        return None
    if isinstance(kblocks, str):
        if kblocks.lower() != 'openblas':
            raise ValueError("kblocks must be None, 'openblas' or a list of block lengths summing to D")
        kblocks = host_blas_kblocks(d)
    kblocks = [int(v) for v in kblocks]
    if sum(kblocks) != d or min(kblocks) <= 0:
        raise ValueError('kblocks {} do not add up to the feature dimension {}'.format(kblocks, d))
    return kblocks if len(kblocks) > 1 else None


_tile_cache = {}   # device index -> {'pd': flat uint8 tensor, 'rk': flat uint8 tensor}: grow-only distance / rank buffers of ranking_tiles


def release_tile_cache(device=None):
    """Drop the cached distance / rank buffers of ``ranking_tiles`` (one device, default: all).  They are grow-only and live for the
    process: 2 x 10 GB after a 50,000-item all-pairs evaluation."""
    if device is None:
        _tile_cache.clear()
    else:
        from sehip.ops import _device_index
        _tile_cache.pop(_device_index(device), None)


def _cached_rows(kind, rows, n, dtype, device):
    """``[rows, n]`` view (row pitch a multiple of 16 bytes, like ``sehip.empty_rows``) of the device's grow-only cached buffer
    ``kind``: a second evaluation in the same process -- the CLI loops over its --feat files -- pays no 10 GB allocation."""
    import torch
    from sehip.ops import _device_index, row_pitch
    pitch = row_pitch(n, dtype)
    need = rows * pitch * torch.empty((), dtype=dtype).element_size()
    slot = _tile_cache.setdefault(_device_index(device), {})
    buf = slot.get(kind)
    if buf is None or buf.numel() < need:
        slot.pop(kind, None)
        buf = None                        # free the old buffer before the larger one is allocated
        buf = torch.empty((max(need, 16),), dtype=torch.uint8, device=device)
        slot[kind] = buf
    mat = buf[:need].view(dtype).view(rows, pitch)
    return mat if pitch == n else mat[:, :n]


RANKING_KERNELS = ('normalize_rows_', 'row_sqnorm', 'pairwise_dist', 'rank_rows')


def _native_pairwise_dist(a, b, cosine, sqa, sqb, kblocks, out=None):
    import sehip
    return sehip.pairwise_dist(a, b, metric=sehip.METRIC_COSINE if cosine else sehip.METRIC_EUCLID, sqa=sqa, sqb=sqb, kblocks=kblocks, out=out)


F64_RANKING_KERNELS = ('pairwise_dist_f64', 'rank_rows_f64')


def _native_pairwise_dist_f64(a, b, cosine, sqa, sqb, out=None, img=True):
    import sehip
    return sehip.pairwise_dist_f64(a, b, metric=sehip.METRIC_COSINE if cosine else sehip.METRIC_EUCLID, sqa=sqa, sqb=sqb, out=out, img=img)


def is_float64(precision):
    """``precision`` of the retrieval entry points: None (the float32 kernels) or 'float64' (float64 distances, ranked exactly)."""
    if precision not in (None, 'float64'):
        raise ValueError("precision must be None or 'float64', not {!r}".format(precision))
    return precision == 'float64'


def host_normalize_f64(features):
    """The reference's own line (evaluate_retrieval.py:58) on a float64 matrix: float64-identical to it by construction."""
    return features / np.linalg.norm(features, axis=-1, keepdims=True)


def host_sqnorm_f64(features):
    """``np.sum(features ** 2, axis = -1)`` (evaluate_retrieval.py:61) on a float64 matrix."""
    return np.sum(features ** 2, axis=-1)


def to_device_f64(x, dev):
    """The float64 feature matrix ``x`` (array or tensor) as a device tensor of its own; anything but float64 raises: upcasting
    would compute something the reference never does."""
    import torch
    if (x.dtype != torch.float64) if torch.is_tensor(x) else (not isinstance(x, np.ndarray) or x.dtype != np.float64):
        raise ValueError("precision='float64' takes float64 features, got {}: float32 features are what the float32 kernels "
                         "(precision=None) rank bit for bit like the reference".format(getattr(x, 'dtype', type(x).__name__)))
    if torch.is_tensor(x):
        return x.detach().to(device=dev).contiguous().clone()
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def resolve_kernels(kernels, names):
    """``kernels`` (None, or the CPU stand-ins of the tests) as a new dict in which every one of ``names`` it lacks is the native
    one: the ``sehip`` function of that name, ``pairwise_dist(a, b, cosine, sqa, sqb, kblocks, out)`` the one adapter of
    ``sehip.pairwise_dist``, ``'ranking_tiles'`` the generator of this module and ``'device'`` the current ROCm device (a
    ``torch.device`` either way).  Nothing but ``names`` is looked up."""
    kernels = dict(kernels or {})
    if 'device' in names:
        import torch
        kernels['device'] = torch.device(kernels.get('device') or torch.device('cuda', torch.cuda.current_device()))
    own = {'pairwise_dist': _native_pairwise_dist, 'pairwise_dist_f64': _native_pairwise_dist_f64, 'ranking_tiles': ranking_tiles}
    for k in names:
        if k not in kernels and k in own:
            kernels[k] = own[k]
        elif k not in kernels:
            import sehip
            kernels[k] = getattr(sehip, k)
    return kernels


def ranking_tiles(features, normalize=False, tile_rows=None, idx64=False, queries=None, kblocks=None, whole_if_fits=True,
                  prenormalized=False, idx16=False, gallery=None, kernels=None, precision=None):
    """Generator over ``(first_row, rank_tile)`` with ``rank_tile`` an int32 (int64 if ``idx64``)
    DEVICE tensor ``[rows, N]``: the canonical ranking of queries ``first_row .. first_row+rows``.
    **A tile is valid until the next one is drawn**: the tiles of one iteration share one distance and one rank buffer.  Without a
    ``gallery`` these are the grow-only per-device buffers of the process-wide tile cache, which every later call reuses
    (``release_tile_cache`` frees them); with one they belong to the iteration (below).

    ``features`` must already be a float32 device tensor ``[N, D]``; it is normalised in place when
    ``normalize`` is set (like the reference mutates its input, evaluate_retrieval.py:58).
    (``prenormalized``: the caller already did that -- normalising twice would change bits.)
    ``queries`` optionally restricts the query rows to ``range(*queries)``; ``kblocks`` (None | 'openblas' | list) makes
    the FMA chain restart per K block like the host BLAS the reference ran on (see ``host_blas_kblocks``).
    ``idx16``: uint16 ranks as an int16 tensor (galleries of at most 53,248 items; what ``hierarchical_precision_device`` asks
    for: half the bytes between the ranking and the metric kernel).
    ``whole_if_fits`` (default since round 6): rank all queries as ONE tile when distances + ranks (8 N^2 bytes) fit into a third of
    the device memory that is free or already held by the tile cache -- all-pairs then takes the symmetric distance kernel
    (3.2 instead of 5.4 ms at 50k x 50k), i.e. the kernels bench.py times.  The first call on a device pays for the two
    allocations once (0.24 s for 2 x 10 GB); with the cache later evaluations do not.

    ``gallery`` (float32 device tensor ``[G, D]``): the rectangular variant -- the rows of ``features`` are QUERIES, every tile is
    the canonical ranking ``[rows, G]`` (int32) of ``rows`` of them against the whole gallery, with the same (distance, index) order
    and the same ``kblocks`` chain as the square one; ``queries`` restricts the query rows, ``normalize`` normalises both operands
    in place.  The two buffers are this iteration's own -- the process-wide cache is not used, so a tile a caller keeps is not
    touched again once the iteration has ended.  ``tile_rows`` defaults to ``DEFAULT_TILE_BYTES`` worth of rows
    (``hierarchical_precision_device(..., rank_gallery=True)`` sizes it from the free device memory instead); ``idx64`` / ``idx16`` /
    ``whole_if_fits`` do not apply.  ``kernels`` (tests): CPU stand-ins ``{'normalize_rows_', 'row_sqnorm', 'pairwise_dist',
    'rank_rows'}``.

    ``precision='float64'`` (opt-in): ``features`` is a float64 device tensor and every tile is the canonical ranking of FLOAT64
    distances -- ``se_pairwise_dist_f64`` (one sequential float64 FMA chain; ``kblocks`` does not apply and must be None), ``se_rank_rows``
    on the float32 image, ``se_rank_refine_f64`` on the runs of equal images.  Rows are normalised / their square norms taken on the
    host with the reference's NumPy lines (N x D: nothing next to N x N).  A tile row holds 8 + 4 bytes per pair next to its ranks,
    which the tile size accounts for.  All-pairs only (``gallery`` raises), int32 or int64 ranks (``idx16`` raises).
    ``kernels`` (tests): ``{'pairwise_dist_f64', 'rank_rows_f64'}``."""
    if is_float64(precision):
        if gallery is not None or idx16:
            raise ValueError("precision='float64' ranks all pairs of one feature matrix into int32 / int64 ranks: a separate gallery "
                             "and 16-bit ranks stay float32")
        if kblocks is not None and len(kblocks):
            raise ValueError("precision='float64' computes ONE float64 FMA chain per distance: kblocks does not apply")
        return _ranking_tiles_f64(features, normalize, tile_rows, idx64, queries, whole_if_fits, prenormalized, kernels)
    return _ranking_tiles_f32(features, normalize, tile_rows, idx64, queries, kblocks, whole_if_fits, prenormalized, idx16, gallery, kernels)


def _ranking_tiles_f32(features, normalize, tile_rows, idx64, queries, kblocks, whole_if_fits, prenormalized, idx16, gallery, kernels):
    """The generator of ``ranking_tiles`` for the float32 kernels."""
    all_pairs = gallery is None
    if not all_pairs and (idx64 or idx16):
        raise ValueError('ranking_tiles(..., gallery=...) writes int32 ranks')
    kernels = resolve_kernels(kernels, RANKING_KERNELS)
    if all_pairs:
        gallery = features
    nq, d = features.shape
    n = int(gallery.shape[0])
    if int(gallery.shape[1]) != int(d):
        raise ValueError('queries have {} feature dimensions, the gallery {}'.format(d, gallery.shape[1]))
    kblocks = _resolve_kblocks(kblocks, d)
    if normalize:
        if not prenormalized:
            kernels['normalize_rows_'](features)
            if not all_pairs:
                kernels['normalize_rows_'](gallery)
        sq_q = sq_g = None
    else:
        sq_q = kernels['row_sqnorm'](features)
        sq_g = sq_q if all_pairs else kernels['row_sqnorm'](gallery)
    q0, q1 = (0, nq) if queries is None else queries
    if tile_rows is None:
        tile_rows = max(128, min(nq, (DEFAULT_TILE_BYTES // (8 * max(n, 1))) // 128 * 128))
        if whole_if_fits and all_pairs and features.is_cuda:
            # distances + ranks of all queries, plus what the ranking will ask of the (grow-only) workspace cache on top of what that
            # cache already holds -- up to ~3 GB for rows above 53,248 columns
            import torch
            import sehip
            extra_ws = max(0, sehip.rank_rows_workspace_bytes(q1 - q0, n) - sehip.workspace_bytes(features.device))
            held = sum(int(b.numel()) for b in _tile_cache.get(sehip.ops._device_index(features.device), {}).values())
            need = (4 + (2 if idx16 else (8 if idx64 else 4))) * n * (q1 - q0)
            if need + extra_ws <= (torch.cuda.mem_get_info(features.device)[0] + held) // 3:
                tile_rows = max(tile_rows, q1 - q0)
    tile_rows = max(1, int(tile_rows))
    pd = rk = None          # (CPU stand-ins of the tests allocate their own results)
    if features.is_cuda and q1 > q0:
        import torch
        import sehip
        rows_max, rk_dtype = min(tile_rows, q1 - q0), torch.int16 if idx16 else (torch.int64 if idx64 else torch.int32)
        if all_pairs:
            pd = _cached_rows('pd', rows_max, n, torch.float32, features.device)
            rk = _cached_rows('rk', rows_max, n, rk_dtype, features.device)
        else:
            pd = sehip.empty_rows(rows_max, n, torch.float32, features.device)
            rk = sehip.empty_rows(rows_max, n, rk_dtype, features.device)
    for r0 in range(q0, q1, tile_rows):
        rows = min(tile_rows, q1 - r0)
        dist = kernels['pairwise_dist'](features[r0:r0 + rows], gallery, normalize, None if sq_q is None else sq_q[r0:r0 + rows], sq_g,
                                        kblocks, None if pd is None else pd[:rows])
        yield r0, (kernels['rank_rows'](dist) if rk is None else kernels['rank_rows'](dist, out=rk[:rows]))


def _ranking_tiles_f64(features, normalize, tile_rows, idx64, queries, whole_if_fits, prenormalized, kernels):
    """The generator of ``ranking_tiles(..., precision='float64')``."""
    import torch
    if not torch.is_tensor(features) or features.dtype != torch.float64:
        raise ValueError("precision='float64' takes a float64 tensor [N, D]")
    kernels = resolve_kernels(kernels, F64_RANKING_KERNELS)
    n, d = features.shape
    sq = None
    if normalize and not prenormalized:
        features.copy_(torch.from_numpy(host_normalize_f64(features.cpu().numpy())))
    elif not normalize:
        sq = torch.from_numpy(host_sqnorm_f64(features.cpu().numpy())).to(features.device)
    q0, q1 = (0, n) if queries is None else queries
    pair_bytes = 8 + 4 + (8 if idx64 else 4)       # float64 distance, float32 image, rank
    if tile_rows is None:
        tile_rows = max(128, min(n, (DEFAULT_TILE_BYTES // (pair_bytes * max(n, 1))) // 128 * 128))
        if whole_if_fits and features.is_cuda:
            import sehip
            ws = max(sehip.rank_rows_workspace_bytes(q1 - q0, n), sehip._lib.call('se_rank_refine_f64_workspace_bytes', q1 - q0, n))
            extra_ws = max(0, ws - sehip.workspace_bytes(features.device))
            held = sum(int(b.numel()) for b in _tile_cache.get(sehip.ops._device_index(features.device), {}).values())
            if pair_bytes * n * (q1 - q0) + extra_ws <= (torch.cuda.mem_get_info(features.device)[0] + held) // 3:
                tile_rows = max(tile_rows, q1 - q0)
    tile_rows = max(1, int(tile_rows))
    pd = im = rk = None          # (CPU stand-ins of the tests allocate their own results)
    if features.is_cuda and q1 > q0:
        rows_max = min(tile_rows, q1 - q0)
        pd = _cached_rows('pd64', rows_max, n, torch.float64, features.device)
        im = _cached_rows('pd', rows_max, n, torch.float32, features.device)
        rk = _cached_rows('rk', rows_max, n, torch.int64 if idx64 else torch.int32, features.device)
    for r0 in range(q0, q1, tile_rows):
        rows = min(tile_rows, q1 - r0)
        dist, image = kernels['pairwise_dist_f64'](features[r0:r0 + rows], features, normalize, None if sq is None else sq[r0:r0 + rows], sq,
                                                   None if pd is None else pd[:rows], True if im is None else im[:rows])
        yield r0, (kernels['rank_rows_f64'](dist, image, idx64=idx64) if rk is None else kernels['rank_rows_f64'](dist, image, out=rk[:rows]))


def pairwise_retrieval(features, normalize=False, return_generator=True, kblocks=None, precision=None):
    """ Uses each image as query and retrieves its nearest neighbors.

    # Arguments (identical to the reference, evaluate_retrieval.py:22-41):

    - features: 2-d numpy array | dict id -> feature vector | dict with key 'feat' | path to a pickle of those.
    - normalize: Whether to L2-normalize the features.
    - return_generator: If True, a generator will be returned instead of a dictionary.
    - kblocks (extension): None | 'openblas' | list -- K-block list of the host BLAS to reproduce for D > 448.
    - precision (extension): None -- the float32 kernels (float64 features are cast, with a warning); 'float64' -- float64 features
      only (float32 ones raise ``ValueError``): float64 distances from one sequential FMA chain, ranked exactly (DESIGN.md section
      3.1), the reference's computation for such features.  ``kblocks`` does not apply.

    # Returns:
        generator (or dict) of ``(image ID, list of all image IDs ordered by increasing distance)``.
    """
    import torch
    import sehip  # raises SehipError if the HIP library is missing -- no CPU fallback

    features, ind2id, owned = _as_feature_matrix(features)
    if is_float64(precision):
        return _pairwise_retrieval_f64(features, ind2id, normalize, return_generator, kblocks)
    if isinstance(features, np.ndarray) and features.dtype == np.float64:
        # the reference computes in the caller's dtype (evaluate_retrieval.py:57-67): float64 features give float64 distances and
        # their ranking.  The kernels are float32 (the dtype of every feature dump the reference writes,
        # learn_image_embeddings.py:270-275): say so instead of casting silently.
        warnings.warn("pairwise_retrieval: float64 features are ranked in float32 here (the reference would compute float64 distances); "
                      "orders can differ where float32 rounding creates or breaks near-ties.  Feature dumps of the reference are float32.",
                      RuntimeWarning, stacklevel=2)
    feats_h = np.ascontiguousarray(features, dtype=np.float32)
    sehip._lib.require_gpu()
    dev = torch.from_numpy(feats_h).cuda()
    kblocks = _resolve_kblocks(kblocks, feats_h.shape[1])
    if normalize:
        # like the reference (`features /= np.linalg.norm(...)`, evaluate_retrieval.py:58) the caller's array is normalised
        # in place at CALL time, before the first ranking is drawn from the generator
        sehip.normalize_rows_(dev)
        if not owned and isinstance(features, np.ndarray) and features.dtype == np.float32:
            np.copyto(features, dev.cpu().numpy())

    g = _ranked_ids(ranking_tiles(dev, normalize, kblocks=kblocks or (), prenormalized=True), ind2id)
    return g if return_generator else dict(g)


def _ranked_ids(tiles, ind2id):
    """``(image ID, list of all image IDs ordered by increasing distance)`` for every row of every ranking tile."""
    for r0, tile in tiles:
        ranks = tile.cpu().numpy()
        for i in range(ranks.shape[0]):
            ret = ranks[i]
            if ind2id is not None:
                yield ind2id[r0 + i], ind2id[ret].tolist()
            else:
                yield r0 + i, ret.tolist()


def _pairwise_retrieval_f64(features, ind2id, normalize, return_generator, kblocks):
    """``pairwise_retrieval(..., precision='float64')``: the checks and the host normalisation come before the GPU is asked for."""
    import torch
    import sehip
    if not isinstance(features, np.ndarray) or features.dtype != np.float64:
        raise ValueError("precision='float64' takes float64 features, got {}: float32 features are what the float32 kernels "
                         "(precision=None) rank bit for bit like the reference".format(getattr(features, 'dtype', type(features).__name__)))
    if kblocks is not None:
        raise ValueError("precision='float64' computes ONE float64 FMA chain per distance: kblocks does not apply")
    if features.ndim != 2:
        raise ValueError('Feature matrix must be 2-dimensional. Actual shape: {}'.format(features.shape))
    if normalize:
        # the reference's line, on the caller's array like the reference (`features /= ...`, evaluate_retrieval.py:58)
        features /= np.linalg.norm(features, axis=-1, keepdims=True)
    sehip._lib.require_gpu()
    dev = torch.from_numpy(np.ascontiguousarray(features)).cuda()
    g = _ranked_ids(ranking_tiles(dev, normalize, prenormalized=True, precision='float64'), ind2id)
    return g if return_generator else dict(g)


def print_performance(perf, metrics=METRICS):
    """Console table: one row per feature file, one column per metric (4 decimals)."""
    name_w = max(map(len, perf))
    col_w = [max(len(m), 6) for m in metrics]
    header = [' ' * name_w] + [m.center(6) for m in metrics]
    print('\n' + ' | '.join(header))
    print('-' * (name_w + sum(3 + w for w in col_w)))
    for name, res in perf.items():
        cells = ['%*.4f' % (w, res[m]) for m, w in zip(metrics, col_w)]
        print(' | '.join([name.ljust(name_w)] + cells))
    print()


def write_performance(perf, csv_file, prec_type='LCS_HEIGHT'):
    """Semicolon-separated P@k table, k = 1.. as long as every result has that cut-off."""
    names = list(perf)
    lines = ['k;' + ';'.join(names)]
    k = 1
    while all('P@%d (%s)' % (k, prec_type) in perf[n] for n in names):
        lines.append(';'.join([str(k)] + [str(perf[n]['P@%d (%s)' % (k, prec_type)]) for n in names]))
        k += 1
    with open(csv_file, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def plot_performance(perf, kmax=100, prec_type='LCS_HEIGHT', clip_ahp=None):
    """Figure 1: hierarchical precision@k curves; figure 2: (clipped) mAHP as horizontal bars."""
    import matplotlib.pyplot as plt

    ks = np.arange(1, kmax + 1)
    fig1, ax = plt.subplots()
    lowest = 1.0
    for name, res in perf.items():
        curve = np.array([res['P@%d (%s)' % (k, prec_type)] for k in ks])
        ax.plot(ks, curve, label=name)
        lowest = min(lowest, float(curve.min()))
    floor = np.floor(lowest * 20) / 20
    ax.set(xlabel='k', ylabel='Hierarchical Precision', xlim=(0, kmax), ylim=(floor if floor >= 0.3 else 0, 1))
    ax.grid(True)
    ax.legend(fontsize='x-small')

    key = 'AHP%s (%s)' % ('@%d' % clip_ahp if clip_ahp else '', prec_type)
    fig2, ax = plt.subplots()
    for pos, (name, res) in enumerate(perf.items()):
        ax.barh(pos + 0.5, res[key], 0.8)
        ax.text(0.01, pos + 0.5, name, va='center', ha='left', color='white', fontsize='small')
        ax.text(res[key] - 0.01, pos + 0.5, '{:.1%}'.format(res[key]), va='center', ha='right', color='white')
    ax.set(xlabel='Mean Average Hierarchical Precision', yticks=[])
    ax.grid(axis='x')
    plt.show()


def str2bool(v):
    """argparse type for the --norm flag: yes/true/t/y/1 and no/false/f/n/0 (case-insensitive)."""
    word = v.lower()
    if word in ('yes', 'true', 't', 'y', '1'):
        return True
    if word in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def build_parser():
    """Same flags, defaults and grouping as the reference CLI (evaluate_retrieval.py:157-174)."""
    p = argparse.ArgumentParser(description='Hierarchical-precision evaluation of nearest-neighbour image retrieval (MI355X kernels).',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = p.add_argument_group('Dataset')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--hierarchy', type=str, required=True, help='Text file with one "<parent> <child>" pair per line.')
    g.add_argument('--is_a', action='store_true', default=False, help='Lines of --hierarchy are "<child> <parent>" instead.')
    g.add_argument('--str_ids', action='store_true', default=False, help='Class IDs are strings (default: integers).')
    g.add_argument('--classes_from', type=str, default=None, help='Pickle with an "ind2label" item restricting/ordering the classes.')
    g = p.add_argument_group('Features')
    g.add_argument('--feat', type=str, action='append', required=True, help='Feature pickle {"feat": {image id: vector}}; repeatable.')
    g.add_argument('--label', type=str, action='append', help='Display name for the matching --feat.')
    g.add_argument('--norm', type=str2bool, action='append', help='L2-normalise the matching --feat (cosine ranking); default no.')
    g = p.add_argument_group('Output')
    g.add_argument('--plot_max', type=int, default=250, help='Largest k of the precision curve; 0 disables plotting.')
    g.add_argument('--prec_type', type=str, default='LCS_HEIGHT', choices=['WUP', 'LCS_HEIGHT'], help='Class-similarity measure for the curve/CSV.')
    g.add_argument('--clip_ahp', type=int, default=None, help='Compute AHP on the first CLIP_AHP ranks only.')
    g.add_argument('--csv', type=str, default=None, help='Write the P@k table to this CSV file.')
    g = p.add_argument_group('Extensions of this build (not in the reference)')
    g.add_argument('--skip_ap', action='store_true', default=False,
                   help='Do not compute AP; with --clip_ahp only the head of each ranking is needed (sharded-gallery top-k under several ranks).')
    g.add_argument('--kblocks', type=str, default=None, help="'openblas': restart the fp32 dot-product chain per OpenBLAS K block (D > 448).")
    add_float64_flag(g)
    add_gallery_flags(g)
    # (absent from the namespace unless given -- a run without it parses to exactly what it did before the flag existed)
    g.add_argument('--rank_gallery', action='store_true', default=argparse.SUPPRESS,
                   help='With --gallery_feat: rank every query against the WHOLE gallery and read every metric off that ranking; '
                        'gives the un-clipped AHP columns, so --clip_ahp is not required (with it, AHP@K comes from the same ranking).')
    add_ndcg_flag(g)
    bootstrap.add_bootstrap_flags(g)
    return p


def _ndcg_cutoff(v):
    k = int(v)
    if k < 0:
        raise argparse.ArgumentTypeError('NDCG cut-offs are integers >= 0 (0: the whole list), got %r' % v)
    return k


def add_ndcg_flag(group):
    """--ndcg of evaluate_retrieval.py and evaluate_rankings.py (absent from the namespace unless given, like --rank_gallery)."""
    group.add_argument('--ndcg', type=_ndcg_cutoff, nargs='+', default=argparse.SUPPRESS, metavar='K',
                       help='Also report NDCG@K (WUP / LCS_HEIGHT): discounted cumulative gain with the class similarities as gains and '
                            '1 / log2(position + 1) as weights, over the ideal ranking of the gallery; K = 0: the whole list '
                            '(needs whole rankings: with --gallery_feat pass --rank_gallery).')


def ndcg_metric_names(cuts):
    """The columns --ndcg adds, in the order they are printed behind the others."""
    from class_hierarchy import _metric_columns, _ndcg_request
    return list(_metric_columns([], False, False, _ndcg_request(cuts))) if cuts else []


def add_gallery_flags(group):
    """--gallery_feat / --gallery_split of evaluate_retrieval.py and plot_recall_precision.py: every --feat file becomes a set of QUERIES
    against the gallery file at the same position (no --gallery_feat: all-pairs on the --feat file, as the reference does)."""
    group.add_argument('--gallery_feat', type=str, action='append',
                       help='Feature pickle of the GALLERY the matching --feat is queried against (not ranked in full: AP is counted, '
                            'P@k / AHP@K come from top-k lists; needs --clip_ahp or --rank_gallery); repeatable.')
    group.add_argument('--gallery_split', type=str, default='train', choices=['train', 'test'],
                       help='Dataset split the ids of --gallery_feat belong to.')


def add_float64_flag(group):
    """--float64 of evaluate_retrieval.py and plot_recall_precision.py (absent from the namespace unless given, like --rank_gallery)."""
    group.add_argument('--float64', action='store_true', default=argparse.SUPPRESS,
                       help='Evaluate float64 --feat files in float64 like the reference: float64 distances, ranked exactly, and no '
                            'cast-to-float32 warning (float32 files are not affected).  All-pairs on one GPU only: --gallery_feat, '
                            '--rank_gallery, --kblocks and the sharded multi-GPU evaluation stay float32 and refuse this flag.')


def check_float64_flag(parser, args):
    """The flag combinations --float64 refuses (both CLIs)."""
    if getattr(args, 'float64', False):
        if args.gallery_feat or getattr(args, 'rank_gallery', False):
            parser.error('--float64 evaluates all pairs of a --feat file: --gallery_feat / --rank_gallery stay float32')
        if args.kblocks:
            parser.error('--float64 computes ONE float64 FMA chain per distance: --kblocks does not apply')
        if int(os.environ.get('WORLD_SIZE', '1')) > 1:
            parser.error('--float64 runs in one process on one GPU: the sharded multi-GPU evaluation stays float32')


def float64_precision(args, features):
    """``precision`` for one --feat file: 'float64' for a float64 matrix under --float64, else None."""
    wanted = getattr(args, 'float64', False) and isinstance(features, np.ndarray) and features.dtype == np.float64
    return 'float64' if wanted else None


def parse_args(argv=None):
    """``build_parser().parse_args(argv)`` plus the checks that span several flags."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if getattr(args, 'rank_gallery', False) and not args.gallery_feat:
        parser.error('--rank_gallery needs --gallery_feat (without a gallery every ranking is a full one already)')
    if 0 in getattr(args, 'ndcg', ()) and args.gallery_feat and not getattr(args, 'rank_gallery', False):
        parser.error('--ndcg 0 (the whole list) needs whole rankings of the gallery: pass --rank_gallery with --gallery_feat, or cut-offs K > 0 only')
    check_float64_flag(parser, args)
    bootstrap.check_bootstrap_flags(parser, args, [feat_entry(args, i)[0] for i in range(len(args.feat))])
    return args


def gallery_arguments(args, i, data_generator, embed_labels):
    """Keyword arguments ``gallery`` / ``gallery_labels`` / ``gallery_ids`` of the device metric functions for the ``i``-th --feat
    file: empty without a matching --gallery_feat.  Gallery items of the 'test' split share their ids with the queries (a query that
    is a gallery item is dropped from its own ranking); items of the 'train' split are other images whatever their number, so
    their ids are made distinct: ``('train', id)``."""
    if not args.gallery_feat or i >= len(args.gallery_feat):
        return {}
    features, ind2id, _ = _as_feature_matrix(args.gallery_feat[i])
    split_labels = data_generator.labels_train if args.gallery_split == 'train' else data_generator.labels_test
    if embed_labels is not None:
        split_labels = [embed_labels[lbl] for lbl in split_labels]
    ids = list(range(len(features))) if ind2id is None else ind2id.tolist()
    if args.gallery_split == 'test':
        return {'gallery': features, 'gallery_labels': split_labels, 'gallery_ids': ids}
    return {'gallery': features, 'gallery_labels': {('train', j): split_labels[j] for j in ids}, 'gallery_ids': [('train', j) for j in ids]}


def init_distributed():
    """One process per GPU when launched by torch.distributed.run (WORLD_SIZE > 1): RCCL ('nccl') on ROCm devices, gloo
    otherwise (CPU tests).  Returns (rank, world)."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1:
        return 0, 1
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % max(torch.cuda.device_count(), 1))
            dist.init_process_group('nccl')
        else:
            dist.init_process_group('gloo')
    return dist.get_rank(), dist.get_world_size()


def load_labels(args):
    """``(data generator, ind2label, test labels)`` of --dataset / --data_root: ``ind2label`` from the --classes_from pickle (else
    None) restricts and orders the classes, and the test split's labels are mapped through it."""
    from datasets import get_data_generator
    embed_labels = None
    if args.classes_from:
        with open(args.classes_from, 'rb') as f:
            embed_labels = pickle.load(f)['ind2label']
    data_generator = get_data_generator(args.dataset, args.data_root, classes=embed_labels)
    labels_test = [embed_labels[lbl] for lbl in data_generator.labels_test] if embed_labels is not None else data_generator.labels_test
    return data_generator, embed_labels, labels_test


def feat_entry(args, i):
    """``(display name, --norm value)`` of the ``i``-th --feat file: the matching --label, else the file's base name; no."""
    name = args.label[i] if (args.label is not None) and (i < len(args.label)) else os.path.splitext(os.path.basename(args.feat[i]))[0]
    return name, (args.norm[i] if (args.norm is not None) and (i < len(args.norm)) else False)


def main(argv=None):
    from class_hierarchy import ClassHierarchy

    args = parse_args(argv)
    rank, world = init_distributed()
    data_generator, embed_labels, labels_test = load_labels(args)

    id_type = str if args.str_ids else int
    hierarchy = ClassHierarchy.from_file(args.hierarchy, is_a_relations=args.is_a, id_type=id_type)

    ks = list(range(1, args.plot_max + 1))
    for k in [1, 10, 50, 100]:
        if (len(ks) == 0) or (ks[-1] < k):
            ks.append(k)
    perf, tables = OrderedDict(), OrderedDict()     # tables: the per-query rows on the device, under --bootstrap only
    for i, feat_dump in tqdm(enumerate(args.feat), total=len(args.feat), disable=rank != 0):
        feat_name, normalize = feat_entry(args, i)
        # reference: hierarchy.hierarchical_precision(pairwise_retrieval(feat_dump, normalize), labels_test, ks, ...)
        # (evaluate_retrieval.py:197-201).  Here rankings and metrics stay on the GPU: no N x N Python lists.
        features, ind2id, _ = _as_feature_matrix(feat_dump)
        # Several ranks: queries sharded (full rankings), or -- when no metric needs more than the head of a ranking
        # (--skip_ap with --clip_ahp) -- the gallery sharded with an all-gather + merge of per-shard top-k lists.
        gallery_kw = gallery_arguments(args, i, data_generator, embed_labels)
        if gallery_kw and getattr(args, 'rank_gallery', False):
            gallery_kw['rank_gallery'] = True
        if float64_precision(args, features):       # (the keyword is only passed when the flag asks for it)
            gallery_kw['precision'] = 'float64'
        if getattr(args, 'ndcg', None):
            gallery_kw['ndcg'] = args.ndcg
        perf[feat_name], rows = hierarchy.hierarchical_precision_device(
            features, labels_test, ks, compute_ahp=args.clip_ahp if args.clip_ahp else True, compute_ap=not args.skip_ap,
            normalize=normalize, ids=None if ind2id is None else ind2id.tolist(), distributed=world > 1,
            kblocks=args.kblocks, per_query='table' if bootstrap.wanted(args) else False,     # the tables / plots below use the means only
            **gallery_kw)
        if rows is not None:
            tables[feat_name] = rows
    if rank != 0:
        return perf

    metrics = list(METRICS)
    if args.skip_ap:
        metrics.remove('AP')
    if args.clip_ahp:
        metrics[4] = 'AHP@{} (WUP)'.format(args.clip_ahp)
        metrics[9] = 'AHP@{} (LCS_HEIGHT)'.format(args.clip_ahp)
    metrics += ndcg_metric_names(getattr(args, 'ndcg', None))
    print_performance(perf, metrics)
    if tables:
        bootstrap.report(args, tables, metrics)
    if args.csv:
        write_performance(perf, args.csv, args.prec_type)
    if args.plot_max > 0:
        plot_performance(perf, args.plot_max, args.prec_type, args.clip_ahp)
    return perf


if __name__ == '__main__':
    main()
