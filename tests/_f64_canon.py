"""Host restatement of the float64 retrieval contract (include/sehip.h) for the tests:

* ``chain_dist``: distances from ONE sequential float64 FMA chain per element, k ascending from +0.0 (``fma`` of libm.so.6 through
  ctypes, vectorised over the output matrix: one libm call per element and k-step would be millions of calls);
* ``canon_rank``: the canonical ranking of a float64 matrix -- (distance, index) ascending, NaN last, -0.0 == +0.0;
* ``refine_runs``: the repair se_rank_refine_f64 makes, restated on the host;
* ``numpy_dist``: the six NumPy lines of the reference's pairwise_retrieval (evaluate_retrieval.py:57-62) in float64.
"""
import ctypes

import numpy as np

_libm = ctypes.CDLL("libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double]
_fma = np.frompyfunc(_libm.fma, 3, 1)


def fma_chain(a, b):
    """C[i, j] = fma(a[i, d-1], b[j, d-1], ... fma(a[i, 0], b[j, 0], +0.0)): float64 [q, n]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(a.shape[1]):
            acc = _fma(a[:, k][:, None], b[:, k][None, :], acc).astype(np.float64)
    return acc


def chain_dist(a, b, cosine, sqa=None, sqb=None):
    """The canonical float64 distances: -C, or (sqa[i] + sqb[j]) - 2 C with one addition and one subtraction, each rounded."""
    c = fma_chain(a, b)
    with np.errstate(all="ignore"):
        if cosine:
            return -c
        return (np.asarray(sqa)[:, None] + np.asarray(sqb)[None, :]) - 2.0 * c


def numpy_dist(features, normalize):
    """evaluate_retrieval.py:57-62 of the reference on a float64 matrix (numexpr's 'A + B - 2 * C' evaluates left to right)."""
    features = np.array(features, dtype=np.float64)
    if normalize:
        features /= np.linalg.norm(features, axis=-1, keepdims=True)
        return -np.dot(features, features.T)
    sqnorm = np.sum(features ** 2, axis=-1)
    return sqnorm[:, None] + sqnorm[None, :] - 2 * np.dot(features, features.T)


def canon_key(d):
    """Sort key of the canonical order: NaN -> +inf rank behind every number (and behind +inf), -0.0 -> +0.0."""
    d = np.asarray(d, dtype=np.float64)
    return np.where(np.isnan(d), np.inf, d + 0.0), np.isnan(d)


def canon_rank(d):
    """Per row: np.lexsort over (index, value, is-NaN) -- value ascending, NaN last, equal values (and +-0) index-ascending."""
    d = np.atleast_2d(d)
    out = np.empty(d.shape, dtype=np.int64)
    idx = np.arange(d.shape[1])
    for i in range(d.shape[0]):
        val, nan = canon_key(d[i])
        out[i] = np.lexsort((idx, val, nan))
    return out


def same_image(x, y):
    return (x == y) | (np.isnan(x) & np.isnan(y))


def refine_runs(d64, img, rank):
    """Host restatement of se_rank_refine_f64 on ONE row: every maximal run of adjacent ranks with equal images, sorted by
    (float64 canonical key, index); everything else untouched."""
    rank = np.array(rank, dtype=np.int64)
    n = len(rank)
    s = 0
    while s < n:
        e = s + 1
        while e < n and same_image(img[rank[e]], img[rank[s]]):
            e += 1
        if e - s >= 2:
            cols = rank[s:e]
            val, nan = canon_key(d64[cols])
            rank[s:e] = cols[np.lexsort((cols, val, nan))]
        s = e
    return rank


def same_bits(got, want):
    """Bit identity of two float arrays, NaN payloads aside (an invalid operation's NaN has the sign bit set on x86 and clear on
    the GPU; both are NaN)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    return np.array_equal(got.view(view)[~nan], want.view(view)[~nan])
