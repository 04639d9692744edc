"""NumPy restatement of the bootstrap index stream of include/sehip.h (se_bootstrap_indices / se_bootstrap_means) and of the
replicate means, for the tests: vectorised uint64 arithmetic for the stream, exact integer arithmetic for the means of dyadic
tables (integers / 2^10), exact rational arithmetic for general float64 tables."""
from fractions import Fraction

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 ints -> 4 uint64 arrays holding 32-bit words."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def indices(q, seed, r, t):
    """idx(seed, r, t, q) for an array of draws ``t`` of replicate ``r`` -> int64 array."""
    q, seed, r = int(q), int(seed) & ((1 << 64) - 1), int(r)
    t = np.atleast_1d(np.asarray(t, dtype=np.uint64))
    b = t >> np.uint64(1)
    x = philox4x32_10((b & MASK, b >> S32, r & 0xFFFFFFFF, (r >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))
    odd = (t & np.uint64(1)).astype(bool)
    lo, hi = np.where(odd, x[2], x[0]), np.where(odd, x[3], x[1])
    # (u * q) >> 64 with u = lo | hi << 32 and q < 2^32: (hi * q + ((lo * q) >> 32)) >> 32, every term below 2^64
    qq = np.uint64(q)
    return ((hi * qq + ((lo * qq) >> S32)) >> S32).astype(np.int64)


def index_matrix(q, seed, rep0, reps, t0=0, count=None):
    """What se_bootstrap_indices writes: int32 [reps, count]."""
    count = q - t0 if count is None else count
    t = np.arange(t0, t0 + count, dtype=np.uint64)
    return np.stack([indices(q, seed, rep0 + i, t) for i in range(reps)]).astype(np.int32) if reps else np.zeros((0, count), np.int32)


def dyadic_means(ints, shift, seed, rep0, reps):
    """Replicate means of the table ints / 2^shift (ints: int64 [q, m], every entry and every column sum of q draws exact in float64):
    exact integer sums, then the one correctly rounded division float64(S) / float64(q) the kernel makes."""
    q = ints.shape[0]
    out = np.empty((reps, ints.shape[1]), dtype=np.float64)
    for i in range(reps):
        s = ints[indices(q, seed, rep0 + i, np.arange(q, dtype=np.uint64))].sum(axis=0, dtype=np.int64)
        assert int(np.abs(s).max()) < (1 << 53)
        out[i] = np.ldexp(s.astype(np.float64), -shift) / np.float64(q)
    return out


def exact_means(vals, seed, rep0, reps):
    """Replicate means of a float64 table as exact rationals: list (replicate) of lists (column) of Fraction."""
    q, m = vals.shape
    fr = [[Fraction(float(v)) for v in row] for row in vals]
    out = []
    for i in range(reps):
        idx = indices(q, seed, rep0 + i, np.arange(q, dtype=np.uint64)).tolist()
        out.append([sum((fr[j][c] for j in idx), Fraction(0)) / q for c in range(m)])
    return out
