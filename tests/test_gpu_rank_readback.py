"""The read-back of the ranking kernels (``RRRead`` of csrc/rank_rows.hip: four steps per transposed LDS read, the last ITEMS % 4
steps by 16-bit reads) through every ``ITEMS`` instantiation, at the last full 512-key step and 37 columns short of it.

Three 3-row calls per length through the C ABI, one per row family: cosine rows of normalised Gaussian features (the image build
where the instantiation has one: two read-backs), non-negative Euclidean-like rows (the window build where it exists: two
read-backs) and rows with one NaN and one -inf (every fast path refuses them: the plain three passes with all their read-backs).
One call of two 70,000-column rows takes a ``SEG`` build.  The buffers, the guard rows with their sentinel, the comparison with
``oracle/retrieval_oracle.py``'s canonical ranking (bit for bit) and the order guard are those of ``tests/test_gpu_rank_matrix.py``.
The CPU test holds the row families to the builds they are meant to reach."""
import functools

import numpy as np
import pytest

import test_gpu_rank_matrix as M

F32 = np.float32
COS, EUC, SPECIAL = "cosine", "euclid", "nan-inf"
FAMILIES = (COS, EUC, SPECIAL)
LONG_N = 70000


def lengths(items):
    return (1024, 987) if items == 2 else (512 * items, 512 * items - 37)


@functools.lru_cache(maxsize=2)
def blocks(n):
    """{family: [3, n] float32} for one row length."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 64)).astype(F32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    cos = -(x[[0, n // 2, n - 1]] @ x.T)
    euc = np.abs(200.0 + 20.0 * rng.standard_normal((3, n))).astype(F32)
    euc[np.arange(3), [(r * 131 + 7) % n for r in range(3)]] = 0.0                  # the query's own distance
    spc = (0.1 * rng.standard_normal((3, n))).astype(F32)
    for r in range(3):
        a, b = rng.choice(n, size=2, replace=False)
        spc[r, a], spc[r, b] = np.nan, -np.inf
    return {COS: np.ascontiguousarray(cos, dtype=F32), EUC: euc, SPECIAL: spc}


def predicted_flag(block, n):
    d = M.rank_dispatch(block.shape[0], n, 0, 0, n)
    return M.detector_flag(block, d.two_ok, d.img_ok, d.wide)


def test_row_families_reach_the_builds_they_are_meant_for():
    """Cosine rows select the image build and Euclidean-like rows the window build wherever the instantiation has one; the
    instantiations are the ones the lengths claim."""
    for items in M.ITEMS_TABLE:
        for n in lengths(items):
            assert M.rank_dispatch(3, n, 0, 0, n).items == items
            if M.is_wide(items):
                b = blocks(n)
                assert predicted_flag(b[COS], n) == (M.V3 if items <= M.RR_IMG_MAX_ITEMS else M.V0), (items, n)
                assert predicted_flag(b[EUC], n) == M.V2, (items, n)
                assert all(M.window_keeps(r) for r in b[EUC]) and not any(M.window_keeps(r) for r in b[SPECIAL])
                assert all(M.image_must_give_up(r) for r in b[SPECIAL])
    d = M.rank_dispatch(2, LONG_N, 0, 0, LONG_N)
    assert (d.path, d.segments, d.items) == ("runs", 2, 72)


@pytest.fixture(scope="module")
def sehip():
    import sehip as m
    m.lib()
    m.rank_rows_init()
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("items", M.ITEMS_TABLE)
def test_read_back_every_items_three_families(sehip, items):
    i = M.ITEMS_TABLE.index(items)
    src = np.arange(3, dtype=np.int64)
    for j, n in enumerate(lengths(items)):
        b = blocks(n)
        for f, fam in enumerate(FAMILIES):
            idx = (i + j + f) % 3
            out = (M.VEC, M.PITCH, M.OFF)[(i + f) % 3]
            flag, _ = M.run_rank(b[fam], src, n, idx, out, M.NAN, predicted_flag(b[fam], n))
            print("ITEMS %d n %d %s: build %d, width %d, %s" % (items, n, fam, flag, idx, out), flush=True)


@pytest.mark.gpu
def test_read_back_long_rows_seg_build(sehip):
    rng = np.random.default_rng(LONG_N)
    x = rng.standard_normal((LONG_N, 64)).astype(F32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    block = np.ascontiguousarray(-(x[[1, LONG_N - 2]] @ x.T), dtype=F32)
    M.run_rank(block, np.arange(2, dtype=np.int64), LONG_N, 0, M.VEC, M.NAN, None)
