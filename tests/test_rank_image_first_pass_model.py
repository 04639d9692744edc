"""CPU model of the image build of the ranking kernel (csrc/rank_rows.hip, VAR 3) with an UNORDERED first pass.

The first 12-bit pass of a two-pass image row counts on one workgroup-shared counter set: keys of equal low digit leave it in whatever
order their returning adds were served.  The second pass is stable, so keys of equal 24-bit image still end next to each other -- in any
order -- and every such block lies inside a run of equal tags, which the repair sorts by (key, index).  This file restates the image
(levels 0 and 1), the two passes and the tag-run repair in NumPy and holds the argument to the rows of
tests/test_gpu_rank_image_first_pass.py:

* with the first pass's tie order reversed and randomly permuted, the (key, index) repair gives ``np.lexsort((index, canon_key))``;
* the earlier repair rule (equal keys keep their places) does not;
* every row the GPU test calls a keeper stays on the fast path at level 0: at most RR_IMG_WL pairs of equal tags, no run above RR_IMG_RUN.

The row generators of the GPU test live here, so both files speak about the same rows.
"""
import functools

import numpy as np

import test_gpu_rank_matrix as M

F32 = np.float32
RR_IMG_RUN, RR_IMG_WL = M.RR_IMG_RUN, M.RR_IMG_WL
LENGTHS = (29697, 32768, 36865, 50000)          # ITEMS 64 ragged, 64 full, 80 (waves may sit a row out), 98 (loads in the scatter)
ITEMS_OF = {29697: 64, 32768: 64, 36865: 80, 50000: 98}


# ------------------------------------------------------------------ the kernel's arithmetic, restated

def image(v, level):
    """24-bit image of a row at level 0 (tight) or 1 (holds every key) -> int64 array, or None when the row cannot take the image path."""
    v = np.ascontiguousarray(v, dtype=F32)
    mb = int((v.view(np.uint32) & 0x7FFFFFFF).max())
    if not (0x0D800000 <= mb < 0x7E800000):
        return None
    e = (mb >> 23) + (1 if (mb & 0x7FFFFF) > 0x400000 else 0) - (1 if level == 0 else 0)
    c = np.array([(e + 1) << 23], dtype=np.uint32).view(F32)[0]
    t = (v + c).astype(F32).view(np.int32).astype(np.int64)
    return np.clip(t - (e << 23), 0, 0xFEFFFF)


def two_passes(q, tie):
    """Positions after pass 0 (low 12 bits; keys of equal digit ordered by ``tie``) and the stable pass 1 (high 12 bits)."""
    o0 = np.lexsort((tie, q & 0xFFF))
    return o0[np.argsort((q >> 12)[o0], kind="stable")]


def tag_runs(q, order):
    """Runs of equal tags (low 8 image bits) along the final positions -> (starts, ends exclusive, pairs)."""
    tag = (q & 0xFF)[order]
    eq = tag[:-1] == tag[1:]
    edge = np.diff(np.concatenate([[False], eq, [False]]).astype(np.int8))
    starts, ends = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0] + 1
    return starts, ends, int(eq.sum())


def repair(order, starts, ends, ck, by_index):
    """The repair: every run of equal tags into key order; ties by index (``by_index``) or left where the passes put them."""
    out = order.copy()
    for a, b in zip(starts, ends):
        run = order[a:b]
        out[a:b] = run[np.lexsort((run, ck[run]))] if by_index else run[np.argsort(ck[run], kind="stable")]
    return out


def model(v, level, tie):
    """-> (ranking with the (key, index) repair, ranking with the earlier rule, pairs, longest run)."""
    q = image(v, level)
    ck = M.canon_key(v)
    order = two_passes(q, tie)
    starts, ends, pairs = tag_runs(q, order)
    longest = int((ends - starts).max()) if len(starts) else 1
    return repair(order, starts, ends, ck, True), repair(order, starts, ends, ck, False), pairs, longest


def is_keeper(v, level=0):
    q = image(v, level)
    if q is None:
        return False
    _, _, pairs, longest = model(v, level, np.arange(len(v)))
    return pairs <= RR_IMG_WL and longest <= RR_IMG_RUN


def canonical(v):
    return np.lexsort((np.arange(len(v)), M.canon_key(v)))


# ------------------------------------------------------------------ rows (shared with the GPU test)

def cosine_like(rng, n):
    """A cosine row as the reference produces it: mixed signs, and the query's own distance of -1."""
    v = (0.1 * rng.standard_normal(n)).astype(F32)
    v[(3 * n) // 7] = F32(-1.0)
    return v


def dups_row(rng, n):
    """600 groups of 2-3 exactly equal keys at random columns."""
    v = cosine_like(rng, n)
    own = (3 * n) // 7
    for k, s in enumerate(rng.choice(n, 600, replace=False)):
        if s == own:
            continue
        dst = rng.choice(n, 1 + k % 2, replace=False)
        v[dst[dst != own]] = v[s]
    return v


def ties_row(rng, n):
    """Exactly equal keys in every relative position of the first pass: the same wave step in neighbouring lanes, the same lane 64
    columns on, one wave apart, first against last column, a triple, a group of five over three waves, and signed zeros."""
    items = ITEMS_OF[n]
    span = items * 64                                   # columns of one wave
    v = cosine_like(rng, n)
    at = lambda wave, step, lane: wave * span + step * 64 + lane     # noqa: E731
    groups = [
        (at(1, 3, 10), at(1, 3, 11)),                                                  # one returning add, neighbouring lanes
        (at(2, 5, 20), at(2, 6, 20)),                                                  # same lane, next step
        (at(0, 7, 33), at(1, 7, 33)),                                                  # one wave apart
        (0, n - 1),                                                                    # first against last column
        (at(3, 1, 63), at(3, 2, 0), at(4, 1, 63)),                                     # a run of three
        (at(0, 0, 5), at(0, 0, 6), at(2, 9, 5), at(5, 0, 0), at(5, items - 1, 63)),    # a run of five
    ]
    vals = (0.01234, -0.04321, 0.1111, -0.2222, 0.05555, -0.00777)
    for cols, val in zip(groups, vals):
        assert max(cols) < n and (3 * n) // 7 not in cols
        v[list(cols)] = F32(val)
    zeros = (at(1, 0, 0), at(0, 2, 17), at(6, 4, 40), at(3, 0, 1))
    v[list(zeros)] = np.array([0.0, -0.0, -0.0, 0.0], dtype=F32)
    return v


def nine_row(rng, n):
    """Nine equal keys: a run above the repair's cap at either level."""
    v = cosine_like(rng, n)
    cols = rng.choice(np.setdiff1d(np.arange(n), [(3 * n) // 7]), 9, replace=False)
    v[cols] = F32(0.03125)
    return v


def retry_row(rng, n):
    """Given up at level 0, kept at level 1: twelve distinct keys next to the -1 lie below the tight image's range and share its
    image 0 -- a run of 13 -- while the image that holds every key tells them apart.  The row's second attempt counts on the set its
    first attempt used."""
    v = dups_row(rng, n)
    own = (3 * n) // 7
    cols = rng.choice(np.setdiff1d(np.arange(n), [own]), 12, replace=False)
    v[cols] = np.linspace(-0.95, -0.55, 12, dtype=F32)
    return v


def nan_row(rng, n):
    v = cosine_like(rng, n)
    v[rng.choice(n, 5, replace=False)] = np.nan
    return v


@functools.lru_cache(maxsize=8)
def block7(n, seed=0):
    """[plain, ties, pair, dups, nine, retry, NaN]: the repeated block of the persistent call.  A workgroup of a 256-workgroup grid
    takes block rows r, r + 4, r + 1 (mod 7): every row that gives up is followed by a keeper, keepers follow keepers."""
    rng = np.random.default_rng(1000 * seed + n)
    rows = [cosine_like(rng, n), ties_row(rng, n), M.pair_row(rng, n), dups_row(rng, n), nine_row(rng, n), retry_row(rng, n), nan_row(rng, n)]
    return np.stack(rows).astype(F32)


@functools.lru_cache(maxsize=8)
def block13(n):
    """One call of 13 rows: plain rows at 0, 6 and 12 (what the detector samples), every other row of two 7-row blocks between them."""
    a, b = block7(n, 0), block7(n, 1)
    rows = [a[0], a[1], a[2], a[3], a[4], a[5], b[0], a[6], b[1], b[3], b[5], b[4], np.random.default_rng(n).permutation(a[0])]
    return np.stack(rows).astype(F32)


KEEPERS_7 = (0, 1, 3)                  # block7 rows that keep the fast path at level 0
KEEPERS_13 = (0, 1, 3, 6, 8, 9, 12)


# ------------------------------------------------------------------ tests

def _tie_orders(n, seed):
    rng = np.random.default_rng(seed)
    return {"reversed": -np.arange(n), "random": rng.permutation(n)}


def test_unordered_first_pass_with_key_index_repair_gives_the_canonical_ranking():
    old_rule_failed = 0
    for n in LENGTHS:
        blk = block13(n)
        for r in KEEPERS_13 + (5, 10):                  # (5, 10: the retry rows, kept at level 1)
            v = blk[r]
            want = canonical(v)
            assert np.array_equal(want, np.argsort(M.canon_key(v), kind="stable"))
            for level in (0, 1):
                for name, tie in _tie_orders(n, 17 * n + r).items():
                    new, old, pairs, longest = model(v, level, tie)
                    assert np.array_equal(new, want), (n, r, level, name)
                    old_rule_failed += not np.array_equal(old, want)
                # a stable first pass: both rules give the canonical order (what the kernel did before)
                new, old, _, _ = model(v, level, np.arange(n))
                assert np.array_equal(new, want) and np.array_equal(old, want), (n, r, level)
    assert old_rule_failed > 0
    # ... and it fails on every row that holds exact ties
    for n in LENGTHS:
        v = block7(n)[1]
        for name, tie in _tie_orders(n, n).items():
            assert not np.array_equal(model(v, 0, tie)[1], canonical(v)), (n, name)


def test_keepers_stay_on_the_fast_path_and_the_other_rows_leave_it():
    for n in LENGTHS:
        for blk, keep in ((block7(n), KEEPERS_7), (block13(n), KEEPERS_13)):
            for r, v in enumerate(blk):
                if r in keep:
                    _, _, pairs, longest = model(v, 0, np.arange(n))
                    print("n=%d row %d: %d pairs, longest run %d" % (n, r, pairs, longest))
                    assert pairs <= RR_IMG_WL and longest <= RR_IMG_RUN, (n, r, pairs, longest)
                else:
                    assert not is_keeper(v, 0), (n, r)
        b = block7(n)
        # worklist overflow and run cap at either level; NaN: no image at all; the retry row: level 0 gives up, level 1 keeps
        assert M.image_must_give_up(b[2]) and M.image_must_give_up(b[4]) and M.image_must_give_up(b[6])
        assert not is_keeper(b[2], 1) and not is_keeper(b[4], 1) and image(b[6], 0) is None
        assert model(b[2], 0, np.arange(n))[2] > RR_IMG_WL and model(b[4], 0, np.arange(n))[3] > RR_IMG_RUN
        assert model(b[5], 0, np.arange(n))[3] > RR_IMG_RUN and is_keeper(b[5], 1)
        assert not M.image_must_give_up(b[5])


def test_tie_rows_hold_every_relative_position():
    for n in LENGTHS:
        items, v = ITEMS_OF[n], block7(n)[1]
        assert M.rank_dispatch(7, n, 0, 0, n).items == items and M.rank_dispatch(7, n, 0, 0, n).img_ok
        ck = M.canon_key(v)
        _, inv, counts = np.unique(ck, return_inverse=True, return_counts=True)
        gaps = set()
        for g in np.nonzero(counts >= 2)[0]:
            cols = np.nonzero(inv == g)[0]
            gaps.update(int(b - a) for a in cols for b in cols if b > a)
        assert {1, 64, items * 64, n - 1} <= gaps, (n, sorted(gaps)[:8])
        z = np.nonzero(v == 0)[0]
        assert len(z) == 4 and set(np.signbit(v[z])) == {True, False}
        assert int(counts.max()) == 5 and 3 in counts


def test_detector_sends_both_calls_to_the_image_build():
    for n in LENGTHS:
        d = M.rank_dispatch(13, n, 0, 0, n)
        blk = block13(n)
        assert M.detector_flag(blk[[0, 6, 12]], d.two_ok, d.img_ok, d.wide) == 3
        b7 = block7(n)
        assert M.detector_flag(b7[[0, 0, 0]], d.two_ok, d.img_ok, d.wide) == 3
