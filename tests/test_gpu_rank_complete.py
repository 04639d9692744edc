"""GPU: se_complete_rankings (sehip.complete_rankings) equals the NumPy restatement of its contract (tests/_complete_canon.py),
integer for integer, `rank` and `status`: gallery sizes at word, wave and step boundaries, list lengths 0, 1, N - 1, N and ragged,
both `order` forms, row pitches above the row lengths, a workgroup that handles many rows (a stale bitmap shows), flagged rows next
to clean ones, duplicates inside one 64-entry chunk and 1,000 entries apart, out-of-range entries, and a gallery above
SE_COMPLETE_LDS_ITEMS (the workspace bitmap).  `rank` is pre-filled with a sentinel: what the contract leaves alone is checked too."""
import numpy as np
import pytest
import torch

from _complete_canon import BAD_DUP, BAD_RANGE, complete_rankings as canon

pytestmark = pytest.mark.gpu

SENTINEL = -77


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def partial_permutations(rng, q, n, L):
    """[q, L] int32: every row the first L entries of a permutation of 0 .. n - 1."""
    if q == 0 or L == 0:
        return np.zeros((q, L), dtype=np.int32)
    return np.argsort(rng.random((q, n)), axis=1)[:, :L].astype(np.int32)


def check(lists, n, lengths=None, order=None, lpad=0, rpad=0, own_out=True):
    """One call against the restatement; ``lpad`` / ``rpad``: extra elements between the rows of lists / rank."""
    import sehip
    q, L = lists.shape
    lists_d = dev(lists)
    if lpad:
        wide = torch.full((q, L + lpad), SENTINEL, dtype=torch.int32, device="cuda")
        wide[:, :L] = lists_d
        lists_d = wide[:, :L]
    out = torch.full((q, n + rpad), SENTINEL, dtype=torch.int32, device="cuda") if own_out else None
    rank, status = sehip.complete_rankings(lists_d, n, None if lengths is None else dev(np.asarray(lengths, dtype=np.int32)),
                                           None if order is None else dev(order), out=out)
    torch.cuda.synchronize()
    want_rank, want_status = canon(lists, n, lengths, order)
    assert rank.dtype == torch.int32 and tuple(rank.shape) == (q, n) and tuple(status.shape) == (q,)
    assert np.array_equal(status.cpu().numpy(), want_status)
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    if own_out and rpad:
        assert bool((out[:, n:] == SENTINEL).all()), "elements gallery .. ldr - 1 of a row were written"
    return want_status


GALLERIES = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 10007]


@pytest.mark.parametrize("with_order", [False, True], ids=["identity", "order"])
@pytest.mark.parametrize("n", GALLERIES)
def test_clean_rows(n, with_order):
    rng = np.random.default_rng(n + 100000 * with_order)
    order = rng.permutation(n).astype(np.int32) if with_order else None
    q = 5
    for L in sorted({0, 1, n - 1, n}):
        lists = partial_permutations(rng, q, n, L)
        assert not check(lists, n, None, order).any()
        assert not check(lists, n, None, order, lpad=3, rpad=5).any()          # neither pitch a multiple of 16 bytes
        assert not check(lists, n, None, order, lpad=4, rpad=8 - n % 4).any()  # rank rows 16-byte aligned (lists too when L % 4 == 0)
    lists = partial_permutations(rng, 7, n, n)
    lengths = np.array([0, n, 1, n - 1, n // 2, rng.integers(0, n + 1), rng.integers(0, n + 1)], dtype=np.int32)
    assert not check(lists, n, lengths, order, own_out=False).any()            # ragged rows in one call; the wrapper's own output
    assert not check(lists, n, lengths, order, lpad=1, rpad=2).any()


def test_single_row_pitches():
    rng = np.random.default_rng(5)
    lists = partial_permutations(rng, 1, 300, 120)
    check(lists, 300, None, None, lpad=8, rpad=4)
    check(lists, 300, [77], rng.permutation(300).astype(np.int32), lpad=1, rpad=1)


def _bad_rows(rng, n):
    """9 rows of a gallery of n >= 2049 items: clean rows with flagged rows directly before and after them."""
    L = n
    lists = partial_permutations(rng, 9, n, L)
    lengths = np.array([n, 1500, n, 1200, n, 40, 3, n // 2, 0], dtype=np.int32)
    lists[1, 70] = lists[1, 65]                # a duplicate inside one 64-entry chunk
    lists[3, 1100] = lists[3, 100]             # ... and 1,000 entries apart
    lists[4, n - 1] = -1                       # out of range
    lists[5, 7] = n
    lists[6, 2] = 2 ** 31 - 1
    lists[7, 5] = lists[7, 6]                  # both: a duplicate and an entry out of range
    lists[7, 900] = n + 5
    lists[3, 1300] = lists[3, 1250]            # behind this row's length: not read
    want = np.array([0, BAD_DUP, 0, BAD_DUP, BAD_RANGE, BAD_RANGE, BAD_RANGE, BAD_DUP | BAD_RANGE, 0], dtype=np.int32)
    return lists, lengths, want


@pytest.mark.parametrize("with_order", [False, True], ids=["identity", "order"])
def test_bad_rows_between_clean_rows(with_order):
    rng = np.random.default_rng(11)
    n = 2049
    order = rng.permutation(n).astype(np.int32) if with_order else None
    lists, lengths, want = _bad_rows(rng, n)
    assert np.array_equal(check(lists, n, lengths, order, rpad=3), want)
    assert np.array_equal(check(lists, n, lengths, order, lpad=3, rpad=0), want)
    # every entry of a full-length list twice: flagged whichever lanes meet
    twice = np.concatenate([lists[:1, :1024], lists[:1, :1024]], axis=1)
    assert check(twice, n, None, order)[0] == BAD_DUP
    # a list longer than the gallery is flagged one way or the other and writes nothing behind the row
    long = np.concatenate([lists[:2], lists[:2, :40]], axis=1)
    assert check(long, n, None, order, rpad=64).all()


@pytest.mark.parametrize("with_order", [False, True], ids=["identity", "order"])
def test_many_rows_per_workgroup(with_order):
    """20,000 rows of a gallery of 16: every workgroup handles many rows, one in ten of them flagged, so a bitmap or flag that
    stayed from the row before shows."""
    rng = np.random.default_rng(3)
    q, n = 20000, 16
    order = rng.permutation(n).astype(np.int32) if with_order else None
    lists = partial_permutations(rng, q, n, n)
    lengths = rng.integers(0, n + 1, size=q).astype(np.int32)
    bad = np.flatnonzero((rng.random(q) < 0.1) & (lengths >= 2))
    kind = rng.integers(0, 3, size=len(bad))
    for r, k in zip(bad.tolist(), kind.tolist()):
        lists[r, lengths[r] - 1] = (lists[r, 0], -1, n)[k]
    status = check(lists, n, lengths, order)
    assert np.array_equal(np.flatnonzero(status), bad)


def test_gallery_above_the_lds_bound():
    """The membership bitmap moves to the workspace: lists of 0, 5 and 1,000 entries, both order forms, then flagged rows."""
    import sehip
    n = sehip.COMPLETE_LDS_ITEMS + 37
    rng = np.random.default_rng(9)
    lists = rng.permutation(n)[:3000].reshape(3, 1000).astype(np.int32)
    lengths = [0, 5, 1000]
    assert not check(lists, n, lengths, None, rpad=3).any()
    assert not check(lists, n, lengths, rng.permutation(n).astype(np.int32)).any()
    lists[1, 900] = lists[1, 17]
    lists[2, 3] = n
    assert np.array_equal(check(lists, n, [1000, 1000, 5], None), [0, BAD_DUP, BAD_RANGE])
    assert not check(lists, n, [1000, 900, 3], None).any()       # the same workspace, cleared again


def test_empty_calls():
    import sehip
    rank, status = sehip.complete_rankings(torch.zeros((0, 5), dtype=torch.int32, device="cuda"), 9)
    assert tuple(rank.shape) == (0, 9) and tuple(status.shape) == (0,)
    rank, status = sehip.complete_rankings(torch.zeros((4, 0), dtype=torch.int32, device="cuda"), 0)
    assert tuple(rank.shape) == (4, 0) and not status.cpu().numpy().any()


def test_wrapper_checks():
    import sehip
    lists = torch.zeros((4, 6), dtype=torch.int32, device="cuda")
    with pytest.raises(sehip.SehipError):
        sehip.complete_rankings(lists.long(), 9)
    with pytest.raises(sehip.SehipError):
        sehip.complete_rankings(lists, 9, lengths=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(sehip.SehipError):
        sehip.complete_rankings(lists, 9, order=torch.arange(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(sehip.SehipError):
        sehip.complete_rankings(lists, 9, out=torch.zeros((4, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(sehip.SehipError):
        sehip.complete_rankings(lists.cpu(), 9)


def test_invalid_arguments_on_device_pointers():
    """SE_ERR_INVALID of the raw entry point with real device buffers (tests/test_ranked_host.py makes the same calls without one)."""
    from test_ranked_host import invalid_calls
    lists = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    rank = torch.zeros((4, 16), dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    invalid_calls(lists.data_ptr(), rank.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    assert not rank.cpu().numpy().any()
