"""GPU: the image build of the ranking kernel (csrc/rank_rows.hip, VAR 3) with its first pass on one workgroup-shared counter set.

Keys of equal low digit leave that pass in no particular order, and the repair puts every run of equal tags into (key, index) order.
The rows are those of tests/test_rank_image_first_pass_model.py (which shows on the CPU that they stay on, or leave, the fast path
as claimed): exact ties in every relative position of the first pass, rows that give the image up through each exit -- worklist
overflow, run cap, a NaN -- next to rows that keep it, and a row that is given up at level 0 and kept at level 1, whose second
attempt counts on the set the first one used.  Lengths: the smallest per code path -- 64 keys per thread ragged and full, 80 (waves
may sit a row out), 98 (the next row's loads inside the last scatter).  One call of 600 rows gives every workgroup more than two rows,
so the shared set is zeroed between rows.

Every call goes through the C ABI in buffers the test owns (``run_rank`` of tests/test_gpu_rank_matrix.py): the ranks equal
``np.lexsort((index, canon_key))`` bit for bit, ``se_rank_rows_check`` counts 0 violations, nothing is written outside the view, and
the detector's word in the workspace is 3.
"""
import numpy as np
import pytest

import test_gpu_rank_matrix as M
import test_rank_image_first_pass_model as R
from oracle import retrieval_oracle as ro


@pytest.fixture(scope="module")
def sehip():
    import sehip as m
    m.lib()
    m.rank_rows_init()
    return m


def _oracle_is_lexsort(block):
    want = ro.canon_rank_rows(block)
    for r, v in enumerate(block):
        assert np.array_equal(want[r], np.lexsort((np.arange(len(v)), M.canon_key(v)))), r


@pytest.mark.gpu
@pytest.mark.parametrize("n", R.LENGTHS)
def test_image_rows_with_exact_ties_vs_lexsort(sehip, n):
    block = R.block13(n)
    _oracle_is_lexsort(block)
    src = np.arange(block.shape[0], dtype=np.int64)
    flag, _ = M.run_rank(block, src, n, 0, M.VEC, M.NAN, 3)
    assert flag == 3


@pytest.mark.gpu
def test_image_rows_600_rows_several_per_workgroup(sehip):
    n = R.LENGTHS[0]
    block = R.block7(n)
    _oracle_is_lexsort(block)
    src = np.arange(600, dtype=np.int64) % block.shape[0]
    src[[0, 300, 599]] = 0                      # the detector's three rows: plain cosine rows
    assert M.resident_bound(R.ITEMS_OF[n], M.V3) == 256 and len(src) > 2 * 256
    flag, _ = M.run_rank(block, src, n, 0, M.VEC, M.TIGHT, 3)
    assert flag == 3
