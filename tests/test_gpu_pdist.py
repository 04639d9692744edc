"""The all-pairs distance kernel (``se_pairwise_dist``, csrc/pdist_mfma.hip) through every instantiation it can launch.

``launch_pdist`` / ``launch_pdist2`` choose one of 24 ``pdist_kernel<METRIC, MULTI_KB, SYM, VEC, EPI_STORE>`` from the call's
metric, its K-block list, whether both operands are the same matrix and whether 16-byte operand loads are legal.
``pdist_dispatch`` restates that choice in Python; a CPU test holds the case table to all 24 tuples (each at two tile
remainders), so that dropping a case can never silently drop an instantiation.  Each case is compared with oracle/canon.c
bit for bit, with NaN in every input byte the kernel must not read and a sentinel in every output byte it must not write.

The real-workload sizes (CUB, NABirds, ILSVRC val) run the whole retrieval step and are checked by oracle/verify.py.
"""
import itertools
from collections import defaultdict

import numpy as np
import pytest

from oracle import retrieval_oracle as ro
from oracle import verify

COS, EUC, DOT = ro.METRIC_COSINE, ro.METRIC_EUCLID, ro.METRIC_DOT
METRIC_NAMES = {COS: "cos", EUC: "euc", DOT: "dot"}
TILE = 128                 # PD_BM = PD_BN: output tile edge of the kernel
MAX_KB = 16                # SE_MAX_KB

# operand modes: b=None (the symmetric candidate), b = the same values in a second buffer, q != n
SYM, COPY, ASYM = "sym", "copy", "asym"
# operand layouts: contiguous rows; pitch padded to a multiple of 4 past D (NaN padding); column slice at offset 1 (base 4 bytes
# off 16-byte alignment, NaN in the skipped column); the first rows of a taller buffer whose following rows are NaN
CONTIG, PADDED, COL1, ROWS = "contig", "padded", "col1", "rows"
# output layouts: sehip.empty_rows (pitch padded to 16 bytes); a caller `out` with ldo = n + 1 one row into a sentinel-filled buffer
EMPTY, GUARDED = "empty_rows", "guarded"


def kb16(d):
    """A full list of 16 K-blocks (SE_MAX_KB) with blocks of length 1, 65 and 2 at its head."""
    rest = d - 68
    return [1, 65, 2] + [rest // 13] * 12 + [rest - 12 * (rest // 13)]


AL1000 = [448, 276, 276]   # OpenBLAS's list for D = 1000 (the ILSVRC features): every block starts on a multiple of 4
UN555 = [278, 277]         # OpenBLAS's list for D = 555 (NABirds): the second block starts at 278

# (metric, mode, q, n, d, kblocks, layout, out_layout); each section is the instantiation pdist_dispatch maps its cases to
CASES = [
    # ---- symmetric, one K-block, 16-byte loads
    (COS, SYM, 129, 129, 64, None, CONTIG, EMPTY),
    (COS, SYM, 256, 256, 3, None, PADDED, GUARDED),
    (EUC, SYM, 130, 130, 100, None, ROWS, GUARDED),
    (EUC, SYM, 385, 385, 65, None, PADDED, EMPTY),
    (DOT, SYM, 131, 131, 1, None, PADDED, EMPTY),
    (DOT, SYM, 257, 257, 64, None, ROWS, GUARDED),
    # ---- symmetric, one K-block, scalar loads
    (COS, SYM, 130, 130, 7, None, CONTIG, GUARDED),
    (COS, SYM, 255, 255, 555, None, COL1, EMPTY),
    (EUC, SYM, 129, 129, 1, None, CONTIG, EMPTY),
    (EUC, SYM, 256, 256, 129, None, ROWS, GUARDED),
    (DOT, SYM, 131, 131, 555, None, CONTIG, EMPTY),
    (DOT, SYM, 700, 700, 2, None, COL1, GUARDED),
    # ---- symmetric, several K-blocks, 16-byte loads
    (COS, SYM, 131, 131, 1000, AL1000, CONTIG, EMPTY),
    (COS, SYM, 257, 257, 129, [64, 65], PADDED, GUARDED),
    (EUC, SYM, 129, 129, 1000, AL1000, ROWS, GUARDED),
    (EUC, SYM, 700, 700, 555, [448, 107], PADDED, EMPTY),
    (DOT, SYM, 130, 130, 100, [64, 36], CONTIG, GUARDED),
    (DOT, SYM, 385, 385, 7, [4, 3], PADDED, EMPTY),
    # ---- symmetric, several K-blocks, scalar loads
    (COS, SYM, 129, 129, 555, UN555, CONTIG, EMPTY),
    (COS, SYM, 700, 700, 100, kb16(100), PADDED, GUARDED),
    (EUC, SYM, 130, 130, 1000, AL1000, COL1, EMPTY),
    (EUC, SYM, 255, 255, 555, kb16(555), CONTIG, GUARDED),
    (DOT, SYM, 131, 131, 65, [1, 64], ROWS, GUARDED),
    (DOT, SYM, 256, 256, 1000, kb16(1000), COL1, EMPTY),
    # ---- general, one K-block, 16-byte loads
    (COS, COPY, 129, 129, 64, None, ROWS, GUARDED),
    (COS, ASYM, 257, 130, 100, None, CONTIG, EMPTY),
    (EUC, COPY, 256, 256, 7, None, PADDED, EMPTY),
    (EUC, ASYM, 131, 385, 64, None, CONTIG, GUARDED),
    (DOT, COPY, 131, 131, 555, None, PADDED, GUARDED),
    (DOT, ASYM, 130, 700, 1000, None, CONTIG, EMPTY),
    # ---- general, one K-block, scalar loads
    (COS, COPY, 130, 130, 63, None, CONTIG, EMPTY),
    (COS, ASYM, 385, 255, 2, None, COL1, GUARDED),
    (EUC, COPY, 257, 257, 3, None, COL1, GUARDED),
    (EUC, ASYM, 129, 131, 555, None, ROWS, EMPTY),
    (DOT, COPY, 129, 129, 65, None, CONTIG, GUARDED),
    (DOT, ASYM, 256, 130, 1, None, ROWS, EMPTY),
    # ---- general, several K-blocks, 16-byte loads
    (COS, COPY, 256, 256, 1000, AL1000, CONTIG, GUARDED),
    (COS, ASYM, 129, 385, 555, [448, 107], PADDED, EMPTY),
    (EUC, COPY, 131, 131, 129, [64, 65], PADDED, EMPTY),
    (EUC, ASYM, 700, 257, 1000, AL1000, ROWS, GUARDED),
    (DOT, COPY, 129, 129, 64, [32, 32], ROWS, EMPTY),
    (DOT, ASYM, 255, 130, 100, [64, 36], CONTIG, GUARDED),
    # ---- general, several K-blocks, scalar loads
    (COS, COPY, 130, 130, 555, UN555, ROWS, EMPTY),
    (COS, ASYM, 131, 256, 129, kb16(129), CONTIG, GUARDED),
    (EUC, COPY, 255, 255, 100, kb16(100), CONTIG, GUARDED),
    (EUC, ASYM, 385, 129, 555, UN555, COL1, EMPTY),
    (DOT, COPY, 257, 257, 1000, kb16(1000), PADDED, EMPTY),
    (DOT, ASYM, 130, 700, 65, [1, 64], CONTIG, GUARDED),
]

N_VALUES = (129, 130, 131, 255, 256, 257, 385, 700)
D_VALUES = (1, 2, 3, 7, 63, 64, 65, 100, 129, 555, 1000)

# (name, n, d, kblocks): the reference's retrieval evaluations at full size
WORKLOADS = [
    ("cub", 5794, 200, None),
    ("nabirds", 24633, 555, UN555),
    ("ilsvrc", 50000, 1000, AL1000),
]


# ------------------------------------------------------------------ the dispatch, restated

def layout_pitch(layout, d):
    """Row pitch (elements) of an operand of depth ``d`` in ``layout``."""
    if layout == PADDED:
        return (d // 4 + 1) * 4
    if layout == COL1:
        return d + 1
    return d


def layout_aligned(layout):
    """Whether the operand's base address is 16-byte aligned (the column slice starts 4 bytes into its buffer)."""
    return layout != COL1


def pdist_dispatch(metric, mode, q, n, d, kblocks, layout):
    """``(metric, multi, sym, vec)`` of the ``pdist_kernel`` that ``se_pairwise_dist`` launches for a case (``launch_pdist`` /
    ``launch_pdist2``).  Both operands of a case share its layout; ``pairwise_dist(a, None)`` passes ``a`` and its norms on both sides."""
    multi = kblocks is not None and len(kblocks) > 1
    # a == b, same pitch, q == n, (Euclid) sqa == sqb, and more than one tile
    sym = mode == SYM and q == n and n > TILE
    # both pitches multiples of 4, 16-byte aligned bases, every K-block starting on a multiple of 4
    starts = np.cumsum([0] + list(kblocks))[:-1] if multi else [0]
    vec = layout_pitch(layout, d) % 4 == 0 and layout_aligned(layout) and all(int(s) % 4 == 0 for s in starts)
    return metric, multi, sym, vec


def case_id(c):
    metric, mode, q, n, d, kb, layout, out_layout = c
    kbs = "kb%d" % len(kb) if kb else "kb1"
    return "%s-%s-%dx%dx%d-%s-%s-%s" % (METRIC_NAMES[metric], mode, q, n, d, kbs, layout, out_layout)


# ------------------------------------------------------------------ CPU: the table reaches every instantiation

def test_case_table_is_well_formed():
    for c in CASES:
        metric, mode, q, n, d, kb, layout, out_layout = c
        assert metric in METRIC_NAMES and mode in (SYM, COPY, ASYM) and layout in (CONTIG, PADDED, COL1, ROWS), c
        assert out_layout in (EMPTY, GUARDED), c
        assert n in N_VALUES and q in N_VALUES and d in D_VALUES, c
        assert (q != n) == (mode == ASYM), c
        if kb is not None:
            assert sum(kb) == d and min(kb) > 0 and 1 < len(kb) <= MAX_KB, c
    assert len({case_id(c) for c in CASES}) == len(CASES)


def test_case_table_reaches_all_24_instantiations():
    """Every (metric, MULTI_KB, SYM, VEC) tuple is launched by at least two cases at different tile remainders n % 128."""
    rem = defaultdict(set)
    for metric, mode, q, n, d, kb, layout, _ in CASES:
        rem[pdist_dispatch(metric, mode, q, n, d, kb, layout)].add(n % TILE)
    want = set(itertools.product((COS, EUC, DOT), (False, True), (False, True), (False, True)))
    assert set(rem) == want, sorted(want - set(rem))
    thin = {t: r for t, r in rem.items() if len(r) < 2}
    assert not thin, thin


def test_case_table_reaches_the_edges():
    """The paths the instantiation matrix alone does not name."""
    disp = [(c, pdist_dispatch(*c[:7])) for c in CASES]
    # symmetric shapes whose last tile row holds 1, 2 and 3 rows (the mirrored tile has that partial width)
    assert {c[3] % TILE for c, t in disp if t[2]} >= {1, 2, 3}
    # 16-byte loads over a pitch padded past D (the load is clamped, the padding masked), with and without K-blocks
    assert {t[1] for c, t in disp if t[3] and c[6] == PADDED and c[4] % 4} == {False, True}
    # output pitches that are (not) multiples of 4 on caller buffers, symmetric and general
    assert {((c[3] + 1) % 4 == 0, t[2]) for c, t in disp if c[7] == GUARDED} == set(itertools.product((False, True), repeat=2))
    # K-blocks of length 1 and 2, and the full SE_MAX_KB list, in all three metrics and both modes
    assert {(c[0], t[2]) for c, t in disp if c[5] and len(c[5]) == MAX_KB} == set(itertools.product((COS, EUC, DOT), (False, True)))
    assert any(c[5] and 1 in c[5] and not t[2] for c, t in disp) and any(c[5] and 2 in c[5] and t[2] for c, t in disp)


def test_real_workloads_take_the_symmetric_kernel():
    """What each full-size workload below exercises: CUB one K-block with 16-byte loads, NABirds several K-blocks with scalar loads
    (its second block starts at 278), ILSVRC val several K-blocks with 16-byte loads."""
    got = [pdist_dispatch(COS, SYM, n, n, d, kb, CONTIG)[1:] for _, n, d, kb in WORKLOADS]
    assert got == [(False, True, True), (True, True, False), (True, True, True)]


# ------------------------------------------------------------------ GPU: the instantiation matrix

@pytest.fixture(scope="module")
def sehip():
    import sehip as m
    m.lib()
    return m


SENTINEL = np.int32(0x7FC0DEAD)     # a quiet NaN with a payload no kernel produces


def mixed_rows(rows, d, seed):
    """Gaussian rows, half of them scaled by powers of two over 41 binades: a K-block restart or an accumulation order that
    differs from the oracle's changes the bits."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, d)).astype(np.float32)
    scaled = np.nonzero(rng.random(rows) < 0.5)[0]
    x[scaled] *= np.exp2(rng.integers(-20, 21, size=len(scaled))).astype(np.float32)[:, None]
    return x


def place(x, layout):
    """Device copy of ``x`` in ``layout``, with NaN in every element of the buffer that is not part of the matrix."""
    import torch
    rows, d = x.shape
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if layout == CONTIG:
        return t
    if layout == ROWS:
        buf = torch.full((rows + 7, d), float("nan"), device="cuda")
        buf[:rows] = t
        return buf[:rows]
    buf = torch.full((rows, layout_pitch(layout, d)), float("nan"), device="cuda")
    if layout == PADDED:
        buf[:, :d] = t
        return buf[:, :d]
    buf[:, 1:] = t
    return buf[:, 1:]


def run_pdist(sehip, a, b, metric, kb, out_layout):
    """pairwise_dist into ``out_layout``; checks the sentinels around a caller buffer and returns the result on the host."""
    import torch
    q, n = a.shape[0], (a if b is None else b).shape[0]
    if out_layout == EMPTY:
        return sehip.pairwise_dist(a, b, metric=metric, kblocks=kb).cpu().numpy()
    buf = torch.full((q + 3, n + 1), int(SENTINEL), dtype=torch.int32, device="cuda").view(torch.float32)
    got = sehip.pairwise_dist(a, b, metric=metric, kblocks=kb, out=buf[1:q + 1, :n])
    assert got.stride(0) == n + 1
    bits = buf.view(torch.int32).cpu().numpy()
    outside = np.ones(bits.shape, dtype=bool)
    outside[1:q + 1, :n] = False
    assert (bits[outside] == SENTINEL).all(), "a store left the output (pitch padding or guard rows)"
    return bits[1:q + 1, :n].view(np.float32).copy()


def bits_equal(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32))


def check_layout(t, layout, d):
    """The operand the kernel sees is the one pdist_dispatch assumed."""
    assert t.stride(0) == layout_pitch(layout, d) and (t.data_ptr() % 16 == 0) == layout_aligned(layout)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_pdist_instantiation_bit_exact(sehip, case):
    """Output == canon_pdist bit for bit; padding / trailing-row NaNs never reach it; the output's padding and guard rows keep their
    sentinels.  Symmetric cases also equal their transpose and the same values run through the general kernel (a second buffer)
    and through the other operand-load path."""
    metric, mode, q, n, d, kb, layout, out_layout = case
    seed = CASES.index(case)
    xa = mixed_rows(q, d, seed)
    xb = None if mode == SYM else (xa if mode == COPY else mixed_rows(n, d, seed + 1000))
    want = ro.canon_pdist(xa, xb, metric, kb)    # Euclid: canon_row_sqsum == row_sqnorm, the norms pairwise_dist computes

    a = place(xa, layout)
    b = None if xb is None else place(xb, layout)
    check_layout(a, layout, d)
    got = run_pdist(sehip, a, b, metric, kb, out_layout)
    assert np.isfinite(got).all(), "non-finite output from finite inputs (padding or trailing rows were read)"
    assert bits_equal(got, want), "%d of %d outputs differ from the oracle" % (int((got != want).sum()), got.size)
    if mode != SYM:
        return

    _, multi, sym, vec = pdist_dispatch(metric, mode, q, n, d, kb, layout)
    assert sym
    assert bits_equal(got, got.T)
    # the same values in a second buffer: the general kernel, same load path
    assert pdist_dispatch(metric, COPY, q, n, d, kb, layout) == (metric, multi, False, vec)
    general = run_pdist(sehip, a, place(xa, layout), metric, kb, out_layout)
    assert bits_equal(general, got)
    # the symmetric kernel with the other load path (16-byte loads where the K-blocks allow them, else the scalar path again)
    other = COL1 if vec else PADDED
    alt = place(xa, other)
    check_layout(alt, other, d)
    assert bits_equal(run_pdist(sehip, alt, None, metric, kb, out_layout), got)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [COS, EUC, DOT], ids=["cos", "euc", "dot"])
@pytest.mark.parametrize("mode", [SYM, COPY])
@pytest.mark.parametrize("kb", [None, [64, 36]], ids=["kb1", "kb2"])
def test_pdist_non_finite_rows(sehip, metric, mode, kb):
    """A row holding +inf and -inf and a row holding a NaN, through the symmetric and the general kernel: inf - inf and NaN
    propagate through the FMA chain, the K-block sum and the Euclidean epilogue exactly as in the oracle."""
    n, d = 257, 100
    x = mixed_rows(n, d, 7)
    x[3, 10], x[3, 77] = np.inf, -np.inf
    x[130, 42] = np.nan
    want = ro.canon_pdist(x, None if mode == SYM else x, metric, kb)
    a = place(x, CONTIG)
    got = run_pdist(sehip, a, None if mode == SYM else place(x, CONTIG), metric, kb, EMPTY)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got, got.T, equal_nan=True)
    fin = np.ones(n, dtype=bool)
    fin[[3, 130]] = False
    assert np.isfinite(got[np.ix_(fin, fin)]).all()


# ------------------------------------------------------------------ GPU: the real workloads at full size

def workload_features(n, d, seed):
    """``mixed_rows`` with 32 pairs of exact duplicates straddling tile boundaries (rows 128 j - 1 and 128 j, copies of one
    random row each): their distance ties cross tiles of the distance kernel, of the ranking and of verify's samples."""
    x = mixed_rows(n, d, seed)
    src = np.random.default_rng(seed + 1).integers(0, n, size=32)
    for j, s in enumerate(src):
        x[TILE * (j + 1) - 1] = x[s]
        x[TILE * (j + 1)] = x[s]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [COS, EUC], ids=["cosine", "euclid"])
@pytest.mark.parametrize("name,n,d,kb", WORKLOADS, ids=["%s-%dx%d" % (w[0], w[1], w[2]) for w in WORKLOADS])
def test_real_workload_retrieval_step(sehip, name, n, d, kb, metric):
    """features -> normalize_rows_ / row_sqnorm -> symmetric pairwise_dist(x, None) -> rank_rows, checked by
    verify.verify_retrieval_step: the matrix equals its transpose, every row is a permutation sorted in tie order, and sampled rows
    on both sides of tile boundaries match the oracle bit for bit.  ILSVRC cosine also goes through evaluate_retrieval.ranking_tiles,
    whose single whole-matrix tile takes the same kernel."""
    import torch
    x = workload_features(n, d, seed=n)
    g = torch.from_numpy(x).cuda()
    if metric == COS:
        sehip.normalize_rows_(g)
        pd = sehip.pairwise_dist(g, None, metric=COS, kblocks=kb)
    else:
        sq = sehip.row_sqnorm(g)
        pd = sehip.pairwise_dist(g, None, metric=EUC, sqa=sq, sqb=sq, kblocks=kb)
    rk = sehip.rank_rows(pd)
    try:
        ok, detail = verify.verify_retrieval_step(g.cpu().numpy(), pd, rk, metric, kblocks=kb)
        assert ok, detail
        assert detail["symmetric"] and detail["rows_checked"] >= 50
        if name == "ilsvrc" and metric == COS:
            import evaluate_retrieval as er
            tiles = 0
            try:
                for r0, t in er.ranking_tiles(torch.from_numpy(x).cuda(), normalize=True, kblocks=kb):
                    assert torch.equal(t, rk[r0:r0 + t.shape[0]]), "ranking_tiles differs from the direct ranking at row %d" % r0
                    tiles += 1
            finally:
                er.release_tile_cache()
            assert tiles == 1
    finally:
        del pd, rk, g
        torch.cuda.empty_cache()
