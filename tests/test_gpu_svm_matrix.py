"""The linear-SVM kernels (csrc/svm.hip) through every instantiation their host code can choose, bit for bit against float64.

``se_svm_margin`` picks ``svm_margin_kernel<MODE, VX, VW>`` and ``se_svm_reduce`` picks ``svm_reduce_kernel<VZ, VX>`` per operand from
``sv_aligned`` (16-byte base, pitch and width multiples of 4, width >= 4); ``sv_slice`` cuts the rows of the reduction into slices of
256 .. 4096 rows.  The functions below restate those choices in Python, and CPU tests hold the case tables to every tuple of them, so
that dropping a case can never silently drop a path.

The exact cases use inputs on a grid: X in {-1, 0, 1}, weights and Z multiples of 1/4, ``cpen = 0.5``.  Every product and every partial
sum is then a multiple of 1/4 (1/16 for the loss) far below 2^24 grid units, so float32 computes it without rounding in any order:
MFMA order, slice order and the float64 combine cannot matter, and the kernels must equal NumPy float64 bit for bit.  Each case
asserts on the host that its magnitudes stay on that grid.  An exact comparison sees what a tolerance band cannot: ``>=`` for ``>`` at
``t == 0`` (the cases hold many such entries), a loss partial credited to the neighbouring block, the bias of another column; a CPU
test feeds the comparators the float64 reference with one such defect at a time and expects each to be rejected.

Inputs sit in views whose pitch padding holds a NaN sentinel (never read into a result), one of them starting one float into its
storage (misaligned base: the element path).  Outputs go to caller buffers whose pitch padding and guard rows hold the same sentinel
and must come back untouched.
"""
import itertools

import numpy as np
import pytest

EPS32 = 2.0 ** -24
GRID_LIMIT = 2.0 ** 24              # exact float32 integers: |value| / grid unit stays below this
BM = BN = 128                       # SV_BM / SV_BN
BK = 32                             # SV_BK
LOSS_ROWS = 64                      # SV_LOSS_ROWS
MIN_SLICE, MAX_SLICE, TARGET_WGS = 256, 4096, 2048
AXPBY_GRID_CAP = 4096               # blocks of 256 threads of svm_axpby_kernel
CPEN = 0.5
GRAD, HV, SCORE = "grad", "hv", "score"

# layouts of X and Z: contiguous rows; pitch + 4 (NaN padding, still 16-byte rows when the width is a multiple of 4); pitch + 1; a view
# one float into its storage whose pitch is a multiple of 4 (misaligned base)
CONTIG, PAD4, PAD1, OFF1 = "contig", "pad4", "pad1", "off1"
LAYOUTS = (CONTIG, PAD4, PAD1, OFF1)
# W and V hold d + 1 columns: pitch d + 4 (float4 when d % 4 == 0), d + 1 and d + 5 (element loads)
W_EXTRA = (4, 1, 5)


def pitch(layout, cols):
    return {CONTIG: cols, PAD4: cols + 4, PAD1: cols + 1, OFF1: cols // 4 * 4 + 4}[layout]


# ------------------------------------------------------------------ the host choices, restated

def sv_aligned(base_aligned, ld, cols):
    return base_aligned and ld % 4 == 0 and cols % 4 == 0 and cols >= 4


def layout_vec(layout, cols):
    return sv_aligned(layout != OFF1, pitch(layout, cols), cols)


def w_vec(extra, d):
    return sv_aligned(True, d + extra, d)


def sv_slice(n, d, c):
    tiles = ((c + BM - 1) // BM) * ((d + 1 + BN - 1) // BN)
    want = (TARGET_WGS + tiles - 1) // tiles
    sl = (n + want - 1) // want
    sl = (sl + BK - 1) // BK * BK
    return min(max(sl, MIN_SLICE), MAX_SLICE)


def n_slices(n, d, c):
    sl = sv_slice(n, d, c)
    return (n + sl - 1) // sl


def loss_blocks(n):
    return (n + LOSS_ROWS - 1) // LOSS_ROWS


# ------------------------------------------------------------------ case tables (the only statement of what runs)

# (n, d, c); every case runs GRAD, HV (on the mask GRAD stored) and SCORE under every pair of LAYOUTS (X) x W_EXTRA (W and V)
MARGIN_CASES = [
    (1, 1, 3),              # minimum sizes
    (129, 4, 4),            # minimal float4 width (the kend - 4 = 0 clamp); one row past a tile
    (127, 36, 129),         # float4 with a partial K chunk; a second column tile of one column; 5 mask words, one bit in the last
    (128, 32, 128),         # exact tiles, one K chunk
    (257, 33, 97),          # element loads only; one element past a K chunk; 3 row tiles; 5 loss blocks, the last of one row
    (65, 64, 132),          # two exact K chunks
    (130, 100, 33),         # product-like width
    (64, 128, 260),         # three column tiles
    (300, 132, 3),          # minimum class count
]
# Gaussian inputs at the product's depths, (n, d, c, X layout): W and V at pitch d + 4 (float4), X float4 and element loads
MARGIN_TOL_CASES = [(130, 1000, 100, CONTIG), (130, 1000, 100, PAD1), (130, 100, 1000, CONTIG), (130, 100, 1000, PAD1)]

REDUCE_CASES = [
    (1, 1, 3),              # minimum sizes
    (257, 4, 4),            # both operands at minimal float4 width; 2 slices, the last of one row
    (513, 127, 128),        # d + 1 = 128: exactly one feature tile; element X; float4 Z
    (300, 128, 129),        # the ones column alone in a second feature tile (k0 == D) under float4 X; two class tiles; element Z
    (4097, 100, 100),       # product-like; 17 slices, the last of one row
    (8200, 36, 7),          # many slices, ragged Z
    (70000, 259, 260),      # 9 tiles: slice length 320, above the 256 minimum
    (135000, 1000, 1000),   # 64 tiles: the 4096 clamp, 33 slices
]
BIG_REDUCE = (135000, 1000, 1000)   # its float64 reference comes from the device (torch.matmul); the others use NumPy
# (Z layout, X layout) of the cases too large for the whole product: one pair per (VZ, VX), every layout once per operand
LARGE_PAIRS = [(CONTIG, CONTIG), (PAD4, OFF1), (OFF1, PAD4), (PAD1, PAD1)]

GRAM_LENS = (1, 255, 256, 257, 1001)
GRAM_ROWS = (1, 37)
AXPBY_SHAPE = (1100, 1001, 1004)    # c, len, ld: more than 4096 x 256 elements, a second trip of the grid-stride loop

# solver primitives: (D, classes) with n = 300; ldv = D + 1 rounded up to 4, so D = 36 gives float4 weights and D = 33 element loads.
# The 40-class problem has two mask words, so its subsets run with a mask pitch above their word count.
SOLVER_N = 300
SOLVER_PROBLEMS = [(36, 12), (33, 12), (36, 40)]


def solver_column_sets(classes):
    return [np.arange(classes), np.array([1, 4, 5, 9, 11]), np.array([2, 7, 10]), np.array([0, 3, 6, 8])]


def reduce_pairs(case):
    n, d, c = case
    return LARGE_PAIRS if n >= 70000 else list(itertools.product(LAYOUTS, LAYOUTS))


def case_id(c):
    return "n%d-d%d-c%d" % tuple(c[:3]) + ("-" + c[3] if len(c) > 3 else "")


# ------------------------------------------------------------------ inputs on the grid, float64 references, comparators

def quarters(rng, lo, hi, shape):
    """Multiples of 1/4 in [lo, hi], float32."""
    return (rng.integers(4 * lo, 4 * hi + 1, shape) * 0.25).astype(np.float32)


def margin_inputs(case):
    """X in {-1, 0, 1}, W and V multiples of 1/4 in [-1, 1] (bias in column d); some labels match no column, the columns are a
    permutation of the classes."""
    n, d, c = case
    rng = np.random.default_rng(n * 7 + d * 3 + c)
    X = rng.integers(-1, 2, (n, d)).astype(np.float32)
    W, V = quarters(rng, -1, 1, (c, d + 1)), quarters(rng, -1, 1, (c, d + 1))
    labels = rng.integers(0, c + 2, n).astype(np.int32)
    perm = rng.permutation(c + 2).astype(np.int32)
    col_class = perm[:c]
    labels[n // 2] = perm[c]                    # a class without a column, whatever the draw
    return X, W, V, labels, col_class


def pack_bits(viol):
    """[n, c] bool -> [n, ceil(c / 32)] uint32: bit j % 32 of word j / 32."""
    n, c = viol.shape
    words = (c + 31) // 32
    padded = np.zeros((n, words * 32), dtype=np.uint64)
    padded[:, :c] = viol
    return (padded.reshape(n, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def margin_reference(X, W, V, labels, col_class, strict=True, bias_col=None):
    """The three epilogues in float64.  strict=False takes ``t >= 0`` for ``t > 0`` and bias_col another bias column: the defects the
    mutation test feeds back."""
    n, d = X.shape
    X64, W64, V64 = X.astype(np.float64), W.astype(np.float64), V.astype(np.float64)
    b = d if bias_col is None else bias_col
    M = X64 @ W64[:, :d].T + W64[:, b]
    Y = np.where(labels[:, None] == col_class[None, :], 1.0, -1.0)
    T = 1.0 - Y * M
    viol = T > 0 if strict else T >= 0
    Mv = X64 @ V64[:, :d].T + V64[:, b]
    L = np.where(viol, T * T, 0.0)
    loss = np.stack([L[k * LOSS_ROWS:(k + 1) * LOSS_ROWS].sum(axis=0) for k in range(loss_blocks(n))], axis=1)
    return {"M": M + 0.0, "T": T, "viol": viol, "Z": np.where(viol, -2 * CPEN * Y * T, 0.0), "words": pack_bits(viol), "loss": loss,
            "Zh": np.where(viol, 2 * CPEN * Mv, 0.0) + 0.0}


def assert_margin_on_grid(X, W, V, ref):
    """max(|X||W| + |b|) in units of 1/4 and the largest 64-row loss sum in units of 1/16 stay below 2^24."""
    d = X.shape[1]
    for P in (W, V):
        P64 = np.abs(P.astype(np.float64))
        assert (np.abs(X.astype(np.float64)) @ P64[:, :d].T + P64[:, d]).max() * 4 < GRID_LIMIT
    assert ref["loss"].max() * 16 < GRID_LIMIT


def same_bits(got, want):
    """got (float32) holds exactly the bits of the float64 array want, which must itself be a float32 array's worth of values."""
    want32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), want), "the reference left the float32 grid"
    got = np.ascontiguousarray(got, dtype=np.float32)
    return got.shape == want32.shape and np.array_equal(got.view(np.uint32), want32.view(np.uint32))


def grad_mismatches(Z, words, loss, ref):
    """Names of the GRAD outputs that differ from the reference: Z, every mask word (bits past column c are zero in the reference),
    every loss partial in its own block."""
    bad = []
    if not same_bits(Z, ref["Z"]):
        bad.append("Z")
    if not np.array_equal(np.asarray(words).view(np.uint32), ref["words"]):
        bad.append("mask")
    if not same_bits(loss, ref["loss"]):
        bad.append("loss")
    return bad


def reduce_inputs(case):
    """Z multiples of 1/4 in [-4, 4] with half zeros and X in {-1, 0, 1}, both as int8 counts of their unit (the large cases
    upload these), drawn as bytes through a table (the largest case has 270 million entries); plus multiples of 1/4 in [-4, 4]."""
    n, d, c = case
    rng = np.random.default_rng(n + d + c)
    zt = np.zeros(256, dtype=np.int8)
    zt[128:] = np.repeat(np.array([v for v in range(-16, 17) if v], dtype=np.int8), 4)
    xt = (np.arange(256) % 3 - 1).astype(np.int8)
    Z4 = zt[np.frombuffer(rng.bytes(n * c), dtype=np.uint8)].reshape(n, c)
    X1 = xt[np.frombuffer(rng.bytes(n * d), dtype=np.uint8)].reshape(n, d)
    P = quarters(rng, -4, 4, (c, d + 1))
    return Z4, X1, P


def assert_reduce_on_grid(Z4, P):
    """max(|plus| + |Z|^T |[X | 1]|) in units of 1/4 stays below 2^24.  |X| <= 1, so the ones column holds the largest sum of every
    class: max |plus| + max_c sum_i |Z[i, c]| bounds the whole table."""
    colsum = np.abs(Z4).sum(axis=0, dtype=np.int64)         # already in units of 1/4
    assert np.abs(P).max() * 4 + colsum.max() < GRID_LIMIT


def reduce_reference(Z4, X1, P, ones=True, omit_row=None, plus_times=1):
    """plus + Z^T [X | 1] in float64.  ones=False drops the ones column, omit_row one row of the sum, plus_times = 2 adds plus
    twice: the defects the mutation test feeds back."""
    Z = Z4.astype(np.float64) * 0.25
    Xa = np.hstack([X1.astype(np.float64), np.full((len(X1), 1), 1.0 if ones else 0.0)])
    if omit_row is not None:
        Z = Z.copy()
        Z[omit_row] = 0
    G = Z.T @ Xa
    return G + plus_times * P.astype(np.float64) if P is not None else G + 0.0


# ------------------------------------------------------------------ CPU: the tables reach every path

def test_margin_case_table_reaches_every_path():
    seen = set()
    for (n, d, c), xl, we in itertools.product(MARGIN_CASES, LAYOUTS, W_EXTRA):
        for mode in (GRAD, HV, SCORE):
            seen.add((mode, layout_vec(xl, d), w_vec(we, d)))
    assert seen == set(itertools.product((GRAD, HV, SCORE), (False, True), (False, True)))
    # the float4 pairs the product runs with, at its depths, under a tolerance
    assert {(layout_vec(xl, d), w_vec(4, d)) for n, d, c, xl in MARGIN_TOL_CASES} == {(True, True), (False, True)}
    assert {(d, c) for n, d, c, xl in MARGIN_TOL_CASES} == {(1000, 100), (100, 1000)}
    # every reason an operand takes the element path although d % 4 == 0: pitch, base; and d % 4 != 0
    assert any(d % 4 == 0 and pitch(xl, d) % 4 for (n, d, c), xl in itertools.product(MARGIN_CASES, LAYOUTS))
    assert any(d % 4 == 0 and xl == OFF1 and pitch(xl, d) % 4 == 0 for (n, d, c), xl in itertools.product(MARGIN_CASES, LAYOUTS))
    assert any(d % 4 for n, d, c in MARGIN_CASES) and any(d == 4 for n, d, c in MARGIN_CASES)
    vec_d = {d for n, d, c in MARGIN_CASES if d % 4 == 0}
    assert any(d % BK for d in vec_d) and any(d % BK == 0 and d > BK for d in vec_d) and any(d % BK == 1 for n, d, c in MARGIN_CASES)
    assert any(c % BN == 1 and c > BN for n, d, c in MARGIN_CASES)             # a one-column tile
    assert any(c % 32 == 1 and c > 32 for n, d, c in MARGIN_CASES)             # a one-bit mask word
    assert any(n % LOSS_ROWS == 1 and n > LOSS_ROWS for n, d, c in MARGIN_CASES)   # a one-row loss block
    assert any(n % BM == 1 and n > BM for n, d, c in MARGIN_CASES) and any(n % BM == 0 and c % BN == 0 for n, d, c in MARGIN_CASES)
    assert any(c == 3 for n, d, c in MARGIN_CASES) and any(c > 2 * BN for n, d, c in MARGIN_CASES)
    assert len(set(MARGIN_CASES)) == len(MARGIN_CASES)


def test_reduce_case_table_reaches_every_path():
    seen, slices = set(), set()
    for case in REDUCE_CASES:
        n, d, c = case
        for zl, xl in reduce_pairs(case):
            seen.add((layout_vec(zl, c), layout_vec(xl, d)))
        slices.add(sv_slice(n, d, c))
    assert seen == set(itertools.product((False, True), repeat=2))
    assert MIN_SLICE in slices and MAX_SLICE in slices and any(MIN_SLICE < s < MAX_SLICE for s in slices)
    assert sv_slice(70000, 259, 260) == 320 and sv_slice(*BIG_REDUCE) == MAX_SLICE and n_slices(*BIG_REDUCE) == 33
    # a last slice of one row, with float4 loads of both operands and with element loads of Z
    one_row = [c for c in REDUCE_CASES if c[0] % sv_slice(*c) == 1 and n_slices(*c) > 1]
    assert any(layout_vec(CONTIG, c[2]) and layout_vec(CONTIG, c[1]) for c in one_row)
    assert any(n_slices(*c) == 17 for c in one_row)
    # k0 == D: the ones column alone in the last feature tile, under float4 X (whose clamp then reads columns D - 4 .. D - 1)
    assert any(d % BN == 0 and any(layout_vec(xl, d) for zl, xl in reduce_pairs((n, d, c))) for n, d, c in REDUCE_CASES)
    assert any((d + 1) % BN == 0 for n, d, c in REDUCE_CASES)                  # exactly full feature tiles
    assert any(c % BM == 1 and c > BM for n, d, c in REDUCE_CASES)             # a one-class tile
    assert any(c % 4 and n_slices(n, d, c) > 2 for n, d, c in REDUCE_CASES)    # ragged Z over many slices
    # the large cases launch all four instantiations between them, and the largest one alone does too
    assert {(layout_vec(zl, 1000), layout_vec(xl, 1000)) for zl, xl in LARGE_PAIRS} == set(itertools.product((False, True), repeat=2))
    assert {l for p in LARGE_PAIRS for l in p} == set(LAYOUTS)
    assert len(set(REDUCE_CASES)) == len(REDUCE_CASES)


def test_small_kernel_and_solver_tables_reach_every_path():
    c, length, ld = AXPBY_SHAPE
    assert c * length > AXPBY_GRID_CAP * 256 and ld > length
    assert {1, 255, 256, 257} <= set(GRAM_LENS) and any(l > 3 * 256 for l in GRAM_LENS)        # below, at and past one block trip
    ldv = lambda D: (D + 1 + 3) // 4 * 4                                                       # noqa: E731
    assert {sv_aligned(True, ldv(D), D) for D, classes in SOLVER_PROBLEMS} == {False, True}
    for D, classes in SOLVER_PROBLEMS:
        sizes = [len(s) for s in solver_column_sets(classes)]
        assert sizes[0] == classes and min(sizes) == 3 and all(s.max() < classes for s in solver_column_sets(classes))
        assert any(np.any(np.diff(s) != 1) for s in solver_column_sets(classes))               # a non-contiguous subset
    # float4 Z views of the solver (rows % 4 == 0 out of a wider buffer) and ragged ones; a mask pitch above the word count
    assert {len(s) % 4 == 0 for D, classes in SOLVER_PROBLEMS for s in solver_column_sets(classes)} == {False, True}
    assert any((classes + 31) // 32 > (len(s) + 31) // 32 for D, classes in SOLVER_PROBLEMS for s in solver_column_sets(classes))


# ------------------------------------------------------------------ CPU: the exact cases stay on the grid

@pytest.mark.parametrize("case", MARGIN_CASES, ids=case_id)
def test_margin_inputs_stay_on_the_grid(case):
    X, W, V, labels, col_class = margin_inputs(case)
    ref = margin_reference(X, W, V, labels, col_class)
    assert_margin_on_grid(X, W, V, ref)
    n, d, c = case
    zero = int((ref["T"] == 0).sum())
    print("%s: %d entries with T == 0, largest |M| %.2f, largest loss partial %.2f" % (case_id(case), zero, np.abs(ref["M"]).max(),
                                                                                      ref["loss"].max()))
    if n >= 64:
        assert zero > 0
    assert n == 1 or not (labels[:, None] == col_class[None, :]).any(axis=1).all()      # some labels match no column
    assert len(set(col_class)) == c and not np.array_equal(col_class, np.arange(c))
    if n >= 64:
        assert ref["viol"].any() and not ref["viol"].all()


@pytest.mark.parametrize("case", REDUCE_CASES, ids=case_id)
def test_reduce_inputs_stay_on_the_grid(case):
    Z4, X1, P = reduce_inputs(case)
    assert_reduce_on_grid(Z4, P)
    assert X1.min() >= -1 and X1.max() <= 1 and Z4.min() >= -16 and Z4.max() <= 16
    if Z4.size > 1000:
        assert 0.4 < (Z4 == 0).mean() < 0.6


def solver_problem(D, classes):
    rng = np.random.default_rng(1000 + D + classes)
    X = rng.integers(-1, 2, (SOLVER_N, D)).astype(np.float32)
    y = rng.integers(0, classes, SOLVER_N)
    return rng, X, y


def solver_vectors(rng, rows, D):
    """W, V (multiples of 1/4 in [-1, 1]) and axpby coefficients (multiples of 1/4 in [-2, 2]), float64."""
    W, V = quarters(rng, -1, 1, (rows, D + 1)).astype(np.float64), quarters(rng, -1, 1, (rows, D + 1)).astype(np.float64)
    return W, V, rng.integers(-8, 9, rows) / 4.0, rng.integers(-8, 9, rows) / 4.0


@pytest.mark.parametrize("D,classes", SOLVER_PROBLEMS)
def test_solver_problems_stay_on_the_grid(D, classes):
    """Margins, loss partials, gradient and Hessian-vector product of the solver problems, from the float64 host primitives."""
    import linear_svm as ls
    rng, X, y = solver_problem(D, classes)
    hops = ls._HostOps(X, y, CPEN, classes)
    for cols in solver_column_sets(classes):
        hops.set_columns(cols)
        W, V, al, be = solver_vectors(rng, len(cols), D)
        ref = margin_reference(X, W.astype(np.float32), V.astype(np.float32), y.astype(np.int32), cols.astype(np.int32))
        assert_margin_on_grid(X, W, V, ref)
        assert (ref["T"] == 0).any()
        Xa = np.abs(hops.Xa)
        assert (np.abs(W) + np.abs(ref["Z"]).T @ Xa).max() * 4 < GRID_LIMIT
        assert (np.abs(V) + np.abs(ref["Zh"]).T @ Xa).max() * 4 < GRID_LIMIT
        f, G, gg = hops.fg(W)
        assert np.array_equal(G, W + ref["Z"].T @ hops.Xa) and np.array_equal(hops.A, ref["viol"])
        assert np.abs(G).max() * 4 < GRID_LIMIT and gg.max() * 16 < 2.0 ** 53
        assert np.abs(hops.axpby(al, G, be, hops.hv(V))).max() * 16 < GRID_LIMIT


# ------------------------------------------------------------------ CPU: the comparators reject every defect

def test_comparator_rejects_mutated_oracle_outputs():
    """The exact comparators accept the float64 reference and reject it with one defect at a time: ``>=`` for ``>`` at T == 0, one
    mask bit flipped, the mask words shifted by one column block, a loss partial moved to the next block, the bias taken from
    column d - 1, the ones column dropped from the reduction, the last row of one slice omitted, ``plus`` added twice."""
    case = (127, 36, 129)
    n, d, c = case
    inp = margin_inputs(case)
    ref = margin_reference(*inp)
    f32 = lambda a: a.astype(np.float32)                                                       # noqa: E731
    assert grad_mismatches(f32(ref["Z"]), ref["words"].view(np.int32), f32(ref["loss"]), ref) == []
    assert same_bits(f32(ref["Zh"]), ref["Zh"]) and same_bits(f32(ref["M"]), ref["M"])
    # >= at T == 0: the mask alone shows it (Z and the loss gain zeros), and so does the Hessian-vector product on that mask
    assert (ref["T"] == 0).sum() > 100
    ge = margin_reference(*inp, strict=False)
    assert "mask" in grad_mismatches(f32(ref["Z"]), ge["words"], f32(ref["loss"]), ref)
    assert np.array_equal(np.abs(ge["Z"]), np.abs(ref["Z"])) and np.array_equal(ge["loss"], ref["loss"])
    assert not same_bits(f32(ge["Zh"]), ref["Zh"])
    # one mask bit: the single bit of the last word, a padding bit past column c, the top bit of a first word
    for row, word, bit in ((5, 4, 0), (5, 4, 1), (n - 1, 0, 31)):
        flipped = ref["words"].copy()
        flipped[row, word] ^= np.uint32(1 << bit)
        assert grad_mismatches(f32(ref["Z"]), flipped, f32(ref["loss"]), ref) == ["mask"]
    # the words of one row written one column block further
    assert grad_mismatches(f32(ref["Z"]), np.roll(ref["words"], 1, axis=1), f32(ref["loss"]), ref) == ["mask"]
    # a loss partial in the neighbouring block
    assert ref["loss"].shape == (c, 2)
    assert grad_mismatches(f32(ref["Z"]), ref["words"], f32(ref["loss"][:, ::-1]), ref) == ["loss"]
    moved = ref["loss"].copy()
    moved[7] = moved[7, ::-1]
    assert grad_mismatches(f32(ref["Z"]), ref["words"], f32(moved), ref) == ["loss"]
    # the bias from column d - 1: all three modes
    wb = margin_reference(*inp, bias_col=d - 1)
    assert set(grad_mismatches(f32(wb["Z"]), wb["words"], f32(wb["loss"]), ref)) == {"Z", "mask", "loss"}
    assert not same_bits(f32(wb["Zh"]), ref["Zh"]) and not same_bits(f32(wb["M"]), ref["M"])
    # the reduction
    rcase = (513, 127, 128)
    Z4, X1, P = reduce_inputs(rcase)
    want = reduce_reference(Z4, X1, P)
    assert same_bits(f32(want), want)
    sl = sv_slice(*rcase)
    assert sl == 256 and Z4[sl - 1].any() and X1[sl - 1].any()
    for bad in (reduce_reference(Z4, X1, P, ones=False), reduce_reference(Z4, X1, P, omit_row=sl - 1),
                reduce_reference(Z4, X1, P, omit_row=2 * sl - 1), reduce_reference(Z4, X1, P, plus_times=2)):
        assert not same_bits(f32(bad), want)
    assert not same_bits(f32(want), reduce_reference(Z4, X1, None))                            # plus = None adds nothing


# ------------------------------------------------------------------ GPU helpers

@pytest.fixture(scope="module")
def sehip():
    import sehip as m
    m.lib()
    return m


SENT = np.int32(0x7FC0DEAD)         # a quiet NaN with a payload no kernel writes


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def place(t, ld, off=0):
    """Device copy of the float32 matrix ``t`` (NumPy or device tensor) as a view of pitch ``ld`` starting ``off`` floats into its
    storage; every other element of the storage holds the NaN sentinel."""
    import torch
    if not torch.is_tensor(t):
        t = dev(np.asarray(t, dtype=np.float32))
    rows, cols = t.shape
    buf = torch.full((rows * ld + 8,), int(SENT), dtype=torch.int32, device="cuda").view(torch.float32)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(t)
    assert v.stride(0) == ld and v.data_ptr() % 16 == 4 * off
    v.whole = buf
    return v


def place_layout(t, layout):
    return place(t, pitch(layout, t.shape[1]), 1 if layout == OFF1 else 0)


def untouched(v):
    """The storage of a view made by place() still holds the sentinel everywhere outside the view."""
    import torch
    rows, cols = v.shape
    whole = v.whole.view(torch.int32).cpu().numpy()
    inside = np.zeros(whole.shape, dtype=bool)
    idx = v.storage_offset() + (np.arange(rows)[:, None] * v.stride(0) + np.arange(cols)[None, :])
    inside[idx.ravel()] = True
    return bool((whole[~inside] == SENT).all())


class Out:
    """A caller output of ``rows`` x ``cols`` (pitch ``ld``), a sentinel guard row before and after it, sentinel pitch padding."""

    def __init__(self, rows, cols, ld, kind="f32"):
        import torch
        self.rows, self.cols = rows, cols
        self.buf = torch.full((rows + 2, ld), int(SENT), dtype=torch.int32, device="cuda")
        self.view = (self.buf.view(torch.float32) if kind == "f32" else self.buf)[1:rows + 1, :cols]

    def bits(self):
        """The output's bits (int32); asserts every element around it still holds the sentinel."""
        b = self.buf.cpu().numpy()
        inside = np.zeros(b.shape, dtype=bool)
        inside[1:self.rows + 1, :self.cols] = True
        assert (b[~inside] == SENT).all(), "a store left the output (pitch padding or guard rows)"
        return b[1:self.rows + 1, :self.cols].copy()

    def f32(self):
        return self.bits().view(np.float32)


# ------------------------------------------------------------------ GPU: margin kernel

@pytest.mark.gpu
@pytest.mark.parametrize("case", MARGIN_CASES, ids=case_id)
def test_margin_every_instantiation_equals_float64(sehip, case):
    n, d, c = case
    X, W, V, labels, col_class = margin_inputs(case)
    ref = margin_reference(X, W, V, labels, col_class)
    assert_margin_on_grid(X, W, V, ref)
    if n >= 64:
        assert (ref["T"] == 0).any()
    words, nblk = (c + 31) // 32, loss_blocks(n)
    assert sehip.ops.svm_loss_blocks(n) == nblk
    ld_, cd = dev(labels), dev(col_class)
    Xb, Wb, Vb = dev(X), dev(W), dev(V)
    launched = set()
    for xl in LAYOUTS:
        Xd = place_layout(Xb, xl)
        for we in W_EXTRA:
            Wd, Vd = place(Wb, d + we), place(Vb, d + we)
            tag = (xl, we)
            launched.add((layout_vec(xl, d), w_vec(we, d)))
            Z, mask, loss = Out(n, c, c + 3), Out(n, words, words + 1, "i32"), Out(c, nblk, nblk + 2)
            sehip.svm_margin(sehip.SVM_GRAD, Xd, Wd, d=d, labels=ld_, col_class=cd, cpen=CPEN, mask=mask.view, out=Z.view,
                             loss_part=loss.view)
            stored = mask.bits()
            assert grad_mismatches(Z.f32(), stored, loss.f32(), ref) == [], tag
            # Hessian-vector mode on the stored mask: 2 cpen (X v + v_b) where the bit is set, +0 elsewhere
            Zh = Out(n, c, c + 3)
            sehip.svm_margin(sehip.SVM_HV, Xd, Vd, d=d, cpen=CPEN, mask=mask.view, out=Zh.view)
            assert same_bits(Zh.f32(), ref["Zh"]), tag
            assert np.array_equal(mask.bits(), stored), tag
            S = Out(n, c, c + 3)
            sehip.svm_margin(sehip.SVM_SCORE, Xd, Wd, d=d, out=S.view)
            assert same_bits(S.f32(), ref["M"]), tag
            assert untouched(Wd) and untouched(Vd), tag
        assert untouched(Xd), xl
    print("%s: svm_margin_kernel<GRAD|HV|SCORE, VX, VW> launched with (VX, VW) in %s; %d entries with T == 0"
          % (case_id(case), sorted(launched), int((ref["T"] == 0).sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MARGIN_TOL_CASES, ids=case_id)
def test_margin_float4_paths_at_product_depth(sehip, case):
    """Gaussian X and W at D = 1000 and C = 1000 with float4 weights (pitch d + 4) and float4 / element X, under the bound
    4 d eps32 (|x||w| + |b|) of a float32 sum of d terms (tests/test_gpu_svm.py derives it)."""
    n, d, c, xl = case
    assert w_vec(4, d)
    rng = np.random.default_rng(n * 7 + d * 3 + c)
    X = rng.standard_normal((n, d)).astype(np.float32)
    W = (rng.standard_normal((c, d + 1)) / np.sqrt(d)).astype(np.float32)
    V = rng.standard_normal((c, d + 1)).astype(np.float32)
    labels = rng.integers(0, c + 2, n).astype(np.int32)
    col_class = rng.permutation(c + 2)[:c].astype(np.int32)
    cpen = 0.7
    Xd, Wd, Vd = place_layout(X, xl), place(W, d + 4), place(V, d + 4)
    words, nblk = (c + 31) // 32, loss_blocks(n)
    Z, mask, loss = Out(n, c, c + 3), Out(n, words, words + 1, "i32"), Out(c, nblk, nblk + 2)
    sehip.svm_margin(sehip.SVM_GRAD, Xd, Wd, d=d, labels=dev(labels), col_class=dev(col_class), cpen=cpen, mask=mask.view, out=Z.view,
                     loss_part=loss.view)
    X64, W64, V64 = X.astype(np.float64), W.astype(np.float64), V.astype(np.float64)
    M = X64 @ W64[:, :d].T + W64[:, d]
    bound = 4 * d * EPS32 * (np.abs(X64) @ np.abs(W64[:, :d]).T + np.abs(W64[:, d])) + 1e-30
    Y = np.where(labels[:, None] == col_class[None, :], 1.0, -1.0)
    T = 1.0 - Y * M
    Zref = np.where(T > 0, -2 * cpen * Y * T, 0.0)
    z = Z.f32()
    assert np.all(np.abs(z - Zref) <= 2 * cpen * bound * 1.01 + 4 * EPS32 * np.abs(Zref))
    m = mask.bits().view(np.uint32)
    bits = ((m[:, np.arange(c) // 32] >> (np.arange(c) % 32).astype(np.uint32)) & 1).astype(bool)
    sure = np.abs(T) > bound
    assert sure.mean() > 0.9 and np.array_equal(bits[sure], (T > 0)[sure])
    assert np.array_equal(bits, z != 0) or np.all((z != 0) <= bits)
    if c % 32:
        assert np.all(m[:, -1] >> np.uint32(c % 32) == 0)
    lp = loss.f32()
    Lref = np.where(bits, np.maximum(T, 0.0) ** 2, 0.0)
    for b in range(nblk):
        rows = slice(b * LOSS_ROWS, (b + 1) * LOSS_ROWS)
        want = Lref[rows].sum(axis=0)
        slack = (2 * np.abs(T[rows]) * bound[rows] + bound[rows] ** 2).sum(axis=0)
        assert np.all(np.abs(lp[:, b] - want) <= 1.01 * slack + 64 * EPS32 * want + 1e-30)
    Zh = Out(n, c, c + 3)
    sehip.svm_margin(sehip.SVM_HV, Xd, Vd, d=d, cpen=cpen, mask=mask.view, out=Zh.view)
    Mv = X64 @ V64[:, :d].T + V64[:, d]
    bv = 4 * d * EPS32 * (np.abs(X64) @ np.abs(V64[:, :d]).T + np.abs(V64[:, d]))
    assert np.all(np.abs(Zh.f32() - np.where(bits, 2 * cpen * Mv, 0.0)) <= 2 * cpen * bv * 1.01 + 1e-30)
    S = Out(n, c, c + 3)
    sehip.svm_margin(sehip.SVM_SCORE, Xd, Wd, d=d, out=S.view)
    assert np.all(np.abs(S.f32() - M) <= bound * 1.01)
    print("%s: svm_margin_kernel<GRAD|HV|SCORE, %s, true>" % (case_id(case), str(layout_vec(xl, d)).lower()))


# ------------------------------------------------------------------ GPU: reduce kernel

@pytest.mark.gpu
@pytest.mark.parametrize("case", REDUCE_CASES, ids=case_id)
def test_reduce_every_instantiation_equals_float64(sehip, case):
    import torch
    n, d, c = case
    Z4, X1, P = reduce_inputs(case)
    assert_reduce_on_grid(Z4, P)
    sl = sv_slice(n, d, c)
    assert sehip.svm_reduce_workspace_bytes(n, d, c) == (n + sl - 1) // sl * c * (d + 1) * 4
    Zb, Xb, Pb = dev(Z4).float().mul_(0.25), dev(X1).float(), dev(P)
    if case == BIG_REDUCE:          # exact integers and quarter-integers: any correct float64 summation gives these bits
        G64 = torch.matmul(Zb.double().t(), torch.cat([Xb.double(), torch.ones((n, 1), dtype=torch.float64, device="cuda")], dim=1))
        want = {True: (G64 + Pb.double()).cpu().numpy(), False: (G64 + 0.0).cpu().numpy()}
        del G64
    else:
        want = {True: reduce_reference(Z4, X1, P), False: reduce_reference(Z4, X1, None)}
    del Z4, X1
    launched = set()
    for zl, xl in reduce_pairs(case):
        launched.add((layout_vec(zl, c), layout_vec(xl, d)))
        Zd, Xd = place_layout(Zb, zl), place_layout(Xb, xl)
        for plus in (True, False):
            Pd = place(Pb, d + 6) if plus else None
            first, again = Out(c, d + 1, d + 4), Out(c, d + 1, d + 4)
            sehip.svm_reduce(Zd, Xd, d=d, plus=Pd, out=first.view)
            sehip.svm_reduce(Zd, Xd, d=d, plus=Pd, out=again.view)
            got = first.f32()
            assert same_bits(got, want[plus]), (zl, xl, plus)
            assert np.array_equal(again.bits(), got.view(np.int32)), (zl, xl, plus)
        if n < 70000:
            assert untouched(Zd) and untouched(Xd)
        del Zd, Xd
    print("%s: svm_reduce_kernel<VZ, VX> launched with (VZ, VX) in %s; slice %d, %d slices, last of %d rows"
          % (case_id(case), sorted(launched), sl, (n + sl - 1) // sl, n - (n - 1) // sl * sl))


# ------------------------------------------------------------------ GPU: gram, rowsum, axpby

def pair_dots(vs):
    return np.stack([np.sum(vs[a] * vs[b], axis=1) for a in range(len(vs)) for b in range(a, len(vs))], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("c", GRAM_ROWS)
@pytest.mark.parametrize("length", GRAM_LENS)
def test_gram_and_rowsum_equal_float64(sehip, c, length):
    """Quarter-integer vectors: every product and sum is exact in float64, so the documented pair order (a <= b, row-major) and
    the row sums come out bit for bit, from rows whose pitch padding holds NaN."""
    rng = np.random.default_rng(c * 10000 + length)
    V = [quarters(rng, -4, 4, (c, length)) for _ in range(4)]
    Vd = [place(v, length + 3) for v in V]
    V64 = [v.astype(np.float64) for v in V]
    for nv in (1, 2, 3, 4):
        q = sehip.svm_gram(Vd[:nv], length=length)
        assert q.dtype.is_floating_point and q.element_size() == 8 and tuple(q.shape) == (c, nv * (nv + 1) // 2)
        assert np.array_equal(q.cpu().numpy(), pair_dots(V64[:nv])), nv
        last = sehip.svm_gram(Vd[4 - nv:], length=length)          # other vectors in the same slots
        assert np.array_equal(last.cpu().numpy(), pair_dots(V64[4 - nv:])), nv
    for v, v64 in zip(Vd, V64):
        assert np.array_equal(sehip.svm_rowsum(v, length=length).cpu().numpy(), v64.sum(axis=1))
        assert untouched(v)


@pytest.mark.gpu
def test_axpby_second_grid_trip_aliasing_and_padding(sehip):
    """out = (float32)(alpha x + beta y) in float64 past the grid cap, with out aliased to x and to y.  alpha and beta carry six
    significant bits, so both float64 products are exact and the sum rounds once, fused or not; the float32 rounding is the
    kernel's own."""
    c, length, ld = AXPBY_SHAPE
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal((c, length)).astype(np.float32), rng.standard_normal((c, length)).astype(np.float32)
    al, be = rng.integers(-32, 33, c) / 8.0, rng.integers(-32, 33, c) / 8.0
    want = (al[:, None] * x.astype(np.float64) + be[:, None] * y.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(want.astype(np.float64), al[:, None] * x.astype(np.float64) + be[:, None] * y.astype(np.float64))
    ald, bed = dev(al), dev(be)
    xd, yd = place(x, ld), place(y, ld)
    out = Out(c, length, ld)
    r = sehip.svm_axpby(ald, xd, bed, yd, out=out.view, length=length)
    assert r.data_ptr() == out.view.data_ptr()
    assert np.array_equal(out.bits(), want.view(np.int32))
    assert untouched(xd) and untouched(yd)
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(yd.cpu().numpy(), y)
    sehip.svm_axpby(ald, xd, bed, yd, out=xd, length=length)                    # out is x
    assert np.array_equal(xd.cpu().numpy().view(np.int32), want.view(np.int32)) and untouched(xd)
    xd = place(x, ld)
    sehip.svm_axpby(ald, xd, bed, yd, out=yd, length=length)                    # out is y
    assert np.array_equal(yd.cpu().numpy().view(np.int32), want.view(np.int32)) and untouched(yd)
    assert np.array_equal(xd.cpu().numpy(), x)


# ------------------------------------------------------------------ GPU: the solver's primitives, device against host

@pytest.mark.gpu
@pytest.mark.parametrize("D,classes", SOLVER_PROBLEMS)
def test_solver_primitives_equal_the_host_ops(sehip, D, classes):
    """_DeviceOps.fg / hv / gram / axpby against _HostOps on exact problems, for the whole class set and for the subsets a
    shrinking working set leaves: a Z[:, :rows] view of the full-width buffer, the full-width mask, loss[:rows]."""
    import torch
    import linear_svm as ls
    rng, X, y = solver_problem(D, classes)
    hops = ls._HostOps(X, y, CPEN, classes)
    dops = ls._DeviceOps(dev(X), y, CPEN, classes)
    assert dops.ldv == (D + 1 + 3) // 4 * 4 and dops.Z.shape[1] == classes

    def vec(a):
        v = dops.zeros(a.shape[0])
        v[:, :D + 1] = dev(a, torch.float32)
        return v

    def host(v):
        a = v.cpu().numpy()
        assert not a[:, D + 1:].any(), "the padding columns of a solver vector must stay zero"
        return a[:, :D + 1].astype(np.float64)

    for cols in solver_column_sets(classes):
        rows = len(cols)
        hops.set_columns(cols)
        dops.set_columns(cols)
        dops.Z.fill_(float("nan"))              # sentinels in the buffers a subset only partly overwrites
        dops.mask.fill_(-1)
        dops.loss.fill_(float("nan"))
        W, V, al, be = solver_vectors(rng, rows, D)
        Wd, Vd = vec(W), vec(V)
        f, G, gg = hops.fg(W)
        fd, Gd, ggd = dops.fg(Wd)
        assert np.array_equal(fd, f) and np.array_equal(host(Gd), G) and np.array_equal(ggd, gg), rows
        Hv = hops.hv(V)
        Hd = dops.hv(Vd)
        assert np.array_equal(host(Hd), Hv), rows
        assert np.array_equal(dops.gram([Wd, Gd, Vd, Hd]), hops.gram([W, G, V, Hv])), rows
        assert np.array_equal(dops.gram([Gd, Hd]), hops.gram([G, Hv])), rows
        want = hops.axpby(al, G, be, Hv)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        assert np.array_equal(host(dops.axpby(al, Gd, be, Hd)), want), rows
        # the working set's columns were written, the other columns of the shared buffers were not
        if rows < classes:
            assert torch.isnan(dops.Z[:, rows:]).all() and not torch.isnan(dops.Z[:, :rows]).any()
            assert torch.isnan(dops.loss[rows:]).all() and not torch.isnan(dops.loss[:rows]).any()
            used = (rows + 31) // 32
            assert (dops.mask[:, used:] == -1).all()
