"""The training-side kernels (csrc/loss_kernels.hip, devise.hip, labelembed.hip) through every path their host code can choose.

The host entry points pick a kernel instantiation from the feature dtype and the gradient dtype, switch between 16-byte and element
loads on ``D``, the row pitches and the pointer alignment (``vec_ok``; ``stage_tile32`` / ``tile32::load_rows`` decide again per operand inside
nn_accuracy), cap the grid of the row kernels (8,192 blocks of 4 rows; labelembed's ``le_grid`` at 4,096) and cut large class sets
into slices whose partial results meet in a finish kernel.  The functions below restate those choices in Python, and CPU tests hold
the case tables to every tuple of them, so that dropping a case can never silently drop a path.

Each case calls the C ABI directly: inputs sit in strided or column-offset views whose padding holds NaN, outputs go to caller
buffers whose pitch padding and guard rows hold a sentinel.  Results are compared with oracle/loss_oracle.py in float64, on the same
bf16-rounded inputs, under PER-ROW bounds (``bound``), and checked bit for bit wherever a kernel promises exactness: bf16 gradients
against the fp32 gradient of the same call rounded to nearest even, the batch mean against a float32 restatement of mean_kernel's
order, nn_accuracy's acc / best against its own returned scores, rows against the same rows in another batch (permuted, past the grid
cap, under another slice count), and out-of-range labels against the clamped labels.
"""
import itertools

import numpy as np
import pytest

from oracle import loss_oracle as lo

U = 2.0 ** -24                      # unit roundoff of float32
EPS32 = np.float32(1e-12)           # L2NORM_EPS
ROWS_PER_BLOCK = 4                  # LOSS_ROWS_PER_BLOCK / LE_ROWS_PER_BLOCK
ROW_GRID_CAP = 256 * 32             # blocks of the cosine / sqdist / l2norm row kernels
LE_GRID_CAP = 4096                  # le_grid
MARGIN = 0.1

# input layouts: contiguous rows; pitch padded to a multiple of 8 past D (NaN padding); a column slice at offset 1 (base off 16-byte
# alignment, NaN in the skipped column).  Every layout is followed by NaN guard rows.
CONTIG, PADDED, COL1 = "contig", "padded", "col1"
# output pitch: D (guard rows only) or D + 3 (pitch padding too; never a multiple of 4 when D is)
TIGHT, WIDE = "tight", "wide"
F32, BF16 = "f32", "bf16"


def pitch(layout, d):
    return {CONTIG: d, PADDED: (d // 8 + 2) * 8, COL1: d + 1}[layout]


def aligned(layout):
    return layout != COL1


def out_pitch(out, d):
    return d if out == TIGHT else d + 3


# ------------------------------------------------------------------ the host choices, restated

def row_grid_capped(B):
    return (B + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK > ROW_GRID_CAP


def le_grid_capped(B):
    return (B + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK > LE_GRID_CAP


def cos_vec(xdt, layout, d, xhat_out=None):
    """``vec_ok`` of se_cosine_loss_fwd (xhat_out = the xhat layout, None when xhat is NULL) and se_cosine_loss_bwd (None)."""
    vq = 8 if xdt == BF16 else 4
    ok = d % vq == 0 and pitch(layout, d) % vq == 0 and pitch(layout, d) % 4 == 0 and aligned(layout)
    if xhat_out is not None:        # the xhat view starts one guard row into its buffer: 16-byte aligned iff its pitch is
        ok = ok and out_pitch(xhat_out, d) % 4 == 0
    return ok


def sq_vec(xdt, layout, d):
    """``vec_ok`` of se_sqdist_loss_fwd (the backward and the l2norm kernels have element loads only)."""
    return xdt == F32 and d % 4 == 0 and pitch(layout, d) % 4 == 0 and aligned(layout)


def nn_acc_tiles_per_block(B, C):
    tiles, blocks = (C + 31) // 32, (B + 31) // 32
    if tiles <= 4 or blocks >= 1024:
        return tiles
    slices = min(1024 // blocks, tiles)
    return (tiles + slices - 1) // slices


def devise_tiles_per_block(B, C):
    tiles, blocks = (C + 31) // 32, (B + 31) // 32
    if tiles <= 2 or blocks >= 1024:
        return tiles
    slices = min(1024 // blocks, tiles)
    return (tiles + slices - 1) // slices


def n_slices(tpb, C):
    """gridDim.y: 1 writes the results directly, more go through the finish kernel."""
    tiles = (C + 31) // 32
    return (tiles + tpb - 1) // tpb


def stage_vec(layout, d):
    """stage_tile32's and tile32::load_rows' per-operand choice: ((ld | K) & 3) == 0 and a 16-byte aligned base."""
    return pitch(layout, d) % 4 == 0 and d % 4 == 0 and aligned(layout)


# ------------------------------------------------------------------ case tables (the only statement of what runs)

ALL, NONE = "all", "none"           # optional forward outputs (xhat / inv_norm / loss_mean; dist_i / loss_mean): all present or NULL

# (B, D, C, x dtype, layout, output pitch, optional outputs).  Every case runs cosine fwd + bwd (4 dtype pairs x per-row weights /
# scalar grad_scale), sqdist fwd + bwd (the same 8) and l2norm fwd + bwd.
ROW_CASES = [
    (1, 1, 1, F32, CONTIG, TIGHT, ALL),
    (3, 2, 5, F32, COL1, WIDE, NONE),
    (37, 3, 7, BF16, PADDED, WIDE, ALL),
    (37, 5, 33, BF16, CONTIG, TIGHT, NONE),
    (256, 16, 31, F32, CONTIG, TIGHT, ALL),           # 16-byte loads, xhat written with float4
    (255, 16, 31, F32, PADDED, WIDE, ALL),            # 16-byte loads of x, xhat pitch not a multiple of 4: fwd falls back
    (257, 64, 100, F32, PADDED, TIGHT, NONE),
    (300, 100, 33, F32, COL1, TIGHT, ALL),
    (5, 1000, 1000, F32, CONTIG, WIDE, ALL),
    (33, 12, 10, BF16, CONTIG, TIGHT, ALL),           # bf16, D % 8 == 4: element loads although D % 4 == 0
    (33, 12, 10, BF16, PADDED, WIDE, NONE),
    (130, 16, 3, BF16, CONTIG, TIGHT, ALL),           # bf16 16-byte loads (8 per lane)
    (70, 64, 3, BF16, PADDED, TIGHT, NONE),
    (66, 63, 1, BF16, COL1, WIDE, ALL),
    (9, 65, 31, F32, CONTIG, TIGHT, ALL),
    (2, 129, 1025, BF16, COL1, TIGHT, NONE),
    (7, 127, 1023, F32, PADDED, WIDE, ALL),
    (ROW_GRID_CAP * ROWS_PER_BLOCK + 3, 3, 5, F32, CONTIG, TIGHT, ALL),      # grid-stride loop, element loads
    (ROW_GRID_CAP * ROWS_PER_BLOCK + 37, 8, 6, BF16, CONTIG, WIDE, NONE),    # grid-stride loop, bf16 16-byte loads
    (ROW_GRID_CAP * ROWS_PER_BLOCK + 5, 4, 9, F32, PADDED, TIGHT, ALL),      # grid-stride loop, fp32 16-byte loads
]
BLOCK = 37          # the grid-cap cases repeat a block of BLOCK rows (labels included): every copy must give the same bits

# nn_accuracy: (dot, B, D, C, k, y_pred layout, emb layout, want scores, want best, feature scale)
NN_CASES = [
    (True, 1, 1, 1, 1, CONTIG, CONTIG, True, True, 1.0),
    (True, 37, 64, 100, 5, CONTIG, PADDED, True, False, 1.0),            # one slice (4 tiles)
    (True, 33, 100, 1023, 1, PADDED, CONTIG, False, True, 1.0),          # several slices, last one partial
    (True, 70, 65, 1025, 2000, COL1, PADDED, True, True, 1.0),           # k > C
    (True, 5, 7, 33, 40, COL1, COL1, True, True, 1.0),
    (True, 64, 16, 161, 1, CONTIG, COL1, True, True, 1.0),               # several slices
    (True, 3, 4, 129, 5, COL1, PADDED, False, False, 1.0),
    (True, 40, 1000, 300, 1, CONTIG, CONTIG, True, True, 1e3),           # ulp(score) >> 1e-6
    (True, 33, 1000, 100, 3, CONTIG, CONTIG, True, True, 1e3),
    (True, 32 * 1024 + 7, 4, 161, 3, CONTIG, CONTIG, True, True, 1.0),   # one slice because the batch fills the chip
    (True, 31, 8, 31, 5, COL1, CONTIG, False, True, 1.0),
    (False, 1, 1, 1, 1, COL1, CONTIG, True, True, 1.0),
    (False, 37, 64, 100, 5, CONTIG, PADDED, True, True, 1.0),
    (False, 33, 100, 1023, 1, PADDED, CONTIG, True, False, 1.0),
    (False, 70, 65, 1025, 2000, COL1, PADDED, False, True, 1.0),
    (False, 5, 7, 33, 40, COL1, COL1, False, True, 1.0),
    (False, 64, 16, 161, 1, COL1, CONTIG, True, True, 1.0),
    (False, 3, 4, 129, 5, PADDED, COL1, True, True, 1.0),
    (False, 40, 1000, 300, 1, CONTIG, CONTIG, True, True, 1e3),
    (False, 33, 1000, 100, 3, CONTIG, CONTIG, True, True, 1e3),
    (False, 32 * 1024 + 7, 4, 161, 3, CONTIG, CONTIG, True, True, 1.0),
    (False, 31, 8, 31, 5, PADDED, COL1, False, False, 1.0),
    (False, 2, 12, 97, 1, COL1, CONTIG, True, False, 1.0),
    (True, 2, 12, 97, 1, PADDED, PADDED, False, False, 1.0),
    (True, 100, 4, 33, 2000, CONTIG, COL1, False, False, 1.0),
]

# devise: (B, D, C, by_label, y_pred layout, output pitch)
DEVISE_CASES = [
    (1, 1, 1, True, CONTIG, TIGHT),
    (5, 7, 3, False, COL1, WIDE),
    (37, 100, 64, True, PADDED, WIDE),           # one slice (2 tiles)
    (37, 100, 64, False, CONTIG, TIGHT),
    (33, 65, 1025, True, COL1, TIGHT),           # several slices
    (70, 129, 1023, False, PADDED, WIDE),
    (3, 1000, 33, False, CONTIG, WIDE),
    (2, 63, 97, True, CONTIG, TIGHT),
]

# labelembed: (B, C, layout)
LE_CASES = [
    (1, 1, CONTIG),
    (7, 5, COL1),
    (37, 100, PADDED),
    (130, 1025, CONTIG),
    (LE_GRID_CAP * ROWS_PER_BLOCK + 9, 5, PADDED),       # grid-stride loop
    (LE_GRID_CAP * ROWS_PER_BLOCK + 3, 33, CONTIG),
]


def row_id(c):
    return "B%d-D%d-C%d-%s-%s-%s-%s" % c


def nn_id(c):
    dot, B, D, C, k, pl, el, ws, wb, sc = c
    return "%s-B%d-D%d-C%d-k%d-%s-%s%s%s%s" % ("dot" if dot else "euc", B, D, C, k, pl, el, "-scores" if ws else "",
                                               "-best" if wb else "", "-x%g" % sc if sc != 1 else "")


# ------------------------------------------------------------------ CPU: the tables reach every path

def nn_k_class(k, C):
    return "1" if k == 1 else (">C" if k > C else "5" if k == 5 else "other")


def test_row_case_table_reaches_every_path():
    fwd, bwd, sqf, sqb, l2f, cap, mean_b = set(), set(), set(), set(), set(), set(), set()
    for B, D, C, xdt, layout, out, opt in ROW_CASES:
        v = cos_vec(xdt, layout, D, out if opt == ALL else None)
        for ptr in ("xhat", "inv_norm", "loss_mean"):
            fwd.add((xdt, v, ptr, opt == ALL))
        for dxdt, weights in itertools.product((F32, BF16), (True, False)):        # every case runs all four pairs, both weightings
            bwd.add((xdt, dxdt, cos_vec(xdt, layout, D), weights))
            sqb.add((xdt, dxdt, weights))
        sqf.add((xdt, sq_vec(xdt, layout, D), opt == ALL))
        l2f.add(xdt)
        cap.add(row_grid_capped(B))
        if opt == ALL:
            mean_b.add("<256" if B < 256 else "=256" if B == 256 else ">cap" if row_grid_capped(B) else ">256")
    assert fwd == set(itertools.product((F32, BF16), (False, True), ("xhat", "inv_norm", "loss_mean"), (False, True)))
    assert bwd == set(itertools.product((F32, BF16), (F32, BF16), (False, True), (False, True)))
    assert sqf == {(F32, False, False), (F32, False, True), (F32, True, False), (F32, True, True), (BF16, False, False),
                   (BF16, False, True)}
    assert sqb == set(itertools.product((F32, BF16), (F32, BF16), (False, True)))
    assert l2f == {F32, BF16} and cap == {False, True}
    assert mean_b == {"<256", "=256", ">256", ">cap"}
    # grid-stride cases of both dtypes, with 16-byte and element loads
    assert {(c[3], cos_vec(c[3], c[4], c[1])) for c in ROW_CASES if row_grid_capped(c[0])} >= {(F32, False), (F32, True), (BF16, True)}


def test_row_case_table_reaches_the_shape_edges():
    Bs = {c[0] for c in ROW_CASES}
    Ds = {c[1] for c in ROW_CASES}
    Cs = {c[2] for c in ROW_CASES}
    assert 1 in Bs and any(b % 4 and b % 32 for b in Bs) and any(b % 4 == 0 and b % 32 for b in Bs)
    assert 1 in Ds and {d % 4 for d in Ds} == {0, 1, 2, 3}
    assert any(d % 8 == 4 for B, d, C, xdt, *_ in ROW_CASES if xdt == BF16)
    assert {63, 65, 127, 129} <= Ds                                  # 64 k +- 1: wave tails
    assert {1, 31, 33, 1023, 1025} <= Cs                             # 32 k +- 1: class-tile tails
    assert {c[4] for c in ROW_CASES} == {CONTIG, PADDED, COL1} and {c[5] for c in ROW_CASES} == {TIGHT, WIDE}
    assert len({row_id(c) for c in ROW_CASES}) == len(ROW_CASES)


def test_nn_case_table_reaches_every_path():
    seen = set()
    per = {}
    for dot, B, D, C, k, pl, el, ws, wb, sc in NN_CASES:
        several = n_slices(nn_acc_tiles_per_block(B, C), C) > 1
        seen.add((dot, several, stage_vec(pl, D), stage_vec(el, D)))
        p = per.setdefault((dot, several), set())
        p.update({("k", nn_k_class(k, C)), ("scores", ws), ("best", wb)})
    assert seen == set(itertools.product((True, False), repeat=4)), sorted(set(itertools.product((True, False), repeat=4)) - seen)
    want = {("k", "1"), ("k", "5"), ("k", ">C"), ("scores", True), ("scores", False), ("best", True), ("best", False)}
    for key in itertools.product((True, False), repeat=2):
        assert per[key] >= want, (key, want - per[key])
    # ulp-sized magnitudes in both metrics and both slice modes; a large batch that takes one slice where a small one takes several
    big = {(c[0], n_slices(nn_acc_tiles_per_block(c[1], c[3]), c[3]) > 1) for c in NN_CASES if c[9] > 1}
    assert big == set(itertools.product((True, False), repeat=2))
    assert {c[0] for c in NN_CASES if c[1] >= 32 * 1024 and c[3] > 128} == {True, False}
    assert {1, 31, 33, 1023, 1025} <= {c[3] for c in NN_CASES}
    assert len({nn_id(c) for c in NN_CASES}) == len(NN_CASES)


def test_devise_and_labelembed_tables_reach_every_path():
    seen = {(c[3], n_slices(devise_tiles_per_block(c[0], c[2]), c[2]) > 1) for c in DEVISE_CASES}
    assert seen == set(itertools.product((True, False), repeat=2))
    assert {le_grid_capped(c[0]) for c in LE_CASES} == {False, True}
    assert {c[2] for c in LE_CASES} == {CONTIG, PADDED, COL1}


# ------------------------------------------------------------------ per-row bounds and the comparator

def bound(n_terms, row_abs, c=4.0):
    """|kernel - float64 oracle| <= c * (n + 4) * 2^-24 * row_abs: a float32 sum of n terms is off by at most n u times the sum of the
    absolute terms; the +4 covers the fixed number of roundings around the sums (sqrt, division, products, the final subtraction)."""
    return c * (n_terms + 4) * U * np.asarray(row_abs, dtype=np.float64)


def within(got, want, tol):
    """Elementwise |got - want| <= tol; NaN must sit exactly where the oracle has NaN, and +-inf must match."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]):
        return False
    tol = np.broadcast_to(tol, want.shape)
    return bool(np.all(np.abs(got[fin] - want[fin]) <= tol[fin]))


def cosine_bounds(x, t, w, d):
    """Per-element / per-row bounds of the cosine head's outputs for rows x against targets t (float64), weights w.
    loss_i: terms 1 and inv x_d t_d.  xhat_d, inv: relative to themselves (inv carries the error of sum x^2).
    dx_d = -w inv (t_d - x_d inv^2 (x . t)): terms |w| inv |t_d| and |w| inv^3 |x_d| sum |x t|."""
    ss = np.sum(x * x, axis=1)
    inv = 1.0 / np.sqrt(np.maximum(ss, float(EPS32)))
    sxt = np.sum(np.abs(x * t), axis=1)
    loss = bound(d, 1.0 + inv * sxt)
    xhat = bound(d, np.abs(x) * inv[:, None])
    invb = bound(d, inv)
    dx = bound(d, np.abs(w)[:, None] * (inv[:, None] * np.abs(t) + (inv ** 3 * sxt)[:, None] * np.abs(x)))
    return loss, xhat, invb, dx


def clamp_edge_dx(x, g):
    """Float64 backward of the l2norm head for upstream gradient g, with the clamp decided by the kernels' predicate: the float32
    sum x^2 >= 1e-12f (for a single non-zero element that sum is fl32(v^2), which float64 would not round).  Returns (dx, on)."""
    ss32 = np.sum(np.square(x.astype(np.float32)), axis=1, dtype=np.float32)
    on = ss32 >= EPS32
    inv = 1.0 / np.sqrt(np.maximum(ss32.astype(np.float64), float(EPS32)))
    xh = x.astype(np.float64) * inv[:, None]
    reg = (g - xh * np.sum(xh * g, axis=1, keepdims=True)) * inv[:, None]
    return np.where(on[:, None], reg, g * inv[:, None]), on


def edge_rows(D=16, col=3):
    """Single-nonzero-element rows: sum x^2 = fl32(v^2) exactly, whatever the summation order.  Squares of neighbouring floats near
    sqrt(1e-12) are two ulps of 1e-12f apart, so the rows are: 0, 1e-12f - 2 ulp, 1e-12f (exactly), 1e-12f + 2 ulp, + 4 ulp, and
    two rows far from the clamp on each side.  The comment of l2norm_bwd_kernel explains why 1e-12f itself is the row that matters."""
    v0 = np.sqrt(EPS32)
    vals = [np.float32(0), np.nextafter(v0, np.float32(0)), v0, np.nextafter(v0, np.float32(1)),
            np.nextafter(np.nextafter(v0, np.float32(1)), np.float32(1)), np.float32(1e-8), np.float32(0.5)]
    x = np.zeros((len(vals), D), dtype=np.float32)
    for i, v in enumerate(vals):
        x[i, col] = v
    sq = (x[:, col] * x[:, col]).astype(np.float32)
    steps = sq.view(np.int32).astype(np.int64) - EPS32.view(np.int32)
    return x, steps


def test_edge_rows_sit_where_they_claim():
    x, steps = edge_rows()
    assert steps[0] < -10 ** 6 and list(steps[1:5]) == [-2, 0, 2, 4]
    ss = np.sum(np.square(x), axis=1, dtype=np.float32)
    assert ss[2] == EPS32 and np.float32(1) / np.sqrt(np.maximum(ss[2], EPS32)) == np.float32(1e6)
    assert list(ss >= EPS32) == [False, False, True, True, True, False, True]


def test_comparator_rejects_mutated_oracle_outputs():
    """The per-row bounds accept a float32 evaluation of the right formula and reject each of: one of D = 1000 terms dropped, the
    neighbouring row's label, the bf16 rounding of x skipped, the clamp branch taken on the wrong side."""
    import torch
    rng = np.random.default_rng(5)
    B, D, C = 16, 1000, 50
    E = rng.standard_normal((C, D))
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    E = E.astype(np.float32).astype(np.float64)
    x_raw = (rng.standard_normal((B, D)) * np.exp2(rng.integers(-8, 9, size=B))[:, None]).astype(np.float32)
    x = torch.from_numpy(x_raw).to(torch.bfloat16).float().numpy().astype(np.float64)
    y = rng.integers(0, C, size=B)
    w = rng.standard_normal(B)
    fwd = lo.cosine_loss_fwd(x, y, E)
    dx = lo.cosine_loss_bwd(x, y, E, w)
    lb, xb, ib, db = cosine_bounds(x, E[y], w, D)
    # a correct float32 evaluation passes
    f32 = lo.cosine_loss_fwd(x, y, E, dtype=np.float32)
    assert within(f32["loss_i"], fwd["loss_i"], lb) and within(f32["xhat"], fwd["xhat"], xb) and within(f32["inv_norm"], fwd["inv_norm"], ib)
    assert within(lo.cosine_loss_bwd(x, y, E, w, dtype=np.float32), dx, db)
    # one element of D = 1000 dropped (the largest term of each row)
    j = np.argmax(np.abs(x * E[y]), axis=1)
    xd = x.copy()
    xd[np.arange(B), j] = 0
    assert not within(lo.cosine_loss_fwd(xd, y, E)["loss_i"], fwd["loss_i"], lb)
    assert not within(lo.cosine_loss_bwd(xd, y, E, w), dx, db)
    # the neighbouring row's label
    assert not within(lo.cosine_loss_fwd(x, np.roll(y, 1), E)["loss_i"], fwd["loss_i"], lb)
    assert not within(lo.cosine_loss_bwd(x, np.roll(y, 1), E, w), dx, db)
    # bf16 rounding of x skipped
    raw = x_raw.astype(np.float64)
    assert not within(lo.cosine_loss_fwd(raw, y, E)["xhat"], fwd["xhat"], xb)
    assert not within(lo.cosine_loss_bwd(raw, y, E, w), dx, db)
    # the clamp branch on the wrong side, on the edge rows
    xe, _ = edge_rows(D=16)
    Ee = rng.standard_normal((3, 16))
    ye = np.arange(len(xe)) % 3
    we = np.ones(len(xe))
    g = -we[:, None] * Ee[ye]
    want, on = clamp_edge_dx(xe, g)
    assert list(on) == [False, False, True, True, True, False, True]
    _, _, _, eb = cosine_bounds(xe.astype(np.float64), Ee[ye], we, 16)
    assert within(lo.cosine_loss_bwd(xe.astype(np.float64), ye, Ee, we, eps=float(EPS32))[3:], want[3:], eb[3:])
    inv = 1.0 / np.sqrt(np.maximum(np.sum(np.square(xe), axis=1, dtype=np.float32).astype(np.float64), float(EPS32)))
    for row in (1, 2, 3):                           # 2 ulps below (clamped), exactly 1e-12f and 2 ulps above (regular)
        flipped = want.copy()
        flipped[row] = np.where(on[row], g[row] * inv[row], want[row])
        if not on[row]:
            xh = xe[row].astype(np.float64) * inv[row]
            flipped[row] = (g[row] - xh * np.dot(xh, g[row])) * inv[row]
        assert not within(flipped, want, eb), row


# ------------------------------------------------------------------ GPU helpers

@pytest.fixture(scope="module")
def sehip():
    import sehip as m
    m.lib()
    return m


SENT32 = np.int32(0x7FC0DEAD)       # a quiet NaN with a payload no kernel writes
SENT16 = np.int16(0x7FDE)


def call(name, *args):
    from sehip._lib import call as c
    return c(name, *args)


def place(a, layout, dtype):
    """Device copy of the float32 matrix ``a`` in ``layout`` and torch ``dtype``; NaN in every element that is not part of it."""
    import torch
    rows, d = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)
    buf = torch.full((rows + 3, pitch(layout, d)), float("nan"), dtype=dtype, device="cuda")
    off = 1 if layout == COL1 else 0
    buf[:rows, off:off + d] = t
    v = buf[:rows, off:off + d]
    assert v.stride(0) == pitch(layout, d) and (v.data_ptr() % 16 == 0) == aligned(layout)
    return v


class Guarded:
    """A caller output of ``rows`` x ``cols`` (pitch ``ld``), one sentinel guard row before and two after it, sentinel pitch padding."""

    def __init__(self, rows, cols, ld, dtype="f32"):
        import torch
        self.rows, self.cols, self.ld = rows, cols, ld
        if dtype == "bf16":
            self.buf = torch.full((rows + 3, ld), int(SENT16), dtype=torch.int16, device="cuda")
            self.view = self.buf.view(torch.bfloat16)[1:rows + 1, :cols]
        elif dtype == "i32":
            self.buf = torch.full((rows + 3, ld), int(SENT32), dtype=torch.int32, device="cuda")
            self.view = self.buf[1:rows + 1, :cols]
        else:
            self.buf = torch.full((rows + 3, ld), int(SENT32), dtype=torch.int32, device="cuda")
            self.view = self.buf.view(torch.float32)[1:rows + 1, :cols]
        self.sent = SENT16 if dtype == "bf16" else SENT32

    def bits(self):
        """The output's bits; asserts every byte around it still holds the sentinel."""
        b = self.buf.cpu().numpy()
        inside = np.zeros(b.shape, dtype=bool)
        inside[1:self.rows + 1, :self.cols] = True
        assert (b[~inside] == self.sent).all(), "a store left the output (pitch padding or guard rows)"
        return b[1:self.rows + 1, :self.cols].copy()

    def f32(self):
        return self.bits().view(np.float32)


def vec_out(n):
    return Guarded(1, n, n)


def rounded(a, xdt):
    """The values the kernel reads: float32, or float32 rounded to bf16 by torch (nearest even)."""
    import torch
    if xdt == F32:
        return a.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def bf16_of(f32_bits):
    """torch's round-to-nearest-even of float32 values, as int16 bits."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(f32_bits).view(np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


def same_bits_or_both_nan16(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan_a = (a & 0x7F80) == 0x7F80
    nan_a &= (a & 0x7F) != 0
    nan_b = (b & 0x7F80) == 0x7F80
    nan_b &= (b & 0x7F) != 0
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a], b[~nan_b])


def mean_kernel_f32(v):
    """mean_kernel in float32: 256 strided sequential partial sums, the halving tree, then / n."""
    v = np.asarray(v, dtype=np.float32)
    n = len(v)
    m = (n + 255) // 256
    pad = np.zeros(m * 256, dtype=np.float32)
    pad[:n] = v
    part = np.zeros(256, dtype=np.float32)
    for i in range(m):
        part = (part + pad[i * 256:(i + 1) * 256]).astype(np.float32)
    off = 128
    while off:
        part[:off] = (part[:off] + part[off:2 * off]).astype(np.float32)
        off >>= 1
    return np.float32(part[0] / np.float32(n))


def row_inputs(case, seed):
    """x rows with magnitudes spread over 2^-8 .. 2^8 (each row's bound scales with it), unit-norm class embeddings, labels with
    -3 and C + 7 among them (clamped by the kernels) and per-row weights."""
    B, D, C = case[:3]
    rng = np.random.default_rng(seed)
    nb = BLOCK if row_grid_capped(B) else B
    x = (rng.standard_normal((nb, D)) * np.exp2(rng.integers(-8, 9, size=nb))[:, None]).astype(np.float32)
    E = rng.standard_normal((C, D))
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    y = rng.integers(0, C, size=nb)
    y[::7] = -3
    y[3::11] = C + 7
    w = rng.standard_normal(nb).astype(np.float32)
    if nb != B:
        reps = (B + nb - 1) // nb
        x, y, w = np.tile(x, (reps, 1))[:B], np.tile(y, reps)[:B], np.tile(w, reps)[:B]
    return x, E, y, w


def run_rows(case, x, E, y, w):
    """Every row-kernel entry point on one case; returns {name: bits}, sentinels checked."""
    import torch
    B, D, C, xdt, layout, out, opt = case
    tdt = torch.float32 if xdt == F32 else torch.bfloat16
    from sehip._lib import DTYPE_BF16, DTYPE_F32
    code = DTYPE_F32 if xdt == F32 else DTYPE_BF16
    xd = place(x, layout, tdt)
    Ed = place(E, layout, torch.float32)
    yd = torch.from_numpy(y.astype(np.int64)).cuda()
    wd = torch.from_numpy(w).cuda()
    ld, lde, ldo = pitch(layout, D), pitch(layout, D), out_pitch(out, D)
    r = {}
    full = opt == ALL
    xhat, inv, loss, mean = Guarded(B, D, ldo), vec_out(B), vec_out(B), vec_out(1)
    call("se_cosine_loss_fwd", xd, code, ld, yd, Ed, lde, B, D, C, xhat.view if full else None, ldo, inv.view[0] if full else None,
         loss.view[0], mean.view[0] if full else None)
    r["loss_i"] = loss.bits()[0]
    if full:
        r["xhat"], r["inv_norm"], r["loss_mean"] = xhat.bits(), inv.bits()[0], mean.bits()[0]
    else:
        for g in (xhat, inv, mean):
            assert (g.buf.cpu().numpy() == SENT32).all(), "a NULL output was written"
    for dxdt, weighted in itertools.product((F32, BF16), (True, False)):
        dx = Guarded(B, D, ldo, "bf16" if dxdt == BF16 else "f32")
        call("se_cosine_loss_bwd", xd, code, ld, yd, Ed, lde, wd if weighted else None, 0.375, B, D, C, dx.view,
             DTYPE_F32 if dxdt == F32 else DTYPE_BF16, ldo)
        r["dx_%s_%s" % (dxdt, "w" if weighted else "s")] = dx.bits()
        dq = Guarded(B, D, ldo, "bf16" if dxdt == BF16 else "f32")
        call("se_sqdist_loss_bwd", xd, code, ld, yd, Ed, lde, wd if weighted else None, 0.375, B, D, C, dq.view,
             DTYPE_F32 if dxdt == F32 else DTYPE_BF16, ldo)
        r["sqdx_%s_%s" % (dxdt, "w" if weighted else "s")] = dq.bits()
    sq, dist, smean = vec_out(B), vec_out(B), vec_out(1)
    call("se_sqdist_loss_fwd", xd, code, ld, yd, Ed, lde, B, D, C, sq.view[0], dist.view[0] if full else None,
         smean.view[0] if full else None)
    r["sq_loss"] = sq.bits()[0]
    if full:
        r["sq_dist"], r["sq_mean"] = dist.bits()[0], smean.bits()[0]
    h, hi, hs = Guarded(B, D, ldo), vec_out(B), vec_out(B)
    call("se_l2norm_fwd", xd, code, ld, B, D, h.view, ldo, hi.view[0], hs.view[0])
    r["l2_xhat"], r["l2_inv"], r["l2_sumsq"] = h.bits(), hi.bits()[0], hs.bits()[0]
    g = place(E[clamp_labels(y, C)] * np.float32(-1.5), layout, torch.float32)     # an upstream gradient (per row), NaN padding
    hx = h.view
    dl = Guarded(B, D, ldo)
    call("se_l2norm_bwd", g, ld, hx, ldo, hi.view[0], hs.view[0], B, D, dl.view, ldo)
    r["l2_dx"] = dl.bits()
    r["l2_g"] = g.cpu().numpy()
    return r


def clamp_labels(y, C):
    return np.clip(y, 0, C - 1)


# ------------------------------------------------------------------ GPU: row kernels

@pytest.mark.gpu
@pytest.mark.parametrize("case", ROW_CASES, ids=[row_id(c) for c in ROW_CASES])
def test_row_kernels_vs_oracle(sehip, case):
    B, D, C, xdt, layout, out, opt = case
    seed = ROW_CASES.index(case)
    x, E, y, w = row_inputs(case, seed)
    r = run_rows(case, x, E, y, w)
    xs = rounded(x, xdt).astype(np.float64)
    E64 = E.astype(np.float64)
    yc = clamp_labels(y, C)
    t = E64[yc]
    f = lambda k: r[k].view(np.float32).astype(np.float64)            # noqa: E731

    # cosine head: loss_i, xhat, inv_norm per row; dx per element for both weightings
    fwd = lo.cosine_loss_fwd(xs, yc, E64)
    lb, xb, ib, _ = cosine_bounds(xs, t, np.ones(B), D)
    assert within(f("loss_i"), fwd["loss_i"], lb)
    if opt == ALL:
        assert within(f("xhat"), fwd["xhat"], xb) and within(f("inv_norm"), fwd["inv_norm"], ib)
        assert r["loss_mean"].view(np.float32) == mean_kernel_f32(r["loss_i"].view(np.float32)), "loss_mean: not mean_kernel's order"
    for weighted in (True, False):
        ww = w.astype(np.float64) if weighted else np.full(B, 0.375)
        want = lo.cosine_loss_bwd(xs, yc, E64, ww, eps=float(EPS32))
        _, _, _, db = cosine_bounds(xs, t, ww, D)
        tag = "w" if weighted else "s"
        assert within(f("dx_f32_" + tag), want, db), "cosine dx (%s)" % tag
        assert same_bits_or_both_nan16(r["dx_bf16_" + tag], bf16_of(r["dx_f32_" + tag])), "bf16 dx != rounded fp32 dx"
        # squared distance backward: dx = 2 w (x - t), two roundings per element
        sw = 2 * ww[:, None] * (xs - t)
        assert within(f("sqdx_f32_" + tag), sw, bound(0, np.abs(sw)))
        assert same_bits_or_both_nan16(r["sqdx_bf16_" + tag], bf16_of(r["sqdx_f32_" + tag]))

    # squared distance forward
    sq = np.sum((xs - t) ** 2, axis=1)
    assert within(f("sq_loss"), sq, bound(D, sq))
    if opt == ALL:
        assert within(f("sq_dist"), np.sqrt(sq), bound(D, np.sqrt(sq)))
        assert r["sq_mean"].view(np.float32) == mean_kernel_f32(r["sq_loss"].view(np.float32))

    # stand-alone l2norm and its backward (= the cosine backward with E[y] = -g, w = 1)
    assert within(f("l2_xhat"), fwd["xhat"], xb) and within(f("l2_inv"), fwd["inv_norm"], ib)
    assert np.array_equal(r["l2_sumsq"].view(np.float32) >= EPS32, np.sum(xs * xs, axis=1) >= float(EPS32))
    g = r["l2_g"].astype(np.float64)
    want = lo.cosine_loss_bwd(xs, np.arange(B), -g, np.ones(B), eps=float(EPS32))
    _, _, _, gb = cosine_bounds(xs, -g, np.ones(B), D)
    assert within(f("l2_dx"), want, gb)

    # the grid-stride cases repeat one block of rows: every copy gives the same bits, and so does the block run on its own
    if row_grid_capped(B):
        small = (BLOCK,) + case[1:]
        rs = run_rows(small, x[:BLOCK], E, y[:BLOCK], w[:BLOCK])
        for k, v in r.items():
            if k in ("loss_mean", "sq_mean", "l2_g"):
                continue
            assert np.array_equal(v, np.resize(rs[k], v.shape)), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", [ROW_CASES[2], ROW_CASES[4], ROW_CASES[7], ROW_CASES[11]], ids=lambda c: row_id(c))
def test_row_kernels_rows_are_independent(sehip, case):
    """A permuted batch gives the permuted bits; a row holding NaN and one holding inf change only their own per-row outputs (and
    the batch means); out-of-range labels give the bits of the clamped labels."""
    B, D, C = case[:3]
    x, E, y, w = row_inputs(case, 100 + ROW_CASES.index(case))
    base = run_rows(case, x, E, y, w)
    perm = np.random.default_rng(1).permutation(B)
    p = run_rows(case, x[perm], E, y[perm], w[perm])
    for k, v in base.items():
        if k in ("loss_mean", "sq_mean"):
            continue
        assert np.array_equal(p[k], v[perm]), k
    clamped = run_rows(case, x, E, clamp_labels(y, C), w)
    for k, v in base.items():
        assert np.array_equal(clamped[k], v), k
    if B < 3:
        return
    xn = x.copy()
    xn[1, D // 2] = np.nan
    xn[2, 0] = np.inf
    n = run_rows(case, xn, E, y, w)
    keep = np.ones(B, dtype=bool)
    keep[[1, 2]] = False
    for k, v in base.items():
        if k in ("loss_mean", "sq_mean", "l2_g"):
            continue
        assert np.array_equal(n[k][keep], v[keep]), k
    assert np.isnan(n["loss_i"][1:3].view(np.float32)).all()       # (fmaxf(NaN, eps) = eps: only the NaN element of xhat is NaN)


@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [F32, BF16])
def test_epsilon_clamp_edge_rows(sehip, xdt):
    """Rows at sum x^2 = 0, 1e-12f - 2 ulp, 1e-12f, + 2 ulp, + 4 ulp (and far from the clamp) through cosine_loss_fwd / bwd,
    l2norm_fwd / bwd and the autograd sehip.l2norm: the gradient branch follows the forward's predicate sum x^2 >= 1e-12f.
    (In bf16 only 0, 1e-8 and 0.5 keep their values: the edge rows round to other sums, whose branch the test derives the same way.)"""
    import torch
    D = 16
    x, _ = edge_rows(D)
    x = rounded(x, xdt)
    B = len(x)
    rng = np.random.default_rng(3)
    E = rng.standard_normal((B, D)).astype(np.float32)
    y = np.arange(B)
    w = np.ones(B)
    case = (B, D, B, xdt, CONTIG, TIGHT, ALL)
    r = run_rows(case, x, E, y, w.astype(np.float32))
    xs = x.astype(np.float64)
    want, on = clamp_edge_dx(x, -E.astype(np.float64))
    _, _, _, db = cosine_bounds(xs, E.astype(np.float64), w, D)
    got = r["dx_f32_w"].view(np.float32)
    for i in range(B):
        assert within(got[i], want[i], db[i]), ("cosine dx", i, on[i])
    # stand-alone l2norm backward on the same rows, upstream gradient g_l2 (run_rows' choice): the same rule
    gl = r["l2_g"].astype(np.float64)
    want_l2, _ = clamp_edge_dx(x, gl)
    _, _, _, gb = cosine_bounds(xs, -gl, w, D)
    got = r["l2_dx"].view(np.float32)
    bad = [i for i in range(B) if not within(got[i], want_l2[i], gb[i])]
    steps = np.sum(np.square(x), axis=1, dtype=np.float32).view(np.int32).astype(np.int64) - EPS32.view(np.int32)
    assert not bad, "se_l2norm_bwd: rows %s (sum x^2 - 1e-12f in ulps: %s) took the wrong branch" % (bad, list(steps[bad]))
    # the autograd function
    xt = torch.from_numpy(x).cuda().to(torch.float32 if xdt == F32 else torch.bfloat16).requires_grad_(True)
    out = sehip.l2norm(xt)
    out.backward(torch.from_numpy(gl.astype(np.float32)).cuda())
    got = xt.grad.float().cpu().numpy()
    if xdt == F32:
        bad = [i for i in range(B) if not within(got[i], want_l2[i], gb[i])]
        assert not bad, "sehip.l2norm backward: rows %s took the wrong branch" % bad
    else:
        assert np.array_equal(xt.grad.cpu().view(torch.int16).numpy(),
                              torch.from_numpy(r["l2_dx"].view(np.float32)).to(torch.bfloat16).view(torch.int16).numpy())


# ------------------------------------------------------------------ GPU: nn_accuracy

def nn_inputs(case, seed):
    dot, B, D, C, k, pl, el, ws, wb, sc = case
    rng = np.random.default_rng(seed)
    nb = min(B, 37) if B > 4096 else B
    E = rng.standard_normal((C, D)).astype(np.float32)
    if dot:
        E /= np.linalg.norm(E, axis=1, keepdims=True)
    y = rng.integers(0, C, size=nb)
    p = (E[y] + 0.5 * rng.standard_normal((nb, D)) / (np.sqrt(D) if dot else 1.0)).astype(np.float32)
    if sc != 1:
        p *= np.float32(sc)
        E = (E * np.float32(sc)).astype(np.float32)
    p[1::9] = E[(y[1::9] + 1) % C]                   # rows that are exactly another class's embedding
    y[::13] = -3
    y[5::17] = C + 7
    if nb != B:
        reps = (B + nb - 1) // nb
        p, y = np.tile(p, (reps, 1))[:B], np.tile(y, reps)[:B]
    return p.astype(np.float32), E.astype(np.float32), y


def run_nn(case, p, E, y):
    import torch
    dot, B, D, C, k, pl, el, ws, wb, sc = case
    pd_ = place(p, pl, torch.float32)
    Ed = place(E, el, torch.float32)
    yd = torch.from_numpy(y.astype(np.int64)).cuda()
    acc, sco, best = vec_out(B), Guarded(B, C, C + 3), Guarded(1, B, B, "i32")
    need = call("se_nn_accuracy_workspace_bytes", B, C)
    assert (need > 0) == (n_slices(nn_acc_tiles_per_block(B, C), C) > 1)
    wsb = torch.empty((max(need // 8, 1),), dtype=torch.int64, device="cuda")
    call("se_nn_accuracy", pd_, pitch(pl, D), yd, Ed, pitch(el, D), B, D, C, int(dot), k, acc.view[0], sco.view if ws else None, C + 3,
         best.view[0] if wb else None, wsb if need else None, need)
    r = {"acc": acc.bits()[0]}
    if ws:
        r["scores"] = sco.bits()
    else:
        assert (sco.buf.cpu().numpy() == SENT32).all()
    if wb:
        r["best"] = best.bits()[0]
    else:
        assert (best.buf.cpu().numpy() == SENT32).all()
    return r


def nn_rule(s, y, dot, k):
    """utils.py:84-95 in the kernel's float32 counting form, on the kernel's own scores."""
    s = s.astype(np.float32)
    st = s[np.arange(len(y)), y][:, None]
    diff = (s - st) if dot else (st - s)
    win = np.abs(diff) < np.float32(1e-6)
    better = ~win & (diff >= np.float32(1e-6))
    acc = win.any(axis=1) & (better.sum(axis=1) < max(k, 1))
    best = np.argmax(s, axis=1) if dot else np.argmin(s, axis=1)
    return acc.astype(np.float32), best.astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NN_CASES, ids=[nn_id(c) for c in NN_CASES])
def test_nn_accuracy_paths(sehip, case):
    dot, B, D, C, k, pl, el, ws, wb, sc = case
    p, E, y = nn_inputs(case, NN_CASES.index(case))
    yc = clamp_labels(y, C)
    full = (dot, B, D, C, k, pl, el, True, True, sc)
    r = run_nn(full, p, E, y)
    s = r["scores"].view(np.float32)
    p64, E64 = p.astype(np.float64), E.astype(np.float64)
    want = lo.class_scores(p64, E64, dot)
    # per element: the D-term product sum (and, for Euclid, the two squared norms)
    pe = np.abs(p64) @ np.abs(E64).T
    abs_terms = pe if dot else (np.sum(p64 ** 2, 1)[:, None] + np.sum(E64 ** 2, 1)[None, :] + 2 * pe)
    assert within(s, want, bound(D, abs_terms))
    acc, best = nn_rule(s, yc, dot, k)
    assert np.array_equal(r["acc"].view(np.float32), acc), "acc != the rule on the kernel's own scores"
    assert np.array_equal(r["best"], best), "best != the lowest-index arg-max / arg-min of the kernel's own scores"
    # (the rule counts the true class within its own band; a true score that were not bit-for-bit its matrix entry would fail
    # the rows the rule accepts once an ulp of the scores exceeds 1e-6)
    if sc > 1:
        assert acc.any() and np.spacing(np.abs(s).max()) > 1e-6
    # requested outputs only, and they do not change what the others compute
    if not (ws and wb):
        rr = run_nn(case, p, E, y)
        assert np.array_equal(rr["acc"], r["acc"])
        if ws:
            assert np.array_equal(rr["scores"], r["scores"])
        if wb:
            assert np.array_equal(rr["best"], r["best"])
    # out-of-range labels == clamped labels
    rc = run_nn(full, p, E, yc)
    for key in r:
        assert np.array_equal(rc[key], r[key]), key
    # a large batch is a repeated block: the block alone runs under another slice count and gives the same bits row for row
    if B > 4096:
        nb = 37
        small = (dot, nb, D, C, k, pl, el, True, True, sc)
        assert n_slices(nn_acc_tiles_per_block(nb, C), C) > 1 and n_slices(nn_acc_tiles_per_block(B, C), C) == 1
        rs = run_nn(small, p[:nb], E, y[:nb])
        assert np.array_equal(np.resize(rs["acc"], B), r["acc"])
        assert np.array_equal(np.resize(rs["best"], B), r["best"])
        assert np.array_equal(np.resize(rs["scores"], r["scores"].shape), r["scores"])


@pytest.mark.gpu
@pytest.mark.parametrize("dot", [True, False], ids=["dot", "euc"])
def test_nn_accuracy_rows_are_independent(sehip, dot):
    """Permuted rows permute the results; a row holding NaN / inf changes only its own acc, best and scores."""
    case = (dot, 70, 65, 1025, 5, CONTIG, CONTIG, True, True, 1.0)
    p, E, y = nn_inputs(case, 77)
    base = run_nn(case, p, E, y)
    perm = np.random.default_rng(2).permutation(70)
    pr = run_nn(case, p[perm], E, y[perm])
    for k in base:
        assert np.array_equal(pr[k], base[k][perm]), k
    pn = p.copy()
    pn[4, 3], pn[9, 0] = np.nan, np.inf
    rn = run_nn(case, pn, E, y)
    keep = np.ones(70, dtype=bool)
    keep[[4, 9]] = False
    for k in base:
        assert np.array_equal(rn[k][keep], base[k][keep]), k


# ------------------------------------------------------------------ GPU: devise and labelembed

@pytest.mark.gpu
@pytest.mark.parametrize("case", DEVISE_CASES, ids=["B%d-D%d-C%d-%s-%s-%s" % (c[0], c[1], c[2], "labels" if c[3] else "ytrue", c[4], c[5])
                                                   for c in DEVISE_CASES])
def test_devise_paths(sehip, case):
    import torch
    B, D, C, by_label, layout, out = case
    rng = np.random.default_rng(200 + DEVISE_CASES.index(case))
    E = rng.standard_normal((C, D))
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    p = lo.l2norm(rng.standard_normal((B, D))).astype(np.float32)
    y = rng.integers(0, C, size=B)
    y[::5] = C + 7
    y[2::7] = -3
    yc = clamp_labels(y, C)
    yt = E[yc] if by_label else lo.l2norm(rng.standard_normal((B, D))).astype(np.float32)
    g = rng.standard_normal(B).astype(np.float32)

    def run(labels):
        pd_ = place(p, layout, torch.float32)
        Ed = place(E, layout, torch.float32)
        ytd = None if by_label else place(yt, layout, torch.float32)
        yd = torch.from_numpy(labels.astype(np.int64)).cuda() if by_label else None
        loss = vec_out(B)
        aux = torch.empty((call("se_devise_aux_floats", B, C),), dtype=torch.float32, device="cuda")
        ld = pitch(layout, D)
        call("se_devise_loss_fwd", pd_, ld, yd, ytd, ld, Ed, ld, B, D, C, MARGIN, loss.view[0], aux)
        res = {"loss": loss.bits()[0], "aux": aux[:2 * B + B * C].cpu().numpy()}
        for weighted in (True, False):
            dp = Guarded(B, D, out_pitch(out, D))
            call("se_devise_loss_bwd", yd, ytd, ld, Ed, ld, torch.from_numpy(g).cuda() if weighted else None, 0.375, B, D, C, aux, dp.view,
                 out_pitch(out, D))
            res["dp_%d" % weighted] = dp.bits()
        return res

    r = run(y)
    p64, E64, yt64 = p.astype(np.float64), E.astype(np.float64), yt.astype(np.float64)
    want = lo.devise_ranking_loss(E64, MARGIN)(yt64, p64)
    ts_abs = np.sum(np.abs(yt64 * p64), axis=1)
    pe_abs = np.abs(p64) @ np.abs(E64).T
    row_abs = np.sum(MARGIN + ts_abs[:, None] + pe_abs, axis=1)
    assert within(r["loss"].view(np.float32), want, bound(D + C, row_abs))
    # the hinge mask: where a hinge is clear of 0 by more than its own bound it is what float64 says; the count is its row sum
    h = MARGIN - np.sum(yt64 * p64, axis=1)[:, None] + p64 @ E64.T
    mask = r["aux"][2 * B:].reshape(B, C)
    clear = np.abs(h) > bound(D, MARGIN + ts_abs[:, None] + pe_abs)
    assert np.array_equal(mask[clear] == 1, h[clear] > 0) and set(np.unique(mask)) <= {0.0, 1.0}
    assert np.array_equal(r["aux"][B:2 * B], mask.sum(axis=1).astype(np.float32))
    # backward against float64 on the kernel's own mask: g (mask . E - n y_true)
    n = mask.sum(axis=1).astype(np.float64)
    for weighted in (True, False):
        gw = g.astype(np.float64) if weighted else np.full(B, 0.375)
        wdp = gw[:, None] * (mask.astype(np.float64) @ E64 - n[:, None] * yt64)
        dabs = np.abs(gw)[:, None] * (mask.astype(np.float64) @ np.abs(E64) + n[:, None] * np.abs(yt64))
        assert within(r["dp_%d" % weighted].view(np.float32), wdp, bound(C, dabs))
    if by_label:
        rc = run(yc)
        for k in r:
            assert np.array_equal(rc[k], r[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", LE_CASES, ids=["B%d-C%d-%s" % c for c in LE_CASES])
def test_labelembed_paths(sehip, case):
    import torch
    B, C, layout = case
    rng = np.random.default_rng(300 + LE_CASES.index(case))
    nb = 37 if le_grid_capped(B) else B
    o1, o2, tr = (rng.standard_normal((nb, C)).astype(np.float32) * 2 for _ in range(3))
    y = rng.integers(0, C, size=nb)
    o2[np.arange(nb)[::2], y[::2] % C] += 7.0                # correct and confident: mask = 1, relu(p - alpha) > 0
    y[1::5] = -3
    y[3::7] = C + 7
    g = rng.standard_normal(nb).astype(np.float32)
    if nb != B:
        reps = (B + nb - 1) // nb
        o1, o2, tr = (np.tile(a, (reps, 1))[:B] for a in (o1, o2, tr))
        y, g = np.tile(y, reps)[:B], np.tile(g, reps)[:B]
    yc = clamp_labels(y, C)

    def run(labels):
        rows = B
        ins = [place(a, layout, torch.float32) for a in (o1, o2, tr)]
        ld = pitch(layout, C)
        loss = vec_out(rows)
        aux = torch.empty((call("se_labelembed_aux_floats", rows),), dtype=torch.float32, device="cuda")
        yd = torch.from_numpy(labels.astype(np.int64)).cuda()
        call("se_labelembed_loss_fwd", ins[0], ld, ins[1], ld, ins[2], ld, yd, rows, C, 2.0, 0.9, 0.5, loss.view[0], aux)
        outs = [Guarded(rows, C, C + 3) for _ in range(3)]
        call("se_labelembed_loss_bwd", ins[0], ld, ins[1], ld, ins[2], ld, yd, torch.from_numpy(g).cuda(), 0.0, rows, C, 2.0, 0.9,
             0.5, aux, outs[0].view, C + 3, outs[1].view, C + 3, outs[2].view, C + 3)
        return {"loss": loss.bits()[0], "d1": outs[0].bits(), "d2": outs[1].bits(), "dt": outs[2].bits()}

    r = run(y)
    want = lo.labelembed_loss(o1, o2, tr, yc)
    d1, d2, dt = lo.labelembed_loss_bwd(o1, o2, tr, yc, g)
    mask = (o2.argmax(axis=1) == yc).astype(np.float64)
    scale = B / (mask.sum() + 1e-8)
    # per row: every term is a C-term sum of probabilities times logits bounded by the row's largest |logit| + log C
    M = 1 + np.abs(o1).max(1) + np.abs(o2).max(1) + np.abs(tr).max(1) + np.log(C)
    row_abs = M * (4 + scale * mask)
    assert within(r["loss"].view(np.float32), want, bound(C + 16, row_abs))
    gb = bound(C + 16, (np.abs(g) * row_abs)[:, None] * np.ones((1, C)))
    for k, ref in (("d1", d1), ("d2", d2), ("dt", dt)):
        assert within(r[k].view(np.float32), ref, gb), k
    rc = run(yc)
    for k in r:
        assert np.array_equal(rc[k], r[k]), k
    if nb != B:                 # the grid-stride case repeats one block of rows (the batch-wide mask scale is one value for all)
        for k, v in r.items():
            assert np.array_equal(np.resize(v[:nb], v.shape), v), k
