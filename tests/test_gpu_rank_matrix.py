"""The ranking (csrc/rank_rows.hip) through every kernel instantiation and path its host code and its detector can choose.

``se_rank_rows`` picks one of 15 ``ITEMS`` (keys per thread) from the row length, and for each the ballot build (``HW = false``:
``SE_RANK_SAFE=1`` or a refuted capability probe), or one of the hardware-ordered builds -- plain (``VAR 0``), group-peeling
(``VAR 1``), and for the wide instantiations (``ITEMS >= 64``) the two-pass window build (``VAR 2``) and, up to 98 keys, the image
build (``VAR 3``): 56 instantiations of ``rank_rows_reg_kernel``.  WHICH hardware-ordered build runs is decided on the device, from
the data, by ``rank_skew_detect_kernel``.  Rows above 53,248 columns are cut into 2 / 4 / 8 segments sorted by six ``SEG`` builds
and merged; rows above 425,984 take the tiled kernel.  The write-out is 16-byte (``vec_ok``) or element stores, in three index widths.

``rank_dispatch`` and ``detector_flag`` restate those choices in Python.  The CPU tests hold the case tables to every one of the 56
pairs -- the predicted detector verdict of a case's own data must be the build the case claims -- and to the widths, write-outs,
512-key step edges, persistent row loops and in-kernel fallbacks of every ``ITEMS``.  No pair needed a pinned child for want of a
row family that reaches it: every (ITEMS, VAR) pair is reached by the product library from the data alone.

Each GPU case calls the C ABI with buffers the test owns: ``pdist`` with NaN (or -inf) in its pitch padding and guard rows, ``rank``
with a sentinel in its pitch padding and guard rows, its own workspace whose word 16 -- where the detector leaves its verdict -- is
poisoned before the call and must read ``detector_flag(...)`` after it.  The ranks must equal ``canon_rank_rows`` bit for bit.

A case's rows are ``base[src]``: a block of distinct rows (one oracle sort each) laid out along the call.  The persistent cases
(2,100 rows: a 512-thread workgroup is 8 waves, a CU holds 32, the chip has 256 CUs, so at most 1,024 workgroups are resident and
every one gets two rows, most a third) repeat their block with a period that shares no factor with any possible grid (256 x 1 .. 4),
so the row a workgroup prefetches next is never the row it has in hand, and are laid out and compared on the device: the oracle
sorts the block once.

Modes that are read once per process (``SE_RANK_SAFE=1``; ``SE_RANK_PEEL=0..3`` of the tuning library) run this file as a child
process, one per mode, one after another.
"""
import collections
import functools
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

TESTS_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(TESTS_DIR)
PKG_DIR = os.path.join(ROOT_DIR, "semantic-embeddings_amd")
if __name__ == "__main__":
    sys.path[:0] = [PKG_DIR, ROOT_DIR, TESTS_DIR]

from oracle import retrieval_oracle as ro  # noqa: E402
import test_gpu_retrieval as T  # noqa: E402   (image_path_rows, long_rows)

# ------------------------------------------------------------------ constants of rank_rows.hip

ITEMS_TABLE = (2, 8, 12, 20, 30, 40, 46, 52, 58, 64, 72, 80, 88, 98, 104)      # launch_rank_reg_items
SEG_ITEMS = (64, 72, 80, 88, 98, 104)                                          # launch_rank_runs_items
RR_THREADS, RR_WAVES = 512, 8
RR_MAX_N = 53248
RR_HW_BITS = 11
RR_WIDE_WORDS = 2048
RR_TWO_SPAN = (1 << 24) - 3
RR_TWO_OUT = 256
RR_IMG_RUN, RR_IMG_WL, RR_IMG_MAX_ITEMS = 8, 3072, 98
RUNS_MAX_SEG = 8
CUS, WAVES_PER_CU, LDS_PER_CU = 256, 32, 160 * 1024
RESIDENT_MAX = CUS * (WAVES_PER_CU // RR_WAVES)                                 # 1,024 workgroups of 8 waves
PERSISTENT_Q = 2100                                                            # > 2 * RESIDENT_MAX: two rows each, most a third
ESZ = {0: 4, 1: 8, 2: 2}                                                       # idx64 code -> bytes per rank
POISON = 0x5EEDF1A6                                                            # word 16 of the workspace before the call
BALLOT, V0, V1, V2, V3 = "ballot", 0, 1, 2, 3


def is_wide(items):
    return RR_THREADS * items * 2 >= RR_WAVES * RR_WIDE_WORDS * 4


def all_pairs():
    """The 56 (ITEMS, build) instantiations of rank_rows_reg_kernel that se_rank_rows can launch."""
    pairs = []
    for items in ITEMS_TABLE:
        pairs += [(items, BALLOT), (items, V0), (items, V1)]
        if is_wide(items):
            pairs.append((items, V2))
            if items <= RR_IMG_MAX_ITEMS:
                pairs.append((items, V3))
    return pairs


def lds_bytes(items, build):
    """launch_rank_reg_variant: rr_region0_bytes + wave_tot + exchange buffer."""
    cnt = RR_WAVES * ((1 << RR_HW_BITS) // 2 if build != BALLOT else 256) * 4
    img = RR_THREADS * items + 32 + RR_IMG_WL * 4
    return (max(cnt, img) if build == V3 else cnt) + 32 * 4 + RR_THREADS * items * 2


def resident_bound(items, build):
    """Upper bound of the grid of a register-path launch: CUs x (waves, LDS) occupancy."""
    return CUS * min(WAVES_PER_CU // RR_WAVES, LDS_PER_CU // lds_bytes(items, build))


# ------------------------------------------------------------------ the host's choices, restated

Dispatch = collections.namedtuple("Dispatch", "path items wide two_ok img_ok vec_ok segments seg_n levels chunk")


def _ceil8(x):
    return (x + 7) // 8 * 8


def rank_runs_segments(n):
    if n <= RR_MAX_N:
        return 0
    sgm = 2
    while sgm <= RUNS_MAX_SEG:
        if _ceil8((n + sgm - 1) // sgm) <= RR_MAX_N:
            return sgm
        sgm *= 2
    return 0


def rank_runs_seg_n(n):
    sgm = rank_runs_segments(n)
    return _ceil8((n + sgm - 1) // sgm)


def rank_runs_items(n):
    items = (rank_runs_seg_n(n) + RR_THREADS - 1) // RR_THREADS
    return next(i for i in SEG_ITEMS if items <= i)


def rank_runs_chunk(q, n):
    """Rows per chunk of the runs path (rank_runs_layout)."""
    sgm, cap = rank_runs_segments(n), RR_THREADS * rank_runs_items(n)
    per_row = 6 * sgm * cap + (8 * (n + 8) if sgm > 2 else 0) + (8 * (n + 8) if sgm > 4 else 0)
    c = min(4096, max(64, 3072 * 1024 * 1024 // per_row))
    return min(q, c)


def rank_dispatch(q, n, idx, rank_ptr_alignment, ldr):
    """What se_rank_rows launches for q rows of n columns, index width code idx (0 int32, 1 int64, 2 uint16), a rank pointer of the
    given alignment (its address modulo 16) and a rank pitch of ldr elements.  None: the call is refused (uint16 above 53,248)."""
    if n <= RR_MAX_N:
        items = next(i for i in ITEMS_TABLE if (n + RR_THREADS - 1) // RR_THREADS <= i)
        wide = is_wide(items)
        vec_ok = rank_ptr_alignment % 16 == 0 and (ldr * ESZ[idx]) % 16 == 0
        return Dispatch("reg", items, wide, wide, wide and items <= RR_IMG_MAX_ITEMS, vec_ok, 0, 0, 0, 0)
    if idx == 2:
        return None
    esz = 8 if idx else 4
    vec_ok = rank_ptr_alignment % 16 == 0 and (ldr * esz) % 16 == 0
    sgm = rank_runs_segments(n)
    if sgm == 0:
        return Dispatch("tiled", 0, False, False, False, False, 0, 0, 0, 0)
    return Dispatch("runs", rank_runs_items(n), True, False, False, vec_ok, sgm, rank_runs_seg_n(n), int(math.log2(sgm)), rank_runs_chunk(q, n))


def canon_key(x):
    """canon_key of se_common.h / oracle/canon.c on a float32 array -> uint32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    k = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = 0xFFFFFFFF
    return k


def detector_flag(pd, two_ok, img_ok, wide):
    """rank_skew_detect_kernel's verdict on the call ``pd`` ([q, n] float32; only rows 0, q / 2 and q - 1 are read)."""
    q, n = pd.shape
    cols = min(n, 1024)
    shift = 20 if wide else 2 * RR_HW_BITS
    sample = (np.arange(cols, dtype=np.int64) * n) // cols
    hist = np.zeros(4096, dtype=np.int64)
    occupied = set()
    hashed = 0
    below_ok = True
    for r, row in enumerate((0, q // 2, q - 1)):
        k = canon_key(pd[row, sample])
        np.add.at(hist, k >> shift, 1)
        real = k[k != 0xFFFFFFFF]
        row_max = int(real.max()) if real.size else 0
        lo = row_max - RR_TWO_SPAN if row_max > RR_TWO_SPAN else 0
        below_ok = below_ok and int((k.astype(np.int64) < lo).sum()) <= 4
        h = ((k[:256] ^ np.uint32((r * 0x3C6EF372) & 0xFFFFFFFF)).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
        hashed += h.size
        occupied.update(int(b) for b in (h >> np.uint64(20)))
    repeats = hashed - len(occupied)            # adds that met an occupied bucket: independent of the order of the adds
    two = two_ok and below_ok
    skewed = 10 * int(hist.max()) >= 3 * 3 * cols
    distinct = repeats < 3 * 96
    return 2 if (two and distinct) else (1 if skewed else (3 if (img_ok and distinct) else 0))


def window_keeps(row):
    """VAR 2, inside the kernel: does the row keep the two-pass window path?  (raw-bit arithmetic of rank_rows.hip)"""
    raw = np.ascontiguousarray(row, dtype=np.float32).view(np.uint32)
    s = raw.view(np.int32).astype(np.int64)
    kmax = int(np.clip(s, 0, 0x7F800000).max())
    if int(raw.max()) > 0xFF800000:             # a NaN with the sign bit set
        kmax = 0x7F800000
    lo = kmax - RR_TWO_SPAN if kmax > RR_TWO_SPAN else 1
    return kmax > 0 and int((s < lo).sum()) <= RR_TWO_OUT


def image_must_give_up(row):
    """VAR 3, inside the kernel: a SUFFICIENT condition for the row to end in the three passes.  The entry test refuses NaN,
    infinities and rows whose largest magnitude is outside [2^-100, 2^126).  Equal keys share an image, so a key that occurs more
    than RR_IMG_RUN times is a run above the cap; and since a run holds at most RR_IMG_RUN entries, more than RR_IMG_RUN x
    RR_IMG_WL entries inside tie groups need more runs than the worklist holds."""
    raw = np.ascontiguousarray(row, dtype=np.float32).view(np.uint32)
    mb = int((raw & 0x7FFFFFFF).max())
    if not (0x0D800000 <= mb < 0x7E800000):
        return True
    _, counts = np.unique(canon_key(row), return_counts=True)
    return int(counts.max()) > RR_IMG_RUN or int(counts[counts >= 2].sum()) > RR_IMG_RUN * RR_IMG_WL


# ------------------------------------------------------------------ row families

COS, EUC, TWO, FOUR, MIX, LONG = "cos", "euc", "two", "four", "mix", "long"
F32 = np.float32


def gauss(rng, n):
    return rng.standard_normal(n).astype(F32)


def plain_row(fam, rng, n, r):
    """One row of the family as the reference produces it: what the detector is meant to see."""
    if fam == COS or fam == MIX:
        return (0.1 * gauss(rng, n)).astype(F32)                                # cosine-like: mixed signs
    if fam == EUC:
        v = (200.0 + 20.0 * gauss(rng, n)).astype(F32)                           # Euclidean-like, with the query's own 0
        v[(r * 131) % n] = 0.0
        return v
    if fam == TWO:
        return rng.choice(np.array([1.0, 2.0], dtype=F32), size=n)
    if fam == FOUR:
        return rng.choice(np.array([1.0, 2.0, 3.0, 4.0], dtype=F32), size=n)
    raise ValueError(fam)


def special_rows(rng, n):
    """Rows every build must order: long tie runs, NaN of both signs, infinities, signed zeros, denormals, one value, sorted keys
    (ascending / descending: every lane of a wave step on one counter)."""
    rows = [rng.integers(-2, 3, size=n).astype(F32)]                            # five values
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, np.inf, -np.inf, 3.4028235e38, -3.4028235e38], dtype=F32)
    v = rng.choice(specials, size=n)
    nanbits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(F32)
    v[::5] = rng.choice(nanbits, size=len(v[::5]))
    rows.append(v)
    w = np.where(rng.random(n) < 0.5, gauss(rng, n), rng.choice(specials, size=n)).astype(F32)
    rows.append(w)
    rows.append(np.full(n, 3.0, dtype=F32))                                     # all equal
    s = np.sort(gauss(rng, n))
    rows.append(s)                                                              # ascending
    rows.append(s[::-1].copy())                                                 # descending
    t = gauss(rng, n)
    t[::7] = np.nan
    rows.append(t)
    return rows


def window_rows(rng, n):
    """Rows aimed at the two-pass window build (the recipe of test_rank_rows_two_pass_path): keys below the window at columns the
    detector does not sample -- none, exactly 256 (kept), 257 (given up) -- ties, the window's lower edge, +inf, NaN of both signs,
    a positive row 2^30 codes wide."""
    free = np.setdiff1d(np.arange(n), (np.arange(1024) * n) // 1024)
    base = lambda: (200.0 + 25.0 * gauss(rng, n)).astype(F32).clip(120.0, 300.0)  # noqa: E731
    neg_nan = np.array([0xFFC00000, 0xFFFFFFFF, 0xFF800001], dtype=np.uint32).view(F32)
    rows = []
    v = base(); v[free[:256]] = rng.choice(np.array([0.0, -0.0, 1e-3, -1e-3, 2.5, 2.5, -7.0], dtype=F32), size=256); rows.append(v)   # 256 below: kept
    v = base(); v[free[:257]] = np.linspace(-1.0, 1.0, 257, dtype=F32); rows.append(v)                                           # 257 below: given up
    rows.append(np.round(base()))                                                                                                # long tie runs inside the window
    rows.append(np.full(n, 210.0, dtype=F32))
    v = base()
    m = F32(v.max())
    edge = (m.view(np.uint32) - np.uint32(RR_TWO_SPAN)).view(F32)
    v[free[:6]] = np.array([edge, np.nextafter(edge, F32(0)), edge, np.nextafter(edge, F32(1e9)), 0.5, edge], dtype=F32)
    rows.append(v)
    v = base(); v[free[10]] = np.inf; rows.append(v)                                                                             # window at +inf: given up
    v = base(); v[free[3:9]] = np.nan; rows.append(v)                                                                            # NaN: given up
    rows.append((1e-3 * np.abs(gauss(rng, n)) + 1e-6).astype(F32))                                                                # 2^30 codes wide: given up
    v = base(); v[free[:20]] = -np.abs(gauss(rng, 20)); rows.append(v)
    v = base(); v[free[40:43]] = neg_nan; rows.append(v)                                                                         # NaN with the sign bit set
    v = base(); v[free[:300:2]] = neg_nan[0]; rows.append(v)
    return rows


def pair_row(rng, n):
    """Every key exactly twice: more tie groups than the image build's worklist holds."""
    d = (0.1 * gauss(rng, (n + 1) // 2)).astype(F32)
    return np.repeat(d, 2)[:n][rng.permutation(n)]


def family_body(fam, rng, n, wide):
    """The rows between the detector's three sampled rows: rows of OTHER families (the detector samples three rows only), the special
    rows, and for the wide instantiations the rows that keep / give up the fast paths inside the kernel."""
    cross = {COS: EUC, EUC: COS, TWO: COS, FOUR: EUC, MIX: EUC}[fam]
    body = [plain_row(cross, rng, n, 1)]
    if fam == MIX:
        body += [plain_row(TWO, rng, n, 2), plain_row(FOUR, rng, n, 3)]
    if wide and fam in (COS, MIX):
        body += list(T.image_path_rows(rng, n)) + [pair_row(rng, n)]
    if wide and fam in (EUC, MIX):
        body += window_rows(rng, n)
    if not wide or fam in (TWO, FOUR, MIX):
        body += special_rows(rng, n)
    else:
        body += special_rows(rng, n)[:2]
    while (2 * len(body) + 3) % 3 == 0:         # the block's period must share no factor with a grid of 256 x 1 .. 4
        body.append(plain_row(fam, rng, n, len(body)))
    return body


@functools.lru_cache(maxsize=4)
def family_block(fam, n, seed):
    """[plain] + body + [plain] + reversed body + [plain]: rows 0, B / 2 and B - 1 are the family's plain rows, and every body row
    stands next to its neighbours in both orders."""
    if fam == LONG:
        rng = np.random.default_rng(seed)
        return np.concatenate([T.long_rows(n, seed), (0.1 * gauss(rng, n))[None, :]], axis=0)       # 7 rows
    rng = np.random.default_rng(seed)
    body = family_body(fam, rng, n, n > 512 * 58)
    rows = [plain_row(fam, rng, n, 0)] + body + [plain_row(fam, rng, n, 1)] + body[::-1] + [plain_row(fam, rng, n, 2)]
    return np.stack(rows).astype(F32)


# ------------------------------------------------------------------ case tables (the only statement of what runs)

# mode: PRODUCT (the product library decides from the data; `build` is the build the case claims), BALLOT (SE_RANK_SAFE=1 child),
# PINNED (product run + one SE_RANK_PEEL child per build, bytes compared).  q: 0 = one block, else the block repeated to q rows.
# out: rank layout -- VEC (pitch a multiple of 16 bytes, padded), PITCH (padded, pitch not a multiple of 16 bytes), OFF (pitch a multiple
# of 16 bytes, the view starts one element in), TIGHT (pitch n).  inp: pdist layout -- TIGHT (pitch n), NAN / NINF (pitch n + 5, the padding
# holds NaN / -inf).  Guard rows in front of and behind both matrices always.
PRODUCT, PINNED = "product", "pinned"
VEC, PITCH, OFF, TIGHT, NAN, NINF = "vec", "pitch", "off", "tight", "nan", "ninf"
Case = collections.namedtuple("Case", "mode items build q n fam idx out inp")
REFERENCE_ROWS = (5794, 8041, 10000, 24633, 50000)      # CUB, Cars, CIFAR-100, NABirds, ILSVRC validation


def case_id(c):
    return "%s-I%d-%s-q%d-n%d-%s-w%d-%s-%s" % (c.mode, c.items, c.build, c.q, c.n, c.fam, c.idx, c.out, c.inp)


def _items_of(n):
    return next(i for i in ITEMS_TABLE if (n + RR_THREADS - 1) // RR_THREADS <= i)


def _build_cases():
    cases = []
    for i, items in enumerate(ITEMS_TABLE):
        prev = ITEMS_TABLE[i - 1] if i else 0
        full, ragged = 512 * items, 512 * prev + 1       # last full / first ragged 512-key step of the instantiation
        mid = ((full + ragged) // 2) | 1
        wide = is_wide(items)
        a, b, c = i % 3, (i + 1) % 3, (i + 2) % 3        # the three index widths, rotated
        P = lambda build, q, n, fam, idx, out, inp: cases.append(Case(PRODUCT, items, build, q, n, fam, idx, out, inp))  # noqa: E731
        P(V0, 0, full, FOUR if wide else COS, a, VEC, TIGHT)
        P(V0, 0, mid, FOUR, c, OFF, NINF)
        P(V1, 0, ragged, TWO if wide else EUC, b, PITCH, NAN)
        P(V1, 0, full, TWO, c, TIGHT, NAN)
        if not wide:
            P(V0, 0, mid + 2, COS, b, PITCH, NAN)
            P(V1, 0, mid + 4, EUC, a, VEC, NINF)
            # persistent row loop: the build a default (Euclidean) evaluation takes, and the cosine one, alternating
            if i % 2:
                P(V1, PERSISTENT_Q, ragged + 99, EUC, c, VEC, NAN)
            else:
                P(V0, PERSISTENT_Q, ragged + 99, COS, c, VEC, NAN)
        else:
            P(V2, 0, full, EUC, a, VEC, NAN)
            P(V2, 0, ragged, EUC, b, OFF, NINF)
            P(V2, PERSISTENT_Q, mid, EUC, c, PITCH, NAN)
            if items <= RR_IMG_MAX_ITEMS:
                P(V3, 0, full, COS, c, PITCH, NAN)
                P(V3, 0, ragged, COS, a, VEC, TIGHT)
                P(V3, PERSISTENT_Q, mid + 2, COS, b, VEC, NINF)
            else:
                P(V0, 0, mid + 2, COS, b, PITCH, NAN)     # 104 keys: no image build -- cosine rows take the plain one
        cases.append(Case(BALLOT, items, BALLOT, 0, full, MIX, a, VEC, TIGHT))
        cases.append(Case(BALLOT, items, BALLOT, 0, ragged, MIX, b, PITCH, NAN))
        cases.append(Case(BALLOT, items, BALLOT, 0, mid, MIX, c, OFF, NINF))
        cases.append(Case(PINNED, items, None, 0, full - 37, MIX, a, (VEC, PITCH, OFF)[i % 3], NAN))
    # the reference's own evaluation sets, in the reference's index dtype, cosine and Euclidean rows
    for n in REFERENCE_ROWS:
        items = _items_of(n)
        cases.append(Case(PRODUCT, items, V3 if is_wide(items) else V0, 0, n, COS, 1, TIGHT, TIGHT))
        cases.append(Case(PRODUCT, items, V2 if is_wide(items) else V1, 0, n, EUC, 1, TIGHT, NAN))
    return cases


CASES = _build_cases()
# cases per build of every ITEMS -- (ballot, VAR 0, VAR 1[, VAR 2[, VAR 3]]), product cases counted under the build their data selects --
# as the census prints them.  A row that leaves the table, or drifts to another build, changes a count.
EXPECTED_COUNTS = {2: (3, 4, 3), 8: (3, 3, 4), 12: (3, 5, 4), 20: (3, 5, 6), 30: (3, 4, 3), 40: (3, 3, 4), 46: (3, 4, 3), 52: (3, 4, 5),
                   58: (3, 4, 3), 64: (3, 2, 2, 3, 3), 72: (3, 2, 2, 3, 3), 80: (3, 2, 2, 3, 3), 88: (3, 2, 2, 3, 3), 98: (3, 2, 2, 4, 4),
                   104: (3, 3, 2, 3)}

# rows above 53,248 columns: every SEG build at 2, 4 and 8 segments (int32 and int64 both run; uint16 must be refused), one case with
# more rows than a chunk, and the tiled kernel behind the last segment count.  n = segments x 512 x ITEMS - 5: full segments but the last.
RunsCase = collections.namedtuple("RunsCase", "q n out inp")
RUNS_CASES = [RunsCase(0, sgm * 512 * items - 5, {2: PITCH, 4: OFF, 8: VEC}[sgm], {2: NAN, 4: NINF, 8: NAN}[sgm])
              for sgm in (2, 4, 8) for items in SEG_ITEMS]
RUNS_CASES.append(RunsCase(600, 8 * 512 * 64 - 5, PITCH, NAN))         # chunk-crossing: 558 rows per chunk at this length
RUNS_CASES.append(RunsCase(0, 8 * RR_MAX_N + 1, PITCH, NAN))           # tiled kernel


def case_seed(c):
    return (c.n * 31 + c.items) % (1 << 31)


def case_block(c):
    return family_block(c.fam, c.n, case_seed(c))


def case_src(c, rows):
    """Block row of every row of the call.  Repeated blocks keep the block's first (plain) row under the detector's three samples."""
    if c.q == 0:
        return np.arange(rows, dtype=np.int64)
    src = np.arange(c.q, dtype=np.int64) % rows
    src[[0, c.q // 2, c.q - 1]] = 0
    return src


def out_layout(out, n, idx):
    """-> (pitch in elements, first column of the view)."""
    e = 16 // ESZ[idx]
    if out == TIGHT:
        return n, 0
    if out in (VEC, OFF):
        return (n + e - 1) // e * e + e, 1 if out == OFF else 0
    ldr = n + 3
    while ldr % e == 0:
        ldr += 1
    return ldr, 0


def out_alignment(out, n, idx):
    """Address of the rank view modulo 16: the buffer is 256-byte aligned, the view starts one guard row (+ its first column) in."""
    ldr, c0 = out_layout(out, n, idx)
    return ((ldr + c0) * ESZ[idx]) % 16


def in_pitch(inp, n):
    return n if inp == TIGHT else n + 5


def case_dispatch(c):
    q = c.q or case_block(c).shape[0]
    return rank_dispatch(q, c.n, c.idx, out_alignment(c.out, c.n, c.idx), out_layout(c.out, c.n, c.idx)[0])


def case_flag(c):
    """The detector's predicted verdict on the case's own data."""
    block = case_block(c)
    src = case_src(c, block.shape[0])
    q = len(src)
    d = case_dispatch(c)
    return detector_flag(block[src[[0, q // 2, q - 1]]], d.two_ok, d.img_ok, d.wide)


# ------------------------------------------------------------------ the comparator

def same_ranking(got, want, idx):
    """Bit equality of a rank matrix with the oracle's int32 ranks (uint16 ranks compared as unsigned)."""
    got = np.asarray(got)
    if idx == 2:
        got = got.view(np.uint16)
    return got.shape == want.shape and bool(np.array_equal(got.astype(np.int64), want.astype(np.int64)))


# ------------------------------------------------------------------ CPU: the tables reach every path

def test_dispatch_restatement_edges():
    assert len(all_pairs()) == 56
    assert [i for i in ITEMS_TABLE if is_wide(i)] == [64, 72, 80, 88, 98, 104]
    for i, items in enumerate(ITEMS_TABLE):
        prev = ITEMS_TABLE[i - 1] if i else 0
        assert rank_dispatch(3, 512 * items, 0, 0, 512 * items).items == items
        assert rank_dispatch(3, 512 * prev + 1, 0, 0, 512 * prev + 1).items == items
    d = rank_dispatch(3, 50000, 0, 0, 50000)
    assert (d.path, d.items, d.wide, d.two_ok, d.img_ok, d.vec_ok) == ("reg", 98, True, True, True, True)
    assert not rank_dispatch(3, 53248, 0, 0, 53248).img_ok
    assert not rank_dispatch(3, 50000, 0, 4, 50000).vec_ok and not rank_dispatch(3, 50001, 0, 0, 50001).vec_ok
    assert rank_dispatch(3, 50001, 0, 0, 50004).vec_ok and not rank_dispatch(3, 50001, 1, 0, 50003).vec_ok
    assert rank_dispatch(3, 50002, 2, 0, 50008).vec_ok and not rank_dispatch(3, 50002, 2, 0, 50004).vec_ok
    # the runs path: lengths of test_rank_rows_long_rows_sorted_runs
    for n, sgm, items in ((53249, 2, 64), (65536, 2, 64), (65537, 2, 72), (106496, 2, 104), (106497, 4, 64), (212992, 4, 104), (212993, 8, 64),
                          (425984, 8, 104)):
        d = rank_dispatch(6, n, 0, 0, n)
        assert (d.path, d.segments, d.items, d.levels) == ("runs", sgm, items, {2: 1, 4: 2, 8: 3}[sgm]), n
        assert d.seg_n % 8 == 0 and d.seg_n * sgm >= n and d.seg_n <= RR_MAX_N
    assert rank_dispatch(6, 425985, 0, 0, 425985).path == "tiled"
    assert rank_dispatch(6, 53249, 2, 0, 53249) is None
    assert rank_dispatch(4200, 53301, 0, 0, 53301).chunk == 4096
    # occupancy bound behind the persistent cases
    assert RESIDENT_MAX == 1024 and PERSISTENT_Q > 2 * RESIDENT_MAX
    assert all(resident_bound(i, b) <= RESIDENT_MAX for i, b in all_pairs())
    assert all(resident_bound(i, b) == 256 for i, b in all_pairs() if is_wide(i) and b != BALLOT)      # one workgroup per CU


def test_detector_restatement_on_the_reference_row_families():
    """8 rows per call, seed 0: cosine-like, gaussian and four-valued rows vs Euclidean-like and two-valued rows."""
    rng = np.random.default_rng(0)
    fams = [lambda n: (0.1 * rng.standard_normal((8, n))).astype(F32), lambda n: rng.standard_normal((8, n)).astype(F32),
            lambda n: rng.choice(np.array([1.0, 2.0, 3.0, 4.0], dtype=F32), size=(8, n)),
            lambda n: (200.0 + 20.0 * rng.standard_normal((8, n))).astype(F32), lambda n: rng.choice(np.array([1.0, 2.0], dtype=F32), size=(8, n))]
    for ns, want in (((5794, 10000, 24633), (0, 0, 0, 1, 1)), ((36000, 40961, 50000), (3, 3, 0, 2, 1)), ((53248,), (0, 0, 0, 2, 1))):
        for n in ns:
            d = rank_dispatch(8, n, 0, 0, n)
            assert tuple(detector_flag(f(n), d.two_ok, d.img_ok, d.wide) for f in fams) == want, n
    # one column: the single sampled key is the whole histogram
    assert detector_flag(np.zeros((3, 1), dtype=F32), False, False, False) == 1
    # keys, as canon.c builds them
    x = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45], dtype=F32)
    assert canon_key(x).tolist() == [0x80000000, 0x80000000, 0xBF800000, 0x407FFFFF, 0xFF800000, 0x007FFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x80000001, 0x7FFFFFFE]


def census():
    """(ITEMS, build) -> the cases that reach it; product cases by their predicted detector verdict."""
    reach = collections.defaultdict(list)
    for c in CASES:
        d = case_dispatch(c)
        assert d.path == "reg" and d.items == c.items, case_id(c)
        if c.mode == PRODUCT:
            reach[(c.items, case_flag(c))].append(c)
        elif c.mode == BALLOT:
            reach[(c.items, BALLOT)].append(c)
    return reach


def test_case_table_reaches_all_56_instantiations_through_the_product_library():
    """The predicted detector verdict of every product case's own data is the build the case claims (a row family that drifts to
    another build fails here, not silently on the device), and the claims cover the 56 pairs."""
    for c in CASES:
        if c.mode == PRODUCT:
            assert case_flag(c) == c.build, (case_id(c), case_flag(c))
    reach = census()
    for pair in all_pairs():
        assert reach[pair], "no case reaches ITEMS %s build %s" % pair
    assert set(reach) == set(all_pairs())
    for items in ITEMS_TABLE:
        assert tuple(len(reach[(it, b)]) for it, b in all_pairs() if it == items) == EXPECTED_COUNTS[items], items
    assert sum(len(v) for v in reach.values()) + len(ITEMS_TABLE) == len(CASES) == len(set(CASES))      # + one pinned case per ITEMS
    print("\ncases per (ITEMS, build):")
    for items in ITEMS_TABLE:
        print("  ITEMS %3d: " % items + "  ".join("%s %d" % (b if b == BALLOT else "VAR%d" % b, len(reach[(items, b)]))
                                                  for it, b in all_pairs() if it == items))


def test_case_table_reaches_widths_writeouts_steps_and_persistent_loops_per_items():
    for i, items in enumerate(ITEMS_TABLE):
        mine = [c for c in CASES if c.items == items]
        prev = ITEMS_TABLE[i - 1] if i else 0
        assert {c.idx for c in mine if c.mode != PINNED} == {0, 1, 2}, items
        assert {case_dispatch(c).vec_ok for c in mine if c.mode == PRODUCT} == {True, False}, items
        assert {case_dispatch(c).vec_ok for c in mine if c.mode == BALLOT} == {True, False}, items
        assert {512 * items, 512 * prev + 1} <= {c.n for c in mine if c.mode == PRODUCT}, items
        assert {512 * items, 512 * prev + 1} <= {c.n for c in mine if c.mode == BALLOT}, items
        assert any(c.q >= PERSISTENT_Q for c in mine if c.mode == PRODUCT), items
        assert {c.inp for c in mine} >= {TIGHT, NAN, NINF} and {c.out for c in mine} >= {VEC, PITCH, OFF, TIGHT}, items
        assert sum(c.mode == PINNED for c in mine) == 1, items
    for c in CASES:
        if c.q:
            rows = case_block(c).shape[0]
            assert c.q > 2 * resident_bound(c.items, c.build)
            assert all(math.gcd(rows, CUS * occ) == 1 for occ in (1, 2, 3, 4)), case_id(c)
    for n in REFERENCE_ROWS:
        assert {c.fam for c in CASES if c.n == n and c.mode == PRODUCT and c.idx == 1} == {COS, EUC}, n
    # the builds a default evaluate_retrieval.py run takes on CIFAR-100 and NABirds
    assert any(c.items == 20 and c.build == V1 and c.n == 10000 for c in CASES)
    assert any(c.items == 52 and c.build == V1 and c.n == 24633 for c in CASES)


def test_window_and_image_cases_cross_a_fallback_with_rows_that_keep_the_fast_path():
    """Every VAR 2 / VAR 3 instantiation: rows that must give the fast path up inside the kernel (257 keys below the window, a NaN, an
    infinity; NaN / infinity, tie groups beyond the worklist, runs above the cap) next to rows that keep it, in both orders -- in the
    block, and in the persistent cases along a workgroup's own sequence of rows (row, row + grid, ...) for every possible grid."""
    for items, build in all_pairs():
        if build not in (V2, V3):
            continue
        mine = [c for c in CASES if c.mode == PRODUCT and c.items == items and c.build == build]
        assert any(c.q for c in mine) and any(not c.q for c in mine), (items, build)
        for c in mine:
            block = case_block(c)
            if build == V2:
                gives = np.array([not window_keeps(r) for r in block])
                wr = lambda k: block[2 + k]                                    # noqa: E731  (plain, cross row, then window_rows)
                assert not window_keeps(wr(1)) and np.isinf(wr(5)).any() and np.isnan(wr(6)).any()     # 257 below, +inf, NaN
                assert window_keeps(block[0]) and window_keeps(wr(0)) and window_keeps(wr(2)) and not window_keeps(block[1])
            else:
                gives = np.array([image_must_give_up(r) for r in block])
                assert not gives[0] and gives.sum() >= 6
                assert image_must_give_up(pair_row(np.random.default_rng(1), c.n))
            src = case_src(c, block.shape[0])
            g = gives[src]
            steps = (1,) if not c.q else tuple(CUS * occ for occ in (1, 2, 3, 4))
            for step in steps:
                if step >= len(g):
                    continue
                assert bool((g[:-step] & ~g[step:]).any()) and bool((~g[:-step] & g[step:]).any()), (case_id(c), step)


def test_runs_case_table_reaches_every_seg_build_and_segment_count():
    seen = set()
    for rc in RUNS_CASES:
        for idx in (0, 1):
            d = rank_dispatch(rc.q or 7, rc.n, idx, out_alignment(rc.out, rc.n, idx), out_layout(rc.out, rc.n, idx)[0])
            if d.path == "runs":
                seen.add((d.items, d.segments, idx, d.vec_ok))
                assert d.levels == {2: 1, 4: 2, 8: 3}[d.segments]
        assert rank_dispatch(rc.q or 7, rc.n, 2, 0, rc.n) is None
    for items in SEG_ITEMS:
        for sgm in (2, 4, 8):
            for idx in (0, 1):
                assert {v for (i, s, w, v) in seen if (i, s, w) == (items, sgm, idx)}, (items, sgm, idx)
        for idx in (0, 1):
            assert {v for (i, s, w, v) in seen if (i, w) == (items, idx)} == {True, False}, (items, idx)
    assert any(rc.q > rank_dispatch(rc.q, rc.n, 0, 0, rc.n).chunk > 0 for rc in RUNS_CASES if rc.q)
    assert any(rank_dispatch(7, rc.n, 0, 0, rc.n).path == "tiled" for rc in RUNS_CASES)
    assert {rc.inp for rc in RUNS_CASES} >= {NAN, NINF}


def test_comparator_rejects_mutated_oracle_outputs():
    rng = np.random.default_rng(4)
    pd = rng.integers(-2, 3, size=(3, 700)).astype(F32)
    want = ro.canon_rank_rows(pd)
    for idx, dt in ((0, np.int32), (1, np.int64), (2, np.uint16)):
        good = want.astype(dt)
        assert same_ranking(good.view(np.int16) if idx == 2 else good, want, idx)
        keys = pd[1][want[1]]
        r = int(np.nonzero(keys[1:] == keys[:-1])[0][0])
        m = good.copy(); m[1, [r, r + 1]] = m[1, [r + 1, r]]                    # two entries of a tie group swapped
        assert not same_ranking(m.view(np.int16) if idx == 2 else m, want, idx)
        m = good.copy(); m[2, 350] += 1                                         # one index off by one
        assert not same_ranking(m.view(np.int16) if idx == 2 else m, want, idx)
        m = good.copy(); m[0, 10] = m[0, 11]                                    # one entry duplicated
        assert not same_ranking(m.view(np.int16) if idx == 2 else m, want, idx)
        m = good.copy(); m[0, [0, -1]] = m[0, [-1, 0]]                          # the first and last entries exchanged
        assert not same_ranking(m.view(np.int16) if idx == 2 else m, want, idx)
    # uint16 ranks above 32,767 are compared as unsigned
    big = np.arange(40000, dtype=np.int32)[None, :]
    assert same_ranking(big.astype(np.uint16).view(np.int16), big, 2)


# ------------------------------------------------------------------ GPU: one case through the C ABI

def _torch_dtype(idx):
    import torch
    return {0: torch.int32, 1: torch.int64, 2: torch.int16}[idx]


SENTINEL = {0: -0x5A5A5A5B, 1: -0x5A5A5A5A5A5A5A5B, 2: -1}     # (uint16: 0xFFFF is no index of a row of <= 53,248 columns)


def run_rank(block, src, n, idx, out, inp, expect_flag, refused=False):
    """One se_rank_rows call on ``block[src]`` in test-owned buffers; every assertion of a GPU case.  -> (detector word, digest)."""
    import ctypes
    import torch
    from sehip import _lib
    q = len(src)
    ldp, fill = in_pitch(inp, n), (float("-inf") if inp == NINF else float("nan"))
    ldr, c0 = out_layout(out, n, idx)
    src_d = torch.from_numpy(src).cuda()
    pd_buf = torch.full((q + 2, ldp), fill, dtype=torch.float32, device="cuda")
    pd_buf[1:q + 1, :n] = torch.from_numpy(block).cuda()[src_d]
    pd = pd_buf[1:q + 1, :n]
    rk_buf = torch.full((q + 2, ldr), SENTINEL[idx], dtype=_torch_dtype(idx), device="cuda")
    rk = rk_buf[1:q + 1, c0:c0 + n]
    assert pd_buf.data_ptr() % 256 == 0 and rk_buf.data_ptr() % 256 == 0
    assert rk.data_ptr() % 16 == out_alignment(out, n, idx) and rk.stride(0) == ldr and pd.stride(0) == ldp
    ws_bytes = (int(_lib.call("se_rank_rows_workspace_bytes", q, n)) + 255) // 256 * 256
    ws = torch.zeros((ws_bytes,), dtype=torch.uint8, device="cuda")
    ws.view(torch.int32)[16] = POISON
    if refused:
        with pytest.raises(_lib.SehipError):
            _lib.call("se_rank_rows", pd, ldp, q, n, rk, idx, ldr, ws, ws.numel())
        torch.cuda.synchronize()
        assert bool((rk_buf == SENTINEL[idx]).all())
        return None, None
    _lib.call("se_rank_rows", pd, ldp, q, n, rk, idx, ldr, ws, ws.numel())
    torch.cuda.synchronize()
    flag = int(ws.view(torch.int32)[16].item()) & 0xFFFFFFFF
    if expect_flag is not None:
        assert flag == expect_flag, "detector word %#x, expected %#x" % (flag, expect_flag)
    # the oracle sorts the block; the call's rows are laid out from it on the device
    want = ro.canon_rank_rows(block)
    plain = [r for r in range(block.shape[0]) if not np.isnan(block[r]).any() and (block[r] != 0).all()][:4]
    for r in plain:                             # no NaN, no signed zeros: NumPy's stable argsort is the same order
        assert np.array_equal(want[r], np.argsort(block[r], kind="stable")), r
    want_t = torch.from_numpy(want.astype(np.uint16).view(np.int16) if idx == 2 else want.astype({0: np.int32, 1: np.int64}[idx])).cuda()
    ok = (rk == want_t[src_d]).all(dim=1)
    if not bool(ok.all()):
        r = int(torch.nonzero(~ok)[0])
        got_r, want_r = rk[r].cpu().numpy(), want[src[r]]
        assert same_ranking(got_r[None, :], want_r[None, :], idx), "row %d (block row %d): first difference at rank %d" % (
            r, src[r], int(np.nonzero((got_r.view(np.uint16) if idx == 2 else got_r).astype(np.int64) != want_r)[0][0]))
    if q <= 64:                                 # the small calls also through the host comparator
        assert same_ranking(rk.cpu().numpy(), want[src], idx)
    # nothing written outside rank[:, :n]: pitch padding and guard rows still hold the sentinel
    digest = hashlib.sha256(rk.contiguous().cpu().numpy().tobytes()).hexdigest() if q <= 256 else None
    rk_keep = rk.clone()
    rk.fill_(SENTINEL[idx])
    assert bool((rk_buf == SENTINEL[idx]).all()), "ranks written outside the view"
    rk.copy_(rk_keep)
    # the order guard agrees, in this width
    bad = ctypes.c_int64(-1)
    cws = torch.empty((int(_lib.call("se_rank_rows_check_workspace_bytes")),), dtype=torch.uint8, device="cuda")
    _lib.call("se_rank_rows_check", pd, ldp, q, n, rk, idx, ldr, cws, cws.numel(), ctypes.byref(bad))
    assert bad.value == 0
    return flag, digest


def run_case(c, mode):
    """mode: PRODUCT (the detector word must be the predicted verdict, which is the claimed build), or a child's mode (no detector runs:
    the word must still hold the poison)."""
    block = case_block(c)
    src = case_src(c, block.shape[0])
    expect = POISON if mode != PRODUCT else case_flag(c)
    if mode == PRODUCT and c.mode == PRODUCT:
        assert expect == c.build
    return run_rank(block, src, c.n, c.idx, c.out, c.inp, expect)


@pytest.fixture(scope="module")
def sehip():
    import sehip as m
    m.lib()
    m.rank_rows_init()          # capability probe + self-test: afterwards se_rank_rows neither probes nor guards
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("items", ITEMS_TABLE)
def test_product_library_cases_vs_oracle(sehip, items):
    """Every product case of one ITEMS: ranks == canon.c, sentinels intact, the detector's word == the restated verdict == the claimed build."""
    for c in CASES:
        if c.items == items and c.mode == PRODUCT:
            flag, _ = run_case(c, PRODUCT)
            print("CASE %s flag %d" % (case_id(c), flag), flush=True)


def _child(mode_env, lib_path, digests, tmp_path, timeout):
    env = dict(os.environ, **mode_env)
    if lib_path:
        env["SEHIP_LIB"] = lib_path
    args = [sys.executable, os.path.abspath(__file__), json.dumps(mode_env)]
    if digests is not None:
        path = os.path.join(str(tmp_path), "digests.json")
        with open(path, "w") as f:
            json.dump(digests, f)
        args.append(path)
    out = subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert out.returncode == 0 and "CHILD-OK" in out.stdout, out.stdout[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_ballot_build_cases_in_one_child(tmp_path):
    """SE_RANK_SAFE=1 (read once per process): all 15 ballot instantiations; the detector is not launched, so its word keeps the poison."""
    out = _child({"SE_RANK_SAFE": "1"}, None, None, tmp_path, 900)
    for c in CASES:
        if c.mode == BALLOT:
            assert "CASE %s ok" % case_id(c) in out, case_id(c)
    assert "hardware-ordered" not in out


@pytest.mark.gpu
def test_pinned_builds_give_the_product_bytes_in_one_child_per_build(sehip, tmp_path):
    """SE_RANK_PEEL=0..3 of the tuning library on the mixed-family case of every ITEMS (builds the instantiation does not have fall to the
    plain one): each pinned build's ranks are the product run's bytes."""
    pinned = [c for c in CASES if c.mode == PINNED]
    digests = {}
    for c in pinned:
        flag, digests[case_id(c)] = run_case(c, PRODUCT)
        print("CASE %s flag %d" % (case_id(c), flag), flush=True)
    tuning = os.path.join(PKG_DIR, "sehip", "libsehip_tuning.so")
    for peel in "0123":         # one child at a time; a failing child ends the test
        out = _child({"SE_RANK_PEEL": peel}, tuning, digests, tmp_path, 900)
        for c in pinned:
            assert "CASE %s ok" % case_id(c) in out, (peel, case_id(c))


@pytest.mark.gpu
@pytest.mark.parametrize("rc", RUNS_CASES, ids=["q%d-n%d-%s-%s" % rc for rc in RUNS_CASES])
def test_long_rows_runs_and_tiled_cases_vs_oracle(sehip, rc):
    """Rows above 53,248 columns: int32 and int64 through the case's output layout, NaN / -inf in the input padding, uint16 refused with
    nothing written."""
    block = family_block(LONG, rc.n, rc.n % 1000)
    q = rc.q or block.shape[0]
    src = np.arange(q, dtype=np.int64) % block.shape[0]
    for idx in ((0,) if rc.q else (0, 1)):
        run_rank(block, src, rc.n, idx, rc.out, rc.inp, None)
    run_rank(block, src[:3], rc.n, 2, TIGHT, rc.inp, None, refused=True)


def _child_main(argv):
    import sehip
    mode_env = json.loads(argv[1])
    digests = json.load(open(argv[2])) if len(argv) > 2 else None
    sehip.lib()
    sehip.rank_rows_init()
    want_mode = BALLOT if "SE_RANK_SAFE" in mode_env else PINNED
    for c in CASES:
        if c.mode != want_mode:
            continue
        _, digest = run_case(c, want_mode)
        if digests is not None:
            assert digest == digests[case_id(c)], "%s: bytes differ from the product run" % case_id(c)
        print("CASE %s ok" % case_id(c), flush=True)
    print("CHILD-OK")


if __name__ == "__main__":
    _child_main(sys.argv)
