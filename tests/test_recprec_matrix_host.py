"""The recall-precision kernels (csrc/recprec.hip: ``relpos_kernel<CLSW, RT>``, ``rp_ap_kernel``, ``rp_sum_kernel``, ``rp_bin_kernel``;
csrc/relcount.hip: ``relcount_kernel``, ``relscan_kernel``) through every instantiation, chunk edge and launch-geometry edge: the host half.

This file restates the launch predicates of the six kernels in plain Python (a change in recprec.hip / relcount.hip / rank_stream.h has
to be mirrored at the top of this file), holds the case tables that tests/test_gpu_recprec_matrix.py runs on the device, states the
host references the device results are compared with -- written from include/sehip.h, not from the kernels -- and asserts on the CPU,
from the restatements and each case's own data alone, that the tables reach every path.  A case that drifts off its path fails here.

References:
  * positions: NumPy on the row with the query's index removed (``flatnonzero(cls[row] == qcls) + 1``), cut to R or padded with 0;
  * reduce: the header contract of ``se_recall_precision_reduce``: float64 left-to-right sums over the class's queries in ``order`` on
    top of the buffer's prior value, integer counts, ``int((j / R) * B)`` with Python floats, max per bin; AP exactly as a Fraction;
  * counting: ``tests/_qg_standins.count_preceding`` / ``count_to_positions`` (NumPy searchsorted on the canonical keys).

Recorded while restating (behaviour, not defects):
  * ``chunk_self < pos`` in relpos_kernel can be read ``<=``: the rank at ``chunk_self`` IS the query and is never a hit, so no list
    tells the two apart.
  * A row whose R hits are found stops before the chunk that holds the query; ``self_before`` is then never needed.
  * ``max_rel`` odd sizes the LDS for ``max_rel + 1`` keys: a list one longer than announced still stays in LDS.
"""
import fractions
import functools
import warnings

import numpy as np
import pytest

# ------------------------------------------------------------------ constants of recprec.hip:27-34, relcount.hip:24-30, rank_stream.h:153

WAVE = 64
RP_THREADS, RP_VEC, RP_GROUPS = 256, 4, 2
RP_WAVES = RP_THREADS // WAVE
RP_GSPAN = RP_THREADS * RP_VEC
RP_CHUNK = RP_GSPAN * RP_GROUPS
RP_HEAD_BYTES = 2 * (RP_GROUPS + 1) * RP_WAVES * 4
RP_MAX_BINS = 1 << 20
AP_GRID_CAP, SUM_GRID_CAP, BIN_GRID_CAP, SCAN_GRID_CAP = 4096, 4096, 8192, 65536
RC_THREADS, RC_VEC, RC_CHUNK, RC_KEY_BYTES = 256, 4, 16384, 12
RC_MAX_KEYS = 64 * 1024 // RC_KEY_BYTES // 2 * 2
CLASS_TABLE_LDS_CAP = 160 * 1024
NUM_CUS = 256                   # the MI355X
RESIDENT_PER_CU = tuple(range(1, 32 // RP_WAVES + 1))     # hipOccupancyMaxActiveBlocksPerMultiprocessor: 1 .. 8 workgroups of 4 waves
RESIDENT_MAX = NUM_CUS * max(RESIDENT_PER_CU)
INT32, UINT16 = "int32", "uint16"
ESIZE = {INT32: 4, UINT16: 2}
GATHER, BYTE, WORD = 0, 1, 2


# ------------------------------------------------------------------ restatements

def clsw(list_len, q, gallery, num_classes):
    """choose_class_table (rank_stream.h:155-162) with relpos_kernel's fixed LDS (recprec.hip:250) -> (CLSW, dynamic LDS bytes)."""
    fixed = RP_HEAD_BYTES
    tab8, tab16 = (gallery + 15) // 16 * 16, (gallery * 2 + 15) // 16 * 16
    if list_len * min(q, 4096) < 8 * gallery:
        return GATHER, fixed
    if num_classes <= 256 and fixed + tab8 <= CLASS_TABLE_LDS_CAP:
        return BYTE, fixed + tab8
    if num_classes <= 65536 and fixed + tab16 <= CLASS_TABLE_LDS_CAP:
        return WORD, fixed + tab16
    return GATHER, fixed


def rank_vec_ok(ldr, rt, base_offset_bytes):
    """ranks_vec_ok<RT, 4> (rank_stream.h:144-149): four ranks are one 16-byte (int32) or one 8-byte (uint16) load."""
    nbytes = min(RP_VEC * ESIZE[rt], 16)
    return (ldr * ESIZE[rt]) % nbytes == 0 and base_offset_bytes % nbytes == 0


def slab_vec_ok(ldp, base_offset_bytes):
    """aligned16(pdist, ldp, 4) (relcount.hip:151)."""
    return base_offset_bytes % 16 == 0 and (ldp * 4) % 16 == 0


def row_chunks(row, cls, qc, self_, R):
    """Chunks of 2048 ranks relpos_kernel reads of one row (recprec.hip:59, 69, 138): until R hits are counted or the list ends."""
    if R <= 0:
        return 0
    hit = (cls[row] == qc) & (row != self_)
    carry = n = 0
    for base in range(0, len(row), RP_CHUNK):
        carry += int(hit[base:base + RP_CHUNK].sum())
        n += 1
        if carry >= R:
            break
    return n


def persistent_grids(q, num_cus=NUM_CUS):
    """persistent_grid (rank_stream.h:167-175): min(q, resident workgroups per CU x CUs) -> every grid the occupancy can give.
    relpos_kernel (recprec.hip:56) strides its rows by it: workgroup b takes rows b, b + grid, b + 2 grid, ..."""
    return sorted({min(q, per_cu * num_cus) for per_cu in RESIDENT_PER_CU})


def workgroup_walks(chunks, grid):
    """What the workgroups of a grid meet in relpos_kernel's row loop: `par` (recprec.hip:55, 137) flips once per chunk and is not
    reset between rows; a row of R = 0 (0 chunks) is skipped and leaves it alone (recprec.hip:59).
    -> (the set of (par at the row's start, chunks of the row), the set of (chunks of a row, chunks of the workgroup's next row))."""
    chunks = np.asarray(chunks)
    starts, pairs = set(), set()
    for b in range(min(grid, len(chunks))):
        par, last = 0, None
        for n in chunks[b::grid].tolist():
            if n == 0:
                continue
            starts.add((par, n))
            if last is not None:
                pairs.add((last, n))
            par, last = (par + n) % 2, n
    return starts, pairs


def count_geometry(q, n_cols, max_rel):
    """se_count_preceding (relcount.hip:147-150) -> (columns per workgroup, nchunks, lds_keys)."""
    keys = RC_MAX_KEYS if (max_rel <= 0 or max_rel > RC_MAX_KEYS) else (max_rel + 1) // 2 * 2
    cols = RC_CHUNK
    while q * ((n_cols + cols - 1) // cols) > 0x40000000:
        cols *= 2
    return cols, (n_cols + cols - 1) // cols, keys


def cut_vector_steps(n_cols, cols):
    """Chunks whose last step of four columns is cut by the chunk's end c1 (relcount.hip:72, 86): only n_cols can cut one."""
    return [c for c in range((n_cols + cols - 1) // cols) if (min((c + 1) * cols, n_cols) - c * cols) % RC_VEC]


def ap_grid(q):
    """rp_ap_kernel (recprec.hip:289-290): a wave per query -> (workgroups, a wave takes a second query)."""
    g = (q + RP_WAVES - 1) // RP_WAVES
    return min(g, AP_GRID_CAP), g > AP_GRID_CAP


def sum_grid(class_len, class_off_last):
    """rp_sum_kernel (recprec.hip:166-167, 293-294): a thread per (class, j) -> (workgroups, a thread takes a second element)."""
    g = (class_len + RP_THREADS - 1) // RP_THREADS
    grid = min(g, SUM_GRID_CAP)
    return grid, min(class_off_last, class_len) > grid * RP_THREADS


def bin_grid(C, B):
    """rp_bin_kernel (recprec.hip:211-212, 299-300): a wave per (class, bin) -> (workgroups, a wave takes a second pair)."""
    g = (C * (B + 1) + RP_WAVES - 1) // RP_WAVES
    grid = min(g, BIN_GRID_CAP)
    return grid, C * (B + 1) > grid * RP_WAVES


def scan_grid(q):
    """relscan_kernel (relcount.hip:163): a workgroup per query -> (workgroups, a workgroup takes a second query)."""
    return min(q, SCAN_GRID_CAP), q > SCAN_GRID_CAP


def py_bin(j, R, B):
    """The contract's bin of hit j of R (sehip.h, se_recall_precision_reduce): Python floats."""
    return int((j / R) * B)


def bin_hits(R, B):
    """How many j of 1 .. R fall into each bin that has any."""
    out = {}
    for j in range(1, R + 1):
        out[py_bin(j, R, B)] = out.get(py_bin(j, R, B), 0) + 1
    return out


# ------------------------------------------------------------------ positions: the case table

LS = (1, 2, 2047, 2048, 2049, 4097, 6148)
SELF_AT = (0, 1, 255, 256, 2046, 2047, 2048, 2049, 4095, 4096)     # and L - 1
GATHER_CLASSES, WORD_CLASSES, BYTE_CLASSES = 70000, 300, 16       # num_classes of the call: above every table / above the byte table
# (pitch padding in elements on top of L rounded up to 4, bytes the base lies behind 16-byte alignment); both types take the same
LAYOUTS = ((0, 0), (4, 8), (1, 0), (0, 4), (8, 0), (2, 8), (4, 0))


def _pos_case(name, L, G, Q, num_classes, layout, kind="scenarios", qidx="given", rt=(INT32, UINT16)):
    pad, off_bytes = layout
    return dict(name=name, L=L, G=G, Q=Q, num_classes=num_classes, ldr=(L + 3) // 4 * 4 + pad, off_bytes=off_bytes, kind=kind, qidx=qidx, rt=rt)


def _pos_cases():
    out = []
    for n, L in enumerate(LS):
        small = L <= 2
        G = 16 if small else L + L // 4 + 64
        Q = 128 if small else 44
        for w, nc in ((GATHER, GATHER_CLASSES), (BYTE, BYTE_CLASSES), (WORD, WORD_CLASSES)):
            out.append(_pos_case("L%d-w%d" % (L, w), L, G, Q, nc, LAYOUTS[(n + w) % len(LAYOUTS)]))
    out.append(_pos_case("few-queries-gather", 2049, 2049 + 512 + 64, 9, BYTE_CLASSES, (0, 0)))
    out.append(_pos_case("null-qidx-4097", 4097, 4097 + 1024 + 64, 44, BYTE_CLASSES, (0, 0), qidx="null"))
    out.append(_pos_case("null-qidx-2", 2, 16, 128, WORD_CLASSES, (1, 4), qidx="null"))
    out.append(_pos_case("q5000-37", 37, 300, 5000, BYTE_CLASSES, (3, 0), kind="short"))
    out.append(_pos_case("q3000-2049", 2049, 2049 + 512 + 64, 3000, BYTE_CLASSES, (3, 0), kind="alternating"))
    out.append(_pos_case("q3000-2049-mixed", 2049, 2049 + 512 + 64, 3000, BYTE_CLASSES, (3, 0), kind="mixed"))
    return out


POS_CASES = _pos_cases()
POS_BY_NAME = {c["name"]: c for c in POS_CASES}
POS_WANTED_CLSW = {c["name"]: int(c["name"].split("-w")[1]) for c in POS_CASES if "-w" in c["name"]}
POS_WANTED_CLSW.update({"few-queries-gather": GATHER, "null-qidx-4097": BYTE, "null-qidx-2": WORD, "q5000-37": BYTE, "q3000-2049": BYTE,
                        "q3000-2049-mixed": BYTE})


def pos_case_clsw(c):
    return clsw(c["L"], c["Q"], c["G"], c["num_classes"])[0]


def pos_case_vec_ok(c, rt):
    return rank_vec_ok(c["ldr"], rt, c["off_bytes"])


def _class_ids(num_classes, n_used):
    """Class values in use, in pairs that a narrower table would confuse: (m, m + 256) once the byte table is out, (m, m + 65536)
    once the 16-bit table is out as well."""
    ids = []
    for m in range(n_used // 2):
        step = n_used // 2
        if num_classes > 256:
            step = 256
        if num_classes > 65536 and m % 2:
            step = 65536
        ids += [m, m + step]
    assert max(ids) < num_classes and len(set(ids)) == n_used
    return np.array(ids, dtype=np.int32)


def _scenarios(L, rng):
    """-> [(position of the query or None, raw positions of the relevant items, how the query is absent, R - hits present)]."""
    def some(n, lo=0, hi=L):
        return set(rng.integers(lo, hi, size=n).tolist()) if hi > lo else set()

    out = []
    if L <= 2:
        for sp in sorted({0, L - 1}) + [None]:
            free = [p for p in range(L) if p != sp]
            for hits in ([], free[:1], free):
                for extra in (0, 3):
                    out.append((sp, set(hits), "in" if sp is not None else ("minus1", "notinlist")[len(hits) % 2], extra))
        out.append((None, set(), "in", "zero"))
        return out
    for sp in sorted({p for p in SELF_AT if p < L} | {L - 1}):
        run = {4 * (sp // 4) + k for k in range(4)}
        out.append((sp, ({sp - 1, sp + 1} | run | some(6) | {L - 1}), "in", 0))      # neighbours and the query's own run of four ranks
        out.append((sp, some(9), "in", 0))
    if L > RP_CHUNK:
        out.append((L - 1, some(8, 0, RP_CHUNK) | {RP_CHUNK - 1}, "in", 0))          # the query in a chunk the row does not read
        out.append((min(RP_CHUNK + 2, L - 1), some(5, 0, RP_CHUNK) | {RP_CHUNK - 1}, "in", -2))  # cut to R inside chunk 0: chunk 1 is not read
    out.append((1000, some(7, 0, 100), "in", 0))                                     # behind the last hit, inside the chunk it reads
    out.append((None, some(9) | {0, L - 1}, "minus1", 0))
    out.append((None, some(9) | {0, L - 1}, "notinlist", 0))
    out.append((L // 2, some(9), "in", "zero"))                                      # hit_off says R = 0: the row is not read at all
    out.append((L // 3, some(9) | {L // 3 + 1}, "in", 3))                            # three hits promised that do not exist
    out.append((3, set(), "in", 0))                                                  # R = 0 and no relevant item either
    out.append((None, some(5), "minus1", 3))
    late = {RP_CHUNK + 1, RP_CHUNK + 7, L - 2, L - 1} if L > 2 * RP_CHUNK else {L - 1}
    out.append((5, some(6, 0, RP_CHUNK) | {4, 6} | late, "in", -2))                  # two hits more than promised, in a chunk it reads
    return out


@functools.lru_cache(maxsize=None)
def pos_data(name):
    """The operands of a case and the NumPy expectation: rk [Q, L] int64, cls [G], qcls [Q], qidx [Q] or None, hit_off [Q + 1],
    want [hit_off[Q]] int32, chunks [Q] (row_chunks)."""
    c = POS_BY_NAME[name]
    L, G, Q = c["L"], c["G"], c["Q"]
    rng = np.random.default_rng(L * 1000003 + G * 101 + Q * 7 + c["num_classes"])
    n_used = 4 if G < 64 else 16
    ids = _class_ids(c["num_classes"], n_used)
    cls = ids[rng.permutation(G) % n_used]
    rk = np.empty((Q, L), dtype=np.int64)
    qcls, qidx, R = np.empty(Q, dtype=np.int32), np.empty(Q, dtype=np.int32), np.empty(Q, dtype=np.int64)
    if c["kind"] == "scenarios":
        plan = _scenarios(L, rng)
        plan = [plan[i % len(plan)] for i in range(Q - 1)] + [plan[-1] if L > 2 else plan[0]]    # L > 2: the last row has hits behind its R
    elif c["kind"] == "short":
        plan = [(int(rng.integers(0, L)), set(rng.integers(0, L, size=int(rng.integers(0, 7))).tolist()), "in", 0) for _ in range(Q)]
    else:
        # alternating: odd rows find all their hits in chunk 0, even rows need chunk 1.  The grid is a multiple of the 256 CUs, so a
        # workgroup's rows b, b + grid, ... all have b's parity and with it ONE chunk count; only neighbouring workgroups differ.
        # mixed: the chunk count of a row is drawn per row, so that under every grid workgroups meet 2 chunks then 1, 1 then 2, and
        # start rows of either kind on either half of the double buffer (test_positions_many_queries_per_workgroup).
        two = (np.arange(Q) % 2 == 0) if c["kind"] == "alternating" else (rng.integers(0, 2, size=Q) == 1)
        plan = [(int(rng.integers(0, L - 1)), set(rng.integers(0, RP_CHUNK, size=5).tolist()) | ({L - 1} if two[i] else set()), "in", 0)
                for i in range(Q)]
    for i, (sp, hits, absent, extra) in enumerate(plan):
        if c["qidx"] == "null":
            sp, absent = None, "minus1"
        qc = int(ids[i % n_used])
        members = rng.permutation(np.flatnonzero(cls == qc))
        others = rng.permutation(np.flatnonzero(cls != qc))
        self_item, members = int(members[0]), members[1:]
        hits = sorted(p for p in hits if 0 <= p < L and p != sp)[:len(members)]
        row = np.full(L, -1, dtype=np.int64)
        row[hits] = members[:len(hits)]
        if sp is not None:
            row[sp] = self_item
        free = row < 0
        row[free] = others[:int(free.sum())]
        rk[i], qcls[i] = row, qc
        qidx[i] = self_item if (sp is not None or absent == "notinlist") else -1
        R[i] = 0 if extra == "zero" else len(hits) + extra
    assert (R >= 0).all() and all(len(set(r.tolist())) == L for r in rk[:64])
    hit_off = np.concatenate([[0], np.cumsum(R)]).astype(np.int64)
    qidx_arg = None if c["qidx"] == "null" else qidx
    want = positions_reference(rk, cls, qcls, qidx_arg, hit_off)
    chunks = np.array([row_chunks(rk[i], cls, qcls[i], -1 if qidx_arg is None else qidx[i], R[i]) for i in range(Q)])
    return dict(rk=rk, cls=cls, qcls=qcls, qidx=qidx_arg, hit_off=hit_off, want=want, chunks=chunks)


def positions_reference(rk, cls, qcls, qidx, hit_off):
    """hit_pos of se_relevant_positions by its header: per query the 1-based places of the items of its class in its row without the
    query; a hit_off that promises more reads 0 there, one that promises fewer gets the first R."""
    out = np.zeros(int(hit_off[-1]), dtype=np.int32)
    for i in range(len(rk)):
        row = rk[i] if qidx is None else rk[i][rk[i] != qidx[i]]
        pos = np.flatnonzero(cls[row] == qcls[i]) + 1
        R = int(hit_off[i + 1] - hit_off[i])
        n = min(R, len(pos))
        out[hit_off[i]:hit_off[i] + n] = pos[:n]
    return out


# ------------------------------------------------------------------ reduce: the reference and the case table

def exact_ap(p):
    """(1 / R) sum_j j / p_j as a Fraction (0 for R = 0); equal terms are added once, times their count."""
    R = len(p)
    if R == 0:
        return fractions.Fraction(0)
    j = np.arange(1, R + 1, dtype=np.int64)
    p = np.asarray(p, dtype=np.int64)
    g = np.gcd(j, p)
    terms, counts = np.unique(((j // g) << 32) | (p // g), return_counts=True)
    total = fractions.Fraction(0)
    for t, n in zip(terms.tolist(), counts.tolist()):
        total += fractions.Fraction((t >> 32) * n, t & 0xFFFFFFFF)
    return total / R


def reduce_reference(hit_pos, hit_off, order, class_start, class_off, bins, prec_sum, first_miss, bin_sum, bin_count):
    """One call of se_recall_precision_reduce on NumPy arrays, by the header: adds into prec_sum [class_len], first_miss [C],
    bin_sum / bin_count [C, bins + 1] in place, in the contract's order; -> the exact AP of every query (Fractions)."""
    q, C = len(hit_off) - 1, len(class_start) - 1
    ap = [exact_ap(hit_pos[hit_off[i]:hit_off[i + 1]]) for i in range(q)]
    for c in range(C):
        a, b = int(class_off[c]), int(class_off[c + 1])
        Rc = b - a
        if Rc == 0:
            continue
        j = np.arange(1, Rc + 1, dtype=np.float64)
        which = [py_bin(jj, Rc, bins) for jj in range(1, Rc + 1)] if bins else None
        for k in range(int(class_start[c]), int(class_start[c + 1])):
            i = int(order[k])
            p = hit_pos[hit_off[i]:hit_off[i + 1]]
            assert len(p) == Rc, "all queries of a class have the class's R"
            prec = j / p.astype(np.float64)
            prec_sum[a:b] = prec_sum[a:b] + prec                     # element by element: one more term on the left-to-right sum
            first_miss[c] += int(p[0] > 1)
            if bins:
                best = {0: 0.0} if p[0] > 1 else {}
                for bi, v in zip(which, prec.tolist()):
                    best[bi] = max(best[bi], v) if bi in best else v
                for bi, v in best.items():
                    bin_sum[c, bi] = bin_sum[c, bi] + v
                    bin_count[c, bi] += 1
    return ap


R_EDGES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000)
BIN_RS = (1, 2, 3, 5, 7, 10, 64, 65, 100, 200, 1000)
BIN_BS = (1, 2, 7, 10, 100, 1000)
POS_MAX = 2 ** 31 - 1
BIG_R = 1048700


def _reduce_cases():
    """R: relevant items per class; NQ: queries per class in the problem; B: every `bins` the problem is run with; tilings: rows per
    tile (0: one tile)."""
    out = [dict(name="r-edges", R=(0, 1, 2, 63, 0, 0, 64, 65, 127, 17, 128, 129, 1000, 0), NQ=(2, 3, 2, 3, 0, 1, 3, 2, 3, 0, 2, 3, 3, 0),
                B=(0, 7), tilings=(0, 13, 1)),
           dict(name="ap-stride", R=(1, 3), NQ=(9000, 11000), B=(0,), tilings=(0,)),
           dict(name="sum-stride", R=(5, BIG_R, 3), NQ=(2, 2, 2), B=(0,), tilings=(0,), style="big")]
    for B in BIN_BS:
        R = BIN_RS + ((0,) + BIN_RS * 3)[:40 - len(BIN_RS)] if B == 1000 else BIN_RS
        out.append(dict(name="bins-%d" % B, R=R, NQ=tuple(3 if r != 200 else 4 for r in R), B=(B,), tilings=(0, 7) if B == 100 else (0,)))
    out.append(dict(name="bins-2^20", R=(3, 1000), NQ=(3, 2), B=(RP_MAX_BINS,), tilings=(0,)))
    return out


REDUCE_CASES = _reduce_cases()
REDUCE_BY_NAME = {c["name"]: c for c in REDUCE_CASES}


def reduce_pairs():
    return sorted({(r, b) for c in REDUCE_CASES for b in c["B"] if b for r in c["R"] if r})


@functools.lru_cache(maxsize=None)
def reduce_data(name):
    """-> qcls [Q] (queries in mixed class order), pos: list of Q int32 arrays (R sorted distinct positions), class_off [C + 1]."""
    c = REDUCE_BY_NAME[name]
    rng = np.random.default_rng(len(name) * 7919 + sum(c["R"]))
    qcls = rng.permutation(np.repeat(np.arange(len(c["R"])), c["NQ"])).astype(np.int32)
    seen, pos = {}, []
    for cl in qcls.tolist():
        R, k = c["R"][cl], seen.get(cl, 0)
        seen[cl] = k + 1
        if c.get("style") == "big" and R == BIG_R:
            p = np.arange(1, R + 1, dtype=np.int64) * (k + 1)          # AP exactly 1, then exactly 1 / 2 with a first-position miss
        elif k % 3 == 0:
            p = np.arange(1, R + 1, dtype=np.int64)                    # p_j = j
        else:
            p = np.cumsum(rng.integers(1, 9 if k % 2 else 3, size=R))
            if k % 3 == 1 and R:
                p += int(rng.integers(1, 5))                           # p_1 > 1: the recall-0 point
            if k % 3 == 2 and R:
                p[-1] = POS_MAX                                        # the largest position an int32 holds
        assert (np.diff(p) > 0).all() and (R == 0 or (p[0] >= 1 and p[-1] <= POS_MAX))
        pos.append(p.astype(np.int32))
    class_off = np.concatenate([[0], np.cumsum(c["R"])]).astype(np.int64)
    return dict(qcls=qcls, pos=pos, class_off=class_off)


def reduce_tiles(name, rows):
    """The calls of a tiling: [(q0, hit_pos, hit_off, order, class_start)] -- tile-local query indices, order by class then index."""
    c, d = REDUCE_BY_NAME[name], reduce_data(name)
    Q, C = len(d["qcls"]), len(c["R"])
    out = []
    for q0 in range(0, Q, rows or Q):
        qc = d["qcls"][q0:q0 + (rows or Q)]
        pos = d["pos"][q0:q0 + (rows or Q)]
        hit_off = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
        hit_pos = np.concatenate(pos + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
        order = np.argsort(qc, kind="stable").astype(np.int32)
        class_start = np.concatenate([[0], np.cumsum(np.bincount(qc, minlength=C))]).astype(np.int32)
        out.append((q0, hit_pos, hit_off, order, class_start))
    return out


def reduce_prior(name, bins):
    """Accumulators that earlier tiles might have left: random values, never zero."""
    c, d = REDUCE_BY_NAME[name], reduce_data(name)
    C, n = len(c["R"]), int(d["class_off"][-1])
    rng = np.random.default_rng(bins + 17)
    return (rng.random(n) * 8, rng.integers(1, 1000, size=C).astype(np.int64), rng.random((C, bins + 1)) * 8,
            rng.integers(1, 1000, size=(C, bins + 1)).astype(np.int64))


@functools.lru_cache(maxsize=None)
def reduce_expected(name, bins):
    """The whole problem in one tile on top of reduce_prior -> (ap Fractions, prec_sum, first_miss, bin_sum, bin_count)."""
    d = reduce_data(name)
    (_, hit_pos, hit_off, order, class_start), = reduce_tiles(name, 0)
    ps, fm, bs, bc = reduce_prior(name, bins)
    ap = reduce_reference(hit_pos, hit_off, order, class_start, d["class_off"], bins, ps, fm, bs, bc)
    return ap, ps, fm, bs, bc


# ------------------------------------------------------------------ counting: the case table

COUNT_N = 32773
COUNT_COLS = (16383, 16384, 16385, 32773)
COUNT_SAME = (RC_CHUNK - 20, RC_CHUNK + 20)            # 40 identical columns across column 16,384
COUNT_R = (300, 0, 7, 1, 700)                          # relevant items of the five queries
COUNT_SELF = {16383: (16382, -1, 5, 16000, 0), 16384: (16380, -1, 5, 16000, 0), 16385: (16384, -1, 5, 16383, 0),
              32773: (20000, -1, 16384, 5, 32772)}     # the queries' own columns: second chunk, absent, chunk edges
COUNT_SLABS = (0, 4999, 16381, 16387, 32773)           # the same gallery as slabs cut at odd columns
SLAB_LAYOUTS = ((3, 0), (0, 4), (4, 8), (0, 0))        # (pitch padding on top of the columns rounded up to 4, base offset in bytes)
KEY_RS = (1, 255, 256, 257, RC_MAX_KEYS, RC_MAX_KEYS + 1)
KEY_COLS = 6003
SCAN_RS = (255, 256, 257, 513, 1025)
SCAN_BIG_Q = 65541
NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00001


def key_max_rels(R):
    return (0, R, R - 1, 10 ** 6)


def _special_distances(rng, pd):
    """NaN of both signs, -0, +0 and +inf at random columns, the 40 identical columns across the chunk edge."""
    u = pd.view(np.uint32)
    for val in (NAN_POS, NAN_NEG, 0x80000000, 0x00000000, 0x7F800000):
        at = rng.random(pd.shape) < 0.01
        u[at] = val
    lo, hi = COUNT_SAME
    if pd.shape[1] >= hi:
        pd[:, lo:hi] = 3.25
    return pd


@functools.lru_cache(maxsize=None)
def count_gallery():
    """[5, 32773] float32 distances on a grid of values (many ties), with the special values."""
    rng = np.random.default_rng(32773)
    return _special_distances(rng, (rng.integers(0, 300, size=(len(COUNT_R), COUNT_N)) / 16).astype(np.float32))


def count_keys(pd, Rs, selfs, n_cols, seed):
    """Relevant items of every query among columns 0 .. n_cols (never the query's own), sorted in the canonical order
    -> hit_off, rel_d, rel_i.  They include identical columns on both sides of the edge and columns of every special value."""
    from _qg_standins import canon_keys
    rng = np.random.default_rng(seed)
    rel_d, rel_i = [], []
    for i, R in enumerate(Rs):
        cand = rng.permutation(n_cols)
        must = [c for c in (COUNT_SAME[0], COUNT_SAME[0] + 1, RC_CHUNK - 1, RC_CHUNK, COUNT_SAME[1] - 1) if c < n_cols]
        u = pd[i, :n_cols].view(np.uint32)
        for val in (NAN_POS, NAN_NEG, 0x80000000, 0x00000000, 0x7F800000):
            must += np.flatnonzero(u == val)[:2].tolist()
        idx = np.array(list(dict.fromkeys([c for c in must + cand.tolist() if c != selfs[i]]))[:R], dtype=np.int64)
        idx = idx[np.argsort(canon_keys(pd[i, idx], idx), kind="stable")]
        rel_i.append(idx.astype(np.int32))
        rel_d.append(pd[i, idx])
    hit_off = np.concatenate([[0], np.cumsum([len(x) for x in rel_i])]).astype(np.int64)
    return hit_off, np.concatenate(rel_d).astype(np.float32), np.concatenate(rel_i).astype(np.int32)


def count_reference(pd, col_offset, hit_off, rel_d, rel_i, qidx, prior):
    """cnt after one se_count_preceding on top of `prior`, by tests/_qg_standins.count_preceding."""
    import torch
    from _qg_standins import count_preceding
    t = torch.from_numpy
    cnt = t(prior.copy())
    count_preceding(t(np.ascontiguousarray(pd)), col_offset, t(hit_off), t(rel_d), t(rel_i), qidx, cnt)
    return cnt.numpy()


@functools.lru_cache(maxsize=None)
def count_case(n_cols):
    """-> pd [5, n_cols], hit_off, rel_d, rel_i, qidx, prior, want (the counts on top of prior)."""
    pd = count_gallery()[:, :n_cols]
    qidx = np.array(COUNT_SELF[n_cols], dtype=np.int32)
    hit_off, rel_d, rel_i = count_keys(pd, COUNT_R, qidx, n_cols, n_cols)
    prior = np.random.default_rng(n_cols).integers(0, 10, size=int(hit_off[-1])).astype(np.int32)
    return dict(pd=pd, hit_off=hit_off, rel_d=rel_d, rel_i=rel_i, qidx=qidx, prior=prior,
                want=count_reference(pd, 0, hit_off, rel_d, rel_i, qidx, prior))


@functools.lru_cache(maxsize=None)
def key_case(R):
    """Three queries on 6,003 columns: a key list of R, none, a list of 3 -> as count_case, prior 0."""
    rng = np.random.default_rng(R)
    pd = _special_distances(rng, (rng.integers(0, 300, size=(3, KEY_COLS)) / 16).astype(np.float32))
    qidx = np.array([KEY_COLS - 1, 7, -1], dtype=np.int32)
    hit_off, rel_d, rel_i = count_keys(pd, (R, 0, 3), qidx, KEY_COLS, R)
    prior = np.zeros(int(hit_off[-1]), dtype=np.int32)
    return dict(pd=pd, hit_off=hit_off, rel_d=rel_d, rel_i=rel_i, qidx=qidx, prior=prior,
                want=count_reference(pd, 0, hit_off, rel_d, rel_i, qidx, prior))


def scan_reference(cnt, hit_off):
    import torch
    from _qg_standins import count_to_positions
    return count_to_positions(torch.from_numpy(cnt.copy()), torch.from_numpy(hit_off)).numpy()


@functools.lru_cache(maxsize=None)
def scan_case(big):
    rng = np.random.default_rng(65541 if big else 1025)
    Rs = rng.integers(0, 4, size=SCAN_BIG_Q) if big else np.array((0,) + SCAN_RS + (1, 0))
    hit_off = np.concatenate([[0], np.cumsum(Rs)]).astype(np.int64)
    cnt = rng.integers(0, 1000, size=int(hit_off[-1])).astype(np.int32)
    return dict(cnt=cnt, hit_off=hit_off, want=scan_reference(cnt, hit_off))


# ------------------------------------------------------------------ CPU tests: the restatements

def test_constants():
    assert (RP_CHUNK, RP_HEAD_BYTES, RC_MAX_KEYS) == (2048, 96, 5460)
    assert AP_GRID_CAP * RP_WAVES == 16384 and SUM_GRID_CAP * RP_THREADS == 1048576 and BIN_GRID_CAP * RP_WAVES == 32768


def test_restated_predicates_at_their_edges():
    assert clsw(37, 4095, 18944, 16)[0] == GATHER and clsw(37, 4096, 18944, 16)[0] == BYTE and clsw(37, 10 ** 6, 18945, 16)[0] == GATHER
    assert clsw(100, 100, 100, 256) == (BYTE, 96 + 112) and clsw(100, 100, 100, 257) == (WORD, 96 + 208)
    assert clsw(10 ** 6, 100, 163744, 16)[0] == BYTE and clsw(10 ** 6, 100, 163745, 16)[0] == GATHER     # 96 + 163,744 = 160 KB
    assert clsw(10 ** 6, 100, 81872, 300)[0] == WORD and clsw(10 ** 6, 100, 81873, 300)[0] == GATHER
    assert clsw(100, 100, 100, 65537)[0] == GATHER
    assert rank_vec_ok(8, INT32, 0) and not rank_vec_ok(8, INT32, 8) and not rank_vec_ok(6, INT32, 0)
    assert rank_vec_ok(8, UINT16, 8) and not rank_vec_ok(8, UINT16, 4) and not rank_vec_ok(6, UINT16, 0) and rank_vec_ok(12, UINT16, 0)
    assert slab_vec_ok(8, 0) and not slab_vec_ok(8, 8) and not slab_vec_ok(6, 0)
    assert count_geometry(5, 16384, 0) == (16384, 1, 5460) and count_geometry(5, 16385, 7) == (16384, 2, 8)
    assert count_geometry(5, 100, 5460)[2] == 5460 and count_geometry(5, 100, 5461)[2] == 5460 and count_geometry(5, 100, 5459)[2] == 5460
    assert count_geometry(2 ** 20, 16384 * 1024 + 1, 0)[:2] == (32768, 513)
    assert ap_grid(16384) == (4096, False) and ap_grid(16385) == (4096, True)
    assert sum_grid(1048576, 1048576) == (4096, False) and sum_grid(1048577, 1048577) == (4096, True)
    assert bin_grid(32, 1023) == (8192, False) and bin_grid(40, 1000) == (8192, True)
    assert scan_grid(65536) == (65536, False) and scan_grid(65537) == (65536, True)


# ------------------------------------------------------------------ CPU tests: the positions table reaches its paths

def test_positions_every_class_source_rank_type_and_length():
    reached = {(pos_case_clsw(c), rt, c["L"]) for c in POS_CASES for rt in c["rt"]}
    assert reached >= {(w, rt, L) for w in (GATHER, BYTE, WORD) for rt in (INT32, UINT16) for L in LS}
    for c in POS_CASES:
        assert pos_case_clsw(c) == POS_WANTED_CLSW[c["name"]], c["name"]
        assert c["G"] <= 65536 and c["ldr"] >= c["L"]
    few = POS_BY_NAME["few-queries-gather"]
    assert few["num_classes"] <= 256 and clsw(few["L"], 4096, few["G"], few["num_classes"])[0] == BYTE      # gathered for its 9 queries alone
    for rt in (INT32, UINT16):            # rows of several chunks with and without vector loads, in both types
        assert {pos_case_vec_ok(c, rt) for c in POS_CASES if c["L"] > RP_CHUNK} == {True, False}
    assert any(pos_case_vec_ok(c, UINT16) and not pos_case_vec_ok(c, INT32) for c in POS_CASES)            # a base 8 bytes off
    assert {c["off_bytes"] for c in POS_CASES} >= {0, 4, 8}


def test_positions_classes_a_narrower_table_would_confuse():
    for c in POS_CASES:
        if c["kind"] != "scenarios":
            continue
        used = set(pos_data(c["name"])["cls"].tolist())
        if c["num_classes"] > 256:
            assert any(v + 256 in used for v in used), c["name"]
        if c["num_classes"] > 65536:
            assert any(v + 65536 in used for v in used), c["name"]
        if pos_case_clsw(c) == BYTE:
            assert max(used) < 256


@pytest.mark.parametrize("name", [c["name"] for c in POS_CASES if "-w" in c["name"]])
def test_positions_scenarios_reach_their_paths(name):
    c, d = POS_BY_NAME[name], pos_data(name)
    L, Q = c["L"], c["Q"]
    rk, cls, qcls, qidx, off = d["rk"], d["cls"], d["qcls"], d["qidx"], d["hit_off"]
    R = np.diff(off)
    at = [np.flatnonzero(rk[i] == qidx[i]) for i in range(Q)]
    sp = [int(a[0]) if len(a) else None for a in at]
    hit = [(cls[rk[i]] == qcls[i]) & (rk[i] != qidx[i]) for i in range(Q)]
    have = np.array([int(h.sum()) for h in hit])
    assert {p for p in sp if p is not None} >= {p for p in SELF_AT if p < L} | {L - 1}
    assert any(qidx[i] == -1 for i in range(Q)) and any(qidx[i] >= 0 and sp[i] is None for i in range(Q))          # both ways of being absent
    assert any(R[i] == have[i] + 3 for i in range(Q)), "three hits promised that the row does not have"
    assert any(R[i] == 0 and 0 < i < Q - 1 and R[i - 1] > 0 and R[i + 1] > 0 for i in range(Q)), "R = 0 between other rows"
    if L > 2:
        assert R[-1] == have[-1] - 2 and R[-1] > 0, "the last row has hits behind its R: the guard is behind it"
        assert any(R[i] == 0 and have[i] > 0 for i in range(Q))
        both = [i for i in range(Q) if sp[i] not in (None, 0, L - 1) and hit[i][sp[i] - 1] and hit[i][sp[i] + 1]]
        assert both, "relevant items directly before and after the query"
        # every other rank of the query's run of four that the list has is a hit (L = 2047 ends inside the run of its last rank)
        run = [i for i in range(Q) if sp[i] is not None
               and hit[i][4 * (sp[i] // 4):4 * (sp[i] // 4) + 4].sum() == min(4 * (sp[i] // 4) + 4, L) - 4 * (sp[i] // 4) - 1 >= 2]
        assert {sp[i] % 4 for i in run} == {0, 1, 2, 3}, "the query in every slot of its run of four"
        assert {sp[i] % 4 for i in run if i in both} >= {0, 1, 3} and (L == 2047 or any(sp[i] % 4 == 2 for i in run if i in both))
        assert any(sp[i] is not None and have[i] and sp[i] > np.flatnonzero(hit[i])[-1] and sp[i] // RP_CHUNK < d["chunks"][i]
                   for i in range(Q)), "behind the last hit, in a chunk the row reads"
    if L > RP_CHUNK:
        assert any(sp[i] is not None and R[i] > 0 and sp[i] // RP_CHUNK >= d["chunks"][i] for i in range(Q)), "the query in an unread chunk"
        assert any(0 < R[i] < have[i] and d["chunks"][i] == 1 for i in range(Q))
        assert L < 2 * RP_CHUNK or any(0 < R[i] < have[i] and d["chunks"][i] > 1 for i in range(Q))
        assert set(d["chunks"].tolist()) >= set(range((L + RP_CHUNK - 1) // RP_CHUNK + 1))
        # hits in a chunk behind the query's chunk (self_before), with the query in chunk 0 and in a later one
        later = [sp[i] // RP_CHUNK for i in range(Q)
                 if sp[i] is not None and sp[i] // RP_CHUNK < d["chunks"][i] - 1 and hit[i][(sp[i] // RP_CHUNK + 1) * RP_CHUNK:].any()]
        assert 0 in later and (L < 2 * RP_CHUNK or max(later) > 0)


def test_positions_null_qidx_cases():
    for name in ("null-qidx-4097", "null-qidx-2"):
        d = pos_data(name)
        assert d["qidx"] is None and np.diff(d["hit_off"]).max() > 0


def test_positions_many_queries_per_workgroup():
    short, alt, mixed = POS_BY_NAME["q5000-37"], POS_BY_NAME["q3000-2049"], POS_BY_NAME["q3000-2049-mixed"]
    assert (short["Q"], short["L"], alt["Q"], alt["L"], mixed["Q"], mixed["L"]) == (5000, 37, 3000, 2049, 3000, 2049)
    assert min(short["Q"], alt["Q"], mixed["Q"]) > RESIDENT_MAX           # more rows than workgroups can be resident: several rows each
    assert set(np.diff(pos_data("q5000-37")["hit_off"]).tolist()) >= {0, 1, 2, 3}
    ch = pos_data("q3000-2049")["chunks"]
    assert (ch[0::2] == 2).all() and (ch[1::2] == 1).all()                # odd rows end in chunk 0, even rows need chunk 1
    assert_par_carries("q3000-2049-mixed", NUM_CUS)
    for grid in persistent_grids(alt["Q"]):                               # an even stride keeps a workgroup on rows of one parity
        assert workgroup_walks(ch, grid)[1] <= {(1, 1), (2, 2)}
    assert workgroup_walks(ch, 255)[1] == {(1, 2), (2, 1)}                # ... an odd one would not
    # rows 0, 2, 4 = 1, 2, 1 chunks: starts on halves 0, 1, 1; rows 1, 3, 5 = skipped, 2, 1: starts on halves 0, 0
    assert workgroup_walks([1, 0, 2, 2, 1, 1], 2) == ({(0, 1), (1, 2), (1, 1), (0, 2)}, {(1, 2), (2, 1)})
    assert workgroup_walks([1, 0, 2, 2, 1, 1], 6) == ({(0, 1), (0, 2)}, set())


def assert_par_carries(name, num_cus):
    """Whatever occupancy persistent_grid finds on `num_cus` CUs: some workgroup runs a 2-chunk row and then a 1-chunk row, some the
    reverse, and rows of either kind start on either half of the s_cnt / s_self double buffer."""
    c, ch = POS_BY_NAME[name], pos_data(name)["chunks"]
    grids = persistent_grids(c["Q"], num_cus)
    assert grids[-1] < c["Q"], "no workgroup takes a second row at full occupancy"
    for grid in grids:
        starts, pairs = workgroup_walks(ch, grid)
        assert starts >= {(0, 1), (0, 2), (1, 1), (1, 2)} and pairs >= {(1, 2), (2, 1)}, (name, grid, starts, pairs)


# ------------------------------------------------------------------ CPU tests: the reduce table reaches its paths

def test_reduce_table_reaches_every_path():
    edges = REDUCE_BY_NAME["r-edges"]
    assert set(edges["R"]) >= set(R_EDGES)
    R, NQ = edges["R"], edges["NQ"]
    assert R[0] == 0 and R[-1] == 0 and any(R[i] == 0 and R[i + 1] == 0 and 0 < i < len(R) - 2 for i in range(len(R) - 1))
    assert any(r == 0 and n > 0 for r, n in zip(R, NQ)) and any(r > 0 and n == 0 for r, n in zip(R, NQ))
    assert 0 in edges["tilings"] and 1 in edges["tilings"] and len(edges["tilings"]) == 3
    assert -(-sum(NQ) // 13) == 3                                         # three tiles
    tiles = reduce_tiles("r-edges", 13)
    assert any((np.diff(t[4]) == 0)[[i for i, r in enumerate(R) if r > 0]].any() for t in tiles)   # a class without a query in a tile
    assert max(R_EDGES) > WAVE and 65 in R and 129 in R                   # rp_ap_kernel's lanes take a second and a third j
    ap = REDUCE_BY_NAME["ap-stride"]
    assert sum(ap["NQ"]) == 20000 and set(ap["R"]) == {1, 3} and ap_grid(sum(ap["NQ"]))[1]
    big = REDUCE_BY_NAME["sum-stride"]
    off = np.concatenate([[0], np.cumsum(big["R"])])
    assert big["R"][1] == BIG_R and big["NQ"][1] == 2 and sum_grid(int(off[-1]), int(off[-1]))[1]
    assert off[1] < SUM_GRID_CAP * RP_THREADS < off[2]                    # the second trip starts inside the large class
    for name in ("r-edges", "ap-stride", "bins-7", "bins-1000"):
        d = reduce_data(name)
        assert (np.diff(d["qcls"]) < 0).any()                            # `order` is no identity
    for c in REDUCE_CASES:
        d = reduce_data(c["name"])
        firsts = {int(p[0]) > 1 for p in d["pos"] if len(p)}
        assert firsts == {True, False}, c["name"]
        if c["name"] not in ("ap-stride", "sum-stride"):
            assert any(len(p) and p[-1] == POS_MAX for p in d["pos"]), c["name"]
            assert any(len(p) > 1 and (p == np.arange(1, len(p) + 1)).all() for p in d["pos"]), c["name"]


def test_reduce_bins_reach_every_path():
    pairs = set(reduce_pairs())
    assert pairs >= {(r, b) for r in BIN_RS for b in BIN_BS} | {(3, RP_MAX_BINS), (1000, RP_MAX_BINS)}
    differ = [(r, b) for r, b in sorted(pairs) if b <= 1000 and any(py_bin(j, r, b) != j * b // r for j in range(1, r + 1))]
    assert len(differ) >= 3 and {(100, 100), (200, 100), (1000, 100)} <= set(differ), differ
    assert py_bin(29, 100, 100) == 28 and py_bin(58, 200, 100) == 28 and py_bin(290, 1000, 100) == 28
    assert max(bin_hits(1000, 7).values()) > 2 * WAVE and min(bin_hits(1000, 7).values()) >= 1      # 142 hits: a third trip of the wave loop
    assert 0 not in bin_hits(5, 10) and 0 in bin_hits(100, 10)            # a miss alone makes bin 0 / a miss and hits share it
    assert len(bin_hits(7, 100)) == 7 < 101                               # B > R: bins no query has
    c = REDUCE_BY_NAME["bins-1000"]
    assert len(c["R"]) == 40 and bin_grid(40, 1000)[1] and 0 in c["R"]
    assert max(len(cc["R"]) * (max(cc["B"]) + 1) for cc in REDUCE_CASES if cc["name"] not in ("bins-1000", "bins-2^20")) <= BIN_GRID_CAP * RP_WAVES
    assert bin_grid(2, RP_MAX_BINS)[1]
    d = reduce_data("bins-10")
    first_miss_r5 = [p for cl, p in zip(d["qcls"].tolist(), d["pos"]) if REDUCE_BY_NAME["bins-10"]["R"][cl] == 5 and p[0] > 1]
    assert first_miss_r5, "a first-position miss in a class whose bin 0 holds no hit"


# ------------------------------------------------------------------ CPU tests: the reduce reference against the project's statement

def _random_problem(seed, C=6, N=70, Q=40):
    rng = np.random.default_rng(seed)
    glabels = rng.integers(0, C, size=N)
    glabels[glabels == C - 1] = 0
    glabels[3] = C - 1                                                    # a class of one gallery item
    qsel = rng.permutation(N)[:Q]
    qsel[0] = 3                                                           # ... which is a query: R = 0
    ranking = np.stack([rng.permutation(N) for _ in range(Q)])
    return ranking, glabels[qsel], glabels, qsel.astype(np.int32)


def _reference_on_problem(ranking, qlabels, glabels, qidx, bins, rows):
    """The problem through positions_reference and reduce_reference in tiles of `rows` queries -> the accumulators."""
    C = int(glabels.max()) + 1
    counts = np.bincount(glabels, minlength=C)
    r_cls = counts - 1                                                    # every query is a gallery item here
    class_off = np.concatenate([[0], np.cumsum(r_cls)]).astype(np.int64)
    Q = len(ranking)
    ap = np.zeros(Q)
    ps, fm = np.zeros(int(class_off[-1])), np.zeros(C, dtype=np.int64)
    bs, bc = np.zeros((C, bins + 1)), np.zeros((C, bins + 1), dtype=np.int64)
    calls = []
    for q0 in range(0, Q, rows):
        qc = qlabels[q0:q0 + rows].astype(np.int32)
        hit_off = np.concatenate([[0], np.cumsum(r_cls[qc])]).astype(np.int64)
        hit_pos = positions_reference(ranking[q0:q0 + rows], glabels.astype(np.int32), qc, qidx[q0:q0 + rows], hit_off)
        order = np.argsort(qc, kind="stable").astype(np.int32)
        class_start = np.concatenate([[0], np.cumsum(np.bincount(qc, minlength=C))]).astype(np.int32)
        calls.append((q0, hit_pos, hit_off, order, class_start))
        exact = reduce_reference(hit_pos, hit_off, order, class_start, class_off, bins, ps, fm, bs, bc)
        ap[q0:q0 + rows] = [float(x) for x in exact]
    return dict(ap=ap, ps=ps, fm=fm, bs=bs, bc=bc, r_cls=r_cls, class_off=class_off, calls=calls,
                nq_cls=np.bincount(qlabels, minlength=C))


@pytest.mark.parametrize("bins", [0, 7, 100])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reduce_reference_is_the_projects_statement(seed, bins):
    """reduce_reference -> recall_precision._merge_levels == recall_precision_host_gallery (levels bit-equal, means and AP to 1e-12),
    whatever the tiling; and bit for bit the stand-in of tests/test_recprec_host.py."""
    import torch
    from recall_precision import _merge_levels, recall_precision_host_gallery
    from test_recprec_host import _cpu_kernels
    ranking, qlabels, glabels, qidx = _random_problem(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        levels, means, mAP, aps = recall_precision_host_gallery(ranking, qlabels.tolist(), glabels.tolist(), qidx, bins or None)
    t = torch.from_numpy
    results = [_reference_on_problem(ranking, qlabels, glabels, qidx, bins, rows) for rows in (len(ranking), 13, 1)]
    for r in results:
        got = _merge_levels(r["ap"], r["r_cls"], r["nq_cls"], r["class_off"], bins, t(r["ps"]), t(r["fm"]), t(r["bs"]) if bins else None,
                            t(r["bc"]) if bins else None)
        assert np.array_equal(got[0], levels)
        assert np.abs(got[1] - means).max() <= 1e-12 and abs(got[2] - mAP) <= 1e-12 and np.abs(got[3] - aps).max() <= 1e-12
        for k in ("ps", "fm", "bs", "bc"):                               # the tiling changes no bit
            assert np.array_equal(r[k].view(np.int64), results[0][k].view(np.int64)), k
    r = results[1]
    standin = _cpu_kernels()["recall_precision_reduce"]
    C = len(r["r_cls"])
    ps, fm = torch.zeros(len(r["ps"]), dtype=torch.float64), torch.zeros(C, dtype=torch.int64)
    bs, bc = torch.zeros((C, bins + 1), dtype=torch.float64), torch.zeros((C, bins + 1), dtype=torch.int64)
    ap = torch.zeros(len(ranking), dtype=torch.float64)
    for q0, hit_pos, hit_off, order, class_start in r["calls"]:
        standin(t(hit_pos), t(hit_off), t(order), t(class_start), t(r["class_off"]), bins, ap[q0:q0 + len(order)], ps, fm, bs, bc)
    assert np.array_equal(ps.numpy().view(np.int64), r["ps"].view(np.int64)) and np.array_equal(fm.numpy(), r["fm"])
    if bins:
        assert np.array_equal(bs.numpy().view(np.int64), r["bs"].view(np.int64)) and np.array_equal(bc.numpy(), r["bc"])
    assert np.abs(ap.numpy() - r["ap"]).max() <= 1e-14          # (R + 2) 2^-53 with R < 70


def test_exact_ap():
    assert exact_ap(np.array([], dtype=np.int32)) == 0
    assert exact_ap(np.array([1, 2, 3])) == 1 and exact_ap(np.array([2, 4, 6, 8])) == fractions.Fraction(1, 2)
    assert exact_ap(np.array([2, 3, POS_MAX])) == (fractions.Fraction(1, 2) + fractions.Fraction(2, 3) + fractions.Fraction(3, POS_MAX)) / 3
    assert exact_ap(np.arange(1, BIG_R + 1) * 2) == fractions.Fraction(1, 2)


# ------------------------------------------------------------------ CPU tests: the counting table reaches its paths

def test_counting_table_reaches_every_path():
    assert [count_geometry(len(COUNT_R), n, max(COUNT_R))[1] for n in COUNT_COLS] == [1, 1, 2, 3]
    assert cut_vector_steps(16383, RC_CHUNK) == [0] and cut_vector_steps(16384, RC_CHUNK) == [] and cut_vector_steps(16385, RC_CHUNK) == [1]
    assert cut_vector_steps(32773, RC_CHUNK) == [2]
    assert COUNT_SELF[32773][0] >= RC_CHUNK and COUNT_SELF[16385][0] == RC_CHUNK            # the query's own column in the second chunk
    pd = count_gallery()
    u = pd.view(np.uint32)
    for val in (NAN_POS, NAN_NEG, 0x80000000, 0, 0x7F800000):
        assert (u == val).sum() > 100
    lo, hi = COUNT_SAME
    assert hi - lo == 40 and lo < RC_CHUNK < hi and (pd[:, lo:hi] == pd[:, lo:lo + 1]).all()
    for n in COUNT_COLS:
        d = count_case(n)
        assert np.diff(d["hit_off"]).tolist() == list(COUNT_R)
        for i in np.flatnonzero(np.diff(d["hit_off"]) >= 300):
            rel = d["rel_i"][d["hit_off"][i]:d["hit_off"][i + 1]]
            assert d["qidx"][i] not in rel
            assert {c for c in (lo, RC_CHUNK - 1, RC_CHUNK) if c < n and c != d["qidx"][i]} <= set(rel.tolist())     # ties by index across the edge
            assert {int(x) for x in pd[i, rel].view(np.uint32)} >= {NAN_POS, NAN_NEG, 0x80000000, 0, 0x7F800000}
        assert (d["want"] != d["prior"]).any()
    assert COUNT_SLABS[0] == 0 and COUNT_SLABS[-1] == COUNT_N and all(s % 2 for s in COUNT_SLABS[1:])
    vec = set()
    for (a, b), (pad, off) in zip(zip(COUNT_SLABS, COUNT_SLABS[1:]), SLAB_LAYOUTS):
        vec.add(slab_vec_ok((b - a + 3) // 4 * 4 + pad, off))
    assert vec == {True, False}
    assert any(b - a > RC_CHUNK for a, b in zip(COUNT_SLABS, COUNT_SLABS[1:]))              # a slab of two chunks at a non-zero offset


def test_key_lists_reach_both_sides_of_every_size():
    assert set(KEY_RS) == {1, 255, 256, 257, 5460, 5461} and KEY_COLS > max(KEY_RS)
    in_lds = {(R, m): R <= count_geometry(3, KEY_COLS, m)[2] for R in KEY_RS for m in key_max_rels(R)}
    assert in_lds[(5460, 0)] and in_lds[(5460, 5460)] and in_lds[(5460, 5459)] and in_lds[(5460, 10 ** 6)]      # exactly RC_MAX_KEYS keys
    assert not any(in_lds[(5461, m)] for m in key_max_rels(5461))                                               # one more: global memory
    assert not in_lds[(255, 254)] and in_lds[(256, 255)] and not in_lds[(257, 256)] and in_lds[(257, 257)]          # (max_rel + 1) / 2 * 2
    assert count_geometry(3, KEY_COLS, 1)[2] == 2 and count_geometry(3, KEY_COLS, 0)[2] == RC_MAX_KEYS
    assert in_lds[(1, 1)] and in_lds[(1, 0)]
    for R in KEY_RS:
        # the other key list of the call (3 keys) is in LDS whenever R's fits, and with max_rel = R - 1 = 0 sizes LDS for RC_MAX_KEYS
        assert np.diff(key_case(R)["hit_off"]).tolist() == [R, 0, 3]


def test_scan_table_reaches_every_path():
    small, big = scan_case(False), scan_case(True)
    assert set(np.diff(small["hit_off"]).tolist()) >= set(SCAN_RS) | {0}
    assert {-(-r // RC_THREADS) for r in SCAN_RS} == {1, 2, 3, 5}                             # steps of a query: the parity carries over
    assert len(big["hit_off"]) - 1 == SCAN_BIG_Q and scan_grid(SCAN_BIG_Q)[1] and set(np.diff(big["hit_off"]).tolist()) == {0, 1, 2, 3}
    assert small["want"][0] == small["cnt"][0] and small["want"].dtype == np.int32
