"""The hierarchical-precision kernels (csrc/hprec.hip: ``se_hierarchical_precision``, ``se_hierarchical_precision_r16``,
``se_hprec_reciprocal_curves``) through every instantiation and data-dependent path: the host half.

``hprec_kernel<CLSW, RT>`` is one body over: the class source CLSW (0 global gather, 1 byte table, 2 16-bit table in LDS), the rank
element type RT (int32 / uint16), NQ = 1 or 2 queries per pass, three chunk forms (general / interior FAST / TAIL), the iota short cut
of the cut-offs, the class-ordered visit with per-XCD tickets or the static visit, and three ways of learning the query's position
(flag 0: searched, flag 1: rank 0, flag 2: absent).  This file restates those choices in plain Python, each next to the lines it
mirrors, holds the case table ``CASES`` that tests/test_gpu_hprec_matrix.py runs on the device, and asserts on the CPU -- from the
restatements and each case's own data alone -- that the table reaches every path.  A case that leaves the table, or drifts to another
path, fails here and not silently on the device.

The oracle of the GPU file is ``_hprec_standin`` (tests/test_dp_gloo.py); it is tied here to ``ClassHierarchy.hierarchical_precision``
(the host mirror that tests/test_host.py holds against the reference's golden values) on the edge cases the table uses.

Recorded while restating (behaviour, not defects):
  * An absent query never takes the FAST or the TAIL form: both ask for ``base > qpos`` and an absent query has ``qpos = L``.
  * A clipped AHP whose last end point ``alen - 1`` is 2047, 2048 or 2049 leaves no FAST chunk at all (chunk 0 holds the query or
    the cut-offs' first ranks and is always general; chunk 1 would need ``2048 + 2046 < alen - 1``).  With ``alen - 1`` in
    {4095, 4096, 4097} chunk 1 is FAST and the chunk that owns the end point is general; 4094 (the last rank of chunk 1's last
    lane) is the largest end point that keeps chunk 1 general.  ``test_fast_settings`` pins all of them.
  * Fewer than 8 queries give ``ceil(Q / 8) = 1`` entry per XCD segment: every draw is a single, whatever the flags.
"""
import functools
import itertools
import zlib

import numpy as np
import pytest

# ------------------------------------------------------------------ constants of hprec.hip:37-44 and rank_stream.h:94

HP_THREADS, HP_ITEMS, HP_WAVES, HP_MAX_KS, HP_WS_HEAD, HP_ORDER_THREADS = 256, 8, 4, 512, 16, 1024
HP_CHUNK = HP_THREADS * HP_ITEMS
CLASS_TABLE_LDS_CAP = 160 * 1024
XCDS = 8
GENERAL, FAST, TAIL = "general", "fast", "tail"
INT32, UINT16 = "int32", "uint16"
ESIZE = {INT32: 4, UINT16: 2}


# ------------------------------------------------------------------ restatements

def fixed_lds(C, nk):
    """hprec.hip:488 -- the kernel's own LDS: [C] double2, the scan / finish / end-point doubles, 2 nk + 12 ints."""
    return C * 16 + (2 * 2 * HP_WAVES * 3 + 2 * HP_WAVES * 3 + 8) * 8 + (2 * nk + 12) * 4


def clsw(list_len, q, gallery, C, nk):
    """choose_class_table (rank_stream.h:96-103) with hp_run's `fixed` (hprec.hip:488-490): -> (CLSW, dynamic LDS bytes), or None
    where hp_run refuses (SE_ERR_UNSUPPORTED: the similarity rows alone exceed the cap)."""
    fixed = fixed_lds(C, nk)
    if fixed > CLASS_TABLE_LDS_CAP:
        return None
    tab8, tab16 = (gallery + 15) // 16 * 16, (gallery * 2 + 15) // 16 * 16
    if list_len * min(q, 4096) < 8 * gallery:
        return 0, fixed
    if C <= 256 and fixed + tab8 <= CLASS_TABLE_LDS_CAP:
        return 1, fixed + tab8
    if C <= 65536 and fixed + tab16 <= CLASS_TABLE_LDS_CAP:
        return 2, fixed + tab16
    return 0, fixed


def vec_ok(ldr, esize, base_offset_bytes):
    """ranks_vec_ok<RT, 8> (rank_stream.h:85-90): 8 ranks are 32 / 16 bytes, the load is 16 bytes in both types."""
    nbytes = min(HP_ITEMS * esize, 16)
    return (ldr * esize) % nbytes == 0 and base_offset_bytes % nbytes == 0


def order_flag(first_rank, qidx):
    """hprec_order_kernel (hprec.hip:105-108).  qidx None: no query ids at all."""
    self_ = -1 if qidx is None else int(qidx)
    return 2 if self_ < 0 else (1 if int(first_rank) == self_ else 0)


def certain_visits(qcls, flags):
    """The draw (hprec.hip:167-208, 435): entries sorted by class, eight segments of ceil(Q / 8), tickets of two aligned at each
    segment's start; a pair iff both entries share class and the same non-zero flag.  The order inside a class is whatever the order
    kernel's atomicAdd made it, so -> the multiset {(kind, flag): count} of visits that happen under ANY within-class order:
    a class whose flags are uniform contributes all of its draws; a class all of whose slots are lone or cross-class draws
    contributes a single per query."""
    qcls, flags = np.asarray(qcls), np.asarray(flags)
    Q = len(qcls)
    seg_len = (Q + XCDS - 1) // XCDS
    at = np.sort(qcls, kind="stable")                          # class of every slot of the order
    paired = np.zeros(Q, dtype=bool)                           # slot is one half of a same-class draw
    for s in range(XCDS):
        lo, hi = s * seg_len, min((s + 1) * seg_len, Q)
        for p in range(lo, hi, 2):
            if p + 1 < hi and at[p] == at[p + 1]:
                paired[p] = paired[p + 1] = True
    out = {}
    for c in np.unique(qcls):
        fl = flags[qcls == c]
        slots = paired[at == c]
        if not slots.any():                                    # every query of the class is drawn alone or next to another class
            for f in fl:
                out[("single", int(f))] = out.get(("single", int(f)), 0) + 1
        elif len(set(fl.tolist())) == 1:
            f = int(fl[0])
            n_pair_slots = int(slots.sum())
            if f != 0:
                out[("pair", f)] = out.get(("pair", f), 0) + n_pair_slots // 2
                if len(fl) - n_pair_slots:
                    out[("single", f)] = out.get(("single", f), 0) + len(fl) - n_pair_slots
            else:
                out[("single", 0)] = out.get(("single", 0), 0) + len(fl)
    return out


def query_state(L, qpos, ks, ahp_len, want_ap):
    """hprec.hip:158, 252-259 -> (eff_len, alen, need, last_pos, kmax).  qpos = L: the query is not in its list."""
    kmax = max(ks) if len(ks) else 0
    eff_len = L - 1 if qpos < L else L
    alen = (min(ahp_len, eff_len) if ahp_len > 0 else eff_len)
    need = kmax
    if ahp_len >= 0:
        need = max(alen, need)
    if want_ap:
        need = eff_len
    last_pos = need + 1 if need < L else L
    return eff_len, alen, need, last_pos, kmax


def form(base, L, qpos, ks, ahp_len, want_ap, vec):
    """The form of the chunk at `base` (hprec.hip:286, 401-405)."""
    eff_len, alen, need, last_pos, kmax = query_state(L, qpos, ks, ahp_len, want_ap)
    cuts = len(ks) > 0 and base <= kmax
    interior = bool(vec) and ahp_len >= 0 and not cuts and base > qpos and base + HP_CHUNK <= last_pos and base + HP_CHUNK - 2 < alen - 1
    tail = ahp_len == 0 and not cuts and base > qpos
    return FAST if interior else (TAIL if tail else GENERAL)


def forms(L, qpos, ks, ahp_len, want_ap, vec):
    """Every chunk the kernel walks for one query (hprec.hip:408: while base < last_pos)."""
    last_pos = query_state(L, qpos, ks, ahp_len, want_ap)[3]
    return [form(b, L, qpos, ks, ahp_len, want_ap, vec) for b in range(0, last_pos, HP_CHUNK)]


def ks_iota(ks):
    """hprec.hip:161-163: the sorted cut-offs are 1 .. K and already in that order."""
    return list(ks) == list(range(1, len(ks) + 1))


def hp_slot(i):
    """hp_slot (hprec.hip:57-61); works on arrays."""
    k, p = i // HP_CHUNK, i % HP_CHUNK
    return (k * HP_ITEMS + p % HP_ITEMS) * HP_THREADS + p // HP_ITEMS


def curve_len(list_len):
    """se_hprec_curve_len (hprec.hip:452-455)."""
    return 0 if list_len <= 0 else (list_len + HP_CHUNK - 1) // HP_CHUNK * HP_CHUNK


def order_classes_per_thread(C):
    """hprec_order_kernel (hprec.hip:92): `per`."""
    return (C + HP_ORDER_THREADS - 1) // HP_ORDER_THREADS


# ------------------------------------------------------------------ the case table

ABS, OUT, LAST = "absent:-1", "absent:index", "last"     # position of a query: an int, LAST (L - 1), qidx = -1, or qidx >= 0 missing from the list
BOTH = (INT32, UINT16)
PAD = 5                                                   # ldo = 2 nk + 3 + PAD


def p16(classes, c_pos=(1, 1000, 2047), f_pos=(2048, 2049, LAST)):
    """16 queries in six classes A < B < C < D < E < F with uniform flags per class: A x 4 at rank 0 (flag 1), B x 4 absent (flag 2),
    C x 3 searched, D x 1 at rank 0, E x 1 absent, F x 3 searched -- interleaved, so the counting sort has work to do.  In class order
    the slots are A 0-3, B 4-7, C 8-10, D 11, E 12, F 13-15; with segments of two: two certain flag-1 pairs, two certain flag-2
    pairs, and singles of every flag.  -> (qcls, pos)."""
    A, B, C_, D, E, F = classes
    blocks = [A, B, C_, D, A, B, C_, E, A, B, C_, F, A, B, F, F]
    it = {A: iter((0,) * 4), B: iter((ABS,) * 4), C_: iter(c_pos), D: iter((0,)), E: iter((ABS,)), F: iter(f_pos)}
    if len(set(classes)) == 1:                            # one class: the positions in block order
        seq = iter([0, ABS, c_pos[0], 0, 0, ABS, c_pos[1], ABS, 0, ABS, c_pos[2], f_pos[0], 0, ABS, f_pos[1], f_pos[2]])
        return tuple(blocks), tuple(next(seq) for _ in blocks)
    return tuple(blocks), tuple(next(it[b]) for b in blocks)


def case(name, L, gallery, Q, C, qcls, pos, ks, calls, rt=BOTH, ldr=None, off=0, qidx="array", class_order="both", rcp_len=None,
         ldo_pad=0, norel=None):
    return dict(name=name, L=L, gallery=gallery, Q=Q, C=C, rt=tuple(rt), ldr=L if ldr is None else ldr, off=off, qidx=qidx,
                qcls=tuple(qcls), pos=tuple(pos), ks=tuple(ks), calls=tuple(calls), class_order=class_order,
                rcp_len=L if rcp_len is None else rcp_len, ldo_pad=ldo_pad, norel=norel)


C23 = (2, 5, 7, 11, 13, 17)
C300 = (2, 50, 120, 200, 260, 299)                        # classes above 255: what a byte table could not hold
C1100 = (3, 400, 1023, 1024, 1025, 1099)                  # both classes of the order kernel's last threads
Q3000 = 3000

CASES = [
    # --- three-chunk lists, byte table.  L = 6148: int32 rows are 24,592 bytes (vec_ok), uint16 rows 12,296 bytes (not): the same
    #     rankings run FAST in one type and TAIL / general in the other.  Cut-offs at 2048 and 2049 (chunk 1 general, chunk 2 FAST);
    #     curves built for 8,197 positions.
    case("byte-6148", 6148, 6148, 16, 23, *p16(C23), ks=(300, 1, 2048, 2049), calls=((0, 1), (6000, 0), (7000, 1), (-1, 0)),
         rcp_len=8197),
    # --- five chunks, rows of 8,197 on a pitch of 8,200 (both types vec_ok, the padding holds indices outside the gallery), ldo
    #     padded, cut-offs confined to the first chunk, unsorted with a duplicate: every AHP end point at a chunk edge
    case("byte-8197-pitch", 8197, 8197, 16, 23, *p16(C23), ks=(250, 1, 2, 10, 2047, 10),
         calls=((0, 1), (-1, 1), (-1, 0), (50, 0), (2047, 0), (2048, 0), (2049, 1), (2050, 0), (4095, 0), (4096, 0), (4097, 1), (4098, 0),
                (9000, 0)),
         ldr=8200, ldo_pad=PAD),
    # --- 16-bit table: C = 300 > 256, L Q >= 8 gallery
    #     the largest cut-off is 2048 itself: behind the query that is position 2048, the first rank of chunk 1 (`base <= kmax`)
    case("w16-6151", 6151, 6151, 16, 300, *p16(C300), ks=(100, 1, 2048), calls=((0, 1), (4097, 0), (7000, 0), (-1, 1)), ldr=6152,
         ldo_pad=PAD),
    # --- gather: L Q = 98,368 < 8 x 40,000; the rankings are subsets of the gallery: a query index that is missing from its list,
    #     and a class (17: the searched queries at 2048, 2049 and L - 1) none of whose other items is in the list
    case("gather-40000", 6148, 40000, 16, 23, *p16(C23, c_pos=(1, 1000, OUT), f_pos=(2048, 2049, LAST)), ks=(3, 1, 2047, 3),
         calls=((0, 1), (4096, 1), (9999, 0), (-1, 0)), ldr=6152, norel=17),
    # --- gather by Q = 5 < 8: every draw a single; a base 16 bytes into the buffer for int32 (vec_ok) and 8 for uint16 (not)
    case("gather-q5-6144", 6144, 6144, 5, 23, (4, 4, 9, 9, 9), (0, 1000, ABS, 2049, LAST), ks=(1, 2, 3),
         calls=((0, 1), (4098, 0), (-1, 1)), off=4),
    # --- no cut-offs at all: out rows of 3 (+ padding), ks NULL
    case("nk0-6144", 6144, 6144, 16, 23, *p16(C23), ks=(), calls=((0, 1), (0, 0), (3000, 0), (-1, 1)), ldo_pad=PAD),
    # --- no query ids (qidx NULL): all pairs of flag 2, k == eff_len == L for absent queries, cut-offs in every chunk
    case("null-qidx-6144", 6144, 6144, 16, 23, (3, 8, 3, 8, 3, 8, 3, 8, 21, 0, 21, 0, 21, 0, 21, 0), (ABS,) * 16,
         ks=(6144, 1, 2048, 2049), calls=((0, 1), (100, 0), (-1, 0)), qidx="null"),
    # --- the iota short cut: 1 .. K for K = 1, 300 (two threads' worth of ranks) and 512 (HP_MAX_KS), lists around one chunk
    case("iota1-2047", 2047, 2047, 16, 23, *p16(C23, c_pos=(1, 1000, 2045), f_pos=(5, 700, LAST)), ks=(1,),
         calls=((0, 1), (100, 0), (-1, 0))),
    case("iota300-2048", 2048, 2048, 16, 23, *p16(C23, c_pos=(1, 150, 299), f_pos=(300, 301, LAST)), ks=range(1, 301),
         calls=((0, 1), (100, 0), (-1, 0))),
    case("iota512-2049", 2049, 2049, 16, 23, *p16(C23, c_pos=(1, 511, 512), f_pos=(2047, 2048, 513)), ks=range(1, 513),
         calls=((0, 1), (2049, 0), (-1, 1))),
    # --- one class: everything is relevant; k == eff_len for present queries (299) next to absent ones
    case("C1-300", 300, 300, 16, 1, *p16((0,) * 6, c_pos=(1, 100, 298), f_pos=(150, 2, LAST)), ks=(299, 1, 150),
         calls=((0, 1), (299, 0), (-1, 0))),
    # --- 1,100 classes: the order kernel takes two classes per thread, almost all of them without a query; 16-bit table
    case("C1100-300", 300, 300, 48, 1100, p16(C1100)[0] * 3, p16(C1100, c_pos=(1, 100, 298), f_pos=(150, 2, LAST))[1] * 3, ks=(10, 1, 200),
         calls=((0, 1), (50, 0))),
    # --- the shortest lists
    case("L1", 1, 1, 9, 23, (0,) * 9, (ABS,) * 9, ks=(1,), calls=((0, 1), (1, 0), (5, 0), (-1, 0))),
    case("L2", 2, 2, 9, 23, (0, 1, 0, 1, 0, 1, 0, 1, 0), (0, 1, ABS, 0, 1, ABS, LAST, 0, ABS), ks=(1,), calls=((0, 1), (1, 0), (-1, 1))),
    # --- 3,000 queries on lists of 37: every resident workgroup draws several times and ends by walking the other XCDs' segments
    case("q3000-37", 37, 37, Q3000, 23, tuple((u * 7 + u // 23) % 23 for u in range(Q3000)),
         tuple((0, ABS, (5 * u) % 37, LAST)[u % 4] for u in range(Q3000)), ks=(36, 1, 10), calls=((0, 1), (20, 0))),
    # --- curves built for 5,000 positions, lists of 300
    case("curves5000-300", 300, 300, 16, 23, *p16(C23, c_pos=(1, 100, 298), f_pos=(150, 2, LAST)), ks=(1, 10, 50), calls=((0, 1), (50, 0)),
         rcp_len=5000),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}

# se_hprec_reciprocal_curves directly: (classes, len); ldb = len + 3 with NaN in the padding.  264,000 positions are 1,032 blocks of 256:
# past the 1,024-block cap, where the grid-stride loop runs.
RCP_CASES = ((3, 1), (3, 2047), (3, 2048), (3, 2049), (3, 5000), (2, 264000))
RCP_GRID_CAP = 1024


# ------------------------------------------------------------------ case data, derived quantities, the oracle

def tables(rng, C):
    """test_gpu_dropin.py:145-146: similarities in [0.1, 0.9], symmetric, unit diagonal."""
    t = rng.random((C, C)) * 0.8 + 0.1
    t = (t + t.T) / 2
    np.fill_diagonal(t, 1.0)
    return t


def best_curves(tab, cls, C, length):
    """test_gpu_dropin.py:147-152: per query class the descending-sorted similarities of the whole gallery, cumulated.  Curves for
    more positions than the gallery has go on rising by 0.5 a position (read by nobody: the lists end before)."""
    counts = np.bincount(cls, minlength=C)
    rows = []
    for c in range(C):
        order = np.argsort(-tab[c], kind="stable")
        rows.append(np.cumsum(np.repeat(tab[c][order], counts[order])))
    best = np.stack(rows)
    if length > best.shape[1]:
        ext = best[:, -1:] + 0.5 * np.arange(1, length - best.shape[1] + 1)[None, :]
        best = np.concatenate([best, ext], axis=1)
    return np.ascontiguousarray(best)


@functools.lru_cache(maxsize=None)                          # (all cases together hold some 100 MB)
def case_data(name):
    """-> dict: rk [Q, L] int32, cls [gallery], qcls [Q], qidx [Q] (or None), tab_w / tab_l [C, C], best_w / best_l [C, >= rcp_len],
    ks [nk], qpos [Q] (L: absent), flags [Q]."""
    c = CASE_BY_NAME[name]
    L, G, Q, C = c["L"], c["gallery"], c["Q"], c["C"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cls = (rng.permutation(np.arange(G) % C) if G >= C else rng.integers(0, C, size=G)).astype(np.int32)
    qcls = np.asarray(c["qcls"], dtype=np.int32)
    own = rng.permutation(G)[np.arange(Q) % G]                  # the gallery index of every query
    if Q <= G:
        cls[own] = qcls                                         # a query is an item of its own class (and its class has an item)
    else:
        qcls = cls[own].copy() if G < C else qcls
    rk = np.empty((Q, L), dtype=np.int32)
    qidx = np.empty(Q, dtype=np.int32)
    for u in range(Q):
        p = c["pos"][u]
        p = L - 1 if p == LAST else p
        keep = np.ones(G, dtype=bool)
        if c["norel"] is not None and qcls[u] == c["norel"]:
            keep &= cls != qcls[u]                              # no item of the query's class in its list
        if p == ABS:
            qidx[u] = -1
            cand = np.flatnonzero(keep)
            rk[u] = cand[rng.permutation(len(cand))[:L]]
            continue
        keep[own[u]] = False
        cand = np.flatnonzero(keep)
        qidx[u] = own[u]
        if p == OUT:
            rk[u] = cand[rng.permutation(len(cand))[:L]]
        else:
            rest = cand[rng.permutation(len(cand))[:L - 1]]
            rk[u] = np.concatenate([rest[:p], [own[u]], rest[p:]])
    tab_w, tab_l = tables(rng, C), tables(rng, C)
    width = max(c["rcp_len"], G)
    best_w, best_l = best_curves(tab_w, cls, C, width), best_curves(tab_l, cls, C, width)
    null = c["qidx"] == "null"
    hit = rk == qidx[:, None]
    qpos = np.where(hit.any(axis=1), hit.argmax(axis=1), L).astype(np.int64)
    flags = np.array([order_flag(rk[u, 0], None if null else qidx[u]) for u in range(Q)])
    return dict(rk=rk, cls=cls, qcls=qcls, qidx=None if null else qidx, tab_w=tab_w, tab_l=tab_l, best_w=best_w, best_l=best_l,
                ks=np.asarray(c["ks"], dtype=np.int32), qpos=qpos, flags=flags)


@functools.lru_cache(maxsize=None)
def case_oracle(name, ahp_len, want_ap):
    """_hprec_standin on the case's rankings: f64 [Q, 2 nk + 3] (columns the call does not produce are 0)."""
    import torch
    from test_dp_gloo import _hprec_standin
    c, d = CASE_BY_NAME[name], case_data(name)
    qidx = d["qidx"] if d["qidx"] is not None else np.full(c["Q"], -1, dtype=np.int32)
    L = c["L"]
    args = [torch.from_numpy(np.ascontiguousarray(a)) for a in (d["rk"], d["cls"], d["qcls"], qidx, d["tab_w"], d["tab_l"],
                                                                 d["best_w"][:, :L], d["best_l"][:, :L], d["ks"])]
    return _hprec_standin(*args, ahp_len=ahp_len, want_ap=bool(want_ap)).numpy()


def case_clsw(c):
    return clsw(c["L"], c["Q"], c["gallery"], c["C"], len(c["ks"]))[0]


def case_vec_ok(c, rt):
    return vec_ok(c["ldr"], ESIZE[rt], c["off"] * ESIZE[rt])


def case_forms(c, rt):
    """{(query, call): [form of every chunk]}"""
    return _case_forms(c["name"], rt)


@functools.lru_cache(maxsize=None)
def _case_forms(name, rt):
    c, d = CASE_BY_NAME[name], case_data(name)
    v = case_vec_ok(c, rt)
    return {(u, call): forms(c["L"], int(d["qpos"][u]), c["ks"], call[0], call[1], v) for u in range(c["Q"]) for call in c["calls"]}


def visits(c):
    """The visit kinds a case certainly takes: {"static"} when it runs without the workspace, and certain_visits with it."""
    d = case_data(c["name"])
    out = set()
    if c["class_order"] in ("off", "both"):
        out.add("static")
    if c["class_order"] in ("on", "both"):
        out |= {"flag-%d %s" % (f, "certain pair" if kind == "pair" else "single") for (kind, f), n in certain_visits(d["qcls"], d["flags"]).items() if n}
    return out


VISITS = {"static", "flag-0 single", "flag-1 single", "flag-1 certain pair", "flag-2 single", "flag-2 certain pair"}


# ------------------------------------------------------------------ CPU: the restatements

def test_restatements_on_known_values():
    assert fixed_lds(23, 8) == 23 * 16 + 80 * 8 + 28 * 4
    # the gather by too little work, the byte table, the 16-bit table by class count, the gather by size
    assert clsw(6148, 16, 40000, 23, 4)[0] == 0 and 6148 * 16 == 98368 < 8 * 40000
    assert clsw(6144, 5, 6144, 23, 3)[0] == 0 and clsw(6144, 8, 6144, 23, 3)[0] == 1
    assert clsw(6151, 16, 6151, 300, 3) == (2, fixed_lds(300, 3) + (6151 * 2 + 15) // 16 * 16)
    assert clsw(5000, 40, 5000, 256, 8)[0] == 1 and clsw(5000, 40, 5000, 257, 8)[0] == 2
    assert clsw(170001, 5, 170001, 23, 8)[0] == 0 and clsw(90000, 4096, 90000, 700, 8)[0] == 0
    # the cap on the similarity rows: 10,300 classes are 164,800 bytes of double2
    assert clsw(8, 8, 8, 10300, 0) is None and clsw(8, 8, 8, 10000, 0) is not None and 10300 * 16 > CLASS_TABLE_LDS_CAP
    # 16-byte loads: L = 6148 gives 24,592-byte int32 rows and 12,296-byte uint16 rows
    assert vec_ok(6148, 4, 0) and not vec_ok(6148, 2, 0) and 6148 * 4 == 24592 and 6148 * 2 == 12296
    assert vec_ok(6152, 2, 0) and vec_ok(6144, 4, 16) and not vec_ok(6144, 2, 8) and not vec_ok(6144, 4, 4) and not vec_ok(3001, 4, 0)
    assert [order_flag(7, None), order_flag(7, -1), order_flag(7, 7), order_flag(7, 8)] == [2, 2, 1, 0]
    assert [hp_slot(i) for i in (0, 1, 7, 8, 2047, 2048, 2049, 4095)] == [0, 256, 1792, 1, 2047, 2048, 2304, 4095]
    for n in (1, 2047, 2048, 2049, 5000):
        i = np.arange(curve_len(n))
        assert sorted(hp_slot(i).tolist()) == i.tolist()            # a permutation of the padded row
    assert [curve_len(n) for n in (0, 1, 2048, 2049, 264000)] == [0, 2048, 2048, 4096, 264192]
    assert [order_classes_per_thread(C) for C in (1, 1024, 1025, 1100)] == [1, 1, 2, 2]
    assert ks_iota([1, 2, 3]) and ks_iota([1]) and not ks_iota([1, 3]) and not ks_iota([2, 1]) and ks_iota([])


def test_query_state_and_forms_on_known_values():
    # present at rank 0, whole list, AP: chunks 1 and 2 interior, the list ends in the fourth
    assert forms(6148, 0, (1, 10), 0, 1, True) == [GENERAL, FAST, FAST, TAIL]
    assert forms(6148, 0, (1, 10), 0, 1, False) == [GENERAL, TAIL, TAIL, TAIL]
    assert forms(6144, 0, (1, 10), 0, 1, True) == [GENERAL, FAST, TAIL]        # the last chunk is full: its last rank is the end point
    # a cut-off at 2048 / 2049 makes chunk 1 general; the query at 2048 / 2049 too
    assert forms(6148, 0, (2048,), 0, 1, True) == [GENERAL, GENERAL, FAST, TAIL]
    assert forms(6148, 2048, (1,), 0, 1, True) == [GENERAL, GENERAL, FAST, TAIL] and forms(6148, 2047, (1,), 0, 1, True)[1] == FAST
    # absent: never FAST or TAIL
    assert set(forms(6148, 6148, (1,), 0, 1, True)) == {GENERAL} and len(forms(6148, 6148, (1,), 0, 1, True)) == 4
    # no AHP: general everywhere; P@k only: the chunks of the cut-offs
    assert forms(6148, 0, (1,), -1, 1, True) == [GENERAL] * 4 and forms(6148, 0, (1, 2049), -1, 0, True) == [GENERAL] * 2
    # clipped AHP: the chunk that owns alen - 1 is general
    assert query_state(8197, 0, (10,), 4096, 0) == (8196, 4096, 4096, 4097, 10)
    assert forms(8197, 0, (10,), 4096, 0, True) == [GENERAL, FAST, GENERAL]    # alen - 1 = 4095: effective rank 4095 is position 4096
    assert forms(8197, 0, (10,), 4095, 0, True) == [GENERAL, GENERAL]          # alen - 1 = 4094 = 2048 + 2046
    assert forms(8197, 0, (10,), 2050, 0, True) == [GENERAL, GENERAL]
    assert forms(8197, 0, (10,), 9000, 0, True) == [GENERAL, FAST, FAST, FAST, GENERAL]     # clamped to eff_len


def test_certain_visits_helper():
    qcls, pos = p16(C23)
    flags = [{0: 1, ABS: 2}.get(p, 0) for p in pos]
    assert certain_visits(qcls, flags) == {("pair", 1): 2, ("pair", 2): 2, ("single", 0): 6, ("single", 1): 1, ("single", 2): 1}
    # mixed flags inside a class that has a same-class draw: nothing is certain about it
    assert certain_visits([1, 1, 1, 1] * 4, [1, 2, 1, 2] * 4) == {}
    # fewer than 8 queries: segments of one, every draw a single whatever the flags
    assert certain_visits([4, 4, 4, 4, 4], [1, 2, 0, 1, 2]) == {("single", 1): 2, ("single", 2): 2, ("single", 0): 1}
    # a class of three in segments of two: slots 0, 1 pair, slot 2 is drawn with the next class
    assert certain_visits([0, 0, 0, 1] * 4, [2] * 16) == {("pair", 2): 8}
    assert certain_visits([0] * 3 + [1] * 13, [2] * 16) == {("pair", 2): 7, ("single", 2): 2}


# ------------------------------------------------------------------ CPU: the table reaches every path

def test_case_table_shape():
    assert len({c["name"] for c in CASES}) == len(CASES) == 16               # a row that leaves the table changes the count
    for c in CASES:
        d = case_data(c["name"])
        nk = len(c["ks"])
        assert len(c["qcls"]) == len(c["pos"]) == c["Q"] and c["ldr"] >= c["L"] and c["rcp_len"] >= c["L"] and nk <= HP_MAX_KS, c["name"]
        assert c["gallery"] >= c["L"] and (UINT16 not in c["rt"] or c["gallery"] <= 65535), c["name"]
        assert clsw(c["L"], c["Q"], c["gallery"], c["C"], nk) is not None and c["calls"], c["name"]
        assert c["class_order"] in ("on", "off", "both") and c["qidx"] in ("array", "null"), c["name"]
        # the declared position pattern is what the data holds
        want = np.array([c["L"] if p in (ABS, OUT) else (c["L"] - 1 if p == LAST else p) for p in c["pos"]])
        assert np.array_equal(d["qpos"], want), c["name"]
        assert all(k >= 1 for k in c["ks"]) and (not nk or max(c["ks"]) <= min(query_state(c["L"], int(q), c["ks"], -1, 0)[0] for q in d["qpos"])), c["name"]
        # the budget: three-chunk lists with a few queries, many queries only on short lists
        assert c["Q"] * c["L"] <= 140000 and c["Q"] * len(c["calls"]) <= 6000, c["name"]
        assert all(a >= -1 and ap in (0, 1) for a, ap in c["calls"]), c["name"]


def test_every_rt_and_class_source_runs_all_three_forms():
    have = {}
    for c in CASES:
        for rt in c["rt"]:
            for (u, call), fs in case_forms(c, rt).items():
                if {GENERAL, FAST, TAIL} <= set(fs):
                    have.setdefault((rt, case_clsw(c)), set()).add(c["name"])
    assert set(have) == set(itertools.product(BOTH, (0, 1, 2))), sorted(have)
    # 16-byte loads of one type only: L = 6148 (row bytes) and a base 8 bytes into the buffer -- FAST for int32, never for uint16
    for name in ("byte-6148", "gather-q5-6144"):
        c = CASE_BY_NAME[name]
        assert case_vec_ok(c, INT32) and not case_vec_ok(c, UINT16), name
        f32, f16 = case_forms(c, INT32), case_forms(c, UINT16)
        assert any(FAST in fs for fs in f32.values()) and not any(FAST in fs for fs in f16.values()), name
        assert any(TAIL in fs for fs in f16.values()), name
    c = CASE_BY_NAME["byte-6148"]
    assert c["L"] == c["ldr"] == 6148 and c["off"] == 0
    # ... and pitched rows whose padding the kernel must not read
    assert any(c["ldr"] > c["L"] and case_vec_ok(c, INT32) and case_vec_ok(c, UINT16) for c in CASES)


def test_every_visit_and_class_source():
    have = {(v, case_clsw(c)) for c in CASES for v in visits(c)}
    assert have >= set(itertools.product(VISITS, (0, 1, 2))), sorted(set(itertools.product(VISITS, (0, 1, 2))) - have)
    # pairs run all three chunk forms (NQ = 2 instantiates each of them once more)
    for w in (0, 1, 2):
        ok = False
        for c in CASES:
            d = case_data(c["name"])
            if case_clsw(c) != w or c["class_order"] == "off" or not certain_visits(d["qcls"], d["flags"]).get(("pair", 1)):
                continue
            pair_cls = {int(k) for k in np.unique(d["qcls"]) if (d["flags"][d["qcls"] == k] == 1).all() and (d["qcls"] == k).sum() >= 2}
            for rt in c["rt"]:
                ok |= any({GENERAL, FAST, TAIL} <= set(fs) for (u, call), fs in case_forms(c, rt).items() if int(d["qcls"][u]) in pair_cls)
        assert ok, w
    # qidx NULL, and every class a uniform flag 2
    c = CASE_BY_NAME["null-qidx-6144"]
    assert c["qidx"] == "null" and set(certain_visits(case_data(c["name"])["qcls"], case_data(c["name"])["flags"])) == {("pair", 2)}
    # the Q = 3,000 case: segments of 375, more draws than any grid of resident workgroups (at most two per CU on 256 CUs), lists of 37
    c = CASE_BY_NAME["q3000-37"]
    assert c["Q"] == 3000 and c["L"] == c["gallery"] == 37 and (c["Q"] + 1) // 2 > 2 * 2 * 256 and c["class_order"] in ("on", "both")
    assert set(case_data(c["name"])["flags"].tolist()) == {0, 1, 2}


def test_fast_settings():
    """FAST under whole-list AHP, under a clipped AHP that spans chunks with its end point on either side of a chunk edge, and under a
    clip beyond the list (clamped)."""
    whole = clamped = False
    ends = {}
    for c in CASES:
        d = case_data(c["name"])
        for rt in c["rt"]:
            if not case_vec_ok(c, rt):
                continue
            for (u, call), fs in case_forms(c, rt).items():
                qpos = int(d["qpos"][u])
                eff_len, alen, need, last_pos, kmax = query_state(c["L"], qpos, c["ks"], call[0], call[1])
                if call[0] == 0 and FAST in fs:
                    whole = True
                if call[0] > eff_len and FAST in fs:
                    clamped = True
                if call[0] > 0 and qpos < HP_CHUNK and kmax < HP_CHUNK and call[0] <= eff_len:
                    ends.setdefault(alen - 1, set()).add(tuple(fs))
    assert whole and clamped
    # the end point in the last lane of chunk 0 / the first lanes of chunk 1 (the query at rank 0 shifts it by one): chunk 1 exists and
    # is general; in the last lane of chunk 1 / the first lanes of chunk 2: chunk 1 is FAST, chunk 2 general
    # (with AP the walk goes on to the end of the list: general chunks)
    # alen - 1 = 4094 = 2048 + 2046 is the last end point chunk 1 owns itself (the last lane's last rank: the query ahead of it
    # shifts effective rank 4094 to position 4095): the largest clip for which chunk 1 is NOT interior
    assert ends.get(2046) and ends.get(4094) == {(GENERAL, GENERAL)}, (ends.get(2046), ends.get(4094))
    for e in (2047, 2048, 2049):
        assert ends.get(e) and all(len(fs) >= 2 and set(fs) == {GENERAL} for fs in ends[e]), (e, ends.get(e))
    for e in (4095, 4096, 4097):
        assert ends.get(e) and all(fs[:3] == (GENERAL, FAST, GENERAL) and fs.count(FAST) == 1 for fs in ends[e]), (e, ends.get(e))
    assert any(len(fs) > 3 for e in (4095, 4096, 4097) for fs in ends[e]) and any(len(fs) == 3 for e in (4095, 4096, 4097) for fs in ends[e])


def test_positions_cutoffs_lengths_and_class_counts():
    qpos_seen, ks_seen, absent_kinds = set(), set(), set()
    for c in CASES:
        d = case_data(c["name"])
        L = c["L"]
        for u, p in enumerate(c["pos"]):
            qpos_seen.add("L-1" if (p == LAST or p == L - 1) and L > 2050 else p)
            if p in (ABS, OUT):
                assert d["qpos"][u] == L and ((d["qidx"] is None or d["qidx"][u] < 0) == (p == ABS)), c["name"]
        eff = {int(query_state(L, int(q), c["ks"], -1, 0)[0]) for q in d["qpos"]}
        ks = list(c["ks"])
        if not ks:
            ks_seen.add("nk0")
        if ks and ks_iota(ks):
            ks_seen.add("iota%d" % len(ks))
        if ks and sorted(ks) != ks and len(set(ks)) < len(ks):
            ks_seen.add("unsorted-dup")
        if ks and max(ks) < HP_CHUNK and L > 2 * HP_CHUNK:
            ks_seen.add("first-chunk")
        if {2048, 2049} <= set(ks):
            ks_seen.add("2048-2049")
        if ks and max(ks) == L - 1 and L - 1 in eff:
            ks_seen.add("k==eff_len present")
        if ks and max(ks) == L and eff == {L}:
            ks_seen.add("k==eff_len absent")
        if ks and max(ks) == L and eff == {L} and L > 2 * HP_CHUNK:
            ks_seen.add("k==eff_len absent, several chunks")
    assert qpos_seen >= {0, 1, 1000, 2047, 2048, 2049, "L-1", ABS, OUT}, qpos_seen
    assert ks_seen >= {"nk0", "iota1", "iota300", "iota512", "unsorted-dup", "first-chunk", "2048-2049", "k==eff_len present",
                       "k==eff_len absent", "k==eff_len absent, several chunks"}, ks_seen
    assert {c["L"] for c in CASES} >= {1, 2, 2047, 2048, 2049, 6144, 6148, 6151, 8197}
    assert {c["C"] for c in CASES} >= {1, 23, 300, 1100}
    # 1,100 classes: two per thread of the order kernel, queries in both classes of a thread, most classes without a query
    c = CASE_BY_NAME["C1100-300"]
    assert order_classes_per_thread(c["C"]) == 2 and {1024, 1025} <= set(c["qcls"]) and len(set(c["qcls"])) < 10 and case_clsw(c) == 2
    # a query none of whose class's items is in its list (present and searched for: the relevant count stays 0 behind its removal)
    c = CASE_BY_NAME["gather-40000"]
    d = case_data(c["name"])
    norel = [u for u in range(c["Q"]) if d["qcls"][u] == c["norel"]]
    assert norel and all(((d["cls"][d["rk"][u]] == c["norel"]) & (d["rk"][u] != (d["qidx"][u]))).sum() == 0 for u in norel)
    assert all(case_oracle(c["name"], 0, 1)[u, -1] == 0.0 for u in norel) and (d["cls"] == c["norel"]).sum() > 100
    assert c["gallery"] == 40000 and case_clsw(c) == 0 and case_clsw(CASE_BY_NAME["gather-q5-6144"]) == 0
    # output rows wider than 2 nk + 3, pitched rankings, a base off the start of its buffer, curves longer than the lists
    assert any(c["ldo_pad"] == 5 and len(c["ks"]) == 0 for c in CASES) and any(c["ldo_pad"] == 5 and len(c["ks"]) > 0 for c in CASES)
    assert any(c["ldr"] > c["L"] for c in CASES) and any(c["off"] for c in CASES)
    assert {(c["rcp_len"], c["L"]) for c in CASES} >= {(5000, 300), (8197, 6148)}
    assert curve_len(8197) != curve_len(6148)                                   # the row pitch of the table differs from the list's own
    # the reciprocal-curve cases
    assert {n for _, n in RCP_CASES} == {1, 2047, 2048, 2049, 5000, 264000} and curve_len(264000) // HP_THREADS > RCP_GRID_CAP


# ------------------------------------------------------------------ CPU: input conditions and the oracle

@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_inputs_and_oracle(name):
    c, d = CASE_BY_NAME[name], case_data(name)
    L, G = c["L"], c["gallery"]
    rk = d["rk"]
    assert rk.min() >= 0 and rk.max() < G and d["cls"].min() >= 0 and d["cls"].max() < c["C"] and d["qcls"].max() < c["C"]
    srt = np.sort(rk, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                                   # distinct indices (so the query's index at most once)
    if d["qidx"] is not None:
        assert ((rk == d["qidx"][:, None]).sum(axis=1) <= 1).all()
    for best in (d["best_w"], d["best_l"]):
        assert best.shape[1] >= c["rcp_len"] and (np.diff(best, axis=1) > 0).all()
        for u in range(c["Q"]):                                                 # ranks behind the query divide by best - 1
            q = int(d["qpos"][u])
            if q < L - 1:
                assert (best[d["qcls"][u], max(q + 1, 1):L] - 1.0 > 0).all(), (name, u)
    for ahp_len, want_ap in c["calls"]:
        out = case_oracle(name, ahp_len, want_ap)
        assert out.shape == (c["Q"], 2 * len(c["ks"]) + 3) and np.isfinite(out).all(), (name, ahp_len, want_ap)


@pytest.mark.parametrize("present", [True, False])
def test_standin_agrees_with_the_host_mirror(present):
    """_hprec_standin == ClassHierarchy.hierarchical_precision (1e-12) with the query at rank 0, in the middle, last and absent, and
    k == eff_len -- the statement tests/test_host.py holds against the reference's own values."""
    import torch
    from class_hierarchy import ClassHierarchy
    from test_dp_gloo import _hprec_standin
    parents = {100: [], 101: [100], 102: [100], 103: [102], 0: [101], 1: [101], 2: [101], 3: [103], 4: [103], 5: [102]}
    children = {}
    for ch, ps in parents.items():
        for p in ps:
            children.setdefault(p, []).append(ch)
    h = ClassHierarchy({k: v for k, v in parents.items() if v}, children)
    classes = [0, 1, 2, 3, 4, 5]
    rng = np.random.default_rng(5 + present)
    L = 41
    cls = rng.permutation(np.arange(L) % 6).astype(np.int32)
    tab_w, tab_l = h.similarity_tables(classes)
    best_w = np.stack([np.cumsum(np.sort(tab_w[c, cls])[::-1]) for c in range(6)])
    best_l = np.stack([np.cumsum(np.sort(tab_l[c, cls])[::-1]) for c in range(6)])
    labels = {i: int(cls[i]) for i in range(L)}
    rows, qids, qcls = [], [], []
    if present:
        for qid, p in ((3, 0), (7, 20), (11, L - 1), (12, 1)):
            rest = [i for i in rng.permutation(L).tolist() if i != qid]
            rows.append(rest[:p] + [qid] + rest[p:])
            qids.append(qid)
            qcls.append(int(cls[qid]))
        ks, eff = [1, 5, L - 1], L - 1
    else:
        for t in range(4):
            qid = 1000 + t
            labels[qid] = t
            rows.append(rng.permutation(L).tolist())
            qids.append(qid)
            qcls.append(t)
        ks, eff = [1, 5, L], L
    args = [torch.from_numpy(np.ascontiguousarray(a)) for a in (np.array(rows, dtype=np.int32), cls, np.array(qcls, dtype=np.int32),
            np.array(qids, dtype=np.int32), tab_w, tab_l, best_w, best_l, np.array(ks, dtype=np.int32))]
    for ahp, ahp_len in ((True, 0), (7, 7), (eff, eff)):
        _, per_q = h.hierarchical_precision({q: r for q, r in zip(qids, rows)}, labels, ks, compute_ahp=ahp, compute_ap=True)
        got = _hprec_standin(*args, ahp_len=ahp_len, want_ap=True).numpy()
        tag = "" if ahp is True else "@%d" % ahp
        names = ["P@%d (WUP)" % k for k in ks] + ["P@%d (LCS_HEIGHT)" % k for k in ks] + ["AHP%s (WUP)" % tag, "AHP%s (LCS_HEIGHT)" % tag, "AP"]
        assert set(names) == set(per_q)
        for col, n in enumerate(names):
            want = np.array([per_q[n][q] for q in qids])
            assert np.isfinite(want).all() and np.abs(got[:, col] - want).max() <= 1e-12, (n, ahp)


# ------------------------------------------------------------------ CPU: would the table notice?  A model of the walk, one defect at a time

DEFECTS = {
    "interior-edge": "hprec.hip:401 `base + HP_CHUNK - 2 <= alen - 1`: the chunk whose last rank is the clip's end point runs FAST",
    "interior-at-query": "hprec.hip:401 `base >= qpos`: a chunk that begins with the query itself runs FAST",
    "tail-mask": "hprec.hip:306 `i <= last_pos`: the TAIL form keeps one position behind the list",
    "cuts-edge": "hprec.hip:286 `base < kmax`: a largest cut-off on the first rank of a chunk is not looked for",
    "last-pos": "hprec.hip:259 `need` for `need + 1`: the walk stops one position early",
    "whole-list-end": "hprec.hip:266 `i_last = eff_len`: the last end point of a query that is last in its list",
    "clip-clamp": "hprec.hip:254 `alen = ahp_len`: a clip beyond the list is not clamped",
}


def model(c, d, u, ahp_len, want_ap, vec, defect=None):
    """One query the way hprec_kernel walks it -- chunk by chunk, each in the form the restatements choose, with the masks, the curve
    half and the end points of that form -- in NumPy's own summation order.  `defect`: one of DEFECTS.  -> [2 nk + 3], NaN where the
    kernel writes nothing."""
    L, ks, nk = c["L"], list(c["ks"]), len(c["ks"])
    qc, qpos = int(d["qcls"][u]), int(d["qpos"][u])
    kmax = max(ks) if nk else 0
    eff_len = L - 1 if qpos < L else L
    alen = min(ahp_len, eff_len) if ahp_len > 0 else eff_len
    if defect == "clip-clamp" and ahp_len > 0:
        alen = ahp_len
    need = kmax
    if ahp_len >= 0:
        need = max(alen, need)
    if want_ap:
        need = eff_len
    last_pos = need + 1 if need < L else L
    if defect == "last-pos":
        last_pos = need if need < L else L
    span = (max(L, last_pos) + HP_CHUNK) // HP_CHUNK * HP_CHUNK + HP_CHUNK
    rank = np.zeros(span, dtype=np.int64)                      # load_ranks: 0 from the bound on
    rank[:L] = d["rk"][u]
    kls = d["cls"][rank]
    sim = np.stack([d["tab_w"][qc][kls], d["tab_l"][qc][kls]])
    best = np.stack([d["best_w"][qc], d["best_l"][qc]])
    with np.errstate(divide="ignore"):
        behind, ahead = np.zeros((2, span)), np.zeros((2, span))      # se_hprec_reciprocal_curves: +0 behind the curve
        n = min(c["rcp_len"], span)
        behind[:, :n], ahead[:, :n] = 1.0 / (best[:, :n] - 1.0), 1.0 / best[:, :n]
    out = np.full(2 * nk + 3, np.nan)
    car, car_r, acc, acc_ap, ends = np.zeros(2), 0, np.zeros(2), 0.0, np.zeros((2, 2))
    for base in range(0, last_pos, HP_CHUNK):
        i = np.arange(base, base + HP_CHUNK)
        cuts = nk > 0 and (base < kmax if defect == "cuts-edge" else base <= kmax)
        edge = (base + HP_CHUNK - 2 <= alen - 1) if defect == "interior-edge" else (base + HP_CHUNK - 2 < alen - 1)
        after = (base >= qpos) if defect == "interior-at-query" else (base > qpos)
        interior = bool(vec) and ahp_len >= 0 and not cuts and after and base + HP_CHUNK <= last_pos and edge
        tail = ahp_len == 0 and not cuts and base > qpos
        if interior:
            live, t = np.ones(HP_CHUNK, dtype=bool), behind[:, i]
        elif tail:
            live, t = (i <= last_pos) if defect == "tail-mask" else (i < last_pos), behind[:, i]
        else:
            live, t = (i < last_pos) & (i != qpos), np.where(i < qpos, ahead[:, i], behind[:, i])
        cum = car[:, None] + np.cumsum(np.where(live, sim[:, i], 0.0), axis=1)
        rel = live & (kls[i] == qc)
        if interior:
            acc += (cum * t).sum(axis=1)
        elif tail:
            acc += (cum * t)[:, i < last_pos].sum(axis=1)
        else:
            j = np.where(i < qpos, i, i - 1)
            ok = (i < last_pos) & (i != qpos)
            with np.errstate(invalid="ignore"):                # 0 x inf in the query's own slot (best[0] - 1 = 0): masked below
                y = cum * t
            if ahp_len >= 0:
                acc += y[:, ok & (j < alen)].sum(axis=1)
                for sel, e in ((ok & (j < alen) & (j == 0), 0), (ok & (j < alen) & (j == alen - 1) & (ahp_len > 0), 1)):
                    if sel.any():
                        ends[:, e] = y[:, sel][:, 0]
            if cuts:
                for s, k in enumerate(ks):
                    sel = ok & (j == k - 1)
                    if sel.any():
                        out[s], out[nk + s] = y[0, sel][0], y[1, sel][0]
        if want_ap:
            j1 = np.where(i < qpos, i + 1, i)
            with np.errstate(divide="ignore"):                 # (a defect may keep the query's own slot at rank 0)
                acc_ap += float(((car_r + np.cumsum(rel))[rel] / j1[rel]).sum())
        car, car_r = cum[:, -1].copy(), car_r + int(rel.sum())
    if ahp_len == 0 and eff_len > 0:
        i_last = eff_len if defect == "whole-list-end" else (eff_len - 1 if eff_len - 1 < qpos else eff_len)
        ends[:, 1] = car * (ahead[:, i_last] if i_last < qpos else behind[:, i_last])
    if ahp_len >= 0:
        out[2 * nk:2 * nk + 2] = (1.0 / (ahp_len if ahp_len > 0 else eff_len)) * (acc - 0.5 * (ends[:, 0] + ends[:, 1]))
    if want_ap:
        out[2 * nk + 2] = acc_ap / car_r if car_r > 0 else 0.0
    return out


def model_rows(c, rt, defect=None, limit=64):
    """{call: (queries, [len(queries), 2 nk + 3])} of the model on (up to `limit`, evenly spread) queries of a case."""
    d = case_data(c["name"])
    us = np.unique(np.linspace(0, c["Q"] - 1, min(c["Q"], limit)).astype(int))
    return {call: (us, np.stack([model(c, d, int(u), call[0], call[1], case_vec_ok(c, rt), defect) for u in us])) for call in c["calls"]}


def model_rejected(c, rt, defect):
    """The GPU test's comparison (1e-10 on every produced column, NaN counts as a miss) applied to the model."""
    nk = len(c["ks"])
    for (ahp_len, want_ap), (us, got) in model_rows(c, rt, defect).items():
        cols = list(range(2 * nk)) + ([2 * nk, 2 * nk + 1] if ahp_len >= 0 else []) + ([2 * nk + 2] if want_ap else [])
        want = case_oracle(c["name"], ahp_len, want_ap)[us]
        if not (np.abs(got[:, cols] - want[:, cols]) <= 1e-10).all():
            return True
    return False


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_model_of_the_walk_agrees_with_the_oracle(name):
    """The restated forms, masks and end points, put together, ARE the reference's numbers on every case: what the CPU tests above
    claim about the paths of a case is a claim about a walk that computes the right thing."""
    c = CASE_BY_NAME[name]
    for rt in c["rt"]:
        assert not model_rejected(c, rt, None), (name, rt)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_table_rejects_a_walk_with_one_defect(defect):
    """Each single-condition defect of the walk, injected into the model, misses the GPU test's bound on at least one case."""
    hit = next((c["name"] + "/" + rt for c in CASES if c["Q"] <= 48 for rt in c["rt"] if model_rejected(c, rt, defect)), None)
    print("%s: first rejected by %s" % (defect, hit))
    assert hit, DEFECTS[defect]
