"""CPU: the instantiation matrix of csrc/hxe.hip -- the host's choices restated, the case tables of tests/test_gpu_hxe_matrix.py tied
to them (all 48 instantiations, every axis on both paths, every claimed label depth), the float64 references on the new inputs
(``range_model`` == canon), and the teeth of the comparators: ``range_model`` with one defect at a time has to be rejected.

The host's choices, restated from se_hxe_* / se_soft_xent_* (change the dispatch in hxe.hip and these with it)
------------------------------------------------------------------------------------------------------------
G: 64 threads per row (a wave; four rows per workgroup) up to C = XE_WAVE_MAX_C = 1024, the 256 threads of a workgroup above.
VEC: the base and the row pitch of every buffer of the call are 16-byte aligned -- the logits; ``pos`` (HXE) or the table (soft
labels); ``dz`` (the _bwd entry points).  The unit is E = 8 classes when the logits or dz are bf16, else 4; a scalar form has E = 1.
48 instantiations: fwd <BF16, VEC, G> 8 + bwd <ZBF, DBF, VEC, G> 16, for each of the two losses."""
import collections
import itertools

import numpy as np
import pytest

import _hxe_canon as hc
from test_class_embedding_host import load_hierarchy

F32, BF16 = 0, 1
WAVE_MAX_C = 1024                       # XE_WAVE_MAX_C (csrc/softmax_xent.h)
ENTRIES = ("hxe_fwd", "hxe_bwd", "soft_fwd", "soft_bwd")


def path_of(C):
    return 64 if C <= WAVE_MAX_C else 256


def unit(zbf, dbf=None):
    return 8 if (zbf or dbf) else 4


def placement(layout, C, dtype):
    """(row pitch, offset of the first element from a 16-byte aligned buffer) in elements of ``dtype``.  contig; pad16: the pitch
    rounded up to a 16-byte multiple plus 16 bytes; odd: C + 1; off1: pad16's pitch one element past the boundary; pitch<N>."""
    per16 = 8 if dtype == BF16 else 4
    padded = -(-C // per16) * per16 + per16
    if layout.startswith("pitch"):
        return int(layout[5:]), 0
    return {"contig": (C, 0), "pad16": (padded, 0), "odd": (C + 1, 0), "off1": (padded, 1)}[layout]


def aligned16(layout, C, dtype):
    ld, off = placement(layout, C, dtype)
    return off == 0 and (ld * (2 if dtype == BF16 else 4)) % 16 == 0


def vec_ok(entry, case):
    """aligned16(logits, ldz) && [aligned16(pos) | aligned16(table, ldt)] && [_bwd: aligned16(dz, lddz)], as the C code decides."""
    C = case.C
    ok = aligned16(case.zlay, C, case.zdt)
    ok = ok and (case.third == "aligned" if entry.startswith("hxe") else aligned16(case.third, C, F32))
    if entry.endswith("bwd"):
        ok = ok and aligned16(case.dlay, C, case.ddt)
    return ok


def instantiation(entry, case):
    """The template arguments the entry point picks: <BF16, VEC, G> forward, <ZBF, DBF, VEC, G> backward."""
    if entry.endswith("fwd"):
        return (bool(case.zdt), vec_ok(entry, case), path_of(case.C))
    return (bool(case.zdt), bool(case.ddt), vec_ok(entry, case), path_of(case.C))


def all_instantiations(entry):
    n = 2 if entry.endswith("fwd") else 3
    return {bools + (G,) for bools in itertools.product((False, True), repeat=n) for G in (64, 256)}


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even) as float32; no NaN comes here."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- trees and problems
_CACHE = {}


def _hierarchy(edges):
    from class_hierarchy import ClassHierarchy
    parents, children = {}, {}
    for p, c in edges:
        parents.setdefault(c, []).append(p)
        children.setdefault(p, []).append(c)
    return ClassHierarchy(parents, children)


def tree(name):
    """(hierarchy, classes, canon, encoding dict) of a named tree, built once."""
    key = ("tree", name)
    if key not in _CACHE:
        if name == "c1":
            h, classes = hc.one_class_tree()
        elif name == "c2":
            h, classes = _hierarchy([(10, 0), (10, 1)]), [0, 1]
        elif name == "cat33":
            h, classes = hc.caterpillar_tree(33)
        elif name == "cat33x1000":
            h, classes = hc.caterpillar_tree(33, 1000)
        elif name == "rand20011":
            h, classes = hc.random_tree(20011, seed=20011, internal=300)
        elif name.startswith("rand"):
            h, classes = hc.random_tree(int(name[4:]), seed=int(name[4:]))
        else:
            h, classes = load_hierarchy(name)
        _CACHE[key] = (h, classes, hc.Canon(h, classes), h.hxe_encoding(classes, alpha=0.1))
    return _CACHE[key]


def depths(name):
    return np.diff(tree(name)[3]["path_off"])


def by_depth(name):
    """One label each at the smallest h of the tree, at 8, 9, 16, 17 and at the largest: the first class of that level count."""
    d = depths(name)
    want = sorted({int(d.min()), 8, 9, 16, 17, int(d.max())} & set(d.tolist()))
    return [int(np.flatnonzero(d == k)[0]) for k in want]


HxeProblem = collections.namedtuple("HxeProblem", "tree labels depths spread")
# labels: a list, "depth" (by_depth) or ("rng", B).  depths: the level counts CLAIMED for the labels (None: not claimed), checked
# against the encoding by test_every_claimed_label_depth_is_the_depth_in_the_encoding.
HXE_PROBLEMS = collections.OrderedDict([
    ("c1", HxeProblem("c1", [0] * 5, [0] * 5, 4.0)),                                       # h = 0: path_off = [0, 0], nnz = 0
    ("c2", HxeProblem("c2", ("rng", 4), [1] * 4, 4.0)),
    ("rand7", HxeProblem("rand7", ("rng", 5), None, 4.0)),
    ("rand8", HxeProblem("rand8", ("rng", 4), None, 15.0)),
    ("rand9", HxeProblem("rand9", ("rng", 1), None, 4.0)),
    ("cat33", HxeProblem("cat33", list(range(33)), list(range(1, 33)) + [32], 4.0)),       # every h from 1 to 32 in one batch
    ("cifar", HxeProblem("cifar", "depth", "measured", 15.0)),
    ("ilsvrc", HxeProblem("ilsvrc", "depth", "measured", 4.0)),
    ("rand1024", HxeProblem("rand1024", ("rng", 5), None, 4.0)),
    ("cat33x1000", HxeProblem("cat33x1000", list(range(33)) + [33, 1032], list(range(1, 33)) + [32, 1, 1], 4.0)),
    ("rand1025", HxeProblem("rand1025", "depth", "measured", 4.0)),
    ("rand1031", HxeProblem("rand1031", ("rng", 2), None, 4.0)),
    ("rand1032", HxeProblem("rand1032", ("rng", 2), None, 15.0)),
    ("inat2018", HxeProblem("inat2018", ("rng", 3), None, 4.0)),
    ("rand20011", HxeProblem("rand20011", "depth", "measured", 4.0)),
])
# what by_depth has to find on the trees whose labels are chosen by depth (measured once on the CPU, asserted ever since)
MEASURED_DEPTHS = {"cifar": [2, 8], "ilsvrc": [2, 8, 9, 16], "rand1025": [1, 8, 9, 16, 17, 24], "rand20011": [1, 8, 9, 16, 17, 21]}

SoftProblem = collections.namedtuple("SoftProblem", "C B table inf")
# table: "synthetic" (hc.synthetic_rows: non-negative, not normalised, a quarter of the entries exactly 0) or "cifar" (the real
# soft_label_table(classes, 10.0)).  inf: row 0 gets a -inf logit under a zero target, row 1 under a non-zero target.
SOFT_PROBLEMS = collections.OrderedDict([
    ("s1", SoftProblem(1, 1, "synthetic", False)),
    ("s2", SoftProblem(2, 4, "synthetic", False)),
    ("s7", SoftProblem(7, 5, "synthetic", False)),
    ("s8", SoftProblem(8, 4, "synthetic", False)),
    ("s9", SoftProblem(9, 5, "synthetic", False)),
    ("scifar", SoftProblem(100, 33, "cifar", False)),
    ("sinf100", SoftProblem(100, 3, "synthetic", True)),
    ("s1000", SoftProblem(1000, 5, "synthetic", False)),                                   # ImageNet-size, 8-wide units in bf16
    ("s1023", SoftProblem(1023, 5, "synthetic", False)),
    ("s1024", SoftProblem(1024, 33, "synthetic", False)),
    ("s1025", SoftProblem(1025, 2, "synthetic", False)),
    ("sinf1025", SoftProblem(1025, 3, "synthetic", True)),
    ("s1031", SoftProblem(1031, 2, "synthetic", False)),
    ("s1032", SoftProblem(1032, 2, "synthetic", False)),
    ("s8142", SoftProblem(8142, 3, "synthetic", False)),
])


def hxe_labels(name):
    p = HXE_PROBLEMS[name]
    if p.labels == "depth":
        return np.asarray(by_depth(p.tree), dtype=np.int64)
    if isinstance(p.labels, tuple):
        C = len(tree(p.tree)[1])
        return np.random.default_rng(C + 77).integers(0, C, size=p.labels[1])
    return np.asarray(p.labels, dtype=np.int64)


def draw_logits(B, C, zdt, seed, spread):
    """float32 [B, C], |z| <= 40, rounded to the logits' dtype: the values the device buffer holds."""
    z = np.clip(np.random.default_rng(seed).standard_normal((B, C)) * spread, -40.0, 40.0).astype(np.float32)
    return bf16_round(z) if zdt == BF16 else z


def hxe_reference(name, zdt):
    """dict of a problem's inputs and its canon result, computed once and never written to: z float32 [B, C] (rounded to the logits'
    dtype), y, ref (Canon.hxe on the rounded inputs), enc (the host encoding), C, B."""
    key = ("href", name, zdt)
    if key not in _CACHE:
        p = HXE_PROBLEMS[name]
        h, classes, canon, enc = tree(p.tree)
        y = hxe_labels(name)
        C, B = len(classes), len(y)
        z = draw_logits(B, C, zdt, seed=C + B, spread=p.spread)
        ref = canon.hxe(z.astype(np.float64), y, alpha=0.1)
        for a in [z, y] + [v for v in ref.values()]:
            a.setflags(write=False)
        _CACHE[key] = {"z": z, "y": y, "ref": ref, "enc": enc, "C": C, "B": B}
    return _CACHE[key]


def soft_reference(name, zdt):
    """As hxe_reference: z, y, rows float32 [B, C] (the table rows of the labels), table (the whole float32 table below C = 1024,
    else None: only the labels' rows exist, the rest of the device table is 0), ref (hc.soft), C, B."""
    key = ("sref", name, zdt)
    if key not in _CACHE:
        p = SOFT_PROBLEMS[name]
        C, B = p.C, p.B
        rng = np.random.default_rng(C * 13 + B)
        if p.table == "cifar":
            h, classes = tree("cifar")[:2]
            table = h.soft_label_table(classes, 10.0)
        else:
            table = hc.synthetic_rows(C, C, seed=C) if C < WAVE_MAX_C else None
        if table is not None:
            y = rng.integers(0, C, size=B)
            rows = table[y]
        else:
            y = np.sort(rng.choice(C, size=B, replace=False))            # distinct: one device row per batch row
            rows = hc.synthetic_rows(C, B, seed=C)
        z = draw_logits(B, C, zdt, seed=C + B + 5, spread=4.0)
        if p.inf:
            z[0, np.flatnonzero(rows[0] == 0)[1]] = -np.inf
            z[1, np.flatnonzero(rows[1] != 0)[1]] = -np.inf
        ref = hc.soft(z.astype(np.float64), np.arange(B), rows)
        for a in [z, y, rows] + [v for v in ref.values()]:
            a.setflags(write=False)
        _CACHE[key] = {"z": z, "y": y, "rows": rows, "table": table, "ref": ref, "C": C, "B": B}
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------- case tables
Case = collections.namedtuple("Case", "problem C B zdt ddt zlay dlay third")        # third: pos (HXE) or table (soft) layout
DT = list(itertools.product((F32, BF16), repeat=2))
# every dtype pair on: all aligned; each buffer of the call misaligned in turn (pitch or base); HXE's pos one int32 into its buffer
FULL_H = [dt + f for dt in DT for f in (("pad16", "pad16", "aligned"), ("odd", "odd", "aligned"), ("off1", "pad16", "aligned"),
                                        ("pad16", "off1", "aligned"), ("pad16", "pad16", "offset"))]
LIGHT_H = [(F32, F32, "contig", "contig", "aligned"), (F32, F32, "pad16", "pad16", "aligned"), (BF16, BF16, "pad16", "pad16", "aligned"),
           (BF16, F32, "pad16", "pad16", "offset"), (F32, BF16, "odd", "pad16", "aligned")]
FULL_S = [dt + f for dt in DT for f in (("pad16", "pad16", "pad16"), ("odd", "odd", "contig"), ("off1", "pad16", "pad16"),
                                        ("pad16", "off1", "pad16"), ("pad16", "pad16", "odd"))]
LIGHT_S = [(F32, F32, "contig", "contig", "contig"), (F32, F32, "pad16", "pad16", "pad16"), (BF16, BF16, "pad16", "pad16", "pad16"),
           (BF16, F32, "pad16", "pad16", "odd"), (F32, BF16, "odd", "pad16", "contig")]
HXE_FORMS = {
    "cat33": FULL_H, "ilsvrc": FULL_H, "cat33x1000": FULL_H, "rand1032": FULL_H,
    # C = 8142: pitch 8144 is 16-byte aligned in both dtypes, the contiguous rows are not (bf16 logits and dz on scalar units above
    # 1024 classes: learn_classifier.py --loss hxe under bf16 autocast on iNaturalist)
    "inat2018": [(F32, F32, "pitch8144", "pitch8144", "aligned"), (BF16, BF16, "pitch8144", "pitch8144", "aligned"),
                 (BF16, BF16, "contig", "contig", "aligned"), (F32, F32, "contig", "contig", "offset")],
    "rand20011": [(F32, F32, "pad16", "pad16", "aligned"), (BF16, BF16, "pad16", "pad16", "aligned"),
                  (F32, BF16, "contig", "contig", "aligned")],
}
SOFT_FORMS = {
    "s1023": FULL_S, "s1024": FULL_S, "s1025": FULL_S, "s1032": FULL_S,
    "s8142": [(F32, F32, "pitch8144", "pitch8144", "pitch8144"), (BF16, BF16, "pitch8144", "pitch8144", "pitch8144"),
              (BF16, BF16, "contig", "contig", "contig"), (F32, BF16, "pad16", "pad16", "odd")],
}


def _hxe_cases():
    out = []
    for name, p in HXE_PROBLEMS.items():
        C = {"c1": 1, "c2": 2, "cat33": 33, "cat33x1000": 1033, "cifar": 100, "ilsvrc": 1000, "inat2018": 8142}.get(p.tree) or int(p.tree[4:])
        B = len(MEASURED_DEPTHS[name]) if p.labels == "depth" else (
            p.labels[1] if isinstance(p.labels, tuple) else len(p.labels))
        out += [Case(name, C, B, *f) for f in HXE_FORMS.get(name, LIGHT_H)]
    return out


HXE_CASES = _hxe_cases()
SOFT_CASES = [Case(name, p.C, p.B, *f) for name, p in SOFT_PROBLEMS.items() for f in SOFT_FORMS.get(name, LIGHT_S)]
DTN = {F32: "f32", BF16: "bf16"}


def case_id(c):
    return "%s-B%d-z%s-dz%s-%s-%s-%s" % (c.problem, c.B, DTN[c.zdt], DTN[c.ddt], c.zlay, c.dlay, c.third)


def entries_of(case):
    return ENTRIES[:2] if case.problem in HXE_PROBLEMS else ENTRIES[2:]


def inst_name(entry, case):
    return "%s<%s>" % (entry, ",".join(str(v).lower() for v in instantiation(entry, case)))


# ---------------------------------------------------------------------------------------------------------------------- comparators
def grad_bound(C, ref, w=1.0):
    with np.errstate(invalid="ignore"):
        return np.where(ref["absgrad"] == 0, 0.0, hc.U * abs(w) * hc.grad_factor(C, ref["x"]) * ref["absgrad"])


def compare_hxe(C, ref, loss, dz):
    """The accuracy checks of a HXE case: -> (worst loss error / bound, worst dz error / bound); AssertionError on an excess."""
    loss, dz = np.asarray(loss, dtype=np.float64), np.asarray(dz, dtype=np.float64)
    bound = hc.loss_k(C) * hc.U * ref["scale"]
    err = np.abs(loss - ref["loss"])
    assert (err <= bound).all(), ("loss", err, bound)
    gb = grad_bound(C, ref)
    gerr = np.abs(dz - ref["dz"])
    assert (gerr <= gb).all(), ("dz", float(np.nan_to_num(gerr / np.maximum(gb, 1e-300), nan=np.inf).max()))
    assert (np.abs(dz.sum(axis=1)) <= gb.sum(axis=1)).all(), "a row's gradients sum to 0"
    return float((err / np.maximum(bound, 1e-300)).max()), float((gerr / np.maximum(gb, 1e-300)).max())


def compare_soft(C, ref, loss, dz):
    """The same for a soft-label case.  A row whose exact loss is +inf (a -inf logit under a non-zero target) has to be +inf; an
    element at -inf has dz = -Q exactly (p = 0), whatever the bound says there."""
    loss, dz = np.asarray(loss, dtype=np.float64), np.asarray(dz, dtype=np.float64)
    lb, gb = hc.soft_bounds(C, ref)
    fin = np.isfinite(ref["loss"])
    assert (loss[~fin] == ref["loss"][~fin]).all(), ("loss of a row with exact loss +inf", loss, ref["loss"])
    err = np.abs(loss[fin] - ref["loss"][fin])
    assert (err <= lb[fin]).all(), ("loss", err, lb[fin])
    gerr = np.abs(dz - ref["dz"])
    assert (gerr <= gb).all(), ("dz", float(np.nan_to_num(gerr / np.maximum(gb, 1e-300), nan=np.inf).max()))
    gone = np.isneginf(ref["x"])
    assert (dz[gone] == ref["dz"][gone]).all(), "dz of a class at -inf"
    rows = np.isfinite(gb).all(axis=1)
    assert (np.abs(dz.sum(axis=1))[rows] <= gb.sum(axis=1)[rows]).all(), "a row's gradients sum to 0"
    ratio = np.where(np.isfinite(gb), gerr / np.maximum(gb, 1e-300), 0.0)
    return float((err / np.maximum(lb[fin], 1e-300)).max()) if fin.any() else 0.0, float(ratio.max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare_layout_bits(results):
    """The backward has no reduction: given the same aux, dz is the same bits in every layout, unit width and logits dtype."""
    first = np.asarray(results[0], dtype=np.float32)
    assert all(same_bits(first, np.asarray(r, dtype=np.float32)) for r in results[1:]), "dz differs between two forms of one problem"


# ---------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("table,entries", [(HXE_CASES, ENTRIES[:2]), (SOFT_CASES, ENTRIES[2:])], ids=["hxe", "soft"])
def test_case_tables_reach_all_48_instantiations(table, entries):
    total = 0
    for entry in entries:
        reached = collections.defaultdict(set)
        for c in table:
            E = unit(c.zdt, c.ddt if entry.endswith("bwd") else None)
            reached[instantiation(entry, c)].add(c.C % E == 0)
        assert set(reached) == all_instantiations(entry), (entry, all_instantiations(entry) - set(reached))
        # each with a part-filled last unit and with C a multiple of the unit width
        assert all(v == {True, False} for v in reached.values()), (entry, {k: v for k, v in reached.items() if len(v) < 2})
        total += len(reached)
    assert total == 24
    assert len({case_id(c) for c in table}) == len(table)


def test_case_tables_hold_every_axis_on_both_paths():
    for table, hxe in ((HXE_CASES, True), (SOFT_CASES, False)):
        sizes = {c.C for c in table}
        assert sizes >= {1, 2, 7, 8, 9, 1024, 1025, 8142} and (20011 in sizes) == hxe
        for G in (64, 256):
            on = [c for c in table if path_of(c.C) == G]
            for dt, E in ((F32, 4), (BF16, 8)):             # C % E in {0, 1, E - 1} on a pad16 pitch, on 16-byte units of E
                entry = "hxe_fwd" if hxe else "soft_fwd"
                rem = {c.C % E for c in on if c.zdt == dt and c.zlay == "pad16" and vec_ok(entry, c)}
                assert rem >= {0, 1, E - 1}, (G, E, rem)
            assert {c.zlay for c in on} >= {"contig", "pad16", "odd", "off1"} and {c.dlay for c in on} >= {"contig", "pad16", "odd", "off1"}, G
            assert {c.third for c in on} >= ({"aligned", "offset"} if hxe else {"contig", "pad16", "odd"}), G
            assert {(c.zdt, c.ddt) for c in on} == set(DT)
            if G == 64:
                assert {c.B for c in on} >= {1, 4, 5, 33}   # slots past the end in the last workgroup: B % 4 = 1, 0, 1, 1
            else:
                assert min(c.B for c in on) >= 2
        c8142 = {(c.zlay, c.dlay) for c in table if c.C == 8142}
        assert ("pitch8144", "pitch8144") in c8142 and ("contig", "contig") in c8142
    for c in HXE_CASES + SOFT_CASES:                        # the table's C and B are the problem's
        r = (hxe_reference if c.problem in HXE_PROBLEMS else soft_reference)
        if c.C <= 1033:                                     # (the large trees: test_range_model_equals_the_canon_on_every_hxe_case)
            assert (r(c.problem, F32)["C"], r(c.problem, F32)["B"]) == (c.C, c.B), c
    assert any(p.table == "cifar" for p in SOFT_PROBLEMS.values())
    for G in (64, 256):
        assert any(p.inf and path_of(p.C) == G for p in SOFT_PROBLEMS.values())
    # the learn_classifier.py --loss hxe case under bf16 autocast on iNaturalist, and ImageNet-size bf16 soft labels
    assert any(c.C == 8142 and instantiation("hxe_bwd", c) == (True, True, False, 256) for c in HXE_CASES)
    assert any(c.C == 1000 and instantiation("soft_fwd", c) == (True, True, 64) for c in SOFT_CASES)


def test_every_claimed_label_depth_is_the_depth_in_the_encoding():
    for name, p in HXE_PROBLEMS.items():
        if p.depths is None:
            continue
        got = depths(p.tree)[hxe_labels(name)].tolist()
        want = MEASURED_DEPTHS[name] if p.depths == "measured" else p.depths
        assert got == want, (name, got, want)
    for name in MEASURED_DEPTHS:                            # by_depth found what the tree has of {min, 8, 9, 16, 17, max}
        d = set(depths(name).tolist())
        assert set(MEASURED_DEPTHS[name]) == {min(d), 8, 9, 16, 17, max(d)} & d
    assert max(MEASURED_DEPTHS["rand20011"]) > 17           # long rows on the workgroup path with a third chunk of levels


def test_caterpillar_trees_hold_every_level_count():
    assert sorted(depths("cat33").tolist()) == list(range(1, 33)) + [32]
    assert depths("cat33").tolist() == list(range(1, 33)) + [32]                 # leaf i has i + 1 levels
    assert depths("cat33x1000").tolist() == list(range(1, 33)) + [32] + [1] * 1000
    for name in ("cat33", "cat33x1000"):
        enc = tree(name)[3]
        assert enc["max_levels"] == hc.MAX_LEVELS and sorted(enc["pos"].tolist()) == list(range(len(enc["pos"])))
    h, classes = hc.caterpillar_tree(34)
    with pytest.raises(ValueError, match="33 levels"):
        h.hxe_encoding(classes)
    enc = tree("c1")[3]
    assert enc["path_off"].tolist() == [0, 0] and len(enc["lvl_lo"]) == 0 and enc["max_levels"] == 0


@pytest.mark.parametrize("name", list(HXE_PROBLEMS))
def test_range_model_equals_the_canon_on_every_hxe_case(name):
    """The reference alone is sound on the new inputs: the arithmetic of sehip.h on the range encoding, in float64, against the
    canon by explicit descendant sets -- for the inputs of every case of the table (both logits dtypes of every problem)."""
    for zdt in sorted({c.zdt for c in HXE_CASES if c.problem == name}):
        r = hxe_reference(name, zdt)
        assert {(c.C, c.B) for c in HXE_CASES if c.problem == name} == {(r["C"], r["B"])}
        m = hc.range_model(r["enc"], r["z"], r["y"])
        assert np.abs(m["loss"] - r["ref"]["loss"]).max() <= 1e-12 and np.abs(m["dz"] - r["ref"]["dz"]).max() <= 1e-12
        assert (r["ref"]["levels"] == np.diff(r["enc"]["path_off"])[r["y"]]).all()
        compare_hxe(r["C"], r["ref"], m["loss"], m["dz"])
        wild = hc.range_model(r["enc"], r["z"][:2], [-3, r["C"] + 5][:r["B"]])     # labels are clamped
        clamped = hc.range_model(r["enc"], r["z"][:2], [0, r["C"] - 1][:r["B"]])
        assert same_bits(wild["dz"], clamped["dz"])


@pytest.mark.parametrize("name", list(SOFT_PROBLEMS))
def test_soft_model_equals_the_canon_on_every_soft_case(name):
    for zdt in (F32, BF16):
        r = soft_reference(name, zdt)
        m = hc.soft_model(r["z"], r["y"], r["rows"])
        fin = np.isfinite(r["ref"]["loss"])
        assert np.abs(m["loss"][fin] - r["ref"]["loss"][fin]).max(initial=0) <= 1e-12 and (m["loss"][~fin] == np.inf).all()
        assert np.abs(m["dz"] - r["ref"]["dz"]).max() <= 1e-12
        compare_soft(r["C"], r["ref"], m["loss"], m["dz"])
        q = r["rows"]
        assert q.dtype == np.float32 and (q >= 0).all()
        if SOFT_PROBLEMS[name].table == "synthetic" and r["C"] >= 100:
            assert 0.2 <= (q == 0).mean() <= 0.3 and np.abs(q.sum(axis=1) - 1.0).min() > 1e-3       # exact zeros, not normalised
        if SOFT_PROBLEMS[name].inf:
            x = r["z"]
            assert np.isneginf(x[0]).sum() == 1 and q[0][np.isneginf(x[0])] == 0 and np.isfinite(r["ref"]["loss"][0])
            assert np.isneginf(x[1]).sum() == 1 and q[1][np.isneginf(x[1])] != 0 and r["ref"]["loss"][1] == np.inf


def _rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("defect", hc.DEFECTS)
def test_the_comparators_reject_every_defect(defect):
    """range_model with one defect at a time, through the comparators the GPU cases use: each has to miss a bound or a bit check
    on at least one case of the table.  Which cases catch it is part of the claim:
      chunk    -- only labels with more than 24 levels (the caterpillar problems);
      h0_slot  -- only h = 0 (c1): with h >= 1 aux slot 2 holds H_1, which IS H_0, so no input can tell the two reads apart;
      tail     -- only 16-byte forms with C no multiple of the unit; also a bit difference against the scalar form."""
    caught = []
    for name in HXE_PROBLEMS:
        if HXE_PROBLEMS[name].tree in ("inat2018", "rand20011"):
            continue                                        # the small problems decide; the large trees cost seconds
        forms = {(c.zdt, unit(c.zdt, c.ddt) if vec_ok("hxe_bwd", c) else 1) for c in HXE_CASES if c.problem == name}
        for zdt, E in sorted(forms):
            r = hxe_reference(name, zdt)
            m = hc.range_model(r["enc"], r["z"], r["y"], defect=defect, E=E)
            if _rejected(compare_hxe, r["C"], r["ref"], m["loss"], m["dz"]):
                caught.append(name)
            elif defect == "tail" and E > 1:
                good = hc.range_model(r["enc"], r["z"], r["y"], E=1)
                assert not _rejected(compare_layout_bits, [good["dz"], m["dz"]])            # C a multiple of E: nothing dropped
                assert r["C"] % E == 0
    caught = set(caught)
    print(defect, "caught by", sorted(caught))
    assert caught, defect
    if defect == "chunk":
        assert caught == {"cat33", "cat33x1000"}
    elif defect == "h0_slot":
        assert caught == {"c1"}
    elif defect == "tail":
        assert caught >= {"cat33", "cat33x1000", "rand7", "rand9"} and "rand8" not in caught and "rand1032" not in caught
        r = hxe_reference("cat33", F32)
        assert _rejected(compare_layout_bits, [hc.range_model(r["enc"], r["z"], r["y"], E=1)["dz"],
                                               np.nan_to_num(hc.range_model(r["enc"], r["z"], r["y"], defect="tail", E=4)["dz"])])
    else:
        # hi: every range of a caterpillar tree (the spine is visited last) and of c2 ends at C, where <= admits no class
        assert caught >= {"cifar", "ilsvrc", "rand1025"} and (defect == "hi" or caught >= {"c2", "cat33", "cat33x1000"})


def test_the_soft_comparator_rejects_a_zero_target_at_minus_infinity():
    for name, p in SOFT_PROBLEMS.items():
        r = soft_reference(name, F32)
        m = hc.soft_model(r["z"], r["y"], r["rows"], defect="zero_inf")
        assert _rejected(compare_soft, r["C"], r["ref"], m["loss"], m["dz"]) == p.inf, name
