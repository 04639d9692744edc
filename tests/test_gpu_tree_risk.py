"""GPU: se_tree_risk_topk -- the risks and the class lists of conditional risk minimisation on a class tree -- against the float64
canon of tests/_tree_risk_canon.py, which takes the heights from explicit descendant sets and knows nothing of the range encoding.

The host's path choice, restated (tree_risk.hip): a 64-lane wave per row (four rows per workgroup) up to C = 1024, the 256 threads
of a workgroup per row above.  Nothing else selects code: no alignment or pitch variant exists, `risk` and `own_h` are run-time
pointers.  The case table below reaches both instantiations, either side of the boundary, rows that share a workgroup with slots
past the end (N = 1, 5, 33 on the wave path), and a last tile / span that is partly filled (C = 37, 65, 1025, 8142).

The bound of check 2 (u = 2^-53; the kernel against the float64 canon on the same float32 inputs)
--------------------------------------------------------------------------------------------------
With s = sum_j |p_j| of the row.  A float64 sum of n terms in ANY order errs by at most (n - 1) u sum|x| to first order.  A mass is
the difference of two entries of the prefix sum, each a sum of at most C values of the row: each entry errs by at most (C - 1) u s,
the subtraction adds u (|S_hi| + |S_lo|) <= 2 u s, so |d m_l| <= 2 C u s (m_{-1} = p_k is exact).  A term lvl_h[l] * (m_l - m_{l-1})
carries the two mass errors (4 C H_max u s), one rounding of the difference (u s) and one of the product (H_max u s): at most
(4 C + 2) H_max u s.  The risk is own_h[k] * p_k (one rounding, H_max u s) plus the L terms, added in a chain of L additions whose
partial sums are at most (L + 1) H_max s in magnitude: L (L + 1) H_max u s.  Together, to first order,
      |d risk_k| <= (L + 1)(4 C + L + 3) H_max u s <= (L + 1)(4 C + L + 8) H_max u s <= 8 (C + 2)(L + 1) H_max u s       (risk_bound)
-- the last step is L <= 4 C + 8, and the ranges of a path grow strictly, so L <= C - 1.  The difference between the last two
expressions, (L + 1)(4 C + 8 - L) H_max u s, is at least C H_max u s, which covers the rounding of the float64 reference P64 @ H^T.
With the lists checked against the kernel's OWN risks (check 3) no near-tie allowance is needed, so no case is left out.
An excess over the bound is a finding to explain, not a reason to widen it."""
import numpy as np
import pytest
import torch

import _tree_risk_canon as tc

pytestmark = pytest.mark.gpu

WAVE_MAX_C = 1024
SENT_I, SENT_F = -7, 777.0
GUARD = 16
_CACHE = {}


def path_of(C):
    return "wave" if C <= WAVE_MAX_C else "workgroup"


# (tree, N, top, extra pitch of probs / risk, base pointer offset in elements, risk requested, synthetic own_h)
CASES = [
    ("c1", 1, 1, 0, 0, True, False), ("c1", 5, 1, 3, 1, True, True),
    ("c2", 1, 2, 0, 0, True, False), ("c2", 33, 1, 3, 0, False, False),
    ("rand37", 1, 20, 0, 0, True, False), ("rand37", 5, 32, 0, 1, True, True), ("rand37", 33, 5, 3, 1, False, False),
    ("rand64", 5, 5, 0, 0, True, False), ("rand64", 33, 32, 3, 0, True, True),
    ("rand65", 1, 32, 3, 1, True, False), ("rand65", 33, 20, 0, 0, False, True),
    ("cifar", 1, 1, 0, 0, True, False), ("cifar", 5, 20, 3, 0, True, False), ("cifar", 33, 32, 0, 1, False, True),
    ("cub", 5, 5, 0, 1, True, False), ("cub", 33, 32, 3, 0, True, True),
    ("ilsvrc", 1, 32, 0, 0, False, False), ("ilsvrc", 5, 20, 0, 0, True, False), ("ilsvrc", 33, 5, 3, 1, True, True),
    ("rand1024", 5, 32, 0, 0, True, False), ("rand1024", 33, 1, 3, 1, True, True),
    ("rand1025", 1, 5, 0, 0, True, False), ("rand1025", 5, 32, 3, 1, True, True), ("rand1025", 33, 20, 0, 0, False, False),
    ("inat2018", 3, 20, 0, 0, True, False), ("inat2018", 3, 32, 3, 1, False, True),
    # caterpillar trees: paths of 1 .. 32 levels, the most a path may hold (TR_LEVELS), on either path
    ("cat33", 5, 32, 0, 0, True, False), ("cat33", 33, 20, 3, 1, True, True),
    ("cat33x1000", 5, 32, 3, 1, True, True), ("cat33x1000", 33, 5, 0, 0, True, False),
]
IDS = ["%s-N%d-top%d-p%d-o%d-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "risk" if c[5] else "norisk", "own" if c[6] else "leaf") for c in CASES]


def test_case_table_reaches_every_instantiation_and_boundary():
    sizes = {len(tc.tree(c[0])[1]) for c in CASES}
    assert sizes == {1, 2, 33, 37, 64, 65, 100, 200, 1000, 1024, 1025, 1033, 8142}
    assert {host_encoding(n)["max_levels"] for n in ("cat33", "cat33x1000")} == {32}
    assert {path_of(C) for C in sizes} == {"wave", "workgroup"} and {WAVE_MAX_C, WAVE_MAX_C + 1} <= sizes
    for C in sizes:
        ns = {c[1] for c in CASES if len(tc.tree(c[0])[1]) == C}
        assert ns == {3} if C == 8142 else len(ns) >= 2, C
        tops = {c[2] for c in CASES if len(tc.tree(c[0])[1]) == C}
        assert (C in tops) if C < 32 else (32 in tops), C
    assert {c[2] for c in CASES} >= {1, 5, 20, 32}
    for p in ("wave", "workgroup"):
        assert {c[1] for c in CASES if path_of(len(tc.tree(c[0])[1])) == p} >= {1, 5, 33}, p
    for col in (3, 4, 5, 6):                                # pitch, offset, risk, own_h: both settings on both paths
        for p in ("wave", "workgroup"):
            assert len({bool(c[col]) for c in CASES if path_of(len(tc.tree(c[0])[1])) == p}) == 2, (col, p)
    import sehip
    assert max(sizes) <= sehip.TREE_RISK_MAX_CLASSES


def host_encoding(name, own=False):
    """A tree's encoding; ``own``: with a synthetic non-zero own_h."""
    key = ("host", name, own)
    if key not in _CACHE:
        h, classes = tc.tree(name)
        enc = dict(h.tree_risk_encoding(classes))
        if own:
            enc["own_h"] = (1 + np.arange(len(classes)) % 5).astype(np.int32)
        _CACHE[key] = enc
    return _CACHE[key]


def encoding(name, own=False):
    """(host dict, device tensors) of a tree's encoding."""
    key = ("enc", name, own)
    if key not in _CACHE:
        enc = host_encoding(name, own)
        _CACHE[key] = (enc, {k: torch.from_numpy(enc[k]).cuda() for k in ("pos", "path_off", "lvl_lo", "lvl_hi", "lvl_h", "own_h")})
    return _CACHE[key]


def reference(name, kind, N, own):
    """(P float32 [N, C], canon risks) -- computed once per (tree, inputs, own_h) and never written to."""
    key = ("ref", name, kind, N, own)
    if key not in _CACHE:
        h, classes = tc.tree(name)
        C = len(classes)
        P = (tc.grid_probs if kind == "grid" else tc.softmax_probs)(N, C, seed=1000 * N + C)
        R = tc.risks(P, tc.height_table(h, classes), host_encoding(name, own)["own_h"] if own else None)
        P.setflags(write=False)
        R.setflags(write=False)
        _CACHE[key] = (P, R)
    return _CACHE[key]


def launch(P, dev, top, extra=0, off=0, want_risk=True, nnz=None, null_own=False):
    """One call on buffers with sentinels around and between everything written: (cls, risk_top, risk | None) as NumPy."""
    from sehip._lib import call
    N, C = P.shape
    ld = C + extra
    pbuf = torch.zeros(off + max(N, 1) * ld + GUARD, dtype=torch.float32, device="cuda")
    pd = pbuf[off:off + N * ld].view(N, ld)
    pd[:, :C].copy_(torch.from_numpy(np.array(P)))
    cls = torch.full((N * top + 2 * GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    rt = torch.full((N * top + 2 * GUARD,), SENT_F, dtype=torch.float64, device="cuda")
    rk = torch.full((N * ld + 2 * GUARD,), SENT_F, dtype=torch.float64, device="cuda") if want_risk else None
    call("se_tree_risk_topk", pd, ld, dev["pos"], dev["path_off"], dev["lvl_lo"], dev["lvl_hi"], dev["lvl_h"],
         int(dev["lvl_h"].numel()) if nnz is None else nnz, None if null_own else dev["own_h"], N, C, top, cls[GUARD:], rt[GUARD:],
         rk[GUARD:] if want_risk else None, ld)
    torch.cuda.synchronize()
    cls, rt = cls.cpu().numpy(), rt.cpu().numpy()
    for buf, sent in ((cls, SENT_I), (rt, SENT_F)):
        assert (buf[:GUARD] == sent).all() and (buf[GUARD + N * top:] == sent).all()
    risk = None
    if want_risk:
        rk = rk.cpu().numpy()
        assert (rk[:GUARD] == SENT_F).all() and (rk[GUARD + N * ld:] == SENT_F).all()
        rows = rk[GUARD:GUARD + N * ld].reshape(N, ld)
        assert (rows[:, C:] == SENT_F).all()                # elements C .. ldr - 1 of every row
        risk = rows[:, :C].copy()
    return cls[GUARD:GUARD + N * top].reshape(N, top), rt[GUARD:GUARD + N * top].reshape(N, top), risk


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_risks_and_lists_against_the_canon(case):
    name, N, top, extra, off, want_risk, own = case
    enc, dev = encoding(name, own)
    C = len(tc.tree(name)[1])
    for kind in ("grid", "softmax"):
        P, want = reference(name, kind, N, own)
        cls, rt, risk = launch(P, dev, top, extra, off, True, null_own=not own)
        if not want_risk:                                   # the lists are the same bits without the risk matrix
            cls2, rt2, _ = launch(P, dev, top, extra, off, False, null_own=not own)
            assert same_bits(cls, cls2) and same_bits(rt, rt2)
        if kind == "grid":                                  # check 1: exact, ties included
            assert np.array_equal(risk, want)
            want_cls, want_rt = tc.lists(want, top)
            assert np.array_equal(cls, want_cls) and np.array_equal(rt, want_rt)
        else:                                               # check 2: the derived bound
            L, H_max = enc["max_levels"], max(int(enc["lvl_h"].max(initial=0)), int(enc["own_h"].max()) if own else 0)
            err, bound = np.abs(risk - want).max(axis=1), tc.risk_bound(P, C, L, H_max)
            print("%s %s: max |risk - canon| / bound = %.3g" % (name, kind, (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (err, bound)
        own_cls, own_rt = tc.lists(risk, top)               # check 3: the canonical order of the kernel's own risks
        assert np.array_equal(cls, own_cls) and same_bits(rt, own_rt)


@pytest.mark.parametrize("name", ["cub", "rand1025"])
def test_same_bits_alone_in_a_batch_and_on_a_second_stream(name):
    enc, dev = encoding(name, True)
    P, _ = reference(name, "softmax", 33, True)
    cls, rt, risk = launch(P, dev, 20)
    for i in (0, 4, 32):                                    # a row alone (another slot of its workgroup, another grid)
        c1, r1, k1 = launch(P[i:i + 1], dev, 20)
        assert same_bits(c1[0], cls[i]) and same_bits(r1[0], rt[i]) and same_bits(k1[0], risk[i]), i
    c5, r5, k5 = launch(P[3:8], dev, 20, extra=3, off=1)
    assert same_bits(c5, cls[3:8]) and same_bits(r5, rt[3:8]) and same_bits(k5, risk[3:8])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        c2, r2, k2 = launch(P, dev, 20)
    assert same_bits(c2, cls) and same_bits(r2, rt) and same_bits(k2, risk)


@pytest.mark.parametrize("name", ["cifar", "rand1025"])
def test_non_finite_rows_get_nan_risks_and_the_first_classes(name):
    enc, dev = encoding(name, False)
    P0, _ = reference(name, "softmax", 5, False)
    clean = launch(P0, dev, 5)
    P = P0.copy()
    P[1, 7] = np.nan
    P[3, len(P[0]) - 1] = np.inf
    cls, rt, risk = launch(P, dev, 5)
    for i in (1, 3):
        assert np.isnan(risk[i]).all() and np.isnan(rt[i]).all() and cls[i].tolist() == [0, 1, 2, 3, 4]
    for i in (0, 2, 4):                                     # the neighbours are untouched
        assert same_bits(cls[i], clean[0][i]) and same_bits(rt[i], clean[1][i]) and same_bits(risk[i], clean[2][i])
    P[3, len(P[0]) - 1] = -np.inf
    assert np.isnan(launch(P, dev, 5)[2][3]).all()


@pytest.mark.parametrize("name", ["cifar", "rand1025"])
def test_garbage_tables_stay_inside_every_buffer(name):
    """The clamps: pos out of range, hi < lo, path_off beyond nnz.  Every access is clamped by construction, so the call returns,
    the classes are valid indices and the sentinels around every buffer (checked by ``launch``) are intact."""
    enc, dev = encoding(name, False)
    C = len(enc["pos"])
    rng = np.random.default_rng(7)
    bad = {"pos": rng.integers(-5 * C, 5 * C, C), "path_off": rng.integers(-50, 3 * len(enc["lvl_h"]), C + 1),
           "lvl_lo": rng.integers(-C, 2 * C, len(enc["lvl_h"])), "lvl_hi": rng.integers(-C, 2 * C, len(enc["lvl_h"])),
           "lvl_h": enc["lvl_h"], "own_h": enc["own_h"]}
    bad_dev = {k: torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda() for k, v in bad.items()}
    P, _ = reference(name, "grid", 5, False)
    for nnz in (None, 3, 0):
        cls, rt, risk = launch(P, bad_dev, 5, extra=3, off=1, nnz=nnz)
        assert ((cls >= 0) & (cls < C)).all() and np.isfinite(risk).all()


def test_wrapper_and_graph_capture():
    import sehip
    h, classes = tc.tree("cub")
    enc = h.tree_risk_encoding(classes)
    P, want = reference("cub", "grid", 33, False)
    Pd = torch.from_numpy(np.array(P)).cuda()
    cls, rt, risk = sehip.tree_risk_topk(Pd, enc, 5, return_risk=True)
    assert np.array_equal(risk.cpu().numpy(), want) and np.array_equal(cls.cpu().numpy(), tc.lists(want, 5)[0])
    assert "_sehip" in enc and len(sehip.tree_risk_topk(Pd[:, :200], enc, 1)) == 2
    with pytest.raises(sehip.SehipError):
        sehip.tree_risk_topk(Pd, enc, 33)
    with pytest.raises(sehip.SehipError):
        sehip.tree_risk_topk(Pd[:, :10], enc, 5)
    stream = torch.cuda.Stream()                            # no allocation, no synchronisation: capturable
    with torch.cuda.stream(stream):
        sehip.tree_risk_topk(Pd, enc, 5)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = sehip.tree_risk_topk(Pd, enc, 5)
        Pd.copy_(torch.from_numpy(np.ascontiguousarray(P[::-1])).cuda())
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), tc.lists(want[::-1], 5)[0])
