"""GPU: the label-embedding loss on the learned table itself (se_labelembed_table_loss_fwd / _bwd, sehip.labelembed_table_loss).

Loss, aux and the logit gradients bit for bit against se_labelembed_loss_fwd / _bwd on the gathered rows ``table[clamp(y)]``; the
table gradient bit for bit against the float32 sum of that call's ``d_tar`` rows per class in batch order (the rule restated in
tests/test_labelembed_host.py, which also holds the case table to the kernel's boundaries); everything against the float64 oracle;
determinism (repeats, a busy second stream), HIP-graph replay, and the autograd op on the halves of one [B, 2 C] tensor."""
import numpy as np
import pytest
import torch

from oracle import loss_oracle as lo
from test_labelembed_host import (COL1, CONTIG, GROUP_CLASSES, NO_MASK_CASE, PADDED, TABLE_CASES, case_inputs, pitch, scan_group_labels,
                                  table_grad_rule)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SENT32 = np.int32(0x7FC0DEAD)       # a quiet NaN with a payload no kernel writes
TAU, ALPHA, BETA = 2.0, 0.9, 0.5
AUX = 12                            # floats of the per-sample record; the batch scale follows the B records


def call(name, *args):
    from sehip._lib import call as c
    return c(name, *args)


def place(a, layout):
    """Device copy of the float32 matrix ``a`` [rows, d] in ``layout``: NaN in the pitch padding / the skipped column, NaN guard rows."""
    rows, d = a.shape
    ld = pitch(layout, d)
    buf = torch.full((rows + 2, ld), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[1:rows + 1, 1:] if layout == COL1 else buf[1:rows + 1, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


class Guarded(object):
    """A [rows, cols] float32 output of pitch ``ld`` inside a sentinel buffer (one guard row before, two after)."""

    def __init__(self, rows, cols, ld):
        self.rows, self.cols = rows, cols
        self.buf = torch.full((rows + 3, ld), int(SENT32), dtype=torch.int32, device="cuda")
        self.view = self.buf.view(torch.float32)[1:rows + 1, :cols]

    def bits(self):
        b = self.buf.cpu().numpy()
        inside = np.zeros(b.shape, dtype=bool)
        inside[1:self.rows + 1, :self.cols] = True
        assert (b[~inside] == SENT32).all(), "a store left the output (pitch padding or guard rows)"
        return b[1:self.rows + 1, :self.cols].copy()


def run_both(case, o1, o2, table, y, g):
    """The table entry points and, on the same device inputs, the existing pair on the materialised gather.  Bit patterns (int32)."""
    B, C, layout = case
    i1, i2, tab = place(o1, layout), place(o2, layout), place(table, layout)
    ld = pitch(layout, C)
    yd = torch.from_numpy(np.asarray(y, dtype=np.int64)).cuda()
    gd = torch.from_numpy(g).cuda()
    n_aux = call("se_labelembed_aux_floats", B)
    out = {}
    # --- the composition the table path replaces
    tar = torch.from_numpy(table[np.clip(y, 0, C - 1)]).cuda()
    loss, aux = torch.zeros(B, device="cuda"), torch.zeros(n_aux, device="cuda")
    call("se_labelembed_loss_fwd", i1, ld, i2, ld, tar, C, yd, B, C, TAU, ALPHA, BETA, loss, aux)
    d = [torch.zeros((B, C), device="cuda") for _ in range(3)]
    call("se_labelembed_loss_bwd", i1, ld, i2, ld, tar, C, yd, gd, 0.0, B, C, TAU, ALPHA, BETA, aux, d[0], C, d[1], C, d[2], C)
    out["ref"] = dict(loss=loss, aux=aux[:B * AUX + 1], d1=d[0], d2=d[1], dtar=d[2])
    # --- the table path, into guarded outputs with pitch padding
    loss_t, aux_t = torch.zeros(B, device="cuda"), torch.zeros(n_aux, device="cuda")
    call("se_labelembed_table_loss_fwd", i1, ld, i2, ld, tab, ld, yd, B, C, TAU, ALPHA, BETA, loss_t, aux_t)
    g1, g2, gt = Guarded(B, C, C + 3), Guarded(B, C, C + 3), Guarded(C, C, C + 3)
    call("se_labelembed_table_loss_bwd", i1, ld, i2, ld, tab, ld, yd, gd, 0.0, B, C, TAU, ALPHA, BETA, aux_t, g1.view, C + 3, g2.view,
         C + 3, gt.view, C + 3)
    torch.cuda.synchronize()
    out["ref"] = {k: v.cpu().numpy().view(np.int32) for k, v in out["ref"].items()}
    out["table"] = dict(loss=loss_t.cpu().numpy().view(np.int32), aux=aux_t[:B * AUX + 1].cpu().numpy().view(np.int32), d1=g1.bits(),
                        d2=g2.bits(), dtab=gt.bits())
    return out


_RESULTS = {}


def results(case):
    """One run per case, shared by the bit-contract and the oracle tests."""
    if case not in _RESULTS:
        _RESULTS[case] = run_both(case, *case_inputs(case))
    return _RESULTS[case]


IDS = ["B%d-C%d-%s" % c for c in TABLE_CASES]


@pytest.mark.parametrize("case", TABLE_CASES, ids=IDS)
def test_bit_contracts(case):
    B, C, layout = case
    o1, o2, table, y, g = case_inputs(case)
    r = results(case)
    ref, tab = r["ref"], r["table"]
    for k in ("loss", "aux", "d1", "d2"):
        assert np.array_equal(tab[k], ref[k]), k
    assert np.isfinite(tab["loss"].view(np.float32)).all()
    want = table_grad_rule(ref["dtar"].view(np.float32), y, C)
    assert np.array_equal(tab["dtab"], want.view(np.int32))
    absent = np.setdiff1d(np.arange(C), np.clip(y, 0, C - 1))
    assert (tab["dtab"][absent] == 0).all()                                     # +0, not -0
    if B > 1:
        assert np.abs(want).max() > 0
    # out-of-range labels are the clamped labels
    rc = run_both(case, o1, o2, table, np.clip(y, 0, C - 1), g)["table"]
    for k in tab:
        assert np.array_equal(rc[k], tab[k]), k


@pytest.mark.parametrize("every_third_out", [False, True], ids=["all-rows-count", "every-third-row-wt0"])
def test_table_grad_group_boundaries(every_third_out):
    """Labels that fix how many rows of a class every ballot of 64 holds (1 ... 9: one, two and three groups of four with every
    remainder, and a partial last ballot).  Every row's true class wins out2 (mask = 1, all rows count); in the second run every
    third row's true class loses it instead, so that rows with wt == 0 sit inside the groups and are skipped."""
    B, C = 300, GROUP_CLASSES
    rng = np.random.default_rng(43)
    y = scan_group_labels(B, rng)
    o1, o2 = (rng.standard_normal((B, C)).astype(np.float32) * 2 for _ in range(2))
    table = (np.eye(C) + 0.5 * rng.standard_normal((C, C))).astype(np.float32)
    g = rng.standard_normal(B).astype(np.float32)
    counts = np.ones(B, dtype=bool)
    if every_third_out:
        counts[::3] = False
    rows = np.arange(B)
    o2[rows[counts], y[counts]] = o2.max(axis=1)[counts] + 7.0
    o2[rows[~counts], y[~counts]] -= 30.0
    r = run_both((B, C, PADDED), o1, o2, table, y, g)
    ref, tab = r["ref"], r["table"]
    mask = ref["aux"].view(np.float32)[:B * AUX].reshape(B, AUX)[:, 4]
    assert np.array_equal(mask != 0, counts)
    want = table_grad_rule(ref["dtar"].view(np.float32), y, C)
    assert (want[:9] != 0).any(axis=1).all()
    assert np.array_equal(tab["dtab"], want.view(np.int32))


def test_no_row_with_mask_one():
    """No sample is classified correctly by out2: the batch scale is B / 1e-8, every wt_i is +-0, d_table is all +0 and the loss finite."""
    case = NO_MASK_CASE
    B, C, _ = case
    o1, o2, table, y, g = case_inputs(case, all_masked_out=True)
    r = run_both(case, o1, o2, table, y, g)
    ref, tab = r["ref"], r["table"]
    aux = tab["aux"].view(np.float32)
    assert not aux[:B * AUX].reshape(B, AUX)[:, 4].any() and aux[B * AUX] == np.float32(B) / np.float32(1e-8)
    assert np.isfinite(tab["loss"].view(np.float32)).all()
    for k in ("loss", "aux", "d1", "d2"):
        assert np.array_equal(tab[k], ref[k]), k
    assert (tab["dtab"] == 0).all()
    assert np.array_equal(tab["dtab"], table_grad_rule(ref["dtar"].view(np.float32), y, C).view(np.int32))


def test_empty_batch_writes_a_zero_table_gradient():
    C = 70
    gt = Guarded(C, C, C + 3)
    call("se_labelembed_table_loss_bwd", None, C, None, C, None, C, None, None, 1.0, 0, C, TAU, ALPHA, BETA, None, None, 0, None, 0,
         gt.view, C + 3)
    torch.cuda.synchronize()
    assert (gt.bits() == 0).all()


@pytest.mark.parametrize("case", TABLE_CASES, ids=IDS)
def test_against_the_float64_oracle(case):
    """oracle/loss_oracle.py in float64 on the gathered rows.  Loss within 1e-4 max(1, |want|), logit gradients within
    1e-5 max(1, |ref|) (the tolerances of tests/test_gpu_loss.py).  d_table against np.add.at of the oracle's d_tar: each of the n_k
    rows of class k carries the per-row gradient bound e = 1e-5 max(1, |d_tar|), and adding n_k float32 terms one by one rounds
    n_k - 1 times, each by at most 2^-24 of a partial sum that is at most sum |terms|: n_k e + n_k 2^-24 sum_i |d_tar[i, c]|."""
    B, C, layout = case
    o1, o2, table, y, g = case_inputs(case)
    yc = np.clip(y, 0, C - 1)
    tab = results(case)["table"]
    want = lo.labelembed_loss(o1, o2, table[yc], yc, tau=TAU, alpha=ALPHA, beta=BETA)
    got = tab["loss"].view(np.float32)
    print("loss err", np.abs(got - want).max(), "bound", 1e-4 * max(1.0, np.abs(want).max()))
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    d1, d2, dt = lo.labelembed_loss_bwd(o1, o2, table[yc], yc, g, tau=TAU, alpha=ALPHA, beta=BETA)
    for k, ref in (("d1", d1), ("d2", d2)):
        err = np.abs(tab[k].view(np.float32) - ref).max()
        print(k, "err", err, "bound", 1e-5 * max(1.0, np.abs(ref).max()))
        assert err <= 1e-5 * max(1.0, np.abs(ref).max()), k
    e = 1e-5 * max(1.0, np.abs(dt).max())
    ref_tab, sum_abs = np.zeros((C, C)), np.zeros((C, C))
    np.add.at(ref_tab, yc, dt)
    np.add.at(sum_abs, yc, np.abs(dt))
    n_k = np.bincount(yc, minlength=C).astype(np.float64)[:, None]
    bound = n_k * e + n_k * U * sum_abs
    err = np.abs(tab["dtab"].view(np.float32) - ref_tab)
    print("dtab err", err.max(), "smallest slack", (bound - err).min())
    assert (err <= bound).all()


def _inputs_on_device(case):
    o1, o2, table, y, g = case_inputs(case)
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (o1, o2, table)] + \
        [torch.from_numpy(y.astype(np.int64)).cuda(), torch.from_numpy(g).cuda()]


def test_determinism_repeats_and_busy_second_stream():
    import sehip
    case = TABLE_CASES[4]
    B, C, _ = case
    o1, o2, table, y, g = _inputs_on_device(case)
    n_aux = call("se_labelembed_aux_floats", B)

    def once():
        loss, aux = torch.zeros(B, device="cuda"), torch.zeros(n_aux, device="cuda")
        d1, d2, dtab = torch.empty((B, C), device="cuda"), torch.empty((B, C), device="cuda"), torch.empty((C, C), device="cuda")
        call("se_labelembed_table_loss_fwd", o1, C, o2, C, table, C, y, B, C, TAU, ALPHA, BETA, loss, aux)
        call("se_labelembed_table_loss_bwd", o1, C, o2, C, table, C, y, g, 0.0, B, C, TAU, ALPHA, BETA, aux, d1, C, d2, C, dtab, C)
        return loss, d1, d2, dtab

    first, second = once(), once()
    feats = torch.randn(4096, 128, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(10):
            sehip.pairwise_dist(feats, None, metric=sehip.METRIC_DOT)          # an unrelated kernel of the library
    busy = once()
    torch.cuda.synchronize()
    for other in (second, busy):
        for a, b in zip(first, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_graph_capture_replays_bit_equal_to_eager():
    """Forward + backward of the op inside torch.cuda.graph (no synchronisation, no workspace); the process keeps the hardware-queue
    count it was started with."""
    import sehip
    case = TABLE_CASES[2]
    o1, o2, table, y, _ = _inputs_on_device(case)
    o1.requires_grad_(True); o2.requires_grad_(True)
    table = torch.nn.Parameter(table)

    def step():
        o1.grad = o2.grad = table.grad = None
        loss = sehip.labelembed_table_loss(o1, o2, table, y, tau=TAU, alpha=ALPHA, beta=BETA).mean()
        loss.backward()
        return loss

    eager = step().detach().clone()
    want = [t.grad.clone() for t in (o1, o2, table)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    o1.grad = o2.grad = table.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gl.view(torch.int32), eager.view(torch.int32))
        for t, w in zip((o1, o2, table), want):
            assert torch.equal(t.grad.view(torch.int32), w.view(torch.int32))


def test_op_on_the_halves_of_one_tensor_and_a_frozen_table(monkeypatch):
    import sehip
    case = TABLE_CASES[2]
    B, C, _ = case
    o1, o2, table, y, g = _inputs_on_device(case)
    a1, a2, ta = o1.clone().requires_grad_(True), o2.clone().requires_grad_(True), table.clone().requires_grad_(True)
    la = sehip.labelembed_table_loss(a1, a2, ta, y)
    la.backward(g)
    # the same logits as the column halves of one [B, 2 C] tensor: pitch 2 C, out2 off 16-byte alignment when C is odd
    wide = torch.cat((o1, o2), dim=1).requires_grad_(True)
    tb = table.clone().requires_grad_(True)
    lb = sehip.labelembed_table_loss(wide[:, :C], wide[:, C:], tb, y)
    lb.backward(g)
    # ... and the packed form, whose gradient is one buffer
    packed = torch.cat((o1, o2), dim=1).requires_grad_(True)
    tc = table.clone().requires_grad_(True)
    lc = sehip.labelembed_table_loss_packed(packed, tc, y)
    lc.backward(g)
    for loss, w, t in ((lb, wide, tb), (lc, packed, tc)):
        assert torch.equal(loss.view(torch.int32), la.view(torch.int32))
        assert torch.equal(w.grad[:, :C].view(torch.int32), a1.grad.view(torch.int32))
        assert torch.equal(w.grad[:, C:].contiguous().view(torch.int32), a2.grad.view(torch.int32))
        assert torch.equal(t.grad.view(torch.int32), ta.grad.view(torch.int32))
    assert float(ta.grad.abs().sum()) > 0
    # against the existing op on the gathered rows, whose d_tar rows torch's embedding backward adds up
    e1, e2, te = o1.clone().requires_grad_(True), o2.clone().requires_grad_(True), table.clone().requires_grad_(True)
    le = sehip.labelembed_loss(e1, e2, te[y.clamp(0, C - 1)], y)
    le.backward(g)
    assert torch.equal(le.view(torch.int32), la.view(torch.int32)) and torch.equal(e1.grad.view(torch.int32), a1.grad.view(torch.int32))
    assert torch.allclose(te.grad, ta.grad, rtol=1e-5, atol=1e-6)
    # needs_input_grad: a frozen table gets no gradient buffer, a frozen out2 neither
    seen = []
    real = sehip.ops.call
    monkeypatch.setattr(sehip.ops, "call", lambda name, *args: (seen.append((name, args)), real(name, *args))[1])
    f1, f2 = o1.clone().requires_grad_(True), o2.clone()
    sehip.labelembed_table_loss(f1, f2, table, y).backward(g)
    (name, args), = [s for s in seen if s[0] == "se_labelembed_table_loss_bwd"]
    assert args[15] is not None and args[17] is None and args[19] is None      # d_out1, d_out2, d_table
    assert table.grad is None and f2.grad is None
    assert torch.equal(f1.grad.view(torch.int32), a1.grad.view(torch.int32))
