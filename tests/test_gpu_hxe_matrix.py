"""GPU: every instantiation of csrc/hxe.hip -- hxe_fwd / hxe_bwd / soft_xent_fwd / soft_xent_bwd, 48 in all -- through the raw C ABI,
on the case tables of tests/test_hxe_matrix_host.py (which restates the host's choices and proves on the CPU that the tables reach
every instantiation, with a part-filled last unit and without, and every level count of a path from 0 to 32).

Every case owns its buffers: NaN in every pitch padding of the inputs, sentinels in and around every output (loss_i, best, above,
loss_mean, aux, dz, the padding columns of dz), so a store outside the output or a read of padding shows.  Accuracy is against the
float64 canon on the rounded inputs under the derived bounds of tests/test_gpu_hxe.py (_hxe_canon.loss_k / grad_factor /
soft_bounds, none restated or widened here); what the contract promises bit for bit is checked bit for bit: the metrics against
se_softmax_xent_fwd, a bf16 dz against the rounded float32 dz, repeats, a row alone against the row in its batch, labels outside
[0, C) against the clamped ones, NULL metric pointers, a power-of-two grad_scale -- and, for the backward kernels, which have no
reduction, the SAME dz bits from every layout, unit width and logits dtype of one problem.

SE_HXE_MATRIX_REPORT=<file> appends one line per case: the instantiations it ran and its worst error / bound."""
import os

import numpy as np
import pytest
import torch

import _hxe_canon as hc
import test_hxe_matrix_host as hm
from test_hxe_matrix_host import BF16, F32

pytestmark = pytest.mark.gpu
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
SENT32 = np.int32(0x7FC0DEAD)       # a quiet NaN with a payload no kernel writes
SENT16 = np.int16(0x7FAD)           # the same for bf16 outputs
GUARD = 16                          # guard elements before an output: a multiple of 16 bytes in every dtype
U = hc.U
_DEV = {}


def call(name, *args):
    from sehip._lib import call as c
    return c(name, *args)


def dev(a, dtype=None):
    """A host array on the device (through a copy: the shared references are read-only)."""
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def place(a, layout, dtype):
    """(view, pitch): the float32 matrix ``a`` on the device in ``dtype`` and ``layout``, NaN in every other element of its buffer."""
    rows, C = a.shape
    ld, off = hm.placement(layout, C, dtype)
    buf = torch.full((off + rows * ld + 8,), float("nan"), dtype=TORCH[dtype], device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + rows * ld].view(rows, ld)[:, :C]
    view.copy_(dev(a, np.float32).to(TORCH[dtype]))
    return view, ld


class Guarded(object):
    """A [rows, cols] output of pitch ``ld`` from element GUARD + ``off`` of a sentinel-filled buffer, GUARD + 8 elements behind."""

    def __init__(self, rows, cols, ld=None, off=0, dtype=torch.float32):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld or cols, dtype
        self.raw = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.sent = SENT16 if dtype == torch.bfloat16 else SENT32
        self.start = GUARD + off
        self.buf = torch.full((self.start + rows * self.ld + GUARD + 8,), int(self.sent), dtype=self.raw, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        view = self.buf[self.start:self.start + rows * self.ld].view(rows, self.ld)[:, :cols]
        self.out = view if dtype == torch.int32 else view.view(dtype)

    def untouched(self):
        return bool((self.buf == int(self.sent)).all())

    def read(self):
        """The output as float32 (bf16 widened: the same bits) or int32, after checking that every other element holds the sentinel."""
        b = self.buf.cpu().numpy()
        inside = np.zeros(b.shape, dtype=bool)
        for r in range(self.rows):
            inside[self.start + r * self.ld:self.start + r * self.ld + self.cols] = True
        assert (b[~inside] == self.sent).all(), "a store left the output (pitch padding or guard elements)"
        got = b[inside].reshape(self.rows, self.cols)
        if self.dtype == torch.bfloat16:
            return (got.astype(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
        return got.view(np.float32).copy() if self.dtype == torch.float32 else got.copy()


def device_encoding(name, pos_layout):
    """A tree's encoding on the device; ``pos`` 16-byte aligned, or a view one int32 into its buffer."""
    key = (name, pos_layout)
    if key not in _DEV:
        enc = hm.tree(name)[3]
        t = {k: dev(enc[k]) for k in ("path_off", "lvl_lo", "lvl_hi", "lvl_w")}
        C = len(enc["pos"])
        off = 1 if pos_layout == "offset" else 0
        buf = torch.full((C + 5,), -7, dtype=torch.int32, device="cuda")
        t["pos"] = buf[off:off + C]
        t["pos"].copy_(dev(enc["pos"]))
        assert (t["pos"].data_ptr() % 16 == 0) == (off == 0)
        t["host"] = torch.from_numpy(np.array(enc["path_off"]))
        t["depth"] = np.diff(enc["path_off"])
        _DEV[key] = t
    return _DEV[key]


def device_table(r, layout):
    """(view [C, C], ldt): the float32 table -- whole, or 0 but for the rows of the labels -- with NaN in its pitch padding."""
    C = r["C"]
    ldt, off = hm.placement(layout, C, F32)
    buf = torch.zeros((C, ldt), dtype=torch.float32, device="cuda")
    assert off == 0 and buf.data_ptr() % 16 == 0
    buf[:, C:] = float("nan")
    if r["table"] is not None:
        buf[:, :C].copy_(dev(r["table"]))
    else:
        buf[dev(r["y"], np.int64), :C] = dev(r["rows"])
    return buf[:, :C], ldt


class Hxe(object):
    """se_hxe_fwd / se_hxe_bwd on one problem's device inputs."""
    n_aux = hc.AUX

    def __init__(self, tree_name, third):
        self.t = device_encoding(tree_name, third)

    def fwd_call(self, zd, zdt, ld, yd, B, C, loss, aux, best, above, mean):
        t = self.t
        call("se_hxe_fwd", zd, zdt, ld, yd, t["pos"], t["path_off"], t["host"], t["lvl_lo"], t["lvl_hi"], t["lvl_w"], B, C, loss, aux,
             best, above, mean)

    def bwd_call(self, zd, zdt, ld, yd, aux, g, scale, B, C, dz, ddt, ldd):
        t = self.t
        call("se_hxe_bwd", zd, zdt, ld, yd, t["pos"], t["path_off"], t["host"], t["lvl_lo"], t["lvl_hi"], t["lvl_w"], aux, g, float(scale),
             B, C, dz, ddt, ldd)


class Soft(object):
    """se_soft_xent_fwd / se_soft_xent_bwd on one problem's device table."""
    n_aux = 3

    def __init__(self, r, third):
        self.table, self.ldt = device_table(r, third)

    def fwd_call(self, zd, zdt, ld, yd, B, C, loss, aux, best, above, mean):
        call("se_soft_xent_fwd", zd, zdt, ld, yd, self.table, self.ldt, B, C, loss, aux, best, above, mean)

    def bwd_call(self, zd, zdt, ld, yd, aux, g, scale, B, C, dz, ddt, ldd):
        call("se_soft_xent_bwd", zd, zdt, ld, yd, self.table, self.ldt, aux, g, float(scale), B, C, dz, ddt, ldd)


def forward(op, zd, zdt, ld, yd, best=True, above=True, mean=True):
    """One forward call into guarded outputs: dict of host arrays; ``aux_dev`` is the device aux for the backward."""
    B, C = zd.shape
    loss = Guarded(1, B)
    aux = Guarded(B, op.n_aux) if op.n_aux == hc.AUX else Guarded(1, 3 * B)
    gb, ga, gm = Guarded(1, B, dtype=torch.int32), Guarded(1, B, dtype=torch.int32), Guarded(1, 1)
    op.fwd_call(zd, zdt, ld, yd, B, C, loss.out, aux.out, gb.out if best else None, ga.out if above else None, gm.out if mean else None)
    torch.cuda.synchronize()
    for g, on in ((gb, best), (ga, above), (gm, mean)):
        assert on or g.untouched()
    return {"loss": loss.read()[0], "aux": aux.read(), "best": gb.read()[0], "above": ga.read()[0], "mean": gm.read()[0, 0],
            "aux_dev": aux.out}


def backward(op, zd, zdt, ld, yd, aux_dev, ddt, dlay, g=None, scale=1.0):
    """One backward call: dz [B, C] as float32 (a bf16 dz widened), its padding columns and guards checked."""
    B, C = zd.shape
    ldd, off = hm.placement(dlay, C, ddt)
    dz = Guarded(B, C, ldd, off, dtype=TORCH[ddt])
    op.bwd_call(zd, zdt, ld, yd, aux_dev, g, scale, B, C, dz.out, ddt, ldd)
    torch.cuda.synchronize()
    return dz.read()


def xent_metrics(zd, zdt, ld, yd):
    B, C = zd.shape
    loss, aux = torch.empty(B, device="cuda"), torch.empty(3 * B, device="cuda")
    best, above = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    call("se_softmax_xent_fwd", zd, zdt, ld, yd, B, C, 0.0, loss, aux, best, above, None)
    return best.cpu().numpy(), above.cpu().numpy()


def same_forward(a, b, rows=slice(None), aux_rows=None):
    return all(hm.same_bits(a[k][rows], b[k]) for k in ("loss", "best", "above")) and \
        hm.same_bits(a["aux"] if aux_rows is None else aux_rows, b["aux"])


def report(case, entries, rl, rg):
    path = os.environ.get("SE_HXE_MATRIX_REPORT")
    line = "%-58s %-34s %-40s loss err/bound %.3f  dz err/bound %.3f" % (hm.case_id(case), hm.inst_name(entries[0], case),
                                                                       hm.inst_name(entries[1], case), rl, rg)
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def run_case(case, r, op, compare, entries):
    """Everything a case checks (the module docstring); ``compare``: hm.compare_hxe / hm.compare_soft."""
    B, C, z, y, ref = r["B"], r["C"], r["z"], r["y"], r["ref"]
    hxe = op.n_aux == hc.AUX
    zd, ld = place(z, case.zlay, case.zdt)
    yd = dev(y, np.int64)
    args = (op, zd, case.zdt, ld, yd)
    f = forward(*args)
    if hxe:                                                 # aux: M, H_0 .. H_h, "the rest unused" -- still the sentinel
        depth = op.t["depth"][y]
        bits = f["aux"].view(np.int32)
        for i in range(B):
            assert np.isfinite(f["aux"][i, :2 + depth[i]]).all() and (bits[i, 2 + depth[i]:] == SENT32).all(), (i, depth[i])
    dz32 = backward(*args, f["aux_dev"], F32, case.dlay)
    rl, rg = compare(C, ref, f["loss"], dz32)               # the derived bounds; a row's dz sums to 0 within the summed bound
    dz = dz32
    if case.ddt == BF16:                                    # a bf16 dz is the float32 result, rounded to nearest even at the store
        dz = backward(*args, f["aux_dev"], BF16, case.dlay)
        assert hm.same_bits(dz, hm.bf16_round(dz32))
    xbest, xabove = xent_metrics(zd, case.zdt, ld, yd)      # the metrics of the cross-entropy kernel on the same buffer
    assert np.array_equal(f["best"], xbest) and np.array_equal(f["above"], xabove)
    fin = np.isfinite(f["loss"])
    if fin.all():
        got = f["loss"].astype(np.float64)
        assert abs(float(f["mean"]) - got.mean()) <= 10 * U * np.abs(got).mean()           # a tree of 8 additions and one division
    # a repeated call
    f2 = forward(*args)
    assert same_forward(f, f2) and hm.same_bits(np.float32(f["mean"]), np.float32(f2["mean"]))
    assert hm.same_bits(backward(*args, f2["aux_dev"], case.ddt, case.dlay), dz)
    # a row alone equals the row inside its batch: the rows of slots 0 .. 3 of the first workgroup, and the last row
    for i in sorted(set(range(min(B, 4))) | {B - 1}) if B > 1 else []:
        one = (op, zd[i:i + 1], case.zdt, ld, yd[i:i + 1].clone())
        f1 = forward(*one)
        assert same_forward(f, f1, slice(i, i + 1), f["aux"][i:i + 1] if hxe else f["aux"][:, i::B]), i
        assert hm.same_bits(backward(*one, f1["aux_dev"], case.ddt, case.dlay), dz[i:i + 1]), i
    # labels outside [0, C) are the clamped labels
    n = min(B, 2)
    outs = []
    for labels in ([-3, C + 5][:n], [0, C - 1][:n]):
        lab = (op, zd[:n], case.zdt, ld, torch.tensor(labels, dtype=torch.int64, device="cuda"))
        fl = forward(*lab)
        outs.append((fl, backward(*lab, fl["aux_dev"], case.ddt, case.dlay)))
    assert same_forward(outs[0][0], outs[1][0]) and hm.same_bits(outs[0][1], outs[1][1])
    # best, above, loss_mean each NULL: every other output keeps its bits
    for k, kw in enumerate(({"best": False}, {"above": False}, {"mean": False})):
        fn = forward(*args, **kw)
        assert all(hm.same_bits(f[name], fn[name]) for name in ("loss", "aux")), kw
        assert all(hm.same_bits(np.asarray(f[name]), np.asarray(fn[name])) for j, name in enumerate(("best", "above", "mean")) if j != k), kw
    # grad_scale a power of two is the scaled dz; grad_loss_i weights the rows under the weighted bound
    assert hm.same_bits(backward(*args, f["aux_dev"], case.ddt, case.dlay, scale=0.25), dz * np.float32(0.25))
    w = np.linspace(-1.5, 2.0, B).astype(np.float32)
    dzw = backward(*args, f["aux_dev"], F32, case.dlay, g=dev(w)).astype(np.float64)
    wn = np.abs(w.astype(np.float64))[:, None]
    gb = hm.grad_bound(C, ref) if hxe else hc.soft_bounds(C, ref)[1]
    with np.errstate(invalid="ignore"):
        wb = np.where(gb == 0, 0.0, wn * gb)
    assert (np.abs(dzw - w.astype(np.float64)[:, None] * ref["dz"]) <= wb + 1e-300).all()
    report(case, entries, rl, rg)


@pytest.mark.parametrize("case", hm.HXE_CASES, ids=[hm.case_id(c) for c in hm.HXE_CASES])
def test_hxe_instantiations_against_the_canon(case):
    r = hm.hxe_reference(case.problem, case.zdt)
    run_case(case, r, Hxe(hm.HXE_PROBLEMS[case.problem].tree, case.third), hm.compare_hxe, hm.ENTRIES[:2])


@pytest.mark.parametrize("case", hm.SOFT_CASES, ids=[hm.case_id(c) for c in hm.SOFT_CASES])
def test_soft_label_instantiations_against_the_canon(case):
    r = hm.soft_reference(case.problem, case.zdt)
    run_case(case, r, Soft(r, case.third), hm.compare_soft, hm.ENTRIES[2:])


LAYOUTS = ("contig", "pad16", "odd", "off1")


@pytest.mark.parametrize("problem", ["c1", "rand8", "cat33", "cat33x1000", "rand1032", "s9", "sinf100", "s1024", "s1025", "s1032"])
def test_backward_bits_do_not_depend_on_the_form(problem):
    """Given the SAME aux, dz of one logical problem (logits that bf16 holds exactly) is bit-equal across both logits dtypes, every
    layout of the logits, of dz and of pos / the table -- 16-byte against scalar units, E = 4 against E = 8: a wrong lane map or a
    dropped tail unit in one form is a bit difference."""
    hxe = problem in hm.HXE_PROBLEMS
    r = (hm.hxe_reference if hxe else hm.soft_reference)(problem, BF16)
    B, C = r["B"], r["C"]
    yd = dev(r["y"], np.int64)
    thirds = ("aligned", "offset") if hxe else ("contig", "pad16", "odd")
    ops = {t: (Hxe(hm.HXE_PROBLEMS[problem].tree, t) if hxe else Soft(r, t)) for t in thirds}
    zd, ld = place(r["z"], "contig", F32)
    aux = forward(ops[thirds[0]], zd, F32, ld, yd)["aux_dev"]
    first, reached = None, set()
    for zdt in (F32, BF16):
        for zlay in LAYOUTS:
            zd, ld = place(r["z"], zlay, zdt)
            for dlay in LAYOUTS:
                for third in thirds:
                    for ddt in (F32, BF16):
                        form = hm.Case(problem, C, B, zdt, ddt, zlay, dlay, third)
                        reached.add(hm.instantiation("hxe_bwd" if hxe else "soft_bwd", form))
                        dz = backward(ops[third], zd, zdt, ld, yd, aux, ddt, dlay)
                        if first is None:
                            first = dz
                        hm.compare_layout_bits([first if ddt == F32 else hm.bf16_round(first), dz])
    assert reached == {i for i in hm.all_instantiations("hxe_bwd") if i[-1] == hm.path_of(C)}
    (hm.compare_hxe if hxe else hm.compare_soft)(C, r["ref"], forward(ops[thirds[0]], zd, BF16, ld, yd)["loss"], first)
