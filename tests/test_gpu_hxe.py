"""GPU: the hierarchy-aware classifier losses -- se_hxe_fwd / _bwd and se_soft_xent_fwd / _bwd against the float64 canon
(tests/_hxe_canon.py, which knows nothing of the range encoding), against se_softmax_xent where the losses coincide, their metrics,
determinism, numerical edges, the autograd ops (HIP-graph capture included) and learn_classifier.py --loss hxe / soft_labels.

The error bounds (u = 2^-24; every quantity is a float32 kernel value against the float64 canon ON THE ROUNDED INPUTS)
---------------------------------------------------------------------------------------------------------------------
A level sum S = sum of e_c = expf(z_c - M) over a range, L = logf(S):
  * z_c - M is rounded once: x_c (1 + d), |d| <= u, changes e_c by the factor exp(x_c d); on the sum that is at most
    u sum_c p_c |x_c| with p_c = e_c / S, and x_c = log p_c + L gives sum_c p_c |x_c| <= |L| + ln C;
  * expf within 2 ulp: 4 u relative on every e_c, so on S;
  * the fixed-order sum of positive values: D u relative, D = the additions on its longest path (_hxe_canon.sum_depth: a thread's
    own values in order, 6 butterfly steps, 2 steps across the waves);
  * logf within 2 ulp: 4 u |L|.
  So |dL| <= u (5 |L| + ln C + 4 + D); L_0 = z_y - M is one rounding, u |L_0|.
HXE loss = sum_l lambda_l (L_{l+1} - L_l): the two logs of a term, its subtraction and its product (u (|L_l| + |L_{l+1}|) each), and
the 6-step tree over the terms (6 u (|L_l| + |L_{l+1}|) lambda_l): at most
      u sum_l lambda_l [13 (|L_l| + |L_{l+1}|) + 2 (ln C + 4 + D)]  <=  k u sum_l lambda_l (|L_l| + |L_{l+1}| + 1),
      k = 13 + 2 (ln C + 4 + D)                                                                  (_hxe_canon.loss_k)
(the float32 weights lambda are inputs: the canon takes them rounded).
HXE gradient dz_c = w (e_c H_lev(c) - [c == y] lambda_0), H_k = sum_{j >= max(k, 1)} (lambda_{j-1} - lambda_j) / S_j: e_c carries
(|x_c| + 4) u; 1 / S_j carries (|L_j| + ln C + 4 + D + 1) u with |L_j| <= max(|x_c|, ln C) because e_c <= S_j <= C for every j the
element belongs to; the difference of the weights, the product and the 5-step suffix scan 7 u more; the last product and
subtraction 3 u.  With a_c = the closed form with every term taken positive (so that e_c |lambda_{j-1} - lambda_j| / S_j summed
over j is at most a_c):
      |d dz_c| <= u |w| (2 |x_c| + 2 ln C + D + 20) a_c                                          (_hxe_canon.grad_factor)
Soft labels, loss = sum_c Q_c (M - z_c) + (sum_c Q_c) log S: the same ingredients give at most
      (D + ln C + 10) u sum_c Q_c (|M - z_c| + |log S| + 1)      and      |d dz_k| <= u |w| (2 |x_k| + 7 ln C + 2 D + 12) (sum(Q) p_k + Q_k).
A bf16 dz is the bf16 rounding of the float32 result, bit for bit (the same arithmetic, rounded at the store).
An excess over these bounds is a finding to explain, not a reason to widen them."""
import json
import os

import numpy as np
import pytest
import torch

import _hxe_canon as hc
from test_class_embedding_host import load_hierarchy

pytestmark = pytest.mark.gpu
U = hc.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_TREES = {}


def _hierarchy(edges):
    from class_hierarchy import ClassHierarchy
    parents, children = {}, {}
    for p, c in edges:
        parents.setdefault(c, []).append(p)
        children.setdefault(p, []).append(c)
    return ClassHierarchy(parents, children)


def tree(name):
    """(hierarchy, classes, canon) of a named tree, built once."""
    if name not in _TREES:
        if name == "c2":
            h, classes = _hierarchy([(10, 0), (10, 1)]), [0, 1]
        elif name == "c3":
            h, classes = _hierarchy([(10, 0), (10, 11), (11, 1), (11, 2)]), [0, 1, 2]
        elif name.startswith("rand"):
            h, classes = hc.random_tree(int(name[4:]), seed=int(name[4:]))
        else:
            h, classes = load_hierarchy(name)
        _TREES[name] = (h, classes, hc.Canon(h, classes))
    return _TREES[name]


def encoding(name, alpha=0.1):
    import sehip
    key = (name, alpha)
    if key not in _TREES:
        h, classes, _ = tree(name)
        _TREES[key] = sehip.HxeEncoding(h.hxe_encoding(classes, alpha=alpha))
    return _TREES[key]


def logits(B, C, dtype, seed, spread=4.0, pitch=None):
    """Device logits [B, C] (a view of a [B, pitch] buffer), |z| <= 40, and their float64 values."""
    rng = np.random.default_rng(seed)
    z = np.clip(rng.standard_normal((B, C)) * spread, -40.0, 40.0).astype(np.float32)
    buf = torch.zeros((B, pitch or C), dtype=dtype, device="cuda")
    zd = buf[:, :C]
    zd.copy_(torch.from_numpy(z))
    y = rng.integers(0, C, size=B)
    return zd, torch.from_numpy(y).cuda(), zd.float().cpu().numpy().astype(np.float64), y


def _code(t):
    return 1 if t.dtype == torch.bfloat16 else 0


def hxe_fwd(zd, yd, enc, mean=False):
    from sehip._lib import call
    B, C = zd.shape
    t = enc.on(zd.device)
    loss = torch.empty(B, device="cuda")
    aux = torch.empty(call("se_hxe_aux_floats", B), device="cuda")
    best, above = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    lm = torch.empty(1, device="cuda") if mean else None
    call("se_hxe_fwd", zd, _code(zd), max(zd.stride(0), C), yd, t["pos"], t["path_off"], enc.host["path_off"], t["lvl_lo"], t["lvl_hi"],
         t["lvl_w"], B, C, loss, aux, best, above, lm)
    return (loss, aux, best, above) + ((lm,) if mean else ())


def hxe_bwd(zd, yd, enc, aux, g=None, scale=1.0, dtype=torch.float32, pitch=None):
    from sehip._lib import call
    B, C = zd.shape
    t = enc.on(zd.device)
    dz = torch.zeros((B, pitch or C), dtype=dtype, device="cuda")[:, :C]
    call("se_hxe_bwd", zd, _code(zd), max(zd.stride(0), C), yd, t["pos"], t["path_off"], enc.host["path_off"], t["lvl_lo"], t["lvl_hi"],
         t["lvl_w"], aux, g, float(scale), B, C, dz, _code(dz), max(dz.stride(0), C))
    return dz


def soft_fwd(zd, yd, table):
    from sehip._lib import call
    B, C = zd.shape
    loss, aux = torch.empty(B, device="cuda"), torch.empty(3 * B, device="cuda")
    best, above = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    call("se_soft_xent_fwd", zd, _code(zd), max(zd.stride(0), C), yd, table, table.stride(0), B, C, loss, aux, best, above, None)
    return loss, aux, best, above


def soft_bwd(zd, yd, table, aux, g=None, scale=1.0, dtype=torch.float32):
    from sehip._lib import call
    B, C = zd.shape
    dz = torch.zeros((B, C), dtype=dtype, device="cuda")
    call("se_soft_xent_bwd", zd, _code(zd), max(zd.stride(0), C), yd, table, table.stride(0), aux, g, float(scale), B, C, dz, _code(dz), C)
    return dz


def xent(zd, yd, smoothing=0.0, want_dz=False):
    from sehip._lib import call
    B, C = zd.shape
    loss, aux = torch.empty(B, device="cuda"), torch.empty(3 * B, device="cuda")
    best, above = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    call("se_softmax_xent_fwd", zd, _code(zd), max(zd.stride(0), C), yd, B, C, float(smoothing), loss, aux, best, above, None)
    if not want_dz:
        return loss, best, above
    dz = torch.zeros((B, C), device="cuda")
    call("se_softmax_xent_bwd", zd, _code(zd), max(zd.stride(0), C), yd, aux, None, 1.0, B, C, float(smoothing), dz, 0, C)
    return loss, best, above, dz


def grad_bound(C, ref, w=1.0):
    with np.errstate(invalid="ignore"):
        return np.where(ref["absgrad"] == 0, 0.0, U * abs(w) * hc.grad_factor(C, ref["x"]) * ref["absgrad"])


# name, B, logits dtype, row pitch of logits and dz (None: C), spread
CASES = [
    ("c2", 5, torch.float32, None, 4.0),            # h = 1
    ("c3", 5, torch.float32, None, 4.0),            # unbalanced: h = 1 and h = 2
    ("c3", 1, torch.bfloat16, None, 4.0),
    ("cifar", 32, torch.float32, None, 4.0),        # depths 3 .. 9, chains dropped
    ("cifar", 5, torch.bfloat16, None, 4.0),
    ("cifar", 5, torch.float32, 103, 15.0),         # C no multiple of 8 on a pitch that is not 16-byte aligned: scalar loads
    ("cifar", 1, torch.bfloat16, 101, 15.0),
    ("ilsvrc", 32, torch.float32, None, 4.0),       # 16 kept levels
    ("ilsvrc", 1, torch.bfloat16, None, 15.0),
    ("rand1024", 5, torch.float32, None, 4.0),      # the last C of the wave-per-row kernels
    ("rand1025", 5, torch.float32, 1028, 4.0),      # the first C of the workgroup-per-row kernels, 16-byte pitch, a part-filled last unit
    ("rand1025", 5, torch.bfloat16, 1032, 4.0),
    ("rand1027", 5, torch.float32, 1029, 4.0),      # workgroup per row, scalar loads
    ("rand1021", 5, torch.bfloat16, 1023, 4.0),     # wave per row, scalar loads, bf16
    ("inat2018", 8, torch.float32, 8144, 4.0),      # C = 8142 on a 16-byte pitch: 32 values per thread, a part-filled last unit
]


@pytest.mark.parametrize("name,B,dtype,pitch,spread", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_hxe_against_the_canon(name, B, dtype, pitch, spread):
    h, classes, canon = tree(name)
    C = len(classes)
    enc = encoding(name)
    zd, yd, z64, y = logits(B, C, dtype, seed=C + B, spread=spread, pitch=pitch)
    ref = canon.hxe(z64, y, alpha=0.1)
    loss, aux, best, above, mean = hxe_fwd(zd, yd, enc, mean=True)
    got = loss.cpu().numpy().astype(np.float64)
    bound = hc.loss_k(C) * U * ref["scale"]
    err = np.abs(got - ref["loss"])
    print("loss: max err %.3g, max err / bound %.3g (k = %.1f)" % (err.max(), (err / bound).max(), hc.loss_k(C)))
    assert (err <= bound).all(), (err, bound)
    # the metrics are those of the cross-entropy kernel on the same logits, bit for bit; the mean is launch_mean's
    _, xbest, xabove = xent(zd, yd)
    assert torch.equal(best, xbest) and torch.equal(above, xabove)
    assert abs(float(mean) - float(got.mean())) <= 10 * U * float(np.abs(got).mean())     # a tree of 8 additions and one division

    dz = hxe_bwd(zd, yd, enc, aux, pitch=pitch)
    gb = grad_bound(C, ref)
    gerr = np.abs(dz.cpu().numpy().astype(np.float64) - ref["dz"])
    print("dz: max err %.3g, max err / bound %.3g" % (gerr.max(), (gerr / np.maximum(gb, 1e-300)).max()))
    assert (gerr <= gb).all()
    assert (np.abs(dz.cpu().numpy().astype(np.float64).sum(axis=1)) <= gb.sum(axis=1)).all()          # a row's gradients sum to 0
    dz16 = hxe_bwd(zd, yd, enc, aux, dtype=torch.bfloat16, pitch=pitch)
    assert torch.equal(dz16, dz.to(torch.bfloat16))                 # bf16 dz: the float32 result, rounded at the store

    # the same bits again; and a row's bits do not depend on the batch around it
    loss2, aux2, _, _ = hxe_fwd(zd, yd, enc)
    assert torch.equal(loss2, loss) and torch.equal(hxe_bwd(zd, yd, enc, aux2, pitch=pitch), dz)
    i = B - 1
    l1, a1, b1, ab1 = hxe_fwd(zd[i:i + 1], yd[i:i + 1].contiguous(), enc)
    assert torch.equal(l1, loss[i:i + 1]) and b1[0] == best[i] and ab1[0] == above[i]
    assert torch.equal(hxe_bwd(zd[i:i + 1], yd[i:i + 1].contiguous(), enc, a1), dz[i:i + 1])

    # grad_loss_i weights the rows, grad_scale all of them
    w = torch.linspace(-1.5, 2.0, B, device="cuda")
    dzw = hxe_bwd(zd, yd, enc, aux, g=w).cpu().numpy().astype(np.float64)
    wn = w.cpu().numpy().astype(np.float64)
    assert (np.abs(dzw - wn[:, None] * ref["dz"]) <= np.abs(wn)[:, None] * gb + 1e-300).all()
    assert torch.equal(hxe_bwd(zd, yd, enc, aux, scale=0.25), (dz * 0.25))      # a power of two: exact


@pytest.mark.parametrize("name,B,dtype", [("cifar", 32, torch.float32), ("rand1025", 5, torch.bfloat16), ("c3", 5, torch.float32)])
def test_alpha_zero_is_the_cross_entropy(name, B, dtype):
    h, classes, canon = tree(name)
    C = len(classes)
    enc = encoding(name, alpha=0.0)
    assert (enc.host["lvl_w"] == 1.0).all()
    zd, yd, z64, y = logits(B, C, dtype, seed=7, spread=2.0)
    ref = canon.hxe(z64, y, alpha=0.0)
    loss, aux, best, above = hxe_fwd(zd, yd, enc)
    xl, xbest, xabove, xdz = xent(zd, yd, want_dz=True)
    ce = -hc.log_softmax(z64)[np.arange(B), y]
    inside = (ce > 1e-6) & (ce < 16.0)                              # strictly inside Keras' clip [1.19e-7, 16.118]
    assert inside.sum() >= max(1, B // 2)
    bound = hc.loss_k(C) * U * ref["scale"]
    d = np.abs(loss.cpu().numpy().astype(np.float64) - xl.cpu().numpy().astype(np.float64))
    print("alpha = 0 vs se_softmax_xent: max |d loss| / bound %.3g" % (d[inside] / bound[inside]).max())
    assert (d[inside] <= bound[inside]).all()
    assert torch.equal(best, xbest) and torch.equal(above, xabove)
    dz = hxe_bwd(zd, yd, enc, aux).cpu().numpy().astype(np.float64)
    gb = grad_bound(C, ref)
    assert (np.abs(dz - xdz.cpu().numpy().astype(np.float64))[inside] <= gb[inside]).all()
    assert (np.abs(dz - (np.exp(hc.log_softmax(z64)) - np.eye(C)[y])) <= gb).all()        # p - onehot


_soft_bounds = hc.soft_bounds          # one copy, shared with tests/test_gpu_hxe_matrix.py


@pytest.mark.parametrize("name,B,dtype,ldt", [("cifar", 32, torch.float32, None), ("cifar", 5, torch.bfloat16, 101),
                                              ("ilsvrc", 5, torch.float32, None), ("rand1025", 5, torch.float32, None),
                                              ("c2", 1, torch.float32, None)], ids=lambda v: str(v).replace("torch.", ""))
def test_soft_labels_against_the_canon(name, B, dtype, ldt):
    h, classes, canon = tree(name)
    C = len(classes)
    table = h.soft_label_table(classes, 10.0)
    td = torch.zeros((C, ldt or C), device="cuda")[:, :C]
    td.copy_(torch.from_numpy(table))
    zd, yd, z64, y = logits(B, C, dtype, seed=11 + C, spread=4.0)
    ref = hc.soft(z64, y, table)
    lb, gb = _soft_bounds(C, ref)
    loss, aux, best, above = soft_fwd(zd, yd, td)
    err = np.abs(loss.cpu().numpy().astype(np.float64) - ref["loss"])
    print("soft loss: max err / bound %.3g" % (err / lb).max())
    assert (err <= lb).all()
    _, xbest, xabove = xent(zd, yd)
    assert torch.equal(best, xbest) and torch.equal(above, xabove)
    dz = soft_bwd(zd, yd, td, aux)
    gerr = np.abs(dz.cpu().numpy().astype(np.float64) - ref["dz"])
    print("soft dz: max err / bound %.3g" % (gerr / np.maximum(gb, 1e-300)).max())
    assert (gerr <= gb).all()
    assert torch.equal(soft_bwd(zd, yd, td, aux, dtype=torch.bfloat16), dz.to(torch.bfloat16))
    loss2, aux2, _, _ = soft_fwd(zd, yd, td)
    assert torch.equal(loss2, loss) and torch.equal(soft_bwd(zd, yd, td, aux2), dz)
    i = B - 1
    l1, a1, _, _ = soft_fwd(zd[i:i + 1], yd[i:i + 1].contiguous(), td)
    assert torch.equal(l1, loss[i:i + 1]) and torch.equal(soft_bwd(zd[i:i + 1], yd[i:i + 1].contiguous(), td, a1), dz[i:i + 1])
    w = torch.linspace(-1.0, 3.0, B, device="cuda")
    wn = w.cpu().numpy().astype(np.float64)
    dzw = soft_bwd(zd, yd, td, aux, g=w).cpu().numpy().astype(np.float64)
    assert (np.abs(dzw - wn[:, None] * ref["dz"]) <= np.abs(wn)[:, None] * gb + 1e-300).all()
    assert torch.equal(soft_bwd(zd, yd, td, aux, scale=0.5), dz * 0.5)


def test_one_hot_and_smoothed_tables_meet_the_other_kernels():
    h, classes, canon = tree("cifar")
    C, B = 100, 32
    zd, yd, z64, y = logits(B, C, torch.float32, seed=3, spread=1.0)
    # a one-hot table is the alpha = 0 HXE
    eye = torch.eye(C, device="cuda")
    sl, saux, _, _ = soft_fwd(zd, yd, eye)
    hl, haux, _, _ = hxe_fwd(zd, yd, encoding("cifar", alpha=0.0))
    ref = canon.hxe(z64, y, alpha=0.0)
    assert (np.abs((sl - hl).cpu().numpy().astype(np.float64)) <= hc.loss_k(C) * U * ref["scale"]).all()
    gb = grad_bound(C, ref)
    assert (np.abs((soft_bwd(zd, yd, eye, saux) - hxe_bwd(zd, yd, encoding("cifar", alpha=0.0), haux)).cpu().numpy()) <= gb).all()
    # a label-smoothing table is se_softmax_xent with that smoothing, where no class leaves Keras' clip
    s = 0.1
    smooth = np.full((C, C), np.float32(s / (C - 1)), dtype=np.float32)
    np.fill_diagonal(smooth, np.float32(1.0 - s))
    t = -hc.log_softmax(z64)
    assert t.max() < 16.0 and t.min() > 1e-6
    sref = hc.soft(z64, y, smooth)
    lb, sgb = _soft_bounds(C, sref)
    td = torch.from_numpy(smooth).cuda()
    sl, saux, _, _ = soft_fwd(zd, yd, td)
    xl, _, _, xdz = xent(zd, yd, smoothing=s, want_dz=True)
    assert (np.abs((sl - xl).cpu().numpy().astype(np.float64)) <= lb).all()
    assert (np.abs((soft_bwd(zd, yd, td, saux) - xdz).cpu().numpy().astype(np.float64)) <= sgb).all()


def test_metrics_of_special_rows_are_the_cross_entropy_kernels():
    """Ties, NaN rows, +inf rows and rows of nothing but -inf: best / above bit-equal to se_softmax_xent_fwd's, loss and dz NaN where
    that kernel's are, and the rows next to them untouched."""
    h, classes, canon = tree("cifar")
    C = 100
    enc = encoding("cifar")
    table = torch.from_numpy(h.soft_label_table(classes, 10.0)).cuda()
    zd, yd, z64, y = logits(8, C, torch.float32, seed=21)
    clean = zd.clone()
    inf, nan = float("inf"), float("nan")
    zd[1, :] = 0.0                                   # all tied
    zd[2, 40] = nan
    zd[2, 70] = nan
    zd[3, 55] = inf
    zd[4, :] = -inf
    zd[5, 10] = zd[5, 90] = 39.0                     # a tied maximum
    zd[6, 5] = inf
    zd[6, 3] = nan
    for fwd, bwd, extra in ((hxe_fwd, hxe_bwd, enc), (soft_fwd, soft_bwd, table)):
        loss, aux, best, above = fwd(zd, yd, extra)[:4]
        xl, xbest, xabove = xent(zd, yd)
        assert torch.equal(best, xbest) and torch.equal(above, xabove)
        assert best[2] == 40 and best[3] == 55 and best[4] == 0 and best[6] == 3 and best[5] == 10 and best[1] == 0
        bad = torch.tensor([0, 0, 1, 1, 1, 0, 1, 0], dtype=torch.bool, device="cuda")
        assert torch.equal(torch.isnan(loss), bad) and torch.equal(torch.isnan(xl), bad)
        dz = bwd(zd, yd, extra, aux)
        assert torch.equal(torch.isnan(dz).all(dim=1), bad) and torch.equal(torch.isnan(dz).any(dim=1), bad)
        cl, caux = fwd(clean, yd, extra)[:2]
        keep = [0, 7]
        assert torch.equal(loss[keep], cl[keep]) and torch.equal(dz[keep], bwd(clean, yd, extra, caux)[keep])


def test_numerical_edges():
    h, classes, canon = tree("cifar")
    C = 100
    enc = encoding("cifar")
    yd = torch.tensor([17, 17, 17, 60], device="cuda")
    z = torch.zeros((4, C), device="cuda")
    z[0, 17] = -200.0                                # the label far below everything: e_y underflows, L_0 = -200 exactly
    sibs = np.flatnonzero(next(e for e in canon.edges(classes[17]) if not e[3])[2])       # the classes of the label's first range
    z[1, torch.from_numpy(sibs).cuda()] = -200.0     # the label's whole first range underflows: S_1 == 0, floored at L_0
    z[2, :] = -float("inf")
    z[2, 17] = 0.0                                   # -inf everywhere else: probability 1
    z[3, 60] = -float("inf")                         # the label itself at -inf: the loss is +inf, as -log 0 is
    loss, aux, best, above = hxe_fwd(z, yd, enc)
    dz = hxe_bwd(z, yd, enc, aux)
    ref = canon.hxe(z[:1].cpu().numpy().astype(np.float64), [17], alpha=0.1)
    assert abs(float(loss[0]) - ref["loss"][0]) <= hc.loss_k(C) * U * ref["scale"][0]
    assert (np.abs(dz[0].cpu().numpy() - ref["dz"][0]) <= grad_bound(C, ref)[0]).all()
    assert torch.isfinite(loss[:3]).all() and torch.isfinite(dz).all()
    # where the floor acts the loss is a bound of the exact value: off by at most ln(size of the range) x the largest weight
    ref1 = canon.hxe(z[1:2].cpu().numpy().astype(np.float64), [17], alpha=0.1)
    assert len(sibs) > 1 and abs(float(loss[1]) - ref1["loss"][0]) <= np.log(len(sibs)) + hc.loss_k(C) * U * ref1["scale"][0]
    assert float(loss[2]) == 0.0 and float(dz[2].abs().max()) <= 8 * U       # H_0 - lambda_0: a telescoping float32 sum
    assert float(loss[3]) == float("inf") and above[3] == C - 1
    lam0 = float(enc.host["lvl_w"][int(enc.host["path_off"][60])])
    assert abs(float(dz[3, 60]) + lam0) <= 1e-6 and abs(float(dz[3].sum())) <= 1e-5
    # soft labels: a class with target 0 contributes nothing, whatever its logit
    eye = torch.eye(C, device="cuda")
    sl, saux, _, _ = soft_fwd(z, yd, eye)
    assert float(sl[2]) == 0.0 and float(sl[3]) == float("inf") and torch.isfinite(sl[:3]).all()
    assert torch.isfinite(soft_bwd(z, yd, eye, saux)).all()


def test_autograd_ops():
    import sehip
    h, classes, canon = tree("cifar")
    C, B = 100, 32
    enc = h.hxe_encoding(classes, alpha=0.1)
    table = sehip.SoftLabelTable(h.soft_label_table(classes, 10.0))
    zd, yd, z64, y = logits(B, C, torch.float32, seed=31, pitch=104)          # a view: rows 104 floats apart
    assert not zd.is_contiguous()
    for op, extra, fwd, bwd, lowlevel in ((sehip.hierarchical_cross_entropy, enc, hxe_fwd, hxe_bwd, sehip.HxeEncoding.of(enc)),
                                          (sehip.soft_label_cross_entropy, table, soft_fwd, soft_bwd, table.on(zd.device))):
        want, aux, wbest, wabove = fwd(zd, yd, lowlevel)[:4]
        wdz = bwd(zd, yd, lowlevel, aux)
        z = zd.detach().requires_grad_(True)
        loss, best, above = op(z, yd, extra, return_metrics=True)
        assert torch.equal(loss, want) and torch.equal(best, wbest) and torch.equal(above, wabove)
        wts = torch.linspace(0.5, 1.5, B, device="cuda")
        (loss * wts).sum().backward()
        assert torch.equal(z.grad, bwd(zd, yd, lowlevel, aux, g=wts))
        for reduction, total in (("sum", want.sum()), ("mean", None)):
            z = zd.detach().requires_grad_(True)
            red = op(z, yd, extra, reduction=reduction)
            assert red.dim() == 0
            if total is not None:
                assert torch.equal(red, total)
            else:
                assert abs(float(red) - float(want.double().mean())) <= 8 * U * float(want.abs().mean())
            red.backward()
            assert torch.allclose(z.grad, wdz * (1.0 if reduction == "sum" else 1.0 / B), rtol=0, atol=2 * U)
        zb = zd.to(torch.bfloat16).requires_grad_(True)
        op(zb, yd, extra, reduction="mean").backward()
        assert zb.grad.dtype == torch.bfloat16 and torch.isfinite(zb.grad).all()
    assert sehip.HxeEncoding.of(enc).on(zd.device) is sehip.HxeEncoding.of(enc).on(zd.device)      # uploaded once


def test_forward_and_backward_replay_in_a_graph_bit_for_bit():
    import sehip
    h, classes, canon = tree("cifar")
    C, B = 100, 32
    enc = sehip.HxeEncoding(h.hxe_encoding(classes, alpha=0.1))
    table = sehip.SoftLabelTable(h.soft_label_table(classes, 10.0))
    zd, yd, _, _ = logits(B, C, torch.float32, seed=41)
    other, yo, _, _ = logits(B, C, torch.float32, seed=42)
    for op, extra in ((sehip.hierarchical_cross_entropy, enc), (sehip.soft_label_cross_entropy, table)):
        zs = zd.clone().requires_grad_(True)
        ys = yd.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):               # uploads and first calls outside the capture
            for _ in range(2):
                l, _, _ = op(zs, ys, extra, return_metrics=True)
                torch.autograd.grad(l.sum(), zs)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gl, gbest, gabove = op(zs, ys, extra, return_metrics=True)
            (gdz,) = torch.autograd.grad(gl.sum(), zs)
        for zz, yy in ((other, yo), (zd, yd)):
            with torch.no_grad():
                zs.copy_(zz)
            ys.copy_(yy)
            g.replay()
            ze = zz.clone().requires_grad_(True)
            el, ebest, eabove = op(ze, yy, extra, return_metrics=True)
            (edz,) = torch.autograd.grad(el.sum(), ze)
            assert torch.equal(gl, el) and torch.equal(gdz, edz) and torch.equal(gbest, ebest) and torch.equal(gabove, eabove)


def _hierarchy_file(tmp_path):
    path = tmp_path / "cifar.parent-child.txt"
    edges = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))["edges"].tolist()
    path.write_text("".join("%d %d\n" % (p, c) for p, c in edges))
    return str(path)


@pytest.mark.parametrize("loss", ["hxe", "soft_labels"])
def test_learn_classifier_cli_with_a_hierarchy_loss(tmp_path, capsys, monkeypatch, loss):
    import learn_classifier as lc
    import train_cli
    seen = {}
    real = train_cli.average_accuracy
    monkeypatch.setattr(train_cli, "average_accuracy", lambda pred, labels: (seen.update(pred=np.asarray(pred), labels=np.asarray(labels)),
                                                                            real(pred, labels))[1])
    logd = str(tmp_path / "log")
    final = lc.main(["--dataset", "synthetic:100x32x192x64", "--data_root", "-", "--architecture", "resnet-32", "--lr_schedule", "SGD",
                     "--sgd_lr", "0.05", "--batch_size", "32", "--val_batch_size", "32", "--epochs", "3", "--top_k_acc", "5",
                     "--log_dir", logd, "--loss", loss, "--hierarchy", _hierarchy_file(tmp_path)])
    out = capsys.readouterr().out
    assert "[engine] training step: HIP-graph replay" in out and "staying eager" not in out
    assert set(final) == {"loss", "acc", "acc5"} and all(np.isfinite(final[k]) for k in final), final
    log = [json.loads(l) for l in open(os.path.join(logd, "training_log.jsonl"))]
    assert [e["epoch"] for e in log] == [1, 2, 3] and all(np.isfinite(v) for e in log for v in e.values())
    print("training loss per epoch:", [e["loss"] for e in log])
    assert log[-1]["loss"] < log[0]["loss"]                          # the loss falls
    assert all(e["acc5"] >= e["acc"] for e in log)
    # the logged accuracy (read from the loss's own forward launch) is the arg-max accuracy of the predicted logits
    assert final["acc"] == float(np.mean(seen["pred"] == seen["labels"]))


def test_replayed_step_has_the_eager_steps_loss_bits(tmp_path):
    import learn_classifier as lc
    from class_hierarchy import ClassHierarchy
    from datasets import SyntheticGenerator
    from engine import Trainer
    h = ClassHierarchy.from_file(_hierarchy_file(tmp_path), id_type=int)
    gen = SyntheticGenerator(100, 32, 3, 64, 32)
    X, y = gen.train_sequence(32, shuffle=False, batch_transform=lc.transform_inputs, batch_transform_kwargs={"num_classes": 100})[0]
    X = X.contiguous()
    for make in (lambda: lc.HierarchicalCrossEntropy(h.hxe_encoding(list(range(100)), alpha=0.1)),
                 lambda: lc.SoftLabelCrossEntropy(h.soft_label_table(list(range(100)), 10.0))):
        got = []
        for graphs in (False, True):
            torch.manual_seed(0)
            model = lc.build_classifier(100, "resnet-32", input_channels=3).cuda()
            losses, metrics = lc.build_losses(0.0, [5], make())
            tr = Trainer(model, losses, metrics, lr=0.05, clipnorm=10.0, autocast_dtype=None, memory_format=torch.contiguous_format)
            if graphs:
                assert tr.enable_graphs(X, y)
            logs = {}
            tr.train_step(X, y, logs)
            torch.cuda.synchronize()
            got.append({k: float(v) for k, v in logs.items()})
            tr.close()
        assert got[0] == got[1] and np.isfinite(got[0]["loss"]), got
