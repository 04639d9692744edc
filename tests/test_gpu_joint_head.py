"""se_joint_head_fwd / se_joint_head_bwd (csrc/joint_head.hip) through the C ABI.

The contract of include/sehip.h: the classifier role carries the bits of se_softmax_xent_fwd / _bwd at smoothing 0; the nearest-class
metric those of se_nn_accuracy(dot_prod_sim = 1) on p; the arg-max metric is np.argmax and a strict count; the embedding loss lies
within a derived float32 bound of the float64 oracle and is reproducible; dp is one float32 product per element.  Shapes are the small
ones at which a kernel changes path: partial and several 32-sample strips, D across the scalar / 16-byte / staged-chunk boundaries,
one class tile up to sliced class sets (C = 1000), the wave (C <= 1024) and workgroup (C = 1025) rows of the cross-entropy, and the
pitches that switch off the vector loads."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON_F = -12345.5
POISON_I = -777
KS = (1, 2, 5)
BS = (1, 31, 33, 67)
SHAPES = [(1, 1), (7, 2), (64, 31), (65, 33), (100, 100), (64, 1000), (64, 1025)]        # (D, C)
SQUARE = [1, 2, 31, 33, 100, 1000, 1025]                                              # D == C of the arg-max metric
LAYOUTS = ("contig", "padded", "off1")
NEAREST, ARGMAX = 0, 1
XE_HI = 16.118095


def _call(*a):
    from sehip._lib import call
    return call(*a)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.dtype == torch.bfloat16 else t)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _place(vals, layout, dtype=None):
    """`vals` [rows, cols] as a view with the layout's pitch / alignment; padding holds NaN.  contig: pitch = cols; padded: pitch =
    cols + 8 rounded to 8 (16-byte loads stay on); off1: base one element past a 16-byte boundary, pitch cols + 1 (scalar paths)."""
    vals = vals.to(dtype or vals.dtype)
    rows, cols = vals.shape
    if layout == "contig":
        return vals.contiguous()
    if layout == "padded":
        buf = torch.full((rows, (cols // 8 + 2) * 8), float("nan"), dtype=vals.dtype, device=vals.device)
        buf[:, :cols] = vals
        return buf[:, :cols]
    assert layout == "off1"
    ld = cols + 1
    buf = torch.full((rows * ld + 8,), float("nan"), dtype=vals.dtype, device=vals.device)
    view = buf[1:1 + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(vals)
    return view


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _dt(t):
    return 0 if t.dtype == torch.float32 else 1


def _out(rows, cols, pad, dtype=torch.float32):
    buf = torch.full((rows, cols + pad), POISON_F, dtype=dtype, device="cuda")
    return buf, buf[:, :cols]


class Result(object):
    pass


def make_inputs(B, D, C, seed=0, unit=True):
    gen = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * D + C)
    emb = torch.nn.functional.normalize(torch.randn((C, D), generator=gen), dim=1)
    if C > 3:
        emb[3] = emb[1]                                   # a table with duplicate rows
    p = torch.randn((B, D), generator=gen)
    if unit:
        p = torch.nn.functional.normalize(p, dim=1)
    labels = torch.randint(0, C, (B,), generator=gen)
    for i in range(0, B, 5):                              # rows equal to a class embedding, every other one its own label's
        p[i] = emb[(i * 7) % C]
        if i % 10 == 0:
            labels[i] = (i * 7) % C
    if B > 5 and C > 3:                                   # the label's score is shared by its duplicate: n_within >= 2
        p[5] = emb[1]
        labels[5] = 3
    z = torch.randn((B, C), generator=gen) * 4
    return p.cuda(), labels.cuda(), emb.cuda(), z.cuda()


def special_logits(z, labels):
    """rows 0-3: a NaN, +inf, nothing but -inf, confidently wrong"""
    B, C = z.shape
    z = z.clone()
    if B > 0:
        z[0, C // 2] = float("nan")
    if B > 1:
        z[1, C - 1] = float("inf")
    if B > 2:
        z[2, :] = float("-inf")
    if B > 3 and C > 1:
        y = int(labels[3])
        z[3, :] = -10.0
        z[3, y] = -40.0
        z[3, (y + 1) % C] = 40.0
    return z


def run_fwd(p, labels, emb, logits, metric, skip=(), lds_pad=0):
    """one se_joint_head_fwd on caller buffers (poisoned, dirty workspace); `skip`: optional outputs passed as NULL"""
    B, D = p.shape
    C = emb.shape[0] if emb is not None else D
    r = Result()
    r.scores_buf, r.scores = _out(B, C, lds_pad)
    for name in ("emb_loss_i", "cls_loss_i"):
        setattr(r, name, torch.full((B,), POISON_F, dtype=torch.float32, device="cuda"))
    r.aux = torch.full((3 * B,), POISON_F, dtype=torch.float32, device="cuda")
    for name in ("n_better", "n_within", "p_best", "p_above", "z_best", "z_above"):
        setattr(r, name, torch.full((B,), POISON_I, dtype=torch.int32, device="cuda"))
    r.need = _call("se_joint_head_workspace_bytes", metric, B, D, C)
    ws = torch.full((r.need // 8,), -1, dtype=torch.int64, device="cuda") if r.need else None

    def opt(name):
        return None if name in skip else getattr(r, name)

    _call("se_joint_head_fwd", p, _ld(p), labels, emb, _ld(emb) if emb is not None else 0, B, D, C, metric, r.emb_loss_i,
          r.n_better if metric == NEAREST else opt("n_better"), r.n_within if metric == NEAREST else opt("n_within"), opt("p_best"),
          r.p_above if metric == ARGMAX else opt("p_above"), opt("scores"), C + lds_pad,
          logits, _dt(logits) if logits is not None else 0, _ld(logits) if logits is not None else 0,
          r.cls_loss_i if logits is not None else None, r.aux if logits is not None else None, opt("z_best"), opt("z_above"), ws, r.need)
    return r


def run_xent(logits, labels, g=None, dz_dtype=None, dz_pad=0):
    """se_softmax_xent_fwd (+ _bwd with per-row weights g) at smoothing 0 on the same logits"""
    B, C = logits.shape
    r = Result()
    r.cls_loss_i = torch.full((B,), POISON_F, dtype=torch.float32, device="cuda")
    r.aux = torch.full((3 * B,), POISON_F, dtype=torch.float32, device="cuda")
    r.z_best = torch.full((B,), POISON_I, dtype=torch.int32, device="cuda")
    r.z_above = torch.full((B,), POISON_I, dtype=torch.int32, device="cuda")
    _call("se_softmax_xent_fwd", logits, _dt(logits), _ld(logits), labels, B, C, 0.0, r.cls_loss_i, r.aux, r.z_best, r.z_above, None)
    if g is not None:
        r.dz_buf, r.dz = _out(B, C, dz_pad, dz_dtype)
        _call("se_softmax_xent_bwd", logits, _dt(logits), _ld(logits), labels, r.aux, g, 0.0, B, C, 0.0, r.dz, _dt(r.dz), C + dz_pad)
    return r


def run_nn(p, labels, emb, lds_pad=0):
    B, D = p.shape
    C = emb.shape[0]
    r = Result()
    r.scores_buf, r.scores = _out(B, C, lds_pad)
    r.p_best = torch.full((B,), POISON_I, dtype=torch.int32, device="cuda")
    need = _call("se_nn_accuracy_workspace_bytes", B, C)
    r.acc = {}
    for k in KS:
        acc = torch.full((B,), POISON_F, dtype=torch.float32, device="cuda")
        ws = torch.empty((need // 8,), dtype=torch.int64, device="cuda") if need else None
        _call("se_nn_accuracy", p, _ld(p), labels, emb, _ld(emb), B, D, C, 1, k, acc, r.scores, C + lds_pad, r.p_best, ws, need)
        r.acc[k] = acc
    return r


def run_bwd(labels, emb, B, D, C, w, logits=None, aux=None, g=None, dz_dtype=None, dp_pad=0, dz_pad=0, want_dp=True):
    """one se_joint_head_bwd; w / g: per-row float32 tensors or Python floats (the scalar scales)"""
    r = Result()
    r.dp_buf, r.dp = _out(B, D, dp_pad)
    r.dz_buf, r.dz = _out(B, C, dz_pad, dz_dtype or torch.float32)
    wt, ws_ = (w, 0.0) if torch.is_tensor(w) else (None, float(w))
    gt, gs = (g, 0.0) if torch.is_tensor(g) else (None, float(g if g is not None else 0.0))
    _call("se_joint_head_bwd", labels, emb, _ld(emb) if emb is not None else 0, B, D, C, wt, ws_, r.dp if want_dp else None, D + dp_pad,
          logits, _dt(logits) if logits is not None else 0, _ld(logits) if logits is not None else 0, aux, gt, gs,
          r.dz if logits is not None else None, _dt(r.dz), C + dz_pad)
    return r


def _acc(r, k):
    return ((r.n_within >= 1) & (r.n_better < k)).float()


def test_shape_table_covers_the_issue_values():
    assert set(BS) == {1, 31, 33, 67}
    assert {(1, 1), (7, 2), (64, 31), (65, 33), (100, 100), (64, 1000), (64, 1025)} <= set(SHAPES)
    import sehip
    lib = sehip.lib()
    assert lib.se_joint_head_workspace_bytes(NEAREST, 67, 64, 1000) > 0          # class slices meet in the workspace
    assert lib.se_joint_head_workspace_bytes(NEAREST, 67, 100, 100) == 0
    assert lib.se_joint_head_workspace_bytes(ARGMAX, 67, 1000, 1000) == 0


@pytest.mark.parametrize("zdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_classifier_role_and_nearest_metric_carry_the_siblings_bits(shape, zdtype):
    D, C = shape
    for B in BS:
        for unit in (True, False):
            p, labels, emb, z = make_inputs(B, D, C, seed=1, unit=unit)
            z = special_logits(z, labels).to(zdtype)
            got = run_fwd(p, labels, emb, z, NEAREST)
            want_x, want_n = run_xent(z, labels), run_nn(p, labels, emb)
            for name in ("cls_loss_i", "aux", "z_best", "z_above"):
                assert _same(getattr(got, name), getattr(want_x, name)), (name, B, unit)
            assert _same(got.scores, want_n.scores) and torch.equal(got.p_best, want_n.p_best), (B, unit)
            for k in KS:
                assert _same(_acc(got, k), want_n.acc[k]), (k, B, unit)
            assert bool((got.p_above == POISON_I).all())
            assert int(got.n_within.min()) >= 1                                  # the label's own score, bit for bit
            if B > 5 and C > 3:
                assert int(got.n_within[5]) >= 2                                 # and its duplicate row's
            # backward: per-row weights, then the scalar scales
            gen = torch.Generator().manual_seed(B)
            g = torch.randn((B,), generator=gen).cuda()
            w = torch.randn((B,), generator=gen).cuda()
            for dzt in (torch.float32, torch.bfloat16):
                bw = run_bwd(labels, emb, B, D, C, w, z, got.aux, g, dzt)
                assert _same(bw.dz, run_xent(z, labels, g, dzt).dz), (B, dzt)
                E = emb.cpu().numpy()[labels.cpu().numpy().clip(0, C - 1)]
                want_dp = (-w.cpu().numpy())[:, None] * E
                assert np.array_equal(bw.dp.cpu().numpy().view(np.int32), want_dp.astype(np.float32).view(np.int32)), B
            bw = run_bwd(labels, emb, B, D, C, 0.25, z, got.aux, 1.0 / B, torch.float32)
            gs = torch.full((B,), 1.0 / B, dtype=torch.float32, device="cuda")
            assert _same(bw.dz, run_xent(z, labels, gs, torch.float32).dz), B
            assert np.array_equal(bw.dp.cpu().numpy().view(np.int32), (np.float32(-0.25) * E).astype(np.float32).view(np.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("zdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pitches_and_alignment(layout, zdtype):
    for D, C in ((64, 31), (100, 100), (64, 1000), (64, 1025)):
        B = 33
        p0, labels, emb0, z0 = make_inputs(B, D, C, seed=2)
        p, emb, z = _place(p0, layout), _place(emb0, layout), _place(special_logits(z0, labels), layout, zdtype)
        got = run_fwd(p, labels, emb, z, NEAREST, lds_pad=3)
        want_x, want_n = run_xent(z, labels), run_nn(p, labels, emb, lds_pad=3)
        for name in ("cls_loss_i", "aux", "z_best", "z_above"):
            assert _same(getattr(got, name), getattr(want_x, name)), (name, D, C)
        assert _same(got.scores, want_n.scores) and torch.equal(got.p_best, want_n.p_best)
        assert bool((got.scores_buf[:, C:] == POISON_F).all()), "scores pitch padding written"
        for k in KS:
            assert _same(_acc(got, k), want_n.acc[k]), (k, D, C)
        # the layout changes no value of the embedding loss's inputs; the bound test covers its values
        g = torch.linspace(-1, 1, B).cuda()
        pad = {"contig": 0, "padded": 8 - C % 8 + 8, "off1": 1}[layout]
        for dzt in (torch.float32, torch.bfloat16):
            bw = run_bwd(labels, emb, B, D, C, g, z, got.aux, g, dzt, dp_pad=pad, dz_pad=pad)
            assert _same(bw.dz, run_xent(z, labels, g, dzt, dz_pad=pad).dz), (D, C, dzt)
            assert bool((bw.dz_buf[:, C:] == POISON_F).all()) and bool((bw.dp_buf[:, D:] == POISON_F).all()), "pitch padding written"
            E = emb.cpu().numpy()[labels.cpu().numpy()]
            assert np.array_equal(bw.dp.cpu().numpy().view(np.int32), ((-g.cpu().numpy())[:, None] * E).astype(np.float32).view(np.int32))


def test_confidently_wrong_row_is_clipped():
    B, D, C = 33, 64, 31
    p, labels, emb, z = make_inputs(B, D, C, seed=3)
    z = special_logits(z, labels)
    got = run_fwd(p, labels, emb, z, NEAREST)
    loss = got.cls_loss_i.cpu().numpy()
    assert loss[3] == np.float32(XE_HI)
    assert np.isnan(loss[:3]).all() and np.isfinite(loss[3:]).all()
    assert got.z_above.cpu().numpy()[:3].tolist() == [C, C, C] and got.z_best.cpu().numpy()[:3].tolist() == [C // 2, C - 1, 0]
    bw = run_bwd(labels, emb, B, D, C, 1.0, z, got.aux, 1.0)
    dz = bw.dz.cpu().numpy()
    assert (dz[3] == 0).all() and np.isnan(dz[:3]).all() and np.isfinite(dz[4:]).all()


def _argmax_inputs(B, C, seed):
    """rows in turn: random, quantised (deliberate ties), softmax-like; row 0 holds a NaN, row 1 a +inf, row 2 nothing but -inf"""
    gen = torch.Generator().manual_seed(31 * seed + 5 * B + C)
    p = torch.randn((B, C), generator=gen)
    p[1::3] = torch.round(p[1::3] * 2) / 2
    p[2::3] = torch.softmax(p[2::3] * 3, dim=-1)
    labels = torch.randint(0, C, (B,), generator=gen)
    for i in range(4, B, 4):                               # the label on a tied maximum that is not the first one
        p[i, :] = torch.round(p[i, :])
        top = (p[i] == p[i].max()).nonzero().flatten()
        labels[i] = top[-1]
    bad = torch.zeros((B,), dtype=torch.bool)
    if B > 0:
        p[0, C // 2] = float("nan"); bad[0] = True
        if C > 2:
            p[0, C - 1] = float("nan")
    if B > 1:
        p[1, C // 3] = float("inf"); bad[1] = True
    if B > 2:
        p[2, :] = float("-inf"); bad[2] = True
    return p, labels, bad


@pytest.mark.parametrize("table", [False, True], ids=["onehot", "table"])
@pytest.mark.parametrize("C", SQUARE)
def test_argmax_metric_is_numpy_argmax_and_a_strict_count(C, table):
    for B in BS:
        for layout in LAYOUTS:
            p0, labels, bad = _argmax_inputs(B, C, seed=4)
            emb = None
            if table:
                emb = _place(torch.nn.functional.normalize(torch.randn((C, C), generator=torch.Generator().manual_seed(C)), dim=1).cuda(), layout)
            p = _place(p0.cuda(), layout)
            got = run_fwd(p, labels.cuda(), emb, None, ARGMAX)
            pn, yn = p0.numpy(), labels.numpy()
            assert np.array_equal(got.p_best.cpu().numpy(), np.argmax(pn, -1).astype(np.int32)), (B, layout)
            above = (pn > pn[np.arange(B), yn][:, None]).sum(-1).astype(np.int32)
            above[bad.numpy()] = C            # se_softmax_xent_fwd's rule for a row with a NaN / +inf / nothing but -inf (tf.nn.in_top_k)
            assert np.array_equal(got.p_above.cpu().numpy(), above), (B, layout)
            for name in ("n_better", "n_within", "z_best", "z_above"):
                assert bool((getattr(got, name) == POISON_I).all()), name
            assert bool((got.scores_buf == POISON_F).all()) and bool((got.cls_loss_i == POISON_F).all())
            loss = got.emb_loss_i.cpu().numpy()
            if not table:
                want = np.float32(1) - pn[np.arange(B), yn]
                nan = np.isnan(want)                        # a NaN's sign and payload are no part of the value
                assert np.array_equal(np.isnan(loss), nan), (B, layout)
                assert np.array_equal(loss[~nan].view(np.int32), want[~nan].astype(np.float32).view(np.int32)), (B, layout)
                w = torch.linspace(-2, 2, B).cuda() if B > 1 else torch.tensor([0.5]).cuda()
                for ww in (w, -0.125):
                    bw = run_bwd(labels.cuda(), None, B, C, C, ww, dp_pad=3)
                    dp = np.zeros((B, C), dtype=np.float32)
                    dp[np.arange(B), yn] = -(w.cpu().numpy() if torch.is_tensor(ww) else np.float32(ww))
                    assert np.array_equal(bw.dp.cpu().numpy().view(np.int32), dp.view(np.int32)), (B, layout)       # +0 elsewhere
                    assert bool((bw.dp_buf[:, C:] == POISON_F).all()) and bool((bw.dz_buf == POISON_F).all())


def _loss_bound(E, p):
    D = p.shape[1]
    return 1.01 * (math.ceil(D / 64) + 10) * 2.0 ** -24 * (1.0 + np.abs(E.astype(np.float64) * p.astype(np.float64)).sum(-1))


@pytest.mark.parametrize("metric", [NEAREST, ARGMAX], ids=["nearest", "argmax"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_embedding_loss_against_the_float64_oracle(layout, metric):
    from oracle import loss_oracle
    shapes = SHAPES if metric == NEAREST else [(c, c) for c in SQUARE]
    for D, C in shapes:
        for B in BS:
            for unit in (True, False):
                p0, labels, emb0, _ = make_inputs(B, D, C, seed=5, unit=unit)
                p, emb = _place(p0, layout), _place(emb0, layout)
                got = run_fwd(p, labels, emb, None, metric)
                again = run_fwd(p, labels, emb, None, metric)
                assert _same(got.emb_loss_i, again.emb_loss_i)                       # same buffers, same bits
                pn, En = p0.cpu().numpy(), emb0.cpu().numpy()[labels.cpu().numpy()]
                want = loss_oracle.inv_correlation(En.astype(np.float64), pn.astype(np.float64))
                err = np.abs(got.emb_loss_i.cpu().numpy().astype(np.float64) - want)
                bound = _loss_bound(En, pn)
                assert (err <= bound).all(), (D, C, B, unit, float((err / bound).max()))
                assert bool((got.cls_loss_i == POISON_F).all()) and bool((got.aux == POISON_F).all())    # logits == NULL


def test_each_optional_output_may_be_null():
    for B, D, C in ((33, 24, 100), (40, 24, 1000)):
        p, labels, emb, z = make_inputs(B, D, C, seed=6)
        full = run_fwd(p, labels, emb, z, NEAREST)
        for name in ("p_best", "scores", "z_best", "z_above", "p_above"):
            got = run_fwd(p, labels, emb, z, NEAREST, skip=(name,))
            for other in ("emb_loss_i", "cls_loss_i", "aux", "n_better", "n_within", "p_best", "scores", "z_best", "z_above"):
                if other != name:
                    assert _same(getattr(got, other), getattr(full, other)), (name, other)
            assert bool((getattr(got, name) == (POISON_F if name == "scores" else POISON_I)).all())
    B, C = 33, 100
    p0, labels, _ = _argmax_inputs(B, C, seed=6)
    p, labels = p0.cuda(), labels.cuda()
    z = torch.randn((B, C), generator=torch.Generator().manual_seed(6)).cuda()
    full = run_fwd(p, labels, None, z, ARGMAX)
    for name in ("p_best", "z_best", "z_above", "n_better", "n_within", "scores"):
        got = run_fwd(p, labels, None, z, ARGMAX, skip=(name,))
        for other in ("emb_loss_i", "cls_loss_i", "aux", "p_best", "p_above", "z_best", "z_above"):
            if other != name:
                assert _same(getattr(got, other), getattr(full, other)), (name, other)
    assert _same(full.cls_loss_i, run_xent(z, labels).cls_loss_i)
    # backward: dp == NULL skips the embedding role, logits == NULL skips dz
    g = torch.linspace(-1, 1, B).cuda()
    only_dz = run_bwd(labels, None, B, C, C, g, z, full.aux, g, want_dp=False)
    assert bool((only_dz.dp_buf == POISON_F).all()) and _same(only_dz.dz, run_xent(z, labels, g, torch.float32).dz)
    only_dp = run_bwd(labels, None, B, C, C, g)
    assert bool((only_dp.dz_buf == POISON_F).all()) and float(only_dp.dp.abs().sum()) > 0


def test_labels_out_of_range_equal_their_clamped_values():
    B, D, C = 33, 64, 31
    p, labels, emb, z = make_inputs(B, D, C, seed=7)
    wild = labels.clone()
    wild[0], wild[1], wild[2] = -5, C, 2 ** 40
    clamped = wild.clamp(0, C - 1)
    g = torch.linspace(-1, 1, B).cuda()
    for metric, e, pp in ((NEAREST, emb, p), (ARGMAX, None, z)):
        a, b = run_fwd(pp, wild, e, z, metric), run_fwd(pp, clamped, e, z, metric)
        for name in ("emb_loss_i", "cls_loss_i", "aux", "n_better", "n_within", "p_best", "p_above", "scores", "z_best", "z_above"):
            assert _same(getattr(a, name), getattr(b, name)), name
        Dm = pp.shape[1]
        x, y = run_bwd(wild, e, B, Dm, C, g, z, a.aux, g), run_bwd(clamped, e, B, Dm, C, g, z, b.aux, g)
        assert _same(x.dp, y.dp) and _same(x.dz, y.dz)


def test_empty_batch_touches_nothing():
    p, labels, emb, z = make_inputs(4, 8, 5, seed=8)
    f = [torch.full((4, 8), POISON_F, device="cuda") for _ in range(6)]
    i = [torch.full((4,), POISON_I, dtype=torch.int32, device="cuda") for _ in range(6)]
    assert _call("se_joint_head_fwd", p, 8, labels, emb, 8, 0, 8, 5, NEAREST, f[0], i[0], i[1], i[2], i[3], f[1], 8, z, 0, 5, f[2], f[3],
                 i[4], i[5], None, 0) == 0
    assert _call("se_joint_head_fwd", None, 8, None, None, 8, 0, 8, 5, NEAREST, None, None, None, None, None, None, 8, None, 0, 5, None, None,
                 None, None, None, 0) == 0
    assert _call("se_joint_head_bwd", labels, emb, 8, 0, 8, 5, None, 1.0, f[4], 8, z, 0, 5, f[3], None, 1.0, f[5], 0, 5) == 0
    assert _call("se_joint_head_bwd", None, None, 8, 0, 8, 5, None, 1.0, None, 8, None, 0, 5, None, None, 1.0, None, 0, 5) == 0
    torch.cuda.synchronize()
    assert all(bool((b == POISON_F).all()) for b in f) and all(bool((b == POISON_I).all()) for b in i)


def test_invalid_arguments_are_refused():
    import sehip
    lib = sehip.lib()
    INVALID = sehip._lib.DEFINES["SE_ERR_INVALID"]
    B, D, C = 64, 24, 1000
    p, labels, emb, z = make_inputs(B, D, C, seed=9)
    sq = torch.randn((B, C), device="cuda")
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    need = lib.se_joint_head_workspace_bytes(NEAREST, B, D, C)
    assert need > 0
    ws = torch.zeros((need // 8 + 2,), dtype=torch.int64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    null = ctypes.c_void_p(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(p=ptr(p), ldp=D, labels=ptr(labels), emb=ptr(emb), lde=D, B=B, D=D, C=C, metric=NEAREST, loss=ptr(f(B)), nb=ptr(i(B)), nw=ptr(i(B)),
                pbest=ptr(i(B)), pabove=ptr(i(B)), scores=ptr(f(B, C)), lds=C, z=ptr(z), zdt=0, ldz=C, closs=ptr(f(B)), aux=ptr(f(3 * B)),
                zbest=ptr(i(B)), zabove=ptr(i(B)), ws=ptr(ws), wsb=need)
    order = list(good)

    def run(**change):
        args = dict(good, **change)
        return lib.se_joint_head_fwd(*[args[k] for k in order], stream)

    assert run() == 0
    onehot = dict(metric=ARGMAX, emb=null, p=ptr(sq), ldp=C, D=C, ws=null, wsb=0)
    assert run(**onehot) == 0
    assert run(pbest=null, scores=null, zbest=null, zabove=null, pabove=null) == 0
    assert run(z=null, closs=null, aux=null) == 0
    bad = [dict(metric=2), dict(metric=-1), dict(zdt=7), dict(p=null), dict(labels=null), dict(loss=null), dict(nb=null), dict(nw=null),
           dict(emb=null), dict(closs=null), dict(aux=null), dict(ldp=D - 1), dict(lde=D - 1), dict(lds=C - 1), dict(ldz=C - 1),
           dict(ws=null), dict(wsb=need - 8), dict(ws=ctypes.c_void_p(ws.data_ptr() + 4)), dict(D=0), dict(C=0), dict(B=-1),
           dict(metric=ARGMAX, emb=null),                                     # the identity table needs D == C
           dict(onehot, metric=NEAREST), dict(onehot, pabove=null), dict(onehot, ldp=C - 1)]
    for change in bad:
        assert run(**change) == INVALID, change
        assert b"se_joint_head_fwd" in lib.se_last_error(), change

    gb = dict(labels=ptr(labels), emb=ptr(emb), lde=D, B=B, D=D, C=C, w=null, ws_=1.0, dp=ptr(f(B, D)), lddp=D, z=ptr(z), zdt=0, ldz=C,
              aux=ptr(f(3 * B)), g=null, gs=1.0, dz=ptr(f(B, C)), dzdt=0, lddz=C)
    border = list(gb)

    def runb(**change):
        args = dict(gb, **change)
        return lib.se_joint_head_bwd(*[args[k] for k in border], stream)

    assert runb() == 0
    assert runb(dp=null) == 0 and runb(z=null, aux=null, dz=null) == 0
    for change in [dict(labels=null), dict(lde=D - 1), dict(lddp=D - 1), dict(ldz=C - 1), dict(lddz=C - 1), dict(aux=null), dict(dz=null),
                   dict(zdt=7), dict(dzdt=7), dict(emb=null), dict(D=0), dict(C=0), dict(B=-1)]:
        assert runb(**change) == INVALID, change
        assert b"se_joint_head_bwd" in lib.se_last_error(), change
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [100, 1000])
def test_graph_replay_equals_eager(C):
    """forward and backward captured as one chain; inputs overwritten in place; C = 1000 covers the workspace re-initialisation"""
    import sehip
    B, D = 64, 24
    p, labels, emb, z = make_inputs(B, D, C, seed=10)
    p.requires_grad_(True); z.requires_grad_(True)
    gw = torch.linspace(0.5, 1.5, B).cuda()

    def step():
        out = sehip.joint_head(p, labels, emb, logits=z, metric="nearest", want_scores=True)
        dp, dz = torch.autograd.grad((out.emb_loss_i * gw).sum() + 0.1 * out.cls_loss_i.sum(), (p, z))
        return tuple(out) + (dp, dz)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (11, 12):
        p2, labels2, _, z2 = make_inputs(B, D, C, seed=seed)
        with torch.no_grad():
            p.copy_(p2); z.copy_(z2); labels.copy_(labels2)
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for n, (a, b) in enumerate(zip(captured, eager)):
            assert (a is None) == (b is None), n
            if a is not None:
                assert _same(a.detach(), b.detach()), n


def test_autograd_makes_one_backward_call(monkeypatch):
    import sehip
    import sehip.ops as ops
    B, D, C = 67, 100, 100
    p, labels, emb, z = make_inputs(B, D, C, seed=13)
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    for zdtype in (torch.float32, torch.bfloat16):
        pp, zz = p.clone().requires_grad_(True), z.to(zdtype).clone().requires_grad_(True)
        out = sehip.joint_head(pp, labels, emb, logits=zz, metric="nearest")
        assert not any(getattr(out, n).requires_grad for n in ("n_better", "n_within", "p_best", "z_best", "z_above"))
        assert out.p_above is None and out.scores is None
        gw, gz = torch.linspace(0.5, 1.5, B).cuda(), torch.linspace(-0.1, 0.1, B).cuda()
        ((out.emb_loss_i * gw).sum() + (out.cls_loss_i * gz).sum()).backward()
        assert names.count("se_joint_head_fwd") == 1 and names.count("se_joint_head_bwd") == 1
        assert not [n for n in names if n in ("se_softmax_xent_fwd", "se_softmax_xent_bwd", "se_nn_accuracy")]
        names.clear()
        want = run_bwd(labels, emb, B, D, C, gw, zz.detach(), run_xent(zz.detach(), labels).aux, gz, zdtype)
        assert _same(pp.grad, want.dp) and _same(zz.grad, want.dz) and zz.grad.dtype == zdtype
    # SEHIP_CHECK_LABELS is honoured
    monkeypatch.setenv("SEHIP_CHECK_LABELS", "1")
    wild = labels.clone(); wild[0] = C
    with pytest.raises(IndexError):
        sehip.joint_head(p, wild, emb, logits=z)
    with pytest.raises(IndexError):
        sehip.joint_head(z, wild, None, metric="argmax")
