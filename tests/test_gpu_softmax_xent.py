"""GPU: se_softmax_xent_fwd / _bwd (the categorical cross-entropy of the softmax classifier, label smoothing, Keras 2.2's probability
clip, arg-max and top-k counts) through the C ABI on NaN-padded pitches into sentinel-guarded outputs, against the float64 oracle of
tests/test_classifier_host.py -- every instantiation and every path the host code can select, named in the test ids -- plus the
crafted rows the clip is about, the fixture recorded from Keras' formula, autograd of sehip.softmax_cross_entropy and determinism
(repeats, a busy second stream, HIP-graph replay)."""
import os

import numpy as np
import pytest
import torch

from test_classifier_host import HI32, LO32, U, Oracle, fixed_order_mean, fixture

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
SENT32 = np.int32(0x7FC0DEAD)       # a quiet NaN with a payload no kernel writes
SENT16 = np.int16(0x7FAD)           # the same for bf16 outputs
WAVE_MAX_C, BLOCK_MAX_C = 1024, 8192          # path selection of csrc/softmax_xent.hip


def call(name, *args):
    from sehip._lib import call as c
    return c(name, *args)


def path_of(C):
    return "wave" if C <= WAVE_MAX_C else ("block" if C <= BLOCK_MAX_C else "stream")


def pitch(C, dtype, vec, variant=0):
    """(row pitch in elements, offset of the first element): 16-byte aligned rows for the vector loads; an odd pitch (variant 0) or
    an aligned pitch behind a base pointer that is not 16-byte aligned (variant 1) for the scalar ones."""
    esz = 2 if dtype == BF16 else 4
    if vec:
        return (C + 7) // 8 * 8 + 8, 0
    if variant == 1:
        return (C + 7) // 8 * 8 + 8, 1
    ld = C + 1
    return (ld if (ld * esz) % 16 else ld + 1), 0


def place(a, ld, off, dtype):
    """Device copy of the float32 matrix ``a`` with row pitch ``ld`` from element ``off`` of its buffer, NaN everywhere else."""
    rows, d = a.shape
    buf = torch.full((max(rows, 1) * ld + 8,), float("nan"), dtype=TORCH[dtype], device="cuda")
    view = buf[off:off + max(rows, 1) * ld].view(max(rows, 1), ld)[:rows, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda().to(TORCH[dtype]))
    return view


class Guarded(object):
    """A [rows, cols] output of pitch ``ld`` from element ``off`` + one guard row of its sentinel buffer (two guard rows behind)."""

    def __init__(self, rows, cols, ld, off=0, dtype=torch.float32):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.raw = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self.sent = SENT16 if dtype == torch.bfloat16 else SENT32
        self.start = ld + off
        self.buf = torch.full(((rows + 3) * ld + 8,), int(self.sent), dtype=self.raw, device="cuda")
        view = self.buf[self.start:self.start + max(rows, 1) * ld].view(max(rows, 1), ld)[:rows, :cols]
        self.out = view if dtype == torch.int32 else view.view(dtype)

    def read(self):
        b = self.buf.cpu().numpy()
        inside = np.zeros(b.shape, dtype=bool)
        for r in range(self.rows):
            inside[self.start + r * self.ld:self.start + r * self.ld + self.cols] = True
        assert (b[~inside] == self.sent).all(), "a store left the output (pitch padding or guard rows)"
        got = b[inside].reshape(self.rows, self.cols)
        if self.dtype == torch.bfloat16:
            return torch.from_numpy(got.copy()).view(torch.bfloat16).float().numpy()
        return got.view(np.float32).copy() if self.dtype == torch.float32 else got.copy()


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def run(z, labels, s, zdt=F32, ddt=F32, vec=True, variant=0, w=None, scale=1.0, metrics=True, mean=True):
    """forward + backward through the C ABI; -> dict of host arrays (loss, best, above, mean, dz)."""
    B, C = z.shape
    ld, off = pitch(C, zdt, vec, variant)
    ldd, offd = pitch(C, ddt, vec, variant)
    zd = place(z, ld, off, zdt)
    yd = torch.from_numpy(np.asarray(labels, dtype=np.int64)).cuda()
    wd = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float32)).cuda()
    n_aux = int(call("se_softmax_xent_aux_floats", B))
    assert n_aux == 3 * B
    loss, aux = Guarded(1, B, B + 4), Guarded(1, n_aux, n_aux + 4)
    best, above = Guarded(1, B, B + 4, dtype=torch.int32), Guarded(1, B, B + 4, dtype=torch.int32)
    lmean = Guarded(1, 1, 4)
    dz = Guarded(B, C, ldd, offd, dtype=TORCH[ddt])
    none = B == 0
    call("se_softmax_xent_fwd", None if none else zd, zdt, ld, None if none else yd, B, C, float(s), None if none else loss.out,
         None if none else aux.out, best.out if metrics and not none else None, above.out if metrics and not none else None,
         lmean.out if mean else None)
    call("se_softmax_xent_bwd", None if none else zd, zdt, ld, None if none else yd, None if none else aux.out, wd, float(scale), B, C,
         float(s), None if none else dz.out, ddt, ldd)
    torch.cuda.synchronize()
    res = {"loss": loss.read()[0], "aux": aux.read()[0], "dz": dz.read(), "mean": lmean.read()[0, 0] if mean else None}
    if metrics:
        res["best"], res["above"] = best.read()[0], above.read()[0]
    if none or not metrics:
        assert (best.buf.cpu().numpy() == SENT32).all() and (above.buf.cpu().numpy() == SENT32).all()
    if not mean:
        assert (lmean.buf.cpu().numpy() == SENT32).all()
    return res


def check(res, z_used, labels, s, ddt, w, tag, worst=None):
    """One run against the oracle: the loss and gradient bounds, exact metrics, the fixed-order mean."""
    o = Oracle(z_used, labels, s)
    B, C = z_used.shape
    assert o.in_window.sum() <= 1e-3 * max(B * C, 1), (tag, "lower-clip window", int(o.in_window.sum()))
    ok = ~o.bad
    err = np.abs(res["loss"].astype(np.float64) - o.loss)
    assert np.all(err[ok] <= o.loss_bound[ok]), (tag, "loss", float((err[ok] / o.loss_bound[ok]).max()))
    assert np.isnan(res["loss"][o.bad]).all(), (tag, "loss of NaN / +inf rows")
    if "best" in res:
        assert np.array_equal(res["best"], o.best), (tag, "best")
        assert np.array_equal(res["above"], o.above), (tag, "above")
    wv = np.asarray(w, dtype=np.float64).reshape(-1, 1)
    ref = wv * o.dz
    bound = np.abs(wv) * o.grad_bound
    if ddt == BF16:
        bound = bound + 2.0 ** -8 * np.abs(ref) + 2.0 ** -133
    gerr = np.abs(res["dz"].astype(np.float64) - ref)
    assert np.all(gerr[ok] <= bound[ok]), (tag, "dz", float((gerr[ok] / bound[ok]).max()))
    assert np.isnan(res["dz"][o.bad]).all(), (tag, "dz of NaN / +inf rows")
    if res.get("mean") is not None and not o.bad.any():
        assert np.float32(res["mean"]).view(np.int32) == fixed_order_mean(res["loss"]).view(np.int32), (tag, "loss_mean")
    if worst is not None and ok.any():
        worst[0] = max(worst[0], float((err[ok] / o.loss_bound[ok]).max()))
        worst[1] = max(worst[1], float((gerr[ok] / bound[ok]).max()))
    return o


# C on both sides of every path boundary, the issue's class counts, and rows too long for the register paths
CS = (1, 2, 3, 100, 1000, 1024, 1025, 8142, 8192, 8193, 20011)
MATRIX = [(C, zdt, ddt, vec) for C in CS for zdt in (F32, BF16) for ddt in (F32, BF16) for vec in (True, False)]


def matrix_id(c):
    C, zdt, ddt, vec = c
    return "C%d-%s-z%s-dz%s-%s" % (C, path_of(C), "bf16" if zdt else "f32", "bf16" if ddt else "f32", "vec16" if vec else "scalar")


def matrix_cases(C, zdt, ddt, vec):
    """B = 0, 1, 37, 128, 1024 (the widest rows: the smaller batches), s = 0 / 0.1 / 1.5 (one-hot again), logit scales 0.5 / 3 / 10,
    labels partly outside [0, C), per-row weights or grad_scale, the scalar variants, metrics / mean pointers present or NULL."""
    Bs = (0, 1, 37, 128, 1024) if C <= 1025 else ((0, 1, 37, 128) if C <= 8193 else (0, 1, 37))
    rng = np.random.default_rng(C * 131 + zdt * 7 + ddt * 3 + int(vec))
    n = 0
    for B in Bs:
        for s in (0.0, 0.1, 1.5):
            if C == 1 and s == 0.1:
                continue                          # SE_ERR_INVALID (tests/test_classifier_host.py)
            n += 1
            scale = (0.5, 3.0, 10.0)[n % 3]
            while True:     # the licence of the lower clip is capped at 0.1 % of a case (check() asserts it): draw until the oracle agrees
                z = (rng.standard_normal((B, C)) * scale).astype(np.float32)
                labels = rng.integers(-2, C + 2, size=B)
                if B == 0 or Oracle(bf16_round(z) if zdt == BF16 else z, labels, s).in_window.sum() <= 1e-3 * B * C:
                    break
            w = rng.uniform(-2.0, 2.0, size=B).astype(np.float32) if n % 2 else None
            yield n, B, s, scale, z, labels, w, np.float32(1.0 / max(B, 1))


@pytest.mark.parametrize("C,zdt,ddt,vec", MATRIX, ids=[matrix_id(c) for c in MATRIX])
def test_every_instantiation_and_path_against_the_oracle(C, zdt, ddt, vec):
    worst = [0.0, 0.0]
    for n, B, s, scale, z, labels, w, gs in matrix_cases(C, zdt, ddt, vec):
        res = run(z, labels, s, zdt, ddt, vec, variant=n % 2, w=w, scale=gs, metrics=n % 4 != 3, mean=n % 5 != 4)
        if B == 0:
            if res["mean"] is not None:
                assert np.float32(res["mean"]).view(np.int32) == 0        # +0
            continue
        z_used = bf16_round(z) if zdt == BF16 else z
        check(res, z_used, labels, s, ddt, w if w is not None else np.full(B, gs), (B, C, s, scale), worst)
    print("worst loss error / bound %.3f, worst dz error / bound %.3f" % tuple(worst))


def crafted(C, y):
    """Rows the clip and the metric rules are about; label column ``y``, C >= 12."""
    o1, o2 = (y + 3) % C, (y + 7) % C
    rows, names = [], []

    def row(name, fill, **cols):
        r = np.full(C, fill, dtype=np.float32)
        for c, v in cols.items():
            r[int(c[1:])] = v
        rows.append(r)
        names.append(name)
    row("wrong", -50.0, **{"c%d" % y: 0.0, "c%d" % o1: 30.0})                    # z_y = 0, another logit 30
    row("right", 0.0, **{"c%d" % y: 30.0})
    row("tie_max", 0.0, **{"c%d" % o2: 7.0, "c%d" % o1: 7.0, "c%d" % (C - 1): 7.0})
    row("tie_zy", 1.0, **{"c%d" % o1: 2.0, "c%d" % o2: 2.0, "c%d" % y: 1.0})    # every other class ties with z_y: not counted
    row("nan", 0.0, **{"c%d" % o2: np.nan, "c%d" % o1: np.nan, "c%d" % ((o1 + 1) % C): np.inf})
    row("inf", 0.0, **{"c%d" % o2: np.inf, "c%d" % o1: np.inf})
    row("neg_inf", 0.0, **{"c%d" % o1: -np.inf, "c%d" % o2: -np.inf})
    row("neg_inf_y", 0.0, **{"c%d" % y: -np.inf})
    return np.stack(rows), names, o1, o2


@pytest.mark.parametrize("vec", [True, False], ids=["vec16", "scalar"])
@pytest.mark.parametrize("zdt", [F32, BF16], ids=["zf32", "zbf16"])
@pytest.mark.parametrize("C", [12, 1500, 9000], ids=["C12-wave", "C1500-block", "C9000-stream"])
def test_crafted_rows(C, zdt, vec):
    y = 5
    z, names, o1, o2 = crafted(C, y)
    B = len(names)
    labels = np.full(B, y)
    i = {n: k for k, n in enumerate(names)}
    first, second = min(o1, o2), max(o1, o2)
    for s in (0.0, 0.1):
        res = run(z, labels, s, zdt, F32, vec, w=None, scale=1.0)
        check(res, z, labels, s, F32, np.ones(B), (C, s))
        loss, dz, best, above = res["loss"], res["dz"], res["best"], res["above"]
        if s == 0.0:
            assert loss[i["wrong"]].view(np.int32) == HI32.view(np.int32) and not dz[i["wrong"]].any()
            assert loss[i["right"]].view(np.int32) == LO32.view(np.int32)
            assert loss[i["neg_inf_y"]].view(np.int32) == HI32.view(np.int32) and not dz[i["neg_inf_y"]].any()
        else:
            assert loss[i["wrong"]] < HI32                                   # (1 - s) HI + s / (C - 1) (LO + (C - 2) HI)
        assert best[i["wrong"]] == o1 and above[i["wrong"]] == 1 and best[i["right"]] == y and above[i["right"]] == 0
        assert best[i["tie_max"]] == first and above[i["tie_max"]] == 3
        assert best[i["tie_zy"]] == first and above[i["tie_zy"]] == 2
        assert best[i["nan"]] == first and above[i["nan"]] == C and np.isnan(loss[i["nan"]]) and np.isnan(dz[i["nan"]]).all()
        assert best[i["inf"]] == first and above[i["inf"]] == C and np.isnan(loss[i["inf"]]) and np.isnan(dz[i["inf"]]).all()
        assert np.isfinite(loss[i["neg_inf"]]) and np.isfinite(dz[i["neg_inf"]]).all() and not dz[i["neg_inf"], [o1, o2]].any()
        assert best[i["neg_inf"]] == min(set(range(3)) - {o1, o2}) and above[i["neg_inf"]] == 0
        assert above[i["neg_inf_y"]] == C - 1 and np.isfinite(dz[i["neg_inf_y"]]).all()
    # labels outside [0, C) behave as clamped; s = 1.5 is one-hot
    zr = (np.random.default_rng(C).standard_normal((64, C)) * 3).astype(np.float32)
    wild = np.random.default_rng(C + 1).integers(-5, C + 5, size=64)
    a = run(zr, wild, 0.1, zdt, F32, vec)
    b = run(zr, np.clip(wild, 0, C - 1), 0.1, zdt, F32, vec)
    c = run(zr, wild, 1.5, zdt, F32, vec)
    d = run(zr, wild, 0.0, zdt, F32, vec)
    for k in ("loss", "dz", "best", "above", "aux"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
        assert np.array_equal(c[k].view(np.int32), d[k].view(np.int32)), k
    assert not np.array_equal(a["loss"], d["loss"])


def test_all_rows_minus_infinity_and_single_class():
    """C = 1: loss LO (p = 1, clipped high), no gradient; a row of -inf only has no softmax: NaN like a row with a NaN, best 0, never in the top k."""
    res = run(np.array([[3.0], [-2.0]], dtype=np.float32), np.array([0, 0]), 0.0)
    assert (res["loss"].view(np.int32) == LO32.view(np.int32)).all() and not res["dz"].any()
    assert res["best"].tolist() == [0, 0] and res["above"].tolist() == [0, 0]
    res = run(np.full((1, 40), -np.inf, dtype=np.float32), np.array([7]), 0.0)
    assert np.isnan(res["loss"][0]) and np.isnan(res["dz"]).all() and res["best"][0] == 0 and res["above"][0] == 40


def test_fixture_cases_on_the_device():
    """The fixture's logits: the kernel against Keras' own float64 values (loss bound; the recorded gradient rows), f32 and bf16."""
    fx = fixture()
    for key in [str(c) for c in fx["cases"]]:
        z, y, gcols = fx[key + "_logits"].astype(np.float32), fx[key + "_labels"], fx[key + "_gcols"]
        for si, s in enumerate(fx["smoothings"]):
            for zdt in (F32, BF16):
                res = run(z, y, s, zdt, F32, vec=(si == 0))
                z_used = bf16_round(z) if zdt == BF16 else z
                o = check(res, z_used, y, s, F32, np.ones(len(y)), (key, s, zdt))
                if zdt == F32:      # the grid values are not exact in bf16: Keras' recorded values apply to the float32 logits only
                    ref64, g64 = fx["%s_s%d_loss64" % (key, si)], fx["%s_s%d_grad64" % (key, si)]
                    assert np.all(np.abs(res["loss"] - ref64) <= o.loss_bound + 2 * U * np.abs(ref64)), (key, s)
                    assert np.all(np.abs(res["dz"][:2][:, gcols] - g64) <= o.grad_bound[:2][:, gcols] + 2 * U * o.Y[:2][:, gcols]), (key, s)


def torch64(z, y, s, C):
    """The clamp form in float64 torch (clamp passes gradient on [LO, HI] inclusive)."""
    from test_classifier_host import HI64, LO64, target
    Y = torch.from_numpy(target(y.cpu().numpy(), C, s)).to(z.device)
    t = torch.logsumexp(z, -1, keepdim=True) - z
    return (Y * torch.clamp(t, LO64, HI64)).sum(-1)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_against_float64_torch(reduction, dtype):
    import sehip
    rng = np.random.default_rng(17)
    B, C, s = 96, 100, 0.1
    wide = torch.from_numpy((rng.standard_normal((B, C + 4)) * 3).astype(np.float32)).cuda().to(dtype)
    z = wide[:, :C].detach().requires_grad_(True)              # a row pitch that is not C
    assert z.stride(0) == C + 4
    y = torch.from_numpy(rng.integers(0, C, size=B)).cuda()
    g = torch.from_numpy(rng.uniform(0.1, 1.0, size=B).astype(np.float32)).cuda()
    out, best, above = sehip.softmax_cross_entropy(z, y, s, reduction=reduction, return_metrics=True)
    z64 = z.detach().double().requires_grad_(True)
    ref = torch64(z64, y, s, C)
    if reduction == "none":
        assert out.shape == (B,)
        out.backward(g)
        ref.backward(g.double())
    else:
        assert out.dim() == 0
        ref = ref.mean() if reduction == "mean" else ref.sum()
        (out * 0.3).backward()
        (ref * 0.3).backward()
    assert out.dtype == torch.float32 and z.grad.dtype == dtype and z.grad.shape == (B, C)
    assert torch.allclose(out.detach().double(), ref.detach(), rtol=1e-5, atol=3e-5)      # the loss bound at C = 100, |z| <= 15
    tol = dict(rtol=1e-4, atol=1e-7) if dtype == torch.float32 else dict(rtol=2.0 ** -7, atol=1e-6)
    assert torch.allclose(z.grad.double(), z64.grad, **tol)
    zn = z.detach().float().cpu().numpy()
    assert np.array_equal(best.cpu().numpy(), zn.argmax(-1))
    assert np.array_equal(above.cpu().numpy(), (zn > zn[np.arange(B), y.cpu().numpy()][:, None]).sum(-1))
    assert best.dtype == torch.int32 and not best.requires_grad
    if reduction == "mean":        # the kernel's fixed-order mean, bit for bit
        li = sehip.softmax_cross_entropy(z.detach(), y, s)
        assert out.detach().cpu().numpy().view(np.int32) == fixed_order_mean(li.cpu().numpy()).view(np.int32)
    with pytest.raises(sehip.SehipError):
        sehip.softmax_cross_entropy(z, y, s, reduction="batchmean")
    with pytest.raises(sehip.SehipError):
        sehip.softmax_cross_entropy(z, y.int(), s)


def _fwd_bwd(z, y, g, s, outs):
    loss, aux, best, above, mean, dz = outs
    B, C = z.shape
    call("se_softmax_xent_fwd", z, F32, z.stride(0), y, B, C, s, loss, aux, best, above, mean)
    call("se_softmax_xent_bwd", z, F32, z.stride(0), y, aux, g, 0.0, B, C, s, dz, F32, dz.stride(0))


def _outs(B, C):
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    i = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    return f(B), f(3 * B), i(B), i(B), f(1), f(B, C)


def _same(a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


@pytest.mark.parametrize("B,C", [(128, 100), (256, 8142), (64, 20011)], ids=["wave", "block", "stream"])
def test_determinism_repeats_and_busy_second_stream(B, C):
    rng = np.random.default_rng(3)
    z = torch.from_numpy((rng.standard_normal((B, C)) * 3).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, C, size=B)).cuda()
    g = torch.from_numpy(rng.uniform(0.1, 1.0, size=B).astype(np.float32)).cuda()
    runs = [_outs(B, C) for _ in range(20)]
    for o in runs:
        _fwd_bwd(z, y, g, 0.1, o)
    torch.cuda.synchronize()
    assert all(_same(o, runs[0]) for o in runs[1:])
    a = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    busy = [_outs(B, C) for _ in range(10)]
    with torch.cuda.stream(side):
        for _ in range(40):
            a = torch.tanh(a @ a * 1e-3)
    for o in busy:
        _fwd_bwd(z, y, g, 0.1, o)
    torch.cuda.synchronize()
    assert all(_same(o, runs[0]) for o in busy)


def test_graph_capture_replays_bit_equal_to_eager():
    import sehip
    rng = np.random.default_rng(4)
    B, C = 128, 1000
    z = torch.from_numpy((rng.standard_normal((B, C)) * 3).astype(np.float32)).cuda().requires_grad_(True)
    y = torch.from_numpy(rng.integers(0, C, size=B)).cuda()

    def step():
        z.grad = None
        loss, best, above = sehip.softmax_cross_entropy(z, y, 0.1, reduction="mean", return_metrics=True)
        (loss * 0.5).backward()
        return loss.detach(), best, above

    el, eb, ea = [t.clone() for t in step()]
    eg = z.grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    z.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl, gb, ga = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gl.view(torch.int32), el.view(torch.int32))
        assert torch.equal(gb, eb) and torch.equal(ga, ea)
        assert torch.equal(z.grad.view(torch.int32), eg.view(torch.int32))
