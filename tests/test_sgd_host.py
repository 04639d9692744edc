"""CPU: the float32 NumPy oracles of se_sgd_step and se_grad_clip_factor (the formulas of include/sehip.h) against the same formulas in
float64 and against engine.Trainer.apply_update on a CPU model, the entry points' host-side argument checks, the binding's refusals,
Trainer(fused_sgd=True)'s refusals and train_cli's SE_FUSED_SGD switch."""
import argparse
import ctypes
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
F = np.float32


def gamma(k):
    """The standard bound k u / (1 - k u) on the relative error of k successive roundings."""
    return k * U / (1.0 - k * U)


def _reg_grad(g, p, l2, grad_scale):
    g = np.asarray(g, dtype=F)
    g1 = g if F(grad_scale) == F(1) else g * F(grad_scale)
    return g1 if l2 is None else g1 + np.asarray(l2, dtype=F) * np.asarray(p, dtype=F)


def sgd_oracle(p, v, g, l2, lr, grad_scale=1.0, clip=None, momentum=0.9, nesterov=False):
    """(p', v') of one se_sgd_step in float32: every NumPy operation below rounds once.  l2 None: no regulariser; clip None: no
    clip, otherwise the float32 factor (stats[1] of se_grad_clip_factor)."""
    p, v = np.asarray(p, dtype=F), np.asarray(v, dtype=F)
    m = F(momentum)
    with np.errstate(all="ignore"):
        g2 = _reg_grad(g, p, l2, grad_scale)
        g3 = g2 if clip is None else g2 * F(clip)
        step = F(lr) * g3
        v2 = m * v - step
        p2 = (p + m * v2) - step if nesterov else p + v2
    assert p2.dtype == F and v2.dtype == F
    return p2, v2


def clip_factor(norm, clipnorm):
    """stats[1] from stats[0]: min(fl(clipnorm / fl(norm + 1e-12f)), 1) in float32, a NaN norm giving NaN."""
    with np.errstate(all="ignore"):
        q = F(clipnorm) / (F(norm) + F(1e-12))
    return F(1) if q > F(1) else F(q)


def clip_oracle(g, p, l2, grad_scale, clipnorm):
    """(norm, factor) of se_grad_clip_factor: the float32 regularised gradient, the correctly rounded sum (math.fsum) of its exact
    float64 squares, norm = (float32)sqrt(S)."""
    with np.errstate(all="ignore"):
        g2 = _reg_grad(g, p, l2, grad_scale).astype(np.float64)
        sq = g2 * g2                                  # exact: a 24-bit significand squared has 48 bits
    S = math.fsum(sq.tolist())
    with np.errstate(all="ignore"):                   # a finite S may lie beyond float32: the norm is then inf
        norm = F(math.sqrt(S)) if S == S else F(np.nan)
    return norm, clip_factor(norm, clipnorm)


def sgd_float64(p, v, g, l2, lr, grad_scale, clip, momentum):
    """The same formula on the same float32 inputs (and float32 lr, scale, factor, momentum) in float64: (step, v', look = m v')."""
    p, v, g = (np.asarray(a, dtype=F).astype(np.float64) for a in (p, v, g))
    g2 = g * np.float64(F(grad_scale))
    if l2 is not None:
        g2 = g2 + np.asarray(l2, dtype=F).astype(np.float64) * p
    if clip is not None:
        g2 = g2 * np.float64(F(clip))
    step = np.float64(F(lr)) * g2
    v2 = np.float64(F(momentum)) * v - step
    return step, v2, np.float64(F(momentum)) * v2


def sgd_inputs(n, seed, with_l2=True):
    """|g| in [1e-6, 1e2], |p| in [1e-3, 10], |v| in [1e-5, 1e-1], both signs, log-uniform; l2 = 2 lambda with lambda in
    {0, 2e-4, 5e-4}.  Every intermediate of the update is then a normal float32 or exactly 0."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice(np.array([-1.0, 1.0]), size=n)
    g = (sign() * 10.0 ** rng.uniform(-6, 2, size=n)).astype(F)
    p = (sign() * 10.0 ** rng.uniform(-3, 1, size=n)).astype(F)
    v = (sign() * 10.0 ** rng.uniform(-5, -1, size=n)).astype(F)
    l2 = (2.0 * rng.choice(np.array([0.0, 2e-4, 5e-4]), size=n)).astype(F) if with_l2 else None
    return p, v, g, l2


def exact_sum_inputs(n, seed, with_l2=True):
    """(g, p, l2) whose regularised gradient g + l2 * p is exact in float32 and whose squares sum exactly in float64 IN ANY ORDER:
    g = +-2^k with k in [-4, 3] (a span of 8), l2 * p in {0, +-2^-6} (l2 = 2^-10, p = +-2^4), so every g2 is a multiple of 2^-6 below
    2^4 and every square a multiple of 2^-12 below 2^8; a sum of n < 2^28 of them is a multiple of 2^-12 below 2^36, which float64
    holds exactly at every stage."""
    rng = np.random.default_rng(seed)
    g = (rng.choice(np.array([-1.0, 1.0]), size=n) * 2.0 ** rng.integers(-4, 4, size=n)).astype(F)
    p = (rng.choice(np.array([-16.0, 16.0]), size=n)).astype(F)
    l2 = (rng.choice(np.array([0.0, 2.0 ** -10]), size=n)).astype(F) if with_l2 else None
    return g, p, l2


# ---------------------------------------------------------------- the oracles against float64

def test_sgd_oracle_agrees_with_float64_within_its_roundings():
    """g, p > 0 and v < 0, so that neither g2 = g1 + l2 p nor v' = m v - step cancels.  Roundings, each at most u = 2^-24 relative:
    g1 1, l2 p 1, g2 2, g3 (the clip) 3, step 4; m v 1; v' = fl(m v - step) max(1, 4) + 1 = 5.  So |v' - V| <= gamma_5 |V| =: e_v.
    Plain: p' = fl(p + v'), so |p' - P| <= e_v + u (|P| + e_v).
    Nesterov: look = fl(m v') carries 6: e_l = gamma_6 |m V|; ahead = fl(p + look): e_a = e_l + u (|p + m V| + e_l);
    p' = fl(ahead - step): e_a + gamma_4 |step| + u (|P| + e_a + gamma_4 |step|).
    Without scale, regulariser, clip and momentum and from p = 0 the update IS -fl(lr g): one rounding."""
    p, v, g, l2 = sgd_inputs(20000, 1)
    p, g, v = np.abs(p), np.abs(g), -np.abs(v)
    lr, scale, clip, m = 0.01, 0.5, F(0.37), 0.9
    step, V, look = sgd_float64(p, v, g, l2, lr, scale, clip, m)
    p64 = p.astype(np.float64)
    e_v = gamma(5) * np.abs(V)
    p2, v2 = sgd_oracle(p, v, g, l2, lr, scale, clip, m, nesterov=False)
    P = p64 + V
    assert np.all(np.abs(v2 - V) <= e_v)
    assert np.all(np.abs(p2 - P) <= e_v + U * (np.abs(P) + e_v))
    p3, v3 = sgd_oracle(p, v, g, l2, lr, scale, clip, m, nesterov=True)
    assert np.array_equal(v3.view(np.int32), v2.view(np.int32))                    # the velocity does not depend on Nesterov
    e_l = gamma(6) * np.abs(look)
    e_a = e_l + U * (np.abs(p64 + look) + e_l)
    P = (p64 + look) - step
    e_s = gamma(4) * np.abs(step)
    assert np.all(np.abs(p3 - P) <= e_a + e_s + U * (np.abs(P) + e_a + e_s))
    z = np.zeros_like(g)
    p4, v4 = sgd_oracle(z, z, g, None, lr, 1.0, None, 0.0)
    want = -np.float64(F(lr)) * g.astype(np.float64)
    assert np.all(np.abs(p4 - want) <= U * np.abs(want)) and np.array_equal(p4.view(np.int32), v4.view(np.int32))


def test_clip_oracle_agrees_with_float64_within_its_roundings():
    """With an exact g2 (no scale, no regulariser) the sum S is correctly rounded (1 rounding, which sqrt halves), sqrt rounds once in
    float64 and once to float32: |norm - N| <= (u + 2 * 2^-53) N, held to 2 u.  The factor is two more float32 roundings (the sum
    with 1e-12, the quotient) of a quotient whose denominator carries the norm's error: 4 u."""
    _, _, g, _ = sgd_inputs(30000, 3, with_l2=False)
    norm, factor = clip_oracle(g, None, None, 1.0, 10.0)
    N = math.sqrt(math.fsum((g.astype(np.float64) ** 2).tolist()))
    assert abs(float(norm) - N) <= 2 * U * N and norm.dtype == F and factor.dtype == F
    assert N > 10.0 and abs(float(factor) - 10.0 / (N + 1e-12)) <= 4 * U * 10.0 / N
    assert clip_oracle(g, None, None, 1.0, 1e6)[1] == F(1)                         # inactive: exactly 1
    # on inputs whose squares sum exactly in any order the float64 sums of np.sum (pairwise), of a running loop and of fsum agree
    g, p, l2 = exact_sum_inputs(4103, 5)
    g2 = _reg_grad(g, p, l2, 1.0).astype(np.float64)
    assert np.array_equal(g2, g.astype(np.float64) + l2.astype(np.float64) * p.astype(np.float64))      # g2 is exact
    sq = g2 * g2
    run = 0.0
    for x in sq[::-1].tolist():
        run += x
    assert math.fsum(sq.tolist()) == float(np.sum(sq)) == run == float(np.sum(np.sort(sq)))


def test_oracles_on_zeros_non_finite_values_zero_momentum_and_nesterov():
    z = np.zeros(4, dtype=F)
    for nesterov in (False, True):
        p2, v2 = sgd_oracle(z, z, z, z + F(4e-4), 0.01, 0.5, F(0.25), 0.9, nesterov)
        assert not p2.view(np.int32).any() and not v2.view(np.int32).any()         # +0 everywhere, bitwise
    norm, factor = clip_oracle(z, z, z + F(4e-4), 0.5, 10.0)
    assert norm.view(np.int32) == 0 and factor == F(1)                             # norm +0, factor exactly 1
    g = np.array([np.nan, 1.0, 2.0], dtype=F)
    norm, factor = clip_oracle(g, None, None, 1.0, 10.0)
    assert np.isnan(norm) and np.isnan(factor)                                     # a NaN norm gives a NaN factor
    for bad in (np.inf, -np.inf):
        norm, factor = clip_oracle(np.array([bad, 1.0], dtype=F), None, None, 1.0, 10.0)
        assert norm == F(np.inf) and factor.view(np.int32) == 0                    # an infinite norm gives factor +0
    norm, factor = clip_oracle(np.array([3e38, 3e38], dtype=F), None, None, 1.0, 10.0)
    assert norm == F(np.inf) and factor == 0                                       # a finite S beyond float32
    g = np.array([np.nan, np.inf, -np.inf, 1.0], dtype=F)
    one = np.ones(4, dtype=F)
    p2, v2 = sgd_oracle(one, one, g, None, 0.01)
    assert np.isnan(p2).tolist() == [True, False, False, False] and np.isinf(p2).tolist() == [False, True, True, False]
    assert np.isnan(sgd_oracle(one, one, g, None, 0.01, clip=F(0))[0]).tolist() == [True, True, True, False]      # inf * 0
    assert np.isnan(sgd_oracle(one, one, one, None, 0.01, clip=F(np.nan))[0]).all()
    # momentum 0: the velocity is minus the step and forgets what it held; p moves by it
    p, v, g, l2 = sgd_inputs(1000, 7)
    p2, v2 = sgd_oracle(p, v, g, l2, 0.01, momentum=0.0)
    step = F(0.01) * (g + l2 * p)
    assert np.array_equal(v2, -step) and np.array_equal(p2, p + v2)
    assert np.array_equal(sgd_oracle(p, v * 0, g, l2, 0.01, momentum=0.0)[1], v2)
    # Nesterov against the plain update: same velocity, p' differs by (m v' - step) - v' = m v' - m v
    pp, vp = sgd_oracle(p, v, g, l2, 0.01, momentum=0.9, nesterov=False)
    pn, vn = sgd_oracle(p, v, g, l2, 0.01, momentum=0.9, nesterov=True)
    assert np.array_equal(vp.view(np.int32), vn.view(np.int32)) and (pp != pn).any()
    diff = pn.astype(np.float64) - pp.astype(np.float64)
    want = np.float64(F(0.9)) * (vp.astype(np.float64) - v.astype(np.float64))
    # each of pp, pn carries at most 2 roundings of size u |p'| plus those of its addends (look, step, v': u each)
    slack = 3 * U * (np.abs(pp) + np.abs(pn) + np.abs(vp) + np.abs(step))
    assert np.all(np.abs(diff - want) <= slack)


# ---------------------------------------------------------------- the oracle against Trainer.apply_update on the CPU

def _cpu_trainer(seed, nesterov, clipnorm, with_l2):
    from engine import Trainer
    torch.manual_seed(seed)
    net = torch.nn.Linear(37, 11)
    l2_of = {id(net.weight): 5e-4} if with_l2 else None
    tr = Trainer(net, {}, lr=0.05, momentum=0.9, nesterov=nesterov, clipnorm=clipnorm, l2_of=l2_of, autocast_dtype=None)
    flat = tr.flat
    rng = np.random.default_rng(seed)
    for off, n in flat.offsets:                       # the padding words between the slices stay +0
        flat.flat_g[off:off + n] = torch.from_numpy(rng.standard_normal(n).astype(F))
        flat.flat_v[off:off + n] = torch.from_numpy((0.01 * rng.standard_normal(n)).astype(F))
    assert flat.total > sum(n for _, n in flat.offsets) and flat.has_l2 == with_l2
    return tr


@pytest.mark.parametrize("branch", ["eager", "lr_tensor"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("with_l2", [False, True], ids=["nol2", "l2"])
def test_oracle_agrees_with_the_torch_composition_on_a_cpu_model(branch, nesterov, with_l2):
    """Trainer.apply_update (the composition the fused kernels stand in for) on a CPU Linear model against sgd_oracle, fed the clip
    factor the composition itself computes from its regularised gradient (torch's float32 norm is another sum: clip_oracle's norm is
    held against it below).  With scale s = 0.5 (exact) the two can differ in these roundings only, each u relative to its result:
      a. l2 * p: addcmul_ may fuse it into the sum (the oracle rounds it): u |l2 p| in g2, times factor * lr in the step;
      b. eager branch only: lr * g3, which add_(g, alpha=-lr) may fuse (the oracle rounds the step): u |step|;
      c. the rounding of v' itself acts on operands that differ by a + b, so the two v' differ by at most a + b + 2 u |v'| =: e_v.
    Plain: p' = fl(p + v'): e_v + 2 u |p'|.
    Nesterov: add_(v, alpha=m) may fuse m * v' (u |m v'|), ahead = fl(p + m v') acts on differing operands (m e_v, then 2 u |ahead|),
    the step is subtracted (b again, and a), and the last rounding gives 2 u |p'|:
      e_p = m e_v + u |m v'| + 2 u |ahead| + (a + b) + 2 u |p'|.
    In the lr_tensor branch without regulariser the plain update has no such rounding at all: it is bit-equal.
    The norm: torch sums n float32 squares (1 rounding each, at most n - 1 additions: gamma_n on S, half of it on the norm, plus the
    square root's rounding), the oracle rounds three times (fsum, sqrt, float32), g2 may differ by a (at most u relative per element,
    so u on the norm): |norm_torch - norm_oracle| <= (n / 2 + 5) u norm with n = the buffer's length."""
    clipnorm, scale, lr, m = 0.5, 0.5, 0.05, 0.9
    tr = _cpu_trainer(11 + nesterov, nesterov, clipnorm, with_l2)
    flat = tr.flat
    p0, v0, g0 = (t.clone().numpy() for t in (flat.flat_p, flat.flat_v, flat.flat_g))
    l2 = flat.flat_l2.numpy().copy() if with_l2 else None
    reg = torch.from_numpy(g0) * scale
    if with_l2:
        reg = reg.addcmul(flat.flat_l2, flat.flat_p)
    tnorm = torch.linalg.vector_norm(reg)
    factor = F(torch.clamp(clipnorm / (tnorm + 1e-12), max=1.0).item())
    assert factor < 1                                                              # the clip is active
    onorm, ofactor = clip_oracle(g0, p0, l2, scale, clipnorm)
    n = flat.total
    assert abs(float(tnorm) - float(onorm)) <= (n / 2 + 5) * U * float(onorm)
    assert abs(float(factor) - float(ofactor)) <= (n / 2 + 8) * U * float(ofactor)   # + the sum with 1e-12, the quotient, and its own rounding
    assert factor == clip_factor(F(tnorm.item()), clipnorm)                        # the factor formula is torch's clamp line, bit for bit

    if branch == "eager":
        tr.apply_update(scale)
    else:
        tr.apply_update(scale, lr_tensor=torch.full((), lr, dtype=torch.float32), count=False)
    assert tr.iterations == (1 if branch == "eager" else 0)
    wp, wv = sgd_oracle(p0, v0, g0, l2, lr, scale, factor, m, nesterov)
    gp, gv = flat.flat_p.numpy(), flat.flat_v.numpy()
    a64 = np.float64
    l2p = np.abs(l2.astype(a64) * p0) if with_l2 else np.zeros(n)
    step = np.abs(a64(F(lr)) * ((g0.astype(a64) * scale + (l2.astype(a64) * p0 if with_l2 else 0.0)) * a64(factor)))
    e_a = U * l2p * float(factor) * lr * (1 + 8 * U)
    e_b = U * step * (1 + 8 * U) if branch == "eager" else 0.0
    e_v = e_a + e_b + 2 * U * np.abs(wv)
    assert np.all(np.abs(gv.astype(a64) - wv) <= e_v)
    if nesterov:
        look = np.abs(a64(F(m)) * wv)
        ahead = np.abs(p0.astype(a64) + a64(F(m)) * wv)
        e_p = m * e_v + U * look + 2 * U * ahead + e_a + e_b + 2 * U * np.abs(wp)
    else:
        e_p = e_v + 2 * U * np.abs(wp)
    assert np.all(np.abs(gp.astype(a64) - wp) <= e_p)
    assert (wp != p0).any() and np.isfinite(wp).all()
    if branch == "lr_tensor" and not with_l2 and not nesterov:
        assert np.array_equal(gp.view(np.int32), wp.view(np.int32)) and np.array_equal(gv.view(np.int32), wv.view(np.int32))
    pad = np.ones(n, dtype=bool)
    for off, k in flat.offsets:
        pad[off:off + k] = False
    assert not wp[pad].view(np.int32).any() and not wv[pad].view(np.int32).any()   # the oracle keeps the padding words +0


# ---------------------------------------------------------------- the C ABI without a device

def test_entry_points_check_their_arguments_without_a_gpu():
    import sehip
    lib = sehip.lib()
    for name in ("se_sgd_step", "se_grad_clip_factor", "se_grad_clip_workspace_bytes"):
        assert name in sehip.EXPORTS and hasattr(lib, name), name
    assert sehip.SGD_MAX_BLOCKS == sehip.ops.DEFINES["SE_SGD_MAX_BLOCKS"] > 0
    assert lib.se_grad_clip_workspace_bytes() >= 8 * sehip.SGD_MAX_BLOCKS           # one float64 partial per workgroup
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def step(p=one, v=one, g=one, l2=z, n=5, lr=0.01, lr_dev=z, scale=1.0, clip=z, m=0.9, nesterov=0):
        return lib.se_sgd_step(p, v, g, l2, n, lr, lr_dev, scale, clip, m, nesterov, z)

    for kw in (dict(p=z), dict(v=z), dict(g=z)):
        assert step(**kw) == -1 and b"se_sgd_step: null pointer" in lib.se_last_error(), kw
    assert step(n=-1) == -1 and b"se_sgd_step" in lib.se_last_error()
    for bad in (-0.5, float("nan")):
        assert step(m=bad) == -1 and b"se_sgd_step" in lib.se_last_error() and b"momentum" in lib.se_last_error()
    assert step(n=0) == 0 and step(p=z, v=z, g=z, n=0) == 0                        # nothing to do: no launch, no device needed

    def clip(g=one, p=z, l2=z, n=5, scale=1.0, clipnorm=10.0, ws=one, stats=one):
        return lib.se_grad_clip_factor(g, p, l2, n, scale, clipnorm, ws, stats, z)

    for kw in (dict(g=z), dict(ws=z), dict(stats=z)):
        assert clip(**kw) == -1 and b"se_grad_clip_factor: null pointer" in lib.se_last_error(), kw
    assert clip(l2=one) == -1 and b"l2 needs p" in lib.se_last_error()
    assert clip(n=-1) == -1 and b"se_grad_clip_factor" in lib.se_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert clip(clipnorm=bad) == -1 and b"clipnorm" in lib.se_last_error(), bad
    assert clip(ws=ctypes.c_void_p(20)) == -1 and b"8-byte" in lib.se_last_error()
    assert clip(n=0) == 0 and clip(g=z, ws=z, stats=z, n=0) == 0                   # no launch; stats is not touched (it is NULL here)


def test_binding_refuses_host_tensors_and_exports_the_names():
    import sehip
    t = torch.zeros(8)
    with pytest.raises(sehip.SehipError):
        sehip.sgd_step_(t, t.clone(), t.clone(), lr=0.01)
    with pytest.raises(sehip.SehipError):
        sehip.grad_clip_factor(t, clipnorm=10.0)
    for name in ("sgd_step_", "grad_clip_factor", "SGD_MAX_BLOCKS"):
        assert name in sehip.ops.__all__ and hasattr(sehip, name), name


# ---------------------------------------------------------------- the trainer's switch

def test_trainer_fused_sgd_argument():
    from engine import Trainer
    tr = Trainer(torch.nn.Linear(3, 2), {}, autocast_dtype=None)
    assert tr.fused_sgd is False and tr.grad_stats is None                         # opt-in
    with pytest.raises(ValueError, match="GPU"):
        Trainer(torch.nn.Linear(3, 2), {}, autocast_dtype=None, fused_sgd=True)    # CPU parameters keep the composition
    with pytest.raises(ValueError, match="adagrad"):
        Trainer(torch.nn.Linear(3, 2), {}, autocast_dtype=None, optimizer="adagrad", fused_sgd=True)


def test_train_cli_reads_the_environment_switch(monkeypatch):
    import train_cli
    seen = []

    def fake_trainer(model, losses, metrics, **kw):
        seen.append(kw)
        return kw

    monkeypatch.setattr(train_cli, "Trainer", fake_trainer)
    args = argparse.Namespace(architecture="resnet-110-fc", sgd_lr=0.1, nesterov=False, clipgrad=10.0)
    for value, want in ((None, False), ("0", False), ("true", False), ("1", True)):
        if value is None:
            monkeypatch.delenv("SE_FUSED_SGD", raising=False)
        else:
            monkeypatch.setenv("SE_FUSED_SGD", value)
        kw = train_cli._trainer(args, None, {}, {}, None, decay=0.0)
        assert kw["fused_sgd"] is want and kw["clipnorm"] == 10.0 and kw["decay"] == 0.0, value
    assert len(seen) == 4
