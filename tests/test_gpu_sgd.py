"""GPU: se_sgd_step bit for bit against the float32 NumPy oracle of test_sgd_host.py and se_grad_clip_factor against its float64
oracle -- every path (16-byte, scalar, tail, more than one trip of the grid-stride loop), regulariser / scale / clip / Nesterov / device
learning rate, zeros, non-finite gradients, HIP-graph capture -- and engine.Trainer(fused_sgd=True) on the flat buffers of a ResNet-32
under the cosine loss."""
import itertools

import numpy as np
import pytest
import torch

from _flat_buffers import SIZES, _big_n, _bits, _dev
from test_sgd_host import F, U, clip_factor, clip_oracle, exact_sum_inputs, sgd_inputs, sgd_oracle

pytestmark = pytest.mark.gpu

LR, MOM = 0.01, 0.9


def test_the_feature_is_exported():
    import sehip
    assert "se_sgd_step" in sehip.EXPORTS and "se_grad_clip_factor" in sehip.EXPORTS
    assert callable(sehip.sgd_step_) and callable(sehip.grad_clip_factor)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_three_steps_are_bit_exact(n, offset):
    """p and v equal sgd_oracle fed the factor read back from stats; g is only read; the factor is the formula of the norm."""
    import sehip
    n = _big_n(sehip.SGD_MAX_BLOCKS) if n == "big" else n
    p0, v0, g0, l20 = sgd_inputs(n, 100 + n % 97)
    grads = [g0] + [sgd_inputs(n, 200 + s + n % 97)[2] for s in (1, 2)]
    clipnorm = 0.5 * float(np.sqrt(n))                     # |g| is log-uniform up to 100: the clip is active
    ws = torch.empty(sehip.SGD_MAX_BLOCKS * 8, dtype=torch.uint8, device="cuda")
    l2d, gds = _dev(l20, offset), [_dev(gh, offset) for gh in grads]
    norms = {}
    for with_l2, scale, with_clip, nesterov, lr_on_device in itertools.product((False, True), (1.0, 0.5), (False, True), (False, True),
                                                                              (False, True)):
        p, v = _dev(p0, offset), _dev(v0, offset)
        l2 = l2d if with_l2 else None
        lr = torch.full((), LR, dtype=torch.float32, device="cuda") if lr_on_device else LR
        stats = torch.zeros(2, dtype=torch.float32, device="cuda")
        wp, wv = p0, v0
        for step, (gh, g) in enumerate(zip(grads, gds)):
            factor = None
            if with_clip:
                sehip.grad_clip_factor(g, p, l2, grad_scale=scale, clipnorm=clipnorm, workspace=ws, out=stats)
            sehip.sgd_step_(p, v, g, l2, lr=lr, grad_scale=scale, clip=stats[1:] if with_clip else None, momentum=MOM, nesterov=nesterov)
            what = (n, offset, with_l2, scale, with_clip, nesterov, lr_on_device, step)
            if with_clip:
                norm, factor = stats.cpu().numpy()
                assert _bits(factor) == _bits(clip_factor(norm, clipnorm)), what
                if step == 0:              # the first norm depends on (regulariser, scale) alone: one oracle sum serves 4 combinations
                    key = (with_l2, scale)
                    if key not in norms:
                        norms[key] = clip_oracle(gh, p0, l20 if with_l2 else None, scale, clipnorm)[0]
                    # 1 float32 ulp (positive floats: adjacent bit patterns): any order of n < 2^28 non-negative float64 additions
                    # errs by less than n 2^-53 relative, far below 2^-24
                    assert abs(int(_bits(norm)) - int(_bits(norms[key]))) <= 1, what
            wp, wv = sgd_oracle(wp, wv, gh, l20 if with_l2 else None, LR, scale, factor, MOM, nesterov)
            assert np.array_equal(_bits(g), _bits(gh)), what                          # g is only read
            assert np.array_equal(_bits(v), _bits(wv)), what
            assert np.array_equal(_bits(p), _bits(wp)), what
        assert np.isfinite(wp).all() and np.isfinite(wv).all()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_norm_is_bit_exact_where_the_squares_sum_exactly(n, offset):
    """Inputs whose squares sum exactly in float64 in any order (test_sgd_host.exact_sum_inputs; the property is checked here on the
    host): the norm equals the oracle's bit for bit, whatever order the kernel adds in.  Two calls give the same bits."""
    import sehip
    n = _big_n(sehip.SGD_MAX_BLOCKS) if n == "big" else n
    g, p, l2 = exact_sum_inputs(n, 300 + n % 89)
    g2 = g.astype(np.float64) + l2.astype(np.float64) * p.astype(np.float64)
    assert np.array_equal((g + l2 * p).astype(np.float64), g2)                       # the float32 g2 is exact
    sq = g2 * g2
    assert np.all(sq * 2.0 ** 12 == np.rint(sq * 2.0 ** 12)) and sq.max() < 2.0 ** 8 and n < 2 ** 28      # multiples of 2^-12: any partial sum is exact
    gd, pd, ld = _dev(g, offset), _dev(p, offset), _dev(l2, offset)
    for with_l2 in (True, False):
        want_norm, want_factor = clip_oracle(g, p, l2 if with_l2 else None, 1.0, 1.0)
        a = sehip.grad_clip_factor(gd, pd if with_l2 else None, ld if with_l2 else None, clipnorm=1.0)
        b = sehip.grad_clip_factor(gd, pd if with_l2 else None, ld if with_l2 else None, clipnorm=1.0)
        assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(a), _bits(np.array([want_norm, want_factor], dtype=F))), (n, offset, with_l2)
    assert np.array_equal(_bits(gd), _bits(g)) and np.array_equal(_bits(pd), _bits(p))


def test_clip_active_inactive_and_all_zero():
    import sehip
    n = 4103
    _, _, gh, _ = sgd_inputs(n, 31, with_l2=False)
    g = _dev(gh, 0)
    norm = float(clip_oracle(gh, None, None, 1.0, 1.0)[0])
    active = sehip.grad_clip_factor(g, clipnorm=norm / 4).cpu().numpy()
    assert active[1] < 1 and abs(active[1] - 0.25) < 1e-6 and _bits(active[1]) == _bits(clip_factor(active[0], norm / 4))
    inactive = sehip.grad_clip_factor(g, clipnorm=norm * 4).cpu().numpy()
    assert _bits(inactive[1]) == _bits(F(1.0)) and _bits(inactive[0]) == _bits(active[0])
    z = torch.zeros(n, dtype=torch.float32, device="cuda")
    for l2 in (None, torch.full((n,), 4e-4, dtype=torch.float32, device="cuda")):
        zero = sehip.grad_clip_factor(z, z.clone(), l2, grad_scale=0.5, clipnorm=10.0).cpu().numpy()
        assert _bits(zero[0]) == 0 and _bits(zero[1]) == _bits(F(1.0))                # norm +0, factor exactly 1
    # zeros stay +0 through the update, with the clip factor of a zero gradient and with an active one
    for clip in (None, torch.tensor([1.0], device="cuda"), torch.tensor([0.25], device="cuda")):
        for nesterov in (False, True):
            p, v = z.clone(), z.clone()
            sehip.sgd_step_(p, v, z, torch.full((n,), 4e-4, device="cuda"), lr=LR, grad_scale=0.5, clip=clip, momentum=MOM, nesterov=nesterov)
            assert not _bits(p).any() and not _bits(v).any() and not _bits(z).any()
    out = torch.tensor([7.0, 7.0], device="cuda")
    empty = torch.zeros(0, device="cuda")
    assert sehip.grad_clip_factor(empty, clipnorm=1.0, out=out) is out and out.tolist() == [7.0, 7.0]     # n = 0 leaves stats alone
    assert sehip.sgd_step_(empty, empty.clone(), empty.clone(), lr=LR) is empty


def test_non_finite_gradients_give_nan_where_the_oracle_has_nan():
    import sehip
    n = 1031
    ph, vh, gh, l2h = sgd_inputs(n, 11)
    gnan, ginf = gh.copy(), gh.copy()
    gnan[5], gnan[64], gnan[700], gnan[n - 1] = np.nan, np.inf, -np.inf, np.nan
    ginf[64], ginf[700] = np.inf, -np.inf
    for offset, l2 in ((0, None), (0, l2h), (1, l2h)):
        l2d = None if l2 is None else _dev(l2, offset)
        for bad, nan_norm in ((gnan, True), (ginf, False)):
            p, v, g = _dev(ph, offset), _dev(vh, offset), _dev(bad, offset)
            stats = sehip.grad_clip_factor(g, p, l2d, clipnorm=10.0)
            norm, factor = stats.cpu().numpy()
            want = clip_oracle(bad, ph, l2, 1.0, 10.0)
            if nan_norm:
                assert np.isnan(norm) and np.isnan(factor) and np.isnan(want[0]) and np.isnan(want[1])
            else:
                assert norm == np.inf and _bits(factor) == 0 and want[0] == np.inf and _bits(want[1]) == 0      # an infinite norm: factor +0
            for clip in (None, stats[1:]):
                p, v = _dev(ph, offset), _dev(vh, offset)
                sehip.sgd_step_(p, v, g, l2d, lr=LR, clip=clip, momentum=MOM)
                wp, wv = sgd_oracle(ph, vh, bad, l2, LR, 1.0, None if clip is None else factor, MOM)
                gp, gv = p.cpu().numpy(), v.cpu().numpy()
                # NaN gradients give NaN; an infinite one gives +-inf, or NaN under the factor 0 of its infinite norm; a NaN factor
                # spreads everywhere
                nans = (n if clip is not None else 2) if nan_norm else (2 if clip is not None else 0)
                assert np.isnan(wp).sum() == nans == np.isnan(wv).sum() and np.isinf(wp).sum() == (2 if clip is None else 0)
                assert np.array_equal(np.isnan(gp), np.isnan(wp)) and np.array_equal(np.isnan(gv), np.isnan(wv))
                ok = ~np.isnan(wp)
                assert np.array_equal(gp[ok].view(np.int32), wp[ok].view(np.int32))
                assert np.array_equal(gv[ok].view(np.int32), wv[ok].view(np.int32))


def test_captured_clip_and_step_follow_the_learning_rate_without_allocating():
    import sehip
    n = 4103
    ph, vh, gh, l2h = sgd_inputs(n, 21)
    p, v, g, l2 = (_dev(a, 0) for a in (ph, vh, gh, l2h))
    lr = torch.full((), 1.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(sehip.SGD_MAX_BLOCKS * 8, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(2, dtype=torch.float32, device="cuda")
    clip = stats[1:]
    clipnorm = 20.0
    sehip.grad_clip_factor(g, p, l2, grad_scale=0.5, clipnorm=clipnorm, workspace=ws, out=stats)      # loads the library before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        sehip.grad_clip_factor(g, p, l2, grad_scale=0.5, clipnorm=clipnorm, workspace=ws, out=stats)
        sehip.sgd_step_(p, v, g, l2, lr=lr, grad_scale=0.5, clip=clip, momentum=MOM, nesterov=True)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before      # workspace and stats were passed in
    want_norm, want_factor = clip_oracle(gh, ph, l2h, 0.5, clipnorm)
    assert want_factor < 1
    for value in (0.01, 0.003):
        p.copy_(torch.from_numpy(ph))
        v.copy_(torch.from_numpy(vh))
        stats.zero_()
        lr.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        ep, ev = _dev(ph, 0), _dev(vh, 0)
        es = sehip.grad_clip_factor(g, ep, l2, grad_scale=0.5, clipnorm=clipnorm)
        sehip.sgd_step_(ep, ev, g, l2, lr=value, grad_scale=0.5, clip=es[1:], momentum=MOM, nesterov=True)
        assert torch.equal(stats.view(torch.int32), es.view(torch.int32))
        assert torch.equal(p.view(torch.int32), ep.view(torch.int32)) and torch.equal(v.view(torch.int32), ev.view(torch.int32))
        norm, factor = stats.cpu().numpy()
        assert abs(int(_bits(norm)) - int(_bits(want_norm))) <= 1 and _bits(factor) == _bits(clip_factor(norm, clipnorm))
        wp, wv = sgd_oracle(ph, vh, gh, l2h, value, 0.5, factor, MOM, True)
        assert np.array_equal(_bits(p), _bits(wp)) and np.array_equal(_bits(v), _bits(wv))


def test_binding_checks_its_tensors():
    import sehip
    p = torch.zeros(8, device="cuda")
    with pytest.raises(sehip.SehipError):
        sehip.sgd_step_(p, p.clone(), torch.zeros(7, device="cuda"), lr=LR)
    with pytest.raises(sehip.SehipError):
        sehip.sgd_step_(p, p.clone(), p.clone().double(), lr=LR)
    with pytest.raises(sehip.SehipError):
        sehip.sgd_step_(p, p.clone(), p.clone(), lr=torch.zeros(2, device="cuda"))
    with pytest.raises(sehip.SehipError):
        sehip.sgd_step_(p, p.clone(), p.clone(), lr=LR, momentum=-1.0)
    with pytest.raises(sehip.SehipError):
        sehip.sgd_step_(p, p.clone(), p.clone(), lr=LR, clip=torch.zeros(1))
    with pytest.raises(sehip.SehipError):
        sehip.grad_clip_factor(p, p.clone(), torch.zeros(7, device="cuda"), clipnorm=1.0)
    with pytest.raises(sehip.SehipError):
        sehip.grad_clip_factor(p, None, p.clone(), clipnorm=1.0)                      # l2 without p
    with pytest.raises(sehip.SehipError):
        sehip.grad_clip_factor(p, clipnorm=0.0)
    with pytest.raises(sehip.SehipError):
        sehip.grad_clip_factor(p, clipnorm=1.0, workspace=torch.zeros(8, device="cuda"))      # too small
    with pytest.raises(sehip.SehipError):
        sehip.grad_clip_factor(p, clipnorm=1.0, out=torch.zeros(3, device="cuda"))


def test_trainer_fused_sgd_on_the_flat_buffers():
    """One eager step of Trainer(fused_sgd=True, clipnorm=0.05) equals sgd_oracle on (weights before, flat_g, zero velocity, flat_l2)
    with the factor of trainer.grad_stats bit for bit; flat_g is left alone; the padding words stay +0; a second step carries the
    velocity; a default trainer given the SAME flat_g agrees within the rounding bound of the host test; enable_graphs leaves the
    state alone, and graph B writes the bits of the eager apply_update.

    The bound against the composition (test_sgd_host.test_oracle_agrees_with_the_torch_composition...: a = u lr f |l2 p|, b =
    u |step|, e_v = a + b + 2 u |v'|, plain e_p = e_v + 2 u |p'|) plus what the clip factor adds here: the composition's factor comes
    from torch's float32 norm, granted 1e-5 relative as in the Adagrad clip test, so the two steps differ by 1e-5 |step| more."""
    import utils
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(0)
    C, D, B, lr, clip, mom = 100, 64, 32, 0.01, 0.05, 0.9
    model = utils.build_network(D, "resnet-32", input_channels=3).cuda()
    E = torch.nn.functional.normalize(torch.randn(C, D), dim=-1).cuda()
    losses = {"embedding": (utils.CosineEmbeddingLoss(E), 1.0)}
    l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
    import copy
    twin = copy.deepcopy(model)
    kw = dict(lr=lr, momentum=mom, clipnorm=clip, autocast_dtype=None, memory_format=torch.contiguous_format)
    tr = Trainer(model, losses, {}, l2_of=l2_of, fused_sgd=True, **kw)
    flat = tr.flat
    assert flat.has_l2 and flat.total > sum(n for _, n in flat.offsets)          # regularisers and padding words are present
    assert tr.grad_stats is not None and tr.grad_stats.is_cuda and tuple(tr.grad_stats.shape) == (2,)
    pad = torch.ones(flat.total, dtype=torch.bool, device="cuda")
    for off, n in flat.offsets:
        pad[off:off + n] = False
    l2 = flat.flat_l2.cpu().numpy()
    X, y = SyntheticGenerator(C, 32, 3, 64, 32).train_sequence(B, shuffle=False)[0]
    X = X.contiguous()

    # step 1, in its two halves: the update must not touch the gradient
    p0, v0 = flat.flat_p.cpu().numpy(), flat.flat_v.cpu().numpy()
    assert not v0.any()
    tr._eager_core(X, y, {})
    g1 = flat.flat_g.clone()
    tr.apply_update(1.0)
    assert torch.equal(flat.flat_g.view(torch.int32), g1.view(torch.int32)) and tr.iterations == 1
    norm, factor = tr.grad_stats.cpu().numpy()
    tnorm = float(torch.linalg.vector_norm(g1 + flat.flat_l2 * torch.from_numpy(p0).cuda()))
    assert tnorm > clip and factor < 1                                             # the clip is active
    assert abs(float(norm) - tnorm) <= 1e-5 * tnorm and _bits(factor) == _bits(clip_factor(norm, clip))
    wp, wv = sgd_oracle(p0, v0, g1.cpu().numpy(), l2, lr, 1.0, factor, mom, False)
    assert np.array_equal(_bits(flat.flat_p), _bits(wp)) and np.array_equal(_bits(flat.flat_v), _bits(wv))
    assert (wp != p0).any() and np.isfinite(wp).all()

    # a default trainer on a copy of the model, given the same gradient
    l2_twin = {id(p): twin.regularizer for p in twin.regularized_parameters()}
    ref = Trainer(twin, {"embedding": (utils.CosineEmbeddingLoss(E), 1.0)}, {}, l2_of=l2_twin, **kw)
    assert not ref.fused_sgd and np.array_equal(_bits(ref.flat.flat_p), _bits(p0))
    ref.flat.flat_g.copy_(g1)
    ref.apply_update(1.0)
    a64 = np.float64
    step = np.abs(a64(F(lr)) * ((g1.cpu().numpy().astype(a64) + l2.astype(a64) * p0) * a64(factor)))
    e_a = U * np.abs(l2.astype(a64) * p0) * float(factor) * lr * (1 + 8 * U)
    e_v = e_a + U * step * (1 + 8 * U) + 1e-5 * step + 2 * U * np.abs(wv)
    e_p = e_v + 2 * U * np.abs(wp)
    assert np.all(np.abs(ref.flat.flat_v.cpu().numpy().astype(a64) - wv) <= e_v)
    assert np.all(np.abs(ref.flat.flat_p.cpu().numpy().astype(a64) - wp) <= e_p)
    ref.close()

    # step 2 through train_step: the velocity carries
    logs = {}
    tr.train_step(X, y, logs)
    factor2 = tr.grad_stats.cpu().numpy()[1]
    wp2, wv2 = sgd_oracle(wp, wv, flat.flat_g.cpu().numpy(), l2, lr, 1.0, factor2, mom, False)
    assert np.array_equal(_bits(flat.flat_p), _bits(wp2)) and np.array_equal(_bits(flat.flat_v), _bits(wv2))
    assert tr.iterations == 2 and float(logs["_n"]) == B
    for buf in (flat.flat_p, flat.flat_v, flat.flat_g, flat.flat_l2):
        assert not buf[pad].view(torch.int32).any()                               # +0 bitwise

    # graph mode: the capture's warm-up steps leave no trace; replayed steps move the weights
    v_before, p_before = flat.flat_v.clone(), flat.flat_p.clone()
    assert tr.enable_graphs(X, y)
    assert torch.equal(flat.flat_v.view(torch.int32), v_before.view(torch.int32))
    assert torch.equal(flat.flat_p.view(torch.int32), p_before.view(torch.int32)) and tr.iterations == 2
    for _ in range(2):
        tr.train_step(X, y, {})
    torch.cuda.synchronize()
    assert tr.iterations == 4 and bool((flat.flat_p != p_before).any()) and bool(torch.isfinite(flat.flat_p).all())
    assert not flat.flat_p[pad].view(torch.int32).any() and not flat.flat_v[pad].view(torch.int32).any()
    # with flat_g held fixed, graph B writes the bits of the eager apply_update at the same learning rate
    g_fix, p_fix, v_fix = flat.flat_g.clone(), flat.flat_p.clone(), flat.flat_v.clone()
    tr._lr_t.fill_(lr)
    tr._graph[1].replay()
    torch.cuda.synchronize()
    p_graph, v_graph, s_graph = flat.flat_p.clone(), flat.flat_v.clone(), tr.grad_stats.clone()
    assert torch.equal(flat.flat_g.view(torch.int32), g_fix.view(torch.int32))
    flat.flat_p.copy_(p_fix)
    flat.flat_v.copy_(v_fix)
    tr.apply_update(1.0, count=False)
    assert torch.equal(flat.flat_p.view(torch.int32), p_graph.view(torch.int32))
    assert torch.equal(flat.flat_v.view(torch.int32), v_graph.view(torch.int32))
    assert torch.equal(tr.grad_stats.view(torch.int32), s_graph.view(torch.int32)) and bool((p_graph != p_fix).any())
    tr.close()
