"""GPU: se_adagrad_step bit for bit against the float32 NumPy oracle of test_adagrad_host.py -- every path (16-byte, scalar, tail,
more than one trip of the grid-stride loop), regulariser / scale / device learning rate, zeros, non-finite gradients, HIP-graph
capture -- and engine.Trainer(optimizer='adagrad') on the flat buffers of a ResNet-32 under the DeViSE loss."""
import itertools

import numpy as np
import pytest
import torch

from _flat_buffers import SIZES, _big_n, _bits, _dev
from test_adagrad_host import F, adagrad_inputs, adagrad_oracle

pytestmark = pytest.mark.gpu

LR, EPS = 0.01, 1e-7


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
def test_three_steps_are_bit_exact(n, offset):
    import sehip
    n = _big_n(sehip.ADAGRAD_MAX_BLOCKS) if n == "big" else n
    p0, a0, g0, l20 = adagrad_inputs(n, 100 + n % 97)
    grads = [g0] + [adagrad_inputs(n, 200 + s + n % 97)[2] for s in (1, 2)]
    for with_l2, scale, lr_on_device in itertools.product((False, True), (1.0, 0.5), (False, True)):
        p, a = _dev(p0, offset), _dev(a0, offset)
        l2 = _dev(l20, offset) if with_l2 else None
        lr = torch.full((), LR, dtype=torch.float32, device="cuda") if lr_on_device else LR
        wp, wa = p0, a0
        for step, gh in enumerate(grads):
            g = _dev(gh, offset)
            sehip.adagrad_step_(p, a, g, l2, lr=lr, grad_scale=scale, epsilon=EPS)
            wp, wa = adagrad_oracle(wp, wa, gh, l20 if with_l2 else None, LR, scale, EPS)
            what = (n, offset, with_l2, scale, lr_on_device, step)
            assert np.array_equal(_bits(g), _bits(gh)), what                      # g is only read
            assert np.array_equal(_bits(a), _bits(wa)), what
            assert np.array_equal(_bits(p), _bits(wp)), what
        assert np.isfinite(wp).all() and (wa > 0).all()


def test_zeros_stay_zero_and_frozen_parameters_stay_put():
    import sehip
    for n, offset in ((4103, 0), (4103, 1)):
        z = np.zeros(n, dtype=F)
        l2h = np.full(n, 4e-4, dtype=F)
        for l2 in (None, l2h):
            p, a, g = _dev(z, offset), _dev(z, offset), _dev(z, offset)
            sehip.adagrad_step_(p, a, g, None if l2 is None else _dev(l2, offset), lr=LR, grad_scale=0.5)
            assert not _bits(p).any() and not _bits(a).any() and not _bits(g).any()       # +0 bitwise
        # a parameter without a gradient whose accumulator already holds something: nothing moves
        ph, ah, _, _ = adagrad_inputs(n, 7)
        ah = np.abs(ph) + F(0.5)
        p, a = _dev(ph, offset), _dev(ah, offset)
        sehip.adagrad_step_(p, a, _dev(z, offset), None, lr=LR)
        assert np.array_equal(_bits(p), _bits(ph)) and np.array_equal(_bits(a), _bits(ah))


def test_non_finite_gradients_give_nan_where_the_oracle_has_nan():
    import sehip
    n = 1031
    ph, _, gh, l2h = adagrad_inputs(n, 11)
    ah = np.full(n, 0.25, dtype=F)
    gh[5], gh[64], gh[700], gh[n - 1] = np.nan, np.inf, -np.inf, np.nan
    for offset, l2 in ((0, None), (0, l2h), (1, l2h)):
        p, a = _dev(ph, offset), _dev(ah, offset)
        sehip.adagrad_step_(p, a, _dev(gh, offset), None if l2 is None else _dev(l2, offset), lr=LR)
        torch.cuda.synchronize()
        wp, wa = adagrad_oracle(ph, ah, gh, l2, LR)
        gp, ga = p.cpu().numpy(), a.cpu().numpy()
        assert np.isnan(wp).sum() == 4 and np.isnan(wa).sum() == 2
        assert np.array_equal(np.isnan(gp), np.isnan(wp)) and np.array_equal(np.isnan(ga), np.isnan(wa))
        ok = ~np.isnan(wp)
        assert np.array_equal(gp[ok].view(np.int32), wp[ok].view(np.int32))
        ok = ~np.isnan(wa)
        assert np.array_equal(ga[ok].view(np.int32), wa[ok].view(np.int32))


def test_captured_step_reads_the_learning_rate_on_the_device():
    import sehip
    n = 4103
    ph, ah, gh, l2h = adagrad_inputs(n, 21)
    p, a, g, l2 = (_dev(v, 0) for v in (ph, ah, gh, l2h))
    lr = torch.full((), 1.0, dtype=torch.float32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sehip.adagrad_step_(p, a, g, l2, lr=lr, grad_scale=0.5)
    for value in (0.01, 0.003):
        p.copy_(torch.from_numpy(ph))
        a.copy_(torch.from_numpy(ah))
        lr.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        ep, ea = _dev(ph, 0), _dev(ah, 0)
        sehip.adagrad_step_(ep, ea, g, l2, lr=value, grad_scale=0.5)
        assert torch.equal(p.view(torch.int32), ep.view(torch.int32)) and torch.equal(a.view(torch.int32), ea.view(torch.int32))
        wp, wa = adagrad_oracle(ph, ah, gh, l2h, value, 0.5)
        assert np.array_equal(_bits(p), _bits(wp)) and np.array_equal(_bits(a), _bits(wa))


def test_binding_checks_its_tensors():
    import sehip
    p = torch.zeros(8, device="cuda")
    with pytest.raises(sehip.SehipError):
        sehip.adagrad_step_(p, p.clone(), torch.zeros(7, device="cuda"), lr=LR)
    with pytest.raises(sehip.SehipError):
        sehip.adagrad_step_(p, p.clone(), p.clone().double(), lr=LR)
    with pytest.raises(sehip.SehipError):
        sehip.adagrad_step_(p, p.clone(), p.clone(), lr=torch.zeros(2, device="cuda"))
    with pytest.raises(sehip.SehipError):
        sehip.adagrad_step_(p, p.clone(), p.clone(), lr=LR, epsilon=-1.0)
    empty = torch.zeros(0, device="cuda")
    assert sehip.adagrad_step_(empty, empty.clone(), empty.clone(), lr=LR) is empty


def test_trainer_adagrad_on_the_flat_buffers():
    """Two eager steps of Trainer(optimizer='adagrad') equal the oracle on (weights before, flat_g, accumulator before, flat_l2) bit
    for bit, the padding words between the parameter slices stay +0, the update leaves flat_g alone; enable_graphs restores the
    accumulator, and replayed steps train."""
    import learn_devise as ld
    import utils
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(0)
    C, D, B, lr = 100, 64, 32, 0.01
    model = utils.build_network(D, "resnet-32", input_channels=3).cuda()
    E = torch.nn.functional.normalize(torch.randn(C, D), dim=-1).cuda()
    losses, metrics = ld.build_losses(E, 0.1)
    l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
    tr = Trainer(model, losses, metrics, lr=lr, l2_of=l2_of, autocast_dtype=None, memory_format=torch.contiguous_format,
                 optimizer="adagrad", momentum=0.9, nesterov=True)               # momentum / nesterov: ignored
    flat = tr.flat
    assert flat.has_l2 and flat.total > sum(n for _, n in flat.offsets)          # regularisers and padding words are present
    pad = torch.ones(flat.total, dtype=torch.bool, device="cuda")
    for off, n in flat.offsets:
        pad[off:off + n] = False
    l2 = flat.flat_l2.cpu().numpy()
    gen = SyntheticGenerator(C, 32, 3, 64, 32)
    seq = gen.train_sequence(B, shuffle=False, batch_transform=ld.transform_inputs, batch_transform_kwargs={"embedding": None})
    X, y = seq[0]
    X = X.contiguous()

    # step 1, in its two halves: the update must not touch the gradient
    p0, v0 = flat.flat_p.cpu().numpy(), flat.flat_v.cpu().numpy()
    assert not v0.any()
    tr._eager_core(X, y, {})
    g1 = flat.flat_g.clone()
    tr.apply_update(1.0)
    assert torch.equal(flat.flat_g.view(torch.int32), g1.view(torch.int32)) and tr.iterations == 1
    wp, wv = adagrad_oracle(p0, v0, g1.cpu().numpy(), l2, lr)
    assert np.array_equal(_bits(flat.flat_p), _bits(wp)) and np.array_equal(_bits(flat.flat_v), _bits(wv))
    assert (wp != p0).any() and np.isfinite(wp).all()
    # step 2 through train_step: the accumulator carries
    logs = {}
    tr.train_step(X, y, logs)
    wp2, wv2 = adagrad_oracle(wp, wv, flat.flat_g.cpu().numpy(), l2, lr)
    assert np.array_equal(_bits(flat.flat_p), _bits(wp2)) and np.array_equal(_bits(flat.flat_v), _bits(wv2))
    assert (wv2 >= wv).all() and (wv2 > wv).any() and float(logs["_n"]) == B and "max_sim_acc" in logs
    for buf in (flat.flat_p, flat.flat_v, flat.flat_g, flat.flat_l2):
        assert not buf[pad].view(torch.int32).any()                               # +0 bitwise

    # graph mode: the capture's warm-up steps leave no trace in the accumulator; replayed steps move the weights
    v_before, p_before = flat.flat_v.clone(), flat.flat_p.clone()
    assert tr.enable_graphs(X, y)
    assert torch.equal(flat.flat_v.view(torch.int32), v_before.view(torch.int32))
    assert torch.equal(flat.flat_p.view(torch.int32), p_before.view(torch.int32)) and tr.iterations == 2
    for _ in range(2):
        tr.train_step(X, y, {})
    torch.cuda.synchronize()
    assert tr.iterations == 4 and bool((flat.flat_p != p_before).any()) and bool((flat.flat_v >= v_before).all())
    assert bool(torch.isfinite(flat.flat_p).all()) and bool(torch.isfinite(flat.flat_v).all())
    assert not flat.flat_p[pad].view(torch.int32).any() and not flat.flat_v[pad].view(torch.int32).any()


def test_trainer_adagrad_with_clipnorm_clips_in_front_of_the_kernel():
    """With clipnorm the scale / regulariser / clip lines of the SGD path run first (flat_g then holds the clipped, regularised
    gradient) and the kernel gets that gradient with scale 1 and no regulariser of its own."""
    import learn_devise as ld
    import utils
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(1)
    C, D, B, lr, clip = 100, 64, 32, 0.01, 0.05
    model = utils.build_network(D, "resnet-32", input_channels=3).cuda()
    E = torch.nn.functional.normalize(torch.randn(C, D), dim=-1).cuda()
    losses, metrics = ld.build_losses(E, 0.1)
    l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
    tr = Trainer(model, losses, metrics, lr=lr, clipnorm=clip, l2_of=l2_of, autocast_dtype=None, memory_format=torch.contiguous_format,
                 optimizer="adagrad")
    flat = tr.flat
    X, y = SyntheticGenerator(C, 32, 3, 64, 32).train_sequence(B, shuffle=False)[0]
    p0 = flat.flat_p.clone()
    tr._eager_core(X.contiguous(), y, {})
    raw = flat.flat_g.clone()
    tr.apply_update(1.0)
    reg = raw + flat.flat_l2 * p0
    norm = float(torch.linalg.vector_norm(reg))
    assert norm > clip                                                            # the clip is active
    g = flat.flat_g
    assert abs(float(torch.linalg.vector_norm(g)) - clip) < 1e-5 * clip
    assert torch.allclose(g, reg * (clip / norm), rtol=1e-5, atol=1e-9)     # atol: addcmul_ may fuse l2 * p into the sum
    wp, wv = adagrad_oracle(p0.cpu().numpy(), np.zeros(flat.total, dtype=F), g.cpu().numpy(), None, lr)
    assert np.array_equal(_bits(flat.flat_p), _bits(wp)) and np.array_equal(_bits(flat.flat_v), _bits(wv))
