"""GPU: the Plain-11 and PyramidNet backbones on the device -- the fused shortcut kernel against the torch composition inside a small
PyramidNet, engine.Trainer steps (HIP-graph replay offered) on both, and learn_image_embeddings with its default architecture."""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_BLOCKS = 6                       # PyramidNet(depth 20, alpha 12, bottleneck): n = 2, widths 18 .. 28


def small_pyramidnet(fused, classes=10, seed=11):
    from models.cifar_pyramidnet import PyramidNet
    torch.manual_seed(seed)
    return PyramidNet(20, 12, bottleneck=True, top_activation=None, classes=classes, fused_shortcut=fused).cuda()


def test_fused_shortcut_matches_the_torch_composition_in_a_small_pyramidnet():
    """Same seed, same batch, one backward: fused_shortcut=True against False, float32, training mode.

    Tolerance, derived and not measured.  Both networks run the same operations except the 6 shortcut adds.  Each of the two
    implementations of a shortcut add stays within (stride^2 + 1) 2^-24 (|pooled| + |s|) of the exact value (tests/
    test_gpu_shortcut_add.py), so they differ from each other by at most EPS = 2 (2^2 + 1) 2^-24 = 6.0e-7 relative to the block output
    (at stride 1 both compute the single float32 add s + x: no difference at all; the budget takes stride 2 for every block).
    A relative perturbation of a block's output travels through the blocks behind it; a residual block is the identity plus a
    branch that starts and ends in a batch normalisation (unit gain), so it at most doubles a relative perturbation: GAIN = 2 per
    block.  Outputs: the 6 blocks' perturbations, each through at most 6 blocks: 6 EPS 2^6 = 2.3e-4 relative.  Gradients go forward and
    back through the same blocks: 6 EPS 2^12 = 1.5e-2 of the whole gradient's norm.  A wrong shortcut (padding on the other side, a
    missing division, the wrong window) changes outputs and gradients by their own size."""
    eps = 2 * (2 * 2 + 1) * 2.0 ** -24
    tol_out, tol_grad = N_BLOCKS * eps * 2.0 ** N_BLOCKS, N_BLOCKS * eps * 2.0 ** (2 * N_BLOCKS)
    x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(12)).cuda()
    w = torch.randn(4, 10, generator=torch.Generator().manual_seed(13)).cuda()
    results = {}
    for fused in (True, False):
        net = small_pyramidnet(fused).train()
        assert len(net.blocks) == N_BLOCKS and [b.stride for b in net.blocks] == [1, 1, 2, 1, 2, 1]
        out = net(x)
        (out * w).sum().backward()
        results[fused] = (out.detach().double(), [(n, p.grad.detach().double()) for n, p in net.named_parameters()])
    (out_f, grads_f), (out_t, grads_t) = results[True], results[False]
    assert torch.isfinite(out_f).all() and out_t.norm() > 0
    assert float((out_f - out_t).norm() / out_t.norm()) <= tol_out
    whole = float(torch.sqrt(sum(g.square().sum() for _, g in grads_t)))
    assert whole > 0 and len(grads_f) == len(grads_t) > 50
    total = 0.0
    for (name, gf), (_, gt) in zip(grads_f, grads_t):
        assert torch.isfinite(gf).all(), name
        d = float((gf - gt).norm())
        assert d <= tol_grad * whole, (name, d, whole)
        total += d * d
    assert total ** 0.5 <= tol_grad * whole


def test_fused_shortcut_is_what_the_device_model_runs(monkeypatch):
    """fused_shortcut=True on device tensors goes through sehip.shortcut_add once per block (and never with False)."""
    import sehip
    from models import cifar_pyramidnet
    calls = []
    real = sehip.shortcut_add
    monkeypatch.setattr(cifar_pyramidnet.sehip, "shortcut_add", lambda s, x, stride=1, pad=0: (calls.append((stride, pad)), real(s, x, stride, pad))[1])
    x = torch.randn(2, 3, 16, 16, device="cuda")
    with torch.no_grad():
        small_pyramidnet(True).eval()(x)
    assert calls == [(1, 0), (1, 0), (2, 0), (1, 0), (2, 0), (1, 0)]
    del calls[:]
    with torch.no_grad():
        small_pyramidnet(False).eval()(x)
    assert calls == []


@pytest.mark.parametrize("arch", ["simple", "small-pyramidnet"])
def test_trainer_steps_with_graph_replay_offered(arch):
    """A few engine.Trainer steps in the CIFAR-sized group's default mode (float32, NCHW, HIP-graph replay offered): enable_graphs
    validates its replay against eager steps and either accepts or falls back cleanly; the steps are finite either way and the
    parameters move."""
    import utils
    from datasets import SyntheticGenerator
    from engine import Trainer, backbone_mode
    size = 32 if arch == "simple" else 16
    E = torch.nn.functional.normalize(torch.randn(10, 10, generator=torch.Generator().manual_seed(2)), dim=-1).cuda()
    adt, fmt = backbone_mode("simple" if arch == "simple" else "pyramidnet-272-200")
    assert adt is None and fmt == torch.contiguous_format
    torch.manual_seed(3)
    model = utils.build_network(10, "simple").cuda() if arch == "simple" else small_pyramidnet(True)
    l2 = {id(p): model.regularizer for p in model.regularized_parameters()}
    tr = Trainer(model, {"l2norm": (utils.CosineEmbeddingLoss(E), 1.0)}, {"l2norm": [utils.nn_accuracy(E, dot_prod_sim=True)]},
                 lr=0.05, clipnorm=10.0, l2_of=l2, autocast_dtype=adt, memory_format=fmt)
    seq = SyntheticGenerator(10, size, 3, 64, 16).train_sequence(16, shuffle=False)
    before = tr.flat.flat_p.clone()
    ok = tr.enable_graphs(*seq[0])
    assert ok in (True, False) and (tr._graph is not None) == ok
    assert torch.equal(tr.flat.flat_p, before)                      # capture and validation leave the state alone
    logs = {}
    losses = [float(tr.train_step(*seq[i % len(seq)], logs)) for i in range(4)]
    torch.cuda.synchronize()
    assert np.isfinite(losses).all() and torch.isfinite(tr.flat.flat_p).all()
    assert not torch.equal(tr.flat.flat_p, before)
    tr.close()


def test_learn_image_embeddings_runs_with_its_default_architecture(tmp_path):
    """The reference's command line with no --architecture: Plain-11, one epoch on a synthetic dataset."""
    import learn_image_embeddings as lie
    rng = np.random.default_rng(4)
    E = rng.standard_normal((10, 10)).astype(np.float32)
    E /= np.linalg.norm(E, axis=-1, keepdims=True)
    emb = str(tmp_path / "emb.pickle")
    with open(emb, "wb") as f:
        pickle.dump({"embedding": E, "ind2label": list(range(10)), "label2ind": {i: i for i in range(10)}}, f)
    assert lie.build_parser().get_default("architecture") == "simple"
    final = lie.main(["--dataset", "synthetic:10x32x64x32", "--data_root", "-", "--embedding", emb, "--epochs", "1", "--batch_size", "32",
                      "--val_batch_size", "32", "--lr_schedule", "SGD", "--sgd_lr", "0.05", "--no_progress"])
    assert final and all(np.isfinite(v) for v in final.values()), final
    assert np.isfinite(final["loss"]) and 0.0 <= final["max_sim_acc"] <= 1.0
