"""The embedding heads in the training loop: utils.CosineEmbeddingHead / SquaredDistanceHead log and differentiate what the separate
loss object + one utils.nn_accuracy per metric do, bit for bit, in one se_embed_head_fwd launch; a metric called on other tensors than
the head's last ones falls back to se_nn_accuracy; learn_image_embeddings.py trains with them."""
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, D, C = 64, 100, 100


def _setup(seed=0):
    gen = torch.Generator().manual_seed(seed)
    emb = torch.nn.functional.normalize(torch.randn((C, D), generator=gen), dim=1).cuda()
    outs = torch.randn((B, D), generator=gen).cuda()
    y = torch.randint(0, C, (B,), generator=gen).cuda()
    return emb, outs, y


def _objects(kind, head, emb, ks):
    import utils
    if head:
        loss = (utils.CosineEmbeddingHead if kind == "cosine" else utils.SquaredDistanceHead)(emb)
        return loss, [loss.accuracy()] + [loss.accuracy(k) for k in ks]
    loss = (utils.CosineEmbeddingLoss if kind == "cosine" else utils.SquaredDistanceLoss)(emb)
    dot = kind == "cosine"
    return loss, [utils.nn_accuracy(emb, dot_prod_sim=dot)] + [utils.nn_accuracy(emb, dot_prod_sim=dot, k=k) for k in ks]


def _trainer(loss, metrics):
    import engine
    model = torch.nn.Linear(2, 2).cuda()
    return engine.Trainer(model, {"embedding": (loss, 1.0)}, {"embedding": metrics}, autocast_dtype=None)


def _step(kind, head, emb, outs, y, ks):
    loss, metrics = _objects(kind, head, emb, ks)
    tr = _trainer(loss, metrics)
    o = outs.clone().requires_grad_(True)
    logs = {}
    total = tr._loss_and_metrics((o,), y, logs)
    total.backward()
    tr.close() if hasattr(tr, "close") else None
    return logs, o.grad, total.detach()


@pytest.mark.parametrize("kind", ["cosine", "sqdist"])
def test_logs_and_gradient_equal_the_separate_objects(kind):
    emb, outs, y = _setup()
    logs_h, grad_h, total_h = _step(kind, True, emb, outs, y, (5,))
    logs_p, grad_p, total_p = _step(kind, False, emb, outs, y, (5,))
    names = ("max_sim_acc", "max_sim_acc5") if kind == "cosine" else ("nn_accuracy", "nn_accuracy5")
    assert sorted(logs_h) == sorted(logs_p) == sorted(("loss", "_n") + names)
    for key in logs_p:
        a, b = torch.as_tensor(logs_h[key]).float().cpu(), torch.as_tensor(logs_p[key]).float().cpu()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), key
    assert torch.equal(grad_h.view(torch.int32), grad_p.view(torch.int32))
    assert torch.equal(total_h.view(torch.int32), total_p.view(torch.int32))
    assert 0 < float(logs_h[names[1]]) <= B          # the metric is not vacuous on these inputs


class _Spy(object):
    def __init__(self, monkeypatch):
        import sehip.ops as ops
        self.names = []
        real = ops.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(ops, "call", call)

    def count(self, name):
        return self.names.count(name)


@pytest.mark.parametrize("kind", ["cosine", "sqdist"])
def test_one_launch_serves_the_loss_and_every_k(kind, monkeypatch):
    emb, outs, y = _setup(1)
    sibling = "se_cosine_loss_fwd" if kind == "cosine" else "se_sqdist_loss_fwd"
    spy = _Spy(monkeypatch)
    _step(kind, True, emb, outs, y, (5, 10))
    assert spy.count("se_embed_head_fwd") == 1
    assert spy.count("se_nn_accuracy") == 0 and spy.count(sibling) == 0
    spy.names.clear()
    _step(kind, False, emb, outs, y, (5, 10))
    assert spy.count(sibling) == 1 and spy.count("se_nn_accuracy") == 3 and spy.count("se_embed_head_fwd") == 0


@pytest.mark.parametrize("kind", ["cosine", "sqdist"])
def test_metric_on_other_tensors_falls_back(kind, monkeypatch):
    import sehip
    import utils
    emb, outs, y = _setup(2)
    head, metrics = _objects(kind, True, emb, (5,))
    dot = kind == "cosine"
    parent = utils.nn_accuracy(emb, dot_prod_sim=dot, k=5)
    spy = _Spy(monkeypatch)
    # on its own, before any loss call
    other = sehip.l2norm(outs) if dot else outs
    got = metrics[1](y, other)
    assert spy.count("se_nn_accuracy") == 1
    assert torch.equal(got, parent(y, other))
    # after a loss call: the head's own tensors take the stored counts, another batch / a modified tensor / gathered rows do not
    head(y, outs)
    m_in = head.last_normalized if dot else outs.detach()
    spy.names.clear()
    fast = metrics[1](y, m_in)
    assert spy.names == []
    assert torch.equal(fast, parent(y, m_in))
    spy.names.clear()
    emb2, outs2, y2 = _setup(3)
    other2 = sehip.l2norm(outs2) if dot else outs2
    assert torch.equal(metrics[1](y2, other2), parent(y2, other2))
    assert torch.equal(metrics[1](y2, m_in), parent(y2, m_in))                   # other labels, same predictions
    assert torch.equal(metrics[1](emb[y], m_in), parent(emb[y], m_in))           # gathered embeddings as y_true
    assert spy.count("se_nn_accuracy") == 6 and spy.count("se_embed_head_fwd") == 0
    spy.names.clear()
    m_in.add_(1.0)                                                               # same storage, new version
    assert torch.equal(metrics[1](y, m_in), parent(y, m_in))
    assert spy.count("se_nn_accuracy") == 2


@pytest.mark.parametrize("loss,keys", [("inv_corr", ("max_sim_acc", "max_sim_acc5")), ("mse", ("nn_accuracy", "nn_accuracy5"))])
def test_learn_image_embeddings_end_to_end(loss, keys, tmp_path):
    import learn_image_embeddings as lie
    rng = np.random.default_rng(4)
    E = rng.standard_normal((10, 10)).astype(np.float32)
    E /= np.linalg.norm(E, axis=-1, keepdims=True)
    emb = str(tmp_path / "emb.pickle")
    with open(emb, "wb") as f:
        pickle.dump({"embedding": E, "ind2label": list(range(10)), "label2ind": {i: i for i in range(10)}}, f)
    final = lie.main(["--dataset", "synthetic:10x16x64x32", "--data_root", "-", "--embedding", emb, "--loss", loss, "--epochs", "1",
                      "--batch_size", "32", "--val_batch_size", "32", "--lr_schedule", "SGD", "--sgd_lr", "0.01", "--top_k_acc", "5",
                      "--no_progress"])
    assert final and all(np.isfinite(v) for v in final.values()), final
    for key in keys:
        assert key in final and 0.0 <= final[key] <= 1.0, final
    assert final[keys[1]] >= final[keys[0]]
