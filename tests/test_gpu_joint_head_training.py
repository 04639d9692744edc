"""The joint head in the training loop: engine.Trainer(joint_head=utils.JointEmbeddingHead(...)) logs the keys of today's objects from
one se_joint_head_fwd per step, with equal metric sums where no tie or clip is involved and losses / gradients within derived float32
bounds of today's torch composition; metrics on other tensors fall back; learn_image_embeddings.py trains under SE_JOINT_HEAD=1.

Bounds (u = 2^-24, S_i = sum_d |e_d p_d|, t_i = the sample's cross-entropy):
  embedding loss   kernel vs exact: 1.01 (ceil(D / 64) + 10) u (1 + S_i), the bound of tests/test_gpu_joint_head.py; torch's sum of D
                   products in any order vs exact: (D + 2) u (1 + S_i).  Tolerance: their sum.
  cross-entropy    either side evaluates C exponentials, a sum of C terms in some order, one logarithm and two additions:
                   (C + 16) u (1 + |t_i|) each, twice that between them.  (No probability leaves [1e-7, 1 - 1e-7] here: no clip.)
  a mean of B such values adds (B + 2) u |mean| on either side.
  dp               one float32 product per element on both paths: bit for bit (one-hot: the kernel's +0 where torch has -w * 0 = -0).
  dz               w (softmax - onehot): the softmax carries the relative error of the cross-entropy's exp / sum, (C + 16) u, on
                   values <= 1, on either side: 2 (C + 16) u |w|."""
import math
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, D, C = 64, 100, 100
U = 2.0 ** -24
CLS_WEIGHT = 0.1


def _setup(seed=0):
    gen = torch.Generator().manual_seed(seed)
    emb = torch.nn.functional.normalize(torch.randn((C, D), generator=gen), dim=1).cuda()
    p = torch.nn.functional.normalize(torch.randn((B, D), generator=gen), dim=1).cuda()
    z = (torch.randn((B, C), generator=gen) * 2).cuda()
    y = torch.randint(0, C, (B,), generator=gen).cuda()
    return emb, p, z, y


def _objects(joint, emb, ks, onehot=False):
    """(losses, metrics, joint head or None) of the two-output model, as learn_image_embeddings.py builds them"""
    import learn_image_embeddings as lie
    import utils
    if joint:
        head = utils.JointEmbeddingHead(None if onehot else emb, "argmax" if onehot else "nearest")
        losses = {"l2norm": (head.inv_correlation, 1.0), "prob": (head.categorical_crossentropy, CLS_WEIGHT)}
        metrics = {"l2norm": [head.accuracy()] + [head.accuracy(k) for k in ks], "prob": [head.cls_accuracy()] + [head.cls_accuracy(k) for k in ks]}
        return losses, metrics, head
    table = torch.eye(C, device="cuda") if onehot else emb
    losses = {"l2norm": (lambda yt, o: utils.inv_correlation(table[yt], o), 1.0), "prob": (lie.categorical_crossentropy, CLS_WEIGHT)}
    first = [lie.accuracy] + [utils.top_k_acc(k) for k in ks] if onehot else \
        [utils.nn_accuracy(emb, dot_prod_sim=True)] + [utils.nn_accuracy(emb, dot_prod_sim=True, k=k) for k in ks]
    return losses, {"l2norm": first, "prob": [lie.accuracy] + [utils.top_k_acc(k) for k in ks]}, None


def _step(joint, emb, p, z, y, ks, onehot=False):
    import engine
    losses, metrics, head = _objects(joint, emb, ks, onehot)
    kw = {"joint_head": head} if head is not None else {}
    tr = engine.Trainer(torch.nn.Linear(2, 2).cuda(), losses, metrics, autocast_dtype=None, **kw)
    pp, zz = p.clone().requires_grad_(True), z.clone().requires_grad_(True)
    logs = {}
    total = tr._loss_and_metrics((pp, zz), [y, y], logs)
    total.backward()
    tr.close()
    return {k: float(v) for k, v in logs.items()}, pp.grad, zz.grad, float(total.detach())


@pytest.mark.parametrize("onehot", [False, True], ids=["table", "onehot"])
def test_logs_and_gradients_against_todays_objects(onehot):
    emb, p, z, y = _setup()
    if onehot:
        p = torch.softmax(p * 5, dim=-1)
    logs_j, dp_j, dz_j, total_j = _step(True, emb, p, z, y, (5, 10), onehot)
    logs_t, dp_t, dz_t, total_t = _step(False, emb, p, z, y, (5, 10), onehot)
    first = ("acc", "acc5", "acc10") if onehot else ("max_sim_acc", "max_sim_acc5", "max_sim_acc10")
    keys = ["loss", "_n", "l2norm_loss", "prob_loss"] + ["l2norm_" + m for m in first] + ["prob_acc", "prob_acc5", "prob_acc10"]
    assert sorted(logs_j) == sorted(logs_t) == sorted(keys)
    for key in keys:
        if not key.endswith("loss"):
            assert logs_j[key] == logs_t[key], key                  # random continuous scores: no tie, no clip
    assert 0 < logs_j["prob_acc5"] <= logs_j["prob_acc10"] <= B and logs_j["l2norm_" + first[1]] <= logs_j["l2norm_" + first[2]] <= B

    E = (np.eye(C, dtype=np.float32) if onehot else emb.cpu().numpy())[y.cpu().numpy()]
    pn, zn = p.cpu().numpy().astype(np.float64), z.cpu().numpy().astype(np.float64)
    S = np.abs(E.astype(np.float64) * pn).sum(-1)
    tol_emb = ((1.01 * (math.ceil(D / 64) + 10) + (D + 2)) * U * (1 + S)).sum()
    exact_emb = (1.0 - (E.astype(np.float64) * pn).sum(-1)).sum()
    tol_emb += 2 * (B + 2) * U * abs(exact_emb)
    print("l2norm_loss", logs_j["l2norm_loss"], logs_t["l2norm_loss"], "tolerance", tol_emb)
    assert abs(logs_j["l2norm_loss"] - logs_t["l2norm_loss"]) <= tol_emb
    lse = np.log(np.exp(zn - zn.max(-1, keepdims=True)).sum(-1)) + zn.max(-1)
    t = lse - zn[np.arange(B), y.cpu().numpy()]
    assert t.max() < 16.0 and t.min() > 1e-6                       # no probability near the clip
    tol_cls = (2 * (C + 16) * U * (1 + np.abs(t))).sum() + 2 * (B + 2) * U * t.sum()
    print("prob_loss", logs_j["prob_loss"], logs_t["prob_loss"], "tolerance", tol_cls)
    assert abs(logs_j["prob_loss"] - logs_t["prob_loss"]) <= tol_cls
    tol_total = (tol_emb + CLS_WEIGHT * tol_cls) / B + 4 * U * abs(total_t)
    print("total", total_j, total_t, "tolerance", tol_total)
    assert abs(total_j - total_t) <= tol_total
    if onehot:          # torch's (-w) * 0 is -0 off the label's column, the kernel writes +0: equal values
        assert torch.equal(dp_j, dp_t)
    else:
        assert torch.equal(dp_j.view(torch.int32), dp_t.view(torch.int32))
    w = CLS_WEIGHT / B
    err = float((dz_j - dz_t).abs().max())
    print("dz", err, "tolerance", 2 * (C + 16) * U * w)
    assert err <= 2 * (C + 16) * U * w


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


def test_one_launch_serves_both_losses_and_every_metric(monkeypatch):
    emb, p, z, y = _setup(1)
    spy = _Spy(monkeypatch)
    _step(True, emb, p, z, y, (5, 10))
    assert spy.count("se_joint_head_fwd") == 1 and spy.count("se_joint_head_bwd") == 1
    assert spy.count("se_nn_accuracy") == 0 and spy.count("se_softmax_xent_fwd") == 0 and spy.count("se_embed_head_fwd") == 0
    spy.names.clear()
    _step(False, emb, p, z, y, (5, 10))
    assert spy.count("se_nn_accuracy") == 3 and spy.count("se_joint_head_fwd") == 0
    spy.names.clear()
    _step(True, emb, torch.softmax(p * 5, -1), z, y, (5, 10), onehot=True)
    assert spy.count("se_joint_head_fwd") == 1 and spy.count("se_joint_head_bwd") == 1 and spy.count("se_nn_accuracy") == 0


def test_embedding_role_alone_serves_a_single_output(monkeypatch):
    """`--cls_weight 0` with unnorm_corr / softmax_corr: outs has one entry; `post` is what the loss applies to it"""
    import engine
    import utils
    emb, p, _, y = _setup(2)
    raw = p * 3
    head = utils.JointEmbeddingHead(emb, "argmax", post=lambda o: torch.softmax(o, -1))
    tr = engine.Trainer(torch.nn.Linear(2, 2).cuda(), {"softmax": (head.inv_correlation, 1.0)}, {"softmax": [head.accuracy(), head.accuracy(5)]},
                        autocast_dtype=None, joint_head=head)
    spy = _Spy(monkeypatch)
    o = raw.clone().requires_grad_(True)
    logs = {}
    tr._loss_and_metrics((o,), y, logs).backward()
    tr.close()
    assert spy.count("se_joint_head_fwd") == 1 and spy.count("se_joint_head_bwd") == 1
    assert sorted(logs) == ["_n", "acc", "acc5", "loss"]
    o2 = raw.clone().requires_grad_(True)
    want = utils.inv_correlation(emb[y], torch.softmax(o2, -1))
    want.mean().backward()
    sm = torch.softmax(raw, -1).cpu().numpy().astype(np.float64)
    S = np.abs(emb.cpu().numpy()[y.cpu().numpy()].astype(np.float64) * sm).sum(-1)
    tol = ((1.01 * (math.ceil(D / 64) + 10) + (D + 2)) * U * (1 + S)).sum() + 2 * (B + 2) * U * abs(float(want.detach().sum()))
    assert abs(float(logs["loss"]) - float(want.detach().sum())) <= tol
    assert float(logs["acc"]) == float((raw.argmax(-1) == y).sum())
    # dp is bit-equal on both paths and the softmax backward is torch's on both: one product's rounding apart at the most
    assert float((o.grad - o2.grad).abs().max()) <= 4 * U * float(o2.grad.abs().max())


def test_metrics_on_other_tensors_fall_back(monkeypatch):
    import learn_image_embeddings as lie
    import utils
    emb, p, z, y = _setup(3)
    losses, metrics, head = _objects(True, emb, (5,))
    parent = utils.nn_accuracy(emb, dot_prod_sim=True, k=5)
    spy = _Spy(monkeypatch)
    # on their own, before any begin()
    assert torch.equal(metrics["l2norm"][1](y, p), parent(y, p)) and spy.count("se_nn_accuracy") == 2
    assert torch.equal(metrics["prob"][1](y, z), utils.top_k_acc(5)(y, z))
    assert torch.equal(head.categorical_crossentropy(y, z), lie.categorical_crossentropy(y, z))
    assert torch.equal(head.inv_correlation(y, p), utils.inv_correlation(emb[y], p))
    # after begin(): the batch's own tensors take the stored results, anything else does not
    assert head.begin([y, y], (p, z)) is True
    want = parent(y, p)
    spy.names.clear()
    fast = metrics["l2norm"][1](y, p.detach())
    assert spy.names == [] and torch.equal(fast, want)
    assert torch.equal(metrics["prob"][0](y, z.detach()), lie.accuracy(y, z)) and spy.names == []
    _, p2, z2, y2 = _setup(4)
    assert torch.equal(metrics["l2norm"][1](y2, p2), parent(y2, p2))
    assert torch.equal(metrics["l2norm"][1](y2, p), parent(y2, p))                         # other labels, same predictions
    assert torch.equal(metrics["l2norm"][1](emb[y], p), parent(emb[y], p))                 # gathered embeddings as y_true
    assert torch.equal(metrics["prob"][1](y2, z2), utils.top_k_acc(5)(y2, z2))
    assert torch.equal(head.inv_correlation(emb[y], p), utils.inv_correlation(emb[y], p))
    assert torch.equal(head.categorical_crossentropy(y2, z), lie.categorical_crossentropy(y2, z))
    assert spy.count("se_joint_head_fwd") == 0 and spy.count("se_nn_accuracy") == 6
    spy.names.clear()
    p.add_(1.0)                                                                            # same storage, new version
    assert torch.equal(metrics["l2norm"][1](y, p), parent(y, p)) and spy.count("se_nn_accuracy") == 2
    # CPU tensors and two different label arrays: begin() declines
    assert head.begin([y.cpu(), y.cpu()], (p.cpu(), z.cpu())) is False
    assert head.begin([y, y2], (p, z)) is False and head.begin([y, y.clone()], (p, z)) is False
    shared = utils.JointEmbeddingHead(emb, "nearest", shared_labels=True)             # the caller's promise: one copy per target is fine
    assert shared.begin([y, y.clone()], (p, z)) is True and shared.begin([y, y.clone().int()], (p, z)) is False
    assert torch.equal(head.categorical_crossentropy(y, z), lie.categorical_crossentropy(y, z))


@pytest.mark.parametrize("embedding", ["table", "onehot"])
def test_learn_image_embeddings_end_to_end(embedding, tmp_path, monkeypatch):
    import learn_image_embeddings as lie
    monkeypatch.setenv("SE_JOINT_HEAD", "1")
    spy = _Spy(monkeypatch)
    emb = "onehot"
    if embedding == "table":
        rng = np.random.default_rng(4)
        E = rng.standard_normal((10, 10)).astype(np.float32)
        E /= np.linalg.norm(E, axis=-1, keepdims=True)
        emb = str(tmp_path / "emb.pickle")
        with open(emb, "wb") as f:
            pickle.dump({"embedding": E, "ind2label": list(range(10)), "label2ind": {i: i for i in range(10)}}, f)
    final = lie.main(["--dataset", "synthetic:10x16x64x32", "--data_root", "-", "--embedding", emb, "--loss", "inv_corr", "--cls_weight", "0.1",
                      "--epochs", "1", "--batch_size", "32", "--val_batch_size", "32", "--lr_schedule", "SGD", "--sgd_lr", "0.01",
                      "--top_k_acc", "5", "--no_progress"])
    assert final and all(np.isfinite(v) for v in final.values()), final
    first = ("l2norm_max_sim_acc", "l2norm_max_sim_acc5") if embedding == "table" else ("l2norm_acc", "l2norm_acc5")
    for key in ("loss", "l2norm_loss", "prob_loss", "prob_acc", "prob_acc5") + first:
        assert key in final, (key, final)
    for a, b in (first, ("prob_acc", "prob_acc5")):
        assert 0.0 <= final[a] <= final[b] <= 1.0, final
    assert spy.count("se_joint_head_fwd") > 0 and spy.count("se_joint_head_fwd") >= spy.count("se_joint_head_bwd") > 0
    assert spy.count("se_nn_accuracy") == 0
