"""Host side of the joint head (no GPU): the header declares se_joint_head_*, learn_image_embeddings.joint_head_by_default follows its
table, utils.JointEmbeddingHead on CPU tensors is today's composition, and a Trainer without ``joint_head`` logs as before."""
import numpy as np
import pytest
import torch

B, D, C = 16, 12, 12


def test_header_declares_the_joint_head():
    from sehip._lib import DEFINES, PROTOTYPES
    assert DEFINES["SE_HEAD_METRIC_NEAREST"] == 0 and DEFINES["SE_HEAD_METRIC_ARGMAX"] == 1
    ws, fwd, bwd = (PROTOTYPES[n] for n in ("se_joint_head_workspace_bytes", "se_joint_head_fwd", "se_joint_head_bwd"))
    assert [p.name for p in ws.params] == ["metric", "B", "D", "C"]
    assert [p.name for p in fwd.params] == [
        "p", "ldp", "labels", "emb", "lde", "B", "D", "C", "metric", "emb_loss_i", "n_better", "n_within", "p_best", "p_above", "scores",
        "lds", "logits", "z_dtype", "ldz", "cls_loss_i", "aux", "z_best", "z_above", "workspace", "workspace_bytes"]
    assert [p.name for p in bwd.params] == [
        "labels", "emb", "lde", "B", "D", "C", "grad_emb_loss_i", "grad_emb_scale", "dp", "lddp", "logits", "z_dtype", "ldz", "aux",
        "grad_cls_loss_i", "grad_cls_scale", "dz", "dz_dtype", "lddz"]
    assert fwd.stream and bwd.stream and not ws.stream and fwd.restype == bwd.restype == "int"


@pytest.mark.parametrize("loss,cls_weight,want", [
    ("inv_corr", 0.1, True), ("unnorm_corr", 0.1, True), ("softmax_corr", 0.1, True),
    ("unnorm_corr", 0.0, True), ("softmax_corr", 0.0, True),
    ("inv_corr", 0.0, False), ("mse", 0.1, False), ("mse", 0.0, False),
])
def test_joint_head_by_default_follows_the_table(loss, cls_weight, want, monkeypatch):
    import learn_image_embeddings as lie
    for onehot in (False, True):
        monkeypatch.delenv("SE_JOINT_HEAD", raising=False)
        assert lie.joint_head_by_default(loss, onehot, cls_weight) is False          # opt-in: nothing changes without the switch
        monkeypatch.setenv("SE_JOINT_HEAD", "0")
        assert lie.joint_head_by_default(loss, onehot, cls_weight) is False
        monkeypatch.setenv("SE_JOINT_HEAD", "1")
        assert lie.joint_head_by_default(loss, onehot, cls_weight) is want


def _cpu_batch(seed=0):
    gen = torch.Generator().manual_seed(seed)
    emb = torch.nn.functional.normalize(torch.randn((C, D), generator=gen), dim=1)
    p = torch.nn.functional.normalize(torch.randn((B, D), generator=gen), dim=1)
    z = torch.randn((B, C), generator=gen) * 3
    y = torch.randint(0, C, (B,), generator=gen)
    return emb, p, z, y


@pytest.mark.parametrize("table", [True, False])
def test_joint_embedding_head_on_cpu_is_the_composition(table):
    import learn_image_embeddings as lie
    import utils
    emb, p, z, y = _cpu_batch()
    head = utils.JointEmbeddingHead(emb if table else None, "nearest" if table else "argmax")
    assert head.begin([y, y], (p, z)) is False                       # CPU tensors: no launch, everything falls back
    E = emb if table else torch.eye(C)
    assert torch.equal(head.inv_correlation(y, p), utils.inv_correlation(E[y], p))
    assert torch.equal(head.inv_correlation(E[y], p), utils.inv_correlation(E[y], p))       # gathered embeddings as y_true
    assert torch.equal(head.categorical_crossentropy(y, z), lie.categorical_crossentropy(y, z))
    assert torch.equal(head.cls_accuracy()(y, z), lie.accuracy(y, z))
    assert torch.equal(head.cls_accuracy(5)(y, z), utils.top_k_acc(5)(y, z))
    assert [m.name for m in (head.cls_accuracy(), head.cls_accuracy(5))] == ["acc", "acc5"]
    if table:
        assert [m.name for m in (head.accuracy(), head.accuracy(5))] == ["max_sim_acc", "max_sim_acc5"]
    else:
        assert [m.name for m in (head.accuracy(), head.accuracy(5))] == ["acc", "acc5"]
        assert torch.equal(head.accuracy()(y, p), lie.accuracy(y, p))
        assert torch.equal(head.accuracy(5)(y, p), utils.top_k_acc(5)(y, p))


def test_joint_embedding_head_rejects_a_table_free_nearest_metric():
    import utils
    with pytest.raises(ValueError):
        utils.JointEmbeddingHead(None, "nearest")
    with pytest.raises(ValueError):
        utils.JointEmbeddingHead(None, "best")


def test_trainer_without_joint_head_logs_as_before():
    import engine
    import learn_image_embeddings as lie
    import utils
    emb, p, z, y = _cpu_batch(1)
    losses = {"l2norm": (lambda yt, o: utils.inv_correlation(emb[yt], o), 1.0), "prob": (lie.categorical_crossentropy, 0.1)}
    metrics = {"prob": [lie.accuracy, utils.top_k_acc(5)]}

    class _Begun(object):
        calls = 0

        def begin(self, ys, outs):
            self.calls += 1
            return False

    def step(**kw):
        tr = engine.Trainer(torch.nn.Linear(2, 2), losses, metrics, autocast_dtype=None, **kw)
        logs = {}
        total = tr._loss_and_metrics((p, z), [y, y], logs)
        return tr, {k: np.float64(v) for k, v in logs.items()}, float(total)

    plain, logs_a, total_a = step()
    assert plain.joint_head is None
    hook = _Begun()
    hooked, logs_b, total_b = step(joint_head=hook)
    assert hooked.joint_head is hook and hook.calls == 1             # once per step, before the losses run
    assert sorted(logs_a) == sorted(["l2norm_loss", "prob_loss", "prob_acc", "prob_acc5", "loss", "_n"])
    assert logs_a == logs_b and total_a == total_b
    want = float((utils.inv_correlation(emb[y], p).mean() + lie.categorical_crossentropy(y, z).mean() * 0.1))
    assert total_a == want
