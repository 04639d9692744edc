"""Host side of the embedding heads (no GPU): the binding declares the new entry points from the header, the heads are the loss classes
with the reference's metric names, the metrics take the stored counts on the head's own tensors and fall back on any others, and the
command line of learn_image_embeddings.py is what it was."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_declares_the_entry_points_of_the_header():
    from sehip import _lib
    src = open(os.path.join(ROOT, "include", "sehip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    for name in ("se_embed_head_fwd", "se_embed_head_workspace_bytes"):
        decl = re.search(r"\b%s\s*\(([^()]*)\)" % name, src).group(1)
        nargs = len(decl.split(","))
        proto = _lib.PROTOTYPES[name]
        assert len(proto.params) + proto.stream == nargs, name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    fwd = _lib.PROTOTYPES["se_embed_head_fwd"]
    assert fwd.stream and fwd.restype == "int" and len(fwd.params) == 23
    assert [p.name for p in fwd.params][:4] == ["mode", "x", "x_dtype", "ldx"]
    assert {p.name: p.pointee for p in fwd.params if p.name in ("n_better", "n_within", "best", "labels", "scores", "workspace")} == \
        {"n_better": "int32_t", "n_within": "int32_t", "best": "int32_t", "labels": "int64_t", "scores": "float", "workspace": "void"}
    ws = _lib.PROTOTYPES["se_embed_head_workspace_bytes"]
    assert ws.restype == "int64_t" and not ws.stream and len(ws.params) == 4


def test_workspace_and_argument_checks_run_on_the_host():
    """(the rules of se_embed_head_fwd that need no device: they run before any launch)"""
    import ctypes
    import sehip
    lib = sehip.lib()
    assert lib.se_embed_head_workspace_bytes(0, 128, 100, 100) == 0             # four class tiles: one workgroup walks them
    need = lib.se_embed_head_workspace_bytes(0, 128, 1000, 1000)
    assert need >= 128 * 16 and need % 8 == 0
    assert lib.se_embed_head_workspace_bytes(1, 128, 1000, 1000) == need
    assert lib.se_embed_head_workspace_bytes(0, 0, 10, 1000) == 0
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(64)
    invalid = sehip._lib.DEFINES["SE_ERR_INVALID"]
    assert lib.se_embed_head_fwd(0, z, 0, 8, z, z, 8, 0, 8, 4, z, 8, z, z, z, z, z, z, z, z, 4, z, 0, z) == 0          # empty batch
    assert lib.se_embed_head_fwd(3, one, 0, 8, one, one, 8, 2, 8, 4, z, 8, z, one, z, z, one, one, z, z, 4, z, 0, z) == invalid
    assert b"mode" in lib.se_last_error()
    assert lib.se_embed_head_fwd(0, one, 0, 8, one, one, 8, 2, 8, 4, z, 8, z, one, z, z, z, one, z, z, 4, z, 0, z) == invalid
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_embed_head_fwd(0, one, 0, 8, one, one, 8, 64, 8, 1000, z, 8, z, one, z, z, one, one, z, z, 1000, z, 0, z) == invalid
    assert b"workspace" in lib.se_last_error()


def test_heads_are_the_loss_classes_with_the_reference_metric_names():
    import utils
    emb = torch.eye(4)
    cos, sq = utils.CosineEmbeddingHead(emb), utils.SquaredDistanceHead(emb)
    assert isinstance(cos, utils.CosineEmbeddingLoss) and isinstance(sq, utils.SquaredDistanceLoss)
    assert cos.name == utils.CosineEmbeddingLoss.name == "inv_correlation"
    assert sq.name == utils.SquaredDistanceLoss.name == "squared_distance"
    assert cos.embedding is emb and sq.embedding is emb
    assert cos.accuracy().name == "max_sim_acc" and cos.accuracy(5).name == "max_sim_acc5"
    assert sq.accuracy().name == "nn_accuracy" and sq.accuracy(k=5).name == "nn_accuracy5"
    for k in (1, 5):
        assert cos.accuracy(k).name == utils.nn_accuracy(emb, dot_prod_sim=True, k=k).name
        assert sq.accuracy(k).name == utils.nn_accuracy(emb, dot_prod_sim=False, k=k).name
    with pytest.raises(ValueError):
        cos(torch.zeros(3, 4), torch.zeros(3, 4))            # gathered rows as y_true: the parent's error
    # gathered rows / host tensors: the squared-distance head is its parent
    yt, yp = torch.randn(3, 4), torch.randn(3, 4)
    assert torch.equal(sq(yt, yp), utils.squared_distance(yt, yp))
    y = torch.tensor([0, 2, 1])
    assert torch.equal(sq(y, yp), utils.squared_distance(emb[y], yp))
    assert sq.counts_for(y, yp) is None


class _StandIn(object):
    """sehip.embedding_head / sehip.nn_accuracy in float64 NumPy on host tensors (cosine scores), counting their calls"""

    def __init__(self):
        self.head_calls, self.metric_calls = 0, 0

    @staticmethod
    def _counts(xhat, labels, emb):
        s = xhat.double() @ emb.double().T
        true = s[torch.arange(len(labels)), labels][:, None]
        within = ((s - true).abs() < 1e-6).sum(dim=1).int()
        better = ((s - true) >= 1e-6).sum(dim=1).int()
        return better, within

    def embedding_head(self, x, labels, embedding, mode="cosine", want_normalized=True, want_scores=False, want_best=False):
        from sehip.ops import EmbeddingHead
        assert mode == "cosine"
        self.head_calls += 1
        xhat = torch.nn.functional.normalize(x.float(), dim=1)
        better, within = self._counts(xhat, labels, embedding)
        loss_i = 1.0 - (xhat * embedding[labels]).sum(dim=1)
        return EmbeddingHead(loss_i, xhat, better, within, None, None)

    def nn_accuracy(self, y_pred, labels, embedding, dot_prod_sim=False, k=1, want_scores=False, want_best=False):
        assert dot_prod_sim and not want_scores and not want_best
        self.metric_calls += 1
        better, within = self._counts(y_pred, labels, embedding)
        return ((within >= 1) & (better < k)).float()


def test_metric_reads_the_heads_counts_on_its_own_tensors_only(monkeypatch):
    import sehip
    import utils
    stand = _StandIn()
    monkeypatch.setattr(sehip, "embedding_head", stand.embedding_head)
    monkeypatch.setattr(sehip, "nn_accuracy", stand.nn_accuracy)
    gen = torch.Generator().manual_seed(0)
    emb = torch.nn.functional.normalize(torch.randn((12, 6), generator=gen), dim=1)
    x, y = torch.randn((40, 6), generator=gen), torch.randint(0, 12, (40,), generator=gen)
    head = utils.CosineEmbeddingHead(emb)
    m1, m5 = head.accuracy(), head.accuracy(5)
    want1 = stand.nn_accuracy(torch.nn.functional.normalize(x, dim=1), y, emb, True, 1)
    want5 = stand.nn_accuracy(torch.nn.functional.normalize(x, dim=1), y, emb, True, 5)
    assert 0 < want1.sum() < want5.sum() < 40                    # the two metrics differ on these inputs
    stand.metric_calls = 0

    # before any loss call: fallback
    xhat0 = torch.nn.functional.normalize(x, dim=1)
    assert torch.equal(m1(y, xhat0), want1) and stand.metric_calls == 1

    loss_i = head(y, x)
    assert stand.head_calls == 1 and loss_i.shape == (40,) and head.last_normalized.shape == (40, 6)
    stand.metric_calls = 0
    got1, got5 = m1(y, head.last_normalized), m5(y, head.last_normalized)
    assert stand.metric_calls == 0 and stand.head_calls == 1     # no launch: the stored counts
    assert got1.dtype == torch.float32 and torch.equal(got1, want1) and torch.equal(got5, want5)
    assert torch.equal(m5(y, head.last_normalized.detach()), want5) and stand.metric_calls == 0     # a detached alias is the same tensor

    # anything else falls back, and is right
    assert torch.equal(m5(y, head.last_normalized.clone()), want5) and stand.metric_calls == 1     # other storage
    assert torch.equal(m5(y.clone(), head.last_normalized), want5) and stand.metric_calls == 2     # other labels storage
    stand.metric_calls = 0
    half = m5(y[:20], head.last_normalized[:20])                                                   # same storage, other shape
    assert stand.metric_calls == 1 and torch.equal(half, want5[:20])
    gathered = m5(emb[y], head.last_normalized)                                                    # the reference's y_true
    assert stand.metric_calls == 2 and torch.equal(gathered, want5)
    y2 = torch.randint(0, 12, (40,), generator=gen)
    stand.metric_calls = 0
    other = m1(y2, head.last_normalized)
    assert stand.metric_calls == 1 and torch.equal(other, stand.nn_accuracy(head.last_normalized, y2, emb, True, 1))
    stand.metric_calls = 0
    y.add_(0)                                                                                      # the labels changed in place since
    assert torch.equal(m1(y, head.last_normalized), want1) and stand.metric_calls == 1
    head(y, x)                                                                                     # a new loss call: its tensors count
    stand.metric_calls = 0
    assert torch.equal(m1(y, head.last_normalized), want1) and stand.metric_calls == 0


def test_command_line_is_unchanged():
    import learn_image_embeddings as lie
    parser = lie.build_parser()
    options = sorted(o for a in parser._actions for o in a.option_strings)
    assert options == ['--architecture', '--batch_size', '--clipgrad', '--clr_max_lr', '--clr_min_lr', '--clr_step_len', '--cls_base', '--cls_weight',
                       '--data_root', '--dataset', '--embedding', '--epochs', '--feature_dump', '--finetune', '--finetune_init', '--gpu_merge',
                       '--gpus', '--help', '--initial_epoch', '--log_dir', '--loss', '--lr_schedule', '--max_decay', '--model_dump', '--nesterov',
                       '--no_progress', '--queue_size', '--read_workers', '--sgd_lr', '--sgd_min_lr', '--sgd_patience', '--sgd_schedule',
                       '--sgdr_base_len', '--sgdr_max_lr', '--sgdr_mul', '--snapshot', '--snapshot_best', '--top_k_acc', '--val_batch_size',
                       '--weight_dump', '-h']
    assert parser.get_default("loss") == "inv_corr" and parser.get_default("top_k_acc") == [] and parser.get_default("cls_weight") == 0.0
    loss = [a for a in parser._actions if a.dest == "loss"][0]
    assert list(loss.choices) == ['mse', 'inv_corr', 'unnorm_corr', 'softmax_corr']
    assert lie.head_by_default('inv_corr', True, 0) is False         # one-hot targets keep their arg-max metrics
