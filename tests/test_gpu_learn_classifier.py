"""GPU: the softmax classifier trained on the device -- one engine.Trainer step against autograd through the float64 oracle, the
learn_classifier.py CLI end to end (HIP-graph replay, label smoothing, top-k accuracy, log, dumps, feature dump through
pairwise_retrieval), --finetune / --finetune_init, --class_list, and a world-2 data-parallel run."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from test_classifier_host import Oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trainer_step_follows_the_gradient_of_the_fused_loss():
    """One eager step: the last layer moves by -lr x the clipped gradient, and that gradient is a positive multiple (<= 1: clipnorm)
    of features^T (dL/dlogits) with dL/dlogits from the float64 oracle on the step's own logits; the metrics of the step are the
    forward call's (one se_softmax_xent_fwd for loss, acc and acc5)."""
    import learn_classifier as lc
    import sehip
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(0)
    s, lr, B, C = 0.1, 0.05, 32, 100
    model = lc.build_classifier(C, "resnet-32", input_channels=3).cuda()
    losses, metrics = lc.build_losses(s, [5])
    tr = Trainer(model, losses, metrics, lr=lr, momentum=0.9, clipnorm=10.0, autocast_dtype=None, memory_format=torch.contiguous_format)
    gen = SyntheticGenerator(C, 32, 3, 64, 32)
    X, y = gen.train_sequence(B, shuffle=False, batch_transform=lc.transform_inputs, batch_transform_kwargs={"num_classes": C})[0]
    X = X.contiguous()                                    # the layout the trainer runs the network in
    W = model.prob.weight
    before = W.detach().clone()
    with torch.no_grad():
        feats = model.features(X).float()                 # train mode: the same batch statistics as the step's forward
        logits = model.prob(feats).float()
    o = Oracle(logits.cpu().numpy(), y.cpu().numpy(), s)
    dz = torch.from_numpy(o.dz / B).cuda()                # d mean loss / d logits
    dW = (dz.t() @ feats.double()).float()
    calls = []
    real = sehip.softmax_cross_entropy
    try:
        lc.sehip.softmax_cross_entropy = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        logs = {}
        tr.train_step(X, y, logs)
    finally:
        lc.sehip.softmax_cross_entropy = real
    torch.cuda.synchronize()
    assert len(calls) == 1                                # loss + acc + acc5: one forward call
    idx = next(i for i, p in enumerate(tr.flat.params) if p is W)
    off, n = tr.flat.offsets[idx]
    g = tr.flat.flat_g[off:off + n].view(C, -1)           # the clipped gradient the update used
    after = W.detach()
    assert torch.allclose(after, before - lr * g, rtol=0, atol=1e-7) and bool((after != before).any())
    factor = float((g * dW).sum() / (dW * dW).sum())
    assert 0.0 < factor <= 1.0 + 1e-5
    assert torch.allclose(g, factor * dW, rtol=2e-3, atol=1e-6)
    assert abs(float(logs["loss"]) / B - o.loss.mean()) < 1e-4
    assert float(logs["acc"]) == float((o.best == o.y).sum()) and float(logs["acc5"]) == float((o.above < 5).sum())
    assert float(logs["acc5"]) >= float(logs["acc"])
    # a metric asked about other logits computes itself (and says what these logits say)
    other = torch.randn(B, C, device="cuda")
    acc = metrics["prob"][0](y, other)
    assert torch.equal(acc, (other.argmax(-1) == y).float())


def _cli(lc, tmp_path, tag, *extra, arch="resnet-110-fc"):
    feat, wts, logd = str(tmp_path / (tag + "_feat.pickle")), str(tmp_path / (tag + "_w.pt")), str(tmp_path / (tag + "_log"))
    final = lc.main(["--dataset", "synthetic:100x32x192x64", "--data_root", "-", "--architecture", arch, "--lr_schedule", "SGD",
                     "--sgd_lr", "0.05", "--batch_size", "32", "--val_batch_size", "32", "--feature_dump", feat, "--weight_dump", wts,
                     "--log_dir", logd] + list(extra))
    return final, feat, wts, logd


def test_learn_classifier_cli_end_to_end(tmp_path, capsys):
    import learn_classifier as lc
    import evaluate_retrieval as er
    final, feat, wts, logd = _cli(lc, tmp_path, "e2e", "--epochs", "2", "--label_smoothing", "0.1", "--top_k_acc", "5")
    out = capsys.readouterr().out
    assert "Average Accuracy:" in out
    assert "[engine] training step: HIP-graph replay" in out and "staying eager" not in out
    keys = {"loss", "acc", "acc5"}
    assert keys == set(final) and all(np.isfinite(final[k]) for k in keys), final
    assert str([final["loss"], final["acc"], final["acc5"]]) in out               # the evaluate list, like the reference prints it
    log = [json.loads(l) for l in open(os.path.join(logd, "training_log.jsonl"))]
    assert [e["epoch"] for e in log] == [1, 2]
    for e in log:
        assert keys | {"val_" + k for k in keys} <= set(e) and all(np.isfinite(v) for v in e.values()), e
        assert e["acc5"] >= e["acc"] and e["val_acc5"] >= e["val_acc"] and 0.0 <= e["acc"] <= 1.0
        assert e["loss"] > 0.0
    model = lc.build_classifier(100, "resnet-110-fc", input_channels=3)
    model.load_state_dict(torch.load(wts))
    with open(feat, "rb") as f:
        dump = pickle.load(f)
    feats = np.stack([dump["feat"][i] for i in range(64)])
    assert feats.shape == (64, model.prob.in_features) and np.isfinite(feats).all()
    ranked = dict(er.pairwise_retrieval(feat, normalize=True, return_generator=False))
    assert sorted(ranked) == list(range(64)) and all(ranked[i][0] == i and len(ranked[i]) == 64 for i in ranked)


def test_finetune_init_trains_the_last_layer_only(tmp_path, capsys, monkeypatch):
    import learn_classifier as lc
    import train_cli
    _, _, wts, _ = _cli(lc, tmp_path, "base", "--epochs", "1", "--no_progress", arch="resnet-32")
    loaded = torch.load(wts)
    capsys.readouterr()
    seen = []

    class Recording(train_cli.Trainer):          # the state every Trainer of the run starts from
        def __init__(self, model, *a, **k):
            seen.append({n: p.detach().clone() for n, p in model.named_parameters()})
            super().__init__(model, *a, **k)
    monkeypatch.setattr(train_cli, "Trainer", Recording)
    _, _, wts2, _ = _cli(lc, tmp_path, "ft", "--epochs", "1", "--finetune", wts, "--finetune_init", "1", "--no_progress", arch="resnet-32")
    out = capsys.readouterr().out
    assert "Loading pre-trained weights" in out and "Average Accuracy:" in out
    assert out.index("Pre-training last layer") < out.index("Full model training")
    assert len(seen) == 2
    start, after_pre = seen
    for name, p in after_pre.items():
        same = torch.equal(p.view(torch.int32), loaded[name].to(p.device).view(torch.int32))
        assert torch.equal(start[name], loaded[name].to(p.device)), name
        assert same != name.startswith("prob."), name         # only the last layer moved
    final = torch.load(wts2)
    assert any(not torch.equal(final[n].cpu(), after_pre[n].cpu()) for n in after_pre if not n.startswith("prob."))


def test_class_list_subset(tmp_path, capsys):
    import learn_classifier as lc
    cl = tmp_path / "classes.txt"
    cl.write_text("".join("%d name%d\n" % (c, c) for c in (3, 1, 4, 15, 9, 2, 6, 3)) + "\n")
    final, _, wts, _ = _cli(lc, tmp_path, "sub", "--epochs", "1", "--no_progress", "--class_list", str(cl), arch="resnet-32")
    state = torch.load(wts)
    assert state["prob.weight"].shape[0] == 7 and state["prob.bias"].shape == (7,)
    assert np.isfinite(final["loss"]) and "Average Accuracy:" in capsys.readouterr().out


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # RCCL refuses two ranks on one device; gloo all-reduces CUDA tensors
    torch.cuda.set_device(0)
    import learn_classifier as lc
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(0)
    model = lc.build_classifier(100, "resnet-32", input_channels=3).cuda()
    losses, metrics = lc.build_losses(0.1, [5])
    tr = Trainer(model, losses, metrics, lr=0.05, clipnorm=10.0, autocast_dtype=None, memory_format=torch.contiguous_format)
    assert tr.world == 2 and tr.reducer.enabled
    gen = SyntheticGenerator(100, 32, 3, 256, 32)
    seq = gen.train_sequence(32, shuffle=False, rank=rank, world_size=world, batch_transform=lc.transform_inputs,
                             batch_transform_kwargs={"num_classes": 100})
    before = tr.flat.flat_p.detach().cpu().clone()
    ok = tr.enable_graphs(*seq[0])
    logs = {}
    for i in range(4):
        tr.train_step(*seq[i % len(seq)], logs)
    torch.cuda.synchronize()
    weights = tr.flat.flat_p.detach().cpu()
    both = [None, None]
    dist.all_gather_object(both, weights.numpy().tobytes())
    if rank == 0:
        torch.save({"ok": ok, "same": both[0] == both[1], "moved": bool((weights != before).any()),
                    "finite": bool(torch.isfinite(weights).all()), "n": float(logs["_n"]), "acc5": float(logs["acc5"]),
                    "acc": float(logs["acc"])}, out)
    dist.destroy_process_group()


def test_world2_weights_stay_identical(tmp_path):
    """Two processes (gloo) on the one GPU, 4 graph-mode steps on their halves of the global batch: identical weights on both ranks."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "w.pt")
    mp.spawn(_dp_worker, args=(2, 29653, out), nprocs=2, join=True)
    got = torch.load(out)
    assert got["ok"] and got["same"] and got["moved"] and got["finite"], got
    assert got["n"] == 64.0 and got["acc5"] >= got["acc"]
