"""GPU: the label-embedding baseline trained on the device -- one engine.Trainer step against the float64 oracle on the step's own
logits, the learn_labelembedding.py CLI end to end (HIP-graph replay, log under the Keras names, dumps, the raw feature dump through
pairwise_retrieval), --finetune / --finetune_init, and a world-2 data-parallel run."""
import json
import os
import pickle
import sys
import time

import numpy as np
import pytest
import torch

from oracle import loss_oracle as lo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"loss", "labelembed_loss_loss", "prob_loss", "prob_acc"}


def _model(C=10):
    import learn_labelembedding as ll
    import utils
    return ll.labelembed_model(utils.build_network(100, "resnet-32", input_channels=3), C)


def test_trainer_step_moves_the_table_along_the_oracle_gradient():
    """One eager engine.Trainer step, resnet-32, B = 32, C = 10: the table moves by -lr x the clipped gradient, which is a positive
    multiple (<= 1: clipnorm) of the float64-oracle table gradient (np.add.at of its d_tar over the labels) on the step's own logits;
    the logged loss is the oracle's, the ``prob`` output's loss is zero."""
    import learn_labelembedding as ll
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(0)
    lr, B, C = 0.05, 32, 10
    model = _model(C).cuda()
    losses, metrics = ll.build_losses(model)
    tr = Trainer(model, losses, metrics, lr=lr, momentum=0.9, clipnorm=10.0, autocast_dtype=None, memory_format=torch.contiguous_format)
    gen = SyntheticGenerator(C, 32, 3, 64, 32)
    seq = gen.train_sequence(B, shuffle=False, batch_transform=ll.transform_trainer_inputs, batch_transform_kwargs={"num_classes": C})
    X, ys = seq[0]
    X = X.contiguous()                                    # the layout the trainer runs the network in
    W = model.labelembeddings.weight
    before = W.detach().clone()
    assert torch.equal(before, torch.eye(C, device="cuda"))
    with torch.no_grad():
        logits2, out1, _ = model(X)                       # train mode: the same batch statistics as the step's forward
    y = ys[0].cpu().numpy()
    o1, o2 = logits2[:, :C].float().cpu().numpy(), logits2[:, C:].float().cpu().numpy()
    tar = before.cpu().numpy()[y]
    want = lo.labelembed_loss(o1, o2, tar, y)
    _, _, dt = lo.labelembed_loss_bwd(o1, o2, tar, y, np.full(B, 1.0 / B))
    dT = np.zeros((C, C))
    np.add.at(dT, y, dt)
    assert (o2.argmax(1) == y).any() and np.abs(dT).max() > 0, "no row with mask = 1: the table has no gradient to follow"
    dT = torch.from_numpy(dT).float().cuda()
    logs = {}
    tr.train_step(X, ys, logs)
    torch.cuda.synchronize()
    idx = next(i for i, p in enumerate(tr.flat.params) if p is W)
    off, n = tr.flat.offsets[idx]
    g = tr.flat.flat_g[off:off + n].view(C, C)            # the clipped gradient the update used
    after = W.detach()
    assert torch.allclose(after, before - lr * g, rtol=0, atol=1e-7) and bool((after != before).any())
    factor = float((g * dT).sum() / (dT * dT).sum())
    assert 0.0 < factor <= 1.0 + 1e-5
    assert torch.allclose(g, factor * dT, rtol=2e-3, atol=1e-6)
    absent = np.setdiff1d(np.arange(C), y)
    assert torch.equal(after[absent], before[absent])
    assert abs(float(logs["labelembed_loss_loss"]) / B - want.mean()) < 1e-4
    assert float(logs["prob_loss"]) == 0.0 and abs(float(logs["loss"]) / B - want.mean()) < 1e-4
    assert float(logs["prob_acc"]) == float((o1.argmax(1) == y).sum()) and float(logs["_n"]) == B


def _cli(ll, tmp_path, tag, *extra):
    feat, wts, logd = str(tmp_path / (tag + "_feat.pickle")), str(tmp_path / (tag + "_w.pt")), str(tmp_path / (tag + "_log"))
    final = ll.main(["--dataset", "synthetic:10x32x96x32", "--data_root", "-", "--architecture", "resnet-32", "--lr_schedule", "SGD",
                     "--sgd_lr", "0.05", "--batch_size", "32", "--val_batch_size", "32", "--feature_dump", feat, "--weight_dump", wts,
                     "--log_dir", logd] + list(extra))
    return final, feat, wts, logd


def test_learn_labelembedding_cli_end_to_end(tmp_path, capsys):
    import learn_labelembedding as ll
    import evaluate_retrieval as er
    final, feat, wts, logd = _cli(ll, tmp_path, "e2e", "--epochs", "2")
    out = capsys.readouterr().out
    assert "Accuracy:" in out.replace("Average Accuracy:", "") and "Average Accuracy:" in out
    assert "[engine] training step: HIP-graph replay" in out and "staying eager" not in out
    assert KEYS <= set(final) and all(np.isfinite(final[k]) for k in KEYS), final
    assert str([final[k] for k in sorted(final)]) in out                               # the evaluate list
    log = [json.loads(l) for l in open(os.path.join(logd, "training_log.jsonl"))]
    assert [e["epoch"] for e in log] == [1, 2]
    for e in log:
        assert KEYS | {"val_" + k for k in KEYS} <= set(e) and all(np.isfinite(v) for v in e.values()), e
        assert e["prob_loss"] == 0.0 and e["val_prob_loss"] == 0.0 and 0.0 <= e["prob_acc"] <= 1.0
        assert e["loss"] >= e["labelembed_loss_loss"] > 0.0                            # plus the L2 penalties of the backbone
    model = _model()
    model.load_state_dict(torch.load(wts))
    table = model.labelembeddings.weight.detach()
    assert torch.isfinite(table).all() and not torch.equal(table, torch.eye(10))
    with open(feat, "rb") as f:
        dump = pickle.load(f)
    feats = np.stack([dump["feat"][i] for i in range(32)])
    assert sorted(dump["feat"]) == list(range(32))
    assert feats.shape == (32, model.embedding_bn.num_features) and np.isfinite(feats).all()
    assert not np.allclose(np.linalg.norm(feats, axis=-1), 1.0, atol=1e-3)                       # the pooled features, raw
    ranked = dict(er.pairwise_retrieval(feat, normalize=True, return_generator=False))
    assert sorted(ranked) == list(range(32)) and all(ranked[i][0] == i and len(ranked[i]) == 32 for i in ranked)


def test_finetune_init_trains_the_new_layers_only(tmp_path, capsys, monkeypatch):
    import learn_labelembedding as ll
    import train_cli
    _, _, wts, _ = _cli(ll, tmp_path, "base", "--epochs", "1", "--no_progress")
    loaded = torch.load(wts)
    capsys.readouterr()
    seen = []

    class Recording(train_cli.Trainer):          # the state every Trainer of the run starts from
        def __init__(self, model, *a, **k):
            seen.append({n: p.detach().clone() for n, p in model.named_parameters()})
            super().__init__(model, *a, **k)
    monkeypatch.setattr(train_cli, "Trainer", Recording)
    _, _, wts2, _ = _cli(ll, tmp_path, "ft", "--epochs", "1", "--finetune", wts, "--finetune_init", "1", "--no_progress")
    out = capsys.readouterr().out
    assert "Loading pre-trained weights" in out and "Average Accuracy:" in out
    assert out.index("Pre-training new layers") < out.index("Full model training")
    assert len(seen) == 2
    start, after_pre = seen
    new = ("embedding_bn.", "prob.", "out2.", "labelembeddings.", "base_model.embedding.")
    assert {n.split(".")[0] for n in after_pre if n.startswith(new)} == {"embedding_bn", "prob", "out2", "labelembeddings"}
    for name, p in after_pre.items():
        same = torch.equal(p.view(torch.int32), loaded[name].to(p.device).view(torch.int32))
        assert torch.equal(start[name], loaded[name].to(p.device)), name
        assert same != name.startswith(new), name         # the named layers moved, nothing else did
    final = torch.load(wts2)
    assert any(not torch.equal(final[n].cpu(), after_pre[n].cpu()) for n in after_pre if not n.startswith(new))


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # RCCL refuses two ranks on one device; gloo all-reduces CUDA tensors
    torch.cuda.set_device(0)
    import learn_labelembedding as ll
    import utils
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(0)
    model = ll.labelembed_model(utils.build_network(100, "resnet-32", input_channels=3), 10).cuda()
    losses, metrics = ll.build_losses(model)
    tr = Trainer(model, losses, metrics, lr=0.05, clipnorm=10.0, autocast_dtype=None, memory_format=torch.contiguous_format)
    assert tr.world == 2 and tr.reducer.enabled
    gen = SyntheticGenerator(10, 32, 3, 128, 32)
    seq = gen.train_sequence(32, shuffle=False, rank=rank, world_size=world, batch_transform=ll.transform_trainer_inputs,
                             batch_transform_kwargs={"num_classes": 10})
    before = tr.flat.flat_p.detach().cpu().clone()
    table_before = model.labelembeddings.weight.detach().cpu().clone()
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
                    "table_moved": bool((model.labelembeddings.weight.detach().cpu() != table_before).any()),
                    "finite": bool(torch.isfinite(weights).all()), "n": float(logs["_n"])}, out)
    dist.destroy_process_group()


def test_world2_weights_stay_identical(tmp_path):
    """Two fresh processes (gloo) on the one GPU, 4 graph-mode steps on their halves of the global batch (each half with its own
    batch-wide mask factor, like a tower of the reference): identical weights on both ranks, the table included."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "w.pt")
    ctx = mp.spawn(_dp_worker, args=(2, 29667, out), nprocs=2, join=False)
    deadline = time.monotonic() + 240
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the data-parallel workers did not finish in time")
    got = torch.load(out)
    assert got["ok"] and got["same"] and got["moved"] and got["table_moved"] and got["finite"], got
    assert got["n"] == 64.0
