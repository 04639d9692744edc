"""GPU: the learn_devise.py CLI end to end (HIP-graph replay of the Adagrad step, log, dumps, feature dump through
pairwise_retrieval), --init_weights with --init_epochs / --ft_epochs on a classifier's weights, a class subset, and a world-2
data-parallel run of Trainer(optimizer='adagrad')."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _embedding_pickle(tmp_path, labels, dim, name="emb.pickle"):
    rng = np.random.default_rng(len(labels) * 1000 + dim)
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        pickle.dump({"ind2label": list(labels), "label2ind": {l: i for i, l in enumerate(labels)},
                     "embedding": rng.standard_normal((len(labels), dim)) * 2.0}, f)          # unnormalised
    return path


def _cli(ld, tmp_path, tag, emb, *extra, arch="resnet-110-fc"):
    feat, wts, logd = str(tmp_path / (tag + "_feat.pickle")), str(tmp_path / (tag + "_w.pt")), str(tmp_path / (tag + "_log"))
    final = ld.main(["--dataset", "synthetic:100x32x192x64", "--data_root", "-", "--embedding", emb, "--architecture", arch,
                     "--batch_size", "32", "--val_batch_size", "32", "--feature_dump", feat, "--weight_dump", wts, "--log_dir", logd]
                    + list(extra))
    return final, feat, wts, logd


def test_learn_devise_cli_end_to_end(tmp_path, capsys):
    import evaluate_retrieval as er
    import learn_devise as ld
    import utils
    emb = _embedding_pickle(tmp_path, range(100), 24)
    final, feat, wts, logd = _cli(ld, tmp_path, "e2e", emb, "--ft_epochs", "2", "--margin", "0.1", "--max_decay", "0.1")
    out = capsys.readouterr().out
    assert "Fine-tuning all layers" in out and "Pre-training linear transformation" not in out
    assert "[engine] training step: HIP-graph replay" in out and "staying eager" not in out
    keys = {"loss", "max_sim_acc"}
    assert keys == set(final) and all(np.isfinite(final[k]) for k in keys), final
    assert str([final["loss"], final["max_sim_acc"]]) in out                        # the evaluate list, like the reference prints it
    log = [json.loads(l) for l in open(os.path.join(logd, "training_log.jsonl"))]
    assert [e["epoch"] for e in log] == [1, 2]
    for e in log:
        assert keys | {"val_" + k for k in keys} <= set(e) and all(np.isfinite(v) for v in e.values()), e
        assert 0.0 <= e["max_sim_acc"] <= 1.0 and 0.0 <= e["val_max_sim_acc"] <= 1.0
    model = utils.build_network(24, "resnet-110-fc", input_channels=3)
    model.load_state_dict(torch.load(wts))
    with open(feat, "rb") as f:
        dump = pickle.load(f)
    feats = np.stack([dump["feat"][i] for i in range(64)])
    assert sorted(dump["feat"]) == list(range(64)) and feats.shape == (64, 24) and np.isfinite(feats).all()
    ranked = dict(er.pairwise_retrieval(feat, normalize=True, return_generator=False))
    assert sorted(ranked) == list(range(64)) and all(ranked[i][0] == i and len(ranked[i]) == 64 for i in ranked)


def test_init_weights_trains_the_linear_transformation_first(tmp_path, capsys, monkeypatch):
    import learn_classifier as lc
    import learn_devise as ld
    import train_cli
    base = str(tmp_path / "classifier.pt")
    lc.main(["--dataset", "synthetic:100x32x192x64", "--data_root", "-", "--architecture", "resnet-32", "--lr_schedule", "SGD",
             "--sgd_lr", "0.05", "--batch_size", "32", "--val_batch_size", "32", "--epochs", "1", "--no_progress", "--weight_dump", base])
    loaded = torch.load(base)
    assert "prob.weight" in loaded
    capsys.readouterr()
    seen = []

    class Recording(train_cli.Trainer):          # the state every Trainer of the run starts from, and the trainer itself
        def __init__(self, model, *a, **k):
            seen.append(({n: p.detach().clone() for n, p in model.named_parameters()}, self, k))
            super().__init__(model, *a, **k)
            self.accumulator_at_start = self.flat.flat_v.clone()
    monkeypatch.setattr(train_cli, "Trainer", Recording)
    emb = _embedding_pickle(tmp_path, range(100), 64)      # resnet-32 emits its 64 pooled features
    _, _, wts, _ = _cli(ld, tmp_path, "ws", emb, "--init_weights", base, "--init_epochs", "1", "--ft_epochs", "1", "--no_progress",
                        arch="resnet-32")
    out = capsys.readouterr().out
    assert "Loading pre-trained weights" in out
    assert out.index("Pre-training linear transformation") < out.index("Fine-tuning all layers")
    assert len(seen) == 2                                                            # two trainers: Keras compiles twice
    (start, pre, pre_kw), (after_pre, ft, ft_kw) = seen
    assert pre_kw["optimizer"] == ft_kw["optimizer"] == "adagrad"
    assert pre.lr == 0.01 and ft.lr == 0.001 and pre.decay == 0.0 and pre.clipnorm is None and ft.clipnorm is None
    assert not ft.accumulator_at_start.any() and not pre.accumulator_at_start.any()  # fresh accumulators
    assert ft.iterations == 192 // 32 and pre.iterations == 192 // 32               # each counted from zero
    assert {n for n in start if n.startswith("embedding.")} == {"embedding.weight", "embedding.bias"}
    assert {n for n, p in pre.model.named_parameters() if n.startswith("embedding.")} and len(pre.flat.params) == 2
    assert len(ft.flat.params) == len(after_pre)
    for name, p in after_pre.items():
        if name.startswith("embedding."):
            assert name not in loaded and not torch.equal(p, start[name]), name      # the new layer: fresh, then trained
        else:
            same = torch.equal(p.view(torch.int32), loaded[name].to(p.device).view(torch.int32))
            assert same and torch.equal(start[name], loaded[name].to(p.device)), name
    final = torch.load(wts)
    assert any(not torch.equal(final[n].cpu(), after_pre[n].cpu()) for n in after_pre if not n.startswith("embedding."))
    assert all(torch.isfinite(v).all() for v in final.values() if v.is_floating_point())


def test_class_subset(tmp_path, capsys):
    import learn_devise as ld
    emb = _embedding_pickle(tmp_path, (3, 1, 4, 15, 9, 2, 6), 64)
    seen = []
    real = ld.build_losses
    try:
        ld.build_losses = lambda e, m: (seen.append(e), real(e, m))[1]
        final, feat, _, _ = _cli(ld, tmp_path, "sub", emb, "--ft_epochs", "1", "--no_progress", arch="resnet-32")
    finally:
        ld.build_losses = real
    assert len(seen) == 1 and tuple(seen[0].shape) == (7, 64)                        # a 7-row table
    assert torch.allclose(seen[0].norm(dim=-1), torch.ones(7, device=seen[0].device), atol=1e-6)
    assert np.isfinite(final["loss"]) and 0.0 <= final["max_sim_acc"] <= 1.0
    assert str([final["loss"], final["max_sim_acc"]]) in capsys.readouterr().out


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # RCCL refuses two ranks on one device; gloo all-reduces CUDA tensors
    torch.cuda.set_device(0)
    import learn_devise as ld
    import utils
    from datasets import SyntheticGenerator
    from engine import Trainer
    torch.manual_seed(0)
    model = utils.build_network(64, "resnet-32", input_channels=3).cuda()
    E = torch.nn.functional.normalize(torch.randn(100, 64), dim=-1).cuda()
    losses, metrics = ld.build_losses(E, 0.1)
    l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
    tr = Trainer(model, losses, metrics, lr=0.01, l2_of=l2_of, autocast_dtype=None, memory_format=torch.contiguous_format,
                 optimizer="adagrad")
    assert tr.world == 2 and tr.reducer.enabled
    gen = SyntheticGenerator(100, 32, 3, 256, 32)
    seq = gen.train_sequence(32, shuffle=False, rank=rank, world_size=world, batch_transform=ld.transform_inputs,
                             batch_transform_kwargs={"embedding": None})
    before = tr.flat.flat_p.detach().cpu().clone()
    ok = tr.enable_graphs(*seq[0])
    logs = {}
    for i in range(4):
        tr.train_step(*seq[i % len(seq)], logs)
    torch.cuda.synchronize()
    weights, accum = tr.flat.flat_p.detach().cpu(), tr.flat.flat_v.detach().cpu()
    both = [None, None]
    dist.all_gather_object(both, weights.numpy().tobytes() + accum.numpy().tobytes())
    if rank == 0:
        torch.save({"ok": ok, "same": both[0] == both[1], "moved": bool((weights != before).any()),
                    "finite": bool(torch.isfinite(weights).all()) and bool(torch.isfinite(accum).all()),
                    "accumulated": bool((accum > 0).any()) and bool((accum >= 0).all()), "n": float(logs["_n"]),
                    "acc": float(logs["max_sim_acc"])}, out)
    dist.destroy_process_group()


def test_world2_weights_and_accumulators_stay_identical(tmp_path):
    """Two processes (gloo) on the one GPU, 4 graph-mode Adagrad steps on their halves of the global batch: byte-identical flat_p and
    flat_v on both ranks (the mean over the ranks is the kernel's grad_scale)."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "w.pt")
    mp.spawn(_dp_worker, args=(2, 29671, out), nprocs=2, join=True)
    got = torch.load(out)
    assert got["ok"] and got["same"] and got["moved"] and got["finite"] and got["accumulated"], got
    assert got["n"] == 64.0 and 0.0 <= got["acc"] <= 64.0
