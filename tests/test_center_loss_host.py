"""CPU: learn_center_loss.py's command line and model (the reference's flags, defaults, layer names and initialisers), and the
host-side argument checks of se_center_loss_centroid_grad and sehip.center_loss."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

# every flag of the reference's learn_center_loss.py:53-83 with its default (utils.add_lr_schedule_arguments adds the --sgd_* /
# --sgdr_* / --clr_* groups)
REFERENCE_FLAGS = {
    "dataset": None, "data_root": None, "class_list": None, "embed_dim": 100, "centroids": None, "center_loss_weight": 0.1,
    "architecture": "simple", "lr_schedule": "SGDR", "clipgrad": 10.0, "max_decay": 0.0, "nesterov": False, "epochs": None,
    "batch_size": 100, "val_batch_size": None, "finetune": None, "finetune_init": 3, "gpus": 1, "read_workers": 8, "queue_size": 100,
    "gpu_merge": False, "model_dump": None, "weight_dump": None, "feature_dump": None, "log_dir": None, "no_progress": False,
}


def test_parser_takes_every_reference_flag_with_its_default():
    import learn_center_loss as lcl
    import utils
    sched = argparse.ArgumentParser()
    utils.add_lr_schedule_arguments(sched)
    sched = {a.dest: a.default for a in sched._actions if a.dest != "help"}
    p = lcl.build_parser()
    acts = {a.dest: a for a in p._actions if a.dest != "help"}
    assert sorted(acts) == sorted(list(REFERENCE_FLAGS) + list(sched))
    assert acts["dataset"].required and acts["data_root"].required
    args = p.parse_args(["--dataset", "d", "--data_root", "r"])
    for name, default in list(REFERENCE_FLAGS.items())[2:] + list(sched.items()):
        assert getattr(args, name) == default, name
    assert acts["architecture"].choices == utils.ARCHITECTURES and acts["lr_schedule"].choices == utils.LR_SCHEDULES
    argv = ["--dataset", "d", "--data_root", "r", "--class_list", "c.txt", "--embed_dim", "64", "--centroids", "e.pickle",
            "--center_loss_weight", "0.5", "--architecture", "resnet-110-fc", "--lr_schedule", "SGD", "--clipgrad", "5", "--max_decay",
            "0.1", "--nesterov", "--epochs", "3", "--batch_size", "32", "--val_batch_size", "64", "--finetune", "w.pt",
            "--finetune_init", "1", "--gpus", "2", "--read_workers", "4", "--queue_size", "10", "--gpu_merge", "--model_dump", "m.pt",
            "--weight_dump", "w2.pt", "--feature_dump", "f.pickle", "--log_dir", "log", "--no_progress", "--sgd_lr", "0.05"]
    a = p.parse_args(argv)
    assert (a.embed_dim, a.center_loss_weight, a.finetune_init, a.nesterov, a.gpu_merge, a.no_progress, a.sgd_lr) == \
        (64, 0.5, 1, True, True, True, 0.05)
    with pytest.raises(SystemExit):
        p.parse_args(["--dataset", "d", "--data_root", "r", "--lr_schedule", "cosine"])


def _backbone():
    import utils
    torch.manual_seed(0)
    return utils.build_network(100, "resnet-110-fc", input_channels=3)


def test_model_layer_names_initialisers_and_outputs():
    import learn_center_loss as lcl
    from models.cifar_resnet import KERAS_BN_EPS, KERAS_BN_MOMENTUM
    model = lcl.CenterLossModel(_backbone(), 10)
    keys = set(model.state_dict())
    assert {"embedding_bn.weight", "embedding_bn.bias", "embedding_bn.running_mean", "embedding_bn.running_var", "prob.weight",
            "prob.bias", "cls_centroids.weight", "embed_model.embedding.weight"} <= keys
    assert all(k.split(".")[0] in ("embed_model", "embedding_bn", "prob", "cls_centroids") for k in keys)
    assert isinstance(model.cls_centroids, torch.nn.Embedding) and model.cls_centroids.weight.shape == (10, 100)
    c = model.cls_centroids.weight.detach()
    assert model.cls_centroids.weight.requires_grad
    assert float(c.abs().max()) <= 0.05 and float(c.abs().max()) > 0.04 and abs(float(c.mean())) < 0.01      # U(-0.05, 0.05)
    bn = model.embedding_bn
    assert isinstance(bn, torch.nn.BatchNorm1d) and bn.eps == KERAS_BN_EPS == 1e-3 and bn.momentum == KERAS_BN_MOMENTUM == 0.01
    assert model.prob.weight.shape == (10, 100) and not model.prob.bias.detach().any()
    lim = np.sqrt(6.0 / (100 + 10))                                                              # Keras' glorot_uniform
    assert float(model.prob.weight.detach().abs().max()) <= lim
    model.eval()
    with torch.no_grad():
        logits, emb = model(torch.randn(2, 3, 32, 32).contiguous(memory_format=torch.channels_last))
    assert logits.shape == (2, 10) and emb.shape == (2, 100)
    X, ys = lcl.transform_inputs("X", "y", 10)
    assert X == "X" and ys == ["y", "y"]


def test_fixed_centroids_are_not_trainable():
    import learn_center_loss as lcl
    E = np.random.default_rng(0).standard_normal((7, 100))
    model = lcl.center_loss_model(_backbone(), E)
    w = model.cls_centroids.weight
    assert not w.requires_grad and torch.equal(w.detach(), torch.from_numpy(E.astype(np.float32)))
    assert model.prob.out_features == 7
    assert lcl.center_loss_model(_backbone(), 7).cls_centroids.weight.requires_grad
    losses, metrics = lcl.build_losses(model, 0.1)
    assert list(losses) == ["prob", "center_loss"] and losses["center_loss"][1] == 0.1 and losses["prob"][1] == 1.0
    assert losses["center_loss"][0].centroids is w and list(metrics) == ["prob"]


def test_class_list_file(tmp_path):
    import learn_center_loss as lcl
    p = tmp_path / "classes.txt"
    p.write_text("5 five\n\n2 two\n5 again\n3\n")
    assert lcl.read_class_list(str(p)) == [5, 2, 3]
    p.write_text("n01 a\nn02\n")
    assert lcl.read_class_list(str(p)) == ["n01", "n02"]


def test_centroid_grad_entry_point_checks_its_arguments_without_a_gpu():
    import sehip
    lib = sehip.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    # se_center_loss_centroid_grad(x, x_dtype, ldx, labels, centroids, ldc, grad_loss_i, grad_scale, B, D, C, dcent, lddc, stream)
    for args in ((z, 0, 4, one, one, 4, z, 1.0, 2, 4, 3, one, 4, z),        # x
                 (one, 0, 4, z, one, 4, z, 1.0, 2, 4, 3, one, 4, z),        # labels
                 (one, 0, 4, one, z, 4, z, 1.0, 2, 4, 3, one, 4, z),        # centroids
                 (one, 0, 4, one, one, 4, z, 1.0, 2, 4, 3, z, 4, z),        # dcent
                 (z, 0, 4, z, one, 4, z, 1.0, 0, 4, 3, z, 4, z)):           # B = 0 still writes dcent
        assert lib.se_center_loss_centroid_grad(*args) == -1
        assert b"se_center_loss_centroid_grad: null pointer" in lib.se_last_error()
    for B, D, C in ((-1, 4, 3), (2, 0, 3), (2, 4, 0)):
        assert lib.se_center_loss_centroid_grad(one, 0, 4, one, one, 4, z, 1.0, B, D, C, one, 4, z) == -1
        assert b"se_center_loss_centroid_grad: bad shape" in lib.se_last_error()
    for ldx, ldc, lddc in ((3, 4, 4), (4, 3, 4), (4, 4, 3)):
        assert lib.se_center_loss_centroid_grad(one, 0, ldx, one, one, ldc, z, 1.0, 2, 4, 3, one, lddc, z) == -1
        assert b"se_center_loss_centroid_grad: leading dimension" in lib.se_last_error()
    for dtype in (2, -1):
        assert lib.se_center_loss_centroid_grad(one, dtype, 4, one, one, 4, z, 1.0, 2, 4, 3, one, 4, z) == -1
        assert b"se_center_loss_centroid_grad: bad dtype" in lib.se_last_error()


def test_center_loss_refuses_host_tensors():
    import sehip
    x = torch.randn(4, 8, requires_grad=True)
    y = torch.zeros(4, dtype=torch.long)
    c = torch.randn(3, 8, requires_grad=True)
    with pytest.raises(sehip.SehipError):
        sehip.center_loss(x, y, c)
    with pytest.raises(sehip.SehipError):
        sehip.center_loss(x.detach(), y, c.detach(), reduction="mean")
