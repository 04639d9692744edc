"""CPU: the softmax classifier's loss entry points (exports, host-side argument checks), learn_classifier.py's command line against
the flag names and defaults recorded from the reference, its transform_inputs / --class_list rules, and the float64 oracle of the
GPU tests against Keras' own formula as the fixture recorded it (tools/make_classifier_golden.py)."""
import argparse
import ctypes
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
# Keras clips the float32 probabilities to [float32(1e-7), float32(1) - float32(1e-7)] = [1.00000001e-7, 1 - 2^-23]
LO64, HI64 = -np.log(np.float64(np.float32(1) - np.float32(1e-7))), -np.log(np.float64(np.float32(1e-7)))
LO32, HI32 = np.float32(1.1920929e-7), np.float32(16.118095)        # the constants of include/sehip.h
WINDOW = 2.0 ** -15       # |t_c - HI| below which float32 may decide the lower clip either way


def fixture():
    return np.load(os.path.join(GOLDEN, "classifier_xent.npz"))


def target(labels, C, s):
    """Y [B, C] float64 of se_softmax_xent_*: the float32 values 1 - s and s / (C - 1) for 0 < s < 1, one-hot for any other s."""
    s = float(np.float32(s))
    on, off = (np.float32(1.0 - s), np.float32(s / (C - 1))) if 0.0 < s < 1.0 else (np.float32(1), np.float32(0))
    Y = np.full((len(labels), C), np.float64(off))
    Y[np.arange(len(labels)), np.clip(labels, 0, C - 1)] = np.float64(on)
    return Y


class Oracle(object):
    """The arithmetic of se_softmax_xent_fwd / _bwd (include/sehip.h) in float64 on the float32 (or bf16-rounded) logits ``z``
    [B, C], with the error bounds the GPU tests hold the kernels to."""

    def __init__(self, z, labels, s):
        z = np.asarray(z, dtype=np.float64)
        B, C = z.shape
        self.B, self.C = B, C
        self.y = np.clip(np.asarray(labels, dtype=np.int64), 0, C - 1)
        self.Y = target(self.y, C, s)
        with np.errstate(all="ignore"):
            self.m = z.max(-1, keepdims=True) if C else np.zeros((B, 1))
            self.lse = self.m + np.log(np.exp(z - self.m).sum(-1, keepdims=True))
            self.t = self.lse - z
            self.q = np.exp(z - self.lse)
            self.loss = np.where(self.Y > 0, self.Y * np.clip(self.t, LO64, HI64), 0.0).sum(-1)
            self.a = np.where((self.t >= LO64) & (self.t <= HI64), self.Y, 0.0)
            self.A = self.a.sum(-1, keepdims=True)
            self.dz = self.A * self.q - self.a                    # for w = 1
            # bounds (the issue's): K = 8 + 2 log2 C; e_c = K u (|z_c - m| + (lse - m) + 1); loss: sum_c Y_c e_c
            K = 8.0 + 2.0 * np.log2(C)
            self.e = K * U * (np.abs(z - self.m) + (self.lse - self.m) + 1.0)
            self.loss_bound = np.where(self.Y > 0, self.Y * self.e, 0.0).sum(-1)
            self.in_window = np.abs(self.t - HI64) < WINDOW
            grad_bound = self.A * self.q * (self.e + 6.0 * U) + U * self.a + 2.0 ** -22 * self.Y.max(-1, keepdims=True)
            # a class inside the window may be decided either way: dz_k then moves by Y_c ((k == c) + q_k)
            wY = np.where(self.in_window, self.Y, 0.0)
            self.grad_bound = np.where(np.isfinite(grad_bound), grad_bound, np.inf) + wY + wY.sum(-1, keepdims=True) * self.q
        self.bad = np.isnan(z).any(-1) | (z == np.inf).any(-1) | (z == -np.inf).all(-1)      # the last: no softmax at all
        self.loss = np.where(self.bad, np.nan, self.loss)
        self.best = np.array([int(np.argmax(r)) for r in z], dtype=np.int64)      # np.argmax: the first NaN, else the first maximum
        zy = z[np.arange(B), self.y]
        with np.errstate(invalid="ignore"):
            self.above = np.where(self.bad, C, (z > zy[:, None]).sum(-1))


def fixed_order_mean(loss_i):
    """loss_mean of include/sehip.h in float32: thread j of 256 adds loss_i[j], loss_i[j + 256], ... in order, then a binary tree
    over the 256 partial sums, divided by B; +0 for B = 0."""
    v = np.asarray(loss_i, dtype=np.float32)
    if len(v) == 0:
        return np.float32(0)
    part = np.zeros(256, dtype=np.float32)
    for j in range(min(256, len(v))):
        acc = np.float32(0)
        for x in v[j::256]:
            acc = np.float32(acc + x)
        part[j] = acc
    off = 128
    while off:
        part[:off] = part[:off] + part[off:2 * off]
        off //= 2
    return np.float32(part[0] / np.float32(len(v)))


# ---------------------------------------------------------------- the C ABI without a device

def test_library_exports_the_softmax_xent_symbols():
    import sehip
    lib = sehip.lib()
    for name in ("se_softmax_xent_aux_floats", "se_softmax_xent_fwd", "se_softmax_xent_bwd"):
        assert name in sehip.EXPORTS and hasattr(lib, name), name
    assert lib.se_softmax_xent_aux_floats(0) == 0 and lib.se_softmax_xent_aux_floats(7) == 21


def test_entry_points_check_their_arguments_without_a_gpu():
    import sehip
    lib = sehip.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def fwd(logits=one, dtype=0, ld=4, labels=one, B=2, C=3, s=0.0, loss_i=one, aux=one):
        return lib.se_softmax_xent_fwd(logits, dtype, ld, labels, B, C, s, loss_i, aux, z, z, z, z)

    def bwd(logits=one, dtype=0, ld=4, labels=one, aux=one, B=2, C=3, s=0.0, dz=one, ddtype=0, ldd=4):
        return lib.se_softmax_xent_bwd(logits, dtype, ld, labels, aux, z, 1.0, B, C, s, dz, ddtype, ldd, z)

    for f, who in ((fwd, b"se_softmax_xent_fwd"), (bwd, b"se_softmax_xent_bwd")):
        for C in (0, -1):
            assert f(C=C) == -1 and who + b": bad shape" in lib.se_last_error()
        assert f(B=-1) == -1 and who + b": bad shape" in lib.se_last_error()
        assert f(C=1, s=0.1) == -1 and b"label smoothing" in lib.se_last_error() and who in lib.se_last_error()
        assert f(C=5, ld=4) == -1 and who + b": leading dimension" in lib.se_last_error()
        assert f(aux=z) == -1 and who + b": null pointer" in lib.se_last_error()
        assert f(logits=z) == -1 and f(labels=z) == -1
        for dtype in (2, -1):
            assert f(dtype=dtype) == -1 and who + b": bad dtype" in lib.se_last_error()
        # B = 0 is accepted, with every pointer NULL (loss_mean NULL: nothing to write, nothing launched)
        assert f(logits=z, labels=z, aux=z, B=0) == 0
        # s outside (0, 1) is one-hot: C = 1 is then legal -- the shape check passes and the next one (null pointer) answers
        assert f(C=1, s=1.5, aux=z) == -1 and b"null pointer" in lib.se_last_error()
    assert fwd(loss_i=z) == -1 and b"null pointer" in lib.se_last_error()
    assert bwd(dz=z) == -1 and b"null pointer" in lib.se_last_error()
    assert bwd(ddtype=3) == -1 and b"bad dtype" in lib.se_last_error()
    assert bwd(ldd=2) == -1 and b"leading dimension" in lib.se_last_error()


def test_softmax_cross_entropy_refuses_host_tensors():
    import sehip
    z = torch.randn(4, 8, requires_grad=True)          # host tensors are refused with or without a device
    y = torch.zeros(4, dtype=torch.long)
    with pytest.raises(sehip.SehipError):
        sehip.softmax_cross_entropy(z, y)
    with pytest.raises(sehip.SehipError):
        sehip.softmax_cross_entropy(z.detach(), y, label_smoothing=0.1, reduction="mean", return_metrics=True)
    import learn_classifier as lc
    with pytest.raises(sehip.SehipError):
        lc.SoftmaxCrossEntropy(0.1)(y, z)
    with pytest.raises(sehip.SehipError):
        lc.SoftmaxCrossEntropy(0.0).acc(y, z)          # a metric on its own computes itself -- on the kernel, nowhere else


# ---------------------------------------------------------------- the command line

def test_parser_has_exactly_the_reference_flags_and_defaults():
    import learn_classifier as lc
    import utils
    flags = json.loads(str(fixture()["flags"]))
    assert {"label_smoothing", "top_k_acc", "snapshot_best", "class_list", "sgd_lr"} <= set(flags)
    p = lc.build_parser()
    acts = {a.dest: a for a in p._actions if a.dest != "help"}
    assert sorted(acts) == sorted(flags)
    required = sorted(k for k, v in flags.items() if v["required"])
    assert required == ["data_root", "dataset"] and all(acts[k].required for k in required)
    args = p.parse_args(["--dataset", "d", "--data_root", "r"])
    for name, spec in flags.items():
        if not spec["required"]:
            assert getattr(args, name) == spec["default"], name
    assert args.finetune_init == 3 and args.label_smoothing == 0.0 and args.top_k_acc == []
    assert acts["architecture"].choices == utils.ARCHITECTURES and acts["lr_schedule"].choices == utils.LR_SCHEDULES
    groups = [g.title for g in p._action_groups]
    assert groups[2:5] == ["Data parameters", "Training parameters", "Output parameters"]      # after argparse's two own groups
    sched = argparse.ArgumentParser()
    utils.add_lr_schedule_arguments(sched)
    assert [g.title for g in sched._action_groups][2:] == groups[5:]
    a = p.parse_args(["--dataset", "d", "--data_root", "r", "--label_smoothing", "0.1", "--top_k_acc", "5", "10", "--snapshot", "s.pt",
                      "--snapshot_best", "--initial_epoch", "3", "--finetune", "w.pt", "--finetune_init", "1", "--class_list", "c.txt",
                      "--architecture", "resnet-110-fc", "--nesterov", "--gpu_merge", "--no_progress", "--sgd_lr", "0.05"])
    assert (a.label_smoothing, a.top_k_acc, a.snapshot_best, a.initial_epoch, a.finetune_init, a.nesterov, a.sgd_lr) == \
        (0.1, [5, 10], "val_loss", 3, 1, True, 0.05)
    assert p.parse_args(["--dataset", "d", "--data_root", "r", "--snapshot_best", "val_acc"]).snapshot_best == "val_acc"


def test_the_scripts_share_one_class_list_reader_and_one_json_logger():
    import learn_center_loss as lcl
    import learn_classifier as lc
    import learn_image_embeddings as lie
    import train_cli
    assert lc.read_class_list is train_cli.read_class_list and lcl.read_class_list is train_cli.read_class_list
    assert lie.JsonLogger is train_cli.JsonLogger


def test_transform_inputs_and_losses():
    import learn_classifier as lc
    X, y = lc.transform_inputs("X", "y", 10, label_smoothing=0.1)
    assert X == "X" and y == "y"
    assert lc.transform_inputs("X", "y", 10) == ("X", "y")
    losses, metrics = lc.build_losses(0.1, [5, 10])
    assert list(losses) == ["prob"] and losses["prob"][1] == 1.0 and losses["prob"][0].label_smoothing == 0.1
    assert [m.name for m in metrics["prob"]] == ["acc", "acc5", "acc10"]
    assert [m.name for m in lc.build_losses(0.0)[1]["prob"]] == ["acc"]


def test_class_list_file(tmp_path):
    import learn_classifier as lc
    p = tmp_path / "classes.txt"
    p.write_text("5 five\n\n2 two\n   \n5 again\n3\n")
    assert lc.read_class_list(str(p)) == [5, 2, 3]                 # ints, first occurrence wins, blank lines skipped
    p.write_text("7 a\nn02 b\n7 c\n")
    assert lc.read_class_list(str(p)) == ["7", "n02"]              # one word that is no int: none is converted
    p.write_text("  n01 a\nn02\n")
    assert lc.read_class_list(str(p)) == ["n01", "n02"]


def test_classifier_model_names_its_last_layer_prob_and_taps_its_input():
    import learn_classifier as lc
    torch.manual_seed(0)
    model = lc.build_classifier(7, "resnet-32", input_channels=3)
    keys = set(model.state_dict())
    assert {"prob.weight", "prob.bias"} <= keys and not any(k.startswith("embedding.") for k in keys)
    assert lc.final_dense(model) is model.prob and model.prob.out_features == 7
    assert any(p is model.prob.weight for p in model.regularized_parameters())
    model.eval()
    tap = lc.FeatureTap(model)
    x = torch.randn(2, 3, 32, 32).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = model(x)
        assert out.shape == (2, 7) and not torch.allclose(out.sum(-1), torch.ones(2))          # logits, no softmax
        assert tap.value.shape == (2, 64) and torch.equal(tap.value, model.features(x))
    tap.close()
    # a BatchNorm directly in front of the final dense layer: the tap is that BatchNorm's input (learn_classifier.py:179)
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.body, self.bn, self.prob = torch.nn.Linear(5, 4), torch.nn.BatchNorm1d(4), torch.nn.Linear(4, 3)

        def forward(self, x):
            return self.prob(self.bn(self.body(x)))
    net = Net().eval()
    tap = lc.FeatureTap(net)
    x = torch.randn(6, 5)
    with torch.no_grad():
        net(x)
        assert torch.equal(tap.value, net.body(x)) and not torch.equal(tap.value, net.bn(net.body(x)))
    tap.close()


# ---------------------------------------------------------------- the oracle against Keras' formula

def test_oracle_reproduces_the_keras_values_of_the_fixture():
    """Loss and gradient of the float64 clamp form == Keras 2.2's categorical_crossentropy fed with the reference's own
    transform_inputs (float64, recorded by the tool); the float32 evaluation of Keras' formula passes the loss bound the kernels
    are held to; the licence window of the lower clip holds at most 0.1 % of every case."""
    fx = fixture()
    cases = [str(c) for c in fx["cases"]]
    assert len(cases) == 15
    worst = 0.0
    for key in cases:
        z, y, gcols = fx[key + "_logits"].astype(np.float32), fx[key + "_labels"], fx[key + "_gcols"]
        for si, s in enumerate(fx["smoothings"]):
            o = Oracle(z, y, s)
            ref64, ref32, g64 = fx["%s_s%d_loss64" % (key, si)], fx["%s_s%d_loss32" % (key, si)], fx["%s_s%d_grad64" % (key, si)]
            # the target values are float32 here (what the kernel gets) and float64 in the reference: 1 ulp of float32 on Y
            assert np.all(np.abs(o.loss - ref64) <= 2.0 * U * np.abs(ref64) + 1e-12), (key, s)
            assert np.all(np.abs(o.dz[:2][:, gcols] - g64) <= 2.0 * U * (np.abs(g64) + o.Y[:2][:, gcols]) + 1e-12), (key, s)
            ratio = np.abs(ref32.astype(np.float64) - ref64) / o.loss_bound
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (key, s, ratio.max())
            assert o.in_window.mean() <= 1e-3, (key, s)
    assert worst > 0.0


def test_oracle_rules_on_crafted_rows():
    z = np.array([[0, 30, 0, 0], [30, 0, 0, 0], [1, 2, 2, 1], [np.nan, 3, np.inf, 0], [-np.inf, 3, np.inf, np.inf], [-np.inf, 0, 0, 0]],
                 dtype=np.float32)
    y = np.array([0, 0, 3, 1, 1, 0])
    o = Oracle(z, y, 0.0)
    assert abs(o.loss[0] - HI32) <= 2 * U * HI32 and not o.dz[0].any()       # confidently wrong: capped, no gradient
    assert abs(o.loss[1] - LO32) <= 2 * U * LO32
    assert o.best.tolist() == [1, 0, 1, 0, 2, 1] and o.above.tolist() == [1, 0, 2, 4, 4, 3]
    assert np.isnan(o.loss[3]) and np.isnan(o.loss[4]) and abs(o.loss[5] - HI32) <= 2 * U * HI32
    assert fixed_order_mean(np.zeros(0)) == 0 and fixed_order_mean(np.arange(600, dtype=np.float32)) == np.float32(299.5)
    assert np.array_equal(target(np.array([1, 9, -2]), 3, 1.5), np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float64))
    t = target(np.array([1]), 3, 0.1)
    assert t[0, 1] == np.float64(np.float32(0.9)) and t[0, 0] == np.float64(np.float32(np.float32(0.1) / 2.0))
