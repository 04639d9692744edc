"""CPU: learn_labelembedding.py's command line and model (the reference's flags, defaults, layer names and initialisers), the
host-side argument checks of se_labelembed_table_loss_fwd / _bwd, the NumPy restatement of the table gradient's accumulation rule
and the table of GPU cases (tests/test_gpu_labelembed_table.py imports both) with the boundaries of the kernel it has to reach."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

# every flag of the reference's learn_labelembedding.py:68-99 with its default (utils.add_lr_schedule_arguments adds the --sgd_* /
# --sgdr_* / --clr_* groups)
REFERENCE_FLAGS = {
    "dataset": None, "data_root": None, "class_list": None, "embed_dim": 100, "tau": 2.0, "alpha": 0.9, "beta": 0.5,
    "architecture": "simple", "lr_schedule": "SGDR", "clipgrad": 10.0, "max_decay": 0.0, "nesterov": False, "epochs": None,
    "batch_size": 100, "val_batch_size": None, "finetune": None, "finetune_init": 3, "gpus": 1, "read_workers": 8, "queue_size": 100,
    "gpu_merge": False, "model_dump": None, "weight_dump": None, "feature_dump": None, "log_dir": None, "no_progress": False,
}


def test_parser_takes_every_reference_flag_with_its_default():
    import learn_labelembedding as ll
    import utils
    sched = argparse.ArgumentParser()
    utils.add_lr_schedule_arguments(sched)
    sched = {a.dest: a.default for a in sched._actions if a.dest != "help"}
    p = ll.build_parser()
    acts = {a.dest: a for a in p._actions if a.dest != "help"}
    assert sorted(acts) == sorted(list(REFERENCE_FLAGS) + list(sched))          # no snapshot flags: the reference has none here
    assert acts["dataset"].required and acts["data_root"].required
    for argv in (["--dataset", "d"], ["--data_root", "r"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    args = p.parse_args(["--dataset", "d", "--data_root", "r"])
    for name, default in list(REFERENCE_FLAGS.items())[2:] + list(sched.items()):
        assert getattr(args, name) == default, name
    assert acts["architecture"].choices == utils.ARCHITECTURES and acts["lr_schedule"].choices == utils.LR_SCHEDULES
    argv = ["--dataset", "d", "--data_root", "r", "--class_list", "c.txt", "--embed_dim", "64", "--tau", "3", "--alpha", "0.8", "--beta",
            "0.25", "--architecture", "resnet-110-fc", "--lr_schedule", "SGD", "--clipgrad", "5", "--max_decay", "0.1", "--nesterov",
            "--epochs", "3", "--batch_size", "32", "--val_batch_size", "64", "--finetune", "w.pt", "--finetune_init", "1", "--gpus", "2",
            "--read_workers", "4", "--queue_size", "10", "--gpu_merge", "--model_dump", "m.pt", "--weight_dump", "w2.pt",
            "--feature_dump", "f.pickle", "--log_dir", "log", "--no_progress", "--sgd_lr", "0.05"]
    a = p.parse_args(argv)
    assert (a.class_list, a.embed_dim, a.tau, a.alpha, a.beta, a.architecture, a.lr_schedule, a.clipgrad, a.max_decay, a.nesterov,
            a.epochs, a.batch_size, a.val_batch_size, a.finetune, a.finetune_init, a.gpus, a.read_workers, a.queue_size, a.gpu_merge,
            a.model_dump, a.weight_dump, a.feature_dump, a.log_dir, a.no_progress, a.sgd_lr) == \
        ("c.txt", 64, 3.0, 0.8, 0.25, "resnet-110-fc", "SGD", 5.0, 0.1, True, 3, 32, 64, "w.pt", 1, 2, 4, 10, True, "m.pt", "w2.pt",
         "f.pickle", "log", True, 0.05)
    for bad in (["--lr_schedule", "cosine"], ["--architecture", "alexnet"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--dataset", "d", "--data_root", "r"] + bad)


def _model(C=10):
    import learn_labelembedding as ll
    import utils
    torch.manual_seed(0)
    return ll.labelembed_model(utils.build_network(100, "resnet-110-fc", input_channels=3), C, tau=3.0, alpha=0.8, beta=0.25)


def test_model_layer_names_initialisers_and_trainer_form():
    import learn_labelembedding as ll
    from models.cifar_resnet import KERAS_BN_EPS, KERAS_BN_MOMENTUM
    model = _model()
    assert {k.split(".")[0] for k in model.state_dict()} == {"base_model", "embedding_bn", "prob", "out2", "labelembeddings"}
    assert {"labelembeddings.weight", "prob.weight", "prob.bias", "out2.weight", "out2.bias", "embedding_bn.weight",
            "embedding_bn.running_var", "base_model.embedding.weight"} <= set(model.state_dict())
    table = model.labelembeddings.weight
    assert isinstance(model.labelembeddings, torch.nn.Embedding) and table.requires_grad
    assert torch.equal(table.detach(), torch.eye(10))
    bn = model.embedding_bn
    assert isinstance(bn, torch.nn.BatchNorm1d) and bn.eps == KERAS_BN_EPS == 1e-3 and bn.momentum == KERAS_BN_MOMENTUM == 0.01
    assert model.prob.weight.shape == (10, 100) and model.out2.weight.shape == (10, 100)
    assert model.kwargs == dict(tau=3.0, alpha=0.8, beta=0.25)
    model.eval()
    with torch.no_grad():
        logits2, out1, emb = model(torch.randn(2, 3, 32, 32).contiguous(memory_format=torch.channels_last))
    assert logits2.shape == (2, 20) and out1.shape == (2, 10) and emb.shape == (2, 100)
    assert torch.equal(logits2[:, :10], out1)
    out = model.embedding_bn(torch.relu(emb))
    assert torch.allclose(logits2[:, 10:], model.out2(out), atol=1e-6)
    # the losses the trainer is built with: the reference's compile()
    losses, metrics = ll.build_losses(model)
    assert list(losses) == ["labelembed_loss", "prob"] and [w for _, w in losses.values()] == [1.0, 1.0]
    assert losses["labelembed_loss"][0].table is table and losses["labelembed_loss"][0].kwargs == model.kwargs
    zero = losses["prob"][0](torch.zeros(2, dtype=torch.long), out1)
    assert zero.shape == (2,) and not zero.any()
    assert list(metrics) == ["prob"] and [m.name for m in metrics["prob"]] == ["acc"]


def test_out2_sees_a_detached_input():
    """Lambda(K.stop_gradient) in front of out2 (learn_labelembedding.py:47): with a plain-torch stand-in for the loss that depends on
    the out2 half only, the head out2 gets a gradient and nothing upstream of it does."""
    model = _model()
    x = torch.randn(4, 3, 32, 32).contiguous(memory_format=torch.channels_last)
    logits2, out1, emb = model(x)
    torch.logsumexp(logits2[:, 10:], dim=1).sum().backward()
    assert model.out2.weight.grad.abs().sum() > 0
    for name, p in model.named_parameters():
        if not name.startswith("out2."):
            assert p.grad is None or not p.grad.any(), name
    model.zero_grad()
    logits2, out1, emb = model(x)
    torch.logsumexp(logits2[:, :10], dim=1).sum().backward()
    assert model.base_model.embedding.weight.grad.abs().sum() > 0 and model.prob.weight.grad.abs().sum() > 0
    assert model.out2.weight.grad is None or not model.out2.weight.grad.any()


def test_batch_transforms():
    import learn_labelembedding as ll
    X, y = torch.zeros(3, 2), torch.tensor([1, 0, 2])
    (X2, y2), targets = ll.transform_inputs(X, y, 3)                        # the reference's form, unchanged
    assert X2 is X and y2 is y and sorted(targets) == ["labelembed_loss", "prob"]
    assert targets["labelembed_loss"].shape == (3, 1) and not targets["labelembed_loss"].any() and targets["prob"] is y
    assert ll.transform_trainer_inputs("X", "y", 3) == ("X", ["y", "y"])


def test_ops_are_exported_and_refuse_host_tensors():
    import sehip
    assert {"labelembed_table_loss", "labelembed_table_loss_packed", "labelembed_loss", "LE_GRID_CAP"} <= set(sehip.ops.__all__)
    assert sehip.LE_GRID_CAP == LE_GRID_CAP
    o = torch.randn(4, 6, requires_grad=True)
    with pytest.raises(sehip.SehipError):
        sehip.labelembed_table_loss(o[:, :3], o[:, 3:], torch.eye(3), torch.zeros(4, dtype=torch.long))
    with pytest.raises(sehip.SehipError):
        sehip.labelembed_table_loss_packed(o, torch.eye(3), torch.zeros(4, dtype=torch.long))


def test_table_entry_points_check_their_arguments_without_a_gpu():
    import sehip
    lib = sehip.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    B, C = 2, 4

    def fwd(out1=one, ld1=C, out2=one, ld2=C, table=one, ldtab=C, targets=one, B=B, C=C, tau=2.0, loss_i=one, aux=one):
        return lib.se_labelembed_table_loss_fwd(out1, ld1, out2, ld2, table, ldtab, targets, B, C, tau, 0.9, 0.5, loss_i, aux, z)

    def bwd(out1=one, ld1=C, out2=one, ld2=C, table=one, ldtab=C, targets=one, B=B, C=C, tau=2.0, aux=one, d1=one, ldd1=C, d2=one,
            ldd2=C, dtab=one, lddtab=C):
        return lib.se_labelembed_table_loss_bwd(out1, ld1, out2, ld2, table, ldtab, targets, z, 1.0, B, C, tau, 0.9, 0.5, aux, d1, ldd1,
                                                d2, ldd2, dtab, lddtab, z)

    for fn, name, pointers, pitches in (
            (fwd, b"se_labelembed_table_loss_fwd", ("out1", "out2", "table", "targets", "loss_i", "aux"), ("ld1", "ld2", "ldtab")),
            (bwd, b"se_labelembed_table_loss_bwd", ("out1", "out2", "table", "targets", "aux"),
             ("ld1", "ld2", "ldtab", "ldd1", "ldd2", "lddtab"))):
        for p in pointers:
            assert fn(**{p: z}) == -1, p
            assert name + b": null pointer" in lib.se_last_error()
        for p in pitches:
            assert fn(**{p: C - 1}) == -1, p
            assert name + b": leading dimension" in lib.se_last_error()
        for tau in (0.0, -1.0, float("nan")):
            assert fn(tau=tau) == -1
            assert name + b": tau" in lib.se_last_error()
        for shape in (dict(B=-1), dict(C=0), dict(C=-3)):
            assert fn(**shape) == -1
            assert name + b": bad shape" in lib.se_last_error()
    # B == 0: nothing to compute and no row input is looked at (a d_table would still be zeroed -- on a device)
    assert fwd(out1=z, out2=z, table=z, targets=z, B=0, loss_i=z, aux=z) == 0
    assert bwd(out1=z, out2=z, table=z, targets=z, B=0, aux=z, d1=z, d2=z, dtab=z) == 0
    # a NULL output of the backward pass needs no pitch
    assert bwd(d1=z, ldd1=0, d2=z, ldd2=0, dtab=z, lddtab=0) == 0


# ------------------------------------------------------------------ the accumulation rule of d_table, restated

def table_grad_rule(d_tar, labels, C):
    """se_labelembed_table_loss_bwd's rule for d_table in float32: every row starts at +0 and takes one float32 addition of
    ``d_tar[i]`` (what se_labelembed_loss_bwd writes for sample i on the gathered rows) per sample of its class (labels clamped to
    [0, C - 1]) in increasing i.  Classes the batch does not hold stay +0."""
    d_tar = np.asarray(d_tar)
    assert d_tar.dtype == np.float32
    out = np.zeros((C, C), dtype=np.float32)
    for i, k in enumerate(np.clip(np.asarray(labels), 0, C - 1)):
        out[k] = out[k] + d_tar[i]
    return out


def test_table_grad_rule_is_ordered_float32_addition():
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    d = np.array([[big, 0], [one, 0], [one, 0], [-big, 0]], dtype=np.float32)
    assert table_grad_rule(d, [0, 0, 0, 0], 2)[0, 0] == 0.0                 # (2^24 + 1) + 1 - 2^24 in float32, in this order
    assert table_grad_rule(d[[1, 2, 0, 3]], [0, 0, 0, 0], 2)[0, 0] == 2.0   # another order, another sum
    got = table_grad_rule(np.array([[-0.0, 1.0], [2.0, 3.0]], dtype=np.float32), [7, -2], 2)
    assert np.array_equal(got.view(np.int32), np.array([[2.0, 3.0], [0.0, 1.0]], dtype=np.float32).view(np.int32))   # -0 + +0 = +0


# ------------------------------------------------------------------ the GPU cases and the boundaries they have to reach

LE_GRID_CAP = 4096              # SE_LABELEMBED_GRID_CAP: workgroups of the per-sample kernels ...
ROWS_PER_BLOCK = 4              # ... of LE_ROWS_PER_BLOCK samples each; larger batches stride
BALLOT = 64                     # labels one ballot of the table-gradient kernel scans
LABELS_IN_FLIGHT = 4 * BALLOT   # class_scan::CHUNKS chunks of labels are loaded together: longer batches go round the outer loop again
ROWS_TOGETHER = 4               # class_scan::ROWS matched rows are loaded together: more matches in one ballot go round the walk again
COLS_PER_WAVE = 4 * 64          # class_scan::COLS columns per lane: wider tables take more than one column block (gridDim.y)
# The grid of the table-gradient kernel is not capped: one wave per (table row, column block), so no row loop exists to reach.

CONTIG, PADDED, COL1 = "contig", "padded", "col1"     # tests/test_gpu_loss_matrix.py's input layouts

# (B, C, layout)
TABLE_CASES = [
    (1, 1, CONTIG),
    (7, 5, COL1),
    (37, 100, PADDED),
    (300, 3, CONTIG),
    (130, 1025, CONTIG),
    (70, 2049, PADDED),
    (LE_GRID_CAP * ROWS_PER_BLOCK + 9, 5, PADDED),
]
NO_MASK_CASE = TABLE_CASES[2]       # run once more with no row of mask = 1: the batch scale is B / 1e-8 and d_table all +0


GROUP_CLASSES = 12              # classes of scan_group_labels: 0 - 8 with fixed counts per ballot, 9 - 11 take the other rows


def scan_group_labels(B, rng):
    """Labels that fix where the per-class scan (csrc/class_scan.h; centroid and table gradients) cuts its groups of ROWS_TOGETHER rows:
    in every full ballot of 64 rows class k = 0 ... 8 holds exactly k + 1 rows at random positions (group remainders 1, 2, 3, 0 over one,
    two and three groups), in a partial last ballot classes 0 ... 7 do; the other rows fall in classes 9 - 11."""
    y = np.empty(B, dtype=np.int64)
    for c0 in range(0, B, BALLOT):
        n = min(BALLOT, B - c0)
        counted = np.arange(9 if n == BALLOT else 8)
        fixed = np.repeat(counted, counted + 1)
        assert fixed.size <= n
        y[c0:c0 + n] = rng.permutation(np.concatenate([fixed, rng.integers(9, GROUP_CLASSES, size=n - fixed.size)]))
    return y


def test_scan_group_labels_fix_every_group_remainder():
    B = 300                                                                     # four full ballots and one of 44 rows
    y = scan_group_labels(B, np.random.default_rng(3))
    assert y.min() == 0 and y.max() < GROUP_CLASSES
    for c0 in range(0, B, BALLOT):
        chunk = y[c0:c0 + BALLOT]
        counted = 9 if chunk.size == BALLOT else 8
        assert [int((chunk == k).sum()) for k in range(counted)] == list(range(1, counted + 1))
        assert (chunk >= counted).sum() == chunk.size - counted * (counted + 1) // 2 and (chunk[chunk >= counted] >= 9).all()
    per_ballot = np.arange(1, 10)
    assert {int(n % ROWS_TOGETHER) for n in per_ballot} == {0, 1, 2, 3} and {int(-(-n // ROWS_TOGETHER)) for n in per_ballot} == {1, 2, 3}
    # the ordered float32 rule takes the pattern and gives every counted class a gradient
    d_tar = np.random.default_rng(4).standard_normal((B, GROUP_CLASSES)).astype(np.float32)
    assert (table_grad_rule(d_tar, y, GROUP_CLASSES)[:9] != 0).all()


def pitch(layout, d):
    return {CONTIG: d, PADDED: (d // 8 + 2) * 8, COL1: d + 1}[layout]


def case_inputs(case, all_masked_out=False):
    """(out1, out2, table, labels, g) of a case: logits of scale 2, every second row with its true class boosted by 7 in out2 (mask = 1
    and an active ReLU term: the recipe of tests/test_gpu_loss.py), labels below 0 and above C - 1 among them.  ``all_masked_out``:
    out2 is lowest at the true class instead, so that no row has mask = 1."""
    B, C, _ = case
    rng = np.random.default_rng(700 + TABLE_CASES.index(case))
    o1, o2 = (rng.standard_normal((B, C)).astype(np.float32) * 2 for _ in range(2))
    table = (np.eye(C) + 0.5 * rng.standard_normal((C, C))).astype(np.float32)
    y = rng.integers(0, C, size=B)
    if all_masked_out:
        o2[np.arange(B), y] -= 30.0
    else:
        o2[np.arange(B)[::2], y[::2]] += 7.0
    y[1::5] = -3
    y[3::7] = C + 7
    g = rng.standard_normal(B).astype(np.float32)
    return o1, o2, table, y, g


def test_table_cases_reach_every_boundary():
    assert {(1, 1), (7, 5), (37, 100), (300, 3), (130, 1025), (70, 2049), (LE_GRID_CAP * 4 + 9, 5)} <= {c[:2] for c in TABLE_CASES}
    assert {c[2] for c in TABLE_CASES} == {CONTIG, PADDED, COL1}
    assert any(pitch(c[2], c[1]) > c[1] and c[1] >= 100 for c in TABLE_CASES)                   # ldtab > C on a real table
    assert {(B + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK > LE_GRID_CAP for B, _, _ in TABLE_CASES} == {False, True}
    assert {B > BALLOT for B, _, _ in TABLE_CASES} == {False, True}                             # more than one ballot
    assert {B > LABELS_IN_FLIGHT for B, _, _ in TABLE_CASES} == {False, True}                   # more than one round of label loads
    assert any(B % BALLOT for B, _, _ in TABLE_CASES if B > BALLOT)                             # a last ballot that is not full
    assert {(C + COLS_PER_WAVE - 1) // COLS_PER_WAVE for _, C, _ in TABLE_CASES} >= {1, 5, 9}   # column blocks, the last one partial
    assert any(C % 64 for _, C, _ in TABLE_CASES if C > COLS_PER_WAVE)
    most = {}
    for case in TABLE_CASES:
        B, C, _ = case
        o1, o2, table, y, g = case_inputs(case)
        yc = np.clip(y, 0, C - 1)
        assert (y < 0).any() or B < 2
        assert (y > C - 1).any() or B < 4
        mask = o2.argmax(1) == yc
        assert mask.any() or B < 2
        assert (~mask).any() or B < 2                                                           # rows the kernel skips (wt = 0)
        live = np.flatnonzero(mask)
        per_ballot = np.zeros(((B + BALLOT - 1) // BALLOT, C), dtype=np.int64)
        np.add.at(per_ballot, (live // BALLOT, yc[live]), 1)
        most[case[:2]] = per_ballot.max()
    o2 = case_inputs(NO_MASK_CASE, all_masked_out=True)[1]
    assert not (o2.argmax(1) == np.clip(case_inputs(NO_MASK_CASE)[3], 0, NO_MASK_CASE[1] - 1)).any()
    assert most[(300, 3)] > 2 * ROWS_TOGETHER and most[(37, 100)] <= ROWS_TOGETHER              # the walk goes round, and does not
    assert any(len(np.setdiff1d(np.arange(C), np.clip(case_inputs(c)[3], 0, C - 1))) for c in TABLE_CASES for C in [c[1]])   # absent classes
