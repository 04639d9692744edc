"""CPU: the float32 NumPy oracle of se_adagrad_step (the four lines of include/sehip.h) against the same formula in float64, the entry
point's host-side argument checks, learn_devise.py's command line against the flag names and defaults of the reference's parser,
its transform_inputs / decay formula / embedding loader, and the trainer's optimizer argument."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

U = 2.0 ** -24
F = np.float32


def adagrad_oracle(p, a, g, l2, lr, grad_scale=1.0, epsilon=1e-7):
    """(p', a') of one se_adagrad_step in float32: every NumPy operation below rounds once, sqrt and / are correctly rounded.
    l2 None: no regulariser."""
    p, a, g = (np.asarray(v, dtype=F) for v in (p, a, g))
    with np.errstate(all="ignore"):
        g1 = g if F(grad_scale) == F(1) else g * F(grad_scale)
        g2 = g1 if l2 is None else g1 + np.asarray(l2, dtype=F) * p
        a2 = a + g2 * g2
        p2 = p - (F(lr) * g2) / (np.sqrt(a2) + F(epsilon))
    assert p2.dtype == F and a2.dtype == F
    return p2, a2


def adagrad_float64(p, a, g, l2, lr, grad_scale=1.0, epsilon=1e-7):
    """The same formula on the same float32 inputs (and float32 lr, grad_scale, epsilon) in float64: (step, a'), p' = p - step."""
    p, a, g = (np.asarray(v, dtype=F).astype(np.float64) for v in (p, a, g))
    g2 = g * np.float64(F(grad_scale))
    if l2 is not None:
        g2 = g2 + np.asarray(l2, dtype=F).astype(np.float64) * p
    a2 = a + g2 * g2
    return np.float64(F(lr)) * g2 / (np.sqrt(a2) + np.float64(F(epsilon))), a2


def adagrad_inputs(n, seed, with_l2=True):
    """|g| in [1e-6, 1e2], |p| in [1e-3, 10], both signs, log-uniform; accum zero; l2 = 2 lambda with lambda in {0, 2e-4, 5e-4}.  Every
    intermediate of the update is then a normal float32 or exactly 0."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice(np.array([-1.0, 1.0]), size=n)
    g = (sign() * 10.0 ** rng.uniform(-6, 2, size=n)).astype(F)
    p = (sign() * 10.0 ** rng.uniform(-3, 1, size=n)).astype(F)
    l2 = (2.0 * rng.choice(np.array([0.0, 2e-4, 5e-4]), size=n)).astype(F) if with_l2 else None
    return p, np.zeros(n, dtype=F), g, l2


# ---------------------------------------------------------------- the oracle against float64

def test_oracle_agrees_with_float64_within_its_roundings():
    """Without regulariser and scale the step takes 6 roundings (g^2, a + ., sqrt, + epsilon, lr g, /), of which sqrt halves what it is
    given: at most 5 u relative, held to 8 u = 8 * 2^-24.  With p = 0 the update p - p' IS the step (0 - s is exact)."""
    _, _, g, _ = adagrad_inputs(20000, 1, with_l2=False)
    p = np.zeros_like(g)
    a = np.zeros_like(g)
    for it in range(3):                          # the accumulator carries
        p2, a2 = adagrad_oracle(p, a, g, None, 0.01)
        step, a64 = adagrad_float64(p, a, g, None, 0.01)
        upd = (p.astype(np.float64) - p2.astype(np.float64))
        assert np.all(np.abs(upd - step) <= 8 * U * np.abs(step)), it
        assert np.all(np.abs(a2 - a64) <= 2 * U * a64)
        assert np.all(np.sign(upd) == np.sign(g))
        a = a2                                   # p stays 0: the bound is on the step alone
    # with scale and regulariser, g and l2 * p of one sign (no cancellation in g2): g2 carries 3 u, lr g2 4 u, g2^2 7 u, a' 8 u,
    # sqrt 5 u, + epsilon 6 u, the quotient 11 u; the final subtraction adds u |p'|
    p, a, g, l2 = adagrad_inputs(20000, 2)
    p, g = np.abs(p), np.abs(g)
    p2, a2 = adagrad_oracle(p, a, g, l2, 0.01, 0.5)
    step, _ = adagrad_float64(p, a, g, l2, 0.01, 0.5)
    want = p.astype(np.float64) - step
    assert np.all(np.abs(p2 - want) <= 12 * U * np.abs(step) + U * np.abs(want))


def test_oracle_on_zeros_and_non_finite_values():
    z = np.zeros(4, dtype=F)
    p2, a2 = adagrad_oracle(z, z, z, z + F(4e-4), 0.01)
    assert not p2.view(np.int32).any() and not a2.view(np.int32).any()            # +0 everywhere, bitwise
    p = np.array([1.5, -2.0, 0.25], dtype=F)
    a = np.array([0.5, 2.0, 1e-3], dtype=F)
    p2, a2 = adagrad_oracle(p, a, np.zeros(3, dtype=F), None, 0.01)
    assert np.array_equal(p2.view(np.int32), p.view(np.int32)) and np.array_equal(a2.view(np.int32), a.view(np.int32))
    g = np.array([np.nan, np.inf, -np.inf, 1.0], dtype=F)
    p2, a2 = adagrad_oracle(np.ones(4, dtype=F), np.ones(4, dtype=F), g, None, 0.01)
    assert np.isnan(p2).tolist() == [True, True, True, False]                     # inf / inf
    assert np.isnan(a2).tolist() == [True, False, False, False] and np.isinf(a2).tolist() == [False, True, True, False]


# ---------------------------------------------------------------- the C ABI without a device

def test_entry_point_checks_its_arguments_without_a_gpu():
    import sehip
    lib = sehip.lib()
    assert "se_adagrad_step" in sehip.EXPORTS and hasattr(lib, "se_adagrad_step")
    assert sehip.ADAGRAD_MAX_BLOCKS == sehip.ops.DEFINES["SE_ADAGRAD_MAX_BLOCKS"] > 0
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def step(p=one, accum=one, g=one, l2=z, n=5, lr=0.01, lr_dev=z, scale=1.0, eps=1e-7):
        return lib.se_adagrad_step(p, accum, g, l2, n, lr, lr_dev, scale, eps, z)

    for kw in (dict(p=z), dict(accum=z), dict(g=z)):
        assert step(**kw) == -1 and b"se_adagrad_step: null pointer" in lib.se_last_error(), kw
    assert step(n=-1) == -1 and b"se_adagrad_step" in lib.se_last_error()
    assert step(eps=-1e-7) == -1 and b"se_adagrad_step" in lib.se_last_error() and b"epsilon" in lib.se_last_error()
    assert step(n=0) == 0 and step(p=z, accum=z, g=z, n=0) == 0                   # nothing to do: no launch, no device needed


def test_adagrad_step_refuses_host_tensors():
    import sehip
    t = torch.zeros(8)
    with pytest.raises(sehip.SehipError):
        sehip.adagrad_step_(t, t.clone(), t.clone(), lr=0.01)
    assert "adagrad_step_" in sehip.ops.__all__


# ---------------------------------------------------------------- the command line

# learn_devise.py:25-48 of the reference: flag -> (group, default or REQUIRED)
REQUIRED = object()
REFERENCE_FLAGS = {
    "dataset": ("Data parameters", REQUIRED), "data_root": ("Data parameters", REQUIRED), "embedding": ("Data parameters", REQUIRED),
    "architecture": ("Training parameters", "simple"), "init_weights": ("Training parameters", None),
    "init_epochs": ("Training parameters", 25), "ft_epochs": ("Training parameters", 75), "init_lr": ("Training parameters", 0.01),
    "ft_lr": ("Training parameters", 0.001), "batch_size": ("Training parameters", 100), "val_batch_size": ("Training parameters", None),
    "max_decay": ("Training parameters", 0.0), "margin": ("Training parameters", 0.1), "read_workers": ("Training parameters", 8),
    "queue_size": ("Training parameters", 100),
    "model_dump": ("Output parameters", None), "weight_dump": ("Output parameters", None), "feature_dump": ("Output parameters", None),
    "log_dir": ("Output parameters", None), "no_progress": ("Output parameters", False),
}


def test_parser_has_the_reference_flags_and_defaults():
    import learn_devise as ld
    import utils
    p = ld.build_parser()
    groups = {a.dest: g.title for g in p._action_groups for a in g._group_actions}
    acts = {a.dest: a for a in p._actions if a.dest != "help"}
    assert sorted(acts) == sorted(list(REFERENCE_FLAGS) + ["gpus"])               # --gpus: the one extension
    assert groups["gpus"] == "Training parameters" and acts["gpus"].default == 1 and not acts["gpus"].required
    args = p.parse_args(["--dataset", "d", "--data_root", "r", "--embedding", "e"])
    for name, (group, default) in REFERENCE_FLAGS.items():
        assert groups[name] == group, name
        assert acts[name].required == (default is REQUIRED), name
        if default is not REQUIRED:
            assert getattr(args, name) == default and type(getattr(args, name)) is type(default), name
    assert acts["architecture"].choices == utils.ARCHITECTURES
    assert [g.title for g in p._action_groups][2:] == ["Data parameters", "Training parameters", "Output parameters"]
    for missing in ("--dataset", "--data_root", "--embedding"):
        argv = [w for k in ("--dataset", "--data_root", "--embedding") if k != missing for w in (k, "x")]
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    a = p.parse_args(["--dataset", "d", "--data_root", "r", "--embedding", "e", "--init_weights", "w.pt", "--init_epochs", "2",
                      "--ft_epochs", "3", "--init_lr", "0.1", "--ft_lr", "0.05", "--max_decay", "0.1", "--margin", "0.2", "--no_progress",
                      "--read_workers", "1", "--queue_size", "2", "--gpus", "8", "--architecture", "resnet-110-fc"])
    assert (a.init_weights, a.init_epochs, a.ft_epochs, a.init_lr, a.ft_lr, a.max_decay, a.margin, a.no_progress, a.gpus) == \
        ("w.pt", 2, 3, 0.1, 0.05, 0.1, 0.2, True, 8)


def test_transform_inputs_and_decay_formula():
    import learn_devise as ld
    import train_cli
    emb = np.eye(3, dtype=np.float32)
    X, y = ld.transform_inputs("X", "y", emb)
    assert X == "X" and y == "y"                                                  # the labels travel; the kernels gather
    assert ld.transform_inputs("X", "y", embedding=emb) == ("X", "y")
    # learn_devise.py:109-112: decay = (1 / max_decay - 1) / ((num_train // batch_size) * ft_epochs), 0 without --max_decay
    assert train_cli.max_decay_rate(0.0, 50000, 100, 75) == 0.0
    assert train_cli.max_decay_rate(0.1, 192, 32, 2) == (1.0 / 0.1 - 1) / ((192 // 32) * 2)
    assert train_cli.max_decay_rate(0.5, 50050, 100, 75) == (1.0 / 0.5 - 1) / (500 * 75)
    d = train_cli.max_decay_rate(0.1, 192, 32, 2)
    assert abs(1.0 / (1.0 + d * 12) - 0.1) < 1e-12                                # lr reaches max_decay * lr after the last step
    losses, metrics = ld.build_losses(torch.eye(3), 0.1)
    assert list(losses) == ["embedding"] and losses["embedding"][1] == 1.0
    assert [m.name for m in metrics["embedding"]] == ["max_sim_acc"]


def test_embedding_loader_normalises_rows_and_hands_on_the_labels(tmp_path):
    import learn_devise as ld
    rng = np.random.default_rng(0)
    E = rng.standard_normal((7, 5)) * 3.0                                          # float64, unnormalised, like the pickles on disk
    labels = [3, 1, 4, 15, 9, 2, 6]
    path = tmp_path / "emb.pickle"
    with open(path, "wb") as f:
        pickle.dump({"ind2label": labels, "label2ind": {l: i for i, l in enumerate(labels)}, "embedding": E}, f)
    ind2label, emb = ld.load_embedding(str(path))
    assert ind2label == labels
    assert emb.dtype == np.float32 and emb.shape == (7, 5)
    assert np.allclose(np.linalg.norm(emb.astype(np.float64), axis=-1), 1.0, atol=1e-6)
    assert np.allclose(emb, E / np.linalg.norm(E, axis=-1, keepdims=True), atol=1e-6)
    from datasets import get_data_generator
    gen = get_data_generator("synthetic:100x32x64x32", "-", classes=ind2label)
    assert gen.classes == labels and gen.num_classes == 7


def test_embedding_layer_is_found_or_appended():
    import learn_devise as ld
    import utils
    torch.manual_seed(0)
    fc = utils.build_network(24, "resnet-110-fc", input_channels=3)
    assert ld.embedding_layer(fc, 24) is fc.embedding
    bare = utils.build_network(64, "resnet-32", input_channels=3)                  # ends in its 64 pooled features
    assert getattr(bare, "embedding", None) is None
    head = ld.embedding_layer(bare, 10)
    assert head is bare.embedding and (head.in_features, head.out_features) == (64, 10)
    assert {"embedding.weight", "embedding.bias"} <= set(bare.state_dict())
    bare.eval()
    with torch.no_grad():
        assert bare(torch.randn(2, 3, 32, 32)).shape == (2, 10)


def test_init_weights_takes_a_state_dict_or_a_whole_model(tmp_path, capsys):
    """What --init_weights loads: tensors that match by name and shape, from a --weight_dump or a --model_dump of the classifier; its
    ``prob`` layer stays behind and ``embedding`` keeps its fresh values."""
    import learn_classifier as lc
    import train_cli
    import utils
    torch.manual_seed(0)
    clf = lc.build_classifier(100, "resnet-110-fc", input_channels=3)
    torch.save(clf.state_dict(), str(tmp_path / "w.pt"))
    torch.save(clf, str(tmp_path / "m.pt"))
    for name in ("w.pt", "m.pt"):
        net = utils.build_network(24, "resnet-110-fc", input_channels=3)
        fresh = {k: v.clone() for k, v in net.embedding.state_dict().items()}
        train_cli.load_pretrained(net, str(tmp_path / name), torch.device("cpu"))
        own, src = net.state_dict(), clf.state_dict()
        assert not any(k.startswith("prob.") for k in own)
        for k, v in own.items():
            if k.startswith("embedding."):
                assert torch.equal(v, fresh[k[len("embedding."):]]), k
            else:
                assert torch.equal(v, src[k]), k
    assert capsys.readouterr().out.count("Loading pre-trained weights") == 2


# ---------------------------------------------------------------- the trainer's optimizer argument

def test_trainer_optimizer_argument():
    from engine import Trainer
    net = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="optimizer"):
        Trainer(net, {}, optimizer="bogus", autocast_dtype=None)
    assert Trainer(net, {}, autocast_dtype=None).optimizer == "sgd"
    tr = Trainer(torch.nn.Linear(3, 2), {}, optimizer="adagrad", autocast_dtype=None)
    assert tr.optimizer == "adagrad" and tr.epsilon == 1e-7 and not tr.flat.flat_v.any()
