"""CPU: the Plain-11 (`simple`) and PyramidNet backbones behind utils.build_network -- shapes, heads, layer lists, parameter counts,
regularisers, the PyramidNet width rule -- and that every training / evaluation command line starts with its default architecture."""
import pytest
import torch
import torch.nn as nn

NEW = ["simple", "pyramidnet-272-200", "pyramidnet-110-270"]
PLAIN11 = [64, 64, 'ap', 128, 128, 128, 'ap', 256, 256, 256, 'ap', 512, 'gap', 'fc512']


@pytest.fixture(scope="module")
def batch():
    return torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(0))


@pytest.fixture(scope="module")
def nets():
    """One instance of every new architecture, shared by the read-only tests."""
    import utils
    torch.manual_seed(1)
    return {name: utils.build_network(100, name).eval() for name in NEW}


@pytest.mark.parametrize("name", NEW)
def test_embedding_head_and_output_shape(nets, batch, name):
    import utils
    assert name in utils.IMPLEMENTED_ARCHITECTURES and name in utils.ARCHITECTURES
    net = nets[name]
    with torch.no_grad():
        out = net(batch)
    assert out.shape == (2, 100) and torch.isfinite(out).all()
    assert isinstance(net.embedding, nn.Linear) and not hasattr(net, "prob") and net.head is net.embedding
    assert net.embedding.in_features == net.num_features
    assert isinstance(net.avg_pool, nn.Module)                    # the named tap of --cls_base avg_pool
    assert all(m.weight.is_contiguous(memory_format=torch.channels_last) for m in net.modules() if isinstance(m, nn.Conv2d))


@pytest.mark.parametrize("name", ["simple", "pyramidnet-110-270"])
def test_classification_heads(batch, name):
    import utils
    net = utils.build_network(10, name, classification=True).eval()
    assert isinstance(net.prob, nn.Linear) and not hasattr(net, "embedding")
    with torch.no_grad():
        p = net(batch)
    assert p.shape == (2, 10) and (p >= 0).all() and torch.allclose(p.sum(-1), torch.ones(2), atol=1e-5)
    logits_net = utils.build_network(10, name, classification=True, no_softmax=True).eval()
    assert isinstance(logits_net.embedding, nn.Linear)            # no activation: the head is called `embedding`
    with torch.no_grad():
        for q, p_ in zip(logits_net.parameters(), net.parameters()):
            q.copy_(p_)
    with torch.no_grad():
        z = logits_net(batch)
    assert not torch.allclose(z.sum(-1), torch.ones(2), atol=1e-3) and torch.allclose(torch.softmax(z, -1), p, atol=1e-6)


@pytest.mark.parametrize("name", ["simple", "pyramidnet-110-270"])
def test_input_channels_and_selu(name):
    import utils
    net = utils.build_network(7, name + "-selu", input_channels=1).eval()
    assert any(isinstance(m, nn.SELU) for m in net.modules()) and not any(isinstance(m, nn.ReLU) for m in net.modules())
    first = net.conv1 if name == "simple" else net.conv0
    assert first.in_channels == 1
    with torch.no_grad():
        assert net(torch.randn(2, 1, 16, 16)).shape == (2, 7)
    assert any(isinstance(m, nn.ReLU) for m in utils.build_network(7, name).modules())


def test_plainnet_layer_list_and_parameter_count(nets):
    net = nets["simple"]
    want, cin = 0, 3
    names = []
    for i, f in enumerate(PLAIN11, start=1):
        if isinstance(f, int):
            want += cin * f * 9 + f + 2 * f                      # kernel, bias, BN gamma and beta
            names += ["conv%d" % i, "bn%d" % i]
            cin = f
        elif f == 'ap':
            names.append("ap%d" % i)
        elif f == 'gap':
            names.append("avg_pool")
        else:
            width = int(f[2:])
            want += cin * width + width + 2 * width
            names += ["fc%d" % i, "bn%d" % i]
            cin = width
    want += cin * 100 + 100
    assert sum(p.numel() for p in net.parameters() if p.requires_grad) == want == 3381796
    have = [n for n, _ in net.named_children() if n != "act"]
    assert have == names + ["embedding"]
    assert net.name == "plain-11" and net.num_features == 512
    # conv, activation, BN: the activation sits in front of the batch normalisation
    seen = []
    hooks = [m.register_forward_hook(lambda mod, i, o, n=n: seen.append(n)) for n, m in net.named_children()]
    with torch.no_grad():
        net(torch.randn(1, 3, 8, 8))
    for h in hooks:
        h.remove()
    assert seen[:3] == ["conv1", "act", "bn1"] and seen[-4:] == ["fc14", "act", "bn14", "embedding"]
    assert isinstance(net.ap3, nn.AvgPool2d) and net.ap3.kernel_size == (2, 2)
    assert net.conv1.bias is not None and net.conv1.padding == (1, 1) and net.bn1.eps == 1e-3 and abs(net.bn1.momentum - 0.01) < 1e-12


def test_plainnet_regulariser_leaves_the_final_dense_layer_out(nets):
    net = nets["simple"]
    assert net.regularizer == 5e-4
    reg = list(net.regularized_parameters())
    convs = [m.weight for m in net.modules() if isinstance(m, nn.Conv2d)]
    assert len(convs) == 9 and len(reg) == 10
    assert all(any(r is w for r in reg) for w in convs + [net.fc14.weight])
    assert not any(r is net.embedding.weight for r in reg)
    assert not any(r.dim() == 1 for r in reg)                     # no bias, no BN


def running_sum_widths(depth, alpha, bottleneck):
    """The reference's rule, restated: start += alpha / (3 n) in front of every block, width = round(start)."""
    n = (depth - 2) // 9 if bottleneck else (depth - 2) // 6
    start, add, widths = 16, float(alpha) / (3 * n), []
    for _ in range(3 * n):
        start += add
        widths.append(round(start))
    return n, widths


@pytest.mark.parametrize("name,depth,alpha,bottleneck,last", [("pyramidnet-272-200", 272, 200, True, 216),
                                                              ("pyramidnet-110-270", 110, 270, False, 286)])
def test_pyramidnet_widths_strides_and_layers(nets, name, depth, alpha, bottleneck, last):
    net = nets[name]
    n, widths = running_sum_widths(depth, alpha, bottleneck)
    blocks = list(net.blocks)
    assert len(blocks) == 3 * n == (90 if bottleneck else 54)
    assert [b.width for b in blocks] == widths and widths[-1] == last
    assert net.num_features == (4 * last if bottleneck else last) == net.embedding.in_features
    assert [k for k, b in enumerate(blocks) if b.stride == 2] == [n, 2 * n]
    cin = 16
    for b in blocks:
        convs = [m for m in b.children() if isinstance(m, nn.Conv2d)]
        kinds = [type(m).__name__ for m in b.children()]
        if bottleneck:
            assert kinds == ["BatchNorm2d", "Conv2d", "BatchNorm2d", "ReLU", "Conv2d", "BatchNorm2d", "ReLU", "Conv2d", "BatchNorm2d"]
            assert [c.kernel_size for c in convs] == [(1, 1), (3, 3), (1, 1)]
            assert [c.stride for c in convs] == [(1, 1), (b.stride, b.stride), (1, 1)]         # the stride sits on the 3x3
            assert [(c.in_channels, c.out_channels) for c in convs] == [(cin, b.width), (b.width, b.width), (b.width, 4 * b.width)]
        else:
            assert kinds == ["BatchNorm2d", "Conv2d", "BatchNorm2d", "ReLU", "Conv2d", "BatchNorm2d"]
            assert [c.stride for c in convs] == [(b.stride, b.stride), (1, 1)]
            assert [(c.in_channels, c.out_channels) for c in convs] == [(cin, b.width), (b.width, b.width)]
        assert all(c.bias is not None for c in convs)
        assert kinds[-1] == "BatchNorm2d"                          # nothing behind the last BN but the add: no activation after it
        assert b.pad == b.out_channels - cin >= 0
        cin = b.out_channels
    assert net.regularizer == 2e-4
    reg = list(net.regularized_parameters())
    assert len(reg) == 1 + sum(3 if bottleneck else 2 for _ in blocks) + 1 and any(r is net.embedding.weight for r in reg)
    assert net.conv0.out_channels == 16 and net.bn0.num_features == 16 and net.name == name


def test_pyramidnet_block_output_is_the_sum_without_activation():
    """A block's output is residual + padded, pooled input: negative values survive (no activation after the add), the appended
    channels come last (pad_before = 0), and a strided block pools its shortcut."""
    from models.cifar_pyramidnet import PyramidBlock
    torch.manual_seed(3)
    for bottleneck in (True, False):
        blk = PyramidBlock(6, 9, stride=2, bottleneck=bottleneck).eval()
        x = torch.randn(2, 6, 8, 8)
        with torch.no_grad():
            out = blk(x)
            s = x
            for name in blk.residual:
                s = getattr(blk, name)(s)
        assert out.shape == (2, blk.out_channels, 4, 4) and (out < 0).any()
        pooled = x.reshape(2, 6, 4, 2, 4, 2).mean(dim=(3, 5))
        assert torch.allclose(out[:, :6], s[:, :6] + pooled, atol=1e-6)
        assert torch.equal(out[:, 6:], s[:, 6:])


def test_fused_flag_and_cpu_path_agree_exactly():
    """On CPU tensors the fused flag changes nothing: both take the torch composition."""
    from models.cifar_pyramidnet import PyramidNet
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(4))
    outs = []
    for fused in (True, False):
        torch.manual_seed(5)
        net = PyramidNet(20, 12, bottleneck=True, top_activation=None, classes=10, fused_shortcut=fused)
        assert net.fused_shortcut is fused and all(b.fused_shortcut is fused for b in net.blocks)
        assert net.widths == [18, 20, 22, 24, 26, 28]
        out = net(x)
        out.square().sum().backward()
        outs.append((out.detach(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert PyramidNet(20, 12).fused_shortcut is False              # the default: the measurement did not favour the kernel


REQUIRED = {"learn_image_embeddings": ["--embedding", "e.pickle"], "learn_devise": ["--embedding", "e.pickle"],
            "evaluate_classification_accuracy": ["--model", "m.pt", "--layer", "prob"]}


@pytest.mark.parametrize("cli", ["learn_image_embeddings", "learn_classifier", "learn_center_loss", "learn_devise", "learn_labelembedding",
                                 "evaluate_classification_accuracy"])
def test_every_command_line_starts_with_its_default_architecture(cli):
    """All six parsers default to the reference's `simple`; a command line without --architecture must reach a network."""
    import utils
    mod = __import__(cli)
    args = mod.build_parser().parse_args(["--dataset", "CIFAR-100", "--data_root", "-"] + REQUIRED.get(cli, []))
    assert args.architecture == "simple"
    net = utils.build_network(100, args.architecture)
    assert isinstance(net, nn.Module) and net.name == "plain-11"


def test_backbone_mode_groups_the_pyramidnets_with_the_cifar_nets():
    import engine
    for name in NEW + ["resnet-110-fc"]:
        assert engine.backbone_mode(name) == (None, torch.contiguous_format)
    assert engine.backbone_mode("resnet-50") == (torch.bfloat16, torch.channels_last)


def test_other_architectures_keep_raising():
    import utils
    for name in ("wrn-28-10", "densenet-100-12", "rn18", "nasnet-a", "resnet-101"):
        with pytest.raises(NotImplementedError):
            utils.build_network(10, name)
    with pytest.raises(ValueError):
        utils.build_network(10, "no-such-net")
