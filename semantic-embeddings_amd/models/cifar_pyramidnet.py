"""PyramidNet for CIFAR (Han et al., "Deep Pyramidal Residual Networks") as a PyTorch-ROCm module.

Architecture and the named layers follow the reference's Keras model (reference: models/cifar_pyramidnet.py:31-191 --
``PyramidNet``): a 3x3 stem ``conv0`` to 16 channels with ``bn0`` and NO activation, three stages of ``n`` blocks whose width grows
by ``alpha / (3 n)`` per block, ``bn4``, ``act4``, the global average pooling ``avg_pool`` and a dense layer called ``embedding`` (no
activation) or ``prob`` (softmax).

* Widths are the reference's running sum (:149-154): ``start += alpha / (3 n)`` in front of every block, width = Python's
  ``round(start)`` -- accumulated in a Python float, because a closed form ``16 + k * add`` can land on the other side of a half.
* The first block of stages 2 and 3 has stride 2, on its 3x3 convolution.
* Basic block (:90-97): BN, conv3x3(stride), BN, act, conv3x3, BN.  Bottleneck block (:100-110): BN, conv1x1, BN, act,
  conv3x3(stride), BN, act, conv1x1 to 4 n, BN.  Neither has an activation after the add.
* The shortcut (:81-87) is an average pooling by ``stride`` when ``stride > 1``, then zero channels appended at the END
  (``ChannelPadding((0, n - c_in))``; ``SmallResNet`` pads both sides).  With ``fused_shortcut`` the pooling, the padding and the add
  are one HIP launch (``sehip.shortcut_add``); otherwise, and on CPU tensors, the torch composition avg_pool2d + pad + add.  The
  default is the composition: measured at PyramidNet-272-200's shapes the kernel wins at the 32 x 32 stage and at the strided blocks
  but loses at the stride-1 blocks of the smaller stages, a loss over the whole network (profiles/shortcut_add_bench.txt).

Keras semantics: every convolution has a bias, Glorot-NORMAL weights (a normal distribution of standard deviation
sqrt(2 / (fan_in + fan_out)), truncated at two standard deviations) and the L2 regulariser 2e-4; the dense layer is Glorot-uniform
with the same regulariser; batch normalisation uses eps = 1e-3 and momentum 0.99.  The blocks' inner layers carry no names in the
reference (Keras numbers them); here they are ``bn1, conv1, bn2, conv2, ...`` inside ``blocks.<k>``.  channels_last memory format.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import sehip

from .cifar_resnet import _ACT, keras_bn, keras_conv, keras_dense


def _glorot_normal_(weight):
    """Keras' ``glorot_normal``: N(0, 2 / (fan_in + fan_out)) truncated at two standard deviations."""
    rf = weight.shape[2] * weight.shape[3]
    std = math.sqrt(2.0 / ((weight.shape[1] + weight.shape[0]) * rf))
    with torch.no_grad():
        nn.init.trunc_normal_(weight, mean=0.0, std=std, a=-2.0 * std, b=2.0 * std)


def _conv(cin, cout, k, stride=1):
    conv = keras_conv(cin, cout, k, stride)
    _glorot_normal_(conv.weight)
    return conv


def block_widths(depth, alpha, bottleneck=True):
    """``(n, [width of every block])``: the reference's running sum (models/cifar_pyramidnet.py:121-124, 149-154)."""
    n = (depth - 2) // 9 if bottleneck else (depth - 2) // 6
    start_channel, add_channel = 16, float(alpha) / (3 * n)
    widths = []
    for _ in range(3 * n):
        start_channel += add_channel
        widths.append(round(start_channel))
    return n, widths


class PyramidBlock(nn.Module):
    """One basic or bottleneck block: ``cin`` channels in, ``out_channels`` = ``width`` (basic) or ``4 * width`` (bottleneck) out."""

    def __init__(self, cin, width, stride=1, bottleneck=True, activation='relu', fused_shortcut=False):
        super().__init__()
        self.stride, self.width, self.fused_shortcut = stride, width, fused_shortcut
        self.out_channels = 4 * width if bottleneck else width
        if cin > self.out_channels:
            raise ValueError('a pyramidal shortcut cannot drop channels ({} -> {})'.format(cin, self.out_channels))
        self.pad = self.out_channels - cin
        act = _ACT[activation]
        if bottleneck:
            layers = [('bn1', keras_bn(cin)), ('conv1', _conv(cin, width, 1)), ('bn2', keras_bn(width)), ('act2', act()),
                      ('conv2', _conv(width, width, 3, stride)), ('bn3', keras_bn(width)), ('act3', act()),
                      ('conv3', _conv(width, 4 * width, 1)), ('bn4', keras_bn(4 * width))]
        else:
            layers = [('bn1', keras_bn(cin)), ('conv1', _conv(cin, width, 3, stride)), ('bn2', keras_bn(width)), ('act2', act()),
                      ('conv2', _conv(width, width, 3)), ('bn3', keras_bn(width))]
        for name, layer in layers:
            self.add_module(name, layer)
        self.residual = [name for name, _ in layers]

    def forward(self, x):
        s = x
        for name in self.residual:
            s = getattr(self, name)(s)
        if self.fused_shortcut and s.is_cuda:
            # one launch; the kernel wants both operands in one dense layout and dtype (the stem's output can differ from a block's)
            fmt = torch.contiguous_format if s.is_contiguous() else torch.channels_last
            return sehip.shortcut_add(s.contiguous(memory_format=fmt), x.to(s.dtype).contiguous(memory_format=fmt), self.stride, 0)
        sc = F.avg_pool2d(x, self.stride) if self.stride > 1 else x
        if self.pad:
            sc = F.pad(sc, (0, 0, 0, 0, 0, self.pad))
        return s + sc


class PyramidNet(nn.Module):
    """``PyramidNet(depth, alpha, bottleneck, include_top, ..., classes, name)`` as in the reference
    (models/cifar_pyramidnet.py:31-36); ``fused_shortcut`` chooses the HIP shortcut kernel (device tensors only)."""

    def __init__(self, depth, alpha, bottleneck=True, include_top=True, weights=None, input_tensor=None, input_shape=None,
                 pooling='avg', regularizer=2e-4, activation='relu', top_activation='softmax', classes=100, name=None,
                 input_channels=None, fused_shortcut=False):
        super().__init__()
        if weights is not None:
            raise NotImplementedError("loading Keras .h5 weights is not supported (no h5py); use torch state_dicts")
        cin = input_channels or (input_shape[-1] if input_shape else 3)
        self.name = name or 'pyramidnet-{}-{}'.format(depth, alpha)
        self.regularizer = float(regularizer or 0.0)
        self.include_top = include_top
        self.pooling = pooling
        self.top_activation = top_activation
        self.fused_shortcut = fused_shortcut
        self.conv0 = _conv(cin, 16, 3)
        self.bn0 = keras_bn(16)
        n, self.widths = block_widths(depth, alpha, bottleneck)
        blocks, prev = [], 16
        for k, width in enumerate(self.widths):
            stride = 2 if (k >= n and k % n == 0) else 1
            blocks.append(PyramidBlock(prev, width, stride, bottleneck, activation, fused_shortcut))
            prev = blocks[-1].out_channels
        self.blocks = nn.Sequential(*blocks)
        self.bn4 = keras_bn(prev)
        self.act4 = _ACT[activation]()
        self.num_features = prev
        self.avg_pool = nn.Identity()      # named tap on the pooled features (--cls_base avg_pool), as in SmallResNet
        if include_top:
            head = keras_dense(prev, classes)
            if top_activation is None:
                self.embedding = head
            else:
                self.prob = head
        self.to(memory_format=torch.channels_last)

    @property
    def head(self):
        return getattr(self, 'embedding', None) or getattr(self, 'prob', None)

    def features(self, x):
        x = self.bn0(self.conv0(x))
        x = self.act4(self.bn4(self.blocks(x)))
        if self.pooling == 'avg':
            x = self.avg_pool(x.mean(dim=(2, 3)))
        elif self.pooling == 'max':
            x = x.amax(dim=(2, 3))
        return x

    def forward(self, x):
        x = self.features(x)
        if self.include_top:
            x = self.head(x)
            if self.top_activation == 'softmax':
                x = torch.softmax(x.float(), dim=-1)
        return x

    def regularized_parameters(self):
        """Kernels carrying the Keras L2 regulariser (conv + dense kernels; not biases, not BN)."""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                yield m.weight
