"""Plain-11 (Barz & Denzler, "Deep Learning is not a Matter of Depth but of Good Training", ICPRAI 2018) as a PyTorch-ROCm module:
the reference's ``--architecture simple``, the default of every training command line.

Layer list and naming follow the reference's Keras model (reference: models/plainnet.py:5-78 -- ``PlainNet``): every integer of
``filters`` is a 3x3 'same' convolution with bias whose activation sits INSIDE the layer, followed by batch normalisation (so the
order is conv, activation, BN); ``'ap'`` / ``'mp'`` a 2x2 average / maximum pooling; ``'gap'`` the global average pooling, named
``avg_pool``; ``'fc<n>'`` a dense layer with the activation, then batch normalisation.  Layers are called ``conv<i>``, ``bn<i>``,
``ap<i>``, ``mp<i>`` and ``fc<i>`` with ``i`` the 1-based position in the list, and the final dense layer ``embedding`` (no
activation) or ``prob`` (softmax).

Keras semantics as in models/cifar_resnet.py: Glorot-uniform kernels (Keras' default), zero biases, batch normalisation with
eps = 1e-3 and momentum 0.99.  The L2 regulariser (5e-4) sits on every convolution and on the ``fc<n>`` kernels, NOT on the final
dense layer (models/plainnet.py:76 gives it none): ``regularized_parameters()`` yields exactly those.  The module runs in
channels_last memory format; MIOpen picks the convolution kernels.
"""
import torch
import torch.nn as nn

from .cifar_resnet import _ACT, KERAS_BN_EPS, KERAS_BN_MOMENTUM, keras_bn, keras_conv, keras_dense

PLAIN11 = (64, 64, 'ap', 128, 128, 128, 'ap', 256, 256, 256, 'ap', 512, 'gap', 'fc512')


def keras_bn1d(c):
    """``keras_bn`` behind a dense layer."""
    bn = nn.BatchNorm1d(c, eps=KERAS_BN_EPS, momentum=KERAS_BN_MOMENTUM)
    bn.register_buffer('num_batches_tracked', None)
    return bn


class PlainNet(nn.Module):
    """``PlainNet(output_dim, filters, activation, regularizer, final_activation, input_shape, pool_size, name)`` as in the
    reference (models/plainnet.py:5-12); ``input_channels`` overrides the last entry of ``input_shape``."""

    def __init__(self, output_dim, filters=PLAIN11, activation='relu', regularizer=5e-4, final_activation=None,
                 input_shape=(None, None, 3), pool_size=(2, 2), name=None, input_channels=None):
        super().__init__()
        if final_activation not in (None, 'softmax'):
            raise ValueError('final_activation must be None or "softmax"')
        self.name = name or 'plain-{}'.format(sum(1 for f in filters if isinstance(f, int) or str(f).startswith('fc')) + 1)
        self.regularizer = float(regularizer or 0.0)
        self.include_top = True
        self.top_activation = final_activation
        self.act = _ACT[activation]()
        prev = input_channels or input_shape[-1]
        self.plan = []                # (kind, layer name, batch-norm name) in forward order
        flattened = False
        for i, f in enumerate(filters, start=1):
            if f in ('ap', 'mp'):
                name_i = '{}{}'.format(f, i)
                setattr(self, name_i, (nn.AvgPool2d if f == 'ap' else nn.MaxPool2d)(tuple(pool_size)))
                self.plan.append(('pool', name_i, None))
            elif f == 'gap':
                self.num_features = prev
                self.avg_pool = nn.Identity()      # named tap on the pooled features (--cls_base avg_pool), as in SmallResNet
                self.plan.append(('gap', 'avg_pool', None))
                flattened = True
            elif isinstance(f, str) and f.startswith('fc'):
                if not flattened:
                    raise NotImplementedError('a dense layer in front of "gap" needs a fixed input size (Flatten): not supported')
                setattr(self, 'fc{}'.format(i), keras_dense(prev, int(f[2:])))
                setattr(self, 'bn{}'.format(i), keras_bn1d(int(f[2:])))
                self.plan.append(('fc', 'fc{}'.format(i), 'bn{}'.format(i)))
                prev = int(f[2:])
            else:
                if flattened:
                    raise ValueError('a convolution cannot follow "gap"')
                setattr(self, 'conv{}'.format(i), keras_conv(prev, int(f), 3))
                setattr(self, 'bn{}'.format(i), keras_bn(int(f)))
                self.plan.append(('conv', 'conv{}'.format(i), 'bn{}'.format(i)))
                prev = int(f)
        if not flattened:
            raise NotImplementedError('a layer list without "gap" needs a fixed input size (Flatten): not supported')
        head = keras_dense(prev, output_dim)
        if final_activation is None:
            self.embedding = head
        else:
            self.prob = head
        self.to(memory_format=torch.channels_last)

    @property
    def head(self):
        return getattr(self, 'embedding', None) or getattr(self, 'prob', None)

    def features(self, x):
        """Everything in front of the final dense layer."""
        for kind, layer, bn in self.plan:
            if kind == 'gap':
                x = self.avg_pool(x.mean(dim=(2, 3)))
            elif kind == 'pool':
                x = getattr(self, layer)(x)
            else:
                x = getattr(self, bn)(self.act(getattr(self, layer)(x)))
        return x

    def forward(self, x):
        x = self.head(self.features(x))
        if self.top_activation == 'softmax':
            x = torch.softmax(x.float(), dim=-1)
        return x

    def regularized_parameters(self):
        """Kernels carrying the Keras L2 regulariser: every convolution and ``fc<n>`` layer, not the final dense layer."""
        for kind, layer, _ in self.plan:
            if kind in ('conv', 'fc'):
                yield getattr(self, layer).weight
