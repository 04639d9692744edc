"""Drop-in for the reference's ``learn_labelembedding.py``: trains the label-embedding baseline of Sun et al. ("Label Embedding
Network: Learning Label Representation for Soft Training of Deep Networks"), same command line (reference:
learn_labelembedding.py:65-208 + utils.py:402-418), on MI355X.

    python learn_labelembedding.py --dataset synthetic-cifar100 --data_root . --architecture resnet-110-fc --batch_size 128 \
        --feature_dump labelembed_features.pickle
    # data parallel, one process per GPU over RCCL (instead of keras.utils.multi_gpu_model)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 learn_labelembedding.py ... --gpus 8

The loss, its gradients and the gradient of the learned ``[C, C]`` label-embedding table run on the HIP kernels
(``sehip.labelembed_table_loss``): the kernels read the table row of every sample in place, and the table's gradient is a
fixed-order per-class reduction, so a step gives the same bits whenever its inputs are the same.  ``cross_entropy``,
``labelembed_loss``, ``labelembed_model`` and ``transform_inputs`` keep the reference's signatures (learn_labelembedding.py:17-61).

Differences from the reference a user can observe: ``--gpus N`` expects to be launched with N processes (torchrun); ``--batch_size``
stays the GLOBAL batch and is split across the ranks like ``multi_gpu_model`` split it across towers -- the loss's batch-wide
factor ``B / (sum mask + 1e-8)`` is taken over each rank's own sub-batch, as it is over each tower's in the reference; models and
weights are torch ``state_dict`` / ``torch.save`` files, not Keras ``.h5``; ``--read_workers`` / ``--queue_size``
set the decode threads (at most 16) and the batches of look-ahead (at most 4) of a dataset that streams its images (``-stream`` names)
and are ignored otherwise (batches are composed on the device); ``--gpu_merge`` is accepted and ignored (weights always live on the GPUs); ``--log_dir`` writes a JSON-lines
log instead of TensorBoard events.
"""
import argparse

import numpy as np
import torch

import train_cli
import utils
from datasets import get_data_generator

# with the backbone's last layer: what --finetune_init trains first (learn_labelembedding.py:142-144; `embedding` is that layer)
NEW_LAYERS = ('embedding', 'embedding_bn', 'prob', 'out2', 'labelembeddings')


def cross_entropy(logit, prob):
    """``K.sum(prob * log_softmax(logit), axis=1)`` (learn_labelembedding.py:17-18).  Plain torch: it is only
    used inside ``labelembed_loss`` in the reference, where the fused kernel computes it."""
    return torch.sum(prob * torch.log_softmax(logit, dim=1), dim=1)


def labelembed_loss(out1, out2, tar, targets, tau=2., alpha=0.9, beta=0.5, num_classes=100):
    """Same signature and meaning as the reference (learn_labelembedding.py:21-37); returns the per-sample loss
    ``[B]`` (the reference's Lambda layer appends ``[:, None]``, learn_labelembedding.py:54).  ``num_classes`` is
    accepted for signature compatibility; the class count is the logits' last dimension."""
    import sehip  # raises SehipError when the HIP library / a ROCm device is missing -- no CPU fallback
    targets = targets.reshape(-1).to(torch.int64).contiguous()
    return sehip.labelembed_loss(out1.float(), out2.float(), tar.float(), targets, tau=tau, alpha=alpha, beta=beta)


class LabelEmbedModel(torch.nn.Module):
    """``labelembed_model(base_model, num_classes, **kwargs)`` (learn_labelembedding.py:40-56) as a module: the base network's
    embedding goes through ReLU -> BatchNorm (``embedding_bn``) into two heads -- ``prob`` (out1) and ``out2``, the latter
    behind a stop-gradient -- and a learnable ``[C, C]`` label-embedding table initialised to the identity
    (``labelembeddings``) supplies ``tar`` for the sample's label.  ``forward(x, labels)`` returns the reference model's three
    outputs ``(embedding, out1, loss[:, None])`` with the loss computed by the fused HIP kernel, which reads the table row of each
    label in place.  ``forward(x)`` is the form ``engine.Trainer`` drives: ``(logits2, out1, embedding)`` with ``logits2`` the
    ``[B, 2 C]`` tensor ``out1 | out2`` for ``LabelEmbedLoss`` (the labels reach the loss as ``y``), ``out1`` for the accuracy of
    ``prob`` and the raw embedding for the feature dump."""

    def __init__(self, base_model, num_classes, embed_dim=None, tau=2., alpha=0.9, beta=0.5):
        super().__init__()
        from models.cifar_resnet import KERAS_BN_EPS, KERAS_BN_MOMENTUM, keras_dense
        self.base_model = base_model
        if embed_dim is None:
            head = getattr(base_model, 'head', None)
            embed_dim = head.out_features if head is not None else base_model.num_features
        self.embedding_bn = torch.nn.BatchNorm1d(embed_dim, eps=KERAS_BN_EPS, momentum=KERAS_BN_MOMENTUM)
        self.prob = keras_dense(embed_dim, num_classes)
        self.out2 = keras_dense(embed_dim, num_classes)
        self.labelembeddings = torch.nn.Embedding(num_classes, num_classes)
        with torch.no_grad():
            self.labelembeddings.weight.copy_(torch.eye(num_classes))
        self.num_classes, self.kwargs = num_classes, dict(tau=tau, alpha=alpha, beta=beta)

    def forward(self, x, labels=None):
        embedding = self.base_model(x)
        out = self.embedding_bn(torch.relu(embedding.float()))
        out1 = self.prob(out)
        out2 = self.out2(out.detach())                                  # Lambda(K.stop_gradient)
        if labels is None:                                              # the form engine.Trainer drives: the labels meet the loss there
            return torch.cat((out1, out2), dim=1), out1, embedding
        import sehip  # raises SehipError when the HIP library / a ROCm device is missing -- no CPU fallback
        labels = labels.reshape(-1).to(torch.int64).contiguous()
        loss = sehip.labelembed_table_loss(out1, out2, self.labelembeddings.weight, labels, **self.kwargs)
        return embedding, out1, loss[:, None]


def labelembed_model(base_model, num_classes, **kwargs):
    """Same call as the reference's factory (learn_labelembedding.py:40)."""
    return LabelEmbedModel(base_model, num_classes, **kwargs)


def transform_inputs(X, y, num_classes):
    """learn_labelembedding.py:59-61: inputs ``[X, y]``, targets for the two trained outputs (a dummy for the loss output, the
    labels -- instead of their one-hot encoding -- for ``prob``)."""
    return [X, y], {'labelembed_loss': torch.zeros((len(X), 1), device=X.device), 'prob': y}


def transform_trainer_inputs(X, y, num_classes):
    """The batch transform of the trainer form: the labels feed both trained outputs -- the label-embedding loss takes them as the
    rows of the table (the reference's second model input), the accuracy of ``prob`` as class indices."""
    return X, [y, y]


class LabelEmbedLoss(object):
    """``loss(labels [B] int64, logits2 [B, 2 C]) -> [B]``: the reference's ``labelembed_loss`` output (its Keras loss is the
    identity, learn_labelembedding.py:146) on ``out1 | out2`` and the table row of each label.  ``table`` is the ``labelembeddings``
    ``Parameter`` itself, not its ``.data``: the trainer re-homes the storage of every trainable parameter into its flat buffer.
    Data parallel: the batch-wide factor ``B / (sum mask + 1e-8)`` is over the rows this rank sees, like a ``multi_gpu_model``
    tower's."""

    name = 'labelembed_loss'

    def __init__(self, table, tau=2., alpha=0.9, beta=0.5):
        self.table, self.kwargs = table, dict(tau=tau, alpha=alpha, beta=beta)

    def __call__(self, y_true, y_pred):
        import sehip
        return sehip.labelembed_table_loss_packed(y_pred.float(), self.table, y_true.reshape(-1).to(torch.int64).contiguous(),
                                                  **self.kwargs)


def zero_loss(y_true, y_pred):
    """The reference's loss of the ``prob`` output (learn_labelembedding.py:146): identically zero; the output is there for its
    accuracy."""
    return torch.zeros((y_pred.shape[0],), dtype=torch.float32, device=y_pred.device)


def build_losses(model):
    """The reference's compile() (learn_labelembedding.py:169-171): output ``labelembed_loss`` with weight 1, output ``prob`` with a
    zero loss and the accuracy metric, in the order of the trainer form's outputs."""
    from learn_image_embeddings import accuracy
    losses = {'labelembed_loss': (LabelEmbedLoss(model.labelembeddings.weight, **model.kwargs), 1.0), 'prob': (zero_loss, 1.0)}
    return losses, {'prob': [accuracy]}


def build_parser():
    parser = argparse.ArgumentParser(description='Trains a label embedding network (Sun et al.) (MI355X build).',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('Data parameters')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--class_list', type=str, default=None, help='File whose lines start with the IDs of the classes to use.')
    g = parser.add_argument_group('Label embedding parameters')
    g.add_argument('--embed_dim', type=int, default=100, help='Embedding dimensionality.')
    g.add_argument('--tau', type=float, default=2., help='Softmax temperature.')
    g.add_argument('--alpha', type=float, default=0.9, help='Threshold of the ReLU term on the probability of the true class.')
    g.add_argument('--beta', type=float, default=0.5, help='Weight of the hard-label term of out1 (1 - beta: the soft-label term).')
    g = parser.add_argument_group('Training parameters')
    g.add_argument('--architecture', type=str, default='simple', choices=utils.ARCHITECTURES, help='Network architecture.')
    train_cli.add_schedule_arguments(g)
    train_cli.add_finetune_and_device_arguments(g, 3, 'Epochs training only the new layers first.')
    g = parser.add_argument_group('Output parameters')
    train_cli.add_output_arguments(g, 'Where to save raw test-image embeddings ({"feat": {i: vec}} pickle).')
    utils.add_lr_schedule_arguments(parser)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.val_batch_size is None:
        args.val_batch_size = args.batch_size

    rank, world, dev = train_cli.init_process(args, 'learn_labelembedding.py')

    # ---- dataset (learn_labelembedding.py:110-119)
    class_list = train_cli.read_class_list(args.class_list) if args.class_list is not None else None
    data_generator = train_cli.configure_loader(args, get_data_generator(args.dataset, args.data_root, classes=class_list))

    # ---- model (learn_labelembedding.py:122-130)
    torch.manual_seed(0)   # identical initial weights on every rank
    embed_model = utils.build_network(args.embed_dim, args.architecture, input_channels=data_generator.num_channels).to(dev)
    width = train_cli.output_width(embed_model, data_generator.num_channels, dev)
    model = labelembed_model(embed_model, data_generator.num_classes, embed_dim=width, tau=args.tau, alpha=args.alpha,
                             beta=args.beta).to(dev)
    if args.finetune:
        train_cli.load_pretrained(model, args.finetune, dev)

    losses, metrics = build_losses(model)
    # Keras kernel regulariser of the backbone folded into the update; the heads and the table carry none
    l2_of = {id(p): embed_model.regularizer for p in embed_model.regularized_parameters()} if getattr(embed_model, 'regularizer', 0) else {}

    dp = dict(rank=rank, world_size=world)
    kw = {'num_classes': data_generator.num_classes}
    train_seq = lambda: data_generator.train_sequence(args.batch_size, batch_transform=transform_trainer_inputs, batch_transform_kwargs=kw, **dp)
    val_seq = lambda: data_generator.test_sequence(args.val_batch_size, batch_transform=transform_trainer_inputs, batch_transform_kwargs=kw, **dp)

    # ---- optional warm-up of the new layers only (learn_labelembedding.py:137-155)
    if args.finetune and args.finetune_init > 0:
        # the backbone's last layer is its dense head `embedding` where it has one (pooled-feature backbones end without parameters)
        train_cli.warm_up(args, model, losses, metrics, l2_of, train_seq, val_seq,
                          lambda n: n.split('.')[0] in NEW_LAYERS or n.startswith('base_model.embedding.'), 'Pre-training new layers')

    # ---- main training (learn_labelembedding.py:157-178)
    trainer = train_cli.fit(args, model, losses, metrics, l2_of, data_generator, train_seq, val_seq, world)

    # ---- final evaluation (learn_labelembedding.py:180-190)
    final = trainer.evaluate(val_seq())
    _, out1, feats = trainer.predict(data_generator.test_sequence(args.val_batch_size))      # every test image, on every rank
    if rank == 0:
        pred, labels_test = out1.argmax(axis=-1), np.asarray(data_generator.labels_test)
        print([final[k] for k in sorted(final)], sorted(final))
        print('Accuracy: {:.4f}'.format(float(np.mean(pred == labels_test))))
        print('Average Accuracy: {:.4f}'.format(train_cli.average_accuracy(pred, labels_test)))

    # ---- dumps (learn_labelembedding.py:192-208): the feature dump holds the RAW embeddings of the backbone
    if rank == 0:
        train_cli.dump_model(args, model)
        if args.feature_dump:
            train_cli.dump_features(args.feature_dump, feats)
    train_cli.finish_process(world)
    return final


if __name__ == '__main__':
    main()
