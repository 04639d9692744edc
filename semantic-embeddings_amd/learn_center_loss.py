"""Drop-in for the reference's ``learn_center_loss.py``: learns image embeddings with a softmax classifier plus the center loss of
Wen et al., same command line (reference: learn_center_loss.py:50-83 + utils.py:402-418), on MI355X.

    python learn_center_loss.py --dataset synthetic-cifar100 --data_root . --architecture resnet-110-fc --batch_size 128 \
        --feature_dump center_loss_features.pickle
    # data parallel, one process per GPU over RCCL (instead of keras.utils.multi_gpu_model)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 learn_center_loss.py ... --gpus 8

The center loss and its gradients run on the HIP kernels (``sehip.center_loss``): the forward pass and the feature gradient on the
squared-distance loss head, the gradient of the learned centroid table on a fixed-order per-class reduction.

Differences from the reference a user can observe: ``--gpus N`` expects to be launched with N processes (torchrun); ``--batch_size``
stays the GLOBAL batch and is split across the ranks like ``multi_gpu_model`` split it across towers; models and weights are torch
``state_dict`` / ``torch.save`` files, not Keras ``.h5``; ``--read_workers`` / ``--queue_size`` set the decode threads (at most 16) and
the batches of look-ahead (at most 4) of a dataset that streams its images (``-stream`` names) and are ignored otherwise (batches are
composed on the device); ``--gpu_merge`` is accepted and ignored (weights always live on the GPUs); ``--log_dir`` writes a JSON-lines log instead of
TensorBoard events; the ``prob`` cross-entropy is computed from the logits, without Keras 2.2's clip of the probabilities to
[1e-7, 1 - 1e-7] (the same as the ``--cls_weight`` head of learn_image_embeddings.py).
"""
import argparse
import pickle

import numpy as np
import torch
import torch.nn as nn

import sehip
import train_cli
import utils
from datasets import get_data_generator
from learn_image_embeddings import accuracy, categorical_crossentropy
from models.cifar_resnet import KERAS_BN_EPS, KERAS_BN_MOMENTUM, keras_dense
from train_cli import read_class_list

NEW_LAYERS = ('embedding_bn', 'prob', 'cls_centroids')    # with the backbone's `embedding` head: what --finetune_init trains first


class CenterLossModel(nn.Module):
    """Embedding model + classifier head (ReLU -> BN ``embedding_bn`` -> Dense ``prob``) + the class centroid table
    ``cls_centroids`` (reference: center_loss_model, learn_center_loss.py:17-41).  ``forward`` returns ``(logits, embedding)``: the
    head emits logits (the categorical cross-entropy is applied on them) and the raw embedding feeds the center loss, which reads
    the table directly instead of looking it up with a second model input.

    ``num_classes_or_centroids``: the number of classes (learned centroids, Keras' ``Embedding`` initialiser U(-0.05, 0.05)) or a
    [C, D] array of fixed centroids (``trainable = False``: the table does not require grad)."""

    def __init__(self, embed_model, num_classes_or_centroids, width=None):
        super().__init__()
        centroids = num_classes_or_centroids if isinstance(num_classes_or_centroids, np.ndarray) else None
        num_classes = centroids.shape[0] if centroids is not None else int(num_classes_or_centroids)
        if width is None:      # output width of the embedding model (resnet-32 / -110 without -fc: the pooled features)
            head = getattr(embed_model, 'head', None)
            width = centroids.shape[1] if centroids is not None else (head.out_features if head is not None else embed_model.num_features)
        self.embed_model = embed_model
        self.embedding_bn = nn.BatchNorm1d(width, eps=KERAS_BN_EPS, momentum=KERAS_BN_MOMENTUM)
        self.embedding_bn.register_buffer('num_batches_tracked', None)     # Keras keeps no batch counter (models/cifar_resnet.keras_bn)
        self.prob = keras_dense(width, num_classes)
        self.cls_centroids = nn.Embedding(num_classes, width)
        with torch.no_grad():
            if centroids is None:
                self.cls_centroids.weight.uniform_(-0.05, 0.05)
            else:
                self.cls_centroids.weight.copy_(torch.from_numpy(np.asarray(centroids, dtype=np.float32)))
        self.cls_centroids.weight.requires_grad_(centroids is None)

    def forward(self, x):
        emb = self.embed_model(x)
        return self.prob(self.embedding_bn(torch.relu(emb.float()))), emb


def center_loss_model(base_model, centroids, width=None):
    """reference: center_loss_model(base_model, centroids) (learn_center_loss.py:17-41)."""
    return CenterLossModel(base_model, centroids, width=width)


def transform_inputs(X, y, num_classes):
    """reference: learn_center_loss.py:44-46.  The labels feed both outputs: the cross-entropy takes them as class indices, the
    center loss as the rows of the centroid table (the reference's second model input)."""
    return X, [y, y]


class CenterLoss(object):
    """``loss(labels [B] int64, embedding [B, D]) -> [B]``: sum_d (embedding - centroids[labels])^2 / 2 (learn_center_loss.py:35-39;
    its Keras loss is the identity).  ``centroids`` is the table's ``Parameter`` itself, not its ``.data``: the trainer re-homes the
    storage of every trainable parameter into its flat buffer."""

    name = 'center_loss'

    def __init__(self, centroids):
        self.centroids = centroids

    def __call__(self, y_true, y_pred):
        return sehip.center_loss(y_pred, y_true, self.centroids)


def build_losses(model, center_loss_weight):
    """The reference's compile() (learn_center_loss.py:162-165): outputs ``prob`` and ``center_loss`` with weights 1 and
    ``center_loss_weight``, accuracy of ``prob``."""
    losses = {'prob': (categorical_crossentropy, 1.0), 'center_loss': (CenterLoss(model.cls_centroids.weight), center_loss_weight)}
    return losses, {'prob': [accuracy]}


def build_parser():
    parser = argparse.ArgumentParser(description='Learns image embeddings using softmax + center loss (Wen et al.) (MI355X build).',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('Data parameters')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--class_list', type=str, default=None, help='File whose lines start with the IDs of the classes to use.')
    g = parser.add_argument_group('Center loss parameters')
    g.add_argument('--embed_dim', type=int, default=100, help='Dimensionality of the learned image embeddings.')
    g.add_argument('--centroids', type=str, default=None,
                   help='Pickle written by compute_class_embedding.py: a fixed set of class centroids instead of learned ones.')
    g.add_argument('--center_loss_weight', type=float, default=0.1, help='Weight of the center loss (the softmax loss has weight 1).')
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

    rank, world, dev = train_cli.init_process(args, 'learn_center_loss.py')

    # ---- class centroids / class list (learn_center_loss.py:93-108)
    centroids = class_list = None
    embed_dim = args.embed_dim
    if args.centroids:
        with open(args.centroids, 'rb') as pf:
            dump = pickle.load(pf)
        class_list, centroids = dump['ind2label'], np.asarray(dump['embedding'])
        embed_dim = centroids.shape[1]
    elif args.class_list is not None:
        class_list = read_class_list(args.class_list)
    data_generator = train_cli.configure_loader(args, get_data_generator(args.dataset, args.data_root, classes=class_list))

    # ---- model (learn_center_loss.py:113-124)
    torch.manual_seed(0)   # identical initial weights on every rank
    embed_model = utils.build_network(embed_dim, args.architecture, input_channels=data_generator.num_channels).to(dev)
    width = train_cli.output_width(embed_model, data_generator.num_channels, dev)
    model = center_loss_model(embed_model, centroids if centroids is not None else data_generator.num_classes, width=width).to(dev)
    if args.finetune:
        train_cli.load_pretrained(model, args.finetune, dev)

    losses, metrics = build_losses(model, args.center_loss_weight)
    # Keras kernel regulariser of the backbone folded into the update; the head and the centroids carry none
    l2_of = {id(p): embed_model.regularizer for p in embed_model.regularized_parameters()} if getattr(embed_model, 'regularizer', 0) else {}

    dp = dict(rank=rank, world_size=world)
    kw = {'num_classes': data_generator.num_classes}
    train_seq = lambda: data_generator.train_sequence(args.batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)
    val_seq = lambda: data_generator.test_sequence(args.val_batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)

    # ---- optional warm-up of the new layers only (learn_center_loss.py:128-148)
    if args.finetune and args.finetune_init > 0:
        if centroids is not None:
            # the reference's layer loops make every layer named cls_centroids trainable here and every layer afterwards
            print('note: --finetune with --finetune_init > 0 trains the --centroids table as well, like the reference')
        train_cli.warm_up(args, model, losses, metrics, l2_of, train_seq, val_seq,
                          lambda n: n.split('.')[0] in NEW_LAYERS or n.startswith('embed_model.embedding.'), 'Pre-training new layers')

    # ---- main training (learn_center_loss.py:150-172)
    trainer = train_cli.fit(args, model, losses, metrics, l2_of, data_generator, train_seq, val_seq, world)

    # ---- final evaluation (learn_center_loss.py:174-180)
    final = trainer.evaluate(val_seq())
    logits, feats = trainer.predict(data_generator.test_sequence(args.val_batch_size))      # every test image, on every rank
    if rank == 0:
        print([final[k] for k in sorted(final)], sorted(final))
        print('Average Accuracy: {:.4f}'.format(train_cli.average_accuracy(logits.argmax(axis=-1), data_generator.labels_test)))

    # ---- dumps (learn_center_loss.py:182-198): the feature dump holds the RAW embeddings
    if rank == 0:
        train_cli.dump_model(args, model)
        if args.feature_dump:
            train_cli.dump_features(args.feature_dump, feats)
    train_cli.finish_process(world)
    return final


if __name__ == '__main__':
    main()
