"""Drop-in for the reference's ``learn_image_embeddings.py``: learns to map images onto class
embeddings (cosine loss on hierarchy-based unit-sphere embeddings by default), same command line
(reference: learn_image_embeddings.py:57-96 + utils.py:402-418), on MI355X.

    # single GPU
    python learn_image_embeddings.py --dataset synthetic-cifar100 --data_root . \
        --embedding embeddings/cifar100.unitsphere.pickle --architecture resnet-110-fc --batch_size 128
    # data parallel, one process per GPU over RCCL (instead of keras.utils.multi_gpu_model)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 learn_image_embeddings.py ... --gpus 8

Differences from the reference a user can observe: ``--gpus N`` expects to be launched with N
processes (torchrun); ``--batch_size`` stays the GLOBAL batch and is split across the ranks like
``multi_gpu_model`` split it across towers; models / snapshots are torch ``state_dict`` files, not
Keras ``.h5``; ``--read_workers`` / ``--queue_size`` set the decode threads (at most 16) and the batches of
look-ahead (at most 4) of a dataset that streams its images (``-stream`` names) and are ignored otherwise
(batches are composed on the device); ``--log_dir`` writes a JSON-lines log instead of TensorBoard events.
"""
import argparse
import os
import pickle

import numpy as np
import torch
import torch.nn as nn

import train_cli
import utils
from datasets import get_data_generator
from models.cifar_resnet import keras_bn, keras_dense
from train_cli import JsonLogger


class ClsModel(nn.Module):
    """Embedding model + classifier head (ReLU -> BN -> Dense softmax named ``prob``), two outputs
    (reference: cls_model, learn_image_embeddings.py:16-45).  The reference appends the classifier to the model that
    already ENDS in the ``l2norm`` Lambda layer (``--loss inv_corr``) or the ``softmax`` activation (``softmax_corr``)
    (learn_image_embeddings.py:127-133), so its base is the normalised / soft-maxed output; that tensor is also the first
    output, which loss and metrics consume.  The head emits logits; the categorical cross-entropy is applied on them."""

    def __init__(self, embed_model, num_classes, cls_base=None, head=None, width=None):
        super().__init__()
        if head not in (None, 'l2norm', 'softmax'):
            raise ValueError('head must be None, "l2norm" or "softmax"')
        self.embed_model = embed_model
        self.head = head
        self._tap = None
        self.cls_base = None
        # cls_base 'l2norm' / 'softmax' names the LAST layer of the reference's embedding model (learn_image_embeddings.py:127-133):
        # its output is the first output itself, i.e. the default base -- nothing to tap.
        if cls_base is not None and str(cls_base) not in ('l2norm', 'softmax'):
            # reference: `embed_model.layers[int(cls_base)].output` / `embed_model.get_layer(cls_base).output`
            # (learn_image_embeddings.py:34-40).  Names are module names of the embedding model ('avg_pool' = the pooled backbone
            # features, 'embedding' = the dense layer in front of l2norm, dotted names for anything deeper); an integer indexes its
            # leaf modules in definition order (Keras numbers its own layer list: indices are not portable between the two).
            named = [(n, m) for n, m in embed_model.named_modules() if n]
            no_such = '--cls_base {!r}: no such layer; the embedding model has {}'.format(cls_base, ', '.join(n for n, _ in named))
            try:
                index = int(cls_base)
            except ValueError:
                index = None
            if index is not None:
                leaves = [(n, m) for n, m in named if not list(m.children())]
                if not -len(leaves) <= index < len(leaves):
                    raise ValueError(no_such + ' ({} leaf layers)'.format(len(leaves)))
                name, tap = leaves[index]
            else:
                found = dict(named)
                if str(cls_base) not in found:
                    raise ValueError(no_such)
                name, tap = str(cls_base), found[str(cls_base)]
            # the tap's width must follow from the layer itself -- the caller's `width` describes the embedding OUTPUT, not an inner layer
            if isinstance(tap, nn.Linear):
                width = tap.out_features
            elif isinstance(tap, (nn.BatchNorm1d, nn.BatchNorm2d)):
                width = tap.num_features
            elif name == 'avg_pool' or name.endswith('.avg_pool'):
                width = embed_model.num_features
            else:
                raise ValueError('--cls_base {!r} ({}): cannot tell the width of that layer\'s output (dense, batch-norm and avg_pool '
                                 'layers are supported)'.format(cls_base, type(tap).__name__))
            self.cls_base = name
            tap.register_forward_hook(self._remember)
        if width is None:       # width of what the embedding model emits (resnet-32 / -110 without -fc: the pooled features)
            width = embed_model.head.out_features if getattr(embed_model, 'head', None) is not None else None
        if width is None:
            raise ValueError('ClsModel needs the output width of the embedding model')
        self.bn = nn.BatchNorm1d(width, eps=1e-3, momentum=0.01)
        self.prob = keras_dense(width, num_classes)
        self.cls_l2 = 5e-4

    def _remember(self, module, inputs, output):
        self._tap = output

    def forward(self, x):
        emb = self.embed_model(x)
        if self.head == 'l2norm':
            base = utils.l2norm(emb)                    # HIP kernel with autograd (utils.py:125-127)
        elif self.head == 'softmax':
            base = torch.softmax(emb.float(), -1)
        else:
            base = emb.float()
        cls_in = base
        if self.cls_base is not None:                   # the classifier hangs off an inner layer; the first output stays the embedding
            cls_in, self._tap = self._tap, None
            if cls_in is None or cls_in.dim() != 2:
                raise ValueError('--cls_base {!r} does not produce a [batch, features] tensor'.format(self.cls_base))
            cls_in = cls_in.float()
        return base, self.prob(self.bn(torch.relu(cls_in)))


def transform_inputs(X, y, embedding=None, num_classes=None):
    """reference: learn_image_embeddings.py:48-50.  The reference gathers ``embedding[y]`` on the
    host; here the labels travel to the fused kernel, which gathers on the device."""
    return (X, y) if num_classes is None else (X, [y, y])


def categorical_crossentropy(y_true, logits):
    return nn.functional.cross_entropy(logits.float(), y_true, reduction='none')


def accuracy(y_true, out):
    return (out.argmax(dim=-1) == y_true).float()


accuracy.name = 'acc'


def head_by_default(loss, onehot_metrics, num_top_k):
    """Whether the embedding head (loss and nearest-class metric in one launch, utils.CosineEmbeddingHead / SquaredDistanceHead)
    replaces the loss object + one utils.nn_accuracy launch per metric.  The logged values are the same bits either way; this only
    chooses the faster sequence, from profiles/embed_head_bench.txt: the head was not slower at any measured shape (128 x 100 x 100 to
    256 x 1000 x 1000, float32 and bfloat16 features), for either loss, against one, two or three metric launches (x1.27 at the
    least), so every such configuration takes it.  One-hot targets use arg-max metrics, which the head does not serve."""
    if onehot_metrics:
        return False
    return True


def joint_head_by_default(loss, onehot, cls_weight):
    """Whether utils.JointEmbeddingHead (embedding loss, classifier cross-entropy and the metrics of both outputs in one launch)
    replaces the torch composition.  It serves `--cls_weight > 0` with `--loss inv_corr | unnorm_corr | softmax_corr`, class table or
    `onehot`, and `--cls_weight 0` with unnorm_corr / softmax_corr; `mse` with a classifier branch and inv_corr without one keep
    what they have.  Unlike head_by_default this one changes logged values (Keras' probability clip in the classifier loss,
    tf.nn.in_top_k's ties for top-k of logits and one-hot outputs, the kernel's summation order in the embedding loss), so it
    stays behind the host-side switch SE_JOINT_HEAD=1 until a change that owns those differences flips the default."""
    if os.environ.get('SE_JOINT_HEAD') != '1':
        return False
    if loss not in ('inv_corr', 'unnorm_corr', 'softmax_corr'):
        return False
    if cls_weight > 0:
        return True
    return loss in ('unnorm_corr', 'softmax_corr')


def build_parser():
    parser = argparse.ArgumentParser(description='Learns to map images onto class embeddings (MI355X build).',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('Data parameters')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--embedding', type=str, required=True,
                   help='Pickle written by compute_class_embedding.py ({"embedding", "ind2label", ...}) or "onehot".')
    g = parser.add_argument_group('Training parameters')
    g.add_argument('--architecture', type=str, default='simple', choices=utils.ARCHITECTURES, help='Network architecture.')
    g.add_argument('--loss', type=str, default='inv_corr', choices=['mse', 'inv_corr', 'unnorm_corr', 'softmax_corr'],
                   help='"inv_corr": cosine loss on L2-normalised outputs (fused HIP kernel); "mse": squared distance; '
                        '"unnorm_corr"/"softmax_corr": negated dot product without normalisation / after softmax.')
    g.add_argument('--cls_weight', type=float, default=0.0, help='Weight of an additional softmax classification loss (0 = off).')
    g.add_argument('--cls_base', type=str, default=None, help='Name or index of the layer that the classification layer should be based on. If not specified, the final embedding layer will be used.')
    train_cli.add_schedule_arguments(g)
    train_cli.add_snapshot_arguments(g)
    train_cli.add_finetune_and_device_arguments(g, 8, 'Epochs training only the new layers first.')
    g = parser.add_argument_group('Output parameters')
    train_cli.add_output_arguments(g, 'Where to save test-image embeddings ({"feat": {i: vec}} pickle).')
    g.add_argument('--top_k_acc', type=int, nargs='+', default=[], help='Also report these top-k accuracies.')
    utils.add_lr_schedule_arguments(parser)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.val_batch_size is None:
        args.val_batch_size = args.batch_size

    rank, world, dev = train_cli.init_process(args, 'learn_image_embeddings.py')

    # ---- class embeddings (learn_image_embeddings.py:105-117)
    if args.embedding == 'onehot':
        embed_labels, embedding = None, None
    else:
        with open(args.embedding, 'rb') as pf:
            dump = pickle.load(pf)
        embed_labels, embedding = dump['ind2label'], dump['embedding']
    data_generator = train_cli.configure_loader(args, get_data_generator(args.dataset, args.data_root, classes=embed_labels))
    if embedding is None:
        embedding = np.eye(data_generator.num_classes)
    emb_dev = torch.from_numpy(np.asarray(embedding, dtype=np.float32)).to(dev).contiguous()   # f64 -> f32 like the TF feed

    # ---- model (learn_image_embeddings.py:120-148)
    torch.manual_seed(0)   # identical initial weights on every rank
    embed_model = utils.build_network(embedding.shape[1], args.architecture, input_channels=data_generator.num_channels).to(dev)
    model = embed_model
    if args.cls_weight > 0:
        width = train_cli.output_width(embed_model, data_generator.num_channels, dev)
        model = ClsModel(embed_model, data_generator.num_classes, args.cls_base,
                         head={'inv_corr': 'l2norm', 'softmax_corr': 'softmax'}.get(args.loss), width=width).to(dev)
    train_cli.resume_from_snapshot(model, args.snapshot, dev)
    if args.finetune:
        train_cli.load_pretrained(model, args.finetune, dev)

    # ---- loss / metrics (learn_image_embeddings.py:160-180)
    onehot_like = (args.loss == 'softmax_corr') or (args.embedding == 'onehot')
    joint = None
    if joint_head_by_default(args.loss, args.embedding == 'onehot', args.cls_weight) and \
            (not onehot_like or emb_dev.shape[1] == data_generator.num_classes):     # arg-max metrics read the label's column
        # one launch per step: embedding loss, Keras' clipped cross-entropy and every metric of both outputs
        post = (lambda o: torch.softmax(o, -1)) if (args.loss == 'softmax_corr' and args.cls_weight <= 0) else None
        joint = utils.JointEmbeddingHead(None if args.embedding == 'onehot' else emb_dev, 'argmax' if onehot_like else 'nearest', post=post,
                                          shared_labels=True)      # transform_inputs feeds [y, y]
        loss = joint.inv_correlation
        metrics = [joint.accuracy()] + [joint.accuracy(k) for k in args.top_k_acc]
    elif args.loss == 'inv_corr' and args.cls_weight > 0:
        # the classifier branch needs the normalised embedding as a tensor of the graph (ClsModel applies the l2norm kernel);
        # the cosine loss is then the plain inv_correlation on it, like the reference (utils.py:44-46)
        loss = lambda y, o: utils.inv_correlation(emb_dev[y], o)
        metrics = [accuracy if onehot_like else utils.nn_accuracy(emb_dev, dot_prod_sim=True)]
        metrics += [utils.top_k_acc(k) if onehot_like else utils.nn_accuracy(emb_dev, dot_prod_sim=True, k=k) for k in args.top_k_acc]
    elif args.loss == 'inv_corr' and head_by_default('inv_corr', onehot_like, len(args.top_k_acc)):
        loss = utils.CosineEmbeddingHead(emb_dev)          # fused l2norm + gather + 1 - <.,.> + the metric's counts, one launch
        metrics = [loss.accuracy()] + [loss.accuracy(k) for k in args.top_k_acc]
    elif args.loss == 'inv_corr':
        loss = utils.CosineEmbeddingLoss(emb_dev)          # fused l2norm + gather + 1 - <.,.>
        metrics = [accuracy if onehot_like else utils.nn_accuracy(emb_dev, dot_prod_sim=True)]
        metrics += [utils.top_k_acc(k) if onehot_like else utils.nn_accuracy(emb_dev, dot_prod_sim=True, k=k) for k in args.top_k_acc]
    elif args.loss.endswith('_corr'):
        # (with --cls_weight the model already emits the soft-maxed output, see ClsModel)
        post = (lambda o: torch.softmax(o.float(), -1)) if (args.loss == 'softmax_corr' and args.cls_weight <= 0) else (lambda o: o.float())
        loss = lambda y, o: utils.inv_correlation(emb_dev[y], post(o))
        metrics = [accuracy if onehot_like else utils.nn_accuracy(emb_dev, dot_prod_sim=True)]
        metrics += [utils.top_k_acc(k) if onehot_like else utils.nn_accuracy(emb_dev, dot_prod_sim=True, k=k) for k in args.top_k_acc]
    elif head_by_default('mse', args.embedding == 'onehot', len(args.top_k_acc)):
        loss = utils.SquaredDistanceHead(emb_dev)          # fused gather + squared distance + the metric's counts, one launch
        metrics = [loss.accuracy()] + [loss.accuracy(k) for k in args.top_k_acc]
    else:
        loss = utils.SquaredDistanceLoss(emb_dev)          # fused gather + squared distance (se_sqdist_loss_fwd / bwd)
        metrics = [accuracy if args.embedding == 'onehot' else utils.nn_accuracy(emb_dev, dot_prod_sim=False)]
        metrics += [utils.top_k_acc(k) if args.embedding == 'onehot' else utils.nn_accuracy(emb_dev, dot_prod_sim=False, k=k) for k in args.top_k_acc]
    embedding_layer_name = {'inv_corr': 'l2norm', 'softmax_corr': 'softmax'}.get(args.loss, 'embedding')
    losses = {embedding_layer_name: (loss, 1.0)}
    all_metrics = {embedding_layer_name: metrics}
    if args.cls_weight > 0:
        losses['prob'] = (joint.categorical_crossentropy if joint else categorical_crossentropy, args.cls_weight)
        all_metrics['prob'] = ([joint.cls_accuracy()] + [joint.cls_accuracy(k) for k in args.top_k_acc]) if joint else \
            ([accuracy] + [utils.top_k_acc(k) for k in args.top_k_acc])
    trainer_kw = {'joint_head': joint} if joint else {}

    # Keras kernel regularisers folded into the update: backbone 2e-4, classifier 5e-4
    l2_of = {id(p): embed_model.regularizer for p in embed_model.regularized_parameters()} if getattr(embed_model, 'regularizer', 0) else {}
    if args.cls_weight > 0:
        l2_of[id(model.prob.weight)] = model.cls_l2

    dp = dict(rank=rank, world_size=world)
    kw = {'embedding': embedding, 'num_classes': data_generator.num_classes if args.cls_weight > 0 else None}
    train_seq = lambda: data_generator.train_sequence(args.batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)
    val_seq = lambda: data_generator.test_sequence(args.val_batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)

    # ---- optional warm-up of the new layers only (learn_image_embeddings.py:183-207)
    if args.finetune and args.finetune_init > 0:
        train_cli.warm_up(args, model, losses, all_metrics, l2_of, train_seq, val_seq,
                          lambda n: ('embedding' in n) or ('prob' in n), 'Pre-training new layers', **trainer_kw)

    # ---- main training (learn_image_embeddings.py:209-243)
    trainer = train_cli.fit(args, model, losses, all_metrics, l2_of, data_generator, train_seq, val_seq, world, **trainer_kw)

    # ---- final evaluation (learn_image_embeddings.py:246-255)
    final = trainer.evaluate(val_seq())
    if rank == 0:
        print([final[k] for k in sorted(final)], sorted(final))
    if (args.cls_weight > 0) or (args.embedding == 'onehot'):
        pred = trainer.predict(data_generator.test_sequence(args.val_batch_size))
        pred = (pred[1] if args.cls_weight > 0 else pred).argmax(axis=-1)
        if rank == 0 and world == 1:
            print('Average Accuracy: {:.4f}'.format(train_cli.average_accuracy(pred, data_generator.labels_test)))

    # ---- dumps (learn_image_embeddings.py:258-275)
    if rank == 0:
        train_cli.dump_model(args, model)
        if args.feature_dump:
            feats = trainer.predict(data_generator.test_sequence(max(args.val_batch_size, 256)))
            feats = feats[0] if args.cls_weight > 0 else feats
            if args.cls_weight > 0:
                pass                        # ClsModel's first output already is the l2norm / softmax layer's
            elif args.loss == 'inv_corr':   # the reference's model ends in the l2norm layer
                feats = utils.l2norm(torch.from_numpy(feats).to(dev)).cpu().numpy()
            elif args.loss == 'softmax_corr':
                feats = torch.softmax(torch.from_numpy(feats), -1).numpy()
            train_cli.dump_features(args.feature_dump, feats)
    train_cli.finish_process(world)
    return final


if __name__ == '__main__':
    main()
