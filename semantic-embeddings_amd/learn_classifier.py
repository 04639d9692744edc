"""Drop-in for the reference's ``learn_classifier.py``: learns a plain softmax image classifier -- the baseline of every comparison
and the source of the weights ``--finetune`` / ``--init_weights`` / ``--model`` of the other scripts consume -- same command line
(reference: learn_classifier.py:29-60 + utils.py:402-418), on MI355X.

    python learn_classifier.py --dataset synthetic-cifar100 --data_root . --architecture resnet-110-fc --batch_size 128 \
        --label_smoothing 0.1 --top_k_acc 5 --weight_dump classifier.pt
    # data parallel, one process per GPU over RCCL (instead of keras.utils.multi_gpu_model)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 learn_classifier.py ... --gpus 8

The network emits logits; the categorical cross-entropy with label smoothing, its gradient, ``accuracy`` and every ``--top_k_acc`` run on
the fused HIP kernel pair (``sehip.softmax_cross_entropy``): one forward and one backward launch per step serve the loss and all
metrics, with Keras 2.2's clip of the probabilities to [1e-7, 1 - 1e-7].

An extension the reference does not have: ``--loss hxe`` (hierarchical cross-entropy, ``--hxe_alpha``) and ``--loss soft_labels``
(cross-entropy against ``softmax(-beta * class distance)``, ``--soft_beta``) train the hierarchy-aware classification baselines on the
class tree given by ``--hierarchy`` / ``--is_a`` / ``--str_ids`` (``sehip.hierarchical_cross_entropy`` / ``sehip.soft_label_cross_entropy``:
again one forward and one backward launch for the loss and all metrics, no clip).  Without ``--loss`` nothing changes.

    python learn_classifier.py --dataset CIFAR-100 --data_root . --architecture resnet-110-fc --loss hxe --hierarchy cifar.parent-child.txt

Differences from the reference a user can observe: ``--gpus N`` expects to be launched with N processes (torchrun); ``--batch_size``
stays the GLOBAL batch and is split across the ranks like ``multi_gpu_model`` split it across towers; models, weights and snapshots
are torch ``state_dict`` / ``torch.save`` files, not Keras ``.h5`` (the saved model emits logits: its last layer is the dense layer
``prob`` without the softmax activation); ``--read_workers`` / ``--queue_size`` set the decode threads (at most 16) and the
batches of look-ahead (at most 4) of a dataset that streams its images (``-stream`` names) and are ignored otherwise (batches are
composed on the device); ``--gpu_merge`` is accepted and ignored (weights always live on the GPUs); ``--log_dir`` writes a JSON-lines log instead of TensorBoard events; ties in
the top-k accuracies are decided on the logits (in favour of the target, like ``tf.nn.in_top_k``), not on the rounded probabilities.
"""
import argparse

import torch
import torch.nn as nn

import sehip
import train_cli
import utils
from datasets import get_data_generator
from train_cli import read_class_list


def transform_inputs(X, y, num_classes, label_smoothing=0):
    """reference: learn_classifier.py:17-22.  The reference expands the labels to a smoothed one-hot matrix on the host; here the
    labels travel to the kernel and the smoothing lives in the loss object (``SoftmaxCrossEntropy``)."""
    return X, y


class SoftmaxCrossEntropy(object):
    """``loss(labels [B] int64, logits [B, C]) -> [B]``: Keras 2.2's 'categorical_crossentropy' of ``softmax(logits)`` against the
    target of the reference's transform_inputs (learn_classifier.py:17-22, 116-117, 146-147), one se_softmax_xent_fwd forward and one
    se_softmax_xent_bwd backward.  The forward call also leaves the arg-max class and the number of classes scoring above the label
    of every row; the metric callables ``acc`` / ``top_k(k)`` take them from there when they are asked about the same logits, so a
    step computes the loss and all metrics in that one launch.  A metric called on other logits computes itself."""

    name = 'categorical_crossentropy'

    def __init__(self, label_smoothing=0.0):
        self.label_smoothing = float(label_smoothing)
        self._last = None          # (logits, version, labels, best, above) of the last forward call
        self.acc = self._metric('acc', lambda y, best, above: best == y)

    def _forward(self, y_pred, y_true):
        return sehip.softmax_cross_entropy(y_pred, y_true, self.label_smoothing, reduction='none', return_metrics=True)

    def __call__(self, y_true, y_pred):
        loss_i, best, above = self._forward(y_pred, y_true)
        # the detached alias keeps the storage alive, so no other tensor can show up at this address with this version
        self._last = (y_pred.detach(), y_pred._version, y_true, best, above)
        return loss_i

    def _scores(self, y_true, y_pred):
        last = self._last
        if last is not None and last[0].data_ptr() == y_pred.data_ptr() and last[0].shape == y_pred.shape \
                and last[0].stride() == y_pred.stride() and last[0].dtype == y_pred.dtype and last[1] == y_pred._version \
                and last[2] is y_true:
            return last[3], last[4]
        with torch.no_grad():
            _, best, above = self._forward(y_pred.detach(), y_true)
        return best, above

    def _metric(self, name, rule):
        def metric(y_true, y_pred):
            best, above = self._scores(y_true, y_pred)
            return rule(y_true, best, above).float()
        metric.name = name
        return metric

    def top_k(self, k):
        """reference: utils.top_k_acc(k) (utils.py:49-54), ``tf.nn.in_top_k``: fewer than k classes score strictly above the label."""
        return self._metric('acc{}'.format(k), lambda y, best, above: above < int(k))


class HierarchicalCrossEntropy(SoftmaxCrossEntropy):
    """``SoftmaxCrossEntropy``'s interface (``__call__``, ``acc``, ``top_k(k)``) for the hierarchical cross-entropy of
    ``ClassHierarchy.hxe_encoding`` (``--loss hxe``): one se_hxe_fwd forward, which also leaves the metrics, one se_hxe_bwd backward."""

    name = 'hierarchical_crossentropy'

    def __init__(self, encoding):
        super(HierarchicalCrossEntropy, self).__init__(0.0)
        self.encoding = sehip.HxeEncoding.of(encoding)

    def _forward(self, y_pred, y_true):
        return sehip.hierarchical_cross_entropy(y_pred, y_true, self.encoding, reduction='none', return_metrics=True)


class SoftLabelCrossEntropy(SoftmaxCrossEntropy):
    """``SoftmaxCrossEntropy``'s interface for the cross-entropy against the soft labels of ``ClassHierarchy.soft_label_table``
    (``--loss soft_labels``): one se_soft_xent_fwd forward, which also leaves the metrics, one se_soft_xent_bwd backward."""

    name = 'soft_label_crossentropy'

    def __init__(self, table):
        super(SoftLabelCrossEntropy, self).__init__(0.0)
        self.table = table if isinstance(table, sehip.SoftLabelTable) else sehip.SoftLabelTable(table)

    def _forward(self, y_pred, y_true):
        return sehip.soft_label_cross_entropy(y_pred, y_true, self.table, reduction='none', return_metrics=True)


def hierarchy_loss(args, classes):
    """The loss object of ``--loss hxe`` / ``--loss soft_labels``: class ``c`` of the data generator is the hierarchy node
    ``classes[c]``, as in evaluate_classification_accuracy.py --hierarchy."""
    from class_hierarchy import ClassHierarchy
    hierarchy = ClassHierarchy.from_file(args.hierarchy, is_a_relations=args.is_a, id_type=str if args.str_ids else int)
    if args.loss == 'hxe':
        return HierarchicalCrossEntropy(hierarchy.hxe_encoding(list(classes), alpha=args.hxe_alpha))
    return SoftLabelCrossEntropy(hierarchy.soft_label_table(list(classes), args.soft_beta))


def build_losses(label_smoothing, top_k_acc=(), loss=None):
    """Both compile() calls of the reference (learn_classifier.py:103-106, 116-117, 146-147): the categorical cross-entropy with
    metrics 'accuracy' and utils.top_k_acc(k) for every ``--top_k_acc``.  ``loss``: another loss object with that interface."""
    if loss is None:
        loss = SoftmaxCrossEntropy(label_smoothing)
    return {'prob': (loss, 1.0)}, {'prob': [loss.acc] + [loss.top_k(k) for k in top_k_acc]}


def build_classifier(num_classes, architecture, input_channels=None):
    """``utils.build_network(num_classes, architecture, classification=True, no_softmax=True)`` (learn_classifier.py:88 builds it
    with the softmax; the kernel consumes logits) whose last dense layer carries the reference's layer name ``prob`` whatever the
    architecture calls a head without activation -- the name --finetune matches weights by."""
    model = utils.build_network(num_classes, architecture, classification=True, no_softmax=True, input_channels=input_channels)
    if getattr(model, 'prob', None) is None and getattr(model, 'embedding', None) is not None:
        model.prob = model.embedding
        del model.embedding
    return model


def final_dense(model):
    head = getattr(model, 'prob', None)
    if head is None:
        head = [m for m in model.modules() if isinstance(m, nn.Linear)][-1]
    return head


class FeatureTap(object):
    """Records the input of the model's final dense layer at every forward call -- or, where a BatchNorm sits directly in front of
    that layer, that BatchNorm's input (learn_classifier.py:179: ``model.layers[-2].output``, ``layers[-3]`` past a BatchNorm)."""

    def __init__(self, model):
        self.value, self._bn = None, None
        self._handles = [final_dense(model).register_forward_pre_hook(self._dense)]
        self._handles += [m.register_forward_hook(self._norm) for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]

    def _norm(self, module, inputs, output):
        self._bn = (inputs[0], output)

    def _dense(self, module, inputs):
        x = inputs[0]
        self.value = self._bn[0] if self._bn is not None and self._bn[1] is x else x

    def close(self):
        for h in self._handles:
            h.remove()
        self._handles = []


def predict_features(trainer, seq):
    """[N, width] float32 features of every image of ``seq`` in its order (``FeatureTap``)."""
    tap = FeatureTap(trainer.model)
    feats = []
    trainer.model.eval()
    try:
        with torch.no_grad():
            for i in range(len(seq)):
                batch = seq[i]
                trainer._forward(batch[0] if isinstance(batch, (tuple, list)) else batch)
                feats.append(tap.value.float().cpu())
    finally:
        tap.close()
        trainer.model.train()
    return torch.cat(feats).numpy()


def add_hierarchy_loss_arguments(group):
    """The flags of the hierarchy-aware losses, which the reference's command line does not have."""
    group.add_argument('--loss', type=str, default='xent', choices=['xent', 'hxe', 'soft_labels'],
                       help='xent: categorical cross-entropy.  hxe: hierarchical cross-entropy, the softmax factorised along the path of the label in the '
                            'class tree.  soft_labels: cross-entropy against softmax(-beta * class distance).  The last two need --hierarchy.')
    group.add_argument('--hierarchy', type=str, default=None, help='Path to a file containing parent-child relationships (one per line): the class tree of --loss hxe / soft_labels.')
    group.add_argument('--is_a', action='store_true', default=False, help='If given, --hierarchy is assumed to contain is-a instead of parent-child relationships.')
    group.add_argument('--str_ids', action='store_true', default=False, help='If given, class IDs are treated as strings instead of integers.')
    group.add_argument('--hxe_alpha', type=float, default=0.1,
                       help='--loss hxe: the edge below a node d edges under the top weighs exp(-alpha * d).  The default lies inside the range the literature sweeps; this project has not measured it.')
    group.add_argument('--soft_beta', type=float, default=10.0,
                       help='--loss soft_labels: the target of class y is softmax_c(-beta * lcs_height(y, c)).  The default lies inside the range the literature sweeps; this project has not measured it.')


def build_parser(hierarchy_losses=False):
    """The reference's command line; with ``hierarchy_losses`` also --loss and the flags that go with it (``parse_args`` asks for them)."""
    parser = argparse.ArgumentParser(description='Learns an image classifier (MI355X build).', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('Data parameters')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--class_list', type=str, default=None, help='File whose lines start with the IDs of the classes to use.')
    g = parser.add_argument_group('Training parameters')
    g.add_argument('--architecture', type=str, default='simple', choices=utils.ARCHITECTURES, help='Network architecture.')
    g.add_argument('--label_smoothing', type=float, default=0.0,
                   help='Smooth the target distribution by subtracting this value from the target probability of the ground-truth class.')
    if hierarchy_losses:
        add_hierarchy_loss_arguments(g)
    train_cli.add_schedule_arguments(g)
    train_cli.add_snapshot_arguments(g)
    train_cli.add_finetune_and_device_arguments(g, 3, 'Epochs training only the last layer first.')
    g = parser.add_argument_group('Output parameters')
    train_cli.add_output_arguments(g, 'Where to save test-image features ({"feat": {i: vec}} pickle).')
    g.add_argument('--top_k_acc', type=int, nargs='+', default=[], help='Also report these top-k accuracies.')
    utils.add_lr_schedule_arguments(parser)
    return parser


def parse_args(argv=None):
    parser = build_parser(hierarchy_losses=True)
    args = parser.parse_args(argv)
    if args.loss != 'xent':         # before any device work
        if not args.hierarchy:
            parser.error('--loss {} needs --hierarchy'.format(args.loss))
        if args.label_smoothing > 0:
            parser.error('--loss {} has a target of its own: it cannot be combined with --label_smoothing'.format(args.loss))
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.val_batch_size is None:
        args.val_batch_size = args.batch_size

    rank, world, dev = train_cli.init_process(args, 'learn_classifier.py')

    # ---- dataset (learn_classifier.py:70-80)
    class_list = read_class_list(args.class_list) if args.class_list is not None else None
    data_generator = train_cli.configure_loader(args, get_data_generator(args.dataset, args.data_root, classes=class_list))

    # ---- model (learn_classifier.py:83-97)
    torch.manual_seed(0)   # identical initial weights on every rank
    model = build_classifier(data_generator.num_classes, args.architecture, input_channels=data_generator.num_channels).to(dev)
    train_cli.resume_from_snapshot(model, args.snapshot, dev)

    losses, metrics = build_losses(args.label_smoothing, args.top_k_acc,
                                   hierarchy_loss(args, data_generator.classes) if args.loss != 'xent' else None)
    # Keras kernel regulariser of the network folded into the update
    l2_of = {id(p): model.regularizer for p in model.regularized_parameters()} if getattr(model, 'regularizer', 0) else {}

    dp = dict(rank=rank, world_size=world)
    kw = {'num_classes': data_generator.num_classes, 'label_smoothing': args.label_smoothing}
    train_seq = lambda: data_generator.train_sequence(args.batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)
    val_seq = lambda: data_generator.test_sequence(args.val_batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)

    # ---- pre-trained weights, and the last layer alone for a few epochs (learn_classifier.py:108-125)
    if args.finetune:
        train_cli.load_pretrained(model, args.finetune, dev)
        if args.finetune_init > 0:
            last = {id(p) for p in final_dense(model).parameters()}
            names = {n for n, p in model.named_parameters() if id(p) in last}
            train_cli.warm_up(args, model, losses, metrics, l2_of, train_seq, val_seq, lambda n: n in names, 'Pre-training last layer')

    # ---- main training (learn_classifier.py:127-155)
    trainer = train_cli.fit(args, model, losses, metrics, l2_of, data_generator, train_seq, val_seq, world)

    # ---- final evaluation (learn_classifier.py:157-163)
    final = trainer.evaluate(val_seq())
    logits = trainer.predict(data_generator.test_sequence(args.val_batch_size))       # every test image, on every rank
    if rank == 0:
        print([final['loss'], final['acc']] + [final['acc{}'.format(k)] for k in args.top_k_acc])
        print('Average Accuracy: {:.4f}'.format(train_cli.average_accuracy(logits.argmax(axis=-1), data_generator.labels_test)))

    # ---- dumps (learn_classifier.py:165-182)
    if rank == 0:
        train_cli.dump_model(args, model)
        if args.feature_dump:
            train_cli.dump_features(args.feature_dump, predict_features(trainer, data_generator.test_sequence(max(args.val_batch_size, 256))))
    train_cli.finish_process(world)
    return final


if __name__ == '__main__':
    main()
