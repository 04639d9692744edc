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

    def __call__(self, y_true, y_pred):
        loss_i, best, above = sehip.softmax_cross_entropy(y_pred, y_true, self.label_smoothing, reduction='none', return_metrics=True)
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
            _, best, above = sehip.softmax_cross_entropy(y_pred.detach(), y_true, self.label_smoothing, return_metrics=True)
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


def build_losses(label_smoothing, top_k_acc=()):
    """Both compile() calls of the reference (learn_classifier.py:103-106, 116-117, 146-147): the categorical cross-entropy with
    metrics 'accuracy' and utils.top_k_acc(k) for every ``--top_k_acc``."""
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


def build_parser():
    parser = argparse.ArgumentParser(description='Learns an image classifier (MI355X build).', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('Data parameters')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--class_list', type=str, default=None, help='File whose lines start with the IDs of the classes to use.')
    g = parser.add_argument_group('Training parameters')
    g.add_argument('--architecture', type=str, default='simple', choices=utils.ARCHITECTURES, help='Network architecture.')
    g.add_argument('--label_smoothing', type=float, default=0.0,
                   help='Smooth the target distribution by subtracting this value from the target probability of the ground-truth class.')
    train_cli.add_schedule_arguments(g)
    train_cli.add_snapshot_arguments(g)
    train_cli.add_finetune_and_device_arguments(g, 3, 'Epochs training only the last layer first.')
    g = parser.add_argument_group('Output parameters')
    train_cli.add_output_arguments(g, 'Where to save test-image features ({"feat": {i: vec}} pickle).')
    g.add_argument('--top_k_acc', type=int, nargs='+', default=[], help='Also report these top-k accuracies.')
    utils.add_lr_schedule_arguments(parser)
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
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

    losses, metrics = build_losses(args.label_smoothing, args.top_k_acc)
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
