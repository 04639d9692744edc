"""Drop-in for the reference's ``learn_devise.py``: learns to map images onto the embeddings of their labels with DeViSE (Frome et
al.) -- a hinge ranking loss on dot products, trained with Adagrad, first the linear transformation on top of a pre-trained network
alone, then all layers -- same command line (reference: learn_devise.py:25-48), on MI355X.

    python learn_devise.py --dataset synthetic-cifar100 --data_root . --embedding embeddings/cifar100.unitsphere.pickle \
        --architecture resnet-110-fc --init_weights classifier.pt --batch_size 128 --feature_dump devise_features.pickle
    # data parallel, one process per GPU over RCCL
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 learn_devise.py ... --gpus 8

The ranking loss and its gradient run on the fused HIP kernel pair (``sehip.devise_ranking_loss``: the labels travel to the kernel,
which gathers the target rows on the device), ``max_sim_acc`` on ``sehip.nn_accuracy``, and Keras 2.2's Adagrad update -- with the
kernel regularisers of the network and the mean over the ranks folded in -- is one launch over the flat parameter buffers
(``sehip.adagrad_step_``).

Differences from the reference a user can observe: ``--gpus N`` (an extension: the reference trains on one GPU) expects to be
launched with N processes (torchrun) and ``--batch_size`` stays the GLOBAL batch; ``--init_weights`` is a torch ``state_dict`` or
``torch.save`` model, not a Keras ``.h5`` model: every tensor that matches the network by name and shape is taken, so a classifier's
``prob`` layer is left behind and the dense layer ``embedding`` starts fresh (a network that ends in its pooled features -- resnet-32,
resnet-110 -- gets that layer appended, like the reference appends it to ``model.layers[-1].input``); models and weights are written
as torch files; ``--read_workers`` / ``--queue_size`` set the decode threads (at most 16) and the batches of look-ahead (at most 4) of a
dataset that streams its images (``-stream`` names) and are ignored otherwise (batches are composed on the device); ``--log_dir``
writes a JSON-lines log instead of TensorBoard events; the model summary is not printed.
"""
import argparse
import pickle

import numpy as np
import torch

import train_cli
import utils
from datasets import get_data_generator
from models.cifar_resnet import keras_dense


def transform_inputs(X, y, embedding):
    """reference: learn_devise.py:16-18.  The reference gathers ``embedding[y]`` on the host; here the labels travel to the fused
    loss and metric kernels, which gather on the device."""
    return X, y


def load_embedding(path):
    """``(ind2label, embedding)`` of a class-embedding pickle, the rows L2-normalised in float32 (learn_devise.py:58-62)."""
    with open(path, 'rb') as pf:
        dump = pickle.load(pf)
    embedding = np.array(dump['embedding'], dtype=np.float32)
    embedding /= np.linalg.norm(embedding, axis=-1, keepdims=True)
    return dump['ind2label'], embedding


def build_losses(embedding, margin):
    """Both compile() calls of the reference (learn_devise.py:87-89, 114-116)."""
    return ({'embedding': (utils.devise_ranking_loss(embedding, margin), 1.0)},
            {'embedding': [utils.nn_accuracy(embedding, dot_prod_sim=True)]})


def embedding_layer(model, width):
    """The final dense layer ``embedding`` of ``model``.  A network that ends in its pooled features has none: it gets one appended,
    the reference's ``Dense(width, name='embedding')(model.layers[-1].input)`` (learn_devise.py:71-72)."""
    head = getattr(model, 'embedding', None)
    if head is None:
        if not hasattr(model, 'num_features') or getattr(model, 'include_top', True):
            raise ValueError('the network has no dense layer named "embedding" and none can be appended to it')
        head = keras_dense(model.num_features, width).to(next(model.parameters()).device)
        model.embedding, model.include_top, model.top_activation = head, True, None
    return head


def build_parser():
    parser = argparse.ArgumentParser(description='Learns to map image features onto word embeddings of labels using DeViSE (MI355X build).',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('Data parameters')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--embedding', type=str, required=True, help='Pickle dump of class embeddings as written by compute_class_embedding.py.')
    g = parser.add_argument_group('Training parameters')
    g.add_argument('--architecture', type=str, default='simple', choices=utils.ARCHITECTURES, help='Network architecture.')
    g.add_argument('--init_weights', type=str, default=None, help='state_dict or model with pre-trained weights (matched by name and shape).')
    g.add_argument('--init_epochs', type=int, default=25, help='Epochs training only the linear transformation layer first.')
    g.add_argument('--ft_epochs', type=int, default=75, help='Epochs fine-tuning the full network.')
    g.add_argument('--init_lr', type=float, default=0.01, help='Adagrad learning rate while training the linear transformation.')
    g.add_argument('--ft_lr', type=float, default=0.001, help='Adagrad learning rate while fine-tuning the full network.')
    g.add_argument('--batch_size', type=int, default=100, help='Global batch size.')
    g.add_argument('--val_batch_size', type=int, default=None, help='Validation batch size.')
    g.add_argument('--max_decay', type=float, default=0.0, help='Learning-rate decay reached at the end of training.')
    g.add_argument('--margin', type=float, default=0.1, help='Margin of the hinge ranking loss.')
    g.add_argument('--read_workers', type=int, default=8,
                   help='Decode threads of a dataset that streams its images ("-stream" names), at most 16; ignored otherwise (device-side batches).')
    g.add_argument('--queue_size', type=int, default=100,
                   help='Batches a streaming dataset decodes ahead of use, at most 4 (each is a device buffer); ignored otherwise.')
    g.add_argument('--gpus', type=int, default=1, help='Number of GPUs = number of launched processes.')
    g = parser.add_argument_group('Output parameters')
    train_cli.add_output_arguments(g, 'Where to save the embeddings of the test images ({"feat": {i: vec}} pickle).')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.val_batch_size is None:
        args.val_batch_size = args.batch_size

    rank, world, dev = train_cli.init_process(args, 'learn_devise.py')

    # ---- class embeddings and dataset (learn_devise.py:57-65)
    embed_labels, embedding = load_embedding(args.embedding)
    data_generator = train_cli.configure_loader(args, get_data_generator(args.dataset, args.data_root, classes=embed_labels))
    emb_dev = torch.from_numpy(embedding).to(dev).contiguous()

    # ---- model (learn_devise.py:67-74)
    torch.manual_seed(0)   # identical initial weights on every rank
    model = utils.build_network(embedding.shape[1], args.architecture, input_channels=data_generator.num_channels).to(dev)
    if args.init_weights:
        print('Initializing with model {}'.format(args.init_weights))
        head = embedding_layer(model, embedding.shape[1])
        train_cli.load_pretrained(model, args.init_weights, dev)

    losses, metrics = build_losses(emb_dev, args.margin)
    # Keras kernel regulariser of the network folded into the update
    l2_of = {id(p): model.regularizer for p in model.regularized_parameters()} if getattr(model, 'regularizer', 0) else {}

    dp = dict(rank=rank, world_size=world)
    kw = {'embedding': embedding}
    train_seq = lambda: data_generator.train_sequence(args.batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)
    val_seq = lambda: data_generator.test_sequence(args.val_batch_size, batch_transform=transform_inputs, batch_transform_kwargs=kw, **dp)
    trainer = None

    # ---- the linear transformation alone (learn_devise.py:82-99)
    if args.init_weights and args.init_epochs > 0:
        print('Pre-training linear transformation')
        last = {id(p) for p in head.parameters()}
        names = {n for n, p in model.named_parameters() if id(p) in last}
        trainer = train_cli.adagrad_trainer(args, model, losses, metrics, l2_of, args.init_lr, trainable=lambda n: n in names)
        trainer.fit(train_seq(), val_seq(), epochs=args.init_epochs, verbose=not args.no_progress)
        for p in model.parameters():
            p.requires_grad_(True)

    # ---- all layers, from zero accumulators and zero iterations like a model Keras compiles again (learn_devise.py:101-123)
    if args.ft_epochs > 0:
        print('Fine-tuning all layers')
        if trainer is not None:
            trainer.close()        # drop its gradient hooks before the second trainer registers its own
        trainer = train_cli.adagrad_trainer(args, model, losses, metrics, l2_of, args.ft_lr, max_decay=args.max_decay,
                                            num_train=data_generator.num_train, epochs=args.ft_epochs)
        callbacks = [train_cli.JsonLogger(args.log_dir)] if args.log_dir else []
        trainer.fit(train_seq(), val_seq(), epochs=args.ft_epochs, callbacks=callbacks, verbose=not args.no_progress)
    if trainer is None:            # nothing to train: the trainer only evaluates and predicts
        trainer = train_cli.adagrad_trainer(args, model, losses, metrics, l2_of, args.ft_lr)

    # ---- final evaluation (learn_devise.py:125-126)
    final = trainer.evaluate(val_seq())
    if rank == 0:
        print([final['loss'], final['max_sim_acc']])

    # ---- dumps (learn_devise.py:128-144)
    if rank == 0:
        train_cli.dump_model(args, model)
        if args.feature_dump:
            train_cli.dump_features(args.feature_dump, trainer.predict(data_generator.test_sequence(max(args.val_batch_size, 256))))
    train_cli.finish_process(world)
    return final


if __name__ == '__main__':
    main()
