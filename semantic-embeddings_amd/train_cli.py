"""What the training command lines (learn_image_embeddings.py, learn_center_loss.py, learn_classifier.py, learn_devise.py,
learn_labelembedding.py) have in common: the shared
flag runs, the process group, loading weights, the ``--finetune_init`` warm-up, the main fit and the dumps.  Plain functions that
each script's ``main()`` calls in order; the model, the losses and what the feature dump holds stay in the scripts."""
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

import utils
from engine import Trainer, backbone_mode


# ---------------------------------------------------------------- flags (utils.py:402-418 of the reference and each script's own list)

def add_schedule_arguments(g):
    g.add_argument('--lr_schedule', type=str, default='SGDR', choices=utils.LR_SCHEDULES, help='Learning-rate schedule.')
    g.add_argument('--clipgrad', type=float, default=10.0, help='Global gradient-norm clip.')
    g.add_argument('--max_decay', type=float, default=0.0, help='Learning-rate decay reached at the end of training.')
    g.add_argument('--nesterov', action='store_true', default=False, help='Nesterov momentum.')
    g.add_argument('--epochs', type=int, default=None, help='Number of training epochs.')
    g.add_argument('--batch_size', type=int, default=100, help='Global batch size.')
    g.add_argument('--val_batch_size', type=int, default=None, help='Validation batch size.')


def add_snapshot_arguments(g):
    g.add_argument('--snapshot', type=str, default=None, help='Checkpoint written after every epoch; resumed from if present.')
    g.add_argument('--snapshot_best', type=str, nargs='?', default=None, const='val_loss', help='Only keep the best checkpoint w.r.t. this metric.')
    g.add_argument('--initial_epoch', type=int, default=0, help='First epoch when resuming.')


def add_finetune_and_device_arguments(g, finetune_init, finetune_init_help):
    g.add_argument('--finetune', type=str, default=None, help='state_dict with pre-trained weights (matched by name, mismatches skipped).')
    g.add_argument('--finetune_init', type=int, default=finetune_init, help=finetune_init_help)
    g.add_argument('--gpus', type=int, default=1, help='Number of GPUs = number of launched processes.')
    g.add_argument('--read_workers', type=int, default=8,
                   help='Decode threads of a dataset that streams its images ("-stream" names), at most 16; ignored otherwise (device-side batches).')
    g.add_argument('--queue_size', type=int, default=100,
                   help='Batches a streaming dataset decodes ahead of use, at most 4 (each is a device buffer); ignored otherwise.')
    g.add_argument('--gpu_merge', action='store_true', default=False, help='Ignored (weights always live on the GPUs).')


def add_output_arguments(g, feature_dump_help):
    g.add_argument('--model_dump', type=str, default=None, help='Where to save the whole model (torch.save of the module).')
    g.add_argument('--weight_dump', type=str, default=None, help='Where to save the state_dict.')
    g.add_argument('--feature_dump', type=str, default=None, help=feature_dump_help)
    g.add_argument('--log_dir', type=str, default=None, help='Directory for a JSON-lines training log.')
    g.add_argument('--no_progress', action='store_true', default=False, help='Only print the final performance.')


def read_class_list(path):
    """``--class_list`` (reference: learn_classifier.py:71-79, learn_center_loss.py:102-108): the first word of every non-empty
    line, first occurrence wins, integers if ALL convert."""
    with open(path) as class_file:
        class_list = list(OrderedDict((l.strip().split()[0], None) for l in class_file if l.strip() != '').keys())
    try:
        return [int(lbl) for lbl in class_list]
    except ValueError:
        return class_list


def configure_loader(args, data_generator):
    """``--read_workers`` / ``--queue_size`` for a generator that may stream its images (datasets/files.py, ``store`` other than
    'resident'): the decode threads, at most 16, and the batches of look-ahead, at most 4 because every slot of the ring is device
    memory.  Every other generator composes its batches from device-resident data and has nothing to configure."""
    if getattr(data_generator, 'store', 'resident') != 'resident':
        data_generator.decode_threads = max(1, min(int(args.read_workers), 16))
        data_generator.prefetch_batches = max(0, min(int(args.queue_size), 4))
    return data_generator


# ---------------------------------------------------------------- process group: one process per GPU over RCCL

def init_process(args, script):
    """``(rank, world, device)`` of this process as torchrun launched it."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if not torch.cuda.is_available():
        raise RuntimeError('{} needs a ROCm GPU (no CPU fallback for the HIP loss kernels)'.format(script))
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', rank=rank, world_size=world)
    if args.gpus != world and rank == 0:
        print('note: --gpus {} but {} process(es) were launched; using {}'.format(args.gpus, world, world))
    return rank, world, torch.device('cuda', torch.cuda.current_device())


def finish_process(world):
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ---------------------------------------------------------------- model

def output_width(embed_model, num_channels, dev):
    """Output width of the embedding model (not every architecture ends in a Dense layer)."""
    with torch.no_grad():
        was = embed_model.training
        embed_model.eval()
        width = int(embed_model(torch.zeros((1, num_channels, 32, 32), device=dev)).shape[-1])
        embed_model.train(was)
    return width


def resume_from_snapshot(model, snapshot, dev):
    if snapshot and os.path.exists(snapshot):
        print('Resuming from snapshot {}'.format(snapshot))
        model.load_state_dict(torch.load(snapshot, map_location=dev)['model'])


def load_pretrained(model, path, dev):
    """``--finetune`` / ``--init_weights``: every tensor of the file whose name and shape the model has too.  The file is a
    ``state_dict`` (``--weight_dump``), a snapshot, or a whole module as ``--model_dump`` writes it (unpickled, so only from a trusted
    source -- like ``evaluate_classification_accuracy.py --model``)."""
    print('Loading pre-trained weights from {}'.format(path))
    try:
        state = torch.load(path, map_location=dev)
    except pickle.UnpicklingError:          # no plain tensor file: a pickled module
        state = torch.load(path, map_location=dev, weights_only=False)
    state = state.state_dict() if isinstance(state, torch.nn.Module) else state.get('model', state)
    own = model.state_dict()
    model.load_state_dict({k: v for k, v in state.items() if k in own and own[k].shape == v.shape}, strict=False)


# ---------------------------------------------------------------- training

def _trainer(args, model, losses, metrics, l2_of, **kw):
    mode = backbone_mode(args.architecture)       # (autocast dtype, memory format) of the PyTorch-ROCm backbone
    # SE_FUSED_SGD=1: the fused clip + update kernels (engine.Trainer(fused_sgd=True)); the default stays the torch composition
    return Trainer(model, losses, metrics, lr=args.sgd_lr, momentum=0.9, nesterov=args.nesterov, clipnorm=args.clipgrad,
                   l2_of=l2_of, autocast_dtype=mode[0], memory_format=mode[1], fused_sgd=os.environ.get('SE_FUSED_SGD') == '1', **kw)


def max_decay_rate(max_decay, num_train, batch_size, epochs):
    """Keras' ``decay`` that brings ``lr / (1 + decay * iterations)`` down to ``max_decay * lr`` at the last step of ``epochs`` epochs
    (learn_devise.py:109-112, the formula every trainer of the reference uses); 0 for ``max_decay <= 0``."""
    return (1.0 / max_decay - 1) / ((num_train // batch_size) * epochs) if max_decay > 0 else 0.0


def adagrad_trainer(args, model, losses, metrics, l2_of, lr, max_decay=0.0, num_train=None, epochs=None, **kw):
    """A trainer like ``keras.optimizers.Adagrad(lr=lr, decay=...)`` compiles (learn_devise.py:87,114): constant ``lr`` apart from
    the ``max_decay`` decay over ``epochs`` epochs of ``num_train`` images, no gradient clipping, zero accumulators and zero
    iterations -- what Keras starts from whenever a model is compiled again."""
    mode = backbone_mode(args.architecture)
    decay = max_decay_rate(max_decay, num_train, args.batch_size, epochs)
    return Trainer(model, losses, metrics, lr=lr, decay=decay, clipnorm=None, l2_of=l2_of, autocast_dtype=mode[0],
                   memory_format=mode[1], optimizer='adagrad', **kw)


def warm_up(args, model, losses, metrics, l2_of, train_seq, val_seq, trainable, message, **trainer_kw):
    """``--finetune_init`` epochs on the parameters ``trainable(name)`` picks; afterwards every parameter of the model trains."""
    print(message)
    pre = _trainer(args, model, losses, metrics, l2_of, trainable=trainable, **trainer_kw)
    pre.fit(train_seq(), val_seq(), epochs=args.finetune_init, verbose=not args.no_progress)
    pre.close()            # drop its gradient hooks before the second trainer registers its own
    for p in model.parameters():
        p.requires_grad_(True)
    print('Full model training')


class JsonLogger(utils.Callback):
    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, 'training_log.jsonl')
        open(self.path, 'w').close()

    def on_epoch_end(self, trainer, epoch, logs):
        if trainer.is_main_process:
            with open(self.path, 'a') as f:
                f.write(json.dumps(dict(logs, epoch=epoch + 1)) + '\n')


def fit(args, model, losses, metrics, l2_of, data_generator, train_seq, val_seq, world, **trainer_kw):
    """The main training run under ``--lr_schedule``; returns its trainer.  ``--snapshot`` / ``--initial_epoch`` apply to the
    scripts whose parser has them; ``trainer_kw`` goes to the ``Trainer`` as it is."""
    sched_args = {k: v for k, v in vars(args).items() if v is not None}
    callbacks, num_epochs = utils.get_lr_schedule(args.lr_schedule, data_generator.num_train, args.batch_size, schedule_args=sched_args)
    epochs = args.epochs if args.epochs else num_epochs
    if args.log_dir:
        callbacks.append(JsonLogger(args.log_dir))
    if getattr(args, 'snapshot', None):
        ck = {'save_best_only': True, 'monitor': args.snapshot_best} if args.snapshot_best else {}
        callbacks.append(utils.ModelCheckpoint(args.snapshot, **ck) if world <= 1 else utils.TemplateModelCheckpoint(model, args.snapshot, **ck))
    decay = max_decay_rate(args.max_decay, data_generator.num_train, args.batch_size, epochs)
    trainer = _trainer(args, model, losses, metrics, l2_of, decay=decay, **trainer_kw)
    trainer.fit(train_seq(), val_seq(), epochs=epochs, initial_epoch=getattr(args, 'initial_epoch', 0), callbacks=callbacks,
                verbose=not args.no_progress)
    return trainer


# ---------------------------------------------------------------- results

def average_accuracy(pred, labels):
    """Class-balanced accuracy of the predicted class indices ``pred`` [N]: the mean over the classes of each class's accuracy."""
    labels = np.asarray(labels)
    freq = np.bincount(labels)
    return ((np.asarray(pred) == labels).astype(np.float64) / freq[labels]).sum() / len(freq)


def dump_model(args, model):
    if args.weight_dump:
        torch.save(model.state_dict(), args.weight_dump)
    if args.model_dump:
        torch.save(model, args.model_dump)


def dump_features(path, feats):
    with open(path, 'wb') as f:
        pickle.dump({'feat': dict(enumerate(feats))}, f)
