"""Nearest-class-embedding classification on the MI355X distance + ranking kernels.

Mirrors the pieces of the reference's ``evaluate_classification_accuracy.py`` that sit on the hot path's kernels:

* ``nn_classification`` (evaluate_classification_accuracy.py:51-71): ``cdist(feat, centroids, 'sqeuclidean').argsort(-1)`` --
  here ``se_row_sqnorm`` + ``se_pairwise_dist(SE_METRIC_EUCLID)`` + ``se_rank_rows`` on device-resident features (straight
  from ``Trainer.predict(..., to_host=False)`` or any float32 ``[N, D]`` array).  SciPy evaluates ``sum((x - c)^2)`` in
  float64; the kernels use the canonical float32 arithmetic of the retrieval path (``|x|^2 + |c|^2 - 2 x.c``), so rankings
  agree wherever two class distances differ by more than float32 round-off -- ties and near-ties come back in canonical
  (distance, class index) order.
* ``evaluate`` (evaluate_classification_accuracy.py:88-108): accuracy, top-5 accuracy, class-balanced accuracy and
  hierarchical accuracy ``1 - lcs_height`` of a class ranking / prediction vector.

* ``train_and_predict`` / ``svm_classification`` (evaluate_classification_accuracy.py:20-48): the reference's default mode --
  scale the features, fit a one-vs-rest ``LinearSVC(C)`` and rank the classes by decision score -- on the device
  (``linear_svm.LinearSVC``: the svm.hip kernels; float32 where scikit-learn uses float64).
* ``extract_predictions`` (evaluate_classification_accuracy.py:74-85): the ``--prob_features`` mode, a descending ranking of
  the model output.
* ``main`` / ``__main__``: the reference's command line and result table (``print_performance``), with features extracted on the
  device from a ``--model_dump`` of learn_image_embeddings.py (``torch.save`` of the module).

* ``knn_classification`` / ``--knn K [K ...]`` (an extension of this build; the reference has none): k-nearest-neighbour
  classification of the test images against the training images -- ``se_retrieve_topk`` for the neighbour lists, ``se_knn_vote``
  (knn_vote.hip) for the vote; ties go to the smaller class index, as in scikit-learn's ``KNeighborsClassifier``.

* ``--mistakes K [K ...]`` / ``--crm`` / ``--crm_logits`` (extensions of this build): the columns ``Mistake Severity`` and
  ``Hier. Dist@K`` (``mistakes.mistake_metrics``, in levels of the hierarchy) for every row, and a second row ``"<name> [CRM]"`` for
  every ``--prob_features`` model, decoded from the same outputs by conditional risk minimisation (``mistakes.crm_classification``:
  ``se_tree_risk_topk`` on a class tree, the dense composition on the existing kernels otherwise).

Class rankings of the new modes come from ``se_rank_rows`` on the negated scores: descending score, ties in ascending class
index (the reference's ``argsort(-1)[:, ::-1]`` breaks ties in an unspecified order).
"""
import argparse
import os
import pickle
import sys
from collections import OrderedDict

import numpy as np

METRICS = ['Accuracy', 'Top-5 Accuracy', 'Avg. Accuracy', 'Hierarchical Accuracy']


def nn_classification(features, centroids, return_device=False):
    """Class ranking ``[N, C]`` (nearest class embedding first) of every feature row.

    ``features``: float32 ``[N, D]`` ndarray or device tensor; ``centroids``: ``[C, D]`` array / tensor, a dict with an
    ``'embedding'`` item or the path of such a pickle (evaluate_classification_accuracy.py:55-58)."""
    import pickle
    import torch
    import sehip

    if isinstance(centroids, str):
        with open(centroids, 'rb') as f:
            centroids = pickle.load(f)
    if isinstance(centroids, dict):
        centroids = centroids['embedding']
    sehip._lib.require_gpu()
    dev = torch.device('cuda', torch.cuda.current_device())

    def to_dev(a):
        if torch.is_tensor(a):
            return a.detach().to(device=dev, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    f, c = to_dev(features), to_dev(centroids)
    pd = sehip.pairwise_dist(f, c, metric=sehip.METRIC_EUCLID, sqa=sehip.row_sqnorm(f), sqb=sehip.row_sqnorm(c))
    rank = sehip.rank_rows(pd)
    return rank if return_device else rank.cpu().numpy()


def evaluate(y_pred, data_generator, hierarchy=None, mistakes=None, height_table=None):
    """Flat, top-5, class-balanced and hierarchical accuracy (evaluate_classification_accuracy.py:88-108).
    ``y_pred``: ``[N]`` predicted class indices or an ``[N, >= 1]`` class ranking.
    ``mistakes`` (an extension; needs ``hierarchy``): a list of K -- the keys of ``mistakes.mistake_metrics`` are added, computed
    on ``height_table`` (default: ``hierarchy.height_table(data_generator.classes)``, built on the device)."""
    from train_cli import average_accuracy      # local like every torch import here: train_cli brings torch and the engine along
    perf = OrderedDict()
    y_true = np.asarray(data_generator.labels_test)
    y_pred = y_lists = np.asarray(y_pred)
    if y_pred.ndim == 2:
        perf['Top-5 Accuracy'] = float(np.mean(np.any(y_pred[:, :5] == y_true[:, None], axis=-1)))
        y_pred = y_pred[:, 0]
    hit = (y_pred == y_true)
    perf['Accuracy'] = float(np.mean(hit))
    perf['Avg. Accuracy'] = float(average_accuracy(y_pred, y_true))
    if hierarchy is not None:
        classes = data_generator.classes
        total = 0.0
        for yp, yt in zip(y_pred, y_true):
            total += 1.0 - hierarchy.lcs_height(classes[int(yp)], classes[int(yt)])
        perf['Hierarchical Accuracy'] = total / len(y_true)
    if mistakes:
        from mistakes import mistake_metrics
        if hierarchy is None:
            raise ValueError('the mistake metrics need a hierarchy')
        if height_table is None:
            height_table = hierarchy.height_table(data_generator.classes)
        perf.update(mistake_metrics(y_lists, y_true, height_table, mistakes))
    return perf


# ---------------------------------------------------------------------------------------------------------------------------------
# SVM and prediction modes, feature extraction, command line (evaluate_classification_accuracy.py:20-48, 74-85, 126-188)
# ---------------------------------------------------------------------------------------------------------------------------------

def _device():
    import torch
    import sehip
    sehip._lib.require_gpu()
    return torch.device('cuda', torch.cuda.current_device())


def _as_device_f32(a):
    import torch
    if torch.is_tensor(a):
        return a.detach().to(device=_device(), dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_device())


def _rank_descending(scores):
    """Class ranking [N, C] of device scores, best first: ``se_rank_rows`` of the negated scores (ties: ascending column)."""
    import sehip
    return sehip.rank_rows(-scores).cpu().numpy()


def preprocess_features(X_train, X_test, normalize):
    """The reference's scaling (evaluate_classification_accuracy.py:33-39) on the device, float32: L2-normalised rows with
    ``normalize``, otherwise both sets divided by ``max(1e-8, max |X_train|)`` per column.  Returns two device tensors."""
    import torch
    X_train, X_test = _as_device_f32(X_train), _as_device_f32(X_test)
    if normalize:
        return (X_train / torch.linalg.vector_norm(X_train, dim=-1, keepdim=True),
                X_test / torch.linalg.vector_norm(X_test, dim=-1, keepdim=True))
    X_max = torch.clamp(X_train.abs().amax(dim=0, keepdim=True), min=1e-8)
    return X_train / X_max, X_test / X_max


def svm_classification(X_train, y_train, X_test, normalize=False, C=1.0, tol=1e-4, max_iter=1000, verbose=0, return_model=False):
    """Scale the features, fit ``linear_svm.LinearSVC(C)`` on (X_train, y_train) and rank the classes of every test row by
    decision score, best first (evaluate_classification_accuracy.py:33-48).  Features: NumPy arrays or device tensors.
    The ranking holds column indices of ``classes_`` (= class indices when every class occurs in y_train)."""
    from linear_svm import LinearSVC
    P_train, P_test = preprocess_features(X_train, X_test, normalize)
    sys.stderr.write('Training SVM...\n')
    svm = LinearSVC(C=C, tol=tol, max_iter=max_iter, verbose=verbose).fit(P_train, y_train)
    sys.stderr.write('Predicting and evaluating...\n')
    rank = _rank_descending(svm.decision_function(P_test, return_device=True))
    return (rank, svm) if return_model else rank


def _layer_output(model, layer):
    """A module around ``model`` whose output is one layer's output (forward hook), or the model output.

    ``layer``: None or -1 -> the model output (its first element when the model returns several); another integer i ->
    ``list(model.children())[i]``, the i-th top-level layer (Keras' ``model.layers[i]``); a string -> the module of that name in
    ``model.named_modules()``.  Outputs with more than 2 dimensions are flattened per sample."""
    import torch

    class LayerOutput(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.model, self.out, self.handle = model, None, None
            target = None
            if isinstance(layer, int) and layer != -1:
                target = list(model.children())[layer]
            elif isinstance(layer, str):
                modules = dict(model.named_modules())
                if layer not in modules:
                    raise ValueError('model has no layer named %r' % layer)
                target = modules[layer]
            if target is not None:
                self.handle = target.register_forward_hook(self._hook)

        def _hook(self, mod, inp, out):
            self.out = out

        def forward(self, X):
            out = self.model(X)
            if self.handle is not None:
                out = self.out
            if isinstance(out, (tuple, list)):
                out = out[0]
            return out.flatten(1) if out.dim() > 2 else out

        def close(self):
            if self.handle is not None:
                self.handle.remove()

    return LayerOutput()


def _load_model(model):
    import torch
    if isinstance(model, str):
        model = torch.load(model, map_location=_device(), weights_only=False)
    return model.to(_device())


def extract_features(data, model, layer=None, which='test', batch_size=1, augmentation_epochs=1):
    """Features of the test set (``which='test'``, batches of ``batch_size``, num_test // batch_size of them) or of
    ``augmentation_epochs`` passes over the training set (batches of 10, augmented when augmentation_epochs > 1), as a float32
    device tensor -- ``Trainer.predict(..., to_host=False)`` over the dataset's device sequences."""
    import torch
    from engine import Trainer
    model = _load_model(model)
    wrap = _layer_output(model, layer)
    try:
        trainer = Trainer(wrap, {}, {}, autocast_dtype=None)
        if which == 'test':
            return trainer.predict(data.test_sequence(batch_size, shuffle=False, augment=False), steps=data.num_test // batch_size,
                                   to_host=False)
        parts = [trainer.predict(data.train_sequence(10, shuffle=False, augment=augmentation_epochs > 1),
                                 steps=data.num_train // 10, to_host=False) for _ in range(augmentation_epochs)]
        return torch.cat(parts)
    finally:
        wrap.close()


def train_and_predict(data, model, layer=None, normalize=False, augmentation_epochs=1, C=1.0, custom_objects={}, batch_size=1):
    """Extract train / test features, fit a linear SVM and return the class ranking of every test image, best first
    (evaluate_classification_accuracy.py:20-48).  ``model``: a module or the path of a ``--model_dump``; ``custom_objects`` is
    accepted for the reference's signature and unused."""
    sys.stderr.write('Extracting features...\n')
    X_train = extract_features(data, model, layer, 'train', augmentation_epochs=augmentation_epochs)
    X_test = extract_features(data, model, layer, 'test', batch_size)
    n = (data.num_train // 10) * 10
    y_train = np.tile(np.asarray(data.labels_train)[:n], augmentation_epochs)
    return svm_classification(X_train, y_train, X_test, normalize, C)


def extract_predictions(data, model, layer=None, custom_objects={}, batch_size=1):
    """Class ranking by descending model output (``--prob_features``, evaluate_classification_accuracy.py:74-85)."""
    sys.stderr.write('Predicting and evaluating...\n')
    return _rank_descending(extract_features(data, model, layer, 'test', batch_size))


def extract_outputs(data, model, layer=None, custom_objects={}, batch_size=1):
    """The model outputs of the test set as a float32 device tensor [N, C]: what ``--prob_features`` ranks and ``--crm`` decodes."""
    sys.stderr.write('Predicting and evaluating...\n')
    return extract_features(data, model, layer, 'test', batch_size)


def crm_predictions(outputs, hierarchy, classes, top=5, logits=False):
    """``--crm``: class lists [N, top] of the model ``outputs`` (probabilities; ``logits``: softmax them first, float32) by
    conditional risk minimisation (``mistakes.crm_classification``)."""
    import torch
    from mistakes import crm_classification
    outputs = _as_device_f32(outputs)
    return crm_classification(torch.softmax(outputs, dim=-1) if logits else outputs, hierarchy, classes, top)


def nn_classification_model(data, centroids, model, layer=None, custom_objects={}, batch_size=1):
    """``--centroids`` mode: test features of ``model`` -> ``nn_classification`` (evaluate_classification_accuracy.py:51-71)."""
    sys.stderr.write('Extracting features...\n')
    feat = extract_features(data, model, layer, 'test', batch_size)
    sys.stderr.write('Searching for nearest class centroids...\n')
    return nn_classification(feat, centroids)


# ---------------------------------------------------------------------------------------------------------------------------------
# k-nearest-neighbour classification (an extension of this build: the reference has no k-NN mode)
# ---------------------------------------------------------------------------------------------------------------------------------

def knn_classification(X_train, y_train, X_test=None, ks=(1,), normalize=False, num_classes=None, top=5, kblocks=None, kernels=None,
                       return_votes=False):
    """k-NN classification of the rows of ``X_test`` against the training set: ``{k: class ranking [N, top] (NumPy int32)}``, best
    class first -- most votes among the k nearest training rows, ties in ascending class index (scikit-learn's
    ``KNeighborsClassifier(weights='uniform')`` rule), classes without a vote behind them in ascending index.  ``evaluate`` takes
    every ranking as it is.

    Features: float32 ``[N, D]`` arrays or device tensors.  With ``normalize`` the rows are L2-normalised (``se_normalize_rows``) and
    the metric is cosine, otherwise squared Euclidean on the raw features -- the two metrics of evaluate_retrieval.py, with its
    canonical (distance, index) order among equal distances.  The neighbour lists are ONE fused distance + top-k call
    (``sehip.retrieve_topk`` with ``k = max(ks)``; ``kblocks``: as in ``pairwise_retrieval``, for the reference's BLAS arithmetic
    at D > 448) and the vote is ``sehip.knn_vote`` over them: the N x N_train distances are never written.
    ``X_test=None``: leave-one-out on the training set -- lists of ``max(ks) + 1`` entries from which every row's own index is dropped.
    ``num_classes`` defaults to ``max(y_train) + 1``; ``top`` is capped at it.  ``max(ks)`` (+ 1) above the number of training rows
    or above ``sehip.TOPK_MAX`` raises ``ValueError`` before anything is launched.
    ``return_votes``: also ``{k: vote counts [N, top]}`` of the ranked classes.
    ``kernels`` (tests): CPU stand-ins ``{'retrieve_topk', 'knn_vote', 'normalize_rows_', 'device'}``."""
    import torch
    import sehip
    from evaluate_retrieval import _resolve_kblocks, resolve_kernels
    from recall_precision import to_device_f32
    ks = [int(k) for k in ([ks] if isinstance(ks, (int, np.integer)) else ks)]
    if not ks or min(ks) < 1:
        raise ValueError('ks must hold at least one k >= 1, got {}'.format(ks))
    loo = X_test is None
    n_train, d = int(X_train.shape[0]), int(X_train.shape[1])
    y = np.asarray(y_train)
    if y.shape != (n_train,) or not np.issubdtype(y.dtype, np.integer):
        raise ValueError('y_train must hold one integer class index per training row')
    list_len = max(ks) + (1 if loo else 0)
    if list_len > n_train:
        raise ValueError('k = {} needs {} training rows{}, there are {}'.format(max(ks), list_len, ' (leave-one-out)' if loo else '', n_train))
    if list_len > sehip.TOPK_MAX:
        raise ValueError('k = {}{} exceeds the longest neighbour list of the fused top-k, {}'.format(
            max(ks), ' (+ 1 for leave-one-out)' if loo else '', sehip.TOPK_MAX))
    if not loo and int(X_test.shape[1]) != d:
        raise ValueError('test rows have {} feature dimensions, training rows {}'.format(X_test.shape[1], d))
    C = int(num_classes) if num_classes is not None else int(y.max()) + 1
    top = min(int(top), C)
    if top < 1 or top > sehip.KNN_TOP_MAX:
        raise ValueError('top must lie in [1, {}], got {}'.format(sehip.KNN_TOP_MAX, top))
    kblocks = _resolve_kblocks(kblocks, d)
    kernels = resolve_kernels(kernels, ('retrieve_topk', 'knn_vote', 'normalize_rows_', 'device'))
    dev = kernels['device']
    gallery = to_device_f32(X_train, dev)
    queries = gallery if loo else to_device_f32(X_test, dev)
    if normalize:
        kernels['normalize_rows_'](gallery)
        if queries is not gallery:
            kernels['normalize_rows_'](queries)
    _, lists = kernels['retrieve_topk'](queries, gallery, list_len, metric=sehip.METRIC_COSINE if normalize else sehip.METRIC_EUCLID,
                                        kblocks=kblocks)
    cuts = sorted(set(ks))
    qidx = torch.arange(n_train, dtype=torch.int32, device=dev) if loo else None
    out_cls, out_votes = kernels['knn_vote'](lists, torch.from_numpy(y.astype(np.int32)).to(dev), C, cuts, top=top, qidx=qidx)
    out_cls, out_votes = out_cls.cpu().numpy(), out_votes.cpu().numpy()
    ranks = OrderedDict((k, out_cls[:, cuts.index(k)]) for k in ks)
    if return_votes:
        return ranks, OrderedDict((k, out_votes[:, cuts.index(k)]) for k in ks)
    return ranks


def knn_classification_model(data, model, layer=None, normalize=False, ks=(1,), custom_objects={}, batch_size=1, top=5):
    """``--knn`` mode: train and test features of ``model`` like ``train_and_predict`` extracts them (one un-augmented pass over the
    training set) -> ``knn_classification``: ``{k: class ranking of every test image}`` of ``top`` classes each."""
    sys.stderr.write('Extracting features...\n')
    X_train = extract_features(data, model, layer, 'train')
    X_test = extract_features(data, model, layer, 'test', batch_size)
    n = (data.num_train // 10) * 10
    sys.stderr.write('Searching for nearest training images...\n')
    return knn_classification(X_train, np.asarray(data.labels_train)[:n], X_test, ks, normalize, num_classes=len(data.classes), top=top)


def print_performance(perf, metrics=METRICS):
    """The reference's result table (evaluate_classification_accuracy.py:111-126)."""
    print()
    max_name_len = max(len(lbl) for lbl in perf.keys())
    print(' | '.join([' ' * max_name_len] + ['{:^6s}'.format(metric) for metric in metrics]))
    print('-' * (max_name_len + sum(3 + max(6, len(metric)) for metric in metrics)))
    for lbl, results in perf.items():
        print('{:{}s} | {}'.format(lbl, max_name_len, ' | '.join(
            '{:>{}.4f}'.format(results[metric], max(len(metric), 6)) if metric in results
            else '{:>{}s}'.format('--', max(len(metric), 6)) for metric in metrics)))
    print()


def str2bool(v):
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    elif v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def build_parser():
    import utils
    parser = argparse.ArgumentParser(description='Evaluates flat, balanced, and hierarchical accuracy of several models.',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = parser.add_argument_group('Dataset')
    g.add_argument('--dataset', type=str, required=True, help='Training dataset. See README.md for a list of available datasets.')
    g.add_argument('--data_root', type=str, required=True, help='Root directory of the dataset.')
    g.add_argument('--hierarchy', type=str, default=None, help='Path to a file containing parent-child relationships (one per line). Used for evaluating hierarchical accuracy.')
    g.add_argument('--is_a', action='store_true', default=False, help='If given, --hierarchy is assumed to contain is-a instead of parent-child relationships.')
    g.add_argument('--str_ids', action='store_true', default=False, help='If given, class IDs are treated as strings instead of integers.')
    g.add_argument('--classes_from', type=str, default=None, help='Optionally, a path to a pickle dump containing a dictionary with item "ind2label" specifying the classes to be considered. These should be in the same order as the classes predicted by the model.')
    g.add_argument('--augmentation_epochs', type=int, default=1, help='Number of training image augmentations when training an SVM on top of embeddings.')
    g.add_argument('--C', type=float, default=0.1, help='Weight of the error in SVM loss.')
    g.add_argument('--batch_size', type=int, default=1, help='Batch size for feature extraction. Must divide the number of test images evenly.')
    g = parser.add_argument_group('Features')
    g.add_argument('--architecture', type=str, default='simple', choices=utils.ARCHITECTURES, help='Type of network architecture.')
    g.add_argument('--model', type=str, action='append', required=True, help='Path to a --model_dump of learn_image_embeddings.py (torch.save of the module) used for extracting image features.')
    g.add_argument('--layer', type=str, action='append', required=True, help='Name (in named_modules()) or index (into the top-level children; -1: the model output) of the layer to extract features from.')
    g.add_argument('--label', type=str, action='append', help='Label for the corresponding features.')
    g.add_argument('--norm', type=str2bool, action='append', help='Whether to L2-normalize the corresponding features or not (defaults to False).')
    g.add_argument('--prob_features', type=str2bool, action='append', help='Whether to use the extracted features as class probabilities instead of training an SVM.')
    g.add_argument('--centroids', type=str, action='append', help='Optionally, a pickle dump containing a dictionary with an item "embedding" referring to a numpy array of class centroids for performing nearest-neighbor classification.')
    g = parser.add_argument_group('Extensions of this build (not in the reference)')
    g.add_argument('--knn', type=int, nargs='+', default=None, metavar='K', help='Classify the test images of every --model that is neither --prob_features nor --centroids by a vote among their K nearest training images instead of an SVM; one table row per K. --norm selects the cosine metric, otherwise squared Euclidean distances are used.')
    g.add_argument('--mistakes', type=int, nargs='+', default=None, metavar='K', help='Adds the columns "Mistake Severity" (mean height of the lowest common subsumer of label and prediction over the misclassified images) and "Hier. Dist@K" (mean LCS height between the label and the K best classes) to every row, in levels of the hierarchy. Each K in [1, 32]. Needs --hierarchy.')
    g.add_argument('--crm', action='store_true', default=False, help='Adds a row "<name> [CRM]" for every --prob_features model: the same outputs, taken as class probabilities, decoded by conditional risk minimisation (the class of smallest expected LCS height instead of the most probable one). Needs --hierarchy.')
    g.add_argument('--crm_logits', action='store_true', default=False, help='Like --crm, for models whose output is logits: a softmax is applied first.')
    return parser


MISTAKES_K_MAX = 32         # SE_TREE_RISK_TOP_MAX: the longest list the CRM decoding returns


def _layer_arg(v):
    try:
        return int(v)
    except ValueError:
        return v


def main(argv=None, modes=None):
    """The reference's command line (evaluate_classification_accuracy.py:138-188); returns the table's OrderedDict.
    ``modes`` (tests): a dict overriding 'svm' / 'centroids' / 'prob' / 'knn' with callables of the same signatures; with the
    extension flags also 'probs' (``extract_outputs``), 'rank' (outputs -> descending class ranking), 'crm' (``crm_predictions``) and
    'height_table' (no arguments -> the integer [C, C] table of the classes).
    ``--mistakes`` / ``--crm`` / ``--crm_logits`` (extensions): the module docstring.
    ``--knn K [K ...]`` (an extension): models that would get an SVM are classified by k-NN, one row ``"<name> [k-NN, k=K]"`` per K."""
    from class_hierarchy import ClassHierarchy
    from evaluate_retrieval import load_labels
    parser = build_parser()
    args = parser.parse_args(argv)
    crm = args.crm or args.crm_logits
    if (args.mistakes or crm) and not args.hierarchy:
        parser.error('--mistakes and --crm need --hierarchy')
    if args.mistakes and not all(1 <= k <= MISTAKES_K_MAX for k in args.mistakes):
        parser.error('--mistakes: every K must lie in [1, {}]'.format(MISTAKES_K_MAX))
    top = max([5] + (args.mistakes or []))
    if args.mistakes and args.knn:
        import sehip
        if top > sehip.KNN_TOP_MAX:
            parser.error('--mistakes with --knn: K = {} exceeds the longest class list of the vote, {}'.format(top, sehip.KNN_TOP_MAX))
    data_generator = load_labels(args)[0]
    id_type = str if args.str_ids else int
    hierarchy = ClassHierarchy.from_file(args.hierarchy, is_a_relations=args.is_a, id_type=id_type) if args.hierarchy else None
    run = {'svm': train_and_predict, 'centroids': nn_classification_model, 'prob': extract_predictions, 'knn': knn_classification_model,
           'probs': extract_outputs, 'rank': lambda outputs: _rank_descending(_as_device_f32(outputs)), 'crm': crm_predictions,
           'height_table': lambda: hierarchy.height_table(data_generator.classes)}
    run.update(modes or {})
    extra = {'mistakes': args.mistakes, 'height_table': run['height_table']()} if args.mistakes else {}
    perf = OrderedDict()
    for i, model in enumerate(args.model):
        model_name = args.label[i] if (args.label is not None) and (i < len(args.label)) else os.path.splitext(os.path.basename(model))[0]
        layer = _layer_arg(args.layer[i]) if (args.layer is not None) and (i < len(args.layer)) else None
        normalize = args.norm[i] if (args.norm is not None) and (i < len(args.norm)) else False
        prob_features = args.prob_features[i] if (args.prob_features is not None) and (i < len(args.prob_features)) else False
        centroids = args.centroids[i] if (args.centroids is not None) and (i < len(args.centroids)) else ''
        sys.stderr.write('-- {} --\n'.format(model_name))
        if prob_features and crm:       # one extraction: the ranking and the CRM lists come from the same outputs
            outputs = run['probs'](data_generator, model, layer, {}, args.batch_size)
            perf[model_name] = evaluate(run['rank'](outputs), data_generator, hierarchy, **extra)
            sys.stderr.write('Decoding by conditional risk minimisation...\n')
            pred = run['crm'](outputs, hierarchy, data_generator.classes, min(top, len(data_generator.classes)), args.crm_logits)
            perf['{} [CRM]'.format(model_name)] = evaluate(pred, data_generator, hierarchy, **extra)
            continue
        elif prob_features:
            pred = run['prob'](data_generator, model, layer, {}, args.batch_size)
        elif centroids:
            pred = run['centroids'](data_generator, centroids, model, layer, {}, args.batch_size)
        elif args.knn:
            knn_top = {'top': top} if args.mistakes else {}
            for k, pred in run['knn'](data_generator, model, layer, normalize, args.knn, {}, args.batch_size, **knn_top).items():
                perf['{} [k-NN, k={}]'.format(model_name, k)] = evaluate(pred, data_generator, hierarchy, **extra)
            continue
        else:
            pred = run['svm'](data_generator, model, layer, normalize, args.augmentation_epochs, args.C, {}, args.batch_size)
        perf[model_name] = evaluate(pred, data_generator, hierarchy, **extra)
    if args.mistakes:
        from mistakes import metric_names
        print_performance(perf, METRICS + metric_names(args.mistakes))
    else:
        print_performance(perf)
    return perf


if __name__ == '__main__':
    main()
