"""Hierarchical-precision evaluation of GIVEN rankings: ``evaluate_retrieval.py`` for rankings that come from somewhere else --
another system, an approximate index, re-ranked or truncated lists -- instead of from feature files.

Every ``--ranking FILE`` (repeatable, named by the matching ``--label``) is either

* a pickle of ``{query id: [ranked gallery ids]}``, which is what ``pairwise_retrieval(..., return_generator=False)`` returns, or
* an ``.npz`` with ``query_ids [Q]``, ``ranking [Q, L]`` (integer ids) and optionally ``lengths [Q]`` (the valid entries per row).

Query ids are ids of the test split.  The gallery is the ``--gallery_split`` (default ``test``: a query that is a gallery item is
dropped from its own ranking unless ``--keep_queries``); ids of the ``train`` split are other images whatever their number, so a
gallery id j of that split is ``('train', j)``, the convention of ``evaluate_retrieval.gallery_arguments``: integer ids in a file
are tagged on loading.  Ids missing from a list are appended in the split's index order (``all_ids``; class_hierarchy.py:262-264)
unless ``--no_all_ids``, under which every list must rank the whole gallery.  The lists are scored on the device by
``ClassHierarchy.hierarchical_precision_ranked`` and, with ``--recprec_csv``, ``recall_precision.recall_precision_ranked``; tables,
CSV and plots are those of ``evaluate_retrieval.py``, and so are ``--bootstrap R`` / ``--compare_to LABEL`` (intervals over queries and paired differences between rankings of the same queries;
``bootstrap.py``)."""
import argparse
import os.path
import pickle
from collections import OrderedDict

import numpy as np

import bootstrap
from evaluate_retrieval import METRICS, add_ndcg_flag, load_labels, ndcg_metric_names, plot_performance, print_performance, write_performance


def build_parser():
    p = argparse.ArgumentParser(description='Hierarchical-precision evaluation of given rankings (MI355X kernels).',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = p.add_argument_group('Dataset')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--hierarchy', type=str, required=True, help='Text file with one "<parent> <child>" pair per line.')
    g.add_argument('--is_a', action='store_true', default=False, help='Lines of --hierarchy are "<child> <parent>" instead.')
    g.add_argument('--str_ids', action='store_true', default=False, help='Class IDs are strings (default: integers).')
    g.add_argument('--classes_from', type=str, default=None, help='Pickle with an "ind2label" item restricting/ordering the classes.')
    g = p.add_argument_group('Rankings')
    g.add_argument('--ranking', type=str, action='append', required=True,
                   help='Pickle {query id: [ranked ids]} or .npz with query_ids, ranking and optionally lengths; repeatable.')
    g.add_argument('--label', type=str, action='append', help='Display name for the matching --ranking.')
    g.add_argument('--gallery_split', type=str, default='test', choices=['test', 'train'], help='Dataset split the ranked ids belong to.')
    g.add_argument('--no_all_ids', action='store_true', default=False,
                   help='Do not complete lists with the ids they lack (every list must then rank the whole gallery).')
    g.add_argument('--keep_queries', action='store_true', default=False, help='Keep a query that is a gallery item in its own ranking.')
    g = p.add_argument_group('Output')
    g.add_argument('--plot_max', type=int, default=250, help='Largest k of the precision curve; 0 disables plotting.')
    g.add_argument('--prec_type', type=str, default='LCS_HEIGHT', choices=['WUP', 'LCS_HEIGHT'], help='Class-similarity measure for the curve/CSV.')
    g.add_argument('--clip_ahp', type=int, default=None, help='Compute AHP on the first CLIP_AHP ranks only.')
    g.add_argument('--skip_ap', action='store_true', default=False,
                   help='Do not compute AP; with --clip_ahp only the head of each ranking is needed (long enough lists are not completed).')
    g.add_argument('--csv', type=str, default=None, help='Write the P@k table to this CSV file.')
    g.add_argument('--recprec_csv', type=str, default=None,
                   help='Also compute the recall-precision curve and the mAP; write "ranking,level,mean_precision" rows to this file.')
    g.add_argument('--bins', type=int, default=None, help='Number of recall bins of the recall-precision curve.')
    add_ndcg_flag(g)
    bootstrap.add_bootstrap_flags(p.add_argument_group('Bootstrap over queries'))
    return p


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    bootstrap.check_bootstrap_flags(parser, args, [ranking_entry(args, i) for i in range(len(args.ranking))])
    return args


def ranking_entry(args, i):
    """Display name of the ``i``-th --ranking file: the matching --label, else the file's base name."""
    return args.label[i] if (args.label is not None) and (i < len(args.label)) else os.path.splitext(os.path.basename(args.ranking[i]))[0]


def load_ranking(path):
    """A --ranking file as ``hierarchical_precision_ranked`` takes it: the pickled dict itself, or the array form of an .npz."""
    if path.endswith('.npz'):
        with np.load(path) as z:
            if 'query_ids' not in z or 'ranking' not in z:
                raise ValueError('{}: an .npz ranking holds "query_ids" and "ranking" (and optionally "lengths")'.format(path))
            return (z['query_ids'], z['ranking'], z['lengths'] if 'lengths' in z else None)
    with open(path, 'rb') as f:
        retrieved = pickle.load(f)
    if not isinstance(retrieved, dict):
        raise ValueError('{}: a pickled ranking is a dict {{query id: [ranked ids]}}'.format(path))
    return retrieved


def tag_train_ids(retrieved):
    """Gallery ids of the train split made distinct from the queries' test-split ids: j -> ('train', j); the array form becomes the
    dict form (tuples are no array elements).  Ids that are tagged already stay."""
    def tag(j):
        return j if isinstance(j, tuple) else ('train', j)
    if isinstance(retrieved, tuple):
        q_ids, ranking, lengths = retrieved
        rows = np.asarray(ranking).tolist()
        lengths = [len(r) for r in rows] if lengths is None else np.asarray(lengths).tolist()
        return OrderedDict((q, [tag(j) for j in r[:n]]) for q, r, n in zip(np.asarray(q_ids).tolist(), rows, lengths))
    return OrderedDict((q, [tag(j) for j in r]) for q, r in retrieved.items())


def gallery_of(args, data_generator, embed_labels, labels_test):
    """``(labels, all_ids)``: the mapping id -> class label over queries and gallery, and the gallery split's ids in index order."""
    if args.gallery_split == 'test':
        return labels_test, list(range(len(labels_test)))
    labels_train = data_generator.labels_train
    if embed_labels is not None:
        labels_train = [embed_labels[lbl] for lbl in labels_train]
    labels = {i: lbl for i, lbl in enumerate(labels_test)}
    labels.update({('train', j): lbl for j, lbl in enumerate(labels_train)})
    return labels, [('train', j) for j in range(len(labels_train))]


def write_recprec_csv(curves, csv_file):
    with open(csv_file, 'w') as f:
        f.write('ranking,level,mean_precision\n')
        for name, (levels, means, _) in curves.items():
            for lv, m in zip(levels.tolist(), means.tolist()):
                f.write('{},{!r},{!r}\n'.format(name, lv, m))


def main(argv=None):
    """Returns ``{ranking name: means}`` (with ``--recprec_csv``: plus an ``'mAP'`` entry per ranking)."""
    from class_hierarchy import ClassHierarchy
    from recall_precision import recall_precision_ranked

    args = parse_args(argv)
    data_generator, embed_labels, labels_test = load_labels(args)
    hierarchy = ClassHierarchy.from_file(args.hierarchy, is_a_relations=args.is_a, id_type=str if args.str_ids else int)
    labels, all_ids = gallery_of(args, data_generator, embed_labels, labels_test)

    ks = list(range(1, args.plot_max + 1))
    for k in [1, 10, 50, 100]:
        if (len(ks) == 0) or (ks[-1] < k):
            ks.append(k)
    perf, curves, tables = OrderedDict(), OrderedDict(), OrderedDict()     # tables: the per-query rows on the device, under --bootstrap only
    for i, path in enumerate(args.ranking):
        name = ranking_entry(args, i)
        retrieved = load_ranking(path)
        if args.gallery_split == 'train':
            retrieved = tag_train_ids(retrieved)
        common = dict(ignore_qids=not args.keep_queries, all_ids=None if args.no_all_ids else all_ids)
        ndcg_kw = {'ndcg': args.ndcg} if getattr(args, 'ndcg', None) else {}
        perf[name], rows = hierarchy.hierarchical_precision_ranked(retrieved, labels, ks, compute_ahp=args.clip_ahp if args.clip_ahp else True,
                                                                   compute_ap=not args.skip_ap,
                                                                   per_query='table' if bootstrap.wanted(args) else False, **common, **ndcg_kw)
        if rows is not None:
            tables[name] = rows
        if args.recprec_csv:
            levels, means, mAP, _ = recall_precision_ranked(retrieved, labels, bins=args.bins, **common)
            curves[name] = (levels, means, mAP)
            perf[name]['mAP'] = mAP
            print('{}: mAP {:.4f}, {} levels'.format(name, mAP, len(levels)))

    metrics = list(METRICS)
    if args.skip_ap:
        metrics.remove('AP')
    if args.clip_ahp:
        metrics[4] = 'AHP@{} (WUP)'.format(args.clip_ahp)
        metrics[9] = 'AHP@{} (LCS_HEIGHT)'.format(args.clip_ahp)
    metrics += ndcg_metric_names(getattr(args, 'ndcg', None))
    print_performance(perf, metrics)
    if tables:
        bootstrap.report(args, tables, metrics)
    if args.csv:
        write_performance(perf, args.csv, args.prec_type)
    if args.recprec_csv:
        write_recprec_csv(curves, args.recprec_csv)
    if args.plot_max > 0:
        plot_performance(perf, args.plot_max, args.prec_type, args.clip_ahp)
    return perf


if __name__ == '__main__':
    main()
