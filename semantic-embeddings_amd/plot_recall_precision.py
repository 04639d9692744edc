"""Drop-in for the reference's ``plot_recall_precision.py`` (same flags, defaults and groups, same label handling): the average
recall-precision curve and the mAP of nearest-neighbour retrieval for each ``--feat`` file, with the ranking and the per-query
metric computed by the MI355X kernels (``recall_precision.recall_precision_device``) instead of a Python loop over N x N lists.

reference: plot_recall_precision.py:19-86.  Differences a user can observe:

* one line per feature file is printed: name, mAP, number of curve levels;
* queries without any other item of their class get AP = 0 and no curve points (the reference adds NaN levels, or raises with
  ``--bins``), with a warning;
* extensions (own argument group): ``--save FILE`` writes the figure instead of showing it (backend from the extension),
  ``--csv FILE`` writes ``feature,level,mean_precision`` rows, ``--kblocks openblas`` reaches the ranking (D > 448);
  ``--gallery_feat FILE`` / ``--gallery_split`` (a group of their own): the matching ``--feat`` file holds queries against that
  gallery, whose relevant items are located by counting instead of by ranking the gallery;
  ``--float64``: float64 ``--feat`` files are ranked in float64 like the reference does (all-pairs only; see evaluate_retrieval.py);
* matplotlib is only imported when a figure is drawn; with ``--csv`` and without matplotlib the figure is skipped.
"""
import argparse
from collections import OrderedDict

from evaluate_retrieval import (_as_feature_matrix, add_float64_flag, add_gallery_flags, check_float64_flag, feat_entry, float64_precision,
                                gallery_arguments, load_labels, str2bool)


def build_parser():
    """Same flags, defaults and grouping as the reference CLI (plot_recall_precision.py:21-32), plus an extension group."""
    p = argparse.ArgumentParser(description='Plots the average recall-precision curve of nearest neighbour search performed on '
                                            'different image embeddings (MI355X kernels).',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    g = p.add_argument_group('Dataset')
    g.add_argument('--dataset', type=str, required=True, help='Dataset name (see datasets.get_data_generator).')
    g.add_argument('--data_root', type=str, required=True, help='Dataset root directory.')
    g.add_argument('--classes_from', type=str, default=None, help='Pickle with an "ind2label" item restricting/ordering the classes.')
    g = p.add_argument_group('Features')
    g.add_argument('--feat', type=str, action='append', required=True, help='Feature pickle {"feat": {image id: vector}}; repeatable.')
    g.add_argument('--label', type=str, action='append', help='Display name for the matching --feat.')
    g.add_argument('--norm', type=str2bool, action='append', help='L2-normalise the matching --feat (cosine ranking); default no.')
    g = p.add_argument_group('Plot')
    g.add_argument('--bins', type=int, default=None, help='Optional, number of recall levels to be distinguished.')
    g = p.add_argument_group('Extensions of this build (not in the reference)')
    g.add_argument('--save', type=str, default=None, help='Write the figure to this file (format from the extension) instead of showing it.')
    g.add_argument('--csv', type=str, default=None, help='Write "feature,level,mean_precision" rows to this file.')
    g.add_argument('--kblocks', type=str, default=None, help="'openblas': restart the fp32 dot-product chain per OpenBLAS K block (D > 448).")
    add_float64_flag(p.add_argument_group('Extensions of this build: float64 feature files (not in the reference)'))
    add_gallery_flags(p.add_argument_group('Extensions of this build: queries against a separate gallery (not in the reference)'))
    return p


def write_csv(curves, csv_file):
    with open(csv_file, 'w') as f:
        f.write('feature,level,mean_precision\n')
        for name, (levels, means, _) in curves.items():
            for lv, m in zip(levels.tolist(), means.tolist()):
                f.write('{},{!r},{!r}\n'.format(name, lv, m))


def plot_curves(curves, save=None):
    import matplotlib
    if save:
        matplotlib.use('Agg')
    import matplotlib.pyplot as plt

    plt.figure()
    plt.xlabel('Recall')
    plt.ylabel('Precision')
    plt.xlim(0, 1)
    plt.ylim(0, 1)
    plt.grid()
    for name, (levels, means, mAP) in curves.items():
        plt.plot(levels, means, label='{} (mAP: {:.2%})'.format(name, mAP))
    plt.legend(fontsize='x-small')
    if save:
        plt.savefig(save)
        plt.close()
    else:
        plt.show()


def main(argv=None):
    """Returns ``{feature name: (levels, mean_precision, mAP)}``."""
    from recall_precision import recall_precision_device

    parser = build_parser()
    args = parser.parse_args(argv)
    check_float64_flag(parser, args)
    if args.bins is not None and args.bins <= 0:
        raise SystemExit('--bins must be positive')
    data_generator, embed_labels, labels_test = load_labels(args)

    curves = OrderedDict()
    for i, feat_dump in enumerate(args.feat):
        feat_name, normalize = feat_entry(args, i)
        features, ind2id, _ = _as_feature_matrix(feat_dump)
        extra = {'precision': 'float64'} if float64_precision(args, features) else {}
        levels, means, mAP, _ = recall_precision_device(features, labels_test, normalize=normalize, bins=args.bins,
                                                        ids=None if ind2id is None else ind2id.tolist(), kblocks=args.kblocks,
                                                        **gallery_arguments(args, i, data_generator, embed_labels), **extra)
        curves[feat_name] = (levels, means, mAP)
        print('{}: mAP {:.4f}, {} levels'.format(feat_name, mAP, len(levels)))
    if args.csv:
        write_csv(curves, args.csv)
    if not args.save:
        try:
            import matplotlib  # noqa: F401
        except ImportError:
            if args.csv:         # the curves are in the CSV: nothing to show without matplotlib
                return curves
            raise
    plot_curves(curves, args.save)
    return curves


if __name__ == '__main__':
    main()
