"""Bootstrap confidence intervals and paired tests for per-query retrieval metrics.

The evaluation tools compare methods by the means of per-query metrics; a difference of means says nothing until it is set against
the spread that the choice of queries causes.  Here the queries are resampled with replacement: ``se_bootstrap_means`` (one launch,
no temporaries) gives the means of ``reps`` resampled query sets, percentile intervals come from their quantiles, and two methods
evaluated on the same queries are compared replicate by replicate -- the index stream is pinned by ``(seed, number of queries)``
alone (include/sehip.h), so replicate r of both methods drew the same queries and the differences are paired by construction.

Everything after the kernel is a few quantiles of ``[reps, columns]`` float64 on the host."""
import argparse
import os
from collections import OrderedDict, namedtuple

import numpy as np

Intervals = namedtuple('Intervals', 'mean lo hi rep_means')        # [m], [m], [m], [reps, m] float64 arrays
PairedDifference = namedtuple('PairedDifference', 'delta lo hi p')  # [m] float64 arrays
MetricTable = namedtuple('MetricTable', 'values columns ids')      # device float64 [queries, columns], {metric name: column}, query ids in row order

REP_CHUNK = 4096        # replicates per launch of confidence_intervals (results do not depend on it)


def _quantile_levels(level):
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError('the confidence level must lie strictly between 0 and 1, not {!r}'.format(level))
    return [(1.0 - level) / 2.0, (1.0 + level) / 2.0]


def replicate_means(table, reps, seed=0, chunk=REP_CHUNK):
    """``[reps, m]`` float64 array: the column means of ``reps`` resamples of the rows of ``table`` (float64 device tensor ``[q, m]``),
    ``chunk`` replicates per launch.  A replicate's bits do not depend on the chunking (``se_bootstrap_means``)."""
    import torch
    import sehip
    reps = int(reps)
    if reps < 1:
        raise ValueError('reps must be a positive number of replicates')
    chunk = max(1, int(chunk))
    wide = sehip.BOOTSTRAP_COLS_MAX
    if table.shape[1] > wide:       # more columns than one launch resamples (--ndcg next to the 11 of the table): groups of columns -- the
        groups = [table[:, c0:c0 + wide].contiguous() for c0 in range(0, table.shape[1], wide)]     # index stream depends on (seed, q) only, so
        return np.concatenate([replicate_means(g, reps, seed, chunk) for g in groups], axis=1)        # replicate r draws the same queries in each
    parts = [sehip.bootstrap_means(table, min(chunk, reps - r0), seed=seed, rep0=r0) for r0 in range(0, reps, chunk)]
    return (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu().numpy()


def confidence_intervals(table, reps=10000, level=0.95, seed=0):
    """Percentile bootstrap intervals of the column means of ``table`` (float64 device tensor ``[q, m]``, one row per query):
    ``Intervals(mean, lo, hi, rep_means)`` with ``lo, hi = np.quantile(rep_means, [(1 - level) / 2, (1 + level) / 2], axis=0)``."""
    levels = _quantile_levels(level)
    rep_means = replicate_means(table, reps, seed)
    mean = table.sum(dim=0).cpu().numpy() / table.shape[0]
    lo, hi = np.quantile(rep_means, levels, axis=0)
    return Intervals(mean, lo, hi, rep_means)


def paired_difference(rep_a, rep_b, mean_a, mean_b, level=0.95):
    """Method b against method a on the SAME queries: ``rep_a`` / ``rep_b`` are the replicate means of both from one seed and one
    number of queries, so row r of both resampled the same queries.  Per column: ``delta = mean_b - mean_a``, the percentile interval
    of ``rep_b - rep_a``, and the two-sided p-value ``min(1, 2 min((1 + #{d <= 0}) / (R + 1), (1 + #{d >= 0}) / (R + 1)))``."""
    rep_a, rep_b = np.asarray(rep_a, dtype=np.float64), np.asarray(rep_b, dtype=np.float64)
    if rep_a.shape != rep_b.shape or rep_a.ndim != 2 or rep_a.shape[0] < 1:
        raise ValueError('paired replicates must be two [reps, columns] arrays of one shape, not {} and {}'.format(rep_a.shape, rep_b.shape))
    d = rep_b - rep_a
    R = d.shape[0]
    lo, hi = np.quantile(d, _quantile_levels(level), axis=0)
    le, ge = (d <= 0).sum(axis=0), (d >= 0).sum(axis=0)
    p = np.minimum(1.0, 2.0 * np.minimum((1.0 + le) / (R + 1.0), (1.0 + ge) / (R + 1.0)))
    return PairedDifference(np.asarray(mean_b, dtype=np.float64) - np.asarray(mean_a, dtype=np.float64), lo, hi, p)


# ---- command-line plumbing shared by evaluate_retrieval.py and evaluate_rankings.py ----

def add_bootstrap_flags(group):
    """--bootstrap and its companions: absent from the namespace unless given, so a run without them parses to what it did before."""
    group.add_argument('--bootstrap', type=int, default=argparse.SUPPRESS, metavar='R',
                       help='Resample the queries R times (se_bootstrap_means) and print "mean [lo, hi]" for the columns of the table.')
    group.add_argument('--bootstrap_seed', type=int, default=argparse.SUPPRESS, metavar='S', help='Seed of the pinned index stream (default 0).')
    group.add_argument('--confidence', type=float, default=argparse.SUPPRESS, metavar='P', help='Confidence level of the intervals (default 0.95).')
    group.add_argument('--compare_to', type=str, default=argparse.SUPPRESS, metavar='LABEL',
                       help='With --bootstrap: paired difference of every other entry to this one, "delta [lo, hi] p=..." (same queries required).')
    group.add_argument('--bootstrap_csv', type=str, default=argparse.SUPPRESS, metavar='FILE',
                       help='With --bootstrap: one line per (label, metric) with mean, lo, hi and, when comparing, delta, dlo, dhi, p.')


def check_bootstrap_flags(parser, args, names):
    """The flag combinations --bootstrap refuses; ``names``: the display names of the entries, in order."""
    reps = getattr(args, 'bootstrap', None)
    if reps is None:
        for flag in ('bootstrap_seed', 'confidence', 'compare_to', 'bootstrap_csv'):
            if hasattr(args, flag):
                parser.error('--{} needs --bootstrap R'.format(flag))
        return
    if reps < 1:
        parser.error('--bootstrap takes a positive number of replicates')
    if not 0.0 < getattr(args, 'confidence', 0.95) < 1.0:
        parser.error('--confidence must lie strictly between 0 and 1')
    if not 0 <= getattr(args, 'bootstrap_seed', 0) < (1 << 64):
        parser.error('--bootstrap_seed must be an unsigned 64-bit number')
    if hasattr(args, 'compare_to') and args.compare_to not in names:
        parser.error('--compare_to {!r} is none of the labels {}'.format(args.compare_to, ', '.join(map(repr, names))))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        parser.error('--bootstrap runs in one process on one GPU')


def wanted(args):
    return getattr(args, 'bootstrap', None) is not None


def report(args, tables, metrics):
    """The --bootstrap output of both tools.  ``tables``: ``{name: MetricTable}`` in display order; ``metrics``: the names of the
    printed columns.  Prints the interval table (and the paired one under --compare_to), writes --bootstrap_csv, and returns
    ``(intervals, differences)``: ``{name: Intervals}`` and ``{name: PairedDifference}`` (empty without --compare_to)."""
    level, seed = getattr(args, 'confidence', 0.95), getattr(args, 'bootstrap_seed', 0)
    base = getattr(args, 'compare_to', None)
    if base is not None:
        for name, t in tables.items():
            if list(t.ids) != list(tables[base].ids):
                raise SystemExit('--compare_to {}: {!r} was evaluated on other queries ({} against {}); a paired comparison needs the same '
                                 'query ids in the same order'.format(base, name, len(t.ids), len(tables[base].ids)))
    intervals = OrderedDict()
    for name, t in tables.items():
        cols = [t.columns[m] for m in metrics]
        intervals[name] = confidence_intervals(t.values[:, cols], args.bootstrap, level, seed)
    print_intervals(intervals, metrics, level, args.bootstrap)
    differences = OrderedDict()
    if base is not None:
        a = intervals[base]
        for name, b in intervals.items():
            if name != base:
                differences[name] = paired_difference(a.rep_means, b.rep_means, a.mean, b.mean, level)
        print_differences(differences, metrics, base, level)
    if getattr(args, 'bootstrap_csv', None):
        write_csv(intervals, differences, metrics, args.bootstrap_csv)
    return intervals, differences


def _print_cells(title, rows, metrics):
    """One table: ``rows`` = {name: [cell text per metric]}."""
    name_w = max(map(len, rows))
    col_w = [max([len(m)] + [len(cells[i]) for cells in rows.values()]) for i, m in enumerate(metrics)]
    print(title)
    print(' | '.join([' ' * name_w] + [m.center(w) for m, w in zip(metrics, col_w)]))
    print('-' * (name_w + sum(3 + w for w in col_w)))
    for name, cells in rows.items():
        print(' | '.join([name.ljust(name_w)] + [c.rjust(w) for c, w in zip(cells, col_w)]))
    print()


def format_interval(mean, lo, hi):
    return '{:.4f} [{:.4f}, {:.4f}]'.format(mean, lo, hi)


def format_difference(delta, lo, hi, p):
    return '{:+.4f} [{:+.4f}, {:+.4f}] p={:.4g}'.format(delta, lo, hi, p)


def print_intervals(intervals, metrics, level, reps):
    """Console table ``mean [lo, hi]``: one row per entry, one column per metric."""
    rows = OrderedDict((name, [format_interval(*v) for v in zip(iv.mean, iv.lo, iv.hi)]) for name, iv in intervals.items())
    _print_cells('{:g}% bootstrap intervals over queries ({} replicates)'.format(100 * level, reps), rows, metrics)


def print_differences(differences, metrics, base, level):
    """Console table ``delta [lo, hi] p=...`` of every entry against ``base``."""
    if not differences:
        return
    rows = OrderedDict((name, [format_difference(*v) for v in zip(d.delta, d.lo, d.hi, d.p)]) for name, d in differences.items())
    _print_cells('Paired difference to {} ({:g}% interval, two-sided p)'.format(base, 100 * level), rows, metrics)


def write_csv(intervals, differences, metrics, csv_file):
    """Semicolon-separated, one line per (label, metric): mean, lo, hi and, when comparing, delta, dlo, dhi, p (empty for the entry
    compared to)."""
    paired = bool(differences)
    lines = ['label;metric;mean;lo;hi' + (';delta;dlo;dhi;p' if paired else '')]
    for name, iv in intervals.items():
        d = differences.get(name)
        for i, m in enumerate(metrics):
            cells = [name, m, repr(float(iv.mean[i])), repr(float(iv.lo[i])), repr(float(iv.hi[i]))]
            if paired:
                cells += [repr(float(v[i])) for v in (d.delta, d.lo, d.hi, d.p)] if d is not None else [''] * 4
            lines.append(';'.join(cells))
    with open(csv_file, 'w') as f:
        f.write('\n'.join(lines) + '\n')
