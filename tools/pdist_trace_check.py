#!/usr/bin/env python
"""Check tests/test_gpu_pdist.py's Python restatement of the distance-kernel dispatch against a kernel trace of that file.

    rocprofv3 --kernel-trace --stats -d <dir> -- python -m pytest tests/test_gpu_pdist.py -q -k "not 50000"
    python tools/pdist_trace_check.py <dir>/<host>/<pid>_results.db

Counts the ``pdist_kernel<METRIC, MULTI_KB, SYM, VEC, EPI_STORE>`` launches the file should make according to ``pdist_dispatch``
(every table case, the two re-runs of each symmetric case, the non-finite cases, the CUB and NABirds workloads) and compares
them, per instantiation, with the launches in the rocpd database.  Exit status 0 when all 24 instantiations appear and every
count matches.
"""
import collections
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "semantic-embeddings_amd")]

import test_gpu_pdist as T  # noqa: E402


def predicted():
    pred = collections.Counter()
    for c in T.CASES:
        metric, mode, q, n, d, kb, layout, _ = c
        t = T.pdist_dispatch(metric, mode, q, n, d, kb, layout)
        pred[t] += 1
        if mode == T.SYM:
            pred[T.pdist_dispatch(metric, T.COPY, q, n, d, kb, layout)] += 1
            pred[T.pdist_dispatch(metric, mode, q, n, d, kb, T.COL1 if t[3] else T.PADDED)] += 1
    for metric in (T.COS, T.EUC, T.DOT):
        for mode in (T.SYM, T.COPY):
            for kb in (None, [64, 36]):
                pred[T.pdist_dispatch(metric, mode, 257, 257, 100, kb, T.CONTIG)] += 1
    for _, n, d, kb in T.WORKLOADS:
        if n != 50000:
            for metric in (T.COS, T.EUC):
                pred[T.pdist_dispatch(metric, T.SYM, n, n, d, kb, T.CONTIG)] += 1
    return pred


def traced(db):
    got = collections.Counter()
    for name, calls in sqlite3.connect(db).execute("select name, total_calls from top_kernels"):
        if "pdist_kernel<" not in name:
            continue
        args = name.split("pdist_kernel<")[1].split(">")[0].split(", ")
        if args[4] == "0":    # EPI_STORE
            got[(int(args[0]), args[1] == "true", args[2] == "true", args[3] == "true")] += calls
    return got


def main():
    pred, got = predicted(), traced(sys.argv[1])
    print("%-8s %-6s %-6s %-6s %10s %10s" % ("metric", "multi", "sym", "vec", "predicted", "traced"))
    for k in sorted(set(pred) | set(got)):
        print("%-8s %-6s %-6s %-6s %10d %10d%s" % (T.METRIC_NAMES[k[0]], k[1], k[2], k[3], pred[k], got[k], "" if pred[k] == got[k] else "  <-"))
    ok = pred == got and len(got) == 24
    print("%d distinct EPI_STORE instantiations traced; launch counts %s" % (len(got), "match" if pred == got else "DIFFER"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
