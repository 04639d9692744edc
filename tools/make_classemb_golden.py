"""Hierarchy fixtures of the class-embedding kernels (classemb.hip): tests/golden/hierarchy_inat2018.npz and
tests/golden/hierarchy_wordnet_dag.npz.

Dev machine only: reads the hierarchy files of a semantic-embeddings checkout (``--src``, default ``$SE_REFERENCE``) and stores
their edges as data, so that no test reads that checkout at run time.

* hierarchy_inat2018.npz  ``edges`` [14,035, 2] (parent, child) of iNaturalist-Hierarchy/hierarchy_inat.txt (string ids; the
  leaves are the 8,142 species '0' .. '8141') and ``classes``: the leaves in integer order;
* hierarchy_wordnet_dag.npz  the edges of ILSVRC/wordnet.parent-child.pruned.txt whose child lies in the ancestor closure of the
  1,000 ILSVRC classes (``classes``, in the order of ILSVRC/imagenet_class_index.json): a real DAG (synsets with several
  hypernyms), whose lcs needs the depth / height / repr tie-break.

    python tools/make_classemb_golden.py --src /path/to/semantic-embeddings
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def read_edges(path):
    with open(path) as f:
        return [tuple(line.split()[:2]) for line in f if line.strip()]


def closure_edges(edges, classes):
    """Edges (parent, child) whose child is one of ``classes`` or an ancestor of one: the whole DAG above the classes."""
    parents = {}
    for p, c in edges:
        parents.setdefault(c, []).append(p)
    seen, stack = set(classes), list(classes)
    while stack:
        for p in parents.get(stack.pop(), ()):
            if p not in seen:
                seen.add(p)
                stack.append(p)
    return [(p, c) for p, c in edges if c in seen], seen


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--src", default=os.environ.get("SE_REFERENCE"), help="semantic-embeddings checkout with the hierarchy files")
    args = ap.parse_args()
    if not args.src:
        sys.exit("--src (or SE_REFERENCE) is required")

    inat = read_edges(os.path.join(args.src, "iNaturalist-Hierarchy", "hierarchy_inat.txt"))
    kids = {p for p, _ in inat}
    leaves = sorted({c for _, c in inat} - kids, key=int)
    assert len(inat) == 14035 and len(leaves) == 8142 and leaves == [str(i) for i in range(8142)]
    np.savez_compressed(os.path.join(GOLDEN, "hierarchy_inat2018.npz"), edges=np.array(inat), classes=np.array(leaves))

    with open(os.path.join(args.src, "ILSVRC", "imagenet_class_index.json")) as f:
        idx = json.load(f)
    classes = [idx[str(i)][0] for i in range(len(idx))]
    dag, nodes = closure_edges(read_edges(os.path.join(args.src, "ILSVRC", "wordnet.parent-child.pruned.txt")), classes)
    multi = sum(1 for c in {c for _, c in dag} if sum(1 for _, x in dag if x == c) > 1) if len(dag) < 5000 else None
    np.savez_compressed(os.path.join(GOLDEN, "hierarchy_wordnet_dag.npz"), edges=np.array(dag), classes=np.array(classes))
    print("inat2018: %d edges, %d classes; wordnet DAG: %d edges, %d nodes, %s nodes with several parents"
          % (len(inat), len(leaves), len(dag), len(nodes), multi))


if __name__ == "__main__":
    main()
