"""Golden fixture of the evaluation of GIVEN, partial rankings: tests/golden/ranked_partial.npz (data only).

Problem: a gallery of 90 items (ids 0 .. 89) in six CIFAR-100 classes, one of them with a single item; 26 queries -- 14 that are
gallery items (their id is a gallery id; some list themselves, some do not) and 12 that are not (ids 1000 ..., one of a class the
gallery lacks).  Every query has a PARTIAL list: 3 to 60 distinct gallery ids in random order.  ``all_ids`` is a shuffled order of
the gallery ids, so the ids a list lacks are appended in that order (class_hierarchy.py:262-264).

Expected values: the imported reference's own ``ClassHierarchy.hierarchical_precision(retrieved, labels, ks=[1, 5, 20, 60],
compute_ahp=A, compute_ap=True, ignore_qids=I, all_ids=all_ids)`` on the CIFAR-100 taxonomy (edges of
tests/golden/hierarchy_cifar.npz) for A in (True, 20) and I in (True, False): per-query values of every metric.  Without
scikit-learn the reference's AP line cannot run: AP is then ``(1 / R) sum_j j / p_j`` in float64 NumPy (0 without a relevant item)
and ``ap_from_numpy`` is set; with it the two are asserted to agree.

    python tools/make_ranked_golden.py            # writes tests/golden/ranked_partial.npz
"""
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_import  # noqa: E402

SEED = 20
KS = [1, 5, 20, 60]
CLASSES = (3, 17, 42, 58, 43, 90)       # 43: a single gallery item; 90: not in the gallery
N_GALLERY, PAD = 90, -1


def problem(seed):
    rng = np.random.default_rng(seed)
    g_ids = np.arange(N_GALLERY, dtype=np.int64)
    g_lab = rng.choice(CLASSES[:4], size=N_GALLERY, p=[0.4, 0.3, 0.2, 0.1]).astype(np.int64)
    g_lab[11] = 43
    inside = rng.choice(N_GALLERY, size=14, replace=False)
    inside[0] = 11
    q_ids = np.concatenate([inside, 1000 + np.arange(12)]).astype(np.int64)
    q_lab = np.concatenate([g_lab[inside], rng.choice(CLASSES[:5], size=12)]).astype(np.int64)
    q_lab[-1] = 90
    lengths = rng.integers(3, 61, size=len(q_ids)).astype(np.int32)
    lists = np.full((len(q_ids), 60), PAD, dtype=np.int64)
    for i, n in enumerate(lengths):
        row = rng.permutation(N_GALLERY)[:n]
        if i < 14 and i % 2 == 0 and q_ids[i] not in row:       # every second inside query lists itself
            row[rng.integers(0, n)] = q_ids[i]
        lists[i, :n] = row
    all_ids = rng.permutation(N_GALLERY).astype(np.int64)
    return g_ids, g_lab, q_ids, q_lab, lists, lengths, all_ids


def numpy_ap(ret, qid, lbl, labels, ignore_qids):
    rel = np.array([labels[r] == lbl for r in ret if (not ignore_qids) or r != qid], dtype=bool)
    hits = np.flatnonzero(rel)
    return float(np.mean(np.arange(1, hits.size + 1) / (hits + 1.0))) if hits.size else 0.0


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not found at " + ref_import.REFERENCE_ROOT)
    try:
        import sklearn.metrics  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
        stub = type(sys)("sklearn.metrics")
        stub.average_precision_score = None
        sys.modules.setdefault("sklearn", type(sys)("sklearn"))
        sys.modules.setdefault("sklearn.metrics", stub)
    if not hasattr(np, "trapz"):        # NumPy 2 renamed the function the reference calls
        np.trapz = np.trapezoid
    ch = ref_import.import_reference("class_hierarchy")
    edges = np.load(os.path.join(ROOT, "tests", "golden", "hierarchy_cifar.npz"))["edges"]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for p, c in edges.tolist():
            f.write("%d %d\n" % (p, c))
    hier = ch.ClassHierarchy.from_file(f.name, id_type=int)
    os.unlink(f.name)

    g_ids, g_lab, q_ids, q_lab, lists, lengths, all_ids = problem(SEED)
    labels = {int(i): int(c) for i, c in zip(g_ids, g_lab)}
    labels.update({int(i): int(c) for i, c in zip(q_ids, q_lab)})
    retrieved = {int(q): lists[i, :lengths[i]].tolist() for i, q in enumerate(q_ids)}
    out = {"seed": np.array(SEED), "ks": np.array(KS), "gallery_ids": g_ids, "gallery_labels": g_lab, "query_ids": q_ids, "query_labels": q_lab,
           "lists": lists, "lengths": lengths, "all_ids": all_ids, "ap_from_numpy": np.array(not have_sklearn)}
    for ahp in (True, 20):
        for ignore in (True, False):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                _, per_q = hier.hierarchical_precision(dict(retrieved), labels, ks=KS, compute_ahp=ahp, compute_ap=have_sklearn,
                                                       ignore_qids=ignore, all_ids=all_ids.tolist())
            names = sorted(per_q)
            values = np.array([[per_q[m][int(i)] for i in q_ids] for m in names], dtype=np.float64)
            ap = []
            for q in q_ids.tolist():
                seen = set(retrieved[q])
                ret = retrieved[q] + [i for i in all_ids.tolist() if i not in seen]
                ap.append(numpy_ap(ret, q, labels[q], labels, ignore))
            ap = np.array(ap)
            if have_sklearn:
                got = np.nan_to_num(values[names.index("AP")], nan=0.0)
                assert np.abs(got - ap).max() <= 1e-12, "the reference's AP and (1 / R) sum j / p_j disagree"
                values[names.index("AP")] = got
            else:
                names.append("AP")
                values = np.concatenate([values, ap[None]])
            assert np.isfinite(values).all(), "a metric of the fixture is not finite"
            key = "ahp%s_ignore%d" % (ahp, ignore)
            out[key + "_metric_names"] = np.array(names)
            out[key + "_per_query"] = values
            print(key, ", ".join("%s %.4f" % (m, v) for m, v in zip(names, values.mean(axis=1))))
    path = os.path.join(ROOT, "tests", "golden", "ranked_partial.npz")
    np.savez_compressed(path, **out)
    print("seed %d -> %s (%d bytes)" % (SEED, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
