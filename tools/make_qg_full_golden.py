"""Golden fixture of query-vs-gallery retrieval evaluation over WHOLE rankings: tests/golden/qg_full_ahp.npz.

The problem of tools/make_qg_golden.py (``problem(SEED)`` of that tool: queries [37, 7] against a gallery [301, 7], six CIFAR-100
classes, class 90 absent from the gallery, class 43 with a single member, five query ids that are gallery ids), for a cosine and a
Euclidean configuration.  The fixture holds no features: tests take them from tests/golden/qg_retrieval.npz and this tool asserts
that they are the same arrays.

Expected values: the imported reference's ``ClassHierarchy.hierarchical_precision(rankings, labels, ks=[1, 10, 50, 100],
compute_ahp=True, compute_ap=True, ignore_qids=True)`` on the CIFAR-100 taxonomy (edges of tests/golden/hierarchy_cifar.npz): means
and per-query values of P@k, ``AHP (WUP)`` / ``AHP (LCS_HEIGHT)`` over the whole list (``np.trapz(cumsum(sim) / cum_best,
dx = 1 / len)``, 301 items, or 300 for a query that is a gallery item) and AP.  Rankings: the reference's distance lines and
``np.argsort`` on the rectangular operands; as in make_qg_golden.py the tool asserts that no row has two equal float32 distances
between items of different classes and that the canonical ranking of the canonical arithmetic gives the same values.  Without
scikit-learn the reference's AP line cannot run: AP is then ``(1 / R) sum_j j / p_j`` in float64 NumPy and ``ap_from_numpy`` is set.

    python tools/make_qg_full_golden.py            # writes tests/golden/qg_full_ahp.npz
"""
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_import  # noqa: E402
from oracle import retrieval_oracle as ro  # noqa: E402
import make_qg_golden as base  # noqa: E402


def evaluate(hier, ranking, q_lab, q_ids, g_lab, g_ids, have_sklearn):
    labels = {int(i): int(c) for i, c in zip(g_ids, g_lab)}
    labels.update({int(i): int(c) for i, c in zip(q_ids, q_lab)})
    retrieved = {int(q_ids[i]): g_ids[ranking[i]].tolist() for i in range(len(q_ids))}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        means, per_q = hier.hierarchical_precision(retrieved, labels, ks=base.KS, compute_ahp=True, compute_ap=have_sklearn, ignore_qids=True)
    names = sorted(per_q)
    values = np.array([[per_q[m][int(i)] for i in q_ids] for m in names], dtype=np.float64)
    qidx = np.array([int(i) if i < 1000 else -1 for i in q_ids], dtype=np.int32)
    ap = np.array([base.numpy_ap(ranking[i][ranking[i] != qidx[i]], g_lab == q_lab[i]) for i in range(len(q_ids))])
    if have_sklearn:
        got = np.nan_to_num(values[names.index("AP")], nan=0.0)       # a query without relevant items: 0 (or NaN, by sklearn version)
        assert np.abs(got - ap).max() <= 1e-12, "the reference's AP and (1 / R) sum j / p_j disagree"
        values[names.index("AP")] = got
    else:
        names.append("AP")
        values = np.concatenate([values, ap[None]])
    assert np.isfinite(values).all(), "a metric of the fixture is not finite"
    assert {"AHP (WUP)", "AHP (LCS_HEIGHT)"} <= set(names)
    return {"metric_names": np.array(names), "per_query": values, "means": values.mean(axis=1), "qidx": qidx}


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not found at " + ref_import.REFERENCE_ROOT)
    ro.build()
    try:
        import sklearn.metrics  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
        stub = type(sys)("sklearn.metrics")
        stub.average_precision_score = None
        sys.modules.setdefault("sklearn", type(sys)("sklearn"))
        sys.modules.setdefault("sklearn.metrics", stub)
    ch = ref_import.import_reference("class_hierarchy")
    edges = np.load(os.path.join(ROOT, "tests", "golden", "hierarchy_cifar.npz"))["edges"]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for p, c in edges.tolist():
            f.write("%d %d\n" % (p, c))
    hier = ch.ClassHierarchy.from_file(f.name, id_type=int)
    os.unlink(f.name)

    q_feat, q_lab, q_ids, g_feat, g_lab, g_ids = base.problem(base.SEED)
    clipped = np.load(os.path.join(ROOT, "tests", "golden", "qg_retrieval.npz"))
    assert np.array_equal(clipped["queries"], q_feat) and np.array_equal(clipped["gallery"], g_feat)
    assert np.array_equal(clipped["query_ids"], q_ids) and np.array_equal(clipped["query_labels"], q_lab)
    assert np.array_equal(clipped["gallery_ids"], g_ids) and np.array_equal(clipped["gallery_labels"], g_lab)
    out = {"seed": np.array(base.SEED), "ks": np.array(base.KS), "query_ids": q_ids.astype(np.int64),
           "ap_from_numpy": np.array(not have_sklearn)}
    for name, normalize in (("cosine", True), ("euclid", False)):
        pd = base.reference_distances(q_feat, g_feat, normalize)
        assert pd.dtype == np.float32
        assert not base.mixed_ties(pd, q_lab, g_lab), "%s: seed %d has a distance tie between classes" % (name, base.SEED)
        res = evaluate(hier, np.argsort(pd, axis=-1), q_lab, q_ids, g_lab, g_ids, have_sklearn)
        # the canonical order of the canonical arithmetic gives the same values (what the kernels are held to)
        qn, gn = (ro.canon_normalize_rows(q_feat), ro.canon_normalize_rows(g_feat)) if normalize else (q_feat, g_feat)
        canon = ro.canon_rank_rows(ro.canon_pdist(qn, gn, ro.METRIC_COSINE if normalize else ro.METRIC_EUCLID))
        chk = evaluate(hier, canon, q_lab, q_ids, g_lab, g_ids, have_sklearn)
        assert np.abs(chk["per_query"] - res["per_query"]).max() <= 1e-12, name
        # P@k and AP do not depend on the AHP clip: the same numbers as the clipped fixture holds
        old = dict(zip(clipped[name + "_metric_names"].tolist(), clipped[name + "_per_query"]))
        for m, v in zip(res["metric_names"].tolist(), res["per_query"]):
            if not m.startswith("AHP"):
                assert np.array_equal(v, old[m]), (name, m)
        out.update({"%s_%s" % (name, k): v for k, v in res.items()})
        print("%s: %s" % (name, ", ".join("%s %.4f" % (m, v) for m, v in zip(res["metric_names"], res["means"]))))
    path = os.path.join(ROOT, "tests", "golden", "qg_full_ahp.npz")
    np.savez_compressed(path, **out)
    print("seed %d -> %s (%d bytes)" % (base.SEED, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
