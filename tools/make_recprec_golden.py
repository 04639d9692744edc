"""Golden fixtures of the recall-precision curve: tests/golden/recprec_*.npz.

Runs the reference's UNMODIFIED plot_recall_precision.py (through ``runpy.run_path``) on clustered float32 features and records
what it computes: the curve it hands to ``plt.plot`` (levels, mean precision) and every value ``average_precision_score``
returns (the mAP at full precision, not the legend's two decimals).  The reference tree must be present (SE_REFERENCE_ROOT);
the GPU tests read only the .npz files.

Stand-ins, set up around the run and removed afterwards: ``datasets`` (an object with ``labels_test`` / ``num_test``),
``numexpr`` (oracle/ref_import.py), ``np.float = float`` (the name left NumPy in 1.24), the Agg backend with ``plt.plot``
recording and ``plt.show`` doing nothing.

A seed is rejected when any query has an exact distance tie between a relevant and an irrelevant item (then the curve would
depend on the sort's tie order), or when the canonical ranking (oracle/retrieval_oracle.py) does not reproduce the recorded
curve through ``recall_precision.recall_precision_host``.

    python tools/make_recprec_golden.py            # writes tests/golden/recprec_{d24,d100}_{cos,euc}.npz
"""
import os
import pickle
import runpy
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_import  # noqa: E402
from oracle import retrieval_oracle as ro  # noqa: E402

BINS = (0, 10, 7, 1000)           # 0: no --bins
CASES = {                         # name: (N, D, classes, normalize, spread of the class centres)
    "d24_cos": (380, 24, 14, True, 0.9),
    "d24_euc": (420, 24, 17, False, 0.9),
    "d100_cos": (460, 100, 20, True, 0.55),
    "d100_euc": (330, 100, 11, False, 0.55),
}


def clustered(n, d, c, rng, spread):
    """Unequal class sizes (>= 2 each, no singletons), overlapping Gaussian clusters (unit noise, centres N(0, spread^2))."""
    w = rng.uniform(0.3, 1.7, size=c)
    sizes = np.maximum(2, np.floor(w / w.sum() * n).astype(int))
    sizes[0] += n - sizes.sum()
    assert sizes.min() >= 2 and sizes.sum() == n
    labels = rng.permutation(np.repeat(np.arange(c), sizes))
    centers = rng.standard_normal((c, d)) * spread
    feats = centers[labels] + rng.standard_normal((n, d))
    return feats.astype(np.float32), labels


def has_mixed_ties(pd, labels):
    for q in range(len(labels)):
        row = np.delete(pd[q], q)
        rel = np.delete(labels == labels[q], q)
        if np.intersect1d(row[rel], row[~rel]).size:
            return True
    return False


def run_reference(feats, labels, normalize, bins):
    """One run of the reference script; returns (levels, means, aps)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import sklearn.metrics

    rec = {"plot": [], "ap": []}
    ev = ref_import.import_reference("evaluate_retrieval")
    ds = types.ModuleType("datasets")
    ds.get_data_generator = lambda *a, **k: types.SimpleNamespace(labels_test=[int(v) for v in labels], num_test=len(labels))
    ne = ref_import._numexpr_stub()
    orig = {"plot": plt.plot, "show": plt.show, "ap": sklearn.metrics.average_precision_score}

    def plot(x, y, *a, **k):
        rec["plot"].append((np.array(x, dtype=np.float64), np.array(y, dtype=np.float64)))
        return orig["plot"](x, y, *a, **k)

    def ap(*a, **k):
        v = orig["ap"](*a, **k)
        rec["ap"].append(float(v))
        return v

    saved_mods = {k: sys.modules.get(k) for k in ("datasets", "numexpr", "evaluate_retrieval")}
    saved_argv, had_float = list(sys.argv), hasattr(np, "float")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "feat.pickle")
        with open(path, "wb") as f:
            pickle.dump(feats.copy(), f)
        sys.argv = ["plot_recall_precision.py", "--dataset", "stub", "--data_root", tmp, "--feat", path,
                    "--norm", "yes" if normalize else "no"] + (["--bins", str(bins)] if bins else [])
        try:
            sys.modules.update({"datasets": ds, "numexpr": ne, "evaluate_retrieval": ev})
            np.float = float
            plt.plot, plt.show, sklearn.metrics.average_precision_score = plot, (lambda *a, **k: None), ap
            sys.dont_write_bytecode = True
            runpy.run_path(os.path.join(ref_import.REFERENCE_ROOT, "plot_recall_precision.py"), run_name="__main__")
        finally:
            plt.plot, plt.show, sklearn.metrics.average_precision_score = orig["plot"], orig["show"], orig["ap"]
            plt.close("all")
            if not had_float:
                del np.float
            sys.argv = saved_argv
            for k, v in saved_mods.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
    assert len(rec["plot"]) == 1 and len(rec["ap"]) == len(labels)
    return rec["plot"][0][0], rec["plot"][0][1], np.array(rec["ap"])


def make_case(name, n, d, c, normalize, spread, seed0):
    from recall_precision import recall_precision_host
    for seed in range(seed0, seed0 + 50):
        rng = np.random.default_rng(seed)
        feats, labels = clustered(n, d, c, rng, spread)
        pd, rank = ro.canon_retrieval(feats, normalize)
        if has_mixed_ties(pd, labels):
            print("%s: seed %d rejected (relevant / irrelevant distance tie)" % (name, seed))
            continue
        out = {"features": feats, "labels": labels.astype(np.int32), "normalize": np.array(normalize), "seed": np.array(seed),
               "bins": np.array(BINS, dtype=np.int32)}
        ok = True
        for b in BINS:
            levels, means, aps = run_reference(feats, labels, normalize, b)
            hl, hm, hmap, _ = recall_precision_host(rank, labels, bins=b or None)
            if not (np.array_equal(hl, levels) and np.allclose(hm, means, rtol=0, atol=1e-12) and abs(hmap - aps.mean()) <= 1e-12):
                print("%s: seed %d rejected (canonical ranking does not reproduce the reference's curve, bins=%d)" % (name, seed, b))
                ok = False
                break
            out["levels_%d" % b], out["means_%d" % b], out["aps_%d" % b] = levels, means, aps
        if ok:
            path = os.path.join(ROOT, "tests", "golden", "recprec_%s.npz" % name)
            np.savez_compressed(path, **out)
            print("%s: seed %d -> %s (%d bytes)" % (name, seed, path, os.path.getsize(path)))
            return
    raise RuntimeError("no usable seed for " + name)


def main():
    if not ref_import.available():
        raise SystemExit("reference tree not found at " + ref_import.REFERENCE_ROOT)
    ro.build()
    for i, (name, (n, d, c, norm, spread)) in enumerate(CASES.items()):
        make_case(name, n, d, c, norm, spread, 1000 * (i + 1))


if __name__ == "__main__":
    main()
