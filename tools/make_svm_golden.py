"""Golden fixtures of the linear SVM: tests/golden/svm_*.npz.

CPU only, scikit-learn and NumPy.  Every case stores raw features (X_train, y_train, X_test: multiples of 1/32 held exactly in float16, which keeps the files
small), the penalty C and the
`normalize` flag of the reference's train_and_predict (evaluate_classification_accuracy.py:20-48), and what a float64 solve of the
preprocessed problem gives:

* coef / intercept (float32) / f_opt (float64): the optimum of f_c (linear_svm.py) from the host trust-region Newton solver (linear_svm.fit_host) run
  to a relative gradient norm of 1e-10 (or to float64 resolution: grad_rel records what was reached, at most 1e-9);
* sk_coef / sk_intercept (float32): scikit-learn's LinearSVC(C, dual=False, tol=1e-10, max_iter=100000);
* scores (float32): the test decision scores of the float64 optimum, X_test' coef^T + intercept (X_test' preprocessed).

Generation asserts that scikit-learn's solution and the host optimum agree to 1e-8 relative in every class objective, which also
pins the objective's formula (squared hinge, bias regularised).  Every assertion runs on the float64 results, before they are
rounded for storage.

    python tools/make_svm_golden.py          # writes tests/golden/svm_{gauss_c1,gauss_c01,cifar_norm,cifar_maxabs,absent}.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))

import linear_svm as ls  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def preprocess(X_train, X_test, normalize):
    """The reference's scaling (evaluate_classification_accuracy.py:33-39), in float32 as Keras features are."""
    X_train, X_test = X_train.astype(np.float32).copy(), X_test.astype(np.float32).copy()
    if normalize:
        X_train /= np.linalg.norm(X_train, axis=-1, keepdims=True)
        X_test /= np.linalg.norm(X_test, axis=-1, keepdims=True)
    else:
        X_max = np.abs(X_train).max(axis=0, keepdims=True)
        X_train /= np.maximum(1e-8, X_max)
        X_test /= np.maximum(1e-8, X_max)
    return X_train, X_test


def grid(X):
    """Features on a 1/32 grid, exactly representable in float16 (|x| < 64)."""
    X = np.round(np.asarray(X, dtype=np.float64) * 32.0) / 32.0
    assert np.abs(X).max() < 64.0
    return X.astype(np.float16)


def gauss(seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((10, 24)) * 1.2
    y = rng.integers(0, 10, 2400)
    X = grid(centres[y] + rng.standard_normal((2400, 24)) * 1.5 + 0.7)
    return X[:2000], y[:2000], X[2000:], y[2000:]


def cifar(seed):
    E = np.load(os.path.join(GOLDEN, "embeddings.npz"))["cifar100_unitsphere"]
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 100, 3100)
    X = grid(E[y] + 0.1 * rng.standard_normal((3100, 100)))
    return X[:3000], y[:3000], X[3000:], y[3000:]


def absent(seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((8, 16))
    y = rng.choice(np.array([0, 1, 2, 4, 5, 6, 7]), 1100)          # class 3 never occurs: classes_ is not 0 .. C - 1
    X = grid(centres[y] + rng.standard_normal((1100, 16)))
    y = np.where(y >= 3, y * 10, y)                                   # and the labels are not consecutive either
    return X[:900], y[:900], X[900:], y[900:]


CASES = {   # name: (data, seed, C, normalize)
    "gauss_c1": (gauss, 1, 1.0, False),
    "gauss_c01": (gauss, 1, 0.1, False),
    "cifar_norm": (cifar, 2, 1.0, True),
    "cifar_maxabs": (cifar, 2, 0.1, False),
    "absent": (absent, 3, 1.0, False),
}


def make(name):
    from sklearn.svm import LinearSVC
    data, seed, C, normalize = CASES[name]
    X_train, y_train, X_test, y_test = data(seed)
    P_train, P_test = preprocess(X_train, X_test, normalize)
    classes = np.unique(y_train)
    y_idx = np.searchsorted(classes, y_train)
    Y = ls.signs(y_idx, len(classes))
    W, _, _ = ls.fit_host(P_train, y_idx, len(classes), C=C, tol=1e-10, max_iter=10000)
    g0 = np.linalg.norm(ls.gradient_host(P_train, Y, np.zeros_like(W), C), axis=1)
    grad_rel = np.linalg.norm(ls.gradient_host(P_train, Y, W, C), axis=1) / g0
    assert grad_rel.max() <= 1e-9, (name, grad_rel.max())
    f_opt = ls.objective_host(P_train, Y, W, C)
    sk = LinearSVC(C=C, dual=False, tol=1e-10, max_iter=100000).fit(P_train.astype(np.float64), y_train)
    assert np.array_equal(sk.classes_, classes)
    Wsk = np.hstack([sk.coef_, sk.intercept_[:, None]])
    f_sk = ls.objective_host(P_train, Y, Wsk, C)
    rel = np.abs(f_sk - f_opt) / f_opt
    assert rel.max() <= 1e-8, (name, rel.max())
    scores = P_test.astype(np.float64) @ W[:, :-1].T + W[:, -1]
    out = os.path.join(GOLDEN, "svm_%s.npz" % name)
    np.savez_compressed(out, X_train=X_train, y_train=y_train, X_test=X_test, y_test=y_test, C=C, normalize=normalize,
                        classes=classes, coef=W[:, :-1].astype(np.float32), intercept=W[:, -1].astype(np.float32), f_opt=f_opt,
                        grad_rel=grad_rel, sk_coef=sk.coef_.astype(np.float32), sk_intercept=sk.intercept_.astype(np.float32),
                        scores=scores.astype(np.float32))
    print("%s: N=%d D=%d classes=%d C=%g normalize=%s  |g|/|g0| <= %.1e  sklearn objective rel. diff %.1e  %d bytes" % (
        name, X_train.shape[0], X_train.shape[1], len(classes), C, normalize, grad_rel.max(), rel.max(), os.path.getsize(out)))


if __name__ == "__main__":
    for name in (sys.argv[1:] or CASES):
        make(name)
