"""Linear SVM, host side: the float64 statement of LinearSVC's objective (linear_svm.py) against finite differences and the golden
optima, the batched trust-region solver on it, argument validation of the svm.hip entry points, and the command line of
evaluate_classification_accuracy.py with CPU stand-ins for the device modes."""
import ctypes
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "svm_*.npz")))


def _scaled(g):
    X_train, X_test = g["X_train"].astype(np.float32).copy(), g["X_test"].astype(np.float32).copy()
    if bool(g["normalize"]):
        X_train /= np.linalg.norm(X_train, axis=-1, keepdims=True)
        X_test /= np.linalg.norm(X_test, axis=-1, keepdims=True)
    else:
        mx = np.maximum(1e-8, np.abs(X_train).max(axis=0, keepdims=True))
        X_train /= mx
        X_test /= mx
    return X_train, X_test


def test_fixtures_present():
    names = {os.path.basename(p) for p in FIXTURES}
    assert {"svm_gauss_c1.npz", "svm_gauss_c01.npz", "svm_cifar_norm.npz", "svm_cifar_maxabs.npz", "svm_absent.npz"} <= names


def test_objective_gradient_hessian_match_finite_differences():
    import linear_svm as ls
    rng = np.random.default_rng(0)
    n, d, c, C = 60, 5, 4, 0.7
    X = rng.standard_normal((n, d))
    Y = ls.signs(rng.integers(0, c, n), c)
    W = rng.standard_normal((c, d + 1)) * 0.3
    f = ls.objective_host(X, Y, W, C)
    G = ls.gradient_host(X, Y, W, C)
    h = 1e-6
    for j in range(d + 1):
        E = np.zeros_like(W)
        E[:, j] = h
        fd = (ls.objective_host(X, Y, W + E, C) - ls.objective_host(X, Y, W - E, C)) / (2 * h)
        assert np.allclose(fd, G[:, j], rtol=1e-6, atol=1e-6)
    # generalised Hessian: the directional derivative of the gradient where the active set does not change
    V = rng.standard_normal((c, d + 1))
    t = 1e-7
    fd = (ls.gradient_host(X, Y, W + t * V, C) - ls.gradient_host(X, Y, W - t * V, C)) / (2 * t)
    assert np.allclose(fd, ls.hessian_vector_host(X, Y, W, V, C), rtol=1e-5, atol=1e-5)
    assert np.all(np.isfinite(f)) and f.shape == (c,)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_host_solver_reproduces_the_fixture_optimum(path):
    import linear_svm as ls
    g = np.load(path)
    C = float(g["C"])
    P_train, P_test = _scaled(g)
    classes = np.unique(g["y_train"])
    assert np.array_equal(classes, g["classes"])
    y_idx = np.searchsorted(classes, g["y_train"])
    W, n_iter, _ = ls.fit_host(P_train, y_idx, len(classes), C=C, tol=1e-8)
    Y = ls.signs(y_idx, len(classes))
    f = ls.objective_host(P_train, Y, W, C)
    assert np.all(np.abs(f - g["f_opt"]) <= 1e-9 * g["f_opt"])
    Wopt = np.hstack([g["coef"], g["intercept"][:, None]])
    assert np.allclose(W, Wopt, rtol=1e-4, atol=1e-5)
    # the optimum is scikit-learn's (checked to 1e-8 at generation) and the fixture's scores are its decision values
    Wsk = np.hstack([g["sk_coef"], g["sk_intercept"][:, None]])
    assert np.all(np.abs(ls.objective_host(P_train, Y, Wsk, C) - g["f_opt"]) <= 1e-8 * g["f_opt"])
    # (coef, intercept and scores are stored in float32)
    assert np.allclose(P_test.astype(np.float64) @ g["coef"].T + g["intercept"], g["scores"], rtol=1e-5, atol=1e-5)
    assert np.all(n_iter >= 1)


def test_solver_compacts_the_working_set_and_pads_it_to_three_rows():
    """Classes that converge early leave the working set; the last live ones run with finished rows as padding, unchanged."""
    import linear_svm as ls
    rng = np.random.default_rng(3)
    n, d, c = 400, 6, 5
    y = rng.integers(0, c, n)
    X = rng.standard_normal((n, d)) + 4.0 * (y[:, None] == np.arange(d)[None, :] % c)
    calls = []

    class Spy(ls._HostOps):
        def set_columns(self, cols):
            calls.append(np.array(cols))
            super().set_columns(cols)

    ops = Spy(X, y, 1.0, c)
    W, n_iter, conv = ls._tron(ops, c, 1e-9, 1000)
    assert conv.all()
    assert len(calls) >= 2 and all(len(cc) >= 3 for cc in calls)
    assert len(set(n_iter.tolist())) > 1
    Y = ls.signs(y, c)
    g0 = np.linalg.norm(ls.gradient_host(X, Y, 0 * W, 1.0), axis=1)
    assert np.all(np.linalg.norm(ls.gradient_host(X, Y, W, 1.0), axis=1) <= 1e-9 * g0 * 1.0001)


def test_linear_svc_parameter_checks_without_gpu():
    import linear_svm as ls
    for kw in ({"penalty": "l1"}, {"loss": "hinge"}, {"multi_class": "crammer_singer"}, {"fit_intercept": False},
               {"intercept_scaling": 2}, {"class_weight": "balanced"}):
        with pytest.raises(NotImplementedError):
            ls.LinearSVC(**kw)
    with pytest.raises(ValueError):
        ls.LinearSVC(C=0.0)
    with pytest.raises(ValueError):          # binary problems: refused before any device work
        ls.LinearSVC().fit(np.zeros((4, 2), np.float32), np.array([0, 1, 0, 1]))


def test_argument_validation_without_gpu():
    """Every svm.hip entry point rejects bad arguments before it touches a device."""
    import sehip
    lib = sehip.lib()
    z = ctypes.c_void_p(0)
    p = ctypes.c_void_p(256)
    GRAD, HV, SCORE = sehip.SVM_GRAD, sehip.SVM_HV, sehip.SVM_SCORE
    ok = dict(mode=GRAD, x=p, ldx=8, n=100, d=8, w=p, ldw=9, c=5, labels=p, col=p, cpen=1.0, mask=p, ldm=1, out=p, ldo=5, loss=p, ldl=2)

    def margin(**kw):
        a = dict(ok, **kw)
        return lib.se_svm_margin(a["mode"], a["x"], a["ldx"], a["n"], a["d"], a["w"], a["ldw"], a["c"], a["labels"], a["col"],
                                 a["cpen"], a["mask"], a["ldm"], a["out"], a["ldo"], a["loss"], a["ldl"], None)

    for bad in ({"mode": 7}, {"c": 2}, {"c": 0}, {"n": 0}, {"d": 0}, {"x": z}, {"w": z}, {"out": z}, {"labels": z}, {"col": z},
                {"mask": z}, {"loss": z}, {"ldx": 7}, {"ldw": 8}, {"ldo": 4}, {"ldm": 0}, {"ldl": 1}, {"cpen": 0.0},
                {"cpen": float("nan")}):
        assert margin(**bad) == -1, bad
    assert margin(mode=HV, c=40, ldo=40, ldm=1) == -1                  # 40 columns need 2 mask words
    assert margin(mode=HV, mask=z) == -1
    assert margin(mode=SCORE, labels=z, col=z, mask=z, loss=z, ldm=0, ldl=0, c=2) == -1
    assert lib.se_svm_loss_blocks(1) == 1 and lib.se_svm_loss_blocks(64) == 1 and lib.se_svm_loss_blocks(65) == 2

    need = lib.se_svm_reduce_workspace_bytes(10000, 8, 5)
    assert need > 0 and need % 4 == 0
    assert lib.se_svm_reduce_workspace_bytes(10 ** 6, 100, 100) <= (10 ** 6 // 256 + 1) * 100 * 101 * 4

    def reduce(**kw):
        a = dict(z=p, ldz=5, x=p, ldx=8, n=10000, d=8, c=5, plus=p, ldp=9, g=p, ldg=9, ws=p, wsb=need)
        a.update(kw)
        return lib.se_svm_reduce(a["z"], a["ldz"], a["x"], a["ldx"], a["n"], a["d"], a["c"], a["plus"], a["ldp"], a["g"], a["ldg"],
                                 a["ws"], a["wsb"], None)

    for bad in ({"c": 2}, {"n": 0}, {"d": 0}, {"z": z}, {"x": z}, {"g": z}, {"ws": z}, {"ldz": 4}, {"ldx": 7}, {"ldg": 8},
                {"ldp": 8}):
        assert reduce(**bad) == -1, bad
    assert reduce(wsb=need - 1) == -4                                  # SE_ERR_WORKSPACE
    assert reduce(ws=ctypes.c_void_p(260)) == -1                       # misaligned workspace
    assert lib.se_svm_gram(p, p, z, z, 3, 10, 5, 10, p, None) == -1
    assert lib.se_svm_gram(p, z, z, z, 5, 10, 5, 10, p, None) == -1
    assert lib.se_svm_gram(p, z, z, z, 1, 9, 5, 10, p, None) == -1
    assert lib.se_svm_rowsum(p, 9, 5, 10, p, None) == -1
    assert lib.se_svm_rowsum(z, 10, 5, 10, p, None) == -1
    assert lib.se_svm_axpby(p, p, 10, z, p, 10, 5, 10, p, 10, None) == -1
    assert lib.se_svm_axpby(p, p, 10, p, p, 9, 5, 10, p, 10, None) == -1
    assert b"se_svm" in lib.se_last_error()


def test_cli_parser_matches_the_reference_flags():
    import evaluate_classification_accuracy as eca
    a = eca.build_parser().parse_args(["--dataset", "CIFAR-100", "--data_root", "/data", "--hierarchy", "h.txt", "--is_a", "--str_ids",
                                       "--classes_from", "c.pickle", "--augmentation_epochs", "3", "--C", "0.5", "--batch_size", "10",
                                       "--architecture", "resnet-110-fc", "--model", "a.pt", "--layer", "-1", "--label", "A",
                                       "--norm", "yes", "--prob_features", "no", "--centroids", "e.pickle",
                                       "--model", "b.pt", "--layer", "prob"])
    assert (a.dataset, a.data_root, a.hierarchy, a.is_a, a.str_ids, a.classes_from) == ("CIFAR-100", "/data", "h.txt", True, True, "c.pickle")
    assert (a.augmentation_epochs, a.C, a.batch_size, a.architecture) == (3, 0.5, 10, "resnet-110-fc")
    assert a.model == ["a.pt", "b.pt"] and a.layer == ["-1", "prob"] and a.label == ["A"] and a.norm == [True]
    assert a.prob_features == [False] and a.centroids == ["e.pickle"]
    d = eca.build_parser().parse_args(["--dataset", "x", "--data_root", "y", "--model", "m", "--layer", "3"])
    assert d.C == 0.1 and d.batch_size == 1 and d.augmentation_epochs == 1 and d.norm is None
    with pytest.raises(SystemExit):
        eca.build_parser().parse_args(["--dataset", "x", "--data_root", "y", "--model", "m"])      # --layer is required


def test_cli_dispatches_svm_centroids_and_prob_modes(capsys):
    """main() sends each --model to the mode the reference would (prob_features > centroids > SVM) with the reference's arguments,
    and prints the table of ``evaluate`` on the returned rankings."""
    import evaluate_classification_accuracy as eca
    from datasets import get_data_generator
    ds = "synthetic:10x8x40x30"
    data = get_data_generator(ds, "-")
    rng = np.random.default_rng(0)
    rankings = {}
    calls = []

    def ranking(name):
        rankings[name] = np.stack([rng.permutation(10) for _ in range(data.num_test)])
        return rankings[name]

    def svm(data_, model, layer, normalize, epochs, C, custom, batch_size):
        calls.append(("svm", model, layer, normalize, epochs, C, batch_size))
        return ranking(model)

    def centroids(data_, cent, model, layer, custom, batch_size):
        calls.append(("centroids", model, layer, cent, batch_size))
        return ranking(model)

    def prob(data_, model, layer, custom, batch_size):
        calls.append(("prob", model, layer, batch_size))
        return ranking(model)

    perf = eca.main(["--dataset", ds, "--data_root", "-", "--C", "0.3", "--augmentation_epochs", "2", "--batch_size", "5",
                     "--model", "m1", "--layer", "-1", "--norm", "1",
                     "--model", "m2", "--layer", "fc", "--norm", "0", "--centroids", "", "--centroids", "c.pickle",
                     "--model", "m3", "--layer", "4", "--label", "one", "--label", "two", "--label", "three",
                     "--prob_features", "0", "--prob_features", "1", "--prob_features", "1"],
                    modes={"svm": svm, "centroids": centroids, "prob": prob})
    # m2 has a centroid file and --prob_features 1: the prediction mode wins, as in the reference
    assert calls == [("svm", "m1", -1, True, 2, 0.3, 5), ("prob", "m2", "fc", 5), ("prob", "m3", 4, 5)]
    assert list(perf) == ["one", "two", "three"]
    for lbl, model in zip(perf, ("m1", "m2", "m3")):
        want = eca.evaluate(rankings[model], data)
        assert perf[lbl] == want
    out = capsys.readouterr().out
    assert "Accuracy" in out and "Top-5 Accuracy" in out and "three" in out
    calls.clear()
    eca.main(["--dataset", ds, "--data_root", "-", "--model", "m4", "--layer", "-1", "--centroids", "c.pickle"],
             modes={"svm": svm, "centroids": centroids, "prob": prob})
    assert calls == [("centroids", "m4", -1, "c.pickle", 1)]


def test_print_performance_matches_the_reference_layout(capsys):
    import evaluate_classification_accuracy as eca
    from collections import OrderedDict
    eca.print_performance(OrderedDict([("model", {"Accuracy": 0.5, "Top-5 Accuracy": 0.75, "Avg. Accuracy": 0.25})]))
    lines = capsys.readouterr().out.splitlines()
    assert lines[1] == "      | Accuracy | Top-5 Accuracy | Avg. Accuracy | Hierarchical Accuracy"
    assert lines[3] == "model |   0.5000 |         0.7500 |        0.2500 |                    --"
