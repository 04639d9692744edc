"""Linear SVM on the MI355X: the margin and reduction kernels of svm.hip against NumPy float64, the batched trust-region fit
against the golden optima (tools/make_svm_golden.py), train_and_predict / the CLI of evaluate_classification_accuracy.py."""
import glob
import os
import pickle

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "svm_*.npz")))
EPS32 = 2.0 ** -24

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device="cuda", dtype=dtype) if dtype is not None else t.cuda()


def _padded(a, ld, dtype=np.float32):
    """[rows, ld] device tensor whose first a.shape[1] columns are a (padding: NaN, which must never be read)."""
    out = np.full((a.shape[0], ld), np.nan, dtype=dtype)
    out[:, :a.shape[1]] = a
    return _dev(out)[:, :a.shape[1]]


def _reference_scaling(X_train, X_test, normalize):
    """evaluate_classification_accuracy.py:33-39 of the reference, in float32 (what tools/make_svm_golden.py fitted)."""
    X_train, X_test = X_train.astype(np.float32).copy(), X_test.astype(np.float32).copy()
    if normalize:
        X_train /= np.linalg.norm(X_train, axis=-1, keepdims=True)
        X_test /= np.linalg.norm(X_test, axis=-1, keepdims=True)
    else:
        X_max = np.abs(X_train).max(axis=0, keepdims=True)
        X_train /= np.maximum(1e-8, X_max)
        X_test /= np.maximum(1e-8, X_max)
    return X_train, X_test


def _problem(rng, n, d, c):
    X = rng.standard_normal((n, d)).astype(np.float32)
    W = (rng.standard_normal((c, d + 1)) / np.sqrt(d)).astype(np.float32)
    labels = rng.integers(0, c + 2, n).astype(np.int32)            # some labels match no column
    col_class = rng.permutation(c + 2)[:c].astype(np.int32)
    return X, W, labels, col_class


@pytest.mark.parametrize("n,d,c,pad", [(1, 1, 3, 0), (37, 3, 100, 5), (4097, 100, 3, 0), (37, 555, 1000, 3), (4097, 1000, 100, 1),
                                       (4097, 100, 1000, 0), (1, 1000, 1000, 2), (37, 1, 1000, 0)])
def test_margin_kernel_all_modes_match_float64(n, d, c, pad):
    import torch
    import sehip
    rng = np.random.default_rng(n * 7 + d * 3 + c)
    X, W, labels, col_class = _problem(rng, n, d, c)
    cpen = 0.7
    Xd = _padded(X, d + pad)
    Wd = _padded(W, d + 1 + 2 * pad)
    words = (c + 31) // 32
    mask = torch.full((n, words + pad), -1, dtype=torch.int32, device="cuda")[:, :words + pad]
    nblk = sehip.ops.svm_loss_blocks(n)
    loss = torch.full((c, nblk + pad), np.nan, dtype=torch.float32, device="cuda")
    Z = torch.full((n, c + pad), np.nan, dtype=torch.float32, device="cuda")[:, :c]
    sehip.svm_margin(sehip.SVM_GRAD, Xd, Wd, d=d, labels=_dev(labels), col_class=_dev(col_class), cpen=cpen, mask=mask, out=Z,
                     loss_part=loss)
    X64, W64 = X.astype(np.float64), W.astype(np.float64)
    M = X64 @ W64[:, :d].T + W64[:, d]
    bound = 4 * d * EPS32 * (np.abs(X64) @ np.abs(W64[:, :d]).T + np.abs(W64[:, d])) + 1e-30
    Y = np.where(labels[:, None] == col_class[None, :], 1.0, -1.0)
    T = 1.0 - Y * M
    Zref = np.where(T > 0, -2 * cpen * Y * T, 0.0)
    z = Z.cpu().numpy()
    assert np.all(np.abs(z - Zref) <= 2 * cpen * bound * 1.01 + 4 * EPS32 * np.abs(Zref))
    # mask: bit j % 32 of word j / 32 wherever the active set is decided beyond round-off; bits past column c are zero
    m = mask.cpu().numpy()[:, :words].astype(np.uint32)
    bits = ((m[:, np.arange(c) // 32] >> (np.arange(c) % 32).astype(np.uint32)) & 1).astype(bool)
    sure = np.abs(T) > bound
    assert np.array_equal(bits[sure], (T > 0)[sure])
    assert np.array_equal(bits, z != 0) or np.all((z != 0) <= bits)
    if c % 32:
        assert np.all(m[:, -1] >> np.uint32(c % 32) == 0)
    # loss partials: sums over 64-row blocks
    lp = loss.cpu().numpy()[:, :nblk]
    Lref = np.where(bits, np.maximum(T, 0.0) ** 2, 0.0)
    for b in range(nblk):
        want = Lref[b * 64:(b + 1) * 64].sum(axis=0)
        slack = (2 * np.abs(T[b * 64:(b + 1) * 64]) * bound[b * 64:(b + 1) * 64] + bound[b * 64:(b + 1) * 64] ** 2).sum(axis=0)
        assert np.all(np.abs(lp[:, b] - want) <= 1.01 * slack + 64 * EPS32 * want + 1e-30)
    # Hessian-vector mode against the stored mask
    V = (rng.standard_normal((c, d + 1))).astype(np.float32)
    Zh = torch.full((n, c), np.nan, dtype=torch.float32, device="cuda")
    sehip.svm_margin(sehip.SVM_HV, Xd, _padded(V, d + 1 + pad), d=d, cpen=cpen, mask=mask, out=Zh)
    V64 = V.astype(np.float64)
    Mv = X64 @ V64[:, :d].T + V64[:, d]
    bv = 4 * d * EPS32 * (np.abs(X64) @ np.abs(V64[:, :d]).T + np.abs(V64[:, d]))
    assert np.all(np.abs(Zh.cpu().numpy() - np.where(bits, 2 * cpen * Mv, 0.0)) <= 2 * cpen * bv * 1.01 + 1e-30)
    # score mode
    S = sehip.svm_margin(sehip.SVM_SCORE, Xd, Wd, d=d)
    assert np.all(np.abs(S.cpu().numpy() - M) <= bound * 1.01)


@pytest.mark.parametrize("n,d,c", [(1, 1, 3), (37, 3, 100), (4097, 100, 3), (4097, 555, 1000), (300000, 100, 100)])
def test_reduce_kernel_matches_float64_and_is_deterministic(n, d, c):
    import torch
    import sehip
    rng = np.random.default_rng(n + d + c)
    Z = rng.standard_normal((n, c)).astype(np.float32)
    Z[rng.random((n, c)) < 0.5] = 0.0
    X = (rng.standard_normal((n, d)) + 0.3).astype(np.float32)
    P = rng.standard_normal((c, d + 1)).astype(np.float32)
    Zd, Xd, Pd = _padded(Z, c + 1), _padded(X, d + 3), _dev(P)
    G1 = sehip.svm_reduce(Zd, Xd, d=d, plus=Pd)
    G2 = sehip.svm_reduce(Zd, Xd, d=d, plus=Pd)
    assert torch.equal(G1, G2)
    Xa = np.hstack([X.astype(np.float64), np.ones((n, 1))])
    want = P + Z.astype(np.float64).T @ Xa
    absum = np.abs(P) + np.abs(Z.astype(np.float64)).T @ np.abs(Xa)
    # fp32 chain over one slice of at most 4096 rows, fp64 across slices: the bound does not grow with n
    bound = (4096 + 2) * EPS32 * absum + EPS32 * np.abs(want)
    err = np.abs(G1.cpu().numpy() - want)
    assert np.all(err <= bound)
    if n >= 100000:      # and in practice the error is far below the worst case
        assert np.max(err / absum) < 1e-5


def test_gram_rowsum_axpby():
    import torch
    import sehip
    rng = np.random.default_rng(5)
    c, length, ld = 37, 1001, 1004
    V = [rng.standard_normal((c, ld)).astype(np.float32) for _ in range(4)]
    Vd = [_dev(v) for v in V]
    q = sehip.svm_gram(Vd, length=length).cpu().numpy()
    p = 0
    for a in range(4):
        for b in range(a, 4):
            want = np.sum(V[a][:, :length].astype(np.float64) * V[b][:, :length], axis=1)
            assert np.allclose(q[:, p], want, rtol=1e-12, atol=1e-9)
            p += 1
    assert np.allclose(sehip.svm_rowsum(Vd[0], length=length).cpu().numpy(), V[0][:, :length].astype(np.float64).sum(1), rtol=1e-12,
                       atol=1e-9)
    al, be = rng.standard_normal(c), rng.standard_normal(c)
    out = sehip.svm_axpby(_dev(al), Vd[1], _dev(be), Vd[2], length=length).cpu().numpy()
    want = (al[:, None] * V[1][:, :length].astype(np.float64) + be[:, None] * V[2][:, :length]).astype(np.float32)
    assert np.array_equal(out[:, :length], want)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fit_reaches_the_optimum_of_every_fixture(path):
    import linear_svm as ls
    g = np.load(path)
    C, normalize = float(g["C"]), bool(g["normalize"])
    P_train, P_test = _reference_scaling(g["X_train"], g["X_test"], normalize)
    svm = ls.LinearSVC(C=C, tol=1e-6).fit(P_train, g["y_train"])
    assert np.array_equal(svm.classes_, g["classes"])
    y_idx = np.searchsorted(svm.classes_, g["y_train"])
    Y = ls.signs(y_idx, len(svm.classes_))
    Wb = np.hstack([svm.coef_, svm.intercept_[:, None]]).astype(np.float64)
    f = ls.objective_host(P_train, Y, Wb, C)
    assert np.all(f <= g["f_opt"] * (1 + 1e-5)), np.max(f / g["f_opt"] - 1)
    # scores: the float32 solution sits within the float32 resolution of the optimum's gradient (about 1e-4 in the weights of the
    # CIFAR-size cases), hence 1e-3 here
    S = svm.decision_function(P_test)
    err = np.abs(S - g["scores"]) / (1 + np.abs(g["scores"]))
    print("%s: max score error %.2e (relative to 1 + |S|), objective excess %.2e" % (os.path.basename(path), err.max(),
                                                                                  np.max(f / g["f_opt"] - 1)))
    assert err.max() <= 1e-3
    srt = np.sort(g["scores"], axis=1)
    clear = srt[:, -1] - srt[:, -2] > 1e-3
    assert np.array_equal(svm.predict(P_test)[clear], g["classes"][np.argmax(g["scores"], axis=1)][clear])
    svm2 = ls.LinearSVC(C=C, tol=1e-6).fit(P_train, g["y_train"])
    assert np.array_equal(svm.coef_, svm2.coef_) and np.array_equal(svm.intercept_, svm2.intercept_)


def test_fewer_than_three_classes_and_non_default_parameters_are_refused():
    import linear_svm as ls
    X = np.random.default_rng(0).standard_normal((20, 3)).astype(np.float32)
    with pytest.raises(ValueError):
        ls.LinearSVC().fit(X, np.arange(20) % 2)
    with pytest.raises(NotImplementedError):
        ls.LinearSVC(loss='hinge')
    with pytest.raises(NotImplementedError):
        ls.LinearSVC().fit(X, np.arange(20) % 3, sample_weight=np.ones(20))


def test_svm_classification_ranks_its_own_decision_scores():
    import torch
    import sehip
    import evaluate_classification_accuracy as eca
    g = np.load(os.path.join(GOLDEN, "svm_cifar_maxabs.npz"))
    for normalize in (False, True):
        rank, svm = eca.svm_classification(g["X_train"], g["y_train"], g["X_test"], normalize, float(g["C"]), return_model=True)
        P_train, P_test = eca.preprocess_features(g["X_train"], g["X_test"], normalize)
        S = svm.decision_function(P_test, return_device=True)
        assert np.array_equal(rank, sehip.rank_rows(-S).cpu().numpy())
        # the preprocessing is the reference's formula
        Xtr, Xte = _reference_scaling(g["X_train"], g["X_test"], normalize)
        assert np.allclose(P_train.cpu().numpy(), Xtr, rtol=4e-7, atol=1e-7)
        assert np.allclose(P_test.cpu().numpy(), Xte, rtol=4e-7, atol=1e-7)
        assert torch.is_tensor(P_train) and P_train.is_cuda


def _model_dump(tmp_path):
    import learn_image_embeddings as lie
    emb = str(tmp_path / "emb.pickle")
    E = np.load(os.path.join(GOLDEN, "embeddings.npz"))["cifar100_unitsphere"]
    with open(emb, "wb") as f:
        pickle.dump({"embedding": E[:10], "ind2label": list(range(10)), "label2ind": {i: i for i in range(10)}}, f)
    dump = str(tmp_path / "model.pt")
    lie.main(["--dataset", "synthetic:10x32x96x64", "--data_root", "-", "--embedding", emb, "--architecture", "resnet-110-fc",
              "--loss", "inv_corr", "--lr_schedule", "SGD", "--sgd_lr", "0.05", "--epochs", "2", "--batch_size", "32",
              "--val_batch_size", "32", "--model_dump", dump, "--no_progress"])
    return dump, emb


def test_cli_end_to_end_svm_centroids_and_prob_features(tmp_path, capsys):
    import evaluate_classification_accuracy as eca
    from datasets import get_data_generator
    dump, emb = _model_dump(tmp_path)
    ds = "synthetic:10x32x96x64"
    data = get_data_generator(ds, "-")
    common = ["--dataset", ds, "--data_root", "-", "--batch_size", "16", "--architecture", "resnet-110-fc"]
    seen = {}
    orig_eval = eca.evaluate

    def spy(pred, gen, hierarchy=None):
        seen.setdefault("preds", []).append(np.asarray(pred))
        return orig_eval(pred, gen, hierarchy)

    eca.evaluate = spy
    try:
        perf = eca.main(common + ["--model", dump, "--layer", "-1", "--label", "svm", "--C", "0.1",
                                  "--model", dump, "--layer", "-1", "--label", "nn", "--centroids", "", "--centroids", emb,
                                  "--model", dump, "--layer", "-1", "--label", "prob", "--prob_features", "0", "--prob_features", "0",
                                  "--prob_features", "1"])
    finally:
        eca.evaluate = orig_eval
    out = capsys.readouterr().out
    for lbl in ("svm", "nn", "prob"):
        assert lbl in out and lbl in perf
    for (lbl, p), pred in zip(perf.items(), seen["preds"]):
        want = orig_eval(pred, data, None)
        for k in eca.METRICS:
            if k in want:
                assert p[k] == want[k]
        assert pred.shape[0] == data.num_test
        if lbl != "prob":      # the prob mode ranks the model's 100 outputs
            assert np.array_equal(np.sort(pred, axis=1), np.tile(np.arange(10), (data.num_test, 1)))


def test_scale_fit_200k_by_1000_by_1000():
    import time
    import torch
    import linear_svm as ls
    import sehip
    g = torch.Generator(device="cuda").manual_seed(0)
    n, d, c = 200000, 1000, 1000
    y = torch.randint(0, c, (n,), device="cuda", generator=g)
    centres = torch.randn((c, d), device="cuda", generator=g) / np.sqrt(d)
    X = centres[y] + 0.5 * torch.randn((n, d), device="cuda", generator=g) / np.sqrt(d)
    t0 = time.time()
    svm = ls.LinearSVC(C=0.1, tol=1e-4, max_iter=200).fit(X, y.cpu().numpy())
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    assert elapsed < 600
    # gradient criterion, checked with the kernels on the returned model: |grad f_c| <= tol |grad f_c(0)| (+ float32 slack)
    ops = ls._DeviceOps(X, y.cpu().numpy(), 0.1, c)
    ops.set_columns(np.arange(c))
    W = ops.zeros(c)
    _, _, gg0 = ops.fg(W)
    W[:, :d + 1] = torch.from_numpy(np.hstack([svm.coef_, svm.intercept_[:, None]])).cuda()
    _, _, gg = ops.fg(W)
    assert np.all(np.sqrt(gg) <= 1e-4 * np.sqrt(gg0) * 1.05)
    print("scale fit %d x %d x %d: %.2f s, %d outer iterations" % (n, d, c, elapsed, svm.n_iter_))
