"""GPU: class similarity tables (se_class_pair_tables) bitwise against ClassHierarchy, the fp64 Cholesky (se_cholesky_f64) against
LAPACK, and the drop-in compute_class_embedding.py against the embeddings the reference ships."""
import os
import pickle

import numpy as np
import pytest

from test_class_embedding_host import GOLDEN, load_hierarchy

pytestmark = pytest.mark.gpu


def _dev_tables(h, classes, **kw):
    wup, lcs = h.similarity_tables_device(classes, **kw)
    return (None if wup is None else wup.cpu().numpy()), (None if lcs is None else lcs.cpu().numpy())


@pytest.mark.parametrize("name", ["cifar", "cub", "ilsvrc", "wordnet_dag"])
def test_device_tables_are_bitwise_the_host_tables(name):
    h, classes = load_hierarchy(name)
    want_wup, want_lcs = h.similarity_tables(classes)
    wup, lcs = _dev_tables(h, classes)
    assert np.array_equal(wup, want_wup)
    assert np.array_equal(lcs, want_lcs)
    if name == "cifar":
        g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
        assert np.array_equal(wup, g["wup"]) and np.array_equal(lcs, g["lcs"])
    # the reference's convention (compute_class_embedding.py: zero distance on the diagonal), similarity and distance forms
    one = want_lcs.copy()
    np.fill_diagonal(one, 1.0)
    none, lcs1 = _dev_tables(h, classes, diag_one=True, want_wup=False)
    assert none is None and np.array_equal(lcs1, one)
    dist = np.array([[h.lcs_height(a, b) for b in classes] for a in classes[:50]])
    _, d = _dev_tables(h, classes, distance=True, want_wup=False)
    assert np.array_equal(d[:50], dist)
    _, d0 = _dev_tables(h, classes, distance=True, diag_one=True, want_wup=False)
    for k in range(50):
        dist[k, k] = 0.0
    assert np.array_equal(d0[:50], dist)


def test_inat_tables_on_100k_random_pairs():
    h, classes = load_hierarchy("inat2018")
    wup, lcs = _dev_tables(h, classes)
    assert wup.shape == (8142, 8142)
    rng = np.random.default_rng(11)
    ii, jj = rng.integers(0, 8142, size=100000), rng.integers(0, 8142, size=100000)
    H = h.max_height
    for i, j in zip(ii.tolist(), jj.tolist()):
        a, b = classes[i], classes[j]
        assert wup[i, j] == h.wup_similarity(a, b)
        assert lcs[i, j] == 1.0 - h.heights[h.lcs(a, b)] / H
    assert np.array_equal(wup, wup.T) and np.array_equal(lcs, lcs.T)


def test_pair_without_common_ancestor_names_it():
    from class_hierarchy import ClassHierarchy
    h = ClassHierarchy({1: [0], 2: [0], 4: [3]}, {0: [1, 2], 3: [4]})
    with pytest.raises(KeyError, match="1 and 4"):
        h.similarity_tables_device([1, 2, 4])


def _inat_similarity(n):
    """1 - lcs_height over the first n iNat species (unit diagonal): a real unit-sphere target."""
    h, classes = load_hierarchy("inat2018")
    _, s = h.similarity_tables_device(classes[:n], diag_one=True, want_wup=False)
    return s


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 1000, 8142])
def test_cholesky_matches_lapack(n):
    import torch
    import sehip
    s = _inat_similarity(n) if n > 2 else torch.tensor([[1.0, 0.25], [0.25, 1.0]], dtype=torch.float64, device="cuda")[:n, :n].contiguous()
    s_h = s.cpu().numpy()
    a = (s.tril() + 7.0 * torch.ones_like(s).triu(1)).contiguous()      # only the lower triangle is read
    _, info = sehip.cholesky_lower_(a)
    assert int(info.item()) == -1
    L = a.cpu().numpy()
    assert np.all(np.triu(L, 1) == 0.0)
    assert np.all(np.diag(L) > 0)
    want = np.linalg.cholesky(s_h)
    err_l = np.abs(L - want).max()
    err_r = float((a @ a.T - s).abs().max())
    assert err_l <= 1e-12, err_l
    assert err_r <= 1e-12, err_r


def test_cholesky_pitch_and_random_spd():
    import torch
    import sehip
    rng = np.random.default_rng(3)
    for n in (97, 130):
        x = rng.standard_normal((n, n + 40))
        s = x @ x.T / (n + 40) + 0.5 * np.eye(n)
        buf = torch.full((n, n + 3), 5.0, dtype=torch.float64, device="cuda")
        buf[:, :n] = torch.from_numpy(s)
        view = buf[:, :n]
        _, info = sehip.cholesky_lower_(view)
        assert int(info.item()) == -1
        assert np.abs(view.cpu().numpy() - np.linalg.cholesky(s)).max() <= 1e-12
        assert torch.all(buf[:, n:] == 5.0)          # columns past n untouched


def test_cholesky_reports_the_failed_row():
    import torch
    import sehip
    cases = []
    cases.append((np.ones((3, 3)), 1))                                       # singular: second pivot exactly 0
    cases.append((np.array([[1, .9, 0], [.9, 1, .9], [0, .9, 1]]), 2))      # indefinite
    rng = np.random.default_rng(8)
    x = rng.standard_normal((200, 260))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    s = x @ x.T
    s[150, 150] = 0.0                                                        # pivot of row 150 < 0, block 3
    cases.append((s, 150))
    t = s.copy()
    t[0, 0] = -1.0
    cases.append((t, 0))
    nan_in = x @ x.T
    nan_in[70, 3] = np.nan
    cases.append((nan_in, 70))
    for m, row in cases:
        a = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64)).cuda()
        _, info = sehip.cholesky_lower_(a)
        assert int(info.item()) == row, (row, int(info.item()))
        L = a.cpu().numpy()
        assert np.isnan(L[row, row])
        assert np.all(np.isnan(np.tril(L)[row + 1:][np.tril(np.ones_like(L, dtype=bool))[row + 1:]]))
        assert np.all(np.triu(L, 1) == 0.0)
        if row > 0 and np.isfinite(m[:row, :row]).all():
            assert np.abs(L[:row, :row] - np.linalg.cholesky(m[:row, :row])).max() <= 1e-12
    z = torch.empty((0, 0), dtype=torch.float64, device="cuda")
    _, info = sehip.cholesky_lower_(z)
    assert int(info.item()) == -1


def test_unitsphere_embedding_warns_and_leaves_nan_rows():
    import compute_class_embedding as cce
    s = np.array([[1, .9, 0], [.9, 1, .9], [0, .9, 1.0]])
    with pytest.warns(RuntimeWarning, match="class #3"):
        e = cce.unitsphere_embedding(s)
    assert np.isfinite(e[:2]).all() and np.isnan(e[2, 2]) and np.isfinite(e[2, :2]).all()


def _write_hierarchy(tmp_path, edges):
    path = str(tmp_path / "hierarchy.txt")
    with open(path, "w") as f:
        for p, c in edges:
            f.write("%s %s\n" % (p, c))
    return path


def _write_classes(tmp_path, classes):
    path = str(tmp_path / "classes.txt")
    with open(path, "w") as f:
        f.write("".join("%s\n" % c for c in classes))
    return path


@pytest.mark.parametrize("name,key", [("cifar", "cifar100_unitsphere"), ("cub", "cub_balanced_unitsphere")])
def test_cli_reproduces_the_shipped_unitsphere_embeddings(name, key, tmp_path, capsys):
    import compute_class_embedding as cce
    g = np.load(os.path.join(GOLDEN, "hierarchy_%s.npz" % name))
    emb = np.load(os.path.join(GOLDEN, "embeddings.npz"))
    labels = emb[key + "__ind2label"].tolist()
    out = str(tmp_path / "e.pickle")
    cce.main(["--hierarchy", _write_hierarchy(tmp_path, g["edges"].tolist()), "--class_list", _write_classes(tmp_path, labels),
              "--out", out])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith('Computed %d-dimensional semantic embeddings for %d classes using the "unitsphere" method in '
                               % (len(labels), len(labels)))
    assert lines[1].startswith("Maximum deviation from target similarities: ")
    assert lines[2].startswith("Average deviation from target similarities: ")
    assert float(lines[1].split(": ")[1]) < 1e-12
    with open(out, "rb") as f:
        dump = pickle.load(f)
    assert set(dump) == {"ind2label", "label2ind", "embedding"}
    assert dump["ind2label"] == labels and dump["label2ind"] == {c: i for i, c in enumerate(labels)}
    assert dump["embedding"].dtype == np.float64
    assert np.abs(dump["embedding"] - emb[key]).max() <= 1e-12
    assert np.all(np.triu(dump["embedding"], 1) == 0.0)


def test_cli_reproduces_the_imagenet_mintree_embedding(tmp_path, capsys):
    import compute_class_embedding as cce
    g = np.load(os.path.join(GOLDEN, "hierarchy_ilsvrc.npz"))
    ref = np.load(os.path.join(GOLDEN, "imagenet_mintree_unitsphere.npz"))
    labels = ref["ind2label"].tolist()
    out = str(tmp_path / "e.pickle")
    cce.main(["--hierarchy", _write_hierarchy(tmp_path, g["edges"].tolist()), "--str_ids",
              "--class_list", _write_classes(tmp_path, labels), "--out", out])
    with open(out, "rb") as f:
        dump = pickle.load(f)
    assert dump["ind2label"] == labels
    err = np.abs(dump["embedding"] - ref["embedding"].astype(np.float64)).max()
    assert err <= float(ref["max_abs_f64_minus_f32"]) + 1e-12, err


def test_spheres_matches_a_host_cholesky_of_the_gram_matrix(tmp_path, capsys):
    import compute_class_embedding as cce
    h, classes = load_hierarchy("cifar")
    d = np.array([[h.lcs_height(a, b) if a != b else 0.0 for b in classes] for a in classes])
    e = cce.euclidean_embedding(d)
    assert e.shape == (100, 99) and np.all(e[0] == 0.0)
    gram = (d[0, 1:, None] ** 2 + d[None, 0, 1:] ** 2 - d[1:, 1:] ** 2) / 2
    assert np.abs(e[1:] - np.linalg.cholesky(gram)).max() <= 1e-12
    diff = e[:, None, :] - e[None, :, :]
    assert np.abs(np.sqrt((diff ** 2).sum(-1)) - d).max() <= 1e-9
    # the CLI path: same embedding, the distance report
    g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
    out = str(tmp_path / "s.pickle")
    cce.main(["--hierarchy", _write_hierarchy(tmp_path, g["edges"].tolist()), "--out", out, "--method", "spheres"])
    lines = capsys.readouterr().out.splitlines()
    assert lines[1].startswith("Maximum deviation from target distances: ") and float(lines[1].split(": ")[1]) < 1e-9
    with open(out, "rb") as f:
        assert np.abs(pickle.load(f)["embedding"] - e).max() <= 1e-12
    # triangle inequality violated at the third class: the reference's message and numbering
    bad = np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 3.0], [1.0, 3.0, 0.0]])
    with pytest.raises(RuntimeError, match=r"^Failed to place class #3: There is no common intersection of all spheres \(offset: 2\.5"):
        cce.euclidean_embedding(bad)


def test_hierarchical_precision_device_tables_change_nothing():
    """hierarchical_precision_device builds its class tables with se_class_pair_tables when the native kernels run; the per-query
    metrics are bitwise those of the same call on host-built tables (a 'device' entry in ``kernels`` keeps the host tables)."""
    import torch
    from test_host import _hierarchy_from_fixture
    import pathlib
    import tempfile
    for name in ("cifar", "cub", "ilsvrc"):
        g = np.load(os.path.join(GOLDEN, "hierarchy_%s.npz" % name))
        if name == "cifar":
            h, _ = load_hierarchy("cifar")
            labels = g["labels"].tolist()
        else:
            with tempfile.TemporaryDirectory() as tmp:
                h, labels = _hierarchy_from_fixture(g, pathlib.Path(tmp))
        ks = g["ks"].tolist()
        for ahp, ap in ((True, True), (50, False)):
            avg, per_q = h.hierarchical_precision_device(g["features"].copy(), labels, ks, compute_ahp=ahp, compute_ap=ap, normalize=True)
            avg_h, per_q_h = h.hierarchical_precision_device(g["features"].copy(), labels, ks, compute_ahp=ahp, compute_ap=ap,
                                                             normalize=True, kernels={"device": torch.device("cuda", 0)})
            assert avg == avg_h
            for m in per_q:
                assert per_q[m] == per_q_h[m], (name, m)
