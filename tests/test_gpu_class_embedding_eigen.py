"""GPU: the eigendecomposition methods of compute_class_embedding.py on the device eigensolver -- sim_approx_factor and mds_factor
against LAPACK (np.linalg.eigh) and the host forms, and the command line with NumPy's eigh disabled.

Tolerances are those of tests/test_gpu_eigh.py (tau = C n 2^-52 with the constant of the NumPy model); the truncated embeddings
are checked through quantities that do not depend on the basis a cluster of equal eigenvalues gets (the class similarities are
heavily degenerate: CIFAR-100 has 44 distinct eigenvalues among 100)."""
import os
import pickle

import numpy as np
import pytest

from test_class_embedding_host import GOLDEN
from test_gpu_eigh import C, EPS, class_tables, double_centred

pytestmark = pytest.mark.gpu


def _tau(n):
    return C * n * EPS


@pytest.mark.parametrize("name", ["cifar", "cub"])
def test_sim_approx_factor_reproduces_the_similarities(name):
    import compute_class_embedding as cce
    s = class_tables(name)[0]
    n = s.shape[0]
    lam = np.linalg.eigh(s)[0]
    scale = np.abs(lam).max()
    e = cce.sim_approx_factor(s).cpu().numpy()
    assert e.shape == (n, n) and e.dtype == np.float64
    assert np.abs(e @ e.T - s).max() <= _tau(n) * scale
    for d in (10, 32):
        e = cce.sim_approx_factor(s, d).cpu().numpy()
        assert e.shape == (n, d)
        assert np.abs((e * e).sum(0) - lam[n - d:]).max() <= _tau(n) * scale         # the d largest eigenvalues, ascending
        lost = float(((e @ e.T - s) ** 2).sum())
        want = float((lam[:n - d] ** 2).sum())
        assert abs(lost - want) <= 1e-9 * want, (d, lost, want)
    assert cce.sim_approx_factor(s, n + 5).shape == (n, n)


def test_sim_approx_factor_rejects_an_indefinite_matrix():
    import compute_class_embedding as cce
    s = class_tables("cifar")[0].copy()
    s[0, 1] = s[1, 0] = 1.5                     # a 2 x 2 minor with determinant < 0
    with pytest.raises(RuntimeError, match="^Given class_sim is not positive semi-definite.$"):
        cce.sim_approx_factor(s)
    s[2, 3] = s[3, 2] = np.nan
    with pytest.raises(RuntimeError, match="NaN"):
        cce.sim_approx_factor(s)


def test_mds_factor_matches_the_host_mds():
    import compute_class_embedding as cce
    dist = class_tables("cub")[1]
    n = dist.shape[0]
    lam = np.linalg.eigh(double_centred(dist))[0]
    scale = np.abs(lam).max()
    desc = lam[::-1]
    gaps = [d for d in range(1, n) if desc[d - 1] - desc[d] > 1e-6 * scale and desc[d - 1] > EPS]
    d = min(gaps, key=lambda k: abs(k - 20))            # a cut between two clusters: the embedding's Gram matrix is then unique
    host = cce.mds(dist, d)
    dev = cce.mds_factor(dist, d).cpu().numpy()
    assert dev.shape == host.shape == (n, d)
    assert np.abs(dev @ dev.T - host @ host.T).max() <= _tau(n) * scale
    assert np.abs((dev * dev).sum(0) - desc[:d]).max() <= _tau(n) * scale            # largest first
    # every eigenvalue above eps (the centred matrix's zero eigenvalue is rounding noise on either side of that threshold, so the
    # column counts may differ by it; the Gram matrix does not notice)
    full_host, full_dev = cce.mds(dist), cce.mds_factor(dist).cpu().numpy()
    assert n - 2 <= full_dev.shape[1] <= n
    assert np.abs(full_dev @ full_dev.T - full_host @ full_host.T).max() <= _tau(n) * scale


def test_cli_runs_approx_sim_without_numpy_eigh(tmp_path, capsys, monkeypatch):
    import compute_class_embedding as cce

    def no_eigh(*args, **kwargs):
        raise AssertionError("np.linalg.eigh was called: the device path did not run")
    g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
    hp, out = str(tmp_path / "hierarchy.txt"), str(tmp_path / "e.pickle")
    with open(hp, "w") as f:
        f.writelines("%s %s\n" % (p, c) for p, c in g["edges"].tolist())
    s = class_tables("cifar")[0]
    lam = np.linalg.eigh(s)[0]
    monkeypatch.setattr(np.linalg, "eigh", no_eigh)
    cce.main(["--hierarchy", hp, "--out", out, "--method", "approx_sim", "--num_dim", "32"])
    monkeypatch.undo()
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith('Computed 32-dimensional semantic embeddings for 100 classes using the "approx_sim" method in ')
    with open(out, "rb") as f:
        dump = pickle.load(f)
    assert set(dump) == {"ind2label", "label2ind", "embedding"}
    assert dump["ind2label"] == list(range(100)) and dump["label2ind"] == {c: c for c in range(100)}
    e = dump["embedding"]
    assert e.shape == (100, 32) and e.dtype == np.float64
    assert np.abs((e * e).sum(0) - lam[-32:]).max() <= _tau(100) * lam[-1]
    err = np.abs(e @ e.T - s)
    assert lines[1].startswith("Maximum deviation from target similarities: ")
    assert lines[2].startswith("Average deviation from target similarities: ")
    assert float(lines[1].split(": ")[1]) == pytest.approx(err.max(), rel=1e-9)
    assert float(lines[2].split(": ")[1]) == pytest.approx(err.mean(), rel=1e-9)
    # mds through the command line as well: the distance report of the device embedding
    monkeypatch.setattr(np.linalg, "eigh", no_eigh)
    cce.main(["--hierarchy", hp, "--out", out, "--method", "mds", "--num_dim", "16"])
    monkeypatch.undo()
    lines = capsys.readouterr().out.splitlines()
    with open(out, "rb") as f:
        m = pickle.load(f)["embedding"]
    assert m.shape == (100, 16) and lines[0].startswith("Computed 16-dimensional")
    diff = np.sqrt(((m[:, None, :] - m[None, :, :]) ** 2).sum(-1))
    assert float(lines[1].split(": ")[1]) == pytest.approx(np.abs(diff - class_tables("cifar")[1]).max(), rel=1e-9)
