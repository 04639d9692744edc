"""CPU: the host side of the symmetric eigensolver (se_eigh_f64) -- the round-robin schedule in its Python statement
(sehip.eigh_schedule) and in the library's (se_eigh_schedule), the argument checks of the entry points, the NumPy model of the
kernel (tools/eigh_model.py) against LAPACK on one small matrix, and compute_class_embedding.main without a GPU."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

from test_class_embedding_host import GOLDEN, ROOT, load_hierarchy


@pytest.mark.parametrize("nb", [2, 4, 6, 8])
def test_schedule_meets_every_pair_once(nb):
    import sehip
    rounds = sehip.eigh_schedule(nb)
    assert len(rounds) == nb - 1
    seen = set()
    for rnd in rounds:
        assert len(rnd) == nb // 2
        members = [b for pair in rnd for b in pair]
        assert sorted(members) == list(range(nb))                # disjoint within the round, and every block plays
        for lo, hi in rnd:
            assert 0 <= lo < hi < nb
            assert (lo, hi) not in seen
            seen.add((lo, hi))
    assert seen == {(i, j) for i in range(nb) for j in range(i + 1, nb)}


@pytest.mark.parametrize("nb", [2, 4, 6, 8, 64, 256])
def test_library_schedule_is_the_python_schedule(nb):
    """The C driver and the kernels derive every round from the rule se_eigh_schedule exports; it is the Python statement's."""
    import sehip
    pairs = np.full((nb - 1, nb // 2, 2), -1, dtype=np.int32)
    assert sehip.lib().se_eigh_schedule(nb, pairs.ctypes.data_as(ctypes.c_void_p)) == 0
    assert pairs.tolist() == [[list(p) for p in rnd] for rnd in sehip.eigh_schedule(nb)]


def test_schedule_rejects_odd_and_small_counts():
    import sehip
    for nb in (0, 1, 3, 7):
        with pytest.raises(sehip.SehipError):
            sehip.eigh_schedule(nb)
        buf = (ctypes.c_int32 * 64)()
        assert sehip.lib().se_eigh_schedule(nb, buf) == -1
    assert sehip.lib().se_eigh_schedule(4, None) == -1
    assert b"null pointer" in sehip.lib().se_last_error()


def test_entry_point_checks_its_arguments_without_a_gpu():
    import sehip
    from sehip import _lib
    lib = sehip.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    # se_eigh_f64(a, lda, n, w, v, ldv, workspace, info, max_sweeps, stream)
    for args in ((z, 4, 4, one, one, 4, one, one, 30), (one, 4, 4, z, one, 4, one, one, 30), (one, 4, 4, one, z, 4, one, one, 30),
                 (one, 4, 4, one, one, 4, z, one, 30), (one, 4, 4, one, one, 4, one, z, 30), (z, 0, 0, z, z, 0, z, z, 30)):
        assert lib.se_eigh_f64(*args, z) == -1
        assert b"null pointer" in lib.se_last_error()
    assert lib.se_eigh_f64(one, 3, 4, one, one, 4, one, one, 30, z) == -1
    assert b"leading dimension" in lib.se_last_error()
    assert lib.se_eigh_f64(one, 4, 4, one, one, 3, one, one, 30, z) == -1
    assert b"leading dimension" in lib.se_last_error()
    assert lib.se_eigh_f64(one, 4, -1, one, one, 4, one, one, 30, z) == -1
    assert lib.se_eigh_f64(one, 4, 4, one, one, 4, one, one, -1, z) == -1
    assert b"max_sweeps" in lib.se_last_error()
    assert lib.se_eigh_f64(one, 4, 4, one, one, 4, ctypes.c_void_p(20), one, 30, z) == -1
    assert b"aligned" in lib.se_last_error()
    assert lib.se_eigh_f64(one, 1 << 20, 1 << 20, one, one, 1 << 20, one, one, 30, z) == _lib.DEFINES["SE_ERR_UNSUPPORTED"]
    assert lib.se_eigh_f64_workspace_bytes(0) >= 0
    assert lib.se_eigh_f64_workspace_bytes(-1) == -1
    assert lib.se_eigh_f64_workspace_bytes(1 << 20) == -1
    for n in (1, 63, 64, 65, 8142):
        pairs = (n + 63) // 64
        assert lib.se_eigh_f64_workspace_bytes(n) >= 8 * (n * n + pairs * 64 * 64 + n) and lib.se_eigh_f64_workspace_bytes(n) % 8 == 0
    assert _lib.DEFINES["SE_EIGH_NOT_CONVERGED"] == -1 and _lib.DEFINES["SE_EIGH_NONFINITE"] == -2


def test_ops_eigh_refuses_host_tensors():
    import torch
    import sehip
    with pytest.raises(sehip.SehipError):
        sehip.eigh(torch.eye(3, dtype=torch.float64))           # a host tensor, with or without a device


def test_numpy_model_of_the_kernel_reaches_lapack():
    """tools/eigh_model.py states the kernel's schedule and skip rule in NumPy (it fixes the tolerance constant of the GPU test):
    three blocks padded to four, an indefinite matrix with zero rows."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eigh_model
    rng = np.random.default_rng(17)
    n = 70
    x = rng.standard_normal((n, n))
    a = x + x.T
    a[5, :] = a[:, 5] = 0.0
    a[69, :] = a[:, 69] = 0.0
    w, v, info = eigh_model.eigh_model(a)
    assert 1 <= info <= 12
    e, r, o = eigh_model.ratios(a, w, v)
    assert max(e, r, o) <= 20.0, (e, r, o)
    assert eigh_model.eigh_model(np.diag(np.arange(5.0)))[2] == 0
    bad = a.copy()
    bad[3, 4] = bad[4, 3] = np.nan
    assert eigh_model.eigh_model(bad)[2] == -2
    assert eigh_model.eigh_model(a, max_sweeps=1)[2] == -1


def test_cli_takes_the_host_eigendecomposition_without_a_gpu(tmp_path, capsys, monkeypatch):
    import torch
    import compute_class_embedding as cce
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # where a GPU is visible: main() as it runs without one
    g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
    hp, out = str(tmp_path / "hierarchy.txt"), str(tmp_path / "e.pickle")
    with open(hp, "w") as f:
        f.writelines("%s %s\n" % (p, c) for p, c in g["edges"].tolist())
    cce.main(["--hierarchy", hp, "--out", out, "--method", "approx_sim", "--num_dim", "32"])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith('Computed 32-dimensional semantic embeddings for 100 classes using the "approx_sim" method in ')
    h, classes = load_hierarchy("cifar")
    _, s = h.similarity_tables(classes)
    np.fill_diagonal(s, 1.0)
    with open(out, "rb") as f:
        dump = pickle.load(f)
    assert set(dump) == {"ind2label", "label2ind", "embedding"} and dump["ind2label"] == classes
    e = dump["embedding"]
    assert e.shape == (100, 32) and e.dtype == np.float64
    lam = np.linalg.eigh(s)[0]
    assert np.abs((e * e).sum(0) - lam[-32:]).max() <= 1e-12
    err = np.abs(e @ e.T - s)
    assert float(lines[1].split(": ")[1]) == pytest.approx(err.max(), rel=1e-9)
    assert float(lines[2].split(": ")[1]) == pytest.approx(err.mean(), rel=1e-9)
    # the other methods still need the device
    import sehip
    with pytest.raises(sehip.SehipError):
        cce.main(["--hierarchy", hp, "--out", out])
