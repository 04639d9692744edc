"""CPU: the opt-in float64 retrieval path (precision='float64', --float64) -- the canonical restatement the GPU tests compare
against, the host restatement of the run repair, the argument checks and the command-line flags.  No GPU is involved."""
import os
import pickle

import numpy as np
import pytest
import torch

import _f64_canon as fc


def _features(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d))


# ---------------------------------------------------------------- the canonical chain

@pytest.mark.parametrize("d", [3, 16, 100])
@pytest.mark.parametrize("normalize", [True, False])
def test_chain_equals_numpy_where_the_host_blas_follows_one_chain(d, normalize):
    """n = 64, d in {3, 16, 100}: shapes at which this image's float64 BLAS returns the sequential FMA chain (it does not at
    every shape -- DESIGN.md section 3.1 -- which is why Gate 1 of the contract is the chain, not the BLAS)."""
    x = _features(64, d, 7 + d)
    want = fc.numpy_dist(x, normalize)
    if normalize:
        xn = x / np.linalg.norm(x, axis=-1, keepdims=True)
        got = fc.chain_dist(xn, xn, True)
    else:
        sq = np.sum(x ** 2, axis=-1)
        got = fc.chain_dist(x, x, False, sq, sq)
    assert fc.same_bits(got, want)


def test_chain_is_sequential_and_fused():
    """One product that only a fused multiply-add keeps: (1 + 2^-30)^2 - 1 needs the 2^-60 term of the exact product."""
    e = 2.0 ** -30
    a = np.array([[1.0, 1.0 + e]])
    b = np.array([[-1.0, 1.0 + e]])
    assert fc.fma_chain(a, b)[0, 0] == 2 * e + e * e
    assert fc.fma_chain(np.zeros((2, 0)), np.zeros((3, 0))).tolist() == [[0.0] * 3] * 2


# ---------------------------------------------------------------- the run repair

def _crafted_rows():
    rng = np.random.default_rng(3)
    rows = []
    base = np.sort(rng.standard_normal(40)).astype(np.float32).astype(np.float64)         # distinct images
    rows.append(rng.permutation(base))
    tied = base.copy()
    tied[5:8] = tied[5] + np.array([2.0, 0.0, 1.0]) * 2.0 ** -40                            # run of 3, out of order
    tied[20:22] = tied[20]                                                                  # exact float64 tie
    tied[30:32] = [0.0, -0.0]
    tied[38:] = np.nan
    rows.append(rng.permutation(tied))
    rows.append(1.0 + np.arange(40)[::-1] * 2.0 ** -40)                                     # one run, descending index order
    return rows


@pytest.mark.parametrize("row", range(3))
def test_refine_runs_restatement_equals_lexsort(row):
    d64 = _crafted_rows()[row]
    img = d64.astype(np.float32)
    first = fc.canon_rank(img.astype(np.float64))[0]          # what se_rank_rows returns for the image
    want = fc.canon_rank(d64)[0]
    if row == 0:
        assert np.array_equal(first, want)
    if row == 2:
        assert np.array_equal(first, np.arange(40)) and np.array_equal(want, np.arange(40)[::-1])
    assert np.array_equal(fc.refine_runs(d64, img, first), want)
    val, nan = fc.canon_key(d64)
    assert np.array_equal(want, np.lexsort((np.arange(40), val, nan)))


# ---------------------------------------------------------------- argument checks

def test_float64_precision_refuses_float32_features():
    import evaluate_retrieval as er
    x32 = _features(8, 4, 0).astype(np.float32)
    with pytest.raises(ValueError, match="float64 features"):
        er.pairwise_retrieval(x32, normalize=True, precision='float64')
    with pytest.raises(ValueError, match="float64 features"):
        er.pairwise_retrieval({i: x32[i] for i in range(8)}, precision='float64')
    with pytest.raises(ValueError, match="kblocks"):
        er.pairwise_retrieval(_features(8, 4, 0), precision='float64', kblocks='openblas')
    with pytest.raises(ValueError, match="precision"):
        er.pairwise_retrieval(x32, precision='float16')
    with pytest.raises(ValueError, match="float64"):
        er.to_device_f64(torch.zeros(3, 2), 'cpu')
    with pytest.raises(ValueError, match="gallery"):
        er.ranking_tiles(torch.zeros((3, 2), dtype=torch.float64), precision='float64', gallery=torch.zeros((3, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="16-bit"):
        er.ranking_tiles(torch.zeros((3, 2), dtype=torch.float64), precision='float64', idx16=True)


def test_default_precision_still_warns_on_float64_features():
    import evaluate_retrieval as er
    with pytest.warns(RuntimeWarning, match='float64 features'):
        try:
            er.pairwise_retrieval(_features(8, 4, 0), normalize=True, precision=None)
        except Exception:       # no GPU here: the call fails loudly AFTER the warning
            pass


def test_device_metric_functions_refuse_gallery_and_kblocks_in_float64():
    from class_hierarchy import ClassHierarchy
    from recall_precision import recall_precision_device
    x = _features(6, 3, 1)
    labels = [0, 1, 0, 1, 2, 2]
    h = None      # (the checks below come before any access to the hierarchy)
    for kw in ({'gallery': x}, {'kblocks': 'openblas'}):
        with pytest.raises(ValueError, match="float64"):
            recall_precision_device(x, labels, precision='float64', **kw)
        with pytest.raises(ValueError, match="float64"):
            ClassHierarchy.hierarchical_precision_device(h, x, labels, precision='float64', **kw)


# ---------------------------------------------------------------- the tile generator on CPU stand-ins

def _standins(calls):
    def pairwise_dist_f64(a, b, cosine, sqa, sqb, out=None, img=True):
        calls.append((tuple(a.shape), cosine, sqa is not None))
        d = fc.chain_dist(a.numpy(), b.numpy(), cosine, None if sqa is None else sqa.numpy(), None if sqb is None else sqb.numpy())
        return torch.from_numpy(d), torch.from_numpy(d.astype(np.float32))

    def rank_rows_f64(d64, img, idx64=False, out=None):
        first = fc.canon_rank(img.numpy().astype(np.float64))
        rk = np.stack([fc.refine_runs(d64.numpy()[i], img.numpy()[i], first[i]) for i in range(len(first))])
        return torch.from_numpy(rk.astype(np.int64 if idx64 else np.int32))
    return {'pairwise_dist_f64': pairwise_dist_f64, 'rank_rows_f64': rank_rows_f64}


@pytest.mark.parametrize("normalize", [True, False])
def test_ranking_tiles_float64_host_arithmetic_and_tiling(normalize):
    """Normalisation / square norms are the reference's NumPy lines; tiles cover the queries in order; the ranks are NumPy's."""
    import evaluate_retrieval as er
    x = _features(37, 5, 11)
    calls = []
    t = torch.from_numpy(x.copy())
    tiles = list(er.ranking_tiles(t, normalize, tile_rows=16, precision='float64', kernels=_standins(calls)))
    assert [r0 for r0, _ in tiles] == [0, 16, 32] and [c[0][0] for c in calls] == [16, 16, 5]
    assert all(c[1] == normalize and c[2] == (not normalize) for c in calls)
    if normalize:
        assert np.array_equal(t.numpy(), x / np.linalg.norm(x, axis=-1, keepdims=True))     # in place, like the float32 path
    got = np.concatenate([tile.numpy() for _, tile in tiles])
    assert got.dtype == np.int32
    assert np.array_equal(got, np.argsort(fc.numpy_dist(x, normalize), axis=-1, kind='stable'))


# ---------------------------------------------------------------- command lines

_BASE = ["--dataset", "d", "--data_root", "r", "--feat", "f.pickle"]


def test_float64_flags_parse():
    import evaluate_retrieval as er
    import plot_recall_precision as prp
    ev = _BASE + ["--hierarchy", "h"]
    assert er.parse_args(ev + ["--float64"]).float64 is True
    assert not hasattr(er.parse_args(ev), "float64")             # a run without the flag parses to what it did before
    assert prp.build_parser().parse_args(_BASE + ["--float64"]).float64 is True
    assert not hasattr(prp.build_parser().parse_args(_BASE), "float64")
    assert "float32" in er.build_parser().format_help().split("--float64")[-1][:700]     # the help says what stays float32
    ns = er.parse_args(ev + ["--float64"])
    assert er.float64_precision(ns, np.zeros((2, 2))) == 'float64'
    assert er.float64_precision(ns, np.zeros((2, 2), dtype=np.float32)) is None
    assert er.float64_precision(er.parse_args(ev), np.zeros((2, 2))) is None


@pytest.mark.parametrize("extra", [["--gallery_feat", "g.pickle", "--clip_ahp", "10"], ["--gallery_feat", "g.pickle", "--rank_gallery"],
                                   ["--kblocks", "openblas"]])
def test_float64_flag_conflicts_raise(extra, capsys):
    import evaluate_retrieval as er
    with pytest.raises(SystemExit):
        er.parse_args(_BASE + ["--hierarchy", "h", "--float64"] + extra)
    assert "--float64" in capsys.readouterr().err
    er.parse_args(_BASE + ["--hierarchy", "h"] + extra)          # (fine without the flag)


def test_float64_flag_refuses_sharded_evaluation_and_plot_cli_conflicts(monkeypatch, capsys):
    import evaluate_retrieval as er
    import plot_recall_precision as prp
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        er.parse_args(_BASE + ["--hierarchy", "h", "--float64"])
    assert "multi-GPU" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit):                               # the plot CLI checks before it loads anything
        prp.main(_BASE + ["--float64", "--gallery_feat", "g.pickle"])
    assert "--float64" in capsys.readouterr().err


def test_float64_pickle_of_lists_is_float64(tmp_path):
    """How float64 features arise: a {id: list} dictionary goes through np.stack."""
    import evaluate_retrieval as er
    path = os.path.join(str(tmp_path), "f.pickle")
    with open(path, "wb") as f:
        pickle.dump({"feat": {i: [float(i), 1.0] for i in range(3)}}, f)
    feats, ids, _ = er._as_feature_matrix(path)
    assert feats.dtype == np.float64 and ids.tolist() == [0, 1, 2]
