"""GPU: se_bootstrap_indices / se_bootstrap_means against the NumPy restatement of the pinned stream (tests/_bootstrap_canon.py),
and the bootstrap output of the evaluation tools end to end.

Bounds.  The index stream is integer arithmetic: equal.  Means of dyadic tables (integers below 2^20 divided by 2^10; at most
65,539 draws, so every partial sum is an integer below 2^37 over 2^10) are exact in every summation order, so the kernel must give
float64(S) / float64(q) bit for bit.  General float64 tables: any order of q non-negative float64 adds errs by at most
(q - 1) 2^-53 sum|v|, plus one rounding of the division: |out - exact| <= q 2^-53 mean|v| over the drawn rows, against the exact
rational mean."""
import os
import pickle
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

import _bootstrap_canon as bc

pytestmark = pytest.mark.gpu

BIG_SEED = 0xfedcba9876543210       # high key word and sign bit set
HIGH_REP = 2 ** 32 + 5              # high counter word


def raw_means(vals_np, ldv, ldo, reps, seed, rep0=0):
    """se_bootstrap_means through the C ABI with chosen pitches: pad columns of the table are NaN, those of the result hold a
    sentinel.  Returns the whole [reps, ldo] result."""
    import sehip
    from sehip import _lib
    q, m = vals_np.shape
    table = torch.full((q, ldv), float("nan"), dtype=torch.float64, device="cuda")
    table[:, :m] = torch.from_numpy(vals_np).cuda()
    out = torch.full((reps, ldo), -7.0, dtype=torch.float64, device="cuda")
    _lib.call("se_bootstrap_means", table, ldv, q, m, sehip.ops._seed_arg(seed), rep0, reps, out, ldo)
    return out.cpu().numpy()


@pytest.mark.parametrize("q", [1, 2, 3, 10, 255, 256, 257, 65539])
def test_index_stream_equals_the_restatement(q):
    import sehip
    for reps in (1, 3, 257):
        for seed, rep0 in ((0, 0), (1, 5), (BIG_SEED, HIGH_REP)):
            if q == 65539 and reps == 257 and seed != BIG_SEED:
                continue        # (one large case is enough: 17 M indices each)
            got = sehip.bootstrap_indices(q, reps, seed=seed, rep0=rep0).cpu().numpy()
            assert got.dtype == np.int32 and got.shape == (reps, q)
            assert np.array_equal(got, bc.index_matrix(q, seed, rep0, reps)), (q, reps, seed, rep0)


def test_index_windows_that_split_a_philox_block():
    import sehip
    for q, t0, count in ((10, 1, 7), (10, 3, 1), (257, 255, 2), (257, 1, 255), (65539, 65537, 1), (65539, 12345, 777), (7, 7, 0)):
        for seed, rep0 in ((0, 0), (BIG_SEED, HIGH_REP)):
            got = sehip.bootstrap_indices(q, 3, seed=seed, rep0=rep0, t0=t0, count=count).cpu().numpy()
            assert np.array_equal(got, bc.index_matrix(q, seed, rep0, 3, t0, count)), (q, t0, count)


def test_index_stream_at_the_largest_q():
    import sehip
    q = 2 ** 31 - 1
    got = sehip.bootstrap_indices(q, 3, seed=0x0123456789abcdef, rep0=3, t0=0, count=4).cpu().numpy()
    assert got[0].tolist() == [548717665, 2017899782, 1530695275, 257359391]
    for seed, rep0 in ((0, 0), (BIG_SEED, HIGH_REP)):
        got = sehip.bootstrap_indices(q, 3, seed=seed, rep0=rep0, t0=q - 8, count=8).cpu().numpy()
        assert np.array_equal(got, bc.index_matrix(q, seed, rep0, 3, q - 8, 8))
        assert got.min() >= 0
    # a pitch wider than the window: the columns behind it stay
    from sehip import _lib
    out = torch.full((2, 5), -1, dtype=torch.int32, device="cuda")
    _lib.call("se_bootstrap_indices", 10, 0, 0, 2, 1, 3, out, 5)
    assert np.array_equal(out.cpu().numpy()[:, :3], bc.index_matrix(10, 0, 0, 2, 1, 3)) and (out[:, 3:] == -1).all()


@pytest.mark.parametrize("q,m,reps", [(1, 1, 4), (2, 3, 5), (3, 11, 3), (257, 16, 7), (1000, 1, 257), (5794, 11, 64), (65539, 2, 3)])
def test_means_of_dyadic_tables_are_exact(q, m, reps):
    """Every summation order is exact here: gathers, pitches and the division, bit for bit.  Odd and even pitches (the kernel's
    16-byte and 8-byte row loads), pad columns NaN on input and untouched on output."""
    import sehip
    ints = np.random.default_rng(q * 31 + m).integers(0, 1 << 20, (q, m))
    vals = ints / 1024.0
    for seed, rep0 in ((0, 0), (BIG_SEED, HIGH_REP)):
        want = bc.dyadic_means(ints, 10, seed, rep0, reps)
        for ldv, ldo in ((m + 1, m + 2), (m + 2 - m % 2, m + 1), (16 if m < 16 else 20, m + 3)):
            got = raw_means(vals, ldv, ldo, reps, seed, rep0)
            assert np.array_equal(got[:, :m], want), (q, m, reps, ldv, np.abs(got[:, :m] - want).max())
            assert (got[:, m:] == -7.0).all()
        # the binding: any row pitch (a column slice of a wider table; a contiguous table)
        wide = torch.zeros((q, m + 5), dtype=torch.float64, device="cuda")
        wide[:, 2:2 + m] = torch.from_numpy(vals).cuda()
        assert np.array_equal(sehip.bootstrap_means(wide[:, 2:2 + m], reps, seed=seed, rep0=rep0).cpu().numpy(), want)
        assert np.array_equal(sehip.bootstrap_means(torch.from_numpy(vals).cuda(), reps, seed=seed, rep0=rep0).cpu().numpy(), want)


@pytest.mark.parametrize("q,m,reps", [(3, 2, 4), (257, 11, 5), (5794, 3, 4)])
def test_means_of_general_float64_tables(q, m, reps):
    import sehip
    vals = np.random.default_rng(q + m).random((q, m))
    got = sehip.bootstrap_means(torch.from_numpy(vals).cuda(), reps, seed=11, rep0=2).cpu().numpy()
    exact = bc.exact_means(vals, 11, 2, reps)
    for i in range(reps):
        for c in range(m):
            err = abs(Fraction(float(got[i, c])) - exact[i][c])
            bound = q * Fraction(1, 2 ** 53) * exact[i][c]        # values are non-negative: mean|v| over the drawn rows is the exact mean
            assert err <= bound, (i, c, float(err), float(bound))


def test_determinism_chunks_and_streams():
    import sehip
    vals = np.random.default_rng(8).random((5794, 11))
    t = torch.from_numpy(vals).cuda()
    whole = sehip.bootstrap_means(t, 10, seed=5)
    again = sehip.bootstrap_means(t, 10, seed=5)
    parts = torch.cat([sehip.bootstrap_means(t, 4, seed=5, rep0=0), sehip.bootstrap_means(t, 6, seed=5, rep0=4)])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = sehip.bootstrap_means(t, 10, seed=5)
    side.synchronize()
    w = whole.cpu().numpy().view(np.int64)
    for name, x in (("again", again), ("chunks", parts), ("stream", other)):
        assert np.array_equal(x.cpu().numpy().view(np.int64), w), name
    assert not np.array_equal(sehip.bootstrap_means(t, 10, seed=6).cpu().numpy(), whole.cpu().numpy())       # the seed matters
    # one launch of many replicates (workgroups stride over them) against single-replicate launches
    many = sehip.bootstrap_means(t[:300], 20000, seed=5).cpu().numpy()
    for r in (0, 16383, 16384, 19999):
        assert np.array_equal(many[r], sehip.bootstrap_means(t[:300], 1, seed=5, rep0=r).cpu().numpy()[0]), r
    # the chunked host driver
    import bootstrap
    assert np.array_equal(bootstrap.replicate_means(t, 10, seed=5, chunk=3), whole.cpu().numpy())
    iv = bootstrap.confidence_intervals(t, reps=10, level=0.9, seed=5)
    assert np.array_equal(iv.rep_means, whole.cpu().numpy())
    lo, hi = np.quantile(iv.rep_means, [(1 - 0.9) / 2, (1 + 0.9) / 2], axis=0)
    assert np.array_equal(iv.lo, lo) and np.array_equal(iv.hi, hi) and np.abs(iv.mean - vals.mean(axis=0)).max() <= 1e-13


def test_a_nan_row_poisons_exactly_the_replicates_that_drew_it():
    import sehip
    q, m, reps, seed = 40, 3, 64, 3
    ints = np.random.default_rng(4).integers(0, 1 << 20, (q, m))
    vals = ints / 1024.0
    vals[17, 1] = np.nan
    drew = np.array([(bc.indices(q, seed, r, np.arange(q)) == 17).any() for r in range(reps)])
    assert drew.any() and not drew.all()        # (1 - 1/40)^40 = 36 % of the replicates miss the row
    got = sehip.bootstrap_means(torch.from_numpy(vals).cuda(), reps, seed=seed).cpu().numpy()
    assert np.array_equal(np.isnan(got[:, 1]), drew)
    assert not np.isnan(got[:, [0, 2]]).any()
    want = bc.dyadic_means(ints, 10, seed, 0, reps)
    assert np.array_equal(got[:, [0, 2]], want[:, [0, 2]]) and np.array_equal(got[~drew, 1], want[~drew, 1])


def test_invalid_arguments_and_empty_requests():
    import sehip
    t = torch.zeros((10, 4), dtype=torch.float64, device="cuda")
    assert sehip.bootstrap_means(t, 0).shape == (0, 4)          # no launch
    assert sehip.bootstrap_indices(10, 0).shape == (0, 10) and sehip.bootstrap_indices(10, 3, t0=4, count=0).shape == (3, 0)
    for bad in (lambda: sehip.bootstrap_means(t.float(), 3), lambda: sehip.bootstrap_means(t.cpu(), 3), lambda: sehip.bootstrap_means(t[0], 3),
                lambda: sehip.bootstrap_means(torch.zeros((10, 17), dtype=torch.float64, device="cuda"), 3),
                lambda: sehip.bootstrap_means(t[:0], 3), lambda: sehip.bootstrap_means(t, -1), lambda: sehip.bootstrap_means(t, 3, rep0=-1),
                lambda: sehip.bootstrap_means(t, 3, seed=1 << 64), lambda: sehip.bootstrap_indices(0, 3), lambda: sehip.bootstrap_indices(2 ** 31, 3, count=1),
                lambda: sehip.bootstrap_indices(10, 3, t0=4, count=7), lambda: sehip.bootstrap_indices(10, 3, t0=-1, count=2),
                lambda: sehip.bootstrap_indices(10, 3, rep0=-1)):
        with pytest.raises(sehip.SehipError):
            bad()


# ---- end to end ----

def synthetic_problem(tmp_path):
    """A synthetic dataset of 300 test images in 100 classes under the CIFAR-100 hierarchy: hierarchy file, test labels, features."""
    from datasets import get_data_generator
    from conftest import GOLDEN
    hpath = tmp_path / "cifar.parent-child.txt"
    with open(hpath, "w") as f:
        for p, c in np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))["edges"]:
            f.write("%d %d\n" % (p, c))
    ds = "synthetic:100x8x200x300"
    lab = list(get_data_generator(ds, None).labels_test)
    rng = np.random.default_rng(200)
    feats = (rng.standard_normal((100, 24))[lab] + 0.8 * rng.standard_normal((len(lab), 24))).astype(np.float32)
    return ds, hpath, lab, feats


def test_per_query_table_equals_the_dictionaries(tmp_path):
    import _qg_standins as qg
    from bootstrap import MetricTable
    ds, hpath, lab, feats = synthetic_problem(tmp_path)
    h, ks = qg.cifar_hierarchy(), [1, 10, 50, 100]
    ids = [1000 + 3 * i for i in range(len(lab))]
    by_id = dict(zip(ids, lab))
    for kw in (dict(compute_ahp=True, compute_ap=True), dict(compute_ahp=50, compute_ap=False)):
        means_d, per_q = h.hierarchical_precision_device(feats.copy(), by_id, ks, normalize=True, ids=ids, per_query=True, **kw)
        means_t, table = h.hierarchical_precision_device(feats.copy(), by_id, ks, normalize=True, ids=ids, per_query="table", **kw)
        means_f, none = h.hierarchical_precision_device(feats.copy(), by_id, ks, normalize=True, ids=ids, per_query=False, **kw)
        assert isinstance(table, MetricTable) and none is None and means_t == means_f
        assert table.values.is_cuda and table.values.dtype == torch.float64 and table.values.shape[0] == len(lab)
        assert list(table.ids) == ids and set(table.columns) == set(per_q) == set(means_d)
        rows = table.values.cpu().numpy()
        for name, c in table.columns.items():
            assert rows[:, c].tolist() == [per_q[name][i] for i in ids], name
    rk = {i: r for i, r in zip(range(len(lab)), np.argsort(-feats @ feats.T, axis=1, kind="stable").tolist())}
    means_d, per_q = h.hierarchical_precision_ranked(rk, lab, ks, compute_ahp=True, compute_ap=True, per_query=True, ignore_qids=False)
    means_t, table = h.hierarchical_precision_ranked(rk, lab, ks, compute_ahp=True, compute_ap=True, per_query="table", ignore_qids=False)
    rows = table.values.cpu().numpy()
    assert list(table.ids) == list(range(len(lab)))
    for name, c in table.columns.items():
        assert rows[:, c].tolist() == [per_q[name][i] for i in table.ids], name


def test_cli_bootstrap_tables_and_csv(tmp_path, capsys):
    """evaluate_rankings.main on two ranking files, one a worse copy of the other (the head of every list shuffled to its end): the
    first table is the one a run without the flags prints, every interval contains its mean, the worse file loses on every metric in
    every one of the 200 replicates (p = 2 / 201), and the CSV holds one line per (label, metric)."""
    import evaluate_rankings as evr
    import evaluate_retrieval as er
    ds, hpath, lab, feats = synthetic_problem(tmp_path)
    with open(tmp_path / "feat.pickle", "wb") as f:
        pickle.dump({"feat": {i: feats[i] for i in range(len(lab))}}, f)
    good = er.pairwise_retrieval(str(tmp_path / "feat.pickle"), True, return_generator=False)
    rng = np.random.default_rng(7)
    bad = {}
    for qid, lst in good.items():       # the 150 best of every list move behind the rest, in random order
        head = list(lst[:150])
        rng.shuffle(head)
        bad[qid] = list(lst[150:]) + head
    for name, r in (("good", good), ("bad", bad)):
        with open(tmp_path / (name + ".pickle"), "wb") as f:
            pickle.dump(r, f)
    common = ["--dataset", ds, "--data_root", str(tmp_path), "--hierarchy", str(hpath), "--plot_max", "0",
              "--ranking", str(tmp_path / "good.pickle"), "--ranking", str(tmp_path / "bad.pickle"), "--label", "good", "--label", "bad"]
    csv = tmp_path / "boot.csv"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        plain_perf = evr.main(common)
        plain = capsys.readouterr().out
        perf = evr.main(common + ["--bootstrap", "200", "--compare_to", "good", "--bootstrap_csv", str(csv)])
        out = capsys.readouterr().out
    assert perf == plain_perf and out.startswith(plain) and "P@1 (WUP)" in plain       # the first table, byte for byte
    assert "95% bootstrap intervals over queries (200 replicates)" in out and "Paired difference to good" in out
    lines = open(csv).read().splitlines()
    assert lines[0] == "label;metric;mean;lo;hi;delta;dlo;dhi;p" and len(lines) == 1 + 2 * len(er.METRICS)
    seen = set()
    for line in lines[1:]:
        label, metric, mean, lo, hi, delta, dlo, dhi, p = line.split(";")
        seen.add((label, metric))
        assert float(lo) <= float(mean) <= float(hi), line
        assert abs(float(mean) - perf[label][metric]) <= 1e-12, line
        if label == "good":
            assert (delta, dlo, dhi, p) == ("", "", "", "")
        else:
            assert abs(float(delta) - (perf["bad"][metric] - perf["good"][metric])) <= 1e-12 and float(delta) < 0, line
            assert float(dlo) <= float(delta) <= float(dhi) < 0, line
            assert float(p) == 2.0 / 201, line
    assert seen == {(l, m) for l in ("good", "bad") for m in er.METRICS}
    # the same seed gives the same file; another seed another one
    evr.main(common + ["--bootstrap", "200", "--compare_to", "good", "--bootstrap_csv", str(tmp_path / "again.csv")])
    evr.main(common + ["--bootstrap", "200", "--bootstrap_seed", "1", "--bootstrap_csv", str(tmp_path / "other.csv")])
    capsys.readouterr()
    assert open(tmp_path / "again.csv").read() == open(csv).read()
    other = open(tmp_path / "other.csv").read().splitlines()
    assert other[0] == "label;metric;mean;lo;hi" and other[1].split(";")[:3] == lines[1].split(";")[:3] and other[1] != ";".join(lines[1].split(";")[:5])


def test_cli_refuses_to_pair_other_queries(tmp_path, capsys):
    import evaluate_rankings as evr
    ds, hpath, lab, feats = synthetic_problem(tmp_path)
    n = len(lab)
    order = np.argsort(-feats @ feats.T, axis=1, kind="stable")
    np.savez(tmp_path / "all.npz", query_ids=np.arange(n), ranking=order)
    np.savez(tmp_path / "some.npz", query_ids=np.arange(n - 10), ranking=order[:n - 10])
    argv = ["--dataset", ds, "--data_root", str(tmp_path), "--hierarchy", str(hpath), "--plot_max", "0", "--keep_queries",
            "--ranking", str(tmp_path / "all.npz"), "--ranking", str(tmp_path / "some.npz"), "--bootstrap", "20", "--compare_to", "all"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(SystemExit) as e:
            evr.main(argv)
    assert "other queries" in str(e.value)
