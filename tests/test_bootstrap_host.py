"""CPU: the bootstrap index stream as include/sehip.h pins it (known answers of Philox4x32-10 and of the index map, on the NumPy
restatement the GPU tests compare the kernels with), the spread of the replicate means it gives, the host statistics of
bootstrap.py on hand-made replicates, the new command-line flags, and the argument checks of both entry points, which run
before any launch."""
import ctypes
import os

import numpy as np
import pytest

import _bootstrap_canon as bc

SEED = 0x0123456789abcdef


def words(x):
    return " ".join("%08x" % int(w[0]) for w in x)


def test_philox_known_answers():
    assert words(bc.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words(bc.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(bc.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_index_known_answers():
    assert bc.indices(10, 0, 0, np.arange(8)).tolist() == [8, 6, 3, 0, 3, 2, 4, 4]
    assert bc.indices(50000, SEED, 3, np.arange(8)).tolist() == [12775, 46982, 35639, 5992, 24011, 4518, 36338, 39594]
    assert bc.indices(2 ** 31 - 1, SEED, 3, np.arange(4)).tolist() == [548717665, 2017899782, 1530695275, 257359391]
    # the window form is the same stream
    assert np.array_equal(bc.index_matrix(50000, SEED, 2, 3, 3, 5)[1], bc.indices(50000, SEED, 3, np.arange(3, 8)))


@pytest.mark.parametrize("q", [1, 2, 3, 7, 2 ** 31 - 1])
def test_every_index_lies_inside_the_table(q):
    for seed in (0, 1, 0xfedcba9876543210):
        for r in (0, 5, 2 ** 32 + 5):
            idx = bc.indices(q, seed, r, np.arange(min(q, 4096)))
            assert idx.min() >= 0 and idx.max() < q


def test_spread_of_the_replicate_means_matches_theory():
    """seed 2024, q = 4096, R = 2000: the standard deviation of the replicate means against std(v) / sqrt(q).  Its sampling error is
    1 / sqrt(2 R) = 1.6 %; the bound is 10 %."""
    q, R = 4096, 2000
    v = np.random.default_rng(5).integers(0, 1024, q)
    means = bc.dyadic_means(v[:, None].astype(np.int64), 10, 2024, 0, R)[:, 0]
    ratio = means.std() / ((v / 1024).std() / np.sqrt(q))
    print("spread ratio", ratio)
    assert abs(ratio - 1.0) <= 0.10, ratio
    assert abs(means.mean() - (v / 1024).mean()) <= 6 * (v / 1024).std() / np.sqrt(q * R)       # and the centre stays: six standard errors


def test_exact_means_agree_with_the_dyadic_ones():
    ints = np.random.default_rng(1).integers(0, 1 << 20, (37, 3))
    a = bc.dyadic_means(ints, 10, 9, 4, 3)
    b = bc.exact_means(ints / 1024.0, 9, 4, 3)
    assert all(float(b[i][c]) == a[i, c] for i in range(3) for c in range(3))


def test_paired_difference_and_quantiles():
    import bootstrap
    R = 200
    rng = np.random.default_rng(3)
    rep_a = rng.random((R, 2))
    half = 1e-3 + rng.random(R // 2)
    shift = np.stack([0.01 + 0.02 * rng.random(R), np.concatenate([half, -half])], axis=1)     # column 0: all positive; column 1: symmetric about 0
    rep_b = rep_a + shift
    d = bootstrap.paired_difference(rep_a, rep_b, [0.5, 0.5], [0.52, 0.5], level=0.9)
    assert d.delta.tolist() == [0.52 - 0.5, 0.0]
    lo, hi = np.quantile(rep_b - rep_a, [(1 - 0.9) / 2, (1 + 0.9) / 2], axis=0)
    assert np.array_equal(d.lo, lo) and np.array_equal(d.hi, hi) and d.lo[0] > 0
    assert d.p[0] == 2.0 / (R + 1)          # every difference positive
    assert d.p[1] == 1.0                    # symmetric differences: 2 (1 + R / 2) / (R + 1) > 1
    back = bootstrap.paired_difference(rep_b, rep_a, [0.52, 0.5], [0.5, 0.5])
    assert back.delta[0] == 0.5 - 0.52 and back.p[0] == 2.0 / (R + 1) and back.hi[0] < 0
    # ties count on both sides
    tie = bootstrap.paired_difference(np.zeros((9, 1)), np.zeros((9, 1)), [0.0], [0.0])
    assert tie.p[0] == 1.0 and tie.lo[0] == 0.0 == tie.hi[0]
    with pytest.raises(ValueError):
        bootstrap.paired_difference(rep_a, rep_b[:5], [0, 0], [0, 0])
    with pytest.raises(ValueError):
        bootstrap.paired_difference(rep_a, rep_b, [0, 0], [0, 0], level=1.0)


def test_formatting_helpers(tmp_path, capsys):
    import bootstrap
    rep = np.linspace(0.0, 1.0, 101)[:, None] * np.array([[1.0, 2.0]])
    iv = {"a": bootstrap.Intervals(np.array([0.5, 1.0]), *np.quantile(rep, [0.025, 0.975], axis=0), rep),
          "b": bootstrap.Intervals(np.array([0.6, 1.1]), *np.quantile(rep + 0.1, [0.025, 0.975], axis=0), rep + 0.1)}
    assert bootstrap.format_interval(0.5, 0.025, 0.975) == "0.5000 [0.0250, 0.9750]"
    assert bootstrap.format_difference(0.1, 0.05, 0.15, 2 / 201) == "+0.1000 [+0.0500, +0.1500] p=0.00995"
    bootstrap.print_intervals(iv, ["m1", "m2"], 0.95, 101)
    out = capsys.readouterr().out
    assert "95% bootstrap intervals" in out and "0.5000 [0.0250, 0.9750]" in out and "1.1000 [0.1500, 2.0500]" in out
    diff = {"b": bootstrap.paired_difference(iv["a"].rep_means, iv["b"].rep_means, iv["a"].mean, iv["b"].mean)}
    bootstrap.print_differences(diff, ["m1", "m2"], "a", 0.95)
    assert "Paired difference to a" in capsys.readouterr().out
    bootstrap.write_csv(iv, diff, ["m1", "m2"], str(tmp_path / "b.csv"))
    lines = open(tmp_path / "b.csv").read().splitlines()
    assert lines[0] == "label;metric;mean;lo;hi;delta;dlo;dhi;p" and len(lines) == 5
    assert lines[1].startswith("a;m1;0.5;") and lines[1].endswith(";;;;") and abs(float(lines[1].split(";")[3]) - 0.025) <= 1e-12
    cells = lines[3].split(";")
    assert cells[:2] == ["b", "m1"] and float(cells[5]) == 0.6 - 0.5 and float(cells[8]) == 2 / 102
    bootstrap.write_csv(iv, {}, ["m1"], str(tmp_path / "c.csv"))
    lines = open(tmp_path / "c.csv").read().splitlines()
    assert lines[0] == "label;metric;mean;lo;hi" and len(lines) == 3 and lines[2].startswith("b;m1;0.6;")


RETRIEVAL = ["--dataset", "x", "--data_root", "y", "--hierarchy", "h", "--feat", "a.pickle", "--feat", "b.pickle", "--label", "A"]
RANKINGS = ["--dataset", "x", "--data_root", "y", "--hierarchy", "h", "--ranking", "a.npz", "--ranking", "b.npz", "--label", "A"]
FLAGS = ("bootstrap", "bootstrap_seed", "confidence", "compare_to", "bootstrap_csv")


@pytest.mark.parametrize("tool,base", [("evaluate_retrieval", RETRIEVAL), ("evaluate_rankings", RANKINGS)])
def test_parser_flags(tool, base, monkeypatch, capsys):
    mod = __import__(tool)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = mod.parse_args(base)
    assert not any(hasattr(args, f) for f in FLAGS)         # absent unless given
    args = mod.parse_args(base + ["--bootstrap", "500"])
    assert args.bootstrap == 500 and not any(hasattr(args, f) for f in FLAGS[1:])
    args = mod.parse_args(base + ["--bootstrap", "500", "--bootstrap_seed", "7", "--confidence", "0.9", "--compare_to", "b", "--bootstrap_csv", "o.csv"])
    assert (args.bootstrap_seed, args.confidence, args.compare_to, args.bootstrap_csv) == (7, 0.9, "b", "o.csv")     # 'b': the second file's base name
    assert mod.parse_args(base + ["--bootstrap", "5", "--compare_to", "A"]).compare_to == "A"
    for bad, text in ((["--compare_to", "A"], "needs --bootstrap"), (["--bootstrap_csv", "o.csv"], "needs --bootstrap"),
                      (["--bootstrap", "5", "--compare_to", "nobody"], "none of the labels"), (["--bootstrap", "0"], "positive"),
                      (["--bootstrap", "5", "--confidence", "1.5"], "between 0 and 1")):
        with pytest.raises(SystemExit):
            mod.parse_args(base + bad)
        assert text in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--bootstrap", "5"])
    assert "one process" in capsys.readouterr().err
    assert not hasattr(mod.parse_args(base), "bootstrap")   # several ranks without the flag parse as before


def test_header_declares_and_binding_derives_both_symbols():
    import sehip
    from sehip import _lib
    src = open(_lib.HEADER_PATH).read()
    assert "#define SE_BOOTSTRAP_COLS_MAX 16" in src and "Philox4x32-10" in src and "0xD2511F53" in src and "0xCD9E8D57" in src
    means, idx = _lib.PROTOTYPES["se_bootstrap_means"], _lib.PROTOTYPES["se_bootstrap_indices"]
    assert [p.ctype for p in means.params] == ["double *", "int64_t", "int64_t", "int", "int64_t", "int64_t", "int64_t", "double *", "int64_t"]
    assert [p.ctype for p in idx.params] == ["int64_t"] * 6 + ["int32_t *", "int64_t"]
    assert means.stream and idx.stream and means.restype == idx.restype == "int"
    assert sehip.BOOTSTRAP_COLS_MAX == _lib.DEFINES["SE_BOOTSTRAP_COLS_MAX"] == 16
    assert callable(sehip.bootstrap_means) and callable(sehip.bootstrap_indices)
    assert sehip.ops._seed_arg(0xfedcba9876543210) == 0xfedcba9876543210 - (1 << 64) and sehip.ops._seed_arg(5) == 5


def test_argument_checks_run_before_any_launch():
    """Both entry points validate on the host; an empty request is SE_OK without a launch (no device is needed to ask)."""
    import sehip
    lib = sehip.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    OK, INVALID = 0, -1
    assert lib.se_bootstrap_means(z, 4, 10, 4, 0, 0, 0, z, 4, z) == OK                 # reps == 0
    assert lib.se_bootstrap_means(z, 4, 10, 4, 0, 0, 3, one, 4, z) == INVALID           # NULL with work to do
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_bootstrap_means(one, 4, 0, 4, 0, 0, 0, one, 4, z) == INVALID          # q < 1
    assert lib.se_bootstrap_means(one, 4, 2 ** 31, 4, 0, 0, 0, one, 4, z) == INVALID    # q > 2^31 - 1
    assert lib.se_bootstrap_means(one, 4, 10, 0, 0, 0, 0, one, 4, z) == INVALID         # m < 1
    assert lib.se_bootstrap_means(one, 32, 10, 17, 0, 0, 0, one, 32, z) == INVALID      # m > SE_BOOTSTRAP_COLS_MAX
    assert lib.se_bootstrap_means(one, 3, 10, 4, 0, 0, 0, one, 4, z) == INVALID         # ldv < m
    assert lib.se_bootstrap_means(one, 4, 10, 4, 0, 0, 0, one, 3, z) == INVALID         # ldo < m
    assert lib.se_bootstrap_means(one, 4, 10, 4, 0, -1, 0, one, 4, z) == INVALID        # rep0 < 0
    assert lib.se_bootstrap_means(one, 4, 10, 4, 0, 0, -1, one, 4, z) == INVALID        # reps < 0
    assert lib.se_bootstrap_indices(10, 0, 0, 0, 0, 10, z, 10, z) == OK                 # reps == 0
    assert lib.se_bootstrap_indices(10, 0, 0, 3, 4, 0, z, 0, z) == OK                   # count == 0
    assert lib.se_bootstrap_indices(10, 0, 0, 3, 0, 10, z, 10, z) == INVALID            # NULL with work to do
    assert lib.se_bootstrap_indices(0, 0, 0, 3, 0, 0, one, 0, z) == INVALID             # q < 1
    assert lib.se_bootstrap_indices(2 ** 31, 0, 0, 3, 0, 1, one, 1, z) == INVALID
    assert lib.se_bootstrap_indices(10, 0, 0, 3, 4, 7, one, 7, z) == INVALID            # window past q
    assert b"window" in lib.se_last_error()
    assert lib.se_bootstrap_indices(10, 0, 0, 3, -1, 2, one, 2, z) == INVALID
    assert lib.se_bootstrap_indices(10, 0, 0, 3, 0, 5, one, 4, z) == INVALID            # ldo < count
    assert lib.se_bootstrap_indices(10, 0, -2, 3, 0, 5, one, 5, z) == INVALID


def test_bindings_refuse_to_run_without_a_device():
    import torch
    import sehip
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    with pytest.raises(sehip.SehipError):
        sehip.bootstrap_means(torch.zeros((4, 2), dtype=torch.float64), 3)
    with pytest.raises(sehip.SehipError):
        sehip.bootstrap_indices(10, 3)
