"""Recall-precision curve and mAP (plot_recall_precision.py:52-79) without a GPU: the host mirror against the golden values the
reference's own script produced (tools/make_recprec_golden.py), the device driver's host logic through CPU stand-ins of its
kernels, the CLI's flags, and the host-side argument checks of the two C entry points."""
import ctypes
import glob
import os
import warnings

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = sorted(os.path.basename(p)[len("recprec_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "recprec_*.npz")))


def _fixture(name):
    return np.load(os.path.join(GOLDEN, "recprec_%s.npz" % name))


def _canon_rank(features, normalize):
    from oracle import retrieval_oracle as ro
    return ro.canon_retrieval(features, normalize)[1]


# ---- CPU stand-ins of the device kernels: the same contracts, written plainly ----

def _cpu_kernels(tile_rows_default=None):
    from oracle import retrieval_oracle as ro

    def ranking_tiles(features, normalize=False, tile_rows=None, kblocks=None):
        f = features.numpy().copy()
        if normalize:
            f = ro.canon_normalize_rows(f)
        metric = ro.METRIC_COSINE if normalize else ro.METRIC_EUCLID
        n = len(f)
        step = tile_rows or tile_rows_default or n
        for r0 in range(0, n, step):
            pd = ro.canon_pdist(f[r0:r0 + step], f, metric)
            yield r0, torch.from_numpy(ro.canon_rank_rows(pd))

    def relevant_positions(rank, cls, qcls, qidx, hit_off, num_classes=None, total=None):
        rank, cls, qcls, hit_off = rank.numpy(), cls.numpy(), qcls.numpy(), hit_off.numpy()
        qidx = None if qidx is None else qidx.numpy()
        out = np.zeros(int(hit_off[-1]), dtype=np.int32)
        for i in range(len(rank)):
            row = rank[i] if qidx is None else rank[i][rank[i] != qidx[i]]
            pos = np.flatnonzero(cls[row] == qcls[i]) + 1
            R = int(hit_off[i + 1] - hit_off[i])
            out[hit_off[i]:hit_off[i] + R] = pos[:R]
        return torch.from_numpy(out)

    def recall_precision_reduce(hit_pos, hit_off, order, class_start, class_off, bins, ap, prec_sum, first_miss, bin_sum, bin_count):
        hp, ho, order, cs, co = hit_pos.numpy(), hit_off.numpy(), order.numpy(), class_start.numpy(), class_off.numpy()
        for q in range(len(order)):
            R = int(ho[q + 1] - ho[q])
            ap[q] = (np.arange(1, R + 1) / hp[ho[q]:ho[q + 1]]).sum() / R if R else 0.0
        for c in range(len(cs) - 1):
            Rc = int(co[c + 1] - co[c])
            for q in order[cs[c]:cs[c + 1]]:
                p = hp[ho[q]:ho[q + 1]]
                if Rc == 0:
                    continue
                j = np.arange(1, Rc + 1)
                prec_sum[co[c]:co[c + 1]] += torch.from_numpy(j / p)
                first_miss[c] += int(p[0] > 1)
                if bins:
                    b = ((j / Rc) * bins).astype(np.int64)
                    best = np.full(bins + 1, -1.0)
                    np.maximum.at(best, b, j / p)
                    if p[0] > 1:
                        best[0] = max(best[0], 0.0)
                    have = best >= 0
                    bin_sum[c, torch.from_numpy(have)] += torch.from_numpy(best[have])
                    bin_count[c, torch.from_numpy(have)] += 1
        return ap

    return {"ranking_tiles": ranking_tiles, "relevant_positions": relevant_positions,
            "recall_precision_reduce": recall_precision_reduce, "device": torch.device("cpu")}


def test_fixtures_present():
    assert set(FIXTURES) >= {"d24_cos", "d24_euc", "d100_cos", "d100_euc"}


@pytest.mark.parametrize("name", FIXTURES)
def test_host_mirror_reproduces_the_reference(name):
    """recall_precision_host on the canonical ranking == what the reference's script computed: the same float64 levels, means and
    mAP to 1e-12, every per-query AP to 1e-12."""
    from recall_precision import recall_precision_host
    g = _fixture(name)
    rank = _canon_rank(g["features"], bool(g["normalize"]))
    for b in g["bins"].tolist():
        levels, means, mAP, aps = recall_precision_host(rank, g["labels"], bins=b or None)
        assert np.array_equal(levels, g["levels_%d" % b]), (name, b)
        assert np.abs(means - g["means_%d" % b]).max() <= 1e-12, (name, b)
        assert abs(mAP - g["aps_%d" % b].mean()) <= 1e-12
        assert np.abs(aps - g["aps_%d" % b]).max() <= 1e-12


@pytest.mark.parametrize("tile_rows", [None, 37, 128])
@pytest.mark.parametrize("bins", [None, 1, 7, 1000])
def test_device_driver_host_logic_matches_host_mirror(tile_rows, bins):
    """recall_precision_device with CPU stand-ins: class-split tiles, binned and unbinned, agree with the host mirror."""
    from recall_precision import recall_precision_device, recall_precision_host
    g = _fixture("d24_euc")
    rank = _canon_rank(g["features"], False)
    want = recall_precision_host(rank, g["labels"], bins=bins)
    got = recall_precision_device(g["features"].copy(), g["labels"].tolist(), bins=bins, tile_rows=tile_rows, kernels=_cpu_kernels())
    assert np.array_equal(got[0], want[0])
    assert np.abs(got[1] - want[1]).max() <= 1e-12
    assert abs(got[2] - want[2]) <= 1e-12
    assert np.abs(got[3] - want[3]).max() <= 1e-12


def test_device_driver_dict_ids_and_normalize():
    """Features as a {id: vector} dict (pairwise_retrieval's input form) and labels as a mapping keyed by those ids."""
    from recall_precision import recall_precision_device, recall_precision_host
    g = _fixture("d24_cos")
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(g["labels"]))
    ids = ["img%04d" % (7 * int(i) + 3) for i in perm]
    feats = {k: g["features"][i] for k, i in zip(ids, perm)}
    labels = {k: "class-%d" % g["labels"][i] for k, i in zip(ids, perm)}
    got = recall_precision_device(feats, labels, normalize=True, bins=10, tile_rows=50, kernels=_cpu_kernels())
    rank = _canon_rank(g["features"][perm], True)
    want = recall_precision_host(rank, [labels[k] for k in ids], bins=10)
    assert np.array_equal(got[0], want[0])
    assert np.abs(got[1] - want[1]).max() <= 1e-12 and abs(got[2] - want[2]) <= 1e-12
    # relabelling does not change the curve: the fixture's own values
    assert np.array_equal(got[0], g["levels_10"]) and np.abs(got[1] - g["means_10"]).max() <= 1e-12


@pytest.mark.parametrize("bins", [None, 7])
def test_singleton_class(bins):
    """A class of one item: its query gets AP 0 and no curve points; one warning per call names the count."""
    from recall_precision import recall_precision_device, recall_precision_host
    g = _fixture("d24_euc")
    labels = g["labels"].copy()
    labels[[5, 77]] = [1000, 1001]            # two singleton classes
    rank = _canon_rank(g["features"], False)
    for fn in (lambda: recall_precision_host(rank, labels, bins=bins),
               lambda: recall_precision_device(g["features"].copy(), labels.tolist(), bins=bins, tile_rows=64, kernels=_cpu_kernels())):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            levels, means, mAP, aps = fn()
        msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
        assert len(msgs) == 1 and msgs[0].startswith("recall-precision: 2 queries"), msgs
        assert aps[5] == 0.0 and aps[77] == 0.0 and abs(mAP - aps.mean()) <= 1e-15
        assert np.isfinite(levels).all() and np.isfinite(means).all()
    with pytest.warns(RuntimeWarning):
        a = recall_precision_host(rank, labels, bins=bins)
    with pytest.warns(RuntimeWarning):
        b = recall_precision_device(g["features"].copy(), labels.tolist(), bins=bins, tile_rows=64, kernels=_cpu_kernels())
    assert np.array_equal(a[0], b[0]) and np.abs(a[1] - b[1]).max() <= 1e-12


def test_cli_parser_matches_the_reference_flags():
    """Flags, defaults, requiredness, append actions and groups of the reference (plot_recall_precision.py:21-32); the extensions
    live in a group of their own."""
    import plot_recall_precision as prp
    p = prp.build_parser()
    groups = {g.title: {a.dest: a for a in g._group_actions} for g in p._action_groups}
    want = {"Dataset": {"dataset": (True, None, "store"), "data_root": (True, None, "store"), "classes_from": (False, None, "store")},
            "Features": {"feat": (True, None, "append"), "label": (False, None, "append"), "norm": (False, None, "append")},
            "Plot": {"bins": (False, None, "store")}}
    for title, flags in want.items():
        assert set(groups[title]) == set(flags), title
        for dest, (req, default, kind) in flags.items():
            a = groups[title][dest]
            assert a.required == req and a.default == default and a.option_strings == ["--" + dest], dest
            assert type(a).__name__ == {"store": "_StoreAction", "append": "_AppendAction"}[kind], dest
    assert set(groups["Extensions of this build (not in the reference)"]) == {"save", "csv", "kblocks"}
    args = p.parse_args(["--dataset", "x", "--data_root", "y", "--feat", "a.pkl", "--feat", "b.pkl", "--norm", "yes", "--norm", "0",
                         "--bins", "10"])
    assert args.feat == ["a.pkl", "b.pkl"] and args.norm == [True, False] and args.bins == 10
    with pytest.raises(SystemExit):
        p.parse_args(["--dataset", "x", "--data_root", "y"])          # --feat is required


def test_csv_writer(tmp_path):
    import plot_recall_precision as prp
    from collections import OrderedDict
    curves = OrderedDict(a=(np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.75, 1 / 3]), 0.5))
    prp.write_csv(curves, str(tmp_path / "c.csv"))
    rows = (tmp_path / "c.csv").read_text().splitlines()
    assert rows[0] == "feature,level,mean_precision" and len(rows) == 4
    assert float(rows[3].split(",")[2]) == 1 / 3                      # full float64 round trip


def test_argument_validation_without_gpu():
    """Host-side checks of se_relevant_positions / se_recall_precision_reduce run before any launch."""
    import sehip
    lib = sehip.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    assert lib.se_relevant_positions(z, 4, 2, 4, z, 4, z, z, 3, z, z, z) == -1
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_relevant_positions_r16(one, 4, 2, 4, one, 70000, one, z, 3, one, one, z) == -1        # 16-bit ranks, gallery > 65536
    assert b"16-bit" in lib.se_last_error()
    assert lib.se_relevant_positions(one, 3, 2, 4, one, 4, one, z, 3, one, one, z) == -1                # ldr < list_len
    assert b"leading dimension" in lib.se_last_error()
    assert lib.se_relevant_positions(one, 4, 0, 4, one, 4, one, z, 3, one, one, z) == 0                 # empty problem is OK
    assert lib.se_recall_precision_reduce(z, z, 2, z, z, 3, z, 0, 0, z, z, z, z, z, z) == -1
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_recall_precision_reduce(one, one, 2, one, one, 3, one, 4, 5, one, one, one, z, z, z) == -1   # bins without buffers
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_recall_precision_reduce(one, one, 2, one, one, 3, one, 4, -1, one, one, one, z, z, z) == -1
    assert b"bad shape" in lib.se_last_error()
    assert lib.se_recall_precision_reduce(one, one, 0, one, one, 3, one, 4, 0, one, one, one, z, z, z) == 0


def test_ops_refuse_without_gpu():
    """No CPU fallback: the ops raise SehipError for host tensors."""
    import sehip
    t = torch.zeros((2, 4), dtype=torch.int32)
    i = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(sehip.SehipError):
        sehip.relevant_positions(t, torch.zeros(4, dtype=torch.int32), i, None, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(sehip.SehipError):
        sehip.recall_precision_reduce(i, torch.zeros(3, dtype=torch.int64), i, torch.zeros(2, dtype=torch.int32),
                                      torch.zeros(2, dtype=torch.int64), 0, torch.zeros(2, dtype=torch.float64),
                                      torch.zeros(0, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
