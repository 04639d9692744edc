"""CPU: the host layer of the mistake metrics and of CRM decoding -- ClassHierarchy.tree_risk_encoding / height_table against the
explicit-set canon (tests/_tree_risk_canon.py), mistakes.mistake_metrics on hand values, mistakes.crm_classification on both of its
paths through CPU stand-ins, the --mistakes / --crm command line of evaluate_classification_accuracy.py, and the argument checks of
se_tree_risk_topk through raw ctypes."""
import ctypes
import io
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _tree_risk_canon as tc

TREES = ["cifar", "cub", "ilsvrc", "rand37", "rand300", "inat400"]


# ---- the encoding ----

@pytest.mark.parametrize("name", TREES)
def test_range_formula_on_the_encoding_equals_the_canon_exactly(name):
    h, classes = tc.tree(name)
    enc = h.tree_risk_encoding(classes)
    C = len(classes)
    for k in ("pos", "path_off", "lvl_lo", "lvl_hi", "lvl_h", "own_h"):
        assert enc[k].dtype == np.int32, k
    assert sorted(enc["pos"].tolist()) == list(range(C)) and enc["path_off"][0] == 0 and enc["path_off"][-1] == len(enc["lvl_h"])
    levels = np.diff(enc["path_off"])
    assert enc["max_levels"] == levels.max() <= 32 and enc["max_height"] == h.max_height
    last = enc["path_off"][1:] - 1
    assert (enc["lvl_lo"][last] == 0).all() and (enc["lvl_hi"][last] == C).all()            # every path ends at the whole tree
    assert enc["lvl_h"].max() == h.max_height and (enc["own_h"] == [h.heights[c] for c in classes]).all()
    hx = h.hxe_encoding(classes)                                                            # one walk: the same ranges
    for k in ("pos", "path_off", "lvl_lo", "lvl_hi"):
        assert np.array_equal(enc[k], hx[k]), k
    H = tc.height_table(h, classes)
    P = tc.grid_probs(4, C, seed=C)
    want = tc.risks(P, H)
    got = tc.range_formula(P, enc)
    assert np.array_equal(got, want)
    ties = sum(len(np.unique(r[:6])) < 6 for r in np.sort(want, axis=1))
    if name == "cub":
        assert ties > 0                                                                     # the tie rule is reachable


def test_random_trees_have_chains_and_empty_inner_nodes():
    empty = 0
    for name in ("rand37", "rand300"):
        h, classes = tc.tree(name)
        enc = h.tree_risk_encoding(classes)
        walked = [len(h.all_hypernym_depths(c)) - 1 for c in classes]
        assert (np.diff(enc["path_off"]) < walked).any()                                    # an edge was dropped: a chain
        empty += len(h.nodes - set().union(*[set(h.all_hypernym_depths(c)) for c in classes]))
    assert empty > 0                                                                        # inner nodes without a class below them


def test_hxe_encoding_is_unchanged():
    """Today's hxe_encoding, restated from the explicit walk, for CIFAR: every array bit for bit."""
    h, classes = tc.tree("cifar")
    top, parent, _, d, rng = h._class_tree(classes)
    lo, hi, w, off = [], [], [], [0]
    for c in classes:
        node = c
        while node != top:
            up = parent[node]
            if rng[up] != rng[node]:
                lo.append(rng[up][0])
                hi.append(rng[up][1])
                w.append(float(np.exp(-0.25 * d[node])))
            node = up
        off.append(len(lo))
    want = {"pos": np.asarray([rng[c][0] for c in classes], dtype=np.int32), "path_off": np.asarray(off, dtype=np.int32),
            "lvl_lo": np.asarray(lo, dtype=np.int32), "lvl_hi": np.asarray(hi, dtype=np.int32), "lvl_w": np.asarray(w, dtype=np.float32)}
    got = h.hxe_encoding(classes, alpha=0.25)
    assert sorted(got) == sorted(list(want) + ["max_levels"]) and got["max_levels"] == int(np.diff(off).max())
    for k, v in want.items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v), k
    risk = h.tree_risk_encoding(classes)                    # the same walk serves both encodings
    assert all(np.array_equal(risk[k], want[k]) for k in ("pos", "path_off", "lvl_lo", "lvl_hi"))
    custom = h.hxe_encoding(classes, weights=lambda node: 2.0)
    assert (custom["lvl_w"] == 2.0).all() and np.array_equal(custom["lvl_lo"], want["lvl_lo"])


def test_a_dag_and_a_forest_are_refused():
    h, classes = tc.tree("wordnet_dag")
    with pytest.raises(ValueError, match="not a tree"):
        h.tree_risk_encoding(classes)
    forest = tc._hierarchy([(10, 0), (10, 1), (11, 2), (11, 3)])
    assert forest.hxe_encoding([0, 1, 2, 3])["max_levels"] == 2                             # the losses take a virtual top
    with pytest.raises(ValueError, match="forest"):
        forest.tree_risk_encoding([0, 1, 2, 3])
    with pytest.raises(ValueError, match="ancestor"):
        tc._hierarchy([(10, 0), (0, 1)]).tree_risk_encoding([0, 1])


def test_height_table_equals_the_canon():
    h, classes = tc.tree("cifar")
    seen = []

    def tables(classes_, distance=False, want_wup=True, device=None):
        seen.append((distance, want_wup))
        return None, torch.from_numpy(1.0 - h.similarity_tables(classes_)[1])               # h / H with float64 round-off

    table = h.height_table(classes, tables=tables)
    assert seen == [(True, False)] and table.dtype == torch.int32
    assert np.array_equal(table.numpy(), tc.height_table(h, classes))
    with pytest.raises(AssertionError):
        h.height_table(classes, tables=lambda *a, **k: (None, torch.full((3, 3), 0.3 / h.max_height, dtype=torch.float64)))


# ---- the metrics ----

def test_mistake_metrics_on_hand_values():
    from mistakes import metric_names, mistake_metrics
    H = np.array([[0, 1, 3], [1, 0, 3], [3, 3, 0]])
    y = np.array([0, 1, 2, 2])
    right = np.array([[0, 1, 2], [1, 0, 2], [2, 0, 1], [2, 1, 0]])
    out = mistake_metrics(right, y, H, [1, 2])
    assert list(out) == ["Hier. Dist@1", "Hier. Dist@2"]                                    # no mistake: no severity
    assert out["Hier. Dist@1"] == 0.0 and out["Hier. Dist@2"] == (1 + 1 + 3 + 3) / 8
    wrong = np.array([[1, 0, 2], [1, 0, 2], [0, 2, 1], [2, 1, 0]])
    out = mistake_metrics(wrong, y, torch.from_numpy(H), [1, 3])
    assert list(out) == metric_names([1, 3]) == ["Mistake Severity", "Hier. Dist@1", "Hier. Dist@3"]
    assert out["Mistake Severity"] == (1 + 3) / 2 and out["Hier. Dist@1"] == (1 + 0 + 3 + 0) / 4
    assert out["Hier. Dist@3"] == ((1 + 0 + 3) + (0 + 1 + 3) + (3 + 0 + 3) + (0 + 3 + 3)) / 12
    assert mistake_metrics(wrong[:, 0], y, H, [1]) == OrderedDict([("Mistake Severity", 2.0), ("Hier. Dist@1", 1.0)])
    with pytest.raises(ValueError):
        mistake_metrics(wrong, y, H, [4])
    rng = np.random.default_rng(0)
    h, classes = tc.tree("cifar")
    Hc = tc.height_table(h, classes)
    pred, yy = np.stack([rng.permutation(100)[:20] for _ in range(50)]), rng.integers(0, 100, 50)
    assert dict(mistake_metrics(pred, yy, Hc, [1, 5, 20])) == tc.metrics(pred, yy, Hc, [1, 5, 20])


# ---- crm_classification through CPU stand-ins ----

def cpu_kernels(calls):
    def tree_risk_topk(P, enc, top, return_risk=False):
        calls.append(("tree_risk_topk", tuple(P.shape), top))
        cls, risk = tc.lists(tc.range_formula(P.numpy(), enc), top)
        return torch.from_numpy(cls), torch.from_numpy(risk)

    def pairwise_dist(a, b, cosine, sqa, sqb, kblocks, out=None):
        calls.append(("pairwise_dist", tuple(a.shape), tuple(b.shape), cosine))
        assert a.dtype == b.dtype == torch.float32
        return -(a @ b.T)

    def topk_rows(pd, k):
        calls.append(("topk_rows", tuple(pd.shape), k))
        cls, d = tc.lists(pd.numpy(), k)
        return torch.from_numpy(d.astype(np.float32)), torch.from_numpy(cls)

    return {"tree_risk_topk": tree_risk_topk, "pairwise_dist": pairwise_dist, "topk_rows": topk_rows, "device": torch.device("cpu")}


def test_crm_classification_takes_the_kernel_on_a_tree():
    from mistakes import crm_classification
    h, classes = tc.tree("cub")
    P = tc.grid_probs(7, len(classes), seed=1)
    calls = []
    got = crm_classification(P, h, classes, top=6, kernels=cpu_kernels(calls))
    assert calls == [("tree_risk_topk", (7, 200), 6)]
    assert got.dtype == np.int32 and np.array_equal(got, tc.lists(tc.risks(P, tc.height_table(h, classes)), 6)[0])
    with pytest.raises(ValueError):
        crm_classification(P, h, classes, top=33, kernels=cpu_kernels(calls))
    with pytest.raises(ValueError):
        crm_classification(P[:, :5], h, classes, top=3, kernels=cpu_kernels(calls))


@pytest.mark.parametrize("name", ["wordnet_dag", "cifar"])
def test_crm_classification_takes_the_dense_path_otherwise(name, monkeypatch):
    import mistakes
    import sehip
    h, classes = tc.tree(name)
    if name == "cifar":                                     # a tree with more classes than the kernel takes
        monkeypatch.setattr(sehip, "TREE_RISK_MAX_CLASSES", 99)
    monkeypatch.setattr(mistakes, "DENSE_TILE_ROWS", 4)
    H = tc.height_table(h, classes)
    C = len(classes)
    assert C * 64 * H.max() < 2 ** 24                       # every float32 sum of the grid rows is exact
    P = tc.grid_probs(6, C, seed=2)
    calls = []
    kernels = cpu_kernels(calls)
    kernels["height_table"] = lambda classes_, device=None: torch.from_numpy(H.astype(np.int32))
    got = mistakes.crm_classification(torch.from_numpy(P), h, classes, top=5, kernels=kernels)
    assert [c[0] for c in calls] == ["pairwise_dist", "topk_rows"] * 2 and calls[0] == ("pairwise_dist", (4, C), (C, C), True)
    assert np.array_equal(got, tc.lists(tc.risks(P, H), 5)[0])


# ---- command line ----

def todays_table(perf, metrics):
    """print_performance as it was before the extension flags existed."""
    out = io.StringIO()
    width = max(len(lbl) for lbl in perf)
    out.write("\n" + " | ".join([" " * width] + ["{:^6s}".format(m) for m in metrics]) + "\n")
    out.write("-" * (width + sum(3 + max(6, len(m)) for m in metrics)) + "\n")
    for lbl, res in perf.items():
        out.write("{:{}s} | {}\n".format(lbl, width, " | ".join(
            "{:>{}.4f}".format(res[m], max(len(m), 6)) if m in res else "{:>{}s}".format("--", max(len(m), 6)) for m in metrics)))
    out.write("\n")
    return out.getvalue()


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from class_hierarchy import ClassHierarchy
    from datasets import get_data_generator
    ds = "synthetic:10x8x40x30"
    data = get_data_generator(ds, "-")
    hier = tmp_path_factory.mktemp("mistakes") / "hierarchy.txt"
    hier.write_text("".join("%d %d\n" % (100 + c // 5, c) for c in range(10)) + "200 100\n200 101\n")
    hierarchy = ClassHierarchy.from_file(str(hier), id_type=int)
    H = tc.height_table(hierarchy, data.classes)
    rng = np.random.default_rng(5)
    outputs = {m: tc.grid_probs(data.num_test, 10, seed=s) for m, s in (("m1", 11), ("m2", 12))}
    svm_rank = np.stack([rng.permutation(10) for _ in range(data.num_test)])
    calls = []

    def rank(out):
        return tc.lists(-np.asarray(out, dtype=np.float64), 10)[0]

    def crm(out, hierarchy_, classes, top, logits):
        calls.append(("crm", top, logits))
        P = torch.softmax(torch.from_numpy(out), dim=-1).numpy() if logits else out
        return tc.lists(tc.risks(P, H), top)[0]

    modes = {"probs": lambda d, model, layer, custom, bs: calls.append(("probs", model)) or outputs[model],
             "prob": lambda d, model, layer, custom, bs: calls.append(("prob", model)) or rank(outputs[model]),
             "svm": lambda *a: calls.append(("svm", a[1])) or svm_rank,
             "rank": rank, "crm": crm, "height_table": lambda: torch.from_numpy(H.astype(np.int32))}
    base = ["--dataset", ds, "--data_root", "-", "--model", "m1", "--layer", "-1", "--prob_features", "1",
            "--model", "m2", "--layer", "-1", "--prob_features", "1", "--model", "m3", "--layer", "-1", "--prob_features", "0"]
    return dict(ds=ds, data=data, hier=str(hier), hierarchy=hierarchy, H=H, outputs=outputs, svm_rank=svm_rank, calls=calls, modes=modes,
                base=base, rank=rank)


def test_cli_columns_and_crm_rows(cli, capsys):
    import evaluate_classification_accuracy as eca
    data, H, calls = cli["data"], cli["H"], cli["calls"]
    y = np.asarray(data.labels_test)
    del calls[:]
    plain = eca.main(cli["base"] + ["--hierarchy", cli["hier"]], modes=cli["modes"])
    printed = capsys.readouterr().out
    assert calls == [("prob", "m1"), ("prob", "m2"), ("svm", "m3")]                         # without the flags: today's modes ...
    assert list(plain) == ["m1", "m2", "m3"] and all(sorted(r) == sorted(eca.METRICS) for r in plain.values())
    assert printed == todays_table(plain, eca.METRICS)                                      # ... and today's table, byte for byte
    assert plain["m3"] == eca.evaluate(cli["svm_rank"], data, cli["hierarchy"])

    del calls[:]
    perf = eca.main(cli["base"] + ["--hierarchy", cli["hier"], "--mistakes", "1", "5", "7", "--crm"], modes=cli["modes"])
    printed = capsys.readouterr().out
    assert calls == [("probs", "m1"), ("crm", 7, False), ("probs", "m2"), ("crm", 7, False), ("svm", "m3")]      # one extraction per model
    assert list(perf) == ["m1", "m1 [CRM]", "m2", "m2 [CRM]", "m3"]
    columns = eca.METRICS + ["Mistake Severity", "Hier. Dist@1", "Hier. Dist@5", "Hier. Dist@7"]
    assert printed == todays_table(perf, columns)
    for name, row in perf.items():
        model = name.split()[0]
        pred = (cli["svm_rank"] if model == "m3" else
                tc.lists(tc.risks(cli["outputs"][model], H), 7)[0] if name.endswith("[CRM]") else cli["rank"](cli["outputs"][model]))
        assert {k: row[k] for k in eca.METRICS} == dict(eca.evaluate(pred, data, cli["hierarchy"])), name
        assert {k: row[k] for k in columns[4:] if k in row} == tc.metrics(pred, y, H, [1, 5, 7]), name
        assert plain.get(name, row)["Accuracy"] == row["Accuracy"]
    # the CRM prediction minimises the expected height: its risk under the model's own probabilities is never above the arg-max's
    R = tc.risks(cli["outputs"]["m1"], H)
    n = np.arange(len(y))
    assert (R[n, tc.lists(R, 1)[0][:, 0]] <= R[n, cli["rank"](cli["outputs"]["m1"])[:, 0]]).all()

    del calls[:]
    perf = eca.main(cli["base"] + ["--hierarchy", cli["hier"], "--crm_logits"], modes=cli["modes"])
    capsys.readouterr()
    assert ("crm", 5, True) in calls and list(perf) == ["m1", "m1 [CRM]", "m2", "m2 [CRM]", "m3"]
    assert all(sorted(r) == sorted(eca.METRICS) for r in perf.values())                     # no --mistakes: no new column


def test_cli_refuses_what_it_cannot_compute(cli, capsys):
    import evaluate_classification_accuracy as eca
    import sehip
    for flags in (["--mistakes", "1"], ["--crm"], ["--crm_logits"]):
        with pytest.raises(SystemExit):
            eca.main(cli["base"] + flags, modes=cli["modes"])
        assert "--hierarchy" in capsys.readouterr().err
    for k in ("0", "33"):
        with pytest.raises(SystemExit):
            eca.main(cli["base"] + ["--hierarchy", cli["hier"], "--mistakes", "5", k], modes=cli["modes"])
    capsys.readouterr()
    assert sehip.KNN_TOP_MAX == 16
    with pytest.raises(SystemExit):
        eca.main(cli["base"] + ["--hierarchy", cli["hier"], "--mistakes", "1", "17", "--knn", "3"], modes=cli["modes"])
    assert "--knn" in capsys.readouterr().err


def test_cli_knn_vote_is_asked_for_the_longest_list(cli, capsys):
    import evaluate_classification_accuracy as eca
    data = cli["data"]
    rng = np.random.default_rng(9)
    seen = []

    def knn(data_, model, layer, normalize, ks, custom, batch_size, top=5):
        seen.append(top)
        return OrderedDict((k, np.stack([rng.permutation(10)[:top] for _ in range(data.num_test)])) for k in ks)

    modes = dict(cli["modes"], knn=knn)
    args = ["--dataset", cli["ds"], "--data_root", "-", "--model", "m3", "--layer", "-1", "--hierarchy", cli["hier"], "--knn", "3"]
    perf = eca.main(args + ["--mistakes", "1", "8"], modes=modes)
    assert seen == [8] and "Hier. Dist@8" in perf["m3 [k-NN, k=3]"]
    perf = eca.main(args + ["--mistakes", "2"], modes=modes)
    assert seen == [8, 5] and "Hier. Dist@2" in perf["m3 [k-NN, k=3]"]
    capsys.readouterr()


# ---- the C ABI without a GPU ----

def test_tree_risk_argument_validation_without_gpu():
    import sehip
    lib = sehip.lib()
    D = sehip._lib.DEFINES
    INVALID, UNSUPPORTED = D["SE_ERR_INVALID"], D["SE_ERR_UNSUPPORTED"]
    assert D["SE_TREE_RISK_TOP_MAX"] == 32 and 8142 <= D["SE_TREE_RISK_MAX_CLASSES"] <= 16384
    z, p = ctypes.c_void_p(0), ctypes.c_void_p(16)          # device pointers are not read before the launch

    def call(probs=p, ldp=100, pos=p, path_off=p, lo=p, hi=p, lh=p, nnz=300, own=z, N=4, C=100, top=5, cls=p, rt=p, risk=z, ldr=0):
        return lib.se_tree_risk_topk(probs, ldp, pos, path_off, lo, hi, lh, nnz, own, N, C, top, cls, rt, risk, ldr, z)

    for name in ("probs", "pos", "path_off", "lo", "hi", "lh", "cls", "rt"):
        assert call(**{name: z}) == INVALID, name
        assert b"se_tree_risk_topk" in lib.se_last_error()
    assert call(lo=z, hi=z, lh=z, nnz=0, N=0) == 0          # no level at all needs no level table
    for bad in (dict(top=0), dict(top=33, C=100), dict(top=6, C=5, ldp=5), dict(ldp=99), dict(risk=p, ldr=99), dict(C=0, ldp=0), dict(N=-1),
                dict(nnz=-1)):
        assert call(**bad) == INVALID, bad
    assert call(C=16385, ldp=16385) == UNSUPPORTED
    assert call(C=D["SE_TREE_RISK_MAX_CLASSES"] + 1, ldp=20000) == UNSUPPORTED
    assert b"SE_TREE_RISK_MAX_CLASSES" in lib.se_last_error()
    assert call(N=0) == 0                                   # an empty batch is OK, without a launch
