"""GPU: the mistake metrics and CRM decoding end to end -- ClassHierarchy.height_table on the device, mistakes.crm_classification on
the real kernels (se_tree_risk_topk on the trees, se_pairwise_dist + se_topk_rows on a DAG) and the --crm / --mistakes command line,
against the explicit-set canon of tests/_tree_risk_canon.py.  Grid probabilities (integers / 1024) make every float32 and float64 sum
exact, so equality is demanded everywhere, ties included."""
import numpy as np
import pytest
import torch

import _tree_risk_canon as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["cifar", "cub"])
def test_height_table_on_the_device(name):
    h, classes = tc.tree(name)
    table = h.height_table(classes)
    assert table.is_cuda and table.dtype == torch.int32
    assert np.array_equal(table.cpu().numpy(), tc.height_table(h, classes))


@pytest.mark.parametrize("name,N,top", [("cifar", 33, 5), ("cub", 5, 20), ("ilsvrc", 5, 32)])
def test_crm_classification_on_the_tree_kernel(name, N, top):
    from mistakes import crm_classification
    h, classes = tc.tree(name)
    P = tc.grid_probs(N, len(classes), seed=N)
    want = tc.lists(tc.risks(P, tc.height_table(h, classes)), top)[0]
    assert np.array_equal(crm_classification(P, h, classes, top=top), want)
    assert np.array_equal(crm_classification(torch.from_numpy(P).cuda(), h, classes, top=top), want)


def test_crm_classification_on_a_dag_takes_the_dense_path():
    """The float32 chain errs by at most C * 2^-24 * H_max * sum p; with grid probabilities every partial sum is an integer below
    2^24 over 1024, so the chain is exact and the lists must equal the float64 canon's, ties included."""
    import mistakes
    h, classes = tc.tree("wordnet_dag")
    H = tc.height_table(h, classes)
    C = len(classes)
    assert C * 64 * H.max() < 2 ** 24
    with pytest.raises(ValueError):
        h.tree_risk_encoding(classes)
    P = tc.grid_probs(5, C, seed=3)
    assert np.array_equal(mistakes.crm_classification(P, h, classes, top=20), tc.lists(tc.risks(P, H), 20)[0])


def test_cli_crm_row_equals_the_canon(tmp_path, capsys):
    import evaluate_classification_accuracy as eca
    from class_hierarchy import ClassHierarchy
    from datasets import get_data_generator
    ds = "synthetic:10x8x40x30"
    data = get_data_generator(ds, "-")
    hier = tmp_path / "hierarchy.txt"
    hier.write_text("".join("%d %d\n" % (100 + c // 5, c) for c in range(10)) + "200 100\n200 101\n")
    hierarchy = ClassHierarchy.from_file(str(hier), id_type=int)
    H = tc.height_table(hierarchy, data.classes)
    y = np.asarray(data.labels_test)
    P = tc.grid_probs(data.num_test, 10, seed=4)
    perf = eca.main(["--dataset", ds, "--data_root", "-", "--hierarchy", str(hier), "--model", "m", "--layer", "-1", "--prob_features", "1",
                     "--mistakes", "1", "5", "--crm"], modes={"probs": lambda *a: P})
    assert "m [CRM]" in capsys.readouterr().out and list(perf) == ["m", "m [CRM]"]
    R = tc.risks(P, H)
    for name, pred in (("m [CRM]", tc.lists(R, 5)[0]), ("m", tc.lists(-P.astype(np.float64), 10)[0])):
        row = perf[name]
        assert {k: row[k] for k in row if k not in eca.METRICS} == tc.metrics(pred, y, H, [1, 5]), name
        assert {k: row[k] for k in eca.METRICS} == dict(eca.evaluate(pred, data, hierarchy)), name
