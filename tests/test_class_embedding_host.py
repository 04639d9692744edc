"""CPU: the host side of the class-embedding kernels -- the preference-rank encoding of se_class_pair_tables (checked through a
NumPy statement of the kernel's intersection rule against ClassHierarchy.lcs / wup_similarity for every pair), the drop-in
compute_class_embedding.py command line and pickle, and the argument checks of the two new entry points."""
import ctypes
import os
import pickle

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_hierarchy(name):
    """(ClassHierarchy, class list) of a hierarchy fixture: cifar / cub / ilsvrc (the WordNet min-tree) / wordnet_dag / inat2018."""
    from class_hierarchy import ClassHierarchy
    g = np.load(os.path.join(GOLDEN, "hierarchy_%s.npz" % name))
    emb = np.load(os.path.join(GOLDEN, "embeddings.npz"))
    if name == "cifar":
        id_type, classes = int, list(range(100))
    elif name == "cub":
        id_type, classes = int, emb["cub_balanced_unitsphere__ind2label"].tolist()
    elif name == "ilsvrc":
        id_type, classes = str, np.load(os.path.join(GOLDEN, "imagenet_mintree_unitsphere.npz"))["ind2label"].tolist()
    else:
        id_type, classes = str, g["classes"].tolist()
    parents, children = {}, {}
    for p, c in g["edges"].tolist():
        p, c = id_type(p), id_type(c)
        parents.setdefault(c, []).append(p)
        children.setdefault(p, []).append(c)
    return ClassHierarchy(parents, children), [id_type(c) for c in classes]


def tables_from_encoding(enc, rows=None, diag_one=False):
    """NumPy statement of pair_tables_kernel: lcs = the common ancestor of smallest preference rank."""
    off, rank, spl = enc["off"], enc["rank"], enc["spl"]
    C, R = len(off) - 1, len(enc["nodes"])
    member = np.zeros((C, R), dtype=bool)
    spl_d = np.full((C, R), -1, dtype=np.int64)
    for c in range(C):
        member[c, rank[off[c]:off[c + 1]]] = True
        spl_d[c, rank[off[c]:off[c + 1]]] = spl[off[c]:off[c + 1]]
    rows = range(C) if rows is None else rows
    wup, lcs = np.empty((len(rows), C)), np.empty((len(rows), C))
    H = float(enc["max_height"])
    for n, i in enumerate(rows):
        common = member[i][None, :] & member
        assert common.any(axis=1).all()
        r = common.argmax(axis=1)                      # first True: the smallest common rank
        ds = enc["depth"][r].astype(np.int64)
        wup[n] = (2.0 * ds) / ((ds + spl_d[i, r]) + (ds + spl_d[np.arange(C), r])).astype(np.float64)
        lcs[n] = 1.0 - enc["height"][r] / H
        if diag_one:
            lcs[n, i] = 1.0
    return wup, lcs


@pytest.mark.parametrize("name", ["cifar", "cub", "ilsvrc", "wordnet_dag"])
def test_encoding_reproduces_lcs_and_wup_for_every_pair(name):
    h, classes = load_hierarchy(name)
    enc = h.pair_table_encoding(classes)
    assert enc["max_anc"] <= 48                      # SE_CLASSEMB_MAX_ANC
    assert all((np.diff(enc["rank"][enc["off"][c]:enc["off"][c + 1]]) > 0).all() for c in range(len(classes)))
    wup, lcs = tables_from_encoding(enc)
    want_wup, want_lcs = h.similarity_tables(classes)
    assert np.array_equal(wup, want_wup)
    assert np.array_equal(lcs, want_lcs)
    if name == "cifar":
        g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
        assert np.array_equal(wup, g["wup"]) and np.array_equal(lcs, g["lcs"])


def test_wordnet_dag_fixture_needs_the_tie_break_and_the_dag_path_length():
    """The DAG fixture is what the encoding is for: classes with several hypernyms, pairs whose lcs is decided by the height /
    repr tie-break among equally deep common ancestors, and ancestors reached more briefly through a higher common ancestor
    than by walking up (spl != upward distance)."""
    h, classes = load_hierarchy("wordnet_dag")
    assert not h.is_tree() and len(h.nodes) == 1860 and len(classes) == 1000
    enc = h.pair_table_encoding(classes)
    off, rank, dep = enc["off"], enc["rank"], enc["depth"]
    member = np.zeros((len(classes), len(enc["nodes"])), dtype=bool)
    for c in range(len(classes)):
        member[c, rank[off[c]:off[c + 1]]] = True
    tied = []
    for i in range(len(classes)):
        common = member[i][None, :] & member
        first = common.argmax(axis=1)
        common[np.arange(len(classes)), first] = False
        second = common.argmax(axis=1)
        for j in np.flatnonzero(common.any(axis=1) & (dep[second] == dep[first])):
            tied.append((i, int(j), enc["nodes"][first[j]]))
    assert len(tied) >= 10                          # pairs with two equally deep common ancestors (24 ordered pairs)
    for i, j, want in tied:
        assert h.lcs(classes[i], classes[j]) == want
    upward = sum(1 for c, i in zip(classes, range(len(classes)))
                 for r, s in zip(enc["rank"][enc["off"][i]:enc["off"][i + 1]], enc["spl"][enc["off"][i]:enc["off"][i + 1]])
                 if h.all_hypernym_distances(c)[enc["nodes"][r]] != s)
    assert upward > 0


def test_inat_encoding_on_sampled_pairs():
    """8,142 iNat species: the encoding reproduces ClassHierarchy on 2,000 random pairs (the device test takes 100k)."""
    h, classes = load_hierarchy("inat2018")
    assert len(classes) == 8142 and h.is_tree()
    enc = h.pair_table_encoding(classes)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, len(classes), size=4).tolist()
    wup, lcs = tables_from_encoding(enc, rows=rows)
    cols = rng.integers(0, len(classes), size=500)
    for n, i in enumerate(rows):
        for j in cols:
            assert wup[n, j] == h.wup_similarity(classes[i], classes[j])
            assert lcs[n, j] == 1.0 - h.heights[h.lcs(classes[i], classes[j])] / h.max_height


def test_cli_parser_matches_the_reference_flags():
    import compute_class_embedding as cce
    p = cce.build_parser()
    acts = {a.dest: a for a in p._actions if a.dest != "help"}
    assert sorted(acts) == sorted(["hierarchy", "is_a", "str_ids", "class_list", "out", "method", "num_dim", "norm"])
    assert acts["hierarchy"].required and acts["out"].required
    assert acts["method"].default == "unitsphere" and acts["method"].choices == ["unitsphere", "approx_sim", "spheres", "mds"]
    assert acts["num_dim"].default is None and acts["num_dim"].type is int
    assert acts["class_list"].default is None
    for flag in ("is_a", "str_ids", "norm"):
        assert acts[flag].default is False and acts[flag].nargs == 0
    a = p.parse_args(["--hierarchy", "h.txt", "--out", "o.pickle"])
    assert (a.method, a.is_a, a.str_ids, a.norm, a.num_dim, a.class_list) == ("unitsphere", False, False, False, None, None)
    with pytest.raises(SystemExit):
        p.parse_args(["--hierarchy", "h.txt", "--out", "o", "--method", "glove"])


def test_class_order_rules(tmp_path):
    from class_hierarchy import ClassHierarchy
    import compute_class_embedding as cce
    h = ClassHierarchy({3: [0], 1: [0], 2: [1], 5: [1]}, {0: [3, 1], 1: [2, 5]})
    assert cce.class_order(h) == [2, 3, 5]
    cl = tmp_path / "classes.txt"
    cl.write_text("5 five\n\n2 two\n5 again\n3\n")
    assert cce.class_order(h, str(cl)) == [5, 2, 3]
    assert cce.class_order(h, str(cl), str_ids=True) == ["5", "2", "3"]


def test_host_eigen_methods_and_pickle_format(tmp_path):
    """sim_approx / mds stay host NumPy: their results reproduce their targets; the pickle holds the reference's three items."""
    import compute_class_embedding as cce
    h, classes = load_hierarchy("cifar")
    _, s = h.similarity_tables(classes)
    emb = cce.sim_approx(s)
    assert emb.shape == (100, 100) and np.abs(emb @ emb.T - s).max() < 1e-12
    assert cce.sim_approx(s, 10).shape == (100, 10)
    d = 1.0 - s
    np.fill_diagonal(d, 0.0)
    m = cce.mds(d, 20)
    assert m.shape[0] == 100 and m.shape[1] <= 20
    with pytest.raises(ValueError):
        cce.unitsphere_embedding(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        cce.euclidean_embedding(np.zeros((0, 0)))
    out = tmp_path / "e.pickle"
    with open(out, "wb") as f:
        pickle.dump({"ind2label": classes, "label2ind": {c: i for i, c in enumerate(classes)}, "embedding": emb}, f)
    with open(out, "rb") as f:
        dump = pickle.load(f)
    assert set(dump) == {"ind2label", "label2ind", "embedding"} and dump["embedding"].dtype == np.float64


def test_new_entry_points_check_their_arguments_without_a_gpu():
    import sehip
    lib = sehip.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)
    # se_class_pair_tables(off, rank, spl, nnz, c, max_anc, depth, height, n_ranks, H, flags, wup, ldw, lcs, ldl, missing, stream)
    assert lib.se_class_pair_tables(z, z, z, 4, 2, 4, z, z, 3, 2, 0, one, 2, one, 2, one, z) == -1
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_class_pair_tables(one, one, one, 4, 2, 4, one, one, 3, 2, 0, z, 2, z, 2, one, z) == -1      # no table asked for
    assert lib.se_class_pair_tables(one, one, one, 4, 2, 49, one, one, 3, 2, 0, one, 2, one, 2, one, z) == -1    # max_anc > 48
    assert b"max_anc" in lib.se_last_error()
    assert lib.se_class_pair_tables(one, one, one, 4, 2, 4, one, one, 3, 2, 8, one, 2, one, 2, one, z) == -1     # unknown flag
    assert lib.se_class_pair_tables(one, one, one, 4, 3, 4, one, one, 3, 2, 0, one, 2, None, 0, one, z) == -1   # ldw < c
    assert b"leading dimension" in lib.se_last_error()
    # se_cholesky_f64(a, lda, n, info, stream)
    assert lib.se_cholesky_f64(z, 4, 4, one, z) == -1
    assert b"null pointer" in lib.se_last_error()
    assert lib.se_cholesky_f64(one, 4, 4, z, z) == -1
    assert lib.se_cholesky_f64(one, 3, 4, one, z) == -1
    assert b"leading dimension" in lib.se_last_error()
    assert lib.se_cholesky_f64(one, 4, -1, one, z) == -1
    from sehip import _lib
    assert _lib.DEFINES["SE_CLASSEMB_MAX_ANC"] == 48
