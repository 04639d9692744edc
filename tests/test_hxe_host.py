"""CPU: the host side of the hierarchy-aware classifier losses -- ClassHierarchy.hxe_encoding against explicit descendant sets,
ClassHierarchy.soft_label_table, the self-checks of the float64 canon (tests/_hxe_canon.py), the argument checks of the four new
entry points and the new flags of learn_classifier.py."""
import ctypes

import numpy as np
import pytest

import _hxe_canon as hc
from test_class_embedding_host import load_hierarchy


@pytest.fixture(scope="module", params=["cifar", "ilsvrc"])
def tree(request):
    h, classes = load_hierarchy(request.param)
    assert h.is_tree()
    return h, classes, h.hxe_encoding(classes, alpha=0.1), hc.Canon(h, classes)


def _levels(enc, i):
    a, b = int(enc["path_off"][i]), int(enc["path_off"][i + 1])
    return enc["lvl_lo"][a:b], enc["lvl_hi"][a:b], enc["lvl_w"][a:b]


def test_encoding_is_the_tree_by_ranges(tree):
    h, classes, enc, canon = tree
    C = len(classes)
    pos = enc["pos"]
    assert pos.dtype == np.int32 and sorted(pos.tolist()) == list(range(C))          # a permutation
    assert enc["path_off"].dtype == np.int32 and enc["path_off"][0] == 0 and enc["path_off"][-1] == len(enc["lvl_lo"])
    assert enc["lvl_lo"].dtype == enc["lvl_hi"].dtype == np.int32 and enc["lvl_w"].dtype == np.float32
    assert enc["max_levels"] == np.diff(enc["path_off"]).max() <= 32
    dropped_somewhere = False
    for i, c in enumerate(classes):
        lo, hi, w = _levels(enc, i)
        edges = canon.edges(c, alpha=0.1)
        kept = [e for e in edges if not e[3]]
        dropped_somewhere |= len(kept) < len(edges)
        assert len(lo) == len(kept)                                 # dropped: exactly the levels whose two leaf sets are equal
        size = 1
        for l, (lam, below, above, _) in enumerate(kept):
            assert 0 <= lo[l] <= pos[i] < hi[l] <= C and hi[l] - lo[l] > size        # nested, strictly growing
            size = hi[l] - lo[l]
            assert np.array_equal((pos >= lo[l]) & (pos < hi[l]), above)             # range membership == descendant set
            assert w[l] == np.float32(lam)
        assert (lo[-1], hi[-1]) == (0, C)
    if len(classes) == 100:
        assert dropped_somewhere                                    # the CIFAR tree has chains


def test_weights_follow_the_depth_rule_and_the_override(tree):
    h, classes, enc, canon = tree
    for i in (0, len(classes) // 2, len(classes) - 1):
        nodes, depth = canon.path(classes[i])
        kept = [l for l, e in enumerate(canon.edges(classes[i])) if not e[3]]
        _, _, w = _levels(enc, i)
        assert np.array_equal(w, np.asarray([np.exp(-0.1 * depth[l]) for l in kept], dtype=np.float32))
        assert depth[-1] == 0 and depth[-2] == 1 and w[-1] == np.float32(np.exp(-0.1))      # the edge below the top
    flat = h.hxe_encoding(classes, weights=lambda node: 0.25)
    assert np.array_equal(flat["lvl_w"], np.full(len(flat["lvl_w"]), 0.25, dtype=np.float32))
    assert np.array_equal(flat["lvl_lo"], enc["lvl_lo"]) and np.array_equal(flat["pos"], enc["pos"])
    by_node = h.hxe_encoding(classes, weights=lambda node: 2.0 if node == classes[3] else 1.0)
    _, _, w3 = _levels(by_node, 3)
    assert w3[0] == (2.0 if not canon.edges(classes[3])[0][3] else 1.0) and (w3[1:] == 1.0).all()
    again = h.hxe_encoding(list(classes), alpha=0.1)
    assert all(np.array_equal(again[k], enc[k]) for k in ("pos", "path_off", "lvl_lo", "lvl_hi", "lvl_w"))


def _hierarchy(edges):
    from class_hierarchy import ClassHierarchy
    parents, children = {}, {}
    for p, c in edges:
        parents.setdefault(c, []).append(p)
        children.setdefault(p, []).append(c)
    return ClassHierarchy(parents, children)


def test_forest_gets_a_virtual_top():
    h = _hierarchy([(10, 0), (10, 1), (11, 2), (11, 3), (12, 11)])
    enc = h.hxe_encoding([0, 1, 2, 3], alpha=0.5)
    assert enc["pos"].tolist() == [0, 1, 2, 3]
    lo, hi, w = _levels(enc, 0)                                     # 0 -> 10 -> virtual top
    assert list(zip(lo, hi)) == [(0, 2), (0, 4)]
    assert np.array_equal(w, np.asarray([np.exp(-1.0), np.exp(-0.5)], dtype=np.float32))     # d(0) = 2, d(10) = 1: the roots have d = 1
    lo, hi, w = _levels(enc, 2)                                     # 2 -> 11 -> 12 (dropped: the same classes) -> virtual top
    assert list(zip(lo, hi)) == [(2, 4), (0, 4)]
    assert np.array_equal(w, np.asarray([np.exp(-1.5), np.exp(-0.5)], dtype=np.float32))     # d(2) = 3, d(12) = 1; the edge 11 -> 12 is gone
    canon = hc.Canon(h, [0, 1, 2, 3])
    assert canon.forest and [e[3] for e in canon.edges(2, 0.5)] == [False, True, False]


def test_refusals_name_the_node():
    h, classes = load_hierarchy("wordnet_dag")
    assert not h.is_tree()
    with pytest.raises(ValueError, match="not a tree: node 'n"):
        h.hxe_encoding(classes)
    t = _hierarchy([(10, 0), (10, 1), (11, 10), (11, 2)])
    with pytest.raises(ValueError, match="class 10 is an ancestor"):
        t.hxe_encoding([0, 1, 10, 2])
    with pytest.raises(ValueError, match="class 10 is an ancestor"):
        t.hxe_encoding([10, 0, 2])
    with pytest.raises(ValueError, match="class 99 is unknown"):
        t.hxe_encoding([0, 1, 99])
    assert t.hxe_encoding([0, 1, 2])["max_levels"] == 2


def test_a_40_level_path_without_chains_is_refused_and_a_chain_is_not():
    comb = [(100 + i + 1, 100 + i) for i in range(40)] + [(100 + i + 1, i + 1) for i in range(40)] + [(100, 0), (100, 99)]
    h = _hierarchy(comb)                                            # class 0 sits 41 nodes below the top, a class joins at every node
    with pytest.raises(ValueError, match="class 0 has 41 levels"):
        h.hxe_encoding([0, 99] + list(range(1, 41)))
    chain = _hierarchy([(100 + i + 1, 100 + i) for i in range(40)] + [(100, 0), (140, 1)])
    enc = chain.hxe_encoding([0, 1])                                # 41 edges above class 0, 40 of them add no class
    assert enc["path_off"].tolist() == [0, 1, 2] and enc["lvl_w"][0] == np.float32(np.exp(-0.1))


def test_canon_self_checks(tree):
    h, classes, enc, canon = tree
    canon_self_checks(h, classes, canon)


@pytest.mark.parametrize("name", ["c1", "cat33", "cat33x1000", "rand20011"])
def test_canon_self_checks_on_the_trees_of_the_instantiation_matrix(name):
    """The one-class tree (no level), the caterpillar trees (every level count up to 32) and the long rows of
    tests/test_hxe_matrix_host.py."""
    import test_hxe_matrix_host as hm
    h, classes, canon, enc = hm.tree(name)
    canon_self_checks(h, classes, canon)


def canon_self_checks(h, classes, canon):
    C, B = len(classes), 6
    rng = np.random.default_rng(5)
    z = rng.standard_normal((B, C)) * 3.0
    y = rng.integers(0, C, size=B)
    flat = canon.hxe(z, y, alpha=0.0)
    assert np.abs(flat["loss"] + hc.log_softmax(z)[np.arange(B), y]).max() <= 1e-12        # alpha = 0: -log softmax
    onehot = np.eye(C)[y]
    assert np.abs(flat["dz"] - (np.exp(hc.log_softmax(z)) - onehot)).max() <= 1e-12
    got = canon.hxe(z, y, alpha=0.3)
    assert np.abs(got["dz"].sum(axis=1)).max() <= 1e-12                                     # every row's gradient sums to 0
    eps = 1e-5
    for i, c in [(0, int(y[0])), (1, (int(y[1]) + 1) % C), (2, int(np.argmax(z[2]))), (3, 0), (4, C - 1), (5, min(C - 1, 31))]:
        zp, zm = z.copy(), z.copy()
        zp[i, c] += eps
        zm[i, c] -= eps
        num = (canon.hxe(zp, y, alpha=0.3)["loss"][i] - canon.hxe(zm, y, alpha=0.3)["loss"][i]) / (2 * eps)
        assert abs(num - got["dz"][i, c]) <= 1e-8, (i, c, num, got["dz"][i, c])
    if C > 2000:
        return                                                      # (a [C, C] table of the long rows: not worth its memory here)
    table = h.soft_label_table(classes, 4.0).astype(np.float64)
    s = hc.soft(z, y, table)
    assert np.abs(s["dz"].sum(axis=1)).max() <= 1e-6                # rows of the float32 table sum to 1 up to its rounding
    zp, zm = z.copy(), z.copy()
    zp[0, 1 % C] += eps
    zm[0, 1 % C] -= eps
    assert abs((hc.soft(zp, y, table)["loss"][0] - hc.soft(zm, y, table)["loss"][0]) / (2 * eps) - s["dz"][0, 1 % C]) <= 1e-8
    assert np.abs(hc.soft(z, y, np.eye(C))["loss"] - flat["loss"]).max() <= 1e-12


def test_soft_label_table(tree):
    h, classes, enc, canon = tree
    C = len(classes)
    t = h.soft_label_table(classes, 10.0)
    assert t.dtype == np.float32 and t.shape == (C, C)
    assert np.abs(t.astype(np.float64).sum(axis=1) - 1.0).max() <= C * 2.0 ** -24
    assert np.array_equal(h.soft_label_table(classes, 0.0), np.full((C, C), np.float32(1.0 / C)))       # beta = 0: uniform
    rows = [0, C // 3, C - 1]
    d = np.asarray([[h.lcs_height(classes[i], c) for c in classes] for i in rows])                      # the definition, by lcs()
    logit = -10.0 * d
    e = np.exp(logit - logit.max(axis=1, keepdims=True))
    assert np.array_equal(t[rows], (e / e.sum(axis=1, keepdims=True)).astype(np.float32))
    assert (t.argmax(axis=1) == np.arange(C)).all()
    # d is symmetric; the table is where the normalisers agree (two classes of one height under one parent), up to the order of
    # the float64 row sums: one float32 ulp
    sib = [(i, j) for i in range(C) for j in range(i + 1, min(C, i + 40))
           if h.parents[classes[i]] == h.parents[classes[j]] and h.heights[classes[i]] == h.heights[classes[j]]]
    assert sib and all(abs(float(t[i, j]) - float(t[j, i])) <= 2.0 ** -23 * float(t[i, j]) for i, j in sib)


def test_soft_label_table_of_a_dag_goes_by_lcs():
    h, classes = load_hierarchy("wordnet_dag")
    sub = classes[:12]
    t = h.soft_label_table(sub, 3.0)
    d = np.asarray([[h.lcs_height(a, b) for b in sub] for a in sub])
    e = np.exp(-3.0 * d - (-3.0 * d).max(axis=1, keepdims=True))
    assert np.array_equal(t, (e / e.sum(axis=1, keepdims=True)).astype(np.float32))


def test_library_exports_the_hxe_symbols():
    import sehip
    lib = sehip.lib()
    for name in ("se_hxe_aux_floats", "se_hxe_fwd", "se_hxe_bwd", "se_soft_xent_fwd", "se_soft_xent_bwd"):
        assert name in sehip.EXPORTS and hasattr(lib, name), name
    assert sehip._lib.DEFINES["SE_HXE_MAX_LEVELS"] == 32
    assert lib.se_hxe_aux_floats(0) == 0 and lib.se_hxe_aux_floats(7) == 7 * 34


def test_entry_points_check_their_arguments_without_a_gpu():
    import sehip
    lib = sehip.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    good = (ctypes.c_int32 * 4)(0, 1, 3, 5)
    long_path = (ctypes.c_int32 * 4)(0, 1, 34, 35)
    shrinking = (ctypes.c_int32 * 4)(0, 2, 1, 3)
    late = (ctypes.c_int32 * 4)(1, 2, 3, 4)

    def hfwd(logits=one, dtype=0, ld=4, labels=one, pos=one, off=one, off_host=good, lo=one, B=2, C=3, loss_i=one, aux=one):
        return lib.se_hxe_fwd(logits, dtype, ld, labels, pos, off, off_host, lo, one, one, B, C, loss_i, aux, z, z, z, z)

    def hbwd(logits=one, dtype=0, ld=4, labels=one, pos=one, off=one, off_host=good, lo=one, B=2, C=3, aux=one, dz=one, ddtype=0, ldd=4):
        return lib.se_hxe_bwd(logits, dtype, ld, labels, pos, off, off_host, lo, one, one, aux, z, 1.0, B, C, dz, ddtype, ldd, z)

    def sfwd(logits=one, dtype=0, ld=4, labels=one, table=one, ldt=4, B=2, C=3, loss_i=one, aux=one):
        return lib.se_soft_xent_fwd(logits, dtype, ld, labels, table, ldt, B, C, loss_i, aux, z, z, z, z)

    def sbwd(logits=one, dtype=0, ld=4, labels=one, table=one, ldt=4, B=2, C=3, aux=one, dz=one, ddtype=0, ldd=4):
        return lib.se_soft_xent_bwd(logits, dtype, ld, labels, table, ldt, aux, z, 1.0, B, C, dz, ddtype, ldd, z)

    for f, who in ((hfwd, b"se_hxe_fwd"), (hbwd, b"se_hxe_bwd"), (sfwd, b"se_soft_xent_fwd"), (sbwd, b"se_soft_xent_bwd")):
        for C in (0, -1):
            assert f(C=C) == -1 and who + b": bad shape" in lib.se_last_error()
        assert f(B=-1) == -1 and who + b": bad shape" in lib.se_last_error()
        assert f(C=5, ld=4) == -1 and who + b": leading dimension" in lib.se_last_error()
        for name in ("logits", "labels", "aux"):
            assert f(**{name: z}) == -1 and who + b": null pointer" in lib.se_last_error(), name
        for dtype in (2, -1):
            assert f(dtype=dtype) == -1 and who + b": bad dtype" in lib.se_last_error()
    for f, who in ((hfwd, b"se_hxe_fwd"), (hbwd, b"se_hxe_bwd")):
        for name in ("pos", "off", "off_host", "lo"):
            assert f(**{name: z}) == -1 and who + b": null pointer" in lib.se_last_error(), name
        assert f(off_host=long_path) == -1 and who + b": class 1 has 33 levels, more than SE_HXE_MAX_LEVELS = 32" in lib.se_last_error()
        assert f(off_host=shrinking) == -1 and who + b": path_off decreases at class 1" in lib.se_last_error()
        assert f(off_host=late) == -1 and who + b": path_off[0] = 1" in lib.se_last_error()
        assert f(logits=z, labels=z, aux=z, pos=z, off=z, off_host=z, lo=z, B=0) == 0           # B = 0: nothing to do, every pointer NULL
    for f, who in ((sfwd, b"se_soft_xent_fwd"), (sbwd, b"se_soft_xent_bwd")):
        assert f(table=z) == -1 and who + b": null pointer" in lib.se_last_error()
        assert f(ldt=2) == -1 and who + b": table leading dimension" in lib.se_last_error()
        assert f(logits=z, labels=z, aux=z, table=z, B=0) == 0
    assert hfwd(loss_i=z) == -1 and sfwd(loss_i=z) == -1 and b"null pointer" in lib.se_last_error()
    for b in (hbwd, sbwd):
        assert b(dz=z) == -1 and b"null pointer" in lib.se_last_error()
        assert b(ddtype=3) == -1 and b"bad dtype" in lib.se_last_error()
        assert b(ldd=2) == -1 and b"leading dimension" in lib.se_last_error()


def test_ops_refuse_host_tensors_and_mismatched_encodings():
    import torch
    import sehip
    h, classes = load_hierarchy("cifar")
    enc = h.hxe_encoding(classes)
    zt, yt = torch.randn(4, 100, requires_grad=True), torch.zeros(4, dtype=torch.long)
    with pytest.raises(sehip.SehipError):
        sehip.hierarchical_cross_entropy(zt, yt, enc)
    with pytest.raises(sehip.SehipError):
        sehip.soft_label_cross_entropy(zt, yt, h.soft_label_table(classes, 1.0))
    with pytest.raises(sehip.SehipError, match="reduction"):
        sehip.hierarchical_cross_entropy(zt, yt, enc, reduction="max")
    assert sehip.HxeEncoding.of(enc) is sehip.HxeEncoding.of(enc) and sehip.HxeEncoding.of(enc).num_classes == 100
    bad = dict(enc, lvl_w=enc["lvl_w"][:-1])
    bad.pop("_sehip", None)
    with pytest.raises(sehip.SehipError, match="lvl_lo, lvl_hi and lvl_w"):
        sehip.HxeEncoding(bad)
    with pytest.raises(sehip.SehipError, match="square"):
        sehip.SoftLabelTable(np.zeros((3, 4), dtype=np.float32))


def test_parser_knows_the_new_losses(capsys):
    import learn_classifier as lc
    base = ["--dataset", "synthetic-cifar100", "--data_root", "-"]
    args = lc.parse_args(base)
    assert args.loss == "xent" and args.hierarchy is None and args.hxe_alpha == 0.1 and args.soft_beta == 10.0
    assert not args.is_a and not args.str_ids
    ok = lc.parse_args(base + ["--loss", "hxe", "--hierarchy", "h.txt", "--hxe_alpha", "0.3", "--is_a", "--str_ids"])
    assert ok.loss == "hxe" and ok.hxe_alpha == 0.3 and ok.is_a and ok.str_ids
    for loss in ("hxe", "soft_labels"):
        with pytest.raises(SystemExit):
            lc.parse_args(base + ["--loss", loss])
        assert "needs --hierarchy" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            lc.parse_args(base + ["--loss", loss, "--hierarchy", "h.txt", "--label_smoothing", "0.1"])
        assert "--label_smoothing" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        lc.parse_args(base + ["--loss", "focal"])
    assert lc.parse_args(base + ["--label_smoothing", "0.1"]).label_smoothing == 0.1             # xent keeps its smoothing
    help_text = " ".join(lc.build_parser(hierarchy_losses=True).format_help().split())
    assert "--hxe_alpha" in help_text and "--soft_beta" in help_text and help_text.count("has not measured") == 2
    assert "--loss" not in lc.build_parser().format_help()                                      # the reference's command line as it was
