"""CPU: host-side logic -- class hierarchy metrics vs values produced by the imported reference,
LR schedules, the Keras-style SGD update on the flat buffers, model factory."""
import os
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def hier():
    from class_hierarchy import ClassHierarchy
    g = np.load(os.path.join(GOLDEN, "hierarchy_cifar.npz"))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for p, c in g["edges"]:
            f.write("%d %d\n" % (p, c))
    h = ClassHierarchy.from_file(f.name, id_type=int)
    os.unlink(f.name)
    return h, g


def test_hierarchy_structure_matches_reference(hier):
    h, g = hier
    assert h.is_tree() and h.max_height == int(g["max_height"])
    assert [h.heights[n] for n in g["nodes"]] == g["heights"].tolist()
    wup = np.array([[h.wup_similarity(a, b) for b in range(100)] for a in range(100)])
    lcs = np.array([[1.0 - h.lcs_height(a, b) for b in range(100)] for a in range(100)])
    assert np.array_equal(wup, g["wup"])
    assert np.array_equal(lcs, g["lcs"])


def test_hierarchical_precision_matches_reference(hier):
    """Rankings come from the canonical oracle here (CPU); the metric values were produced by the
    reference's class_hierarchy + the reference's own rankings (equal up to tie order, which the
    metrics of same-class ties cannot see)."""
    from oracle import retrieval_oracle as ro
    h, g = hier
    labels = g["labels"].tolist()
    ks = g["ks"].tolist()
    want = dict(zip(g["metric_names"].tolist(), g["metric_values"].tolist()))
    for norm in (True, False):
        _, rk = ro.canon_retrieval(g["features"], norm)
        ret = {i: rk[i].tolist() for i in range(len(labels))}
        for ahp in (True, 50):
            avg, per_q = h.hierarchical_precision(ret, labels, ks, compute_ahp=ahp, compute_ap=True, all_ids=list(range(len(labels))))
            for m, v in avg.items():
                assert v == pytest.approx(want["%s|norm=%d|ahp=%s" % (m, norm, ahp)], rel=1e-12, abs=1e-12), (m, norm, ahp)
            assert len(per_q["AP"]) == len(labels)


# The rows of the CUB / ILSVRC fixtures contain exact float32 distance ties between images of DIFFERENT classes (3 adjacent pairs in the
# 520 x 520 Euclidean matrix of CUB; a few hundred among the 1400 x 1400 of ILSVRC): the reference's np.argsort (default kind, unstable)
# orders them arbitrarily, the canonical order by index -- its metric values therefore carry ~1e-9 of tie-order noise, which no
# deterministic implementation can reproduce.
TIE_NOISE = {True: 2e-8, False: 2e-8}


def _hierarchy_from_fixture(g, tmp_path):
    from class_hierarchy import ClassHierarchy
    path = str(tmp_path / "h.txt")
    with open(path, "w") as f:
        for p, c in g["edges"]:
            f.write("%s %s\n" % (p, c))
    id_type = int if str(g["id_type"]) == "int" else str
    labels = [id_type(l) for l in g["labels"].tolist()]
    return ClassHierarchy.from_file(path, id_type=id_type), labels


@pytest.mark.parametrize("name", ["cub", "ilsvrc"])
def test_hierarchical_precision_other_taxonomies_match_reference(name, tmp_path):
    """The host mirror on the two other taxonomies the reference ships (CUB balanced: 200 integer classes; ILSVRC WordNet
    min-tree: 1000 string ids, many classes with a single image -> AP of queries without any relevant item) against the values
    the imported reference produced (tests/golden/hierarchy_{cub,ilsvrc}.npz, oracle/make_golden.py:hierarchy_goldens_more)."""
    from oracle import retrieval_oracle as ro
    g = np.load(os.path.join(GOLDEN, "hierarchy_%s.npz" % name))
    h, labels = _hierarchy_from_fixture(g, tmp_path)
    ks = g["ks"].tolist()
    want = dict(zip(g["metric_names"].tolist(), g["metric_values"].tolist()))
    for norm in (True, False):
        _, rk = ro.canon_retrieval(g["features"], norm)
        ret = {i: rk[i].tolist() for i in range(len(labels))}
        for ahp in (True, 50):
            avg, _ = h.hierarchical_precision(ret, labels, ks, compute_ahp=ahp, compute_ap=True, all_ids=list(range(len(labels))))
            for m, v in avg.items():
                assert v == pytest.approx(want["%s|norm=%d|ahp=%s" % (m, norm, ahp)], rel=TIE_NOISE[norm], abs=TIE_NOISE[norm]), (m, norm, ahp)


def test_hierarchy_generator_input_and_save_roundtrip(hier, tmp_path):
    from class_hierarchy import ClassHierarchy
    h, g = hier
    h.save(str(tmp_path / "h.txt"))
    h2 = ClassHierarchy.from_file(str(tmp_path / "h.txt"), id_type=int)
    assert h2.heights == h.heights
    h.save(str(tmp_path / "isa.txt"), is_a_relations=True)
    h3 = ClassHierarchy.from_file(str(tmp_path / "isa.txt"), is_a_relations=True, id_type=int)
    assert h3.lcs(3, 7) == h.lcs(3, 7)
    labels = g["labels"].tolist()[:30]
    ret = ((i, list(range(30))) for i in range(30))
    avg, _ = h.hierarchical_precision(ret, labels, [1, 5], compute_ahp=False, compute_ap=False)
    assert set(avg) == {"P@1 (WUP)", "P@1 (LCS_HEIGHT)", "P@5 (WUP)", "P@5 (LCS_HEIGHT)"}


# ---------------------------------------------------------------- schedules

class FakeTrainer:
    lr = None
    is_main_process = True


def test_sgdr_schedule_values():
    import utils
    cbs, n = utils.get_lr_schedule("SGDR", 50000, 128, {})
    assert n == 372
    t = FakeTrainer()
    cbs[0].on_train_begin(t)
    assert t.lr == 0.1
    lrs = []
    for ep in range(14):
        lrs.append(t.lr)
        cbs[0].on_epoch_end(t, ep, {})
    # sgdr_callback.py:63-87: after the i-th epoch of a cycle the lr is f(i + 1), i.e. f(1) is skipped
    f = lambda i, T: 1e-6 + 0.5 * (0.1 - 1e-6) * (1 + np.cos(np.pi * i / T))
    want = [0.1] + [f(i, 12) for i in range(2, 13)] + [0.1]
    assert np.allclose(lrs[:13], want)
    assert lrs[13] == pytest.approx(f(2, 24))


def test_sgd_clr_and_resnet_schedules():
    import utils
    cbs, n = utils.get_lr_schedule("SGD", 1000, 10, {"sgd_schedule": "1:0.1,31:0.01,41:0.001,50"})
    assert n == 50
    t = FakeTrainer(); t.lr = 0.5
    got = []
    for ep in (0, 29, 30, 39, 40, 49):
        cbs[0].on_epoch_begin(t, ep); got.append(t.lr)
    assert got == [0.1, 0.1, 0.01, 0.01, 0.001, 0.001]
    cbs, n = utils.get_lr_schedule("CLR", 1000, 10, {})
    assert n == 240
    t = FakeTrainer(); cbs[0].on_train_begin(t)
    assert t.lr == 1e-5
    for b in range(1200):
        cbs[0].on_batch_end(t, b, {})
    assert t.lr == pytest.approx(0.1)
    cbs, n = utils.get_lr_schedule("ResNet-Schedule", 1000, 10, {})
    assert n == 164
    t = FakeTrainer(); t.lr = 1.0
    got = []
    for ep in (0, 1, 79, 80, 120):
        cbs[0].on_epoch_begin(t, ep); got.append(t.lr)
    assert got == [0.01, 0.1, 0.1, 0.01, 0.001]
    cbs, n = utils.get_lr_schedule("SGD", 1000, 10, {})
    assert n == 200 and isinstance(cbs[0], utils.ReduceLROnPlateau)
    with pytest.raises(ValueError):
        utils.get_lr_schedule("nope", 1, 1)


# ---------------------------------------------------------------- model factory + update rule

def test_build_network_contract():
    import utils
    m = utils.build_network(100, "resnet-110-fc", input_channels=3)
    assert sum(p.numel() for p in m.parameters()) == 1737860
    assert hasattr(m, "embedding") and m(torch.randn(2, 3, 32, 32)).shape == (2, 100)
    assert utils.build_network(100, "resnet-110").forward(torch.randn(2, 3, 32, 32)).shape == (2, 64)   # the 64-d trap
    c = utils.build_network(10, "resnet-32", classification=True)
    assert hasattr(c, "prob") and torch.allclose(c(torch.randn(2, 3, 32, 32)).sum(-1), torch.ones(2), atol=1e-5)
    w = utils.build_network(100, "resnet-110-wfc")
    assert w.num_features == 128
    r = utils.build_network(200, "resnet-50")
    assert r(torch.randn(1, 3, 64, 64)).shape == (1, 200) and hasattr(r, "embedding")
    with pytest.raises(NotImplementedError):
        utils.build_network(10, "wrn-28-10")
    with pytest.raises(ValueError):
        utils.build_network(10, "not-a-net")
    assert "ChannelPadding" in utils.get_custom_objects("resnet-110-fc")
    assert utils.ARCHITECTURES[0] == "simple" and utils.LR_SCHEDULES == ["SGD", "SGDR", "CLR", "ResNet-Schedule"]


def test_keras_sgd_update_on_flat_buffers():
    """v = m v - lr g ; w += v with the L2 term added before global-norm clipping."""
    import engine
    torch.manual_seed(0)
    lin = torch.nn.Linear(5, 3)
    w0, b0 = lin.weight.detach().clone(), lin.bias.detach().clone()
    loss_fn = lambda y, o: ((o - y) ** 2).sum(-1)
    tr = engine.Trainer(lin, {"out": (loss_fn, 1.0)}, {}, lr=0.1, momentum=0.9, clipnorm=0.5, l2_of={id(lin.weight): 0.01},
                        autocast_dtype=None)
    X, Y = torch.randn(4, 5), torch.randn(4, 3)
    ref = torch.nn.Linear(5, 3)
    ref.load_state_dict({"weight": w0, "bias": b0})
    vw, vb = torch.zeros_like(w0), torch.zeros_like(b0)
    for step in range(3):
        tr.train_step(X, Y, {})
        l = ((ref(X) - Y) ** 2).sum(-1).mean() + 0.01 * (ref.weight ** 2).sum()
        gw, gb = torch.autograd.grad(l, [ref.weight, ref.bias])
        norm = torch.sqrt((gw ** 2).sum() + (gb ** 2).sum())
        s = min(1.0, 0.5 / float(norm))
        vw = 0.9 * vw - 0.1 * gw * s
        vb = 0.9 * vb - 0.1 * gb * s
        with torch.no_grad():
            ref.weight += vw
            ref.bias += vb
        assert torch.allclose(lin.weight, ref.weight, atol=1e-6), step
        assert torch.allclose(lin.bias, ref.bias, atol=1e-6), step


def test_stolen_gradient_mode_equals_accumulating_mode_and_backbone_modes(monkeypatch):
    """engine.Trainer packs stolen gradients (p.grad = None + one cat) when every parameter is contiguous and no bucket hooks
    run, and accumulates into flat views otherwise; both give the same training trajectory."""
    import engine
    import utils
    assert engine.backbone_mode("resnet-110-fc") == (None, torch.contiguous_format)
    assert engine.backbone_mode("resnet-50") == (torch.bfloat16, torch.channels_last)
    monkeypatch.setenv("SE_TRAIN_DTYPE", "bf16"); monkeypatch.setenv("SE_TRAIN_LAYOUT", "nhwc")
    assert engine.backbone_mode("resnet-32") == (torch.bfloat16, torch.channels_last)
    monkeypatch.setenv("SE_TRAIN_LAYOUT", "sideways")
    with pytest.raises(ValueError):
        engine.backbone_mode("resnet-32")

    def make(fmt):
        torch.manual_seed(3)
        m = utils.build_network(10, "resnet-32", classification=True, no_softmax=True, input_channels=3)
        l2 = {id(p): m.regularizer for p in m.regularized_parameters()}
        return engine.Trainer(m, {"o": (lambda y, x: torch.nn.functional.cross_entropy(x, y, reduction="none"), 1.0)}, {}, lr=0.05,
                              momentum=0.9, clipnorm=5.0, l2_of=l2, autocast_dtype=None, memory_format=fmt)
    a, b = make(torch.contiguous_format), make(torch.contiguous_format)
    assert a.flat.all_contiguous and not make(torch.channels_last).flat.all_contiguous
    b.flat.all_contiguous = False            # same layout, accumulating mode
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        X, y = torch.randn(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)
        la, lb = float(a.train_step(X, y, {})), float(b.train_step(X, y, {}))
        assert abs(la - lb) < 1e-5
    assert not a._grads_bound and b._grads_bound
    pa = torch.cat([p.detach().reshape(-1) for p in a.model.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in b.model.parameters()])
    assert torch.allclose(pa, pb, rtol=1e-4, atol=1e-6)
    # switching a trainer back to accumulating mode re-binds p.grad to the flat buffer
    a.reducer.enabled = True
    a.reducer.finish = lambda: 1.0
    a._eager_core(X, y, {})
    assert a._grads_bound and all(p.grad.data_ptr() >= a.flat.flat_g.data_ptr() for p in a.flat.params)


def test_synthetic_generator_interface():
    from datasets import get_data_generator
    g = get_data_generator("synthetic:10x8x64x32", ".")
    assert (g.num_classes, g.num_train, g.num_test, g.num_channels) == (10, 64, 32, 3)
    seq = g.train_sequence(16, shuffle=False)
    assert len(seq) == 4
    X, y = seq[1]
    assert X.shape == (16, 3, 8, 8) and y.dtype == torch.int64 and len(g.labels_test) == 32
    X2, _ = seq[1]
    assert torch.equal(X, X2)                       # seeded per batch
    half = g.train_sequence(16, shuffle=False, rank=1, world_size=2)[1]
    assert half[0].shape[0] == 8 and torch.equal(half[1], y[1::2])
    with pytest.raises(NotImplementedError):
        get_data_generator("ilsvrc", ".")


def test_cli_parsers_accept_every_reference_flag():
    """Drop-in CLIs: the option sets of the reference's learn_image_embeddings.py:57-94 (+ utils.py:402-418) and
    evaluate_retrieval.py:157-174, listed here verbatim (the reference tree is not read at test time)."""
    import learn_image_embeddings as lie
    import evaluate_retrieval as er
    train_flags = ("--dataset --data_root --embedding --architecture --loss --cls_weight --cls_base --lr_schedule --clipgrad --max_decay "
                   "--nesterov --epochs --batch_size --val_batch_size --snapshot --snapshot_best --initial_epoch --finetune --finetune_init "
                   "--gpus --read_workers --queue_size --gpu_merge --model_dump --weight_dump --feature_dump --log_dir --no_progress --top_k_acc "
                   "--sgd_patience --sgd_lr --sgd_min_lr --sgd_schedule --sgdr_base_len --sgdr_mul --sgdr_max_lr --clr_step_len --clr_min_lr "
                   "--clr_max_lr").split()
    eval_flags = "--dataset --data_root --hierarchy --is_a --str_ids --classes_from --feat --label --norm --plot_max --prec_type --clip_ahp --csv".split()
    for parser, flags in ((lie.build_parser(), train_flags), (er.build_parser(), eval_flags)):
        have = {o for a in parser._actions for o in a.option_strings}
        assert not [f for f in flags if f not in have], [f for f in flags if f not in have]
    a = lie.build_parser().parse_args("--dataset CIFAR-100 --data_root /d --embedding e.pickle --architecture resnet-110-fc --loss inv_corr "
                                      "--lr_schedule SGDR --sgdr_max_lr 0.1 --max_decay 0 --epochs 372 --batch_size 100 --gpus 4 --read_workers 8 "
                                      "--queue_size 100 --gpu_merge --snapshot s.h5 --model_dump m.h5 --feature_dump f.pickle --top_k_acc 5".split())
    assert a.architecture == "resnet-110-fc" and a.sgdr_max_lr == 0.1 and a.gpus == 4 and a.top_k_acc == [5]       # the README's CIFAR-100 command line


def test_bench_traffic_record_matches_the_committed_pmc_profile():
    """bench.py's roofline.traffic comes from profiles/pmc_traffic.json (rocprofv3 PMC passes it cannot run itself): right shape only,
    FETCH_SIZE correction applied, and in the neighbourhood of the algorithmic bytes of the ranking kernel (one read + one write per element;
    the fabric-side counter also sees the row lines the L2 lost again before use, 1.19 x on the read side, and -- image path, round 5 -- the
    64-byte requests of the repair's key gathers: 27 GB against 20 GB, most of the excess served by the Infinity Cache)."""
    import bench
    tr = bench.pmc_traffic_gb("rank_rows", 50000, 50000, 100)
    assert tr is not None and os.path.exists(os.path.join(os.path.dirname(bench.__file__), tr["source"].split(" ")[0]))
    assert 0.95 < tr["bytes"] / 20e9 < 1.45 and abs(tr["read_GB"] + tr["write_GB"] - tr["bytes"] / 1e9) < 1e-6
    assert bench.pmc_traffic_gb("rank_rows", 1000, 50000, 100) is None and bench.pmc_traffic_gb("nope", 50000, 50000, 100) is None


def test_bench_gpus_flag_spawns_that_many_ranks():
    """`python bench.py --gpus 2` without a launcher re-launches itself as 2 ranks (torch.distributed.run, 127.0.0.1) and
    reports the size of the live process group; --dry keeps it on CPU/gloo with stand-in kernels."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["dry"] is True and rec["sharded_topk_matches_unsharded"] is True
    # the communicator's identity travels with the line: backend, world size, one (rank, device, pid) triple per rank, collected THROUGH it
    assert rec["rccl"]["backend"] == "gloo" and rec["rccl"]["world"] == 2 and sorted(r["rank"] for r in rec["rccl"]["ranks_seen"]) == [0, 1]
    assert rec["multi_gpu"]["n_gpus"] == 2


def test_bench_dry_run_with_8_ranks_completes_every_leg():
    """`bench.py --gpus 8 --dry --scaling strong --full` (gloo, 8 ranks on CPU): the launcher, the 8-way gallery shards + all-gather +
    merge of the `sharded_gallery` leg, the query-sharded ranking and the DP training step all complete and agree with one process."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry", "--scaling", "strong", "--full"], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["dry"] is True and rec["scaling"] == "strong"
    assert rec["sharded_gallery"] == {"parts": 8, "matches_unsharded": True}
    assert rec["retrieval"]["query_shards"] == 8 and rec["retrieval"]["rows_ranked"] == 64 * 8 and rec["retrieval"]["matches_unsharded"] is True
    assert rec["train"]["ranks"] == 8 and rec["train"]["replicas_identical"] is True and rec["train"]["loss_finite"] is True
    # the preflight ran first (communicator, 4-byte all-reduce, packed [2, 8, 251] all-gather, rank -> device map, gradient all-reduce
    # timings flat / bucketed) and its record travels with the line
    pre = rec["preflight"]
    assert pre["world"] == 8 and sorted(r["rank"] for r in pre["ranks"]) == list(range(8))
    assert all(set(v) >= {"flat_ms", "buckets_25MB_ms", "bytes"} for v in pre["grad_allreduce"].values())
    assert "[bench.py preflight] 8 ranks, backend gloo" in out.stderr


def test_bench_refuses_more_gpus_than_visible():
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 64:
        pytest.skip("unexpectedly many devices")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode != 0 and "visible" in (out.stderr + out.stdout)


def test_bench_plain_run_leaves_every_secondary_leg_to_full(monkeypatch, capsys):
    """A plain run prints the headline line and starts none of the checks or secondary legs; --full starts every one of them, for
    the retrieval and the training workload alike (the legs and the step are stand-ins here: this is the dispatch in main)."""
    import json
    import bench
    import train_bench
    calls = []

    def stand_in(name, ret):
        return lambda *a, **k: calls.append(name) or dict(ret)
    monkeypatch.setattr(bench, "init_dist", lambda args: (0, 1, 0))
    monkeypatch.setattr(bench, "comm_identity", lambda world, dry=False: {"backend": "none (single process)"})
    monkeypatch.setattr(bench, "bench_retrieval", lambda args, rank, world: (
        {"metric": "retrieval_Mpairs_per_sec", "value": 1.0, "roofline": {}, "config": {}, "kernels": {"rank_rows": {}}}, None, None))
    legs = ("bench_metrics", "bench_guaranteed_order", "cpu_baseline_retrieval", "bench_topk_all_pairs", "bench_rank_long_rows",
            "bench_eval_e2e", "bench_sharded_gallery")
    for name in legs:
        monkeypatch.setattr(bench, name, stand_in(name, {"ms_scaled_to_step": 1.0}))
    monkeypatch.setattr(train_bench, "bench_train", stand_in("bench_train", {"value": 1.0, "ms_per_step": 1.0}))
    monkeypatch.setattr(train_bench, "cpu_baseline_train", stand_in("cpu_baseline_train", {}))
    assert bench.parse([]).full is False and bench.parse(["--full"]).full is True
    bench.main(["--steps", "3"])
    assert calls == [] and json.loads(capsys.readouterr().out) == {"metric": "retrieval_Mpairs_per_sec", "value": 1.0, "roofline": {},
                                                                   "config": {}, "kernels": {"rank_rows": {}},
                                                                   "rccl": {"backend": "none (single process)"}}
    bench.main(["--steps", "3", "--full"])
    assert set(calls) == set(legs) | {"bench_train", "cpu_baseline_train"}
    assert {"hierarchical_precision", "guaranteed_order", "cpu_baseline", "retrieve_topk", "rank_long_rows", "eval_e2e", "sharded_gallery",
            "train", "train_r50"} <= set(json.loads(capsys.readouterr().out))
    del calls[:]
    bench.main(["--workload", "train"])
    assert calls == ["bench_train"] and "cpu_baseline" not in json.loads(capsys.readouterr().out)
    bench.main(["--workload", "train", "--full"])
    assert calls == ["bench_train"] * 2 + ["cpu_baseline_train"] and "cpu_baseline" in json.loads(capsys.readouterr().out)


def test_bench_cost_model_counts_executed_flops():
    import bench
    b, full, ex, floor = bench.pdist_cost_model(50000, 50000, 100, symmetric=True)
    assert b == 4.0 * 50000 * 50000 + 4.0 * 100000 * 100
    assert full == 5.0e11
    t = 391
    assert ex == (t * (t + 1) // 2) * 128 * 128 * 200.0 and 0.5 * full < ex < 0.51 * full
    assert abs(floor - max(ex / 157.3e12, b / 8e12) * 1e3) < 1e-12 and 1.5 < floor < 1.7
    _, _, ex_g, floor_g = bench.pdist_cost_model(50000, 50000, 100, symmetric=False)
    assert ex_g == full and 3.1 < floor_g < 3.3


def test_bench_dump_outputs_writes_a_seeded_row_sample_within_budget(tmp_path):
    """--dump-outputs: float32 / float64 .npy files, the same seeded rows on every call, no more bytes than the budget, and the
    written rows are the rows of the step's outputs; --steps sets the timed steps, so fewer than one is refused."""
    import bench
    q, n, d = 300, 500, 7
    rng = np.random.default_rng(3)
    feats = torch.from_numpy(rng.standard_normal((q, d)).astype(np.float32))
    pd = torch.from_numpy(rng.standard_normal((q, n)).astype(np.float32))
    rk = torch.from_numpy(np.argsort(pd.numpy(), axis=1, kind="stable").astype(np.int32))
    budget = 200000
    a = bench.dump_outputs(str(tmp_path / "a"), feats, pd, rk, budget=budget)
    b = bench.dump_outputs(str(tmp_path / "b"), feats, pd, rk, budget=budget)
    assert a["files"] == ["distances", "features", "ranking", "rows"] and 0 < a["bytes"] <= budget + 4 * 128
    assert a["rows"] == budget // (8 + 4 * d + 12 * n) < q
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in a["files"]}
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.array_equal(v, np.load(str(tmp_path / "b" / (k + ".npy")))), k
    rows = got["rows"].astype(np.int64)
    assert len(rows) == a["rows"] and np.all(np.diff(rows) > 0) and rows[-1] < q
    assert np.array_equal(got["features"], feats.numpy()[rows]) and np.array_equal(got["distances"], pd.numpy()[rows])
    assert np.array_equal(got["ranking"], rk.numpy()[rows].astype(np.float64))
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "c"), feats, pd, rk, budget=1000)
    assert bench.parse(["--steps", "7", "--dump-outputs", "x"]).steps == 7
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--workload", "train", "--dump-outputs", "x"], ["--dry", "--dump-outputs", "x"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def _write_cifar100(root, n_train=60, n_test=24, seed=0):
    import pickle
    rng = np.random.default_rng(seed)
    for name, n in (("train", n_train), ("test", n_test)):
        dump = {b"data": rng.integers(0, 256, size=(n, 3072), dtype=np.uint8), b"fine_labels": rng.integers(0, 100, size=n).tolist()}
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump(dump, f)


def test_cifar_reader_standardisation_matches_keras_featurewise(tmp_path):
    """the CIFAR python-pickle reader (datasets/cifar.py:9-84) + TinyDatasetGenerator's pre-processing
    (datasets/common.py:635-669,771-796): Keras ImageDataGenerator(featurewise_center, featurewise_std_normalization)
    statistics are PER CHANNEL over (samples, rows, columns); standardize is (x - mean) / (std + 1e-6)."""
    import pickle
    from datasets import get_data_generator
    root = str(tmp_path)
    _write_cifar100(root)
    gen = get_data_generator("cifar-100", root)
    assert gen.num_train == 60 and gen.num_test == 24 and gen.num_channels == 3 and gen.num_classes == max(gen.labels_train) + 1
    with open(os.path.join(root, "train"), "rb") as f:
        tr = pickle.load(f)
    with open(os.path.join(root, "test"), "rb") as f:
        te = pickle.load(f)
    X = tr[b"data"].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1).astype(np.float32)       # datasets/cifar.py: NHWC float images
    mean = X.mean(axis=(0, 1, 2))
    std = (X - mean).std(axis=(0, 1, 2))
    assert gen.mean.shape == (1, 1, 1, 3) and np.allclose(gen.mean.ravel(), mean, rtol=1e-6)
    assert np.allclose(gen.std.ravel(), std + 1e-6, rtol=1e-6)
    Xt = te[b"data"].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1).astype(np.float32)
    want = ((Xt - mean) / (std + 1e-6)).transpose(0, 3, 1, 2)
    got = gen.compose_batch(np.arange(24), train=False, augment=False).cpu().numpy()
    assert got.shape == (24, 3, 32, 32) and np.allclose(got, want, rtol=1e-5, atol=1e-5)
    assert gen.labels_test == list(te[b"fine_labels"])
    # sequences: labels travel with the rows, the short last batch survives data-parallel sharding without empty shards
    seq = gen.test_sequence(batch_size=10)
    assert len(seq) == 3
    Xb, yb = seq[2]
    assert Xb.shape[0] == 4 and yb.tolist() == gen.labels_test[20:24]
    shards = [gen.test_sequence(batch_size=10, rank=r, world_size=8)[2] for r in range(8)]
    assert all(s[0].shape[0] >= 1 for s in shards)


def test_cifar_reader_augmentation_is_flip_plus_bilinear_shift(tmp_path):
    from datasets.common import InMemoryDatasetGenerator
    h = w = 32
    rr, cc = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    ramp = np.stack([rr, cc, rr + 2 * cc], axis=-1)[None].repeat(40, axis=0)               # linear ramps: bilinear shifts are exact
    gen = InMemoryDatasetGenerator(ramp, ramp[:4], [0] * 40, [0] * 4, shift_range=0.15, horizontal_flip=False)
    gen.mean, gen.std = np.zeros((1, 1, 1, 3), np.float32), np.ones((1, 1, 1, 3), np.float32)
    torch.manual_seed(3)
    out = gen.compose_batch(np.arange(40), train=True, augment=True).cpu().numpy()
    ty = out[:, 0, 16, 16] - 16.0
    tx = out[:, 1, 16, 16] - 16.0
    assert np.abs(ty).max() <= 0.15 * h + 1e-4 and np.abs(tx).max() <= 0.15 * w + 1e-4
    assert ty.std() > 1.0 and tx.std() > 1.0 and np.abs(ty - np.round(ty)).max() > 0.05      # continuous, per-sample offsets
    inner = slice(6, 26)
    assert np.allclose(out[:, 0, inner, inner], rr[inner, inner][None] + ty[:, None, None], atol=1e-3)
    assert np.allclose(out[:, 2, inner, inner], (rr + 2 * cc)[inner, inner][None] + (ty + 2 * tx)[:, None, None], atol=1e-3)
    assert out.min() >= -1e-4 and out[:, 0].max() <= 31 + 1e-4                                # edges replicated, nothing extrapolated
    flip = InMemoryDatasetGenerator(ramp, ramp[:4], [0] * 40, [0] * 4, shift_range=0.0, horizontal_flip=True)
    flip.mean, flip.std = gen.mean, gen.std
    f = flip.compose_batch(np.arange(40), train=True, augment=True).cpu().numpy()
    mirrored = np.isclose(f[:, 1, 0, 0], 31.0)
    assert 5 < mirrored.sum() < 35
    assert np.allclose(f[mirrored][:, 1], cc[:, ::-1][None]) and np.allclose(f[~mirrored][:, 1], cc[None])


def test_cls_base_taps_named_or_indexed_layers():
    """--cls_base (reference: cls_model, learn_image_embeddings.py:16-45): the classifier head hangs off a named layer ('avg_pool':
    the pooled backbone features, 'embedding': the dense layer in front of l2norm) or a leaf-module index of the embedding model,
    while the first output stays the embedding; unknown names are rejected with the list of layers."""
    import torch
    import utils
    import learn_image_embeddings as lie
    torch.manual_seed(0)
    net = utils.build_network(10, 'resnet-110-fc', input_channels=3)         # CIFAR ResNet with the 'embedding' dense layer
    x = torch.randn(4, 3, 32, 32)
    net.eval()
    feats = net.features(x)
    emb = net(x)
    for base, want_in in (('avg_pool', feats), ('embedding', emb)):
        m = lie.ClsModel(net, 7, cls_base=base).eval()
        first, logits = m(x)
        assert torch.allclose(first, emb.float())
        assert logits.shape == (4, 7)
        assert torch.allclose(logits, m.prob(m.bn(torch.relu(want_in.float()))), atol=1e-6)
        assert m.bn.num_features == want_in.shape[1]
    leaves = [n for n, mod in net.named_modules() if n and not list(mod.children())]
    m = lie.ClsModel(net, 7, cls_base=str(leaves.index('avg_pool'))).eval()       # by index
    assert m.cls_base == 'avg_pool' and m(x)[1].shape == (4, 7)
    with pytest.raises(ValueError, match='no such layer'):
        lie.ClsModel(net, 7, cls_base='does_not_exist')
    with pytest.raises(ValueError, match='cannot tell the width'):            # a convolution's 4-d output cannot feed the dense classifier,
        lie.ClsModel(net, 7, cls_base='conv0', width=10)                     # whatever width the caller knows for the embedding OUTPUT
    with pytest.raises(ValueError, match='no such layer'):                    # an index past the last leaf: the same message, not IndexError
        lie.ClsModel(net, 7, cls_base=str(len(leaves) + 5))
    m = lie.ClsModel(net, 7, cls_base='l2norm', head='l2norm', width=10)      # the reference's last layer == the default base
    assert m.cls_base is None


def test_float64_features_are_not_cast_silently():
    """The reference computes in the caller's dtype (evaluate_retrieval.py:57-67); the drop-in ranks in float32 and says so."""
    import evaluate_retrieval as er
    x = np.random.default_rng(0).standard_normal((8, 4))
    with pytest.warns(RuntimeWarning, match='float64 features'):
        try:
            er.pairwise_retrieval(x, normalize=True)
        except Exception:       # no GPU here: the call fails loudly AFTER the warning (no CPU fallback)
            pass


# ---------------------------------------------------------------- in-memory data path pinned to the reference's own classes

def _cifar_fixture(tmp_path):
    """tests/golden/cifar_pipeline.npz (oracle/make_golden.py cifar_pipeline_goldens: outputs of the reference's unmodified
    datasets/cifar.py + datasets/common.py on a synthetic CIFAR-100 pickle pair) and the same pickles written to tmp_path."""
    import pickle
    g = np.load(os.path.join(ROOT, "tests", "golden", "cifar_pipeline.npz"))
    for name, raw, lab in (("train", g["raw_train"], g["y_train"]), ("test", g["raw_test"], g["y_test"])):
        with open(os.path.join(str(tmp_path), name), "wb") as f:
            pickle.dump({b"data": raw, b"fine_labels": lab.tolist()}, f)
    return g


def _nhwc(t):
    return t.permute(0, 2, 3, 1).cpu().numpy()


def test_cifar_pipeline_equals_the_reference_generator(tmp_path):
    """CifarGenerator / InMemoryDatasetGenerator / DeviceBatchSequence against what the reference's CifarGenerator /
    TinyDatasetGenerator / DataSequence produced (datasets/cifar.py:9-84, datasets/common.py:26-122,635-796): training-set
    statistics, every un-augmented batch and its labels, the batch_transform hook, class restriction with re-enumeration."""
    import torch
    from datasets.cifar import CifarGenerator
    g = _cifar_fixture(tmp_path)
    gen = CifarGenerator(str(tmp_path))
    gen.device = torch.device("cpu")
    assert (gen.num_classes, gen.num_train, gen.num_test) == (int(g["num_classes"]), int(g["num_train"]), int(g["num_test"]))
    assert np.allclose(gen.mean.reshape(-1), g["mean"].reshape(-1), rtol=1e-6)
    assert np.allclose(gen.std.reshape(-1), g["std"].reshape(-1) + 1e-6, rtol=1e-6)
    for split, seq, bs in (("test", gen.test_sequence(batch_size=24), 24), ("train", gen.train_sequence(batch_size=50, shuffle=False, augment=False), 50)):
        assert len(seq) == int(g[split + "_batches"])
        xs, ys = zip(*[seq[i] for i in range(len(seq))])
        X, y = _nhwc(torch.cat(xs)), torch.cat(ys).numpy()
        assert np.array_equal(y, g[split + "_y"])
        keep = len(g[split + "_X"])
        assert np.abs(X[:keep] - g[split + "_X"]).max() < 2e-6                      # (x - mean) / (std + 1e-6) in float32, like Keras
        assert np.allclose(X.astype(np.float64).sum(axis=(1, 2, 3)), g[split + "_image_sums"], atol=2e-3)
    seq = gen.test_sequence(batch_size=24, batch_transform=lambda X, y, scale: (X * scale, y + 1), batch_transform_kwargs={"scale": 2.0})
    X0, y0 = seq[0]
    assert np.abs(_nhwc(X0) - g["transformed_X0"]).max() < 4e-6 and np.array_equal(y0.numpy(), g["transformed_y0"])
    gen_r = CifarGenerator(str(tmp_path), classes=g["restricted_classes"].tolist(), reenumerate=True)
    gen_r.device = torch.device("cpu")
    assert gen_r.num_train == int(g["restricted_num_train"]) and np.allclose(gen_r.mean.reshape(-1), g["restricted_mean"].reshape(-1), rtol=1e-6)
    Xr, yr = gen_r.test_sequence(batch_size=1000)[0]
    assert np.array_equal(yr.numpy(), g["restricted_test_y"]) and np.abs(_nhwc(Xr) - g["restricted_test_X"]).max() < 2e-6


def test_device_augmentation_equals_keras_transform_on_the_same_parameters(tmp_path):
    """The (row shift, column shift, flip) the reference's generator drew, replayed through InMemoryDatasetGenerator.apply_transform:
    shift (bilinear, edges replicated) then flip, then -- commuting with it -- the standardisation."""
    import torch
    from datasets.cifar import CifarGenerator
    g = _cifar_fixture(tmp_path)
    gen = CifarGenerator(str(tmp_path))
    gen.device = torch.device("cpu")
    n = len(g["aug_X"])
    x = gen.compose_batch(np.arange(n), train=True, augment=False)
    p = g["aug_params"]
    got = gen.apply_transform(x.contiguous(), torch.from_numpy(p[:, 0]).float(), torch.from_numpy(p[:, 1]).float(), torch.from_numpy(p[:, 2] != 0))
    assert (p[:, 2] != 0).any() and (p[:, 2] == 0).any() and np.abs(p[:, :2]).max() <= 0.15 * 32 + 1e-9
    assert np.abs(_nhwc(got) - g["aug_X"]).max() < 2e-4
