"""CPU, world_size = 2 over gloo: query-vs-gallery evaluation with the gallery sharded across the ranks -- every rank counts over
its shard, one integer all-reduce adds the counts -- equals the single-process result exactly (integer adds commute, and nothing
behind them is reduced across ranks in floating point)."""
import os
import pickle
import sys
import warnings

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _evaluate(distributed):
    import _qg_standins as qg
    from recall_precision import recall_precision_device
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    res = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for bins in (None, 10):
            res["recprec_%s" % bins] = recall_precision_device(queries.copy(), labels, normalize=True, bins=bins, kernels=qg.cpu_kernels(True),
                                                               tile_rows=16, tile_cols=64, distributed=distributed, **kw)
    means, per_query = qg.cifar_hierarchy().hierarchical_precision_device(
        queries.copy(), labels, g["ks"].tolist(), compute_ahp=int(g["ahp_clip"]), compute_ap=True, normalize=True,
        kernels=qg.cpu_kernels(True), tile_rows=16, tile_cols=64, distributed=distributed, **kw)
    res["hprec_per_query"] = {m: [per_query[m][i] for i in g["query_ids"].tolist()] for m in per_query}
    return res


def _worker(rank, world, port, out):
    for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from test_dp_gloo import _setup
    _setup(rank, world, port)
    res = _evaluate(True)
    with open("%s.%d" % (out, rank), "wb") as f:
        pickle.dump(res, f)
    dist.destroy_process_group()


def test_sharded_counting_equals_the_single_process_result(tmp_path):
    out = str(tmp_path / "qg")
    mp.spawn(_worker, args=(2, 29631, out), nprocs=2, join=True)
    want = _evaluate(False)
    for rank in range(2):
        with open("%s.%d" % (out, rank), "rb") as f:
            got = pickle.load(f)
        for bins in (None, 10):
            for a, b in zip(got["recprec_%s" % bins], want["recprec_%s" % bins]):
                assert np.array_equal(a, b), (rank, bins)
        assert got["hprec_per_query"] == want["hprec_per_query"], rank
