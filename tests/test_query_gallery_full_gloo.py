"""CPU, world_size = 2 over gloo: hierarchical_precision_device(..., gallery=..., rank_gallery=True) with the QUERIES sharded across
the ranks and the gallery replicated -- every rank ranks its own query rows against the whole gallery -- returns the rows of one
process: gathered per query, or only their sums reduced."""
import os
import pickle
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _evaluate(distributed, seen=None):
    import _qg_standins as qg
    g = qg.load_fixture()
    queries, labels, kw = qg.fixture_arguments(g)
    kernels = qg.cpu_kernels(True)
    if seen is not None:        # the query rows this process ranks, and against how many gallery items
        inner = kernels["rank_rows"]
        kernels["rank_rows"] = lambda pd: seen.append(tuple(pd.shape)) or inner(pd)
    res = {}
    for name, more in (("gathered", {}), ("sums", {"gather_per_query": False}), ("clipped", {"compute_ahp": 250})):
        args = dict(compute_ahp=True, compute_ap=True, normalize=True, kernels=kernels, tile_rows=7, distributed=distributed,
                    rank_gallery=True, **kw)
        args.update(more)
        means, per_query = qg.cifar_hierarchy().hierarchical_precision_device(queries.copy(), labels, g["ks"].tolist(), **args)
        res[name] = (means, {m: {int(i): v for i, v in rows.items()} for m, rows in per_query.items()})
    return res


def _worker(rank, world, port, out):
    for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from test_dp_gloo import _setup
    _setup(rank, world, port)
    seen = []
    res = _evaluate(True, seen)
    with open("%s.%d" % (out, rank), "wb") as f:
        pickle.dump((res, seen), f)
    dist.destroy_process_group()


def test_sharded_queries_return_the_rows_of_one_rank(tmp_path):
    from sharded_retrieval import shard_bounds
    out = str(tmp_path / "qgfull")
    mp.spawn(_worker, args=(2, 29641, out), nprocs=2, join=True)
    want = _evaluate(False)
    ids = list(want["gathered"][1]["AP"])
    assert len(ids) == 37
    for rank, (q0, q1) in enumerate(shard_bounds(37, 2)):
        with open("%s.%d" % (out, rank), "rb") as f:
            got, seen = pickle.load(f)
        # the gallery is replicated, the queries are not: this rank ranked q1 - q0 rows of 301 columns per evaluation
        assert all(s[1] == 301 for s in seen) and sum(s[0] for s in seen) == 3 * (q1 - q0), (rank, seen)
        for name in ("gathered", "clipped"):
            assert got[name][1] == want[name][1], (rank, name)                       # every query's row, bit for bit
            for m, v in want[name][0].items():
                assert got[name][0][m] == v, (rank, name, m)
        means, local = got["sums"]
        for m, rows in local.items():                                                # only this rank's rows, the means of all
            assert rows == {i: want["gathered"][1][m][i] for i in ids[q0:q1]}, (rank, m)
            assert abs(means[m] - want["gathered"][0][m]) <= 1e-13, (rank, m)
    assert np.isfinite(list(want["gathered"][0].values())).all()
