#!/usr/bin/env python
"""bench.py -- headline benchmark of the cosine-embedding training + retrieval hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload retrieval|train] [--dump-outputs DIR] [--full]

One JSON line on stdout (rank 0).  See DESIGN.md section 6 for what a "step" is:

* retrieval (default; BASELINE.json configs[2], "CIFAR-100 50k-query x 50k-gallery retrieval"):
  one step = the whole ``pairwise_retrieval`` device path on synthetic float32 features already
  resident in HBM -- row normalisation, all-pairs cosine distance matrix, full canonical ranking.
  value = query x gallery pairs ranked per second (Mpairs/s), summed over ranks.  With N > 1 every
  rank evaluates its own 50k x 50k feature set (weak scaling, no data-path collective: retrieval jobs
  and the rows of a ranking are independent -- SURVEY.md section 8e row 2).
* a plain run does only what the headline needs: set-up, warm-up, the timed steps, ``--dump-outputs`` and the line, whose
  ``roofline`` / ``kernels`` objects come from the HIP events of the timed steps themselves (no runs of their own).
* ``--full`` adds everything else, none of it part of ``value``: AFTER the timed region the last step's results are checked
  against the oracle at full size (``"verified"``, oracle/verify.py), and the line carries, as objects next to the headline
  (all timed the same way): ``train`` (BASELINE.json configs[1]: ResNet-110-fc step, images/s), ``train_r50`` (configs[3]:
  ResNet-50 224x224, 200 classes, per-GPU batch 64), ``sharded_gallery`` (configs[4], the north_star retrieval split: 50,000
  queries x N x 160,146 gallery rows x D = 1000, per-shard fused distance + top-251 -> RCCL all-gather -> k-way merge, with the
  three phases timed separately), the CPU baselines, hierarchical precision, the guaranteed-order ranking, fused top-k,
  long-row ranking and end-to-end evaluation legs, and at N > 1 the preflight's gradient all-reduce timings.
* ``--workload train`` makes the training step the primary metric (``--full``: with its loss-head kernel times, standalone
  gradient all-reduce and CPU baseline).
* ``--dump-outputs DIR`` (retrieval): after the timed steps, rank 0 writes what the last timed step computed -- a fixed, seeded
  sample of the rows of its distance matrix and ranking, and those rows of the features they were computed from -- as float32 /
  float64 ``DIR/<name>.npy``, under 64 MB in all (``dump_outputs``).  The inputs are seeded, so two builds run with the same
  arguments can be compared output for output.

``--gpus N`` with N > 1 and no torch.distributed environment makes this process re-launch itself as N ranks
(``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...``); under an existing launcher the
world size comes from the environment and must equal ``--gpus``.  ``n_gpus`` in the line is the size of the live process group.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32 matrix peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 peak
# LDS floor of the 3-pass register-resident ranking: LDS wave-instructions per key x measured cycles per
# wave-instruction of each kind (tools/probes/lds_throughput.hip, profiles/r01_i_lds_throughput_probe.txt) at 2.4 GHz, 256 CUs
RANK_LDS_FLOOR_CYCLES_PER_KEY = 73000.0 / 50000.0
# the two-pass path (rows whose keys lie within 2^24 codes of their maximum: the synthetic Euclidean rows do): 7 random + 3 linear
# LDS operations per key instead of 12 + 5
RANK_LDS_FLOOR_CYCLES_PER_KEY_TWO_PASS = 43300.0 / 50000.0
# the image path (round 5; cosine rows: two passes on a 24-bit image of the key + tag scan + repair): the 7 random + 3 linear
# operations of the two passes, one linear tag write and one random tag read per key (784 wave-instructions each per 50,000-column
# row at 6.4 / 3.5 / 5.9 cycles), the scan's linear index read (0.25 per key)
RANK_LDS_FLOOR_CYCLES_PER_KEY_IMAGE = (43300.0 + 784 * 3.5 + 784 * 5.9 + 196 * 3.5) / 50000.0
MFMA_F16_PEAK_TFLOPS = 2500.0   # dense fp16 = bf16 peak (MI355X_MICROARCH.md)
SHADER_CLOCK_GHZ = 2.4
# what the chip SUSTAINS under the retrieval kernels (GRBM_GUI_ACTIVE / duration, profiles/r05_pmc_rank_pdist.txt: 1.9 - 2.13 GHz): the LDS
# floor of the ranking kernel is reported at both clocks -- at 2.4 GHz it is a floor the chip cannot reach
SUSTAINED_CLOCK_GHZ = 2.1
N_CUS = 256


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="retrieval", choices=["retrieval", "train"])
    ap.add_argument("--n", type=int, default=50000, help="gallery rows (retrieval)")
    ap.add_argument("--q", type=int, default=None, help="query rows per rank (retrieval; default = n)")
    ap.add_argument("--d", type=int, default=100, help="feature dimension (retrieval)")
    ap.add_argument("--metric", default="cosine", choices=["cosine", "euclid"])
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every check and secondary measurement: post-run oracle check, CPU baselines, "
                         "the other retrieval and training legs, per-leg rooflines (default off: the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--cpu-sample-queries", type=int, default=16384, help="query rows of the timed CPU sample (~13 s of host work, ~10 GB of host memory)")
    ap.add_argument("--with-train", dest="with_train", action="store_true", default=True,
                    help="--full: also time the ResNet-110-fc and ResNet-50 training steps (adds 'train' / 'train_r50' objects; default on)")
    ap.add_argument("--no-train", dest="with_train", action="store_false")
    ap.add_argument("--no-sharded", dest="with_sharded", action="store_false", default=True,
                    help="--full: skip the sharded-gallery top-k leg (configs[4])")
    ap.add_argument("--no-verify", dest="verify", action="store_false", default=True, help="--full: skip the post-run oracle check")
    ap.add_argument("--batch", type=int, default=128, help="per-GPU batch (train)")
    ap.add_argument("--arch", default="resnet-110-fc")
    ap.add_argument("--shard-rows", type=int, default=160146, help="gallery rows per rank of the sharded-gallery leg (1,281,167 / 8)")
    ap.add_argument("--shard-queries", type=int, default=50000)
    ap.add_argument("--shard-dim", type=int, default=1000)
    ap.add_argument("--shard-k", type=int, default=251)
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: fixed work per GPU (50k queries / 128 images per rank); strong: ONE problem split over the ranks -- the "
                         "reference's multi_gpu_model semantics for training (global batch 128), query rows sharded for retrieval")
    ap.add_argument("--dry", action="store_true",
                    help="CPU plumbing test: gloo process group, tiny shapes, CPU stand-ins for the kernels (no measurement)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="retrieval: write a seeded row sample of the last timed step's outputs to DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs is not None and (args.dry or args.workload != "retrieval"):
        ap.error("--dump-outputs applies to the retrieval workload only")
    return args


# ---------------------------------------------------------------------------------------------
# process group
# ---------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def maybe_spawn(args, argv):
    """``--gpus N`` without a launcher: re-exec as N ranks.  Returns the exit code of the launcher, or None to continue."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return None
    if not args.dry:
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit("bench.py --gpus %d: only %d ROCm device(s) visible" % (args.gpus, have))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # dmabuf IPC only on this host driver (RCCL / tensor sharing)
    return subprocess.call(cmd, env=env)


def init_dist(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(args.gpus, 1):
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s)" % (args.gpus, world))
    if not args.dry:
        if torch.cuda.device_count() <= local:
            raise SystemExit("bench.py: rank %d has no device %d (%d visible)" % (rank, local, torch.cuda.device_count()))
        torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if args.dry else "nccl", rank=rank, world_size=world)   # "nccl" == RCCL on ROCm
        world = dist.get_world_size()        # n_gpus = the live process group
    return rank, world, local


def preflight(args, rank, world, local):
    """Before any large allocation: prove that the communicator this run depends on exists and moves data in the shapes the legs use,
    and say which rank drives which device.  N > 1 only (the first 8-GPU run of this repository is also its first RCCL run with more
    than one rank): a 4-byte all-reduce, ONE all_gather_into_tensor of the packed [2, 8, 251] top-k layout of the sharded-gallery leg,
    the rank -> device -> PCI bus id map gathered through the communicator, and with --full the standalone all-reduce time of the two
    gradient buffers the training legs exchange (ResNet-110-fc: 7 MB, ResNet-50: 96 MB) as one flat call and as 25 MB buckets.  Any
    inconsistency ends the run with ONE line naming it.  --dry runs the same sequence on gloo / CPU tensors."""
    info = {"world": world}
    if world <= 1:
        return info
    dev = "cpu" if args.dry else "cuda"
    t0 = time.perf_counter()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if not args.dry:
        vis = torch.cuda.device_count()
        if vis < local_world:
            raise SystemExit("bench.py preflight: LOCAL_WORLD_SIZE=%d but only %d ROCm device(s) visible to rank %d (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES?)"
                             % (local_world, vis, rank))
        if local >= vis:
            raise SystemExit("bench.py preflight: rank %d has LOCAL_RANK=%d but sees %d device(s)" % (rank, local, vis))
    one = torch.ones(1, dtype=torch.float32, device=dev)
    dist.all_reduce(one)
    if int(one.item()) != world:
        raise SystemExit("bench.py preflight: 4-byte all-reduce over %d ranks returned %s" % (world, one.item()))
    packed = torch.full((2, 8, 251), rank, dtype=torch.int32, device=dev)            # the sharded-gallery leg's send block, 8 queries
    got = torch.empty((world, 2, 8, 251), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(got.view(-1), packed.view(-1))
    if not bool((got[:, 0, 0, 0].cpu() == torch.arange(world, dtype=torch.int32)).all()):
        raise SystemExit("bench.py preflight: all_gather_into_tensor of the packed [2, 8, 251] layout returned the blocks out of rank order")
    # rank -> device -> PCI bus id, through the communicator
    bus = -1
    name = "cpu"
    if not args.dry:
        p = torch.cuda.get_device_properties(local)
        name = p.name
        bus = (int(getattr(p, "pci_domain_id", 0)) << 16) | (int(getattr(p, "pci_bus_id", -1)) << 8) | int(getattr(p, "pci_device_id", 0))
    me = torch.tensor([rank, local, bus, os.getpid()], dtype=torch.int64, device=dev)
    seen = torch.empty((world, 4), dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(seen.view(-1), me)
    rows = seen.cpu().tolist()
    info["ranks"] = [{"rank": int(r), "local_device": int(d), "pci": ("%04x:%02x:%02x" % (b >> 16, (b >> 8) & 255, b & 255)) if b >= 0 else None, "pid": int(pid)}
                     for r, d, b, pid in rows]
    info["device_name"] = name
    if not args.dry and all(b >= 0 for _, _, b, _ in rows) and len({(b) for _, _, b, _ in rows}) != world:
        raise SystemExit("bench.py preflight: %d ranks share %d distinct PCI devices -- two ranks drive one GPU (LOCAL_RANK / visible-device mismatch)"
                         % (world, len({(b) for _, _, b, _ in rows})))
    # --full: standalone gradient all-reduce of the two training buffers: one flat call vs 25 MB buckets (what engine.BucketedAllReduce
    # issues)
    sizes = {"resnet110_fc_7MB": 6986752, "resnet50_96MB": 95777792} if not args.dry else {"tiny_64KB": 65536}
    ar = {}
    for key, nbytes in sizes.items() if args.full else ():
        buf = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
        bucket = 25 * (1 << 20) // 4
        res = {}
        for mode in ("flat", "buckets_25MB"):
            ts = []
            for it in range(4):
                barrier_sync(world, dry=args.dry)
                t1 = time.perf_counter()
                if mode == "flat":
                    dist.all_reduce(buf)
                else:
                    works = [dist.all_reduce(buf[o:o + bucket], async_op=True) for o in range(0, buf.numel(), bucket)]
                    for w in works:
                        w.wait()
                barrier_sync(world, dry=args.dry)
                if it:
                    ts.append(time.perf_counter() - t1)
            ms = max_over_ranks(float(np.median(ts)), world, dev) * 1e3
            res[mode + "_ms"] = ms
            res[mode + "_busbw_GBps"] = 2.0 * (world - 1) / world * nbytes / 1e6 / ms
        ar[key] = dict(res, bytes=nbytes)
        del buf
    if args.full:
        info["grad_allreduce"] = ar
    info["seconds"] = time.perf_counter() - t0
    if rank == 0:
        print("[bench.py preflight] %d ranks, backend %s: %s" % (world, dist.get_backend(), json.dumps(info)), file=sys.stderr, flush=True)
    return info


def barrier_sync(world, dry=False):
    if world > 1:
        dist.barrier()
    if not dry:
        torch.cuda.synchronize()


def max_over_ranks(value, world, device):
    if world == 1:
        return value
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def comm_identity(world, dry=False):
    """What the live communicator is, for the driver to confirm that N ranks really met over RCCL: backend name, library version as
    torch reports it (torch.cuda.nccl.version() is RCCL's on ROCm), world size of the process group, and the (rank, device, PCI bus id)
    triples collected THROUGH the communicator (an all-gather on the device for "nccl")."""
    info = {"backend": None, "version": None, "world": world, "ranks_seen": []}
    if world == 1:
        info["backend"] = "none (single process)"
        if not dry:
            p = torch.cuda.get_device_properties(torch.cuda.current_device())
            info["ranks_seen"] = [{"rank": 0, "device": torch.cuda.current_device(), "name": p.name}]
        return info
    info["backend"] = dist.get_backend()
    if info["backend"] == "nccl":
        try:
            info["version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception as e:      # noqa: BLE001
            info["version"] = "unknown (%s)" % type(e).__name__
        info["library"] = "RCCL (torch's 'nccl' backend on ROCm)"
        info["hip"] = torch.version.hip
    dev = "cpu" if dry else "cuda"
    me = torch.tensor([dist.get_rank(), -1 if dry else torch.cuda.current_device(), os.getpid()], dtype=torch.int64, device=dev)
    seen = torch.empty((world, 3), dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(seen.view(-1), me)
    info["ranks_seen"] = [{"rank": int(r), "device": int(d), "pid": int(p)} for r, d, p in seen.cpu().tolist()]
    info["distinct_devices"] = len({(int(d)) for _, d, _ in seen.cpu().tolist()})
    return info


def multi_gpu_summary(out, world):
    """At N > 1: the phases that actually cross xGMI, promoted next to the headline so that a SCALE run explains itself (the weak
    headline is N independent retrieval jobs with no collective and says nothing about the fabric)."""
    if world <= 1:
        return None
    summ = {"n_gpus": world, "headline_has_collective": False}
    sg = out.get("sharded_gallery")
    if isinstance(sg, dict) and "ms" in sg:
        summ["sharded_gallery"] = {"all_gather_ms": sg["ms"]["all_gather"], "local_topk_ms": sg["ms"]["local_topk"], "merge_ms": sg["ms"]["merge"],
                                   "all_gather_bytes_per_rank": sg.get("all_gather_bytes_per_rank"),
                                   "all_gather_GBps_per_rank": sg.get("all_gather_GBps_per_rank"),
                                   "exchange_frac_of_step": sg["ms"]["all_gather"] / sg["ms"]["total"], "collectives_per_step": 1}
    for leg in ("train", "train_bf16", "train_r50", "train_r50_b128", "train_r50_ilsvrc"):
        t = out.get(leg)
        if isinstance(t, dict) and t.get("grad_allreduce_ms") is not None:
            ar, step = t["grad_allreduce_ms"], t["ms_per_step"]
            summ[leg] = {"images_per_sec": t["value"], "ms_per_step": step, "grad_allreduce_ms": ar, "grad_bytes": t.get("grad_bytes"),
                         "allreduce_busbw_GBps": 2.0 * (world - 1) / world * t.get("grad_bytes", 0) / 1e6 / ar if ar else None,
                         # exposed exchange time = step time - the same step's time with the collective hidden perfectly (unknown here);
                         # the bound reported is the standalone all-reduce as a fraction of the step: overlap can only make it smaller
                         "allreduce_frac_of_step_upper_bound": ar / step}
    return summ


class KernelTimer:
    """HIP-event timing of individual launches on the stream they are enqueued on (torch's current
    stream, which is the stream handed to the C ABI)."""

    def __init__(self):
        self.records = {}

    def time(self, name, fn):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.records.setdefault(name, []).append((a, b))
        return out

    def avg_ms(self):
        torch.cuda.synchronize()
        return {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in self.records.items()}


# ---------------------------------------------------------------------------------------------
# retrieval workload
# ---------------------------------------------------------------------------------------------

def pdist_cost_model(q, n, d, symmetric, tile=128):
    """Algorithmic bytes, executed flops and the binding floor of one se_pairwise_dist launch.  In symmetric
    mode only the upper-triangle tiles are computed (each is stored twice), so the matrix pipe executes about half of 2 q n d."""
    bytes_ = 4.0 * q * n + 4.0 * (q + n) * d
    full = 2.0 * q * n * d
    if symmetric:
        t = (n + tile - 1) // tile
        executed = (t * (t + 1) // 2) * (tile * tile) * 2.0 * d
    else:
        executed = full
    floor_ms = max(executed / (MFMA_F32_PEAK_TFLOPS * 1e12), bytes_ / (HBM_PEAK_GBS * 1e9)) * 1e3
    return bytes_, full, executed, floor_ms


def bench_retrieval(args, rank, world):
    import sehip
    n, d = args.n, args.d
    q = args.q or n
    metric = sehip.METRIC_COSINE if args.metric == "cosine" else sehip.METRIC_EUCLID
    # SURVEY.md 8d synthetic features.  Weak scaling: every rank evaluates its OWN feature file of the same shape
    # (rank r: seed r), i.e. N independent `evaluate_retrieval` jobs -- identical work per rank, no data-path collective.
    strong = args.scaling == "strong" and world > 1
    rng = np.random.default_rng(0 if strong else rank)
    feats_h = rng.standard_normal((n, d)).astype(np.float32)
    gallery0 = torch.from_numpy(feats_h).cuda()
    qrows = None
    if strong:
        # ONE feature set: rank r ranks its shard of the query rows against the whole (replicated) gallery -- SURVEY.md 8e row 2
        from sharded_retrieval import shard_bounds
        qrows = shard_bounds(n, world)[rank]
        q = qrows[1] - qrows[0]
        queries0 = gallery0[qrows[0]:qrows[1]].clone()
    elif q == n:
        queries0 = None        # all-pairs within the feature set (the reference's only mode): symmetric kernel
    else:
        qrng = np.random.default_rng(100 + rank)
        queries0 = torch.from_numpy(qrng.standard_normal((q, d)).astype(np.float32)).cuda()

    pd = torch.empty((q, n), dtype=torch.float32, device="cuda")
    rk = torch.empty((q, n), dtype=torch.int32, device="cuda")
    timer = None
    last = {}

    def step():
        g = gallery0.clone()
        qs = g if queries0 is None else queries0.clone()
        t = timer.time if timer is not None else (lambda name, fn: fn())
        if metric == sehip.METRIC_COSINE:
            t("normalize_rows", lambda: sehip.normalize_rows_(g))
            if qs is not g:
                sehip.normalize_rows_(qs)
            t("pairwise_dist", lambda: sehip.pairwise_dist(qs, g, metric=metric, out=pd))
        else:
            sq = t("row_sqnorm", lambda: sehip.row_sqnorm(g))
            sqq = sq if qs is g else sehip.row_sqnorm(qs)
            t("pairwise_dist", lambda: sehip.pairwise_dist(qs, g, metric=metric, sqa=sqq, sqb=sq, out=pd))
        t("rank_rows", lambda: sehip.rank_rows(pd, out=rk))
        last["g"], last["q"] = g, (None if qs is g else qs)

    for _ in range(args.warmup):
        step()
    timer = KernelTimer()
    barrier_sync(world)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier_sync(world)
    elapsed = max_over_ranks(time.perf_counter() - t0, world, "cuda")
    kms = timer.avg_ms()
    dumped = None
    if args.dump_outputs is not None and rank == 0:
        dumped = dump_outputs(args.dump_outputs, last["g"] if last["q"] is None else last["q"], pd, rk)

    pairs_per_step = float(n) * n if strong else float(q) * n * world
    value = pairs_per_step * args.steps / elapsed / 1e6
    # algorithmic bytes / flops per launch
    pd_bytes, pd_full, pd_exec, pd_floor = pdist_cost_model(q, n, d, symmetric=queries0 is None)
    rk_bytes = 4.0 * q * n + 4.0 * q * n
    # what the ranking kernel's detector selects for these rows (tests/test_gpu_retrieval.py::test_rank_rows_detector_picks_the_variant...)
    two_pass = metric == sehip.METRIC_EUCLID and 32768 <= n <= 53248
    image = metric == sehip.METRIC_COSINE and 32768 <= n <= 50176
    rk_floor_cpk = RANK_LDS_FLOOR_CYCLES_PER_KEY_TWO_PASS if two_pass else (RANK_LDS_FLOOR_CYCLES_PER_KEY_IMAGE if image else RANK_LDS_FLOOR_CYCLES_PER_KEY)
    rk_lds_floor_ms = rk_floor_cpk * q * n / (N_CUS * SHADER_CLOCK_GHZ * 1e9) * 1e3
    pms, rms = kms["pairwise_dist"], kms["rank_rows"]
    kernels = {
        "pairwise_dist": {"ms": pms, "algorithmic_GB": pd_bytes / 1e9, "GBps": pd_bytes / 1e6 / pms, "frac_hbm": pd_bytes / 1e6 / pms / HBM_PEAK_GBS,
                          "mode": "symmetric (upper-triangle tiles, mirrored stores)" if queries0 is None else "general",
                          "flops_full_matrix": pd_full, "flops_executed": pd_exec,
                          "TFLOPs_executed": pd_exec / 1e9 / pms, "frac_mfma_f32": pd_exec / 1e9 / pms / MFMA_F32_PEAK_TFLOPS,
                          "floor_ms": pd_floor, "floor": "max(executed flops / 157.3 TFLOP/s, algorithmic bytes / 8 TB/s)",
                          "frac_of_floor": pd_floor / pms},
        "rank_rows": {"ms": rms, "algorithmic_GB": rk_bytes / 1e9, "GBps": rk_bytes / 1e6 / rms, "frac_hbm": rk_bytes / 1e6 / rms / HBM_PEAK_GBS,
                      "lds_floor_ms": rk_lds_floor_ms, "frac_of_lds_floor": rk_lds_floor_ms / rms,
                      "lds_floor_ms_sustained_clock": rk_lds_floor_ms * SHADER_CLOCK_GHZ / SUSTAINED_CLOCK_GHZ,
                      "frac_of_lds_floor_sustained_clock": rk_lds_floor_ms * SHADER_CLOCK_GHZ / SUSTAINED_CLOCK_GHZ / rms,
                      "sustained_clock_GHz": SUSTAINED_CLOCK_GHZ,
                      "variant": "two lossless passes (window)" if two_pass else ("image path: two passes on a 24-bit image + tag scan + repair" if image else "three passes"),
                      "lds_floor": ("2-pass LSD radix on 24 significant key bits, 10" if two_pass else
                                    ("2-pass LSD radix on a 24-bit image + tag write / read + scan, 12.25" if image else "3-pass LSD radix, 17.25")) +
                                   " LDS wave-instructions per 64 keys at their measured throughput (DESIGN.md 5.2), 256 CUs x 2.4 GHz"},
    }
    dominant = max(("pairwise_dist", "rank_rows"), key=lambda k: kms[k])
    tr = pmc_traffic_gb(dominant, q, n, d)
    # `frac` is always the HBM fraction (algorithmic bytes / time / 8 TB/s).  The ranking kernel moves 1.03x its algorithmic bytes
    # (PMC) and still sits far below the HBM roofline: what binds it is the LDS pipe, reported as such.
    roofline = {"kernel": dominant, "bound": "lds" if dominant == "rank_rows" else "hbm", "achieved": kernels[dominant]["GBps"],
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": kernels[dominant]["frac_hbm"],
                "traffic": None if tr is None else tr["bytes"],          # HBM bytes per launch (PMC), vs algorithmic_GB below
                "algorithmic_bytes": kernels[dominant]["algorithmic_GB"] * 1e9, "traffic_detail": tr}
    if dominant == "rank_rows":
        roofline["lds_floor_ms"] = rk_lds_floor_ms
        roofline["frac_of_lds_floor"] = rk_lds_floor_ms / rms
        roofline["frac_of_lds_floor_sustained_clock"] = rk_lds_floor_ms * SHADER_CLOCK_GHZ / SUSTAINED_CLOCK_GHZ / rms
    else:
        roofline["floor_ms"] = pd_floor
        roofline["frac_of_floor"] = pd_floor / pms
    out = {
        "metric": "retrieval_Mpairs_per_sec", "value": value, "unit": "Mpairs/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "CIFAR-100-sized retrieval: %d queries/GPU x %d gallery, D=%d, %s, "
                               "normalise + all-pairs distance + full canonical ranking" % (q, n, d, args.metric),
                   "queries_per_gpu": q, "gallery": n, "dim": d,
                   "parallelism": ("query rows of ONE feature set sharded %d ways, gallery replicated (no collective)" % world) if strong
                                  else "%d independent feature sets, one per GPU (no collective)" % world},
        "roofline": roofline, "kernels": kernels,
    }
    if dumped is not None:
        out["dump_outputs"] = dumped
    if args.full and args.verify:
        out.update(verify_last_step(last, pd, rk, metric, world))
        # scalars the driver's parsed subset keeps (it drops nested objects below `roofline` / `config`)
        out["roofline"]["verified"] = out["verified"]
        out["config"]["verified"] = out["verified"]
    return out, feats_h, rk


DUMP_BUDGET_BYTES = 60 * 10 ** 6      # --dump-outputs: below 64 MB in all, with room for the .npy headers


def dump_outputs(out_dir, feats, pd, rk, budget=DUMP_BUDGET_BYTES, seed=0):
    """--dump-outputs: what the last timed step returned to its caller, as .npy files in float32 / float64.  The [q, n] outputs
    are too large to write whole (2 x 10 GB at 50k x 50k), so the same seeded sample of their rows is written on every run with
    the same shapes -- as many rows as fit in `budget` bytes:
        rows.npy       [r]     float64  the sampled query rows, ascending
        features.npy   [r, d]  float32  those rows of the features the distances were computed from (normalised in place for cosine)
        distances.npy  [r, n]  float32  those rows of the pairwise_dist output
        ranking.npy    [r, n]  float64  those rows of the rank_rows output (gallery indices, exact in float64)"""
    q, n = pd.shape
    d = feats.shape[1]
    r = min(q, budget // (8 + 4 * d + 4 * n + 8 * n))
    if r < 1:
        raise ValueError("--dump-outputs: one row of a %d-column output does not fit in %d bytes" % (n, budget))
    rows = np.sort(np.random.default_rng(seed).choice(q, size=r, replace=False))
    idx = torch.from_numpy(rows).to(pd.device)
    arrays = {"rows": rows.astype(np.float64),
              "features": feats.index_select(0, idx).cpu().numpy().astype(np.float32),
              "distances": pd.index_select(0, idx).cpu().numpy().astype(np.float32),
              "ranking": rk.index_select(0, idx).cpu().numpy().astype(np.float64)}
    os.makedirs(out_dir, exist_ok=True)
    nbytes = 0
    for name, a in arrays.items():
        path = os.path.join(out_dir, name + ".npy")
        np.save(path, a)
        nbytes += os.path.getsize(path)
    return {"dir": os.path.abspath(out_dir), "rows": int(r), "files": sorted(arrays), "bytes": nbytes}


def bench_metrics(args, rk, reps=3):
    """SURVEY.md 8(f) row 1, the consumer of the step's rankings: hierarchical precision (P@k for k = 1..250, whole-list AHP, AP) of
    every query of the last step from its ranking, on a synthetic 100-class hierarchy (random symmetric similarity tables, random
    labels; the best-possible curves built the way ClassHierarchy.hierarchical_precision_device builds them).  Reported beside the
    step, not part of `value`."""
    import sehip
    q, n = rk.shape
    C = 100
    rng = np.random.default_rng(1)
    cls_h = rng.integers(0, C, size=n).astype(np.int32)
    tab = rng.random((C, C)); tab = (tab + tab.T) / 2; np.fill_diagonal(tab, 1.0)
    counts = np.bincount(cls_h, minlength=C)
    best = np.stack([np.cumsum(np.repeat(tab[c][np.argsort(-tab[c], kind="stable")], counts[np.argsort(-tab[c], kind="stable")])) for c in range(C)])
    cls = torch.from_numpy(cls_h).cuda()
    tab_d, best_d = torch.from_numpy(tab).cuda(), torch.from_numpy(best).cuda()
    qcls = cls[:q].contiguous() if q <= n else cls[torch.arange(q, device="cuda") % n].contiguous()
    qidx = torch.arange(q, dtype=torch.int32, device="cuda")
    ks = torch.arange(1, 251, dtype=torch.int32, device="cuda")
    curves = sehip.hprec_reciprocal_curves(best_d, best_d)

    def run():
        return sehip.hierarchical_precision(rk, cls, qcls, qidx, tab_d, tab_d, best_d, best_d, ks, ahp_len=0, want_ap=True, curves=curves)
    res = run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ms = float(np.median(ts))
    return {"ms": ms, "queries": int(q), "ranks_per_query": int(n), "Mranks_per_sec": q * n / ms / 1e3, "rank_GBps": 4.0 * q * n / ms / 1e6,
            "metrics": "P@1..250 (WUP, LCS), whole-list AHP (WUP, LCS), AP; 100 classes", "finite": bool(torch.isfinite(res).all().item())}


def bench_guaranteed_order(args, q=8192, reps=3):
    """The headline's stable order rests on a probed hardware property (gfx950's LDS serves same-address returning adds in lane
    order: include/sehip.h, se_rank_rows_init).  This leg times the ranking WITHOUT it -- a child process with SE_RANK_SAFE=1, the
    ballot kernels every device can run -- on q cosine rows of the benchmark's shape, once, outside the timed region, and scales the
    time to the step's row count."""
    import subprocess
    code = (
        "import sys, json, numpy as np, torch\n"
        "sys.path[:0] = %r\n"
        "import sehip\n"
        "n, d, q, reps = %d, %d, %d, %d\n"
        "x = torch.from_numpy(np.random.default_rng(0).standard_normal((n, d)).astype(np.float32)).cuda()\n"
        "sehip.normalize_rows_(x)\n"
        "pd = sehip.pairwise_dist(x[:q], x, metric=sehip.METRIC_COSINE)\n"
        "rk = torch.empty((q, n), dtype=torch.int32, device='cuda')\n"
        "sehip.rank_rows(pd, out=rk); torch.cuda.synchronize()\n"
        "ts = []\n"
        "for _ in range(reps):\n"
        "    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)\n"
        "    a.record(); sehip.rank_rows(pd, out=rk); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))\n"
        "print(json.dumps({'ms': float(np.median(ts)), 'violations': int(sehip.rank_rows_check(pd, rk))}))\n"
    ) % ([os.path.join(ROOT, "semantic-embeddings_amd"), ROOT], args.n, args.d, min(q, args.q or args.n), reps)
    env = dict(os.environ, SE_RANK_SAFE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600)
    got = json.loads(res.stdout.strip().splitlines()[-1])
    rows = min(q, args.q or args.n)
    return {"rows_timed": rows, "ms_rows_timed": got["ms"], "order_guard_violations": got["violations"],
            "ms_scaled_to_step": got["ms"] * (args.q or args.n) / rows,
            "what": "se_rank_rows with SE_RANK_SAFE=1 (guaranteed-order ballot kernels, no reliance on the LDS lane order), child process"}


def bench_eval_e2e(args, reps=2):
    """What evaluate_retrieval.py's main() does per --feat file, end to end in wall time: features on the host -> device, distances,
    full ranking, hierarchical precision (P@1..250, whole-list AHP, AP) of every query on the CIFAR-100 hierarchy of the golden
    fixtures -> the averages back on the host.  Both branches of the CLI (--norm yes / the Euclidean default).  The reference's own
    stages for the same input on the survey host: BASELINE.md section 2 (distance + ranking 166.5 s, metrics ~0.6 h)."""
    from class_hierarchy import ClassHierarchy
    import tempfile
    g = np.load(os.path.join(ROOT, "tests", "golden", "hierarchy_cifar.npz"))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for p_, c_ in g["edges"]:
            f.write("%d %d\n" % (p_, c_))
    h = ClassHierarchy.from_file(f.name, id_type=int)
    os.unlink(f.name)
    rng = np.random.default_rng(0)
    classes = sorted(set(g["labels"].tolist()))
    n, d = args.n, args.d
    labels = [classes[i] for i in rng.integers(0, len(classes), size=n)]
    centers = rng.standard_normal((max(classes) + 1, d)).astype(np.float32)
    feats = (centers[labels] + 0.8 * rng.standard_normal((n, d))).astype(np.float32)
    ks = list(range(1, 251))
    out = {"items": n, "dim": d, "metrics": "P@1..250 (WUP, LCS_HEIGHT), whole-list AHP, AP; CIFAR-100 hierarchy",
           "reference_host_stages": "BASELINE.md section 2: distance + ranking 166.5 s, hierarchical_precision ~0.6 h (8 vCPU survey host)"}
    for name, norm in (("cosine", True), ("euclid", False)):
        h.hierarchical_precision_device(feats[:4096].copy(), labels[:4096], ks, compute_ahp=True, compute_ap=True, normalize=norm, per_query=False)
        ts = []
        for _ in range(reps + 1):        # the first full-size call allocates the whole-matrix tile cache (reported separately)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            avg, _ = h.hierarchical_precision_device(feats.copy(), labels, ks, compute_ahp=True, compute_ap=True, normalize=norm, per_query=False)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name] = {"first_call_s": ts[0], "wall_s": float(np.median(ts[1:])), "AHP_WUP": float(avg["AHP (WUP)"]), "AP": float(avg["AP"])}
    import evaluate_retrieval
    evaluate_retrieval.release_tile_cache()
    return out


def bench_rank_long_rows(args, reps=3, q=8192, n=100000):
    """Full ranking of rows above the 53,248-column limit of the register-resident kernel (SURVEY.md 8a row 10 has no size limit:
    evaluate_retrieval.py:67): q queries against an n-row gallery, real cosine distances.  Two sorted runs per row + merge
    (DESIGN.md 5.2); reported as time per key beside the headline kernel's."""
    import sehip
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((n, args.d)).astype(np.float32)).cuda()
    sehip.normalize_rows_(x)
    pd = sehip.pairwise_dist(x[:q], x, metric=sehip.METRIC_COSINE)
    rk = torch.empty((q, n), dtype=torch.int32, device="cuda")
    sehip.rank_rows(pd, out=rk)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); sehip.rank_rows(pd, out=rk); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ms = float(np.median(ts))
    bad = sehip.rank_rows_check(pd, rk)
    return {"ms": ms, "queries": q, "gallery": n, "ps_per_key": ms * 1e9 / (q * n), "algorithmic_GBps": 8.0 * q * n / ms / 1e6,
            "order_guard_violations": int(bad)}


def bench_topk_all_pairs(args, feats_h, reps=3, k=251):
    """The fused distance + top-k on the headline problem (se_retrieve_topk, all-pairs: every item query and gallery item): what
    `evaluate_retrieval.py --clip_ahp K --skip_ap` runs instead of distance matrix + full ranking.  No [Q, N] matrix exists:
    algorithmic bytes = 4 (Q + N) D + 8 Q k.  Checked against the head of this step's full ranking by the GPU tests
    (tests/test_gpu_topk.py); here only timed."""
    import sehip
    x = torch.from_numpy(feats_h).cuda()
    if args.metric == "cosine":
        sehip.normalize_rows_(x)
        metric, sq = sehip.METRIC_COSINE, None
    else:
        metric, sq = sehip.METRIC_EUCLID, sehip.row_sqnorm(x)
    run = lambda: sehip.retrieve_topk(x, x, k, metric=metric, sqq=sq, sqg=sq)   # noqa: E731
    d, i = run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ms = float(np.median(ts))
    n, dd = feats_h.shape
    self_first = bool((i[:, 0] == torch.arange(n, device="cuda", dtype=torch.int32)).all().item()) if args.metric == "cosine" else None
    out = {"ms": ms, "k": k, "Mpairs_per_sec": float(n) * n / ms / 1e3, "algorithmic_GB": (8.0 * n * dd + 8.0 * n * k) / 1e9,
           "vs_distance_plus_ranking": "replaces pairwise_dist + rank_rows of the step above when only the first k ranks are consumed",
           "every_query_finds_itself_first": self_first}
    out.update(topk_phase_rooflines(run, n, n, dd, k, shared_image=True))
    return out


def topk_phase_rooflines(run, q, n, d, k, shared_image):
    """One more call of a fused distance + top-k leg with the library's phase events on (se_phase_timing: HIP events on the launch
    stream behind every phase of se_retrieve_topk) -> a roofline object per dominant phase, from what the phase EXECUTES:
      filter      fp16 matrix-core pass over the scaled half-precision images: 2 q n kp flop (kp = d padded to a multiple of 128) / time
                  against the dense fp16 peak;
      refinement  the exact fp32 chains of the survivors: every recomputed entry gathers one gallery row (4 d bytes) / time against HBM
                  peak (the counter is the library's own: entries recomputed, summed over the queries);
    and the bytes the whole call moves against SURVEY.md 8d's algorithmic 4 (q + n) d + 8 q k."""
    import sehip
    try:
        sehip.phase_timing(True)
        run()
        phases, cnt = sehip.phase_timing_read()
    finally:
        sehip.phase_timing(False)
    kp = (d + 127) // 128 * 128
    S = 4096 if n >= 65536 else 2048                                   # sampled gallery rows of the threshold pass (topk.hip: fused_plan_compute)
    filt_ms, ref_ms = phases.get("filter"), phases.get("refine")
    res = {"phase_ms": phases}
    if filt_ms:
        fl = 2.0 * q * n * kp
        res["roofline_filter"] = {"kernel": "pf_big_kernel" if kp >= 256 else "pf_tile_kernel", "bound": "mfma", "achieved": fl / 1e9 / filt_ms,
                                  "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": fl / 1e9 / filt_ms / MFMA_F16_PEAK_TFLOPS, "dtype": "f16",
                                  "flops_executed": fl, "ms": filt_ms}
    if ref_ms and cnt:
        gathered = 4.0 * d * cnt["recomputed"]
        lists = 8.0 * cnt["candidates"]
        res["roofline_refine"] = {"kernel": "pf_refine_kernel", "bound": "hbm", "achieved": (gathered + lists) / 1e6 / ref_ms, "peak": HBM_PEAK_GBS,
                                  "unit": "GB/s", "frac": (gathered + lists) / 1e6 / ref_ms / HBM_PEAK_GBS, "ms": ref_ms,
                                  "gathered_row_bytes": gathered, "list_bytes": lists,
                                  "recomputed_per_query": cnt["recomputed"] / max(1, cnt["queries"]),
                                  "candidates_per_query": cnt["candidates"] / max(1, cnt["queries"]), "queries_redone_exactly": cnt["redone"]}
        algo = 4.0 * (q + n) * d + 8.0 * q * k
        images = (4.0 * d + 2.0 * kp) * (n if shared_image else q + n)          # fp32 rows read + half-precision images written
        moved = images + 2.0 * kp * (n + q) + 2.0 * kp * S + gathered + 2.0 * lists + 8.0 * q * k
        res["traffic_vs_algorithmic"] = {"moved_bytes_model": moved, "algorithmic_bytes": algo, "ratio": moved / algo,
                                         "why": "bit-exact results need the exact fp32 chain for every survivor of the half-precision bound: each "
                                                "recomputed entry re-reads one fp32 gallery row (the gather term dominates); the images are read "
                                                "once per pass out of L2 / Infinity Cache and are counted once"}
    return res


def verify_last_step(last, pd, rk, metric, world):
    """AFTER the timed region: the last step's distance matrix and ranking against the oracle (oracle/verify.py -- the checker,
    never the thing measured): every row a permutation / sorted / index-ascending inside ties, the all-pairs matrix equal to its
    transpose bitwise, >= 50 sampled rows bit-equal to canon.c's FMA chain and canonical ranking."""
    try:
        from oracle import verify
        t0 = time.perf_counter()
        feats = last["g"].cpu().numpy()
        queries = None if last["q"] is None else last["q"].cpu().numpy()
        ok, detail = verify.verify_retrieval_step(feats, pd, rk, metric, queries=queries)
        import sehip
        detail["rank_order_guard_violations"] = sehip.rank_rows_check(pd, rk)       # the library's own audit (se_rank_rows_check), all rows
        ok = ok and detail["rank_order_guard_violations"] == 0
        detail["seconds"] = time.perf_counter() - t0
    except Exception as e:       # a checker failure must not lose the measurement, but it must show
        ok, detail = False, {"error": "%s: %s" % (type(e).__name__, e)}
    if world > 1:
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(int(flag.item()))
    return {"verified": bool(ok), "verify_detail": detail}


def pmc_traffic_gb(kernel, q, n, d):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 PMC passes (profiles/pmc_traffic.json:
    FETCH_SIZE with the gfx950 correction of MI355X_MICROARCH.md where it applies, plus WRITE_SIZE, both in KB), or None when
    no profile of this exact shape is committed.  bench.py cannot collect counters itself."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            rec = json.load(f)[kernel]
        if [rec["q"], rec["n"], rec["d"]] != [q, n, d]:
            return None
        ff = rec.get("fetch_factor", 2)   # gfx950: FETCH_SIZE halves wide coalesced reads (x2); other widths count in full
        return {"bytes": (rec["fetch_kb"] * ff + rec["write_kb"]) * 1024.0, "read_GB": rec["fetch_kb"] * ff * 1024 / 1e9,
                "write_GB": rec["write_kb"] * 1024 / 1e9, "source": rec["source"]}
    except Exception:
        return None


def cpu_baseline_retrieval(args, feats_h, rk_gpu=None):
    """The reference's NumPy op sequence (oracle port) on a bounded query sample, host cores.  `value` uses the reference's own
    call, ``np.argsort`` with the default kind (evaluate_retrieval.py:67; NumPy 2.x: a vectorised quicksort); the stable kind
    (the canonical tie order) is timed beside it.

    Same-node parity evidence (not timed): ``host_blas_is_fma_chain`` -- does THIS host's BLAS compute the sequential fp32 FMA chain
    the kernels reproduce (oracle/retrieval_oracle.probe_host_blas_is_fma_chain)?  When it does, the rankings the GPU produced in the
    last timed step (``rk_gpu``) are compared with the host NumPy rankings of the same sampled queries: a row counts as different
    when the distance sequences along the two rankings differ anywhere, i.e. when the rankings disagree OUTSIDE groups of exactly
    equal distances (inside such a group np.argsort's default kind is free to order as it likes).  Expected: 0."""
    from oracle import retrieval_oracle as ro
    qn = min(args.cpu_sample_queries, feats_h.shape[0])
    f = feats_h.copy()
    t0 = time.perf_counter()
    pdm = ro.pdist_numpy(f, normalize=(args.metric == "cosine"), queries=slice(0, qn))
    t1 = time.perf_counter()
    rank = np.argsort(pdm, axis=-1)
    t2 = time.perf_counter()
    qs = min(qn, 2048)                     # the stable kind (canonical tie order) is ~7x slower: timed on a slice
    rank_s = np.argsort(pdm[:qs], axis=-1, kind="stable")
    t3 = time.perf_counter()
    assert rank.shape == (qn, feats_h.shape[0]) and rank_s.shape == (qs, feats_h.shape[0])
    n = feats_h.shape[0]
    parity = {"host_blas_is_fma_chain": None, "gpu_vs_host_rows_compared": 0, "gpu_vs_host_rows_differing_outside_ties": None}
    try:
        parity["host_blas_is_fma_chain"] = bool(ro.probe_host_blas_is_fma_chain(d=feats_h.shape[1]))
        if rk_gpu is not None and parity["host_blas_is_fma_chain"] and tuple(rk_gpu.shape) == (n, n):
            differing = identical = 0
            for r0 in range(0, qn, 2048):
                r1 = min(qn, r0 + 2048)
                g = rk_gpu[r0:r1].cpu().numpy().astype(np.int64)
                a = np.take_along_axis(pdm[r0:r1], g, axis=1)
                b = np.take_along_axis(pdm[r0:r1], rank[r0:r1], axis=1)
                differing += int((a != b).any(axis=1).sum())
                identical += int((g == rank[r0:r1]).all(axis=1).sum())
            parity.update(gpu_vs_host_rows_compared=qn, gpu_vs_host_rows_differing_outside_ties=differing,
                          gpu_vs_host_rows_identical_including_tie_order=identical)
    except Exception as e:       # noqa: BLE001
        parity["error"] = "%s: %s" % (type(e).__name__, e)
    return {"value": qn * n / (t2 - t0) / 1e6, "unit": "Mpairs/s", "cores": os.cpu_count(), "kind": "port", "same_node_parity": parity,
            "value_stable_argsort": n / ((t1 - t0) / qn + (t3 - t2) / qs) / 1e6,
            "seconds": {"norm_and_dot": t1 - t0, "argsort_default": t2 - t1, "argsort_stable_%d_rows" % qs: t3 - t2},
            "sample": "%d of %d queries x %d gallery, D=%d: np.linalg.norm + np.dot (BLAS threads = all cores) + np.argsort "
                      "(default kind as the reference calls it; single-threaded in NumPy), %.1f s" % (qn, n, n, feats_h.shape[1], t2 - t0)}


# ---------------------------------------------------------------------------------------------
# sharded-gallery leg (BASELINE.json configs[4]; north_star: "retrieval shards the gallery with a final RCCL all-gather of
# per-shard top-k")
# ---------------------------------------------------------------------------------------------

def bench_sharded_gallery(args, rank, world, reps=2):
    """50,000 queries (replicated) x world * 160,146 gallery rows (sharded) x D = 1000, k = 251: per-shard fused distance +
    top-k (se_retrieve_topk) -> RCCL all-gather of the [Q, k] (f32, i32) lists -> se_topk_merge; each phase timed separately
    with barriers in between (HIP events on the launch stream for the kernels, host clock around the collective).

    The headline of the leg uses the arithmetic that REPRODUCES the reference at this depth: at D = 1000 the host BLAS behind
    `np.dot` (evaluate_retrieval.py:59) restarts its fp32 chain per K block -- `host_blas_kblocks(1000)` = [448, 276, 276] --
    and one single chain does not give the reference's near-tie order (tests/golden/topk_head_d1000_*).  The single-chain time
    stands beside it (`ms.local_topk_single_chain`).  AFTER the timed region >= 50 sampled queries of this rank's shard result
    are compared with oracle/canon.c run with the same K-block list (`verified`)."""
    import sehip
    from evaluate_retrieval import host_blas_kblocks
    from sharded_retrieval import all_gather_packed
    Q, NS, D, K = args.shard_queries, args.shard_rows, args.shard_dim, args.shard_k
    kblocks = host_blas_kblocks(D)
    kblocks = kblocks if len(kblocks) > 1 else None
    gen = torch.Generator(device="cuda").manual_seed(1000 + rank)
    shard = torch.randn((NS, D), generator=gen, device="cuda", dtype=torch.float32)
    gq = torch.Generator(device="cuda").manual_seed(7)              # the same queries on every rank
    queries = torch.randn((Q, D), generator=gq, device="cuda", dtype=torch.float32)
    sehip.normalize_rows_(shard)
    sehip.normalize_rows_(queries)
    off = rank * NS
    t_local, t_single, t_gather, t_merge = [], [], [], []
    packed = torch.empty((2, Q, K), dtype=torch.int32, device="cuda")          # this rank's all-gather send block: (distance bits | indices)
    d, i = packed[0].view(torch.float32), packed[1]
    md = mi = None
    for it in range(reps + 1):
        barrier_sync(world)
        t0 = time.perf_counter()
        sehip.retrieve_topk(queries, shard, K, metric=sehip.METRIC_COSINE, col_offset=off, kblocks=kblocks, out=(d, i))
        barrier_sync(world)
        t1 = time.perf_counter()
        gathered = all_gather_packed(packed, world)                 # ONE all-gather of the packed lists
        barrier_sync(world)
        t2 = time.perf_counter()
        md, mi = sehip.topk_merge(gathered)                          # se_topk_merge_packed, straight out of the receive buffer
        barrier_sync(world)
        t3 = time.perf_counter()
        if kblocks is not None:                                      # beside it: the one-chain arithmetic (not the reference's at D > 448)
            sehip.retrieve_topk(queries, shard, K, metric=sehip.METRIC_COSINE, col_offset=off)
            barrier_sync(world)
        t4 = time.perf_counter()
        if it > 0:            # first round: workspace allocation, RCCL channel set-up
            t_local.append(t1 - t0)
            t_gather.append(t2 - t1)
            t_merge.append(t3 - t2)
            t_single.append(t4 - t3)
    loc, gat, mer, sgl = (max_over_ranks(float(np.mean(t)), world, "cuda") * 1e3 for t in (t_local, t_gather, t_merge, t_single))
    # size-independent sanity of the merged lists
    sorted_ok = bool((md[:, 1:] >= md[:, :-1]).all()) and bool(((md[:, 1:] > md[:, :-1]) | (mi[:, 1:] > mi[:, :-1])).all())
    in_range = bool(((mi >= 0) & (mi < world * NS)).all())
    total = loc + gat + mer
    flops = 2.0 * Q * NS * D
    out = {"metric": "sharded_retrieval_Mpairs_per_sec", "value": float(Q) * NS * world / total / 1e3, "unit": "Mpairs/s", "n_gpus": world,
           "ms": {"local_topk": loc, "all_gather": gat, "merge": mer, "total": total,
                  "local_topk_single_chain": sgl if kblocks is not None else loc}, "reps": reps,
           "config": {"workload": "ILSVRC-sized sharded-gallery retrieval: %d queries x %d x %d gallery rows, D=%d, k=%d, cosine"
                                  % (Q, world, NS, D, K), "queries": Q, "gallery_rows_per_gpu": NS, "dim": D, "k": K,
                      "kblocks": kblocks, "arithmetic": "fp32 FMA chain restarted per host-BLAS K block (what np.dot computes at this depth)"
                      if kblocks is not None else "one fp32 FMA chain",
                      "parallelism": "gallery sharded %d ways, ONE RCCL all-gather of the packed per-shard top-k lists, canonical merge" % world},
           "all_gather_bytes_per_rank": Q * K * 8, "all_gather_GBps_per_rank": (world - 1) * Q * K * 8 / 1e6 / gat if world > 1 else None,
           "local_topk_useful_TFLOPs": flops / 1e9 / loc,
           "local_topk_note": "useful flops 2 Q N D over the time of the whole call (no peak applies to it: the call bounds the distances on "
                              "the fp16 matrix cores and computes exact fp32 chains only for the survivors -- see roofline_filter / roofline_refine)",
           "merged_lists_sorted_with_index_tiebreak": sorted_ok, "merged_indices_in_range": in_range, "scaling": "weak",
           "data": "synthetic"}
    try:
        out.update(topk_phase_rooflines(lambda: sehip.retrieve_topk(queries, shard, K, metric=sehip.METRIC_COSINE, col_offset=off, kblocks=kblocks, out=(d, i)),
                                        Q, NS, D, K, shared_image=False))
    except Exception as e:      # noqa: BLE001 -- a measuring aid must not lose the leg
        out["phase_ms"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if args.verify:
        try:
            from oracle import verify
            t0 = time.perf_counter()
            rows = verify.sample_rows(Q, n_random=36)
            det = verify.verify_topk_sample(queries.cpu().numpy(), shard.cpu().numpy(), 0, K, d, i, rows, col_offset=off, kblocks=kblocks)
            det["seconds"] = time.perf_counter() - t0
            ok = det["distances_bit_equal"] and det["indices_equal"] and sorted_ok and in_range
        except Exception as e:
            ok, det = False, {"error": "%s: %s" % (type(e).__name__, e)}
        if world > 1:
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device="cuda")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok = bool(int(flag.item()))
        out["verified"], out["verify_detail"] = bool(ok), det
    return out


# ---------------------------------------------------------------------------------------------
# dry mode (CPU plumbing test of the launcher / process-group / line assembly; no kernels, no measurement)
# ---------------------------------------------------------------------------------------------

def bench_dry(args, rank, world):
    """Every leg of the real line on CPU / gloo with oracle stand-ins for the kernels and tiny shapes: the launcher, the process
    group, the sharding arithmetic and the collectives of `sharded_gallery` (gallery shards + all-gather + merge), the
    query-sharded full ranking, and the DP training step (bucketed all-reduce of the flat gradient) -- no measurement."""
    from oracle import retrieval_oracle as ro
    import sharded_retrieval as sr
    import engine
    rng = np.random.default_rng(0)
    gallery = rng.standard_normal((64 * world, 16)).astype(np.float32)
    queries = torch.from_numpy(gallery[:8].copy())
    lo, hi = sr.shard_bounds(len(gallery), world)[rank]

    def local_topk(q, g, k, off, kblocks=None):
        d, i = ro.canon_topk_rows(ro.canon_pdist(q.numpy(), g.numpy(), ro.METRIC_COSINE, kblocks=kblocks), k, col_offset=off)
        return torch.from_numpy(d), torch.from_numpy(i)

    def merge(d, i):
        md, mi = ro.canon_topk_merge(d.numpy(), i.numpy())
        return torch.from_numpy(md), torch.from_numpy(mi)

    barrier_sync(world, dry=True)
    t0 = time.perf_counter()
    # ---- sharded_gallery: every rank holds 1 / world of the gallery; per-shard top-k -> all-gather -> merge ----
    d, i = sr.sharded_topk(queries, torch.from_numpy(gallery[lo:hi]), 5, lo, local_topk=local_topk, merge=merge)
    want = ro.canon_topk_rows(ro.canon_pdist(gallery[:8], gallery, ro.METRIC_COSINE), 5)[1]
    sharded = {"parts": world, "matches_unsharded": bool(np.array_equal(i.numpy(), want))}
    # ---- retrieval, strong scaling: the query rows of ONE feature set sharded, gallery replicated, no data-path collective ----
    q0, q1 = sr.shard_bounds(len(gallery), world)[rank]
    mine = ro.canon_rank_rows(ro.canon_pdist(gallery[q0:q1], gallery, ro.METRIC_COSINE)) if q1 > q0 else np.zeros((0, len(gallery)), np.int32)
    sums = torch.tensor([float(mine.astype(np.int64).sum()), float(mine.shape[0])], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(sums)
    full = ro.canon_rank_rows(ro.canon_pdist(gallery, gallery, ro.METRIC_COSINE))
    retrieval = {"query_shards": world, "rows_ranked": int(sums[1].item()),
                 "matches_unsharded": bool(np.array_equal(mine, full[q0:q1])) and int(sums[1].item()) == len(gallery)
                 and float(sums[0].item()) == float(full.astype(np.int64).sum())}
    # ---- train: DP step (one process per rank, flat gradient buffer, bucketed all-reduce, update); strong scaling splits ONE batch ----
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4))
    tr = engine.Trainer(model, {"o": (lambda y, x: ((x - y) ** 2).sum(-1), 1.0)}, {}, lr=0.05, momentum=0.9, clipnorm=10.0,
                        autocast_dtype=None, bucket_bytes=256)
    g = torch.Generator().manual_seed(1)
    per = 4
    X, Y = torch.randn(per * world, 6, generator=g), torch.randn(per * world, 4, generator=g)
    logs = {}
    for _ in range(2):
        tr.train_step(X[rank * per:(rank + 1) * per], Y[rank * per:(rank + 1) * per], logs)
    csum = torch.tensor([float(tr.flat.flat_p.double().sum())], dtype=torch.float64)
    lo_hi = torch.stack([csum, -csum])
    if world > 1:
        dist.all_reduce(lo_hi, op=dist.ReduceOp.MAX)
    train = {"ranks": world, "global_batch": per * world, "replicas_identical": bool(abs(float(lo_hi[0]) + float(lo_hi[1])) < 1e-9),
             "loss_finite": bool(np.isfinite(float(torch.as_tensor(logs["loss"]))))}
    barrier_sync(world, dry=True)
    dt = max_over_ranks(time.perf_counter() - t0, world, "cpu")
    return {"metric": "dry_run", "value": 0.0, "unit": "none", "n_gpus": world, "dry": True, "steps": 1, "warmup": 0, "scaling": args.scaling,
            "ms_per_step": dt * 1e3, "sharded_topk_matches_unsharded": sharded["matches_unsharded"], "sharded_gallery": sharded,
            "retrieval": retrieval, "train": train, "data": "synthetic"}


# ---------------------------------------------------------------------------------------------

def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    rc = maybe_spawn(args, argv)
    if rc is not None:
        sys.exit(rc)
    rank, world, local = init_dist(args)
    pre = preflight(args, rank, world, local)
    if args.dry:
        out = bench_dry(args, rank, world)
    elif args.workload == "train":
        from train_bench import bench_train
        out = bench_train(args, rank, world, scaling=args.scaling)
        if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
            from train_bench import cpu_baseline_train
            out["cpu_baseline"] = cpu_baseline_train(args)
    else:
        out, feats_h, rk = bench_retrieval(args, rank, world)
        if args.full:                 # a plain run stops at the headline: every secondary leg below is --full only

            def leg(name, fn):        # the retrieval line must survive a failure of a secondary leg -- but every rank must agree
                try:
                    out[name] = fn()
                except Exception as e:
                    out[name] = {"error": "%s: %s" % (type(e).__name__, e)}

            leg("hierarchical_precision", lambda: bench_metrics(args, rk))
            if rank == 0 and world == 1 and "error" not in out and args.metric == "cosine":
                leg("guaranteed_order", lambda: bench_guaranteed_order(args))
                if "kernels" in out and "error" not in out.get("guaranteed_order", {"error": 1}):
                    out["kernels"]["rank_rows"]["guaranteed_order_ms"] = out["guaranteed_order"]["ms_scaled_to_step"]
            if rank == 0 and world == 1 and not args.no_cpu_baseline:      # reported baseline: rank 0 at N = 1 only, bounded sample; it also
                leg("cpu_baseline", lambda: cpu_baseline_retrieval(args, feats_h, rk))   # compares rk with the host ranks
            del rk
            torch.cuda.empty_cache()
            leg("retrieve_topk", lambda: bench_topk_all_pairs(args, feats_h))
            torch.cuda.empty_cache()
            leg("rank_long_rows", lambda: bench_rank_long_rows(args))
            torch.cuda.empty_cache()
            if rank == 0 and world == 1:
                leg("eval_e2e", lambda: bench_eval_e2e(args))
                torch.cuda.empty_cache()
            if args.with_sharded:
                leg("sharded_gallery", lambda: bench_sharded_gallery(args, rank, world))
                torch.cuda.empty_cache()
            if args.with_train:
                from train_bench import bench_train
                sc = args.scaling
                # configs[1]: ResNet-110-fc, batch 128.  The product default for the CIFAR nets is fp32 + HIP-graph replay (bf16 autocast only
                # adds cast launches to 16-64-channel convolutions); BASELINE says bf16, so that number stands beside it.
                leg("train", lambda: bench_train(args, rank, world, scaling=sc))
                leg("train_bf16", lambda: bench_train(args, rank, world, dtype="bf16", scaling=sc))
                if "error" not in out["train"] and "error" not in out["train_bf16"]:
                    out["train"]["bf16_images_per_sec"] = out["train_bf16"]["value"]
                if "error" not in out["train"] and sc == "weak":
                    # per-GPU batch sweep beside the stated batch: shows how far configs[1] sits inside the launch-bound regime
                    sweep = {str(args.batch): {"images_per_sec": out["train"]["value"], "ms_per_step": out["train"]["ms_per_step"]}}
                    for bsz in (256, 512):
                        if bsz == args.batch:
                            continue
                        try:
                            r = bench_train(argparse.Namespace(**dict(vars(args), batch=bsz, steps=min(args.steps, 10), warmup=min(args.warmup, 3))), rank, world, scaling=sc)
                            sweep[str(bsz)] = {"images_per_sec": r["value"], "ms_per_step": r["ms_per_step"]}
                        except Exception as e:
                            sweep[str(bsz)] = {"error": "%s: %s" % (type(e).__name__, e)}
                        torch.cuda.empty_cache()
                    out["train"]["batch_sweep_per_gpu"] = sweep
                r50 = argparse.Namespace(**dict(vars(args), arch="resnet-50", batch=64))
                leg("train_r50", lambda: bench_train(r50, rank, world, scaling=sc))                            # configs[3]: CUB, 200 classes
                leg("train_r50_ilsvrc", lambda: bench_train(r50, rank, world, classes=1000, scaling=sc))    # configs[4]: C = D = 1000
                r50b = argparse.Namespace(**dict(vars(args), arch="resnet-50", batch=128))                  # B = 128 per GPU
                leg("train_r50_b128", lambda: bench_train(r50b, rank, world, scaling=sc))
                leg("train_r50_ilsvrc_b128", lambda: bench_train(r50b, rank, world, classes=1000, scaling=sc))
            if rank == 0 and world == 1 and not args.no_cpu_baseline:      # reported baselines: rank 0 at N = 1 only, bounded samples
                if args.with_train and "error" not in out["train"]:
                    try:
                        from train_bench import cpu_baseline_train
                        out["train"]["cpu_baseline"] = cpu_baseline_train(args)
                    except Exception as e:
                        out["train"]["cpu_baseline"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if isinstance(out.get("roofline"), dict) and isinstance(out.get("config"), dict) and not args.dry and args.workload != "train":
        # scalars mirrored to where the driver's parsed subset keeps them
        sg, cb = out.get("sharded_gallery"), out.get("cpu_baseline")
        if isinstance(sg, dict) and "verified" in sg:
            out["roofline"]["sharded_gallery_verified"] = out["config"]["sharded_gallery_verified"] = sg["verified"]
        if isinstance(cb, dict) and isinstance(cb.get("same_node_parity"), dict):
            v = cb["same_node_parity"].get("gpu_vs_host_rows_differing_outside_ties")
            out["roofline"]["same_node_rows_differing_outside_ties"] = v
            cb["gpu_vs_host_rows_differing_outside_ties"] = v
    if world > 1:
        out["preflight"] = pre
    try:
        out["rccl"] = comm_identity(world, dry=args.dry)
        mg = multi_gpu_summary(out, world)
        if mg is not None:
            out["multi_gpu"] = mg
    except Exception as e:       # noqa: BLE001 -- identity fields must never lose the measurement
        out["rccl"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if rank == 0:
        print(json.dumps(out))
        sys.stdout.flush()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
