#!/usr/bin/env python
"""Kernel-level microbenchmarks (HIP-event timing on the launch stream) used while tuning.
    python tools/bench_kernels.py pdist|rank|loss|topk [--n 50000 --d 100 --reps 5]
    python tools/bench_kernels.py pdist64 [--n 50000 --d 100]   (the opt-in float64 retrieval step, leg by leg: float64 distances, their float32
                                                  image, se_rank_rows on it, se_rank_refine_f64; the float32 step next to them)
    python tools/bench_kernels.py hxe            (se_hxe_fwd + _bwd and se_soft_xent_fwd + _bwd next to a torch composition of each loss and
                                                  to se_softmax_xent_fwd + _bwd: 128 x 100 on the CIFAR tree, 128 x 1000 on the ILSVRC
                                                  min-tree, 256 x 8142 on the iNaturalist 2018 tree; --n / --d are not used)
    python tools/bench_kernels.py crm            (CRM decoding with top = 20: se_tree_risk_topk next to the dense composition on se_pairwise_dist +
                                                  se_topk_rows and to a torch float64 composition: 10,000 x 100 on the CIFAR tree, 50,000 x 1000
                                                  on the ILSVRC min-tree, 24,426 x 8142 on the iNaturalist 2018 tree; --n / --d are not used)
    python tools/bench_kernels.py knn            (se_knn_vote next to the torch composition gather -> scatter_add -> topk, and the whole
                                                  knn_classification: 10,000 x 50,000 x 100 with k = 20, 100 classes; 50,000 x 50,000 x 100 with
                                                  k = 200, 1000 classes; --n / --d are not used)
    python tools/bench_kernels.py ranked         (se_complete_rankings at 10,000 x 10,000 and 50,000 x 50,000, list lengths 0 / 250 / N, both
                                                  order forms, next to a copy of the same bytes and a torch composition; the whole
                                                  hierarchical_precision_ranked next to the host function; --n / --d are not used)
    python tools/bench_kernels.py bootstrap      (se_bootstrap_means at q = 10,000 and 50,000 queries x 11 columns x 10,000 replicates next to
                                                  the torch composition randint -> index_select -> mean in chunks that fit memory; --n / --d
                                                  are not used)
    python tools/bench_kernels.py recprec        (10k x 10k and 50k x 50k, 100 classes; --n is not used)
    python tools/bench_kernels.py svm            (margin + reduction kernels and whole LinearSVC fits: 50,000 x 100 x 100 and
                                                  1,281,167 x 1000 x 1000; --n / --d are not used; --svm-sizes small skips the large one)
    python tools/bench_kernels.py classemb       (class pair tables, fp64 Cholesky and the fp64 eigensolver (next to np.linalg.eigh) at C = 1000
                                                  (ILSVRC WordNet DAG) and 8,142 (iNat 2018), and whole compute_class_embedding.py runs on the
                                                  iNat hierarchy: unitsphere, and approx_sim with the device and the host eigensolver)
    python tools/bench_kernels.py center         (center loss forward / input gradient / centroid gradient at D = 100, and the
                                                  ResNet-110-fc center-loss training step next to the cosine-loss one)
    python tools/bench_kernels.py xent           (softmax cross-entropy forward + backward next to the torch composition the sibling
                                                  CLIs use, f32 / bf16 logits, s = 0 / 0.1, and the ResNet-110 classifier step)
    python tools/bench_kernels.py image          (se_image_batch: a batch of 128 at the CUB preset (375 x 500 sources, shorter side 512,
                                                  crop 448) and at the NAB preset (about 768 x 1024 sources, random zoom 256-480, crop
                                                  224): kernel time, host time, bytes over kernel time, next to the ResNet-50 step)
    python tools/bench_kernels.py adagrad        (se_adagrad_step over the flat buffers of ResNet-110-fc and ResNet-50, with and without the
                                                  regulariser, next to the torch composition of the same update, and the ResNet-110-fc
                                                  DeViSE training step next to the cosine-loss one)
    python tools/bench_kernels.py sgd            (the fused Keras-SGD pair sehip.grad_clip_factor + sehip.sgd_step_ next to the torch composition
                                                  of Trainer.apply_update at 1.75 M, 25.6 M and 68 M floats per buffer, {clip + regulariser,
                                                  clip only, neither} x {plain, Nesterov}, and the ResNet-110-fc cosine-loss step with and
                                                  without Trainer(fused_sgd=True))
    python tools/bench_kernels.py labelembed     (label-embedding loss forward + backward on the learned table next to the composition it
                                                  replaces -- Embedding gather, loss on the gathered rows, torch's embedding backward -- as
                                                  bare kernels and through autograd, and the ResNet-110-fc label-embedding training step
                                                  next to the classifier step)
    python tools/bench_kernels.py tiny           (se_tiny_batch: batches of 128 and 512 CIFAR images with the 'cifar-10' preset -- shifts,
                                                  zoom, flip -- as the bare kernel and as the whole compose_batch, next to the torch
                                                  composition of the default shift + flip batch)
    python tools/bench_kernels.py shortcut       (sehip.shortcut_add forward + backward next to the torch composition avg_pool2d + pad + add
                                                  at PyramidNet-272-200's shapes for batch 128: the widest stride-1 block of each stage and
                                                  both stride-2 blocks, fp32 NCHW and bf16 NHWC)
    python tools/bench_kernels.py stream         (the streamed image store, datasets/files.py: 2,048 seeded 500 x 375 JPEGs written to a
                                                  temporary directory, the ILSVRC preset at batch 128 with 16 decode threads: images/s of
                                                  streamed composition with look-ahead 0, 2 and 4, its split into decode, packing, upload
                                                  and tables + se_image_batch, and the resident composition of the same images)
    python tools/bench_kernels.py joint          (the joint head of --cls_weight, forward + backward: today's torch composition, the
                                                  embedding role and se_softmax_xent_* as separate launches, and the one joint launch)
    python tools/bench_kernels.py qg [--small] [--ranking-path]
                                                 (one query-vs-gallery AP leg, recall_precision_device(..., gallery=...): 50,000 queries x
                                                  1,281,167 gallery rows x D = 1000, 1000 classes of ~1281 rows; --small: 2,000 x 60,000 x
                                                  100, 100 classes; --q / --n / --d override.  Time per phase: relevant keys, distance
                                                  slabs, counting, scan + reduce.  --ranking-path: the same positions from full rankings of
                                                  --rank-rows query rows -- se_pairwise_dist + se_rank_rows + se_relevant_positions, the only
                                                  way before the counting kernel -- scaled to all queries.  Then the whole-list phase:
                                                  hierarchical_precision_device(..., gallery=..., rank_gallery=True) with un-clipped AHP +
                                                  AP on the CIFAR-100 taxonomy (classes folded onto its 100 leaves) -- distances, ranking
                                                  and metric kernel per phase -- next to the clipped top-k + counting path (AHP@250 + AP)
                                                  on the same problem; --whole-rows N ranks only the first N queries and scales, for
                                                  galleries whose rows take the tiled ranking kernel; --whole-only skips the AP leg)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
import sehip  # noqa: E402


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def windows(fns, reps, batch):
    """The method of the alternating benchmarks: 3 warm-up calls of every candidate, then ``reps`` rounds in which the candidates take
    turns (the same machine state for every candidate), each timed by HIP events around a window of ``batch`` back-to-back calls.
    Per candidate: (median, 10th percentile, 90th percentile) of the per-call time in microseconds."""
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                f()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / batch * 1e3)
    return [(float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pdist", "rank", "loss", "topk", "fused", "hprec", "recprec", "shard", "rownorm", "svm", "classemb",
                                     "center", "xent", "image", "adagrad", "labelembed", "tiny", "shortcut", "qg", "stream", "head", "joint", "sgd", "pdist64", "knn", "ranked", "bootstrap", "ndcg", "hxe", "crm"])
    ap.add_argument("--small", action="store_true", help="qg: 2,000 x 60,000 x 100 instead of 50,000 x 1,281,167 x 1000")
    ap.add_argument("--ranking-path", action="store_true", help="qg: time full rankings of --rank-rows queries of the same problem instead")
    ap.add_argument("--rank-rows", type=int, default=1024, help="qg --ranking-path: query rows ranked (the time is scaled to all queries)")
    ap.add_argument("--whole-rows", type=int, default=None, help="qg, whole-list phase: rank the first N queries only (times scaled to all)")
    ap.add_argument("--whole-only", action="store_true", help="qg: the whole-list phase only")
    ap.add_argument("--classes", type=int, default=None, help="qg: number of classes")
    ap.add_argument("--noise", type=float, default=0.7, help="qg: standard deviation of the noise around the class centres (0.7: separable classes, mAP 1)")
    ap.add_argument("--hp-mode", default="all", choices=["all", "whole", "sweep"], help="hprec: every configuration, or whole-list AHP + AP in class order only (profiling)")
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--q", type=int, default=None)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--k", type=int, default=251)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--svm-sizes", default="all", choices=["all", "small"], help="svm: both sizes, or 50,000 x 100 x 100 only")
    args = ap.parse_args()
    if args.what == "classemb":
        return bench_classemb(args.reps)
    if args.what == "center":
        return bench_center()
    if args.what == "ndcg":
        return bench_ndcg()
    if args.what == "xent":
        return bench_xent()
    if args.what == "hxe":
        return bench_hxe()
    if args.what == "crm":
        return bench_crm()
    if args.what == "image":
        return bench_image()
    if args.what == "adagrad":
        return bench_adagrad()
    if args.what == "sgd":
        return bench_sgd()
    if args.what == "labelembed":
        return bench_labelembed()
    if args.what == "tiny":
        return bench_tiny()
    if args.what == "shortcut":
        return bench_shortcut()
    if args.what == "qg":
        return bench_qg(args)
    if args.what == "stream":
        return bench_stream()
    if args.what == "head":
        return bench_head()
    if args.what == "joint":
        return bench_joint()
    if args.what == "knn":
        return bench_knn()
    if args.what == "ranked":
        return bench_ranked()
    if args.what == "bootstrap":
        return bench_bootstrap()
    if args.what == "pdist64":
        return bench_pdist64(args.n, args.d, max(args.reps, 10))
    n, d = args.n, args.d
    q = args.q or n
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((n, d)).astype(np.float32)).cuda()
    sehip.normalize_rows_(x)
    if args.what == "rownorm":
        # se_normalize_rows / se_row_sqnorm at the retrieval shapes: CIFAR (50k x 100: one lane per row) and one ILSVRC gallery
        # shard (160,146 x 1000: one wave per row)
        for rows, dd in ((50000, 100), (160146, 1000), (160146, 555), (40000, 4096)):
            y = torch.from_numpy(np.random.default_rng(3).standard_normal((rows, dd)).astype(np.float32)).cuda()
            med, mn = timeit(lambda: sehip.normalize_rows_(y), args.reps)
            print("normalize_rows %d x %d: median %.3f ms (min %.3f)  %.2f TB/s (read + write)" % (rows, dd, med, mn, 8.0 * rows * dd / med / 1e9))
            med, mn = timeit(lambda: sehip.row_sqnorm(y), args.reps)
            print("row_sqnorm     %d x %d: median %.3f ms (min %.3f)  %.2f TB/s (read)" % (rows, dd, med, mn, 4.0 * rows * dd / med / 1e9))
        return
    if args.what == "pdist":
        out = torch.empty((q, n), dtype=torch.float32, device="cuda")
        y = x.clone()
        for name, b in (("symmetric(a==b)", x), ("general(a!=b)", y)):
            med, mn = timeit(lambda: sehip.pairwise_dist(x[:q], b, metric=sehip.METRIC_COSINE, out=out), args.reps)
            gb = (4.0 * q * n + 4.0 * (q + n) * d) / 1e9
            print("pdist %-16s q=%d n=%d d=%d: median %.3f ms (min %.3f)  %.1f GB/s algorithmic, %.1f TFLOP/s useful" %
                  (name, q, n, d, med, mn, gb / med * 1e3, 2.0 * q * n * d / med / 1e9))
        xe = torch.from_numpy(np.random.default_rng(0).standard_normal((n, d)).astype(np.float32)).cuda()
        sq = sehip.row_sqnorm(xe)
        for name, b in (("Euclid symmetric", xe), ("Euclid general", xe.clone())):
            med, mn = timeit(lambda: sehip.pairwise_dist(xe[:q], b, metric=sehip.METRIC_EUCLID, sqa=sq[:q], sqb=sq, out=out), args.reps)
            print("pdist %-16s q=%d n=%d d=%d: median %.3f ms (min %.3f)  %.1f GB/s algorithmic" % (name, q, n, d, med, mn, gb / med * 1e3))
    elif args.what == "rank":
        pd = sehip.pairwise_dist(x[:q], x, metric=sehip.METRIC_COSINE)
        rk = torch.empty((q, n), dtype=torch.int32, device="cuda")
        med, mn = timeit(lambda: sehip.rank_rows(pd, out=rk), args.reps)
        print("rank q=%d n=%d: median %.3f ms (min %.3f)  %.1f GB/s algorithmic, %.1f Mkeys/s" % (q, n, med, mn, 8.0 * q * n / med / 1e6, q * n / med / 1e3))
        # the CLI-default Euclidean branch: all-positive distances (skewed top digit -> the group-peeling build)
        xe = torch.from_numpy(np.random.default_rng(0).standard_normal((n, d)).astype(np.float32)).cuda()
        sq = sehip.row_sqnorm(xe)
        pd = sehip.pairwise_dist(xe[:q], xe, metric=sehip.METRIC_EUCLID, sqa=sq[:q], sqb=sq, out=pd)
        med, mn = timeit(lambda: sehip.rank_rows(pd, out=rk), args.reps)
        print("rank (Euclidean rows) q=%d n=%d: median %.3f ms (min %.3f)  %.1f GB/s algorithmic" % (q, n, med, mn, 8.0 * q * n / med / 1e6))
        # rows above 53,248 columns: two sorted runs + merge (real cosine rows: 8,192 queries against a 100,000-row gallery)
        del pd, rk
        xl = torch.from_numpy(np.random.default_rng(2).standard_normal((100000, d)).astype(np.float32)).cuda()
        sehip.normalize_rows_(xl)
        pdl = sehip.pairwise_dist(xl[:8192], xl, metric=sehip.METRIC_COSINE)
        rkl = torch.empty((8192, 100000), dtype=torch.int32, device="cuda")
        med, mn = timeit(lambda: sehip.rank_rows(pdl, out=rkl), args.reps)
        print("rank (long rows) q=8192 n=100000: median %.3f ms (min %.3f)  %.2f ps per key, %.1f GB/s algorithmic" % (med, mn, med * 1e9 / (8192 * 100000), 8.0 * 8192 * 100000 / med / 1e6))
    elif args.what == "hprec":
        C = 100
        rng = np.random.default_rng(1)
        cls = torch.from_numpy(rng.integers(0, C, size=n).astype(np.int32)).cuda()
        tab = rng.random((C, C)); tab = (tab + tab.T) / 2; np.fill_diagonal(tab, 1.0)
        counts = np.bincount(cls.cpu().numpy(), minlength=C)
        best = np.stack([np.cumsum(np.repeat(tab[c][np.argsort(-tab[c], kind="stable")], counts[np.argsort(-tab[c], kind="stable")])) for c in range(C)])
        tab_d, best_d = torch.from_numpy(tab).cuda(), torch.from_numpy(best).cuda()
        qq = min(q, 8192) if args.q is None else q          # (--q given: that many queries, e.g. the full 50,000)
        pd = sehip.pairwise_dist(x[:qq], x, metric=sehip.METRIC_COSINE)
        rk = sehip.rank_rows(pd)
        ks = torch.arange(1, 251, dtype=torch.int32, device="cuda")
        qidx = torch.arange(qq, dtype=torch.int32, device="cuda")
        curves = sehip.hprec_reciprocal_curves(best_d, best_d)
        qcls = cls[:qq].contiguous()
        for name, ahp in (("whole-list AHP + AP", 0), ("AHP@250, no AP", 250))[:1 if args.hp_mode != "all" else 2]:
            for order in (True, False)[:1 if args.hp_mode != "all" else 2]:
                med, mn = timeit(lambda: sehip.hierarchical_precision(rk, cls, qcls, qidx, tab_d, tab_d, best_d, best_d, ks, ahp_len=ahp,
                                                                      want_ap=(ahp == 0), curves=curves, class_order=order), args.reps)
                print("hprec %-22s %-14s q=%d n=%d: median %.3f ms (min %.3f)  %.1f GB/s of ranks, %.1f Mranks/s" %
                      (name, "class order" if order else "query order", qq, n, med, mn, 4.0 * qq * n / med / 1e6, qq * n / med / 1e3))
        if args.hp_mode == "sweep":     # per-query overhead (intercept) vs per-rank cost (slope)
            for ll in (512, 4096, 8192, 16384, 32768, n):
                med, mn = timeit(lambda: sehip.hierarchical_precision(rk, cls, qcls, qidx, tab_d, tab_d, best_d, best_d, ks, ahp_len=0, want_ap=True,
                                                                      curves=curves, class_order=True, list_len=ll), args.reps)
                print("hprec sweep list_len=%d: median %.3f ms" % (ll, med))
        med, mn = timeit(lambda: sehip.hprec_reciprocal_curves(best_d, best_d), args.reps)
        print("hprec reciprocal curves C=%d n=%d: median %.3f ms" % (C, n, med))
    elif args.what == "recprec":
        # se_relevant_positions (kernel A) and se_recall_precision_reduce (kernel B) on full all-pairs rankings of clustered features,
        # 100 classes; labels drawn at random per item, or class-sorted (item i of class i * C // n).  Kernel A's bytes are those of
        # the 2048-rank chunks it streams before its early exit (one chunk of look-ahead included).
        C, chunk = 100, 2048
        for nn in (10000, 50000):
            rng = np.random.default_rng(7)
            for layout in ("random ids", "class-sorted ids"):
                lab = rng.integers(0, C, size=nn) if layout == "random ids" else (np.arange(nn) * C // nn)
                feats = (rng.standard_normal((C, d)) * 0.5)[lab] + rng.standard_normal((nn, d))
                xf = torch.from_numpy(feats.astype(np.float32)).cuda()
                sehip.normalize_rows_(xf)
                rk = sehip.rank_rows(sehip.pairwise_dist(xf, None, metric=sehip.METRIC_COSINE))
                cls_h = lab.astype(np.int32)
                counts = np.bincount(cls_h, minlength=C)
                r_cls = counts - 1
                hit_off_h = np.concatenate([[0], np.cumsum(r_cls[cls_h])]).astype(np.int64)
                class_off = torch.from_numpy(np.concatenate([[0], np.cumsum(r_cls)]).astype(np.int64)).cuda()
                order = torch.from_numpy(np.argsort(cls_h, kind="stable").astype(np.int32)).cuda()
                cstart = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
                cls, hit_off = torch.from_numpy(cls_h).cuda(), torch.from_numpy(hit_off_h).cuda()
                qidx = torch.arange(nn, dtype=torch.int32, device="cuda")
                out = torch.empty(int(hit_off_h[-1]), dtype=torch.int32, device="cuda")
                run_a = lambda r: sehip.relevant_positions(r, cls, cls, qidx, hit_off, num_classes=C, total=int(hit_off_h[-1]), out=out)
                med, mn = timeit(lambda: run_a(rk), args.reps)
                last = out.cpu().numpy()[hit_off_h[1:] - 1].astype(np.int64)
                read = np.minimum((last + chunk) // chunk + 1, (nn + chunk - 1) // chunk) * chunk
                frac = float(np.minimum(read, nn).sum()) / (float(nn) * nn)
                gbs = 4.0 * frac * nn * nn / med / 1e6
                print("recprec A  int32 %-16s %d x %d: median %.3f ms (min %.3f)  %.1f%% of rank bytes read, %.2f TB/s over them "
                      "(%.0f%% of ~6.3 TB/s)" % (layout, nn, nn, med, mn, 100 * frac, gbs / 1e3, gbs / 63.0))
                rk16 = sehip.rank_rows(sehip.pairwise_dist(xf, None, metric=sehip.METRIC_COSINE), idx16=True)
                med, mn = timeit(lambda: run_a(rk16), args.reps)
                print("recprec A  uint16 %-15s %d x %d: median %.3f ms (min %.3f)" % (layout, nn, nn, med, mn))
                del rk16
                apv = torch.zeros(nn, dtype=torch.float64, device="cuda")
                psum = torch.zeros(int(class_off[-1].item()), dtype=torch.float64, device="cuda")
                miss = torch.zeros(C, dtype=torch.int64, device="cuda")
                for bins in (0, 10, 1000):
                    bs = torch.zeros((C, bins + 1), dtype=torch.float64, device="cuda")
                    bc = torch.zeros((C, bins + 1), dtype=torch.int64, device="cuda")
                    med, mn = timeit(lambda: sehip.recall_precision_reduce(out, hit_off, order, cstart, class_off, bins, apv, psum, miss,
                                                                           bs, bc), args.reps)
                    print("recprec B  bins=%-5d %-16s %d x %d: median %.3f ms (min %.3f)  %d positions" %
                          (bins, layout, nn, nn, med, mn, int(hit_off_h[-1])))
                del rk, xf, out
                torch.cuda.empty_cache()
    elif args.what == "svm":
        # Both kernels of svm.hip and whole fits (linear_svm.LinearSVC, C = 0.1, tol 1e-4) on clustered features: class centres
        # plus noise, labels uniform.  MFMA peak: 157.3 TFLOP/s fp32 (MI355X_MICROARCH.md); a kernel's FLOPs are 2 N D C.
        import time
        import linear_svm as ls
        peak = 157.3e12
        sizes = [(50000, 100, 100)] + ([] if args.svm_sizes == "small" else [(1281167, 1000, 1000)])
        for n, dd, c in sizes:
            g = torch.Generator(device="cuda").manual_seed(0)
            y = torch.randint(0, c, (n,), device="cuda", generator=g)
            X = torch.randn((c, dd), device="cuda", generator=g)[y] / np.sqrt(dd)
            X += 0.5 * torch.randn((n, dd), device="cuda", generator=g) / np.sqrt(dd)
            y_h = y.cpu().numpy()
            ops = ls._DeviceOps(X, y_h, 0.1, c)
            ops.set_columns(np.arange(c))
            W = ops.zeros(c)
            W[:, :dd + 1] = 0.01 * torch.randn((c, dd + 1), device="cuda", generator=g)
            flops = 2.0 * n * dd * c
            nblk = sehip.ops.svm_loss_blocks(n)
            for mode, name in ((sehip.SVM_GRAD, "margin/grad"), (sehip.SVM_HV, "margin/Hv"), (sehip.SVM_SCORE, "margin/score")):
                run = lambda: sehip.svm_margin(mode, X, W, d=dd, labels=ops.labels, col_class=ops.cols, cpen=0.1, mask=ops.mask,
                                               out=ops.Z, loss_part=ops.loss if mode == sehip.SVM_GRAD else None)
                med, mn = timeit(run, args.reps)
                print("svm %-13s %d x %d x %d: median %.3f ms (min %.3f)  %.1f TFLOP/s = %.2f of fp32 MFMA peak" %
                      (name, n, dd, c, med, mn, flops / med / 1e9, flops / med / 1e9 / (peak / 1e12)))
            ws = ops._workspace(c)
            G = ops.zeros(c)
            med, mn = timeit(lambda: sehip.svm_reduce(ops.Z, X, d=dd, plus=W, out=G, workspace=ws), args.reps)
            f2 = 2.0 * n * (dd + 1) * c
            print("svm %-13s %d x %d x %d: median %.3f ms (min %.3f)  %.1f TFLOP/s = %.2f of fp32 MFMA peak  (workspace %.0f MB)" %
                  ("reduce", n, dd, c, med, mn, f2 / med / 1e9, f2 / med / 1e9 / (peak / 1e12), ws.numel() / 1e6))
            del ops, G, ws, W
            torch.cuda.empty_cache()
            for rep in range(2):             # the first fit includes first-launch costs
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                svm = ls.LinearSVC(C=0.1).fit(X, y_h)
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
            print("svm fit           %d x %d x %d: %.3f s (second fit), %d outer iterations (max over classes)" % (n, dd, c, t, svm.n_iter_))
            del X, svm
            torch.cuda.empty_cache()
    elif args.what == "shard":
        # BASELINE.json configs[4], one rank's share: 50,000 queries x (1,281,167 / 8) gallery rows, D = 1000, top-251, then the
        # merge of the 8 all-gathered lists (synthetic: 8 copies with shifted indices)
        D, Q, NS, K = 1000, args.q or 50000, 160146, args.k
        g = torch.from_numpy(np.random.default_rng(1).standard_normal((NS, D)).astype(np.float32)).cuda()
        qq = torch.from_numpy(np.random.default_rng(2).standard_normal((Q, D)).astype(np.float32)).cuda()
        sehip.normalize_rows_(g); sehip.normalize_rows_(qq)
        med, mn = timeit(lambda: sehip.retrieve_topk(qq, g, K, metric=sehip.METRIC_COSINE, col_offset=NS), max(2, args.reps // 2))
        print("shard retrieve_topk (one chain) q=%d n=%d d=%d k=%d: median %.1f ms (min %.1f)  %.1f Mpairs/s, %.1f TFLOP/s useful" %
              (Q, NS, D, K, med, mn, Q * NS / med / 1e3, 2.0 * Q * NS * D / med / 1e9))
        kb = [448, 276, 276]                  # evaluate_retrieval.host_blas_kblocks(1000): the arithmetic that reproduces np.dot at this depth
        med, mn = timeit(lambda: sehip.retrieve_topk(qq, g, K, metric=sehip.METRIC_COSINE, col_offset=NS, kblocks=kb), max(2, args.reps // 2))
        print("shard retrieve_topk (K-blocks %s) q=%d n=%d d=%d k=%d: median %.1f ms (min %.1f)  %.1f Mpairs/s, %.1f TFLOP/s useful" %
              (kb, Q, NS, D, K, med, mn, Q * NS / med / 1e3, 2.0 * Q * NS * D / med / 1e9))
        od, oi = sehip.retrieve_topk(qq, g, K, metric=sehip.METRIC_COSINE)
        dd = torch.stack([od + 1e-3 * r for r in range(8)]); ii = torch.stack([oi + NS * r for r in range(8)])
        med, mn = timeit(lambda: sehip.topk_merge(dd, ii), args.reps)
        print("topk_merge parts=8 q=%d k=%d: median %.3f ms  (all-gather payload %.1f MB per rank)" % (Q, K, med, Q * K * 8 / 1e6))
    elif args.what == "fused":
        # se_retrieve_topk, all-pairs (queries == gallery): distances + top-k with no [q, n] matrix
        for metric, name in ((sehip.METRIC_COSINE, "cosine"), (sehip.METRIC_EUCLID, "Euclid")):
            sq = sehip.row_sqnorm(x) if metric == sehip.METRIC_EUCLID else None
            med, mn = timeit(lambda: sehip.retrieve_topk(x[:q], x, args.k, metric=metric, sqq=None if sq is None else sq[:q], sqg=sq), args.reps)
            print("fused retrieve_topk %-6s q=%d n=%d d=%d k=%d: median %.3f ms (min %.3f)  %.1f Mpairs/s, %.1f TFLOP/s (fp32 MFMA), %.2f GB algorithmic" %
                  (name, q, n, d, args.k, med, mn, q * n / med / 1e3, 2.0 * q * n * d / med / 1e9, (4.0 * (q + n) * d + 8.0 * q * args.k) / 1e9))
    elif args.what == "topk":
        pd = sehip.pairwise_dist(x[:q], x, metric=sehip.METRIC_COSINE)
        med, mn = timeit(lambda: sehip.topk_rows(pd, args.k), args.reps)
        print("topk k=%d q=%d n=%d: median %.3f ms (min %.3f)  %.1f GB/s" % (args.k, q, n, med, mn, 4.0 * q * n / med / 1e6))
    else:
        B, D = 65536, 1000
        xx = torch.randn(B, D, device="cuda")
        E = torch.nn.functional.normalize(torch.randn(1000, D, device="cuda"), dim=-1)
        yy = torch.randint(0, 1000, (B,), device="cuda")
        med, mn = timeit(lambda: sehip.cosine_loss_forward(xx, yy, E), args.reps)
        print("loss fwd B=%d D=%d f32: median %.3f ms  %.1f GB/s" % (B, D, med, (B * D * 12.0) / med / 1e6))
        med, mn = timeit(lambda: sehip.cosine_loss_backward(xx, yy, E, grad_scale=1.0 / B), args.reps)
        print("loss bwd B=%d D=%d f32: median %.3f ms  %.1f GB/s" % (B, D, med, (B * D * 12.0) / med / 1e6))
        xb = xx.bfloat16()
        med, mn = timeit(lambda: sehip.cosine_loss_forward(xb, yy, E, want_xhat=False), args.reps)
        print("loss fwd (no xhat) bf16: median %.3f ms  %.1f GB/s" % (med, (B * D * 6.0) / med / 1e6))
        # DeViSE ranking loss (utils.py:103-122), forward + backward: the fused MFMA kernels against the same loss written in torch ops
        for C2, B3 in ((100, 128), (1000, 128), (1000, 1024)):
            Ed = torch.nn.functional.normalize(torch.randn(C2, C2, device="cuda"), dim=-1)
            yp = torch.nn.functional.normalize(torch.randn(B3, C2, device="cuda"), dim=-1).requires_grad_(True)
            yl = torch.randint(0, C2, (B3,), device="cuda")

            def hip_step():
                yp.grad = None
                sehip.devise_ranking_loss(yp, yl, Ed, 0.1).mean().backward()

            def torch_step():
                yp.grad = None
                true = (yp * Ed[yl]).sum(-1)
                (torch.relu(0.1 - true[:, None] + yp @ Ed.t()).sum(-1) - 0.1).mean().backward()
            mh, _ = timeit(hip_step, 20)
            mt, _ = timeit(torch_step, 20)
            print("devise fwd+bwd B=%d C=D=%d: HIP %.1f us, torch ops %.1f us" % (B3, C2, mh * 1e3, mt * 1e3))
        B2 = 128
        x2, y2, E2 = torch.randn(B2, 100, device="cuda"), torch.randint(0, 100, (B2,), device="cuda"), E[:100, :100].contiguous()
        med, mn = timeit(lambda: sehip.cosine_loss_forward(x2, y2, E2), 20)
        print("loss fwd B=128 D=100: median %.1f us" % (med * 1e3))


FP64_VECTOR_PEAK_TFLOPS = 78.6     # AMD's published FP64 vector rate of the MI355X (MI355X_MICROARCH.md lists no FP64 row)
HBM_MEASURED_TBS = 6.29            # MI355X_MICROARCH.md: float4 copy


def bench_pdist64(n, d, reps):
    """The float64 retrieval step (precision='float64') on one tile of an n x n x d all-pairs problem, tiled as
    evaluate_retrieval.ranking_tiles tiles it (whole when 16 B per pair fit a third of the free device memory, else
    DEFAULT_TILE_BYTES worth of rows), every leg on its own: se_pairwise_dist_f64 without and with the float32 image, se_rank_rows
    on the image, se_rank_refine_f64; the float32 step (se_pairwise_dist + se_rank_rows) of the same tile next to them.  One
    process; 3 warm-up calls per leg, then `reps` rounds in which the legs take turns, HIP events around each call: median
    (10th-90th percentile) in ms.  The tile's time is scaled to the whole problem by the number of tiles.
    Bounds of the distance leg: 2 q n d operations over AMD's published FP64 vector rate, and 12 q n bytes written over the measured
    copy bandwidth; the larger is the least time the hardware could take."""
    import evaluate_retrieval as er
    rng = np.random.default_rng(0)
    x64 = torch.from_numpy(rng.standard_normal((n, d))).cuda()
    x64.copy_(torch.from_numpy(er.host_normalize_f64(x64.cpu().numpy())))
    x32 = x64.float()
    sehip.normalize_rows_(x32)
    pair_bytes = 16
    rows = max(128, min(n, (er.DEFAULT_TILE_BYTES // (pair_bytes * n)) // 128 * 128))
    if pair_bytes * n * n <= torch.cuda.mem_get_info()[0] // 3:
        rows = n
    tiles = -(-n // rows)
    pd64, img = sehip.empty_rows(rows, n, torch.float64, "cuda"), sehip.empty_rows(rows, n, torch.float32, "cuda")
    rk, pd32 = sehip.empty_rows(rows, n, torch.int32, "cuda"), sehip.empty_rows(rows, n, torch.float32, "cuda")
    sehip.pairwise_dist_f64(x64[:rows], x64, out=pd64, img=img)
    sehip.rank_rows(img, out=rk)
    first = rk.clone()
    torch.cuda.synchronize()
    runs = int((torch.gather(img[:256], 1, first[:256, 1:].long()) == torch.gather(img[:256], 1, first[:256, :-1].long())).sum())

    def refine():                        # (every call repairs the same image ranking: the copy is timed on its own and subtracted)
        rk.copy_(first)
        sehip.rank_refine_f64_(pd64, img, rk)
    legs = [("se_pairwise_dist_f64, no image", lambda: sehip.pairwise_dist_f64(x64[:rows], x64, out=pd64, img=None)),
            ("se_pairwise_dist_f64 + image", lambda: sehip.pairwise_dist_f64(x64[:rows], x64, out=pd64, img=img)),
            ("se_rank_rows on the image", lambda: sehip.rank_rows(img, out=rk)),
            ("rank copy + se_rank_refine_f64", refine),
            ("rank copy alone", lambda: rk.copy_(first)),
            ("float32: se_pairwise_dist", lambda: sehip.pairwise_dist(x32[:rows], x32, out=pd32)),
            ("float32: se_rank_rows", lambda: sehip.rank_rows(pd32, out=rk))]
    res = windows([f for _, f in legs], reps, 1)
    print("pdist64 n=%d d=%d: tile of %d rows (%d tile%s; whole-problem times = tile x %d), %d rounds, ms per call: median (10th-90th percentile)"
          % (n, d, rows, tiles, "" if tiles == 1 else "s", tiles, reps))
    for (name, _), (med, lo, hi) in zip(legs, res):
        print("  %-34s %9.3f (%9.3f - %9.3f)   whole problem %9.2f" % (name, med / 1e3, lo / 1e3, hi / 1e3, med / 1e3 * tiles))
    t = {name: med / 1e3 for (name, _), (med, _, _) in zip(legs, res)}
    dist = t["se_pairwise_dist_f64 + image"]
    t_flop, t_mem = 2.0 * rows * n * d / (FP64_VECTOR_PEAK_TFLOPS * 1e9), 12.0 * rows * n / (HBM_MEASURED_TBS * 1e9)
    print("  distance + image: %.1f TFLOP/s = %.2f of the %.1f TFLOP/s FP64 vector rate; %.2f TB/s written; least time %.3f ms (%s bound) = %.2f of the leg"
          % (2.0 * rows * n * d / dist / 1e9, t_flop / dist, FP64_VECTOR_PEAK_TFLOPS, 12.0 * rows * n / dist / 1e9, max(t_flop, t_mem),
             "operation" if t_flop > t_mem else "memory", max(t_flop, t_mem) / dist))
    repair = t["rank copy + se_rank_refine_f64"] - t["rank copy alone"]
    print("  repair alone: %.3f ms = %.2f x the se_rank_rows leg; %.1f pairs of adjacent ranks per row share an image (first 256 rows)"
          % (repair, repair / t["se_rank_rows on the image"], runs / min(256, rows)))
    f64 = dist + t["se_rank_rows on the image"] + repair
    f32 = t["float32: se_pairwise_dist"] + t["float32: se_rank_rows"]
    print("  float64 step %.3f ms, float32 step %.3f ms: %.1f x" % (f64, f32, f64 / f32))


def bench_eigh(s, label):
    """se_eigh_f64 (two-sided block Jacobi) of the symmetric device matrix ``s`` against np.linalg.eigh of the same matrix on this
    host: wall-clock seconds of whole calls (the device figure includes the input copy, the workspace, every sweep's
    synchronisation, the sort and the gather), and the accuracy ratios against LAPACK."""
    import time
    C = s.shape[0]
    s_h = s.cpu().numpy()
    sehip.eigh(s[:65, :65].contiguous())                         # first-call costs (code object load) stay out of the timing
    torch.cuda.synchronize()
    runs, hosts = [], []
    for _ in range(2 if C > 4000 else 3):
        t0 = time.time()
        w, v, sweeps = sehip.eigh(s)
        torch.cuda.synchronize()
        runs.append(time.time() - t0)
    for _ in range(1 if C > 4000 else 3):
        t0 = time.time()
        lam = np.linalg.eigh(s_h)[0]
        hosts.append(time.time() - t0)
    scale = float(np.abs(lam).max())
    ne = C * 2.0 ** -52
    e_w = float(np.abs(w.cpu().numpy() - lam).max()) / scale / ne
    e_r = float((s @ v - v * w[None, :]).abs().max()) / scale / ne
    e_o = float((v.T @ v - torch.eye(C, dtype=torch.float64, device="cuda")).abs().max()) / ne
    print("eigh n=%d f64 (%s; block Jacobi, b = 32): %s s, %d sweeps; np.linalg.eigh on this host (%s threads): %s s; "
          "eigenvalues %.2f residual %.2f orthogonality %.2f (x n eps)"
          % (C, label, " / ".join("%.4f" % t for t in runs), sweeps, os.environ.get("OMP_NUM_THREADS", "default"),
             " / ".join("%.4f" % t for t in hosts), e_w, e_r, e_o))


def bench_classemb(reps):
    """se_class_pair_tables (both tables), se_cholesky_f64 and se_eigh_f64 of S = 1 - lcs_height (unit diagonal; the eigensolver
    next to np.linalg.eigh on this host), plus the full CLI on iNat (unitsphere; approx_sim with the device and the host eigensolver)."""
    import pickle
    import subprocess
    import tempfile
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_class_embedding_host import load_hierarchy
    for name in ("wordnet_dag", "inat2018"):
        h, classes = load_hierarchy(name)
        enc = h.pair_table_encoding(classes)
        ints = {k: torch.from_numpy(enc[k]).cuda() for k in ("off", "rank", "spl", "depth", "height")}
        C = len(classes)

        def tables():
            return sehip.class_pair_tables(ints["off"], ints["rank"], ints["spl"], ints["depth"], ints["height"], enc["max_anc"],
                                           enc["max_height"])
        med, mn = timeit(tables, reps)
        print("pair tables C=%d (%s, max %d ancestors): median %.3f ms (min %.3f)  %.1f GB/s written"
              % (C, name, enc["max_anc"], med, mn, 16.0 * C * C / med / 1e6))
        _, s, _ = sehip.class_pair_tables(ints["off"], ints["rank"], ints["spl"], ints["depth"], ints["height"], enc["max_anc"],
                                          enc["max_height"], diag_one=True, want_wup=False)
        a = torch.empty_like(s)

        def chol():
            a.copy_(s)
            sehip.cholesky_lower_(a)
        cp, _ = timeit(lambda: a.copy_(s), reps)
        med, mn = timeit(chol, reps)
        flop = C ** 3 / 3.0
        print("cholesky n=%d f64: median %.3f ms (min %.3f; %.3f ms of it the copy)  %.2f TFLOP/s"
              % (C, med, mn, cp, flop / ((med - cp) * 1e-3) / 1e12))
        bench_eigh(s, name)
        if name == "inat2018":
            bench_eigh(s[:512, :512].contiguous(), "inat2018, first 512 classes")
    # the sizes at which compute_class_embedding.main takes the device solver (EIGH_DEVICE_MAX_CLASSES)
    for name in ("cifar", "cub"):
        h, classes = load_hierarchy(name)
        _, s = h.similarity_tables_device(classes, diag_one=True, want_wup=False)
        bench_eigh(s, name)
    g = np.load(os.path.join(ROOT, "tests", "golden", "hierarchy_inat2018.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        hp, cl, out = os.path.join(tmp, "h.txt"), os.path.join(tmp, "c.txt"), os.path.join(tmp, "e.pickle")
        with open(hp, "w") as f:
            f.writelines("%s %s\n" % (p, c) for p, c in g["edges"].tolist())
        with open(cl, "w") as f:
            f.writelines("%s\n" % c for c in g["classes"].tolist())
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "semantic-embeddings_amd", "compute_class_embedding.py"), "--hierarchy", hp,
                            "--str_ids", "--class_list", cl, "--out", out], capture_output=True, text=True)
        wall = time.time() - t0
        print(r.stdout.strip())
        if r.returncode != 0:
            print(r.stderr[-2000:])
            raise SystemExit(r.returncode)
        with open(out, "rb") as f:
            e = pickle.load(f)["embedding"]
        print("compute_class_embedding.py iNat 2018 (8,142 classes, unitsphere): %.1f s wall (process start to exit), finite %s"
              % (wall, bool(np.isfinite(e).all())))
        # --method approx_sim --num_dim 128: the device eigensolver (forced: main() takes the host's eigh above
        # EIGH_DEVICE_MAX_CLASSES classes) against the command as shipped, which is the host eigendecomposition it took before
        cli = os.path.join(ROOT, "semantic-embeddings_amd", "compute_class_embedding.py")
        argv = ["--hierarchy", hp, "--str_ids", "--class_list", cl, "--out", out, "--method", "approx_sim", "--num_dim", "128"]
        forced = ("import sys; sys.path.insert(0, %r); import compute_class_embedding as cce; "
                  "cce.EIGH_DEVICE_MAX_CLASSES = 1 << 30; cce.main(sys.argv[1:])" % os.path.dirname(cli))
        for label, cmd in (("device eigensolver (forced)", [sys.executable, "-c", forced] + argv), ("host np.linalg.eigh (as shipped)", [sys.executable, cli] + argv)):
            t0 = time.time()
            r = subprocess.run(cmd, capture_output=True, text=True)
            wall = time.time() - t0
            print(r.stdout.strip())
            if r.returncode != 0:
                print(r.stderr[-2000:])
                raise SystemExit(r.returncode)
            print("compute_class_embedding.py iNat 2018 approx_sim --num_dim 128, %s: %.1f s wall" % (label, wall))


def bench_center(reps=200, steps=200):
    """Center loss (learn_center_loss.py): forward (se_sqdist_loss_fwd + the halving), input gradient (se_sqdist_loss_bwd) and
    centroid gradient (se_center_loss_centroid_grad) at D = 100, then one ResNet-110-fc training step (batch 128, fp32, HIP-graph
    replay) with the center-loss model next to the cosine-loss model, the two timed alternately."""
    from sehip._lib import call
    sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
    D = 100
    for B in (128, 1024):
        for C in (100, 1000, 8142):
            rng = np.random.default_rng(B + C)
            x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).cuda()
            c = torch.from_numpy(rng.uniform(-0.05, 0.05, (C, D)).astype(np.float32)).cuda()
            y = torch.from_numpy(rng.integers(0, C, B)).cuda()
            g = torch.full((B,), 0.1 / B, device="cuda")
            loss_i, dx, dc = torch.empty(B, device="cuda"), torch.empty(B, D, device="cuda"), torch.empty(C, D, device="cuda")

            def fwd():
                call("se_sqdist_loss_fwd", x, 0, D, y, c, D, B, D, C, loss_i, None, None)
                loss_i.mul_(0.5)

            def bwd_x():
                call("se_sqdist_loss_bwd", x, 0, D, y, c, D, g, 0.0, B, D, C, dx, 0, D)

            def bwd_c():
                call("se_center_loss_centroid_grad", x, 0, D, y, c, D, g, 0.0, B, D, C, dc, D)
            t = [timeit(f, reps)[0] * 1e3 for f in (fwd, bwd_x, bwd_c)]
            print("center loss B=%d D=%d C=%d: forward %.1f us, input gradient %.1f us, centroid gradient %.1f us "
                  "(median of %d; HIP events around one call)" % (B, D, C, t[0], t[1], t[2], reps))

    import utils
    import learn_center_loss as lcl
    from datasets import SyntheticGenerator
    from engine import Trainer
    E = np.load(os.path.join(ROOT, "tests", "golden", "embeddings.npz"))["cifar100_unitsphere"]
    Ed = torch.from_numpy(E.astype(np.float32)).cuda()
    trainers = {}
    for name in ("cosine", "center"):
        torch.manual_seed(0)
        model = utils.build_network(100, "resnet-110-fc", input_channels=3).cuda()
        l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
        if name == "cosine":
            tr = Trainer(model, {"l2norm": (utils.CosineEmbeddingLoss(Ed), 1.0)}, {"l2norm": [utils.nn_accuracy(Ed, dot_prod_sim=True)]},
                         lr=0.1, momentum=0.9, clipnorm=10.0, l2_of=l2_of, autocast_dtype=None, memory_format=torch.contiguous_format)
            transform, kw = None, {}
        else:
            model = lcl.CenterLossModel(model, 100).cuda()
            losses, metrics = lcl.build_losses(model, 0.1)
            tr = Trainer(model, losses, metrics, lr=0.1, momentum=0.9, clipnorm=10.0, l2_of=l2_of, autocast_dtype=None,
                         memory_format=torch.contiguous_format)
            transform, kw = lcl.transform_inputs, {"num_classes": 100}
        seq = SyntheticGenerator(100, 32, 3, 128 * 8, 128).train_sequence(128, shuffle=False, batch_transform=transform,
                                                                          batch_transform_kwargs=kw)
        batches = [seq[i] for i in range(8)]
        assert tr.enable_graphs(*batches[0]), name
        for i in range(10):
            tr.train_step(*batches[i % 8], {})
        trainers[name] = (tr, batches)
    ms = {name: [] for name in trainers}
    for _ in range(3):                       # alternate the two models: the same machine state for both
        for name, (tr, batches) in trainers.items():
            logs = {}
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                tr.train_step(*batches[i % 8], logs)
            b.record()
            torch.cuda.synchronize()
            assert np.isfinite(float(logs["loss"]))
            ms[name].append(a.elapsed_time(b) / steps)
    for name in trainers:
        step = float(np.median(ms[name]))
        print("ResNet-110-fc %s-loss step, batch 128, fp32, HIP-graph replay: %.3f ms/step (median of 3 x %d steps; %s), "
              "%.0f images/s" % (name, step, steps, ", ".join("%.3f" % v for v in ms[name]), 128 / step * 1e3))


def bench_xent(reps=60, batch=20, steps=200):
    """Softmax cross-entropy (learn_classifier.py): se_softmax_xent_fwd (loss, arg-max, top-k count, mean) + se_softmax_xent_bwd through
    the C ABI on preallocated buffers, the same through the autograd op, and the torch composition the sibling CLIs use
    (F.cross_entropy forward + backward, argmax, topk(5)), timed alternately in one process: per shape `reps` windows of `batch`
    back-to-back calls each (HIP events around a window), median / 10th / 90th percentile of the per-call time.  Bytes: the logits
    read by the forward and the backward pass and the gradient written, over the kernels' time, against the 6.29 TB/s a float4 copy
    reaches on MI355X (8 TB/s spec).  Then one ResNet-110 classifier training step (batch 128, fp32, HIP-graph replay) with the
    fused head next to the torch head."""
    import torch.nn.functional as F
    from sehip._lib import call
    HBM = 6.29e12

    for dtype, dcode, esz in ((torch.float32, 0, 4), (torch.bfloat16, 1, 2)):
        for B, C in ((128, 100), (128, 1000), (1024, 1000), (256, 8142)):
            for s in (0.0, 0.1):
                rng = np.random.default_rng(B + C)
                z = torch.from_numpy((rng.standard_normal((B, C)) * 3).astype(np.float32)).cuda().to(dtype)
                y = torch.from_numpy(rng.integers(0, C, B)).cuda()
                loss_i, aux, mean = torch.empty(B, device="cuda"), torch.empty(3 * B, device="cuda"), torch.empty(1, device="cuda")
                best, above = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
                dz = torch.empty(B, C, dtype=dtype, device="cuda")
                za, zt = z.clone().requires_grad_(True), z.clone().requires_grad_(True)

                def kernels():
                    call("se_softmax_xent_fwd", z, dcode, C, y, B, C, s, loss_i, aux, best, above, mean)
                    call("se_softmax_xent_bwd", z, dcode, C, y, aux, None, 1.0 / B, B, C, s, dz, dcode, C)

                def op():
                    za.grad = None
                    loss, _, _ = sehip.softmax_cross_entropy(za, y, s, reduction="mean", return_metrics=True)
                    loss.backward()

                def composition():
                    zt.grad = None
                    F.cross_entropy(zt.float(), y, label_smoothing=s).backward()
                    zt.argmax(dim=-1)
                    zt.topk(5, dim=-1)
                k, o, t = windows((kernels, op, composition), reps, batch)
                gbs = 3.0 * B * C * esz / (k[0] * 1e-6)
                print("xent B=%d C=%d %s s=%.1f: kernels %.1f us (%.1f-%.1f), autograd op %.1f us (%.1f-%.1f), torch composition %.1f us "
                      "(%.1f-%.1f): x%.2f / x%.2f; kernels move %.0f GB/s = %.1f%% of the HBM copy rate"
                      % (B, C, "bf16" if dcode else "f32", s, k[0], k[1], k[2], o[0], o[1], o[2], t[0], t[1], t[2], t[0] / k[0], t[0] / o[0],
                         gbs / 1e9, 100.0 * gbs / HBM))

    sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
    import utils
    import learn_classifier as lc
    from learn_image_embeddings import accuracy, categorical_crossentropy
    from datasets import SyntheticGenerator
    from engine import Trainer
    trainers = {}
    for name in ("fused", "torch"):
        torch.manual_seed(0)
        model = lc.build_classifier(100, "resnet-110", input_channels=3).cuda()
        l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
        if name == "fused":
            losses, metrics = lc.build_losses(0.0, [5])
        else:
            losses, metrics = {"prob": (categorical_crossentropy, 1.0)}, {"prob": [accuracy, utils.top_k_acc(5)]}
        tr = Trainer(model, losses, metrics, lr=0.1, momentum=0.9, clipnorm=10.0, l2_of=l2_of, autocast_dtype=None,
                     memory_format=torch.contiguous_format)
        seq = SyntheticGenerator(100, 32, 3, 128 * 8, 128).train_sequence(128, shuffle=False)
        batches = [seq[i] for i in range(8)]
        assert tr.enable_graphs(*batches[0]), name
        for i in range(10):
            tr.train_step(*batches[i % 8], {})
        trainers[name] = (tr, batches)
    ms = {name: [] for name in trainers}
    for _ in range(3):                       # alternate the two heads: the same machine state for both
        for name, (tr, batches) in trainers.items():
            logs = {}
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                tr.train_step(*batches[i % 8], logs)
            b.record()
            torch.cuda.synchronize()
            assert np.isfinite(float(logs["loss"]))
            ms[name].append(a.elapsed_time(b) / steps)
    for name in trainers:
        step = float(np.median(ms[name]))
        print("ResNet-110 classifier step (%s head: loss + acc + acc5), batch 128, fp32, HIP-graph replay: %.3f ms/step (median of 3 x %d "
              "steps; %s), %.0f images/s" % (name, step, steps, ", ".join("%.3f" % v for v in ms[name]), 128 / step * 1e3))


def _bench_tree(name, seed=0):
    """(ClassHierarchy, classes, note) of a hierarchy fixture under tests/golden -- 'cifar', 'ilsvrc' (the WordNet min-tree) or
    'inat2018' -- or, where the fixture is no tree, a seeded random tree with as many classes (the note says so)."""
    from class_hierarchy import ClassHierarchy
    golden = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(golden, "hierarchy_%s.npz" % name))
    if name == "cifar":
        id_type, classes = int, list(range(100))
    elif name == "ilsvrc":
        id_type, classes = str, np.load(os.path.join(golden, "imagenet_mintree_unitsphere.npz"))["ind2label"].tolist()
    else:
        id_type, classes = str, g["classes"].tolist()

    def build(edges):
        parents, children = {}, {}
        for p, c in edges:
            parents.setdefault(c, []).append(p)
            children.setdefault(p, []).append(c)
        return ClassHierarchy(parents, children)
    h = build([(id_type(p), id_type(c)) for p, c in g["edges"].tolist()])
    if h.is_tree():
        return h, [id_type(c) for c in classes], "the %s tree" % name
    rng = np.random.default_rng(seed)
    C, inner = len(classes), max(2, len(classes) // 3)
    edges = [(10 ** 6 + int(rng.integers(i // 2, i)), 10 ** 6 + i) for i in range(1, inner)]
    edges += [(10 ** 6 + int(rng.integers(0, inner)), c) for c in range(C)]
    return build(edges), list(range(C)), "a seeded random tree of %d classes (the %s fixture is not a tree)" % (C, name)


def bench_hxe(reps=40, batch=20):
    """Hierarchy-aware classifier losses: se_hxe_fwd + se_hxe_bwd and se_soft_xent_fwd + se_soft_xent_bwd (loss, arg-max, top-k count,
    mean, gradient) through the C ABI on preallocated buffers, next to a torch composition of each loss (HXE: exp(z - max) times a
    dense [C, nodes] membership matrix gives every node sum, then logs, a gather along the label's path and the weights; soft
    labels: log_softmax times the gathered table rows; both with backward, argmax and topk(5)) and to se_softmax_xent_fwd + _bwd at
    the same shape for scale.  All timed alternately in one process: per shape `reps` windows of `batch` back-to-back calls each (HIP
    events around a window) after 3 warm-up calls, median / 10th / 90th percentile of the per-call time."""
    import torch.nn.functional as F
    from sehip._lib import call
    print("hierarchy-aware losses, forward + backward, float32 logits; us per call, median (10th-90th percentile) of %d windows of %d "
          "calls, candidates alternating" % (reps, batch))
    for B, name in ((128, "cifar"), (128, "ilsvrc"), (256, "inat2018")):
        h, classes, note = _bench_tree(name)
        C = len(classes)
        enc_h = h.hxe_encoding(classes, alpha=0.1)
        enc = sehip.HxeEncoding(enc_h)
        t = enc.on(torch.device("cuda", torch.cuda.current_device()))
        table = torch.from_numpy(h.soft_label_table(classes, 10.0)).cuda()
        rng = np.random.default_rng(B + C)
        z = torch.from_numpy((rng.standard_normal((B, C)) * 3).astype(np.float32)).cuda()
        y = torch.from_numpy(rng.integers(0, C, B)).cuda()
        loss_i, mean = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
        aux_h, aux = torch.empty(call("se_hxe_aux_floats", B), device="cuda"), torch.empty(3 * B, device="cuda")
        best, above = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        dz = torch.empty(B, C, device="cuda")
        zt = z.clone().requires_grad_(True)
        # the composition's tables: one column of `member` per distinct range, the label's path as node indices (padded with the top)
        off, lo, hi, w = enc_h["path_off"], enc_h["lvl_lo"], enc_h["lvl_hi"], enc_h["lvl_w"]
        ranges = sorted(set(zip(lo.tolist(), hi.tolist())))
        col = {r: i for i, r in enumerate(ranges)}
        pos = enc_h["pos"].astype(np.int64)
        member = torch.from_numpy(np.stack([(pos >= a) & (pos < b) for a, b in ranges], axis=1).astype(np.float32)).cuda()
        hmax = int(enc_h["max_levels"])
        par = np.full((C, hmax), col[(0, C)], dtype=np.int64)
        wt = np.zeros((C, hmax), dtype=np.float32)
        for c in range(C):
            n = off[c + 1] - off[c]
            par[c, :n] = [col[r] for r in zip(lo[off[c]:off[c + 1]].tolist(), hi[off[c]:off[c + 1]].tolist())]
            wt[c, :n] = w[off[c]:off[c + 1]]
        par, wt = torch.from_numpy(par).cuda(), torch.from_numpy(wt).cuda()

        def hxe_kernels():
            call("se_hxe_fwd", z, 0, C, y, t["pos"], t["path_off"], enc.host["path_off"], t["lvl_lo"], t["lvl_hi"], t["lvl_w"], B, C, loss_i,
                 aux_h, best, above, mean)
            call("se_hxe_bwd", z, 0, C, y, t["pos"], t["path_off"], enc.host["path_off"], t["lvl_lo"], t["lvl_hi"], t["lvl_w"], aux_h, None,
                 1.0 / B, B, C, dz, 0, C)

        def soft_kernels():
            call("se_soft_xent_fwd", z, 0, C, y, table, C, B, C, loss_i, aux, best, above, mean)
            call("se_soft_xent_bwd", z, 0, C, y, table, C, aux, None, 1.0 / B, B, C, dz, 0, C)

        def xent_kernels():
            call("se_softmax_xent_fwd", z, 0, C, y, B, C, 0.0, loss_i, aux, best, above, mean)
            call("se_softmax_xent_bwd", z, 0, C, y, aux, None, 1.0 / B, B, C, 0.0, dz, 0, C)

        def hxe_composition():
            zt.grad = None
            x = zt - zt.max(dim=1, keepdim=True).values
            up = torch.log(x.exp() @ member).gather(1, par[y])
            down = torch.cat([x.gather(1, y[:, None]), up[:, :-1]], dim=1)
            (wt[y] * (up - down)).sum(dim=1).mean().backward()
            zt.argmax(dim=-1)
            zt.topk(5, dim=-1)

        def soft_composition():
            zt.grad = None
            (-(table[y] * F.log_softmax(zt, dim=-1)).sum(dim=1)).mean().backward()
            zt.argmax(dim=-1)
            zt.topk(5, dim=-1)

        # the composition computes the kernel's loss (checked once, so that the two sides time the same thing)
        hxe_kernels()
        x = z - z.max(dim=1, keepdim=True).values
        up = torch.log(x.exp() @ member).gather(1, par[y])
        want = float((wt[y] * (up - torch.cat([x.gather(1, y[:, None]), up[:, :-1]], dim=1))).sum(dim=1).mean())
        assert abs(float(mean) - want) <= 1e-4 * max(1.0, abs(want)), (float(mean), want)
        hk, sk, xk, hc_, sc = windows((hxe_kernels, soft_kernels, xent_kernels, hxe_composition, soft_composition), reps, batch)
        print("B=%d C=%d on %s (%d levels at most, %d distinct ranges):" % (B, C, note, hmax, len(ranges)))
        print("  hxe:         kernels %.1f us (%.1f-%.1f), torch composition %.1f us (%.1f-%.1f): %s by x%.2f"
              % (hk[0], hk[1], hk[2], hc_[0], hc_[1], hc_[2], "kernels win" if hk[0] < hc_[0] else "composition wins",
                 max(hk[0], hc_[0]) / min(hk[0], hc_[0])))
        print("  soft labels: kernels %.1f us (%.1f-%.1f), torch composition %.1f us (%.1f-%.1f): %s by x%.2f"
              % (sk[0], sk[1], sk[2], sc[0], sc[1], sc[2], "kernels win" if sk[0] < sc[0] else "composition wins",
                 max(sk[0], sc[0]) / min(sk[0], sc[0])))
        print("  for scale, se_softmax_xent_fwd + _bwd: %.1f us (%.1f-%.1f); hxe takes x%.2f of it, soft labels x%.2f"
              % (xk[0], xk[1], xk[2], hk[0] / xk[0], sk[0] / xk[0]), flush=True)


def bench_crm(reps=12, top=20):
    """CRM decoding (mistakes.crm_classification), top = 20 classes of smallest expected LCS height per row of probabilities, three
    ways on the same device inputs and preallocated outputs where the interface allows: se_tree_risk_topk (float64 risks from one
    prefix sum per row); the dense composition on the existing kernels, se_pairwise_dist(P, -H, cosine) in slabs of
    mistakes.DENSE_TILE_ROWS rows + se_topk_rows (float32 chain); a torch composition, P.double() @ H.T then topk(largest=False)
    (float64).  Timed alternately in one process: per shape `reps` windows of `batch` back-to-back calls (HIP events around a
    window) after 3 warm-up calls, median / 10th / 90th percentile of the per-call time.  The agreement of the three class lists is
    printed, not asserted: the float32 chain and another float64 summation order may order near-ties differently."""
    import mistakes
    from sehip._lib import call
    print("CRM decoding, top = %d; ms per call, median (10th-90th percentile) of %d windows, candidates alternating" % (top, reps))
    for N, name, batch in ((10000, "cifar", 10), (50000, "ilsvrc", 3), (24426, "inat2018", 2)):
        h, classes, note = _bench_tree(name)
        C = len(classes)
        enc_h = h.tree_risk_encoding(classes)
        enc = sehip.TreeRiskEncoding(enc_h)
        t = enc.on(torch.device("cuda", torch.cuda.current_device()))
        H = h.height_table(classes)
        negH, H64 = -H.to(torch.float32), H.to(torch.float64)
        rng = np.random.default_rng(N + C)
        P = torch.softmax(torch.from_numpy((3.0 * rng.standard_normal((N, C))).astype(np.float32)).cuda(), dim=-1)
        cls, rt = torch.empty((N, top), dtype=torch.int32, device="cuda"), torch.empty((N, top), dtype=torch.float64, device="cuda")
        rows = mistakes.DENSE_TILE_ROWS
        slab = torch.empty((min(rows, N), C), dtype=torch.float32, device="cuda")
        dcls, dd = torch.empty((N, top), dtype=torch.int32, device="cuda"), torch.empty((N, top), dtype=torch.float32, device="cuda")
        kept = {}

        def tree_kernel():
            call("se_tree_risk_topk", P, C, t["pos"], t["path_off"], t["lvl_lo"], t["lvl_hi"], t["lvl_h"], enc.nnz, t["own_h"], N, C, top,
                 cls, rt, None, 0)

        def dense_kernels():
            for r0 in range(0, N, rows):
                n = min(rows, N - r0)
                call("se_pairwise_dist", P[r0:r0 + n], C, negH, C, None, None, n, C, C, sehip.METRIC_COSINE, None, 0, slab, C)
                call("se_topk_rows", slab, C, n, C, 0, top, dd[r0:r0 + n], dcls[r0:r0 + n])

        def torch_composition():
            kept["torch"] = (P.double() @ H64.T).topk(top, dim=1, largest=False).indices

        tk, dk, tc_ = windows((tree_kernel, dense_kernels, torch_composition), reps, batch)
        same_d = float((cls == dcls).all(dim=1).float().mean())
        same_t = float((cls.long() == kept["torch"]).all(dim=1).float().mean())
        ms = lambda v: (v[0] / 1e3, v[1] / 1e3, v[2] / 1e3)
        print("N=%d C=%d on %s (%d levels at most):" % (N, C, note, enc_h["max_levels"]))
        print("  se_tree_risk_topk          %9.3f ms (%.3f-%.3f)   4 N C bytes of input over this time: %.2f TB/s" % (ms(tk) + (4.0 * N * C / tk[0] / 1e6,)))
        print("  dense on existing kernels  %9.3f ms (%.3f-%.3f)   x%.2f of the tree kernel" % (ms(dk) + (dk[0] / tk[0],)))
        print("  torch float64 composition  %9.3f ms (%.3f-%.3f)   x%.2f of the tree kernel" % (ms(tc_) + (tc_[0] / tk[0],)))
        print("  rows whose %d classes agree with the tree kernel's: dense %.4f, torch %.4f" % (top, same_d, same_t), flush=True)


def bench_labelembed(reps=60, batch=20, steps=200):
    """Label-embedding loss (learn_labelembedding.py) on the learned [C, C] table: se_labelembed_table_loss_fwd / _bwd (loss, both logit
    gradients and the fixed-order table gradient) next to the composition they replace -- the Embedding gather of the table rows,
    se_labelembed_loss_fwd / _bwd on the gathered rows and torch's embedding backward into a dense [C, C] gradient (atomic adds) -- both
    as calls on preallocated buffers and through autograd (forward, mean, backward), timed alternately in one process: per shape `reps`
    windows of `batch` back-to-back calls each (HIP events around a window), median / 10th / 90th percentile of the per-call time.
    Every second row has out2 right about its class (mask = 1), so half of the rows contribute to the table gradient.  Then one
    ResNet-110-fc training step (batch 128, fp32, HIP-graph replay) of the label-embedding model next to the classifier's."""
    import torch.nn.functional as F
    from sehip._lib import call

    for B, C in ((128, 100), (128, 1000), (256, 8142)):
        rng = np.random.default_rng(B + C)
        o1, o2 = (torch.from_numpy((rng.standard_normal((B, C)) * 2).astype(np.float32)).cuda() for _ in range(2))
        y = torch.from_numpy(rng.integers(0, C, B)).cuda()
        o2[torch.arange(0, B, 2, device="cuda"), y[::2]] += 7.0
        table = torch.eye(C, device="cuda") + 0.1 * torch.randn(C, C, device="cuda")
        g = torch.full((B,), 1.0 / B, device="cuda")
        loss_i, aux = torch.empty(B, device="cuda"), torch.empty(call("se_labelembed_aux_floats", B), device="cuda")
        loss_c, aux_c = torch.empty_like(loss_i), torch.empty_like(aux)
        d1, d2, dtar, dtab = [torch.empty(B, C, device="cuda") for _ in range(3)] + [torch.empty(C, C, device="cuda")]
        res = {}

        def kernels():
            call("se_labelembed_table_loss_fwd", o1, C, o2, C, table, C, y, B, C, 2.0, 0.9, 0.5, loss_i, aux)
            call("se_labelembed_table_loss_bwd", o1, C, o2, C, table, C, y, g, 0.0, B, C, 2.0, 0.9, 0.5, aux, d1, C, d2, C, dtab, C)

        def composed_kernels():
            tar = F.embedding(y, table)
            call("se_labelembed_loss_fwd", o1, C, o2, C, tar, C, y, B, C, 2.0, 0.9, 0.5, loss_c, aux_c)
            call("se_labelembed_loss_bwd", o1, C, o2, C, tar, C, y, g, 0.0, B, C, 2.0, 0.9, 0.5, aux_c, d1, C, d2, C, dtar, C)
            res["dtab"] = torch.ops.aten.embedding_dense_backward(dtar, y, C, -1, False)

        a1, a2, ta = o1.clone().requires_grad_(True), o2.clone().requires_grad_(True), table.clone().requires_grad_(True)
        c1, c2, tc = o1.clone().requires_grad_(True), o2.clone().requires_grad_(True), table.clone().requires_grad_(True)

        def op():
            a1.grad = a2.grad = ta.grad = None
            sehip.labelembed_table_loss(a1, a2, ta, y).mean().backward()

        def composed_op():
            c1.grad = c2.grad = tc.grad = None
            sehip.labelembed_loss(c1, c2, F.embedding(y, tc), y).mean().backward()
        k, ck, o, co = windows((kernels, composed_kernels, op, composed_op), reps, batch)
        parts = [timeit(f, reps)[0] * 1e3 for f in (
            lambda: call("se_labelembed_table_loss_fwd", o1, C, o2, C, table, C, y, B, C, 2.0, 0.9, 0.5, loss_i, aux),
            lambda: call("se_labelembed_table_loss_bwd", o1, C, o2, C, table, C, y, g, 0.0, B, C, 2.0, 0.9, 0.5, aux, d1, C, d2, C, None, 0),
            lambda: call("se_labelembed_table_loss_bwd", o1, C, o2, C, table, C, y, g, 0.0, B, C, 2.0, 0.9, 0.5, aux, None, 0, None, 0, dtab, C))]
        print("labelembed B=%d C=%d, one call each (median of %d; HIP events around one call): forward %.1f us, logit gradients %.1f us, "
              "table gradient %.1f us (writes %.1f MB)" % (B, C, reps, parts[0], parts[1], parts[2], 4e-6 * C * C))
        same = torch.equal(loss_i.view(torch.int32), loss_c.view(torch.int32))
        diff = float((dtab - res["dtab"]).abs().max())
        print("labelembed B=%d C=%d: table kernels %.1f us (%.1f-%.1f) vs gather + loss kernels + embedding backward %.1f us (%.1f-%.1f): "
              "x%.2f; autograd op %.1f us (%.1f-%.1f) vs composed op %.1f us (%.1f-%.1f): x%.2f; loss bits equal %s, table gradients "
              "differ by at most %.2e" % (B, C, k[0], k[1], k[2], ck[0], ck[1], ck[2], ck[0] / k[0], o[0], o[1], o[2], co[0], co[1], co[2],
                                          co[0] / o[0], same, diff))

    sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
    import utils
    import learn_classifier as lc
    import learn_labelembedding as ll
    from datasets import SyntheticGenerator
    from engine import Trainer
    trainers = {}
    for name in ("classifier", "labelembed"):
        torch.manual_seed(0)
        if name == "classifier":
            model = lc.build_classifier(100, "resnet-110-fc", input_channels=3).cuda()
            l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
            losses, metrics = lc.build_losses(0.0)
            transform, kw = None, {}
        else:
            base = utils.build_network(100, "resnet-110-fc", input_channels=3).cuda()
            l2_of = {id(p): base.regularizer for p in base.regularized_parameters()}
            model = ll.labelembed_model(base, 100).cuda()
            losses, metrics = ll.build_losses(model)
            transform, kw = ll.transform_trainer_inputs, {"num_classes": 100}
        tr = Trainer(model, losses, metrics, lr=0.1, momentum=0.9, clipnorm=10.0, l2_of=l2_of, autocast_dtype=None,
                     memory_format=torch.contiguous_format)
        seq = SyntheticGenerator(100, 32, 3, 128 * 8, 128).train_sequence(128, shuffle=False, batch_transform=transform,
                                                                          batch_transform_kwargs=kw)
        batches = [seq[i] for i in range(8)]
        assert tr.enable_graphs(*batches[0]), name
        for i in range(10):
            tr.train_step(*batches[i % 8], {})
        trainers[name] = (tr, batches)
    ms = {name: [] for name in trainers}
    for _ in range(3):                       # alternate the two models: the same machine state for both
        for name, (tr, batches) in trainers.items():
            logs = {}
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                tr.train_step(*batches[i % 8], logs)
            b.record()
            torch.cuda.synchronize()
            assert np.isfinite(float(logs["loss"]))
            ms[name].append(a.elapsed_time(b) / steps)
    for name in trainers:
        step = float(np.median(ms[name]))
        print("ResNet-110-fc %s step, batch 128, 100 classes, fp32, HIP-graph replay: %.3f ms/step (median of 3 x %d steps; %s), "
              "%.0f images/s" % (name, step, steps, ", ".join("%.3f" % v for v in ms[name]), 128 / step * 1e3))


def bench_head(reps=40, batch=20):
    """Embedding heads (learn_image_embeddings.py --loss inv_corr / mse): se_embed_head_fwd -- loss and the nearest-class metric's counts
    in one launch -- next to the sequence it replaces for the same outputs, se_cosine_loss_fwd (or se_sqdist_loss_fwd) plus 1, 2 and 3
    se_nn_accuracy launches (no --top_k_acc, one k, two k), as calls on preallocated buffers, timed alternately in one process: per
    shape `reps` windows of `batch` back-to-back calls each (HIP events around a window), median / 10th / 90th percentile of the
    per-call time.  The head is timed with and without the xhat output (the training loop keeps it for feature dumps; the fused
    contraction does not read it back).  The sequence's xhat always goes through memory: the metric reads it."""
    from sehip._lib import call

    print("embedding heads: one se_embed_head_fwd vs loss launch + n se_nn_accuracy launches; us per call, median (10th-90th percentile) of "
          "%d windows of %d calls, candidates alternating" % (reps, batch))
    for mode, mname in ((0, "cosine"), (1, "sqdist")):
        for B, D, C in ((128, 100, 100), (128, 200, 200), (128, 555, 555), (128, 1000, 1000), (256, 1000, 1000)):
            for dtype, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
                rng = np.random.default_rng(B + D + C)
                x = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).cuda().to(dtype)
                emb = torch.from_numpy(rng.standard_normal((C, D)).astype(np.float32)).cuda()
                sehip.normalize_rows_(emb)
                y = torch.from_numpy(rng.integers(0, C, B)).cuda()
                code = 0 if dtype == torch.float32 else 1
                f = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
                i = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
                xhat, loss_i, nb, nw = f(B, D), f(B), i(B), i(B)
                xhat_s, loss_s, accs = f(B, D), f(B), [f(B) for _ in range(3)]
                need = call("se_embed_head_workspace_bytes", mode, B, D, C)
                ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device="cuda")
                need_s = call("se_nn_accuracy_workspace_bytes", B, C)
                ws_s = torch.empty(max(need_s // 8, 1), dtype=torch.int64, device="cuda")

                def head(with_xhat):
                    call("se_embed_head_fwd", mode, x, code, D, y, emb, D, B, D, C, xhat if with_xhat else None, D, None, loss_i, None, None,
                         nb, nw, None, None, C, ws, need)

                def sequence(n):
                    if mode == 0:
                        call("se_cosine_loss_fwd", x, code, D, y, emb, D, B, D, C, xhat_s, D, None, loss_s, None)
                        yp = xhat_s
                    else:
                        call("se_sqdist_loss_fwd", x, code, D, y, emb, D, B, D, C, loss_s, None, None)
                        yp = x if dtype == torch.float32 else x.float()       # the Python path widens bf16 features before the metric
                    for j in range(n):
                        call("se_nn_accuracy", yp, D, y, emb, D, B, D, C, 1 - mode, (1, 5, 10)[j], accs[j], None, C, None, ws_s, need_s)

                fns = [lambda: head(True), lambda: head(False)] + [lambda n=n: sequence(n) for n in (1, 2, 3)]
                if mode == 1:
                    fns = fns[:1] + fns[2:]
                t = windows(fns, reps, batch)
                same = torch.equal(loss_i.view(torch.int32), loss_s.view(torch.int32))
                for j, k in enumerate((1, 5, 10)):
                    same = same and torch.equal(((nw >= 1) & (nb < k)).float(), accs[j])
                if mode == 0:
                    same = same and torch.equal(xhat.view(torch.int32), xhat_s.view(torch.int32))
                names = (["head", "head without xhat"] if mode == 0 else ["head"]) + ["loss + 1 metric", "loss + 2 metrics", "loss + 3 metrics"]
                ref = t[0][0]
                print("head %-6s %4d x %4d x %4d %-4s: " % (mname, B, D, C, dname) +
                      "; ".join("%s %.1f (%.1f-%.1f)" % (nm, v[0], v[1], v[2]) for nm, v in zip(names, t)) +
                      "; head vs 1 / 2 / 3 metrics: x%.2f x%.2f x%.2f; bits equal %s" % (t[-3][0] / ref, t[-2][0] / ref, t[-1][0] / ref, same))


def bench_joint(reps=40, batch=10):
    """Joint head of `--cls_weight` (learn_image_embeddings.py with SE_JOINT_HEAD=1), forward + backward of loss and metrics for one
    batch, three sequences timed alternately in one process (per shape `reps` windows of `batch` back-to-back steps, HIP events
    around a window; median / 10th / 90th percentile of the per-step time):
      composition  today's default: utils.inv_correlation(emb[y], p) + nn.functional.cross_entropy through autograd, and per metric
                   one utils.nn_accuracy (class table) or arg-max / top-k (one-hot) on the first output and arg-max / top-k on the
                   logits; with 1 and with 3 metrics per output (no --top_k_acc, two k)
      separate     se_joint_head_fwd without logits + se_softmax_xent_fwd, se_joint_head_bwd without logits + se_softmax_xent_bwd:
                   four launches on preallocated buffers
      joint        one se_joint_head_fwd + one se_joint_head_bwd on the same buffers
    The two kernel sequences deliver the counts every k is read from, so the number of metrics does not change them."""
    import utils
    from sehip._lib import call

    print("joint head, forward + backward: torch composition (1 / 3 metrics per output) vs separate launches vs one joint launch; us per "
          "step, median (10th-90th percentile) of %d windows of %d steps, candidates alternating" % (reps, batch))
    for B, D, C, onehot in ((128, 100, 100, False), (96, 200, 200, False), (128, 555, 555, False), (128, 1000, 1000, False),
                            (128, 8142, 8142, True)):
        rng = np.random.default_rng(B + D + C)
        p = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).cuda()
        p = torch.softmax(p, -1) if onehot else torch.nn.functional.normalize(p, dim=-1)
        z = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32) * 3).cuda()
        y = torch.from_numpy(rng.integers(0, C, B)).cuda()
        emb = None
        if not onehot:
            emb = torch.from_numpy(rng.standard_normal((C, D)).astype(np.float32)).cuda()
            sehip.normalize_rows_(emb)
        table = torch.eye(C, device="cuda") if onehot else emb
        metric = 1 if onehot else 0
        f = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        i = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
        out = {n: dict(el=f(B), nb=i(B), nw=i(B), pb=i(B), pa=i(B), cl=f(B), aux=f(3 * B), zb=i(B), za=i(B), dp=f(B, D), dz=f(B, C)) for n in ("sep", "joint")}
        need = call("se_joint_head_workspace_bytes", metric, B, D, C)
        ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device="cuda")
        lde = D if emb is not None else 0
        wc = 0.1 / B

        def kernels(o, joint):
            zz = z if joint else None
            call("se_joint_head_fwd", p, D, y, emb, lde, B, D, C, metric, o["el"], o["nb"], o["nw"], o["pb"], o["pa"], None, C,
                 zz, 0, C, o["cl"] if joint else None, o["aux"] if joint else None, o["zb"], o["za"], ws, need)
            if not joint:
                call("se_softmax_xent_fwd", z, 0, C, y, B, C, 0.0, o["cl"], o["aux"], o["zb"], o["za"], None)
            call("se_joint_head_bwd", y, emb, lde, B, D, C, None, 1.0 / B, o["dp"], D, zz, 0, C, o["aux"] if joint else None, None, wc,
                 o["dz"] if joint else None, 0, C)
            if not joint:
                call("se_softmax_xent_bwd", z, 0, C, y, o["aux"], None, wc, B, C, 0.0, o["dz"], 0, C)

        first = [utils.nn_accuracy(emb, dot_prod_sim=True, k=k) for k in (1, 5, 10)] if not onehot else \
            [lambda yt, o: (o.argmax(-1) == yt).float(), utils.top_k_acc(5), utils.top_k_acc(10)]
        second = [lambda yt, o: (o.argmax(-1) == yt).float(), utils.top_k_acc(5), utils.top_k_acc(10)]

        def composition(n):
            pp, zz = p.detach().requires_grad_(True), z.detach().requires_grad_(True)
            total = utils.inv_correlation(table[y], pp).mean() + 0.1 * torch.nn.functional.cross_entropy(zz, y, reduction="none").mean()
            with torch.no_grad():
                for m in first[:n]:
                    m(y, pp.detach()).sum()
                for m in second[:n]:
                    m(y, zz.detach()).sum()
            total.backward()
            return pp.grad, zz.grad

        t = windows([lambda: composition(1), lambda: composition(3), lambda: kernels(out["sep"], False), lambda: kernels(out["joint"], True)], reps, batch)
        same = all(torch.equal(out["sep"][k].view(torch.int32), out["joint"][k].view(torch.int32))
                   for k in ("el", "cl", "aux", "zb", "za", "dp", "dz", "pb") + (("pa",) if onehot else ("nb", "nw")))
        names = ["composition, 1 metric", "composition, 3 metrics", "separate launches", "joint launch"]
        print("joint %4d x %4d x %4d %-7s: " % (B, D, C, "one-hot" if onehot else "table") +
              "; ".join("%s %.1f (%.1f-%.1f)" % (nm, v[0], v[1], v[2]) for nm, v in zip(names, t)) +
              "; separate / joint: x%.2f; composition (1 / 3 metrics) / joint: x%.2f x%.2f; separate and joint bits equal %s" %
              (t[2][0] / t[3][0], t[0][0] / t[3][0], t[1][0] / t[3][0], same))


def bench_image(B=128, reps=20, stored=256):
    """Composing a batch of a file-based dataset (datasets/files.py): the host part -- drawing the augmentation parameters, building
    the resampling tables (sehip.resample_tables) and uploading them in one copy, host clock around work that ends in a device
    synchronise -- and the kernel, se_image_batch, HIP events around one launch on tables that are already on the device, `reps`
    different batches each, medians.  Bytes: the source pixels inside the row / column span each sample's tables reach + the tables +
    the batch written, over the kernel time, against the 6.29 TB/s a float4 copy reaches on MI355X.  The store holds `stored` images of
    uniform noise, float32 and bfloat16 batches.  Last, the ResNet-50 training step of the same batch size (bench.py's configuration:
    224 x 224, 200 classes, bf16 autocast, channels_last) in the same process: the loader keeps up when host + kernel stay below it."""
    import argparse as ap
    import time
    from datasets.files import DEFAULT_ERASE_PARAMS, FileDatasetGenerator, pack_batch_tables
    HBM = 6.29e12
    rng = np.random.default_rng(0)
    cases = (("CUB preset: 375 x 500 -> shorter side 512, crop 448 x 448", lambda n: np.tile([[375, 500]], (n, 1)),
              dict(cropsize=(448, 448), default_target_size=512, randzoom_range=None)),
             ("NAB preset: about 768 x 1024 -> random zoom 256-480, crop 224 x 224",
              lambda n: np.stack((rng.integers(700, 840, n), rng.integers(950, 1100, n)), axis=1),
              dict(cropsize=(224, 224), default_target_size=256, randzoom_range=(256, 480))))
    worst = 0.0
    for title, make_sizes, kw in cases:
        gen = FileDatasetGenerator(".", randerase_prob=0.5, randerase_params=DEFAULT_ERASE_PARAMS, **kw)
        gen._compute_stats([125.30513277, 129.66606421, 118.45121113], [57.0045467, 56.70059436, 68.44430446])
        sizes = make_sizes(stored).astype(np.int32)
        nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
        offsets = np.concatenate(([0], np.cumsum(nbytes)[:-1]))
        arena = torch.randint(0, 256, (int(nbytes.sum()),), dtype=torch.uint8, device="cuda")
        mean, std = gen._device_stats()
        crop = (kw["cropsize"][1], kw["cropsize"][0])
        host_ms, kern_ms, moved, taps = [], {torch.float32: [], torch.bfloat16: []}, [], None
        draw = np.random.default_rng(1)
        for it in range(reps + 2):
            idx = draw.choice(stored, B, replace=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            params = gen.draw_params(sizes[idx], True, True, draw)
            buf, views = pack_batch_tables(offsets[idx], sizes[idx], params, crop)
            dbuf = torch.from_numpy(buf).cuda()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            t = {name: (dbuf[a:b].view(torch.int64) if name == "src_off" else dbuf[a:b].view(shape)) for name, (a, b, shape) in views.items()}
            xmap, ymap = (buf[views[k][0]:views[k][1]].reshape(views[k][2]) for k in ("xmap", "ymap"))
            span = lambda m: (m[:, :, 1] + m[:, :, 2]).max(axis=1) - m[:, :, 1].min(axis=1)
            src_bytes = int((span(xmap).astype(np.int64) * span(ymap) * 3).sum())
            taps = (views["xk"][2][2], views["yk"][2][2])
            for dtype, esz in ((torch.float32, 4), (torch.bfloat16, 2)):
                out = torch.empty((B,) + crop + (3,), dtype=dtype, device="cuda")
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                sehip.image_batch(arena, t["src_off"], t["src_hw"], t["xmap"], t["xk"], t["ymap"], t["yk"], t["erase"], t["seed"], mean, std,
                                  dtype=dtype, out=out)
                b.record()
                torch.cuda.synchronize()
                if it >= 2:                                   # two warm-up batches
                    kern_ms[dtype].append(a.elapsed_time(b))
                    if dtype == torch.float32:
                        moved.append(src_bytes + buf.nbytes + out.numel() * esz)
            if it >= 2:
                host_ms.append((t1 - t0) * 1e3)
        h, k32, k16 = (float(np.median(v)) for v in (host_ms, kern_ms[torch.float32], kern_ms[torch.bfloat16]))
        gbs = float(np.median(moved)) / (k32 * 1e-3)
        worst = max(worst, h + k32)
        print("image batch, B = %d, %s (taps %d x %d): kernel %.3f ms f32 (%.3f-%.3f) / %.3f ms bf16; host (draw + tables + upload of "
              "%.2f MB) %.3f ms (%.3f-%.3f); host + kernel %.3f ms = %.0f images/s; f32 kernel moves %.1f MB = %.0f GB/s = %.1f%% of the "
              "HBM copy rate" % (B, title, taps[0], taps[1], k32, min(kern_ms[torch.float32]), max(kern_ms[torch.float32]), k16,
                                 buf.nbytes / 1e6, h, min(host_ms), max(host_ms), h + k32, B / (h + k32) * 1e3, np.median(moved) / 1e6,
                                 gbs / 1e9, 100.0 * gbs / HBM), flush=True)
        del arena
    sys.path.insert(0, ROOT)
    import train_bench
    r = train_bench.bench_train(ap.Namespace(arch="resnet-50", batch=B, steps=30, warmup=5, workload="train", full=False), 0, 1)
    print("ResNet-50 training step, 224 x 224, 200 classes, batch %d, %s: %.2f ms/step = %.0f images/s; slowest batch composition "
          "(host + kernel) %.2f ms: the loader %s" % (B, r["dtype"], r["ms_per_step"], r["value"], worst,
                                                      "keeps up with the network" if worst < r["ms_per_step"] else "DOES NOT keep up: it sets images/s"))


def bench_stream(images=2048, B=128, threads=16, classes=8):
    """The streamed tier of the file-based datasets (datasets/files.py) at the ILSVRC preset -- shorter side 256 .. 480, crop 224 x 224,
    batch `B`, `threads` decode threads -- on `images` JPEGs of 500 x 375 (quality 90; smooth content plus noise from a fixed seed)
    written to a temporary directory in ILSVRC's layout.  Whole epochs of train_sequence(B) (host clock, device synchronised at the
    end, the second epoch of each generator: the files are in the page cache) with look-ahead 0, 2 and 4, next to the resident tier on
    the same images.  Then one epoch of un-announced batches taken apart, a device synchronise after every part, medians per batch:
    decode (the pool), packing into the pinned slot, upload, and draw + tables + their upload + se_image_batch."""
    import io
    import tempfile
    import time
    from concurrent.futures import ThreadPoolExecutor
    import PIL.Image
    from datasets import ILSVRCGenerator
    from datasets.files import compose_on_device

    def jpeg(k):
        rng = np.random.default_rng(k)
        yy, xx = np.mgrid[0:375, 0:500].astype(np.float64)
        img = np.stack([128 + 100 * np.sin(xx / (9 + 5 * c) + rng.uniform(0, 6)) * np.cos(yy / (11 + 3 * c) + rng.uniform(0, 6)) for c in range(3)], axis=-1)
        buf = io.BytesIO()
        PIL.Image.fromarray(np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90)
        return buf.getvalue()

    def epoch(gen):
        seq = gen.train_sequence(B, shuffle=True)
        rates = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(len(seq)):
                seq[b]
            torch.cuda.synchronize()
            rates.append(len(seq) * B / (time.perf_counter() - t0))
            seq.on_epoch_end()
        return rates

    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=threads) as pool:
            blobs = list(pool.map(jpeg, range(images)))
        for k, blob in enumerate(blobs):
            d = os.path.join(root, "ILSVRC2012_img_train", "n%08d" % (k % classes))
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "n%08d_%d.JPEG" % (k % classes, k)), "wb") as f:
                f.write(blob)
        os.makedirs(os.path.join(root, "ILSVRC2012_img_val"))
        print("stream: wrote %d JPEGs of 500 x 375, %.1f MB (%.0f KB each), in %.1f s; %d decode threads, batch %d, ILSVRC preset"
              % (images, sum(map(len, blobs)) / 1e6, np.mean([len(b) for b in blobs]) / 1e3, time.perf_counter() - t0, threads, B), flush=True)
        del blobs
        for ahead in (0, 2, 4):
            gen = ILSVRCGenerator(root, store="stream", prefetch_batches=ahead, decode_threads=threads, dtype=torch.bfloat16)
            first, second = epoch(gen)
            print("streamed, look-ahead %d (ring of %d slots): %.0f images/s (first epoch %.0f)" % (ahead, ahead + 2, second, first), flush=True)
        gen = ILSVRCGenerator(root, store="resident", dtype=torch.bfloat16)
        t0 = time.perf_counter()
        st = gen._store(True)
        built = time.perf_counter() - t0
        first, second = epoch(gen)
        print("resident (store of %.2f GB decoded and uploaded in %.1f s = %.0f images/s, once): %.0f images/s (first epoch %.0f)"
              % (st.device_arena.numel() / 1e9, built, images / built, second, first), flush=True)
        # one epoch of the streamed tier taken apart
        gen = ILSVRCGenerator(root, store="stream", prefetch_batches=0, decode_threads=threads, dtype=torch.bfloat16)
        st, rng, crop = gen._store(True), np.random.default_rng(0), (224, 224)
        parts = {"decode": [], "pack": [], "upload": [], "tables + se_image_batch": []}
        for b in range(images // B + 1):
            idx = rng.choice(images, B, replace=False)
            torch.cuda.synchronize()
            t = [time.perf_counter()]
            key, decoded = st.collect(idx)
            t.append(time.perf_counter())
            st.pending[key] = {i: _Done(a) for i, a in decoded.items()}          # stage() finds the batch decoded: what is left is packing
            slot, nbytes, offsets, sizes = st.stage(idx)
            t.append(time.perf_counter())
            arena = st.upload(slot, nbytes, gen._dev())
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            params = gen.draw_params(sizes, True, True, rng)
            compose_on_device(arena, offsets, sizes, params, crop, gen._device_stats(), False, gen.dtype)
            st.launched(slot)
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            if b:                                                                 # the first batch warms up
                for name, dt in zip(parts, np.diff(t)):
                    parts[name].append(dt * 1e3)
        med = {name: float(np.median(v)) for name, v in parts.items()}
        total = sum(med.values())
        print("one streamed batch of %d taken apart (medians of %d batches, %.1f MB staged): %s; sum %.2f ms = %.0f images/s without overlap"
              % (B, len(parts["decode"]), nbytes / 1e6, "; ".join("%s %.2f ms (%.0f %%)" % (n, v, 100 * v / total) for n, v in med.items()),
                 total, B / total * 1e3), flush=True)
        print("decode alone: %.0f images/s on %d threads = %.2f ms per image and thread" % (B / med["decode"] * 1e3, threads, med["decode"] * threads / B))


class _Done(object):
    """A finished future, for handing already decoded images to _StreamStore.stage."""

    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value

    def cancel(self):
        return False


def bench_tiny(reps=40, batch=20, stored=10000):
    """The in-memory batch (datasets/common.py) at 128 x 32 x 32 x 3 and 512 x 32 x 32 x 3 from a store of `stored` CIFAR-sized images:
    se_tiny_batch with the 'cifar-10' preset (shifts +-15 %, zoom 0.75 .. 1.25, flip) as the bare kernel (parameters already on the
    device) and as the whole compose_batch (draw_affine + affine_matrices on the host, one upload, one launch), next to the torch
    composition of the default shift + flip batch (index upload, index_select, device draws, grid_sample, where, channels_last copy) and
    its device part alone (apply_transform + channels_last copy on a gathered batch with drawn parameters).  The four timed alternately
    in one process: `reps` windows of `batch` back-to-back calls each (HIP events around a window) after 3 warm-up calls, median / 10th
    / 90th percentile of the per-call time.  Bytes: the float32 batch out, over the kernel's time (its reads hit the same few images'
    cache lines four times over)."""
    sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
    from datasets import CIFAR10_AUGMENTATION, InMemoryDatasetGenerator
    from datasets.common import affine_matrices

    rng = np.random.default_rng(0)
    X = rng.integers(0, 256, (stored, 32, 32, 3)).astype(np.float32)
    labels = [0] * stored
    affine = InMemoryDatasetGenerator(X, X[:16], labels, labels[:16], train_generator_kwargs=dict(CIFAR10_AUGMENTATION))
    plain = InMemoryDatasetGenerator(X, X[:16], labels, labels[:16])
    assert affine.affine is not None and plain.affine is None
    for B in (128, 512):
        idx = rng.permutation(stored)[:B]
        draws = np.random.default_rng(1)
        store = affine._raw_store(True)
        p = affine.draw_affine(B, 32, 32, draws)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        index, M, flags = dev(idx.astype(np.int64)), dev(affine_matrices(p, 32, 32)), dev(p["hflip"].astype(np.int32))
        out = torch.empty((B, 32, 32, 3), device="cuda")
        gathered = plain.compose_batch(idx, train=True, augment=False).contiguous()
        drawn = plain.draw_transform(B, 32, 32, gathered.device)
        kernel = lambda: sehip.tiny_batch(store, index, M, flags, affine._stats[0], affine._stats[1], "nearest", 0.0, out=out)
        whole = lambda: affine.compose_batch(idx, train=True, augment=True, rng=draws)
        torch_whole = lambda: plain.compose_batch(idx, train=True, augment=True)
        torch_dev = lambda: plain.apply_transform(gathered, *drawn).contiguous(memory_format=torch.channels_last)
        k, w, tw, td = windows((kernel, whole, torch_whole, torch_dev), reps, batch)
        assert bool(torch.isfinite(out).all())
        nbytes = 4.0 * B * 32 * 32 * 3
        print("tiny batch %d x 32 x 32 x 3 ('cifar-10' preset): se_tiny_batch %.1f us (%.1f-%.1f), %.2f MB out = %.0f GB/s; whole compose_batch "
              "(host draws + matrices + upload + launch) %.1f us (%.1f-%.1f); torch composition of the shift + flip batch: device part %.1f us "
              "(%.1f-%.1f) = x%.2f of the kernel, whole compose_batch %.1f us (%.1f-%.1f) = x%.2f of the affine compose_batch"
              % (B, k[0], k[1], k[2], nbytes / 1e6, nbytes / (k[0] * 1e-6) / 1e9, w[0], w[1], w[2], td[0], td[1], td[2], td[0] / k[0],
                 tw[0], tw[1], tw[2], tw[0] / w[0]), flush=True)


def bench_knn(reps=30, batch=10):
    """k-NN classification (evaluate_classification_accuracy.knn_classification): se_knn_vote alone on the neighbour lists of
    se_retrieve_topk next to the torch composition it replaces -- cls[idx] -> scatter_add into a [q, C] int32 histogram -> topk(5) --
    the two timed alternately in one process: `reps` windows of `batch` back-to-back calls each (HIP events around a window) after 3
    warm-up calls, median / 10th / 90th percentile of the per-call time.  Then the whole knn_classification on features already on the
    device (lists + vote + the copy of the [q, 5] rankings to the host; host clock around a call that ends in that copy, median of 5
    after one warm-up call).  Shapes: 10,000 test x 50,000 training rows x D = 100 with k = 20 and 100 classes; 50,000 x 50,000 x 100
    with k = 200 and 1000 classes; seeded Gaussian features, squared Euclidean distances.  Bytes of the vote: the lists in, the two
    [q, 5] results out (the class table stays in cache)."""
    import time
    import evaluate_classification_accuracy as eca
    rng = np.random.default_rng(0)
    for q, n, d, k, C in ((10000, 50000, 100, 20, 100), (50000, 50000, 100, 200, 1000)):
        train = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
        test = torch.from_numpy(rng.standard_normal((q, d)).astype(np.float32)).cuda()
        y = rng.integers(0, C, size=n)
        cls = torch.from_numpy(y.astype(np.int32)).cuda()
        _, lists = sehip.retrieve_topk(test, train, k, metric=sehip.METRIC_EUCLID)
        cls64, lists64 = cls.long(), lists.long()      # (the composition's index conversions are not timed)
        ones = torch.ones((q, k), dtype=torch.int32, device="cuda")

        def kernel():
            return sehip.knn_vote(lists, cls, C, [k], top=5)

        def composition():
            hist = torch.zeros((q, C), dtype=torch.int32, device="cuda").scatter_add_(1, cls64[lists64], ones)
            return torch.topk(hist, 5, dim=1)
        votes_k, votes_t = kernel()[1][:, 0], composition()[0]
        assert torch.equal(votes_k, votes_t.int()), "the two legs disagree on the vote counts"
        kt, tt = windows((kernel, composition), reps, batch)
        moved = 4.0 * q * k + 2 * 4.0 * q * 5
        print("knn vote q=%d k=%d C=%d: se_knn_vote %.1f us (%.1f-%.1f), torch composition %.1f us (%.1f-%.1f): x%.2f; the kernel moves %.1f MB "
              "= %.0f GB/s" % (q, k, C, kt[0], kt[1], kt[2], tt[0], tt[1], tt[2], tt[0] / kt[0], moved / 1e6, moved / (kt[0] * 1e-6) / 1e9), flush=True)
        eca.knn_classification(train, y, test, ks=[k], num_classes=C)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eca.knn_classification(train, y, test, ks=[k], num_classes=C)
            ts.append((time.perf_counter() - t0) * 1e3)
        print("knn_classification %d x %d x %d, k=%d, C=%d, features on the device: median %.2f ms (min %.2f, max %.2f) per call, rankings on the host"
              % (q, n, d, k, C, float(np.median(ts)), min(ts), max(ts)), flush=True)
        del train, test, lists, lists64, ones


def bench_ndcg(rounds=12, batch=3):
    """se_ndcg next to se_hierarchical_precision on the SAME int32 rankings (all pairs of seeded Gaussian features, cosine, 100 classes):
    ks = 1..250 with the whole list (want_full = 1) against ks = 1..250 with whole-list AHP and AP in class order (ahp_len = 0,
    want_ap = 1), the two timed alternately in one process: `rounds` windows of `batch` back-to-back calls each (HIP events around a
    window) after 3 warm-up calls, median / 10th / 90th percentile of the per-call time.  Shapes: 50,000 x 50,000, 10,000 x 10,000, and
    the head-only form -- 50,000 lists of 251 entries, want_full = 0 against AHP@250 without AP.  (profiles/ndcg_bench.txt)"""
    C, d = 100, 100
    ks = torch.arange(1, 251, dtype=torch.int32, device="cuda")
    for n, head in ((10000, False), (50000, False), (50000, True)):
        rng = np.random.default_rng(1)
        x = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).cuda()
        sehip.normalize_rows_(x)
        cls = torch.from_numpy(rng.integers(0, C, size=n).astype(np.int32)).cuda()
        tab = rng.random((C, C)); tab = (tab + tab.T) / 2; np.fill_diagonal(tab, 1.0)
        counts = np.bincount(cls.cpu().numpy(), minlength=C)
        order = [np.argsort(-tab[c], kind="stable") for c in range(C)]
        best = np.stack([np.cumsum(np.repeat(tab[c][order[c]], counts[order[c]])) for c in range(C)])
        tab_d, best_d = torch.from_numpy(tab).cuda(), torch.from_numpy(best).cuda()
        rk = sehip.rank_rows(sehip.pairwise_dist(x, x, metric=sehip.METRIC_COSINE))
        qidx = torch.arange(n, dtype=torch.int32, device="cuda")
        disc = sehip.ndcg_discounts(n, "cuda")
        one = sehip.ndcg_ideal(tab_d, counts, disc, ks.tolist(), full=not head)
        ideal = torch.stack([one, one], dim=2).contiguous()
        if head:
            rk = rk[:, :251].contiguous()
            best_d = best_d[:, :252].contiguous()
        L = rk.shape[1]
        curves = sehip.hprec_reciprocal_curves(best_d, best_d)

        def ndcg():
            return sehip.ndcg(rk, cls, cls, qidx, tab_d, tab_d, disc, ideal, ks, want_full=not head, list_len=L)

        def hprec():
            return sehip.hierarchical_precision(rk, cls, cls, qidx, tab_d, tab_d, best_d, best_d, ks, ahp_len=250 if head else 0,
                                                want_ap=not head, curves=curves, list_len=L)
        got = ndcg()
        assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0 + 1e-9, "NDCG outside [0, 1]"
        nt, ht = windows((ndcg, hprec), rounds, batch)
        print("ndcg %-9s q=%d list_len=%d C=%d nk=250: se_ndcg %.1f us (%.1f-%.1f), se_hierarchical_precision %.1f us (%.1f-%.1f): x%.2f; "
              "%.1f GB/s of ranks" % ("head only" if head else "whole", n, L, C, nt[0], nt[1], nt[2], ht[0], ht[1], ht[2], ht[0] / nt[0],
                                      4.0 * n * L / (nt[0] * 1e-6) / 1e9), flush=True)
        del x, rk, best_d, curves


def bench_bootstrap(rounds=10, reps=10000, m=11, chunk_bytes=512 << 20):
    """Bootstrap over queries: se_bootstrap_means (sehip.bootstrap_means on a [q, 11] float64 table, row pitch padded to 16 doubles
    once, outside the timing) next to the torch composition of the same work -- torch.randint -> index_select -> mean(dim=1), in
    chunks of replicates whose gathered rows fit `chunk_bytes` -- the two timed alternately in one process: `rounds` rounds of one
    call each (HIP events around a call) after 3 warm-up calls, median / 10th / 90th percentile.  The composition draws another
    stream, so the legs are compared on their spread, not on their values.  GB/s: reps x q gathered rows of m doubles over the
    kernel's time.  Shapes: q = 10,000 and 50,000 queries, m = 11 metric columns, 10,000 replicates; seeded uniform values."""
    rng = np.random.default_rng(0)
    for q in (10000, 50000):
        vals = torch.from_numpy(rng.random((q, m))).cuda()
        padded = torch.zeros((q, 16), dtype=torch.float64, device="cuda")
        padded[:, :m] = vals
        table = padded[:, :m]          # pitch 16: a row inside one 128-byte line; the binding takes it as it is
        chunk = max(1, min(reps, chunk_bytes // (q * m * 8)))

        def kernel():
            return sehip.bootstrap_means(table, reps, seed=1)

        def composition():
            out = torch.empty((reps, m), dtype=torch.float64, device="cuda")
            for r0 in range(0, reps, chunk):
                c = min(chunk, reps - r0)
                idx = torch.randint(q, (c * q,), device="cuda")
                out[r0:r0 + c] = vals.index_select(0, idx).view(c, q, m).mean(dim=1)
            return out
        k, t = kernel(), composition()
        sd = float(vals.std(dim=0, unbiased=False).mean()) / np.sqrt(q)
        for name, x in (("kernel", k), ("composition", t)):      # both legs resample: the spread of their replicate means is the theory's
            ratio = float(x.std(dim=0, unbiased=False).mean()) / sd
            assert abs(ratio - 1.0) < 0.05, (name, ratio)
        kt, tt = windows((kernel, composition), rounds, 1)
        moved = 8.0 * m * q * reps
        print("bootstrap q=%d m=%d reps=%d: se_bootstrap_means %.2f ms (%.2f-%.2f), torch composition in chunks of %d replicates %.2f ms "
              "(%.2f-%.2f): x%.2f; the kernel gathers %.1f GB of rows = %.0f GB/s"
              % (q, m, reps, kt[0] / 1e3, kt[1] / 1e3, kt[2] / 1e3, chunk, tt[0] / 1e3, tt[1] / 1e3, tt[2] / 1e3, tt[0] / kt[0], moved / 1e9,
                 moved / (kt[0] * 1e-6) / 1e9), flush=True)
        del vals, padded, table


def bench_ranked(reps=10, batch=3, host_rows=500):
    """Evaluation of given rankings.  se_complete_rankings at 10,000 x 10,000 and 50,000 x 50,000 with lists of 0, 250 and N entries
    and both `order` forms (NULL; a random permutation), next to a device-to-device copy of the same 4 q N bytes and next to a torch
    composition of the same completion -- key = position in the list for listed items, list length + position in `order` for the
    others, then argsort(key) -- the three timed alternately: `reps` windows of `batch` back-to-back calls (HIP events around a
    window) after 3 warm-up calls, median / 10th / 90th percentile of the per-call time.  At 50,000 x 50,000 the composition runs on
    a tile of 10,000 rows and its time is multiplied by 5.  Lists: row i is the permutation j -> ((10 i + 3) j + 7 i) mod N (10 i + 3
    is coprime to N = 2^a 5^b), cut to the list length.  Then the whole hierarchical_precision_ranked (P@1..250, whole-list AHP, AP;
    100 classes) at 10,000 x 10,000 on a dictionary of top-250 lists with all_ids, host clock around the call (median of 3 after a
    warm-up call), next to the host hierarchical_precision on the first `host_rows` queries of the same dictionary (one call, scaled to
    all queries)."""
    import time
    import tempfile
    rng = np.random.default_rng(0)
    for q, n in ((10000, 10000), (50000, 50000)):
        rows = torch.arange(q, dtype=torch.int64, device="cuda")[:, None]
        full = torch.empty((q, n), dtype=torch.int32, device="cuda")
        for r0 in range(0, q, 5000):
            full[r0:r0 + 5000] = (((10 * rows[r0:r0 + 5000] + 3) * torch.arange(n, dtype=torch.int64, device="cuda")[None, :] + 7 * rows[r0:r0 + 5000]) % n).int()
        order = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
        inv = torch.empty(n, dtype=torch.int64, device="cuda")
        inv[order.long()] = torch.arange(n, dtype=torch.int64, device="cuda")
        out, dst = sehip.empty_rows(q, n, torch.int32, "cuda"), torch.empty((q, n), dtype=torch.int32, device="cuda")
        tq = min(q, 10000)          # rows of the torch composition
        for L in (0, 250, n):
            lists = full[:, :L]
            lists64 = lists[:tq].long()
            pos = torch.arange(L, dtype=torch.int64, device="cuda")[None, :].expand(tq, L)
            for name, od, key0 in (("NULL", None, torch.arange(n, dtype=torch.int64, device="cuda")), ("permutation", order, inv)):
                def kernel():
                    return sehip.complete_rankings(lists, n, order=od, out=out)

                def copy():
                    return dst.copy_(out)

                def composition():
                    key = (L + key0)[None, :].repeat(tq, 1)
                    if L:
                        key.scatter_(1, lists64, pos)
                    return torch.argsort(key, dim=1).int()
                rank, status = kernel()
                assert not bool(status.any()) and torch.equal(rank[:tq], composition()), "the two legs disagree"
                kt, ct, tt = windows((kernel, copy, composition), reps, batch)
                scale = q / tq
                print("complete_rankings %d x %d, list length %d, order %s: se_complete_rankings %.0f us (%.0f-%.0f) = %.2f TB/s written; "
                      "copy of the same %.1f GB %.0f us (%.0f-%.0f): kernel / copy x%.2f; torch composition%s %.0f us (%.0f-%.0f): x%.1f the kernel"
                      % (q, n, L, name, kt[0], kt[1], kt[2], 4.0 * q * n / (kt[0] * 1e-6) / 1e12, 4.0 * q * n / 1e9, ct[0], ct[1], ct[2], kt[0] / ct[0],
                         "" if tq == q else " (%d rows, x%d)" % (tq, scale), tt[0] * scale, tt[1] * scale, tt[2] * scale, tt[0] * scale / kt[0]), flush=True)
            del lists64, pos
        del full, out, dst
        torch.cuda.empty_cache()

    # ---- the whole evaluation at 10,000 x 10,000 ----
    from class_hierarchy import ClassHierarchy
    n = q = 10000
    edges = np.load(os.path.join(ROOT, "tests", "golden", "hierarchy_cifar.npz"))["edges"]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        for p, c in edges.tolist():
            f.write("%d %d\n" % (p, c))
    hier = ClassHierarchy.from_file(f.name, id_type=int)
    os.unlink(f.name)
    labels = rng.integers(0, 100, size=n).tolist()
    i = np.arange(q, dtype=np.int64)[:, None]
    top = (((10 * i + 3) * np.arange(250, dtype=np.int64)[None, :] + i) % n)        # (j = 0 is the query itself)
    retrieved = {k: top[k].tolist() for k in range(q)}
    all_ids = list(range(n))
    ks = list(range(1, 251))

    def device():
        return hier.hierarchical_precision_ranked(retrieved, labels, ks, compute_ahp=True, compute_ap=True, all_ids=all_ids, per_query=False)[0]
    got = device()
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device()
        ts.append(time.perf_counter() - t0)
    head = {k: retrieved[k] for k in range(host_rows)}
    t0 = time.perf_counter()
    _, host_q = hier.hierarchical_precision(head, labels, ks, compute_ahp=True, compute_ap=True, all_ids=all_ids)
    th = (time.perf_counter() - t0) * q / host_rows
    _, dev_q = hier.hierarchical_precision_ranked(head, labels, ks, compute_ahp=True, compute_ap=True, all_ids=all_ids)
    err = max(abs(dev_q[m][k] - host_q[m][k]) for m in host_q for k in head)
    print("hierarchical_precision_ranked %d x %d (top-250 lists as a dict, all_ids, P@1..250 + AHP + AP, 100 classes): median %.3f s (min %.3f, "
          "max %.3f) per call; host hierarchical_precision on the same dictionary: %.1f s (%d queries timed, scaled): x%.0f; largest per-query "
          "difference on those queries %.1e; mean AP %.4f" % (q, n, float(np.median(ts)), min(ts), max(ts), th, host_rows, th / float(np.median(ts)), err,
                                                              got["AP"]), flush=True)


def bench_adagrad(reps=40, batch=20, steps=200):
    """The Adagrad update (learn_devise.py): se_adagrad_step over the flat parameter / accumulator / gradient / L2 buffers engine.FlatState
    builds for ResNet-110-fc (100 outputs) and ResNet-50 (1000 outputs), with and without the regulariser stream, next to the torch
    composition of the same update on the same buffers with the learning rate in a device scalar (what a captured step would launch: g +=
    l2 * p; a += g * g; p -= (g * lr) / (sqrt(a) + eps): 7 launches, 6 without the regulariser), the four timed alternately in one
    process: `reps` windows of `batch` back-to-back calls each (HIP events around a window) after 3 warm-up calls, median / 10th / 90th
    percentile of the per-call time.  Bytes: 3 streams in (4 with the regulariser) and 2 out, over the kernel's time, against the 6.29 TB/s
    a float4 copy reaches on MI355X (8 TB/s spec); the ResNet-110-fc buffers (7 MB each) stay in the on-chip caches between calls, so their
    rate is not an HBM rate.  Then one ResNet-110-fc training step (batch 128, fp32, HIP-graph replay) under the DeViSE loss with
    Trainer(optimizer='adagrad') next to the cosine-loss step with SGD, the two timed alternately."""
    sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
    import utils
    import learn_devise as ld
    from datasets import SyntheticGenerator
    from engine import FlatState, Trainer
    HBM = 6.29e12
    lr, eps = 0.001, 1e-7

    for arch, outputs in (("resnet-110-fc", 100), ("resnet-50", 1000)):
        torch.manual_seed(0)
        model = utils.build_network(outputs, arch, input_channels=3).cuda()
        flat = FlatState(model, {id(p): model.regularizer for p in model.regularized_parameters()})
        n = flat.total
        p, a, l2 = flat.flat_p, flat.flat_v, flat.flat_l2
        g = torch.randn(n, device="cuda") * 1e-2
        lr_t = torch.full((), lr, device="cuda")

        def kernel(l2):
            return lambda: sehip.adagrad_step_(p, a, g, l2, lr=lr_t, epsilon=eps)

        def composition(l2):
            def f():
                if l2 is not None:
                    g.addcmul_(l2, p)
                a.addcmul_(g, g)
                p.sub_((g * lr_t).div_(a.sqrt().add_(eps)))
            return f
        k1, k0, t1, t0 = windows((kernel(l2), kernel(None), composition(l2), composition(None)), reps, batch)
        assert bool(torch.isfinite(p).all())
        for what, k, t, streams in (("with the regulariser", k1, t1, 6), ("without", k0, t0, 5)):
            gbs = streams * 4.0 * n / (k[0] * 1e-6)
            print("adagrad %s, %d floats per buffer (%.1f MB), %s: kernel %.1f us (%.1f-%.1f), torch composition %.1f us (%.1f-%.1f): x%.2f; "
                  "the kernel moves %.0f MB = %.0f GB/s = %.1f%% of the HBM copy rate"
                  % (arch, n, 4.0 * n / 1e6, what, k[0], k[1], k[2], t[0], t[1], t[2], t[0] / k[0], streams * 4.0 * n / 1e6, gbs / 1e9,
                     100.0 * gbs / HBM), flush=True)
        del model, flat, p, a, l2, g

    E = np.load(os.path.join(ROOT, "tests", "golden", "embeddings.npz"))["cifar100_unitsphere"]
    Ed = torch.from_numpy(E.astype(np.float32)).cuda()
    trainers = {}
    for name in ("cosine", "devise"):
        torch.manual_seed(0)
        model = utils.build_network(100, "resnet-110-fc", input_channels=3).cuda()
        l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
        if name == "cosine":
            tr = Trainer(model, {"l2norm": (utils.CosineEmbeddingLoss(Ed), 1.0)}, {"l2norm": [utils.nn_accuracy(Ed, dot_prod_sim=True)]},
                         lr=0.1, momentum=0.9, clipnorm=10.0, l2_of=l2_of, autocast_dtype=None, memory_format=torch.contiguous_format)
        else:
            losses, metrics = ld.build_losses(Ed, 0.1)
            tr = Trainer(model, losses, metrics, lr=0.001, l2_of=l2_of, autocast_dtype=None, memory_format=torch.contiguous_format,
                         optimizer="adagrad")
        seq = SyntheticGenerator(100, 32, 3, 128 * 8, 128).train_sequence(128, shuffle=False)
        batches = [seq[i] for i in range(8)]
        assert tr.enable_graphs(*batches[0]), name
        for i in range(10):
            tr.train_step(*batches[i % 8], {})
        trainers[name] = (tr, batches)
    ms = {name: [] for name in trainers}
    for _ in range(3):                       # alternate the two models: the same machine state for both
        for name, (tr, batches) in trainers.items():
            logs = {}
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                tr.train_step(*batches[i % 8], logs)
            b.record()
            torch.cuda.synchronize()
            assert np.isfinite(float(logs["loss"]))
            ms[name].append(a.elapsed_time(b) / steps)
    for name, what in (("cosine", "cosine-loss step, SGD"), ("devise", "DeViSE step, fused Adagrad")):
        step = float(np.median(ms[name]))
        print("ResNet-110-fc %s, batch 128, fp32, HIP-graph replay: %.3f ms/step (median of 3 x %d steps; %s), "
              "%.0f images/s" % (what, step, steps, ", ".join("%.3f" % v for v in ms[name]), 128 / step * 1e3))


def bench_sgd(reps=30, batch=10, steps=200):
    """The Keras-SGD update of the four SGD trainers (engine.Trainer.apply_update): the fused pair sehip.grad_clip_factor +
    sehip.sgd_step_ next to the torch composition of the same update, whose lines are copied here as the trainer runs them in a
    captured step (learning rate in a device scalar, one process: no gradient scale).  Flat buffers of 1.75 M (ResNet-110-fc), 25.6 M
    (ResNet-50) and 68 M floats (the [8142, 8142] label-embedding table and its backbone); {clip + regulariser, clip only, neither} x
    {plain, Nesterov}; the candidates timed alternately in one process: `reps` windows of `batch` back-to-back calls each (HIP events
    around a window) after 3 warm-up calls, median / 10th / 90th percentile of the per-call time.  Bytes of the fused pair: 1 stream (3
    with the regulariser) for the norm, 3 (4) in and 2 out for the update, over its time, against the 6.29 TB/s a float4 copy
    reaches on MI355X; the 7 MB buffers stay in the on-chip caches between calls, so theirs is not an HBM rate.  Then one
    ResNet-110-fc training step (batch 128, fp32, HIP-graph replay, cosine loss, clipnorm 10) with Trainer(fused_sgd=True) next to the
    default trainer, the two timed alternately."""
    sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
    import utils
    from datasets import SyntheticGenerator
    from engine import Trainer
    HBM = 6.29e12
    lr, mom, clipnorm = 0.001, 0.9, 10.0

    for n in (1750016, 25600000, 68000000):
        gen = torch.Generator(device="cuda").manual_seed(0)
        p = torch.randn(n, device="cuda", generator=gen) * 0.05
        g = torch.randn(n, device="cuda", generator=gen) * 1e-2
        l2 = torch.full((n,), 1e-3, device="cuda")
        v, gc = torch.zeros_like(p), g.clone()                # gc: the composition overwrites its gradient
        lr_t = torch.full((), lr, device="cuda")
        ws = torch.empty(sehip.SGD_MAX_BLOCKS * 8, dtype=torch.uint8, device="cuda")
        stats = torch.zeros(2, device="cuda")

        def fused(clip, reg, nesterov):
            def f():
                if clip:
                    sehip.grad_clip_factor(g, p, l2 if reg else None, clipnorm=clipnorm, workspace=ws, out=stats)
                sehip.sgd_step_(p, v, g, l2 if reg else None, lr=lr_t, clip=stats[1:] if clip else None, momentum=mom, nesterov=nesterov)
            return f

        def composition(clip, reg, nesterov):
            def f():                                          # engine.Trainer.apply_update with lr_tensor, grad_scale == 1
                if reg:
                    gc.addcmul_(l2, p)
                if clip:
                    norm = torch.linalg.vector_norm(gc)
                    gc.mul_(torch.clamp(clipnorm / (norm + 1e-12), max=1.0))
                step = gc * lr_t
                v.mul_(mom).sub_(step)
                if nesterov:
                    p.add_(v, alpha=mom).sub_(step)
                else:
                    p.add_(v)
            return f

        configs = [(c, r, nes) for c, r in ((True, True), (True, False), (False, False)) for nes in (False, True)]
        res = windows([fn(*cfg) for cfg in configs for fn in (fused, composition)], reps, batch)
        assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(v).all())
        for i, (clip, reg, nes) in enumerate(configs):
            k, t = res[2 * i], res[2 * i + 1]
            streams = ((3 if reg else 1) if clip else 0) + (4 if reg else 3) + 2
            gbs = streams * 4.0 * n / (k[0] * 1e-6)
            verdict = "the ranges overlap" if k[2] >= t[1] else "apart"
            print("sgd %d floats per buffer (%.1f MB), %s, %s: fused %.1f us (%.1f-%.1f), torch composition %.1f us (%.1f-%.1f): x%.2f, %s; "
                  "the fused pair moves %.0f MB = %.0f GB/s = %.1f%% of the HBM copy rate"
                  % (n, 4.0 * n / 1e6, "clip + regulariser" if reg else ("clip only" if clip else "no clip, no regulariser"),
                     "Nesterov" if nes else "plain", k[0], k[1], k[2], t[0], t[1], t[2], t[0] / k[0], verdict, streams * 4.0 * n / 1e6,
                     gbs / 1e9, 100.0 * gbs / HBM), flush=True)
        del p, g, l2, v, gc

    E = np.load(os.path.join(ROOT, "tests", "golden", "embeddings.npz"))["cifar100_unitsphere"]
    Ed = torch.from_numpy(E.astype(np.float32)).cuda()
    trainers = {}
    for name in ("composition", "fused"):
        torch.manual_seed(0)
        model = utils.build_network(100, "resnet-110-fc", input_channels=3).cuda()
        l2_of = {id(p): model.regularizer for p in model.regularized_parameters()}
        tr = Trainer(model, {"l2norm": (utils.CosineEmbeddingLoss(Ed), 1.0)}, {"l2norm": [utils.nn_accuracy(Ed, dot_prod_sim=True)]},
                     lr=0.1, momentum=0.9, clipnorm=10.0, l2_of=l2_of, autocast_dtype=None, memory_format=torch.contiguous_format,
                     fused_sgd=name == "fused")
        seq = SyntheticGenerator(100, 32, 3, 128 * 8, 128).train_sequence(128, shuffle=False)
        batches = [seq[i] for i in range(8)]
        assert tr.enable_graphs(*batches[0]), name
        for i in range(10):
            tr.train_step(*batches[i % 8], {})
        trainers[name] = (tr, batches)
    ms = {name: [] for name in trainers}
    for _ in range(5):                       # alternate the two trainers: the same machine state for both
        for name, (tr, batches) in trainers.items():
            logs = {}
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                tr.train_step(*batches[i % 8], logs)
            b.record()
            torch.cuda.synchronize()
            assert np.isfinite(float(logs["loss"]))
            ms[name].append(a.elapsed_time(b) / steps)
    for name, what in (("composition", "default trainer (torch composition)"), ("fused", "Trainer(fused_sgd=True), as SE_FUSED_SGD=1 builds it")):
        step = float(np.median(ms[name]))
        print("ResNet-110-fc cosine-loss step, %s, batch 128, fp32, HIP-graph replay: %.3f ms/step (median of 5 x %d steps; %s), "
              "%.0f images/s" % (what, step, steps, ", ".join("%.3f" % v for v in sorted(ms[name])), 128 / step * 1e3))


def bench_shortcut(reps=30, batch=10, B=128):
    """The pyramidal shortcut (models/cifar_pyramidnet.py): sehip.shortcut_add against s + F.pad(F.avg_pool2d(x, stride), ...) at the
    shapes of PyramidNet-272-200 for batch 128 -- the widest stride-1 block of each stage (blocks 29, 59, 89) and both stride-2 blocks
    (30, 60) -- in fp32 NCHW (the trainer's default for the CIFAR-sized nets) and bf16 channels_last.  One call = forward + backward
    through autograd (torch.autograd.grad of the output w.r.t. s and x), so both candidates pay the same autograd bookkeeping; the
    two are timed alternately in one process: `reps` windows of `batch` back-to-back calls each (HIP events around a window) after 3
    warm-up calls, median / 10th / 90th percentile of the per-call time.  Bytes the fused pair has to move: s and x in, out out, the
    shortcut's slice of dout in, dx out; over its time, against the 6.29 TB/s a float4 copy reaches on MI355X."""
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, "semantic-embeddings_amd"))
    from models.cifar_pyramidnet import block_widths
    HBM = 6.29e12
    n, widths = block_widths(272, 200, True)
    shapes = []
    for k in (n - 1, n, 2 * n - 1, 2 * n, 3 * n - 1):
        stage, stride = k // n, 2 if k in (n, 2 * n) else 1
        hw_out = 32 >> stage
        shapes.append((k, 4 * widths[k - 1], 4 * widths[k], hw_out * stride, stride))

    for dtype, fmt, label in ((torch.float32, torch.contiguous_format, "fp32 NCHW"), (torch.bfloat16, torch.channels_last, "bf16 NHWC")):
        for k, cin, c, hx, stride in shapes:
            h = hx // stride
            gen = torch.Generator(device="cuda").manual_seed(k)
            s = torch.randn(B, c, h, h, device="cuda", generator=gen).to(dtype).contiguous(memory_format=fmt).requires_grad_(True)
            x = torch.randn(B, cin, hx, hx, device="cuda", generator=gen).to(dtype).contiguous(memory_format=fmt).requires_grad_(True)
            g = torch.randn(B, c, h, h, device="cuda", generator=gen).to(dtype).contiguous(memory_format=fmt)

            def fused():
                return torch.autograd.grad(sehip.shortcut_add(s, x, stride, 0), (s, x), g)

            def composition():
                sc = F.avg_pool2d(x, stride) if stride > 1 else x
                return torch.autograd.grad(s + F.pad(sc, (0, 0, 0, 0, 0, c - cin)), (s, x), g)
            (fs, fx), (ts_, tx) = fused(), composition()
            assert torch.equal(fs, ts_) and float((fx.float() - tx.float()).abs().max()) <= 2.0 ** -7 * float(tx.float().abs().max())
            kf, kt = windows((fused, composition), reps, batch)
            eb = 4 if dtype == torch.float32 else 2
            nbytes = eb * (2 * s.numel() + 2 * x.numel() + B * cin * h * h)
            print("shortcut %s, block %d: s %d x %d x %d x %d, x %d channels at %d x %d, stride %d: fused %.1f us (%.1f-%.1f), torch "
                  "composition %.1f us (%.1f-%.1f): x%.2f; the fused pair moves %.0f MB = %.0f GB/s = %.1f%% of the HBM copy rate"
                  % (label, k, B, c, h, h, cin, hx, hx, stride, kf[0], kf[1], kf[2], kt[0], kt[1], kt[2], kt[0] / kf[0], nbytes / 1e6,
                     nbytes / (kf[0] * 1e-6) / 1e9, 100.0 * nbytes / (kf[0] * 1e-6) / HBM), flush=True)
            del s, x, g, fs, fx, ts_, tx


def bench_qg(args):
    """One query-vs-gallery leg on synthetic unit-norm features (class centre + noise), per phase (HIP events around every kernel call
    of the driver, summed) and as wall time of the whole call."""
    import time
    import warnings
    from recall_precision import recall_precision_device
    big = not args.small
    q = args.q or (50000 if big else 2000)
    given = {a.split("=")[0] for a in sys.argv[1:]}                          # --n / --d have defaults meant for the other benchmarks
    n = args.n if "--n" in given else (1281167 if big else 60000)
    d = args.d if "--d" in given else (1000 if big else 100)
    C = args.classes or (1000 if big else 100)
    gen = torch.Generator(device="cuda").manual_seed(0)
    centers = torch.randn((C, d), device="cuda", generator=gen)

    def features(rows, cls):
        f = torch.empty((rows, d), dtype=torch.float32, device="cuda")
        for r0 in range(0, rows, 65536):           # in pieces: no second rows x d temporary
            r1 = min(rows, r0 + 65536)
            f[r0:r1] = centers[cls[r0:r1]] + args.noise * torch.randn((r1 - r0, d), device="cuda", generator=gen)
        return sehip.normalize_rows_(f)

    gcls = torch.arange(n, device="cuda") % C                              # ILSVRC's layout: C classes of n / C rows
    qcls = torch.arange(q, device="cuda") % C
    fg, fq = features(n, gcls), features(q, qcls)
    g_lab, q_lab = gcls.cpu().tolist(), qcls.cpu().tolist()
    print("query-vs-gallery: q=%d n=%d d=%d classes=%d (R = %d per query), noise %.1f, cosine" % (q, n, d, C, n // C, args.noise))
    if args.ranking_path:
        rows = min(q, args.rank_rows)
        pd = sehip.empty_rows(rows, n, torch.float32, "cuda")
        rk = sehip.empty_rows(rows, n, torch.int32, "cuda")
        cls_d, qc = gcls.to(torch.int32), qcls[:rows].to(torch.int32).contiguous()
        hit_off = torch.arange(rows + 1, dtype=torch.int64, device="cuda") * 0
        hit_off[1:] = torch.cumsum(torch.bincount(gcls, minlength=C)[qcls[:rows]], 0)
        total = int(hit_off[-1])
        steps = (("se_pairwise_dist", lambda: sehip.pairwise_dist(fq[:rows], fg, metric=sehip.METRIC_COSINE, out=pd)),
                 ("se_rank_rows", lambda: sehip.rank_rows(pd, out=rk)),
                 ("se_relevant_positions", lambda: sehip.relevant_positions(rk, cls_d, qc, None, hit_off, num_classes=C, total=total)))
        tot = 0.0
        for name, fn in steps:
            med, mn = timeit(fn, max(1, min(args.reps, 3)))
            tot += med
            print("  %-24s %d rows: median %.2f ms (min %.2f)" % (name, rows, med, mn))
        print("  ranking path: %.2f ms per %d rows -> %.2f s for all %d queries (scaled by %d / %d)" % (tot, rows, tot * q / rows / 1e3, q, q, rows))
        return
    phases = {}

    def timed(phase, fn):
        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            phases.setdefault(phase(*a, **k) if callable(phase) else phase, []).append((e0, e1))
            return out
        return run

    def pdist(a, b, cosine, sqa, sqb, kblocks, out=None):
        return sehip.pairwise_dist(a, b, metric=sehip.METRIC_COSINE, kblocks=kblocks, out=out)

    kernels = {"normalize_rows_": lambda x: x,                             # the features are unit-norm already
               "pairwise_dist": timed(lambda a, b, c, sa, sb, kb, out=None: "distance slabs" if out is not None else "relevant keys", pdist),
               "rank_rows": timed("relevant keys", sehip.rank_rows), "count_preceding": timed("counting", sehip.count_preceding),
               "count_to_positions": timed("scan + reduce", sehip.count_to_positions),
               "recall_precision_reduce": timed("scan + reduce", sehip.recall_precision_reduce)}
    for rep in range(0 if args.whole_only else 2):                         # the first call pays allocations and the ranking probe
        phases.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            levels, means, mAP, _ = recall_precision_device(fq, q_lab, normalize=True, gallery=fg, gallery_labels=g_lab, kernels=kernels)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        print("  run %d: wall %.3f s, mAP %.4f, %d levels" % (rep, wall, mAP, len(levels)))
        for name in ("relevant keys", "distance slabs", "counting", "scan + reduce"):
            ms = sum(a.elapsed_time(b) for a, b in phases.get(name, []))
            extra = ""
            if name == "counting":
                extra = "  slab read %.1f GB -> %.2f TB/s" % (4.0 * q * n / 1e9, 4.0 * q * n / ms / 1e9) if ms > 0 else ""
            if name == "distance slabs":
                extra = "  %.1f TFLOP/s, slab write %.1f GB" % (2.0 * q * n * d / ms / 1e9, 4.0 * q * n / 1e9) if ms > 0 else ""
            print("    %-15s %10.2f ms in %6d calls%s" % (name, ms, len(phases.get(name, [])), extra))
    bench_qg_whole_list(args, fq, fg, q_lab, g_lab, timed, phases)


def bench_qg_whole_list(args, fq, fg, q_lab, g_lab, timed, phases):
    """Whole-list phase of the qg leg: every query ranked against the whole gallery (rank_gallery=True: un-clipped AHP + AP from one
    ranking), per phase and as wall time, next to the clipped path (fused top-k lists for P@k / AHP@250, counted AP)."""
    import tempfile
    from class_hierarchy import ClassHierarchy
    edges = np.load(os.path.join(ROOT, "tests", "golden", "hierarchy_cifar.npz"))["edges"]
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        for p, c in edges.tolist():
            f.write("%d %d\n" % (p, c))
        f.flush()
        hier = ClassHierarchy.from_file(f.name, id_type=int)
    q, n = int(fq.shape[0]), int(fg.shape[0])
    rows = min(q, args.whole_rows or q)
    scale = q / rows
    q_lab, g_lab = [c % 100 for c in q_lab[:rows]], [c % 100 for c in g_lab]      # the taxonomy has 100 leaves
    g_ids = [("g", j) for j in range(n)]
    kw = dict(ids=list(range(rows)), gallery=fg, gallery_labels=dict(zip(g_ids, g_lab)), gallery_ids=g_ids, normalize=True, per_query=False)
    ks = [1, 10, 50, 100]
    print("whole-list phase: %d of %d queries x %d gallery items, %d classes%s" % (rows, q, n, len(set(g_lab)), "" if rows == q else
                                                                                   " (times below are for %d rows; x %.1f for all)" % (rows, scale)))
    # both paths run as a user's call runs them (kernels=None): the entry points are timed by wrapping sehip's attributes, which the
    # host code looks up at call time
    slab = lambda a, b=None, out=None, **k: "distances" if out is not None else "relevant keys"       # noqa: E731
    patched = {"pairwise_dist": timed(slab, sehip.pairwise_dist), "rank_rows": timed(lambda pd, **k: "ranking" if k.get("out") is not None else "relevant keys", sehip.rank_rows),
               "hierarchical_precision": timed("metrics", sehip.hierarchical_precision), "retrieve_topk": timed("fused top-k", sehip.retrieve_topk),
               "count_preceding": timed("counting", sehip.count_preceding), "count_to_positions": timed("scan + reduce", sehip.count_to_positions),
               "recall_precision_reduce": timed("scan + reduce", sehip.recall_precision_reduce)}
    legs = (("whole list, rank_gallery=True (AHP + AP)", dict(compute_ahp=True, rank_gallery=True), ("distances", "ranking", "metrics")),
            ("clipped, top-k + counting (AHP@250 + AP)", dict(compute_ahp=250),
             ("fused top-k", "metrics", "relevant keys", "distances", "counting", "scan + reduce")))
    originals = {k: getattr(sehip, k) for k in patched}
    for k, v in patched.items():
        setattr(sehip, k, v)
    try:
        _qg_whole_list_legs(legs, hier, fq, rows, n, q_lab, ks, kw, phases)
    finally:
        for k, v in originals.items():
            setattr(sehip, k, v)


def _qg_whole_list_legs(legs, hier, fq, rows, n, q_lab, ks, kw, phases):
    import time
    import warnings
    for title, more, names in legs:
        for rep in range(2):
            phases.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                try:
                    means, _ = hier.hierarchical_precision_device(fq[:rows], q_lab, ks, compute_ap=True, **kw, **more)
                except ValueError as e:                                    # the memory estimate does not admit this shape
                    print("  %s: refused -- %s" % (title, e))
                    break
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            ahp = [k for k in means if k.startswith("AHP") and k.endswith("(WUP)")][0]
            print("  %s, run %d: wall %.3f s, %s %.4f, AP %.4f" % (title, rep, wall, ahp, means[ahp], means["AP"]))
            tot = 0.0
            for name in names:
                ms = sum(a.elapsed_time(b) for a, b in phases.get(name, []))
                tot += ms
                extra = ""
                if name == "ranking" and ms > 0:
                    extra = "  %.1f GB of distances in, as many of ranks out -> %.2f TB/s" % (4.0 * rows * n / 1e9, 8.0 * rows * n / ms / 1e9)
                if name == "metrics" and ms > 0 and more.get("rank_gallery"):
                    extra = "  %.1f GB of ranks read -> %.2f TB/s" % (4.0 * rows * n / 1e9, 4.0 * rows * n / ms / 1e9)
                print("    %-15s %10.2f ms in %6d calls%s" % (name, ms, len(phases.get(name, [])), extra))
            print("    %-15s %10.2f ms" % ("timed kernels", tot))


if __name__ == "__main__":
    main()
