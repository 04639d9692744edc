#!/usr/bin/env python
"""Every retrieval / loss / optimizer / input-pipeline entry point under two-stream contention: result of a call made while a second stream keeps the CUs busy
== result of the same call made alone, bit for bit.

Round 4 found se_topk_rows returning unsorted rows whenever another stream's kernels shared its CUs (a work-group barrier compiled
without the LDS wait); no single-stream test could see that.  This runs each entry point `iters` times with
three kinds of side work (distance tiles: MFMA + LDS; rankings: LDS atomics; top-k selects: barrier-dense) and compares with the
solo result.  Solo results themselves are what the GPU parity tests hold against the oracle.

    python tools/stress_streams.py [iters]          # exit 1 on any difference
"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "semantic-embeddings_amd"), ROOT):
    sys.path.insert(0, p)
import sehip

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
f32 = lambda *s: rng.standard_normal(s).astype(np.float32)

# ---- inputs ----
g20 = dev(f32(20000, 100)); sehip.normalize_rows_(g20)
g3 = dev(f32(3001, 200)); sehip.normalize_rows_(g3)
gw = dev(f32(20000, 320)); sehip.normalize_rows_(gw)              # padded width 384: the 256 x 256 LDS-DMA filter kernel
raw = dev(f32(8192, 1000))
sq20 = sehip.row_sqnorm(g20)
pd_short = sehip.pairwise_dist(g3[:512], g3)                       # 3001 columns: short-row instantiations
pd_mid = sehip.pairwise_dist(g20[:1024], g20)                      # 20,000 columns
gl = dev(f32(60000, 64)); sehip.normalize_rows_(gl)
pd_long = sehip.pairwise_dist(gl[:256], gl)                        # 60,000 columns: two sorted runs + merge
C = 100
cls = dev(rng.integers(0, C, size=20000).astype(np.int32))
tab = rng.random((C, C)); tab = (tab + tab.T) / 2; np.fill_diagonal(tab, 1.0)
counts = np.bincount(cls.cpu().numpy(), minlength=C)
best = np.stack([np.cumsum(np.repeat(tab[c][np.argsort(-tab[c], kind="stable")], counts[np.argsort(-tab[c], kind="stable")])) for c in range(C)])
tab_d, best_d = dev(tab), dev(best)
rk_mid = sehip.rank_rows(pd_mid)
g64 = g20[:4096].double()                                           # float64 retrieval: distances + image, ranking + run repair
pd64, img64 = sehip.pairwise_dist_f64(g64[:1024], g64)
pd64[:, 100:1300] = 1.0 + pd64[:, 100:1300] * 2.0 ** -30; img64 = pd64.float()   # 1,200 columns of image 1.0f: a run beyond the LDS sort
ks = torch.arange(1, 251, dtype=torch.int32, device="cuda")
qidx = torch.arange(1024, dtype=torch.int32, device="cuda")
curves = sehip.hprec_reciprocal_curves(best_d, best_d)
nd_disc = sehip.ndcg_discounts(20000, "cuda")
nd_one = sehip.ndcg_ideal(tab_d, counts, nd_disc, ks.tolist(), full=True)
nd_ideal = torch.stack([nd_one, nd_one], dim=2).contiguous()
cr_len = dev(rng.integers(0, 251, size=1024).astype(np.int32))       # se_complete_rankings: ragged top-250 lists, a shuffled all_ids order
cr_order = dev(rng.permutation(20000).astype(np.int32))
emb = dev(f32(C, 100)); sehip.normalize_rows_(emb)
xb = dev(f32(4096, 100)); yb = dev(rng.integers(0, C, size=4096).astype(np.int64))
emb_wide = dev(f32(1000, 100)); sehip.normalize_rows_(emb_wide)      # 32 class tiles: the embedding head cuts them into slices
parts = torch.stack([torch.stack([sehip.topk_rows(pd_mid[:, i * 2500:(i + 1) * 2500].contiguous(), 251, col_offset=i * 2500)[j].view(torch.int32)
                                  for j in (0, 1)]) for i in range(8)])     # [8, 2, Q, k] packed lists

# a batch of the file-dataset input pipeline: 32 images of 96 x 128 .. 200 x 260 noise, random zoom 64-120, crop 56 x 56, erasing
from datasets.files import DEFAULT_ERASE_PARAMS, FileDatasetGenerator, pack_batch_tables
img_gen = FileDatasetGenerator(".", cropsize=(56, 56), default_target_size=64, randzoom_range=(64, 120), randerase_prob=0.5, randerase_params=DEFAULT_ERASE_PARAMS)
img_sizes = np.stack((rng.integers(96, 200, 32), rng.integers(128, 260, 32)), axis=1).astype(np.int32)
img_bytes = img_sizes[:, 0].astype(np.int64) * img_sizes[:, 1] * 3
img_arena = dev(rng.integers(0, 256, int(img_bytes.sum()), dtype=np.uint8))
img_buf, img_views = pack_batch_tables(np.concatenate(([0], np.cumsum(img_bytes)[:-1])), img_sizes, img_gen.draw_params(img_sizes, True, True, rng), (56, 56))
img_dbuf = dev(img_buf)
img_t = {k: (img_dbuf[a:b].view(torch.int64) if k == "src_off" else img_dbuf[a:b].view(shape)) for k, (a, b, shape) in img_views.items()}
img_stats = (dev(np.float32([125.3, 129.7, 118.5])), dev(np.float32([57.0, 56.7, 68.4])))

# one Adagrad step over 3,000,005 parameters (two trips of the grid-stride loop and a tail), regulariser and scale folded in
ag_p, ag_a, ag_g = dev(f32(3000005)), dev(np.abs(f32(3000005))), dev(f32(3000005))
ag_l2 = dev(np.full(3000005, 4e-4, dtype=np.float32))
# the fused SGD pair over the same buffers: norm + clip factor (a workgroup reduction and a finalising wave), then the update
sgd_ws = torch.empty(sehip.SGD_MAX_BLOCKS * 8, dtype=torch.uint8, device="cuda")


def sgd_pair(p, v):
    stats = sehip.grad_clip_factor(ag_g, p, ag_l2, grad_scale=0.5, clipnorm=10.0, workspace=sgd_ws)
    sehip.sgd_step_(p, v, ag_g, ag_l2, lr=0.01, grad_scale=0.5, clip=stats[1:], momentum=0.9, nesterov=True)
    return p, v, stats


zb = dev(f32(4096, C) * 3)                                         # logits: a wave per row
zb_wide = dev(f32(512, 1000) * 3)


def joint_step(p, table, z, metric):
    """one se_joint_head_fwd and one se_joint_head_bwd through autograd"""
    p, z = p.detach().requires_grad_(True), z.detach().requires_grad_(True)
    out = sehip.joint_head(p, yb[:p.shape[0]], table, logits=z, metric=metric)
    dp, dz = torch.autograd.grad(out.emb_loss_i.sum() + 0.1 * out.cls_loss_i.sum(), (p, z))
    return tuple(t.detach() for t in out if t is not None) + (dp, dz)


def as_tuple(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


OPS = {
    "normalize_rows_": lambda: sehip.normalize_rows_(raw.clone()),
    "row_sqnorm": lambda: sehip.row_sqnorm(raw),
    "pairwise_dist cosine symmetric": lambda: sehip.pairwise_dist(g20[:4096], g20[:4096]),
    "pairwise_dist Euclid general": lambda: sehip.pairwise_dist(g20[:2048], g20, metric=sehip.METRIC_EUCLID, sqa=sq20[:2048], sqb=sq20),
    "rank_rows 3,001 columns": lambda: sehip.rank_rows(pd_short),
    "rank_rows 20,000 columns": lambda: sehip.rank_rows(pd_mid),
    "rank_rows 60,000 columns (runs + merge)": lambda: sehip.rank_rows(pd_long),
    "pairwise_dist_f64 cosine": lambda: sehip.pairwise_dist_f64(g64[:2048], g64),
    "rank_rows_f64 (image ranking + run repair)": lambda: sehip.rank_rows_f64(pd64, img64),
    "topk_rows k=251": lambda: sehip.topk_rows(pd_mid, 251),
    "topk_rows k=1000": lambda: sehip.topk_rows(pd_mid, 1000),
    "topk_merge packed 8 parts": lambda: sehip.topk_merge(parts),
    "retrieve_topk fused cosine": lambda: sehip.retrieve_topk(g20[:4096], g20, 251),
    "retrieve_topk fused Euclid": lambda: sehip.retrieve_topk(g20[:4096], g20, 100, metric=sehip.METRIC_EUCLID, sqq=sq20[:4096], sqg=sq20),
    "retrieve_topk fused, long rows (LDS-DMA)": lambda: sehip.retrieve_topk(gw[:4096], gw, 251),
    "retrieve_topk slab (3,001 rows)": lambda: sehip.retrieve_topk(g3[:512], g3, 64),
    "hierarchical_precision": lambda: sehip.hierarchical_precision(rk_mid, cls, cls[:1024].contiguous(), qidx, tab_d, tab_d, best_d, best_d, ks,
                                                                     ahp_len=0, want_ap=True, curves=curves),
    "ndcg": lambda: sehip.ndcg(rk_mid, cls, cls[:1024].contiguous(), qidx, tab_d, tab_d, nd_disc, nd_ideal, ks, want_full=True),
    "knn_vote (LDS vote tables)": lambda: sehip.knn_vote(rk_mid[:, :201], cls, C, [1, 5, 20, 200], top=5, qidx=qidx),
    "complete_rankings (LDS bitmap, ragged)": lambda: sehip.complete_rankings(rk_mid[:, :250], 20000, lengths=cr_len, order=cr_order),
    "complete_rankings (whole lists)": lambda: sehip.complete_rankings(rk_mid, 20000),
    "cosine_loss fwd+bwd": lambda: (sehip.cosine_loss_forward(xb, yb, emb)[0], sehip.cosine_loss_backward(xb, yb, emb)),
    "nn_accuracy": lambda: sehip.nn_accuracy(xb, yb, emb, dot_prod_sim=True, k=5),
    "embed_head cosine": lambda: sehip.embed_head_forward(xb, yb, emb, mode="cosine", want_best=True),
    "embed_head sqdist, class slices": lambda: sehip.embed_head_forward(xb[:512], yb[:512], emb_wide, mode="sqdist", want_dist=True, want_best=True),
    "joint_head nearest fwd+bwd": lambda: joint_step(xb, emb, zb, "nearest"),
    "joint_head nearest, class slices": lambda: joint_step(xb[:512], emb_wide, zb_wide, "nearest"),
    "joint_head argmax, one-hot": lambda: joint_step(zb, None, zb, "argmax"),
    "devise_ranking_loss": lambda: sehip.devise_ranking_loss(xb, yb, emb),
    "image_batch": lambda: sehip.image_batch(img_arena, img_t["src_off"], img_t["src_hw"], img_t["xmap"], img_t["xk"], img_t["ymap"], img_t["yk"],
                                             img_t["erase"], img_t["seed"], img_stats[0], img_stats[1]),
    "adagrad_step_": lambda: (lambda p, acc: (sehip.adagrad_step_(p, acc, ag_g, ag_l2, lr=0.01, grad_scale=0.5), acc))(ag_p.clone(), ag_a.clone()),
    "grad_clip_factor": lambda: sehip.grad_clip_factor(ag_g, ag_p, ag_l2, grad_scale=0.5, clipnorm=10.0, workspace=sgd_ws),
    "grad_clip_factor + sgd_step_": lambda: sgd_pair(ag_p.clone(), ag_a.clone()),
}
SIDE = {
    "distance tiles": lambda: sehip.pairwise_dist(g20[:6000], g20[:6000]),
    "rankings": lambda: sehip.rank_rows(pd_mid[:256]),
    "top-k selects": lambda: sehip.topk_rows(pd_mid[:512], 251),
}

side = torch.cuda.Stream()
failed = 0
for name, op in OPS.items():
    torch.cuda.synchronize()
    want = [t.clone() for t in as_tuple(op()) if torch.is_tensor(t)]
    torch.cuda.synchronize()
    again = [t for t in as_tuple(op()) if torch.is_tensor(t)]
    torch.cuda.synchronize()
    if not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(want, again)):
        print("%-42s NOT deterministic alone -- skipped" % name); continue
    line = "%-42s" % name
    for sname, noise in SIDE.items():
        bad = 0
        for it in range(iters):
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    noise()
            got = [t for t in as_tuple(op()) if torch.is_tensor(t)]
            bad += not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(want, got))
        torch.cuda.synchronize()
        line += "  %s: %d/%d differ" % (sname, bad, iters)
        failed += bad
    print(line, flush=True)
print("stress_streams: %d differing calls" % failed)
sys.exit(1 if failed else 0)
