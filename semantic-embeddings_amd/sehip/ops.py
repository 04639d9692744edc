"""Torch-facing wrappers of the HIP hot path (device tensors in, device tensors out).

Every function here calls straight through the C ABI of libsehip.so on the current torch stream (``_lib.call``: the declarations
come from include/sehip.h); PyTorch only provides device memory, streams and autograd plumbing.  Reference citations are into
the cvjena/semantic-embeddings checkout.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from ._lib import DEFINES, DTYPE_BF16, DTYPE_F32, METRIC_COSINE, METRIC_DOT, METRIC_EUCLID, SehipError, call, require_gpu

__all__ = [
    "cosine_embedding_loss", "cosine_loss_forward", "cosine_loss_backward", "squared_distance_loss", "sqdist_loss_forward",
    "sqdist_loss_backward", "center_loss", "softmax_cross_entropy", "hierarchical_cross_entropy", "soft_label_cross_entropy", "HxeEncoding", "SoftLabelTable", "TreeRiskEncoding", "tree_risk_topk", "TREE_RISK_TOP_MAX", "TREE_RISK_MAX_CLASSES", "l2norm", "nn_accuracy", "embed_head_forward", "embedding_head", "joint_head", "labelembed_loss", "labelembed_table_loss", "labelembed_table_loss_packed", "LE_GRID_CAP",
    "devise_ranking_loss", "DEVISE_TORCH_ABOVE",
    "adagrad_step_", "ADAGRAD_MAX_BLOCKS", "grad_clip_factor", "sgd_step_", "SGD_MAX_BLOCKS", "shortcut_add", "LAYOUT_NCHW", "LAYOUT_NHWC",
    "row_sqnorm", "normalize_rows_", "empty_rows", "pairwise_dist", "rank_rows_init", "workspace_bytes", "release_workspace",
    "phase_timing", "phase_timing_read", "rank_rows_workspace_bytes", "RANK_U16_MAX_N", "rank_rows", "rank_rows_check", "pairwise_dist_f64",
    "rank_refine_f64_", "rank_rows_f64", "topk_rows",
    "topk_merge", "retrieve_topk", "knn_vote", "KNN_TOP_MAX", "bootstrap_means", "bootstrap_indices", "BOOTSTRAP_COLS_MAX", "complete_rankings", "COMPLETE_LDS_ITEMS", "HprecCurves", "hprec_reciprocal_curves", "hierarchical_precision", "ndcg_discounts", "ndcg_ideal", "ndcg", "NDCG_CHUNK", "relevant_positions",
    "recall_precision_reduce", "count_preceding", "count_to_positions", "svm_margin", "svm_loss_blocks", "svm_reduce_workspace_bytes", "svm_reduce", "svm_gram", "svm_rowsum",
    "svm_axpby", "class_pair_tables", "cholesky_lower_", "eigh", "eigh_schedule", "EIGH_NOT_CONVERGED", "EIGH_NONFINITE", "image_batch", "resample_tables", "tiny_batch", "TINY_BATCH_MAX_BLOCKS", "FILL_MODES",
    "METRIC_COSINE", "METRIC_EUCLID", "METRIC_DOT",
]


# --------------------------------------------------------------------------------------------
# argument helpers
# --------------------------------------------------------------------------------------------

def _device_index(device=None):
    """Ordinal of a CUDA ``device``; None or a device without an index is the current device."""
    index = None if device is None else torch.device(device).index
    return torch.cuda.current_device() if index is None else index


def _dtype_code(t):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise SehipError("features must be float32 or bfloat16, got %s" % t.dtype)
    return DTYPE_F32 if t.dtype == torch.float32 else DTYPE_BF16


_RANK_WIDTH_CODES = {torch.int32: 0, torch.int64: 1, torch.int16: 2}


def _rank_width_code(t):
    """Index width code of se_rank_rows / se_rank_rows_check for a rank tensor: int32 -> 0, int64 -> 1, int16 (the BIT PATTERN of
    uint16 gallery indices: torch has no full uint16) -> 2."""
    if t.dtype not in _RANK_WIDTH_CODES:
        raise SehipError("ranks must be int32, int64 or int16 (uint16 bit patterns), not %s" % t.dtype)
    return _RANK_WIDTH_CODES[t.dtype]


def _kblocks_arg(kblocks):
    if kblocks is None or len(kblocks) <= 1:
        return None, 0
    return (ctypes.c_int32 * len(kblocks))(*[int(v) for v in kblocks]), len(kblocks)


def _rows(t, what):
    if t.dim() != 2 or t.stride(1) != 1:
        raise SehipError("%s must be a 2-d tensor with contiguous rows" % what)
    return t


def _f32_rows(t, what):
    if t.dtype != torch.float32:
        raise SehipError("%s must be float32" % what)
    return _rows(t, what)


def _i32(t, name):
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise SehipError("%s must be contiguous int32" % name)


def _i64(t, name):
    if t.dtype != torch.int64 or not t.is_contiguous():
        raise SehipError("%s must be contiguous int64" % name)


def _check_curves(*tables):
    for t in tables:
        if t.dtype != torch.float64 or t.dim() != 2 or t.stride(1) != 1:
            raise SehipError("the similarity tables / best curves must be float64 matrices with contiguous rows")


def _f32_2d(t, name, min_cols):
    if t is None or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.shape[1] < min_cols:
        raise SehipError("%s must be a 2-d float32 tensor with contiguous rows and >= %d columns" % (name, min_cols))
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _class_loss_shapes(x, labels, embedding):
    """(B, D, C) of a loss of the rows of x [B, D] against embedding[labels]: embedding float32 [C, D], labels contiguous int64 [B]."""
    _rows(x, "x"); _rows(embedding, "embedding")
    B, D = x.shape
    if embedding.shape[1] != D or embedding.dtype != torch.float32:
        raise SehipError("embedding must be float32 [C, %d]" % D)
    if labels.dtype != torch.int64 or labels.numel() != B or not labels.is_contiguous():
        raise SehipError("labels must be a contiguous int64 [B] tensor")
    return B, D, embedding.shape[0]


# --------------------------------------------------------------------------------------------
# training side
# --------------------------------------------------------------------------------------------

def cosine_loss_forward(x, labels, embedding, want_xhat=True):
    """Fused l2norm + gather + inv_correlation (+ batch mean).

    reference: utils.l2norm (utils.py:125-127), transform_inputs (learn_image_embeddings.py:48-50),
    utils.inv_correlation (utils.py:44-46).  Returns (xhat | None, inv_norm, loss_i, loss_mean)."""
    require_gpu(x, labels, embedding)
    B, D, C = _class_loss_shapes(x, labels, embedding)
    xhat = torch.empty((B, D), dtype=torch.float32, device=x.device) if want_xhat else None
    inv_norm = torch.empty((B,), dtype=torch.float32, device=x.device)
    loss_i = torch.empty((B,), dtype=torch.float32, device=x.device)
    loss_mean = torch.empty((1,), dtype=torch.float32, device=x.device)
    call("se_cosine_loss_fwd", x, _dtype_code(x), x.stride(0), labels, embedding, embedding.stride(0), B, D, C, xhat, D, inv_norm,
         loss_i, loss_mean)
    return xhat, inv_norm, loss_i, loss_mean


def _class_loss_backward(entry, x, labels, embedding, grad_loss_i, grad_scale, out_dtype):
    require_gpu(x, labels, embedding, grad_loss_i)
    B, D, C = _class_loss_shapes(x, labels, embedding)
    dx = torch.empty((B, D), dtype=out_dtype or x.dtype, device=x.device)
    if grad_loss_i is not None:
        grad_loss_i = grad_loss_i.to(torch.float32).contiguous()
    call(entry, x, _dtype_code(x), x.stride(0), labels, embedding, embedding.stride(0), grad_loss_i, float(grad_scale), B, D, C, dx,
         _dtype_code(dx), D)
    return dx


def cosine_loss_backward(x, labels, embedding, grad_loss_i=None, grad_scale=1.0, out_dtype=None):
    """Closed-form backward of cosine_loss_forward w.r.t. x (what TF autodiff derives from
    utils.py:44-46,125-127)."""
    return _class_loss_backward("se_cosine_loss_bwd", x, labels, embedding, grad_loss_i, grad_scale, out_dtype)


def _check_loss_inputs(labels, embedding, what):
    """The loss kernels gather ``embedding[label]`` with the label CLAMPED to [0, C - 1] (a device kernel cannot raise the IndexError
    the reference's ``embedding[y]`` gather would), and they return no gradient for the class-embedding table (it is a precomputed
    constant in the reference: learn_image_embeddings.py:48-50).  ``SEHIP_CHECK_LABELS=1`` validates the labels on the host
    (one synchronising min / max per call: a debugging aid); a table that asks for a gradient is refused always."""
    if embedding.requires_grad:
        raise SehipError("%s: the class-embedding table is a constant of this loss (no gradient is computed for it); detach() it" % what)
    _check_labels(labels, embedding, what)


def _check_labels(labels, embedding, what):
    """``SEHIP_CHECK_LABELS=1``: the labels must index rows of ``embedding`` (one synchronising min / max)."""
    if os.environ.get("SEHIP_CHECK_LABELS"):
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= embedding.shape[0]:
            raise IndexError("%s: labels span [%d, %d] but the embedding table has %d rows" % (what, lo, hi, embedding.shape[0]))


class _CosineEmbeddingLoss(torch.autograd.Function):
    """Per-sample loss_i = 1 - <l2norm(x_i), E[y_i]> with the HIP forward/backward; also returns
    the normalised features the forward kernel produces anyway (non-differentiable by-product)."""

    @staticmethod
    def forward(ctx, x, labels, embedding, want_xhat):
        _check_loss_inputs(labels, embedding, "cosine_embedding_loss")
        x = x if x.stride(-1) == 1 else x.contiguous()
        xhat, _, loss_i, _ = cosine_loss_forward(x, labels, embedding, want_xhat=want_xhat)
        ctx.save_for_backward(x, labels, embedding)
        if xhat is None:
            xhat = loss_i.new_empty(0)
        ctx.mark_non_differentiable(xhat)
        return loss_i, xhat

    @staticmethod
    def backward(ctx, grad_loss_i, _grad_xhat):
        x, labels, embedding = ctx.saved_tensors
        dx = cosine_loss_backward(x, labels, embedding, grad_loss_i.contiguous())
        return dx, None, None, None


def cosine_embedding_loss(x, labels, embedding, reduction="mean", return_normalized=False):
    """Differentiable cosine-embedding loss on un-normalised features ``x`` [B, D].

    Equivalent to the reference's ``Lambda(utils.l2norm)`` head followed by
    ``utils.inv_correlation(embedding[y], .)`` and Keras' batch mean.  With ``return_normalized``
    the L2-normalised features (what the reference's model outputs) are returned as well."""
    loss_i, xhat = _CosineEmbeddingLoss.apply(x, labels, embedding, bool(return_normalized))
    if reduction == "mean":
        loss_i = loss_i.mean()
    elif reduction == "sum":
        loss_i = loss_i.sum()
    return (loss_i, xhat) if return_normalized else loss_i


def sqdist_loss_forward(x, labels, embedding, want_dist=False):
    """``se_sqdist_loss_fwd``: loss_i = sum_d (x - E[y])^2 (utils.squared_distance on transform_inputs' gather, utils.py:34-36,
    learn_image_embeddings.py:48-50) and, on request, dist_i = sqrt(loss_i) (utils.mean_distance, utils.py:39-41).
    Returns (loss_i, dist_i | None, loss_mean)."""
    require_gpu(x, labels, embedding)
    B, D, C = _class_loss_shapes(x, labels, embedding)
    loss_i = torch.empty((B,), dtype=torch.float32, device=x.device)
    dist_i = torch.empty((B,), dtype=torch.float32, device=x.device) if want_dist else None
    loss_mean = torch.empty((1,), dtype=torch.float32, device=x.device)
    call("se_sqdist_loss_fwd", x, _dtype_code(x), x.stride(0), labels, embedding, embedding.stride(0), B, D, C, loss_i, dist_i,
         loss_mean)
    return loss_i, dist_i, loss_mean


def sqdist_loss_backward(x, labels, embedding, grad_loss_i=None, grad_scale=1.0, out_dtype=None):
    """``se_sqdist_loss_bwd``: dx = 2 w (x - E[y])."""
    return _class_loss_backward("se_sqdist_loss_bwd", x, labels, embedding, grad_loss_i, grad_scale, out_dtype)


class _SquaredDistanceLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, embedding):
        _check_loss_inputs(labels, embedding, "squared_distance_loss")
        x = x if x.stride(-1) == 1 else x.contiguous()
        loss_i, _, _ = sqdist_loss_forward(x, labels, embedding)
        ctx.save_for_backward(x, labels, embedding)
        return loss_i

    @staticmethod
    def backward(ctx, grad_loss_i):
        x, labels, embedding = ctx.saved_tensors
        return sqdist_loss_backward(x, labels, embedding, grad_loss_i.contiguous()), None, None


def squared_distance_loss(x, labels, embedding, reduction="none"):
    """Differentiable ``utils.squared_distance(embedding[labels], x)`` (the `--loss mse` training loss) in one HIP launch forward,
    one backward; ``reduction``: "none" (Keras-style per-sample tensor), "mean" or "sum"."""
    loss_i = _SquaredDistanceLoss.apply(x, labels, embedding)
    if reduction == "mean":
        return loss_i.mean()
    if reduction == "sum":
        return loss_i.sum()
    return loss_i


class _CenterLoss(torch.autograd.Function):
    """reference: the center loss of learn_center_loss.py:35-39, sum_d (x - c[y])^2 / 2, and what TF autodiff derives from it for the
    features and the (learned) centroids.  Halving is exact, so the forward pass is 0.5 * se_sqdist_loss_fwd and the feature gradient
    se_sqdist_loss_bwd with the weights w / 2 (2 (w / 2) = w); the centroid gradient is se_center_loss_centroid_grad."""

    @staticmethod
    def forward(ctx, x, labels, centroids):
        require_gpu(x, labels, centroids)
        x = x if x.stride(-1) == 1 else x.contiguous()
        B, D, C = _class_loss_shapes(x, labels, centroids)
        _check_labels(labels, centroids, "center_loss")
        loss_i = torch.empty((B,), dtype=torch.float32, device=x.device)
        call("se_sqdist_loss_fwd", x, _dtype_code(x), x.stride(0), labels, centroids, centroids.stride(0), B, D, C, loss_i, None, None)
        ctx.save_for_backward(x, labels, centroids)
        return loss_i.mul_(0.5)

    @staticmethod
    def backward(ctx, grad_loss_i):
        x, labels, centroids = ctx.saved_tensors
        B, D, C = _class_loss_shapes(x, labels, centroids)
        g = grad_loss_i.to(torch.float32).contiguous()
        dx = dc = None
        if ctx.needs_input_grad[0]:
            dx = sqdist_loss_backward(x, labels, centroids, g * 0.5)
        if ctx.needs_input_grad[2]:
            dc = torch.empty((C, D), dtype=torch.float32, device=x.device)
            call("se_center_loss_centroid_grad", x, _dtype_code(x), x.stride(0), labels, centroids, centroids.stride(0), g, 0.0, B, D, C,
                 dc, D)
        return dx, None, dc


def center_loss(x, labels, centroids, reduction="none"):
    """Differentiable center loss (Wen et al.; learn_center_loss.py:35-39): sum_d (x - centroids[labels])^2 / 2 per row of ``x``
    [B, D] (float32 or bfloat16; ``dx`` in x's dtype), labels contiguous int64 [B] (clamped to [0, C - 1] like every loss gather;
    ``SEHIP_CHECK_LABELS=1`` checks them), centroids float32 [C, D] -- learned (``requires_grad``: its gradient is the fixed-order
    per-class sum of se_center_loss_centroid_grad) or fixed.  ``reduction``: "none" (per-sample [B]), "mean" or "sum"."""
    loss_i = _CenterLoss.apply(x, labels, centroids)
    if reduction == "mean":
        return loss_i.mean()
    if reduction == "sum":
        return loss_i.sum()
    return loss_i


class _SoftmaxCrossEntropy(torch.autograd.Function):
    """reference: Keras 2.2's 'categorical_crossentropy' on the softmax output against transform_inputs' smoothed one-hot target
    (learn_classifier.py:17-22, 116-117, 146-147), 'accuracy' and utils.top_k_acc (utils.py:49-54) of the same scores: one
    se_softmax_xent_fwd; the gradient with respect to the logits is one se_softmax_xent_bwd."""

    @staticmethod
    def forward(ctx, logits, labels, smoothing, want_mean):
        require_gpu(logits, labels)
        if logits.dim() != 2:
            raise SehipError("logits must be a 2-d [B, C] tensor")
        B, C = logits.shape
        z = logits if logits.stride(1) == 1 and (B <= 1 or logits.stride(0) >= C) else logits.contiguous()
        if labels.dtype != torch.int64 or labels.numel() != B or not labels.is_contiguous():
            raise SehipError("labels must be a contiguous int64 [B] tensor")
        if os.environ.get("SEHIP_CHECK_LABELS") == "1" and B and (int(labels.min()) < 0 or int(labels.max()) >= C):
            raise SehipError("softmax_cross_entropy: labels outside [0, %d)" % C)
        dev = z.device
        loss_i = torch.empty((B,), dtype=torch.float32, device=dev)
        aux = torch.empty((call("se_softmax_xent_aux_floats", B),), dtype=torch.float32, device=dev)
        best = torch.empty((B,), dtype=torch.int32, device=dev)
        above = torch.empty((B,), dtype=torch.int32, device=dev)
        loss_mean = torch.empty((1,), dtype=torch.float32, device=dev) if want_mean else None
        ldz = z.stride(0) if B > 1 else max(z.stride(0), C)
        call("se_softmax_xent_fwd", z, _dtype_code(z), ldz, labels, B, C, float(smoothing), loss_i, aux, best, above, loss_mean)
        ctx.save_for_backward(z, labels, aux)
        ctx.smoothing, ctx.ldz = float(smoothing), ldz
        ctx.mark_non_differentiable(best, above)
        if want_mean:
            return loss_i, best, above, loss_mean
        return loss_i, best, above

    @staticmethod
    def backward(ctx, grad_loss_i, _best, _above, grad_mean=None):
        z, labels, aux = ctx.saved_tensors
        B, C = z.shape
        g = grad_loss_i.to(torch.float32)
        if grad_mean is not None:           # d mean / d loss_i = 1 / B
            g = g + grad_mean.to(torch.float32) / max(B, 1)
        dz = torch.empty((B, C), dtype=z.dtype, device=z.device)
        call("se_softmax_xent_bwd", z, _dtype_code(z), ctx.ldz, labels, aux, g.contiguous(), 0.0, B, C, ctx.smoothing, dz, _dtype_code(dz), C)
        return dz, None, None, None


def softmax_cross_entropy(logits, labels, label_smoothing=0.0, reduction="none", return_metrics=False):
    """Differentiable categorical cross-entropy of ``softmax(logits)`` as Keras 2.2 computes it (probabilities clipped to
    [1e-7, 1 - 1e-7]: a sample's loss is capped at 16.118 and a class whose probability left the range gets no gradient), against the
    target ``1 - label_smoothing`` for the label and ``label_smoothing / (C - 1)`` for every other class (one-hot unless
    ``0 < label_smoothing < 1``, the reference's rule): one HIP launch forward, one backward.
    logits [B, C] float32 or bfloat16 with any row pitch (``d logits`` in the same dtype), labels contiguous int64 [B] (clamped to
    [0, C - 1]; ``SEHIP_CHECK_LABELS=1`` checks them).  ``reduction``: "none" (per-sample [B]), "mean" (the kernel's fixed-order
    mean) or "sum".  With ``return_metrics`` the result is ``(loss, best, above)``: int32 [B] arg-max class of every row (lowest
    index on ties) and the number of classes scoring strictly above the label's -- ``best == labels`` is Keras' accuracy,
    ``above < k`` is ``tf.nn.in_top_k``."""
    if reduction not in ("none", "mean", "sum"):
        raise SehipError("reduction must be none, mean or sum, got %r" % (reduction,))
    out = _SoftmaxCrossEntropy.apply(logits, labels, float(label_smoothing), reduction == "mean")
    loss = out[3][0] if reduction == "mean" else (out[0].sum() if reduction == "sum" else out[0])
    return (loss, out[1], out[2]) if return_metrics else loss


class HxeEncoding(object):
    """``ClassHierarchy.hxe_encoding``'s arrays for the kernels: uploaded once per device and kept on this object; ``path_off``
    also stays on the host, where the entry points check it before every launch."""

    def __init__(self, encoding):
        import numpy as np
        self.host = {k: torch.from_numpy(np.ascontiguousarray(encoding[k], dtype=np.float32 if k == "lvl_w" else np.int32))
                     for k in ("pos", "path_off", "lvl_lo", "lvl_hi", "lvl_w")}
        self.num_classes = int(self.host["pos"].numel())
        if self.host["path_off"].numel() != self.num_classes + 1:
            raise SehipError("hxe encoding: path_off must hold C + 1 = %d entries" % (self.num_classes + 1))
        nnz = int(self.host["path_off"][-1])
        if any(int(self.host[k].numel()) != nnz for k in ("lvl_lo", "lvl_hi", "lvl_w")):
            raise SehipError("hxe encoding: lvl_lo, lvl_hi and lvl_w must hold path_off[C] = %d entries" % nnz)
        self._device = {}

    def on(self, device):
        key = (device.type, device.index)
        if key not in self._device:
            self._device[key] = {k: v.to(device) for k, v in self.host.items()}
        return self._device[key]

    @classmethod
    def of(cls, encoding):
        """``encoding`` itself, or the object kept with the dict ``hxe_encoding`` returned (so its uploads are shared by every call)."""
        if isinstance(encoding, cls):
            return encoding
        if "_sehip" not in encoding:
            encoding["_sehip"] = cls(encoding)
        return encoding["_sehip"]


TREE_RISK_TOP_MAX = DEFINES["SE_TREE_RISK_TOP_MAX"]
TREE_RISK_MAX_CLASSES = DEFINES["SE_TREE_RISK_MAX_CLASSES"]


class TreeRiskEncoding(object):
    """``ClassHierarchy.tree_risk_encoding``'s arrays for ``se_tree_risk_topk``: uploaded once per device and kept on this object."""

    KEYS = ("pos", "path_off", "lvl_lo", "lvl_hi", "lvl_h", "own_h")

    def __init__(self, encoding):
        self.host = {k: torch.from_numpy(np.ascontiguousarray(encoding[k], dtype=np.int32)) for k in self.KEYS}
        self.num_classes = int(self.host["pos"].numel())
        if self.host["path_off"].numel() != self.num_classes + 1 or self.host["own_h"].numel() != self.num_classes:
            raise SehipError("tree risk encoding: path_off must hold C + 1 = %d entries, own_h C" % (self.num_classes + 1))
        self.nnz = int(self.host["path_off"][-1])
        if any(int(self.host[k].numel()) != self.nnz for k in ("lvl_lo", "lvl_hi", "lvl_h")):
            raise SehipError("tree risk encoding: lvl_lo, lvl_hi and lvl_h must hold path_off[C] = %d entries" % self.nnz)
        self._device = {}

    on = HxeEncoding.on

    @classmethod
    def of(cls, encoding):
        """``encoding`` itself, or the object kept with the dict ``tree_risk_encoding`` returned."""
        if isinstance(encoding, cls):
            return encoding
        if "_sehip" not in encoding:
            encoding["_sehip"] = cls(encoding)
        return encoding["_sehip"]


def tree_risk_topk(probs, encoding, top, return_risk=False):
    """Conditional risk minimisation on a class tree (``se_tree_risk_topk``; include/sehip.h states the arithmetic): for every row
    of ``probs`` (float32 [N, C] device tensor, any row pitch) the ``top`` classes of smallest expected LCS height
    ``sum_j p_j * height(lcs(k, j))`` in ascending (risk, class index) order.  ``encoding``: ``ClassHierarchy.tree_risk_encoding``
    (the dict, or a ``TreeRiskEncoding`` of it), uploaded once per device.  Returns ``(cls int32 [N, top], risk_top float64
    [N, top])`` and, with ``return_risk``, the float64 [N, C] risks of every class.  A row with a NaN or an infinity: NaN risks,
    classes ``0 .. top - 1``."""
    require_gpu(probs)
    enc = TreeRiskEncoding.of(encoding)
    if probs.dim() != 2 or probs.dtype != torch.float32:
        raise SehipError("probs must be a 2-d float32 [N, C] tensor")
    N, C = probs.shape
    if C != enc.num_classes:
        raise SehipError("tree_risk_topk: the probabilities have %d classes, the encoding %d" % (C, enc.num_classes))
    top = int(top)
    if top < 1 or top > min(C, TREE_RISK_TOP_MAX):
        raise SehipError("top must lie in [1, min(C = %d, %d)], got %d" % (C, TREE_RISK_TOP_MAX, top))
    p = probs if probs.stride(1) == 1 and (N <= 1 or probs.stride(0) >= C) else probs.contiguous()
    t = enc.on(p.device)
    cls = torch.empty((N, top), dtype=torch.int32, device=p.device)
    risk_top = torch.empty((N, top), dtype=torch.float64, device=p.device)
    risk = torch.empty((N, C), dtype=torch.float64, device=p.device) if return_risk else None
    call("se_tree_risk_topk", p, p.stride(0) if N > 1 else max(p.stride(0), C), t["pos"], t["path_off"], t["lvl_lo"], t["lvl_hi"],
         t["lvl_h"], enc.nnz, t["own_h"], N, C, top, cls, risk_top, risk, C)
    return (cls, risk_top, risk) if return_risk else (cls, risk_top)


class SoftLabelTable(object):
    """A float32 [C, C] table of target distributions (``ClassHierarchy.soft_label_table``): uploaded once per device and kept here."""

    def __init__(self, table):
        t = table if torch.is_tensor(table) else torch.from_numpy(table)
        if t.dim() != 2 or t.shape[0] != t.shape[1]:
            raise SehipError("a soft-label table is a square [C, C] matrix, got %s" % (tuple(t.shape),))
        self.host = t.to(torch.float32).contiguous()
        self.num_classes = int(t.shape[0])
        self._device = {}

    def on(self, device):
        key = (device.type, device.index)
        if key not in self._device:
            self._device[key] = self.host.to(device)
        return self._device[key]


def _logit_rows(logits, labels, C_want, what):
    require_gpu(logits, labels)
    if logits.dim() != 2:
        raise SehipError("logits must be a 2-d [B, C] tensor")
    B, C = logits.shape
    if C != C_want:
        raise SehipError("%s: the logits have %d classes, the %s %d" % (what, C, "encoding" if what.startswith("hier") else "table", C_want))
    z = logits if logits.stride(1) == 1 and (B <= 1 or logits.stride(0) >= C) else logits.contiguous()
    if labels.dtype != torch.int64 or labels.numel() != B or not labels.is_contiguous():
        raise SehipError("labels must be a contiguous int64 [B] tensor")
    if os.environ.get("SEHIP_CHECK_LABELS") == "1" and B and (int(labels.min()) < 0 or int(labels.max()) >= C):
        raise SehipError("%s: labels outside [0, %d)" % (what, C))
    return z, B, C, (z.stride(0) if B > 1 else max(z.stride(0), C))


def _loss_outputs(B, dev, aux_floats, want_mean):
    return (torch.empty((B,), dtype=torch.float32, device=dev), torch.empty((aux_floats,), dtype=torch.float32, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
            torch.empty((1,), dtype=torch.float32, device=dev) if want_mean else None)


def _row_grads(grad_loss_i, grad_mean, B):
    g = grad_loss_i.to(torch.float32)
    if grad_mean is not None:           # d mean / d loss_i = 1 / B
        g = g + grad_mean.to(torch.float32) / max(B, 1)
    return g.contiguous()


class _HierarchicalCrossEntropy(torch.autograd.Function):
    """One se_hxe_fwd forward (loss and the metrics of the same logits), one se_hxe_bwd backward."""

    @staticmethod
    def forward(ctx, logits, labels, enc, want_mean):
        z, B, C, ldz = _logit_rows(logits, labels, enc.num_classes, "hierarchical_cross_entropy")
        t = enc.on(z.device)
        loss_i, aux, best, above, loss_mean = _loss_outputs(B, z.device, call("se_hxe_aux_floats", B), want_mean)
        call("se_hxe_fwd", z, _dtype_code(z), ldz, labels, t["pos"], t["path_off"], enc.host["path_off"], t["lvl_lo"], t["lvl_hi"],
             t["lvl_w"], B, C, loss_i, aux, best, above, loss_mean)
        ctx.save_for_backward(z, labels, aux)
        ctx.enc, ctx.ldz = enc, ldz
        ctx.mark_non_differentiable(best, above)
        return (loss_i, best, above, loss_mean) if want_mean else (loss_i, best, above)

    @staticmethod
    def backward(ctx, grad_loss_i, _best, _above, grad_mean=None):
        z, labels, aux = ctx.saved_tensors
        B, C = z.shape
        t = ctx.enc.on(z.device)
        dz = torch.empty((B, C), dtype=z.dtype, device=z.device)
        call("se_hxe_bwd", z, _dtype_code(z), ctx.ldz, labels, t["pos"], t["path_off"], ctx.enc.host["path_off"], t["lvl_lo"], t["lvl_hi"],
             t["lvl_w"], aux, _row_grads(grad_loss_i, grad_mean, B), 0.0, B, C, dz, _dtype_code(dz), C)
        return dz, None, None, None


class _SoftLabelCrossEntropy(torch.autograd.Function):
    """One se_soft_xent_fwd forward (loss and the metrics of the same logits), one se_soft_xent_bwd backward."""

    @staticmethod
    def forward(ctx, logits, labels, table, want_mean):
        z, B, C, ldz = _logit_rows(logits, labels, int(table.shape[0]), "soft_label_cross_entropy")
        loss_i, aux, best, above, loss_mean = _loss_outputs(B, z.device, 3 * B, want_mean)
        call("se_soft_xent_fwd", z, _dtype_code(z), ldz, labels, table, table.stride(0), B, C, loss_i, aux, best, above, loss_mean)
        ctx.save_for_backward(z, labels, aux, table)
        ctx.ldz = ldz
        ctx.mark_non_differentiable(best, above)
        return (loss_i, best, above, loss_mean) if want_mean else (loss_i, best, above)

    @staticmethod
    def backward(ctx, grad_loss_i, _best, _above, grad_mean=None):
        z, labels, aux, table = ctx.saved_tensors
        B, C = z.shape
        dz = torch.empty((B, C), dtype=z.dtype, device=z.device)
        call("se_soft_xent_bwd", z, _dtype_code(z), ctx.ldz, labels, table, table.stride(0), aux, _row_grads(grad_loss_i, grad_mean, B), 0.0,
             B, C, dz, _dtype_code(dz), C)
        return dz, None, None, None


def _reduced(out, reduction, return_metrics):
    if reduction not in ("none", "mean", "sum"):
        raise SehipError("reduction must be none, mean or sum, got %r" % (reduction,))
    loss = out[3][0] if reduction == "mean" else (out[0].sum() if reduction == "sum" else out[0])
    return (loss, out[1], out[2]) if return_metrics else loss


def hierarchical_cross_entropy(logits, labels, encoding, reduction="none", return_metrics=False):
    """Differentiable hierarchical cross-entropy: the softmax of ``logits`` factorised along the label's path in the class tree,
    ``sum_l lambda_l * -log p(a_l | a_{l+1})`` (include/sehip.h states the arithmetic; no probability clip): one HIP launch forward,
    one backward.  ``encoding``: ``ClassHierarchy.hxe_encoding(classes, alpha)`` (the dict, or an ``HxeEncoding`` of it): uploaded
    once per device and kept with that object.  logits [B, C] float32 or bfloat16 with any row pitch (``d logits`` in the same dtype),
    labels contiguous int64 [B].  ``reduction`` and ``return_metrics`` as in ``softmax_cross_entropy``."""
    if reduction not in ("none", "mean", "sum"):
        raise SehipError("reduction must be none, mean or sum, got %r" % (reduction,))
    out = _HierarchicalCrossEntropy.apply(logits, labels, HxeEncoding.of(encoding), reduction == "mean")
    return _reduced(out, reduction, return_metrics)


def soft_label_cross_entropy(logits, labels, table, reduction="none", return_metrics=False):
    """Differentiable cross-entropy of ``softmax(logits)`` against row ``labels[i]`` of ``table`` -- float32 [C, C] target
    distributions, ``ClassHierarchy.soft_label_table(classes, beta)`` -- without a probability clip: one HIP launch forward, one
    backward.  ``table``: a ``SoftLabelTable`` (uploaded once per device and kept there), a device tensor (used as it is, any row
    pitch) or an array (uploaded by this call).  Otherwise as ``hierarchical_cross_entropy``."""
    if reduction not in ("none", "mean", "sum"):
        raise SehipError("reduction must be none, mean or sum, got %r" % (reduction,))
    require_gpu(logits)
    if not (torch.is_tensor(table) and table.is_cuda):
        table = (table if isinstance(table, SoftLabelTable) else SoftLabelTable(table)).on(logits.device)
    if table.dim() != 2 or table.dtype != torch.float32 or table.stride(1) != 1 or table.shape[0] != table.shape[1]:
        raise SehipError("table must be a float32 [C, C] tensor with unit column stride")
    out = _SoftLabelCrossEntropy.apply(logits, labels, table, reduction == "mean")
    return _reduced(out, reduction, return_metrics)


class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        require_gpu(x)
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        x2 = x2 if x2.stride(-1) == 1 else x2.contiguous()
        B, D = x2.shape
        xhat = torch.empty((B, D), dtype=torch.float32, device=x.device)
        inv = torch.empty((B,), dtype=torch.float32, device=x.device)
        sumsq = torch.empty((B,), dtype=torch.float32, device=x.device)
        call("se_l2norm_fwd", x2, _dtype_code(x2), x2.stride(0), B, D, xhat, D, inv, sumsq)
        ctx.save_for_backward(xhat, inv, sumsq)
        ctx.in_dtype = x.dtype
        return xhat.reshape(shape)

    @staticmethod
    def backward(ctx, grad):
        xhat, inv, sumsq = ctx.saved_tensors
        B, D = xhat.shape
        g = grad.reshape(B, D).to(torch.float32).contiguous()
        dx = torch.empty_like(xhat)
        call("se_l2norm_bwd", g, D, xhat, D, inv, sumsq, B, D, dx, D)
        return dx.reshape(grad.shape).to(ctx.in_dtype)


def l2norm(x):
    """reference: utils.l2norm (utils.py:125-127) == tf.nn.l2_normalize(x, -1); float32 output."""
    return _L2Norm.apply(x)


def nn_accuracy(y_pred, labels, embedding, dot_prod_sim=False, k=1, want_scores=False, want_best=False):
    """reference: utils.nn_accuracy(embedding, dot_prod_sim, k)(embedding[labels], y_pred) (utils.py:57-100).

    Returns acc [B] float32 (and optionally the [B, C] score matrix and the best class per row)."""
    require_gpu(y_pred, labels, embedding)
    y_pred = _rows(y_pred.to(torch.float32), "y_pred")
    _rows(embedding, "embedding")
    B, D = y_pred.shape
    C = embedding.shape[0]
    acc = torch.empty((B,), dtype=torch.float32, device=y_pred.device)
    scores = torch.empty((B, C), dtype=torch.float32, device=y_pred.device) if want_scores else None
    best = torch.empty((B,), dtype=torch.int32, device=y_pred.device) if want_best else None
    need = call("se_nn_accuracy_workspace_bytes", B, C)
    ws = torch.empty((need // 8,), dtype=torch.int64, device=y_pred.device) if need else None     # (fresh: the call may be captured in a HIP graph)
    call("se_nn_accuracy", y_pred, y_pred.stride(0), labels, embedding, embedding.stride(0), B, D, C, int(bool(dot_prod_sim)), int(k),
         acc, scores, C, best, ws, need)
    out = (acc,)
    if want_scores:
        out += (scores,)
    if want_best:
        out += (best,)
    return out if len(out) > 1 else acc


EMBED_HEAD_MODES = {"cosine": 0, "sqdist": 1}
EmbedHeadForward = collections.namedtuple("EmbedHeadForward", "loss_i xhat inv_norm dist_i loss_mean n_better n_within best scores")
EmbeddingHead = collections.namedtuple("EmbeddingHead", "loss_i xhat n_better n_within best scores")


def _embed_head_mode(mode):
    if mode not in EMBED_HEAD_MODES:
        raise SehipError("mode must be 'cosine' or 'sqdist', got %r" % (mode,))
    return EMBED_HEAD_MODES[mode]


def embed_head_forward(x, labels, embedding, mode="cosine", want_xhat=True, want_inv_norm=False, want_dist=False, want_mean=False,
                       want_scores=False, want_best=False):
    """``se_embed_head_fwd``: the loss of ``cosine_loss_forward`` (mode 'cosine') or ``sqdist_loss_forward`` (mode 'sqdist') and the
    two counts of ``nn_accuracy`` on the same batch, in one launch and bit for bit: ``n_within`` classes score within 1e-6 of the
    label's, ``n_better`` beyond it, so ``nn_accuracy(k)`` is ``(n_within >= 1) & (n_better < k)`` for every k.
    Returns an ``EmbedHeadForward`` whose unwanted (or other-mode) fields are None."""
    require_gpu(x, labels, embedding)
    code = _embed_head_mode(mode)
    B, D, C = _class_loss_shapes(x, labels, embedding)
    dev = x.device

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)

    xhat = f32(B, D) if (code == 0 and want_xhat) else None
    inv_norm = f32(B) if (code == 0 and want_inv_norm) else None
    dist_i = f32(B) if (code == 1 and want_dist) else None
    loss_mean = f32(1) if want_mean else None
    loss_i, n_better, n_within = f32(B), i32(B), i32(B)
    best = i32(B) if want_best else None
    scores = f32(B, C) if want_scores else None
    need = call("se_embed_head_workspace_bytes", code, B, D, C)
    ws = torch.empty((need // 8,), dtype=torch.int64, device=dev) if need else None     # (fresh: the call may be captured in a HIP graph)
    call("se_embed_head_fwd", code, x, _dtype_code(x), x.stride(0), labels, embedding, embedding.stride(0), B, D, C, xhat, D, inv_norm,
         loss_i, dist_i, loss_mean, n_better, n_within, best, scores, C, ws, need)
    return EmbedHeadForward(loss_i, xhat, inv_norm, dist_i, loss_mean, n_better, n_within, best, scores)


class _EmbedHead(torch.autograd.Function):
    """Per-sample loss of _CosineEmbeddingLoss / _SquaredDistanceLoss with the metric counts of the same batch as non-differentiable
    by-products of the one forward launch; the backward is the siblings' (se_cosine_loss_bwd / se_sqdist_loss_bwd)."""

    @staticmethod
    def forward(ctx, x, labels, embedding, mode, want_xhat, want_scores, want_best):
        _check_loss_inputs(labels, embedding, "embedding_head")
        x = x if x.stride(-1) == 1 else x.contiguous()
        out = embed_head_forward(x, labels, embedding, mode, want_xhat=want_xhat, want_scores=want_scores, want_best=want_best)
        ctx.save_for_backward(x, labels, embedding)
        ctx.mode = mode
        extras = tuple(out.loss_i.new_empty(0) if t is None else t for t in (out.xhat, out.n_better, out.n_within, out.best, out.scores))
        ctx.mark_non_differentiable(*extras)
        return (out.loss_i,) + extras

    @staticmethod
    def backward(ctx, grad_loss_i, *_unused):
        x, labels, embedding = ctx.saved_tensors
        bwd = cosine_loss_backward if ctx.mode == "cosine" else sqdist_loss_backward
        return bwd(x, labels, embedding, grad_loss_i.contiguous()), None, None, None, None, None, None


def embedding_head(x, labels, embedding, mode="cosine", want_normalized=True, want_scores=False, want_best=False):
    """The loss head of ``--loss inv_corr`` (mode 'cosine': ``cosine_embedding_loss`` on un-normalised features) or ``--loss mse``
    (mode 'sqdist': ``squared_distance_loss``) together with the nearest-class metric of the batch, in one HIP launch forward.

    Returns ``EmbeddingHead(loss_i, xhat, n_better, n_within, best, scores)``: ``loss_i`` [B] is differentiable with respect to ``x``
    (the siblings' backward kernels); the rest is not.  ``xhat`` [B, D] are the normalised features (cosine head with
    ``want_normalized``), ``n_better`` / ``n_within`` int32 [B] the metric's counts -- ``nn_accuracy(..., k)`` of the same batch is
    ``(n_within >= 1) & (n_better < k)`` for every k --, ``best`` int32 [B] the nearest class and ``scores`` [B, C] the similarity /
    distance matrix on request; fields not asked for are None.  Every value carries the bits of the separate calls."""
    _embed_head_mode(mode)
    want_xhat = bool(want_normalized) and mode == "cosine"
    loss_i, xhat, n_better, n_within, best, scores = _EmbedHead.apply(x, labels, embedding, mode, want_xhat, bool(want_scores), bool(want_best))
    return EmbeddingHead(loss_i, xhat if want_xhat else None, n_better, n_within, best if want_best else None, scores if want_scores else None)


JOINT_HEAD_METRICS = {"nearest": DEFINES["SE_HEAD_METRIC_NEAREST"], "argmax": DEFINES["SE_HEAD_METRIC_ARGMAX"]}
JointHead = collections.namedtuple("JointHead", "emb_loss_i cls_loss_i n_better n_within p_best p_above scores z_best z_above")


def _pitch(t):
    """Row pitch of a 2-d tensor with contiguous rows (a single row has no meaningful stride)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


class _JointHead(torch.autograd.Function):
    """Embedding loss on ``p``, cross-entropy on ``logits`` and the metrics of both in one se_joint_head_fwd; the gradients with
    respect to ``p`` and ``logits`` in one se_joint_head_bwd.  Every integer output is a non-differentiable by-product."""

    @staticmethod
    def forward(ctx, p, logits, labels, embedding, metric, want_scores):
        require_gpu(p, labels, embedding, logits)
        code = JOINT_HEAD_METRICS[metric]
        _f32_rows(p, "p")
        B, D = p.shape
        if labels.dtype != torch.int64 or labels.numel() != B or not labels.is_contiguous():
            raise SehipError("labels must be a contiguous int64 [B] tensor")
        if embedding is not None:
            _f32_rows(embedding, "embedding")
            if embedding.shape[1] != D:
                raise SehipError("embedding must be float32 [C, %d]" % D)
            _check_loss_inputs(labels, embedding, "joint_head")
            C = embedding.shape[0]
        else:
            C = D
            if os.environ.get("SEHIP_CHECK_LABELS") and B and (int(labels.min()) < 0 or int(labels.max()) >= C):
                raise IndexError("joint_head: labels span [%d, %d] but there are %d classes" % (int(labels.min()), int(labels.max()), C))
        if logits is not None:
            _rows(logits, "logits")
            if logits.shape[0] != B or logits.shape[1] != C:
                raise SehipError("logits must be [%d, %d], got %s" % (B, C, tuple(logits.shape)))
        dev = p.device

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        def i32(*shape):
            return torch.empty(shape, dtype=torch.int32, device=dev)

        nearest = metric == "nearest"
        emb_loss_i = f32(B)
        n_better, n_within = (i32(B), i32(B)) if nearest else (None, None)
        p_best = i32(B)
        p_above = None if nearest else i32(B)
        scores = f32(B, C) if (want_scores and nearest) else None
        cls_loss_i = aux = z_best = z_above = None
        if logits is not None:
            cls_loss_i, aux = f32(B), f32(call("se_softmax_xent_aux_floats", B))
            z_best, z_above = i32(B), i32(B)
        need = call("se_joint_head_workspace_bytes", code, B, D, C)
        ws = torch.empty((need // 8,), dtype=torch.int64, device=dev) if need else None     # (fresh: the call may be captured in a HIP graph)
        call("se_joint_head_fwd", p, _pitch(p), labels, embedding, _pitch(embedding) if embedding is not None else 0, B, D, C, code,
             emb_loss_i, n_better, n_within, p_best, p_above, scores, C,
             logits, _dtype_code(logits) if logits is not None else DTYPE_F32, _pitch(logits) if logits is not None else 0, cls_loss_i, aux,
             z_best, z_above, ws, need)
        ctx.save_for_backward(labels, embedding, logits, aux)
        ctx.dims = (B, D, C)
        empty_f, empty_i = emb_loss_i.new_empty(0), p_best.new_empty(0)
        extras = tuple(empty_i if t is None else t for t in (n_better, n_within, p_best, p_above)) + \
            (empty_f if scores is None else scores,) + tuple(empty_i if t is None else t for t in (z_best, z_above))
        ctx.mark_non_differentiable(*extras)
        if cls_loss_i is None:
            cls_loss_i = emb_loss_i.new_empty(0)
            ctx.mark_non_differentiable(cls_loss_i)
        return (emb_loss_i, cls_loss_i) + extras

    @staticmethod
    def backward(ctx, grad_emb, grad_cls, *_unused):
        labels, embedding, logits, aux = ctx.saved_tensors
        B, D, C = ctx.dims
        dp = dz = None
        if ctx.needs_input_grad[0]:
            dp = torch.empty((B, D), dtype=torch.float32, device=labels.device)
        z = logits if (logits is not None and ctx.needs_input_grad[1]) else None
        if z is not None:
            dz = torch.empty((B, C), dtype=z.dtype, device=z.device)
        ge = grad_emb.to(torch.float32).contiguous() if dp is not None else None
        gc = grad_cls.to(torch.float32).contiguous() if dz is not None else None
        call("se_joint_head_bwd", labels, embedding, _pitch(embedding) if embedding is not None else 0, B, D, C, ge, 0.0, dp, D,
             z, _dtype_code(z) if z is not None else DTYPE_F32, _pitch(z) if z is not None else 0, aux, gc, 0.0, dz,
             _dtype_code(dz) if dz is not None else DTYPE_F32, C)
        return dp, dz, None, None, None, None


def joint_head(p, labels, embedding, logits=None, metric="nearest", want_scores=False):
    """The head of ``--cls_weight``: the embedding loss ``1 - <embedding[y], p>`` on the model's first output ``p`` [B, D] float32 --
    used as it comes, the l2norm / softmax layer of the model has already run --, Keras 2.2's clipped cross-entropy on ``logits``
    [B, C] (float32 / bfloat16; None: the embedding part alone) and the metrics of both outputs, in ONE HIP launch forward and one
    backward (se_joint_head_fwd / se_joint_head_bwd).  ``embedding`` float32 [C, D], or None for the identity table of one-hot
    targets (then D == C and ``metric`` must be "argmax").

    Returns ``JointHead(emb_loss_i, cls_loss_i, n_better, n_within, p_best, p_above, scores, z_best, z_above)``.  ``emb_loss_i`` and
    ``cls_loss_i`` [B] are differentiable with respect to ``p`` and ``logits``; the rest are int32 [B] by-products (``scores`` [B, C]
    float32 with ``want_scores``), None where they do not apply:
      metric "nearest": ``nn_accuracy(p, labels, embedding, dot_prod_sim=True, k)`` is ``(n_within >= 1) & (n_better < k)`` for every
                        k, ``p_best`` the nearest class, ``scores`` the similarity matrix -- the bits of se_nn_accuracy;
      metric "argmax":  ``p_best`` = arg-max of the row of p (np.argmax rules), ``p_above`` = entries strictly above the label's:
                        ``p_best == labels`` is Keras' accuracy, ``p_above < k`` is tf.nn.in_top_k;
      ``z_best`` / ``z_above``: the same two for the logits, ``cls_loss_i`` and they the bits of ``softmax_cross_entropy``.
    Labels are clamped to [0, C - 1]; ``SEHIP_CHECK_LABELS=1`` checks them on the host."""
    if metric not in JOINT_HEAD_METRICS:
        raise SehipError("metric must be 'nearest' or 'argmax', got %r" % (metric,))
    if embedding is None and metric != "argmax":
        raise SehipError("joint_head: the identity table (embedding None) goes with metric 'argmax'")
    p = p if p.stride(-1) == 1 else p.contiguous()
    if logits is not None and logits.stride(-1) != 1:
        logits = logits.contiguous()
    out = _JointHead.apply(p, logits, labels, embedding, metric, bool(want_scores))
    emb_loss_i, cls_loss_i, n_better, n_within, p_best, p_above, scores, z_best, z_above = out
    nearest, cls = metric == "nearest", logits is not None
    return JointHead(emb_loss_i, cls_loss_i if cls else None, n_better if nearest else None, n_within if nearest else None, p_best,
                     None if nearest else p_above, scores if (nearest and want_scores) else None, z_best if cls else None,
                     z_above if cls else None)


class _LabelEmbedLoss(torch.autograd.Function):
    """reference: labelembed_loss (learn_labelembedding.py:21-37) and its TF-autodiff backward."""

    @staticmethod
    def forward(ctx, out1, out2, tar, targets, tau, alpha, beta):
        require_gpu(out1, out2, tar, targets)
        for t, name in ((out1, "out1"), (out2, "out2"), (tar, "tar")):
            _f32_rows(t, name)
        B, C = out1.shape
        if out2.shape != (B, C) or tar.shape != (B, C):
            raise SehipError("out1, out2 and tar must share the shape [B, C]")
        if targets.dtype != torch.int64 or targets.numel() != B or not targets.is_contiguous():
            raise SehipError("targets must be a contiguous int64 [B] tensor")
        loss_i = torch.empty((B,), dtype=torch.float32, device=out1.device)
        aux = torch.empty((max(call("se_labelembed_aux_floats", B), 1),), dtype=torch.float32, device=out1.device)
        call("se_labelembed_loss_fwd", out1, out1.stride(0), out2, out2.stride(0), tar, tar.stride(0), targets, B, C, float(tau),
             float(alpha), float(beta), loss_i, aux)
        ctx.save_for_backward(out1, out2, tar, targets, aux)
        ctx.hyper = (float(tau), float(alpha), float(beta))
        return loss_i

    @staticmethod
    def backward(ctx, grad):
        out1, out2, tar, targets, aux = ctx.saved_tensors
        tau, alpha, beta = ctx.hyper
        B, C = out1.shape
        grad = grad.contiguous().to(torch.float32)
        need = ctx.needs_input_grad
        d1 = torch.empty_like(out1, memory_format=torch.contiguous_format) if need[0] else None
        d2 = torch.empty_like(out2, memory_format=torch.contiguous_format) if need[1] else None
        dt = torch.empty_like(tar, memory_format=torch.contiguous_format) if need[2] else None
        call("se_labelembed_loss_bwd", out1, out1.stride(0), out2, out2.stride(0), tar, tar.stride(0), targets, grad, 0.0, B, C,
             tau, alpha, beta, aux, d1, C, d2, C, dt, C)
        return d1, d2, dt, None, None, None, None


def labelembed_loss(out1, out2, tar, targets, tau=2.0, alpha=0.9, beta=0.5):
    """Per-sample label-embedding loss [B] (learn_labelembedding.py:21-37), differentiable w.r.t. out1, out2, tar."""
    return _LabelEmbedLoss.apply(out1, out2, tar, targets, tau, alpha, beta)


LE_GRID_CAP = DEFINES["SE_LABELEMBED_GRID_CAP"]     # grid cap of the per-sample label-embedding kernels: 4 samples per workgroup


class _LabelEmbedTableLoss(torch.autograd.Function):
    """reference: labelembed_loss on ``tar = labelembeddings(targets)`` (learn_labelembedding.py:21-37, 51-54) and its TF-autodiff
    backward, the gradient of the Embedding table included: se_labelembed_table_loss_fwd / _bwd read the table row of every sample
    in place and reduce the table's gradient per class in batch order.  ``out2 is None``: ``out1`` is the packed [B, 2 C] tensor
    ``out1 | out2`` and its gradient one [B, 2 C] buffer both halves are written into through their pitch."""

    @staticmethod
    def forward(ctx, out1, out2, table, targets, tau, alpha, beta):
        require_gpu(out1, out2, table, targets)
        packed = out2 is None
        if packed:
            whole = out1 if out1.dim() != 2 or out1.stride(1) == 1 else out1.contiguous()
            if whole.dim() != 2 or whole.shape[1] % 2:
                raise SehipError("the packed logits must be a [B, 2 C] tensor")
            half = whole.shape[1] // 2
            out1, out2 = whole[:, :half], whole[:, half:]
        out1, out2, table = (t if t.dim() != 2 or t.stride(1) == 1 else t.contiguous() for t in (out1, out2, table))
        ld1, ld2, ldtab = _f32_2d(out1, "out1", 1), _f32_2d(out2, "out2", 1), _f32_2d(table, "table", 1)
        B, C = out1.shape
        if out2.shape != (B, C) or table.shape != (C, C):
            raise SehipError("out1 and out2 must share the shape [B, C] and the table must be [C, C]")
        if targets.dtype != torch.int64 or targets.numel() != B or not targets.is_contiguous():
            raise SehipError("targets must be a contiguous int64 [B] tensor")
        loss_i = torch.empty((B,), dtype=torch.float32, device=out1.device)
        aux = torch.empty((max(call("se_labelembed_aux_floats", B), 1),), dtype=torch.float32, device=out1.device)
        call("se_labelembed_table_loss_fwd", out1, ld1, out2, ld2, table, ldtab, targets, B, C, float(tau), float(alpha), float(beta),
             loss_i, aux)
        ctx.save_for_backward(out1, out2, table, targets, aux)
        ctx.hyper = (float(tau), float(alpha), float(beta), ld1, ld2, ldtab, packed)
        return loss_i

    @staticmethod
    def backward(ctx, grad):
        out1, out2, table, targets, aux = ctx.saved_tensors
        tau, alpha, beta, ld1, ld2, ldtab, packed = ctx.hyper
        B, C = out1.shape
        grad = grad.contiguous().to(torch.float32)
        need = ctx.needs_input_grad
        both = d1 = d2 = dtab = None
        ldd = C
        if packed:
            if need[0]:
                both = torch.empty((B, 2 * C), dtype=torch.float32, device=out1.device)
                d1, d2, ldd = both[:, :C], both[:, C:], 2 * C
        else:
            d1 = torch.empty((B, C), dtype=torch.float32, device=out1.device) if need[0] else None
            d2 = torch.empty((B, C), dtype=torch.float32, device=out1.device) if need[1] else None
        if need[2]:
            dtab = torch.empty((C, C), dtype=torch.float32, device=out1.device)
        call("se_labelembed_table_loss_bwd", out1, ld1, out2, ld2, table, ldtab, targets, grad, 0.0, B, C, tau, alpha, beta, aux,
             d1, ldd, d2, ldd, dtab, C)
        return (both if packed else d1), d2 if not packed else None, dtab, None, None, None, None


def labelembed_table_loss(out1, out2, table, targets, tau=2.0, alpha=0.9, beta=0.5):
    """Per-sample label-embedding loss [B] (learn_labelembedding.py:21-37) with ``tar`` read from the learned ``[C, C]`` float32
    ``table`` (row ``clamp(targets[i], 0, C - 1)`` for sample i) instead of a gathered copy; differentiable w.r.t. ``out1``, ``out2``
    and ``table``.  ``out1`` / ``out2`` [B, C] float32 need unit stride in the last dimension only (e.g. the column halves of one
    [B, 2 C] tensor: their row pitch is passed through).  Loss and logit gradients are bit for bit those of ``labelembed_loss`` on
    ``table[targets]``; the table gradient is the sum of that call's ``d_tar`` rows per class in batch order -- the same inputs give
    the same bits (torch's embedding backward adds with atomics).  Only the inputs that require a gradient get one."""
    return _LabelEmbedTableLoss.apply(out1, out2, table, targets, tau, alpha, beta)


def labelembed_table_loss_packed(logits2, table, targets, tau=2.0, alpha=0.9, beta=0.5):
    """``labelembed_table_loss(logits2[:, :C], logits2[:, C:], ...)`` for the packed head output ``logits2 = out1 | out2`` [B, 2 C]:
    the same bits, but the gradient of ``logits2`` is ONE [B, 2 C] buffer that the kernel writes both halves of through their pitch
    (slicing first makes autograd pad each half's gradient into a zero [B, 2 C] tensor and add the two)."""
    return _LabelEmbedTableLoss.apply(logits2, None, table, targets, tau, alpha, beta)


class _DeviseLoss(torch.autograd.Function):
    """reference: utils.devise_ranking_loss (utils.py:103-122) and its TF-autodiff backward w.r.t. y_pred."""

    @staticmethod
    def forward(ctx, y_pred, target, embedding, margin):
        require_gpu(y_pred, target, embedding)
        yp = _rows(y_pred.to(torch.float32), "y_pred")
        yp = yp if yp.stride(1) == 1 else yp.contiguous()
        _f32_rows(embedding, "embedding")
        B, D = yp.shape
        C = embedding.shape[0]
        if embedding.shape[1] != D or embedding.device != yp.device:
            raise SehipError("embedding must be a float32 [C, %d] tensor on %s" % (D, yp.device))
        if target.dim() == 1 and not target.is_floating_point():
            labels, yt, ldt = target.long().contiguous(), None, 0
            if labels.numel() != B:
                raise SehipError("labels must be an integer [B] tensor")
        else:
            labels, yt = None, _rows(target.to(torch.float32).contiguous(), "y_true")
            ldt = yt.stride(0)
        loss_i = torch.empty((B,), dtype=torch.float32, device=yp.device)
        aux = torch.empty((max(call("se_devise_aux_floats", B, C), 1),), dtype=torch.float32, device=yp.device)
        call("se_devise_loss_fwd", yp, yp.stride(0), labels, yt, ldt, embedding, embedding.stride(0), B, D, C, margin, loss_i, aux)
        ctx.save_for_backward(aux, embedding, labels if labels is not None else yt)
        ctx.by_label, ctx.shape, ctx.in_dtype = labels is not None, (B, D, C), y_pred.dtype
        return loss_i

    @staticmethod
    def backward(ctx, grad_loss_i):
        aux, embedding, tgt = ctx.saved_tensors
        B, D, C = ctx.shape
        g = grad_loss_i.to(torch.float32).contiguous()
        dp = torch.empty((B, D), dtype=torch.float32, device=g.device)
        labels, yt = (tgt, None) if ctx.by_label else (None, tgt)
        call("se_devise_loss_bwd", labels, yt, 0 if yt is None else yt.stride(0), embedding, embedding.stride(0), g, 1.0, B, D, C,
             aux, dp, D)
        return dp.to(ctx.in_dtype), None, None, None


DEVISE_TORCH_ABOVE = 1 << 29      # B * C * D from which the loss is written with PyTorch ops instead of the fused kernels


def devise_ranking_loss(y_pred, target, embedding, margin=0.1):
    """Per-sample DeViSE ranking loss [B] (utils.py:103-122), differentiable w.r.t. ``y_pred``; ``target`` = int64 labels [B]
    (rows of ``embedding`` gathered on the device) or an explicit float ``y_true`` [B, D].

    Fused fp32-MFMA kernels (``se_devise_loss_fwd/bwd``) up to ``B * C * D < DEVISE_TORCH_ABOVE``; larger problems -- batch 1024 at
    C = D = 1000 -- take the same expression in PyTorch ops: there the one-wave-per-tile forward kernel (111 us) loses to
    hipBLASLt's GEMM + elementwise kernels (measured: 223 vs 206 us forward + backward), while at the training sizes (batch 128)
    the fused pair wins (165 vs 208 us at C = D = 1000; profiles/r04_d_devise_microbench.txt).  Both are float32 and
    differentiable; the kernels are what the parity tests hold to the reference-produced fixtures."""
    B, D = y_pred.shape
    if B * embedding.shape[0] * D >= DEVISE_TORCH_ABOVE and y_pred.is_cuda:
        yp = y_pred.to(torch.float32)
        yt = embedding[target.long().clamp(0, embedding.shape[0] - 1)] if (target.dim() == 1 and not target.is_floating_point()) \
            else target.to(torch.float32)
        true_sim = (yt * yp).sum(-1)
        return torch.relu(float(margin) - true_sim[:, None] + yp @ embedding.t()).sum(-1) - float(margin)
    return _DeviseLoss.apply(y_pred, target, embedding, float(margin))


def _flat_f32(n, device, *named):
    """Every tensor of ``named`` ((tensor or None, name) pairs) is a contiguous float32 tensor of ``n`` elements on ``device``."""
    for t, what in named:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or t.device != device):
            raise SehipError("%s must be a contiguous float32 tensor of %d elements on %s" % (what, n, device))


def _lr_arg(lr, device):
    """``(lr, lr_dev)`` of an entry point that reads its learning rate from the argument or from a device scalar."""
    if not torch.is_tensor(lr):
        return float(lr), None
    require_gpu(lr)
    if lr.dtype != torch.float32 or lr.numel() != 1 or lr.device != device:
        raise SehipError("a learning-rate tensor must hold one float32 value on %s" % (device,))
    return 0.0, lr


ADAGRAD_MAX_BLOCKS = DEFINES["SE_ADAGRAD_MAX_BLOCKS"]     # grid cap of se_adagrad_step: 256 threads per workgroup, 4 elements per thread


def adagrad_step_(p, accum, g, l2=None, lr=0.01, grad_scale=1.0, epsilon=1e-7):
    """In place, one launch (``se_adagrad_step``): Keras 2.2's Adagrad update ``accum += g2 * g2; p -= lr * g2 / (sqrt(accum) + epsilon)``
    with ``g2 = g * grad_scale + l2 * p`` (keras.optimizers.Adagrad as learn_devise.py:87,114 uses it; every operation a separately
    rounded float32 operation, include/sehip.h).  ``p``, ``accum``, ``g`` and ``l2`` (None: no regulariser) are contiguous float32
    device tensors of one size; ``g`` is only read.  ``lr``: a float, or a 0-dim float32 device tensor that is read on the device
    when the kernel runs (a captured launch then follows the schedule).  Returns ``p``."""
    require_gpu(p, accum, g, l2)
    n = p.numel()
    _flat_f32(n, p.device, (p, "p"), (accum, "accum"), (g, "g"), (l2, "l2"))
    lr, lr_dev = _lr_arg(lr, p.device)
    call("se_adagrad_step", p, accum, g, l2, n, lr, lr_dev, float(grad_scale), float(epsilon))
    return p


SGD_MAX_BLOCKS = DEFINES["SE_SGD_MAX_BLOCKS"]     # grid cap of se_grad_clip_factor / se_sgd_step: 256 threads per workgroup, 4 elements per thread


def grad_clip_factor(g, p=None, l2=None, grad_scale=1.0, clipnorm=None, workspace=None, out=None):
    """``stats`` = [norm, factor] (a 2-element float32 device tensor) of the regularised gradient ``g2 = g * grad_scale + l2 * p``
    (``se_grad_clip_factor``: two launches): the Euclidean norm, its squares summed in float64 in an order that ``g.numel()`` and the
    pointers' alignment fix, and ``factor = min(clipnorm / (norm + 1e-12), 1)``, NaN for a NaN norm -- what
    ``torch.clamp(clipnorm / (norm + 1e-12), max=1.0)`` gives.  ``g``, ``p`` and ``l2`` (None: no regulariser; ``p`` is then not
    read) are contiguous float32 device tensors of one size and only read.  ``workspace`` (any device tensor of at least
    ``se_grad_clip_workspace_bytes()`` bytes) and ``out`` are used when given, so that a captured call allocates nothing.  Of an
    empty ``g`` the norm is 0 and the factor 1 when ``out`` is not given; a given ``out`` is left alone."""
    require_gpu(g, p, l2, workspace, out)
    if clipnorm is None:
        raise SehipError("grad_clip_factor needs clipnorm")
    n = g.numel()
    _flat_f32(n, g.device, (g, "g"), (p, "p"), (l2, "l2"))
    if l2 is not None and p is None:
        raise SehipError("l2 needs p")
    need = int(call("se_grad_clip_workspace_bytes"))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=g.device)
    elif workspace.numel() * workspace.element_size() < need or not workspace.is_contiguous() or workspace.device != g.device:
        raise SehipError("the workspace must be a contiguous tensor of at least %d bytes on %s" % (need, g.device))
    if out is None:
        out = torch.tensor([0.0, 1.0], dtype=torch.float32, device=g.device)
    elif out.dtype != torch.float32 or out.numel() != 2 or not out.is_contiguous() or out.device != g.device:
        raise SehipError("out must be a contiguous float32 tensor of 2 elements on %s" % (g.device,))
    call("se_grad_clip_factor", g, p if l2 is not None else None, l2, n, float(grad_scale), float(clipnorm), workspace, out)
    return out


def sgd_step_(p, v, g, l2=None, lr=0.01, grad_scale=1.0, clip=None, momentum=0.9, nesterov=False):
    """In place, one launch (``se_sgd_step``): Keras 2.2's SGD update ``v = momentum * v - lr * g3; p += v`` (Nesterov:
    ``p += momentum * v - lr * g3``) with ``g3 = (g * grad_scale + l2 * p) * clip[0]`` (keras.optimizers.SGD with ``clipnorm``; every
    operation a separately rounded float32 operation, include/sehip.h).  ``p``, ``v``, ``g`` and ``l2`` (None: no regulariser) are
    contiguous float32 device tensors of one size; ``g`` is only read.  ``lr``: a float, or a 0-dim float32 device tensor that is read
    on the device when the kernel runs (a captured launch then follows the schedule).  ``clip``: None, or a float32 device tensor
    whose first element is read on the device as the clip factor (``grad_clip_factor(...)[1:]``).  Returns ``p``."""
    require_gpu(p, v, g, l2, clip)
    n = p.numel()
    _flat_f32(n, p.device, (p, "p"), (v, "v"), (g, "g"), (l2, "l2"))
    lr, lr_dev = _lr_arg(lr, p.device)
    if clip is not None and (clip.dtype != torch.float32 or clip.numel() < 1 or clip.device != p.device):
        raise SehipError("a clip-factor tensor must hold a float32 value on %s" % (p.device,))
    call("se_sgd_step", p, v, g, l2, n, lr, lr_dev, float(grad_scale), clip, float(momentum), int(bool(nesterov)))
    return p


LAYOUT_NCHW, LAYOUT_NHWC = DEFINES["SE_LAYOUT_NCHW"], DEFINES["SE_LAYOUT_NHWC"]
_LAYOUT_FORMATS = ((LAYOUT_NCHW, torch.contiguous_format), (LAYOUT_NHWC, torch.channels_last))


def _common_layout(what, *tensors):
    """``(layout code, memory format)`` in which every one of the 4-d ``tensors`` is dense; ``SehipError`` when there is none (mixed
    or strided operands).  Where both hold for all of them -- one channel, 1 x 1 images, or no element at all, which torch calls
    contiguous whatever the strides -- the two address the same memory, and the strides decide which one the results are allocated
    in: channels_last when an operand carries its strides (channel stride 1, column stride C), NCHW otherwise."""
    dense = [(code, fmt) for code, fmt in _LAYOUT_FORMATS if all(t.is_contiguous(memory_format=fmt) for t in tensors)]
    if not dense:
        raise SehipError("%s: the operands must share one dense layout, contiguous (NCHW) or channels_last (NHWC); got strides %s"
                         % (what, ", ".join(str(tuple(t.stride())) for t in tensors)))
    if len(dense) == 2 and any(t.shape[1] > 1 and t.stride(1) == 1 and t.stride(3) == t.shape[1] for t in tensors):
        return dense[1]
    return dense[0]


class _ShortcutAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, x, stride, pad_before):
        layout, fmt = _common_layout("shortcut_add", s, x)
        out = torch.empty(s.shape, dtype=s.dtype, device=s.device, memory_format=fmt)
        (B, C, H, W), (_, Cin, Hx, Wx) = s.shape, x.shape
        call("se_shortcut_add_fwd", s, x, out, _dtype_code(s), layout, B, C, H, W, Cin, Hx, Wx, stride, pad_before)
        ctx.geometry = (x.shape, stride, pad_before, layout, fmt)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x_shape, stride, pad_before, layout, fmt = ctx.geometry
        dx = None
        if ctx.needs_input_grad[1]:
            g = grad_out.contiguous(memory_format=fmt)          # no copy when autograd hands the gradient over in the forward's layout
            dx = torch.empty(x_shape, dtype=g.dtype, device=g.device, memory_format=fmt)
            (B, C, H, W), (_, Cin, Hx, Wx) = g.shape, x_shape
            call("se_shortcut_add_bwd", g, dx, _dtype_code(g), layout, B, C, H, W, Cin, Hx, Wx, stride, pad_before)
        return grad_out, dx, None, None         # the gradient of s is the incoming tensor itself: no kernel, no copy


def shortcut_add(s, x, stride=1, pad_before=0):
    """``s + ChannelPadding((pad_before, C - Cin - pad_before))(AveragePooling2D(stride)(x))`` in one launch (``se_shortcut_add_fwd``;
    the residual add at the end of every PyramidNet block, models/cifar_pyramidnet.py:81-110), with autograd: the gradient of ``s`` is
    the incoming gradient tensor itself, that of ``x`` one launch of ``se_shortcut_add_bwd``.  ``s`` [B, C, H, W] and ``x``
    [B, Cin, Hx, Wx] are float32 or bfloat16 device tensors of one dtype, both contiguous or both channels_last; ``stride`` 1 or 2
    (H = Hx // stride, W = Wx // stride).  The arithmetic is fixed in include/sehip.h."""
    require_gpu(s, x)
    if s.dim() != 4 or x.dim() != 4 or s.shape[0] != x.shape[0]:
        raise SehipError("shortcut_add takes s [B, C, H, W] and x [B, Cin, Hx, Wx]; got %s and %s" % (tuple(s.shape), tuple(x.shape)))
    if s.dtype != x.dtype or s.device != x.device:
        raise SehipError("shortcut_add: s (%s, %s) and x (%s, %s) must share dtype and device" % (s.dtype, s.device, x.dtype, x.device))
    _dtype_code(s)
    return _ShortcutAdd.apply(s, x, int(stride), int(pad_before))


# --------------------------------------------------------------------------------------------
# retrieval side
# --------------------------------------------------------------------------------------------

def row_sqnorm(x):
    """float32 ``np.sum(x ** 2, axis=-1)``, bit-exact (evaluate_retrieval.py:61)."""
    require_gpu(x)
    _f32_rows(x, "x")
    sq = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    call("se_row_sqnorm", x, x.stride(0), x.shape[0], x.shape[1], sq)
    return sq


def normalize_rows_(x):
    """In-place ``x /= np.linalg.norm(x, axis=-1, keepdims=True)``, bit-exact (evaluate_retrieval.py:58)."""
    require_gpu(x)
    _f32_rows(x, "x")
    call("se_normalize_rows", x, x.stride(0), x.shape[0], x.shape[1])
    return x


def row_pitch(n, dtype):
    """Elements per row of an n-column ``dtype`` matrix whose rows start a multiple of 16 bytes apart."""
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    return (n + per16 - 1) // per16 * per16


def empty_rows(q, n, dtype, device):
    """[q, n] matrix whose row pitch is a multiple of 16 bytes (a view of a wider buffer when n is not): the distance and ranking
    kernels stream rows out with 16-byte stores and fall back to element stores on unaligned pitches -- 24,633 columns (odd): distances
    1.50 -> 1.18 ms, ranking 3.37 -> 3.01 ms (tools/bench_odd_pitch.py)."""
    pitch = row_pitch(n, dtype)
    buf = torch.empty((q, pitch), dtype=dtype, device=device)
    return buf if pitch == n else buf[:, :n]


def pairwise_dist(a, b=None, metric=METRIC_COSINE, sqa=None, sqb=None, kblocks=None, out=None):
    """All-pairs distances [q, n] (evaluate_retrieval.py:59 / :61-62) with the canonical FMA chain."""
    require_gpu(a, b, sqa, sqb, out)
    b = a if b is None else b
    _f32_rows(a, "a"); _f32_rows(b, "b")
    q, d = a.shape
    n = b.shape[0]
    if b.shape[1] != d:
        raise SehipError("a and b must have the same number of columns")
    if metric == METRIC_EUCLID:
        if sqa is None:
            sqa = row_sqnorm(a)
        if sqb is None:
            sqb = sqa if b is a else row_sqnorm(b)
    if out is None:
        out = empty_rows(q, n, torch.float32, a.device)
    kb, nkb = _kblocks_arg(kblocks)
    call("se_pairwise_dist", a, a.stride(0), b, b.stride(0), sqa, sqb, q, n, d, int(metric), kb, nkb, out, out.stride(0))
    return out


_ws_cache = {}


def _workspace(nbytes, device, kind=None):
    """Grow-only per-device scratch buffer (the C ABI never allocates).  ``kind``: a buffer of its own under that name, for an entry
    point that keeps state in its workspace between its launches while another may run on a second stream."""
    key = _device_index(device) if kind is None else (kind, _device_index(device))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _ws_cache.pop(key, None)
        ws = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


_rank_ready = set()


def rank_rows_init(device=None):
    """``se_rank_rows_init`` on ``device`` (default: current): capability probe + self-test of every hardware-ordered ranking kernel
    variant; the one synchronising call of the ranking.  ``rank_rows`` calls it by itself before its first ranking on a device, so
    that every later ``se_rank_rows`` is purely asynchronous (graph-capturable)."""
    require_gpu()
    key = _device_index(device)
    with torch.cuda.device(key):
        ws = torch.empty((call("se_rank_rows_init_workspace_bytes"),), dtype=torch.uint8, device=torch.device("cuda", key))
        call("se_rank_rows_init", ws, ws.numel())
    _rank_ready.add(key)


def workspace_bytes(device=None):
    """Bytes the per-device workspace cache currently holds."""
    ws = _ws_cache.get(_device_index(device))
    return 0 if ws is None else int(ws.numel())


def release_workspace(device=None):
    """Drop the grow-only scratch buffer of ``device`` (default: every device): the long-row ranking grows it to ~3 GB, the fused
    top-k to ~4 GB, and it is otherwise kept for the life of the process."""
    if device is None:
        _ws_cache.clear()
    else:
        for key in [k for k in _ws_cache if k == _device_index(device) or (isinstance(k, tuple) and k[1] == _device_index(device))]:
            _ws_cache.pop(key)


def phase_timing(on=True):
    """``se_phase_timing``: switch the library's phase events on / off (a measuring aid: bench.py's per-leg rooflines)."""
    call("se_phase_timing", 1 if on else 0)


def phase_timing_read():
    """``se_phase_timing_read`` -> (dict phase -> total ms since the last read, counters or None).  counters = {"redone", "recomputed",
    "candidates", "queries"} of the last ``retrieve_topk`` call (its workspace -- the per-device cache -- is still alive)."""
    cap = 96
    names = (ctypes.c_char_p * cap)()
    ms = (ctypes.c_float * cap)()
    cnt = (ctypes.c_int64 * 5)()
    n = call("se_phase_timing_read", names, ms, cap, cnt)
    out = {}
    for i in range(n):
        out[names[i].decode()] = out.get(names[i].decode(), 0.0) + float(ms[i])
    counters = None if cnt[4] < 0 else {"redone": int(cnt[1]), "recomputed": int(cnt[2]), "candidates": int(cnt[3]), "queries": int(cnt[4])}
    return out, counters


def rank_rows_workspace_bytes(q, n):
    return call("se_rank_rows_workspace_bytes", int(q), int(n))


RANK_U16_MAX_N = 53248     # rows the register-resident ranking kernel takes: the only ones it writes 16-bit ranks for


def rank_rows(pdist, idx64=False, out=None, idx16=False):
    """Canonical ``np.argsort(pdist, axis=-1)`` (evaluate_retrieval.py:67): (distance, index) ascending.
    ``idx16``: uint16 ranks (returned as an int16 tensor holding their bit patterns; rows of at most 53,248 columns) -- half the
    bytes for ``hierarchical_precision`` to read."""
    require_gpu(pdist, out)
    _f32_rows(pdist, "pdist")
    if _device_index(pdist.device) not in _rank_ready:
        rank_rows_init(pdist.device)
    q, n = pdist.shape
    if out is None:
        out = empty_rows(q, n, torch.int16 if idx16 else (torch.int64 if idx64 else torch.int32), pdist.device)
    ws = _workspace(call("se_rank_rows_workspace_bytes", q, n), pdist.device)
    call("se_rank_rows", pdist, pdist.stride(0), q, n, out, _rank_width_code(out), out.stride(0), ws, ws.numel())
    return out


def _f64_rows(t, what):
    if t.dtype != torch.float64:
        raise SehipError("%s must be float64" % what)
    return _rows(t, what)


def pairwise_dist_f64(a, b=None, metric=METRIC_COSINE, sqa=None, sqb=None, out=None, img=True):
    """Float64 all-pairs distances ``[q, n]`` of float64 operands (``se_pairwise_dist_f64``: ONE sequential float64 FMA chain per
    element) and their float32 image.  ``sqa`` / ``sqb``: float64 row square norms, required for the
    Euclidean metric -- the caller computes them with the reference's NumPy line (evaluate_retrieval.py:61).  ``img``: True
    (allocate), a float32 ``[q, n]`` tensor, or None / False (no image).  Returns ``(out, img)``."""
    require_gpu(a, b, sqa, sqb, out, img if isinstance(img, torch.Tensor) else None)
    b = a if b is None else b
    _f64_rows(a, "a"); _f64_rows(b, "b")
    q, d = a.shape
    n = b.shape[0]
    if b.shape[1] != d:
        raise SehipError("a and b must have the same number of columns")
    if metric == METRIC_EUCLID:
        if sqa is None or (sqb is None and b is not a):
            raise SehipError("the float64 Euclidean metric needs sqa and sqb (np.sum(x ** 2, axis=-1) of the host)")
        sqb = sqa if sqb is None else sqb
        for t, rows in ((sqa, q), (sqb, n)):
            if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != rows:
                raise SehipError("sqa / sqb must be contiguous float64 vectors of one entry per row")
    if out is None:
        out = empty_rows(q, n, torch.float64, a.device)
    _f64_rows(out, "out")
    if img is True:
        img = empty_rows(q, n, torch.float32, a.device)
    elif img is False:
        img = None
    if img is not None:
        _f32_rows(img, "img")
    if tuple(out.shape) != (q, n) or (img is not None and tuple(img.shape) != (q, n)):
        raise SehipError("out / img must be [%d, %d] matrices" % (q, n))
    call("se_pairwise_dist_f64", a, a.stride(0), b, b.stride(0), sqa, sqb, q, n, d, int(metric), out, out.stride(0), img,
         0 if img is None else img.stride(0))
    return out, img


def rank_refine_f64_(pdist64, img, rank):
    """``se_rank_refine_f64``: ``rank = rank_rows(img)`` (int32 or int64) becomes, in place, the canonical ranking of the float64
    distances ``pdist64`` -- every run of adjacent ranks with equal float32 images is sorted by (float64 distance, index)."""
    require_gpu(pdist64, img, rank)
    _f64_rows(pdist64, "pdist64"); _f32_rows(img, "img")
    if rank.dtype not in (torch.int32, torch.int64) or rank.dim() != 2 or rank.stride(1) != 1:
        raise SehipError("rank must be an int32 or int64 matrix with contiguous rows")
    if img.shape != pdist64.shape or rank.shape != pdist64.shape:
        raise SehipError("pdist64, img and rank must have the same shape")
    q, n = pdist64.shape
    # (a buffer of its own: the row flags the first launch leaves for the second must not meet a ranking on another stream)
    ws = _workspace(call("se_rank_refine_f64_workspace_bytes", q, n), pdist64.device, kind="refine_f64")
    call("se_rank_refine_f64", pdist64, pdist64.stride(0), img, img.stride(0), q, n, rank, _rank_width_code(rank), rank.stride(0), ws,
         ws.numel())
    return rank


def rank_rows_f64(pdist64, img, idx64=False, out=None):
    """Canonical ``np.argsort`` of float64 distances: ``rank_rows`` of their float32 image, then ``rank_refine_f64_``."""
    return rank_refine_f64_(pdist64, img, rank_rows(img, idx64=idx64, out=out))


def rank_rows_check(pdist, rank):
    """Order guard (``se_rank_rows_check``): number of rows of ``rank`` that are not the canonical ranking of ``pdist`` as far as
    adjacent entries can tell -- 0 for every output of ``rank_rows``.  Synchronises the stream."""
    require_gpu(pdist, rank)
    _f32_rows(pdist, "pdist")
    if rank.dtype not in (torch.int32, torch.int64, torch.int16) or rank.stride(1) != 1 or rank.shape != pdist.shape:
        raise SehipError("rank must be an int32 / int64 / int16 (uint16 bit patterns) matrix of pdist's shape with contiguous rows")
    q, n = pdist.shape
    ws = torch.empty((call("se_rank_rows_check_workspace_bytes"),), dtype=torch.uint8, device=pdist.device)
    bad = ctypes.c_int64(0)
    call("se_rank_rows_check", pdist, pdist.stride(0), q, n, rank, _rank_width_code(rank), rank.stride(0), ws, ws.numel(),
         ctypes.byref(bad))
    return int(bad.value)


def topk_rows(pdist, k, col_offset=0):
    """k nearest columns per row under the canonical order -> (dist [q,k] f32, idx [q,k] i32)."""
    require_gpu(pdist)
    _f32_rows(pdist, "pdist")
    q, n = pdist.shape
    od = torch.empty((q, k), dtype=torch.float32, device=pdist.device)
    oi = torch.empty((q, k), dtype=torch.int32, device=pdist.device)
    call("se_topk_rows", pdist, pdist.stride(0), q, n, int(col_offset), int(k), od, oi)
    return od, oi


def topk_merge(d, idx=None):
    """Merge per-shard lists [parts, q, k] (e.g. an all-gather result) into the global top-k.  With ``idx=None``, ``d`` is a PACKED
    int32 buffer [parts, 2, q, k] -- per part the float32 distance bits followed by the indices, the receive buffer of ONE
    all-gather (``se_topk_merge_packed``)."""
    require_gpu(d, idx)
    if idx is None and (d.dim() != 4 or d.shape[1] != 2 or d.dtype != torch.int32):
        raise SehipError("packed lists must be an int32 tensor [parts, 2, q, k]")
    d = d.contiguous()
    parts, q, k = (d.shape[0], d.shape[2], d.shape[3]) if idx is None else d.shape
    od = torch.empty((q, k), dtype=torch.float32, device=d.device)
    oi = torch.empty((q, k), dtype=torch.int32, device=d.device)
    if idx is None:
        call("se_topk_merge_packed", d, parts, q, k, od, oi)
    else:
        call("se_topk_merge", d, idx.contiguous(), parts, q, k, od, oi)
    return od, oi


def retrieve_topk(queries, gallery, k, metric=METRIC_COSINE, col_offset=0, sqq=None, sqg=None, kblocks=None, out=None):
    """Fused distances + top-k (``se_retrieve_topk``): the first k entries of every query's canonical ranking against ``gallery``
    without the [q, n] matrix; ``kblocks`` = the BLAS K-block list of ``pairwise_dist`` (D > 448).  ``out``: optional
    ``(dist f32 [q, k], idx i32 [q, k])`` contiguous destination tensors (e.g. the two halves of a packed all-gather send buffer)."""
    require_gpu(queries, gallery, sqq, sqg)
    _f32_rows(queries, "queries"); _f32_rows(gallery, "gallery")
    q, d = queries.shape
    n = gallery.shape[0]
    if gallery.shape[1] != d:
        raise SehipError("queries and gallery must have the same number of columns")
    if metric == METRIC_EUCLID:
        sqq = row_sqnorm(queries) if sqq is None else sqq
        sqg = row_sqnorm(gallery) if sqg is None else sqg
    if out is None:
        od = torch.empty((q, k), dtype=torch.float32, device=queries.device)
        oi = torch.empty((q, k), dtype=torch.int32, device=queries.device)
    else:
        od, oi = out
        require_gpu(od, oi)
        if od.dtype != torch.float32 or oi.dtype != torch.int32 or tuple(od.shape) != (q, k) or tuple(oi.shape) != (q, k) \
                or not od.is_contiguous() or not oi.is_contiguous():
            raise SehipError("out must be contiguous (float32 [q, k], int32 [q, k]) tensors")
    ws = _workspace(call("se_retrieve_topk_workspace_bytes", q, n, d, gallery.stride(0), int(k)), queries.device)
    kb, nkb = _kblocks_arg(kblocks)
    call("se_retrieve_topk", queries, queries.stride(0), gallery, gallery.stride(0), sqq, sqg, q, n, d, int(metric), kb, nkb,
         int(col_offset), int(k), od, oi, ws, ws.numel())
    return od, oi


KNN_TOP_MAX = DEFINES["SE_KNN_TOP_MAX"]     # classes se_knn_vote reports per (query, cut-off)


def knn_vote(idx, cls, num_classes, ks, top=5, qidx=None):
    """k-NN class votes over neighbour lists (``se_knn_vote``): for every query and every cut-off of ``ks``, the ``top`` classes with
    the most votes among its first k neighbours -- votes descending, ties in ascending class index, classes without a vote behind
    them in ascending index -- and their vote counts.

    idx [Q, L] int32 neighbour lists, best first, as ``retrieve_topk`` / ``topk_merge`` write them (contiguous rows; any row
    pitch); cls [N] int32; ``ks``: strictly ascending host integers in [1, L]; qidx [Q] int32 | None: the gallery index of each
    query, dropped from its list (leave-one-out).  Entries outside [0, N) are skipped.  Returns ``(out_cls, out_votes)``, int32
    ``[Q, len(ks), top]``."""
    require_gpu(idx, cls, qidx)
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.stride(1) != 1:
        raise SehipError("idx must be a 2-d int32 tensor with contiguous rows")
    _i32(cls, "cls")
    if qidx is not None:
        _i32(qidx, "qidx")
        if qidx.numel() != idx.shape[0]:
            raise SehipError("qidx must hold one gallery index per query")
    ks = [int(k) for k in ks]
    Q, L = idx.shape
    out_cls = torch.empty((Q, len(ks), int(top)), dtype=torch.int32, device=idx.device)
    out_votes = torch.empty_like(out_cls)
    ldi = idx.stride(0) if Q > 1 else max(idx.stride(0), L)
    call("se_knn_vote", idx, ldi, Q, L, cls, cls.numel(), int(num_classes), qidx, (ctypes.c_int32 * len(ks))(*ks), len(ks), int(top),
         out_cls, out_votes)
    return out_cls, out_votes


BOOTSTRAP_COLS_MAX = DEFINES["SE_BOOTSTRAP_COLS_MAX"]     # columns se_bootstrap_means resamples per call


def _seed_arg(seed):
    """A seed of up to 64 bits as the int64 that carries them across the C ABI (read there as unsigned)."""
    seed = int(seed)
    if not -(1 << 63) <= seed < (1 << 64):
        raise SehipError("seed must fit 64 bits")
    seed &= (1 << 64) - 1
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def bootstrap_means(vals, reps, seed=0, rep0=0):
    """Means of the rows of ``vals`` resampled with replacement (``se_bootstrap_means``): replicate ``rep0 + i`` draws ``q`` rows by
    the index stream pinned in include/sehip.h and row ``i`` of the result is the mean of each column over them.

    vals [q, m] float64 device tensor, any row pitch, 1 <= m <= ``BOOTSTRAP_COLS_MAX``; ``seed``: up to 64 bits.  The same
    ``(seed, q)`` draws the same queries whatever the values, and a replicate has the same bits whichever call computes it.
    A table whose rows could straddle 128-byte lines is first copied to a power-of-two pitch (m up to 16 doubles: one line per
    drawn row).  Returns float64 ``[reps, m]``."""
    require_gpu(vals)
    if vals.dtype != torch.float64 or vals.dim() != 2 or (vals.shape[1] > 1 and vals.stride(1) != 1):
        raise SehipError("vals must be a 2-d float64 tensor with contiguous rows")
    q, m = vals.shape
    reps, rep0 = int(reps), int(rep0)
    if q < 1 or not 1 <= m <= BOOTSTRAP_COLS_MAX:
        raise SehipError("vals must hold at least one row of 1 .. %d columns, not %s" % (BOOTSTRAP_COLS_MAX, tuple(vals.shape)))
    if reps < 0 or rep0 < 0:
        raise SehipError("reps and rep0 must be non-negative")
    ldv = vals.stride(0) if q > 1 else max(vals.stride(0), m)
    pitch = 1 << (m - 1).bit_length()
    if reps > 0 and q > 1 and (ldv < m or ldv % pitch or vals.data_ptr() % (8 * pitch)):
        padded = torch.empty((q, pitch), dtype=torch.float64, device=vals.device)
        padded[:, :m] = vals
        vals, ldv = padded, pitch
    out = torch.empty((reps, m), dtype=torch.float64, device=vals.device)
    call("se_bootstrap_means", vals, ldv, q, m, _seed_arg(seed), rep0, reps, out, m)
    return out


def bootstrap_indices(q, reps, seed=0, rep0=0, t0=0, count=None, device=None):
    """The index stream of ``bootstrap_means`` (``se_bootstrap_indices``): int32 ``[reps, count]``, entry ``[i, j]`` the row that
    draw ``t0 + j`` of replicate ``rep0 + i`` takes from a table of ``q`` rows.  ``count`` defaults to ``q - t0``."""
    require_gpu()
    q, reps, rep0, t0 = int(q), int(reps), int(rep0), int(t0)
    count = q - t0 if count is None else int(count)
    if reps < 0 or count < 0:
        raise SehipError("reps and count must be non-negative")
    out = torch.empty((reps, count), dtype=torch.int32, device=torch.device("cuda", _device_index(device)))
    call("se_bootstrap_indices", q, _seed_arg(seed), rep0, reps, t0, count, out, count)
    return out


COMPLETE_LDS_ITEMS = DEFINES["SE_COMPLETE_LDS_ITEMS"]     # galleries up to this size need no workspace in complete_rankings


def complete_rankings(lists, gallery, lengths=None, order=None, out=None):
    """Given ranked lists completed to rankings of the whole gallery (``se_complete_rankings``; class_hierarchy.py:262-264:
    ``ret + [id for id in all_ids if id not in sret]``).

    lists [Q, L] int32 gallery indices, best first (contiguous rows; any row pitch); ``gallery``: the number of gallery items;
    lengths [Q] int32 | None: the valid entries of each row, in [0, L] (None: all L); order [gallery] int32 | None: the
    ``all_ids`` order as gallery indices, a permutation of 0 .. gallery - 1 (None: the identity); out: int32 [Q, >= gallery]
    with contiguous rows to write into (columns ``gallery ..`` stay as they are).
    Returns ``(rank, status)``: rank [Q, gallery] int32 (a view of ``out`` when that is given), status [Q] int32 -- 0 for a clean
    row, bit 0: an entry outside [0, gallery), bit 1: an index more than once.  A row with a non-zero status holds ``order``
    itself, which means nothing: look at ``status`` before scoring."""
    require_gpu(lists, lengths, order, out)
    if lists.dtype != torch.int32 or lists.dim() != 2 or (lists.shape[1] > 0 and lists.stride(1) != 1):
        raise SehipError("lists must be a 2-d int32 tensor with contiguous rows")
    Q, L = lists.shape
    gallery = int(gallery)
    if gallery < 0:
        raise SehipError("gallery must be a non-negative number of items")
    if lengths is not None:
        _i32(lengths, "lengths")
        if lengths.numel() != Q:
            raise SehipError("lengths must hold one entry per row of lists")
    if order is not None:
        _i32(order, "order")
        if order.numel() != gallery:
            raise SehipError("order must hold the %d gallery indices, it holds %d" % (gallery, order.numel()))
    if out is None:
        out = empty_rows(Q, gallery, torch.int32, lists.device)
    elif out.dtype != torch.int32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != Q or out.shape[1] < gallery:
        raise SehipError("out must be an int32 [%d, >= %d] tensor with contiguous rows" % (Q, gallery))
    status = (torch.empty if gallery > 0 else torch.zeros)((Q,), dtype=torch.int32, device=lists.device)     # (no gallery: no launch)
    ldl = lists.stride(0) if Q > 1 and L > 0 else max(lists.stride(0), L)
    ldr = out.stride(0) if Q > 1 else max(out.stride(0), gallery)
    nbytes = call("se_complete_rankings_workspace_bytes", Q, gallery)
    ws = _workspace(nbytes, lists.device, "complete_rankings") if nbytes else None
    call("se_complete_rankings", lists if L > 0 else None, ldl, lengths, Q, L, order, gallery, out, ldr, status, ws,
         ws.numel() if ws is not None else 0)
    return out[:, :gallery], status


class HprecCurves:
    """Result of ``hprec_reciprocal_curves``: the table and the list length it covers."""
    __slots__ = ("data", "list_len")

    def __init__(self, data, list_len):
        self.data, self.list_len = data, int(list_len)


def hprec_reciprocal_curves(best_wup, best_lcs, list_len=None):
    """The best-possible curves pre-divided and laid out for ``hierarchical_precision`` (``se_hprec_reciprocal_curves``): once per
    gallery.  best_* [C, >=L] f64 -> ``HprecCurves`` (f64 [C, 2, curve_len(L), 2]); pass it as ``curves=``."""
    require_gpu(best_wup, best_lcs)
    _check_curves(best_wup, best_lcs)
    if best_wup.shape != best_lcs.shape or best_wup.stride(0) != best_lcs.stride(0):
        raise SehipError("best_wup and best_lcs must have the same shape and row stride")
    L = best_wup.shape[1] if list_len is None else int(list_len)
    C = best_wup.shape[0]
    out = torch.empty((C, 2, call("se_hprec_curve_len", L), 2), dtype=torch.float64, device=best_wup.device)
    call("se_hprec_reciprocal_curves", best_wup, best_lcs, best_wup.stride(0), C, L, out)
    return HprecCurves(out, L)


def hierarchical_precision(rank, cls, qcls, qidx, wup, lcs, best_wup, best_lcs, ks, ahp_len=-1, want_ap=False, list_len=None, curves=None,
                           class_order=None):
    """Per-query hierarchical precision metrics from device rankings (class_hierarchy.py:211-316).

    rank [Q, >=L] int32, cls [N] int32, qcls [Q] int32, qidx [Q] int32 | None, wup / lcs [C, C] f64,
    best_* [C, >=L] f64, ks [nk] int32; ``curves`` = ``hprec_reciprocal_curves(best_wup, best_lcs)`` (built here when omitted: callers
    that evaluate tile after tile build it once).  ``class_order``: visit the queries class by class (keeps the best curve in L2; same results) -- by default for
    lists of 4096 ranks and more, where it pays for the counting sort.
    Returns f64 [Q, 2 nk + 3]: P@k (WUP), P@k (LCS_HEIGHT), AHP (WUP), AHP (LCS_HEIGHT), AP."""
    require_gpu(rank, cls, qcls, wup, lcs, best_wup, best_lcs, ks)
    if rank.dtype not in (torch.int32, torch.int16) or rank.stride(1) != 1:
        raise SehipError("rank must be int32 (or int16: the uint16 bit patterns rank_rows(idx16=True) writes) with contiguous rows")
    for t, name in ((cls, "cls"), (qcls, "qcls"), (ks, "ks")):
        _i32(t, name)
    _check_curves(wup, lcs, best_wup, best_lcs)
    Q = rank.shape[0]
    L = rank.shape[1] if list_len is None else int(list_len)
    C = wup.shape[0]
    nk = ks.numel()
    if curves is None:
        curves = hprec_reciprocal_curves(best_wup, best_lcs, min(L, best_wup.shape[1]))
    if not isinstance(curves, HprecCurves) or curves.data.shape[0] != best_wup.shape[0] or curves.data.device != rank.device:
        raise SehipError("curves must come from hprec_reciprocal_curves for these best curves")
    out = torch.zeros((Q, 2 * nk + 3), dtype=torch.float64, device=rank.device)
    if class_order is None:
        class_order = L >= 4096
    order_ws = torch.empty((call("se_hprec_order_workspace_bytes", Q),), dtype=torch.uint8, device=rank.device) if class_order else None
    call("se_hierarchical_precision_r16" if rank.dtype == torch.int16 else "se_hierarchical_precision",
         rank, rank.stride(0), Q, L, cls, cls.numel(), qcls, qidx, wup, lcs, C, curves.data, curves.list_len, ks, nk,
         int(ahp_len), int(bool(want_ap)), out, out.stride(0), order_ws)
    return out


NDCG_CHUNK = DEFINES["SE_NDCG_CHUNK"]     # ranks a workgroup of se_ndcg takes per step


def ndcg_discounts(n, device=None):
    """The position weights of NDCG, ``1 / log2(p + 1)`` for p = 1 .. n, as a float64 tensor on ``device``: built by NumPy on the
    host and uploaded, so that every caller (and every test) divides by the same bits -- ``se_ndcg`` computes no logarithm."""
    disc = torch.from_numpy(1 / np.log2(np.arange(2, int(n) + 2)))
    return disc if device is None else disc.to(device)


def ndcg_ideal(gain, counts, disc, ks, full=True):
    """The ideal DCG of every query class for one gain table: float64 ``[C, 2, nk + 1]`` on ``disc``'s device, indexed
    ``[class][member][slot]``; slot t < nk is the cut-off ``ks[t]``, slot nk the whole list (0 unless ``full``).

    The ideal list of class c is row c of ``gain`` ([C, C], row = query class) sorted descending, each value repeated by the
    gallery's count of its class (``counts`` [C]); member 1 -- the query is a gallery item and is dropped from its own ranking --
    holds one item of class c fewer (where there is one).  No [C, G] list is made: with D = the float64 prefix sums of ``disc``,
    a run of equal values ``v`` over positions (start, end] contributes ``v * (D[end] - D[start])``, clipped at the cut-off, so a
    class costs its C runs plus one binary search per cut-off.  A cut-off beyond the list takes the list's end.  ``disc`` must
    reach the longest ideal list that is asked for: ``max(ks)``, or the gallery when ``full``."""
    g = gain.detach().cpu().numpy() if torch.is_tensor(gain) else np.asarray(gain)
    g = np.ascontiguousarray(g, dtype=np.float64)
    cnt = (counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)).astype(np.int64)
    C, ks = g.shape[0], [int(k) for k in ks]
    if g.shape != (C, C) or cnt.shape != (C,) or (cnt < 0).any():
        raise SehipError("gain must be [C, C] and counts [C] non-negative")
    if any(k < 1 for k in ks):
        raise SehipError("cut-offs must be >= 1")
    total = int(cnt.sum())
    reach = min(total, max([total if full else 0] + ks))
    if disc.dtype != torch.float64 or disc.dim() != 1 or disc.numel() < reach:
        raise SehipError("disc must be a float64 vector of >= %d positions" % reach)
    D = np.concatenate(([0.0], np.cumsum(disc[:reach].detach().cpu().numpy())))
    cut = np.asarray(ks + [total if full else 0], dtype=np.int64)
    out = np.zeros((C, 2, len(ks) + 1))
    order = np.argsort(-g, axis=1, kind='stable')
    for c in range(C):
        vals = g[c, order[c]]
        for member in (0, 1):
            reps = cnt[order[c]].copy()
            if member and cnt[c] > 0:
                reps[order[c] == c] -= 1
            ends = np.cumsum(reps)
            starts = ends - reps
            runs = np.concatenate(([0.0], np.cumsum(vals * (D[np.minimum(ends, reach)] - D[np.minimum(starts, reach)]))))   # whole runs in front of run r
            k = np.minimum(cut, ends[-1])                       # a cut-off beyond the list scores its end
            at = np.minimum(np.searchsorted(ends, k, side='left'), C - 1)       # the run that position k lies in
            out[c, member] = runs[at] + vals[at] * (D[k] - D[np.minimum(starts[at], k)])
    if not full:
        out[:, :, -1] = 0.0
    return torch.from_numpy(out).to(disc.device)


def ndcg(rank, cls, qcls, qidx, gain_a, gain_b, disc, ideal, ks, want_full=False, list_len=None):
    """Per-query NDCG with two class-gain tables from device rankings (``se_ndcg``; host statement: ``ClassHierarchy.ndcg``).

    rank [Q, >=L] int32, cls [N] int32, qcls [Q] int32, qidx [Q] int32 | None (gallery index of the query itself, dropped from its
    ranking; -1: not a gallery item), gain_a / gain_b [C, C] f64 (row = query class), disc [>= L] f64 (``ndcg_discounts``), ideal
    [C, 2, 2, nk + 1] f64 (``torch.stack`` of the two tables' ``ndcg_ideal`` along dim 2), ks [nk] int32 cut-offs.  Without
    ``want_full`` only the first ``max(ks) + 1`` ranks of a row are read.
    Returns f64 [Q, 2 nk + 2]: NDCG@k (a), NDCG@k (b), NDCG (a), NDCG (b); the last two are 0 unless ``want_full``."""
    require_gpu(rank, cls, qcls, qidx, gain_a, gain_b, disc, ideal, ks)
    if rank.dtype != torch.int32 or rank.dim() != 2 or rank.stride(1) != 1:
        raise SehipError("rank must be a 2-d int32 tensor with contiguous rows")
    for t, name in ((cls, "cls"), (qcls, "qcls"), (ks, "ks")) + (((qidx, "qidx"),) if qidx is not None else ()):
        _i32(t, name)
    _check_curves(gain_a, gain_b)
    Q = rank.shape[0]
    L = rank.shape[1] if list_len is None else int(list_len)
    C, nk = gain_a.shape[0], ks.numel()
    if gain_a.shape != (C, C) or gain_b.shape != (C, C) or not (gain_a.is_contiguous() and gain_b.is_contiguous()):
        raise SehipError("gain_a and gain_b must be contiguous [C, C] float64 tables")
    if disc.dtype != torch.float64 or disc.dim() != 1 or not disc.is_contiguous():
        raise SehipError("disc must be a contiguous float64 vector")
    if ideal.dtype != torch.float64 or tuple(ideal.shape) != (C, 2, 2, nk + 1) or not ideal.is_contiguous():
        raise SehipError("ideal must be a contiguous float64 [C, 2, 2, nk + 1] tensor, C = %d, nk = %d" % (C, nk))
    if L > rank.shape[1] or qcls.numel() != Q or (qidx is not None and qidx.numel() != Q):
        raise SehipError("list_len exceeds the rankings, or qcls / qidx do not have one entry per row")
    out = torch.zeros((Q, 2 * nk + 2), dtype=torch.float64, device=rank.device)
    call("se_ndcg", rank, rank.stride(0) if Q > 1 else max(rank.stride(0), L), Q, L, cls, cls.numel(), qcls, qidx, gain_a, gain_b, C,
         disc, disc.numel(), ideal, ks, nk, int(bool(want_full)), out, out.stride(0))
    return out


def relevant_positions(rank, cls, qcls, qidx, hit_off, list_len=None, out=None, num_classes=None, total=None):
    """1-based positions (query removed) of the items of each query's class in its ranking (plot_recall_precision.py:52-79).

    rank [Q, >=L] int32 (or int16: the uint16 bit patterns rank_rows(idx16=True) writes), cls [N] int32 class of every gallery
    item, qcls [Q] int32, qidx [Q] int32 | None (gallery index of the query, dropped from its ranking), hit_off [Q + 1] int64 (prefix
    sum of R_i, the relevant items of query i).  Returns int32 [hit_off[Q]]: the positions of query i at hit_off[i] .. hit_off[i + 1].
    ``num_classes`` (classes are 0 .. num_classes - 1) and ``total`` (= hit_off[Q]) spare the two device reads that find them
    otherwise; callers that evaluate tile after tile know both on the host."""
    require_gpu(rank, cls, qcls, qidx, hit_off, out)
    if rank.dtype not in (torch.int32, torch.int16) or rank.dim() != 2 or rank.stride(1) != 1:
        raise SehipError("rank must be a 2-d int32 (or int16) tensor with contiguous rows")
    for t, name in ((cls, "cls"), (qcls, "qcls")) + (((qidx, "qidx"),) if qidx is not None else ()):
        _i32(t, name)
    _i64(hit_off, "hit_off")
    Q = rank.shape[0]
    if qcls.numel() != Q or hit_off.numel() != Q + 1 or (qidx is not None and qidx.numel() != Q):
        raise SehipError("qcls / qidx need one entry per ranking row and hit_off one more")
    L = rank.shape[1] if list_len is None else int(list_len)
    total = int(total) if total is not None else (int(hit_off[-1].item()) if Q > 0 else 0)
    if out is None:
        out = torch.empty((max(total, 1),), dtype=torch.int32, device=rank.device)
    else:
        _i32(out, "out")
        if out.numel() < total:
            raise SehipError("out holds %d positions, hit_off asks for %d" % (out.numel(), total))
    if num_classes is not None:
        C = int(num_classes)
    else:
        C = int(max(int(cls.max().item()), int(qcls.max().item()) if Q > 0 else 0)) + 1 if cls.numel() > 0 else 1
    call("se_relevant_positions_r16" if rank.dtype == torch.int16 else "se_relevant_positions",
         rank, rank.stride(0), Q, L, cls, cls.numel(), qcls, qidx, C, hit_off, out)
    return out[:total]


def recall_precision_reduce(hit_pos, hit_off, order, class_start, class_off, bins, ap, prec_sum, first_miss, bin_sum=None,
                            bin_count=None):
    """Per-query AP and per-class recall-precision sums of one tile (se_recall_precision_reduce; plot_recall_precision.py:52-79).

    hit_pos / hit_off: from ``relevant_positions``; order [Q] int32 (queries sorted by class, stable), class_start [C + 1] int32,
    class_off [C + 1] int64 (prefix sum of the per-class R).  Writes ap [Q] f64; ADDS to prec_sum [class_off[C]] f64,
    first_miss [C] int64 and, with bins > 0, bin_sum [C, bins + 1] f64 / bin_count [C, bins + 1] int64 (accumulate tiles in order)."""
    bins = int(bins or 0)
    require_gpu(hit_pos, hit_off, order, class_start, class_off, ap, prec_sum, first_miss, bin_sum, bin_count)
    _i32(hit_pos, "hit_pos"); _i32(order, "order"); _i32(class_start, "class_start")
    _i64(hit_off, "hit_off"); _i64(class_off, "class_off"); _i64(first_miss, "first_miss")
    for t, name in ((ap, "ap"), (prec_sum, "prec_sum")) + (((bin_sum, "bin_sum"),) if bins > 0 else ()):
        if t is None or t.dtype != torch.float64 or not t.is_contiguous():
            raise SehipError("%s must be contiguous float64" % name)
    Q = order.numel()
    C = class_start.numel() - 1
    if C < 1 or class_off.numel() != C + 1 or first_miss.numel() != C or hit_off.numel() != Q + 1 or ap.numel() != Q:
        raise SehipError("recall_precision_reduce: inconsistent shapes (Q = %d, C = %d)" % (Q, C))
    class_len = prec_sum.numel()
    if bins > 0:
        _i64(bin_count, "bin_count")
        if bin_sum.numel() != C * (bins + 1) or bin_count.numel() != C * (bins + 1):
            raise SehipError("bin_sum / bin_count must hold [C, bins + 1] entries")
    call("se_recall_precision_reduce", hit_pos, hit_off, Q, order, class_start, C, class_off, class_len, bins, ap, prec_sum,
         first_miss, bin_sum if bins > 0 else None, bin_count if bins > 0 else None)
    return ap


def count_preceding(pdist, col_offset, hit_off, rel_d, rel_i, qidx, cnt, max_rel=0):
    """Count one distance slab into the per-relevant-item histogram ``cnt`` (``se_count_preceding``): the positions of a query's
    relevant items in a gallery it is not ranked against in full.

    pdist [Q, n_cols] f32 (distances to gallery rows ``col_offset ..``), hit_off [Q + 1] int64, rel_d f32 / rel_i int32
    [hit_off[Q]] (the relevant items' keys, per query ascending in the canonical order), qidx [Q] int32 | None (global gallery index
    of the query itself, < 0: not in the gallery), cnt int32 [>= hit_off[Q]] in/out (zero before the first slab); ``max_rel``: the
    longest key list, when the caller knows it.  Slabs and shards accumulate in any order.  Returns ``cnt``."""
    require_gpu(pdist, hit_off, rel_d, rel_i, qidx, cnt)
    _f32_rows(pdist, "pdist")
    _i64(hit_off, "hit_off"); _i32(rel_i, "rel_i"); _i32(cnt, "cnt")
    if qidx is not None:
        _i32(qidx, "qidx")
    if rel_d.dtype != torch.float32 or not rel_d.is_contiguous():
        raise SehipError("rel_d must be contiguous float32")
    Q, n_cols = pdist.shape
    if hit_off.numel() != Q + 1 or (qidx is not None and qidx.numel() != Q) or rel_d.numel() != rel_i.numel() or cnt.numel() < rel_d.numel():
        raise SehipError("count_preceding: hit_off needs Q + 1 entries, qidx Q, and rel_d / rel_i / cnt one per relevant item")
    call("se_count_preceding", pdist, pdist.stride(0), Q, n_cols, int(col_offset), hit_off, rel_d, rel_i, qidx, int(max_rel), cnt)
    return cnt


def count_to_positions(cnt, hit_off, out=None):
    """``se_count_to_positions``: per-query inclusive prefix sum of the bins ``count_preceding`` filled -> the 1-based positions
    (query removed) ``relevant_positions`` would have read off a full ranking.  ``out`` may be ``cnt`` itself (the default)."""
    require_gpu(cnt, hit_off, out)
    _i32(cnt, "cnt"); _i64(hit_off, "hit_off")
    out = cnt if out is None else out
    _i32(out, "out")
    if out.numel() < cnt.numel():
        raise SehipError("out holds %d positions, cnt %d" % (out.numel(), cnt.numel()))
    call("se_count_to_positions", cnt, hit_off, hit_off.numel() - 1, out)
    return out


# --------------------------------------------------------------------------------------------
# classification side: linear SVM (svm.hip; the solver is linear_svm.py)
# --------------------------------------------------------------------------------------------

def svm_margin(mode, x, w, d=None, labels=None, col_class=None, cpen=1.0, mask=None, out=None, loss_part=None):
    """``se_svm_margin``: margins x w[:, :d]^T + w[:, d] with the fused epilogue of ``mode`` (SVM_GRAD / SVM_HV / SVM_SCORE).

    x [N, >= d] float32, w [C, >= d + 1] float32 (bias in column d; d defaults to w.shape[1] - 1).  SVM_GRAD needs labels [N] /
    col_class [C] int32, mask [N, >= ceil(C / 32)] int32 (written) and loss_part [C, >= se_svm_loss_blocks(N)] float32 (written);
    SVM_HV reads mask.  Returns ``out`` [N, C] float32 (Z, Z' or the scores)."""
    require_gpu(x, w, labels, col_class, mask, out, loss_part)
    d = w.shape[1] - 1 if d is None else int(d)
    ldx, ldw = _f32_2d(x, "x", d), _f32_2d(w, "w", d + 1)
    N, C = x.shape[0], w.shape[0]
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    ldo = _f32_2d(out, "out", C)
    ldm = 0
    if mask is not None:
        if mask.dtype != torch.int32 or mask.dim() != 2 or mask.stride(1) != 1:
            raise SehipError("mask must be a 2-d int32 tensor with contiguous rows")
        ldm = mask.stride(0) if mask.shape[0] > 1 else mask.shape[1]
    for t, name in ((labels, "labels"), (col_class, "col_class")):
        if t is not None:
            _i32(t, name)
    ldl = _f32_2d(loss_part, "loss_part", 1) if loss_part is not None else 0
    call("se_svm_margin", int(mode), x, ldx, N, d, w, ldw, C, labels, col_class, float(cpen), mask, ldm, out, ldo, loss_part, ldl)
    return out


def svm_loss_blocks(n):
    return call("se_svm_loss_blocks", int(n))


def svm_reduce_workspace_bytes(n, d, c):
    return call("se_svm_reduce_workspace_bytes", int(n), int(d), int(c))


def svm_reduce(z, x, d=None, plus=None, out=None, workspace=None):
    """``se_svm_reduce``: out [C, d + 1] = plus + z^T [x[:, :d] | 1] (fp32 partials over fixed row slices, fp64 combine).
    z [N, >= C] float32 (C = out.shape[0], or z.shape[1] when out is None), x [N, >= d] float32."""
    require_gpu(z, x, plus, out, workspace)
    d = x.shape[1] if d is None else int(d)
    N = x.shape[0]
    C = out.shape[0] if out is not None else z.shape[1]
    ldz, ldx = _f32_2d(z, "z", C), _f32_2d(x, "x", d)
    if z.shape[0] != N:
        raise SehipError("z and x need the same number of rows")
    if out is None:
        out = torch.empty((C, d + 1), dtype=torch.float32, device=x.device)
    ldg = _f32_2d(out, "out", d + 1)
    ldp = _f32_2d(plus, "plus", d + 1) if plus is not None else 0
    need = svm_reduce_workspace_bytes(N, d, C)
    ws = _workspace(need, x.device) if workspace is None else workspace
    call("se_svm_reduce", z, ldz, x, ldx, N, d, C, plus, ldp, out, ldg, ws, ws.numel())
    return out


def svm_gram(vecs, length=None, out=None):
    """``se_svm_gram``: per-row fp64 dot products of 1..4 float32 [C, >= length] tensors with one leading dimension ->
    float64 [C, nv (nv + 1) / 2] (pairs (a, b), a <= b, row-major)."""
    vecs = list(vecs)
    require_gpu(*vecs)
    if not 1 <= len(vecs) <= 4:
        raise SehipError("svm_gram takes 1 to 4 vectors")
    length = vecs[0].shape[1] if length is None else int(length)
    lds = {_f32_2d(v, "vector", length) for v in vecs}
    if len(lds) != 1 or any(v.shape[0] != vecs[0].shape[0] for v in vecs):
        raise SehipError("svm_gram: the vectors need one shape and one leading dimension")
    C, nv = vecs[0].shape[0], len(vecs)
    if out is None:
        out = torch.empty((C, nv * (nv + 1) // 2), dtype=torch.float64, device=vecs[0].device)
    call("se_svm_gram", *(vecs + [None] * (4 - nv)), nv, lds.pop(), C, length, out)
    return out


def svm_rowsum(a, length=None, out=None):
    """``se_svm_rowsum``: fp64 sum of every row of a float32 [C, >= length] tensor."""
    require_gpu(a, out)
    length = a.shape[1] if length is None else int(length)
    lda = _f32_2d(a, "a", length)
    if out is None:
        out = torch.empty((a.shape[0],), dtype=torch.float64, device=a.device)
    call("se_svm_rowsum", a, lda, a.shape[0], length, out)
    return out


def svm_axpby(alpha, x, beta, y, out=None, length=None):
    """``se_svm_axpby``: out = alpha[:, None] x + beta[:, None] y over the first ``length`` columns, in fp64, rounded to float32.
    alpha / beta: float64 [C] device tensors; out may be x or y."""
    require_gpu(alpha, x, beta, y, out)
    length = x.shape[1] if length is None else int(length)
    for t, name in ((alpha, "alpha"), (beta, "beta")):
        if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != x.shape[0]:
            raise SehipError("%s must be a contiguous float64 tensor with one entry per row" % name)
    if out is None:
        out = torch.zeros_like(x)
    ldx, ldy, ldo = _f32_2d(x, "x", length), _f32_2d(y, "y", length), _f32_2d(out, "out", length)
    call("se_svm_axpby", alpha, x, ldx, beta, y, ldy, x.shape[0], length, out, ldo)
    return out


# --------------------------------------------------------------------------------------------
# class embeddings: similarity tables of a hierarchy, Cholesky factor, symmetric eigensolver (classemb.hip, eigh.hip; the CLI is
# compute_class_embedding.py)
# --------------------------------------------------------------------------------------------

def class_pair_tables(off, rank, spl, depth, height, max_anc, max_height, diag_one=False, distance=False, want_wup=True,
                      want_lcs=True):
    """``se_class_pair_tables`` over the encoding of ``ClassHierarchy.pair_table_encoding`` (contiguous int32 device tensors).
    Returns ``(wup, lcs, missing)``: float64 [C, C] tables (None when not wanted) and an int64 [1] device tensor holding
    i C + j of the first pair without a common ancestor, or -1.  ``distance``: lcs holds h / H; ``diag_one``: lcs diagonal 1
    (0 with ``distance``)."""
    require_gpu(off, rank, spl, depth, height)
    for t, name in ((off, "off"), (rank, "rank"), (spl, "spl"), (depth, "depth"), (height, "height")):
        _i32(t, name)
    if rank.numel() != spl.numel() or depth.numel() != height.numel():
        raise SehipError("class_pair_tables: rank / spl and depth / height need one length each")
    if not (want_wup or want_lcs):
        raise SehipError("class_pair_tables: no table requested")
    C = off.numel() - 1
    dev = off.device
    wup = torch.empty((C, C), dtype=torch.float64, device=dev) if want_wup else None
    lcs = torch.empty((C, C), dtype=torch.float64, device=dev) if want_lcs else None
    missing = torch.empty((1,), dtype=torch.int64, device=dev)
    flags = (DEFINES["SE_CLASSEMB_DIAG_ONE"] if diag_one else 0) | (DEFINES["SE_CLASSEMB_DIST"] if distance else 0)
    call("se_class_pair_tables", off, rank, spl, rank.numel(), C, int(max_anc), depth, height, depth.numel(), int(max_height), flags,
         wup, max(C, 1), lcs, max(C, 1), missing)
    return wup, lcs, missing


def cholesky_lower_(a, info=None):
    """``se_cholesky_f64`` in place on a float64 [n, n] device tensor with contiguous rows: the lower Cholesky factor, exact zeros
    above the diagonal.  Returns ``(a, info)``: info an int32 [1] device tensor, -1 on success, else the first row (0-based)
    whose pivot was <= 0 or NaN -- that row's diagonal and every later row are NaN.  Nothing is synchronised."""
    require_gpu(a, info)
    if a.dtype != torch.float64 or a.dim() != 2 or a.shape[0] != a.shape[1] or (a.shape[0] > 1 and a.stride(1) != 1):
        raise SehipError("cholesky_lower_ takes a square float64 matrix with contiguous rows")
    n = a.shape[0]
    if info is None:
        info = torch.empty((1,), dtype=torch.int32, device=a.device)
    _i32(info, "info")
    call("se_cholesky_f64", a, a.stride(0) if n > 1 else max(n, 1), n, info)
    return a, info


EIGH_NOT_CONVERGED, EIGH_NONFINITE = DEFINES["SE_EIGH_NOT_CONVERGED"], DEFINES["SE_EIGH_NONFINITE"]


def eigh_schedule(nb):
    """The rounds of one sweep of ``se_eigh_f64`` over ``nb`` blocks (even, >= 2): a list of nb - 1 rounds, each a list of nb / 2
    disjoint pairs ``(lo, hi)``, lo < hi, every unordered pair of blocks exactly once per sweep.  The circle method: round r pairs
    block r with block nb - 1 and, for k = 1 .. nb / 2 - 1, block (r + k) mod (nb - 1) with block (r - k) mod (nb - 1).  Pure
    Python (the library's ``se_eigh_schedule`` and its kernels follow the same rule; tests/test_eigh_host.py compares them)."""
    nb = int(nb)
    if nb < 2 or nb % 2:
        raise SehipError("eigh_schedule: nb=%d must be even and >= 2" % nb)
    m = nb - 1
    return [[(r, m)] + [tuple(sorted(((r + k) % m, (r - k) % m))) for k in range(1, nb // 2)] for r in range(m)]


def eigh(a, max_sweeps=60, overwrite_a=False, out_v=None):
    """``se_eigh_f64`` of a symmetric float64 [n, n] device matrix with contiguous rows (any row pitch): ``(w, v, info)`` with
    ``w`` [n] ascending, ``v`` [n, n] whose column j belongs to ``w[j]`` (numpy.linalg.eigh's conventions; signs and the basis
    of a degenerate cluster unspecified) and ``info`` a Python int: the sweeps used, or ``EIGH_NOT_CONVERGED`` (w / v finite,
    the state after ``max_sweeps``) or ``EIGH_NONFINITE`` (NaN / infinite input; w / v NaN).  ``a`` is copied unless
    ``overwrite_a``; ``max_sweeps`` bounds the outer loop (random matrices take 5 to 8 sweeps, the clustered class similarities
    28 at n = 1,000 and 8,142: the default leaves twice that); ``out_v`` may name the [n, n] float64 destination (contiguous rows, any pitch).  Synchronises the stream."""
    require_gpu(a, out_v)
    if a.dtype != torch.float64 or a.dim() != 2 or a.shape[0] != a.shape[1] or (a.shape[0] > 1 and a.stride(1) != 1):
        raise SehipError("eigh takes a square float64 matrix with contiguous rows")
    n = a.shape[0]
    if not overwrite_a:
        a = a.clone(memory_format=torch.contiguous_format)
    v = torch.empty((n, n), dtype=torch.float64, device=a.device) if out_v is None else out_v
    if v.dtype != torch.float64 or tuple(v.shape) != (n, n) or (n > 1 and v.stride(1) != 1):
        raise SehipError("eigh: out_v must be a float64 [n, n] matrix with contiguous rows")
    w = torch.empty((n,), dtype=torch.float64, device=a.device)
    info = torch.empty((1,), dtype=torch.int32, device=a.device)
    nbytes = call("se_eigh_f64_workspace_bytes", n)
    if nbytes < 0:
        raise SehipError("eigh: n=%d is out of range" % n)
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=a.device)
    call("se_eigh_f64", a, a.stride(0) if n > 1 else max(n, 1), n, w, v, v.stride(0) if n > 1 else max(n, 1), ws, info, int(max_sweeps))
    return w, v, int(info.item())


# --------------------------------------------------------------------------------------------
# input pipeline: batches of file-based datasets composed on the device (image_batch.hip; the generators are datasets/files.py)
# --------------------------------------------------------------------------------------------

_RESAMPLE_BITS = 22        # Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)


def _axis_tables(src, dst, crop, offs, pad, flip):
    """Tables of one axis for a whole batch: ``(map [B, crop, 3] = (u, first source index, taps), weights [B, crop, K])``."""
    src, dst, offs, pad = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (src, dst, offs, pad))
    if src.size and (src.min() < 1 or dst.min() < 1):
        raise SehipError("resample_tables: image sizes must be positive")
    # output coordinate -> coordinate u in the zoomed, flipped image: crop offset, then np.pad(..., 'reflect') of period 2 (n - 1)
    p = np.arange(crop, dtype=np.int64)[None, :] + (offs - pad)[:, None]
    period = np.maximum(2 * (dst - 1), 1)[:, None]
    m = np.mod(p, period)
    u = np.where(m < dst[:, None], m, period - m)
    idx = u if flip is None else np.where(np.asarray(flip, dtype=bool).reshape(-1, 1), dst[:, None] - 1 - u, u)
    # Pillow's precompute_coeffs (bilinear: support 1), in its order of operations, float64
    same = src == dst
    scale = src.astype(np.float64) / dst.astype(np.float64)
    fs = np.maximum(scale, 1.0)
    support = fs * 1.0
    taps = np.ceil(support).astype(np.int64) * 2 + 1
    K = int(np.max(np.where(same, 1, taps))) if src.size else 1
    center = (idx + 0.5) * scale[:, None]
    ss = 1.0 / fs
    lo = np.maximum((center - support[:, None] + 0.5).astype(np.int64), 0)
    hi = np.minimum((center + support[:, None] + 0.5).astype(np.int64), src[:, None])
    n = hi - lo
    i = np.arange(K, dtype=np.int64)[None, None, :]
    w = np.abs(((i + lo[:, :, None]) - center[:, :, None] + 0.5) * ss[:, None, None])
    w = np.where((w < 1.0) & (i < n[:, :, None]), 1.0 - w, 0.0)
    ww = np.cumsum(w, axis=2)[:, :, -1:]                         # summed in order, like the C loop
    w = np.divide(w, ww, out=w.copy(), where=ww != 0.0)
    k = (0.5 + w * float(1 << _RESAMPLE_BITS)).astype(np.int64)
    # an axis whose size does not change is not resampled by Pillow: the single tap reproduces the pixel
    sm = same[:, None]
    lo = np.where(sm, idx, lo)
    n = np.where(sm, 1, n)
    one = np.zeros((1, 1, K), dtype=np.int64)
    one[0, 0, 0] = 1 << _RESAMPLE_BITS
    k = np.where(sm[:, :, None], one, k)
    return np.stack((u, lo, n), axis=2).astype(np.int32), np.ascontiguousarray(k.astype(np.int32))


def resample_tables(src_sizes, dst_sizes, crop, offsets=None, pads=None, flips=None):
    """The tables ``se_image_batch`` resamples with, for a whole batch, in vectorised NumPy float64 on the HOST (the device's float64
    with possible FMA contraction would not reproduce Pillow's quantised weights).

    ``src_sizes`` [B, 2] = (h, w) of the stored images, ``dst_sizes`` [B, 2] = (H', W') of the zoomed images, ``crop`` = (ch, cw),
    ``offsets`` [B, 2] = (y, x) of the crop window in the zoomed image (an axis larger than the crop), ``pads`` [B, 2] = (y, x) rows /
    columns of reflect padding in front (an axis smaller than the crop), ``flips`` [B] horizontal flips.  The tables are indexed by
    OUTPUT coordinate: crop offset, reflect padding (``np.pad(..., 'reflect')``: period 2 (n - 1), a size-1 axis repeats) and flip are
    applied by gathering rows of Pillow's coefficient table (``PIL.Image.resize(size, BILINEAR)``: ImagingResample's
    precompute_coeffs + normalize_coeffs_8bpc).  Returns ``(xmap [B, cw, 3], xk [B, cw, Kx], ymap [B, ch, 3], yk [B, ch, Ky])`` int32."""
    src = np.asarray(src_sizes, dtype=np.int64).reshape(-1, 2)
    dst = np.asarray(dst_sizes, dtype=np.int64).reshape(-1, 2)
    B = src.shape[0]
    offs = np.zeros((B, 2), np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64).reshape(-1, 2)
    pad = np.zeros((B, 2), np.int64) if pads is None else np.asarray(pads, dtype=np.int64).reshape(-1, 2)
    if not (dst.shape[0] == offs.shape[0] == pad.shape[0] == B):
        raise SehipError("resample_tables: one row per sample in every argument")
    ch, cw = int(crop[0]), int(crop[1])
    ymap, yk = _axis_tables(src[:, 0], dst[:, 0], ch, offs[:, 0], pad[:, 0], None)
    xmap, xk = _axis_tables(src[:, 1], dst[:, 1], cw, offs[:, 1], pad[:, 1], flips)
    return xmap, xk, ymap, yk


def image_batch(arena, src_off, src_hw, xmap, xk, ymap, yk, erase, seed, mean, std, bgr=False, dtype=torch.float32, out=None):
    """``se_image_batch``: one launch composes the batch from the uint8 ``arena`` (see include/sehip.h for every argument; all device
    tensors: ``src_off`` int64 [B], ``seed`` int32 / uint32 bit patterns [B], ``mean`` / ``std`` float32 [3], the rest int32).
    Returns ``out`` [B, ch, cw, 3] (NHWC) of ``dtype`` float32 or bfloat16; ``out.permute(0, 3, 1, 2)`` is the channels_last batch."""
    require_gpu(arena, src_off, src_hw, xmap, xk, ymap, yk, erase, seed, mean, std, out)
    if arena.dtype != torch.uint8 or not arena.is_contiguous():
        raise SehipError("image_batch: the arena must be a contiguous uint8 tensor")
    _i64(src_off, "src_off")
    for t, name in ((src_hw, "src_hw"), (xmap, "xmap"), (xk, "xk"), (ymap, "ymap"), (yk, "yk"), (erase, "erase")):
        _i32(t, name)
    if not seed.is_contiguous() or not mean.is_contiguous() or not std.is_contiguous() or mean.numel() != 3 or std.numel() != 3:
        raise SehipError("image_batch: seed must be contiguous, mean / std contiguous float32 [3]")
    B = src_off.numel()
    if xmap.dim() != 3 or ymap.dim() != 3 or xk.dim() != 3 or yk.dim() != 3 or xmap.shape[2] != 3 or ymap.shape[2] != 3:
        raise SehipError("image_batch: xmap / ymap must be [B, crop, 3], xk / yk [B, crop, K]")
    ch, cw, Kx, Ky = ymap.shape[1], xmap.shape[1], xk.shape[2], yk.shape[2]
    if not (xmap.shape[0] == ymap.shape[0] == xk.shape[0] == yk.shape[0] == B) or xk.shape[1] != cw or yk.shape[1] != ch \
            or src_hw.numel() != 2 * B or erase.numel() != 4 * B or seed.numel() != B:
        raise SehipError("image_batch: the tables do not describe one batch of %d samples" % B)
    if dtype not in (torch.float32, torch.bfloat16):
        raise SehipError("image_batch: output must be float32 or bfloat16, got %s" % dtype)
    if out is None:
        out = torch.empty((B, ch, cw, 3), dtype=dtype, device=arena.device)
    elif out.dtype != dtype or tuple(out.shape) != (B, ch, cw, 3) or not out.is_contiguous():
        raise SehipError("image_batch: out must be a contiguous [B, ch, cw, 3] tensor of the requested dtype")
    call("se_image_batch", arena, arena.numel(), src_off, src_hw, xmap, xk, ymap, yk, erase, seed, mean, std, int(bool(bgr)), out,
         DTYPE_F32 if dtype == torch.float32 else DTYPE_BF16, B, ch, cw, Kx, Ky)
    return out


TINY_BATCH_MAX_BLOCKS = DEFINES["SE_TINY_BATCH_MAX_BLOCKS"]
FILL_MODES = {"nearest": DEFINES["SE_FILL_NEAREST"], "constant": DEFINES["SE_FILL_CONSTANT"], "reflect": DEFINES["SE_FILL_REFLECT"]}


def tiny_batch(images, index, affine, flags, mean, stdp, fill_mode="nearest", cval=0.0, dtype=torch.float32, out=None):
    """``se_tiny_batch``: one launch composes the batch from the float32 store ``images`` [N, H, W, C] (see include/sehip.h for every
    argument; all device tensors: ``index`` int64 [B], ``affine`` float64 [B, 6], ``flags`` int32 [B] (bit 0 horizontal, bit 1 vertical
    flip), ``mean`` / ``stdp`` float32 [C]); ``fill_mode`` 'nearest', 'constant' or 'reflect'.
    Returns ``out`` [B, H, W, C] (NHWC) of ``dtype`` float32 or bfloat16; ``out.permute(0, 3, 1, 2)`` is the channels_last batch."""
    require_gpu(images, index, affine, flags, mean, stdp, out)
    if images.dtype != torch.float32 or images.dim() != 4 or not images.is_contiguous():
        raise SehipError("tiny_batch: the store must be a contiguous float32 [N, H, W, C] tensor")
    N, H, W, C = images.shape
    if not 1 <= C <= 4 or H < 1 or W < 1:
        raise SehipError("tiny_batch: images of %d x %d x %d: 1 to 4 channels and at least one pixel" % (H, W, C))
    _i64(index, "index")
    _i32(flags, "flags")
    B = index.numel()
    if affine.dtype != torch.float64 or not affine.is_contiguous() or tuple(affine.shape) != (B, 6):
        raise SehipError("tiny_batch: affine must be a contiguous float64 [B, 6] tensor")
    if index.dim() != 1 or tuple(flags.shape) != (B,):
        raise SehipError("tiny_batch: index and flags must be [B]")
    for t, name in ((mean, "mean"), (stdp, "stdp")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C:
            raise SehipError("tiny_batch: %s must be contiguous float32 [%d]" % (name, C))
    if fill_mode not in FILL_MODES:
        raise SehipError("tiny_batch: fill_mode must be one of %s, got %r" % (sorted(FILL_MODES), fill_mode))
    if dtype not in (torch.float32, torch.bfloat16):
        raise SehipError("tiny_batch: output must be float32 or bfloat16, got %s" % dtype)
    if out is None:
        out = torch.empty((B, H, W, C), dtype=dtype, device=images.device)
    elif out.dtype != dtype or tuple(out.shape) != (B, H, W, C) or not out.is_contiguous():
        raise SehipError("tiny_batch: out must be a contiguous [B, H, W, C] tensor of the requested dtype")
    call("se_tiny_batch", images, N, index, affine, flags, mean, stdp, FILL_MODES[fill_mode], float(cval), out,
         DTYPE_F32 if dtype == torch.float32 else DTYPE_BF16, B, H, W, C)
    return out
