// joint_head.hip -- the head of `--cls_weight`: embedding loss, cross-entropy of the classifier branch and the metrics of both
// outputs in ONE forward launch, both gradients in one backward launch (reference: learn_image_embeddings.py:160-180 with
// utils.inv_correlation, utils.py:44-46; utils.nn_accuracy, utils.py:57-100; utils.top_k_acc, utils.py:49-54; Keras 2.2's
// 'categorical_crossentropy' and 'accuracy').
//
// Two roles share a grid; which one a workgroup plays is decided by its block index alone (workgroup-uniform):
//   embedding role   blocks [0, emb_blocks)
//       nearest-class metric: head::head_strip<2> of embed_head.h -- a strip of 32 samples against a slice of the class tiles, the
//           loss rows (1 - p . emb[y], the dt of row_reduce) taken by the first slice.  p is used as it comes: the model's l2norm /
//           softmax layer has normalised it where the loss asks for that, and the classifier branch reads the same tensor.
//       arg-max metric: a wave per row of p, one scan for the arg-max class and the number of entries above the label's, with the
//           non-finite rules of the cross-entropy's best / above (softmax_xent.h); the loss is the row chain again, or the single
//           operation 1 - p[y] against the identity table of `--embedding onehot` (emb == NULL).
//   classifier role  blocks [emb_blocks, emb_blocks + cls_blocks)
//       xe_fwd_reg_rows / xe_bwd_rows of softmax_xent.h: the very row code of se_softmax_xent_fwd / _bwd, smoothing 0.
// Each role's results depend on its own inputs only, so the bits are those of the separate entry points whatever the geometry.
// The forward register paths end at C = 8192; longer rows of logits go to se_softmax_xent_fwd's streaming kernel as a second launch.
#include "embed_head.h"
#include "softmax_xent.h"

namespace se {
namespace joint {

constexpr int ROWS_PER_BLOCK = 4;       // wave-per-row roles: 4 waves = 256 threads

struct FwdArgs {
    // embedding role
    const float *p; int64_t ldp;
    const int64_t *labels;
    const float *emb; int64_t lde;
    int64_t B, D, C;
    float *emb_loss_i;
    int32_t *n_better, *n_within, *p_best, *p_above;
    float *scores; int64_t lds;
    int loss_vec, p_vec, e_vec, tiles_per_block;
    unsigned strips, slices, emb_blocks;
    unsigned long long *part_best; uint32_t *part_cnt, *ticket;
    // classifier role
    const void *logits; int64_t ldz;
    float *cls_loss_i, *aux;
    int32_t *z_best, *z_above;
};

// arg-max metric: one wave per row of p [B, D], D == C
__device__ __forceinline__ void argmax_row(const FwdArgs &a, int64_t row)
{
    const int lane = lane_id();
    const float *prow = a.p + row * a.ldp;
    const int64_t y = clamp_label(a.labels[row], a.C);
    const float py = prow[y];
    float m = -INFINITY;
    int am = INT_MAX, nan_at = INT_MAX, cnt = 0;
    auto see = [&](float x, int c) {                       // a lane's columns ascend: its first maximum stays
        if (x != x) nan_at = min(nan_at, c);
        if (x > m) { m = x; am = c; }
        cnt += x > py ? 1 : 0;
    };
    if (a.p_vec) {
        const float4 *pv = (const float4 *)prow;
        for (int64_t i = lane; i < a.D / 4; i += WAVE) {
            const float4 q = pv[i];
            const int c = (int)(4 * i);
            see(q.x, c); see(q.y, c + 1); see(q.z, c + 2); see(q.w, c + 3);
        }
    } else {
        for (int64_t i = lane; i < a.D; i += WAVE) see(prow[i], (int)i);
    }
    const float M = wave_max(m);
    nan_at = wave_min(nan_at);
    const int cand = wave_min(m == M ? am : INT_MAX);
    cnt = wave_sum(cnt);
    float loss;
    if (a.emb) {
        float ss, dt;
        row_reduce<false>(prow, a.emb + y * a.lde, a.D, a.loss_vec != 0, ss, dt);
        loss = 1.0f - dt;
    } else {
        loss = 1.0f - py;
    }
    if (lane == 0) {
        a.emb_loss_i[row] = loss;
        if (a.p_best) a.p_best[row] = xe_best_class(nan_at, cand);
        a.p_above[row] = xe_bad_row(nan_at, M) ? (int32_t)a.C : cnt;
    }
}

// METRIC: SE_HEAD_METRIC_*;  ZBF / ZVEC / G: dtype, 16-byte loads and threads per row (64: C <= 1024, 256: C <= 8192) of the logits
template <int METRIC, bool ZBF, bool ZVEC, int G>
__global__ __launch_bounds__(256) void joint_head_fwd_kernel(const FwdArgs a)
{
    const unsigned b = blockIdx.x;
    if (b < a.emb_blocks) {
        if constexpr (METRIC == SE_HEAD_METRIC_NEAREST) {
            head::head_strip<2, false>(b % a.strips, b / a.strips, a.slices, a.p, a.ldp, a.labels, a.emb, a.lde, a.B, a.D, a.C, nullptr, 0,
                                       nullptr, a.emb_loss_i, nullptr, a.n_better, a.n_within, a.p_best, a.scores, a.lds, a.loss_vec, a.p_vec,
                                       a.e_vec, a.tiles_per_block, a.part_best, a.part_cnt, a.ticket);
        } else {
            const int64_t row = (int64_t)b * ROWS_PER_BLOCK + (threadIdx.x >> 6);
            if (row < a.B) argmax_row(a, row);
        }
        return;
    }
    xe_fwd_reg_rows<ZBF, ZVEC, G, G == 64 ? XE_WAVE_NV : XE_BLOCK_NV>(b - a.emb_blocks, a.logits, a.ldz, a.labels, a.B, (int)a.C, 1.0f, 0.0f,
                                                                     a.cls_loss_i, a.aux, a.z_best, a.z_above);
}

struct BwdArgs {
    const int64_t *labels;
    const float *emb; int64_t lde;
    int64_t B, D, C;
    const float *grad_emb_loss_i; float grad_emb_scale;
    float *dp; int64_t lddp;
    unsigned emb_blocks;
    const void *logits; int64_t ldz;
    const float *aux, *grad_cls_loss_i; float grad_cls_scale;
    void *dz; int64_t lddz;
};

// dp = -w emb[y] (emb == NULL: -w at column y, +0 elsewhere), a wave per row; dz: the rows of se_softmax_xent_bwd
template <bool ZBF, bool DBF, bool VEC, int G>
__global__ __launch_bounds__(256) void joint_head_bwd_kernel(const BwdArgs a)
{
    const unsigned b = blockIdx.x;
    if (b < a.emb_blocks) {
        const int lane = lane_id();
        const int64_t row = (int64_t)b * ROWS_PER_BLOCK + (threadIdx.x >> 6);
        if (row >= a.B) return;
        const int64_t y = clamp_label(a.labels[row], a.C);
        const float nw = -(a.grad_emb_loss_i ? a.grad_emb_loss_i[row] : a.grad_emb_scale);
        float *drow = a.dp + row * a.lddp;
        if (a.emb) {
            const float *trow = a.emb + y * a.lde;
            for (int64_t i = lane; i < a.D; i += WAVE) drow[i] = nw * trow[i];
        } else {
            for (int64_t i = lane; i < a.D; i += WAVE) drow[i] = i == y ? nw : 0.f;
        }
        return;
    }
    xe_bwd_rows<ZBF, DBF, VEC, G>(b - a.emb_blocks, a.logits, a.ldz, a.labels, a.aux, a.grad_cls_loss_i, a.grad_cls_scale, a.B, (int)a.C, 1.0f,
                                  0.0f, a.dz, a.lddz);
}

inline bool sliced(int64_t B, int64_t C) { return (int64_t)head::tiles_per_block(B, C) * 32 < C; }

}  // namespace joint
}  // namespace se

using namespace se;

extern "C" int64_t se_joint_head_workspace_bytes(int metric, int64_t B, int64_t D, int64_t C)
{
    (void)D;
    if (metric != SE_HEAD_METRIC_NEAREST || B <= 0 || C <= 0 || !joint::sliced(B, C)) return 0;
    return metric::workspace_bytes(B, (B + 31) / 32);     // per strip: one ticket
}

extern "C" int se_joint_head_fwd(const float *p, int64_t ldp, const int64_t *labels, const float *emb, int64_t lde, int64_t B, int64_t D,
                                 int64_t C, int metric, float *emb_loss_i, int32_t *n_better, int32_t *n_within, int32_t *p_best,
                                 int32_t *p_above, float *scores, int64_t lds, const void *logits, int z_dtype, int64_t ldz,
                                 float *cls_loss_i, float *aux, int32_t *z_best, int32_t *z_above, void *workspace,
                                 int64_t workspace_bytes, se_stream_t stream)
{
    const bool nearest = metric == SE_HEAD_METRIC_NEAREST;
    if (!nearest && metric != SE_HEAD_METRIC_ARGMAX)
        return fail(SE_ERR_INVALID, "se_joint_head_fwd: bad metric %d (SE_HEAD_METRIC_NEAREST, SE_HEAD_METRIC_ARGMAX)", metric);
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_joint_head_fwd: bad shape B=%lld D=%lld C=%lld", (long long)B, (long long)D, (long long)C);
    if (C > INT_MAX - 16 || B > INT_MAX) return fail(SE_ERR_UNSUPPORTED, "se_joint_head_fwd: B or C too large");
    if (B == 0) return SE_OK;
    if (!p || !labels || !emb_loss_i) return fail(SE_ERR_INVALID, "se_joint_head_fwd: null pointer");
    if (nearest ? (!emb || !n_better || !n_within) : !p_above)
        return fail(SE_ERR_INVALID, nearest ? "se_joint_head_fwd: the nearest-class metric needs emb, n_better and n_within"
                                            : "se_joint_head_fwd: the arg-max metric needs p_above");
    if (!nearest && D != C)      // the label indexes the columns of p
        return fail(SE_ERR_INVALID, "se_joint_head_fwd: the arg-max metric needs D == C, got D=%lld C=%lld", (long long)D, (long long)C);
    if (ldp < D || (emb && lde < D) || (nearest && scores && lds < C)) return fail(SE_ERR_INVALID, "se_joint_head_fwd: leading dimension too small");
    if (logits) {
        if (!is_float_dtype(z_dtype)) return fail(SE_ERR_INVALID, "se_joint_head_fwd: bad dtype %d", z_dtype);
        if (ldz < C) return fail(SE_ERR_INVALID, "se_joint_head_fwd: leading dimension %lld < C=%lld", (long long)ldz, (long long)C);
        if (!cls_loss_i || !aux) return fail(SE_ERR_INVALID, "se_joint_head_fwd: logits need cls_loss_i and aux");
    }
    const int64_t need = se_joint_head_workspace_bytes(metric, B, D, C);
    if (need > 0 && (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 7)))
        return fail(SE_ERR_INVALID, "se_joint_head_fwd: needs %lld bytes of 8-byte aligned workspace (se_joint_head_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)stream;

    joint::FwdArgs a = {};
    a.p = p; a.ldp = ldp; a.labels = labels; a.emb = emb; a.lde = lde; a.B = B; a.D = D; a.C = C;
    a.emb_loss_i = emb_loss_i; a.n_better = n_better; a.n_within = n_within; a.p_best = p_best; a.p_above = p_above;
    a.scores = nearest ? scores : nullptr; a.lds = lds;
    a.loss_vec = emb ? cosine_rows_vec16(p, SE_DTYPE_F32, ldp, emb, lde, D) : 0;
    a.p_vec = ((ldp | D) & 3) == 0 && aligned16(p);          // four consecutive values per load (any path gives the same values)
    a.e_vec = emb && ((lde | D) & 3) == 0 && aligned16(emb);
    if (nearest) {
        a.tiles_per_block = head::tiles_per_block(B, C);
        a.strips = (unsigned)((B + 31) / 32);
        a.slices = (unsigned)(((C + 31) / 32 + a.tiles_per_block - 1) / a.tiles_per_block);
        a.emb_blocks = a.strips * a.slices;
        const metric::Workspace ws = metric::workspace(workspace, B, need > 0, true);
        a.part_best = ws.part_best; a.part_cnt = ws.part_cnt; a.ticket = ws.ticket;
        if (need > 0) SE_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)need, s));
    } else {
        a.emb_blocks = (unsigned)((B + joint::ROWS_PER_BLOCK - 1) / joint::ROWS_PER_BLOCK);
    }
    const bool in_grid = logits && C <= XE_BLOCK_MAX_C;      // the register paths of the cross-entropy
    const bool wave_rows = C <= XE_WAVE_MAX_C;
    unsigned cls_blocks = 0;
    bool zbf = false, zvec = false;
    if (in_grid) {
        a.logits = logits; a.ldz = ldz; a.cls_loss_i = cls_loss_i; a.aux = aux; a.z_best = z_best; a.z_above = z_above;
        cls_blocks = wave_rows ? (unsigned)((B + 3) / 4) : (unsigned)B;
        zbf = z_dtype == SE_DTYPE_BF16;
        zvec = aligned16(logits, ldz, zbf ? 2 : 4);
    }
    const dim3 grid(a.emb_blocks + cls_blocks);
    dispatch_bools(nearest, zbf, zvec, [&](auto N, auto ZB, auto ZV) {
        constexpr int M = N() ? SE_HEAD_METRIC_NEAREST : SE_HEAD_METRIC_ARGMAX;
        if (wave_rows) hipLaunchKernelGGL((joint::joint_head_fwd_kernel<M, ZB(), ZV(), 64>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((joint::joint_head_fwd_kernel<M, ZB(), ZV(), 256>), grid, dim3(256), 0, s, a);
    });
    SE_LAUNCH_CHECK();
    if (logits && !in_grid)
        return se_softmax_xent_fwd(logits, z_dtype, ldz, labels, B, C, 0.f, cls_loss_i, aux, z_best, z_above, nullptr, stream);
    return SE_OK;
}

extern "C" int se_joint_head_bwd(const int64_t *labels, const float *emb, int64_t lde, int64_t B, int64_t D, int64_t C,
                                 const float *grad_emb_loss_i, float grad_emb_scale, float *dp, int64_t lddp, const void *logits,
                                 int z_dtype, int64_t ldz, const float *aux, const float *grad_cls_loss_i, float grad_cls_scale, void *dz,
                                 int dz_dtype, int64_t lddz, se_stream_t stream)
{
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_joint_head_bwd: bad shape B=%lld D=%lld C=%lld", (long long)B, (long long)D, (long long)C);
    if (C > INT_MAX - 16 || B > INT_MAX) return fail(SE_ERR_UNSUPPORTED, "se_joint_head_bwd: B or C too large");
    if (B == 0) return SE_OK;
    if (!labels) return fail(SE_ERR_INVALID, "se_joint_head_bwd: null pointer");
    if (dp) {
        if (!emb && D != C) return fail(SE_ERR_INVALID, "se_joint_head_bwd: the identity table (emb == NULL) needs D == C, got D=%lld C=%lld", (long long)D, (long long)C);
        if (lddp < D || (emb && lde < D)) return fail(SE_ERR_INVALID, "se_joint_head_bwd: leading dimension < D");
    }
    if (logits) {
        if (!is_float_dtype(z_dtype) || !is_float_dtype(dz_dtype)) return fail(SE_ERR_INVALID, "se_joint_head_bwd: bad dtype");
        if (ldz < C || lddz < C) return fail(SE_ERR_INVALID, "se_joint_head_bwd: leading dimension < C=%lld", (long long)C);
        if (!aux || !dz) return fail(SE_ERR_INVALID, "se_joint_head_bwd: logits need aux and dz");
    }
    if (!dp && !logits) return SE_OK;

    joint::BwdArgs a = {};
    a.labels = labels; a.emb = emb; a.lde = lde; a.B = B; a.D = D; a.C = C;
    a.grad_emb_loss_i = grad_emb_loss_i; a.grad_emb_scale = grad_emb_scale; a.dp = dp; a.lddp = lddp;
    a.emb_blocks = dp ? (unsigned)((B + joint::ROWS_PER_BLOCK - 1) / joint::ROWS_PER_BLOCK) : 0u;
    const bool wave_rows = C <= XE_WAVE_MAX_C;
    unsigned cls_blocks = 0;
    bool zbf = false, dbf = false, vec = false;
    if (logits) {
        a.logits = logits; a.ldz = ldz; a.aux = aux; a.grad_cls_loss_i = grad_cls_loss_i; a.grad_cls_scale = grad_cls_scale;
        a.dz = dz; a.lddz = lddz;
        cls_blocks = wave_rows ? (unsigned)((B + 3) / 4) : (unsigned)B;
        zbf = z_dtype == SE_DTYPE_BF16; dbf = dz_dtype == SE_DTYPE_BF16;
        vec = aligned16(logits, ldz, zbf ? 2 : 4) && aligned16(dz, lddz, dbf ? 2 : 4);
    }
    const dim3 grid(a.emb_blocks + cls_blocks);
    dispatch_bools(zbf, dbf, vec, [&](auto ZB, auto DB, auto V) {
        if (wave_rows) hipLaunchKernelGGL((joint::joint_head_bwd_kernel<ZB(), DB(), V(), 64>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((joint::joint_head_bwd_kernel<ZB(), DB(), V(), 256>), grid, dim3(256), 0, (hipStream_t)stream, a);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}
