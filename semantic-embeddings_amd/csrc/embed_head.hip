// embed_head.hip -- the two embedding heads the reference trains with, loss AND nearest-class metric in one forward launch
// (reference: utils.py:44-46 / :34-36 for the loss, utils.py:57-100 for the metric).
//
//   se_embed_head_fwd(mode 0) : what se_cosine_loss_fwd writes  +  what se_nn_accuracy(dot_prod_sim = 1) computes from that xhat
//   se_embed_head_fwd(mode 1) : what se_sqdist_loss_fwd writes  +  what se_nn_accuracy(dot_prod_sim = 0) computes from float32(x)
//
// bit for bit, with the metric delivered as its two counts (n_better, n_within) so that every k is read off one contraction.
//
// Layout: a workgroup of four waves owns a strip of 32 samples and a slice of the class tiles.
//   1. loss:   each wave reduces 8 of the strip's rows with the row chains of loss_head.h, the ones the kernels of loss_kernels.hip
//              call.  The cosine head keeps the 32 inverse norms in LDS; the normalised features themselves are never read back:
//              every operand chunk of the contraction is rebuilt from x as x * inv_norm, the very product xhat holds, while it is
//              staged.  xhat goes to global memory only when the caller asks for it.
//   2. true:   the label's score per sample, with the arithmetic of the class-tile loop (k-ascending FMA chain; |e|^2 as even + odd
//              sum), on operands staged through LDS with coalesced loads -- the sibling walks two global rows per lane here.
//   3. tiles:  the four waves take four class tiles at a time on v_mfma_f32_32x32x2_f32, sharing ONE staged feature chunk; each wave
//              stages its own class chunk.  A finished tile goes through the metric epilogue of loss_head.h (se_nn_accuracy's).
//              Counts and the best class meet in LDS (integer atomics), and, when the class set is cut into slices, in the
//              workspace; the last slice of a strip to finish writes the strip's results (ticket counter).
// No floating-point atomics; counts are integer sums and the best class is an ordered-word maximum, so the result does not depend
// on the launch geometry or on the order in which workgroups finish.
#include "embed_head.h"

namespace se {
namespace head {

template <int MODE, bool BF16>
__global__ __launch_bounds__(THREADS) void embed_head_kernel(
    const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels, const float *__restrict__ emb, int64_t lde,
    int64_t B, int64_t D, int64_t C, float *__restrict__ xhat, int64_t ldxhat, float *__restrict__ inv_norm, float *__restrict__ loss_i,
    float *__restrict__ dist_i, int32_t *__restrict__ n_better_out, int32_t *__restrict__ n_within_out, int32_t *__restrict__ best_out,
    float *__restrict__ scores, int64_t lds_, int loss_vec, int x_vec, int e_vec, int tiles_per_block,
    unsigned long long *__restrict__ part_best, uint32_t *__restrict__ part_cnt, uint32_t *__restrict__ ticket)
{
    // grid = (32-sample strips, class slices of tiles_per_block x 32 classes)
    head_strip<MODE, BF16>(blockIdx.x, blockIdx.y, gridDim.y, x, ldx, labels, emb, lde, B, D, C, xhat, ldxhat, inv_norm, loss_i, dist_i,
                           n_better_out, n_within_out, best_out, scores, lds_, loss_vec, x_vec, e_vec, tiles_per_block, part_best, part_cnt,
                           ticket);
}

}  // namespace head
}  // namespace se

using namespace se;

extern "C" int64_t se_embed_head_workspace_bytes(int mode, int64_t B, int64_t D, int64_t C)
{
    (void)mode; (void)D;
    if (B <= 0 || C <= 0) return 0;
    if ((int64_t)head::tiles_per_block(B, C) * 32 >= C) return 0;
    const int64_t strips = (B + 31) / 32;
    return metric::workspace_bytes(B, strips);     // per strip: one ticket
}

extern "C" int se_embed_head_fwd(int mode, const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *emb, int64_t lde,
                                 int64_t B, int64_t D, int64_t C, float *xhat, int64_t ldxhat, float *inv_norm, float *loss_i, float *dist_i,
                                 float *loss_mean, int32_t *n_better, int32_t *n_within, int32_t *best, float *scores, int64_t lds,
                                 void *workspace, int64_t workspace_bytes, se_stream_t stream)
{
    if (mode != 0 && mode != 1) return fail(SE_ERR_INVALID, "se_embed_head_fwd: bad mode %d (0: cosine head, 1: squared-distance head)", mode);
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_embed_head_fwd: bad shape B=%lld D=%lld C=%lld", (long long)B, (long long)D, (long long)C);
    if (B == 0) return SE_OK;
    if (!x || !labels || !emb || !loss_i || !n_better || !n_within) return fail(SE_ERR_INVALID, "se_embed_head_fwd: null pointer");
    if (!is_float_dtype(x_dtype)) return fail(SE_ERR_INVALID, "se_embed_head_fwd: bad dtype %d", x_dtype);
    if (mode == 1) { xhat = nullptr; inv_norm = nullptr; }
    else dist_i = nullptr;
    if (ldx < D || lde < D || (xhat && ldxhat < D) || (scores && lds < C))
        return fail(SE_ERR_INVALID, "se_embed_head_fwd: leading dimension too small");
    const int64_t need = se_embed_head_workspace_bytes(mode, B, D, C);
    if (need > 0 && (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 7)))
        return fail(SE_ERR_INVALID, "se_embed_head_fwd: needs %lld bytes of 8-byte aligned workspace (se_embed_head_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const bool bf = x_dtype == SE_DTYPE_BF16;
    const int loss_vec = mode == 0 ? cosine_rows_vec16(x, x_dtype, ldx, emb, lde, D, xhat, ldxhat) : sqdist_rows_vec16(x, x_dtype, ldx, emb, lde, D);
    // staging: four consecutive k per load (any path gives the same values)
    const int x_vec = ((ldx | D) & 3) == 0 && ((((uintptr_t)x) & (bf ? 7 : 15)) == 0);
    const int e_vec = ((lde | D) & 3) == 0 && aligned16(emb);
    const int tpb = head::tiles_per_block(B, C);
    const int64_t strips = (B + 31) / 32, slices = ((C + 31) / 32 + tpb - 1) / tpb;
    const metric::Workspace ws = metric::workspace(workspace, B, need > 0, true);
    if (need > 0) SE_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)need, s));
    dispatch_bools(mode == 1, bf, [&](auto M, auto XB) {
        hipLaunchKernelGGL((head::embed_head_kernel<M() ? 1 : 0, XB()>), dim3((unsigned)strips, (unsigned)slices), dim3(head::THREADS), 0, s,
                           x, ldx, labels, emb, lde, B, D, C, xhat, ldxhat, inv_norm, loss_i, dist_i, n_better, n_within, best, scores, lds,
                           loss_vec, x_vec, e_vec, tpb, ws.part_best, ws.part_cnt, ws.ticket);
    });
    SE_LAUNCH_CHECK();
    if (loss_mean) {
        launch_mean(loss_i, B, loss_mean, s);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}
