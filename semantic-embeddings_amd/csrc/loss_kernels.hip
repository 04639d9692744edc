// loss_kernels.hip -- training-side hot path.
//
//   se_cosine_loss_fwd : l2norm head + class-embedding gather + inv_correlation + batch mean
//                        (reference: utils.py:125-127, learn_image_embeddings.py:48-50,127-128,
//                         utils.py:44-46)
//   se_cosine_loss_bwd : closed-form backward of the above
//   se_nn_accuracy     : nearest-class-embedding accuracy, y_pred @ emb^T on
//                        v_mfma_f32_32x32x2_f32 (reference: utils.py:57-100)
//
// Layout: one 64-lane wavefront owns one feature row; rows are streamed with coalesced
// 16-byte loads (float4 / 8 x bf16) when the row pitch allows it, the two row reductions
// (sum x^2 and x . emb[y]) are done with DPP/shuffle wave reductions -- no LDS, no atomics.
// The kernels are HBM-bound: algorithmic bytes per row = D*s_x (x) + D*4 (emb row, L2-resident)
// + D*4 (xhat) + 16.
// The row chains, their host predicates and the metric's tile epilogue are in loss_head.h, shared with embed_head.hip.
#include "loss_head.h"

namespace se {

constexpr int LOSS_ROWS_PER_BLOCK = 4;  // 4 waves = 256 threads

template <bool BF16>
__global__ __launch_bounds__(256) void cosine_loss_fwd_kernel(
    const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels,
    const float *__restrict__ emb, int64_t lde, int64_t B, int64_t D, int64_t C,
    float *__restrict__ xhat, int64_t ldxhat, float *__restrict__ inv_norm, float *__restrict__ loss_i,
    int vec_ok)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * LOSS_ROWS_PER_BLOCK + wave; row < B;
         row += (int64_t)gridDim.x * LOSS_ROWS_PER_BLOCK) {
        const char *xrow = (const char *)x + row * ldx * (BF16 ? 2 : 4);
        const int64_t y = clamp_label(labels[row], C);
        const float *trow = emb + y * lde;
        float ss, dt;
        row_reduce<BF16>(xrow, trow, D, vec_ok != 0, ss, dt);
        const float inv = 1.0f / sqrtf(fmaxf(ss, L2NORM_EPS));
        if (lane == 0) {
            if (inv_norm) inv_norm[row] = inv;
            loss_i[row] = 1.0f - dt * inv;
        }
        if (xhat) write_xhat_row<BF16>(xrow, xhat + row * ldxhat, D, vec_ok != 0, inv);
    }
}

// Deterministic mean of n floats: one 256-thread block, fixed tree; +0 for n = 0.
__global__ __launch_bounds__(256) void mean_kernel(const float *__restrict__ v, int64_t n, float *__restrict__ out)
{
    __shared__ float part[256];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += v[i];
    const float total = block_sum_256(s, part);
    if (threadIdx.x == 0) out[0] = n > 0 ? total / (float)n : 0.f;
}

void launch_mean(const float *v, int64_t n, float *out, hipStream_t s) { hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, v, n, out); }

template <bool BF16, bool DX_BF16>
__global__ __launch_bounds__(256) void cosine_loss_bwd_kernel(
    const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels,
    const float *__restrict__ emb, int64_t lde, const float *__restrict__ grad_loss_i, float grad_scale,
    int64_t B, int64_t D, int64_t C, void *__restrict__ dx, int64_t lddx, int vec_ok)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * LOSS_ROWS_PER_BLOCK + wave; row < B;
         row += (int64_t)gridDim.x * LOSS_ROWS_PER_BLOCK) {
        const char *xrow = (const char *)x + row * ldx * (BF16 ? 2 : 4);
        const int64_t y = clamp_label(labels[row], C);
        const float *trow = emb + y * lde;
        float ss, dt;
        row_reduce<BF16>(xrow, trow, D, vec_ok != 0, ss, dt);
        const float w = grad_loss_i ? grad_loss_i[row] : grad_scale;
        const float inv = 1.0f / sqrtf(fmaxf(ss, L2NORM_EPS));
        const bool clamped = !(ss >= L2NORM_EPS);
        // g = -w t ; proj = xhat . g = -w inv (x . t)
        const float proj = clamped ? 0.f : (-w * inv * dt);
        // dx_d = (g_d - xhat_d proj) inv = (-w t_d - x_d inv proj) inv
        const float c_t = -w * inv;
        const float c_x = -inv * proj * inv;
        char *drow = (char *)dx + row * lddx * (DX_BF16 ? 2 : 4);
        for (int64_t i = lane; i < D; i += WAVE) {
            float v = fmaf(c_t, trow[i], c_x * ld_elem<BF16>(xrow, i));
            st_elem<DX_BF16>(drow, i, v);
        }
    }
}

// ---- squared-distance loss of `--loss mse` (utils.squared_distance, utils.py:34-36; metric utils.mean_distance, :39-41) ----
// One wave per row, like the cosine head: loss_i = sum_d (x_d - E[y]_d)^2 (fp32 FMA accumulation per lane, wave tree), dist_i = sqrt(loss_i)
// when asked for; backward dx = 2 w (x - E[y]), w = grad_loss_i[row] or the scalar grad_scale.
template <bool BF16>
__global__ __launch_bounds__(256) void sqdist_loss_fwd_kernel(const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels,
                                                              const float *__restrict__ emb, int64_t lde, int64_t B, int64_t D, int64_t C,
                                                              float *__restrict__ loss_i, float *__restrict__ dist_i, int vec_ok)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * LOSS_ROWS_PER_BLOCK + wave; row < B; row += (int64_t)gridDim.x * LOSS_ROWS_PER_BLOCK) {
        const char *xrow = (const char *)x + row * ldx * (BF16 ? 2 : 4);
        const int64_t y = clamp_label(labels[row], C);
        const float *trow = emb + y * lde;
        const float s = row_sqdist<BF16>(xrow, trow, D, vec_ok != 0);
        if (lane == 0) {
            loss_i[row] = s;
            if (dist_i) dist_i[row] = sqrtf(s);
        }
    }
}

template <bool BF16, bool DX_BF16>
__global__ __launch_bounds__(256) void sqdist_loss_bwd_kernel(const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels,
                                                              const float *__restrict__ emb, int64_t lde, const float *__restrict__ grad_loss_i,
                                                              float grad_scale, int64_t B, int64_t D, int64_t C, void *__restrict__ dx, int64_t lddx)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * LOSS_ROWS_PER_BLOCK + wave; row < B; row += (int64_t)gridDim.x * LOSS_ROWS_PER_BLOCK) {
        const char *xrow = (const char *)x + row * ldx * (BF16 ? 2 : 4);
        const int64_t y = clamp_label(labels[row], C);
        const float *trow = emb + y * lde;
        const float w2 = 2.0f * (grad_loss_i ? grad_loss_i[row] : grad_scale);
        char *drow = (char *)dx + row * lddx * (DX_BF16 ? 2 : 4);
        for (int64_t i = lane; i < D; i += WAVE) {
            const float v = w2 * (ld_elem<BF16>(xrow, i) - trow[i]);
            st_elem<DX_BF16>(drow, i, v);
        }
    }
}

// Stand-alone l2norm head (utils.py:125-127) for inference / feature dumps and for callers that
// keep the Keras-style ``Lambda(l2norm)`` layer separate from the loss.
template <bool BF16>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const void *__restrict__ x, int64_t ldx, int64_t B, int64_t D,
                                                         float *__restrict__ xhat, int64_t ldo, float *__restrict__ inv_norm,
                                                         float *__restrict__ sumsq)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * LOSS_ROWS_PER_BLOCK + wave; row < B;
         row += (int64_t)gridDim.x * LOSS_ROWS_PER_BLOCK) {
        const char *xrow = (const char *)x + row * ldx * (BF16 ? 2 : 4);
        float s = 0.f;
        for (int64_t i = lane; i < D; i += WAVE) { const float p = ld_elem<BF16>(xrow, i); s = fmaf(p, p, s); }
        s = wave_sum(s);
        const float inv = 1.0f / sqrtf(fmaxf(s, L2NORM_EPS));
        if (lane == 0) {
            if (inv_norm) inv_norm[row] = inv;
            if (sumsq) sumsq[row] = s;
        }
        float *orow = xhat + row * ldo;
        for (int64_t i = lane; i < D; i += WAVE) orow[i] = ld_elem<BF16>(xrow, i) * inv;
    }
}

// dx = (g - xhat (xhat . g)) * inv_norm ; rows on the epsilon clamp (!(sum x^2 >= 1e-12), the forward's predicate): dx = g * inv_norm.
// The clamp is decided from the forward's sum x^2, not from inv_norm: sum x^2 = 1e-12f and its next float both give inv_norm == 1e6f.
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float *__restrict__ g, int64_t ldg,
                                                         const float *__restrict__ xhat, int64_t ldh,
                                                         const float *__restrict__ inv_norm, const float *__restrict__ sumsq,
                                                         int64_t B, int64_t D, float *__restrict__ dx, int64_t lddx)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    for (int64_t row = (int64_t)blockIdx.x * LOSS_ROWS_PER_BLOCK + wave; row < B;
         row += (int64_t)gridDim.x * LOSS_ROWS_PER_BLOCK) {
        const float *gr = g + row * ldg, *hr = xhat + row * ldh;
        float s = 0.f;
        for (int64_t i = lane; i < D; i += WAVE) s = fmaf(gr[i], hr[i], s);
        const float inv = inv_norm[row];
        const float proj = (sumsq[row] >= L2NORM_EPS) ? wave_sum(s) : 0.f;
        float *o = dx + row * lddx;
        for (int64_t i = lane; i < D; i += WAVE) o[i] = (gr[i] - hr[i] * proj) * inv;
    }
}

// ------------------------------------------------------------------------------------------------
// nn_accuracy: one wave owns a strip of 32 samples and walks all classes in tiles of 32 with
// v_mfma_f32_32x32x2_f32.  Operands are staged through LDS in K-chunks of 64, stored with even
// and odd k de-interleaved so that lanes 0-31 (k = 2t) and 32-63 (k = 2t+1) each read 16 B.
// (The same tile as tile32.h, which the DeViSE kernels use; this kernel keeps its own staging and chunk loop: every spelling
// through the shared helpers measured 1 - 3 us per call slower, profiles/loss_head_refactor_equivalence.txt section 3.)
// What happens to a finished tile (the counting form of the metric, the best class) is metric:: of loss_head.h.
// ------------------------------------------------------------------------------------------------
using tile32::f32x16;

constexpr int ACC_BK = tile32::BK, ACC_LD = tile32::LD;    // k per staged chunk; padded row pitch (floats)

__device__ __forceinline__ void stage_tile32(float *lds, const float *src, int64_t ld, int64_t row0,
                                             int64_t nrows, int64_t k0, int64_t K)
{
    // 32 rows x 64 k, each lane moves 8 float4 (row = idx / 16, 4 consecutive k = idx % 16).  The loads are unconditional
    // (out-of-range elements read a valid address and are zeroed afterwards) so that all of them are in flight together.
    const int lane = lane_id();
    float v[8][4];
    const bool vec = ((ld | K) & 3) == 0 && (((uintptr_t)src) & 15) == 0;          // wave-uniform
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const int idx = it * 64 + lane;
        const int r = idx >> 4, kq = (idx & 15) * 4;
        const bool rok = row0 + r < nrows;
        const float *p = src + (rok ? row0 + r : row0) * ld;
        if (vec) {
            const bool ok = rok && k0 + kq < K;
            const float4 t = *(const float4 *)(p + (k0 + kq < K ? k0 + kq : 0));
            v[it][0] = ok ? t.x : 0.f; v[it][1] = ok ? t.y : 0.f; v[it][2] = ok ? t.z : 0.f; v[it][3] = ok ? t.w : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool kok = k0 + kq + j < K;
                const float t = p[kok ? k0 + kq + j : 0];
                v[it][j] = (rok && kok) ? t : 0.f;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < 8; it++) {
        const int idx = it * 64 + lane;
        const int r = idx >> 4, kq = (idx & 15) * 4;
        float *o = lds + r * ACC_LD;
        // even k -> [0, 32), odd k -> [32, 64)
        o[(kq >> 1)] = v[it][0];
        o[(kq >> 1) + 1] = v[it][2];
        o[32 + (kq >> 1)] = v[it][1];
        o[32 + (kq >> 1) + 1] = v[it][3];
    }
}

__global__ __launch_bounds__(64) void nn_accuracy_kernel(
    const float *__restrict__ yp, int64_t ldp, const int64_t *__restrict__ labels,
    const float *__restrict__ emb, int64_t lde, int64_t B, int64_t D, int64_t C, int dot_prod_sim, int k,
    float *__restrict__ acc_out, float *__restrict__ scores, int64_t lds_, int32_t *__restrict__ best_out,
    int tiles_per_block, uint32_t *__restrict__ part_cnt, unsigned long long *__restrict__ part_best)
{
    // grid = (32-sample blocks, class slices of tiles_per_block x 32 classes).  One slice: results are written directly; several
    // (large class sets -- at ILSVRC size, C = D = 1000, a batch of 64 was TWO waves walking 32 class tiles each: 2.6 ms): every
    // slice adds its counts / proposes its best class into part_cnt / part_best and nn_accuracy_finish_kernel closes the metric.
    __shared__ __attribute__((aligned(16))) float sA[32 * ACC_LD];
    __shared__ __attribute__((aligned(16))) float sB[32 * ACC_LD];
    __shared__ float sTrue[32], sPn[32], sCn[32];

    const int lane = lane_id();
    const int col = lane & 31, hi = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * 32;
    const bool dot = dot_prod_sim != 0;

    // "true" score per sample.  The reference forms it with a separate elementwise reduction
    // (utils.py:80 / :91) and then needs the 1e-6 band to absorb the float32 noise between that
    // reduction and the matmul.  Here the true score is rebuilt with exactly the arithmetic the
    // class-tile loop uses for column y (k-ascending fmaf chain == MFMA; |e|^2 as even-k sum +
    // odd-k sum), so the true class always matches its own matrix entry bit-for-bit.
    {
        const int64_t r = row0 + col;
        float t = 0.f, pn = 0.f;
        if (r < B) {
            const int64_t y = clamp_label(labels[r], C);
            const float *p = yp + r * ldp, *e = emb + y * lde;
            if (hi == 0) {
                float s = 0.f;
                for (int64_t d = 0; d < D; d++) s = fmaf(p[d], e[d], s);
                t = s;                                   // S[r, y]
            } else if (!dot) {
                float ce = 0.f, co = 0.f;
                for (int64_t d = 0; d < D; d += 2) {
                    ce = fmaf(e[d], e[d], ce);
                    if (d + 1 < D) co = fmaf(e[d + 1], e[d + 1], co);
                }
                for (int64_t d = 0; d < D; d++) pn = fmaf(p[d], p[d], pn);
                t = ce + co;                             // |e_y|^2
            }
        }
        const float other = __shfl_xor(t, 32, 64);       // hi==0: |e_y|^2 ; hi==1: S[r, y]
        pn = __shfl_xor(pn, 32, 64);                     // hi==0 lanes receive |p|^2
        if (hi == 0) {
            sPn[col] = pn;
            sTrue[col] = dot ? t : ((pn + other) - 2.0f * t);
        }
    }
    wg_barrier();

    metric::Tally tally[16];
#pragma unroll
    for (int r = 0; r < 16; r++) tally[r] = metric::empty_tally(dot);

    const int64_t c_beg = (int64_t)blockIdx.y * tiles_per_block * 32;
    const int64_t c_end = (c_beg + (int64_t)tiles_per_block * 32 < C) ? c_beg + (int64_t)tiles_per_block * 32 : C;
    for (int64_t c0 = c_beg; c0 < c_end; c0 += 32) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        float cn = 0.f;  // |emb_c|^2 for this lane's class (Euclidean variant), half of D per lane
        for (int64_t k0 = 0; k0 < D; k0 += ACC_BK) {
            wg_barrier();
            stage_tile32(sA, yp, ldp, row0, B, k0, D);
            stage_tile32(sB, emb, lde, c0, C, k0, D);
            wg_barrier();
            const int64_t kc = (D - k0 < ACC_BK) ? (D - k0) : ACC_BK;
            const int steps = (int)((kc + 1) / 2);           // MFMA steps (2 k each), zero padded
            const float *pa = sA + col * ACC_LD + hi * 32;
            const float *pb = sB + col * ACC_LD + hi * 32;
            for (int s = 0; s < steps; s += 4) {
                const float4 a4 = *(const float4 *)(pa + s);
                const float4 b4 = *(const float4 *)(pb + s);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
                if (s + 1 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
                if (s + 2 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
                if (s + 3 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
                if (!dot) cn = metric::class_norm_steps(cn, b4, s, steps);
            }
        }
        if (!dot) {
            cn += __shfl_xor(cn, 32, 64);
            wg_barrier();
            if (hi == 0) sCn[col] = cn;
            wg_barrier();
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int lr = tile32::acc_row(r, hi);
            metric::update(tally[r], dot, acc[r], sPn, sCn[col], sTrue, lr, row0 + lr, B, c0 + col, C, scores, lds_);
        }
    }

    // reduce over the 32 lanes (classes) that share `hi`
#pragma unroll
    for (int r = 0; r < 16; r++) {
        metric::reduce32(tally[r], dot);
        const int lr = tile32::acc_row(r, hi);
        if (col == 0 && row0 + lr < B) {
            if (gridDim.y == 1) {
                acc_out[row0 + lr] = (tally[r].n_within >= 1 && tally[r].n_better < k) ? 1.0f : 0.0f;
                if (best_out) best_out[row0 + lr] = tally[r].best_c;
            } else {
                atomicAdd(&part_cnt[2 * (row0 + lr)], (uint32_t)tally[r].n_better);
                atomicAdd(&part_cnt[2 * (row0 + lr) + 1], (uint32_t)tally[r].n_within);
                if (tally[r].best_c != metric::NO_CLASS)
                    atomicMax(&part_best[row0 + lr], metric::best_word(tally[r].best_v, tally[r].best_c, dot));
            }
        }
    }
}

__global__ __launch_bounds__(256) void nn_accuracy_finish_kernel(const uint32_t *__restrict__ part_cnt, const unsigned long long *__restrict__ part_best,
                                                                int64_t B, int k, float *__restrict__ acc_out, int32_t *__restrict__ best_out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= B) return;
    acc_out[r] = (part_cnt[2 * r + 1] >= 1u && part_cnt[2 * r] < (uint32_t)k) ? 1.0f : 0.0f;
    if (best_out) best_out[r] = metric::best_class(part_best[r]);
}

}  // namespace se

using namespace se;

extern "C" int se_cosine_loss_fwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels,
                                  const float *emb, int64_t lde, int64_t B, int64_t D, int64_t C,
                                  float *xhat, int64_t ldxhat, float *inv_norm, float *loss_i,
                                  float *loss_mean, se_stream_t stream)
{
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_cosine_loss_fwd: bad shape B=%lld D=%lld C=%lld", (long long)B, (long long)D, (long long)C);
    if (B == 0) return SE_OK;
    if (!x || !labels || !emb || !loss_i) return fail(SE_ERR_INVALID, "se_cosine_loss_fwd: null pointer");
    if (ldx < D || lde < D || (xhat && ldxhat < D)) return fail(SE_ERR_INVALID, "se_cosine_loss_fwd: leading dimension < D");
    if (!is_float_dtype(x_dtype)) return fail(SE_ERR_INVALID, "se_cosine_loss_fwd: bad dtype %d", x_dtype);
    hipStream_t s = (hipStream_t)stream;
    const int vec_ok = cosine_rows_vec16(x, x_dtype, ldx, emb, lde, D, xhat, ldxhat);
    const unsigned blocks = row_blocks(B, LOSS_ROWS_PER_BLOCK, 256 * 32);
    dispatch_bools(x_dtype == SE_DTYPE_BF16, [&](auto XB) {
        hipLaunchKernelGGL(cosine_loss_fwd_kernel<XB()>, dim3(blocks), dim3(256), 0, s, x, ldx, labels, emb, lde, B, D, C, xhat, ldxhat, inv_norm, loss_i, vec_ok);
    });
    SE_LAUNCH_CHECK();
    if (loss_mean) {
        launch_mean(loss_i, B, loss_mean, s);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}

extern "C" int se_cosine_loss_bwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels,
                                  const float *emb, int64_t lde, const float *grad_loss_i, float grad_scale,
                                  int64_t B, int64_t D, int64_t C, void *dx, int dx_dtype, int64_t lddx,
                                  se_stream_t stream)
{
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_cosine_loss_bwd: bad shape");
    if (B == 0) return SE_OK;
    if (!x || !labels || !emb || !dx) return fail(SE_ERR_INVALID, "se_cosine_loss_bwd: null pointer");
    if (ldx < D || lde < D || lddx < D) return fail(SE_ERR_INVALID, "se_cosine_loss_bwd: leading dimension < D");
    hipStream_t s = (hipStream_t)stream;
    const bool bf = x_dtype == SE_DTYPE_BF16, dbf = dx_dtype == SE_DTYPE_BF16;
    if (!is_float_dtype(x_dtype) || !is_float_dtype(dx_dtype)) return fail(SE_ERR_INVALID, "se_cosine_loss_bwd: bad dtype");
    const int vec_ok = cosine_rows_vec16(x, x_dtype, ldx, emb, lde, D);
    const unsigned blocks = row_blocks(B, LOSS_ROWS_PER_BLOCK, 256 * 32);
    dispatch_bools(bf, dbf, [&](auto XB, auto DB) {
        hipLaunchKernelGGL((cosine_loss_bwd_kernel<XB(), DB()>), dim3(blocks), dim3(256), 0, s, x, ldx, labels, emb, lde, grad_loss_i, grad_scale, B, D, C, dx, lddx, vec_ok);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_sqdist_loss_fwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *emb, int64_t lde,
                                  int64_t B, int64_t D, int64_t C, float *loss_i, float *dist_i, float *loss_mean, se_stream_t stream)
{
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_sqdist_loss_fwd: bad shape B=%lld D=%lld C=%lld", (long long)B, (long long)D, (long long)C);
    if (B == 0) return SE_OK;
    if (!x || !labels || !emb || !loss_i) return fail(SE_ERR_INVALID, "se_sqdist_loss_fwd: null pointer");
    if (ldx < D || lde < D) return fail(SE_ERR_INVALID, "se_sqdist_loss_fwd: leading dimension < D");
    if (!is_float_dtype(x_dtype)) return fail(SE_ERR_INVALID, "se_sqdist_loss_fwd: bad dtype %d", x_dtype);
    hipStream_t s = (hipStream_t)stream;
    const int vec_ok = sqdist_rows_vec16(x, x_dtype, ldx, emb, lde, D);
    const unsigned blocks = row_blocks(B, LOSS_ROWS_PER_BLOCK, 256 * 32);
    dispatch_bools(x_dtype == SE_DTYPE_BF16, [&](auto XB) {
        hipLaunchKernelGGL(sqdist_loss_fwd_kernel<XB()>, dim3(blocks), dim3(256), 0, s, x, ldx, labels, emb, lde, B, D, C, loss_i, dist_i, vec_ok);
    });
    SE_LAUNCH_CHECK();
    if (loss_mean) {
        launch_mean(loss_i, B, loss_mean, s);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}

extern "C" int se_sqdist_loss_bwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *emb, int64_t lde,
                                  const float *grad_loss_i, float grad_scale, int64_t B, int64_t D, int64_t C, void *dx, int dx_dtype,
                                  int64_t lddx, se_stream_t stream)
{
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_sqdist_loss_bwd: bad shape");
    if (B == 0) return SE_OK;
    if (!x || !labels || !emb || !dx) return fail(SE_ERR_INVALID, "se_sqdist_loss_bwd: null pointer");
    if (ldx < D || lde < D || lddx < D) return fail(SE_ERR_INVALID, "se_sqdist_loss_bwd: leading dimension < D");
    hipStream_t s = (hipStream_t)stream;
    const bool bf = x_dtype == SE_DTYPE_BF16, dbf = dx_dtype == SE_DTYPE_BF16;
    if (!is_float_dtype(x_dtype) || !is_float_dtype(dx_dtype)) return fail(SE_ERR_INVALID, "se_sqdist_loss_bwd: bad dtype");
    const unsigned blocks = row_blocks(B, LOSS_ROWS_PER_BLOCK, 256 * 32);
    dispatch_bools(bf, dbf, [&](auto XB, auto DB) {
        hipLaunchKernelGGL((sqdist_loss_bwd_kernel<XB(), DB()>), dim3(blocks), dim3(256), 0, s, x, ldx, labels, emb, lde, grad_loss_i, grad_scale, B, D, C, dx, lddx);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}

constexpr int NN_ACC_MIN_TILES = 4;     // up to 4 class tiles: one wave walks them all (tile32::tiles_per_block)

extern "C" int64_t se_nn_accuracy_workspace_bytes(int64_t B, int64_t C)
{
    if (B <= 0 || C <= 0) return 0;
    return tile32::tiles_per_block(B, C, NN_ACC_MIN_TILES) * 32 >= C ? 0 : metric::workspace_bytes(B, 0);
}

extern "C" int se_nn_accuracy(const float *y_pred, int64_t ldp, const int64_t *labels, const float *emb,
                              int64_t lde, int64_t B, int64_t D, int64_t C, int dot_prod_sim, int k,
                              float *acc, float *scores, int64_t lds, int32_t *best, void *workspace, int64_t workspace_bytes,
                              se_stream_t stream)
{
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_nn_accuracy: bad shape");
    if (B == 0) return SE_OK;
    if (!y_pred || !labels || !emb || !acc) return fail(SE_ERR_INVALID, "se_nn_accuracy: null pointer");
    if (ldp < D || lde < D || (scores && lds < C)) return fail(SE_ERR_INVALID, "se_nn_accuracy: leading dimension too small");
    if (k < 1) k = 1;
    const int64_t need = se_nn_accuracy_workspace_bytes(B, C);
    if (need > 0 && (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 7)))
        return fail(SE_ERR_WORKSPACE, "se_nn_accuracy: needs %lld bytes of 8-byte aligned workspace (se_nn_accuracy_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const int tpb = tile32::tiles_per_block(B, C, NN_ACC_MIN_TILES);
    const int64_t slices = ((C + 31) / 32 + tpb - 1) / tpb;
    const metric::Workspace ws = metric::workspace(workspace, B, need > 0, false);
    if (need > 0) SE_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)need, s));
    hipLaunchKernelGGL(nn_accuracy_kernel, dim3((unsigned)((B + 31) / 32), (unsigned)slices), dim3(64), 0, s,
                       y_pred, ldp, labels, emb, lde, B, D, C, dot_prod_sim, k, acc, scores, lds, best, tpb, ws.part_cnt, ws.part_best);
    SE_LAUNCH_CHECK();
    if (slices > 1) {
        hipLaunchKernelGGL(nn_accuracy_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, ws.part_cnt, ws.part_best, B, k, acc, best);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}

extern "C" int se_l2norm_fwd(const void *x, int x_dtype, int64_t ldx, int64_t B, int64_t D, float *xhat,
                             int64_t ldxhat, float *inv_norm, float *sumsq, se_stream_t stream)
{
    if (B < 0 || D <= 0) return fail(SE_ERR_INVALID, "se_l2norm_fwd: bad shape");
    if (B == 0) return SE_OK;
    if (!x || !xhat || ldx < D || ldxhat < D) return fail(SE_ERR_INVALID, "se_l2norm_fwd: bad argument");
    if (!is_float_dtype(x_dtype)) return fail(SE_ERR_INVALID, "se_l2norm_fwd: bad dtype %d", x_dtype);
    const unsigned blocks = row_blocks(B, LOSS_ROWS_PER_BLOCK, 256 * 32);
    dispatch_bools(x_dtype == SE_DTYPE_BF16, [&](auto XB) {
        hipLaunchKernelGGL(l2norm_fwd_kernel<XB()>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, B, D, xhat, ldxhat, inv_norm, sumsq);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_l2norm_bwd(const float *grad, int64_t ldg, const float *xhat, int64_t ldxhat, const float *inv_norm,
                             const float *sumsq, int64_t B, int64_t D, float *dx, int64_t lddx, se_stream_t stream)
{
    if (B < 0 || D <= 0) return fail(SE_ERR_INVALID, "se_l2norm_bwd: bad shape");
    if (B == 0) return SE_OK;
    if (!grad || !xhat || !inv_norm || !sumsq || !dx || ldg < D || ldxhat < D || lddx < D) return fail(SE_ERR_INVALID, "se_l2norm_bwd: bad argument");
    const unsigned blocks = row_blocks(B, LOSS_ROWS_PER_BLOCK, 256 * 32);
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grad, ldg, xhat, ldxhat, inv_norm, sumsq, B, D, dx, lddx);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
