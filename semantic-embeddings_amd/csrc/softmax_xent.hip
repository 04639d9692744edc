// softmax_xent.hip -- categorical cross-entropy of the softmax classifier on LOGITS, with label smoothing, Keras 2.2's clip of the
// probabilities and the accuracy / top-k metrics of the same scores; forward + backward.
//
// Replaces `transform_inputs` (learn_classifier.py:17-22: to_categorical + label smoothing on the host), the
// 'categorical_crossentropy' loss and the 'accuracy' metric of both compile() calls (learn_classifier.py:116-117, 146-147),
// utils.top_k_acc (utils.py:49-54) and what TF autodiff derives from the loss with respect to the logits.
//
// Per row z with label y (clamped to [0, C - 1]):  m = max z,  lse = m + log sum_c exp(z_c - m),  t_c = lse - z_c = -log softmax(z)_c.
// Target Y_c = 1 - s (c == y), s / (C - 1) otherwise when 0 < s < 1; one-hot for every other s.  Keras' loss is
// -sum_c Y_c log(clip(p_c / sum p, eps, 1 - eps)), eps = float32(1e-7); in the log domain, with LO = -log(1 - eps), HI = -log(eps):
//     loss = sum_c Y_c min(max(t_c, LO), HI)        a_c = Y_c where LO <= t_c <= HI, else 0        A = sum_c a_c
//     dz_k = w (A exp(z_k - lse) - a_k)
// t_c is evaluated as (m - z_c) + log(sum): for the arg-max class that is log(sum) itself, at full relative precision, so the upper
// clip (p > 1 - eps, t < 1.2e-7) is decided by the last bit of the float32 sum as it would be on probabilities -- lse - z_c would
// round t to a multiple of ulp(lse), ~2e-6 for logits around 30.  aux keeps m and log(sum) apart for the same reason: the backward
// pass recomputes the forward's t_c bit for bit, so a_k and A always agree.
// (sum p = 1 up to rounding: the renormalisation is exact in this form.)  best = arg-max class (lowest index on ties; the first NaN
// if the row holds one), above = number of classes whose logit is strictly greater than z_y (tf.nn.in_top_k(k) == above < k).
// A row that holds a NaN or +inf, or nothing but -inf: loss, m, log(sum) and A are NaN (so the whole dz row is NaN), above = C.
//
// Forward paths, picked by C (xe_launch_fwd):
//   wave   C <= 1024   one 64-lane wave per row, 16 values per lane in registers, shuffle reductions only (no LDS, no barrier)
//   block  C <= 8192   one 256-thread workgroup per row, 32 values per thread in registers, 2 (s = 0) or 3 barriers
//   stream otherwise   one workgroup per row, online max + sum in one read; a smoothed target takes a second read for the clamped sum
// The row is read from memory once on the register paths (plus one broadcast load of z_y); s = 0 skips the off-target sum.
// Each path comes with 16-byte loads (pointer and pitch 16-byte aligned) or scalar loads (any pitch).  The backward is one pass
// over [B, C] (a wave per row up to C = 1024, a workgroup per row above); everything row-wide it needs is in aux.
// No atomics, no workspace, no host synchronisation: every reduction is a fixed tree, so the same inputs give the same bits.
#include "softmax_xent.h"

namespace se {

template <bool BF16, bool VEC, int G, int NV>
__global__ __launch_bounds__(256) void xent_fwd_reg_kernel(const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                           int64_t B, int C, float y_on, float y_off, float *__restrict__ loss_i,
                                                           float *__restrict__ aux, int32_t *__restrict__ best, int32_t *__restrict__ above)
{
    xe_fwd_reg_rows<BF16, VEC, G, NV>(blockIdx.x, z, ldz, labels, B, C, y_on, y_off, loss_i, aux, best, above);
}

// Rows too long for registers: one workgroup per row, each thread keeps a running (max, sum of exp) over its units.
template <bool BF16, bool VEC>
__global__ __launch_bounds__(256) void xent_fwd_stream_kernel(const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                              int64_t B, int C, float y_on, float y_off, float *__restrict__ loss_i,
                                                              float *__restrict__ aux, int32_t *__restrict__ best,
                                                              int32_t *__restrict__ above)
{
    constexpr int E = VEC ? (BF16 ? 8 : 4) : 1;
    const int t = threadIdx.x, wave = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    const void *zrow = BF16 ? (const void *)((const uint16_t *)z + row * ldz) : (const void *)((const float *)z + row * ldz);
    const int y = (int)clamp_label(labels[row], C);
    const float zy = ld_elem<BF16>(zrow, y);
    const int64_t units = ((int64_t)C + E - 1) / E;

    float m = -INFINITY, ssum = 0.f;
    int am = INT_MAX, nan_at = INT_MAX, cnt = 0;
    for (int64_t u = t; u < units; u += 256) {
        const int64_t c0 = u * E;
        float v[E];
        xe_ld_unit<BF16, E>(zrow, c0, C, v);
        float um = -INFINITY;
        int uam = INT_MAX;
#pragma unroll
        for (int k = 0; k < E; k++) {
            if (v[k] != v[k]) nan_at = min(nan_at, (int)(c0 + k));
            if (v[k] > um) { um = v[k]; uam = (int)(c0 + k); }
            cnt += v[k] > zy ? 1 : 0;
        }
        if (um > m) {                                       // columns ascend within a thread: the first maximum stays
            ssum = m == -INFINITY ? 0.f : ssum * expf(m - um);
            m = um;
            am = uam;
        }
        if (m != -INFINITY) {
#pragma unroll
            for (int k = 0; k < E; k++) ssum += expf(v[k] - m);
        }
    }
    __shared__ XeShared sh;
    float M = wave_max(m);
    nan_at = wave_min(nan_at);
    if (lane_id() == 0) { sh.f[0][wave] = M; sh.i[0][wave] = nan_at; }
    wg_barrier();
    M = fmaxf(fmaxf(sh.f[0][0], sh.f[0][1]), fmaxf(sh.f[0][2], sh.f[0][3]));
    nan_at = min(min(sh.i[0][0], sh.i[0][1]), min(sh.i[0][2], sh.i[0][3]));
    float S = wave_sum(m == -INFINITY ? 0.f : ssum * expf(m - M));
    int cand = wave_min(m == M ? am : INT_MAX);
    cnt = wave_sum(cnt);
    if (lane_id() == 0) { sh.f[1][wave] = S; sh.i[1][wave] = cand; sh.i[2][wave] = cnt; }
    wg_barrier();
    S = (sh.f[1][0] + sh.f[1][1]) + (sh.f[1][2] + sh.f[1][3]);
    cand = min(min(sh.i[1][0], sh.i[1][1]), min(sh.i[1][2], sh.i[1][3]));
    cnt = (sh.i[2][0] + sh.i[2][1]) + (sh.i[2][2] + sh.i[2][3]);
    const float lS = logf(S);                               // lse = M + lS; t_c = (M - z_c) + lS keeps the arg-max class's t = lS
    const bool bad = xe_bad_row(nan_at, M);
    float loss, A;
    if (y_off != 0.f) {                                     // second read of the row (the first left it in the L2)
        float la[E], aa[E];
#pragma unroll
        for (int k = 0; k < E; k++) la[k] = aa[k] = 0.f;
        for (int64_t u = t; u < units; u += 256) {
            const int64_t c0 = u * E;
            float v[E];
            xe_ld_unit<BF16, E>(zrow, c0, C, v);
#pragma unroll
            for (int k = 0; k < E; k++) {
                const float tc = (M - v[k]) + lS;
                const float Y = c0 + k < C ? (c0 + k == y ? y_on : y_off) : 0.f;
                la[k] += Y * xe_clamp(tc);
                aa[k] += xe_inside(tc) ? Y : 0.f;
            }
        }
        loss = wave_sum(xe_tree_sum<E>(la));
        A = wave_sum(xe_tree_sum<E>(aa));
        if (lane_id() == 0) { sh.f[2][wave] = loss; sh.f[3][wave] = A; }
        wg_barrier();
        loss = (sh.f[2][0] + sh.f[2][1]) + (sh.f[2][2] + sh.f[2][3]);
        A = (sh.f[3][0] + sh.f[3][1]) + (sh.f[3][2] + sh.f[3][3]);
    } else {
        const float ty = (M - zy) + lS;
        loss = y_on * xe_clamp(ty);
        A = xe_inside(ty) ? y_on : 0.f;
    }
    if (t == 0) xe_write_row(row, B, C, bad, loss, M, lS, A, nan_at, cand, cnt, loss_i, aux, best, above);
}

template <bool ZBF, bool DBF, bool VEC, int G>
__global__ __launch_bounds__(256) void xent_bwd_kernel(const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                       const float *__restrict__ aux, const float *__restrict__ grad_loss_i,
                                                       float grad_scale, int64_t B, int C, float y_on, float y_off,
                                                       void *__restrict__ dz, int64_t lddz)
{
    xe_bwd_rows<ZBF, DBF, VEC, G>(blockIdx.x, z, ldz, labels, aux, grad_loss_i, grad_scale, B, C, y_on, y_off, dz, lddz);
}

}  // namespace se

using namespace se;

// target weights: (1 - s, s / (C - 1)) for 0 < s < 1, one-hot otherwise (learn_classifier.py:20)
static inline void xe_target(float smoothing, int64_t C, float &y_on, float &y_off)
{
    const bool smooth = smoothing > 0.f && smoothing < 1.f;
    y_on = smooth ? (float)(1.0 - (double)smoothing) : 1.0f;
    y_off = smooth ? (float)((double)smoothing / (double)(C - 1)) : 0.0f;
}

static int xe_check(const char *who, const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, int64_t B, int64_t C,
                    float smoothing, const float *aux)
{
    if (B < 0 || C < 1) return fail(SE_ERR_INVALID, "%s: bad shape B=%lld C=%lld", who, (long long)B, (long long)C);
    if (smoothing > 0.f && smoothing < 1.f && C < 2) return fail(SE_ERR_INVALID, "%s: label smoothing %g needs at least 2 classes", who, (double)smoothing);
    if (!is_float_dtype(z_dtype)) return fail(SE_ERR_INVALID, "%s: bad dtype %d", who, z_dtype);
    if (ldz < C) return fail(SE_ERR_INVALID, "%s: leading dimension %lld < C=%lld", who, (long long)ldz, (long long)C);
    if (C > INT_MAX - 16 || B > INT_MAX) return fail(SE_ERR_UNSUPPORTED, "%s: B or C too large", who);
    if (B > 0 && (!logits || !labels || !aux)) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    return SE_OK;
}

extern "C" int64_t se_softmax_xent_aux_floats(int64_t B) { return B > 0 ? 3 * B : 0; }

template <bool BF16, bool VEC>
static void xe_launch_fwd(const void *z, int64_t ldz, const int64_t *labels, int64_t B, int C, float y_on, float y_off, float *loss_i,
                          float *aux, int32_t *best, int32_t *above, hipStream_t s)
{
    if (C <= XE_WAVE_MAX_C)
        hipLaunchKernelGGL((xent_fwd_reg_kernel<BF16, VEC, 64, XE_WAVE_NV>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, z, ldz, labels, B,
                           C, y_on, y_off, loss_i, aux, best, above);
    else if (C <= XE_BLOCK_MAX_C)
        hipLaunchKernelGGL((xent_fwd_reg_kernel<BF16, VEC, 256, XE_BLOCK_NV>), dim3((unsigned)B), dim3(256), 0, s, z, ldz, labels, B, C, y_on,
                           y_off, loss_i, aux, best, above);
    else
        hipLaunchKernelGGL((xent_fwd_stream_kernel<BF16, VEC>), dim3((unsigned)B), dim3(256), 0, s, z, ldz, labels, B, C, y_on, y_off, loss_i,
                           aux, best, above);
}

extern "C" int se_softmax_xent_fwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, int64_t B, int64_t C,
                                   float smoothing, float *loss_i, float *aux, int32_t *best, int32_t *above, float *loss_mean,
                                   se_stream_t stream)
{
    const int rc = xe_check("se_softmax_xent_fwd", logits, z_dtype, ldz, labels, B, C, smoothing, aux);
    if (rc != SE_OK) return rc;
    if (B > 0 && !loss_i) return fail(SE_ERR_INVALID, "se_softmax_xent_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (B > 0) {
        float y_on, y_off;
        xe_target(smoothing, C, y_on, y_off);
        const bool bf = z_dtype == SE_DTYPE_BF16;
        const bool vec = aligned16(logits, ldz, bf ? 2 : 4);
        dispatch_bools(bf, vec, [&](auto BF, auto VEC) {
            xe_launch_fwd<BF(), VEC()>(logits, ldz, labels, B, (int)C, y_on, y_off, loss_i, aux, best, above, s);
        });
        SE_LAUNCH_CHECK();
    }
    if (loss_mean) {
        launch_mean(loss_i, B, loss_mean, s);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}

template <bool ZBF, bool DBF, bool VEC>
static void xe_launch_bwd(const void *z, int64_t ldz, const int64_t *labels, const float *aux, const float *gl, float gs, int64_t B, int C,
                          float y_on, float y_off, void *dz, int64_t lddz, hipStream_t s)
{
    if (C <= XE_WAVE_MAX_C)
        hipLaunchKernelGGL((xent_bwd_kernel<ZBF, DBF, VEC, 64>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, z, ldz, labels, aux, gl, gs, B,
                           C, y_on, y_off, dz, lddz);
    else
        hipLaunchKernelGGL((xent_bwd_kernel<ZBF, DBF, VEC, 256>), dim3((unsigned)B), dim3(256), 0, s, z, ldz, labels, aux, gl, gs, B, C, y_on,
                           y_off, dz, lddz);
}

extern "C" int se_softmax_xent_bwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const float *aux,
                                   const float *grad_loss_i, float grad_scale, int64_t B, int64_t C, float smoothing, void *dz,
                                   int dz_dtype, int64_t lddz, se_stream_t stream)
{
    const int rc = xe_check("se_softmax_xent_bwd", logits, z_dtype, ldz, labels, B, C, smoothing, aux);
    if (rc != SE_OK) return rc;
    if (!is_float_dtype(dz_dtype)) return fail(SE_ERR_INVALID, "se_softmax_xent_bwd: bad dtype %d", dz_dtype);
    if (lddz < C) return fail(SE_ERR_INVALID, "se_softmax_xent_bwd: leading dimension %lld < C=%lld", (long long)lddz, (long long)C);
    if (B == 0) return SE_OK;
    if (!dz) return fail(SE_ERR_INVALID, "se_softmax_xent_bwd: null pointer");
    float y_on, y_off;
    xe_target(smoothing, C, y_on, y_off);
    const bool zbf = z_dtype == SE_DTYPE_BF16, dbf = dz_dtype == SE_DTYPE_BF16;
    const bool vec = aligned16(logits, ldz, zbf ? 2 : 4) && aligned16(dz, lddz, dbf ? 2 : 4);
    hipStream_t s = (hipStream_t)stream;
    dispatch_bools(zbf, dbf, vec, [&](auto ZBF, auto DBF, auto VEC) {
        xe_launch_bwd<ZBF(), DBF(), VEC()>(logits, ldz, labels, aux, grad_loss_i, grad_scale, B, (int)C, y_on, y_off, dz, lddz, s);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}
