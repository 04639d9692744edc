// labelembed.hip -- label-embedding baseline loss, forward + backward.
//
// Replaces `labelembed_loss(out1, out2, tar, targets, tau, alpha, beta)` (learn_labelembedding.py:21-37,
// with `cross_entropy` :17-18) and what TF autodiff derives from it.  Per sample i with label y:
//     L_o1_y   = -(log c_y - log sum_j c_j),  c = clip(softmax(out1), 1e-7, 1 - 1e-7)
//                (Keras 2.2 sparse_categorical_crossentropy on probabilities: clip, log, then TF's
//                 sparse_softmax_cross_entropy_with_logits, which renormalises the clipped probabilities)
//     L_o1_emb = -sum_c softmax(tar)_c * log_softmax(out1)_c          (softmax(tar) is stop_gradient)
//     L_o2_y   = the same on softmax(out2)
//     L_emb_o2 = -sum_c softmax(out2 / tau)_c * log_softmax(tar)_c * mask_i * B / (sum_j mask_j + 1e-8)
//                mask_i = [argmax(out2) == y]                         (softmax(out2/tau) and mask are stop_gradient)
//     L_re     = relu(softmax(out2)[y] - alpha)
//     loss_i   = beta L_o1_y + (1 - beta) L_o1_emb + L_o2_y + L_emb_o2 + L_re
//
// Layout: three [B, C] float32 logit matrices, one 64-lane wavefront per sample; every row statistic (3 maxima,
// 4 exp-sums, 2 weighted sums, the arg-max) is a DPP/shuffle wave reduction -- no LDS, no atomics.  The one
// batch-wide quantity, sum_j mask_j, is reduced in a fixed order by a single-block finish kernel, so results
// are run-to-run deterministic.  HBM-bound: 12 C bytes read per sample forward, 12 C read + 12 C written backward.
//
// The table form (se_labelembed_table_loss_fwd / _bwd) is the same pair of kernel bodies reading the `tar` row of sample i straight
// from the learned [C, C] label-embedding table (row clamp(targets[i])) instead of a materialised [B, C] gather, plus the gradient
// of that table: d_table[k] = sum over {i : clamp(targets[i]) = k} of the d_tar row of sample i, added from +0 in INCREASING i.
// Layout of that reduction: one wave owns 256 columns of one table row k and walks its class's batch rows with the fixed-order scan
// of class_scan.h (the order and constants of the centroid gradient of center_loss.hip); softmax(table[k]) is evaluated once, at the
// first matched row, and stays in registers.
#include "class_scan.h"

namespace se {

constexpr int LE_ROWS_PER_BLOCK = 4;   // 4 waves = 256 threads
constexpr float KERAS_EPS = 1e-7f;     // keras.backend.epsilon(): probabilities are clipped to [eps, 1 - eps]
constexpr int LE_AUX = 12;             // per-sample record kept for the backward pass
using class_scan::WAVES, class_scan::COLS, class_scan::ROWS;    // table gradient: a wave owns 256 columns of one table row

// aux[i] = { lse(out1), lse(out2), lse(tar), lse(out2 / tau), mask, A_i = -sum tau2 * log_softmax(tar), base_i, p2_y,
//            S1 = sum_j clip(p1_j), R1 = sum_j 1{eps < p1_j < 1 - eps} p1_j, S2, R2 }
// TABLE: `tar` is the [C, C] table and the row of a sample is the row of its (clamped) label; otherwise the [B, C] gather.
template <bool TABLE>
__global__ __launch_bounds__(256) void labelembed_fwd_kernel(
    const float *__restrict__ out1, int64_t ld1, const float *__restrict__ out2, int64_t ld2, const float *__restrict__ tar, int64_t ldt,
    const int64_t *__restrict__ targets, int64_t B, int64_t C, float tau, float alpha, float beta, float *__restrict__ aux)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const float inv_tau = 1.0f / tau;
    for (int64_t row = (int64_t)blockIdx.x * LE_ROWS_PER_BLOCK + wave; row < B; row += (int64_t)gridDim.x * LE_ROWS_PER_BLOCK) {
        const float *o1 = out1 + row * ld1, *o2 = out2 + row * ld2, *tr = tar + row * ldt;
        const int64_t y = clamp_label(targets[row], C);
        if constexpr (TABLE) tr = tar + y * ldt;
        // pass 1: maxima and the arg-max of out2 (first maximum, like K.argmax)
        float m1 = -INFINITY, m2 = -INFINITY, mt = -INFINITY;
        int64_t am = 0;
        for (int64_t c = lane; c < C; c += WAVE) {
            m1 = fmaxf(m1, o1[c]);
            mt = fmaxf(mt, tr[c]);
            const float v = o2[c];
            if (v > m2) { m2 = v; am = c; }
        }
        m1 = wave_max(m1);
        mt = wave_max(mt);
        const float m2w = wave_max(m2);
        const int64_t cand = wave_min((m2 == m2w) ? am : C);      // lowest column holding the row maximum
        // pass 2: exp-sums and the two weighted sums
        float s1 = 0.f, s2 = 0.f, st = 0.f, s2t = 0.f, w_t_o1 = 0.f, w_tau_t = 0.f;
        for (int64_t c = lane; c < C; c += WAVE) {
            const float a = o1[c], b = o2[c], t = tr[c];
            s1 += expf(a - m1);
            s2 += expf(b - m2w);
            const float et = expf(t - mt), e2t = expf((b - m2w) * inv_tau);
            st += et;
            s2t += e2t;
            w_t_o1 += et * a;     // sum_c exp(t_c - mt) * out1_c
            w_tau_t += e2t * t;   // sum_c exp((o2_c - m2) / tau) * tar_c
        }
        s1 = wave_sum(s1); s2 = wave_sum(s2); st = wave_sum(st); s2t = wave_sum(s2t);
        w_t_o1 = wave_sum(w_t_o1); w_tau_t = wave_sum(w_tau_t);
        const float lse1 = m1 + logf(s1), lse2 = m2w + logf(s2);
        // pass 3: sums of the clipped probabilities (the renormalisation inside Keras' sparse CE) and of the un-clipped ones
        float S1 = 0.f, R1 = 0.f, S2 = 0.f, R2 = 0.f;
        for (int64_t c = lane; c < C; c += WAVE) {
            const float p1 = expf(o1[c] - lse1), p2 = expf(o2[c] - lse2);
            S1 += fminf(fmaxf(p1, KERAS_EPS), 1.0f - KERAS_EPS);
            S2 += fminf(fmaxf(p2, KERAS_EPS), 1.0f - KERAS_EPS);
            R1 += (p1 > KERAS_EPS && p1 < 1.0f - KERAS_EPS) ? p1 : 0.f;
            R2 += (p2 > KERAS_EPS && p2 < 1.0f - KERAS_EPS) ? p2 : 0.f;
        }
        S1 = wave_sum(S1); S2 = wave_sum(S2); R1 = wave_sum(R1); R2 = wave_sum(R2);
        if (lane == 0) {
            const float lset = mt + logf(st), lse2t = m2w * inv_tau + logf(s2t);
            const float p1y = expf(o1[y] - lse1), p2y = expf(o2[y] - lse2);
            const float l_o1_y = -(logf(fminf(fmaxf(p1y, KERAS_EPS), 1.0f - KERAS_EPS)) - logf(S1));
            const float l_o2_y = -(logf(fminf(fmaxf(p2y, KERAS_EPS), 1.0f - KERAS_EPS)) - logf(S2));
            const float l_o1_emb = -(w_t_o1 / st - lse1);         // -sum softmax(tar) * (out1 - lse1)
            const float a_i = -(w_tau_t / s2t - lset);            // -sum softmax(out2/tau) * (tar - lset)
            const float l_re = fmaxf(p2y - alpha, 0.f);
            float *r = aux + row * LE_AUX;
            r[0] = lse1; r[1] = lse2; r[2] = lset; r[3] = lse2t;
            r[4] = (cand == y) ? 1.0f : 0.0f;
            r[5] = a_i;
            r[6] = beta * l_o1_y + (1.0f - beta) * l_o1_emb + l_o2_y + l_re;
            r[7] = p2y;
            r[8] = S1; r[9] = R1; r[10] = S2; r[11] = R2;
        }
    }
}

// One block: sum of the masks in a fixed order -> scale = B / (sum + 1e-8); loss_i = base_i + A_i mask_i scale.
__global__ __launch_bounds__(256) void labelembed_finish_kernel(const float *__restrict__ aux, int64_t B, float *__restrict__ loss_i,
                                                                float *__restrict__ scale_out)
{
    __shared__ float part[256];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < B; i += 256) s += aux[i * LE_AUX + 4];
    const float scale = (float)B / (block_sum_256(s, part) + 1e-8f);
    if (threadIdx.x == 0) scale_out[0] = scale;
    for (int64_t i = threadIdx.x; i < B; i += 256) loss_i[i] = aux[i * LE_AUX + 6] + aux[i * LE_AUX + 5] * aux[i * LE_AUX + 4] * scale;
}

// With in_j = 1{eps < p_j < 1 - eps} (clip_by_value passes gradient strictly inside the range), S = sum_j clip(p_j), R = sum_j in_j p_j:
//   ce'(p)_c = in_y (p_c - onehot_c) + p_c (in_c - R) / S          (= p - onehot when nothing is clipped)
// d out1 = g [ beta ce'(softmax1) + (1 - beta) (softmax1 - softmax(tar)) ]
// d out2 = g [ ce'(softmax2) + 1{p2_y > alpha} p2_y (onehot_y - softmax2) ]
// d tar  = g mask_i scale (softmax(tar) - softmax(out2 / tau))
template <bool TABLE>
__global__ __launch_bounds__(256) void labelembed_bwd_kernel(const float *__restrict__ out1, int64_t ld1, const float *__restrict__ out2,
                                                             int64_t ld2, const float *__restrict__ tar, int64_t ldt,
                                                             const int64_t *__restrict__ targets, const float *__restrict__ grad_loss_i,
                                                             float grad_scale, int64_t B, int64_t C, float tau, float alpha, float beta,
                                                             const float *__restrict__ aux, const float *__restrict__ scale,
                                                             float *__restrict__ d1, int64_t ldd1, float *__restrict__ d2, int64_t ldd2,
                                                             float *__restrict__ dt, int64_t lddt)
{
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const float inv_tau = 1.0f / tau, sc = scale[0];
    for (int64_t row = (int64_t)blockIdx.x * LE_ROWS_PER_BLOCK + wave; row < B; row += (int64_t)gridDim.x * LE_ROWS_PER_BLOCK) {
        const float *o1 = out1 + row * ld1, *o2 = out2 + row * ld2, *tr = tar + row * ldt;
        const int64_t y = clamp_label(targets[row], C);
        if constexpr (TABLE) tr = tar + y * ldt;
        const float *r = aux + row * LE_AUX;
        const float lse1 = r[0], lse2 = r[1], lset = r[2], lse2t = r[3], mask = r[4], p2y = r[7];
        const float g = grad_loss_i ? grad_loss_i[row] : grad_scale;
        const float p1y = expf(o1[y] - lse1);
        const float k1 = (p1y > KERAS_EPS && p1y < 1.0f - KERAS_EPS) ? 1.f : 0.f;   // clip_by_value passes gradient inside the range only
        const float k2 = (p2y > KERAS_EPS && p2y < 1.0f - KERAS_EPS) ? 1.f : 0.f;
        const float rS1 = 1.0f / r[8], R1 = r[9], rS2 = 1.0f / r[10], R2 = r[11];
        const float kre = (p2y > alpha) ? p2y : 0.f;
        const float wt = g * mask * sc;
        for (int64_t c = lane; c < C; c += WAVE) {
            const float sm1 = expf(o1[c] - lse1), sm2 = expf(o2[c] - lse2), smt = expf(tr[c] - lset);
            const float sm2t = expf(o2[c] * inv_tau - lse2t);
            const float hot = (c == y) ? 1.f : 0.f;
            const float in1 = (sm1 > KERAS_EPS && sm1 < 1.0f - KERAS_EPS) ? 1.f : 0.f, in2 = (sm2 > KERAS_EPS && sm2 < 1.0f - KERAS_EPS) ? 1.f : 0.f;
            if (d1) d1[row * ldd1 + c] = g * (beta * (k1 * (sm1 - hot) + sm1 * (in1 - R1) * rS1) + (1.0f - beta) * (sm1 - smt));
            if (d2) d2[row * ldd2 + c] = g * ((k2 * (sm2 - hot) + sm2 * (in2 - R2) * rS2) + kre * (hot - sm2));
            if (dt) dt[row * lddt + c] = wt * (smt - sm2t);
        }
    }
}

// d_table[k, c] = sum over {i : clamp(targets[i]) = k}, in increasing i from +0, of wt_i (softmax(table[k])_c - softmax(out2_i / tau)_c):
// the value labelembed_bwd_kernel writes to d_tar[i, c], by the same operations (-ffp-contract=off: no fma).  Rows with wt_i == 0
// (mask_i = 0: most rows early in training) are skipped; they would add +-0 to a sum that starts at +0.
__global__ __launch_bounds__(64 * WAVES) void labelembed_table_grad_kernel(
    const float *__restrict__ out2, int64_t ld2, const float *__restrict__ table, int64_t ldtab, const int64_t *__restrict__ targets,
    const float *__restrict__ grad_loss_i, float grad_scale, int64_t B, int64_t C, float tau, const float *__restrict__ aux,
    float *__restrict__ dtab, int64_t lddtab)
{
    const int lane = lane_id();
    const int64_t k = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);      // wave-uniform
    if (k >= C) return;
    const int64_t c0 = (int64_t)blockIdx.y * (64 * COLS);
    const float inv_tau = 1.0f / tau, sc = B > 0 ? aux[B * LE_AUX] : 0.f;
    float acc[COLS], smt[COLS];
#pragma unroll
    for (int r = 0; r < COLS; r++) acc[r] = smt[r] = 0.f;
    bool have_smt = false;
    float wt = 0.f, lset = 0.f, lse2t = 0.f;                                                   // this lane's row of the current chunk, if it is one of class k
    class_scan::scan(
        targets, B, C, k,
        [&](int64_t i, bool mine) {
            wt = 0.f; lset = 0.f; lse2t = 0.f;
            if (mine) {
                const float *r = aux + i * LE_AUX;
                const float g = grad_loss_i ? grad_loss_i[i] : grad_scale;
                wt = g * r[4] * sc;
                lset = r[2];
                lse2t = r[3];
            }
            return mine && wt != 0.f;
        },
        [&](int first) {
            if (have_smt) return;                                               // softmax(table[k]): once per class, kept in registers
            const float l = __shfl(lset, first, 64);                            // every row of the class holds the same lse(table[k])
#pragma unroll
            for (int r = 0; r < COLS; r++) {
                const int64_t c = c0 + r * 64 + lane;
                smt[r] = c < C ? expf(table[k * ldtab + c] - l) : 0.f;
            }
            have_smt = true;
        },
        [&](const class_scan::Group &g) {
            float w[ROWS], l2[ROWS], v[ROWS][COLS];
#pragma unroll
            for (int q = 0; q < ROWS; q++) {
                w[q] = __shfl(wt, g.lane[q], 64);
                l2[q] = __shfl(lse2t, g.lane[q], 64);
                const float *o2 = out2 + g.row[q] * ld2;
#pragma unroll
                for (int r = 0; r < COLS; r++) {
                    const int64_t c = c0 + r * 64 + lane;
                    v[q][r] = c < C ? o2[c] : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < ROWS; q++) {
                if (q < g.n) {
#pragma unroll
                    for (int r = 0; r < COLS; r++) {
                        const float sm2t = expf(v[q][r] * inv_tau - l2[q]);
                        const float p = w[q] * (smt[r] - sm2t);
                        acc[r] = acc[r] + p;
                    }
                }
            }
        });
#pragma unroll
    for (int r = 0; r < COLS; r++) {
        const int64_t c = c0 + r * 64 + lane;
        if (c < C) dtab[k * lddtab + c] = acc[r];
    }
}

}  // namespace se

using namespace se;

static int le_grid(int64_t B)
{
    int64_t g = (B + LE_ROWS_PER_BLOCK - 1) / LE_ROWS_PER_BLOCK;
    return (int)(g < 1 ? 1 : (g > SE_LABELEMBED_GRID_CAP ? SE_LABELEMBED_GRID_CAP : g));
}

extern "C" int64_t se_labelembed_aux_floats(int64_t B) { return B > 0 ? B * LE_AUX + 4 : 0; }

// The plain and the table entry points differ in where a sample's `tar` row lives (TABLE) and, backwards, in a few checks and in the
// table's own gradient; `who` names the entry point in the error texts.
template <bool TABLE>
static int labelembed_fwd(const char *who, const float *out1, int64_t ld1, const float *out2, int64_t ld2, const float *tar, int64_t ldt,
                          const int64_t *targets, int64_t B, int64_t C, float tau, float alpha, float beta, float *loss_i, float *aux,
                          se_stream_t stream)
{
    if (B < 0 || C <= 0) return fail(SE_ERR_INVALID, "%s: bad shape B=%lld C=%lld", who, (long long)B, (long long)C);
    if (B == 0) return SE_OK;
    if (!out1 || !out2 || !tar || !targets || !loss_i || !aux) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (ld1 < C || ld2 < C || ldt < C) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    if (!(tau > 0.f)) return fail(SE_ERR_INVALID, "%s: tau must be positive", who);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(labelembed_fwd_kernel<TABLE>, dim3(le_grid(B)), dim3(256), 0, s, out1, ld1, out2, ld2, tar, ldt, targets, B, C, tau,
                       alpha, beta, aux);
    SE_LAUNCH_CHECK();
    hipLaunchKernelGGL(labelembed_finish_kernel, dim3(1), dim3(256), 0, s, aux, B, loss_i, aux + B * LE_AUX);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

// d_tar: the [B, C] gradient of the gather, or (TABLE) the [C, C] gradient of the table.  The plain form has nothing to write at
// B == 0 and never looked at tau or the input pitches; the table form writes every row of d_tar at any B (all +0 at B == 0).
template <bool TABLE>
static int labelembed_bwd(const char *who, const float *out1, int64_t ld1, const float *out2, int64_t ld2, const float *tar, int64_t ldt,
                          const int64_t *targets, const float *grad_loss_i, float grad_scale, int64_t B, int64_t C, float tau, float alpha,
                          float beta, const float *aux, float *d_out1, int64_t ldd1, float *d_out2, int64_t ldd2, float *d_tar, int64_t lddt,
                          se_stream_t stream)
{
    if (B < 0 || C <= 0) return fail(SE_ERR_INVALID, "%s: bad shape B=%lld C=%lld", who, (long long)B, (long long)C);
    if (!TABLE && B == 0) return SE_OK;
    if (B > 0 && (!out1 || !out2 || !tar || !targets || !aux)) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (TABLE && B > 0 && (ld1 < C || ld2 < C || ldt < C)) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    if ((d_out1 && ldd1 < C) || (d_out2 && ldd2 < C) || (d_tar && lddt < C)) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    if (TABLE && !(tau > 0.f)) return fail(SE_ERR_INVALID, "%s: tau must be positive", who);
    hipStream_t s = (hipStream_t)stream;
    if (B > 0 && (!TABLE || d_out1 || d_out2)) {
        hipLaunchKernelGGL(labelembed_bwd_kernel<TABLE>, dim3(le_grid(B)), dim3(256), 0, s, out1, ld1, out2, ld2, tar, ldt, targets, grad_loss_i,
                           grad_scale, B, C, tau, alpha, beta, aux, aux + B * LE_AUX, d_out1, ldd1, d_out2, ldd2,
                           TABLE ? (float *)nullptr : d_tar, TABLE ? (int64_t)0 : lddt);
        SE_LAUNCH_CHECK();
    }
    if (TABLE && d_tar) {
        const int64_t bx = (C + WAVES - 1) / WAVES, by = (C + 64 * COLS - 1) / (64 * COLS);
        if (bx > 0x7FFFFFFF || by > 65535) return fail(SE_ERR_UNSUPPORTED, "%s: C too large", who);
        hipLaunchKernelGGL(labelembed_table_grad_kernel, dim3((unsigned)bx, (unsigned)by), dim3(64 * WAVES), 0, s, out2, ld2, tar, ldt,
                           targets, grad_loss_i, grad_scale, B, C, tau, aux, d_tar, lddt);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}

extern "C" int se_labelembed_loss_fwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2, const float *tar,
                                      int64_t ldt, const int64_t *targets, int64_t B, int64_t C, float tau, float alpha,
                                      float beta, float *loss_i, float *aux, se_stream_t stream)
{
    return labelembed_fwd<false>("se_labelembed_loss_fwd", out1, ld1, out2, ld2, tar, ldt, targets, B, C, tau, alpha, beta, loss_i, aux, stream);
}

extern "C" int se_labelembed_loss_bwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2, const float *tar,
                                      int64_t ldt, const int64_t *targets, const float *grad_loss_i, float grad_scale,
                                      int64_t B, int64_t C, float tau, float alpha, float beta, const float *aux,
                                      float *d_out1, int64_t ldd1, float *d_out2, int64_t ldd2, float *d_tar, int64_t lddt,
                                      se_stream_t stream)
{
    return labelembed_bwd<false>("se_labelembed_loss_bwd", out1, ld1, out2, ld2, tar, ldt, targets, grad_loss_i, grad_scale, B, C, tau, alpha,
                                 beta, aux, d_out1, ldd1, d_out2, ldd2, d_tar, lddt, stream);
}

extern "C" int se_labelembed_table_loss_fwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2, const float *table,
                                            int64_t ldtab, const int64_t *targets, int64_t B, int64_t C, float tau, float alpha,
                                            float beta, float *loss_i, float *aux, se_stream_t stream)
{
    return labelembed_fwd<true>("se_labelembed_table_loss_fwd", out1, ld1, out2, ld2, table, ldtab, targets, B, C, tau, alpha, beta, loss_i, aux,
                                stream);
}

extern "C" int se_labelembed_table_loss_bwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2, const float *table,
                                            int64_t ldtab, const int64_t *targets, const float *grad_loss_i, float grad_scale,
                                            int64_t B, int64_t C, float tau, float alpha, float beta, const float *aux,
                                            float *d_out1, int64_t ldd1, float *d_out2, int64_t ldd2, float *d_table, int64_t lddtab,
                                            se_stream_t stream)
{
    return labelembed_bwd<true>("se_labelembed_table_loss_bwd", out1, ld1, out2, ld2, table, ldtab, targets, grad_loss_i, grad_scale, B, C, tau,
                                alpha, beta, aux, d_out1, ldd1, d_out2, ldd2, d_table, lddtab, stream);
}
