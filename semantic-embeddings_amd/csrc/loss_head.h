// loss_head.h -- what the loss heads share: the per-row chains of the cosine and squared-distance losses with the host predicates
// that pick their 16-byte paths, and the epilogue of the nearest-class metric on the 32 x 32 tile of tile32.h.  se_embed_head_fwd
// (embed_head.hip) promises the bytes of se_cosine_loss_fwd / se_sqdist_loss_fwd / se_nn_accuracy (loss_kernels.hip); both files take
// every piece of that promise from here, so there is one text to edit.
#pragma once
#include "se_common.h"
#include "tile32.h"

namespace se {

constexpr float L2NORM_EPS = 1e-12f;    // tf.nn.l2_normalize default epsilon (TF 1.x)

// ---- row chains: one 64-lane wavefront owns one feature row; every lane gets the totals ----

// ss = sum x^2, dt = sum x * t over one row
template <bool BF16>
__device__ __forceinline__ void row_reduce(const void *xrow, const float *trow, int64_t D, bool vec_ok, float &ss, float &dt)
{
    const int lane = lane_id();
    float s = 0.f, t = 0.f;
    if (vec_ok) {
        if constexpr (BF16) {
            const uint4 *xv = (const uint4 *)xrow;  // 8 bf16 per 16 B
            const float4 *tv = (const float4 *)trow;
            for (int64_t i = lane; i < D / 8; i += WAVE) {
                uint4 p = xv[i];
                float4 t0 = tv[2 * i], t1 = tv[2 * i + 1];
                float xs[8];
                unpack_bf16x8(p, xs);
                float ts[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    s = fmaf(xs[j], xs[j], s);
                    t = fmaf(xs[j], ts[j], t);
                }
            }
        } else {
            const float4 *xv = (const float4 *)xrow;
            const float4 *tv = (const float4 *)trow;
            for (int64_t i = lane; i < D / 4; i += WAVE) {
                float4 p = xv[i], q = tv[i];
                s = fmaf(p.x, p.x, s); s = fmaf(p.y, p.y, s); s = fmaf(p.z, p.z, s); s = fmaf(p.w, p.w, s);
                t = fmaf(p.x, q.x, t); t = fmaf(p.y, q.y, t); t = fmaf(p.z, q.z, t); t = fmaf(p.w, q.w, t);
            }
        }
    } else {
        for (int64_t i = lane; i < D; i += WAVE) {
            float p = ld_elem<BF16>(xrow, i);
            s = fmaf(p, p, s);
            t = fmaf(p, trow[i], t);
        }
    }
    ss = wave_sum(s);
    dt = wave_sum(t);
}

// sum (x - t)^2 over one row (bf16 rows have no 16-byte path)
template <bool BF16>
__device__ __forceinline__ float row_sqdist(const void *xrow, const float *trow, int64_t D, bool vec_ok)
{
    const int lane = lane_id();
    float s = 0.f;
    if (vec_ok && !BF16) {
        const float4 *xv = (const float4 *)xrow, *tv = (const float4 *)trow;
        for (int64_t i = lane; i < D / 4; i += WAVE) {
            const float4 p = xv[i], q = tv[i];
            const float a = p.x - q.x, b = p.y - q.y, c = p.z - q.z, e = p.w - q.w;
            s = fmaf(a, a, s); s = fmaf(b, b, s); s = fmaf(c, c, s); s = fmaf(e, e, s);
        }
    } else {
        for (int64_t i = lane; i < D; i += WAVE) {
            const float a = ld_elem<BF16>(xrow, i) - trow[i];
            s = fmaf(a, a, s);
        }
    }
    return wave_sum(s);
}

// xhat row = x row * inv_norm
template <bool BF16>
__device__ __forceinline__ void write_xhat_row(const void *xrow, float *orow, int64_t D, bool vec_ok, float inv)
{
    const int lane = lane_id();
    if (vec_ok && !BF16) {
        const float4 *xv = (const float4 *)xrow;
        float4 *ov = (float4 *)orow;
        for (int64_t i = lane; i < D / 4; i += WAVE) {
            float4 p = xv[i];
            ov[i] = make_float4(p.x * inv, p.y * inv, p.z * inv, p.w * inv);
        }
    } else {
        for (int64_t i = lane; i < D; i += WAVE) orow[i] = ld_elem<BF16>(xrow, i) * inv;
    }
}

// Host: do the rows of a launch take the 16-byte paths above?  The answer fixes the summation order of the row chains, so every
// entry point that promises another one's bytes asks here.  xhat: the optional output of the cosine forward (nullptr: none).
inline int cosine_rows_vec16(const void *x, int x_dtype, int64_t ldx, const float *emb, int64_t lde, int64_t D, const float *xhat = nullptr,
                             int64_t ldxhat = 0)
{
    const int vq = x_dtype == SE_DTYPE_BF16 ? 8 : 4;
    return (D % vq == 0) && (ldx % vq == 0) && (lde % 4 == 0) && aligned16(x) && aligned16(emb) &&
           (!xhat || ((ldxhat % 4 == 0) && aligned16(xhat)));
}

inline int sqdist_rows_vec16(const void *x, int x_dtype, int64_t ldx, const float *emb, int64_t lde, int64_t D)
{
    return x_dtype != SE_DTYPE_BF16 && (D % 4 == 0) && (ldx % 4 == 0) && (lde % 4 == 0) && aligned16(x) && aligned16(emb);
}

// ---- nearest-class metric on the 32 x 32 tile: a lane holds 16 samples (tile32::acc_row) of ONE class, column lane & 31 ----
// Instead of materialising top-k, the metric uses the equivalent counting form  acc = (#within >= 1) && (#better < k)
// with  within = |score - true| < 1e-6,  better = score beyond true by >= 1e-6   (utils.py:84-95).
// dot: scores are dot products (larger is better), else squared Euclidean distances |p|^2 + |e|^2 - 2 p.e (smaller is better).
namespace metric {

constexpr int NO_CLASS = 0x7FFFFFFF;   // "no class seen yet": loses every lower-index tie

// what a lane keeps per accumulator register (= per sample) while it walks its classes
struct Tally {
    int n_better, n_within;     // classes beyond the true class's score by >= 1e-6 / within 1e-6 of it
    float best_v; int best_c;   // best score so far and its class
};

__device__ __forceinline__ Tally empty_tally(bool dot) { return {0, 0, dot ? -INFINITY : INFINITY, NO_CLASS}; }

// |emb_c|^2 of this lane's class beside the four MFMA steps of one 16-byte operand read (half of the k per lane)
__device__ __forceinline__ float class_norm_steps(float cn, const float4 &b4, int s, int steps)
{
    cn = fmaf(b4.x, b4.x, cn);
    if (s + 1 < steps) cn = fmaf(b4.y, b4.y, cn);
    if (s + 2 < steps) cn = fmaf(b4.z, b4.z, cn);
    if (s + 3 < steps) cn = fmaf(b4.w, b4.w, cn);
    return cn;
}

// one accumulator register of a finished class tile: a = p . e of sample `row` (lr within its strip of 32) against class c;
// sPn / sTrue: |p|^2 and the true class's score per sample of the strip; cn: |e_c|^2 (both read by distances only).
// scores: optional [B, lds_] output.
__device__ __forceinline__ void update(Tally &t, bool dot, float a, const float *sPn, const float &cn, const float *sTrue, int lr,
                                       int64_t row, int64_t B, int64_t c, int64_t C, float *scores, int64_t lds_)
{
    float sc = a;
    if (!dot) sc = (sPn[lr] + cn) - 2.0f * sc;
    const bool valid = (c < C) && (row < B);
    if (valid) {
        if (scores) scores[row * lds_ + c] = sc;
        const float diff = dot ? (sc - sTrue[lr]) : (sTrue[lr] - sc);  // > 0: better than true
        if (fabsf(diff) < 1e-6f) t.n_within++;
        else if (diff >= 1e-6f) t.n_better++;
        const bool better = dot ? (sc > t.best_v) : (sc < t.best_v);
        if (better) { t.best_v = sc; t.best_c = (int)c; }
    }
}

// over the 32 lanes (classes) that share lane >> 5: counts add up, the best class wins by score, then by the LOWER index
__device__ __forceinline__ void reduce32(Tally &t, bool dot)
{
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        t.n_better += __shfl_xor(t.n_better, off, 64);
        t.n_within += __shfl_xor(t.n_within, off, 64);
        const float ov = __shfl_xor(t.best_v, off, 64);
        const int oc = __shfl_xor(t.best_c, off, 64);
        const bool take = dot ? (ov > t.best_v || (ov == t.best_v && oc < t.best_c))
                              : (ov < t.best_v || (ov == t.best_v && oc < t.best_c));
        if (take) { t.best_v = ov; t.best_c = oc; }
    }
}

// best class of a set as one ordered word for atomicMax: score (larger word = better), then the LOWER class index.  0 = empty set.
__device__ __forceinline__ unsigned long long best_word(float v, int c, bool dot)
{
    if (v == 0.f) v = 0.f;                                     // -0 ties with +0
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);            // ascending with the value
    if (!dot) u = ~u;                                          // distances: smaller is better
    return ((unsigned long long)u << 32) | (uint32_t)(NO_CLASS - c);
}

__device__ __forceinline__ int32_t best_class(unsigned long long word) { return NO_CLASS - (int32_t)(uint32_t)(word & 0xFFFFFFFFull); }

// Workspace of a launch whose class set is cut into slices: per sample one best word, then two counters (n_better, n_within); then
// `tickets` 32-bit arrival counters (none: nullptr), padded to 8 bytes.  The caller zeroes all of it.
struct Workspace { unsigned long long *part_best; uint32_t *part_cnt, *ticket; };

inline int64_t workspace_bytes(int64_t B, int64_t tickets) { return B * 16 + (tickets * 4 + 7) / 8 * 8; }

inline Workspace workspace(void *ws, int64_t B, bool sliced, bool tickets)
{
    return {(unsigned long long *)ws, sliced ? (uint32_t *)((char *)ws + B * 8) : nullptr,
            sliced && tickets ? (uint32_t *)((char *)ws + B * 16) : nullptr};
}

}  // namespace metric
}  // namespace se
