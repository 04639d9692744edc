// softmax_xent.h -- the row code of the softmax cross-entropy (softmax_xent.hip explains the arithmetic): what one wave or one
// workgroup does with its row of logits, forward on the register paths and backward.  se_softmax_xent_fwd / _bwd (softmax_xent.hip)
// and the classifier role of se_joint_head_fwd / _bwd (joint_head.hip) both run this text, so the joint head carries the bits of
// the stand-alone entry points by construction.  The hierarchy-aware losses of hxe.hip share the per-value scan (xe_scan), the
// bad-row / arg-max rules, the row writers and the load / store helpers, so their metrics are this file's as well.
#pragma once
#include "se_common.h"
#include <limits.h>

namespace se {

constexpr float XE_LO = 1.1920929e-7f;     // -log(1 - eps), eps = float32(1e-7)
constexpr float XE_HI = 16.118095f;        // -log(eps)
constexpr int XE_WAVE_NV = 16;             // values per lane of the wave path:        C <= 64 * 16
constexpr int XE_BLOCK_NV = 32;            // values per thread of the workgroup path: C <= 256 * 32
constexpr int XE_WAVE_MAX_C = 64 * XE_WAVE_NV, XE_BLOCK_MAX_C = 256 * XE_BLOCK_NV;

// E consecutive values from column c0 (16-byte aligned address): E = 4 or 8 float32 (one or two 16-byte loads), E = 8 bf16 (one)
template <bool BF16, int E>
__device__ __forceinline__ void xe_ld_vec(const void *row, int64_t c0, float *v)
{
    if constexpr (BF16) {
        static_assert(E == 8, "bf16 units hold 8 values");
        unpack_bf16x8(*(const uint4 *)((const uint16_t *)row + c0), v);
    } else {
#pragma unroll
        for (int k = 0; k < E; k += 4) {
            const float4 p = *(const float4 *)((const float *)row + c0 + k);
            v[k] = p.x; v[k + 1] = p.y; v[k + 2] = p.z; v[k + 3] = p.w;
        }
    }
}

template <bool BF16, int E>
__device__ __forceinline__ void xe_st_vec(void *row, int64_t c0, const float *v)
{
    if constexpr (BF16) {
        static_assert(E == 8, "bf16 units hold 8 values");
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = (uint32_t)f32_to_bf16(v[2 * k]) | ((uint32_t)f32_to_bf16(v[2 * k + 1]) << 16);
        *(uint4 *)((uint16_t *)row + c0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < E; k += 4) *(float4 *)((float *)row + c0 + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
}

// sum of a[0 .. N) as a balanced tree (N a power of two); a is consumed
template <int N>
__device__ __forceinline__ float xe_tree_sum(float *a)
{
#pragma unroll
    for (int stride = 1; stride < N; stride *= 2)
#pragma unroll
        for (int i = 0; i < N; i += 2 * stride) a[i] += a[i + stride];
    return a[0];
}

__device__ __forceinline__ float xe_clamp(float t) { return fminf(fmaxf(t, XE_LO), XE_HI); }
__device__ __forceinline__ bool xe_inside(float t) { return t >= XE_LO && t <= XE_HI; }      // false for NaN

// The values a row statistic needs from every wave of a 256-thread workgroup (slot: one per reduction, never reused within a row)
struct XeShared {
    float f[4][4];
    int i[3][4];
};

// A row that holds a NaN or +inf, or nothing but -inf, has no softmax (nan_at: column of its first NaN, INT_MAX: none; M: its maximum)
__device__ __forceinline__ bool xe_bad_row(int nan_at, float M) { return nan_at != INT_MAX || M == INFINITY || M == -INFINITY; }
// np.argmax of a row: its first NaN, else the first maximum (cand; INT_MAX: every value is -inf, class 0)
__device__ __forceinline__ int xe_best_class(int nan_at, int cand) { return nan_at != INT_MAX ? nan_at : (cand == INT_MAX ? 0 : cand); }

// one value of a row's scan (columns ascend within a thread): first NaN, first maximum, classes strictly above the label's logit
__device__ __forceinline__ void xe_scan(float x, int c, float zy, float &m, int &am, int &nan_at, int &cnt)
{
    if (x != x) nan_at = min(nan_at, c);
    if (x > m) { m = x; am = c; }
    cnt += x > zy ? 1 : 0;
}

// the metrics of a row, shared by every loss on softmax logits (hxe.hip writes them with a loss of its own)
__device__ __forceinline__ void xe_write_metrics(int64_t row, int C, bool bad, int nan_at, int cand, int cnt, int32_t *__restrict__ best,
                                                 int32_t *__restrict__ above)
{
    if (best) best[row] = xe_best_class(nan_at, cand);
    if (above) above[row] = bad ? C : cnt;
}

// what the last step of every forward path writes for its row
__device__ __forceinline__ void xe_write_row(int64_t row, int64_t B, int C, bool bad, float loss, float m, float logsum, float A, int nan_at, int cand,
                                             int cnt, float *__restrict__ loss_i, float *__restrict__ aux, int32_t *__restrict__ best,
                                             int32_t *__restrict__ above)
{
    const float nan = __uint_as_float(0x7FC00000u);
    loss_i[row] = bad ? nan : loss;
    aux[row] = bad ? nan : m;
    aux[B + row] = bad ? nan : logsum;
    aux[2 * B + row] = bad ? nan : A;
    xe_write_metrics(row, C, bad, nan_at, cand, cnt, best, above);
}

// E values of a row from column c0, -inf past the row's end
template <bool BF16, int E>
__device__ __forceinline__ void xe_ld_unit(const void *zrow, int64_t c0, int C, float *v)
{
    if constexpr (E > 1) {
        if (c0 + E <= C) {
            xe_ld_vec<BF16, E>(zrow, c0, v);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < E; k++) v[k] = c0 + k < C ? ld_elem<BF16>(zrow, c0 + k) : -INFINITY;
}

// Register paths.  G = 64: a wave per row, 4 rows per workgroup; G = 256: a workgroup per row.  Value slot s of thread t is column
// ((s / E) * G + t) * E + s % E with 16-byte loads (E values each), s * G + t with scalar loads: ascending in s either way.
// `block`: which group of 256 / G consecutive rows this workgroup takes (all 256 threads call).
template <bool BF16, bool VEC, int G, int NV>
__device__ __forceinline__ void xe_fwd_reg_rows(int64_t block, const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                int64_t B, int C, float y_on, float y_off, float *__restrict__ loss_i,
                                                float *__restrict__ aux, int32_t *__restrict__ best, int32_t *__restrict__ above)
{
    constexpr int E = VEC ? (BF16 ? 8 : 4) : 1;
    static_assert(NV % E == 0, "whole units per thread");
    const int t = threadIdx.x % G, wave = threadIdx.x >> 6;
    const int64_t row = block * (256 / G) + threadIdx.x / G;
    if (row >= B) return;                                   // G = 64: the whole wave leaves (this path has no barrier); G = 256: never
    const void *zrow = BF16 ? (const void *)((const uint16_t *)z + row * ldz) : (const void *)((const float *)z + row * ldz);
    const int y = (int)clamp_label(labels[row], C);
    const float zy = ld_elem<BF16>(zrow, y);
    auto col = [&](int s) { return VEC ? ((s / E) * G + t) * E + s % E : s * G + t; };

    float v[NV];
#pragma unroll
    for (int j = 0; j < NV / E; j++) {
        xe_ld_unit<BF16, E>(zrow, col(j * E), C, v + j * E);
    }

    float m = -INFINITY;
    int am = INT_MAX, nan_at = INT_MAX, cnt = 0;
#pragma unroll
    for (int s = 0; s < NV; s++) {
        xe_scan(v[s], col(s), zy, m, am, nan_at, cnt);
    }
    __shared__ XeShared sh;
    float M = wave_max(m);
    nan_at = wave_min(nan_at);
    if constexpr (G == 256) {
        if (lane_id() == 0) { sh.f[0][wave] = M; sh.i[0][wave] = nan_at; }
        wg_barrier();
        M = fmaxf(fmaxf(sh.f[0][0], sh.f[0][1]), fmaxf(sh.f[0][2], sh.f[0][3]));
        nan_at = min(min(sh.i[0][0], sh.i[0][1]), min(sh.i[0][2], sh.i[0][3]));
    }
    float e[NV];
#pragma unroll
    for (int s = 0; s < NV; s++) e[s] = expf(v[s] - M);
    float S = wave_sum(xe_tree_sum<NV>(e));
    int cand = wave_min(m == M ? am : INT_MAX);
    cnt = wave_sum(cnt);
    if constexpr (G == 256) {
        if (lane_id() == 0) { sh.f[1][wave] = S; sh.i[1][wave] = cand; sh.i[2][wave] = cnt; }
        wg_barrier();
        S = (sh.f[1][0] + sh.f[1][1]) + (sh.f[1][2] + sh.f[1][3]);
        cand = min(min(sh.i[1][0], sh.i[1][1]), min(sh.i[1][2], sh.i[1][3]));
        cnt = (sh.i[2][0] + sh.i[2][1]) + (sh.i[2][2] + sh.i[2][3]);
    }
    const float lS = logf(S);                               // lse = M + lS; t_c = (M - z_c) + lS keeps the arg-max class's t = lS
    const bool bad = xe_bad_row(nan_at, M);
    float loss, A;
    if (y_off != 0.f) {                                     // smoothed target: every class contributes
        float a[NV];
#pragma unroll
        for (int s = 0; s < NV; s++) {
            const int c = col(s);
            const float tc = (M - v[s]) + lS;
            const float Y = c < C ? (c == y ? y_on : y_off) : 0.f;
            e[s] = Y * xe_clamp(tc);
            a[s] = xe_inside(tc) ? Y : 0.f;
        }
        loss = wave_sum(xe_tree_sum<NV>(e));
        A = wave_sum(xe_tree_sum<NV>(a));
        if constexpr (G == 256) {
            if (lane_id() == 0) { sh.f[2][wave] = loss; sh.f[3][wave] = A; }
            wg_barrier();
            loss = (sh.f[2][0] + sh.f[2][1]) + (sh.f[2][2] + sh.f[2][3]);
            A = (sh.f[3][0] + sh.f[3][1]) + (sh.f[3][2] + sh.f[3][3]);
        }
    } else {                                                // one-hot: the target class alone
        const float ty = (M - zy) + lS;
        loss = y_on * xe_clamp(ty);
        A = xe_inside(ty) ? y_on : 0.f;
    }
    if (t == 0) xe_write_row(row, B, C, bad, loss, M, lS, A, nan_at, cand, cnt, loss_i, aux, best, above);
}

// dz_k = w (A exp(-t_k) - a_k): one pass, G threads per row (64: a wave, 4 rows per workgroup; 256: a workgroup)
template <bool ZBF, bool DBF, bool VEC, int G>
__device__ __forceinline__ void xe_bwd_rows(int64_t block, const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                            const float *__restrict__ aux, const float *__restrict__ grad_loss_i, float grad_scale,
                                            int64_t B, int C, float y_on, float y_off, void *__restrict__ dz, int64_t lddz)
{
    constexpr int E = VEC ? ((ZBF || DBF) ? 8 : 4) : 1;
    const int t = threadIdx.x % G;
    const int64_t row = block * (256 / G) + threadIdx.x / G;
    if (row >= B) return;
    const void *zrow = ZBF ? (const void *)((const uint16_t *)z + row * ldz) : (const void *)((const float *)z + row * ldz);
    void *drow = DBF ? (void *)((uint16_t *)dz + row * lddz) : (void *)((float *)dz + row * lddz);
    const int y = (int)clamp_label(labels[row], C);
    const float m = aux[row], lS = aux[B + row], A = aux[2 * B + row];
    const float w = grad_loss_i ? grad_loss_i[row] : grad_scale;
    const int64_t units = ((int64_t)C + E - 1) / E;
    for (int64_t u = t; u < units; u += G) {
        const int64_t c0 = u * E;
        const bool full = E > 1 && c0 + E <= C;
        float v[E], d[E];
        xe_ld_unit<ZBF, E>(zrow, c0, C, v);
#pragma unroll
        for (int k = 0; k < E; k++) {
            const float tc = (m - v[k]) + lS;               // the forward's t_c, bit for bit
            const float Y = c0 + k == y ? y_on : y_off;
            const float a = xe_inside(tc) ? Y : 0.f;
            const float q = expf(-tc);
            d[k] = w * (A * q - a);
        }
        if constexpr (E > 1) {
            if (full) {
                xe_st_vec<DBF, E>(drow, c0, d);
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < E; k++)
            if (c0 + k < C) st_elem<DBF>(drow, c0 + k, d[k]);
    }
}

}  // namespace se
