// hxe.hip -- hierarchy-aware classifier losses on LOGITS: hierarchical cross-entropy (HXE) and cross-entropy against soft labels,
// forward + backward, with the accuracy / top-k metrics of the same scores (include/sehip.h states the arithmetic).
//
// HXE.  On a depth-first order of the class tree every ancestor of the label is one range of positions, so ONE pass over the row
// gives every level sum: per element one exponential and, per level of the label's path, one unsigned compare
// (pos[c] - lo < hi - lo) and one predicated add -- O(B C h) compares and O(B C) exponentials where dense [C, levels, C] masks
// take O(B C C h).  The label's levels are uniform per row: lane l of every wave loads level l once (at most 32 (lo, hi, w)
// triples), v_readlane hands them to the element loop as wave-uniform values, and the per-level tail (logs, weights, the suffix
// sums H_k) runs with level l on lane l.  The backward finds lev(c) by counting the ranges an element lies outside of (they are
// nested) and fetches H_lev(c) from the lane that holds it.
//
// Both losses read a row twice: statistics first (maximum, first NaN, arg-max, classes above the label: xe_scan, softmax_xent.h),
// then the sums that need the maximum; the second read hits the cache.  Paths, as in softmax_xent.hip: a 64-lane wave per row up to
// C = 1024 (4 rows per workgroup, shuffles only, no barrier), a 256-thread workgroup per row above (2 barriers); each with 16-byte
// or scalar loads.  No atomics, no workspace, no host synchronisation; every reduction is a fixed tree.
#include "softmax_xent.h"

namespace se {

constexpr int HXE_MAX = SE_HXE_MAX_LEVELS;
constexpr int HXE_AUX = HXE_MAX + 2;       // floats of aux per row: M, H_0 .. H_32
static_assert(HXE_MAX == 32, "four chunks of 8 levels; level l lives on lane l");

// E positions from class c0, -1 (in no range) past the row's end
template <int E>
__device__ __forceinline__ void hxe_ld_pos(const int32_t *__restrict__ pos, int64_t c0, int C, int *p)
{
    if constexpr (E > 1) {
        if (c0 + E <= C) {
#pragma unroll
            for (int k = 0; k < E; k += 4) {
                const int4 q = *(const int4 *)(pos + c0 + k);
                p[k] = q.x; p[k + 1] = q.y; p[k + 2] = q.z; p[k + 3] = q.w;
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < E; k++) p[k] = c0 + k < C ? pos[c0 + k] : -1;
}

// E values of a float32 table row from column c0, 0 past the row's end
template <int E>
__device__ __forceinline__ void sx_ld_q(const float *__restrict__ q, int64_t c0, int C, float *v)
{
    if constexpr (E > 1) {
        if (c0 + E <= C) {
            xe_ld_vec<false, E>(q, c0, v);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < E; k++) v[k] = c0 + k < C ? q[c0 + k] : 0.f;
}

// First read of a row by its G threads: this thread's maximum m and its column am, the row's maximum M and first NaN, this thread's
// count of classes above the label (G = 256: one barrier, slot 0 of sh)
template <bool BF16, int E, int G>
__device__ __forceinline__ void xe_stream_stats(const void *zrow, int C, float zy, int t, int wave, XeShared &sh, float &m, int &am,
                                                float &M, int &nan_at, int &cnt)
{
    m = -INFINITY;
    am = INT_MAX; nan_at = INT_MAX; cnt = 0;
    const int64_t units = ((int64_t)C + E - 1) / E;
    for (int64_t u = t; u < units; u += G) {
        float v[E];
        xe_ld_unit<BF16, E>(zrow, u * E, C, v);
#pragma unroll
        for (int k = 0; k < E; k++) xe_scan(v[k], (int)(u * E + k), zy, m, am, nan_at, cnt);
    }
    M = wave_max(m);
    nan_at = wave_min(nan_at);
    if constexpr (G == 256) {
        if (lane_id() == 0) { sh.f[0][wave] = M; sh.i[0][wave] = nan_at; }
        wg_barrier();
        M = fmaxf(fmaxf(sh.f[0][0], sh.f[0][1]), fmaxf(sh.f[0][2], sh.f[0][3]));
        nan_at = min(min(sh.i[0][0], sh.i[0][1]), min(sh.i[0][2], sh.i[0][3]));
    }
}

// The levels of label y, level l on lane l of the calling wave; lanes past h hold the range `fill` wide from 0 and weight 0.
// Indices are clamped: whatever the device tables hold, nothing is read outside lvl_*[0 .. nnz).
struct HxeLevels {
    int h, lo;
    uint32_t wd;
    float w;
};
__device__ __forceinline__ HxeLevels hxe_load_levels(const int32_t *__restrict__ path_off, const int32_t *__restrict__ lvl_lo,
                                                     const int32_t *__restrict__ lvl_hi, const float *__restrict__ lvl_w, int nnz, int y,
                                                     uint32_t fill)
{
    HxeLevels lv;
    int start = path_off[y], h = path_off[y + 1] - start;
    h = max(0, min(h, min(HXE_MAX, nnz)));
    start = max(0, min(start, nnz - h));
    lv.h = __builtin_amdgcn_readfirstlane(h);
    start = __builtin_amdgcn_readfirstlane(start);
    const int l = lane_id();
    lv.lo = 0; lv.wd = fill; lv.w = 0.f;
    if (l < lv.h) {
        const int lo = lvl_lo[start + l], hi = lvl_hi[start + l];
        lv.lo = lo;
        lv.wd = hi > lo ? (uint32_t)(hi - lo) : 0u;
        lv.w = lvl_w[start + l];
    }
    return lv;
}

// lo and width of all 32 levels as wave-uniform values
#define HXE_UNIFORM_LEVELS(lv, lo_s, wd_s)                                                    \
    int lo_s[HXE_MAX];                                                                        \
    uint32_t wd_s[HXE_MAX];                                                                   \
    _Pragma("unroll") for (int l = 0; l < HXE_MAX; l++) {                                     \
        lo_s[l] = __builtin_amdgcn_readlane(lv.lo, l);                                        \
        wd_s[l] = (uint32_t)__builtin_amdgcn_readlane((int)lv.wd, l);                         \
    }

template <bool BF16, bool VEC, int G>
__global__ __launch_bounds__(256) void hxe_fwd_kernel(const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                      const int32_t *__restrict__ pos, const int32_t *__restrict__ path_off,
                                                      const int32_t *__restrict__ lvl_lo, const int32_t *__restrict__ lvl_hi,
                                                      const float *__restrict__ lvl_w, int nnz, int64_t B, int C,
                                                      float *__restrict__ loss_i, float *__restrict__ aux, int32_t *__restrict__ best,
                                                      int32_t *__restrict__ above)
{
    constexpr int E = VEC ? (BF16 ? 8 : 4) : 1;
    const int t = threadIdx.x % G, wave = threadIdx.x >> 6, lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (row >= B) return;                                   // G = 64: the whole wave leaves (this path has no barrier); G = 256: never
    const void *zrow = BF16 ? (const void *)((const uint16_t *)z + row * ldz) : (const void *)((const float *)z + row * ldz);
    const int y = (int)clamp_label(labels[row], C);
    const float zy = ld_elem<BF16>(zrow, y);
    __shared__ XeShared sh;
    __shared__ float shS[4][HXE_MAX];

    const HxeLevels lv = hxe_load_levels(path_off, lvl_lo, lvl_hi, lvl_w, nnz, y, 0u);
    HXE_UNIFORM_LEVELS(lv, lo_s, wd_s)

    float m, M;
    int am, nan_at, cnt;
    xe_stream_stats<BF16, E, G>(zrow, C, zy, t, wave, sh, m, am, M, nan_at, cnt);

    float acc[HXE_MAX];
#pragma unroll
    for (int l = 0; l < HXE_MAX; l++) acc[l] = 0.f;
    const int64_t units = ((int64_t)C + E - 1) / E;
    for (int64_t u = t; u < units; u += G) {
        float v[E];
        int p[E];
        xe_ld_unit<BF16, E>(zrow, u * E, C, v);
        hxe_ld_pos<E>(pos, u * E, C, p);
#pragma unroll
        for (int k = 0; k < E; k++) {
            const float e = expf(v[k] - M);
#pragma unroll
            for (int j = 0; j < HXE_MAX; j += 8) {
                if (lv.h > j) {
#pragma unroll
                    for (int l = j; l < j + 8; l++) acc[l] += (uint32_t)(p[k] - lo_s[l]) < wd_s[l] ? e : 0.f;
                }
            }
        }
    }
    float Sv = 0.f;                                         // lane l: S_{l+1}
#pragma unroll
    for (int j = 0; j < HXE_MAX; j += 8) {
        if (lv.h > j) {
#pragma unroll
            for (int l = j; l < j + 8; l++) {
                const float s = wave_sum(acc[l]);
                if (lane == l) Sv = s;
            }
        }
    }
    int cand = wave_min(m == M ? am : INT_MAX);
    cnt = wave_sum(cnt);
    if constexpr (G == 256) {
        if (lane < HXE_MAX) shS[wave][lane] = Sv;
        if (lane == 0) { sh.i[1][wave] = cand; sh.i[2][wave] = cnt; }
        wg_barrier();
        Sv = lane < HXE_MAX ? (shS[0][lane] + shS[1][lane]) + (shS[2][lane] + shS[3][lane]) : 0.f;
        cand = min(min(sh.i[1][0], sh.i[1][1]), min(sh.i[1][2], sh.i[1][3]));
        cnt = (sh.i[2][0] + sh.i[2][1]) + (sh.i[2][2] + sh.i[2][3]);
    }

    // the levels' tail, level l on lane l: L_{l+1}, the weighted differences, and H_k as suffix sums of (lambda_{j-1} - lambda_j) / S_j
    const bool on = lane < lv.h;
    const float L0 = zy - M;
    const float Lme = on ? fmaxf(logf(Sv), L0) : L0;
    float Lprev = __shfl_up(Lme, 1, 64);
    if (lane == 0) Lprev = L0;
    const float loss = wave_sum(on && Lme != Lprev ? lv.w * (Lme - Lprev) : 0.f);
    const float wnext = __shfl_down(lv.w, 1, 64);           // lane h - 1 gets lambda_h = 0 (the weight of a lane past h)
    float g = on && Sv != 0.f ? (lv.w - wnext) * (1.0f / Sv) : 0.f;
#pragma unroll
    for (int off = 1; off < HXE_MAX; off *= 2) {
        const float o = __shfl_down(g, off, 64);
        if (lane + off < 64) g += o;
    }
    if (threadIdx.x % G < 64) {                             // one wave writes the row: g of lane l is H_{l+1}; H_0 = H_1
        const bool bad = xe_bad_row(nan_at, M);
        const float nan = __uint_as_float(0x7FC00000u);
        float *a = aux + row * HXE_AUX;
        if (on) a[2 + lane] = bad ? nan : g;
        if (lane == 0) {
            a[0] = bad ? nan : M;
            a[1] = bad ? nan : g;
            loss_i[row] = bad ? nan : loss;
            xe_write_metrics(row, C, bad, nan_at, cand, cnt, best, above);
        }
    }
}

template <bool ZBF, bool DBF, bool VEC, int G>
__global__ __launch_bounds__(256) void hxe_bwd_kernel(const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                      const int32_t *__restrict__ pos, const int32_t *__restrict__ path_off,
                                                      const int32_t *__restrict__ lvl_lo, const int32_t *__restrict__ lvl_hi,
                                                      const float *__restrict__ lvl_w, int nnz, const float *__restrict__ aux,
                                                      const float *__restrict__ grad_loss_i, float grad_scale, int64_t B, int C,
                                                      void *__restrict__ dz, int64_t lddz)
{
    constexpr int E = VEC ? ((ZBF || DBF) ? 8 : 4) : 1;
    const int t = threadIdx.x % G, lane = lane_id();
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (row >= B) return;
    const void *zrow = ZBF ? (const void *)((const uint16_t *)z + row * ldz) : (const void *)((const float *)z + row * ldz);
    void *drow = DBF ? (void *)((uint16_t *)dz + row * lddz) : (void *)((float *)dz + row * lddz);
    const int y = (int)clamp_label(labels[row], C);
    const float w = grad_loss_i ? grad_loss_i[row] : grad_scale;

    const HxeLevels lv = hxe_load_levels(path_off, lvl_lo, lvl_hi, lvl_w, nnz, y, 0xFFFFFFFFu);   // past h: a range nothing lies outside of
    HXE_UNIFORM_LEVELS(lv, lo_s, wd_s)
    const float *a = aux + row * HXE_AUX;
    const float M = a[0];
    const float Hl = lane <= lv.h ? a[1 + lane] : 0.f;      // lane k: H_k
    const float lam0 = __shfl(lv.w, 0, 64);

    // every lane takes every trip (the H look-up reads other lanes); a unit past the row's end loads and stores nothing
    const int64_t units = ((int64_t)C + E - 1) / E;
    for (int64_t u0 = 0; u0 < units; u0 += G) {
        const int64_t c0 = (u0 + t) * E;
        float v[E], d[E];
        int p[E];
        xe_ld_unit<ZBF, E>(zrow, c0, C, v);
        hxe_ld_pos<E>(pos, c0, C, p);
#pragma unroll
        for (int k = 0; k < E; k++) {
            int out = 0;
#pragma unroll
            for (int j = 0; j < HXE_MAX; j += 8) {
                if (lv.h > j) {
#pragma unroll
                    for (int l = j; l < j + 8; l++) out += (uint32_t)(p[k] - lo_s[l]) < wd_s[l] ? 0 : 1;
                }
            }
            const bool label = c0 + k == y;
            const float H = __shfl(Hl, label ? 0 : 1 + out, 64);       // lev(c): the ranges are nested
            d[k] = w * (expf(v[k] - M) * H - (label ? lam0 : 0.f));
        }
        if constexpr (E > 1) {
            if (c0 + E <= C) {
                xe_st_vec<DBF, E>(drow, c0, d);
                continue;
            }
        }
#pragma unroll
        for (int k = 0; k < E; k++)
            if (c0 + k < C) st_elem<DBF>(drow, c0 + k, d[k]);
    }
}

template <bool BF16, bool VEC, int G>
__global__ __launch_bounds__(256) void soft_xent_fwd_kernel(const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                            const float *__restrict__ table, int64_t ldt, int64_t B, int C,
                                                            float *__restrict__ loss_i, float *__restrict__ aux,
                                                            int32_t *__restrict__ best, int32_t *__restrict__ above)
{
    constexpr int E = VEC ? (BF16 ? 8 : 4) : 1;
    const int t = threadIdx.x % G, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (row >= B) return;
    const void *zrow = BF16 ? (const void *)((const uint16_t *)z + row * ldz) : (const void *)((const float *)z + row * ldz);
    const int y = (int)clamp_label(labels[row], C);
    const float zy = ld_elem<BF16>(zrow, y);
    const float *qrow = table + (int64_t)y * ldt;
    __shared__ XeShared sh;

    float m, M;
    int am, nan_at, cnt;
    xe_stream_stats<BF16, E, G>(zrow, C, zy, t, wave, sh, m, am, M, nan_at, cnt);

    float se[E], sa[E], sq[E];
#pragma unroll
    for (int k = 0; k < E; k++) se[k] = sa[k] = sq[k] = 0.f;
    const int64_t units = ((int64_t)C + E - 1) / E;
    for (int64_t u = t; u < units; u += G) {
        float v[E], q[E];
        xe_ld_unit<BF16, E>(zrow, u * E, C, v);
        sx_ld_q<E>(qrow, u * E, C, q);
#pragma unroll
        for (int k = 0; k < E; k++) {
            se[k] += expf(v[k] - M);
            sa[k] += q[k] != 0.f ? q[k] * (M - v[k]) : 0.f;
            sq[k] += q[k];
        }
    }
    float S = wave_sum(xe_tree_sum<E>(se)), A = wave_sum(xe_tree_sum<E>(sa)), Q = wave_sum(xe_tree_sum<E>(sq));
    int cand = wave_min(m == M ? am : INT_MAX);
    cnt = wave_sum(cnt);
    if constexpr (G == 256) {
        if (lane_id() == 0) { sh.f[1][wave] = S; sh.f[2][wave] = A; sh.f[3][wave] = Q; sh.i[1][wave] = cand; sh.i[2][wave] = cnt; }
        wg_barrier();
        S = (sh.f[1][0] + sh.f[1][1]) + (sh.f[1][2] + sh.f[1][3]);
        A = (sh.f[2][0] + sh.f[2][1]) + (sh.f[2][2] + sh.f[2][3]);
        Q = (sh.f[3][0] + sh.f[3][1]) + (sh.f[3][2] + sh.f[3][3]);
        cand = min(min(sh.i[1][0], sh.i[1][1]), min(sh.i[1][2], sh.i[1][3]));
        cnt = (sh.i[2][0] + sh.i[2][1]) + (sh.i[2][2] + sh.i[2][3]);
    }
    const float lS = logf(S);
    if (t == 0) xe_write_row(row, B, C, xe_bad_row(nan_at, M), A + Q * lS, M, lS, Q, nan_at, cand, cnt, loss_i, aux, best, above);
}

template <bool ZBF, bool DBF, bool VEC, int G>
__global__ __launch_bounds__(256) void soft_xent_bwd_kernel(const void *__restrict__ z, int64_t ldz, const int64_t *__restrict__ labels,
                                                            const float *__restrict__ table, int64_t ldt, const float *__restrict__ aux,
                                                            const float *__restrict__ grad_loss_i, float grad_scale, int64_t B, int C,
                                                            void *__restrict__ dz, int64_t lddz)
{
    constexpr int E = VEC ? ((ZBF || DBF) ? 8 : 4) : 1;
    const int t = threadIdx.x % G;
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (row >= B) return;
    const void *zrow = ZBF ? (const void *)((const uint16_t *)z + row * ldz) : (const void *)((const float *)z + row * ldz);
    void *drow = DBF ? (void *)((uint16_t *)dz + row * lddz) : (void *)((float *)dz + row * lddz);
    const int y = (int)clamp_label(labels[row], C);
    const float *qrow = table + (int64_t)y * ldt;
    const float M = aux[row], lS = aux[B + row], Q = aux[2 * B + row];
    const float w = grad_loss_i ? grad_loss_i[row] : grad_scale;
    const int64_t units = ((int64_t)C + E - 1) / E;
    for (int64_t u = t; u < units; u += G) {
        const int64_t c0 = u * E;
        float v[E], q[E], d[E];
        xe_ld_unit<ZBF, E>(zrow, c0, C, v);
        sx_ld_q<E>(qrow, c0, C, q);
#pragma unroll
        for (int k = 0; k < E; k++) d[k] = w * (Q * expf(-((M - v[k]) + lS)) - q[k]);
        if constexpr (E > 1) {
            if (c0 + E <= C) {
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

using namespace se;

static int hl_check(const char *who, const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, int64_t B, int64_t C,
                    const float *aux)
{
    if (B < 0 || C < 1) return fail(SE_ERR_INVALID, "%s: bad shape B=%lld C=%lld", who, (long long)B, (long long)C);
    if (!is_float_dtype(z_dtype)) return fail(SE_ERR_INVALID, "%s: bad dtype %d", who, z_dtype);
    if (ldz < C) return fail(SE_ERR_INVALID, "%s: leading dimension %lld < C=%lld", who, (long long)ldz, (long long)C);
    if (C > INT_MAX - 16 || B > INT_MAX) return fail(SE_ERR_UNSUPPORTED, "%s: B or C too large", who);
    if (B > 0 && (!logits || !labels || !aux)) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    return SE_OK;
}

static int hl_check_dz(const char *who, const void *dz, int dz_dtype, int64_t lddz, int64_t B, int64_t C)
{
    if (!is_float_dtype(dz_dtype)) return fail(SE_ERR_INVALID, "%s: bad dtype %d", who, dz_dtype);
    if (lddz < C) return fail(SE_ERR_INVALID, "%s: leading dimension %lld < C=%lld", who, (long long)lddz, (long long)C);
    if (B > 0 && !dz) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    return SE_OK;
}

// the encoding's pointers, and the host copy of path_off: starts at 0, every path 0 .. SE_HXE_MAX_LEVELS levels; nnz = its last entry
static int hxe_check_paths(const char *who, const int32_t *pos, const int32_t *path_off, const int32_t *path_off_host,
                           const int32_t *lvl_lo, const int32_t *lvl_hi, const float *lvl_w, int64_t B, int64_t C, int &nnz)
{
    nnz = 0;
    if (!path_off_host) return B > 0 ? fail(SE_ERR_INVALID, "%s: null pointer", who) : SE_OK;
    if (path_off_host[0] != 0) return fail(SE_ERR_INVALID, "%s: path_off[0] = %d, not 0", who, (int)path_off_host[0]);
    for (int64_t c = 0; c < C; c++) {
        const int64_t h = (int64_t)path_off_host[c + 1] - path_off_host[c];
        if (h < 0) return fail(SE_ERR_INVALID, "%s: path_off decreases at class %lld", who, (long long)c);
        if (h > HXE_MAX)
            return fail(SE_ERR_INVALID, "%s: class %lld has %lld levels, more than SE_HXE_MAX_LEVELS = %d", who, (long long)c, (long long)h,
                        HXE_MAX);
    }
    nnz = path_off_host[C];
    if (B > 0 && (!pos || !path_off || (nnz > 0 && (!lvl_lo || !lvl_hi || !lvl_w)))) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    return SE_OK;
}

extern "C" int64_t se_hxe_aux_floats(int64_t B) { return B > 0 ? (int64_t)HXE_AUX * B : 0; }

extern "C" int se_hxe_fwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const int32_t *pos,
                          const int32_t *path_off, const int32_t *path_off_host, const int32_t *lvl_lo, const int32_t *lvl_hi,
                          const float *lvl_w, int64_t B, int64_t C, float *loss_i, float *aux, int32_t *best, int32_t *above,
                          float *loss_mean, se_stream_t stream)
{
    const char *who = "se_hxe_fwd";
    int rc = hl_check(who, logits, z_dtype, ldz, labels, B, C, aux), nnz;
    if (rc != SE_OK) return rc;
    if (B > 0 && !loss_i) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    rc = hxe_check_paths(who, pos, path_off, path_off_host, lvl_lo, lvl_hi, lvl_w, B, C, nnz);
    if (rc != SE_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (B > 0) {
        const bool bf = z_dtype == SE_DTYPE_BF16;
        const bool vec = aligned16(logits, ldz, bf ? 2 : 4) && aligned16(pos);
        dispatch_bools(bf, vec, [&](auto BF, auto VEC) {
            if (C <= XE_WAVE_MAX_C)
                hipLaunchKernelGGL((hxe_fwd_kernel<BF(), VEC(), 64>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits, ldz, labels, pos,
                                   path_off, lvl_lo, lvl_hi, lvl_w, nnz, B, (int)C, loss_i, aux, best, above);
            else
                hipLaunchKernelGGL((hxe_fwd_kernel<BF(), VEC(), 256>), dim3((unsigned)B), dim3(256), 0, s, logits, ldz, labels, pos, path_off,
                                   lvl_lo, lvl_hi, lvl_w, nnz, B, (int)C, loss_i, aux, best, above);
        });
        SE_LAUNCH_CHECK();
    }
    if (loss_mean) {
        launch_mean(loss_i, B, loss_mean, s);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}

extern "C" int se_hxe_bwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const int32_t *pos,
                          const int32_t *path_off, const int32_t *path_off_host, const int32_t *lvl_lo, const int32_t *lvl_hi,
                          const float *lvl_w, const float *aux, const float *grad_loss_i, float grad_scale, int64_t B, int64_t C,
                          void *dz, int dz_dtype, int64_t lddz, se_stream_t stream)
{
    const char *who = "se_hxe_bwd";
    int rc = hl_check(who, logits, z_dtype, ldz, labels, B, C, aux), nnz;
    if (rc != SE_OK) return rc;
    rc = hl_check_dz(who, dz, dz_dtype, lddz, B, C);
    if (rc != SE_OK) return rc;
    rc = hxe_check_paths(who, pos, path_off, path_off_host, lvl_lo, lvl_hi, lvl_w, B, C, nnz);
    if (rc != SE_OK) return rc;
    if (B == 0) return SE_OK;
    const bool zbf = z_dtype == SE_DTYPE_BF16, dbf = dz_dtype == SE_DTYPE_BF16;
    const bool vec = aligned16(logits, ldz, zbf ? 2 : 4) && aligned16(dz, lddz, dbf ? 2 : 4) && aligned16(pos);
    hipStream_t s = (hipStream_t)stream;
    dispatch_bools(zbf, dbf, vec, [&](auto ZBF, auto DBF, auto VEC) {
        if (C <= XE_WAVE_MAX_C)
            hipLaunchKernelGGL((hxe_bwd_kernel<ZBF(), DBF(), VEC(), 64>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits, ldz, labels,
                               pos, path_off, lvl_lo, lvl_hi, lvl_w, nnz, aux, grad_loss_i, grad_scale, B, (int)C, dz, lddz);
        else
            hipLaunchKernelGGL((hxe_bwd_kernel<ZBF(), DBF(), VEC(), 256>), dim3((unsigned)B), dim3(256), 0, s, logits, ldz, labels, pos,
                               path_off, lvl_lo, lvl_hi, lvl_w, nnz, aux, grad_loss_i, grad_scale, B, (int)C, dz, lddz);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}

static int sx_check_table(const char *who, const float *table, int64_t ldt, int64_t B, int64_t C)
{
    if (ldt < C) return fail(SE_ERR_INVALID, "%s: table leading dimension %lld < C=%lld", who, (long long)ldt, (long long)C);
    if (B > 0 && !table) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    return SE_OK;
}

extern "C" int se_soft_xent_fwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const float *table, int64_t ldt,
                                int64_t B, int64_t C, float *loss_i, float *aux, int32_t *best, int32_t *above, float *loss_mean,
                                se_stream_t stream)
{
    const char *who = "se_soft_xent_fwd";
    int rc = hl_check(who, logits, z_dtype, ldz, labels, B, C, aux);
    if (rc != SE_OK) return rc;
    if (B > 0 && !loss_i) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    rc = sx_check_table(who, table, ldt, B, C);
    if (rc != SE_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (B > 0) {
        const bool bf = z_dtype == SE_DTYPE_BF16;
        const bool vec = aligned16(logits, ldz, bf ? 2 : 4) && aligned16(table, ldt, 4);
        dispatch_bools(bf, vec, [&](auto BF, auto VEC) {
            if (C <= XE_WAVE_MAX_C)
                hipLaunchKernelGGL((soft_xent_fwd_kernel<BF(), VEC(), 64>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits, ldz, labels,
                                   table, ldt, B, (int)C, loss_i, aux, best, above);
            else
                hipLaunchKernelGGL((soft_xent_fwd_kernel<BF(), VEC(), 256>), dim3((unsigned)B), dim3(256), 0, s, logits, ldz, labels, table, ldt,
                                   B, (int)C, loss_i, aux, best, above);
        });
        SE_LAUNCH_CHECK();
    }
    if (loss_mean) {
        launch_mean(loss_i, B, loss_mean, s);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}

extern "C" int se_soft_xent_bwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const float *table, int64_t ldt,
                                const float *aux, const float *grad_loss_i, float grad_scale, int64_t B, int64_t C, void *dz,
                                int dz_dtype, int64_t lddz, se_stream_t stream)
{
    const char *who = "se_soft_xent_bwd";
    int rc = hl_check(who, logits, z_dtype, ldz, labels, B, C, aux);
    if (rc != SE_OK) return rc;
    rc = hl_check_dz(who, dz, dz_dtype, lddz, B, C);
    if (rc != SE_OK) return rc;
    rc = sx_check_table(who, table, ldt, B, C);
    if (rc != SE_OK) return rc;
    if (B == 0) return SE_OK;
    const bool zbf = z_dtype == SE_DTYPE_BF16, dbf = dz_dtype == SE_DTYPE_BF16;
    const bool vec = aligned16(logits, ldz, zbf ? 2 : 4) && aligned16(dz, lddz, dbf ? 2 : 4) && aligned16(table, ldt, 4);
    hipStream_t s = (hipStream_t)stream;
    dispatch_bools(zbf, dbf, vec, [&](auto ZBF, auto DBF, auto VEC) {
        if (C <= XE_WAVE_MAX_C)
            hipLaunchKernelGGL((soft_xent_bwd_kernel<ZBF(), DBF(), VEC(), 64>), dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits, ldz,
                               labels, table, ldt, aux, grad_loss_i, grad_scale, B, (int)C, dz, lddz);
        else
            hipLaunchKernelGGL((soft_xent_bwd_kernel<ZBF(), DBF(), VEC(), 256>), dim3((unsigned)B), dim3(256), 0, s, logits, ldz, labels, table,
                               ldt, aux, grad_loss_i, grad_scale, B, (int)C, dz, lddz);
    });
    SE_LAUNCH_CHECK();
    return SE_OK;
}
