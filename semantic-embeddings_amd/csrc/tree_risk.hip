// tree_risk.hip -- conditional risk minimisation (CRM) on a class TREE: for every row of class probabilities the expected height of
// the lowest common subsumer, risk_k = sum_j p_j * height(lcs(k, j)), of every class k, and the `top` classes of smallest risk
// (include/sehip.h states the arithmetic).
//
// The dense form is P @ H^T with the [C, C] height table, O(C^2) per row.  On the depth-first class order of
// ClassHierarchy.hxe_encoding every ancestor of k is one range of positions (hxe.hip rests on the same fact), and the classes whose
// lcs with k is the level-l ancestor are that ancestor's range minus the range below it.  So ONE float64 prefix sum of the row in
// depth-first order gives the mass of every range as a difference of two entries, and a risk costs two LDS look-ups per level of
// k's path: O(C * levels) per row, the row read once from memory.
//
// Per row, by a group of G threads (a 64-lane wave up to C = 1024, four rows per workgroup; the 256 threads of a workgroup above):
//   1. the row is scattered into depth-first order in LDS (float64), non-finite values are noticed on the way;
//   2. inclusive float64 scan: every wave scans a contiguous span in tiles of 64 (DPP scan + running carry), the spans' totals are
//      added on in wave order -- the order of the sums is a function of C alone;
//   3. every thread walks the levels of its classes k = t, t + G, ... and leaves risk_k in a second LDS row;
//   4. `top` rounds of a (risk, class) arg-min over per-thread candidates; the winner's thread rescans its own classes.
// Both LDS rows hold C float64 values: 16 C bytes per row in flight, which bounds C (SE_TREE_RISK_MAX_CLASSES).  No atomics, no
// workspace, no host synchronisation.  Every wave of a workgroup takes every barrier (rows past the end are computed on the last row
// and store nothing).
#include <limits.h>

#include "se_common.h"

namespace se {

constexpr int TR_WAVE_MAX_C = 1024;                    // a wave per row up to here, a workgroup per row above
constexpr int TR_LEVELS = SE_HXE_MAX_LEVELS;
static_assert(SE_TREE_RISK_MAX_CLASSES * 16 + 1024 <= 160 * 1024, "two float64 rows and the exchange slots fit the 160 KiB LDS");
static_assert(TR_WAVE_MAX_C * 16 * 4 + 1024 <= 160 * 1024, "four rows of the wave path fit as well");

// (a, ia) strictly before (b, ib) in ascending (risk, class) order: numbers by value (-0 == +0), NaN behind every number
__device__ __forceinline__ bool tr_before(double a, int ia, double b, int ib)
{
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? ia < ib : bn;
    return a < b || (a == b && ia < ib);
}

// the first of this thread's classes t, t + G, ... in (risk, class) order; a taken class holds NaN.  None left: (NaN, INT_MAX)
template <int G>
__device__ __forceinline__ void tr_local_best(const double *R, int C, int t, double &v, int &idx)
{
    v = __longlong_as_double(0x7FF8000000000000ll);
    idx = INT_MAX;
    for (int k = t; k < C; k += G) {
        const double r = R[k];
        if (r == r && tr_before(r, k, v, idx)) { v = r; idx = k; }
    }
}

template <int G>
__global__ __launch_bounds__(256) void tree_risk_kernel(const float *__restrict__ probs, int64_t ldp, const int32_t *__restrict__ pos,
                                                        const int32_t *__restrict__ path_off, const int32_t *__restrict__ lvl_lo,
                                                        const int32_t *__restrict__ lvl_hi, const int32_t *__restrict__ lvl_h, int nnz,
                                                        const int32_t *__restrict__ own_h, int64_t N, int C, int top,
                                                        int32_t *__restrict__ out_cls, double *__restrict__ out_risk,
                                                        double *__restrict__ risk, int64_t ldr)
{
    constexpr int NW = G / 64, ROWS = 256 / G;              // waves per row, rows per workgroup
    extern __shared__ double tr_lds[];
    __shared__ double sh_tot[4];                            // G = 256: the scan totals of the four spans
    __shared__ double sh_v[2][4];                           // G = 256: the waves' candidates of a round (two rounds in flight)
    __shared__ int sh_i[2][4];
    __shared__ int sh_bad[4];

    const int t = threadIdx.x % G, slot = threadIdx.x / G, wave = threadIdx.x >> 6, lane = lane_id();
    const int64_t row_raw = (int64_t)blockIdx.x * ROWS + slot;
    const bool live = row_raw < N;                          // a slot past the last row recomputes it and stores nothing
    const int64_t row = live ? row_raw : N - 1;
    const float *__restrict__ prow = probs + row * ldp;
    double *S = tr_lds + (size_t)slot * 2 * C, *R = S + C;  // S: the row in depth-first order, then its inclusive prefix sums

    // 1. zero (a pos table that is no permutation leaves no slot unwritten), then scatter
    for (int k = t; k < C; k += G) S[k] = 0.0;
    wg_barrier();
    bool bad = false;
    for (int k = t; k < C; k += G) {
        const float p = prow[k];
        bad |= !(fabsf(p) <= 3.402823466e+38f);             // NaN or an infinity
        S[min(max(pos[k], 0), C - 1)] = (double)p;
    }
    bad = __any(bad);
    if constexpr (NW > 1) {
        if (lane == 0) sh_bad[wave] = bad;
    }
    wg_barrier();
    if constexpr (NW > 1) bad = (sh_bad[0] | sh_bad[1] | sh_bad[2] | sh_bad[3]) != 0;

    // 2. inclusive scan: wave w of the row owns positions [w * span, (w + 1) * span)
    {
        const int w = NW > 1 ? wave : 0;
        const int span = 64 * ((C + 64 * NW - 1) / (64 * NW));
        const int end = min(C, (w + 1) * span);
        double carry = 0.0;
        for (int i0 = w * span; i0 < end; i0 += 64) {
            const int i = i0 + lane;
            const double v = carry + wave_incl_scan(i < C ? S[i] : 0.0);
            if (i < end) S[i] = v;
            carry = __shfl(v, 63, 64);
        }
        if constexpr (NW > 1) {
            if (lane == 0) sh_tot[wave] = carry;
            wg_barrier();
            if (w > 0) {
                double off = sh_tot[0];
                for (int j = 1; j < w; j++) off += sh_tot[j];
                for (int i = w * span + lane; i < end; i += 64) S[i] = off + S[i];
            }
        }
    }
    wg_barrier();

    // 3. the risks of this thread's classes
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int k = t; k < C; k += G) {
        int start = path_off[k], h = path_off[k + 1] - start;
        h = max(0, min(h, min(TR_LEVELS, nnz)));
        start = max(0, min(start, nnz - h));
        const double pk = (double)prow[k];
        double r = (double)(own_h ? own_h[k] : 0) * pk, below = pk;
        for (int l = 0; l < h; l++) {
            const int lo = min(max(lvl_lo[start + l], 0), C), hi = min(max(lvl_hi[start + l], 0), C);
            const double m = hi > lo ? S[hi - 1] - (lo > 0 ? S[lo - 1] : 0.0) : 0.0;
            r += (double)lvl_h[start + l] * (m - below);
            below = m;
        }
        if (bad) r = nan;
        R[k] = r;
        if (risk && live) risk[row * ldr + k] = r;
    }
    wg_barrier();

    // 4. the `top` first classes in (risk, class) order
    double v;
    int idx;
    tr_local_best<G>(R, C, t, v, idx);
    for (int round = 0; round < top; round++) {
        double bv = v;
        int bi = idx;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (tr_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if constexpr (NW > 1) {
            const int par = round & 1;
            if (lane == 0) { sh_v[par][wave] = bv; sh_i[par][wave] = bi; }
            wg_barrier();
            bv = sh_v[par][0]; bi = sh_i[par][0];
#pragma unroll
            for (int j = 1; j < 4; j++) {
                const double ov = sh_v[par][j];
                const int oi = sh_i[par][j];
                if (tr_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
        }
        if (t == 0 && live) {
            out_cls[row * top + round] = bad ? round : bi;
            out_risk[row * top + round] = bad ? nan : bv;
        }
        if (bi == idx && idx < C) {                         // the winner's thread takes it out and looks for its next one
            R[idx] = nan;
            tr_local_best<G>(R, C, t, v, idx);
        }
    }
}

}  // namespace se

using namespace se;

extern "C" int se_tree_risk_topk(const float *probs, int64_t ldp, const int32_t *pos, const int32_t *path_off, const int32_t *lvl_lo,
                                 const int32_t *lvl_hi, const int32_t *lvl_h, int nnz, const int32_t *own_h, int64_t N, int C, int top,
                                 int32_t *out_cls, double *out_risk, double *risk, int64_t ldr, se_stream_t stream)
{
    const char *who = "se_tree_risk_topk";
    if (N < 0 || C < 1 || nnz < 0) return fail(SE_ERR_INVALID, "%s: bad shape N=%lld C=%d nnz=%d", who, (long long)N, C, nnz);
    if (top < 1 || top > C || top > SE_TREE_RISK_TOP_MAX)
        return fail(SE_ERR_INVALID, "%s: top=%d outside [1, min(C=%d, %d)]", who, top, C, SE_TREE_RISK_TOP_MAX);
    if (ldp < C) return fail(SE_ERR_INVALID, "%s: leading dimension %lld < C=%d", who, (long long)ldp, C);
    if (risk && ldr < C) return fail(SE_ERR_INVALID, "%s: risk leading dimension %lld < C=%d", who, (long long)ldr, C);
    if (C > SE_TREE_RISK_MAX_CLASSES)
        return fail(SE_ERR_UNSUPPORTED, "%s: C=%d exceeds SE_TREE_RISK_MAX_CLASSES = %d", who, C, SE_TREE_RISK_MAX_CLASSES);
    if (N > INT_MAX) return fail(SE_ERR_UNSUPPORTED, "%s: N too large", who);
    if (!probs || !pos || !path_off || !out_cls || !out_risk || (nnz > 0 && (!lvl_lo || !lvl_hi || !lvl_h)))
        return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (N == 0) return SE_OK;
    hipStream_t s = (hipStream_t)stream;
    if (C <= TR_WAVE_MAX_C) {
        const size_t lds = (size_t)4 * 2 * C * sizeof(double);
        SE_HIP_CHECK(hipFuncSetAttribute((const void *)tree_risk_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(tree_risk_kernel<64>, dim3((unsigned)((N + 3) / 4)), dim3(256), lds, s, probs, ldp, pos, path_off, lvl_lo, lvl_hi,
                           lvl_h, nnz, own_h, N, C, top, out_cls, out_risk, risk, ldr);
    } else {
        const size_t lds = (size_t)2 * C * sizeof(double);
        SE_HIP_CHECK(hipFuncSetAttribute((const void *)tree_risk_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(tree_risk_kernel<256>, dim3((unsigned)N), dim3(256), lds, s, probs, ldp, pos, path_off, lvl_lo, lvl_hi, lvl_h,
                           nnz, own_h, N, C, top, out_cls, out_risk, risk, ldr);
    }
    SE_LAUNCH_CHECK();
    return SE_OK;
}
