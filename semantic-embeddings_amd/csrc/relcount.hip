// relcount.hip -- positions of the relevant items of a query in a gallery it is NOT ranked against in full: by counting.
//
// Replaces, for a gallery that is not the query set, the `se_rank_rows` + `se_relevant_positions` pair behind AP, mAP and the
// recall-precision curve (plot_recall_precision.py:52-79, class_hierarchy.py:310-314): the 1-based position of a relevant item in
// the canonical ranking is the number of gallery columns that precede it, plus one -- a counting pass over distance slabs instead
// of an N-wide sort per query.  Two steps:
//
// * relcount_kernel (se_count_preceding): one 256-thread workgroup per (query, chunk of columns).  The query's relevant keys --
//   sorted ascending by the caller, (canon_key(distance) << 32 | global index): the total order of rank_rows.hip, NaN last,
//   -0 == +0, ties by index -- are staged in LDS next to an integer histogram with one bin per key.  The threads stride over the
//   chunk's distances (16-byte loads when the slab allows), build each column's key, find by binary search the number p of
//   relevant keys strictly before it and count the column in bin p; columns behind the last relevant key (p == R) are dropped.
//   The histogram is flushed with integer global adds: they commute, so the counts do not depend on the launch geometry, the
//   tiling of the gallery or the order in which shards are counted.  A key list that does not fit the LDS is searched in global
//   memory and counted with global adds directly.
// * relscan_kernel (se_count_to_positions): inclusive prefix sum of every query's bins.  Every column -- the relevant ones land in
//   their own bins -- was counted, so the sum up to bin s is the position of the (s + 1)-th relevant item.
#include "se_common.h"

#include <limits.h>

namespace se {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / WAVE;
constexpr int RC_VEC = 4;                          // consecutive columns per thread and step (one 16-byte load)
constexpr int RC_CHUNK = 16384;                    // columns of a workgroup: 16 steps
constexpr int RC_LDS_MAX = 64 * 1024;              // dynamic LDS a workgroup may own without a function attribute
constexpr int RC_KEY_BYTES = 12;                   // per relevant item: 8 bytes of key + 4 of histogram
constexpr int RC_MAX_KEYS = RC_LDS_MAX / RC_KEY_BYTES / 2 * 2;

__device__ __forceinline__ uint64_t rc_key(float d, int32_t idx) { return ((uint64_t)canon_key(d) << 32) | (uint32_t)idx; }

// number of keys[0 .. R) strictly below k (keys ascending); KEYS: m -> key m
template <class KEYS>
__device__ __forceinline__ int rc_lower_bound(KEYS keys, int R, uint64_t k)
{
    int lo = 0, len = R;
    while (len > 0) {
        const int half = len >> 1;
        if (keys(lo + half) < k) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo;
}

// cols: columns per workgroup (a multiple of RC_VEC); lds_keys: keys the dynamic LDS holds
__global__ __launch_bounds__(RC_THREADS) void relcount_kernel(const float *__restrict__ pdist, int64_t ldp, int64_t n_cols, int64_t col_offset,
                                                              const int64_t *__restrict__ hit_off, const float *__restrict__ rel_d,
                                                              const int32_t *__restrict__ rel_i, const int32_t *__restrict__ qidx,
                                                              int32_t *__restrict__ cnt, int64_t cols, int64_t nchunks, int lds_keys, int vec_ok)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_raw[];
    uint64_t *s_key = reinterpret_cast<uint64_t *>(rc_raw);
    int *s_hist = reinterpret_cast<int *>(rc_raw + (size_t)lds_keys * sizeof(uint64_t));
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
    const int64_t off = hit_off[i];
    const int64_t Rl = hit_off[i + 1] - off;
    if (Rl <= 0) return;                                              // uniform: nothing relevant, the row's bins do not exist
    const int R = (int)(Rl > INT_MAX ? INT_MAX : Rl);
    const bool in_lds = R <= lds_keys;                                // uniform
    const float *kd = rel_d + off;
    const int32_t *ki = rel_i + off;
    int32_t *bins = cnt + off;
    if (in_lds) {
        for (int m = tid; m < R; m += RC_THREADS) { s_key[m] = rc_key(kd[m], ki[m]); s_hist[m] = 0; }
        wg_barrier();
    }
    const int64_t self = qidx ? (int64_t)qidx[i] : -1;                // global index of the query's own gallery row; negative: absent
    const float *row = pdist + i * ldp;
    const int64_t c0 = chunk * cols, c1 = (c0 + cols < n_cols) ? c0 + cols : n_cols;
    auto count = [&](float d, int64_t j) {
        const int64_t g = col_offset + j;
        if (g == self) return;
        const uint64_t k = rc_key(d, (int32_t)g);
        if (in_lds) {
            const int p = rc_lower_bound([&](int m) { return s_key[m]; }, R, k);
            if (p < R) atomicAdd(&s_hist[p], 1);
        } else {
            const int p = rc_lower_bound([&](int m) { return rc_key(kd[m], ki[m]); }, R, k);
            if (p < R) atomicAdd(&bins[p], 1);
        }
    };
    for (int64_t j = c0 + (int64_t)tid * RC_VEC; j < c1; j += RC_THREADS * RC_VEC) {
        if (vec_ok && j + RC_VEC <= c1) {
            const float4 v = *reinterpret_cast<const float4 *>(row + j);
            count(v.x, j); count(v.y, j + 1); count(v.z, j + 2); count(v.w, j + 3);
        } else {
            for (int e = 0; e < RC_VEC && j + e < c1; e++) count(row[j + e], j + e);
        }
    }
    if (in_lds) {
        wg_barrier();
        for (int m = tid; m < R; m += RC_THREADS) {
            const int v = s_hist[m];
            if (v) atomicAdd(&bins[m], v);
        }
    }
}

// inclusive prefix sum of every query's bins; one workgroup per query at a time, RC_THREADS bins per step
__global__ __launch_bounds__(RC_THREADS) void relscan_kernel(const int32_t *__restrict__ cnt, const int64_t *__restrict__ hit_off, int64_t Q,
                                                             int32_t *__restrict__ hit_pos)
{
    __shared__ int s_tot[2][RC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int par = 0;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const int64_t off = hit_off[q];
        const int64_t R = hit_off[q + 1] - off;
        int carry = 0;                                                // sum of the steps before this one (the same in every thread)
        for (int64_t base = 0; base < R; base += RC_THREADS) {        // uniform trip count
            const int64_t m = base + tid;
            const int v = wave_incl_scan(m < R ? cnt[off + m] : 0);
            if (lane == WAVE - 1) s_tot[par][wave] = v;
            wg_barrier();   // the only barrier of a step: the other half of s_tot is written next time
            int before = carry, total = 0;
#pragma unroll
            for (int w = 0; w < RC_WAVES; w++) {
                const int t = s_tot[par][w];
                if (w < wave) before += t;
                total += t;
            }
            if (m < R) hit_pos[off + m] = before + v;
            carry += total;
            par ^= 1;
        }
    }
}

}  // namespace se

using namespace se;

extern "C" int se_count_preceding(const float *pdist, int64_t ldp, int64_t q, int64_t n_cols, int64_t col_offset, const int64_t *hit_off,
                                  const float *rel_d, const int32_t *rel_i, const int32_t *qidx, int64_t max_rel, int32_t *cnt,
                                  se_stream_t stream)
{
    if (q < 0 || n_cols < 0 || q > 0x7FFFFFFF || col_offset < 0 || col_offset + n_cols > 0x7FFFFFFF)
        return fail(SE_ERR_INVALID, "se_count_preceding: bad shape q=%lld n_cols=%lld col_offset=%lld", (long long)q, (long long)n_cols,
                    (long long)col_offset);
    if (q == 0 || n_cols == 0) return SE_OK;
    if (!pdist || !hit_off || !rel_d || !rel_i || !cnt) return fail(SE_ERR_INVALID, "se_count_preceding: null pointer");
    if (ldp < n_cols) return fail(SE_ERR_INVALID, "se_count_preceding: leading dimension too small");
    // LDS for the longest key list the caller announces (unknown: all a workgroup may own); longer lists are searched in global memory
    int64_t keys = (max_rel <= 0 || max_rel > RC_MAX_KEYS) ? RC_MAX_KEYS : (max_rel + 1) / 2 * 2;
    int64_t cols = RC_CHUNK;
    while (q * ((n_cols + cols - 1) / cols) > 0x40000000) cols *= 2;  // a one-dimensional grid
    const int64_t nchunks = (n_cols + cols - 1) / cols;
    const int vec_ok = aligned16(pdist, ldp, (int)sizeof(float)) ? 1 : 0;
    hipLaunchKernelGGL(relcount_kernel, dim3((unsigned)(q * nchunks)), dim3(RC_THREADS), (size_t)keys * RC_KEY_BYTES, (hipStream_t)stream, pdist,
                       ldp, n_cols, col_offset, hit_off, rel_d, rel_i, qidx, cnt, cols, nchunks, (int)keys, vec_ok);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_count_to_positions(const int32_t *cnt, const int64_t *hit_off, int64_t q, int32_t *hit_pos, se_stream_t stream)
{
    if (q < 0 || q > 0x7FFFFFFF) return fail(SE_ERR_INVALID, "se_count_to_positions: bad shape q=%lld", (long long)q);
    if (q == 0) return SE_OK;
    if (!cnt || !hit_off || !hit_pos) return fail(SE_ERR_INVALID, "se_count_to_positions: null pointer");
    hipLaunchKernelGGL(relscan_kernel, dim3((unsigned)(q < 65536 ? q : 65536)), dim3(RC_THREADS), 0, (hipStream_t)stream, cnt, hit_off, q, hit_pos);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
