// pdist_f64.hip -- float64 all-pairs distances (se_pairwise_dist_f64): the opt-in path for float64 feature files, where the
// reference ranks float64 distances (evaluate_retrieval.py:57-67 works in the caller's dtype).
//
// Canonical arithmetic (include/sehip.h): C[i, j] is ONE sequential float64 FMA chain over k = 0 .. d - 1
// from +0.0 -- no K blocks, no split accumulators.  The chain runs on the vector unit (v_fma_f64): a thread owns a 4 x 4 block of
// a 64 x 64 output tile and feeds its 16 chains one k at a time, in order, from two k-major LDS panels of 16 k-steps.  The fp64
// MFMA (v_mfma_f64_16x16x4_f64) is not used: the order in which it accumulates its four k-steps is not documented, and the
// vector unit has the same float64 FMA rate.
// Epilogue (contraction off, every operation rounded on its own): cosine -C; Euclidean (sqa[i] + sqb[j]) - 2 C, the left-to-right
// evaluation of numexpr's 'A + B - 2 * C' (2 C is exact).  img = (float)out, round to nearest even: a monotone map, which is what
// lets se_rank_rows order the images and se_rank_refine_f64 repair only the runs of equal images.
#include "se_common.h"

namespace se {

constexpr int P64_THREADS = 256;
constexpr int P64_TILE = 64;                // output tile side
constexpr int P64_KC = 16;                  // k-steps per LDS panel
constexpr int P64_LD = P64_TILE + 2;        // panel row pitch in doubles: rows stay 16-byte aligned for the 4-double reads

// One [P64_KC][P64_TILE] panel of x (rows r0 .. r0 + 63, columns k0 .. k0 + kn - 1), k-major; rows past `rows` read as +0.
__device__ __forceinline__ void p64_stage(double *__restrict__ panel, const double *__restrict__ x, int64_t ldx, int64_t r0, int64_t rows,
                                          int64_t k0, int kn, int tid)
{
#pragma unroll
    for (int e = tid; e < P64_TILE * P64_KC; e += P64_THREADS) {
        const int r = e / P64_KC, k = e % P64_KC;        // 16 consecutive threads read 128 contiguous bytes of one row
        double v = 0.0;
        if (r0 + r < rows && k < kn) v = x[(r0 + r) * ldx + k0 + k];
        panel[k * P64_LD + r] = v;
    }
}

template <int METRIC>
__global__ __launch_bounds__(P64_THREADS) void pdist_f64_kernel(const double *__restrict__ a, int64_t lda, const double *__restrict__ b,
                                                                int64_t ldb, const double *__restrict__ sqa, const double *__restrict__ sqb,
                                                                int64_t q, int64_t n, int64_t d, double *__restrict__ out, int64_t ldo,
                                                                float *__restrict__ img, int64_t ldi, int64_t tiles_n)
{
    __shared__ __attribute__((aligned(16))) double pa[P64_KC * P64_LD];
    __shared__ __attribute__((aligned(16))) double pb[P64_KC * P64_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = ((int64_t)blockIdx.x / tiles_n) * P64_TILE, j0 = ((int64_t)blockIdx.x % tiles_n) * P64_TILE;

    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0.0;

    for (int64_t k0 = 0; k0 < d; k0 += P64_KC) {
        const int kn = (int)(d - k0 < P64_KC ? d - k0 : P64_KC);
        p64_stage(pa, a, lda, i0, q, k0, kn, tid);
        p64_stage(pb, b, ldb, j0, n, k0, kn, tid);
        wg_barrier();
        auto step = [&](int k) {        // k-step k of all 16 chains of this thread
            double av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; r++) av[r] = pa[k * P64_LD + 4 * ty + r];
#pragma unroll
            for (int c = 0; c < 4; c++) bv[c] = pb[k * P64_LD + 4 * tx + c];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] = fma(av[r], bv[c], acc[r][c]);
        };
        // only the kn real k-steps enter the chains: the chain of d steps is the contract, not a chain padded with zero products
        if (kn == P64_KC) {
#pragma unroll
            for (int k = 0; k < P64_KC; k++) step(k);
        } else {
            for (int k = 0; k < kn; k++) step(k);
        }
        wg_barrier();
    }

#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t i = i0 + 4 * ty + r;
        if (i >= q) continue;
        double sa = 0.0;
        if (METRIC == SE_METRIC_EUCLID) sa = sqa[i];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int64_t j = j0 + 4 * tx + c;
            if (j >= n) continue;
            double v;
            if (METRIC == SE_METRIC_EUCLID) {
                const double s = sa + sqb[j];
                v = s - 2.0 * acc[r][c];
            } else {
                v = -acc[r][c];
            }
            out[i * ldo + j] = v;
            if (img) img[i * ldi + j] = __double2float_rn(v);
        }
    }
}

}  // namespace se

using namespace se;

extern "C" int se_pairwise_dist_f64(const double *a, int64_t lda, const double *b, int64_t ldb, const double *sqa, const double *sqb,
                                    int64_t q, int64_t n, int64_t d, int metric, double *out, int64_t ldo, float *img, int64_t ldi,
                                    se_stream_t stream)
{
    const char *who = "se_pairwise_dist_f64";
    if (q < 0 || n < 0 || d < 0) return fail(SE_ERR_INVALID, "%s: negative shape q=%lld n=%lld d=%lld", who, (long long)q, (long long)n, (long long)d);
    if (metric != SE_METRIC_COSINE && metric != SE_METRIC_EUCLID) return fail(SE_ERR_INVALID, "%s: metric must be SE_METRIC_COSINE or SE_METRIC_EUCLID", who);
    if (q == 0 || n == 0) return SE_OK;
    if (!a || !b || !out) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (metric == SE_METRIC_EUCLID && (!sqa || !sqb)) return fail(SE_ERR_INVALID, "%s: the Euclidean metric needs sqa and sqb", who);
    if (lda < d || ldb < d || ldo < n || (img && ldi < n)) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    const int64_t tiles_q = (q + P64_TILE - 1) / P64_TILE, tiles_n = (n + P64_TILE - 1) / P64_TILE;
    if (tiles_q > 0x7FFFFFFF / tiles_n) return fail(SE_ERR_UNSUPPORTED, "%s: too many tiles (%lld x %lld)", who, (long long)tiles_q, (long long)tiles_n);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles_q * tiles_n)), block(P64_THREADS);
    if (metric == SE_METRIC_EUCLID)
        hipLaunchKernelGGL(pdist_f64_kernel<SE_METRIC_EUCLID>, grid, block, 0, s, a, lda, b, ldb, sqa, sqb, q, n, d, out, ldo, img, ldi, tiles_n);
    else
        hipLaunchKernelGGL(pdist_f64_kernel<SE_METRIC_COSINE>, grid, block, 0, s, a, lda, b, ldb, sqa, sqb, q, n, d, out, ldo, img, ldi, tiles_n);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
