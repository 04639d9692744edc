// bootstrap.hip -- bootstrap over queries: means of per-query metric rows resampled with replacement (se_bootstrap_means), and the
// pinned index stream behind it (se_bootstrap_indices).
//
// Replaces the host composition np.random.randint(q, size = (R, q)) -> table[idx].mean(axis = 1): R x q row gathers (5e8 at q = 50,000
// and R = 10,000) of rows of ~11 doubles, tens of seconds in NumPy, hundreds of 400 MB temporaries as a torch composition -- and no
// generator of either promises the same stream on the next version.  Here the stream is part of the ABI (include/sehip.h):
// Philox4x32-10 keyed by the seed, counter = (block of two draws, replicate), index = high half of u64 * q.
//
// bootstrap_means_kernel: ONE 256-THREAD WORKGROUP per replicate (workgroups stride over the replicates).  Thread j takes the Philox
// blocks j, j + 256, ... of its replicate: one Philox call, two indices, two row gathers, m float64 adds per row in draw order.  The
// table is a few MB (50,000 x 11 doubles = 4.4 MB: over one XCD's L2, far inside the Infinity Cache), every draw lands on a random
// row, so the kernel is a gather kernel: a row is read by ONE lane in 16-byte pieces, and the binding pads the row pitch so that a
// row stays inside one 128-byte line (sehip.bootstrap_means).  The 256 thread sums of a column are combined without atomics in an
// order that only the source fixes: a butterfly inside each wave, then the four wave sums in wave order through LDS.  Nothing in the
// order depends on reps, rep0 or the grid, so a replicate has the same bits whichever call computes it.
#include "se_common.h"

namespace se {

constexpr int BS_THREADS = 256;
constexpr int BS_WAVES = BS_THREADS / WAVE;

// Philox4x32-10 (Salmon et al., SC'11), as include/sehip.h states it
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// the two draws 2 b and 2 b + 1 of replicate r: both lie in [0, q) for every u (u * q < 2^64 * q)
__device__ __forceinline__ void bootstrap_pair(uint64_t seed, uint64_t r, uint64_t b, uint32_t q, uint32_t &i0, uint32_t &i1)
{
    const uint4 x = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)r, (uint32_t)(r >> 32)), (uint32_t)seed, (uint32_t)(seed >> 32));
    // (u * q) >> 64 with u = lo | hi << 32 and q < 2^32:  (hi * q + ((lo * q) >> 32)) >> 32, which cannot overflow 64 bits
    i0 = (uint32_t)(((uint64_t)x.y * q + __umulhi(x.x, q)) >> 32);
    i1 = (uint32_t)(((uint64_t)x.w * q + __umulhi(x.z, q)) >> 32);
}

// v[c] = row[c], c < M.  VEC: every row starts on a 16-byte boundary (base aligned, even pitch)
template <int M, bool VEC>
__device__ __forceinline__ void load_row(const double *__restrict__ row, double *v)
{
    if constexpr (VEC) {
#pragma unroll
        for (int c = 0; c + 1 < M; c += 2) {
            const double2 p = *(const double2 *)(row + c);
            v[c] = p.x;
            v[c + 1] = p.y;
        }
        if constexpr (M & 1) v[M - 1] = row[M - 1];
    } else {
#pragma unroll
        for (int c = 0; c < M; c++) v[c] = row[c];
    }
}

template <int M, bool VEC>
__global__ __launch_bounds__(BS_THREADS) void bootstrap_means_kernel(const double *__restrict__ vals, int64_t ldv, uint32_t q, uint64_t seed,
                                                                     int64_t rep0, int64_t reps, double *__restrict__ out, int64_t ldo)
{
    __shared__ double part[BS_WAVES][SE_BOOTSTRAP_COLS_MAX];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t nblk = ((uint64_t)q + 1) >> 1;
    const double qd = (double)q;
    for (int64_t rr = blockIdx.x; rr < reps; rr += gridDim.x) {
        const uint64_t r = (uint64_t)(rep0 + rr);
        double acc[M];
#pragma unroll
        for (int c = 0; c < M; c++) acc[c] = 0.0;
        for (uint64_t b = threadIdx.x; b < nblk; b += BS_THREADS) {
            uint32_t i0, i1;
            bootstrap_pair(seed, r, b, q, i0, i1);
            const bool two = 2 * b + 1 < q;         // an odd q ends in the middle of a block
            double v0[M], v1[M];
            load_row<M, VEC>(vals + (int64_t)i0 * ldv, v0);
            if (two) load_row<M, VEC>(vals + (int64_t)i1 * ldv, v1);
#pragma unroll
            for (int c = 0; c < M; c++) acc[c] += v0[c];
            if (two) {
#pragma unroll
                for (int c = 0; c < M; c++) acc[c] += v1[c];
            }
        }
#pragma unroll
        for (int c = 0; c < M; c++) {
            const double s = wave_sum(acc[c]);
            if (lane == 0) part[wave][c] = s;
        }
        wg_barrier();
        if ((int)threadIdx.x < M) {
            const int c = threadIdx.x;
            out[rr * ldo + c] = (((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) / qd;
        }
        wg_barrier();       // part is rewritten for the next replicate
    }
}

// one thread per (replicate, Philox block) of the window; it writes the one or two draws of its block that lie inside
__global__ __launch_bounds__(BS_THREADS) void bootstrap_indices_kernel(uint32_t q, uint64_t seed, int64_t rep0, int64_t reps, int64_t t0, int64_t count,
                                                                       int32_t *__restrict__ out, int64_t ldo)
{
    const int64_t b0 = t0 >> 1, nb = ((t0 + count - 1) >> 1) - b0 + 1;
    const int64_t total = reps * nb;
    for (int64_t e = (int64_t)blockIdx.x * BS_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * BS_THREADS) {
        const int64_t rr = e / nb, b = b0 + e % nb;
        uint32_t i0, i1;
        bootstrap_pair(seed, (uint64_t)(rep0 + rr), (uint64_t)b, q, i0, i1);
        const int64_t t = 2 * b;
        if (t >= t0 && t < t0 + count) out[rr * ldo + (t - t0)] = (int32_t)i0;
        if (t + 1 >= t0 && t + 1 < t0 + count) out[rr * ldo + (t + 1 - t0)] = (int32_t)i1;
    }
}

template <int M>
static void launch_means(bool vec, unsigned blocks, hipStream_t s, const double *vals, int64_t ldv, uint32_t q, uint64_t seed, int64_t rep0,
                         int64_t reps, double *out, int64_t ldo)
{
    dispatch_bools(vec, [&](auto v) {
        hipLaunchKernelGGL((bootstrap_means_kernel<M, decltype(v)::value>), dim3(blocks), dim3(BS_THREADS), 0, s, vals, ldv, q, seed, rep0, reps, out, ldo);
    });
}

template <int M = 1>
static void dispatch_means(int m, bool vec, unsigned blocks, hipStream_t s, const double *vals, int64_t ldv, uint32_t q, uint64_t seed, int64_t rep0,
                           int64_t reps, double *out, int64_t ldo)
{
    if constexpr (M <= SE_BOOTSTRAP_COLS_MAX) {
        if (m == M) launch_means<M>(vec, blocks, s, vals, ldv, q, seed, rep0, reps, out, ldo);
        else dispatch_means<M + 1>(m, vec, blocks, s, vals, ldv, q, seed, rep0, reps, out, ldo);
    }
}

static int check_stream_args(const char *who, int64_t q, int64_t rep0, int64_t reps)
{
    if (q < 1 || q > 2147483647LL) return fail(SE_ERR_INVALID, "%s: q=%lld outside [1, 2^31 - 1]", who, (long long)q);
    if (rep0 < 0 || reps < 0 || rep0 > INT64_MAX - reps)
        return fail(SE_ERR_INVALID, "%s: replicates rep0=%lld reps=%lld must be non-negative", who, (long long)rep0, (long long)reps);
    return SE_OK;
}

}  // namespace se

using namespace se;

extern "C" int se_bootstrap_means(const double *vals, int64_t ldv, int64_t q, int m, int64_t seed, int64_t rep0, int64_t reps, double *out,
                                  int64_t ldo, se_stream_t stream)
{
    const int rc = check_stream_args("se_bootstrap_means", q, rep0, reps);
    if (rc != SE_OK) return rc;
    if (m < 1 || m > SE_BOOTSTRAP_COLS_MAX) return fail(SE_ERR_INVALID, "se_bootstrap_means: m=%d outside [1, %d]", m, SE_BOOTSTRAP_COLS_MAX);
    if (ldv < m || ldo < m)
        return fail(SE_ERR_INVALID, "se_bootstrap_means: leading dimensions ldv=%lld ldo=%lld below m=%d", (long long)ldv, (long long)ldo, m);
    if (reps == 0) return SE_OK;
    if (!vals || !out) return fail(SE_ERR_INVALID, "se_bootstrap_means: null pointer");
    const unsigned blocks = row_blocks(reps, 1, (int64_t)num_cus() * 64);
    dispatch_means(m, aligned16(vals, ldv, 8), blocks, (hipStream_t)stream, vals, ldv, (uint32_t)q, (uint64_t)seed, rep0, reps, out, ldo);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_bootstrap_indices(int64_t q, int64_t seed, int64_t rep0, int64_t reps, int64_t t0, int64_t count, int32_t *out, int64_t ldo,
                                    se_stream_t stream)
{
    const int rc = check_stream_args("se_bootstrap_indices", q, rep0, reps);
    if (rc != SE_OK) return rc;
    if (t0 < 0 || count < 0 || t0 > q || count > q - t0)
        return fail(SE_ERR_INVALID, "se_bootstrap_indices: window t0=%lld count=%lld outside [0, q=%lld]", (long long)t0, (long long)count, (long long)q);
    if (ldo < count) return fail(SE_ERR_INVALID, "se_bootstrap_indices: leading dimension %lld below count=%lld", (long long)ldo, (long long)count);
    if (reps == 0 || count == 0) return SE_OK;
    if (!out) return fail(SE_ERR_INVALID, "se_bootstrap_indices: null pointer");
    const int64_t nb = ((t0 + count - 1) >> 1) - (t0 >> 1) + 1;
    if (reps > INT64_MAX / nb) return fail(SE_ERR_INVALID, "se_bootstrap_indices: reps=%lld x count=%lld overflows", (long long)reps, (long long)count);
    const unsigned blocks = row_blocks(reps * nb, BS_THREADS, (int64_t)num_cus() * 16);
    hipLaunchKernelGGL(bootstrap_indices_kernel, dim3(blocks), dim3(BS_THREADS), 0, (hipStream_t)stream, (uint32_t)q, (uint64_t)seed, rep0, reps, t0,
                       count, out, ldo);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
