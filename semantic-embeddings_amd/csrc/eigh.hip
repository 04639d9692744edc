// eigh.hip -- symmetric float64 eigendecomposition on the device: two-sided block Jacobi with a round-robin (tournament) ordering.
//
// Replaces the np.linalg.eigh of compute_class_embedding.py's sim_approx (:44-72) and mds (:134-160).
//
// Columns are grouped in blocks of EIGH_B = 32; the matrix is taken as padded with exact zeros to nb = an even number of blocks
// (the padding is never stored: loads past n read 0, stores past n are dropped).  One sweep is nb - 1 rounds of nb / 2 disjoint
// block pairs (se_eigh_schedule: the circle method, every unordered pair of blocks once), and a round is three launches:
//
// * eigh_pair_kernel: one workgroup per pair loads the symmetric 64 x 64 sub-block of its two blocks into LDS and diagonalises it
//   by cyclic Jacobi (the same circle method over its 64 indices: 63 rounds of 32 disjoint rotations, three barriers a round), at
//   most EIGH_MAX_INNER inner sweeps, ending early once no entry needs a rotation.  A rotation is skipped when its off-diagonal
//   entry is exactly 0 (so the zero padding never mixes with real rows), or negligible: |a_pq| <= 2^-54 sqrt(|a_pp a_qq|) or
//   <= 2^-54 |A|_F / n.  The diagonalised sub-block goes back to A, the accumulated rotation J -- transposed -- to the workspace,
//   and a flag says whether the pair rotated at all (late sweeps: most do not, and their updates return at once).
// * eigh_update_kernel<false>: A[:, pair] <- A[:, pair] J and V[:, pair] <- V[:, pair] J as 64 x 64 tiles on
//   v_mfma_f64_16x16x4_f64 (operand and C/D lane maps of chol_update_kernel, classemb.hip); the rows of the pair itself are
//   left to the pair kernel's exact sub-block.
// * eigh_update_kernel<true>: A[pair, :] <- J^T A[pair, :], the same tiles with the operand roles swapped.
//
// eigh_norms_kernel sums off(A)^2 = sum_{i != j} a_ij^2 directly (|A|_F^2 - sum diag^2 would stall at 1e-8 by cancellation) in
// a fixed order; the host reads one double per sweep and stops at off <= sqrt(n) 2^-53 |A|_F (the level the skip rule can
// always reach).  Every loop is bounded: max_sweeps outer, EIGH_MAX_INNER inner; non-convergence and non-finite input are
// reported through `info`.  Eigenvalues are sorted on the host (n values), eigenvectors gathered on the device.
#include "se_common.h"

#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace se {

constexpr int EIGH_B = 32;                  // block width
constexpr int EIGH_P = 2 * EIGH_B;          // pair width
constexpr int EIGH_THREADS = 256;
constexpr int EIGH_LDS = EIGH_P + 1;        // pair kernel: [64][65] doubles (conflict-free rows and columns)
constexpr int EIGH_LDU = EIGH_P + 2;        // update operands: [64][66] doubles, as chol_update_kernel
constexpr int EIGH_MAX_INNER = 12;          // inner sweeps of one pair at most
constexpr int EIGH_NORM_BLOCKS = 256;
constexpr int64_t EIGH_MAX_N = (int64_t)1 << 17;

typedef double dbl4 __attribute__((ext_vector_type(4)));

// pair k (0 .. m / 2 - 1) of round r (0 .. m - 2) of the circle method over m players (m even): (lo, hi), lo < hi
__host__ __device__ inline void eigh_pair_of(int m, int r, int k, int &lo, int &hi)
{
    const int c = m - 1;
    int a, b;
    if (k == 0) {
        a = r;
        b = c;
    } else {
        a = (r + k) % c;
        b = (r - k + c) % c;
    }
    lo = a < b ? a : b;
    hi = a < b ? b : a;
}

// global row / column of local index l (0 .. 63) of the pair (p, q)
__device__ __forceinline__ int64_t eigh_gidx(int p, int q, int l)
{
    return l < EIGH_B ? (int64_t)p * EIGH_B + l : (int64_t)q * EIGH_B + (l - EIGH_B);
}

__device__ __forceinline__ bool eigh_needs_rotation(double app, double aqq, double apq, double delta)
{
    const double x = fabs(apq);
    return apq != 0.0 && x > delta && x > 0x1p-54 * sqrt(fabs(app * aqq));
}

// V = I
__global__ __launch_bounds__(EIGH_THREADS) void eigh_identity_kernel(double *__restrict__ v, int64_t ldv, int64_t n)
{
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x)
        for (int64_t c = threadIdx.x; c < n; c += EIGH_THREADS) v[i * ldv + c] = c == i ? 1.0 : 0.0;
}

__global__ __launch_bounds__(EIGH_THREADS) void eigh_fill_nan_kernel(double *__restrict__ w, double *__restrict__ v, int64_t ldv, int64_t n)
{
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        if (threadIdx.x == 0) w[i] = nan;
        for (int64_t c = threadIdx.x; c < n; c += EIGH_THREADS) v[i * ldv + c] = nan;
    }
}

// part[2 b] = sum of a_ij^2 over the rows of workgroup b with i != j, part[2 b + 1] = the same with the diagonal
__global__ __launch_bounds__(EIGH_THREADS) void eigh_norms_kernel(const double *__restrict__ a, int64_t lda, int64_t n, double *__restrict__ part)
{
    __shared__ double red[2 * EIGH_THREADS / WAVE];
    double off = 0.0, all = 0.0;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x)
        for (int64_t c = threadIdx.x; c < n; c += EIGH_THREADS) {
            const double x = a[i * lda + c], sq = x * x;
            all += sq;
            if (c != i) off += sq;
        }
    off = wave_sum(off);
    all = wave_sum(all);
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) {
        red[2 * wave] = off;
        red[2 * wave + 1] = all;
    }
    wg_barrier();
    if (threadIdx.x == 0) {
        double o = 0.0, f = 0.0;
        for (int w = 0; w < EIGH_THREADS / WAVE; w++) {
            o += red[2 * w];
            f += red[2 * w + 1];
        }
        part[2 * blockIdx.x] = o;
        part[2 * blockIdx.x + 1] = f;
    }
}

// out[0] = off(A)^2, out[1] = |A|_F^2: the partial sums added in order
__global__ __launch_bounds__(WAVE) void eigh_norms_finish_kernel(const double *__restrict__ part, int blocks, double *__restrict__ out)
{
    if (threadIdx.x == 0) {
        double o = 0.0, f = 0.0;
        for (int b = 0; b < blocks; b++) {
            o += part[2 * b];
            f += part[2 * b + 1];
        }
        out[0] = o;
        out[1] = f;
    }
}

// One workgroup per block pair of the round: cyclic Jacobi on its 64 x 64 sub-block in LDS.
__global__ __launch_bounds__(EIGH_THREADS) void eigh_pair_kernel(double *__restrict__ a, int64_t lda, int64_t n, int nb, int round,
                                                                 double delta, double *__restrict__ jt_ws, int32_t *__restrict__ rotated)
{
    __shared__ double S[EIGH_P * EIGH_LDS];
    __shared__ double J[EIGH_P * EIGH_LDS];
    __shared__ double s_c[EIGH_B], s_s[EIGH_B];
    __shared__ int s_p[EIGH_B], s_q[EIGH_B];
    __shared__ int s_todo;
    const int tid = threadIdx.x;
    int p, q;
    eigh_pair_of(nb, round, (int)blockIdx.x, p, q);

    for (int idx = tid; idx < EIGH_P * EIGH_P; idx += EIGH_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        const int64_t gr = eigh_gidx(p, q, r), gc = eigh_gidx(p, q, c);
        S[r * EIGH_LDS + c] = (gr < n && gc < n) ? a[gr * lda + gc] : 0.0;
        J[r * EIGH_LDS + c] = r == c ? 1.0 : 0.0;
    }
    if (tid == 0) s_todo = 0;
    wg_barrier();

    bool any = false;
    for (int sweep = 0; sweep < EIGH_MAX_INNER; sweep++) {
        // does any entry above the diagonal still need a rotation?
        bool mine = false;
        for (int idx = tid; idx < EIGH_P * EIGH_P; idx += EIGH_THREADS) {
            const int r = idx >> 6, c = idx & 63;
            if (c > r && eigh_needs_rotation(S[r * EIGH_LDS + r], S[c * EIGH_LDS + c], S[r * EIGH_LDS + c], delta)) mine = true;
        }
        if (mine) s_todo = sweep + 1;           // every writer stores the same value
        wg_barrier();
        if (s_todo != sweep + 1) break;         // uniform: read after the barrier, written again only after the next one
        any = true;
        for (int rr = 0; rr < EIGH_P - 1; rr++) {
            if (tid < EIGH_B) {
                int lo, hi;
                eigh_pair_of(EIGH_P, rr, tid, lo, hi);
                const double app = S[lo * EIGH_LDS + lo], aqq = S[hi * EIGH_LDS + hi], apq = S[lo * EIGH_LDS + hi];
                double c = 1.0, s = 0.0;
                if (eigh_needs_rotation(app, aqq, apq, delta)) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                }
                s_c[tid] = c;
                s_s[tid] = s;
                s_p[tid] = lo;
                s_q[tid] = hi;
            }
            wg_barrier();
            // columns of S and J: (p, q) <- (c p - s q, s p + c q); thread = (rotation, row)
            for (int idx = tid; idx < EIGH_B * EIGH_P; idx += EIGH_THREADS) {
                const int k = idx >> 6, i = idx & 63;
                const double c = s_c[k], s = s_s[k];
                if (s != 0.0) {
                    const int lo = s_p[k], hi = s_q[k];
                    const double x = S[i * EIGH_LDS + lo], y = S[i * EIGH_LDS + hi];
                    S[i * EIGH_LDS + lo] = c * x - s * y;
                    S[i * EIGH_LDS + hi] = s * x + c * y;
                    const double jx = J[i * EIGH_LDS + lo], jy = J[i * EIGH_LDS + hi];
                    J[i * EIGH_LDS + lo] = c * jx - s * jy;
                    J[i * EIGH_LDS + hi] = s * jx + c * jy;
                }
            }
            wg_barrier();
            // rows of S alike; thread = (rotation, column); the rotated entry itself becomes an exact 0
            // (the column pass and the row pass round (i, j) and (j, i) in different orders: S stays symmetric to rounding only.
            // Decisions read the upper triangle; eigh_norms_kernel sums both, which differ at rounding level of entries that
            // are themselves below the stopping level)
            for (int idx = tid; idx < EIGH_B * EIGH_P; idx += EIGH_THREADS) {
                const int k = idx >> 6, j = idx & 63;
                const double c = s_c[k], s = s_s[k];
                if (s != 0.0) {
                    const int lo = s_p[k], hi = s_q[k];
                    const double x = S[lo * EIGH_LDS + j], y = S[hi * EIGH_LDS + j];
                    S[lo * EIGH_LDS + j] = (j == hi) ? 0.0 : c * x - s * y;
                    S[hi * EIGH_LDS + j] = (j == lo) ? 0.0 : s * x + c * y;
                }
            }
            wg_barrier();
        }
    }

    if (tid == 0) rotated[blockIdx.x] = any ? 1 : 0;
    if (!any) return;                           // nothing changed: A keeps its sub-block, the updates of this pair are skipped
    double *jt = jt_ws + (int64_t)blockIdx.x * EIGH_P * EIGH_P;
    for (int idx = tid; idx < EIGH_P * EIGH_P; idx += EIGH_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        const int64_t gr = eigh_gidx(p, q, r), gc = eigh_gidx(p, q, c);
        if (gr < n && gc < n) a[gr * lda + gc] = S[r * EIGH_LDS + c];
        jt[r * EIGH_P + c] = J[c * EIGH_LDS + r];
    }
}

// ROWS = false: M[tile rows, pair] <- M[tile rows, pair] J for M = A (blockIdx.z = 0; the pair's own rows are skipped) and
//               M = V (blockIdx.z = 1).
// ROWS = true:  A[pair, tile columns] <- J^T A[pair, tile columns] (the pair's own columns are skipped).
// blockIdx.x: pair of the round, blockIdx.y: tile of 64 rows / columns.
template <bool ROWS>
__global__ __launch_bounds__(EIGH_THREADS) void eigh_update_kernel(double *__restrict__ a, int64_t lda, double *__restrict__ v, int64_t ldv,
                                                                   int64_t n, int nb, int round, const double *__restrict__ jt_ws,
                                                                   const int32_t *__restrict__ rotated)
{
    __shared__ double xs[EIGH_P * EIGH_LDU];    // ROWS: [tile column][pair row] (the tile transposed); else [tile row][pair column]
    __shared__ double js[EIGH_P * EIGH_LDU];    // J^T: [j][k] = J[k][j]
    if (!rotated[blockIdx.x]) return;           // uniform over the workgroup, before any barrier
    const bool is_v = !ROWS && blockIdx.z == 1;
    double *m = is_v ? v : a;
    const int64_t ld = is_v ? ldv : lda;
    int p, q;
    eigh_pair_of(nb, round, (int)blockIdx.x, p, q);
    const int64_t t0 = (int64_t)blockIdx.y * EIGH_P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *jt = jt_ws + (int64_t)blockIdx.x * EIGH_P * EIGH_P;

    for (int idx = tid; idx < EIGH_P * EIGH_P; idx += EIGH_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        js[r * EIGH_LDU + c] = jt[r * EIGH_P + c];
        if (ROWS) {
            const int64_t gr = eigh_gidx(p, q, r), gc = t0 + c;
            xs[c * EIGH_LDU + r] = (gr < n && gc < n) ? m[gr * ld + gc] : 0.0;
        } else {
            const int64_t gr = t0 + r, gc = eigh_gidx(p, q, c);
            xs[r * EIGH_LDU + c] = (gr < n && gc < n) ? m[gr * ld + gc] : 0.0;
        }
    }
    wg_barrier();

    const double *opa = ROWS ? js : xs, *opb = ROWS ? xs : js;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    dbl4 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; bi++)
#pragma unroll
        for (int bj = 0; bj < 2; bj++) acc[bi][bj] = dbl4{0.0, 0.0, 0.0, 0.0};
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 4
    for (int ks = 0; ks < EIGH_P; ks += 4) {
        // out[i][j] = sum_k opa[i][k] opb[j][k]:  lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15]
        const double a0 = opa[(wr + lr) * EIGH_LDU + ks + lk], a1 = opa[(wr + 16 + lr) * EIGH_LDU + ks + lk];
        const double b0 = opb[(wc + lr) * EIGH_LDU + ks + lk], b1 = opb[(wc + 16 + lr) * EIGH_LDU + ks + lk];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int bi = 0; bi < 2; bi++)
#pragma unroll
        for (int bj = 0; bj < 2; bj++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = wr + 16 * bi + lk + 4 * e, j = wc + 16 * bj + lr;
                const int64_t gr = ROWS ? eigh_gidx(p, q, i) : t0 + i, gc = ROWS ? t0 + j : eigh_gidx(p, q, j);
                if (gr >= n || gc >= n) continue;
                if (!is_v) {
                    const int64_t blk = (ROWS ? gc : gr) / EIGH_B;     // the pair's own sub-block belongs to the pair kernel
                    if (blk == p || blk == q) continue;
                }
                m[gr * ld + gc] = acc[bi][bj][e];
            }
}

__global__ __launch_bounds__(EIGH_THREADS) void eigh_diag_kernel(const double *__restrict__ a, int64_t lda, int64_t n, double *__restrict__ d)
{
    const int64_t i = (int64_t)blockIdx.x * EIGH_THREADS + threadIdx.x;
    if (i < n) d[i] = a[i * lda + i];
}

// w[j] = d[perm[j]], v[:, j] = vw[:, perm[j]]
__global__ __launch_bounds__(EIGH_THREADS) void eigh_gather_kernel(const double *__restrict__ d, const double *__restrict__ vw, int64_t n,
                                                                   const int32_t *__restrict__ perm, double *__restrict__ w,
                                                                   double *__restrict__ v, int64_t ldv)
{
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x)
        for (int64_t c = threadIdx.x; c < n; c += EIGH_THREADS) {
            const int64_t src = perm[c];
            if (i == 0) w[c] = d[src];
            v[i * ldv + c] = vw[i * n + src];
        }
}

// workspace layout (doubles first, every part a multiple of 8 bytes)
struct EighWs {
    int64_t vw, jt, diag, norms, part, perm, rotated, bytes;
};

static inline EighWs eigh_layout(int64_t n)
{
    const int64_t pairs = (n + EIGH_P - 1) / EIGH_P > 0 ? (n + EIGH_P - 1) / EIGH_P : 1;     // nb / 2
    EighWs w;
    int64_t off = 0;
    w.vw = off;
    off += n * n * 8;
    w.jt = off;
    off += pairs * EIGH_P * EIGH_P * 8;
    w.diag = off;
    off += n * 8;
    w.norms = off;
    off += 2 * 8;
    w.part = off;
    off += 2 * EIGH_NORM_BLOCKS * 8;
    w.perm = off;
    off += ((n + 1) / 2) * 8;
    w.rotated = off;
    off += ((pairs + 1) / 2) * 8;
    w.bytes = off;
    return w;
}

}  // namespace se

using namespace se;

extern "C" int64_t se_eigh_f64_workspace_bytes(int64_t n)
{
    if (n < 0 || n > EIGH_MAX_N) return -1;
    return eigh_layout(n).bytes;
}

extern "C" int se_eigh_schedule(int nb, int32_t *pairs)
{
    const char *who = "se_eigh_schedule";
    if (nb < 2 || (nb & 1)) return fail(SE_ERR_INVALID, "%s: nb=%d must be even and >= 2", who, nb);
    if (!pairs) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    for (int r = 0; r < nb - 1; r++)
        for (int k = 0; k < nb / 2; k++) {
            int lo, hi;
            eigh_pair_of(nb, r, k, lo, hi);
            pairs[((int64_t)r * (nb / 2) + k) * 2] = lo;
            pairs[((int64_t)r * (nb / 2) + k) * 2 + 1] = hi;
        }
    return SE_OK;
}

extern "C" int se_eigh_f64(double *a, int64_t lda, int64_t n, double *w, double *v, int64_t ldv, void *workspace, int32_t *info,
                           int max_sweeps, se_stream_t stream)
{
    const char *who = "se_eigh_f64";
    if (n < 0) return fail(SE_ERR_INVALID, "%s: bad size n=%lld", who, (long long)n);
    if (n > EIGH_MAX_N) return fail(SE_ERR_UNSUPPORTED, "%s: n=%lld above %lld", who, (long long)n, (long long)EIGH_MAX_N);
    if (max_sweeps < 0) return fail(SE_ERR_INVALID, "%s: max_sweeps=%d must be >= 0", who, max_sweeps);
    if (!info || (n > 0 && (!a || !w || !v || !workspace))) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (n > 0 && (lda < n || ldv < n)) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    if (((uintptr_t)workspace) & 7) return fail(SE_ERR_INVALID, "%s: workspace must be 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    int32_t code = 0;
    if (n == 0) {
        SE_HIP_CHECK(hipMemcpyAsync(info, &code, sizeof(code), hipMemcpyHostToDevice, s));
        SE_HIP_CHECK(hipStreamSynchronize(s));
        return SE_OK;
    }
    const EighWs L = eigh_layout(n);
    char *base = (char *)workspace;
    double *vw = (double *)(base + L.vw), *jt = (double *)(base + L.jt), *diag = (double *)(base + L.diag);
    double *norms = (double *)(base + L.norms), *part = (double *)(base + L.part);
    int32_t *perm = (int32_t *)(base + L.perm), *rotated = (int32_t *)(base + L.rotated);
    const int pairs = (int)((n + EIGH_P - 1) / EIGH_P), nb = 2 * pairs;
    const unsigned tiles = (unsigned)pairs;                                   // 64-row / 64-column tiles: ceil(n / 64)
    const unsigned rows_grid = (unsigned)(n < 1024 ? n : 1024);
    const int norm_blocks = (int)(n < EIGH_NORM_BLOCKS ? n : EIGH_NORM_BLOCKS);

    double h_norms[2] = {0.0, 0.0};
    auto read_norms = [&]() -> int {
        hipLaunchKernelGGL(eigh_norms_kernel, dim3(norm_blocks), dim3(EIGH_THREADS), 0, s, (const double *)a, lda, n, part);
        SE_LAUNCH_CHECK();
        hipLaunchKernelGGL(eigh_norms_finish_kernel, dim3(1), dim3(WAVE), 0, s, (const double *)part, norm_blocks, norms);
        SE_LAUNCH_CHECK();
        SE_HIP_CHECK(hipMemcpyAsync(h_norms, norms, sizeof(h_norms), hipMemcpyDeviceToHost, s));
        SE_HIP_CHECK(hipStreamSynchronize(s));
        return SE_OK;
    };

    int rc = read_norms();
    if (rc != SE_OK) return rc;
    const double fro2 = h_norms[1];
    if (!std::isfinite(fro2)) {
        code = SE_EIGH_NONFINITE;
        hipLaunchKernelGGL(eigh_fill_nan_kernel, dim3(rows_grid), dim3(EIGH_THREADS), 0, s, w, v, ldv, n);
        SE_LAUNCH_CHECK();
        SE_HIP_CHECK(hipMemcpyAsync(info, &code, sizeof(code), hipMemcpyHostToDevice, s));
        SE_HIP_CHECK(hipStreamSynchronize(s));
        return SE_OK;
    }
    hipLaunchKernelGGL(eigh_identity_kernel, dim3(rows_grid), dim3(EIGH_THREADS), 0, s, vw, n, n);
    SE_LAUNCH_CHECK();

    const double tol2 = ((double)n * 0x1p-106) * fro2;                         // off <= sqrt(n) 2^-53 |A|_F
    const double delta = 0x1p-54 * sqrt(fro2) / (double)n;
    code = SE_EIGH_NOT_CONVERGED;
    for (int sweep = 0; sweep <= max_sweeps; sweep++) {
        if (sweep > 0) {
            rc = read_norms();
            if (rc != SE_OK) return rc;
        }
        if (h_norms[0] <= tol2) {
            code = sweep;
            break;
        }
        if (sweep == max_sweeps || !std::isfinite(h_norms[0])) break;
        for (int r = 0; r < nb - 1; r++) {
            hipLaunchKernelGGL(eigh_pair_kernel, dim3(pairs), dim3(EIGH_THREADS), 0, s, a, lda, n, nb, r, delta, jt, rotated);
            SE_LAUNCH_CHECK();
            hipLaunchKernelGGL(eigh_update_kernel<false>, dim3(pairs, tiles, 2), dim3(EIGH_THREADS), 0, s, a, lda, vw, n, n, nb, r,
                               (const double *)jt, (const int32_t *)rotated);
            SE_LAUNCH_CHECK();
            hipLaunchKernelGGL(eigh_update_kernel<true>, dim3(pairs, tiles, 1), dim3(EIGH_THREADS), 0, s, a, lda, vw, n, n, nb, r,
                               (const double *)jt, (const int32_t *)rotated);
            SE_LAUNCH_CHECK();
        }
    }

    // ascending eigenvalues: argsort of the diagonal on the host, gather on the device
    hipLaunchKernelGGL(eigh_diag_kernel, dim3((unsigned)((n + EIGH_THREADS - 1) / EIGH_THREADS)), dim3(EIGH_THREADS), 0, s,
                       (const double *)a, lda, n, diag);
    SE_LAUNCH_CHECK();
    std::vector<double> d((size_t)n);
    std::vector<int32_t> order((size_t)n);
    SE_HIP_CHECK(hipMemcpyAsync(d.data(), diag, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    SE_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        const double dx = d[(size_t)x], dy = d[(size_t)y];
        return dx < dy || (dy != dy && dx == dx);         // a NaN (non-converged overflow) sorts last
    });
    SE_HIP_CHECK(hipMemcpyAsync(perm, order.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(eigh_gather_kernel, dim3(rows_grid), dim3(EIGH_THREADS), 0, s, (const double *)diag, (const double *)vw, n,
                       (const int32_t *)perm, w, v, ldv);
    SE_LAUNCH_CHECK();
    SE_HIP_CHECK(hipMemcpyAsync(info, &code, sizeof(code), hipMemcpyHostToDevice, s));
    SE_HIP_CHECK(hipStreamSynchronize(s));
    return SE_OK;
}
