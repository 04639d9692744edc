// classemb.hip -- step 1 of the method on the device: class similarity tables from a hierarchy and the unit-sphere / spheres
// class embeddings (the Cholesky factor of a similarity or Gram matrix).
//
// Replaces compute_class_embedding.py's pairwise lcs_height loop (:212-216), ClassHierarchy.similarity_tables' double loop and the
// per-class np.linalg.solve of unitsphere_embedding (:14-40), whose result is exactly the lower Cholesky factor of S = 1 - D.
//
// * pair_tables_kernel (se_class_pair_tables): the host gives every node of the classes' ancestor closure a preference rank --
//   depth descending, height ascending, repr ascending, the order in which ClassHierarchy.lcs picks among common ancestors -- and
//   every class its ancestors (itself included) as a rank-sorted list with the host's shortest_path_length to each.  lcs(a, b) is
//   then the FIRST common entry of two sorted lists (a merge walk).  A 256-thread workgroup owns a 64 x 64 tile of pairs: the 64
//   row lists and the 64 column lists are staged in LDS position-major ([position][class], conflict-free for the column lists,
//   a broadcast for the row list a wave shares); thread t takes column t & 63 and every 4th row.  The tables are written with the
//   host's formulas in IEEE float64 (no reciprocal multiply, -ffp-contract=off): the same bits as similarity_tables.
// * se_cholesky_f64: right-looking blocked Cholesky, block column NB = 64.  Per block column: chol_diag_kernel factors the 64 x 64
//   diagonal block in LDS (one workgroup, two barriers per column), chol_panel_kernel solves the panel below it (one thread per row,
//   the row in registers, the diagonal block broadcast from LDS), chol_update_kernel subtracts L21 L21^T from the lower triangle of
//   the trailing matrix as 64 x 64 tiles on v_mfma_f64_16x16x4_f64 (4 waves x 2 x 2 16 x 16 blocks, K = 64 from LDS).  No host
//   synchronisation: a failed pivot is recorded in a device int32 by the diagonal kernel, and chol_finish_kernel turns the rows from
//   it onward into NaN the way the reference's sqrt of a negative does.
#include "se_common.h"

#include <math.h>

namespace se {

// ------------------------------------------------------------------------------------------------ pair tables

constexpr int PT_THREADS = 256;
constexpr int PT_TILE = 64;                 // classes per tile side
constexpr int PT_ROWS_PER_THREAD = PT_TILE * PT_TILE / PT_THREADS;

__global__ __launch_bounds__(PT_THREADS) void pair_tables_kernel(const int32_t *__restrict__ off, const int32_t *__restrict__ anc_rank,
                                                                 const int32_t *__restrict__ anc_spl, int64_t nnz, int64_t C, int max_anc,
                                                                 const int32_t *__restrict__ rdepth, const int32_t *__restrict__ rheight,
                                                                 int64_t n_ranks, int H, int flags, double *__restrict__ wup, int64_t ldw,
                                                                 double *__restrict__ lcs, int64_t ldl, unsigned long long *missing,
                                                                 int64_t tiles)
{
    extern __shared__ __attribute__((aligned(16))) int pt_raw[];
    // [2][max_anc][PT_TILE] ranks, then the same for spl, then [2][PT_TILE] list lengths (0: rows of the tile, 1: columns)
    int *s_rank = pt_raw;
    int *s_spl = s_rank + 2 * max_anc * PT_TILE;
    int *s_len = s_spl + 2 * max_anc * PT_TILE;
    const int tid = threadIdx.x;
    const int64_t ti = (int64_t)blockIdx.x / tiles, tj = (int64_t)blockIdx.x % tiles;
    const int64_t base[2] = {ti * PT_TILE, tj * PT_TILE};

    for (int s = 0; s < 2; s++) {
        for (int k = tid; k < PT_TILE; k += PT_THREADS) {
            const int64_t c = base[s] + k;
            int len = 0;
            if (c < C) {
                const int64_t b = off[c], e = off[c + 1];
                len = (int)(e - b);
                len = len < 0 ? 0 : (len > max_anc ? max_anc : len);
                if (b < 0 || b + len > nnz) len = 0;
            }
            s_len[s * PT_TILE + k] = len;
        }
    }
    wg_barrier();
    for (int s = 0; s < 2; s++) {
        for (int idx = tid; idx < max_anc * PT_TILE; idx += PT_THREADS) {
            const int k = idx / max_anc, p = idx % max_anc;     // consecutive threads walk one class's list (coalesced reads)
            const int64_t c = base[s] + k;
            if (p < s_len[s * PT_TILE + k]) {
                const int64_t g = off[c] + p;
                s_rank[(s * max_anc + p) * PT_TILE + k] = anc_rank[g];
                s_spl[(s * max_anc + p) * PT_TILE + k] = anc_spl[g];
            }
        }
    }
    wg_barrier();

    const int col = tid & (PT_TILE - 1);
    const int64_t j = base[1] + col;
    if (j >= C) return;
    const int lb = s_len[PT_TILE + col];
    const int *cr = s_rank + max_anc * PT_TILE + col, *cs = s_spl + max_anc * PT_TILE + col;
    const double Hd = (double)H;
    for (int m = 0; m < PT_ROWS_PER_THREAD; m++) {
        const int row = (tid >> 6) + 4 * m;
        const int64_t i = base[0] + row;
        if (i >= C) break;
        const int la = s_len[row];
        const int *ar = s_rank + row, *as = s_spl + row;
        int pa = 0, pb = 0, r = -1, spa = 0, spb = 0;
        while (pa < la && pb < lb) {
            const int x = ar[pa * PT_TILE], y = cr[pb * PT_TILE];
            if (x == y) {
                r = x;
                spa = as[pa * PT_TILE];
                spb = cs[pb * PT_TILE];
                break;
            }
            if (x < y) pa++;
            else pb++;
        }
        double w, l;
        if (r < 0 || r >= n_ranks) {
            const int64_t a = i < j ? i : j, b = i < j ? j : i;
            atomicMin(missing, (unsigned long long)(a * C + b));
            w = l = __longlong_as_double(0x7FF8000000000000LL);
        } else {
            const int ds = rdepth[r], h = rheight[r];
            w = (2.0 * (double)ds) / (double)((ds + spa) + (ds + spb));
            const double hr = (double)h / Hd;
            l = (flags & SE_CLASSEMB_DIST) ? hr : 1.0 - hr;
            if (i == j && (flags & SE_CLASSEMB_DIAG_ONE)) l = (flags & SE_CLASSEMB_DIST) ? 0.0 : 1.0;
        }
        if (wup) wup[i * ldw + j] = w;
        if (lcs) lcs[i * ldl + j] = l;
    }
}

// ------------------------------------------------------------------------------------------------ Cholesky

constexpr int CH_NB = 64;                   // block column
constexpr int CH_THREADS = 256;
constexpr int CH_LDT = CH_NB + 1;           // diagonal block in LDS: [64][65] doubles
constexpr int CH_LDU = CH_NB + 2;           // update operands in LDS: [64][66] doubles (conflict-free 16-row x 2-k half-wave reads)
constexpr int CH_PANEL_ROWS = 64;           // rows per panel workgroup (one thread each)

typedef double dbl4 __attribute__((ext_vector_type(4)));

// Strictly upper triangle -> 0; info -> -1.
__global__ __launch_bounds__(CH_THREADS) void chol_init_kernel(double *__restrict__ a, int64_t lda, int64_t n, int32_t *info)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *info = -1;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x)
        for (int64_t c = i + 1 + threadIdx.x; c < n; c += CH_THREADS) a[i * lda + c] = 0.0;
}

// Unblocked Cholesky of the nb x nb diagonal block at (k, k), in LDS.  The first pivot that is not > 0 (or NaN) is recorded.
__global__ __launch_bounds__(CH_THREADS) void chol_diag_kernel(double *__restrict__ a, int64_t lda, int64_t k, int nb, int32_t *info)
{
    __shared__ double t[CH_NB * CH_LDT];
    __shared__ int s_fail;
    const int tid = threadIdx.x;
    if (tid == 0) s_fail = -1;
    for (int idx = tid; idx < nb * nb; idx += CH_THREADS) {
        const int r = idx / nb, c = idx % nb;
        t[r * CH_LDT + c] = c <= r ? a[(k + r) * lda + k + c] : 0.0;
    }
    wg_barrier();
    for (int j = 0; j < nb; j++) {
        const double d = t[j * CH_LDT + j];
        if (tid == 0 && !(d > 0.0) && s_fail < 0) s_fail = j;
        const double piv = sqrt(d);
        // column j below the pivot (thread r owns row r)
        for (int r = j + 1 + tid; r < nb; r += CH_THREADS) t[r * CH_LDT + j] = t[r * CH_LDT + j] / piv;
        wg_barrier();
        if (tid == 0) t[j * CH_LDT + j] = piv;
        // rank-1 update of the trailing lower triangle of the block
        const int m = nb - j - 1;
        for (int idx = tid; idx < m * m; idx += CH_THREADS) {
            const int r = j + 1 + idx / m, c = j + 1 + idx % m;
            if (c <= r) t[r * CH_LDT + c] -= t[r * CH_LDT + j] * t[c * CH_LDT + j];
        }
        wg_barrier();
    }
    for (int idx = tid; idx < nb * nb; idx += CH_THREADS) {
        const int r = idx / nb, c = idx % nb;
        if (c <= r) a[(k + r) * lda + k + c] = t[r * CH_LDT + c];
    }
    if (tid == 0 && s_fail >= 0 && *info < 0) *info = (int32_t)(k + s_fail);
}

// L21 = A21 L11^-T for rows k + 64 .. n - 1: thread per row, the row in registers, L11 broadcast from LDS.
__global__ __launch_bounds__(CH_PANEL_ROWS) void chol_panel_kernel(double *__restrict__ a, int64_t lda, int64_t n, int64_t k)
{
    __shared__ double l11[CH_NB * CH_LDT];
    __shared__ double rows[CH_PANEL_ROWS * CH_LDT];
    const int tid = threadIdx.x;
    const int64_t r0 = k + CH_NB + (int64_t)blockIdx.x * CH_PANEL_ROWS;
    for (int idx = tid; idx < CH_NB * CH_NB; idx += CH_PANEL_ROWS) {
        const int r = idx / CH_NB, c = idx % CH_NB;
        l11[r * CH_LDT + c] = a[(k + r) * lda + k + c];
    }
    for (int idx = tid; idx < CH_PANEL_ROWS * CH_NB; idx += CH_PANEL_ROWS) {
        const int r = idx / CH_NB, c = idx % CH_NB;
        rows[r * CH_LDT + c] = r0 + r < n ? a[(r0 + r) * lda + k + c] : 0.0;
    }
    wg_barrier();
    double x[CH_NB];
#pragma unroll
    for (int j = 0; j < CH_NB; j++) {
        double s = rows[tid * CH_LDT + j];
#pragma unroll
        for (int p = 0; p < j; p++) s -= x[p] * l11[j * CH_LDT + p];
        x[j] = s / l11[j * CH_LDT + j];
    }
    if (r0 + tid < n) {
#pragma unroll
        for (int j = 0; j < CH_NB; j++) rows[tid * CH_LDT + j] = x[j];
    }
    wg_barrier();
    for (int idx = tid; idx < CH_PANEL_ROWS * CH_NB; idx += CH_PANEL_ROWS) {
        const int r = idx / CH_NB, c = idx % CH_NB;
        if (r0 + r < n) a[(r0 + r) * lda + k + c] = rows[r * CH_LDT + c];
    }
}

// A22 -= L21 L21^T on the lower triangle of the trailing matrix (rows / columns r0 .. n - 1), 64 x 64 tiles (ti >= tj).
__global__ __launch_bounds__(CH_THREADS) void chol_update_kernel(double *__restrict__ a, int64_t lda, int64_t n, int64_t k)
{
    __shared__ double li[CH_NB * CH_LDU];
    __shared__ double lj[CH_NB * CH_LDU];
    const int64_t r0 = k + CH_NB;
    // linear tile id -> (ti, tj), tj <= ti
    const int64_t id = blockIdx.x;
    int64_t ti = (int64_t)((sqrt(8.0 * (double)id + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > id) ti--;
    while ((ti + 1) * (ti + 2) / 2 <= id) ti++;
    const int64_t tj = id - ti * (ti + 1) / 2;
    const int64_t gi = r0 + ti * CH_NB, gj = r0 + tj * CH_NB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 64 rows x 64 doubles per operand, one row per wave-instruction (any lda: the caller's matrix may have an odd pitch)
    for (int idx = tid; idx < CH_NB * CH_NB; idx += CH_THREADS) {
        const int r = idx >> 6, c = idx & 63;
        li[r * CH_LDU + c] = gi + r < n ? a[(gi + r) * lda + k + c] : 0.0;
        lj[r * CH_LDU + c] = gj + r < n ? a[(gj + r) * lda + k + c] : 0.0;
    }
    wg_barrier();

    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    if (ti == tj && wc > wr) return;            // this wave's 32 x 32 block lies above the diagonal
    dbl4 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; bi++)
#pragma unroll
        for (int bj = 0; bj < 2; bj++) acc[bi][bj] = dbl4{0.0, 0.0, 0.0, 0.0};
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 4
    for (int ks = 0; ks < CH_NB; ks += 4) {
        // A[i][k] = L21[gi + i][k], B[k][j] = L21[gj + j][k]:  lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15]
        const double a0 = li[(wr + lr) * CH_LDU + ks + lk], a1 = li[(wr + 16 + lr) * CH_LDU + ks + lk];
        const double b0 = lj[(wc + lr) * CH_LDU + ks + lk], b1 = lj[(wc + 16 + lr) * CH_LDU + ks + lk];
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
                const int64_t R = gi + wr + 16 * bi + lk + 4 * e, Cc = gj + wc + 16 * bj + lr;
                if (R < n && Cc <= R) a[R * lda + Cc] -= acc[bi][bj][e];
            }
}

// After a failed pivot at row f: L[f][f] and rows f + 1 .. n - 1 (lower triangle) -> NaN.
__global__ __launch_bounds__(CH_THREADS) void chol_finish_kernel(double *__restrict__ a, int64_t lda, int64_t n, const int32_t *info)
{
    const int64_t f = *info;
    if (f < 0) return;
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    for (int64_t i = f + blockIdx.x; i < n; i += gridDim.x) {
        if (i == f) {
            if (threadIdx.x == 0) a[i * lda + i] = nan;
            continue;
        }
        for (int64_t c = threadIdx.x; c <= i; c += CH_THREADS) a[i * lda + c] = nan;
    }
}

constexpr int64_t CE_MAX_DIM = (int64_t)1 << 31;

}  // namespace se

using namespace se;

extern "C" int se_class_pair_tables(const int32_t *anc_off, const int32_t *anc_rank, const int32_t *anc_spl, int64_t nnz, int64_t c,
                                    int max_anc, const int32_t *rank_depth, const int32_t *rank_height, int64_t n_ranks, int max_height,
                                    int flags, double *wup, int64_t ldw, double *lcs, int64_t ldl, int64_t *missing, se_stream_t stream)
{
    const char *who = "se_class_pair_tables";
    if (c < 0 || c >= CE_MAX_DIM || nnz < 0 || n_ranks < 0 || n_ranks >= CE_MAX_DIM)
        return fail(SE_ERR_INVALID, "%s: bad shape c=%lld nnz=%lld ranks=%lld", who, (long long)c, (long long)nnz, (long long)n_ranks);
    if (flags & ~(SE_CLASSEMB_DIAG_ONE | SE_CLASSEMB_DIST)) return fail(SE_ERR_INVALID, "%s: unknown flags %d", who, flags);
    if (max_anc < 1 || max_anc > SE_CLASSEMB_MAX_ANC)
        return fail(SE_ERR_INVALID, "%s: max_anc=%d outside 1 .. %d", who, max_anc, SE_CLASSEMB_MAX_ANC);
    if (max_height < 1) return fail(SE_ERR_INVALID, "%s: max_height must be >= 1", who);
    if (!anc_off || !anc_rank || !anc_spl || !rank_depth || !rank_height || !missing || (!wup && !lcs))
        return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if ((wup && ldw < c) || (lcs && ldl < c)) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    hipStream_t s = (hipStream_t)stream;
    SE_HIP_CHECK(hipMemsetAsync(missing, 0xFF, sizeof(int64_t), s));
    if (c == 0) return SE_OK;
    const int64_t tiles = (c + PT_TILE - 1) / PT_TILE;
    if (tiles * tiles > 0x7FFFFFFF) return fail(SE_ERR_UNSUPPORTED, "%s: too many tiles", who);
    const size_t lds = (size_t)(4 * max_anc * PT_TILE + 2 * PT_TILE) * sizeof(int);
    hipLaunchKernelGGL(pair_tables_kernel, dim3((unsigned)(tiles * tiles)), dim3(PT_THREADS), lds, s, anc_off, anc_rank, anc_spl, nnz, c,
                       max_anc, rank_depth, rank_height, n_ranks, max_height, flags, wup, ldw, lcs, ldl,
                       reinterpret_cast<unsigned long long *>(missing), tiles);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_cholesky_f64(double *a, int64_t lda, int64_t n, int32_t *info, se_stream_t stream)
{
    const char *who = "se_cholesky_f64";
    if (n < 0 || n >= CE_MAX_DIM) return fail(SE_ERR_INVALID, "%s: bad size n=%lld", who, (long long)n);
    if (!info || (n > 0 && !a)) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (n > 0 && lda < n) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    hipStream_t s = (hipStream_t)stream;
    const unsigned rows_grid = (unsigned)(n < 1024 ? (n > 0 ? n : 1) : 1024);
    hipLaunchKernelGGL(chol_init_kernel, dim3(rows_grid), dim3(CH_THREADS), 0, s, a, lda, n, info);
    SE_LAUNCH_CHECK();
    for (int64_t k = 0; k < n; k += CH_NB) {
        const int nb = (int)(n - k < CH_NB ? n - k : CH_NB);
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(CH_THREADS), 0, s, a, lda, k, nb, info);
        SE_LAUNCH_CHECK();
        const int64_t m = n - k - nb;                   // trailing rows (nb == CH_NB whenever m > 0)
        if (m <= 0) break;
        hipLaunchKernelGGL(chol_panel_kernel, dim3((unsigned)((m + CH_PANEL_ROWS - 1) / CH_PANEL_ROWS)), dim3(CH_PANEL_ROWS), 0, s, a,
                           lda, n, k);
        SE_LAUNCH_CHECK();
        const int64_t t = (m + CH_NB - 1) / CH_NB;
        hipLaunchKernelGGL(chol_update_kernel, dim3((unsigned)(t * (t + 1) / 2)), dim3(CH_THREADS), 0, s, a, lda, n, k);
        SE_LAUNCH_CHECK();
    }
    if (n > 0) {
        hipLaunchKernelGGL(chol_finish_kernel, dim3(rows_grid), dim3(CH_THREADS), 0, s, a, lda, n, (const int32_t *)info);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}
