// svm.hip -- linear SVM (scikit-learn LinearSVC defaults: L2 penalty, squared hinge, one-vs-rest, regularised bias) on the device.
//
// Replaces the LinearSVC fit / decision_function of the reference's evaluate_classification_accuracy.py:20-48.  The solver
// (linear_svm.py) is liblinear's primal trust-region Newton method run for all classes at once; every O(N) step is one of two
// fp32 MFMA contractions over the features, the rest is O(C (D + 1)) vector algebra in this file:
//
// * svm_margin_kernel  (se_svm_margin): M = X [N, D] . W[:, :D]^T + W[:, D] on v_mfma_f32_32x32x2_f32 (128 x 128 tiles, 4 waves of
//   2 x 2 blocks of 32 x 32, K staged through LDS in chunks of 32 with a register prefetch of the next chunk).  The margins never
//   leave the registers: the epilogue (template mode) writes the scaled squared-hinge derivative Z, the active-set bit mask and
//   per-(64-row block, class) loss sums (gradient), the generalised Hessian's Z' = 2C A (X v + v_b) (Hessian-vector), or the
//   scores (decision_function).
// * svm_reduce_kernel  (se_svm_reduce): G = Z^T [X | 1] over fixed slices of at most SV_MAX_SLICE rows, fp32 partial tiles into the
//   caller's workspace, then svm_combine_kernel adds the partials of every element in slice order in fp64 (plus an optional
//   vector).  No atomics: the result is a function of the shapes and the data only, and the fp32 part of the round-off is bounded
//   by the slice length, not by N.
// * svm_gram_kernel / svm_rowsum_kernel / svm_axpby_kernel: per-class fp64 dot products, row sums and axpby of the solver's
//   [C, D + 1] vectors (one workgroup per class row, fixed reduction trees).
#include "se_common.h"

namespace se {

typedef float sv_f32x16 __attribute__((ext_vector_type(16)));

constexpr int SV_THREADS = 256;
constexpr int SV_BM = 128, SV_BN = 128, SV_BK = 32;
constexpr int SV_LD = SV_BK + 4;              // margin kernel: LDS row pitch (k inner; even k in [0, 16), odd k in [16, 32))
constexpr int SV_RP = SV_BM + 4;              // reduce kernel: LDS row pitch (tile columns inner)
constexpr int SV_LOSS_ROWS = 64;              // rows per loss partial sum
constexpr int64_t SV_MAX_SLICE = 4096;        // rows per fp32 partial of the reduction (bounds its round-off)
constexpr int64_t SV_MIN_SLICE = 256;
constexpr int64_t SV_TARGET_WGS = 2048;

__device__ __forceinline__ float sv_keep(float x, bool keep) { return __uint_as_float(__float_as_uint(x) & (keep ? 0xFFFFFFFFu : 0u)); }

// Global -> registers for the margin kernel: rows [row0, row0 + 128) x k [k0, k0 + 32) of a row-major matrix, 8 threads per row,
// float4 per thread, 4 passes.  Addresses are clamped into the valid rows / k (the values are masked when stored).
template <bool VEC>
__device__ __forceinline__ void sv_load_k(float4 (&v)[4], const float *__restrict__ src, int64_t ld, int64_t row0, int64_t nrows,
                                          int64_t k0, int64_t kend)
{
    const int tid = threadIdx.x, r0 = tid >> 3, kq = (tid & 7) * 4;
#pragma unroll
    for (int it = 0; it < 4; it++) {
        int64_t r = row0 + it * 32 + r0;
        r = r < nrows ? r : nrows - 1;
        const float *row = src + r * ld;
        if (VEC) {   // ld % 4 == 0, kend % 4 == 0, 16-byte aligned base
            int64_t k = k0 + kq;
            k = k + 4 <= kend ? k : kend - 4;
            v[it] = *(const float4 *)(row + k);
        } else {
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t k = k0 + kq + j;
                e[j] = row[k < kend ? k : kend - 1];
            }
            v[it] = make_float4(e[0], e[1], e[2], e[3]);
        }
    }
}

__device__ __forceinline__ void sv_store_k(float *lds, const float4 (&v)[4], int64_t row0, int64_t nrows, int64_t k0, int64_t kend)
{
    const int tid = threadIdx.x, r0 = tid >> 3, kq = (tid & 7) * 4;
    const int64_t nk = kend - k0 - kq;
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const bool rok = row0 + it * 32 + r0 < nrows;
        float *o = lds + (it * 32 + r0) * SV_LD + (kq >> 1);
        *(float2 *)o = make_float2(sv_keep(v[it].x, rok && nk > 0), sv_keep(v[it].z, rok && nk > 2));
        *(float2 *)(o + SV_BK / 2) = make_float2(sv_keep(v[it].y, rok && nk > 1), sv_keep(v[it].w, rok && nk > 3));
    }
}

template <int MODE, bool VX, bool VW>
__global__ __launch_bounds__(SV_THREADS) void svm_margin_kernel(const float *__restrict__ x, int64_t ldx, int64_t N, int64_t D,
                                                                 const float *__restrict__ w, int64_t ldw, int64_t C,
                                                                 const int32_t *__restrict__ labels, const int32_t *__restrict__ col_class,
                                                                 float cpen, uint32_t *__restrict__ mask, int64_t ldm,
                                                                 float *__restrict__ out, int64_t ldo, float *__restrict__ loss_part,
                                                                 int64_t ldl, int64_t tiles_n)
{
    __shared__ __attribute__((aligned(16))) float sA[SV_BM * SV_LD];
    __shared__ __attribute__((aligned(16))) float sB[SV_BN * SV_LD];
    const int64_t m0 = (int64_t)(blockIdx.x / tiles_n) * SV_BM, n0 = (int64_t)(blockIdx.x % tiles_n) * SV_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, col = lane & 31, hi = lane >> 5;

    sv_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    float4 va[4], vb[4];
    sv_load_k<VX>(va, x, ldx, m0, N, 0, D);
    sv_load_k<VW>(vb, w, ldw, n0, C, 0, D);
    const float *pa = sA + (wm * 64 + col) * SV_LD + hi * (SV_BK / 2);
    const float *pb = sB + (wn * 64 + col) * SV_LD + hi * (SV_BK / 2);
    for (int64_t k0 = 0; k0 < D; k0 += SV_BK) {
        wg_barrier();                                  // every wave is done reading the previous chunk
        sv_store_k(sA, va, m0, N, k0, D);
        sv_store_k(sB, vb, n0, C, k0, D);
        wg_barrier();
        if (k0 + SV_BK < D) {                          // next chunk in flight during the MFMAs
            sv_load_k<VX>(va, x, ldx, m0, N, k0 + SV_BK, D);
            sv_load_k<VW>(vb, w, ldw, n0, C, k0 + SV_BK, D);
        }
#pragma unroll
        for (int s = 0; s < SV_BK / 2; s += 4) {
            const float4 a0 = *(const float4 *)(pa + s), a1 = *(const float4 *)(pa + 32 * SV_LD + s);
            const float4 b0 = *(const float4 *)(pb + s), b1 = *(const float4 *)(pb + 32 * SV_LD + s);
#define SV_MF(F)                                                                         \
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b0.F, acc[0][0], 0, 0, 0);    \
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b1.F, acc[0][1], 0, 0, 0);    \
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b0.F, acc[1][0], 0, 0, 0);    \
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b1.F, acc[1][1], 0, 0, 0);
            SV_MF(x) SV_MF(y) SV_MF(z) SV_MF(w)
#undef SV_MF
        }
    }

    // ---- epilogue: lane (col, hi) of wave (wm, wn) holds, per block (bi, bj), rows m0 + wm*64 + bi*32 + (r & 3) + 8 (r >> 2) + 4 hi
    //      of column n0 + wn*64 + bj*32 + col ----
#pragma unroll
    for (int bj = 0; bj < 2; bj++) {
        const int64_t cb = n0 + wn * 64 + bj * 32;     // first column of the 32-column block (a multiple of 32: one mask word)
        const int64_t c = cb + col;
        const bool cok = c < C;
        const int64_t cc = cok ? c : C - 1;
        const float bias = w[cc * ldw + D];
        const int cls = (MODE == SE_SVM_GRAD && cok) ? col_class[cc] : -1;
        float lsum = 0.f;
#pragma unroll
        for (int bi = 0; bi < 2; bi++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int64_t i = m0 + wm * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const bool ok = cok && i < N;
                const float m = acc[bi][bj][r] + bias;
                if (MODE == SE_SVM_SCORE) {
                    if (ok) out[i * ldo + c] = m;
                } else if (MODE == SE_SVM_GRAD) {
                    const int lab = i < N ? labels[i] : -2;
                    const float y = lab == cls ? 1.f : -1.f;
                    const float t = 1.f - y * m;
                    const bool viol = ok && t > 0.f;
                    if (ok) out[i * ldo + c] = viol ? -2.f * cpen * y * t : 0.f;
                    lsum += viol ? t * t : 0.f;
                    const uint64_t bits = __ballot(viol);
                    if (col == 0 && i < N && cb < C) mask[i * ldm + (cb >> 5)] = (uint32_t)(bits >> (32 * hi));
                } else {   // SE_SVM_HV
                    const uint32_t word = (i < N && cb < C) ? mask[i * ldm + (cb >> 5)] : 0u;   // blocks past column c own no word
                    const bool act = ok && ((word >> col) & 1u);
                    if (ok) out[i * ldo + c] = act ? 2.f * cpen * m : 0.f;
                }
            }
        }
        if (MODE == SE_SVM_GRAD) {
            lsum += __shfl_xor(lsum, 32, 64);          // the two row halves of the column (a + b == b + a: both lanes agree)
            if (hi == 0 && cok) {
                const int64_t blk = (m0 + wm * 64) / SV_LOSS_ROWS;
                if (blk * SV_LOSS_ROWS < N) loss_part[c * ldl + blk] = lsum;
            }
        }
    }
}

// Reduce kernel: partial [C, D + 1] tile of slice s = sum over the slice's rows i of Z[i, c] * Xa[i, k], Xa = [X | 1].
// Tile rows = classes (128), tile columns = features (128), K = rows of X in chunks of 32; both operands are row-major along the
// tile's M / N index, staged as [k][m] in LDS (32 rows of one chunk, 8 threads x float4 per 32 tile columns).
template <bool VEC, bool ONES>
__device__ __forceinline__ void sv_load_m(float4 (&v)[4], const float *__restrict__ src, int64_t ld, int64_t i0, int64_t iend,
                                          int64_t c0, int64_t cend)
{
    const int tid = threadIdx.x, r0 = tid >> 5, cq = (tid & 31) * 4;
#pragma unroll
    for (int it = 0; it < 4; it++) {
        int64_t i = i0 + it * 8 + r0;
        i = i < iend ? i : iend - 1;
        const float *row = src + i * ld;
        if (VEC) {
            int64_t c = c0 + cq;
            c = c + 4 <= cend ? c : cend - 4;
            v[it] = *(const float4 *)(row + c);
        } else {
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t c = c0 + cq + j;
                e[j] = row[c < cend ? c : cend - 1];
            }
            v[it] = make_float4(e[0], e[1], e[2], e[3]);
        }
    }
}

template <bool ONES>
__device__ __forceinline__ void sv_store_m(float *lds, const float4 (&v)[4], int64_t i0, int64_t iend, int64_t c0, int64_t cend)
{
    const int tid = threadIdx.x, r0 = tid >> 5, cq = (tid & 31) * 4;
    const int64_t nc = cend - c0 - cq;         // valid columns from this thread's first one
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const bool rok = i0 + it * 8 + r0 < iend;
        float4 o;
        o.x = sv_keep(v[it].x, rok && nc > 0);
        o.y = sv_keep(v[it].y, rok && nc > 1);
        o.z = sv_keep(v[it].z, rok && nc > 2);
        o.w = sv_keep(v[it].w, rok && nc > 3);
        if (ONES) {                                // column D of [X | 1]
            o.x = (rok && nc == 0) ? 1.f : o.x;
            o.y = (rok && nc == 1) ? 1.f : o.y;
            o.z = (rok && nc == 2) ? 1.f : o.z;
            o.w = (rok && nc == 3) ? 1.f : o.w;
        }
        *(float4 *)(lds + (it * 8 + r0) * SV_RP + cq) = o;
    }
}

template <bool VZ, bool VX>
__global__ __launch_bounds__(SV_THREADS) void svm_reduce_kernel(const float *__restrict__ z, int64_t ldz, const float *__restrict__ x,
                                                                 int64_t ldx, int64_t N, int64_t D, int64_t C, int64_t slice,
                                                                 int64_t tiles_m, int64_t tiles_n, float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float sZ[SV_BK * SV_RP];
    __shared__ __attribute__((aligned(16))) float sX[SV_BK * SV_RP];
    const int64_t tiles = tiles_m * tiles_n;
    const int64_t s = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int64_t c0 = (t / tiles_n) * SV_BM, k0 = (t % tiles_n) * SV_BN;
    const int64_t ibeg = s * slice, iend = (ibeg + slice < N) ? ibeg + slice : N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, col = lane & 31, hi = lane >> 5;

    sv_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    float4 vz[4], vx[4];
    sv_load_m<VZ, false>(vz, z, ldz, ibeg, iend, c0, C);
    sv_load_m<VX, true>(vx, x, ldx, ibeg, iend, k0, D);
    const float *pa = sZ + hi * SV_RP + wm * 64 + col;
    const float *pb = sX + hi * SV_RP + wn * 64 + col;
    for (int64_t i0 = ibeg; i0 < iend; i0 += SV_BK) {
        wg_barrier();
        sv_store_m<false>(sZ, vz, i0, iend, c0, C);
        sv_store_m<true>(sX, vx, i0, iend, k0, D);
        wg_barrier();
        if (i0 + SV_BK < iend) {
            sv_load_m<VZ, false>(vz, z, ldz, i0 + SV_BK, iend, c0, C);
            sv_load_m<VX, true>(vx, x, ldx, i0 + SV_BK, iend, k0, D);
        }
#pragma unroll
        for (int st = 0; st < SV_BK / 2; st++) {
            const float a0 = pa[2 * st * SV_RP], a1 = pa[2 * st * SV_RP + 32];
            const float b0 = pb[2 * st * SV_RP], b1 = pb[2 * st * SV_RP + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // partial tile -> part[s][c][k], k in [0, D]
    float *ps = part + s * C * (D + 1);
#pragma unroll
    for (int bj = 0; bj < 2; bj++) {
        const int64_t k = k0 + wn * 64 + bj * 32 + col;
#pragma unroll
        for (int bi = 0; bi < 2; bi++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int64_t c = c0 + wm * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (c < C && k <= D) ps[c * (D + 1) + k] = acc[bi][bj][r];
            }
    }
}

// Fixed-order block sum of one double per thread (a binary tree in LDS); the result is in every thread.
__device__ __forceinline__ double sv_block_sum(double v, double *sred)
{
    const int tid = threadIdx.x;
    wg_barrier();                                      // sred is free (a previous call's readers are done)
    sred[tid] = v;
    wg_barrier();
#pragma unroll
    for (int o = SV_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sred[tid] += sred[tid + o];
        wg_barrier();
    }
    return sred[0];
}

// out[c, k] = (float)(plus[c, k] + sum_s part[s][c][k])  -- the sum over s in ascending order in fp64; one workgroup per class
__global__ __launch_bounds__(SV_THREADS) void svm_combine_kernel(const float *__restrict__ part, int64_t S, int64_t C, int64_t D,
                                                                  const float *__restrict__ plus, int64_t ldp, float *__restrict__ g,
                                                                  int64_t ldg)
{
    const int64_t c = blockIdx.x;
    for (int64_t k = threadIdx.x; k <= D; k += SV_THREADS) {
        double sum = 0.0;
        for (int64_t s = 0; s < S; s++) sum += (double)part[(s * C + c) * (D + 1) + k];
        if (plus) sum += (double)plus[c * ldp + k];
        g[c * ldg + k] = (float)sum;
    }
}

// out[c, p] = sum_k V_a[c, k] V_b[c, k] in fp64 for the pairs a <= b of nv vectors (row-major upper triangle)
struct SvVecs { const float *v[4]; };
__global__ __launch_bounds__(SV_THREADS) void svm_gram_kernel(SvVecs vs, int nv, int64_t ld, int64_t len, double *__restrict__ out)
{
    __shared__ double sred[SV_THREADS];
    const int64_t c = blockIdx.x;
    const int np = nv * (nv + 1) / 2;
    double acc[10];
#pragma unroll
    for (int p = 0; p < 10; p++) acc[p] = 0.0;
    for (int64_t k = threadIdx.x; k < len; k += SV_THREADS) {
        double e[4];
#pragma unroll
        for (int a = 0; a < 4; a++) e[a] = a < nv ? (double)vs.v[a][c * ld + k] : 0.0;
        int p = 0;
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = a; b < 4; b++) {
                if (a < nv && b < nv) acc[p] += e[a] * e[b];
                p += (a < nv && b < nv) ? 1 : 0;
            }
    }
    for (int p = 0; p < np; p++) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 10; q++) v = q == p ? acc[q] : v;
        v = sv_block_sum(v, sred);
        if (threadIdx.x == 0) out[c * np + p] = v;
    }
}

__global__ __launch_bounds__(SV_THREADS) void svm_rowsum_kernel(const float *__restrict__ a, int64_t lda, int64_t len, double *__restrict__ out)
{
    __shared__ double sred[SV_THREADS];
    const int64_t c = blockIdx.x;
    double v = 0.0;
    for (int64_t k = threadIdx.x; k < len; k += SV_THREADS) v += (double)a[c * lda + k];
    v = sv_block_sum(v, sred);
    if (threadIdx.x == 0) out[c] = v;
}

__global__ __launch_bounds__(SV_THREADS) void svm_axpby_kernel(const double *__restrict__ alpha, const float *__restrict__ x, int64_t ldx,
                                                                const double *__restrict__ beta, const float *__restrict__ y, int64_t ldy,
                                                                int64_t C, int64_t len, float *__restrict__ out, int64_t ldo)
{
    const int64_t total = C * len;
    for (int64_t e = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * SV_THREADS) {
        const int64_t c = e / len, k = e % len;
        const double v = alpha[c] * (double)x[c * ldx + k] + beta[c] * (double)y[c * ldy + k];
        out[c * ldo + k] = (float)v;
    }
}

static bool sv_aligned(const void *p, int64_t ld, int64_t cols)
{
    return (reinterpret_cast<uintptr_t>(p) % 16 == 0) && ld % 4 == 0 && cols % 4 == 0 && cols >= 4;
}

static int64_t sv_slice(int64_t n, int64_t d, int64_t c)
{
    const int64_t tiles = ((c + SV_BM - 1) / SV_BM) * ((d + 1 + SV_BN - 1) / SV_BN);
    const int64_t want = (SV_TARGET_WGS + tiles - 1) / tiles;
    int64_t sl = (n + want - 1) / want;
    sl = (sl + SV_BK - 1) / SV_BK * SV_BK;
    return sl < SV_MIN_SLICE ? SV_MIN_SLICE : (sl > SV_MAX_SLICE ? SV_MAX_SLICE : sl);
}

constexpr int64_t SV_MAX_DIM = (int64_t)1 << 40;

}  // namespace se

using namespace se;

extern "C" int64_t se_svm_loss_blocks(int64_t n) { return n <= 0 ? 0 : (n + SV_LOSS_ROWS - 1) / SV_LOSS_ROWS; }

extern "C" int se_svm_margin(int mode, const float *x, int64_t ldx, int64_t n, int64_t d, const float *w, int64_t ldw, int64_t c,
                             const int32_t *labels, const int32_t *col_class, float cpen, uint32_t *mask, int64_t ldm, float *out,
                             int64_t ldo, float *loss_part, int64_t ldl, se_stream_t stream)
{
    const char *who = "se_svm_margin";
    if (mode != SE_SVM_GRAD && mode != SE_SVM_HV && mode != SE_SVM_SCORE) return fail(SE_ERR_INVALID, "%s: unknown mode %d", who, mode);
    if (n < 1 || d < 1 || c < 3 || n > SV_MAX_DIM || d > SV_MAX_DIM || c > SV_MAX_DIM)
        return fail(SE_ERR_INVALID, "%s: bad shape n=%lld d=%lld c=%lld (n >= 1, d >= 1, c >= 3)", who, (long long)n, (long long)d, (long long)c);
    if (!x || !w || !out) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (ldx < d || ldw < d + 1 || ldo < c) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    const int64_t words = (c + 31) / 32;
    if (mode != SE_SVM_SCORE) {
        if (!mask) return fail(SE_ERR_INVALID, "%s: null mask", who);
        if (ldm < words) return fail(SE_ERR_INVALID, "%s: mask leading dimension %lld < %lld words", who, (long long)ldm, (long long)words);
        if (!(cpen > 0.f) || cpen > 3.0e38f) return fail(SE_ERR_INVALID, "%s: C must be positive and finite", who);
    }
    if (mode == SE_SVM_GRAD) {
        if (!labels || !col_class || !loss_part) return fail(SE_ERR_INVALID, "%s: null pointer", who);
        if (ldl < se_svm_loss_blocks(n)) return fail(SE_ERR_INVALID, "%s: loss leading dimension too small", who);
    }
    const int64_t tiles_m = (n + SV_BM - 1) / SV_BM, tiles_n = (c + SV_BN - 1) / SV_BN;
    if (tiles_m * tiles_n > 0x7FFFFFFF) return fail(SE_ERR_UNSUPPORTED, "%s: too many tiles", who);
    const bool vx = sv_aligned(x, ldx, d), vw = sv_aligned(w, ldw, d);
    hipStream_t s = (hipStream_t)stream;
#define SV_M(MODE, VX, VW)                                                                                                          \
    hipLaunchKernelGGL((svm_margin_kernel<MODE, VX, VW>), dim3((unsigned)(tiles_m * tiles_n)), dim3(SV_THREADS), 0, s, x, ldx, n, d, w, \
                       ldw, c, labels, col_class, cpen, mask, ldm, out, ldo, loss_part, ldl, tiles_n)
#define SV_MV(MODE) \
    if (vx && vw) SV_M(MODE, true, true); else if (vx) SV_M(MODE, true, false); else if (vw) SV_M(MODE, false, true); else SV_M(MODE, false, false);
    if (mode == SE_SVM_GRAD) { SV_MV(SE_SVM_GRAD) }
    else if (mode == SE_SVM_HV) { SV_MV(SE_SVM_HV) }
    else { SV_MV(SE_SVM_SCORE) }
#undef SV_MV
#undef SV_M
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int64_t se_svm_reduce_workspace_bytes(int64_t n, int64_t d, int64_t c)
{
    if (n < 1 || d < 1 || c < 1 || n > SV_MAX_DIM || d > SV_MAX_DIM || c > SV_MAX_DIM) return 0;
    const int64_t sl = sv_slice(n, d, c);
    return (n + sl - 1) / sl * c * (d + 1) * (int64_t)sizeof(float);
}

extern "C" int se_svm_reduce(const float *z, int64_t ldz, const float *x, int64_t ldx, int64_t n, int64_t d, int64_t c, const float *plus,
                             int64_t ldp, float *g, int64_t ldg, void *workspace, int64_t workspace_bytes, se_stream_t stream)
{
    const char *who = "se_svm_reduce";
    if (n < 1 || d < 1 || c < 3 || n > SV_MAX_DIM || d > SV_MAX_DIM || c > SV_MAX_DIM)
        return fail(SE_ERR_INVALID, "%s: bad shape n=%lld d=%lld c=%lld (n >= 1, d >= 1, c >= 3)", who, (long long)n, (long long)d, (long long)c);
    if (!z || !x || !g || !workspace) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (ldz < c || ldx < d || ldg < d + 1 || (plus && ldp < d + 1)) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    const int64_t need = se_svm_reduce_workspace_bytes(n, d, c);
    if (workspace_bytes < need)
        return fail(SE_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(SE_ERR_INVALID, "%s: workspace must be 16-byte aligned", who);
    const int64_t sl = sv_slice(n, d, c), S = (n + sl - 1) / sl;
    const int64_t tiles_m = (c + SV_BM - 1) / SV_BM, tiles_n = (d + 1 + SV_BN - 1) / SV_BN;
    if (S * tiles_m * tiles_n > 0x7FFFFFFF || c > 0x7FFFFFFF) return fail(SE_ERR_UNSUPPORTED, "%s: too many tiles", who);
    // [X | 1] has d + 1 columns: the float4 path needs d % 4 == 0 (the ones column is synthesised, never read)
    const bool vz = sv_aligned(z, ldz, c), vx = sv_aligned(x, ldx, d);
    float *part = (float *)workspace;
    hipStream_t s = (hipStream_t)stream;
#define SV_R(VZ, VX)                                                                                                                 \
    hipLaunchKernelGGL((svm_reduce_kernel<VZ, VX>), dim3((unsigned)(S * tiles_m * tiles_n)), dim3(SV_THREADS), 0, s, z, ldz, x, ldx, n, d, \
                       c, sl, tiles_m, tiles_n, part)
    if (vz && vx) SV_R(true, true); else if (vz) SV_R(true, false); else if (vx) SV_R(false, true); else SV_R(false, false);
#undef SV_R
    SE_LAUNCH_CHECK();
    hipLaunchKernelGGL(svm_combine_kernel, dim3((unsigned)c), dim3(SV_THREADS), 0, s, part, S, c, d, plus, ldp, g, ldg);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_svm_gram(const float *v0, const float *v1, const float *v2, const float *v3, int nv, int64_t ld, int64_t c, int64_t len,
                           double *out, se_stream_t stream)
{
    const char *who = "se_svm_gram";
    if (nv < 1 || nv > 4 || c < 1 || len < 1 || c > 0x7FFFFFFF || len > SV_MAX_DIM)
        return fail(SE_ERR_INVALID, "%s: bad shape nv=%d c=%lld len=%lld", who, nv, (long long)c, (long long)len);
    if (ld < len) return fail(SE_ERR_INVALID, "%s: leading dimension too small", who);
    SvVecs vs{{v0, v1, v2, v3}};
    for (int a = 0; a < nv; a++)
        if (!vs.v[a]) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    if (!out) return fail(SE_ERR_INVALID, "%s: null pointer", who);
    hipLaunchKernelGGL(svm_gram_kernel, dim3((unsigned)c), dim3(SV_THREADS), 0, (hipStream_t)stream, vs, nv, ld, len, out);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_svm_rowsum(const float *a, int64_t lda, int64_t c, int64_t len, double *out, se_stream_t stream)
{
    if (c < 1 || len < 1 || c > 0x7FFFFFFF || len > SV_MAX_DIM)
        return fail(SE_ERR_INVALID, "se_svm_rowsum: bad shape c=%lld len=%lld", (long long)c, (long long)len);
    if (!a || !out) return fail(SE_ERR_INVALID, "se_svm_rowsum: null pointer");
    if (lda < len) return fail(SE_ERR_INVALID, "se_svm_rowsum: leading dimension too small");
    hipLaunchKernelGGL(svm_rowsum_kernel, dim3((unsigned)c), dim3(SV_THREADS), 0, (hipStream_t)stream, a, lda, len, out);
    SE_LAUNCH_CHECK();
    return SE_OK;
}

extern "C" int se_svm_axpby(const double *alpha, const float *x, int64_t ldx, const double *beta, const float *y, int64_t ldy, int64_t c,
                            int64_t len, float *out, int64_t ldo, se_stream_t stream)
{
    if (c < 1 || len < 1 || c > SV_MAX_DIM || len > SV_MAX_DIM)
        return fail(SE_ERR_INVALID, "se_svm_axpby: bad shape c=%lld len=%lld", (long long)c, (long long)len);
    if (!alpha || !x || !beta || !y || !out) return fail(SE_ERR_INVALID, "se_svm_axpby: null pointer");
    if (ldx < len || ldy < len || ldo < len) return fail(SE_ERR_INVALID, "se_svm_axpby: leading dimension too small");
    const int64_t blocks = (c * len + SV_THREADS - 1) / SV_THREADS;
    hipLaunchKernelGGL(svm_axpby_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(SV_THREADS), 0, (hipStream_t)stream, alpha,
                       x, ldx, beta, y, ldy, c, len, out, ldo);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
