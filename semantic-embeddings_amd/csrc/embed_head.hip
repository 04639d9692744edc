// embed_head.hip -- the two embedding heads the reference trains with, loss AND nearest-class metric in one forward launch
// (reference: utils.py:44-46 / :34-36 for the loss, utils.py:57-100 for the metric).
//
//   se_embed_head_fwd(mode 0) : what se_cosine_loss_fwd writes  +  what se_nn_accuracy(dot_prod_sim = 1) computes from that xhat
//   se_embed_head_fwd(mode 1) : what se_sqdist_loss_fwd writes  +  what se_nn_accuracy(dot_prod_sim = 0) computes from float32(x)
//
// bit for bit, with the metric delivered as its two counts (n_better, n_within) so that every k is read off one contraction.
//
// Layout: a workgroup of four waves owns a strip of 32 samples and a slice of the class tiles.
//   1. loss:   each wave reduces 8 of the strip's rows with the per-lane FMA chains and the wave tree of loss_kernels.hip (its own
//              copy: the kernels there stay as they are).  The cosine head keeps the 32 inverse norms in LDS; the normalised
//              features themselves are never read back: every operand chunk of the contraction is rebuilt from x as x * inv_norm,
//              the very product xhat holds, while it is staged.  xhat goes to global memory only when the caller asks for it.
//   2. true:   the label's score per sample, with the arithmetic of the class-tile loop (k-ascending FMA chain; |e|^2 as even + odd
//              sum), on operands staged through LDS with coalesced loads -- the sibling walks two global rows per lane here.
//   3. tiles:  the four waves take four class tiles at a time on v_mfma_f32_32x32x2_f32, sharing ONE staged feature chunk; each wave
//              stages its own class chunk.  Counts and the best class meet in LDS (integer atomics), and, when the class set is cut
//              into slices, in the workspace; the last slice of a strip to finish writes the strip's results (ticket counter).
// No floating-point atomics; counts are integer sums and the best class is an ordered-word maximum, so the result does not depend
// on the launch geometry or on the order in which workgroups finish.
#include "se_common.h"
#include "tile32.h"

namespace se {
namespace head {

using tile32::f32x16;

constexpr int THREADS = 256, WAVES = 4;
constexpr int ROWS_PER_WAVE = 32 / WAVES;
constexpr int BK = tile32::BK, LD = tile32::LD;
constexpr float L2NORM_EPS = 1e-12f;    // tf.nn.l2_normalize default epsilon (TF 1.x), as in loss_kernels.hip
constexpr int NO_CLASS = 0x7FFFFFFF;

// ss = sum x^2, dt = sum x * t over one row: the lane partition, FMA order and wave tree of loss_kernels.hip's row_reduce
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

// sum (x - t)^2 over one row, as sqdist_loss_fwd_kernel forms it
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

// The strip's feature chunk (32 rows x 64 k) -> LDS by all 256 threads, two (row, 4 consecutive k) items each: the cosine head
// scales every element by its row's inverse norm (the product xhat holds), the distance head widens it.  Loads are unconditional
// (tile32.h): out-of-range items read row0 / k = 0 and are zeroed afterwards.
template <int MODE, bool BF16>
__device__ __forceinline__ void stage_x(float *lds, const void *x, int64_t ldx, int64_t row0, int64_t B, int64_t k0, int64_t D, bool vec,
                                        const float *sInv)
{
    float v[2][4];
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int idx = it * THREADS + (int)threadIdx.x;
        const int r = idx >> 4, kq = (idx & 15) * 4;
        const bool rok = row0 + r < B;
        const char *p = (const char *)x + (rok ? row0 + r : row0) * ldx * (BF16 ? 2 : 4);
        const int64_t kk = k0 + kq;
        bool ok[4];
        if (vec) {
            const int64_t base = kk < D ? kk : 0;
            if constexpr (BF16) {
                const uint2 w = *(const uint2 *)(p + base * 2);
                v[it][0] = __uint_as_float(w.x << 16); v[it][1] = __uint_as_float(w.x & 0xFFFF0000u);
                v[it][2] = __uint_as_float(w.y << 16); v[it][3] = __uint_as_float(w.y & 0xFFFF0000u);
            } else {
                const float4 t = *(const float4 *)(p + base * 4);
                v[it][0] = t.x; v[it][1] = t.y; v[it][2] = t.z; v[it][3] = t.w;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) ok[j] = rok && kk < D;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool kok = kk + j < D;
                v[it][j] = ld_elem<BF16>(p, kok ? kk + j : 0);
                ok[j] = rok && kok;
            }
        }
        const float inv = MODE == 0 ? sInv[r] : 1.f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (MODE == 0) v[it][j] = v[it][j] * inv;
            v[it][j] = ok[j] ? v[it][j] : 0.f;
        }
    }
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int idx = it * THREADS + (int)threadIdx.x;
        tile32::put<BK>(lds, idx >> 4, (idx & 15) * 4, v[it]);
    }
}

// the label rows emb[y[r]] of the strip, same chunk, same layout, by all 256 threads (rows outside the batch: zero)
__device__ __forceinline__ void stage_label_rows(float *lds, const float *emb, int64_t lde, const int *sY, int64_t k0, int64_t D, bool vec)
{
    float v[2][4];
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int idx = it * THREADS + (int)threadIdx.x;
        const int r = idx >> 4, kq = (idx & 15) * 4;
        const int y = sY[r];
        const bool rok = y >= 0;
        const float *p = emb + (int64_t)(rok ? y : 0) * lde;
        const int64_t kk = k0 + kq;
        if (vec) {
            const bool ok = rok && kk < D;
            const float4 t = *(const float4 *)(p + (kk < D ? kk : 0));
            v[it][0] = ok ? t.x : 0.f; v[it][1] = ok ? t.y : 0.f; v[it][2] = ok ? t.z : 0.f; v[it][3] = ok ? t.w : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool kok = kk + j < D;
                const float t = p[kok ? kk + j : 0];
                v[it][j] = (rok && kok) ? t : 0.f;
            }
        }
    }
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const int idx = it * THREADS + (int)threadIdx.x;
        tile32::put<BK>(lds, idx >> 4, (idx & 15) * 4, v[it]);
    }
}

// element k of a staged row (even k in [0, 32), odd k in [32, 64))
__device__ __forceinline__ float staged(const float *row, int k) { return row[(k & 1) * (BK / 2) + (k >> 1)]; }

// best class of a set as one ordered word: score (larger word = better), then the LOWER class index (nn_accuracy_kernel's word)
template <int MODE>
__device__ __forceinline__ unsigned long long best_word(float v, int c)
{
    if (v == 0.f) v = 0.f;                                     // -0 ties with +0
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);            // ascending with the value
    if (MODE == 1) u = ~u;                                     // distances: smaller is better
    return ((unsigned long long)u << 32) | (uint32_t)(NO_CLASS - c);
}

template <int MODE, bool BF16>
__global__ __launch_bounds__(THREADS) void embed_head_kernel(
    const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels, const float *__restrict__ emb, int64_t lde,
    int64_t B, int64_t D, int64_t C, float *__restrict__ xhat, int64_t ldxhat, float *__restrict__ inv_norm, float *__restrict__ loss_i,
    float *__restrict__ dist_i, int32_t *__restrict__ n_better_out, int32_t *__restrict__ n_within_out, int32_t *__restrict__ best_out,
    float *__restrict__ scores, int64_t lds_, int loss_vec, int x_vec, int e_vec, int tiles_per_block,
    unsigned long long *__restrict__ part_best, uint32_t *__restrict__ part_cnt, uint32_t *__restrict__ ticket)
{
    // grid = (32-sample strips, class slices of tiles_per_block x 32 classes)
    __shared__ __attribute__((aligned(16))) float sA[32 * LD];
    __shared__ __attribute__((aligned(16))) float sB[WAVES][32 * LD];
    __shared__ float sInv[32], sTrue[32], sPn[32], sDot[32], sEn[32];
    __shared__ int sY[32];
    __shared__ int sCnt[64];
    __shared__ unsigned long long sBest[32];
    __shared__ int sLast;

    const int tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
    const int col = lane & 31, hi = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * 32;
    const bool first_slice = blockIdx.y == 0;

    if (tid < 32) {
        sY[tid] = row0 + tid < B ? (int)clamp_label(labels[row0 + tid], C) : -1;
        sCnt[2 * tid] = 0; sCnt[2 * tid + 1] = 0;
        sBest[tid] = 0ull;
        sPn[tid] = 0.f; sEn[tid] = 0.f;
    }

    // ---- 1. the loss of the strip's rows (written by the first class slice; every slice of the cosine head needs the inverse norms)
    if (MODE == 0 || first_slice) {
        for (int j = 0; j < ROWS_PER_WAVE; j++) {
            const int lr = wave * ROWS_PER_WAVE + j;
            const int64_t row = row0 + lr;
            float inv = 0.f;
            if (row < B) {
                const char *xrow = (const char *)x + row * ldx * (BF16 ? 2 : 4);
                const float *trow = emb + clamp_label(labels[row], C) * lde;
                if constexpr (MODE == 0) {
                    float ss, dt;
                    row_reduce<BF16>(xrow, trow, D, loss_vec != 0, ss, dt);
                    inv = 1.0f / sqrtf(fmaxf(ss, L2NORM_EPS));
                    if (first_slice) {
                        if (lane == 0) {
                            if (inv_norm) inv_norm[row] = inv;
                            loss_i[row] = 1.0f - dt * inv;
                        }
                        if (xhat) {
                            float *orow = xhat + row * ldxhat;
                            if (loss_vec && !BF16) {
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
                    }
                } else {
                    const float s = row_sqdist<BF16>(xrow, trow, D, loss_vec != 0);
                    if (lane == 0) {
                        loss_i[row] = s;
                        if (dist_i) dist_i[row] = sqrtf(s);
                    }
                }
            }
            if (MODE == 0 && lane == 0) sInv[lr] = inv;
        }
    }

    // ---- 2. "true" score per sample, rebuilt with exactly the arithmetic the class-tile loop uses for column y (k-ascending fmaf
    // chain == MFMA; |e|^2 as even-k sum + odd-k sum; |p|^2 as one chain), so the true class matches its own matrix entry bit for bit.
    // Wave 0 walks the dot products, wave 1 the class norms, wave 2 the feature norms, one sample per lane of their lower halves.
    {
        float t = 0.f, ce = 0.f, co = 0.f;
        for (int64_t k0 = 0; k0 < D; k0 += BK) {
            wg_barrier();
            stage_x<MODE, BF16>(sA, x, ldx, row0, B, k0, D, x_vec != 0, sInv);
            stage_label_rows(sB[0], emb, lde, sY, k0, D, e_vec != 0);
            wg_barrier();
            const int kc = (int)((D - k0 < BK) ? (D - k0) : BK);
            if (lane < 32) {
                const float *pa = sA + lane * LD, *pe = sB[0] + lane * LD;
                if (wave == 0) {
                    for (int k = 0; k < kc; k++) t = fmaf(staged(pa, k), staged(pe, k), t);
                } else if (MODE == 1 && wave == 1) {
                    for (int k = 0; k < kc; k += 2) {
                        ce = fmaf(staged(pe, k), staged(pe, k), ce);
                        if (k + 1 < kc) co = fmaf(staged(pe, k + 1), staged(pe, k + 1), co);
                    }
                } else if (MODE == 1 && wave == 2) {
                    for (int k = 0; k < kc; k++) t = fmaf(staged(pa, k), staged(pa, k), t);
                }
            }
        }
        if (lane < 32) {
            if (wave == 0) sDot[lane] = t;
            else if (MODE == 1 && wave == 1) sEn[lane] = ce + co;
            else if (MODE == 1 && wave == 2) sPn[lane] = t;
        }
        wg_barrier();
        if (tid < 32) sTrue[tid] = MODE == 0 ? sDot[tid] : ((sPn[tid] + sEn[tid]) - 2.0f * sDot[tid]);
    }

    // ---- 3. class tiles: four at a time, one per wave, on one shared feature chunk
    int n_better[16], n_within[16];
    float best_v[16];
    int best_c[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        n_better[r] = 0; n_within[r] = 0;
        best_v[r] = MODE == 0 ? -INFINITY : INFINITY;
        best_c[r] = NO_CLASS;
    }

    const int64_t c_beg = (int64_t)blockIdx.y * tiles_per_block * 32;
    const int64_t c_end = (c_beg + (int64_t)tiles_per_block * 32 < C) ? c_beg + (int64_t)tiles_per_block * 32 : C;
    for (int64_t cr = c_beg; cr < c_end; cr += 32 * WAVES) {
        const int64_t c0 = cr + 32 * wave;
        const bool active = c0 < c_end;                       // wave-uniform
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        float cn = 0.f;  // |emb_c|^2 for this lane's class (distance head), half of D per lane
        for (int64_t k0 = 0; k0 < D; k0 += BK) {
            wg_barrier();
            stage_x<MODE, BF16>(sA, x, ldx, row0, B, k0, D, x_vec != 0, sInv);
            if (active) tile32::stage(sB[wave], emb, lde, c0, C, k0, D);
            wg_barrier();
            if (!active) continue;
            const int64_t kc = (D - k0 < BK) ? (D - k0) : BK;
            const int steps = (int)((kc + 1) / 2);           // MFMA steps (2 k each), zero padded
            const float *pa = sA + col * LD + hi * 32;
            const float *pb = sB[wave] + col * LD + hi * 32;
            for (int s = 0; s < steps; s += 4) {
                const float4 a4 = *(const float4 *)(pa + s);
                const float4 b4 = *(const float4 *)(pb + s);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
                if (s + 1 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
                if (s + 2 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
                if (s + 3 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
                if (MODE == 1) {
                    cn = fmaf(b4.x, b4.x, cn);
                    if (s + 1 < steps) cn = fmaf(b4.y, b4.y, cn);
                    if (s + 2 < steps) cn = fmaf(b4.z, b4.z, cn);
                    if (s + 3 < steps) cn = fmaf(b4.w, b4.w, cn);
                }
            }
        }
        if (!active) continue;
        if (MODE == 1) cn += __shfl_xor(cn, 32, 64);          // both halves hold even + odd (the sum commutes)
        const int64_t c = c0 + col;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int lr = tile32::acc_row(r, hi);
            float sc = acc[r];
            if (MODE == 1) sc = (sPn[lr] + cn) - 2.0f * sc;
            const bool valid = (c < C) && (row0 + lr < B);
            if (valid) {
                if (scores) scores[(row0 + lr) * lds_ + c] = sc;
                const float diff = MODE == 0 ? (sc - sTrue[lr]) : (sTrue[lr] - sc);  // > 0: better than true
                if (fabsf(diff) < 1e-6f) n_within[r]++;
                else if (diff >= 1e-6f) n_better[r]++;
                const bool better = MODE == 0 ? (sc > best_v[r]) : (sc < best_v[r]);
                if (better) { best_v[r] = sc; best_c[r] = (int)c; }
            }
        }
    }

    // reduce over the 32 lanes (classes) that share `hi`, then over the four waves in LDS
#pragma unroll
    for (int r = 0; r < 16; r++) {
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            n_better[r] += __shfl_xor(n_better[r], off, 64);
            n_within[r] += __shfl_xor(n_within[r], off, 64);
            const float ov = __shfl_xor(best_v[r], off, 64);
            const int oc = __shfl_xor(best_c[r], off, 64);
            const bool take = MODE == 0 ? (ov > best_v[r] || (ov == best_v[r] && oc < best_c[r]))
                                        : (ov < best_v[r] || (ov == best_v[r] && oc < best_c[r]));
            if (take) { best_v[r] = ov; best_c[r] = oc; }
        }
        const int lr = tile32::acc_row(r, hi);
        if (col == 0) {
            atomicAdd(&sCnt[2 * lr], n_better[r]);
            atomicAdd(&sCnt[2 * lr + 1], n_within[r]);
            if (best_c[r] != NO_CLASS) atomicMax(&sBest[lr], best_word<MODE>(best_v[r], best_c[r]));
        }
    }
    wg_barrier();

    const int64_t row = row0 + tid;
    const bool mine = tid < 32 && row < B;
    if (gridDim.y == 1) {
        if (mine) {
            n_better_out[row] = sCnt[2 * tid];
            n_within_out[row] = sCnt[2 * tid + 1];
            if (best_out) best_out[row] = NO_CLASS - (int32_t)(uint32_t)(sBest[tid] & 0xFFFFFFFFull);
        }
        return;
    }
    // several slices: add into the workspace; the last slice of this strip to arrive writes the strip's results
    if (mine) {
        atomicAdd(&part_cnt[2 * row], (uint32_t)sCnt[2 * tid]);
        atomicAdd(&part_cnt[2 * row + 1], (uint32_t)sCnt[2 * tid + 1]);
        if (sBest[tid] != 0ull) atomicMax(&part_best[row], sBest[tid]);
    }
    // Every word the slices share is touched by device-scope atomics only (they execute where all compute dies see them), and
    // this workgroup's adds are released and drained before its ticket is drawn: whoever draws the last ticket reads complete sums.
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_barrier();
    if (tid == 0) sLast = atomicAdd(&ticket[blockIdx.x], 1u) == gridDim.y - 1 ? 1 : 0;
    wg_barrier();
    if (!sLast) return;
    __threadfence();
    if (mine) {
        n_better_out[row] = (int32_t)atomicAdd(&part_cnt[2 * row], 0u);          // atomic reads: the other slices' sums live in L2
        n_within_out[row] = (int32_t)atomicAdd(&part_cnt[2 * row + 1], 0u);
        if (best_out) best_out[row] = NO_CLASS - (int32_t)(uint32_t)(atomicMax(&part_best[row], 0ull) & 0xFFFFFFFFull);
    }
}

// class tiles (of 32) one workgroup walks, four at a time: all of them while the class set is small or the strips alone fill the
// chip, else slices of a multiple of four tiles, aiming at ~256 workgroups
inline int tiles_per_block(int64_t B, int64_t C)
{
    const int64_t tiles = (C + 31) / 32, strips = (B + 31) / 32;
    if (tiles <= WAVES || strips >= 256) return (int)tiles;
    int64_t slices = 256 / strips;
    const int64_t rounds = (tiles + WAVES - 1) / WAVES;
    if (slices > rounds) slices = rounds;
    const int64_t per = (tiles + slices - 1) / slices;
    return (int)((per + WAVES - 1) / WAVES * WAVES);
}

}  // namespace head
}  // namespace se

using namespace se;

extern "C" int64_t se_embed_head_workspace_bytes(int mode, int64_t B, int64_t D, int64_t C)
{
    (void)mode; (void)D;
    if (B <= 0 || C <= 0) return 0;
    if ((int64_t)head::tiles_per_block(B, C) * 32 >= C) return 0;
    const int64_t strips = (B + 31) / 32;
    return B * 16 + (strips * 4 + 7) / 8 * 8;      // per sample: one ordered word + two counters; per strip: one ticket
}

extern "C" int se_embed_head_fwd(int mode, const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *emb, int64_t lde,
                                 int64_t B, int64_t D, int64_t C, float *xhat, int64_t ldxhat, float *inv_norm, float *loss_i, float *dist_i,
                                 float *loss_mean, int32_t *n_better, int32_t *n_within, int32_t *best, float *scores, int64_t lds,
                                 void *workspace, int64_t workspace_bytes, se_stream_t stream)
{
    if (mode != 0 && mode != 1) return fail(SE_ERR_INVALID, "se_embed_head_fwd: bad mode %d (0: cosine head, 1: squared-distance head)", mode);
    if (B < 0 || D <= 0 || C <= 0) return fail(SE_ERR_INVALID, "se_embed_head_fwd: bad shape B=%lld D=%lld C=%lld", (long long)B, (long long)D, (long long)C);
    if (B == 0) return SE_OK;
    if (!x || !labels || !emb || !loss_i || !n_better || !n_within) return fail(SE_ERR_INVALID, "se_embed_head_fwd: null pointer");
    if (!is_float_dtype(x_dtype)) return fail(SE_ERR_INVALID, "se_embed_head_fwd: bad dtype %d", x_dtype);
    if (mode == 1) { xhat = nullptr; inv_norm = nullptr; }
    else dist_i = nullptr;
    if (ldx < D || lde < D || (xhat && ldxhat < D) || (scores && lds < C))
        return fail(SE_ERR_INVALID, "se_embed_head_fwd: leading dimension too small");
    const int64_t need = se_embed_head_workspace_bytes(mode, B, D, C);
    if (need > 0 && (!workspace || workspace_bytes < need || (((uintptr_t)workspace) & 7)))
        return fail(SE_ERR_INVALID, "se_embed_head_fwd: needs %lld bytes of 8-byte aligned workspace (se_embed_head_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)stream;
    const bool bf = x_dtype == SE_DTYPE_BF16;
    // the 16-byte paths of the loss rows: the siblings' own predicates (they decide the summation order)
    int loss_vec;
    if (mode == 0) {
        const int vq = bf ? 8 : 4;
        loss_vec = (D % vq == 0) && (ldx % vq == 0) && (lde % 4 == 0) && aligned16(x) && aligned16(emb) &&
                   (!xhat || ((ldxhat % 4 == 0) && aligned16(xhat)));
    } else {
        loss_vec = !bf && (D % 4 == 0) && (ldx % 4 == 0) && (lde % 4 == 0) && aligned16(x) && aligned16(emb);
    }
    // staging: four consecutive k per load (any path gives the same values)
    const int x_vec = ((ldx | D) & 3) == 0 && ((((uintptr_t)x) & (bf ? 7 : 15)) == 0);
    const int e_vec = ((lde | D) & 3) == 0 && aligned16(emb);
    const int tpb = head::tiles_per_block(B, C);
    const int64_t strips = (B + 31) / 32, slices = ((C + 31) / 32 + tpb - 1) / tpb;
    unsigned long long *part_best = (unsigned long long *)workspace;
    uint32_t *part_cnt = need > 0 ? (uint32_t *)((char *)workspace + B * 8) : nullptr;
    uint32_t *ticket = need > 0 ? (uint32_t *)((char *)workspace + B * 16) : nullptr;
    if (need > 0) SE_HIP_CHECK(hipMemsetAsync(workspace, 0, (size_t)need, s));
    dispatch_bools(mode == 1, bf, [&](auto M, auto XB) {
        hipLaunchKernelGGL((head::embed_head_kernel<M() ? 1 : 0, XB()>), dim3((unsigned)strips, (unsigned)slices), dim3(head::THREADS), 0, s,
                           x, ldx, labels, emb, lde, B, D, C, xhat, ldxhat, inv_norm, loss_i, dist_i, n_better, n_within, best, scores, lds,
                           loss_vec, x_vec, e_vec, tpb, part_best, part_cnt, ticket);
    });
    SE_LAUNCH_CHECK();
    if (loss_mean) {
        launch_mean(loss_i, B, loss_mean, s);
        SE_LAUNCH_CHECK();
    }
    return SE_OK;
}
