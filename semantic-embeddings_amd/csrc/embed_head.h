// embed_head.h -- the workgroup of the embedding heads (embed_head.hip explains the layout): loss rows, the label's score and the
// class tiles of one 32-sample strip, with the helpers that stage its operands.  se_embed_head_fwd (embed_head.hip) launches it as
// a kernel of its own; the embedding role of se_joint_head_fwd (joint_head.hip) runs the same text beside the classifier's rows.
#pragma once
#include "loss_head.h"

namespace se {
namespace head {

using tile32::f32x16;

constexpr int THREADS = 256, WAVES = 4;
constexpr int ROWS_PER_WAVE = 32 / WAVES;
constexpr int BK = tile32::BK, LD = tile32::LD;

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

// the label rows emb[y[r]] of the strip, same chunk, same layout, by all 256 threads (rows outside the batch: zero).
// This is tile32::load_rows / put_rows spread over 256 threads, kept written out: as a tile32::stage_rows<256> call with a row-pointer
// functor the squared-distance head measured up to 2.3 us (1.6 %) above the parent's range (profiles/loss_head_dedup.txt section 3).
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

// What one workgroup does: strip `strip` of 32 samples against class slice `slice` of `slices` (tiles_per_block x 32 classes each).
// MODE 0: cosine head on raw features, MODE 1: squared-distance head, MODE 2: correlation head on features that are used as they
// come (x float32: loss_i = 1 - x . emb[y], no norm, no xhat; the metric is MODE 0's on x itself) -- se_joint_head_fwd.
template <int MODE, bool BF16>
__device__ __forceinline__ void head_strip(
    const unsigned strip, const unsigned slice, const unsigned slices,
    const void *__restrict__ x, int64_t ldx, const int64_t *__restrict__ labels, const float *__restrict__ emb, int64_t lde,
    int64_t B, int64_t D, int64_t C, float *__restrict__ xhat, int64_t ldxhat, float *__restrict__ inv_norm, float *__restrict__ loss_i,
    float *__restrict__ dist_i, int32_t *__restrict__ n_better_out, int32_t *__restrict__ n_within_out, int32_t *__restrict__ best_out,
    float *__restrict__ scores, int64_t lds_, int loss_vec, int x_vec, int e_vec, int tiles_per_block,
    unsigned long long *__restrict__ part_best, uint32_t *__restrict__ part_cnt, uint32_t *__restrict__ ticket)
{
    static_assert(MODE != 2 || !BF16, "the correlation head reads float32");
    __shared__ __attribute__((aligned(16))) float sA[32 * LD];
    __shared__ __attribute__((aligned(16))) float sB[WAVES][32 * LD];
    __shared__ float sInv[32], sTrue[32], sPn[32], sDot[32], sEn[32];
    __shared__ int sY[32];
    __shared__ int sCnt[64];
    __shared__ unsigned long long sBest[32];
    __shared__ int sLast;

    const int tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
    const int col = lane & 31, hi = lane >> 5;
    const int64_t row0 = (int64_t)strip * 32;
    const bool first_slice = slice == 0;

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
                        if (xhat) write_xhat_row<BF16>(xrow, xhat + row * ldxhat, D, loss_vec != 0, inv);
                    }
                } else if constexpr (MODE == 2) {
                    float ss, dt;
                    row_reduce<BF16>(xrow, trow, D, loss_vec != 0, ss, dt);
                    if (lane == 0) loss_i[row] = 1.0f - dt;
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
        if (tid < 32) sTrue[tid] = MODE != 1 ? sDot[tid] : ((sPn[tid] + sEn[tid]) - 2.0f * sDot[tid]);
    }

    // ---- 3. class tiles: four at a time, one per wave, on one shared feature chunk
    constexpr bool DOT = MODE != 1;
    metric::Tally tally[16];
#pragma unroll
    for (int r = 0; r < 16; r++) tally[r] = metric::empty_tally(DOT);

    const int64_t c_beg = (int64_t)slice * tiles_per_block * 32;
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
                if (!DOT) cn = metric::class_norm_steps(cn, b4, s, steps);
            }
        }
        if (!active) continue;
        if (!DOT) cn += __shfl_xor(cn, 32, 64);          // both halves hold even + odd (the sum commutes)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int lr = tile32::acc_row(r, hi);
            metric::update(tally[r], DOT, acc[r], sPn, cn, sTrue, lr, row0 + lr, B, c0 + col, C, scores, lds_);
        }
    }

    // reduce over the 32 lanes (classes) that share `hi`, then over the four waves in LDS
#pragma unroll
    for (int r = 0; r < 16; r++) {
        metric::reduce32(tally[r], DOT);
        const int lr = tile32::acc_row(r, hi);
        if (col == 0) {
            atomicAdd(&sCnt[2 * lr], tally[r].n_better);
            atomicAdd(&sCnt[2 * lr + 1], tally[r].n_within);
            if (tally[r].best_c != metric::NO_CLASS) atomicMax(&sBest[lr], metric::best_word(tally[r].best_v, tally[r].best_c, DOT));
        }
    }
    wg_barrier();

    const int64_t row = row0 + tid;
    const bool mine = tid < 32 && row < B;
    if (slices == 1) {
        if (mine) {
            n_better_out[row] = sCnt[2 * tid];
            n_within_out[row] = sCnt[2 * tid + 1];
            if (best_out) best_out[row] = metric::best_class(sBest[tid]);
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
    if (tid == 0) sLast = atomicAdd(&ticket[strip], 1u) == slices - 1 ? 1 : 0;
    wg_barrier();
    if (!sLast) return;
    __threadfence();
    if (mine) {
        n_better_out[row] = (int32_t)atomicAdd(&part_cnt[2 * row], 0u);          // atomic reads: the other slices' sums live in L2
        n_within_out[row] = (int32_t)atomicAdd(&part_cnt[2 * row + 1], 0u);
        if (best_out) best_out[row] = metric::best_class(atomicMax(&part_best[row], 0ull));
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
