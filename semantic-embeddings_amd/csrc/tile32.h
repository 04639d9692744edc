// tile32.h -- the fp32 32 x 32 output tile on v_mfma_f32_32x32x2_f32 of the DeViSE kernels (devise.hip): one wave per tile, operands
// staged through LDS in K-chunks (64 k unless a kernel asks for more) with even and odd k de-interleaved, so that lanes 0-31 (k = 2t)
// and 32-63 (k = 2t + 1) each feed four MFMA steps from one 16-byte LDS read.  nn_accuracy_kernel (loss_kernels.hip) works on the same
// tile and shares acc_row and tiles_per_block; its staging and chunk loop are its own (see the comment there).  The embedding heads
// (embed_head.hip) stage their class chunks with stage(); the chunks their four waves share are staged by all 256 threads with the
// head's own loops in this layout.  What these kernels do with a finished tile of class scores is metric:: of loss_head.h.
#pragma once
#include "se_common.h"

namespace se {
namespace tile32 {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BK = 64;            // k per staged chunk
constexpr int LD = BK + 4;        // padded row pitch (floats): conflict-free ds_read_b128

// row of the 32 x 32 tile that accumulator register r holds in the lanes of half `hi` (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// Staging loads are UNCONDITIONAL (out-of-range rows / k read a valid in-range address and are zeroed afterwards): with a branch per
// element the compiler waited for every load before issuing the next one, which was most of these kernels' time.
template <int CK = BK>
__device__ __forceinline__ void put(float *lds, int r, int kq, const float v[4])
{
    float *o = lds + r * (CK + 4);                   // even k to [0, CK / 2), odd k to [CK / 2, CK) of the row
    o[(kq >> 1)] = v[0];
    o[(kq >> 1) + 1] = v[2];
    o[CK / 2 + (kq >> 1)] = v[1];
    o[CK / 2 + (kq >> 1) + 1] = v[3];
}

// 8 x (one row's 4 consecutive k) per lane; rowp(r) = pointer to LDS row r's source row, or nullptr outside the matrix.
// Split in two so that a kernel can keep the NEXT chunk's loads in flight while the matrix pipe works on the current one.
template <int CK = BK, class RowPtr>
__device__ __forceinline__ void load_rows(float (&v)[CK / 8][4], RowPtr rowp, const float *any_valid_row, int64_t ld, int64_t k0, int64_t K)
{
    const int lane = lane_id();
    const bool vec = ((ld | K) & 3) == 0 && (((uintptr_t)any_valid_row) & 15) == 0;          // wave-uniform
#pragma unroll
    for (int it = 0; it < CK / 8; it++) {
        const int idx = it * 64 + lane;
        const int r = idx / (CK / 4), kq = (idx % (CK / 4)) * 4;
        const float *p = rowp(r);
        const bool rok = p != nullptr;
        if (!rok) p = any_valid_row;
        if (vec) {
            const bool ok = rok && k0 + kq < K;
            const float4 t = *(const float4 *)(p + (k0 + kq < K ? k0 + kq : 0));
            v[it][0] = ok ? t.x : 0.f; v[it][1] = ok ? t.y : 0.f; v[it][2] = ok ? t.z : 0.f; v[it][3] = ok ? t.w : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool kok = k0 + kq + j < K;
                const float t = p[kok ? k0 + kq + j : 0];
                v[it][j] = (rok && kok) ? t : 0.f;
            }
        }
    }
}

template <int CK = BK>
__device__ __forceinline__ void put_rows(float *lds, const float (&v)[CK / 8][4])
{
    const int lane = lane_id();
#pragma unroll
    for (int it = 0; it < CK / 8; it++) {
        const int idx = it * 64 + lane;
        put<CK>(lds, idx / (CK / 4), (idx % (CK / 4)) * 4, v[it]);
    }
}

template <class RowPtr>
__device__ __forceinline__ void stage_rows(float *lds, RowPtr rowp, const float *any_valid_row, int64_t ld, int64_t k0, int64_t K)
{
    float v[BK / 8][4];
    load_rows<BK>(v, rowp, any_valid_row, ld, k0, K);
    put_rows<BK>(lds, v);
}

// 32 rows x 64 k of a row-major [rows, K] matrix -> LDS; zero outside
__device__ __forceinline__ void stage(float *lds, const float *src, int64_t ld, int64_t row0, int64_t nrows, int64_t k0, int64_t K)
{
    stage_rows(lds, [=](int r) -> const float * { return row0 + r < nrows ? src + (row0 + r) * ld : nullptr; }, src, ld, k0, K);
}

// the same tile of the TRANSPOSE of a row-major [K, cols] matrix: LDS row r = column col0 + r of `src`, k = its row index
__device__ __forceinline__ void stage_t(float *lds, const float *src, int64_t ld, int64_t col0, int64_t ncols, int64_t k0, int64_t K)
{
    const int lane = lane_id();
    const int r = lane & 31;
    const bool cok = col0 + r < ncols;
    const float *p = src + (cok ? col0 + r : col0);
    float v[32];
#pragma unroll
    for (int it = 0; it < 32; it++) {
        const int k = it * 2 + (lane >> 5);                                 // 32 consecutive columns of one source row per half-wave
        const bool kok = k0 + k < K;
        const float t = p[(kok ? k0 + k : 0) * ld];
        v[it] = (cok && kok) ? t : 0.f;
    }
#pragma unroll
    for (int it = 0; it < 32; it++) {
        const int k = it * 2 + (lane >> 5);
        lds[r * LD + ((k & 1) ? 32 : 0) + (k >> 1)] = v[it];
    }
}

// acc += A[32, kc] . B[32, kc]^T over one staged chunk (kc <= CK valid k, zero padded to whole MFMA steps of 2 k)
template <int CK = BK>
__device__ __forceinline__ f32x16 mma_chunk(f32x16 acc, const float *sA, const float *sB, int col, int hi, int64_t kc)
{
    const int steps = (int)((kc + 1) / 2);
    const float *pa = sA + col * (CK + 4) + hi * (CK / 2);
    const float *pb = sB + col * (CK + 4) + hi * (CK / 2);
    for (int s = 0; s < steps; s += 4) {
        const float4 a4 = *(const float4 *)(pa + s);
        const float4 b4 = *(const float4 *)(pb + s);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
        if (s + 1 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
        if (s + 2 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
        if (s + 3 < steps) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
    }
    return acc;
}

// class tiles (of 32) one workgroup walks: all of them while that still fills the chip or the class set is small (<= min_tiles), else slices
inline int tiles_per_block(int64_t B, int64_t C, int64_t min_tiles)
{
    const int64_t tiles = (C + 31) / 32, sample_blocks = (B + 31) / 32;
    if (tiles <= min_tiles || sample_blocks >= 1024) return (int)tiles;
    int64_t slices = 1024 / sample_blocks;                  // aim for ~1024 waves
    if (slices > tiles) slices = tiles;
    return (int)((tiles + slices - 1) / slices);
}

}  // namespace tile32
}  // namespace se
