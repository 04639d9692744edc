// image_batch.hip -- one launch composes a training / test batch [B, ch, cw, 3] (NHWC) from variable-sized uint8 RGB images that
// stay resident in device memory: Pillow's 8-bit bilinear resize, normalisation, optional BGR order, flip, random erasing, crop
// and reflect padding.
//
// Replaces: datasets/common.py:380-581 (FileDatasetGenerator.compose_batch / _load_image / _transform: PIL.Image.resize(size,
//           BILINEAR) of the decoded image, img_to_array, (x - mean) / std, RGB -> BGR, horizontal flip, random erasing, random or
//           centre crop, np.pad(..., 'reflect')), which the reference runs per sample in 8 worker processes.
//
// The kernel knows nothing of crop, pad or flip: the host folds them into per-output-column / per-output-row tables (xmap / xk,
// ymap / yk: first source index, tap count and Pillow's 22-bit fixed-point weights; sehip.resample_tables), so an output pixel is
//     t(r) = clip8((2^21 + sum_i xk[cx, i] * src[r, xmin + i, c]) >> 22)        horizontal pass, uint8 between the passes
//     v    = clip8((2^21 + sum_j yk[cy, j] * t(ymin + j)) >> 22)                vertical pass
//     out  = (float(v) - mean[c]) / std[c]                                      IEEE subtract and divide
// which is Pillow's ImagingResample for 8-bit images, integer for integer.  Inside a sample's erase rectangle (given in the
// coordinates `u` of the zoomed, flipped image that the tables carry) the value is (U - mean[c']) / std[c'] with U uniform in
// [0, 255) from a counter-based hash of (seed, u_y, u_x, c'); c' is the POSITION of the channel in the output, as in the reference,
// which normalises its noise with the RGB-ordered statistics even in BGR mode (common.py:538-540).
//
// Layout: one 256-thread workgroup per (sample, band of IB_BAND output rows).  It stages the sample's column table and the 256-entry
// normalisation table of each channel (768 divisions per workgroup instead of one per output value) in LDS, then walks its band in
// sub-bands whose source rows fit the LDS tile: horizontal pass of those source rows into LDS as uint8, wg_barrier(), vertical pass
// from LDS + table look-up + coalesced stores (adjacent lanes write adjacent output elements).  A sub-band is as many rows of the band
// as fit, found from the row table itself, so any zoom factor and any reflect-padding pattern is served by the same loop; the host
// only guarantees that ONE output row's taps fit (Ky rows).
// Every index read from a table is clamped to its image before it is used, and a sample whose image does not lie inside the arena
// is written as NaN: wrong tables give wrong pixels, never an out-of-bounds access.
#include "se_common.h"

namespace se {

constexpr int IB_THREADS = 256;
constexpr int IB_BAND = 8;                 // output rows per workgroup
constexpr int IB_LDS_MAX = 64 * 1024;      // dynamic LDS a workgroup may own without a function attribute

__device__ __forceinline__ int ib_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// counter-based noise: murmur3's finaliser over the sample's seed and the (row, column, channel) of the zoomed, flipped image
__device__ __forceinline__ uint32_t ib_mix(uint32_t h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ float ib_noise(uint32_t seed, int uy, int ux, int c)
{
    uint32_t h = ib_mix(seed ^ 0x9E3779B9u);
    h = ib_mix(h ^ ((uint32_t)uy * 0x9E3779B1u));
    h = ib_mix(h ^ ((uint32_t)ux * 0x85EBCA77u));
    h = ib_mix(h ^ ((uint32_t)c * 0xC2B2AE3Du + 0x27D4EB2Fu));
    return ((float)(h >> 8) * (1.0f / 16777216.0f)) * 255.0f;          // [0, 255): the largest value rounds to 255 - 2^-16
}

template <bool BF16>
__global__ __launch_bounds__(IB_THREADS) void image_batch_kernel(const uint8_t *__restrict__ arena, int64_t arena_bytes,
                                                                 const int64_t *__restrict__ src_off, const int32_t *__restrict__ src_hw,
                                                                 const int32_t *__restrict__ xmap, const int32_t *__restrict__ xk,
                                                                 const int32_t *__restrict__ ymap, const int32_t *__restrict__ yk,
                                                                 const int32_t *__restrict__ erase, const uint32_t *__restrict__ seed,
                                                                 const float *__restrict__ mean, const float *__restrict__ stdv, int bgr,
                                                                 void *__restrict__ out, int ch, int cw, int Kx, int Ky, int tile_rows)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ib_lds[];
    __shared__ int yband[IB_BAND][3];          // (u, ymin, n) of the band's rows, clamped to the image

    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int cy0 = blockIdx.x * IB_BAND;
    const int nrows = min(IB_BAND, ch - cy0);
    const int row_elems = cw * 3;
    const int row_bytes = (row_elems + 3) & ~3;

    float *lut = (float *)ib_lds;                       // [3][256]: (v - mean[c]) / std[c]
    int *xmn = (int *)(lut + 768);                      // [cw][3]: (u, xmin, n), clamped
    int *xw = xmn + 3 * cw;                             // [cw][Kx]
    uint8_t *tile = (uint8_t *)(xw + (int64_t)cw * Kx); // [tile_rows][row_bytes]

    const int h = src_hw[b * 2], w = src_hw[b * 2 + 1];
    const int64_t off = src_off[b];
    if (h <= 0 || w <= 0 || off < 0 || off > arena_bytes || (int64_t)h * w * 3 > arena_bytes - off) {   // wave-uniform
        for (int idx = tid; idx < nrows * row_elems; idx += IB_THREADS)
            st_elem<BF16>(out, ((b * ch + cy0) * (int64_t)cw) * 3 + idx, __uint_as_float(0x7FC00000u));
        return;
    }
    const uint8_t *src = arena + off;

    // ---- stage the tables ----
    for (int i = tid; i < 768; i += IB_THREADS) {
        const int c = i >> 8;
        lut[i] = ((float)(i & 255) - mean[c]) / stdv[c];
    }
    for (int cx = tid; cx < cw; cx += IB_THREADS) {
        const int32_t *m = xmap + (b * cw + cx) * 3;
        int x0 = m[1], n = m[2];
        x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0);
        n = n < 0 ? 0 : min(n, min(Kx, w - x0));
        xmn[3 * cx] = m[0];
        xmn[3 * cx + 1] = x0;
        xmn[3 * cx + 2] = n;
    }
    for (int i = tid; i < cw * Kx; i += IB_THREADS) xw[i] = xk[b * (int64_t)cw * Kx + i];
    if (tid < nrows) {
        const int32_t *m = ymap + (b * ch + cy0 + tid) * 3;
        int y0 = m[1], n = m[2];
        y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0);
        n = n < 0 ? 0 : min(n, min(min(Ky, tile_rows), h - y0));
        yband[tid][0] = m[0];
        yband[tid][1] = y0;
        yband[tid][2] = n;
    }
    const int ey = erase[b * 4], ex = erase[b * 4 + 1], eh = erase[b * 4 + 2], ew = erase[b * 4 + 3];
    const uint32_t sd = seed[b];
    wg_barrier();

    int r0 = 0;
    while (r0 < nrows) {
        // ---- the sub-band: rows r0 .. r1 - 1 whose source rows [lo, hi) fit the tile (the same scalar loop in every thread) ----
        int lo = yband[r0][1], hi = lo + yband[r0][2], r1 = r0 + 1;
        while (r1 < nrows) {
            const int l2 = min(lo, yband[r1][1]), h2 = max(hi, yband[r1][1] + yband[r1][2]);
            if (h2 - l2 > tile_rows) break;
            lo = l2; hi = h2; r1++;
        }
        // ---- horizontal pass: source rows lo .. hi - 1 -> tile, uint8 ----
        const int items = (hi - lo) * cw;
        for (int idx = tid; idx < items; idx += IB_THREADS) {
            const int r = idx / cw, cx = idx - r * cw;
            const int x0 = xmn[3 * cx + 1], n = xmn[3 * cx + 2];
            const uint8_t *p = src + ((int64_t)(lo + r) * w + x0) * 3;
            const int *k = xw + cx * Kx;
            int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
            for (int i = 0; i < n; i++) {
                const int wt = k[i];
                s0 += wt * (int)p[3 * i];
                s1 += wt * (int)p[3 * i + 1];
                s2 += wt * (int)p[3 * i + 2];
            }
            uint8_t *t = tile + r * row_bytes + cx * 3;
            t[0] = (uint8_t)ib_clip8(s0 >> 22);
            t[1] = (uint8_t)ib_clip8(s1 >> 22);
            t[2] = (uint8_t)ib_clip8(s2 >> 22);
        }
        wg_barrier();
        // ---- vertical pass + normalisation + erase: one output element per item, adjacent lanes adjacent elements ----
        const int oitems = (r1 - r0) * row_elems;
        for (int idx = tid; idx < oitems; idx += IB_THREADS) {
            const int rr = idx / row_elems, e = idx - rr * row_elems;
            const int cx = e / 3, cpos = e - cx * 3;              // cpos: position in the output; c: source channel
            const int c = bgr ? 2 - cpos : cpos;
            const int row = r0 + rr, cy = cy0 + row;
            const int uy = yband[row][0], y0 = yband[row][1], n = yband[row][2];
            const int ux = xmn[3 * cx];
            float val;
            if (eh > 0 && uy >= ey && uy < ey + eh && ux >= ex && ux < ex + ew) {
                val = (ib_noise(sd, uy, ux, cpos) - mean[cpos]) / stdv[cpos];
            } else {
                const int32_t *k = yk + (b * ch + cy) * (int64_t)Ky;
                const uint8_t *t = tile + (y0 - lo) * row_bytes + cx * 3 + c;
                int s = 1 << 21;
                for (int j = 0; j < n; j++) s += k[j] * (int)t[j * row_bytes];
                val = lut[c * 256 + ib_clip8(s >> 22)];
            }
            st_elem<BF16>(out, ((b * ch + cy) * (int64_t)cw) * 3 + e, val);
        }
        r0 = r1;
        if (r0 < nrows) wg_barrier();          // the next sub-band overwrites the tile
    }
}

}  // namespace se

using namespace se;

extern "C" int se_image_batch(const void *arena, int64_t arena_bytes, const int64_t *src_off, const int32_t *src_hw, const int32_t *xmap,
                              const int32_t *xk, const int32_t *ymap, const int32_t *yk, const int32_t *erase, const uint32_t *seed,
                              const float *mean, const float *std, int bgr, void *out, int out_dtype, int64_t B, int ch, int cw, int Kx,
                              int Ky, se_stream_t stream)
{
    if (B < 0 || ch <= 0 || cw <= 0 || Kx <= 0 || Ky <= 0 || arena_bytes < 0)
        return fail(SE_ERR_INVALID, "se_image_batch: bad shape B=%lld ch=%d cw=%d Kx=%d Ky=%d arena_bytes=%lld", (long long)B, ch, cw, Kx, Ky,
                    (long long)arena_bytes);
    if (!is_float_dtype(out_dtype)) return fail(SE_ERR_INVALID, "se_image_batch: bad output dtype %d", out_dtype);
    if (B == 0) return SE_OK;
    if (!arena || !src_off || !src_hw || !xmap || !xk || !ymap || !yk || !erase || !seed || !mean || !std || !out)
        return fail(SE_ERR_INVALID, "se_image_batch: null pointer");
    if (B > 65535) return fail(SE_ERR_UNSUPPORTED, "se_image_batch: B=%lld exceeds 65535 samples per launch", (long long)B);
    if (cw > (1 << 20) || ch > (1 << 20) || Kx > 4096 || Ky > 4096) return fail(SE_ERR_UNSUPPORTED, "se_image_batch: crop or tap count too large");
    // LDS: normalisation table + column table + tile.  The tile holds at least one output row's taps (Ky rows) and at most what a
    // band needs at the largest zoom factor its tap count admits (scale <= (Ky - 1) / 2).
    const int64_t row_bytes = ((int64_t)cw * 3 + 3) & ~(int64_t)3;
    const int64_t fixed = 768 * 4 + (int64_t)cw * 3 * 4 + (int64_t)cw * Kx * 4;
    const int64_t fit = fixed < IB_LDS_MAX ? (IB_LDS_MAX - fixed) / row_bytes : 0;
    if (fit < Ky)
        return fail(SE_ERR_UNSUPPORTED, "se_image_batch: crop width %d with %d x %d taps needs more LDS than a workgroup may own", cw, Kx, Ky);
    const int64_t want = (int64_t)(IB_BAND - 1) * (Ky - 1) / 2 + Ky + 1;
    const int tile_rows = (int)(want < fit ? want : fit);
    const size_t lds = (size_t)(fixed + tile_rows * row_bytes);
    const dim3 grid((unsigned)((ch + IB_BAND - 1) / IB_BAND), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == SE_DTYPE_BF16)
        hipLaunchKernelGGL(image_batch_kernel<true>, grid, dim3(IB_THREADS), lds, s, (const uint8_t *)arena, arena_bytes, src_off, src_hw, xmap, xk,
                           ymap, yk, erase, seed, mean, std, bgr, out, ch, cw, Kx, Ky, tile_rows);
    else
        hipLaunchKernelGGL(image_batch_kernel<false>, grid, dim3(IB_THREADS), lds, s, (const uint8_t *)arena, arena_bytes, src_off, src_hw, xmap, xk,
                           ymap, yk, erase, seed, mean, std, bgr, out, ch, cw, Kx, Ky, tile_rows);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
