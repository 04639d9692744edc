// tiny_batch.hip -- one launch composes a batch [B, H, W, C] (NHWC) from a device-resident store of small float32 images: gather by
// index, Keras' affine random_transform (rotation, shifts, shear, zoom) with bilinear interpolation and one of three fill modes, both
// flips, standardisation, f32 or bf16 output.
//
// Replaces: datasets/common.py:638-670, 771-796 (TinyDatasetGenerator: keras ImageDataGenerator.random_transform + standardize per
//           sample [third party: keras_preprocessing 1.0.x], whose apply_affine_transform calls scipy.ndimage.affine_transform(order = 1)
//           channel by channel).
//
// Per output element (b, r, c, k), everything in float64, every operation separately rounded (no contraction), in the order of scipy's
// NI_GeometricTransform (so that not only the typical pixel but every near-tie of the float32 rounding and every coordinate that lands
// on an edge agrees):
//     r' = vflip ? H - 1 - r : r,   c' = hflip ? W - 1 - c : c                    Keras flips AFTER the transform
//     y  = (r' * M00 + c' * M01) + M02,   x = (r' * M10 + c' * M11) + M12          the output -> source map of sample b
//     per axis: the fill mode's coordinate rule (tb_axis below) -> taps i0, i1 and the fraction f = v - floor(v)
//     w0 = 1 - f,  w1 = 1 - w0                                                      per axis (scipy: the last weight is 1 - the others)
//     t  = (((0 + (a00 * wy0) * wx0) + (a01 * wy0) * wx1) + (a10 * wy1) * wx0) + (a11 * wy1) * wx1
//     out = (float(t) - mean[k]) / stdp[k]                                         IEEE f32 subtract and divide
// 'constant' outside the image: float(cval) takes the place of float(t) (Keras standardises after the transform).
// A streaming gather: one output element per thread and trip, adjacent lanes adjacent NHWC elements, nothing shared between
// elements, so no LDS, no barrier, no atomics and the same bits whatever the launch geometry.  int64 element offsets; a grid-stride
// loop under a capped grid.  A sample whose index is outside the store is written as NaN; every tap is inside its image by
// construction, whatever the matrix holds (NaN and infinities included).
#include "se_common.h"

#pragma clang fp contract(off)

namespace se {

constexpr int TB_THREADS = 256;

// reflect ('abcd' -> 'dcba|abcd|dcba') of a tap index: period 2 n
__device__ __forceinline__ int tb_fold(int i, int n)
{
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// One axis of length n at coordinate v: taps i0, i1 (inside [0, n - 1]) and the fraction f.  false: 'constant' and outside.
template <int MODE>
__device__ __forceinline__ bool tb_axis(double v, int n, int &i0, int &i1, double &f)
{
    const double last = (double)(n - 1);
    if constexpr (MODE == SE_FILL_REFLECT) {
        const double len = (double)n, p = 2.0 * len;
        if (n == 1) {
            v = 0.0;
        } else if (v < 0.0) {
            if (v < -p) {
                const double q = trunc(-v / p);
                const double s = p * q;
                v = s + v;
            }
            v = v < -len ? v + p : -v - 1.0;
        } else if (v > last) {
            const double q = trunc(v / p);
            const double s = p * q;
            v = v - s;
            if (v >= len) v = p - v - 1.0;
        }
        const double fl = floor(v);
        f = v - fl;
        int i = fl >= -1.0 ? (fl <= last ? (int)fl : n - 1) : -1;       // [-1, n - 1] for every v the rule yields; a NaN lands on -1
        i0 = tb_fold(i, n);
        i1 = tb_fold(i + 1, n);
    } else {
        // 'nearest' does not move the coordinate: the TAPS are clamped, so outside the image both land on the edge pixel
        if (MODE == SE_FILL_CONSTANT && (v < 0.0 || v > last)) return false;
        const double fl = floor(v);
        f = v - fl;
        const int i = fl >= -1.0 ? (fl <= last ? (int)fl : n - 1) : -1;   // every tap pair the clamp can tell apart; a NaN lands on -1
        i0 = i < 0 ? 0 : i;
        i1 = i + 1 < n ? i + 1 : n - 1;
    }
    return true;
}

template <int MODE, bool BF16>
__global__ __launch_bounds__(TB_THREADS) void tiny_batch_kernel(const float *__restrict__ images, int64_t N, const int64_t *__restrict__ index,
                                                                const double *__restrict__ affine, const int32_t *__restrict__ flags,
                                                                const float *__restrict__ mean, const float *__restrict__ stdp, float cval,
                                                                void *__restrict__ out, int64_t total, int H, int W, int C)
{
    const int row_elems = W * C;
    const int img_elems = H * row_elems;                // <= 2^30 (checked by the host)
    const int64_t stride = (int64_t)gridDim.x * TB_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * TB_THREADS + threadIdx.x; e < total; e += stride) {
        const int64_t b = e / img_elems;
        const int rem = (int)(e - b * img_elems);
        const int r = rem / row_elems, re = rem - r * row_elems;
        const int c = re / C, k = re - c * C;
        const int64_t src = index[b];
        if (src < 0 || src >= N) {
            st_elem<BF16>(out, e, __uint_as_float(0x7FC00000u));
            continue;
        }
        const int fl = flags[b];
        const double rr = (double)((fl & 2) ? H - 1 - r : r), cc = (double)((fl & 1) ? W - 1 - c : c);
        const double *m = affine + b * 6;
        const double y0 = rr * m[0], y1 = cc * m[1], y2 = y0 + y1, y = y2 + m[2];
        const double x0 = rr * m[3], x1 = cc * m[4], x2 = x0 + x1, x = x2 + m[5];
        int iy0, iy1, ix0, ix1;
        double fy, fx;
        float v32 = cval;
        if (tb_axis<MODE>(y, H, iy0, iy1, fy) && tb_axis<MODE>(x, W, ix0, ix1, fx)) {
            const float *img = images + src * (int64_t)img_elems + k;
            const double a00 = (double)img[iy0 * row_elems + ix0 * C], a01 = (double)img[iy0 * row_elems + ix1 * C];
            const double a10 = (double)img[iy1 * row_elems + ix0 * C], a11 = (double)img[iy1 * row_elems + ix1 * C];
            const double wy0 = 1.0 - fy, wy1 = 1.0 - wy0, wx0 = 1.0 - fx, wx1 = 1.0 - wx0;
            const double p00 = a00 * wy0, p01 = a01 * wy0, p10 = a10 * wy1, p11 = a11 * wy1;
            const double q00 = p00 * wx0, q01 = p01 * wx1, q10 = p10 * wx0, q11 = p11 * wx1;
            const double t0 = 0.0 + q00, t1 = t0 + q01, t2 = t1 + q10, t = t2 + q11;
            v32 = (float)t;
        }
        const float d = v32 - mean[k];
        st_elem<BF16>(out, e, d / stdp[k]);
    }
}

template <int MODE>
inline void tb_launch(bool bf16, dim3 grid, hipStream_t s, const float *images, int64_t N, const int64_t *index, const double *affine,
                      const int32_t *flags, const float *mean, const float *stdp, float cval, void *out, int64_t total, int H, int W, int C)
{
    if (bf16)
        hipLaunchKernelGGL((tiny_batch_kernel<MODE, true>), grid, dim3(TB_THREADS), 0, s, images, N, index, affine, flags, mean, stdp, cval, out,
                           total, H, W, C);
    else
        hipLaunchKernelGGL((tiny_batch_kernel<MODE, false>), grid, dim3(TB_THREADS), 0, s, images, N, index, affine, flags, mean, stdp, cval, out,
                           total, H, W, C);
}

}  // namespace se

using namespace se;

extern "C" int se_tiny_batch(const float *images, int64_t N, const int64_t *index, const double *affine, const int32_t *flags,
                             const float *mean, const float *stdp, int fill_mode, float cval, void *out, int out_dtype, int64_t B, int H,
                             int W, int C, se_stream_t stream)
{
    if (B < 0 || N < 0 || H <= 0 || W <= 0 || C < 1 || C > 4)
        return fail(SE_ERR_INVALID, "se_tiny_batch: bad shape B=%lld N=%lld H=%d W=%d C=%d (C in 1..4)", (long long)B, (long long)N, H, W, C);
    if (fill_mode != SE_FILL_NEAREST && fill_mode != SE_FILL_CONSTANT && fill_mode != SE_FILL_REFLECT)
        return fail(SE_ERR_INVALID, "se_tiny_batch: bad fill mode %d", fill_mode);
    if (!is_float_dtype(out_dtype)) return fail(SE_ERR_INVALID, "se_tiny_batch: bad output dtype %d", out_dtype);
    if ((int64_t)H * W * C > ((int64_t)1 << 30))
        return fail(SE_ERR_UNSUPPORTED, "se_tiny_batch: an image of %d x %d x %d elements is not a small image", H, W, C);
    if (B == 0) return SE_OK;
    if (!images || !index || !affine || !flags || !mean || !stdp || !out) return fail(SE_ERR_INVALID, "se_tiny_batch: null pointer");
    const int64_t total = B * ((int64_t)H * W * C);
    const dim3 grid(row_blocks(total, TB_THREADS, SE_TINY_BATCH_MAX_BLOCKS));
    hipStream_t s = (hipStream_t)stream;
    const bool bf16 = out_dtype == SE_DTYPE_BF16;
    if (fill_mode == SE_FILL_NEAREST) tb_launch<SE_FILL_NEAREST>(bf16, grid, s, images, N, index, affine, flags, mean, stdp, cval, out, total, H, W, C);
    else if (fill_mode == SE_FILL_CONSTANT) tb_launch<SE_FILL_CONSTANT>(bf16, grid, s, images, N, index, affine, flags, mean, stdp, cval, out, total, H, W, C);
    else tb_launch<SE_FILL_REFLECT>(bf16, grid, s, images, N, index, affine, flags, mean, stdp, cval, out, total, H, W, C);
    SE_LAUNCH_CHECK();
    return SE_OK;
}
